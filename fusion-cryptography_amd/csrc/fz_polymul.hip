// fz_polymul.hip -- the negacyclic product INTT(NTT(f) * NTT(g)) in one launch, in its radix-4 form (polymul_fused) and on the
// 16-per-lane transforms (polymul16); the passes of both are fz_ntt_dev.h's.
#include "fz_ntt_dev.h"
#include "../../include/fusion_hip.h"

namespace {
// ------------------------------------------------------------------------------------------
// Negacyclic product INTT(NTT(f) * NTT(g)) in one launch (algebra/ntt.py:380-484 ntt_poly_mult; the product the
// reference's schoolbook PolynomialCoefficientRepresentation.__mul__, polynomials.py:171-216, is tested against):
// both forward transforms, the pointwise product and the inverse stay in registers / LDS; HBM sees 12*D bytes per
// product (f, g in; f*g out) instead of the 36*D of three transform launches plus a pointwise one.  Radix-4 layout:
// the forward passes leave a lane's values at bit-reversed positions 4mm..4mm+3, exactly where the inverse picks up.
// `out` may alias `f` or `g` (a wave has read its whole polynomials before it writes).
// ------------------------------------------------------------------------------------------
template <int LOGD, bool FAST>
__global__ __launch_bounds__(64 * kWavesPerBlock) void polymul_fused(const int32_t *f, const int32_t *g, int32_t *out, size_t batch,
                                                                     const double2 *__restrict__ tw2,
                                                                     const double2 *__restrict__ itw2, FzTwA twA, FzTwA itwA,
                                                                     FzMod m) {
    using TW = double2;
    constexpr int D = 1 << LOGD, LP = D / 4, PPW = 64 / LP, P = LOGD / 2;
    static_assert(LOGD % 2 == 0 && LOGD >= 6 && LOGD <= 8, "radix-4 kernel: degree 64 or 256");
    __shared__ __attribute__((aligned(16))) double lds[kWavesPerBlock * 256];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;      // the wave index is uniform: say so (scalar address arithmetic)
    const int p = lane / LP, mm = lane % LP;
    double *region = lds + wave * 256 + p * D;
    const size_t tasks = (batch + PPW - 1) / PPW;
    const size_t first = (size_t)blockIdx.x * kWavesPerBlock + wave, stride = (size_t)gridDim.x * kWavesPerBlock;
    if (first >= tasks) return;

    TW twf[P - 1][3], twi[P - 1][3];
    fwd4_load_twiddles<LOGD, TW>(twf, tw2, mm);
    inv4_load_twiddles<LOGD, TW>(twi, itw2, mm);

    for (size_t task = first; task < tasks; task += stride) {
        const size_t poly = task * PPW + p;
        const bool valid = poly < batch;
        const size_t row = (valid ? poly : batch - 1) * D + mm;
        int xf[4], xg[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) xf[k] = f[row + k * LP];
#pragma unroll
        for (int k = 0; k < 4; ++k) xg[k] = g[row + k * LP];
        double a[4], b[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k] = (double)xf[k];
        fwd4_passes_n<LOGD, FAST, 1, TW>(reinterpret_cast<double (&)[1][4]>(a), region, twf, twA, m, mm);
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k] = fz_cent(a[k], m);         // one centred factor keeps the product below 2^66
        wave_sync();                                                 // g's first-pass writes vs f's last-pass reads
#pragma unroll
        for (int k = 0; k < 4; ++k) b[k] = (double)xg[k];
        fwd4_passes_n<LOGD, FAST, 1, TW>(reinterpret_cast<double (&)[1][4]>(b), region, twf, twA, m, mm);
#pragma unroll
        for (int k = 0; k < 4; ++k) b[k] = fz_mulmod(a[k], b[k], m);
        wave_sync();
        inv4_passes_n<LOGD, FAST, 1, TW>(reinterpret_cast<double (&)[1][4]>(b), region, twi, itwA, m, mm);
        if (valid) {
            int32_t *dst = out + poly * D + mm;
#pragma unroll
            for (int k = 0; k < 4; ++k) __builtin_nontemporal_store((int)fz_cent(b[k], m), dst + k * LP);
        }
        wave_sync();      // the next product's first-pass writes must not overtake this one's last reads
    }
}

// ------------------------------------------------------------------------------------------
// The same product on the 16-per-lane transforms (32 <= D <= 256): ONE exchange through LDS per transform instead of the three
// of the radix-4 passes (polymul_fused above spends half its LDS pipe and a fifth of its cycles waiting on them,
// profiles/r06_shape_ceilings.txt), global traffic as 16 bytes per lane like ntt_fwd16 / ntt_inv16.  For batches that give
// every SIMD a few of these 128-register waves; smaller ones stay with the radix-4 kernel (fz_launch_polymul_fused chooses).
// A wave-task is one 4 KiB chunk of f, of g and of the product (PPW polynomials).  Pipeline: f's next chunk is requested at
// the top of an iteration and g's next chunk once g's current image has left the registers, so at most two chunks are held
// in registers; f waits in the staging image, g in registers; the stores are the youngest operations (see fwd16_run).
// `out` may alias `f` or `g`: a wave reads chunk t of both before it writes chunk t, and no other wave touches chunk t.
// ------------------------------------------------------------------------------------------
template <int LOGD> constexpr int lds_pm16_doubles() {
    using G = Geom<LOGD>;
    return kWavesPerBlock * G::PPW * G::PS + 4 * G::NE * G::L;      // a transpose region per wave + both per-lane twiddle tables
}

template <int LOGD, bool FAST>
__global__ __launch_bounds__(64 * kWavesPerBlock, 3) void polymul16(const int32_t *f, const int32_t *g, int32_t *out, size_t batch,
                                                                 const double2 *__restrict__ twB, const double2 *__restrict__ itwB,
                                                                 const FzTwA *tabs, FzMod m) {
    using G = Geom<LOGD>;
    constexpr int D = G::D, L = G::L, PPW = G::PPW, NE = G::NE, PS = G::PS;
    constexpr int REGION = PPW * PS;
    // The wave-uniform tables of both directions are 2 x 60 scalar registers where 102 exist: as kernel arguments they are loaded
    // once and then spilled into vector lanes (180 v_readlane per iteration).  They are read from constant memory instead, each
    // direction where it is used: the empty asm makes the pointer opaque, so the loads cannot be hoisted back out of the loop.
    typedef const __attribute__((address_space(4))) FzTwA *TabPtr;
    __shared__ __attribute__((aligned(16))) double lds[lds_pm16_doubles<LOGD>()];
    double2 *s_tw = reinterpret_cast<double2 *>(lds + kWavesPerBlock * REGION), *s_itw = s_tw + NE * L;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int p = lane / L, r = lane % L;
    const size_t total = batch * D;
    const size_t tasks = (total + kChunk - 1) / kChunk;
    const size_t first = (size_t)blockIdx.x * kWavesPerBlock + wave;
    const size_t stride = (size_t)gridDim.x * kWavesPerBlock;
    Chunk rawF = {}, rawG = {};
    if (first < tasks) {                                  // before the tables: see fwd16_run
        rawF = chunk_load(f, first, total, lane);
        rawG = chunk_load(g, first, total, lane);
    }
    for (int i = threadIdx.x; i < NE * L; i += 64 * kWavesPerBlock) {
        s_tw[i] = twB[i];
        s_itw[i] = itwB[i];
    }
    __syncthreads();                                      // the only workgroup-wide barrier
    double *region = lds + wave * REGION;
    int32_t *stage = reinterpret_cast<int32_t *>(region);
    double *row = region + p * PS;
    if (first >= tasks) return;
    chunk_to_lds(stage, lane, rawF);

    // element r + L*k of the lane's polynomial in the staging image: pad4(p * D + r + L * k) = pad4(p * D) + r + pad4(L * k), because
    // r < L and L divides 16 -- one address register and sixteen constant offsets instead of sixteen registers
    int32_t *strided = stage + pad4(p * D) + r;
    auto strided_from_stage = [&](double (&a)[16]) __attribute__((always_inline)) {
        int x[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) x[k] = strided[pad4(L * k)];
#pragma unroll
        for (int k = 0; k < 16; ++k) a[k] = (double)x[k];
    };
    auto iteration = [&](const size_t task, auto more_tag) __attribute__((always_inline)) {       // peeling: see fwd16_run
        constexpr bool more = decltype(more_tag)::value;
        if (more) rawF = chunk_load(f, task + stride, total, lane);
        wave_sync();
        double b[16];
        int fa[16];                                       // NTT(f), centred: 16 registers while g is transformed, not 32
        TabPtr tf = (TabPtr)tabs;
        asm volatile("" : "+s"(tf));
        strided_from_stage(b);
        wave_sync();
        fwd16_passes<LOGD, FAST>(b, row, r, s_tw, tf[0], m);
#pragma unroll
        for (int k = 0; k < 16; ++k) fa[k] = (int)fz_cent(b[k], m);
        chunk_to_lds(stage, lane, rawG);                               // waits for g's chunk; f's next one is younger
        if (more) rawG = chunk_load(g, task + stride, total, lane);
        wave_sync();
        strided_from_stage(b);
        wave_sync();
        fwd16_passes<LOGD, FAST>(b, row, r, s_tw, tf[0], m);
        TabPtr ti = (TabPtr)tabs + 1;
        asm volatile("" : "+s"(ti));
#pragma unroll
        for (int k = 0; k < 16; ++k) b[k] = fz_mulmod(b[k], (double)fa[k], m);      // |b * fa| < 2^69; |result| <= q/2 + 1: an input the inverse accepts
        inv16_passes<LOGD, FAST>(b, row, r, s_itw, ti[0], m);
#pragma unroll
        for (int k = 0; k < 16; ++k) strided[pad4(L * k)] = (int)fz_cent(b[k], m);
        wave_sync();
        const int4 o0 = *reinterpret_cast<const int4 *>(stage + pad4(4 * lane));
        const int4 o1 = *reinterpret_cast<const int4 *>(stage + pad4(256 + 4 * lane));
        const int4 o2 = *reinterpret_cast<const int4 *>(stage + pad4(512 + 4 * lane));
        const int4 o3 = *reinterpret_cast<const int4 *>(stage + pad4(768 + 4 * lane));
        wave_sync();
        if (more) chunk_to_lds(stage, lane, rawF);        // waits for f's next chunk; g's next one and the stores are younger
        chunk_store(out, task, total, lane, o0, o1, o2, o3);
    };
    size_t task = first;
    for (; task + stride < tasks; task += stride) iteration(task, std::true_type());
    iteration(task, std::false_type());
}

}  // namespace

// the 16-per-lane form of the fused product (degrees 32..256, 16-byte aligned operands)
template <int LOGD, bool FAST>
static int launch_polymul16(fz_ctx *ctx, const int32_t *f, const int32_t *g, int32_t *out, size_t batch) {
    if (ctx->grid_pm16 == 0) {
        const int rc = fz_resident_grid(ctx, polymul16<LOGD, FAST>, 64 * kWavesPerBlock, "occupancy query (polymul16)", &ctx->grid_pm16);
        if (rc != FZ_OK) return rc;
    }
    const size_t tasks = (batch * (size_t)ctx->degree + kChunk - 1) / kChunk, blocks = (tasks + kWavesPerBlock - 1) / kWavesPerBlock;
    const dim3 grid((unsigned)(blocks < (size_t)ctx->grid_pm16 ? blocks : (size_t)ctx->grid_pm16)), block(64 * kWavesPerBlock);
    hipLaunchKernelGGL((polymul16<LOGD, FAST>), grid, block, 0, ctx->stream, f, g, out, batch, (const double2 *)ctx->d_twB,
                       (const double2 *)ctx->d_itwB, (const FzTwA *)ctx->d_twAB, ctx->mod);
    return fz_check_hip(hipGetLastError(), "polymul16 launch");
}

// Which form (tools/probes/polymul_crossover.py, profiles/r06_polymul_crossover.txt): at degree 256 the 16-per-lane kernel from
// 2^14 products on (18.2 against 19.3 us there, 118 against 130 us at 2^17: 42.6 % of 8 TB/s against 38.8 %; below, its start-up
// -- a table twice the size, two chunks per wave before the first butterfly -- costs more than the exchanges it saves); at
// degree 64 the radix-4 kernel at every size (three passes instead of four: 45.5 % at 2^17 products against 44.7 %); degrees
// 32 and 128 have no radix-4 form.  FZ_POLYMUL_FORM = 1 | 2 forces one.
constexpr size_t kPolymul16MinRows256 = (size_t)1 << 14;

bool fz_polymul16_ok(const fz_ctx *ctx, const int32_t *f, const int32_t *g, const int32_t *out, size_t batch) {
    if (ctx->logd < 5 || ctx->logd > 8 || ctx->knob_polymul_form == 1) return false;
    if ((((uintptr_t)f | (uintptr_t)g | (uintptr_t)out) & 15) != 0) return false;
    if (ctx->logd == 5 || ctx->logd == 7 || ctx->knob_polymul_form == 2) return true;
    return ctx->logd == 8 && batch >= kPolymul16MinRows256;
}

// fused product: degrees 64 / 256 in either form, 32 / 128 in the 16-per-lane form; the caller composes the generic path otherwise
int fz_launch_polymul_fused(fz_ctx *ctx, const int32_t *f, const int32_t *g, int32_t *out, size_t batch) {
    if (batch == 0) return FZ_OK;
    if (fz_polymul16_ok(ctx, f, g, out, batch))
        return fz_dispatch<5, 6, 7, 8>(ctx, FZ_E_UNSUPPORTED, [&](auto logd, auto fast) { return launch_polymul16<logd(), fast()>(ctx, f, g, out, batch); });
    if (ctx->logd != 6 && ctx->logd != 8) return fz_set_error(FZ_E_UNSUPPORTED, "fused product: degree 64 or 256, or 16-byte aligned operands of degree 32..256");
    return fz_dispatch<6, 8>(ctx, FZ_E_UNSUPPORTED, [&](auto logd, auto fast) {
        auto kernel = polymul_fused<logd(), fast()>;
        const int ppw = 64 / (ctx->degree / 4);
        const size_t tasks = (batch + ppw - 1) / ppw, blocks = (tasks + kWavesPerBlock - 1) / kWavesPerBlock;
        if (ctx->grid_pm == 0) {
            const int rc = fz_resident_grid(ctx, kernel, 64 * kWavesPerBlock, "occupancy query (polymul)", &ctx->grid_pm);
            if (rc != FZ_OK) return rc;
        }
        const dim3 grid((unsigned)(blocks < (size_t)ctx->grid_pm ? blocks : (size_t)ctx->grid_pm)), block(64 * kWavesPerBlock);
        hipLaunchKernelGGL(kernel, grid, block, 0, ctx->stream, f, g, out, batch, (const double2 *)ctx->d_tw2, (const double2 *)ctx->d_itw2,
                           ctx->twA, ctx->itwA, ctx->mod);
        return fz_check_hip(hipGetLastError(), "polymul_fused launch");
    });
}
