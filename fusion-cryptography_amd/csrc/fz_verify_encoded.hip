// fz_verify_encoded.hip -- signatures and aggregates verified straight from their compact byte encoding:
// verify_encoded unpacks a record's chunk, range-checks it, transforms it, multiplies by A and accumulates, so that no int32 row
// of the record ever reaches memory; verify_encoded_finish compares the sums of a record that several workgroups shared.
#include "fz_records_dev.h"
#include "../../include/fusion_hip.h"

namespace {

// one record's slot of the shared area (R > 1): D int64 sums, then one status word (64 bits wide: the slot stays 8-byte strided)
template <int D> constexpr size_t venc_slot_words() { return (size_t)D + 1; }

// the centred target of coefficient i of record g: formed from the key, cent(vkL (.) c + vkR) (the one-time scheme's equation,
// as in verify_fused), or the caller's word centred.  Any int32 key, challenge and word: |vkL * c| < 2^62 (fz_mulmod),
// |. + vkR| < 2^32 (fz_cent).
template <int D>
__device__ __forceinline__ int venc_want(const int32_t *target, const int32_t *vk, const int32_t *chal, size_t g, int i, const FzMod &m) {
    if (vk != nullptr) {
        const int32_t kL = vk[g * 2 * D + i], kR = vk[g * 2 * D + D + i], kc = chal[g * D + i];
        return (int)fz_cent(fz_mulmod((double)kL, (double)kc, m) + (double)kR, m);
    }
    return (int)fz_cent((double)target[g * D + i], m);
}

// verdict[g] of record g = blockIdx.y against its target, straight from the record's bytes.  The unpacked fields ARE
// cent(INTT(row)) + B, so of verify_fused's work the inverse transform, the norm scan and the centring are gone: the norm test
// is the canonicity test u <= 2B, a compare on integers the kernel holds anyway, and what is left per row is one forward
// transform and the multiply-accumulate with A.
//   FZ_VERDICT_ENCODING (6)         some field of the record is above 2B: the record has no defined value, so this comes first
//   FZ_VERDICT_TARGET_MISMATCH (3)  else, when sum_k NTT(z_k) (.) A_k differs from the target mod q
//   0                               else
// FZ_VERDICT_NORM (4) and FZ_VERDICT_WEIGHT (5) cannot occur: a canonical record is within B by construction, and the encoding
// never checked the weight (section G: omega_vf = d, a row cannot fail it).
// A wave-task is one 1024-value chunk of the record, PPW whole polynomials = rows chunk * PPW .. of the record; the gridDim.x = R
// workgroups of a record take its chunks round-robin by wave (chunk = 4 r + wave, stride 4 R).  Pipeline of records_decode:
// the wave's next chunk is requested before this one is unpacked, the last one is peeled off.  Lane (p, r) ends the passes with
// outputs 16r .. 16r + 15 of row chunk * PPW + p and multiplies them by A[row][16r ..] (four 16-byte loads, A is L2-resident
// and shared by all records).
// Exactness: every product is made canonical, |p| <= (q-1)/2 < 2^31, and a record adds l of them per coefficient: the fp64 sums
// (per lane, then over the PPW slots and the four waves in LDS) stay below 2^53 for l < 2^22; the launcher refuses larger l.
// A is any int32: the bounds of the product are mulacc16's (fz_records_dev.h).
// A non-canonical record cannot fault: u - B is just an integer (its low 32 bits), and nothing is indexed by it.
// Slots of a tail chunk past row l - 1 read no bytes (packed_load stops at the record's length), read no A, raise no range
// flag and are not accumulated.
// R == 1: the workgroup owns the record, compares and writes the verdict; no other workgroup is involved and `share` is not
// touched.  R > 1: the workgroup adds its D sums to the record's slot of `share` with 64-bit integer atomics (exact and
// commutative: the order of arrival cannot change a bit) and ORs its range flag into the slot's status word; the caller cleared
// the slots before this launch and runs verify_encoded_finish after it -- stream order is the only ordering relied upon.
// LDS: that of the transforms, not a word more (wave_lds: the packed chunk lies behind the int32 image in the wave's region;
// the workgroup's flags are the pad words of lane 0's sums in every wave's region, one range flag and one mismatch flag per
// wave, OR-ed by whoever reads them after a barrier).
template <int LOGD, bool FAST>
__global__ __launch_bounds__(64 * kWavesPerBlock) void verify_encoded(const uint8_t *in, const int32_t *__restrict__ A, unsigned rec_values,
                                                                      unsigned rec_bytes, int l, int w, int bound,
                                                                      const int32_t *__restrict__ target, const int32_t *__restrict__ vk,
                                                                      const int32_t *__restrict__ chal, unsigned long long *share,
                                                                      int *verdict, const double2 *__restrict__ twB, const FzTwA *tab, FzMod m) {
    using G = Geom<LOGD>;
    constexpr int D = G::D, L = G::L, PPW = G::PPW, PS = G::PS, REGION = PPW * PS;
    static_assert(D <= 64 * kWavesPerBlock, "one thread per coefficient in the combine step");
    __shared__ __attribute__((aligned(16))) double lds[lds16_doubles<LOGD>()];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int p = lane / L, r = lane % L;
    const unsigned R = gridDim.x;
    const size_t g = blockIdx.y;
    in += g * rec_bytes;
    const unsigned chunks = (rec_values + kChunk - 1) / kChunk;
    const unsigned first = blockIdx.x * kWavesPerBlock + wave, stride = R * kWavesPerBlock;
    const bool any = first < chunks;
    Packed raw0 = {};
    if (any) raw0 = packed_load(in, first, rec_bytes, w, lane);       // before the table and the target: see fwd16_run
    // R == 1: the three words (or the one) a comparing thread needs are requested right behind the first chunk, so the latencies
    // overlap; the centred target waits in ONE register across the row loop
    int want = 0;
    if (R == 1 && threadIdx.x < D) want = venc_want<D>(target, vk, chal, g, threadIdx.x, m);
    const double2 *s_tw = twiddles_to_lds<LOGD>(lds, twB);
    const WaveLds W = wave_lds<LOGD>(lds, wave, p);
    double acc[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[k] = 0.0;
    // what only the lanes' own address arithmetic uses: VALU operands, out of the scalar file (see RecWalk)
    const int32_t *arow = A + (size_t)p * D + 16 * r;
    unsigned bnd = (unsigned)bound, two_b = 2u * (unsigned)bound, rows = (unsigned)l, rv = rec_values;
    asm volatile("" : "+v"(arow), "+v"(bnd), "+v"(two_b), "+v"(rows), "+v"(rv));
    bool bad = false;

    auto iteration = [&](const unsigned c, auto more_tag) __attribute__((always_inline)) {       // pipeline and peeling: see fwd16_run
        constexpr bool more = decltype(more_tag)::value;
        const bool live = c * PPW + p < rows;             // the lane's polynomial is a row of the record
        int4 al[4];                                       // A[row][16r .. 16r + 15] (L2)
#pragma unroll
        for (int k = 0; k < 4; ++k) al[k] = make_int4(0, 0, 0, 0);
        if (live) {
#pragma unroll
            for (int k = 0; k < 4; ++k) al[k] = *reinterpret_cast<const int4 *>(arow + (size_t)c * kChunk + 4 * k);
        }
        Packed raw = {};
        if (more) raw = packed_load(in, c + stride, rec_bytes, w, lane);
        wave_sync();
        uint32_t u[16];
        const uint32_t mx = fields_to_image(W.pk, W.stage, w, bnd, lane, u);
        // the lane's 16 fields are values c * 1024 + 16 lane .. of the record: past its end they are the zero units, not fields
        bad |= __ballot(mx > two_b && c * (unsigned)kChunk + 16u * lane < rv) != 0;       // wave-uniform
        wave_sync();
        double a[16];
        image_fwd16<LOGD, FAST>(W.stage, a, W.row, p, r, s_tw, tab, m);
        // lane (p, r): outputs 16r .. 16r + 15 of row c * PPW + p by A[row][16r ..].  mulacc16's text, kept here: beside the other
        // helpers its call makes the compiler zero the 16 sums in another order in this kernel (docs/HISTORY.md section M)
        const int av[16] = {al[0].x, al[0].y, al[0].z, al[0].w, al[1].x, al[1].y, al[1].z, al[1].w,
                            al[2].x, al[2].y, al[2].z, al[2].w, al[3].x, al[3].y, al[3].z, al[3].w};
        if (live) {
#pragma unroll
            for (int k = 0; k < 16; ++k) acc[k] += fz_cent(fz_mulmod(a[k], (double)av[k], m), m);
        }
        if (more) packed_to_lds(W.pk, raw, w, lane);      // waits for the prefetched chunk (the passes are done with the region)
    };
    if (any) {
        packed_to_lds(W.pk, raw0, w, lane);
        unsigned c = first;
        for (; c + stride < chunks; c += stride) iteration(c, std::true_type());
        iteration(c, std::false_type());
    }
    // the 16 sums of every lane meet in LDS over the PPW slots and the four waves: lane's 16 at doubles 18 * lane .. of its wave's
    // region, i.e. coefficient i of slot q at q * PS + pad16(i)
    wave_sync();
    sums_to_lds(W.region, acc, lane);
    if (lane == 0) W.region[16] = bad ? 1.0 : 0.0;       // the pad behind lane 0's sums: the wave's range flag
    __syncthreads();
    double sum = 0.0;
    if (threadIdx.x < D) {
        for (int v = 0; v < kWavesPerBlock; ++v)
#pragma unroll
            for (int q = 0; q < PPW; ++q) sum += lds[v * REGION + q * PS + pad16((int)threadIdx.x)];
    }
    bool wg_bad = false;
    for (int v = 0; v < kWavesPerBlock; ++v) wg_bad |= lds[v * REGION + 16] != 0.0;
    if (R == 1) {                                         // the whole record is this workgroup's: nothing to share
        const bool miss = threadIdx.x < D && (int)fz_cent_wide(sum, m) != want;
        const bool wave_miss = __ballot(miss) != 0;
        if (lane == 0) W.region[17] = wave_miss ? 1.0 : 0.0;     // the other pad word: the wave's mismatch flag
        __syncthreads();
        if (threadIdx.x == 0) {
            bool wg_miss = false;
            for (int v = 0; v < kWavesPerBlock; ++v) wg_miss |= lds[v * REGION + 17] != 0.0;
            verdict[g] = wg_bad ? FZ_VERDICT_ENCODING : (wg_miss ? FZ_VERDICT_TARGET_MISMATCH : FZ_VERDICT_OK);
        }
        return;
    }
    unsigned long long *slot = share + g * venc_slot_words<D>();
    if (threadIdx.x < D) atomicAdd(slot + threadIdx.x, (unsigned long long)(long long)sum);
    if (threadIdx.x == 0 && wg_bad) atomicOr(slot + D, 1ull);
}

// R > 1: the verdicts of the records whose sums verify_encoded left in `share` (a workgroup per record, a thread per coefficient)
template <int LOGD>
__global__ __launch_bounds__(1 << LOGD) void verify_encoded_finish(const unsigned long long *share, const int32_t *__restrict__ target,
                                                                   const int32_t *__restrict__ vk, const int32_t *__restrict__ chal,
                                                                   int *verdict, FzMod m) {
    constexpr int D = 1 << LOGD;
    __shared__ int s_miss;
    const size_t g = blockIdx.x;
    const unsigned long long *slot = share + g * venc_slot_words<D>();
    if (threadIdx.x == 0) s_miss = 0;
    __syncthreads();
    // the sums are any int64 as far as this kernel knows: centred as such (fz_cent_i64)
    const int got = (int)fz_cent_i64((long long)slot[threadIdx.x], m);
    if (got != venc_want<D>(target, vk, chal, g, threadIdx.x, m)) atomicOr(&s_miss, 1);
    __syncthreads();
    if (threadIdx.x == 0)
        verdict[g] = slot[D] != 0 ? FZ_VERDICT_ENCODING : (s_miss ? FZ_VERDICT_TARGET_MISMATCH : FZ_VERDICT_OK);
}

}  // namespace

// the shared area of the launches with R > 1, a slot per record: R >= 2 means 2 * records <= 2 * num_cu, so num_cu slots (526 KB
// on 256 CUs at degree 256).  Allocated once per context, at its creation (degrees 64 / 256; nothing at the others).
int fz_verify_encoded_setup(fz_ctx *ctx) {
    if (ctx->logd != 6 && ctx->logd != 8) return FZ_OK;
    const size_t bytes = (size_t)ctx->num_cu * ((size_t)ctx->degree + 1) * sizeof(unsigned long long);
    const int rc = fz_check_hip(hipMalloc((void **)&ctx->d_venc, bytes), "verify_encoded area alloc");
    if (rc == FZ_OK) ctx->venc_bytes = bytes;
    else ctx->d_venc = nullptr;
    return rc;
}

// fz_verify_encoded_async: one launch per at most max-grid-y records (blockIdx.y is the record).  R workgroups per record by
// launch_verify_fused's rule: about one chunk per wave, capped by what fills the chip twice over, 2 * num_cu / N.  R == 1: the
// kernel writes the verdicts.  R > 1 (then N <= num_cu: one launch, and the context's shared area, ctx->d_venc, holds a slot per
// record): the slots are cleared on the stream, the kernel adds into them, the finish kernel compares.
int fz_launch_verify_encoded(fz_ctx *ctx, const int32_t *A, const uint8_t *bytes, size_t N, int l, int w, int64_t bound,
                             const int32_t *target, const int32_t *vk, const int32_t *chal, int *d_verdict) {
    // the fp64 sums of l canonical products, each below 2^31, are exact below 2^53
    if (l >= (1 << 22)) return fz_set_error(FZ_E_UNSUPPORTED, "l=%d too large for exact fp64 accumulation (< 2^22)", l);
    int ymax = 0;
    int rc = fz_check_hip(hipDeviceGetAttribute(&ymax, hipDeviceAttributeMaxGridDimY, ctx->device), "max grid y");
    if (rc != FZ_OK) return rc;
    if (ymax < 1) return fz_set_error(FZ_E_HIP, "max grid y reported as %d", ymax);
    const size_t D = (size_t)ctx->degree;
    const unsigned rv = (unsigned)l * (unsigned)D, rb = (unsigned)fz_record_bytes(ctx->degree, l, w);
    const size_t chunks = ((size_t)rv + kChunk - 1) / kChunk;
    size_t R = (chunks + kWavesPerBlock - 1) / kWavesPerBlock;
    const size_t fill = (size_t)ctx->num_cu * 2 / N;
    if (R > fill) R = fill;
    if (R < 1) R = 1;
    if (R > 64) R = 64;
    unsigned long long *share = ctx->d_venc;
    if (R > 1) {
        if (N * (D + 1) * sizeof(unsigned long long) > ctx->venc_bytes)
            return fz_set_error(FZ_E_HIP, "verify_encoded: %zu records do not fit the shared area", N);
        rc = fz_check_hip(hipMemsetAsync(share, 0, N * (D + 1) * sizeof(unsigned long long), ctx->stream), "verify_encoded area clear");
        if (rc != FZ_OK) return rc;
    }
    for (size_t g0 = 0; g0 < N; g0 += (size_t)ymax) {
        const size_t n = N - g0 < (size_t)ymax ? N - g0 : (size_t)ymax;
        const dim3 grid((unsigned)R, (unsigned)n), block(64 * kWavesPerBlock);
        rc = fz_dispatch<6, 8>(ctx, FZ_E_UNSUPPORTED, [&](auto logd, auto fast) {
            hipLaunchKernelGGL((verify_encoded<logd(), fast()>), grid, block, 0, ctx->stream, bytes + g0 * rb, A, rv, rb, l, w, (int)bound,
                               target ? target + g0 * D : nullptr, vk ? vk + g0 * 2 * D : nullptr, chal ? chal + g0 * D : nullptr, share,
                               d_verdict + g0, (const double2 *)ctx->d_twB, (const FzTwA *)ctx->d_twAB, ctx->mod);
            return FZ_OK;
        });
        if (rc == FZ_OK) rc = fz_check_hip(hipGetLastError(), "verify_encoded launch");
        if (rc != FZ_OK) return rc;
    }
    if (R == 1) return FZ_OK;
    rc = fz_dispatch<6, 8>(ctx, FZ_E_UNSUPPORTED, [&](auto logd, auto) {
        hipLaunchKernelGGL((verify_encoded_finish<logd()>), dim3((unsigned)N), dim3(1 << logd()), 0, ctx->stream,
                           (const unsigned long long *)share, target, vk, chal, d_verdict, ctx->mod);
        return FZ_OK;
    });
    return rc != FZ_OK ? rc : fz_check_hip(hipGetLastError(), "verify_encoded_finish launch");
}
