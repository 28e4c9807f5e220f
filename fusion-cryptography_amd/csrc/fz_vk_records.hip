// fz_vk_records.hip -- verification keys derived straight from compact secret-key records: vk_records
// unpacks a chunk of one half of a key, range-checks it, transforms it, multiplies by A and accumulates, so that no int32 row of
// the key ever reaches memory, and stores the centred sums; its launcher.
#include "fz_records_dev.h"
#include "../../include/fusion_hip.h"

namespace {

// packed_load for a half that begins 8 mod 16 (degree 64 with l * wk odd: the right half of every key, and both halves of every
// other key): the same units of the same chunk, each read as its two 8-byte words, which ARE aligned.  A half is a multiple of 8
// bytes, so its last unit may be the low word alone; nothing past the half is read.
__device__ __forceinline__ Packed half_load8(const uint8_t *in, size_t task, size_t total_bytes, int w, int lane) {
    Packed c;
    const size_t base = task * 128 * (size_t)w;
    const size_t left = total_bytes - base;
    const unsigned cb = (unsigned)(left < (size_t)128 * w ? left : (size_t)128 * w);      // the chunk's bytes (uniform)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        c.u[j] = make_int4(0, 0, 0, 0);
        if (64u * 16u * j < cb) {
            const unsigned off = 16u * (64u * j + lane);
            if (off < cb) {
                const fz_v2i t = __builtin_nontemporal_load(reinterpret_cast<const fz_v2i *>(in + base + off));
                c.u[j].x = t.x;
                c.u[j].y = t.y;
            }
            if (off + 8 < cb) {
                const fz_v2i t = __builtin_nontemporal_load(reinterpret_cast<const fz_v2i *>(in + base + off + 8));
                c.u[j].z = t.x;
                c.u[j].w = t.y;
            }
        }
    }
    return c;
}

// vk[b][h] = cent(sum_k cent(FWD(s[b][h][k]) (.) A[k])) of unit g = blockIdx.x = 2 b + h, straight from the key's bytes: half h of
// key record b is l rows of wk-bit fields u = s + B that begin at byte g * half_bytes of the stream -- verify_encoded's record of
// l rows (fz_verify_encoded.hip) in its R == 1 form, with a store where the compare was.  A wave-task is one 1024-value chunk of
// the half, PPW whole rows; the workgroup's four waves take the chunks round-robin.  Pipeline, peeling, the steps from the packed
// chunk to the transform's outputs and the meeting of the sums in LDS are that kernel's, and so are its arguments: the range
// test is u <= 2B on integers the kernel holds anyway, slots of a tail chunk past row l - 1 read nothing and add nothing, a
// non-canonical field cannot fault (u - B is just an integer), A is any int32, and the fp64 sums of l canonical products are
// exact for l < 2^22 (the launcher refuses the rest).
// status[b] |= FZ_VERDICT_ENCODING where some field of the half is above 2B: one atomic per workgroup.  The other half's
// workgroup does not see the flag: the caller cleared the words before this launch and zeroes the refused keys' vk after it.
// A half begins on a multiple of 8 bytes (l * D / 8 * wk, D >= 64) and on 16 unless D = 64 and l * wk is odd: `split` (uniform)
// says which load reads this one.
// LDS: that of the transforms, not a word more (wave_lds; the range flags are the pad word of lane 0's sums in every wave's region).
template <int LOGD, bool FAST>
__global__ __launch_bounds__(64 * kWavesPerBlock) void vk_records(const uint8_t *in, const int32_t *__restrict__ A, unsigned rec_values,
                                                                  size_t half_bytes, int l, int w, int bound, int32_t *vk, int *status,
                                                                  const double2 *__restrict__ twB, const FzTwA *tab, FzMod m) {
    using G = Geom<LOGD>;
    constexpr int D = G::D, L = G::L, PPW = G::PPW, PS = G::PS, REGION = PPW * PS;
    static_assert(D <= 64 * kWavesPerBlock, "one thread per coefficient in the combine step");
    __shared__ __attribute__((aligned(16))) double lds[lds16_doubles<LOGD>()];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int p = lane / L, r = lane % L;
    const size_t g = blockIdx.x;
    in += g * half_bytes;
    const bool split = (reinterpret_cast<uintptr_t>(in) & 15) != 0;      // uniform
    const unsigned chunks = (rec_values + kChunk - 1) / kChunk;
    const unsigned first = wave, stride = kWavesPerBlock;
    const bool any = first < chunks;
    auto load = [&](unsigned c) __attribute__((always_inline)) {
        return split ? half_load8(in, c, half_bytes, w, lane) : packed_load(in, c, half_bytes, w, lane);
    };
    Packed raw0 = {};
    if (any) raw0 = load(first);                          // before the table: see fwd16_run
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
        const bool live = c * PPW + p < rows;             // the lane's polynomial is a row of the half
        int4 al[4];                                       // A[row][16r .. 16r + 15] (L2)
#pragma unroll
        for (int k = 0; k < 4; ++k) al[k] = make_int4(0, 0, 0, 0);
        if (live) {
#pragma unroll
            for (int k = 0; k < 4; ++k) al[k] = *reinterpret_cast<const int4 *>(arow + (size_t)c * kChunk + 4 * k);
        }
        Packed raw = {};
        if (more) raw = load(c + stride);
        wave_sync();
        uint32_t u[16];
        const uint32_t mx = fields_to_image(W.pk, W.stage, w, bnd, lane, u);
        // the lane's 16 fields are values c * 1024 + 16 lane .. of the half: past its end they are the zero units, not fields
        bad |= __ballot(mx > two_b && c * (unsigned)kChunk + 16u * lane < rv) != 0;       // wave-uniform
        wave_sync();
        double a[16];
        image_fwd16<LOGD, FAST>(W.stage, a, W.row, p, r, s_tw, tab, m);
        if (live) mulacc16(acc, a, al, m);
        if (more) packed_to_lds(W.pk, raw, w, lane);      // waits for the prefetched chunk (the passes are done with the region)
    };
    if (any) {
        packed_to_lds(W.pk, raw0, w, lane);
        unsigned c = first;
        for (; c + stride < chunks; c += stride) iteration(c, std::true_type());
        iteration(c, std::false_type());
    }
    // the 16 sums of every lane meet in LDS over the PPW slots and the four waves (sums_to_lds: coefficient i of slot q at
    // q * PS + pad16(i)); the pad behind lane 0's sums is the wave's range flag
    wave_sync();
    sums_to_lds(W.region, acc, lane);
    if (lane == 0) W.region[16] = bad ? 1.0 : 0.0;
    __syncthreads();
    if (threadIdx.x < D) {
        double sum = 0.0;
        for (int v = 0; v < kWavesPerBlock; ++v)
#pragma unroll
            for (int q = 0; q < PPW; ++q) sum += lds[v * REGION + q * PS + pad16((int)threadIdx.x)];
        vk[g * D + threadIdx.x] = (int)fz_cent_wide(sum, m);
    }
    if (threadIdx.x == 0) {
        bool wg_bad = false;
        for (int v = 0; v < kWavesPerBlock; ++v) wg_bad |= lds[v * REGION + 16] != 0.0;
        if (wg_bad) atomicOr(status + (g >> 1), FZ_VERDICT_ENCODING);
    }
}

}  // namespace

// fz_vk_records_async: a workgroup per (key, half) in one grid, as a fz_records_pass whose records are the keys' vk [2][degree]
// (status cleared, the launch, refused keys' vk zeroed: three stream-ordered steps, no allocation).  The grid comes from n alone:
// the caller holds 2 n within a grid's first dimension.
int fz_launch_vk_records(fz_ctx *ctx, const int32_t *A, const uint8_t *key_bytes, int wk, int64_t key_bound, size_t n, int l,
                         int32_t *d_vk, int *d_status) {
    // the fp64 sums of l canonical products, each below 2^31, are exact below 2^53
    if (l >= (1 << 22)) return fz_set_error(FZ_E_UNSUPPORTED, "l=%d too large for exact fp64 accumulation (< 2^22)", l);
    const unsigned rv = (unsigned)l * (unsigned)ctx->degree;
    const size_t half_bytes = fz_record_bytes(ctx->degree, l, wk);
    const auto launch = [&]() {
        return fz_dispatch<6, 8>(ctx, FZ_E_UNSUPPORTED, [&](auto logd, auto fast) {
            hipLaunchKernelGGL((vk_records<logd(), fast()>), dim3((unsigned)(2 * n)), dim3(64 * kWavesPerBlock), 0, ctx->stream, key_bytes, A,
                               rv, half_bytes, l, wk, (int)key_bound, d_vk, d_status, (const double2 *)ctx->d_twB,
                               (const FzTwA *)ctx->d_twAB, ctx->mod);
            return FZ_OK;
        });
    };
    return fz_records_pass(ctx, d_status, n, "vk_records launch", launch, d_vk, 2 * (size_t)ctx->degree * sizeof(int32_t));
}
