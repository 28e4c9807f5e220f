// fz_aggregate_encoded.hip -- signatures aggregated straight from their compact byte encoding:
// encoded_check, the range check of a byte stream without its transform, and aggregate_encoded, which unpacks a record's chunk,
// transforms it, multiplies by the signer's alpha_hat and accumulates, so that no int32 row of a signature ever reaches memory.
#include "fz_records_dev.h"
#include "../../include/fusion_hip.h"

namespace {

// the range check of records_decode alone: the byte stream's chunk walk, no transform and no output rows; status word of a
// record |= FZ_VERDICT_ENCODING where some field > 2B.  LDS: the packed chunk of each wave.
__global__ __launch_bounds__(64 * kWavesPerBlock) void encoded_check(const uint8_t *in, size_t total, unsigned rec_values, int w, int bound,
                                                                     int *status) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kWavesPerBlock * kPackBytes];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const size_t tasks = (total + kChunk - 1) / kChunk;
    const size_t total_bytes = total / 8 * (size_t)w;
    const size_t first = (size_t)blockIdx.x * kWavesPerBlock + wave;
    const size_t stride = (size_t)gridDim.x * kWavesPerBlock;
    if (first >= tasks) return;                           // (no workgroup-wide barrier in this kernel)
    uint8_t *pk = lds + wave * kPackBytes;
    packed_to_lds(pk, packed_load(in, first, total_bytes, w, lane), w, lane);
    RecWalk walk(first, stride, rec_values, lane);
    const uint32_t two_b = 2u * (unsigned)bound;

    auto iteration = [&](const size_t task, auto more_tag) __attribute__((always_inline)) {       // pipeline and peeling: see fwd16_run
        constexpr bool more = decltype(more_tag)::value;
        Packed raw = {};
        if (more) raw = packed_load(in, task + stride, total_bytes, w, lane);
        wave_sync();
        uint32_t u[16], mx = 0;
        fields_unpack(reinterpret_cast<const uint16_t *>(pk) + lane * w, u, w);
#pragma unroll
        for (int k = 0; k < 16; ++k) mx = max(mx, u[k]);
        wave_sync();
        if (more) packed_to_lds(pk, raw, w, lane);
        const bool valid = task * kChunk + 16 * lane < total;
        records_flag(status, walk.rec, mx > two_b && valid, FZ_VERDICT_ENCODING, lane);
        walk.step();
    };
    size_t task = first;
    for (; task + stride < tasks; task += stride) iteration(task, std::true_type());
    iteration(task, std::false_type());
}

// partial [rec_values] int64 += sum over the signers i of this workgroup's slice with skip[i] == 0 of
// cent(NTT(z_i) (.) alpha_hat_i), z_i = the fields of record i minus B; the caller zeroed `partial`.
// A wave-task is (signer i, chunk c of that signer's record): chunk c of every signer covers the same 1024 coefficients
// [1024c, 1024c + 1024) of the [l][d] aggregate, so a workgroup owns ONE chunk column (blockIdx.x) for one slice of the signers
// (blockIdx.y), its four waves take the slice's signers round-robin, each wave sums its products in 16 fp64 registers per lane
// (exact: every product is canonical, |p| <= (q-1)/2, and N < 2^22 of them stay below 2^53), the four waves' sums meet in LDS
// and the workgroup adds its 1024 integers to `partial` with 64-bit integer atomics (agent scope, executed at the memory side:
// integer addition is exact and commutative, so the order of arrival cannot change a bit of the result).
// Pipeline of records_decode: the next signer's packed chunk is in flight while the current one is transformed, the wave's last
// signer is peeled off.  A skipped signer's bytes are never read (one task is one record: the test is wave-uniform); whether
// the signer after next is skipped is asked for BEFORE the prefetch is issued, so the answer is older than the prefetch in the
// in-order memory counter and waiting for it does not wait for the prefetch.
// The lanes of a tail chunk past the record's end read nothing (packed_load stops at the record's length); what they compute from
// zero units stays in whole polynomials of their own and is never added to `partial`.
// LDS: that of the transforms (wave_lds: the packed chunk lies behind the int32 image in the wave's region).
template <int LOGD, bool FAST>
__global__ __launch_bounds__(64 * kWavesPerBlock) void aggregate_encoded(const uint8_t *in, const int32_t *__restrict__ alpha,
                                                                         const int *__restrict__ skip, unsigned n, unsigned rec_values,
                                                                         unsigned rec_bytes, int w, int bound, unsigned long long *partial,
                                                                         const double2 *__restrict__ twB, const FzTwA *tab, FzMod m) {
    using G = Geom<LOGD>;
    constexpr int D = G::D, L = G::L, REGION = G::PPW * G::PS;
    __shared__ __attribute__((aligned(16))) double lds[lds16_doubles<LOGD>()];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int p = lane / L, r = lane % L;
    const unsigned col = blockIdx.x;
    // the slice's signers [lo, hi): n / slices each, the first n % slices slices one more (slices <= n: none is empty; n < 2^22)
    const unsigned slices = gridDim.y, s = blockIdx.y, base = n / slices, extra = n % slices;
    const unsigned lo = s * base + (s < extra ? s : extra), hi = lo + base + (s < extra ? 1 : 0);
    // the wave's next signer at or after j that is not skipped (hi or more: none)
    auto next_ok = [&](unsigned j) __attribute__((always_inline)) {
        if (skip != nullptr)
            while (j < hi && skip[j] != 0) j += kWavesPerBlock;
        return j;
    };
    unsigned cur = next_ok(lo + wave);
    const bool any = cur < hi;
    Packed raw0 = {};
    if (any) raw0 = packed_load(in + (size_t)cur * rec_bytes, col, rec_bytes, w, lane);      // before the table: see fwd16_run
    const double2 *s_tw = twiddles_to_lds<LOGD>(lds, twB);
    const WaveLds W = wave_lds<LOGD>(lds, wave, p);
    double acc[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[k] = 0.0;
    // what only the lanes' own address arithmetic and the epilogue use: VALU operands, out of the scalar file (see RecWalk)
    const int32_t *arow = alpha + 16 * r;
    unsigned bnd = (unsigned)bound;
    const unsigned left = rec_values - col * (unsigned)kChunk;      // the column's coefficients: 1024, or the record's tail
    unsigned valid = left < (unsigned)kChunk ? left : (unsigned)kChunk;
    unsigned long long *dst = partial + (size_t)col * kChunk;
    asm volatile("" : "+v"(arow), "+v"(bnd), "+v"(valid), "+v"(dst));

    // one signer; MORE = another signer `nxt` of this wave follows (its chunk is requested first).  -> skip[nxt + 4] (0 past the slice)
    auto iteration = [&](const unsigned i, const unsigned nxt, auto more_tag) __attribute__((always_inline)) {
        constexpr bool more = decltype(more_tag)::value;
        int after = 0;
        if (more && skip != nullptr && nxt + kWavesPerBlock < hi) after = skip[nxt + kWavesPerBlock];
        int4 al[4];                                       // alpha_hat_i[16r .. 16r + 15]: the row is shared by the signer's chunks (L2)
#pragma unroll
        for (int k = 0; k < 4; ++k) al[k] = *reinterpret_cast<const int4 *>(arow + (size_t)i * D + 4 * k);
        Packed raw = {};
        if (more) raw = packed_load(in + (size_t)nxt * rec_bytes, col, rec_bytes, w, lane);
        wave_sync();
        uint32_t u[16];
        fields_to_image(W.pk, W.stage, w, bnd, lane, u);  // no range test here: the skip words carry its outcome
        wave_sync();
        double a[16];
        image_fwd16<LOGD, FAST>(W.stage, a, W.row, p, r, s_tw, tab, m);
        mulacc16(acc, a, al, m);                          // lane (p, r): outputs 16r .. 16r + 15 of polynomial p by alpha_hat_i[16r ..]
        if (more) packed_to_lds(W.pk, raw, w, lane);      // waits for the prefetched chunk (the passes are done with the region)
        return after;
    };
    if (any) {
        packed_to_lds(W.pk, raw0, w, lane);
        unsigned nxt = next_ok(cur + kWavesPerBlock);
        while (nxt < hi) {
            const int after = iteration(cur, nxt, std::true_type());
            cur = nxt;
            nxt = cur + kWavesPerBlock;
            if (after != 0) nxt = next_ok(nxt + kWavesPerBlock);
        }
        iteration(cur, cur, std::false_type());
    }
    // the four waves' sums meet in LDS: lane's 16 at doubles 18 * lane .. (element e = 16 * lane + k of the chunk at pad16(e))
    sums_to_lds(W.region, acc, lane);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kChunk / (64 * kWavesPerBlock); ++j) {
        const unsigned e = threadIdx.x + 64 * kWavesPerBlock * j;
        double sum = 0.0;
#pragma unroll
        for (int v = 0; v < kWavesPerBlock; ++v) sum += lds[v * REGION + pad16((int)e)];
        if (e < valid) atomicAdd(dst + e, (unsigned long long)(long long)sum);
    }
}

template <int LOGD, bool FAST>
int launch_aggregate_encoded(fz_ctx *ctx, const uint8_t *bytes, const int32_t *alpha, const int *skip, size_t n, unsigned rv, unsigned rb,
                             int w, int bound, int64_t *partial) {
    // columns x slices ~ the resident grid, and no more slices than give every wave of a workgroup a signer
    const size_t columns = (rv + kChunk - 1) / kChunk, per_wg = (n + kWavesPerBlock - 1) / kWavesPerBlock;
    size_t slices = (size_t)ctx->grid_aggenc / columns;
    slices = slices < 1 ? 1 : slices;
    slices = slices < per_wg ? slices : per_wg;
    slices = slices < 65535 ? slices : 65535;
    hipLaunchKernelGGL((aggregate_encoded<LOGD, FAST>), dim3((unsigned)columns, (unsigned)slices), dim3(64 * kWavesPerBlock), 0, ctx->stream,
                       bytes, alpha, skip, (unsigned)n, rv, rb, w, bound, (unsigned long long *)partial,
                       (const double2 *)ctx->d_twB, (const FzTwA *)ctx->d_twAB, ctx->mod);
    return FZ_OK;
}

}  // namespace

// resident grids of the two kernels this context launches (context creation; degrees 64 / 256, nothing to query at the others),
// then what the other consumer of the bytes needs from context creation (fz_verify_encoded.hip), as fz_ntt_query_grid goes on to
// fz_records_query_grid
int fz_aggregate_encoded_query_grid(fz_ctx *ctx) {
    const int rc = fz_dispatch<6, 8>(ctx, FZ_OK, [&](auto logd, auto fast) {
        const int rc = fz_resident_grid(ctx, aggregate_encoded<logd(), fast()>, 64 * kWavesPerBlock, "occupancy query (aggregate_encoded)",
                                        &ctx->grid_aggenc);
        return rc != FZ_OK ? rc : fz_resident_grid(ctx, encoded_check, 64 * kWavesPerBlock, "occupancy query (encoded_check)", &ctx->grid_check);
    });
    return rc != FZ_OK ? rc : fz_verify_encoded_setup(ctx);
}

// fz_check_records_async: d_status cleared, then the range check over the byte stream (asynchronous, allocation-free)
int fz_launch_check_records(fz_ctx *ctx, const uint8_t *bytes, size_t n, int rows, int w, int64_t bound, int *d_status) {
    const unsigned rv = (unsigned)rows * (unsigned)ctx->degree;
    const size_t total = n * rv;
    int rc = fz_check_hip(hipMemsetAsync(d_status, 0, n * sizeof(int), ctx->stream), "records status clear");
    if (rc != FZ_OK) return rc;
    const size_t tasks = (total + kChunk - 1) / kChunk, blocks = (tasks + kWavesPerBlock - 1) / kWavesPerBlock;
    const size_t cap = (size_t)ctx->grid_check;
    hipLaunchKernelGGL(encoded_check, dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(64 * kWavesPerBlock), 0, ctx->stream, bytes, total,
                       rv, w, (int)bound, d_status);
    return fz_check_hip(hipGetLastError(), "encoded_check launch");
}

// fz_aggregate_encoded_async: d_partial zeroed, the fused pass, then cent() of the sums when the caller wants int32
// (fz_reduce_i64's kernel).  Record lengths are multiples of 16 bytes here (the entry checks it): every signer's chunks start
// 16-byte aligned.
int fz_launch_aggregate_encoded(fz_ctx *ctx, const uint8_t *bytes, const int32_t *alpha, const int *skip, size_t n, int l, int w,
                                int64_t bound, int64_t *d_partial, int32_t *d_out) {
    const unsigned rv = (unsigned)l * (unsigned)ctx->degree, rb = (unsigned)fz_record_bytes(ctx->degree, l, w);
    int rc = fz_check_hip(hipMemsetAsync(d_partial, 0, (size_t)rv * sizeof(int64_t), ctx->stream), "aggregate partial clear");
    if (rc != FZ_OK) return rc;
    rc = fz_dispatch<6, 8>(ctx, FZ_E_UNSUPPORTED, [&](auto logd, auto fast) {
        return launch_aggregate_encoded<logd(), fast()>(ctx, bytes, alpha, skip, n, rv, rb, w, (int)bound, d_partial);
    });
    if (rc == FZ_OK) rc = fz_check_hip(hipGetLastError(), "aggregate_encoded launch");
    if (rc != FZ_OK || d_out == nullptr) return rc;
    return fz_launch_reduce_i64(ctx, d_partial, d_out, rv);
}
