// fz_aggregate_encoded.hip -- signatures aggregated straight from their compact byte encoding:
// encoded_check, the range check of a byte stream without its transform, and aggregate_encoded, which unpacks a record's chunk,
// transforms it, multiplies by the signer's alpha_hat and accumulates, so that no int32 row of a signature ever reaches memory.
#include "fz_aggregate_encoded_dev.h"
#include "../../include/fusion_hip.h"

namespace {

// the range check of records_decode alone: the byte stream's chunk walk, no transform and no output rows; status word of a
// record |= FZ_VERDICT_ENCODING where some field > 2B.  LDS: the packed chunk of each wave.
__global__ __launch_bounds__(64 * kWavesPerBlock) void encoded_check(const uint8_t *in, size_t total, unsigned rec_values, int w, int bound,
                                                                     int *status) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kWavesPerBlock * kPackBytes];
    const int lane = threadIdx.x & 63;
    const ChunkTasks T(total);
    const size_t total_bytes = total / 8 * (size_t)w;
    if (T.first >= T.tasks) return;                       // (no workgroup-wide barrier in this kernel)
    uint8_t *pk = lds + T.wave * kPackBytes;
    packed_to_lds(pk, packed_load(in, T.first, total_bytes, w, lane), w, lane);
    RecWalk walk(T.first, T.stride, rec_values, lane);
    const uint32_t two_b = 2u * (unsigned)bound;

    auto iteration = [&](const size_t task, auto more_tag) __attribute__((always_inline)) {       // pipeline and peeling: see fwd16_run
        constexpr bool more = decltype(more_tag)::value;
        Packed raw = {};
        if (more) raw = packed_load(in, task + T.stride, total_bytes, w, lane);
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
    size_t task = T.first;
    for (; task + T.stride < T.tasks; task += T.stride) iteration(task, std::true_type());
    iteration(task, std::false_type());
}

// partial [rec_values] int64 += sum over the signers i with skip[i] == 0 of cent(NTT(z_i) (.) alpha_hat_i), z_i = the fields of
// record i minus B; the caller zeroed `partial`.  A workgroup owns ONE chunk column (blockIdx.x) for one slice of the signers
// (blockIdx.y): the whole array is one group of aggregate_encoded_slice (fz_aggregate_encoded_dev.h), where the walk over a slice,
// its pipeline and the epilogue are written.
// LDS: that of the transforms.
template <int LOGD, bool FAST>
__global__ __launch_bounds__(64 * kWavesPerBlock) void aggregate_encoded(const uint8_t *in, const int32_t *__restrict__ alpha,
                                                                         const int *__restrict__ skip, unsigned n, unsigned rec_values,
                                                                         unsigned rec_bytes, int w, int bound, unsigned long long *partial,
                                                                         const double2 *__restrict__ twB, const FzTwA *tab, FzMod m) {
    __shared__ __attribute__((aligned(16))) double lds[lds16_doubles<LOGD>()];
    // the slice's signers [lo, hi): n / slices each, the first n % slices slices one more (slices <= n: none is empty; n < 2^22)
    const unsigned slices = gridDim.y, s = blockIdx.y, base = n / slices, extra = n % slices;
    const unsigned lo = s * base + (s < extra ? s : extra), hi = lo + base + (s < extra ? 1 : 0);
    aggregate_encoded_slice<LOGD, FAST>(lds, in, alpha, skip, lo, hi, blockIdx.x, rec_values, rec_bytes, w, bound, partial, twB, tab, m);
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

// resident grids of the two kernels this context launches (context creation; degrees 64 / 256, nothing to query at the others)
int fz_aggregate_encoded_query_grid(fz_ctx *ctx) {
    return fz_dispatch<6, 8>(ctx, FZ_OK, [&](auto logd, auto fast) {
        const int rc = fz_resident_grid(ctx, aggregate_encoded<logd(), fast()>, 64 * kWavesPerBlock, "occupancy query (aggregate_encoded)",
                                        &ctx->grid_aggenc);
        return rc != FZ_OK ? rc : fz_resident_grid(ctx, encoded_check, 64 * kWavesPerBlock, "occupancy query (encoded_check)", &ctx->grid_check);
    });
}

// fz_check_records_async: d_status cleared, then the range check over the byte stream (asynchronous, allocation-free)
int fz_launch_check_records(fz_ctx *ctx, const uint8_t *bytes, size_t n, int rows, int w, int64_t bound, int *d_status) {
    const unsigned rv = (unsigned)rows * (unsigned)ctx->degree;
    const size_t total = n * rv;
    int rc = fz_check_hip(hipMemsetAsync(d_status, 0, n * sizeof(int), ctx->stream), "records status clear");
    if (rc != FZ_OK) return rc;
    hipLaunchKernelGGL(encoded_check, chunk_grid(total, ctx->grid_check), dim3(64 * kWavesPerBlock), 0, ctx->stream, bytes, total, rv, w,
                       (int)bound, d_status);
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
