// fz_aggregate_target_encoded.hip -- many committees' aggregates AND verification targets straight from the signatures' compact byte
// encoding in one launch ("Aggregate and verify in one pass"): aggregate_target_encoded_ragged, the grid
// of aggregate_encoded_ragged (fz_aggregate_many_encoded.hip) with one more block column, whose workgroups form the targets' int64
// partial sums as the int32-row kernels do (agg_target4, fz_stream_dev.h).  What an aggregator that checks its own output needs
// for fz_verify_partials_batch_async, without a second clear and a second launch.
#include "fz_aggregate_encoded_dev.h"
#include "fz_stream_dev.h"
#include "../../include/fusion_hip.h"

namespace {

// aggregate_encoded_ragged's opening, here for both kinds of column (that kernel keeps its text: behind these two its code comes
// out with two operands exchanged).  The slice blockIdx.y of group blockIdx.z: signers [lo, hi) of the concatenated arrays.  The slice count is the launch's, not the
// group's: slice s of group g holds rag.base[g] signers, the first rag.extra[g] slices one more, and a group of fewer signers than
// slices leaves the slices behind its last signer empty (lo == hi).
__device__ __forceinline__ void ragged_slice(const FzRagged &rag, unsigned &lo, unsigned &hi) {
    const unsigned g = blockIdx.z, s = blockIdx.y, base = rag.base[g], extra = rag.extra[g];
    lo = rag.off[g] + s * base + (s < extra ? s : extra);
    hi = lo + base + (s < extra ? 1 : 0);
}

// is any signer of [lo, hi) summed (skip NULL: all are)?  Every wave of the workgroup reads the slice's skip words alike, 64 per
// round and none at or past hi, so the answer is the workgroup's.
__device__ __forceinline__ bool slice_live(const int *__restrict__ skip, unsigned lo, unsigned hi) {
    if (skip == nullptr) return true;
    const unsigned lane = threadIdx.x & 63;
    bool live = false;
    for (unsigned j = lo; j < hi && !live; j += 64) live = __ballot(j + lane < hi && skip[j + lane] == 0) != 0;
    return live;
}

// tpartial [D] int64 += sum over the signers i in [lo, hi) with skip[i] == 0 of (vkL_i (.) c_i + vkR_i) (.) alpha_i, the term of
// agg_target4 per coefficient; the caller zeroed `tpartial`.  vk [N][2][D] is read in place: L_i at vk + 2 i D, R_i a row behind.
// A thread owns one int4 column of the target for every (256 / (D / 4))-th signer of the slice: a wave is one signer's row at
// degree 256 and four signers' rows at degree 64, every load is 16 bytes and a wave's loads of one array are contiguous.  A
// skipped signer's rows are not read (the test is the lane's own: nothing here is collective before the barrier).  The sums are
// exact in fp64 (every term is within 2^18 of q/2, fewer than 2^22 of them stay below 2^53), the threads' sums meet in LDS, and the
// workgroup adds its D integers with 64-bit integer atomics, as aggregate_encoded_slice does for its column.
// `lds`: at least 1024 doubles.  One workgroup barrier inside: every wave of the workgroup calls this, with the same arguments.
template <int LOGD>
__device__ __forceinline__ void target_slice(double *lds, const int32_t *__restrict__ vk, const int32_t *__restrict__ chal,
                                             const int32_t *__restrict__ alpha, const int *__restrict__ skip, const unsigned lo,
                                             const unsigned hi, unsigned long long *tpartial, const FzMod &m) {
    constexpr int D = 1 << LOGD, D4 = D / 4, STEP = 64 * kWavesPerBlock / D4;      // STEP signers per round of the workgroup
    static_assert(64 * kWavesPerBlock * 4 <= lds16_doubles<LOGD>(), "a thread's four sums fit the transforms' LDS");
    const unsigned col = threadIdx.x % D4, sub = threadIdx.x / D4;
    const int4 *vk4 = reinterpret_cast<const int4 *>(vk) + col;
    const int4 *c4 = reinterpret_cast<const int4 *>(chal) + col, *a4 = reinterpret_cast<const int4 *>(alpha) + col;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 2
    for (unsigned i = lo + sub; i < hi; i += STEP) {
        if (skip != nullptr && skip[i] != 0) continue;
        const size_t o = (size_t)i * D4;
        agg_target4(vk4[2 * o], vk4[2 * o + D4], c4[o], a4[o], acc, m);
    }
    // thread (sub, col): coefficients 4 col .. 4 col + 3 of row `sub`
    *reinterpret_cast<double2 *>(lds + 4 * threadIdx.x) = make_double2(acc[0], acc[1]);
    *reinterpret_cast<double2 *>(lds + 4 * threadIdx.x + 2) = make_double2(acc[2], acc[3]);
    __syncthreads();
    if (threadIdx.x < D) {
        double sum = 0.0;
#pragma unroll
        for (int v = 0; v < STEP; ++v) sum += lds[v * D + threadIdx.x];
        atomicAdd(tpartial + threadIdx.x, (unsigned long long)(long long)sum);
    }
}

// Grid (chunk columns + 1, slices, groups).  Workgroups of the first gridDim.x - 1 columns, the record's chunks, are aggregate_encoded_ragged's, their
// code aggregate_encoded_slice: partial + g * pstride [rec_values] int64 += the aggregate's sums of their (column, slice, group).
// Workgroups of the last column: tpartial + g * tstride [degree] int64 += the target's sums of their (slice, group) from vk
// [N][2][degree] and chal [N][degree] (target_slice).  The caller zeroed the partials of both kinds.  The slices, the group table
// and the early exits -- an empty slice, a slice whose every signer is skipped: the workgroup leaves as a whole before its first
// barrier and writes nothing -- are aggregate_encoded_ragged's (ragged_slice, slice_live), the same for both kinds of column: a
// skipped signer contributes to neither sum.
// LDS: that of the transforms.  Registers and LDS stay within aggregate_encoded_ragged's of the same (LOGD, FAST), which is what
// lets the launcher size the grid by that kernel's resident grid (tests/test_aggregate_target_encoded_host.py holds it to that).
template <int LOGD, bool FAST>
__global__ __launch_bounds__(64 * kWavesPerBlock) void aggregate_target_encoded_ragged(
    const uint8_t *in, const int32_t *__restrict__ alpha, const int *__restrict__ skip, const FzRagged rag, unsigned rec_values,
    unsigned rec_bytes, int w, int bound, unsigned long long *partial, size_t pstride, const double2 *__restrict__ twB, const FzTwA *tab,
    FzMod m, const int32_t *__restrict__ vk, const int32_t *__restrict__ chal, unsigned long long *tpartial, size_t tstride) {
    __shared__ __attribute__((aligned(16))) double lds[lds16_doubles<LOGD>()];
    unsigned lo, hi;
    ragged_slice(rag, lo, hi);
    if (lo >= hi || !slice_live(skip, lo, hi)) return;
    if (blockIdx.x * (unsigned)kChunk >= rec_values) {    // the column behind the record's last chunk
        target_slice<LOGD>(lds, vk, chal, alpha, skip, lo, hi, tpartial + (size_t)blockIdx.z * tstride, m);
        return;
    }
    aggregate_encoded_slice<LOGD, FAST>(lds, in, alpha, skip, lo, hi, blockIdx.x, rec_values, rec_bytes, w, bound,
                                        partial + (size_t)blockIdx.z * pstride, twB, tab, m);
}

// the launch of groups [0, groups) of h_offsets (at most kFzRaggedMax).  The slice count is launch_aggregate_encoded_ragged's
// policy (ragged_slices) on the resident grid of aggregate_encoded_ragged -- this kernel's allocation is no larger, so it is
// resident as often -- with the target's column counted among the columns: short as its workgroups are, each holds a place of the
// resident grid while it runs.  Counted without it, one group of 1024 signers at secpar 256 is 24 slices x 21 columns = 504
// workgroups, the 24 of the target make 528 of 512, and the sixteen that wait for a place cost 23 us of 61 (DESIGN.md section
// 5.20); with it, 23 slices x 22 = 506.
template <int LOGD, bool FAST>
int launch_aggregate_target_encoded_ragged(fz_ctx *ctx, const uint8_t *bytes, const int32_t *alpha, const int *skip, const int32_t *vk,
                                           const int32_t *chal, const size_t *h_offsets, size_t groups, unsigned rv, unsigned rb, int w,
                                           int bound, int64_t *partial, size_t pstride, int64_t *tpartial, size_t tstride) {
    FzRagged rag;
    const size_t columns = (rv + kChunk - 1) / kChunk;
    const size_t slices = ragged_slices((size_t)ctx->grid_aggenc_rag, columns + 1, h_offsets, groups, rag);
    if (slices == 0) return FZ_OK;                        // nobody adds to these partials: they stay as the entry cleared them
    hipLaunchKernelGGL((aggregate_target_encoded_ragged<LOGD, FAST>), dim3((unsigned)columns + 1, (unsigned)slices, (unsigned)groups),
                       dim3(64 * kWavesPerBlock), 0, ctx->stream, bytes, alpha, skip, rag, rv, rb, w, bound, (unsigned long long *)partial,
                       pstride, (const double2 *)ctx->d_twB, (const FzTwA *)ctx->d_twAB, ctx->mod, vk, chal, (unsigned long long *)tpartial,
                       tstride);
    return fz_check_hip(hipGetLastError(), "aggregate_target_encoded_ragged launch");
}

}  // namespace

// fz_aggregate_target_encoded_ragged_async: the partials of both kinds zeroed (theirs alone), the fused pass in launches of
// kFzRaggedMax groups, then cent() of the aggregates' sums when the caller wants int32 -- fz_launch_aggregate_encoded_ragged's
// sequence with the targets beside it.  Record lengths are multiples of 16 bytes here (the entry checks it).
int fz_launch_aggregate_target_encoded_ragged(fz_ctx *ctx, const uint8_t *bytes, const int32_t *alpha, const int *skip, const int32_t *vk,
                                              const int32_t *chal, const size_t *h_offsets, size_t groups, int l, int w, int64_t bound,
                                              int64_t *d_partial, size_t pstride, int64_t *d_target_partial, size_t tstride, int32_t *d_out) {
    const unsigned rv = (unsigned)l * (unsigned)ctx->degree, rb = (unsigned)fz_record_bytes(ctx->degree, l, w);
    int rc = partials_clear(ctx, d_partial, pstride, rv, groups, "aggregate partials clear");
    if (rc == FZ_OK) rc = partials_clear(ctx, d_target_partial, tstride, (size_t)ctx->degree, groups, "target partials clear");
    for (size_t g0 = 0; rc == FZ_OK && g0 < groups; g0 += (size_t)kFzRaggedMax) {
        const size_t n = groups - g0 < (size_t)kFzRaggedMax ? groups - g0 : (size_t)kFzRaggedMax;
        rc = fz_dispatch<6, 8>(ctx, FZ_E_UNSUPPORTED, [&](auto logd, auto fast) {
            return launch_aggregate_target_encoded_ragged<logd(), fast()>(ctx, bytes, alpha, skip, vk, chal, h_offsets + g0, n, rv, rb, w,
                                                                          (int)bound, d_partial + g0 * pstride, pstride,
                                                                          d_target_partial + g0 * tstride, tstride);
        });
    }
    if (rc != FZ_OK || d_out == nullptr) return rc;
    return partials_cent(ctx, d_partial, pstride, rv, groups, d_out);
}
