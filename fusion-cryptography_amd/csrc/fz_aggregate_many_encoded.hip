// fz_aggregate_many_encoded.hip -- many committees' signatures aggregated straight from their compact byte encoding in one launch
// ("Many committees in one launch"): aggregate_encoded_ragged, the walk of aggregate_encoded
// (fz_aggregate_encoded_dev.h) over groups of signers of different sizes, each with a partial of its own.
#include "fz_aggregate_encoded_dev.h"
#include "../../include/fusion_hip.h"

namespace {

// partial + g * pstride [rec_values] int64 += sum over the signers i of group g, rows [rag.off[g], rag.off[g + 1]) of the
// concatenated byte stream, of `alpha` and of `skip`, with skip[i] == 0 of cent(NTT(z_i) (.) alpha_hat_i); the caller zeroed the
// partials.  Grid (chunk columns, slices, groups): a workgroup owns one chunk column for one slice of one group's signers.  The
// slice count is the launch's, not the group's: slice s of group g holds rag.base[g] signers, the first rag.extra[g] slices one
// more, and a group of fewer signers than slices leaves the slices behind its last signer empty.
// A workgroup whose slice is empty -- a group smaller than the slice count, a group of no signers, a slice whose every signer is
// skipped -- leaves as a whole before the first barrier and writes nothing: the decision is made from the group table and the
// slice's skip words alone, which every wave of the workgroup reads alike (64 words per round, none at or past the slice's end).
// Signer indices are those of the concatenated arrays (32 bits: fewer than 2^32 records per call), so the bytes, alpha_hat and
// the skip words have no base per group; the partial's lives in the lanes' address arithmetic (aggregate_encoded_slice: dst).
// LDS: that of the transforms.
template <int LOGD, bool FAST>
__global__ __launch_bounds__(64 * kWavesPerBlock) void aggregate_encoded_ragged(const uint8_t *in, const int32_t *__restrict__ alpha,
                                                                                const int *__restrict__ skip, const FzRagged rag,
                                                                                unsigned rec_values, unsigned rec_bytes, int w, int bound,
                                                                                unsigned long long *partial, size_t pstride,
                                                                                const double2 *__restrict__ twB, const FzTwA *tab, FzMod m) {
    __shared__ __attribute__((aligned(16))) double lds[lds16_doubles<LOGD>()];
    const unsigned g = blockIdx.z, s = blockIdx.y, base = rag.base[g], extra = rag.extra[g];
    const unsigned lo = rag.off[g] + s * base + (s < extra ? s : extra), hi = lo + base + (s < extra ? 1 : 0);
    if (lo >= hi) return;
    if (skip != nullptr) {
        const unsigned lane = threadIdx.x & 63;
        bool live = false;
        for (unsigned j = lo; j < hi && !live; j += 64) live = __ballot(j + lane < hi && skip[j + lane] == 0) != 0;
        if (!live) return;
    }
    aggregate_encoded_slice<LOGD, FAST>(lds, in, alpha, skip, lo, hi, blockIdx.x, rec_values, rec_bytes, w, bound,
                                        partial + (size_t)g * pstride, twB, tab, m);
}

// the launch of groups [0, groups) of h_offsets (at most kFzRaggedMax); the slice count is the launch's (ragged_slices)
template <int LOGD, bool FAST>
int launch_aggregate_encoded_ragged(fz_ctx *ctx, const uint8_t *bytes, const int32_t *alpha, const int *skip, const size_t *h_offsets,
                                    size_t groups, unsigned rv, unsigned rb, int w, int bound, int64_t *partial, size_t pstride) {
    FzRagged rag;
    const size_t columns = (rv + kChunk - 1) / kChunk;
    const size_t slices = ragged_slices((size_t)ctx->grid_aggenc_rag, columns, h_offsets, groups, rag);
    if (slices == 0) return FZ_OK;                        // nobody adds to these partials: they stay as the entry cleared them
    hipLaunchKernelGGL((aggregate_encoded_ragged<LOGD, FAST>), dim3((unsigned)columns, (unsigned)slices, (unsigned)groups),
                       dim3(64 * kWavesPerBlock), 0, ctx->stream, bytes, alpha, skip, rag, rv, rb, w, bound, (unsigned long long *)partial,
                       pstride, (const double2 *)ctx->d_twB, (const FzTwA *)ctx->d_twAB, ctx->mod);
    return fz_check_hip(hipGetLastError(), "aggregate_encoded_ragged launch");
}

}  // namespace

// the kernel's own resident grid (context creation; degrees 64 / 256, nothing to query at the others)
int fz_aggregate_many_encoded_query_grid(fz_ctx *ctx) {
    return fz_dispatch<6, 8>(ctx, FZ_OK, [&](auto logd, auto fast) {
        return fz_resident_grid(ctx, aggregate_encoded_ragged<logd(), fast()>, 64 * kWavesPerBlock,
                                "occupancy query (aggregate_encoded_ragged)", &ctx->grid_aggenc_rag);
    });
}

// fz_aggregate_encoded_ragged_async: the partials zeroed (theirs alone: the words between two partials are not touched), the fused
// pass in launches of kFzRaggedMax groups, then cent() of the sums when the caller wants int32 (fz_reduce_i64's kernel: one launch
// over all groups when the partials are contiguous, one per group otherwise).  Record lengths are multiples of 16 bytes here (the
// entry checks it): every signer's chunks start 16-byte aligned.
int fz_launch_aggregate_encoded_ragged(fz_ctx *ctx, const uint8_t *bytes, const int32_t *alpha, const int *skip, const size_t *h_offsets,
                                       size_t groups, int l, int w, int64_t bound, int64_t *d_partial, size_t pstride, int32_t *d_out) {
    const unsigned rv = (unsigned)l * (unsigned)ctx->degree, rb = (unsigned)fz_record_bytes(ctx->degree, l, w);
    int rc = partials_clear(ctx, d_partial, pstride, rv, groups, "aggregate partials clear");
    for (size_t g0 = 0; rc == FZ_OK && g0 < groups; g0 += (size_t)kFzRaggedMax) {
        const size_t n = groups - g0 < (size_t)kFzRaggedMax ? groups - g0 : (size_t)kFzRaggedMax;
        rc = fz_dispatch<6, 8>(ctx, FZ_E_UNSUPPORTED, [&](auto logd, auto fast) {
            return launch_aggregate_encoded_ragged<logd(), fast()>(ctx, bytes, alpha, skip, h_offsets + g0, n, rv, rb, w, (int)bound,
                                                                   d_partial + g0 * pstride, pstride);
        });
    }
    if (rc != FZ_OK || d_out == nullptr) return rc;
    return partials_cent(ctx, d_partial, pstride, rv, groups, d_out);
}
