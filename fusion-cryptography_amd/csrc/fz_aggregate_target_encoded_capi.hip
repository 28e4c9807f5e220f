// fz_aggregate_target_encoded_capi.hip -- the entry of the C ABI that aggregates many committees from their compact bytes and forms
// their verification targets in the same launch (include/fusion_hip.h).  Host code only: the argument
// rules are the compact-bytes entries' (fz_records_args.h), the kernel and its launcher are the unit fz_aggregate_target_encoded.hip.
#include "fz_records_args.h"

extern "C" {

// fz_aggregate_encoded_ragged_async's rules in their order (records_ragged_args), then what the targets add: their pointers (the
// keys and challenges are read for signers only: a call whose groups are all empty may leave them NULL), their alignment, the stride.
int fz_aggregate_target_encoded_ragged_async(fz_ctx *ctx, const uint8_t *d_bytes, const int32_t *d_alpha_hat, const int *d_skip,
                                             const int32_t *d_vk, const int32_t *d_c_hat, const size_t *h_offsets, size_t groups, int l,
                                             int64_t bound, int64_t *d_partial, size_t partial_stride, int64_t *d_target_partial,
                                             size_t target_stride, int32_t *d_out) {
    int w = 0;
    FZ_TRY(records_ragged_args(ctx, d_bytes, d_alpha_hat, h_offsets, groups, l, bound, d_partial, partial_stride, d_out, &w));
    if (groups == 0) return FZ_OK;
    FZ_REQUIRE(d_target_partial && (h_offsets[groups] == 0 || (d_vk && d_c_hat)), "NULL argument");
    FZ_REQUIRE((((uintptr_t)d_vk | (uintptr_t)d_c_hat) & 15) == 0, "keys and challenges must be 16-byte aligned");
    FZ_REQUIRE(((uintptr_t)d_target_partial & 7) == 0, "target partials must be 8-byte aligned");
    FZ_REQUIRE(target_stride >= (size_t)ctx->degree && (groups == 1 || (target_stride & 1) == 0),
               "target_stride must be at least the degree, and even for more than one group");
    FZ_DEV(ctx);
    return fz_launch_aggregate_target_encoded_ragged(ctx, d_bytes, d_alpha_hat, d_skip, d_vk, d_c_hat, h_offsets, groups, l, w, bound,
                                                     d_partial, partial_stride, d_target_partial, target_stride, d_out);
}

}  // extern "C"
