// fz_records_capi.hip -- the compact-bytes entries of the C ABI (include/fusion_hip.h): encode, decode
// and check, signing and key generation straight to records, aggregation and verification straight from them.  Host code only: the
// argument rules the entries share (fz_records_args.h), and per entry what is its own; the kernels and their launchers are the units
// fz_records.hip, fz_sign_encoded.hip, fz_sign_records.hip, fz_keygen_records.hip, fz_aggregate_encoded.hip,
// fz_aggregate_many_encoded.hip and fz_verify_encoded.hip.
#include "fz_records_args.h"      // records_bound, records_args, records_ptrs, records_whole_units, records_ragged_args: shared

extern "C" {

int fz_encode_records_async(fz_ctx *ctx, const int32_t *d_rows, size_t n, int rows, int coef, int64_t bound, uint8_t *d_bytes,
                            int *d_status) {
    int w = 0;
    FZ_TRY(records_args(ctx, n, rows, bound, records_ptrs(d_rows, d_bytes, d_status), &w));
    if (n == 0) return FZ_OK;
    FZ_DEV(ctx);
    return fz_launch_records(ctx, false, d_rows, d_bytes, n, rows, coef != 0, w, bound, d_status);
}

int fz_decode_records_async(fz_ctx *ctx, const uint8_t *d_bytes, size_t n, int rows, int coef, int64_t bound, int32_t *d_rows,
                            int *d_status) {
    int w = 0;
    FZ_TRY(records_args(ctx, n, rows, bound, records_ptrs(d_bytes, d_rows, d_status), &w));
    if (n == 0) return FZ_OK;
    FZ_DEV(ctx);
    return fz_launch_records(ctx, true, d_bytes, d_rows, n, rows, coef != 0, w, bound, d_status);
}

int fz_check_records_async(fz_ctx *ctx, const uint8_t *d_bytes, size_t n, int rows, int64_t bound, int *d_status) {
    int w = 0;
    FZ_TRY(records_args(ctx, n, rows, bound, records_ptrs(d_bytes, d_status), &w));
    if (n == 0) return FZ_OK;
    FZ_DEV(ctx);
    return fz_launch_check_records(ctx, d_bytes, n, rows, w, bound, d_status);
}

// sigma = left_sk_hat * c_hat + right_sk_hat (fusion/fusion.py:534-557) and its encoding in one pass: the signature's rows never
// reach memory
int fz_sign_encoded_async(fz_ctx *ctx, const int32_t *d_sk_hat, const int32_t *d_c_hat, size_t N, int l, int64_t bound, uint8_t *d_bytes,
                          int *d_status) {
    int w = 0;
    const char *ptrs_wrong = records_ptrs(d_sk_hat, d_bytes, d_status);
    if (!ptrs_wrong) ptrs_wrong = records_ptrs(d_c_hat);
    FZ_TRY(records_args(ctx, N, l, bound, ptrs_wrong, &w));
    if (N == 0) return FZ_OK;
    FZ_DEV(ctx);
    return fz_launch_sign_encoded(ctx, d_sk_hat, d_c_hat, N, l, w, bound, d_bytes, d_status);
}

// the same from the key's "secret" record: z = INTT(NTT(sL) * c_hat) + sR, the right half added in the coefficient domain
// (fusion/fusion.py:534-557 by linearity), and its encoding in one pass: neither the key's nor the signature's rows reach memory.
// fz_sign_encoded_async's checks in its order; the key's bound is held to the output bound's range
int fz_sign_records_async(fz_ctx *ctx, const uint8_t *d_key_bytes, int64_t key_bound, const int32_t *d_c_hat, size_t N, int l,
                          int64_t bound, uint8_t *d_bytes, int *d_status) {
    int w = 0, wk = 0;
    const char *ptrs_wrong = records_ptrs(d_key_bytes, d_bytes, d_status);
    if (!ptrs_wrong) ptrs_wrong = records_ptrs(d_c_hat);
    FZ_REQUIRE(ctx && l >= 1, "bad argument");
    FZ_TRY(records_bound(ctx, key_bound, "key bound", &wk));
    FZ_TRY(records_args(ctx, N, l, bound, ptrs_wrong, &w));
    if (N == 0) return FZ_OK;
    FZ_DEV(ctx);
    return fz_launch_sign_records(ctx, d_key_bytes, wk, key_bound, d_c_hat, N, l, w, bound, d_bytes, d_status);
}

// Key generation straight to "secret" records: records of 2 l rows under the key's bound, so the shared checks in their order
// behind the form of the coefficients; then the entry's own limit, a workgroup per (key, half) in one grid.
int fz_keygen_records_async(fz_ctx *ctx, const int32_t *d_A, const int32_t *d_coef, int coef_rows, size_t N, int l, int64_t key_bound,
                            uint8_t *d_key_bytes, int32_t *d_vk, int *d_status) {
    int wk = 0;
    FZ_REQUIRE(ctx && l >= 1, "bad argument");
    FZ_REQUIRE(coef_rows == 1 || coef_rows == l, "coef_rows %d: 1 or l = %d", coef_rows, l);
    FZ_TRY(records_bound(ctx, key_bound, "key bound", &wk));
    FZ_TRY(records_args(ctx, N, 2 * (int64_t)l, key_bound, records_ptrs(d_A, d_coef, d_key_bytes, d_vk, d_status), &wk));
    if (N == 0) return FZ_OK;
    FZ_REQUIRE(N <= 0x3fffffffu, "%zu keys of %d rows are too many", N, l);
    FZ_DEV(ctx);
    return fz_launch_keygen_records(ctx, d_A, d_coef, coef_rows == l && l > 1, N, l, wk, key_bound, d_key_bytes, d_vk, d_status);
}

int fz_aggregate_encoded_async(fz_ctx *ctx, const uint8_t *d_bytes, const int32_t *d_alpha_hat, const int *d_skip, size_t N, int l,
                               int64_t bound, int64_t *d_partial, int32_t *d_out) {
    int w = 0;
    FZ_REQUIRE(N == 0 || d_alpha_hat, "NULL argument");
    FZ_REQUIRE((((uintptr_t)d_alpha_hat | (uintptr_t)d_out) & 15) == 0, "alpha_hat and the aggregate must be 16-byte aligned");
    FZ_TRY(records_args(ctx, N, l, bound, records_ptrs(d_bytes, d_partial, d_alpha_hat), &w));
    if (N == 0) return FZ_OK;
    FZ_TRY(records_whole_units(ctx, l, w));
    if (N >= ((size_t)1 << 22))
        return fz_set_error(FZ_E_UNSUPPORTED, "N=%zu too large for exact fp64 accumulation (< 2^22)", N);
    FZ_DEV(ctx);
    return fz_launch_aggregate_encoded(ctx, d_bytes, d_alpha_hat, d_skip, N, l, w, bound, d_partial, d_out);
}

// many committees in one launch: group g owns records [h_offsets[g], h_offsets[g + 1]).  The argument rules are
// fz_aggregate_encoded_async's, in its order, then the offsets and the stride (records_ragged_args).
int fz_aggregate_encoded_ragged_async(fz_ctx *ctx, const uint8_t *d_bytes, const int32_t *d_alpha_hat, const int *d_skip,
                                      const size_t *h_offsets, size_t groups, int l, int64_t bound, int64_t *d_partial,
                                      size_t partial_stride, int32_t *d_out) {
    int w = 0;
    FZ_TRY(records_ragged_args(ctx, d_bytes, d_alpha_hat, h_offsets, groups, l, bound, d_partial, partial_stride, d_out, &w));
    if (groups == 0) return FZ_OK;
    FZ_DEV(ctx);
    return fz_launch_aggregate_encoded_ragged(ctx, d_bytes, d_alpha_hat, d_skip, h_offsets, groups, l, w, bound, d_partial, partial_stride,
                                              d_out);
}

int fz_verify_encoded_async(fz_ctx *ctx, const int32_t *d_A, const uint8_t *d_bytes, size_t N, int l, int64_t bound,
                            const int32_t *d_target, const int32_t *d_vk, const int32_t *d_c_hat, int *d_verdicts) {
    int w = 0;
    FZ_REQUIRE((d_target != nullptr) != (d_vk != nullptr || d_c_hat != nullptr) && (d_vk != nullptr) == (d_c_hat != nullptr),
               "exactly one of d_target, or the pair d_vk and d_c_hat, must be given");
    const char *ptrs_wrong = nullptr;
    if (!d_A || !d_bytes || !d_verdicts) ptrs_wrong = "NULL argument";
    else if ((((uintptr_t)d_bytes | (uintptr_t)d_A) & 15) != 0) ptrs_wrong = "the bytes and A must be 16-byte aligned";
    else if ((((uintptr_t)d_target | (uintptr_t)d_vk | (uintptr_t)d_c_hat | (uintptr_t)d_verdicts) & 3) != 0)
        ptrs_wrong = "target, keys, challenges and verdicts must be 4-byte aligned";
    FZ_TRY(records_args(ctx, N, l, bound, ptrs_wrong, &w));
    if (N == 0) return FZ_OK;
    FZ_TRY(records_whole_units(ctx, l, w));
    const size_t rb = fz_record_bytes(ctx->degree, l, w);
    if (rb > 0xffffffffull) return fz_set_error(FZ_E_UNSUPPORTED, "records of %zu bytes are too long", rb);
    FZ_DEV(ctx);
    return fz_launch_verify_encoded(ctx, d_A, d_bytes, N, l, w, bound, d_target, d_vk, d_c_hat, d_verdicts);
}

}  // extern "C"
