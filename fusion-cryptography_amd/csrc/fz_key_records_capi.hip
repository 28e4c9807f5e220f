// fz_key_records_capi.hip -- the entries of the C ABI that read a key's "secret" record for something other than signing
// (include/fusion_hip.h): the verification key straight from the key's bytes.  Host code only: the
// argument rules are the compact-bytes entries' (fz_records_args.h), the kernel and its launcher are the unit fz_vk_records.hip.
#include "fz_records_args.h"

extern "C" {

// vk = cent(sum_k A_k (.) FWD(s_k)) per half (fusion/fusion.py:363-370) from the fields of the record.  Records of 2 l rows under the
// key's bound: fz_keygen_records_async's checks in their order; then the entry's own limits, a workgroup per (key, half) in one
// grid here and the exactness of the sums in the launcher.
int fz_vk_records_async(fz_ctx *ctx, const int32_t *d_A, const uint8_t *d_key_bytes, int64_t key_bound, size_t N, int l, int32_t *d_vk,
                        int *d_status) {
    int wk = 0;
    FZ_REQUIRE(ctx && l >= 1, "bad argument");
    FZ_TRY(records_bound(ctx, key_bound, "key bound", &wk));
    FZ_TRY(records_args(ctx, N, 2 * (int64_t)l, key_bound, records_ptrs(d_A, d_key_bytes, d_vk, d_status), &wk));
    if (N == 0) return FZ_OK;
    FZ_REQUIRE(N <= 0x3fffffffu, "%zu keys of %d rows are too many", N, l);
    FZ_DEV(ctx);
    return fz_launch_vk_records(ctx, d_A, d_key_bytes, wk, key_bound, N, l, d_vk, d_status);
}

}  // extern "C"
