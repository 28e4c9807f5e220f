// fz_records_args.h -- the argument rules the compact-bytes entries of the C ABI share, written once for the host units that hold
// such entries (fz_records_capi.hip, fz_key_records_capi.hip, fz_aggregate_target_encoded_capi.hip).  Host code only; everything is private to the unit that includes it.
#ifndef FZ_RECORDS_ARGS_H
#define FZ_RECORDS_ARGS_H

#include "fz_internal.h"
#include "../../include/fusion_hip.h"

// a bound B of some kind of record, `what` for the message: B in [1, (q-1)/2] -> *w = bit_length(2 B), the kind's field width
static int records_bound(const fz_ctx *ctx, int64_t bound, const char *what, int *w) {
    FZ_REQUIRE(bound >= 1 && bound <= ((int64_t)ctx->q - 1) / 2, "%s %lld outside [1, (q-1)/2]", what, (long long)bound);
    int b = 0;
    while ((2 * bound) >> b) ++b;
    *w = b;
    return FZ_OK;
}

// compact byte encoding: the checks of all ten entries, in the order that decides the return code when more than one thing is
// wrong: context, rows and bound; n == 0 is FZ_OK from here on; the entry's pointers (`ptrs_wrong`: what is wrong with them, NULL
// when nothing is -- which pointers an entry takes and how they must be aligned is its own business); degree; size.
// -> *w = the field width (records_bound).  Conditions of an entry that hold whatever n is come before this call, its own limits after it.
static int records_args(fz_ctx *ctx, size_t n, int64_t rows, int64_t bound, const char *ptrs_wrong, int *w) {
    FZ_REQUIRE(ctx && rows >= 1, "bad argument");
    FZ_TRY(records_bound(ctx, bound, "bound", w));
    if (n == 0) return FZ_OK;
    FZ_REQUIRE(!ptrs_wrong, "%s", ptrs_wrong);
    if (ctx->logd != 6 && ctx->logd != 8) return fz_set_error(FZ_E_UNSUPPORTED, "the byte encoding needs degree 64 or 256");
    FZ_REQUIRE((uint64_t)rows * (uint64_t)ctx->degree <= 0x7fffffffull && n <= ((size_t)-1 >> 3) / ((size_t)rows * ctx->degree),
               "%zu records of %lld rows are too many", n, (long long)rows);
    return FZ_OK;
}

// the buffers of an entry that wants all of them 16-byte aligned
template <class... P>
static const char *records_ptrs(const P *...p) {
    if (!(p && ...)) return "NULL argument";
    return (((uintptr_t)p | ...) & 15) != 0 ? "buffers must be 16-byte aligned" : nullptr;
}

// the consumers that walk ONE record's chunks (blockIdx names the record): every record must begin on a 16-byte unit
static inline int records_whole_units(const fz_ctx *ctx, int rows, int w) {
    const size_t rb = fz_record_bytes(ctx->degree, rows, w);
    if (rb % 16 != 0) return fz_set_error(FZ_E_UNSUPPORTED, "records of %zu bytes: reading them record by record needs a multiple of 16", rb);
    return FZ_OK;
}

// many committees in one launch, group g owning records [h_offsets[g], h_offsets[g + 1]): the rules of
// fz_aggregate_encoded_ragged_async, which every entry of that form shares, in their order -- fz_aggregate_encoded_async's, then the
// offsets and the stride.  -> *w; with groups == 0 nothing behind records_args is looked at, and the caller returns FZ_OK.
static inline int records_ragged_args(fz_ctx *ctx, const uint8_t *d_bytes, const int32_t *d_alpha_hat, const size_t *h_offsets, size_t groups,
                                      int l, int64_t bound, const int64_t *d_partial, size_t partial_stride, const int32_t *d_out, int *w) {
    FZ_REQUIRE(groups == 0 || h_offsets, "NULL argument");
    const size_t total = groups ? h_offsets[groups] : 0;
    FZ_REQUIRE(total == 0 || d_alpha_hat, "NULL argument");
    FZ_REQUIRE((((uintptr_t)d_alpha_hat | (uintptr_t)d_out) & 15) == 0, "alpha_hat and the aggregates must be 16-byte aligned");
    // (a call whose groups are all empty reads no byte: the stream may be NULL then)
    FZ_TRY(records_args(ctx, groups == 0 ? 0 : (total ? total : 1), l, bound,
                        total ? records_ptrs(d_bytes, d_partial, d_alpha_hat) : records_ptrs(d_partial), w));
    if (groups == 0) return FZ_OK;
    FZ_TRY(records_whole_units(ctx, l, *w));
    for (size_t g = 0; g < groups; ++g) FZ_REQUIRE(h_offsets[g] <= h_offsets[g + 1], "offsets must not decrease");
    FZ_REQUIRE(groups == 1 || (partial_stride >= (size_t)l * ctx->degree && (partial_stride & 1) == 0),
               "partial_stride must be at least l * degree, and even (16-byte aligned partials)");
    for (size_t g = 0; g < groups; ++g)
        if (h_offsets[g + 1] - h_offsets[g] >= ((size_t)1 << 22))
            return fz_set_error(FZ_E_UNSUPPORTED, "group %zu: %zu signers are too many for exact fp64 accumulation (< 2^22)", g,
                                h_offsets[g + 1] - h_offsets[g]);
    if (total >= 0xffffffc0ull) return fz_set_error(FZ_E_UNSUPPORTED, "%zu records in one call: signer indices are 32-bit", total);
    return FZ_OK;
}

#endif
