// fz_records_args.h -- the argument rules the compact-bytes entries of the C ABI share, written once for the host units that hold
// such entries (fz_records_capi.hip, fz_key_records_capi.hip).  Host code only; everything is private to the unit that includes it.
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

#endif
