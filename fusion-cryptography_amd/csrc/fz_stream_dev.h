// fz_stream_dev.h -- what the units of streaming kernels share (fz_pointwise.hip, fz_aggregate.hip): the workgroup size, the
// centring to int32, the streaming 16-byte accesses, the grid of a flat launch, and the term of the verification target, which
// fz_aggregate_target_encoded.hip forms as fz_aggregate.hip does.  No kernels here; everything is private to the
// unit that includes it.
#ifndef FZ_STREAM_DEV_H
#define FZ_STREAM_DEV_H

#include "fz_internal.h"

namespace {

constexpr int kBlock = 256;

__device__ __forceinline__ int cent_i32(double x, const FzMod m) { return (int)fz_cent(x, m); }

// streaming (non-temporal) 16-byte load: operands a kernel reads exactly once
typedef int fz_v4i __attribute__((ext_vector_type(4)));      // 16-byte vector the non-temporal builtins accept
__device__ __forceinline__ int4 ld_stream4(const int4 *p) {
    const fz_v4i t = __builtin_nontemporal_load(reinterpret_cast<const fz_v4i *>(p));
    return make_int4(t.x, t.y, t.z, t.w);
}
__device__ __forceinline__ void st_stream4(int4 *p, const int4 &v) {
    const fz_v4i t = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(t, reinterpret_cast<fz_v4i *>(p));
}

// one int4 column of the verification target: acc += (L * c + R) * alpha, the inner value |L * c mod q + R| < 2^32
__device__ __forceinline__ void agg_target4(int4 L, int4 R, int4 ch, int4 a, double (&acc)[4], FzMod m) {
    acc[0] += fz_mulmod(fz_mulmod((double)L.x, (double)ch.x, m) + (double)R.x, (double)a.x, m);
    acc[1] += fz_mulmod(fz_mulmod((double)L.y, (double)ch.y, m) + (double)R.y, (double)a.y, m);
    acc[2] += fz_mulmod(fz_mulmod((double)L.z, (double)ch.z, m) + (double)R.z, (double)a.z, m);
    acc[3] += fz_mulmod(fz_mulmod((double)L.w, (double)ch.w, m) + (double)R.w, (double)a.w, m);
}

unsigned grid_for(fz_ctx *ctx, size_t work_items, int per_cu = -1) {
    size_t blocks = (work_items + kBlock - 1) / kBlock;
    // default: a flat grid, one item per thread (45.0 us per 1024 signatures for sign_core against 49.7 with the grid capped at
    // 8 workgroups per CU, cold: round 2)
    // A launch's threads, gridDim.x * blockDim.x, must stay below 2^32: the runtime refuses a product of exactly 2^32 ("invalid
    // configuration argument": 2^32 items, a fill of 16 GiB) and takes it mod 2^32 beyond.  Every caller walks its items with a
    // grid-stride loop, so the flat grid ends there.
    size_t cap = per_cu > 0 ? (size_t)ctx->num_cu * per_cu : (size_t)0xffffffffu / kBlock;
    if (blocks < 1) blocks = 1;
    return (unsigned)(blocks < cap ? blocks : cap);
}

}  // namespace

#endif
