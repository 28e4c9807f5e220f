// fz_aggregate_encoded_dev.h -- the body the two aggregations straight from the bytes share (fz_aggregate_encoded.hip: one
// committee per launch; fz_aggregate_many_encoded.hip: many committees of different sizes per launch): one workgroup's walk over
// one slice of signers for one chunk column, from the first prefetch to the atomics of the epilogue; and what the launches of many
// committees share (fz_aggregate_many_encoded.hip, fz_aggregate_target_encoded.hip): the launch's slice count and group table, the clearing of the partials and their centring.  No kernels here;
// private to the unit that includes it.
#ifndef FZ_AGGREGATE_ENCODED_DEV_H
#define FZ_AGGREGATE_ENCODED_DEV_H

#include "fz_records_dev.h"

namespace {

// partial [rec_values] int64 += sum over the signers i in [lo, hi) with skip[i] == 0 of cent(NTT(z_i) (.) alpha_hat_i), z_i = the
// fields of record i minus B, for the chunk column `col` of the records; the caller zeroed `partial`.  `in`, `alpha` and `skip`
// are the whole arrays and i indexes them: a group of signers is a range of i, so nothing but `partial` is per group.
// A wave-task is (signer i, chunk col of that signer's record): chunk c of every signer covers the same 1024 coefficients
// [1024c, 1024c + 1024) of the [l][d] aggregate.  The workgroup's four waves take the slice's signers round-robin, each wave sums
// its products in 16 fp64 registers per lane (exact: every product is canonical, |p| <= (q-1)/2, and fewer than 2^22 of them stay
// below 2^53), the four waves' sums meet in LDS and the workgroup adds its 1024 integers to `partial` with 64-bit integer atomics
// (agent scope, executed at the memory side: integer addition is exact and commutative, so the order of arrival cannot change a
// bit of the result).
// Pipeline of records_decode: the next signer's packed chunk is in flight while the current one is transformed, the wave's last
// signer is peeled off.  A skipped signer's bytes are never read (one task is one record: the test is wave-uniform); whether
// the signer after next is skipped is asked for BEFORE the prefetch is issued, so the answer is older than the prefetch in the
// in-order memory counter and waiting for it does not wait for the prefetch.  Neither the test nor the look-ahead reads a skip
// word at or past hi.
// The lanes of a tail chunk past the record's end read nothing (packed_load stops at the record's length); what they compute from
// zero units stays in whole polynomials of their own and is never added to `partial`.
// `lds`: the workgroup's lds16_doubles<LOGD>() doubles (wave_lds: the packed chunk lies behind the int32 image in the wave's
// region).  Workgroup barriers inside: every wave of the workgroup calls this, with the same arguments.
template <int LOGD, bool FAST>
__device__ __forceinline__ void aggregate_encoded_slice(double *lds, const uint8_t *in, const int32_t *__restrict__ alpha,
                                                        const int *__restrict__ skip, const unsigned lo, const unsigned hi,
                                                        const unsigned col, unsigned rec_values, unsigned rec_bytes, int w, int bound,
                                                        unsigned long long *partial, const double2 *__restrict__ twB, const FzTwA *tab,
                                                        const FzMod &m) {
    using G = Geom<LOGD>;
    constexpr int D = G::D, L = G::L, REGION = G::PPW * G::PS;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int p = lane / L, r = lane % L;
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

// ---- many committees per launch: grid (.., slices, groups), host code ----

// The slice count of the launch of groups [0, groups) of h_offsets (at most kFzRaggedMax) on `columns` chunk columns, for a kernel
// of resident grid `grid`, and the launch's group table; -> 0 when every group is empty (nothing to launch):
// * one round: when columns x groups divides the kernel's resident grid well -- floor(grid / (columns x groups)) slices fill at
//   least 7/8 of it -- that many slices, as aggregate_encoded chooses them: every workgroup is resident from the first moment and
//   none waits for a second round (one group of 1024 signers at secpar 256: 56 us so, 67-69 us with two or four times as many);
// * several rounds of short workgroups otherwise -- a badly filled grid (16 groups x 21 columns = 336 of 512) or more columns x
//   groups than the grid holds, where the groups' sizes decide how long the last workgroup runs -- about four times the
//   resident grid, but no slices of fewer than 16 signers of the largest group (a wave needs a few signers for its prefetch to
//   pay the workgroup's prologue): 16 x 256 signers 279 -> 211 us, 70 groups of 1 .. 194 signers 390 -> 352 us.
// Never more slices than give every wave of a workgroup of the LARGEST group a signer, never above the grid limit.  The figures:
// DESIGN.md section 5.16, profiles/r16_aggregate_many_encoded.txt.
inline size_t ragged_slices(size_t grid, size_t columns, const size_t *h_offsets, size_t groups, FzRagged &rag) {
    size_t nmax = 0;
    for (size_t g = 0; g < groups; ++g) nmax = nmax < h_offsets[g + 1] - h_offsets[g] ? h_offsets[g + 1] - h_offsets[g] : nmax;
    if (nmax == 0) return 0;
    const size_t cg = columns * groups;
    size_t slices = grid / cg, cap = (nmax + kWavesPerBlock - 1) / kWavesPerBlock;
    if (slices < 1 || 8 * slices * cg < 7 * grid) {
        slices = (4 * grid + cg - 1) / cg;
        cap = (nmax + 4 * kWavesPerBlock - 1) / (4 * kWavesPerBlock);
    }
    slices = slices < cap ? slices : cap;
    slices = slices < 65535 ? slices : 65535;
    for (size_t g = 0; g < groups; ++g) {                 // as fill_ragged (fz_aggregate.hip)
        const size_t ng = h_offsets[g + 1] - h_offsets[g];
        rag.off[g] = (unsigned)h_offsets[g];
        rag.base[g] = (unsigned)(ng / slices);
        rag.extra[g] = (unsigned)(ng % slices);
    }
    rag.off[groups] = (unsigned)h_offsets[groups];
    return slices;
}

// `groups` partials of `width` int64, `stride` apart, zeroed: theirs alone, the words between two partials are not touched
inline int partials_clear(fz_ctx *ctx, int64_t *d_partial, size_t stride, size_t width, size_t groups, const char *what) {
    if (stride == width || groups == 1)
        return fz_check_hip(hipMemsetAsync(d_partial, 0, groups * width * sizeof(int64_t), ctx->stream), what);
    return fz_check_hip(hipMemset2DAsync(d_partial, stride * sizeof(int64_t), 0, width * sizeof(int64_t), groups, ctx->stream), what);
}

// d_out [groups][width] = cent() of the partials (fz_reduce_i64's kernel: one launch over all groups when the partials are
// contiguous, one per group otherwise)
inline int partials_cent(fz_ctx *ctx, const int64_t *d_partial, size_t stride, size_t width, size_t groups, int32_t *d_out) {
    if (stride == width || groups == 1) return fz_launch_reduce_i64(ctx, d_partial, d_out, groups * width);
    int rc = FZ_OK;
    for (size_t g = 0; rc == FZ_OK && g < groups; ++g) rc = fz_launch_reduce_i64(ctx, d_partial + g * stride, d_out + g * width, width);
    return rc;
}

}  // namespace

#endif
