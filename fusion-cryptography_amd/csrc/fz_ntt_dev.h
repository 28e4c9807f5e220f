// fz_ntt_dev.h -- the device building blocks that more than one unit uses (fz_ntt.hip, which describes the schedules, fz_polymul.hip,
// fz_records.hip, fz_scheme_fused.hip): geometry, chunk staging, passes and pipelined loop of the 16-per-lane schedule; the radix-4
// passes, twiddle loaders and wave-tasks.  No kernels and no host code here; everything is private to the unit that includes it.
#ifndef FZ_NTT_DEV_H
#define FZ_NTT_DEV_H

#include "fz_internal.h"
#include <utility>

namespace {
typedef int fz_v4i __attribute__((ext_vector_type(4)));

template <int LOGD>
struct Geom {
    static constexpr int D = 1 << LOGD;
    static constexpr int L = D / 16;              // lanes per polynomial
    static constexpr int PPW = 64 / L;            // polynomials per wave
    static constexpr int SB = LOGD - 4;           // stages of the contiguous pass
    static constexpr int NE = 16 - (16 >> SB);    // per-lane twiddles of the contiguous pass
    static constexpr int PS = D + 2 * (D / 16);   // doubles per polynomial in LDS (16-B pad per 16)
};

__device__ __forceinline__ int pad16(int j) { return j + 2 * (j >> 4); }

// ------------------------------------------------------------------------------------------
// Global <-> LDS staging shared by both directions.
// A wave-task covers PPW consecutive polynomials = ONE contiguous chunk of 1024 int32 (4 KiB) of
// the batch, whatever the degree.  All global traffic is 16 bytes per lane, 1 KiB contiguous per
// wave instruction (4 instructions per task); the lane <-> coefficient mappings the passes need are
// produced by LDS reads/writes.  int32 staging image: chunk element j at word j + 4*(j>>4)
// (20-word rows: the 16-byte-per-lane accesses at a 64-byte lane stride stay conflict free).
// ------------------------------------------------------------------------------------------
constexpr int kChunk = 1024;                         // int32 per wave-task
constexpr int kStageWords = kChunk + 4 * (kChunk / 16);   // 1280 words = 5 KiB

__device__ __forceinline__ int pad4(int j) { return j + 4 * (j >> 4); }

struct Chunk { int4 v0, v1, v2, v3; };

// issue the task's 4 coalesced 16-byte loads.  `task` is wave-uniform, so "does the whole chunk lie inside the batch" is a
// scalar test: every chunk but a ragged last one takes ONE scalar base and the lane's 32-bit offset (the four loads differ
// in their immediate offsets only); the ragged one clamps each piece to the last valid 16 bytes.
// Streaming loads: the 16-per-lane kernels run on batches far larger than the caches and read every input once
// (+2-4 % at 2^18..2^20 rows, +9 % at 2^16 with cold inputs; the radix-4 kernels, used for small batches whose
// data may well be cache-resident, keep normal loads: streaming ones cost them 3-5 % at 2^12 rows)
__device__ __forceinline__ int4 nt_load4(const int32_t *p) {
    const fz_v4i t = __builtin_nontemporal_load(reinterpret_cast<const fz_v4i *>(p));
    return make_int4(t.x, t.y, t.z, t.w);
}

__device__ __forceinline__ Chunk chunk_load(const int32_t *in, size_t task, size_t total, int lane) {
    Chunk c;
    if ((task + 1) * kChunk <= total) {
        const int32_t *b = in + task * kChunk;
        c.v0 = nt_load4(b + 4 * lane);
        c.v1 = nt_load4(b + 4 * lane + 256);
        c.v2 = nt_load4(b + 4 * lane + 512);
        c.v3 = nt_load4(b + 4 * lane + 768);
    } else {
        const size_t base = task * kChunk + 4 * lane;
        const size_t last = total - 4;
        c.v0 = nt_load4(in + (base < total ? base : last));
        c.v1 = nt_load4(in + (base + 256 < total ? base + 256 : last));
        c.v2 = nt_load4(in + (base + 512 < total ? base + 512 : last));
        c.v3 = nt_load4(in + (base + 768 < total ? base + 768 : last));
    }
    return c;
}

__device__ __forceinline__ void chunk_to_lds(int32_t *stage, int lane, const Chunk &c) {
    *reinterpret_cast<int4 *>(stage + pad4(4 * lane)) = c.v0;
    *reinterpret_cast<int4 *>(stage + pad4(256 + 4 * lane)) = c.v1;
    *reinterpret_cast<int4 *>(stage + pad4(512 + 4 * lane)) = c.v2;
    *reinterpret_cast<int4 *>(stage + pad4(768 + 4 * lane)) = c.v3;
}

// a lane's 16 consecutive values of the image as doubles (LANDED: of the unpadded chunk as chunk_load_lds leaves it, below)
template <bool LANDED = false>
__device__ __forceinline__ void image_to_doubles(const int32_t *img, int lane, double (&a)[16]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int4 t = *reinterpret_cast<const int4 *>(img + (LANDED ? 16 * lane + 4 * k : pad4(16 * lane + 4 * k)));
        a[4 * k + 0] = (double)t.x;
        a[4 * k + 1] = (double)t.y;
        a[4 * k + 2] = (double)t.z;
        a[4 * k + 3] = (double)t.w;
    }
}

// Wave-local synchronisation.  Every LDS exchange in these kernels is between lanes of ONE wave
// (each wave owns a private staging region), and a wave's DS instructions execute in order, so no
// s_barrier is needed: the release/acquire pair makes the compiler wait for the outstanding LDS
// operations (s_waitcnt lgkmcnt(0)) and keeps it from moving LDS accesses across this point.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// The same for the stretch of an iteration in which a direct-to-LDS chunk (chunk_load_lds) is in flight: a release at workgroup
// scope would wait for that chunk (it writes LDS), which is the one thing the stretch exists not to do.  Wavefront scope still
// keeps the compiler from moving LDS accesses across; a wave's DS instructions execute in order, and the data dependences on
// the reads bring their own waits.
__device__ __forceinline__ void wave_sync_inflight() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// A WHOLE chunk straight into LDS: four global_load_lds_dwordx4 (1 KiB per wave instruction, lane i's 16 bytes at LDS base + 16 i;
// the instruction offset advances the global and the LDS address alike), same scalar base, lane offset and streaming policy as
// chunk_load.  The image at `land` is the chunk as it lies in memory: 4 KiB, no padding.  The chunk costs no register while in
// flight and no ds_write afterwards; the compiler does not follow it into LDS, so the reader waits itself (chunk_landed).
constexpr int kLandOff = kStageWords;                // word offset of the landing area in a wave's region: behind the staging image
__device__ __forceinline__ void chunk_load_lds(const int32_t *in, size_t task, int lane, int32_t *land) {
    typedef const __attribute__((address_space(1))) void *gptr;
    typedef __attribute__((address_space(3))) void *lptr;
    const gptr g = (gptr)(in + task * kChunk + 4 * lane);
    const lptr l = (lptr)land;
    __builtin_amdgcn_global_load_lds(g, l, 16, 0, 2);         // aux 2: nt
    __builtin_amdgcn_global_load_lds(g, l, 16, 1024, 2);
    __builtin_amdgcn_global_load_lds(g, l, 16, 2048, 2);
    __builtin_amdgcn_global_load_lds(g, l, 16, 3072, 2);
}

// wait until a chunk_load_lds has landed that was followed by exactly YOUNGER vector memory operations (vmcnt counts loads and
// stores in order of issue: s_waitcnt vmcnt(YOUNGER), the other counters left alone)
template <int YOUNGER>
__device__ __forceinline__ void chunk_landed() {
    static_assert(YOUNGER >= 0 && YOUNGER < 16, "low four bits of vmcnt");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_s_waitcnt(0x0F70 | YOUNGER);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

constexpr int kWavesPerBlock = 4;

// Streaming (non-temporal) stores for outputs the kernel never reads back.  A normal store allocates the line
// dirty in this XCD's 4 MiB L2; for a transform that writes as much as it reads, half of the L2 then holds data
// nobody will hit, and the dirty lines are written back in bursts (and at the end of the kernel).  Measured on the
// NTT kernels: 2^14..2^18 rows 14-20 % faster (2^18 rows: 66 % -> 77 % of HBM peak), the bench's 2^12 rows 3-5 %.
__device__ __forceinline__ void nt_store4(int32_t *p, const int4 &v) {
    fz_v4i t = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(t, reinterpret_cast<fz_v4i *>(p));
}

// the same as a normal store: for outputs the NEXT launch of the stream transforms (ntt_jobs16, fz_multi_plan)
__device__ __forceinline__ void plain_store4(int32_t *p, const int4 &v) {
    fz_v4i t = {v.x, v.y, v.z, v.w};
    *reinterpret_cast<fz_v4i *>(p) = t;
}

// the task's 4 coalesced 16-byte stores (same scalar split as chunk_load: only a ragged last chunk predicates its lanes);
// PLAIN: normal instead of streaming stores (ntt_jobs16_keep)
// the stores of a chunk known to be whole: exactly four vector memory operations, and global ones whatever the compiler knows of
// the pointer (the job tables of at most eight entries hand it over as a generic one: a flat store counts in lgkmcnt as well)
template <bool PLAIN = false>
__device__ __forceinline__ void chunk_store_whole(int32_t *out, size_t task, int lane, const int4 &o0, const int4 &o1, const int4 &o2,
                                                  const int4 &o3) {
    typedef __attribute__((address_space(1))) fz_v4i *gptr;
    const gptr b = (gptr)(out + task * kChunk + 4 * lane);
    const fz_v4i t0 = {o0.x, o0.y, o0.z, o0.w}, t1 = {o1.x, o1.y, o1.z, o1.w}, t2 = {o2.x, o2.y, o2.z, o2.w}, t3 = {o3.x, o3.y, o3.z, o3.w};
    if constexpr (PLAIN) {
        b[0] = t0;
        b[64] = t1;
        b[128] = t2;
        b[192] = t3;
    } else {
        __builtin_nontemporal_store(t0, b);
        __builtin_nontemporal_store(t1, b + 64);
        __builtin_nontemporal_store(t2, b + 128);
        __builtin_nontemporal_store(t3, b + 192);
    }
}

template <bool PLAIN = false>
__device__ __forceinline__ void chunk_store(int32_t *out, size_t task, size_t total, int lane, const int4 &o0, const int4 &o1,
                                            const int4 &o2, const int4 &o3) {
    if ((task + 1) * kChunk <= total) {
        int32_t *b = out + task * kChunk;
        if constexpr (PLAIN) {
            plain_store4(b + 4 * lane, o0);
            plain_store4(b + 4 * lane + 256, o1);
            plain_store4(b + 4 * lane + 512, o2);
            plain_store4(b + 4 * lane + 768, o3);
        } else {
            nt_store4(b + 4 * lane, o0);
            nt_store4(b + 4 * lane + 256, o1);
            nt_store4(b + 4 * lane + 512, o2);
            nt_store4(b + 4 * lane + 768, o3);
        }
    } else {
        const size_t base = task * kChunk + 4 * lane;
        if (base < total) nt_store4(out + base, o0);
        if (base + 256 < total) nt_store4(out + base + 256, o1);
        if (base + 512 < total) nt_store4(out + base + 512, o2);
        if (base + 768 < total) nt_store4(out + base + 768, o3);
    }
}

// one twiddle multiply: 4-op pseudo-Mersenne form when FAST (operand bound |a| <= 2^38), else 6-op
template <bool FAST>
__device__ __forceinline__ double tw_mul(double a, double w, double w2, const FzMod m) {
    return FAST ? fz_mulmod4(a, w, w2, m) : fz_mulmod(a, w, m);
}

// ------------------------------------------------------------------------------------------
// forward: strided pass -> transpose -> contiguous pass
// ------------------------------------------------------------------------------------------
// doubles of LDS a workgroup of the 16-per-lane kernels needs: a transpose region per wave + the per-lane twiddle table
template <int LOGD> constexpr int lds16_doubles() {
    using G = Geom<LOGD>;
    return kWavesPerBlock * G::PPW * G::PS + 2 * G::NE * G::L;
}

// f(integral_constant<int, 0>) .. f(integral_constant<int, N - 1>), in order
template <class F, int... I>
__device__ __forceinline__ void static_for_seq(const F &f, std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>()), ...); }
template <int N, class F>
__device__ __forceinline__ void static_for(const F &f) { static_for_seq(f, std::make_integer_sequence<int, N>()); }

// The contiguous pass's per-lane twiddle pairs in the order the butterflies use them, cut into groups of at most four pairs
// of ONE stage (16 registers): stage ls of SB has 16 >> (SB - ls) pairs in the forward direction (FWD), 8 >> ls in the inverse.
template <int SB, bool FWD>
struct TwGroups {
    static constexpr int kPairs = 4;
    static constexpr int pairs(int ls) { return FWD ? 16 >> (SB - ls) : 8 >> ls; }
    static constexpr int groups_of(int ls) { return (pairs(ls) + kPairs - 1) / kPairs; }
    static constexpr int count() { int n = 0; for (int ls = 0; ls < SB; ++ls) n += groups_of(ls); return n; }
    static constexpr int kGroups = count();
    static constexpr int stage(int gi) { int ls = 0; while (gi >= groups_of(ls)) gi -= groups_of(ls++); return ls; }
    static constexpr int first(int gi) { int ls = 0; while (gi >= groups_of(ls)) gi -= groups_of(ls++); return gi * kPairs; }
};

// The two passes of the 16-per-lane forward transform on a lane's registers: in, a[k] = element r + L*k of the lane's polynomial
// (|a| <= 2^31); out, a[k] = element 16 * lane' + k of the transform in the order algebra/ntt.py:271-291 leaves it (lane' = the
// lane's index inside its polynomial), NOT reduced (|a| < 2^(34+SB)).  `row` is the polynomial's transpose buffer in LDS; the
// caller has finished reading whatever the buffer held before (a wave_sync) and may write it again after the return.
// `transposed` is called once the transpose buffer has been read back: from there on the wave's region is the caller's again.
struct NoHook { __device__ __forceinline__ void operator()() const {} };

template <int LOGD, bool FAST, bool STAGED = false, class TA, class HOOK = NoHook>
__device__ __forceinline__ void fwd16_passes(double (&a)[16], double *row, const int r, const double2 *s_tw, const TA &twA,
                                             const FzMod &m, const HOOK &transposed = HOOK()) {
    using G = Geom<LOGD>;
    constexpr int L = G::L, SB = G::SB;
    // strided pass: a 16-point LN transform over k with table entries 1..15 (|a| < 2^34 throughout)
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int tk = 8 >> s;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            if (k & tk) continue;
            const int e = (1 << s) + (k >> (4 - s));
            const double v = tw_mul<FAST>(a[k + tk], twA.w[e], twA.w2[e], m);
            const double u = a[k];
            a[k] = u + v;
            a[k + tk] = u - v;
        }
    }

    // transpose: element j = r + L*k  ->  lane j/16, register j%16
#pragma unroll
    for (int k = 0; k < 16; ++k) (row + r)[pad16(L * k)] = a[k];       // = row[pad16(r + L * k)]: r < L and L divides 16 (constant offsets)
    wave_sync();
    {
        const double2 *blk = reinterpret_cast<const double2 *>(row + 18 * r);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            double2 t = blk[k];
            a[2 * k] = t.x;
            a[2 * k + 1] = t.y;
        }
    }
    wave_sync();
    transposed();

    // contiguous pass: stages with distance 2^(SB-1) .. 1, per-lane twiddles
    if constexpr (!STAGED) {
#pragma unroll
        for (int ls = 0; ls < SB; ++ls) {
            const int t = 1 << (SB - 1 - ls);
            const int ebase = (16 >> SB) * ((1 << ls) - 1);
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                if (k & t) continue;
                const int g = k >> (SB - ls);
                const double2 w = s_tw[(ebase + g) * L + r];
                const double v = tw_mul<FAST>(a[k + t], w.x, w.y, m);
                const double u = a[k];
                a[k] = u + v;
                a[k + t] = u - v;
            }
        }
    } else {
        // the same butterflies, their (w, w2) pairs read a GROUP ahead (TwGroups): the next group's reads are issued before
        // this group's first multiply and nothing crosses the group's end, so a group's LDS round trip hides behind the
        // one before and at most two groups of pairs (32 registers) are live
        using TG = TwGroups<SB, true>;
        double2 w[2][TwGroups<SB, true>::kPairs];
        auto read = [&](auto gi_tag) __attribute__((always_inline)) {
            constexpr int gi = decltype(gi_tag)::value, ls = TG::stage(gi), g0 = TG::first(gi);
            constexpr int ebase = (16 >> SB) * ((1 << ls) - 1);
#pragma unroll
            for (int i = 0; i < TG::kPairs; ++i)
                if (g0 + i < TG::pairs(ls)) w[gi & 1][i] = s_tw[(ebase + g0 + i) * L + r];
        };
        read(std::integral_constant<int, 0>());
        static_for<TG::kGroups>([&](auto gi_tag) __attribute__((always_inline)) {
            constexpr int gi = decltype(gi_tag)::value, ls = TG::stage(gi), g0 = TG::first(gi);
            if constexpr (gi + 1 < TG::kGroups) read(std::integral_constant<int, gi + 1>());
            constexpr int t = 1 << (SB - 1 - ls);
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int g = k >> (SB - ls);
                if ((k & t) || g < g0 || g >= g0 + TG::kPairs) continue;
                const double2 ww = w[gi & 1][g - g0];
                const double v = tw_mul<FAST>(a[k + t], ww.x, ww.y, m);
                const double u = a[k];
                a[k] = u + v;
                a[k + t] = u - v;
            }
            __builtin_amdgcn_sched_barrier(0);
        });
    }
}

// ... and of the inverse: in, a[k] = element 16 * lane' + k (|a| <= 2^31); out, a[k] = element r + L*k, scaled by n^-1, NOT
// centred (|a| <= q/2 + q * 2^-13: every output has passed the last stage's multiply).
template <int LOGD, bool FAST, bool STAGED = false, class TA, class HOOK = NoHook>
__device__ __forceinline__ void inv16_passes(double (&a)[16], double *row, const int r, const double2 *s_tw, const TA &twA,
                                             const FzMod &m, const HOOK &transposed = HOOK()) {
    using G = Geom<LOGD>;
    constexpr int L = G::L, SB = G::SB;
    // contiguous pass: GS stages with distance 1, 2, .. 2^(SB-1); operands |u - v| <= 2^(32+ls)
    if constexpr (!STAGED) {
#pragma unroll
        for (int ls = 0; ls < SB; ++ls) {
            const int t = 1 << ls;
            const int ebase = 16 - (16 >> ls);
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                if (k & t) continue;
                const int g = k >> (ls + 1);
                const double2 w = s_tw[(ebase + g) * L + r];
                const double u = a[k], v = a[k + t];
                a[k] = u + v;
                a[k + t] = tw_mul<FAST>(u - v, w.x, w.y, m);
            }
        }
    } else {
        // pairs read a group ahead: see fwd16_passes
        using TG = TwGroups<SB, false>;
        double2 w[2][TwGroups<SB, false>::kPairs];
        auto read = [&](auto gi_tag) __attribute__((always_inline)) {
            constexpr int gi = decltype(gi_tag)::value, ls = TG::stage(gi), g0 = TG::first(gi);
            constexpr int ebase = 16 - (16 >> ls);
#pragma unroll
            for (int i = 0; i < TG::kPairs; ++i)
                if (g0 + i < TG::pairs(ls)) w[gi & 1][i] = s_tw[(ebase + g0 + i) * L + r];
        };
        read(std::integral_constant<int, 0>());
        static_for<TG::kGroups>([&](auto gi_tag) __attribute__((always_inline)) {
            constexpr int gi = decltype(gi_tag)::value, ls = TG::stage(gi), g0 = TG::first(gi);
            if constexpr (gi + 1 < TG::kGroups) read(std::integral_constant<int, gi + 1>());
            constexpr int t = 1 << ls;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int g = k >> (ls + 1);
                if ((k & t) || g < g0 || g >= g0 + TG::kPairs) continue;
                const double2 ww = w[gi & 1][g - g0];
                const double u = a[k], v = a[k + t];
                a[k] = u + v;
                a[k + t] = tw_mul<FAST>(u - v, ww.x, ww.y, m);
            }
            __builtin_amdgcn_sched_barrier(0);
        });
    }

    // After the contiguous pass a[0] (the sum of the lane's 16 inputs, up to 2^(31+SB)) is the one value no multiply
    // has reduced; a[1] <= 2^(29+SB), the rest less.  One fold (2 ops) brings the largest operand of the strided pass
    // down to 2^(29+SB) * 2^4 <= 2^37: the last stage can then use the 4-op multiply (16 x 2 ops saved per lane).
    if (FAST && 31 + SB + 4 > 38) a[0] = fz_fold(a[0], m);
    // transpose back to the strided layout
    {
        double2 *blk = reinterpret_cast<double2 *>(row + 18 * r);
#pragma unroll
        for (int k = 0; k < 8; ++k) blk[k] = make_double2(a[2 * k], a[2 * k + 1]);
    }
    wave_sync();
#pragma unroll
    for (int k = 0; k < 16; ++k) a[k] = (row + r)[pad16(L * k)];       // = row[pad16(r + L * k)] (see fwd16_passes)
    wave_sync();
    transposed();

    // strided pass: GS stages with distance L, 2L, 4L, 8L; uniform twiddles; n^-1 folded into the last stage.
    // Operands stay below 2^38 (see the fold above), so every stage uses the 4-op multiply when the modulus admits it.
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int tk = 1 << s;
        const int h = 8 >> s;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            if (k & tk) continue;
            const double u = a[k], v = a[k + tk];
            if (s == 3) {
                a[k] = tw_mul<FAST>(u + v, twA.n_inv, twA.n_inv2, m);
                a[k + tk] = tw_mul<FAST>(u - v, twA.w1_n_inv, twA.w1_n_inv2, m);
            } else {
                const int e = h + (k >> (s + 1));
                a[k] = u + v;
                a[k + tk] = tw_mul<FAST>(u - v, twA.w[e], twA.w2[e], m);
            }
        }
        if constexpr (STAGED) __builtin_amdgcn_sched_barrier(0);      // a stage's eight butterflies interleave, stages do not: the 6-op multiply's temporaries of two stages at once cost 8-14 registers
    }
}

// does an unpadded chunk fit a wave's region behind the staging image (the landing area of chunk_load_lds)?
template <int LOGD> constexpr bool landing_fits() {
    using G = Geom<LOGD>;
    return G::PPW * G::PS * 8 - kLandOff * 4 >= kChunk * 4 && (kLandOff * 4) % 16 == 0;
}

// the order of a wave's iterations: `whole` chunks lie inside the batch, a ragged last one (tasks == whole + 1) does not.
// iteration(task, NEXT, LANDED): NEXT, the wave's next chunk is whole and is requested during this iteration; LANDED, this
// one is whole and was.  The ragged chunk is a batch's last task and one wave's: it loads its own chunk (see fwd16_run).
template <class IT>
__device__ __forceinline__ void run16_chunks(const size_t first, const size_t stride, const size_t tasks, const size_t whole,
                                             const IT &iteration) {
    size_t task = first;
    if (task < whole) {
        for (; task + stride < whole; task += stride) iteration(task, std::true_type(), std::true_type());
        iteration(task, std::false_type(), std::true_type());
        task += stride;
    }
    if (task < tasks) iteration(task, std::false_type(), std::false_type());
}

// the whole forward kernel as a function of (block index, blocks that share the batch): ntt_fwd16 runs it over the grid,
// ntt_jobs16 over the run of workgroups a job owns
template <int LOGD, bool FAST, bool PLAIN = false>
__device__ __forceinline__ void fwd16_run(const int32_t *in, int32_t *out, size_t batch, unsigned block, unsigned nblocks, double *lds,
                                          const double2 *__restrict__ twB, const FzTwA &twA, const FzMod &m) {
    using G = Geom<LOGD>;
    constexpr int D = G::D, L = G::L, PPW = G::PPW, SB = G::SB, NE = G::NE, PS = G::PS;
    constexpr int REGION = PPW * PS;                      // doubles per wave
    static_assert(REGION * 2 >= kStageWords, "staging image must fit in the transpose buffer");
    static_assert(landing_fits<LOGD>() && landing_fits<5>() && landing_fits<6>() && landing_fits<7>() && landing_fits<8>(),
                  "a 4 KiB chunk must fit the wave's region behind the staging image, at every degree the bodies serve");
    double2 *s_tw = reinterpret_cast<double2 *>(lds + kWavesPerBlock * REGION);      // (w, w2) pairs, [NE][L]

    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;      // the wave index is uniform: say so (scalar address arithmetic)
    const int p = lane / L, r = lane % L;
    const size_t total = batch * D;
    const size_t tasks = (total + kChunk - 1) / kChunk;
    const size_t first = (size_t)block * kWavesPerBlock + wave;
    const size_t stride = (size_t)nblocks * kWavesPerBlock;
    // the wave's first chunk is requested BEFORE the twiddle table is staged: two memory latencies overlapped instead of added (a
    // launch of 2^16 rows is four iterations per wave: a microsecond of start-up is 4 % of it)
    const size_t whole = total / kChunk;                  // chunks that lie inside the batch: all but a ragged last one
    double *region = lds + wave * REGION;
    int32_t *stage = reinterpret_cast<int32_t *>(region);
    int32_t *land = stage + kLandOff;
    if (first < whole) chunk_load_lds(in, first, lane, land);          // nothing else is in the region yet
    for (int i = threadIdx.x; i < NE * L; i += 64 * kWavesPerBlock) s_tw[i] = twB[i];
    chunk_landed<0>();
    __syncthreads();                                      // the only workgroup-wide barrier
    double *row = region + p * PS;
    if (first >= tasks) return;
    // Software pipeline.  gfx9 has ONE in-order counter (vmcnt) for loads and stores, so a wait for a
    // prefetched load also waits for every store issued before... and, at a loop header, the compiler must
    // assume the worst over all entry paths.  A whole chunk comes by chunk_load_lds into the LANDING AREA, the 4 KiB of the
    // wave's region behind the staging image: the transposed doubles cover it only between the transpose's write and read, so
    // an iteration (1) reads its inputs from the landing area, (2) computes up to the transpose, (3) requests the NEXT chunk
    // into the landing area, (4) computes the rest and moves the outputs through the staging image, (5) issues the global
    // stores and (6) waits until all but those four stores have retired (chunk_landed<4>): the chunk has had the second
    // half of the iteration to arrive, the stores have a whole iteration, and the chunk holds no register meanwhile.

    // One iteration.  NEXT: another WHOLE chunk of this wave follows and is requested here.  LANDED: this chunk is whole and its
    // inputs are in the landing area; else it is the ragged last chunk of the batch -- one wave's last task -- and takes the
    // register path every chunk took through round 11 (chunk_load clamps, chunk_to_lds stages the padded image, chunk_store
    // predicates), loaded at the top of its own iteration: prefetched, its sixteen registers would set the peak of every kernel
    // for the sake of one wave per batch.  The forms are peeled (run16_chunks), not branched: a run-time condition around
    // loads made the compiler wait for ALL memory operations -- the previous iteration's stores -- at the loop header (rounds
    // 1-5: 3-8 % on the stand-alone kernels), and chunk_landed<4> counts on exactly four stores behind the request.
    auto iteration = [&](const size_t task, auto next_tag, auto landed_tag) __attribute__((always_inline)) {
        constexpr bool next = decltype(next_tag)::value;
        constexpr bool landed = decltype(landed_tag)::value;
        if constexpr (!landed) chunk_to_lds(stage, lane, chunk_load(in, task, total, lane));
        wave_sync();
        double a[16];
        {
            int x[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) x[k] = landed ? land[p * D + r + L * k] : (stage + pad4(p * D) + r)[pad4(L * k)];      // = stage[pad4(p * D + r + L * k)]: r < L and L divides 16
#pragma unroll
            for (int k = 0; k < 16; ++k) a[k] = (double)x[k];
        }
        wave_sync();

        fwd16_passes<LOGD, FAST, true>(a, row, r, s_tw, twA, m, [&]() __attribute__((always_inline)) {
            if constexpr (next) chunk_load_lds(in, task + stride, lane, land);
        });

        // lane holds chunk elements [16*lane, 16*lane + 16): centre, stage, store coalesced
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int4 o;
            o.x = (int)fz_cent(a[4 * k + 0], m);
            o.y = (int)fz_cent(a[4 * k + 1], m);
            o.z = (int)fz_cent(a[4 * k + 2], m);
            o.w = (int)fz_cent(a[4 * k + 3], m);
            *reinterpret_cast<int4 *>(stage + pad4(16 * lane + 4 * k)) = o;
        }
        wave_sync_inflight();
        const int4 o0 = *reinterpret_cast<const int4 *>(stage + pad4(4 * lane));
        const int4 o1 = *reinterpret_cast<const int4 *>(stage + pad4(256 + 4 * lane));
        const int4 o2 = *reinterpret_cast<const int4 *>(stage + pad4(512 + 4 * lane));
        const int4 o3 = *reinterpret_cast<const int4 *>(stage + pad4(768 + 4 * lane));
        wave_sync_inflight();
        if constexpr (landed) chunk_store_whole<PLAIN>(out, task, lane, o0, o1, o2, o3);
        else chunk_store<PLAIN>(out, task, total, lane, o0, o1, o2, o3);
        if constexpr (next) chunk_landed<4>();
    };
    run16_chunks(first, stride, tasks, whole, iteration);
}

// ------------------------------------------------------------------------------------------
// inverse: contiguous pass -> transpose -> strided pass (n^{-1} folded into the last stage)
// ------------------------------------------------------------------------------------------
template <int LOGD, bool FAST, bool PLAIN = false>
__device__ __forceinline__ void inv16_run(const int32_t *in, int32_t *out, size_t batch, unsigned block, unsigned nblocks, double *lds,
                                          const double2 *__restrict__ itwB, const FzTwA &twA, const FzMod &m) {
    using G = Geom<LOGD>;
    constexpr int D = G::D, L = G::L, PPW = G::PPW, SB = G::SB, NE = G::NE, PS = G::PS;
    constexpr int REGION = PPW * PS;
    double2 *s_tw = reinterpret_cast<double2 *>(lds + kWavesPerBlock * REGION);

    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;      // the wave index is uniform: say so (scalar address arithmetic)
    const int p = lane / L, r = lane % L;
    const size_t total = batch * D;
    const size_t tasks = (total + kChunk - 1) / kChunk;
    const size_t first = (size_t)block * kWavesPerBlock + wave;
    const size_t stride = (size_t)nblocks * kWavesPerBlock;
    const size_t whole = total / kChunk;
    double *region = lds + wave * REGION;
    int32_t *stage = reinterpret_cast<int32_t *>(region);
    int32_t *land = stage + kLandOff;
    if (first < whole) chunk_load_lds(in, first, lane, land);          // before the table, landing area, waits: see fwd16_run
    for (int i = threadIdx.x; i < NE * L; i += 64 * kWavesPerBlock) s_tw[i] = itwB[i];
    chunk_landed<0>();
    __syncthreads();
    double *row = region + p * PS;
    if (first >= tasks) return;

    auto iteration = [&](const size_t task, auto next_tag, auto landed_tag) __attribute__((always_inline)) {       // pipeline and peeling: see fwd16_run
        constexpr bool next = decltype(next_tag)::value;
        constexpr bool landed = decltype(landed_tag)::value;
        if constexpr (!landed) chunk_to_lds(stage, lane, chunk_load(in, task, total, lane));
        wave_sync();
        double a[16];
        image_to_doubles<landed>(landed ? land : stage, lane, a);
        wave_sync();

        inv16_passes<LOGD, FAST, true>(a, row, r, s_tw, twA, m, [&]() __attribute__((always_inline)) {
            if constexpr (next) chunk_load_lds(in, task + stride, lane, land);
        });

#pragma unroll
        for (int k = 0; k < 16; ++k) (stage + pad4(p * D) + r)[pad4(L * k)] = (int)fz_cent(a[k], m);      // = stage[pad4(p * D + r + L * k)]: r < L and L divides 16 (constant offsets)
        wave_sync_inflight();
        const int4 o0 = *reinterpret_cast<const int4 *>(stage + pad4(4 * lane));
        const int4 o1 = *reinterpret_cast<const int4 *>(stage + pad4(256 + 4 * lane));
        const int4 o2 = *reinterpret_cast<const int4 *>(stage + pad4(512 + 4 * lane));
        const int4 o3 = *reinterpret_cast<const int4 *>(stage + pad4(768 + 4 * lane));
        wave_sync_inflight();
        if constexpr (landed) chunk_store_whole<PLAIN>(out, task, lane, o0, o1, o2, o3);
        else chunk_store<PLAIN>(out, task, total, lane, o0, o1, o2, o3);
        if constexpr (next) chunk_landed<4>();
    };
    run16_chunks(first, stride, tasks, whole, iteration);
}

// ------------------------------------------------------------------------------------------
// 4 coefficients per lane ("radix-4 in place"): the low-latency schedule for batches that give the
// 16-per-lane kernels less than a few waves per SIMD (BASELINE's B = 4096 is one wave per SIMD
// there).  D/4 lanes own a polynomial; log4(D) passes of two stages each on 4 registers
// {base + k*s}, s = D/4, D/16, .., 1; between passes the polynomial lives in LDS as doubles at
// XOR-swizzled natural positions (conflict-free ds_read/write_b64 for every pass stride, 2-way on
// the final 16-byte accesses).  Global traffic needs no staging: the first pass reads
// x[m + (D/4)k] (256 B contiguous per wave instruction), the last leaves 4 contiguous outputs per
// lane (16-byte coalesced stores); mirrored for the inverse.  Pass 0 twiddles are wave-uniform
// (SGPR); each later pass uses 3 per-lane twiddles kept in registers across tasks.
// Only even log2(D) (the scheme's degrees 64 and 256).
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ int swz4(int j) { return j ^ (((j >> 4) & 7) << 2); }


// per-lane twiddles are kept either as (w, w * K/q) pairs or as w alone with the quotient twiddle recomputed at each use
// (one more fp64 multiply per twiddle and pass, half the registers: the fused kernels trade it for occupancy)
__device__ __forceinline__ double tw_w(const double2 &t) { return t.x; }
__device__ __forceinline__ double tw_q(const double2 &t, const FzMod &) { return t.y; }
__device__ __forceinline__ double tw_w(const double &t) { return t; }
__device__ __forceinline__ double tw_q(const double &t, const FzMod &m) {
    double w = t;
    asm volatile("" : "+v"(w));        // opaque: the product must be recomputed where it is used, not hoisted into nine more registers
    return w * m.kq;                   // the same IEEE product the host table holds
}
__device__ __forceinline__ void tw_set(double2 &dst, const double2 &src) { dst = src; }
__device__ __forceinline__ void tw_set(double &dst, const double2 &src) { dst = src.x; }

// the log4(D) in-place passes of the radix-4 forward transform on one lane's 4 values per row group (natural positions
// mm + (D/4)k in, bit-reversed-order positions 4mm..4mm+3 out, NOT yet centred).  NR independent row groups (a wave's 64
// lanes hold 64 / (D/4) polynomials per group) go through the passes in lock step: one wave-local synchronisation per
// pass whatever NR is, twiddles and LDS offsets computed once, and NR independent dependency chains for the fp64 pipeline.
// Row group r of this lane's polynomial lives at region + r * 256 doubles.
template <int LOGD, bool FAST, int NR, typename TW = double2, typename TWA = FzTwA>
__device__ __forceinline__ void fwd4_passes_n(double (&a)[NR][4], double *region, const TW (&twl)[LOGD / 2 - 1][3],
                                              const TWA &twA, const FzMod &m, int mm) {
    constexpr int D = 1 << LOGD, P = LOGD / 2;
#pragma unroll
    for (int i = 0; i < P; ++i) {
        const int s = D >> (2 * i + 2);
        const int base = (mm / s) * 4 * s + mm % s;
        double wA, wA2, wB0, wB02, wB1, wB12;
        if (i == 0) {
            wA = twA.w[1]; wA2 = twA.w2[1]; wB0 = twA.w[2]; wB02 = twA.w2[2]; wB1 = twA.w[3]; wB12 = twA.w2[3];
        } else {
            wA = tw_w(twl[i - 1][0]); wA2 = tw_q(twl[i - 1][0], m);
            wB0 = tw_w(twl[i - 1][1]); wB02 = tw_q(twl[i - 1][1], m);
            wB1 = tw_w(twl[i - 1][2]); wB12 = tw_q(twl[i - 1][2], m);
            wave_sync();
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const double *reg = region + r * 256;
                if (s == 1) {
                    const double2 lo = *reinterpret_cast<const double2 *>(reg + swz4(base));
                    const double2 hi = *reinterpret_cast<const double2 *>(reg + swz4(base + 2));
                    a[r][0] = lo.x; a[r][1] = lo.y; a[r][2] = hi.x; a[r][3] = hi.y;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) a[r][k] = reg[swz4(base + k * s)];
                }
            }
        }
        // stage 2i: distance 2s, one twiddle; stage 2i+1: distance s, two twiddles
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            double v = tw_mul<FAST>(a[r][2], wA, wA2, m), u = a[r][0];
            a[r][0] = u + v; a[r][2] = u - v;
            v = tw_mul<FAST>(a[r][3], wA, wA2, m); u = a[r][1];
            a[r][1] = u + v; a[r][3] = u - v;
            v = tw_mul<FAST>(a[r][1], wB0, wB02, m); u = a[r][0];
            a[r][0] = u + v; a[r][1] = u - v;
            v = tw_mul<FAST>(a[r][3], wB1, wB12, m); u = a[r][2];
            a[r][2] = u + v; a[r][3] = u - v;
        }
        if (i < P - 1) {
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                double *reg = region + r * 256;
#pragma unroll
                for (int k = 0; k < 4; ++k) reg[swz4(base + k * s)] = a[r][k];
            }
        }
    }
}

template <int LOGD, typename TW = double2>
__device__ __forceinline__ void fwd4_load_twiddles(TW (&twl)[LOGD / 2 - 1][3], const double2 *__restrict__ tw2, int mm) {
    constexpr int D = 1 << LOGD, P = LOGD / 2;
#pragma unroll
    for (int i = 1; i < P; ++i) {
        const int s = D >> (2 * i + 2), g = mm / s, pw = 1 << (2 * i);
        if constexpr (__is_same(TW, double2)) {
            twl[i - 1][0] = tw2[pw + g];
            twl[i - 1][1] = tw2[2 * pw + 2 * g];
            twl[i - 1][2] = tw2[2 * pw + 2 * g + 1];
        } else {
            twl[i - 1][0] = tw2[pw + g].x;
            twl[i - 1][1] = tw2[2 * pw + 2 * g].x;
            twl[i - 1][2] = tw2[2 * pw + 2 * g + 1].x;
        }
    }
}

// One wave-task = NR row groups (NR * 64 / (D/4) consecutive polynomials), one task per wave, WAVES waves per workgroup,
// grid = tasks / WAVES: no persistent loop (a loop's bookkeeping -- 64-bit task arithmetic, the prefetch state, the
// conditional refill -- cost the one-row-per-wave kernel 7-9 % at the bench's 4096 rows: 4.74 -> 4.32 us cold).
// Measured on one box, forward, degree 256, cold operands (tools/microbench/ntt_variants.hip, profiles/r03_ntt_variants.txt):
//   4096 rows: NR = 1 4.32 us (the loop kernel 4.74; NR = 2 4.51; NR = 4 5.4 -- too few waves);
//   8192 rows: NR = 2 6.03 us (NR = 1 6.23-6.51; the loop kernel 7.09; the 16-per-lane kernel 6.52);
//   16384 rows: NR = 4 9.24 us (NR = 2 10.3; NR = 1 10.6; the loop kernel 11.3; 16-per-lane 9.40);
//   from 32768 rows the 16-per-lane kernel leads (15.0 us against 16.6).
// The waves of a workgroup never talk to each other (wave-private LDS regions, no s_barrier).
// one wave-task of the forward transform: NR row groups starting at polynomial poly0 (this lane's polynomial of group 0)
template <int LOGD, bool FAST, int NR>
__device__ __forceinline__ void fwd4_task(const int32_t *in, int32_t *out, size_t batch, size_t poly0, double *region, int mm,
                                          const double2 *__restrict__ tw2, const FzTw4 &twA, const FzMod &m) {
    constexpr int D = 1 << LOGD, LP = D / 4, PPW = 64 / LP, P = LOGD / 2;
    int x[NR][4];                                 // the data loads first: they have the longest way to go
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const size_t poly = poly0 + (size_t)r * PPW;
        const int32_t *src = in + (poly < batch ? poly : batch - 1) * D + mm;
#pragma unroll
        for (int k = 0; k < 4; ++k) x[r][k] = src[k * LP];
    }
    double2 twl[P - 1][3];
    fwd4_load_twiddles<LOGD>(twl, tw2, mm);
    double a[NR][4];
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
        for (int k = 0; k < 4; ++k) a[r][k] = (double)x[r][k];
    fwd4_passes_n<LOGD, FAST, NR>(a, region, twl, twA, m, mm);
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const size_t poly = poly0 + (size_t)r * PPW;
        if (poly < batch)
            nt_store4(out + poly * D + 4 * mm, make_int4((int)fz_cent(a[r][0], m), (int)fz_cent(a[r][1], m), (int)fz_cent(a[r][2], m),
                                                          (int)fz_cent(a[r][3], m)));
    }
}

// the log4(D) in-place passes of the radix-4 inverse on one lane's 4 values per row group (bit-reversed positions
// 4mm..4mm+3 in, natural positions mm + (D/4)k out, n^-1 applied, NOT yet centred); NR row groups in lock step (see
// fwd4_passes_n)
template <int LOGD, bool FAST, int NR, typename TW = double2, typename TWA = FzTwA>
__device__ __forceinline__ void inv4_passes_n(double (&a)[NR][4], double *region, const TW (&twl)[LOGD / 2 - 1][3],
                                              const TWA &twA, const FzMod &m, int mm) {
    constexpr int P = LOGD / 2;
#pragma unroll
    for (int i = 0; i < P; ++i) {
        const int s = 1 << (2 * i);
        const int base = (mm / s) * 4 * s + mm % s;
        if (i > 0) {
            wave_sync();
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const double *reg = region + r * 256;
#pragma unroll
                for (int k = 0; k < 4; ++k) a[r][k] = reg[swz4(base + k * s)];
            }
        }
        if (i < P - 1) {
            // GS stage 2i (distance s, two twiddles) then stage 2i+1 (distance 2s, one twiddle);
            // operands stay below 2^(33+2i+1) <= 2^38
            const double w0 = tw_w(twl[i][0]), q0 = tw_q(twl[i][0], m), w1 = tw_w(twl[i][1]), q1 = tw_q(twl[i][1], m),
                         w2_ = tw_w(twl[i][2]), q2 = tw_q(twl[i][2], m);
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                double u = a[r][0], v = a[r][1];
                a[r][0] = u + v; a[r][1] = tw_mul<FAST>(u - v, w0, q0, m);
                u = a[r][2]; v = a[r][3];
                a[r][2] = u + v; a[r][3] = tw_mul<FAST>(u - v, w1, q1, m);
                u = a[r][0]; v = a[r][2];
                a[r][0] = u + v; a[r][2] = tw_mul<FAST>(u - v, w2_, q2, m);
                u = a[r][1]; v = a[r][3];
                a[r][1] = u + v; a[r][3] = tw_mul<FAST>(u - v, w2_, q2, m);
                // Degree 256 with raw int32 inputs: a[0] is the only value no multiply has reduced (the sum of four inputs, up
                // to 2^33; a[1] <= 2^31.1, a[2], a[3] <= 2^30.1).  Folding it once (2 ops) keeps every later operand below
                // 2^31.1 * 2^6 = 2^37.1, inside the 4-op multiply's 2^38 bound up to and including the final stage -- which
                // otherwise needs the general 6-op form four times (8 extra ops per lane).
                if (FAST && i == 0 && 31 + LOGD > 38) a[r][0] = fz_fold(a[r][0], m);
                double *reg = region + r * 256;
                if (s == 1) {
                    *reinterpret_cast<double2 *>(reg + swz4(base)) = make_double2(a[r][0], a[r][1]);
                    *reinterpret_cast<double2 *>(reg + swz4(base + 2)) = make_double2(a[r][2], a[r][3]);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) reg[swz4(base + k * s)] = a[r][k];
                }
            }
        } else {
            // last pass: uniform twiddles itw[2], itw[3], itw[1]; n^-1 folded into the final stage.
            // Its operands are below 2^38 for raw int32 inputs: 2^(31+LOGD) up to degree 128, 2^37.1 at degree 256
            // thanks to the fold after pass 0 -- so the 4-op multiply serves whenever the modulus admits it.
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                double u = a[r][0], v = a[r][1];
                a[r][0] = u + v; a[r][1] = tw_mul<FAST>(u - v, twA.w[2], twA.w2[2], m);
                u = a[r][2]; v = a[r][3];
                a[r][2] = u + v; a[r][3] = tw_mul<FAST>(u - v, twA.w[3], twA.w2[3], m);
                u = a[r][0]; v = a[r][2];
                a[r][0] = tw_mul<FAST>(u + v, twA.n_inv, twA.n_inv2, m);
                a[r][2] = tw_mul<FAST>(u - v, twA.w1_n_inv, twA.w1_n_inv2, m);
                u = a[r][1]; v = a[r][3];
                a[r][1] = tw_mul<FAST>(u + v, twA.n_inv, twA.n_inv2, m);
                a[r][3] = tw_mul<FAST>(u - v, twA.w1_n_inv, twA.w1_n_inv2, m);
            }
        }
    }
}

template <int LOGD, typename TW = double2>
__device__ __forceinline__ void inv4_load_twiddles(TW (&twl)[LOGD / 2 - 1][3], const double2 *__restrict__ itw2, int mm) {
    constexpr int D = 1 << LOGD, P = LOGD / 2;
#pragma unroll
    for (int i = 0; i < P - 1; ++i) {
        const int s = 1 << (2 * i), g = mm / s;
        tw_set(twl[i][0], itw2[D / (2 * s) + 2 * g]);
        tw_set(twl[i][1], itw2[D / (2 * s) + 2 * g + 1]);
        tw_set(twl[i][2], itw2[D / (4 * s) + g]);
    }
}

template <int LOGD, bool FAST, int NR>
__device__ __forceinline__ void inv4_task(const int32_t *in, int32_t *out, size_t batch, size_t poly0, double *region, int mm,
                                          const double2 *__restrict__ itw2, const FzTw4 &twA, const FzMod &m) {
    constexpr int D = 1 << LOGD, LP = D / 4, PPW = 64 / LP, P = LOGD / 2;
    int4 x[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const size_t poly = poly0 + (size_t)r * PPW;
        x[r] = *reinterpret_cast<const int4 *>(in + (poly < batch ? poly : batch - 1) * D + 4 * mm);
    }
    double2 twl[P - 1][3];
    inv4_load_twiddles<LOGD>(twl, itw2, mm);
    double a[NR][4];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        a[r][0] = (double)x[r].x; a[r][1] = (double)x[r].y; a[r][2] = (double)x[r].z; a[r][3] = (double)x[r].w;
    }
    inv4_passes_n<LOGD, FAST, NR>(a, region, twl, twA, m, mm);
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const size_t poly = poly0 + (size_t)r * PPW;
        if (poly < batch) {
            int32_t *dst = out + poly * D + mm;
#pragma unroll
            for (int k = 0; k < 4; ++k) __builtin_nontemporal_store((int)fz_cent(a[r][k], m), dst + k * LP);
        }
    }
}

}  // namespace

#endif
