// fz_aggregate.hip -- the aggregation engine: aggregate_onepass (signer slices, shared accumulator words), aggregate_direct (no
// slices, for aggregates of a few hundred signers), the generic kernel for the contexts those two do not cover, and the tile
// policy of fz_launch_aggregate.  The fused sign + aggregate path and the batch queue's ragged launches run on it.  HBM-bound
// like the other streaming kernels (fz_pointwise.hip): 16-byte-per-lane coalesced accesses, fp64 exact arithmetic from fz_arith.h.
//
// Reference formulas: fusion/fusion.py:557 (sign), :670-676 (aggregate), :706-714 (the verification target).  Every partial
// result the reference centres is congruent mod q to the lazily accumulated value here, and the final value is centred once --
// identical output.
#include "fz_stream_dev.h"
#include "../../include/fusion_hip.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------
// One-pass aggregation (fusion/fusion.py:670-676, and the verification target of :706-714 as extra columns).
//
//   out[g][k][j] = sum_i sig[g][i][k][j] * alpha[g][i][j]      (mod q; centred int32 or int64 partial sums)
//
// Work split: a workgroup owns 1024 consecutive coefficients of the aggregate (kAggR = 4 int4 columns per lane, i.e.
// four rows at degree 256, sixteen at degree 64) for ONE slice of the signers; its WAVES waves take the slice's
// signers round-robin and never talk to each other until the end.  Per signer a lane loads ONE int4 of alpha (its
// position j is the same for its four columns) and four int4 of sigma, the next signer's five loads in flight
// meanwhile.  Arithmetic: alpha = hi * 2^16 + lo (hi in [-2^15, 2^15), lo in [0, 2^16)), so x * hi and x * lo are
// below 2^47 for any int32 x and sixteen signers accumulate EXACTLY in fp64 (< 2^51) with two FMAs per coefficient
// and no reduction at all; every kAggFold signers the two sums fold back below q (fz_fold, exact).  The split of
// alpha costs 16 integer/convert operations per signer and lane, shared by the lane's 16 coefficients.
// End of the workgroup: the WAVES partials meet in LDS; with one slice per aggregate the result is written directly;
// with several, each workgroup adds its 1024 exact integers into the tile's 64-bit accumulator words with returning
// agent-scope atomics (performed at the memory side: coherent across the 8 XCD L2s without any fence); a word also
// counts its arrivals, so the thread whose add comes last holds the finished sum and writes the output (see below).
// Only sigma and alpha are ever read: no scratch round trip, no second launch.
// Workgroup -> XCD placement (speed only): workgroups b and b + 8 share an XCD, so all column blocks of one
// (aggregate, slice) pair get block ids equal mod 8 and each alpha row is fetched into ONE L2.
// ---------------------------------------------------------------------------------------------------------------
constexpr int kAggR = 4;          // int4 columns per lane (the default; 3 and 2 are instantiated too: the launcher picks what fills the chip)
constexpr int kAggDepth = 3;      // signers in flight per wave
constexpr int kAggFold = 16;      // signers between folds: 16 * 2^31 * 2^16 = 2^51 < 2^53
constexpr int kAggTile = 64 * kAggR * 4;   // coefficients per workgroup (1024)

struct AggDiv {                   // host-side arithmetic of the tile mapping (see the kernel)
    unsigned m_ncb, m_nsl;        // ceil(2^32 / ncb), ceil(2^32 / nsl): __umulhi(x, m) == x / d exactly for x * d < 2^32
    unsigned per_xcd;             // ceil(tiles / 8)
    unsigned base, extra;         // N / nsl, N % nsl
};

// The signer step of both tiled kernels, written once.  alpha = ah * 2^16 + al with ah in [-2^15, 2^15) and al in [0, 2^16), so
// x * ah and x * al are below 2^47 for any int32 x, kAggFold = 16 of them sum EXACTLY in fp64 (< 2^51, far below 2^53), and a fold
// (fz_fold, exact) brings lo + hi * 2^16 back below q before the next sixteen.  Arrays by reference, the int4s of the target term
// by value: the forms under which every instantiation compiles to the code it had with the text written out (docs/HISTORY.md §O).
__device__ __forceinline__ void agg_split(const int4 &a, double (&ah)[4], double (&al)[4]) {
    const int av[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        ah[k] = (double)(av[k] >> 16);
        al[k] = (double)(av[k] & 0xffff);
    }
}
// one int4 column of sigma (as doubles) times the split alpha, into the column's two running sums
__device__ __forceinline__ void agg_fma4(const double (&xv)[4], const double (&ah)[4], const double (&al)[4], double (&hi)[4],
                                         double (&lo)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        hi[k] = __builtin_fma(xv[k], ah[k], hi[k]);
        lo[k] = __builtin_fma(xv[k], al[k], lo[k]);
    }
}
// lo <- fold(lo) + fold(hi * 2^16), hi <- 0: every kAggFold signers, and once more at the end (where zeroing hi is dead code)
template <int R>
__device__ __forceinline__ void agg_fold(double (&lo)[R][4], double (&hi)[R][4], const FzMod m) {
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            lo[r][k] = fz_fold(lo[r][k], m) + fz_fold(hi[r][k] * 65536.0, m);
            hi[r][k] = 0.0;
        }
}
// (the term of the verification target, agg_target4: fz_stream_dev.h)

// RAG = FzNoRag: `groups` aggregates of N signers each, aggregate g's rows at g * N; RAG = FzRagged: aggregates of DIFFERENT
// sizes in one launch (fz_aggregate_*_ragged: many independent aggregate() calls, fusion.py:655, batched) -- aggregate g's
// signers are rows [off[g], off[g+1]) of the concatenated arrays, its slices from the table's base / extra
// SIGN (round 4): the signatures do not exist yet -- sigma_i = L_i * c_i + R_i (fusion.py:557) is computed from the secret key
// rows (sk_hat [N][2][l][degree]) and the challenge c [N][degree] as the signer comes up, written to sig_out, and aggregated
// from registers: what sign_core + this kernel read and write in two launches ((3l + 1) + (l + 1) rows per signature) becomes
// 3l + 2 rows in one -- the l rows of sigma are never read back.  Two signers in flight per wave instead of three (the key
// halves are two loads per column instead of one).
struct FzNoRag {};
template <int WAVES, typename RAG, bool SIGN = false, int AR = kAggR>
__global__ __launch_bounds__(64 * WAVES) void aggregate_onepass(const int32_t *sig, const int32_t *alpha, const int32_t *vkL,
                                                                const int32_t *vkR, const int32_t *c, size_t N, int l, int d4,
                                                                int ncb_a, int ncb, int nsl, int pairs, AggDiv dv,
                                                                unsigned long long *accum, int64_t *out64, size_t pstride,
                                                                int64_t *tout64, size_t tstride, int32_t *out32, FzMod m, RAG rag,
                                                                const int32_t *sk_hat = nullptr, int32_t *sig_out = nullptr) {
    constexpr bool RAGGED = !__is_same(RAG, FzNoRag);
    constexpr int DEPTH = SIGN ? 2 : kAggDepth;
    constexpr int TILE = 64 * AR * 4;                 // coefficients per workgroup: AR int4 columns per lane (1024 at AR = 4)
    __shared__ __attribute__((aligned(16))) double red[WAVES * TILE];      // 64 KiB at 8 waves
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;      // the wave index is uniform: say so (scalar address arithmetic)
    // block id -> tile t = p * ncb + cb (p = g * nsl + sb: the (aggregate, slice) pair, cb the column block).  Workgroups
    // b and b + 8 share an XCD, so XCD x = b % 8 gets the CONTIGUOUS run of tiles [x * per_xcd, (x + 1) * per_xcd): equal
    // load on every XCD (a pair-per-XCD mapping left XCDs with 21 and others with 42 workgroups at 12 slices: 30.7 us
    // instead of 21.9), and an alpha row is still fetched into one L2, two where a run of tiles ends inside a pair
    // (no integer division on the device: a uniform 64-bit divide is ~100 instructions in front of the first load;
    // quotients by ncb and nsl come from host-computed reciprocals, exact for these ranges -- AggDiv)
    const unsigned tiles = (unsigned)pairs * (unsigned)ncb, per_xcd = dv.per_xcd;
    const unsigned tl = (blockIdx.x & 7u) * per_xcd + (blockIdx.x >> 3);
    if ((blockIdx.x >> 3) >= per_xcd || tl >= tiles) return;
    const unsigned pu = ncb > 1 ? __umulhi(tl, dv.m_ncb) : tl;
    const int cb = (int)(tl - pu * (unsigned)ncb);
    const unsigned gu = nsl > 1 ? __umulhi(pu, dv.m_nsl) : pu;
    const size_t g = (size_t)gu;
    const int sb = (int)(pu - gu * (unsigned)nsl);
    size_t base = dv.base, extra = dv.extra, first_row = g * N;
    if constexpr (RAGGED) {
        base = rag.base[gu];
        extra = rag.extra[gu];
        first_row = rag.off[gu];
    }
    const size_t i0 = (size_t)sb * base + ((size_t)sb < extra ? (size_t)sb : extra);
    const size_t i1 = i0 + base + ((size_t)sb < extra ? 1 : 0);
    const bool tgt = cb >= ncb_a;
    const size_t cols_a = (size_t)l * d4;
    const int4 *alpha4 = reinterpret_cast<const int4 *>(alpha) + first_row * (size_t)d4;

    double lo[AR][4];
#pragma unroll
    for (int r = 0; r < AR; ++r)
#pragma unroll
        for (int k = 0; k < 4; ++k) lo[r][k] = 0.0;

    if (!tgt) {
        double hi[AR][4];
#pragma unroll
        for (int r = 0; r < AR; ++r)
#pragma unroll
            for (int k = 0; k < 4; ++k) hi[r][k] = 0.0;
        const int j4 = lane & (d4 - 1);                   // d4 (a power of two) divides 64: the same position for the lane's four columns
        size_t col[AR];
#pragma unroll
        for (int r = 0; r < AR; ++r) {
            const size_t cr = (size_t)cb * (64 * AR) + (size_t)r * 64 + lane;
            col[r] = cr < cols_a ? cr : cols_a - 1;       // clamped lanes compute garbage that is never written
        }
        const int4 *sig4 = reinterpret_cast<const int4 *>(sig) + first_row * cols_a;
        const int4 *sk4 = reinterpret_cast<const int4 *>(sk_hat) + first_row * 2 * cols_a;        // SIGN: [signer][L | R][l * d4]
        const int4 *c4 = reinterpret_cast<const int4 *>(c) + first_row * (size_t)d4;
        int4 *so4 = reinterpret_cast<int4 *>(sig_out) + first_row * cols_a;
        bool live[AR];                                 // SIGN: this lane's column exists (a clamped lane must not store)
#pragma unroll
        for (int r = 0; r < AR; ++r) live[r] = (size_t)cb * (64 * AR) + (size_t)r * 64 + lane < cols_a;
        // DEPTH signers in flight per wave (5 loads of 16 bytes per lane each; 10 with SIGN): a wave's signers are a SEQUENTIAL
        // chain of memory latencies otherwise (first version, one signer ahead: N = 1024 took 29 us, 11 signers per wave
        // at ~2 us each)
        int4 a_q[DEPTH], x_q[DEPTH][AR], c_q[SIGN ? DEPTH : 1], r_q[SIGN ? DEPTH : 1][AR];
        auto load = [&](int s, size_t i) {
            a_q[s] = alpha4[i * d4 + j4];
            if constexpr (SIGN) {
                c_q[s] = c4[i * d4 + j4];
#pragma unroll
                for (int r = 0; r < AR; ++r) {
                    x_q[s][r] = ld_stream4(sk4 + i * 2 * cols_a + col[r]);                  // L
                    r_q[s][r] = ld_stream4(sk4 + (i * 2 + 1) * cols_a + col[r]);            // R
                }
            } else {
#pragma unroll
                for (int r = 0; r < AR; ++r) x_q[s][r] = ld_stream4(sig4 + i * cols_a + col[r]);      // read once (alpha: by every column block)
            }
        };
        const size_t first = i0 + wave;
        int since = 0;
        // one signer from slot s: alpha split, (SIGN: the signature made and stored,) the AR x 4 products accumulated
        auto consume = [&](int s, size_t is) __attribute__((always_inline)) {
            double ah[4], al[4];
            agg_split(a_q[s], ah, al);
#pragma unroll
            for (int r = 0; r < AR; ++r) {
                double xv[4] = {(double)x_q[s][r].x, (double)x_q[s][r].y, (double)x_q[s][r].z, (double)x_q[s][r].w};
                if constexpr (SIGN) {                 // sigma = cent(cent(L * c) + R), exactly sign_kernel's arithmetic
                    const double cv[4] = {(double)c_q[s].x, (double)c_q[s].y, (double)c_q[s].z, (double)c_q[s].w};
                    const double rv[4] = {(double)r_q[s][r].x, (double)r_q[s][r].y, (double)r_q[s][r].z, (double)r_q[s][r].w};
                    int sv[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        sv[k] = cent_i32(fz_mulmod(xv[k], cv[k], m) + rv[k], m);
                        xv[k] = (double)sv[k];
                    }
                    if (live[r]) st_stream4(so4 + is * cols_a + col[r], make_int4(sv[0], sv[1], sv[2], sv[3]));     // never read back here
                }
                agg_fma4(xv, ah, al, hi[r], lo[r]);
            }
            if (++since == kAggFold) {
                since = 0;
                agg_fold<AR>(lo, hi, m);
            }
        };
        // The wave's signers first, first + WAVES, ... in a rolling window of DEPTH slots.  The loop that carries the bulk has NO
        // condition around its loads: gfx9 counts outstanding loads in ONE in-order counter, and the compiler, which must assume
        // the fewest loads any path may have issued, answered a run-time `if (next < i1) load(...)` with a wait for ALL loads at
        // the loop header -- the window drained once per DEPTH signers (one whole memory latency each time; rounds 3-4).
        // Steady loop: every slot full, every refill valid.  Then ONE pass whose refills may run out, then the drain.
        // (Written out here and in aggregate_direct: behind one helper that takes the load and consume steps, aggregate_direct's
        // generated code changes -- docs/HISTORY.md §O.)
        size_t i = first;
        if (first + (size_t)(DEPTH - 1) * WAVES < i1) {                          // wave-uniform: at least DEPTH signers
#pragma unroll
            for (int s = 0; s < DEPTH; ++s) load(s, first + (size_t)s * WAVES);
            for (; i + (size_t)(2 * DEPTH - 1) * WAVES < i1; i += (size_t)DEPTH * WAVES) {
#pragma unroll
                for (int s = 0; s < DEPTH; ++s) {
                    const size_t is = i + (size_t)s * WAVES;
                    consume(s, is);
                    load(s, is + (size_t)DEPTH * WAVES);
                }
            }
#pragma unroll
            for (int s = 0; s < DEPTH; ++s) {
                const size_t is = i + (size_t)s * WAVES, in = is + (size_t)DEPTH * WAVES;
                consume(s, is);
                if (in < i1) load(s, in);
            }
            i += (size_t)DEPTH * WAVES;
        } else {
#pragma unroll
            for (int s = 0; s < DEPTH; ++s)
                if (first + (size_t)s * WAVES < i1) load(s, first + (size_t)s * WAVES);
        }
#pragma unroll
        for (int s = 0; s < DEPTH; ++s) {                                        // the drain: fewer than DEPTH signers are left
            const size_t is = i + (size_t)s * WAVES;
            if (is < i1) consume(s, is);
        }
        agg_fold<AR>(lo, hi, m);
    } else {
        // verification target: sum_i (vkL_i * c_i + vkR_i) * alpha_i, degree/4 int4 columns in lo[0]
        const size_t tcol = (size_t)(cb - ncb_a) * 64 + lane;
        const size_t tc = tcol < (size_t)d4 ? tcol : (size_t)d4 - 1;
        const int4 *L4 = reinterpret_cast<const int4 *>(vkL) + first_row * (size_t)d4;
        const int4 *R4 = reinterpret_cast<const int4 *>(vkR) + first_row * (size_t)d4;
        const int4 *C4 = reinterpret_cast<const int4 *>(c) + first_row * (size_t)d4;
#pragma unroll 2
        for (size_t i = i0 + wave; i < i1; i += WAVES) {
            const size_t o = i * d4 + tc;
            agg_target4(L4[o], R4[o], C4[o], alpha4[o], lo[0], m);
        }
    }

    // the WAVES partials meet in LDS: element e of the tile = coefficient cb * 1024 + e of the aggregate
    {
        double *mine = red + wave * TILE + lane * 4;
#pragma unroll
        for (int r = 0; r < AR; ++r) {
            *reinterpret_cast<double2 *>(mine + r * 256) = make_double2(lo[r][0], lo[r][1]);
            *reinterpret_cast<double2 *>(mine + r * 256 + 2) = make_double2(lo[r][2], lo[r][3]);
        }
    }
    __syncthreads();
    constexpr int PER = (TILE + 64 * WAVES - 1) / (64 * WAVES);          // elements per thread in the combine steps (AR = 3: the last half is idle)
    const size_t limit = tgt ? (size_t)d4 * 4 : cols_a * 4;
    const size_t k0 = tgt ? (size_t)(cb - ncb_a) * 256 : (size_t)cb * TILE;
    const int span = tgt ? 256 : TILE;
    double sum[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const int e = threadIdx.x + u * 64 * WAVES;
        double s = 0.0;
        if (e < TILE) {
#pragma unroll
            for (int w = 0; w < WAVES; ++w) s += red[w * TILE + e];
        }
        sum[u] = s;
    }
    auto emit = [&](int e, long long v) {
        const size_t k = k0 + (size_t)e;
        if (tgt) tout64[g * tstride + k] = v;
        else if (out64) out64[g * pstride + k] = v;
        else out32[g * cols_a * 4 + k] = (int)fz_cent_i64(v, m);
    };
    if (nsl == 1) {
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int e = threadIdx.x + u * 64 * WAVES;
            if (e < span && k0 + (size_t)e < limit) emit(e, (long long)sum[u]);
        }
        return;
    }
    // Several slices per aggregate: every workgroup ADDS its exact integers into the tile's accumulator words with one
    // returning agent-scope atomic per coefficient (executed at the memory side: coherent across the 8 XCD L2s, no
    // fence).  A word carries the running sum in its low 54 bits (two's complement, |sum| < 2^53) and the number of
    // arrivals above them (each add also adds 2^54), so the value an add returns tells its thread whether it was the
    // LAST of the nsl adders of that coefficient: that thread then holds the complete sum, writes the output and
    // re-arms the word for the next launch by subtracting what it read.  No ticket, no barrier, no read-back pass:
    // the tail of the kernel is one atomic round trip (the first version -- fp64 adds, a ticket per tile, the last
    // workgroup swapping the sums out -- spent three: 8 us of fixed cost per launch, of which this removes ~2.5).
    unsigned long long *acc = accum + (g * (size_t)ncb + (size_t)cb) * TILE;
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const int e = threadIdx.x + u * 64 * WAVES;
        if (e < span && k0 + (size_t)e < limit) {
            const unsigned long long add = (unsigned long long)(long long)sum[u] + (1ull << 54);
            const unsigned long long now = __hip_atomic_fetch_add(acc + e, add, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + add;
            if ((unsigned)((now + (1ull << 53)) >> 54) == (unsigned)nsl) {
                emit(e, (long long)(now - ((unsigned long long)nsl << 54)));
                __hip_atomic_fetch_add(acc + e, 0ull - now, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // back to zero
            }
        }
    }
}


// ---------------------------------------------------------------------------------------------------------------
// Aggregation WITHOUT signer slices, for aggregates of a few hundred signers (round 4).  aggregate_onepass fills the chip
// by cutting the SIGNERS of an aggregate into slices, and pays for it at the end: every workgroup adds its tile into shared
// accumulator words (one returning atomic round trip to the memory side) and the last adder writes the output -- about
// 2 of the ~6 us a launch costs whatever N is (N = 256: 9.1 us = 30 % of the HBM roofline).  Here the chip is filled by
// cutting the COEFFICIENTS finer instead: a workgroup owns 16 int4 columns (256 contiguous bytes of a row) of R rows of the
// aggregate for ALL signers, so nothing is shared between workgroups, the result is written directly, and the only
// synchronisation is one workgroup barrier.  A wave's 64 lanes are 16 columns x 4 signers; its WAVES waves take the signers
// round-robin, DEPTH signers (R + 1 loads of 16 bytes each) in flight per lane; the 4 * WAVES partial sums of a coefficient meet
// first inside the wave (v_permlane32_swap / v_permlane16_swap: lanes 0..15 collect the other three quarters, no LDS) and
// then in 64 R doubles of LDS per wave.  R rows of a tile share ONE alpha load per signer (R = 4: 84 tiles per aggregate at
// rank 83, R = 2: 168; one row per tile and whole-row tiles were measured and dropped: every CU of an XCD then asks the L2 for
// the same alpha lines at the same time -- 256 x 4 signers 30 us against 20.7 -- profiles/r04_aggregate_direct_ab.txt).
// Same arithmetic as aggregate_onepass (alpha = hi * 2^16 + lo, exact fp64 sums folded every kAggFold signers), same outputs
// (int64 partial sums or centred int32; the verification target as extra tiles), uniform and ragged groups.
// ---------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ double dir_from_upper(double x) {        // lanes 0..31: the value lanes 32..63 hold
    unsigned lo = (unsigned)__double2loint(x), hi = (unsigned)__double2hiint(x), lo2 = lo, hi2 = hi;
    auto r = __builtin_amdgcn_permlane32_swap(lo, lo2, false, false);
    lo2 = r[1];
    r = __builtin_amdgcn_permlane32_swap(hi, hi2, false, false);
    hi2 = r[1];
    return __hiloint2double((int)hi2, (int)lo2);
}
__device__ __forceinline__ double dir_from_odd_row(double x) {      // lanes of even 16-lane rows: the value the next row holds
    unsigned lo = (unsigned)__double2loint(x), hi = (unsigned)__double2hiint(x), lo2 = lo, hi2 = hi;
    auto r = __builtin_amdgcn_permlane16_swap(lo, lo2, false, false);
    lo2 = r[1];
    r = __builtin_amdgcn_permlane16_swap(hi, hi2, false, false);
    hi2 = r[1];
    return __hiloint2double((int)hi2, (int)lo2);
}

// CW: int4 columns per tile (16: a quarter row of degree 256, four signers side by side in a wave; 64: a whole row, one signer)
template <int CW, int R, int DEPTH, int WAVES, typename RAG>
__global__ __launch_bounds__(64 * WAVES) void aggregate_direct(const int32_t *sig, const int32_t *alpha, const int32_t *vkL,
                                                               const int32_t *vkR, const int32_t *c, size_t N, int l, int d4,
                                                               int ntile_a, int64_t *out64, size_t pstride, int64_t *tout64,
                                                               size_t tstride, int32_t *out32, FzMod m, RAG rag) {
    constexpr bool RAGGED = !__is_same(RAG, FzNoRag);
    constexpr int kDirCW = CW, kDirSub = 64 / CW;
    constexpr int STEP = kDirSub * WAVES;                          // signers the workgroup takes per round
    __shared__ __attribute__((aligned(16))) double red[WAVES * CW * 4 * R];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int colw = lane & (kDirCW - 1), sub = lane / kDirCW;
    const size_t g = blockIdx.y;
    const int t = blockIdx.x;
    size_t first_row = g * N, n = N;
    if constexpr (RAGGED) {
        first_row = rag.off[g];
        n = rag.off[g + 1] - rag.off[g];
    }
    const bool tgt = t >= ntile_a;
    const int ncg = d4 / kDirCW;                                   // column groups per row (4 at degree 256, 1 at degree 64)
    const int tt = tgt ? t - ntile_a : t;
    const int cg = tt % ncg, rg = tt / ncg;
    const int j4 = cg * kDirCW + colw;
    const size_t cols_a = (size_t)l * d4;
    const int4 *alpha4 = reinterpret_cast<const int4 *>(alpha) + first_row * (size_t)d4 + j4;
    double lo[R][4];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int k = 0; k < 4; ++k) lo[r][k] = 0.0;
    const size_t i_first = (size_t)wave * kDirSub + sub;

    if (!tgt) {
        double hi[R][4];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int k = 0; k < 4; ++k) hi[r][k] = 0.0;
        size_t rowoff[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int k = rg * R + r;
            rowoff[r] = (size_t)(k < l ? k : l - 1) * d4 + j4;       // clamped rows compute garbage that is never written
        }
        const int4 *sig4 = reinterpret_cast<const int4 *>(sig) + first_row * cols_a;
        int4 a_q[DEPTH], x_q[DEPTH][R];
        // Rounds of STEP signers (a lane group takes signer `sub` of its wave's share of the round).  The round count is
        // wave-uniform; a lane whose signer of a round does not exist requests the aggregate's LAST signer instead and leaves it
        // out of the sums.  Round 5: requests are issued by the whole wave on every path -- with the lane-dependent
        // `if (i < n) load(...)` of round 4 the compiler could not count what is outstanding (one in-order counter for all
        // loads) and waited for EVERYTHING before every signer: the DEPTH-deep window was drained at each step, a whole memory
        // latency per round (N = 256: eight of them in a 9 us kernel).  Same scheme as aggregate_onepass: a steady loop whose
        // refills all exist, one pass whose refills run out, the drain -- written out in both, since behind one helper that takes
        // the load and consume steps this kernel's generated code changes (docs/HISTORY.md §O).
        const size_t w0 = (size_t)wave * kDirSub;
        const int rounds = n > w0 ? (int)((n - w0 + STEP - 1) / STEP) : 0;
        auto load = [&](int s, int round) __attribute__((always_inline)) {
            const size_t i = i_first + (size_t)round * STEP, ic = i < n ? i : n - 1;
            a_q[s] = alpha4[ic * d4];
#pragma unroll
            for (int r = 0; r < R; ++r) x_q[s][r] = ld_stream4(sig4 + ic * cols_a + rowoff[r]);
        };
        auto consume = [&](int s, int round) __attribute__((always_inline)) {
            if (i_first + (size_t)round * STEP < n) {
                double ah[4], al[4];
                agg_split(a_q[s], ah, al);
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const double xv[4] = {(double)x_q[s][r].x, (double)x_q[s][r].y, (double)x_q[s][r].z, (double)x_q[s][r].w};
                    agg_fma4(xv, ah, al, hi[r], lo[r]);
                }
            }
        };
        int since = 0;
        auto fold_if_due = [&]() __attribute__((always_inline)) {
            since += DEPTH;
            if (since + DEPTH > kAggFold) {                        // lanes of a wave differ by at most one signer: fold together
                since = 0;
                agg_fold<R>(lo, hi, m);
            }
        };
        int k0 = 0;
        if (rounds >= DEPTH) {                                       // wave-uniform
#pragma unroll
            for (int s = 0; s < DEPTH; ++s) load(s, s);
            for (; k0 + 2 * DEPTH - 1 < rounds; k0 += DEPTH) {
#pragma unroll
                for (int s = 0; s < DEPTH; ++s) {
                    consume(s, k0 + s);
                    load(s, k0 + s + DEPTH);
                }
                fold_if_due();
            }
#pragma unroll
            for (int s = 0; s < DEPTH; ++s) {
                consume(s, k0 + s);
                if (k0 + s + DEPTH < rounds) load(s, k0 + s + DEPTH);
            }
            fold_if_due();
            k0 += DEPTH;
        } else {
#pragma unroll
            for (int s = 0; s < DEPTH; ++s)
                if (s < rounds) load(s, s);
        }
#pragma unroll
        for (int s = 0; s < DEPTH; ++s)                              // the drain: fewer than DEPTH rounds are left
            if (k0 + s < rounds) consume(s, k0 + s);
        agg_fold<R>(lo, hi, m);
    } else {
        // verification target sum_i (vkL_i * c_i + vkR_i) * alpha_i (fusion.py:706-714): 16 columns of the one target row
        const int4 *L4 = reinterpret_cast<const int4 *>(vkL) + first_row * (size_t)d4 + j4;
        const int4 *R4 = reinterpret_cast<const int4 *>(vkR) + first_row * (size_t)d4 + j4;
        const int4 *C4 = reinterpret_cast<const int4 *>(c) + first_row * (size_t)d4 + j4;
#pragma unroll 2
        for (size_t i = i_first; i < n; i += STEP) {
            const size_t o = i * d4;
            agg_target4(L4[o], R4[o], C4[o], alpha4[o], lo[0], m);
        }
    }
    // the four signer quarters of the wave meet in lanes 0..15, then the waves in LDS: red[wave][r][column][k]
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            double v = lo[r][k];
            if constexpr (CW == 16) {
                v += dir_from_upper(v);
                v += dir_from_odd_row(v);
            }
            lo[r][k] = v;
        }
    if (lane < kDirCW) {
        double *mine = red + (wave * R) * (CW * 4) + lane * 4;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            *reinterpret_cast<double2 *>(mine + r * (CW * 4)) = make_double2(lo[r][0], lo[r][1]);
            *reinterpret_cast<double2 *>(mine + r * (CW * 4) + 2) = make_double2(lo[r][2], lo[r][3]);
        }
    }
    __syncthreads();
    const int rows_here = tgt ? 1 : R;
    for (int e = threadIdx.x; e < rows_here * (CW * 4); e += 64 * WAVES) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) s += red[w * R * (CW * 4) + e];
        const int r = e / (CW * 4), k = tgt ? 0 : rg * R + r;
        if (k >= l) continue;
        const size_t coef = (size_t)k * d4 * 4 + (size_t)cg * (kDirCW * 4) + (e % (CW * 4));
        const long long v = (long long)s;
        if (tgt) tout64[g * tstride + coef] = v;
        else if (out64) out64[g * pstride + coef] = v;
        else out32[g * cols_a * 4 + coef] = (int)fz_cent_i64(v, m);
    }
}

// any degree, any N: one thread per coefficient of the aggregate (and of the target), all signers in sequence.
// Only for parameter sets the one-pass kernel does not cover (degree not a power of two <= 256).
__global__ __launch_bounds__(kBlock) void aggregate_generic_kernel(const int32_t *sig, const int32_t *alpha, const int32_t *vkL,
                                                                   const int32_t *vkR, const int32_t *c, size_t N, int l, int degree,
                                                                   int64_t *out64, size_t pstride, int64_t *tout64, size_t tstride,
                                                                   int32_t *out32, FzMod m) {
    const size_t g = blockIdx.z, per = (size_t)l * degree, total = per + (vkL ? (size_t)degree : 0);
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const size_t j = e % (size_t)degree;
        double s = 0.0;
        if (e < per) {
            for (size_t i = 0; i < N; ++i)
                s += fz_mulmod((double)sig[(g * N + i) * per + e], (double)alpha[(g * N + i) * degree + j], m);
            if (out64) out64[g * pstride + e] = (int64_t)s;
            else out32[g * per + e] = (int)fz_cent_wide(s, m);
        } else {
            for (size_t i = 0; i < N; ++i) {
                const size_t o = (g * N + i) * degree + j;
                s += fz_mulmod(fz_mulmod((double)vkL[o], (double)c[o], m) + (double)vkR[o], (double)alpha[o], m);
            }
            tout64[g * tstride + j] = (int64_t)s;
        }
    }
}

}  // namespace

constexpr int kAggWaves = 8;      // waves per one-pass workgroup (4-wave workgroups, two per CU, measured no better at any size: profiles/r03_aggregate_shapes.txt)

// the host-side arithmetic of the one-pass tile mapping
static AggDiv agg_div(size_t N, int ncb, int nsl, int pairs) {
    AggDiv dv;
    dv.m_ncb = ncb > 1 ? (unsigned)((0x100000000ull + (unsigned)ncb - 1) / (unsigned)ncb) : 0u;      // unused for a divisor of 1
    dv.m_nsl = nsl > 1 ? (unsigned)((0x100000000ull + (unsigned)nsl - 1) / (unsigned)nsl) : 0u;
    dv.per_xcd = (unsigned)(((size_t)pairs * ncb + 7) / 8);
    dv.base = (unsigned)(N / (size_t)nsl);
    dv.extra = (unsigned)(N % (size_t)nsl);
    return dv;
}

template <int WAVES, int AR>
static void launch_onepass(fz_ctx *ctx, unsigned grid, const int32_t *sig, const int32_t *alpha, const int32_t *vkL,
                           const int32_t *vkR, const int32_t *c, size_t N, int l, int d4, int ncb_a, int ncb, int nsl, int pairs,
                           unsigned long long *acc, int64_t *out64, size_t pstride, int64_t *tout64, size_t tstride,
                           int32_t *out32, const FzRagged *rag, const int32_t *sk_hat = nullptr, int32_t *sig_out = nullptr) {
    const AggDiv dv = agg_div(N, ncb, nsl, pairs);
    if (sk_hat)
        hipLaunchKernelGGL((aggregate_onepass<WAVES, FzNoRag, true, AR>), dim3(grid), dim3(64 * WAVES), 0, ctx->stream, sig, alpha, vkL, vkR, c, N,
                           l, d4, ncb_a, ncb, nsl, pairs, dv, acc, out64, pstride, tout64, tstride, out32, ctx->mod, FzNoRag(), sk_hat, sig_out);
    else if (rag)
        hipLaunchKernelGGL((aggregate_onepass<WAVES, FzRagged, false, AR>), dim3(grid), dim3(64 * WAVES), 0, ctx->stream, sig, alpha, vkL, vkR, c, N,
                           l, d4, ncb_a, ncb, nsl, pairs, dv, acc, out64, pstride, tout64, tstride, out32, ctx->mod, *rag, nullptr, nullptr);
    else
        hipLaunchKernelGGL((aggregate_onepass<WAVES, FzNoRag, false, AR>), dim3(grid), dim3(64 * WAVES), 0, ctx->stream, sig, alpha, vkL, vkR, c, N,
                           l, d4, ncb_a, ncb, nsl, pairs, dv, acc, out64, pstride, tout64, tstride, out32, ctx->mod, FzNoRag(), nullptr, nullptr);
}

template <int CW, int R, int DEPTH>
static void launch_direct(fz_ctx *ctx, dim3 grid, const int32_t *sig, const int32_t *alpha, const int32_t *vkL, const int32_t *vkR,
                          const int32_t *c, size_t N, int l, int d4, int ntile_a, int64_t *out64, size_t pstride, int64_t *tout64,
                          size_t tstride, int32_t *out32, const FzRagged *rag) {
    constexpr int WAVES = 8;
    if (rag)
        hipLaunchKernelGGL((aggregate_direct<CW, R, DEPTH, WAVES, FzRagged>), grid, dim3(64 * WAVES), 0, ctx->stream, sig, alpha, vkL, vkR, c, N, l,
                           d4, ntile_a, out64, pstride, tout64, tstride, out32, ctx->mod, *rag);
    else
        hipLaunchKernelGGL((aggregate_direct<CW, R, DEPTH, WAVES, FzNoRag>), grid, dim3(64 * WAVES), 0, ctx->stream, sig, alpha, vkL, vkR, c, N, l,
                           d4, ntile_a, out64, pstride, tout64, tstride, out32, ctx->mod, FzNoRag());
}

// do the tiled kernels (aggregate_onepass, aggregate_direct) cover this context: int4 rows of a power-of-two degree <= 256
static bool agg_tiled(int d, uintptr_t align) { return d % 4 == 0 && (align & 15) == 0 && (d & (d - 1)) == 0 && d <= 256; }

// the group table of a ragged launch: aggregate g's rows, and its signers per slice and their remainder (aggregate_direct has no
// slices and reads `off` alone)
static void fill_ragged(FzRagged &rag, const size_t *h_offsets, size_t groups, size_t nsl) {
    for (size_t g = 0; g < groups; ++g) {
        const size_t ng = h_offsets[g + 1] - h_offsets[g];
        rag.off[g] = (unsigned)h_offsets[g];
        rag.base[g] = (unsigned)(ng / nsl);
        rag.extra[g] = (unsigned)(ng % nsl);
    }
    rag.off[groups] = (unsigned)h_offsets[groups];
}

// The one-pass tile choice: AR int4 columns per lane, the column blocks of the aggregate (ncb_a) and with the target's (ncb), and
// the signer slices per aggregate.
// Slices of the signers per aggregate: as many tiles (column block x aggregate x slice) as the chip holds at once --
// one 8-wave workgroup per CU (180-220 VGPRs: two waves per SIMD) -- so that every CU streams from the first moment
// and nothing waits for a second round (a 257th workgroup costs a third more: 264 tiles 28.1 us against 20.8 for 176);
// at least kAggDepth signers per wave.  Rows per column block (AR = 4 | 3 | 2 int4 columns per lane): whichever leaves the
// fewest CUs idle -- 4 aggregates of 256 signers + targets are 88 tiles per slice at AR = 4 (2 slices: 176 of 256 CUs)
// and 116 at AR = 3 (2 slices: 232).
struct AggShape { int ar, ncb_a, ncb; size_t nsl; };
static AggShape onepass_shape(size_t capacity, size_t cols_a, bool have_sig, bool have_tgt, size_t groups, size_t N) {
    const int tgt = have_tgt ? 1 : 0;                                // d4 <= 64: the target fits one column block
    auto blocks_a = [&](int ar) { return have_sig ? (int)((cols_a + 64 * ar - 1) / (64 * ar)) : 0; };
    AggShape sh = {0, 0, 0, 1};
    size_t best_tiles = 0;
    for (int cand = kAggR; cand >= 2; --cand) {
        const int na = blocks_a(cand), nb = na + tgt;
        const size_t blocks_min = (size_t)nb * groups;
        size_t ns = capacity / blocks_min;
        const size_t most = N / ((size_t)kAggWaves * kAggDepth);
        if (ns > most) ns = most;
        if (ns < 1) ns = 1;
        if (ns > 512) ns = 512;                    // the arrival count shares a 64-bit word with the sum (10 bits)
        if (ns > N && N > 0) ns = N;
        if (N == 0) ns = 1;
        const size_t tiles = blocks_min * ns;
        // the widest block stands unless a narrower one puts at least 1/16 more workgroups into the ONE round
        // (launches of more than one round keep the widest block: fewest workgroups)
        const bool take = sh.ar == 0 || (best_tiles <= capacity && tiles <= capacity && tiles * 16 >= best_tiles * 17);
        if (take) { sh = {cand, na, nb, ns}; best_tiles = tiles; }
    }
    // More tiles than CUs even at the widest block (many small aggregates in one launch: the batch queue's ragged launches):
    // the launch runs in several rounds, and at AR = 4 (190 VGPRs: one 8-wave workgroup per CU) a CU's next workgroup cannot
    // start before the previous one has drained its LDS reduction and stores.  AR = 2 (114 VGPRs: TWO workgroups per CU)
    // overlaps one workgroup's tail with the other's loads: 64 aggregates of 64 signers + targets 80.4 -> 74.0 us (0.57 ->
    // 0.62 of the HBM peak by bytes moved), 128 x 32: 95.8 -> 80.6, 256 x 16: 121 -> 99.5, 16 x 64: 23.9 -> 20.0; launches
    // of one round lose with it (8 x 128: 20.3 -> 23.5 us) and keep the rule above (profiles/r05_queue_aggregates.txt).
    if ((size_t)(blocks_a(kAggR) + tgt) * groups > capacity) sh = {2, blocks_a(2), blocks_a(2) + tgt, 1};
    return sh;
}

// out64 != nullptr: int64 partial sums at out64 + g*pstride; else centred int32 at out32 + g*l*degree.
// vkL != nullptr: the verification target's int64 partial sums go to tout64 + g*tstride in the same launch.
// h_offsets != nullptr (ragged): aggregate g's signers are rows [h_offsets[g], h_offsets[g+1]) of the arrays, groups <=
// kFzRaggedMax, N = the largest group; sig == nullptr then means "verification targets only".  Tiled kernels only.
// sk_hat != nullptr (fused signing, one-pass kernel only): sig is the OUTPUT sig_out, c the signers' challenges (required).
int fz_launch_aggregate(fz_ctx *ctx, const int32_t *sig, const int32_t *alpha, int64_t *out64, size_t pstride,
                        int32_t *out32, size_t groups, size_t N, int l, const int32_t *vkL, const int32_t *vkR,
                        const int32_t *c, int64_t *tout64, size_t tstride, const size_t *h_offsets, const int32_t *sk_hat,
                        int32_t *sig_out) {
    if (groups == 0) return FZ_OK;
    const int d = ctx->degree;
    const uintptr_t align = (uintptr_t)sig | (uintptr_t)alpha | (uintptr_t)vkL | (uintptr_t)vkR | (uintptr_t)c | (uintptr_t)sk_hat | (uintptr_t)sig_out;
    const bool tiled = agg_tiled(d, align);
    if (sk_hat && !(tiled && !h_offsets && c && sig_out))
        return fz_set_error(FZ_E_UNSUPPORTED, "fused signing + aggregation: power-of-two degree <= 256, 16-byte aligned rows, equal-size aggregates");
    if (sk_hat) sig = sig_out;                        // "signatures present" for the tile arithmetic below
    if (h_offsets && !(tiled && groups <= (size_t)kFzRaggedMax))
        return fz_set_error(FZ_E_UNSUPPORTED, "ragged aggregation: power-of-two degree <= 256, 16-byte aligned rows, <= %d aggregates per launch", kFzRaggedMax);
    if (!tiled) {                                     // not a power of two, > 256, or unaligned rows
        const size_t total = (size_t)l * d + (vkL ? (size_t)d : 0);
        hipLaunchKernelGGL(aggregate_generic_kernel, dim3(grid_for(ctx, total), 1, (unsigned)groups), dim3(kBlock), 0, ctx->stream,
                           sig, alpha, vkL, vkR, c, N, l, d, out64, pstride, tout64, tstride, out32, ctx->mod);
        return fz_check_hip(hipGetLastError(), "aggregate (generic) launch");
    }
    const int d4 = d / 4;
    FzRagged rag;
    const FzRagged *rp = h_offsets ? &rag : nullptr;
    // Few signers in the whole launch: no signer slices, no shared accumulators (aggregate_direct).  Measured on cold
    // operands, both forms forced (profiles/r05_aggregate_direct_ab.txt; round 5, after the sliced kernel's streaming loads and
    // this kernel's exact wait counts): one aggregate of 8 / 32 / 96 signers 3.4 / 3.9 / 5.0 us against 4.6 / 4.8 / 5.2 us for
    // the sliced kernel, 128: 5.6 either way, 192 / 256: 6.7 / 8.0 against 6.3 / 7.8; two of 64: 5.6 against 5.8, two of
    // 128: 8.1 against 7.3 -- so up to 128 signers per launch (round 4: 256); with the verification target in the same
    // launch the sliced kernel leads throughout.  FZ_AGG_DIRECT = -1: never; 2 | 4: always, with that many rows per tile
    // (the tests force both forms through every output mode).
    const bool direct_auto = !vkL && groups * N <= 128;
    if (!sk_hat && d4 >= 16 && ctx->knob_agg_direct >= 0 && (ctx->knob_agg_direct > 0 || direct_auto) && groups <= 65535) {
        int R = ctx->knob_agg_direct;
        if (R != 2 && R != 4) R = groups <= 2 ? 2 : 4;          // rows of a tile share one alpha load; 168 / 84 tiles per aggregate at rank 83
        const int ncg = d4 / 16;
        const int ntile_a = sig ? ((l + R - 1) / R) * ncg : 0;
        const int ntile = ntile_a + (vkL ? ncg : 0);
        if (h_offsets) fill_ragged(rag, h_offsets, groups, 1);
        const dim3 grid((unsigned)ntile, (unsigned)groups);
        if (R == 4) launch_direct<16, 4, 3>(ctx, grid, sig, alpha, vkL, vkR, c, N, l, d4, ntile_a, out64, pstride, tout64, tstride, out32, rp);
        else launch_direct<16, 2, 5>(ctx, grid, sig, alpha, vkL, vkR, c, N, l, d4, ntile_a, out64, pstride, tout64, tstride, out32, rp);
        return fz_check_hip(hipGetLastError(), "aggregate (direct) launch");
    }
    const AggShape sh = onepass_shape((size_t)ctx->num_cu, (size_t)l * d4, sig != nullptr, vkL != nullptr, groups, N);
    const int ncb = sh.ncb;
    const size_t nsl = sh.nsl, pairs = groups * nsl;
    // the kernel divides tile numbers by ncb and nsl with 32-bit reciprocals: exact while tiles * divisor < 2^32
    if (pairs * (size_t)ncb > 0x3fffffffull || pairs * (size_t)ncb * (size_t)(ncb > (int)nsl ? ncb : (int)nsl) >= 0x100000000ull)
        return fz_set_error(FZ_E_UNSUPPORTED, "aggregate: grid too large (%zu aggregates x %zu slices x %d column blocks)", groups, nsl, ncb);
    unsigned long long *acc = nullptr;
    if (nsl > 1) {
        int rc = fz_agg_scratch(ctx, groups * (size_t)ncb, (size_t)kAggTile, &acc);       // (sized for the widest tile)
        if (rc != FZ_OK) return rc;
    }
    const unsigned grid = (unsigned)(8 * ((pairs * (size_t)ncb + 7) / 8));
    if (h_offsets) fill_ragged(rag, h_offsets, groups, nsl);
#define FZ_ONEPASS(AR_) launch_onepass<kAggWaves, AR_>(ctx, grid, sig, alpha, vkL, vkR, c, N, l, d4, sh.ncb_a, ncb, (int)nsl, (int)pairs, acc, out64, \
                                                        pstride, tout64, tstride, out32, rp, sk_hat, sig_out)
    if (sh.ar == 4) FZ_ONEPASS(4);
    else if (sh.ar == 3) FZ_ONEPASS(3);
    else FZ_ONEPASS(2);
#undef FZ_ONEPASS
    const int rc = fz_check_hip(hipGetLastError(), "aggregate launch");
    if (rc != FZ_OK && nsl > 1) ctx->agg_dirty = 1;              // accumulators / tickets may no longer be zero
    return rc;
}
