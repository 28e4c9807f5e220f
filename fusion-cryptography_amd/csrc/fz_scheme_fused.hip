// fz_scheme_fused.hip -- the scheme's fused kernels on the radix-4 passes of fz_ntt_dev.h, with their launchers: key generation
// (keygen_fused; keygen_bcast_fused) and verification (verify_fused, whose cross-workgroup protocol tests/test_isa_checks.py pins).
#include "fz_ntt_dev.h"
#include "../../include/fusion_hip.h"

namespace {
// ------------------------------------------------------------------------------------------
// Fused keygen arithmetic (fusion/fusion.py:363-370), one workgroup per (key, half): every secret row is
// transformed (radix-4 forward), written to sk_hat, and -- while still in registers -- multiplied by the
// matching row of the public challenge A and accumulated; the l partial products are reduced through LDS
// into the verification-key row.  sk_hat is never re-read: 342 KB of HBM traffic per key instead of 508 KB.
// ------------------------------------------------------------------------------------------
// IMAD: A[k] (.) y accumulates in 64-bit INTEGERS: A = hi * 2^16 + lo (hi = A >> 16, lo = A & 0xffff, two integer ops on the
// int32 row as it is loaded), then acc_hi += y * hi and acc_lo += y * lo are one v_mad_i64_i32 each -- |y * hi|, |y * lo| < 2^47,
// so 2^15 rows sum without overflow (fz_arith.h; the launcher falls back to the fp64 form beyond) and nothing is reduced inside the loop: 4 operations per coefficient instead of 8
// (conversion of A, the 6-op FMA-Barrett multiply, the accumulate).  The integer form of y is the value keygen stores anyway.
// (Measured and dropped: A pre-split into fp64 (hi, lo) pairs by the host -- two FMAs per coefficient, but 64 bytes of L2
// traffic per lane and row instead of 16: keygen 79 -> 109 us per 1024 keys, verify 256 -> 270 us per 8192 aggregates,
// profiles/r03_presplit_A_experiment.txt.)
// (fz_imad_total, the sums' way back to fp64, lives in fz_arith.h.)
// One row group per wave iteration, rows requested one iteration ahead, per-lane twiddles as (w, w * K/q) pairs: round 3 measured
// two row groups, a second iteration of prefetch and twiddles kept as w alone (five waves per SIMD) -- 81.7 / 81.7 / 82.0 / 81.1
// and 79.2 / 77.7 us per 1024 keys, all within 2 % (profiles/r03_keygen_ab.txt) -- and round 4 removed those instantiations.
// Round 5: the secret rows (read once) by streaming loads, sk_hat (never read here) by streaming stores: 81.3 -> 77.6 us alone,
// keygen + sign chained 119.4 -> 112.1 us per 1024 keys.  The `if`s around the next rows' request and around the store make the
// compiler's wait before the store a wait for ALL outstanding operations (one in-order counter); the form with exact wait
// counts (everything unconditional, rows clamped) is 4-5 % faster alone and 2-6 % SLOWER between two sign launches, the
// scheme's order -- measured on three boxes and dropped (profiles/r05_keygen_exact_waits_experiment.txt).
template <int LOGD, bool FAST, bool IMAD>
__global__ __launch_bounds__(64 * kWavesPerBlock) __attribute__((amdgpu_waves_per_eu(4, 6))) void keygen_fused(const int32_t *A, const int32_t *coef,
                                                                    size_t coef_seg_stride,
                                                                    size_t coef_row_stride, int32_t *sk_hat,
                                                                    int32_t *vk, int l, const double2 *__restrict__ tw2,
                                                                    FzTwA twA, FzMod m) {
    constexpr int NR = 1, PF = 1;
    using TW = double2;
    constexpr int D = 1 << LOGD, LP = D / 4, PPW = 64 / LP;
    __shared__ __attribute__((aligned(16))) double lds[kWavesPerBlock * 256 * (NR + 1)];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;      // the wave index is uniform: say so (scalar address arithmetic)
    const int p = lane / LP, mm = lane % LP;
    double *region = lds + wave * NR * 256 + p * D;
    double *accbuf = lds + kWavesPerBlock * NR * 256;
    const size_t seg = blockIdx.x;                      // (key, half)
    coef += seg * coef_seg_stride;                      // row stride 0: one secret polynomial per (key, half), as the
    sk_hat += seg * (size_t)l * D;                      // reference's seeded sampler produces (polynomials.py:436-467)

    TW twl[LOGD / 2 - 1][3];
    fwd4_load_twiddles<LOGD, TW>(twl, tw2, mm);

    double acc[4] = {0, 0, 0, 0};
    long long ihi[4] = {0, 0, 0, 0}, ilo[4] = {0, 0, 0, 0};      // IMAD: exact integer sums of y * hi and y * lo
    const int tasks = (l + PPW - 1) / PPW;
    constexpr int STEP = kWavesPerBlock * NR;           // a wave's iteration covers tasks t, t + 4, .. (NR of them)
    int xq[PF][NR][4];                                  // the next PF iterations' rows, in flight
    auto fetch = [&](int (&x)[NR][4], int task) {
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const int row = (task + r * kWavesPerBlock) * PPW + p;
            const int32_t *src = coef + (size_t)(row < l ? row : l - 1) * coef_row_stride + mm;
#pragma unroll
            for (int k = 0; k < 4; ++k) x[r][k] = __builtin_nontemporal_load(src + k * LP);
        }
    };
#pragma unroll
    for (int h = 0; h < PF; ++h)
        if (wave + h * STEP < tasks) fetch(xq[h], wave + h * STEP);
    for (int task0 = wave; task0 < tasks; task0 += PF * STEP) {
#pragma unroll
        for (int h = 0; h < PF; ++h) {
            const int task = task0 + h * STEP;
            if (task >= tasks) break;
            double a[NR][4];
            int4 ak[NR];
#pragma unroll
            for (int r = 0; r < NR; ++r) {
#pragma unroll
                for (int k = 0; k < 4; ++k) a[r][k] = (double)xq[h][r][k];
                const int row = (task + r * kWavesPerBlock) * PPW + p;
                ak[r] = *reinterpret_cast<const int4 *>(A + (size_t)(row < l ? row : l - 1) * D + 4 * mm);
            }
            if (task + PF * STEP < tasks) fetch(xq[h], task + PF * STEP);
            fwd4_passes_n<LOGD, FAST, NR, TW>(a, region, twl, twA, m, mm);
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const int row = (task + r * kWavesPerBlock) * PPW + p;
                const double y0 = fz_cent(a[r][0], m), y1 = fz_cent(a[r][1], m), y2 = fz_cent(a[r][2], m), y3 = fz_cent(a[r][3], m);
                if (row < l) {
                    const int4 yi = make_int4((int)y0, (int)y1, (int)y2, (int)y3);
                    nt_store4(sk_hat + (size_t)row * D + 4 * mm, yi);
                    if constexpr (IMAD) {
                        const int yv[4] = {yi.x, yi.y, yi.z, yi.w}, av[4] = {ak[r].x, ak[r].y, ak[r].z, ak[r].w};
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            ihi[k] += (long long)yv[k] * (long long)(av[k] >> 16);
                            ilo[k] += (long long)yv[k] * (long long)(av[k] & 0xffff);
                        }
                    } else {
                        acc[0] += fz_mulmod(y0, (double)ak[r].x, m);
                        acc[1] += fz_mulmod(y1, (double)ak[r].y, m);
                        acc[2] += fz_mulmod(y2, (double)ak[r].z, m);
                        acc[3] += fz_mulmod(y3, (double)ak[r].w, m);
                    }
                }
            }
            wave_sync();
        }
    }
    if constexpr (IMAD) {
        const bool small = tasks <= 32 * kWavesPerBlock;          // rows per wave <= 32
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = fz_imad_total(ihi[k], ilo[k], small, m);
    }
    double *mine = accbuf + wave * 256 + p * D + 4 * mm;
    mine[0] = acc[0]; mine[1] = acc[1]; mine[2] = acc[2]; mine[3] = acc[3];
    __syncthreads();
    if (threadIdx.x < D) {
        double sum = 0;
#pragma unroll
        for (int w = 0; w < kWavesPerBlock; ++w)
#pragma unroll
            for (int q = 0; q < PPW; ++q) sum += accbuf[w * 256 + q * D + threadIdx.x];
        vk[seg * D + threadIdx.x] = (int)fz_cent(sum, m);
    }
}

// The reference's SEEDED keygen samples every entry of a key half with the same seed (fusion.py:156-173): the l rows of a half
// are one polynomial, so their transforms are one transform.  fz_keygen_core_bcast (one polynomial per (key, half)) therefore
// transforms it ONCE per workgroup -- every wave for itself: a transform is cheaper than an exchange -- and the rest is the l
// stores of the row and the accumulation of A_k (.) y over k: a streaming kernel (85 KiB written per half, A from the L2)
// instead of l transforms.  Same results as the three launches other degrees take (rows expanded, transformed, multiplied by
// A: FZ_UNFUSED=1 runs them at these degrees too; tests/test_gpu_variants.py compares both with the oracle).
template <int LOGD, bool FAST>
__global__ __launch_bounds__(64 * kWavesPerBlock) void keygen_bcast_fused(const int32_t *A, const int32_t *coef, int32_t *sk_hat,
                                                                          int32_t *vk, int l, const double2 *__restrict__ tw2,
                                                                          FzTwA twA, FzMod m) {
    constexpr int D = 1 << LOGD, LP = D / 4, PPW = 64 / LP;
    __shared__ __attribute__((aligned(16))) double lds[kWavesPerBlock * 256 * 2];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int p = lane / LP, mm = lane % LP;
    double *region = lds + wave * 256 + p * D;
    double *accbuf = lds + kWavesPerBlock * 256;
    const size_t seg = blockIdx.x;                      // (key, half)
    coef += seg * (size_t)D;
    sk_hat += seg * (size_t)l * D;
    double2 twl[LOGD / 2 - 1][3];
    fwd4_load_twiddles<LOGD, double2>(twl, tw2, mm);
    double a[1][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) a[0][k] = (double)coef[mm + k * LP];
    fwd4_passes_n<LOGD, FAST, 1, double2>(a, region, twl, twA, m, mm);
    const int4 yi = make_int4((int)fz_cent(a[0][0], m), (int)fz_cent(a[0][1], m), (int)fz_cent(a[0][2], m), (int)fz_cent(a[0][3], m));
    const int yv[4] = {yi.x, yi.y, yi.z, yi.w};
    // sum_k A_k (.) y = (sum_k A_k) (.) y: the rows of A this lane's row slots cover, summed in integers (|A| <= 2^31, l <= 2^31
    // rows: no overflow of int64), one multiply at the end
    long long asum[4] = {0, 0, 0, 0};
    constexpr int U = 4;
    const int step = kWavesPerBlock * PPW;
    for (int row0 = wave * PPW + p; row0 < l; row0 += U * step) {
        int4 ak[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int row = row0 + u * step;
            ak[u] = *reinterpret_cast<const int4 *>(A + (size_t)(row < l ? row : l - 1) * D + 4 * mm);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int row = row0 + u * step;
            if (row < l) {
                nt_store4(sk_hat + (size_t)row * D + 4 * mm, yi);
                asum[0] += ak[u].x; asum[1] += ak[u].y; asum[2] += ak[u].z; asum[3] += ak[u].w;
            }
        }
    }
    double *mine = accbuf + wave * 256 + p * D + 4 * mm;
#pragma unroll
    for (int k = 0; k < 4; ++k) mine[k] = fz_mulmod(fz_cent_i64(asum[k], m), (double)yv[k], m);      // |.| <= q/2 + eps each
    __syncthreads();
    if (threadIdx.x < D) {
        double sum = 0;
#pragma unroll
        for (int w = 0; w < kWavesPerBlock; ++w)
#pragma unroll
            for (int q = 0; q < PPW; ++q) sum += accbuf[w * 256 + q * D + threadIdx.x];
        vk[seg * D + threadIdx.x] = (int)fz_cent(sum, m);
    }
}

// ------------------------------------------------------------------------------------------
// Fused verification (fusion/fusion.py:690-727): sigma is read ONCE.  While a row of sigma is in registers it
// feeds both (a) observed += A[k] (.) sigma[k] and (b) the radix-4 inverse transform, whose centred outputs are
// only reduced (max |x| per aggregate, weight per row) and never stored.  The l rows of one aggregate are spread
// over gridDim.x workgroups (a single aggregate -- the common call -- would otherwise occupy one CU): each
// adds its exact partial of `observed` into the aggregate's accumulator and counts itself (and its norm / weight
// failures) in the aggregate's state word; the workgroup that arrives last compares with the target, applies the
// reference's verdict order (target mismatch, norm, weight) and re-arms accumulator and state for the next launch.
// ------------------------------------------------------------------------------------------
constexpr int kVerifyWaves = 4;

// 4 consecutive stored values of a row, as loaded (the request is issued one row ahead of its use) and as doubles:
// int32 rows as they are (any int32), int64 rows -- exact partial sums straight from the cross-GPU all-reduce --
// centred on unpacking
template <typename T> struct Raw4;
template <> struct Raw4<int32_t> {
    int4 v;
    __device__ __forceinline__ void load(const int32_t *p) { v = nt_load4(p); }      // an aggregate's rows are read once
    __device__ __forceinline__ void unpack(double (&a)[4], const FzMod &) const {
        a[0] = (double)v.x; a[1] = (double)v.y; a[2] = (double)v.z; a[3] = (double)v.w;
    }
    __device__ __forceinline__ void ints(int (&s)[4], const double (&)[4]) const { s[0] = v.x; s[1] = v.y; s[2] = v.z; s[3] = v.w; }
};
template <> struct Raw4<int64_t> {
    longlong2 lo, hi;
    __device__ __forceinline__ void load(const int64_t *p) {
        lo = reinterpret_cast<const longlong2 *>(p)[0];
        hi = reinterpret_cast<const longlong2 *>(p)[1];
    }
    __device__ __forceinline__ void unpack(double (&a)[4], const FzMod &m) const {
        a[0] = fz_cent_i64(lo.x, m); a[1] = fz_cent_i64(lo.y, m);          // exact for any int64
        a[2] = fz_cent_i64(hi.x, m); a[3] = fz_cent_i64(hi.y, m);
    }
    __device__ __forceinline__ void ints(int (&s)[4], const double (&a)[4]) const {       // the centred values just unpacked
        s[0] = (int)a[0]; s[1] = (int)a[1]; s[2] = (int)a[2]; s[3] = (int)a[3];
    }
};
__device__ __forceinline__ int centred_any(int32_t v, const FzMod &) { return v; }
__device__ __forceinline__ int centred_any(int64_t v, const FzMod &m) { return (int)fz_cent_i64(v, m); }

// IMAD: A (.) sigma in 64-bit integer multiply-adds (see keygen_fused).  `lazy` (host-decided, uniform): beta < q/2 - q * 2^-12, so the norm
// test needs no centring at all -- the inverse transform's outputs r satisfy |r| <= q/2 + q * 2^-13; if |r| <= beta then r is
// already the centred residue and passes; if |r| > beta then |cent(r)| >= q - |r| >= q/2 - q * 2^-13 > beta (or cent(r) = r):
// max |r| > beta <=> max |cent(r)| > beta.  Likewise r == 0 (mod q) <=> r == 0, since |r| < q.  Saves 8 of ~180 ops per row.
//
// Target from the key (vk != nullptr, uniform; per-signature verification, fz_verify_signatures_async): the comparison's
// target is not read from `target` but formed here, cent(vkL (.) c + vkR), from the key rows [groups][2][D] and the
// challenges [groups][D] -- the one-time scheme's own equation, i.e. a single signer with alpha_hat == 1.  The three words a
// comparing thread needs are requested at kernel entry, so their latency hides under the row loop.  A run-time argument
// and not a template parameter: the 32 instantiations stay what tests/test_isa_checks.py pins, and both compare sites of
// the new form are in them.  Any int32 key and challenge: |vkL * c| < 2^62 (fz_mulmod), |. + vkR| < 2^32 (fz_cent).
template <int LOGD, bool FAST, typename T, bool ORDERED, bool IMAD>
__global__ __launch_bounds__(64 * kVerifyWaves) void verify_fused(const int32_t *A, const T *sig,
                                                                  size_t sig_stride,
                                                                  const T *target, size_t target_stride, int l, long long beta,
                                                                  long long omega, int lazy, const double2 *__restrict__ itw2,
                                                                  FzTwA twA, FzMod m, double *part, int *state, int *verdict,
                                                                  const int32_t *vk, const int32_t *chal) {
    constexpr int NR = 1;                 // one row group per wave iteration (two: 248.5 against 243.9 us per 8192 aggregates, round 3)
    using TW = double2;
    constexpr int D = 1 << LOGD, LP = D / 4, PPW = 64 / LP;
    static_assert(D <= 64 * kVerifyWaves, "one thread per coefficient in the combine steps");
    __shared__ __attribute__((aligned(16))) double lds[kVerifyWaves * 256 * (NR + 1)];
    __shared__ int s_flags, s_last;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;      // the wave index is uniform: say so (scalar address arithmetic)
    const int p = lane / LP, mm = lane % LP;
    double *region = lds + wave * NR * 256 + p * D;
    double *accbuf = lds + kVerifyWaves * NR * 256;
    if (threadIdx.x == 0) s_flags = 0;
    const int R = gridDim.x, r = blockIdx.x, g = blockIdx.y;
    sig += (size_t)g * sig_stride;
    target += (size_t)g * target_stride;
    part += (size_t)g * D;                          // [groups][D] exact fp64 sums of `observed`, zero between launches
    state += g;                                     // arrivals (bits 0-15), norm failures (16-23), weight failures (24-31)
    const bool keyed = vk != nullptr;
    __shared__ int s_tgt[D];                        // keyed: the target, formed before the row loop
    // the value a comparing thread (threadIdx.x < D) compares with, centred (s_tgt: written by this same thread)
    auto want = [&]() -> int { return keyed ? s_tgt[threadIdx.x] : centred_any(target[threadIdx.x], m); };

    TW twl[LOGD / 2 - 1][3];
    inv4_load_twiddles<LOGD, TW>(twl, itw2, mm);

    double acc[4] = {0, 0, 0, 0};
    double mx = 0.0;                                // max |centred output|, kept as a double: |.| <= q/2, exact
    int wfail = 0;
    const bool weigh = omega < (long long)D;        // a row has D coefficients: a bound of D or more cannot fail
    const unsigned long long gmask = LP == 64 ? ~0ull : (((1ull << (LP & 63)) - 1ull) << ((LP * p) & 63));
    const int tasks = (l + PPW - 1) / PPW, step = R * kVerifyWaves;
    // a wave's rows are a sequential chain: the next row (sigma from HBM, A from the L2) is requested before this row's
    // passes start -- unconditionally, clamped to the last task, so that no branch stands between request and use.  Without
    // it a workgroup per aggregate (many aggregates per launch) paid one memory latency per row: 24 % of the HBM peak.
    // NR row groups per iteration (tasks t, t + step, ..): they go through the inverse passes in lock step (inv4_passes_n)
    Raw4<T> rn[NR];
    int4 an[NR];
    auto fetch = [&](int t) {
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            const int row = (t + j * step) * PPW + p;
            const size_t off = (size_t)(row < l ? row : l - 1) * D + 4 * mm;
            an[j] = *reinterpret_cast<const int4 *>(A + off);
            rn[j].load(sig + off);
        }
    };
    long long ihi[4] = {0, 0, 0, 0}, ilo[4] = {0, 0, 0, 0};      // IMAD: exact integer sums of sigma * hi and sigma * lo
    int task = r * kVerifyWaves + wave;
    if (task < tasks) fetch(task);
    // keyed: the key and challenge words are requested right behind the first row, so the two latencies overlap (the row
    // loop waits for that row anyway); the target goes to LDS, not into a register held across the loop -- the other
    // forms' register count, hence occupancy, is what it was
    if (keyed && threadIdx.x < D) {
        const int32_t kL = vk[(size_t)g * 2 * D + threadIdx.x], kR = vk[(size_t)g * 2 * D + D + threadIdx.x];
        const int32_t kc = chal[(size_t)g * D + threadIdx.x];
        s_tgt[threadIdx.x] = (int)fz_cent(fz_mulmod((double)kL, (double)kc, m) + (double)kR, m);
    }
    for (; task < tasks; task += NR * step) {
        double a[NR][4];
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            const int row = (task + j * step) * PPW + p;
            const bool valid = row < l;
            const int4 ak = an[j];
            int si[4];
            rn[j].unpack(a[j], m);
            if constexpr (IMAD) rn[j].ints(si, a[j]);
            if (valid) {
                if constexpr (IMAD) {
                    const int av[4] = {ak.x, ak.y, ak.z, ak.w};
#pragma unroll
                    for (int k = 0; k < 4; ++k) {       // any int32 sigma, any int32 A: |sigma * hi|, |sigma * lo| < 2^47
                        ihi[k] += (long long)si[k] * (long long)(av[k] >> 16);
                        ilo[k] += (long long)si[k] * (long long)(av[k] & 0xffff);
                    }
                } else {
                    acc[0] += fz_mulmod(a[j][0], (double)ak.x, m);
                    acc[1] += fz_mulmod(a[j][1], (double)ak.y, m);
                    acc[2] += fz_mulmod(a[j][2], (double)ak.z, m);
                    acc[3] += fz_mulmod(a[j][3], (double)ak.w, m);
                }
            }
        }
        fetch(task + NR * step < tasks ? task + NR * step : tasks - 1);
        inv4_passes_n<LOGD, FAST, NR, TW>(a, region, twl, twA, m, mm);
        // norm and weight of the rows stay in the fp64 lanes (no conversions): a slot past the last row repeats row l - 1, which
        // changes neither the maximum nor any row's weight.  Weight = population count of "non-zero" ballots (scalar unit).
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            if (!lazy) {
#pragma unroll
                for (int k = 0; k < 4; ++k) a[j][k] = fz_cent(a[j][k], m);          // canonical: zero mod q <=> 0
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) mx = __builtin_fmax(mx, __builtin_fabs(a[j][k]));
            if (weigh) {
                int cnt = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) cnt += __popcll(__ballot(a[j][k] != 0.0) & gmask);
                if ((long long)cnt > omega) wfail = 1;
            }
        }
        wave_sync();      // the next rows' first-pass writes must not overtake these rows' last reads
    }
    if constexpr (IMAD) {
        const bool small = tasks <= 32 * step;                    // rows per wave <= 32
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = fz_imad_total(ihi[k], ilo[k], small, m);
    }
    // partial products of this wave, indexed by (row slot p, position)
    double *mine = accbuf + wave * 256 + p * D + 4 * mm;
    mine[0] = acc[0]; mine[1] = acc[1]; mine[2] = acc[2]; mine[3] = acc[3];
    if (mx > (double)beta) atomicOr(&s_flags, 2);       // mx < 2^31 and integer-valued; beta as a double rounds only above 2^53
    if (wfail) atomicOr(&s_flags, 4);
    __syncthreads();
    if (R == 1) {                                   // the whole aggregate is this workgroup's: nothing to share
        if (threadIdx.x < D) {
            double sum = 0;
            for (int w = 0; w < kVerifyWaves; ++w)
#pragma unroll
                for (int q = 0; q < PPW; ++q) sum += accbuf[w * 256 + q * D + threadIdx.x];
            if ((int)fz_cent_wide(sum, m) != want()) atomicOr(&s_flags, 1);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const int f = s_flags;
            verdict[g] = (f & 1) ? FZ_VERDICT_TARGET_MISMATCH : ((f & 2) ? FZ_VERDICT_NORM : ((f & 4) ? FZ_VERDICT_WEIGHT : FZ_VERDICT_OK));
        }
        return;
    }
    // Cross-workgroup combine WITHOUT device-scope fences (a __threadfence() is an L2 write-back on this chip: several
    // microseconds each, serialised over the workgroups).  Everything shared travels in device-scope atomics, which
    // are performed at the memory side: exact fp64 adds of integer partials (|.| < l * q < 2^53, order-independent),
    // then ONE integer add that counts the arrival and the norm / weight failures.  A returning atomic has been
    // performed when its result is back, so "data before arrival" needs no fence.
    if (threadIdx.x < D) {
        double sum = 0;
        for (int w = 0; w < kVerifyWaves; ++w)
#pragma unroll
            for (int q = 0; q < PPW; ++q) sum += accbuf[w * 256 + q * D + threadIdx.x];
        const double before = __hip_atomic_fetch_add(part + threadIdx.x, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        region[0] = before;                         // consume the result: the add is complete before the barrier below
    }
    // ... and say so to the hardware in so many words (inline asm: no compiler pass may drop or move it): every
    // add of this wave has been performed -- its old value is back -- before the wave reaches the barrier
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        const int f = s_flags;
        const unsigned inc = 1u + ((f & 2) ? (1u << 16) : 0u) + ((f & 4) ? (1u << 24) : 0u);
        // ORDERED (FZ_VERIFY_ORDERED=1): the arrival carries release/acquire semantics at agent scope as the HIP memory
        // model words it (one L2 write-back + L1 invalidate per workgroup).  The default relies on what the hardware
        // does with these operations: every shared word is ONLY ever touched by agent-scope atomics, which execute at
        // the memory side (MI355X_MICROARCH.md, "Global float atomics"), so no cache holds a copy that could be stale,
        // and the arrival cannot overtake the adds because they have returned (the wait above, the barrier).
        const unsigned old = __hip_atomic_fetch_add(reinterpret_cast<unsigned *>(state), inc,
                                                    ORDERED ? __ATOMIC_ACQ_REL : __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned now = old + inc;
        s_last = ((old & 0xffffu) == (unsigned)(R - 1));
        s_flags = (((now >> 16) & 0xffu) ? 2 : 0) | ((now >> 24) ? 4 : 0);
    }
    __syncthreads();
    if (!s_last) return;
    if (threadIdx.x < D) {                          // read and re-arm in one operation
        const double sum = __hip_atomic_exchange(part + threadIdx.x, 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((int)fz_cent_wide(sum, m) != want()) atomicOr(&s_flags, 1);   // both centred
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        __hip_atomic_exchange(reinterpret_cast<unsigned *>(state), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int f = s_flags;
        verdict[g] = (f & 1) ? FZ_VERDICT_TARGET_MISMATCH : ((f & 2) ? FZ_VERDICT_NORM : ((f & 4) ? FZ_VERDICT_WEIGHT : FZ_VERDICT_OK));
    }
}

}  // namespace

int fz_launch_keygen_fused(fz_ctx *ctx, const int32_t *A, const int32_t *coef, int32_t *sk_hat, int32_t *vk, size_t segments,
                           int l, bool broadcast) {
    const dim3 grid((unsigned)segments), block(64 * kWavesPerBlock);
    if (broadcast) {
        // one polynomial per (key, half): ONE transform per workgroup, then l stores (see keygen_bcast_fused); other degrees: the
        // caller's three launches
        if (ctx->logd != 6 && ctx->logd != 8) return fz_set_error(FZ_E_UNSUPPORTED, "one-polynomial keygen: degree 64 or 256 only");
        return fz_dispatch<6, 8>(ctx, FZ_E_UNSUPPORTED, [&](auto logd, auto fast) {
            hipLaunchKernelGGL((keygen_bcast_fused<logd(), fast()>), grid, block, 0, ctx->stream, A, coef, sk_hat, vk, l,
                               (const double2 *)ctx->d_tw2, ctx->twA, ctx->mod);
            return fz_check_hip(hipGetLastError(), "keygen_bcast_fused launch");
        });
    }
    if (ctx->logd != 6 && ctx->logd != 8) return fz_set_error(FZ_E_UNSUPPORTED, "fused keygen: degree 64 or 256 only");
    const size_t seg_stride = (size_t)l * ctx->degree, row_stride = (size_t)ctx->degree;
    // integer accumulation is exact for at most 2^15 products per lane (fz_arith.h): longer sums take the fp64 form
    const bool imad_k = !ctx->knob_no_imad && l <= (1 << 15);
    return fz_dispatch<6, 8>(ctx, FZ_E_UNSUPPORTED, [&](auto logd, auto fast) {
        constexpr int LOGD = logd();
        constexpr bool FAST = fast();
        auto launch = [&](auto imad) {
            hipLaunchKernelGGL((keygen_fused<LOGD, FAST, decltype(imad)::value>), grid, block, 0, ctx->stream, A, coef, seg_stride, row_stride,
                               sk_hat, vk, l, (const double2 *)ctx->d_tw2, ctx->twA, ctx->mod);
        };
        if (imad_k) launch(std::true_type()); else launch(std::false_type());
        return fz_check_hip(hipGetLastError(), "keygen_fused launch");
    });
}

template <typename T>
static int launch_verify_fused(fz_ctx *ctx, const int32_t *A, const T *sig, size_t sig_stride, const T *target,
                               size_t target_stride, size_t groups, int l, int64_t beta, int64_t omega, int *d_verdict,
                               const int32_t *vk = nullptr, const int32_t *chal = nullptr) {
    if (ctx->logd != 6 && ctx->logd != 8) return fz_set_error(FZ_E_UNSUPPORTED, "fused verify: degree 64 or 256 only");
    // about one row per wave while that leaves the chip under-filled (measured: one aggregate 22 us with one workgroup,
    // 4.5 us with 21; 64 aggregates 9.2 us with 4-8 workgroups each, 14.6 us with 22)
    const int ppw = 64 / (ctx->degree / 4), tasks = (l + ppw - 1) / ppw;
    int R = (tasks + kVerifyWaves - 1) / kVerifyWaves;
    const int fill = (int)((size_t)ctx->num_cu * 2 / groups);
    if (R > fill) R = fill;
    if (R < 1) R = 1;
    if (R > 64) R = 64;
    // the inverse passes leave |r| <= q/2 + q * 2^-13 (4-op multiply) -- see the kernel's header for why no centring is needed then
    const int lazy = (beta >= 0 && (double)beta < 0.5 * ctx->mod.q - ctx->mod.q / 4096.0 && !ctx->knob_verify_cent) ? 1 : 0;
    // (Round 3 also ran launches with a workgroup per aggregate through a 16-per-lane kernel, verify_many16: 245 us against 237
    // per 8192 aggregates at (83, 256), 130 against 119 at (195, 64) -- profiles/r03_verify_ab.txt -- although its transform
    // structure is 28-54 % faster from registers and LDS alone (profiles/r03_ntt_structures.txt): 149 VGPRs, 3 waves per SIMD
    // against 5.  Removed in round 4; tools/microbench/ntt_structures.hip keeps the structure comparison.)
    double *part = nullptr;
    int *state = nullptr;
    int rc = fz_verify_scratch(ctx, groups, (size_t)ctx->degree, &part, &state);
    if (rc != FZ_OK) return rc;
    const dim3 grid((unsigned)R, (unsigned)groups), block(64 * kVerifyWaves);
    // integer accumulation of A * sigma pays its once-per-wave conversion back only over several rows per wave (measured: 1.18 M
    // vector instructions against 1.10 M per launch when the l rows are spread one per wave over 21 workgroups)
    // ... and it is exact for at most 2^15 products per lane (fz_arith.h): a longer sum takes the fp64 form
    const bool imad = !ctx->knob_no_imad && l <= (1 << 15) && (tasks + R * kVerifyWaves - 1) / (R * kVerifyWaves) >= 4;
    fz_dispatch<6, 8>(ctx, FZ_OK, [&](auto logd, auto fast) {
        constexpr int LOGD = logd();
        constexpr bool FAST = fast();
        auto launch = [&](auto ordered, auto im) {
            hipLaunchKernelGGL((verify_fused<LOGD, FAST, T, decltype(ordered)::value, decltype(im)::value>), grid, block, 0, ctx->stream, A, sig,
                               sig_stride, target, target_stride, l, (long long)beta, (long long)omega, lazy, (const double2 *)ctx->d_itw2,
                               ctx->itwA, ctx->mod, part, state, d_verdict, vk, chal);
        };
        if (ctx->knob_verify_ordered) { if (imad) launch(std::true_type(), std::true_type()); else launch(std::true_type(), std::false_type()); }
        else { if (imad) launch(std::false_type(), std::true_type()); else launch(std::false_type(), std::false_type()); }
        return FZ_OK;
    });
    rc = fz_check_hip(hipGetLastError(), "verify_fused launch");
    if (rc != FZ_OK) ctx->verify_dirty = 1;          // the accumulators may be left non-zero: re-zeroed before the next launch
    return rc;
}

int fz_launch_verify_fused(fz_ctx *ctx, const int32_t *A, const int32_t *sig, const int32_t *target, size_t groups, int l,
                           int64_t beta, int64_t omega, int *d_verdict) {
    return launch_verify_fused<int32_t>(ctx, A, sig, (size_t)l * ctx->degree, target, (size_t)ctx->degree, groups, l, beta, omega,
                                        d_verdict);
}

// per-signature verification: signer g's target formed in the kernel from its key row vk [g][2][D] and challenge c [g][D]
// (verify_fused, "target from the key").  One launch per at most max-grid-y signers (blockIdx.y is the signer); the chunks
// share the verification scratch, which every launch re-arms, so they simply follow each other on the stream.
int fz_launch_verify_signatures(fz_ctx *ctx, const int32_t *A, const int32_t *sig, const int32_t *vk, const int32_t *c, size_t N,
                                int l, int64_t beta, int64_t omega, int *d_verdict) {
    int ymax = 0;
    int rc = fz_check_hip(hipDeviceGetAttribute(&ymax, hipDeviceAttributeMaxGridDimY, ctx->device), "max grid y");
    if (rc != FZ_OK) return rc;
    if (ymax < 1) return fz_set_error(FZ_E_HIP, "max grid y reported as %d", ymax);
    const size_t D = (size_t)ctx->degree, sig_stride = (size_t)l * D;
    for (size_t g0 = 0; g0 < N; g0 += (size_t)ymax) {
        const size_t n = N - g0 < (size_t)ymax ? N - g0 : (size_t)ymax;
        rc = launch_verify_fused<int32_t>(ctx, A, sig + g0 * sig_stride, sig_stride, nullptr, 0, n, l, beta, omega, d_verdict + g0,
                                          vk + g0 * 2 * D, c + g0 * D);
        if (rc != FZ_OK) return rc;
    }
    return FZ_OK;
}

// the aggregates and targets as int64 partial sums (e.g. straight after the all-reduce), group g at base + g * stride
int fz_launch_verify_fused_i64(fz_ctx *ctx, const int32_t *A, const int64_t *sig, size_t sig_stride, const int64_t *target,
                               size_t target_stride, size_t groups, int l, int64_t beta, int64_t omega, int *d_verdict) {
    return launch_verify_fused<int64_t>(ctx, A, sig, sig_stride, target, target_stride, groups, l, beta, omega, d_verdict);
}
