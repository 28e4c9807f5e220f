// fz_ntt.hip -- batched negacyclic NTT / INTT kernels for gfx950, their launchers and the launch-floor diagnostics.
//
// Computes exactly what cooley_tukey_ntt (algebra/ntt.py:216-291) and gentleman_sande_intt (algebra/ntt.py:294-377) compute for
// each row: natural order in / bit-reversed order out for the forward transform, the reverse for the inverse (including the
// n^{-1} scaling), every output the centred residue.  The butterflies are the Longa-Naehrig merged-twiddle butterflies of the
// reference; only the schedule differs.  The device code of both schedules is in fz_ntt_dev.h, which other units build on too.
//
// 16 per lane (degree D = 16*L, 32 <= D <= 256; tools/ntt_layout_model.py is the index model): ntt_fwd16 / ntt_inv16
//   * L lanes of a wave own one polynomial, 16 coefficients per lane, 64/L polynomials per wave = one 4 KiB chunk of the batch;
//     four waves per workgroup, each with a private LDS region (the one workgroup-wide barrier follows the staging of the
//     twiddle table; every other synchronisation is wave-local).
//   * strided pass: lane r holds x[r + L*k], k = 0..15.  The four stages with butterfly distance >= L pair registers of the same
//     lane, and their twiddles depend only on k: wave-uniform, scalar (SGPR) operands from the kernarg segment.
//   * one transpose through LDS (padded rows: conflict-free ds_write_b64 / ds_read_b128).
//   * contiguous pass: lane b holds x[16b .. 16b+15]; the remaining log2(D)-4 stages are again register-local.  Their twiddles
//     differ per lane: a [NE][L] table of (w, w * K/q) pairs staged in LDS.
//   * values are exact integers in fp64 with lazy accumulation (fz_arith.h): one multiply + add + sub per butterfly -- the 4-op
//     pseudo-Mersenne multiply where the modulus admits it (FAST; one fold in the inverse keeps its operands below 2^38), else
//     the 6-op FMA-Barrett form -- and one centring per output.
//   * a resident grid strides over the chunks in a software pipeline: the next chunk is requested straight into LDS
//     (global_load_lds_dwordx4, into the part of the wave's region the transpose has just left) half an iteration ahead, the wait
//     for it leaves the iteration's stores outstanding, and a wave's last chunk is peeled off so that no run-time branch
//     surrounds the request (fwd16_run).
// 4 per lane (radix-4 in place, degrees 64 and 256, small batches): ntt_fwd4 / ntt_inv4, one wave-task per wave, no loop.
// ntt_jobs4 / ntt_jobs16 / ntt_jobs16_keep serve a table of jobs with the same wave-tasks in ONE dispatch (fz_ntt_multi).
// D <= 16: a thread per polynomial (ntt_small); D = 512 .. 4096: a workgroup per polynomial through LDS (ntt_big).
#include "fz_ntt_dev.h"
#include "../../include/fusion_hip.h"
#include "../../include/fusion_hip_diag.h"
#include <hip/hip_ext.h>
#include <algorithm>

namespace {
template <int LOGD, bool FAST>
__global__ __launch_bounds__(64 * kWavesPerBlock) void ntt_fwd16(const int32_t *in, int32_t *out, size_t batch,
                                                                 const double2 *__restrict__ twB, FzTwA twA, FzMod m) {
    __shared__ __attribute__((aligned(16))) double lds[lds16_doubles<LOGD>()];
    fwd16_run<LOGD, FAST>(in, out, batch, blockIdx.x, gridDim.x, lds, twB, twA, m);
}

template <int LOGD, bool FAST>
__global__ __launch_bounds__(64 * kWavesPerBlock) void ntt_inv16(const int32_t *in, int32_t *out, size_t batch,
                                                                 const double2 *__restrict__ itwB, FzTwA twA, FzMod m) {
    __shared__ __attribute__((aligned(16))) double lds[lds16_doubles<LOGD>()];
    inv16_run<LOGD, FAST>(in, out, batch, blockIdx.x, gridDim.x, lds, itwB, twA, m);
}

template <int LOGD, bool FAST, int NR, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void ntt_fwd4(const int32_t *in, int32_t *out, size_t batch,
                                                       const double2 *__restrict__ tw2, FzTw4 twA, FzMod m) {
    constexpr int D = 1 << LOGD, LP = D / 4, PPW = 64 / LP;
    static_assert(LOGD % 2 == 0 && LOGD >= 6 && LOGD <= 8, "radix-4 kernel: degree 64 or 256");
    __shared__ __attribute__((aligned(16))) double lds[WAVES * NR * 256];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;      // the wave index is uniform: say so (scalar address arithmetic)
    const int p = lane / LP, mm = lane % LP;
    double *region = lds + wave * NR * 256 + p * D;
    const size_t task = (size_t)blockIdx.x * WAVES + wave;
    if (task * (NR * PPW) >= batch) return;
    fwd4_task<LOGD, FAST, NR>(in, out, batch, task * (NR * PPW) + p, region, mm, tw2, twA, m);      // row group r: polynomial poly0 + r * PPW
}

template <int LOGD, bool FAST, int NR, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void ntt_inv4(const int32_t *in, int32_t *out, size_t batch,
                                                       const double2 *__restrict__ itw2, FzTw4 twA, FzMod m) {
    constexpr int D = 1 << LOGD, LP = D / 4, PPW = 64 / LP;
    static_assert(LOGD % 2 == 0 && LOGD >= 6 && LOGD <= 8, "radix-4 kernel: degree 64 or 256");
    __shared__ __attribute__((aligned(16))) double lds[WAVES * NR * 256];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;      // the wave index is uniform: say so (scalar address arithmetic)
    const int p = lane / LP, mm = lane % LP;
    double *region = lds + wave * NR * 256 + p * D;
    const size_t task = (size_t)blockIdx.x * WAVES + wave;      // one task per wave: see ntt_fwd4
    if (task * (NR * PPW) >= batch) return;
    inv4_task<LOGD, FAST, NR>(in, out, batch, task * (NR * PPW) + p, region, mm, itw2, twA, m);
}

// ------------------------------------------------------------------------------------------
// Many independent transforms in ONE dispatch (fz_ntt_multi).  The reference issues its transforms one polynomial at a
// time (fusion/fusion.py:363-368: 2*rank per key; :690-692: rank per verification), and a launch of a few thousand rows
// sits on the dispatch floor (a 4096-row launch costs ~4 us of which ~2 are the empty dispatch).  Here a job table --
// (in, out, rows, direction) per job, in the kernarg segment -- is served by one grid of the SAME wave-tasks the one-job
// kernels above run: every job owns a run of workgroups (J.end[j] = workgroups up to and including job j), a workgroup finds
// its job by a scalar scan of at most 32 entries and then is a workgroup of ntt_fwd4 or ntt_inv4 (the direction is uniform
// per workgroup: one twiddle set in registers, as there).  Round 4: this replaced the persistent one-wave-per-workgroup
// kernel of rounds 2-3 (ntt_multi4), which cost 6.9 us for two jobs of 4096 rows where ONE job of 8192 rows costs 5.55
// (profiles/r03_ntt_small_batches.txt) -- a forward job and an inverse job of 4096 rows in one launch is the software-pipelined
// form of BASELINE configs[1]'s step (forward of batch i+1 beside the inverse of batch i), so that gap was the headline's.
// ------------------------------------------------------------------------------------------
// which job a workgroup belongs to: first / last = the run of workgroups [first, last) the job owns, rw = its rows (bit 31:
// inverse), in / out its buffers
template <typename JT>
__device__ __forceinline__ void pick_job(const JT &J, const unsigned b, unsigned &first, unsigned &last, unsigned &rw,
                                         const int32_t *&in, int32_t *&out) {
    constexpr int NJ = JT::kJobs;
    first = 0;
    if constexpr (NJ <= 8) {
        // The job WITHOUT a dependent load: every table entry is requested together with everything else the workgroup
        // reads from the kernel arguments and the job is picked by scalar selects (a scan would be a chain of scalar-load
        // round trips in front of the first data load: one job through a scanning kernel cost 5.0 us against 4.2 for
        // ntt_fwd4; round 4 did this for four entries and scanned from the fifth on, round 5's headline launch has eight).
        // Entries past the last job hold the launch's total, so they are never chosen.
        unsigned e[NJ], r[NJ];
        const int32_t *ip[NJ];
        int32_t *op[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            e[j] = J.end[j]; r[j] = J.rows[j]; ip[j] = J.in[j]; op[j] = J.out[j];
            // (opaque to the optimiser: it would otherwise turn the selects below into branches that load only the chosen
            // entry -- the dependent load this path exists to avoid)
            asm volatile("" : "+s"(e[j]), "+s"(r[j]), "+s"(ip[j]), "+s"(op[j]));
        }
        rw = r[0]; in = ip[0]; out = op[0]; last = e[0];
#pragma unroll
        for (int j = 1; j < NJ; ++j) {
            const bool g = b >= e[j - 1];                               // (ends never decrease: the last true one wins)
            first = g ? e[j - 1] : first;
            last = g ? e[j] : last;
            rw = g ? r[j] : rw;
            in = g ? ip[j] : in;
            out = g ? op[j] : out;
        }
    } else {
        // Larger tables would not fit the scalar registers (32 entries = 192 of them): the workgroup counts of ALL jobs come
        // with the first request (32 dwords), the job's index is found by scalar compares, and its three other entries are
        // ONE dependent round of scalar loads -- instead of a scan's one round trip per job passed.
        unsigned mask = 0;
#pragma unroll
        for (int k = 0; k < NJ - 1; ++k) {
            const unsigned ek = J.end[k];
            const bool g = b >= ek;
            first = g ? ek : first;                                     // (ends never decrease: the last true one wins)
            mask |= g ? (1u << k) : 0u;
        }
        const unsigned j = __builtin_amdgcn_readfirstlane(__builtin_popcount(mask));
        rw = J.rows[j]; in = J.in[j]; out = J.out[j]; last = J.end[j];
    }
}

// JT: FzJobsN<4 | 8 | 32> -- the table of a launch of at most that many jobs (24 bytes of kernel arguments per entry).
// `stamp` (diagnostics, NULL otherwise): one {entry, exit} pair of the 100 MHz reference counter per WORKGROUP, written by
// the workgroup's first wave after its stores have left (fz_diag_stamps_*): the chip's own record of when a launch ran,
// which no profiler serialises.  (ntt_jobs16 and ntt_jobs16_keep repeat this frame in so many words: docs/HISTORY.md, G.)
template <int LOGD, bool FAST, int NR, int WAVES, typename JT>
__global__ __launch_bounds__(64 * WAVES) void ntt_jobs4(JT J, const double2 *__restrict__ tw2, const double2 *__restrict__ itw2,
                                                        FzTw4 twA, FzTw4 itwA, FzMod m, unsigned long long *stamp) {
    constexpr int D = 1 << LOGD, LP = D / 4, PPW = 64 / LP, NJ = JT::kJobs;
    __shared__ __attribute__((aligned(16))) double lds[WAVES * NR * 256];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int p = lane / LP, mm = lane % LP;
    double *region = lds + wave * NR * 256 + p * D;
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();   // (unconditional: a branch on `stamp` here would put a scalar-load round trip in front of everything else)
    unsigned first, last, rw;
    const int32_t *in;
    int32_t *out;
    pick_job(J, blockIdx.x, first, last, rw, in, out);
    const size_t rows = rw & 0x7fffffffu;
    const bool inverse = (rw >> 31) != 0;
    const size_t task = (size_t)(blockIdx.x - first) * WAVES + wave;
    if (task * (NR * PPW) >= rows) return;                              // (never a workgroup's first wave: the grid is cut to whole tasks)
    if (inverse) inv4_task<LOGD, FAST, NR>(in, out, rows, task * (NR * PPW) + p, region, mm, itw2, itwA, m);
    else fwd4_task<LOGD, FAST, NR>(in, out, rows, task * (NR * PPW) + p, region, mm, tw2, twA, m);
    if (stamp && wave == 0) {
        __builtin_amdgcn_s_waitcnt(0);                                  // this wave's stores have been acknowledged
        const unsigned long long t1 = __builtin_amdgcn_s_memrealtime();
        if (lane == 0) {
            stamp[2 * (size_t)blockIdx.x] = t0;
            stamp[2 * (size_t)blockIdx.x + 1] = t1;
        }
    }
}

// The same job table served by the 16-per-lane kernels (round 5): a launch of 24 576 rows and more (fz_ctx::small_batch_rows)
// -- the headline's sixteen forward + sixteen inverse batches of 4096 -- is past the point where the radix-4 wave-tasks lead
// (one job: 25.5 us against 30 us at 65 536 rows; eight jobs of 4096: 15.9 us against 17.2).  A job owns a run of workgroups;
// the run IS a grid of ntt_fwd16 or ntt_inv16 over the job's batch (resident workgroups striding over 4 KiB chunks, next
// chunk prefetched into registers), sized by the launcher in proportion to the job's share of the launch.
template <int LOGD, bool FAST, typename JT>
__global__ __launch_bounds__(64 * kWavesPerBlock) void ntt_jobs16(JT J, const double2 *__restrict__ twB, const double2 *__restrict__ itwB,
                                                                  FzTwA twA, FzTwA itwA, FzMod m, unsigned long long *stamp) {
    __shared__ __attribute__((aligned(16))) double lds[lds16_doubles<LOGD>()];
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    unsigned first, last, rw;
    const int32_t *in;
    int32_t *out;
    pick_job(J, blockIdx.x, first, last, rw, in, out);
    const size_t rows = rw & 0x7fffffffu;
    if ((rw >> 31) != 0) inv16_run<LOGD, FAST>(in, out, rows, blockIdx.x - first, last - first, lds, itwB, itwA, m);
    else fwd16_run<LOGD, FAST>(in, out, rows, blockIdx.x - first, last - first, lds, twB, twA, m);
    if (stamp && threadIdx.x < 64) {                                    // fz_diag_stamps_*: see ntt_jobs4
        __builtin_amdgcn_s_waitcnt(0);
        const unsigned long long t1 = __builtin_amdgcn_s_memrealtime();
        if (threadIdx.x == 0) {
            stamp[2 * (size_t)blockIdx.x] = t0;
            stamp[2 * (size_t)blockIdx.x + 1] = t1;
        }
    }
}

// ntt_jobs16 for a launch whose outputs of ONE direction are the stream's next launch's inputs (fz_multi_plan): KEEP = 1, the
// forward jobs store normally instead of streaming so that their lines stay in the caches, KEEP = 2, the inverse jobs do.  A
// kernel of its own with two job bodies, like ntt_jobs16 (which is untouched: tables without consumers run exactly what they
// ran before): one kernel holding both store kinds of both bodies, chosen by a flag in the table, ran 2 % slower on EVERY path,
// and a wave-uniform run-time branch around the stores 2.5 % (profiles/r08_multi_order_ab.txt).
template <int LOGD, bool FAST, typename JT, int KEEP>
__global__ __launch_bounds__(64 * kWavesPerBlock) void ntt_jobs16_keep(JT J, const double2 *__restrict__ twB, const double2 *__restrict__ itwB,
                                                                       FzTwA twA, FzTwA itwA, FzMod m, unsigned long long *stamp) {
    __shared__ __attribute__((aligned(16))) double lds[lds16_doubles<LOGD>()];
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    unsigned first, last, rw;
    const int32_t *in;
    int32_t *out;
    pick_job(J, blockIdx.x, first, last, rw, in, out);
    const size_t rows = rw & 0x7fffffffu;
    if ((rw >> 31) != 0) inv16_run<LOGD, FAST, KEEP == 2>(in, out, rows, blockIdx.x - first, last - first, lds, itwB, itwA, m);
    else fwd16_run<LOGD, FAST, KEEP == 1>(in, out, rows, blockIdx.x - first, last - first, lds, twB, twA, m);
    if (stamp && threadIdx.x < 64) {                                    // fz_diag_stamps_*: see ntt_jobs4
        __builtin_amdgcn_s_waitcnt(0);
        const unsigned long long t1 = __builtin_amdgcn_s_memrealtime();
        if (threadIdx.x == 0) {
            stamp[2 * (size_t)blockIdx.x] = t0;
            stamp[2 * (size_t)blockIdx.x + 1] = t1;
        }
    }
}

// ------------------------------------------------------------------------------------------
// D <= 16: one thread per polynomial, everything in registers, twiddles uniform
// ------------------------------------------------------------------------------------------
template <int LOGD, bool INVERSE>
__global__ __launch_bounds__(256) void ntt_small(const int32_t *in, int32_t *out, size_t batch,
                                                 FzTwA twA, FzMod m) {
    constexpr int D = 1 << LOGD;
    const size_t poly = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (poly >= batch) return;
    double a[D];
#pragma unroll
    for (int k = 0; k < D; ++k) a[k] = (double)in[poly * D + k];
    if (!INVERSE) {
#pragma unroll
        for (int s = 0; s < LOGD; ++s) {
            const int t = D >> (s + 1);
#pragma unroll
            for (int k = 0; k < D; ++k) {
                if (k & t) continue;
                const double w = twA.w[(1 << s) + (k / (2 * t))];
                const double v = fz_mulmod(a[k + t], w, m);
                const double u = a[k];
                a[k] = u + v;
                a[k + t] = u - v;
            }
        }
    } else {
#pragma unroll
        for (int s = 0; s < LOGD; ++s) {
            const int t = 1 << s;
            const int h = D >> (s + 1);
#pragma unroll
            for (int k = 0; k < D; ++k) {
                if (k & t) continue;
                const double w = twA.w[h + (k / (2 * t))];
                const double u = a[k], v = a[k + t];
                a[k] = u + v;
                a[k + t] = fz_mulmod(u - v, w, m);
            }
        }
#pragma unroll
        for (int k = 0; k < D; ++k) a[k] = fz_mulmod(a[k], twA.n_inv, m);
    }
#pragma unroll
    for (int k = 0; k < D; ++k) out[poly * D + k] = (int)fz_cent(a[k], m);
}

// ------------------------------------------------------------------------------------------
// D = 512 .. 4096 (round 5): one workgroup per polynomial, the polynomial in LDS as doubles, one workgroup barrier per stage,
// twiddles from the device table.  The reference transforms any power-of-two length over any odd prime with a 2n-th root
// (algebra/ntt.py:239-270); the scheme's own degrees (64, 256) never come here -- this is generality, not a hot path.
// Forward: lazy sums (a value grows by at most q/2 per stage: 12 stages stay below 2^35).  Inverse: u + v doubles per
// stage, so it is folded below q at every stage (fz_fold: 2 operations) and u - v stays inside fz_mulmod's bound.
// ------------------------------------------------------------------------------------------
template <bool INVERSE>
__global__ __launch_bounds__(256) void ntt_big(const int32_t *in, int32_t *out, size_t batch, int logd, const double *__restrict__ tw,
                                               FzMod m, double n_inv) {
    extern __shared__ double big_a[];
    const int d = 1 << logd, half = d >> 1, tid = threadIdx.x;
    for (size_t poly = blockIdx.x; poly < batch; poly += gridDim.x) {
        for (int i = tid; i < d; i += 256) big_a[i] = (double)in[poly * d + i];
        __syncthreads();
        if (!INVERSE) {
            for (int mm = 1, t = half; mm < d; mm <<= 1, t >>= 1) {            // ntt.py:274-290
                for (int b = tid; b < half; b += 256) {
                    const int i = b / t, j = 2 * i * t + (b - i * t);
                    const double v = fz_mulmod(big_a[j + t], tw[mm + i], m), u = big_a[j];
                    big_a[j] = u + v;
                    big_a[j + t] = u - v;
                }
                __syncthreads();
            }
            for (int i = tid; i < d; i += 256) out[poly * d + i] = (int)fz_cent(big_a[i], m);
        } else {
            for (int h = half, t = 1; h >= 1; h >>= 1, t <<= 1) {               // ntt.py:354-372
                for (int b = tid; b < half; b += 256) {
                    const int i = b / t, j = 2 * i * t + (b - i * t);
                    const double u = big_a[j], v = big_a[j + t];
                    big_a[j] = fz_fold(u + v, m);
                    big_a[j + t] = fz_mulmod(u - v, tw[h + i], m);
                }
                __syncthreads();
            }
            for (int i = tid; i < d; i += 256) out[poly * d + i] = (int)fz_cent(fz_mulmod(big_a[i], n_inv, m), m);      // ntt.py:373-376
        }
        __syncthreads();                                                         // (the next polynomial reuses the array)
    }
}

int launch_big(fz_ctx *ctx, const int32_t *in, int32_t *out, size_t batch, bool inverse) {
    const size_t lds = sizeof(double) << ctx->logd;
    const size_t cap = (size_t)ctx->num_cu * 8;
    const unsigned grid = (unsigned)(batch < cap ? batch : cap);
    if (!inverse)
        hipLaunchKernelGGL((ntt_big<false>), dim3(grid), dim3(256), lds, ctx->stream, in, out, batch, ctx->logd, (const double *)ctx->d_tw, ctx->mod, 0.0);
    else
        hipLaunchKernelGGL((ntt_big<true>), dim3(grid), dim3(256), lds, ctx->stream, in, out, batch, ctx->logd, (const double *)ctx->d_itw, ctx->mod,
                           ctx->itwA.n_inv);
    return fz_check_hip(hipGetLastError(), "ntt_big launch");
}

// the event pair that times this dispatch itself (fz_profile_begin/end; hipExtLaunchKernelGGL binds it to the kernel) when profiling
// is on and it is this dispatch's turn, else none.  kind: 0 forward, 1 inverse, 2 multi-job (takes its turns with the forward: prof_seen[0])
struct ProfEvents { hipEvent_t e0 = nullptr, e1 = nullptr; };
ProfEvents prof_events(fz_ctx *ctx, int kind) {
    ProfEvents ev;
    if (ctx->prof_on && ctx->prof_n < ctx->prof_cap && (ctx->prof_seen[kind == 1 ? 1 : 0]++ % ctx->prof_every) == 0) {
        ev.e0 = ctx->prof_ev[2 * ctx->prof_n];
        ev.e1 = ctx->prof_ev[2 * ctx->prof_n + 1];
        ctx->prof_kind[ctx->prof_n++] = (unsigned char)kind;
    }
    return ev;
}

template <int LOGD, bool FAST>
int launch16f(fz_ctx *ctx, const int32_t *in, int32_t *out, size_t batch, bool inverse) {
    const size_t tasks = (batch * Geom<LOGD>::D + kChunk - 1) / kChunk;
    const size_t blocks = (tasks + kWavesPerBlock - 1) / kWavesPerBlock;
    const size_t cap = (size_t)(inverse ? ctx->grid_inv : ctx->grid_fwd);
    const unsigned grid = (unsigned)(blocks < cap ? blocks : cap);
    const ProfEvents ev = prof_events(ctx, inverse ? 1 : 0);
    const dim3 block(64 * kWavesPerBlock);
    if (!inverse)
        hipExtLaunchKernelGGL((ntt_fwd16<LOGD, FAST>), dim3(grid), block, 0, ctx->stream, ev.e0, ev.e1, 0, in, out, batch,
                              (const double2 *)ctx->d_twB, ctx->twA, ctx->mod);
    else
        hipExtLaunchKernelGGL((ntt_inv16<LOGD, FAST>), dim3(grid), block, 0, ctx->stream, ev.e0, ev.e1, 0, in, out, batch,
                              (const double2 *)ctx->d_itwB, ctx->itwA, ctx->mod);
    return fz_check_hip(hipGetLastError(), "ntt16 launch");
}

// The launch shape of the radix-4 wave-tasks, one job or many, by `waves1`, the launch's waves at one row group per wave.
// Rows per wave: enough waves to fill the chip first (about four per SIMD), then more rows per wave (FZ_NTT_ROWS forces a
// count: the tests run every one at small sizes).  Waves per workgroup at one row per wave: 8 once that still leaves a workgroup
// for every CU (fewer, fatter workgroups are handed out sooner), else 4, else 1 -- 4096 rows of degree 64 are 1024 waves: as 128
// workgroups they would leave half the chip idle; at 2 or 4 rows per wave, 2 (4 or 8 waves per workgroup: 6.11 / 6.04 us against
// 5.99 for the two-job launch).  f(rows per wave, waves per workgroup) as std::integral_constants.
template <class F>
void with_shape4(const fz_ctx *ctx, size_t waves1, F &&f) {
    using std::integral_constant;
    int nr = ctx->knob_ntt_rows;
    if (nr != 1 && nr != 2 && nr != 4) nr = waves1 <= (size_t)24 * ctx->num_cu ? 1 : (waves1 <= (size_t)48 * ctx->num_cu ? 2 : 4);
    if (nr == 4) f(integral_constant<int, 4>(), integral_constant<int, 2>());
    else if (nr == 2) f(integral_constant<int, 2>(), integral_constant<int, 2>());
    else if (waves1 >= (size_t)8 * ctx->num_cu) f(integral_constant<int, 1>(), integral_constant<int, 8>());
    else if (waves1 >= (size_t)4 * ctx->num_cu) f(integral_constant<int, 1>(), integral_constant<int, 4>());
    else f(integral_constant<int, 1>(), integral_constant<int, 1>());
}

template <int LOGD, bool FAST>
int launch4f(fz_ctx *ctx, const int32_t *in, int32_t *out, size_t batch, bool inverse) {
    constexpr int PPW = 64 / ((1 << LOGD) / 4);
    const size_t waves1 = (batch + PPW - 1) / PPW;                   // waves at one row group per wave
    if (waves1 > 0x7fffffffull) return fz_set_error(FZ_E_UNSUPPORTED, "batch too large for the radix-4 schedule");
    const ProfEvents ev = prof_events(ctx, inverse ? 1 : 0);
    with_shape4(ctx, waves1, [&](auto nr, auto waves) {
        constexpr int NR = nr(), WAVES = waves();
        const size_t tasks = (batch + (size_t)NR * PPW - 1) / ((size_t)NR * PPW);
        const dim3 grid((unsigned)((tasks + WAVES - 1) / WAVES)), block(64 * WAVES);
        if (!inverse)
            hipExtLaunchKernelGGL((ntt_fwd4<LOGD, FAST, NR, WAVES>), grid, block, 0, ctx->stream, ev.e0, ev.e1, 0, in, out, batch,
                                  (const double2 *)ctx->d_tw2, fz_tw4(ctx->twA), ctx->mod);
        else
            hipExtLaunchKernelGGL((ntt_inv4<LOGD, FAST, NR, WAVES>), grid, block, 0, ctx->stream, ev.e0, ev.e1, 0, in, out, batch,
                                  (const double2 *)ctx->d_itw2, fz_tw4(ctx->itwA), ctx->mod);
    });
    return fz_check_hip(hipGetLastError(), "ntt4 launch");
}

int launch16(fz_ctx *ctx, const int32_t *in, int32_t *out, size_t batch, bool inverse) {
    return fz_dispatch<5, 6, 7, 8>(ctx, FZ_E_UNSUPPORTED, [&](auto logd, auto fast) {
        if constexpr (logd() == 6 || logd() == 8) {
            // schedule choice: the radix-4 kernel below `small_batch_rows` rows (latency-bound regime)
            const bool small = ctx->force_kernel == 4 || (ctx->force_kernel == 0 && batch < (size_t)ctx->small_batch_rows);
            if (small) return launch4f<logd(), fast()>(ctx, in, out, batch, inverse);
        }
        return launch16f<logd(), fast()>(ctx, in, out, batch, inverse);
    });
}

template <int LOGD>
int launch_small(fz_ctx *ctx, const int32_t *in, int32_t *out, size_t batch, bool inverse) {
    const unsigned grid = (unsigned)((batch + 255) / 256);
    if (!inverse)
        hipLaunchKernelGGL((ntt_small<LOGD, false>), dim3(grid), dim3(256), 0, ctx->stream, in, out, batch,
                           ctx->twA, ctx->mod);
    else
        hipLaunchKernelGGL((ntt_small<LOGD, true>), dim3(grid), dim3(256), 0, ctx->stream, in, out, batch,
                           ctx->itwA, ctx->mod);
    return fz_check_hip(hipGetLastError(), "ntt_small launch");
}

}  // namespace

int fz_ntt_query_grid(fz_ctx *ctx) {
    if (ctx->logd < 5 || ctx->logd > 8) { ctx->grid_fwd = ctx->grid_inv = 0; return FZ_OK; }
    int fwd = 0, inv = 0;
    const int rc = fz_dispatch<5, 6, 7, 8>(ctx, FZ_OK, [&](auto logd, auto fast) {
        const int rf = fz_resident_grid(ctx, ntt_fwd16<logd(), fast()>, 64 * kWavesPerBlock, "occupancy query (fwd)", &fwd);
        return rf != FZ_OK ? rf : fz_resident_grid(ctx, ntt_inv16<logd(), fast()>, 64 * kWavesPerBlock, "occupancy query (inv)", &inv);
    });
    if (rc == FZ_OK) { ctx->grid_fwd = fwd; ctx->grid_inv = inv; }       // both or neither
    return rc;
}

int fz_launch_ntt(fz_ctx *ctx, const int32_t *d_in, int32_t *d_out, size_t batch, bool inverse) {
    if (ctx->logd < 0) return fz_set_error(FZ_E_UNSUPPORTED, "ring-only context (created with root 0) has no transforms");
    if (batch == 0) return FZ_OK;
    if ((((uintptr_t)d_in | (uintptr_t)d_out) & 15) != 0 && ctx->logd >= 2)
        return fz_set_error(FZ_E_BADARG, "transform buffers must be 16-byte aligned");
    switch (ctx->logd) {
        case 1: return launch_small<1>(ctx, d_in, d_out, batch, inverse);
        case 2: return launch_small<2>(ctx, d_in, d_out, batch, inverse);
        case 3: return launch_small<3>(ctx, d_in, d_out, batch, inverse);
        case 4: return launch_small<4>(ctx, d_in, d_out, batch, inverse);
        case 5: case 6: case 7: case 8: return launch16(ctx, d_in, d_out, batch, inverse);
        case 9: case 10: case 11: case 12: return launch_big(ctx, d_in, d_out, batch, inverse);
        default: return fz_set_error(FZ_E_UNSUPPORTED, "degree %d not supported (2..%d)", ctx->degree, kFzMaxDegree);
    }
}

// fz_diag_stamps_*: a launch's workgroups get a run of {entry, exit} slots (NULL: stamps off, or the recording is full)
static unsigned long long *stamp_slots(fz_ctx *ctx, unsigned total) {
    if (!ctx->stamp_on || !ctx->area[FZ_A_STAMP].p || ctx->stamp_n >= ctx->stamp_launch_cap || ctx->stamp_used + total > ctx->stamp_wg_cap) return nullptr;
    unsigned long long *stamp = (unsigned long long *)ctx->area[FZ_A_STAMP].p + 2 * ctx->stamp_used;
    ctx->stamp_first[ctx->stamp_n] = ctx->stamp_used;
    ctx->stamp_count[ctx->stamp_n++] = total;
    ctx->stamp_used += total;
    return stamp;
}

// the table as the kernels take it: f(FzJobsN<4 | 8 | 32>), the smallest that holds the launch's jobs (the caller fills the rest: pick_job)
template <class F>
static void with_jobs_table(const FzMultiJobs &J, F &&f) {
    auto table = [&](auto nj) {
        FzJobsN<nj()> S;
        for (int j = 0; j < nj(); ++j) { S.in[j] = J.in[j]; S.out[j] = J.out[j]; S.end[j] = J.end[j]; S.rows[j] = J.rows[j]; }
        return S;
    };
    if (J.n <= 4) f(table(std::integral_constant<int, 4>()));
    else if (J.n <= 8) f(table(std::integral_constant<int, 8>()));
    else f(table(std::integral_constant<int, kFzMultiMax>()));
}

// one radix-4 launch over a job table (at most kFzMultiMax jobs, degree 64 / 256)
template <int LOGD, bool FAST, int NR, int WAVES>
static void launch_jobs(fz_ctx *ctx, FzMultiJobs &J, hipEvent_t e0, hipEvent_t e1) {
    constexpr unsigned PPW = 64 / ((1 << LOGD) / 4);
    unsigned total = 0;
    for (int j = 0; j < J.n; ++j) {
        const unsigned rows = J.rows[j] & 0x7fffffffu;
        const unsigned tasks = (rows + NR * PPW - 1) / (NR * PPW);
        total += (tasks + WAVES - 1) / WAVES;
        J.end[j] = total;
    }
    for (int j = J.n; j < kFzMultiMax; ++j) { J.end[j] = total; J.rows[j] = 0; J.in[j] = nullptr; J.out[j] = nullptr; }   // (never chosen: see the kernel)
    unsigned long long *stamp = stamp_slots(ctx, total);
    with_jobs_table(J, [&](auto S) {
        hipExtLaunchKernelGGL((ntt_jobs4<LOGD, FAST, NR, WAVES, decltype(S)>), dim3(total), dim3(64 * WAVES), 0, ctx->stream, e0, e1, 0, S,
                              (const double2 *)ctx->d_tw2, (const double2 *)ctx->d_itw2, fz_tw4(ctx->twA), fz_tw4(ctx->itwA), ctx->mod, stamp);
    });
}

// The layout of a 16-per-lane multi-job launch (host only; fz_diag_multi_order shows it to the tests).
// A launch that transforms what the context's previous multi-job launch wrote (the software-pipelined step: forward of the next
// batches beside the inverse of the last ones) re-reads those bytes one launch later.  Workgroups take their slots in blockIdx
// order -- with two chains in flight a launch's workgroups enter over half its duration -- so the jobs' runs of workgroups are laid
// out in the order the launch should do its work: first the CONSUMERS, the jobs whose input is an output of the previous launch
// (rows <= the rows written), the most recently written first, then the other jobs in table order: what this launch writes for the
// next one is written last and read first.  In such a launch the other jobs are taken for producers of the next launch and, when
// they all have one direction and no consumer shares it, store normally (ntt_jobs16_keep) so that their lines stay in the
// caches; consumers, and every job of a table without consumers, keep the streaming stores, and such a table its table order and
// the very kernel of rounds 5-6.  Workgroups per job are unchanged:
// min(its workgroups, its share of the resident grid); more, shorter-lived generations of workgroups sharpen the order and cost
// more in start-ups than the order brings (profiles/r08_multi_order_ab.txt).
// *keep: whose outputs store normally -- the producers' direction (1 forward, 2 inverse) when there are consumers, the producers
// all have one direction and no consumer shares it (the kernel chooses the store kind by direction), else 0.  (Only whole chunks
// of a kept job store normally: a ragged last chunk, at most 4 KiB of a job, streams as before.)
unsigned fz_multi_plan(const FzMultiJobs &J, int degree, const FzProduced *prev, int n_prev, bool ordered, unsigned resident, int *order,
                       unsigned *end, int *consumers, int *keep) {
    auto tasks_of = [&](int j) { return ((size_t)(J.rows[j] & 0x7fffffffu) * (size_t)degree + kChunk - 1) / kChunk; };
    bool taken[kFzMultiMax] = {};
    int n = 0;
    if (ordered)
        for (int k = n_prev - 1; k >= 0; --k)                                // the most recently produced first
            for (int j = 0; j < J.n; ++j) {
                const unsigned rows = J.rows[j] & 0x7fffffffu;
                if (taken[j] || rows == 0 || J.in[j] != prev[k].out || rows > prev[k].rows) continue;
                taken[j] = true;
                order[n++] = j;
            }
    *consumers = n;
    for (int j = 0; j < J.n; ++j)
        if (!taken[j]) order[n++] = j;
    size_t all_tasks = 0;
    for (int j = 0; j < J.n; ++j) all_tasks += tasks_of(j);
    unsigned total = 0;
    for (int k = 0; k < J.n; ++k) {
        const size_t tasks = tasks_of(order[k]);
        const size_t blocks = (tasks + kWavesPerBlock - 1) / kWavesPerBlock;
        size_t share = all_tasks ? ((size_t)resident * tasks + all_tasks - 1) / all_tasks : 0;   // proportional, rounded up, at least one
        if (share < 1) share = 1;
        total += (unsigned)(tasks ? std::min(blocks, share) : 0);
        end[k] = total;
    }
    unsigned dirs_cons = 0, dirs_prod = 0;                                  // bit 0: forward jobs among them, bit 1: inverse jobs
    for (int k = 0; k < J.n; ++k) (k < *consumers ? dirs_cons : dirs_prod) |= 1u << (J.rows[order[k]] >> 31);
    *keep = *consumers > 0 && (dirs_prod == 1 || dirs_prod == 2) && (dirs_cons & dirs_prod) == 0 ? (int)dirs_prod : 0;
    return total;
}

// what the launch just issued wrote, in the order it ran (order == nullptr: table order), and the layout it ran in
// (fz_diag_multi_last)
static void record_produced(fz_ctx *ctx, const FzMultiJobs &J, const int *order, int consumers, int keep) {
    ctx->last_n = J.n; ctx->last_consumers = consumers; ctx->last_keep = keep;
    for (int k = 0; k < J.n; ++k) ctx->last_order[k] = order ? order[k] : k;
    ctx->n_produced = 0;
    if (!ctx->knob_multi_order) return;
    for (int k = 0; k < J.n; ++k) {
        const int j = order ? order[k] : k;
        ctx->produced[ctx->n_produced++] = FzProduced{J.out[j], J.rows[j] & 0x7fffffffu};
    }
}

// the 16-per-lane form of a multi-job launch: job j gets min(its workgroups, its share of the resident grid) workgroups
template <int LOGD, bool FAST>
static int launch_jobs16(fz_ctx *ctx, const FzMultiJobs &J, hipEvent_t e0, hipEvent_t e1) {
    const unsigned cap = (unsigned)std::min(ctx->grid_fwd, ctx->grid_inv);  // workgroups the chip holds at once
    int order[kFzMultiMax];
    FzMultiJobs P;                                                           // the table in execution order (the caller's is left alone)
    int consumers = 0, keep = 0;
    const unsigned total = fz_multi_plan(J, 1 << LOGD, ctx->produced, ctx->n_produced, ctx->knob_multi_order != 0, cap, order, P.end,
                                         &consumers, &keep);
    P.n = J.n;
    for (int k = 0; k < J.n; ++k) { P.in[k] = J.in[order[k]]; P.out[k] = J.out[order[k]]; P.rows[k] = J.rows[order[k]]; }
    for (int k = J.n; k < kFzMultiMax; ++k) { P.end[k] = total; P.rows[k] = 0; P.in[k] = nullptr; P.out[k] = nullptr; }
    if (total == 0) return FZ_OK;
    unsigned long long *stamp = stamp_slots(ctx, total);
    const dim3 grid(total), block(64 * kWavesPerBlock);
    auto by_size = [&](auto kp) {
        constexpr int KP = decltype(kp)::value;
        with_jobs_table(P, [&](auto S) {
            if constexpr (KP == 0)
                hipExtLaunchKernelGGL((ntt_jobs16<LOGD, FAST, decltype(S)>), grid, block, 0, ctx->stream, e0, e1, 0, S,
                                      (const double2 *)ctx->d_twB, (const double2 *)ctx->d_itwB, ctx->twA, ctx->itwA, ctx->mod, stamp);
            else
                hipExtLaunchKernelGGL((ntt_jobs16_keep<LOGD, FAST, decltype(S), KP>), grid, block, 0, ctx->stream, e0, e1, 0, S,
                                      (const double2 *)ctx->d_twB, (const double2 *)ctx->d_itwB, ctx->twA, ctx->itwA, ctx->mod, stamp);
        });
    };
    if (keep == 1) by_size(std::integral_constant<int, 1>());
    else if (keep == 2) by_size(std::integral_constant<int, 2>());
    else by_size(std::integral_constant<int, 0>());
    record_produced(ctx, J, order, consumers, keep);
    return fz_check_hip(hipGetLastError(), "ntt_jobs16 launch");
}

template <int LOGD, bool FAST>
static int launch_jobs_f(fz_ctx *ctx, FzMultiJobs &J) {
    constexpr unsigned PPW = 64 / ((1 << LOGD) / 4);
    unsigned long long waves1 = 0;                                     // waves at one row group per wave, over all jobs
    for (int j = 0; j < J.n; ++j) waves1 += ((J.rows[j] & 0x7fffffffu) + PPW - 1) / PPW;
    if (waves1 == 0) return FZ_OK;
    if (waves1 > 0x7fffffffull) return fz_set_error(FZ_E_UNSUPPORTED, "too many rows for one multi-job launch");
    // the schedule by the launch's TOTAL rows, as for one job (launch16): the 16-per-lane kernels from `small_batch_rows` on
    // (FZ_NTT_KERNEL forces either)
    size_t all_rows = 0;
    for (int j = 0; j < J.n; ++j) all_rows += J.rows[j] & 0x7fffffffu;
    const bool big = ctx->force_kernel == 16 || (ctx->force_kernel == 0 && all_rows >= (size_t)ctx->small_batch_rows);
    const ProfEvents ev = prof_events(ctx, 2);
    if (big) return launch_jobs16<LOGD, FAST>(ctx, J, ev.e0, ev.e1);
    // the same launch shapes, by the same rule, as the one-job kernels (launch4f): rows per wave by the launch's total
    with_shape4(ctx, (size_t)waves1, [&](auto nr, auto waves) { launch_jobs<LOGD, FAST, nr(), waves()>(ctx, J, ev.e0, ev.e1); });
    record_produced(ctx, J, nullptr, 0, 0);                                  // (one wave-task per wave: the grid runs in table order)
    return fz_check_hip(hipGetLastError(), "ntt_jobs4 launch");
}

// J.in / J.out / J.rows (bit 31: inverse) / J.n filled by the caller; J.end (workgroups per job) is computed here by the radix-4
// path only: the 16-per-lane path leaves J alone and lays out a permuted copy of it (fz_multi_plan)
int fz_launch_ntt_multi(fz_ctx *ctx, FzMultiJobs &J) {
    if (ctx->logd != 6 && ctx->logd != 8) return fz_set_error(FZ_E_UNSUPPORTED, "multi-job transform: degree 64 or 256 only");
    if (J.n <= 0) return FZ_OK;
    return fz_dispatch<6, 8>(ctx, FZ_E_UNSUPPORTED, [&](auto logd, auto fast) { return launch_jobs_f<logd(), fast()>(ctx, J); });
}

// ------------------------------------------------------------------------------------------
// Launch-floor diagnostics (fz_diag_*): what a dispatch of NO work and a plain copy of the same bytes cost on this
// device, measured next to the transforms so that a small batch can be judged against a same-run floor.
// ------------------------------------------------------------------------------------------
namespace {
__global__ __launch_bounds__(64) void diag_empty_kernel() {}
__global__ __launch_bounds__(64) void diag_copy_kernel(const int4 *__restrict__ src, int4 *__restrict__ dst, size_t n16) {
    const size_t stride = (size_t)gridDim.x * 64;
    for (size_t i = (size_t)blockIdx.x * 64 + threadIdx.x; i < n16; i += stride) {
        const fz_v4i t = *reinterpret_cast<const fz_v4i *>(src + i);
        __builtin_nontemporal_store(t, reinterpret_cast<fz_v4i *>(dst + i));
    }
}
// one wave that watches the clocks for `ticks` periods of the 100 MHz reference counter: shader cycles (s_memtime) per
// reference tick = the frequency the chip actually runs at while whatever else is resident executes
__global__ __launch_bounds__(64) void diag_clock_kernel(unsigned long long ticks, unsigned long long *out) {
    const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    unsigned long long r1 = r0;
    while (r1 - r0 < ticks) {             // every wave reaches the exit: the reference counter never stops
        __builtin_amdgcn_s_sleep(8);
        r1 = __builtin_amdgcn_s_memrealtime();
    }
    if (threadIdx.x == 0 && out) { out[0] = __builtin_amdgcn_s_memtime() - t0; out[1] = r1 - r0; }
}
}  // namespace

int fz_launch_diag_clock(hipStream_t stream, unsigned long long ticks, unsigned long long *d_out) {
    hipLaunchKernelGGL(diag_clock_kernel, dim3(1), dim3(64), 0, stream, ticks, d_out);
    return fz_check_hip(hipGetLastError(), "diag clock launch");
}

int fz_launch_diag(fz_ctx *ctx, int what, const void *src, void *dst, size_t bytes) {
    if (what == 0) {
        hipLaunchKernelGGL(diag_empty_kernel, dim3(4096), dim3(64), 0, ctx->stream);
    } else {
        const size_t n16 = bytes / 16;
        if (n16 == 0) return FZ_OK;
        // flat grid, one 16-byte item per thread: a capped grid-stride loop streams 1 GiB at 4.9-5.5 TB/s, the flat grid at
        // 6.2 TB/s (profiles/r02_launch_floor.txt) -- the ceiling this kernel exists to show
        const size_t blocks = (n16 + 63) / 64, cap = (size_t)0x7fffffff;
        hipLaunchKernelGGL(diag_copy_kernel, dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(64), 0, ctx->stream,
                           (const int4 *)src, (int4 *)dst, n16);
    }
    return fz_check_hip(hipGetLastError(), "diag launch");
}
