// fz_internal.h -- shared declarations between the translation units of libfusion_hip.so.
#ifndef FZ_INTERNAL_H
#define FZ_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <mutex>
#include <type_traits>
#include "fz_arith.h"
#include "../../include/fusion_hip.h"

// Wave-uniform twiddles of the strided pass, passed BY VALUE so they live in the kernarg
// segment and reach the kernel as scalar loads (SGPR operands of the fp64 multiplies).
struct FzTwA {
    double w[16];      // entries 1..15 of the bit-reversed power table (entry 0 unused)
    double w2[16];     // w[i] * K / q (quotient twiddles of fz_mulmod4)
    double n_inv;      // degree^{-1} mod q            (inverse only)
    double w1_n_inv;   // w[1] * degree^{-1} mod q      (inverse only: n^{-1} folded into last stage)
    double n_inv2, w1_n_inv2;   // their quotient twiddles
};

// the same for the radix-4 kernels, which use entries 1..3 only: 96 bytes of kernel arguments instead of 288 per direction
// (the multi-job launch carries both directions: a launch's scalar loads are in front of its first data load)
struct FzTw4 {
    double w[4], w2[4];
    double n_inv, w1_n_inv, n_inv2, w1_n_inv2;
};
static inline FzTw4 fz_tw4(const FzTwA &a) {
    FzTw4 t;
    for (int i = 0; i < 4; ++i) { t.w[i] = a.w[i]; t.w2[i] = a.w2[i]; }
    t.n_inv = a.n_inv; t.w1_n_inv = a.w1_n_inv; t.n_inv2 = a.n_inv2; t.w1_n_inv2 = a.w1_n_inv2;
    return t;
}

// most jobs of one fz_ntt_multi launch (the table travels in the kernarg segment: FzMultiJobs below)
constexpr int kFzMultiMax = 32;

// what one multi-job launch wrote, in the order its jobs ran: the next launch of the context runs the jobs that read these first
struct FzProduced {
    const int32_t *out;
    unsigned rows;
};

// A device area of the context that is replaced by a larger one on demand: the pointer and its capacity in bytes.  Every
// area follows ONE rule, fz_area_fit below.
struct FzArea {
    void *p;
    size_t bytes;
};
enum {
    FZ_A_SCRATCH, FZ_A_SCRATCH2,   // host-pointer entry points, int64 partial sums
    FZ_A_VERDICT,                  // verdicts of fz_verify_with_target_batch, one int per aggregate
    FZ_A_VPART, FZ_A_VSTATE,       // fused verification (fz_verify_scratch)
    FZ_A_AGGACC,                   // one-pass aggregation (fz_agg_scratch)
    FZ_A_CHAL_TAB,                 // weight table of the challenge decoder (fz_challenge.hip), built on first use
    FZ_A_STAMP,                    // fz_diag_stamps_*
    FZ_A_COUNT
};

struct fz_ctx {
    int device;
    int num_cu;
    hipStream_t stream;
    hipEvent_t ev0, ev1;
    uint32_t q, root, inv_root;
    int degree, logd;
    FzMod mod;
    // host tables, bit-reversed powers in [0,q)
    uint32_t *h_tw, *h_itw;
    // device tables
    double *d_tw, *d_itw;        // [degree] as doubles (generic / small kernels)
    double *d_twB, *d_itwB;      // per-lane tables of the contiguous pass, [NE][L] pairs (w, w*K/q)
    double *d_twAB;              // {twA, itwA} as two FzTwA in device memory (polymul16 reads them as constants, per direction)
    double *d_tw2, *d_itw2;      // full tables as (w, w*K/q) pairs, [degree] (radix-4 kernels)
    int small_batch_rows;        // below this many rows the radix-4 (4 coefficients per lane) kernels run
    int force_kernel;            // 0 auto, 4 radix-4, 16 sixteen-per-lane (env FZ_NTT_KERNEL; tests and A/B runs)
    FzTwA twA, itwA;
    FzArea area[FZ_A_COUNT];     // the growable device areas (fz_area_fit); fz_ctx_destroy releases every one
    int grid_fwd, grid_inv;      // resident-grid caps for the persistent NTT kernels
    int grid_pm;                 // resident grid of the fused product kernel (0 = not queried yet)
    int grid_pm16;               // ... of its 16-per-lane form
    int grid_rec[4];             // ... of the byte-encoding kernels: [encode, decode] x [coefficient kinds, keys] (degree 64 / 256)
    int grid_aggenc, grid_check; // ... of aggregate_encoded and encoded_check (fz_aggregate_encoded.hip; degree 64 / 256)
    int grid_signenc;            // ... of sign_encode (fz_sign_encoded.hip; degree 64 / 256)
    int grid_aggenc_rag;         // ... of aggregate_encoded_ragged (fz_aggregate_many_encoded.hip; degree 64 / 256)
    int grid_signrec;            // ... of sign_records (fz_sign_records.hip; degree 64 / 256)
    int grid_keyrec;             // ... of keygen_records_bcast (fz_keygen_records.hip; degree 64 / 256)
    // verification from the bytes with several workgroups per record (fz_verify_encoded.hip; degree 64 / 256): a slot of int64 sums
    // and a status word per record, venc_bytes in all; allocated once at context creation (fz_verify_encoded_setup), never grown --
    // the entry is allocation-free and capturable from its first call -- and released by fz_ctx_destroy
    unsigned long long *d_venc;
    size_t venc_bytes;
    int knob_ntt_rows;           // FZ_NTT_ROWS = 1 | 2 | 4: row groups per wave of the radix-4 kernels (0 = by batch size)
    // per-dispatch timing of the NTT kernels (fz_profile_begin/end): event pairs bound to the
    // dispatch itself via hipExtLaunchKernelGGL, i.e. kernel begin -> kernel end on its own stream
    int prof_on, prof_cap, prof_n, prof_every, prof_seen[2];
    hipEvent_t *prof_ev;         // 2 * prof_cap events
    unsigned char *prof_kind;    // 0 forward, 1 inverse
    int capturing;               // between fz_graph_begin and fz_graph_end: nothing may allocate or synchronise
    // fused verification: per-aggregate fp64 accumulators of `observed` [groups][degree] and state words
    // (arrival / failure counts); all zero between launches -- the kernel re-arms them itself
    // (areas FZ_A_VPART, FZ_A_VSTATE)
    int verify_dirty;            // a verify launch failed: accumulators / state words are re-zeroed before the next one
    // one-pass aggregation: per (aggregate, column block) accumulator words [tiles][tile_words] (running sum + arrival
    // count, see aggregate_onepass); all zero between launches (the last adder of a word re-arms it)
    // (area FZ_A_AGGACC)
    int agg_dirty;
    uint32_t *d_mt_init;         // MT19937 state after init_genrand(19650218) (fz_sample_secret_polys_dev), lazily
    int chal_tab_ib, chal_tab_degree;   // what the table in FZ_A_CHAL_TAB was built for
    // Pinned, device-visible staging for the SMALL host inputs of the fused challenge kernel (message bytes + offsets, or the
    // digests) and of the sampler (the seeds): the kernel reads them in place over the host link (three coalesced requests per
    // wave), so a call uploads nothing and does not synchronise.  Two slots in turn; a slot's event is recorded after the launch
    // that reads it and waited for before the slot is written again (stage_take / stage_release, fz_staged_capi.hip).
    struct FzStage { uint8_t *h; size_t bytes; hipEvent_t ev; int busy; };
    FzStage chal_stage[2];
    int chal_stage_next;
    // benchmarking knobs, read ONCE at context creation
    int knob_agg_direct;         // FZ_AGG_DIRECT: -1 = never the slice-free aggregation kernel, 2 | 4 = always, with that many rows per tile (0 = by size)
    int knob_shake_full;         // FZ_SHAKE_FORM: 1 = lane pairs, 2 = whole state per lane, 3 = a wave per signer (0 = by batch size)
    int knob_verify_ordered;     // FZ_VERIFY_ORDERED=1 (and every device that is not gfx950): acquire / release on verify_fused's arrival atomic
    int knob_polymul_form;       // FZ_POLYMUL_FORM: 1 = the radix-4 product kernel, 2 = the 16-per-lane one (0 = by batch size)
    int knob_unfused;            // FZ_UNFUSED=1: the multi-launch paths of keygen / verification / the coefficient-domain product (what degrees other than 64 / 256 take anyway)
    hipStream_t diag_stream;     // fz_diag_shader_clock: the probe's private stream and result words (created on first use)
    unsigned long long *d_diag;
    int knob_matvec_slices;      // FZ_MATVEC_SLICES = 1 | 2 | 4: k-range slices per column of the integer matvec kernel (0 = by batch size, -1 = the fp64 kernel)
    int knob_no_imad;            // FZ_NO_IMAD=1: A (.) y through the general fp64 multiply instead of integer multiply-adds (A/B runs)
    int knob_verify_cent;        // FZ_VERIFY_CENT=1: centre the inverse transform's outputs before the norm test even when beta allows skipping it
    int knob_hash_ag_order;      // FZ_HASH_AG_ORDER=0: the device hash_ag hands its waves the committees in the caller's order (1, the default: longest first)
    int knob_multi_order;        // FZ_MULTI_ORDER=0: a multi-job launch runs its jobs in table order, streaming stores throughout (1, the default: fz_multi_plan)
    // the previous multi-job launch's outputs in the order they were produced (host memory, written when a launch is issued or
    // CAPTURED: a graph replays the order it was captured with)
    FzProduced produced[kFzMultiMax];
    int n_produced;
    int last_order[kFzMultiMax], last_n, last_consumers, last_keep;   // the layout of the last multi-job launch (fz_diag_multi_last)
    // device allocations replaced by a larger one while a captured graph may still hold their address: kept until
    // fz_ctx_destroy (a replay must never touch freed memory)
    int graphs_captured;
    void **retired;
    int n_retired, cap_retired;
    // fz_malloc / fz_free keep large blocks for reuse (hipFree of anything from 16 MiB up costs ~180 us AND synchronises the
    // device): live blocks with their sizes, and the blocks handed back, at most pool_cap bytes of them (FZ_POOL_MB, 0 = off)
    // `ev`: recorded on the context's stream when the block came back (fz_free), waited for by the stream that reuses it.
    // The arrays are guarded by pool_mu: a DeviceBuffer.__del__ may run on any thread (cyclic garbage collection).
    struct FzBlock { void *p; size_t bytes; hipEvent_t ev; };
    FzBlock *live_blocks, *pool_blocks;
    int n_live, cap_live, n_pool, cap_pool;
    size_t pool_bytes, pool_cap;
    std::mutex pool_mu;
    // RCCL (fz_comm_*): communicators are owned by the caller; nothing here
    // fz_diag_stamps_*: device-side launch timestamps of the multi-job transform ({entry, exit} of the 100 MHz reference counter
    // per workgroup); launch k of the recording owns slots [stamp_first[k], stamp_first[k] + stamp_count[k])
    int stamp_on, stamp_n, stamp_launch_cap;
    size_t stamp_used, stamp_wg_cap;     // (the slots are area FZ_A_STAMP)
    size_t *stamp_first;
    unsigned *stamp_count;
};

// group table of a ragged aggregation launch (kernarg segment): signers of aggregate g are rows [off[g], off[g+1]) of the
// concatenated signature / coefficient arrays; base / extra = its signers per slice and the remainder
constexpr int kFzRaggedMax = 64;
struct FzRagged {
    unsigned off[kFzRaggedMax + 1];
    unsigned base[kFzRaggedMax], extra[kFzRaggedMax];
};

// the job table of one fz_ntt_multi launch travels in the kernarg segment (no device copy, capturable in a graph)
struct FzMultiJobs {
    const int32_t *in[kFzMultiMax];
    int32_t *out[kFzMultiMax];
    unsigned end[kFzMultiMax];   // running total of WORKGROUPS up to and including job j (the radix-4 path fills it; the 16-per-lane path its own permuted copy)
    unsigned rows[kFzMultiMax];  // rows of job j; bit 31 set: inverse transform
    int n;
};

// the table as the kernel takes it: N = 4 | 8 | 32 entries, 24 bytes of kernel arguments each (a launch of four jobs
// carries 96 bytes of table instead of 772)
template <int N> struct FzJobsN {
    static constexpr int kJobs = N;
    const int32_t *in[N];
    int32_t *out[N];
    unsigned end[N];
    unsigned rows[N];
};

struct fz_graph {
    hipGraph_t graph;
    hipGraphExec_t exec;
    int device;
};

// largest transform length: up to 256 the register / LDS schedules of fz_ntt_dev.h, beyond it one workgroup per polynomial through LDS
constexpr int kFzMaxDegree = 4096;

// error plumbing (fz_context.hip)
int fz_set_error(int code, const char *fmt, ...);
int fz_check_hip(hipError_t e, const char *what);
#define FZ_TRY(x) do { int rc_ = (x); if (rc_ != FZ_OK) return rc_; } while (0)
#define FZ_HIP(x, what) FZ_TRY(fz_check_hip((x), what))
#define FZ_REQUIRE(cond, ...) do { if (!(cond)) return fz_set_error(FZ_E_BADARG, __VA_ARGS__); } while (0)
// Every entry point that touches the device makes the context's device current first: a process may hold contexts on
// several GPUs (and other code -- torch -- may have changed the current device behind our back); kernels, scratch
// allocations and events must land on ctx->device whatever stream the caller attached.
#define FZ_DEV(ctx) FZ_HIP(hipSetDevice((ctx)->device), "hipSetDevice")

// Is work on this context being recorded rather than executed?  Either the context opened a capture itself (fz_graph_begin) or
// its stream was drawn into another context's capture by fz_event_wait on an event recorded there (the fork / join of a
// two-stream capture): the runtime knows, so ask it -- nothing may allocate, copy to the host or synchronise in either case.
static inline bool fz_capturing(fz_ctx *ctx) {
    if (ctx->capturing) return true;
    if (!ctx->stream) return false;
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(ctx->stream, &st) != hipSuccess) { (void)hipGetLastError(); return false; }
    return st == hipStreamCaptureStatusActive;
}

// The one rule of the growable areas (fz_context.hip).  fz_area_replace: refused with FZ_E_BADARG during capture, before any
// runtime call (the open capture stays valid); otherwise the context's stream is drained (the area's previous users are
// stream-ordered before this point), the old allocation goes to fz_retire, the area is marked empty and `capacity` bytes are
// allocated -- a failure leaves the area empty, never dangling.  The contents are undefined.  fz_area_fit: a request that fits
// makes no runtime call; one that does not replaces the area and sets *fresh.
int fz_area_replace(fz_ctx *ctx, int which, size_t capacity);
static inline int fz_area_fit(fz_ctx *ctx, int which, size_t need, size_t capacity, bool *fresh = nullptr) {
    if (need <= ctx->area[which].bytes) return FZ_OK;
    if (fresh) *fresh = true;
    return fz_area_replace(ctx, which, capacity);
}
static inline int fz_scratch(fz_ctx *ctx, size_t bytes, void **out, int which = FZ_A_SCRATCH) {
    FZ_TRY(fz_area_fit(ctx, which, bytes, bytes + bytes / 4 + 4096));
    *out = ctx->area[which].p;
    return FZ_OK;
}
// The layout of one entry's scratch, written once: take(bytes) -> the segment's offset, each segment starting on the next multiple
// of 256 behind the one before; take_packed: straight behind it instead.  end = where the last segment ends (what most entries
// request), next = where take() would put another (the request of an entry that rounds its last segment too, and what a layout
// occupies in front of segments carved on top of it).  fit() sizes the area for `bytes` of it; at<T>(offset) = the segment there.
struct FzCarve {
    size_t end = 0, next = 0;
    void *base = nullptr;                          // (the area, once fit() has sized it)
    size_t take(size_t bytes) { return place(next, bytes); }
    size_t take_packed(size_t bytes) { return place(end, bytes); }
    int fit(fz_ctx *ctx, size_t bytes, int which = FZ_A_SCRATCH) { return fz_scratch(ctx, bytes, &base, which); }
    template <class T> T *at(size_t offset) const { return (T *)((char *)base + offset); }
    size_t place(size_t offset, size_t bytes) { end = offset + bytes; next = offset + ((bytes + 255) & ~(size_t)255); return offset; }
};
int fz_verdict_area(fz_ctx *ctx, size_t groups, int **d_verdict);
int fz_verify_scratch(fz_ctx *ctx, size_t groups, size_t doubles_per_group, double **part, int **state);
int fz_agg_scratch(fz_ctx *ctx, size_t tiles, size_t tile_words, unsigned long long **acc);
int fz_retire(fz_ctx *ctx, void *d_ptr, const char *what);       // hipFree, or keep until destroy when graphs were captured

// The host dispatch on (degree, multiply form), written once: f(std::integral_constant<int, LOGD>, std::bool_constant<FAST>) for
// the context's degree, when it is one of 2^LOGDS, and its modulus' multiply form (4-op pseudo-Mersenne when mod.fast) -> what f
// returns; `other` when the degree is none of them.  f is instantiated for the named degrees only, in both forms.
template <int... LOGDS, class F>
int fz_dispatch(const fz_ctx *ctx, int other, F &&f) {
    int rc = other;
    (void)((ctx->logd == LOGDS && ((rc = ctx->mod.fast ? f(std::integral_constant<int, LOGDS>(), std::true_type())
                                                       : f(std::integral_constant<int, LOGDS>(), std::false_type())), true)) || ...);
    return rc;
}

// how many workgroups of `kernel` (`threads` each, static LDS only) the chip holds at once, at least one per CU: the resident
// grid a persistent kernel is capped at
template <class K>
int fz_resident_grid(const fz_ctx *ctx, K kernel, int threads, const char *what, int *grid) {
    int n = 0;
    const int rc = fz_check_hip(hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, threads, 0), what);
    if (rc == 0) *grid = (n < 1 ? 1 : n) * ctx->num_cu;       // (0: FZ_OK)
    return rc;
}

// What each kernel unit needs from context creation, which runs them in this order for every context with transforms (fz_context.hip)
// and stops at the first error: the resident grid of each persistent kernel (ctx->grid_*; degrees 64 / 256 -- the transforms' 32
// to 256 -- and nothing to query at the others) and the one allocation, ctx->d_venc.  Each does its own unit's work alone.
int fz_ntt_query_grid(fz_ctx *ctx);                     // grid_fwd, grid_inv (fz_ntt.hip)
int fz_records_query_grid(fz_ctx *ctx);                 // grid_rec (fz_records.hip)
int fz_aggregate_encoded_query_grid(fz_ctx *ctx);       // grid_aggenc, grid_check (fz_aggregate_encoded.hip)
int fz_verify_encoded_setup(fz_ctx *ctx);               // d_venc, venc_bytes (fz_verify_encoded.hip)
int fz_sign_encoded_query_grid(fz_ctx *ctx);            // grid_signenc (fz_sign_encoded.hip)
int fz_aggregate_many_encoded_query_grid(fz_ctx *ctx);  // grid_aggenc_rag (fz_aggregate_many_encoded.hip)
int fz_sign_records_query_grid(fz_ctx *ctx);            // grid_signrec (fz_sign_records.hip)
int fz_keygen_records_query_grid(fz_ctx *ctx);          // grid_keyrec (fz_keygen_records.hip)

// transforms (fz_ntt.hip)
int fz_launch_ntt(fz_ctx *ctx, const int32_t *d_in, int32_t *d_out, size_t batch, bool inverse);
int fz_launch_ntt_multi(fz_ctx *ctx, FzMultiJobs &jobs);           // degree 64 / 256; the radix-4 path fills jobs.end
// the layout of a 16-per-lane multi-job launch: order[k] = the table entry that runs k-th (the first *consumers of them read what
// `prev` wrote), end[k] = workgroups up to and including it, for `resident` workgroups on the chip at once, *keep = the direction
// whose outputs store normally (0 none, 1 forward, 2 inverse); -> workgroups in all
unsigned fz_multi_plan(const FzMultiJobs &J, int degree, const FzProduced *prev, int n_prev, bool ordered, unsigned resident, int *order,
                       unsigned *end, int *consumers, int *keep);
int fz_launch_diag_clock(hipStream_t stream, unsigned long long ticks, unsigned long long *d_out);
int fz_launch_diag(fz_ctx *ctx, int what, const void *src, void *dst, size_t bytes);

// fused products (fz_polymul.hip)
int fz_launch_polymul_fused(fz_ctx *ctx, const int32_t *f, const int32_t *g, int32_t *out, size_t batch);
bool fz_polymul16_ok(const fz_ctx *ctx, const int32_t *f, const int32_t *g, const int32_t *out, size_t batch);

// compact byte encoding (fz_records.hip; degree 64 / 256): n records of rows * degree values, w-bit fields u = z + bound; encode (decode =
// false) rows -> bytes, decode bytes -> rows; d_status [n] cleared, then 0 or FZ_VERDICT_NORM / FZ_VERDICT_ENCODING; failed records zeroed
// bytes of ONE record: rows * degree fields of w bits (the degree is a multiple of 8)
static inline size_t fz_record_bytes(int degree, int rows, int w) { return (size_t)rows * (size_t)degree / 8 * (size_t)w; }
int fz_launch_records(fz_ctx *ctx, bool decode, const void *src, void *dst, size_t n, int rows, bool coef, int w, int64_t bound,
                      int *d_status);
// the follow-up of every launch that leaves records and status words: record i of `dst` (rec_bytes each, a multiple of 8) is
// zeroed where d_status[i] != 0
int fz_launch_records_zero(fz_ctx *ctx, const int *d_status, size_t n, void *dst, size_t rec_bytes);
// the launch sequence of every pass that leaves records and status words: d_status [n] cleared, launch() (the caller's dispatch on
// degree and multiply form; FZ_OK when it launched), the launch error named `what`, then the zeroing above.  Asynchronous and
// allocation-free: a graph capture records all three.
template <class F>
int fz_records_pass(fz_ctx *ctx, int *d_status, size_t n, const char *what, F &&launch, void *dst, size_t rec_bytes) {
    int rc = fz_check_hip(hipMemsetAsync(d_status, 0, n * sizeof(int), ctx->stream), "records status clear");
    if (rc != FZ_OK) return rc;
    rc = launch();
    if (rc == FZ_OK) rc = fz_check_hip(hipGetLastError(), what);
    if (rc != FZ_OK) return rc;
    return fz_launch_records_zero(ctx, d_status, n, dst, rec_bytes);
}

// signing straight to the bytes (fz_sign_encoded.hip; degree 64 / 256): record i of d_bytes = the encoding of
// cent(cent(L_i (.) c_i) + R_i) from sk_hat [n][2][l][degree] and c_hat [n][degree], any int32; d_status [n] cleared, then 0 or
// FZ_VERDICT_NORM; refused records zeroed
int fz_launch_sign_encoded(fz_ctx *ctx, const int32_t *sk_hat, const int32_t *c_hat, size_t n, int l, int w, int64_t bound,
                           uint8_t *d_bytes, int *d_status);

// signing straight from "secret" records to the bytes (fz_sign_records.hip; degree 64 / 256): record i of d_bytes = the encoding of
// cent(INV(cent(FWD(sL_i) (.) c_i)) + sR_i) from key records [n][2][l][degree] of wk-bit fields s + key_bound and c_hat [n][degree], any
// int32; d_status [n] cleared, then 0, FZ_VERDICT_NORM or FZ_VERDICT_ENCODING (a key field above 2 key_bound); refused records zeroed
int fz_launch_sign_records(fz_ctx *ctx, const uint8_t *key_bytes, int wk, int64_t key_bound, const int32_t *c_hat, size_t n, int l,
                           int w, int64_t bound, uint8_t *d_bytes, int *d_status);

// key generation straight to "secret" records (fz_keygen_records.hip; degree 64 / 256): record i of d_bytes = the fields s + key_bound
// (wk bits) of s = cent(coef mod q) over [2][l][degree], from coef [n][2][degree] (one polynomial per half for all l rows) or,
// with `rows`, [n][2][l][degree]; d_vk [n][2][degree] as fz_launch_keygen_fused writes it; d_status [n] cleared, then 0 or
// FZ_VERDICT_NORM; refused records zeroed
int fz_launch_keygen_records(fz_ctx *ctx, const int32_t *A, const int32_t *coef, bool rows, size_t n, int l, int wk, int64_t key_bound,
                             uint8_t *d_bytes, int32_t *d_vk, int *d_status);

// verification keys straight from "secret" records (fz_vk_records.hip; degree 64 / 256): d_vk [n][2][degree] = per half
// cent(sum_k cent(FWD(s_k) (.) A_k)) from key records [n][2][l][degree] of wk-bit fields s + key_bound and A [l][degree], any int32;
// d_status [n] cleared, then 0 or FZ_VERDICT_ENCODING (a key field above 2 key_bound); refused keys' vk zeroed.  2 n fits a
// grid's first dimension (the entry sees to it); FZ_E_UNSUPPORTED for l >= 2^22
int fz_launch_vk_records(fz_ctx *ctx, const int32_t *A, const uint8_t *key_bytes, int wk, int64_t key_bound, size_t n, int l,
                         int32_t *d_vk, int *d_status);

// the byte encoding's consumers without rows (fz_aggregate_encoded.hip; degree 64 / 256): the range check of a byte stream alone
// (d_status [n] cleared, then 0 or FZ_VERDICT_ENCODING), and the aggregate of N signature records of l rows straight from
// their bytes: d_partial [l][degree] int64 zeroed, then sum_i cent(NTT(z_i) (.) alpha_hat_i) over the signers with skip[i] == 0
// (skip NULL: all), d_out = cent(d_partial) when not NULL.  Records of the aggregation are multiples of 16 bytes.
int fz_launch_check_records(fz_ctx *ctx, const uint8_t *bytes, size_t n, int rows, int w, int64_t bound, int *d_status);
int fz_launch_aggregate_encoded(fz_ctx *ctx, const uint8_t *bytes, const int32_t *alpha, const int *skip, size_t n, int l, int w,
                                int64_t bound, int64_t *d_partial, int32_t *d_out);

// many aggregates of different sizes straight from the bytes in one launch (fz_aggregate_many_encoded.hip; degree 64 / 256): group g
// of `groups` owns records [h_offsets[g], h_offsets[g + 1]) of the concatenated byte stream and the same rows of alpha and skip;
// its int64 partial [l][degree] at d_partial + g * pstride is zeroed, then summed as fz_launch_aggregate_encoded does; d_out
// [groups][l][degree] = cent(partial) when not NULL.  h_offsets is read before the call returns.
int fz_launch_aggregate_encoded_ragged(fz_ctx *ctx, const uint8_t *bytes, const int32_t *alpha, const int *skip, const size_t *h_offsets,
                                       size_t groups, int l, int w, int64_t bound, int64_t *d_partial, size_t pstride, int32_t *d_out);

// the same with the groups' verification targets beside the aggregates (fz_aggregate_target_encoded.hip; degree 64 / 256): the
// int64 partial [degree] at d_target_partial + g * tstride is zeroed, then summed over group g's signers with skip[i] == 0 as
// fz_launch_aggregate sums it with tout64 (the term of agg_target4) from vk [N][2][degree] and chal [N][degree]; one launch per
// kFzRaggedMax groups for both kinds of sums.  d_partial, pstride and d_out as above.
int fz_launch_aggregate_target_encoded_ragged(fz_ctx *ctx, const uint8_t *bytes, const int32_t *alpha, const int *skip, const int32_t *vk,
                                              const int32_t *chal, const size_t *h_offsets, size_t groups, int l, int w, int64_t bound,
                                              int64_t *d_partial, size_t pstride, int64_t *d_target_partial, size_t tstride, int32_t *d_out);

// verification straight from the bytes (fz_verify_encoded.hip; degree 64 / 256): d_verdict [N] = 0, FZ_VERDICT_TARGET_MISMATCH or
// FZ_VERDICT_ENCODING of N records of l rows against `target` [N][degree] (any residues) or, when vk != NULL, against
// cent(vkL (.) c + vkR) from vk [N][2][degree] and chal [N][degree].  Records are multiples of 16 bytes.
int fz_launch_verify_encoded(fz_ctx *ctx, const int32_t *A, const uint8_t *bytes, size_t N, int l, int w, int64_t bound,
                             const int32_t *target, const int32_t *vk, const int32_t *chal, int *d_verdict);

// fused keygen and verification (fz_scheme_fused.hip)
int fz_launch_keygen_fused(fz_ctx *ctx, const int32_t *A, const int32_t *coef, int32_t *sk_hat, int32_t *vk, size_t segments,
                           int l, bool broadcast = false);
int fz_launch_verify_fused_i64(fz_ctx *ctx, const int32_t *A, const int64_t *sig, size_t sig_stride, const int64_t *target,
                               size_t target_stride, size_t groups, int l, int64_t beta, int64_t omega, int *d_verdict);
int fz_launch_verify_fused(fz_ctx *ctx, const int32_t *A, const int32_t *sig, const int32_t *target, size_t groups, int l,
                           int64_t beta, int64_t omega, int *d_verdict);
int fz_launch_verify_signatures(fz_ctx *ctx, const int32_t *A, const int32_t *sig, const int32_t *vk, const int32_t *c, size_t N,
                                int l, int64_t beta, int64_t omega, int *d_verdict);

// challenge pipeline on the device (fz_challenge.hip; its entries and their host side: fz_staged_capi.hip) and the pieces it shares
// with the host serialiser (fz_host.cpp)
constexpr int kFzShakeRate = 136;        // SHAKE-256 / SHA3-256 rate in bytes (17 lanes of 64 bits): a block of text, of stream
struct fz_scheme_params;
int fz_launch_challenge(fz_ctx *ctx, const fz_scheme_params *P, const int32_t *d_vk, const uint8_t *d_pre, const uint32_t *d_dec, size_t N,
                        uint8_t *d_text, size_t text_stride, int *d_nblocks, uint32_t *d_xof, size_t xstride, int out_blocks,
                        const uint32_t *d_tab, int32_t *d_coefs);
void fz_mt_init_table(uint32_t *h_tab);                                              // 624 words
// d_state: [2 * nkeys][624] words of scratch for the two-kernel form, or NULL for the one-kernel form
int fz_launch_mt_sample(fz_ctx *ctx, const unsigned long long *d_seeds, size_t nkeys, int degree, uint32_t bound, int kbits,
                        const uint32_t *d_init, int32_t *d_out, int *d_fail, uint32_t *d_state);
bool fz_challenge_wave_ok(const fz_scheme_params *P);        // the fused one-wave-per-signer form takes these parameters
int fz_launch_challenge_wave(fz_ctx *ctx, const fz_scheme_params *P, const int32_t *d_vk, const uint8_t *d_pre, const uint8_t *d_msgs,
                             const unsigned long long *d_off, uint8_t *d_pre_out, size_t N, size_t text_stride, int out_blocks,
                             const uint32_t *d_tab, int32_t *d_coefs);
int fz_launch_prehash(fz_ctx *ctx, const fz_scheme_params *P, const uint8_t *d_msgs, const unsigned long long *d_off, size_t N,
                      uint8_t *d_pre, uint32_t *d_dec);          // d_dec [N][16]: the integers in base 10^9 + chunk count
void fz_challenge_weight_table(int index_bytes, int degree, uint32_t *h_tab);      // (degree + 1) * 16 words
// fz_challenge_hat_msgs_dev's pipeline with the digests left in device memory (fz_staged_capi.hip; the entry: fz_vk_order_capi.hip)
int challenge_msgs_keep_dev(fz_ctx *ctx, const fz_scheme_params *P, const int32_t *d_vk, const char *h_msgs, const size_t *h_msg_off, size_t N,
                            int32_t *d_c_hat, uint8_t *d_prehash_out);
void fz_host_vk_text_parts(const fz_scheme_params *P, char *s0, int *n0, char *s1, int *n1, char *s2, int *n2, int cap);
size_t fz_host_challenge_needed_bytes(const fz_scheme_params *P, int *sign_bytes, int *coef_bytes, int *index_bytes);
bool fz_host_params_ok(const fz_scheme_params *P);

// hash_ag for many committees on the device (fz_hash_ag.hip; its entry: fz_hash_ag_capi.hip) and the pieces it shares with the host
// serialiser (fz_host.cpp)
bool fz_hash_ag_wave_ok(const fz_scheme_params *P, const char **why);   // *why (optional): the message of the refusal
// ord [M] row indices and grp [G] pairs of uint32 (first entry of ord, signers >= 1), both device-visible; one coefficient row of
// d_alpha per entry of ord, nothing else written
int fz_launch_hash_ag(fz_ctx *ctx, const fz_scheme_params *P, const int32_t *d_vk, const uint8_t *d_pre, const int32_t *d_c_hat,
                      const uint32_t *ord, const void *grp, size_t G, const uint32_t *d_tab, int32_t *d_alpha);
void fz_host_agg_text_parts(const fz_scheme_params *P, char *q0, char *q1, char *q2a, char *q2b, char *q3, int *n, int cap);
size_t fz_host_agg_section_bytes(const fz_scheme_params *P, int *sign_bytes, int *coef_bytes, int *index_bytes);

// the key sort of hash_ag for many committees on the device (fz_vk_order.hip; its entries: fz_vk_order_capi.hip)
// grp [G] uint4 (first row, rows >= 1, first entry of d_order, 0) and valid (a byte per row, or NULL: all), both device-visible;
// d_order: per committee the global indices of its rows with valid set, in the text order of str(vk), stable
int fz_launch_vk_order(fz_ctx *ctx, const int32_t *d_vk, int degree, const void *grp, size_t G, const uint8_t *valid, uint32_t *d_order);
// d_vk [N][2][degree] -> d_left [N][degree], d_right [N][degree] (degree a power of two >= 4, 16-byte aligned pointers)
int fz_launch_vk_halves(fz_ctx *ctx, const int32_t *d_vk, size_t N, int degree, int32_t *d_left, int32_t *d_right);

// launchers of the streaming kernels (fz_pointwise.hip; fz_launch_aggregate: fz_aggregate.hip)
int fz_launch_fill_synthetic(fz_ctx *ctx, int32_t *out, size_t count, unsigned long long seed);
int fz_launch_bcast_rows(fz_ctx *ctx, const int32_t *in, int32_t *out, size_t segments, int l);
enum { FZ_OP_MUL = 0, FZ_OP_ADD = 1, FZ_OP_SUB = 2, FZ_OP_NEG = 3, FZ_OP_MULACC = 4 };
int fz_launch_pw(fz_ctx *ctx, int op, const int32_t *a, const int32_t *b, int32_t *out, size_t count);
int fz_launch_pw_bcast(fz_ctx *ctx, const int32_t *a, const int32_t *s, int32_t *out, size_t rows);
int fz_launch_matvec(fz_ctx *ctx, const int32_t *A, const int32_t *S, int32_t *out, size_t batch, int l);
int fz_launch_sign(fz_ctx *ctx, const int32_t *sk_hat, const int32_t *c_hat, int32_t *sig, size_t batch, int l);
int fz_launch_aggregate(fz_ctx *ctx, const int32_t *sig, const int32_t *alpha, int64_t *out64, size_t pstride,
                        int32_t *out32, size_t groups, size_t N, int l, const int32_t *vkL = nullptr,
                        const int32_t *vkR = nullptr, const int32_t *c = nullptr, int64_t *tout64 = nullptr, size_t tstride = 0,
                        const size_t *h_offsets = nullptr, const int32_t *sk_hat = nullptr, int32_t *sig_out = nullptr);
int fz_launch_target_partial(fz_ctx *ctx, const int32_t *vkL, const int32_t *vkR, const int32_t *c, const int32_t *alpha,
                             int64_t *partial, size_t pstride, size_t groups, size_t N);
int fz_launch_reduce_i64(fz_ctx *ctx, const int64_t *in, int32_t *out, size_t count);
int fz_launch_norm_weight(fz_ctx *ctx, const int32_t *coef, size_t batch, int64_t *max_abs, int32_t *weight);
int fz_launch_verdict(fz_ctx *ctx, const int32_t *target, const int32_t *observed, const int64_t *max_abs,
                      const int32_t *weight, size_t groups, int l, int64_t beta, int64_t omega, int *d_verdict);

#endif
