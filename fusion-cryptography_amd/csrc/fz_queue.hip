// fz_queue.hip -- asynchronous batch queue below the host language (C ABI section "asynchronous batch queue").
//
// The reference is called once per key and once per signature (fusion/fusion.py:338-373 keygen, :534-557 sign) and once per
// aggregate (:655-677, :680-728).  One such call is a latency chain that leaves most of the chip idle (0.93 M pairs/s from one
// host thread at 1024 keys per call: profiles/r03_concurrent_batches.txt; an aggregate of a few dozen signers is a launch at the
// dispatch floor behind milliseconds of host hashing).  The queue closes that gap below Python:
//
//   * a submit copies the call's inputs (seeds or keys, message bytes), hands back a ticket and returns -- microseconds;
//   * W worker threads, each owning a context, a HIP stream and its scratch, take EVERYTHING that is pending of one kind (up to
//     max_rows rows) as ONE batch: every row is independent, so n calls of 1024 rows are one launch sequence of n * 1024 rows;
//     results are cut back into the calls' rows, bit-identical to separate calls (tests/test_gpu_queue.py);
//   * while one worker's batch sits in a latency-bound kernel another worker's batch runs beside it (W streams);
//   * keygen + sign: verification keys go back to the callers' (pinned: fz_pinned_alloc) buffers with asynchronous copies; secret
//     keys and signatures stay in device memory, owned by the batch and freed when every call of it has been released;
//   * aggregate + verify and verify: the challenge pipeline of all signers in one launch sequence, hash_ag's serial sponge of
//     every aggregate on its own host thread, then ONE ragged launch for all partial sums and ONE for all verdicts.
//
// One context still serves one host thread: a worker's context is touched by that worker alone (the blocks of released batches
// are handed back to the worker to free).  No C++ exception leaves a worker thread or crosses the C ABI.
// tests/test_queue_host.py runs this unit on the CPU, and holds the order of its runtime calls against a recorded trace.
#include "fz_internal.h"
#include "../../include/fusion_hip.h"

#include <atomic>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <unordered_map>
#include <unordered_set>
#include <utility>
#include <vector>

namespace {

struct Worker;

struct Batch {                         // device results of one coalesced batch, shared by its calls
    Worker *owner;
    int32_t *d_sk = nullptr, *d_vk = nullptr, *d_sig = nullptr;      // fz_malloc blocks of the owner's context (nullptr: worker scratch, not kept)
    std::atomic<int> refs{0};
    // events recorded on CONSUMERS' streams behind their last use of the rows (fz_queue_release_after); the worker's stream
    // waits for every one of them before the blocks go back to the pool, whose reuse is ordered on the worker's stream only
    // (guarded by the queue's mutex until the batch is garbage, then the worker's alone)
    std::vector<hipEvent_t> after;
};

enum { KIND_KEYGEN_SIGN = 0, KIND_AGGREGATE_VERIFY = 1, KIND_VERIFY = 2 };

struct Job {
    uint64_t ticket;
    size_t n;
    int flags;
    std::vector<uint64_t> seeds;
    std::string msgs;
    std::vector<size_t> off;           // n + 1 offsets into msgs
    int32_t *h_vk_out = nullptr;       // [n][2][degree] or nullptr
    // aggregate / verify calls
    int kind = KIND_KEYGEN_SIGN;
    std::vector<int32_t> vk;           // [n][2][degree]: public keys, copied at submit (2 KiB per signer)
    const int32_t *rows = nullptr;     // KIND_AGGREGATE_VERIFY: the signatures [n][rank][degree]; KIND_VERIFY: the aggregate [rank][degree]
                                       // (caller-owned, valid until the call has finished; host unless FZ_QUEUE_ROWS_ON_DEVICE)
    int32_t *h_agg_out = nullptr;      // [rank][degree] or nullptr
    int *h_verdict_out = nullptr;      // FZ_VERDICT_* or nullptr
};

struct Done {
    int status;
    std::string error;
    Batch *batch;
    size_t row0, n;
    bool keep_sk;                      // this call asked for its secret keys (another call of the batch may have: the batch then holds them)
};

// What a worker holds in device memory besides the batches it hands out, in the order its thread's exit frees them.  Each area
// grows on its own (fit) and is the worker's until then.
enum Area {
    S_COEF, S_C, S_SK, S_VK, S_SIG,    // keygen + sign: secret polynomials, challenges, and -- for batches nobody keeps -- keys and signatures
    W_A,                               // the matrix A [rank][degree], from fz_queue_create on
    A_SIG, A_VK, A_L, A_R, A_C, A_AL, A_AGG, A_TGT, A_VERD,       // aggregate / verify: everything is scratch (results go to the callers' host buffers)
    A_PSUM, A_TSUM,                    // ... and the exact int64 sums
    AREA_COUNT
};

struct Worker {
    std::thread th;
    fz_ctx *ctx = nullptr;
    void *stream = nullptr;
    struct { void *p = nullptr; size_t rows = 0; } area[AREA_COUNT];
    std::vector<Batch *> garbage;      // released batches, freed by the worker itself (guarded by the queue's mutex)
    const int32_t *d_A() const { return (const int32_t *)area[W_A].p; }
};

}  // namespace

struct fz_queue {
    int device, l, degree;
    fz_scheme_params P;
    int64_t beta_sk, omega_sk;
    size_t max_rows;
    std::vector<int32_t> A;
    std::mutex mu;
    std::condition_variable cv_work, cv_done;
    std::deque<Job> pending;
    std::unordered_map<uint64_t, Done> done;        // finished calls whose results (or error) somebody may still ask for
    std::unordered_set<uint64_t> live;              // submitted, not finished
    int first_error = FZ_OK;                        // of a FZ_QUEUE_DISCARD call since the last drain
    std::string first_error_text;
    uint64_t next_ticket = 1;
    size_t inflight = 0;               // submitted and not yet completed
    bool stopping = false;
    std::vector<Worker> workers;       // (never resized once the threads run: a Batch points at its owner)
    uint64_t st_jobs = 0, st_batches = 0, st_rows = 0;
    // aggregate / verify calls (fz_queue_enable_aggregate)
    bool agg_enabled = false;
    int64_t beta_vf = 0, omega_vf = 0;
    size_t capacity = 0;
    int host_threads = 1;
};

namespace {

// Area `which` with room for `rows` rows of `row_bytes`: kept while it is large enough, else freed and allocated anew (nothing in
// it outlives a batch).  rc is sticky: after a failure (nullptr) the fits that follow do nothing, so a run of them is tested once.
template <class T = int32_t>
T *fit(Worker &w, Area which, size_t rows, size_t row_bytes, int &rc) {
    auto &a = w.area[which];
    if (rc != FZ_OK) return nullptr;
    if (rows <= a.rows) return (T *)a.p;
    if (a.p) {
        rc = fz_free(w.ctx, a.p);
        a.p = nullptr;
        a.rows = 0;
        if (rc != FZ_OK) return nullptr;
    }
    if ((rc = fz_malloc(w.ctx, rows * row_bytes, &a.p)) != FZ_OK) return nullptr;
    a.rows = rows;
    return (T *)a.p;
}

// (the owner's thread, or fz_queue_create before the thread exists)
void worker_close(Worker &w) {
    if (!w.ctx) return;
    for (auto &a : w.area)
        if (a.p) (void)fz_free(w.ctx, a.p);
    (void)fz_ctx_set_stream(w.ctx, nullptr);
    if (w.stream) (void)fz_stream_destroy(w.ctx, w.stream);
    (void)fz_ctx_destroy(w.ctx);
    w.ctx = nullptr;
}

void free_batch(Batch *b) {                         // (the owner's thread)
    Worker &w = *b->owner;
    for (hipEvent_t ev : b->after) {                // the consumers' kernels first: fz_free orders reuse behind THIS stream
        (void)hipStreamWaitEvent((hipStream_t)w.stream, ev, 0);
        (void)hipEventDestroy(ev);                  // (released by the runtime once the wait above has been satisfied)
    }
    if (b->d_sk) (void)fz_free(w.ctx, b->d_sk);
    if (b->d_vk) (void)fz_free(w.ctx, b->d_vk);
    if (b->d_sig) (void)fz_free(w.ctx, b->d_sig);
    delete b;
}
struct BatchFree { void operator()(Batch *b) const { free_batch(b); } };
using BatchPtr = std::unique_ptr<Batch, BatchFree>;     // a batch on its way to its calls: every failing exit frees its blocks

// the calls of one batch back to back
struct Coalesced {
    std::vector<size_t> row0;          // [calls + 1]: each call's first row, then the total
    std::string msgs;                  // the calls' message bytes
    std::vector<size_t> off;           // [total + 1]: the rows' offsets into msgs
    size_t rows() const { return row0.back(); }
};
void coalesce(const std::vector<Job> &jobs, Coalesced &c) {
    size_t msg_bytes = 0;
    c.row0.assign(1, 0);
    c.row0.reserve(jobs.size() + 1);
    for (auto &j : jobs) { c.row0.push_back(c.row0.back() + j.n); msg_bytes += j.msgs.size(); }
    c.msgs.reserve(msg_bytes);
    c.off.reserve(c.rows() + 1);
    c.off.push_back(0);
    for (auto &j : jobs) {
        const size_t base = c.msgs.size();
        c.msgs += j.msgs;
        for (size_t i = 1; i <= j.n; ++i) c.off.push_back(base + j.off[i]);
    }
}

// one coalesced batch of keygen + sign calls; *out: the blocks its kept calls share (none: a batch nobody keeps ran in scratch)
int run_batch(fz_queue *Q, Worker &w, std::vector<Job> &jobs, BatchPtr &out, std::vector<size_t> &row0) {
    const int d = Q->degree, l = Q->l;
    bool keep = false, keep_sk = false;
    for (auto &j : jobs) {
        if (!(j.flags & FZ_QUEUE_DISCARD)) keep = true;
        if ((j.flags & FZ_QUEUE_KEEP_SK) && !(j.flags & FZ_QUEUE_DISCARD)) keep_sk = true;
    }
    Coalesced c;
    coalesce(jobs, c);
    const size_t N = c.rows(), poly = (size_t)d * 4;
    std::vector<uint64_t> seeds;
    seeds.reserve(N);
    for (auto &j : jobs) seeds.insert(seeds.end(), j.seeds.begin(), j.seeds.end());
    int rc = FZ_OK;
    int32_t *d_coef = fit(w, S_COEF, N, 2 * poly, rc), *d_c = fit(w, S_C, N, poly, rc);
    if (rc != FZ_OK) return rc;
    BatchPtr b;
    if (keep) {
        b.reset(new Batch());
        b->owner = &w;
        const struct { int32_t *Batch::*block; size_t bytes; bool wanted; } blocks[3] = {
            {&Batch::d_vk, N * 2 * poly, true}, {&Batch::d_sig, N * (size_t)l * poly, true}, {&Batch::d_sk, N * 2 * (size_t)l * poly, keep_sk}};
        for (auto &blk : blocks) {
            void *p = nullptr;
            if (blk.wanted && (rc = fz_malloc(w.ctx, blk.bytes, &p)) != FZ_OK) return rc;
            (*b).*blk.block = (int32_t *)p;
        }
    }
    int32_t *d_sk = (b && b->d_sk) ? b->d_sk : fit(w, S_SK, N, 2 * (size_t)l * poly, rc);
    int32_t *d_vk = b ? b->d_vk : fit(w, S_VK, N, 2 * poly, rc);
    int32_t *d_sig = b ? b->d_sig : fit(w, S_SIG, N, (size_t)l * poly, rc);
    if (rc != FZ_OK) return rc;
    // the path itself, exactly what BatchScheme.keygen_batch + sign_batch issue for one call (fusion.py:338-373, :534-557)
    rc = fz_sample_secret_polys_dev(w.ctx, seeds.data(), N, Q->P.modulus, d, Q->beta_sk, Q->omega_sk, d_coef);
    if (rc == FZ_OK) rc = fz_keygen_core_bcast(w.ctx, w.d_A(), d_coef, d_sk, d_vk, N, l);
    if (rc == FZ_OK) rc = fz_challenge_hat_msgs_dev(w.ctx, &Q->P, d_vk, c.msgs.data(), c.off.data(), N, d_c, nullptr);
    if (rc == FZ_OK) rc = fz_sign_core(w.ctx, d_sk, d_c, d_sig, N, l);
    if (rc == FZ_OK) {
        for (size_t k = 0; k < jobs.size() && rc == FZ_OK; ++k)
            if (jobs[k].h_vk_out)
                rc = fz_check_hip(hipMemcpyAsync(jobs[k].h_vk_out, d_vk + c.row0[k] * 2 * (size_t)d, jobs[k].n * 2 * poly, hipMemcpyDeviceToHost,
                                                 (hipStream_t)w.stream), "queue: verification keys to the host");
        if (rc == FZ_OK) rc = fz_ctx_synchronize(w.ctx);
    } else {
        (void)fz_ctx_synchronize(w.ctx);                    // a failed step: nothing of the batch is in flight when its blocks go back
    }
    if (rc != FZ_OK) return rc;
    out = std::move(b);
    row0 = std::move(c.row0);
    return FZ_OK;
}

// hash_ag (fusion.py:632-652) of every aggregate of a batch: sort by str(vk) (:661-663, :693), ONE serial SHAKE-256, decode; the
// rows of alpha go back to the callers' order (the sums do not care).  Independent aggregates on independent host threads.
int hash_ag_all(const fz_queue *Q, const std::vector<Job> &jobs, const std::vector<size_t> &offs, const int32_t *L, const int32_t *R, const int32_t *c_hat,
                const uint8_t *pre, int32_t *alpha) {
    const size_t d = (size_t)Q->degree, poly = d * 4, G = jobs.size();
    std::atomic<size_t> next(0);
    std::atomic<int> first_rc(FZ_OK);
    auto work = [&]() {
        for (;;) {
            const size_t g = next.fetch_add(1);
            if (g >= G) return;
            int r;
            try {
                const size_t n = jobs[g].n, o = offs[g];
                std::vector<size_t> order(n);
                r = fz_sort_by_vk_string(&Q->P, L + o * d, R + o * d, n, order.data(), 1);
                if (r == FZ_OK) {
                    std::vector<int32_t> sL(n * d), sR(n * d), sC(n * d), sA(n * d);
                    std::vector<uint8_t> sP(n * 32);
                    for (size_t i = 0; i < n; ++i) {
                        const size_t k = o + order[i];
                        memcpy(sL.data() + i * d, L + k * d, poly);
                        memcpy(sR.data() + i * d, R + k * d, poly);
                        memcpy(sC.data() + i * d, c_hat + k * d, poly);
                        memcpy(sP.data() + i * 32, pre + k * 32, 32);
                    }
                    r = fz_aggregation_coefficients(&Q->P, sL.data(), sR.data(), sP.data(), sC.data(), n, sA.data(), 1);
                    if (r == FZ_OK)
                        for (size_t i = 0; i < n; ++i) memcpy(alpha + (o + order[i]) * d, sA.data() + i * d, poly);
                }
            } catch (const std::exception &) {              // (a pool thread: nothing may leave it)
                r = FZ_E_HIP;
            }
            if (r != FZ_OK) { int e = FZ_OK; first_rc.compare_exchange_strong(e, r); }
        }
    };
    const size_t T = std::min<size_t>(G, (size_t)std::max(1, Q->host_threads));
    std::vector<std::thread> pool;
    try {
        for (size_t t = 1; t < T; ++t) pool.emplace_back(work);
    } catch (const std::exception &) {}                     // fewer threads than asked for: the ones that started (and this one) do the work
    work();
    for (auto &th : pool) th.join();
    if (first_rc.load() != FZ_OK) return fz_set_error(first_rc.load(), "queue: hash_ag failed for an aggregate of the batch");
    return FZ_OK;
}

// one coalesced batch of aggregate+verify (kind 1) or verify (kind 2) calls: G aggregates, their signers back to back.
// The flow of BatchScheme._hash_ag_many (the challenge pass and alpha_hat of the call's _Committees) + aggregate_target_partial_ragged
// + verify_partials (fusion_hip/scheme.py), in C.  The keys go up three times (whole, left, right) and are sorted on the host:
// fz_vk_halves_async and the device sort would change the calls this unit makes (docs/HISTORY.md AH).
int run_agg_batch_steps(fz_queue *Q, Worker &w, std::vector<Job> &jobs, int kind);
// Every exit of the steps below that reports a failure may leave copies FROM THE CALLERS' ROWS in flight on the worker's stream
// (they are enqueued first): the stream is drained before the failure is reported, so that a caller who frees or recycles its
// rows on an error never races with them.
int run_agg_batch(fz_queue *Q, Worker &w, std::vector<Job> &jobs, int kind) {
    const int rc = run_agg_batch_steps(Q, w, jobs, kind);
    if (rc != FZ_OK) (void)fz_ctx_synchronize(w.ctx);
    return rc;
}
int run_agg_batch_steps(fz_queue *Q, Worker &w, std::vector<Job> &jobs, int kind) {
    const size_t d = (size_t)Q->degree, l = (size_t)Q->l, poly = d * 4, G = jobs.size();
    const bool agg = kind == KIND_AGGREGATE_VERIFY;
    Coalesced c;
    coalesce(jobs, c);
    const std::vector<size_t> &offs = c.row0;
    const size_t N = c.rows();
    // host staging: keys as one [N][2][d] array and as left / right rows
    std::vector<int32_t> vk(N * 2 * d), L(N * d), R(N * d), c_hat(N * d), alpha(N * d);
    std::vector<uint8_t> pre(N * 32);
    std::vector<int> verdicts(G, FZ_VERDICT_OK);
    for (size_t g = 0; g < G; ++g) memcpy(vk.data() + offs[g] * 2 * d, jobs[g].vk.data(), jobs[g].n * 2 * poly);
    for (size_t i = 0; i < N; ++i) {
        memcpy(L.data() + i * d, vk.data() + (2 * i) * d, poly);
        memcpy(R.data() + i * d, vk.data() + (2 * i + 1) * d, poly);
    }
    int rc = FZ_OK;
    int32_t *a_vk = fit(w, A_VK, N, 2 * poly, rc), *a_L = fit(w, A_L, N, poly, rc), *a_R = fit(w, A_R, N, poly, rc), *a_c = fit(w, A_C, N, poly, rc);
    int32_t *a_al = fit(w, A_AL, N, poly, rc), *a_agg = fit(w, A_AGG, G, l * poly, rc), *a_tgt = fit(w, A_TGT, G, poly, rc);
    int *a_verd = fit<int>(w, A_VERD, G, sizeof(int), rc);
    int64_t *tsum = fit<int64_t>(w, A_TSUM, G, d * 8, rc);
    int32_t *a_sig = agg ? fit(w, A_SIG, N, l * poly, rc) : nullptr;
    int64_t *psum = agg ? fit<int64_t>(w, A_PSUM, G, l * d * 8, rc) : nullptr;
    if (rc != FZ_OK) return rc;
    hipStream_t st = (hipStream_t)w.stream;
    // the callers' rows start their way to the device first (the signatures are the largest transfer, and nothing below needs them
    // before the sums): call g's signatures to its signers' rows, or its aggregate to row g
    for (size_t g = 0; g < G; ++g) {
        const hipMemcpyKind dir = (jobs[g].flags & FZ_QUEUE_ROWS_ON_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        int32_t *dst = agg ? a_sig + offs[g] * l * d : a_agg + g * l * d;
        rc = fz_check_hip(hipMemcpyAsync(dst, jobs[g].rows, (agg ? jobs[g].n : 1) * l * poly, dir, st), agg ? "queue: signatures" : "queue: aggregates");
        if (rc != FZ_OK) return rc;
    }
    // hash_ch of every signer (fusion.py:511-531) on the device; the pre-hashes and c_hat come back for hash_ag's text
    if ((rc = fz_memcpy_h2d(w.ctx, a_vk, vk.data(), N * 2 * poly)) != FZ_OK) return rc;
    if ((rc = fz_challenge_hat_msgs_dev(w.ctx, &Q->P, a_vk, c.msgs.data(), c.off.data(), N, a_c, pre.data())) != FZ_OK) return rc;
    if ((rc = fz_memcpy_d2h(w.ctx, c_hat.data(), a_c, N * poly)) != FZ_OK) return rc;
    if ((rc = hash_ag_all(Q, jobs, offs, L.data(), R.data(), c_hat.data(), pre.data(), alpha.data())) != FZ_OK) return rc;
    if ((rc = fz_memcpy_h2d(w.ctx, a_al, alpha.data(), N * poly)) != FZ_OK) return rc;
    if ((rc = fz_ntt_forward(w.ctx, a_al, a_al, N)) != FZ_OK) return rc;
    if ((rc = fz_memcpy_h2d(w.ctx, a_L, L.data(), N * poly)) != FZ_OK) return rc;
    if ((rc = fz_memcpy_h2d(w.ctx, a_R, R.data(), N * poly)) != FZ_OK) return rc;
    if (agg) {
        // ONE launch: exact int64 partial sums of every aggregate (fusion.py:670-676) and of every verification target (:706-714)
        rc = fz_aggregate_target_partial_ragged(w.ctx, a_sig, a_al, a_L, a_R, a_c, offs.data(), G, (int)l, psum, l * d, tsum, d);
        // ONE launch: every verdict straight from the sums (fusion.py:690-727)
        if (rc == FZ_OK) rc = fz_verify_partials_batch_async(w.ctx, w.d_A(), psum, l * d, tsum, d, G, (int)l, Q->beta_vf, Q->omega_vf, a_verd);
        if (rc == FZ_OK) rc = fz_reduce_i64(w.ctx, psum, a_agg, G * l * d);
        for (size_t g = 0; g < G && rc == FZ_OK; ++g)
            if (jobs[g].h_agg_out)
                rc = fz_check_hip(hipMemcpyAsync(jobs[g].h_agg_out, a_agg + g * l * d, l * poly, hipMemcpyDeviceToHost, st), "queue: aggregate to the host");
    } else {
        rc = fz_aggregate_target_partial_ragged(w.ctx, nullptr, a_al, a_L, a_R, a_c, offs.data(), G, (int)l, nullptr, 0, tsum, d);
        if (rc == FZ_OK) rc = fz_reduce_i64(w.ctx, tsum, a_tgt, G * d);
        if (rc == FZ_OK) rc = fz_verify_with_target_batch_async(w.ctx, w.d_A(), a_agg, a_tgt, G, (int)l, Q->beta_vf, Q->omega_vf, a_verd);
    }
    if (rc == FZ_OK) rc = fz_memcpy_d2h(w.ctx, verdicts.data(), a_verd, G * sizeof(int));       // (synchronises the stream)
    else (void)fz_ctx_synchronize(w.ctx);
    if (rc != FZ_OK) return rc;
    for (size_t g = 0; g < G; ++g)
        if (jobs[g].h_verdict_out)                             // fusion.py:686-687: the capacity is checked before anything else
            *jobs[g].h_verdict_out = jobs[g].n > Q->capacity ? FZ_VERDICT_TOO_MANY_KEYS : verdicts[g];
    return FZ_OK;
}
// ---- a worker's thread: free what was released, take a batch, run it, complete its calls -------------------------------------

// (under Q->mu) the queue's first error since the last drain: of a FZ_QUEUE_DISCARD call, or of a result that could not be stored
void note_first_error(fz_queue *Q, int rc, const char *text) {
    if (Q->first_error != FZ_OK) return;
    Q->first_error = rc;
    try { Q->first_error_text = text; } catch (const std::bad_alloc &) {}
}

bool free_garbage(Worker &w, std::unique_lock<std::mutex> &lk) {
    if (w.garbage.empty()) return false;
    std::vector<Batch *> g;
    g.swap(w.garbage);
    lk.unlock();
    for (Batch *b : g) free_batch(b);
    lk.lock();
    return true;
}

// (under Q->mu, something is pending) everything that is pending, up to max_rows rows: one batch.  Calls are taken in order and
// a batch is a run of calls of ONE kind; what is left (another kind, or over max_rows) is another worker's.  -> the batch's rows
size_t take_batch(fz_queue *Q, std::vector<Job> &jobs) {
    size_t rows = 0;
    const int kind = Q->pending.front().kind;
    while (!Q->pending.empty() && Q->pending.front().kind == kind && (jobs.empty() || rows + Q->pending.front().n <= Q->max_rows)) {
        rows += Q->pending.front().n;
        jobs.push_back(std::move(Q->pending.front()));
        Q->pending.pop_front();
    }
    if (!Q->pending.empty()) Q->cv_work.notify_one();
    return rows;
}

struct Ran { int rc = FZ_OK; std::string err; BatchPtr batch; std::vector<size_t> row0; };

void run(fz_queue *Q, Worker &w, std::vector<Job> &jobs, Ran &r) {
    try {
        r.rc = jobs[0].kind == KIND_KEYGEN_SIGN ? run_batch(Q, w, jobs, r.batch, r.row0) : run_agg_batch(Q, w, jobs, jobs[0].kind);
    } catch (const std::exception &) {              // the coalesced host copies (bad_alloc) or a thread that would not start: an error of these calls, not std::terminate
        (void)fz_ctx_synchronize(w.ctx);
        r.rc = fz_set_error(FZ_E_HIP, "queue worker: out of host memory while coalescing %zu calls", jobs.size());
    }
    try {
        if (r.rc != FZ_OK) r.err = fz_last_error();
    } catch (const std::bad_alloc &) {}
}

// (under Q->mu) Completion bookkeeping: nothing here may leave the thread as an exception (std::terminate in a library thread).
// A record that cannot be stored (out of host memory) is reported through fz_queue_drain's first error and the call's ticket then
// reads as finished-with-nothing.
void complete(fz_queue *Q, Worker &w, std::unique_lock<std::mutex> &lk, const std::vector<Job> &jobs, size_t rows, Ran &r) {
    Batch *b = r.batch.release();
    int kept = 0;
    for (size_t k = 0; k < jobs.size(); ++k) {
        Q->live.erase(jobs[k].ticket);
        if (jobs[k].flags & FZ_QUEUE_DISCARD) {                 // fire and forget: only a failure is remembered (for fz_queue_drain)
            if (r.rc != FZ_OK) note_first_error(Q, r.rc, r.err.c_str());
            continue;
        }
        try {
            Q->done.emplace(jobs[k].ticket, Done{r.rc, r.err, b, k < r.row0.size() ? r.row0[k] : 0, jobs[k].n, (jobs[k].flags & FZ_QUEUE_KEEP_SK) != 0});
            if (b) ++kept;
        } catch (const std::bad_alloc &) {
            note_first_error(Q, FZ_E_HIP, "out of host memory while recording a call's result");
        }
    }
    if (b) {
        if (kept) b->refs = kept;
        else {
            try { w.garbage.push_back(b); }
            catch (const std::bad_alloc &) { lk.unlock(); free_batch(b); lk.lock(); }
        }
    }
    Q->inflight -= jobs.size();
    Q->st_jobs += jobs.size();
    Q->st_batches += 1;
    Q->st_rows += rows;
    Q->cv_done.notify_all();
}

void worker_main(fz_queue *Q, int index) {
    Worker &w = Q->workers[index];
    (void)hipSetDevice(Q->device);                  // a new thread starts on device 0; every fz_* call below selects the context's device again
    std::unique_lock<std::mutex> lk(Q->mu);
    for (;;) {
        Q->cv_work.wait(lk, [&] { return Q->stopping || !Q->pending.empty() || !w.garbage.empty(); });
        if (free_garbage(w, lk)) continue;
        if (Q->pending.empty()) {
            if (Q->stopping) break;
            continue;
        }
        std::vector<Job> jobs;
        const size_t rows = take_batch(Q, jobs);
        lk.unlock();
        Ran r;
        run(Q, w, jobs, r);
        lk.lock();
        complete(Q, w, lk, jobs, rows, r);
    }
    lk.unlock();
    worker_close(w);
}

int worker_init(fz_queue *Q, Worker &w) {
    int rc = fz_ctx_create(Q->device, (uint32_t)Q->P.modulus, Q->degree, (uint32_t)Q->P.root, (uint32_t)Q->P.inv_root, &w.ctx);
    if (rc != FZ_OK) return rc;
    if ((rc = fz_stream_create(w.ctx, &w.stream)) != FZ_OK) return rc;
    if ((rc = fz_ctx_set_stream(w.ctx, w.stream)) != FZ_OK) return rc;
    int32_t *d_A = fit(w, W_A, (size_t)Q->l, (size_t)Q->degree * 4, rc);
    if (rc != FZ_OK) return rc;
    if ((rc = fz_memcpy_h2d(w.ctx, d_A, Q->A.data(), Q->A.size() * 4)) != FZ_OK) return rc;
    return fz_ctx_synchronize(w.ctx);
}

// ---- what the submits share ---------------------------------------------------------------------------------------------------

// The rules of a call's rows, tested row by row in this order (the earlier row names the refusal): offsets from 0, not decreasing;
// no seed 2^64 - 1 (h_seeds NULL: the call has no seeds); bytes only with a text.
int check_rows(const char *h_msgs, const size_t *h_msg_off, size_t n, const uint64_t *h_seeds) {
    if (h_msg_off[0] != 0) return fz_set_error(FZ_E_BADARG, "h_msg_off[0] must be 0");
    for (size_t i = 0; i < n; ++i) {
        if (h_msg_off[i + 1] < h_msg_off[i]) return fz_set_error(FZ_E_BADARG, "message offsets must not decrease");
        if (h_seeds && h_seeds[i] == ~0ull) return fz_set_error(FZ_E_UNSUPPORTED, "seed 2^64 - 1: seed + 1 wraps (use the Python sampler)");
    }
    if (h_msg_off[n] && !h_msgs) return fz_set_error(FZ_E_BADARG, "h_msgs is NULL");
    return FZ_OK;
}

// A call of n rows joins the queue: fill(job) copies its own inputs (outside the lock), the messages are copied here.  Whatever
// can throw does so before the queue's state changes, and no C++ exception crosses the C ABI.
template <class Fill>
int enqueue(fz_queue *Q, size_t n, const char *h_msgs, const size_t *h_msg_off, int flags, uint64_t *out_ticket, Fill fill) {
    try {
        Job j;
        j.n = n;
        j.flags = flags;
        fill(j);
        j.msgs.assign(h_msgs ? h_msgs : "", h_msg_off[n]);
        j.off.assign(h_msg_off, h_msg_off + n + 1);
        std::lock_guard<std::mutex> lk(Q->mu);
        if (Q->stopping) return fz_set_error(FZ_E_BADARG, "the queue is shutting down");
        Q->live.reserve(Q->live.size() + 1);
        Q->pending.push_back(std::move(j));
        Job &q = Q->pending.back();
        q.ticket = Q->next_ticket++;
        *out_ticket = q.ticket;
        Q->live.insert(q.ticket);
        Q->inflight += 1;
    } catch (const std::bad_alloc &) {
        return fz_set_error(FZ_E_HIP, "out of host memory while copying the call's inputs");
    }
    Q->cv_work.notify_one();
    return FZ_OK;
}

// (under Q->mu) waits until the call of `ticket` has finished; *out: its record, or NULL (a FZ_QUEUE_DISCARD call, or released before)
int finished(fz_queue *Q, std::unique_lock<std::mutex> &lk, uint64_t ticket, Done **out) {
    *out = nullptr;
    if (ticket == 0 || ticket >= Q->next_ticket) return fz_set_error(FZ_E_BADARG, "unknown ticket");
    Q->cv_done.wait(lk, [&] { return Q->live.count(ticket) == 0; });
    auto it = Q->done.find(ticket);
    if (it != Q->done.end()) *out = &it->second;
    return FZ_OK;
}

struct EventGuard {                    // an event nobody has taken over is destroyed on the way out
    hipEvent_t ev = nullptr;
    void reset() { if (ev) (void)hipEventDestroy(ev); ev = nullptr; }
    ~EventGuard() { reset(); }
};

}  // namespace

extern "C" {

int fz_pinned_alloc(size_t bytes, void **h_out) {
    if (!h_out) return fz_set_error(FZ_E_BADARG, "h_out is NULL");
    *h_out = nullptr;
    return fz_check_hip(hipHostMalloc(h_out, bytes ? bytes : 1, hipHostMallocDefault), "pinned host allocation");
}

int fz_pinned_free(void *h_ptr) {
    if (!h_ptr) return FZ_OK;
    return fz_check_hip(hipHostFree(h_ptr), "pinned host free");
}

int fz_queue_create(int device, const fz_scheme_params *P, int rank, int64_t beta_sk, int64_t omega_sk, const int32_t *h_A,
                    int workers, size_t max_rows, fz_queue **out) {
    if (!P || !h_A || !out) return fz_set_error(FZ_E_BADARG, "NULL argument");
    *out = nullptr;
    if (rank < 1 || workers < 1 || workers > 16 || max_rows < 1)
        return fz_set_error(FZ_E_BADARG, "rank >= 1, 1 <= workers <= 16, max_rows >= 1");
    if (P->modulus <= 0 || P->modulus >= (1ll << 32) || P->degree < 1) return fz_set_error(FZ_E_BADARG, "bad parameter set");
    fz_queue *Q = new (std::nothrow) fz_queue();
    if (!Q) return fz_set_error(FZ_E_HIP, "out of host memory");
    Q->device = device;
    Q->l = rank;
    Q->degree = P->degree;
    Q->P = *P;
    Q->beta_sk = beta_sk;
    Q->omega_sk = omega_sk;
    Q->max_rows = max_rows;
    Q->A.assign(h_A, h_A + (size_t)rank * P->degree);
    Q->workers.resize((size_t)workers);
    // contexts are created HERE, on the caller's thread (errors come back as this call's error), then handed to the threads
    for (auto &w : Q->workers) {
        const int rc = worker_init(Q, w);
        if (rc != FZ_OK) {
            for (auto &v : Q->workers) worker_close(v);
            delete Q;
            return rc;
        }
    }
    for (int i = 0; i < workers; ++i) Q->workers[(size_t)i].th = std::thread(worker_main, Q, i);
    *out = Q;
    return FZ_OK;
}

int fz_queue_destroy(fz_queue *Q) {
    if (!Q) return FZ_OK;
    {
        std::unique_lock<std::mutex> lk(Q->mu);
        // what was submitted is finished first; results nobody released go back to their workers
        Q->cv_done.wait(lk, [&] { return Q->inflight == 0; });
        for (auto &kv : Q->done)
            if (kv.second.batch && --kv.second.batch->refs == 0) kv.second.batch->owner->garbage.push_back(kv.second.batch);
        Q->done.clear();
        Q->stopping = true;
        Q->cv_work.notify_all();
    }
    for (auto &w : Q->workers)
        if (w.th.joinable()) w.th.join();
    delete Q;
    return FZ_OK;
}

int fz_queue_submit_keygen_sign(fz_queue *Q, const uint64_t *h_seeds, size_t n, const char *h_msgs, const size_t *h_msg_off,
                                int32_t *h_vk_out, int flags, uint64_t *out_ticket) {
    if (!Q || !out_ticket || (n && (!h_seeds || !h_msg_off))) return fz_set_error(FZ_E_BADARG, "NULL argument");
    if (n == 0 || n > Q->max_rows) return fz_set_error(FZ_E_BADARG, "between 1 and max_rows (%zu) keys per call", Q->max_rows);
    const int rc = check_rows(h_msgs, h_msg_off, n, h_seeds);
    if (rc != FZ_OK) return rc;
    return enqueue(Q, n, h_msgs, h_msg_off, flags, out_ticket, [&](Job &j) {
        j.seeds.assign(h_seeds, h_seeds + n);
        j.h_vk_out = h_vk_out;
    });
}

int fz_queue_enable_aggregate(fz_queue *Q, int64_t beta_vf, int64_t omega_vf, size_t capacity, int host_threads) {
    if (!Q) return fz_set_error(FZ_E_BADARG, "queue is NULL");
    if (beta_vf < 0 || omega_vf < 0 || capacity < 1 || host_threads < 1 || host_threads > 256)
        return fz_set_error(FZ_E_BADARG, "bounds >= 0, capacity >= 1, 1 <= host_threads <= 256");
    std::lock_guard<std::mutex> lk(Q->mu);
    Q->beta_vf = beta_vf;
    Q->omega_vf = omega_vf;
    Q->capacity = capacity;
    Q->host_threads = host_threads;
    Q->agg_enabled = true;
    return FZ_OK;
}

static int submit_agg(fz_queue *Q, int kind, const int32_t *h_vk, const char *h_msgs, const size_t *h_msg_off, size_t n, const int32_t *rows,
                      int32_t *h_agg_out, int *h_verdict_out, int flags, uint64_t *out_ticket) {
    if (!Q || !out_ticket || !h_vk || !h_msg_off || !rows) return fz_set_error(FZ_E_BADARG, "NULL argument");
    if (!Q->agg_enabled) return fz_set_error(FZ_E_BADARG, "fz_queue_enable_aggregate has not been called");
    if (n == 0 || n > Q->max_rows) return fz_set_error(FZ_E_BADARG, "between 1 and max_rows (%zu) signers per call", Q->max_rows);
    if (n >= ((size_t)1 << 21)) return fz_set_error(FZ_E_UNSUPPORTED, "too many signers for exact accumulation (< 2^21)");
    const int rc = check_rows(h_msgs, h_msg_off, n, nullptr);
    if (rc != FZ_OK) return rc;
    if (flags & ~FZ_QUEUE_ROWS_ON_DEVICE) return fz_set_error(FZ_E_BADARG, "only FZ_QUEUE_ROWS_ON_DEVICE applies to aggregate / verify calls");
    return enqueue(Q, n, h_msgs, h_msg_off, flags, out_ticket, [&](Job &j) {
        j.kind = kind;
        j.vk.assign(h_vk, h_vk + n * 2 * (size_t)Q->degree);
        j.rows = rows;
        j.h_agg_out = h_agg_out;
        j.h_verdict_out = h_verdict_out;
    });
}

int fz_queue_submit_aggregate_verify(fz_queue *Q, const int32_t *h_vk, const char *h_msgs, const size_t *h_msg_off, size_t n,
                                     const int32_t *sig, int32_t *h_agg_out, int *h_verdict_out, int flags, uint64_t *out_ticket) {
    return submit_agg(Q, KIND_AGGREGATE_VERIFY, h_vk, h_msgs, h_msg_off, n, sig, h_agg_out, h_verdict_out, flags, out_ticket);
}

int fz_queue_submit_verify(fz_queue *Q, const int32_t *h_vk, const char *h_msgs, const size_t *h_msg_off, size_t n,
                           const int32_t *aggregate, int *h_verdict_out, int flags, uint64_t *out_ticket) {
    if (!h_verdict_out) return fz_set_error(FZ_E_BADARG, "h_verdict_out is NULL");
    return submit_agg(Q, KIND_VERIFY, h_vk, h_msgs, h_msg_off, n, aggregate, nullptr, h_verdict_out, flags, out_ticket);
}

int fz_queue_wait(fz_queue *Q, uint64_t ticket, fz_queue_result *out) {
    if (!Q) return fz_set_error(FZ_E_BADARG, "queue is NULL");
    std::unique_lock<std::mutex> lk(Q->mu);
    Done *dn;
    const int rc = finished(Q, lk, ticket, &dn);
    if (rc != FZ_OK) return rc;
    if (out) memset(out, 0, sizeof(*out));
    if (!dn) return FZ_OK;                                   // finished, nothing to hand out
    if (out) {
        out->status = dn->status;
        out->n = dn->n;
        if (dn->batch) {
            const size_t d = (size_t)Q->degree, l = (size_t)Q->l;
            out->d_vk = dn->batch->d_vk + dn->row0 * 2 * d;
            out->d_sig = dn->batch->d_sig + dn->row0 * l * d;
            out->d_sk_hat = (dn->keep_sk && dn->batch->d_sk) ? dn->batch->d_sk + dn->row0 * 2 * l * d : nullptr;
        }
    }
    if (dn->status != FZ_OK) return fz_set_error(dn->status, "queued batch failed: %s", dn->error.c_str());
    return FZ_OK;
}

// consumer != NULL: the rows may still be in use by work ALREADY QUEUED on the consumer's stream -- an event recorded there now
// is what the owning worker's stream waits for before the blocks return to the pool (the pool orders reuse on the worker's stream
// only, so a release right behind an asynchronous kernel on the rows would let the next batch overwrite them)
static int queue_release(fz_queue *Q, uint64_t ticket, fz_ctx *consumer) {
    if (!Q) return fz_set_error(FZ_E_BADARG, "queue is NULL");
    EventGuard e;
    int rc = FZ_OK;
    if (consumer) {
        if (hipSetDevice(consumer->device) != hipSuccess) return fz_set_error(FZ_E_HIP, "cannot select the consumer's device");
        rc = fz_check_hip(hipEventCreateWithFlags(&e.ev, hipEventDisableTiming), "queue: release event");
        if (rc == FZ_OK) rc = fz_check_hip(hipEventRecord(e.ev, consumer->stream), "queue: release event record");
        if (rc != FZ_OK) return rc;
    }
    std::unique_lock<std::mutex> lk(Q->mu);
    Done *dn;
    if ((rc = finished(Q, lk, ticket, &dn)) != FZ_OK || !dn) return rc;      // (released before: idempotent)
    Batch *b = dn->batch;
    Q->done.erase(ticket);
    if (!b) return FZ_OK;
    if (e.ev) {
        try { b->after.push_back(e.ev); e.ev = nullptr; }
        catch (const std::bad_alloc &) {}
    }
    if (e.ev) {                                             // could not be attached: wait for the consumer here instead
        lk.unlock();
        rc = fz_check_hip(hipEventSynchronize(e.ev), "queue: release event wait");
        e.reset();
        lk.lock();
    }
    if (--b->refs == 0) {
        try { b->owner->garbage.push_back(b); }
        catch (const std::bad_alloc &) { ++b->refs; return fz_set_error(FZ_E_HIP, "out of host memory while releasing a call"); }
        Q->cv_work.notify_all();
    }
    return rc;
}

int fz_queue_release(fz_queue *Q, uint64_t ticket) { return queue_release(Q, ticket, nullptr); }

int fz_queue_release_after(fz_queue *Q, uint64_t ticket, fz_ctx *consumer) {
    if (!consumer) return fz_set_error(FZ_E_BADARG, "consumer context is NULL (fz_queue_release is the form without one)");
    return queue_release(Q, ticket, consumer);
}

int fz_queue_drain(fz_queue *Q) {
    if (!Q) return fz_set_error(FZ_E_BADARG, "queue is NULL");
    std::unique_lock<std::mutex> lk(Q->mu);
    Q->cv_done.wait(lk, [&] { return Q->inflight == 0; });
    const int rc = std::exchange(Q->first_error, FZ_OK);
    if (rc == FZ_OK) return FZ_OK;
    const std::string text = std::move(Q->first_error_text);
    Q->first_error_text.clear();
    return fz_set_error(rc, "a discarded call failed: %s", text.c_str());
}

int fz_queue_stats(fz_queue *Q, uint64_t *out_calls, uint64_t *out_batches, uint64_t *out_rows) {
    if (!Q) return fz_set_error(FZ_E_BADARG, "queue is NULL");
    std::lock_guard<std::mutex> lk(Q->mu);
    if (out_calls) *out_calls = Q->st_jobs;
    if (out_batches) *out_batches = Q->st_batches;
    if (out_rows) *out_rows = Q->st_rows;
    return FZ_OK;
}

}  // extern "C"
