"""The batch queue (csrc/fz_queue.hip) without a GPU: its coalescing, row ownership, error paths, refusals and locking.

fz_queue.hip, fz_context.hip and fz_diag.hip are compiled for the host and linked, as a stand-alone program, with the real
fz_host.cpp, the stub HIP runtime of tests/_hip_stub.py and the driver below.  Contexts, streams, fz_malloc / fz_free, the error
text, fz_sort_by_vk_string and fz_aggregation_coefficients are the product's own code; the driver supplies only the nine compute
entries the queue calls, as a MODEL SCHEME in plain loops mod q on the stub's "device" memory (host memory).  The model has the
scheme's linear shape (fz_pointwise.hip, fz_aggregate.hip: sig = L (.) c + R per row, vk = A . sk, target = sum (vkL (.) c + vkR)
(.) alpha_hat), is row-wise and deterministic, and its challenge depends on every byte of a signer's message: an honest aggregate
verifies, one coefficient off by one does not, and a wrong row0, message offset or scatter of alpha gives other integers.  Every
model entry records its arguments and the calling thread, can block on a gate and can fail on its k-th call -- controls of the
driver, not of the product.  Every expected value is the model applied to that call's inputs alone; comparisons are exact.

The program runs with FZ_POOL_MB=0 (every fz_free is a hipFree: AddressSanitizer sees a read of a block that went back too
early) in three builds: address + undefined behaviour with leak detection, ThreadSanitizer, and no sanitizer.  Scenarios
S1 .. S11 are listed at their functions.

With "trace" as its argument the program prints, instead, the trace of fixed one-worker flows, one line per event: every call of
the stub runtime (function, bytes -- for a free, the bytes of its block --, copy kind, the caller's or the worker's thread, the
worker's stream, a consumer's or none), every model entry (entry, N, G, offsets, sig_null), every refusal of S8 and every batch
failure with its code and its whole error text; no addresses, no tickets.  tests/golden/queue_runtime_trace.txt is that output
of the unit as it was BEFORE its steps were written once (docs/HISTORY.md AH); all three builds must print exactly it, so a
runtime call, allocation or copy that moved, changed thread or changed stream shows as a differing line.  The one path the trace
cannot reach is fz_queue_release_after waiting on its event itself: it needs std::vector::push_back to throw under the queue's
mutex, and the stub's controls fail device allocations and event creations only."""
import os
import subprocess

import pytest

from _hip_stub import CSRC, STUB, build_driver, sanitizer_links, toolchain

UNITS = ("fz_queue", "fz_context", "fz_diag")

DRIVER = STUB + r'''
#include <chrono>
#include <condition_variable>
#include <deque>
#include <map>
#include <memory>
#include <thread>

#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s   (last error: %s)\n", __LINE__, #cond, fz_last_error()); fflush(stdout); _exit(1); } } while (0)
#include <unistd.h>

// ---- the model scheme ------------------------------------------------------------------------------------------------
static const int64_t MQ = 2147465729ll;
static const int D = 64, RANK = 3;
static const int64_t BETA_SK = 52, OMEGA_SK = 64, BETA_VF = 1000, OMEGA_VF = 64;
static std::vector<int32_t> g_A;                         // [RANK][D], no entry 0 mod q
static inline int32_t md(int64_t x) { x %= MQ; return (int32_t)(x < 0 ? x + MQ : x); }
static inline uint64_t mix(uint64_t x) {
    x += 0x9e3779b97f4a7c15ull; x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull; x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}
// secret polynomials [N][2][D] from the seed alone
static void m_sample(const uint64_t *seeds, size_t N, int32_t *coef) {
    for (size_t i = 0; i < N; ++i)
        for (int h = 0; h < 2; ++h)
            for (int j = 0; j < D; ++j) coef[(i * 2 + h) * D + j] = md((int64_t)(mix(mix(seeds[i]) + (uint64_t)(h * 1000 + j)) >> 2));
}
// sk [N][2][l][D]: row k of half h = coef_h * (k + 2) + h;  vk [N][2][D] = A . sk_h
static void m_keygen(const int32_t *A, const int32_t *coef, int32_t *sk, int32_t *vk, size_t N, int l) {
    for (size_t i = 0; i < N; ++i)
        for (int h = 0; h < 2; ++h)
            for (int j = 0; j < D; ++j) {
                int64_t acc = 0;
                for (int k = 0; k < l; ++k) {
                    const int32_t s = md((int64_t)coef[(i * 2 + h) * D + j] * (k + 2) + h);
                    sk[((i * 2 + h) * l + k) * D + j] = s;
                    acc = md(acc + md((int64_t)A[k * D + j] * s));
                }
                vk[(i * 2 + h) * D + j] = (int32_t)acc;
            }
}
// c [N][D], prehash [N][32]: a hash over EVERY byte of the signer's message (and its length), mixed with the signer's key
static void m_challenge(const int32_t *vk, const char *msgs, const size_t *off, size_t N, int32_t *c, uint8_t *pre) {
    for (size_t i = 0; i < N; ++i) {
        uint64_t h = 0xcbf29ce484222325ull ^ (uint64_t)(off[i + 1] - off[i]);
        for (size_t b = off[i]; b < off[i + 1]; ++b) h = mix(h ^ (uint8_t)msgs[b]);
        uint64_t k = h;
        for (int j = 0; j < 2 * D; ++j) k = mix(k ^ (uint32_t)vk[i * 2 * D + j]);
        for (int j = 0; j < D; ++j) c[i * D + j] = md((int64_t)(mix(k + (uint64_t)j) >> 2));
        if (pre) for (int b = 0; b < 32; ++b) pre[i * 32 + b] = (uint8_t)(mix(h + 7777u + (uint64_t)(b / 8)) >> (8 * (b % 8)));
    }
}
// sig [N][l][D] = skL (.) c + skR
static void m_sign(const int32_t *sk, const int32_t *c, int32_t *sig, size_t N, int l) {
    for (size_t i = 0; i < N; ++i)
        for (int k = 0; k < l; ++k)
            for (int j = 0; j < D; ++j)
                sig[(i * l + k) * D + j] = md((int64_t)sk[((i * 2) * l + k) * D + j] * c[i * D + j] + sk[((i * 2 + 1) * l + k) * D + j]);
}
// the "transform": any fixed map per coefficient will do (in place is allowed)
static void m_ntt(const int32_t *in, int32_t *out, size_t N) {
    for (size_t i = 0; i < N; ++i)
        for (int j = 0; j < D; ++j) out[i * D + j] = md((int64_t)md(in[i * D + j]) * 5 + 7 + j);
}
static void m_ragged(const int32_t *sig, const int32_t *al, const int32_t *vL, const int32_t *vR, const int32_t *c, const size_t *offs, size_t G,
                     int l, int64_t *psum, size_t pstride, int64_t *tsum, size_t tstride) {
    for (size_t g = 0; g < G; ++g) {
        for (int j = 0; j < D; ++j) {
            int64_t t = 0;
            for (size_t i = offs[g]; i < offs[g + 1]; ++i)
                t += md((int64_t)md((int64_t)md((int64_t)vL[i * D + j] * c[i * D + j]) + vR[i * D + j]) * al[i * D + j]);
            tsum[g * tstride + j] = t;
        }
        if (sig)
            for (int k = 0; k < l; ++k)
                for (int j = 0; j < D; ++j) {
                    int64_t s = 0;
                    for (size_t i = offs[g]; i < offs[g + 1]; ++i) s += md((int64_t)sig[(i * l + k) * D + j] * al[i * D + j]);
                    psum[g * pstride + k * D + j] = s;
                }
    }
}
template <class T, class U>
static int m_verdict(const int32_t *A, const T *agg, const U *tgt, int l) {        // A . agg == target (mod q) in every coefficient
    for (int j = 0; j < D; ++j) {
        int64_t acc = 0;
        for (int k = 0; k < l; ++k) acc = md(acc + md((int64_t)A[k * D + j] * md((int64_t)agg[k * D + j])));
        if (acc != md((int64_t)tgt[j])) return FZ_VERDICT_TARGET_MISMATCH;
    }
    return FZ_VERDICT_OK;
}

// ---- the controls of the nine entries --------------------------------------------------------------------------------
enum { E_SAMPLE, E_KEYGEN, E_CHAL, E_SIGN, E_NTT, E_RAGGED, E_VPART, E_VTGT, E_REDUCE, E_COUNT };
struct MRec { int entry; size_t N, G; std::vector<size_t> offs; bool sig_null; int tid; unsigned long seq; };
static std::mutex m_mu;
static std::condition_variable m_cv;
static std::vector<MRec> m_log;
static long m_calls[E_COUNT], m_fail_at[E_COUNT] = {-1, -1, -1, -1, -1, -1, -1, -1, -1};
static int m_fail_code = FZ_E_HIP, m_gate = -1;          // m_gate: the entry whose calls block (-1: none)
static std::string m_fail_msg;
static long m_blocked = 0;
static int enter(int entry, size_t N, size_t G, const size_t *offs, size_t n_offs, bool sig_null) {
    const unsigned long seq = stub_seq();
    const int tid = stub_tid();
    std::unique_lock<std::mutex> lk(m_mu);
    m_log.push_back({entry, N, G, std::vector<size_t>(offs, offs + n_offs), sig_null, tid, seq});
    const long k = m_calls[entry]++;
    if (m_gate == entry) {
        ++m_blocked;
        m_cv.notify_all();
        m_cv.wait(lk, [&] { return m_gate != entry; });
        --m_blocked;
    }
    if (k == m_fail_at[entry]) {
        const int code = m_fail_code;
        const std::string msg = m_fail_msg;
        lk.unlock();
        return fz_set_error(code, "%s", msg.c_str());
    }
    return FZ_OK;
}
static void gate_close(int entry) { std::lock_guard<std::mutex> g(m_mu); m_gate = entry; }
static void gate_open() { std::lock_guard<std::mutex> g(m_mu); m_gate = -1; m_cv.notify_all(); }
static void wait_blocked() { std::unique_lock<std::mutex> lk(m_mu); m_cv.wait(lk, [] { return m_blocked >= 1; }); }
static void arm(int entry, long skip, int code, const std::string &msg) {          // the (skip + 1)-th call of `entry` from now fails
    std::lock_guard<std::mutex> g(m_mu);
    m_fail_at[entry] = m_calls[entry] + skip;
    m_fail_code = code;
    m_fail_msg = msg;
}
static void disarm() { std::lock_guard<std::mutex> g(m_mu); for (long &f : m_fail_at) f = -1; }
static std::vector<MRec> model_log(size_t mark = 0) { std::lock_guard<std::mutex> g(m_mu); return std::vector<MRec>(m_log.begin() + (long)mark, m_log.end()); }
static size_t model_mark() { std::lock_guard<std::mutex> g(m_mu); return m_log.size(); }

// ---- the trace mode ("trace" as the program's argument): what the flows at the end of this file print -------------------
static bool g_trace = false, g_quiet = false;           // g_quiet: this part of a trace run is checked, not printed
static int g_caller_tid = -1;                            // main's; every other thread that logs in a one-worker flow is the worker
static std::set<const void *> g_consumer_streams;
static size_t g_stub_mark = 0, g_model_mark = 0;
static const char *const ENTRY[E_COUNT] = {"sample", "keygen", "challenge", "sign", "ntt", "ragged", "verify_partials", "verify_target", "reduce"};
static int R(int rc) { if (g_trace && !g_quiet && rc != FZ_OK) printf("refusal code=%d text=%s\n", rc, fz_last_error()); return rc; }
static int F(const char *where, int rc) { if (g_trace && !g_quiet && rc != FZ_OK) printf("failure %s code=%d text=%s\n", where, rc, fz_last_error()); return rc; }
// both logs since the last dump, merged by sequence number: no addresses, no tickets
static void tdump(bool print = true) {
    if (!g_trace) return;
    print = print && !g_quiet;
    const std::vector<Call> s = stub_log(g_stub_mark);
    const std::vector<MRec> m = model_log(g_model_mark);
    g_stub_mark += s.size();
    g_model_mark += m.size();
    static std::map<const void *, size_t> bytes;         // a free prints the size of its block: which block went, without its address
    static const char *const KIND[5] = {"h2h", "h2d", "d2h", "d2d", "default"};
    for (size_t i = 0, j = 0; i < s.size() || j < m.size();) {
        if (j == m.size() || (i < s.size() && s[i].seq < m[j].seq)) {
            const Call &r = s[i++];
            if (r.fn == "hipMalloc" || r.fn == "hipHostMalloc") bytes[r.p] = r.n;
            const size_t n = r.fn == "hipFree" || r.fn == "hipHostFree" ? bytes[r.p] : r.n;
            if (!print) continue;
            printf("hip %s n=%zu kind=%s thread=%s stream=%s\n", r.fn.c_str(), n, r.kind < 0 || r.kind > 4 ? "-" : KIND[r.kind],
                   r.tid == g_caller_tid ? "caller" : "worker", !r.stream ? "none" : g_consumer_streams.count(r.stream) ? "consumer" : "worker");
        } else {
            const MRec &r = m[j++];
            if (!print) continue;
            printf("model %s N=%zu G=%zu offs=[", ENTRY[r.entry], r.N, r.G);
            for (size_t k = 0; k < r.offs.size(); ++k) printf(k ? ",%zu" : "%zu", r.offs[k]);
            printf("] sig_null=%d thread=%s\n", (int)r.sig_null, r.tid == g_caller_tid ? "caller" : "worker");
        }
    }
    fflush(stdout);
}

extern "C" {
int fz_sample_secret_polys_dev(fz_ctx *, const uint64_t *h_seeds, size_t N, int64_t modulus, int degree, int64_t norm_bound, int64_t weight_bound, int32_t *d_out) {
    CHECK(modulus == MQ && degree == D && norm_bound == BETA_SK && weight_bound == OMEGA_SK);
    const int rc = enter(E_SAMPLE, N, 0, nullptr, 0, false);
    if (rc == FZ_OK) m_sample(h_seeds, N, d_out);
    return rc;
}
int fz_keygen_core_bcast(fz_ctx *, const int32_t *d_A, const int32_t *d_coef, int32_t *d_sk_hat, int32_t *d_vk, size_t batch, int l) {
    const int rc = enter(E_KEYGEN, batch, 0, nullptr, 0, false);
    if (rc == FZ_OK) m_keygen(d_A, d_coef, d_sk_hat, d_vk, batch, l);
    return rc;
}
int fz_challenge_hat_msgs_dev(fz_ctx *, const fz_scheme_params *, const int32_t *d_vk, const char *h_msgs, const size_t *h_msg_off, size_t N, int32_t *d_c_hat, uint8_t *h_prehash_out) {
    const int rc = enter(E_CHAL, N, 0, h_msg_off, N + 1, false);
    if (rc == FZ_OK) m_challenge(d_vk, h_msgs, h_msg_off, N, d_c_hat, h_prehash_out);
    return rc;
}
int fz_sign_core(fz_ctx *, const int32_t *d_sk_hat, const int32_t *d_c_hat, int32_t *d_sig, size_t batch, int l) {
    const int rc = enter(E_SIGN, batch, 0, nullptr, 0, false);
    if (rc == FZ_OK) m_sign(d_sk_hat, d_c_hat, d_sig, batch, l);
    return rc;
}
int fz_ntt_forward(fz_ctx *, const int32_t *d_in, int32_t *d_out, size_t batch) {
    const int rc = enter(E_NTT, batch, 0, nullptr, 0, false);
    if (rc == FZ_OK) m_ntt(d_in, d_out, batch);
    return rc;
}
int fz_aggregate_target_partial_ragged(fz_ctx *, const int32_t *d_sig, const int32_t *d_alpha_hat, const int32_t *d_vkL, const int32_t *d_vkR, const int32_t *d_c_hat,
                                       const size_t *h_offsets, size_t groups, int l, int64_t *d_partial, size_t partial_stride, int64_t *d_target_partial, size_t target_stride) {
    const int rc = enter(E_RAGGED, h_offsets[groups], groups, h_offsets, groups + 1, d_sig == nullptr);
    if (rc == FZ_OK) m_ragged(d_sig, d_alpha_hat, d_vkL, d_vkR, d_c_hat, h_offsets, groups, l, d_partial, partial_stride, d_target_partial, target_stride);
    return rc;
}
int fz_verify_partials_batch_async(fz_ctx *, const int32_t *d_A, const int64_t *d_partial, size_t partial_stride, const int64_t *d_target_partial, size_t target_stride,
                                   size_t groups, int l, int64_t beta_vf, int64_t omega_vf, int *d_verdicts) {
    CHECK(beta_vf == BETA_VF && omega_vf == OMEGA_VF);
    const int rc = enter(E_VPART, 0, groups, nullptr, 0, false);
    if (rc == FZ_OK) for (size_t g = 0; g < groups; ++g) d_verdicts[g] = m_verdict(d_A, d_partial + g * partial_stride, d_target_partial + g * target_stride, l);
    return rc;
}
int fz_verify_with_target_batch_async(fz_ctx *, const int32_t *d_A, const int32_t *d_sig, const int32_t *d_target, size_t groups, int l, int64_t beta_vf, int64_t omega_vf, int *d_verdicts) {
    CHECK(beta_vf == BETA_VF && omega_vf == OMEGA_VF);
    const int rc = enter(E_VTGT, 0, groups, nullptr, 0, false);
    if (rc == FZ_OK) for (size_t g = 0; g < groups; ++g) d_verdicts[g] = m_verdict(d_A, d_sig + g * (size_t)l * D, d_target + g * D, l);
    return rc;
}
int fz_reduce_i64(fz_ctx *, const int64_t *d_in, int32_t *d_out, size_t count) {
    const int rc = enter(E_REDUCE, count, 0, nullptr, 0, false);
    if (rc == FZ_OK) for (size_t i = 0; i < count; ++i) d_out[i] = md(d_in[i]);
    return rc;
}
}

// ---- calls and what the model expects of each, from that call's inputs alone -----------------------------------------
static fz_scheme_params params() {
    fz_scheme_params P;
    memset(&P, 0, sizeof(P));
    P.modulus = MQ; P.secpar = 128; P.degree = D; P.root = 23584283; P.inv_root = 540632852; P.root_order = 128; P.omega_ch = 31; P.omega_ag = 31;
    P.beta_ch = 1; P.beta_ag = 1; P.bytes_for_one_coef_bdd_by_beta_ch = 17; P.bytes_for_poly_shuffle = 1088;
    P.sign_pre_hash_dst[0] = 0; P.sign_pre_hash_dst[1] = 0; P.sign_hash_dst[0] = 1; P.sign_hash_dst[1] = 1; P.agg_xof_dst[0] = 2; P.agg_xof_dst[1] = 1;
    return P;
}
static const fz_scheme_params g_P = params();
static std::atomic<uint64_t> g_tag(1);
static const int32_t VK_SENTINEL = 0x7b7b7b7b;

struct KS {                                                // a keygen-sign call
    std::vector<uint64_t> seeds;
    std::string msgs;
    std::vector<size_t> off;
    std::vector<int32_t> vk_out, e_sk, e_vk, e_sig;
    bool want_vk = true;
    int flags = 0;
    uint64_t ticket = 0;
    fz_queue_result res;
    size_t n() const { return seeds.size(); }
};
static void fill_msgs(size_t n, uint64_t tag, std::string &msgs, std::vector<size_t> &off) {       // lengths 0 .. 39, an empty one among them
    off.assign(1, 0);
    for (size_t i = 0; i < n; ++i) {
        const size_t len = (size_t)((tag * 7 + i * 13) % 40);
        for (size_t k = 0; k < len; ++k) msgs += (char)('a' + mix(tag * 131 + i * 17 + k) % 26);
        off.push_back(msgs.size());
    }
}
static std::unique_ptr<KS> make_ks(size_t n, int flags, bool want_vk = true) {
    std::unique_ptr<KS> c(new KS());
    const uint64_t tag = g_tag++;
    for (size_t i = 0; i < n; ++i) c->seeds.push_back(mix(tag * 100003 + i) >> 1);
    fill_msgs(n, tag, c->msgs, c->off);
    c->flags = flags;
    c->want_vk = want_vk;
    c->vk_out.assign(n * 2 * D, VK_SENTINEL);
    std::vector<int32_t> coef(n * 2 * D), ch(n * D);
    c->e_sk.resize(n * 2 * RANK * D); c->e_vk.resize(n * 2 * D); c->e_sig.resize(n * RANK * D);
    m_sample(c->seeds.data(), n, coef.data());
    m_keygen(g_A.data(), coef.data(), c->e_sk.data(), c->e_vk.data(), n, RANK);
    m_challenge(c->e_vk.data(), c->msgs.data(), c->off.data(), n, ch.data(), nullptr);
    m_sign(c->e_sk.data(), ch.data(), c->e_sig.data(), n, RANK);
    return c;
}
static void submit(fz_queue *Q, KS &c) {
    CHECK(fz_queue_submit_keygen_sign(Q, c.seeds.data(), c.n(), c.msgs.data(), c.off.data(), c.want_vk ? c.vk_out.data() : nullptr, c.flags, &c.ticket) == FZ_OK);
}
static void check_ks(fz_queue *Q, KS &c, bool release = true) {
    fz_queue_result r;
    memset(&r, 0xff, sizeof(r));
    CHECK(fz_queue_wait(Q, c.ticket, &r) == FZ_OK);
    const size_t n = c.n();
    if (c.want_vk) CHECK(c.vk_out == c.e_vk); else CHECK(c.vk_out == std::vector<int32_t>(n * 2 * D, VK_SENTINEL));
    c.res = r;
    if (c.flags & FZ_QUEUE_DISCARD) { CHECK(r.status == 0 && r.n == 0 && !r.d_vk && !r.d_sig && !r.d_sk_hat); return; }
    CHECK(r.status == FZ_OK && r.n == n && r.d_vk && r.d_sig);
    CHECK(!memcmp(r.d_vk, c.e_vk.data(), n * 2 * D * 4) && !memcmp(r.d_sig, c.e_sig.data(), n * RANK * D * 4));
    if (c.flags & FZ_QUEUE_KEEP_SK) CHECK(r.d_sk_hat && !memcmp(r.d_sk_hat, c.e_sk.data(), n * 2 * RANK * D * 4)); else CHECK(!r.d_sk_hat);
    if (release) CHECK(fz_queue_release(Q, c.ticket) == FZ_OK);
}

static const int32_t AGG_SENTINEL = 0x5a5a5a5a;
static const int VERDICT_SENTINEL = -77;
struct AG {                                                // an aggregate-verify call, or (verify_only) a verify call of `rows`
    size_t n = 0;
    std::vector<int32_t> vk, sig, agg_out, e_agg, rows;
    std::string msgs;
    std::vector<size_t> off;
    bool verify_only = false, want_agg = true, want_verdict = true, identity_order = true;
    int flags = 0, verdict = VERDICT_SENTINEL, e_verdict = 0;
    void *d_rows = nullptr;                                // FZ_QUEUE_ROWS_ON_DEVICE: a "device" copy of the rows
    uint64_t ticket = 0;
    const int32_t *src() const { return d_rows ? (const int32_t *)d_rows : verify_only ? rows.data() : sig.data(); }
};
// n honest signers; the expected aggregate and verdict with alpha from the product's own sort + coefficients on this call alone
static std::unique_ptr<AG> make_ag(size_t n, size_t capacity, int flags = 0) {
    std::unique_ptr<AG> a(new AG());
    std::unique_ptr<KS> k = make_ks(n, 0);
    a->n = n; a->vk = k->e_vk; a->sig = k->e_sig; a->msgs = k->msgs; a->off = k->off; a->flags = flags;
    a->agg_out.assign(RANK * D, AGG_SENTINEL);
    std::vector<int32_t> L(n * D), R(n * D), c(n * D), alpha(n * D), al(n * D);
    std::vector<uint8_t> pre(n * 32);
    for (size_t i = 0; i < n; ++i) { memcpy(&L[i * D], &a->vk[2 * i * D], D * 4); memcpy(&R[i * D], &a->vk[(2 * i + 1) * D], D * 4); }
    m_challenge(a->vk.data(), a->msgs.data(), a->off.data(), n, c.data(), pre.data());
    std::vector<size_t> order(n);
    CHECK(fz_sort_by_vk_string(&g_P, L.data(), R.data(), n, order.data(), 1) == FZ_OK);
    std::vector<int32_t> sL(n * D), sR(n * D), sC(n * D), sA(n * D);
    std::vector<uint8_t> sP(n * 32);
    for (size_t i = 0; i < n; ++i) {
        if (order[i] != i) a->identity_order = false;
        memcpy(&sL[i * D], &L[order[i] * D], D * 4); memcpy(&sR[i * D], &R[order[i] * D], D * 4);
        memcpy(&sC[i * D], &c[order[i] * D], D * 4); memcpy(&sP[i * 32], &pre[order[i] * 32], 32);
    }
    CHECK(fz_aggregation_coefficients(&g_P, sL.data(), sR.data(), sP.data(), sC.data(), n, sA.data(), 1) == FZ_OK);
    for (size_t i = 0; i < n; ++i) memcpy(&alpha[order[i] * D], &sA[i * D], D * 4);
    m_ntt(alpha.data(), al.data(), n);
    std::vector<int64_t> ps(RANK * D), ts(D);
    const size_t offs[2] = {0, n};
    m_ragged(a->sig.data(), al.data(), L.data(), R.data(), c.data(), offs, 1, RANK, ps.data(), RANK * D, ts.data(), D);
    a->e_agg.resize(RANK * D);
    for (int i = 0; i < RANK * D; ++i) a->e_agg[i] = md(ps[i]);
    a->e_verdict = n > capacity ? FZ_VERDICT_TOO_MANY_KEYS : m_verdict(g_A.data(), ps.data(), ts.data(), RANK);
    CHECK(m_verdict(g_A.data(), ps.data(), ts.data(), RANK) == FZ_VERDICT_OK);                    // the model verifies an honest aggregate
    if (flags & FZ_QUEUE_ROWS_ON_DEVICE) { CHECK(hipMalloc(&a->d_rows, a->sig.size() * 4) == hipSuccess); memcpy(a->d_rows, a->sig.data(), a->sig.size() * 4); }
    return a;
}
// verify() of a's aggregate (tamper: one coefficient + 1)
static std::unique_ptr<AG> make_vf(size_t n, size_t capacity, bool tamper, int flags = 0) {
    std::unique_ptr<AG> a = make_ag(n, capacity, 0);
    a->verify_only = true; a->want_agg = false; a->flags = flags;
    a->rows = a->e_agg;
    if (tamper) { a->rows[(size_t)(RANK - 1) * D + 5] += 1; if (a->e_verdict == FZ_VERDICT_OK) a->e_verdict = FZ_VERDICT_TARGET_MISMATCH; }
    if (flags & FZ_QUEUE_ROWS_ON_DEVICE) { CHECK(hipMalloc(&a->d_rows, a->rows.size() * 4) == hipSuccess); memcpy(a->d_rows, a->rows.data(), a->rows.size() * 4); }
    return a;
}
static int submit_rc(fz_queue *Q, AG &a) {
    return a.verify_only ? fz_queue_submit_verify(Q, a.vk.data(), a.msgs.data(), a.off.data(), a.n, a.src(), a.want_verdict ? &a.verdict : nullptr, a.flags, &a.ticket)
                         : fz_queue_submit_aggregate_verify(Q, a.vk.data(), a.msgs.data(), a.off.data(), a.n, a.src(), a.want_agg ? a.agg_out.data() : nullptr,
                                                            a.want_verdict ? &a.verdict : nullptr, a.flags, &a.ticket);
}
static void submit(fz_queue *Q, AG &a) { CHECK(submit_rc(Q, a) == FZ_OK); }
static void check_ag(fz_queue *Q, AG &a) {
    fz_queue_result r;
    memset(&r, 0xff, sizeof(r));
    CHECK(fz_queue_wait(Q, a.ticket, &r) == FZ_OK);
    CHECK(r.status == FZ_OK && r.n == a.n && !r.d_vk && !r.d_sig && !r.d_sk_hat);
    if (a.want_verdict) CHECK(a.verdict == a.e_verdict);
    if (!a.verify_only && a.want_agg) CHECK(a.agg_out == a.e_agg); else CHECK(a.agg_out == std::vector<int32_t>(RANK * D, AGG_SENTINEL));
    CHECK(fz_queue_release(Q, a.ticket) == FZ_OK);
    if (a.d_rows) { CHECK(hipFree(a.d_rows) == hipSuccess); a.d_rows = nullptr; }
}

static fz_queue *mkq(int workers, size_t max_rows, size_t capacity = 64, int host_threads = 1) {
    fz_queue *Q = nullptr;
    CHECK(fz_queue_create(0, &g_P, RANK, BETA_SK, OMEGA_SK, g_A.data(), workers, max_rows, &Q) == FZ_OK && Q);
    if (capacity) CHECK(fz_queue_enable_aggregate(Q, BETA_VF, OMEGA_VF, capacity, host_threads) == FZ_OK);
    return Q;
}
struct Stats { uint64_t calls, batches, rows; };
static Stats stats(fz_queue *Q) { Stats s; CHECK(fz_queue_stats(Q, &s.calls, &s.batches, &s.rows) == FZ_OK); return s; }
// A one-worker queue is held by a discarded call of one row that blocks in the sampler: what is submitted until open() is pending
// together, so how the worker cuts it into batches does not depend on timing.
struct Hold {
    std::unique_ptr<KS> b;
    explicit Hold(fz_queue *Q) { gate_close(E_SAMPLE); b = make_ks(1, FZ_QUEUE_DISCARD, false); submit(Q, *b); wait_blocked(); }
    void open() { gate_open(); }
};
// one more call through a one-worker queue: the worker frees what was released before it takes the call
static void flush(fz_queue *Q) {
    std::unique_ptr<KS> f = make_ks(1, FZ_QUEUE_DISCARD, false);
    submit(Q, *f);
    CHECK(fz_queue_wait(Q, f->ticket, nullptr) == FZ_OK);
}
static long live_allocs() { long a, e, s; stub_live(&a, &e, &s); return a; }
static size_t count(const std::vector<Call> &log, const char *fn, const void *p) {
    size_t c = 0;
    for (const Call &r : log) c += r.fn == fn && r.p == p;
    return c;
}
static const Call *find(const std::vector<Call> &log, const char *fn, const void *p) {
    for (const Call &r : log) if (r.fn == fn && r.p == p) return &r;
    return nullptr;
}
static std::vector<MRec> only(const std::vector<MRec> &log, int entry) {
    std::vector<MRec> out;
    for (const MRec &r : log) if (r.entry == entry) out.push_back(r);
    return out;
}
static fz_ctx *consumer(hipStream_t *st) {
    fz_ctx *c = nullptr;
    CHECK(fz_ctx_create(0, (uint32_t)MQ, D, 23584283u, 540632852u, &c) == FZ_OK);
    CHECK(fz_stream_create(c, (void **)st) == FZ_OK && fz_ctx_set_stream(c, *st) == FZ_OK);
    return c;
}
static void consumer_destroy(fz_ctx *c, hipStream_t st) {
    CHECK(fz_ctx_set_stream(c, nullptr) == FZ_OK && fz_stream_destroy(c, st) == FZ_OK && fz_ctx_destroy(c) == FZ_OK);
}

// ---- S1: the cut at max_rows ------------------------------------------------------------------------------------------
static void s1_cut() {
    fz_queue *Q = mkq(1, 10);
    const size_t m0 = model_mark();
    const size_t sizes[6] = {2, 4, 6, 1, 10, 3};
    std::vector<std::unique_ptr<KS>> calls;
    gate_close(E_SAMPLE);
    for (int k = 0; k < 6; ++k) {
        calls.push_back(make_ks(sizes[k], k == 2 ? FZ_QUEUE_KEEP_SK : 0));
        submit(Q, *calls.back());
        if (k == 0) wait_blocked();                      // the worker took the first call alone and sits in the sampler
    }
    gate_open();
    for (auto &c : calls) check_ks(Q, *c, false);
    const std::vector<MRec> log = model_log(m0), smp = only(log, E_SAMPLE), chal = only(log, E_CHAL);
    const size_t want[5] = {2, 10, 1, 10, 3};
    CHECK(smp.size() == 5 && chal.size() == 5);
    for (int k = 0; k < 5; ++k) CHECK(smp[k].N == want[k] && chal[k].N == want[k]);
    // the shared batch: the second call's message offsets rebased behind the first call's bytes
    CHECK(chal[1].offs.size() == 11);
    for (size_t i = 0; i <= 4; ++i) CHECK(chal[1].offs[i] == calls[1]->off[i]);
    for (size_t i = 1; i <= 6; ++i) CHECK(chal[1].offs[4 + i] == calls[1]->msgs.size() + calls[2]->off[i]);
    CHECK(calls[2]->res.d_vk - calls[1]->res.d_vk == 4 * 2 * D && calls[2]->res.d_sig - calls[1]->res.d_sig == 4 * RANK * D);
    const Stats s = stats(Q);
    CHECK(s.calls == 6 && s.batches == 5 && s.rows == 26);
    for (auto &c : calls) CHECK(fz_queue_release(Q, c->ticket) == FZ_OK);
    CHECK(fz_queue_destroy(Q) == FZ_OK);
}

// ---- S2: a batch is a run of calls of ONE kind, taken in order --------------------------------------------------------
static void s2_kinds() {
    fz_queue *Q = mkq(1, 64);
    Hold h(Q);
    const size_t m0 = model_mark();
    std::vector<std::unique_ptr<KS>> ks;
    std::vector<std::unique_ptr<AG>> ag;
    ks.push_back(make_ks(3, 0)); ks.push_back(make_ks(5, 0));
    ag.push_back(make_ag(4, 64)); ag.push_back(make_ag(2, 64));
    ag.push_back(make_vf(3, 64, false)); ag.push_back(make_vf(5, 64, true));
    ks.push_back(make_ks(2, 0));
    submit(Q, *ks[0]); submit(Q, *ks[1]);
    for (auto &a : ag) submit(Q, *a);
    submit(Q, *ks[2]);
    h.open();
    for (auto &c : ks) check_ks(Q, *c);
    for (auto &a : ag) check_ag(Q, *a);
    std::vector<MRec> seq;
    for (const MRec &r : model_log(m0)) if (r.entry == E_SAMPLE || r.entry == E_RAGGED) seq.push_back(r);
    CHECK(seq.size() == 4);
    CHECK(seq[0].entry == E_SAMPLE && seq[0].N == 8);
    CHECK(seq[1].entry == E_RAGGED && !seq[1].sig_null && seq[1].G == 2 && seq[1].offs == (std::vector<size_t>{0, 4, 6}));
    CHECK(seq[2].entry == E_RAGGED && seq[2].sig_null && seq[2].G == 2 && seq[2].offs == (std::vector<size_t>{0, 3, 8}));
    CHECK(seq[3].entry == E_SAMPLE && seq[3].N == 2);
    const Stats s = stats(Q);
    CHECK(s.calls == 8 && s.batches == 5 && s.rows == 1 + 8 + 6 + 8 + 2);
    CHECK(fz_queue_destroy(Q) == FZ_OK);
}

// ---- S3: flags within one batch; a batch nobody keeps owns no blocks --------------------------------------------------
static void s3_flags() {
    fz_queue *Q = mkq(1, 64);
    {
        Hold h(Q);
        const size_t m0 = model_mark();
        std::vector<std::unique_ptr<KS>> c;
        for (int flags : {0, FZ_QUEUE_KEEP_SK, FZ_QUEUE_DISCARD, FZ_QUEUE_DISCARD | FZ_QUEUE_KEEP_SK}) { c.push_back(make_ks(3 + c.size(), flags)); submit(Q, *c.back()); }
        h.open();
        for (auto &k : c) check_ks(Q, *k);               // (d_sk_hat only for the kept KEEP_SK call; all four h_vk_out filled)
        CHECK(only(model_log(m0), E_SAMPLE).size() == 1 && only(model_log(m0), E_SAMPLE)[0].N == 3 + 4 + 5 + 6);
        CHECK(fz_queue_drain(Q) == FZ_OK);
    }
    long before = 0;
    for (int round = 0; round < 2; ++round) {            // the first round warms the worker's scratch
        flush(Q);
        before = live_allocs();
        const size_t mark = stub_mark();
        Hold h(Q);
        std::vector<std::unique_ptr<KS>> c;
        for (int flags : {FZ_QUEUE_DISCARD, FZ_QUEUE_DISCARD | FZ_QUEUE_KEEP_SK, FZ_QUEUE_DISCARD}) { c.push_back(make_ks(20 + c.size(), flags)); submit(Q, *c.back()); }
        h.open();
        for (auto &k : c) check_ks(Q, *k);
        CHECK(fz_queue_drain(Q) == FZ_OK);
        if (round == 1) {
            CHECK(live_allocs() == before);
            for (const Call &r : stub_log(mark)) CHECK(r.fn != "hipMalloc" && r.fn != "hipFree");
        }
    }
    CHECK(fz_queue_destroy(Q) == FZ_OK);
}

// ---- S4: the batch blocks live until the LAST release, and go back once, on the owning worker's thread ----------------
static void s4_release_counts() {
    fz_queue *Q = mkq(1, 64);
    Hold h(Q);
    const size_t m0 = model_mark();
    std::vector<std::unique_ptr<KS>> c;
    c.push_back(make_ks(2, FZ_QUEUE_KEEP_SK)); c.push_back(make_ks(3, 0)); c.push_back(make_ks(4, FZ_QUEUE_KEEP_SK));
    for (auto &k : c) submit(Q, *k);
    h.open();
    for (auto &k : c) check_ks(Q, *k, false);
    const std::vector<MRec> smp = only(model_log(m0), E_SAMPLE);
    CHECK(smp.size() == 1 && smp[0].N == 9);
    const void *blocks[3] = {c[0]->res.d_vk, c[0]->res.d_sig, c[0]->res.d_sk_hat};      // row0 == 0: the blocks themselves
    const size_t mark = stub_mark();
    CHECK(fz_queue_release(Q, c[0]->ticket) == FZ_OK && fz_queue_release(Q, c[1]->ticket) == FZ_OK);
    flush(Q);
    for (const void *p : blocks) CHECK(count(stub_log(mark), "hipFree", p) == 0);
    check_ks(Q, *c[2], false);                           // still readable and right
    CHECK(fz_queue_release(Q, c[2]->ticket) == FZ_OK);
    flush(Q);
    std::vector<Call> log = stub_log(mark);
    for (const void *p : blocks) { CHECK(count(log, "hipFree", p) == 1 && find(log, "hipFree", p)->tid == smp[0].tid); }
    const size_t mark2 = stub_mark();
    for (auto &k : c) CHECK(fz_queue_release(Q, k->ticket) == FZ_OK);                   // released before: a no-op
    flush(Q);
    for (const Call &r : stub_log(mark2)) CHECK(r.fn != "hipFree" || (r.p != blocks[0] && r.p != blocks[1] && r.p != blocks[2]));
    fz_queue_result r;
    memset(&r, 0xff, sizeof(r));
    CHECK(fz_queue_wait(Q, c[1]->ticket, &r) == FZ_OK && r.status == 0 && r.n == 0 && !r.d_vk && !r.d_sig && !r.d_sk_hat);
    std::unique_ptr<KS> last = make_ks(1, 0);
    submit(Q, *last);
    check_ks(Q, *last);
    for (uint64_t t : {(uint64_t)0, last->ticket + 1}) {
        CHECK(fz_queue_wait(Q, t, &r) == FZ_E_BADARG && fz_queue_release(Q, t) == FZ_E_BADARG);
    }
    CHECK(fz_queue_destroy(Q) == FZ_OK);
}

// ---- S5: release_after -- the worker's stream waits for the consumers' events before the blocks go back ---------------
static void s5_release_after() {
    hipStream_t cs[2];
    fz_ctx *cons[2] = {consumer(&cs[0]), consumer(&cs[1])};
    fz_queue *Q = mkq(1, 64);
    Hold h(Q);
    std::vector<std::unique_ptr<KS>> c;
    c.push_back(make_ks(3, 0)); c.push_back(make_ks(2, FZ_QUEUE_KEEP_SK));
    const size_t mark0 = stub_mark();
    for (auto &k : c) submit(Q, *k);
    h.open();
    for (auto &k : c) check_ks(Q, *k, false);
    const std::vector<Call> log0 = stub_log(mark0);
    const Call *to_host = find(log0, "hipMemcpyAsync", c[0]->vk_out.data());
    CHECK(to_host && to_host->kind == (int)hipMemcpyDeviceToHost && to_host->stream);
    const void *wstream = to_host->stream;
    CHECK(wstream != cs[0] && wstream != cs[1]);
    CHECK(c[1]->res.d_vk - c[0]->res.d_vk == 3 * 2 * D);                                 // one batch
    const void *blocks[2] = {c[0]->res.d_vk, c[0]->res.d_sig};
    const size_t mark = stub_mark();
    CHECK(fz_queue_release_after(Q, c[0]->ticket, cons[0]) == FZ_OK);
    CHECK(fz_queue_release_after(Q, c[1]->ticket, cons[1]) == FZ_OK);
    CHECK(fz_queue_release_after(Q, c[1]->ticket, nullptr) == FZ_E_BADARG);
    flush(Q);
    const std::vector<Call> log = stub_log(mark);
    unsigned long first_free = ~0ul, last_wait = 0;
    for (const void *p : blocks) { CHECK(count(log, "hipFree", p) == 1); first_free = std::min(first_free, find(log, "hipFree", p)->seq); }
    for (int k = 0; k < 2; ++k) {
        const Call *record = nullptr, *wait = nullptr, *destroy = nullptr;
        for (const Call &r : log) if (r.fn == "hipEventRecord" && r.stream == cs[k]) { CHECK(!record); record = &r; }
        CHECK(record);
        const void *ev = record->p;
        for (const Call &r : log) {
            if (r.fn == "hipStreamWaitEvent" && r.p == ev) { CHECK(!wait && r.stream == wstream); wait = &r; }
            if (r.fn == "hipEventDestroy" && r.p == ev) { CHECK(!destroy); destroy = &r; }
        }
        CHECK(wait && destroy && record->seq < wait->seq && wait->seq < destroy->seq && destroy->seq < first_free);
        last_wait = std::max(last_wait, wait->seq);
    }
    CHECK(last_wait < first_free);
    CHECK(fz_queue_destroy(Q) == FZ_OK);
    for (int k = 0; k < 2; ++k) consumer_destroy(cons[k], cs[k]);
}

// ---- S6: a failing step reaches every call of its batch, drains the stream, frees the blocks, writes nothing ----------
static void s6_errors() {
    fz_queue *Q = mkq(1, 64);
    auto ks_batch = [&](std::vector<std::unique_ptr<KS>> &c) {
        c.clear();
        c.push_back(make_ks(3, 0)); c.push_back(make_ks(2, FZ_QUEUE_KEEP_SK)); c.push_back(make_ks(4, FZ_QUEUE_DISCARD));
    };
    std::vector<std::unique_ptr<KS>> c;
    {   // warm the worker's scratch with a batch of the same shape
        Hold h(Q);
        ks_batch(c);
        for (auto &k : c) submit(Q, *k);
        h.open();
        for (auto &k : c) check_ks(Q, *k);
        flush(Q);
    }
    const int codes[3] = {FZ_E_HIP, FZ_E_UNSUPPORTED, FZ_E_BADARG};
    int injected = 0;
    for (int entry : {E_SAMPLE, E_KEYGEN, E_CHAL, E_SIGN}) {
        const int code = codes[injected % 3];
        const std::string text = "injected failure #" + std::to_string(injected++);
        const long before = live_allocs();
        const Stats s0 = stats(Q);
        Hold h(Q);
        arm(entry, entry == E_SAMPLE ? 0 : 1, code, text);          // (the holding call is in the sampler already and runs the other steps once)
        ks_batch(c);
        for (auto &k : c) submit(Q, *k);
        const size_t m0 = model_mark(), mark = stub_mark();
        h.open();
        for (int k = 0; k < 2; ++k) {
            fz_queue_result r;
            memset(&r, 0xff, sizeof(r));
            CHECK(fz_queue_wait(Q, c[k]->ticket, &r) == code && strstr(fz_last_error(), text.c_str()) && strstr(fz_last_error(), "queued batch failed"));
            CHECK(r.status == code && !r.d_vk && !r.d_sig && !r.d_sk_hat);
        }
        // the stream was drained behind the failing step, on the worker's thread
        const std::vector<MRec> mlog = only(model_log(m0), entry);
        CHECK(!mlog.empty());
        const MRec &failed = mlog.back();
        bool drained = false;
        for (const Call &r : stub_log(mark)) drained |= r.fn == "hipStreamSynchronize" && r.seq > failed.seq && r.tid == failed.tid;
        CHECK(drained);
        CHECK(fz_queue_wait(Q, c[2]->ticket, nullptr) == FZ_OK);
        int rc = fz_queue_drain(Q);
        CHECK(rc == code && strstr(fz_last_error(), "a discarded call failed") && strstr(fz_last_error(), text.c_str()));
        CHECK(fz_queue_drain(Q) == FZ_OK);
        for (int k = 0; k < 2; ++k) CHECK(fz_queue_release(Q, c[k]->ticket) == FZ_OK);
        disarm();
        flush(Q);
        CHECK(live_allocs() == before);                  // the batch blocks went back on the way out
        const Stats s1 = stats(Q);
        CHECK(s1.calls == s0.calls + 5 && s1.batches == s0.batches + 3 && s1.rows == s0.rows + 1 + 9 + 1);
        ks_batch(c);                                     // the next batch is right
        for (auto &k : c) { submit(Q, *k); check_ks(Q, *k); }
        CHECK(fz_queue_drain(Q) == FZ_OK);
        flush(Q);
    }
    for (int verify = 0; verify < 2; ++verify) {
        std::vector<std::unique_ptr<AG>> a;
        auto ag_batch = [&]() {
            a.clear();
            for (size_t n : {3, 1, 4}) a.push_back(verify ? make_vf(n, 64, n == 1) : make_ag(n, 64));
        };
        {
            Hold h(Q);
            ag_batch();
            for (auto &x : a) submit(Q, *x);
            h.open();
            for (auto &x : a) check_ag(Q, *x);
            flush(Q);
        }
        const std::vector<int> steps = verify ? std::vector<int>{E_CHAL, E_NTT, E_RAGGED, E_REDUCE, E_VTGT} : std::vector<int>{E_CHAL, E_NTT, E_RAGGED, E_VPART, E_REDUCE};
        for (int entry : steps) {
            const int code = codes[injected % 3];
            const std::string text = "injected failure #" + std::to_string(injected++);
            const long before = live_allocs();
            const Stats s0 = stats(Q);
            Hold h(Q);
            arm(entry, entry == E_CHAL ? 1 : 0, code, text);
            ag_batch();
            for (auto &x : a) submit(Q, *x);
            const size_t m0 = model_mark(), mark = stub_mark();
            h.open();
            for (auto &x : a) {
                fz_queue_result r;
                memset(&r, 0xff, sizeof(r));
                CHECK(fz_queue_wait(Q, x->ticket, &r) == code && strstr(fz_last_error(), text.c_str()));
                CHECK(r.status == code && !r.d_vk && !r.d_sig && !r.d_sk_hat);
                CHECK(x->verdict == VERDICT_SENTINEL && x->agg_out == std::vector<int32_t>(RANK * D, AGG_SENTINEL));
            }
            // every copy that reads a caller's rows is behind a synchronise of its stream that follows the failing step
            const std::vector<MRec> mlog = only(model_log(m0), entry);
            CHECK(!mlog.empty());
            const MRec &failed = mlog.back();
            const std::vector<Call> log = stub_log(mark);
            for (auto &x : a) {
                const Call *copy = nullptr;
                for (const Call &r : log) if (r.fn == "hipMemcpyAsync" && r.src == x->src()) { CHECK(!copy); copy = &r; }
                CHECK(copy && copy->kind == (int)hipMemcpyHostToDevice && copy->seq < failed.seq);
                bool drained = false;
                for (const Call &r : log) drained |= r.fn == "hipStreamSynchronize" && r.stream == copy->stream && r.seq > failed.seq && r.tid == failed.tid;
                CHECK(drained);
            }
            CHECK(fz_queue_drain(Q) == FZ_OK);           // nothing of this batch was a discarded call
            for (auto &x : a) CHECK(fz_queue_release(Q, x->ticket) == FZ_OK);
            disarm();
            flush(Q);
            CHECK(live_allocs() == before);
            const Stats s1 = stats(Q);
            CHECK(s1.calls == s0.calls + 5 && s1.batches == s0.batches + 3 && s1.rows == s0.rows + 1 + 8 + 1);
            ag_batch();
            for (auto &x : a) { submit(Q, *x); check_ag(Q, *x); }
            flush(Q);
        }
    }
    CHECK(fz_queue_destroy(Q) == FZ_OK);
}

// ---- S7: destroy with results nobody released and calls still pending -------------------------------------------------
static void s7_destroy() {
    long a0, e0, st0, a1, e1, st1;
    stub_live(&a0, &e0, &st0);
    fz_queue *Q = mkq(2, 16);
    std::vector<std::unique_ptr<KS>> c;
    for (int flags : {0, FZ_QUEUE_KEEP_SK, 0}) { c.push_back(make_ks(5, flags)); submit(Q, *c.back()); }
    for (auto &k : c) check_ks(Q, *k, false);            // finished, never released
    std::unique_ptr<AG> a = make_ag(3, 64);
    submit(Q, *a);
    CHECK(fz_queue_wait(Q, a->ticket, nullptr) == FZ_OK);
    gate_close(E_SAMPLE);
    for (int flags : {0, FZ_QUEUE_KEEP_SK, FZ_QUEUE_DISCARD, 0, FZ_QUEUE_KEEP_SK}) { c.push_back(make_ks(7, flags)); submit(Q, *c.back()); }
    wait_blocked();                                      // a worker sits in the sampler: destroy starts with work outstanding
    std::thread opener([] { std::this_thread::sleep_for(std::chrono::milliseconds(30)); gate_open(); });
    CHECK(fz_queue_destroy(Q) == FZ_OK);                 // finishes what is pending, frees everything, joins
    opener.join();
    for (size_t k = 3; k < c.size(); ++k) CHECK(c[k]->vk_out == c[k]->e_vk);
    stub_live(&a1, &e1, &st1);
    CHECK(a1 == a0 && e1 == e0 && st1 == st0);
}

// ---- S8: every refusal returns its code, enqueues nothing and consumes no ticket --------------------------------------
static void s8_refusals() {
    fz_queue *Q = nullptr;
    fz_scheme_params bad = g_P;
    CHECK(R(fz_queue_create(0, nullptr, RANK, BETA_SK, OMEGA_SK, g_A.data(), 1, 8, &Q)) == FZ_E_BADARG);
    CHECK(R(fz_queue_create(0, &g_P, RANK, BETA_SK, OMEGA_SK, nullptr, 1, 8, &Q)) == FZ_E_BADARG);
    CHECK(R(fz_queue_create(0, &g_P, RANK, BETA_SK, OMEGA_SK, g_A.data(), 1, 8, nullptr)) == FZ_E_BADARG);
    Q = (fz_queue *)&bad;
    CHECK(R(fz_queue_create(0, &g_P, 0, BETA_SK, OMEGA_SK, g_A.data(), 1, 8, &Q)) == FZ_E_BADARG && !Q);
    for (int w : {0, 17}) CHECK(R(fz_queue_create(0, &g_P, RANK, BETA_SK, OMEGA_SK, g_A.data(), w, 8, &Q)) == FZ_E_BADARG && !Q);
    CHECK(R(fz_queue_create(0, &g_P, RANK, BETA_SK, OMEGA_SK, g_A.data(), 1, 0, &Q)) == FZ_E_BADARG && !Q);
    bad.modulus = 0;
    CHECK(R(fz_queue_create(0, &bad, RANK, BETA_SK, OMEGA_SK, g_A.data(), 1, 8, &Q)) == FZ_E_BADARG && !Q);
    bad.modulus = 1ll << 32;
    CHECK(R(fz_queue_create(0, &bad, RANK, BETA_SK, OMEGA_SK, g_A.data(), 1, 8, &Q)) == FZ_E_BADARG && !Q);
    bad = g_P;
    bad.degree = 0;
    CHECK(R(fz_queue_create(0, &bad, RANK, BETA_SK, OMEGA_SK, g_A.data(), 1, 8, &Q)) == FZ_E_BADARG && !Q);

    Q = mkq(1, (size_t)1 << 22, 0);                      // aggregate calls not enabled yet
    uint64_t last = 0;
    Stats s0 = stats(Q);
    auto accepted = [&]() {                              // the next accepted call gets the consecutive ticket
        std::unique_ptr<KS> k = make_ks(1, 0);
        submit(Q, *k);
        CHECK(k->ticket == ++last);
        check_ks(Q, *k);
        s0 = stats(Q);
    };
    auto refused = [&](int rc, int code, const char *text = "") {        // (text: part of the refusal's own message)
        CHECK(R(rc) == code && fz_last_error()[0] && strstr(fz_last_error(), text));
        const Stats s = stats(Q);
        CHECK(s.calls == s0.calls && s.batches == s0.batches && s.rows == s0.rows);
        accepted();
    };
    accepted();
    std::unique_ptr<KS> k = make_ks(3, 0);
    std::vector<size_t> off = k->off;
    std::vector<uint64_t> seeds = k->seeds;
    uint64_t t = 999;
    auto ks = [&](const uint64_t *sd, size_t n, const char *m, const size_t *o, uint64_t *out) { return fz_queue_submit_keygen_sign(Q, sd, n, m, o, nullptr, 0, out); };
    refused(ks(seeds.data(), 3, k->msgs.data(), off.data(), nullptr), FZ_E_BADARG);
    refused(fz_queue_submit_keygen_sign(nullptr, seeds.data(), 3, k->msgs.data(), off.data(), nullptr, 0, &t), FZ_E_BADARG);
    refused(ks(nullptr, 3, k->msgs.data(), off.data(), &t), FZ_E_BADARG);
    refused(ks(seeds.data(), 3, k->msgs.data(), nullptr, &t), FZ_E_BADARG);
    refused(ks(seeds.data(), 0, k->msgs.data(), off.data(), &t), FZ_E_BADARG);
    refused(ks(seeds.data(), ((size_t)1 << 22) + 1, k->msgs.data(), off.data(), &t), FZ_E_BADARG);
    off[0] = 1;
    refused(ks(seeds.data(), 3, k->msgs.data(), off.data(), &t), FZ_E_BADARG);
    off = k->off;
    CHECK(off[2] > 0);
    off[3] = off[2] - 1;
    refused(ks(seeds.data(), 3, k->msgs.data(), off.data(), &t), FZ_E_BADARG);
    off = k->off;
    seeds[2] = ~0ull;
    refused(ks(seeds.data(), 3, k->msgs.data(), off.data(), &t), FZ_E_UNSUPPORTED);
    seeds = k->seeds;
    CHECK(off[3] > 0);
    refused(ks(seeds.data(), 3, nullptr, off.data(), &t), FZ_E_BADARG);
    // two faults in one call: the rules are tested row by row, so the fault in the earlier row names the refusal (S11 pins these)
    const std::string text30(30, 'x');
    seeds = k->seeds;
    seeds[0] = ~0ull;
    off = {0, 10, 20, 19};
    refused(ks(seeds.data(), 3, text30.data(), off.data(), &t), FZ_E_UNSUPPORTED, "seed 2^64 - 1");
    seeds = k->seeds;
    seeds[2] = ~0ull;
    off = {0, 10, 9, 30};
    refused(ks(seeds.data(), 3, text30.data(), off.data(), &t), FZ_E_BADARG, "message offsets must not decrease");
    seeds = k->seeds;
    off = {1, 10, 20, 30};
    refused(ks(seeds.data(), 0, text30.data(), off.data(), &t), FZ_E_BADARG, "between 1 and max_rows");
    CHECK(t == 999);

    std::unique_ptr<AG> a = make_ag(3, 64), v = make_vf(3, 64, false);
    refused(submit_rc(Q, *a), FZ_E_BADARG);              // before fz_queue_enable_aggregate
    refused(submit_rc(Q, *v), FZ_E_BADARG);
    CHECK(R(fz_queue_enable_aggregate(nullptr, BETA_VF, OMEGA_VF, 64, 1)) == FZ_E_BADARG);
    CHECK(R(fz_queue_enable_aggregate(Q, -1, OMEGA_VF, 64, 1)) == FZ_E_BADARG && R(fz_queue_enable_aggregate(Q, BETA_VF, -1, 64, 1)) == FZ_E_BADARG);
    CHECK(R(fz_queue_enable_aggregate(Q, BETA_VF, OMEGA_VF, 0, 1)) == FZ_E_BADARG);
    for (int th : {0, 257}) CHECK(R(fz_queue_enable_aggregate(Q, BETA_VF, OMEGA_VF, 64, th)) == FZ_E_BADARG);
    refused(submit_rc(Q, *a), FZ_E_BADARG);              // a refused enable enables nothing
    CHECK(fz_queue_enable_aggregate(Q, BETA_VF, OMEGA_VF, 64, 1) == FZ_OK);
    for (int verify = 0; verify < 2; ++verify) {
        AG &x = verify ? *v : *a;
        auto ag = [&](const int32_t *vk, const char *m, const size_t *o, size_t n, const int32_t *rows, int flags, uint64_t *out) {
            return verify ? fz_queue_submit_verify(Q, vk, m, o, n, rows, &x.verdict, flags, out)
                          : fz_queue_submit_aggregate_verify(Q, vk, m, o, n, rows, x.agg_out.data(), &x.verdict, flags, out);
        };
        refused(ag(nullptr, x.msgs.data(), x.off.data(), 3, x.src(), 0, &t), FZ_E_BADARG);
        refused(ag(x.vk.data(), x.msgs.data(), nullptr, 3, x.src(), 0, &t), FZ_E_BADARG);
        refused(ag(x.vk.data(), x.msgs.data(), x.off.data(), 3, nullptr, 0, &t), FZ_E_BADARG);
        refused(ag(x.vk.data(), x.msgs.data(), x.off.data(), 3, x.src(), 0, nullptr), FZ_E_BADARG);
        refused(ag(x.vk.data(), x.msgs.data(), x.off.data(), 0, x.src(), 0, &t), FZ_E_BADARG);
        refused(ag(x.vk.data(), x.msgs.data(), x.off.data(), ((size_t)1 << 22) + 1, x.src(), 0, &t), FZ_E_BADARG);
        refused(ag(x.vk.data(), x.msgs.data(), x.off.data(), (size_t)1 << 21, x.src(), 0, &t), FZ_E_UNSUPPORTED);      // exact accumulation
        off = x.off;
        off[0] = 1;
        refused(ag(x.vk.data(), x.msgs.data(), off.data(), 3, x.src(), 0, &t), FZ_E_BADARG);
        off = x.off;
        CHECK(off[2] > 0);
        off[3] = off[2] - 1;
        refused(ag(x.vk.data(), x.msgs.data(), off.data(), 3, x.src(), 0, &t), FZ_E_BADARG);
        CHECK(x.off[3] > 0);
        refused(ag(x.vk.data(), nullptr, x.off.data(), 3, x.src(), 0, &t), FZ_E_BADARG);
        for (int flags : {FZ_QUEUE_KEEP_SK, FZ_QUEUE_DISCARD, FZ_QUEUE_ROWS_ON_DEVICE | FZ_QUEUE_DISCARD, 8})
            refused(ag(x.vk.data(), x.msgs.data(), x.off.data(), 3, x.src(), flags, &t), FZ_E_BADARG);
        off = x.off;                                     // two faults in one call (S11 pins these)
        off[0] = 1;
        refused(ag(x.vk.data(), x.msgs.data(), off.data(), 0, x.src(), 0, &t), FZ_E_BADARG, "between 1 and max_rows");
        refused(ag(x.vk.data(), nullptr, x.off.data(), 3, x.src(), 8, &t), FZ_E_BADARG, "h_msgs is NULL");
        CHECK(x.verdict == VERDICT_SENTINEL && t == 999);
    }
    refused(fz_queue_submit_verify(Q, v->vk.data(), v->msgs.data(), v->off.data(), 3, v->src(), nullptr, 0, &t), FZ_E_BADARG);
    submit(Q, *a);                                       // and both are accepted as they are
    CHECK(a->ticket == ++last);
    check_ag(Q, *a);
    submit(Q, *v);
    CHECK(v->ticket == ++last);
    check_ag(Q, *v);
    CHECK(R(fz_queue_wait(nullptr, 1, nullptr)) == FZ_E_BADARG && R(fz_queue_release(nullptr, 1)) == FZ_E_BADARG && R(fz_queue_drain(nullptr)) == FZ_E_BADARG);
    CHECK(R(fz_queue_stats(nullptr, nullptr, nullptr, nullptr)) == FZ_E_BADARG && fz_queue_destroy(nullptr) == FZ_OK);
    for (uint64_t unknown : {(uint64_t)0, last + 1}) {   // (S4 checks these codes; here their texts are on record)
        CHECK(R(fz_queue_wait(Q, unknown, nullptr)) == FZ_E_BADARG && R(fz_queue_release(Q, unknown)) == FZ_E_BADARG);
    }
    CHECK(R(fz_queue_release_after(Q, last, nullptr)) == FZ_E_BADARG);
    CHECK(fz_queue_destroy(Q) == FZ_OK);
}

// ---- S9: the aggregate flow -- alpha scattered back to the callers' order, G = 1 and 9, optional outputs, capacity, row kinds ----
static void s9_aggregate() {
    for (int threads : {1, 4}) {
        fz_queue *Q = mkq(1, 64, 64, threads);
        for (size_t G : {(size_t)1, (size_t)9}) {
            Hold h(Q);
            const size_t m0 = model_mark(), mark = stub_mark();
            std::vector<std::unique_ptr<AG>> a;
            bool permuted = false;
            for (size_t g = 0; g < G; ++g) {
                const int flags = g % 2 ? FZ_QUEUE_ROWS_ON_DEVICE : 0;
                a.push_back(g % 3 == 2 ? make_vf(G == 1 ? 6 : g + 1, 64, g == 5, flags) : make_ag(G == 1 ? 6 : g + 1, 64, flags));
                a.back()->want_agg = g != 3;
                a.back()->want_verdict = a.back()->verify_only || g != 4;
                permuted |= !a.back()->identity_order;
            }
            CHECK(permuted);                             // the order of submission is not the sorted one
            for (auto &x : a) submit(Q, *x);
            h.open();
            std::vector<const void *> srcs;
            std::vector<int> kinds;
            for (auto &x : a) { srcs.push_back(x->src()); kinds.push_back(x->d_rows ? (int)hipMemcpyDeviceToDevice : (int)hipMemcpyHostToDevice); }
            for (auto &x : a) check_ag(Q, *x);
            const std::vector<Call> log = stub_log(mark);
            for (size_t g = 0; g < G; ++g) {
                const Call *copy = nullptr;
                for (const Call &r : log) if (r.fn == "hipMemcpyAsync" && r.src == srcs[g]) { CHECK(!copy); copy = &r; }
                CHECK(copy && copy->kind == kinds[g]);
            }
            if (G == 9) {                                // runs of one kind: {0, 1}, {2}, {3, 4}, {5}, {6, 7}, {8}
                const std::vector<MRec> rag = only(model_log(m0), E_RAGGED);
                CHECK(rag.size() == 6 && rag[0].G == 2 && rag[1].G == 1 && rag[1].sig_null && rag[2].offs == (std::vector<size_t>{0, 4, 9}));
            }
        }
        CHECK(fz_queue_destroy(Q) == FZ_OK);
    }
    fz_queue *Q = mkq(1, 64, 3);                         // capacity 3: checked before anything else, the aggregate is still delivered
    std::vector<std::unique_ptr<AG>> a;
    a.push_back(make_ag(4, 3)); a.push_back(make_ag(3, 3)); a.push_back(make_vf(4, 3, false)); a.push_back(make_vf(3, 3, false));
    CHECK(a[0]->e_verdict == FZ_VERDICT_TOO_MANY_KEYS && a[1]->e_verdict == FZ_VERDICT_OK && a[2]->e_verdict == FZ_VERDICT_TOO_MANY_KEYS && a[3]->e_verdict == FZ_VERDICT_OK);
    for (auto &x : a) submit(Q, *x);
    for (auto &x : a) check_ag(Q, *x);
    CHECK(fz_queue_destroy(Q) == FZ_OK);
}

// ---- S10: four workers, four submitters, waits and releases on other threads ------------------------------------------
struct Item { std::unique_ptr<KS> ks; std::unique_ptr<AG> ag; };
static void s10_races(int per_thread) {
    fz_queue *Q = mkq(4, 24, 64, 4);
    std::mutex mu;
    std::condition_variable cv;
    std::deque<Item> handed;
    int submitters_left = 4;
    auto submitter = [&](int id) {
        for (int i = 0; i < per_thread; ++i) {
            const uint64_t r = mix((uint64_t)id * 1000 + (uint64_t)i);
            const size_t n = 1 + r % 9;
            Item it;
            switch ((r >> 8) % 6) {
                case 4: it.ag = make_ag(n, 64, (r >> 16) % 2 ? FZ_QUEUE_ROWS_ON_DEVICE : 0); submit(Q, *it.ag); break;
                case 5: it.ag = make_vf(n, 64, (r >> 20) % 2, (r >> 16) % 2 ? FZ_QUEUE_ROWS_ON_DEVICE : 0); submit(Q, *it.ag); break;
                default: it.ks = make_ks(n, (int)((r >> 8) % 6), (r >> 24) % 4 != 0); submit(Q, *it.ks);
            }
            std::lock_guard<std::mutex> g(mu);
            handed.push_back(std::move(it));
            cv.notify_one();
        }
        std::lock_guard<std::mutex> g(mu);
        --submitters_left;
        cv.notify_all();
    };
    auto waiter = [&](int id) {
        hipStream_t cs;
        fz_ctx *cons = consumer(&cs);
        for (int k = 0;; ++k) {
            Item it;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return !handed.empty() || submitters_left == 0; });
                if (handed.empty()) break;
                it = std::move(handed.front());
                handed.pop_front();
            }
            if (it.ag) { check_ag(Q, *it.ag); continue; }
            check_ks(Q, *it.ks, false);
            if ((k + id) % 3 == 0) CHECK(fz_queue_release_after(Q, it.ks->ticket, cons) == FZ_OK);
            else CHECK(fz_queue_release(Q, it.ks->ticket) == FZ_OK);
        }
        consumer_destroy(cons, cs);
    };
    std::vector<std::thread> th;
    for (int id = 0; id < 4; ++id) th.emplace_back(submitter, id);
    for (int id = 0; id < 3; ++id) th.emplace_back(waiter, id);
    for (auto &t : th) t.join();
    CHECK(fz_queue_drain(Q) == FZ_OK);
    const Stats s = stats(Q);
    CHECK(s.calls == (uint64_t)4 * per_thread && s.batches <= s.calls);
    CHECK(fz_queue_destroy(Q) == FZ_OK);
}

// ---- S11: a failing allocation -- in fz_queue_create, and in a batch on a cold worker ----------------------------------
// The stub's control fails allocations [at, at + 2): fz_malloc tries a failed hipMalloc once more, so two in a row fail one fz_malloc.
static long allocs_now() { std::lock_guard<std::mutex> g(g_log_mu); return g_allocs; }
static void fail_allocs(long at) { std::lock_guard<std::mutex> g(g_log_mu); g_fail_at = at; g_fail_n = at < 0 ? 1 : 2; }
static long s11_create() {
    long a0, e0, st0, a1, e1, st1;
    stub_live(&a0, &e0, &st0);
    const long base = allocs_now();
    fz_queue *Q = nullptr;
    CHECK(fz_queue_create(0, &g_P, RANK, BETA_SK, OMEGA_SK, g_A.data(), 2, 16, &Q) == FZ_OK && Q);
    const long total = allocs_now() - base;
    CHECK(total > 0 && fz_queue_destroy(Q) == FZ_OK);
    tdump(false);                                        // (two workers close side by side: no fixed order to print)
    for (long i = 0; i < total; ++i) {
        g_quiet = i != total - 1;                        // the trace holds the last one: the first worker whole, the second without its matrix
        fz_set_error(FZ_OK, "%s", "");
        fail_allocs(allocs_now() + i);
        Q = (fz_queue *)&a0;
        const int rc = fz_queue_create(0, &g_P, RANK, BETA_SK, OMEGA_SK, g_A.data(), 2, 16, &Q);
        fail_allocs(-1);
        tdump();
        CHECK(R(rc) != FZ_OK && fz_last_error()[0] && !Q);
        stub_live(&a1, &e1, &st1);
        CHECK(a1 == a0 && e1 == e0 && st1 == st0);
    }
    return total;
}
enum { FLOW_KS, FLOW_AG, FLOW_VF };
struct Cell {
    std::vector<std::unique_ptr<KS>> ks;
    std::vector<std::unique_ptr<AG>> ag;
    explicit Cell(int flow) {
        if (flow == FLOW_KS) { ks.push_back(make_ks(3, 0)); ks.push_back(make_ks(2, FZ_QUEUE_KEEP_SK)); ks.push_back(make_ks(4, FZ_QUEUE_DISCARD)); }
        else for (size_t n : {3, 1, 4}) ag.push_back(flow == FLOW_VF ? make_vf(n, 64, n == 1) : make_ag(n, 64));
    }
    void submit_all(fz_queue *Q) { for (auto &k : ks) submit(Q, *k); for (auto &x : ag) submit(Q, *x); }
    void check_all(fz_queue *Q) { for (auto &k : ks) check_ks(Q, *k); for (auto &x : ag) check_ag(Q, *x); }
};
// the allocations one batch of `flow` makes on a cold worker behind Hold (whose one-row call has grown the keygen-sign scratch)
static long s11_count(int flow) {
    fz_queue *Q = mkq(1, 64);
    Hold h(Q);
    Cell c(flow);
    const long base = allocs_now();
    c.submit_all(Q);
    h.open();
    for (auto &k : c.ks) CHECK(fz_queue_wait(Q, k->ticket, nullptr) == FZ_OK);
    for (auto &x : c.ag) CHECK(fz_queue_wait(Q, x->ticket, nullptr) == FZ_OK);
    const long total = allocs_now() - base;
    c.check_all(Q);
    CHECK(total > 0 && fz_queue_destroy(Q) == FZ_OK);
    return total;
}
static void s11_cell(int flow, long i) {
    fz_queue *Q = mkq(1, 64);
    Hold h(Q);
    Cell c(flow);
    const long before = live_allocs();
    const size_t mark = stub_mark();
    fail_allocs(allocs_now() + i);
    c.submit_all(Q);
    h.open();
    int worker_tid = -1;
    auto failed = [&](uint64_t ticket) {
        fz_queue_result r;
        memset(&r, 0xff, sizeof(r));
        CHECK(F("wait", fz_queue_wait(Q, ticket, &r)) == FZ_E_HIP && strstr(fz_last_error(), "queued batch failed"));
        CHECK(r.status == FZ_E_HIP && !r.d_vk && !r.d_sig && !r.d_sk_hat);
    };
    for (int k = 0; k < 2 && flow == FLOW_KS; ++k) failed(c.ks[k]->ticket);
    for (auto &x : c.ag) failed(x->ticket);
    if (flow == FLOW_KS) {                               // the discarded call: its failure surfaces once, in drain
        CHECK(fz_queue_wait(Q, c.ks[2]->ticket, nullptr) == FZ_OK);
        CHECK(F("drain", fz_queue_drain(Q)) == FZ_E_HIP && strstr(fz_last_error(), "a discarded call failed"));
    }
    CHECK(fz_queue_drain(Q) == FZ_OK);
    fail_allocs(-1);
    for (auto &k : c.ks) CHECK(k->vk_out == std::vector<int32_t>(k->n() * 2 * D, VK_SENTINEL));
    for (auto &x : c.ag) CHECK(x->verdict == VERDICT_SENTINEL && x->agg_out == std::vector<int32_t>(RANK * D, AGG_SENTINEL));
    // every copy that read a caller's rows is behind a synchronise of its stream on the worker's thread
    const std::vector<Call> log = stub_log(mark);
    for (const Call &r : log) if (r.fn == "hipMalloc failed") worker_tid = r.tid;
    CHECK(worker_tid >= 0 && worker_tid != stub_tid());
    for (auto &x : c.ag)
        for (const Call &r : log) {
            if (r.fn != "hipMemcpyAsync" || r.src != x->src()) continue;
            bool drained = false;
            for (const Call &s : log) drained |= s.fn == "hipStreamSynchronize" && s.stream == r.stream && s.seq > r.seq && s.tid == worker_tid;
            CHECK(drained);
        }
    for (int k = 0; k < 2 && flow == FLOW_KS; ++k) CHECK(fz_queue_release(Q, c.ks[k]->ticket) == FZ_OK);
    for (auto &x : c.ag) CHECK(fz_queue_release(Q, x->ticket) == FZ_OK);
    flush(Q);
    // What the batch took is back.  A keygen-sign batch replaces scratch the holding call had grown, and the flush grows the one
    // area that was lost again: the count is the one before the batch.  The aggregate scratch was cold: the i areas fitted
    // before the failing one stay the worker's scratch (as after a batch that succeeds), and nothing else does.
    CHECK(live_allocs() == before + (flow == FLOW_KS ? 0 : i));
    Hold again(Q);                                       // the same batch again is right
    c.submit_all(Q);
    again.open();
    c.check_all(Q);
    CHECK(fz_queue_destroy(Q) == FZ_OK);
    tdump();
}
static void s11_alloc() {
    const long create = s11_create();
    long n[3];
    for (int flow : {FLOW_KS, FLOW_AG, FLOW_VF}) {
        g_quiet = true;
        n[flow] = s11_count(flow);
        tdump();
        for (long i = 0; i < n[flow]; ++i) {
            // the trace holds two cells: the second block of a kept batch (the first goes back), an area in the middle of the aggregate scratch
            g_quiet = !((flow == FLOW_KS && i == 3) || (flow == FLOW_AG && i == 5));
            if (g_trace && !g_quiet) printf("# %s, allocation %ld of the batch fails\n", flow == FLOW_KS ? "keygen-sign" : "aggregate-verify", i);
            s11_cell(flow, i);
        }
    }
    g_quiet = false;
    if (!g_trace) printf("S11 allocations: create %ld, keygen-sign %ld, aggregate-verify %ld, verify %ld\n", create, n[0], n[1], n[2]);
}

// ---- the recorded trace: fixed one-worker flows, one line per event (tests/golden/queue_runtime_trace.txt) ----------------
// A flow keeps one thread at a time busy (Hold, waits, flush), so the order of the two logs does not depend on timing.
static void t_idle() {
    printf("# flow 1: create, enable and destroy an idle queue\n");
    fz_queue *Q = mkq(1, 64);
    CHECK(fz_queue_destroy(Q) == FZ_OK);
    tdump();
}
static void t_flags() {
    printf("# flow 2: the S3 batches, cold scratch then warm\n");
    fz_queue *Q = mkq(1, 64);
    for (int round = 0; round < 2; ++round) {
        for (int part = 0; part < 2; ++part) {
            printf("# round %d, %s\n", round, part ? "a batch nobody keeps" : "mixed flags");
            Hold h(Q);
            std::vector<std::unique_ptr<KS>> c;
            if (part == 0) for (int flags : {0, FZ_QUEUE_KEEP_SK, FZ_QUEUE_DISCARD, FZ_QUEUE_DISCARD | FZ_QUEUE_KEEP_SK}) c.push_back(make_ks(3 + c.size(), flags));
            else for (int flags : {FZ_QUEUE_DISCARD, FZ_QUEUE_DISCARD | FZ_QUEUE_KEEP_SK, FZ_QUEUE_DISCARD}) c.push_back(make_ks(20 + c.size(), flags));
            for (auto &k : c) submit(Q, *k);
            h.open();
            for (auto &k : c) check_ks(Q, *k);
            CHECK(fz_queue_drain(Q) == FZ_OK);
            flush(Q);
            tdump();
        }
    }
    CHECK(fz_queue_destroy(Q) == FZ_OK);
    tdump();
}
static void t_grow() {
    printf("# flow 3: batches that grow the scratch, 4 rows then 40\n");
    fz_queue *Q = mkq(1, 64);
    for (size_t n : {4, 40}) {
        Hold h(Q);
        std::unique_ptr<KS> k = make_ks(n, FZ_QUEUE_DISCARD);
        submit(Q, *k);
        h.open();
        check_ks(Q, *k);
        tdump();
    }
    for (size_t n : {4, 40})
        for (int verify = 0; verify < 2; ++verify) {
            std::unique_ptr<AG> a = verify ? make_vf(n, 64, false) : make_ag(n, 64);
            submit(Q, *a);
            check_ag(Q, *a);
            tdump();
        }
    CHECK(fz_queue_destroy(Q) == FZ_OK);
    tdump();
}
static void t_aggregate() {
    for (int threads : {1, 4}) {
        printf("# flow 4: the aggregate batch of S9, G = 9, host_threads %d\n", threads);
        fz_queue *Q = mkq(1, 64, 64, threads);
        Hold h(Q);
        std::vector<std::unique_ptr<AG>> a;
        for (size_t g = 0; g < 9; ++g) {
            const int flags = g % 2 ? FZ_QUEUE_ROWS_ON_DEVICE : 0;
            a.push_back(g % 3 == 2 ? make_vf(g + 1, 64, g == 5, flags) : make_ag(g + 1, 64, flags));
            a.back()->want_agg = g != 3;
            a.back()->want_verdict = a.back()->verify_only || g != 4;
        }
        for (auto &x : a) submit(Q, *x);
        h.open();
        for (auto &x : a) CHECK(fz_queue_wait(Q, x->ticket, nullptr) == FZ_OK);      // (the callers' device rows are freed once the worker is idle)
        for (auto &x : a) check_ag(Q, *x);
        CHECK(fz_queue_destroy(Q) == FZ_OK);
        tdump();
    }
}
static void t_failing_steps() {
    printf("# flow 5: one failing step of each kind\n");
    fz_queue *Q = mkq(1, 64);
    const int codes[3] = {FZ_E_HIP, FZ_E_UNSUPPORTED, FZ_E_BADARG};
    int injected = 0;
    for (int entry : {E_SAMPLE, E_KEYGEN, E_CHAL, E_SIGN}) {
        printf("# keygen-sign, %s fails\n", ENTRY[entry]);
        Hold h(Q);
        arm(entry, entry == E_SAMPLE ? 0 : 1, codes[injected % 3], "injected failure #" + std::to_string(injected));
        ++injected;
        Cell c(FLOW_KS);
        c.submit_all(Q);
        h.open();
        for (int k = 0; k < 2; ++k) CHECK(F("wait", fz_queue_wait(Q, c.ks[k]->ticket, nullptr)) != FZ_OK);
        CHECK(fz_queue_wait(Q, c.ks[2]->ticket, nullptr) == FZ_OK);
        CHECK(F("drain", fz_queue_drain(Q)) != FZ_OK && fz_queue_drain(Q) == FZ_OK);
        for (int k = 0; k < 2; ++k) CHECK(fz_queue_release(Q, c.ks[k]->ticket) == FZ_OK);
        disarm();
        flush(Q);
        tdump();
    }
    // (the verify flow shares its first steps with the aggregate flow: S6 fails each of them, the trace holds the one that is its own)
    const std::pair<int, int> steps[6] = {{FLOW_AG, E_CHAL}, {FLOW_AG, E_NTT}, {FLOW_AG, E_RAGGED}, {FLOW_AG, E_VPART}, {FLOW_AG, E_REDUCE}, {FLOW_VF, E_VTGT}};
    for (const auto &step : steps) {
        const int flow = step.first, entry = step.second;
        printf("# %s, %s fails\n", flow == FLOW_VF ? "verify" : "aggregate-verify", ENTRY[entry]);
        Hold h(Q);
        arm(entry, entry == E_CHAL ? 1 : 0, codes[injected % 3], "injected failure #" + std::to_string(injected));
        ++injected;
        Cell c(flow);
        c.submit_all(Q);
        h.open();
        for (auto &x : c.ag) CHECK(F("wait", fz_queue_wait(Q, x->ticket, nullptr)) != FZ_OK);
        CHECK(fz_queue_drain(Q) == FZ_OK);
        for (auto &x : c.ag) CHECK(fz_queue_release(Q, x->ticket) == FZ_OK);
        disarm();
        flush(Q);
        tdump();
    }
    CHECK(fz_queue_destroy(Q) == FZ_OK);
    tdump();
    printf("# a failing allocation: in create, then in each batch (S11)\n");
    s11_alloc();
}
static void t_release() {
    printf("# flow 6: release, release_after with one consumer, release of a released ticket\n");
    hipStream_t cs;
    fz_ctx *cons = consumer(&cs);
    g_consumer_streams.insert(cs);
    fz_queue *Q = mkq(1, 64);
    Hold h(Q);
    std::vector<std::unique_ptr<KS>> c;
    c.push_back(make_ks(3, 0)); c.push_back(make_ks(2, FZ_QUEUE_KEEP_SK));
    for (auto &k : c) submit(Q, *k);
    h.open();
    for (auto &k : c) check_ks(Q, *k, false);
    CHECK(fz_queue_release(Q, c[0]->ticket) == FZ_OK);
    CHECK(fz_queue_release_after(Q, c[1]->ticket, cons) == FZ_OK);
    flush(Q);
    tdump();
    printf("# released before\n");
    CHECK(fz_queue_release(Q, c[0]->ticket) == FZ_OK && fz_queue_release_after(Q, c[1]->ticket, cons) == FZ_OK);
    flush(Q);
    CHECK(fz_queue_destroy(Q) == FZ_OK);
    tdump();
    consumer_destroy(cons, cs);
    tdump();
    g_consumer_streams.clear();
}
static void t_destroy() {
    printf("# flow 7: destroy with two results unreleased\n");
    fz_queue *Q = mkq(1, 64);
    Hold h(Q);
    std::vector<std::unique_ptr<KS>> c;
    c.push_back(make_ks(3, 0)); c.push_back(make_ks(2, FZ_QUEUE_KEEP_SK));
    for (auto &k : c) submit(Q, *k);
    h.open();
    for (auto &k : c) check_ks(Q, *k, false);
    CHECK(fz_queue_destroy(Q) == FZ_OK);
    tdump();
}

int main(int argc, char **argv) {
    setenv("FZ_POOL_MB", "0", 1);                        // every fz_free is a hipFree
    for (int i = 0; i < RANK * D; ++i) g_A.push_back(1 + md((int64_t)(mix(777 + (uint64_t)i) >> 2)) % (int32_t)(MQ - 1));
    g_caller_tid = stub_tid();
    if (argc > 1 && !strcmp(argv[1], "trace")) {
        g_trace = true;
        t_idle(); t_flags(); t_grow(); t_aggregate(); t_failing_steps(); t_release(); t_destroy();
        printf("# the refusals of S8\n");
        s8_refusals();
        printf("# end\n");
        return 0;
    }
    long a0, e0, st0, a1, e1, st1;
    stub_live(&a0, &e0, &st0);
    s1_cut();        printf("S1 ok\n");
    s2_kinds();      printf("S2 ok\n");
    s3_flags();      printf("S3 ok\n");
    s4_release_counts(); printf("S4 ok\n");
    s5_release_after();  printf("S5 ok\n");
    s6_errors();     printf("S6 ok\n");
    s7_destroy();    printf("S7 ok\n");
    s8_refusals();   printf("S8 ok\n");
    s9_aggregate();  printf("S9 ok\n");
    s10_races(argc > 1 ? atoi(argv[1]) : 50); printf("S10 ok\n");
    s11_alloc();     printf("S11 ok\n");
    stub_live(&a1, &e1, &st1);
    CHECK(a1 == a0 && e1 == e0 && st1 == st0);           // every queue and context gave back what it took
    printf("done\n");
    return 0;
}
'''

SCENARIOS = ["S%d ok" % k for k in range(1, 12)]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "queue_runtime_trace.txt")
PLAIN = "-fno-sanitize=all"                                   # the build without a sanitizer, in the place of a sanitizer's option


def _run(tmp_path, san, name, env):
    """-> (the scenarios' run, the trace's run) of one build"""
    toolchain()                                               # (skips without hipcc)
    if not sanitizer_links(tmp_path, san):
        pytest.skip("the runtime of %s is not available" % san)
    exe = build_driver(tmp_path, UNITS, DRIVER, san, name=name, sources=[os.path.join(CSRC, "fz_host.cpp")],
                       flags=["-fno-sanitize-recover=all"] if "address" in san else [])
    env = dict(os.environ, FZ_POOL_MB="0", **env)
    return [subprocess.run([str(exe)] + args, capture_output=True, text=True, timeout=300, env=env) for args in ([], ["trace"])]


def _same_trace(r):
    """the trace of this build is the recorded one (tests/golden: recorded from the unit before its steps were written once)"""
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    got = r.stdout.splitlines()
    with open(GOLDEN) as fh:
        want = fh.read().splitlines()
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, "trace line %d: got %r, recorded %r (after %r)" % (k + 1, g, w, got[max(0, k - 3):k])
    assert len(got) == len(want) and got[-1] == "# end", "the trace has %d lines, the recorded one %d" % (len(got), len(want))


def test_queue_under_asan_ubsan_and_leak_detection(tmp_path):
    r, t = _run(tmp_path, "-fsanitize=address,undefined", "queue_asan",
                dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert [ln for ln in r.stdout.splitlines() if ln.endswith(" ok")] == SCENARIOS and r.stdout.splitlines()[-1] == "done"
    assert "ERROR" not in t.stderr and "runtime error" not in t.stderr, t.stderr[-3000:]
    _same_trace(t)


def test_queue_under_tsan(tmp_path):
    r, t = _run(tmp_path, "-fsanitize=thread", "queue_tsan", dict(TSAN_OPTIONS="halt_on_error=0:report_signal_unsafe=0"))
    if "FATAL: ThreadSanitizer" in r.stderr and "unexpected memory mapping" in r.stderr:
        pytest.skip("ThreadSanitizer cannot map its shadow memory in this container")
    assert "WARNING: ThreadSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    assert [ln for ln in r.stdout.splitlines() if ln.endswith(" ok")] == SCENARIOS and r.stdout.splitlines()[-1] == "done"
    assert "WARNING: ThreadSanitizer" not in t.stderr, t.stderr[-4000:]
    _same_trace(t)


def test_queue_trace_without_a_sanitizer(tmp_path):
    r, t = _run(tmp_path, PLAIN, "queue_plain", {})
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    assert [ln for ln in r.stdout.splitlines() if ln.endswith(" ok")] == SCENARIOS and r.stdout.splitlines()[-1] == "done"
    _same_trace(t)
