"""The lifetime logic of a context (csrc/fz_context.hip, csrc/fz_diag.hip) without a GPU: the two units are compiled for the host
with AddressSanitizer + UndefinedBehaviorSanitizer and linked, as a stand-alone program, against the stub HIP runtime of
tests/_hip_stub.py.  The stub backs device and pinned memory with malloc / free and streams, events and graphs with small heap
objects, logs every call with its arguments and has two controls: "the stream is capturing" and "the k-th allocation (or event
creation) fails".  The driver asserts the one rule of the growable areas from that log (fit, growth, capacities, zeroing, retire
after a capture, refusal during one, the dirty re-zero), that fz_ctx_destroy misses nothing (leak detection reports a stub
allocation that is never released, ASan a double free) and that every allocation site of the two units may be the failing one."""
import os
import re
import subprocess

from _hip_stub import CSRC, STUB, build_driver, toolchain

UNITS = ("fz_context", "fz_diag")
# what fz_last_error() names when an allocation of the two units fails: one entry per site (the areas share fz_area_replace)
ALLOC_WHATS = {"table alloc", "verdict alloc", "scratch alloc", "scratch2 alloc", "verify scratch alloc", "verify state alloc",
               "aggregation scratch alloc", "challenge table alloc", "stamp buffer alloc", "diag alloc", "hipMalloc", "event create"}

DRIVER = STUB + r'''
// ---- the driver ------------------------------------------------------------------------------------------------------
#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s   (last error: %s)\n", __LINE__, #cond, fz_last_error()); exit(1); } } while (0)
static const uint32_t Q = 2147465729u;
static size_t count(size_t mark, const char *fn, const void *p = nullptr, bool match_p = false) {
    size_t c = 0;
    for (size_t i = mark; i < g_log.size(); ++i) c += g_log[i].fn == fn && (!match_p || g_log[i].p == p);
    return c;
}
static size_t heavy(size_t mark) {        // what a capture must not see
    return count(mark, "hipMalloc") + count(mark, "hipMalloc failed") + count(mark, "hipFree") + count(mark, "hipStreamSynchronize") +
           count(mark, "hipMemsetAsync");
}
static bool has(size_t mark, const char *fn, const void *p, size_t n, const void *stream) {
    for (size_t i = mark; i < g_log.size(); ++i)
        if (g_log[i].fn == fn && g_log[i].p == p && g_log[i].n == n && g_log[i].stream == stream) return true;
    return false;
}
static fz_ctx *make(int kind, hipStream_t *stream) {      // 0: degree 256, 1: degree 64, 2: ring-only; on a stream of its own
    fz_ctx *c = nullptr;
    const int rc = kind == 0 ? fz_ctx_create(0, Q, 256, 3337519u, 1978410468u, &c)
                 : kind == 1 ? fz_ctx_create(0, Q, 64, 23584283u, 540632852u, &c) : fz_ctx_create(0, Q, 100, 0, 0, &c);
    if (rc != FZ_OK) { CHECK(c == nullptr); return nullptr; }
    CHECK(fz_stream_create(c, (void **)stream) == FZ_OK && fz_ctx_set_stream(c, *stream) == FZ_OK);
    return c;
}

// one way of asking per area: ask(n) requests n units; need(n) / cap(n) = bytes asked for / allocated when it does not fit
struct Area {
    int which;
    std::function<int(fz_ctx *, size_t)> ask;
    std::function<size_t(size_t)> need, cap;
    bool zeroed;
};
static const size_t kTileWords = 24, kDeg = 64;
static std::vector<Area> areas() {
    void *vp = nullptr; double *part = nullptr; int *state = nullptr; unsigned long long *acc = nullptr; int *verdict = nullptr;
    return {
        {FZ_A_SCRATCH, [=](fz_ctx *c, size_t n) mutable { return fz_scratch(c, n, &vp); }, [](size_t n) { return n; }, [](size_t n) { return n + n / 4 + 4096; }, false},
        {FZ_A_SCRATCH2, [=](fz_ctx *c, size_t n) mutable { return fz_scratch(c, n, &vp, FZ_A_SCRATCH2); }, [](size_t n) { return n; }, [](size_t n) { return n + n / 4 + 4096; }, false},
        {FZ_A_VERDICT, [=](fz_ctx *c, size_t n) mutable { return fz_verdict_area(c, n, &verdict); }, [](size_t n) { return n * 4; }, [](size_t n) { return n * 4; }, false},
        // n doubles in ONE group: the state words (capacity 17 groups) stay as they are
        {FZ_A_VPART, [=](fz_ctx *c, size_t n) mutable { return fz_verify_scratch(c, 1, n, &part, &state); }, [](size_t n) { return n * 8; }, [](size_t n) { return (n + n / 4) * 8; }, true},
        // n groups of ONE double: the accumulators (grown first) stay as they are
        {FZ_A_VSTATE, [=](fz_ctx *c, size_t n) mutable { return fz_verify_scratch(c, n, 1, &part, &state); }, [](size_t n) { return n * 8; }, [](size_t n) { return (n + n / 4 + 16) * 8; }, true},
        {FZ_A_AGGACC, [=](fz_ctx *c, size_t n) mutable { return fz_agg_scratch(c, n, kTileWords, &acc); }, [](size_t n) { return n * kTileWords * 8; }, [](size_t n) { return (n + n / 4 + 8) * kTileWords * 8; }, true},
    };
}

static void test_fit_growth_zeroing() {
    hipStream_t st = nullptr;
    fz_ctx *c = make(1, &st);
    CHECK(c && c->area[FZ_A_VERDICT].bytes == 64 * sizeof(int));          // 64 ints at creation
    {   // both verify areas exist, at their smallest: from here on a request grows ONE area
        double *part = nullptr; int *state = nullptr;
        CHECK(fz_verify_scratch(c, 1, 1, &part, &state) == FZ_OK && c->area[FZ_A_VPART].bytes == 8 && c->area[FZ_A_VSTATE].bytes == 17 * 8);
    }
    for (const Area &a : areas()) {
        FzArea &A = c->area[a.which];
        // sizes: n1 does not fit what exists, n2 does not fit n1's capacity
        const size_t n1 = a.which == FZ_A_VERDICT ? 100 : a.which == FZ_A_VSTATE ? 40 : 3000;
        const size_t n2 = a.which == FZ_A_VERDICT ? 101 : 4 * n1;
        for (size_t n : {n1, n2}) {
            CHECK(a.need(n) > A.bytes);
            void *old = A.p;
            size_t mark = g_log.size();
            CHECK(a.ask(c, n) == FZ_OK);
            CHECK(count(mark, "hipStreamSynchronize") == 1 && has(mark, "hipStreamSynchronize", nullptr, 0, st));
            CHECK(count(mark, "hipFree") == (old ? 1u : 0u) && count(mark, "hipFree", old, true) == (old ? 1u : 0u));
            CHECK(count(mark, "hipMalloc") == 1 && has(mark, "hipMalloc", A.p, a.cap(n), nullptr) && A.bytes == a.cap(n));
            // new verify / aggregation areas: zeroed over the whole capacity on the context's stream, nothing on the null stream
            CHECK(count(mark, "hipMemsetAsync") == (a.zeroed ? (a.which == FZ_A_AGGACC ? 1u : 2u) : 0u));
            if (a.zeroed) CHECK(has(mark, "hipMemsetAsync", A.p, A.bytes, st));
            for (size_t i = mark; i < g_log.size(); ++i) CHECK(g_log[i].fn != "hipMemsetAsync" || g_log[i].stream == st);
            void *p = A.p;
            mark = g_log.size();
            CHECK(a.ask(c, n) == FZ_OK && a.ask(c, n - 1) == FZ_OK && a.ask(c, n) == FZ_OK);      // equal, smaller, equal
            CHECK(g_log.size() == mark && A.p == p);                                               // no runtime call at all
        }
    }
    // a different tile size cannot alias: the capacity is in bytes
    unsigned long long *acc = nullptr;
    const size_t tiles = c->area[FZ_A_AGGACC].bytes / (kTileWords * 8), mark = g_log.size();
    CHECK(fz_agg_scratch(c, tiles, 2 * kTileWords, &acc) == FZ_OK && count(mark, "hipMalloc") == 1);
    CHECK(c->area[FZ_A_AGGACC].bytes == (tiles + tiles / 4 + 8) * 2 * kTileWords * 8);
    CHECK(fz_ctx_destroy(c) == FZ_OK);
    CHECK(hipStreamDestroy(st) == hipSuccess);
}

// the dirty flags, set the way the launchers set them after a failed launch
static void test_dirty() {
    hipStream_t st = nullptr;
    fz_ctx *c = make(1, &st);
    double *part; int *state; unsigned long long *acc;
    CHECK(c && fz_verify_scratch(c, 4, kDeg, &part, &state) == FZ_OK && fz_agg_scratch(c, 9, kTileWords, &acc) == FZ_OK);
    CHECK(!c->verify_dirty && !c->agg_dirty);
    size_t mark = g_log.size();
    c->verify_dirty = 1;
    CHECK(fz_verify_scratch(c, 4, kDeg, &part, &state) == FZ_OK && !c->verify_dirty && g_log.size() == mark + 2);
    CHECK(has(mark, "hipMemsetAsync", c->area[FZ_A_VPART].p, c->area[FZ_A_VPART].bytes, st));
    CHECK(has(mark, "hipMemsetAsync", c->area[FZ_A_VSTATE].p, c->area[FZ_A_VSTATE].bytes, st));
    mark = g_log.size();
    c->agg_dirty = 1;
    CHECK(fz_agg_scratch(c, 9, kTileWords, &acc) == FZ_OK && !c->agg_dirty && g_log.size() == mark + 1);
    CHECK(has(mark, "hipMemsetAsync", c->area[FZ_A_AGGACC].p, c->area[FZ_A_AGGACC].bytes, st));
    CHECK(fz_verify_scratch(c, 4, kDeg, &part, &state) == FZ_OK && fz_agg_scratch(c, 9, kTileWords, &acc) == FZ_OK && g_log.size() == mark + 1);
    CHECK(fz_ctx_destroy(c) == FZ_OK && hipStreamDestroy(st) == hipSuccess);
}

// every growing request is refused before any runtime call, every fitting one succeeds; `own`: the context's own capture
// (fz_graph_begin), else only the runtime reports one (the stream joined another context's capture)
static void test_capture(bool own) {
    hipStream_t st = nullptr;
    fz_ctx *c = make(0, &st);
    CHECK(c != nullptr);
    std::vector<size_t> fit;
    for (const Area &a : areas()) { fit.push_back(a.which == FZ_A_VSTATE ? 10 : 64); CHECK(a.ask(c, fit.back()) == FZ_OK); }
    CHECK(fz_area_replace(c, FZ_A_CHAL_TAB, 4096) == FZ_OK && fz_diag_stamps_begin(c, 4, 64) == FZ_OK);
    if (own) CHECK(fz_graph_begin(c) == FZ_OK && c->capturing); else g_report_capture = true;
    const size_t mark = g_log.size();
    size_t k = 0;
    for (const Area &a : areas()) {
        const size_t n = fit[k++];
        void *p = c->area[a.which].p;
        CHECK(a.ask(c, n) == FZ_OK);
        CHECK(a.ask(c, c->area[a.which].bytes + 1) == FZ_E_BADARG && strstr(fz_last_error(), "would grow during graph capture"));
        CHECK(a.ask(c, n) == FZ_OK && c->area[a.which].p == p);
    }
    CHECK(fz_area_replace(c, FZ_A_CHAL_TAB, 8192) == FZ_E_BADARG && fz_diag_stamps_begin(c, 4, 128) == FZ_E_BADARG);
    double *part; int *state; unsigned long long *acc;
    c->verify_dirty = 1;
    CHECK(fz_verify_scratch(c, 1, 64, &part, &state) == FZ_E_BADARG && strstr(fz_last_error(), "not during graph capture") && c->verify_dirty);
    c->agg_dirty = 1;
    CHECK(fz_agg_scratch(c, 64, kTileWords, &acc) == FZ_E_BADARG && strstr(fz_last_error(), "not during graph capture") && c->agg_dirty);
    CHECK(heavy(mark) == 0);
    fz_graph *G = nullptr;
    if (own) CHECK(fz_graph_end(c, &G) == FZ_OK && G); else g_report_capture = false;
    // outside the capture the re-zero happens
    CHECK(fz_verify_scratch(c, 1, 64, &part, &state) == FZ_OK && fz_agg_scratch(c, 64, kTileWords, &acc) == FZ_OK && !c->verify_dirty && !c->agg_dirty);
    CHECK(count(mark, "hipMemsetAsync") == 3);
    CHECK(fz_graph_destroy(G) == FZ_OK && fz_ctx_destroy(c) == FZ_OK && hipStreamDestroy(st) == hipSuccess);
}

// once a graph was captured, growth frees nothing: the old areas live until fz_ctx_destroy, which frees each exactly once
static void test_retire() {
    hipStream_t st = nullptr;
    fz_ctx *c = make(1, &st);
    CHECK(c != nullptr);
    for (const Area &a : areas()) CHECK(a.ask(c, a.which == FZ_A_VSTATE ? 10 : 64) == FZ_OK);
    CHECK(fz_area_replace(c, FZ_A_CHAL_TAB, 4096) == FZ_OK && fz_diag_stamps_begin(c, 4, 64) == FZ_OK);
    fz_graph *G = nullptr;
    CHECK(fz_graph_begin(c) == FZ_OK && fz_graph_end(c, &G) == FZ_OK);
    std::vector<void *> old;
    for (const FzArea &A : c->area) { CHECK(A.p); old.push_back(A.p); }
    const size_t mark = g_log.size();
    for (const Area &a : areas()) CHECK(a.ask(c, 100000) == FZ_OK);
    CHECK(fz_area_replace(c, FZ_A_CHAL_TAB, 8192) == FZ_OK && fz_diag_stamps_begin(c, 4, 128) == FZ_OK);
    for (size_t i = 0; i < old.size(); ++i) CHECK(c->area[i].p != old[i]);
    CHECK(count(mark, "hipFree") == 0 && c->n_retired == FZ_A_COUNT);
    CHECK(fz_graph_launch(c, G) == FZ_OK);
    CHECK(fz_ctx_destroy(c) == FZ_OK);
    for (void *p : old) CHECK(count(mark, "hipFree", p, true) == 1);
    CHECK(fz_graph_destroy(G) == FZ_OK && hipStreamDestroy(st) == hipSuccess);
}

// Everything a context can own, then destroy: the script of the failing-allocation runs (armed: calls may fail, every failure is
// an error code and its text is collected) and of "destroy misses nothing" (unarmed: every call succeeds)
static std::set<std::string> g_whats;
static void script(int kind, bool armed) {
    auto ok = [&](int rc) {
        if (rc != FZ_OK) {
            CHECK(armed && (rc == FZ_E_HIP || rc == FZ_E_BADARG));
            const char *e = fz_last_error(), *colon = strchr(e, ':');
            g_whats.insert(colon ? std::string(e, colon) : std::string(e));
        }
        return rc == FZ_OK;
    };
    hipStream_t st = nullptr;
    fz_ctx *c = nullptr;
    {
        const int rc = kind == 0 ? fz_ctx_create(0, Q, 256, 3337519u, 1978410468u, &c)
                     : kind == 1 ? fz_ctx_create(0, Q, 64, 23584283u, 540632852u, &c) : fz_ctx_create(0, Q, 100, 0, 0, &c);
        if (!ok(rc)) { CHECK(c == nullptr); return; }
    }
    CHECK(fz_stream_create(c, (void **)&st) == FZ_OK && fz_ctx_set_stream(c, st) == FZ_OK);
    for (int round = 0; round < 2; ++round) {                 // the second round grows everything once more
        for (const Area &a : areas()) ok(a.ask(c, (a.which == FZ_A_VSTATE ? 10 : 64) << (12 * round)));
        ok(fz_area_replace(c, FZ_A_CHAL_TAB, 4096 << round));
        ok(fz_profile_begin(c, 4 << round, 1));
        double fwd = 0, inv = 0;
        int nf = 0, ni = 0;
        ok(fz_profile_end(c, &fwd, &nf, &inv, &ni));          // (a capture is refused while profiling is on)
        ok(fz_diag_stamps_begin(c, 4, 64 << round));
        double mhz = 0;
        ok(fz_diag_shader_clock(c, 10, &mhz));
        if (round == 0) {                                     // retire from here on
            fz_graph *G = nullptr;
            if (ok(fz_graph_begin(c)) && ok(fz_graph_end(c, &G))) CHECK(fz_graph_destroy(G) == FZ_OK);
        }
    }
    // the lazily created fields these units only release
    if (!c->d_mt_init && hipMalloc((void **)&c->d_mt_init, 624 * 4) != hipSuccess) c->d_mt_init = nullptr;
    for (auto &s : c->chal_stage) {
        if (hipHostMalloc((void **)&s.h, 1024, 0) == hipSuccess) s.bytes = 1024; else s.h = nullptr;
        if (hipEventCreateWithFlags(&s.ev, 0) == hipSuccess) { CHECK(hipEventRecord(s.ev, st) == hipSuccess); s.busy = 1; }
    }
    // the block pool: A comes back and is handed out again (a live block with an event), B stays in the pool, C is never freed
    void *A = nullptr, *A2 = nullptr, *B = nullptr, *C = nullptr;
    if (ok(fz_malloc(c, 1 << 20, &A))) ok(fz_free(c, A));
    ok(fz_malloc(c, 1 << 20, &A2));
    if (!armed) CHECK(A2 == A && c->n_live == 1 && c->live_blocks[0].ev);
    if (ok(fz_malloc(c, 3 << 20, &B))) ok(fz_free(c, B));
    ok(fz_malloc(c, 5 << 20, &C));
    if (!armed) CHECK(c->n_pool == 1 && c->n_live == 2);
    CHECK(fz_ctx_destroy(c) == FZ_OK);
    if (A2) CHECK(hipFree(A2) == hipSuccess);                 // blocks the caller never freed stay the caller's
    if (C) CHECK(hipFree(C) == hipSuccess);
    CHECK(hipStreamDestroy(st) == hipSuccess);
}

int main() {
    test_fit_growth_zeroing();
    test_dirty();
    test_capture(true);
    test_capture(false);
    test_retire();
    for (int kind = 0; kind < 3; ++kind) {
        g_allocs = g_events = 0;
        script(kind, false);                                  // destroy misses nothing (leak detection at exit)
        const long allocs = g_allocs, events = g_events;
        printf("kind %d: %ld allocations, %ld events\n", kind, allocs, events);
        for (g_fail_n = 1; g_fail_n <= 2; ++g_fail_n)         // two in a row: fz_malloc retries once after flushing the pools
            for (long k = 0; k < allocs; ++k) { g_allocs = 0; g_fail_at = k; script(kind, true); }
        g_fail_at = -1;
        g_fail_n = 1;
        for (long k = 0; k < events; ++k) { g_events = 0; g_fail_event_at = k; script(kind, true); }
        g_fail_event_at = -1;
    }
    for (const std::string &w : g_whats) printf("what: %s\n", w.c_str());
    printf("done\n");
    return 0;
}
'''


def test_context_lifetime_under_asan_ubsan_and_leak_detection(tmp_path):
    toolchain()                                               # (skips without hipcc)
    # a new allocation site in the two units has to become the failing one in the script (and be named in ALLOC_WHATS)
    text = "".join(open(os.path.join(CSRC, unit + ".hip")).read() for unit in UNITS)
    assert len(re.findall(r"\bhip(?:Host)?Malloc\w*\(", text)) == 5, "allocation sites changed: extend the driver's script"
    exe = build_driver(tmp_path, UNITS, DRIVER, "-fsanitize=address,undefined", flags=["-fno-sanitize-recover=all"])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    assert "done" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    whats = {ln[len("what: "):] for ln in r.stdout.splitlines() if ln.startswith("what: ")}
    assert ALLOC_WHATS <= whats, sorted(ALLOC_WHATS - whats)
