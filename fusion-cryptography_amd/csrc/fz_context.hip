// fz_context.hip -- what a context owns (include/fusion_hip.h): error reporting, creation and destruction with the twiddle
// tables and the knobs, the growable device areas, streams, graph capture, events and the block pool behind fz_malloc / fz_free.
#include "fz_internal.h"
#include "../../include/fusion_hip.h"
#include "../../include/fusion_hip_diag.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <atomic>
#include <mutex>

// block pool + context registry (defined with fz_malloc / fz_free below)
static void pool_release_locked(fz_ctx *ctx, size_t keep);
static void fz_registry_add(fz_ctx *c);
static void fz_registry_remove(fz_ctx *c);

static thread_local char g_err[512] = "";

int fz_set_error(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int fz_check_hip(hipError_t e, const char *what) {
    if (e == hipSuccess) return FZ_OK;
    return fz_set_error(FZ_E_HIP, "%s: %s", what, hipGetErrorString(e));
}

static uint64_t powmod_u64(uint64_t b, uint64_t e, uint64_t q) {
    unsigned __int128 r = 1, x = b % q;
    while (e) {
        if (e & 1) r = (r * x) % q;
        x = (x * x) % q;
        e >>= 1;
    }
    return (uint64_t)r;
}

static unsigned bitrev(unsigned i, int k) {
    unsigned r = 0;
    for (int b = 0; b < k; ++b) r |= ((i >> b) & 1u) << (k - 1 - b);
    return r;
}

// A device allocation that is being replaced by a larger one.  A graph captured on this context may hold its address
// (fz_graph_*: recorded pointers are fixed), and a replay must never touch freed memory: once any graph was captured the
// old allocation is kept until fz_ctx_destroy instead of being freed.
int fz_retire(fz_ctx *ctx, void *d_ptr, const char *what) {
    if (!d_ptr) return FZ_OK;
    if (!ctx->graphs_captured) return fz_check_hip(hipFree(d_ptr), what);
    if (ctx->n_retired == ctx->cap_retired) {
        const int cap = ctx->cap_retired ? 2 * ctx->cap_retired : 16;
        void **r = (void **)realloc(ctx->retired, sizeof(void *) * (size_t)cap);
        if (!r) return fz_set_error(FZ_E_HIP, "out of host memory");
        ctx->retired = r;
        ctx->cap_retired = cap;
    }
    ctx->retired[ctx->n_retired++] = d_ptr;
    return FZ_OK;
}

// what the messages call each area (FZ_A_*)
static const char *const kAreaName[FZ_A_COUNT] = {"scratch", "scratch2", "verdict", "verify scratch", "verify state", "aggregation scratch",
                                                  "challenge table", "stamp buffer"};

int fz_area_replace(fz_ctx *ctx, int which, size_t capacity) {
    FzArea &a = ctx->area[which];
    const char *name = kAreaName[which];
    if (fz_capturing(ctx))
        return fz_set_error(FZ_E_BADARG, "%s would grow during graph capture: run the sequence once before fz_graph_begin", name);
    char what[48];
    snprintf(what, sizeof what, "%s sync", name);
    FZ_HIP(hipStreamSynchronize(ctx->stream), what);
    snprintf(what, sizeof what, "%s free", name);
    FZ_TRY(fz_retire(ctx, a.p, what));             // a captured sequence keeps a valid (if stale) area
    a.p = nullptr;
    a.bytes = 0;
    snprintf(what, sizeof what, "%s alloc", name);
    FZ_HIP(hipMalloc(&a.p, capacity), what);
    a.bytes = capacity;
    return FZ_OK;
}

// `dirty`: an earlier launch failed, or the area is new -- do not trust "zero between launches".  On the context's stream: a
// null-stream memset is not ordered with a non-blocking stream (found by tools/soak.py)
static int rezero(fz_ctx *ctx, int *dirty, int first, int last, const char *name) {
    if (!*dirty) return FZ_OK;
    if (fz_capturing(ctx)) return fz_set_error(FZ_E_BADARG, "%s must be re-zeroed: not during graph capture", name);
    for (int w = first; w <= last; ++w) {
        char what[48];
        snprintf(what, sizeof what, "%s clear", kAreaName[w]);
        FZ_HIP(hipMemsetAsync(ctx->area[w].p, 0, ctx->area[w].bytes, ctx->stream), what);
    }
    *dirty = 0;
    return FZ_OK;
}

int fz_verify_scratch(fz_ctx *ctx, size_t groups, size_t doubles_per_group, double **part, int **state) {
    const size_t need = groups * doubles_per_group, cap = groups + groups / 4 + 16;
    bool fresh = false;
    FZ_TRY(fz_area_fit(ctx, FZ_A_VPART, need * sizeof(double), (need + need / 4) * sizeof(double), &fresh));
    FZ_TRY(fz_area_fit(ctx, FZ_A_VSTATE, groups * 2 * sizeof(int), cap * 2 * sizeof(int), &fresh));
    if (fresh) ctx->verify_dirty = 1;
    FZ_TRY(rezero(ctx, &ctx->verify_dirty, FZ_A_VPART, FZ_A_VSTATE, "verify scratch"));
    *part = (double *)ctx->area[FZ_A_VPART].p;
    *state = (int *)ctx->area[FZ_A_VSTATE].p;
    return FZ_OK;
}

// the verdicts of fz_verify_with_target_batch: 64 ints from context creation on, then exactly what is asked for
int fz_verdict_area(fz_ctx *ctx, size_t groups, int **d_verdict) {
    FZ_TRY(fz_area_fit(ctx, FZ_A_VERDICT, groups * sizeof(int), groups * sizeof(int)));
    *d_verdict = (int *)ctx->area[FZ_A_VERDICT].p;
    return FZ_OK;
}

// accumulator words of the one-pass aggregation (zero between launches; see aggregate_onepass)
int fz_agg_scratch(fz_ctx *ctx, size_t tiles, size_t tile_words, unsigned long long **acc) {
    const size_t word = tile_words * sizeof(unsigned long long);
    bool fresh = false;
    FZ_TRY(fz_area_fit(ctx, FZ_A_AGGACC, tiles * word, (tiles + tiles / 4 + 8) * word, &fresh));
    if (fresh) ctx->agg_dirty = 1;
    FZ_TRY(rezero(ctx, &ctx->agg_dirty, FZ_A_AGGACC, FZ_A_AGGACC, "aggregation scratch"));
    *acc = (unsigned long long *)ctx->area[FZ_A_AGGACC].p;
    return FZ_OK;
}

extern "C" {

const char *fz_version(void) { return "fusion_hip 0.1.0 (gfx950)"; }
const char *fz_last_error(void) { return g_err; }

int fz_device_count(int *out_count) {
    FZ_REQUIRE(out_count, "out_count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *out_count = 0;
        return fz_set_error(FZ_E_NODEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    *out_count = n;
    return FZ_OK;
}

static int upload_doubles(const double *h, size_t n, double **d_out) {
    FZ_HIP(hipMalloc((void **)d_out, (n ? n : 1) * sizeof(double)), "table alloc");
    if (n) FZ_HIP(hipMemcpy(*d_out, h, n * sizeof(double), hipMemcpyHostToDevice), "table upload");
    return FZ_OK;
}

// what the kernel units need from context creation (fz_internal.h), in the order it runs them
static int (*const kUnitSetup[])(fz_ctx *) = {
    fz_ntt_query_grid,           fz_records_query_grid,                fz_aggregate_encoded_query_grid, fz_verify_encoded_setup,
    fz_sign_encoded_query_grid,  fz_aggregate_many_encoded_query_grid, fz_sign_records_query_grid,      fz_keygen_records_query_grid,
};

// h_fwd / h_inv != NULL: the context's twiddle tables are THESE (fz_ctx_create_tables) instead of the bit-reversed powers of a root
static int ctx_create(int device_id, uint32_t q, int degree, uint32_t root, uint32_t inv_root, const uint32_t *h_fwd, const uint32_t *h_inv,
                      fz_ctx **out) {
    FZ_REQUIRE(out, "out is NULL");
    *out = nullptr;
    // any odd modulus below 2^32: centred residues |x| <= (q - 1) / 2 < 2^31 are int32 whatever q is, and every bound of
    // fz_arith.h is in terms of 2^31-sized operands and twiddles below 2^32 (round 5; rounds 1-4 refused q >= 2^31)
    FZ_REQUIRE(q >= 3 && (q & 1u), "modulus %u must be odd and >= 3", q);
    // root == 0: "ring-only" context (pointwise ops, norm/weight, matvec on rows of `degree` values;
    // no transform tables).  The reference lets polynomial objects exist for parameter tuples that
    // admit no NTT (e.g. root_order 1), and their + - * norm weight still work.
    const bool tables = h_fwd != nullptr;
    const bool ring_only = !tables && (root == 0);
    if (ring_only) {
        FZ_REQUIRE(degree >= 1 && degree <= (1 << 20), "degree %d out of range", degree);
    } else {
        FZ_REQUIRE(degree >= 2 && (degree & (degree - 1)) == 0, "degree %d must be a power of two >= 2", degree);
        if (degree > kFzMaxDegree) return fz_set_error(FZ_E_UNSUPPORTED, "degree %d > %d not supported by the NTT kernels", degree, kFzMaxDegree);
        if (tables) {
            FZ_REQUIRE(h_inv, "both tables are required");
        } else {
            FZ_REQUIRE(((uint64_t)q - 1) % (2u * (uint64_t)degree) == 0, "2*degree=%d does not divide q-1", 2 * degree);
            FZ_REQUIRE(root > 0 && root < q && inv_root > 0 && inv_root < q, "root / inv_root must be in (0, q)");
            // primitive 2*degree-th root (order a power of two): root^degree == -1
            FZ_REQUIRE(powmod_u64(root, (uint64_t)degree, q) == (uint64_t)q - 1,
                       "root %u is not a primitive %d-th root of unity mod %u", root, 2 * degree, q);
            FZ_REQUIRE(((uint64_t)root * inv_root) % q == 1, "root * inv_root != 1 mod q");
        }
    }

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fz_set_error(FZ_E_NODEVICE, "no HIP device available");
    FZ_REQUIRE(device_id >= 0 && device_id < ndev, "device_id %d out of range (0..%d)", device_id, ndev - 1);
    FZ_HIP(hipSetDevice(device_id), "hipSetDevice");

    fz_ctx *c = new (std::nothrow) fz_ctx();
    if (!c) return fz_set_error(FZ_E_HIP, "out of host memory");      // (value-initialised: every field is zero)
    c->device = device_id;
    hipDeviceProp_t prop;
    int rc = fz_check_hip(hipGetDeviceProperties(&prop, device_id), "hipGetDeviceProperties");
    if (rc != FZ_OK) { delete c; return rc; }
    c->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    c->q = q; c->root = root; c->inv_root = inv_root;
    c->degree = degree;
    c->logd = ring_only ? -1 : 0;
    if (!ring_only) while ((1 << c->logd) < degree) ++c->logd;
    c->mod = fz_make_mod(q);

    double *tw = nullptr, *itw = nullptr, *twB = nullptr, *itwB = nullptr, *pairs = nullptr;
    size_t nB = 0;
    const int n = ring_only ? 0 : degree, k = c->logd;
    if (!ring_only) {
        c->h_tw = (uint32_t *)malloc(sizeof(uint32_t) * n);
        c->h_itw = (uint32_t *)malloc(sizeof(uint32_t) * n);
        tw = (double *)malloc(sizeof(double) * n);
        itw = (double *)malloc(sizeof(double) * n);
        if (k >= 5 && k <= 8) {             // per-lane tables of the contiguous pass, (w, w * K / q) pairs: filled below
            nB = (size_t)(16 - (16 >> (k - 4))) * (n / 16) * 2;
            twB = (double *)malloc(sizeof(double) * nB);
            itwB = (double *)malloc(sizeof(double) * nB);
        }
        pairs = (double *)malloc(sizeof(double) * 4 * (size_t)n);
        if (!c->h_tw || !c->h_itw || !tw || !itw || (nB && (!twB || !itwB)) || !pairs) {
            free(tw); free(itw); free(twB); free(itwB); free(pairs);
            fz_ctx_destroy(c);
            return fz_set_error(FZ_E_HIP, "out of host memory");
        }
        for (int i = 0; i < n; ++i) {
            // bit_reverse_copy([pow(root, i, q)])  (algebra/polynomials.py:396-397, :416-417) -- or whatever table the caller
            // hands to cooley_tukey_ntt / gentleman_sande_intt (ntt.py:274-290, :354-372 use it as it is)
            c->h_tw[i] = tables ? h_fwd[i] % q : (uint32_t)powmod_u64(root, bitrev((unsigned)i, k), q);
            c->h_itw[i] = tables ? h_inv[i] % q : (uint32_t)powmod_u64(inv_root, bitrev((unsigned)i, k), q);
            tw[i] = (double)c->h_tw[i];
            itw[i] = (double)c->h_itw[i];
        }
        const uint64_t n_inv = powmod_u64((uint64_t)n, (uint64_t)q - 2, q);
        for (int i = 0; i < 16; ++i) {
            c->twA.w[i] = (i < n) ? tw[i] : 0.0;
            c->itwA.w[i] = (i < n) ? itw[i] : 0.0;
            c->twA.w2[i] = c->twA.w[i] * c->mod.kq;
            c->itwA.w2[i] = c->itwA.w[i] * c->mod.kq;
        }
        c->twA.n_inv = c->itwA.n_inv = (double)n_inv;
        c->twA.w1_n_inv = 0.0;
        c->itwA.w1_n_inv = (double)(((unsigned __int128)c->h_itw[1] * n_inv) % q);
        c->twA.n_inv2 = c->itwA.n_inv2 = c->itwA.n_inv * c->mod.kq;
        c->twA.w1_n_inv2 = 0.0;
        c->itwA.w1_n_inv2 = c->itwA.w1_n_inv * c->mod.kq;

        // per-lane tables of the contiguous pass ([NE][L]); see fz_ntt_dev.h / tools/ntt_layout_model.py
        if (k >= 5 && k <= 8) {
            const int L = n / 16, SB = k - 4;
            for (int ls = 0; ls < SB; ++ls) {
                {   // forward: distance 2^(SB-1-ls), ng groups per lane
                    const int t = 1 << (SB - 1 - ls), ng = 16 / (2 * t);
                    const int ebase = (16 >> SB) * ((1 << ls) - 1);
                    for (int g = 0; g < ng; ++g)
                        for (int b = 0; b < L; ++b) {
                            const double w = tw[(16 << ls) + b * ng + g];
                            twB[((size_t)(ebase + g) * L + b) * 2] = w;
                            twB[((size_t)(ebase + g) * L + b) * 2 + 1] = w * c->mod.kq;
                        }
                }
                {   // inverse: distance 2^ls
                    const int ng = 8 >> ls, ebase = 16 - (16 >> ls);
                    for (int g = 0; g < ng; ++g)
                        for (int b = 0; b < L; ++b) {
                            const double w = itw[(n >> (ls + 1)) + b * ng + g];
                            itwB[((size_t)(ebase + g) * L + b) * 2] = w;
                            itwB[((size_t)(ebase + g) * L + b) * 2 + 1] = w * c->mod.kq;
                        }
                }
            }
        }
    }

    rc = fz_check_hip(hipEventCreate(&c->ev0), "event create");
    if (rc == FZ_OK) rc = fz_check_hip(hipEventCreate(&c->ev1), "event create");
    if (rc == FZ_OK) rc = upload_doubles(tw, n, &c->d_tw);
    if (rc == FZ_OK) rc = upload_doubles(itw, n, &c->d_itw);
    if (rc == FZ_OK && !ring_only) {
        for (int i = 0; i < n; ++i) {
            pairs[2 * i] = tw[i];
            pairs[2 * i + 1] = tw[i] * c->mod.kq;
            pairs[2 * n + 2 * i] = itw[i];
            pairs[2 * n + 2 * i + 1] = itw[i] * c->mod.kq;
        }
        rc = upload_doubles(pairs, 2 * (size_t)n, &c->d_tw2);
        if (rc == FZ_OK) rc = upload_doubles(pairs + 2 * n, 2 * (size_t)n, &c->d_itw2);
    }
    {
        // every benchmarking / test knob is read HERE, once: no entry point consults the environment afterwards (DESIGN.md
        // section 10 lists them; round 4 removed the knobs of closed experiments together with their instantiations)
        auto knob = [](const char *name) { const char *v = getenv(name); return v ? atoi(v) : 0; };
        c->force_kernel = knob("FZ_NTT_KERNEL");
        c->knob_ntt_rows = knob("FZ_NTT_ROWS");
        // measured crossover, inputs NOT cache-resident, both schedules on one box: degree 256 -- the radix-4 kernels lead up to
        // 2^14 rows (4.23 / 5.58 / 8.47 us at 2^12 .. 2^14 against 4.97 / 6.53 / 9.10 for the 16-per-lane kernel), the 16-per-lane
        // kernel from 24 576 rows (6 x 4096: 13.7 us against 14.2; 2^15: 14.6 against 15.6) -- round 5's kernel, whose start-up
        // overlaps the first chunk with the twiddle table (profiles/r05_ntt_crossover.txt; rounds 3-4: from 2^16);
        // degree 64 -- radix-4 up to 2^18 rows (round 2's measurement)
        c->small_batch_rows = degree == 256 ? (3 << 13) : (1 << 19);
        c->knob_agg_direct = knob("FZ_AGG_DIRECT");
        c->knob_shake_full = knob("FZ_SHAKE_FORM");
        c->knob_verify_ordered = knob("FZ_VERIFY_ORDERED");
        // The fence-free cross-workgroup combine of verify_fused (relaxed agent-scope atomics on the library's own
        // coarse-grained scratch, ordered by data dependence: csrc/fz_scheme_fused.hip) is an argument about THIS chip's memory-side
        // atomics; anything that does not report gfx950 gets the acquire/release instantiation.
        if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) c->knob_verify_ordered = 1;
        c->knob_unfused = knob("FZ_UNFUSED");
        c->knob_polymul_form = knob("FZ_POLYMUL_FORM");
        c->knob_no_imad = knob("FZ_NO_IMAD");
        c->knob_matvec_slices = knob("FZ_MATVEC_SLICES");
        c->knob_verify_cent = knob("FZ_VERIFY_CENT");
        c->knob_multi_order = getenv("FZ_MULTI_ORDER") ? knob("FZ_MULTI_ORDER") : 1;
        c->knob_hash_ag_order = getenv("FZ_HASH_AG_ORDER") ? knob("FZ_HASH_AG_ORDER") : 1;
        // fz_malloc's block pool: FZ_POOL_MB megabytes at most over all contexts of the process (default 4096, 0 = every fz_free is a hipFree)
        c->pool_cap = (size_t)(getenv("FZ_POOL_MB") ? (knob("FZ_POOL_MB") < 0 ? 0 : knob("FZ_POOL_MB")) : 4096) << 20;
    }
    if (rc == FZ_OK) rc = upload_doubles(twB, nB, &c->d_twB);
    if (rc == FZ_OK) rc = upload_doubles(itwB, nB, &c->d_itwB);
    if (rc == FZ_OK && nB) {
        static_assert(sizeof(FzTwA) == 36 * sizeof(double), "FzTwA is 36 doubles");
        const FzTwA both[2] = {c->twA, c->itwA};
        rc = upload_doubles(reinterpret_cast<const double *>(both), 72, &c->d_twAB);
    }
    int *d_verdict = nullptr;
    if (rc == FZ_OK) rc = fz_verdict_area(c, 64, &d_verdict);
    for (const auto setup : kUnitSetup)
        if (rc == FZ_OK && !ring_only) rc = setup(c);
    free(tw); free(itw); free(twB); free(itwB); free(pairs);
    if (rc != FZ_OK) { fz_ctx_destroy(c); return rc; }
    fz_registry_add(c);
    *out = c;
    return FZ_OK;
}

int fz_ctx_create(int device_id, uint32_t q, int degree, uint32_t root, uint32_t inv_root, fz_ctx **out) {
    return ctx_create(device_id, q, degree, root, inv_root, nullptr, nullptr, out);
}

// cooley_tukey_ntt / gentleman_sande_intt take the twiddle table as an ARGUMENT and use whatever they are handed
// (algebra/ntt.py:274-290, :354-372: `s = bit_rev_root_powers[m + i]`): a context whose tables are the caller's own lists --
// not necessarily the powers of one root -- runs the same butterfly network on them.  Entries are reduced mod q.
int fz_ctx_create_tables(int device_id, uint32_t q, int degree, const uint32_t *h_fwd, const uint32_t *h_inv, fz_ctx **out) {
    FZ_REQUIRE(h_fwd && h_inv, "both tables are required (pass the same one twice when only one direction is used)");
    return ctx_create(device_id, q, degree, 0, 0, h_fwd, h_inv, out);
}

int fz_ctx_destroy(fz_ctx *ctx) {
    if (!ctx) return FZ_OK;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    // the fixed tables and the lazily built ones
    void *const fixed[] = {ctx->d_tw, ctx->d_itw, ctx->d_tw2, ctx->d_itw2, ctx->d_twB, ctx->d_itwB, ctx->d_twAB, ctx->d_mt_init, ctx->d_diag, ctx->d_venc};
    for (void *p : fixed)
        if (p) (void)hipFree(p);
    for (FzArea &a : ctx->area)
        if (a.p) (void)hipFree(a.p);
    for (int i = 0; i < 2 * ctx->prof_cap; ++i) (void)hipEventDestroy(ctx->prof_ev[i]);
    free(ctx->prof_ev);
    free(ctx->prof_kind);
    for (int i = 0; i < ctx->n_retired; ++i) (void)hipFree(ctx->retired[i]);
    free(ctx->retired);
    fz_registry_remove(ctx);
    {
        std::lock_guard<std::mutex> g(ctx->pool_mu);
        pool_release_locked(ctx, 0);
        for (int i = 0; i < ctx->n_live; ++i)
            if (ctx->live_blocks[i].ev) (void)hipEventDestroy(ctx->live_blocks[i].ev);
    }
    free(ctx->pool_blocks);
    free(ctx->live_blocks);          // (blocks the caller never freed stay the caller's)
    for (auto &st : ctx->chal_stage) {
        if (st.ev) { if (st.busy) (void)hipEventSynchronize(st.ev); (void)hipEventDestroy(st.ev); }
        if (st.h) (void)hipHostFree(st.h);
    }
    if (ctx->diag_stream) (void)hipStreamDestroy(ctx->diag_stream);
    free(ctx->stamp_first);
    free(ctx->stamp_count);
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    free(ctx->h_tw);
    free(ctx->h_itw);
    delete ctx;
    return FZ_OK;
}

int fz_ctx_set_stream(fz_ctx *ctx, void *hip_stream) {
    FZ_REQUIRE(ctx, "ctx is NULL");
    if (fz_capturing(ctx)) return fz_set_error(FZ_E_BADARG, "the stream cannot change during graph capture");
    if (ctx->stream != (hipStream_t)hip_stream) {
        // the accumulator words of the one-pass aggregation / fused verification, the scratch areas and the blocks of the
        // pool belong to the context, not to a stream: work still in flight on the old stream must not share them with
        // work on the new one.  Unconditional on every change (a context with only pooled or live blocks used to skip it).
        FZ_DEV(ctx);
        FZ_HIP(hipStreamSynchronize(ctx->stream), "stream change: synchronise the old stream");
    }
    ctx->stream = (hipStream_t)hip_stream;
    return FZ_OK;
}

int fz_ctx_synchronize(fz_ctx *ctx) {
    FZ_REQUIRE(ctx, "ctx is NULL");
    FZ_DEV(ctx);
    if (fz_capturing(ctx)) return fz_set_error(FZ_E_BADARG, "synchronisation is not allowed during graph capture");
    FZ_HIP(hipStreamSynchronize(ctx->stream), "stream synchronize");
    return FZ_OK;
}

int fz_stream_create(fz_ctx *ctx, void **out_stream) {
    FZ_REQUIRE(ctx && out_stream, "NULL argument");
    FZ_DEV(ctx);
    hipStream_t s = nullptr;
    FZ_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), "stream create");
    *out_stream = (void *)s;
    return FZ_OK;
}

int fz_stream_create_priority(fz_ctx *ctx, int high, void **out_stream) {
    FZ_REQUIRE(ctx && out_stream, "NULL argument");
    FZ_DEV(ctx);
    int least = 0, greatest = 0;                     // numerically LOWER = higher priority
    FZ_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest), "stream priority range");
    hipStream_t s = nullptr;
    FZ_HIP(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, high ? greatest : least), "stream create");
    *out_stream = (void *)s;
    return FZ_OK;
}

int fz_stream_destroy(fz_ctx *ctx, void *hip_stream) {
    FZ_REQUIRE(ctx, "ctx is NULL");
    FZ_DEV(ctx);
    if (!hip_stream) return FZ_OK;
    if (ctx->stream == (hipStream_t)hip_stream) return fz_set_error(FZ_E_BADARG, "the stream is still attached to this context");
    FZ_HIP(hipStreamDestroy((hipStream_t)hip_stream), "stream destroy");
    return FZ_OK;
}

// ---- graph capture: a launch-bound sequence of device-pointer calls recorded once, replayed with one call ------
int fz_graph_begin(fz_ctx *ctx) {
    FZ_REQUIRE(ctx, "ctx is NULL");
    FZ_DEV(ctx);
    if (fz_capturing(ctx)) return fz_set_error(FZ_E_BADARG, "a capture is already open on this context (or its stream has joined another context's)");
    if (ctx->stream == nullptr)
        return fz_set_error(FZ_E_BADARG, "graph capture needs a non-default stream (fz_ctx_set_stream)");
    if (ctx->prof_on) return fz_set_error(FZ_E_BADARG, "per-dispatch profiling is on: events cannot be captured");
    FZ_HIP(hipSetDevice(ctx->device), "hipSetDevice");
    FZ_HIP(hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeRelaxed), "begin capture");
    ctx->capturing = 1;
    return FZ_OK;
}

int fz_graph_end(fz_ctx *ctx, fz_graph **out_graph) {
    FZ_REQUIRE(ctx && out_graph, "NULL argument");
    FZ_DEV(ctx);
    if (!ctx->capturing) return fz_set_error(FZ_E_BADARG, "no capture is open on this context");
    ctx->capturing = 0;
    hipGraph_t g = nullptr;
    FZ_HIP(hipStreamEndCapture(ctx->stream, &g), "end capture");
    if (!g) return fz_set_error(FZ_E_HIP, "the capture produced no graph (a captured call failed)");
    hipGraphExec_t ex = nullptr;
    hipError_t e = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
    if (e != hipSuccess) {
        (void)hipGraphDestroy(g);
        return fz_check_hip(e, "graph instantiate");
    }
    fz_graph *G = new (std::nothrow) fz_graph;
    if (!G) {
        (void)hipGraphExecDestroy(ex);
        (void)hipGraphDestroy(g);
        return fz_set_error(FZ_E_HIP, "out of host memory");
    }
    ctx->graphs_captured++;
    G->graph = g;
    G->exec = ex;
    G->device = ctx->device;
    *out_graph = G;
    return FZ_OK;
}

int fz_graph_launch(fz_ctx *ctx, fz_graph *graph) {
    FZ_REQUIRE(ctx && graph, "NULL argument");
    FZ_DEV(ctx);
    if (fz_capturing(ctx)) return fz_set_error(FZ_E_BADARG, "a graph cannot be launched into its own capture");
    if (graph->device != ctx->device) return fz_set_error(FZ_E_BADARG, "graph was captured on device %d", graph->device);
    FZ_HIP(hipGraphLaunch(graph->exec, ctx->stream), "graph launch");
    return FZ_OK;
}

int fz_graph_destroy(fz_graph *graph) {
    if (!graph) return FZ_OK;
    (void)hipGraphExecDestroy(graph->exec);
    (void)hipGraphDestroy(graph->graph);
    delete graph;
    return FZ_OK;
}

// ---- events: ordering between the streams of two contexts ------------------------------------------------------------
struct fz_event {
    hipEvent_t ev;
    int device;
};

int fz_event_create(fz_ctx *ctx, fz_event **out) {
    FZ_REQUIRE(ctx && out, "NULL argument");
    *out = nullptr;
    FZ_DEV(ctx);
    fz_event *e = new (std::nothrow) fz_event();
    if (!e) return fz_set_error(FZ_E_HIP, "out of host memory");
    e->device = ctx->device;
    hipError_t rc = hipEventCreateWithFlags(&e->ev, hipEventDisableTiming);
    if (rc != hipSuccess) { delete e; return fz_check_hip(rc, "event create"); }
    *out = e;
    return FZ_OK;
}

int fz_event_record(fz_ctx *ctx, fz_event *ev) {
    FZ_REQUIRE(ctx && ev, "NULL argument");
    if (ev->device != ctx->device) return fz_set_error(FZ_E_BADARG, "event was created on device %d", ev->device);
    FZ_DEV(ctx);
    FZ_HIP(hipEventRecord(ev->ev, ctx->stream), "event record");
    return FZ_OK;
}

int fz_event_wait(fz_ctx *ctx, fz_event *ev) {
    FZ_REQUIRE(ctx && ev, "NULL argument");
    if (ev->device != ctx->device) return fz_set_error(FZ_E_BADARG, "event was created on device %d", ev->device);
    FZ_DEV(ctx);
    FZ_HIP(hipStreamWaitEvent(ctx->stream, ev->ev, 0), "stream wait event");
    return FZ_OK;
}

int fz_event_destroy(fz_event *ev) {
    if (!ev) return FZ_OK;
    (void)hipSetDevice(ev->device);
    hipError_t rc = hipEventDestroy(ev->ev);
    delete ev;
    return fz_check_hip(rc, "event destroy");
}

int fz_ctx_twiddles(fz_ctx *ctx, uint32_t *h_fwd, uint32_t *h_inv) {
    FZ_REQUIRE(ctx, "ctx is NULL");
    if (ctx->logd < 0) return fz_set_error(FZ_E_UNSUPPORTED, "ring-only context has no transform tables");
    if (h_fwd) memcpy(h_fwd, ctx->h_tw, sizeof(uint32_t) * ctx->degree);
    if (h_inv) memcpy(h_inv, ctx->h_itw, sizeof(uint32_t) * ctx->degree);
    return FZ_OK;
}

// Blocks of kPoolMin bytes or more that come back through fz_free are kept and handed out again by fz_malloc for requests
// they fit without wasting more than a quarter: hipFree of a large block takes ~180 us and synchronises the whole device
// (measured: 1 MiB 1 us, 16 MiB - 1 GiB 178-190 us; hipMalloc 10-12 us), which is most of what a 1024-key keygen_batch spent
// outside its kernels.
// Safety of reuse: fz_free records an event on the context's stream and the stream that takes the block out of the pool
// waits for it, so the block's previous users (queued on the context's stream at fz_free time -- the documented requirement
// of fz_free, include/fusion_hip.h) finish before its next ones start, whatever fz_ctx_set_stream did in between (which
// also drains the old stream on every change).  The arrays are guarded by pool_mu.
// Budget: ONE process-wide cap (FZ_POOL_MB, default 4096) over the pools of all contexts -- sixteen private contexts
// (tools/probes/concurrent_batches.py) share it instead of stranding 4 GiB each; fz_pool_trim gives a context's blocks back
// (Context.close calls it); a failed hipMalloc flushes the pools of EVERY context on the device before it retries.
static const size_t kPoolMin = 256 << 10;
static std::mutex g_ctx_mu;                       // registry of live contexts (fz_ctx_create / fz_ctx_destroy)
static fz_ctx *g_ctxs[256];
static int g_nctx = 0;
static std::atomic<size_t> g_pool_bytes{0};       // bytes idle in all pools of the process

static void fz_registry_add(fz_ctx *c) {
    std::lock_guard<std::mutex> g(g_ctx_mu);
    if (g_nctx < 256) g_ctxs[g_nctx++] = c;
}

static void fz_registry_remove(fz_ctx *c) {
    std::lock_guard<std::mutex> g(g_ctx_mu);
    for (int i = 0; i < g_nctx; ++i)
        if (g_ctxs[i] == c) { g_ctxs[i] = g_ctxs[--g_nctx]; break; }
}

static bool grow(fz_ctx::FzBlock *&arr, int &cap, int need) {
    if (need <= cap) return true;
    const int ncap = cap ? 2 * cap : 64;
    fz_ctx::FzBlock *n = (fz_ctx::FzBlock *)realloc(arr, (size_t)ncap * sizeof(fz_ctx::FzBlock));
    if (!n) return false;
    arr = n;
    cap = ncap;
    return true;
}

// pool_mu held: hand pooled blocks back to the runtime, oldest first, until at most `keep` bytes stay
static void pool_release_locked(fz_ctx *ctx, size_t keep) {
    int k = 0;
    while (k < ctx->n_pool && ctx->pool_bytes > keep) {
        fz_ctx::FzBlock &b = ctx->pool_blocks[k++];
        (void)hipFree(b.p);                          // synchronises the device: whatever still used the block has finished
        if (b.ev) (void)hipEventDestroy(b.ev);
        ctx->pool_bytes -= b.bytes;
        g_pool_bytes -= b.bytes;
    }
    for (int i = k; i < ctx->n_pool; ++i) ctx->pool_blocks[i - k] = ctx->pool_blocks[i];
    ctx->n_pool -= k;
}

// a hipMalloc failed: idle blocks of ANY context on this device may be what stands in the way
static void pool_flush_device(int device) {
    std::lock_guard<std::mutex> g(g_ctx_mu);
    for (int i = 0; i < g_nctx; ++i) {
        fz_ctx *c = g_ctxs[i];
        if (c->device != device) continue;
        std::lock_guard<std::mutex> gp(c->pool_mu);
        pool_release_locked(c, 0);
    }
}

int fz_pool_trim(fz_ctx *ctx, size_t keep_bytes) {
    FZ_REQUIRE(ctx, "ctx is NULL");
    FZ_DEV(ctx);
    if (fz_capturing(ctx)) return fz_set_error(FZ_E_BADARG, "the pool cannot be trimmed during graph capture (hipFree synchronises)");
    std::lock_guard<std::mutex> g(ctx->pool_mu);
    pool_release_locked(ctx, keep_bytes);
    return FZ_OK;
}

int fz_malloc(fz_ctx *ctx, size_t bytes, void **d_out) {
    FZ_REQUIRE(ctx && d_out, "NULL argument");
    FZ_DEV(ctx);
    if (bytes == 0) bytes = 1;
    void *p = nullptr;
    hipEvent_t ev = nullptr;
    if (bytes >= kPoolMin && !fz_capturing(ctx)) {       // (a pooled block's event was recorded outside the capture: not waitable inside one)
        std::lock_guard<std::mutex> g(ctx->pool_mu);
        int best = -1;
        for (int i = 0; i < ctx->n_pool; ++i) {
            const size_t b = ctx->pool_blocks[i].bytes;
            if (b >= bytes && b - bytes <= bytes / 4 && (best < 0 || b < ctx->pool_blocks[best].bytes)) best = i;
        }
        if (best >= 0) {
            p = ctx->pool_blocks[best].p;
            bytes = ctx->pool_blocks[best].bytes;
            ev = ctx->pool_blocks[best].ev;
            ctx->pool_bytes -= bytes;
            g_pool_bytes -= bytes;
            for (int k = best + 1; k < ctx->n_pool; ++k) ctx->pool_blocks[k - 1] = ctx->pool_blocks[k];    // keeps age order
            --ctx->n_pool;
        }
    }
    if (p && ev) {
        // the next users of the block run after its previous ones (a no-op when both are on one stream)
        hipError_t e = hipStreamWaitEvent(ctx->stream, ev, 0);
        if (e != hipSuccess) { (void)hipGetLastError(); (void)hipEventSynchronize(ev); }
    }
    if (!p) {
        hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) {                        // out of memory: give every idle block on this device back and try once more
            (void)hipGetLastError();
            pool_flush_device(ctx->device);
            e = hipMalloc(&p, bytes);
        }
        FZ_HIP(e, "hipMalloc");
    }
    if (bytes >= kPoolMin && ctx->pool_cap) {
        std::lock_guard<std::mutex> g(ctx->pool_mu);
        if (!grow(ctx->live_blocks, ctx->cap_live, ctx->n_live + 1)) {
            (void)hipFree(p);
            if (ev) (void)hipEventDestroy(ev);
            return fz_set_error(FZ_E_HIP, "out of host memory");
        }
        ctx->live_blocks[ctx->n_live++] = {p, bytes, ev};
    } else if (ev) {
        (void)hipEventDestroy(ev);
    }
    *d_out = p;
    return FZ_OK;
}

int fz_free(fz_ctx *ctx, void *d_ptr) {
    FZ_REQUIRE(ctx, "ctx is NULL");
    FZ_DEV(ctx);
    if (!d_ptr) return FZ_OK;
    hipEvent_t stale = nullptr;
    {
        std::lock_guard<std::mutex> g(ctx->pool_mu);
        for (int i = ctx->n_live - 1; i >= 0; --i) {
            if (ctx->live_blocks[i].p != d_ptr) continue;
            fz_ctx::FzBlock b = ctx->live_blocks[i];
            ctx->live_blocks[i] = ctx->live_blocks[--ctx->n_live];
            stale = b.ev;
            if (fz_capturing(ctx) || b.bytes > ctx->pool_cap || !grow(ctx->pool_blocks, ctx->cap_pool, ctx->n_pool + 1)) break;
            // room under the process-wide cap: this context's oldest blocks go first; if other contexts hold the rest, do not pool
            if (g_pool_bytes + b.bytes > ctx->pool_cap) {
                const size_t over = g_pool_bytes + b.bytes - ctx->pool_cap;
                pool_release_locked(ctx, ctx->pool_bytes > over ? ctx->pool_bytes - over : 0);
            }
            if (g_pool_bytes + b.bytes > ctx->pool_cap) break;
            if (!b.ev && hipEventCreateWithFlags(&b.ev, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); b.ev = nullptr; break; }
            if (hipEventRecord(b.ev, ctx->stream) != hipSuccess) { (void)hipGetLastError(); break; }
            ctx->pool_blocks[ctx->n_pool++] = b;
            ctx->pool_bytes += b.bytes;
            g_pool_bytes += b.bytes;
            return FZ_OK;
        }
    }
    if (stale) (void)hipEventDestroy(stale);
    FZ_HIP(hipFree(d_ptr), "hipFree");
    return FZ_OK;
}

int fz_memcpy_h2d(fz_ctx *ctx, void *d_dst, const void *h_src, size_t bytes) {
    FZ_REQUIRE(ctx && (bytes == 0 || (d_dst && h_src)), "NULL argument");
    FZ_DEV(ctx);
    if (bytes) FZ_HIP(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, ctx->stream), "memcpy h2d");
    return FZ_OK;
}

int fz_memcpy_d2h(fz_ctx *ctx, void *h_dst, const void *d_src, size_t bytes) {
    FZ_REQUIRE(ctx && (bytes == 0 || (h_dst && d_src)), "NULL argument");
    FZ_DEV(ctx);
    if (fz_capturing(ctx)) return fz_set_error(FZ_E_BADARG, "a synchronous device-to-host copy cannot be captured");
    if (bytes) FZ_HIP(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream), "memcpy d2h");
    FZ_HIP(hipStreamSynchronize(ctx->stream), "memcpy d2h sync");
    return FZ_OK;
}

}  // extern "C"
