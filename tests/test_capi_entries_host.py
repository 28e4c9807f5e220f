"""Every entry of csrc/fz_capi.hip (the int32-row entries) and csrc/fz_staged_capi.hip (the challenge pipeline's and the sampler's, which
take their small host inputs through the pinned staging slots) without a GPU: which refusal wins, which runtime calls it makes, where
in which area every pointer it hands a launcher lies.

fz_capi.hip, fz_staged_capi.hip, fz_context.hip and fz_diag.hip are compiled for the host with fz_host.cpp under AddressSanitizer and UBSan and linked,
as a stand-alone program, against the stub HIP runtime of tests/_hip_stub.py and recording stand-ins for every fz_launch_*.  A
stand-in records the counts and every pointer it was handed: a pointer into a growable area of the context, a staging slot or
the sampler's table as that area's name plus the byte offset, a caller's pointer as its argument's name plus the offset.  The
runtime calls the entry made are recorded the same way (function, size, the ends of a copy).  One line per call: the return
code, the error text, the launcher records, the runtime calls.

What is walked: on contexts of degree 256 and 64 (the fused paths), 128 (the generic paths: where the scratch layouts are used),
12 with root 0 (ring-only) and 16 with a modulus above 2^31 (the negation refusal), every entry's good call at batch 3, l = 2,
groups 2, N = 3, its empty call with NULL pointers and, where it reads knob_unfused, the good call with the knob set; on degree
256 its LADDER besides -- each single fault in the order the entry checks them and each adjacent pair (the pair pins the order); on
degree 128 and the ring-only context the single faults (the pair of a fault with what the context itself is refused for), with
the wide modulus the ladders of the pointwise entries.  Every
area-using entry runs small, large, small on a fresh context of degree 128 and one of 256 (the log shows which call allocates,
and how much).  The challenge pipeline runs in both forms, from digests and from messages, with and without the digests
returned and the transform, at N = 0, 1, 5 and 65536 + 3 (two chunks: that scratch is backed by one byte and no copy touches
memory), three calls in a row (the two slots in turn, the wait on reuse), a long call (a slot grows), and its refusals; the
sampler in its two forms (N = 4096, 4097) with its refusals, the table uploaded on first use only.

tests/golden/capi_entries.txt is that output for the sources BEFORE the entries' rules and scratch layouts were written once
(docs/HISTORY.md section AA), all of them still in fz_capi.hip: the refactored units must reproduce it line for line."""
import os
import re
import subprocess

import pytest

from _hip_stub import CSRC, STUB, build_driver

UNITS = ("fz_capi", "fz_staged_capi", "fz_context", "fz_diag")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "capi_entries.txt")

DRIVER_BODY = r'''
// ---- names: a pointer as the area (slot, table, argument) it lies in plus the byte offset ----
constexpr size_t SLOT = (size_t)1 << 19;
alignas(256) static char g_buf[8][SLOT];                 // the call's arguments, in the entry's order: real memory (the host-pointer entries copy)
static fz_ctx *g_ctx = nullptr;
static std::vector<std::string> g_names;
struct Range { std::string name; const char *p; size_t bytes; };
static std::vector<Range> g_extra;                       // further ranges of the caller's (offset tables, far dummies)
static const char *AREA[FZ_A_COUNT] = {"scratch", "scratch2", "verdict", "vpart", "vstate", "aggacc", "chal_tab", "stamp"};
constexpr size_t FAKE = (size_t)1 << 28;                 // areas above this are backed by one byte: their range is looked at last
static std::string at(const std::string &name, const char *p, const char *base) { return name + "+" + std::to_string((size_t)(p - base)); }
static std::string nm(const void *pv) {
    if (!pv) return "0";
    const char *p = (const char *)pv;
    for (size_t k = 0; k < 8; ++k)
        if (p >= g_buf[k] && p < g_buf[k] + SLOT) return at(k < g_names.size() ? g_names[k] : "buf" + std::to_string(k), p, g_buf[k]);
    for (const Range &r : g_extra) if (p >= r.p && p < r.p + r.bytes) return at(r.name, p, r.p);
    if (!g_ctx) return "?";
    for (int k = 0; k < 2; ++k) {
        const fz_ctx::FzStage &st = g_ctx->chal_stage[k];
        if (st.h && p >= (const char *)st.h && p < (const char *)st.h + st.bytes) return at("stage" + std::to_string(k), p, (const char *)st.h);
        if (st.ev && pv == (const void *)st.ev) return "stage" + std::to_string(k) + ".ev";
    }
    if (g_ctx->d_mt_init && p >= (const char *)g_ctx->d_mt_init && p < (const char *)g_ctx->d_mt_init + 624 * 4) return at("mt_init", p, (const char *)g_ctx->d_mt_init);
    for (int big = 0; big < 2; ++big)
        for (int k = 0; k < FZ_A_COUNT; ++k) {
            const FzArea &a = g_ctx->area[k];
            if (a.p && (a.bytes > FAKE) == (big == 1) && p >= (const char *)a.p && p < (const char *)a.p + a.bytes) return at(AREA[k], p, (const char *)a.p);
        }
    return "?";
}
#define S(p) nm(p).c_str()
#define LL(x) (long long)(x)

// ---- recording stand-ins for every launcher the unit reaches ----
static std::vector<std::string> g_recs;
static int g_launch_rc = FZ_OK;                          // control: what the challenge-wave and sampler stand-ins return
static bool g_wave_ok = true, g_mt_fail = false;         // controls: fz_challenge_wave_ok; the sampler's kernels raise their flag
static int recd(const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_recs.push_back(buf);
    return FZ_OK;
}
int fz_launch_ntt(fz_ctx *, const int32_t *in, int32_t *out, size_t batch, bool inv) { return recd("ntt(in=%s out=%s batch=%zu inverse=%d)", S(in), S(out), batch, (int)inv); }
int fz_launch_ntt_multi(fz_ctx *, FzMultiJobs &J) {
    std::string s = "ntt_multi(n=" + std::to_string(J.n);
    for (int j = 0; j < J.n; ++j) s += " [in=" + nm(J.in[j]) + " out=" + nm(J.out[j]) + " rows=" + std::to_string(J.rows[j]) + "]";
    return recd("%s)", s.c_str());
}
int fz_launch_polymul_fused(fz_ctx *, const int32_t *f, const int32_t *g, int32_t *out, size_t batch) { return recd("polymul_fused(f=%s g=%s out=%s batch=%zu)", S(f), S(g), S(out), batch); }
bool fz_polymul16_ok(const fz_ctx *, const int32_t *, const int32_t *, const int32_t *, size_t) { return false; }
int fz_launch_keygen_fused(fz_ctx *, const int32_t *A, const int32_t *coef, int32_t *sk, int32_t *vk, size_t segs, int l, bool bc) {
    return recd("keygen_fused(A=%s coef=%s sk_hat=%s vk=%s segments=%zu l=%d broadcast=%d)", S(A), S(coef), S(sk), S(vk), segs, l, (int)bc);
}
int fz_launch_verify_fused_i64(fz_ctx *, const int32_t *A, const int64_t *sig, size_t ss, const int64_t *t, size_t ts, size_t groups, int l, int64_t beta, int64_t omega, int *v) {
    return recd("verify_fused_i64(A=%s sig=%s sig_stride=%zu target=%s target_stride=%zu groups=%zu l=%d beta=%lld omega=%lld verdict=%s)", S(A), S(sig), ss, S(t), ts, groups, l, LL(beta), LL(omega), S(v));
}
int fz_launch_verify_fused(fz_ctx *, const int32_t *A, const int32_t *sig, const int32_t *t, size_t groups, int l, int64_t beta, int64_t omega, int *v) {
    return recd("verify_fused(A=%s sig=%s target=%s groups=%zu l=%d beta=%lld omega=%lld verdict=%s)", S(A), S(sig), S(t), groups, l, LL(beta), LL(omega), S(v));
}
int fz_launch_verify_signatures(fz_ctx *, const int32_t *A, const int32_t *sig, const int32_t *vk, const int32_t *c, size_t N, int l, int64_t beta, int64_t omega, int *v) {
    return recd("verify_signatures(A=%s sig=%s vk=%s c=%s N=%zu l=%d beta=%lld omega=%lld verdict=%s)", S(A), S(sig), S(vk), S(c), N, l, LL(beta), LL(omega), S(v));
}
int fz_launch_challenge(fz_ctx *, const fz_scheme_params *, const int32_t *vk, const uint8_t *pre, const uint32_t *dec, size_t N, uint8_t *text, size_t text_stride, int *nb,
                        uint32_t *xof, size_t xstride, int out_blocks, const uint32_t *tab, int32_t *coefs) {
    return recd("challenge(vk=%s pre=%s dec=%s N=%zu text=%s text_stride=%zu nblocks=%s xof=%s xstride=%zu out_blocks=%d tab=%s coefs=%s)", S(vk), S(pre), S(dec), N, S(text),
                text_stride, S(nb), S(xof), xstride, out_blocks, S(tab), S(coefs));
}
int fz_launch_challenge_wave(fz_ctx *, const fz_scheme_params *, const int32_t *vk, const uint8_t *pre, const uint8_t *msgs, const unsigned long long *off, uint8_t *pre_out,
                             size_t N, size_t text_stride, int out_blocks, const uint32_t *tab, int32_t *coefs) {
    recd("challenge_wave(vk=%s pre=%s msgs=%s off=%s pre_out=%s N=%zu text_stride=%zu out_blocks=%d tab=%s coefs=%s)", S(vk), S(pre), S(msgs), S(off), S(pre_out), N, text_stride,
         out_blocks, S(tab), S(coefs));
    return g_launch_rc == FZ_OK ? FZ_OK : fz_set_error(g_launch_rc, "the stand-in's launch error");
}
int fz_launch_prehash(fz_ctx *, const fz_scheme_params *, const uint8_t *msgs, const unsigned long long *off, size_t N, uint8_t *pre, uint32_t *dec) {
    return recd("prehash(msgs=%s off=%s N=%zu pre=%s dec=%s)", S(msgs), S(off), N, S(pre), S(dec));
}
void fz_mt_init_table(uint32_t *tab) { memset(tab, 0, 624 * 4); }
int fz_launch_mt_sample(fz_ctx *, const unsigned long long *seeds, size_t n, int degree, uint32_t bound, int kbits, const uint32_t *init, int32_t *out, int *fail, uint32_t *state) {
    recd("mt_sample(seeds=%s nkeys=%zu degree=%d bound=%u kbits=%d init=%s out=%s fail=%s state=%s)", S(seeds), n, degree, bound, kbits, S(init), S(out), S(fail), S(state));
    if (g_mt_fail) *fail = 1;
    return g_launch_rc == FZ_OK ? FZ_OK : fz_set_error(g_launch_rc, "the stand-in's launch error");
}
bool fz_challenge_wave_ok(const fz_scheme_params *) { return g_wave_ok; }
void fz_challenge_weight_table(int, int, uint32_t *) {}
int fz_launch_fill_synthetic(fz_ctx *, int32_t *out, size_t count, unsigned long long seed) { return recd("fill_synthetic(out=%s count=%zu seed=%llu)", S(out), count, seed); }
int fz_launch_bcast_rows(fz_ctx *, const int32_t *in, int32_t *out, size_t segs, int l) { return recd("bcast_rows(in=%s out=%s segments=%zu l=%d)", S(in), S(out), segs, l); }
int fz_launch_pw(fz_ctx *, int op, const int32_t *a, const int32_t *b, int32_t *out, size_t count) { return recd("pw(op=%d a=%s b=%s out=%s count=%zu)", op, S(a), S(b), S(out), count); }
int fz_launch_pw_bcast(fz_ctx *, const int32_t *a, const int32_t *s, int32_t *out, size_t rows) { return recd("pw_bcast(a=%s s=%s out=%s rows=%zu)", S(a), S(s), S(out), rows); }
int fz_launch_matvec(fz_ctx *, const int32_t *A, const int32_t *Sx, int32_t *out, size_t batch, int l) { return recd("matvec(A=%s S=%s out=%s batch=%zu l=%d)", S(A), S(Sx), S(out), batch, l); }
int fz_launch_sign(fz_ctx *, const int32_t *sk, const int32_t *c, int32_t *sig, size_t batch, int l) { return recd("sign(sk_hat=%s c_hat=%s sig=%s batch=%zu l=%d)", S(sk), S(c), S(sig), batch, l); }
int fz_launch_aggregate(fz_ctx *, const int32_t *sig, const int32_t *alpha, int64_t *out64, size_t ps, int32_t *out32, size_t groups, size_t N, int l, const int32_t *vkL,
                        const int32_t *vkR, const int32_t *c, int64_t *t64, size_t ts, const size_t *off, const int32_t *sk, int32_t *sig_out) {
    return recd("aggregate(sig=%s alpha=%s out64=%s pstride=%zu out32=%s groups=%zu N=%zu l=%d vkL=%s vkR=%s c=%s tout64=%s tstride=%zu offsets=%s sk_hat=%s sig_out=%s)", S(sig), S(alpha),
                S(out64), ps, S(out32), groups, N, l, S(vkL), S(vkR), S(c), S(t64), ts, S(off), S(sk), S(sig_out));
}
int fz_launch_target_partial(fz_ctx *, const int32_t *vkL, const int32_t *vkR, const int32_t *c, const int32_t *alpha, int64_t *partial, size_t ps, size_t groups, size_t N) {
    return recd("target_partial(vkL=%s vkR=%s c=%s alpha=%s partial=%s pstride=%zu groups=%zu N=%zu)", S(vkL), S(vkR), S(c), S(alpha), S(partial), ps, groups, N);
}
int fz_launch_reduce_i64(fz_ctx *, const int64_t *in, int32_t *out, size_t count) { return recd("reduce_i64(in=%s out=%s count=%zu)", S(in), S(out), count); }
int fz_launch_norm_weight(fz_ctx *, const int32_t *coef, size_t batch, int64_t *mx, int32_t *wt) { return recd("norm_weight(coef=%s batch=%zu max_abs=%s weight=%s)", S(coef), batch, S(mx), S(wt)); }
int fz_launch_verdict(fz_ctx *, const int32_t *t, const int32_t *obs, const int64_t *mx, const int32_t *wt, size_t groups, int l, int64_t beta, int64_t omega, int *v) {
    return recd("verdict(target=%s observed=%s max_abs=%s weight=%s groups=%zu l=%d beta=%lld omega=%lld verdict=%s)", S(t), S(obs), S(mx), S(wt), groups, l, LL(beta), LL(omega), S(v));
}

// ---- one line per call ----
static void line(const std::string &ctxname, const std::string &entry, const std::string &what, size_t mark, size_t recs, int rc) {
    printf("%s %s [%s] -> rc=%d", ctxname.c_str(), entry.c_str(), what.c_str(), rc);
    if (rc != FZ_OK) printf(" \"%s\"", fz_last_error());
    printf(" |");
    for (size_t k = recs; k < g_recs.size(); ++k) printf(" %s", g_recs[k].c_str());
    printf(" |");
    for (const Call &c : stub_log(mark)) {
        if (c.kind >= 0) printf(" %s(dst=%s src=%s n=%zu)", c.fn.c_str(), S(c.p), S(c.src), c.n);
        else if (c.fn == "hipMalloc" || c.fn == "hipHostMalloc") printf(" %s(%zu)=%s", c.fn.c_str(), c.n, S(c.p));
        else if (c.fn.compare(0, 8, "hipEvent") == 0) printf(" %s(%s)", c.fn.c_str(), S(c.p));
        else if (c.fn == "hipMemsetAsync") printf(" %s(dst=%s n=%zu)", c.fn.c_str(), S(c.p), c.n);
        else if (c.n) printf(" %s(%zu)", c.fn.c_str(), c.n);
        else printf(" %s", c.fn.c_str());
    }
    printf("\n");
}

// ---- a call's arguments, the faults that spoil them, the entries ----
static const uint32_t Q = 2147465729u;
static int g_d = 0;
static std::string g_cname;
struct Args {
    fz_ctx *ctx;
    char *p[8];
    size_t n, groups, ps, ts;
    int l, op;
    int64_t beta, omega;
    std::vector<size_t> off;                             // the ragged entries' offsets (empty: NULL)
};
struct Fault { std::string name; std::function<void(Args &)> spoil; };
enum { UNFUSED = 1, AREAS = 2, EMPTY_GROUPS = 4 };
struct Entry { const char *name; std::vector<std::string> names; std::function<int(Args &)> call; std::vector<Fault> ladder; int flags; std::vector<Fault> variants; };

static Fault F(const std::string &name, std::function<void(Args &)> f) { return {name, f}; }
static Fault null_at(int k) { return F("null" + std::to_string(k), [k](Args &a) { a.p[k] = nullptr; }); }
static Fault mis_at(int k, int by) { return F("mis" + std::to_string(k), [k, by](Args &a) { a.p[k] += by; }); }
static std::vector<Fault> nulls(std::initializer_list<int> ks) { std::vector<Fault> v; for (int k : ks) v.push_back(null_at(k)); return v; }
static std::vector<Fault> operator+(std::vector<Fault> a, const std::vector<Fault> &b) { a.insert(a.end(), b.begin(), b.end()); return a; }
static const Fault f_ctx = F("ctx", [](Args &a) { a.ctx = nullptr; }), f_l0 = F("l0", [](Args &a) { a.l = 0; }), f_n0 = F("n0", [](Args &a) { a.n = 0; }),
                   f_nbig = F("n_big", [](Args &a) { a.n = (size_t)1 << 21; }), f_g0 = F("groups0", [](Args &a) { a.groups = 0; }),
                   f_gbig = F("groups_big", [](Args &a) { a.groups = 65536; }), f_ps = F("ps_short", [](Args &a) { a.ps = 1; }), f_ts = F("ts_short", [](Args &a) { a.ts = 1; }),
                   f_offnull = F("offsets_null", [](Args &a) { a.off.clear(); }), f_dec = F("decreasing", [](Args &a) { a.groups = 2; a.off = {0, 2, 1}; }),
                   f_grpbig = F("group_big", [](Args &a) { a.groups = 2; a.off = {0, 1, 1 + ((size_t)1 << 21)}; }),
                   f_total = F("total_big", [](Args &a) { a.groups = 2049; a.off.assign(2050, 0); for (size_t g = 0; g <= 2049; ++g) a.off[g] = g * (0xfffffffeull / 2049); a.off[2049] = 0xffffffffull; });
using V = std::vector<Fault>;
#define I32(k) (const int32_t *)a.p[k]
#define O32(k) (int32_t *)a.p[k]
#define O64(k) (int64_t *)a.p[k]
#define OFF(a) ((a).off.empty() ? nullptr : (a).off.data())

static std::vector<Entry> entries() {
    std::vector<Entry> E;
    auto add = [&](const char *name, std::vector<std::string> names, std::function<int(Args &)> call, V ladder, int flags = 0, V variants = {}) {
        E.push_back({name, names, call, ladder, flags, variants});
    };
    add("fz_ntt_forward", {"d_in", "d_out"}, [](Args &a) { return fz_ntt_forward(a.ctx, I32(0), O32(1), a.n); }, V{f_ctx} + nulls({0, 1}));
    add("fz_ntt_inverse", {"d_in", "d_out"}, [](Args &a) { return fz_ntt_inverse(a.ctx, I32(0), O32(1), a.n); }, V{f_ctx} + nulls({0, 1}));
    add("fz_ntt_forward_host", {"h_data"}, [](Args &a) { return fz_ntt_forward_host(a.ctx, O32(0), a.n); }, V{f_ctx} + nulls({0}), AREAS);
    add("fz_ntt_inverse_host", {"h_data"}, [](Args &a) { return fz_ntt_inverse_host(a.ctx, O32(0), a.n); }, V{f_ctx} + nulls({0}), AREAS);
    add("fz_pw_mul", {"a", "b", "out"}, [](Args &a) { return fz_pw_mul(a.ctx, I32(0), I32(1), O32(2), a.n); }, V{f_ctx} + nulls({0, 1, 2}));
    add("fz_pw_add", {"a", "b", "out"}, [](Args &a) { return fz_pw_add(a.ctx, I32(0), I32(1), O32(2), a.n); }, V{f_ctx} + nulls({0, 1, 2}));
    add("fz_pw_sub", {"a", "b", "out"}, [](Args &a) { return fz_pw_sub(a.ctx, I32(0), I32(1), O32(2), a.n); }, V{f_ctx} + nulls({0, 1, 2}));
    add("fz_pw_neg", {"a", "out"}, [](Args &a) { return fz_pw_neg(a.ctx, I32(0), O32(1), a.n); }, V{f_ctx} + nulls({0, 1}));
    add("fz_pw_mulacc", {"acc", "a", "b"}, [](Args &a) { return fz_pw_mulacc(a.ctx, O32(0), I32(1), I32(2), a.n); }, V{f_ctx} + nulls({0, 1, 2}));
    add("fz_pw_mul_bcast", {"a", "s", "out"}, [](Args &a) { return fz_pw_mul_bcast(a.ctx, I32(0), I32(1), O32(2), a.n); }, V{f_ctx} + nulls({0, 1, 2}));
    add("fz_pw_binary_host", {"h_a", "h_b", "h_out"}, [](Args &a) { return fz_pw_binary_host(a.ctx, a.op, I32(0), I32(1), O32(2), a.n); },
        V{F("op_low", [](Args &a) { a.op = -1; }), F("op_high", [](Args &a) { a.op = 5; }), f_ctx} + nulls({0, 1, 2}), AREAS,      // (one check: its text names the op)
        V{F("add", [](Args &a) { a.op = 1; }), F("sub", [](Args &a) { a.op = 2; }), F("neg", [](Args &a) { a.op = 3; }), F("neg, no b", [](Args &a) { a.op = 3; a.p[1] = nullptr; }),
          F("neg, empty", [](Args &a) { a.op = 3; a.n = 0; }), F("neg, no a", [](Args &a) { a.op = 3; a.p[0] = nullptr; })});
    add("fz_fill_synthetic", {"d_out"}, [](Args &a) { return fz_fill_synthetic(a.ctx, O32(0), a.n, 7); }, V{f_ctx} + nulls({0}));
    add("fz_poly_mul", {"d_f", "d_g", "d_out"}, [](Args &a) { return fz_poly_mul(a.ctx, I32(0), I32(1), O32(2), a.n); }, V{f_ctx} + nulls({0, 1, 2}) + V{mis_at(0, 2), mis_at(2, 2)},
        UNFUSED | AREAS);
    add("fz_poly_mul_host", {"h_f", "h_g", "h_out"}, [](Args &a) { return fz_poly_mul_host(a.ctx, I32(0), I32(1), O32(2), a.n); }, V{f_ctx} + nulls({0, 1, 2}), UNFUSED | AREAS);
    add("fz_matvec", {"A", "S", "out"}, [](Args &a) { return fz_matvec(a.ctx, I32(0), I32(1), O32(2), a.n, a.l); }, V{f_ctx, f_l0} + nulls({0, 1, 2}));
    add("fz_matvec_host", {"h_A", "h_S", "h_out"}, [](Args &a) { return fz_matvec_host(a.ctx, I32(0), I32(1), O32(2), a.n, a.l); }, V{f_ctx, f_l0} + nulls({0, 1, 2}), AREAS);
    const V keygen_variants{mis_at(0, 4), mis_at(2, 8), F("batch_2_31", [](Args &a) { a.n = 0x40000000; })};
    add("fz_keygen_core", {"d_A", "d_coef", "d_sk_hat", "d_vk"}, [](Args &a) { return fz_keygen_core(a.ctx, I32(0), I32(1), O32(2), O32(3), a.n, a.l); },
        V{f_ctx, f_l0} + nulls({0, 1, 2, 3}), UNFUSED, keygen_variants);
    add("fz_keygen_core_bcast", {"d_A", "d_coef", "d_sk_hat", "d_vk"}, [](Args &a) { return fz_keygen_core_bcast(a.ctx, I32(0), I32(1), O32(2), O32(3), a.n, a.l); },
        V{f_ctx, f_l0} + nulls({0, 1, 2, 3}), UNFUSED, keygen_variants);
    add("fz_sign_core", {"d_sk_hat", "d_c_hat", "d_sig"}, [](Args &a) { return fz_sign_core(a.ctx, I32(0), I32(1), O32(2), a.n, a.l); }, V{f_ctx, f_l0} + nulls({0, 1, 2}));
    add("fz_aggregate_partial_batch", {"d_sig", "d_alpha_hat", "d_partial"}, [](Args &a) { return fz_aggregate_partial_batch(a.ctx, I32(0), I32(1), O64(2), a.ps, a.groups, a.n, a.l); },
        V{f_ctx, f_l0} + nulls({2, 0, 1}) + V{f_nbig, f_gbig, f_ps}, 0, V{F("one group, no stride", [](Args &a) { a.groups = 1; a.ps = 0; }), F("no groups, no inputs", [](Args &a) { a.groups = 0; a.p[0] = a.p[1] = nullptr; })});
    add("fz_aggregate_target_partial_batch", {"d_sig", "d_alpha_hat", "d_vkL", "d_vkR", "d_c_hat", "d_partial", "d_target_partial"},
        [](Args &a) { return fz_aggregate_target_partial_batch(a.ctx, I32(0), I32(1), I32(2), I32(3), I32(4), O64(5), a.ps, O64(6), a.ts, a.groups, a.n, a.l); },
        V{f_ctx, f_l0} + nulls({5, 6, 0, 1, 2, 3, 4}) + V{f_nbig, f_gbig, f_ps, f_ts, mis_at(2, 4), mis_at(0, 8)}, 0, V{F("one group, no strides", [](Args &a) { a.groups = 1; a.ps = a.ts = 0; })});
    add("fz_sign_aggregate_target_partial_batch", {"d_sk_hat", "d_c_hat", "d_alpha_hat", "d_vkL", "d_vkR", "d_sig", "d_partial", "d_target_partial"},
        [](Args &a) { return fz_sign_aggregate_target_partial_batch(a.ctx, I32(0), I32(1), I32(2), I32(3), I32(4), O32(5), O64(6), a.ps, O64(7), a.ts, a.groups, a.n, a.l); },
        V{f_ctx, f_l0, null_at(6), F("vk_half", [](Args &a) { a.p[3] = nullptr; }), F("no_target", [](Args &a) { a.p[7] = nullptr; })} + nulls({0, 1, 2, 5}) + V{f_nbig, f_gbig, f_ps, f_ts}, UNFUSED,
        V{F("no keys", [](Args &a) { a.p[3] = a.p[4] = a.p[7] = nullptr; }), F("no keys, short target stride", [](Args &a) { a.p[3] = a.p[4] = a.p[7] = nullptr; a.ts = 1; }),
          mis_at(0, 4), F("no signers", [](Args &a) { a.n = 0; a.p[0] = nullptr; })});
    add("fz_aggregate_partial", {"d_sig", "d_alpha_hat", "d_partial"}, [](Args &a) { return fz_aggregate_partial(a.ctx, I32(0), I32(1), O64(2), a.n, a.l); },
        V{f_ctx, f_l0} + nulls({2, 0, 1}) + V{f_nbig});
    add("fz_aggregate_core_ragged", {"d_sig", "d_alpha_hat", "d_out"}, [](Args &a) { return fz_aggregate_core_ragged(a.ctx, I32(0), I32(1), OFF(a), a.groups, a.l, O32(2)); },
        V{f_ctx, f_l0, f_offnull} + nulls({0, 1, 2}) + V{f_dec, f_grpbig, f_total}, EMPTY_GROUPS,
        V{F("65 groups", [](Args &a) { a.groups = 65; a.off.resize(66); for (size_t g = 0; g <= 65; ++g) a.off[g] = 2 * g; })});
    add("fz_aggregate_target_partial_ragged", {"d_sig", "d_alpha_hat", "d_vkL", "d_vkR", "d_c_hat", "d_partial", "d_target_partial"},
        [](Args &a) { return fz_aggregate_target_partial_ragged(a.ctx, I32(0), I32(1), I32(2), I32(3), I32(4), OFF(a), a.groups, a.l, O64(5), a.ps, O64(6), a.ts); },
        V{f_ctx, f_l0, f_offnull} + nulls({6, 1, 2, 3, 4}) + V{F("sig_alone", [](Args &a) { a.p[5] = nullptr; }), f_ps, f_ts, f_dec, f_grpbig, f_total}, EMPTY_GROUPS,
        V{F("targets only", [](Args &a) { a.p[0] = a.p[5] = nullptr; a.ps = 0; }), F("one group, no strides", [](Args &a) { a.groups = 1; a.off = {0, 3}; a.ps = a.ts = 0; })});
    add("fz_reduce_i64", {"d_in", "d_out"}, [](Args &a) { return fz_reduce_i64(a.ctx, (const int64_t *)a.p[0], O32(1), a.n); }, V{f_ctx} + nulls({0, 1}));
    add("fz_aggregate_core", {"d_sig", "d_alpha_hat", "d_out"}, [](Args &a) { return fz_aggregate_core(a.ctx, I32(0), I32(1), O32(2), a.n, a.l); }, V{f_ctx, f_l0, f_n0} + nulls({0, 1, 2}) + V{f_nbig});
    add("fz_target_partial_batch", {"d_vkL", "d_vkR", "d_c_hat", "d_alpha_hat", "d_partial"},
        [](Args &a) { return fz_target_partial_batch(a.ctx, I32(0), I32(1), I32(2), I32(3), O64(4), a.ts, a.groups, a.n); }, V{f_ctx} + nulls({4, 0, 1, 2, 3}) + V{f_nbig, f_gbig, f_ts}, 0,
        V{F("one group, no stride", [](Args &a) { a.groups = 1; a.ts = 0; })});
    add("fz_target_partial", {"d_vkL", "d_vkR", "d_c_hat", "d_alpha_hat", "d_partial"}, [](Args &a) { return fz_target_partial(a.ctx, I32(0), I32(1), I32(2), I32(3), O64(4), a.n); },
        V{f_ctx} + nulls({4, 0, 1, 2, 3}) + V{f_nbig});
    add("fz_norm_weight", {"d_coef", "d_max_abs", "d_weight"}, [](Args &a) { return fz_norm_weight(a.ctx, I32(0), a.n, O64(1), O32(2)); }, V{f_ctx} + nulls({0, 1, 2}));
    add("fz_norm_weight_host", {"h_coef", "h_max_abs", "h_weight"}, [](Args &a) { return fz_norm_weight_host(a.ctx, I32(0), a.n, O64(1), O32(2)); }, V{f_ctx} + nulls({0, 1, 2}), AREAS);
    add("fz_verify_with_target_batch", {"d_A", "d_sig", "d_target", "h_verdicts"},
        [](Args &a) { return fz_verify_with_target_batch(a.ctx, I32(0), I32(1), I32(2), a.groups, a.l, a.beta, a.omega, (int *)a.p[3]); }, V{f_ctx, f_l0, f_g0, f_gbig} + nulls({0, 1, 2, 3}), UNFUSED | AREAS);
    add("fz_verify_with_target_batch_async", {"d_A", "d_sig", "d_target", "d_verdicts"},
        [](Args &a) { return fz_verify_with_target_batch_async(a.ctx, I32(0), I32(1), I32(2), a.groups, a.l, a.beta, a.omega, (int *)a.p[3]); }, V{f_ctx, f_l0, f_g0, f_gbig} + nulls({0, 1, 2, 3}));
    add("fz_verify_signatures_async", {"d_A", "d_sig", "d_vk", "d_c_hat", "d_verdicts"},
        [](Args &a) { return fz_verify_signatures_async(a.ctx, I32(0), I32(1), I32(2), I32(3), a.n, a.l, a.beta, a.omega, (int *)a.p[4]); },
        V{f_ctx, f_l0, F("beta_neg", [](Args &a) { a.beta = -1; }), F("omega_neg", [](Args &a) { a.omega = -1; })} + nulls({0, 1, 2, 3, 4}) + V{mis_at(0, 4), mis_at(1, 8)}, 0,
        V{F("empty, bad l", [](Args &a) { a.n = 0; a.l = 0; })});
    add("fz_verify_partials_batch_async", {"d_A", "d_partial", "d_target_partial", "d_verdicts"},
        [](Args &a) { return fz_verify_partials_batch_async(a.ctx, I32(0), (const int64_t *)a.p[1], a.ps, (const int64_t *)a.p[2], a.ts, a.groups, a.l, a.beta, a.omega, (int *)a.p[3]); },
        V{f_ctx, f_l0, f_g0, f_gbig} + nulls({0, 1, 2, 3}) + V{f_ps, f_ts, mis_at(1, 8), mis_at(2, 8), mis_at(0, 4), F("ps_odd", [](Args &a) { a.ps += 1; })}, 0,
        V{F("one group, no strides", [](Args &a) { a.groups = 1; a.ps = a.ts = 0; })});
    add("fz_verify_with_target", {"d_A", "d_sig", "d_target", "h_verdict"}, [](Args &a) { return fz_verify_with_target(a.ctx, I32(0), I32(1), I32(2), a.l, a.beta, a.omega, (int *)a.p[3]); },
        V{f_ctx, f_l0} + nulls({0, 1, 2, 3}), UNFUSED | AREAS);
    add("fz_verify_core", {"d_A", "d_sig", "d_vkL", "d_vkR", "d_c_hat", "d_alpha_hat", "h_verdict"},
        [](Args &a) { return fz_verify_core(a.ctx, I32(0), I32(1), I32(2), I32(3), I32(4), I32(5), a.n, a.l, a.beta, a.omega, (int *)a.p[6]); },
        V{f_ctx, f_l0, f_n0} + nulls({0, 1, 2, 3, 4, 5, 6}) + V{f_nbig}, UNFUSED | AREAS);
    // two jobs: rows n forward, 5 rows inverse (groups: how many of them the call is handed)
    add("fz_ntt_multi", {"in0", "out0", "in1", "out1"},
        [](Args &a) {
            fz_ntt_job jobs[3] = {{I32(0), O32(1), a.n, 0}, {I32(2), O32(3), 5, 1}, {I32(0) ? I32(0) + 64 : nullptr, O32(1) ? O32(1) + 64 : nullptr, (size_t)a.l - 2, 0}};
            return fz_ntt_multi(a.ctx, a.op == 0 ? jobs : nullptr, a.groups);
        },
        V{f_ctx, F("jobs_null", [](Args &a) { a.op = 1; }), null_at(0), F("rows_big", [](Args &a) { a.n = (size_t)1 << 31; }), mis_at(2, 4)}, EMPTY_GROUPS,
        V{F("three jobs, one empty", [](Args &a) { a.groups = 3; }), F("three jobs", [](Args &a) { a.groups = 3; a.l = 9; }), F("empty job, no buffers", [](Args &a) { a.n = 0; a.p[0] = a.p[1] = nullptr; a.groups = 2; })});
    return E;
}

// ---- the walk ----
static Args good(fz_ctx *c, const Entry &e) {
    Args a{c, {}, 3, 2, (size_t)2 * g_d, (size_t)g_d, 2, 0, 5, 7, {0, 1, 3}};
    for (size_t k = 0; k < 8; ++k) a.p[k] = k < e.names.size() ? g_buf[k] : nullptr;
    return a;
}
static int run(const Entry &e, const std::string &what, Args a) {
    g_names = e.names;
    g_extra.clear();
    if (!a.off.empty()) g_extra.push_back({"h_offsets", (const char *)a.off.data(), a.off.size() * sizeof(size_t)});
    const size_t mark = stub_mark(), recs = g_recs.size();
    const int rc = e.call(a);
    line(g_cname, e.name, what, mark, recs, rc);
    return rc;
}
static void walk(fz_ctx *c, const Entry &e, bool singles, bool pairs) {
    const V &L = e.ladder;
    run(e, "good", good(c, e));
    if (e.flags & UNFUSED) { c->knob_unfused = 1; run(e, "good, unfused", good(c, e)); c->knob_unfused = 0; }
    for (const Fault &f : e.variants) { Args a = good(c, e); f.spoil(a); run(e, "good, " + f.name, a); }
    for (size_t i = 0; singles && i < L.size(); ++i) { Args a = good(c, e); L[i].spoil(a); run(e, L[i].name, a); }
    for (size_t i = 0; pairs && i + 1 < L.size(); ++i) {       // the later fault first: where both touch one argument, the earlier one's value stands
        Args a = good(c, e);
        L[i + 1].spoil(a);
        L[i].spoil(a);
        run(e, L[i].name + "+" + L[i + 1].name, a);
    }
    Args a = good(c, e);
    a.n = 0;
    if (e.flags & EMPTY_GROUPS) a.groups = 0;
    for (int k = 0; k < 8; ++k) a.p[k] = nullptr;
    run(e, "empty", a);
}
static fz_ctx *make_ctx(const std::string &name) {
    const uint64_t r256 = 3337519u, i256 = 1978410468u;
    fz_ctx *c = nullptr;
    int rc;
    if (name == "d256") { g_d = 256; rc = fz_ctx_create(0, Q, 256, (uint32_t)r256, (uint32_t)i256, &c); }
    else if (name == "d64") { g_d = 64; rc = fz_ctx_create(0, Q, 64, 23584283u, 540632852u, &c); }
    else if (name == "d128") { g_d = 128; rc = fz_ctx_create(0, Q, 128, (uint32_t)(r256 * r256 % Q), (uint32_t)(i256 * i256 % Q), &c); }
    else if (name == "ring12") { g_d = 12; rc = fz_ctx_create(0, Q, 12, 0, 0, &c); }
    else { g_d = 16; rc = fz_ctx_create(0, 4294967291u, 16, 0, 0, &c); }        // "q32": 2^32 - 5
    if (rc != FZ_OK) { printf("FAIL context %s: %s\n", name.c_str(), fz_last_error()); exit(2); }
    g_ctx = c;
    g_cname = name;
    return c;
}
static void drop_ctx(fz_ctx *c) { g_ctx = nullptr; fz_ctx_destroy(c); }

// small, large, small on a fresh context: which call allocates, and how much
static void growth(const std::string &cname, const Entry &e) {
    fz_ctx *c = make_ctx(cname);
    for (int step = 0; step < 3; ++step) {
        Args a = good(c, e);
        if (step == 1) { a.n = 8; a.groups = 5; a.l = 4; a.ps = (size_t)4 * g_d; }
        run(e, step == 1 ? "grow: large" : step ? "grow: small again" : "grow: small", a);
    }
    if (std::string(e.name) == "fz_poly_mul_host" || std::string(e.name) == "fz_verify_core") {       // the other path on the same context, larger still
        c->knob_unfused = 1;
        Args a = good(c, e);
        a.n = 12; a.l = 5;
        run(e, "grow: larger, unfused", a);
    }
    drop_ctx(c);
}

// ---- the challenge pipeline ----
static fz_scheme_params params(int degree, int64_t modulus) {
    fz_scheme_params P;
    memset(&P, 0, sizeof(P));
    P.modulus = modulus; P.root = 3; P.inv_root = 5; P.degree = degree; P.root_order = 2 * degree; P.secpar = 128;
    P.omega_ch = degree; P.omega_ag = degree; P.beta_ch = 1; P.beta_ag = 1;
    P.bytes_for_one_coef_bdd_by_beta_ch = 17; P.bytes_for_poly_shuffle = 0;
    P.sign_pre_hash_dst[1] = 1; P.sign_hash_dst[1] = 2; P.agg_xof_dst[1] = 3;
    return P;
}
struct Chal {
    fz_ctx *ctx; fz_scheme_params P; bool have_P;
    const int32_t *vk; const uint8_t *pre; const char *msgs; std::vector<size_t> off; bool off_null; uint8_t *pre_out; size_t N; int32_t *out;
    int entry;                                           // 0 coefficients (digests), 1 hat (digests), 2 hat from messages
};
static Chal chal_good(fz_ctx *c, int entry, size_t N, size_t msg_len = 3) {
    Chal a{c, params(g_d, (int64_t)c->q), true, (const int32_t *)g_buf[0], (const uint8_t *)g_buf[1], g_buf[2], {}, false, (uint8_t *)g_buf[3], N, (int32_t *)g_buf[4], entry};
    a.off.resize(N + 1);
    for (size_t i = 0; i <= N; ++i) a.off[i] = 7 + i * msg_len;             // (the first message does not start the buffer)
    return a;
}
static int chal_run(const std::string &what, Chal a) {
    g_names = {"d_vk", "h_prehash", "h_msgs", "h_prehash_out", "d_out"};
    g_extra.clear();
    g_extra.push_back({"h_msg_off", (const char *)a.off.data(), a.off.size() * sizeof(size_t)});
    if ((const char *)a.vk == (const char *)((uintptr_t)1 << 44)) {
        g_extra.push_back({"d_vk", (const char *)a.vk, (size_t)1 << 40}); g_extra.push_back({"d_out", (const char *)a.out, (size_t)1 << 40});
        g_extra.push_back({"h_prehash", (const char *)a.pre, (size_t)1 << 40}); g_extra.push_back({"h_prehash_out", (const char *)a.pre_out, (size_t)1 << 40});
    }
    const size_t mark = stub_mark(), recs = g_recs.size();
    const fz_scheme_params *P = a.have_P ? &a.P : nullptr;
    const size_t *off = a.off_null ? nullptr : a.off.data();
    const int rc = a.entry == 0 ? fz_challenge_coefficients_dev(a.ctx, P, a.vk, a.pre, a.N, a.out)
                 : a.entry == 1 ? fz_challenge_hat_dev(a.ctx, P, a.vk, a.pre, a.N, a.out)
                                : fz_challenge_hat_msgs_dev(a.ctx, P, a.vk, a.msgs, off, a.N, a.out, a.pre_out);
    static const char *names[3] = {"fz_challenge_coefficients_dev", "fz_challenge_hat_dev", "fz_challenge_hat_msgs_dev"};
    line(g_cname, names[a.entry], what, mark, recs, rc);
    return rc;
}
static void challenge_walk() {
    for (const char *cname : {"d256", "d64", "d128"}) {
        fz_ctx *c = make_ctx(cname);
        for (int form = 0; form < 2; ++form) {                                 // the wave form, the chunked one
            c->knob_shake_full = form ? 1 : 0;
            const std::string f = form ? "chunked" : "wave";
            for (size_t N : {(size_t)0, (size_t)1, (size_t)5})
                for (int entry = 0; entry < 3; ++entry) {
                    chal_run(f + " N=" + std::to_string(N), chal_good(c, entry, N));
                    if (entry == 2 && N) { Chal a = chal_good(c, entry, N); a.pre_out = nullptr; chal_run(f + " N=" + std::to_string(N) + ", digests not returned", a); }
                }
        }
        c->knob_shake_full = 0;
        drop_ctx(c);
    }
    fz_ctx *c = make_ctx("d256");
    // the form decision: by the batch size, by the knob, by what the wave form takes
    chal_run("N=4608: wave", chal_good(c, 1, 4608));
    chal_run("N=4609: chunked", chal_good(c, 1, 4609));
    c->knob_shake_full = 3; chal_run("N=4609, knob 3: wave", chal_good(c, 1, 4609));
    g_wave_ok = false; chal_run("N=5, knob 3, parameters the wave form does not take: chunked", chal_good(c, 1, 5)); g_wave_ok = true;
    c->knob_shake_full = 2; chal_run("N=5, knob 2: chunked", chal_good(c, 1, 5));
    c->knob_shake_full = 0;
    drop_ctx(c);
    // slots: three calls take slot 0, 1, 0 (the third waits for the first's event); a long call grows its slot; a failed launch still marks the slot
    c = make_ctx("d256");
    for (int k = 0; k < 3; ++k) chal_run("slots: call " + std::to_string(k), chal_good(c, 2, 5));
    chal_run("slots: a long call", chal_good(c, 2, 5, 60001));
    chal_run("slots: a short call in the other slot", chal_good(c, 2, 5));
    chal_run("slots: a short call in the grown slot", chal_good(c, 2, 5));
    g_launch_rc = FZ_E_HIP; chal_run("slots: the launch fails", chal_good(c, 2, 5)); g_launch_rc = FZ_OK;
    chal_run("slots: the call after it", chal_good(c, 2, 5));
    chal_run("slots: and the next waits", chal_good(c, 2, 5));
    drop_ctx(c);
    // two chunks: the scratch is backed by one byte, no copy touches memory, the rows and the digests are far dummies
    c = make_ctx("d256");
    g_copy_nothing = true; g_fake_above = FAKE;                  // (to the end of the context: its scratch stays the one byte)
    for (int entry = 1; entry < 3; ++entry) {
        Chal a = chal_good(c, entry, 65536 + 3, 2);
        a.vk = (const int32_t *)((uintptr_t)1 << 44); a.out = (int32_t *)((uintptr_t)1 << 45);
        a.pre = (const uint8_t *)((uintptr_t)3 << 44); a.pre_out = (uint8_t *)((uintptr_t)5 << 44);
        chal_run("two chunks", a);
        chal_run("small after two chunks", chal_good(c, entry, 5));
    }
    drop_ctx(c);
    g_copy_nothing = false; g_fake_above = 0;
    // the refusals, in the order they are made; then each with the one after it
    c = make_ctx("d256");
    struct CF { std::string name; std::function<void(Chal &)> spoil; bool msgs_only = false; };
    const std::vector<CF> all = {
        {"entry: no digests / offsets", [](Chal &a) { a.pre = nullptr; a.off_null = true; }},
        {"ctx", [](Chal &a) { a.ctx = nullptr; }},
        {"params_null", [](Chal &a) { a.have_P = false; }},
        {"vk_null", [](Chal &a) { a.vk = nullptr; }},
        {"out_null", [](Chal &a) { a.out = nullptr; }},
        {"msgs_null", [](Chal &a) { a.msgs = nullptr; }, true},
        {"offsets_decrease", [](Chal &a) { a.off[2] = a.off[1] - 1; }, true},
        {"params_bad", [](Chal &a) { a.P.secpar = 0; }},
        {"params_foreign", [](Chal &a) { a.P.degree = 128; }},
        {"capture", [](Chal &a) { a.ctx->capturing = 1; }},
        {"not_ternary", [](Chal &a) { a.P.beta_ch = 2; }},
        {"omega", [](Chal &a) { a.P.omega_ch = a.P.degree + 1; }},
        {"misaligned", [](Chal &a) { a.vk += 1; }},
    };
    for (int entry = 1; entry < 3; ++entry) {
        std::vector<CF> L;
        for (const CF &f : all) if (entry == 2 || !f.msgs_only) L.push_back(f);
        for (size_t i = 0; i < L.size(); ++i) { Chal a = chal_good(c, entry, 5); L[i].spoil(a); chal_run(L[i].name, a); c->capturing = 0; }
        for (size_t i = 0; i + 1 < L.size(); ++i) { Chal a = chal_good(c, entry, 5); L[i + 1].spoil(a); L[i].spoil(a); chal_run(L[i].name + "+" + L[i + 1].name, a); c->capturing = 0; }
        Chal a = chal_good(c, entry, 0);
        a.vk = nullptr; a.pre = nullptr; a.msgs = nullptr; a.off_null = true; a.out = nullptr; a.pre_out = nullptr;
        chal_run("empty", a);
        a.P.beta_ch = 2; chal_run("empty, not_ternary", a);
    }
    { Chal a = chal_good(c, 2, 5); for (size_t i = 0; i <= 5; ++i) a.off[i] = 9; a.msgs = nullptr; chal_run("five empty messages, no bytes", a); }
    drop_ctx(c);
    c = make_ctx("ring12");
    { Chal a = chal_good(c, 0, 5); chal_run("degree 12", a); }
    drop_ctx(c);
    // a ring-only context whose degree the pipeline takes: the transform is refused, the coefficients are not
    { g_d = 16; g_cname = "ring16"; fz_ctx *r = nullptr; if (fz_ctx_create(0, Q, 16, 0, 0, &r) != FZ_OK) exit(2); g_ctx = r;
      chal_run("coefficients", chal_good(r, 0, 5)); chal_run("transform", chal_good(r, 1, 5)); chal_run("transform, empty", chal_good(r, 1, 0));
      // the table follows the parameters it was built for
      Chal a = chal_good(r, 0, 5); a.P.bytes_for_poly_shuffle = 3; chal_run("coefficients again", a); a.P.omega_ch = 3; chal_run("another weight", a);
      drop_ctx(r); }
}

// ---- the sampler ----
static void sampler_walk() {
    fz_ctx *c = make_ctx("d256");
    static uint64_t seeds[4097];
    for (size_t i = 0; i < 4097; ++i) seeds[i] = 1000 + i;
    g_names = {"d_out"};
    auto run = [&](const std::string &what, fz_ctx *ctx, const uint64_t *h_seeds, size_t N, int64_t modulus, int degree, int64_t norm, int64_t weight, int32_t *out) {
        g_extra.clear();
        const size_t mark = stub_mark(), recs = g_recs.size();
        const int rc = fz_sample_secret_polys_dev(ctx, h_seeds, N, modulus, degree, norm, weight, out);
        line(g_cname, "fz_sample_secret_polys_dev", what, mark, recs, rc);
    };
    int32_t *out = (int32_t *)g_buf[0];
    run("N=3: the table is uploaded", c, seeds, 3, Q, 256, 52, 256, out);
    run("N=3 again", c, seeds, 3, Q, 256, 52, 256, out);
    run("N=4096: two kernels", c, seeds, 4096, Q, 256, 52, 256, out);
    run("N=4097: one kernel", c, seeds, 4097, Q, 256, 52, 256, out);
    run("N=3 after them", c, seeds, 3, Q, 256, 52, 256, out);
    run("the largest bound", c, seeds, 3, (int64_t)1 << 33, 256, INT32_MAX, 256, out);
    run("norm bound above the modulus' half", c, seeds, 3, 101, 256, 52, 256, out);
    g_mt_fail = true; run("the generators run out", c, seeds, 3, Q, 256, 52, 256, out); g_mt_fail = false;
    g_launch_rc = FZ_E_HIP; run("the launch fails", c, seeds, 3, Q, 256, 52, 256, out); g_launch_rc = FZ_OK;
    run("the call after it", c, seeds, 3, Q, 256, 52, 256, out);
    run("and the next waits", c, seeds, 3, Q, 256, 52, 256, out);
    run("empty", c, nullptr, 0, Q, 256, 52, 256, nullptr);
    // the refusals in the order they are made, then each with the one after it
    struct SA { fz_ctx *ctx; const uint64_t *s; size_t N; int64_t q; int degree; int64_t norm, weight; int32_t *out; };
    struct SF { std::string name; std::function<void(SA &)> spoil; };
    static uint64_t first[3] = {UINT64_MAX, 5, 6}, last[3] = {5, 6, UINT64_MAX};
    const std::vector<SF> L = {
        {"ctx", [](SA &a) { a.ctx = nullptr; }}, {"seeds_null", [](SA &a) { a.s = nullptr; }}, {"out_null", [](SA &a) { a.out = nullptr; }},
        {"degree0", [](SA &a) { a.degree = 0; }}, {"modulus1", [](SA &a) { a.q = 1; }}, {"capture", [](SA &a) { a.ctx->capturing = 1; }},
        {"empty_range", [](SA &a) { a.norm = 0; }}, {"range_2_32", [](SA &a) { a.q = (int64_t)1 << 40; a.norm = (int64_t)1 << 32; }},
        {"bound_above_int32", [](SA &a) { a.q = (int64_t)1 << 40; a.norm = (int64_t)1 << 31; }}, {"weight_below_degree", [](SA &a) { a.weight = a.degree - 1; }},
        {"seed_max_first", [](SA &a) { a.s = first; }}, {"seed_max_last", [](SA &a) { a.s = last; }},
    };
    auto call = [&](const std::string &what, SA a) { run(what, a.ctx, a.s, a.N, a.q, a.degree, a.norm, a.weight, a.out); c->capturing = 0; };
    const SA ok{c, seeds, 3, Q, 256, 52, 256, out};
    for (size_t i = 0; i < L.size(); ++i) { SA a = ok; L[i].spoil(a); call(L[i].name, a); }
    for (size_t i = 0; i + 1 < L.size(); ++i) { SA a = ok; L[i + 1].spoil(a); L[i].spoil(a); call(L[i].name + "+" + L[i + 1].name, a); }
    { SA a = ok; a.N = 0; a.s = nullptr; a.out = nullptr; a.weight = 0; call("empty, weight_below_degree", a); }
    drop_ctx(c);
}

int main() {
#if defined(__has_feature)
#if __has_feature(address_sanitizer)
    printf("sanitizers: address on\n");
#endif
#endif
    const std::vector<Entry> E = entries();
    for (const char *cname : {"d256", "d64", "d128", "ring12", "q32"}) {
        fz_ctx *c = make_ctx(cname);
        const std::string s = cname;
        for (const Entry &e : E) {
            const bool pw = std::string(e.name).compare(0, 5, "fz_pw") == 0;
            walk(c, e, s == "d256" || s == "d128" || s == "ring12" || (s == "q32" && pw), s == "d256" || (s == "q32" && pw));
        }
        drop_ctx(c);
    }
    for (const Entry &e : E)
        if (e.flags & AREAS) { growth("d128", e); growth("d256", e); }
    challenge_walk();
    sampler_walk();
    long a = 0, e = 0, st = 0;
    stub_live(&a, &e, &st);
    if (a || e || st) { printf("FAIL: something is left allocated\n"); return 1; }
    printf("ALL OK\n");
    return 0;
}
'''

DRIVER = STUB + "#include <cstdarg>\n" + DRIVER_BODY


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("capi_entries")
    exe = build_driver(tmp, UNITS, DRIVER, "-fsanitize=address,undefined", name="capi_entries", sources=[os.path.join(CSRC, "fz_host.cpp")],
                       flags=["-fno-sanitize-recover=all"])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=dict(os.environ, FZ_POOL_MB="0"))
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout.splitlines()


def test_driver_runs_clean_under_the_sanitizers(lines):
    assert lines[0] == "sanitizers: address on" and lines[-1] == "ALL OK"
    assert not [ln for ln in lines if ln.startswith("FAIL")]


def test_output_is_the_recorded_one_line_for_line(lines):
    want = open(GOLDEN).read().splitlines()
    diff = [(i + 1, a, b) for i, (a, b) in enumerate(zip(want, lines)) if a != b]
    assert not diff and len(want) == len(lines), diff[:5]


LINE = re.compile(r'^(\w+) (fz_\w+) \[([^\]]*)\] -> (rc=-?\d+(?: "[^"]*")?) \|(.*) \|(.*)$')


def parsed(lines):
    """(context, entry) -> {what: (rc and text, launcher records, runtime calls)}; a label used twice keeps its first line"""
    out = {}
    for ln in lines[1:-1]:
        m = LINE.match(ln)
        assert m, ln
        out.setdefault((m.group(1), m.group(2)), {}).setdefault(m.group(3), (m.group(4), m.group(5).strip(), m.group(6).strip()))
    return out


def test_every_entry_of_the_unit_is_walked(lines):
    """every extern "C" function of the two units has its lines on every context it is walked on, with the good call and the empty
    one; the entries with walks of their own (challenge_walk, sampler_walk) are exactly those of fz_staged_capi.hip"""
    rows, staged = (set(re.findall(r"^int (fz_\w+)\(", open(os.path.join(CSRC, unit + ".hip")).read(), re.M)) for unit in ("fz_capi", "fz_staged_capi"))
    exported = rows | staged
    assert len(exported) >= 40 and not rows & staged
    table = parsed(lines)
    assert {e for _, e in table} == exported
    special = ("fz_challenge_coefficients_dev", "fz_challenge_hat_dev", "fz_challenge_hat_msgs_dev", "fz_sample_secret_polys_dev")
    assert staged == set(special)
    for e in exported - set(special):
        for c in ("d256", "d64", "d128", "ring12", "q32"):
            assert {"good", "empty"} <= set(table[(c, e)]), (c, e)
        assert [w for w in table[("d256", e)] if "+" in w], e


def test_the_earlier_fault_of_every_adjacent_pair_wins(lines):
    pairs = 0
    for (c, e), rows in parsed(lines).items():
        for w in rows:
            first = w.split("+")[0]
            if "+" in w and first in rows:
                assert rows[w] == rows[first], (c, e, w, rows[w], rows[first])
                pairs += 1
    assert pairs >= 250


def test_verify_core_parks_its_target_behind_the_inner_layout(lines):
    """degree 128, l = 2: observed 512 | coef 1024 | max_abs 256 | weight 256 bytes -> the partial at 2048, the target 1024 behind it;
    the inner entry's own request fits the area the outer one sized: one allocation in the whole call"""
    for c, partial, target in (("d128", 2048, 3072), ("d256", 3584, 5632)):
        rc, recs, calls = parsed(lines)[(c, "fz_verify_core")]["grow: small"]
        assert rc == "rc=0"
        assert "target_partial(" in recs and "partial=scratch+%d " % partial in recs
        assert "reduce_i64(in=scratch+%d out=scratch+%d " % (partial, target) in recs
        assert calls.count("hipMalloc(") == 1 and "=scratch+0" in calls and "src=verdict+0" in calls    # (the verdict area is there from context creation)
        if c == "d128":
            assert "verdict(target=scratch+%d observed=scratch+0 max_abs=scratch+1536 weight=scratch+1792 " % target in recs
        else:
            assert "verify_fused(" in recs and "target=scratch+%d " % target in recs
