"""The argument rules of the nine compact-bytes entries (csrc/fz_records_capi.hip) without a GPU: which refusal wins.

The unit is compiled for the host with fz_context.hip and fz_diag.hip under AddressSanitizer and UBSan and linked, as a stand-alone
program, against the stub HIP runtime of tests/_hip_stub.py and recording stand-ins for the fz_launch_* the entries reach.  For each
entry the driver holds its LADDER: its faults in the order its documentation gives them (conditions that hold whatever n is, the
context and the rows, the bounds, the pointers -- NULL before misaligned --, the degree, the size, the entry's own limits).  On a
context of degree 256, one of degree 64 and one of degree 128 (the degree's rung is the context's) it prints one line per call: the
good call (which reaches its launcher once: every count, width, bound and pointer it was handed is printed), each single fault,
each adjacent pair of faults, n == 0 with every pointer NULL and with every pointer misaligned.  A refused call and a call with
n == 0 must make no runtime call and reach no launcher (the driver checks both itself).

tests/golden/records_entries.txt is that output.  It was not written by hand: the same driver was built against the sources in which
eight of the entries lived in fz_capi.hip and the keygen entry, with its checks written out by hand, in fz_keygen_records.hip, and the
two outputs were compared line for line.  They are equal but for one wording, which docs/HISTORY.md section Z lists: the keygen
entry's size refusal now speaks of "N records of 2 l rows" as every entry does, no longer of "N keys of l rows".  The test requires
the recorded output line for line, and, from the lines
alone, that the earlier fault of every adjacent pair wins."""
import os
import re
import subprocess

import pytest

from _hip_stub import STUB, build_driver

UNITS = ("fz_records_capi", "fz_context", "fz_diag")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "records_entries.txt")

DRIVER_BODY = r'''
// ---- recording stand-ins for the launchers: everything they were handed, pointers as offsets into the driver's dummy block ----
alignas(64) static char g_dummy[4096];
static std::vector<std::string> g_recs;
static long long off_of(const void *p) { return p ? (long long)((const char *)p - g_dummy) : -1; }
#define LL(x) (long long)(x)
static int recd(const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_recs.push_back(buf);
    return FZ_OK;
}
int fz_launch_records(fz_ctx *, bool decode, const void *src, void *dst, size_t n, int rows, bool coef, int w, int64_t bound, int *st) {
    return recd("records(decode=%d src=%lld dst=%lld n=%zu rows=%d coef=%d w=%d bound=%lld status=%lld)", (int)decode, off_of(src), off_of(dst), n, rows, (int)coef, w, LL(bound), off_of(st));
}
int fz_launch_check_records(fz_ctx *, const uint8_t *b, size_t n, int rows, int w, int64_t bound, int *st) {
    return recd("check_records(bytes=%lld n=%zu rows=%d w=%d bound=%lld status=%lld)", off_of(b), n, rows, w, LL(bound), off_of(st));
}
int fz_launch_sign_encoded(fz_ctx *, const int32_t *sk, const int32_t *c, size_t n, int l, int w, int64_t bound, uint8_t *b, int *st) {
    return recd("sign_encoded(sk=%lld c=%lld n=%zu l=%d w=%d bound=%lld bytes=%lld status=%lld)", off_of(sk), off_of(c), n, l, w, LL(bound), off_of(b), off_of(st));
}
int fz_launch_sign_records(fz_ctx *, const uint8_t *key, int wk, int64_t kb, const int32_t *c, size_t n, int l, int w, int64_t bound, uint8_t *b, int *st) {
    return recd("sign_records(key=%lld wk=%d key_bound=%lld c=%lld n=%zu l=%d w=%d bound=%lld bytes=%lld status=%lld)", off_of(key), wk, LL(kb), off_of(c), n, l, w,
                LL(bound), off_of(b), off_of(st));
}
int fz_launch_keygen_records(fz_ctx *, const int32_t *A, const int32_t *coef, bool rows, size_t n, int l, int wk, int64_t kb, uint8_t *b, int32_t *vk, int *st) {
    return recd("keygen_records(A=%lld coef=%lld rows=%d n=%zu l=%d wk=%d key_bound=%lld bytes=%lld vk=%lld status=%lld)", off_of(A), off_of(coef), (int)rows, n, l, wk,
                LL(kb), off_of(b), off_of(vk), off_of(st));
}
int fz_launch_aggregate_encoded(fz_ctx *, const uint8_t *b, const int32_t *alpha, const int *skip, size_t n, int l, int w, int64_t bound, int64_t *part, int32_t *out) {
    return recd("aggregate_encoded(bytes=%lld alpha=%lld skip=%lld n=%zu l=%d w=%d bound=%lld partial=%lld out=%lld)", off_of(b), off_of(alpha), off_of(skip), n, l, w,
                LL(bound), off_of(part), off_of(out));
}
int fz_launch_aggregate_encoded_ragged(fz_ctx *, const uint8_t *b, const int32_t *alpha, const int *skip, const size_t *off, size_t groups, int l, int w, int64_t bound,
                                       int64_t *part, size_t stride, int32_t *out) {
    return recd("aggregate_encoded_ragged(bytes=%lld alpha=%lld skip=%lld groups=%zu total=%zu l=%d w=%d bound=%lld partial=%lld stride=%zu out=%lld)", off_of(b),
                off_of(alpha), off_of(skip), groups, off[groups], l, w, LL(bound), off_of(part), stride, off_of(out));
}
int fz_launch_verify_encoded(fz_ctx *, const int32_t *A, const uint8_t *b, size_t n, int l, int w, int64_t bound, const int32_t *target, const int32_t *vk,
                             const int32_t *chal, int *verdict) {
    return recd("verify_encoded(A=%lld bytes=%lld n=%zu l=%d w=%d bound=%lld target=%lld vk=%lld chal=%lld verdict=%lld)", off_of(A), off_of(b), n, l, w, LL(bound),
                off_of(target), off_of(vk), off_of(chal), off_of(verdict));
}

// ---- a call's arguments, the faults that spoil them, the entries ----
static const uint32_t Q = 2147465729u;
static int g_d = 0;                                      // the context's degree
struct Args {
    fz_ctx *ctx;
    size_t n;
    int l, coef_rows;
    int64_t bound, key_bound;
    char *p[6];                                          // the entry's pointers, in its own order
    std::vector<size_t> off;                             // the ragged entry's offsets (empty: NULL), its groups and stride
    size_t groups, stride;
};
struct Fault { std::string name; std::function<void(Args &)> spoil; int only_degree; };
struct Entry { const char *name; int nptr; std::function<int(Args &)> call; std::vector<Fault> ladder; };

static Fault F(const char *name, std::function<void(Args &)> f, int only_degree = 0) { return {name, f, only_degree}; }
static Fault null_at(int k) { return F(("null" + std::to_string(k)).c_str(), [k](Args &a) { a.p[k] = nullptr; }); }
static Fault mis_at(int k, int by = 8) { return F(("mis" + std::to_string(k)).c_str(), [k, by](Args &a) { a.p[k] += by; }); }
// the rungs every entry shares; `per`: rows of a record per l (2 for the key records)
static std::vector<Fault> head() {
    return {F("ctx", [](Args &a) { a.ctx = nullptr; }), F("l0", [](Args &a) { a.l = 0; })};
}
static std::vector<Fault> bound_rung() {
    return {F("bound0", [](Args &a) { a.bound = 0; }), F("bound_hi", [](Args &a) { a.bound = ((int64_t)Q - 1) / 2 + 1; })};
}
static std::vector<Fault> key_bound_rung() {
    return {F("key_bound0", [](Args &a) { a.key_bound = 0; }), F("key_bound_hi", [](Args &a) { a.key_bound = ((int64_t)Q - 1) / 2 + 1; })};
}
static std::vector<Fault> size_rung(int per) {
    return {F("size_rows", [per](Args &a) { a.l = 0x7fffffff / (per * g_d) + 1; }),
            F("size_n", [per](Args &a) { a.n = ((size_t)-1 >> 3) / ((size_t)per * a.l * g_d) + 1; })};
}
static std::vector<Fault> operator+(std::vector<Fault> a, const std::vector<Fault> &b) { a.insert(a.end(), b.begin(), b.end()); return a; }
// records of 24 bytes (one row of degree 64, 3-bit fields): no multiple of 16.  At degree 256 every record is one.
static Fault part_units() { return F("part_units", [](Args &a) { a.l = 1; a.bound = 2; }, 64); }

static std::vector<Entry> entries() {
    std::vector<Entry> E;
    E.push_back({"encode_records", 3, [](Args &a) { return fz_encode_records_async(a.ctx, (const int32_t *)a.p[0], a.n, a.l, 1, a.bound, (uint8_t *)a.p[1], (int *)a.p[2]); },
                 head() + bound_rung() + std::vector<Fault>{null_at(0), null_at(1), null_at(2), mis_at(0), mis_at(1), mis_at(2)} + size_rung(1)});
    E.push_back({"decode_records", 3, [](Args &a) { return fz_decode_records_async(a.ctx, (const uint8_t *)a.p[0], a.n, a.l, 0, a.bound, (int32_t *)a.p[1], (int *)a.p[2]); },
                 head() + bound_rung() + std::vector<Fault>{null_at(0), null_at(1), null_at(2), mis_at(0), mis_at(1), mis_at(2)} + size_rung(1)});
    E.push_back({"check_records", 2, [](Args &a) { return fz_check_records_async(a.ctx, (const uint8_t *)a.p[0], a.n, a.l, a.bound, (int *)a.p[1]); },
                 head() + bound_rung() + std::vector<Fault>{null_at(0), null_at(1), mis_at(0), mis_at(1)} + size_rung(1)});
    // p: sk_hat, bytes, status, c_hat -- the first three are looked at before the challenges
    E.push_back({"sign_encoded", 4, [](Args &a) { return fz_sign_encoded_async(a.ctx, (const int32_t *)a.p[0], (const int32_t *)a.p[3], a.n, a.l, a.bound, (uint8_t *)a.p[1], (int *)a.p[2]); },
                 head() + bound_rung() + std::vector<Fault>{null_at(0), null_at(1), null_at(2), mis_at(0), mis_at(1), mis_at(2), null_at(3), mis_at(3)} + size_rung(1)});
    // p: key bytes, bytes, status, c_hat
    E.push_back({"sign_records", 4, [](Args &a) { return fz_sign_records_async(a.ctx, (const uint8_t *)a.p[0], a.key_bound, (const int32_t *)a.p[3], a.n, a.l, a.bound, (uint8_t *)a.p[1], (int *)a.p[2]); },
                 head() + key_bound_rung() + bound_rung() +
                     std::vector<Fault>{null_at(0), null_at(1), null_at(2), mis_at(0), mis_at(1), mis_at(2), null_at(3), mis_at(3)} + size_rung(1)});
    // p: A, coef, key bytes, vk, status
    E.push_back({"keygen_records", 5, [](Args &a) { return fz_keygen_records_async(a.ctx, (const int32_t *)a.p[0], (const int32_t *)a.p[1], a.coef_rows, a.n, a.l, a.key_bound, (uint8_t *)a.p[2], (int32_t *)a.p[3], (int *)a.p[4]); },
                 head() + std::vector<Fault>{F("coef_rows", [](Args &a) { a.coef_rows = 2; })} + key_bound_rung() +
                     std::vector<Fault>{null_at(0), null_at(1), null_at(2), null_at(3), null_at(4), mis_at(0), mis_at(1), mis_at(2), mis_at(3), mis_at(4)} + size_rung(2) +
                     std::vector<Fault>{F("grid", [](Args &a) { a.n = 0x40000000; })}});
    // p: bytes, partial, alpha_hat, out, skip -- alpha_hat and out are looked at first, whatever N is
    E.push_back({"aggregate_encoded", 5, [](Args &a) { return fz_aggregate_encoded_async(a.ctx, (const uint8_t *)a.p[0], (const int32_t *)a.p[2], (const int *)a.p[4], a.n, a.l, a.bound, (int64_t *)a.p[1], (int32_t *)a.p[3]); },
                 std::vector<Fault>{null_at(2), mis_at(2), mis_at(3)} + head() + bound_rung() + std::vector<Fault>{null_at(0), null_at(1), mis_at(0), mis_at(1)} + size_rung(1) +
                     std::vector<Fault>{part_units(), F("signers", [](Args &a) { a.n = (size_t)1 << 22; })}});
    // the same, then the offsets and the stride.  (size_n: the total; the records of group 0 stay few)
    E.push_back({"aggregate_encoded_ragged", 5, [](Args &a) { return fz_aggregate_encoded_ragged_async(a.ctx, (const uint8_t *)a.p[0], (const int32_t *)a.p[2], (const int *)a.p[4], a.off.empty() ? nullptr : a.off.data(), a.groups, a.l, a.bound, (int64_t *)a.p[1], a.stride, (int32_t *)a.p[3]); },
                 std::vector<Fault>{F("offsets_null", [](Args &a) { a.off.clear(); }), null_at(2), mis_at(2), mis_at(3)} + head() + bound_rung() +
                     std::vector<Fault>{null_at(0), null_at(1), mis_at(0), mis_at(1),
                                        F("size_rows", [](Args &a) { a.l = 0x7fffffff / g_d + 1; }),
                                        F("size_n", [](Args &a) { a.groups = 2; a.off = {0, 1, ((size_t)-1 >> 3) / ((size_t)a.l * g_d) + 1}; }),
                                        part_units(),
                                        F("decreasing", [](Args &a) { a.groups = 2; a.off = {0, 2, 1}; }),
                                        F("stride_short", [](Args &a) { a.stride = (size_t)a.l * g_d - 2; }),
                                        F("stride_odd", [](Args &a) { a.stride += 1; }),
                                        F("signers", [](Args &a) { a.groups = 2; a.off = {0, (size_t)1 << 22, ((size_t)1 << 22) + 1}; }),
                                        F("total", [](Args &a) { a.groups = 1025; a.off.assign(1026, 0); for (size_t g = 0; g < 1025; ++g) a.off[g] = g * (((size_t)1 << 22) - 1); a.off[1025] = 0xffffffc0ull; })}});
    // p: A, bytes, verdicts, target, vk, c_hat -- target against the pair first, whatever N is
    E.push_back({"verify_encoded", 4, [](Args &a) { return fz_verify_encoded_async(a.ctx, (const int32_t *)a.p[0], (const uint8_t *)a.p[1], a.n, a.l, a.bound, (const int32_t *)a.p[3], (const int32_t *)a.p[4], (const int32_t *)a.p[5], (int *)a.p[2]); },
                 std::vector<Fault>{F("target_and_pair", [](Args &a) { a.p[4] = g_dummy + 64 * 5; a.p[5] = g_dummy + 64 * 6; }), F("half_pair", [](Args &a) { a.p[4] = g_dummy + 64 * 5; })} +
                     head() + bound_rung() + std::vector<Fault>{null_at(0), null_at(1), null_at(2), mis_at(1), mis_at(0), mis_at(3, 2), mis_at(2, 2)} + size_rung(1) +
                     std::vector<Fault>{part_units(), F("record_long", [](Args &a) { a.l = (0x7fffffff / g_d) & ~1; a.bound = ((int64_t)Q - 1) / 2; })}});
    return E;
}

// ---- the walk ----
static int g_fail = 0;
static Args good(fz_ctx *c, const Entry &e) {
    Args a{c, 3, 4, 1, 1, 2, {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}, {0, 1, 3}, 2, (size_t)4 * g_d};
    for (int k = 0; k < e.nptr; ++k) a.p[k] = g_dummy + 64 * (k + 1);
    if (std::string(e.name) == "aggregate_encoded_ragged") a.n = 0;      // (unused: the offsets say how many)
    return a;
}
static void run(const Entry &e, const std::string &what, Args a, bool expect_quiet) {
    const size_t mark = stub_mark(), recs = g_recs.size();
    const int rc = e.call(a);
    const size_t calls = stub_mark() - mark, reached = g_recs.size() - recs;
    printf("d%d %s [%s] -> rc=%d", g_d, e.name, what.c_str(), rc);
    if (rc != FZ_OK) printf(" \"%s\"", fz_last_error());
    for (size_t k = recs; k < g_recs.size(); ++k) printf(" %s", g_recs[k].c_str());
    printf(" calls=%zu\n", calls);
    if ((rc != FZ_OK || expect_quiet) && (calls || reached)) { printf("FAIL: a refused or empty call reached the runtime or a launcher\n"); ++g_fail; }
    if (rc == FZ_OK && !expect_quiet && reached != 1) { printf("FAIL: an accepted call reached %zu launchers\n", reached); ++g_fail; }
}
static void walk(fz_ctx *c, const Entry &e) {
    std::vector<Fault> L;
    for (const Fault &f : e.ladder) if (!f.only_degree || f.only_degree == g_d) L.push_back(f);
    run(e, "good", good(c, e), false);
    for (size_t i = 0; i < L.size(); ++i) {
        Args a = good(c, e);
        L[i].spoil(a);
        run(e, L[i].name, a, false);
    }
    for (size_t i = 0; i + 1 < L.size(); ++i) {            // the later fault first: where both touch one argument, the earlier one's value stands
        Args a = good(c, e);
        L[i + 1].spoil(a);
        L[i].spoil(a);
        run(e, L[i].name + "+" + L[i + 1].name, a, false);
    }
    const bool ragged = std::string(e.name) == "aggregate_encoded_ragged";
    for (int bad = 0; bad < 2; ++bad) {                     // nothing to do: FZ_OK whatever the pointers (but for what an entry looks at first)
        Args a = good(c, e);
        a.n = 0;
        if (ragged) a.groups = 0;
        for (int k = 0; k < 6; ++k) a.p[k] = bad ? (a.p[k] ? a.p[k] + 4 : nullptr) : nullptr;
        if (!bad && std::string(e.name) == "verify_encoded") a.p[3] = g_dummy + 2;      // (exactly one of the target and the pair, whatever N is)
        run(e, bad ? "n0 misaligned" : "n0 null", a, true);
    }
    if (ragged) {                                           // every group empty: no byte is read, the stream may be NULL
        Args a = good(c, e);
        a.off = {0, 0, 0};
        a.p[0] = nullptr; a.p[2] = nullptr;
        run(e, "empty groups, no stream", a, false);
    }
    if (std::string(e.name) == "verify_encoded") {          // against the keys and challenges instead of a target
        Args a = good(c, e);
        a.p[3] = nullptr; a.p[4] = g_dummy + 64 * 5; a.p[5] = g_dummy + 64 * 6;
        run(e, "good, the pair", a, false);
    }
    if (std::string(e.name) == "keygen_records") {          // l polynomials per half
        Args a = good(c, e);
        a.coef_rows = a.l;
        run(e, "good, coef_rows = l", a, false);
    }
}

int main() {
#if defined(__has_feature)
#if __has_feature(address_sanitizer)
    printf("sanitizers: address on\n");
#endif
#endif
    const uint64_t r256 = 3337519u, i256 = 1978410468u;
    for (int d : {256, 64, 128}) {
        fz_ctx *c = nullptr;
        const int rc = d == 256 ? fz_ctx_create(0, Q, 256, (uint32_t)r256, (uint32_t)i256, &c)
                     : d == 64 ? fz_ctx_create(0, Q, 64, 23584283u, 540632852u, &c)
                               : fz_ctx_create(0, Q, 128, (uint32_t)(r256 * r256 % Q), (uint32_t)(i256 * i256 % Q), &c);
        if (rc != FZ_OK) { printf("FAIL context of degree %d: %s\n", d, fz_last_error()); return 2; }
        g_d = d;
        for (const Entry &e : entries()) walk(c, e);
        fz_ctx_destroy(c);
    }
    long a = 0, e = 0, st = 0;
    stub_live(&a, &e, &st);
    if (a || e || st) { printf("FAIL: something is left allocated\n"); ++g_fail; }
    printf(g_fail ? "FAILED %d\n" : "ALL OK\n", g_fail);
    return g_fail ? 1 : 0;
}
'''

DRIVER = STUB + "#include <cstdarg>\n" + DRIVER_BODY
ENTRIES = ("encode_records", "decode_records", "check_records", "sign_encoded", "sign_records", "keygen_records", "aggregate_encoded",
           "aggregate_encoded_ragged", "verify_encoded")           #


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("records_entries")
    exe = build_driver(tmp, UNITS, DRIVER, "-fsanitize=address,undefined", name="records_entries", flags=["-fno-sanitize-recover=all"])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=dict(os.environ, FZ_POOL_MB="0"))
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout.splitlines()


def test_driver_runs_clean_under_the_sanitizers(lines):
    assert lines[0] == "sanitizers: address on" and lines[-1] == "ALL OK"
    assert not [ln for ln in lines if ln.startswith("FAIL")]


def test_output_is_the_recorded_one_line_for_line(lines):
    want = open(GOLDEN).read().splitlines()
    diff = [(i + 1, a, b) for i, (a, b) in enumerate(zip(want, lines)) if a != b]
    assert not diff and len(want) == len(lines), diff[:5]


LINE = re.compile(r'^d(\d+) (\w+) \[([^\]]*)\] -> (rc=-?\d+(?: "[^"]*")?)(.*) calls=(\d+)$')


def parsed(lines):
    """(degree, entry) -> {what: (rc and text with every number masked, launcher records)}"""
    out = {}
    for ln in lines[1:-1]:
        m = LINE.match(ln)
        assert m, ln
        out.setdefault((int(m.group(1)), m.group(2)), {})[m.group(3)] = (re.sub(r"\d+", "#", m.group(4).replace("rc=-", "rc=m")), m.group(5).strip())
    return out


def test_every_entry_is_walked_on_every_context(lines):
    table = parsed(lines)
    assert set(table) == {(d, e) for d in (256, 64, 128) for e in ENTRIES}
    for (d, e), rows in table.items():
        singles = [w for w in rows if "+" not in w and w not in ("good", "n0 null", "n0 misaligned") and not w.startswith(("good,", "empty"))]
        pairs = [w for w in rows if "+" in w]
        assert len(singles) >= 10 and len(pairs) == len(singles) - 1, (d, e)
        # a single fault is refused on a context whose degree the entries take; the good call goes through there, once
        for w in singles:
            assert rows[w][0] != "rc=#" and not rows[w][1], (d, e, w)
        if d != 128:
            assert rows["good"][0] == "rc=#" and rows["good"][1].startswith(e.replace("encode_", "").replace("decode_", "") + "("), (d, e)
        else:
            assert rows["good"][0] == 'rc=m# "the byte encoding needs degree # or #"', (d, e)


def test_the_earlier_fault_of_every_adjacent_pair_wins(lines):
    for (d, e), rows in parsed(lines).items():
        for w in rows:
            if "+" in w:
                first = w.split("+")[0]
                assert rows[w] == rows[first], (d, e, w, rows[w], rows[first])


def test_nothing_to_do_is_ok_whatever_the_pointers(lines):
    """n == 0 (groups == 0) with every pointer NULL, and with every pointer misaligned -- but for the conditions an entry states
    to hold whatever n is: the aggregation entries want alpha_hat and the aggregate aligned"""
    for (d, e), rows in parsed(lines).items():
        assert rows["n0 null"] == ("rc=#", ""), (d, e)
        if e.startswith("aggregate_encoded"):
            assert rows["n0 misaligned"][0].startswith('rc=m# "alpha_hat and the aggregate'), (d, e)
        else:
            assert rows["n0 misaligned"] == ("rc=#", ""), (d, e)
