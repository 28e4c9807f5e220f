"""The argument rules of fz_vk_records_async (csrc/fz_key_records_capi.hip) without a GPU: which refusal wins.

In the manner of tests/test_records_entries_host.py: the unit is compiled for the host with fz_context.hip and fz_diag.hip under
AddressSanitizer and UBSan and linked, as a stand-alone program, against the stub HIP runtime of tests/_hip_stub.py and a recording
stand-in for fz_launch_vk_records, the one launcher the unit reaches.  The driver holds the entry's LADDER -- its faults in the
order include/fusion_hip.h gives them: the context and l, the key's bound, the pointers (NULL before misaligned), the degree (the
context's), the size of N records of 2 l rows, the entry's own limit on N -- and prints, on a context of degree 256, one of degree
64 and one of degree 128, one line per call: the good call (which reaches the launcher once, with everything it was handed), each
single fault, each adjacent pair of faults, N == 0 with every pointer NULL and with every pointer misaligned.  A refused call and
a call with N == 0 must make no runtime call and reach no launcher (the driver checks both itself).

tests/golden/key_records_entries.txt is that output; the test requires it line for line and, from the lines alone, that the
earlier fault of every adjacent pair wins.  (l >= 2^22 is the launcher's refusal, behind the device: tests/test_gpu_vk_records.py.)"""
import os
import subprocess

import pytest

from _hip_stub import STUB, build_driver
from test_records_entries_host import parsed

UNITS = ("fz_key_records_capi", "fz_context", "fz_diag")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "key_records_entries.txt")

DRIVER_BODY = r'''
alignas(64) static char g_dummy[4096];
static std::vector<std::string> g_recs;
static long long off_of(const void *p) { return p ? (long long)((const char *)p - g_dummy) : -1; }
int fz_launch_vk_records(fz_ctx *, const int32_t *A, const uint8_t *key, int wk, int64_t kb, size_t n, int l, int32_t *vk, int *st) {
    char buf[512];
    snprintf(buf, sizeof(buf), "vk_records(A=%lld key=%lld wk=%d key_bound=%lld n=%zu l=%d vk=%lld status=%lld)", off_of(A), off_of(key), wk,
             (long long)kb, n, l, off_of(vk), off_of(st));
    g_recs.push_back(buf);
    return FZ_OK;
}

static const uint32_t Q = 2147465729u;
static int g_d = 0;                                      // the context's degree
struct Args {
    fz_ctx *ctx;
    size_t n;
    int l;
    int64_t key_bound;
    char *p[4];                                          // A, key bytes, vk, status
};
struct Fault { std::string name; std::function<void(Args &)> spoil; };
static int call(Args &a) {
    return fz_vk_records_async(a.ctx, (const int32_t *)a.p[0], (const uint8_t *)a.p[1], a.key_bound, a.n, a.l, (int32_t *)a.p[2], (int *)a.p[3]);
}
static std::vector<Fault> ladder() {
    std::vector<Fault> L = {{"ctx", [](Args &a) { a.ctx = nullptr; }},
                            {"l0", [](Args &a) { a.l = 0; }},
                            {"key_bound0", [](Args &a) { a.key_bound = 0; }},
                            {"key_bound_hi", [](Args &a) { a.key_bound = ((int64_t)Q - 1) / 2 + 1; }}};
    for (int k = 0; k < 4; ++k) L.push_back({"null" + std::to_string(k), [k](Args &a) { a.p[k] = nullptr; }});
    for (int k = 0; k < 4; ++k) L.push_back({"mis" + std::to_string(k), [k](Args &a) { a.p[k] += 8; }});
    L.push_back({"size_rows", [](Args &a) { a.l = 0x7fffffff / (2 * g_d) + 1; }});
    L.push_back({"size_n", [](Args &a) { a.n = ((size_t)-1 >> 3) / ((size_t)2 * a.l * g_d) + 1; }});
    L.push_back({"grid", [](Args &a) { a.n = 0x40000000; }});
    return L;
}

static int g_fail = 0;
static Args good(fz_ctx *c) {
    Args a{c, 3, 4, 52, {nullptr, nullptr, nullptr, nullptr}};
    for (int k = 0; k < 4; ++k) a.p[k] = g_dummy + 64 * (k + 1);
    return a;
}
static void run(const std::string &what, Args a, bool expect_quiet) {
    const size_t mark = stub_mark(), recs = g_recs.size();
    const int rc = call(a);
    const size_t calls = stub_mark() - mark, reached = g_recs.size() - recs;
    printf("d%d vk_records [%s] -> rc=%d", g_d, what.c_str(), rc);
    if (rc != FZ_OK) printf(" \"%s\"", fz_last_error());
    for (size_t k = recs; k < g_recs.size(); ++k) printf(" %s", g_recs[k].c_str());
    printf(" calls=%zu\n", calls);
    if ((rc != FZ_OK || expect_quiet) && (calls || reached)) { printf("FAIL: a refused or empty call reached the runtime or the launcher\n"); ++g_fail; }
    if (rc == FZ_OK && !expect_quiet && reached != 1) { printf("FAIL: an accepted call reached the launcher %zu times\n", reached); ++g_fail; }
}
static void walk(fz_ctx *c) {
    const std::vector<Fault> L = ladder();
    run("good", good(c), false);
    for (size_t i = 0; i < L.size(); ++i) {
        Args a = good(c);
        L[i].spoil(a);
        run(L[i].name, a, false);
    }
    for (size_t i = 0; i + 1 < L.size(); ++i) {            // the later fault first: where both touch one argument, the earlier one's value stands
        Args a = good(c);
        L[i + 1].spoil(a);
        L[i].spoil(a);
        run(L[i].name + "+" + L[i + 1].name, a, false);
    }
    for (int bad = 0; bad < 2; ++bad) {                     // nothing to do: FZ_OK whatever the pointers
        Args a = good(c);
        a.n = 0;
        for (int k = 0; k < 4; ++k) a.p[k] = bad ? a.p[k] + 4 : nullptr;
        run(bad ? "n0 misaligned" : "n0 null", a, true);
    }
    {                                                       // the largest N the grid takes
        Args a = good(c);
        a.n = 0x3fffffff;
        run("good, N at the grid's limit", a, false);
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
        walk(c);
        fz_ctx_destroy(c);
    }
    long a = 0, e = 0, st = 0;
    stub_live(&a, &e, &st);
    if (a || e || st) { printf("FAIL: something is left allocated\n"); ++g_fail; }
    printf(g_fail ? "FAILED %d\n" : "ALL OK\n", g_fail);
    return g_fail ? 1 : 0;
}
'''

DRIVER = STUB + DRIVER_BODY


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("key_records_entries")
    exe = build_driver(tmp, UNITS, DRIVER, "-fsanitize=address,undefined", name="key_records_entries", flags=["-fno-sanitize-recover=all"])
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


def test_the_entry_is_walked_on_every_context(lines):
    table = parsed(lines)
    assert set(table) == {(d, "vk_records") for d in (256, 64, 128)}
    for (d, e), rows in table.items():
        singles = [w for w in rows if "+" not in w and w not in ("good", "n0 null", "n0 misaligned") and not w.startswith("good,")]
        pairs = [w for w in rows if "+" in w]
        assert len(singles) == 15 and len(pairs) == 14, (d, singles)
        for w in singles:                                   # a single fault is refused, and reaches nothing
            assert rows[w][0] != "rc=#" and not rows[w][1], (d, w)
        if d != 128:
            for w in ("good", "good, N at the grid's limit"):
                assert rows[w][0] == "rc=#" and rows[w][1].startswith("vk_records("), (d, w)
        else:
            assert rows["good"][0] == 'rc=m# "the byte encoding needs degree # or #"', d


def test_the_good_call_hands_the_launcher_what_it_was_given(lines):
    """the key's width from its bound (52 -> 7 bits), the counts and the four pointers in the launcher's order"""
    for d in (256, 64):
        good = [ln for ln in lines if ln.startswith(f"d{d} vk_records [good]")]
        assert len(good) == 1
        assert "vk_records(A=64 key=128 wk=7 key_bound=52 n=3 l=4 vk=192 status=256)" in good[0], good[0]


def test_the_rules_are_the_documented_ones_in_their_order(lines):
    rows = {d: parsed(lines)[(d, "vk_records")] for d in (256, 64, 128)}
    for d in (256, 64):
        r = rows[d]
        assert r["ctx"][0] == r["l0"][0] == 'rc=m# "bad argument"'
        assert r["key_bound0"][0] == r["key_bound_hi"][0] and "key bound" in r["key_bound0"][0]
        assert all(r[f"null{k}"][0] == 'rc=m# "NULL argument"' for k in range(4))
        assert all(r[f"mis{k}"][0] == 'rc=m# "buffers must be #-byte aligned"' for k in range(4))
        assert "records of # rows are too many" in r["size_rows"][0] and "records of # rows are too many" in r["size_n"][0]
        assert "keys of # rows are too many" in r["grid"][0]
    # the degree comes behind the pointers and in front of the sizes
    r = rows[128]
    assert r["mis3"][0] == 'rc=m# "buffers must be #-byte aligned"'
    assert r["size_rows"][0] == r["size_n"][0] == r["grid"][0] == r["good"][0]


def test_the_earlier_fault_of_every_adjacent_pair_wins(lines):
    for (d, e), rows in parsed(lines).items():
        for w in rows:
            if "+" in w:
                first = w.split("+")[0]
                assert rows[w] == rows[first], (d, w, rows[w], rows[first])


def test_nothing_to_do_is_ok_whatever_the_pointers(lines):
    for (d, e), rows in parsed(lines).items():
        assert rows["n0 null"] == ("rc=#", "") and rows["n0 misaligned"] == ("rc=#", ""), d
