"""The argument rules of fz_aggregate_target_encoded_ragged_async (csrc/fz_aggregate_target_encoded_capi.hip) without a GPU: which
refusal wins.

In the manner of tests/test_records_entries_host.py: the unit is compiled for the host with fz_context.hip and fz_diag.hip under
AddressSanitizer and UBSan and linked, as a stand-alone program, against the stub HIP runtime of tests/_hip_stub.py and a recording
stand-in for fz_launch_aggregate_target_encoded_ragged, the one launcher the unit reaches.  The driver holds the entry's LADDER --
the faults of fz_aggregate_encoded_ragged_async in its order (the offsets, alpha_hat and the aggregates' alignment, which are looked
at whatever the groups hold; the context and l; the bound; the pointers, NULL before misaligned; the degree, the context's; the
sizes; records that are no whole units; decreasing offsets; the partials' stride; a group of 2^22 signers; 2^32 - 64 records), then
what the targets add: their pointers, NULL before misaligned, and their stride -- and prints, on a context of degree 256, one of
degree 64 and one of degree 128, one line per call: the good call (which reaches the launcher once, with everything it was
handed), each single fault, each adjacent pair of faults, groups == 0 with every pointer NULL and with every pointer misaligned,
and N == 0 in all groups with no stream, no coefficients, no keys and no challenges.  A refused call and a call with groups == 0
must make no runtime call and reach no launcher (the driver checks both itself).

tests/golden/aggregate_target_encoded_entries.txt is that output; the test requires it line for line and, from the lines alone,
that the earlier fault of every adjacent pair wins."""
import os
import subprocess

import pytest

from _hip_stub import STUB, build_driver
from test_records_entries_host import parsed

UNITS = ("fz_aggregate_target_encoded_capi", "fz_context", "fz_diag")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "aggregate_target_encoded_entries.txt")
ENTRY = "aggregate_target_encoded_ragged"

DRIVER_BODY = r'''
alignas(64) static char g_dummy[4096];
static std::vector<std::string> g_recs;
static long long off_of(const void *p) { return p ? (long long)((const char *)p - g_dummy) : -1; }
int fz_launch_aggregate_target_encoded_ragged(fz_ctx *, const uint8_t *b, const int32_t *alpha, const int *skip, const int32_t *vk, const int32_t *chal,
                                              const size_t *off, size_t groups, int l, int w, int64_t bound, int64_t *part, size_t stride, int64_t *tpart,
                                              size_t tstride, int32_t *out) {
    char buf[640];
    snprintf(buf, sizeof(buf), "aggregate_target_encoded_ragged(bytes=%lld alpha=%lld skip=%lld vk=%lld chal=%lld groups=%zu total=%zu l=%d w=%d bound=%lld "
             "partial=%lld stride=%zu target=%lld tstride=%zu out=%lld)", off_of(b), off_of(alpha), off_of(skip), off_of(vk), off_of(chal), groups, off[groups],
             l, w, (long long)bound, off_of(part), stride, off_of(tpart), tstride, off_of(out));
    g_recs.push_back(buf);
    return FZ_OK;
}

static const uint32_t Q = 2147465729u;
static int g_d = 0;                                      // the context's degree
struct Args {
    fz_ctx *ctx;
    int l;
    int64_t bound;
    char *p[8];                                          // bytes, partial, alpha_hat, out, skip, vk, c_hat, target partial
    std::vector<size_t> off;                             // the offsets (empty: NULL), the groups and the strides
    size_t groups, stride, tstride;
};
struct Fault { std::string name; std::function<void(Args &)> spoil; int only_degree; };
static Fault F(const std::string &name, std::function<void(Args &)> f, int only_degree = 0) { return {name, f, only_degree}; }
static Fault null_at(int k) { return F("null" + std::to_string(k), [k](Args &a) { a.p[k] = nullptr; }); }
static Fault mis_at(int k, int by = 8) { return F("mis" + std::to_string(k), [k, by](Args &a) { a.p[k] += by; }); }
static int call(Args &a) {
    return fz_aggregate_target_encoded_ragged_async(a.ctx, (const uint8_t *)a.p[0], (const int32_t *)a.p[2], (const int *)a.p[4], (const int32_t *)a.p[5],
                                                    (const int32_t *)a.p[6], a.off.empty() ? nullptr : a.off.data(), a.groups, a.l, a.bound,
                                                    (int64_t *)a.p[1], a.stride, (int64_t *)a.p[7], a.tstride, (int32_t *)a.p[3]);
}
static std::vector<Fault> ladder() {
    return {F("offsets_null", [](Args &a) { a.off.clear(); }), null_at(2), mis_at(2), mis_at(3),
            F("ctx", [](Args &a) { a.ctx = nullptr; }), F("l0", [](Args &a) { a.l = 0; }),
            F("bound0", [](Args &a) { a.bound = 0; }), F("bound_hi", [](Args &a) { a.bound = ((int64_t)Q - 1) / 2 + 1; }),
            null_at(0), null_at(1), mis_at(0), mis_at(1),
            F("size_rows", [](Args &a) { a.l = 0x7fffffff / g_d + 1; }),
            F("size_n", [](Args &a) { a.groups = 2; a.off = {0, 1, ((size_t)-1 >> 3) / ((size_t)a.l * g_d) + 1}; }),
            // records of 24 bytes (one row of degree 64, 3-bit fields): no multiple of 16.  At degree 256 every record is one.
            F("part_units", [](Args &a) { a.l = 1; a.bound = 2; }, 64),
            F("decreasing", [](Args &a) { a.groups = 2; a.off = {0, 2, 1}; }),
            F("stride_short", [](Args &a) { a.stride = (size_t)a.l * g_d - 2; }),
            F("stride_odd", [](Args &a) { a.stride += 1; }),
            F("signers", [](Args &a) { a.groups = 2; a.off = {0, (size_t)1 << 22, ((size_t)1 << 22) + 1}; }),
            F("total", [](Args &a) { a.groups = 1025; a.off.assign(1026, 0); for (size_t g = 0; g < 1025; ++g) a.off[g] = g * (((size_t)1 << 22) - 1); a.off[1025] = 0xffffffc0ull; }),
            null_at(7), null_at(5), null_at(6), mis_at(5), mis_at(6), mis_at(7, 4),
            F("tstride_short", [](Args &a) { a.tstride = (size_t)g_d - 2; }),
            F("tstride_odd", [](Args &a) { a.tstride += 1; })};
}

static int g_fail = 0;
static Args good(fz_ctx *c) {
    Args a{c, 4, 2, {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}, {0, 1, 3}, 2, (size_t)4 * g_d, (size_t)g_d + 2};
    for (int k = 0; k < 8; ++k) a.p[k] = g_dummy + 64 * (k + 1);
    return a;
}
static void run(const std::string &what, Args a, bool expect_quiet) {
    const size_t mark = stub_mark(), recs = g_recs.size();
    const int rc = call(a);
    const size_t calls = stub_mark() - mark, reached = g_recs.size() - recs;
    printf("d%d aggregate_target_encoded_ragged [%s] -> rc=%d", g_d, what.c_str(), rc);
    if (rc != FZ_OK) printf(" \"%s\"", fz_last_error());
    for (size_t k = recs; k < g_recs.size(); ++k) printf(" %s", g_recs[k].c_str());
    printf(" calls=%zu\n", calls);
    if ((rc != FZ_OK || expect_quiet) && (calls || reached)) { printf("FAIL: a refused or empty call reached the runtime or the launcher\n"); ++g_fail; }
    if (rc == FZ_OK && !expect_quiet && reached != 1) { printf("FAIL: an accepted call reached the launcher %zu times\n", reached); ++g_fail; }
}
static void walk(fz_ctx *c) {
    std::vector<Fault> L;
    for (const Fault &f : ladder()) if (!f.only_degree || f.only_degree == g_d) L.push_back(f);
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
    for (int bad = 0; bad < 2; ++bad) {                     // nothing to do: FZ_OK whatever the pointers (but for what the entry looks at first)
        Args a = good(c);
        a.groups = 0;
        for (int k = 0; k < 8; ++k) a.p[k] = bad ? a.p[k] + 4 : nullptr;
        run(bad ? "n0 misaligned" : "n0 null", a, true);
    }
    {                                                       // every group empty: nothing is read, only the partials are needed
        Args a = good(c);
        a.off = {0, 0, 0};
        a.p[0] = a.p[2] = a.p[4] = a.p[5] = a.p[6] = nullptr;
        run("empty groups, no stream", a, false);
    }
    {                                                       // one group: neither stride is looked at for parity
        Args a = good(c);
        a.groups = 1; a.off = {0, 3}; a.stride = 1; a.tstride = (size_t)g_d + 1; a.p[3] = nullptr;
        run("good, one group", a, false);
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
NEW_RUNGS = ("null7", "null5", "null6", "mis5", "mis6", "mis7", "tstride_short", "tstride_odd")


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("aggregate_target_encoded_entries")
    exe = build_driver(tmp, UNITS, DRIVER, "-fsanitize=address,undefined", name="aggregate_target_encoded_entries",
                       flags=["-fno-sanitize-recover=all"])
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
    assert set(table) == {(d, ENTRY) for d in (256, 64, 128)}
    for (d, e), rows in table.items():
        singles = [w for w in rows if "+" not in w and w not in ("good", "n0 null", "n0 misaligned") and not w.startswith(("good,", "empty"))]
        pairs = [w for w in rows if "+" in w]
        assert len(singles) == (28 if d == 64 else 27) and len(pairs) == len(singles) - 1, (d, singles)
        for w in singles:                                   # a single fault is refused, and reaches nothing
            assert rows[w][0] != "rc=#" and not rows[w][1], (d, w)
        for w in ("good", "good, one group", "empty groups, no stream"):
            if d != 128:
                assert rows[w][0] == "rc=#" and rows[w][1].startswith(ENTRY + "("), (d, w)
            else:
                assert rows[w][0] == 'rc=m# "the byte encoding needs degree # or #"', (d, w)


def test_the_good_call_hands_the_launcher_what_it_was_given(lines):
    """the width from the bound (2 -> 3 bits), the groups, both strides and the eight pointers in the launcher's order"""
    for d in (256, 64):
        good = [ln for ln in lines if ln.startswith(f"d{d} {ENTRY} [good]")]
        assert len(good) == 1
        assert (f"{ENTRY}(bytes=64 alpha=192 skip=320 vk=384 chal=448 groups=2 total=3 l=4 w=3 bound=2 partial=128 stride={4 * d} "
                f"target=512 tstride={d + 2} out=256)") in good[0], good[0]
        empty = [ln for ln in lines if ln.startswith(f"d{d} {ENTRY} [empty groups, no stream]")]
        assert len(empty) == 1 and "(bytes=-1 alpha=-1 skip=-1 vk=-1 chal=-1 groups=2 total=0 " in empty[0], empty


def test_the_rules_are_the_ragged_entrys_then_the_targets(lines):
    """the old rungs answer with fz_aggregate_encoded_ragged_async's own words (tests/golden/records_entries.txt holds them for that
    entry: same rung, same context, same text); the new ones come behind all of them"""
    here = parsed(lines)
    with open(os.path.join(os.path.dirname(GOLDEN), "records_entries.txt")) as fh:
        there = parsed(fh.read().splitlines())
    for d in (256, 64, 128):
        new, old = here[(d, ENTRY)], there[(d, "aggregate_encoded_ragged")]
        shared = [w for w in old if "+" not in w and w not in ("good", "n0 null", "empty groups, no stream")]
        assert len(shared) >= 20, shared
        for w in shared:
            assert new[w][0] == old[w][0], (d, w, new[w], old[w])
    for d in (256, 64):
        r = here[(d, ENTRY)]
        assert r["null7"][0] == r["null5"][0] == r["null6"][0] == 'rc=m# "NULL argument"'
        assert r["mis5"][0] == r["mis6"][0] == 'rc=m# "keys and challenges must be #-byte aligned"'
        assert r["mis7"][0] == 'rc=m# "target partials must be #-byte aligned"'
        assert r["tstride_short"][0] == r["tstride_odd"][0] and "target_stride" in r["tstride_short"][0]
        assert r["total+null7"] == r["total"]               # the last of the old rules in front of the first of the new
    r = here[(128, ENTRY)]                                  # the degree comes in front of everything the targets add
    assert all(r[w][0] == r["good"][0] for w in NEW_RUNGS)


def test_the_earlier_fault_of_every_adjacent_pair_wins(lines):
    for (d, e), rows in parsed(lines).items():
        for w in rows:
            if "+" in w:
                first = w.split("+")[0]
                assert rows[w] == rows[first], (d, w, rows[w], rows[first])


def test_no_groups_is_ok_whatever_the_pointers_but_the_first_rule(lines):
    for (d, e), rows in parsed(lines).items():
        assert rows["n0 null"] == ("rc=#", ""), d
        assert rows["n0 misaligned"][0].startswith('rc=m# "alpha_hat and the aggregate'), d
