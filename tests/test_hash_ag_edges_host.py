"""hash_ag for many committees on the device, the parts that need no GPU: the fixtures of tests/_hash_ag_edges.py sit on the edges
they claim and the host pipeline agrees with the plain-Python model on all of them; the kernel's build uses no scratch and spills
nothing; the argument rules of fz_hash_ag_ragged_dev, walked by a stand-alone driver (csrc/fz_hash_ag_capi.hip compiled for the host
under AddressSanitizer and UBSan with the stub HIP runtime of tests/_hip_stub.py and recording stand-ins for the two launchers it
reaches); the ragged key sort; BatchScheme's option and its "auto" rule."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import _hash_ag_edges as H
from _challenge_edges import RATE, SETS, chunks_of
from _hip_stub import CSRC, STUB, build_driver

ALL_SETS = ("s128", "s256", "d128w64", "d16", "d4")


def _sets_with_text_edges():
    return [s for s in ALL_SETS if SETS[s].degree >= 16]


def _cases(set_name):
    return H.all_cases(set_name)


# ---- the fixtures reach their edges --------------------------------------------------------------------------------------------
def test_section_sizes_are_the_issue_s():
    assert H.section_bytes(SETS["s256"]) == 3968 and H.section_bytes(SETS["s128"]) == 1195
    assert 17 * 3968 == 496 * RATE and (18 * 3968) % RATE and all((k * 3968) % RATE for k in range(1, 17))
    assert (136 * 1195) % RATE == 0 and all((k * 1195) % RATE for k in range(1, 136))
    # degree 256: 195 shuffle draws, index bytes for 60 of them -- the rest slice b"" and take j = 0
    ps = SETS["s256"]
    assert ps.degree - 1 - ps.omega_ag == 195 and ps.omega_ag == 60


@pytest.mark.parametrize("set_name", _sets_with_text_edges())
def test_text_fixtures_sit_on_their_residues(set_name):
    ps = SETS[set_name]
    assert [k.residue for k in H.residue_cases(set_name)] == [0, 1, 134, 135]
    for k in H.residue_cases(set_name):
        assert len(H.committee_text(ps, k.vk, k.pre, k.c)) % RATE == k.residue, k.name
    assert [k.piece for k in H.boundary_cases(set_name)] == [0, 1, 2]
    for k in H.boundary_cases(set_name):
        ends = H.piece_ends(ps, k.vk, k.pre, k.c)
        assert ends[k.piece] % RATE == 0 and ends[k.piece] > 0, (k.name, ends)
        t = H.committee_text(ps, k.vk, k.pre, k.c).decode()
        assert t[ends[0]] == "]" and t[ends[1]] == "]" and t[ends[2] - 2:ends[2] + 2] == ")), ", k.name


@pytest.mark.parametrize("set_name", ALL_SETS)
def test_value_fixtures_hold_their_values(set_name):
    ps = SETS[set_name]
    ext, dig = H.value_cases(set_name)
    assert {0, 1, -1, H.HALF, -H.HALF} <= set(int(v) for v in ext.c[:2].ravel()) and len(str(-H.HALF)) == 11
    assert int.from_bytes(bytes(dig.pre[0]), "little") == 0 and len(str(int.from_bytes(bytes(dig.pre[1]), "little"))) == 78
    ch = chunks_of(int.from_bytes(bytes(dig.pre[2]), "little"))
    assert len(ch) == 9 and ch[dig.zero_chunk] == 0 and all(c for j, c in enumerate(ch) if j != dig.zero_chunk)
    assert [k.signers for k in H.stream_cases(set_name)] == list(H.STREAM_SIZES[set_name])
    assert ps.name == set_name


@pytest.mark.parametrize("set_name", ALL_SETS)
def test_host_pipeline_agrees_with_the_model_on_every_fixture(set_name):
    """hashlib's SHAKE-256 of the text the fixture module builds, decoded by fz_decode_coefficients, is what
    fz_aggregation_coefficients returns: a fixture cannot quietly miss its edge, and the model is the host entry's"""
    from fusion_hip import hostpipe as hp
    ps = SETS[set_name]
    P = hp.scheme_params(ps)
    n = H.section_bytes(ps)
    rows = H.case_rows(set_name)
    for k in _cases(set_name):
        got = hp.aggregation_coefficients(P, k.vk[:, 0], k.vk[:, 1], k.pre, k.c, 2)
        b = hashlib.shake_256(H.committee_text(ps, k.vk, k.pre, k.c)).digest(n * len(k.vk))
        via = np.array([hp.decode_coefficients(b[i * n:(i + 1) * n], ps.secpar, ps.modulus, ps.degree, ps.beta_ag, ps.omega_ag)
                        for i in range(len(k.vk))])
        assert np.array_equal(got, via), k.name
        assert np.array_equal(got, rows[k.name]), k.name
        assert (np.count_nonzero(got, axis=1) == min(ps.omega_ag, ps.degree)).all(), k.name


def test_layout_call_names_a_permutation_and_leaves_rows_out():
    vk, pre, c, order, off, want = H.layout_call("s128")
    g = len(off) - 1
    assert g % H.WAVES == 1 and len(set(np.diff(off))) > 1 and len(set(order)) == len(order) == off[-1] < len(vk)
    named = np.zeros(len(vk), dtype=bool)
    named[order] = True
    assert (want[~named] == 0).all() and (np.count_nonzero(want[named], axis=1) == SETS["s128"].omega_ag).all()


# ---- the ragged key sort --------------------------------------------------------------------------------------------------------
def test_ragged_sort_is_the_single_sort_per_group():
    from fusion_hip import hostpipe as hp
    ps = SETS["s128"]
    P = hp.scheme_params(ps)
    sizes = [5, 1, 9, 2, 70]
    n = sum(sizes)
    vk = H.base_rows(ps, n, 60)[0]
    vk[7] = vk[9]                                # equal keys: the sort is stable
    vk[20:, 0, :3] = vk[20, 0, :3]               # long common prefixes
    off = np.concatenate([[0], np.cumsum(sizes)])
    got = hp.sort_by_vk_string_ragged(P, vk[:, 0], vk[:, 1], off, 4)
    for a, b in zip(off[:-1], off[1:]):
        assert np.array_equal(got[a:b], a + hp.sort_by_vk_string(P, vk[a:b, 0], vk[a:b, 1], 1))
    texts = [hp.format_vk(P, vk[i, 0], vk[i, 1]) for i in range(n)]
    a, b = off[2], off[3]
    assert list(got[a:b]) == sorted(range(a, b), key=lambda i: texts[i])
    with pytest.raises(ValueError):
        hp.sort_by_vk_string_ragged(P, vk[:, 0], vk[:, 1], off[:-1], 1)


# ---- the build ------------------------------------------------------------------------------------------------------------------
def test_kernel_compiles_without_spills_or_scratch():
    """hash_ag_wave_kernel: three instantiations (stream words per index chunk), no spill, no scratch, dynamic LDS only"""
    import __graft_entry__ as GE
    from _isa import asm, metadata
    assert "fz_hash_ag.hip" in GE.SOURCES and "fz_hash_ag_capi.hip" in GE.SOURCES
    kernels = metadata(asm("fz_hash_ag"), "hash_ag_wave_kernel")
    assert len(kernels) == 3, sorted(kernels)
    for name, f in kernels.items():
        assert f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] == 0 and f["private_segment_fixed_size"] == 0, (name, f)
        assert f["lds"] == 0, (name, f)


def test_challenge_units_do_not_include_the_new_kernel():
    text = open(os.path.join(CSRC, "fz_challenge.hip")).read()
    assert "fz_hash_ag" not in text


# ---- BatchScheme's option ----------------------------------------------------------------------------------------------------------
def _scheme(hash_ag, threads=16, secpar=256):
    import types
    from fusion_hip import scheme
    bs = scheme.BatchScheme.__new__(scheme.BatchScheme)
    bs.params = types.SimpleNamespace(secpar=secpar)
    bs.hash_ag, bs.device_hash_ag, bs.threads = hash_ag, True, threads
    return bs


def test_option_is_validated_and_defaults_to_host():
    import inspect
    from fusion_hip import scheme
    from fusion_hip._lib import FZ_E_BADARG, FusionHipError
    assert inspect.signature(scheme.BatchScheme.__init__).parameters["hash_ag"].default == "host"
    with pytest.raises(FusionHipError) as e:
        scheme.BatchScheme(SETS["s256"], hash_ag="gpu")
    assert e.value.code == FZ_E_BADARG and "hash_ag" in str(e.value)
    import fusion.fusion as F
    for fn in (F.aggregate_many_from_bytes, F.verify_many_from_bytes, F.aggregate_verify_many_from_bytes):
        assert inspect.signature(fn).parameters["hash_ag"].default == "host"


def test_form_rule():
    assert _scheme("host")._hash_ag_form([16] * 4096) == "host"
    assert _scheme("device")._hash_ag_form([1]) == "device"
    auto = _scheme("auto")
    assert auto._hash_ag_form([16] * 4096) == "device"          # thousands of committees in flight
    assert auto._hash_ag_form([16]) == "host"                   # one serial chain: the host core wins
    assert auto._hash_ag_form([]) == "host"
    auto.device_hash_ag = False                                 # after the first FZ_E_UNSUPPORTED
    assert auto._hash_ag_form([16] * 4096) == "host"
    dev = _scheme("device")
    dev.device_hash_ag = False
    assert dev._hash_ag_form([16] * 4096) == "host"


# ---- the entry's argument rules, by a stand-alone driver -----------------------------------------------------------------------------
DRIVER_BODY = r'''
alignas(64) static char g_dummy[1 << 16];
static int g_launch = 0, g_ntt = 0;
static std::string g_last;
bool fz_challenge_wave_ok(const fz_scheme_params *P) { return P->omega_ch <= 64 && P->degree <= 256 && P->degree >= 4; }
void fz_challenge_weight_table(int, int degree, uint32_t *t) { memset(t, 0, (size_t)(degree + 1) * 16 * 4); }
int fz_launch_ntt(fz_ctx *, const int32_t *, int32_t *, size_t, bool) { ++g_ntt; return FZ_OK; }
int fz_launch_hash_ag(fz_ctx *, const fz_scheme_params *, const int32_t *, const uint8_t *, const int32_t *, const uint32_t *ord, const void *grp,
                      size_t G, const uint32_t *, int32_t *) {
    ++g_launch;
    const uint32_t *g = (const uint32_t *)grp;
    g_last = "groups:";
    for (size_t k = 0; k < G; ++k) {
        g_last += " (" + std::to_string(g[2 * k]) + "+" + std::to_string(g[2 * k + 1]) + ":";
        for (uint32_t i = 0; i < g[2 * k + 1]; ++i) g_last += " " + std::to_string(ord[g[2 * k] + i]);
        g_last += ")";
    }
    return FZ_OK;
}

static fz_scheme_params params(int secpar, int degree, int64_t root, int64_t inv_root, int w_ch, int w_ag) {
    fz_scheme_params P;
    memset(&P, 0, sizeof(P));
    P.modulus = 2147465729; P.root = root; P.inv_root = inv_root; P.degree = degree; P.root_order = 2 * degree; P.secpar = secpar;
    P.omega_ch = w_ch; P.omega_ag = w_ag; P.beta_ch = 1; P.beta_ag = 1;
    P.agg_xof_dst[0] = '3'; P.agg_xof_dst[1] = '2';
    return P;
}
struct Args {
    fz_ctx *ctx; fz_scheme_params P; bool noP;
    char *vk, *pre, *c, *al;
    size_t N, G;
    std::vector<uint32_t> ord; std::vector<size_t> off;
    bool no_ord, no_off;
};
static int g_fail = 0;
static void run(const char *what, Args a, int want_rc) {
    const size_t mark = stub_mark();
    const int l0 = g_launch, n0 = g_ntt;
    const int rc = fz_hash_ag_ragged_dev(a.ctx, a.noP ? nullptr : &a.P, (const int32_t *)a.vk, (const uint8_t *)a.pre, (const int32_t *)a.c, a.N,
                                         a.no_ord ? nullptr : a.ord.data(), a.no_off ? nullptr : a.off.data(), a.G, (int32_t *)a.al);
    size_t enq = 0;
    for (const Call &k : stub_log(mark)) enq += k.fn != "hipSetDevice" && k.fn != "hipStreamIsCapturing";
    printf("[%s] -> rc=%d", what, rc);
    if (rc != FZ_OK) printf(" \"%s\"", fz_last_error());
    printf(" launches=%d transforms=%d", g_launch - l0, g_ntt - n0);
    if (g_launch != l0) printf(" %s", g_last.c_str());
    printf("\n");
    if (rc != want_rc) { printf("FAIL: code %d expected\n", want_rc); ++g_fail; }
    if (rc != FZ_OK && (enq || g_launch != l0 || g_ntt != n0)) { printf("FAIL: a refused call reached the runtime or a launcher\n"); ++g_fail; }
}

int main() {
#if defined(__has_feature)
#if __has_feature(address_sanitizer)
    printf("sanitizers: address on\n");
#endif
#endif
    const uint32_t Q = 2147465729u;
    fz_ctx *c = nullptr, *ring = nullptr;
    if (fz_ctx_create(0, Q, 256, 3337519u, 1978410468u, &c) != FZ_OK) { printf("FAIL context: %s\n", fz_last_error()); return 2; }
    if (fz_ctx_create(0, Q, 256, 0, 0, &ring) != FZ_OK) { printf("FAIL ring context: %s\n", fz_last_error()); return 2; }
    g_copy_nothing = false;
    Args good{c, params(256, 256, 3337519, 1978410468, 60, 60), false, g_dummy + 64, g_dummy + 16384, g_dummy + 32768, g_dummy + 49152,
              6, 3, {4, 0, 5, 2, 1}, {0, 2, 3, 5}, false, false};
    good.N = 6;
    // (the dummy output must hold N rows: the entry clears it)
    static std::vector<int32_t> out(6 * 256 + 64);
    good.al = (char *)(((uintptr_t)out.data() + 63) & ~(uintptr_t)63);
    run("good", good, FZ_OK);
    { Args a = good; a.off = {0, 1, 2, 5}; run("longest first", a, FZ_OK); }
    { Args a = good; a.ctx = nullptr; run("ctx", a, FZ_E_BADARG); }
    { Args a = good; a.noP = true; run("params", a, FZ_E_BADARG); }
    { Args a = good; a.vk = nullptr; run("null vk", a, FZ_E_BADARG); }
    { Args a = good; a.pre = nullptr; run("null pre", a, FZ_E_BADARG); }
    { Args a = good; a.c = nullptr; run("null c_hat", a, FZ_E_BADARG); }
    { Args a = good; a.al = nullptr; run("null alpha", a, FZ_E_BADARG); }
    { Args a = good; a.no_off = true; run("null off", a, FZ_E_BADARG); }
    { Args a = good; a.no_ord = true; run("null order", a, FZ_E_BADARG); }
    { Args a = good; a.P.degree = 64; run("foreign params", a, FZ_E_BADARG); }
    { Args a = good; a.vk += 8; run("misaligned vk", a, FZ_E_BADARG); }
    { Args a = good; a.pre += 2; run("misaligned pre", a, FZ_E_BADARG); }
    { Args a = good; c->capturing = 1; run("capture", a, FZ_E_BADARG); c->capturing = 0; }
    { Args a = good; a.off = {1, 2, 3, 5}; run("off from 1", a, FZ_E_BADARG); }
    { Args a = good; a.off = {0, 3, 2, 5}; run("off decreasing", a, FZ_E_BADARG); }
    { Args a = good; a.off = {0, 2, 2, 5}; run("empty group", a, FZ_E_BADARG); }
    { Args a = good; a.N = 4; a.ord = {3, 0, 1, 2, 1}; run("more entries than rows", a, FZ_E_BADARG); }
    { Args a = good; a.ord = {4, 0, 6, 2, 1}; run("order entry >= N", a, FZ_E_BADARG); }
    { Args a = good; a.ord = {4, 0, 5, 0, 1}; run("order entry twice", a, FZ_E_BADARG); }
    { Args a = good; a.P.beta_ag = 2; run("beta_ag 2", a, FZ_E_UNSUPPORTED); }
    { Args a = good; a.P.omega_ag = 65; run("omega_ag 65", a, FZ_E_UNSUPPORTED); }
    { Args a = good; a.P.omega_ch = 65; run("omega_ch 65", a, FZ_E_UNSUPPORTED); }
    { Args a = good; a.P.secpar = 400; run("index chunks of 51 bytes", a, FZ_E_UNSUPPORTED); }
    { Args a = good; a.ctx = ring; run("ring-only context", a, FZ_E_UNSUPPORTED); }
    { Args a = good; a.G = 0; a.no_off = a.no_ord = true; run("G = 0", a, FZ_OK); }
    { Args a = good; a.N = 0; a.G = 0; a.vk = a.pre = a.c = a.al = nullptr; a.no_off = a.no_ord = true; run("N = 0", a, FZ_OK); }
    fz_ctx_destroy(c);
    fz_ctx_destroy(ring);
    // degrees the kernel does not take (contexts of their own: the parameters must belong to the context)
    fz_ctx *big = nullptr;
    if (fz_ctx_create(0, Q, 512, 0, 0, &big) == FZ_OK) {
        Args a = good; a.ctx = big; a.P.degree = 512; a.P.root_order = 1024;
        run("degree 512", a, FZ_E_UNSUPPORTED);
        fz_ctx_destroy(big);
    } else { printf("FAIL context of degree 512: %s\n", fz_last_error()); ++g_fail; }
    long al = 0, ev = 0, st = 0;
    stub_live(&al, &ev, &st);
    if (al || ev || st) { printf("FAIL: something is left allocated (%ld %ld %ld)\n", al, ev, st); ++g_fail; }
    printf(g_fail ? "FAILED %d\n" : "ALL OK\n", g_fail);
    return g_fail ? 1 : 0;
}
'''


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("hash_ag_entry")
    exe = build_driver(tmp, ("fz_hash_ag_capi", "fz_context", "fz_diag"), STUB + DRIVER_BODY, "-fsanitize=address,undefined", name="hash_ag_entry",
                       sources=[os.path.join(CSRC, "fz_host.cpp")], flags=["-fno-sanitize-recover=all"])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=dict(os.environ, FZ_POOL_MB="0"))
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    return {ln[1:ln.index("]")]: ln[ln.index("]") + 5:] for ln in r.stdout.splitlines() if ln.startswith("[")}


def test_entry_good_call_clears_launches_and_transforms(lines):
    assert lines["good"].startswith("rc=0 launches=1 transforms=1 groups:")
    # the group table is handed out longest first, ties in the caller's order; every group keeps its own rows in its own order
    assert lines["good"].endswith("groups: (0+2: 4 0) (3+2: 2 1) (2+1: 5)")
    assert lines["longest first"].endswith("groups: (2+3: 5 2 1) (0+1: 4) (1+1: 0)")


def test_entry_refusals_their_codes_and_messages(lines):
    for what in ("ctx", "params", "null vk", "null pre", "null c_hat", "null alpha", "null off", "null order"):
        assert lines[what] == 'rc=-1 "NULL argument" launches=0 transforms=0', what
    assert "do not belong to this context" in lines["foreign params"]
    assert lines["misaligned vk"].startswith('rc=-1 "misaligned device pointer"') and lines["misaligned pre"] == lines["misaligned vk"]
    assert "not during graph capture" in lines["capture"]
    assert 'rc=-1 "offsets must start at 0 (got 1)"' in lines["off from 1"]
    assert 'rc=-1 "offsets must not decrease (group 1)"' in lines["off decreasing"]
    assert 'rc=-1 "group 1 is empty"' in lines["empty group"]
    assert 'rc=-1 "5 order entries for 4 rows"' in lines["more entries than rows"]
    assert 'rc=-1 "order entry 2 names row 6 of 6"' in lines["order entry >= N"]
    assert 'rc=-1 "order entry 3 names row 0 a second time"' in lines["order entry twice"]
    assert lines["beta_ag 2"].startswith('rc=-2 "device hash_ag: ternary aggregation coefficients (norm bound 1) only')
    assert lines["degree 512"].startswith('rc=-2 "device hash_ag: degree 4..256, a power of two, only')
    assert lines["omega_ag 65"].startswith('rc=-2 "device hash_ag: weight <= min(64, degree)')
    assert lines["index chunks of 51 bytes"] == lines["omega_ag 65"]
    assert lines["omega_ch 65"].startswith('rc=-2 "device hash_ag: outside the wave form of the challenge pipeline')
    assert lines["ring-only context"].startswith('rc=-2 "ring-only context')
    for what, ln in lines.items():
        if not ln.startswith("rc=0"):
            assert ln.endswith("launches=0 transforms=0"), what


def test_entry_nothing_to_hash_launches_nothing(lines):
    assert lines["G = 0"] == "rc=0 launches=0 transforms=0" and lines["N = 0"] == "rc=0 launches=0 transforms=0"


# ---- the device form through BatchScheme, on a stand-in context (tests/_scheme_buffers.py): what crosses the host link --------------
def _stand_in(monkeypatch, hash_ag):
    import fusion.fusion as F
    from _scheme_buffers import no_finalizers, scheme_on, stand_in_context
    params = F.fusion_setup(128, 1)
    no_finalizers(monkeypatch)
    ctx = stand_in_context(params)
    bs = scheme_on(ctx, params)
    bs.hash_ag = hash_ag
    return params, ctx, bs


MANY = {
    "aggregate_many": lambda bs, a, M, S: bs.aggregate_many(a["vk"], M, a["sig"], S),
    "verify_many": lambda bs, a, M, S: bs.verify_many(a["vk"], M, a["aggs"], S),
    "verify_many_encoded": lambda bs, a, M, S: bs.verify_many_encoded(a["vk"], M, a["aggrecs"], S),
    "aggregate_many_encoded": lambda bs, a, M, S: bs.aggregate_many_encoded(a["vk"], M, a["recs"], S),
    "aggregate_many_encoded[screened]": lambda bs, a, M, S: bs.aggregate_many_encoded(a["vk"], M, a["recs"], S, screened=True),
    "aggregate_verify_many_encoded": lambda bs, a, M, S: bs.aggregate_verify_many_encoded(a["vk"], M, a["recs"], S),
    "hash_ag_many_dev": lambda bs, a, M, S: bs.hash_ag_many_dev(a["vk"], M, S),
}


@pytest.mark.parametrize("name", sorted(MANY))
def test_device_form_downloads_no_c_hat_and_uploads_no_coefficients(name, monkeypatch):
    """under hash_ag="device" a many-committee call reaches fz_hash_ag_ragged_dev once, with the keys and c_hat where the challenge
    pass left them; no [N][d] array is downloaded before it or uploaded at all, and the host's hash_ag is not called"""
    from _scheme_buffers import MESSAGES, N, SIZES, host_inputs
    from fusion_hip import hostpipe
    params, ctx, bs = _stand_in(monkeypatch, "device")
    monkeypatch.setattr(hostpipe, "aggregation_coefficients", lambda *a, **k: pytest.fail("the host's hash_ag ran"))
    before = dict(ctx.ledger.live)
    result = MANY[name](bs, host_inputs(params), MESSAGES, SIZES)
    assert ctx.ledger.settle(before, result) == []
    d = params.degree
    entry = [c for c in ctx.calls if c[0] == "hash_ag_ragged_dev"]
    assert len(entry) == 1 and entry[0][5] == N, ctx.calls
    order, off = entry[0][6], entry[0][7]
    assert order[1] == (N,) and off[1] == (len(SIZES) + 1,)
    at = ctx.calls.index(entry[0])
    rows = ("int32", (N, d))
    assert not [c for c in ctx.calls[:at] if c[0] == "d2h" and c[2:] == rows], "c_hat was downloaded"
    assert not [c for c in ctx.calls if c[0] == "ntt_forward_dev"], "the coefficients were transformed outside the entry"
    if name != "hash_ag_many_dev":
        # against the same call in the host form: one download of [N][d] rows fewer (c_hat) and one upload fewer (the coefficients;
        # what verify_many uploads of that shape besides are the keys' halves, in both forms)
        _, host, hs = _stand_in(monkeypatch, "host")
        monkeypatch.undo()
        MANY[name](hs, host_inputs(params), MESSAGES, SIZES)
        count = lambda calls, kind, shape: sum(c[0] == kind and (c[2][:2] if kind == "h2d" else c[2:]) == shape for c in calls)    # noqa: E731
        assert count(ctx.calls, "d2h", rows) == count(host.calls, "d2h", rows) - 1
        assert count(ctx.calls, "h2d", rows) == count(host.calls, "h2d", rows) - 1
    assert [c for c in ctx.calls if c[0] == "h2d" and c[2][:2] == ("uint8", (N, 32))], "the prehashes were not uploaded"


@pytest.mark.parametrize("name", sorted(MANY))
def test_device_form_frees_every_buffer_when_the_entry_raises(name, monkeypatch):
    from _scheme_buffers import MESSAGES, SIZES, host_inputs
    from fusion_hip._lib import FZ_E_HIP, FusionHipError
    params, ctx, bs = _stand_in(monkeypatch, "device")

    def boom(*a, **k):
        raise FusionHipError(FZ_E_HIP, "injected")
    ctx.hash_ag_ragged_dev = boom
    before = dict(ctx.ledger.live)
    with pytest.raises(FusionHipError):
        MANY[name](bs, host_inputs(params), MESSAGES, SIZES)
    assert ctx.ledger.settle(before, None) == []


@pytest.mark.parametrize("name", sorted(k for k in MANY if k != "hash_ag_many_dev"))
def test_unsupported_falls_back_to_the_host_once_and_stays_there(name, monkeypatch):
    from _scheme_buffers import MESSAGES, SIZES, host_inputs
    params, ctx, bs = _stand_in(monkeypatch, "device")
    ctx.unsupported = ("hash_ag_ragged_dev",)
    before = dict(ctx.ledger.live)
    assert ctx.ledger.settle(before, MANY[name](bs, host_inputs(params), MESSAGES, SIZES)) == []
    assert bs.device_hash_ag is False and sum(c[0] == "hash_ag_ragged_dev" for c in ctx.calls) == 1
    assert [c for c in ctx.calls if c[0] == "ntt_forward_dev"], "the host form did not finish the call"
    del ctx.calls[:]
    assert ctx.ledger.settle(before, MANY[name](bs, host_inputs(params), MESSAGES, SIZES)) == []
    assert not [c for c in ctx.calls if c[0] == "hash_ag_ragged_dev"]


def test_host_form_is_the_default_and_makes_the_calls_it_made(monkeypatch):
    from _scheme_buffers import MESSAGES, SIZES, host_inputs
    params, ctx, bs = _stand_in(monkeypatch, "host")
    for name in sorted(k for k in MANY if k != "hash_ag_many_dev"):
        MANY[name](bs, host_inputs(params), MESSAGES, SIZES)
    assert not [c for c in ctx.calls if c[0] == "hash_ag_ragged_dev"]
