"""The fixtures of tests/_encoded_edges.py on the CPU: the context-parametric spec against the scheme's own spec and the golden
digests, the coverage the GPU module (tests/test_gpu_encoded_edges.py) rests on -- both multiply forms at both degrees, moduli
at or above 2^31 of both context kinds, every field width 2 .. 32 -- the canonicity of every decoder-side record, the exact
maxima of the encoder-side ones, and a replay of the kernels' arithmetic with fz_arith.h built for the host: mulacc16's step at
its operand bounds, and the forward passes with the 4-op multiply put in the 6-op form's place at a modulus that is not fast,
which changes the fixtures' expectations (so the kernels doing the same would be caught).  For the many-committee module
(tests/test_gpu_many_encoded_edges.py): the per-group spec against the single-group one, the sums of one sign at exactly
+-N_g (q - 1) / 2, and that module's own case lists held to the same coverage."""
import ctypes
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O

import _encoded_edges as X
import _transform_edges as E
from test_encoding_host import GOLDEN_OBJECTS, TABLE, golden_rows, spec_encode, spec_pack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(os.path.dirname(__file__), "golden")
SRC = r'''
#include "fz_arith.h"
extern "C" {
double t_mulacc(double a, double x, unsigned q) { FzMod m = fz_make_mod(q); return fz_cent(fz_mulmod(a, x, m), m); }
double t_mulmod(double a, double w, unsigned q) { FzMod m = fz_make_mod(q); return fz_mulmod(a, w, m); }
double t_mulmod4(double a, double w, unsigned q) { FzMod m = fz_make_mod(q); return fz_mulmod4(a, w, w * m.kq, m); }
int t_fast(unsigned q) { return fz_make_mod(q).fast; }
}
'''


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("encoded_edges")
    src = d / "t.cpp"
    src.write_text(SRC)
    so = d / "libt.so"
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I",
                           os.path.join(ROOT, "fusion-cryptography_amd", "csrc"), "-o", str(so), str(src)])
    L = ctypes.CDLL(str(so))
    for name in ("t_mulacc", "t_mulmod", "t_mulmod4"):
        getattr(L, name).restype = ctypes.c_double
        getattr(L, name).argtypes = [ctypes.c_double, ctypes.c_double, ctypes.c_uint]
    L.t_fast.argtypes = [ctypes.c_uint]
    return L


# ---- the spec on the scheme's own context ------------------------------------------------------------------------------------
@pytest.mark.parametrize("secpar", [128, 256])
def test_parametric_spec_equals_the_schemes_spec_on_the_golden_objects(secpar):
    spec, d = (secpar, "params"), O.PARAMS[secpar]["d"]
    with open(os.path.join(G, "encoding.json")) as fh:
        want = json.load(fh)[str(secpar)]
    for name, (kind, key) in GOLDEN_OBJECTS.items():
        rows, B, w, rb = TABLE[kind][secpar]
        r = golden_rows(secpar, key)
        assert X.width(B) == w and X.record_bytes(d, rows, w) == rb
        z = X.values(spec, d, r, kind != "vk")
        data, st = X.encoded(z, B)
        assert not st.any() and data.shape == (r.shape[0], rb)
        assert np.array_equal(data, spec_encode(secpar, kind, r)), (secpar, name)
        assert hashlib.sha3_256(data.tobytes()).hexdigest() == want[name], (secpar, name)
        back = X.decoded(spec, d, z, kind != "vk")
        assert np.array_equal(back, X.cent(r, X.modulus(spec)))              # decode(encode(rows)) == cent(rows)


# ---- what the GPU module's coverage rests on -----------------------------------------------------------------------------------
def test_contexts_cover_both_forms_both_kinds_and_every_width(lib):
    forms = {(n, E.mod_form(X.modulus(s))[2]) for s in X.SPECS for n in X.DEGREES}
    assert forms == {(64, True), (64, False), (256, True), (256, False)}
    for s in X.SPECS:
        assert lib.t_fast(X.modulus(s)) == int(E.mod_form(X.modulus(s))[2]), s
    wide = {s[1] == "root" for s in X.SPECS if X.modulus(s) >= 2 ** 31}
    assert wide == {True, False}                                               # a table and a root context at or above 2^31
    assert all(not E.mod_form(X.modulus(s))[2] for s in X.SPECS if X.modulus(s) >= 2 ** 31)
    assert {(k, "odd") for k in E.TABLE_MODULI} <= set(X.SPECS) and {(k, "root") for k in E.ROOT_MODULI} <= set(X.SPECS)
    assert {("d32767", "q1"), ("k17", "q1"), ("scheme", "q1"), ("top", "root")} <= set(X.SPECS)
    # the full-range bound of the widest moduli is a 32-bit field, of the scheme's prime a 31-bit one
    assert X.width(X.half(("w32", "odd"))) == X.width(X.half(("p31", "odd"))) == X.width(X.half(("top", "root"))) == 32
    assert X.width(X.half(("scheme", "root"))) == 31 and X.width(X.half(("q3", "odd"))) == 2
    # the sweep: every width, its smallest and largest bound, each on a fast and on a 6-op context where a fast one can hold it
    assert sorted({w for w, _ in X.SWEEP}) == list(range(2, 33)) and len(X.SWEEP) == 61
    for w, B in X.SWEEP:
        assert X.width(B) == w and (B == 1 << (w - 2) or B == (1 << (w - 1)) - 1)
        assert X.width(B - 1) < w or B > 1 << (w - 2) or w == 2               # the smallest of its width
        assert X.width(B + 1) > w or B < (1 << (w - 1)) - 1                    # the largest
        specs = X.sweep_specs(B)
        fast = {E.mod_form(X.modulus(s))[2] for s in specs}
        assert False in fast and (True in fast or w == 32), (w, B)
        if w <= 30 or B == 1 << 29:
            assert {s for s in specs if s[1] == "root"} == {("scheme", "root"), ("top", "root")}
    assert X.sweep_specs(1 << 30) == [("w32", "odd"), ("p31", "odd"), ("top", "root")]
    assert X.sweep_specs((1 << 31) - 1) == [("w32", "odd")]
    # the "top" context: q = 4294828033 with the root tests/test_gpu_generic_params.py finds at degree 256, its 4th power at 64
    q, r256, _ = X.root_of(("top", "root"), 256)
    q64, r64, i64 = X.root_of(("top", "root"), 64)
    assert q == q64 == 4294828033 and pow(r256, 256, q) == q - 1 and r64 == pow(r256, 4, q) and pow(r64, 64, q) == q - 1
    assert r64 * i64 % q == 1
    # degree 64, an odd width and an odd record count: the stream ends 8 bytes into a 16-byte unit
    assert all((c * X.record_bytes(64, r, 3)) % 16 == 8 for c in (1, 5) for r in (1, 3))
    assert X.record_bytes(64, 2, 31) % 16 == 0 and X.record_bytes(64, 1, 31) % 16 == 8


# ---- the records ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", X.DEGREES)
@pytest.mark.parametrize("spec", X.SPECS, ids=X.sid)
def test_decoder_records_are_canonical_and_one_past_is_not(spec, n):
    q, B = X.modulus(spec), X.half(spec)
    w = X.width(B)
    names, z = X.decoder_rows(spec, n)
    assert names[:2] == ["+B", "-B"] and len(names) == 2 + 2 * (n.bit_length() - 1) + 1
    assert np.abs(z).max() == B and (z[0] == B).all() and (z[1] == -B).all()
    assert all(abs(int(r.sum())) % 2 == 1 for r in z[2:-1])             # the stage patterns: an odd sum
    for per in (1, 2, 5):
        rec = X.records_of(z, per)
        assert rec.shape[0] * per >= z.shape[0] and rec.shape[1:] == (per, n)
        data, st = X.encoded(rec, B)
        assert not st.any() and np.array_equal(data, spec_pack(rec, B, w))
        for i in (0, rec.shape[0] - 1):
            assert X.canonical(data[i], B, (per, n))
            for j in (0, per * n // 2, per * n - 1):
                bad = X.one_past(data[i], j, B)
                assert bad is not None and 2 * B + 1 == q                      # q < 2^w whatever the modulus: q - 1 has w bits, q is odd
                assert X.get_field(bad, j, w) == q and not X.canonical(bad, B, (per, n))


@pytest.mark.parametrize("n", X.DEGREES)
@pytest.mark.parametrize("spec", X.SPECS, ids=X.sid)
def test_encoder_records_have_known_exact_maxima(spec, n):
    """bound = M encodes the record, bound = M - 1 refuses it, in the spec; for the coefficient kinds M is the norm of the
    reference inverse of int32-extreme rows, for keys of their centred values"""
    q = X.modulus(spec)
    rows = X.encoder_rows(spec, n)
    assert rows.min() == E.I32_MIN and rows.max() == E.I32_MAX
    for coef in (True, False):
        z = X.values(spec, n, rows[:, None, :], coef)
        assert np.abs(z).max() <= (q - 1) // 2
        if not coef:
            assert all(E.cent(int(v), q) == int(c) for v, c in zip(rows[:, 0], z[:, 0, 0]))
        for per in (1, 2, 5):
            rec = X.records_of(rows, per)
            zr = X.values(spec, n, rec, coef)
            M = X.maxima(zr)
            assert M.shape == (rec.shape[0],)
            for i, m in enumerate(M.tolist()):
                if m >= 1:
                    assert X.encoded(zr[i:i + 1], m)[1].tolist() == [0]
                if m >= 2:
                    data, st = X.encoded(zr[i:i + 1], m - 1)
                    assert st.tolist() == [4] and not data.any()
    if q > 3:
        assert len(set(X.maxima(X.values(spec, n, rows[:, None, :], True)).tolist())) > 1


def test_sweep_fields_hit_both_ends_of_every_record():
    for w, B in X.SWEEP[::7] + X.SWEEP[-2:]:
        for n in X.DEGREES:
            for rows in X.sweep_shapes(n):
                u = X.edge_fields(B, 5, rows, n, w).reshape(5, -1)
                assert u.min() == 0 and u.max() == 2 * B
                assert u[0, 0] == 0 and u[0, -1] == 2 * B and u[1, 0] == 2 * B and u[1, -1] == 0
                assert sorted({int(v) for v in u[:, rows * n // 2 + 3]}) == [0, 2 * B]
                z = (u - B).reshape(5, rows, n)
                data, st = X.encoded(z, B)
                assert not st.any() and data.shape == (5, X.record_bytes(n, rows, w))


def test_multipliers_carry_the_int32_extremes():
    for n in X.DEGREES:
        m = X.multipliers(67, n, 1)
        assert m.min() == E.I32_MIN and m.max() == E.I32_MAX and (m == -1).any()
        assert len({r.tobytes() for r in m}) > 30                              # ... and random rows
        vk, c = X.key_inputs(5, n, 2)
        assert vk.shape == (5, 2, n) and [int(v) for v in vk[0, :, 0]] + [int(c[0, 0])] == [E.I32_MIN, E.I32_MAX, E.I32_MAX]
        spec = ("top", "root")
        sums = X.cent(np.arange(5 * n).reshape(5, n) * 1234567891, X.modulus(spec))
        solved = X.solve_right_key(spec, vk, c, sums)
        assert np.array_equal(X.keyed_target(spec, solved, c), sums) and E.I32_MIN <= solved.min() and solved.max() <= E.I32_MAX
        assert X.verdicts(spec, sums, X.other_representative(sums, X.modulus(spec))).tolist() == [0] * 5
        moved = sums.copy()
        moved[3, n - 1] += 1
        assert X.verdicts(spec, sums, moved).tolist() == [0, 0, 0, 3, 0]


# ---- the many-committee fixtures (tests/test_gpu_many_encoded_edges.py) ----------------------------------------------------------
def test_group_partials_and_targets_are_the_single_group_spec_per_group():
    spec, n, l = ("top", "root"), 64, 2
    q = X.modulus(spec)
    z = X.records_of(X.decoder_rows(spec, n)[1], l, 5)[np.arange(9) % 5]
    alpha = X.multipliers(9, n, 1)
    vk, c = X.key_inputs(9, n, 2)
    assert np.array_equal(X.group_partials(spec, n, z, alpha, [9])[0], X.aggregate_partial(spec, n, z, alpha))
    skip = np.where(np.arange(9) % 3 == 0, 6, 0).astype(np.int32)
    keep = skip == 0
    got = X.group_partials(spec, n, z, alpha, [9], skip)
    assert got.shape == (1, l, n) and got.dtype == np.int64
    assert np.array_equal(got[0], X.aggregate_partial(spec, n, z[keep], alpha[keep])) and not np.array_equal(got[0], X.aggregate_partial(spec, n, z, alpha))
    # several groups: an empty one and one whose every signer is skipped give zeros, the others their own records' sums
    sizes, skip = [0, 4, 2, 3], np.array([0, 6, 0, 0, 3, 3, 0, 0, 6], dtype=np.int32)
    got, tgt = X.group_partials(spec, n, z, alpha, sizes, skip), X.group_targets(spec, vk, c, alpha, sizes, skip)
    assert got.shape == (4, l, n) and tgt.shape == (4, n) and tgt.dtype == np.int64
    assert not (got[0].any() or got[2].any() or tgt[0].any() or tgt[2].any())
    assert np.array_equal(got[1], X.aggregate_partial(spec, n, z[[0, 2, 3]], alpha[[0, 2, 3]]))
    assert np.array_equal(got[3], X.aggregate_partial(spec, n, z[[6, 7]], alpha[[6, 7]]))
    assert np.array_equal(X.group_partials(spec, n, z, alpha, sizes, np.full(9, 6))[1:], np.zeros((3, l, n), dtype=np.int64))
    # the targets in Python integers, signer by signer
    for g, members in ((1, [0, 2, 3]), (3, [6, 7])):
        for j in (0, n // 2, n - 1):
            want = sum(E.cent(E.cent(int(vk[i, 0, j]) * int(c[i, j]) + int(vk[i, 1, j]), q) * int(alpha[i, j]), q) for i in members)
            assert int(tgt[g, j]) == want
    assert np.array_equal(X.group_targets(spec, vk, c, alpha, [9])[0], X.group_targets(spec, vk, c, alpha, [4, 5]).sum(axis=0))


def test_same_sign_inputs_leave_the_largest_sums(lib):
    import test_gpu_many_encoded_edges as M
    assert M.SAME_SIGN_SPECS == [(k, "root") for k in E.ROOT_MODULI] + [("top", "root")]
    for spec in M.SAME_SIGN_SPECS:
        q, h = X.modulus(spec), X.half(spec)
        assert all(pow(a, q - 1, q) == 1 for a in (2, 3, 5, 7))
        for n in X.DEGREES:
            l, B, sizes = M._agg_ls(n)[1], M.SAME_SIGN_BOUNDS[n], [67, 1, 33]
            for sign in (1, -1):
                z, alpha = X.same_sign_inputs(spec, n, l, sum(sizes), B, sign)
                assert z.shape == (101, l, n) and np.abs(z).max() <= B and not X.encoded(z, B)[1].any()
                assert alpha.shape == (101, n) and E.I32_MIN <= alpha.min() and alpha.max() <= E.I32_MAX
                assert len({r.tobytes() for r in z[:, 0]}) == 5 and (z == z[:, :1]).all()
                got = X.group_partials(spec, n, z, alpha, sizes)
                for g, ng in enumerate(sizes):
                    assert (got[g] == sign * ng * h).all(), (spec, n, sign, g)
                assert np.array_equal(X.group_partials(spec, n, z[:67], alpha[:67], [67])[0], got[0])
                # one step of the kernels' sum, in their arithmetic: the product is exactly sign * h
                assert lib.t_mulacc(float(X.forward(spec, n, z[3, 0])[5]), float(alpha[3, 5]), q) == sign * h


def test_the_many_committee_cases_cover_both_forms_the_wide_moduli_and_every_width(lib):
    import test_gpu_many_encoded_edges as M
    assert sorted(M.CASES) == sorted((s, n) for s in X.SPECS for n in X.DEGREES) and len(M.CASES) == 38
    assert sorted(M.A_CASES) == sorted((s, n, l) for s, n in M.CASES for l in M._agg_ls(n))
    for n in X.DEGREES:
        specs = [s for s, d in M.CASES if d == n]
        assert {lib.t_fast(X.modulus(s)) for s in specs} == {0, 1}
        assert len({X.modulus(s) for s in specs if X.modulus(s) >= 2 ** 31}) >= 4
        assert {"odd", "q1", "root"} == {s[1] for s in specs}
        # odd tables and a root's on both forms; the top tables (every entry q - 1) are on fast moduli only
        assert {s[1] for s in specs if not lib.t_fast(X.modulus(s))} == {"odd", "root"}
    assert all(X.width(X.half(s)) < 32 for s in X.SPECS if lib.t_fast(X.modulus(s)))           # no fast modulus holds a 32-bit field
    # the seam: either form, either kind of context, either side of 2^31
    assert {(lib.t_fast(X.modulus(s)), s[1] == "root", X.modulus(s) >= 2 ** 31) for s in M.SEAM_SPECS} == \
        {(1, True, False), (0, True, True), (0, False, True), (1, False, False)}
    # the width sweep
    for n in X.DEGREES:
        reach = {0: set(), 1: set()}
        for s, d in M.SWEEP_CASES:
            if d == n:
                reach[lib.t_fast(X.modulus(s))] |= {w for w, B in X.SWEEP if s in X.sweep_specs(B)}
        assert reach[1] == set(range(2, 32)) and reach[0] == set(range(2, 33))
    assert set(M.MASKS) == {"none", "zeros", "thirds", "group", "all"} and [67, 1, 33] in M.SHAPES and [40, 1] in M.SHAPES
    for sizes in M.SHAPES:
        N = sum(sizes)
        assert M.mask_of("none", sizes) is None and not M.mask_of("zeros", sizes).any() and M.mask_of("all", sizes).all()
        g = M.mask_of("group", sizes)
        a, b = X.group_bounds(sizes)[int(np.argmax(sizes))]
        assert g[a:b].all() and int((g != 0).sum()) == b - a == max(sizes)
        assert (M.mask_of("thirds", sizes) != 0).tolist() == [i % 3 == 0 for i in range(N)]


# ---- the kernels' arithmetic on the host ---------------------------------------------------------------------------------------
REPLAY_MODULI = (2 ** 32 - 1, 2 ** 31 + 1, 2 ** 31 - 32769, E.PRIME)


def _forward_peak(q):
    """the largest |output| the forward passes leave over the decoder-side rows of the fixture contexts on q (both degrees)"""
    top = 0
    for spec in X.SPECS:
        if X.modulus(spec) == q:
            for n in X.DEGREES:
                _, fwd, _ = X.tables(spec, n)
                for z in X.decoder_rows(spec, n)[1]:
                    out, peak = X.lazy_forward(z, q, fwd)
                    assert [E.cent(v, q) for v in out] == O.py_ntt_forward([int(v) for v in z], q, fwd)
                    top = max(top, peak)
    return top


@pytest.mark.parametrize("q", REPLAY_MODULI)
def test_mulacc16_step_is_exact_at_its_operand_bounds(q, lib):
    """fz_cent(fz_mulmod(a, x)) == cent(a * x) for a = +-(2^38 - 1), the kernels' stated bound on a forward output, and at the
    largest output the fixtures leave, with the multipliers INT32_MIN, INT32_MAX and -1"""
    peak = _forward_peak(q)
    assert (q - 1) // 2 <= peak <= 9 * ((q - 1) // 2) < 2 ** 38               # |z| + log2(256) canonical products
    for a in (2 ** 38 - 1, -(2 ** 38 - 1), peak, -peak, peak - 1, 1 - peak):
        for x in (E.I32_MIN, E.I32_MAX, -1):
            got = lib.t_mulacc(float(a), float(x), q)
            assert got == int(got) and int(got) == E.cent(a * x, q), (q, a, x)


def test_the_four_op_multiply_in_place_of_the_six_op_one_changes_the_expectations(lib):
    """the mutation the GPU fixtures must catch: the forward passes of the decoder-side rows at 2^31 + 1 (K = 2^32, delta =
    2^31 - 1: not fast) with fz_mulmod as the twiddle multiply are the reference transform; with fz_mulmod4 in its place at
    least one row's outputs change.  At the scheme's prime (fast) the two forms agree on every row.  (2^31 + 1 is the sentinel:
    with operands below 2^35 here, |c| * delta stays under 2^53 for every other fixture modulus, whose 4-op form the rows of
    tests/_transform_edges.py defeat at degree 128 instead.)"""
    for spec, differs in ((("p31", "odd"), True), (("scheme", "root"), False)):
        q = X.modulus(spec)
        assert E.mod_form(q)[2] != differs
        changed = 0
        for n in X.DEGREES:
            _, fwd, _ = X.tables(spec, n)
            for z in X.decoder_rows(spec, n)[1]:
                want = O.py_ntt_forward([int(v) for v in z], q, fwd)
                six, _ = X.lazy_forward(z, q, fwd, lambda a, w: int(lib.t_mulmod(float(a), float(w), q)))
                assert [E.cent(v, q) for v in six] == want
                four, _ = X.lazy_forward(z, q, fwd, lambda a, w: int(lib.t_mulmod4(float(a), float(w), q)))
                changed += [E.cent(v, q) for v in four] != want
        assert (changed > 0) == differs, (spec, changed)


def test_the_range_test_model_is_the_spec_and_its_high_half_is_implied():
    """records_encode's test in its own 64-bit arithmetic refuses exactly |z| > B, at every bound the fixtures use and on both
    sides of every edge.  Dropping the `hi` half changes NO verdict for an int32 z and B < 2^31: for z < -B the low word is
    2^32 + z + B > 2B because z > B - 2^32.  No fixture can therefore tell that half's absence -- the other mutation (the test
    above) is the one the fixtures are shown to catch; both sides of the compare that does decide are pinned at M and M - 1."""
    bounds = sorted({1, 2, 2 ** 30 - 1, 2 ** 30, 2 ** 31 - 1} | {X.half(s) for s in X.SPECS} | {B for _, B in X.SWEEP})
    for B in bounds:
        for z in (-B - 1, -B, -B + 1, B - 1, B, B + 1, 0, E.I32_MIN, E.I32_MIN + 1, E.I32_MAX, -2 * B - 1, 2 * B + 1):
            if E.I32_MIN <= z <= E.I32_MAX:
                assert X.encoder_refuses(z, B) == (abs(z) > B) == X.encoder_refuses(z, B, hi=False), (B, z)
