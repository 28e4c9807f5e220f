"""The fixtures of tests/test_gpu_saturation.py, checked on the host: their closed-form expectations equal the C oracle and a
Python-integer computation, and each one is adversarial -- without the fold or guard it targets, the exact arithmetic the
kernel would then do (tests/_saturation.py's models of its per-lane sums) gives a different result mod q.  A fixture that
stops being adversarial fails here, not silently on the GPU.  The shapes are modelled at the MI355X's 256 CUs; the GPU test
checks the same claims at the device's own count."""
import numpy as np
import pytest

from oracle import oracle as O

import _saturation as S

CU = 256
Q = O.PRIME
MODULI = (Q, S.Q_WIDE)


def _py_agg(sig, alpha, q):
    """cent(sum_i sig_i * alpha_i) in Python integers, [l][d]"""
    n, l, d = sig.shape
    out = np.empty((l, d), dtype=np.int64)
    for k in range(l):
        for j in range(d):
            out[k, j] = S.cent(sum(int(sig[i, k, j]) * int(alpha[i, j]) for i in range(n)), q)
    return out


def _py_matvec(A, Srows, q):
    l, d = A.shape
    return np.array([S.cent(sum(int(A[k, j]) * int(Srows[k, j]) for k in range(l)), q) for j in range(d)], dtype=np.int64)


@pytest.mark.parametrize("q", MODULI)
@pytest.mark.parametrize("n", [1, 15, 16, 17, 49, 65, 129])
def test_aggregation_closed_form(n, q, coracle):
    d, l = 24, 2
    sig, alpha = S.agg_inputs(n, l, d)
    want = S.agg_expected(n, l, d, q)
    assert np.array_equal(_py_agg(sig, alpha, q), want)
    if q == Q:
        assert np.array_equal(coracle.aggregate_core(sig, alpha, q), want)
    vkL, vkR, c = S.target_inputs(n, d)
    t = [S.cent(sum((int(vkL[i, j]) * int(c[i, j]) + int(vkR[i, j])) * int(alpha[i, j]) for i in range(n)), q) for j in range(d)]
    assert S.target_expected(n, d, q).tolist() == t
    sk, ch, sg = S.sign_inputs(n, l, d, q)
    for i in range(n):
        for k in range(l):
            for j in range(d):
                assert sg[i, k, j] == S.cent(S.cent(int(sk[i, 0, k, j]) * int(ch[i, j]), q) + int(sk[i, 1, k, j]), q)
    assert np.array_equal(S.sign_agg_expected(n, l, d, q), _py_agg(sg, alpha, q))
    # the fixture holds the extremes it claims
    assert {S.I32_MIN, S.I32_MAX, S.I32_MIN + 1} <= set(sig.ravel().tolist())
    assert {-1, S.I32_MIN, S.I32_MAX, S.HI_ODD} <= set(alpha.ravel().tolist())


@pytest.mark.parametrize("secpar", [128, 256])
def test_sign_closed_form_against_the_oracle(secpar, coracle):
    P = O.PARAMS[secpar]
    q, d = P["q"], P["d"]
    sk, ch, sg = S.sign_inputs(3, 2, d, q)
    assert np.array_equal(coracle.sign_core(sk, ch, q).reshape(sg.shape), sg)


@pytest.mark.parametrize("q", MODULI)
@pytest.mark.parametrize("l", [1, 2, 32, 33, 100, 101])
def test_matvec_closed_form(l, q, coracle):
    d = 18
    A, Sb = S.mv_inputs(l, d, batch=2)
    want = S.mv_expected(l, d, q)
    assert _py_matvec(A, Sb[0], q).tolist() == want.tolist()
    if q == Q:
        assert np.array_equal(coracle.matvec(A, Sb, q), np.stack([want, want]))


@pytest.mark.parametrize("secpar", [128, 256])
def test_keygen_impulse_transform_is_constant(secpar, coracle):
    """NTT([v, 0, .., 0]) = v in every coefficient: keygen's y saturates the centred range in every row"""
    P = O.PARAMS[secpar]
    q, d = P["q"], P["d"]
    v = S.odd_half_q(q)
    assert v % 2 == 1 and v in ((q - 1) // 2, (q - 3) // 2)
    for l in (1, 3):
        coef = S.impulse_rows(2, l, d, v)
        A = S.keygen_A(l, d)
        sk, vk = coracle.keygen_core(A, coef, q, P["root"])
        assert (sk[:, 0] == v).all() and (sk[:, 1] == -v).all()
        assert np.array_equal(vk, np.broadcast_to(S.keygen_expected(l, d, q, v), vk.shape))
    # ... and the closed form at a long l equals the sum in Python integers
    l = 2064
    Acol, _ = S.mv_row_values(1)
    want = S.keygen_expected(l, d, q, v)
    for j in range(min(d, 2 * S.NMV)):
        assert want[0, j] == S.cent(sum(int(Acol[j % S.NMV]) * v for _ in range(l)), q)


@pytest.mark.parametrize("secpar", [128, 256])
def test_i64_rows_closed_form(secpar, coracle):
    P = O.PARAMS[secpar]
    q, d = P["q"], P["d"]
    l = 5
    A, _ = S.mv_inputs(l, d)
    rows = S.i64_rows(l, d)
    assert {S.I64_MIN, S.I64_MAX} <= set(rows.ravel().tolist())
    cent = np.array([[S.cent(int(x), q) for x in r] for r in rows], dtype=np.int32)
    assert np.array_equal(coracle.matvec(A, cent, q).reshape(d), S.i64_expected(A, l, d, q))
    t = S.i64_expected(A, l, d, q)
    for top in (True, False):
        far = [S.far_representative(x, q, top) for x in t]
        assert all(S.I64_MIN <= f <= S.I64_MAX and (f - int(x)) % q == 0 for f, x in zip(far, t))
        assert min(abs(f - (S.I64_MAX if top else S.I64_MIN)) for f in far) < q


# ---- each fixture is adversarial for the bound it targets ----------------------------------------------------------------
def _lo_patterns():
    return [i for i, p in enumerate(S.AGG_PATTERNS) if p[0] in ("lo+", "lo-", "both+")]


def test_onepass_fixture_defeats_a_missing_fold():
    """257 aggregates of 520 signers at degree 64, l = 1 (and 129 with the target columns): more tiles than CUs at the widest
    block, so one slice per aggregate and 65 signers per lane -- 65 odd products near 2^47 pass 2^53: without the in-loop fold
    the fp64 sums round"""
    for groups, target in ((257, False), (129, True)):
        ar, nsl = S.onepass_shape(CU, groups, 520, 1, 64, target=target)
        assert nsl == 1, (groups, target)
        lanes = S.onepass_lanes(520, nsl)
        assert S.max_lane_products(lanes) == 65 > S.AGG_FOLD
        for p in _lo_patterns():
            assert S.agg_max_lane_sum(lanes, p, 520) > 2 ** 53
            assert S.agg_fold_free_error(lanes, p, 520) % Q != 0, S.AGG_PATTERNS[p][0]
    # with the fold, every lane sum stays below 2^51 + 2^47 (the bound the kernel documents)
    assert S.AGG_FOLD * 2 ** 31 * 2 ** 16 == 2 ** 51


def test_direct_fixture_defeats_a_missing_fold():
    """aggregate_direct, one aggregate of 4145 signers: 32 lane groups of 129-130 signers; the lo columns pass 2^53 after 65,
    the odd hi columns (|x * hi| ~ 2^46) after 129"""
    n = 4145
    lanes = S.direct_lanes(n)
    assert len(lanes) == 32 and S.max_lane_products(lanes) == 130
    names = [p[0] for p in S.AGG_PATTERNS]
    for name in ("lo+", "lo-", "both+", "hi_odd-", "hi_odd+", "mixed"):
        p = names.index(name)
        assert S.agg_fold_free_error(lanes, p, n) % Q != 0, name
    for name in ("lo_even", "hi_even", "hi_min"):          # even products: exact in fp64 at any length here (not adversarial)
        assert S.agg_fold_free_error(lanes, names.index(name), n) == 0, name


def test_cadence_counts_reach_the_fold():
    """the GPU test's signer counts put 15 .. 17 products into one lane's sum around the fold, per kernel: 32 signers per
    round in aggregate_direct; 8 per round in aggregate_onepass once there is one slice per aggregate (257 aggregates at degree
    64, l = 1) -- one aggregate is cut into slices of 24 or more signers instead"""
    for k in (15, 16, 17):
        assert S.max_lane_products(S.direct_lanes(k * 32)) == k
        ar, nsl = S.onepass_shape(CU, 257, 8 * k, 1, 64)
        assert nsl == 1 and S.max_lane_products(S.onepass_lanes(8 * k, nsl)) == k
    assert S.onepass_shape(CU, 1, 129, 3, 256)[1] == 5
    ar, nsl = S.onepass_shape(CU, 1, 300, 83, 256)
    assert nsl > 1                                             # shared accumulator words


def test_matvec_fixture_defeats_small_and_the_guard():
    Q32 = Q
    odd = [p[0] for p in S.MV_PATTERNS].index("lo_odd")
    # `small` (l <= 32): at l = 32 / 33 every total is exact in fp64 anyway; at 100 and 32768 the odd column's is not
    for l in (32, 33):
        assert not any(S.inexact_in_fp64(h) or S.inexact_in_fp64(lo) for h, lo in S.mv_totals(l))
    for l in (100, 32768):
        h, lo = S.mv_totals(l)[odd]
        assert abs(lo) > 2 ** 53 and S.inexact_in_fp64(lo)
        err = 65536 * (int(float(h)) - h) + (int(float(lo)) - lo)
        assert err % Q32 != 0
    # the integer form's guard (l <= 32768): |y * lo| <= 2^31 * 0xffff = 2^47 - 2^31, so an int64 sum of 65537 of them still
    # fits (2^63 - 2^31); 65538 do not
    assert not any(S.outside_int64(h) or S.outside_int64(lo) for h, lo in S.mv_totals(65537))
    h, lo = S.mv_totals(65538)[[p[0] for p in S.MV_PATTERNS].index("lo_min")]
    assert S.outside_int64(lo) and ((lo + 2 ** 63) % 2 ** 64 - 2 ** 63 - lo) % Q32 != 0
    # which knobs take the sliced kernel at a batch of 3
    for d in (64, 256):
        assert [k for k in (-1, 0, 1, 2, 4, 8, 16) if S.matvec_sliced_taken(k, 3, 100, d, CU)] == [1, 2, 4, 8, 16]
        assert not any(S.matvec_sliced_taken(k, 3, 65538, d, CU) for k in (-1, 0, 1, 2, 4, 8, 16))
        assert [k for k in (-1, 0, 1, 2, 4, 8, 16) if S.matvec_sliced_taken(k, 3, 65538, d, CU, guard=False)] == [1, 2, 4, 8, 16]


@pytest.mark.parametrize("d,l_edge,l_long", [(64, 512, 2064), (256, 128, 516)])
def test_keygen_fixture_defeats_small(d, l_edge, l_long):
    """keygen_fused's `small` (tasks <= 32 * 4 waves): exact at the edge and one above it; at l_long a lane holds 129
    products of |y| * 0xffff ~ 2^46, past 2^53"""
    v = S.odd_half_q(Q)
    assert S.keygen_small(l_edge, d) and not S.keygen_small(l_edge + 1, d) and not S.keygen_small(l_long, d)
    assert S.max_lane_products(S.keygen_lanes(l_edge, d)[1]) == 32
    assert S.max_lane_products(S.keygen_lanes(l_long, d)[1]) == 129
    assert all(S.keygen_lane_error(l_edge + 1, d, Q, v, p) == 0 for p in range(S.NMV))
    assert S.keygen_lane_error(l_long, d, Q, v, 0) % Q != 0


def test_verify_fixture_defeats_small():
    """verify_fused's `small` (tasks <= 32 * 4R): one aggregate of 16640 rows at degree 256 runs 64 workgroups of 4 waves, 65
    rows per lane, in the integer form -- 65 odd products near 2^47"""
    R, imad, small, lanes = S.verify_shape(16640, 256, 2, CU)
    assert (R, imad, small, S.max_lane_products(lanes)) == (64, True, False, 65)
    assert S.imad_small_error(lanes, 16640, 0) % Q != 0
    for l, want_small in ((8192, True), (8193, False)):
        R, imad, small, lanes = S.verify_shape(l, 256, 1, CU)
        assert imad and small == want_small
    R, imad, small, lanes = S.verify_shape(32768, 64, 1, CU)
    assert imad and small and S.max_lane_products(lanes) == 32
    assert not S.verify_shape(32769, 64, 1, CU)[1]          # beyond 2^15 rows: the fp64 form
    assert not S.verify_shape(8193, 256, 1, CU, no_imad=True)[1]


@pytest.mark.parametrize("secpar", [128, 256])
def test_verify_rows_fail_the_norm(secpar, coracle):
    """the saturating signature rows fail the norm bound (so the verdict with the exact target is 4, never 3): every kind of
    row the fixture holds -- row 0, an odd and an even row of the first half, and the last row"""
    P = O.PARAMS[secpar]
    q, d = P["q"], P["d"]
    l = 101
    _, Sb = S.mv_inputs(l, d)
    rows = Sb[0][[0, 1, 2, l - 1]]
    mx, _ = coracle.norm_weight(coracle.ntt_inverse(rows, q, P["inv_root"]), q)
    assert (mx > P["beta_vf"]).all()
    cent = np.array([[S.cent(int(x), q) for x in S.i64_rows(1, d)[0]]], dtype=np.int32)
    mx, _ = coracle.norm_weight(coracle.ntt_inverse(cent, q, P["inv_root"]), q)
    assert (mx > P["beta_vf"]).all()
