"""The fixtures of tests/test_gpu_verdict_edges.py, checked on the host: their signatures have exactly the norm and weight they
claim, their targets and keys are consistent, and both oracles (the pure-Python restatement and the C one) flip their verdicts
exactly at beta = M and omega = W, in the reference's order (fusion.py:718-727).  Also the weight of stored values for small
moduli, where an int32 holds unreduced multiples of q (algebra/polynomials.py:226-227: x % q, not x != 0)."""
import numpy as np
import pytest

from oracle import oracle as O

import _verdict_edges as E


def _ones(d):
    return np.ones((1, d), dtype=np.int32)


def _cverdict(coracle, fx, g, beta, omega, vkR=None):
    vkR = fx.vkR if vkR is None else vkR
    return coracle.verify_core(fx.A, fx.sig[g], fx.vkL[g:g + 1], vkR[g:g + 1], fx.c[g:g + 1], _ones(fx.d), fx.q,
                               fx.P["inv_root"], beta, omega)


def _pyverdict(fx, g, beta, omega, vkR=None):
    vkR = fx.vkR if vkR is None else vkR
    q, d = fx.q, fx.d
    itw = O.py_twiddles(fx.P["inv_root"], q, d)
    rows = lambda a: [[int(v) for v in r] for r in np.asarray(a).reshape(-1, d)]       # noqa: E731
    return O.py_verify_core(rows(fx.A), rows(fx.sig[g]), rows(fx.vkL[g]), rows(vkR[g]), rows(fx.c[g]), rows(_ones(d)), q, itw,
                            beta, omega)


def _specs(d, l, M, W):
    last = l - 1
    return [dict(M=M, W=W, heavy=0, extreme=0, pos=0),
            dict(M=M, W=W, heavy=last, extreme=last, pos=d - 1, sign=-1),
            dict(M=M, W=W, heavy=last, extreme=0, pos=d // 2),
            dict(M=M, W=W, heavy=0, extreme=last, pos=1, sign=-1)]


@pytest.mark.parametrize("secpar", [128, 256])
def test_builder_gives_exact_norm_weight_and_consistent_targets(secpar, coracle):
    P = O.PARAMS[secpar]
    q, d = P["q"], P["d"]
    for l, M, W in ((3, 3172, d // 2 + 1), (P["rank"], 536321760, d - 1), (5, (q - 1) // 2, d), (4, E.lazy_beta_max(q) + 1, 2)):
        fx = E.build(P, l, _specs(d, l, M, W), 10 * l + secpar, coracle)
        assert np.array_equal(coracle.ntt_inverse(fx.sig.reshape(-1, d), q, P["inv_root"]).reshape(fx.z.shape), fx.z)
        assert fx.M.tolist() == [M] * fx.G and fx.W.tolist() == [W] * fx.G
        for g, s in enumerate(_specs(d, l, M, W)):
            assert fx.z[g, s["extreme"], s["pos"]] == s.get("sign", 1) * M
            wt = (fx.z[g] != 0).sum(axis=1)
            assert wt[s["heavy"]] == W and (np.delete(wt, s["heavy"]) < W).all()
        assert np.array_equal(fx.target, coracle.matvec(fx.A, fx.sig, q).reshape(fx.G, d))
        L, R, C, T = (a.astype(object) for a in (fx.vkL, fx.vkR, fx.c, fx.target))     # exact Python integers
        assert ((L * C + R - T) % q == 0).all()
        for a in (fx.vkL, fx.vkR, fx.c):
            assert a.dtype == np.int32
        ext = np.concatenate([fx.vkL.ravel(), fx.vkR.ravel(), fx.c.ravel()])
        assert {E.I32_MIN, E.I32_MAX} <= set(ext.tolist())                               # the keyed form's extremes are in


@pytest.mark.parametrize("secpar", [128, 256])
def test_oracles_flip_exactly_at_the_bounds(secpar, coracle):
    P = O.PARAMS[secpar]
    d = P["d"]
    M, W = 4264, d // 2
    fx = E.build(P, 3, _specs(d, 3, M, W), 7 + secpar, coracle)
    for g in range(fx.G):
        for beta in (M - 1, M, M + 1):
            for omega in (W - 1, W, W + 1):
                want = E.expect(M, W, False, beta, omega)
                assert _cverdict(coracle, fx, g, beta, omega) == want, (g, beta, omega)
        assert [_pyverdict(fx, g, M, W), _pyverdict(fx, g, M - 1, W), _pyverdict(fx, g, M, W - 1)] == [0, 4, 5], g
    # the flags at the scheme rank, through the C oracle
    l = P["rank"]
    fx = E.build(P, l, _specs(d, l, M, W), 70 + secpar, coracle)
    for g in range(fx.G):
        assert [_cverdict(coracle, fx, g, b, o) for b, o in ((M, W), (M - 1, W), (M, W - 1), (M - 1, W - 1), (M, d))] == \
            [0, 4, 5, 4, 0], g


@pytest.mark.parametrize("secpar", [128, 256])
def test_reference_verdict_order(secpar, coracle):
    """a mismatch that also breaks norm and weight is 3; norm and weight together are 4"""
    P = O.PARAMS[secpar]
    d = P["d"]
    M, W = 100, 9
    fx = E.build(P, 3, _specs(d, 3, M, W), 3 + secpar, coracle)
    _, badR = fx.tampered(range(fx.G))
    for g in range(fx.G):
        assert _cverdict(coracle, fx, g, M - 1, W - 1, vkR=badR) == 3
        assert _pyverdict(fx, g, M - 1, W - 1, vkR=badR) == 3
        assert _cverdict(coracle, fx, g, M, W, vkR=badR) == 3
        assert _cverdict(coracle, fx, g, M - 1, W - 1) == 4 == _pyverdict(fx, g, M - 1, W - 1)
        assert _cverdict(coracle, fx, g, M, W - 1) == 5
    assert E.expect([M, M, M, M], [W] * 4, [True, False, False, False], M - 1, [W - 1, W - 1, W, W - 1]) == [3, 4, 4, 4]


def test_lazy_threshold_is_the_launchers_fp64_compare():
    """launch_verify_fused skips centring iff (double)beta < 0.5 * q - q / 4096.0: lazy_beta_max is the last beta that does"""
    for q in (O.PRIME, 3, 17, 12289, 1073741789, 4294967291, 2 ** 31 - 1):
        b = E.lazy_beta_max(q)
        assert float(b) < 0.5 * q - q / 4096.0
        assert not float(b + 1) < 0.5 * q - q / 4096.0


def test_degenerate_fixtures(coracle):
    """an all-zero signature (M = W = 0) and one with a single non-zero coefficient: the bounds 0 flip exactly there too"""
    P = O.PARAMS[128]
    d = P["d"]
    fx = E.build(P, 3, [dict(M=0, W=0), dict(M=1, W=1, heavy=2, extreme=2, pos=d - 1, sign=-1)], 5, coracle)
    assert fx.M.tolist() == [0, 1] and fx.W.tolist() == [0, 1]
    assert [_cverdict(coracle, fx, 0, 0, 0), _cverdict(coracle, fx, 1, 0, 1), _cverdict(coracle, fx, 1, 1, 0),
            _cverdict(coracle, fx, 1, 1, 1)] == [0, 4, 5, 0]
    assert _pyverdict(fx, 0, 0, 0) == 0 and _pyverdict(fx, 1, 1, 0) == 5


@pytest.mark.parametrize("q", E.SMALL_MODULI)
def test_small_modulus_weight_counts_residues(q, coracle):
    """weight() counts x % q != 0 over the STORED values: an unreduced multiple of q (2q, -3q, ..) weighs nothing"""
    rows = E.small_modulus_rows(q, 64, q % 1000)
    mx, wt = coracle.norm_weight(rows, q)
    pm, pw = E.py_norm_weight(rows, q)
    assert mx.tolist() == pm and wt.tolist() == pw
    assert pw[0] == 0 and all(w == 0 for w in pw[:-6])                 # the multiples-only rows
    if q < 2 ** 30:
        assert max(pm[:-6]) >= 2 * q                                   # ... hold multiples beyond +-q
    assert pw[-5] == 1 and pw[-4] == 1
