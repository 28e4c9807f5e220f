"""The verdict predicates pinned where they flip, on every path that produces a verdict.  The reference rejects when
norm("infty") > beta_vf or weight() > omega_vf (algebra/polynomials.py:221-227, fusion/fusion.py:718-728); the kernels' arithmetic
is checked elsewhere, this module checks the compares: signatures of exactly known norm M and weight W (tests/_verdict_edges.py)
against beta in {M-1, M, M+1} and omega in {W-1, W, W+1}, through the fused kernel's int32, int64-partial and keyed forms,
verify_core, and the multi-launch path (norm_weight_kernel + verdict_kernel), under every knob that changes how verify_fused
compares; then the scheme's faces at the measured bounds of an honest aggregate, and norm / weight of stored values for small
moduli, where an int32 holds unreduced multiples of q."""
import copy
import os

import numpy as np
import pytest

from oracle import oracle as O

import _verdict_edges as E

pytestmark = pytest.mark.gpu

KNOBS = [
    {},
    {"FZ_VERIFY_CENT": "1"},
    {"FZ_NO_IMAD": "1"},
    {"FZ_VERIFY_ORDERED": "1"},
    {"FZ_UNFUSED": "1"},                       # verify_with_target / verify_core take the multi-launch path
]
_FIXTURES = {}


def _ident(env):
    return ",".join(f"{k[3:]}={v}" for k, v in env.items()) or "defaults"


def _ctx(P, env):
    import fusion_hip
    for k, v in env.items():
        os.environ[k] = v
    try:
        return fusion_hip.Context(P["q"], P["d"], P["root"], P["inv_root"])
    finally:
        for k in env:
            os.environ.pop(k, None)


def _num_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _around(M0, W0):
    """(M, W) of nine aggregates: every pair of M0 + {-1, 0, 1} and W0 + {-1, 0, 1}"""
    return [(M0 + a, W0 + b) for a in (-1, 0, 1) for b in (-1, 0, 1)]


def _fixtures(P, coracle):
    """named Fixtures at one parameter set (built once per module)"""
    key = (P["q"], P["d"], P["rank"])
    if key in _FIXTURES:
        return _FIXTURES[key]
    q, d, rank = P["q"], P["d"], P["rank"]
    M0, W0 = 4264, d // 2 + 1
    out = {}
    # l = 3: one workgroup per aggregate (R == 1); extreme coefficient and heaviest row first and last
    l = 3
    out["small"] = E.build(P, l, [dict(M=M, W=W, heavy=(0, l - 1)[i % 2], extreme=(0, l - 1)[(i // 2) % 2],
                                        pos=(0, d - 1, d // 2)[i % 3], sign=(1, -1)[i % 2])
                                   for i, (M, W) in enumerate(_around(M0, W0) + _around(M0, W0)[:3])], 11, coracle)
    # one rank that spreads an aggregate over many workgroups (cross-workgroup combine): 83 rows at degree 256 (R = 21), 195
    # at degree 64 (R = 13, four rows per wave); the heaviest row in each of the four row slots of a wave and in row l - 1,
    # which sits in a partial last task at degree 64 (195 = 48 * 4 + 3: the padding slot repeats it)
    l = 83 if d == 256 else 195
    place = [(0, 0), (l - 1, l - 1), (4, 7), (5, 6), (6, 5), (7, 4), (l - 1, 0), (0, l - 1), (l - 2, l - 3)]
    out["cross"] = E.build(P, l, [dict(M=M, W=W, heavy=h, extreme=x, pos=(d - 1) * (i % 2), sign=(1, -1)[i % 2])
                                  for i, ((M, W), (h, x)) in enumerate(zip(_around(M0, W0), place))], 12, coracle)
    # 2 * CUs + 1 aggregates at the scheme rank: one workgroup each again (R == 1), many rows per wave
    G = 2 * _num_cu() + 1
    pairs = _around(M0, W0)
    out["many"] = E.build(P, rank, [dict(M=pairs[g % 9][0], W=pairs[g % 9][1], heavy=(g * 7) % rank, extreme=(g * 13) % rank,
                                         pos=(g * 5) % d, sign=(1, -1)[g % 2]) for g in range(G)], 13, coracle)
    # the lazy norm test's threshold T: rows with M just below, at and just above it, and +-(q - 1) / 2, every coefficient of
    # the same order (spread = M): the inverse transform's raw outputs sit near +-q/2 there
    T, H = E.lazy_beta_max(q), (q - 1) // 2
    out["lazy"] = E.build(P, 3, [dict(M=M, W=W, heavy=h, extreme=x, pos=p, sign=s)
                                 for M in (T - 1, T, T + 1, T + 2, H - 1, H) for (W, h, x, p, s) in ((d, 0, 2, d - 1, 1), (d - 2, 2, 0, 0, -1))],
                          14, coracle)
    # degenerate: all-zero, one non-zero coefficient (first / last), a dense row at the largest magnitude
    out["degenerate"] = E.build(P, 3, [dict(M=0, W=0), dict(M=1, W=1, heavy=2, extreme=2, pos=d - 1, sign=-1),
                                       dict(M=1, W=1, heavy=0, extreme=0, pos=0), dict(M=H, W=d, heavy=1, extreme=1, pos=3)],
                                15, coracle)
    _FIXTURES[key] = out
    return out


class _Dev:
    """one Fixture's device buffers on one context; aggregates g % 4 == 3 get a tampered target (verdict 3 whatever the bounds)"""

    def __init__(self, ctx, fx, fused):
        import fusion_hip
        DA = fusion_hip.DeviceArray
        self.ctx, self.fx, self.fused = ctx, fx, fused
        rng = np.random.default_rng(fx.G + fx.l)
        self.mis = np.arange(fx.G) % 4 == 3
        tgt, vkR = fx.tampered(np.flatnonzero(self.mis))
        arrays = [fx.A, fx.sig, tgt, np.stack([fx.vkL, vkR], axis=1), fx.c]
        if fused:        # int64 partials: the same values shifted by multiples of q
            arrays += [fx.sig.astype(np.int64) + fx.q * rng.integers(-500, 500, size=fx.sig.shape),
                       tgt.astype(np.int64) + fx.q * rng.integers(-500, 500, size=tgt.shape)]
        self.bufs = [DA.from_numpy(ctx, np.ascontiguousarray(a)) for a in arrays]
        self.dV = DA(ctx, (fx.G,))
        # verify_core, one signer with alpha_hat == 1, the honest target: for the first aggregates only
        self.core = [[DA.from_numpy(ctx, np.ascontiguousarray(a)) for a in (fx.sig[g], fx.vkL[g:g + 1], fx.vkR[g:g + 1], fx.c[g:g + 1])]
                     for g in range(min(fx.G, 4))]
        self.ones = DA.from_numpy(ctx, np.ones((1, fx.d), dtype=np.int32))

    def verdicts(self, beta, omega):
        """-> {path: verdict list} for these bounds"""
        ctx, fx = self.ctx, self.fx
        dA, dS, dT, dK, dC = self.bufs[:5]
        out = {"target": ctx.verify_with_target_batch_dev(dA.ptr, dS.ptr, dT.ptr, fx.G, fx.l, beta, omega)}
        if self.fused:
            d64, dT64 = self.bufs[5:]
            ctx.verify_partials_batch_async_dev(dA.ptr, d64.ptr, fx.l * fx.d, dT64.ptr, fx.d, fx.G, fx.l, beta, omega, self.dV.ptr)
            out["partials"] = self.dV.numpy().tolist()
            ctx.verify_signatures_async_dev(dA.ptr, dS.ptr, dK.ptr, dC.ptr, fx.G, fx.l, beta, omega, self.dV.ptr)
            out["keyed"] = self.dV.numpy().tolist()
        out["core"] = [ctx.verify_core_dev(dA.ptr, s.ptr, L.ptr, R.ptr, c.ptr, self.ones.ptr, 1, fx.l, beta, omega)
                       for s, L, R, c in self.core]
        return out

    def expected(self, beta, omega):
        fx = self.fx
        want = E.expect(fx.M, fx.W, self.mis, beta, omega)
        return {"target": want, "partials": want, "keyed": want, "core": E.expect(fx.M, fx.W, False, beta, omega)[:len(self.core)]}

    def check(self, beta, omega, tag):
        got, want = self.verdicts(beta, omega), self.expected(beta, omega)
        for path, v in got.items():
            assert v == want[path], (tag, path, beta, omega, np.flatnonzero(np.array(v) != np.array(want[path])).tolist()[:8])

    def free(self):
        for b in self.bufs + [self.dV, self.ones] + [x for row in self.core for x in row]:
            b.free()


def _sweep(ctx, fx, fused, bounds, tag):
    dev = _Dev(ctx, fx, fused)
    try:
        for beta, omega in bounds:
            dev.check(beta, omega, tag)
    finally:
        dev.free()


@pytest.mark.parametrize("env", KNOBS, ids=_ident)
@pytest.mark.parametrize("secpar", [128, 256])
def test_verdicts_flip_exactly_at_the_bounds(secpar, env, coracle):
    P = O.PARAMS[secpar]
    q, d = P["q"], P["d"]
    fx = _fixtures(P, coracle)
    ctx = _ctx(P, env)
    M0, W0 = 4264, d // 2 + 1
    grid = [(M0 + a, W0 + b) for a in (-1, 0, 1) for b in (-1, 0, 1)]
    try:
        for name in ("small", "cross", "many"):
            _sweep(ctx, fx[name], True, grid + [(M0, d), (M0 + 1, d - 1)], name)
        T, H = E.lazy_beta_max(q), (q - 1) // 2
        lazy = [(b, w) for b in (T - 1, T, T + 1, T + 2, H - 2, H - 1) for w in (d - 2, d - 1, d)]
        _sweep(ctx, fx["lazy"], True, lazy + [(H, d), (H + 1, d - 3), (2 ** 40, d)], "lazy")
        _sweep(ctx, fx["degenerate"], True, [(b, w) for b in (0, 1, H - 1, H) for w in (0, 1, d - 1, d, d + 1)], "degenerate")
    finally:
        ctx.close()


@pytest.mark.parametrize("degree", [32, 128])
def test_multi_launch_degrees(degree, coracle):
    """degrees without a fused kernel: verify_with_target and verify_core always take matvec + transform + norm_weight_kernel +
    verdict_kernel"""
    P0 = O.PARAMS[256]
    q = P0["q"]
    root = pow(P0["root"], 256 // degree, q)                  # a primitive 2 * degree-th root of unity
    P = dict(q=q, d=degree, root=root, inv_root=pow(root, q - 2, q), rank=5)
    M0, W0 = 4264, degree // 2 + 1
    fx = E.build(P, 5, [dict(M=M, W=W, heavy=(0, 4)[i % 2], extreme=(4, 0)[i % 2], pos=(0, degree - 1)[(i // 2) % 2],
                             sign=(1, -1)[i % 2]) for i, (M, W) in enumerate(_around(M0, W0))], 16, coracle)
    T, H = E.lazy_beta_max(q), (q - 1) // 2
    big = E.build(P, 2, [dict(M=M, W=degree, heavy=1, extreme=0, pos=1) for M in (T, T + 1, H)] +
                  [dict(M=0, W=0), dict(M=1, W=1, heavy=1, extreme=1, pos=degree - 1, sign=-1)], 17, coracle)
    ctx = _ctx(P, {})
    try:
        _sweep(ctx, fx, False, [(M0 + a, W0 + b) for a in (-1, 0, 1) for b in (-1, 0, 1)] + [(M0, degree)], "multi")
        _sweep(ctx, big, False, [(b, w) for b in (0, 1, T, T + 1, H - 1, H) for w in (0, 1, degree - 1, degree)], "multi-big")
    finally:
        ctx.close()


# ---- the scheme's faces ----------------------------------------------------------------------------------------------------
_SCHEME = {}


def _honest(secpar):
    import fusion.fusion as F
    from fusion_hip.scheme import BatchScheme
    if secpar not in _SCHEME:
        params = F.fusion_setup(secpar, 3000 + secpar)
        bs = BatchScheme(params, threads=4)
        n = 10
        seeds = [9000 + secpar + 3 * i for i in range(n)]
        msgs = [f"edge-{secpar}-{i}" for i in range(n)]
        sk, vk = bs.keygen_batch(seeds)
        sig = bs.sign_batch(sk, vk, msgs)
        _SCHEME[secpar] = (params, bs, vk, msgs, sig)
    return _SCHEME[secpar]


def _bounded(params, beta, omega):
    p = copy.copy(params)
    p.beta_vf, p.omega_vf = beta, omega
    return p


@pytest.mark.parametrize("secpar", [128, 256])
def test_scheme_verify_at_the_measured_bounds_of_an_honest_aggregate(secpar, coracle):
    """BatchScheme.verify, verify_many, the drop-in verify and the batch queue accept at beta_vf = M (omega_vf = W) and return
    the reference's strings at M - 1 and W - 1, M / W measured from the aggregate itself"""
    import fusion.fusion as F
    from fusion_hip.queue import BatchQueue
    from fusion_hip.scheme import BatchScheme, signature_to_object, vk_to_object
    params, bs, vk, msgs, sig = _honest(secpar)
    q, d = params.modulus, params.degree
    agg = bs.aggregate(vk, msgs, sig)
    coef = coracle.ntt_inverse(agg, q, params.inv_root % q)
    mx, wt = coracle.norm_weight(coef, q)
    M, W = int(mx.max()), int(wt.max())
    assert 0 < M <= params.beta_vf and 0 < W <= d
    norm, weight = "Norm of aggregate signature too large.", "Weight of aggregate signature too large."
    keys = [vk_to_object(params, v) for v in vk]
    agg_obj = signature_to_object(params, agg)
    n = len(msgs)
    for beta, omega, want in ((M, d, (True, "")), (M, W, (True, "")), (M - 1, d, (False, norm)), (M, W - 1, (False, weight)),
                              (M - 1, W - 1, (False, norm))):
        p = _bounded(params, beta, omega)
        b = BatchScheme(p, threads=4)
        try:
            assert b.verify(vk, msgs, agg) == want, (beta, omega)
            assert b.verify_many(np.concatenate([vk, vk]), msgs + msgs, np.stack([agg, agg]), [n, n]) == [want, want], (beta, omega)
        finally:
            b.close()
        assert F.verify(p, keys, msgs, agg_obj) == want, (beta, omega)
        with BatchQueue(p, workers=1, max_rows=64) as bq:
            assert bq.wait_verdict(bq.submit_verify(vk, msgs, agg)) == want, (beta, omega)


@pytest.mark.parametrize("secpar", [128, 256])
def test_signature_screening_at_one_signers_norm(secpar, coracle, monkeypatch):
    """verify_signatures with beta = one signer's norm passes exactly the signers at or under it (and omega = one signer's
    weight those at or under that); aggregate_screened with signature_bound patched to that norm keeps the same signers and
    returns aggregate() of them"""
    import fusion_hip.scheme as S
    params, bs, vk, msgs, sig = _honest(secpar)
    q, d = params.modulus, params.degree
    coef = coracle.ntt_inverse(sig.reshape(-1, d), q, params.inv_root % q)
    mx, wt = coracle.norm_weight(coef, q)
    norms, weights = mx.reshape(len(msgs), -1).max(axis=1), wt.reshape(len(msgs), -1).max(axis=1)
    beta = int(np.sort(norms)[len(msgs) // 2])
    want = E.expect(norms, weights, False, beta, d)
    assert 0 in want and 4 in want
    assert bs.verify_signatures(vk, msgs, sig, beta=beta).tolist() == want
    assert bs.verify_signatures(vk, msgs, sig, beta=beta - 1).tolist() == E.expect(norms, weights, False, beta - 1, d)
    omega = int(weights.min())
    assert bs.verify_signatures(vk, msgs, sig, beta=2 ** 40, omega=omega).tolist() == E.expect(norms, weights, False, 2 ** 40, omega)
    assert bs.verify_signatures(vk, msgs, sig, beta=2 ** 40, omega=omega - 1).tolist() == [5] * len(msgs)
    monkeypatch.setattr(S, "signature_bound", lambda params: beta)
    agg, codes = bs.aggregate_screened(vk, msgs, sig)
    assert codes.tolist() == want
    ok = codes == 0
    assert np.array_equal(agg, bs.aggregate(vk[ok], [m for m, k in zip(msgs, ok) if k], sig[ok]))


# ---- small moduli -------------------------------------------------------------------------------------------------------
def _root(q, d):
    """a primitive 2d-th root of unity mod the prime q, or None"""
    if (q - 1) % (2 * d):
        return None
    for x in range(2, 1000):
        r = pow(x, (q - 1) // (2 * d), q)
        if pow(r, d, q) == q - 1:
            return r
    return None


@pytest.mark.parametrize("q", E.SMALL_MODULI)
def test_norm_weight_of_stored_values_for_small_moduli(q):
    """Context.norm_weight / norm_weight_dev (ring-only and transform contexts) and the drop-in's norm / weight count what the
    reference counts: max |x| over the stored values, #{x : x % q != 0} -- an unreduced 2q or -3q weighs nothing"""
    import fusion_hip
    from algebra.matrices import GeneralMatrix
    from algebra.polynomials import PolynomialCoefficientRepresentation as PCR
    d = 64
    rows = E.small_modulus_rows(q, d, q % 1000)
    pm, pw = E.py_norm_weight(rows, q)
    ctxs = [fusion_hip.Context(q, d, 0, 0)]
    r = _root(q, d)
    if r is not None:
        ctxs.append(fusion_hip.Context(q, d, r, pow(r, q - 2, q)))
    try:
        for ctx in ctxs:
            mx, wt = ctx.norm_weight(rows)
            assert mx.tolist() == pm and wt.tolist() == pw, (q, ctx.root)
            dR = fusion_hip.DeviceArray.from_numpy(ctx, rows)
            dM, dW = fusion_hip.DeviceArray(ctx, (rows.shape[0],), np.int64), fusion_hip.DeviceArray(ctx, (rows.shape[0],))
            try:
                ctx.norm_weight_dev(dR.ptr, rows.shape[0], dM.ptr, dW.ptr)
                assert dM.numpy().tolist() == pm and dW.numpy().tolist() == pw, (q, ctx.root)
            finally:
                for b in (dR, dM, dW):
                    b.free()
    finally:
        for ctx in ctxs:
            ctx.close()
    polys = [PCR(q, d, 1, 1, 1, [int(x) for x in row]) for row in rows]
    assert [z.weight() for z in polys] == pw and [z.norm("infty") for z in polys] == pm
    for i in range(0, len(polys) - 1, 2):
        m = GeneralMatrix([[polys[i]], [polys[i + 1]]])
        assert m.weight() == max(pw[i], pw[i + 1]) and m.norm("infty") == max(pm[i], pm[i + 1])


def test_drop_in_weight_of_unreduced_multiples():
    """the case that names the defect: 34 = 2 * 17 stored in a degree-8 polynomial mod 17 has weight 0; and the wide path
    (q >= 2^32), whose kernel counts non-zero STORED values -- the drop-in reduces its rows first, so multiples of q weigh
    nothing there either"""
    from algebra.matrices import GeneralMatrix
    from algebra.polynomials import PolynomialCoefficientRepresentation as PCR
    from fusion_hip.wide import get_wide_context
    z = PCR(17, 8, 3, 6, 16, [34, 0, 0, 0, 0, 0, 0, 0])
    assert z.weight() == 0 and z.norm("infty") == 34
    assert GeneralMatrix([[z], [PCR(17, 8, 3, 6, 16, [-51, 17, 1, 0, 0, 0, 0, 0])]]).weight() == 1
    qw = 2 ** 32 + 15
    vals = [2 * qw, -3 * qw, qw, 0, 1, -1, 5 * qw + 2, -(2 ** 40) * qw]
    w = PCR(qw, 8, 1, 1, 1, vals)
    assert w.weight() == sum(1 for x in vals if x % qw) == 3
    assert w.norm("infty") == max(abs(x) for x in vals)
    wctx = get_wide_context(qw, 8)
    mx, wt = wctx.norm_weight(np.array([[qw, -qw, 0, 0, 0, 0, 0, 0], [0] * 8], dtype=np.int64))
    assert wt.tolist() == [2, 0] and mx.tolist() == [qw, 0]         # the wide kernel's own semantics: non-zero stored values
