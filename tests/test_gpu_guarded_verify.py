"""Where the verification entries write: verify_fused with one workgroup per aggregate and with several (R > 1), from int32 rows, from
strided int64 partial sums and keyed, and the unfused route (matvec + inverse transform + norm_weight_kernel + verdict_kernel).
Every input and the device verdict array sit in guarded arenas (tests/_guarded.py): a workgroup that writes verdict[g] for a wrong g,
or any input word, is seen.  The three aggregates of a case have three different verdicts; expectations come from the fixtures of
tests/_verdict_edges.py (built with the C oracle) and from the oracle's verify_core."""
import numpy as np
import pytest

from oracle import oracle as O

import _guarded as G
import _saturation as S
import _verdict_edges as V

pytestmark = pytest.mark.gpu
Q = O.PRIME
BADARG = -1
OMEGA = 10
PAD, TPAD = 24, 8
KNOBS = [{}, {"FZ_UNFUSED": "1"}, {"FZ_VERIFY_ORDERED": "1"}, {"FZ_VERIFY_CENT": "1"}, {"FZ_NO_IMAD": "1"}]
# (d, l, workgroups per aggregate)
SHAPES = [(256, 3, 1), (64, 5, 1), (256, 5, 2), (64, 17, 2)]


@pytest.fixture(scope="module")
def ctxs():
    c = G.Contexts()
    yield c
    c.close()


_fixtures = {}


def _fixture(coracle, d, l):
    """three aggregates: within both bounds (0), norm one above beta (4), weight one above omega (5)"""
    if (d, l) not in _fixtures:
        P = O.PARAMS[{64: 128, 256: 256}[d]]
        beta = P["beta_vf"]
        specs = [dict(M=beta, W=OMEGA), dict(M=beta + 1, W=OMEGA, extreme=l - 1, heavy=l - 1, pos=d - 1, sign=-1),
                 dict(M=beta, W=OMEGA + 1, heavy=l // 2, extreme=l // 2)]
        _fixtures[(d, l)] = V.build(P, l, specs, 900 + d + l, coracle)
    return _fixtures[(d, l)]


def _ident(env):
    return ",".join(f"{k[3:]}={v}" for k, v in env.items()) or "defaults"


@pytest.mark.parametrize("env", KNOBS, ids=_ident)
@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("d,l,R", SHAPES, ids=str)
def test_verify_entries(d, l, R, groups, env, coracle, ctxs):
    fx = _fixture(coracle, d, l)
    P, beta = fx.P, fx.P["beta_vf"]
    assert S.verify_shape(l, d, groups, G.num_cu())[0] == R
    ctx = ctxs.get(G.scheme_ring(d), env)
    A, sig, tgt = fx.A, fx.sig[:groups], fx.target[:groups]
    bad_t, bad_r = fx.tampered([groups - 1])
    want = V.expect(fx.M[:groups], fx.W[:groups], False, beta, OMEGA)
    want_bad = V.expect(fx.M[:groups], fx.W[:groups], [g == groups - 1 for g in range(groups)], beta, OMEGA)
    assert want == [0, 4, 5][:groups] and want_bad[-1] == 3
    ones = np.ones((1, d), np.int32)
    for g in range(groups):                                   # the oracle's own verdicts (one signer, alpha_hat = 1)
        assert coracle.verify_core(A, sig[g], fx.vkL[g:g + 1], fx.vkR[g:g + 1], fx.c[g:g + 1], ones, Q, P["inv_root"], beta, OMEGA) == want[g]
    for target, vkR, verdicts in ((tgt, fx.vkR[:groups], want), (bad_t[:groups], bad_r[:groups], want_bad)):
        Wd = np.array(verdicts, np.int32)
        base = [G.inp("A", A), G.inp("sig", sig.reshape(-1, d)), G.inp("target", target)]
        # host verdicts
        rets = G.on_device(ctx, base, lambda p: ctx.verify_with_target_batch_dev(p["A"].ptr, p["sig"].ptr, p["target"].ptr, groups, l, beta, OMEGA))
        assert rets == [verdicts, verdicts]
        one = [G.inp("A", A), G.inp("sig", sig[groups - 1]), G.inp("target", target[groups - 1])]
        rets = G.on_device(ctx, one, lambda p: ctx.verify_with_target_dev(p["A"].ptr, p["sig"].ptr, p["target"].ptr, l, beta, OMEGA))
        assert rets == [verdicts[-1]] * 2
        g = groups - 1
        core = [G.inp("A", A), G.inp("sig", sig[g]), G.inp("vkL", fx.vkL[g:g + 1]), G.inp("vkR", vkR[g:g + 1]), G.inp("c", fx.c[g:g + 1]),
                G.inp("alpha", ones)]
        rets = G.on_device(ctx, core, lambda p: ctx.verify_core_dev(p["A"].ptr, p["sig"].ptr, p["vkL"].ptr, p["vkR"].ptr, p["c"].ptr, p["alpha"].ptr,
                                                                   1, l, beta, OMEGA))
        assert rets == [verdicts[-1]] * 2
        # device verdicts, in an arena
        G.on_device(ctx, base + [G.out("verdicts", Wd)],
                    lambda p: ctx.verify_with_target_batch_async_dev(p["A"].ptr, p["sig"].ptr, p["target"].ptr, groups, l, beta, OMEGA, p["verdicts"].ptr))
        # int64 partial sums `stride` apart, any representative of the residues
        rng = np.random.default_rng(5)
        sig64 = sig.astype(np.int64).reshape(groups, l * d) + Q * rng.integers(-2 ** 31, 2 ** 31, size=(groups, l * d))
        tgt64 = target.astype(np.int64) + Q * rng.integers(-2 ** 31, 2 ** 31, size=(groups, d))
        ops = [G.inp("A", A), G.inp("partial", sig64, stride=l * d + PAD), G.inp("target", tgt64, stride=d + TPAD), G.out("verdicts", Wd)]
        G.on_device(ctx, ops, lambda p: ctx.verify_partials_batch_async_dev(p["A"].ptr, p["partial"].ptr, l * d + PAD, p["target"].ptr, d + TPAD, groups,
                                                                           l, beta, OMEGA, p["verdicts"].ptr))
        # keyed: the target formed from vk [N][2][d] and c
        vk = np.stack([fx.vkL[:groups], vkR], axis=1)
        ops = [G.inp("A", A), G.inp("sig", sig.reshape(-1, d)), G.inp("vk", vk.reshape(-1, d)), G.inp("c", fx.c[:groups]), G.out("verdicts", Wd)]
        G.on_device(ctx, ops, lambda p: ctx.verify_signatures_async_dev(p["A"].ptr, p["sig"].ptr, p["vk"].ptr, p["c"].ptr, groups, l, beta, OMEGA,
                                                                       p["verdicts"].ptr))


def test_refused_calls_write_nothing(ctxs):
    d, l = 64, 2
    ctx = ctxs.get(G.scheme_ring(d))
    z = np.zeros((l, d), np.int32)
    ops = [G.inp("A", z), G.inp("sig", z), G.inp("target", z[:1]), G.inp("vk", z), G.inp("c", z[:1]), G.inp("alpha", z[:1]),
           G.inp("partial", np.zeros((2, l * d), np.int64), stride=l * d + PAD), G.inp("target64", np.zeros((2, d), np.int64), stride=d + TPAD),
           G.out("verdicts", np.zeros(2, np.int32)), G.inp("sig4", z, offset=4)]
    P = lambda p, n: p[n].ptr                                                   # noqa: E731
    G.refused(ctx, ops, lambda p: ctx.verify_with_target_batch_dev(P(p, "A"), P(p, "sig"), P(p, "target"), 1, 0, 1, 1), BADARG)
    G.refused(ctx, ops, lambda p: ctx.verify_with_target_dev(P(p, "A"), P(p, "sig"), 0, l, 1, 1), BADARG)
    G.refused(ctx, ops, lambda p: ctx.verify_with_target_batch_async_dev(P(p, "A"), P(p, "sig"), P(p, "target"), 1, l, 1, 1, 0), BADARG)
    G.refused(ctx, ops, lambda p: ctx.verify_partials_batch_async_dev(P(p, "A"), P(p, "partial"), l * d + 1, P(p, "target64"), d + TPAD, 2, l, 1, 1,
                                                                     P(p, "verdicts")), BADARG)
    G.refused(ctx, ops, lambda p: ctx.verify_signatures_async_dev(P(p, "A"), P(p, "sig4"), P(p, "vk"), P(p, "c"), 1, l, 1, 1, P(p, "verdicts")), BADARG)
    G.refused(ctx, ops, lambda p: ctx.verify_core_dev(P(p, "A"), P(p, "sig"), P(p, "vk"), P(p, "vk"), P(p, "c"), P(p, "alpha"), 0, l, 1, 1), BADARG)
