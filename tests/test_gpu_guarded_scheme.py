"""Where matvec, signing and key generation write: every kernel of fz_launch_matvec (split, sliced at KS = 1 .. 16, the eight-row
fp64 kernel, the scalar kernel), sign_kernel / sign_scalar_kernel, keygen_fused in both multiply forms, keygen_bcast_fused, the
unfused routes and bcast_rows_kernel, every operand in a guarded arena (tests/_guarded.py).  The route of each case is asserted
with the launcher's model (tests/_saturation.py: matvec_route) or forced by a knob, a degree or an alignment that the code maps to
one kernel.  Expectations: the C oracle; inputs: any int32, the extremes planted."""
import numpy as np
import pytest

from oracle import oracle as O

import _guarded as G
import _saturation as S

pytestmark = pytest.mark.gpu
Q = O.PRIME
BADARG = -1


@pytest.fixture(scope="module")
def ctxs():
    c = G.Contexts()
    yield c
    c.close()


def _ring(d):
    if d in (64, 256):
        return G.scheme_ring(d)
    if d == 32:
        return (Q, d) + G.root_pair(Q, d)
    return (Q, d, 0, 0)                                       # ring-only


# ---- matvec ---------------------------------------------------------------------------------------------------------------------
def _matvec(ctxs, coracle, d, knob, batch, l, route, offsets=(0, 0, 0), seed=0):
    env = {} if knob is None else {"FZ_MATVEC_SLICES": str(knob)}
    ctx = ctxs.get(_ring(d), env)
    assert S.matvec_route(0 if knob is None else knob, batch, l, d, G.num_cu(), aligned=not any(offsets)) == route
    rng = np.random.default_rng(1000 + 7 * d + 3 * l + batch + seed)
    A, Sb = G.any_int32(rng, (l, d)), G.any_int32(rng, (batch, l, d))
    ops = [G.inp("A", A, offset=offsets[0]), G.inp("S", Sb, offset=offsets[1]), G.out("out", coracle.matvec(A, Sb, Q), offset=offsets[2])]
    G.on_device(ctx, ops, lambda p: ctx.matvec_dev(p["A"].ptr, p["S"].ptr, p["out"].ptr, batch, l))


@pytest.mark.parametrize("l", [1, 5])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("d", [16, 4096])
def test_matvec_split(d, batch, l, coracle, ctxs):
    """degree 16: 256 slices of the k range, more than there are rows; degree 4096: one slice"""
    _matvec(ctxs, coracle, d, 0, batch, l, "split")


# l -> the KS that runs under each knob: `while (ks > 1 && l / ks < 8) ks >>= 1`
SLICED = [(knob, l, min(knob, {8: 1, 17: 2, 131: 16}[l])) for knob in (1, 2, 4, 8, 16) for l in (8, 17, 131)]


@pytest.mark.parametrize("knob,l,ks", SLICED, ids=lambda v: str(v))
def test_matvec_sliced(knob, l, ks, coracle, ctxs):
    """batch 3 at degree 64: 48 columns, so 48 of 256 / 128 / 64 lanes of the one workgroup are live and the idle ones shadow the
    last column; at KS = 16 and l = 131 every slice holds nine rows and the last one none"""
    assert (knob, l) != (16, 131) or (-(-131 // 16) == 9 and 15 * 9 >= 131)
    _matvec(ctxs, coracle, 64, knob, 3, l, ("sliced", ks))
    if l == 131:
        _matvec(ctxs, coracle, 256, knob, 3, l, ("sliced", ks), seed=1)        # 192 columns: a whole and a partly filled workgroup at KS >= 2


@pytest.mark.parametrize("l", [7, 8, 9])
def test_matvec_kernel(l, coracle, ctxs):
    """the eight-row fp64 kernel, on both sides of its unroll.  With FZ_MATVEC_SLICES=-1 a power-of-two degree of this batch goes to
    the split kernel, so the degree is 12 (int4 rows, not a power of two)"""
    _matvec(ctxs, coracle, 12, -1, 3, l, "kernel")


@pytest.mark.parametrize("l", [1, 9])
@pytest.mark.parametrize("d,offsets", [(13, (0, 0, 0)), (64, (4, 0, 0)), (64, (0, 4, 0)), (64, (0, 0, 4)), (64, (4, 4, 4))], ids=str)
def test_matvec_scalar(d, offsets, l, coracle, ctxs):
    """a degree that is no multiple of 4, or any one operand 4 bytes off"""
    _matvec(ctxs, coracle, d, None, 3, l, "scalar", offsets)


def test_matvec_refusals(ctxs):
    ctx = ctxs.get(_ring(64))
    z = np.zeros((1, 64), np.int32)
    ops = [G.inp("A", z), G.inp("S", z), G.out("out", z)]
    G.refused(ctx, ops, lambda p: ctx.matvec_dev(p["A"].ptr, p["S"].ptr, p["out"].ptr, 1, 0), BADARG)
    G.refused(ctx, ops, lambda p: ctx.matvec_dev(p["A"].ptr, 0, p["out"].ptr, 1, 1), BADARG)


# ---- sign -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 4], ids=["aligned", "plus4"])
@pytest.mark.parametrize("batch,l", [(1, 1), (3, 3)])
@pytest.mark.parametrize("d", [64, 256, 12, 13])
def test_sign_core(d, batch, l, offset, coracle, ctxs):
    """sign_kernel (int4 rows: degrees 64, 256, 12 aligned); sign_scalar_kernel (degree 13, or 4 bytes off)"""
    ctx = ctxs.get(_ring(d))
    rng = np.random.default_rng(2000 + d + batch)
    sk, c = G.any_int32(rng, (batch, 2, l, d)), G.any_int32(rng, (batch, d))
    ops = [G.inp("sk_hat", sk, offset=offset), G.inp("c_hat", c, offset=offset), G.out("sig", coracle.sign_core(sk, c, Q), offset=offset)]
    G.on_device(ctx, ops, lambda p: ctx.sign_core_dev(p["sk_hat"].ptr, p["c_hat"].ptr, p["sig"].ptr, batch, l))


def test_sign_refusals(ctxs):
    ctx = ctxs.get(_ring(64))
    z = np.zeros((1, 64), np.int32)
    ops = [G.inp("sk_hat", np.zeros((2, 64), np.int32)), G.inp("c_hat", z), G.out("sig", z)]
    G.refused(ctx, ops, lambda p: ctx.sign_core_dev(p["sk_hat"].ptr, p["c_hat"].ptr, p["sig"].ptr, 1, 0), BADARG)
    G.refused(ctx, ops, lambda p: ctx.sign_core_dev(p["sk_hat"].ptr, p["c_hat"].ptr, 0, 1, 1), BADARG)


# ---- keygen ---------------------------------------------------------------------------------------------------------------------
def _keygen(ctx, coracle, d, batch, l, bcast=False, offsets=None, seed=0):
    """offsets: name -> 4 for the operands placed 4 bytes off"""
    offsets = offsets or {}
    ring = _ring(d)
    rng = np.random.default_rng(3000 + 11 * d + 5 * l + batch + seed)
    A = G.any_int32(rng, (l, d))
    polys = G.any_int32(rng, (batch, 2, d))
    coef = np.ascontiguousarray(np.broadcast_to(polys[:, :, None, :], (batch, 2, l, d))) if bcast else G.any_int32(rng, (batch, 2, l, d))
    sk, vk = coracle.keygen_core(A, coef, Q, ring[2])
    ops = [G.inp("A", A, offset=offsets.get("A", 0)), G.inp("coef", polys if bcast else coef, offset=offsets.get("coef", 0)),
           G.out("sk_hat", sk, offset=offsets.get("sk_hat", 0)), G.out("vk", vk, offset=offsets.get("vk", 0))]
    fn = ctx.keygen_core_bcast_dev if bcast else ctx.keygen_core_dev
    return ops, (lambda p: fn(p["A"].ptr, p["coef"].ptr, p["sk_hat"].ptr, p["vk"].ptr, batch, l))


KEYGEN_SHAPES = [(64, l) for l in (1, 3, 5, 17)] + [(256, l) for l in (1, 3, 5)]


@pytest.mark.parametrize("no_imad", [False, True], ids=["imad", "fp64"])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("d,l", KEYGEN_SHAPES)
def test_keygen_fused(d, l, batch, no_imad, coracle, ctxs):
    """degree 64: four rows per wave, sixteen per round of the workgroup -- l = 1, 3, 5 leave row slots and whole waves idle (clamped
    onto the last row, storing nothing), 17 puts one row into a second round; degree 256: one row per wave.  vk may lie anywhere:
    it is written one coefficient per thread"""
    ctx = ctxs.get(_ring(d), {"FZ_NO_IMAD": "1"} if no_imad else {})
    G.on_device(ctx, *_keygen(ctx, coracle, d, batch, l))
    G.on_device(ctx, *_keygen(ctx, coracle, d, batch, l, offsets={"vk": 4}, seed=1))


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("d,l", KEYGEN_SHAPES + [(64, 65)])
def test_keygen_bcast_fused(d, l, batch, coracle, ctxs):
    """one polynomial per (key, half); at degree 64 a round covers step * U = 16 * 4 rows: l = 65 puts one row into a second"""
    ctx = ctxs.get(_ring(d))
    G.on_device(ctx, *_keygen(ctx, coracle, d, batch, l, bcast=True))


@pytest.mark.parametrize("d,l", [(64, 5), (256, 3)])
def test_keygen_unfused(d, l, coracle, ctxs):
    """FZ_UNFUSED=1: transform + matvec, and the row expansion (bcast_rows_kernel) of the one-polynomial form; without the knob,
    A alone 4 bytes off leaves the fused kernel for the same launches with matvec_scalar_kernel"""
    ctx = ctxs.get(_ring(d), {"FZ_UNFUSED": "1"})
    for bcast in (False, True):
        G.on_device(ctx, *_keygen(ctx, coracle, d, 3, l, bcast=bcast))
    ctx = ctxs.get(_ring(d))
    for bcast in (False, True):
        G.on_device(ctx, *_keygen(ctx, coracle, d, 3, l, bcast=bcast, offsets={"A": 4}, seed=2))


@pytest.mark.parametrize("d", [32])
def test_keygen_bcast_rows_generic_degree(d, coracle, ctxs):
    ctx = ctxs.get(_ring(d))
    G.on_device(ctx, *_keygen(ctx, coracle, d, 3, 3, bcast=True))
    G.on_device(ctx, *_keygen(ctx, coracle, d, 1, 3, bcast=False))


def test_keygen_refusals(ctxs):
    """l = 0 and a NULL operand; secret rows 4 bytes off have no route (the transforms take 16-byte aligned rows): refused before
    anything is written"""
    for d in (64, 256):
        ctx = ctxs.get(_ring(d))
        z = np.zeros((2, d), np.int32)
        ops = [G.inp("A", z[:1]), G.inp("coef", z), G.out("sk_hat", z), G.out("vk", z)]
        for fn in (ctx.keygen_core_dev, ctx.keygen_core_bcast_dev):
            G.refused(ctx, ops, lambda p: fn(p["A"].ptr, p["coef"].ptr, p["sk_hat"].ptr, p["vk"].ptr, 1, 0), BADARG)
            G.refused(ctx, ops, lambda p: fn(p["A"].ptr, p["coef"].ptr, p["sk_hat"].ptr, 0, 1, 1), BADARG)
        off = [G.inp("A", z[:1]), G.inp("coef", z, offset=4), G.out("sk_hat", z), G.out("vk", z)]
        G.refused(ctx, off, lambda p: ctx.keygen_core_dev(p["A"].ptr, p["coef"].ptr, p["sk_hat"].ptr, p["vk"].ptr, 1, 1), BADARG)
