"""Where the transforms outside the 16-per-lane landing tests write: ntt_small (degrees 2, 8, 16), the radix-4 kernels at one, two and
four row groups per wave (FZ_NTT_KERNEL=4, FZ_NTT_ROWS), ntt_big (512, 4096) and the negacyclic product in both fused forms and its
composed route (FZ_POLYMUL_FORM), out of place and with `out` aliasing `f`.  Inputs and outputs sit in guarded arenas
(tests/_guarded.py): 16 KiB on either side, far more than the guard row of test_gpu_ntt_landing.py.  Row counts 1, 3, 5, 9 leave
the last wave's row slots partly filled at every degree.  Expectations: the C oracle's transforms (and pw_mul between them for the
product); inputs: any int32."""
import numpy as np
import pytest

from oracle import oracle as O

import _guarded as G

pytestmark = pytest.mark.gpu
Q = O.PRIME
BADARG, UNSUPPORTED = -1, -2
ROWS = [1, 3, 5, 9]
# degree -> modulus: the scheme's prime has roots of order up to 512; 12289 and 65537 serve the one-workgroup-per-row kernels
MODULUS = {512: 12289, 4096: 65537}


@pytest.fixture(scope="module")
def ctxs():
    c = G.Contexts()
    yield c
    c.close()


def _ring(d):
    if d in (64, 256):
        return G.scheme_ring(d)
    q = MODULUS.get(d, Q)
    return (q, d) + G.root_pair(q, d)


def _both_directions(ctx, coracle, ring, rows, seed):
    q, d, root, inv = ring
    x = G.any_int32(np.random.default_rng(seed), (rows, d))
    for inverse in (False, True):
        want = coracle.ntt_inverse(x, q, inv) if inverse else coracle.ntt_forward(x, q, root)
        fn = ctx.ntt_inverse_dev if inverse else ctx.ntt_forward_dev
        G.on_device(ctx, [G.inp("in", x), G.out("out", want.reshape(rows, d))], lambda p: fn(p["in"].ptr, p["out"].ptr, rows))


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("d", [2, 8, 16])
def test_ntt_small(d, rows, coracle, ctxs):
    ring = _ring(d)
    _both_directions(ctxs.get(ring), coracle, ring, rows, 10 * d + rows)


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("nr", [1, 2, 4])
@pytest.mark.parametrize("d", [64, 256])
def test_radix4(d, nr, rows, coracle, ctxs):
    ring = _ring(d)
    ctx = ctxs.get(ring, {"FZ_NTT_KERNEL": "4", "FZ_NTT_ROWS": str(nr)})
    assert ctx.diag_ntt_schedule(rows) == 4
    _both_directions(ctx, coracle, ring, rows, 100 * nr + d + rows)


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("d", [512, 4096])
def test_ntt_big(d, rows, coracle, ctxs):
    ring = _ring(d)
    ctx = ctxs.get(ring)
    assert ctx.diag_ntt_schedule(rows) == 0
    _both_directions(ctx, coracle, ring, rows, 1000 + d + rows)


# ---- the negacyclic product ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 3, 5])
@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("d", [32, 64, 128, 256])
def test_poly_mul(d, form, rows, coracle, ctxs):
    """FZ_POLYMUL_FORM=1: polymul_fused at degrees 64 and 256, the composed route (two transforms into scratch, the product, the inverse
    into out) at 32 and 128; =2: polymul16 at all four.  out of place; and out = f, which the header allows: g must come back unchanged"""
    ring = _ring(d)
    q, _, root, inv = ring
    ctx = ctxs.get(ring, {"FZ_POLYMUL_FORM": str(form)})
    rng = np.random.default_rng(2000 + 10 * d + rows + form)
    f, g = G.any_int32(rng, (rows, d)), G.any_int32(rng, (rows, d))
    want = coracle.ntt_inverse(coracle.pw_mul(coracle.ntt_forward(f, q, root), coracle.ntt_forward(g, q, root), q), q, inv).reshape(rows, d)
    G.on_device(ctx, [G.inp("f", f), G.inp("g", g), G.out("out", want)], lambda p: ctx.poly_mul_dev(p["f"].ptr, p["g"].ptr, p["out"].ptr, rows))
    G.on_device(ctx, [G.inout("f", f, want), G.inp("g", g)], lambda p: ctx.poly_mul_dev(p["f"].ptr, p["g"].ptr, p["f"].ptr, rows))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_write_nothing(ctxs):
    ring = _ring(64)
    ctx = ctxs.get(ring)
    z = np.zeros((2, 64), np.int32)
    ops = [G.inp("in", z), G.inp("in4", z, offset=4), G.inp("g", z), G.out("out", z), G.out("out4", z, offset=4)]
    P = lambda p, n: p[n].ptr                                                   # noqa: E731
    for fn in (ctx.ntt_forward_dev, ctx.ntt_inverse_dev):
        G.refused(ctx, ops, lambda p: fn(P(p, "in"), 0, 2), BADARG)
        G.refused(ctx, ops, lambda p: fn(P(p, "in4"), P(p, "out"), 2), BADARG)          # rows must be 16-byte aligned
        G.refused(ctx, ops, lambda p: fn(P(p, "in"), P(p, "out4"), 2), BADARG)
    G.refused(ctx, ops, lambda p: ctx.poly_mul_dev(P(p, "in"), 0, P(p, "out"), 2), BADARG)
    ring12 = (Q, 12, 0, 0)                                                       # ring-only: no transforms
    ctx12 = ctxs.get(ring12)
    z12 = np.zeros((2, 12), np.int32)
    ops12 = [G.inp("in", z12), G.inp("g", z12), G.out("out", z12)]
    G.refused(ctx12, ops12, lambda p: ctx12.ntt_forward_dev(P(p, "in"), P(p, "out"), 2), UNSUPPORTED)
    G.refused(ctx12, ops12, lambda p: ctx12.poly_mul_dev(P(p, "in"), P(p, "g"), P(p, "out"), 2), UNSUPPORTED)
