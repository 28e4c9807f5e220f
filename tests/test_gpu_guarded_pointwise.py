"""Where the pointwise entries write: pw_kernel (mul, add, sub, neg, mulacc), pw_bcast_kernel, fill_synthetic_kernel,
reduce_i64_kernel and norm_weight_kernel, every operand in a guarded arena (tests/_guarded.py), at the smallest counts that reach
the int4 body, the ragged tail and a second block, 16-byte aligned and 4 bytes past it (pw_kernel with vec == 0).  Expectations
come from the C oracle and from Python integers; inputs are any int32 with the extremes planted."""
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
    return G.scheme_ring(d) if d in (64, 256) else (Q, d, 0, 0)


# ---- the harness itself, end to end on the device -----------------------------------------------------------------------------
def test_the_device_backend_reports_a_write_past_the_declared_interior(ctxs):
    """fz_pw_add is asked for four rows of 16 while `out` declares three: the fourth row lands in out's trail guard (inside its
    allocation) and the harness names it; no kernel is changed"""
    ctx = ctxs.get(_ring(64))
    rng = np.random.default_rng(1)
    a, b = G.any_int32(rng, (4, 16)), G.any_int32(rng, (4, 16))
    want = S.cent_arr(a.astype(np.int64) + b, Q).astype(np.int32)
    ops = [G.inp("a", a), G.inp("b", b), G.out("out", want[:3])]
    with pytest.raises(G.GuardError, match=r"out: guard word written: trail guard, 0 element\(s\) after the interior \(index 48\).*16 guard word"):
        G.on_device(ctx, ops, lambda p: ctx.pw_dev(1, p["a"].ptr, p["b"].ptr, p["out"].ptr, 64))
    ops[2] = G.out("out", want)
    G.on_device(ctx, ops, lambda p: ctx.pw_dev(1, p["a"].ptr, p["b"].ptr, p["out"].ptr, 64))


# ---- pw_kernel ------------------------------------------------------------------------------------------------------------------
COUNTS = [1, 3, 4, 5, 1021]


@pytest.mark.parametrize("offset", [0, 4], ids=["aligned", "plus4"])
@pytest.mark.parametrize("count", COUNTS)
def test_pw_kernel(count, offset, coracle, ctxs):
    ctx = ctxs.get(_ring(64))
    rng = np.random.default_rng(100 + count)
    a, b, acc = (G.any_int32(rng, (count,)) for _ in range(3))
    for op, name in ((0, "pw_mul"), (1, "pw_add"), (2, "pw_sub")):
        want = getattr(coracle, name)(a, b, Q)
        ops = [G.inp("a", a, offset=offset), G.inp("b", b, offset=offset), G.out("out", want, offset=offset)]
        G.on_device(ctx, ops, lambda p: ctx.pw_dev(op, p["a"].ptr, p["b"].ptr, p["out"].ptr, count))
    ops = [G.inp("a", a, offset=offset), G.out("out", coracle.pw_neg(a, Q), offset=offset)]
    G.on_device(ctx, ops, lambda p: ctx.pw_neg_dev(p["a"].ptr, p["out"].ptr, count))
    # fz_pw_mulacc reads its output by specification: the accumulator's previous contents are data, not fill
    ops = [G.inout("acc", acc, coracle.pw_mulacc(acc, a, b, Q), offset=offset), G.inp("a", a, offset=offset), G.inp("b", b, offset=offset)]
    G.on_device(ctx, ops, lambda p: ctx.pw_mulacc_dev(p["acc"].ptr, p["a"].ptr, p["b"].ptr, count))


def test_pw_kernel_one_unaligned_operand_is_enough_for_the_scalar_route(coracle, ctxs):
    """vec is the OR of the three addresses: each operand alone 4 bytes off"""
    ctx = ctxs.get(_ring(64))
    rng = np.random.default_rng(7)
    a, b = G.any_int32(rng, (13,)), G.any_int32(rng, (13,))
    want = coracle.pw_mul(a, b, Q)
    for who in range(3):
        off = [4 if k == who else 0 for k in range(3)]
        ops = [G.inp("a", a, offset=off[0]), G.inp("b", b, offset=off[1]), G.out("out", want, offset=off[2])]
        G.on_device(ctx, ops, lambda p: ctx.pw_dev(0, p["a"].ptr, p["b"].ptr, p["out"].ptr, 13))


# ---- pw_bcast_kernel: its first parity test ----------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 4], ids=["aligned", "plus4"])
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("d", [1, 12, 64])
def test_pw_mul_bcast(d, rows, offset, ctxs):
    """out[r][j] = cent(a[r][j] * s[j]), in Python integers; s holds the int32 extremes"""
    ctx = ctxs.get(_ring(d))
    rng = np.random.default_rng(200 + d + rows)
    a, s = G.any_int32(rng, (rows, d)), G.any_int32(rng, (d,))
    s[:: 3] = np.array([-2 ** 31, 2 ** 31 - 1, -1])[np.arange(len(s[:: 3])) % 3]
    want = np.array([[S.cent(int(x) * int(y), Q) for x, y in zip(row, s)] for row in a], dtype=np.int32)
    ops = [G.inp("a", a, offset=offset), G.inp("s", s, offset=offset), G.out("out", want, offset=offset)]
    G.on_device(ctx, ops, lambda p: ctx.pw_mul_bcast_dev(p["a"].ptr, p["s"].ptr, p["out"].ptr, rows))


# ---- fill_synthetic_kernel, reduce_i64_kernel ----------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 4], ids=["aligned", "plus4"])
@pytest.mark.parametrize("count", [1, 255, 257])
def test_fill_synthetic(count, offset, ctxs):
    ctx = ctxs.get(_ring(64))
    for seed in (5, 2 ** 63 + 11):
        ops = [G.out("out", O.splitmix_centered(seed, count), offset=offset)]
        G.on_device(ctx, ops, lambda p: ctx.fill_synthetic_dev(p["out"].ptr, count, seed))


@pytest.mark.parametrize("offset", [0, 4], ids=["aligned", "plus4"])
@pytest.mark.parametrize("count", [1, 255, 257])
def test_reduce_i64(count, offset, ctxs):
    """cent(x) of any int64, the extremes among them, in Python integers"""
    ctx = ctxs.get(_ring(64))
    rng = np.random.default_rng(300 + count)
    x = rng.integers(-2 ** 63, 2 ** 63 - 1, size=count, dtype=np.int64, endpoint=True)
    edge = np.array([-2 ** 63, 2 ** 63 - 1, 0, -1, Q, -Q, Q // 2, Q // 2 + 1], dtype=np.int64)
    x[: min(count, 8)] = edge[: min(count, 8)]
    want = np.array([S.cent(int(v), Q) for v in x], dtype=np.int32)
    ops = [G.inp("in", x), G.out("out", want, offset=offset)]
    G.on_device(ctx, ops, lambda p: ctx.reduce_i64_dev(p["in"].ptr, p["out"].ptr, count))


# ---- norm_weight_kernel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 4], ids=["aligned", "plus4"])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("d", [1, 63, 65, 256])
def test_norm_weight(d, batch, offset, coracle, ctxs):
    """max |x| over stored values and #{x : x mod q != 0} per row (the C oracle, and Python integers for the first row); the
    multiples of q and -2^31 among the values"""
    ctx = ctxs.get(_ring(d))
    rng = np.random.default_rng(400 + d + batch)
    x = G.any_int32(rng, (batch, d))
    x[rng.random((batch, d)) < 0.2] = 0
    x[-1, -1] = Q
    x[0, d // 2] = -Q if d > 1 else x[0, 0]
    mx, wt = coracle.norm_weight(x, Q)
    assert int(mx[0]) == max(abs(int(v)) for v in x[0]) and int(wt[0]) == sum(1 for v in x[0] if int(v) % Q)
    ops = [G.inp("coef", x, offset=offset), G.out("max_abs", mx), G.out("weight", wt, offset=offset)]
    G.on_device(ctx, ops, lambda p: ctx.norm_weight_dev(p["coef"].ptr, batch, p["max_abs"].ptr, p["weight"].ptr))


# ---- refusals: a NULL operand; nothing may be written ----------------------------------------------------------------------------
def test_refused_calls_write_nothing(ctxs):
    ctx = ctxs.get(_ring(64))
    z = np.zeros(64, np.int32)
    three = [G.inp("a", z), G.inp("b", z), G.out("out", z)]
    for op in (0, 1, 2):
        G.refused(ctx, three, lambda p: ctx.pw_dev(op, p["a"].ptr, 0, p["out"].ptr, 64), BADARG)
    G.refused(ctx, three, lambda p: ctx.pw_neg_dev(0, p["out"].ptr, 64), BADARG)
    G.refused(ctx, three, lambda p: ctx.pw_mulacc_dev(p["out"].ptr, p["a"].ptr, 0, 64), BADARG)
    G.refused(ctx, three, lambda p: ctx.pw_mul_bcast_dev(p["a"].ptr, 0, p["out"].ptr, 1), BADARG)
    G.refused(ctx, three, lambda p: ctx.fill_synthetic_dev(0, 64, 1), BADARG)
    G.refused(ctx, [G.inp("in", np.zeros(64, np.int64)), G.out("out", z)], lambda p: ctx.reduce_i64_dev(p["in"].ptr, 0, 64), BADARG)
    G.refused(ctx, [G.inp("coef", z), G.out("max_abs", np.zeros(1, np.int64)), G.out("weight", np.zeros(1, np.int32))],
              lambda p: ctx.norm_weight_dev(p["coef"].ptr, 1, 0, p["weight"].ptr), BADARG)
