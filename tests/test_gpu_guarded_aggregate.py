"""Where the aggregation entries write: aggregate_onepass at AR = 4, 3, 2 with several signer slices and with one, aggregate_direct at
two and four rows per tile, aggregate_generic_kernel, the ragged launches across the 64-aggregate seam, the fused sign + aggregate
and target_kernel -- every operand in a guarded arena (tests/_guarded.py), the int64 partials `stride` apart with the gap words in the
guard.  Routes: FZ_AGG_DIRECT and the launcher's models in tests/_saturation.py (onepass_shape, direct_taken) at this device's CU
count.  Expectations: the C oracle's pointwise steps and aggregate_core, summed in Python integers; inputs: any int32.  The int64
partial sums are specified modulo q ("the same sum without the final reduction"): they are compared as centred residues."""
import numpy as np
import pytest

from oracle import oracle as O

import _guarded as G
import _saturation as S

pytestmark = pytest.mark.gpu
Q = O.PRIME
BADARG, UNSUPPORTED = -1, -2
PAD, TPAD = 24, 8                                              # partial_stride = l * d + PAD, target_stride = d + TPAD
CANON = G.cent_mod(Q)


@pytest.fixture(scope="module")
def ctxs():
    c = G.Contexts()
    yield c
    c.close()


def _ring(d):
    return G.scheme_ring(d) if d in (64, 256) else (Q, d, 0, 0)


def _ctx(ctxs, d, direct=None):
    return ctxs.get(_ring(d), {} if direct is None else {"FZ_AGG_DIRECT": str(direct)})


class Problem:
    """`sizes` aggregates of l rows at degree d: inputs (concatenated over the aggregates) and what every entry must leave"""

    def __init__(self, coracle, sizes, l, d, seed):
        rng = np.random.default_rng(seed)
        self.sizes, self.l, self.d, self.G = list(sizes), l, d, len(sizes)
        n = sum(sizes)
        self.off = np.concatenate([[0], np.cumsum(sizes)]).astype(int).tolist()
        self.sk = G.any_int32(rng, (max(n, 1), 2, l, d))[:n]
        self.c, self.alpha, self.vkL, self.vkR = (G.any_int32(rng, (max(n, 1), d))[:n] for _ in range(4))
        self.sig = G.any_int32(rng, (max(n, 1), l, d))[:n]
        self.signed = coracle.sign_core(self.sk, self.c, Q) if n else self.sig
        term = coracle.pw_mul(coracle.pw_add(coracle.pw_mul(self.vkL, self.c, Q), self.vkR, Q), self.alpha, Q) if n else self.c
        agg, sagg, tgt = [], [], []
        for g in range(self.G):
            lo, hi = self.off[g], self.off[g + 1]
            zero = np.zeros((l, d), np.int32)
            agg.append(coracle.aggregate_core(self.sig[lo:hi], self.alpha[lo:hi], Q) if hi > lo else zero)
            sagg.append(coracle.aggregate_core(self.signed[lo:hi], self.alpha[lo:hi], Q) if hi > lo else zero)
            tgt.append(S.cent_arr(term[lo:hi].astype(np.int64).sum(axis=0), Q))
        self.agg, self.sagg, self.tgt = np.stack(agg), np.stack(sagg), np.stack(tgt).astype(np.int64)

    # operands
    def ins(self, *names, offset=None):
        offset = offset or {}
        return [G.inp(n, getattr(self, n).reshape(-1, self.d), offset=offset.get(n, 0)) for n in names]

    def partial(self, signed=False, stride=True):
        want = (self.sagg if signed else self.agg).astype(np.int64).reshape(self.G, self.l * self.d)
        return G.out("partial", want, stride=self.l * self.d + (PAD if stride else 0), canon=CANON)

    def target(self, stride=True):
        return G.out("target", self.tgt, stride=self.d + (TPAD if stride else 0), canon=CANON)


def _equal_sizes(ctx, pb, entries=("core", "partial", "target", "sign"), offset=None):
    """the four equal-size entries on one problem (every aggregate of pb.sizes[0] signers; `core` takes the first aggregate)"""
    N, l, d, groups = pb.sizes[0], pb.l, pb.d, pb.G
    ps, ts = l * d + PAD, d + TPAD
    if "core" in entries:
        one = [G.inp("sig", pb.sig[:N].reshape(-1, d), offset=(offset or {}).get("sig", 0)), G.inp("alpha", pb.alpha[:N]), G.out("out", pb.agg[0])]
        G.on_device(ctx, one, lambda p: ctx.aggregate_core_dev(p["sig"].ptr, p["alpha"].ptr, p["out"].ptr, N, l))
    if "partial" in entries:
        G.on_device(ctx, pb.ins("sig", "alpha", offset=offset) + [pb.partial()],
                    lambda p: ctx.aggregate_partial_batch_dev(p["sig"].ptr, p["alpha"].ptr, p["partial"].ptr, ps, groups, N, l))
    if "target" in entries:
        G.on_device(ctx, pb.ins("sig", "alpha", "vkL", "vkR", "c") + [pb.partial(), pb.target()],
                    lambda p: ctx.aggregate_target_partial_batch_dev(p["sig"].ptr, p["alpha"].ptr, p["vkL"].ptr, p["vkR"].ptr, p["c"].ptr,
                                                                     p["partial"].ptr, ps, p["target"].ptr, ts, groups, N, l))
    if "sign" in entries:
        # the fused sign + aggregate: sigma is an OUTPUT (the live[r] store), with and without the target columns
        sig_out = G.out("sig", pb.signed.reshape(-1, d), offset=(offset or {}).get("sig", 0))
        G.on_device(ctx, pb.ins("sk", "c", "alpha", "vkL", "vkR") + [sig_out, pb.partial(signed=True), pb.target()],
                    lambda p: ctx.sign_aggregate_target_partial_batch_dev(p["sk"].ptr, p["c"].ptr, p["alpha"].ptr, p["vkL"].ptr, p["vkR"].ptr,
                                                                          p["sig"].ptr, p["partial"].ptr, ps, p["target"].ptr, ts, groups, N, l))
        G.on_device(ctx, pb.ins("sk", "c", "alpha") + [sig_out, pb.partial(signed=True)],
                    lambda p: ctx.sign_aggregate_target_partial_batch_dev(p["sk"].ptr, p["c"].ptr, p["alpha"].ptr, 0, 0, p["sig"].ptr,
                                                                          p["partial"].ptr, ps, 0, 0, groups, N, l))


# ---- aggregate_onepass, several slices ---------------------------------------------------------------------------------------------
# (d, l) -> AR: what the launcher's rule gives aggregates of 129 signers, one or two of them, with or without the target columns
# (nsl is capped by 129 / 24 signers per slice, so the CU count does not enter while it is at least 5 * the column blocks)
ONEPASS = {(64, 1): 4, (256, 1): 4, (256, 4): 3, (64, 13): 3, (256, 3): 2, (64, 9): 2}


@pytest.mark.parametrize("d,l", list(ONEPASS), ids=str)
def test_onepass_sliced(d, l, coracle, ctxs):
    """129 signers: several slices share the accumulator words, and the last column block is partly filled (l * d / 4 columns over
    blocks of 64 * AR).  One aggregate (aggregate_core_dev) and two (the strided entries), each at the AR the table names"""
    cu, ar = G.num_cu(), ONEPASS[(d, l)]
    for groups, target in ((1, False), (2, False), (2, True)):
        got, nsl = S.onepass_shape(cu, groups, 129, l, d, target=target)
        assert got == ar and nsl > 1, (groups, target, got, nsl)
    assert (l * (d // 4)) % (64 * ar) != 0
    assert not S.direct_taken(-1, 2, 129, d)
    ctx = _ctx(ctxs, d, -1)
    _equal_sizes(ctx, Problem(coracle, [129, 129], l, d, 10 * d + l))


# ---- aggregate_onepass, one slice ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target", [False, True], ids=["plain", "target"])
def test_onepass_one_slice(target, coracle, ctxs):
    """more tiles than CUs: one slice per aggregate, AR = 2 (cu + 1 aggregates of 24 signers, l = 1, degree 64)"""
    cu, d, N = G.num_cu(), 64, 24
    groups = cu // 2 + 1 if target else cu + 1
    assert S.onepass_shape(cu, groups, N, 1, d, target=target) == (2, 1)
    ctx = _ctx(ctxs, d, -1)
    _equal_sizes(ctx, Problem(coracle, [N] * groups, 1, d, 77 + target), entries=("target", "sign") if target else ("partial", "sign"))


# ---- aggregate_direct ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 256])
@pytest.mark.parametrize("knob,l", [(2, 1), (2, 3), (4, 1), (4, 3), (4, 5)], ids=str)
def test_direct(knob, l, d, coracle, ctxs):
    """R rows per tile: l = 1, 3 (R = 2) and 1, 3, 5 (R = 4) leave the `k >= l` rows of the last tile; 1, 4 and 33 signers: fewer
    than a wave's four, one round, a second round of one signer"""
    ctx = _ctx(ctxs, d, knob)
    for N in (1, 4, 33):
        assert S.direct_taken(knob, 2, N, d) and S.direct_taken(knob, 2, N, d, target=True)
        _equal_sizes(ctx, Problem(coracle, [N, N], l, d, 100 * knob + 10 * l + N), entries=("core", "partial", "target"))


def test_direct_by_default_for_small_launches(coracle, ctxs):
    """without the knob: up to 128 signers per launch and no target columns"""
    assert S.direct_taken(0, 2, 33, 64) and not S.direct_taken(0, 2, 33, 64, target=True) and not S.direct_taken(0, 2, 65, 64)
    ctx = _ctx(ctxs, 64)
    _equal_sizes(ctx, Problem(coracle, [33, 33], 3, 64, 5))


# ---- aggregate_generic_kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 9])
def test_generic_degree_12(N, coracle, ctxs):
    """a ring-only context of degree 12: not a power of two, so every entry takes the generic kernel (the fused sign + aggregate its
    two launches)"""
    ctx = _ctx(ctxs, 12)
    _equal_sizes(ctx, Problem(coracle, [N, N], 3, 12, 300 + N))


def test_generic_unaligned_signatures(coracle, ctxs):
    """degree 64, the signatures 4 bytes off: aggregate_generic_kernel (agg_tiled wants 16-byte rows) where the entry allows it;
    fz_aggregate_target_partial_batch wants every input aligned and refuses, writing nothing"""
    ctx, d, l, N = _ctx(ctxs, 64), 64, 3, 9
    pb = Problem(coracle, [N, N], l, d, 400)
    _equal_sizes(ctx, pb, entries=("core", "partial", "sign"), offset={"sig": 4})
    ops = pb.ins("sig", "alpha", "vkL", "vkR", "c", offset={"sig": 4}) + [pb.partial(), pb.target()]
    G.refused(ctx, ops, lambda p: ctx.aggregate_target_partial_batch_dev(p["sig"].ptr, p["alpha"].ptr, p["vkL"].ptr, p["vkR"].ptr, p["c"].ptr,
                                                                         p["partial"].ptr, l * d + PAD, p["target"].ptr, d + TPAD, 2, N, l),
              BADARG)


# ---- ragged ------------------------------------------------------------------------------------------------------------------------------
def _ragged(ctx, pb):
    l, d = pb.l, pb.d
    ps, ts = l * d + PAD, d + TPAD
    G.on_device(ctx, pb.ins("sig", "alpha") + [G.out("out", pb.agg.reshape(-1, d))],
                lambda p: ctx.aggregate_core_ragged_dev(p["sig"].ptr, p["alpha"].ptr, pb.off, l, p["out"].ptr))
    G.on_device(ctx, pb.ins("sig", "alpha", "vkL", "vkR", "c") + [pb.partial(), pb.target()],
                lambda p: ctx.aggregate_target_partial_ragged_dev(p["sig"].ptr, p["alpha"].ptr, p["vkL"].ptr, p["vkR"].ptr, p["c"].ptr, pb.off, l,
                                                                  p["partial"].ptr, ps, p["target"].ptr, ts))
    # targets only: d_sig = d_partial = 0
    G.on_device(ctx, pb.ins("alpha", "vkL", "vkR", "c") + [pb.target()],
                lambda p: ctx.aggregate_target_partial_ragged_dev(0, p["alpha"].ptr, p["vkL"].ptr, p["vkR"].ptr, p["c"].ptr, pb.off, l,
                                                                  0, 0, p["target"].ptr, ts))


@pytest.mark.parametrize("direct", [-1, None], ids=["onepass", "default"])
@pytest.mark.parametrize("d", [64, 256])
def test_ragged_sizes_with_an_empty_aggregate(d, direct, coracle, ctxs):
    assert direct is None or not S.direct_taken(direct, 4, 17, d)
    _ragged(_ctx(ctxs, d, direct), Problem(coracle, [5, 0, 1, 17], 3, d, 500 + d))


@pytest.mark.parametrize("direct", [-1, None], ids=["onepass", "default"])
@pytest.mark.parametrize("d", [64, 256])
def test_ragged_across_the_64_aggregate_seam(d, direct, coracle, ctxs):
    """70 aggregates of 1 .. 5 signers: two launches, the second at d_partial + 64 * partial_stride and d_target + 64 * target_stride
    with both strides larger than the rows; the arena's gap words on both sides of aggregate 63 / 64 are checked like every other"""
    sizes = [1 + (g * 7) % 5 for g in range(70)]
    pb = Problem(coracle, sizes, 2, d, 600 + d)
    assert len({int(pb.agg[g, 0, 0]) for g in (62, 63, 64, 65)}) == 4          # neighbours differ: a shifted aggregate would show
    _ragged(_ctx(ctxs, d, direct), pb)


# ---- target_kernel -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 4], ids=["aligned", "plus4"])
@pytest.mark.parametrize("N", [1, 7, 9])
@pytest.mark.parametrize("d", [12, 64, 256])
def test_target_kernel(d, N, offset, coracle, ctxs):
    """target_partial_dev (one aggregate) and target_partial_batch_dev (two, a stride gap between them); 7 and 9 signers: one and
    two slices of the signers (at least eight per thread), the second slice of one signer"""
    ctx = _ctx(ctxs, d)
    pb = Problem(coracle, [N, N], 1, d, 700 + d + N)
    off = {n: offset for n in ("vkL", "vkR", "c", "alpha")}
    one = [G.inp(n, getattr(pb, n)[:N], offset=offset) for n in ("vkL", "vkR", "c", "alpha")] + [G.out("target", pb.tgt[:1], canon=CANON)]
    G.on_device(ctx, one, lambda p: ctx.target_partial_dev(p["vkL"].ptr, p["vkR"].ptr, p["c"].ptr, p["alpha"].ptr, p["target"].ptr, N))
    G.on_device(ctx, pb.ins("vkL", "vkR", "c", "alpha", offset=off) + [pb.target()],
                lambda p: ctx.target_partial_batch_dev(p["vkL"].ptr, p["vkR"].ptr, p["c"].ptr, p["alpha"].ptr, p["target"].ptr, d + TPAD, 2, N))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_write_nothing(coracle, ctxs):
    d, l, N = 64, 2, 3
    ctx = _ctx(ctxs, d)
    pb = Problem(coracle, [N, N], l, d, 800)
    ps, ts = l * d + PAD, d + TPAD
    every = pb.ins("sig", "alpha", "vkL", "vkR", "c", "sk") + [G.out("out", pb.agg[0]), pb.partial(), pb.target()]
    P = lambda p, n: p[n].ptr                                                   # noqa: E731
    G.refused(ctx, every, lambda p: ctx.aggregate_core_dev(P(p, "sig"), P(p, "alpha"), P(p, "out"), N, 0), BADARG)
    G.refused(ctx, every, lambda p: ctx.aggregate_partial_batch_dev(P(p, "sig"), P(p, "alpha"), P(p, "partial"), l * d - 1, 2, N, l), BADARG)
    G.refused(ctx, every, lambda p: ctx.aggregate_target_partial_batch_dev(P(p, "sig"), P(p, "alpha"), P(p, "vkL"), P(p, "vkR"), P(p, "c"),
                                                                           P(p, "partial"), ps, P(p, "target"), d - 1, 2, N, l), BADARG)
    G.refused(ctx, every, lambda p: ctx.sign_aggregate_target_partial_batch_dev(P(p, "sk"), P(p, "c"), P(p, "alpha"), P(p, "vkL"), 0, P(p, "sig"),
                                                                                P(p, "partial"), ps, P(p, "target"), ts, 2, N, l), BADARG)
    G.refused(ctx, every, lambda p: ctx.aggregate_core_ragged_dev(P(p, "sig"), P(p, "alpha"), [0, 3, 2], l, P(p, "out")), BADARG)
    G.refused(ctx, every, lambda p: ctx.aggregate_target_partial_ragged_dev(P(p, "sig"), P(p, "alpha"), P(p, "vkL"), P(p, "vkR"), P(p, "c"), [0, 3, 6], l,
                                                                            P(p, "partial"), l * d - 1, P(p, "target"), ts), BADARG)
    G.refused(ctx, every, lambda p: ctx.target_partial_batch_dev(P(p, "vkL"), P(p, "vkR"), P(p, "c"), P(p, "alpha"), P(p, "target"), d - 1, 2, N), BADARG)
    G.refused(ctx, every, lambda p: ctx.target_partial_dev(0, P(p, "vkR"), P(p, "c"), P(p, "alpha"), P(p, "target"), N), BADARG)
    # the ragged launches have no generic kernel: a ring-only degree is refused as unsupported
    ctx12 = _ctx(ctxs, 12)
    pb12 = Problem(coracle, [N, N], l, 12, 801)
    G.refused(ctx12, pb12.ins("sig", "alpha") + [G.out("out", pb12.agg.reshape(-1, 12))],
              lambda p: ctx12.aggregate_core_ragged_dev(P(p, "sig"), P(p, "alpha"), pb12.off, l, P(p, "out")), UNSUPPORTED)
