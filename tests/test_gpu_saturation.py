"""The lazily reduced sums of every accumulating kernel, driven to their documented bounds with int32 (and int64) extremes and
compared bit for bit with closed-form expectations (tests/_saturation.py; checked against the oracles and shown adversarial
in tests/test_saturation_host.py).  Each path is forced through its knob at context creation:

- aggregation: aggregate_onepass and aggregate_direct (FZ_AGG_DIRECT = -1 | 2 | 4 | default), int32 and int64 outputs, with
  and without the target columns, ragged, the fused sign + aggregate, target_kernel, the generic kernel of a ring-only
  context; signer counts on both sides of the 16-signer fold, one slice per aggregate with 65 signers per lane, 130 per lane
  in aggregate_direct, and the sliced launch run twice (its accumulator words re-arm after saturated sums);
- matvec: FZ_MATVEC_SLICES = -1 .. 16 on both sides of `small` (l <= 32) and of the integer form's guard (l <= 32768), and at
  l = 65538, where an int64 sum of saturating products leaves int64;
- keygen_fused (integer and fp64 forms) and keygen_bcast_fused with secrets whose transform is (q - 3) / 2 everywhere;
- verify_fused from saturating raw rows (the exact target: verdict 4, never 3; one coefficient off: 3) and from int64 partial
  sums at the int64 extremes, on both sides of its `small` flag and with 65 rows per lane.

Reference arithmetic: fusion/fusion.py:363-370 (keygen), :557 (sign), :670-676 (aggregate), :706-727 (verify)."""
import os

import numpy as np
import pytest

from oracle import oracle as O

import _saturation as S

pytestmark = pytest.mark.gpu

AGG_KNOBS = [{"FZ_AGG_DIRECT": "-1"}, {"FZ_AGG_DIRECT": "2"}, {"FZ_AGG_DIRECT": "4"}, {}]
# (name, q, d, root, inv_root): both parameter sets, and a ring-only context with a modulus above 2^31
RINGS = {
    "128": (O.PRIME, 64, O.PARAMS[128]["root"], O.PARAMS[128]["inv_root"]),
    "256": (O.PRIME, 256, O.PARAMS[256]["root"], O.PARAMS[256]["inv_root"]),
    "wide256": (S.Q_WIDE, 256, 0, 0),
}


def _ident(env):
    return ",".join(f"{k[3:]}={v}" for k, v in env.items()) or "defaults"


def _ctx(ring, env=None):
    import fusion_hip
    q, d, root, inv = ring
    env = env or {}
    for k, v in env.items():
        os.environ[k] = v
    try:
        return fusion_hip.Context(q, d, root, inv)
    finally:
        for k in env:
            os.environ.pop(k, None)


def _num_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


class _Dev:
    """device copies of numpy arrays, freed together"""

    def __init__(self, ctx):
        self.ctx, self.bufs = ctx, []

    def put(self, a):
        import fusion_hip
        b = fusion_hip.DeviceArray.from_numpy(self.ctx, np.ascontiguousarray(a))
        self.bufs.append(b)
        return b

    def new(self, shape, dtype=np.int32):
        import fusion_hip
        b = fusion_hip.DeviceArray(self.ctx, shape, dtype)
        self.bufs.append(b)
        return b

    def free(self):
        for b in self.bufs:
            b.free()
        self.bufs = []


def _c(a, q):
    return S.cent_arr(a, q)


# ---- aggregation --------------------------------------------------------------------------------------------------------
def _check_aggregate_paths(ctx, ring, n, l, runs=1):
    """every output form of one aggregate of n signers: int32, int64 partials (two groups), with the target columns, ragged,
    target_kernel, the fused sign + aggregate"""
    q, d = ring[0], ring[1]
    sig, alpha = S.agg_inputs(n, l, d)
    want, twant = S.agg_expected(n, l, d, q), S.target_expected(n, d, q)
    vkL, vkR, c = S.target_inputs(n, d)
    dev = _Dev(ctx)
    try:
        dS, dA = dev.put(sig), dev.put(alpha)
        dS2, dA2 = dev.put(np.concatenate([sig, sig])), dev.put(np.concatenate([alpha, alpha]))
        dL2, dR2, dC2 = dev.put(np.concatenate([vkL, vkL])), dev.put(np.concatenate([vkR, vkR])), dev.put(np.concatenate([c, c]))
        dO, dP, dT = dev.new((l, d)), dev.new((2, l, d), np.int64), dev.new((2, d), np.int64)
        for run in range(runs):
            ctx.aggregate_core_dev(dS.ptr, dA.ptr, dO.ptr, n, l)
            assert np.array_equal(dO.numpy(), want), ("int32", n, run)
            ctx.aggregate_partial_batch_dev(dS2.ptr, dA2.ptr, dP.ptr, l * d, 2, n, l)
            assert np.array_equal(_c(dP.numpy(), q), np.stack([want, want])), ("partial", n, run)
            ctx.aggregate_target_partial_batch_dev(dS2.ptr, dA2.ptr, dL2.ptr, dR2.ptr, dC2.ptr, dP.ptr, l * d, dT.ptr, d, 2, n, l)
            assert np.array_equal(_c(dP.numpy(), q), np.stack([want, want])), ("partial+target", n, run)
            assert np.array_equal(_c(dT.numpy(), q), np.stack([twant, twant])), ("target", n, run)
        # target_kernel
        ctx.h2d(dT.ptr, np.full((2, d), 12345, dtype=np.int64))          # target_partial zeroes what it accumulates into
        ctx.target_partial_batch_dev(dL2.ptr, dR2.ptr, dC2.ptr, dA2.ptr, dT.ptr, d, 2, n)
        assert np.array_equal(_c(dT.numpy(), q), np.stack([twant, twant])), ("target_kernel", n)
        # ragged: this aggregate, one of 17 and one of 1 signer
        sizes = [n, 17, 1]
        parts = [S.agg_inputs(m, l, d) for m in sizes]
        keys = [S.target_inputs(m, d) for m in sizes]
        off = np.concatenate([[0], np.cumsum(sizes)]).tolist()
        rS, rA = dev.put(np.concatenate([p[0] for p in parts])), dev.put(np.concatenate([p[1] for p in parts]))
        rL, rR, rC = (dev.put(np.concatenate([k[i] for k in keys])) for i in range(3))
        rO, rP, rT = dev.new((3, l, d)), dev.new((3, l, d), np.int64), dev.new((3, d), np.int64)
        rwant = np.stack([S.agg_expected(m, l, d, q) for m in sizes])
        rtwant = np.stack([S.target_expected(m, d, q) for m in sizes])
        if d in (64, 256):                                  # (ragged launches: power-of-two degrees <= 256)
            ctx.aggregate_core_ragged_dev(rS.ptr, rA.ptr, off, l, rO.ptr)
            assert np.array_equal(rO.numpy(), rwant), ("ragged int32", n)
            ctx.aggregate_target_partial_ragged_dev(rS.ptr, rA.ptr, rL.ptr, rR.ptr, rC.ptr, off, l, rP.ptr, l * d, rT.ptr, d)
            assert np.array_equal(_c(rP.numpy(), q), rwant), ("ragged partial", n)
            assert np.array_equal(_c(rT.numpy(), q), rtwant), ("ragged target", n)
        # the fused sign + aggregate: sigma = cent(cent(L * c) + R) of extremes, written out and aggregated
        sk, ch, sg = S.sign_inputs(n, l, d, q)
        kS, kC, kOut = dev.put(sk), dev.put(ch), dev.new((n, l, d))
        ctx.sign_aggregate_target_partial_batch_dev(kS.ptr, kC.ptr, dA.ptr, dL2.ptr, dR2.ptr, kOut.ptr, dP.ptr, l * d, dT.ptr, d,
                                                    1, n, l)
        assert np.array_equal(kOut.numpy(), sg), ("signed", n)
        assert np.array_equal(_c(dP.numpy()[0], q), S.sign_agg_expected(n, l, d, q)), ("sign+aggregate", n)
        assert np.array_equal(_c(dT.numpy()[0], q), twant), ("sign+aggregate target", n)
    finally:
        dev.free()


@pytest.mark.parametrize("env", AGG_KNOBS, ids=_ident)
@pytest.mark.parametrize("ring", list(RINGS), ids=str)
def test_aggregation_around_the_fold(ring, env):
    """signer counts on both sides of the fold cadence, and 300 at rank 83 (several slices: shared accumulator words), the
    sliced launches run twice"""
    ctx = _ctx(RINGS[ring], env)
    try:
        for n in (15, 16, 17, 48, 49, 64, 65, 129):
            _check_aggregate_paths(ctx, RINGS[ring], n, 3)
        if ring != "128":
            assert S.onepass_shape(_num_cu(), 1, 300, 83, 256)[1] > 1
            _check_aggregate_paths(ctx, RINGS[ring], 300, 83, runs=2)
    finally:
        ctx.close()


@pytest.mark.parametrize("q", [O.PRIME, S.Q_WIDE])
def test_generic_kernel_ring_only(q):
    """degree 12 (a ring-only context: not a power of two): aggregate_generic_kernel, its target columns, target_kernel"""
    ring = (q, 12, 0, 0)
    ctx = _ctx(ring)
    try:
        for n in (16, 17, 65, 129, 700):
            _check_aggregate_paths(ctx, ring, n, 3)
    finally:
        ctx.close()


def test_onepass_one_slice_65_per_lane():
    """257 aggregates (129 with the target columns) at degree 64, l = 1: one slice per aggregate, so 8 signers per round of
    a workgroup -- 15, 16, 17 and 65 signers per lane.  At 65, the lo columns' unfolded sums pass 2^53 (odd products)."""
    ring = RINGS["128"]
    q, d = ring[0], ring[1]
    cu = _num_cu()
    ctx = _ctx(ring)
    try:
        for n in (120, 128, 136, 520):
            for groups, target in ((cu + 1, False), (cu // 2 + 1, True)):           # more tiles than CUs: one slice each
                assert S.onepass_shape(cu, groups, n, 1, d, target=target)[1] == 1
                lanes = S.onepass_lanes(n, 1)
                assert S.max_lane_products(lanes) == n // 8
                if n == 520:
                    assert S.agg_fold_free_error(lanes, 0, n) % q != 0            # adversarial at this device's shape
                sig, alpha = S.agg_inputs(n, 1, d)
                want, twant = S.agg_expected(n, 1, d, q), S.target_expected(n, d, q)
                vkL, vkR, c = S.target_inputs(n, d)
                rep = lambda a: np.broadcast_to(a, (groups,) + a.shape).reshape((groups * a.shape[0],) + a.shape[1:])  # noqa: E731
                dev = _Dev(ctx)
                try:
                    dS, dA, dP = dev.put(rep(sig)), dev.put(rep(alpha)), dev.new((groups, d), np.int64)
                    if target:
                        dL, dR, dC, dT = dev.put(rep(vkL)), dev.put(rep(vkR)), dev.put(rep(c)), dev.new((groups, d), np.int64)
                        ctx.aggregate_target_partial_batch_dev(dS.ptr, dA.ptr, dL.ptr, dR.ptr, dC.ptr, dP.ptr, d, dT.ptr, d,
                                                               groups, n, 1)
                        assert np.array_equal(_c(dT.numpy(), q), np.broadcast_to(twant, (groups, d))), (n, "target")
                    else:
                        ctx.aggregate_partial_batch_dev(dS.ptr, dA.ptr, dP.ptr, d, groups, n, 1)
                    assert np.array_equal(_c(dP.numpy(), q), np.broadcast_to(want[0], (groups, d))), (n, groups)
                finally:
                    dev.free()
    finally:
        ctx.close()


@pytest.mark.parametrize("env", AGG_KNOBS, ids=_ident)
@pytest.mark.parametrize("secpar", [128, 256])
def test_aggregation_long_lanes(secpar, env):
    """one aggregate of 4145 signers: aggregate_direct (FZ_AGG_DIRECT = 2 | 4) puts 129-130 into each lane's sums -- both the
    lo and the odd hi columns pass 2^53 unfolded; the sliced kernel (default, -1) takes it in slices"""
    ring = RINGS[str(secpar)]
    q, d = ring[0], ring[1]
    n = 4145
    if S.direct_taken(int(env.get("FZ_AGG_DIRECT", "0")), 1, n, d):
        lanes = S.direct_lanes(n)
        assert S.max_lane_products(lanes) == 130
        assert all(S.agg_fold_free_error(lanes, p, n) % q for p in range(S.NPAT) if S.AGG_PATTERNS[p][0] in ("lo+", "hi_odd+"))
    ctx = _ctx(ring, env)
    try:
        _check_aggregate_paths(ctx, ring, n, 3, runs=2)
    finally:
        ctx.close()


# ---- matvec -------------------------------------------------------------------------------------------------------------
MATVEC_SLICES = (-1, 0, 1, 2, 4, 8, 16)


def _matvec_all_knobs(ring, l, batch=3):
    q, d = ring[0], ring[1]
    A, Sb = S.mv_inputs(l, d, batch)
    want = np.broadcast_to(S.mv_expected(l, d, q), (batch, d))
    for k in MATVEC_SLICES:
        ctx = _ctx(ring, {"FZ_MATVEC_SLICES": str(k)})
        try:
            assert np.array_equal(ctx.matvec(A, Sb), want), (l, k)
        finally:
            ctx.close()


@pytest.mark.parametrize("ring,l", [(r, l) for r in ("128", "256") for l in (32, 33, 100, 32768, 32769)] +
                         [("wide256", l) for l in (32, 33, 100)], ids=str)
def test_matvec_either_side_of_small_and_the_guard(ring, l):
    _matvec_all_knobs(RINGS[ring], l)


@pytest.mark.parametrize("l", [65537, 65538])
def test_matvec_beyond_int64(l):
    """l = 65538 rows of |y * lo| = 2^47 - 2^31: an int64 sum of them leaves int64 (65537 still fit) -- the fp64 kernels must
    take them.  Degree 64 (A and the batch of 3: 17 and 50 MiB)."""
    assert S.outside_int64(S.mv_totals(65538)[1][1])
    _matvec_all_knobs(RINGS["128"], l)


# ---- keygen -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("no_imad", [False, True], ids=["imad", "fp64"])
@pytest.mark.parametrize("secpar", [128, 256])
def test_keygen_saturating_secrets(secpar, no_imad):
    """every secret row [v, 0, .., 0], v = (q - 3) / 2 (its transform: v in every coefficient), the other half -v: at l = 32 * 4
    task rows (the edge of `small`), one above it, and long enough for 129 products of |v| * 0xffff per lane"""
    ring = RINGS[str(secpar)]
    q, d = ring[0], ring[1]
    v = S.odd_half_q(q)
    edge = 128 * (256 // d)
    ctx = _ctx(ring, {"FZ_NO_IMAD": "1"} if no_imad else {})
    try:
        for l in (edge, edge + 1, 129 * 4 * (256 // d)):
            n = 2
            A, coef = S.keygen_A(l, d), S.impulse_rows(n, l, d, v)
            want = np.broadcast_to(S.keygen_expected(l, d, q, v), (n, 2, d))
            if not no_imad and l > edge + 1:
                assert S.keygen_lane_error(l, d, q, v, 0) % q != 0
            dev = _Dev(ctx)
            try:
                dA, dC, dS, dV = dev.put(A), dev.put(coef), dev.new(coef.shape), dev.new((n, 2, d))
                ctx.keygen_core_dev(dA.ptr, dC.ptr, dS.ptr, dV.ptr, n, l)
                sk = dS.numpy()
                assert (sk[:, 0] == v).all() and (sk[:, 1] == -v).all(), l
                assert np.array_equal(dV.numpy(), want), (l, "keygen")
                dP = dev.put(np.ascontiguousarray(coef[:, :, 0, :]))
                ctx.h2d(dV.ptr, np.zeros((n, 2, d), dtype=np.int32))
                ctx.keygen_core_bcast_dev(dA.ptr, dP.ptr, dS.ptr, dV.ptr, n, l)
                assert np.array_equal(dV.numpy(), want), (l, "bcast")
                assert (dS.numpy()[:, 0] == v).all(), l
            finally:
                dev.free()
    finally:
        ctx.close()


# ---- verify -------------------------------------------------------------------------------------------------------------
VERIFY_KNOBS = [{}, {"FZ_NO_IMAD": "1"}, {"FZ_VERIFY_CENT": "1"}]
# (degree, l, groups): the edge of `small` (32 rows per lane) and one above it; 65 rows per lane; degree 64 at its edge
# (32768 rows) and one above (beyond 2^15 rows: the fp64 form)
VERIFY_CASES = [(256, 8192, 1), (256, 8193, 1), (256, 16640, 2), (64, 32768, 1), (64, 32769, 1)]


@pytest.mark.parametrize("env", VERIFY_KNOBS, ids=_ident)
@pytest.mark.parametrize("case", VERIFY_CASES, ids=lambda c: f"d{c[0]}-l{c[1]}-g{c[2]}")
def test_verify_saturating_rows(case, env):
    """raw int32 extremes in every row of the signature and of A: with the exact product as the target the verdict is the
    norm code, 4 (never 3); with one target coefficient off by one it is 3"""
    d, l, groups = case
    ring = RINGS["128" if d == 64 else "256"]
    q = ring[0]
    P = O.PARAMS[128 if d == 64 else 256]
    R, imad, small, lanes = S.verify_shape(l, d, groups, _num_cu(), no_imad="FZ_NO_IMAD" in env)
    if (d, l) == (256, 16640) and imad:
        assert not small and S.max_lane_products(lanes) == 65 and S.imad_small_error(lanes, l, 0) % q != 0
    A, Sb = S.mv_inputs(l, d, groups)
    target = np.broadcast_to(S.mv_expected(l, d, q), (groups, d)).astype(np.int32)
    bad = target.copy()
    bad[:, 7] += 1 if bad[0, 7] < 0 else -1
    ctx = _ctx(ring, env)
    dev = _Dev(ctx)
    try:
        dA, dS, dT, dB = dev.put(A), dev.put(Sb), dev.put(target), dev.put(bad)
        assert ctx.verify_with_target_batch_dev(dA.ptr, dS.ptr, dT.ptr, groups, l, P["beta_vf"], d) == [4] * groups
        assert ctx.verify_with_target_batch_dev(dA.ptr, dS.ptr, dB.ptr, groups, l, P["beta_vf"], d) == [3] * groups
    finally:
        dev.free()
        ctx.close()


@pytest.mark.parametrize("env", VERIFY_KNOBS, ids=_ident)
@pytest.mark.parametrize("secpar", [128, 256])
def test_verify_int64_partials_at_the_extremes(secpar, env):
    """int64 partial rows holding INT64_MIN / MAX (centred on load, fz_cent_i64) and targets within q of INT64_MAX / MIN"""
    ring = RINGS[str(secpar)]
    q, d = ring[0], ring[1]
    P = O.PARAMS[secpar]
    ctx = _ctx(ring, env)
    try:
        for l in (129, 8193):
            groups = 2
            A, _ = S.mv_inputs(l, d)
            rows = np.ascontiguousarray(np.broadcast_to(S.i64_rows(l, d), (groups, l, d)))
            t = S.i64_expected(A, l, d, q)
            tgt = np.array([[S.far_representative(x, q, top=(g == 0)) for x in t] for g in range(groups)], dtype=np.int64)
            bad = tgt.copy()
            bad[0, 5] -= 1                                             # within q of INT64_MAX: one down
            bad[1, 5] += 1                                             # within q of INT64_MIN: one up
            dev = _Dev(ctx)
            try:
                dA, dS, dT, dB, dV = dev.put(A), dev.put(rows), dev.put(tgt), dev.put(bad), dev.new((groups,))
                ctx.verify_partials_batch_async_dev(dA.ptr, dS.ptr, l * d, dT.ptr, d, groups, l, P["beta_vf"], d, dV.ptr)
                assert dV.numpy().tolist() == [4] * groups, l
                ctx.verify_partials_batch_async_dev(dA.ptr, dS.ptr, l * d, dB.ptr, d, groups, l, P["beta_vf"], d, dV.ptr)
                assert dV.numpy().tolist() == [3] * groups, l
            finally:
                dev.free()
    finally:
        ctx.close()
