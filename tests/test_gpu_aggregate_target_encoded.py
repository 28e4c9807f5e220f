"""Many committees' aggregates and verification targets straight from the compact bytes in one launch, on the device
(fz_aggregate_target_encoded_ragged_async, BatchScheme.aggregate_verify_encoded / aggregate_verify_many_encoded,
fusion.fusion.aggregate_verify_from_bytes / aggregate_verify_many_from_bytes).

Every entry case is held, bit for bit on int64, to the two calls the entry replaces, run on the same device arrays:
fz_aggregate_encoded_ragged_async for the aggregates' partials and d_out, and fz_aggregate_target_partial_ragged with d_sig == NULL
on the compacted non-skipped rows for the targets' partials (a call whose every signer is skipped has nothing to hand that oracle:
the entry's contract says zero).  Both kinds of partials lie stride = width + 2 words apart inside 16 KiB guards of sentinels, as
does d_out, and every word that is not an output is found as it was.  Contexts: the scheme's two parameter sets (the 4-op multiply)
and q = 4294828033 at either degree (the 6-op multiply).  All four instantiations run here, but the "top" contexts are compared with
sibling kernels only -- the aggregates share aggregate_encoded_slice with their oracle, the targets agg_target4 with theirs, so a
mistake in a shared piece cancels out; what these comparisons say is that both entries leave the same int64 words.  The kernels are
held to the spec at the 6-op form, at moduli at or above 2^31 and at every field width in tests/test_gpu_many_encoded_edges.py.  The
scheme cases run the reference-made flows of tests/golden/scheme_many_*.  No tolerance anywhere."""
import functools
import json
import os

import numpy as np
import pytest

import _encoded_edges as EE
from test_encoding_host import TABLE, spec_pack
from test_gpu_encoding import scheme, set_field

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
GUARD = 16384                                              # bytes on either side of every output (tests/_guarded.py's)
P_FILL, O_FILL = 0x5a5a5a5a5a5a5a5a, 0x5a5a5a5a
BOUNDS = {256: 3172, 64: 4264}                            # the bound of one signature at the degree's parameter set
FULL_L = {256: 83, 64: 195}
CONTEXTS = [("scheme", 256), ("scheme", 64), ("top", 256), ("top", 64)]
_TOP = {}


def context(kind, d):
    """-> (context, q): the scheme's own at this degree, or one on q = 4294828033 (above 2^31: the 6-op multiply)"""
    from fusion_hip import Context
    if kind == "scheme":
        bs = scheme(256 if d == 256 else 128)[1]
        assert bs.d == d
        return bs.ctx, bs.q
    if d not in _TOP:
        q, r, ir = EE.root_of(("top", "root"), d)
        _TOP[d] = Context(q, d, r, ir)
    return _TOP[d], EE.Q_TOP


def inputs(q, d, l, n, seed, extreme=False):
    """n canonical records of l rows at the degree's bound with the fields 0 and 2B among them, alpha_hat / vk / c_hat rows: random
    centred residues with the int32 extremes among the first rows, or (extreme) the int32 extremes on every coefficient and
    every field at 0 or 2B"""
    rng = np.random.default_rng(seed)
    B, h = BOUNDS[d], (q - 1) // 2
    u = rng.integers(0, 2 * B + 1, size=(n, l, d), dtype=np.int64)
    rows = {k: rng.integers(-h, h + 1, size=shape, dtype=np.int64) for k, shape in (("alpha", (n, d)), ("vk", (n, 2, d)), ("chal", (n, d)))}
    if extreme:
        u = rng.integers(0, 2, size=(n, l, d), dtype=np.int64) * 2 * B
        rows = {k: np.where(rng.integers(0, 2, size=v.shape) == 1, I32_MAX, I32_MIN) for k, v in rows.items()}
    elif n:
        u[0, 0, 0], u[-1, -1, -1], u[n // 2, 0, 1], u[n // 2, -1, -2] = 0, 2 * B, 2 * B, 0
        for i in range(min(n, 4)):
            for k, v in rows.items():
                v[i].flat[::3] = [I32_MIN, I32_MAX, h, -h][(i + len(k)) % 4]
    data = spec_pack(u - B, B, (2 * B).bit_length())
    return data, rows["alpha"].astype(np.int32), rows["vk"].astype(np.int32), rows["chal"].astype(np.int32)


class Guarded:
    """an output of `rows` rows of `row` elements `stride` apart between two guards, sentinels everywhere"""

    def __init__(self, ctx, rows, row, stride, dtype, fill):
        from fusion_hip import DeviceArray
        self.rows, self.row, self.stride, self.fill = rows, row, stride, fill
        self.lead = GUARD // np.dtype(dtype).itemsize
        self.buf = DeviceArray.from_numpy(ctx, np.full(2 * self.lead + rows * stride, fill, dtype=dtype))
        self.ptr = self.buf.ptr + GUARD

    def read(self, written=True):
        """-> [rows][row], every other word found as it was (written=False: the rows too)"""
        a = self.buf.numpy()
        assert (a[:self.lead] == self.fill).all() and (a[self.lead + self.rows * self.stride:] == self.fill).all(), "a guard was written"
        body = a[self.lead:self.lead + self.rows * self.stride].reshape(self.rows, self.stride)
        assert (body[:, self.row:] == self.fill).all(), "a word between two rows was written"
        assert written or (body == self.fill).all(), "an output that was not asked for was written"
        return body[:, :self.row].copy()

    def dirty(self, ctx, fill):
        ctx.h2d(self.buf.ptr, np.full(2 * self.lead + self.rows * self.stride, fill, dtype=self.buf.dtype))
        self.fill = fill


def run(ctx, d, l, data, alpha, vk, chal, skip, sizes, want_out=True, oracles=True):
    """the entry on host arrays -> (partials [G][l * d] int64, targets [G][d] int64, out [G][l * d] int32); with `oracles` the same
    from the two calls it replaces, required equal"""
    from fusion_hip import DeviceArray
    g, per, B = len(sizes), l * d, BOUNDS[d]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(off[-1])
    up = lambda a: DeviceArray.from_numpy(ctx, np.ascontiguousarray(a)) if a is not None and len(a) else None      # noqa: E731
    ptr = lambda b: b.ptr if b is not None else 0                                                                 # noqa: E731
    dB, dA, dK, dC, dS = up(data), up(alpha), up(vk), up(chal), up(skip)
    outs = [Guarded(ctx, g, per, per + 2, np.int64, P_FILL), Guarded(ctx, g, d, d + 2, np.int64, P_FILL), Guarded(ctx, g, per, per, np.int32, O_FILL)]
    held = [dB, dA, dK, dC, dS] + [o.buf for o in outs]
    try:
        ctx.aggregate_target_encoded_ragged_async_dev(ptr(dB), ptr(dA), ptr(dS), ptr(dK), ptr(dC), off, l, B, outs[0].ptr, per + 2,
                                                      outs[1].ptr, d + 2, outs[2].ptr if want_out else 0)
        ctx.synchronize()
        p, t, o = outs[0].read(), outs[1].read(), outs[2].read(want_out)
        for b, a in ((dB, data), (dA, alpha), (dK, vk), (dC, chal), (dS, skip)):
            assert b is None or np.array_equal(b.numpy().ravel(), np.asarray(a).ravel()), "an input was written"
        if not oracles:
            return p, t, o
        # the aggregates: fz_aggregate_encoded_ragged_async on the same arrays
        ref = [Guarded(ctx, g, per, per + 2, np.int64, P_FILL), Guarded(ctx, g, per, per, np.int32, O_FILL)]
        held += [r.buf for r in ref]
        ctx.aggregate_encoded_ragged_async_dev(ptr(dB), ptr(dA), ptr(dS), off, l, B, ref[0].ptr, per + 2, ref[1].ptr if want_out else 0)
        ctx.synchronize()
        assert np.array_equal(p, ref[0].read()), "the aggregates' partials differ from fz_aggregate_encoded_ragged_async's"
        assert np.array_equal(o, ref[1].read(want_out)), "d_out differs from fz_aggregate_encoded_ragged_async's"
        # the targets: fz_aggregate_target_partial_ragged(d_sig = NULL) on the compacted non-skipped rows
        keep = np.arange(n) if skip is None else np.flatnonzero(np.asarray(skip) == 0)
        want = np.zeros((g, d), dtype=np.int64)
        if keep.size:
            coff = np.concatenate([[0], np.cumsum([int(((keep >= a) & (keep < b)).sum()) for a, b in zip(off, off[1:])])])
            cA, cL, cR, cC = up(alpha[keep]), up(vk[keep, 0]), up(vk[keep, 1]), up(chal[keep])
            dT = DeviceArray.from_numpy(ctx, np.full((g, d), P_FILL, dtype=np.int64))
            held += [cA, cL, cR, cC, dT]
            ctx.aggregate_target_partial_ragged_dev(0, cA.ptr, cL.ptr, cR.ptr, cC.ptr, coff, l, 0, 0, dT.ptr, d)
            ctx.synchronize()
            want = dT.numpy()
        assert np.array_equal(t, want), "the targets' partials differ from fz_aggregate_target_partial_ragged's"
        return p, t, o
    finally:
        for b in held:
            if b is not None:
                b.free()


# ---- the entry against the two calls it replaces ---------------------------------------------------------------------------
# one group of fewer than, as many as and more than the workgroup's four waves; empty groups first, last and adjacent; a group
# smaller than the launch's slice count ([40, 1] at one column: ten slices of four)
SHAPES = ([1], [4], [5], [9], [0, 1, 7], [3, 0, 0, 2], [40, 1])


@pytest.mark.parametrize("kind,d", CONTEXTS)
@pytest.mark.parametrize("l", [1, 4, 5])
def test_small_records_at_every_group_shape(kind, d, l):
    """l = 1, 4, 5: one column that is a tail, one full column, a column and a tail (d = 256; a sixteenth of that at d = 64)"""
    ctx, q = context(kind, d)
    for k, sizes in enumerate(SHAPES):
        n = sum(sizes)
        data, alpha, vk, chal = inputs(q, d, l, n, 100 * l + k)
        p, t, o = run(ctx, d, l, data, alpha, vk, chal, None, sizes)
        for g, ng in enumerate(sizes):
            assert ng or not (p[g].any() or t[g].any() or o[g].any()), (sizes, g)
        assert t.any() and np.abs(t).max() <= max(sizes) * (q // 2 + 2 ** 18)


@pytest.mark.parametrize("d", [256, 64])
def test_the_schemes_records(d):
    """l = 83 at d = 256 (21 248 values: twenty columns and a tail of 768), l = 195 at d = 64 (twelve and a tail of 192)"""
    ctx, q = context("scheme", d)
    l = FULL_L[d]
    for k, sizes in enumerate(([9], [0, 1, 7])):
        data, alpha, vk, chal = inputs(q, d, l, sum(sizes), d + k)
        run(ctx, d, l, data, alpha, vk, chal, None, sizes, want_out=bool(k))


@pytest.mark.parametrize("kind,d", CONTEXTS)
def test_skip_words(kind, d):
    """all zero (equal to NULL); every signer of one group; every signer of one slice (signers 4 .. 7 of the forty: slice 1 of ten);
    alternating; and skipped rows that would change both sums if read: fields above 2B, alpha_hat and keys at the extremes"""
    ctx, q = context(kind, d)
    l, sizes = 5, [40, 1, 6]
    n = sum(sizes)
    data, alpha, vk, chal = inputs(q, d, l, n, 7 + d)
    base = run(ctx, d, l, data, alpha, vk, chal, None, sizes, oracles=False)
    same = run(ctx, d, l, data, alpha, vk, chal, np.zeros(n, dtype=np.int32), sizes)
    assert all(np.array_equal(a, b) for a, b in zip(base, same))
    masks = {"group": np.r_[np.zeros(41), np.full(6, 6)], "lone group": np.r_[np.zeros(40), [3], np.zeros(6)],
             "slice": np.r_[np.zeros(4), np.full(4, 6), np.zeros(39)], "alternating": np.arange(n) % 2 * 6,
             "all": np.full(n, 6)}
    for name, mask in masks.items():
        skip = mask.astype(np.int32)
        x, a, k, c = data.copy(), alpha.copy(), vk.copy(), chal.copy()
        x[skip != 0], a[skip != 0], k[skip != 0], c[skip != 0] = 0xff, I32_MAX, I32_MIN, I32_MAX
        p, t, o = run(ctx, d, l, x, a, k, c, skip, sizes)
        clean = run(ctx, d, l, data, alpha, vk, chal, skip, sizes, oracles=False)
        assert all(np.array_equal(u, v) for u, v in zip((p, t, o), clean)), name      # what a skipped row holds does not matter
        if name == "group":
            assert not (p[2].any() or t[2].any() or o[2].any())
            assert np.array_equal(p[:2], base[0][:2]) and np.array_equal(t[:2], base[1][:2])
        if name == "all":
            assert not (p.any() or t.any() or o.any())


@pytest.mark.parametrize("kind,d", CONTEXTS)
def test_sixty_five_groups_run_as_two_launches(kind, d):
    ctx, q = context(kind, d)
    sizes = [1 + g % 2 for g in range(65)]
    data, alpha, vk, chal = inputs(q, d, 1, sum(sizes), 65 + d)
    p, t, o = run(ctx, d, 1, data, alpha, vk, chal, None, sizes)
    assert t[63].any() and t[64].any() and p[64].any()            # both sides of the seam


@pytest.mark.parametrize("kind,d", CONTEXTS)
def test_operands_at_the_int32_extremes_and_fields_at_their_ends(kind, d):
    ctx, q = context(kind, d)
    for l, sizes in ((5, [9, 2]), (1, [5])):
        data, alpha, vk, chal = inputs(q, d, l, sum(sizes), 31 + l, extreme=True)
        p, t, o = run(ctx, d, l, data, alpha, vk, chal, None, sizes)
        assert np.abs(t).max() <= max(sizes) * (q // 2 + 2 ** 18)


@pytest.mark.parametrize("d", [256, 64])
def test_graph_capture_replays_the_entry_onto_dirtied_partials(d):
    from fusion_hip import DeviceArray
    from fusion_hip.scheme import BatchScheme
    params, shared = scheme(256 if d == 256 else 128)
    l, sizes = 5, [5, 0, 9]
    n, per, B = sum(sizes), 5 * d, BOUNDS[d]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    data, alpha, vk, chal = inputs(shared.q, d, l, n, 3 + d)
    skip = np.zeros(n, dtype=np.int32)
    skip[6] = 6
    want = run(shared.ctx, d, l, data, alpha, vk, chal, skip, sizes)
    bs = BatchScheme(params, private_context=True)
    try:
        ctx = bs.ctx
        ins = [DeviceArray.from_numpy(ctx, a) for a in (data, alpha, skip, vk, chal)]
        outs = [Guarded(ctx, 3, per, per + 2, np.int64, P_FILL), Guarded(ctx, 3, d, d + 2, np.int64, P_FILL), Guarded(ctx, 3, per, per, np.int32, O_FILL)]
        ctx.graph_begin()
        ctx.aggregate_target_encoded_ragged_async_dev(ins[0].ptr, ins[1].ptr, ins[2].ptr, ins[3].ptr, ins[4].ptr, off, l, B, outs[0].ptr,
                                                      per + 2, outs[1].ptr, d + 2, outs[2].ptr)
        graph = ctx.graph_end()
        for fill64, fill32 in ((0x0123456789abcdef, 0x01234567), (-1, -1)):      # the clears are part of the captured work
            outs[0].dirty(ctx, fill64), outs[1].dirty(ctx, fill64), outs[2].dirty(ctx, fill32)
            graph.launch()
            ctx.synchronize()
            got = [x.read() for x in outs]
            assert all(np.array_equal(a, b) for a, b in zip(got, want))
        graph.destroy()
        for b in ins + [x.buf for x in outs]:
            b.free()
    finally:
        bs.close()


def test_refusals_behind_the_binding_write_nothing():
    """a group of 2^22 signers, by its offsets alone (the sums would no longer be exact); the targets' own rules; groups == 0"""
    from fusion_hip import DeviceArray, FusionHipError
    from fusion_hip._lib import FZ_E_BADARG, FZ_E_UNSUPPORTED
    ctx, q = context("scheme", 64)
    d, l, B = 64, 2, 5
    dB = DeviceArray.from_numpy(ctx, np.zeros(4096, dtype=np.uint8))
    dA, dC = (DeviceArray.from_numpy(ctx, np.zeros((4, d), dtype=np.int32)) for _ in range(2))
    dK = DeviceArray.from_numpy(ctx, np.zeros((4, 2, d), dtype=np.int32))
    outs = [Guarded(ctx, 2, l * d, l * d + 2, np.int64, P_FILL), Guarded(ctx, 2, d, d + 2, np.int64, P_FILL), Guarded(ctx, 2, l * d, l * d, np.int32, O_FILL)]
    call = ctx.aggregate_target_encoded_ragged_async_dev
    good = dict(b=dB.ptr, a=dA.ptr, k=dK.ptr, c=dC.ptr, off=[0, 1, 2], ps=l * d + 2, t=outs[1].ptr, ts=d + 2)
    try:
        cases = [(dict(off=[0, 2 ** 22, 2 ** 22 + 1]), FZ_E_UNSUPPORTED), (dict(off=[0, 2, 1]), FZ_E_BADARG), (dict(k=0), FZ_E_BADARG),
                 (dict(c=0), FZ_E_BADARG), (dict(k=dK.ptr + 8), FZ_E_BADARG), (dict(c=dC.ptr + 4), FZ_E_BADARG), (dict(t=outs[1].ptr + 4), FZ_E_BADARG),
                 (dict(ts=d - 2), FZ_E_BADARG), (dict(ts=d + 1), FZ_E_BADARG), (dict(ps=l * d + 1), FZ_E_BADARG)]
        for change, code in cases:
            a = dict(good, **change)
            with pytest.raises(FusionHipError) as e:
                call(a["b"], a["a"], 0, a["k"], a["c"], a["off"], l, B, outs[0].ptr, a["ps"], a["t"], a["ts"], outs[2].ptr)
            assert e.value.code == code, change
        call(dB.ptr, dA.ptr, 0, dK.ptr, dC.ptr, [0], l, B, outs[0].ptr, l * d + 2, outs[1].ptr, d + 2, outs[2].ptr)      # groups == 0
        ctx.synchronize()
        for x in outs:
            x.read(written=False)
    finally:
        for b in [dB, dA, dC, dK] + [x.buf for x in outs]:
            b.free()


# ---- the scheme: the reference-made flows of tests/golden/scheme_many_* -------------------------------------------------------
@functools.lru_cache(maxsize=None)
def flow(secpar):
    """the golden flow's scheme, keys, messages, signature records and reference-made aggregates (32 signers at secpar 128, 16 at 256)"""
    import fusion.fusion as F
    from fusion_hip.scheme import BatchScheme
    S = np.load(os.path.join(G, f"scheme_many_{secpar}.npz"))
    with open(os.path.join(G, "scheme_many.json")) as fh:
        m = json.load(fh)[str(secpar)]
    bs = BatchScheme(F.fusion_setup(secpar, m["setup_seed"]), threads=4)
    sk, vk = bs.keygen_batch(m["key_seeds"])
    assert np.array_equal(vk, S["vk"])
    data, codes = bs.sign_batch_encoded(sk, vk, m["messages"])
    assert not codes.any()
    return bs, vk, list(m["messages"]), data, S, m


MISMATCH = (False, "Target doesn't match image of aggregate signature.")


def forged(secpar, record):
    """a canonical record with one field moved by one inside the bound"""
    from test_verify_encoded_host import get_field
    rows, B, w, rb = TABLE["signature"][secpar]
    u = get_field(record, 11, w)
    return set_field(record, 11, u + 1 if u < 2 * B else u - 1, w)


@pytest.mark.parametrize("secpar", [128, 256])
def test_one_committee_all_honest_refused_forged(secpar):
    bs, vk, msgs, data, S, m = flow(secpar)
    rows, B, w, rb = TABLE["signature"][secpar]
    n = len(msgs)
    agg, codes, verdict = bs.aggregate_verify_encoded(vk, msgs, data)
    one, c1 = bs.aggregate_encoded(vk, msgs, data)
    assert np.array_equal(agg, S[f"agg_0_{n}"]) and np.array_equal(agg, one) and agg.dtype == np.int32
    assert codes.tolist() == c1.tolist() == [0] * n and codes.dtype == np.int32 and verdict == (True, "") == tuple(m["agg"][f"0_{n}"]["verdict"])
    # one record with a field at 2B + 1: code 6 there, the aggregate and a true verdict over the rest
    bad = data.copy()
    bad[3] = set_field(bad[3], 5, 2 * B + 1, w)
    agg, codes, verdict = bs.aggregate_verify_encoded(vk, msgs, bad)
    one, c1 = bs.aggregate_encoded(vk, msgs, bad)
    ok = codes == 0
    assert codes.tolist() == c1.tolist() == [6 if i == 3 else 0 for i in range(n)] and np.array_equal(agg, one)
    assert verdict == (True, "") == bs.verify(vk[ok], [x for x, k in zip(msgs, ok) if k], one)
    # one canonical record changed by one inside the bound: the aggregate is still aggregate_encoded's, and it does not verify
    bad = data.copy()
    bad[n // 2] = forged(secpar, bad[n // 2])
    agg, codes, verdict = bs.aggregate_verify_encoded(vk, msgs, bad.tobytes())
    one, _ = bs.aggregate_encoded(vk, msgs, bad)
    assert not codes.any() and np.array_equal(agg, one) and verdict == MISMATCH == bs.verify(vk, msgs, one)
    # every record refused
    bad = data.copy()
    for i in range(n):
        bad[i] = set_field(bad[i], i, 2 * B + 1, w)
    agg, codes, verdict = bs.aggregate_verify_encoded(vk, msgs, bad)
    assert agg is None and verdict is None and codes.tolist() == [6] * n


@pytest.mark.parametrize("secpar", [128, 256])
def test_many_committees_equal_the_single_call_per_group(secpar):
    from fusion_hip import DeviceArray
    bs, vk, msgs, data, S, m = flow(secpar)
    rows, B, w, rb = TABLE["signature"][secpar]
    # the reference's three committees, honest
    subsets = m["subsets"][1:]
    sizes = [hi - lo for lo, hi in subsets]
    aggs, codes, verdicts = bs.aggregate_verify_many_encoded(vk, msgs, data, sizes)
    assert not codes.any() and verdicts == [(True, "")] * 3
    for g, (lo, hi) in enumerate(subsets):
        assert np.array_equal(aggs[g], S[f"agg_{lo}_{hi}"]), (lo, hi)
    # five committees: the second all refused, the third forged, the last with one refused record
    sizes = [1, 5, 15, 2, 9] if secpar == 128 else [1, 3, 7, 2, 3]
    off = np.concatenate([[0], np.cumsum(sizes)])
    bad = data.copy()
    for i in range(off[1], off[2]):
        bad[i] = set_field(bad[i], i, 2 * B + 1, w)
    bad[off[2] + 1] = forged(secpar, bad[off[2] + 1])
    bad[off[4]] = set_field(bad[off[4]], 0, (1 << w) - 1, w)
    aggs, codes, verdicts = bs.aggregate_verify_many_encoded(vk, msgs, bad, sizes)
    for g, (a, b) in enumerate(zip(off, off[1:])):
        one, c1, v1 = bs.aggregate_verify_encoded(vk[a:b], msgs[a:b], bad[a:b])
        assert codes[a:b].tolist() == c1.tolist() and verdicts[g] == v1, g
        assert np.array_equal(aggs[g], one if one is not None else np.zeros_like(aggs[g])), g
    assert verdicts == [(True, ""), None, MISMATCH, (True, ""), (True, "")] and not aggs[1].any()
    plain, pcodes = bs.aggregate_many_encoded(vk, msgs, bad, sizes)
    assert np.array_equal(aggs, plain) and codes.tolist() == pcodes.tolist()
    # bytes in, bytes out; device-resident bytes and keys
    recs, c2, acodes, v2 = bs.aggregate_verify_many_encoded(vk, msgs, bad, sizes, encoded=True)
    want, wcodes = bs.encode("aggregate", aggs)
    _, _, pacodes = bs.aggregate_many_encoded(vk, msgs, bad, sizes, encoded=True)
    assert np.array_equal(recs, want) and acodes.tolist() == wcodes.tolist() == pacodes.tolist() and c2.tolist() == codes.tolist() and v2 == verdicts
    dB, dK = DeviceArray.from_numpy(bs.ctx, bad), DeviceArray.from_numpy(bs.ctx, vk)
    try:
        a3, c3, v3 = bs.aggregate_verify_many_encoded(dK, msgs, dB, sizes)
        assert np.array_equal(a3, aggs) and c3.tolist() == codes.tolist() and v3 == verdicts
        assert np.array_equal(dB.numpy(), bad) and np.array_equal(dK.numpy(), vk)
    finally:
        dB.free(), dK.free()


@pytest.mark.parametrize("secpar", [128, 256])
def test_object_face(secpar):
    import fusion.fusion as F
    from fusion_hip.scheme import vk_to_object
    bs, vk, msgs, data, S, m = flow(secpar)
    rows, B, w, rb = TABLE["signature"][secpar]
    params = bs.params
    keys = [vk_to_object(params, row) for row in vk]
    blobs = [data[i].tobytes() for i in range(len(msgs))]
    lo, hi = m["subsets"][1]
    sig, verdict = F.aggregate_verify_from_bytes(params, keys[lo:hi], msgs[lo:hi], blobs[lo:hi])
    assert str(sig) == str(F.aggregate_from_bytes(params, keys[lo:hi], msgs[lo:hi], blobs[lo:hi])) and verdict == (True, "")
    assert F.verify(params, keys[lo:hi], msgs[lo:hi], sig) == (True, "")
    groups = m["subsets"][1:]
    per = lambda x: [x[a:b] for a, b in groups]      # noqa: E731
    sigs, verdicts = F.aggregate_verify_many_from_bytes(params, per(keys), per(msgs), per(blobs))
    assert [str(s) for s in sigs] == [str(s) for s in F.aggregate_many_from_bytes(params, per(keys), per(msgs), per(blobs))]
    assert verdicts == [(True, "")] * 3 and str(sigs[0]) == str(sig)
    swapped = per(msgs)
    swapped[1] = swapped[1][::-1]
    assert F.aggregate_verify_many_from_bytes(params, per(keys), swapped, per(blobs))[1] == [(True, ""), MISMATCH, (True, "")]
    tampered = per(blobs)
    tampered[2][1] = set_field(np.frombuffer(tampered[2][1], dtype=np.uint8), 5, 2 * B + 1, w).tobytes()
    with pytest.raises(ValueError, match=r"group 2 record 1: Encoding is not canonical\."):
        F.aggregate_verify_many_from_bytes(params, per(keys), per(msgs), tampered)
    with pytest.raises(ValueError, match=r"record 1: Encoding is not canonical\."):
        F.aggregate_verify_from_bytes(params, per(keys)[2], per(msgs)[2], tampered[2])
