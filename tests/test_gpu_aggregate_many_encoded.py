"""Many committees aggregated straight from their compact bytes in one launch, on the device (fz_aggregate_encoded_ragged_async,
BatchScheme.aggregate_many_encoded / verify_many_encoded, fusion.fusion.aggregate_many_from_bytes / verify_many_from_bytes): bit for
bit the reference-made golden aggregates of three committees of different sizes, the numpy spec per group at every slice shape
and chunk geometry, the skip words at the groups' borders, the single-committee calls per group, graph capture and the entry's
refusals.  No tolerance anywhere."""
import json
import os

import numpy as np
import pytest

from test_encoding_host import TABLE, spec_pack
from test_gpu_aggregate_encoded import cent, special_alpha, spec_partial
from test_gpu_encoding import scheme, set_field

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
P_FILL, O_FILL, PAD = 0x5a5a5a5a5a5a5a5a, 0x5a5a5a5a, 24


def fields(n, l, d, B, seed):
    """centred integers z [n][l][d] of canonical records at bound B, the extremes 0 and 2B of the fields among them"""
    rng = np.random.default_rng(seed)
    u = rng.integers(0, 2 * B + 1, size=(n, l, d), dtype=np.int64)
    if n:
        u[0, 0, 0], u[-1, -1, -1], u[n // 2, 0, 1], u[n // 2, -1, -2] = 0, 2 * B, 2 * B, 0
    return u - B


def run_ragged(ctx, data, alpha, skip, sizes, l, B, d, want_out=True, stride=None):
    """fz_aggregate_encoded_ragged_async on host arrays, the partials partial_stride = l * d + 24 words apart with guard words
    between them, behind the last one and behind the last d_out row, all found untouched, as are the bytes
    -> (partials [G][l][d] int64, out [G][l][d] int32)"""
    from fusion_hip import DeviceArray
    g, per = len(sizes), l * d
    stride = per + PAD if stride is None else stride
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    raw = np.concatenate([np.asarray(data, dtype=np.uint8).ravel(), np.full(64, 0xab, dtype=np.uint8)])
    dB = DeviceArray.from_numpy(ctx, raw)
    dA = DeviceArray.from_numpy(ctx, np.ascontiguousarray(np.concatenate([alpha, np.zeros((1, d), dtype=np.int32)]), dtype=np.int32))
    dS = DeviceArray.from_numpy(ctx, np.ascontiguousarray(skip, dtype=np.int32)) if skip is not None else None
    dP = DeviceArray.from_numpy(ctx, np.full(g * stride + PAD, P_FILL, dtype=np.int64))
    dO = DeviceArray.from_numpy(ctx, np.full((g + 1, l, d), O_FILL, dtype=np.int32))
    try:
        ctx.aggregate_encoded_ragged_async_dev(dB.ptr, dA.ptr, dS.ptr if dS else 0, off, l, B, dP.ptr, stride, dO.ptr if want_out else 0)
        p, o, b = dP.numpy(), dO.numpy(), dB.numpy()
        assert np.array_equal(b, raw)
        assert (p[g * stride:] == P_FILL).all()
        body = p[:g * stride].reshape(g, stride)
        assert (body[:, per:] == P_FILL).all()
        assert (o[g] == O_FILL).all() and (want_out or (o == O_FILL).all())
        return body[:, :per].reshape(g, l, d).copy(), o[:g]
    finally:
        for x in (dB, dA, dS, dP, dO):
            if x is not None:
                x.free()


def want_partials(bs, z, alpha, sizes, skip=None):
    off = np.concatenate([[0], np.cumsum(sizes)])
    out = np.zeros((len(sizes),) + z.shape[1:], dtype=np.int64)
    for g, (a, b) in enumerate(zip(off, off[1:])):
        keep = np.arange(a, b) if skip is None else np.arange(a, b)[np.asarray(skip[a:b]) == 0]
        if keep.size:
            out[g] = spec_partial(bs, z[keep], alpha[keep])
    return out


# ---- the reference's aggregates ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("secpar", [128, 256])
def test_golden_aggregates_of_three_committees(secpar):
    import fusion.fusion as F
    from fusion_hip import ENCODING_REASONS
    from fusion_hip.scheme import BatchScheme
    S = np.load(os.path.join(G, f"scheme_many_{secpar}.npz"))
    with open(os.path.join(G, "scheme_many.json")) as fh:
        m = json.load(fh)[str(secpar)]
    bs = BatchScheme(F.fusion_setup(secpar, m["setup_seed"]), threads=4)      # (the setup of these goldens, not scheme()'s)
    subsets = m["subsets"][1:]                                       # the three consecutive ones: 5 / 12 / 15 or 3 / 6 / 7 signers
    sizes = [hi - lo for lo, hi in subsets]
    assert subsets[0][0] == 0 and all(a[1] == b[0] for a, b in zip(subsets, subsets[1:])) and sum(sizes) == len(m["messages"])
    msgs = m["messages"]
    sk, vk = bs.keygen_batch(m["key_seeds"])
    assert np.array_equal(vk, S["vk"])
    dD, codes = bs.sign_batch_encoded(sk, vk, msgs, device=True)
    try:
        assert not np.asarray(codes).any()
        out, codes = bs.aggregate_many_encoded(vk, msgs, dD, sizes)
        assert out.dtype == np.int32 and codes.dtype == np.int32 and codes.tolist() == [0] * sum(sizes)
        for g, (lo, hi) in enumerate(subsets):
            assert np.array_equal(out[g], S[f"agg_{lo}_{hi}"]), (secpar, lo, hi)
        recs, codes, acodes = bs.aggregate_many_encoded(vk, msgs, dD, sizes, encoded=True)
    finally:
        dD.free()
    rows, B, w, rb = TABLE["aggregate"][secpar]
    assert recs.shape == (3, rb) and recs.dtype == np.uint8 and acodes.tolist() == [0, 0, 0] and not codes.any()
    assert bs.verify_many_encoded(vk, msgs, recs, sizes) == [(True, "")] * 3
    for g, (lo, hi) in enumerate(subsets):
        info = m["agg"][f"{lo}_{hi}"]
        # a tamper that keeps every field in range: decode, +1 on one coefficient, encode
        back, _ = bs.decode("aggregate", recs[g])
        z = bs.ctx.ntt_inverse(back.reshape(-1, bs.d)).reshape(rows, bs.d)
        r, c = info["tampered_at"][0] % rows, info["tampered_at"][1]
        z[r, c] += 1 if z[r, c] < B else -1
        bad, bcodes = bs.encode("aggregate", bs.ctx.ntt_forward(z)[None])
        assert bcodes.tolist() == [0]
        t = recs.copy()
        t[g] = bad[0]
        want = [(True, "")] * 3
        want[g] = tuple(info["tampered_verdict"])
        assert bs.verify_many_encoded(vk, msgs, t, sizes) == want
        t = recs.copy()
        t[g] = set_field(t[g], 7 + g, 2 * B + 1, w)
        want[g] = (False, ENCODING_REASONS[6])
        assert bs.verify_many_encoded(vk, msgs, t.tobytes(), sizes) == want


# ---- the C entry against the CPU spec ----------------------------------------------------------------------------------------
SHAPES = {"fewer-than-waves": [1, 2, 3, 5], "uneven-slices": [67, 1, 33], "zero-signer-group": [4, 0, 4],
          "two-launches": [1 + (3 * g) % 5 for g in range(70)]}


@pytest.mark.parametrize("secpar,l", [(128, 18), (256, 5)])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_entry_equals_the_spec_per_group(secpar, l, shape):
    """a chunk and a tail per record at either degree; slices that are empty, uneven, of a group without signers, and 70 groups
    (two launches, looked at on both sides of the seam)"""
    _, bs = scheme(secpar)
    sizes, d = SHAPES[shape], bs.d
    B = TABLE["signature"][secpar][1]
    n = sum(sizes)
    z = fields(n, l, d, B, 11 * n + secpar)
    data = spec_pack(z, B, (2 * B).bit_length())
    alpha = special_alpha(bs, n, n + secpar)
    off = np.concatenate([[0], np.cumsum(sizes)])
    for g in range(1, len(sizes)):                                   # the int32 extremes at the head of every group, not of the first alone
        if sizes[g]:
            alpha[off[g]:off[g + 1]] = special_alpha(bs, sizes[g], g + secpar)
    p, o = run_ragged(bs.ctx, data, alpha, None, sizes, l, B, d)
    look = range(len(sizes)) if len(sizes) <= 4 else (0, 63, 64, 69)
    want = want_partials(bs, z, alpha, sizes)
    for g in look:
        assert np.array_equal(p[g], want[g]), (shape, g)
        assert np.array_equal(o[g], cent(want[g], bs.q)), (shape, g)
        assert np.abs(p[g]).max() <= sizes[g] * (bs.q - 1) // 2
    assert np.array_equal(p, want) and np.array_equal(o, cent(want, bs.q))
    if shape == "zero-signer-group":
        assert not p[1].any() and not o[1].any()
    p2, _ = run_ragged(bs.ctx, data, alpha, np.zeros(n, dtype=np.int32), sizes, l, B, d, want_out=False)      # a mask that skips nobody
    assert np.array_equal(p2, p)


@pytest.mark.parametrize("secpar,l", [(256, 1), (256, 4), (256, 5), (256, 83), (128, 2), (128, 16), (128, 18), (128, 195)])
def test_chunk_geometry_per_group(secpar, l):
    """degree 256: a 256-value tail only, exactly one chunk, a chunk and a tail, the real record; degree 64 likewise; field widths 2
    and the kind's 13 / 14"""
    _, bs = scheme(secpar)
    d, sizes = bs.d, [3, 2]
    for B in (1, TABLE["signature"][secpar][1]):
        w = (2 * B).bit_length()
        assert (l * d * w // 8) % 16 == 0
        z = fields(5, l, d, B, l + w + secpar)
        alpha = special_alpha(bs, 5, l + w)
        want = want_partials(bs, z, alpha, sizes)
        p, o = run_ragged(bs.ctx, spec_pack(z, B, w), alpha, None, sizes, l, B, d)
        assert np.array_equal(p, want), (secpar, l, B)
        assert np.array_equal(o, cent(want, bs.q)), (secpar, l, B)


# ---- skip words ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("secpar", [128, 256])
def test_skip_words_stop_at_the_groups_borders(secpar):
    """64 groups of the real record (more workgroups than the chip holds: one slice per group, so a wave walks several signers and
    looks ahead on the skip words); group 0's last and group 1's first record skipped, group 2 skipped whole; the next group's
    first word set and cleared: the group in front of it does not change"""
    _, bs = scheme(secpar)
    rows, B, w, rb = TABLE["signature"][secpar]
    sizes = [13, 9, 6] + [1 + g % 2 for g in range(61)]
    n, d = sum(sizes), bs.d
    off = np.concatenate([[0], np.cumsum(sizes)])
    z = fields(n, rows, d, B, 5 * secpar)
    data = spec_pack(z, B, w)
    alpha = special_alpha(bs, n, secpar)
    skip = np.zeros(n, dtype=np.int32)
    skip[off[1] - 1], skip[off[1]], skip[off[2]:off[3]], skip[off[5]] = 6, 3, 6, 4
    skip[4], skip[8] = 6, 6                                          # a wave of group 0 whose signer after next is skipped
    data[skip != 0] = 0xff                                           # bytes that would change the sum if read
    want = want_partials(bs, z, alpha, sizes, skip)
    p, o = run_ragged(bs.ctx, data, alpha, skip, sizes, rows, B, d)
    assert np.array_equal(p, want) and np.array_equal(o, cent(want, bs.q))
    assert not p[2].any() and not o[2].any() and not p[5].any()
    for g in (0, 1, 3):                                              # the first word of the group behind g, either way round
        s2 = skip.copy()
        s2[off[g + 1]] = 0 if skip[off[g + 1]] else 6
        p2, _ = run_ragged(bs.ctx, data, alpha, s2, sizes, rows, B, d, want_out=False)
        assert np.array_equal(p2[g], want[g]), g
        assert np.array_equal(p2[:g + 1], want[:g + 1]) and np.array_equal(p2[g + 2:], want[g + 2:])


# ---- the single-committee calls per group --------------------------------------------------------------------------------------
def signed_groups(bs, sizes, tag):
    n = sum(sizes)
    seeds = [1300 + 17 * k for k in range(n)]
    msgs = [f"{tag}-{bs.params.secpar}-{k}" for k in range(n)]
    sk, vk = bs.keygen_batch(seeds)
    return vk, msgs, bs.sign_batch(sk, vk, msgs)


@pytest.mark.parametrize("secpar", [128, 256])
def test_equals_the_single_committee_calls_per_group(secpar):
    from fusion_hip import DeviceArray
    _, bs = scheme(secpar)
    rows, B, w, rb = TABLE["signature"][secpar]
    sizes = [7, 1, 8]
    off = np.concatenate([[0], np.cumsum(sizes)])
    vk, msgs, sig = signed_groups(bs, sizes, "many")
    data, codes = bs.encode("signature", sig)
    assert not codes.any()
    for g in (0, 2):                                                 # records 2 and 5 of the groups that have them, as `spoil` does
        data[off[g] + 2] = set_field(data[off[g] + 2], 0, 2 * B + 1, w)
        data[off[g] + 5] = set_field(data[off[g] + 5], rb * 8 // w - 1, (1 << w) - 1, w)
    data[off[1]] = set_field(data[off[1]], 3, 2 * B + 1, w)          # the one-signer group has no accepted signer
    msgs = list(msgs)
    msgs[off[2] + 1] += " (another message)"                         # a signer whose signature is for something else
    groups = [(vk[a:b], msgs[a:b], data[a:b]) for a, b in zip(off, off[1:])]
    out, codes = bs.aggregate_many_encoded(vk, msgs, data, sizes)
    for g, (k, m, x) in enumerate(groups):
        one, c = bs.aggregate_encoded(k, m, x)
        assert codes[off[g]:off[g + 1]].tolist() == c.tolist()
        assert np.array_equal(out[g], one if one is not None else np.zeros_like(out[g])), g
    assert codes.tolist() == [0, 0, 6, 0, 0, 6, 0, 6, 0, 0, 6, 0, 0, 6, 0, 0] and not out[1].any()
    outs, scodes = bs.aggregate_many_encoded(vk, msgs, data, sizes, screened=True)
    for g, (k, m, x) in enumerate(groups):
        one, c = bs.aggregate_encoded_screened(k, m, x)
        assert scodes[off[g]:off[g + 1]].tolist() == c.tolist()
        assert np.array_equal(outs[g], one if one is not None else np.zeros_like(outs[g])), g
    assert scodes.tolist() == [0, 0, 6, 0, 0, 6, 0, 6, 0, 3, 6, 0, 0, 6, 0, 0]
    recs, c2, acodes = bs.aggregate_many_encoded(vk, msgs, data, sizes, screened=True, encoded=True)
    want, wcodes = bs.encode("aggregate", outs)
    assert np.array_equal(recs, want) and acodes.tolist() == wcodes.tolist() == [0, 0, 0] and c2.tolist() == scodes.tolist()
    verdicts = bs.verify_many_encoded(vk, msgs, recs, sizes)
    assert verdicts == [bs.verify_encoded(k, m, recs[g]) for g, (k, m, _) in enumerate(groups)]
    assert verdicts[0] == (False, "Target doesn't match image of aggregate signature.")      # (verified against ALL the group's keys)
    ok = scodes == 0
    sz = [int(ok[a:b].sum()) for a, b in zip(off, off[1:])]
    keep = [g for g in range(3) if sz[g]]
    vk_ok, msgs_ok = vk[ok], [m for m, k in zip(msgs, ok) if k]
    assert bs.verify_many_encoded(vk_ok, msgs_ok, recs[keep], [sz[g] for g in keep]) == [(True, "")] * len(keep)
    # device-resident bytes and keys
    dB, dK, dR = DeviceArray.from_numpy(bs.ctx, data), DeviceArray.from_numpy(bs.ctx, vk), DeviceArray.from_numpy(bs.ctx, recs)
    try:
        for screened in (False, True):
            o2, c2 = bs.aggregate_many_encoded(dK, msgs, dB, sizes, screened=screened)
            assert np.array_equal(o2, outs if screened else out) and c2.tolist() == (scodes if screened else codes).tolist()
        assert bs.verify_many_encoded(dK, msgs, dR, sizes) == verdicts
        assert np.array_equal(dB.numpy(), data) and np.array_equal(dK.numpy(), vk) and np.array_equal(dR.numpy(), recs)
    finally:
        for b in (dB, dK, dR):
            b.free()


@pytest.mark.parametrize("secpar", [128, 256])
def test_object_face(secpar):
    import fusion.fusion as F
    params, _ = scheme(secpar)
    rows, B, w, rb = TABLE["signature"][secpar]
    keys = [F.keygen(params, 800 + k) for k in range(3)]
    vks = [[keys[0][1]], [keys[1][1], keys[2][1]]]
    msgs = [[f"many-from-bytes-{secpar}-0"], [f"many-from-bytes-{secpar}-{k}" for k in (1, 2)]]
    blobs = [[F.to_bytes(params, F.sign(params, keys[0], msgs[0][0]))],
             [F.to_bytes(params, F.sign(params, keys[k], msgs[1][k - 1])) for k in (1, 2)]]
    aggs = F.aggregate_many_from_bytes(params, vks, msgs, blobs)
    assert [str(a) for a in aggs] == [str(F.aggregate_from_bytes(params, vks[g], msgs[g], blobs[g])) for g in range(2)]
    ablobs = [F.to_bytes(params, a, aggregate=True) for a in aggs]
    assert F.verify_many_from_bytes(params, vks, msgs, ablobs) == [(True, "")] * 2
    assert F.verify_many_from_bytes(params, vks, msgs, ablobs[::-1]) == \
        [F.verify_from_bytes(params, vks[g], msgs[g], ablobs[1 - g]) for g in range(2)]
    bad = [blobs[0], [blobs[1][0], set_field(np.frombuffer(blobs[1][1], dtype=np.uint8), 5, 2 * B + 1, w).tobytes()]]
    with pytest.raises(ValueError, match=r"group 1 record 1: Encoding is not canonical\."):
        F.aggregate_many_from_bytes(params, vks, msgs, bad)


# ---- graph capture -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("secpar,l", [(128, 18), (256, 5)])
def test_graph_capture_replays_the_entry(secpar, l):
    from fusion_hip import DeviceArray
    from fusion_hip.scheme import BatchScheme
    params, shared = scheme(secpar)
    B, d, sizes = TABLE["signature"][secpar][1], shared.d, [5, 0, 9]
    n, per = sum(sizes), l * shared.d
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    z = fields(n, l, d, B, 3 + secpar)
    alpha = special_alpha(shared, n, 3 * secpar)
    skip = np.zeros(n, dtype=np.int32)
    skip[6] = 6
    want = want_partials(shared, z, alpha, sizes, skip)
    bs = BatchScheme(params, private_context=True)
    try:
        ctx = bs.ctx
        dB, dA, dS = (DeviceArray.from_numpy(ctx, a) for a in (spec_pack(z, B, (2 * B).bit_length()), alpha, skip))
        dP, dO = DeviceArray(ctx, (3, per + PAD), np.int64), DeviceArray(ctx, (3, l, d))
        ctx.graph_begin()
        ctx.aggregate_encoded_ragged_async_dev(dB.ptr, dA.ptr, dS.ptr, off, l, B, dP.ptr, per + PAD, dO.ptr)
        g = ctx.graph_end()
        ctx.h2d(dP.ptr, np.full((3, per + PAD), P_FILL, dtype=np.int64))
        ctx.h2d(dO.ptr, np.full((3, l, d), O_FILL, dtype=np.int32))
        g.launch()
        ctx.synchronize()
        p = dP.numpy()
        assert np.array_equal(p[:, :per].reshape(3, l, d), want) and (p[:, per:] == P_FILL).all()
        assert np.array_equal(dO.numpy(), cent(want, bs.q))
        g.destroy()
        for b in (dB, dA, dS, dP, dO):
            b.free()
    finally:
        bs.close()


# ---- the entry's refusals ------------------------------------------------------------------------------------------------------
def test_entry_refusals():
    from fusion_hip import Context, DeviceArray, FusionHipError
    from fusion_hip._lib import FZ_E_BADARG, FZ_E_UNSUPPORTED
    _, bs = scheme(128)
    ctx, d = bs.ctx, bs.d
    dB = DeviceArray.from_numpy(ctx, np.zeros(4096, dtype=np.uint8))
    dA = DeviceArray.from_numpy(ctx, np.zeros((4, d), dtype=np.int32))
    dP = DeviceArray.from_numpy(ctx, np.full((2, 2 * d + PAD), P_FILL, dtype=np.int64))
    dO = DeviceArray.from_numpy(ctx, np.full((2, 2, d), O_FILL, dtype=np.int32))
    call = ctx.aggregate_encoded_ragged_async_dev
    try:
        bad = [(dB.ptr, dA.ptr, [0, 2, 1], 2, 5, dP.ptr, 2 * d + PAD, dO.ptr),           # decreasing offsets
               (dB.ptr, dA.ptr, [0, 1, 2], 2, 5, dP.ptr, 2 * d - 2, dO.ptr),             # a short stride
               (dB.ptr + 4, dA.ptr, [0, 1, 2], 2, 5, dP.ptr, 2 * d + PAD, dO.ptr),       # misaligned pointers
               (dB.ptr, dA.ptr + 4, [0, 1, 2], 2, 5, dP.ptr, 2 * d + PAD, dO.ptr),
               (dB.ptr, dA.ptr, [0, 1, 2], 2, 5, dP.ptr + 8, 2 * d + PAD, dO.ptr),
               (dB.ptr, dA.ptr, [0, 1, 2], 2, 5, dP.ptr, 2 * d + PAD, dO.ptr + 4),
               (dB.ptr, dA.ptr, [0, 1, 2], 2, 0, dP.ptr, 2 * d + PAD, dO.ptr),           # the rules of fz_aggregate_encoded_async
               (dB.ptr, dA.ptr, [0, 1, 2], 0, 5, dP.ptr, 2 * d + PAD, dO.ptr)]
        for args in bad:
            with pytest.raises(FusionHipError) as e:
                call(args[0], args[1], 0, *args[2:])
            assert e.value.code == FZ_E_BADARG, args[2:5]
        with pytest.raises(FusionHipError) as e:                   # degree 64, l = 1, bound = 2: l * w odd, 24-byte records
            call(dB.ptr, dA.ptr, 0, [0, 1, 2], 1, 2, dP.ptr, d + PAD, dO.ptr)
        assert e.value.code == FZ_E_UNSUPPORTED
        ring = Context(bs.q, d, 0, 0)                               # a ring-only context: no transforms, logd < 0
        try:
            with pytest.raises(FusionHipError) as e:
                ring.aggregate_encoded_ragged_async_dev(dB.ptr, dA.ptr, 0, [0, 1, 2], 2, 5, dP.ptr, 2 * d + PAD, dO.ptr)
            assert e.value.code == FZ_E_UNSUPPORTED
        finally:
            ring.close()
        call(dB.ptr, dA.ptr, 0, [0], 2, 5, dP.ptr, 2 * d + PAD, dO.ptr)                   # groups == 0: OK, nothing written
        ctx.synchronize()
        assert (dP.numpy() == P_FILL).all() and (dO.numpy() == O_FILL).all()
    finally:
        for x in (dB, dA, dP, dO):
            x.free()
