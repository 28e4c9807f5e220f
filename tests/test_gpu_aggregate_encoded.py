"""Aggregation straight from the compact byte encoding on the device (fz_check_records_async, fz_aggregate_encoded_async,
BatchScheme.aggregate_encoded, fusion.fusion.aggregate_from_bytes): bit for bit the reference-made golden aggregates, the existing
decode -> aggregate path at every walk shape, the numpy spec at every chunk geometry, the skip mask, graph capture, the object face
and device-resident input.  No tolerance anywhere."""
import json
import os

import numpy as np
import pytest

from test_encoding_host import TABLE, spec_pack
from test_gpu_encoding import honest_rows, scheme, set_field

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
_ORACLE = []


def oracle():
    from oracle import oracle as O
    if not _ORACLE:
        _ORACLE.append(O.COracle())
    return O, _ORACLE[0]


def cent(x, q):
    return (np.asarray(x, dtype=np.int64) + q // 2) % q - q // 2


def spec_partial(bs, z, alpha):
    """the int64 sums the fused entry leaves: sum_i cent(NTT(z_i) (.) alpha_i), z [N][l][d] centred integers, alpha [N][d] any int32
    (|NTT(z)| < 2^30 and |alpha| <= 2^31: the products fit int64)"""
    O, orc = oracle()
    P = O.PARAMS[bs.params.secpar]
    n, l, d = z.shape
    f = orc.ntt_forward(np.ascontiguousarray(z, dtype=np.int32).reshape(-1, d), bs.q, P["root"]).reshape(n, l, d).astype(np.int64)
    return cent(f * np.asarray(alpha, dtype=np.int64)[:, None, :], bs.q).sum(axis=0)


def special_alpha(bs, n, seed):
    """random centred rows; among the first rows +(q-1)/2, -(q-1)/2, zero, INT32_MIN and INT32_MAX (raw int32 is accepted), which
    of them depending on n when there are fewer than five signers"""
    rng = np.random.default_rng(seed)
    h = (bs.q - 1) // 2
    alpha = rng.integers(-h, h + 1, size=(n, bs.d), dtype=np.int64)
    for i in range(min(n, 5)):
        alpha[i] = [h, -h, 0, I32_MIN, I32_MAX][(i + n) % 5]
    return alpha.astype(np.int32)


def run_entry(ctx, data, alpha, skip, n, l, bound, d, guard=0, want_out=True):
    """fz_aggregate_encoded_async on host arrays -> (partial [l][d] int64, out [l][d] int32 or None, and what lies behind each)"""
    from fusion_hip import DeviceArray
    raw = np.concatenate([np.asarray(data, dtype=np.uint8).ravel(), np.full(guard, 0xab, dtype=np.uint8)])
    dB = DeviceArray.from_numpy(ctx, raw)
    dA = DeviceArray.from_numpy(ctx, np.ascontiguousarray(alpha, dtype=np.int32))
    dS = DeviceArray.from_numpy(ctx, np.ascontiguousarray(skip, dtype=np.int32)) if skip is not None else None
    dP = DeviceArray.from_numpy(ctx, np.full((2, l, d), 0x5a5a5a5a5a5a5a5a, dtype=np.int64))
    dO = DeviceArray.from_numpy(ctx, np.full((2, l, d), 0x5a5a5a5a, dtype=np.int32))
    try:
        ctx.aggregate_encoded_async_dev(dB.ptr, dA.ptr, dS.ptr if dS else 0, n, l, bound, dP.ptr, dO.ptr if want_out else 0)
        p, o, b = dP.numpy(), dO.numpy(), dB.numpy()
        assert (b[raw.size - guard:] == 0xab).all() and np.array_equal(b, raw)
        return p, o
    finally:
        for x in (dB, dA, dS, dP, dO):
            if x is not None:
                x.free()


# ---- golden ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("secpar", [128, 256])
def test_golden_aggregates(secpar):
    _, bs = scheme(secpar)
    S = np.load(os.path.join(G, f"scheme_{secpar}.npz"))
    with open(os.path.join(G, "scheme.json")) as fh:
        J = json.load(fh)[str(secpar)]
    rows, B, w, rb = TABLE["signature"][secpar]
    for k in (1, 2, 4):
        order = J["agg"][str(k)]["order"]
        data, codes = bs.encode("signature", S["sig"][order])
        assert codes.tolist() == [0] * k
        p, o = run_entry(bs.ctx, data, S[f"alpha_hat_{k}"], None, k, rows, B, bs.d)
        assert np.array_equal(o[0], S[f"agg_{k}"]), (secpar, k)
        assert np.array_equal(cent(p[0], bs.q), S[f"agg_{k}"]) and np.abs(p[0]).max() <= k * (bs.q - 1) // 2
        assert (p[1] == 0x5a5a5a5a5a5a5a5a).all() and (o[1] == 0x5a5a5a5a).all()
    data, _ = bs.encode("signature", S["sig"])
    out, codes = bs.aggregate_encoded(S["vk"], J["messages"], data.tobytes())
    assert codes.dtype == np.int32 and codes.tolist() == [0] * 4
    assert out.dtype == np.int32 and np.array_equal(out, S["agg_4"])


# ---- the existing path at every walk shape -----------------------------------------------------------------------------------
@pytest.mark.parametrize("secpar", [128, 256])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 33, 67, 1024])
def test_equals_decode_then_aggregate_core(secpar, n):
    """fewer signers than waves (1, 2, 3), an uneven round-robin (5), uneven slices (33, 67), more wave-tasks than the resident
    grid (1024)"""
    _, bs = scheme(secpar)
    rows, B, w, rb = TABLE["signature"][secpar]
    x, z = honest_rows(bs, "signature", n, 7000 + n + secpar)
    data, codes = bs.encode("signature", x)
    assert not codes.any()
    alpha = special_alpha(bs, n, n + secpar)
    back, codes = bs.decode("signature", data)
    assert not codes.any()
    want = bs.ctx.aggregate_core(back, alpha)
    p, o = run_entry(bs.ctx, data, alpha, None, n, rows, B, bs.d)
    assert np.array_equal(o[0], want)
    assert np.array_equal(cent(p[0], bs.q), want) and np.abs(p[0]).max() <= n * (bs.q - 1) // 2
    assert (p[1] == 0x5a5a5a5a5a5a5a5a).all() and (o[1] == 0x5a5a5a5a).all()
    if n <= 5:
        _, orc = oracle()
        assert np.array_equal(o[0], orc.aggregate_core(x, alpha, bs.q))
        assert np.array_equal(p[0], spec_partial(bs, z, alpha))
    p2, _ = run_entry(bs.ctx, data, alpha, np.zeros(n, dtype=np.int32), n, rows, B, bs.d, want_out=False)      # a mask that skips nobody
    assert np.array_equal(p2, p)


# ---- chunk geometry: free l and bound through the C entry --------------------------------------------------------------------
@pytest.mark.parametrize("secpar,l", [(256, 1), (256, 4), (256, 5), (256, 83), (128, 2), (128, 16), (128, 18), (128, 195)])
def test_chunk_geometry(secpar, l):
    """degree 256: a 256-value tail only, exactly one chunk, a chunk and a tail, the real record; degree 64 likewise; field widths
    2, the kind's 13 / 14, and 31"""
    _, bs = scheme(secpar)
    d, n = bs.d, 3
    for B in (1, TABLE["signature"][secpar][1], (bs.q - 1) // 2):
        w = (2 * B).bit_length()
        if (l * d * w // 8) % 16:                                  # degree 64 with l * w odd (195 x 31): the entry refuses such records
            assert d == 64 and l * w % 2 == 1
            continue
        rng = np.random.default_rng(l + w + secpar)
        u = rng.integers(0, 2 * B + 1, size=(n, l, d), dtype=np.int64)
        u[0, 0, 0], u[1, -1, -1], u[2, 0, 1], u[2, -1, -2] = 0, 2 * B, 2 * B, 0
        z = u - B
        data = spec_pack(z, B, w)
        assert data.shape == (n, l * d * w // 8)
        alpha = special_alpha(bs, n, l + w)
        want = spec_partial(bs, z, alpha)
        p, o = run_entry(bs.ctx, data, alpha, None, n, l, B, d, guard=64)
        assert np.array_equal(p[0], want), (secpar, l, B)
        assert np.array_equal(o[0], cent(want, bs.q)), (secpar, l, B)
        assert (p[1] == 0x5a5a5a5a5a5a5a5a).all() and (o[1] == 0x5a5a5a5a).all()


def test_entry_refusals():
    from fusion_hip import DeviceArray, FusionHipError
    from fusion_hip._lib import FZ_E_BADARG, FZ_E_UNSUPPORTED
    _, bs = scheme(128)
    ctx, d = bs.ctx, bs.d
    dB = DeviceArray.from_numpy(ctx, np.zeros(4096, dtype=np.uint8))
    dA = DeviceArray.from_numpy(ctx, np.zeros((2, d), dtype=np.int32))
    dV = DeviceArray.from_numpy(ctx, np.full(8, 0x7f7f7f7f, dtype=np.int32))
    dP = DeviceArray.from_numpy(ctx, np.full((2, d), 0x5a5a5a5a5a5a5a5a, dtype=np.int64))
    dO = DeviceArray.from_numpy(ctx, np.full((2, d), 0x5a5a5a5a, dtype=np.int32))
    try:
        with pytest.raises(FusionHipError) as e:                   # degree 64, l = 1, bound = 2: 24-byte records
            ctx.aggregate_encoded_async_dev(dB.ptr, dA.ptr, 0, 2, 1, 2, dP.ptr, dO.ptr)
        assert e.value.code == FZ_E_UNSUPPORTED
        bad = [(dB.ptr, dA.ptr, 2, 2, 0), (dB.ptr, dA.ptr, 2, 2, (bs.q - 1) // 2 + 1), (dB.ptr, dA.ptr, 2, 0, 5),
               (dB.ptr + 4, dA.ptr, 2, 2, 5), (dB.ptr, dA.ptr + 4, 2, 2, 5)]
        for b, a, n, l, bound in bad:
            with pytest.raises(FusionHipError) as e:
                ctx.aggregate_encoded_async_dev(b, a, 0, n, l, bound, dP.ptr, dO.ptr)
            assert e.value.code == FZ_E_BADARG, (n, l, bound)
        for ptrs in ((dP.ptr + 8, dO.ptr), (dP.ptr, dO.ptr + 4)):
            with pytest.raises(FusionHipError) as e:
                ctx.aggregate_encoded_async_dev(dB.ptr, dA.ptr, 0, 2, 2, 5, *ptrs)
            assert e.value.code == FZ_E_BADARG
        for n, rows, bound, b, v in ((2, 2, 0, dB.ptr, dV.ptr), (2, 0, 5, dB.ptr, dV.ptr), (2, 2, 5, dB.ptr + 4, dV.ptr),
                                     (2, 2, 5, dB.ptr, dV.ptr + 4)):
            with pytest.raises(FusionHipError) as e:
                ctx.check_records_async_dev(b, n, rows, bound, v)
            assert e.value.code == FZ_E_BADARG
        ctx.aggregate_encoded_async_dev(dB.ptr, dA.ptr, 0, 0, 2, 5, dP.ptr, dO.ptr)       # N = 0: OK, nothing written
        ctx.check_records_async_dev(dB.ptr, 0, 2, 5, dV.ptr)
        ctx.synchronize()
        assert (dP.numpy() == 0x5a5a5a5a5a5a5a5a).all() and (dO.numpy() == 0x5a5a5a5a).all() and (dV.numpy() == 0x7f7f7f7f).all()
    finally:
        for x in (dB, dA, dV, dP, dO):
            x.free()


# ---- skip mask and canonicity ----------------------------------------------------------------------------------------------
def signed_batch(bs, n, tag):
    seeds = [900 + 13 * k for k in range(n)]
    msgs = [f"{tag}-{bs.params.secpar}-{k}" for k in range(n)]
    sk, vk = bs.keygen_batch(seeds)
    return vk, msgs, bs.sign_batch(sk, vk, msgs)


def spoil(data, secpar, kind="signature"):
    """records 2 and 5 made non-canonical: field 0 = 2B + 1, the last field = 2^w - 1"""
    rows, B, w, rb = TABLE[kind][secpar]
    d2 = data.copy()
    d2[2] = set_field(d2[2], 0, 2 * B + 1, w)
    d2[5] = set_field(d2[5], rb * 8 // w - 1, (1 << w) - 1, w)
    return d2


@pytest.mark.parametrize("secpar", [128, 256])
def test_check_gives_decodes_codes(secpar):
    from fusion_hip import DeviceArray
    _, bs = scheme(secpar)
    for kind, n in (("signature", 7), ("vk", 5), ("aggregate", 5)):
        rows, B, w, rb = TABLE[kind][secpar]
        x, _ = honest_rows(bs, kind, n, 40 + secpar + n)
        data, _ = bs.encode(kind, x)
        if n == 7:
            data = spoil(data, secpar)
        else:
            data[1] = set_field(data[1], rows * bs.d // 2, 2 * B + 1, w)
            data[n - 1] = set_field(data[n - 1], rows * bs.d - 1, (1 << w) - 1, w)
        _, want = bs.decode(kind, data)
        dB = DeviceArray.from_numpy(bs.ctx, data)
        dV = DeviceArray.from_numpy(bs.ctx, np.full(n + 16, 0x7f7f7f7f, dtype=np.int32))
        try:
            bs.ctx.check_records_async_dev(dB.ptr, n, rows, B, dV.ptr)
            st = dV.numpy()
            assert st[:n].tolist() == want.tolist() and (st[n:] == 0x7f7f7f7f).all() and np.array_equal(dB.numpy(), data)
            assert want.tolist() == ([0, 0, 6, 0, 0, 6, 0] if n == 7 else [0, 6, 0, 0, 6])
        finally:
            dB.free()
            dV.free()


@pytest.mark.parametrize("secpar", [128, 256])
def test_refused_records_are_skipped(secpar):
    _, bs = scheme(secpar)
    rows, B, w, rb = TABLE["signature"][secpar]
    n = 7
    vk, msgs, sig = signed_batch(bs, n, "skip")
    good, codes = bs.encode("signature", sig)
    assert not codes.any()
    data = spoil(good, secpar)
    out, codes = bs.aggregate_encoded(vk, msgs, data)
    assert codes.tolist() == [0, 0, 6, 0, 0, 6, 0]
    ok = codes == 0
    back, dcodes = bs.decode("signature", data)
    assert dcodes.tolist() == codes.tolist()
    assert np.array_equal(out, bs.aggregate(vk[ok], [m for m, k in zip(msgs, ok) if k], back[ok]))
    # the result is a function of the accepted records and their alpha_hat alone, whatever bytes a refused record holds
    alpha = special_alpha(bs, n, secpar)
    z = bs.ctx.ntt_inverse(sig.reshape(-1, bs.d)).reshape(sig.shape).astype(np.int64)
    want = spec_partial(bs, z[ok], alpha[ok])
    for fill in (None, 0xff, 0x00):
        d2 = data.copy()
        if fill is not None:
            d2[~ok] = fill
        p, o = run_entry(bs.ctx, d2, alpha, codes, n, rows, B, bs.d)
        assert np.array_equal(p[0], want) and np.array_equal(o[0], cent(want, bs.q)), fill
    # every record refused
    out, codes = bs.aggregate_encoded(vk, msgs, np.full((n, rb), 0xff, dtype=np.uint8))
    assert out is None and codes.tolist() == [6] * n
    p, o = run_entry(bs.ctx, data, alpha, np.full(n, 6, dtype=np.int32), n, rows, B, bs.d)
    assert not p[0].any() and not o[0].any()


# ---- stale outputs and graph capture ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("secpar", [128, 256])
def test_graph_capture_replays_check_and_aggregation(secpar):
    from fusion_hip import DeviceArray
    from fusion_hip.scheme import BatchScheme
    params, shared = scheme(secpar)
    rows, B, w, rb = TABLE["signature"][secpar]
    n = 7
    x, _ = honest_rows(shared, "signature", n, 5 + secpar)
    data, _ = shared.encode("signature", x)
    data[3] = set_field(data[3], 17, 2 * B + 1, w)
    alpha = special_alpha(shared, n, 3 * secpar)
    bs = BatchScheme(params, private_context=True)
    try:
        ctx = bs.ctx
        dB, dA = DeviceArray.from_numpy(ctx, data), DeviceArray.from_numpy(ctx, alpha)
        dV, dP, dO = DeviceArray(ctx, (n,)), DeviceArray(ctx, (rows, bs.d), np.int64), DeviceArray(ctx, (rows, bs.d))
        ctx.check_records_async_dev(dB.ptr, n, rows, B, dV.ptr)
        ctx.aggregate_encoded_async_dev(dB.ptr, dA.ptr, dV.ptr, n, rows, B, dP.ptr, dO.ptr)
        want_v, want_p, want_o = dV.numpy(), dP.numpy(), dO.numpy()
        assert want_v.tolist() == [6 if k == 3 else 0 for k in range(n)]
        back, _ = shared.decode("signature", data)                 # (the refused record's rows are zero)
        assert np.array_equal(want_o, shared.ctx.aggregate_core(back, alpha))
        ctx.graph_begin()
        ctx.check_records_async_dev(dB.ptr, n, rows, B, dV.ptr)
        ctx.aggregate_encoded_async_dev(dB.ptr, dA.ptr, dV.ptr, n, rows, B, dP.ptr, dO.ptr)
        g = ctx.graph_end()
        for _ in range(2):
            ctx.h2d(dV.ptr, np.full(n, 0x7f7f7f7f, dtype=np.int32))
            ctx.h2d(dP.ptr, np.full((rows, bs.d), 0x5a5a5a5a5a5a5a5a, dtype=np.int64))
            ctx.h2d(dO.ptr, np.full((rows, bs.d), 0x5a5a5a5a, dtype=np.int32))
            g.launch()
            ctx.synchronize()
            assert np.array_equal(dV.numpy(), want_v) and np.array_equal(dP.numpy(), want_p) and np.array_equal(dO.numpy(), want_o)
        g.destroy()
        for b in (dB, dA, dV, dP, dO):
            b.free()
    finally:
        bs.close()


# ---- object face and device-resident input ---------------------------------------------------------------------------------
@pytest.mark.parametrize("secpar", [128, 256])
def test_object_face(secpar):
    import fusion.fusion as F
    params, _ = scheme(secpar)
    rows, B, w, rb = TABLE["signature"][secpar]
    keys = [F.keygen(params, 700 + k) for k in range(3)]
    vks = [k[1] for k in keys]
    msgs = [f"from-bytes-{secpar}-{k}" for k in range(3)]
    blobs = [F.to_bytes(params, F.sign(params, keys[k], msgs[k])) for k in range(3)]
    agg = F.aggregate_from_bytes(params, vks, msgs, blobs)
    want = F.aggregate(params, vks, msgs, [F.from_bytes(params, "signature", b) for b in blobs])
    assert isinstance(agg, F.Signature) and str(agg) == str(want)
    assert F.verify(params, vks, msgs, agg) == (True, "")
    bad = list(blobs)
    bad[1] = set_field(np.frombuffer(blobs[1], dtype=np.uint8), 5, 2 * B + 1, w).tobytes()
    with pytest.raises(ValueError, match=r"record 1: Encoding is not canonical\."):
        F.aggregate_from_bytes(params, vks, msgs, bad)
    with pytest.raises(ValueError):
        F.aggregate_from_bytes(params, vks, msgs, [blobs[0], blobs[1][:-1], blobs[2]])
    with pytest.raises(ValueError):
        F.aggregate_from_bytes(params, vks, msgs[:2], blobs)


@pytest.mark.parametrize("secpar", [128, 256])
def test_device_resident_and_other_input_forms(secpar):
    from fusion_hip import DeviceArray
    _, bs = scheme(secpar)
    vk, msgs, sig = signed_batch(bs, 3, "forms")
    data, _ = bs.encode("signature", sig)
    want = bs.aggregate(vk, msgs, sig)
    b = data.tobytes()
    dB = DeviceArray.from_numpy(bs.ctx, data)
    try:
        for form in (b, bytearray(b), memoryview(b), data, data.ravel(), dB, dB):
            out, codes = bs.aggregate_encoded(vk, msgs, form)
            assert codes.tolist() == [0, 0, 0] and np.array_equal(out, want)
        assert np.array_equal(dB.numpy(), data)                    # still there: the call did not free it
    finally:
        dB.free()
