"""The compact byte encoding on the device (BatchScheme.encode / decode, fz_encode_records_async / fz_decode_records_async, the
object face's to_bytes / from_bytes): bit for bit the numpy spec of tests/test_encoding_host.py and the golden digests, round
trips at every batch shape, the bounds exactly, canonicity, graph capture, and decoded signatures straight into verification
and aggregation."""
import hashlib
import json
import os

import numpy as np
import pytest

from test_encoding_host import GOLDEN_OBJECTS, TABLE, golden_rows, spec_encode, spec_pack

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
_SCHEMES = {}


def scheme(secpar):
    import fusion.fusion as F
    from fusion_hip.scheme import BatchScheme
    if secpar not in _SCHEMES:
        with open(os.path.join(G, "scheme.json")) as fh:
            seed = json.load(fh)[str(secpar)]["setup_seed"]
        params = F.fusion_setup(secpar, seed)
        _SCHEMES[secpar] = (params, BatchScheme(params, threads=4))
    return _SCHEMES[secpar]


def honest_rows(bs, kind, n, seed):
    """-> (rows as the device holds them, the centred integers z the encoding carries): coefficient-domain rows drawn in
    [-B, B] and carried over with the forward transform; keys: any int32"""
    rows, B, w, _ = TABLE[kind][bs.params.secpar]
    rng = np.random.default_rng(seed)
    if kind == "vk":
        x = rng.integers(-2 ** 31, 2 ** 31, size=(n, rows, bs.d), dtype=np.int64).astype(np.int32)
        return x, (x.astype(np.int64) + bs.q // 2) % bs.q - bs.q // 2
    z = rng.integers(-B, B + 1, size=(n, rows, bs.d), dtype=np.int64).astype(np.int32)
    return bs.ctx.ntt_forward(z.reshape(-1, bs.d)).reshape(z.shape), z.astype(np.int64)


def set_field(record, j, u, w):
    """a copy of one record's bytes with field j set to u"""
    bits = np.unpackbits(record, bitorder="little").reshape(-1, w)
    bits[j] = (np.int64(u) >> np.arange(w, dtype=np.int64)) & 1
    return np.packbits(bits.ravel(), bitorder="little")


# ---- golden and round trip -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("secpar", [128, 256])
def test_golden_bytes_equal_the_spec_and_the_digests(secpar):
    _, bs = scheme(secpar)
    with open(os.path.join(G, "encoding.json")) as fh:
        want = json.load(fh)[str(secpar)]
    for name, (kind, key) in GOLDEN_OBJECTS.items():
        rows = golden_rows(secpar, key)
        data, codes = bs.encode(kind, rows)
        assert data.dtype == np.uint8 and data.shape == (rows.shape[0], TABLE[kind][secpar][3])
        assert codes.dtype == np.int32 and codes.tolist() == [0] * rows.shape[0]
        assert np.array_equal(data, spec_encode(secpar, kind, rows)), (secpar, name)
        assert hashlib.sha3_256(data.tobytes()).hexdigest() == want[name], (secpar, name)
        back, codes = bs.decode(kind, data.tobytes())
        assert codes.tolist() == [0] * rows.shape[0] and np.array_equal(back, rows)
    # one [l][d] aggregate is N = 1
    agg = golden_rows(secpar, "agg_4")[0]
    assert np.array_equal(bs.encode("aggregate", agg)[0], bs.encode("aggregate", agg[None])[0])


@pytest.mark.parametrize("secpar", [128, 256])
@pytest.mark.parametrize("kind", sorted(TABLE))
@pytest.mark.parametrize("n", [1, 2, 3, 5, 64, 1024])
def test_round_trip(secpar, kind, n):
    from fusion_hip import DeviceArray
    _, bs = scheme(secpar)
    rows, B, w, rb = TABLE[kind][secpar]
    x, z = honest_rows(bs, kind, n, 1000 * n + secpar + len(kind))
    data, codes = bs.encode(kind, x)
    assert data.shape == (n, rb) and codes.tolist() == [0] * n
    pick = np.arange(n) if n <= 64 else np.array([0, 1, n // 2, n - 2, n - 1])
    assert np.array_equal(data[pick], spec_pack(z[pick], B, w))
    want = x if kind != "vk" else z.astype(np.int32)                 # decode(encode(x)) == cent(x mod q)
    for device in (False, True):
        back, codes = bs.decode(kind, data, device=device)
        assert codes.tolist() == [0] * n
        if device:
            assert isinstance(back, DeviceArray) and back.shape == (n, rows, bs.d) and back.dtype == np.int32
            dB = DeviceArray.from_numpy(bs.ctx, data)
            again, codes = bs.encode(kind, back)                   # encode(decode(b)) == b, all on the device
            assert codes.tolist() == [0] * n and np.array_equal(again, data)
            back2, _ = bs.decode(kind, dB)                          # a uint8 DeviceArray as input
            assert np.array_equal(back2, want)
            back, _ = back.numpy(), back.free()
            dB.free()
        assert np.array_equal(back, want)
    assert np.array_equal(bs.encode(kind, want)[0], data)


@pytest.mark.parametrize("secpar", [128, 256])
def test_input_forms_of_decode(secpar):
    _, bs = scheme(secpar)
    x, _ = honest_rows(bs, "signature", 3, 5)
    data, _ = bs.encode("signature", x)
    b = data.tobytes()
    for form in (b, bytearray(b), memoryview(b), data, data.ravel()):
        back, codes = bs.decode("signature", form)
        assert codes.tolist() == [0, 0, 0] and np.array_equal(back, x)


# ---- bounds and canonicity -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("secpar", [128, 256])
@pytest.mark.parametrize("kind", ["signature", "aggregate"])
def test_bounds_exactly(secpar, kind):
    params, bs = scheme(secpar)
    rows, B, w, rb = TABLE[kind][secpar]
    assert B == (int(params.beta_vf) if kind == "aggregate" else {128: 4264, 256: 3172}[secpar])
    n, i = 5, 2
    _, z = honest_rows(bs, kind, n, 77 + secpar)
    z[:, 0, 0], z[:, -1, -1], z[:, 1, 3] = B, -B, B                  # the bound itself encodes
    fwd = lambda zz: bs.ctx.ntt_forward(zz.astype(np.int32).reshape(-1, bs.d)).reshape(zz.shape)
    base, codes = bs.encode(kind, fwd(z))
    assert codes.tolist() == [0] * n and np.array_equal(base, spec_pack(z, B, w))
    for over in (B + 1, -B - 1):
        for pos in ((0, 0), (rows - 1, bs.d - 1), (rows // 2, 7)):
            zz = z.copy()
            zz[i][pos] = over
            data, codes = bs.encode(kind, fwd(zz))
            assert codes.tolist() == [4 if k == i else 0 for k in range(n)], (over, pos)
            assert not data[i].any()
            assert np.array_equal(np.delete(data, i, 0), np.delete(base, i, 0))


@pytest.mark.parametrize("secpar", [128, 256])
def test_over_norm_signatures_agree_with_verify_signatures(secpar):
    _, bs = scheme(secpar)
    n = 12
    seeds = [31 + 7 * k for k in range(n)]
    msgs = [f"enc-{secpar}-{k}" for k in range(n)]
    sk, vk = bs.keygen_batch(seeds)
    sig = bs.sign_batch(sk, vk, msgs)
    # the over_norm recipe of test_gpu_signature_screening.py: secret rows far above beta_sk, signed with the context's cores
    rng = np.random.default_rng(secpar)
    loud = [3, 4, 9]
    coef = rng.integers(-10 ** 4, 10 ** 4 + 1, size=(len(loud), 2, bs.l, bs.d)).astype(np.int32)
    lsk, lvk = bs.ctx.keygen_core(bs.A, coef)
    for k, j in enumerate(loud):
        vk[j], msgs[j] = lvk[k], f"loud-{secpar}-{k}"
    c_hat, _ = bs.challenges(lvk, [msgs[j] for j in loud])
    sig[loud] = bs.ctx.sign_core(lsk, c_hat)
    verdicts = bs.verify_signatures(vk, msgs, sig)
    _, codes = bs.encode("signature", sig)
    assert sorted(np.flatnonzero(codes == 4).tolist()) == loud
    assert ((codes == 4) == (verdicts == 4)).all() and set(codes.tolist()) <= {0, 4}


@pytest.mark.parametrize("secpar", [128, 256])
@pytest.mark.parametrize("kind", sorted(TABLE))
def test_non_canonical_records_are_refused_alone(secpar, kind):
    _, bs = scheme(secpar)
    rows, B, w, rb = TABLE[kind][secpar]
    n = 5
    x, _ = honest_rows(bs, kind, n, 11 + secpar)
    data, _ = bs.encode(kind, x)
    good, _ = bs.decode(kind, data)
    fields = rows * bs.d
    bad_values = [2 * B + 1, (1 << w) - 1]
    if kind == "vk":
        assert 2 * B + 1 == bs.q
        bad_values += [bs.q + 1, 2 ** 31 - 2]
    for i in (0, 2, n - 1):
        for u in bad_values:
            for j in (0, fields // 3, fields - 1):
                d2 = data.copy()
                d2[i] = set_field(d2[i], j, u, w)
                back, codes = bs.decode(kind, d2)
                assert codes.tolist() == [6 if k == i else 0 for k in range(n)], (i, u, j)
                assert not back[i].any()
                assert np.array_equal(np.delete(back, i, 0), np.delete(good, i, 0))


# ---- integration -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("secpar", [128, 256])
def test_lengths_and_empty_batches(secpar):
    from fusion_hip import FusionHipError
    from fusion_hip._lib import FZ_E_BADARG
    from fusion_hip.scheme import encoded_size
    params, bs = scheme(secpar)
    for kind in TABLE:
        rb = encoded_size(params, kind)
        for nbytes in (1, rb - 1, rb + 1, 2 * rb + 16):
            with pytest.raises(FusionHipError) as e:
                bs.decode(kind, bytes(nbytes))
            assert e.value.code == FZ_E_BADARG
        rows = TABLE[kind][secpar][0]
        data, codes = bs.encode(kind, np.zeros((0, rows, bs.d), dtype=np.int32))
        assert data.shape == (0, rb) and codes.shape == (0,)
        back, codes = bs.decode(kind, b"")
        assert back.shape == (0, rows, bs.d) and codes.shape == (0,)
    with pytest.raises(FusionHipError) as e:
        bs.encode("signature", np.zeros((2, 2, bs.d), dtype=np.int32))
    assert e.value.code == FZ_E_BADARG
    # the C entries' own checks: a bound out of range, rows < 1
    from fusion_hip import DeviceArray
    ctx = bs.ctx
    rows = TABLE["signature"][secpar][0]
    dX, dB, dV = DeviceArray(ctx, (1, rows, bs.d)), DeviceArray(ctx, (1, rows * bs.d * 4), np.uint8), DeviceArray(ctx, (1,))
    for bound, r in ((0, rows), ((bs.q - 1) // 2 + 1, rows), (5, 0)):
        with pytest.raises(FusionHipError) as e:
            ctx.encode_records_async_dev(dX.ptr, 1, r, True, bound, dB.ptr, dV.ptr)
        assert e.value.code == FZ_E_BADARG
        with pytest.raises(FusionHipError) as e:
            ctx.decode_records_async_dev(dB.ptr, 1, r, True, bound, dX.ptr, dV.ptr)
        assert e.value.code == FZ_E_BADARG
    with pytest.raises(FusionHipError) as e:
        ctx.encode_records_async_dev(dX.ptr + 4, 1, rows, True, 5, dB.ptr, dV.ptr)      # misaligned
    assert e.value.code == FZ_E_BADARG
    for b in (dX, dB, dV):
        b.free()


@pytest.mark.parametrize("secpar", [128, 256])
def test_decoded_signatures_feed_verification_and_aggregation(secpar):
    _, bs = scheme(secpar)
    S = np.load(os.path.join(G, f"scheme_{secpar}.npz"))
    with open(os.path.join(G, "scheme.json")) as fh:
        msgs = json.load(fh)[str(secpar)]["messages"]
    data, codes = bs.encode("signature", S["sig"])
    assert codes.tolist() == [0] * 4
    dS, codes = bs.decode("signature", data.tobytes(), device=True)
    kb, _ = bs.encode("vk", S["vk"])
    dK, _ = bs.decode("vk", kb, device=True)
    try:
        assert codes.tolist() == [0] * 4
        assert bs.verify_signatures(dK, msgs, dS).tolist() == [0] * 4
        assert np.array_equal(bs.aggregate(S["vk"], msgs, dS), S["agg_4"])
    finally:
        dS.free()
        dK.free()


def test_a_launch_larger_than_the_resident_grid():
    """4096 signatures at secpar 128: 4096 * 195 * 64 values are 49 920 chunks, several per wave of the capped grid"""
    _, bs = scheme(128)
    rows, B, w, rb = TABLE["signature"][128]
    x, z = honest_rows(bs, "signature", 4096, 4096)
    data, codes = bs.encode("signature", x)
    assert not codes.any() and data.shape == (4096, rb)
    pick = np.array([0, 1, 1234, 2047, 2048, 4095])
    assert np.array_equal(data[pick], spec_pack(z[pick], B, w))
    back, codes = bs.decode("signature", data)
    assert not codes.any() and np.array_equal(back, x)


@pytest.mark.parametrize("secpar", [128, 256])
def test_graph_capture_replays_the_pair(secpar):
    import fusion.fusion as F
    from fusion_hip import DeviceArray
    from fusion_hip.scheme import BatchScheme
    params, shared = scheme(secpar)
    rows, B, w, rb = TABLE["signature"][secpar]
    n = 7
    x, _ = honest_rows(shared, "signature", n, 3 + secpar)
    x[3, 0, 0] += 12345                                            # one record over the bound: status and zeroing replay too
    want_b, want_c = shared.encode("signature", x)
    bs = BatchScheme(params, private_context=True)
    try:
        ctx = bs.ctx
        dX = DeviceArray.from_numpy(ctx, x)
        dB, dV = DeviceArray(ctx, (n, rb), np.uint8), DeviceArray(ctx, (n,))
        dR, dW = DeviceArray(ctx, (n, rows, bs.d)), DeviceArray(ctx, (n,))
        want_r, want_w = shared.decode("signature", want_b)
        ctx.graph_begin()
        ctx.encode_records_async_dev(dX.ptr, n, rows, True, B, dB.ptr, dV.ptr)
        ctx.decode_records_async_dev(dB.ptr, n, rows, True, B, dR.ptr, dW.ptr)
        g = ctx.graph_end()
        for _ in range(2):
            # stale contents must not survive a replay: every output poisoned, the status words included (a graph that lost the
            # captured clearing of d_status would keep them)
            ctx.h2d(dB.ptr, np.full((n, rb), 0xff, dtype=np.uint8))
            ctx.h2d(dR.ptr, np.full((n, rows, bs.d), 0x7f7f7f7f, dtype=np.int32))
            for dS in (dV, dW):
                ctx.h2d(dS.ptr, np.full(n, 0x7f7f7f7f, dtype=np.int32))
            g.launch()
            ctx.synchronize()
            assert np.array_equal(dB.numpy(), want_b) and np.array_equal(dV.numpy(), want_c)
            assert np.array_equal(dR.numpy(), want_r) and np.array_equal(dW.numpy(), want_w)
        assert want_c.tolist() == [4 if k == 3 else 0 for k in range(n)] and not want_b[3].any()
        g.destroy()
        for b in (dX, dB, dV, dR, dW):
            b.free()
    finally:
        bs.close()


@pytest.mark.parametrize("coef", [True, False])
@pytest.mark.parametrize("n", [1, 33, 1025])
def test_c_abi_stream_ending_in_half_a_unit(coef, n):
    """the C entries with rows = 1 and bound = 2 at degree 64: w = 3, 24-byte records, so an odd n ends the byte stream 8 bytes
    into a 16-byte unit, which the kernels read and write as 8 bytes.  Bit for bit the spec, nothing past the stream, the rows
    or the status words is touched, and a bad last field of the last record is refused alone."""
    from fusion_hip import DeviceArray
    _, bs = scheme(128)
    ctx, d = bs.ctx, bs.d
    B, w, rb, guard = 2, 3, 24, 64
    assert d == 64 and d * w // 8 == rb and (n * rb) % 16 == 8
    rng = np.random.default_rng(n + 2 * coef)
    z = rng.integers(-B, B + 1, size=(n, 1, d)).astype(np.int32)
    z[-1, 0, -1], z[0, 0, 0] = B, -B
    x = ctx.ntt_forward(z.reshape(-1, d)).reshape(z.shape) if coef else z
    dX = DeviceArray.from_numpy(ctx, x)
    dB = DeviceArray.from_numpy(ctx, np.full(n * rb + guard, 0xab, dtype=np.uint8))
    dV = DeviceArray.from_numpy(ctx, np.full(n + 16, 0x7f7f7f7f, dtype=np.int32))
    dR = DeviceArray.from_numpy(ctx, np.full((n + 1, 1, d), 0x5a5a5a5a, dtype=np.int32))
    try:
        ctx.encode_records_async_dev(dX.ptr, n, 1, coef, B, dB.ptr, dV.ptr)
        got, st = dB.numpy(), dV.numpy()
        assert np.array_equal(got[:n * rb].reshape(n, rb), spec_pack(z, B, w))
        assert (got[n * rb:] == 0xab).all() and not st[:n].any() and (st[n:] == 0x7f7f7f7f).all()
        ctx.decode_records_async_dev(dB.ptr, n, 1, coef, B, dR.ptr, dV.ptr)
        back, st = dR.numpy(), dV.numpy()
        assert np.array_equal(back[:n], x) and (back[n] == 0x5a5a5a5a).all()
        assert not st[:n].any() and (st[n:] == 0x7f7f7f7f).all()
        bad = got[:n * rb].reshape(n, rb).copy()
        bad[-1] = set_field(bad[-1], d - 1, (1 << w) - 1, w)
        ctx.h2d(dB.ptr, bad)
        ctx.decode_records_async_dev(dB.ptr, n, 1, coef, B, dR.ptr, dV.ptr)
        back, st = dR.numpy(), dV.numpy()
        assert st[:n].tolist() == [0] * (n - 1) + [6] and (st[n:] == 0x7f7f7f7f).all()
        assert not back[n - 1].any() and np.array_equal(back[:n - 1], x[:n - 1]) and (back[n] == 0x5a5a5a5a).all()
        assert (dB.numpy()[n * rb:] == 0xab).all()
    finally:
        for b in (dX, dB, dV, dR):
            b.free()


# ---- object face -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("secpar", [128, 256])
def test_object_face_round_trip(secpar):
    import fusion.fusion as F
    from fusion_hip.scheme import encoded_size
    params, _ = scheme(secpar)
    keys = [F.keygen(params, 500 + k) for k in range(3)]
    msgs = [f"bytes-{secpar}-{k}" for k in range(3)]
    sigs = [F.sign(params, keys[k], msgs[k]) for k in range(3)]
    agg = F.aggregate(params, [k[1] for k in keys], msgs, sigs)
    vks = []
    for (_, vk), s in zip(keys, sigs):
        b = F.to_bytes(params, vk)
        assert isinstance(b, bytes) and len(b) == encoded_size(params, "vk")
        vk2 = F.from_bytes(params, "vk", b)
        assert str(vk2) == str(vk) and F.to_bytes(params, vk2) == b
        vks.append(vk2)
        sb = F.to_bytes(params, s)
        assert len(sb) == encoded_size(params, "signature")
        s2 = F.from_bytes(params, "signature", sb)
        assert str(s2) == str(s) and F.to_bytes(params, s2) == sb
    ab = F.to_bytes(params, agg, aggregate=True)
    assert len(ab) == encoded_size(params, "aggregate")
    agg2 = F.from_bytes(params, "aggregate", ab)
    assert str(agg2) == str(agg)
    assert F.verify(params, vks, msgs, agg2) == (True, "")
    # tampered: a field above 2B, a wrong length, an aggregate over the single-signature bound
    w = TABLE["signature"][secpar][2]
    bad = bytearray(sb)
    bad[0], bad[1] = 0xff, bad[1] | ((1 << (w - 8)) - 1)
    with pytest.raises(ValueError, match="Encoding is not canonical."):
        F.from_bytes(params, "signature", bytes(bad))
    with pytest.raises(ValueError):
        F.from_bytes(params, "signature", sb[:-1])
    with pytest.raises(ValueError):
        F.from_bytes(params, "vk", sb)
    from fusion_hip.scheme import signature_from_object
    _, bs = scheme(secpar)
    if np.abs(bs.ctx.ntt_inverse(signature_from_object(params, agg))).max() > TABLE["signature"][secpar][1]:
        with pytest.raises(ValueError, match="Norm too large to encode."):
            F.to_bytes(params, agg)
    else:
        assert F.to_bytes(params, agg) != ab
