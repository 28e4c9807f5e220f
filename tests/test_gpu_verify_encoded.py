"""Verification straight from the compact byte encoding on the device (fz_verify_encoded_async, BatchScheme.verify_signatures_encoded,
aggregate_encoded_screened, verify_encoded, fusion.fusion.verify_signatures_from_bytes / verify_from_bytes): the reference-made
golden signatures and aggregates, the numpy spec at every chunk geometry and in both grid forms, the existing decode ->
verify_signatures / aggregate_screened / verify paths, canonicity, graph capture, the object face and device-resident input.
No tolerance anywhere."""
import json
import os

import numpy as np
import pytest

from test_encoding_host import TABLE, spec_pack
from test_gpu_aggregate_encoded import cent, oracle, signed_batch, spoil
from test_gpu_encoding import scheme, set_field
from test_verify_encoded_host import aggregate_target, get_field, keyed_targets, spec_verdicts

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
POISON = 0x7f7f7f7f


def c_forward(bs):
    """the C oracle's forward transform of [.., d] rows of centred integers -> int64"""
    O, orc = oracle()
    root = O.PARAMS[bs.params.secpar]["root"]

    def fwd(z):
        z = np.asarray(z)
        return orc.ntt_forward(np.ascontiguousarray(z, dtype=np.int32).reshape(-1, bs.d), bs.q, root).reshape(z.shape).astype(np.int64)
    return fwd


def num_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def run_entry(ctx, A, data, n, l, bound, target=None, vk=None, c_hat=None, guard=0):
    """fz_verify_encoded_async on host arrays -> verdicts [n]; the bytes (and `guard` bytes of 0xab behind them) are unchanged and
    the words behind the verdicts untouched"""
    from fusion_hip import DeviceArray
    raw = np.concatenate([np.asarray(data, dtype=np.uint8).ravel(), np.full(guard, 0xab, dtype=np.uint8)])
    bufs = dict(B=DeviceArray.from_numpy(ctx, raw), A=DeviceArray.from_numpy(ctx, np.ascontiguousarray(A, dtype=np.int32)),
                V=DeviceArray.from_numpy(ctx, np.full(n + 16, POISON, dtype=np.int32)))
    for name, a in (("T", target), ("K", vk), ("C", c_hat)):
        if a is not None:
            bufs[name] = DeviceArray.from_numpy(ctx, np.ascontiguousarray(a, dtype=np.int32))
    ptr = lambda k: bufs[k].ptr if k in bufs else 0
    try:
        ctx.verify_encoded_async_dev(ptr("A"), ptr("B"), n, l, bound, ptr("T"), ptr("K"), ptr("C"), ptr("V"))
        v, b = bufs["V"].numpy(), bufs["B"].numpy()
        assert (v[n:] == POISON).all() and np.array_equal(b, raw)
        return v[:n]
    finally:
        for x in bufs.values():
            x.free()


def other_value(u, B):
    """a field value in [0, 2B] next to u"""
    return u + 1 if u < 2 * B else u - 1


# ---- golden ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("secpar", [128, 256])
def test_golden_signatures_and_aggregates(secpar):
    _, bs = scheme(secpar)
    S = np.load(os.path.join(G, f"scheme_{secpar}.npz"))
    with open(os.path.join(G, "scheme.json")) as fh:
        J = json.load(fh)[str(secpar)]
    assert np.array_equal(bs.A.reshape(S["A"].shape), S["A"])
    rows, B, w, rb = TABLE["signature"][secpar]
    data, codes = bs.encode("signature", S["sig"])
    assert not codes.any()
    assert run_entry(bs.ctx, S["A"], data, 4, rows, B, vk=S["vk"], c_hat=S["c_hat"]).tolist() == [0, 0, 0, 0]
    assert run_entry(bs.ctx, S["A"], data, 4, rows, B, target=cent(keyed_targets(bs.q, S["vk"], S["c_hat"]), bs.q)).tolist() == [0] * 4
    got = bs.verify_signatures_encoded(S["vk"], J["messages"], data.tobytes())
    assert got.dtype == np.int32 and got.tolist() == [0, 0, 0, 0]
    out, codes = bs.aggregate_encoded_screened(S["vk"], J["messages"], data)
    assert codes.tolist() == [0, 0, 0, 0] and out.dtype == np.int32 and np.array_equal(out, S["agg_4"])
    rows, B, w, rb = TABLE["aggregate"][secpar]
    for k in (1, 2, 4):
        order = J["agg"][str(k)]["order"]
        rec, codes = bs.encode("aggregate", S[f"agg_{k}"])
        assert codes.tolist() == [0] and rec.shape == (1, rb)
        t = cent(aggregate_target(bs.q, S["vk"][order], S["c_hat"][order], S[f"alpha_hat_{k}"]), bs.q)
        assert run_entry(bs.ctx, S["A"], rec, 1, rows, B, target=t[None]).tolist() == [0], (secpar, k)
        keys, msgs = S["vk"][:k], J["messages"][:k]
        assert bs.verify_encoded(keys, msgs, rec.tobytes()) == (True, "") == bs.verify(keys, msgs, S[f"agg_{k}"])
        bad = set_field(rec[0], 4321, other_value(get_field(rec[0], 4321, w), B), w)
        assert bs.verify_encoded(keys, msgs, bad) == (False, "Target doesn't match image of aggregate signature.")
        assert bs.verify_encoded(keys, msgs, bad) == bs.verify(keys, msgs, bs.decode("aggregate", bad)[0][0])
        assert bs.verify_encoded(keys, msgs, set_field(rec[0], 4321, 2 * B + 1, w)) == (False, "Encoding is not canonical.")
        assert bs.verify_encoded(keys, msgs[:-1] + [msgs[-1] + "?"], rec)[0] is False


# ---- chunk geometry: free l and bound through the C entry --------------------------------------------------------------------
@pytest.mark.parametrize("secpar,l", [(256, 1), (256, 4), (256, 5), (256, 83), (128, 2), (128, 16), (128, 18), (128, 195)])
def test_chunk_geometry(secpar, l):
    """degree 256: a 256-value tail only, exactly one chunk, a chunk and a one-row tail, the real record; degree 64 likewise; field
    widths 2, the kind's 13 / 14, and 31"""
    from fusion_hip import FusionHipError
    from fusion_hip._lib import FZ_E_UNSUPPORTED
    _, bs = scheme(secpar)
    d, n, q = bs.d, 3, bs.q
    fwd = c_forward(bs)
    for B in (1, TABLE["signature"][secpar][1], (q - 1) // 2):
        w = (2 * B).bit_length()
        rng = np.random.default_rng(l + w + secpar)
        A = rng.integers(I32_MIN, I32_MAX + 1, size=(l, d), dtype=np.int64)
        A[0, 0], A[-1, -1], A[0, 1], A[-1, -2] = I32_MIN, I32_MAX, I32_MAX, I32_MIN
        if (l * d * w // 8) % 16:                                  # degree 64 with l * w odd (195 x 31): the entry refuses such records
            assert d == 64 and l * w % 2 == 1
            with pytest.raises(FusionHipError) as e:
                run_entry(bs.ctx, A, np.zeros((n, l * d * w // 8), dtype=np.uint8), n, l, B, target=np.zeros((n, d), dtype=np.int32))
            assert e.value.code == FZ_E_UNSUPPORTED
            continue
        u = rng.integers(0, 2 * B + 1, size=(n, l, d), dtype=np.int64)
        u[0, 0, 0], u[1, -1, -1], u[2, 0, 1], u[2, -1, -2] = 0, 2 * B, 2 * B, 0
        data = spec_pack(u - B, B, w)
        assert data.shape == (n, l * d * w // 8)
        codes, sums = spec_verdicts(q, data, A, np.zeros((n, d), dtype=np.int64), B, w, fwd)
        assert sums.any() and set(codes.tolist()) == {3}
        t = cent(sums, q)
        assert spec_verdicts(q, data, A, t, B, w, fwd)[0].tolist() == [0] * n
        assert run_entry(bs.ctx, A, data, n, l, B, target=t, guard=64).tolist() == [0] * n, (secpar, l, B)
        # the same residues, every positive word as word - q
        assert run_entry(bs.ctx, A, data, n, l, B, target=np.where(t > 0, t - q, t), guard=64).tolist() == [0] * n, (secpar, l, B)
        for rec, pos in ((0, 0), (0, d - 1), (n - 1, d // 2 + 3), (n - 1, d - 1)):
            t2 = t.copy()
            t2[rec, pos] += 1 if t2[rec, pos] < 0 else -1
            want = [3 if i == rec else 0 for i in range(n)]
            assert run_entry(bs.ctx, A, data, n, l, B, target=t2).tolist() == want, (secpar, l, B, rec, pos)
        # one field of the LAST valid row (the tail chunk's last row), in the first and in the last record
        for rec, j in ((0, (l - 1) * d + 5), (n - 1, l * d - 1)):
            d2 = data.copy()
            d2[rec] = set_field(d2[rec], j, other_value(get_field(d2[rec], j, w), B), w)
            want = [3 if i == rec else 0 for i in range(n)]
            assert spec_verdicts(q, d2, A, t, B, w, fwd)[0].tolist() == want
            assert run_entry(bs.ctx, A, d2, n, l, B, target=t, guard=64).tolist() == want, (secpar, l, B, rec, j)
            if rec == 0:
                # the same three records tiled past the switch to ONE workgroup per record (the runs above shared a record
                # among several whenever it has more than four chunks)
                big = 2 * num_cu() + 2
                idx = np.arange(big) % n
                assert run_entry(bs.ctx, A, d2[idx], big, l, B, target=t[idx], guard=64).tolist() == [want[i] for i in idx]
            d2[rec] = set_field(d2[rec], j, 2 * B + 1, w)          # ... and above 2B there: no value at all
            want = [6 if i == rec else 0 for i in range(n)]
            assert run_entry(bs.ctx, A, d2, n, l, B, target=t, guard=64).tolist() == want, (secpar, l, B, rec, j)


# ---- both grid forms -------------------------------------------------------------------------------------------------------
def encoded_mixture(bs, n, seed):
    """n signers, each honest, tampered inside the bound (one field of the record moved by one), with the message changed or
    with the keys swapped with the next signer -> (vk, msgs, data)"""
    rows, B, w, rb = TABLE["signature"][bs.params.secpar]
    rng = np.random.default_rng(seed)
    vk, msgs, sig = signed_batch(bs, n, f"mix{seed}")
    data, codes = bs.encode("signature", sig)
    assert not codes.any()
    vk, msgs = vk.copy(), list(msgs)
    kind = rng.integers(0, 4, size=n) if n > 1 else np.array([seed % 2])
    for i in range(n):
        if kind[i] == 1:
            j = int(rng.integers(rows * bs.d))
            data[i] = set_field(data[i], j, other_value(get_field(data[i], j, w), B), w)
        elif kind[i] == 2:
            msgs[i] = msgs[i] + "!"
        elif kind[i] == 3 and n > 1:
            j = (i + 1) % n
            vk[[i, j]] = vk[[j, i]]
    return vk, msgs, data


def switch_counts():
    """record counts on either side of the launcher's switch: R = min(chunks / 4, 2 num_cu / N) workgroups per record, so N = num_cu
    is the last count with two workgroups per record and num_cu + 1 the first with one"""
    return num_cu(), num_cu() + 1


@pytest.mark.parametrize("secpar", [128, 256])
@pytest.mark.parametrize("n", [1, 7, "below", "above", 1024])
def test_both_grid_forms_equal_the_spec_and_the_decoded_path(secpar, n):
    _, bs = scheme(secpar)
    if isinstance(n, str):
        n = switch_counts()[0 if n == "below" else 1]
    rows, B, w, rb = TABLE["signature"][secpar]
    vk, msgs, data = encoded_mixture(bs, n, 10 * n + secpar)
    got = bs.verify_signatures_encoded(vk, msgs, data)
    back, dcodes = bs.decode("signature", data, device=True)
    try:
        assert not dcodes.any()
        want = bs.verify_signatures(vk, msgs, back)
    finally:
        back.free()
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert set(want.tolist()) <= {0, 3}
    if n >= 7:
        assert set(want.tolist()) == {0, 3}
    if n <= 7:
        c_hat, _ = bs.challenges(vk, msgs)
        spec, _ = spec_verdicts(bs.q, data, bs.A.reshape(rows, bs.d), keyed_targets(bs.q, vk, c_hat), B, w, c_forward(bs))
        assert np.array_equal(got, spec)


def test_interleaved_calls_share_no_state():
    """a small-N call (several workgroups per record, the context's shared area), a large-N call (one workgroup each) and the
    small one again, verify() between them, twice over: the area is cleared by every call that uses it"""
    _, bs = scheme(256)
    small = encoded_mixture(bs, 5, 91)
    large = encoded_mixture(bs, 600, 92)
    lone = encoded_mixture(bs, 1, 94)
    want = {}
    for name, (vk, msgs, data) in (("small", small), ("large", large), ("lone", lone)):
        want[name] = bs.verify_signatures(vk, msgs, bs.decode("signature", data)[0])
    assert 0 < np.count_nonzero(want["large"]) < 600
    vk, msgs, sig = signed_batch(bs, 4, "between")
    agg = bs.aggregate(vk, msgs, sig)
    rec, _ = bs.encode("aggregate", agg)
    bad = agg.copy()
    bad[2, 2] += 1
    for _ in range(2):
        assert np.array_equal(bs.verify_signatures_encoded(*small), want["small"])
        assert bs.verify(vk, msgs, agg) == (True, "")
        assert bs.verify_encoded(vk, msgs, rec) == (True, "")
        assert np.array_equal(bs.verify_signatures_encoded(*large), want["large"])
        assert np.array_equal(bs.verify_signatures_encoded(*lone), want["lone"])
        assert bs.verify(vk, msgs, bad)[0] is False
        assert np.array_equal(bs.verify_signatures_encoded(*small), want["small"])


# ---- canonicity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("secpar", [128, 256])
def test_records_that_are_not_canonical_get_code_6_first(secpar):
    _, bs = scheme(secpar)
    rows, B, w, rb = TABLE["signature"][secpar]
    n = 7
    vk, msgs, sig = signed_batch(bs, n, "canon")
    good, codes = bs.encode("signature", sig)
    assert not codes.any()
    data = spoil(good, secpar)
    assert bs.verify_signatures_encoded(vk, msgs, data).tolist() == [0, 0, 6, 0, 0, 6, 0]
    # a record that is tampered AND not canonical: 6; a tampered one beside it: 3
    data[2] = set_field(data[2], 99, other_value(get_field(data[2], 99, w), B), w)
    data[3] = set_field(data[3], 99, other_value(get_field(data[3], 99, w), B), w)
    assert bs.verify_signatures_encoded(vk, msgs, data).tolist() == [0, 0, 6, 3, 0, 6, 0]
    wrong = list(msgs)
    wrong[5] += "?"
    assert bs.verify_signatures_encoded(vk, wrong, data).tolist() == [0, 0, 6, 3, 0, 6, 0]
    every = np.full((n, rb), 0xff, dtype=np.uint8)
    assert bs.verify_signatures_encoded(vk, msgs, every).tolist() == [6] * n
    out, codes = bs.aggregate_encoded_screened(vk, msgs, every)
    assert out is None and codes.tolist() == [6] * n
    # the large-N form (one workgroup per record) on the same bytes, through the entry: every third record spoiled
    big = np.tile(good, (100, 1))[:600]
    big[::3, -1] = 0xff
    A = bs.A.reshape(rows, bs.d)
    c_hat, _ = bs.challenges(vk, msgs)
    idx = np.arange(600) % n
    got = run_entry(bs.ctx, A, big, 600, rows, B, vk=vk[idx], c_hat=c_hat[idx])
    assert got.tolist() == [6 if i % 3 == 0 else 0 for i in range(600)]


# ---- screened aggregation --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("secpar", [128, 256])
def test_screened_aggregation_equals_the_decoded_paths(secpar):
    _, bs = scheme(secpar)
    rows, B, w, rb = TABLE["signature"][secpar]
    n = 7
    vk, msgs, sig = signed_batch(bs, n, "screened")
    good, _ = bs.encode("signature", sig)
    data = good.copy()
    data[1] = set_field(data[1], 1000, other_value(get_field(data[1], 1000, w), B), w)          # tampered inside the bound
    data[4] = set_field(data[4], 0, 2 * B + 1, w)                                              # not canonical
    out, codes = bs.aggregate_encoded_screened(vk, msgs, data)
    assert codes.tolist() == [0, 3, 0, 0, 6, 0, 0]
    ok = codes == 0
    back, dcodes = bs.decode("signature", data)
    assert dcodes.tolist() == [0, 0, 0, 0, 6, 0, 0]
    m_ok = [m for m, k in zip(msgs, ok) if k]
    assert out.dtype == np.int32 and np.array_equal(out, bs.aggregate(vk[ok], m_ok, back[ok]))
    ref, rcodes = bs.aggregate_screened(vk, msgs, back)
    assert np.array_equal(out, ref) and np.array_equal(rcodes == 0, ok)
    assert bs.verify(vk[ok], m_ok, out) == (True, "")
    # every signer honest: aggregate_encoded's result
    out2, codes2 = bs.aggregate_encoded_screened(vk, msgs, good)
    want2, _ = bs.aggregate_encoded(vk, msgs, good)
    assert codes2.tolist() == [0] * n and np.array_equal(out2, want2) and np.array_equal(out2, bs.aggregate(vk, msgs, sig))


# ---- the entry's refusals --------------------------------------------------------------------------------------------------
def test_entry_refusals():
    from fusion_hip import DeviceArray, FusionHipError
    from fusion_hip._lib import FZ_E_BADARG, FZ_E_UNSUPPORTED
    _, bs = scheme(128)
    ctx, d = bs.ctx, bs.d
    dB = DeviceArray.from_numpy(ctx, np.zeros(4096, dtype=np.uint8))
    dA = DeviceArray.from_numpy(ctx, np.zeros((2, d), dtype=np.int32))
    dT = DeviceArray.from_numpy(ctx, np.zeros((3, d), dtype=np.int32))
    dK = DeviceArray.from_numpy(ctx, np.zeros((3, 2, d), dtype=np.int32))
    dC = DeviceArray.from_numpy(ctx, np.zeros((3, d), dtype=np.int32))
    dV = DeviceArray.from_numpy(ctx, np.full(8, POISON, dtype=np.int32))
    A, Bp, T, K, C, V = dA.ptr, dB.ptr, dT.ptr, dK.ptr, dC.ptr, dV.ptr
    try:
        with pytest.raises(FusionHipError) as e:                   # degree 64, l = 1, bound = 2: 24-byte records
            ctx.verify_encoded_async_dev(A, Bp, 2, 1, 2, T, 0, 0, V)
        assert e.value.code == FZ_E_UNSUPPORTED
        half = (bs.q - 1) // 2
        bad = [(A, Bp, 2, 2, 5, T, K, C, V), (A, Bp, 2, 2, 5, 0, 0, 0, V), (A, Bp, 2, 2, 5, T, K, 0, V), (A, Bp, 2, 2, 5, 0, K, 0, V),
               (A, Bp, 2, 2, 5, 0, 0, C, V),                                                  # both target forms, neither, half a pair
               (A, Bp, 2, 2, 0, T, 0, 0, V), (A, Bp, 2, 2, half + 1, T, 0, 0, V), (A, Bp, 2, 0, 5, T, 0, 0, V),      # bound, l
               (A, Bp + 4, 2, 2, 5, T, 0, 0, V), (A + 4, Bp, 2, 2, 5, T, 0, 0, V), (A, Bp, 2, 2, 5, T + 2, 0, 0, V),
               (A, Bp, 2, 2, 5, 0, K + 1, C, V), (A, Bp, 2, 2, 5, 0, K, C + 2, V), (A, Bp, 2, 2, 5, T, 0, 0, V + 1),  # alignment
               (0, Bp, 2, 2, 5, T, 0, 0, V), (A, 0, 2, 2, 5, T, 0, 0, V), (A, Bp, 2, 2, 5, T, 0, 0, 0)]                # NULL
        for args in bad:
            with pytest.raises(FusionHipError) as e:
                ctx.verify_encoded_async_dev(*args)
            assert e.value.code == FZ_E_BADARG, args[2:5]
        ctx.verify_encoded_async_dev(A, Bp, 0, 2, 5, T, 0, 0, V)   # N = 0: OK, nothing written
        ctx.verify_encoded_async_dev(A, Bp, 0, 2, 5, 0, K, C, V)
        ctx.synchronize()
        assert (dV.numpy() == POISON).all()
        # 4-byte aligned targets, keys, challenges and verdicts are taken: two zero records (u = 0, z = -5) against themselves
        ctx.verify_encoded_async_dev(A, Bp, 2, 2, 5, T + 4, 0, 0, V + 4)
        ctx.verify_encoded_async_dev(A, Bp, 2, 2, 5, 0, K + 4, C + 4, V + 12)
        ctx.synchronize()
        assert dV.numpy().tolist() == [POISON, 0, 0, 0, 0, POISON, POISON, POISON]
    finally:
        for x in (dB, dA, dT, dK, dC, dV):
            x.free()


# ---- graph capture ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("secpar", [128, 256])
def test_graph_capture_replays_both_forms(secpar):
    """on a private context, without a warm-up call (nothing is allocated by the entry): the keyed form at N = 7 and a lone record
    against a target array (several workgroups, the shared area and its clear are part of the captured work), replayed twice
    over poisoned verdicts"""
    from fusion_hip import DeviceArray
    from fusion_hip.scheme import BatchScheme
    params, shared = scheme(secpar)
    rows, B, w, rb = TABLE["signature"][secpar]
    n = 7
    vk, msgs, data = encoded_mixture(shared, n, 10 * n + secpar)
    data[3] = set_field(data[3], 17, 2 * B + 1, w)
    c_hat, _ = shared.challenges(vk, msgs)
    want7 = shared.verify_signatures_encoded(vk, msgs, data)
    assert want7[3] == 6 and set(want7.tolist()) == {0, 3, 6}
    t = cent(keyed_targets(shared.q, vk, c_hat), shared.q).astype(np.int32)
    honest_one = int(np.flatnonzero(want7 == 0)[0])
    other = (honest_one + 1) % n
    bs = BatchScheme(params, private_context=True)
    try:
        ctx = bs.ctx
        dA = DeviceArray.from_numpy(ctx, shared.A)
        dB, dK, dC, dT = (DeviceArray.from_numpy(ctx, a) for a in (data, vk, c_hat, t))
        dV, dW, dX = DeviceArray(ctx, (n,)), DeviceArray(ctx, (1,)), DeviceArray(ctx, (1,))
        ctx.graph_begin()
        ctx.verify_encoded_async_dev(dA.ptr, dB.ptr, n, rows, B, 0, dK.ptr, dC.ptr, dV.ptr)
        ctx.verify_encoded_async_dev(dA.ptr, dB.ptr + honest_one * rb, 1, rows, B, dT.ptr + honest_one * bs.d * 4, 0, 0, dW.ptr)
        ctx.verify_encoded_async_dev(dA.ptr, dB.ptr + honest_one * rb, 1, rows, B, dT.ptr + other * bs.d * 4, 0, 0, dX.ptr)      # another signer's target
        g = ctx.graph_end()
        for _ in range(2):
            for b, k in ((dV, n), (dW, 1), (dX, 1)):
                ctx.h2d(b.ptr, np.full(k, POISON, dtype=np.int32))
            g.launch()
            ctx.synchronize()
            assert np.array_equal(dV.numpy(), want7) and dW.numpy().tolist() == [0]
            assert dX.numpy().tolist() == [3]
        g.destroy()
        for b in (dA, dB, dK, dC, dT, dV, dW, dX):
            b.free()
    finally:
        bs.close()


# ---- input forms, device residency and the object face ---------------------------------------------------------------------
@pytest.mark.parametrize("secpar", [128, 256])
def test_device_resident_and_other_input_forms(secpar):
    from fusion_hip import DeviceArray
    _, bs = scheme(secpar)
    rows, B, w, rb = TABLE["signature"][secpar]
    vk, msgs, sig = signed_batch(bs, 3, "forms")
    data, _ = bs.encode("signature", sig)
    data[1] = set_field(data[1], 50, other_value(get_field(data[1], 50, w), B), w)
    ok = np.array([True, False, True])
    want = bs.aggregate(vk[ok], [msgs[0], msgs[2]], sig[ok])
    b = data.tobytes()
    dB, dK = DeviceArray.from_numpy(bs.ctx, data), DeviceArray.from_numpy(bs.ctx, vk)
    agg = bs.aggregate(vk, msgs, sig)
    rec, _ = bs.encode("aggregate", agg)
    dR = DeviceArray.from_numpy(bs.ctx, rec)
    try:
        for form in (b, bytearray(b), memoryview(b), data, data.ravel(), dB, dB):
            for keys in (vk, dK):
                assert bs.verify_signatures_encoded(keys, msgs, form).tolist() == [0, 3, 0]
                out, codes = bs.aggregate_encoded_screened(keys, msgs, form)
                assert codes.tolist() == [0, 3, 0] and np.array_equal(out, want)
        rb_ = rec.tobytes()
        for form in (rb_, bytearray(rb_), memoryview(rb_), rec, rec.ravel(), dR, dR):
            for keys in (vk, dK):
                assert bs.verify_encoded(keys, msgs, form) == (True, "")
        assert np.array_equal(dB.numpy(), data) and np.array_equal(dK.numpy(), vk) and np.array_equal(dR.numpy(), rec)   # not freed
    finally:
        for x in (dB, dK, dR):
            x.free()


@pytest.mark.parametrize("secpar", [128, 256])
def test_object_face(secpar):
    import fusion.fusion as F
    params, _ = scheme(secpar)
    rows, B, w, rb = TABLE["signature"][secpar]
    keys = [F.keygen(params, 700 + k) for k in range(3)]
    vks = [k[1] for k in keys]
    msgs = [f"verify-from-bytes-{secpar}-{k}" for k in range(3)]
    sigs = [F.sign(params, keys[k], msgs[k]) for k in range(3)]
    blobs = [F.to_bytes(params, s) for s in sigs]
    assert F.verify_signatures_from_bytes(params, vks, msgs, blobs) == [(True, "")] * 3
    bad = list(blobs)
    rec = np.frombuffer(blobs[1], dtype=np.uint8)
    bad[1] = set_field(rec, 5, other_value(get_field(rec, 5, w), B), w).tobytes()
    assert F.verify_signatures_from_bytes(params, vks, msgs, bad) == \
        [(True, ""), (False, "Target doesn't match image of signature."), (True, "")]
    bad[2] = set_field(np.frombuffer(blobs[2], dtype=np.uint8), 5, 2 * B + 1, w).tobytes()
    assert F.verify_signatures_from_bytes(params, vks, msgs, bad) == \
        [(True, ""), (False, "Target doesn't match image of signature."), (False, "Encoding is not canonical.")]
    with pytest.raises(ValueError):
        F.verify_signatures_from_bytes(params, vks, msgs, [blobs[0], blobs[1][:-1], blobs[2]])
    with pytest.raises(ValueError):
        F.verify_signatures_from_bytes(params, vks, msgs[:2], blobs)
    agg = F.aggregate(params, vks, msgs, sigs)
    blob = F.to_bytes(params, agg, aggregate=True)
    assert F.verify_from_bytes(params, vks, msgs, blob) == F.verify(params, vks, msgs, agg) == (True, "")
    wrong = msgs[:2] + ["other"]
    assert F.verify_from_bytes(params, vks, wrong, blob) == F.verify(params, vks, wrong, agg)
    assert F.verify_from_bytes(params, vks, wrong, blob) == (False, "Target doesn't match image of aggregate signature.")
    assert F.verify_from_bytes(params, vks[:2], msgs, blob) == F.verify(params, vks[:2], msgs, agg)
    _, Ba, wa, _ = TABLE["aggregate"][secpar]
    spoiled = set_field(np.frombuffer(blob, dtype=np.uint8), 0, 2 * Ba + 1, wa).tobytes()
    assert F.verify_from_bytes(params, vks, msgs, spoiled) == (False, "Encoding is not canonical.")
    with pytest.raises(ValueError):
        F.verify_from_bytes(params, vks, msgs, blob[:-1])
