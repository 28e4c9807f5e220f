"""Signing straight to the compact byte encoding on the device (fz_sign_encoded_async, BatchScheme.sign_batch_encoded,
fusion.fusion.sign_to_bytes): the reference-made golden keys and challenges, the existing sign -> encode pair at every walk shape,
the bound exactly at the first and last value of a record and in a chunk two records share, any int32 operand at every multiply
form and context of tests/_encoded_edges.py, every field width, graph capture with the keyed verification behind it, the
consumers of the bytes, the object face and the refusals of the C entry.  No tolerance anywhere."""
import hashlib
import json
import os

import numpy as np
import pytest

import _encoded_edges as X
import test_gpu_encoded_edges as GE
from test_encoding_host import TABLE, spec_encode, spec_pack
from test_gpu_encoding import scheme
from test_sign_encoded_host import spec_sign

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
BYTE_POISON, WORD_POISON = 0xab, 0x7f7f7f7f


def run_sign(ctx, sk_hat, c_hat, B):
    """fz_sign_encoded_async on sk_hat [N][2][l][n] and c_hat [N][n] -> (bytes [N][record bytes], status [N]); the guard bytes and
    the poisoned record area behind the stream and the status words behind the last one are untouched, the inputs unchanged"""
    N, _, l, n = sk_hat.shape
    rb = X.record_bytes(n, l, X.width(B))
    sk, c = np.ascontiguousarray(sk_hat, dtype=np.int32), np.ascontiguousarray(c_hat, dtype=np.int32).reshape(N, n)
    bufs = GE.Bufs(ctx)
    try:
        dK, dC = bufs.put(sk), bufs.put(c)
        dB = bufs.put(np.full(N * rb + rb + GE.GUARD, BYTE_POISON, dtype=np.uint8))
        dV = bufs.put(np.full(N + 16, WORD_POISON, dtype=np.int32))
        ctx.sign_encoded_async_dev(dK.ptr, dC.ptr, N, l, B, dB.ptr, dV.ptr)
        got, st = dB.numpy(), dV.numpy()
        assert (got[N * rb:] == BYTE_POISON).all() and (st[N:] == WORD_POISON).all()
        assert np.array_equal(dK.numpy(), sk) and np.array_equal(dC.numpy(), c)
        return got[:N * rb].reshape(N, rb), st[:N]
    finally:
        bufs.free()


def run_pair(ctx, sk_hat, c_hat, B):
    """the two existing entries: fz_sign_core, then fz_encode_records_async on its rows"""
    sig = ctx.sign_core(np.ascontiguousarray(sk_hat, dtype=np.int32), np.ascontiguousarray(c_hat, dtype=np.int32))
    return GE.run_encode(ctx, sig, True, B)


def solve_keys(q, sigma, seed):
    """(sk_hat [N][2][l][n], c_hat [N][n]) with cent(L (.) c + R) = sigma [N][l][n] (centred): L and c at random over all of int32,
    R = cent(sigma - cent(L c))"""
    rng = np.random.default_rng(seed)
    N, l, n = sigma.shape
    L = rng.integers(I32_MIN, I32_MAX + 1, size=(N, l, n), dtype=np.int64)
    c = rng.integers(I32_MIN, I32_MAX + 1, size=(N, n), dtype=np.int64)
    R = X.cent(np.asarray(sigma, dtype=np.int64) - X.cent(L * c[:, None, :], q), q)
    return np.stack([L, R], axis=1), c


def honest(bs, n, tag):
    seeds = [700 + 11 * k for k in range(n)]
    msgs = [f"{tag}-{bs.params.secpar}-{k}" for k in range(n)]
    sk, vk = bs.keygen_batch(seeds)
    return sk, vk, msgs


# ---- golden ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("secpar", [128, 256])
def test_golden_keys_give_the_spec_bytes_and_the_digest(secpar):
    _, bs = scheme(secpar)
    S = np.load(os.path.join(G, f"scheme_{secpar}.npz"))
    with open(os.path.join(G, "scheme.json")) as fh:
        msgs = json.load(fh)[str(secpar)]["messages"]
    with open(os.path.join(G, "encoding.json")) as fh:
        digest = json.load(fh)[str(secpar)]["sig"]
    rows, B, w, rb = TABLE["signature"][secpar]
    want = spec_encode(secpar, "signature", spec_sign(bs.q, S["sk_hat"], S["c_hat"]))
    data, st = run_sign(bs.ctx, S["sk_hat"], S["c_hat"], B)
    assert st.tolist() == [0] * 4 and np.array_equal(data, want)
    assert hashlib.sha3_256(data.tobytes()).hexdigest() == digest
    data, codes = bs.sign_batch_encoded(S["sk_hat"], S["vk"], msgs)
    assert data.dtype == np.uint8 and data.shape == (4, rb) and codes.dtype == np.int32 and codes.tolist() == [0] * 4
    assert np.array_equal(data, want) and hashlib.sha3_256(data.tobytes()).hexdigest() == digest


# ---- the existing pair at every walk shape -----------------------------------------------------------------------------------
@pytest.mark.parametrize("secpar", [128, 256])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 33, 67, 512])
def test_equals_sign_then_encode(secpar, n):
    """fewer tasks than waves of a workgroup's worth of records, record boundaries inside chunks (a record is 12.1875 / 20.75
    chunks), an uneven tail, and at 512 more wave-tasks than any resident grid"""
    _, bs = scheme(secpar)
    rows, B, w, rb = TABLE["signature"][secpar]
    sk, vk, msgs = honest(bs, n, "walk")
    c_hat, _ = bs.challenges(vk, msgs)
    want_b, want_c = bs.encode("signature", bs.sign_batch(sk, vk, msgs))
    data, st = run_sign(bs.ctx, sk, c_hat, B)
    assert st.tolist() == want_c.tolist() == [0] * n
    assert np.array_equal(data, want_b)
    if n <= 5:
        assert np.array_equal(data, spec_encode(secpar, "signature", spec_sign(bs.q, sk, c_hat)))
    data, codes = bs.sign_batch_encoded(sk, vk, msgs)
    assert codes.tolist() == [0] * n and np.array_equal(data, want_b)


# ---- the bound exactly -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("secpar", [128, 256])
def test_the_bound_exactly(secpar):
    """five records with +B and -B at the first value of a record, at its last value and in a chunk that two records share: all
    encode to the spec's bytes; one step further in record 2 refuses that record alone (status 4, zero bytes)"""
    _, bs = scheme(secpar)
    rows, B, w, rb = TABLE["signature"][secpar]
    d, rv = bs.d, rows * bs.d
    shared = 100                                                   # record 2 begins inside a chunk: this value lies in it
    assert (2 * rv) % 1024 and (2 * rv + shared) // 1024 == (2 * rv - 1) // 1024
    rng = np.random.default_rng(secpar)
    z = rng.integers(-B, B + 1, size=(5, rows, d), dtype=np.int64)
    flat = z.reshape(5, rv)
    for i in range(5):
        flat[i, 0], flat[i, rv - 1], flat[i, shared], flat[i, shared + 1] = B, -B, -B, B
    def inputs(zz):
        sigma = bs.ctx.ntt_forward(zz.astype(np.int32).reshape(-1, d)).reshape(zz.shape)
        return solve_keys(bs.q, sigma, 5 + secpar)
    sk, c = inputs(z)
    good = spec_pack(z, B, w)
    data, st = run_sign(bs.ctx, sk, c, B)
    assert st.tolist() == [0] * 5 and np.array_equal(data, good)
    alone, st = run_sign(bs.ctx, sk[1:2], c[1:2], B)
    assert st.tolist() == [0] and np.array_equal(alone[0], good[1])
    for pos in (0, rv - 1, shared):
        for v in (B + 1, -B - 1):
            z2 = z.copy()
            z2.reshape(5, rv)[2, pos] = v
            sk, c = inputs(z2)
            data, st = run_sign(bs.ctx, sk, c, B)
            assert st.tolist() == [0, 0, 4, 0, 0], (pos, v)
            assert not data[2].any() and np.array_equal(data[[0, 1, 3, 4]], good[[0, 1, 3, 4]]), (pos, v)
            pb, ps = run_pair(bs.ctx, sk, c, B)
            assert ps.tolist() == st.tolist() and np.array_equal(pb, data)


# ---- any int32 in, both multiply forms, every context ------------------------------------------------------------------------
@pytest.mark.parametrize("case", GE.CASES, ids=GE._cid)
def test_any_int32_operands_at_every_context(case):
    """key halves and challenges at the int32 extremes and at random, records of 1 and 3 rows: at B = the largest |z| of the
    batch everything encodes, at B - 1 exactly the records at the maximum are refused; the existing pair agrees"""
    spec, n = case
    q = X.modulus(spec)
    ctx = GE._ctx(spec, n)
    try:
        for R in (1, 3):
            vk, _ = X.key_inputs(5 * R, n, 31 + R)
            _, c = X.key_inputs(5, n, 47 + R)
            sk = np.stack([vk[:, 0].reshape(5, R, n), vk[:, 1].reshape(5, R, n)], axis=1)
            sigma = X.cent(sk[:, 0] * c[:, None, :] + sk[:, 1], q)
            assert np.array_equal(sigma, spec_sign(q, sk, c))
            z = X.inverse(spec, n, sigma)
            top = int(X.maxima(z).max())
            for B in (top, top - 1):
                if B < 1:                                          # q = 3: the largest |z| is 1, and no bound lies below it
                    continue
                want, wst = X.encoded(z, B)
                assert (wst != 0).tolist() == ((X.maxima(z) == top) & (B < top)).tolist()
                data, st = run_sign(ctx, sk, c, B)
                assert st.tolist() == wst.tolist(), (R, B)
                assert np.array_equal(data, want), (R, B)
                pb, ps = run_pair(ctx, sk, c, B)
                assert ps.tolist() == wst.tolist() and np.array_equal(pb, want), (R, B)
    finally:
        ctx.close()


# ---- the width sweep ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GE.SWEEP_CASES, ids=GE._cid)
def test_every_field_width(case):
    """every w in 2 .. 32 the modulus admits at the smallest and the largest bound of that width, 1, 2 and 5 records of 1 row (at
    degree 64 of 3 rows as well: for odd w an odd record count ends the stream 8 bytes into a 16-byte unit).  Where the tables are
    a root's the inputs are constructed from fields that include 0 and 2B and every record encodes to them; elsewhere the spec is
    the inverse transform of the same inputs, whatever it refuses."""
    spec, n = case
    q = X.modulus(spec)
    ctx = GE._ctx(spec, n)
    seen = set()
    try:
        for w, B in X.SWEEP:
            if B > X.half(spec):
                continue
            seen.add(w)
            for R in X.sweep_shapes(n):
                z = X.edge_fields(B, 5, R, n, 100 * w + R) - B
                sk, c = solve_keys(q, X.forward(spec, n, z), 7 * w + R)
                if spec[1] == "root":
                    want, wst = X.encoded(z, B)
                    assert not wst.any()
                else:
                    want, wst = X.encoded(X.inverse(spec, n, spec_sign(q, sk, c)), B)
                for sel in (slice(0, 1), slice(1, 3), slice(0, 5)):
                    N = sel.stop - sel.start
                    if n == 64 and R * w % 2 and N % 2:
                        assert (N * want.shape[1]) % 16 == 8
                    data, st = run_sign(ctx, sk[sel], c[sel], B)
                    assert st.tolist() == wst[sel].tolist(), (w, B, R, N)
                    assert np.array_equal(data, want[sel]), (w, B, R, N)
    finally:
        ctx.close()
    assert seen == set(range(2, X.width(X.half(spec)) + 1))


# ---- graph capture -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("secpar", [128, 256])
def test_graph_capture_replays_signing_and_the_keyed_verification(secpar):
    from fusion_hip import DeviceArray
    from fusion_hip.scheme import BatchScheme
    params, shared = scheme(secpar)
    rows, B, w, rb = TABLE["signature"][secpar]
    n, d = 7, shared.d
    contents = []
    for r in range(2):
        sk, vk, msgs = honest(shared, n, f"graph{r}")
        c_hat, _ = shared.challenges(vk, msgs)
        if r == 1:
            sk = sk.copy()
            sk[3, 1, 0, 0] += 12345                                # one record over the bound: status, zeroing and verdict replay too
        contents.append((sk, vk, c_hat))
    bs = BatchScheme(params, private_context=True)
    try:
        ctx = bs.ctx
        dA = DeviceArray.from_numpy(ctx, shared.A)
        dK, dVK, dC = DeviceArray(ctx, (n, 2, rows, d)), DeviceArray(ctx, (n, 2, d)), DeviceArray(ctx, (n, d))
        dB, dV, dW = DeviceArray(ctx, (n, rb), np.uint8), DeviceArray(ctx, (n,)), DeviceArray(ctx, (n,))

        def poison():
            ctx.h2d(dB.ptr, np.full((n, rb), 0xff, dtype=np.uint8))
            for dS in (dV, dW):
                ctx.h2d(dS.ptr, np.full(n, WORD_POISON, dtype=np.int32))

        def calls():
            ctx.sign_encoded_async_dev(dK.ptr, dC.ptr, n, rows, B, dB.ptr, dV.ptr)
            ctx.verify_encoded_async_dev(dA.ptr, dB.ptr, n, rows, B, 0, dVK.ptr, dC.ptr, dW.ptr)

        eager = []
        for sk, vk, c_hat in contents:
            for dst, a in ((dK, sk), (dVK, vk), (dC, c_hat)):
                ctx.h2d(dst.ptr, np.ascontiguousarray(a, dtype=np.int32))
            poison()
            calls()
            ctx.synchronize()
            eager.append((dB.numpy(), dV.numpy(), dW.numpy()))
            want_b, want_c = shared.encode("signature", shared.ctx.sign_core(sk, c_hat))
            assert np.array_equal(eager[-1][0], want_b) and np.array_equal(eager[-1][1], want_c)
        assert eager[0][1].tolist() == [0] * n and eager[0][2].tolist() == [0] * n
        assert eager[1][1].tolist() == [4 if k == 3 else 0 for k in range(n)] and not eager[1][0][3].any()
        assert eager[1][2].tolist() == [3 if k == 3 else 0 for k in range(n)]
        ctx.graph_begin()
        calls()
        g = ctx.graph_end()
        for r in (0, 1, 0):
            sk, vk, c_hat = contents[r]
            for dst, a in ((dK, sk), (dVK, vk), (dC, c_hat)):
                ctx.h2d(dst.ptr, np.ascontiguousarray(a, dtype=np.int32))
            poison()
            g.launch()
            ctx.synchronize()
            for got, want in zip((dB.numpy(), dV.numpy(), dW.numpy()), eager[r]):
                assert np.array_equal(got, want), r
        g.destroy()
        for b in (dA, dK, dVK, dC, dB, dV, dW):
            b.free()
    finally:
        bs.close()


# ---- the consumers of the bytes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("secpar", [128, 256])
def test_device_bytes_feed_verification_and_aggregation(secpar):
    from fusion_hip import DeviceArray
    _, bs = scheme(secpar)
    rows, B, w, rb = TABLE["signature"][secpar]
    n = 33
    sk, vk, msgs = honest(bs, n, "feed")
    dK = DeviceArray.from_numpy(bs.ctx, sk)
    dB, codes = bs.sign_batch_encoded(dK, vk, msgs, device=True)
    try:
        assert isinstance(dB, DeviceArray) and dB.dtype == np.uint8 and dB.shape == (n, rb)
        assert codes.dtype == np.int32 and codes.tolist() == [0] * n
        assert np.array_equal(dK.numpy(), sk)
        assert bs.verify_signatures_encoded(vk, msgs, dB).tolist() == [0] * n
        agg, codes = bs.aggregate_encoded(vk, msgs, dB)
        assert codes.tolist() == [0] * n
        assert np.array_equal(agg, bs.aggregate(vk, msgs, bs.sign_batch(sk, vk, msgs)))
        assert bs.verify(vk, msgs, agg) == (True, "")
    finally:
        dB.free()
        dK.free()


# ---- object face -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("secpar", [128, 256])
def test_object_face(secpar):
    import fusion.fusion as F
    from fusion_hip.scheme import encoded_size
    params, _ = scheme(secpar)
    for k in range(2):
        key, m = F.keygen(params, 800 + k), f"to-bytes-{secpar}-{k}"
        b = F.sign_to_bytes(params, key, m)
        assert isinstance(b, bytes) and len(b) == encoded_size(params, "signature")
        assert b == F.to_bytes(params, F.sign(params, key, m))
        ok = F.verify_signatures(params, [key[1]], [m], [F.from_bytes(params, "signature", b)])
        assert ok == [(True, "")]


# ---- refusals of the C entry -------------------------------------------------------------------------------------------------
def test_refusals_of_the_entry():
    import fusion_hip
    from fusion_hip import DeviceArray, FusionHipError
    from fusion_hip._lib import FZ_E_BADARG, FZ_E_UNSUPPORTED
    _, bs = scheme(256)
    ctx, d, q = bs.ctx, bs.d, bs.q
    l, B = 2, 5
    rb = X.record_bytes(d, l, X.width(B))
    dK = DeviceArray.from_numpy(ctx, np.zeros((2, 2, l, d) , dtype=np.int32))
    dC = DeviceArray.from_numpy(ctx, np.zeros((2, d), dtype=np.int32))
    dB = DeviceArray.from_numpy(ctx, np.full(2 * rb + 64, BYTE_POISON, dtype=np.uint8))
    dV = DeviceArray.from_numpy(ctx, np.full(16, WORD_POISON, dtype=np.int32))
    try:
        for args in ((dK.ptr, dC.ptr, 2, l, B, dB.ptr + 8, dV.ptr), (dK.ptr + 4, dC.ptr, 2, l, B, dB.ptr, dV.ptr),
                     (dK.ptr, dC.ptr + 8, 2, l, B, dB.ptr, dV.ptr), (0, dC.ptr, 2, l, B, dB.ptr, dV.ptr),
                     (dK.ptr, dC.ptr, 2, l, B, 0, dV.ptr), (dK.ptr, dC.ptr, 2, l, B, dB.ptr, 0),
                     (dK.ptr, dC.ptr, 2, l, 0, dB.ptr, dV.ptr), (dK.ptr, dC.ptr, 2, l, (q - 1) // 2 + 1, dB.ptr, dV.ptr),
                     (dK.ptr, dC.ptr, 0, l, 0, dB.ptr, dV.ptr), (dK.ptr, dC.ptr, 2, 0, B, dB.ptr, dV.ptr)):
            with pytest.raises(FusionHipError) as e:
                ctx.sign_encoded_async_dev(*args)
            assert e.value.code == FZ_E_BADARG, args
        ctx.sign_encoded_async_dev(dK.ptr, dC.ptr, 0, l, B, dB.ptr, dV.ptr)                 # N = 0: OK, nothing written
        ctx.sign_encoded_async_dev(0, 0, 0, l, (q - 1) // 2, 0, 0)
        ctx.synchronize()
        assert (dB.numpy() == BYTE_POISON).all() and (dV.numpy() == WORD_POISON).all()
        q128, root, inv_root = X.E.root_of("scheme", 128)
        other = fusion_hip.Context(q128, 128, root, inv_root)
        try:
            with pytest.raises(FusionHipError) as e:
                other.sign_encoded_async_dev(dK.ptr, dC.ptr, 2, l, B, dB.ptr, dV.ptr)
            assert e.value.code == FZ_E_UNSUPPORTED
        finally:
            other.close()
        ctx.synchronize()
        assert (dB.numpy() == BYTE_POISON).all() and (dV.numpy() == WORD_POISON).all()
    finally:
        for b in (dK, dC, dB, dV):
            b.free()
