"""Signing straight from compact secret-key records on the device (fz_sign_records_async, BatchScheme.sign_batch_records and
keygen_batch_encoded, the "secret" kind, fusion.fusion.sign_from_bytes): the reference-made golden keys and challenges, the
existing decode -> sign pair at every walk shape, the output bound exactly at the first and last value of a record and in a chunk
two records share, the key's fields exactly at the ends of either half, any int32 challenge at every multiply form and context of
tests/_encoded_edges.py, every field width on either side, graph capture with the keyed verification behind it, the flow from
seeds to a verified aggregate with nothing expanded, the object face and the refusals of the C entry.  No tolerance anywhere."""
import hashlib
import json
import os

import numpy as np
import pytest

import _encoded_edges as X
import test_gpu_encoded_edges as GE
from test_encoding_host import TABLE, spec_encode, spec_pack
from test_gpu_encoding import scheme
from test_gpu_sign_encoded import honest, run_sign
from test_sign_records_host import BETA_SK, SECRET, golden_secret_records, spec_sign_records, spec_values_from_records

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
BYTE_POISON, WORD_POISON = 0xab, 0x7f7f7f7f


def run_sign_records(ctx, key_bytes, key_bound, c_hat, l, B):
    """fz_sign_records_async on key records [N][2 l n wk / 8] and c_hat [N][n] -> (bytes [N][record bytes], status [N]); the guard
    bytes and the poisoned record area behind the stream and the status words behind the last one are untouched, the inputs
    unchanged"""
    c = np.ascontiguousarray(c_hat, dtype=np.int32)
    N, n = c.shape
    rb = X.record_bytes(n, l, X.width(B))
    key = np.ascontiguousarray(key_bytes, dtype=np.uint8).reshape(N, X.record_bytes(n, 2 * l, X.width(key_bound)))
    bufs = GE.Bufs(ctx)
    try:
        dK, dC = bufs.put(key), bufs.put(c)
        dB = bufs.put(np.full(N * rb + rb + GE.GUARD, BYTE_POISON, dtype=np.uint8))
        dV = bufs.put(np.full(N + 16, WORD_POISON, dtype=np.int32))
        ctx.sign_records_async_dev(dK.ptr, key_bound, dC.ptr, N, l, B, dB.ptr, dV.ptr)
        got, st = dB.numpy(), dV.numpy()
        assert (got[N * rb:] == BYTE_POISON).all() and (st[N:] == WORD_POISON).all()
        assert np.array_equal(dK.numpy(), key) and np.array_equal(dC.numpy(), c)
        return got[:N * rb].reshape(N, rb), st[:N]
    finally:
        bufs.free()


def run_pair(ctx, key_bytes, key_bound, c_hat, l, B):
    """the two existing entries: fz_decode_records_async(rows = 2 l, coef = 1, key_bound), then fz_sign_encoded_async on its rows
    -> (bytes, status of the signing, status of the decoding)"""
    c = np.ascontiguousarray(c_hat, dtype=np.int32)
    N, n = c.shape
    key = np.ascontiguousarray(key_bytes, dtype=np.uint8).reshape(N, -1)
    rows, dst = GE.run_decode(ctx, key, 2 * l, n, True, key_bound)
    data, st = run_sign(ctx, rows.reshape(N, 2, l, n), c, B)
    return data, st, dst


def pack_fields(u, w):
    """fields [N][..] in [0, 2^w) -> [N][bytes]: the format, whatever the fields hold"""
    u = np.asarray(u, dtype=np.int64).reshape(u.shape[0], -1)
    bits = ((u[..., None] >> np.arange(w, dtype=np.int64)) & 1).astype(np.uint8)
    return np.packbits(bits.reshape(u.shape[0], -1), axis=1, bitorder="little")


def any_int32(shape, seed):
    return np.random.default_rng(seed).integers(I32_MIN, I32_MAX + 1, size=shape, dtype=np.int64)


# ---- golden ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("secpar", [128, 256])
def test_golden_keys_give_the_spec_bytes_and_the_digests(secpar):
    _, bs = scheme(secpar)
    S = np.load(os.path.join(G, f"scheme_{secpar}.npz"))
    with open(os.path.join(G, "scheme.json")) as fh:
        msgs = json.load(fh)[str(secpar)]["messages"]
    with open(os.path.join(G, "encoding.json")) as fh:
        digest = json.load(fh)[str(secpar)]["sig"]
    with open(os.path.join(G, "secret_encoding.json")) as fh:
        key_digest = json.load(fh)[str(secpar)]["sk"]
    _, B, w, rb = TABLE["signature"][secpar]
    krows, KB, wk, kb = SECRET[secpar]
    recs = golden_secret_records(secpar)
    want = spec_encode(secpar, "signature", S["sig"])
    data, st = run_sign_records(bs.ctx, recs, KB, S["c_hat"], bs.l, B)
    assert st.tolist() == [0] * 4 and np.array_equal(data, want)
    assert hashlib.sha3_256(data.tobytes()).hexdigest() == digest
    assert np.array_equal(data, spec_sign_records(secpar, recs, KB, S["c_hat"], bs.l, B)[0])
    data, codes = bs.sign_batch_records(recs, S["vk"], msgs)
    assert data.dtype == np.uint8 and data.shape == (4, rb) and codes.dtype == np.int32 and codes.tolist() == [0] * 4
    assert np.array_equal(data, want) and hashlib.sha3_256(data.tobytes()).hexdigest() == digest
    for sk in (S["sk_hat"], S["sk_hat"].reshape(4, krows, bs.d)):
        enc, codes = bs.encode("secret", sk)
        assert enc.shape == (4, kb) and codes.tolist() == [0] * 4 and np.array_equal(enc, recs)
        assert hashlib.sha3_256(enc.tobytes()).hexdigest() == key_digest
    back, codes = bs.decode("secret", recs)
    assert back.shape == (4, 2, bs.l, bs.d) and codes.tolist() == [0] * 4 and np.array_equal(back, S["sk_hat"])


# ---- the existing pair at every walk shape -----------------------------------------------------------------------------------
@pytest.mark.parametrize("secpar", [128, 256])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 33, 67, 512])
def test_equals_decode_then_sign(secpar, n):
    """fewer tasks than waves, record boundaries inside chunks (a record is 12.1875 / 20.75 chunks), an uneven tail, and at 512
    more wave-tasks than any resident grid"""
    _, bs = scheme(secpar)
    _, B, w, rb = TABLE["signature"][secpar]
    KB = SECRET[secpar][1]
    sk, vk, msgs = honest(bs, n, "records")
    recs, codes = bs.encode("secret", sk)
    assert codes.tolist() == [0] * n
    c_hat, _ = bs.challenges(vk, msgs)
    data, st = run_sign_records(bs.ctx, recs, KB, c_hat, bs.l, B)
    assert st.tolist() == [0] * n
    rows, codes = bs.decode("secret", recs)
    assert codes.tolist() == [0] * n and np.array_equal(rows, sk)
    want_b, want_c = bs.sign_batch_encoded(rows, vk, msgs)
    assert want_c.tolist() == [0] * n and np.array_equal(data, want_b)
    assert np.array_equal(data, bs.encode("signature", bs.sign_batch(sk, vk, msgs))[0])
    if n <= 5:
        sb, ss = spec_sign_records(secpar, recs, KB, c_hat, bs.l, B)
        assert ss.tolist() == [0] * n and np.array_equal(data, sb)
    for form in (recs, recs.tobytes(), bytearray(recs.tobytes()), memoryview(recs.tobytes())) if n == 3 else (recs,):
        data, codes = bs.sign_batch_records(form, vk, msgs)
        assert codes.tolist() == [0] * n and np.array_equal(data, want_b)


# ---- the output bound exactly ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("secpar", [128, 256])
def test_the_output_bound_exactly(secpar):
    """five records of five rows with +B and -B at the first value of a record, at its last value and in a chunk that two records
    share, the right half carrying the target (key bound (q - 1) / 2): all encode to the spec's bytes; one step further in record
    2 refuses that record alone (status 4, zero bytes); the existing pair agrees"""
    _, bs = scheme(secpar)
    _, B, w, _ = TABLE["signature"][secpar]
    spec, d, l, q = (secpar, "params"), bs.d, 5, bs.q
    KB = (q - 1) // 2
    wk = X.width(KB)
    rv, shared = l * d, 100
    assert (2 * rv) % 1024 and (2 * rv + shared) // 1024 == (2 * rv - 1) // 1024
    rng = np.random.default_rng(secpar)
    z = rng.integers(-B, B + 1, size=(5, l, d), dtype=np.int64)
    flat = z.reshape(5, rv)
    for i in range(5):
        flat[i, 0], flat[i, rv - 1], flat[i, shared], flat[i, shared + 1] = B, -B, -B, B
    sL = rng.integers(-KB, KB + 1, size=(5, l, d), dtype=np.int64)
    c = any_int32((5, d), secpar + 1)
    t = X.inverse(spec, d, X.cent(X.forward(spec, d, sL) * c[:, None, :], q))

    def records(zz):
        return pack_fields(np.stack([sL, X.cent(zz - t, q)], axis=1) + KB, wk)
    good = spec_pack(z, B, w)
    data, st = run_sign_records(bs.ctx, records(z), KB, c, l, B)
    assert st.tolist() == [0] * 5 and np.array_equal(data, good)
    alone, st = run_sign_records(bs.ctx, records(z)[1:2], KB, c[1:2], l, B)
    assert st.tolist() == [0] and np.array_equal(alone[0], good[1])
    for pos in (0, rv - 1, shared):
        for v in (B + 1, -B - 1):
            z2 = z.copy()
            z2.reshape(5, rv)[2, pos] = v
            data, st = run_sign_records(bs.ctx, records(z2), KB, c, l, B)
            assert st.tolist() == [0, 0, 4, 0, 0], (pos, v)
            assert not data[2].any() and np.array_equal(data[[0, 1, 3, 4]], good[[0, 1, 3, 4]]), (pos, v)
            pb, ps, pd = run_pair(bs.ctx, records(z2), KB, c, l, B)
            assert pd.tolist() == [0] * 5 and ps.tolist() == st.tolist() and np.array_equal(pb, data)


# ---- the key's fields exactly --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("secpar", [128, 256])
def test_the_key_fields_exactly(secpar):
    """a field of 2 key_bound at the first and last field of either half and in a chunk two records share: all sign to the spec's
    bytes.  2 key_bound + 1 at each of those places gives status 6 for that record alone, with zero bytes; beside a record over
    the output bound the statuses are 6 and 4; a record with both faults reports 6."""
    _, bs = scheme(secpar)
    spec, d, l, q = (secpar, "params"), bs.d, 5, bs.q
    KB, wk = BETA_SK, 7
    rv, shared = l * d, 100
    u = np.random.default_rng(secpar + 7).integers(0, 2 * KB + 1, size=(5, 2 * rv), dtype=np.int64)
    places = (0, rv - 1, rv, 2 * rv - 1, shared, rv + shared)
    for i in range(5):
        for pos in places:
            u[i, pos] = 2 * KB
    c = any_int32((5, d), secpar + 2)
    recs = pack_fields(u, wk)
    z, bad = spec_values_from_records(spec, recs, KB, c, l)
    assert not bad.any()
    M = X.maxima(z)
    order = np.argsort(M)
    top, B = int(order[-1]), int(M[order[-2]])                     # at this bound exactly the record with the largest |z| is over
    assert M[top] > B >= 1
    free = (q - 1) // 2                                            # ... and at this one none is
    good, st = run_sign_records(bs.ctx, recs, KB, c, l, free)
    assert st.tolist() == [0] * 5 and np.array_equal(good, spec_pack(z, free, X.width(free)))
    pb, ps, pd = run_pair(bs.ctx, recs, KB, c, l, free)
    assert pd.tolist() == ps.tolist() == [0] * 5 and np.array_equal(pb, good)
    tight, want_st = spec_sign_records(spec, recs, KB, c, l, B)
    assert want_st.tolist() == [4 if i == top else 0 for i in range(5)]
    other = (top + 2) % 5
    for pos in places:
        for rec, bound, want in ((2, free, [6 if i == 2 else 0 for i in range(5)]),
                                 (other, B, [6 if i == other else 4 if i == top else 0 for i in range(5)]),
                                 (top, B, [6 if i == top else 0 for i in range(5)])):
            r2 = recs.copy()
            r2[rec] = X.set_field(r2[rec], pos, 2 * KB + 1, wk)
            data, st = run_sign_records(bs.ctx, r2, KB, c, l, bound)
            assert st.tolist() == want, (pos, rec)
            ref = good if bound == free else tight
            keep = [i for i in range(5) if want[i] == 0]
            assert not data[[i for i in range(5) if want[i]]].any() and np.array_equal(data[keep], ref[keep]), (pos, rec)
            sb, ss = spec_sign_records(spec, r2, KB, c, l, bound)
            assert ss.tolist() == want and np.array_equal(sb, data)


# ---- any int32 challenge, both multiply forms, every context -----------------------------------------------------------------
@pytest.mark.parametrize("case", GE.CASES, ids=GE._cid)
def test_any_int32_challenge_at_every_context(case):
    """challenges at the int32 extremes and at random, key fields over all of [0, 2 key_bound], records of 1 and 3 rows per half:
    at B = the largest |z| of the batch everything encodes, at B - 1 exactly the records at the maximum are refused; where the
    tables are a root's the existing pair agrees"""
    spec, n = case
    KB = min(BETA_SK, X.half(spec))
    wk = X.width(KB)
    ctx = GE._ctx(spec, n)
    try:
        for R in (1, 3):
            _, c = X.key_inputs(5, n, 47 + R)
            recs = pack_fields(X.edge_fields(KB, 5, 2 * R, n, 31 + R), wk)
            z, bad = spec_values_from_records(spec, recs, KB, c, R)
            assert not bad.any()
            top = int(X.maxima(z).max())
            for B in (top, top - 1):
                if B < 1:                                          # q = 3: the largest |z| is 1, and no bound lies below it
                    continue
                want, wst = X.encoded(z, B)
                assert (wst != 0).tolist() == ((X.maxima(z) == top) & (B < top)).tolist()
                data, st = run_sign_records(ctx, recs, KB, c, R, B)
                assert st.tolist() == wst.tolist(), (R, B)
                assert np.array_equal(data, want), (R, B)
                if spec[1] == "root":
                    pb, ps, pd = run_pair(ctx, recs, KB, c, R, B)
                    assert not pd.any() and ps.tolist() == wst.tolist() and np.array_equal(pb, want), (R, B)
    finally:
        ctx.close()


# ---- the width sweeps --------------------------------------------------------------------------------------------------------
SELECTIONS = (slice(0, 1), slice(1, 3), slice(0, 5))


@pytest.mark.parametrize("case", GE.SWEEP_CASES, ids=GE._cid)
def test_every_key_field_width(case):
    """every wk in 2 .. 32 the modulus admits at the smallest and the largest key bound of that width, fields that include 0 and
    2 key_bound at the ends of the record, the output bound fixed at (q - 1) / 2 (nothing is over it); 1, 2 and 5 records of 1 row
    per half, at degree 64 of 3 rows as well (an odd record count then ends the output stream 8 bytes into a 16-byte unit)"""
    spec, n = case
    B = X.half(spec)
    ctx = GE._ctx(spec, n)
    seen = set()
    try:
        for wk, KB in X.SWEEP:
            if KB > X.half(spec):
                continue
            seen.add(wk)
            for R in X.sweep_shapes(n):
                recs = pack_fields(X.edge_fields(KB, 5, 2 * R, n, 100 * wk + R), wk)
                c = any_int32((5, n), 7 * wk + R)
                want, wst = spec_sign_records(spec, recs, KB, c, R, B)
                assert not wst.any()
                for sel in SELECTIONS:
                    N = sel.stop - sel.start
                    if n == 64 and R * X.width(B) % 2 and N % 2:
                        assert (N * want.shape[1]) % 16 == 8
                    data, st = run_sign_records(ctx, recs[sel], KB, c[sel], R, B)
                    assert st.tolist() == [0] * N, (wk, KB, R, N)
                    assert np.array_equal(data, want[sel]), (wk, KB, R, N)
    finally:
        ctx.close()
    assert seen == set(range(2, X.width(X.half(spec)) + 1))


@pytest.mark.parametrize("case", GE.SWEEP_CASES, ids=GE._cid)
def test_every_output_field_width(case):
    """every w in 2 .. 32 the modulus admits at the smallest and the largest bound of that width, key_bound = 52.  The left half
    is the constant 1 in every row (its transform is all ones), so the challenge carries the target: where the tables are a
    root's, z = INV(c) + sR is constructed from fields that include 0 and 2B and every record encodes to them; elsewhere the spec
    is the formula on the same inputs, whatever it refuses."""
    spec, n = case
    q, KB, wk = X.modulus(spec), BETA_SK, 7
    ctx = GE._ctx(spec, n)
    seen = set()
    try:
        for w, B in X.SWEEP:
            if B > X.half(spec):
                continue
            seen.add(w)
            for R in X.sweep_shapes(n):
                rng = np.random.default_rng(100 * w + R)
                z1 = X.edge_fields(B, 5, 1, n, 100 * w + R) - B                    # [5][1][n]: every row of a record holds it
                sR1 = rng.integers(-KB, KB + 1, size=(5, 1, n), dtype=np.int64)
                c = X.forward(spec, n, X.cent(z1 - sR1, q)[:, 0])
                sL = np.zeros((5, R, n), dtype=np.int64)
                sL[:, :, 0] = 1
                recs = pack_fields(np.stack([sL, np.repeat(sR1, R, axis=1)], axis=1) + KB, wk)
                want, wst = spec_sign_records(spec, recs, KB, c, R, B)
                if spec[1] == "root":
                    assert not wst.any() and np.array_equal(want, spec_pack(np.repeat(z1, R, axis=1), B, w))
                for sel in SELECTIONS:
                    N = sel.stop - sel.start
                    if n == 64 and R * w % 2 and N % 2:
                        assert (N * want.shape[1]) % 16 == 8
                    data, st = run_sign_records(ctx, recs[sel], KB, c[sel], R, B)
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
    _, KB, wk, kb = SECRET[secpar]
    n, d = 7, shared.d
    contents = []
    for r in range(2):
        sk, vk, msgs = honest(shared, n, f"rgraph{r}")
        c_hat, _ = shared.challenges(vk, msgs)
        recs, codes = shared.encode("secret", sk)
        assert not codes.any()
        want = shared.encode("signature", shared.ctx.sign_core(sk, c_hat))[0]
        if r == 1:                                                 # a non-canonical key record: status, zeroing and verdict replay too
            recs[3] = X.set_field(recs[3], rows * d + 17, 2 * KB + 1, wk)
            want[3] = 0
        contents.append((recs, vk, c_hat, want))
    bs = BatchScheme(params, private_context=True)
    try:
        ctx = bs.ctx
        dA = DeviceArray.from_numpy(ctx, shared.A)
        dK, dVK, dC = DeviceArray(ctx, (n, kb), np.uint8), DeviceArray(ctx, (n, 2, d)), DeviceArray(ctx, (n, d))
        dB, dV, dW = DeviceArray(ctx, (n, rb), np.uint8), DeviceArray(ctx, (n,)), DeviceArray(ctx, (n,))

        def load(r):
            recs, vk, c_hat, _ = contents[r]
            ctx.h2d(dK.ptr, recs)
            for dst, a in ((dVK, vk), (dC, c_hat)):
                ctx.h2d(dst.ptr, np.ascontiguousarray(a, dtype=np.int32))
            ctx.h2d(dB.ptr, np.full((n, rb), 0xff, dtype=np.uint8))
            for dS in (dV, dW):
                ctx.h2d(dS.ptr, np.full(n, WORD_POISON, dtype=np.int32))

        def calls():
            ctx.sign_records_async_dev(dK.ptr, KB, dC.ptr, n, rows, B, dB.ptr, dV.ptr)
            ctx.verify_encoded_async_dev(dA.ptr, dB.ptr, n, rows, B, 0, dVK.ptr, dC.ptr, dW.ptr)

        eager = []
        for r in range(2):
            load(r)
            calls()
            ctx.synchronize()
            eager.append((dB.numpy(), dV.numpy(), dW.numpy()))
            assert np.array_equal(eager[-1][0], contents[r][3])
        assert eager[0][1].tolist() == [0] * n and eager[0][2].tolist() == [0] * n
        assert eager[1][1].tolist() == [6 if k == 3 else 0 for k in range(n)]
        assert eager[1][2].tolist() == [3 if k == 3 else 0 for k in range(n)]      # zero bytes are a canonical record: the wrong one
        ctx.graph_begin()
        calls()
        g = ctx.graph_end()
        for r in (0, 1, 0):
            load(r)
            g.launch()
            ctx.synchronize()
            for got, want in zip((dB.numpy(), dV.numpy(), dW.numpy()), eager[r]):
                assert np.array_equal(got, want), r
        g.destroy()
        for b in (dA, dK, dVK, dC, dB, dV, dW):
            b.free()
    finally:
        bs.close()


# ---- from seeds to a verified aggregate, nothing expanded --------------------------------------------------------------------
@pytest.mark.parametrize("secpar", [128, 256])
def test_the_flow_with_nothing_expanded(secpar):
    from fusion_hip import DeviceArray
    _, bs = scheme(secpar)
    _, B, w, rb = TABLE["signature"][secpar]
    kb = SECRET[secpar][3]
    n = 33
    seeds = [700 + 11 * k for k in range(n)]
    msgs = [f"flow-{secpar}-{k}" for k in range(n)]
    sk, vk = bs.keygen_batch(seeds)
    want_recs, codes = bs.encode("secret", sk)
    assert codes.tolist() == [0] * n
    recs, vk2 = bs.keygen_batch_encoded(seeds)
    assert isinstance(recs, np.ndarray) and recs.dtype == np.uint8 and recs.shape == (n, kb)
    assert np.array_equal(recs, want_recs) and np.array_equal(vk2, vk)
    for some in (np.array(seeds[:3]), np.array(seeds[:3], dtype=np.uint64), tuple(seeds[:3]), [np.int64(s) for s in seeds[:3]]):
        recs3, vk3 = bs.keygen_batch_encoded(some)
        assert np.array_equal(recs3, want_recs[:3]) and np.array_equal(vk3, vk[:3])
    odd = [-5, 2 ** 70]                                            # seeds only the Python sampler takes
    recs2, vk2 = bs.keygen_batch_encoded(odd)
    sk2, want_vk2 = bs.keygen_batch(odd)
    assert np.array_equal(recs2, bs.encode("secret", sk2)[0]) and np.array_equal(vk2, want_vk2)
    dK, vk3 = bs.keygen_batch_encoded(seeds, device=True)
    dB = None
    try:
        assert isinstance(dK, DeviceArray) and dK.dtype == np.uint8 and dK.shape == (n, kb)
        assert np.array_equal(dK.numpy(), want_recs) and np.array_equal(vk3, vk)
        dB, codes = bs.sign_batch_records(dK, vk, msgs, device=True)
        assert isinstance(dB, DeviceArray) and dB.dtype == np.uint8 and dB.shape == (n, rb)
        assert codes.dtype == np.int32 and codes.tolist() == [0] * n
        assert np.array_equal(dK.numpy(), want_recs)
        assert np.array_equal(dB.numpy(), bs.sign_batch_encoded(sk, vk, msgs)[0])
        assert bs.verify_signatures_encoded(vk, msgs, dB).tolist() == [0] * n
        agg, codes = bs.aggregate_encoded(vk, msgs, dB)
        assert codes.tolist() == [0] * n
        assert np.array_equal(agg, bs.aggregate(vk, msgs, bs.sign_batch(sk, vk, msgs)))
        assert bs.verify(vk, msgs, agg) == (True, "")
    finally:
        dK.free()
        if dB is not None:
            dB.free()
    # a non-canonical record among honest ones: code 6 and zero bytes for it alone
    bad = want_recs.copy()
    bad[5] = X.set_field(bad[5], 3, 2 * BETA_SK + 1, 7)
    data, codes = bs.sign_batch_records(bad, vk, msgs)
    assert codes.tolist() == [6 if k == 5 else 0 for k in range(n)] and not data[5].any()
    keep = [k for k in range(n) if k != 5]
    assert np.array_equal(data[keep], bs.sign_batch_encoded(sk, vk, msgs)[0][keep])
    rows, codes = bs.decode("secret", bad)
    assert codes.tolist() == [6 if k == 5 else 0 for k in range(n)] and not rows[5].any()
    over = sk[:2].copy()
    over[1, 1, 2, 9] += 12345                                      # a key keygen cannot make: |s| > beta_sk
    assert bs.encode("secret", over)[1].tolist() == [0, 4]


# ---- object face -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("secpar", [128, 256])
def test_object_face_round_trip(secpar):
    import fusion.fusion as F
    from fusion_hip.scheme import encoded_size
    params, _ = scheme(secpar)
    q = params.modulus
    for k in range(2):
        key, m = F.keygen(params, 900 + k), f"from-bytes-{secpar}-{k}"
        b = F.to_bytes(params, key[0])
        assert isinstance(b, bytes) and len(b) == encoded_size(params, "secret")
        back = F.from_bytes(params, "secret", b)
        assert isinstance(back, F.OneTimeSigningKey) and back.seed is None
        assert np.array_equal(F._rows_of(back.left_sk_hat, q), F._rows_of(key[0].left_sk_hat, q))
        assert np.array_equal(F._rows_of(back.right_sk_hat, q), F._rows_of(key[0].right_sk_hat, q))
        s = F.sign_from_bytes(params, b, key[1], m)
        assert isinstance(s, bytes) and s == F.sign_to_bytes(params, key, m) == F.sign_to_bytes(params, (back, key[1]), m)
    with pytest.raises(ValueError):
        F.sign_from_bytes(params, b[:-1], key[1], m)
    bad = X.set_field(np.frombuffer(b, dtype=np.uint8), 0, 2 * BETA_SK + 1, 7).tobytes()
    from fusion_hip import ENCODING_REASONS
    for call in (lambda: F.sign_from_bytes(params, bad, key[1], m), lambda: F.from_bytes(params, "secret", bad)):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == ENCODING_REASONS[6]


# ---- refusals of the C entry -------------------------------------------------------------------------------------------------
def test_refusals_of_the_entry():
    import fusion_hip
    from fusion_hip import DeviceArray, FusionHipError
    from fusion_hip._lib import FZ_E_BADARG, FZ_E_UNSUPPORTED
    _, bs = scheme(256)
    ctx, d, q = bs.ctx, bs.d, bs.q
    l, B, KB = 2, 5, 52
    rb, kb = X.record_bytes(d, l, X.width(B)), X.record_bytes(d, 2 * l, X.width(KB))
    top = (q - 1) // 2
    dK = DeviceArray.from_numpy(ctx, np.zeros(2 * kb + 64, dtype=np.uint8))
    dC = DeviceArray.from_numpy(ctx, np.zeros((2, d), dtype=np.int32))
    dB = DeviceArray.from_numpy(ctx, np.full(2 * rb + 64, BYTE_POISON, dtype=np.uint8))
    dV = DeviceArray.from_numpy(ctx, np.full(16, WORD_POISON, dtype=np.int32))
    try:
        for args in ((dK.ptr, KB, dC.ptr, 2, l, B, dB.ptr + 8, dV.ptr), (dK.ptr + 4, KB, dC.ptr, 2, l, B, dB.ptr, dV.ptr),
                     (dK.ptr + 2, KB, dC.ptr, 2, l, B, dB.ptr, dV.ptr), (dK.ptr, KB, dC.ptr + 8, 2, l, B, dB.ptr, dV.ptr),
                     (dK.ptr, KB, dC.ptr, 2, l, B, dB.ptr, dV.ptr + 4),
                     (0, KB, dC.ptr, 2, l, B, dB.ptr, dV.ptr), (dK.ptr, KB, 0, 2, l, B, dB.ptr, dV.ptr),
                     (dK.ptr, KB, dC.ptr, 2, l, B, 0, dV.ptr), (dK.ptr, KB, dC.ptr, 2, l, B, dB.ptr, 0),
                     (dK.ptr, KB, dC.ptr, 2, l, 0, dB.ptr, dV.ptr), (dK.ptr, KB, dC.ptr, 2, l, top + 1, dB.ptr, dV.ptr),
                     (dK.ptr, 0, dC.ptr, 2, l, B, dB.ptr, dV.ptr), (dK.ptr, top + 1, dC.ptr, 2, l, B, dB.ptr, dV.ptr),
                     (dK.ptr, -1, dC.ptr, 2, l, B, dB.ptr, dV.ptr),
                     (dK.ptr, KB, dC.ptr, 0, l, 0, dB.ptr, dV.ptr), (dK.ptr, 0, dC.ptr, 0, l, B, dB.ptr, dV.ptr),
                     (dK.ptr, KB, dC.ptr, 2, 0, B, dB.ptr, dV.ptr), (dK.ptr, KB, dC.ptr, 0, 0, B, dB.ptr, dV.ptr)):
            with pytest.raises(FusionHipError) as e:
                ctx.sign_records_async_dev(*args)
            assert e.value.code == FZ_E_BADARG, args
        ctx.sign_records_async_dev(dK.ptr, KB, dC.ptr, 0, l, B, dB.ptr, dV.ptr)             # N = 0: OK, nothing written
        ctx.sign_records_async_dev(0, top, 0, 0, l, top, 0, 0)
        ctx.synchronize()
        assert (dB.numpy() == BYTE_POISON).all() and (dV.numpy() == WORD_POISON).all()
        q128, root, inv_root = X.E.root_of("scheme", 128)
        other = fusion_hip.Context(q128, 128, root, inv_root)
        try:
            with pytest.raises(FusionHipError) as e:                                        # a bad bound comes before the degree
                other.sign_records_async_dev(dK.ptr, KB, dC.ptr, 2, l, 0, dB.ptr, dV.ptr)
            assert e.value.code == FZ_E_BADARG
            with pytest.raises(FusionHipError) as e:                                        # ... and so do the pointers
                other.sign_records_async_dev(dK.ptr, KB, dC.ptr, 2, l, B, dB.ptr + 8, dV.ptr)
            assert e.value.code == FZ_E_BADARG
            other.sign_records_async_dev(dK.ptr, KB, dC.ptr, 0, l, B, dB.ptr, dV.ptr)       # N = 0 before the degree as well
            with pytest.raises(FusionHipError) as e:
                other.sign_records_async_dev(dK.ptr, KB, dC.ptr, 2, l, B, dB.ptr, dV.ptr)
            assert e.value.code == FZ_E_UNSUPPORTED
        finally:
            other.close()
        ctx.synchronize()
        assert (dB.numpy() == BYTE_POISON).all() and (dV.numpy() == WORD_POISON).all()
        assert not dK.numpy().any()
    finally:
        for b in (dK, dC, dB, dV):
            b.free()
