"""Key generation straight to compact secret-key records on the device (fz_keygen_records_async, Context.keygen_records,
BatchScheme.keygen_batch_encoded, fusion.fusion.keygen_to_bytes): the reference-made golden keys, the existing pair
fz_keygen_core[_bcast] + fz_encode_records_async and the CPU spec of tests/test_keygen_records_host.py in both forms at every walk
shape, every field width, the bound exactly at the ends of either half, any int32 coefficient, every multiply form and context of
tests/_encoded_edges.py, graph capture, the refusals of the C entry, the flow from seeds to a verified aggregate with nothing
expanded and the object face.  Every call runs with guards behind its three outputs.  No tolerance anywhere."""
import hashlib
import json
import os
import random

import numpy as np
import pytest

import _encoded_edges as X
import test_gpu_encoded_edges as GE
from test_encoding_host import TABLE, spec_pack
from test_gpu_encoding import scheme
from test_keygen_records_host import spec_keygen_records
from test_sign_records_host import BETA_SK, SECRET, golden_secret_records

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
BYTE_POISON, WORD_POISON = 0xab, 0x7f7f7f7f


def run_keygen_records(ctx, A, coef, coef_rows, l, KB):
    """fz_keygen_records_async on A [l][n] and coef [N][2][n] (coef_rows = 1) or [N][2][l][n] (coef_rows = l) -> (bytes [N][record
    bytes], status [N], vk [N][2][n]); a poisoned record and guard bytes behind the last record, a poisoned key behind d_vk[N - 1]
    and poisoned words behind d_status[N - 1] are untouched, the inputs unchanged"""
    A = np.ascontiguousarray(A, dtype=np.int32)
    c = np.ascontiguousarray(coef, dtype=np.int32)
    N, n = c.shape[0], c.shape[-1]
    assert A.shape == (l, n) and c.shape == ((N, 2, n) if coef_rows == 1 else (N, 2, l, n))
    rb = X.record_bytes(n, 2 * l, X.width(KB))
    bufs = GE.Bufs(ctx)
    try:
        dA, dC = bufs.put(A), bufs.put(c)
        dB = bufs.put(np.full(N * rb + rb + GE.GUARD, BYTE_POISON, dtype=np.uint8))
        dK = bufs.put(np.full((N + 1, 2, n), WORD_POISON, dtype=np.int32))
        dV = bufs.put(np.full(N + 16, WORD_POISON, dtype=np.int32))
        ctx.keygen_records_async_dev(dA.ptr, dC.ptr, coef_rows, N, l, KB, dB.ptr, dK.ptr, dV.ptr)
        got, vk, st = dB.numpy(), dK.numpy(), dV.numpy()
        assert (got[N * rb:] == BYTE_POISON).all() and (vk[N:] == WORD_POISON).all() and (st[N:] == WORD_POISON).all()
        assert np.array_equal(dA.numpy(), A) and np.array_equal(dC.numpy(), c)
        return got[:N * rb].reshape(N, rb), st[:N], vk[:N]
    finally:
        bufs.free()


def run_pair(ctx, A, coef, coef_rows, l, KB):
    """the two existing entries: fz_keygen_core (coef_rows = l) or fz_keygen_core_bcast (coef_rows = 1), then
    fz_encode_records_async(rows = 2 l, coef = 1, KB) on its key -> (bytes, status, vk)"""
    A = np.ascontiguousarray(A, dtype=np.int32)
    c = np.ascontiguousarray(coef, dtype=np.int32)
    N, n = c.shape[0], c.shape[-1]
    bufs = GE.Bufs(ctx)
    try:
        dA, dC = bufs.put(A), bufs.put(c)
        dS, dK = bufs.put(np.zeros((N, 2, l, n), dtype=np.int32)), bufs.put(np.zeros((N, 2, n), dtype=np.int32))
        (ctx.keygen_core_bcast_dev if coef_rows == 1 else ctx.keygen_core_dev)(dA.ptr, dC.ptr, dS.ptr, dK.ptr, N, l)
        sk, vk = dS.numpy(), dK.numpy()
    finally:
        bufs.free()
    data, st = GE.run_encode(ctx, sk.reshape(N, 2 * l, n), True, KB)
    return data, st, vk


def any_int32(shape, seed):
    return np.random.default_rng(seed).integers(I32_MIN, I32_MAX + 1, size=shape, dtype=np.int64)


def coefficients(N, l, n, coef_rows, KB, seed):
    return np.random.default_rng(seed).integers(-KB, KB + 1, size=(N, 2, n) if coef_rows == 1 else (N, 2, l, n), dtype=np.int64)


def check_against_spec(spec, A, coef, coef_rows, l, KB, got, keys=None):
    """the entry's (bytes, status, vk) against the spec; keys: the spec's transforms for these keys only (the fields of all)"""
    data, st, vk = got
    N = coef.shape[0]
    idx = np.arange(N) if keys is None else np.array(sorted(set(keys)))
    wb, ws, wv = spec_keygen_records(spec, A, coef[idx], coef_rows, l, KB)
    assert st[idx].tolist() == ws.tolist()
    assert np.array_equal(data[idx], wb) and np.array_equal(vk[idx], wv)
    if keys is not None and (N <= 64 or (l == 1 and N <= 4096)):                     # the records of every key: no transform needed
        q = X.modulus(spec if isinstance(spec, tuple) else (spec, "params"))
        s = X.cent(np.asarray(coef, dtype=np.int64), q)
        over = np.abs(s).reshape(N, -1).max(axis=1) > KB
        assert st.tolist() == np.where(over, 4, 0).tolist()
        full = np.broadcast_to(s.reshape(N, 2, 1, -1), (N, 2, l, s.shape[-1])) if coef_rows == 1 else s
        ok = np.flatnonzero(~over)
        assert np.array_equal(data[ok], spec_pack(full[ok].reshape(len(ok), 2 * l, -1), KB, X.width(KB)))
        assert not data[over].any()


# ---- golden ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("secpar", [128, 256])
def test_golden_seeds_give_the_golden_records_and_keys(secpar):
    from fusion_hip import hostpipe
    params, bs = scheme(secpar)
    S = np.load(os.path.join(G, f"scheme_{secpar}.npz"))
    with open(os.path.join(G, "scheme.json")) as fh:
        seeds = json.load(fh)[str(secpar)]["key_seeds"]
    with open(os.path.join(G, "secret_encoding.json")) as fh:
        digest = json.load(fh)[str(secpar)]["sk"]
    _, KB, wk, kb = SECRET[secpar]
    want = golden_secret_records(secpar)
    recs, vk = bs.keygen_batch_encoded(seeds)
    assert recs.dtype == np.uint8 and recs.shape == (len(seeds), kb) and vk.dtype == np.int32
    assert hashlib.sha3_256(recs.tobytes()).hexdigest() == digest and np.array_equal(recs, want)
    assert np.array_equal(vk, S["vk"])
    polys = hostpipe.sample_secret_polys(np.array(seeds, dtype=np.uint64), bs.q, bs.d, params.beta_sk, params.omega_sk)
    data, st, vk = run_keygen_records(bs.ctx, S["A"], polys, 1, bs.l, KB)
    assert st.tolist() == [0] * len(seeds) and np.array_equal(data, want) and np.array_equal(vk, S["vk"])
    assert hashlib.sha3_256(data.tobytes()).hexdigest() == digest
    data, st, vk = run_keygen_records(bs.ctx, S["A"], S["coef"], bs.l, bs.l, KB)       # the reference's own matrices, all l rows
    assert st.tolist() == [0] * len(seeds) and np.array_equal(data, want) and np.array_equal(vk, S["vk"])
    data, vk, codes = bs.ctx.keygen_records(S["A"], polys, KB)
    assert codes.tolist() == [0] * len(seeds) and np.array_equal(data, want) and np.array_equal(vk, S["vk"])


# ---- the existing pair and the spec at every walk shape, both forms ----------------------------------------------------------
@pytest.mark.parametrize("secpar", [128, 256])
@pytest.mark.parametrize("form", ["one", "rows"])
@pytest.mark.parametrize("shape", ["own", 1, 2, 3, 5])
def test_equals_keygen_then_encode_and_the_spec(secpar, form, shape):
    """the scheme's own l with 1, 2, 3, 5 and 33 keys (fewer units than waves, a ragged last task at degree 64), and l = 1, 2, 3, 5
    with 1, 7 and 4096 keys: at l = 1 that is more (key, half) units than any resident grid at degree 256, where a workgroup's
    round is 4 units; at degree 64 it is 16, and 16384 keys are"""
    _, bs = scheme(secpar)
    KB, n = BETA_SK, bs.d
    l = bs.l if shape == "own" else shape
    for N in ((1, 2, 3, 5, 33) if shape == "own" else (1, 7, 4096) + ((16384,) if l == 1 and n == 64 else ())):
        rows = 1 if form == "one" else l
        A = any_int32((l, n), 1000 * l + N)
        coef = coefficients(N, l, n, rows, KB, 7 * l + N + (form == "rows"))
        got = run_keygen_records(bs.ctx, A, coef, rows, l, KB)
        pb, ps, pv = run_pair(bs.ctx, A, coef, rows, l, KB)
        assert got[1].tolist() == ps.tolist() == [0] * N
        assert np.array_equal(got[0], pb), (l, N)
        assert np.array_equal(got[2], pv), (l, N)
        few = N * (1 if rows == 1 else l) <= 40
        check_against_spec(secpar, A, coef, rows, l, KB, got, None if few else (0, N // 2, N - 1) if rows == 1 or l <= 5 else (N - 1,))


# ---- every field width ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GE.SWEEP_CASES, ids=GE._cid)
def test_every_field_width(case):
    """every wk in 2 .. 32 the modulus admits at the smallest and the largest bound of that width, coefficients that include
    -key_bound and +key_bound at the ends of the polynomials; 5 keys of l = 1 and l = 3 in both forms: at degree 64 with l * wk
    odd the right half of a record begins 8 bytes into a 16-byte unit.  The polynomials are drawn from a pool of six, so that the
    spec transforms few rows."""
    spec, n = case
    ctx = GE._ctx(spec, n)
    seen, odd_halves = set(), 0
    try:
        for wk, KB in X.SWEEP:
            if KB > X.half(spec):
                continue
            seen.add(wk)
            rng = np.random.default_rng(100 * wk + KB % 97)
            pool = rng.integers(-KB, KB + 1, size=(6, n), dtype=np.int64)
            pool[0, 0], pool[0, -1], pool[1, 0], pool[1, -1], pool[2, n // 2 + 3] = -KB, KB, KB, -KB, KB
            for l, rows in ((1, 1), (3, 1), (3, 3)):
                pick = rng.integers(0, 6, size=(5, 2) if rows == 1 else (5, 2, l))
                pick.reshape(5, -1)[:, 0] = [0, 1, 2, 0, 1]
                coef = pool[pick]
                A = any_int32((l, n), wk + l)
                odd_halves += n == 64 and (l * wk) % 2
                got = run_keygen_records(ctx, A, coef, rows, l, KB)
                assert got[1].tolist() == [0] * 5, (wk, KB, l, rows)
                check_against_spec(spec, A, coef, rows, l, KB, got)
    finally:
        ctx.close()
    assert seen == set(range(2, X.width(X.half(spec)) + 1))
    assert (odd_halves > 0) == (n == 64)


# ---- the bound, exactly ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("secpar", [128, 256])
@pytest.mark.parametrize("form", ["one", "rows"])
def test_the_bound_exactly(secpar, form):
    """+key_bound and -key_bound at the first and last value of either half and of a middle row of every key (in the one-polynomial
    form: of the polynomial) encode as fields 2 key_bound and 0; one step further in key 0, 2 or 4 refuses that key alone (status
    4, zero bytes), its neighbours bit-identical to the honest run and its vk still the existing entry's"""
    _, bs = scheme(secpar)
    KB, n, l, N = BETA_SK, bs.d, 3, 5
    wk = X.width(KB)
    rows = 1 if form == "one" else l
    A = any_int32((l, n), secpar + 3)
    coef = coefficients(N, l, n, rows, KB - 1, secpar + (form == "rows"))
    flat = coef.reshape(N, 2, -1)                                      # [N][2][values of a half as given]
    per = flat.shape[2]
    places = [(h, p) for h in (0, 1) for p in (0, per - 1, per // 2 + 3)] + ([(0, n), (1, 2 * n - 1)] if rows == l else [])
    for k, (h, p) in enumerate(places):
        flat[:, h, p] = KB if k % 2 == 0 else -KB
    good = run_keygen_records(bs.ctx, A, coef, rows, l, KB)
    assert good[1].tolist() == [0] * N
    check_against_spec(secpar, A, coef, rows, l, KB, good)
    pb, ps, pv = run_pair(bs.ctx, A, coef, rows, l, KB)
    assert np.array_equal(pb, good[0]) and ps.tolist() == [0] * N and np.array_equal(pv, good[2])
    half_fields = l * n
    for k, (h, p) in enumerate(places):                                # the fields themselves: 2 key_bound and 0
        for rep in range(l if rows == 1 else 1):
            f = X.get_field(good[0][2], h * half_fields + rep * n + p, wk)
            assert f == (2 * KB if k % 2 == 0 else 0), (h, p, rep)
    for key in (0, 2, 4):
        for h, p in places:
            for v in (KB + 1, -KB - 1):
                c2 = coef.copy()
                c2.reshape(N, 2, -1)[key, h, p] = v
                data, st, vk = run_keygen_records(bs.ctx, A, c2, rows, l, KB)
                assert st.tolist() == [4 if i == key else 0 for i in range(N)], (key, h, p, v)
                keep = [i for i in range(N) if i != key]
                assert not data[key].any() and np.array_equal(data[keep], good[0][keep]), (key, h, p, v)
                assert np.array_equal(vk[keep], good[2][keep])
                if (h, p) == places[0] or key == 4:                     # vk of the refused key: the existing entry's
                    pb, ps, pv = run_pair(bs.ctx, A, c2, rows, l, KB)
                    assert np.array_equal(pv, vk) and ps.tolist() == st.tolist() and np.array_equal(pb, data), (key, h, p, v)


# ---- any int32 coefficient ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("secpar", [128, 256])
@pytest.mark.parametrize("form", ["one", "rows"])
def test_any_int32_coefficient(secpar, form):
    """q + 3 and -q - 3 encode as +3 and -3; INT32_MIN, INT32_MAX and a random int32 row are refused unless they are in range after
    reduction (at key_bound = (q - 1) / 2 everything is); vk is fz_keygen_core's whatever the status"""
    _, bs = scheme(secpar)
    q, n, l, N = bs.q, bs.d, 2, 6
    rows = 1 if form == "one" else l
    A = any_int32((l, n), secpar + 5)
    coef = coefficients(N, l, n, rows, 3, secpar + 9)
    flat = coef.reshape(N, -1)
    flat[0, ::2], flat[0, 1::2] = q + 3, -q - 3
    flat[1, 0], flat[2, -1] = I32_MIN, I32_MAX
    flat[3, -n:] = any_int32((n,), secpar + 11)
    flat[4, n // 2] = q + 3                                            # honest after reduction, beside the refused ones
    assert q + 3 <= I32_MAX and -q - 3 >= I32_MIN
    for KB, want in ((BETA_SK, [0, 4, 4, 4, 0, 0]), ((q - 1) // 2, [0] * N)):
        got = run_keygen_records(bs.ctx, A, coef, rows, l, KB)
        assert got[1].tolist() == want
        check_against_spec(secpar, A, coef, rows, l, KB, got)
        wk = X.width(KB)
        assert [X.get_field(got[0][0], j, wk) - KB for j in (0, 1)] == [3, -3]
        pb, ps, pv = run_pair(bs.ctx, A, coef, rows, l, KB)
        assert ps.tolist() == want and np.array_equal(pb, got[0]) and np.array_equal(pv, got[2])


# ---- every multiply form and context -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GE.CASES, ids=GE._cid)
def test_every_multiply_form_and_context(case):
    """the scheme's modulus, the table moduli, the top prime and arbitrary-table contexts: 3 keys of l = 2 in both forms, A at the
    int32 extremes, against the spec; where the tables are a root's the existing pair agrees"""
    spec, n = case
    KB = min(BETA_SK, X.half(spec))
    l, N = 2, 3
    ctx = GE._ctx(spec, n)
    try:
        A = X.multipliers(l, n, 5)
        for rows in (1, l):
            coef = coefficients(N, l, n, rows, KB, 31 + rows)
            coef.reshape(N, -1)[1, 0] = KB + 1 if KB < X.half(spec) else KB       # a refused key between two honest ones
            got = run_keygen_records(ctx, A, coef, rows, l, KB)
            assert got[1].tolist() == [0, 4 if KB < X.half(spec) else 0, 0]
            check_against_spec(spec, A, coef, rows, l, KB, got)
            if spec[1] == "root":
                pb, ps, pv = run_pair(ctx, A, coef, rows, l, KB)
                assert ps.tolist() == got[1].tolist() and np.array_equal(pb, got[0]) and np.array_equal(pv, got[2]), rows
    finally:
        ctx.close()


# ---- graph capture -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("secpar", [128, 256])
def test_graph_capture_replays_the_status_and_the_zeroing(secpar):
    from fusion_hip import DeviceArray
    from fusion_hip.scheme import BatchScheme
    params, shared = scheme(secpar)
    _, KB, wk, kb = SECRET[secpar]
    N, n, l = 5, shared.d, shared.l
    honest = coefficients(N, l, n, 1, KB, secpar)
    refused = honest.copy()
    refused[3, 1, 7] = -KB - 1
    A = shared.A
    want = {id(c): spec_keygen_records(secpar, A, c, 1, l, KB) for c in (honest, refused)}
    assert want[id(refused)][1].tolist() == [0, 0, 0, 4, 0] and not want[id(honest)][1].any()
    bs = BatchScheme(params, private_context=True)
    try:
        ctx = bs.ctx
        dA = DeviceArray.from_numpy(ctx, np.ascontiguousarray(A, dtype=np.int32))
        dC = DeviceArray.from_numpy(ctx, np.ascontiguousarray(refused, dtype=np.int32))
        dB = DeviceArray.from_numpy(ctx, np.full(N * kb + kb + GE.GUARD, BYTE_POISON, dtype=np.uint8))
        dK = DeviceArray.from_numpy(ctx, np.full((N + 1, 2, n), WORD_POISON, dtype=np.int32))
        dV = DeviceArray.from_numpy(ctx, np.full(N + 16, WORD_POISON, dtype=np.int32))
        ctx.graph_begin()
        ctx.keygen_records_async_dev(dA.ptr, dC.ptr, 1, N, l, KB, dB.ptr, dK.ptr, dV.ptr)
        g = ctx.graph_end()
        for c in (refused, honest, refused):
            ctx.h2d(dC.ptr, np.ascontiguousarray(c, dtype=np.int32))    # the input changed in place
            g.launch()
            ctx.synchronize()
            got, vk, st = dB.numpy(), dK.numpy(), dV.numpy()
            wb, ws, wv = want[id(c)]
            assert st[:N].tolist() == ws.tolist()
            assert np.array_equal(got[:N * kb].reshape(N, kb), wb) and np.array_equal(vk[:N], wv)
            assert (got[N * kb:] == BYTE_POISON).all() and (vk[N:] == WORD_POISON).all() and (st[N:] == WORD_POISON).all()
        g.destroy()
        for b in (dA, dC, dB, dK, dV):
            b.free()
    finally:
        bs.close()


# ---- argument rules ----------------------------------------------------------------------------------------------------------
def test_refusals_of_the_entry():
    import fusion_hip
    from fusion_hip import DeviceArray, FusionHipError
    from fusion_hip._lib import FZ_E_BADARG, FZ_E_UNSUPPORTED
    _, bs = scheme(256)
    ctx, d, q = bs.ctx, bs.d, bs.q
    l, KB = 2, 52
    kb = X.record_bytes(d, 2 * l, X.width(KB))
    top = (q - 1) // 2
    dA = DeviceArray.from_numpy(ctx, np.zeros(l * d + 16, dtype=np.int32))
    dC = DeviceArray.from_numpy(ctx, np.zeros(2 * 2 * l * d + 16, dtype=np.int32))
    dB = DeviceArray.from_numpy(ctx, np.full(2 * kb + 64, BYTE_POISON, dtype=np.uint8))
    dK = DeviceArray.from_numpy(ctx, np.full(2 * 2 * d + 16, WORD_POISON, dtype=np.int32))
    dV = DeviceArray.from_numpy(ctx, np.full(16, WORD_POISON, dtype=np.int32))

    def untouched():
        ctx.synchronize()
        assert (dB.numpy() == BYTE_POISON).all() and (dK.numpy() == WORD_POISON).all() and (dV.numpy() == WORD_POISON).all()
        assert not dA.numpy().any() and not dC.numpy().any()

    try:
        good = [dA.ptr, dC.ptr, 1, 2, l, KB, dB.ptr, dK.ptr, dV.ptr]
        bad = []
        for coef_rows in (0, 3, -1, l + 1):                            # the form: 1 or l
            bad.append(good[:2] + [coef_rows] + good[3:])
        for ll in (0, -1):
            bad.append(good[:2] + [1, 2, ll] + good[5:])
        for kbd in (0, -1, top + 1):
            bad.append(good[:5] + [kbd] + good[6:])
        for i in (0, 1, 6, 7, 8):                                      # each of the five pointers: off by 4, by 8, NULL
            for p in (good[i] + 4, good[i] + 8, 0):
                bad.append(good[:i] + [p] + good[i + 1:])
        bad.append(good[:3] + [0, l, 0] + good[6:])                    # N = 0 does not excuse a bad bound, l or form
        bad.append(good[:3] + [0, 0, KB] + good[6:])
        bad.append(good[:2] + [3, 0, l, KB] + good[6:])
        for args in bad:
            with pytest.raises(FusionHipError) as e:
                ctx.keygen_records_async_dev(*args)
            assert e.value.code == FZ_E_BADARG, args
        ctx.keygen_records_async_dev(*(good[:2] + [l] + good[3:]))      # both forms are taken ...
        ctx.synchronize()
        assert dV.numpy()[:2].tolist() == [0, 0] and (dV.numpy()[2:] == WORD_POISON).all()
        ctx.h2d(dB.ptr, np.full(2 * kb + 64, BYTE_POISON, dtype=np.uint8))
        ctx.h2d(dK.ptr, np.full(2 * 2 * d + 16, WORD_POISON, dtype=np.int32))
        ctx.h2d(dV.ptr, np.full(16, WORD_POISON, dtype=np.int32))
        ctx.keygen_records_async_dev(*(good[:3] + [0] + good[4:]))      # N = 0: OK, nothing written
        ctx.keygen_records_async_dev(0, 0, l, 0, l, top, 0, 0, 0)       # ... whatever the pointers
        untouched()
        q128, root, inv_root = X.E.root_of("scheme", 128)
        other = fusion_hip.Context(q128, 128, root, inv_root)
        try:
            for args in (good[:5] + [0] + good[6:], good[:2] + [3] + good[3:],       # a bad bound or form comes before the degree
                         good[:6] + [dB.ptr + 8] + good[7:], good[:7] + [0] + good[8:]):     # ... and so do the pointers
                with pytest.raises(FusionHipError) as e:
                    other.keygen_records_async_dev(*args)
                assert e.value.code == FZ_E_BADARG, args
            other.keygen_records_async_dev(*(good[:3] + [0] + good[4:]))             # N = 0 before the degree as well
            with pytest.raises(FusionHipError) as e:
                other.keygen_records_async_dev(*good)
            assert e.value.code == FZ_E_UNSUPPORTED
        finally:
            other.close()
        untouched()
    finally:
        for b in (dA, dC, dB, dK, dV):
            b.free()


# ---- from seeds to a verified aggregate, nothing expanded --------------------------------------------------------------------
@pytest.mark.parametrize("secpar", [128, 256])
def test_the_flow_with_nothing_expanded(secpar):
    from fusion_hip import DeviceArray, FusionHipError
    from fusion_hip._lib import FZ_E_BADARG
    _, bs = scheme(secpar)
    _, B, w, rb = TABLE["signature"][secpar]
    kb = SECRET[secpar][3]
    n = 33
    seeds = [900 + 13 * k for k in range(n)]
    msgs = [f"keygen-flow-{secpar}-{k}" for k in range(n)]
    sk, vk = bs.keygen_batch(seeds)
    want_recs, codes = bs.encode("secret", sk)
    assert codes.tolist() == [0] * n
    want_sig = bs.sign_batch(sk, vk, msgs)
    dK, vk2, dVk = bs.keygen_batch_encoded(seeds, device=True, keep_vk=True)
    dB = None
    try:
        assert isinstance(dK, DeviceArray) and dK.dtype == np.uint8 and dK.shape == (n, kb)
        assert isinstance(dVk, DeviceArray) and dVk.dtype == np.int32 and dVk.shape == (n, 2, bs.d)
        assert isinstance(vk2, np.ndarray) and vk2.dtype == np.int32
        assert np.array_equal(dK.numpy(), want_recs) and np.array_equal(vk2, vk) and np.array_equal(dVk.numpy(), vk)
        dB, codes = bs.sign_batch_records(dK, dVk, msgs, device=True)
        assert isinstance(dB, DeviceArray) and dB.shape == (n, rb) and codes.tolist() == [0] * n
        assert np.array_equal(dB.numpy(), bs.encode("signature", want_sig)[0])
        assert np.array_equal(dK.numpy(), want_recs) and np.array_equal(dVk.numpy(), vk)
        assert bs.verify_signatures_encoded(vk, msgs, dB).tolist() == bs.verify_signatures(vk, msgs, want_sig).tolist() == [0] * n
        agg, codes = bs.aggregate_encoded(vk, msgs, dB)
        assert codes.tolist() == [0] * n
        assert np.array_equal(agg, bs.aggregate(vk, msgs, want_sig))
        assert bs.verify(vk, msgs, agg) == (True, "")
    finally:
        dK.free()
        dVk.free()
        if dB is not None:
            dB.free()
    # the host forms, and the samplers keygen_batch chooses between
    recs, vk3, dVk = bs.keygen_batch_encoded(seeds[:5], keep_vk=True)
    try:
        assert isinstance(recs, np.ndarray) and np.array_equal(recs, want_recs[:5]) and np.array_equal(vk3, vk[:5])
        assert np.array_equal(dVk.numpy(), vk[:5])
    finally:
        dVk.free()
    odd = [-5, 2 ** 70]                                            # seeds only the Python sampler takes
    sk2, want_vk2 = bs.keygen_batch(odd)
    recs2, vk2 = bs.keygen_batch_encoded(odd)
    assert np.array_equal(recs2, bs.encode("secret", sk2)[0]) and np.array_equal(vk2, want_vk2)
    was = bs.device_sampler
    try:
        bs.device_sampler = False                                  # the host clone
        recs3, vk3 = bs.keygen_batch_encoded(seeds[:5])
        assert np.array_equal(recs3, want_recs[:5]) and np.array_equal(vk3, vk[:5])
    finally:
        bs.device_sampler = was
    # a key over beta_sk: the error names it
    try:
        polys = np.zeros((3, 2, bs.d), dtype=np.int32)
        polys[1, 0, 4] = bs.params.beta_sk + 1
        bs._sample_polys = lambda s, seeds_: polys
        with pytest.raises(FusionHipError) as e:
            bs.keygen_batch_encoded([1, 2, 3])
        assert e.value.code == FZ_E_BADARG and "key 1" in str(e.value)
    finally:
        del bs._sample_polys


# ---- object face -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("secpar", [128, 256])
def test_keygen_to_bytes_equals_keygen_then_to_bytes(secpar):
    import fusion.fusion as F
    from fusion_hip.scheme import encoded_size
    params, _ = scheme(secpar)
    for seed in (4100 + secpar, 77):
        random.seed(12345)
        key = F.keygen(params, seed)
        after_keygen = random.getstate()
        want = F.to_bytes(params, key[0])
        random.seed(12345)
        data, vkey = F.keygen_to_bytes(params, seed)
        assert random.getstate() == after_keygen
        assert isinstance(data, bytes) and len(data) == encoded_size(params, "secret") and data == want
        assert isinstance(vkey, F.OneTimeVerificationKey) and str(vkey) == str(key[1])
