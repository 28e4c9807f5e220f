"""Verification keys derived straight from compact secret-key records on the device (fz_vk_records_async, Context.vk_records,
BatchScheme.vk_from_records / sign_batch_secret / check_keypairs, fusion.fusion.vk_of_secret_bytes / sign_from_secret_bytes):
everything is compared with the CPU spec of tests/test_vk_records_host.py (spec_vk_records) bit for bit, status words and the
zero rows of refused keys included.  The raw entry runs inside the guarded arena of tests/_guarded.py, which takes byte operands
as it takes words: every operand between 16 KiB guards, once per fill of the guards and of the outputs' previous contents, the
guards intact, the inputs unchanged and the outputs the same under both fills.  No tolerance anywhere."""
import os

import numpy as np
import pytest

import _encoded_edges as X
import _guarded as GD
import test_gpu_encoded_edges as GE
from test_gpu_encoding import scheme
from test_gpu_sign_records import pack_fields
from test_sign_records_host import BETA_SK, SECRET
from test_vk_records_host import spec_vk_records

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
WORD_POISON = 0x5a5a5a5a
SECPAR_OF = {64: 128, 256: 256}


def run_vk(ctx, recs, KB, A, l, want_vk, want_st):
    """fz_vk_records_async on key records [N][2 l n wk / 8] and A [l][n] inside the guarded arena: vk and status are want_vk and
    want_st exactly under both fills, nothing else is written, the inputs are unchanged"""
    recs = np.ascontiguousarray(recs, dtype=np.uint8)
    N = recs.shape[0]
    ops = [GD.inp("A", np.ascontiguousarray(A).astype(np.int32)), GD.inp("key", recs),
           GD.out("vk", np.asarray(want_vk).astype(np.int32)), GD.out("status", np.asarray(want_st, dtype=np.int32))]
    GD.on_device(ctx, ops, lambda p: ctx.vk_records_async_dev(p["A"].ptr, p["key"].ptr, int(KB), N, l, p["vk"].ptr, p["status"].ptr))


def check(ctx, spec, recs, KB, A, l, counts=None):
    """the spec of all the records once; the entry on the first N of them for every N of `counts` (default: all)"""
    want_vk, want_st = spec_vk_records(spec, recs, KB, A, l)
    for N in counts or (recs.shape[0],):
        run_vk(ctx, recs[:N], KB, A, l, want_vk[:N], want_st[:N])
    return want_vk, want_st


# ---- scheme shapes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("secpar", [128, 256])
def test_scheme_shapes(secpar):
    from fusion_hip import DeviceArray
    _, bs = scheme(secpar)
    _, KB, wk, kb = SECRET[secpar]
    n = 5
    seeds = [4100 + 13 * k for k in range(n)]
    msgs = [f"vk-records-{secpar}-{k}" for k in range(n)]
    recs, vk, dVK = bs.keygen_batch_encoded(seeds, keep_vk=True)
    dVK.free()
    assert recs.shape == (n, kb)
    want_vk, want_st = spec_vk_records(secpar, recs, KB, bs.A, bs.l)
    assert not want_st.any() and np.array_equal(want_vk, vk)
    got, codes = bs.vk_from_records(recs)
    assert isinstance(got, np.ndarray) and got.dtype == np.int32 and got.shape == (n, 2, bs.d)
    assert codes.dtype == np.int32 and codes.tolist() == [0] * n and np.array_equal(got, vk)
    dV, codes = bs.vk_from_records(recs.tobytes(), device=True)
    try:
        assert isinstance(dV, DeviceArray) and dV.shape == (n, 2, bs.d) and dV.dtype == np.int32
        assert codes.tolist() == [0] * n and np.array_equal(dV.numpy(), vk)
        want_b, want_c = bs.sign_batch_records(recs, vk, msgs)
        data, codes = bs.sign_batch_records(recs, dV, msgs)                   # the derived keys as they are
        assert codes.tolist() == want_c.tolist() == [0] * n and np.array_equal(data, want_b)
        c_hat, _ = bs.challenges_dev(dV, msgs)
        try:
            assert np.array_equal(c_hat.numpy(), bs.challenges(vk, msgs)[0])
        finally:
            c_hat.free()
    finally:
        dV.free()
    for device in (False, True):
        data, codes, keys = bs.sign_batch_secret(recs, msgs, device=device)
        if device:
            assert isinstance(data, DeviceArray)
            host = data.numpy()
            data.free()
            data = host
        assert codes.tolist() == [0] * n and np.array_equal(data, want_b)
        assert isinstance(keys, np.ndarray) and np.array_equal(keys, vk)
    # the staged host face of the context
    got, codes = bs.ctx.vk_records(recs, KB, bs.A, bs.l)
    assert codes.tolist() == [0] * n and np.array_equal(got, vk)
    # check_keypairs: the pairs, two keys swapped, a record that is not canonical
    assert bs.check_keypairs(recs, vk).tolist() == [0] * n
    assert bs.check_keypairs(recs, X.other_representative(vk, bs.q).astype(np.int32)).tolist() == [0] * n      # equal mod q
    swapped = vk.copy()
    swapped[[1, 3]] = vk[[3, 1]]
    assert bs.check_keypairs(recs, swapped).tolist() == [0, 3, 0, 3, 0]
    bad = recs.copy()
    bad[2] = X.set_field(bad[2], bs.l * bs.d + 9, 2 * KB + 1, wk)
    assert bs.check_keypairs(bad, swapped).tolist() == [0, 3, 6, 3, 0]
    keys, codes = bs.vk_from_records(bad)
    assert codes.tolist() == [0, 0, 6, 0, 0] and not keys[2].any() and np.array_equal(keys[[0, 1, 3, 4]], vk[[0, 1, 3, 4]])
    # a record with code 6 signs nothing, the others as before
    data, codes, keys = bs.sign_batch_secret(bad, msgs)
    assert codes.tolist() == [0, 0, 6, 0, 0] and not data[2].any() and not keys[2].any()
    assert np.array_equal(data[[0, 1, 3, 4]], want_b[[0, 1, 3, 4]]) and np.array_equal(keys[[0, 1, 3, 4]], vk[[0, 1, 3, 4]])


@pytest.mark.parametrize("secpar", [128, 256])
def test_object_face(secpar):
    import fusion.fusion as F
    from fusion_hip import ENCODING_REASONS
    params, _ = scheme(secpar)
    q = params.modulus
    b, vk = F.keygen_to_bytes(params, 977)
    got = F.vk_of_secret_bytes(params, b)
    assert isinstance(got, F.OneTimeVerificationKey)
    for side in ("left_vk_hat", "right_vk_hat"):
        assert np.array_equal(F._rows_of(getattr(got, side), q), F._rows_of(getattr(vk, side), q))
    assert str(got) == str(vk)                                                  # what hash_ch hashes
    s, key = F.sign_from_secret_bytes(params, b, "from the record alone")
    assert isinstance(s, bytes) and s == F.sign_from_bytes(params, b, vk, "from the record alone") and str(key) == str(vk)
    bad = X.set_field(np.frombuffer(b, dtype=np.uint8), 0, 2 * BETA_SK + 1, 7).tobytes()
    for call in (lambda: F.vk_of_secret_bytes(params, bad), lambda: F.sign_from_secret_bytes(params, bad, "m")):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == ENCODING_REASONS[6]
    with pytest.raises(ValueError):
        F.vk_of_secret_bytes(params, b[:-1])


# ---- general rows ------------------------------------------------------------------------------------------------------------
ROWS = [(256, l) for l in (1, 3, 4, 5, 9)] + [(64, l) for l in (1, 15, 16, 17, 33)]


@pytest.mark.parametrize("n,l", ROWS, ids=lambda v: str(v))
def test_independent_rows_at_every_tail_and_key_count(n, l):
    """independent random fields in [0, 2B] per row with 0 and 2B at the ends of every record, random and int32-extreme A; fewer
    rows than a chunk holds, exactly a chunk, one more, and a third chunk with one row in it; 1, 2, 3 and 7 keys (more chunks
    than a workgroup has waves, the pipelined loop: l = 195 below and l = 83 of the scheme's own shape)"""
    secpar = SECPAR_OF[n]
    _, bs = scheme(secpar)
    KB, wk = BETA_SK, 7
    recs = pack_fields(X.edge_fields(KB, 7, 2 * l, n, 1000 * n + l), wk)
    A = X.multipliers(l, n, 3 * l + n)
    want_vk, want_st = check(bs.ctx, secpar, recs, KB, A, l, counts=(1, 2, 3, 7))
    assert not want_st.any() and want_vk.any()


@pytest.mark.parametrize("l,wk", [(1, 7), (3, 7), (195, 7), (2, 7), (1, 8)])
def test_degree_64_halves_on_either_alignment(l, wk):
    """l * wk odd: the right half of every key, and both halves of every other key, begin 8 mod 16; even: every half on 16"""
    _, bs = scheme(128)
    n, KB = 64, {7: BETA_SK, 8: 100}[wk]
    assert X.width(KB) == wk and (X.record_bytes(n, l, wk) % 16 == 8) == (l * wk % 2 == 1)
    recs = pack_fields(X.edge_fields(KB, 3, 2 * l, n, 64 * l + wk), wk)
    check(bs.ctx, 128, recs, KB, X.multipliers(l, n, l + wk), l, counts=(1, 3))


@pytest.mark.parametrize("n", [64, 256])
@pytest.mark.parametrize("wk,KB", [(2, 1), (7, 52), (8, 100), (13, 4000), (31, None)])
def test_field_widths_odd_and_even(n, wk, KB):
    secpar = SECPAR_OF[n]
    _, bs = scheme(secpar)
    KB = (bs.q - 1) // 2 if KB is None else KB
    assert X.width(KB) == wk
    l = 3
    recs = pack_fields(X.edge_fields(KB, 3, 2 * l, n, 77 * wk + n), wk)
    check(bs.ctx, secpar, recs, KB, X.multipliers(l, n, wk), l)


@pytest.mark.parametrize("n", [64, 256])
def test_field_width_32(n):
    spec = ("top", "root")
    KB = X.half(spec)
    assert X.width(KB) == 32
    ctx = GE._ctx(spec, n)
    try:
        l = 3
        recs = pack_fields(X.edge_fields(KB, 3, 2 * l, n, 32 + n), 32)
        check(ctx, spec, recs, KB, X.multipliers(l, n, 32), l)
    finally:
        ctx.close()


@pytest.mark.parametrize("n", [64, 256])
@pytest.mark.parametrize("which", ["one", "half"])
def test_bounds_with_fields_at_zero_and_twice_the_bound_everywhere(n, which):
    """B = 1 and B = (q - 1) / 2, every field 0 or 2B: s = -B or +B on every coefficient, the largest operands the passes see"""
    secpar = SECPAR_OF[n]
    _, bs = scheme(secpar)
    KB = 1 if which == "one" else (bs.q - 1) // 2
    l, rng = 3, np.random.default_rng(n + KB % 97)
    u = np.stack([np.zeros((2 * l, n), dtype=np.int64), np.full((2 * l, n), 2 * KB, dtype=np.int64),
                  np.tile(np.array([0, 2 * KB], dtype=np.int64), (2 * l, n // 2)),
                  rng.integers(0, 2, size=(2 * l, n), dtype=np.int64) * 2 * KB])
    want_vk, want_st = check(bs.ctx, secpar, pack_fields(u, X.width(KB)), KB, X.multipliers(l, n, 11), l)
    assert not want_st.any()


# ---- both multiply forms and table contexts ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GE.SWEEP_CASES, ids=GE._cid)
def test_both_multiply_forms_and_table_contexts(case):
    spec, n = case
    l = 5 if n == 256 else 17
    ctx = GE._ctx(spec, n)
    try:
        for KB in sorted({min(BETA_SK, X.half(spec)), X.half(spec)}):
            recs = pack_fields(X.edge_fields(KB, 3, 2 * l, n, 900 + n + KB % 89), X.width(KB))
            check(ctx, spec, recs, KB, X.multipliers(l, n, 5 + KB % 7), l)
    finally:
        ctx.close()


# ---- status isolation --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 256])
def test_a_refused_key_is_refused_alone(n):
    """a field at 2B + 1 in the last row of the right half of key 1 of 3, and in the first row of the left half: key 1 is zero in
    BOTH halves (the other half's workgroup never saw the flag), keys 0 and 2 are what they were"""
    secpar = SECPAR_OF[n]
    _, bs = scheme(secpar)
    KB, wk, l = BETA_SK, 7, 5 if n == 256 else 17
    recs = pack_fields(X.edge_fields(KB, 3, 2 * l, n, 500 + n), wk)
    A = X.multipliers(l, n, 9)
    good_vk, good_st = check(bs.ctx, secpar, recs, KB, A, l)
    assert not good_st.any() and good_vk[1, 0].any() and good_vk[1, 1].any()
    for field in (2 * l * n - 1, (2 * l - 1) * n, 0, n - 1):
        bad = recs.copy()
        bad[1] = X.set_field(bad[1], field, 2 * KB + 1, wk)
        want_vk, want_st = check(bs.ctx, secpar, bad, KB, A, l)
        assert want_st.tolist() == [0, 6, 0] and not want_vk[1].any() and np.array_equal(want_vk[[0, 2]], good_vk[[0, 2]]), field


# ---- stale outputs -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 256])
def test_outputs_that_hold_the_answer_of_another_input(n):
    """d_vk and d_status hold the expected answer of a DIFFERENT input (another key refused, other fields) before the call"""
    secpar = SECPAR_OF[n]
    _, bs = scheme(secpar)
    ctx, KB, wk, l = bs.ctx, BETA_SK, 7, 3
    A = np.ascontiguousarray(X.multipliers(l, n, 21)).astype(np.int32)
    inputs = []
    for k, refused in enumerate((1, 2)):
        recs = pack_fields(X.edge_fields(KB, 4, 2 * l, n, 640 + n + k), wk)
        recs[refused] = X.set_field(recs[refused], 3 + k * l * n, 2 * KB + 1, wk)
        inputs.append((recs,) + spec_vk_records(secpar, recs, KB, A, l))
    assert inputs[0][2].tolist() == [0, 6, 0, 0] and inputs[1][2].tolist() == [0, 0, 6, 0]
    bufs = GE.Bufs(ctx)
    try:
        dA = bufs.put(A)
        for this, other in ((0, 1), (1, 0)):
            recs, want_vk, want_st = inputs[this]
            dK = bufs.put(recs)
            dV = bufs.put(np.concatenate([inputs[other][1].astype(np.int32).ravel(), np.full(64, WORD_POISON, dtype=np.int32)]))
            dS = bufs.put(np.concatenate([inputs[other][2], np.full(16, WORD_POISON, dtype=np.int32)]))
            ctx.vk_records_async_dev(dA.ptr, dK.ptr, KB, 4, l, dV.ptr, dS.ptr)
            vk, st = dV.numpy(), dS.numpy()
            assert st[:4].tolist() == want_st.tolist() and (st[4:] == WORD_POISON).all()
            assert np.array_equal(vk[:4 * 2 * n].reshape(4, 2, n), want_vk) and (vk[4 * 2 * n:] == WORD_POISON).all()
            assert np.array_equal(dK.numpy(), recs) and np.array_equal(dA.numpy(), A)
    finally:
        bufs.free()


# ---- many units --------------------------------------------------------------------------------------------------------------
def test_more_units_than_a_grid_dimension_of_65535():
    """l = 1 at degree 64 (a key is 112 bytes at wk = 7), 40 000 keys: 80 000 (key, half) units, every key compared.  The spec
    of so many rows is the transform as a matrix product in int64 (|s| <= 52, entries below 2^31, 64 terms: below 2^44), held to
    spec_vk_records on the first keys"""
    _, bs = scheme(128)
    ctx, n, l, KB, wk, N = bs.ctx, 64, 1, BETA_SK, 7, 40000
    q = bs.q
    rng = np.random.default_rng(40000)
    u = rng.integers(0, 2 * KB + 1, size=(N, 2 * n), dtype=np.int64)
    refused = [0, 777, 39999]
    u[0, 5], u[777, n + 1], u[39999, 2 * n - 1] = 2 * KB + 1, 2 * KB + 1, 127
    recs = pack_fields(u, wk)
    assert recs.shape == (N, 112)
    A = X.multipliers(l, n, 4)
    F = X.forward((128, "params"), n, np.eye(n, dtype=np.int64))              # row i: FWD(e_i)
    fwd = X.cent((u - KB).reshape(2 * N, n) @ F, q)
    want = X.cent(X.cent(fwd * A[0][None], q), q).reshape(N, 2, n)
    want[refused] = 0
    want_st = np.zeros(N, dtype=np.int32)
    want_st[refused] = 6
    head_vk, head_st = spec_vk_records(128, recs[:8], KB, A, l)
    assert np.array_equal(head_vk, want[:8]) and np.array_equal(head_st, want_st[:8])
    bufs = GE.Bufs(ctx)
    try:
        dA, dK = bufs.put(np.ascontiguousarray(A).astype(np.int32)), bufs.put(recs)
        dV = bufs.put(np.full(N * 2 * n + 64, WORD_POISON, dtype=np.int32))
        dS = bufs.put(np.full(N + 16, WORD_POISON, dtype=np.int32))
        ctx.vk_records_async_dev(dA.ptr, dK.ptr, KB, N, l, dV.ptr, dS.ptr)
        vk, st = dV.numpy(), dS.numpy()
        assert np.array_equal(st[:N], want_st) and (st[N:] == WORD_POISON).all()
        assert np.array_equal(vk[:N * 2 * n].reshape(N, 2, n), want) and (vk[N * 2 * n:] == WORD_POISON).all()
        assert np.array_equal(dK.numpy(), recs)
    finally:
        bufs.free()


# ---- graph capture -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("secpar", [128, 256])
def test_graph_capture_as_the_first_call_of_a_context(secpar):
    from fusion_hip import DeviceArray
    from fusion_hip.scheme import BatchScheme
    params, shared = scheme(secpar)
    rows, KB, wk, kb = SECRET[secpar]
    l, d, n = rows // 2, shared.d, 5
    contents = []
    for r in range(2):
        recs = pack_fields(X.edge_fields(KB, n, 2 * l, d, 300 + secpar + r), wk)
        if r == 1:                                                 # a refused key: status and zeroing replay too
            recs[3] = X.set_field(recs[3], l * d + 17, 2 * KB + 1, wk)
        contents.append((recs,) + spec_vk_records(secpar, recs, KB, shared.A, l))
    assert contents[0][2].tolist() == [0] * n and contents[1][2].tolist() == [0, 0, 0, 6, 0]
    bs = BatchScheme(params, private_context=True)
    try:
        ctx = bs.ctx
        dA = DeviceArray.from_numpy(ctx, shared.A)
        dK, dV, dS = DeviceArray(ctx, (n, kb), np.uint8), DeviceArray(ctx, (n, 2, d)), DeviceArray(ctx, (n,))

        def load(r):
            ctx.h2d(dK.ptr, contents[r][0])
            ctx.h2d(dV.ptr, np.full((n, 2, d), WORD_POISON, dtype=np.int32))
            ctx.h2d(dS.ptr, np.full(n, WORD_POISON, dtype=np.int32))

        load(0)
        ctx.graph_begin()                                          # the context has launched nothing yet
        ctx.vk_records_async_dev(dA.ptr, dK.ptr, KB, n, l, dV.ptr, dS.ptr)
        g = ctx.graph_end()
        for r in (0, 1, 0):
            load(r)
            g.launch()
            ctx.synchronize()
            assert dS.numpy().tolist() == contents[r][2].tolist(), r
            assert np.array_equal(dV.numpy(), contents[r][1]), r
        g.destroy()
        load(1)                                                    # ... and the same eagerly
        ctx.vk_records_async_dev(dA.ptr, dK.ptr, KB, n, l, dV.ptr, dS.ptr)
        assert dS.numpy().tolist() == contents[1][2].tolist() and np.array_equal(dV.numpy(), contents[1][1])
        for b in (dA, dK, dV, dS):
            b.free()
    finally:
        bs.close()


# ---- refusals of the entry that need a device --------------------------------------------------------------------------------
def test_too_many_rows_for_exact_sums_are_refused():
    """l = 2^22 at degree 64 passes every shared check (2 l * 64 = 2^29 values per record) and is the launcher's to refuse:
    FZ_E_UNSUPPORTED, nothing written.  At degree 256 the same l is over the size of a record: FZ_E_BADARG."""
    from fusion_hip._lib import FZ_E_BADARG, FZ_E_UNSUPPORTED
    for secpar, code in ((128, FZ_E_UNSUPPORTED), (256, FZ_E_BADARG)):
        _, bs = scheme(secpar)
        ctx, n = bs.ctx, bs.d
        ops = [GD.inp("A", np.zeros((1, n), dtype=np.int32)), GD.inp("key", np.zeros((1, 112), dtype=np.uint8)),
               GD.out("vk", np.zeros((1, 2, n), dtype=np.int32)), GD.out("status", np.zeros(1, dtype=np.int32))]
        GD.refused(ctx, ops, lambda p: ctx.vk_records_async_dev(p["A"].ptr, p["key"].ptr, BETA_SK, 1, 1 << 22, p["vk"].ptr, p["status"].ptr), code)
        if secpar == 128:                                          # one row fewer goes to the kernel's side of the line: not run here
            GD.refused(ctx, ops, lambda p: ctx.vk_records_async_dev(p["A"].ptr, p["key"].ptr, BETA_SK, 1, 1 << 23, p["vk"].ptr, p["status"].ptr),
                       FZ_E_UNSUPPORTED)
