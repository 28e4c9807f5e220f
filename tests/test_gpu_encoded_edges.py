"""The compact-bytes kernels (records_encode / records_decode, encoded_check, aggregate_encoded, verify_encoded and its finish
kernel) at every multiply form and field width, through the C-ABI device entries of fusion_hip.Context, against the
context-parametric spec of tests/_encoded_edges.py: the moduli and tables of tests/_transform_edges.py on either side of `fast`
and q = 4294828033 (so the 6-op instantiations and 32-bit fields run), degrees 64 and 256, int32-extreme rows on the encoder's
side with the bound at each record's exact maximum M and at M - 1, fields at 0 and 2B in the stage sign patterns at
B = (q - 1) / 2 on the decoder's, int32-extreme multipliers, every field width 2 .. 32 at its smallest and largest bound (in the
record walkers and in the per-record consumers), a stream that ends half a 16-byte unit in, both grid forms of the verification.  Buffers are exactly sized with poisoned guards
behind every output; everything is compared bit for bit."""
import functools

import numpy as np
import pytest

import _encoded_edges as X
import test_gpu_aggregate_encoded as GA
import test_gpu_verify_encoded as GV

pytestmark = pytest.mark.gpu

GUARD = 64
BYTE_POISON, ROW_POISON, WORD_POISON = 0xab, 0x5a5a5a5a, 0x7f7f7f7f
CASES = [(s, n) for s in X.SPECS for n in X.DEGREES]
SWEEP_CASES = [(s, n) for s in X.SWEEP_SPECS for n in X.DEGREES]


def _cid(c):
    return f"{X.sid(c[0])}-d{c[1]}"


def _ctx(spec, n):
    """as tests/test_gpu_transform_edges.py builds them: a table context for the top / odd tables, the ordinary root context
    (which builds the tables X.tables lists) for the primes with roots"""
    import fusion_hip
    if spec[1] == "root":
        q, root, inv_root = X.root_of(spec, n)
        return fusion_hip.Context(q, n, root, inv_root)
    q, fwd, inv = X.tables(spec, n)
    return fusion_hip.Context(q, n, 0, 0, tables=(fwd, inv))


@functools.lru_cache(maxsize=None)
def _num_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


class Bufs:
    """device arrays freed together"""

    def __init__(self, ctx):
        self.ctx, self.all = ctx, []

    def put(self, a):
        from fusion_hip import DeviceArray
        self.all.append(DeviceArray.from_numpy(self.ctx, a))
        return self.all[-1]

    def free(self):
        for b in self.all:
            b.free()


def _guarded(payload, dtype, poison, guard):
    return np.full(payload + guard, poison, dtype=dtype)


def run_encode(ctx, rows, coef, B):
    """fz_encode_records_async on rows [N][R][n] -> (bytes [N][record bytes], status [N]); nothing behind the stream or the
    status words is touched, the rows are unchanged"""
    N, R, n = rows.shape
    rb = X.record_bytes(n, R, X.width(B))
    x = np.ascontiguousarray(rows, dtype=np.int32)
    bufs = Bufs(ctx)
    try:
        dX, dB = bufs.put(x), bufs.put(_guarded(N * rb, np.uint8, BYTE_POISON, GUARD))
        dV = bufs.put(_guarded(N, np.int32, WORD_POISON, 16))
        ctx.encode_records_async_dev(dX.ptr, N, R, coef, B, dB.ptr, dV.ptr)
        got, st = dB.numpy(), dV.numpy()
        assert (got[N * rb:] == BYTE_POISON).all() and (st[N:] == WORD_POISON).all() and np.array_equal(dX.numpy(), x)
        return got[:N * rb].reshape(N, rb), st[:N]
    finally:
        bufs.free()


def run_decode(ctx, data, R, n, coef, B, check=False):
    """fz_decode_records_async (or fz_check_records_async) on bytes [N][record bytes] -> (rows [N][R][n], status [N]); the row
    behind the last record and the status words behind the last one are untouched, the bytes unchanged (check: no rows at all)"""
    N = data.shape[0]
    raw = np.concatenate([np.ascontiguousarray(data, dtype=np.uint8).ravel(), np.full(GUARD, BYTE_POISON, dtype=np.uint8)])
    bufs = Bufs(ctx)
    try:
        dB, dV = bufs.put(raw), bufs.put(_guarded(N, np.int32, WORD_POISON, 16))
        dR = bufs.put(np.full((N + 1, R, n), ROW_POISON, dtype=np.int32))
        if check:
            ctx.check_records_async_dev(dB.ptr, N, R, B, dV.ptr)
        else:
            ctx.decode_records_async_dev(dB.ptr, N, R, coef, B, dR.ptr, dV.ptr)
        back, st = dR.numpy(), dV.numpy()
        assert (st[N:] == WORD_POISON).all() and np.array_equal(dB.numpy(), raw)
        assert (back[N if not check else 0:] == ROW_POISON).all()
        return back[:N], st[:N]
    finally:
        bufs.free()


def _spoil(data, B, rows_n, which):
    """(copy of data with the records of `which` = [(record, field)] set to 2B + 1 there, the codes the decoder owes)"""
    d2, codes = data.copy(), np.zeros(data.shape[0], dtype=np.int32)
    for i, j in which:
        bad = X.one_past(d2[i], j % rows_n, B)
        if bad is not None:
            d2[i], codes[i] = bad, 6
    return d2, codes


def _decode_and_check(ctx, data, want_rows, R, n, coef, B, spoil):
    """decode and check of canonical bytes, then of the same bytes with the records of `spoil` one past the bound"""
    N = data.shape[0]
    back, st = run_decode(ctx, data, R, n, coef, B)
    assert not st.any() and np.array_equal(back, want_rows)
    _, st = run_decode(ctx, data, R, n, coef, B, check=True)
    assert not st.any()
    d2, codes = _spoil(data, B, R * n, spoil)
    if codes.any():
        want = np.where((codes != 0)[:, None, None], 0, want_rows)
        back, st = run_decode(ctx, d2, R, n, coef, B)
        assert st.tolist() == codes.tolist() and np.array_equal(back, want)
        _, st = run_decode(ctx, d2, R, n, coef, B, check=True)
        assert st.tolist() == codes.tolist()
    assert N == want_rows.shape[0]


# ---- encode ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_encode_at_each_records_exact_maximum(case):
    """int32-extreme rows in records of 1, 2 and 5: at B = (q - 1) / 2 every record encodes to the spec's bytes; at bound = M
    of a record every record with maximum <= M encodes and the others are refused (status 4, all-zero bytes), at M - 1 that
    record is refused too.  Root contexts and keys: decoding the full-range bytes returns the centred rows."""
    spec, n = case
    q, B = X.modulus(spec), X.half(spec)
    rows = X.encoder_rows(spec, n)
    ctx = _ctx(spec, n)
    try:
        for coef in (True, False):
            for per in (1, 2, 5):
                rec = X.records_of(rows, per)
                z = X.values(spec, n, rec, coef)
                want, wst = X.encoded(z, B)
                assert not wst.any()
                data, st = run_encode(ctx, rec, coef, B)
                assert not st.any(), (coef, per, st)
                assert np.array_equal(data, want), (coef, per)
                if spec[1] == "root" or not coef:
                    back, st = run_decode(ctx, data, per, n, coef, B)
                    assert not st.any() and np.array_equal(back, X.cent(rec, q)), (coef, per)
                for m in sorted(set(X.maxima(z).tolist())):
                    for bound in (m, m - 1):
                        if bound < 1:
                            continue
                        want, wst = X.encoded(z, bound)
                        data, st = run_encode(ctx, rec, coef, bound)
                        assert st.tolist() == wst.tolist(), (coef, per, bound)
                        assert np.array_equal(data, want), (coef, per, bound)
                        assert (wst[X.maxima(z) == m] == (0 if bound == m else 4)).all()
    finally:
        ctx.close()


# ---- decode and check --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_decode_and_check_full_range_fields(case):
    """fields at 0 and 2B = q - 1 on every coefficient, in the stage sign patterns and at random, in records of 1, 2 and 5 rows:
    decode leaves cent(NTT(z)) (keys: z), check the same codes and no rows; a record with one field at q is refused alone"""
    spec, n = case
    B = X.half(spec)
    _, z = X.decoder_rows(spec, n)
    ctx = _ctx(spec, n)
    try:
        for coef in (True, False):
            for per in (1, 2, 5):
                rec = X.records_of(z, per)
                data, st = X.encoded(rec, B)
                assert not st.any()
                N = rec.shape[0]
                spoil = [(0, per * n - 1), (N - 1, 0), (N // 2, per * n // 2)]
                _decode_and_check(ctx, data, X.decoded(spec, n, rec, coef), per, n, coef, B, spoil)
    finally:
        ctx.close()


# ---- the width sweep ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SWEEP_CASES, ids=_cid)
def test_every_field_width(case):
    """every w in 2 .. 32 the modulus admits, at the smallest and the largest bound of that width, with 1, 2 and 5 records of 1
    row (and of 3 at degree 64: for odd w an odd record count ends the stream 8 bytes into a 16-byte unit); field 0, the last
    field and one in the middle at 0 and at 2B.  Encode (keys on every context, the coefficient kinds where the tables are a
    root's), decode and check meet the spec and touch nothing past the stream, the rows or the status words."""
    spec, n = case
    ctx = _ctx(spec, n)
    seen = set()
    try:
        for w, B in X.SWEEP:
            if B > X.half(spec):
                continue
            seen.add(w)
            for R in X.sweep_shapes(n):
                z = X.edge_fields(B, 5, R, n, 100 * w + R) - B
                data, st = X.encoded(z, B)
                assert not st.any() and data.shape[1] == X.record_bytes(n, R, w)
                F = X.forward(spec, n, z)
                for sel in (slice(0, 1), slice(1, 3), slice(0, 5)):
                    N = sel.stop - sel.start
                    if n == 64 and R * w % 2 and N % 2:
                        assert (N * data.shape[1]) % 16 == 8
                    for coef in (False, True):
                        want = (F if coef else z)[sel]
                        _decode_and_check(ctx, data[sel], want, R, n, coef, B, [(N - 1, R * n - 1), (0, 0)][:N])
                        if not coef or spec[1] == "root":
                            got, st = run_encode(ctx, want, coef, B)
                            assert not st.any() and np.array_equal(got, data[sel]), (w, B, R, N, coef)
    finally:
        ctx.close()
    assert seen == set(range(2, X.width(X.half(spec)) + 1))


# ---- the per-record consumers' refusal -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", [("scheme", "root"), ("top", "root"), ("w32", "odd")], ids=X.sid)
def test_records_that_are_no_whole_units_are_refused(spec):
    """degree 64 with rows * w odd: 8-byte-ending records, which the consumers that walk one record's chunks do not take"""
    from fusion_hip import FusionHipError
    from fusion_hip._lib import FZ_E_UNSUPPORTED
    n = 64
    ctx = _ctx(spec, n)
    bufs = Bufs(ctx)
    try:
        dB = bufs.put(np.zeros(4096, dtype=np.uint8))
        dA = bufs.put(np.zeros((3, n), dtype=np.int32))
        dP, dV = bufs.put(np.zeros((3, n), dtype=np.int64)), bufs.put(np.full(8, WORD_POISON, dtype=np.int32))
        for l, B in ((1, 2), (3, 2), (1, X.half(spec) if X.width(X.half(spec)) % 2 else 2 ** 29)):
            rb = X.record_bytes(n, l, X.width(B))
            assert rb % 16 == 8
            msg = f"records of {rb} bytes: reading them record by record needs a multiple of 16"
            with pytest.raises(FusionHipError) as e:
                ctx.aggregate_encoded_async_dev(dB.ptr, dA.ptr, 0, 2, l, B, dP.ptr, 0)
            assert e.value.code == FZ_E_UNSUPPORTED and msg in str(e.value)
            with pytest.raises(FusionHipError) as e:
                ctx.verify_encoded_async_dev(dA.ptr, dB.ptr, 2, l, B, dA.ptr, 0, 0, dV.ptr)
            assert e.value.code == FZ_E_UNSUPPORTED and msg in str(e.value)
        ctx.synchronize()
        assert (dV.numpy() == WORD_POISON).all() and not dP.numpy().any()
    finally:
        bufs.free()
        ctx.close()


# ---- aggregation from the bytes ----------------------------------------------------------------------------------------------
def _agg_ls(n):
    """a tail only, and a chunk plus a tail (degree 64: l * w must be even)"""
    return (1, 5) if n == 256 else (2, 18)


def _agg_check(ctx, spec, n, pool, B, N, l, seed, masked):
    idx = np.arange(N) % pool.shape[0]
    data, st = X.encoded(pool, B)
    assert not st.any()
    alpha = X.multipliers(N, n, seed)
    skip = np.where(np.arange(N) % 3 == 0, 6, 0).astype(np.int32) if masked else None
    want = X.aggregate_partial(spec, n, pool[idx], alpha, skip)
    p, o = GA.run_entry(ctx, data[idx], alpha, skip, N, l, B, n, guard=GUARD)
    assert np.array_equal(p[0], want), (N, l, B, masked)
    assert np.array_equal(o[0], X.cent(want, X.modulus(spec))), (N, l, B, masked)
    assert (p[1] == 0x5a5a5a5a5a5a5a5a).all() and (o[1] == ROW_POISON).all()


@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_aggregate_encoded_full_range_fields_and_extreme_multipliers(case):
    """1, 5 and 67 records tiled from five distinct ones of the decoder-side rows at B = (q - 1) / 2, alpha_hat at the int32
    extremes and random, with and without a skip mask (N = 1 masked: every record skipped): the int64 partial and the centred
    aggregate; then random fields with 0 and 2B at both ends at the narrowest bound (w = 2) and at the widest again"""
    spec, n = case
    B = X.half(spec)
    _, z = X.decoder_rows(spec, n)
    ctx = _ctx(spec, n)
    try:
        for l in _agg_ls(n):
            pool = X.records_of(z, l, 5)
            for N in (1, 5, 67):
                for masked in (False, True):
                    _agg_check(ctx, spec, n, pool, B, N, l, N + l, masked)
        l = _agg_ls(n)[1]
        for bound in sorted({1, B}):
            pool = X.edge_fields(bound, 5, l, n, bound % 1000 + n) - bound
            _agg_check(ctx, spec, n, pool, bound, 5, l, 3, False)
    finally:
        ctx.close()


# ---- verification from the bytes ---------------------------------------------------------------------------------------------
def _verify_ls(n):
    """one chunk (the workgroup owns the record whatever the count), and five chunks: two workgroups per record, the context's
    shared area and the finish kernel while the records are few (degree 64: l * w must be even)"""
    return (1, 17) if n == 256 else (2, 66)


VERIFY_CASES = [(s, n, l, grid) for s, n in CASES for l in _verify_ls(n) for grid in ("few", "many")]


@pytest.mark.parametrize("case", VERIFY_CASES, ids=lambda c: f"{X.sid(c[0])}-d{c[1]}-l{c[2]}-{c[3]}")
def test_verify_encoded_full_range_fields_and_extreme_multipliers(case):
    """five distinct records of the decoder-side rows at B = (q - 1) / 2, A at the int32 extremes and random; "few": the five,
    "many": num_cu + 1 tiled from them (one workgroup per record).  The honest target in either int32 representative gives 0
    everywhere -- any wrong coefficient of any record would make a 3; every other record's target moved by one in a coefficient
    that walks over the positions gives 3 there alone; a field at q gives 6 whatever the target; the keyed form, vk and c_hat
    at the int32 extremes, with the right key half solved for in two records of three and left as it is in the third"""
    spec, n, l, grid = case
    q, B = X.modulus(spec), X.half(spec)
    w = X.width(B)
    _, z = X.decoder_rows(spec, n)
    pool = X.records_of(z, l, 5)
    N = 5 if grid == "few" else _num_cu() + 1
    chunks = -(-l * n // 1024)
    assert (min(-(-chunks // 4), max(2 * _num_cu() // N, 1)) > 1) == (grid == "few" and chunks > 4)
    idx = np.arange(N) % 5
    A = X.multipliers(l, n, l + n)
    data, st = X.encoded(pool, B)
    assert not st.any()
    data = data[idx]
    sums = X.verify_sums(spec, n, pool, A)[idx]
    ctx = _ctx(spec, n)
    try:
        run = lambda d, **kw: GV.run_entry(ctx, A, d, N, l, B, guard=GUARD, **kw).tolist()      # noqa: E731
        assert run(data, target=sums) == [0] * N
        # (a centred word t has another int32 representative only where |t| >= q - 2^31: everywhere below 2^31, hardly anywhere
        # near 2^32 -- there the run repeats the honest target)
        other = X.other_representative(sums, q)
        assert ((other != sums).any() or q > 2 ** 31 + 1) and X.verdicts(spec, sums, other).tolist() == [0] * N
        assert run(data, target=other) == [0] * N
        # every odd record's target one off in coefficient j: j walks over n / 2 .. positions per case, the other half of the
        # positions in the next context
        off = (X.SPECS.index(spec) % 2) * (n // 2) + (l % 2)
        moved = sums.copy()
        for i in range(1, N, 2):
            j = (off + i // 2) % n
            moved[i, j] += 1 if moved[i, j] < 0 else -1
        want = [3 if i % 2 else 0 for i in range(N)]
        assert X.verdicts(spec, sums, moved).tolist() == want
        assert run(data, target=moved) == want
        # one field at 2B + 1 = q in the first and the last record: 6, under the honest target and under a wrong one
        d2, codes = _spoil(data, B, l * n, [(0, l * n - 1), (N - 1, (l - 1) * n)])
        assert codes[0] == codes[N - 1] == 6 and 2 * B + 1 < 1 << w
        assert run(d2, target=sums) == [6 if c else 0 for c in codes]
        assert run(d2, target=moved) == [6 if c else v for c, v in zip(codes, want)]
        # the keyed form
        vk, ch = X.key_inputs(N, n, N + l)
        keep = np.arange(N) % 3 == 2
        vk = np.where(keep[:, None, None], vk, X.solve_right_key(spec, vk, ch, sums))
        want = X.verdicts(spec, sums, X.keyed_target(spec, vk, ch))
        assert not want[~keep].any() and (N < 3 or want[keep].all())
        assert run(data, vk=vk, c_hat=ch) == want.tolist()
    finally:
        ctx.close()


@pytest.mark.parametrize("case", SWEEP_CASES, ids=_cid)
def test_every_field_width_in_the_per_record_consumers(case):
    """aggregate_encoded and verify_encoded unpack with instantiations of their own: every width the modulus admits at its
    smallest and largest bound, three records of 1 row (degree 64: of 2, so that rows * w is even), field 0, the last field
    and one in the middle at 0 and at 2B -- the partial and the aggregate, the honest target (0), the last record's target
    one off (3), and a field at 2B + 1 in the first record (6)"""
    spec, n = case
    q = X.modulus(spec)
    l, N = (2 if n == 64 else 1), 3
    ctx = _ctx(spec, n)
    try:
        for w, B in X.SWEEP:
            if B > X.half(spec):
                continue
            z = X.edge_fields(B, N, l, n, 200 * w + n) - B
            data, st = X.encoded(z, B)
            assert not st.any() and data.shape[1] % 16 == 0
            alpha, A = X.multipliers(N, n, w), X.multipliers(l, n, w + 1)
            want = X.aggregate_partial(spec, n, z, alpha)
            p, o = GA.run_entry(ctx, data, alpha, None, N, l, B, n, guard=GUARD)
            assert np.array_equal(p[0], want) and np.array_equal(o[0], X.cent(want, q)), (w, B)
            assert (p[1] == 0x5a5a5a5a5a5a5a5a).all() and (o[1] == ROW_POISON).all()
            sums = X.verify_sums(spec, n, z, A)
            assert GV.run_entry(ctx, A, data, N, l, B, target=sums, guard=GUARD).tolist() == [0] * N, (w, B)
            moved = sums.copy()
            j = (7 * w + B) % n
            moved[N - 1, j] += 1 if moved[N - 1, j] < 0 else -1
            d2, codes = _spoil(data, B, l * n, [(0, l * n - 1)])
            assert codes.tolist() == [6, 0, 0]
            assert GV.run_entry(ctx, A, d2, N, l, B, target=moved, guard=GUARD).tolist() == [6, 0, 3], (w, B)
    finally:
        ctx.close()


def test_the_moved_coefficient_walks_over_every_position():
    """the positions the cases above move, taken together: all of them at both degrees"""
    for n in X.DEGREES:
        seen = set()
        for s in X.SPECS:
            for l in _verify_ls(n):
                off = (X.SPECS.index(s) % 2) * (n // 2) + (l % 2)
                seen |= {(off + i // 2) % n for i in range(1, _num_cu() + 1, 2)}
        assert seen == set(range(n))
