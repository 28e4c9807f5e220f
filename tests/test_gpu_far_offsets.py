"""Operands past 4 GiB on the device: every case of tests/_far.py CASES, two checks each.

SAMPLED ROWS: the rows of the case's sample set (first, last, both sides of every crossed threshold, and their alias rows at byte
offset - 2^32, element index - 2^31 and - 2^32) against the C oracle on the same synthetic stream, bit for bit.  The output is
filled with another stream (the poison) before the call, or is an input the result differs from.  An alias row must hold its own
result: not the result of the row that a wrapped offset would have sent there, and not poison.

ALL ROWS, BY BASE SHIFT: the same entry is called on pieces of at most 0x70000000 bytes, each at a shifted base pointer, on
inputs that fz_fill_synthetic wrote piece by piece under the shifted seed (no offset inside a piece reaches 2^31 bytes, no piece
boundary falls on a threshold; these are sizes the rest of the suite pins against the oracle).  Piece result minus the whole
call's rows, on the device, reduced per row with fz_norm_weight to "all zero": the pattern of
test_gpu_fullsize.py::test_config2_sweep_maximum_2_22_rows.

No host array of an operand's size exists at any time, except for the wide path, whose entries take host arrays; at most one far operand set is alive at a time; every test frees what it
allocated (FZ_POOL_MB=0: a freed block goes back to the runtime) and skips only when the device lacks the memory it states."""
import numpy as np
import pytest

from oracle import oracle as O

import _far as F

pytestmark = pytest.mark.gpu

SEEDS = (0x5EED0001, 0x5EED0002)
POISON = 0x0BAD5EED
GIB = 1 << 30
PIECE = F.PIECE_BYTES


def _params(case):
    return O.PARAMS[256 if case.degree == 256 else 128]


def _need(nbytes):
    """skip unless the device has nbytes free (plus 1 GiB for the runtime and the reduction arrays)"""
    import torch
    free, _total = torch.cuda.mem_get_info()
    if free < nbytes + GIB:
        pytest.skip("needs %.1f GiB of free device memory, %.1f GiB are free" % ((nbytes + GIB) / GIB, free / GIB))


def _context(case, monkeypatch):
    """a fresh context: the route's knobs are read at creation"""
    import fusion_hip
    for k, v in case.route.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("FZ_POOL_MB", "0")
    P = _params(case)
    return fusion_hip.Context(P["q"], P["d"], P["root"], P["inv_root"])


class Bufs:
    def __init__(self, ctx):
        self.ctx, self.bufs = ctx, []

    def new(self, nbytes):
        import fusion_hip
        b = fusion_hip.DeviceBuffer(self.ctx, nbytes)
        self.bufs.append(b)
        return b

    def put(self, arr):
        import fusion_hip
        b = fusion_hip.DeviceBuffer.from_numpy(self.ctx, np.ascontiguousarray(arr))
        self.bufs.append(b)
        return b

    def close(self):
        for b in self.bufs:
            b.free()
        self.ctx.pool_trim(0)
        self.ctx.close()


def _read(ctx, ptr, first_elem, shape):
    got = np.empty(shape, np.int32)
    ctx.d2h(got, ptr + first_elem * 4)
    return got


class AllZero:
    """is a run of centred int32 on the device zero everywhere?  fz_norm_weight per row of `degree` values (a centred value is
    nonzero exactly when it counts towards its row's weight), then fz_norm_weight over the weights themselves, so that only one
    word per degree^2 values comes back to the host.  At most max_rows rows per call."""

    def __init__(self, ctx, bufs, degree, max_rows):
        import fusion_hip
        self.ctx, self.d, self.sub = ctx, degree, fusion_hip.OP_SUB
        self.cap = -(-max_rows // degree)                                        # rows of weights
        self.dm, self.dw = bufs.new(max(max_rows, self.cap) * 8), bufs.new(self.cap * degree * 4)
        self.dw2 = bufs.new(self.cap * 4)

    def __call__(self, ptr, rows):
        ctx, d = self.ctx, self.d
        top = -(-rows // d)
        ctx.pw_dev(self.sub, self.dw.ptr, self.dw.ptr, self.dw.ptr, top * d)     # x - x: the last row of weights ends in zeros
        ctx.norm_weight_dev(ptr, rows, self.dm.ptr, self.dw.ptr)
        ctx.norm_weight_dev(self.dw.ptr, top, self.dm.ptr, self.dw2.ptr)
        w = np.empty(top, np.int32)
        ctx.d2h(w, self.dw2.ptr)
        return not w.any()


def _run_stream(ctx, bufs, case, in_units, out_unit, over, call, expect, side_unit=0, in_place=False):
    """one streaming case.  Inputs i = stream SEEDS[i] with in_units[i] elements per row; the output has out_unit elements per row
    and overwrites input `over` (None: a buffer of its own, poisoned).  call(in_ptrs, out_ptr, rows) launches the entry,
    expect(in_arrays) -> the oracle's output rows for input rows [(n, unit), ...].  side_unit > 0: the entry has a second,
    poisoned output of that many elements per row; call(in_ptrs, out_ptr, rows, side_ptr) and expect -> (rows, side rows).
    in_place: the piecewise pass runs over the far input itself, so the peak is the two far buffers and the reduction arrays."""
    import fusion_hip
    rows, d = case.rows, case.degree
    ins = [bufs.new(rows * u * 4) for u in in_units]
    for b, u, s in zip(ins, in_units, SEEDS):
        ctx.fill_synthetic_dev(b.ptr, rows * u, s)
    if over is None:
        out = bufs.new(rows * out_unit * 4)
        ctx.fill_synthetic_dev(out.ptr, rows * out_unit, POISON)
    else:
        assert in_units[over] == out_unit
        out = ins[over]
    outs, units = [out], [out_unit]
    if side_unit:
        outs.append(bufs.new(rows * side_unit * 4))
        units.append(side_unit)
        ctx.fill_synthetic_dev(outs[1].ptr, rows * side_unit, POISON + 1)
    call([b.ptr for b in ins], out.ptr, rows, *[o.ptr for o in outs[1:]])         # THE far call
    # (1) sampled rows against the oracle
    for first, n in F.windows(case):
        xs = [F.stream_run(s, first * u, n * u).reshape(n, u) for u, s in zip(in_units, SEEDS)]
        wants = expect(xs)
        for o, u, want in zip(outs, units, wants if side_unit else [wants]):
            got = _read(ctx, o.ptr, first * u, (n, u))
            bad = np.flatnonzero((got != np.asarray(want).reshape(n, u)).any(axis=1))
            assert bad.size == 0, "%s: rows %s of the window at row %d differ from the oracle" % (case.name, (first + bad[:8]).tolist(), first)
    # (2) all rows: the entry on pieces at shifted bases
    if in_place:                                # ... over the input itself (one input, one output of its shape): no piece buffers
        assert over is None and not side_unit and in_units == [out_unit]
        per = PIECE // (out_unit * 4)
        per -= per % 4
        zero = AllZero(ctx, bufs, d, per * out_unit // d)
        for first in range(0, rows, per):
            n, at = min(per, rows - first), ins[0].ptr + first * out_unit * 4
            call([at], at, n)
            ctx.pw_dev(fusion_hip.OP_SUB, at, out.ptr + first * out_unit * 4, at, n * out_unit)
            whole, tail = divmod(n * out_unit, d)                                 # (a ragged end: fewer than d values, read back)
            assert zero(at, whole), "%s: the whole call and the piece at row %d differ somewhere" % (case.name, first)
            assert not _read(ctx, at, whole * d, (tail,)).any(), "%s: the whole call's last values differ" % case.name
        return
    # ... from inputs made piece by piece
    per = PIECE // (max(in_units + units) * 4)
    per -= per % 4                                                                # (16-byte aligned pieces at one element per row)
    tin = [bufs.new(per * u * 4) for u in in_units]
    touts = [tin[over] if over is not None else bufs.new(per * out_unit * 4)] + [bufs.new(per * u * 4) for u in units[1:]]
    assert all(per * u % d == 0 for u in units)
    zero = AllZero(ctx, bufs, d, per * max(units) // d)
    for first in range(0, rows, per):
        n = min(per, rows - first)
        for t, u in zip(touts, units):
            if n * u % d:                                                         # a ragged last piece: the reduction's last row ends in zeros
                ctx.pw_dev(fusion_hip.OP_SUB, t.ptr, t.ptr, t.ptr, per * u)
        for b, u, s in zip(tin, in_units, SEEDS):
            ctx.fill_synthetic_dev(b.ptr, n * u, F.shifted_seed(s, first * u))
        call([b.ptr for b in tin], touts[0].ptr, n, *[t.ptr for t in touts[1:]])
        for t, o, u in zip(touts, outs, units):
            ctx.pw_dev(fusion_hip.OP_SUB, t.ptr, o.ptr + first * u * 4, t.ptr, n * u)
            assert zero(t.ptr, -(-n * u // d)), "%s: the whole call and the piece at row %d differ somewhere" % (case.name, first)


# ---- transforms ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ntt_forward16_d256", "ntt_inverse16_d256", "ntt_forward16_d64", "ntt_inverse16_d64"])
def test_transform16_past_t1_t2_t3(name, coracle, monkeypatch):
    """16-per-lane schedule, 2^32 elements + 3 rows (16 GiB in, 16 GiB out): chunk_load_lds / chunk_load / chunk_store[_whole]'s
    scalar base + 32-bit lane offset at every threshold.  The piecewise pass runs in place over the input.  Peak device memory:
    2 x 16 GiB + 16 bytes per piece row."""
    _transform(F.CASE[name], coracle, monkeypatch)


@pytest.mark.parametrize("name", ["ntt_forward16_d256_t1", "ntt_inverse16_d256_t1", "ntt_forward16_d64_t1", "ntt_inverse16_d64_t1"])
def test_transform16_past_t1(name, coracle, monkeypatch):
    """the quick half of test_transform16_past_t1_t2_t3: 2^30 elements + 3 rows (4 GiB in, 4 GiB out).  Peak device memory:
    2 x 4 GiB + 16 bytes per piece row."""
    _transform(F.CASE[name], coracle, monkeypatch)


@pytest.mark.parametrize("name", ["ntt_forward4_d256", "ntt_inverse4_d256"])
def test_transform4_past_t1(name, coracle, monkeypatch):
    """radix-4 schedule, 2^22 + 3 rows of degree 256 (4 GiB in, 4 GiB out; its waves1 cap of 2^31 - 1 is 2 TiB away).  Peak
    device memory: 2 x 4 GiB + 16 bytes per piece row."""
    _transform(F.CASE[name], coracle, monkeypatch)


def _transform(case, coracle, monkeypatch):
    P, d = _params(case), case.degree
    inverse = "inverse" in case.name
    _need(2 * F.nbytes(case))
    ctx = _context(case, monkeypatch)
    bufs = Bufs(ctx)
    try:
        fn = ctx.ntt_inverse_dev if inverse else ctx.ntt_forward_dev
        ref = (lambda x: coracle.ntt_inverse(x[0], P["q"], P["inv_root"])) if inverse else (lambda x: coracle.ntt_forward(x[0], P["q"], P["root"]))
        _run_stream(ctx, bufs, case, [d], d, None, lambda i, o, n: fn(i[0], o, n), ref, in_place=True)
    finally:
        bufs.close()


@pytest.mark.parametrize("name", ["ntt_multi_planned", "ntt_multi_table_order"])
def test_ntt_multi_one_far_job_beside_a_small_one(name, coracle, monkeypatch):
    """fz_ntt_multi: job 0 forward over 2^22 + 3 rows (4 GiB in, 4 GiB out), job 1 inverse over 96 rows, one dispatch, under both
    FZ_MULTI_ORDER settings; the pieces are plain forward transforms, in place over the input.  Peak device memory: 2 x 4 GiB."""
    case = F.CASE[name]
    P, d = _params(case), case.degree
    _need(2 * F.nbytes(case))
    ctx = _context(case, monkeypatch)
    bufs = Bufs(ctx)
    try:
        small = O.splitmix_centered(77, 96 * d).reshape(96, d)
        ds_in, ds_out = bufs.put(small), bufs.put(np.full((96, d), 0x5A5A5A5A, np.int32))

        def call(i, o, n):
            if n == case.rows:
                ctx.ntt_multi_dev([(i[0], o, n, False), (ds_in.ptr, ds_out.ptr, 96, True)])
            else:
                ctx.ntt_forward_dev(i[0], o, n)
        _run_stream(ctx, bufs, case, [d], d, None, call, lambda x: coracle.ntt_forward(x[0], P["q"], P["root"]), in_place=True)
        assert np.array_equal(ds_out.to_numpy(np.int32, (96, d)), coracle.ntt_inverse(small, P["q"], P["inv_root"]).reshape(96, d))
    finally:
        bufs.close()


@pytest.mark.parametrize("name", ["poly_mul_radix4", "poly_mul_16"])
def test_poly_mul_past_t1(name, coracle, monkeypatch):
    """fz_poly_mul in both FZ_POLYMUL_FORMs, 2^22 + 3 products of degree 256, the product written over g.  Peak device memory:
    2 x 4 GiB + two pieces (3.5 GiB)."""
    case = F.CASE[name]
    P, d = _params(case), case.degree
    q = P["q"]
    _need(2 * F.nbytes(case) + 2 * PIECE)
    ctx = _context(case, monkeypatch)
    bufs = Bufs(ctx)
    try:
        def ref(x):
            return coracle.ntt_inverse(coracle.pw_mul(coracle.ntt_forward(x[0], q, P["root"]), coracle.ntt_forward(x[1], q, P["root"]), q), q, P["inv_root"])
        _run_stream(ctx, bufs, case, [d, d], d, 1, lambda i, o, n: ctx.poly_mul_dev(i[0], i[1], o, n), ref)
    finally:
        bufs.close()


# ---- pointwise ---------------------------------------------------------------------------------------------------------------------
def test_fill_synthetic_past_t1_t2_t3(monkeypatch):
    """fz_fill_synthetic over 2^32 + 1027 values (16 GiB): the samples on both sides of every threshold against the indexable
    stream AND against oracle.splitmix_centered under the shifted seed; all values against fills of pieces.  Peak device memory:
    16 GiB + one piece (1.75 GiB)."""
    _fill(F.CASE["fill_synthetic"], monkeypatch)


def test_fill_synthetic_past_t1(monkeypatch):
    """the quick half: 2^30 + 1027 values (4 GiB).  Peak device memory: 4 GiB + one piece (1.75 GiB)."""
    _fill(F.CASE["fill_synthetic_t1"], monkeypatch)


def test_fill_synthetic_of_exactly_2_32_values(monkeypatch):
    """2^32 values are 2^24 workgroups of 256 threads: exactly 2^32 threads, which the runtime refuses ("invalid configuration
    argument") -- the flat grid of the streaming kernels ends below that and the grid-stride loop walks the rest
    (fz_stream_dev.h grid_for).  Both ends and both sides of 2^31 elements against the stream.  Peak device memory: 16 GiB."""
    case = F.CASE["fill_synthetic"]
    count = 1 << 32
    _need(count * 4)
    ctx = _context(case, monkeypatch)
    bufs = Bufs(ctx)
    try:
        out = bufs.new(count * 4)
        ctx.fill_synthetic_dev(out.ptr, count, SEEDS[0])
        for first in (0, (1 << 30) - 2048, (1 << 31) - 2048, count - 4096):
            assert np.array_equal(_read(ctx, out.ptr, first, (4096,)), F.stream_run(SEEDS[0], first, 4096)), first
    finally:
        bufs.close()


def _fill(case, monkeypatch):
    import fusion_hip
    count, d = case.rows, case.degree
    _need(F.nbytes(case) + PIECE)
    ctx = _context(case, monkeypatch)
    bufs = Bufs(ctx)
    try:
        out = bufs.new(count * 4)
        ctx.fill_synthetic_dev(out.ptr, count, SEEDS[0])
        for first, n in F.windows(case):
            got = _read(ctx, out.ptr, first, (n,))
            assert np.array_equal(got, F.stream_run(SEEDS[0], first, n)), first
            assert np.array_equal(got, O.splitmix_centered(F.shifted_seed(SEEDS[0], first), n)), first
        per = PIECE // 4
        tmp = bufs.new(per * 4)
        zero = AllZero(ctx, bufs, d, per // d)
        for first in range(0, count, per):
            n = min(per, count - first)
            if n % d:
                ctx.pw_dev(fusion_hip.OP_SUB, tmp.ptr, tmp.ptr, tmp.ptr, per)
            ctx.fill_synthetic_dev(tmp.ptr, n, F.shifted_seed(SEEDS[0], first))
            ctx.pw_dev(fusion_hip.OP_SUB, tmp.ptr, out.ptr + first * 4, tmp.ptr, n)
            assert zero(tmp.ptr, -(-n // d)), first
    finally:
        bufs.close()


@pytest.mark.parametrize("name", ["pw_mul", "pw_add", "pw_sub"])
def test_pw_binary_past_t1_t2_t3(name, coracle, monkeypatch):
    """fz_pw_mul / add / sub over 2^32 + 1027 values (a count that is no multiple of 4), the result written over b: b's own
    values are the poison (a * b, a + b and a - b all differ from b).  Peak device memory: 2 x 16 GiB + two pieces (3.5 GiB)."""
    _pw_binary(name, coracle, monkeypatch)


@pytest.mark.parametrize("name", ["pw_mul_t1", "pw_add_t1", "pw_sub_t1"])
def test_pw_binary_past_t1(name, coracle, monkeypatch):
    """the quick half of test_pw_binary_past_t1_t2_t3: 2^30 + 1027 values.  Peak device memory: 2 x 4 GiB + two pieces (3.5 GiB)."""
    _pw_binary(name, coracle, monkeypatch)


def _pw_binary(name, coracle, monkeypatch):
    import fusion_hip
    case = F.CASE[name]
    q = _params(case)["q"]
    op, ref = {"pw_mul": (fusion_hip.OP_MUL, coracle.pw_mul), "pw_add": (fusion_hip.OP_ADD, coracle.pw_add),
               "pw_sub": (fusion_hip.OP_SUB, coracle.pw_sub)}[name[:6]]
    _need(2 * F.nbytes(case) + 2 * PIECE)
    ctx = _context(case, monkeypatch)
    bufs = Bufs(ctx)
    try:
        _run_stream(ctx, bufs, case, [1, 1], 1, 1, lambda i, o, n: ctx.pw_dev(op, i[0], i[1], o, n), lambda x: ref(x[0], x[1], q))
    finally:
        bufs.close()


def test_pw_neg_past_t1_t2_t3(coracle, monkeypatch):
    """fz_pw_neg over 2^32 + 1027 values into a poisoned buffer; the piecewise pass runs in place over the input.  Peak device
    memory: 2 x 16 GiB + 16 bytes per 256 values of a piece."""
    _pw_neg(F.CASE["pw_neg"], coracle, monkeypatch)


def test_pw_neg_past_t1(coracle, monkeypatch):
    """the quick half: 2^30 + 1027 values.  Peak device memory: 2 x 4 GiB + 16 bytes per 256 values of a piece."""
    _pw_neg(F.CASE["pw_neg_t1"], coracle, monkeypatch)


def _pw_neg(case, coracle, monkeypatch):
    q = _params(case)["q"]
    _need(2 * F.nbytes(case))
    ctx = _context(case, monkeypatch)
    bufs = Bufs(ctx)
    try:
        _run_stream(ctx, bufs, case, [1], 1, None, lambda i, o, n: ctx.pw_neg_dev(i[0], o, n), lambda x: coracle.pw_neg(x[0], q), in_place=True)
    finally:
        bufs.close()


def test_pw_mulacc_past_t1(coracle, monkeypatch):
    """fz_pw_mulacc over 2^30 + 1027 values: acc += a * a (both factors are the one far input, so that two far buffers serve).
    Peak device memory: 2 x 4 GiB + two pieces (3.5 GiB)."""
    case = F.CASE["pw_mulacc"]
    q = _params(case)["q"]
    _need(2 * F.nbytes(case) + 2 * PIECE)
    ctx = _context(case, monkeypatch)
    bufs = Bufs(ctx)
    try:
        _run_stream(ctx, bufs, case, [1, 1], 1, 1, lambda i, o, n: ctx.pw_mulacc_dev(o, i[0], i[0], n),
                    lambda x: coracle.pw_mulacc(x[1], x[0], x[0], q))
    finally:
        bufs.close()


def test_pw_mul_bcast_past_t1(coracle, monkeypatch):
    """fz_pw_mul_bcast over 2^22 + 3 rows of degree 256 into a poisoned buffer; pieces in place over the input.  Peak device
    memory: 2 x 4 GiB."""
    case = F.CASE["pw_mul_bcast"]
    P, d = _params(case), case.degree
    _need(2 * F.nbytes(case) + 2 * PIECE)
    ctx = _context(case, monkeypatch)
    bufs = Bufs(ctx)
    try:
        s = O.splitmix_centered(31, d)
        ds = bufs.put(s)
        _run_stream(ctx, bufs, case, [d], d, None, lambda i, o, n: ctx.pw_mul_bcast_dev(i[0], ds.ptr, o, n),
                    lambda x: coracle.pw_mul(x[0], np.broadcast_to(s, x[0].shape), P["q"]), in_place=True)
    finally:
        bufs.close()


# ---- matvec, signing ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["matvec_sliced", "matvec_fp64"])
def test_matvec_s_past_t1(name, coracle, monkeypatch):
    """fz_matvec, l = 4, 2^20 + 3 products: S is 4 GiB + 12 KiB, out 1 GiB, on the sliced integer kernel (the default at this size)
    and on the fp64 grid-stride kernel.  Peak device memory: 4 GiB + 1 GiB + two pieces (1.75 GiB + 0.44 GiB)."""
    case = F.CASE[name]
    P, d, l = _params(case), case.degree, 4
    _need(F.nbytes(case) * 5 // 4 + 2 * PIECE)
    ctx = _context(case, monkeypatch)
    bufs = Bufs(ctx)
    try:
        A = O.splitmix_centered(41, l * d).reshape(l, d)
        dA = bufs.put(A)
        _run_stream(ctx, bufs, case, [l * d], d, None, lambda i, o, n: ctx.matvec_dev(dA.ptr, i[0], o, n, l),
                    lambda x: coracle.matvec(A, x[0].reshape(-1, l, d), P["q"]))
    finally:
        bufs.close()


def test_sign_core_sk_hat_past_t1(coracle, monkeypatch):
    """fz_sign_core, l = 4, 2^19 + 3 signers: sk_hat is 4 GiB + 24 KiB, c_hat 0.5 GiB, sig 2 GiB.  Peak device memory: 6.5 GiB +
    three pieces (1.75 + 0.22 + 0.88 GiB)."""
    case = F.CASE["sign_core"]
    P, d, l = _params(case), case.degree, 4
    _need(F.nbytes(case) * 13 // 8 + 2 * PIECE)
    ctx = _context(case, monkeypatch)
    bufs = Bufs(ctx)
    try:
        _run_stream(ctx, bufs, case, [2 * l * d, d], l * d, None, lambda i, o, n: ctx.sign_core_dev(i[0], i[1], o, n, l),
                    lambda x: coracle.sign_core(x[0].reshape(-1, 2, l, d), x[1], P["q"]))
    finally:
        bufs.close()


@pytest.mark.parametrize("name", ["keygen_core", "keygen_core_bcast"])
def test_keygen_sk_hat_out_past_t1(name, coracle, monkeypatch):
    """fz_keygen_core / fz_keygen_core_bcast (the fused launch), l = 4, 2^19 + 3 keys: sk_hat out is 4 GiB + 24 KiB, vk out 1 GiB;
    the coefficients in are 4 GiB (one row per secret row) or 1 GiB (one polynomial per key half).  Peak device memory: 9 GiB
    (6 GiB) + three pieces (1.75 + 1.75 + 0.44 GiB)."""
    case = F.CASE[name]
    P, d, l = _params(case), case.degree, 4
    bcast = name.endswith("bcast")
    _need(F.nbytes(case) * 9 // 4 + 2 * PIECE)
    ctx = _context(case, monkeypatch)
    bufs = Bufs(ctx)
    try:
        A = O.splitmix_centered(43, l * d).reshape(l, d)
        dA = bufs.put(A)
        fn = ctx.keygen_core_bcast_dev if bcast else ctx.keygen_core_dev

        def ref(x):
            coef = x[0].reshape(-1, 2, 1, d).repeat(l, axis=2) if bcast else x[0].reshape(-1, 2, l, d)
            return coracle.keygen_core(A, np.ascontiguousarray(coef), P["q"], P["root"])
        _run_stream(ctx, bufs, case, [2 * d if bcast else 2 * l * d], 2 * l * d, None, lambda i, o, n, vk: fn(dA.ptr, i[0], o, vk, n, l), ref,
                    side_unit=2 * d)
    finally:
        bufs.close()


# ---- compact bytes ---------------------------------------------------------------------------------------------------------------------
RECORD_CASES = {"rows": ("encode_records_rows", "decode_records_rows"),
                "bytes": ("encode_records_bytes", "decode_records_bytes", "check_records_bytes")}


def _pack_fields(u, w):
    """[fields] unsigned -> the record's bytes: w-bit fields, LSB first (no range check: a planted field may be above 2B)"""
    bits = ((np.asarray(u, dtype=np.int64)[:, None] >> np.arange(w, dtype=np.int64)) & 1).astype(np.uint8)
    return np.packbits(bits.reshape(-1), bitorder="little")


@pytest.mark.parametrize("crossing", ["rows", "bytes"])
def test_records_encode_check_decode_past_t1(crossing, monkeypatch):
    """fz_encode_records_async, fz_check_records_async and fz_decode_records_async on verification-key records (2 rows of degree
    256, 31-bit fields: 2048 bytes of int32 rows, 1984 bytes of record), with the int32 rows the smallest that cross 2^32 bytes
    (2^21 + 3 records; the bytes stay below) and with the bytes the smallest that cross (2 164 806 records; both cross).  A record
    over the bound (encode, status 4, bytes zeroed) and a field above 2B (check and decode, status 6, rows zeroed) are planted
    at record 3, two records below the threshold record, one above it and at the last but one: the status index and the zeroing
    run on both sides.  Sampled records against the numpy specification; ALL status words read back; all rows by decoding (then
    encoding) pieces at shifted bases.  Peak device memory: the rows (4 GiB / 4.13 GiB) + the bytes (3.88 GiB / 4 GiB) + one piece
    of rows (1.75 GiB) + the status words."""
    import fusion_hip
    from test_encoding_host import spec_pack
    names = RECORD_CASES[crossing]
    case = F.CASE[names[0]]
    # the rows come from the synthetic stream of a SMALLER modulus, so that they lie within a bound a value can exceed (at the
    # key kind's own bound, (q - 1) / 2, no centred value is out of range): |z| <= B = (QS - 1) / 2, fields of 31 bits as well
    QS = (1 << 30) + 3
    R, B = 2, (QS - 1) // 2
    w = (2 * B).bit_length()
    d, n = case.degree, case.rows
    rv, rb = R * d, R * d // 8 * w
    assert F.CASE[names[1]].rows == n and w == 31 and rb == 1984 and rv == 512
    views = [F.CASE["encode_records_rows"]._replace(rows=n), F.CASE["encode_records_bytes"]._replace(rows=n)]
    wins = sorted({r for v in views for lo, k in F.windows(v) for r in range(lo, lo + k)})
    thr = (F.T1_BYTES // (rv * 4)) if crossing == "rows" else F.T1_BYTES // rb
    planted = [3, thr - 2, thr + 1, n - 2]
    assert all(0 <= r < n for r in planted)
    _need(n * (rv * 4 + rb) + 2 * PIECE)
    ctx = _context(case, monkeypatch)
    bufs = Bufs(ctx)
    fctx = fusion_hip.Context(QS, d, 0, 0)                                       # ring-only: its fz_fill_synthetic draws mod QS
    try:
        rows, data, status = bufs.new(n * rv * 4), bufs.new(n * rb), bufs.new(n * 4)
        fctx.fill_synthetic_dev(rows.ptr, n * rv, SEEDS[0])
        fctx.synchronize()
        ctx.fill_synthetic_dev(data.ptr, n * rb // 4, POISON)
        ctx.fill_synthetic_dev(status.ptr, n, POISON)

        def stream_rec(r, k=1):
            return F.stream_run(SEEDS[0], r * rv, k * rv, q=QS).reshape(k, R, d)

        def read_bytes(r):
            got = np.empty(rb, np.uint8)
            ctx.d2h(got, data.ptr + r * rb)
            return got
        for r in planted:                                                        # one value over the bound
            ctx.h2d(rows.ptr + (r * rv + 77) * 4, np.array([B + 1], np.int32))
        ctx.encode_records_async_dev(rows.ptr, n, R, False, B, data.ptr, status.ptr)          # THE far encode
        want_st = np.zeros(n, np.int32)
        want_st[planted] = 4
        assert np.array_equal(status.to_numpy(np.int32, (n,)), want_st), "encode: status words"
        for r in sorted(set(wins) | set(planted)):
            want = np.zeros(rb, np.uint8) if r in planted else spec_pack(stream_rec(r), B, w)[0]
            assert np.array_equal(read_bytes(r), want), ("encode", r)
        # the planted records get their honest bytes and rows back, then a field above 2B each (2B + 1 = q fits 31 bits)
        for r in planted:
            z = stream_rec(r).reshape(-1).astype(np.int64)
            ctx.h2d(rows.ptr + (r * rv + 77) * 4, z[77:78].astype(np.int32))
            u = z + B
            u[200] = 2 * B + 1
            ctx.h2d(data.ptr + r * rb, _pack_fields(u, w))
        ctx.fill_synthetic_dev(status.ptr, n, POISON)
        ctx.check_records_async_dev(data.ptr, n, R, B, status.ptr)                                 # THE far check
        want_st[planted] = 6
        assert np.array_equal(status.to_numpy(np.int32, (n,)), want_st), "check: status words"
        # decode over the rows buffer, poisoned first; the honest rows come back from the stream, piece by piece
        ctx.fill_synthetic_dev(rows.ptr, n * rv, POISON)
        ctx.fill_synthetic_dev(status.ptr, n, POISON)
        ctx.decode_records_async_dev(data.ptr, n, R, False, B, rows.ptr, status.ptr)              # THE far decode
        assert np.array_equal(status.to_numpy(np.int32, (n,)), want_st), "decode: status words"
        for r in sorted(set(wins) | set(planted)):
            want = np.zeros((R, d), np.int32) if r in planted else stream_rec(r)[0]
            assert np.array_equal(_read(ctx, rows.ptr, r * rv, (R, d)), want), ("decode", r)
        for r in planted:                                                        # (the refused records' rows, for the all-rows pass)
            ctx.h2d(rows.ptr + r * rv * 4, stream_rec(r))
            ctx.h2d(data.ptr + r * rb, spec_pack(stream_rec(r), B, w)[0])
        per = PIECE // (rv * 4)
        tmp, tst = bufs.new(per * rv * 4), bufs.new(per * 4)
        zero = AllZero(ctx, bufs, d, per * R)
        for first in range(0, n, per):
            k = min(per, n - first)
            # the whole decode's rows are the stream's ...
            fctx.fill_synthetic_dev(tmp.ptr, k * rv, F.shifted_seed(SEEDS[0], first * rv))
            fctx.synchronize()
            ctx.pw_dev(fusion_hip.OP_SUB, tmp.ptr, rows.ptr + first * rv * 4, tmp.ptr, k * rv)
            assert zero(tmp.ptr, k * R), ("decode: all rows", first)
            # ... and the whole encode's bytes decode, piece by piece at a shifted base, to the stream's rows
            ctx.decode_records_async_dev(data.ptr + first * rb, k, R, False, B, tmp.ptr, tst.ptr)
            assert not tst.to_numpy(np.int32, (k,)).any()
            ctx.pw_dev(fusion_hip.OP_SUB, tmp.ptr, rows.ptr + first * rv * 4, tmp.ptr, k * rv)
            assert zero(tmp.ptr, k * R), ("encode: all bytes", first)
    finally:
        bufs.close()
        fctx.close()


def test_sign_encoded_sk_hat_past_t1(coracle, monkeypatch):
    """fz_sign_encoded_async, l = 3 (768 values per record: the chunk walk's last chunk is partial and its last workgroup has an
    idle wave), 699 054 signers: sk_hat is 4 GiB + 18 KiB, c_hat 0.67 GiB, the bytes 1.94 GiB at the widest bound ((q - 1) / 2,
    31-bit fields: every value of the stream is in range).  Sampled records against sign_core + the numpy packing; all records:
    the bytes decoded piece by piece at shifted bases equal fz_sign_core's rows on inputs made piece by piece.  Peak device
    memory: 6.6 GiB + four pieces (1.75 + 0.29 + 0.88 + 0.88 GiB)."""
    import fusion_hip
    from test_encoding_host import spec_pack
    case = F.CASE["sign_encoded"]
    P, d, l, n = _params(case), case.degree, 3, case.rows
    q, B = P["q"], (P["q"] - 1) // 2
    rv, w = l * d, (2 * B).bit_length()
    rb = rv // 8 * w
    assert case.unit == 2 * rv and w == 31 and rb % 16 == 0 and (n * rv) % F.CHUNK and -(-n * rv // F.CHUNK) % F.WAVES_PER_BLOCK
    _need(n * (2 * rv * 4 + d * 4 + rb) + 3 * PIECE)
    ctx = _context(case, monkeypatch)
    bufs = Bufs(ctx)
    try:
        sk, c, data, status = bufs.new(n * 2 * rv * 4), bufs.new(n * d * 4), bufs.new(n * rb), bufs.new(n * 4)
        ctx.fill_synthetic_dev(sk.ptr, n * 2 * rv, SEEDS[0])
        ctx.fill_synthetic_dev(c.ptr, n * d, SEEDS[1])
        ctx.fill_synthetic_dev(data.ptr, n * rb // 4, POISON)
        ctx.fill_synthetic_dev(status.ptr, n, POISON)
        ctx.sign_encoded_async_dev(sk.ptr, c.ptr, n, l, B, data.ptr, status.ptr)                  # THE far call
        assert not status.to_numpy(np.int32, (n,)).any()
        for first, k in F.windows(case):
            ks = F.stream_run(SEEDS[0], first * 2 * rv, k * 2 * rv).reshape(k, 2, l, d)
            cs = F.stream_run(SEEDS[1], first * d, k * d).reshape(k, d)
            z = coracle.ntt_inverse(coracle.sign_core(ks, cs, q).reshape(-1, d), q, P["inv_root"]).reshape(k, l, d)
            got = np.empty((k, rb), np.uint8)
            ctx.d2h(got, data.ptr + first * rb)
            assert np.array_equal(got, spec_pack(z, B, w)), first
        per = PIECE // (2 * rv * 4)
        tk, tc, ts, td, tst = bufs.new(per * 2 * rv * 4), bufs.new(per * d * 4), bufs.new(per * rv * 4), bufs.new(per * rv * 4), bufs.new(per * 4)
        zero = AllZero(ctx, bufs, d, per * l)
        for first in range(0, n, per):
            k = min(per, n - first)
            ctx.fill_synthetic_dev(tk.ptr, k * 2 * rv, F.shifted_seed(SEEDS[0], first * 2 * rv))
            ctx.fill_synthetic_dev(tc.ptr, k * d, F.shifted_seed(SEEDS[1], first * d))
            ctx.sign_core_dev(tk.ptr, tc.ptr, ts.ptr, k, l)
            ctx.decode_records_async_dev(data.ptr + first * rb, k, l, True, B, td.ptr, tst.ptr)
            assert not tst.to_numpy(np.int32, (k,)).any()
            ctx.pw_dev(fusion_hip.OP_SUB, td.ptr, ts.ptr, td.ptr, k * rv)
            assert zero(td.ptr, k * l), ("all records", first)
    finally:
        bufs.close()


def test_sample_secret_polys_out_past_t1(monkeypatch):
    """fz_sample_secret_polys_dev, degree 256, norm bound 52, 2^21 + 3 keys: the output [N][2][256] is 4 GiB + 6 KiB.  The sampled
    keys' seeds against random.Random (the reference's sampler, polynomials.py:436-467); all keys against calls on pieces of the
    seed list at shifted bases.  Peak device memory: 4 GiB + one piece (1.75 GiB)."""
    import random
    import fusion_hip
    case = F.CASE["sample_secret_polys"]
    P, d, n, bound = _params(case), case.degree, case.rows, 52
    _need(F.nbytes(case) + 2 * PIECE)
    ctx = _context(case, monkeypatch)
    bufs = Bufs(ctx)
    try:
        with np.errstate(over="ignore"):
            seeds = np.arange(1, n + 1, dtype=np.uint64) * np.uint64(F.GAMMA) >> np.uint64(1)          # distinct, below 2^63
        out = bufs.new(n * 2 * d * 4)
        ctx.fill_synthetic_dev(out.ptr, n * 2 * d, POISON)
        ctx.sample_secret_polys_dev(seeds, P["q"], d, bound, d, out.ptr)                           # THE far call
        for first, k in F.windows(case):
            got = _read(ctx, out.ptr, first * 2 * d, (k, 2, d))
            for i in range(k):
                for h in (0, 1):
                    rng = random.Random(int(seeds[first + i]) + h)
                    want = [(1 + rng.randrange(bound)) * (1 - 2 * rng.randrange(2)) for _ in range(d)]
                    assert got[i, h].tolist() == want, (first + i, h)
        per = PIECE // (2 * d * 4)
        tmp = bufs.new(per * 2 * d * 4)
        zero = AllZero(ctx, bufs, d, per * 2)
        for first in range(0, n, per):
            k = min(per, n - first)
            ctx.sample_secret_polys_dev(seeds[first:first + k], P["q"], d, bound, d, tmp.ptr)
            ctx.pw_dev(fusion_hip.OP_SUB, tmp.ptr, out.ptr + first * 2 * d * 4, tmp.ptr, k * 2 * d)
            assert zero(tmp.ptr, k * 2), ("all keys", first)
    finally:
        bufs.close()


# ---- int32-row aggregation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["aggregate_onepass", "aggregate_direct4"])
def test_aggregate_sig_past_t1(name, coracle, monkeypatch):
    """fz_aggregate_core, degree 256, l = 4, 2^20 + 3 signers: sig is 4 GiB + 12 KiB, alpha 1 GiB.  Sampled coefficient columns
    against the sum over ALL signers from the indexable stream (int64, reduced after every product); all columns against three
    part-aggregates at shifted bases (none reaches 2^31 bytes) summed with fz_pw_add.  Peak device memory: 5 GiB."""
    import fusion_hip
    case = F.CASE[name]
    P, d, l = _params(case), case.degree, 4
    q, N = P["q"], case.rows
    _need(F.nbytes(case) * 5 // 4)
    ctx = _context(case, monkeypatch)
    bufs = Bufs(ctx)
    try:
        sig, alpha = bufs.new(N * l * d * 4), bufs.new(N * d * 4)
        ctx.fill_synthetic_dev(sig.ptr, N * l * d, SEEDS[0])
        ctx.fill_synthetic_dev(alpha.ptr, N * d, SEEDS[1])
        out = bufs.put(np.full((l, d), 0x5A5A5A5A, np.int32))
        ctx.aggregate_core_dev(sig.ptr, alpha.ptr, out.ptr, N, l)                   # THE far call
        got = out.to_numpy(np.int32, (l, d))
        for k, j in ((0, 0), (0, 1), (1, 63), (2, 64), (3, 254), (3, 255), (1, 130)):
            assert got[k, j] == F.accumulate_column(case, SEEDS[0], SEEDS[1], k, j, l, q), (k, j)
        part, acc = bufs.new(l * d * 4), bufs.put(np.zeros((l, d), np.int32))
        per = -(-N // 3)
        assert per * l * d * 4 < 1 << 31
        for first in range(0, N, per):
            n = min(per, N - first)
            ctx.aggregate_core_dev(sig.ptr + first * l * d * 4, alpha.ptr + first * d * 4, part.ptr, n, l)
            ctx.pw_dev(fusion_hip.OP_ADD, acc.ptr, part.ptr, acc.ptr, l * d)
        assert np.array_equal(got, acc.to_numpy(np.int32, (l, d))), "the whole aggregate differs from the sum of its parts"
    finally:
        bufs.close()


def test_aggregate_encoded_bytes_past_t1(monkeypatch):
    """fz_aggregate_encoded_async, degree 256, l = 4, bound (q - 1) / 2 (31-bit fields, 3968 bytes per record), 1 082 405 signers:
    the bytes are 4 GiB + 9.5 KiB.  The bytes are made by fz_encode_records_async on pieces of the synthetic int32 rows (sizes
    the suite pins), so the aggregate is that of the rows.  The skip mask has set words at both ends, on both sides of the
    record that straddles 2^32 bytes, and a run of nine in front of it.  Sampled coefficient columns against the sum over ALL kept
    signers from the indexable stream (int64, reduced after every product); all columns against fz_aggregate_core on three pieces
    of the rows at shifted bases, the skipped signers' multipliers zeroed, summed with fz_pw_add.  Peak device memory: the bytes
    (4 GiB) + the rows (4.13 GiB) + the multipliers (1.03 GiB) + the skip words."""
    import fusion_hip
    case = F.CASE["aggregate_encoded"]
    P, d, l, N = _params(case), case.degree, 4, case.rows
    q, B = P["q"], (P["q"] - 1) // 2
    rv, w = l * d, (2 * B).bit_length()
    rb = rv // 8 * w
    assert rb == case.unit and N < 1 << 22
    _need(N * (rb + rv * 4 + d * 4 + 8))
    ctx = _context(case, monkeypatch)
    bufs = Bufs(ctx)
    try:
        rows, alpha, data, status = bufs.new(N * rv * 4), bufs.new(N * d * 4), bufs.new(N * rb), bufs.new(N * 4)
        ctx.fill_synthetic_dev(rows.ptr, N * rv, SEEDS[0])
        ctx.fill_synthetic_dev(alpha.ptr, N * d, SEEDS[1])
        per = PIECE // (rv * 4)
        for first in range(0, N, per):
            k = min(per, N - first)
            ctx.encode_records_async_dev(rows.ptr + first * rv * 4, k, l, True, B, data.ptr + first * rb, status.ptr + first * 4)
        assert not status.to_numpy(np.int32, (N,)).any()
        thr = F.T1_BYTES // rb
        skip = np.zeros(N, np.int32)
        skip[[1, thr - 1, thr + 2, N - 1] + list(range(thr - 14, thr - 5))] = 1
        dskip = bufs.put(skip)
        part, out = bufs.put(np.full(rv, -1, np.int64)), bufs.put(np.full((l, d), 0x5A5A5A5A, np.int32))
        ctx.aggregate_encoded_async_dev(data.ptr, alpha.ptr, dskip.ptr, N, l, B, part.ptr, out.ptr)        # THE far call
        got, p64 = out.to_numpy(np.int32, (l, d)), part.to_numpy(np.int64, (l, d))
        assert np.array_equal(((p64 + q // 2) % q - q // 2).astype(np.int32), got) and np.abs(p64).max() < N * (q // 2)
        view = F.CASE["aggregate_onepass"]._replace(rows=N)
        for kk, j in ((0, 0), (0, 1), (1, 63), (2, 64), (3, 254), (3, 255), (1, 130)):
            assert got[kk, j] == F.accumulate_column(view, SEEDS[0], SEEDS[1], kk, j, l, q, keep=skip == 0), (kk, j)
        for i in np.flatnonzero(skip):
            ctx.h2d(alpha.ptr + int(i) * d * 4, np.zeros(d, np.int32))
        tmp, acc = bufs.new(rv * 4), bufs.put(np.zeros((l, d), np.int32))
        for first in range(0, N, per):
            k = min(per, N - first)
            ctx.aggregate_core_dev(rows.ptr + first * rv * 4, alpha.ptr + first * d * 4, tmp.ptr, k, l)
            ctx.pw_dev(fusion_hip.OP_ADD, acc.ptr, tmp.ptr, acc.ptr, rv)
        assert np.array_equal(got, acc.to_numpy(np.int32, (l, d))), "the aggregate from the bytes differs from the aggregate of the rows"
    finally:
        bufs.close()


def test_verify_encoded_bytes_past_t1(coracle, monkeypatch):
    """fz_verify_encoded_async against given targets, degree 256, l = 4, bound (q - 1) / 2, 1 082 405 records: the bytes are 4 GiB +
    9.5 KiB (made by fz_encode_records_async on pieces of the synthetic rows), the targets fz_matvec's products of pieces of the
    rows.  Failing signers on both sides of the record that straddles 2^32 bytes and at both ends: a target off by one (verdict
    3) and a field above 2B (verdict 6).  EVERY verdict is read back.  Peak device memory: the bytes (4 GiB) + the rows (4.13 GiB)
    + the targets (1.03 GiB) + the verdicts."""
    case = F.CASE["verify_encoded"]
    P, d, l, N = _params(case), case.degree, 4, case.rows
    q, B = P["q"], (P["q"] - 1) // 2
    rv, w = l * d, (2 * B).bit_length()
    rb = rv // 8 * w
    assert rb == case.unit
    _need(N * (rb + rv * 4 + d * 4 + 8))
    ctx = _context(case, monkeypatch)
    bufs = Bufs(ctx)
    try:
        A = O.splitmix_centered(47, l * d).reshape(l, d)
        dA = bufs.put(A)
        rows, target, data, status = bufs.new(N * rv * 4), bufs.new(N * d * 4), bufs.new(N * rb), bufs.new(N * 4)
        ctx.fill_synthetic_dev(rows.ptr, N * rv, SEEDS[0])
        per = PIECE // (rv * 4)
        for first in range(0, N, per):
            k = min(per, N - first)
            ctx.encode_records_async_dev(rows.ptr + first * rv * 4, k, l, True, B, data.ptr + first * rb, status.ptr + first * 4)
            ctx.matvec_dev(dA.ptr, rows.ptr + first * rv * 4, target.ptr + first * d * 4, k, l)
        assert not status.to_numpy(np.int32, (N,)).any()
        thr = F.T1_BYTES // rb
        off_by_one, bad_field = [0, thr - 1, thr + 1, N - 1], [5, thr - 2, thr + 2]
        for i in off_by_one:
            t = _read(ctx, target.ptr, i * d + 9, (1,))
            ctx.h2d(target.ptr + (i * d + 9) * 4, t + (1 if t[0] < B else -1))
        for i in bad_field:
            x = F.stream_run(SEEDS[0], i * rv, rv).reshape(l, d)
            u = coracle.ntt_inverse(x, q, P["inv_root"]).reshape(-1).astype(np.int64) + B
            u[300] = 2 * B + 1
            ctx.h2d(data.ptr + i * rb, _pack_fields(u, w))
        ctx.fill_synthetic_dev(status.ptr, N, POISON)
        ctx.verify_encoded_async_dev(dA.ptr, data.ptr, N, l, B, target.ptr, None, None, status.ptr)     # THE far call
        want = np.zeros(N, np.int32)
        want[off_by_one], want[bad_field] = 3, 6
        got = status.to_numpy(np.int32, (N,))
        assert np.array_equal(got, want), np.flatnonzero(got != want)[:8].tolist()
    finally:
        bufs.close()


# ---- the wide path: entries that take HOST arrays ------------------------------------------------------------------------------------
def _wide_call(wc, fn, *args):
    from fusion_hip._lib import check
    check(wc._lib, fn(*args))


def test_wide_ntt_values_past_t1():
    """fz_wide_ntt_host, forward, length 256, modulus 2^61 - 1, 2^21 + 3 rows: 4 GiB + 6 KiB of int64 in and out.  The entry takes
    host arrays, so this test holds the operand on the host: 2 x 4 GiB of host memory (input filled in slices from the indexable
    host stream, output poisoned) + one piece's output (1.75 GiB); on the device the entry itself allocates 2 x 4 GiB.  Sampled
    rows (both ends: the first rows are the alias of the rows past 2^32 bytes) against the reference's loop on Python integers;
    all rows against the entry on slices of the input below 2^31 bytes each."""
    from ctypes import POINTER, c_int64
    from fusion_hip.wide import WideContext
    case = F.CASE["wide_ntt"]
    d, rows, q = case.degree, case.rows, F.WIDE_Q
    _need(2 * F.nbytes(case))
    tab = [int(v) for v in F.stream_run(3, 0, d).astype(np.int64) % q]
    wc = WideContext(q, d, tab, tab)
    x, out = np.empty(rows * d, np.int64), np.full(rows * d, 0x5A5A5A5A5A5A5A5A, np.int64)
    step = 1 << 24
    for lo in range(0, x.size, step):
        x[lo:lo + step] = F.wide_run(lo, min(step, x.size - lo))
    p64 = POINTER(c_int64)
    _wide_call(wc, wc._lib.fz_wide_ntt_host, wc.device, q, d, wc._tables[0], wc._n_inv, 0, x.ctypes.data_as(p64), out.ctypes.data_as(p64), rows)
    for first, n in F.windows(case):
        for r in range(first, first + n):
            assert out[r * d:(r + 1) * d].tolist() == O.py_ntt_forward([int(v) for v in F.wide_run(r * d, d)], q, tab), r
    for first, n in F.pieces(case):
        assert np.array_equal(wc.ntt_forward(x[first * d:(first + n) * d]), out[first * d:(first + n) * d]), first


def test_wide_pw_values_past_t1():
    """fz_wide_pw_host, multiplication, modulus 2^61 - 1, 2^29 + 1027 values (no multiple of 4): 4 GiB + 8 KiB of int64 per
    operand.  Host memory: 3 x 4 GiB (a, b = a shifted by 7 places in the stream, out poisoned) + one piece's output (1.75 GiB);
    on the device the entry allocates 3 x 4 GiB.  Sampled values against Python integers, all values against the entry on
    slices below 2^31 bytes each."""
    from ctypes import POINTER, c_int64
    from fusion_hip.wide import OP_MUL, WideContext
    case = F.CASE["wide_pw"]
    n, q = case.rows, F.WIDE_Q
    _need(3 * F.nbytes(case))
    wc = WideContext(q, case.degree)
    a, b, out = np.empty(n, np.int64), np.empty(n, np.int64), np.full(n, 0x5A5A5A5A5A5A5A5A, np.int64)
    step = 1 << 24
    for lo in range(0, n, step):
        k = min(step, n - lo)
        a[lo:lo + k], b[lo:lo + k] = F.wide_run(lo, k), F.wide_run(lo + 7, k)
    p64 = POINTER(c_int64)
    _wide_call(wc, wc._lib.fz_wide_pw_host, wc.device, q, OP_MUL, a.ctypes.data_as(p64), b.ctypes.data_as(p64), out.ctypes.data_as(p64), n)
    hw = (q - 1) // 2
    for first, k in F.windows(case):
        xs, ys = F.wide_run(first, k).tolist(), F.wide_run(first + 7, k).tolist()
        assert out[first:first + k].tolist() == [(u * v + hw) % q - hw for u, v in zip(xs, ys)], first
    for first, k in F.pieces(case):
        assert np.array_equal(wc.pw_mul(a[first:first + k], b[first:first + k]), out[first:first + k]), first
