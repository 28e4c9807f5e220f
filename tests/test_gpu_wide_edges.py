"""The generic int64 path (csrc/fz_wide.hip) on the device, at its modulus, product and row-walk edges.

Expectations are the plain Python-integer operations of tests/_wide_edges.py (the transforms: oracle.py's py_ntt_forward /
py_ntt_inverse); every comparison is exact.  The C entries are called directly and
- through tests/_guarded.py's run_case with its HostBackend: every operand the entry reads or writes through a host pointer sits
  between 16 KiB guards, once per fill; outputs must equal the expectation, guards and inputs must be unchanged, and both fills
  must leave the same outputs;
- after a DECOY: the same entry at the same sizes on other data, so that a device block recycled by hipMalloc holds another
  call's answer and a skipped store cannot compare equal (docs/HISTORY.md section R found that for the int32 rows).
The scaling factor of every inverse transform is the one the library's own face (WideContext) hands over.
The row walks are called without guards (two fills of 134 MB operands would be most of their time); they still run after a decoy."""
import random
from ctypes import POINTER, c_int32, c_int64, c_uint64

import numpy as np
import pytest

import _guarded as G
import _wide_edges as W
from oracle import oracle as O

pytestmark = pytest.mark.gpu

QS, IDS = list(W.MODULI.values()), list(W.MODULI)
QBIG = 2 ** 63 - 25
GOLD = np.uint64(0x9E3779B97F4A7C15)


@pytest.fixture(scope="module")
def lib():
    import fusion_hip
    return fusion_hip.load_library()


def i64(x):
    return np.ascontiguousarray(np.array(x, dtype=np.int64))


def ptr(a, t=c_int64):
    return None if a is None else a.ctypes.data_as(POINTER(t))


def other(a):
    """other data of the same shape and type (any bit pattern is a valid input of every entry)"""
    if a is None:
        return None
    return (np.ascontiguousarray(a).view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)[::-1] + (GOLD if a.dtype.itemsize == 8 else np.uint32(0x9E3779B9))).view(a.dtype).copy()


def n_inv_of_the_face(q, n):
    from fusion_hip.wide import WideContext
    return WideContext(q, n, [0] * n, [0] * n)._n_inv


def guarded(operands, entry, args):
    """entry(*args(p)) after a decoy, through run_case; args(p) -> the argument list with p[name] -> the placed arrays"""
    data = {op.name: op for op in operands}

    def call(p):
        decoy = {n: other(op.data) if op.role == "in" else np.empty_like(op.expect) for n, op in data.items()}
        return entry(*args(decoy)), entry(*args({n: pl.ptr for n, pl in p.items()}))
    rets = G.run_case(G.HostBackend(), operands, call)
    assert rets == [(0, 0), (0, 0)], rets


def pw(lib, q, op, a, b, expect):
    a, b = i64(a), None if b is None else i64(b)
    ops = [G.inp("a", a)] + ([] if b is None else [G.inp("b", b)]) + [G.out("out", i64(expect).reshape(a.shape))]
    guarded(ops, lib.fz_wide_pw_host, lambda p: (0, q, op, ptr(p["a"]), ptr(p.get("b")), ptr(p["out"]), a.size))


def ntt(lib, q, table, inverse, rows, expect, n_inv=None):
    rows, tab = i64(rows), np.array(table, dtype=np.uint64)
    n = tab.size
    assert rows.ndim == 2 and rows.shape[1] == n
    n_inv = n_inv_of_the_face(q, n) if n_inv is None else n_inv
    ops = [G.inp("table", tab), G.inp("in", rows), G.out("out", i64(expect).reshape(rows.shape))]
    guarded(ops, lib.fz_wide_ntt_host, lambda p: (0, q, n, ptr(p["table"], c_uint64), n_inv, inverse, ptr(p["in"]), ptr(p["out"]), rows.shape[0]))


def matvec(lib, q, A, S, expect):
    A, S = i64(A), i64(S)
    l, d = A.shape
    assert S.ndim == 3 and S.shape[1:] == (l, d)
    ops = [G.inp("A", A), G.inp("S", S), G.out("out", i64(expect).reshape(S.shape[0], d))]
    guarded(ops, lib.fz_wide_matvec_host, lambda p: (0, q, d, ptr(p["A"]), ptr(p["S"]), ptr(p["out"]), S.shape[0], l))


def norm_weight(lib, rows, mx, wt):
    rows = i64(rows)
    ops = [G.inp("rows", rows), G.out("mx", np.array(mx, dtype=np.uint64)), G.out("wt", np.array(wt, dtype=np.int32))]
    guarded(ops, lib.fz_wide_norm_weight_host, lambda p: (0, ptr(p["rows"]), rows.shape[0], rows.shape[1], ptr(p["mx"], c_uint64), ptr(p["wt"], c_int32)))


# ---- the event fixtures, at every modulus ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", QS, ids=IDS)
def test_event_fixtures_through_every_kernel(lib, q):
    """every case of _wide_edges.cases(q): each product / wadd / wsub / wcanon / wcent / negation fixture through the four pointwise
    operations, the length-2 transforms with the pair as (value, table entry), matvec with l = 1 and l = 2 and the first, middle
    and last element of a row of 5"""
    for c in W.cases(q):
        want = c.plain(q)
        try:
            if c.entry == "pw":
                pw(lib, q, c.op, c.a, c.b, want)
            elif c.entry == "ntt":
                ntt(lib, q, c.table, c.inverse, c.rows, want)
            else:
                matvec(lib, q, c.A, c.S, want)
        except AssertionError as e:
            raise AssertionError(f"{c.name}: {e}") from None


# ---- transforms ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 4, 256, 512, 1024])
@pytest.mark.parametrize("q", [2 ** 32 + 15, 2 ** 32 + 1, 3 * 2 ** 50 + 1, QBIG, 2 ** 63 - 1], ids=lambda q: W.NAME_OF[q])
def test_transforms_both_directions_one_to_three_rows(lib, q, n):
    """half below a wave (2, 4), half equal to the block (512), the first length that strides (1024); random tables and tables of 0, 1
    and q - 1; prime and composite moduli; rows with the extremes of the type"""
    rnd = random.Random(n + q % 1009)
    rows = [[rnd.randint(W.INT64_MIN, W.INT64_MAX) for _ in range(n)] for _ in range(3)]
    rows[1][0], rows[1][-1], rows[2][n // 2] = W.INT64_MIN, W.INT64_MAX, q - 1
    tables = {"random": [rnd.randrange(q) for _ in range(n)], "edge": [(0, 1, q - 1)[rnd.randrange(3)] for _ in range(n)]}
    for name, tab in tables.items():
        for inverse, plain in ((0, W.p_forward), (1, W.p_inverse)):
            want = [plain(r, q, tab) for r in rows]
            for k in (1, 2, 3):
                try:
                    ntt(lib, q, tab, inverse, rows[:k], want[:k])
                except AssertionError as e:
                    raise AssertionError(f"{name} table, inverse={inverse}, {k} row(s): {e}") from None


@pytest.mark.parametrize("q", [3, 2 ** 32 - 1, 2 ** 32 + 15, 3 * 2 ** 50 + 1, QBIG, 2 ** 63 - 1], ids=lambda q: W.NAME_OF[q])
def test_c_abi_reduces_the_table_and_the_scaling_factor_it_is_handed(lib, q):
    """table entries q, q + 1, 2^64 - 1 (and multiples of q above any residue) and n_inv >= q through the C ABI: the rows of the reduced values"""
    n = 8
    rnd = random.Random(q % 977)
    red = [rnd.randrange(q) for _ in range(n)]
    top = (W.M64 - 1) // q
    tab = [q, q + 1, W.M64 - 1] + [r + rnd.randint(1, top - 1) * q for r in red[3:]]
    red[:3] = [0, 1, (W.M64 - 1) % q]
    assert all(t >= q and t < W.M64 and t % q == r for t, r in zip(tab, red))
    rows = [[rnd.randrange(q) for _ in range(n)] for _ in range(2)]
    n_inv = W.scaling_factor(n, q)
    big = n_inv + (W.M64 - 1 - n_inv) // q * q
    assert big >= q and big % q == n_inv
    ntt(lib, q, tab, 0, rows, [W.p_forward(r, q, red) for r in rows])
    ntt(lib, q, red, 0, rows, [W.p_forward(r, q, red) for r in rows])
    want = [W.p_inverse(r, q, red) for r in rows]
    ntt(lib, q, tab, 1, rows, want, n_inv=big)
    ntt(lib, q, red, 1, rows, want, n_inv=n_inv)
    ntt(lib, q, red, 1, rows, want)                        # and the face's own factor is that one


# ---- norm and weight -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 255, 256, 257, 511, 700])
def test_norm_weight_positions_extremes_and_empty_rows(lib, d):
    """one element per thread and several; the maximum in the first slot, the last, thread 255's, and thread 0's second element
    (index 256); INT64_MIN (|x| = 2^63, an unsigned answer), INT64_MAX, -INT64_MAX; a full row, a zero row, rows with one value"""
    rnd = random.Random(d)
    positions = sorted({p for p in (0, d - 1, 255, 256) if p < d})
    rows = []
    for p in positions:
        for v in (W.INT64_MIN, W.INT64_MAX, -W.INT64_MAX, 5):
            r = [rnd.randint(-2 ** 40, 2 ** 40) if rnd.random() < 0.7 else 0 for _ in range(d)]
            r[p] = v
            rows.append(r)                                 # the maximum at p among other values (v = 5: among zeros and larger values)
            one = [0] * d
            one[p] = v
            rows.append(one)                               # one non-zero value, at p
    rows.append([rnd.choice((-1, 1)) * rnd.randint(1, 2 ** 62) for _ in range(d)])      # full: weight d
    rows.append([0] * d)
    rows.append([W.INT64_MAX] * d)
    rows += [[0] * d] * (-len(rows) % 3)
    for k in range(0, len(rows), 3):
        batch = rows[k:k + 3]
        mw = [W.p_norm_weight(r) for r in batch]
        norm_weight(lib, batch, [m for m, _ in mw], [w for _, w in mw])


# ---- matvec ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [3, 2 ** 32 + 1, QBIG, 2 ** 63 - 1], ids=lambda q: W.NAME_OF[q])
def test_matvec_every_product_the_largest(lib, q):
    """l = 1, 2, 7, 300 with every product (q - 1)^2 (the accumulator takes l additions of the same largest Montgomery product), d = 1,
    3, 48, one signature and five; the later signatures of a batch of five are random, so that an index error shows"""
    rnd = random.Random(q % 9973)
    for l in (1, 2, 7, 300):
        for d in (1, 3, 48):
            A = [[q - 1] * d for _ in range(l)]
            for batch in (1, 5):
                S = [[[q - 1] * d for _ in range(l)]] + [[[rnd.randint(W.INT64_MIN, W.INT64_MAX) for _ in range(d)] for _ in range(l)] for _ in range(batch - 1)]
                want = W.p_matvec(A, S, q)
                assert want[0] == [W.cent(l, q)] * d           # l (q - 1)^2 = l (mod q)
                try:
                    matvec(lib, q, A, S, want)
                except AssertionError as e:
                    raise AssertionError(f"l={l} d={d} batch={batch}: {e}") from None


# ---- row walks ---------------------------------------------------------------------------------------------------------------------
# The caps, read from csrc/fz_wide.hip: wide_ntt_kernel and wide_norm_weight_kernel are launched with min(batch, kWideMaxGrid = 2^20)
# workgroups, one row each per turn of `rowi += gridDim.x`; wide_pw_kernel and wide_matvec_kernel with min(ceil(count / 256), 65535)
# workgroups of 256 threads, one element each per turn of the grid-stride loop.  The shapes below are the smallest that take every
# loop into its second turn (3 or 5 elements past the cap).
WALK_ROWS = (1 << 20) + 3
WALK_COUNT = 65535 * 256 + 5
DISTINCT = 1021


def cycled(distinct, n):
    """n rows: the distinct rows (an array [DISTINCT][w]) over and over"""
    distinct = np.asarray(distinct)
    reps = -(-n // len(distinct))
    return np.ascontiguousarray(np.tile(distinct, (reps,) + (1,) * (distinct.ndim - 1))[:n])


def same(got, want, what):
    if not np.array_equal(got, want):
        i = int(np.flatnonzero(got.reshape(-1) != want.reshape(-1))[0])
        raise AssertionError(f"{what}: first difference at flat index {i} of {got.size}: got {got.reshape(-1)[i]}, expected {want.reshape(-1)[i]}")


def test_walk_transform_rows_beyond_the_grid(lib):
    """length 2, 2^20 + 3 rows: rows 2^20 .. 2^20 + 2 are the second turn of workgroups 0 .. 2"""
    q, n = QBIG, 2
    rnd = random.Random(1)
    tab = [rnd.randrange(q), rnd.randrange(q)]
    ctab = (c_uint64 * 2)(*tab)
    dist = [[rnd.randint(W.INT64_MIN, W.INT64_MAX) for _ in range(n)] for _ in range(DISTINCT)]
    x = cycled(i64(dist), WALK_ROWS)
    decoy = other(x)
    n_inv = n_inv_of_the_face(q, n)
    for inverse, plain in ((0, W.p_forward), (1, W.p_inverse)):
        want = cycled(i64([plain(r, q, tab) for r in dist]), WALK_ROWS)
        out = np.empty_like(x)
        assert lib.fz_wide_ntt_host(0, q, n, ctab, n_inv, inverse, ptr(decoy), ptr(out), WALK_ROWS) == 0, lib.fz_last_error()
        assert lib.fz_wide_ntt_host(0, q, n, ctab, n_inv, inverse, ptr(x), ptr(out), WALK_ROWS) == 0, lib.fz_last_error()
        same(out, want, f"transform walk, inverse={inverse}")


def test_walk_norm_weight_rows_beyond_the_grid(lib):
    """degree 3, 2^20 + 3 rows"""
    rnd = random.Random(2)
    dist = [[rnd.choice((0, rnd.randint(W.INT64_MIN, W.INT64_MAX))) for _ in range(3)] for _ in range(DISTINCT)]
    dist[5], dist[6] = [0, 0, 0], [0, W.INT64_MIN, 1]
    x = cycled(i64(dist), WALK_ROWS)
    mw = [W.p_norm_weight(r) for r in dist]
    want_mx = cycled(np.array([m for m, _ in mw], dtype=np.uint64), WALK_ROWS)
    want_wt = cycled(np.array([w for _, w in mw], dtype=np.int32), WALK_ROWS)
    mx, wt = np.empty(WALK_ROWS, dtype=np.uint64), np.empty(WALK_ROWS, dtype=np.int32)
    assert lib.fz_wide_norm_weight_host(0, ptr(other(x)), WALK_ROWS, 3, ptr(mx, c_uint64), ptr(wt, c_int32)) == 0, lib.fz_last_error()
    assert lib.fz_wide_norm_weight_host(0, ptr(x), WALK_ROWS, 3, ptr(mx, c_uint64), ptr(wt, c_int32)) == 0, lib.fz_last_error()
    same(mx, want_mx, "norm walk")
    same(wt, want_wt, "weight walk")


@pytest.mark.parametrize("op", [W.OP_ADD, W.OP_MUL], ids=["add", "mul"])
def test_walk_pointwise_elements_beyond_the_grid(lib, op):
    """65 535 * 256 + 5 elements: the last five are the second turn of threads 0 .. 4 (134 MB per operand: the loop's own cap)"""
    q = QBIG
    rnd = random.Random(3 + op)
    da = [rnd.randint(W.INT64_MIN, W.INT64_MAX) for _ in range(DISTINCT)]
    db = [rnd.randint(W.INT64_MIN, W.INT64_MAX) for _ in range(DISTINCT)]
    a, b = cycled(i64(da), WALK_COUNT), cycled(i64(db), WALK_COUNT)
    want = cycled(i64(W.p_pw(op, da, db, q)), WALK_COUNT)
    out = np.empty_like(a)
    assert lib.fz_wide_pw_host(0, q, op, ptr(a), ptr(a), ptr(out), WALK_COUNT) == 0, lib.fz_last_error()      # the decoy: a + a, a * a
    assert lib.fz_wide_pw_host(0, q, op, ptr(a), ptr(b), ptr(out), WALK_COUNT) == 0, lib.fz_last_error()
    same(out, want, "pointwise walk")


def test_walk_matvec_elements_beyond_the_grid(lib):
    """l = 1, d = 3, batch 5 592 322: 3 * batch = 65 535 * 256 + 6 elements"""
    q, d, batch = QBIG, 3, 5592322
    assert d * batch == 65535 * 256 + 6
    rnd = random.Random(4)
    A = [[rnd.randint(W.INT64_MIN, W.INT64_MAX) for _ in range(d)]]
    dist = [[rnd.randint(W.INT64_MIN, W.INT64_MAX) for _ in range(d)] for _ in range(DISTINCT)]
    S = cycled(i64(dist), batch)
    want = cycled(i64([W.p_matvec(A, [[r]], q)[0] for r in dist]), batch)
    out = np.empty_like(S)
    cA = i64(A)
    assert lib.fz_wide_matvec_host(0, q, d, ptr(other(cA)), ptr(S), ptr(out), batch, 1) == 0, lib.fz_last_error()      # the decoy: another A
    assert lib.fz_wide_matvec_host(0, q, d, ptr(cA), ptr(S), ptr(out), batch, 1) == 0, lib.fz_last_error()
    same(out, want, "matvec walk")


# ---- both contexts on narrow parameters ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 8, 64, 256, 1024, 4096])
@pytest.mark.parametrize("q", [65537, 2147465729, 2 ** 32 - 5, 2 ** 32 - 1], ids=lambda q: W.NAME_OF[q])
def test_the_int32_context_the_generic_context_and_the_model_agree(q, d):
    """one library, one answer: Context(tables=...) (the int32 kernels), WideContext (the generic kernels) and the Python-integer
    model on the same narrow modulus, length and random tables -- transforms both ways, + - *, the (1 x 3)(3 x 1) product, norm
    and weight; negation where the int32 face has a representative (q < 2^31).  On the composite 2^32 - 1 the inverse transforms
    agree only because both scale by n^(q-2) mod q."""
    import fusion_hip
    from fusion_hip.wide import WideContext
    rnd = random.Random(q % 4093 + d)
    h = (q - 1) // 2
    fwd, inv = [rnd.randrange(q) for _ in range(d)], [rnd.randrange(q) for _ in range(d)]
    rows = [[rnd.randint(-h, h) for _ in range(d)] for _ in range(3)]
    rows[0][0], rows[0][-1] = h, -h
    others = [[rnd.randint(-h, h) for _ in range(d)] for _ in range(3)]
    narrow = fusion_hip.Context(q, d, 0, 0, tables=(fwd, inv))
    try:
        wide = WideContext(q, d, fwd, inv)
        x32, y32 = np.array(rows, dtype=np.int32), np.array(others, dtype=np.int32)
        x64, y64 = x32.astype(np.int64), y32.astype(np.int64)

        def three(name, got32, got64, want):
            assert got64.dtype == np.int64 and got32.dtype == np.int32
            assert got64.tolist() == want, f"{name}: the generic context differs from the model"
            assert got32.astype(np.int64).tolist() == want, f"{name}: the int32 context differs from the model"
        three("forward", narrow.ntt_forward(x32), wide.ntt_forward(x64), [W.p_forward(r, q, fwd) for r in rows])
        three("inverse", narrow.ntt_inverse(x32), wide.ntt_inverse(x64), [W.p_inverse(r, q, inv) for r in rows])
        three("add", narrow.pw_add(x32, y32), wide.pw_add(x64, y64), [W.p_add(r, s, q) for r, s in zip(rows, others)])
        three("sub", narrow.pw_sub(x32, y32), wide.pw_sub(x64, y64), [W.p_sub(r, s, q) for r, s in zip(rows, others)])
        three("mul", narrow.pw_mul(x32, y32), wide.pw_mul(x64, y64), [W.p_mul(r, s, q) for r, s in zip(rows, others)])
        S = [rows, others]
        three("matvec", narrow.matvec(y32, np.array(S, dtype=np.int32)), wide.matvec(y64, np.array(S, dtype=np.int64)), W.p_matvec(others, S, q))
        assert wide.pw_neg(x64).tolist() == [W.p_neg(r, q) for r in rows]
        if q < 2 ** 31:
            assert narrow.pw_neg(x32).astype(np.int64).tolist() == [W.p_neg(r, q) for r in rows]
        rows[1] = [0] * d
        z = np.array(rows, dtype=np.int32)
        (m32, w32), (m64, w64) = narrow.norm_weight(z), wide.norm_weight(z.astype(np.int64))
        want = [W.p_norm_weight(r) for r in rows]
        assert [(int(m), int(w)) for m, w in zip(m32, w32)] == want == [(int(m), int(w)) for m, w in zip(m64, w64)]
    finally:
        narrow.close()


# ---- the drop-in classes at a narrow modulus and a long length ---------------------------------------------------------------------
def test_drop_in_classes_at_a_narrow_modulus_and_a_long_length():
    """q = 65537, d = 8192: the transforms and products run on the generic path (int64 rows), + - and negation on the ring context of
    the int32 path (the degree does not matter to it); results of either are operands of the other"""
    from algebra.polynomials import PolynomialCoefficientRepresentation as PC, transform
    q, d = 65537, 8192
    root = next(r for r in (pow(g, (q - 1) // (2 * d), q) for g in range(2, 100)) if pow(r, d, q) == q - 1)
    inv = pow(root, q - 2, q)
    rnd = random.Random(8192)
    h = q // 2
    f, g = [rnd.randint(-h, h) for _ in range(d)], [rnd.randint(-h, h) for _ in range(d)]
    sparse = [0] * d
    for pos, v in ((0, h), (4097, -1), (d - 1, -h)):
        sparse[pos] = v
    F, Gp, Sp = (PC(q, d, root, inv, 2 * d, list(v)) for v in (f, g, sparse))
    assert (F + Gp).coefficients == W.p_add(f, g, q)
    assert (F - Gp).coefficients == W.p_sub(f, g, q)
    assert (-F).coefficients == W.p_neg(f, q)
    school = [0] * d
    for pos, v in ((0, h), (4097, -1), (d - 1, -h)):           # f * sparse mod (X^d + 1), term by term
        for i, x in enumerate(f):
            k = i + pos
            school[k % d] += x * v if k < d else -x * v
    school = [W.cent(v, q) for v in school]
    prod = F * Sp
    assert prod.coefficients == school
    tw, itw = O.py_twiddles(root, q, d), O.py_twiddles(inv, q, d)
    Fh, Gh = transform(F), transform(Gp)
    fh, gh = W.p_forward(f, q, tw), W.p_forward(g, q, tw)
    assert Fh.values == fh and Gh.values == gh
    assert transform(Fh).coefficients == f == W.p_inverse(fh, q, itw)
    assert (Fh * Gh).values == W.p_mul(fh, gh, q)
    assert (Fh * transform(Sp)).values == W.p_forward(school, q, tw)          # the convolution theorem, through both paths
    # an int64 row of the generic path and an int32 row of the ring context as operands of one another (reading .coefficients or
    # .values turns an object's row into a list, so these are fresh results)
    prod, ring_sum = F * Sp, F + Gp
    assert prod._arr is not None and prod._arr.dtype == np.int64 and ring_sum._arr is not None and ring_sum._arr.dtype == np.int32
    mixed, back = prod + ring_sum, ring_sum - prod
    assert mixed.coefficients == W.p_add(school, W.p_add(f, g, q), q)
    assert back.coefficients == W.p_sub(W.p_add(f, g, q), school, q)
    wide_row, ring_row = transform(F), transform(F) + transform(Gp)
    assert wide_row._arr.dtype == np.int64 and ring_row._arr.dtype == np.int32
    assert (wide_row + ring_row).values == W.p_add(fh, W.p_add(fh, gh, q), q)
    assert (transform(F) * ring_row).values == W.p_mul(fh, W.p_add(fh, gh, q), q)
