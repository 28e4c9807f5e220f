"""Every transform family at the edge of the 4-op twiddle multiply (tests/_transform_edges.py): moduli on both sides of
`fast` (delta = K - q < 2^15, q < 2^31), tables of top and odd twiddles, and int32-extreme rows whose pure-add sums reach 2^38
at degree 128 and would reach 2^39 at degree 256 without the inverse kernels' folds.  Every row is compared with the
reference loops (oracle.py_ntt_forward / py_ntt_inverse on Python integers, the same tables):

- ntt_small (d <= 16); the radix-4 kernels under FZ_NTT_ROWS = 1 / 2 / 4, with 1-, 4- and 8-wave workgroups reached by the
  row count; the 16-per-lane kernels (FZ_NTT_KERNEL = 16, and degrees 32 / 128); ntt_multi with 4-, 8- and 32-entry job
  tables in its radix-4 (jobs4) and 16-per-lane (jobs16) forms; ntt_big at 512 and 4096;
- poly_mul under FZ_POLYMUL_FORM = 1 and 2, against the composition of the reference loops;
- the fused kernels whose inverse is fed by a lazily reduced product, polymul16 (and polymul_fused), with that product at
  +-(q - 1) / 2 on every coefficient; verify_fused, whose inverse takes the signature rows as they are, with int32-extreme
  rows and rows lifted by q (sums near 2^39, inverse c * e0) at the largest fast delta of a prime with roots, its verdicts at
  the exact norm and weight of each row."""
import functools
import os

import numpy as np
import pytest

from oracle import oracle as O

import _transform_edges as E

pytestmark = pytest.mark.gpu

SPECS = [(k, "odd") for k in E.TABLE_MODULI] + [("d32767", "q1"), ("k17", "q1"), ("scheme", "q1")] + \
    [(k, "root") for k in E.ROOT_MODULI]
# ntt_big (like ntt_small) has no 4-op form -- only the 6-op fz_mulmod, folding every sum -- so the threshold cannot move it:
# three moduli at 512 and 4096 keep its share of the Python reference loops small
BIG_SPECS = [("d32767", "odd"), ("p31", "odd"), ("q3", "odd")]


def _sid(s):
    return f"{s[0]}-{s[1]}"


def _ctx(spec, n, env=None):
    """a table context (fz_ctx_create_tables) for the top / odd tables; the primes of E.ROOT_MODULI through the ordinary root
    context, which builds its own tables from (root, inv_root) -- the ones E.root_tables lists for the reference loops"""
    import fusion_hip
    env = env or {}
    for k, v in env.items():
        os.environ[k] = v
    try:
        if spec[1] == "root":
            q, root, inv_root = E.root_of(spec[0], n)
            return fusion_hip.Context(q, n, root, inv_root)
        q, fwd, inv = E.tables(spec[0], n, spec[1])
        return fusion_hip.Context(q, n, 0, 0, tables=(fwd, inv))
    finally:
        for k in env:
            os.environ.pop(k, None)


@functools.lru_cache(maxsize=None)
def _fixture(spec, n):
    """(rows [R][n] int32, forward [R][n], inverse [R][n]) by the reference loops"""
    q, fwd, inv = E.tables(spec[0], n, spec[1])
    rows = E.few_rows(q, n) if n > 256 else E.rows(q, n)
    x = np.array([r for _, r in rows], dtype=np.int64)
    f = [O.py_ntt_forward([int(v) for v in r], q, fwd) for r in x]
    i = [O.py_ntt_inverse([int(v) for v in r], q, inv) for r in x]
    return x.astype(np.int32), np.array(f, dtype=np.int32), np.array(i, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def _product(spec, n):
    """(f, g, INTT(NTT(f) * NTT(g))): row i times row i + 1 of the fixture"""
    q, fwd, inv = E.tables(spec[0], n, spec[1])
    x, F, _ = _fixture(spec, n)
    g = np.roll(x, -1, axis=0)
    Fg = np.roll(F, -1, axis=0)
    want = [O.py_ntt_inverse(O.py_pw_mul([int(v) for v in a], [int(v) for v in b], q), q, inv) for a, b in zip(F, Fg)]
    return x, g, np.array(want, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def _num_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _tiled(a, rows):
    return np.ascontiguousarray(np.tile(a, (-(-rows // a.shape[0]), 1))[:rows])


# (id, degrees, env, rows): rows = None for the fixture rows alone, or a function of (degree, CUs) for the radix-4 workgroup
# shapes (nr = 1: 8 waves per workgroup from 8 waves per CU, 4 from 4, else 1; a wave holds 256 / degree rows)
FAMILIES = [
    ("small", (2, 4, 16), {}, None),
    ("r4-rows1-w1", (64, 256), {"FZ_NTT_KERNEL": "4", "FZ_NTT_ROWS": "1"}, None),
    ("r4-rows1-w4", (64, 256), {"FZ_NTT_KERNEL": "4", "FZ_NTT_ROWS": "1"}, lambda n, cu: 4 * cu * (256 // n)),
    ("r4-rows1-w8", (64, 256), {"FZ_NTT_KERNEL": "4", "FZ_NTT_ROWS": "1"}, lambda n, cu: 8 * cu * (256 // n) + 3),
    ("r4-rows2", (64, 256), {"FZ_NTT_KERNEL": "4", "FZ_NTT_ROWS": "2"}, lambda n, cu: 97),
    ("r4-rows4", (64, 256), {"FZ_NTT_KERNEL": "4", "FZ_NTT_ROWS": "4"}, lambda n, cu: 101),
    ("k16", (32, 64, 128, 256), {"FZ_NTT_KERNEL": "16"}, lambda n, cu: 4096 // n * 3 + 1),
]
CASES = [(f, n) for f in FAMILIES for n in f[1]]


@pytest.mark.parametrize("spec", SPECS, ids=_sid)
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0][0]}-d{c[1]}")
def test_transforms_at_the_edge(case, spec):
    (name, _, env, nrows), n = case
    x, F, I = _fixture(spec, n)
    rows = nrows(n, _num_cu()) if nrows else x.shape[0]
    ctx = _ctx(spec, n, env)
    try:
        xs = _tiled(x, rows)
        assert np.array_equal(ctx.ntt_forward(xs), _tiled(F, rows)), "forward"
        assert np.array_equal(ctx.ntt_inverse(xs), _tiled(I, rows)), "inverse"
    finally:
        ctx.close()


@pytest.mark.parametrize("spec", BIG_SPECS, ids=_sid)
@pytest.mark.parametrize("n", [512, 4096])
def test_big_transforms_at_the_edge(n, spec):
    x, F, I = _fixture(spec, n)
    ctx = _ctx(spec, n)
    try:
        assert np.array_equal(ctx.ntt_forward(x), F) and np.array_equal(ctx.ntt_inverse(x), I)
    finally:
        ctx.close()


@pytest.mark.parametrize("spec", SPECS, ids=_sid)
@pytest.mark.parametrize("jobs", [4, 8, 32])
@pytest.mark.parametrize("form", ["4", "16"])
@pytest.mark.parametrize("n", [64, 256])
def test_multi_job_transforms_at_the_edge(n, form, jobs, spec):
    """one fz_ntt_multi launch of `jobs` jobs (the 4-, 8- or 32-entry job table), forward and inverse alternating, every job
    the fixture rows (ragged: job j drops its last j % 3 rows)"""
    import fusion_hip
    x, F, I = _fixture(spec, n)
    ctx = _ctx(spec, n, {"FZ_NTT_KERNEL": form})
    bufs = []
    try:
        plan = []
        for j in range(jobs):
            r = x.shape[0] - j % 3
            src = fusion_hip.DeviceArray.from_numpy(ctx, np.ascontiguousarray(x[:r]))
            dst = fusion_hip.DeviceArray(ctx, (r, n))
            bufs += [src, dst]
            plan.append((src, dst, r, j % 2 == 1))
        ctx.ntt_multi_dev([(s.ptr, d.ptr, r, inv) for s, d, r, inv in plan])
        for j, (_, d, r, inv) in enumerate(plan):
            assert np.array_equal(d.numpy(), (I if inv else F)[:r]), (j, "inverse" if inv else "forward")
    finally:
        for b in bufs:
            b.free()
        ctx.close()


@pytest.mark.parametrize("spec", SPECS, ids=_sid)
@pytest.mark.parametrize("form,n", [("1", 64), ("1", 256), ("2", 32), ("2", 64), ("2", 128), ("2", 256)])
def test_poly_mul_at_the_edge(form, n, spec):
    f, g, want = _product(spec, n)
    ctx = _ctx(spec, n, {"FZ_POLYMUL_FORM": form})
    try:
        assert np.array_equal(ctx.poly_mul(f, g), want)
    finally:
        ctx.close()


def _half_patterns(q, n, root):
    """NTT-domain rows at +-(q - 1) / 2 on every coefficient: both constants and, where the tables are a root's (so that a
    coefficient row with that transform exists), the stage sign patterns with an odd sum"""
    h = (q - 1) // 2
    pats = [[h] * n, [-h] * n]
    if root:
        for _, row in E.rows(q, n)[6:]:
            p = [h if v > 0 else -h for v in row]
            p[0] -= 1 if p[0] > 0 else -1
            pats.append(p)
        pats.append([h] * (n - 1) + [h - 1])
    return pats


@pytest.mark.parametrize("spec", SPECS, ids=_sid)
@pytest.mark.parametrize("form,n", [("2", 32), ("2", 64), ("2", 128), ("2", 256), ("1", 64), ("1", 256)])
def test_fused_product_inverse_fed_at_half_q(form, n, spec):
    """f = 1 (transform: all ones, whatever the tables), g with transform P: the inverse inside the fused product takes
    P = +-(q - 1) / 2 at every coefficient (the largest lazily reduced product) and must return INTT(P)"""
    q, fwd, inv = E.tables(spec[0], n, spec[1])
    root = spec[1] == "root"
    pats = _half_patterns(q, n, root)
    if root:
        g = np.array([O.py_ntt_inverse(list(p), q, inv) for p in pats], dtype=np.int32)
    else:
        g = np.zeros((len(pats), n), np.int32)
        g[:, 0] = [p[0] for p in pats]                     # c * e0: its transform is c everywhere, for any table
    for p, r in zip(pats, g):
        assert O.py_ntt_forward([int(v) for v in r], q, fwd) == [E.cent(v, q) for v in p]
    f = np.zeros_like(g)
    f[:, 0] = 1
    want = np.array([O.py_ntt_inverse(list(p), q, inv) for p in pats], dtype=np.int32)
    ctx = _ctx(spec, n, {"FZ_POLYMUL_FORM": form})
    try:
        rows = 4096 // n * 4 + 1
        assert np.array_equal(ctx.poly_mul(_tiled(f, rows), _tiled(g, rows)), _tiled(want, rows))
    finally:
        ctx.close()


@pytest.mark.parametrize("env", [{}, {"FZ_VERIFY_CENT": "1"}], ids=lambda e: ",".join(e) or "defaults")
@pytest.mark.parametrize("name", ["r28159", "scheme"])
@pytest.mark.parametrize("n", [64, 256])
def test_verify_fused_inverse_at_the_edge(n, name, env):
    """verify_fused transforms each signature row as it is: an int32-extreme row reaches its inverse unreduced.  Per row (one
    group of one row), the verdict at beta = M - 1 / M and omega = W - 1 / W, M and W the exact norm and weight of the
    reference inverse: a transform off by one anywhere moves M or W and with it one of these verdicts"""
    import fusion_hip
    q, _, inv = E.tables(name, n, "root")
    ctx = _ctx((name, "root"), n, env)
    rng = np.random.default_rng(n)
    A = rng.integers(-1000, 1000, size=(1, n)).astype(np.int32)
    bufs = []
    try:
        dA = fusion_hip.DeviceArray.from_numpy(ctx, A)
        bufs.append(dA)
        for rname, row in E.rows(q, n) + E.lifted_rows(q, n):
            t = O.py_ntt_inverse([int(v) for v in row], q, inv)
            M, W = max(abs(v) for v in t), sum(1 for v in t if v)
            assert W >= 1
            target = np.array([O.py_pw_mul([int(v) for v in A[0]], [int(v) for v in row], q)], dtype=np.int32)
            dS = fusion_hip.DeviceArray.from_numpy(ctx, np.array([row], dtype=np.int32))
            dT = fusion_hip.DeviceArray.from_numpy(ctx, target)
            bufs += [dS, dT]
            got = [ctx.verify_with_target_batch_dev(dA.ptr, dS.ptr, dT.ptr, 1, 1, b, w)[0]
                   for b, w in ((M, W), (M - 1, W), (M, W - 1))]
            assert got == [0, 4, 5], (rname, M, W, got)
    finally:
        for b in bufs:
            b.free()
        ctx.close()
