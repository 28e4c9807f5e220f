"""The ordering rule of a multi-job transform launch (fz_multi_plan, through fz_diag_multi_order: host arithmetic only, no GPU):
the execution order is a permutation of the table, the jobs that read what the previous launch wrote come first -- the most
recently written first -- the others follow in table order, the jobs' runs of workgroups cover the grid exactly, and a table
that consumes nothing (or FZ_MULTI_ORDER=0) keeps table order."""
import ctypes

import pytest

J = 4 << 20


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    import fusion_hip
    return fusion_hip.load_library()


def plan(lib, table, prev, degree=256, resident=1024, ordered=1):
    from fusion_hip._lib import NttJob
    t = (NttJob * max(1, len(table)))(*[NttJob(i, o, r, inv) for i, o, r, inv in table])
    p = (NttJob * max(1, len(prev)))(*[NttJob(i, o, r, inv) for i, o, r, inv in prev])
    order, end, cons, keep = (ctypes.c_int * 32)(), (ctypes.c_uint32 * 32)(), ctypes.c_int(-1), ctypes.c_int(-1)
    rc = lib.fz_diag_multi_order(t, len(table), p, len(prev), degree, resident, ordered, order, end, ctypes.byref(cons), ctypes.byref(keep))
    assert rc == 0, lib.fz_last_error()
    plan.keep = keep.value                     # the direction whose outputs store normally: 0 none, 1 forward, 2 inverse
    return list(order)[:len(table)], list(end)[:len(table)], cons.value


def test_which_outputs_are_kept_in_the_caches(lib):
    """normal stores for the producers' direction only when there are consumers, every producer has that direction and no consumer does"""
    a, b, c, e = 0x10000000, 0x20000000, 0x30000000, 0x40000000
    prev = [(a + j * J, b + j * J, 100, 0) for j in range(4)]
    cons_inv = [(b + j * J, c + j * J, 100, 1) for j in range(4)]
    cons_fwd = [(b + j * J, c + j * J, 100, 0) for j in range(4)]
    prod_fwd = [(a + (4 + j) * J, e + j * J, 100, 0) for j in range(4)]
    prod_inv = [(a + (4 + j) * J, e + j * J, 100, 1) for j in range(4)]

    def keep(table, prev_=prev, ordered=1):
        _, _, cons = plan(lib, table, prev_, ordered=ordered)
        return cons, plan.keep
    assert keep(prod_fwd + cons_inv) == (4, 1)               # the bench's launch: forward producers beside inverse consumers
    assert keep(prod_inv + cons_fwd) == (4, 2)               # mirrored
    assert keep(prod_fwd[:1] + cons_inv[:1]) == (1, 1) and keep(cons_fwd[:3] + prod_inv[:1]) == (3, 2)
    assert keep(prod_fwd + cons_fwd) == (4, 0)               # a consumer shares the producers' direction
    assert keep(prod_fwd + cons_inv[:3] + cons_fwd[3:]) == (4, 0)
    assert keep(prod_fwd[:2] + prod_inv[2:] + cons_inv) == (4, 0)      # producers of both directions
    assert keep(cons_inv) == (4, 0)                          # no producers (a closing launch)
    assert keep(prod_fwd) == (0, 0) and keep(prod_fwd + cons_inv, prev_=[]) == (0, 0)      # no consumers
    assert keep(prod_fwd + cons_inv, ordered=0) == (0, 0)    # FZ_MULTI_ORDER=0


def test_the_bench_launch_runs_its_inverse_jobs_first_newest_first(lib):
    x, y, z = 0x10000000, 0x20000000, 0x30000000
    prev = [(x + j * J, y + j * J, 4096, 0) for j in range(16)]                                    # in the order they ran
    table = [(x + (16 + j) * J, y + (16 + j) * J, 4096, 0) for j in range(16)] + [(y + j * J, z + j * J, 4096, 1) for j in range(16)]
    order, end, cons = plan(lib, table, prev)
    assert order == list(range(31, 15, -1)) + list(range(16)) and cons == 16
    assert end == [32 * (k + 1) for k in range(32)]                    # every job its share of the resident grid, as before
    # what THIS launch produced, in the order it ran, is the next launch's previous table: LIFO again
    ran = [table[j] for j in order]
    nxt = [(x + (32 + j) * J, y + (32 + j) * J, 4096, 0) for j in range(16)] + [(y + (16 + j) * J, z + (16 + j) * J, 4096, 1) for j in range(16)]
    order2, _, cons2 = plan(lib, nxt, ran)
    assert order2 == list(range(31, 15, -1)) + list(range(16)) and cons2 == 16
    # table order when nothing is consumed, and under FZ_MULTI_ORDER=0
    assert plan(lib, table, [])[0] == list(range(32)) and plan(lib, table, [])[2] == 0
    assert plan(lib, table[:16], prev)[0] == list(range(16)) and plan(lib, table[:16], prev)[2] == 0
    o0, e0, c0 = plan(lib, table, prev, ordered=0)
    assert o0 == list(range(32)) and c0 == 0 and e0 == end


def test_partial_consumers_rows_and_shared_inputs(lib):
    a, b, c = 0x10000000, 0x20000000, 0x30000000
    prev = [(a, b, 100, 1), (a + J, b + J, 200, 0), (a + 2 * J, b + 2 * J, 300, 1)]
    table = [(a + 5 * J, c, 50, 0),                  # 0: reads nothing of prev
             (b, c + J, 100, 0),                     # 1: the oldest output
             (b + 2 * J, c + 2 * J, 300, 1),         # 2: the newest
             (b + J, c + 3 * J, 201, 0),             # 3: MORE rows than were written: not a consumer
             (b + 2 * J, c + 4 * J, 7, 0),           # 4: the newest again (two jobs on one input, fewer rows)
             (b + J, b + J, 200, 1),                 # 5: in place
             (b + 16, c + 5 * J, 10, 0)]             # 6: inside an output, not AT it: not a consumer
    order, end, cons = plan(lib, table, prev, resident=64)
    assert sorted(order) == list(range(7))
    assert order == [2, 4, 5, 1, 0, 3, 6] and cons == 4
    assert all(e1 > e0 for e0, e1 in zip([0] + end, end))              # every job owns at least one workgroup, runs are contiguous


@pytest.mark.parametrize("degree", [64, 256])
@pytest.mark.parametrize("resident", [1, 7, 256, 1024])
def test_runs_cover_the_grid_exactly(lib, degree, resident):
    import random
    rng = random.Random(degree * 10000 + resident)
    for _ in range(50):
        n, m = rng.randint(1, 32), rng.randint(0, 32)
        prev = [(0x100000 * (k + 1), 0x40000000 + 0x1000000 * k, rng.choice([1, 3, 4095, 4097, 70000]), rng.randint(0, 1)) for k in range(m)]
        table = []
        for j in range(n):
            rows = rng.choice([1, 3, 16, 4095, 4096, 4097, 65536])
            src = rng.choice(prev)[1] if prev and rng.random() < 0.5 else 0x7000000 + 0x100000 * j
            table.append((src, 0x50000000 + 0x1000000 * j, rows, rng.randint(0, 1)))
        order, end, cons = plan(lib, table, prev, degree, resident)
        assert sorted(order) == list(range(n))
        is_cons = lambda j: any(table[j][0] == p[1] and table[j][2] <= p[2] for p in prev)
        assert [is_cons(j) for j in order] == [True] * cons + [False] * (n - cons)
        assert [j for j in order[cons:]] == sorted(order[cons:])       # the others: table order
        newest = [max(k for k, p in enumerate(prev) if table[j][0] == p[1] and table[j][2] <= p[2]) for j in order[:cons]]
        assert newest == sorted(newest, reverse=True)                  # consumers: the most recently produced first
        # workgroups: the same count per job as in table order (min(its workgroups, its share)), contiguous runs, no gaps
        _, end0, _ = plan(lib, table, prev, degree, resident, ordered=0)
        size0 = [e - s for s, e in zip([0] + end0, end0)]
        size = [e - s for s, e in zip([0] + end, end)]
        assert [size[order.index(j)] for j in range(n)] == size0
        tasks = [(r * degree + 1023) // 1024 for _, _, r, _ in table]
        assert all(1 <= size0[j] <= (tasks[j] + 3) // 4 for j in range(n)) and end[-1] == sum(size0)


def test_arguments_are_checked(lib):
    from fusion_hip._lib import NttJob
    t = (NttJob * 1)(NttJob(16, 32, 1, 0))
    order, end = (ctypes.c_int * 32)(), (ctypes.c_uint32 * 32)()
    assert lib.fz_diag_multi_order(t, 33, t, 0, 256, 1024, 1, order, end, None, None) == -1
    assert lib.fz_diag_multi_order(t, 1, None, 1, 256, 1024, 1, order, end, None, None) == -1
    assert lib.fz_diag_multi_order(t, 1, t, 0, 100, 1024, 1, order, end, None, None) == -1
    assert lib.fz_diag_multi_order(t, 1, t, 0, 256, 1024, 1, order, end, None, None) == 0 and order[0] == 0 and end[0] == 1
