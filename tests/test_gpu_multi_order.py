"""The execution order of a multi-job transform launch (fz_multi_plan: the jobs that read what the context's previous launch
wrote run first, the most recently written first, and the other jobs of such a launch store normally instead of streaming) changes
WHEN and HOW bytes move, never which: every output row of every launch is bit-equal to the oracle's transform (ntt.py:216-291,
:294-377) and to the same calls under FZ_MULTI_ORDER=0 (table order, streaming stores: the layout before the rule)."""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu
Q = O.PRIME


def _params(d):
    P = O.PARAMS[{64: 128, 256: 256}[d]]
    assert P["d"] == d
    return P["root"], P["inv_root"]


def _expected(coracle, d, bufs, launches):
    """the launches on the host: the jobs of one launch are independent (each reads the state before the launch)"""
    root, inv = _params(d)
    state = {k: v.copy() for k, v in bufs.items()}
    for table in launches:
        before = {k: v.copy() for k, v in state.items()}
        for src, dst, rows, inverse in table:
            x = np.ascontiguousarray(before[src][:rows])
            state[dst][:rows] = (coracle.ntt_inverse(x, Q, inv) if inverse else coracle.ntt_forward(x, Q, root)).reshape(rows, d)
    return state


def _run(monkeypatch, d, bufs, launches, ordered, kernel16, graph_replays=0, stream=True):
    """the launches on the device, one fz_ntt_multi call each -> every buffer afterwards"""
    import fusion_hip
    if ordered:
        monkeypatch.delenv("FZ_MULTI_ORDER", raising=False)
    else:
        monkeypatch.setenv("FZ_MULTI_ORDER", "0")
    if kernel16:
        monkeypatch.setenv("FZ_NTT_KERNEL", "16")
    else:
        monkeypatch.delenv("FZ_NTT_KERNEL", raising=False)
    root, inv = _params(d)
    ctx = fusion_hip.Context(Q, d, root, inv)
    s = ctx.stream_create() if stream else 0
    if stream:
        ctx.set_stream(s)
    dev = {k: fusion_hip.DeviceBuffer.from_numpy(ctx, v) for k, v in bufs.items()}
    tables = [[(dev[a].ptr, dev[b].ptr, r, inv_) for a, b, r, inv_ in t] for t in launches]
    if graph_replays:
        ctx.graph_begin()
        for t in tables:
            ctx.ntt_multi_dev(t)
        g = ctx.graph_end()
        for _ in range(graph_replays):
            g.launch()
        ctx.synchronize()
        g.destroy()
    else:
        for t in tables:
            ctx.ntt_multi_dev(t)
        ctx.synchronize()
    out = {k: dev[k].to_numpy(np.int32, bufs[k].shape) for k in bufs}
    if stream:
        ctx.set_stream(0)
        ctx.stream_destroy(s)
    for b in dev.values():
        b.free()
    return out


def _check(monkeypatch, coracle, d, bufs, launches, kernel16, graph_replays=0):
    want = _expected(coracle, d, bufs, launches)
    new = _run(monkeypatch, d, bufs, launches, True, kernel16, graph_replays)
    old = _run(monkeypatch, d, bufs, launches, False, kernel16, graph_replays)
    for k in bufs:
        assert np.array_equal(new[k], want[k]), f"buffer {k}: ordered launch differs from the oracle"
        assert np.array_equal(old[k], want[k]), f"buffer {k}: FZ_MULTI_ORDER=0 differs from the oracle"
        assert np.array_equal(new[k], old[k]), f"buffer {k}: ordered launch differs from FZ_MULTI_ORDER=0"


def _chain(depth, B, d, launches_mixed=2, seed=0):
    """bench.py's chain: an opening forward launch, mixed launches (forward of the next `depth` batches + inverse of the last
    ones), a closing inverse launch"""
    n = depth * (launches_mixed + 1)
    bufs = {}
    for b in range(n):
        bufs[f"x{b}"] = O.splitmix_centered(9000 + 97 * seed + b, B * d).reshape(B, d)
        bufs[f"y{b}"] = np.zeros((B, d), np.int32)
        bufs[f"z{b}"] = np.zeros((B, d), np.int32)
    launches, prev = [], []
    for l in range(launches_mixed + 1):
        new = list(range(l * depth, (l + 1) * depth))
        launches.append([(f"x{b}", f"y{b}", B, False) for b in new] + [(f"y{b}", f"z{b}", B, True) for b in prev])
        prev = new
    launches.append([(f"y{b}", f"z{b}", B, True) for b in prev])
    return bufs, launches


@pytest.mark.parametrize("d", [64, 256])
@pytest.mark.parametrize("depth", [1, 3, 8, 16])
def test_the_bench_chain_is_bit_equal_in_both_layouts(depth, d, coracle, monkeypatch):
    """opening forward launch, two mixed launches, closing inverse launch at the bench's depths; degree 256 at depth 16 in the
    headline's own size (4096 rows per batch: the launch takes the 16-per-lane kernel by itself), the others forced onto it"""
    headline = d == 256 and depth == 16
    bufs, launches = _chain(depth, 4096 if headline else 300, d, seed=depth)
    _check(monkeypatch, coracle, d, bufs, launches, kernel16=not headline)
    # and the chain is a round trip
    want = _expected(coracle, d, bufs, launches)
    assert all(np.array_equal(want[f"z{b}"], bufs[f"x{b}"]) for b in range(depth * 3))


@pytest.mark.parametrize("d", [64, 256])
def test_forward_consumers_partial_consumers_ragged_rows_and_shared_inputs(d, coracle, monkeypatch):
    rows = [1, 3, 4095, 4097, 200, 64]
    cap = max(rows)
    bufs = {f"a{k}": O.splitmix_centered(500 + k, cap * d).reshape(cap, d) for k in range(6)}
    for name in ("b", "c", "e"):
        bufs.update({f"{name}{k}": np.zeros((cap, d), np.int32) for k in range(6)})
    launches = [
        # inverse jobs produce b (ragged rows)
        [(f"a{k}", f"b{k}", rows[k], True) for k in range(6)],
        # consumers that are FORWARD jobs (b -> c), only some of the table: jobs 1, 3, 5 read fresh inputs instead; job 0 reads
        # fewer rows than were written, job 2 MORE rows than were written (not a consumer: the rest of its input is older data)
        [("b0", "c0", 1, False), ("a1", "c1", rows[1], True), ("b2", "c2", 4096, False), ("a3", "c3", 77, False),
         ("b4", "c4", 100, False), ("a5", "c5", rows[5], False)],
        # two jobs reading ONE input (both consumers), an in-place consumer, an in-place job that consumes nothing
        [("c0", "e0", 1, True), ("c0", "e1", 1, False), ("c2", "c2", 4095, True), ("a4", "a4", 3, False), ("c4", "e4", 100, True),
         ("c5", "e5", 64, True)],
        # the in-place outputs are consumed in turn
        [("c2", "e2", 4095, False), ("a4", "e3", 3, True)],
    ]
    _check(monkeypatch, coracle, d, bufs, launches, kernel16=True)
    _check(monkeypatch, coracle, d, bufs, launches, kernel16=False)      # by size: the radix-4 wave-tasks record what they wrote too


def test_a_captured_chain_replayed_twice(coracle, monkeypatch):
    """the order is fixed when the launches are captured; a replay runs the same order on the same buffers"""
    bufs, launches = _chain(3, 500, 256, seed=77)
    _check(monkeypatch, coracle, 256, bufs, launches, kernel16=True, graph_replays=2)


def test_two_contexts_on_two_streams_keep_their_own_records(coracle, monkeypatch):
    """two chains interleaved launch by launch, as bench.py issues them: a context's consumers are found in ITS previous launch"""
    import fusion_hip
    monkeypatch.delenv("FZ_MULTI_ORDER", raising=False)
    monkeypatch.setenv("FZ_NTT_KERNEL", "16")
    d = 256
    root, inv = _params(d)
    chains = []
    for c in range(2):
        ctx = fusion_hip.Context(Q, d, root, inv)
        s = ctx.stream_create()
        ctx.set_stream(s)
        bufs, launches = _chain(4, 256 + 13 * c, d, seed=200 + c)
        dev = {k: fusion_hip.DeviceBuffer.from_numpy(ctx, v) for k, v in bufs.items()}
        chains.append((ctx, s, bufs, launches, dev))
    for l in range(len(chains[0][3])):
        for ctx, s, bufs, launches, dev in chains:
            ctx.ntt_multi_dev([(dev[a].ptr, dev[b].ptr, r, i) for a, b, r, i in launches[l]])
    for ctx, s, bufs, launches, dev in chains:
        ctx.synchronize()
        want = _expected(coracle, d, bufs, launches)
        for k in bufs:
            assert np.array_equal(dev[k].to_numpy(np.int32, bufs[k].shape), want[k]), k
        ctx.set_stream(0)
        ctx.stream_destroy(s)
        for b in dev.values():
            b.free()


def _mirrored_chain(depth, B, d, seed):
    """the bench's chain with the directions swapped: an opening INVERSE launch, mixed launches of inverse producers beside FORWARD
    consumers, a closing forward launch -- the launches whose inverse jobs store normally (ntt_jobs16_keep<.., 2>)"""
    bufs, launches = _chain(depth, B, d, seed=seed)
    return bufs, [[(a, b, r, not inv) for a, b, r, inv in t] for t in launches]


@pytest.mark.parametrize("d", [64, 256])
@pytest.mark.parametrize("depth", [2, 4, 16])
def test_the_mirrored_chain_keeps_its_inverse_outputs_and_is_bit_equal(depth, d, coracle, monkeypatch):
    """inverse producers + forward consumers at the 4-, 8- and 32-entry tables (2 x depth jobs per mixed launch), both degrees"""
    bufs, launches = _mirrored_chain(depth, 300, d, seed=300 + depth)
    _check(monkeypatch, coracle, d, bufs, launches, kernel16=True)


@pytest.mark.parametrize("mirrored", [False, True])
def test_the_device_path_takes_the_layout_the_plan_gives(mirrored, monkeypatch):
    """what the launcher really did with each launch (fz_diag_multi_last): consumers first, newest first, the producers' direction
    kept -- forward (1) in the bench's chain, inverse (2) in the mirrored one; table order and streaming stores in the opening
    launch, no kept direction in the closing one (no producers), table order throughout under FZ_MULTI_ORDER=0 and on the radix-4
    schedule"""
    import fusion_hip
    d, depth = 256, 4
    root, inv = _params(d)
    bufs, launches = (_mirrored_chain if mirrored else _chain)(depth, 64, d, seed=5)
    for ordered, kernel in ((True, "16"), (False, "16"), (True, "4")):
        if ordered:
            monkeypatch.delenv("FZ_MULTI_ORDER", raising=False)
        else:
            monkeypatch.setenv("FZ_MULTI_ORDER", "0")
        monkeypatch.setenv("FZ_NTT_KERNEL", kernel)
        ctx = fusion_hip.Context(Q, d, root, inv)
        dev = {k: fusion_hip.DeviceBuffer.from_numpy(ctx, v) for k, v in bufs.items()}
        seen = []
        for t in launches:
            ctx.ntt_multi_dev([(dev[a].ptr, dev[b].ptr, r, i) for a, b, r, i in t])
            seen.append(ctx.diag_multi_last())
        ctx.synchronize()
        table = list(range(2 * depth))
        if ordered and kernel == "16":
            mixed = (list(range(2 * depth - 1, depth - 1, -1)) + list(range(depth)), depth, 2 if mirrored else 1)
            assert seen == [(table[:depth], 0, 0), mixed, mixed, (list(range(depth - 1, -1, -1)), depth, 0)], seen
        else:
            assert seen == [(table[:depth], 0, 0), (table, 0, 0), (table, 0, 0), (table[:depth], 0, 0)], seen
        for b in dev.values():
            b.free()
