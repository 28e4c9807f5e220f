"""The 16-per-lane transforms with their chunks landed in LDS by direct loads (fwd16_run / inv16_run: chunk_load_lds into the
landing area behind the staging image, the ragged last chunk through registers): every shape at which the loop takes another form,
bit for bit against the C oracle.  Outputs go into a poisoned buffer with a guard row on either side; inputs are any int32, with
+-(q-1)/2, 0, -2^31 and 2^31-1 among them.  The schedule is forced with FZ_NTT_KERNEL=16."""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu
Q = O.PRIME
POISON = 0x5a5a5a5a


def _root_for(q, d):
    for g in range(2, 2000):
        r = pow(g, (q - 1) // (2 * d), q)
        if pow(r, d, q) == q - 1:
            return r
    raise AssertionError("no root")


def _roots(d):
    root = {64: O.PARAMS[128]["root"], 256: O.PARAMS[256]["root"]}.get(d) or _root_for(Q, d)
    return root, pow(root, Q - 2, Q)


def _ctx(monkeypatch, d):
    import fusion_hip
    monkeypatch.setenv("FZ_NTT_KERNEL", "16")
    root, inv = _roots(d)
    return fusion_hip.Context(Q, d, root, inv)                 # a fresh context: the knob is read here


def _inputs(rows, d, seed):
    """any int32, the edge values in every row's first lanes' worth and scattered through the rest"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-2**31, 2**31, size=(rows, d), dtype=np.int64)
    h = (Q - 1) // 2
    edge = np.array([h, -h, 0, -2**31, 2**31 - 1], dtype=np.int64)
    x[:, :5] = np.roll(edge, seed % 5)
    x[:, -5:] = edge
    hit = rng.random((rows, d)) < 0.05
    x[hit] = edge[rng.integers(0, 5, size=int(hit.sum()))]
    return x.astype(np.int32)


def _want(coracle, x, d, inverse):
    root, inv = _roots(d)
    if x.shape[0] == 0:
        return x.copy()
    return (coracle.ntt_inverse(x, Q, inv) if inverse else coracle.ntt_forward(x, Q, root)).reshape(x.shape)


class Guarded:
    """`rows` rows of device memory between two guard rows, everything poisoned"""

    def __init__(self, ctx, rows, d):
        import fusion_hip
        self.ctx, self.rows, self.d = ctx, rows, d
        self.buf = fusion_hip.DeviceBuffer.from_numpy(ctx, np.full((rows + 2, d), POISON, np.int32))
        self.ptr = self.buf.ptr + 4 * d

    def poison(self):
        self.ctx.h2d(self.buf.ptr, np.full((self.rows + 2, self.d), POISON, np.int32))

    def read(self):
        a = self.buf.to_numpy(np.int32, (self.rows + 2, self.d))
        assert np.all(a[0] == POISON) and np.all(a[-1] == POISON), "a guard row was written"
        return a[1:-1]

    def free(self):
        self.buf.free()


_grid = {}


def _resident_workgroups(ctx, d):
    """the workgroups the context gives a transform launch larger than the chip holds at once: what one huge job of a stamped
    multi-job launch runs with (fz_diag_stamps_read reports the workgroups that stamped).  Degrees 32 and 128 have no multi-job
    kernel to stamp: they take degree 64's figure (same workgroup shape, LDS within 2 KiB), which only has to be near enough for
    every wave to meet a second chunk."""
    import fusion_hip
    dd = d if d in (64, 256) else 64
    if dd not in _grid:
        if dd != d:
            root, inv = _roots(dd)
            ctx = fusion_hip.Context(Q, dd, root, inv)
        rows = (1 << 24) // dd                                   # 16384 chunks = 4096 workgroups' worth at one chunk per wave
        src = fusion_hip.DeviceBuffer(ctx, rows * dd * 4)
        dst = fusion_hip.DeviceBuffer(ctx, rows * dd * 4)
        ctx.diag_stamps_begin(1, 8192)
        ctx.ntt_multi_dev([(src.ptr, dst.ptr, rows, False)])
        ctx.diag_stamps_stop()
        wg = ctx.diag_stamps_read(1)[3]
        src.free(); dst.free()
        if dd != d:
            ctx.close()
        assert len(wg) == 1 and 0 < int(wg[0]) < 4096, wg      # capped by the resident grid, not by the job's size
        _grid[dd] = int(wg[0])
    return _grid[dd]


def _both_directions(ctx, coracle, rows, d, seed):
    import fusion_hip
    x = _inputs(rows, d, seed)
    src = fusion_hip.DeviceBuffer.from_numpy(ctx, x)
    out = Guarded(ctx, rows, d)
    for inverse in (False, True):
        out.poison()
        (ctx.ntt_inverse_dev if inverse else ctx.ntt_forward_dev)(src.ptr, out.ptr, rows)
        ctx.synchronize()
        assert np.array_equal(out.read(), _want(coracle, x, d, inverse)), (d, rows, "inverse" if inverse else "forward")
    src.free(); out.free()


# ---- case 1: one-job launches at degree 256 (four rows per chunk) -------------------------------------------------------------
@pytest.mark.parametrize("rows", [4, 5, 7, 16, 20])
def test_one_job_small_shapes(rows, coracle, monkeypatch):
    """one chunk in one wave; a ragged last chunk of one and of three rows; one chunk in every wave of a workgroup; five chunks"""
    ctx = _ctx(monkeypatch, 256)
    _both_directions(ctx, coracle, rows, 256, 100 + rows)
    ctx.close()


@pytest.mark.parametrize("extra", [4, 5])
def test_one_wave_of_the_grid_iterates_twice(extra, coracle, monkeypatch):
    """4 x (resident waves) + 4 rows: the grid's first wave requests a second chunk behind its first transpose and finds it landed;
    + 5: the second wave's second chunk is the ragged one"""
    ctx = _ctx(monkeypatch, 256)
    waves = 4 * _resident_workgroups(ctx, 256)
    _both_directions(ctx, coracle, 4 * waves + extra, 256, 200 + extra)
    ctx.close()


def test_every_wave_iterates_three_times_and_the_batch_ends_ragged(coracle, monkeypatch):
    """3 x (resident waves) + 1 whole chunks and a ragged one: the steady-state form runs twice in a row in every wave (the wait
    at its end is followed by another request), the first wave four times, the second ends on the ragged chunk"""
    ctx = _ctx(monkeypatch, 256)
    waves = 4 * _resident_workgroups(ctx, 256)
    _both_directions(ctx, coracle, 4 * (3 * waves + 1) + 3, 256, 300)
    ctx.close()


# ---- case 2: the other degrees (1024 / d rows per chunk) -------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 32, 128])
def test_other_degrees(d, coracle, monkeypatch):
    """one chunk, one chunk and a ragged one, 2 x 64 + 1 chunks"""
    ctx = _ctx(monkeypatch, d)
    per = 1024 // d
    for rows in (per, per + 1, (2 * 64 + 1) * per):
        _both_directions(ctx, coracle, rows, d, 400 + d + rows)
    ctx.close()


@pytest.mark.parametrize("d", [64, 32, 128])
def test_other_degrees_with_every_wave_iterating(d, coracle, monkeypatch):
    """two chunks and more in every wave of the resident grid, the last one ragged"""
    ctx = _ctx(monkeypatch, d)
    per = 1024 // d
    waves = 4 * _resident_workgroups(ctx, d)
    _both_directions(ctx, coracle, (2 * waves + 3) * per + 1, d, 500 + d)
    ctx.close()


# ---- case 3: multi-job launches ------------------------------------------------------------------------------------------------
def _multi(ctx, coracle, d, tables, bufs, graph_replays=0):
    """tables of (src, dst, rows, inverse) over named host arrays; outputs into guarded, poisoned buffers -> checked against the
    oracle, launch by launch"""
    import fusion_hip
    state = {k: v.copy() for k, v in bufs.items()}
    for t in tables:
        before = {k: v.copy() for k, v in state.items()}
        for src, dst, rows, inverse in t:
            state[dst][:rows] = _want(coracle, np.ascontiguousarray(before[src][:rows]), d, inverse)
    written = {dst for t in tables for _, dst, _, _ in t}
    dev = {}
    for k, v in bufs.items():
        dev[k] = Guarded(ctx, v.shape[0], d)
        if k not in written:
            ctx.h2d(dev[k].ptr, v)
    dtables = [[(dev[a].ptr, dev[b].ptr, r, i) for a, b, r, i in t] for t in tables]
    if graph_replays:
        s = ctx.stream_create()
        ctx.set_stream(s)
        ctx.graph_begin()
        for t in dtables:
            ctx.ntt_multi_dev(t)
        g = ctx.graph_end()
        for _ in range(graph_replays):
            g.launch()
        ctx.synchronize()
        g.destroy()
        ctx.set_stream(0)
        ctx.stream_destroy(s)
    else:
        for t in dtables:
            ctx.ntt_multi_dev(t)
        ctx.synchronize()
    for k in bufs:
        got = dev[k].read()
        rows = max([r for t in tables for _, dst, r, _ in t if dst == k], default=bufs[k].shape[0])
        assert np.array_equal(got[:rows], state[k][:rows]), k
        if k in written:
            assert np.all(got[rows:] == POISON), k
        dev[k].free()


def test_two_jobs_of_four_rows(coracle, monkeypatch):
    d = 256
    ctx = _ctx(monkeypatch, d)
    bufs = {"a": _inputs(4, d, 1), "b": _inputs(4, d, 2), "x": np.zeros((4, d), np.int32), "y": np.zeros((4, d), np.int32)}
    _multi(ctx, coracle, d, [[("a", "x", 4, False), ("b", "y", 4, True)]], bufs)
    ctx.close()


def test_thirty_two_jobs_of_eight_rows_mixed_directions(coracle, monkeypatch):
    d = 256
    ctx = _ctx(monkeypatch, d)
    bufs, table = {}, []
    for k in range(32):
        bufs[f"a{k}"] = _inputs(8, d, 600 + k)
        bufs[f"x{k}"] = np.zeros((8, d), np.int32)
        table.append((f"a{k}", f"x{k}", 8, k % 3 != 0))
    _multi(ctx, coracle, d, [table], bufs)
    ctx.close()


def _chain(depth, B, d, mirrored):
    """bench.py's chain in three launches: an opening launch, a mixed launch (the next batches beside the transforms back of the
    last ones), a closing launch; mirrored: the directions swapped (the kept direction is then the inverse)"""
    bufs = {}
    for b in range(2 * depth):
        bufs[f"x{b}"] = _inputs(B, d, 700 + b)
        bufs[f"y{b}"] = np.zeros((B, d), np.int32)
        bufs[f"z{b}"] = np.zeros((B, d), np.int32)
    first, second = list(range(depth)), list(range(depth, 2 * depth))
    tables = [[(f"x{b}", f"y{b}", B, mirrored) for b in first],
              [(f"x{b}", f"y{b}", B, mirrored) for b in second] + [(f"y{b}", f"z{b}", B, not mirrored) for b in first],
              [(f"y{b}", f"z{b}", B, not mirrored) for b in second]]
    return bufs, tables


@pytest.mark.parametrize("graph_replays", [0, 2])
@pytest.mark.parametrize("mirrored", [False, True])
def test_a_chain_of_three_launches_in_the_bench_shape(mirrored, graph_replays, coracle, monkeypatch):
    """64 rows per batch, sixteen batches per launch: the mixed launch stores its producers' outputs normally (ntt_jobs16_keep with
    the forward direction kept, mirrored the inverse); issued directly, and captured into a graph and replayed twice"""
    d = 256
    ctx = _ctx(monkeypatch, d)
    bufs, tables = _chain(16, 64, d, mirrored)
    if not graph_replays:
        import fusion_hip
        dev = {k: fusion_hip.DeviceBuffer.from_numpy(ctx, v) for k, v in bufs.items()}
        kept = []
        for t in tables:
            ctx.ntt_multi_dev([(dev[a].ptr, dev[b].ptr, r, i) for a, b, r, i in t])
            kept.append(ctx.diag_multi_last()[2])
        ctx.synchronize()
        assert kept[1] == (2 if mirrored else 1), kept          # the kernel this test is about did run
        for b in dev.values():
            b.free()
    _multi(ctx, coracle, d, tables, bufs, graph_replays)
    ctx.close()


# ---- case 4: in place ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [16, 23])
def test_in_place_jobs(rows, coracle, monkeypatch):
    """a job whose input and output are one buffer (the parent supports it: a wave stores chunk i while chunk i + stride lands)"""
    d = 256
    ctx = _ctx(monkeypatch, d)
    waves = 4 * _resident_workgroups(ctx, d)
    big = 4 * (2 * waves + 2) + 1
    for n in (rows, big):
        for inverse in (False, True):
            x = _inputs(n, d, 800 + n % 1000 + inverse)
            g = Guarded(ctx, n, d)
            ctx.h2d(g.ptr, x)
            (ctx.ntt_inverse_dev if inverse else ctx.ntt_forward_dev)(g.ptr, g.ptr, n)
            ctx.synchronize()
            assert np.array_equal(g.read(), _want(coracle, x, d, inverse)), (n, inverse)
            ctx.h2d(g.ptr, x)
            ctx.ntt_multi_dev([(g.ptr, g.ptr, n, inverse)])
            ctx.synchronize()
            assert np.array_equal(g.read(), _want(coracle, x, d, inverse)), (n, inverse, "multi")
            g.free()
    ctx.close()
