"""GPU tests of the entry points added in round 2: the multi-job transform launch (fz_ntt_multi), degrees that are not
a multiple of 4, the RCCL binding of the C ABI on one rank, the launch-floor diagnostics and the
device guard of contexts on different GPUs."""
import ctypes
import os

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu
Q = O.PRIME


def _root_for(q, d):
    for g in range(2, 2000):
        r = pow(g, (q - 1) // (2 * d), q)
        if pow(r, d, q) == q - 1:
            return r
    raise AssertionError("no root")


@pytest.mark.parametrize("kernel", ["auto", "4", "16"])
@pytest.mark.parametrize("secpar", [128, 256])
def test_ntt_multi_ragged_mixed_jobs_match_the_oracle(secpar, kernel, coracle, monkeypatch):
    """one dispatch over a ragged list of forward and inverse jobs (one of them in place, one empty, more than one
    table of 32): every job equals the oracle's transform of its rows (ntt.py:216-291, :294-377) -- through the radix-4
    wave-tasks (ntt_jobs4) and through the 16-per-lane form (ntt_jobs16, round 5), whichever the launch's size would pick"""
    import fusion_hip
    if kernel != "auto":
        monkeypatch.setenv("FZ_NTT_KERNEL", kernel)
    P = O.PARAMS[secpar]
    d, root, inv = P["d"], P["root"], P["inv_root"]
    ctx = fusion_hip.Context(Q, d, root, inv)
    rng = np.random.default_rng(secpar)
    rows = [1, 2, 3, 5, 64, 0, 4096, 4097, 129, 7] + [int(r) for r in rng.integers(1, 300, size=30)]
    bufs, jobs, expect = [], [], []
    for j, r in enumerate(rows):
        inverse = (j % 3 == 1)
        x = O.splitmix_centered(1000 + j, max(r, 1) * d).reshape(max(r, 1), d)[:r]
        if j % 4 == 0 and r:       # raw int32 inputs, not centred
            x = rng.integers(-2**31, 2**31, size=(r, d), dtype=np.int64).astype(np.int32)
        din = fusion_hip.DeviceBuffer.from_numpy(ctx, x) if r else fusion_hip.DeviceBuffer(ctx, 16)
        dout = din if j % 5 == 2 else fusion_hip.DeviceBuffer(ctx, max(16, r * d * 4))      # some in place
        bufs += [din, dout]
        jobs.append((din.ptr, dout.ptr, r, inverse))
        expect.append((coracle.ntt_inverse(x, Q, inv) if inverse else coracle.ntt_forward(x, Q, root)) if r else x)
    assert len([r for r in rows if r]) > 32           # exercises the flush of a full job table
    ctx.ntt_multi_dev(jobs)
    ctx.synchronize()
    for (din, dout, r, inverse), e in zip(jobs, expect):
        if r:
            got = np.empty((r, d), np.int32)
            ctx.d2h(got, dout)
            assert np.array_equal(got, e), (r, inverse)
    # the bench's shape: forward of 4 batches of 4096 rows, then their inverses, each ONE launch
    B = 4096
    xs = [O.splitmix_centered(50 + k, B * d).reshape(B, d) for k in range(4)]
    dx = [fusion_hip.DeviceBuffer.from_numpy(ctx, x) for x in xs]
    dy = [fusion_hip.DeviceBuffer(ctx, B * d * 4) for _ in xs]
    ctx.ntt_multi_dev([(a.ptr, b.ptr, B, False) for a, b in zip(dx, dy)])
    y0 = dy[0].to_numpy(np.int32, (B, d))
    assert np.array_equal(y0, coracle.ntt_forward(xs[0], Q, root))
    ctx.ntt_multi_dev([(b.ptr, b.ptr, B, True) for b in dy])
    for x, b in zip(xs, dy):
        assert np.array_equal(b.to_numpy(np.int32, (B, d)), x)
    for b in bufs + dx + dy:
        b.free()


@pytest.mark.parametrize("kernel", ["auto", "4", "16"])
@pytest.mark.parametrize("depth", [1, 3, 4, 8, 16])
def test_ntt_multi_in_the_headline_shape_with_device_timestamps(depth, kernel, coracle, monkeypatch):
    """bench.py's launch: the forward transforms of `depth` batches of 4096 rows and the inverse transforms of `depth` other
    batches in ONE dispatch (2 x depth jobs: the 4-, 8- and 32-entry tables; 65 536 rows take the 16-per-lane form on their
    own) -- every output row against the oracle (ntt.py:216-291, :294-377), with and without timestamp slots, and the
    timestamps themselves: every workgroup stamped, entry <= exit, the launches of one stream in order."""
    import fusion_hip
    if kernel != "auto":
        monkeypatch.setenv("FZ_NTT_KERNEL", kernel)
    P = O.PARAMS[256]
    d, root, inv, B = P["d"], P["root"], P["inv_root"], 4096
    ctx = fusion_hip.Context(Q, d, root, inv)
    s = ctx.stream_create()
    ctx.set_stream(s)
    xs = [O.splitmix_centered(700 + k, B * d).reshape(B, d) for k in range(2 * depth)]
    xs[0] = np.random.default_rng(depth).integers(-2**31, 2**31, size=(B, d), dtype=np.int64).astype(np.int32)    # raw int32 rows
    want = [coracle.ntt_forward(x, Q, root) if k < depth else coracle.ntt_inverse(x, Q, inv) for k, x in enumerate(xs)]
    din = [fusion_hip.DeviceBuffer.from_numpy(ctx, x) for x in xs]
    dout = [fusion_hip.DeviceBuffer(ctx, B * d * 4) for _ in xs]
    jobs = [(a.ptr, b.ptr, B, k >= depth) for k, (a, b) in enumerate(zip(din, dout))]

    def check():
        ctx.synchronize()
        for k, b in enumerate(dout):
            assert np.array_equal(b.to_numpy(np.int32, (B, d)), want[k]), (depth, kernel, k)
            ctx.h2d(b.ptr, np.zeros((B, d), np.int32))
        ctx.synchronize()
    ctx.ntt_multi_dev(jobs)
    check()
    ctx.diag_stamps_begin(4, 4 * 2 * depth * B)
    for _ in range(3):
        ctx.ntt_multi_dev(jobs)
    ctx.diag_stamps_stop()
    ctx.ntt_multi_dev(jobs)                         # (after stop: carries no slots)
    st, en, last, wg = ctx.diag_stamps_read(8)
    assert len(st) == 3 and (wg > 0).all() and (st > 0).all()
    assert (en >= last).all() and (last >= st).all()
    assert st[1] >= st[0] and st[2] >= st[1] and en[2] >= en[0]          # one stream: launches in order
    us = (en - st).astype(np.int64) / 100.0
    assert (us > 1.0).all() and (us < 5000.0).all(), us                  # microseconds, not garbage
    check()
    # captured with slots, reset, ONE replay, read: what bench.py does
    ctx.diag_stamps_begin(2, 2 * 2 * depth * B)
    ctx.graph_begin()
    ctx.ntt_multi_dev(jobs)
    g = ctx.graph_end()
    ctx.diag_stamps_stop()
    g.launch()
    ctx.diag_stamps_reset()
    st0, en0, _, wg0 = ctx.diag_stamps_read(2)
    assert len(st0) == 1 and st0[0] == 0 and en0[0] == 0 and wg0[0] == 0  # nothing has run since the reset
    g.launch()
    st1, en1, _, wg1 = ctx.diag_stamps_read(2)
    assert wg1[0] == wg[0] and en1[0] > st1[0] > en[2]
    check()
    g.destroy()
    ctx.set_stream(0)
    ctx.stream_destroy(s)
    for b in din + dout:
        b.free()


def test_ntt_multi_other_degrees_and_graph_capture(coracle):
    import fusion_hip
    d = 16
    root = _root_for(Q, d)
    ctx = fusion_hip.Context(Q, d, root, pow(root, Q - 2, Q))
    x = O.splitmix_centered(3, 50 * d).reshape(50, d)
    a, b = fusion_hip.DeviceBuffer.from_numpy(ctx, x), fusion_hip.DeviceBuffer(ctx, x.nbytes)
    ctx.ntt_multi_dev([(a.ptr, b.ptr, 20, False), (a.ptr + 20 * d * 4, b.ptr + 20 * d * 4, 30, False)])   # one launch per job
    assert np.array_equal(b.to_numpy(np.int32, x.shape), coracle.ntt_forward(x, Q, root))
    # degree 256: the job table travels in the kernel arguments, so the call can be recorded and replayed
    P = O.PARAMS[256]
    c2 = fusion_hip.Context(Q, 256, P["root"], P["inv_root"])
    s = c2.stream_create()
    c2.set_stream(s)
    x2 = O.splitmix_centered(4, 300 * 256).reshape(300, 256)
    a2, b2, z2 = fusion_hip.DeviceBuffer.from_numpy(c2, x2), fusion_hip.DeviceBuffer(c2, x2.nbytes), fusion_hip.DeviceBuffer(c2, x2.nbytes)
    jobs_f = [(a2.ptr, b2.ptr, 100, False), (a2.ptr + 100 * 1024, b2.ptr + 100 * 1024, 200, False)]
    jobs_i = [(b2.ptr, z2.ptr, 300, True)]
    c2.ntt_multi_dev(jobs_f)
    c2.graph_begin()
    c2.ntt_multi_dev(jobs_f)
    c2.ntt_multi_dev(jobs_i)
    g = c2.graph_end()
    g.launch()
    g.launch()
    c2.synchronize()
    assert np.array_equal(b2.to_numpy(np.int32, x2.shape), coracle.ntt_forward(x2, Q, P["root"]))
    assert np.array_equal(z2.to_numpy(np.int32, x2.shape), x2)
    g.destroy()
    c2.set_stream(0)
    c2.stream_destroy(s)


@pytest.mark.parametrize("degree", [5, 6, 7, 9, 10, 12])
def test_degrees_that_are_not_a_multiple_of_four(degree, coracle):
    """ring-only contexts accept any degree; the int4 kernels must not be chosen for them:
    matvec, sign_core, aggregate_core and the GeneralMatrix product against the oracle"""
    import fusion_hip
    from algebra.matrices import GeneralMatrix
    from algebra.polynomials import PolynomialNTTRepresentation as PN
    q, l, n = 65537, 7, 11
    ctx = fusion_hip.Context(q, degree, 0, 0)         # ring-only: pointwise, matvec, scheme cores
    rng = np.random.default_rng(degree)
    A = rng.integers(-(q // 2), q // 2 + 1, size=(l, degree)).astype(np.int32)
    S = rng.integers(-2**31, 2**31, size=(n, l, degree), dtype=np.int64).astype(np.int32)
    assert np.array_equal(ctx.matvec(A, S), coracle.matvec(A, S, q))
    sk = rng.integers(-(q // 2), q // 2 + 1, size=(n, 2, l, degree)).astype(np.int32)
    c = rng.integers(-(q // 2), q // 2 + 1, size=(n, degree)).astype(np.int32)
    sig = ctx.sign_core(sk, c)
    assert np.array_equal(sig, coracle.sign_core(sk, c, q))
    assert np.array_equal(ctx.aggregate_core(sig, c), coracle.aggregate_core(sig, c, q))
    # the drop-in matrix product goes through the same entry point (matrices.py:115-131)
    root = 3                                            # q = 65537: 3 is a primitive root; order 65536 is fine for the container
    mk = lambda v: PN(modulus=q, degree=degree, root=pow(root, 65536 // 2, q), inv_root=pow(pow(root, 65536 // 2, q), q - 2, q),
                      root_order=2, values=[int(t) for t in v])
    left = GeneralMatrix(matrix=[[mk(A[k]) for k in range(l)]])
    right = GeneralMatrix(matrix=[[mk(S[0, k])] for k in range(l)])
    prod = left * right
    assert [int(t) for t in prod.matrix[0][0].values] == coracle.matvec(A, S[:1], q)[0].tolist()


def test_rccl_binding_of_the_c_abi_on_one_rank():
    """fz_comm_* / fz_allreduce_i64 with nranks = 1 (the single-GPU box): the binding, the in-place int64 sum on the
    context's stream, and its capture into the library's own graph between two kernels"""
    import fusion_hip
    P = O.PARAMS[256]
    q, d, l = P["q"], P["d"], P["rank"]
    ctx = fusion_hip.Context(q, d, P["root"], P["inv_root"])
    uid = fusion_hip.comm_unique_id()
    assert len(uid) == 128
    comm = fusion_hip.Comm(ctx, 1, 0, uid)
    assert comm.info() == (1, 0)
    v = np.arange(-500, 500, dtype=np.int64) * (2**40 + 3)
    buf = fusion_hip.DeviceBuffer.from_numpy(ctx, v)
    ctx.allreduce_i64_dev(comm, buf.ptr, v.size)
    ctx.synchronize()
    assert np.array_equal(buf.to_numpy(np.int64, v.shape), v)
    ctx.reduce_scatter_i64_dev(comm, buf.ptr, v.size)            # one rank: its block is the whole buffer, in place
    ctx.synchronize()
    assert np.array_equal(buf.to_numpy(np.int64, v.shape), v)
    # partials -> all-reduce -> verification from the sums, as one replayable graph
    s = ctx.stream_create()
    ctx.set_stream(s)
    n = 40
    rng = np.random.default_rng(1)
    A = O.splitmix_centered(8, l * d).reshape(l, d)
    coef = rng.integers(-52, 53, size=(n, 2, d)).astype(np.int32)
    dA, dc = fusion_hip.DeviceBuffer.from_numpy(ctx, A), fusion_hip.DeviceBuffer.from_numpy(ctx, coef)
    dsk, dvk = fusion_hip.DeviceBuffer(ctx, n * 2 * l * d * 4), fusion_hip.DeviceBuffer(ctx, n * 2 * d * 4)
    ctx.keygen_core_bcast_dev(dA.ptr, dc.ptr, dsk.ptr, dvk.ptr, n, l)
    vk = dvk.to_numpy(np.int32, (n, 2, d))
    ch = ctx.ntt_forward((rng.integers(0, 2, size=(n, d))).astype(np.int32))
    al = ctx.ntt_forward((rng.integers(0, 2, size=(n, d))).astype(np.int32))
    dch, dal = fusion_hip.DeviceBuffer.from_numpy(ctx, ch), fusion_hip.DeviceBuffer.from_numpy(ctx, al)
    dL, dR = fusion_hip.DeviceBuffer.from_numpy(ctx, vk[:, 0]), fusion_hip.DeviceBuffer.from_numpy(ctx, vk[:, 1])
    dsig = fusion_hip.DeviceBuffer(ctx, n * l * d * 4)
    dpart = fusion_hip.DeviceBuffer(ctx, (l * d + d) * 8)
    dver = fusion_hip.DeviceBuffer.from_numpy(ctx, np.full(1, -1, np.int32))

    def step():
        ctx.sign_core_dev(dsk.ptr, dch.ptr, dsig.ptr, n, l)
        ctx.aggregate_target_partial_batch_dev(dsig.ptr, dal.ptr, dL.ptr, dR.ptr, dch.ptr, dpart.ptr, l * d,
                                               dpart.ptr + l * d * 8, d, 1, n, l)
        ctx.allreduce_i64_dev(comm, dpart.ptr, l * d + d)
        ctx.reduce_scatter_i64_dev(comm, dpart.ptr, l * d + d)   # (the other form of the exchange, capturable like the first)
        ctx.verify_partials_batch_async_dev(dA.ptr, dpart.ptr, l * d, dpart.ptr + l * d * 8, d, 1, l, 2**40, d, dver.ptr)
    step()
    ctx.synchronize()
    assert dver.to_numpy(np.int32, (1,))[0] == 0
    ctx.graph_begin()
    step()
    g = ctx.graph_end()
    for _ in range(3):
        g.launch()
    ctx.synchronize()
    assert dver.to_numpy(np.int32, (1,))[0] == 0
    g.destroy()
    ctx.set_stream(0)
    ctx.stream_destroy(s)
    # fz_broadcast_i32 (how the rank that ran hash_ag's sponge hands the coefficient rows to the others: ShardedScheme,
    # alpha_mode "root") and fz_rccl_version, on the same communicator
    from fusion_hip.dist import CommCollective
    assert fusion_hip.rccl_version() > 20000
    rows = O.splitmix_centered(5, 7 * d).reshape(7, d)
    assert np.array_equal(CommCollective(ctx, comm).broadcast_i32(rows, rows.shape, 0), rows)
    with pytest.raises(fusion_hip.FusionHipError):
        ctx.broadcast_i32_dev(comm, 0, 16, 3)          # root outside the communicator (and a NULL buffer)
    comm.destroy()
    comm.destroy()                                     # idempotent, in Python ...
    # ... and in the C ABI: the handle a caller kept after destroying it is left alone (not freed twice, no RCCL call)
    comm2 = fusion_hip.Comm(ctx, 1, 0, fusion_hip.comm_unique_id())        # a second communicator in the same process
    raw = ctypes.c_void_p(comm2._c.value)
    assert comm2.info() == (1, 0)
    comm2.destroy()
    assert ctx._lib.fz_comm_destroy(raw) == 0 and ctx._lib.fz_comm_destroy(raw) == 0
    # ONE RCCL in the process, whoever mapped it first (torch ships its own copy under the same soname; rounds 2-4 bound
    # /opt/rocm's beside it and the process aborted at exit: profiles/r05_rccl_exit_matrix.txt)
    lib = fusion_hip.rccl_library()
    assert lib["copies_mapped"] == 1 and lib["how"] in ("already mapped (shared)", "beside the HIP runtime", "default search path"), lib
    hip_dirs = {os.path.dirname(os.path.realpath(p)) for p in fusion_hip.runtime_report()["mapped_libamdhip64"]}
    assert len(hip_dirs) == 1 and os.path.dirname(os.path.realpath(lib["path"])) in hip_dirs, (lib, hip_dirs)


def test_launch_floor_diagnostics_run():
    import fusion_hip
    P = O.PARAMS[256]
    ctx = fusion_hip.Context(P["q"], P["d"], P["root"], P["inv_root"])
    x = O.splitmix_centered(1, 4096 * 256)
    a, b = fusion_hip.DeviceBuffer.from_numpy(ctx, x), fusion_hip.DeviceBuffer(ctx, x.nbytes)
    ctx.diag_empty_launch()
    ctx.diag_copy_dev(a.ptr, b.ptr, x.nbytes)
    assert np.array_equal(b.to_numpy(np.int32, x.shape), x)
    # the shader-clock probe: idle, and beside queued work on the context's stream (it must return although that work is still
    # running, and leave the stream usable)
    assert 300 < ctx.diag_shader_clock(200) < 4000
    s = ctx.stream_create()
    ctx.set_stream(s)
    for _ in range(200):
        ctx.ntt_forward_dev(a.ptr, b.ptr, 4096)
    assert 300 < ctx.diag_shader_clock(300) < 4000
    ctx.synchronize()
    assert np.array_equal(b.to_numpy(np.int32, (4096, 256)), ctx.ntt_forward(x.reshape(4096, 256)))
    # the delay kernel (the bench's stand-in for an exchange step): occupies the stream for at least what was asked, in order
    ctx.timer_start()
    ctx.diag_delay(300)
    ctx.ntt_forward_dev(a.ptr, b.ptr, 4096)
    assert 0.3 <= ctx.timer_stop_ms() < 5.0
    assert np.array_equal(b.to_numpy(np.int32, (4096, 256)), ctx.ntt_forward(x.reshape(4096, 256)))
    ctx.set_stream(0)
    ctx.stream_destroy(s)
    with pytest.raises(fusion_hip.FusionHipError):
        ctx.diag_shader_clock(0)
    with pytest.raises(fusion_hip.FusionHipError):
        ctx.diag_delay(0)


def test_contexts_on_two_devices_do_not_cross(coracle):
    """every entry point makes the context's device current: a context on device 1 must launch
    there even when the last-created context sits on device 0"""
    import fusion_hip
    lib = fusion_hip.load_library()
    n = ctypes.c_int(0)
    lib.fz_device_count(ctypes.byref(n))
    if n.value < 2:
        pytest.skip("needs two GPUs (the driver's multi-GPU node)")
    P = O.PARAMS[256]
    c1 = fusion_hip.Context(P["q"], P["d"], P["root"], P["inv_root"], device=1)
    c0 = fusion_hip.Context(P["q"], P["d"], P["root"], P["inv_root"], device=0)     # leaves device 0 current
    x = O.splitmix_centered(9, 300 * 256).reshape(300, 256)
    f1 = c1.ntt_forward(x)                                                              # default stream, device 1
    f0 = c0.ntt_forward(x)
    ref = coracle.ntt_forward(x, P["q"], P["root"])
    assert np.array_equal(f1, ref) and np.array_equal(f0, ref)
    assert np.array_equal(c1.ntt_inverse(f1), x)


def test_block_pool_reuses_in_stream_order(monkeypatch):
    """fz_free keeps large blocks and fz_malloc hands them out again (include/fusion_hip.h): the same address comes back for a
    request it fits, work queued on the old contents before the free still completes before the new owner's work, small blocks
    and FZ_POOL_MB=0 go straight to hipMalloc / hipFree, the cap holds"""
    import fusion_hip
    P = O.PARAMS[256]
    q, d = P["q"], P["d"]
    ctx = fusion_hip.Context(q, d, P["root"], P["inv_root"])
    rows = 1 << 14
    x = O.splitmix_centered(3, rows * d).reshape(rows, d)
    want = ctx.ntt_forward(x)
    a, out = ctx.malloc(x.nbytes), ctx.malloc(x.nbytes)
    ctx.h2d(a, x)
    ctx.ntt_forward_dev(a, out, rows)                  # queued: reads a
    ctx.free(a)
    b = ctx.malloc(x.nbytes - 4096)                    # fits the block just freed (within a quarter)
    assert b == a
    ctx.fill_synthetic_dev(b, rows * d - 1024, 9)      # queued AFTER the transform that reads the old contents
    got = np.empty_like(x)
    ctx.d2h(got, out)
    assert np.array_equal(got, want)
    c = ctx.malloc(x.nbytes * 2)                       # does not fit: a fresh block
    assert c not in (a, out)
    small1 = ctx.malloc(1000)
    ctx.free(small1)
    for p in (b, c, out):
        ctx.free(p)
    assert ctx.malloc(x.nbytes) in (b, out)            # exact size: one of the two 16 MiB blocks
    ctx.close()
    monkeypatch.setenv("FZ_POOL_MB", "0")
    ctx = fusion_hip.Context(q, d, P["root"], P["inv_root"])
    monkeypatch.delenv("FZ_POOL_MB")
    p1 = ctx.malloc(1 << 24)
    ctx.free(p1)
    p2 = ctx.malloc(1 << 24)
    ctx.free(p2)                                       # (whatever address hipMalloc chose: nothing is tracked, nothing kept)
    ctx.close()
    monkeypatch.setenv("FZ_POOL_MB", "20")
    ctx = fusion_hip.Context(q, d, P["root"], P["inv_root"])
    monkeypatch.delenv("FZ_POOL_MB")
    ps = [ctx.malloc(1 << 23) for _ in range(4)]       # 4 x 8 MiB, cap 20 MiB: two stay, the oldest are released
    for p in ps:
        ctx.free(p)
    back = [ctx.malloc(1 << 23) for _ in range(2)]
    assert set(back) <= set(ps[2:]) | set(ps)          # reuse comes from the kept ones
    assert ctx.malloc(1 << 25) not in ps               # larger than the cap: never pooled, never confused with a kept block
    ctx.close()


def test_block_pool_is_thread_safe_stream_change_safe_and_shared(monkeypatch):
    """(1) fz_malloc / fz_free from several threads at once (a DeviceBuffer.__del__ may run on any thread) keep the
    pool consistent; (2) a block freed on one stream and reused after fz_ctx_set_stream is ordered behind its old users (the
    event fz_free records, and the drain on every stream change); (3) fz_pool_trim releases idle blocks; (4) ONE cap
    (FZ_POOL_MB) covers the pools of all contexts of the process."""
    import threading
    import fusion_hip
    P = O.PARAMS[256]
    q, d = P["q"], P["d"]
    ctx = fusion_hip.Context(q, d, P["root"], P["inv_root"])
    errors = []

    def churn(seed):
        rng = np.random.default_rng(seed)
        held = []
        try:
            for _ in range(300):
                if held and rng.random() < 0.5:
                    ctx.free(held.pop(int(rng.integers(len(held)))))
                else:
                    held.append(ctx.malloc(int(rng.integers(256 << 10, 3 << 20))))
            for p in held:
                ctx.free(p)
        except Exception as e:                      # noqa: BLE001 - surfaced below
            errors.append(repr(e))
    threads = [threading.Thread(target=churn, args=(s,)) for s in range(6)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    # (2) free on stream A, switch to stream B, reuse: the transform queued on A before the free still reads the old contents
    rows = 1 << 14
    x = O.splitmix_centered(3, rows * d).reshape(rows, d)
    want = ctx.ntt_forward(x)
    sa, sb = ctx.stream_create(), ctx.stream_create()
    ctx.set_stream(sa)
    a, out = ctx.malloc(x.nbytes), ctx.malloc(x.nbytes)
    ctx.h2d(a, x)
    for _ in range(20):
        ctx.ntt_forward_dev(a, out, rows)              # queued on A: reads a
    ctx.free(a)
    ctx.set_stream(sb)                                 # only pooled / live blocks exist: round 3 skipped the drain here
    b = ctx.malloc(x.nbytes)
    assert b == a
    ctx.fill_synthetic_dev(b, rows * d, 9)             # on B: must not overtake the transforms on A
    got = np.empty_like(x)
    ctx.d2h(got, out)
    assert np.array_equal(got, want)
    ctx.free(b)
    ctx.free(out)
    ctx.pool_trim(0)                                   # (3) everything idle goes back to the runtime
    c = ctx.malloc(x.nbytes)
    ctx.free(c)
    ctx.set_stream(0)
    ctx.stream_destroy(sa)
    ctx.stream_destroy(sb)
    ctx.close()
    # (4) two contexts, a 20 MiB budget for the process: three 8 MiB blocks freed through either context -- at most two stay
    monkeypatch.setenv("FZ_POOL_MB", "20")
    c1 = fusion_hip.Context(q, d, P["root"], P["inv_root"])
    c2 = fusion_hip.Context(q, d, P["root"], P["inv_root"])
    monkeypatch.delenv("FZ_POOL_MB")
    p1, p2, p3 = c1.malloc(1 << 23), c1.malloc(1 << 23), c2.malloc(1 << 23)
    c1.free(p1)
    c1.free(p2)
    c2.free(p3)                                        # over the shared budget: c2 holds nothing it could drop, so p3 is not kept
    assert c2.malloc(1 << 23) != p3 or True            # (whatever hipMalloc returns: the point is that nothing crashes or leaks)
    assert c1.malloc(1 << 23) in (p1, p2)
    c1.close()
    c2.close()


def test_bench_headline_keeps_its_streams_with_rccl_in_the_process():
    """An N > 1 run of bench.py has a torch.distributed "nccl" group and a C-ABI communicator in its process, and RCCL takes
    hardware queues for its own streams: chains created AFTER it share queues and the multi-stream headline falls to 0.7-1.4 x
    the one-stream rate (profiles/r04_hw_queue_oversubscription.txt).  bench.py creates its chains first; rehearsed here on one
    GPU with communicators of ONE rank (--single-rank-comm).  The check is inside one run: the device timestamps must show the
    two chains' launches overlapping, and two streams must beat one."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--full", "--headline-only", "--single-rank-comm", "--full-out", os.devnull],
                       capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')][-1]
    d = json.loads(line)
    assert d["ranks"]["n"] == 1 and d["ranks"]["same"]["rccl_nranks"] == 1 and d["config"]["streams"] == 2
    one, chip = d["roofline"]["frac"], d["roofline"]["chip"]["frac"]
    dev = d["roofline"]["chip"]["device_clock"]
    # by the chip's own clock: the two chains' launches really ran side by side (queue-sharing chains run one after the other)
    assert dev["in_flight"] > 1.5, f"{dev}: the chains share a hardware queue"
    assert chip > 1.05 * one, f"two streams reach {chip:.3f} of the peak against {one:.3f} on one"


def test_bench_plain_run_times_its_steps_and_dumps_the_last_step(coracle, tmp_path):
    """A plain bench.py run (no --full) times exactly --steps steps and measures nothing else; --dump-outputs writes what the
    last of them computed.  K = 37 steps on 2 chains: step 36 is chain 0's 19th, whose batch is rotation index 18 (seed
    20261003 + 18 000): the inverse output is that batch, the forward output its transforms by the oracle."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    full_out, dump = tmp_path / "full.json", tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "37", "--warmup", "3",
                        "--dump-outputs", str(dump), "--full-out", str(full_out)], capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')][-1])
    assert d["steps"] == 37 and d["warmup"] == 3 and d["unit"] == "NTT/s" and d["dtype"] == "f64" and d["higher_is_better"] is True
    assert d["value"] > 0 and d["ms_per_step"] > 0 and "the 37 steps" in d["config"]["launch"] and d["config"]["streams"] == 2
    assert d["roofline"] == {} and d["cpu_baseline"] is None and "sign_verify" not in d and "full" not in d
    assert not full_out.exists()
    fwd, inv = np.load(dump / "ntt_forward.npy"), np.load(dump / "ntt_inverse.npy")
    assert fwd.dtype == inv.dtype == np.float64 and fwd.shape == inv.shape == (4096, 256)
    P = O.PARAMS[256]
    x = O.splitmix_centered(20261003 + 18 * 1000, 4096 * 256).reshape(4096, 256)
    assert np.array_equal(inv, x.astype(np.float64))
    assert np.array_equal(fwd, coracle.ntt_forward(x, P["q"], P["root"]).astype(np.float64))


def test_bench_sign_verify_leg_with_the_exchange_on_its_second_stream():
    """bench.py's sign_verify leg as an N > 1 run executes it, rehearsed on one GPU: a one-rank RCCL communicator (so the
    all-reduce is a real RCCL launch inside the captured graph, on the high-priority exchange stream, ordered by fz_event_*) plus
    a 20 us stand-in for the exchange's latency; the leg asserts every verdict itself.  Its rate must stay within reach of the
    plain run's (an exchange serialised behind sign_core's workgroups more than doubles the step)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    vals = {}
    for name, extra in (("plain", []), ("exchange", ["--single-rank-comm", "--exchange-standin-us", "20"])):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--full", "--no-extra-legs", "--no-cpu-baseline", "--full-out", os.devnull] + extra,
                           capture_output=True, text=True, timeout=400, cwd=root)
        assert r.returncode == 0, r.stderr[-2000:]
        d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')][-1])
        sv = d["sign_verify"]
        assert "error" not in sv and sv["value"] > 0, sv
        vals[name] = sv["ms_per_step"]
        if extra:
            assert "RCCL counts 1 rank" in sv["collective"]
    assert vals["exchange"] < 1.6 * vals["plain"], vals


def test_the_library_says_which_transform_schedule_a_launch_takes(monkeypatch):
    """fz_diag_ntt_schedule: bench.py names its dominant kernel by it (no mirrored crossover): radix-4 wave-tasks below 24 576 rows
    at degree 256, 16 per lane from there; FZ_NTT_KERNEL forces either; degree 128 has no radix-4 kernels; degree 16 neither family"""
    import fusion_hip
    P = O.PARAMS[256]
    ctx = fusion_hip.Context(Q, 256, P["root"], P["inv_root"])
    assert [ctx.diag_ntt_schedule(r) for r in (1, 4096, 24575, 24576, 65536, 1 << 22)] == [4, 4, 4, 16, 16, 16]
    monkeypatch.setenv("FZ_NTT_KERNEL", "16")
    assert fusion_hip.Context(Q, 256, P["root"], P["inv_root"]).diag_ntt_schedule(1) == 16
    monkeypatch.setenv("FZ_NTT_KERNEL", "4")
    assert fusion_hip.Context(Q, 256, P["root"], P["inv_root"]).diag_ntt_schedule(1 << 22) == 4
    monkeypatch.delenv("FZ_NTT_KERNEL")
    q2 = 65537
    r128 = next(r for r in (pow(g, (q2 - 1) // 256, q2) for g in range(2, 200)) if pow(r, 128, q2) == q2 - 1)
    assert fusion_hip.Context(q2, 128, r128, pow(r128, q2 - 2, q2)).diag_ntt_schedule(10) == 16
    r16 = next(r for r in (pow(g, (q2 - 1) // 32, q2) for g in range(2, 200)) if pow(r, 16, q2) == q2 - 1)
    assert fusion_hip.Context(q2, 16, r16, pow(r16, q2 - 2, q2)).diag_ntt_schedule(10) == 0
