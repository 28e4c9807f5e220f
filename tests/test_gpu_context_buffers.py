"""The rule of the context's growable device areas (fz_area_replace, csrc/fz_context.hip) on the real runtime: a captured
sequence that would make an area grow is refused with an argument error BEFORE any runtime call, so the open capture stays
valid and ends in a graph that works; the same calls succeed outside the capture, and the graph keeps replaying from the areas
that were retired for it.  (tests/test_context_host.py checks the same rule call by call against a stub runtime.)"""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu


def test_growth_is_refused_inside_a_capture_and_the_capture_survives(coracle):
    import fusion_hip
    P = O.PARAMS[128]
    q, d, l = P["q"], P["d"], 2
    ctx = fusion_hip.Context(q, d, P["root"], P["inv_root"])
    s = ctx.stream_create()
    ctx.set_stream(s)
    rng = np.random.default_rng(2026)
    DB = fusion_hip.DeviceBuffer
    bufs = []

    def dev(a):
        bufs.append(DB.from_numpy(ctx, a) if isinstance(a, np.ndarray) else DB(ctx, a))
        return bufs[-1]

    def cent(x):
        return ((x + q // 2) % q - q // 2).astype(np.int32)
    # One aggregate of 144 signers at (l, d) = (2, 64).  fz_launch_aggregate: 144 signers are more than the 128 of the slice-free
    # kernel; l * d / 4 = 32 int4 columns are ONE column block at every block width; slices = min(CUs / 1 block, 144 / (8 waves x 3
    # signers in flight)) = 6 > 1, so the launch uses the accumulator words: 1 tile, capacity 1 + 1/4 + 8 = 9 tiles.  Ten such
    # aggregates in one launch: min(CUs / 10, 6) = 6 slices again and 10 tiles > 9.
    # Verification of one aggregate: d = 64 accumulator doubles, capacity 64 + 64/4 = 80; two aggregates need 128 > 80.
    n, many = 144, 10
    sig = rng.integers(-(q // 2), q // 2, size=(many * n, l, d)).astype(np.int32)
    al = rng.integers(-(q // 2), q // 2, size=(many * n, d)).astype(np.int32)
    A = O.splitmix_centered(5, l * d).reshape(l, d)
    want = [coracle.aggregate_core(sig[g * n:(g + 1) * n], al[g * n:(g + 1) * n], q) for g in range(many)]
    # verdicts: beta = q and omega = l * d bound nothing, so an aggregate against its own image is accepted (0) and against
    # another target refused (3)
    two = np.stack(want[:2])
    targets = coracle.matvec(A, two, q).astype(np.int32)
    targets[1, 3] += 1
    dA, d_sig, d_al = dev(A), dev(sig), dev(al)
    d_out, d_verd = dev(l * d * 4), dev(4)
    d_two, d_tgt, d_verd2, d_part = dev(two), dev(targets), dev(2 * 4), dev(many * l * d * 8)

    def small():
        ctx.aggregate_core_dev(d_sig.ptr, d_al.ptr, d_out.ptr, n, l)
        ctx.verify_with_target_batch_async_dev(dA.ptr, d_out.ptr, d_tgt.ptr, 1, l, q, l * d, d_verd.ptr)

    def check_small():
        assert np.array_equal(d_out.to_numpy(np.int32, (l, d)), want[0])
        assert d_verd.to_numpy(np.int32, (1,)).tolist() == [0]

    # 1. un-captured: sizes the areas
    small()
    check_small()
    # 2. captured: the same calls fit; the larger ones are refused and leave the capture open and valid
    ctx.graph_begin()
    small()
    for larger in (lambda: ctx.verify_with_target_batch_async_dev(dA.ptr, d_two.ptr, d_tgt.ptr, 2, l, q, l * d, d_verd2.ptr),
                   lambda: ctx.aggregate_partial_batch_dev(d_sig.ptr, d_al.ptr, d_part.ptr, l * d, many, n, l)):
        with pytest.raises(fusion_hip.FusionHipError) as e:
            larger()
        assert e.value.code == -1 and "graph capture" in str(e.value)
    # 3. the capture ends in a graph that works
    g = ctx.graph_end()
    ctx.h2d(d_out.ptr, np.zeros((l, d), np.int32))
    ctx.h2d(d_verd.ptr, np.full(1, -1, np.int32))
    g.launch()
    check_small()
    # 4. outside the capture the larger calls succeed (the areas grow; the graph's are retired, not freed)
    ctx.verify_with_target_batch_async_dev(dA.ptr, d_two.ptr, d_tgt.ptr, 2, l, q, l * d, d_verd2.ptr)
    ctx.aggregate_partial_batch_dev(d_sig.ptr, d_al.ptr, d_part.ptr, l * d, many, n, l)
    assert d_verd2.to_numpy(np.int32, (2,)).tolist() == [0, 3]
    part = d_part.to_numpy(np.int64, (many, l, d))
    for k in range(many):
        assert np.array_equal(cent(part[k]), want[k]), k
    ctx.h2d(d_out.ptr, np.zeros((l, d), np.int32))
    ctx.h2d(d_verd.ptr, np.full(1, -1, np.int32))
    g.launch()
    check_small()
    g.destroy()
    ctx.set_stream(0)
    ctx.stream_destroy(s)
    for b in bufs:
        b.free()
    ctx.close()
