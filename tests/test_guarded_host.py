"""tests/_guarded.py on its numpy backend: a fake entry (out[r][j] = a[r][j] + b[j], rows `stride` apart) that is correct passes;
the same entry with one planted fault at a time fails, and the message names the operand and the index."""
import numpy as np
import pytest

import _guarded as G

ROWS, ROW, STRIDE = 3, 5, 8


def _operands(offset=0, dtype=np.int32):
    rng = np.random.default_rng(7)
    a = G.any_int32(rng, (ROWS, ROW)).astype(dtype)
    b = G.any_int32(rng, (ROW,)).astype(dtype)
    want = (a.astype(np.int64) + b.astype(np.int64)).astype(dtype)           # wraps like the fake entry does
    return [G.inp("a", a, stride=STRIDE, offset=offset), G.inp("b", b, offset=offset),
            G.out("out", want, stride=STRIDE, offset=offset)]


def _entry(fault=None):
    """the fake entry; p[name].ptr is a view that begins at the interior's first element (negative indices: before it)"""
    def call(p):
        a, b, o = p["a"].ptr, p["b"].ptr, p["out"].ptr
        base = {n: p[n].handle for n in p}
        lead = {n: len(base[n]) - len(p[n].ptr) for n in p}
        with np.errstate(over="ignore"):
            for r in range(ROWS):
                for j in range(ROW):
                    if fault == "stale" and (r, j) == (1, 2):
                        continue
                    x = a[r * STRIDE + j]
                    if fault == "reads_guard" and (r, j) == (2, ROW - 1):
                        x = a[r * STRIDE + j + 1]                             # one past the end of a's last row
                    o[r * STRIDE + j] = x + b[j]
        if fault == "before":
            base["out"][lead["out"] - 1] = 1
        if fault == "after":
            o[(ROWS - 1) * STRIDE + ROW] = 1
        if fault == "gap":
            o[1 * STRIDE + ROW + 2] = 1
        if fault == "flip":
            base["b"][lead["b"] + 3] ^= 4
        return "done"
    return call


@pytest.mark.parametrize("offset,dtype", [(0, np.int32), (4, np.int32), (0, np.int64)])     # (the 4-byte offset: int32 operands only)
def test_the_correct_entry_passes(offset, dtype):
    assert G.run_case(G.HostBackend(), _operands(offset, dtype), _entry()) == ["done", "done"]


FAULTS = {
    "before": r"out: guard word written: lead guard, 1 element\(s\) before the interior \(index -1\)",
    "after": rf"out: guard word written: trail guard, 0 element\(s\) after the interior \(index {(ROWS - 1) * STRIDE + ROW}\)",
    "gap": rf"out: guard word written: stride gap after row 1, gap word 2 \(index {STRIDE + ROW + 2}\)",
    "flip": r"b: input changed: row 0, column 3 \(index 3\)",
    "stale": rf"out: output differs from the expectation: row 1, column 2 \(index {STRIDE + 2}\): got \d+ \(still the previous contents\)",
    "reads_guard": rf"out: output depends on the fill: row 2, column {ROW - 1} \(index {2 * STRIDE + ROW - 1}\)",
}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_each_planted_fault_is_reported_with_operand_and_index(fault):
    with pytest.raises(G.GuardError, match=FAULTS[fault]):
        G.run_case(G.HostBackend(), _operands(), _entry(fault))


def test_a_clean_run_reports_nothing_and_faults_do_not_leak_between_cases():
    G.run_case(G.HostBackend(), _operands(), _entry())
    with pytest.raises(G.GuardError):
        G.run_case(G.HostBackend(), _operands(), _entry("after"))
    G.run_case(G.HostBackend(), _operands(), _entry())


def test_layout():
    """guards of at least 16 KiB on either side, the interior at 16 k (+ 4) bytes, the gap words in the guard"""
    for offset in (0, 4):
        ar = G.Arena(_operands(offset)[0])
        assert ar.byte_offset % 16 == offset and ar.byte_offset >= 16384
        assert (ar.total - ar.lead - ar.span) * 4 >= 16384
        assert int(ar.interior.sum()) == ROWS * ROW and not ar.interior[ar.lead + ROW] and ar.interior[ar.lead + STRIDE]
    ar = G.Arena(G.out("p", np.zeros((2, 3), np.int64), stride=4))
    assert ar.lead * 8 == 16384 and (ar.total - ar.lead - ar.span) * 8 == 16384
    img = ar.image(G.FILLS[0])
    assert int(img.view(np.uint64)[0]) == 0x5a5a5a5a5a5a5a5a
    assert int(ar.image(G.FILLS[1]).view(np.uint64)[0]) == 0x8000000080000000


def test_a_refused_call_must_leave_every_word():
    class Refused(Exception):
        code = -1

    def refuses(p):
        raise Refused()

    def refuses_late(p):
        p["out"].ptr[0] = 0
        raise Refused()

    G.run_refusal(G.HostBackend(), _operands(), refuses, -1)
    with pytest.raises(G.GuardError, match=r"out: written by a refused call: row 0, column 0 \(index 0\)"):
        G.run_refusal(G.HostBackend(), _operands(), refuses_late, -1)
    with pytest.raises(AssertionError, match="expected refusal code -1"):
        G.run_refusal(G.HostBackend(), _operands(), lambda p: None, -1)


# ---- expectations the GPU files compose from oracle steps, and the route model they assert with ---------------------------------
def test_the_composed_product_expectation_is_the_negacyclic_product(coracle):
    """test_gpu_guarded_transforms.py expects INTT(NTT(f) . NTT(g)) from the oracle's transforms: for any int32 operands that is the
    centred schoolbook product mod (X^d + 1), in Python integers"""
    from oracle import oracle as O
    q, d = O.PRIME, 32
    root, inv = G.root_pair(q, d)
    rng = np.random.default_rng(3)
    f, g = G.any_int32(rng, (1, d)), G.any_int32(rng, (1, d))
    want = coracle.ntt_inverse(coracle.pw_mul(coracle.ntt_forward(f, q, root), coracle.ntt_forward(g, q, root), q), q, inv).reshape(d)
    conv = [0] * (2 * d)
    for i, x in enumerate(f[0]):
        for j, y in enumerate(g[0]):
            conv[i + j] += int(x) * int(y)
    assert want.tolist() == [O.py_cent(a - b, q) for a, b in zip(conv[:d], conv[d:])]


def test_matvec_route_model():
    """tests/_saturation.py: matvec_route restates fz_launch_matvec's choice; the shapes test_gpu_guarded_scheme.py relies on, at 256 CUs"""
    import _saturation as S
    cu = 256
    assert S.matvec_route(0, 3, 5, 16, cu) == "split" and S.matvec_route(0, 3, 5, 4096, cu) == "split"
    assert S.matvec_route(0, 2 * cu + 1, 8, 64, cu) == ("sliced", 1)                 # waves1 = 129 * 16 / 64 -> by the wave count, then l / ks >= 8
    assert [S.matvec_route(k, 3, 131, 64, cu) for k in (1, 2, 4, 8, 16)] == [("sliced", k) for k in (1, 2, 4, 8, 16)]
    assert [S.matvec_route(16, 3, l, 64, cu) for l in (8, 17, 131)] == [("sliced", 1), ("sliced", 2), ("sliced", 16)]
    assert S.matvec_route(-1, 3, 8, 64, cu) == "split" and S.matvec_route(-1, 3, 8, 12, cu) == "kernel"
    assert S.matvec_route(-1, 4096, 8, 64, cu) == "kernel" and S.matvec_route(4, 3, 32769, 64, cu) == "kernel"
    assert S.matvec_route(0, 3, 8, 13, cu) == "scalar" and S.matvec_route(4, 3, 8, 64, cu, aligned=False) == "scalar"
    # the model agrees with matvec_sliced_taken wherever that one applies (aligned int4 rows of a power-of-two degree)
    for knob in (-1, 0, 1, 16):
        for batch in (1, 3, 2 * cu + 1):
            for l in (8, 131, 32769):
                assert (S.matvec_route(knob, batch, l, 64, cu)[0] == "sliced") == S.matvec_sliced_taken(knob, batch, l, 64, cu)
