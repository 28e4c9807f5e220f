"""hash_ag for many committees on the device (fz_hash_ag_ragged_dev: a wave per committee) on a GPU.

Pinned to the reference: the committees of tests/golden/scheme_many_{128,256}.npz (32, 5, 12, 15 signers at secpar 128; 16, 3, 6, 7 at
256) and the first 1, 2 and 4 signers of tests/golden/scheme_{128,256}.npz, all groups of a file in ONE ragged call, bit for bit
against the reference's alpha_hat, mapped through its order.  Any secpar-256 committee takes the j = 0 draws (195 shuffle draws,
index bytes for 60).
Pinned to the host pipeline: the fixtures of tests/_hash_ag_edges.py (text lengths on every padding edge, piece boundaries on
block boundaries, extreme values and digests, streams that end on block boundaries, ragged layouts), whose rows
tests/test_hash_ag_edges_host.py holds to fz_aggregation_coefficients and to a plain-Python model; transforms by the C oracle.
Through the scheme: the five many-committee methods of BatchScheme return under hash_ag="device" bit for bit what they return
under "host"."""
import copy
import json
import os

import numpy as np
import pytest

import _hash_ag_edges as H
from _challenge_edges import SETS

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
POISON = 0x5A5A5A5A
ALL_SETS = ("s128", "s256", "d128w64", "d16", "d4")


def _run(ctx, P, vk, pre, c, order, off, d, guard=2):
    """one call of the entry on host arrays: -> alpha_hat [N][d]; the output sits between `guard` poisoned rows on either side,
    which must keep their poison"""
    import fusion_hip
    n = len(vk)
    bufs = [fusion_hip.DeviceBuffer.from_numpy(ctx, np.ascontiguousarray(a)) for a in (vk, pre, c)]
    dout = fusion_hip.DeviceBuffer(ctx, (n + 2 * guard) * d * 4)
    try:
        ctx.h2d(dout.ptr, np.full((n + 2 * guard, d), POISON, dtype=np.int32))
        ctx.hash_ag_ragged_dev(P, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, n, order, off, dout.ptr + guard * d * 4)
        got = dout.to_numpy(np.int32, (n + 2 * guard, d))
        assert (got[:guard] == POISON).all() and (got[n + guard:] == POISON).all(), "a row outside the output was written"
        return got[guard:n + guard]
    finally:
        for b in bufs + [dout]:
            b.free()


# ---- pinned to the reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("secpar", [128, 256])
def test_golden_committees_in_one_ragged_call(secpar):
    import fusion.fusion as F
    from fusion_hip.scheme import BatchScheme
    S = np.load(os.path.join(G, f"scheme_many_{secpar}.npz"))
    with open(os.path.join(G, "scheme_many.json")) as fh:
        m = json.load(fh)[str(secpar)]
    sizes = [hi - lo for lo, hi in m["subsets"]]
    assert sizes == ([32, 5, 12, 15] if secpar == 128 else [16, 3, 6, 7])
    params = F.fusion_setup(secpar, m["setup_seed"])
    bs = BatchScheme(params)
    rows = np.concatenate([np.arange(lo, hi) for lo, hi in m["subsets"]])      # the committees overlap: every one gets its own rows
    dC, dAl, off = bs.hash_ag_many_dev(S["vk"][rows], [m["messages"][r] for r in rows], sizes)
    try:
        alpha = dAl.numpy()
        assert np.array_equal(dC.numpy(), bs.challenges(S["vk"][rows], [m["messages"][r] for r in rows])[0])
    finally:
        dC.free()
        dAl.free()
        bs.close()
    assert off.tolist() == np.concatenate([[0], np.cumsum(sizes)]).tolist()
    for g, (lo, hi) in enumerate(m["subsets"]):
        mine = alpha[off[g]:off[g + 1]]
        assert np.array_equal(mine[m["agg"][f"{lo}_{hi}"]["order"]], S[f"alpha_hat_sorted_{lo}_{hi}"]), (lo, hi)


@pytest.mark.parametrize("secpar", [128, 256])
def test_golden_first_signers_in_one_ragged_call(secpar):
    import fusion.fusion as F
    from fusion_hip import hostpipe
    from fusion_hip.scheme import BatchScheme
    S = np.load(os.path.join(G, f"scheme_{secpar}.npz"))
    with open(os.path.join(G, "scheme.json")) as fh:
        m = json.load(fh)[str(secpar)]
    params = F.fusion_setup(secpar, m["setup_seed"])
    bs = BatchScheme(params)
    rows = np.concatenate([np.arange(k) for k in (1, 2, 4)])
    pre = hostpipe.hash_messages(bs.P, [m["messages"][r] for r in rows])
    order = np.concatenate([np.array(m["agg"][str(k)]["order"]) + base for k, base in ((1, 0), (2, 1), (4, 3))])
    try:
        got = _run(bs.ctx, bs.P, S["vk"][rows], pre, S["c_hat"][rows], order, [0, 1, 3, 7], bs.d)      # the reference's own c_hat
    finally:
        bs.close()
    for k, base in ((1, 0), (2, 1), (4, 3)):
        assert np.array_equal(got[base:base + k][m["agg"][str(k)]["order"]], S[f"alpha_hat_{k}"]), k


# ---- pinned to the host pipeline ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def contexts():
    import fusion_hip
    made = {}

    def get(set_name):
        if set_name not in made:
            ps = SETS[set_name]
            made[set_name] = fusion_hip.Context(ps.modulus, ps.degree, ps.root, ps.inv_root)
        return made[set_name]
    yield get
    for c in made.values():
        c.close()


@pytest.mark.parametrize("set_name", ALL_SETS)
def test_edge_committees(set_name, contexts, coracle):
    """every committee fixture of the set as one group of ONE ragged call (G groups of different sizes, longest first in the
    launch), and the first, the last and the longest again as calls of their own (G = 1): the same rows"""
    from fusion_hip import hostpipe
    ps, cases, rows = SETS[set_name], H.all_cases(set_name), H.case_rows(set_name)
    d = ps.degree
    P, ctx = hostpipe.scheme_params(ps), contexts(set_name)
    vk, pre, c = (np.concatenate([getattr(k, f) for k in cases]) for f in ("vk", "pre", "c"))
    off = np.concatenate([[0], np.cumsum([len(k.vk) for k in cases])])
    want = coracle.ntt_forward(np.concatenate([rows[k.name] for k in cases]), ps.modulus, ps.root).reshape(-1, d)
    got = _run(ctx, P, vk, pre, c, np.arange(off[-1]), off, d)
    for g, k in enumerate(cases):
        assert np.array_equal(got[off[g]:off[g + 1]], want[off[g]:off[g + 1]]), k.name
    longest = int(np.argmax(np.diff(off)))
    for g in sorted({0, len(cases) - 1, longest}):
        k = cases[g]
        alone = _run(ctx, P, k.vk, k.pre, k.c, np.arange(len(k.vk)), [0, len(k.vk)], d)
        assert np.array_equal(alone, want[off[g]:off[g + 1]]), k.name


@pytest.mark.parametrize("set_name", ["s128", "s256"])
def test_ragged_layout(set_name, contexts, coracle):
    """one more group than a multiple of the workgroup's waves, different sizes, an order list that permutes the whole row range:
    rows that no group names come back all zero, the guard rows keep their poison, and every group's rows are bit for bit those of
    the call with that group alone"""
    from fusion_hip import hostpipe
    ps = SETS[set_name]
    d = ps.degree
    P, ctx = hostpipe.scheme_params(ps), contexts(set_name)
    vk, pre, c, order, off, want = H.layout_call(set_name)
    hat = coracle.ntt_forward(want, ps.modulus, ps.root).reshape(-1, d)
    got = _run(ctx, P, vk, pre, c, order, off, d)
    named = np.zeros(len(vk), dtype=bool)
    named[order] = True
    assert (got[~named] == 0).all() and (~named).sum() == 5
    assert np.array_equal(got, hat)
    for g in range(len(off) - 1):
        rows = order[int(off[g]):int(off[g + 1])]
        alone = _run(ctx, P, vk, pre, c, rows, [0, len(rows)], d)
        assert np.array_equal(alone[rows], got[rows]) and (np.delete(alone, rows, axis=0) == 0).all(), g


def test_nothing_to_hash_and_refusals_write_nothing(contexts):
    import fusion_hip
    from fusion_hip import hostpipe
    from fusion_hip._lib import FZ_E_BADARG, FZ_E_UNSUPPORTED, FusionHipError
    ps = SETS["s128"]
    d = ps.degree
    P, ctx = hostpipe.scheme_params(ps), contexts("s128")
    vk, pre, c = H.base_rows(ps, 3, 70)
    none = _run(ctx, P, vk, pre, c, np.zeros(0, dtype=np.uint32), [0], d)          # G = 0: N zero rows, no kernel
    assert (none == 0).all()
    bad = copy.copy(ps)
    bad.beta_ag = 2
    bufs = [fusion_hip.DeviceBuffer.from_numpy(ctx, np.ascontiguousarray(a)) for a in (vk, pre, c)]
    dout = fusion_hip.DeviceBuffer(ctx, 3 * d * 4)
    try:
        ctx.h2d(dout.ptr, np.full((3, d), POISON, dtype=np.int32))
        for params, order, off, code in ((hostpipe.scheme_params(bad), [0, 1, 2], [0, 3], FZ_E_UNSUPPORTED),
                                         (P, [0, 1, 1], [0, 3], FZ_E_BADARG), (P, [0, 1, 3], [0, 3], FZ_E_BADARG),
                                         (P, [0, 1, 2], [0, 1, 1, 3], FZ_E_BADARG)):
            with pytest.raises(FusionHipError) as e:
                ctx.hash_ag_ragged_dev(params, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, 3, order, off, dout.ptr)
            assert e.value.code == code
        assert (dout.to_numpy(np.int32, (3, d)) == POISON).all()
    finally:
        for b in bufs + [dout]:
            b.free()


# ---- through the scheme ----------------------------------------------------------------------------------------------------------------
def _same(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b


@pytest.mark.parametrize("secpar", [128, 256])
def test_many_committee_methods_device_equals_host(secpar, monkeypatch):
    """the golden committees, one of them split so that its last signer is a group of its own; then with one tampered record
    (screened=True: code 3) and with that lone signer's record not canonical (a group with no accepted signer)"""
    import fusion.fusion as F
    from fusion_hip import hostpipe
    from fusion_hip.context import Context
    from fusion_hip.scheme import BatchScheme
    S = np.load(os.path.join(G, f"scheme_many_{secpar}.npz"))
    with open(os.path.join(G, "scheme_many.json")) as fh:
        m = json.load(fh)[str(secpar)]
    params = F.fusion_setup(secpar, m["setup_seed"])
    parts = m["subsets"][1:]
    sizes = [hi - lo for lo, hi in parts]
    sizes = sizes[:-1] + [sizes[-1] - 1, 1]
    msgs = m["messages"]
    host, dev = BatchScheme(params, hash_ag="host"), BatchScheme(params, hash_ag="device")
    calls = []
    entry = Context.hash_ag_ragged_dev
    monkeypatch.setattr(Context, "hash_ag_ragged_dev", lambda self, *a: (calls.append(len(a[5])), entry(self, *a))[1])
    try:
        sk, vk = host.keygen_batch(m["key_seeds"])
        sig = host.sign_batch(sk, vk, msgs)
        data, codes = host.encode("signature", sig)
        assert not codes.any()
        aggs = host.aggregate_many(vk, msgs, sig, sizes)
        for g, (lo, hi) in enumerate(parts[:-1]):
            assert np.array_equal(aggs[g], S[f"agg_{lo}_{hi}"])
        arecs = host.encode("aggregate", aggs)[0]
        tampered = data.copy()
        tampered[3, 5] ^= 1                                 # still canonical, no longer the signer's: code 3 under screened=True
        lone = data.copy()
        lone[-1] = 0xff                                     # not canonical: code 6, and its group has no accepted signer
        runs = {
            "aggregate_many": lambda bs: bs.aggregate_many(vk, msgs, sig, sizes),
            "verify_many": lambda bs: bs.verify_many(vk, msgs, aggs, sizes),
            "verify_many_encoded": lambda bs: bs.verify_many_encoded(vk, msgs, arecs, sizes),
            "aggregate_many_encoded": lambda bs: bs.aggregate_many_encoded(vk, msgs, data, sizes),
            "aggregate_many_encoded[screened, tampered]": lambda bs: bs.aggregate_many_encoded(vk, msgs, tampered, sizes, screened=True),
            "aggregate_many_encoded[no accepted signer]": lambda bs: bs.aggregate_many_encoded(vk, msgs, lone, sizes, encoded=True),
            "aggregate_verify_many_encoded": lambda bs: bs.aggregate_verify_many_encoded(vk, msgs, data, sizes),
            "aggregate_verify_many_encoded[no accepted signer]": lambda bs: bs.aggregate_verify_many_encoded(vk, msgs, lone, sizes),
        }
        for name, run in runs.items():
            want = run(host)
            assert not calls, name
            with monkeypatch.context() as mp:
                mp.setattr(hostpipe, "aggregation_coefficients", lambda *a, **k: pytest.fail("the host's hash_ag ran"))
                got = run(dev)
            assert len(calls) == 1, name
            entries = calls.pop()
            assert _same(got, want), name
            if "tampered" in name:
                assert want[1][3] != 0 and not np.delete(want[1], 3).any() and entries == sum(sizes) - 1
            if "no accepted" in name:
                assert want[1][-1] == 6 and entries == sum(sizes) - 1
                if name.startswith("aggregate_verify"):         # rows: the group's aggregate is zero and it has no verdict
                    assert (want[0][-1] == 0).all() and want[2][-1] is None and want[2][0] == (True, "")
        assert dev.device_hash_ag
    finally:
        host.close()
        dev.close()


def test_auto_falls_back_on_a_parameter_set_the_kernel_does_not_take(monkeypatch):
    import fusion.fusion as F
    from fusion_hip import scheme
    params = copy.copy(F.fusion_setup(128, 9))
    params.beta_ag = 2                                      # coefficients in {-2, .., 2}: the host pipeline's alone
    monkeypatch.setattr(scheme, "_HASH_AG_HOST_US", 1e6)    # "auto" predicts the device form for any sizes
    host, auto = scheme.BatchScheme(params, hash_ag="host"), scheme.BatchScheme(params, hash_ag="auto")
    try:
        sizes = [2, 1, 3]
        msgs = [f"m{i}" for i in range(6)]
        sk, vk = host.keygen_batch([900 + i for i in range(6)])
        sig = host.sign_batch(sk, vk, msgs)
        assert auto._hash_ag_form(sizes) == "device"
        got = auto.aggregate_many(vk, msgs, sig, sizes)
        assert auto.device_hash_ag is False and auto._hash_ag_form(sizes) == "host"
        assert np.array_equal(got, host.aggregate_many(vk, msgs, sig, sizes))
        assert np.array_equal(auto.aggregate_many(vk, msgs, sig, sizes), got)
    finally:
        host.close()
        auto.close()


def test_drop_in_face_passes_the_option_on(monkeypatch):
    import fusion.fusion as F
    from fusion_hip.context import Context
    params = F.fusion_setup(128, 9)
    keys = [F.keygen(params, 700 + i) for i in range(4)]
    msgs = [f"drop-in {i}" for i in range(4)]
    blobs = [F.sign_to_bytes(params, k, mm) for k, mm in zip(keys, msgs)]
    kg, mg, bg = [[k[1] for k in keys[:1]], [k[1] for k in keys[1:]]], [msgs[:1], msgs[1:]], [blobs[:1], blobs[1:]]
    calls = []
    entry = Context.hash_ag_ragged_dev
    monkeypatch.setattr(Context, "hash_ag_ragged_dev", lambda self, *a: (calls.append(1), entry(self, *a))[1])
    want = F.aggregate_verify_many_from_bytes(params, kg, mg, bg)
    assert not calls
    got = F.aggregate_verify_many_from_bytes(params, kg, mg, bg, hash_ag="device")
    assert len(calls) == 1 and got[1] == want[1] == [(True, ""), (True, "")]
    assert [str(a) for a in got[0]] == [str(a) for a in want[0]]
    aggs = F.aggregate_many_from_bytes(params, kg, mg, bg, hash_ag="device")
    assert [str(a) for a in aggs] == [str(a) for a in want[0]]
    recs = [F.to_bytes(params, a, aggregate=True) for a in aggs]
    assert F.verify_many_from_bytes(params, kg, mg, recs, hash_ag="device") == [(True, ""), (True, "")] and len(calls) == 3
