"""Many committees aggregated AND their verification targets formed straight from the compact bytes in one launch
(fz_aggregate_target_encoded_ragged_async, BatchScheme.aggregate_verify_encoded / aggregate_verify_many_encoded,
fusion.fusion.aggregate_verify_from_bytes / aggregate_verify_many_from_bytes), on the CPU: the census of the new translation unit,
its register and LDS budget against aggregate_encoded_ragged's -- the launcher sizes its grid by that kernel's resident grid, which
is sound only while the new kernel's allocation is no larger --, the binding of the C entry, the refusals that happen before a
device is touched, and on the stand-in context of tests/_scheme_buffers.py how often each step of the one pass runs.  The device
tests are tests/test_gpu_aggregate_target_encoded.py, the entry's refusal ladder tests/test_aggregate_target_encoded_entries_host.py."""
import copy
import functools
import os
import re
import types

import numpy as np
import pytest

from _scheme_buffers import no_finalizers, scheme_on, stand_in_context
from test_aggregate_encoded_host import _scheme_without_device
from test_encoding_host import TABLE, params_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = r"ILi(\d)ELb(\d)E"


def test_new_unit_holds_the_four_instantiations_within_the_ragged_kernels_budget():
    """fz_aggregate_target_encoded: aggregate_target_encoded_ragged for degrees 64 and 256 x both multiply forms and nothing else;
    no spill, no scratch; per (LOGD, FAST) no more VGPRs and no more LDS than aggregate_encoded_ragged"""
    import __graft_entry__ as GE
    from _isa import asm, metadata
    assert "fz_aggregate_target_encoded.hip" in GE.SOURCES and "fz_aggregate_target_encoded_capi.hip" in GE.SOURCES
    unit = metadata(asm("fz_aggregate_target_encoded"))
    assert len(unit) == 4, sorted(unit)
    new = {re.search("aggregate_target_encoded_ragged" + KEY, k).groups(): v for k, v in unit.items()}
    assert sorted(new) == [("6", "0"), ("6", "1"), ("8", "0"), ("8", "1")], sorted(unit)
    old = {re.search("aggregate_encoded_ragged" + KEY, k).groups(): v for k, v in metadata(asm("fz_aggregate_many_encoded")).items()}
    assert sorted(old) == sorted(new)
    for key, f in new.items():
        assert f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] == 0 and f["private_segment_fixed_size"] == 0, (key, f)
        assert f["vgpr_count"] <= old[key]["vgpr_count"], (key, f["vgpr_count"], old[key]["vgpr_count"])
        assert 0 < f["lds"] <= old[key]["lds"], (key, f["lds"], old[key]["lds"])


def test_entry_is_declared_and_bound_with_fifteen_arguments():
    from fusion_hip._lib import SIGNATURES
    from fusion_hip.context import Context
    with open(os.path.join(ROOT, "include", "fusion_hip.h")) as fh:
        header = fh.read()
    m = re.search(r"FZ_API int fz_aggregate_target_encoded_ragged_async\(([^;]*)\);", header)
    assert m and len(m.group(1).split(",")) == 15, m
    restype, argtypes = SIGNATURES["fz_aggregate_target_encoded_ragged_async"]
    assert len(argtypes) == 15
    assert callable(getattr(Context, "aggregate_target_encoded_ragged_async_dev"))


@pytest.mark.parametrize("secpar", [128, 256])
def test_aggregate_verify_many_encoded_refuses_before_touching_a_device(secpar):
    from fusion_hip import FusionHipError
    from fusion_hip._lib import FZ_E_BADARG
    from fusion_hip.scheme import encoded_size
    bs = _scheme_without_device(secpar)
    rb = TABLE["signature"][secpar][3]
    vk = np.zeros((3, 2, bs.d), dtype=np.int32)
    msgs = ["a", "b", "c"]
    cases = [
        (vk, msgs, bytes(3 * rb), [1, 1]),                         # sizes that do not sum
        (vk, msgs, bytes(3 * rb), [2, 2]),
        (vk, msgs, bytes(3 * rb), [3, 0]),                         # a size of 0
        (vk, msgs, bytes(3 * rb), [4, -1]),
        (vk, msgs, bytes(3 * rb - 1), [1, 2]),                     # a partial record
        (vk, msgs, np.zeros(3 * rb + 1, dtype=np.uint8), [1, 2]),
        (vk, msgs[:2], bytes(3 * rb), [1, 2]),                     # wrong counts: messages, keys, records
        (vk[:2], msgs, bytes(3 * rb), [1, 2]),
        (vk, msgs, bytes(2 * rb), [1, 2]),
        (vk, msgs, bytes(4 * rb), [1, 2]),
        (vk, msgs, np.zeros(3 * rb // 4, dtype=np.int32), [1, 2]),  # not bytes
    ]
    for encoded in (False, True):
        for keys, m, data, sizes in cases:
            with pytest.raises(FusionHipError) as e:
                bs.aggregate_verify_many_encoded(keys, m, data, sizes, encoded=encoded)
            assert e.value.code == FZ_E_BADARG, (sizes, len(m))
    out, codes, verdicts = bs.aggregate_verify_many_encoded(vk[:0], [], b"", [])     # nothing to do: no device either
    assert out.shape == (0, bs.l, bs.d) and out.dtype == np.int32 and codes.shape == (0,) and codes.dtype == np.int32 and verdicts == []
    recs, codes, acodes, verdicts = bs.aggregate_verify_many_encoded(vk[:0], [], b"", [], encoded=True)
    assert recs.shape == (0, encoded_size(bs.params, "aggregate")) and recs.dtype == np.uint8
    assert codes.shape == (0,) and acodes.shape == (0,) and acodes.dtype == np.int32 and verdicts == []


@pytest.mark.parametrize("secpar", [128, 256])
def test_aggregate_verify_encoded_refuses_before_touching_a_device(secpar):
    from fusion_hip import FusionHipError
    from fusion_hip._lib import FZ_E_BADARG
    bs = _scheme_without_device(secpar)
    rb = TABLE["signature"][secpar][3]
    vk = np.zeros((2, 2, bs.d), dtype=np.int32)
    for data in (bytes(2 * rb - 1), bytes(2 * rb + 16), bytearray(1), np.zeros(rb + 1, dtype=np.uint8), memoryview(bytes(rb - 1))):
        with pytest.raises(FusionHipError) as e:
            bs.aggregate_verify_encoded(vk, ["a", "b"], data)
        assert e.value.code == FZ_E_BADARG
    for keys, msgs, n in ((vk, ["a"], 2), (vk[:1], ["a", "b"], 2), (vk, ["a", "b"], 3), (vk, ["a", "b"], 1), (vk, ["a", "b"], 0),
                          (vk[:0], ["a"], 0)):
        with pytest.raises(FusionHipError) as e:
            bs.aggregate_verify_encoded(keys, msgs, bytes(n * rb))
        assert e.value.code == FZ_E_BADARG
    with pytest.raises(FusionHipError) as e:
        bs.aggregate_verify_encoded(vk, ["a", "b"], np.zeros(2 * rb // 4, dtype=np.int32))       # not bytes
    assert e.value.code == FZ_E_BADARG
    out, codes, verdict = bs.aggregate_verify_encoded(vk[:0], [], b"")                          # nothing to do: no device either
    assert out is None and codes.shape == (0,) and codes.dtype == np.int32 and verdict is None


@pytest.mark.parametrize("secpar", [128, 256])
def test_object_face_refuses_before_touching_a_device(secpar, monkeypatch):
    import fusion.fusion as F
    import fusion_hip.scheme as scheme_mod

    def no_scheme(*a, **k):
        raise AssertionError("a BatchScheme was created before the arguments were refused")
    monkeypatch.setattr(scheme_mod, "BatchScheme", no_scheme)
    p = params_of(secpar)
    rb = TABLE["signature"][secpar][3]
    k = [types.SimpleNamespace() for _ in range(3)]
    # the single call
    for ks, ms, blobs in ((k[:2], ["a"], [bytes(rb)] * 2), (k[:1], ["a", "b"], [bytes(rb)] * 2), (k[:2], ["a", "b"], [bytes(rb)]),
                          ([], [], [])):
        with pytest.raises(ValueError):
            F.aggregate_verify_from_bytes(p, ks, ms, blobs)
    with pytest.raises(ValueError, match="record 1"):
        F.aggregate_verify_from_bytes(p, k[:2], ["a", "b"], [bytes(rb), bytes(rb - 1)])
    with pytest.raises(ValueError, match="record 0"):
        F.aggregate_verify_from_bytes(p, k[:2], ["a", "b"], [bytes(rb + 1), bytes(rb)])
    # many committees
    keys, msgs = [k[:1], k[1:]], [["a"], ["b", "c"]]
    good = [[bytes(rb)], [bytes(rb)] * 2]
    for ks, ms, blobs in ((keys, msgs[:1], good), (keys[:1], msgs, good), (keys, msgs, good[:1]),      # numbers of groups
                          (keys, [["a"], ["b"]], good), (keys, msgs, [[bytes(rb)], [bytes(rb)]]),      # counts within group 1
                          ([k[:1], []], [["a"], []], [[bytes(rb)], []])):                              # a group of 0 signers
        with pytest.raises(ValueError):
            F.aggregate_verify_many_from_bytes(p, ks, ms, blobs)
    with pytest.raises(ValueError, match="group 1"):
        F.aggregate_verify_many_from_bytes(p, keys, [["a"], ["b"]], good)
    with pytest.raises(ValueError, match="group 1 record 1"):
        F.aggregate_verify_many_from_bytes(p, keys, msgs, [[bytes(rb)], [bytes(rb), bytes(rb - 1)]])
    with pytest.raises(ValueError, match="group 0 record 0"):
        F.aggregate_verify_many_from_bytes(p, keys, msgs, [[bytes(rb + 1)], [bytes(rb)] * 2])
    assert F.aggregate_verify_many_from_bytes(p, [], [], []) == ([], [])


# ---- the one pass on the stand-in context: how often each step runs, and that every buffer goes ----
SIZES = [1, 4, 2]
MESSAGES = [f"message {i}" for i in range(sum(SIZES))]


@functools.lru_cache(maxsize=None)
def _setup_params():
    import fusion.fusion as F
    return F.fusion_setup(128, 1)


def _one_pass(monkeypatch, status, capacity=None, fail_at=None, single=False):
    """aggregate_verify_many_encoded (or the single call on all seven signers) on the stand-in context, the range check's status
    words read back as `status`: -> (result or the exception, the context, how often hash_ag's serial step ran, per call the
    number of signers it was given)"""
    from fusion_hip import hostpipe
    from fusion_hip.context import DeviceArray
    from fusion_hip.scheme import encoded_size
    p = _setup_params()
    if capacity is not None:
        p = copy.copy(p)
        p.capacity = capacity
    no_finalizers(monkeypatch)
    ctx = stand_in_context(p)
    bs = scheme_on(ctx, p)
    n = sum(SIZES)
    hashed = []
    real = hostpipe.aggregation_coefficients

    def counting(P, L, R, pre, c_hat, threads=None):
        hashed.append(len(L))
        return real(P, L, R, pre, c_hat, threads)
    monkeypatch.setattr(hostpipe, "aggregation_coefficients", counting)
    d2h = type(ctx).d2h

    def d2h_status(self, arr, dptr):                     # the first int32 [n] download is the range check's status
        d2h(self, arr, dptr)
        if arr.shape == (n,) and arr.dtype == np.int32:
            arr[...] = status
        return arr
    monkeypatch.setattr(type(ctx), "d2h", d2h_status)
    rng = np.random.default_rng(7)
    vk = rng.integers(-3, 4, size=(n, 2, p.degree)).astype(np.int32)
    recs = np.zeros((n, encoded_size(p, "signature")), dtype=np.uint8)
    before = dict(ctx.ledger.live)
    ctx.started = len(ctx.names)                         # (behind the scheme's resident public challenge)
    del ctx.calls[:]
    if fail_at is not None:
        ctx.arm(len(ctx.names) + fail_at, "hip")
    try:
        result = bs.aggregate_verify_encoded(vk, MESSAGES, recs) if single else bs.aggregate_verify_many_encoded(vk, MESSAGES, recs, SIZES)
    except Exception as e:                               # noqa: BLE001 (the injected failure; reported to the caller)
        result = e
    assert isinstance(bs._dA, DeviceArray)
    wrong = ctx.ledger.settle(before, None if isinstance(result, Exception) else result)
    assert not wrong, wrong
    return result, ctx, hashed


def test_one_pass_runs_each_step_once_and_hash_ag_once_per_group(monkeypatch):
    status = np.array([0, 0, 6, 0, 0, 0, 0], dtype=np.int32)
    (aggs, codes, verdicts), ctx, hashed = _one_pass(monkeypatch, status)
    assert sorted(hashed) == [1, 2, 3]                    # once per group, over its accepted signers (on the pool: any order)
    names = [c[0] for c in ctx.calls]
    assert names.count("challenge_msgs_dev") == 1
    assert names.count("check_records_async_dev") == 1 and names.count("aggregate_target_encoded_ragged_async_dev") == 1
    assert names.count("verify_partials_batch_async_dev") == 1 and names.count("ntt_forward_dev") == 1
    assert not [x for x in names if x in ("aggregate_encoded_ragged_async_dev", "aggregate_target_partial_ragged_dev", "verify_core_dev")]
    n, d = sum(SIZES), 64
    uploads = [c for c in ctx.calls if c[0] == "h2d"]
    assert len([c for c in uploads if c[2][1] == (n, 2, d)]) == 1, uploads      # vk: once
    assert len(uploads) == 3                                                   # the bytes, the keys, the coefficients
    assert np.array_equal(codes, status) and aggs.shape[0] == 3
    assert verdicts == [(True, "")] * 3                   # (the stand-in's verdict words read back as zero)


def test_a_group_without_an_accepted_signer_is_not_hashed_and_has_no_verdict(monkeypatch):
    status = np.array([0, 6, 6, 6, 6, 0, 6], dtype=np.int32)
    (aggs, codes, verdicts), ctx, hashed = _one_pass(monkeypatch, status)
    assert sorted(hashed) == [1, 1]
    assert verdicts[0] == (True, "") and verdicts[1] is None and verdicts[2] == (True, "")
    (agg, codes, verdict), ctx, hashed = _one_pass(monkeypatch, np.full(7, 6, dtype=np.int32), single=True)
    assert agg is None and verdict is None and hashed == [] and np.array_equal(codes, np.full(7, 6))


def test_more_accepted_signers_than_capacity_is_refused_with_the_aggregate_present(monkeypatch):
    from fusion_hip import VERDICT_REASONS
    (aggs, codes, verdicts), ctx, hashed = _one_pass(monkeypatch, np.zeros(7, dtype=np.int32), capacity=3)
    assert verdicts == [(True, ""), (False, VERDICT_REASONS[1]), (True, "")]
    assert aggs.shape == (3, 195, 64) and sorted(hashed) == [1, 2, 4]
    # three accepted of the four: within capacity again
    (aggs, codes, verdicts), ctx, hashed = _one_pass(monkeypatch, np.array([0, 0, 6, 0, 0, 0, 0], dtype=np.int32), capacity=3)
    assert verdicts == [(True, "")] * 3
    # the single call over all seven
    (agg, codes, verdict), ctx, hashed = _one_pass(monkeypatch, np.zeros(7, dtype=np.int32), capacity=3, single=True)
    assert verdict == (False, VERDICT_REASONS[1]) and agg.shape == (195, 64) and hashed == [7]


def test_every_buffer_is_freed_whatever_raises(monkeypatch):
    """the k-th interaction with the device fails, for every k the call has: nothing stays allocated (_one_pass settles the ledger)"""
    for single in (False, True):
        with pytest.MonkeyPatch.context() as mp:
            _, ctx, _ = _one_pass(mp, np.zeros(7, dtype=np.int32), single=single)
        total = len(ctx.names) - ctx.started
        assert total > 15
        for k in range(1, total + 1):
            with pytest.MonkeyPatch.context() as mp:
                result, ctx, _ = _one_pass(mp, np.zeros(7, dtype=np.int32), fail_at=k, single=single)
            assert isinstance(result, Exception), (single, k)
