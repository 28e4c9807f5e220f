"""Many committees aggregated straight from their compact bytes in one launch (fz_aggregate_encoded_ragged_async,
BatchScheme.aggregate_many_encoded / verify_many_encoded, fusion.fusion.aggregate_many_from_bytes / verify_many_from_bytes), on
the CPU: the census and the register and LDS budget of the new translation unit, the binding of the C entry, and the refusals that
happen before a device is touched.  The device tests are tests/test_gpu_aggregate_many_encoded.py."""
import os
import re
import types

import numpy as np
import pytest

from test_aggregate_encoded_host import _scheme_without_device
from test_encoding_host import TABLE, params_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_unit_holds_the_four_instantiations_within_the_transforms_budget():
    """fz_aggregate_many_encoded: aggregate_encoded_ragged for degrees 64 and 256 x both multiply forms and nothing else; no spill,
    no scratch, no more LDS than ntt_fwd16 of the same degree"""
    import __graft_entry__ as GE
    from _isa import asm, metadata
    assert "fz_aggregate_many_encoded.hip" in GE.SOURCES
    unit = metadata(asm("fz_aggregate_many_encoded"))
    assert len(unit) == 4, sorted(unit)
    assert sorted(re.search(r"aggregate_encoded_raggedILi(\d)ELb(\d)E", k).groups() for k in unit) == \
        [("6", "0"), ("6", "1"), ("8", "0"), ("8", "1")], sorted(unit)
    lds = {k: v["lds"] for k, v in metadata(asm("fz_transforms"), "ntt_fwd16").items()}
    for name, f in unit.items():
        assert f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] == 0 and f["private_segment_fixed_size"] == 0, (name, f)
        logd = re.search(r"aggregate_encoded_raggedILi(\d)E", name).group(1)
        same = [v for k, v in lds.items() if f"16ILi{logd}E" in k]
        assert same and 0 < f["lds"] <= max(same), (name, f["lds"], same)


def test_entry_is_declared_and_bound_with_eleven_arguments():
    from fusion_hip._lib import SIGNATURES
    from fusion_hip.context import Context
    with open(os.path.join(ROOT, "include", "fusion_hip.h")) as fh:
        header = fh.read()
    m = re.search(r"FZ_API int fz_aggregate_encoded_ragged_async\(([^;]*)\);", header)
    assert m and len(m.group(1).split(",")) == 11, m
    restype, argtypes = SIGNATURES["fz_aggregate_encoded_ragged_async"]
    assert len(argtypes) == 11
    assert callable(getattr(Context, "aggregate_encoded_ragged_async_dev"))


@pytest.mark.parametrize("secpar", [128, 256])
def test_aggregate_many_encoded_refuses_before_touching_a_device(secpar):
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
    for screened in (False, True):
        for encoded in (False, True):
            for keys, m, data, sizes in cases:
                with pytest.raises(FusionHipError) as e:
                    bs.aggregate_many_encoded(keys, m, data, sizes, screened=screened, encoded=encoded)
                assert e.value.code == FZ_E_BADARG, (sizes, len(m))
    out, codes = bs.aggregate_many_encoded(vk[:0], [], b"", [])     # nothing to do: no device either
    assert out.shape == (0, bs.l, bs.d) and out.dtype == np.int32 and codes.shape == (0,) and codes.dtype == np.int32
    recs, codes, acodes = bs.aggregate_many_encoded(vk[:0], [], b"", [], encoded=True)
    assert recs.shape == (0, encoded_size(bs.params, "aggregate")) and recs.dtype == np.uint8
    assert codes.shape == (0,) and acodes.shape == (0,) and acodes.dtype == np.int32


@pytest.mark.parametrize("secpar", [128, 256])
def test_verify_many_encoded_refuses_before_touching_a_device(secpar):
    from fusion_hip import FusionHipError
    from fusion_hip._lib import FZ_E_BADARG
    bs = _scheme_without_device(secpar)
    rb = TABLE["aggregate"][secpar][3]
    vk = np.zeros((3, 2, bs.d), dtype=np.int32)
    msgs = ["a", "b", "c"]
    cases = [
        (vk, msgs, bytes(2 * rb), [1, 1]),                         # sizes that do not sum
        (vk, msgs, bytes(2 * rb), [2, 2]),
        (vk, msgs, bytes(2 * rb), [3, 0]),                         # a size of 0
        (vk, msgs, bytes(2 * rb - 1), [1, 2]),                     # a partial record
        (vk, msgs[:2], bytes(2 * rb), [1, 2]),                     # wrong counts: messages, keys, records
        (vk[:2], msgs, bytes(2 * rb), [1, 2]),
        (vk, msgs, bytes(rb), [1, 2]),
        (vk, msgs, bytes(3 * rb), [1, 2]),
        (vk, msgs, np.zeros(2 * rb // 4, dtype=np.int32), [1, 2]),  # not bytes
    ]
    for keys, m, data, sizes in cases:
        with pytest.raises(FusionHipError) as e:
            bs.verify_many_encoded(keys, m, data, sizes)
        assert e.value.code == FZ_E_BADARG, (sizes, len(m))
    assert bs.verify_many_encoded(vk[:0], [], b"", []) == []


@pytest.mark.parametrize("secpar", [128, 256])
def test_object_face_refuses_before_touching_a_device(secpar, monkeypatch):
    import fusion.fusion as F
    import fusion_hip.scheme as scheme_mod

    def no_scheme(*a, **k):
        raise AssertionError("a BatchScheme was created before the arguments were refused")
    monkeypatch.setattr(scheme_mod, "BatchScheme", no_scheme)
    p = params_of(secpar)
    rb, ab = TABLE["signature"][secpar][3], TABLE["aggregate"][secpar][3]
    k = [types.SimpleNamespace() for _ in range(3)]
    keys, msgs = [k[:1], k[1:]], [["a"], ["b", "c"]]
    good = [[bytes(rb)], [bytes(rb)] * 2]
    for ks, ms, blobs in ((keys, msgs[:1], good), (keys[:1], msgs, good), (keys, msgs, good[:1]),      # numbers of groups
                          (keys, [["a"], ["b"]], good), (keys, msgs, [[bytes(rb)], [bytes(rb)]]),      # counts within group 1
                          ([k[:1], []], [["a"], []], [[bytes(rb)], []])):                              # a group of 0 signers
        with pytest.raises(ValueError):
            F.aggregate_many_from_bytes(p, ks, ms, blobs)
    with pytest.raises(ValueError, match="group 1"):
        F.aggregate_many_from_bytes(p, keys, [["a"], ["b"]], good)
    with pytest.raises(ValueError, match="group 1 record 1"):
        F.aggregate_many_from_bytes(p, keys, msgs, [[bytes(rb)], [bytes(rb), bytes(rb - 1)]])
    with pytest.raises(ValueError, match="group 0 record 0"):
        F.aggregate_many_from_bytes(p, keys, msgs, [[bytes(rb + 1)], [bytes(rb)] * 2])
    assert F.aggregate_many_from_bytes(p, [], [], []) == []
    for ks, ms, blobs in ((keys, msgs[:1], [bytes(ab)] * 2), (keys, msgs, [bytes(ab)]), (keys, msgs, [bytes(ab)] * 3),
                          (keys, [["a"], ["b"]], [bytes(ab)] * 2), ([k[:1], []], [["a"], []], [bytes(ab)] * 2)):
        with pytest.raises(ValueError):
            F.verify_many_from_bytes(p, ks, ms, blobs)
    with pytest.raises(ValueError, match="group 1"):
        F.verify_many_from_bytes(p, keys, msgs, [bytes(ab), bytes(ab - 1)])
    assert F.verify_many_from_bytes(p, [], [], []) == []
