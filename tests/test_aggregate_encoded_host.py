"""Aggregation straight from the compact byte encoding (BatchScheme.aggregate_encoded, fz_aggregate_encoded_async), on the CPU: the
spec the device tests of tests/test_gpu_aggregate_encoded.py are held to (unpack the fields, transform, multiply by alpha_hat,
add: the reference-made golden aggregates), the register and LDS budget of the new translation unit's kernels, and the refusals
that happen before a device is touched."""
import json
import os
import re
import types

import numpy as np
import pytest

from test_encoding_host import TABLE, params_of, spec_encode, spec_unpack

G = os.path.join(os.path.dirname(__file__), "golden")


def spec_aggregate(secpar, data, alpha_hat):
    """[N][record bytes] uint8 signature records, alpha_hat [N][d] -> the aggregate [l][d]: cent(sum_i NTT(z_i) (.) alpha_hat_i)
    with the oracle's Python-integer transform and aggregation"""
    from oracle.oracle import PARAMS, py_aggregate_core, py_ntt_forward, py_twiddles
    P = PARAMS[secpar]
    q, d = P["q"], P["d"]
    rows, B, w, _ = TABLE["signature"][secpar]
    z = spec_unpack(data, B, w, (rows, d))
    tw = py_twiddles(P["root"], q, d)
    sigs = [[py_ntt_forward([int(v) for v in row], q, tw) for row in rec] for rec in z]
    return np.array(py_aggregate_core(sigs, [[int(v) for v in a] for a in alpha_hat], q), dtype=np.int64)


@pytest.mark.parametrize("secpar", [128, 256])
def test_spec_reproduces_the_golden_aggregates(secpar):
    S = np.load(os.path.join(G, f"scheme_{secpar}.npz"))
    with open(os.path.join(G, "scheme.json")) as fh:
        agg = json.load(fh)[str(secpar)]["agg"]
    data = spec_encode(secpar, "signature", S["sig"])
    assert data.shape == (4, TABLE["signature"][secpar][3])
    for k in (1, 2, 4):
        order = agg[str(k)]["order"]                               # alpha_hat_k is stored in the sorted order of the keys
        assert np.array_equal(spec_aggregate(secpar, data[order], S[f"alpha_hat_{k}"]), S[f"agg_{k}"]), (secpar, k)


def test_new_kernels_compile_without_spills_and_within_the_transforms_lds():
    """fz_aggregate_encoded: the range check (one instantiation) and the fused aggregation for degrees 64 and 256 x both multiply
    forms (four); no spill, no scratch, no more LDS than ntt_fwd16 of the same degree"""
    from _isa import asm, metadata
    unit = metadata(asm("fz_aggregate_encoded"))
    assert len(unit) == 5, sorted(unit)
    assert len([k for k in unit if "encoded_check" in k]) == 1, sorted(unit)
    fused = [k for k in unit if "aggregate_encoded" in k]
    assert len(fused) == 4 and sorted(re.search(r"aggregate_encodedILi(\d)ELb(\d)E", k).groups() for k in fused) == \
        [("6", "0"), ("6", "1"), ("8", "0"), ("8", "1")], sorted(unit)
    assert not [k for k in unit if "records_" in k or "aggregate_onepass" in k]
    lds = {k: v["lds"] for k, v in metadata(asm("fz_transforms"), "ntt_fwd16").items()}
    for name, f in unit.items():
        assert f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] == 0 and f["private_segment_fixed_size"] == 0, (name, f)
        logd = re.search(r"aggregate_encodedILi(\d)E", name)
        same = [v for k, v in lds.items() if logd is None or f"16ILi{logd.group(1)}E" in k]
        assert same and f["lds"] <= (max(same) if logd else min(same)), (name, f["lds"], same)


class _NoDevice:
    """a context that fails the test when anything is asked of it"""
    def __getattr__(self, name):
        raise AssertionError(f"the device was touched ({name}) before the arguments were refused")


def _scheme_without_device(secpar):
    from fusion_hip.scheme import BatchScheme
    p = params_of(secpar)
    bs = BatchScheme.__new__(BatchScheme)
    bs.params, bs.d, bs.l, bs.q, bs.ctx = p, p.degree, p.num_rows_sk, p.modulus, _NoDevice()
    bs.threads, bs._pool, bs.device_hash = 1, None, True
    return bs


@pytest.mark.parametrize("secpar", [128, 256])
def test_aggregate_encoded_refuses_before_touching_a_device(secpar):
    from fusion_hip import FusionHipError
    from fusion_hip._lib import FZ_E_BADARG
    bs = _scheme_without_device(secpar)
    rb = TABLE["signature"][secpar][3]
    vk = np.zeros((2, 2, bs.d), dtype=np.int32)
    for data in (bytes(2 * rb - 1), bytes(2 * rb + 16), bytearray(1), np.zeros(rb + 1, dtype=np.uint8), memoryview(bytes(rb - 1))):
        with pytest.raises(FusionHipError) as e:
            bs.aggregate_encoded(vk, ["a", "b"], data)
        assert e.value.code == FZ_E_BADARG
    for keys, msgs, n in ((vk, ["a"], 2), (vk[:1], ["a", "b"], 2), (vk, ["a", "b"], 3), (vk, ["a", "b"], 1)):
        with pytest.raises(FusionHipError) as e:
            bs.aggregate_encoded(keys, msgs, bytes(n * rb))
        assert e.value.code == FZ_E_BADARG
    with pytest.raises(FusionHipError) as e:
        bs.aggregate_encoded(vk, ["a", "b"], np.zeros(2 * rb // 4, dtype=np.int32))       # not bytes
    assert e.value.code == FZ_E_BADARG
    out, codes = bs.aggregate_encoded(vk[:0], [], b"")                                   # nothing to do: no device either
    assert out is None and codes.shape == (0,) and codes.dtype == np.int32


@pytest.mark.parametrize("secpar", [128, 256])
def test_aggregate_from_bytes_refuses_before_touching_a_device(secpar, monkeypatch):
    import fusion.fusion as F
    import fusion_hip.scheme as scheme_mod

    def no_scheme(*a, **k):
        raise AssertionError("a BatchScheme was created before the arguments were refused")
    monkeypatch.setattr(scheme_mod, "BatchScheme", no_scheme)
    p = params_of(secpar)
    rb = TABLE["signature"][secpar][3]
    keys = [types.SimpleNamespace(), types.SimpleNamespace()]
    for k, m, blobs in ((keys, ["a"], [bytes(rb)] * 2), (keys[:1], ["a", "b"], [bytes(rb)] * 2), (keys, ["a", "b"], [bytes(rb)])):
        with pytest.raises(ValueError):
            F.aggregate_from_bytes(p, k, m, blobs)
    with pytest.raises(ValueError, match="record 1"):
        F.aggregate_from_bytes(p, keys, ["a", "b"], [bytes(rb), bytes(rb - 1)])
    with pytest.raises(ValueError, match="record 0"):
        F.aggregate_from_bytes(p, keys, ["a", "b"], [bytes(rb + 1), bytes(rb)])
