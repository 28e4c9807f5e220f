"""Verification straight from the compact byte encoding (fz_verify_encoded_async, BatchScheme.verify_signatures_encoded /
aggregate_encoded_screened / verify_encoded), on the CPU: the spec the device tests of tests/test_gpu_verify_encoded.py are held
to (unpack the fields, transform, multiply by A, add, compare: checked on the reference-made golden signatures and aggregates),
the kernel count and the register and LDS budget of the new translation unit, and the refusals that happen before a device is
touched."""
import json
import os
import re
import types

import numpy as np
import pytest

from test_aggregate_encoded_host import _scheme_without_device
from test_encoding_host import TABLE, params_of, spec_encode, spec_unpack

G = os.path.join(os.path.dirname(__file__), "golden")


def py_forward(secpar):
    """the oracle's Python-integer forward transform of the rows of an [.., d] array, as a function -> int64 array"""
    from oracle.oracle import PARAMS, py_ntt_forward, py_twiddles
    P = PARAMS[secpar]
    q, d = P["q"], P["d"]
    tw = py_twiddles(P["root"], q, d)

    def fwd(z):
        z = np.asarray(z, dtype=np.int64)
        return np.array([py_ntt_forward([int(v) for v in row], q, tw) for row in z.reshape(-1, d)], dtype=np.int64).reshape(z.shape)
    return fwd


def spec_verdicts(q, data, A, target, B, w, forward):
    """[N][record bytes] uint8 records of A.shape[0] rows, A [l][d] any int32, target [N][d] any integers, `forward` the
    transform of [.., d] rows -> the verdicts [N] and the sums [N][d] in [0, q) (zero for a record without a value):
    6 where a field is above 2B, else 3 where sum_k NTT(z_k) (.) A_k differs from the target mod q, else 0"""
    data = np.asarray(data, dtype=np.uint8)
    l, d = A.shape
    A = np.asarray(A, dtype=np.int64)
    codes, sums = [], np.zeros((data.shape[0], d), dtype=np.int64)
    for i, rec in enumerate(data):
        try:
            z = spec_unpack(rec[None], B, w, (l, d))[0]
        except ValueError:
            codes.append(6)
            continue
        f = forward(z) % q                                         # < 2^32; A % q likewise: the products stay below 2^64
        sums[i] = ((f.astype(object) * (A % q).astype(object)) % q).sum(axis=0) % q
        codes.append(0 if np.array_equal(sums[i], np.asarray(target[i], dtype=np.int64) % q) else 3)
    return np.array(codes, dtype=np.int32), sums


def keyed_targets(q, vk, c_hat):
    """vkL (.) c + vkR mod q per signer, [N][d]"""
    vk, c = np.asarray(vk, dtype=np.int64).astype(object), np.asarray(c_hat, dtype=np.int64).astype(object)
    return ((vk[:, 0] * c + vk[:, 1]) % q).astype(np.int64)


def aggregate_target(q, vk, c_hat, alpha_hat):
    """sum_i alpha_hat_i (vkL_i c_i + vkR_i) mod q, [d]"""
    t = keyed_targets(q, vk, c_hat).astype(object) * np.asarray(alpha_hat, dtype=np.int64).astype(object)
    return (t.sum(axis=0) % q).astype(np.int64)


def set_field(record, j, u, w):
    """a copy of one record's bytes with field j set to u"""
    bits = np.unpackbits(record, bitorder="little").reshape(-1, w)
    bits[j] = (np.int64(u) >> np.arange(w, dtype=np.int64)) & 1
    return np.packbits(bits.ravel(), bitorder="little")


def get_field(record, j, w):
    bits = np.unpackbits(record, bitorder="little").reshape(-1, w)
    return int(bits[j].astype(np.int64) @ (np.int64(1) << np.arange(w, dtype=np.int64)))


@pytest.mark.parametrize("secpar", [128, 256])
def test_spec_accepts_the_golden_signatures_and_aggregates(secpar):
    from oracle.oracle import PARAMS
    q = PARAMS[secpar]["q"]
    S = np.load(os.path.join(G, f"scheme_{secpar}.npz"))
    with open(os.path.join(G, "scheme.json")) as fh:
        agg = json.load(fh)[str(secpar)]["agg"]
    fwd = py_forward(secpar)
    rows, B, w, rb = TABLE["signature"][secpar]
    data = spec_encode(secpar, "signature", S["sig"])
    tgt = keyed_targets(q, S["vk"], S["c_hat"])
    codes, _ = spec_verdicts(q, data, S["A"], tgt, B, w, fwd)
    assert codes.tolist() == [0, 0, 0, 0]
    # one field changed by +-1 (inside the bound): that signer's target is missed; one field 2B + 1: no value at all
    for rec, j, step in ((1, 0, 1), (2, rows * S["A"].shape[1] - 1, -1), (0, 777, 1)):
        d2 = data.copy()
        u = get_field(d2[rec], j, w)
        u2 = u + step if 0 <= u + step <= 2 * B else u - step
        d2[rec] = set_field(d2[rec], j, u2, w)
        codes, _ = spec_verdicts(q, d2[rec:rec + 1], S["A"], tgt[rec:rec + 1], B, w, fwd)
        assert codes.tolist() == [3]
        d2[rec] = set_field(d2[rec], j, 2 * B + 1, w)
        codes, _ = spec_verdicts(q, d2[rec:rec + 1], S["A"], tgt[rec:rec + 1], B, w, fwd)
        assert codes.tolist() == [6]
    rows, B, w, rb = TABLE["aggregate"][secpar]
    for k in (1, 2, 4):
        order = agg[str(k)]["order"]                               # alpha_hat_k is stored in the sorted order of the keys
        t = aggregate_target(q, S["vk"][order], S["c_hat"][order], S[f"alpha_hat_{k}"])
        rec = spec_encode(secpar, "aggregate", S[f"agg_{k}"][None])
        assert rec.shape == (1, rb)
        codes, _ = spec_verdicts(q, rec, S["A"], t[None], B, w, fwd)
        assert codes.tolist() == [0], (secpar, k)
        if k == 4:
            u = get_field(rec[0], 12345, w)
            codes, _ = spec_verdicts(q, set_field(rec[0], 12345, u - 1 if u else 1, w)[None], S["A"], t[None], B, w, fwd)
            assert codes.tolist() == [3]
            codes, _ = spec_verdicts(q, set_field(rec[0], 12345, 2 * B + 1, w)[None], S["A"], t[None], B, w, fwd)
            assert codes.tolist() == [6]


def test_new_unit_has_six_kernels_without_spills_within_the_transforms_lds():
    """fz_verify_encoded: verify_encoded for degrees 64 and 256 x both multiply forms (four) and the finish kernel of the shared
    form for the two degrees (two), nothing else; no spill, no scratch, no more LDS than ntt_fwd16 of the same degree"""
    import __graft_entry__ as GE
    from _isa import asm, metadata
    assert "fz_verify_encoded.hip" in GE.SOURCES
    unit = metadata(asm("fz_verify_encoded"))
    assert len(unit) == 6, sorted(unit)
    main = [k for k in unit if re.search(r"\d+verify_encodedILi", k)]
    assert len(main) == 4 and sorted(re.search(r"verify_encodedILi(\d)ELb(\d)E", k).groups() for k in main) == \
        [("6", "0"), ("6", "1"), ("8", "0"), ("8", "1")], sorted(unit)
    finish = [k for k in unit if "verify_encoded_finish" in k]
    assert sorted(re.search(r"verify_encoded_finishILi(\d)E", k).group(1) for k in finish) == ["6", "8"], sorted(unit)
    assert len(main) + len(finish) == len(unit), sorted(unit)
    lds = {k: v["lds"] for k, v in metadata(asm("fz_transforms"), "ntt_fwd16").items()}
    for name, f in unit.items():
        assert f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] == 0 and f["private_segment_fixed_size"] == 0, (name, f)
        logd = re.search(r"verify_encoded(?:_finish)?ILi(\d)E", name).group(1)
        same = [v for k, v in lds.items() if f"16ILi{logd}E" in k]
        assert same and f["lds"] <= max(same), (name, f["lds"], same)


@pytest.mark.parametrize("secpar", [128, 256])
def test_the_scheme_calls_refuse_before_touching_a_device(secpar):
    from fusion_hip import FusionHipError
    from fusion_hip._lib import FZ_E_BADARG
    bs = _scheme_without_device(secpar)
    bs.params.capacity = 1000
    rb = TABLE["signature"][secpar][3]
    ab = TABLE["aggregate"][secpar][3]
    vk = np.zeros((2, 2, bs.d), dtype=np.int32)
    for call in (bs.verify_signatures_encoded, bs.aggregate_encoded_screened):
        for data in (bytes(2 * rb - 1), bytes(2 * rb + 16), bytearray(1), np.zeros(rb + 1, dtype=np.uint8), memoryview(bytes(rb - 1))):
            with pytest.raises(FusionHipError) as e:               # a ragged length
                call(vk, ["a", "b"], data)
            assert e.value.code == FZ_E_BADARG
        for keys, msgs, n in ((vk, ["a"], 2), (vk[:1], ["a", "b"], 2), (vk, ["a", "b"], 3), (vk, ["a", "b"], 1)):
            with pytest.raises(FusionHipError) as e:               # unequal counts
                call(keys, msgs, bytes(n * rb))
            assert e.value.code == FZ_E_BADARG
        with pytest.raises(FusionHipError) as e:                   # two "aggregate" records where "signature" records are expected
            call(vk, ["a", "b"], bytes(2 * ab))
        assert e.value.code == FZ_E_BADARG
        with pytest.raises(FusionHipError) as e:                   # not bytes
            call(vk, ["a", "b"], np.zeros(2 * rb // 4, dtype=np.int32))
        assert e.value.code == FZ_E_BADARG
    assert bs.verify_signatures_encoded(vk[:0], [], b"").shape == (0,)                   # nothing to do: no device either
    out, codes = bs.aggregate_encoded_screened(vk[:0], [], b"")
    assert out is None and codes.shape == (0,) and codes.dtype == np.int32
    # verify_encoded takes exactly one "aggregate" record
    for data in (bytes(ab - 1), bytes(ab + 1), bytes(rb), bytes(2 * ab), b"", np.zeros(ab // 4, dtype=np.int32)):
        with pytest.raises(FusionHipError) as e:
            bs.verify_encoded(vk, ["a", "b"], data)
        assert e.value.code == FZ_E_BADARG
    # ... and runs verify()'s capacity and length checks before any device work
    bs.params.capacity = 1
    assert bs.verify_encoded(vk, ["a", "b"], bytes(ab)) == (False, "Too many keys.")
    bs.params.capacity = 1000
    assert bs.verify_encoded(vk, ["a"], bytes(ab)) == (False, "Number of keys and messages must be equal.")


@pytest.mark.parametrize("secpar", [128, 256])
def test_the_object_face_refuses_before_touching_a_device(secpar, monkeypatch):
    import fusion.fusion as F
    import fusion_hip.scheme as scheme_mod

    def no_scheme(*a, **k):
        raise AssertionError("a BatchScheme was created before the arguments were refused")
    monkeypatch.setattr(scheme_mod, "BatchScheme", no_scheme)
    p = params_of(secpar)
    rb, ab = TABLE["signature"][secpar][3], TABLE["aggregate"][secpar][3]
    keys = [types.SimpleNamespace(), types.SimpleNamespace()]
    for k, m, blobs in ((keys, ["a"], [bytes(rb)] * 2), (keys[:1], ["a", "b"], [bytes(rb)] * 2), (keys, ["a", "b"], [bytes(rb)])):
        with pytest.raises(ValueError):
            F.verify_signatures_from_bytes(p, k, m, blobs)
    with pytest.raises(ValueError, match="record 1"):
        F.verify_signatures_from_bytes(p, keys, ["a", "b"], [bytes(rb), bytes(rb - 1)])
    with pytest.raises(ValueError, match="record 0"):
        F.verify_signatures_from_bytes(p, keys, ["a", "b"], [bytes(ab), bytes(rb)])
    assert F.verify_signatures_from_bytes(p, [], [], []) == []
    for blob in (bytes(ab - 1), bytes(ab + 16), bytes(rb), b""):
        with pytest.raises(ValueError, match="'aggregate' record"):
            F.verify_from_bytes(p, keys, ["a", "b"], blob)
