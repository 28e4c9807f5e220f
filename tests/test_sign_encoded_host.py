"""Signing straight to the compact byte encoding (fz_sign_encoded_async, BatchScheme.sign_batch_encoded,
fusion.fusion.sign_to_bytes), on the CPU: the spec the device tests of tests/test_gpu_sign_encoded.py are held to (sigma =
cent(L c + R) in Python integers, then the format of tests/test_encoding_host.py: checked against the digests of the golden
signatures), the kernel count and the register and LDS budget of the new translation unit, the export of the entry, and the
refusals that happen before a device is touched."""
import hashlib
import json
import os
import re
import types

import numpy as np
import pytest

from test_aggregate_encoded_host import _scheme_without_device
from test_encoding_host import TABLE, params_of, spec_encode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(os.path.dirname(__file__), "golden")


def spec_sign(q, sk_hat, c_hat):
    """sigma [N][l][d] int64 = cent(L (.) c + R) of sk_hat [N][2][l][d] and c_hat [N][d], any int32, in Python integers"""
    sk = np.asarray(sk_hat, dtype=np.int64).astype(object)
    c = np.asarray(c_hat, dtype=np.int64).astype(object)
    s = (sk[:, 0] * c[:, None, :] + sk[:, 1]) % q
    return np.where(s > (q - 1) // 2, s - q, s).astype(np.int64)


@pytest.mark.parametrize("secpar", [128, 256])
def test_spec_reproduces_the_golden_signature_bytes(secpar):
    from oracle.oracle import PARAMS
    S = np.load(os.path.join(G, f"scheme_{secpar}.npz"))
    sigma = spec_sign(PARAMS[secpar]["q"], S["sk_hat"], S["c_hat"])
    assert np.array_equal(sigma, S["sig"])
    data = spec_encode(secpar, "signature", sigma)
    assert data.shape == (S["sig"].shape[0], TABLE["signature"][secpar][3])
    with open(os.path.join(G, "encoding.json")) as fh:
        assert hashlib.sha3_256(data.tobytes()).hexdigest() == json.load(fh)[str(secpar)]["sig"]


def test_new_unit_has_four_kernels_without_spills_within_the_transforms_lds():
    """fz_sign_encoded: sign_encode for degrees 64 and 256 x both multiply forms, nothing else; no spill, no scratch, no more
    LDS than ntt_inv16 of the same degree"""
    import __graft_entry__ as GE
    from _isa import asm, assert_fits_transforms, metadata
    assert "fz_sign_encoded.hip" in GE.SOURCES
    unit = metadata(asm("fz_sign_encoded"))
    assert len(unit) == 4, sorted(unit)
    assert sorted(re.search(r"\d+sign_encodeILi(\d)ELb(\d)E", k).groups() for k in unit) == \
        [("6", "0"), ("6", "1"), ("8", "0"), ("8", "1")], sorted(unit)
    assert_fits_transforms(unit, r"sign_encodeILi(\d)E", "ntt_inv16")          # (every kernel has a degree: the line above)


def test_the_entry_is_declared_and_has_a_signature():
    from fusion_hip._lib import SIGNATURES
    with open(os.path.join(ROOT, "include", "fusion_hip.h")) as fh:
        header = fh.read()
    assert re.search(r"FZ_API\s+int\s+fz_sign_encoded_async\s*\(", header)
    assert "fz_sign_encoded_async" in SIGNATURES
    # the arguments of fz_encode_records_async with the two inputs in place of the rows, `rows` and `coef`
    assert SIGNATURES["fz_sign_encoded_async"][0] is SIGNATURES["fz_encode_records_async"][0]
    assert len(SIGNATURES["fz_sign_encoded_async"][1]) == 8


@pytest.mark.parametrize("secpar", [128, 256])
def test_sign_batch_encoded_refuses_before_touching_a_device(secpar):
    from fusion_hip import FusionHipError
    from fusion_hip._lib import FZ_E_BADARG
    bs = _scheme_without_device(secpar)
    rb = TABLE["signature"][secpar][3]
    l, d = bs.l, bs.d
    vk = np.zeros((2, 2, d), dtype=np.int32)
    good = np.zeros((2, 2, l, d), dtype=np.int32)
    for sk in (good.reshape(2, 2 * l, d), good.reshape(2, 2, l * d), good.reshape(4, l, d), good[:, :1], good[:, :, :-1], good[:, :, :, :-1],
               np.zeros((2, 2, l + 1, d), dtype=np.int32), np.zeros((2, l, 2, d), dtype=np.int32), good.ravel(), good[0]):
        with pytest.raises(FusionHipError) as e:                   # not [N][2][l][d]
            bs.sign_batch_encoded(sk, vk, ["a", "b"])
        assert e.value.code == FZ_E_BADARG
    three = np.zeros((3, 2, l, d), dtype=np.int32)
    for sk, keys, msgs in ((good, vk, ["a"]), (good, vk[:1], ["a", "b"]), (three, vk, ["a", "b"]), (good[:1], vk, ["a", "b"]),
                           (good, vk, ["a", "b", "c"]), (good[:0], vk, ["a", "b"]), (good, vk[:0], [])):
        with pytest.raises(FusionHipError) as e:                   # unequal counts of key rows, keys and messages
            bs.sign_batch_encoded(sk, keys, msgs)
        assert e.value.code == FZ_E_BADARG
    for device in (False, True):                                   # nothing to do: no device either
        data, codes = bs.sign_batch_encoded(good[:0], vk[:0], [], device=device)
        assert isinstance(data, np.ndarray) and data.shape == (0, rb) and data.dtype == np.uint8
        assert codes.shape == (0,) and codes.dtype == np.int32


@pytest.mark.parametrize("secpar", [128, 256])
def test_the_object_face_reports_a_refused_record_as_to_bytes_does(secpar, monkeypatch):
    import fusion.fusion as F
    from fusion_hip import ENCODING_REASONS
    p = params_of(secpar)
    rb = TABLE["signature"][secpar][3]
    seen = []

    class FakeContext:
        def sign_encoded(self, sk_hat, c_hat, bound):
            seen.append((np.shape(sk_hat), np.shape(c_hat), bound))
            return np.zeros((1, rb), dtype=np.uint8), np.array([FakeContext.code], dtype=np.int32)

    rows = np.zeros((p.num_rows_sk, p.degree), dtype=np.int32)
    monkeypatch.setattr(F, "_ctx", lambda params: FakeContext())
    monkeypatch.setattr(F, "_rows_of", lambda matrix, q: rows)
    monkeypatch.setattr(F, "hash_ch", lambda params, key, message: types.SimpleNamespace(
        c_hat=types.SimpleNamespace(_i32=lambda: np.zeros(p.degree, dtype=np.int32))))
    key = (types.SimpleNamespace(left_sk_hat=None, right_sk_hat=None), types.SimpleNamespace())
    FakeContext.code = 4
    with pytest.raises(ValueError) as e:
        F.sign_to_bytes(p, key, "m")
    assert str(e.value) == ENCODING_REASONS[4]
    FakeContext.code = 0
    assert F.sign_to_bytes(p, key, "m") == bytes(rb)
    assert seen == [((1, 2, p.num_rows_sk, p.degree), (1, p.degree), TABLE["signature"][secpar][1])] * 2
