"""Signing straight from compact secret-key records to signature records (fz_sign_records_async, BatchScheme.sign_batch_records,
keygen_batch_encoded, the "secret" kind, fusion.fusion.sign_from_bytes), on the CPU: the spec the device tests of
tests/test_gpu_sign_records.py are held to -- z = cent(INV(cent(FWD(sL) (.) c)) + sR) in integers on the fields of the key
record, then the format of tests/test_encoding_host.py -- checked against the golden keys and the digests of the golden
signatures; the format table of the fourth kind and the pinned digests of the golden keys' records; the kernel count and the
register and LDS budget of the new translation unit; the export of the entry; the refusals that happen before a device is
touched; who frees the device buffers of the new methods; and the object face's reasons."""
import hashlib
import json
import os
import re
import types

import numpy as np
import pytest

import _encoded_edges as X
from test_aggregate_encoded_host import _scheme_without_device
from test_encoding_host import TABLE, params_of, spec_encode, spec_pack, spec_values

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(os.path.dirname(__file__), "golden")
BETA_SK = 52
# secpar -> (rows, B, w, record bytes) of the "secret" kind: the fourth row of the table of INTEGRATION.md section G
SECRET = {128: (390, BETA_SK, 7, 21840), 256: (166, BETA_SK, 7, 37184)}


def secret_params(secpar):
    p = params_of(secpar)
    p.beta_sk = BETA_SK
    return p


def unpack_fields(data, w):
    """[N][record bytes] uint8 -> [N][fields] int64: the w-bit fields, whatever they hold"""
    data = np.asarray(data, dtype=np.uint8)
    bits = np.unpackbits(data, axis=1, bitorder="little").reshape(data.shape[0], -1, w).astype(np.int64)
    return bits @ (np.int64(1) << np.arange(w, dtype=np.int64))


def spec_values_from_records(spec, key_bytes, key_bound, c_hat, l):
    """(z [N][l][n] int64, non-canonical [N] bool) of N key records of [2][l][n] fields s + key_bound of bit_length(2 key_bound)
    bits under c_hat [N][n], any int32: z = cent(INV(cent(FWD(sL) (.) c)) + sR), FWD / INV the transforms of the context `spec`
    (tests/_encoded_edges.py; a security parameter: the scheme's own).  A record with a field above 2 key_bound has no value: zeros."""
    if not isinstance(spec, tuple):
        spec = (spec, "params")
    q = X.modulus(spec)
    c = np.asarray(c_hat, dtype=np.int64)
    N, n = c.shape
    wk = X.width(key_bound)
    key = np.frombuffer(key_bytes, dtype=np.uint8) if isinstance(key_bytes, (bytes, bytearray)) else np.asarray(key_bytes, dtype=np.uint8)
    u = unpack_fields(key.reshape(N, X.record_bytes(n, 2 * l, wk)), wk)
    bad = (u > 2 * key_bound).any(axis=1)
    s = np.where(~bad[:, None], u - key_bound, 0).reshape(N, 2, l, n)
    prod = X.cent(X.forward(spec, n, s[:, 0]) * c[:, None, :], q)
    return X.cent(X.inverse(spec, n, prod) + s[:, 1], q), bad


def spec_sign_records(spec, key_bytes, key_bound, c_hat, l, bound):
    """what fz_sign_records_async leaves: (bytes [N][l n w / 8], status [N]): the fields z + bound of spec_values_from_records;
    status 6 where a key field is above 2 key_bound, else 4 where some |z| > bound, else 0; a refused record is zero bytes."""
    z, bad = spec_values_from_records(spec, key_bytes, key_bound, c_hat, l)
    status = np.where(bad, 6, np.where(X.maxima(z) > bound, 4, 0)).astype(np.int32)
    w = X.width(bound)
    data = np.zeros((z.shape[0], X.record_bytes(z.shape[2], l, w)), dtype=np.uint8)
    if (status == 0).any():
        data[status == 0] = spec_pack(z[status == 0], bound, w)
    return data, status


def golden_secret_records(secpar):
    """the golden keys as "secret" records, by the spec of the format alone"""
    S = np.load(os.path.join(G, f"scheme_{secpar}.npz"))
    rows, B, w, rb = SECRET[secpar]
    sk = S["sk_hat"]
    z = spec_values(secpar, "signature", sk.reshape(sk.shape[0], rows, sk.shape[-1]))
    assert np.abs(z).max() <= B
    return spec_pack(z, B, w)


@pytest.mark.parametrize("secpar", [128, 256])
def test_spec_on_the_golden_keys_gives_the_golden_signature_bytes(secpar):
    S = np.load(os.path.join(G, f"scheme_{secpar}.npz"))
    rows, B, w, rb = SECRET[secpar]
    recs = golden_secret_records(secpar)
    assert recs.shape == (S["sk_hat"].shape[0], rb)
    with open(os.path.join(G, "secret_encoding.json")) as fh:
        assert hashlib.sha3_256(recs.tobytes()).hexdigest() == json.load(fh)[str(secpar)]["sk"]
    data, st = spec_sign_records(secpar, recs, B, S["c_hat"], rows // 2, TABLE["signature"][secpar][1])
    assert st.tolist() == [0] * recs.shape[0]
    assert np.array_equal(data, spec_encode(secpar, "signature", S["sig"]))
    with open(os.path.join(G, "encoding.json")) as fh:
        assert hashlib.sha3_256(data.tobytes()).hexdigest() == json.load(fh)[str(secpar)]["sig"]
    # a field above 2B refuses its record alone, before anything else
    bad = recs.copy()
    bad[1] = X.set_field(bad[1], 5, 2 * B + 1, w)
    data2, st = spec_sign_records(secpar, bad, B, S["c_hat"], rows // 2, TABLE["signature"][secpar][1])
    assert st.tolist() == [0, 6, 0, 0] and not data2[1].any() and np.array_equal(data2[[0, 2, 3]], data[[0, 2, 3]])


@pytest.mark.parametrize("secpar", [128, 256])
def test_the_format_table_of_the_secret_kind(secpar):
    from fusion_hip.scheme import _encoding, encoded_size
    p = secret_params(secpar)
    rows, B, w, rb = SECRET[secpar]
    assert rows == 2 * p.num_rows_sk
    assert encoded_size(p, "secret") == rb
    assert _encoding(p, "secret")[:5] == (rows, True, B, w, rb)
    assert (2 * B).bit_length() == w and rows * p.degree * w % 8 == 0 and rb % 16 == 0
    assert round(rows * p.degree * 4 / rb, 2) == 4.57
    # the key record is a multiple of 16 bytes for every l and width at both degrees
    assert all((2 * l * d * wk // 8) % 16 == 0 for d in (64, 256) for l in (1, 2, 3, 5) for wk in range(2, 33))


def test_new_unit_has_four_kernels_without_spills_within_the_transforms_lds():
    """fz_sign_records: sign_records for degrees 64 and 256 x both multiply forms, nothing else; no spill, no scratch, no more
    LDS than ntt_inv16 of the same degree"""
    import __graft_entry__ as GE
    from _isa import asm, assert_fits_transforms, metadata
    assert "fz_sign_records.hip" in GE.SOURCES
    unit = metadata(asm("fz_sign_records"))
    assert len(unit) == 4, sorted(unit)
    assert sorted(re.search(r"\d+sign_recordsILi(\d)ELb(\d)E", k).groups() for k in unit) == \
        [("6", "0"), ("6", "1"), ("8", "0"), ("8", "1")], sorted(unit)
    assert_fits_transforms(unit, r"sign_recordsILi(\d)E", "ntt_inv16")          # (every kernel has a degree: the line above)


def test_the_entry_is_declared_has_a_signature_and_is_exported():
    import subprocess
    import __graft_entry__ as GE
    import fusion_hip
    from fusion_hip._lib import SIGNATURES
    with open(os.path.join(ROOT, "include", "fusion_hip.h")) as fh:
        header = fh.read()
    assert re.search(r"FZ_API\s+int\s+fz_sign_records_async\s*\(", header)
    assert "fz_sign_records_async" in SIGNATURES
    # fz_sign_encoded_async's arguments with the key's bytes and their bound in place of sk_hat
    assert SIGNATURES["fz_sign_records_async"][0] is SIGNATURES["fz_sign_encoded_async"][0]
    assert len(SIGNATURES["fz_sign_records_async"][1]) == 9
    GE.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", fusion_hip.LIB_PATH], text=True)
    assert "fz_sign_records_async" in [line.split()[-1] for line in out.splitlines() if " T " in line]


@pytest.mark.parametrize("secpar", [128, 256])
def test_the_new_methods_refuse_before_touching_a_device(secpar):
    from fusion_hip import FusionHipError
    from fusion_hip._lib import FZ_E_BADARG
    bs = _scheme_without_device(secpar)
    bs.params = secret_params(secpar)
    kb, rb = SECRET[secpar][3], TABLE["signature"][secpar][3]
    l, d = bs.l, bs.d
    vk = np.zeros((2, 2, d), dtype=np.int32)

    def refused(call):
        with pytest.raises(FusionHipError) as e:
            call()
        assert e.value.code == FZ_E_BADARG

    for data in (bytes(2 * kb - 1), bytes(2 * kb + 16), bytearray(1), np.zeros(kb + 1, dtype=np.uint8), memoryview(bytes(kb - 1)),
                 np.zeros(2 * kb // 4, dtype=np.int32)):
        refused(lambda: bs.sign_batch_records(data, vk, ["a", "b"]))         # not whole records, or not bytes
        refused(lambda: bs.decode("secret", data))
    for keys, msgs, n in ((vk, ["a"], 2), (vk[:1], ["a", "b"], 2), (vk, ["a", "b"], 3), (vk, ["a", "b"], 1), (vk, ["a", "b", "c"], 2),
                          (vk, ["a", "b"], 0), (vk[:0], [], 2)):
        refused(lambda: bs.sign_batch_records(bytes(n * kb), keys, msgs))     # unequal counts of records, keys and messages
    good = np.zeros((2, 2, l, d), dtype=np.int32)
    for sk in (good.reshape(2, 2, l * d), good.reshape(4, l, d), good[:, :1], good[:, :, :-1], good[:, :, :, :-1],
               np.zeros((2, 2, l + 1, d), dtype=np.int32), np.zeros((2, l, 2, d), dtype=np.int32), good.ravel(), good[0],
               good.reshape(2, 2 * l, d)[:, :-1]):
        refused(lambda: bs.encode("secret", sk))                              # neither [N][2][l][d] nor [N][2l][d]
    for device in (False, True):                                              # nothing to do: no device either
        data, codes = bs.sign_batch_records(b"", vk[:0], [], device=device)
        assert isinstance(data, np.ndarray) and data.shape == (0, rb) and data.dtype == np.uint8
        assert codes.shape == (0,) and codes.dtype == np.int32
    for sk in (good[:0], good.reshape(2, 2 * l, d)[:0]):
        data, codes = bs.encode("secret", sk)
        assert data.shape == (0, kb) and data.dtype == np.uint8 and codes.shape == (0,)
    rows, codes = bs.decode("secret", b"")
    assert rows.shape == (0, 2, l, d) and rows.dtype == np.int32 and codes.shape == (0,)
    # keygen_batch_encoded: seeds that are not a flat sequence of integers, and the empty batch
    for seeds in ([1.5, 2], [1.0], [[1, 2], [3, 4]], [[1], [2]], ["7"], [None], [1, "2"], [True, 2], [np.float64(3)], [(1,)], 5, None,
                  np.array([1.0, 2.0]), np.array([[1, 2]]), np.array(3), np.array(["1"]), np.array([True])):
        for device in (False, True):
            refused(lambda: bs.keygen_batch_encoded(seeds, device=device))
    for seeds in ([], (), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.uint64), np.array([])):
        for device in (False, True):
            recs, keys = bs.keygen_batch_encoded(seeds, device=device)
            assert isinstance(recs, np.ndarray) and recs.shape == (0, kb) and recs.dtype == np.uint8
            assert isinstance(keys, np.ndarray) and keys.shape == (0, 2, d) and keys.dtype == np.int32


# ---- who frees the device buffers ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def params128():
    import fusion.fusion as F
    return F.fusion_setup(128, 1)


def _scope_cases(params):
    from fusion_hip.scheme import encoded_size
    kb = encoded_size(params, "secret")
    d, l = params.degree, params.num_rows_sk
    recs = np.zeros((3, kb), dtype=np.uint8)
    sk = np.zeros((3, 2, l, d), dtype=np.int32)
    vk = np.zeros((3, 2, d), dtype=np.int32)
    msgs = ["first", "second message", "3"]
    c = np.zeros((3, d), dtype=np.int32)
    out = {}
    for device in (False, True):
        out[f"keygen_batch_encoded[device={device}]"] = lambda bs, dv=device: bs.keygen_batch_encoded([5, 6, 7], device=dv)
        out[f"sign_batch_records[device={device}]"] = lambda bs, dv=device: bs.sign_batch_records(recs, vk, msgs, device=dv)
        out[f"decode-secret[device={device}]"] = lambda bs, dv=device: bs.decode("secret", recs, device=dv)
    out["encode-secret"] = lambda bs: bs.encode("secret", sk)
    out["Context.sign_records"] = lambda bs: bs.ctx.sign_records(recs[:, :2 * 2 * d * 7 // 8], BETA_SK, c, 2, 4264)
    return out


def _scope_run(params, name, fail_at=None, kind=None, unsupported=()):
    import _scheme_buffers as SB
    from fusion_hip import FusionHipError
    from fusion_hip.context import Context
    ctx = SB.stand_in_context(params)
    type(ctx).sign_records = Context.sign_records          # the staged host face under test is Context's own code
    bs = SB.scheme_on(ctx, params)
    before = set(ctx.ledger.live)
    ctx.unsupported = unsupported
    del ctx.names[:], ctx.calls[:]
    ctx.arm(fail_at, kind)
    result = raised = None
    try:
        result = _scope_cases(params)[name](bs)
    except (FusionHipError, MemoryError) as e:
        raised = e
    return ctx, ctx.ledger.settle(before, result), raised


@pytest.mark.parametrize("name", ["keygen_batch_encoded[device=False]", "keygen_batch_encoded[device=True]",
                                  "sign_batch_records[device=False]", "sign_batch_records[device=True]",
                                  "decode-secret[device=False]", "decode-secret[device=True]", "encode-secret", "Context.sign_records"])
def test_every_device_buffer_of_the_new_methods_is_freed_whatever_raises(params128, name, monkeypatch):
    import _scheme_buffers as SB
    SB.no_finalizers(monkeypatch)
    fallbacks = ("challenge_msgs_dev", "sample_secret_polys_dev")
    clean, wrong, raised = _scope_run(params128, name)
    assert raised is None and not wrong, (name, raised, wrong)
    assert len(clean.names) >= 2
    walks = [((), clean.names)]
    if any(n in fallbacks for n in clean.names):
        fb, wrong, raised = _scope_run(params128, name, unsupported=fallbacks)
        assert raised is None and not wrong, (name, "fallback", raised, wrong)
        walks.append((fallbacks, fb.names))
    for unsupported, names in walks:
        for k, interaction in enumerate(names, 1):
            for kind in ("error", "memory") if interaction == "malloc" else ("error",):
                _, wrong, raised = _scope_run(params128, name, k, kind, unsupported)
                what = (name, unsupported, k, interaction, kind, raised, wrong)
                assert raised is not None and f"injected at interaction {k} " in str(raised), what
                assert not wrong, what
    if name.startswith("sign_batch_records"):
        assert [n for n in clean.names if n.endswith("_async_dev")] == ["sign_records_async_dev"]      # one launch


# ---- object face -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("secpar", [128, 256])
def test_the_object_face_reports_the_codes_as_value_errors(secpar, monkeypatch):
    import fusion.fusion as F
    import fusion_hip.scheme as SCH
    from fusion_hip import ENCODING_REASONS
    p = secret_params(secpar)
    kb, rb = SECRET[secpar][3], TABLE["signature"][secpar][3]
    seen = []

    class FakeContext:
        def sign_records(self, key_bytes, key_bound, c_hat, l, bound):
            seen.append((len(key_bytes), key_bound, np.shape(c_hat), l, bound))
            return np.zeros((1, rb), dtype=np.uint8), np.array([FakeContext.code], dtype=np.int32)

    monkeypatch.setattr(F, "_ctx", lambda params: FakeContext())
    monkeypatch.setattr(F, "hash_ch", lambda params, key, message: types.SimpleNamespace(
        c_hat=types.SimpleNamespace(_i32=lambda: np.zeros(p.degree, dtype=np.int32))))
    for code in (4, 6):
        FakeContext.code = code
        with pytest.raises(ValueError) as e:
            F.sign_from_bytes(p, bytes(kb), None, "m")
        assert str(e.value) == ENCODING_REASONS[code]
    FakeContext.code = 0
    assert F.sign_from_bytes(p, bytes(kb), None, "m") == bytes(rb)
    assert seen == [(kb, BETA_SK, (1, p.degree), p.num_rows_sk, TABLE["signature"][secpar][1])] * 3
    for wrong in (bytes(kb - 1), bytes(kb + 16), b""):
        with pytest.raises(ValueError) as e:
            F.sign_from_bytes(p, wrong, None, "m")
        assert str(kb) in str(e.value)
        with pytest.raises(ValueError):
            F.from_bytes(p, "secret", wrong)
    assert len(seen) == 3

    # to_bytes / from_bytes of a key: the batch face's codes as reasons
    class FakeScheme:
        def __init__(self, params):
            pass

        def close(self):
            pass

        def encode(self, kind, rows):
            assert kind == "secret" and np.shape(rows) == (1, 2, p.num_rows_sk, p.degree)
            return np.zeros((1, kb), dtype=np.uint8), np.array([FakeScheme.code], dtype=np.int32)

        def decode(self, kind, data):
            assert kind == "secret" and len(data) == kb
            return np.zeros((1, 2, p.num_rows_sk, p.degree), dtype=np.int32), np.array([FakeScheme.code], dtype=np.int32)

    monkeypatch.setattr(SCH, "BatchScheme", FakeScheme)
    monkeypatch.setattr(F, "_rows_of", lambda matrix, q: np.zeros((p.num_rows_sk, p.degree), dtype=np.int32))
    key = F.OneTimeSigningKey(seed=1, left_sk_hat=None, right_sk_hat=None)
    FakeScheme.code = 4
    with pytest.raises(ValueError) as e:
        F.to_bytes(p, key)
    assert str(e.value) == ENCODING_REASONS[4]
    FakeScheme.code = 6
    with pytest.raises(ValueError) as e:
        F.from_bytes(p, "secret", bytes(kb))
    assert str(e.value) == ENCODING_REASONS[6]
    FakeScheme.code = 0
    assert F.to_bytes(p, key) == bytes(kb)
