"""Verification keys derived straight from compact secret-key records (fz_vk_records_async, Context.vk_records[_async_dev],
BatchScheme.vk_from_records / sign_batch_secret / check_keypairs, fusion.fusion.vk_of_secret_bytes / sign_from_secret_bytes), on
the CPU: the spec the device tests of tests/test_gpu_vk_records.py are held to -- vk = cent(sum_k cent(FWD(s_k) (.) A_k)) per half
in integers on the fields of the key record -- checked against the reference-made golden keys; the kernel count and the register
and LDS budget of the new translation unit; the declaration, signature and export of the entry; the refusals that happen before
a device is touched; who frees the device buffers of the new methods; and the object face's reasons."""
import os
import re
import types

import numpy as np
import pytest

import _encoded_edges as X
from test_aggregate_encoded_host import _scheme_without_device
from test_encoding_host import TABLE
from test_sign_records_host import BETA_SK, SECRET, golden_secret_records, secret_params, unpack_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(os.path.dirname(__file__), "golden")


def spec_vk_records(spec, key_bytes, key_bound, A, l):
    """what fz_vk_records_async leaves: (vk [N][2][n] int64, status [N] int32) of N key records of [2][l][n] fields s + key_bound
    of bit_length(2 key_bound) bits under A [l][n], any int32: vk[b][h] = cent(sum_k cent(FWD(s[b][h][k]) (.) A[k])), FWD the
    forward transform of the context `spec` (tests/_encoded_edges.py; a security parameter: the scheme's own).  Status 6 where a
    field of the record, in either half, is above 2 key_bound, and that key's vk is zero."""
    if not isinstance(spec, tuple):
        spec = (spec, "params")
    A = np.asarray(A, dtype=np.int64)
    assert A.shape[0] == l
    n = A.shape[1]
    wk = X.width(key_bound)
    key = np.frombuffer(key_bytes, dtype=np.uint8) if isinstance(key_bytes, (bytes, bytearray)) else np.asarray(key_bytes, dtype=np.uint8)
    u = unpack_fields(key.reshape(-1, X.record_bytes(n, 2 * l, wk)), wk)
    N = u.shape[0]
    bad = (u > 2 * key_bound).any(axis=1)
    s = np.where(~bad[:, None], u - key_bound, 0).reshape(2 * N, l, n)
    vk = X.verify_sums(spec, n, s, A).reshape(N, 2, n)
    vk[bad] = 0
    return vk, np.where(bad, 6, 0).astype(np.int32)


@pytest.mark.parametrize("secpar", [128, 256])
def test_spec_on_the_golden_records_gives_the_golden_keys(secpar):
    S = np.load(os.path.join(G, f"scheme_{secpar}.npz"))
    rows, B, w, rb = SECRET[secpar]
    l, n = rows // 2, S["A"].shape[1]
    recs = golden_secret_records(secpar)
    vk, st = spec_vk_records(secpar, recs, B, S["A"], l)
    assert st.tolist() == [0] * recs.shape[0]
    assert np.array_equal(vk, S["vk"])
    # a field at 2B + 1 refuses that key alone, whichever half it is in
    for field in (5, l * n + 5, 2 * l * n - 1):
        bad = recs.copy()
        bad[1] = X.set_field(bad[1], field, 2 * B + 1, w)
        vk2, st2 = spec_vk_records(secpar, bad, B, S["A"], l)
        assert st2.tolist() == [0, 6, 0, 0], field
        assert not vk2[1].any() and np.array_equal(vk2[[0, 2, 3]], S["vk"][[0, 2, 3]]), field
    # a field at 2B is a value like any other: the key changes, nothing is refused
    edge = recs.copy()
    edge[2] = X.set_field(edge[2], l * n + 7, 2 * B, w)
    vk3, st3 = spec_vk_records(secpar, edge, B, S["A"], l)
    assert st3.tolist() == [0] * 4 and np.array_equal(vk3[:, 0], S["vk"][:, 0]) and np.array_equal(vk3[[0, 1, 3]], S["vk"][[0, 1, 3]])
    assert not np.array_equal(vk3[2, 1], S["vk"][2, 1])


def test_new_unit_has_four_kernels_without_spills_within_the_transforms_lds():
    """fz_vk_records: vk_records for degrees 64 and 256 x both multiply forms, nothing else; no spill, no scratch, no more LDS
    than ntt_fwd16 of the same degree"""
    import __graft_entry__ as GE
    from _isa import asm, assert_fits_transforms, metadata
    assert "fz_vk_records.hip" in GE.SOURCES and "fz_key_records_capi.hip" in GE.SOURCES
    unit = metadata(asm("fz_vk_records"))
    assert len(unit) == 4, sorted(unit)
    assert sorted(re.search(r"\d+vk_recordsILi(\d)ELb(\d)E", k).groups() for k in unit) == \
        [("6", "0"), ("6", "1"), ("8", "0"), ("8", "1")], sorted(unit)
    assert_fits_transforms(unit, r"vk_recordsILi(\d)E", "ntt_fwd16")             # (every kernel has a degree: the line above)
    # the host unit of the entry holds no kernel
    assert metadata(asm("fz_key_records_capi")) == {}


def test_the_entry_is_declared_has_a_signature_and_is_exported():
    import subprocess
    import __graft_entry__ as GE
    import fusion_hip
    from fusion_hip._lib import SIGNATURES
    with open(os.path.join(ROOT, "include", "fusion_hip.h")) as fh:
        header = fh.read()
    assert re.search(r"FZ_API\s+int\s+fz_vk_records_async\s*\(", header)
    assert header.index("fz_keygen_records_async(") < header.index("fz_vk_records_async(") < header.index("fz_check_records_async(")
    assert "fz_vk_records_async" in SIGNATURES
    assert SIGNATURES["fz_vk_records_async"][0] is SIGNATURES["fz_keygen_records_async"][0]
    assert len(SIGNATURES["fz_vk_records_async"][1]) == 8
    GE.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", fusion_hip.LIB_PATH], text=True)
    assert "fz_vk_records_async" in [line.split()[-1] for line in out.splitlines() if " T " in line]


@pytest.mark.parametrize("secpar", [128, 256])
def test_the_new_methods_refuse_before_touching_a_device(secpar):
    from fusion_hip import FusionHipError
    from fusion_hip._lib import FZ_E_BADARG
    bs = _scheme_without_device(secpar)
    bs.params = secret_params(secpar)
    kb, rb = SECRET[secpar][3], TABLE["signature"][secpar][3]
    d = bs.d
    vk = np.zeros((2, 2, d), dtype=np.int32)

    def refused(call):
        with pytest.raises(FusionHipError) as e:
            call()
        assert e.value.code == FZ_E_BADARG

    for data in (bytes(2 * kb - 1), bytes(2 * kb + 16), bytearray(1), np.zeros(kb + 1, dtype=np.uint8), memoryview(bytes(kb - 1)),
                 np.zeros(2 * kb // 4, dtype=np.int32)):
        for device in (False, True):
            refused(lambda: bs.vk_from_records(data, device=device))          # not whole records, or not bytes
            refused(lambda: bs.sign_batch_secret(data, ["a", "b"], device=device))
        refused(lambda: bs.check_keypairs(data, vk))
    for msgs, n in ((["a"], 2), (["a", "b"], 3), (["a", "b"], 1), (["a", "b", "c"], 2), (["a", "b"], 0), ([], 2)):
        refused(lambda: bs.sign_batch_secret(bytes(n * kb), msgs))              # unequal counts of records and messages
    for keys, n in ((vk, 1), (vk, 3), (vk[:1], 2), (vk, 0), (vk[:0], 2), (np.zeros((2, 2, d + 1), dtype=np.int32), 2)):
        refused(lambda: bs.check_keypairs(bytes(n * kb), keys))                 # unequal counts of records and keys
    for device in (False, True):                                                # nothing to do: no device either
        keys, codes = bs.vk_from_records(b"", device=device)
        assert isinstance(keys, np.ndarray) and keys.shape == (0, 2, d) and keys.dtype == np.int32
        assert codes.shape == (0,) and codes.dtype == np.int32
        data, codes, keys = bs.sign_batch_secret(b"", [], device=device)
        assert isinstance(data, np.ndarray) and data.shape == (0, rb) and data.dtype == np.uint8
        assert codes.shape == (0,) and codes.dtype == np.int32
        assert isinstance(keys, np.ndarray) and keys.shape == (0, 2, d) and keys.dtype == np.int32
    codes = bs.check_keypairs(b"", vk[:0])
    assert codes.shape == (0,) and codes.dtype == np.int32


def test_check_keypairs_compares_mod_q_and_puts_the_encoding_first(monkeypatch):
    """the host half of check_keypairs on derived keys it is handed: equal mod q is 0 (any representative), a difference in either
    half is 3, a refused record is 6 whatever its key"""
    bs = _scheme_without_device(128)
    bs.params = secret_params(128)
    kb, d, q = SECRET[128][3], bs.d, bs.q
    rng = np.random.default_rng(5)
    derived = rng.integers(-(q // 2), q // 2 + 1, size=(5, 2, d)).astype(np.int32)
    derived[4] = 0
    monkeypatch.setattr(type(bs), "vk_from_records", lambda self, secret: (derived, np.array([0, 0, 0, 0, 6], dtype=np.int32)))
    want = derived.astype(np.int64)
    want[1] = X.other_representative(want[1], q)              # the same class mod q
    want[2, 1, d - 1] += 1                                    # one coefficient of the right half
    want[3, 0, 0] -= 1                                        # one of the left half
    assert bs.check_keypairs(bytes(5 * kb), want.astype(np.int32)).tolist() == [0, 0, 3, 3, 6]


# ---- who frees the device buffers ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def params128():
    import fusion.fusion as F
    return F.fusion_setup(128, 1)


def _scope_cases(params):
    from fusion_hip.scheme import encoded_size
    kb = encoded_size(params, "secret")
    d = params.degree
    recs = np.zeros((3, kb), dtype=np.uint8)
    vk = np.zeros((3, 2, d), dtype=np.int32)
    msgs = ["first", "second message", "3"]
    A = np.zeros((2, d), dtype=np.int32)
    out = {}
    for device in (False, True):
        out[f"vk_from_records[device={device}]"] = lambda bs, dv=device: bs.vk_from_records(recs, device=dv)
        out[f"sign_batch_secret[device={device}]"] = lambda bs, dv=device: bs.sign_batch_secret(recs, msgs, device=dv)
    out["check_keypairs"] = lambda bs: bs.check_keypairs(recs, vk)
    out["Context.vk_records"] = lambda bs: bs.ctx.vk_records(recs[:, :2 * 2 * d * 7 // 8], BETA_SK, A, 2)
    return out


def _scope_run(params, name, fail_at=None, kind=None, unsupported=()):
    import _scheme_buffers as SB
    from fusion_hip import FusionHipError
    from fusion_hip.context import Context
    ctx = SB.stand_in_context(params)
    type(ctx).vk_records = Context.vk_records              # the staged host face under test is Context's own code
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


@pytest.mark.parametrize("name", ["vk_from_records[device=False]", "vk_from_records[device=True]", "sign_batch_secret[device=False]",
                                  "sign_batch_secret[device=True]", "check_keypairs", "Context.vk_records"])
def test_every_device_buffer_of_the_new_methods_is_freed_whatever_raises(params128, name, monkeypatch):
    import _scheme_buffers as SB
    SB.no_finalizers(monkeypatch)
    fallbacks = ("challenge_msgs_dev",)
    clean, wrong, raised = _scope_run(params128, name)
    assert raised is None and not wrong, (name, raised, wrong)
    assert len(clean.names) >= 2
    walks = [((), clean.names)]
    if any(n in fallbacks for n in clean.names):
        fb, wrong, raised = _scope_run(params128, name, unsupported=fallbacks)
        assert raised is None and not wrong, (name, "fallback", raised, wrong)
        assert "ntt_forward" in fb.names                    # the host pipeline made the challenges
        walks.append((fallbacks, fb.names))
    assert (len(walks) == 2) == name.startswith("sign_batch_secret")
    for unsupported, names in walks:
        for k, interaction in enumerate(names, 1):
            for kind in ("error", "memory") if interaction == "malloc" else ("error",):
                _, wrong, raised = _scope_run(params128, name, k, kind, unsupported)
                what = (name, unsupported, k, interaction, kind, raised, wrong)
                assert raised is not None and f"injected at interaction {k} " in str(raised), what
                assert not wrong, what
    launches = [n for n in clean.names if n.endswith("_async_dev")]
    if name.startswith("sign_batch_secret"):
        # the key pass, the challenge pass on the resident keys, one signing launch; the only upload is the records'
        assert launches == ["vk_records_async_dev", "sign_records_async_dev"]
        assert clean.names.index("vk_records_async_dev") < clean.names.index("challenge_msgs_dev") < clean.names.index("sign_records_async_dev")
        uploads = [c for c in clean.calls if c[0] == "h2d"]
        assert len(uploads) == 1 and uploads[0][2][:2] == ("uint8", (3, SECRET[128][3])), uploads
    else:
        assert launches == ["vk_records_async_dev"]


# ---- object face -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("secpar", [128, 256])
def test_the_object_face_reports_the_codes_as_value_errors(secpar, monkeypatch):
    import fusion.fusion as F
    from fusion_hip import ENCODING_REASONS
    p = F.fusion_setup(secpar, 1)                             # (the keys it wraps belong to a real ring)
    kb, rb = SECRET[secpar][3], TABLE["signature"][secpar][3]
    l, d = p.num_rows_sk, p.degree
    assert int(p.beta_sk) == BETA_SK
    seen, hashed = [], []
    key_rows = np.arange(2 * d, dtype=np.int32).reshape(1, 2, d)

    class FakeContext:
        code = sign_code = 0

        def vk_records(self, key_bytes, key_bound, A, l_):
            seen.append(("vk", len(key_bytes), key_bound, np.shape(A), l_))
            return key_rows.copy(), np.array([FakeContext.code], dtype=np.int32)

        def sign_records(self, key_bytes, key_bound, c_hat, l_, bound):
            seen.append(("sign", len(key_bytes), key_bound, np.shape(c_hat), l_, bound))
            return np.zeros((1, rb), dtype=np.uint8), np.array([FakeContext.sign_code], dtype=np.int32)

    def fake_hash_ch(params, key, message):
        hashed.append((key, message))
        return types.SimpleNamespace(c_hat=types.SimpleNamespace(_i32=lambda: np.zeros(d, dtype=np.int32)))

    monkeypatch.setattr(F, "_ctx", lambda params: FakeContext())
    monkeypatch.setattr(F, "_rows_of", lambda matrix, q: np.zeros((l, d), dtype=np.int32))
    monkeypatch.setattr(F, "hash_ch", fake_hash_ch)
    FakeContext.code = 6
    for call in (lambda: F.vk_of_secret_bytes(p, bytes(kb)), lambda: F.sign_from_secret_bytes(p, bytes(kb), "m")):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == ENCODING_REASONS[6]
    assert not hashed and seen == [("vk", kb, BETA_SK, (l, d), l)] * 2      # a refused key is not signed with
    FakeContext.code = 0
    vk = F.vk_of_secret_bytes(p, bytes(kb))
    assert isinstance(vk, F.OneTimeVerificationKey)
    assert np.array_equal(F._backend.stack_polys([vk.left_vk_hat.matrix[0][0], vk.right_vk_hat.matrix[0][0]], p.modulus), key_rows[0])
    del seen[:]
    data, vk2 = F.sign_from_secret_bytes(p, bytes(kb), "m")
    assert data == bytes(rb) and isinstance(vk2, F.OneTimeVerificationKey)
    assert seen == [("vk", kb, BETA_SK, (l, d), l), ("sign", kb, BETA_SK, (1, d), l, TABLE["signature"][secpar][1])]
    assert len(hashed) == 1 and hashed[0][0] is vk2 and hashed[0][1] == "m"  # through hash_ch, whoever stands behind that name
    FakeContext.sign_code = 4
    with pytest.raises(ValueError) as e:
        F.sign_from_secret_bytes(p, bytes(kb), "m")
    assert str(e.value) == ENCODING_REASONS[4]
    FakeContext.sign_code = 0
    del seen[:]
    for wrong in (bytes(kb - 1), bytes(kb + 16), b""):
        for call in (lambda: F.vk_of_secret_bytes(p, wrong), lambda: F.sign_from_secret_bytes(p, wrong, "m")):
            with pytest.raises(ValueError) as e:
                call()
            assert str(kb) in str(e.value)
    assert not seen
