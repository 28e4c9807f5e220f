"""Key generation straight to compact secret-key records (fz_keygen_records_async, Context.keygen_records[_async_dev],
BatchScheme.keygen_batch_encoded, fusion.fusion.keygen_to_bytes), on the CPU: the spec the device tests of
tests/test_gpu_keygen_records.py are held to -- s = cent(coef mod q), its fields in the format of tests/test_encoding_host.py,
vk = cent(sum_k A_k (.) FWD(s_k)) in integers -- checked against the reference-made golden keys; the kernels of the new
translation unit by name and count with their register, scratch and LDS budget; the declaration, signature and export of the
entry; the refusals that happen before a device is touched; who frees the device buffers; and the object face."""
import hashlib
import json
import os
import re

import numpy as np
import pytest

import _encoded_edges as X
from test_aggregate_encoded_host import _scheme_without_device
from test_encoding_host import spec_pack
from test_sign_records_host import BETA_SK, SECRET, golden_secret_records, secret_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(os.path.dirname(__file__), "golden")


def spec_keygen_records(spec, A, coef, coef_rows, l, key_bound):
    """what fz_keygen_records_async leaves: (bytes [N][2 l n wk / 8], status [N], vk [N][2][n]) for A [l][n] and coef [N][2][n]
    (coef_rows = 1: the one polynomial stands for the l rows) or [N][2][l][n] (coef_rows = l), any int32, on the context `spec`
    (tests/_encoded_edges.py; a security parameter: the scheme's own).  s = cent(coef mod q); status 4 where some |s| >
    key_bound, the record then zero bytes; the fields s + key_bound, left half first; vk[h] = cent(sum_k A_k (.) FWD(s[h][k])),
    whatever the status."""
    if not isinstance(spec, tuple):
        spec = (spec, "params")
    q = X.modulus(spec)
    A = np.asarray(A, dtype=np.int64)
    coef = np.asarray(coef, dtype=np.int64)
    n = coef.shape[-1]
    assert coef_rows in (1, l) and A.shape == (l, n)
    N = coef.shape[0]
    s = X.cent(coef, q)
    s = np.ascontiguousarray(np.broadcast_to(s.reshape(N, 2, 1, n), (N, 2, l, n))) if coef_rows == 1 else s.reshape(N, 2, l, n)
    status = np.where(np.abs(s).reshape(N, -1).max(axis=1) > key_bound, 4, 0).astype(np.int32)
    wk = X.width(key_bound)
    data = np.zeros((N, X.record_bytes(n, 2 * l, wk)), dtype=np.uint8)
    if (status == 0).any():
        data[status == 0] = spec_pack(s[status == 0].reshape(-1, 2 * l, n), key_bound, wk)
    vk = X.cent(X.cent(X.forward(spec, n, s) * A[None, None], q).sum(axis=2), q)
    return data, status, vk


# ---- the spec against the keys the reference made --------------------------------------------------------------------------
@pytest.mark.parametrize("secpar", [128, 256])
def test_spec_on_the_golden_seeds_gives_the_golden_records_and_keys(secpar):
    from fusion_hip import hostpipe
    from oracle.oracle import PARAMS
    P = PARAMS[secpar]
    S = np.load(os.path.join(G, f"scheme_{secpar}.npz"))
    with open(os.path.join(G, "scheme.json")) as fh:
        seeds = json.load(fh)[str(secpar)]["key_seeds"]
    with open(os.path.join(G, "secret_encoding.json")) as fh:
        digest = json.load(fh)[str(secpar)]["sk"]
    rows, B, wk, rb = SECRET[secpar]
    l, d = rows // 2, P["d"]
    polys = hostpipe.sample_secret_polys(np.array(seeds, dtype=np.uint64), P["q"], d, B, d)
    assert polys.shape == (len(seeds), 2, d)
    data, st, vk = spec_keygen_records(secpar, S["A"], polys, 1, l, B)
    assert st.tolist() == [0] * len(seeds) and data.shape == (len(seeds), rb)
    assert hashlib.sha3_256(data.tobytes()).hexdigest() == digest
    assert np.array_equal(data, golden_secret_records(secpar))
    assert np.array_equal(vk, S["vk"])
    # the general form on the reference's own coefficient matrices: the same records and keys
    assert np.array_equal(S["coef"], np.broadcast_to(polys[:, :, None, :], S["coef"].shape))
    data2, st2, vk2 = spec_keygen_records(secpar, S["A"], S["coef"], l, l, B)
    assert st2.tolist() == st.tolist() and np.array_equal(data2, data) and np.array_equal(vk2, vk)
    # one value past the bound refuses its key alone; vk does not depend on the norm
    over = polys.astype(np.int64)
    over[1, 1, 5] = B + 1
    data3, st3, vk3 = spec_keygen_records(secpar, S["A"], over, 1, l, B)
    assert st3.tolist() == [0, 4, 0, 0] and not data3[1].any() and np.array_equal(data3[[0, 2, 3]], data[[0, 2, 3]])
    assert np.array_equal(vk3[[0, 2, 3]], vk[[0, 2, 3]]) and not np.array_equal(vk3[1, 1], vk[1, 1]) and np.array_equal(vk3[1, 0], vk[1, 0])


# ---- the unit ----------------------------------------------------------------------------------------------------------------
def test_new_unit_has_eight_kernels_without_spills_within_keygen_bcast_fuseds_lds():
    """fz_keygen_records: keygen_records_bcast (the seeded form) and keygen_records_rows (the general form) for degrees 64 and
    256 x both multiply forms, nothing else; no spill, no scratch.  Both are built on the radix-4 structure of
    keygen_bcast_fused / keygen_fused (fz_scheme_fused.hip), so their LDS is held to keygen_bcast_fused's of the same degree."""
    import __graft_entry__ as GE
    from _isa import asm, metadata
    assert "fz_keygen_records.hip" in GE.SOURCES
    unit = metadata(asm("fz_keygen_records"))
    assert len(unit) == 8, sorted(unit)
    names = sorted(re.search(r"\d+(keygen_records_(?:bcast|rows))ILi(\d)ELb(\d)E", k).groups() for k in unit)
    assert names == [(f, d, m) for f in ("keygen_records_bcast", "keygen_records_rows") for d in ("6", "8") for m in ("0", "1")], sorted(unit)
    ref = metadata(asm("fz_transforms"), "keygen_bcast_fused")
    assert len(ref) == 4
    for name, f in unit.items():
        assert f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] == 0 and f["private_segment_fixed_size"] == 0, (name, f)
        logd = re.search(r"keygen_records_\w+?ILi(\d)E", name).group(1)
        same = [v["lds"] for k, v in ref.items() if f"keygen_bcast_fusedILi{logd}E" in k]
        assert len(same) == 2 and f["lds"] <= max(same), (name, f["lds"], same)


def test_the_entry_is_declared_has_a_signature_and_is_exported():
    import subprocess
    import __graft_entry__ as GE
    import fusion_hip
    from fusion_hip._lib import SIGNATURES
    with open(os.path.join(ROOT, "include", "fusion_hip.h")) as fh:
        header = fh.read()
    assert re.search(r"FZ_API\s+int\s+fz_keygen_records_async\s*\(", header)
    assert header.index("fz_sign_records_async(") < header.index("fz_keygen_records_async(") < header.index("fz_check_records_async(")
    assert "fz_keygen_records_async" in SIGNATURES
    assert SIGNATURES["fz_keygen_records_async"][0] is SIGNATURES["fz_sign_records_async"][0]
    assert len(SIGNATURES["fz_keygen_records_async"][1]) == 10
    GE.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", fusion_hip.LIB_PATH], text=True)
    assert "fz_keygen_records_async" in [line.split()[-1] for line in out.splitlines() if " T " in line]


# ---- refusals before a device is touched -------------------------------------------------------------------------------------
@pytest.mark.parametrize("secpar", [128, 256])
def test_the_new_faces_refuse_before_touching_a_device(secpar):
    from fusion_hip import FusionHipError
    from fusion_hip._lib import FZ_E_BADARG
    from fusion_hip.context import Context
    bs = _scheme_without_device(secpar)
    bs.params = secret_params(secpar)
    kb = SECRET[secpar][3]
    l, d = bs.l, bs.d

    def refused(call):
        with pytest.raises(FusionHipError) as e:
            call()
        assert e.value.code == FZ_E_BADARG

    for seeds in ([1.5, 2], [1.0], [[1, 2], [3, 4]], [[1], [2]], ["7"], [None], [1, "2"], [True, 2], [np.float64(3)], [(1,)], 5, None,
                  np.array([1.0, 2.0]), np.array([[1, 2]]), np.array(3), np.array(["1"]), np.array([True])):
        for device in (False, True):
            refused(lambda: bs.keygen_batch_encoded(seeds, device=device, keep_vk=True))
    for seeds in ([], (), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.uint64), np.array([])):
        for device in (False, True):
            two = bs.keygen_batch_encoded(seeds, device=device)
            three = bs.keygen_batch_encoded(seeds, device=device, keep_vk=True)
            assert len(two) == 2 and len(three) == 3
            for a, b in zip(two, three):                           # the two values of the two-value form ...
                assert type(a) is type(b) is np.ndarray and a.shape == b.shape and a.dtype == b.dtype
            recs, keys, dkeys = three
            assert recs.shape == (0, kb) and recs.dtype == np.uint8
            for k in (keys, dkeys):                                # ... and no device for the third either
                assert isinstance(k, np.ndarray) and k.shape == (0, 2, d) and k.dtype == np.int32

    # Context.keygen_records: a coef that is neither [batch][2][d] nor [batch][2][l][d] for A's l and d
    ctx = Context.__new__(Context)                                 # no library, no device: the shape check comes first
    A = np.zeros((l, d), dtype=np.int32)
    good = np.zeros((2, 2, l, d), dtype=np.int32)
    for coef in (good.reshape(2, 2, l * d), good.reshape(4, l, d), good[:, :1], good[:, :, :-1], good[:, :, :, :-1], good[:, :, 0, :-1],
                 np.zeros((2, 2, l + 1, d), dtype=np.int32), np.zeros((2, l, 2, d), dtype=np.int32), good.ravel(), good[0],
                 good[0, 0], np.zeros((2, 3, d), dtype=np.int32), np.zeros((2, d), dtype=np.int32), np.zeros((2, 2, 2, l, d), dtype=np.int32)):
        refused(lambda: Context.keygen_records(ctx, A, coef, BETA_SK))
    refused(lambda: Context.keygen_records(ctx, A[0], good[:, :, 0], BETA_SK))


# ---- who frees the device buffers ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def params128():
    import fusion.fusion as F
    return F.fusion_setup(128, 1)


N_KEYS = 3


def _scope_cases(params):
    d, l = params.degree, 2
    A = np.zeros((l, d), dtype=np.int32)
    out = {}
    for device in (False, True):
        for keep in (False, True):
            out[f"keygen_batch_encoded[device={device},keep_vk={keep}]"] = \
                lambda bs, dv=device, k=keep: bs.keygen_batch_encoded([5, 6, 7], device=dv, keep_vk=k)
        out[f"keygen_batch_encoded(negative seed)[device={device},keep_vk=True]"] = \
            lambda bs, dv=device: bs.keygen_batch_encoded([-5, 6, 7], device=dv, keep_vk=True)
    out["Context.keygen_records[one polynomial]"] = lambda bs: bs.ctx.keygen_records(A, np.zeros((N_KEYS, 2, d), dtype=np.int32), BETA_SK)
    out["Context.keygen_records[l polynomials]"] = lambda bs: bs.ctx.keygen_records(A, np.zeros((N_KEYS, 2, l, d), dtype=np.int32), BETA_SK)
    return out


def _scope_run(params, name, fail_at=None, kind=None, unsupported=()):
    import _scheme_buffers as SB
    from fusion_hip import FusionHipError
    from fusion_hip.context import Context
    ctx = SB.stand_in_context(params)
    type(ctx).keygen_records = Context.keygen_records      # the staged host face under test is Context's own code
    bs = SB.scheme_on(ctx, params)
    before = set(ctx.ledger.live)
    ctx.unsupported = unsupported
    del ctx.names[:], ctx.calls[:], ctx.ledger.sizes[:]
    ctx.arm(fail_at, kind)
    result = raised = None
    try:
        result = _scope_cases(params)[name](bs)
    except (FusionHipError, MemoryError) as e:
        raised = e
    n_returned = len(result) if isinstance(result, tuple) else 0
    return ctx, ctx.ledger.settle(before, result), raised, n_returned


@pytest.mark.parametrize("name", ["keygen_batch_encoded[device=False,keep_vk=False]", "keygen_batch_encoded[device=True,keep_vk=False]",
                                  "keygen_batch_encoded[device=False,keep_vk=True]", "keygen_batch_encoded[device=True,keep_vk=True]",
                                  "keygen_batch_encoded(negative seed)[device=False,keep_vk=True]",
                                  "keygen_batch_encoded(negative seed)[device=True,keep_vk=True]",
                                  "Context.keygen_records[one polynomial]", "Context.keygen_records[l polynomials]"])
def test_every_device_buffer_of_the_new_methods_is_freed_whatever_raises(params128, name, monkeypatch):
    import _scheme_buffers as SB
    SB.no_finalizers(monkeypatch)
    fallbacks = ("sample_secret_polys_dev",)
    clean, wrong, raised, n_returned = _scope_run(params128, name)
    assert raised is None and not wrong, (name, raised, wrong)
    assert n_returned == (3 if "keep_vk=True" in name or name.startswith("Context.") else 2)
    walks = [((), clean)]
    if any(n in fallbacks for n in clean.names):
        fb, wrong, raised, _ = _scope_run(params128, name, unsupported=fallbacks)
        assert raised is None and not wrong, (name, "fallback", raised, wrong)
        walks.append((fallbacks, fb))
    d, l = params128.degree, (params128.num_rows_sk if name.startswith("keygen_batch") else 2)
    for unsupported, run in walks:
        # one launch, and -- where the polynomials stand for all l rows -- no allocation the size of the int32 key
        assert [n for n in run.names if n.endswith("_async_dev")] == ["keygen_records_async_dev"], run.names
        assert not [n for n in run.names if n.startswith(("keygen_core", "encode_records"))], run.names
        if "l polynomials" not in name:
            assert run.ledger.sizes and max(run.ledger.sizes) < N_KEYS * 2 * l * d * 4, run.ledger.sizes
        for k, interaction in enumerate(run.names, 1):
            for kind in ("error", "memory") if interaction == "malloc" else ("error",):
                _, wrong, raised, _ = _scope_run(params128, name, k, kind, unsupported)
                what = (name, unsupported, k, interaction, kind, raised, wrong)
                assert raised is not None and f"injected at interaction {k} " in str(raised), what
                assert not wrong, what


# ---- object face -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("secpar", [128, 256])
def test_the_object_face_reports_code_4_as_a_value_error_and_chooses_the_form(secpar, monkeypatch):
    import fusion.fusion as F
    from fusion_hip import ENCODING_REASONS
    from oracle.oracle import PARAMS
    p = secret_params(secpar)
    P = PARAMS[secpar]
    d, l = p.degree, p.num_rows_sk
    kb = SECRET[secpar][3]
    p.root, p.inv_root, p.root_order, p.omega_sk, p.num_cols_sk, p.public_challenge = P["root"], P["inv_root"], 2 * d, d, 1, None
    seen = []

    class FakeContext:
        def keygen_records(self, A, coef, key_bound):
            seen.append((np.shape(A), np.shape(coef), key_bound))
            return np.full((1, kb), 7, dtype=np.uint8), np.arange(2 * d, dtype=np.int32).reshape(1, 2, d), np.array([FakeContext.code], dtype=np.int32)

    monkeypatch.setattr(F, "_ctx", lambda params: FakeContext())
    monkeypatch.setattr(F, "_rows_of", lambda matrix, q: np.zeros((l, d), dtype=np.int32))
    monkeypatch.setattr(F, "_sample_half", lambda params, s: np.full(d, s % 3, dtype=np.int32))
    monkeypatch.setattr(F, "_column", lambda params, arr: np.array(arr))
    FakeContext.code = 4
    with pytest.raises(ValueError) as e:
        F.keygen_to_bytes(p, 11)
    assert str(e.value) == ENCODING_REASONS[4]
    FakeContext.code = 0
    data, vkey = F.keygen_to_bytes(p, 11)
    assert isinstance(data, bytes) and data == bytes([7]) * kb
    assert isinstance(vkey, F.OneTimeVerificationKey)
    assert np.array_equal(vkey.left_vk_hat, np.arange(d).reshape(1, d)) and np.array_equal(vkey.right_vk_hat, np.arange(d, 2 * d).reshape(1, d))
    assert seen == [((l, d), (1, 2, d), BETA_SK)] * 2               # pristine samplers: one polynomial per half
    # somebody patched sample_coefficient_matrix: its matrices are taken as they come, all l rows
    calls = []

    def patched(seed, **kw):
        calls.append((seed, kw["num_rows"], kw["norm_bound"]))
        return None
    monkeypatch.setattr(F, "sample_coefficient_matrix", patched)
    assert not F._pristine("sample_coefficient_matrix", "transform")
    F.keygen_to_bytes(p, 11)
    assert calls == [(11, l, BETA_SK), (12, l, BETA_SK)]
    assert seen[-1] == ((l, d), (1, 2, l, d), BETA_SK)
