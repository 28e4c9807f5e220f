"""Per-signature verification (BatchScheme.verify_signatures, fz_verify_signatures_async, the "target from the key" form of
verify_fused) and screened aggregation (BatchScheme.aggregate_screened), against the golden keys, the C oracle's verify_core
with alpha_hat == 1 and the existing aggregate() / verify() paths."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
_SCHEMES = {}


def scheme(secpar):
    import fusion.fusion as F
    from fusion_hip.scheme import BatchScheme
    if secpar not in _SCHEMES:
        params = F.fusion_setup(secpar, 1000 + secpar)
        _SCHEMES[secpar] = (params, BatchScheme(params, threads=4))
    return _SCHEMES[secpar]


def honest(bs, n, seed0):
    seeds = [seed0 + 7 * i for i in range(n)]
    msgs = [f"screen-{seed0}-{i}" for i in range(n)]
    sk, vk = bs.keygen_batch(seeds)
    return vk, msgs, bs.sign_batch(sk, vk, msgs)


def over_norm(bs, n, seed):
    """keys from secret coefficient rows far above beta_sk (up to +-10^4), signed with the context's cores: |sigma| < 6.1e5"""
    rng = np.random.default_rng(seed)
    coef = rng.integers(-10 ** 4, 10 ** 4 + 1, size=(n, 2, bs.l, bs.d)).astype(np.int32)
    sk, vk = bs.ctx.keygen_core(bs.A, coef)
    msgs = [f"loud-{seed}-{i}" for i in range(n)]
    c_hat, _ = bs.challenges(vk, msgs)
    return vk, msgs, bs.ctx.sign_core(sk, c_hat)


def mixture(bs, n, seed):
    """n signers, each honest, tampered (a coefficient / the message / keys swapped with another signer) or over the norm
    bound -> (vk, msgs, sig)"""
    rng = np.random.default_rng(seed)
    vk, msgs, sig = honest(bs, n, seed)
    vk, sig = vk.copy(), sig.copy()
    loud = over_norm(bs, min(n, 8), seed + 1)
    kind = rng.integers(0, 5, size=n) if n > 1 else np.array([seed % 5])
    for i in range(n):
        if kind[i] == 1:
            sig[i, rng.integers(bs.l), rng.integers(bs.d)] += int(rng.integers(1, 1000))
        elif kind[i] == 2:
            msgs[i] = msgs[i] + "!"
        elif kind[i] == 3 and n > 1:
            j = (i + 1) % n
            vk[[i, j]] = vk[[j, i]]
        elif kind[i] == 4:
            k = i % loud[0].shape[0]
            vk[i], msgs[i], sig[i] = loud[0][k], loud[1][k], loud[2][k]
    return vk, msgs, sig


def oracle_codes(coracle, bs, vk, msgs, sig, beta, omega):
    q, d = bs.q, bs.d
    c_hat, _ = bs.challenges(vk, msgs)
    one = np.ones((1, d), dtype=np.int32)
    return np.array([coracle.verify_core(bs.A, sig[i], vk[i:i + 1, 0], vk[i:i + 1, 1], c_hat[i:i + 1], one, q,
                                         bs.params.inv_root % q, beta, omega) for i in range(len(msgs))], dtype=np.int32)


@pytest.mark.parametrize("secpar", [128, 256])
def test_golden_signatures_pass(secpar):
    import fusion.fusion as F
    from fusion_hip.scheme import BatchScheme
    S = np.load(os.path.join(G, f"scheme_{secpar}.npz"))
    with open(os.path.join(G, "scheme.json")) as fh:
        m = json.load(fh)[str(secpar)]
    bs = BatchScheme(F.fusion_setup(secpar, m["setup_seed"]))
    codes = bs.verify_signatures(S["vk"], m["messages"], S["sig"])
    assert codes.dtype == np.int32 and codes.tolist() == [0] * len(m["messages"])


@pytest.mark.parametrize("secpar", [128, 256])
def test_tampering_flags_exactly_that_signer(secpar):
    _, bs = scheme(secpar)
    vk, msgs, sig = honest(bs, 6, 300 + secpar)
    assert bs.verify_signatures(vk, msgs, sig).tolist() == [0] * 6
    j, i = 4, 1
    want = [0] * 6
    want[j] = 3
    bad = sig.copy()
    bad[j, 7, 3] += 1
    assert bs.verify_signatures(vk, msgs, bad).tolist() == want
    wrong = list(msgs)
    wrong[j] += "?"
    assert bs.verify_signatures(vk, wrong, sig).tolist() == want
    swapped = vk.copy()
    swapped[[i, j]] = swapped[[j, i]]
    both = [0] * 6
    both[i] = both[j] = 3
    assert bs.verify_signatures(swapped, msgs, sig).tolist() == both


@pytest.mark.parametrize("secpar", [128, 256])
def test_over_norm_signers_get_code_4_but_pass_the_aggregate_of_one(secpar):
    _, bs = scheme(secpar)
    vk_h, m_h, sig_h = honest(bs, 3, 500 + secpar)
    vk_l, m_l, sig_l = over_norm(bs, 3, 600 + secpar)
    vk, msgs, sig = np.concatenate([vk_h, vk_l]), m_h + m_l, np.concatenate([sig_h, sig_l])
    assert np.abs(bs.ctx.ntt_inverse(sig_l.reshape(-1, bs.d))).max() < 610000
    assert bs.verify_signatures(vk, msgs, sig).tolist() == [0, 0, 0, 4, 4, 4]
    for j in range(3):          # the looser check: aggregate + verify of one signer still accepts it
        agg = bs.aggregate(vk_l[j:j + 1], m_l[j:j + 1], sig_l[j:j + 1])
        assert bs.verify(vk_l[j:j + 1], m_l[j:j + 1], agg) == (True, "")


@pytest.mark.parametrize("secpar", [128, 256])
@pytest.mark.parametrize("n", [1, 7, 100, 1024])
def test_codes_equal_the_oracle(secpar, n, coracle):
    from fusion_hip import DeviceArray
    from fusion_hip.scheme import signature_bound
    params, bs = scheme(secpar)
    vk, msgs, sig = mixture(bs, n, 10 * n + secpar)
    beta, omega = signature_bound(params), params.omega_vf
    want = oracle_codes(coracle, bs, vk, msgs, sig, beta, omega)
    if n >= 7:
        assert set(want.tolist()) >= {0, 3, 4}
    assert np.array_equal(bs.verify_signatures(vk, msgs, sig), want)
    dK, dS = DeviceArray.from_numpy(bs.ctx, vk), DeviceArray.from_numpy(bs.ctx, sig)
    try:
        assert np.array_equal(bs.verify_signatures(dK, msgs, dS), want)
        # the weight check (omega below a row's weight) and an explicit beta, against the oracle too
        assert np.array_equal(bs.verify_signatures(dK, msgs, dS, omega=bs.d // 2),
                              oracle_codes(coracle, bs, vk, msgs, sig, beta, bs.d // 2))
        assert np.array_equal(bs.verify_signatures(dK, msgs, dS, beta=700000),
                              oracle_codes(coracle, bs, vk, msgs, sig, 700000, omega))
    finally:
        dK.free()
        dS.free()


def test_device_resident_keys_and_signatures_from_the_batch_calls():
    _, bs = scheme(256)
    seeds = list(range(40, 72))
    msgs = [f"dev-{s}" for s in seeds]
    dsk, _, dvk = bs.keygen_batch(seeds, device=True, keep_vk=True)
    dsig = bs.sign_batch(dsk, dvk, msgs, device=True)
    try:
        assert bs.verify_signatures(dvk, msgs, dsig).tolist() == [0] * len(seeds)
        wrong = list(msgs)
        wrong[31] += "."
        assert bs.verify_signatures(dvk, wrong, dsig).tolist() == [0] * 31 + [3]
    finally:
        for b in (dsk, dvk, dsig):
            b.free()


def test_caller_errors_raise():
    from fusion_hip import FusionHipError
    from fusion_hip._lib import FZ_E_BADARG
    _, bs = scheme(128)
    vk, msgs, sig = honest(bs, 3, 77)
    with pytest.raises(FusionHipError) as e:
        bs.verify_signatures(vk, msgs[:2], sig)
    assert e.value.code == FZ_E_BADARG
    assert bs.verify_signatures(vk[:0], [], sig[:0]).shape == (0,)


def test_interleaves_with_verify_on_one_context(coracle):
    """small-N (several workgroups per signer), large-N (one each), small again, with verify() / verify_many() between: the
    shared accumulators are re-armed by every launch of either kind"""
    from fusion_hip.scheme import signature_bound
    params, bs = scheme(256)
    beta = signature_bound(params)
    small = mixture(bs, 5, 91)
    large = mixture(bs, 1024, 92)
    want_s = oracle_codes(coracle, bs, *small, beta, params.omega_vf)
    want_l = oracle_codes(coracle, bs, *large, beta, params.omega_vf)
    vk, msgs, sig = honest(bs, 4, 93)
    agg = bs.aggregate(vk, msgs, sig)
    bad = agg.copy()
    bad[2, 2] += 1
    for _ in range(2):
        assert np.array_equal(bs.verify_signatures(*small), want_s)
        assert bs.verify(vk, msgs, agg) == (True, "")
        assert np.array_equal(bs.verify_signatures(*large), want_l)
        assert [ok for ok, _ in bs.verify_many(np.concatenate([vk, vk]), msgs + msgs, np.stack([agg, bad]), [4, 4])] == [True, False]
        assert np.array_equal(bs.verify_signatures(*small), want_s)
        assert bs.verify(vk, msgs, bad)[0] is False


@pytest.mark.parametrize("secpar", [128, 256])
def test_aggregate_screened_equals_aggregate_of_the_valid_subset(secpar):
    _, bs = scheme(secpar)
    vk, msgs, sig = mixture(bs, 40, 700 + secpar)
    agg, codes = bs.aggregate_screened(vk, msgs, sig)
    ok = codes == 0
    assert 0 < ok.sum() < 40
    assert np.array_equal(codes, bs.verify_signatures(vk, msgs, sig))
    m_ok = [m for m, k in zip(msgs, ok) if k]
    want = bs.aggregate(vk[ok], m_ok, sig[ok])
    assert np.array_equal(agg, want)
    assert bs.verify(vk[ok], m_ok, agg) == (True, "")
    assert bs.verify(vk, msgs, bs.aggregate(vk, msgs, sig))[0] is False     # what screening saves the aggregator from
    # every signer valid: aggregate() of all of them
    vk2, msgs2, sig2 = honest(bs, 12, 800 + secpar)
    agg2, codes2 = bs.aggregate_screened(vk2, msgs2, sig2)
    assert codes2.tolist() == [0] * 12 and np.array_equal(agg2, bs.aggregate(vk2, msgs2, sig2))
    # none valid
    bad = sig2.copy()
    bad[:, 0, 0] += 1
    agg3, codes3 = bs.aggregate_screened(vk2, msgs2, bad)
    assert agg3 is None and codes3.tolist() == [3] * 12


def test_object_face_equals_the_array_path():
    import fusion.fusion as F
    from fusion_hip import SIGNATURE_REASONS
    from fusion_hip.scheme import signature_to_object, vk_to_object
    params, bs = scheme(128)
    vk, msgs, sig = mixture(bs, 9, 5)
    codes = bs.verify_signatures(vk, msgs, sig)
    keys = [vk_to_object(params, v) for v in vk]
    sigs = [signature_to_object(params, s) for s in sig]
    got = F.verify_signatures(params, keys, msgs, sigs)
    assert got == [(int(c) == 0, SIGNATURE_REASONS[int(c)]) for c in codes]
    assert {r for _, r in got} >= {"", "Target doesn't match image of signature."}


def test_launch_is_chunked_over_the_grid_limit():
    """more signers than a grid's y dimension holds (65536 on this device family; the launcher queries it): one case spans
    the boundary, with bad signers on both sides of it.  Secpar 128: 3.3 GB of signatures."""
    from fusion_hip import DeviceArray
    params, bs = scheme(128)
    base = 64
    vk_b, m_b, sig_b = honest(bs, base, 4242)
    vk_l, m_l, sig_l = over_norm(bs, 1, 4343)
    N = 65536 + base
    idx = np.arange(N) % base
    vk = vk_b[idx]
    msgs = [m_b[i] for i in idx]
    dS = DeviceArray(bs.ctx, (N, bs.l, bs.d))
    row = bs.l * bs.d * 4
    try:
        for k in range(N // base):
            bs.ctx.h2d(dS.ptr + k * base * row, sig_b)
        want = np.zeros(N, dtype=np.int32)
        msgs[65535] += "x"                                     # last signer of the first chunk
        want[65535] = 3
        t = sig_b[0].copy()                                    # first signer of the second chunk
        t[100, 9] -= 1
        bs.ctx.h2d(dS.ptr + 65536 * row, t)
        want[65536] = 3
        vk[N - 1], msgs[N - 1] = vk_l[0], m_l[0]               # the last signer, over the norm
        bs.ctx.h2d(dS.ptr + (N - 1) * row, sig_l[0])
        want[N - 1] = 4
        want[1] = 3
        msgs[1] += "y"
        codes = bs.verify_signatures(vk, msgs, dS)
        assert np.array_equal(np.flatnonzero(codes), np.flatnonzero(want))
        assert np.array_equal(codes, want)
    finally:
        dS.free()
