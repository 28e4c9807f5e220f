"""Per-signature screening, the parts that need no GPU: the single-signature bound and the bookkeeping of screened aggregation
(hash_ag over the valid subset, coefficients scattered back with zero rows for the rejected signers) on the host C pipeline."""
import types

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    import fusion_hip
    return fusion_hip.load_library()


def _params(secpar):
    import fusion.fusion as F
    return types.SimpleNamespace(secpar=secpar, **F.PREFIX_PARAMETERS[secpar])


def test_signature_bound_is_the_drop_in_constant():
    import fusion.fusion as F
    from fusion_hip import FusionHipError
    from fusion_hip._lib import FZ_E_BADARG
    from fusion_hip.scheme import signature_bound
    assert signature_bound(_params(128)) == F.VF_BD_INTERMEDIATE_128 == 4264
    assert signature_bound(_params(256)) == F.VF_BD_INTERMEDIATE_256 == 3172
    for other in (192, None):
        with pytest.raises(FusionHipError) as e:
            signature_bound(types.SimpleNamespace(secpar=other))
        assert e.value.code == FZ_E_BADARG
    with pytest.raises(FusionHipError):
        signature_bound(object())


def test_signature_reasons_sit_beside_the_verdict_reasons():
    import fusion_hip
    assert sorted(fusion_hip.SIGNATURE_REASONS) == [0, 3, 4, 5]
    assert fusion_hip.SIGNATURE_REASONS[0] == "" and fusion_hip.SIGNATURE_REASONS[3] == "Target doesn't match image of signature."


def _inputs(secpar, n, seed):
    from oracle.oracle import splitmix_centered
    from fusion_hip import hostpipe
    p = _params(secpar)
    P = hostpipe.scheme_params(p)
    d = p.degree
    L = splitmix_centered(seed, n * d).reshape(n, d)
    R = splitmix_centered(seed + 1, n * d).reshape(n, d)
    c_hat = splitmix_centered(seed + 2, n * d).reshape(n, d)
    pre = (splitmix_centered(seed + 3, n * 32) & 0xff).astype(np.uint8).reshape(n, 32)
    return P, L, R, pre, c_hat


def _composition(P, L, R, pre, c_hat, valid):
    """the independent statement: compact the valid signers, sort + hash_ag them, scatter back with numpy"""
    from fusion_hip import hostpipe
    idx = np.flatnonzero(valid)
    out = np.zeros_like(L)
    if idx.size:
        Lv, Rv, pv, cv = L[idx], R[idx], pre[idx], c_hat[idx]
        order = hostpipe.sort_by_vk_string(P, Lv, Rv, 2)
        rows = hostpipe.aggregation_coefficients(P, Lv[order], Rv[order], pv[order], cv[order], 2)
        out[idx[order]] = rows
    return out


@pytest.mark.parametrize("secpar", [128, 256])
def test_screened_coefficients_equal_hash_ag_of_the_valid_subset(lib, secpar):
    from fusion_hip.scheme import screened_alpha_coefficients
    from fusion_hip import hostpipe
    n = 23
    P, L, R, pre, c_hat = _inputs(secpar, n, 40 + secpar)
    rng = np.random.default_rng(secpar)
    valid = rng.random(n) < 0.6
    valid[0], valid[5] = False, True
    order, alpha = screened_alpha_coefficients(P, L, R, pre, c_hat, valid, threads=2)
    assert alpha.shape == (n, P.degree) and alpha.dtype == np.int32
    assert np.array_equal(alpha, _composition(P, L, R, pre, c_hat, valid))
    assert not alpha[~valid].any()                                     # rejected signers: zero rows
    assert (alpha[valid] != 0).any(axis=1).all()                       # every valid signer has a coefficient
    assert sorted(order.tolist()) == np.flatnonzero(valid).tolist()
    # the full sort filtered to the valid signers (what a caller that sorted beforehand passes) gives the same rows
    full = hostpipe.sort_by_vk_string(P, L, R, 2)
    order2, alpha2 = screened_alpha_coefficients(P, L, R, pre, c_hat, valid, threads=2, order=full)
    assert np.array_equal(order2, order) and np.array_equal(alpha2, alpha)


@pytest.mark.parametrize("secpar", [128, 256])
def test_screened_coefficients_with_every_signer_valid(lib, secpar):
    from fusion_hip.scheme import screened_alpha_coefficients
    n = 17
    P, L, R, pre, c_hat = _inputs(secpar, n, 7 + secpar)
    want = _composition(P, L, R, pre, c_hat, np.ones(n, dtype=bool))
    for valid in (None, np.ones(n, dtype=bool)):
        _, alpha = screened_alpha_coefficients(P, L, R, pre, c_hat, valid, threads=2)
        assert (alpha != 0).any(axis=1).all()
        assert np.array_equal(alpha, want)


def test_screened_coefficients_with_no_signer_valid(lib):
    from fusion_hip.scheme import screened_alpha_coefficients
    P, L, R, pre, c_hat = _inputs(256, 5, 3)
    order, alpha = screened_alpha_coefficients(P, L, R, pre, c_hat, np.zeros(5, dtype=bool), threads=2)
    assert order.size == 0 and alpha.shape == (5, 256) and not alpha.any()
