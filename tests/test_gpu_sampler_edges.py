"""The device key sampler (csrc/fz_sample.hip) on the fixtures of tests/_sampler_edges.py: pass-through lanes, carries over a
generation boundary, rows that end on a generation's first or last output, the 16-generation limit from both sides, the
smallest and the largest bound -- in the two-kernel form (mt_seed_kernel + mt_draw_kernel, up to 4096 keys per call) and the
one-kernel form (mt_sample_kernel, above).  Expected rows come from CPython's `random` (E.plain_model), not from the C clone;
every call writes into a poisoned buffer with a poisoned guard row in front of the output and one behind it.
tests/test_sampler_edges_host.py shows which fixture notices which fault."""
import numpy as np
import pytest

import _sampler_edges as E
from oracle import oracle as O

pytestmark = pytest.mark.gpu

Q_MAX = 2 ** 32 - 1                  # the sampler's modulus only caps the bound at q // 2 = 2^31 - 1
PAIRS = sorted({(f[0], f[1]) for f in E.all_fixtures()})
ONE_KERNEL_KEYS = 4097               # above the launcher's switch; 8194 polynomials: a last wave with two live lanes


def _ctx():
    import fusion_hip
    P = O.PARAMS[256]
    return fusion_hip.get_context(P["q"], P["d"], P["root"], P["inv_root"])


def _good_keys(degree, bound):
    """the key seeds of the pair's fixtures whose two halves both fit the 9984 outputs, in fixture order"""
    keys = []
    for fx in E.all_fixtures():
        if (fx[0], fx[1]) == (degree, bound) and not E.key_fails(fx) and fx[2] not in keys:
            keys.append(fx[2])
    return keys


def _want(keys, degree, bound):
    """[N][2][degree] int32 from the plain model, each distinct key computed once"""
    distinct = sorted(set(keys))
    table = np.stack([E.expected_key(k, degree, bound) for k in distinct]).astype(np.int32)
    return table[np.searchsorted(distinct, keys)]


class Guarded:
    """a device buffer [1 + 2 N + 1][degree] int32, poisoned before every call: the output and a guard row on either side"""

    def __init__(self, ctx, n, degree):
        import fusion_hip
        self.ctx, self.n, self.degree = ctx, n, degree
        self.poison = np.full((2 * n + 2, degree), E.POISON, dtype=np.int32)
        self.buf = fusion_hip.DeviceBuffer(ctx, self.poison.nbytes)

    def sample(self, keys, bound, modulus=Q_MAX):
        assert len(keys) == self.n
        self.ctx.h2d(self.buf.ptr, self.poison)
        self.ctx.sample_secret_polys_dev(keys, modulus, self.degree, bound, self.degree, self.buf.ptr + 4 * self.degree)

    def guards_intact(self):
        front, back = np.empty(self.degree, dtype=np.int32), np.empty(self.degree, dtype=np.int32)
        self.ctx.d2h(front, self.buf.ptr)
        self.ctx.d2h(back, self.buf.ptr + 4 * self.degree * (2 * self.n + 1))
        return bool((front == E.POISON).all() and (back == E.POISON).all())

    def rows(self):
        return self.buf.to_numpy(np.int32, (2 * self.n + 2, self.degree))[1:-1].reshape(self.n, 2, self.degree)

    def free(self):
        self.buf.free()


def _check(ctx, keys, degree, bound):
    g = Guarded(ctx, len(keys), degree)
    try:
        g.sample(keys, bound)
        assert g.guards_intact(), (degree, bound, keys[:8])
        got, want = g.rows(), _want(keys, degree, bound)
        if not np.array_equal(got, want):
            bad = np.argwhere(got != want)
            i, h, j = (int(x) for x in bad[0])
            raise AssertionError(f"degree {degree} bound {bound}: {len(bad)} coefficients differ, first at key {i} (seed {keys[i]}) half {h} "
                                 f"index {j}: got {got[i, h, j]}, CPython {want[i, h, j]}")
    finally:
        g.free()


# ---- the two-kernel form ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree,bound", PAIRS)
def test_two_kernel_form_on_every_fixture(degree, bound):
    ctx = _ctx()
    keys = _good_keys(degree, bound)
    assert keys
    _check(ctx, keys, degree, bound)                             # one call per pair
    _check(ctx, keys + keys[:1], degree, bound)
    n = len(keys)
    for i, k in enumerate(keys):
        a, b = keys[(i + 1) % n], keys[(i + 2) % n]
        _check(ctx, [k], degree, bound)                          # a workgroup with two of its four waves live
        _check(ctx, [k, a], degree, bound)
        _check(ctx, [a, b, k], degree, bound)                    # the edge key last, in a ragged workgroup, right before the guard row
        _check(ctx, [k, a, b], degree, bound)


# ---- the one-kernel form, and the other side of the switch --------------------------------------------------------------------
@pytest.mark.parametrize("nkeys", [ONE_KERNEL_KEYS, ONE_KERNEL_KEYS - 1])
@pytest.mark.parametrize("degree,bound", PAIRS)
def test_both_forms_at_the_switch(degree, bound, nkeys):
    good = _good_keys(degree, bound)
    keys = [good[i % len(good)] for i in range(nkeys)]
    _check(_ctx(), keys, degree, bound)


# ---- exhaustion -----------------------------------------------------------------------------------------------------------------
def _limit_keys():
    fit = [fx[2] for fam in ("gens16", "exact_9984") for fx in E.FIXTURES[fam] if (fx[0], fx[1]) == (2496, 64)]
    short = [fx[2] for fx in E.FIXTURES["one_short"]]
    out = [fx[2] for fx in E.FIXTURES["runs_out"]]
    return sorted(set(fit)), short, out


@pytest.mark.parametrize("nkeys", [7, ONE_KERNEL_KEYS], ids=["two-kernel", "one-kernel"])
def test_the_generation_limit_from_both_sides(nkeys):
    """rows that need all 16 generations (exactly 9984 outputs among them) succeed; one row that needs 9985 outputs, or more,
    makes the call return FZ_E_UNSUPPORTED -- an ordinary error: the guard rows are intact and the next call succeeds"""
    import fusion_hip
    from fusion_hip._lib import FZ_E_UNSUPPORTED
    degree, bound = 2496, 64
    fit, short, out = _limit_keys()
    assert len(fit) >= 5 and all(E.plain_model(k + h, degree, bound)[1] <= E.AVAILABLE for k in fit for h in (0, 1))
    assert any(E.plain_model(k + h, degree, bound)[1] == E.AVAILABLE for k in fit for h in (0, 1))
    ctx = _ctx()
    good = [fit[i % len(fit)] for i in range(nkeys)]
    want = _want(good, degree, bound)
    g = Guarded(ctx, nkeys, degree)
    try:
        g.sample(good, bound)
        assert g.guards_intact() and np.array_equal(g.rows(), want)
        for bad_key in (short[0], short[1], out[0], out[1]):
            for pos in (0, nkeys // 2, nkeys - 1):
                keys = list(good)
                keys[pos] = bad_key
                with pytest.raises(fusion_hip.FusionHipError) as e:
                    g.sample(keys, bound)
                assert e.value.code == FZ_E_UNSUPPORTED, (bad_key, pos)
                assert g.guards_intact(), (bad_key, pos)
        g.sample(good, bound)                                    # the same context, after the refusals
        assert g.guards_intact() and np.array_equal(g.rows(), want)
    finally:
        g.free()


# ---- the bound's range ------------------------------------------------------------------------------------------------------------
def test_the_largest_bound_on_the_device_and_the_first_refused_one():
    import fusion_hip
    from fusion_hip._lib import FZ_E_UNSUPPORTED
    ctx = _ctx()
    keys = [0, 1, 2 ** 32 - 1, 2 ** 40 + 3, 77]
    _check(ctx, keys, 96, 2 ** 31 - 1)
    assert np.abs(_want(keys, 96, 2 ** 31 - 1).astype(np.int64)).max() > 2 ** 30
    g = Guarded(ctx, len(keys), 96)
    try:
        g.sample(keys, 2 ** 31 + 5)                              # capped by q // 2 = 2^31 - 1
        assert g.guards_intact() and np.array_equal(g.rows(), _want(keys, 96, 2 ** 31 - 1))
        for modulus, norm_bound in ((2 ** 34, 2 ** 31 + 100), (2 ** 32, 2 ** 31), (2 ** 40, 2 ** 32 - 1)):
            with pytest.raises(fusion_hip.FusionHipError) as e:
                g.sample(keys, norm_bound, modulus)
            assert e.value.code == FZ_E_UNSUPPORTED and "2^31 - 1" in str(e.value)
            assert g.guards_intact() and (g.rows() == E.POISON).all()        # refused before anything ran
    finally:
        g.free()


# ---- the scheme's face --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("secpar", [128, 256])
def test_keygen_batch_on_the_scheme_fixtures(secpar):
    """BatchScheme.keygen_batch on the bound-52 fixtures: the keys of fusion.keygen, and secret polynomials that are CPython's"""
    import fusion.fusion as F
    from fusion_hip.scheme import BatchScheme, signature_from_object
    params = F.fusion_setup(secpar, 42)
    d = params.degree
    assert params.beta_sk == 52 and params.omega_sk == d
    seeds = _good_keys(d, 52)
    assert len(seeds) >= 4
    bs = BatchScheme(params)
    assert bs.device_sampler
    sk, vk = bs.keygen_batch(seeds)
    assert bs.device_sampler                                     # no fallback happened
    n, l = len(seeds), sk.shape[2]
    coef = bs.ctx.ntt_inverse(np.ascontiguousarray(sk).reshape(-1, d)).reshape(n, 2, l, d)
    want = _want(seeds, d, 52)
    for r in range(l):                                           # every row of a secret matrix is the same polynomial
        assert np.array_equal(coef[:, :, r], want), r
    for i, s in enumerate(seeds):
        sk_o, vk_o = F.keygen(params, s)
        assert np.array_equal(vk[i, 0], np.array(vk_o.left_vk_hat.matrix[0][0].values)), s
        assert np.array_equal(vk[i, 1], np.array(vk_o.right_vk_hat.matrix[0][0].values)), s
        assert np.array_equal(sk[i, 0], signature_from_object(params, F.Signature(signature_hat=sk_o.left_sk_hat))), s
        assert np.array_equal(sk[i, 1], signature_from_object(params, F.Signature(signature_hat=sk_o.right_sk_hat))), s
