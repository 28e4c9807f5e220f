"""The many-committee compact-bytes kernels (aggregate_encoded_ragged, aggregate_target_encoded_ragged) at every multiply form and
field width, through their two C-ABI device entries, against the context-parametric spec of tests/_encoded_edges.py
(group_partials, group_targets): the 19 contexts of tests/test_gpu_encoded_edges.py at degrees 64 and 256 -- moduli on either side
of `fast`, four of them at or above 2^31, odd and top twiddle tables -- with fields at 0 and 2B in the stage sign patterns at
B = (q - 1) / 2, int32-extreme alpha_hat / vk / c_hat, group tables with empty groups, groups smaller than the slice count and
uneven slices, skip masks that empty a slice, a group and the whole call, 65 groups (two launches), every field width 2 .. 32 at
its smallest and largest bound, and sums of one sign at the largest magnitude a group can leave.

Nothing here is kernel against kernel.  The aggregates' int64 partials and d_out are compared bit for bit (every term is
canonical); the targets' partials are specified modulo q only, so their centred residues are compared, and each is held to
|t[g]| <= sizes[g] * (q // 2 + 2^18), target_slice's bound on a term.  Every output lies between guards with padded strides; after
every call the inputs read back unchanged and every guard and gap word is as it was.  No tolerance anywhere."""
import numpy as np
import pytest

import _encoded_edges as X
from test_gpu_aggregate_target_encoded import Guarded, O_FILL, P_FILL
from test_gpu_encoded_edges import _agg_ls, _cid, _ctx

pytestmark = pytest.mark.gpu

I32_MIN, I32_MAX = X.I32_MIN, X.I32_MAX
CASES = [(s, n) for s in X.SPECS for n in X.DEGREES]
SEAM_SPECS = [("scheme", "root"), ("top", "root"), ("w32", "odd"), ("m31", "odd")]
SWEEP_CASES = [(s, n) for s in X.SWEEP_SPECS for n in X.DEGREES]
SAME_SIGN_SPECS = [s for s in X.SPECS if s[1] == "root"]          # every one a prime modulus
SAME_SIGN_BOUNDS = {256: 3172, 64: 4264}                          # one signature's bound at the degree's parameter set
# one group of fewer than, as many as and more than the workgroup's four waves; empty groups first, in the middle and adjacent;
# a group smaller than the launch's slice count; slices of unequal length
SHAPES = ([1], [4], [5], [0, 1, 7], [3, 0, 0, 2], [40, 1], [67, 1, 33])
MASKS = ("none", "zeros", "thirds", "group", "all")


def mask_of(name, sizes):
    """the skip words of a mask: None; all zero; every third signer; every signer of the largest group; every signer"""
    N = sum(sizes)
    if name == "none":
        return None
    skip = np.zeros(N, dtype=np.int32)
    if name == "thirds":
        skip[::3] = 6
    elif name == "group":
        a, b = X.group_bounds(sizes)[int(np.argmax(sizes))]
        skip[a:b] = 3
    elif name == "all":
        skip[:] = 6
    return skip


def run_both(ctx, n, l, B, data, alpha, vk, chal, skip, sizes, pad=2):
    """both entries on the same device arrays -> ((partials [G][l][n] int64, out [G][l][n] int32) of
    fz_aggregate_encoded_ragged_async, (partials, targets [G][n] int64, out) of fz_aggregate_target_encoded_ragged_async);
    partials and targets lie `pad` words further apart than they are wide"""
    from fusion_hip import DeviceArray
    G, per = len(sizes), l * n
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    host = [np.ascontiguousarray(data, dtype=np.uint8), np.ascontiguousarray(alpha, dtype=np.int32), np.ascontiguousarray(vk, dtype=np.int32),
            np.ascontiguousarray(chal, dtype=np.int32)] + ([] if skip is None else [np.ascontiguousarray(skip, dtype=np.int32)])
    assert host[0].shape == (off[-1], X.record_bytes(n, l, X.width(B))) and host[0].shape[1] % 16 == 0
    dev = [DeviceArray.from_numpy(ctx, a) for a in host]
    dB, dA, dK, dC = (b.ptr for b in dev[:4])
    dS = dev[4].ptr if skip is not None else 0
    plain = [Guarded(ctx, G, per, per + pad, np.int64, P_FILL), Guarded(ctx, G, per, per, np.int32, O_FILL)]
    fused = [Guarded(ctx, G, per, per + pad, np.int64, P_FILL), Guarded(ctx, G, n, n + pad, np.int64, P_FILL), Guarded(ctx, G, per, per, np.int32, O_FILL)]
    try:
        ctx.aggregate_encoded_ragged_async_dev(dB, dA, dS, off, l, B, plain[0].ptr, per + pad, plain[1].ptr)
        ctx.synchronize()
        one = [x.read() for x in plain]
        ctx.aggregate_target_encoded_ragged_async_dev(dB, dA, dS, dK, dC, off, l, B, fused[0].ptr, per + pad, fused[1].ptr, n + pad, fused[2].ptr)
        ctx.synchronize()
        two = [x.read() for x in fused]
        for b, a in zip(dev, host):
            assert np.array_equal(b.numpy().reshape(a.shape), a), "an input was written"
    finally:
        for b in dev + [x.buf for x in plain + fused]:
            b.free()
    shape = (G, l, n)
    return (one[0].reshape(shape), one[1].reshape(shape)), (two[0].reshape(shape), two[1], two[2].reshape(shape))


def check(ctx, spec, n, l, B, z, alpha, vk, chal, skip, sizes, what, pad=2):
    """both entries on records z [N][l][n] at bound B, against the spec; skipped rows hold bytes 0xff and int32-extreme
    multipliers, which a kernel that read them would add -> what the entries left"""
    q = X.modulus(spec)
    data, st = X.encoded(z, B)
    assert not st.any()
    alpha, vk, chal = (np.array(a, dtype=np.int64) for a in (alpha, vk, chal))
    want_p = X.group_partials(spec, n, z, alpha, sizes, skip)
    want_t = X.group_targets(spec, vk, chal, alpha, sizes, skip)
    if skip is not None and skip.any():
        data = data.copy()
        data[skip != 0], alpha[skip != 0], vk[skip != 0], chal[skip != 0] = 0xff, I32_MAX, I32_MIN, I32_MAX
    one, two = run_both(ctx, n, l, B, data, alpha, vk, chal, skip, sizes, pad)
    for name, (p, o) in (("aggregate_encoded_ragged", one), ("aggregate_target_encoded_ragged", (two[0], two[2]))):
        assert np.array_equal(p, want_p), (name, "partials", what)
        assert np.array_equal(o, X.cent(want_p, q)), (name, "d_out", what)
    t = two[1]
    assert np.array_equal(X.cent(t, q), X.cent(want_t, q)), ("targets", what)
    assert (np.abs(t).max(axis=1) <= np.asarray(sizes) * (q // 2 + 2 ** 18)).all(), ("targets' size", what)
    kept = [(b - a if skip is None else int((skip[a:b] == 0).sum())) for a, b in X.group_bounds(sizes)]
    for g, k in enumerate(kept):
        assert k or not (one[0][g].any() or one[1][g].any() or two[0][g].any() or t[g].any() or two[2][g].any()), (what, g)
    return one, two


def tiled(pool, N):
    return pool[np.arange(N) % pool.shape[0]]


# ---- a. every context ----------------------------------------------------------------------------------------------------------
A_CASES = [(s, n, l) for s, n in CASES for l in _agg_ls(n)]


@pytest.mark.parametrize("case", A_CASES, ids=lambda c: f"{X.sid(c[0])}-d{c[1]}-l{c[2]}")
def test_every_context_at_every_group_shape_and_mask(case):
    """records tiled from five distinct ones of the decoder-side rows at B = (q - 1) / 2, alpha_hat, vk and c_hat at the int32
    extremes and random, at every group shape under every mask: no mask; all zeros, which leaves what no mask leaves; every
    third signer; every signer of the largest group; every signer, which leaves zeros.  Then the same with random fields that
    include 0 and 2B, at the narrowest bound (w = 2) and at the widest"""
    spec, n, l = case
    half = X.half(spec)
    _, rows = X.decoder_rows(spec, n)
    pools = [("rows", half, X.records_of(rows, l, 5))]
    pools += [(f"fields B={b}", b, X.edge_fields(b, 5, l, n, b % 1000 + n + l) - b) for b in sorted({1, half})]
    ctx = _ctx(spec, n)
    try:
        for name, B, pool in pools:
            for k, sizes in enumerate(SHAPES):
                N = sum(sizes)
                z = tiled(pool, N)
                alpha = X.multipliers(N, n, N + l)
                vk, chal = X.key_inputs(N, n, N + l + k)
                left = {}
                for mask in MASKS:
                    left[mask] = check(ctx, spec, n, l, B, z, alpha, vk, chal, mask_of(mask, sizes), sizes, (name, sizes, mask))
                same = zip(left["none"][0] + left["none"][1], left["zeros"][0] + left["zeros"][1])
                assert all(np.array_equal(a, b) for a, b in same), (name, sizes)      # the targets too, word for word
                assert left["none"][1][1].any() and not any(a.any() for a in left["all"][0] + left["all"][1]), (name, sizes)
    finally:
        ctx.close()


# ---- b. the 64-group seam ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(s, n) for s in SEAM_SPECS for n in X.DEGREES], ids=_cid)
def test_sixty_five_groups_are_the_spec_on_both_sides_of_the_seam(case):
    """65 groups of 1 and 2 signers run as two launches: every group against the spec, not only those beside the seam; with every
    third signer skipped the partials lie contiguous (one clear and one centring launch across the seam)"""
    spec, n = case
    l, B = (1 if n == 256 else 2), X.half(spec)
    sizes = [1 + g % 2 for g in range(65)]
    N = sum(sizes)
    z = tiled(X.records_of(X.decoder_rows(spec, n)[1], l, 5), N)
    alpha = X.multipliers(N, n, 65 + n)
    vk, chal = X.key_inputs(N, n, 66 + n)
    ctx = _ctx(spec, n)
    try:
        one, two = check(ctx, spec, n, l, B, z, alpha, vk, chal, None, sizes, "no mask")
        assert all(two[1][g].any() and one[0][g].any() for g in (63, 64))
        check(ctx, spec, n, l, B, z, alpha, vk, chal, mask_of("thirds", sizes), sizes, "thirds, contiguous", pad=0)
    finally:
        ctx.close()


# ---- c. every field width ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SWEEP_CASES, ids=_cid)
def test_every_field_width(case):
    """the ragged kernels unpack with instantiations of their own: every width the modulus admits at its smallest and largest
    bound, groups of 3 and 2 records of 1 row (degree 64: of 2, so that records stay multiples of 16 bytes), field 0, the last
    field and one in the middle at 0 and at 2B"""
    spec, n = case
    l, sizes = (2 if n == 64 else 1), [3, 2]
    ctx = _ctx(spec, n)
    seen = set()
    try:
        for w, B in X.SWEEP:
            if spec not in X.sweep_specs(B):
                continue
            seen.add(w)
            z = X.edge_fields(B, 5, l, n, 300 * w + n) - B
            vk, chal = X.key_inputs(5, n, w)
            check(ctx, spec, n, l, B, z, X.multipliers(5, n, w), vk, chal, None, sizes, (w, B))
    finally:
        ctx.close()
    assert seen == set(range(2, X.width(X.half(spec)) + 1))


# ---- d. sums of one sign -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sign", [1, -1], ids=["plus", "minus"])
@pytest.mark.parametrize("case", [(s, n) for s in SAME_SIGN_SPECS for n in X.DEGREES], ids=_cid)
def test_sums_of_one_sign_at_the_largest_magnitude(case, sign):
    """every product is sign * h, h = (q - 1) / 2: every partial of a group of N_g signers is sign * N_g * h and d_out its
    centred residue -- the fp64 lane sums and their meeting in LDS, the conversion of a negative sum to the atomics' unsigned
    words and the centring of the int64 sums, at the largest magnitude N_g signers can leave"""
    spec, n = case
    q, h, l, B = X.modulus(spec), X.half(spec), _agg_ls(n)[1], SAME_SIGN_BOUNDS[n]
    ctx = _ctx(spec, n)
    try:
        for sizes in ([67], [67, 1, 33]):
            N = sum(sizes)
            z, alpha = X.same_sign_inputs(spec, n, l, N, B, sign)
            vk, chal = X.key_inputs(N, n, N + n)
            one, two = check(ctx, spec, n, l, B, z, alpha, vk, chal, None, sizes, (sizes, sign))
            for p, o in (one, (two[0], two[2])):
                for g, ng in enumerate(sizes):
                    assert (p[g] == sign * ng * h).all() and (o[g] == X.E.cent(sign * ng * h, q)).all(), (sizes, sign, g)
    finally:
        ctx.close()
