"""The device key sort of hash_ag for many committees (fz_sort_by_vk_string_ragged_dev: a wave per committee), the entries built on
it and BatchScheme(key_sort="device"), on a GPU.

1. The order, against hostpipe.sort_by_vk_string_ragged and -- committees of 16 keys or fewer -- against Python's sorted() of the
   key objects' str(): hand-built keys that first differ at coefficient 0, 1, 7, 8, d - 2, d - 1 of the left row and 0, d - 1 of the
   right row, with values whose decimals are prefixes of each other, negative values and both ends of int32 there; identical keys;
   committees of 1, 2, 63, 64, 65 and 130 keys in one call and one of 300 alone.
2. Masks: the host order filtered, compacted committee after committee, nothing written behind the last valid row.
3. fz_hash_ag_ragged_sorted_dev against fz_hash_ag_ragged_dev fed the host sort's order: every row of alpha_hat, bit for bit.
4. fz_challenge_hat_msgs_keep_dev against fz_challenge_hat_msgs_dev: digests and c_hat, on both of its paths.
5. BatchScheme(hash_ag="device", key_sort="device") against hash_ag="device" and against the default scheme, keys on the device,
   with the host sort made to raise."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
Q = 2147465729
TRAPS = [0, 1, 10, 12, 123, -1, -12, -123, 9, -9, 2147483647, -2147483648, (Q - 1) // 2, -(Q - 1) // 2]
SENTINEL = 0xFFFFFFF0


def _positions(d):
    return [(0, 0), (0, 1), (0, 7), (0, 8), (0, d - 2), (0, d - 1), (1, 0), (1, d - 1)]


def trap_committees(d, rng):
    """a committee per position: keys equal everywhere but there, where they take every trap value; then committees with 2, 3 and 5
    identical keys among distinct ones"""
    base = rng.integers(-50, 50, size=(2, d)).astype(np.int64)
    out = []
    for half, pos in _positions(d):
        rows = np.repeat(base[None], len(TRAPS), axis=0)
        rows[:, half, pos] = TRAPS
        out.append(rows[rng.permutation(len(TRAPS))])
    for same in (2, 3, 5):
        rows = np.repeat(base[None], same + 4, axis=0)
        rows[same:, 0, 0] = [12, 123, -12, 1]
        out.append(rows[rng.permutation(same + 4)])
    return out


def mixed_committee(n, d, rng):
    """n keys around one base key: each differs from it at one of the positions, by a trap value; about one in eight is a copy of
    the key before it.  Most pairs agree on coefficient 0, so the order is decided further along, in either row"""
    base = rng.integers(-2 ** 31, 2 ** 31, size=(2, d)).astype(np.int64)
    rows = np.repeat(base[None], n, axis=0)
    pos = _positions(d)
    for i in range(n):
        if i and rng.integers(8) == 0:
            rows[i] = rows[i - 1]
            continue
        half, p = pos[rng.integers(len(pos))]
        rows[i, half, p] = TRAPS[rng.integers(len(TRAPS))]
    return rows


def _cat(groups):
    vk = np.ascontiguousarray(np.concatenate(groups).astype(np.int32))
    return vk, [len(g) for g in groups]


@pytest.fixture(scope="module")
def schemes():
    import fusion.fusion as F
    from fusion_hip.scheme import BatchScheme
    made = {}

    def get(secpar):
        if secpar not in made:
            made[secpar] = BatchScheme(F.fusion_setup(secpar, 11), hash_ag="device", key_sort="device")
        return made[secpar]
    yield get
    for bs in made.values():
        bs.close()


def _host_order(bs, vk, sizes):
    from fusion_hip import hostpipe
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return hostpipe.sort_by_vk_string_ragged(bs.P, vk[:, 0], vk[:, 1], off, 4), off


def _check_order(bs, vk, sizes):
    from fusion_hip.scheme import vk_to_object
    want, off = _host_order(bs, vk, sizes)
    got = bs.sort_keys_many_dev(vk, sizes)
    assert got.dtype == np.int64 and got.shape == want.shape
    for g, (a, b) in enumerate(zip(off[:-1], off[1:])):
        assert np.array_equal(got[a:b], want[a:b]), (g, b - a, got[a:b], want[a:b])
        if b - a <= 16:
            texts = {i: str(vk_to_object(bs.params, vk[i])) for i in range(a, b)}
            assert list(got[a:b]) == sorted(range(a, b), key=lambda i: texts[i]), g


# ---- 1. the order ---------------------------------------------------------------------------------------------------------------------
def test_order_on_the_trap_keys_and_every_tile_count_in_one_call(schemes):
    bs = schemes(128)
    d = bs.d
    rng = np.random.default_rng(1)
    groups = trap_committees(d, rng) + [mixed_committee(n, d, rng) for n in (1, 2, 63, 64, 65, 130)]
    groups.append(rng.integers(-2 ** 31, 2 ** 31, size=(70, 2, d)))          # decided on coefficient 0, as real keys are
    vk, sizes = _cat(groups)
    _check_order(bs, vk, sizes)
    # the prefix rule flips at a row's last coefficient: "12" before "123" inside a row, behind it at the end
    got = bs.sort_keys_many_dev(vk, sizes)
    off = np.concatenate([[0], np.cumsum(sizes)])
    for g, (half, pos) in enumerate(_positions(d)):
        vals = [int(vk[i, half, pos]) for i in got[off[g]:off[g + 1]]]
        assert (vals.index(123) < vals.index(12)) == (pos == d - 1), (g, vals)
        neg = [-123, -12, -1] if pos == d - 1 else [-1, -12, -123]           # by their digits, and by what follows the shorter one
        assert [v for v in vals if v in neg] == neg and vals.index(-123) < vals.index(-2147483648) < vals.index(0), (g, vals)


def test_order_of_one_committee_of_300(schemes):
    bs = schemes(128)
    _check_order(bs, *_cat([mixed_committee(300, bs.d, np.random.default_rng(2))]))


def test_order_on_the_trap_keys_at_secpar_256(schemes):
    bs = schemes(256)
    rng = np.random.default_rng(3)
    _check_order(bs, *_cat(trap_committees(bs.d, rng) + [mixed_committee(65, bs.d, rng)]))


def test_order_of_device_resident_keys_is_the_same(schemes):
    from fusion_hip.context import DeviceArray
    bs = schemes(128)
    vk, sizes = _cat([mixed_committee(n, bs.d, np.random.default_rng(4)) for n in (5, 66)])
    dK = DeviceArray.from_numpy(bs.ctx, vk)
    try:
        assert np.array_equal(bs.sort_keys_many_dev(dK, sizes), _host_order(bs, vk, sizes)[0])
    finally:
        dK.free()


# ---- 2. masks -------------------------------------------------------------------------------------------------------------------------
def test_masked_order_is_the_host_order_filtered_and_compacted(schemes):
    from fusion_hip.context import DeviceArray
    bs = schemes(128)
    rng = np.random.default_rng(5)
    groups = [mixed_committee(n, bs.d, rng) for n in (9, 14, 7, 70, 1, 64)]
    vk, sizes = _cat(groups)
    n = len(vk)
    want, off = _host_order(bs, vk, sizes)
    valid = rng.integers(0, 2, size=n).astype(bool)
    valid[off[0]:off[1]] = False                                             # no valid row
    valid[off[1]:off[2]] = False
    valid[off[2] - 1] = True                                                 # only the last row
    valid[off[2]:off[3]] = True                                              # every row
    filtered = want[valid[want]]
    assert np.array_equal(bs.sort_keys_many_dev(vk, sizes, valid), filtered)
    dK, dO = DeviceArray.from_numpy(bs.ctx, vk), DeviceArray.from_numpy(bs.ctx, np.full(n + 8, SENTINEL, dtype=np.uint32))
    try:
        bs.ctx.sort_by_vk_string_ragged_dev(bs.P, dK.ptr, n, off, valid, dO.ptr)
        got = dO.numpy()
    finally:
        dK.free()
        dO.free()
    m = int(valid.sum())
    assert np.array_equal(got[:m], filtered) and (got[m:] == SENTINEL).all()


# ---- 3. the coefficients ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("secpar", [128, 256])
def test_sorted_entry_writes_what_the_entry_writes_for_the_host_order(schemes, secpar, masked):
    from fusion_hip.context import DeviceArray
    bs = schemes(secpar)
    d = bs.d
    rng = np.random.default_rng(secpar + masked)
    traps = trap_committees(d, rng)
    groups = [traps[5][:1], traps[7][:2], traps[9][:5], mixed_committee(64, d, rng), mixed_committee(65, d, rng)]
    groups[1][1] = groups[1][0]                                              # one key twice, with different messages: the callers' order
    vk, sizes = _cat(groups)
    assert sizes == [1, 2, 5, 64, 65]
    n = len(vk)
    pre = rng.integers(0, 256, size=(n, 32)).astype(np.uint8)
    c_hat = rng.integers(-2 ** 31, 2 ** 31, size=(n, d)).astype(np.int32)
    order, off = _host_order(bs, vk, sizes)
    valid = None
    goff = off
    if masked:
        valid = rng.integers(0, 4, size=n) > 0
        valid[:3] = True
        valid[off[2]:off[3]] = False                                        # a committee without a valid signer
        valid[off[4] - 1] = False
        keep = valid[order]
        counts = np.add.reduceat(keep.astype(np.int64), off[:-1])
        order = order[keep]
        goff = np.concatenate([[0], np.cumsum(counts[counts > 0])])
    bufs = [DeviceArray.from_numpy(bs.ctx, a) for a in (vk, pre, c_hat)]
    outs = [DeviceArray.from_numpy(bs.ctx, np.full((n, d), 0x5A5A5A5A, dtype=np.int32)) for _ in range(2)]
    try:
        bs.ctx.hash_ag_ragged_dev(bs.P, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, n, order, goff, outs[0].ptr)
        bs.ctx.hash_ag_ragged_sorted_dev(bs.P, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, n, off, valid, outs[1].ptr)
        want, got = outs[0].numpy(), outs[1].numpy()
    finally:
        for b in bufs + outs:
            b.free()
    assert want.any() and np.array_equal(got, want)
    if masked:
        assert not got[~valid].any()
    assert not np.array_equal(got[1], got[2])                                # (the twin keys' rows differ: their order mattered)


# ---- 4. the digests ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5, 4609])
def test_keep_entry_leaves_the_same_digests_and_challenges(schemes, n):
    from fusion_hip import hostpipe
    from fusion_hip.context import DeviceArray
    bs = schemes(128)
    d = bs.d
    rng = np.random.default_rng(n)
    vk = rng.integers(-2 ** 31, 2 ** 31, size=(n, 2, d)).astype(np.int32)
    msgs = ["", "x" * 137, "a", "é" * 200, "m" * 135][:n] + [f"message {i}" * (i % 23) for i in range(5, n)]
    blob, moff = hostpipe._pack_messages(msgs)
    dK = DeviceArray.from_numpy(bs.ctx, vk)
    dC = [DeviceArray.from_numpy(bs.ctx, np.full((n, d), 0x5A5A5A5A, dtype=np.int32)) for _ in range(2)]
    dP = DeviceArray.from_numpy(bs.ctx, np.full((n + 1, 32), 0xA5, dtype=np.uint8))
    try:
        pre = bs.ctx.challenge_msgs_dev(bs.P, dK.ptr, blob, moff, n, dC[0].ptr, True)
        bs.ctx.challenge_msgs_keep_dev(bs.P, dK.ptr, blob, moff, n, dC[1].ptr, dP.ptr)
        kept = dP.numpy()
        assert np.array_equal(kept[:n], pre) and (kept[n] == 0xA5).all()
        assert np.array_equal(dC[1].numpy(), dC[0].numpy())
        assert np.array_equal(pre, hostpipe.hash_messages(bs.P, msgs))
    finally:
        for b in [dK, dP] + dC:
            b.free()


# ---- 5. end to end ----------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b


def test_many_committee_methods_with_the_device_sort_equal_the_host_sort(monkeypatch):
    import fusion.fusion as F
    from fusion_hip import hostpipe
    from fusion_hip.context import DeviceArray
    from fusion_hip.scheme import BatchScheme
    params = F.fusion_setup(128, 11)
    sizes = [1, 2, 3, 5, 9, 4]
    n = sum(sizes)
    off = np.concatenate([[0], np.cumsum(sizes)])
    msgs = [f"committee message {i}" for i in range(n)]
    plain, dev, both = BatchScheme(params), BatchScheme(params, hash_ag="device"), BatchScheme(params, hash_ag="device", key_sort="device")
    dK = None
    try:
        sk, vk = plain.keygen_batch([4000 + i for i in range(n)])
        sig = plain.sign_batch(sk, vk, msgs)
        data, codes = plain.encode("signature", sig)
        assert not codes.any()
        arecs = plain.encode("aggregate", plain.aggregate_many(vk, msgs, sig, sizes))[0]
        tampered = data.copy()
        tampered[off[:-1], 5] ^= 1                                           # one signature per committee is no longer its signer's
        dK = DeviceArray.from_numpy(plain.ctx, vk)
        runs = {
            "aggregate_verify_many_encoded": lambda bs: bs.aggregate_verify_many_encoded(dK, msgs, data, sizes),
            "aggregate_many_encoded[screened, tampered]": lambda bs: bs.aggregate_many_encoded(dK, msgs, tampered, sizes, screened=True),
            "verify_many_encoded": lambda bs: bs.verify_many_encoded(dK, msgs, arecs, sizes),
            "aggregate_many": lambda bs: bs.aggregate_many(dK, msgs, sig, sizes),
            "verify_many": lambda bs: bs.verify_many(dK, msgs, plain.decode("aggregate", arecs)[0], sizes),
        }
        down = []
        numpy_of = DeviceArray.numpy
        for name, run in runs.items():
            want = run(dev)
            with monkeypatch.context() as mp:
                for fn in ("sort_by_vk_string", "sort_by_vk_string_ragged"):
                    mp.setattr(hostpipe, fn, lambda *a, _fn=fn, **k: pytest.fail(f"hostpipe.{_fn} ran"))
                mp.setattr(DeviceArray, "numpy", lambda self: (down.append((self.shape, str(self.dtype))), numpy_of(self))[1])
                got = run(both)
            assert _same(got, want), name
            assert _same(got, run(plain)), name
            assert ((n, 2, params.degree), "int32") not in down and ((n, 32), "uint8") not in down, (name, down)
            if "tampered" in name:
                assert (want[1][off[:-1]] != 0).all() and not np.delete(want[1], off[:-1]).any()
                assert not want[0][0].any() and want[0][1].any()           # the lone signer's committee has no accepted signer left
            if name == "aggregate_verify_many_encoded":
                assert want[2] == [(True, "")] * len(sizes)
            if name.startswith("verify_many"):
                assert want == [(True, "")] * len(sizes)
        assert both.device_hash_ag and both.device_hash
    finally:
        if dK is not None:
            dK.free()
        for bs in (plain, dev, both):
            bs.close()


def test_drop_in_face_passes_the_option_on(monkeypatch):
    import fusion.fusion as F
    from fusion_hip.context import Context
    params = F.fusion_setup(128, 9)
    keys = [F.keygen(params, 700 + i) for i in range(4)]
    msgs = [f"drop-in {i}" for i in range(4)]
    blobs = [F.sign_to_bytes(params, k, mm) for k, mm in zip(keys, msgs)]
    kg, mg, bg = [[k[1] for k in keys[:1]], [k[1] for k in keys[1:]]], [msgs[:1], msgs[1:]], [blobs[:1], blobs[1:]]
    calls = []
    entry = Context.hash_ag_ragged_sorted_dev
    monkeypatch.setattr(Context, "hash_ag_ragged_sorted_dev", lambda self, *a: (calls.append(1), entry(self, *a))[1])
    want = F.aggregate_verify_many_from_bytes(params, kg, mg, bg)
    got = F.aggregate_verify_many_from_bytes(params, kg, mg, bg, hash_ag="device", key_sort="device")
    assert len(calls) == 1 and got[1] == want[1] == [(True, ""), (True, "")]
    assert [str(a) for a in got[0]] == [str(a) for a in want[0]]
    aggs = F.aggregate_many_from_bytes(params, kg, mg, bg, hash_ag="device", key_sort="device")
    assert [str(a) for a in aggs] == [str(a) for a in want[0]]
    recs = [F.to_bytes(params, a, aggregate=True) for a in aggs]
    assert F.verify_many_from_bytes(params, kg, mg, recs, hash_ag="device", key_sort="device") == [(True, ""), (True, "")] and len(calls) == 3
