"""Every form of the device challenge pipeline (FZ_SHAKE_FORM = 1: a Keccak state on a lane pair, 2: on a lane, 3: on a wave
with the whole pipeline of a signer fused; and the default choice) on the fixtures of tests/_challenge_edges.py: digests of every
digit count, chunk count and chunk shape; key values on every dec_len threshold in every slot of a lane and at the ends of both
rows, raw int32 extremes, the shortest and the longest text; texts of every length mod 136; messages of every length up to two
blocks, on the block boundaries up to eight blocks and of 20 000 / 200 000 bytes among short ones.

Expected rows: the plain-Python model of that module (str(), hashlib, the decoder on int.from_bytes) and, for the two scheme
sets, what the reference itself returned (tests/golden/challenge_edges.npz); transforms by the C oracle.  Bit-exact.  The
batches (387 signers, 311 messages) leave the last wave / workgroup of every form partly empty; the output buffer is poisoned
and the row after the batch must keep its poison."""
import hashlib
import os

import numpy as np
import pytest

import _challenge_edges as E

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
POISON = 0x5A5A5A5A

CASES = [(name, form) for name in E.SCHEME_SETS for form in ("1", "2", "3", None)] + \
    [(name, form) for name in E.EXTRA_SETS for form in ("1", "3")]


def _cid(c):
    return f"{c[0]}-form{c[1] or 'default'}"


def _context(ps, form, monkeypatch):
    """a fresh context: the knob is read when it is created"""
    import fusion_hip
    if form is None:
        monkeypatch.delenv("FZ_SHAKE_FORM", raising=False)
    else:
        monkeypatch.setenv("FZ_SHAKE_FORM", form)
    ctx = fusion_hip.Context(ps.modulus, ps.degree, ps.root, ps.inv_root)
    monkeypatch.delenv("FZ_SHAKE_FORM", raising=False)
    return ctx


def _wrong(got, want, names):
    return [names[k] for k in np.argwhere((got != want).any(axis=1))[:8, 0]]


@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_key_and_digest_fixtures(case, coracle, monkeypatch):
    import fusion_hip
    from fusion_hip import hostpipe
    name, form = case
    ps, fx = E.SETS[name], E.fixtures(name)
    n, d = len(fx), ps.degree
    assert n % 64 and n % 32 and n % 4
    want = E.model_rows(name)
    if ps.scheme:
        gold = np.load(os.path.join(G, "challenge_edges.npz"))
        assert str(gold[f"fixtures_sha256_{name}"]) == fx.sha256()
        assert np.array_equal(gold[f"rows_{name}"].astype(np.int32), want)
    P = hostpipe.scheme_params(ps)
    ctx = _context(ps, form, monkeypatch)
    dvk = fusion_hip.DeviceBuffer.from_numpy(ctx, fx.vk)
    dout = fusion_hip.DeviceBuffer(ctx, (n + 1) * d * 4)
    poison = np.full((n + 1, d), POISON, dtype=np.int32)
    try:
        ctx.h2d(dout.ptr, poison)
        ctx.challenge_dev(P, dvk.ptr, fx.pre, n, dout.ptr, transform=False)
        got = dout.to_numpy(np.int32, (n + 1, d))
        assert (got[n] == POISON).all(), "the row after the batch was written"
        assert np.array_equal(got[:n], want), _wrong(got[:n], want, fx.names)
        ctx.h2d(dout.ptr, poison)
        ctx.challenge_dev(P, dvk.ptr, fx.pre, n, dout.ptr, transform=True)
        got = dout.to_numpy(np.int32, (n + 1, d))
        hat = coracle.ntt_forward(want, ps.modulus, ps.root).reshape(n, d)
        assert (got[n] == POISON).all(), "the row after the batch was written"
        assert np.array_equal(got[:n], hat), _wrong(got[:n], hat, fx.names)
    finally:
        dvk.free()
        dout.free()
        ctx.close()


@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_message_fixtures(case, coracle, monkeypatch):
    import fusion_hip
    from fusion_hip import hostpipe
    name, form = case
    ps = E.SETS[name]
    d = ps.degree
    names = [nm for nm, _ in E.message_fixtures()]
    msgs = [m for _, m in E.message_fixtures()]
    n = len(msgs)
    assert n % 64 and n % 32 and n % 4
    vk = E.message_keys(ps)
    dig, rows = E.message_model(name)
    for k in (0, 1, 100, 200, n - 1):
        assert bytes(dig[k]) == hashlib.sha3_256(ps.sign_pre_hash_dst + b"," + msgs[k].encode("utf-8")).digest()
    if ps.scheme:
        gold = np.load(os.path.join(G, "challenge_edges.npz"))
        assert str(gold[f"messages_sha256_{name}"]) == E.messages_sha256(ps)
        assert np.array_equal(gold[f"message_rows_{name}"].astype(np.int32), rows)
    hat = coracle.ntt_forward(rows, ps.modulus, ps.root).reshape(n, d)
    blob, off = hostpipe._pack_messages(msgs)
    P = hostpipe.scheme_params(ps)
    ctx = _context(ps, form, monkeypatch)
    dvk = fusion_hip.DeviceBuffer.from_numpy(ctx, vk)
    dout = fusion_hip.DeviceBuffer(ctx, (n + 1) * d * 4)
    poison = np.full((n + 1, d), POISON, dtype=np.int32)
    try:
        ctx.h2d(dout.ptr, poison)
        pre = ctx.challenge_msgs_dev(P, dvk.ptr, blob, off, n, dout.ptr, want_prehash=True)
        assert np.array_equal(pre, dig), _wrong(pre, dig, names)
        got = dout.to_numpy(np.int32, (n + 1, d))
        assert (got[n] == POISON).all(), "the row after the batch was written"
        assert np.array_equal(got[:n], hat), _wrong(got[:n], hat, names)
        # once more from a non-zero origin in the keys, the offsets and the output: the long messages lie behind it
        k = 77
        ctx.h2d(dout.ptr, poison)
        pre = ctx.challenge_msgs_dev(P, dvk.ptr + k * 2 * d * 4, blob, off[k:], n - k, dout.ptr + k * d * 4, want_prehash=True)
        assert np.array_equal(pre, dig[k:]), _wrong(pre, dig[k:], names[k:])
        got = dout.to_numpy(np.int32, (n + 1, d))
        assert (got[:k] == POISON).all() and (got[n] == POISON).all(), "rows outside the batch were written"
        assert np.array_equal(got[k:n], hat[k:]), _wrong(got[k:n], hat[k:], names[k:])
    finally:
        dvk.free()
        dout.free()
        ctx.close()
