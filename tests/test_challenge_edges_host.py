"""The fixtures of tests/_challenge_edges.py reach every edge they are meant to pin, the plain-Python model returns what the
reference returned for them (tests/golden/challenge_edges.npz), every plausible fault of a serialiser / sponge / decoder
changes the row of a fixture, and the C host pipeline (csrc/fz_host.cpp) agrees with the model on all of them.  No GPU."""
import hashlib
import json
import os

import numpy as np
import pytest

import _challenge_edges as E

G = os.path.join(os.path.dirname(__file__), "golden")
ALL_SETS = list(E.SETS)


@pytest.fixture(scope="module")
def hp():
    import __graft_entry__ as g
    g.build()
    from fusion_hip import hostpipe
    return hostpipe


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(G, "challenge_edges.npz"))


def _texts(ps, fx):
    return [E.text(ps, fx.vk[k, 0], fx.vk[k, 1], fx.ints[k]) for k in range(len(fx))]


def coverage_gaps(ps, fx):
    """the edges that the key / digest fixtures `fx` of parameter set `ps` do NOT reach (empty for a complete set)"""
    gaps = []
    d, n = ps.degree, 2 * ps.degree
    # ---- str(int(prehash)) ----
    chunks = [E.chunks_of(v) for v in fx.ints]
    if {len(str(v)) for v in fx.ints} != set(range(1, 79)):
        gaps.append("digit counts 1..78")
    if {len(c) for c in chunks} != set(range(1, 10)):
        gaps.append("chunk counts 1..9")
    if {len(str(c[-1])) for c in chunks} != set(range(1, 10)):
        gaps.append("top-chunk widths 1..9")
    for j in range(8):
        def others_full(c):
            return len(c) == 9 and all(10 ** 8 <= c[t] < 10 ** 9 - 1 for t in range(8) if t != j)
        for tag, cond in (("zero", lambda v: v == 0), ("all nines", lambda v: v == 10 ** 9 - 1), ("short", lambda v: 0 < v < 10 ** 8)):
            if not any(others_full(c) and cond(c[j]) for c in chunks):
                gaps.append(f"chunk {j} {tag}")
    if len({len(str(c[j])) for c in chunks for j in range(min(8, len(c) - 1))}) < 9:
        gaps.append("inner chunks of every width 1..9")
    # ---- padding ----
    lens = [len(t) for t in _texts(ps, fx)]
    missing = set(range(E.RATE)) - {v % E.RATE for v in lens}
    if missing:
        gaps.append(f"text lengths mod 136: {sorted(missing)[:8]} ... ({len(missing)} residues) never reached")
    shortest = len(E.text(ps, [0] * d, [0] * d, 0)) // E.RATE + 1
    longest = len(E.text(ps, [E.I32_MIN] * d, [E.I32_MIN] * d, 2 ** 256 - 1)) // E.RATE + 1
    if min(lens) // E.RATE + 1 != shortest or max(lens) // E.RATE + 1 != longest:
        gaps.append(f"block counts {shortest} and {longest}")
    # ---- dec_len and the character writer ----
    at = {(int(v), k) for row in fx.vk.reshape(len(fx), n) for k, v in enumerate(row)}
    slots = {(v, k % E.vpl(ps)) for v, k in at}
    for v in E.THRESHOLDS:
        if any((v, s) not in slots for s in range(E.vpl(ps))):
            gaps.append(f"value {v} in every slot of a lane")
        if any((v, k) not in at for k in (0, d - 1, d, n - 1)):
            gaps.append(f"value {v} at indices 0, degree - 1, degree, 2 * degree - 1")
    keys = fx.vk.reshape(len(fx), n)
    if not (keys == 0).all(axis=1).any():
        gaps.append("the all-zero key")
    if not any(all(len(str(int(v))) == 11 for v in row) for row in keys):
        gaps.append("a key of 2 * degree values of eleven characters")
    # ---- every form's last wave / workgroup partly empty: 64 signers per wave, 32, or 4 waves of one ----
    if len(fx) % 64 == 0 or len(fx) % 32 == 0 or len(fx) % 4 == 0:
        gaps.append(f"a batch of {len(fx)} leaves no wave partly empty")
    return gaps


@pytest.mark.parametrize("name", ALL_SETS)
def test_fixtures_reach_every_edge(name):
    ps, fx = E.SETS[name], E.fixtures(name)
    assert coverage_gaps(ps, fx) == []
    assert len(set(fx.names)) == len(fx)
    if ps.scheme:
        nb = [len(t) // E.RATE + 1 for t in _texts(ps, fx)]
        assert (min(nb), max(nb)) == {"s128": (7, 17), "s256": (15, 54)}[name]
    # the sweep alone: 136 consecutive lengths, from digests of two different digit counts at least
    sw = [k for k in range(len(fx)) if fx.family[k] == "sweep"]
    lens = sorted(len(E.text(ps, fx.vk[k, 0], fx.vk[k, 1], fx.ints[k])) for k in sw)
    assert lens == list(range(lens[0], lens[0] + E.RATE))
    assert len({len(str(fx.ints[k])) for k in sw}) >= 2
    if ps.scheme or name == "d128w64":                       # keys that differ only in how many values have two digits
        assert all(set(np.unique(fx.vk[k])) <= {7, 12} for k in sw)
    # the longest text fits the row that challenge_geometry (csrc/fz_staged_capi.hip) sizes: 13 bytes per value and 78 digits
    s0, s1, s2 = E.text_pieces(ps)
    blocks = (len(s0) + len(s1) + len(s2) + 2 * ps.degree * 13 + 78) // E.RATE + 1
    blocks += blocks & 1
    assert max(len(t) for t in _texts(ps, fx)) // E.RATE + 1 <= blocks


@pytest.mark.parametrize("family,expect", [("digest", "digit counts 1..78"), ("key", "value 0 in every slot of a lane"),
                                           ("sweep", "text lengths mod 136")])
def test_a_missing_family_is_noticed(family, expect):
    """the conditions above are not vacuous: without any one family they fail"""
    for name in ("s128", "d16"):
        gaps = coverage_gaps(E.SETS[name], E.Fixtures(E.SETS[name], drop=(family,)))
        assert any(g.startswith(expect) for g in gaps), (name, family, gaps)


def test_message_fixtures_reach_every_edge():
    msgs = E.message_fixtures()
    blen = [len(m.encode("utf-8")) for _, m in msgs]
    assert set(range(281)) <= set(blen)
    for k in range(1, 9):                                    # 3 prefix bytes + message + the suffix byte = k whole blocks, and one off
        assert {E.RATE * k - 5, E.RATE * k - 4, E.RATE * k - 3} <= set(blen), k
    multi = [len(m.encode("utf-8")) for _, m in msgs if len(m.encode("utf-8")) != len(m)]
    assert {131, 132, 133, 268} <= set(multi)
    # each long message shares its wave of 32 (lane-pair form) and of 64 (lane form) with short ones
    for at, n in E.LONG_MESSAGES.items():
        assert blen[at] == n
        assert all(blen[k] <= 2 * E.RATE for k in range(at // 64 * 64, at // 64 * 64 + 64) if k != at)
    assert len(msgs) % 64 and len(msgs) % 32 and len(msgs) % 4


def test_scheme_constants_are_the_scheme_s():
    import fusion.fusion as F
    for name in E.SCHEME_SETS:
        ps, params = E.SETS[name], F.fusion_setup(E.SETS[name].secpar, 5)
        for f in ("modulus", "degree", "root", "inv_root", "root_order", "omega_ch", "omega_ag", "beta_ch", "beta_ag",
                  "sign_pre_hash_dst", "sign_hash_dst", "agg_xof_dst"):
            assert getattr(ps, f) == getattr(params, f), (name, f)


@pytest.mark.parametrize("name", E.SCHEME_SETS)
def test_model_returns_what_the_reference_returned(name, golden):
    ps, fx = E.SETS[name], E.fixtures(name)
    assert str(golden[f"fixtures_sha256_{name}"]) == fx.sha256(), "fixtures changed: regenerate tests/golden/challenge_edges.npz"
    assert str(golden[f"messages_sha256_{name}"]) == E.messages_sha256(ps), "messages changed: regenerate the golden file"
    want, got = golden[f"rows_{name}"].astype(np.int32), E.model_rows(name)
    assert np.array_equal(got, want), [fx.names[k] for k in np.argwhere((got != want).any(axis=1))[:5, 0]]
    dig, rows = E.message_model(name)
    want = golden[f"message_rows_{name}"].astype(np.int32)
    assert np.array_equal(rows, want), [E.message_fixtures()[k][0] for k in np.argwhere((rows != want).any(axis=1))[:5, 0]]
    assert (np.abs(got).sum(axis=1) == ps.omega_ch).all() and (np.abs(rows).sum(axis=1) == ps.omega_ch).all()


def test_model_text_reproduces_the_reference_kat_rows():
    """hash_vk_and_int_to_bytes rows of the reference's KAT file (tests/golden/kat.json)"""
    with open(os.path.join(G, "kat.json")) as fh:
        rows = json.load(fh)["hash_vk_and_int_to_bytes"]
    assert rows
    ps = E.SETS["s128"]
    for r in rows:
        t = E.text(ps, r["vk_left"], r["vk_right"], int(r["i"]))
        assert hashlib.sha256(hashlib.shake_256(t).digest(r["n"])).hexdigest() == r["sha256_expected_bytes"]
        assert E.mech_blocks(ps, r["vk_left"], r["vk_right"], int(r["i"])) == E.padded(t)


@pytest.mark.parametrize("name", ALL_SETS)
def test_mechanical_statement_equals_the_model(name):
    """the text as the kernels build it and the plain sponge: equal to str() and hashlib on every fixture / on a sample"""
    ps, fx = E.SETS[name], E.fixtures(name)
    texts = _texts(ps, fx)
    for k, t in enumerate(texts):
        assert E.mech_blocks(ps, fx.vk[k, 0], fx.vk[k, 1], fx.ints[k]) == E.padded(t), fx.names[k]
    by_res = {len(t) % E.RATE: k for k, t in enumerate(texts)}
    for k in (0, by_res[0], by_res[1], by_res[134], by_res[135], len(fx) - 1):
        n = E.challenge_bytes(ps)
        assert E.sponge(E.padded(texts[k]), n) == hashlib.shake_256(texts[k]).digest(n), fx.names[k]
        assert E.mech_row(ps, fx.vk[k, 0], fx.vk[k, 1], fx.ints[k]) == E.model_rows(name)[k].tolist()


def fault_witnesses(name, fault, fx=None, limit=2):
    """(names of the fixtures whose padded blocks `fault` changes, names of those -- `limit` at most looked at -- whose ROW it
    changes)"""
    ps = E.SETS[name]
    fx = fx or E.fixtures(name)
    if fault in ("sign-bits-reversed", "mod-i"):             # the decoder's: the blocks stay, every row is a candidate
        cand = list(range(len(fx)))
    else:
        cand = [k for k in range(len(fx))
                if E.mech_blocks(ps, fx.vk[k, 0], fx.vk[k, 1], fx.ints[k], fault) != E.padded(E.text(ps, fx.vk[k, 0], fx.vk[k, 1], fx.ints[k]))]
    rows = [k for k in cand[:limit] if E.mech_row(ps, fx.vk[k, 0], fx.vk[k, 1], fx.ints[k], fault) != E.row(ps, fx.vk[k, 0], fx.vk[k, 1], fx.ints[k])]
    return [fx.names[k] for k in cand], [fx.names[k] for k in rows]


def _fid(f):
    return f if isinstance(f, str) else f"{f[0]}-{f[1]}"


@pytest.mark.parametrize("fault", E.FAULTS, ids=_fid)
@pytest.mark.parametrize("name", ["s128", "s256"])
def test_the_fixtures_can_fail(name, fault):
    """a pipeline with this fault would return a wrong row for at least one fixture"""
    ps, fx = E.SETS[name], E.fixtures(name)
    changed, wrong_rows = fault_witnesses(name, fault)
    assert wrong_rows, f"no fixture of {name} notices the fault {fault}"
    fam = {n.split(":")[0] for n in changed}
    res = {n: len(t) % E.RATE for n, t in zip(fx.names, _texts(ps, fx))}
    # each fault is found by the family built for it, and the padding faults ONLY at their residue
    if fault in ("no-zero-padding", "count-nonzero-chunks", "top-chunk-9-wide"):
        assert "digest" in fam, changed[:5]
    elif fault == "pad-assigned":
        assert {res[n] for n in changed} == {135}, changed[:5]
    elif fault == "blocks-ceil":
        assert {res[n] for n in changed} == {0}, changed[:5]
    elif fault not in ("sign-bits-reversed", "mod-i"):
        assert any(n.startswith("key:rot") for n in changed), changed[:5]
    if isinstance(fault, tuple):                             # the comparison with 10^k: exactly the keys that hold +-10^k
        k = fault[1]
        holds = {fx.names[i] for i in range(len(fx)) if (np.abs(fx.vk[i].astype(np.int64)) == 10 ** k).any()}
        assert set(changed) == holds and holds
    if fault == "abs-wraps":
        holds = {fx.names[i] for i in range(len(fx)) if (fx.vk[i] == E.I32_MIN).any()}
        assert set(changed) == holds and holds


@pytest.mark.parametrize("family,fault", [("digest", "count-nonzero-chunks"), ("key", ("dec-len-gt", 9)), ("key", "abs-wraps")])
def test_a_fault_needs_its_family(family, fault):
    """without the family built for it nothing finds the fault: the fixtures isolate their edges"""
    fx = E.Fixtures(E.SETS["s128"], drop=(family,))
    changed, _ = fault_witnesses("s128", fault, fx=fx, limit=0)
    assert changed == [], changed[:5]


# ---- the C host pipeline on the same fixtures ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_SETS)
def test_host_pipeline_pieces_equal_the_model(name, hp):
    """fz_format_vk + fz_shake256 + fz_decode_coefficients"""
    ps, fx = E.SETS[name], E.fixtures(name)
    P = hp.scheme_params(ps)
    want = E.model_rows(name)
    n = E.challenge_bytes(ps)
    bad = []
    for k in range(len(fx)):
        vk_text = hp.format_vk(P, fx.vk[k, 0], fx.vk[k, 1])
        assert vk_text == E.vk_text(ps, fx.vk[k, 0], fx.vk[k, 1]), fx.names[k]
        t = ps.sign_hash_dst + b"," + vk_text.encode() + b"," + str(fx.ints[k]).encode()
        got = hp.decode_coefficients(hp.shake256(t, n), ps.secpar, ps.modulus, ps.degree, ps.beta_ch, ps.omega_ch)
        if got.tolist() != want[k].tolist():
            bad.append(fx.names[k])
    assert not bad, bad[:8]


@pytest.mark.parametrize("name", ["s128", "s256", "d16"])
def test_host_aggregation_coefficients_print_every_digest(name, hp):
    """fz_aggregation_coefficients prints the injected digests through u256_decimal: one batch of every fixture, in sorted key
    order, against hash_vks_and_ints_and_challs_to_bytes + the decoder in plain Python"""
    from oracle.oracle import splitmix_centered
    ps, fx = E.SETS[name], E.fixtures(name)
    P = hp.scheme_params(ps)
    order = sorted(range(len(fx)), key=lambda k: E.vk_text(ps, fx.vk[k, 0], fx.vk[k, 1]))
    assert {fx.family[k] for k in order} == {"digest", "key", "sweep"}
    vk, pre = fx.vk[order], fx.pre[order]
    ints = [fx.ints[k] for k in order]
    c_hat = splitmix_centered(0xA66 + ps.degree, len(fx) * ps.degree).reshape(len(fx), ps.degree)
    want = np.array(E.aggregation_rows(ps, vk, ints, c_hat), dtype=np.int32)
    for threads in (1, 4):
        got = hp.aggregation_coefficients(P, np.ascontiguousarray(vk[:, 0]), np.ascontiguousarray(vk[:, 1]), pre, c_hat, threads=threads)
        assert np.array_equal(got, want), [fx.names[order[k]] for k in np.argwhere((got != want).any(axis=1))[:5, 0]]


@pytest.mark.parametrize("name", ALL_SETS)
def test_host_pipeline_on_the_message_fixtures(name, hp):
    """fz_challenge_coefficients: SHA3-256 of every message length, the digest printed by u256_decimal"""
    ps = E.SETS[name]
    P = hp.scheme_params(ps)
    vk = E.message_keys(ps)
    msgs = [m for _, m in E.message_fixtures()]
    dig, rows = E.message_model(name)
    coefs, pre = hp.challenge_coefficients(P, np.ascontiguousarray(vk[:, 0]), np.ascontiguousarray(vk[:, 1]), msgs)
    assert np.array_equal(pre, dig), [E.message_fixtures()[k][0] for k in np.argwhere((pre != dig).any(axis=1))[:5, 0]]
    assert np.array_equal(coefs, rows), [E.message_fixtures()[k][0] for k in np.argwhere((coefs != rows).any(axis=1))[:5, 0]]
