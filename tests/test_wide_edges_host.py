"""The generic int64 path without a GPU: the model and fixtures of tests/_wide_edges.py (every fixture carries the event it is named
after, no family is redundant, the step-by-step restatement equals the plain operations, every fault is noticed by a named case or
is argued equivalent, the composite fixtures tell the two scaling factors apart), the marshalling and routing of
algebra/_backend.py, the wide context cache, and every refusal of the four C entries (all argument checks precede the device)."""
import collections
import ctypes
from ctypes import POINTER, c_int32, c_int64, c_uint64

import numpy as np
import pytest

import _wide_edges as W

QS = list(W.MODULI.values())
IDS = list(W.MODULI)


# ---- moduli, fixtures, events ---------------------------------------------------------------------------------------------------
def test_the_moduli_are_what_their_lists_say():
    assert all(W.is_prime(q) for q in W.PRIMES.values())
    assert not any(W.is_prime(q) for q in W.COMPOSITES.values())
    assert all(q % 2 == 1 and 3 <= q < 2 ** 63 for q in QS) and len(set(QS)) == 15
    assert all(q % f == 0 and 1 < f < q for q, f in W.SMALL_FACTOR.items()) and set(W.SMALL_FACTOR) == set(W.COMPOSITES.values())
    assert (2 ** 63 - 1) % 49 == 0 and (2 ** 63 - 1) % 73 == 0
    assert not any(W.is_prime(q) for q in range(2 ** 63 - 24, 2 ** 63, 2))          # 2^63 - 25 is the largest prime the path accepts
    assert all(q % 2 ** 15 == 1 for q in (W.Q33, W.Q62, W.Q63)) and 2 ** 32 < W.Q33 < 2 ** 33 and W.Q62 < 2 ** 62 < W.Q63 < 2 ** 63


@pytest.mark.parametrize("q", QS, ids=IDS)
def test_every_fixture_carries_its_event_and_every_possible_event_has_fixtures(q):
    fx = W.fixtures(q)
    for kind, events in (("product", W.PRODUCT_EVENTS), ("wadd", W.ADD_EVENTS), ("wsub", W.SUB_EVENTS)):
        assert tuple(fx[kind]) == events
        for event, pairs in fx[kind].items():
            assert len(set(pairs)) == len(pairs)
            for a, b in pairs:
                assert 0 <= a < q and 0 <= b < q and event in W.events_of(kind, a, b, q), (kind, event, a, b)
            if kind == "product":
                assert len(pairs) == W.expected_count(event, q), (event, len(pairs))
            else:
                assert len(pairs) >= 1
    m = W.Model(q)
    cv = W.canon_values(q)
    assert {"0", "+1", "-1", "-q", "+q", "INT64_MIN", "INT64_MAX", "top", "bot", "top-1", "bot+1"} <= set(cv)
    assert cv["top"] % q == 0 and cv["top"] + q > W.INT64_MAX and cv["bot"] % q == 0 and cv["bot"] - q < W.INT64_MIN
    for name, x in cv.items():
        assert m.wcanon(x) == x % q, name
    if q == 2 ** 63 - 1:
        assert m.wcanon(W.INT64_MAX) == 0 and m.wcanon(W.INT64_MIN) == q - 1 and "+(q+1)" not in cv
    if q <= 7:                                             # half = 1 .. 3: INT64_MIN is folded by almost the whole type
        assert m.half == (q - 1) // 2 <= 3 and m.wcanon(W.INT64_MIN) == (-2 ** 63) % q
    h = (q - 1) // 2
    assert [m.wcent(v) for v in W.cent_values(q).values()] == [h, -h, -1, 0]
    assert [W.p_neg([v], q)[0] for v in W.neg_values(q).values()] == [0, -1, -(q - 1)]


def test_what_a_modulus_cannot_show_is_stated():
    """every product event with fewer than two pairs somewhere has its reason in CANNOT; the reasons' arithmetic claims hold"""
    for q in QS:
        for event, pairs in W.fixtures(q)["product"].items():
            if len(pairs) < {"hi_max": 1}.get(event, 2):
                assert any(ev == event and pred(q) for ev, _, pred, _ in W.CANNOT), (W.NAME_OF[q], event)
    for q in QS:
        if q < 2 ** 32:                                    # u <= q below 2^32: (q - 1)^2 + (2^64 - 1) q < (q + 1) 2^64
            assert (q - 1) ** 2 + (W.M64 - 1) * q < (q + 1) * W.M64
    for q in (2 ** 32 + 1, 2 ** 32 + 15, W.Q33):           # one operand below q with 32 factors of two
        assert [a for a in range(2 ** 32, q, 2 ** 32)] == [2 ** 32]


def test_no_family_of_fixtures_is_redundant():
    """for every family there is a modulus at which only that family's pairs show its event"""
    for kind, events in (("product", W.PRODUCT_EVENTS), ("wadd", W.ADD_EVENTS), ("wsub", W.SUB_EVENTS)):
        for event in events:
            alone = []
            for q in QS:
                fx = W.fixtures(q)[kind]
                if fx[event] and not any(event in W.events_of(kind, a, b, q) for other, pairs in fx.items() if other != event for a, b in pairs):
                    alone.append(q)
            assert alone, (kind, event)


# ---- the model ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", QS, ids=IDS)
def test_the_restatement_equals_the_plain_operations(q):
    m = W.Model(q)
    assert m.qneg_inv * q % W.M64 == W.M64 - 1 and m.r2 == pow(2, 128, q) and m.half == (q - 1) // 2
    for c in W.cases(q):
        assert c.model(m) == c.plain(q), c.name
    # table entries and n_inv at or above q (the C ABI takes any uint64): the same rows as the reduced values
    tab = [q, q + 1, W.M64 - 1, W.M64 - 2]
    rows = [1, q - 1, 2, (q - 1) // 2]
    red = [t % q for t in tab]
    assert m.ntt(rows, tab, 0) == m.ntt(rows, red, 0) == W.p_forward(rows, q, red)
    n_inv = W.scaling_factor(4, q)
    big = n_inv + (W.M64 - 1 - n_inv) // q * q
    assert big >= q and m.ntt(rows, tab, 1, n_inv=big) == m.ntt(rows, red, 1, n_inv=n_inv) == W.p_inverse(rows, q, red)


def test_the_events_occur_inside_the_kernels_that_are_said_to_have_them():
    """a product fixture's wmont(a, b) is really executed by the pointwise product, the length-2 transforms and the matvec cases"""
    for q in (2 ** 32 + 1, 3 * 2 ** 50 + 1, W.Q62, 2 ** 63 - 1):
        for event, pairs in W.fixtures(q)["product"].items():
            for n, (a, b) in enumerate(pairs):
                for c in W.cases(q):
                    if c.name.startswith(f"{W.NAME_OF[q]}/{event}#{n}/"):
                        tr = []
                        c.model(W.Model(q, trace=tr))
                        assert any((x, y) == (a, b) for x, y, *_ in tr), c.name


@pytest.mark.parametrize("fault", W.FAULTS)
def test_every_fault_is_noticed_by_a_named_case_or_is_equivalent(fault):
    noticed = {W.NAME_OF[q]: W.noticed_by(fault, q) for q in QS}
    total = sum(len(v) for v in noticed.values())
    if fault in W.EQUIVALENT:
        assert total == 0, (fault, "is listed as equivalent but changes", [v[0] for v in noticed.values() if v])
        assert len(W.EQUIVALENT[fault]) > 40              # the argument is written down
    else:
        assert total > 0, f"{fault}: no case of any modulus notices it"
        assert NOTICED_AT[fault] == {n for n, v in noticed.items() if v}, (fault, sorted(n for n, v in noticed.items() if v))


ALL = set(IDS)
WIDE = {n for n, q in W.MODULI.items() if q > 2 ** 32}
R_IS_NOT_1 = ALL - {"q3", "q5", "q65537", "2^32-1", "2^32+1"}        # 2^64 = 1 (mod q) exactly when q divides 2^64 - 1 = 3 5 17 257 641 65537 6700417
# fault -> the moduli at which some case notices it (the model's own statement, pinned so that a change of fixtures shows here)
NOTICED_AT = {
    "carry_always_1": ALL, "carry_always_0": ALL,
    "carry_if_operands_nonzero": WIDE,                     # only lo0_nonzero pairs tell it from the right carry: q > 2^32
    "canon_no_sign_fix": ALL, "canon_unsigned": ALL, "wcent_ge": ALL, "half_plus_1": ALL, "neg_centred": ALL,
    "mul_no_r2": R_IS_NOT_1, "r2_single": R_IS_NOT_1, "matvec_no_r2": R_IS_NOT_1,
    # four iterations give the inverse to 48 bits: the upper 16 are right by accident at most of these moduli
    "newton_4": {"q3", "q5", "2^32-5"},
    "n_inv_modular_inverse": {"2^32-1", "3*2^50+1", "2^63-1"},
    "fwd_twiddle_i": ALL, "inv_twiddle_mm": ALL, "scale_forward": ALL,
}


def test_the_fault_table_is_complete():
    assert set(NOTICED_AT) | set(W.EQUIVALENT) == set(W.FAULTS) and not set(NOTICED_AT) & set(W.EQUIVALENT)
    assert all(q not in (3, 5, 65537, 2 ** 32 - 1, 2 ** 32 + 1) or (2 ** 64 - 1) % q == 0 for q in QS)
    assert {n for n, q in W.MODULI.items() if (2 ** 64 - 1) % q} == R_IS_NOT_1


def test_the_composite_fixtures_tell_the_two_scaling_factors_apart():
    """n^(q-2) and n^-1 differ at 2^32 - 1, 3 2^50 + 1 and 2^63 - 1 for n = 2, 8 and 64, agree at 2^32 + 1 and at every prime; the
    inverse-transform cases of the three moduli change under the modular inverse"""
    for q in QS:
        for n in (2, 8, 64):
            same = pow(n, q - 2, q) == pow(n, -1, q)
            assert same == (q in W.PRIMES.values() or q == 2 ** 32 + 1), (q, n)
    for q in (2 ** 32 - 1, 3 * 2 ** 50 + 1, 2 ** 63 - 1):
        names = W.noticed_by("n_inv_modular_inverse", q)
        assert names and all("/inv" in n for n in names)
        assert any(n.endswith("/random/inv4") for n in names) and any(n.endswith("/inv2") for n in names)


# ---- algebra/_backend.py: marshalling and routing, no device ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    import fusion_hip
    return fusion_hip.load_library()


@pytest.mark.parametrize("q", [2 ** 32 + 1, 2 ** 32 + 15, W.Q62, 2 ** 63 - 25, 2 ** 63 - 1])
def test_to_i32_on_a_wide_modulus(lib, q):
    from algebra._backend import to_i32
    h = q // 2
    flat = [h, -h, h + 1, -(h + 1), 0, 1, -1, q, -q, q - 1, 1 - q]
    huge = [2 ** 63, 2 ** 63 + 5, -2 ** 63 - 1, -2 ** 64, 3 * q + 7, 2 ** 200 + 1, -2 ** 63, 2 ** 63 - 1]
    for rows in (flat, huge, flat + huge, [flat, flat[::-1]], [flat + huge, (flat + huge)[::-1]], [], [[]], [[], []]):
        a = to_i32(rows, q)
        assert a.dtype == np.int64
        want = [[W.cent(v, q) for v in r] for r in rows] if rows and isinstance(rows[0], list) else [W.cent(v, q) for v in rows]
        assert a.tolist() == want, rows
    assert to_i32([h + 1], q).tolist() == [-h] and to_i32([-(h + 1)], q).tolist() == [h]


@pytest.mark.parametrize("q", [3, 65537, 2147465729, 2 ** 32 - 5, 2 ** 32 - 1])
def test_to_i32_on_a_narrow_modulus(lib, q):
    """int32 rows: values that fit int32 are handed over as they are (the int32 entries reduce unreduced rows), values beyond are
    the centred residue; everything is congruent to what went in"""
    from algebra._backend import to_i32
    h = q // 2
    fits = [h, -h, h + 1, -(h + 1), 0, 1, -1, 2 ** 31 - 1, -2 ** 31]
    beyond = [2 ** 31, -2 ** 31 - 1, 2 ** 32, 2 ** 63, -2 ** 63 - 1, 2 ** 63 - 1, -2 ** 63, 2 ** 200 + 1]
    for rows in (fits, beyond, fits + beyond, [fits, fits[::-1]], [fits + beyond, (fits + beyond)[::-1]], [], [[]]):
        a = to_i32(rows, q)
        assert a.dtype == np.int32
        nested = bool(rows) and isinstance(rows[0], list)
        got, src = (sum(a.tolist(), []), sum(rows, [])) if nested else (a.tolist(), rows)
        assert len(got) == len(src) and a.ndim == (2 if nested else 1)
        reduced = any(not -2 ** 31 <= v < 2 ** 31 for v in src)
        for g, v in zip(got, src):
            assert (g - v) % q == 0 and (g == (W.cent(v, q) if reduced else v)), (v, g)


def test_routing_between_the_two_contexts(lib, monkeypatch):
    import algebra._backend as B
    import fusion_hip.context
    import fusion_hip.wide
    calls = []
    monkeypatch.setattr(B, "get_context", lambda *a: calls.append(("int32", a[:2])) or "int32")
    monkeypatch.setattr(fusion_hip.context, "get_table_context", lambda *a: calls.append(("int32-table", a[:2])) or "int32")
    monkeypatch.setattr(fusion_hip.wide, "get_wide_context", lambda *a: calls.append(("generic", a[:2])) or "generic")
    narrow = 2 ** 32 - 5
    for q, d, route in ((narrow, 4096, "int32"), (narrow, 8192, "generic"), (2 ** 32 + 15, 2, "generic"), (65537, 2, "int32")):
        assert B.ntt_ctx(q, d, 3, pow(3, q - 2, q)) == route, (q, d)
        assert B.table_ctx(q, d, list(range(d)), list(range(d))) == route, (q, d)
    assert B.ring_ctx(narrow, 8192) == "int32" and B.ring_ctx(65537, 1 << 20) == "int32"          # no transform: the degree does not matter
    assert B.ring_ctx(2 ** 32 + 15, 2) == "generic" and B.ring_ctx(2 ** 63 - 25, 8192) == "generic"
    assert [c[0] for c in calls] == ["int32", "int32-table", "generic", "generic", "generic", "generic", "int32", "int32-table", "int32", "int32",
                                     "generic", "generic"]
    assert calls[2][1] == (narrow, 8192) and calls[4][1] == (2 ** 32 + 15, 2)
    assert B.is_wide(2 ** 32) and not B.is_wide(2 ** 32 - 1)


def test_check_modulus_refuses_what_the_kernels_do_not_take(lib):
    import fusion_hip
    from algebra._backend import check_modulus, ntt_ctx, ring_ctx, table_ctx
    for bad in (1, 2, 0, -3, 4, 6, 2 ** 32, 2 ** 40, 2 ** 62, 2 ** 63, 2 ** 63 + 1, 2 ** 64 + 1, 7.0, "7", None, np.int64(7), (7,)):
        for f in (check_modulus, lambda q: ntt_ctx(q, 8, 1, 1), lambda q: table_ctx(q, 8, [0] * 8, [0] * 8), lambda q: ring_ctx(q, 8)):
            with pytest.raises(fusion_hip.FusionHipError) as e:
                f(bad)
            assert e.value.code == -2 and "3 <= q < 2^63" in str(e.value) and "no CPU fallback" in str(e.value), bad
    for good in (3, 5, 2 ** 32 - 1, 2 ** 32 + 1, 2 ** 63 - 1):
        check_modulus(good)


# ---- the wide context cache (constructing a context loads the library and touches no device) -------------------------------------
def test_the_wide_context_cache(lib, monkeypatch):
    import fusion_hip.wide as FW
    monkeypatch.setattr(FW, "_WIDE_CACHE", collections.OrderedDict())
    q, d = 2 ** 32 + 15, 4
    t1, t2 = (1, 2, 3, 4), (1, 2, 3, 5)
    a = FW.get_wide_context(q, d, t1, t1)
    b = FW.get_wide_context(q, d, t2, t1)
    assert a is not b and FW.get_wide_context(q, d, t1, t1) is a and FW.get_wide_context(q, d, t2, t1) is b
    assert FW.get_wide_context(q, d) is not a and len(FW._WIDE_CACHE) == 3
    assert list(a._tables[0]) == [1, 2, 3, 4] and list(b._tables[0]) == [1, 2, 3, 5] and a._n_inv == pow(4, q - 2, q)
    FW._WIDE_CACHE.clear()
    ctxs = [FW.get_wide_context(q, 2 ** k) for k in range(1, 9)]              # eight keys: full
    assert len(FW._WIDE_CACHE) == FW._WIDE_MAX == 8
    assert FW.get_wide_context(q, 2) is ctxs[0]                              # a hit refreshes its position: 4 is now the oldest
    ninth = FW.get_wide_context(q, 2 ** 9)
    assert len(FW._WIDE_CACHE) == 8 and FW.get_wide_context(q, 2 ** 9) is ninth
    assert [k[1] for k in FW._WIDE_CACHE] == [8, 16, 32, 64, 128, 256, 2, 512]
    assert FW.get_wide_context(q, 2) is ctxs[0]                              # survived the eviction
    assert FW.get_wide_context(q, 4) is not ctxs[1]                          # the least recently used one did not
    # the scaling factor a context hands over is the reference's expression, composite modulus or not
    for qq in (2 ** 32 - 1, 2 ** 32 + 1, 3 * 2 ** 50 + 1, 2 ** 63 - 1, 2 ** 63 - 25):
        for n in (2, 8, 64):
            assert FW.WideContext(qq, n, [0] * n, [0] * n)._n_inv == W.scaling_factor(n, qq)
        assert FW.WideContext(qq, 8)._n_inv == 0


# ---- the C entries' refusals: every argument check precedes the device ------------------------------------------------------------
BAD_MODULI = (0, 1, 2, 2 ** 40, 2 ** 63, 2 ** 63 + 1, 2 ** 64 - 1)
BADARG, UNSUPPORTED, NODEVICE = -1, -2, -4


def _p(a, t=c_int64):
    return a.ctypes.data_as(POINTER(t))


def _refused(lib, rc, code, phrase):
    msg = (lib.fz_last_error() or b"").decode()
    assert rc == code and phrase in msg, (rc, msg)


def _valid(lib, rc):
    """a valid non-empty call: no device here, so FZ_E_NODEVICE (with a device it runs)"""
    msg = (lib.fz_last_error() or b"").decode()
    n = ctypes.c_int(0)
    lib.fz_device_count(ctypes.byref(n))
    if n.value > 0:
        assert rc == 0, msg
    else:
        assert rc == NODEVICE and "no HIP device available" in msg, (rc, msg)


def test_refusals_of_the_transform_entry(lib):
    q = 2 ** 32 + 15
    x, y = np.arange(8, dtype=np.int64), np.full(8, -7, dtype=np.int64)
    tab = (c_uint64 * 8)(*range(8))
    f = lib.fz_wide_ntt_host
    for d in (0, 1, 3, 12, -4):
        _refused(lib, f(0, q, d, tab, 1, 0, _p(x), _p(y), 1), BADARG, "power of two")
    for bad in BAD_MODULI:
        _refused(lib, f(0, bad, 8, tab, 1, 0, _p(x), _p(y), 1), UNSUPPORTED, "odd, 3 <= q < 2^63")
        _refused(lib, f(0, bad, 8, tab, 1, 0, _p(x), _p(y), 0), UNSUPPORTED, "odd, 3 <= q < 2^63")       # even with nothing to do
    _refused(lib, f(0, q, 8, None, 1, 0, _p(x), _p(y), 1), BADARG, "NULL argument")
    _refused(lib, f(0, q, 8, None, 1, 0, None, None, 0), BADARG, "NULL argument")                       # the table is always needed
    _refused(lib, f(0, q, 8, tab, 1, 0, None, _p(y), 1), BADARG, "NULL argument")
    _refused(lib, f(0, q, 8, tab, 1, 1, _p(x), None, 1), BADARG, "NULL argument")
    _refused(lib, f(0, q, 8, tab, 1, 0, _p(x), _p(y), 2 ** 31), BADARG, "2^31 - 1 rows")
    assert f(0, q, 8, tab, 1, 0, None, None, 0) == 0 and f(0, q, 8, tab, 1, 1, _p(x), _p(y), 0) == 0
    assert y.tolist() == [-7] * 8
    _valid(lib, f(0, q, 8, tab, 1, 0, _p(x), _p(y), 1))


def test_refusals_of_the_pointwise_entry(lib):
    q = 2 ** 32 + 15
    x, y, z = np.arange(4, dtype=np.int64), np.arange(4, dtype=np.int64), np.full(4, -7, dtype=np.int64)
    f = lib.fz_wide_pw_host
    for op in (-1, 4, 100):
        _refused(lib, f(0, q, op, _p(x), _p(y), _p(z), 4), BADARG, f"bad op {op}")
    for bad in BAD_MODULI:
        for op in range(4):
            _refused(lib, f(0, bad, op, _p(x), _p(y), _p(z), 4), UNSUPPORTED, "odd, 3 <= q < 2^63")
    _refused(lib, f(0, q, 0, None, _p(y), _p(z), 4), BADARG, "NULL argument")
    _refused(lib, f(0, q, 1, _p(x), None, _p(z), 4), BADARG, "NULL argument")
    _refused(lib, f(0, q, 2, _p(x), _p(y), None, 4), BADARG, "NULL argument")
    _refused(lib, f(0, q, 3, None, None, _p(z), 4), BADARG, "NULL argument")
    assert f(0, q, 0, None, None, None, 0) == 0 and f(0, q, 3, _p(x), None, _p(z), 0) == 0
    assert z.tolist() == [-7] * 4
    _valid(lib, f(0, q, 3, _p(x), None, _p(z), 4))                       # negation takes no second operand
    _valid(lib, f(0, q, 0, _p(x), _p(y), _p(z), 4))


def test_refusals_of_the_matvec_entry(lib):
    q = 2 ** 32 + 15
    A, S, out = np.arange(6, dtype=np.int64), np.arange(12, dtype=np.int64), np.full(6, -7, dtype=np.int64)
    f = lib.fz_wide_matvec_host
    for d, l in ((0, 2), (-1, 2), (3, 0), (3, -1)):
        _refused(lib, f(0, q, d, _p(A), _p(S), _p(out), 2, l), BADARG, "must be positive")
    for bad in BAD_MODULI:
        _refused(lib, f(0, bad, 3, _p(A), _p(S), _p(out), 2, 2), UNSUPPORTED, "odd, 3 <= q < 2^63")
    for args in ((None, _p(S), _p(out)), (_p(A), None, _p(out)), (_p(A), _p(S), None)):
        _refused(lib, f(0, q, 3, *args, 2, 2), BADARG, "NULL argument")
    assert f(0, q, 3, None, None, None, 0, 2) == 0 and f(0, q, 3, _p(A), _p(S), _p(out), 0, 2) == 0
    assert out.tolist() == [-7] * 6
    _valid(lib, f(0, q, 3, _p(A), _p(S), _p(out), 2, 2))


def test_refusals_of_the_norm_weight_entry(lib):
    rows = np.arange(6, dtype=np.int64)
    mx, wt = np.full(2, 9, dtype=np.uint64), np.full(2, -7, dtype=np.int32)
    f = lib.fz_wide_norm_weight_host
    for d in (0, -1):
        _refused(lib, f(0, _p(rows), 2, d, _p(mx, c_uint64), _p(wt, c_int32)), BADARG, "must be positive")
    for args in ((None, _p(mx, c_uint64), _p(wt, c_int32)), (_p(rows), None, _p(wt, c_int32)), (_p(rows), _p(mx, c_uint64), None)):
        _refused(lib, f(0, args[0], 2, 3, args[1], args[2]), BADARG, "NULL argument")
    _refused(lib, f(0, _p(rows), 2 ** 31, 3, _p(mx, c_uint64), _p(wt, c_int32)), BADARG, "2^31 - 1 rows")
    assert f(0, None, 0, 3, None, None) == 0 and f(0, _p(rows), 0, 3, _p(mx, c_uint64), _p(wt, c_int32)) == 0
    assert mx.tolist() == [9, 9] and wt.tolist() == [-7, -7]
    _valid(lib, f(0, _p(rows), 2, 3, _p(mx, c_uint64), _p(wt, c_int32)))
