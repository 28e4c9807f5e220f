"""The fixtures of tests/_sampler_edges.py show the events they are labelled with and no family of them can be dropped, the
plain model is CPython's `random` driven the reference's way (algebra/polynomials.py:436-467), the step-by-step restatement of
mt_draw_kernel (csrc/fz_sample.hip) equals it, and every fault switch of the restatement changes a named fixture's row, its
fail verdict, or a word outside the row -- so a kernel with that fault fails tests/test_gpu_sampler_edges.py.  Then the host
clone (fz_sample_secret_polys, fz_sample_coefficients_state) against the same model, and the largest bound the int32
coefficients hold."""
import random
import types

import numpy as np
import pytest

import _sampler_edges as E

FX = E.all_fixtures()


def _id(fx):
    return f"d{fx[0]}-b{fx[1]}-k{fx[2]}-h{fx[3]}-{'+'.join(fx[4])}"


# ---- fixtures -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fx", FX, ids=_id)
def test_fixture_shows_its_events_and_the_models_agree(fx):
    degree, bound, key_seed, half, events = fx
    s = key_seed + half
    shown = E.classify(s, degree, bound)
    assert set(events) <= shown, (fx, sorted(shown))
    want, used = E.plain_model(s, degree, bound)                # asserts == random.Random(s) driven the reference's way
    assert ("runs_out" in shown) == (used > E.AVAILABLE)
    row, fail, outside = E.mech_row(s, degree, bound)
    assert fail == (used > E.AVAILABLE) and outside == 0
    if not fail:
        assert np.array_equal(row, want)


def test_plain_model_consumption_is_cpythons():
    """the count of consumed outputs: the generator afterwards is where CPython's is"""
    for degree, bound, key_seed, half, _ in FX[::5]:
        s = key_seed + half
        rng = random.Random(s)
        for _ in range(degree):
            rng.randrange(bound), rng.randrange(2)
        used = E.plain_model(s, degree, bound)[1]
        assert int(E.stream(s, used + 1)[used]) == rng.getrandbits(32), (s, degree, bound)


def test_seeding_model_is_cpythons():
    for s in (0, 1, 5, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 40 + 7, 2 ** 64 - 2):
        assert tuple(E.init_by_array(E.key_words(s))) + (E.GEN,) == random.Random(s).getstate()[1], s
        assert np.array_equal(E.stream_of_key(E.key_words(s), 700), E.stream(s, 700)), s


def test_every_family_is_needed():
    assert E.coverage_gaps(E.FIXTURES) == []
    assert set(E.FIXTURES) == set(E.EVENTS)
    for fam in E.FIXTURES:
        rest = {k: v for k, v in E.FIXTURES.items() if k != fam}
        assert E.coverage_gaps(rest), f"the fixtures of {fam} add nothing"
    # the scheme's two sets, a power-of-two bound, rows above 624 coefficients, the smallest and the largest bound
    pairs = {(f[0], f[1]) for f in FX}
    assert {(256, 52), (64, 52), (256, 64), (2400, 64), (2496, 64), (1, 1), (2, 2 ** 31 - 1), (700, 3)} <= pairs
    # no key of a batch that must succeed runs out; every key of the two failing families does
    for fam, fxs in E.FIXTURES.items():
        for fx in fxs:
            assert E.key_fails(fx) == (fam in ("one_short", "runs_out")), fx
    # the failing keys fail by the labelled half alone
    for fam in ("one_short", "runs_out"):
        for degree, bound, key_seed, half, _ in E.FIXTURES[fam]:
            assert not E.runs_out(key_seed + 1 - half, degree, bound)


# ---- faults -------------------------------------------------------------------------------------------------------------------
# fault -> (family, index) of the fixtures that must notice it
NOTICED_BY = {
    "sentinel_em": [("pass", 0), ("pass2", 1)],
    "sentinel_es": [("pass2", 0), ("pass", 2)],
    "sentinel_apply": [("carry_pass0", 0), ("carry_pass0", 1), ("chain", 0), ("chain", 1)],      # nothing but these two families does
    "compose_order": [("pass62", 0)],
    "cm_for_cs": [("carry", 0)],
    "drop_carry": [("carry", 1), ("carry", 3)],
    "pad_real": [("pass62", 2)],
    "lane62_full": [("carry_pass0", 1)],
    "no_guard": [("end_mid_lane", 1), ("end_mid_lane", 3), ("end_mid_lane", 5)],
    "limit15": [("exact_9984", 0), ("gens16", 3)],
    "limit17": [("one_short", 0), ("one_short", 1)],
    "kbits_minus": [("end_last", 0), ("nomag", 0)],
    "sign_low": [("end_mid_lane", 3), ("gens1", 0)],
    "swap_halves": [("gens1", 0), ("gens2", 0)],
    "key_word": [("gens1", 0), ("pass", 0), ("gens3", 2)],
}


def _notices(fx, fault):
    degree, bound, key_seed, half, _ = fx
    fails = E.key_fails(fx)
    if fault in ("swap_halves", "key_word"):                    # faults of the launcher's part: the whole key, guard rows included
        buf, fail, beyond = E.mech_batch([key_seed], degree, bound, fault)
        return bool(fail != fails or beyond or (buf[[0, 3]] != E.POISON).any()
                    or (not fails and not np.array_equal(buf[1:3], E.expected_key(key_seed, degree, bound))))
    s = key_seed + half
    row, fail, outside = E.mech_row(s, degree, bound, fault)
    want, used = E.plain_model(s, degree, bound)
    return bool(fail != (used > E.AVAILABLE) or outside or (not fail and not np.array_equal(row, want)))


def test_every_fault_has_named_fixtures():
    assert set(NOTICED_BY) == set(E.FAULTS)


@pytest.mark.parametrize("fault", E.FAULTS)
def test_fault_changes_a_named_fixture(fault):
    for fam, i in NOTICED_BY[fault]:
        fx = E.FIXTURES[fam][i]
        assert not _notices(fx, None), (fam, i)
        assert _notices(fx, fault), (fault, fam, i, fx)


def test_the_rare_branch_is_seen_by_its_own_families_only():
    """apply()'s carry_mag branch with a pass-through (fault sentinel_apply): among all fixtures, exactly those that show
    carry_pass0 notice it -- the arbitrary seeds of the other sampler tests do not reach it (17 in 40 000 seeds do)"""
    for fx in FX:
        if fx[0] > 700:
            continue                                            # (the long rows say the same and take a second each)
        shown = E.classify(fx[2] + fx[3], fx[0], fx[1])
        assert _notices(fx, "sentinel_apply") == ("carry_pass0" in shown), fx


def test_the_write_guard_fault_leaves_the_row_and_hits_the_guard_row():
    degree, bound, key_seed, half, _ = E.FIXTURES["end_mid_lane"][1]
    buf, fail, beyond = E.mech_batch([key_seed], degree, bound, "no_guard")
    assert not fail and ((buf[3] != E.POISON).any() or beyond)             # the last row's stray writes land behind the output
    buf, fail, beyond = E.mech_batch([key_seed], degree, bound)
    assert not fail and beyond == 0 and (buf[[0, 3]] == E.POISON).all()


# ---- the host clone ---------------------------------------------------------------------------------------------------------------
Q_MAX = 2 ** 32 - 1                  # the modulus only caps the bound at q // 2 = 2^31 - 1


def test_host_clone_equals_the_plain_model_on_every_fixture():
    from fusion_hip import hostpipe
    for degree, bound in sorted({(f[0], f[1]) for f in FX}):
        keys = sorted({f[2] for f in FX if (f[0], f[1]) == (degree, bound)})           # the host clone has no output limit
        got = hostpipe.sample_secret_polys(np.array(keys, dtype=np.uint64), Q_MAX, degree, bound, degree, threads=2)
        for i, k in enumerate(keys):
            assert np.array_equal(got[i], E.expected_key(k, degree, bound)), (degree, bound, k)


# a seed whose 4475th coefficient has magnitude 2147483673 at norm bound 2^31 + 100 (the 17 886th output of its generator,
# 0x80000018, is kept as a magnitude): before the entries refused such bounds they stored it as +2147483623
WRAP_SEED, WRAP_DEGREE, WRAP_INDEX, WRAP_Q, WRAP_BOUND = 82, 4480, 4474, 2 ** 34, 2 ** 31 + 100


def test_a_bound_above_int32_is_refused():
    from fusion_hip import hostpipe
    from fusion_hip._lib import FZ_E_UNSUPPORTED, FusionHipError
    want = E.cpython_poly(WRAP_SEED, WRAP_DEGREE, WRAP_BOUND)
    assert want[WRAP_INDEX] == -2147483673 and max(abs(v) for v in want) > 2 ** 31 - 1     # no int32 row can equal CPython's
    calls = [lambda: hostpipe.sample_coefficients(WRAP_SEED, WRAP_Q, WRAP_DEGREE, WRAP_BOUND, WRAP_DEGREE),
             lambda: hostpipe.sample_coefficients_with_state(WRAP_SEED, WRAP_Q, WRAP_DEGREE, WRAP_BOUND, WRAP_DEGREE),
             lambda: hostpipe.sample_secret_polys([WRAP_SEED], WRAP_Q, WRAP_DEGREE, WRAP_BOUND, WRAP_DEGREE, threads=2),
             lambda: hostpipe.sample_secret_polys([WRAP_SEED - 1], WRAP_Q, WRAP_DEGREE, 2 ** 31, WRAP_DEGREE, threads=1)]
    for call in calls:
        with pytest.raises(FusionHipError) as e:
            call()
        assert e.value.code == FZ_E_UNSUPPORTED and "2^31 - 1" in str(e.value)
    # nothing is drawn with weight bound 0: the bound does not matter then (as for the empty-range check)
    assert not hostpipe.sample_coefficients(WRAP_SEED, WRAP_Q, 8, WRAP_BOUND, 0).any()


def test_the_largest_bound_is_exact_on_the_host():
    """bound 2^31 - 1 (modulus 2^32 - 1): magnitudes up to 2^31 - 1, both signs, the state afterwards included"""
    from fusion_hip import hostpipe
    bound, degree = 2 ** 31 - 1, 96
    seeds = [0, 1, 2 ** 32 - 1, 2 ** 40 + 3]
    got = hostpipe.sample_secret_polys(np.array(seeds, dtype=np.uint64), Q_MAX, degree, 2 ** 31 + 5, degree, threads=2)    # capped by q // 2
    for i, s in enumerate(seeds):
        assert np.array_equal(got[i], E.expected_key(s, degree, bound)), s
    assert np.abs(got.astype(np.int64)).max() > 2 ** 30
    row, state = hostpipe.sample_coefficients_with_state(7, Q_MAX, degree, bound, degree)
    rng = random.Random(7)
    assert row.tolist() == [(1 + rng.randrange(bound)) * (1 - 2 * rng.randrange(2)) for _ in range(degree)]
    assert state == rng.getstate()[1]


def test_sample_half_falls_back_to_python_for_a_refused_bound(monkeypatch):
    """fusion.fusion._sample_half catches the refusal and lets the Python sampler produce the result -- here the reference's
    own error for such a ring, after its draws on the process-global generator"""
    import fusion.fusion as F
    from fusion_hip import hostpipe
    from fusion_hip._lib import FZ_E_UNSUPPORTED, FusionHipError
    seen = []
    real = hostpipe.sample_coefficients_with_state

    def spy(*a):
        try:
            return real(*a)
        except FusionHipError as e:
            seen.append(e.code)
            raise
    monkeypatch.setattr(hostpipe, "sample_coefficients_with_state", spy)
    p = types.SimpleNamespace(modulus=WRAP_Q, degree=8, beta_sk=WRAP_BOUND, omega_sk=8, root_order=16, root=3, inv_root=3)
    with pytest.raises(ValueError):                              # PolynomialCoefficientRepresentation's: 16 does not divide 2^34 - 1
        F._sample_half(p, 5)
    assert seen == [FZ_E_UNSUPPORTED]
    rng = random.Random(5)
    for _ in range(8):
        rng.randrange(WRAP_BOUND), rng.randrange(2)
    assert random.getstate() == rng.getstate()                   # the Python sampler ran: its draws are on the global generator
    # ... and the largest accepted bound takes the C path and equals CPython
    p = types.SimpleNamespace(modulus=Q_MAX, degree=8, beta_sk=2 ** 31 - 1, omega_sk=8, root_order=16, root=3, inv_root=3)
    assert F._sample_half(p, 5).tolist() == E.cpython_poly(5, 8, 2 ** 31 - 1)
    assert seen == [FZ_E_UNSUPPORTED]
