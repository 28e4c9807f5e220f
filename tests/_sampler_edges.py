"""Fixtures that put the device key sampler (csrc/fz_sample.hip: CPython's MT19937 sampler, mt_sample_kernel and
mt_seed_kernel + mt_draw_kernel) on the edges its control logic depends on, and two models of it in plain Python.

The operation: a secret polynomial is `degree` pairs (1 + randrange(bound)) * (1 - 2 * randrange(2)) drawn from
random.Random(seed) (algebra/polynomials.py:436-467 with weight bound = degree; fusion.py:339-362: the left half of a key is
seeded with the key's seed, the right half with seed + 1).  randrange(n) keeps getrandbits(n.bit_length()) if it is below n.

- stream(s, n) is the generator's first n 32-bit outputs, taken from CPython itself (getrandbits(32 * n) is n outputs, least
  significant first).  plain_model() is the operation written on that stream; it asserts that it equals random.Random(s)
  driven the reference's way, and also says how many outputs were consumed.  It calls nothing of this project.
- mech_draw() restates mt_draw_kernel step by step: generation g holds outputs 624 g .. 624 g + 623, lane L owns ten slots
  10 L .. 10 L + 9 of it (lane 62: four outputs and six padding slots, lane 63: padding only), walks them from both entry
  states ("magnitude next" and "sign pending"), the summaries (em, cm, es, cs) are composed over the wave by six shuffle
  steps (es == 0xffffffff: no sign taken, the pending magnitude passes through), shifted by one lane, applied to the
  wave-uniform carry (carry_mag, t), and every lane walks once more from its true entry state and writes under the guard
  tl < degree; after 16 generations (9984 outputs) the call fails.  mech_batch() puts the launcher's part around it (the
  polynomial's seed and half, the key words of init_by_array, kbits) and writes into a poisoned buffer with a guard row on
  either side.  Every plausible fault is a switch (FAULTS); tests/test_sampler_edges_host.py shows that each changes a named
  fixture's row, its fail verdict, or a word outside the row.
- classify() names the events of a (seed, degree, bound) triple (EVENTS); search() (python -m tests._sampler_edges --search,
  not run by the tests) finds seeds per event; FIXTURES are the seeds it found, committed as literals."""
import functools
import random
import sys

import numpy as np

GEN = 624                       # outputs per generation
PER_LANE = 10
MAX_GENERATIONS = 16
AVAILABLE = GEN * MAX_GENERATIONS          # 9984
SENT = 0xffffffff
POISON = -(2 ** 31)             # never a coefficient: |coefficient| <= bound <= 2^31 - 1

EVENTS = ("pass", "pass2", "pass62", "carry", "carry_pass0", "chain", "nomag", "end_last", "end_first", "end_mid_lane",
          "gens1", "gens2", "gens3", "gens16", "exact_9984", "one_short", "runs_out")
FAULTS = ("sentinel_em", "sentinel_es", "sentinel_apply", "compose_order", "cm_for_cs", "drop_carry", "pad_real", "lane62_full", "no_guard", "limit15",
          "limit17", "kbits_minus", "sign_low", "swap_halves", "key_word")


# ---- the stream and the plain model ---------------------------------------------------------------------------------------------
def stream(s, n):
    """the first n outputs of random.Random(s), uint32"""
    return np.frombuffer(random.Random(s).getrandbits(32 * n).to_bytes(4 * n, "little"), dtype="<u4")


def cpython_poly(s, degree, bound):
    """the reference's sampler on CPython's generator"""
    rng = random.Random(s)
    return [(1 + rng.randrange(bound)) * (1 - 2 * rng.randrange(2)) for _ in range(degree)]


def _draw_plain(y, degree, bound):
    """-> (row, outputs consumed), or (None, None) if y is too short"""
    k = bound.bit_length()
    v, sg = (y >> np.uint32(32 - k)).tolist(), (y >> np.uint32(30)).tolist()
    row, i, n = [], 0, len(v)
    for _ in range(degree):
        while i < n and v[i] >= bound:          # randrange(bound)
            i += 1
        if i >= n:
            return None, None
        mag = 1 + v[i]
        i += 1
        while i < n and sg[i] >= 2:             # randrange(2): getrandbits(2) kept if below 2
            i += 1
        if i >= n:
            return None, None
        row.append(mag * (1 - 2 * sg[i]))
        i += 1
    return row, i


@functools.lru_cache(maxsize=None)
def plain_model(s, degree, bound):
    """-> (row as a read-only int64 array, outputs consumed); asserts the row is CPython's"""
    n = GEN * (4 * degree // GEN + 2)
    while True:
        row, used = _draw_plain(stream(s, n), degree, bound)
        if row is not None:
            break
        n *= 2
    assert row == cpython_poly(s, degree, bound), (s, degree, bound)
    row = np.array(row, dtype=np.int64)
    row.flags.writeable = False
    return row, used


def runs_out(s, degree, bound):
    return plain_model(s, degree, bound)[1] > AVAILABLE


def expected_key(key_seed, degree, bound):
    """[2][degree] int64: the key's left (seed) and right (seed + 1) polynomial"""
    return np.stack([plain_model(key_seed + h, degree, bound)[0] for h in (0, 1)])


# ---- events -------------------------------------------------------------------------------------------------------------------
def classify(s, degree, bound):
    """the set of EVENTS that the polynomial of generator seed s shows.  Lane events count where the kernel's walk can still
    matter: in the first 16 generations, in lanes that begin at or before the output that completes the row."""
    k = bound.bit_length()
    n = GEN * (4 * degree // GEN + 2)
    while True:
        y = stream(s, n)
        okm, oks = ((y >> np.uint32(32 - k)) < bound).tolist(), ((y >> np.uint32(30)) < 2).tolist()
        pend, pin, sign, magt = False, [], [], []
        for a, b in zip(okm, oks):              # the automaton, never stopping: the kernel's lanes walk a whole generation
            pin.append(pend)
            ts, tm = pend and b, (not pend) and a
            sign.append(ts)
            magt.append(tm)
            pend = (pend and not ts) or tm
        done = np.cumsum(sign)
        if done[-1] >= degree:
            break
        n *= 2
    end = int(np.searchsorted(done, degree))    # index of the output that completes the row
    used = end + 1
    gens = end // GEN + 1
    ev = set()
    if used > AVAILABLE:
        ev.add("runs_out")
        if used == AVAILABLE + 1:
            ev.add("one_short")
    else:
        if gens in (1, 2, 3, 16):
            ev.add(f"gens{gens}")
        if used == AVAILABLE:
            ev.add("exact_9984")
        if end % GEN == GEN - 1:
            ev.add("end_last")
        if end % GEN == 0:
            ev.add("end_first")
        if (end % GEN) % PER_LANE < PER_LANE - 1 and any(sign[end + 1:gens * GEN]):
            ev.add("end_mid_lane")
    G = min(gens, MAX_GENERATIONS)
    last = min(end, AVAILABLE - 1)

    def lanes(flags):
        a = np.zeros((G, 64 * PER_LANE), dtype=bool)
        a[:, :GEN] = np.array(flags[:G * GEN], dtype=bool).reshape(G, GEN)
        return a.reshape(G, 64, PER_LANE)
    P, S, M = lanes(pin), lanes(sign), lanes(magt)
    base = GEN * np.arange(G)[:, None] + PER_LANE * np.arange(64)[None, :]
    live = (base <= last) & (np.arange(64)[None, :] <= 62)
    passes = live & P[:, :, 0] & ~S.any(axis=2)
    if passes[:, :62].any():
        ev.add("pass")
    if (passes[:, :61] & passes[:, 1:62]).any():
        ev.add("pass2")
    if passes[:, 62].any():
        ev.add("pass62")
    if (live[:, :62] & ~P[:, :62, 0] & ~M[:, :62].any(axis=2)).any():
        ev.add("nomag")
    carry = live[1:, 0] & P[1:, 0, 0]
    if carry.any():
        ev.add("carry")
    if (carry & passes[1:, 0]).any():
        ev.add("carry_pass0")
    if (carry & passes[1:, 0] & passes[:-1, 62]).any():
        ev.add("chain")
    return ev


# ---- MT19937 seeding, for the faults that change the key --------------------------------------------------------------------------
def init_by_array(key):
    """Modules/_randommodule.c init_by_array -> the 624 state words"""
    mt = [19650218]
    for i in range(1, GEN):
        mt.append((1812433253 * (mt[-1] ^ (mt[-1] >> 30)) + i) & SENT)
    i, j = 1, 0
    for _ in range(max(GEN, len(key))):
        mt[i] = ((mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1664525)) + key[j] + j) & SENT
        i, j = i + 1, (j + 1) % len(key)
        if i >= GEN:
            mt[0], i = mt[GEN - 1], 1
    for _ in range(GEN - 1):
        mt[i] = ((mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1566083941)) - i) & SENT
        i += 1
        if i >= GEN:
            mt[0], i = mt[GEN - 1], 1
    mt[0] = 0x80000000
    return mt


def stream_of_key(key, n):
    """the first n outputs of the generator that init_by_array(key) seeds (CPython does the regeneration and tempering)"""
    rng = random.Random()
    rng.setstate((3, tuple(init_by_array(key)) + (GEN,), None))
    return np.frombuffer(rng.getrandbits(32 * n).to_bytes(4 * n, "little"), dtype="<u4")


def key_words(seed, fault=None):
    """the kernels' key: one word below 2^32, else two (seeds are below 2^64)"""
    key0, key1 = seed & SENT, seed >> 32
    two = (key0 != 0) if fault == "key_word" else (key1 != 0)
    return [key0, key1] if two else [key0]


# ---- mt_draw_kernel, restated -----------------------------------------------------------------------------------------------------
def _i32(x):
    x &= SENT
    return x - 2 ** 32 if x >= 2 ** 31 else x


def mech_draw(y, degree, bound, fault=None):
    """y: at least 17 generations of outputs -> (writes as a list of (index, value) in program order per lane, fail)"""
    kbits = (bound - 1).bit_length() if fault == "kbits_minus" else bound.bit_length()
    shift = 32 - kbits
    limit = {"limit15": 15, "limit17": 17}.get(fault, MAX_GENERATIONS)
    real_to = {"pad_real": 64 * PER_LANE, "lane62_full": 63 * PER_LANE}.get(fault, GEN)
    ys = [int(w) for w in y[:GEN * limit]]
    writes = []
    t, carry_mag = 0, 0

    def compose(p, a):
        """the lanes of p first, then the lanes of a"""
        p_em, p_cm, p_es, p_cs = p
        a_em, a_cm, a_es, a_cs = a
        a_cs_r = a_cm if fault == "cm_for_cs" else a_cs
        n_em = a_em if p_em == 0 else (p_em if a_es == SENT and fault != "sentinel_em" else a_es)
        n_cm = p_cm + (a_cm if p_em == 0 else a_cs_r)
        n_es = a_es if p_es == SENT else (a_em if p_es == 0 else (p_es if a_es == SENT and fault != "sentinel_es" else a_es))
        n_cs = p_cs + (a_cm if p_es == 0 else a_cs_r)
        return (n_em, n_cm, n_es, n_cs)

    def apply(s):
        s_em, s_cm, s_es, s_cs = s
        if carry_mag == 0:
            return s_em, t + s_cm
        return (carry_mag if s_es == SENT and fault != "sentinel_apply" else s_es), t + (s_cm if fault == "cm_for_cs" else s_cs)

    for gen in range(limit):
        g = ys[GEN * gen:GEN * gen + GEN]
        v, sg = [], []
        for lane in range(64):
            lv, ls = [], []
            for u in range(PER_LANE):
                i = lane * PER_LANE + u
                w = g[min(i, GEN - 1)]
                lv.append((w >> shift) if i < real_to else SENT)
                ls.append(((w & 3) if fault == "sign_low" else (w >> 30)) if i < real_to else 3)
            v.append(lv)
            sg.append(ls)

        def walk(lane, mag):
            cnt = 0
            for u in range(PER_LANE):
                take_sign = mag != 0 and sg[lane][u] < 2
                take_mag = mag == 0 and v[lane][u] < bound
                cnt += take_sign
                mag = 0 if take_sign else (v[lane][u] + 1 if take_mag else mag)
            return mag, cnt
        acc = []
        for lane in range(64):
            em, cm = walk(lane, 0)
            es, cs = walk(lane, SENT)
            acc.append((em, cm, es, cs))
        off = 1
        while off < 64:                         # inclusive scan: six shuffle steps
            prev = list(acc)
            for lane in range(off, 64):
                acc[lane] = compose(acc[lane], prev[lane - off]) if fault == "compose_order" else compose(prev[lane - off], acc[lane])
            off <<= 1
        next_mag, next_t = apply(acc[63])
        for lane in range(64):
            mag, tl = (carry_mag, t) if lane == 0 else apply(acc[lane - 1])      # exclusive: the lanes before this one
            for u in range(PER_LANE):
                take_sign = mag != 0 and sg[lane][u] < 2
                take_mag = mag == 0 and v[lane][u] < bound
                if take_sign:
                    if tl < degree or fault == "no_guard":
                        writes.append((tl, _i32(-mag) if sg[lane][u] else _i32(mag)))
                    tl += 1
                mag = 0 if take_sign else (v[lane][u] + 1 if take_mag else mag)
        carry_mag, t = (0 if fault == "drop_carry" else next_mag), next_t
        if t >= degree:
            return writes, False
    return writes, True


def mech_batch(key_seeds, degree, bound, fault=None):
    """fz_sample_secret_polys_dev's two-kernel form on a poisoned buffer [1 + 2 N + 1][degree] (a guard row in front and one
    behind) -> (buffer int64, fail, words that would have been written past the buffer)"""
    npoly = 2 * len(key_seeds)
    buf = np.full((npoly + 2) * degree, POISON, dtype=np.int64)
    fail, beyond = False, 0
    for p in range(npoly):
        half = p & 1
        seed = key_seeds[p >> 1] + ((1 - half) if fault == "swap_halves" else half)
        key = key_words(seed, fault)
        y = stream_of_key(key, GEN * (MAX_GENERATIONS + 1)) if fault == "key_word" else stream(seed, GEN * (MAX_GENERATIONS + 1))
        writes, f = mech_draw(y, degree, bound, fault)
        fail |= f
        for tl, val in writes:
            at = (1 + p) * degree + tl
            if at < buf.size:
                buf[at] = val
            else:
                beyond += 1
    return buf.reshape(npoly + 2, degree), fail, beyond


def mech_row(s, degree, bound, fault=None):
    """one polynomial (generator seed s) through mech_draw -> (row [degree] with POISON where nothing was written, fail, number
    of writes outside the row)"""
    writes, fail = mech_draw(stream(s, GEN * (MAX_GENERATIONS + 1)), degree, bound, fault)
    row = np.full(degree, POISON, dtype=np.int64)
    outside = 0
    for tl, val in writes:
        if tl < degree:
            row[tl] = val
        else:
            outside += 1
    return row, fail, outside


# ---- the search ---------------------------------------------------------------------------------------------------------------
I31 = 2 ** 31 - 1
SEARCH_TABLE = (
    # (degree, bound, seed ranges (first, count))
    (256, 52, ((0, 100000), (2 ** 32 - 2000, 4000), (2 ** 40, 4000))),       # the scheme's set at secpar 256 (chain: 3 in 100 000)
    (64, 52, ((0, 4000), (2 ** 32 - 200, 400))),                             # ... and at secpar 128
    (256, 64, ((0, 40000),)),
    (2400, 64, ((0, 4000),)),
    (2496, 64, ((0, 1500), (2 ** 32 - 300, 600), (2 ** 50, 600))),           # 9984 outputs expected: half the seeds run out
    (400, 64, ((0, 1500), (2 ** 32 - 100, 200))),                            # three generations
    (156, 64, ((0, 3000),)),                                                 # 624 outputs expected: rows end near a generation's edge
    (1, 1, ((0, 200),)),
    (2, I31, ((0, 200),)),
    (700, 3, ((0, 600),)),
)


def search(table=SEARCH_TABLE, per_event=6, out=sys.stdout):
    """prints, per (degree, bound), the first seeds that show each event (and at (2496, 64) whether both neighbours fit, so that
    the seed can be either half of a key that does not run out)"""
    import time
    for degree, bound, ranges in table:
        t0 = time.time()
        found = {e: [] for e in EVENTS}
        count = {e: 0 for e in EVENTS}
        n = 0
        for first, cnt in ranges:
            for s in range(first, first + cnt):
                n += 1
                for e in classify(s, degree, bound):
                    count[e] += 1
                    if len([x for x in found[e] if first <= x < first + cnt]) < per_event:
                        found[e].append(s)
        print(f"({degree}, {bound}): {n} seeds, {time.time() - t0:.0f} s", file=out)
        for e in EVENTS:
            note = ""
            if degree * 4 >= AVAILABLE - 400 and found[e]:
                note = "   neighbours fit (s - 1, s + 1): " + str([(not runs_out(s - 1, degree, bound) if s else None,
                                                                     not runs_out(s + 1, degree, bound)) for s in found[e]])
            print(f"  {e:13s} {count[e]:6d}  {found[e]}{note}", file=out)
        out.flush()


# ---- the fixtures: (degree, bound, key seed, half, events) ----------------------------------------------------------------------
# The polynomial that shows the events is the key's half `half`: its generator seed is key_seed + half.  A fixture is labelled
# with the events it is there for (it shows others too); tests/test_sampler_edges_host.py checks that it shows them, and that
# no family can be dropped.
FIXTURES = {
    "pass": [(256, 52, 16, 0, ("pass",)), (64, 52, 125, 1, ("pass",)), (256, 52, 4294965306, 0, ("pass",)),
             (256, 52, 1099511627810, 1, ("pass",)), (64, 52, 277, 0, ("pass",)), (64, 52, 4294967185, 1, ("pass",))],
    "pass2": [(256, 52, 26814, 0, ("pass2",)), (256, 52, 26886, 1, ("pass2",)), (2400, 64, 1347, 0, ("pass2",)),
              (256, 64, 32452, 1, ("pass2",))],
    "pass62": [(256, 52, 12, 0, ("pass62",)), (256, 52, 18, 1, ("pass62",)), (700, 3, 10, 0, ("pass62",)),
               (156, 64, 119, 1, ("pass62",))],
    "carry": [(256, 52, 0, 0, ("carry",)), (256, 52, 2, 1, ("carry",)), (700, 3, 0, 0, ("carry",)),
              (256, 52, 1099511627776, 0, ("carry",))],
    "carry_pass0": [(256, 52, 4577, 0, ("carry_pass0",)), (256, 52, 7550, 1, ("carry_pass0",)), (2400, 64, 71, 0, ("carry_pass0",)),
                    (400, 64, 4294967258, 1, ("carry_pass0",)), (156, 64, 910, 0, ("carry_pass0",)), (700, 3, 70, 1, ("carry_pass0",))],
    "chain": [(256, 52, 63744, 0, ("chain",)), (256, 52, 73864, 1, ("chain",)), (256, 64, 15733, 0, ("chain",)),
              (2400, 64, 306, 1, ("chain",))],
    "nomag": [(256, 64, 15, 0, ("nomag",)), (256, 64, 33, 1, ("nomag",)), (1, 1, 95, 0, ("nomag",)), (1, 1, 94, 1, ("nomag",))],
    "end_last": [(156, 64, 68, 0, ("end_last",)), (156, 64, 77, 1, ("end_last",))],
    "end_first": [(156, 64, 82, 0, ("end_first",)), (156, 64, 118, 1, ("end_first",)), (2400, 64, 2922, 0, ("end_first",))],
    "end_mid_lane": [(256, 52, 3, 0, ("end_mid_lane",)), (64, 52, 0, 0, ("end_mid_lane",)), (64, 52, 0, 1, ("end_mid_lane",)),
                     (2, I31, 0, 0, ("end_mid_lane",)), (2, I31, 0, 1, ("end_mid_lane",)), (1, 1, 0, 0, ("end_mid_lane",)),
                     (1, 1, 0, 1, ("end_mid_lane",)), (700, 3, 1, 0, ("end_mid_lane",))],
    # the key 2^32 - 1: its left half is the last one-word key, its right half (2^32) the first two-word key
    "gens1": [(64, 52, 2 ** 32 - 1, 0, ("gens1",)), (64, 52, 2 ** 32 - 1, 1, ("gens1",)), (156, 64, 4, 0, ("gens1",)),
              (2, I31, 2, 1, ("gens1",)), (1, 1, 5, 0, ("gens1",))],
    "gens2": [(256, 52, 2 ** 32 - 1, 0, ("gens2",)), (256, 52, 2 ** 32 - 1, 1, ("gens2",)), (156, 64, 0, 0, ("gens2",))],
    "gens3": [(400, 64, 0, 0, ("gens3",)), (400, 64, 0, 1, ("gens3",)), (400, 64, 2 ** 32 - 1, 0, ("gens3",)),
              (400, 64, 2 ** 32 - 1, 1, ("gens3",))],
    # at (2496, 64) half of all seeds run out: these keys are chosen so that the OTHER half of the key fits
    "gens16": [(2496, 64, 2, 0, ("gens16",)), (2496, 64, 2, 1, ("gens16",)), (2496, 64, 8, 0, ("gens16",)),
               (2400, 64, 0, 0, ("gens16",)), (2400, 64, 0, 1, ("gens16",))],
    "exact_9984": [(2496, 64, 30, 1, ("exact_9984",)), (2496, 64, 893, 0, ("exact_9984",)), (2496, 64, 4294967222, 0, ("exact_9984",)),
                   (2496, 64, 4294967221, 1, ("exact_9984",))],
    "one_short": [(2496, 64, 1409, 0, ("one_short",)), (2496, 64, 1198, 1, ("one_short",)), (2496, 64, 4294967429, 1, ("one_short",))],
    "runs_out": [(2496, 64, 4, 0, ("runs_out",)), (2496, 64, 5, 1, ("runs_out",))],
}
# pass2, carry_pass0 and chain at the scheme's bound of 52: the search above finds all three at (256, 52) (chain after about
# 80 s of one core); (64, 52) rows end in their first generation and show none of the boundary events.


def all_fixtures():
    return [f for fam in FIXTURES.values() for f in fam]


def key_fails(fx):
    """does either half of the fixture's key run out of the 9984 outputs"""
    degree, bound, key_seed = fx[:3]
    return any(runs_out(key_seed + h, degree, bound) for h in (0, 1))


def coverage_gaps(families):
    """what a set of fixture families fails to cover: every event in at least two fixtures and in both halves; one-word and
    two-word key seeds and the crossing from 2^32 - 1 to 2^32; every (degree, bound) of the scheme"""
    fx = [f for fam in families.values() for f in fam]
    gaps = []
    for e in EVENTS:
        hit = [f for f in fx if e in f[4]]
        if len(hit) < 2:
            gaps.append(f"{e}: {len(hit)} fixtures")
        for h in (0, 1):
            if not any(f[3] == h for f in hit):
                gaps.append(f"{e}: no fixture in half {h}")
    seeds = [f[2] for f in fx]
    if not any(s + 1 < 2 ** 32 for s in seeds):
        gaps.append("no one-word key seed")
    if not any(s >= 2 ** 32 for s in seeds):
        gaps.append("no two-word key seed")
    if 2 ** 32 - 1 not in seeds:
        gaps.append("no key whose halves are seeded 2^32 - 1 and 2^32")
    for e in ("pass2", "carry_pass0", "chain"):
        if not any(e in f[4] and f[1] == 52 for f in fx):
            gaps.append(f"{e}: not at the scheme's bound")
    return gaps


if __name__ == "__main__":
    if "--search" in sys.argv:
        search()
    else:
        print(__doc__)
