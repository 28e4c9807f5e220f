"""Fixtures that put the generic int64 path (csrc/fz_wide.hip: wmont / wadd / wsub / wcanon / wcent, wide_pw_kernel, wide_ntt_kernel,
wide_matvec_kernel, wide_norm_weight_kernel; fusion_hip/wide.py) on the edges its arithmetic depends on, and two models of it in
plain Python.

- The PLAIN operations (cent, p_add, p_sub, p_mul, p_neg, p_matvec, p_norm_weight, p_forward, p_inverse) are the operations written on
  Python integers; the transforms are oracle.py's py_ntt_forward / py_ntt_inverse (the reference's loops, the scaling factor
  n^(q-2) mod q included).  They call nothing of this project's device code and are the expectation of every test.
- Model restates the kernels' arithmetic step by step, everything mod 2^64 where the C type wraps: make_mod (the Newton inverse with
  its iteration count, r2, half), wmont (lo, hi, k, the carry, the conditional subtraction), wadd, wsub, wcanon (C's truncating %),
  wcent, the pointwise product's second wmont by r2, the table's conversion to Montgomery form with its % q, the loop nests in the
  kernel's b -> (i, jj, j) indexing, matvec's accumulate-then-r2, and the face's choice of the scaling factor.  Every plausible
  fault is a switch (FAULTS).  tests/test_wide_edges_host.py shows that without a fault the model equals the plain operations on every
  case, and that each fault changes a named case's output or is in EQUIVALENT with the argument why nothing can show it.
- product_events / add_events / sub_events name what an operand pair does under a modulus (the model labels them); fixtures(q)
  holds, per event, pairs made by a constructive recipe or a bounded search (recipes below; CANNOT says which moduli cannot show
  an event, or where the bounded search finds none, and why).  cases(q) pushes every fixture through every kernel that has the
  step: the four pointwise operations, a length-2 forward and inverse transform with the pair as (value, table entry), a matvec
  with l = 1 and l = 2, and the first, middle and last element of a row of 5.

A table entry reaches wmont in Montgomery form (t * 2^64 mod q), so "pair (a, b) as (value, table entry)" means the entry
b * 2^-64 mod q: its Montgomery form is b and the butterfly's wmont sees exactly (a, b)."""
import functools
import random

from oracle import oracle as O

M64 = 1 << 64
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
OP_MUL, OP_ADD, OP_SUB, OP_NEG = 0, 1, 2, 3


def is_prime(n):
    """deterministic Miller-Rabin for n < 2^64"""
    if n < 2:
        return False
    for p in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if n % p == 0:
            return n == p
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def prime_near(start, step, down=False):
    """the first prime q = 1 (mod step) at or after `start` (down: at or before)"""
    q = start - (start - 1) % step if down else start + (1 - start) % step
    while not is_prime(q):
        q += -step if down else step
    return q


Q33 = prime_near(2 ** 32, 2 ** 15)               # just above 2^32, has 2^15-th roots of unity
Q62 = prime_near(2 ** 62, 2 ** 15, down=True)    # just below 2^62
Q63 = prime_near(2 ** 63 - 1, 2 ** 15, down=True)   # the largest prime = 1 (mod 2^15) the path takes

PRIMES = {"q3": 3, "q5": 5, "q7": 7, "q65537": 65537, "scheme": 2147465729, "2^32-5": 2 ** 32 - 5, "2^32+15": 2 ** 32 + 15, "Q33": Q33,
          "Q62": Q62, "Q63": Q63, "2^63-25": 2 ** 63 - 25}
COMPOSITES = {"2^32-1": 2 ** 32 - 1, "2^32+1": 2 ** 32 + 1, "3*2^50+1": 3 * 2 ** 50 + 1, "2^63-1": 2 ** 63 - 1}
SMALL_FACTOR = {2 ** 32 - 1: 3, 2 ** 32 + 1: 641, 3 * 2 ** 50 + 1: 13, 2 ** 63 - 1: 7}
MODULI = dict(sorted({**PRIMES, **COMPOSITES}.items(), key=lambda kv: kv[1]))
NAME_OF = {q: n for n, q in MODULI.items()}
NARROW = tuple(q for q in MODULI.values() if q < 2 ** 32)


# ---- the plain operations -------------------------------------------------------------------------------------------------------
def cent(x, q):
    y = x % q
    return y - q if y > (q - 1) // 2 else y


def p_add(a, b, q):
    return [cent(x + y, q) for x, y in zip(a, b)]


def p_sub(a, b, q):
    return [cent(x - y, q) for x, y in zip(a, b)]


def p_mul(a, b, q):
    return [cent(x * y, q) for x, y in zip(a, b)]


def p_neg(a, q):
    return [-(x % q) for x in a]


def p_pw(op, a, b, q):
    return p_neg(a, q) if op == OP_NEG else (p_mul, p_add, p_sub)[op](a, b, q)


def p_matvec(A, S, q):
    """A [l][d], S [batch][l][d] -> [batch][d]"""
    return [[cent(sum(A[k][j] * Sb[k][j] for k in range(len(A))), q) for j in range(len(A[0]))] for Sb in S]


def p_norm_weight(row):
    return max(abs(x) for x in row), sum(1 for x in row if x != 0)


def p_forward(row, q, table):
    return O.py_ntt_forward(list(row), q, list(table))


def p_inverse(row, q, table):
    return O.py_ntt_inverse(list(row), q, list(table))


def scaling_factor(n, q):
    """the library's scaling factor of the inverse transform: the reference's expression (ntt.py:353)"""
    return pow(n, q - 2, q)


# ---- the step-by-step model -----------------------------------------------------------------------------------------------------
FAULTS = ("carry_always_1", "carry_always_0", "carry_if_operands_nonzero", "u_gt_q", "wadd_gt", "wsub_gt", "canon_no_sign_fix", "canon_unsigned",
          "wcent_ge", "half_plus_1", "neg_centred", "mul_no_r2", "r2_single", "newton_4", "table_not_reduced", "n_inv_not_reduced",
          "n_inv_modular_inverse", "fwd_twiddle_i", "inv_twiddle_mm", "scale_forward", "matvec_no_r2")

# faults that no input can show, with the argument (the host test checks that the model agrees on every case)
EQUIVALENT = {
    "u_gt_q": "u == q is then returned as q instead of 0: a residue stored as q.  Every consumer absorbs it: wadd(x, q) = x (x + q >= q) "
              "and wadd(q, q) = q; wsub(x, q) = x + q - q = x, wsub(q, x) = q - x, the right residue in (0, q]; a later wmont with an "
              "operand q gives u = q (r + k') / 2^64 in {0, q}, i.e. 0 or q again (q * q < 2^126 does not overflow the two words); "
              "and the last step of every kernel is wcent, where q > half gives q - q = 0",
    "wadd_gt": "a + b == q is then returned as q instead of 0: the same stored q, absorbed in the same way (see u_gt_q); matvec's "
               "final wmont(q, r2) is 0 or q, and wcent(q) = 0",
    "wsub_gt": "a == b then gives a + q - b = q instead of 0: the same stored q, absorbed in the same way (see u_gt_q)",
    "table_not_reduced": "the conversion is (h << 64) % q in 128-bit arithmetic: h < 2^64 so h << 64 < 2^128 does not overflow, and "
                         "((h % q) << 64) % q == (h << 64) % q exactly.  The % q is redundant, not wrong; the GPU file still pins "
                         "unreduced tables against reduced ones through the C ABI",
    "n_inv_not_reduced": "the same 128-bit argument as table_not_reduced",
}


def to_signed(v):
    v %= M64
    return v - M64 if v >= 1 << 63 else v


class Model:
    """csrc/fz_wide.hip on Python integers; `faults`: names from FAULTS; `trace`: a list that receives every wmont's (a, b, lo, hi, k, u)"""

    def __init__(self, q, faults=(), trace=None):
        self.f = frozenset(faults)
        assert self.f <= set(FAULTS), self.f - set(FAULTS)
        self.trace = trace
        assert 3 <= q < 1 << 63 and q % 2 == 1
        inv = q                                            # make_mod: Newton, correct to 3 bits at the start
        for _ in range(4 if "newton_4" in self.f else 6):
            inv = inv * ((2 - q * inv) % M64) % M64
        self.q, self.qneg_inv = q, (-inv) % M64
        r = M64 % q
        self.r2 = r if "r2_single" in self.f else r * r % q
        self.half = q // 2 + 1 if "half_plus_1" in self.f else (q - 1) // 2

    def wmont(self, a, b):
        q = self.q
        p = a * b
        lo, hi = p % M64, p >> 64
        assert hi < M64
        k = lo * self.qneg_inv % M64
        carry = int(lo != 0)
        if "carry_always_1" in self.f:
            carry = 1
        if "carry_always_0" in self.f:
            carry = 0
        if "carry_if_operands_nonzero" in self.f:
            carry = int(a != 0 and b != 0)
        u = (hi + (k * q >> 64) + carry) % M64
        if self.trace is not None:
            self.trace.append((a, b, lo, hi, k, u))
        return (u - q) % M64 if (u > q if "u_gt_q" in self.f else u >= q) else u

    def wadd(self, a, b):
        s = (a + b) % M64
        return (s - self.q) % M64 if (s > self.q if "wadd_gt" in self.f else s >= self.q) else s

    def wsub(self, a, b):
        return (a - b) % M64 if (a > b if "wsub_gt" in self.f else a >= b) else (a + self.q - b) % M64

    def wcanon(self, x):
        assert INT64_MIN <= x <= INT64_MAX
        if "canon_unsigned" in self.f:
            return (x % M64) % self.q
        r = abs(x) % self.q                                # C's %: truncating, the sign of the dividend
        if x < 0:
            r = -r
        if r < 0 and "canon_no_sign_fix" not in self.f:
            r += self.q
        return r % M64

    def wcent(self, v):
        return to_signed(v - self.q) if (v >= self.half if "wcent_ge" in self.f else v > self.half) else to_signed(v)

    def pw(self, op, a, b):
        out = []
        for i, xv in enumerate(a):
            x = self.wcanon(xv)
            if op == OP_NEG:
                out.append(self.wcent(self.wsub(0, x)) if "neg_centred" in self.f else to_signed(-x))
                continue
            y = self.wcanon(b[i])
            if op == OP_ADD:
                r = self.wadd(x, y)
            elif op == OP_SUB:
                r = self.wsub(x, y)
            else:
                r = self.wmont(x, y)
                if "mul_no_r2" not in self.f:
                    r = self.wmont(r, self.r2)
            out.append(self.wcent(r))
        return out

    def mont_form(self, h, fault):
        """the host's conversion of a table entry or of n_inv: ((h % q) << 64) % q in 128-bit arithmetic"""
        assert 0 <= h < M64
        h = h if fault in self.f else h % self.q
        assert h << 64 < 1 << 128
        return (h << 64) % self.q

    def face_n_inv(self, n):
        """what WideContext hands over as n_inv"""
        return pow(n, -1, self.q) if "n_inv_modular_inverse" in self.f else pow(n, self.q - 2, self.q)

    def ntt(self, row, table, inverse, n_inv=None):
        """one row through wide_ntt_kernel; table: the caller's `n` entries (any uint64); n_inv: the C ABI's argument (default: the face's)"""
        n = len(row)
        assert n >= 2 and n & (n - 1) == 0 and len(table) == n
        tab = [self.mont_form(h, "table_not_reduced") for h in table] + [0] * n      # (a faulty index past the table reads 0 here)
        n_inv_mont = self.mont_form(self.face_n_inv(n) if n_inv is None else n_inv, "n_inv_not_reduced")
        v = [self.wcanon(x) for x in row]
        half = n // 2
        if not inverse:
            mm, t = 1, half
            while mm < n:
                for b in range(half):
                    i, jj = divmod(b, t)
                    j = 2 * i * t + jj
                    U, V = v[j], self.wmont(v[j + t], tab[i if "fwd_twiddle_i" in self.f else mm + i])
                    v[j], v[j + t] = self.wadd(U, V), self.wsub(U, V)
                mm, t = mm * 2, t // 2
        else:
            mm, t = n, 1
            while mm > 1:
                h = mm // 2
                for b in range(half):
                    i, jj = divmod(b, t)
                    j = 2 * i * t + jj
                    U, V = v[j], v[j + t]
                    v[j], v[j + t] = self.wadd(U, V), self.wmont(self.wsub(U, V), tab[mm + i if "inv_twiddle_mm" in self.f else h + i])
                mm, t = mm // 2, t * 2
        if inverse or "scale_forward" in self.f:
            v = [self.wmont(x, n_inv_mont) for x in v]
        return [self.wcent(x) for x in v]

    def matvec(self, A, S):
        l, d = len(A), len(A[0])
        out = []
        for Sb in S:
            row = []
            for j in range(d):
                acc = 0
                for k in range(l):
                    acc = self.wadd(acc, self.wmont(self.wcanon(A[k][j]), self.wcanon(Sb[k][j])))
                row.append(self.wcent(acc if "matvec_no_r2" in self.f else self.wmont(acc, self.r2)))
            out.append(row)
        return out


# ---- events ---------------------------------------------------------------------------------------------------------------------
PRODUCT_EVENTS = ("lo0_nonzero", "lo_eq_q", "u_eq_q", "sub_taken", "sub_not_taken_u_qm1", "hi_max", "zero_operand", "operand_1")
ADD_EVENTS = ("sum_eq_q", "sum_eq_qm1", "sum_eq_2qm2")
SUB_EVENTS = ("a_eq_b", "zero_minus_1", "zero_minus_qm1", "a_eq_bm1")
CENT_EVENTS = ("cent_half", "cent_half_p1", "cent_qm1", "cent_0")
NEG_EVENTS = ("neg_0", "neg_1", "neg_qm1")


def product_events(a, b, q):
    """the events of wmont(a, b) for residues a, b in [0, q), read off the model's own trace"""
    tr = []
    Model(q, trace=tr).wmont(a, b)
    _, _, lo, hi, k, u = tr[0]
    ev = set()
    if lo == 0 and a * b != 0:
        assert hi != 0
        ev.add("lo0_nonzero")
    if lo == q:
        assert k == M64 - 1
        ev.add("lo_eq_q")
    if u == q:
        ev.add("u_eq_q")
    if u > q and lo != q:                                  # (lo == q always subtracts, u = hi + q: its own event)
        ev.add("sub_taken")
    if u == q - 1:
        ev.add("sub_not_taken_u_qm1")
    if a == b == q - 1:
        ev.add("hi_max")
    if a == 0 or b == 0:
        ev.add("zero_operand")
    elif a == 1 or b == 1:
        ev.add("operand_1")
    return ev


def add_events(a, b, q):
    return {n for n, s in (("sum_eq_q", q), ("sum_eq_qm1", q - 1), ("sum_eq_2qm2", 2 * q - 2)) if a + b == s}


def sub_events(a, b, q):
    ev = set()
    if a == b:
        ev.add("a_eq_b")
    if (a, b) == (0, 1):
        ev.add("zero_minus_1")
    if (a, b) == (0, q - 1):
        ev.add("zero_minus_qm1")
    if a == b - 1 and a > 0:                               # (0 - 1 is its own event)
        ev.add("a_eq_bm1")
    return ev


def events_of(kind, a, b, q):
    return {"product": product_events, "wadd": add_events, "wsub": sub_events}[kind](a, b, q)


# ---- recipes --------------------------------------------------------------------------------------------------------------------
def _take(q, event, candidates, want=2):
    got = []
    for a, b in candidates:
        if 0 <= a < q and 0 <= b < q and (a, b) not in got and event in product_events(a, b, q):
            got.append((a, b))
            if len(got) == want:
                break
    return got


def _split_candidates(q, multiples, wraps):
    """factor pairs (a, b), both below q, of c q + t 2^64 (so that lo = c q mod 2^64, k = 2^64 - c): by small divisors, then pairs
    just below q -- a bounded search"""
    for c in multiples:
        for t in wraps:
            N = c * q + (t << 64)
            for s in range(2, 4096):
                if N % s == 0 and N // s < q:
                    yield s, N // s
                    yield N // s, s
    for i in range(1, 48):
        for j in range(1, 48):
            yield q - i, q - j
    if q >= 1 << 40:                                       # a = c q / b (mod 2^64) is below q for about one odd b in 2^64 / q
        for b in range(3, 1 << 16, 2):
            for c in multiples:
                yield c * q * pow(b, -1, M64) % M64, b


def product_fixtures(q):
    """event -> list of (a, b), residues in [0, q)"""
    R = M64 % q
    fx = {}
    e = (q - 1).bit_length() - 1                           # 2^e: the largest power of two below q
    odd = (1, 3, 5, 7)
    fx["lo0_nonzero"] = _take(q, "lo0_nonzero", [(c << ee, d << (64 - ee)) for ee in range(e, 31, -1) for c in odd for d in odd])
    # lo == q: a b = q + t 2^64; t = 0, a factor pair of a composite q (which is u_eq_q as well), only where no other is found
    fx["lo_eq_q"] = _take(q, "lo_eq_q", _split_candidates(q, (1,), list(range(1, 65)) + [0]))
    f = SMALL_FACTOR.get(q)
    fx["u_eq_q"] = _take(q, "u_eq_q", [(f, q // f), (2 * f, q // f), (q // f, 3 * f)]) if f else []
    # u > q: lo = c q mod 2^64 gives k = 2^64 - c and u = q + (a b - c q) / 2^64: any such pair with a b > c q
    fx["sub_taken"] = _take(q, "sub_taken", _split_candidates(q, range(2, 10), range(1, 33)))
    fx["sub_not_taken_u_qm1"] = _take(q, "sub_not_taken_u_qm1", [(q - 1, R), (2, (q - R) * pow(2, -1, q) % q), (q - 2, R * pow(2, -1, q) % q), (1, q - R)])   # a b = -2^64 (mod q)
    fx["hi_max"] = [(q - 1, q - 1)]
    fx["zero_operand"] = [(0, q - 1), (q - 2, 0), (0, 0)]
    fx["operand_1"] = _take(q, "operand_1", [(1, q - 1), (q - 2, 1), (1, 1), (1, 2)])
    return fx


def add_fixtures(q):
    h = (q - 1) // 2
    return {"sum_eq_q": [(1, q - 1), (h + 1, h)], "sum_eq_qm1": [(0, q - 1), (h, h)], "sum_eq_2qm2": [(q - 1, q - 1)]}


def sub_fixtures(q):
    return {"a_eq_b": [(0, 0), (q - 1, q - 1)], "zero_minus_1": [(0, 1)], "zero_minus_qm1": [(0, q - 1)], "a_eq_bm1": [(q - 2, q - 1), (1, 2)]}


def canon_values(q):
    """name -> int64 for wcanon; at q = 2^63 - 1 INT64_MAX is q (-> 0) and INT64_MIN is -q - 1 (-> q - 1)"""
    top, bot = INT64_MAX // q * q, -((1 << 63) // q * q)
    v = {"0": 0, "+1": 1, "-1": -1, "+q": q, "-q": -q, "+(q+1)": q + 1, "-(q+1)": -(q + 1), "+(q-1)": q - 1, "-(q-1)": -(q - 1), "INT64_MIN": INT64_MIN,
         "INT64_MAX": INT64_MAX, "top": top, "top-1": top - 1, "top+1": top + 1, "bot": bot, "bot+1": bot + 1, "bot-1": bot - 1}
    return {n: x for n, x in v.items() if INT64_MIN <= x <= INT64_MAX}


def cent_values(q):
    """name -> residue v in [0, q) whose wcent is the event (reached as v + 0)"""
    h = (q - 1) // 2
    return {"cent_half": h, "cent_half_p1": h + 1, "cent_qm1": q - 1, "cent_0": 0}


def neg_values(q):
    return {"neg_0": 0, "neg_1": 1, "neg_qm1": q - 1}


@functools.lru_cache(maxsize=None)
def fixtures(q):
    """kind -> event -> list of pairs"""
    fx = {"product": product_fixtures(q), "wadd": add_fixtures(q), "wsub": sub_fixtures(q)}
    return {kind: {e: list(dict.fromkeys(pairs)) for e, pairs in by.items()} for kind, by in fx.items()}     # (recipes coincide at q = 3)


# (event, reason, predicate on q): the moduli at which FIXTURES holds fewer than two pairs (none, unless `one` says one), and why
CANNOT = (
    ("lo0_nonzero", "a b = 0 (mod 2^64) with a b != 0 needs a b >= 2^64, i.e. q > 2^32", lambda q: q <= 2 ** 32, 0),
    ("lo0_nonzero", "at q = 2^32 + 1, 2^32 + 15 and Q33 the only operand below q with 32 factors of two is 2^32: one pair, (2^32, 2^32)",
     lambda q: q in (2 ** 32 + 1, 2 ** 32 + 15, Q33), 1),
    ("lo_eq_q", "a b < 2^64 for q <= 2^32, so lo = a b = q needs a factor pair: no prime q <= 2^32 has one", lambda q: q < 2 ** 32 and is_prime(q), 0),
    ("lo_eq_q", "a b = q + t 2^64 with both factors below q ~ 2^32 leaves a window of q - 2^64 / q operands either side; about "
                "(window)^2 / 2^64 pairs are expected (2^-54 at 2^32 + 15, 2^-25 at Q33) and the bounded search finds none",
     lambda q: q in (2 ** 32 + 15, Q33), 0),
    ("u_eq_q", "u == q means a b = 0 (mod q) with a, b != 0: zero divisors, composite moduli only", is_prime, 0),
    ("sub_taken", "u < q + q^2 / 2^64: below 2^32 u <= q, and u == q is u_eq_q, so the strict u > q cannot occur", lambda q: q < 2 ** 32, 0),
    ("sub_taken", "u > q needs k q within (1 + hi) 2^64 of q 2^64 with hi <= 1: about one pair in 2^32 at q ~ 2^32, and the bounded "
                  "search (factor pairs of c q + t 2^64 by small divisors, pairs just below q) finds none",
     lambda q: q in (2 ** 32 + 1, 2 ** 32 + 15, Q33), 0),
)


def expected_count(event, q):
    """how many pairs fixtures(q) must hold for a product event: 2 (hi_max is one pair, a zero operand three), or what CANNOT says"""
    for ev, _, pred, n in CANNOT:
        if ev == event and pred(q):
            return n
    return {"hi_max": 1, "zero_operand": 3}.get(event, 2)


# ---- cases: every fixture through every kernel that has the step ----------------------------------------------------------------
class Case:
    """one call: entry 'pw' (op, a, b), 'ntt' (inverse, table, rows) or 'matvec' (A, S); family: the fixture family it carries"""

    def __init__(self, name, family, entry, **kw):
        self.name, self.family, self.entry = name, family, entry
        self.__dict__.update(kw)

    def plain(self, q):
        if self.entry == "pw":
            return p_pw(self.op, self.a, self.b, q)
        if self.entry == "ntt":
            return [(p_inverse if self.inverse else p_forward)(r, q, self.table) for r in self.rows]
        return p_matvec(self.A, self.S, q)

    def model(self, m):
        if self.entry == "pw":
            return m.pw(self.op, self.a, self.b)
        if self.entry == "ntt":
            return [m.ntt(r, self.table, self.inverse) for r in self.rows]
        return m.matvec(self.A, self.S)


def _filler(q, n, seed):
    rnd = random.Random(seed)
    return [rnd.randrange(q) for _ in range(n)]


@functools.lru_cache(maxsize=None)
def cases(q):
    """the named cases of modulus q, in a fixed order"""
    qn = NAME_OF[q]
    Rinv = pow(M64, -1, q)
    out = []
    fx = fixtures(q)
    for event, pairs in fx["product"].items():
        for n, (a, b) in enumerate(pairs):
            tag = f"{qn}/{event}#{n}"
            out.append(Case(f"{tag}/mul", event, "pw", op=OP_MUL, a=[a], b=[b]))
            # (value, table entry): the entry whose Montgomery form is b; forward: V = wmont(v[1], tab[1]); inverse: wmont(v[0] - v[1], tab[1])
            out.append(Case(f"{tag}/fwd2", event, "ntt", inverse=0, table=[0, b * Rinv % q], rows=[[0, a], [a, a]]))
            out.append(Case(f"{tag}/inv2", event, "ntt", inverse=1, table=[0, b * Rinv % q], rows=[[a, 0], [0, (q - a) % q]]))
            out.append(Case(f"{tag}/matvec1", event, "matvec", A=[[a]], S=[[[b]]]))
            o, p = _filler(q, 2, a ^ b)
            out.append(Case(f"{tag}/matvec2", event, "matvec", A=[[a], [b]], S=[[[b], [a]], [[o], [p]]]))
            for pos in (0, 2, 4):
                fa, fb = _filler(q, 5, pos + a), _filler(q, 5, pos + b + 1)
                fa[pos], fb[pos] = a, b
                out.append(Case(f"{tag}/mul5@{pos}", event, "pw", op=OP_MUL, a=fa, b=fb))
                out.append(Case(f"{tag}/matvec5@{pos}", event, "matvec", A=[fa], S=[[fb]]))
    for kind, op in (("wadd", OP_ADD), ("wsub", OP_SUB)):
        for event, pairs in fx[kind].items():
            for n, (a, b) in enumerate(pairs):
                tag = f"{qn}/{event}#{n}"
                out.append(Case(f"{tag}/pw", event, "pw", op=op, a=[a], b=[b]))
                # table entry 1: V = b, so the butterfly is (wadd(a, b), wsub(a, b)) in either direction
                out.append(Case(f"{tag}/fwd2", event, "ntt", inverse=0, table=[0, 1], rows=[[a, b]]))
                out.append(Case(f"{tag}/inv2", event, "ntt", inverse=1, table=[0, 1], rows=[[a, b]]))
                if kind == "wadd":                           # matvec's accumulation: wmont(a 2^64, 1) = a, then acc = wadd(a, b)
                    out.append(Case(f"{tag}/matvec2", event, "matvec", A=[[a * M64 % q], [b * M64 % q]], S=[[[1], [1]]]))
                for pos in (0, 2, 4):
                    fa, fb = _filler(q, 5, pos + a), _filler(q, 5, pos + b + 1)
                    fa[pos], fb[pos] = a, b
                    out.append(Case(f"{tag}/pw5@{pos}", event, "pw", op=op, a=fa, b=fb))
    cv = canon_values(q)
    vals = list(cv.values())
    other = [vals[(i + 5) % len(vals)] for i in range(len(vals))]
    for opn, op in (("mul", OP_MUL), ("add", OP_ADD), ("sub", OP_SUB), ("neg", OP_NEG)):
        out.append(Case(f"{qn}/wcanon/{opn}", "wcanon", "pw", op=op, a=vals, b=other))
        out.append(Case(f"{qn}/wcanon/{opn}-swapped", "wcanon", "pw", op=op, a=other, b=vals))
    out.append(Case(f"{qn}/wcanon/add0", "wcanon", "pw", op=OP_ADD, a=vals, b=[0] * len(vals)))
    pad = vals + [0] * (32 - len(vals))
    tab = _filler(q, 32, 32)
    out.append(Case(f"{qn}/wcanon/fwd32", "wcanon", "ntt", inverse=0, table=tab, rows=[pad, pad[::-1]]))
    out.append(Case(f"{qn}/wcanon/inv32", "wcanon", "ntt", inverse=1, table=tab, rows=[pad, pad[::-1]]))
    out.append(Case(f"{qn}/wcanon/matvec", "wcanon", "matvec", A=[vals, other], S=[[other, vals], [vals, vals]]))
    for event, v in cent_values(q).items():
        out.append(Case(f"{qn}/{event}/add0", event, "pw", op=OP_ADD, a=[v], b=[0]))
        out.append(Case(f"{qn}/{event}/sub0", event, "pw", op=OP_SUB, a=[v], b=[0]))
        out.append(Case(f"{qn}/{event}/mul1", event, "pw", op=OP_MUL, a=[v], b=[1]))
        out.append(Case(f"{qn}/{event}/fwd2", event, "ntt", inverse=0, table=[0, 1], rows=[[v, 0]]))
        out.append(Case(f"{qn}/{event}/matvec1", event, "matvec", A=[[v]], S=[[[1]]]))
    for event, v in neg_values(q).items():
        for pos in (0, 2, 4):
            fa = _filler(q, 5, pos + v)
            fa[pos] = v
            out.append(Case(f"{qn}/{event}/neg5@{pos}", event, "pw", op=OP_NEG, a=fa, b=None))
    # longer transforms with random tables (the twiddle-index faults need a stage whose index is not 1) and tables of 0, 1, q - 1
    rnd = random.Random(q % 8191)
    for n in (4, 8, 16):
        tab, rows = [rnd.randrange(q) for _ in range(n)], [[rnd.randrange(q) for _ in range(n)] for _ in range(2)]
        edge = [(0, 1, q - 1)[i % 3] for i in range(n)]
        for inverse, d in ((0, "fwd"), (1, "inv")):
            out.append(Case(f"{qn}/random/{d}{n}", "random", "ntt", inverse=inverse, table=tab, rows=rows))
            out.append(Case(f"{qn}/edge-table/{d}{n}", "edge-table", "ntt", inverse=inverse, table=edge, rows=rows))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def noticed_by(fault, q):
    """names of the cases of modulus q whose output the fault changes in the model"""
    m = Model(q, (fault,))
    return [c.name for c in cases(q) if c.model(m) != c.plain(q)]
