"""Moduli, twiddle tables and rows that drive the transform kernels' twiddle multiplies to the edge of the 4-op form, and an
exact model of the largest operand each inverse schedule hands to a multiply.

fz_make_mod (csrc/fz_arith.h) sets `fast` when delta = K - q < 2^15 and q < 2^31 (K = the smallest power of two >= q); the
4-op fz_mulmod4 is then used for every twiddle multiply of the radix-4 and 16-per-lane kernels.  It computes t = a*w - c*K
with c ~ a*w/q, so |t| ~ |c| * delta: exact while |a| <= 2^38, but once |c| * delta reaches 2^53 an ODD t is rounded.  Hence
the fixtures' operands are odd where they are meant to be large (a sum of 2^k equal int32 values is even, and an even t
stays exact up to 2^54), and the tables hold odd twiddles next to q - 1.

The inverse kernels keep their operands under 2^38 by folding at fixed places (csrc/fz_ntt_dev.h):
- 16-per-lane (inv16_passes: ntt_inv16, ntt_jobs16, polymul16): after the contiguous pass (GS stages of distance 1 ..
  2^(SB-1), SB = log2(D) - 4) the value at positions 0 mod 16 is folded when 31 + SB + 4 > 38, i.e. at degree 256 only;
- radix-4 (inv4_passes_n: ntt_inv4, ntt_jobs4, polymul_fused, verify_fused): after pass 0 (distances 1 and 2) the value at
  positions 0 mod 4 is folded when 31 + log2(D) > 38, i.e. at degree 256 only.
Without a fold the sum of all D inputs reaches the last stage: exactly 2^38 for D = 128 inputs of INT32_MIN, 2^39 at 256.
The transform network is the reference's (algebra/ntt.py gentleman_sande_intt) in every schedule; only the fold sites and
the order differ, so inverse_model below runs the reference's loop on (exact part, reduced-term count) pairs.

tests/test_transform_edges_host.py checks the model against a replay of the butterfly loop and shows with fz_arith.h on the
host that each fixture's (a, w, q) is exact as the kernels use it and inexact past the threshold or a removed fold;
tests/test_gpu_transform_edges.py runs every transform family on these moduli, tables and rows."""
import numpy as np

I32_MIN, I32_MAX = -(2 ** 31), 2 ** 31 - 1
PRIME = 2147465729                         # the scheme's modulus, delta = 17919


def mod_form(q, threshold=32768, below_2_31=True):
    """(K, delta, fast) as fz_make_mod computes them; threshold / below_2_31 describe the rule itself (the host test varies
    them to show what a wider rule would admit)"""
    K = 1
    while K < q:
        K <<= 1
    return K, K - q, (K - q) < threshold and (q < 2 ** 31 or not below_2_31)


def n_inv(q, n):
    return pow(n, q - 2, q)


def cent(v, q):
    r = int(v) % q
    return r - q if r > q // 2 else r


# ---- moduli -----------------------------------------------------------------------------------------------------------------
# table contexts (fz_ctx_create_tables: any odd q, no root needed); name -> q
TABLE_MODULI = {
    "d32767": 2 ** 31 - 32767,             # K = 2^31, the largest fast delta
    "d32769": 2 ** 31 - 32769,             # the first delta that is not fast
    "d65535": 2 ** 31 - 65535,             # delta in [2^15, 2^16), q < 2^31
    "k17": 2 ** 17 - 32767,                # K = 2^17, delta = 2^15 - 1 (fast)
    "f65537": 65537,                       # K = 2^17, delta = 65535 (not fast)
    "m31": 2 ** 31 - 1,                    # fast, delta = 1
    "p31": 2 ** 31 + 1,                    # K = 2^32: not fast
    "w32": 2 ** 32 - 1,                    # delta = 1 but q >= 2^31: not fast
    "w32d32767": 2 ** 32 - 32767,          # delta = 2^15 - 1 but q >= 2^31: not fast
    "q3": 3,                               # K = 4, delta = 1: fast
    "scheme": PRIME,                       # the control
}
# primes with a 512-th root of unity next to the edges (ordinary root contexts, every degree up to 256)
def root_512(q):
    """a primitive 512-th root of unity mod q"""
    for g in range(2, 5000):
        r = pow(g, (q - 1) // 512, q)
        if pow(r, 256, q) == q - 1:
            return r
    raise AssertionError("no root of order 512")


# name -> (q, root of order 512)
ROOT_MODULI = {name: (q, root_512(q)) for name, q in (
    ("r28159", 2147455489),                # the largest fast delta of a K = 2^31 prime = 1 mod 512
    ("r33279", 2147450369),                # the smallest delta above 2^15 of such a prime
    ("r61951", 2147421697),                # the largest delta below 2^16 of such a prime
    ("scheme", PRIME),
)}


def bitrev_powers(r, q, n):
    k = n.bit_length() - 1
    return [pow(r, int(format(i, f"0{k}b")[::-1], 2) if k else 0, q) for i in range(n)]


def root_of(name, n):
    """(q, root, inv_root): a primitive 2n-th root of a ROOT_MODULI prime, as an ordinary root context takes it"""
    q, r512 = ROOT_MODULI[name]
    r = pow(r512, 256 // n, q)
    return q, r, pow(r, q - 2, q)


def root_tables(name, n):
    """bit-reversed powers of root_of's root and of its inverse (algebra/polynomials.py:396-397): the tables such a context
    builds for itself"""
    q, r, ir = root_of(name, n)
    return bitrev_powers(r, q, n), bitrev_powers(ir, q, n)


def top_tables(q, n, kind):
    """"q1": every entry q - 1; "odd": every entry q - 2 (odd, so odd operands give odd products) and the inverse table's
    entry 1 -- the last stage's twiddle, which the kernels fold with n_inv(q, n) -- chosen so that w1 * n_inv = q - 2 as well.
    n_inv is pow(n, q - 2, q) as the reference computes it, which is n^-1 only for prime q; it is a unit for every odd q (a
    power of the unit n), so w1 = (q - 2) / n_inv exists whatever q is."""
    if kind == "q1":
        return [q - 1] * n, [q - 1] * n
    fwd, inv = [q - 2] * n, [q - 2] * n
    if n >= 2:
        inv[1] = (q - 2) * pow(n_inv(q, n), -1, q) % q
    return fwd, inv


def tables(name, n, kind="odd"):
    """(q, fwd, inv) of a fixture modulus at degree n"""
    if kind == "root":
        return (ROOT_MODULI[name][0],) + tuple(root_tables(name, n))
    q = TABLE_MODULI[name]
    return (q,) + tuple(top_tables(q, n, kind))


# ---- rows -------------------------------------------------------------------------------------------------------------------
def _odd(row, n):
    """make the row's sum (and its half-differences) odd: the first entry moves one step towards zero"""
    row = list(row)
    row[0] += 1 if row[0] < 0 else -1
    return row


def rows(q, n):
    """(name, row) in the transform's input order.  The constant rows feed the pure-add path to the last stage's n^-1
    multiply (sum of all n inputs); "stage s" feeds the pure-add path to stage s's multiply: sign + on blocks of 2^s, - on the
    next, so u - v at distance 2^s is 2^(s+1) * 2^31 - O(1) -- the halves pattern (s = log2 n - 1) reaches the last stage's
    w1 * n^-1 multiply with n * 2^31."""
    top = min(q - 1, I32_MAX)
    out = [("min", [I32_MIN] * n), ("max", [I32_MAX] * n), ("q-1", [top] * n), ("-(q-1)", [-top] * n),
           ("min_odd", _odd([I32_MIN] * n, n)), ("max_odd", _odd([I32_MAX] * n, n))]
    for s in range(n.bit_length() - 1):
        out.append((f"stage{s}", _odd([I32_MAX if ((j >> s) & 1) == 0 else I32_MIN for j in range(n)], n)))
        out.append((f"stage{s}-", _odd([I32_MIN if ((j >> s) & 1) == 0 else I32_MAX for j in range(n)], n)))
    return out


def lifted_rows(q, n):
    """rows congruent to the constant c everywhere, every entry but the first lifted by -q (or +q): their inverse is c at
    coefficient 0 and zero elsewhere (norm |c|, weight 1), yet the kernel sums n - 1 lifted values -- an odd sum of about
    n * q (2^39 at degree 256 for q near 2^31).  (q - 1 < 2^31 + c; the +q rows need c + q < 2^31, i.e. c < delta.)"""
    K, delta, _ = mod_form(q)
    out = []
    for c in (1, 12345, (q - 1) // 2):
        if c - q >= I32_MIN:
            out.append((f"lift-{c}", [c] + [c - q] * (n - 1)))
    for c in (1, delta - 1):
        if 0 < c and c + q <= I32_MAX:
            out.append((f"lift+{c}", [c] + [c + q] * (n - 1)))
    return out


def few_rows(q, n):
    """the subset used at degrees 512 .. 4096 (whose reference loops cost more in Python)"""
    k = n.bit_length() - 1
    keep = {"min", "max", "q-1", "min_odd", "max_odd", "stage0", f"stage{k - 1}", f"stage{k - 1}-"}
    return [(nm, r) for nm, r in rows(q, n) if nm in keep]


# ---- the model --------------------------------------------------------------------------------------------------------------
def fold_sites(family, logd, fast):
    """[(after GS stage index, position modulus)]: where the inverse schedule folds (csrc/fz_ntt_dev.h's conditions verbatim);
    stage index i is the GS stage of distance 2^i.  family: "16" (inv16_passes), "4" (inv4_passes_n), "small" / "big" (no
    4-op multiply: ntt_big folds every sum into the 6-op form's range, ntt_small needs none below 2^35)"""
    if family == "16" and 5 <= logd <= 8:
        SB = logd - 4
        return [(SB - 1, 16)] if fast and 31 + SB + 4 > 38 else []
    if family == "4" and logd in (6, 8):
        return [(1, 4)] if fast and 31 + logd > 38 else []
    return []


def reduced_bound(q):
    """|value| bound of a multiply or fold output (fz_mulmod4: q/2 + q * 2^-13; fz_fold and fz_mulmod are tighter)"""
    return q / 2 + q * 2.0 ** -13


def inverse_model(row, q, folds):
    """The largest operand of every multiply of the inverse for `row`, with the given fold sites: the reference's GS loop on
    (exact, n) pairs -- exact = the pure-add part (an exact integer), n = how many multiply / fold outputs the value also sums.
    -> list over stages of (max exact |operand| among pure-add operands, max bound |exact| + n * reduced_bound(q) over all
    operands); the last entry is the final stage's two multiplies (u + v by n^-1, u - v by w1 * n^-1)."""
    n = len(row)
    val = [(int(x), 0) for x in row]
    R = reduced_bound(q)
    out = []
    t, stage = 1, 0
    while t < n:
        last = 2 * t == n
        ex, bd = 0, 0.0
        for j1 in range(0, n, 2 * t):
            for j in range(j1, j1 + t):
                (eu, nu), (ev, nv) = val[j], val[j + t]
                ops = [(eu - ev, nu + nv)] + ([(eu + ev, nu + nv)] if last else [])
                for e, k in ops:
                    if k == 0:
                        ex = max(ex, abs(e))
                    bd = max(bd, abs(e) + k * R)
                val[j] = (eu + ev, nu + nv)
                val[j + t] = (0, 1)
        out.append((ex, bd))
        for after, every in folds:
            if after == stage:
                for j in range(0, n, every):
                    val[j] = (0, 1)
        t, stage = 2 * t, stage + 1
    return out


def peak(model):
    """the largest operand bound over all stages of an inverse_model result"""
    return max(bd for _, bd in model)
