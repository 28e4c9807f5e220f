"""The compact byte encoding as a function of the CONTEXT -- (q, degree, forward table, inverse table,
rows, bound), not of a security parameter -- with the contexts, rows, fields and multipliers that take the records kernels
(csrc/fz_records.hip, fz_aggregate_encoded.hip, fz_verify_encoded.hip) where the scheme's own objects never go:

- both twiddle-multiply forms at degrees 64 and 256: the moduli and tables of tests/_transform_edges.py on either side of `fast`,
  and q = 4294828033, a prime in [2^31, 2^32) with roots, so that the 6-op instantiations and a field width of 32 are reached;
- encoder side: the int32-extreme rows of _transform_edges.rows as they are, with the exact maximum M = max |z| of every record
  (bound = M encodes, bound = M - 1 refuses: the range test on both sides, for q on either side of 2^31);
- decoder side: fields at 0 and 2B on every coefficient and in the stage sign patterns, at B = (q - 1) / 2 -- the largest operands
  a canonical record can hand to the forward passes;
- multipliers (alpha_hat, A, vk / c_hat) at the int32 extremes (the column patterns of tests/_saturation.py) beside random rows;
- every field width 2 .. 32 at the smallest and the largest bound of that width.

Everything is Python integers or int64 numpy; the transforms are the reference loops (oracle.py_ntt_forward / py_ntt_inverse) with
the same tables the context is given, each distinct row transformed once.  The bytes are spec_pack / spec_unpack of
tests/test_encoding_host.py (functions of (B, w) alone).  tests/test_encoded_edges_host.py checks these fixtures on the CPU;
tests/test_gpu_encoded_edges.py holds the kernels to them, tests/test_gpu_many_encoded_edges.py the many-committee kernels
(group_partials, group_targets, same_sign_inputs)."""
import functools

import numpy as np

from oracle import oracle as O

import _saturation as S
import _transform_edges as E
from test_encoding_host import spec_pack, spec_unpack
from test_verify_encoded_host import get_field, set_field      # noqa: F401 (the GPU module takes them from here)

I32_MIN, I32_MAX = E.I32_MIN, E.I32_MAX
Q_TOP = 4294828033                         # 2^32 - 139263 = 1 (mod 8192): tests/test_gpu_generic_params.py's prime at degree 256
DEGREES = (64, 256)

# (name, kind): kind "odd" / "q1" a table context on E.TABLE_MODULI[name], "root" an ordinary root context; (secpar, "params") is
# the scheme's own context (oracle.PARAMS), which the host test holds against the golden objects
SPECS = [(k, "odd") for k in E.TABLE_MODULI] + [("d32767", "q1"), ("k17", "q1"), ("scheme", "q1")] + \
    [(k, "root") for k in E.ROOT_MODULI] + [("top", "root")]
# the width sweep's contexts: a fast and a 6-op table context that reach w = 31 and w = 32 (2^31 - 1: (q - 1) / 2 = 2^30 - 1;
# 2^32 - 1: 2^31 - 1), 2^31 + 1 for (w, B) = (32, 2^30), and a root context of either form for the encoder's coefficient kinds
SWEEP_SPECS = [("m31", "odd"), ("w32", "odd"), ("p31", "odd"), ("scheme", "root"), ("top", "root")]


def sid(spec):
    return f"{spec[0]}-{spec[1]}"


@functools.lru_cache(maxsize=None)
def _top_root_512():
    return E.root_512(Q_TOP)               # the search of test_gpu_generic_params.root_of(Q_TOP, 256)


def root_of(spec, n):
    """(q, root, inv_root) of a root context: a primitive 2n-th root, for "top" the 256 / n-th power of the degree-256 root"""
    if spec[0] == "top":
        r = pow(_top_root_512(), 256 // n, Q_TOP)
        return Q_TOP, r, pow(r, Q_TOP - 2, Q_TOP)
    return E.root_of(spec[0], n)


@functools.lru_cache(maxsize=None)
def tables(spec, n):
    """(q, fwd, inv): the tables the context of `spec` at degree n transforms with"""
    if spec[1] == "params":
        P = O.PARAMS[spec[0]]
        assert n == P["d"]
        return P["q"], O.py_twiddles(P["root"], P["q"], n), O.py_twiddles(P["inv_root"], P["q"], n)
    if spec[1] == "root":
        q, r, ir = root_of(spec, n)
        return q, E.bitrev_powers(r, q, n), E.bitrev_powers(ir, q, n)
    return E.tables(spec[0], n, spec[1])


def modulus(spec):
    if spec[1] == "params":
        return O.PARAMS[spec[0]]["q"]
    return Q_TOP if spec[0] == "top" else (E.ROOT_MODULI[spec[0]][0] if spec[1] == "root" else E.TABLE_MODULI[spec[0]])


def half(spec):
    return (modulus(spec) - 1) // 2


def width(B):
    return (2 * B).bit_length()


def record_bytes(n, rows, w):
    return rows * n // 8 * w


def cent(a, q):
    return S.cent_arr(a, q)


# ---- the transforms: the reference loops, one call per distinct row --------------------------------------------------------
_DONE = {}


def _transform(spec, n, a, inverse):
    a = np.asarray(a, dtype=np.int64)
    q, fwd, inv = tables(spec, n)
    out = np.empty_like(a)
    flat, oflat = a.reshape(-1, n), out.reshape(-1, n)
    for i, row in enumerate(flat):
        key = (spec, n, inverse, row.tobytes())
        if key not in _DONE:
            v = [int(x) for x in row]
            _DONE[key] = np.array(O.py_ntt_inverse(v, q, inv) if inverse else O.py_ntt_forward(v, q, fwd), dtype=np.int64)
        oflat[i] = _DONE[key]
    return out


def forward(spec, n, z):
    """cent(NTT(z)) of every row of an [.., n] array"""
    return _transform(spec, n, z, False)


def inverse(spec, n, rows):
    """cent(INTT(row)) of every row of an [.., n] array of any int32"""
    return _transform(spec, n, rows, True)


# ---- the spec --------------------------------------------------------------------------------------------------------------
def values(spec, n, rows, coef):
    """the centred integers z a record carries: cent(INTT(row)) for the coefficient kinds, cent(row) for keys"""
    return inverse(spec, n, rows) if coef else cent(rows, modulus(spec))


def decoded(spec, n, z, coef):
    """the rows decode leaves: cent(NTT(z)), keys z"""
    return forward(spec, n, z) if coef else np.asarray(z, dtype=np.int64)


def maxima(z):
    """[N]: the exact M = max |z| of every record of z [N][rows][n]"""
    return np.abs(z).reshape(z.shape[0], -1).max(axis=1)


def encoded(z, B):
    """what the encoder leaves at bound B for records z [N][rows][n]: (bytes [N][record bytes], status [N]); a record with some
    |z| > B has status 4 and all-zero bytes"""
    w = width(B)
    st = np.where(maxima(z) > B, 4, 0).astype(np.int32)
    data = np.zeros((z.shape[0], record_bytes(z.shape[2], z.shape[1], w)), dtype=np.uint8)
    if (st == 0).any():
        data[st == 0] = spec_pack(z[st == 0], B, w)
    return data, st


def canonical(record, B, shape):
    """is every field of one record's bytes at most 2B?"""
    try:
        spec_unpack(record[None], B, width(B), shape)
        return True
    except ValueError:
        return False


def one_past(record, j, B):
    """a copy of the record with field j at 2B + 1 (None when that is no w-bit value)"""
    w = width(B)
    return set_field(record, j, 2 * B + 1, w) if 2 * B + 1 < (1 << w) else None


def aggregate_partial(spec, n, z, alpha, skip=None):
    """[l][n] int64: sum over the records i with skip[i] == 0 of cent(NTT(z_i) (.) alpha_i); z [N][l][n], alpha [N][n] any int32
    (|NTT(z)| < 2^31 and |alpha| <= 2^31: every product fits int64)"""
    q = modulus(spec)
    prod = cent(forward(spec, n, z) * np.asarray(alpha, dtype=np.int64)[:, None, :], q)
    if skip is not None:
        prod = prod[np.asarray(skip) == 0]
    return prod.sum(axis=0).astype(np.int64).reshape(z.shape[1:])


def group_bounds(sizes):
    """[(first, one past the last)] record of every group of consecutive records"""
    off = np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))])
    return [(int(a), int(b)) for a, b in zip(off, off[1:])]


def group_partials(spec, n, z, alpha, sizes, skip=None):
    """[G][l][n] int64: aggregate_partial of every group of sizes[g] consecutive records of z [N][l][n] / alpha [N][n] / skip [N];
    a group with no kept record (none at all, or every one skipped) gives zeros"""
    z, alpha = np.asarray(z, dtype=np.int64), np.asarray(alpha, dtype=np.int64)
    assert sum(sizes) == z.shape[0] == alpha.shape[0] and (skip is None or len(skip) == z.shape[0])
    out = np.zeros((len(sizes),) + z.shape[1:], dtype=np.int64)
    for g, (a, b) in enumerate(group_bounds(sizes)):
        sk = None if skip is None else np.asarray(skip)[a:b]
        if b > a and (sk is None or (sk == 0).any()):
            out[g] = aggregate_partial(spec, n, z[a:b], alpha[a:b], sk)
    return out


def group_targets(spec, vk, c_hat, alpha, sizes, skip=None):
    """[G][n] int64: per group of sizes[g] consecutive signers the sum, over those with skip[i] == 0, of
    cent(keyed_target(spec, vk_i, c_i) * alpha_i); vk [N][2][n], c_hat / alpha [N][n] any int32 (every factor is below 2^31 in
    size: the products fit int64).  The kernels' target partials are these sums modulo q only"""
    q = modulus(spec)
    term = cent(keyed_target(spec, vk, c_hat) * np.asarray(alpha, dtype=np.int64), q)
    assert sum(sizes) == term.shape[0] and (skip is None or len(skip) == term.shape[0])
    keep = np.ones(term.shape[0], dtype=bool) if skip is None else np.asarray(skip) == 0
    out = np.zeros((len(sizes), term.shape[1]), dtype=np.int64)
    for g, (a, b) in enumerate(group_bounds(sizes)):
        out[g] = term[a:b][keep[a:b]].sum(axis=0)
    return out


def verify_sums(spec, n, z, A):
    """[N][n] centred: cent(sum_k A_k (.) NTT(z_k)); z [N][l][n], A [l][n] any int32"""
    q = modulus(spec)
    return cent(cent(forward(spec, n, z) * np.asarray(A, dtype=np.int64)[None], q).sum(axis=1), q)


def keyed_target(spec, vk, c_hat):
    """[N][n] centred: cent(vk_L (.) c + vk_R); vk [N][2][n], c_hat [N][n] any int32 (|vk_L c + vk_R| < 2^63)"""
    vk, c = np.asarray(vk, dtype=np.int64), np.asarray(c_hat, dtype=np.int64)
    return cent(vk[:, 0] * c + vk[:, 1], modulus(spec))


def verdicts(spec, sums, target):
    """0 where the target is the sums' class mod q, else 3"""
    q = modulus(spec)
    return np.where(((np.asarray(target, dtype=np.int64) - sums) % q != 0).any(axis=1), 3, 0).astype(np.int32)


def other_representative(t, q):
    """the centred words t as another int32 of the same class where there is one: t - q, else t + q"""
    t = np.asarray(t, dtype=np.int64)
    return np.where(t - q >= I32_MIN, t - q, np.where(t + q <= I32_MAX, t + q, t))


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def records_of(rowlist, per, count=None):
    """[N][per][n]: record r holds rows r * per .., the list taken cyclically (N = enough records to hold every row once)"""
    a = np.asarray(rowlist, dtype=np.int64)
    count = count or -(-a.shape[0] // per)
    idx = (np.arange(count * per) % a.shape[0]).reshape(count, per)
    return a[idx]


def encoder_rows(spec, n):
    """the encoder's inputs: _transform_edges.rows as they are (any int32), [R][n]"""
    return np.array([r for _, r in E.rows(modulus(spec), n)], dtype=np.int64)


def decoder_rows(spec, n):
    """(names, z [R][n]) with every |z| <= B = (q - 1) / 2: the constants +B and -B, the stage sign patterns of
    _transform_edges.rows scaled to +-B with the first entry one step towards zero (an odd sum), and one random row"""
    q, B = modulus(spec), half(spec)
    names, out = ["+B", "-B"], [[B] * n, [-B] * n]
    for name, row in E.rows(q, n)[6:]:
        p = [B if v > 0 else -B for v in row]
        p[0] -= 1 if p[0] > 0 else -1
        names.append(name)
        out.append(p)
    rng = np.random.default_rng(n + q % 1000)
    names.append("random")
    out.append(rng.integers(-B, B + 1, size=n, dtype=np.int64).tolist())
    return names, np.array(out, dtype=np.int64)


def edge_fields(B, count, rows, n, seed):
    """fields [count][rows][n] in [0, 2B], random but for field 0, the last field and one in the middle of every record: 0, 2B, 0
    in the even records and 2B, 0, 2B in the odd ones"""
    rng = np.random.default_rng(seed)
    u = rng.integers(0, 2 * B + 1, size=(count, rows * n), dtype=np.int64)
    for i in range(count):
        a, b = (0, 2 * B) if i % 2 == 0 else (2 * B, 0)
        u[i, 0], u[i, -1], u[i, rows * n // 2 + 3] = a, b, a
    return u.reshape(count, rows, n)


def _columns(values_, n):
    v = np.array(values_, dtype=np.int64)
    return v[np.arange(n) % len(v)]


def extreme_rows(n):
    """[8][n] int32-extreme multiplier rows: the column patterns of _saturation (AGG_PATTERNS' alpha and sigma values,
    MV_PATTERNS' A and y values, KEY_PATTERNS' three columns) and one row of INT32_MIN / INT32_MAX / -1 by column"""
    return np.stack([_columns([p[2] for p in S.AGG_PATTERNS], n), _columns([p[1] for p in S.AGG_PATTERNS], n),
                     _columns([p[1] for p in S.MV_PATTERNS], n), _columns([p[2] for p in S.MV_PATTERNS], n),
                     _columns([p[0] for p in S.KEY_PATTERNS], n), _columns([p[1] for p in S.KEY_PATTERNS], n),
                     _columns([p[2] for p in S.KEY_PATTERNS], n), _columns([I32_MIN, I32_MAX, -1], n)])


def multipliers(count, n, seed):
    """[count][n] any int32: extreme_rows first (cyclically from `seed`), every third row from the eighth on random"""
    ext = extreme_rows(n)
    rng = np.random.default_rng(seed)
    out = ext[(np.arange(count) + seed) % len(ext)].copy()
    for i in range(count):
        if i % 3 == 2 or i >= 2 * len(ext):
            out[i] = rng.integers(I32_MIN, I32_MAX + 1, size=n, dtype=np.int64)
    return out


def key_inputs(count, n, seed):
    """(vk [count][2][n], c_hat [count][n]) any int32: KEY_PATTERNS' columns in the even records, random in the odd ones"""
    L, R, c = (a.astype(np.int64) for a in S.target_inputs(count, n))
    rng = np.random.default_rng(seed)
    vk, ch = np.stack([L, R], axis=1), c.copy()
    for i in range(1, count, 2):
        vk[i] = rng.integers(I32_MIN, I32_MAX + 1, size=(2, n), dtype=np.int64)
        ch[i] = rng.integers(I32_MIN, I32_MAX + 1, size=n, dtype=np.int64)
    return vk, ch


def same_sign_inputs(spec, n, l, N, B, sign):
    """(z [N][l][n], alpha [N][n]) on a root context with a prime modulus: every product cent(NTT(z_i) (.) alpha_i) is exactly
    sign * h, h = (q - 1) / 2, so every partial of a group of N_g signers is sign * N_g * h -- the largest sum N_g signers can
    leave.  A record is l copies of one of five random rows with |z| <= B whose forward coefficients are all units, and
    alpha_i = cent(sign * h * NTT(z_i)^-1)"""
    q, h = modulus(spec), half(spec)
    assert spec[1] == "root" and sign in (1, -1)         # (the inverses are Fermat's: the products are checked below)
    rng = np.random.default_rng(n + l + q % 1000)
    pool = rng.integers(-B, B + 1, size=(5, n), dtype=np.int64)
    F = forward(spec, n, pool)
    assert (F % q != 0).all(), "a forward coefficient is 0 mod q: it has no inverse"
    inv = np.array([[pow(int(v) % q, q - 2, q) for v in row] for row in F], dtype=object)
    alpha = cent(np.array((sign * h * inv) % q, dtype=np.int64), q)
    assert (cent(F * alpha, q) == sign * h).all() and I32_MIN <= alpha.min() and alpha.max() <= I32_MAX
    idx = np.arange(N) % 5
    return np.repeat(pool[idx][:, None, :], l, axis=1), alpha[idx]


def solve_right_key(spec, vk, c_hat, sums):
    """vk with its right half replaced by cent(sums - vk_L (.) c): the keyed target of the result is `sums`"""
    q = modulus(spec)
    vk = np.array(vk, dtype=np.int64)
    vk[:, 1] = cent(np.asarray(sums, dtype=np.int64) - cent(vk[:, 0] * np.asarray(c_hat, dtype=np.int64), q), q)
    return vk


# ---- the width sweep ---------------------------------------------------------------------------------------------------------
def sweep_bounds(w):
    """the smallest and the largest bound of width w: 2^(w-2) and 2^(w-1) - 1 (w = 2: both are 1)"""
    return sorted({1 << (w - 2), (1 << (w - 1)) - 1})


WIDTHS = tuple(range(2, 33))
SWEEP = [(w, B) for w in WIDTHS for B in sweep_bounds(w)]


def sweep_specs(B):
    """the sweep contexts whose modulus admits the bound"""
    return [s for s in SWEEP_SPECS if B <= half(s)]


def sweep_shapes(n):
    """rows per record of the record walkers (encode, decode, check): 1, and at degree 64 also 3, so that for odd w an odd
    record count ends the stream 8 bytes into a 16-byte unit"""
    return (1, 3) if n == 64 else (1,)


# ---- the kernels' arithmetic, for the host replay ----------------------------------------------------------------------------
def encoder_refuses(z, B, hi=True):
    """records_encode's range test on one centred value, in its own arithmetic: s = z + B as a 64-bit word; refused when the
    high word is set (`hi`: z < -B) or the low word exceeds 2B (z > B).  hi=False: the test without its first half"""
    s = (int(z) + B) & (2 ** 64 - 1)
    return (hi and (s >> 32) != 0) or (s & 0xffffffff) > 2 * B


def lazy_forward(z, q, fwd, mul=None):
    """the forward passes as the kernels run them (fwd16_passes): the reference's Cooley-Tukey network, only the twiddle
    product reduced and the sums left to grow -- -> (unreduced outputs, the largest |operand| of a multiply or |output|).
    mul(a, w) is the twiddle multiply (default: the canonical product); the outputs are NTT(z) mod q whatever exact multiply is
    used, and |output| <= |z| + log2(n) * max |product|"""
    mul = mul or (lambda a, w: E.cent(a * w, q))
    val = [int(v) for v in z]
    n = len(val)
    top = max(abs(v) for v in val)
    t, m = n, 1
    while m < n:
        t //= 2
        for i in range(m):
            s = fwd[m + i]
            for j in range(2 * i * t, 2 * i * t + t):
                u, v = val[j], mul(val[j + t], s)
                val[j], val[j + t] = u + v, u - v
                top = max(top, abs(u + v), abs(u - v))
        m *= 2
    return val, top
