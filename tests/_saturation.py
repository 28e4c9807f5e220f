"""Inputs that drive the lazily reduced sums of the accumulating kernels to their documented bounds, their expected outputs in
closed form, and a model of how many products each kernel puts into one lane's sum before it folds or converts it.

The kernels add raw products and reduce only at a cadence (aggregate_onepass: every kAggFold = 16 signers; aggregate_direct:
fold_if_due) or pick an exact form by size (matvec_sliced_kernel / keygen_fused / verify_fused: `small`; fz_launch_matvec and
the keygen / verify launchers: the integer form only while l <= 2^15).  Random operands never reach those bounds -- a sum of
random products grows like sqrt(N) -- so every fixture here is built from int32 extremes, one pattern per coefficient
column, constant over rows and (but for one mixed column) over signers: the exact sums are then closed forms in Python
integers, however long.  The products are ODD wherever the sum is meant to leave fp64's exact range: a sum of even products
such as INT32_MIN * 0xffff stays representable far beyond 2^53, and dropping a fold would go unseen.

tests/test_saturation_host.py checks the closed forms against the oracles and that each fixture defeats the kernel it
targets once the fold or guard is removed (agg_fold_free_error, imad_small_error, keygen_lane_error, outside_int64: the exact
fp64 / int64 arithmetic the kernel would do without it); tests/test_gpu_saturation.py runs them."""
import numpy as np

I32_MIN, I32_MAX = -(2 ** 31), 2 ** 31 - 1
I64_MIN, I64_MAX = -(2 ** 63), 2 ** 63 - 1
Q_WIDE = 4294967291                       # the largest int32-context modulus: 2^32 - 5
HI_ODD = -32767 * 65536                   # alpha / A with hi = -32767 (odd), lo = 0


def cent(v, q):
    """the reference's centred residue of a Python integer"""
    r = int(v) % q
    return r - q if r > q // 2 else r


def cent_arr(a, q):
    a = np.asarray(a, dtype=np.int64) % q
    return np.where(a > q // 2, a - q, a)


def split(a):
    """the kernels' split of an int32: a = hi * 2^16 + lo, hi = a >> 16 (arithmetic), lo = a & 0xffff"""
    return int(a) >> 16, int(a) & 0xffff


# ---- aggregation: one (sigma, alpha) pattern per coefficient column ------------------------------------------------------
# (x, a): the column's signature value (every row) and its alpha coefficient; "mixed" flips x's sign on alternate blocks of 32
# signers in the first half (the sum first cancels, then grows)
AGG_PATTERNS = (
    ("lo+", I32_MAX, -1),                 # lo = 0xffff, odd products near 2^47
    ("lo-", I32_MIN + 1, -1),
    ("lo_even", I32_MIN, -1),             # the issue's INT32_MIN * 0xffff: exact in fp64 up to 2^84 (kept for the sign)
    ("both+", I32_MAX, I32_MAX),          # hi = 32767, lo = 0xffff
    ("hi_odd-", I32_MAX, HI_ODD),         # hi = -32767, lo = 0: odd products near 2^46
    ("hi_odd+", I32_MIN + 1, HI_ODD),
    ("hi_even", I32_MAX, I32_MIN),        # hi = -2^15: multiples of 2^15, exact in fp64 up to 2^68
    ("hi_min", I32_MIN, I32_MIN),
    ("mixed", I32_MAX, -1),
)
NPAT = len(AGG_PATTERNS)


def mixed_sign(n):
    """[n] +-1: -1 on odd blocks of 32 signers in the first half"""
    i = np.arange(n)
    return np.where(((i // 32) % 2 == 1) & (i < n // 2), -1, 1)


def agg_signer_values(n):
    """(X, Al) [n][NPAT] int64: signer i's value and alpha coefficient in a column of each pattern"""
    X = np.tile(np.array([p[1] for p in AGG_PATTERNS], dtype=np.int64), (n, 1))
    Al = np.tile(np.array([p[2] for p in AGG_PATTERNS], dtype=np.int64), (n, 1))
    m = [p[0] for p in AGG_PATTERNS].index("mixed")
    X[:, m] *= mixed_sign(n)
    return X, Al


def agg_inputs(n, l, d):
    """(sig [n][l][d], alpha [n][d]) int32: column j follows pattern j % NPAT, every row alike"""
    X, Al = agg_signer_values(n)
    cols = np.arange(d) % NPAT
    sig = np.broadcast_to(X[:, None, cols], (n, l, d)).astype(np.int32)
    return np.ascontiguousarray(sig), np.ascontiguousarray(Al[:, cols].astype(np.int32))


def agg_expected(n, l, d, q):
    """[l][d] centred: cent(sum_i sigma_i * alpha_i), in Python integers"""
    X, Al = agg_signer_values(n)
    per = [cent(sum(int(x) * int(a) for x, a in zip(X[:, p], Al[:, p])), q) for p in range(NPAT)]
    row = np.array([per[j % NPAT] for j in range(d)], dtype=np.int64)
    return np.broadcast_to(row, (l, d)).copy()


# the verification target's inputs: per column (vkL, c, vkR), the same for every signer
KEY_PATTERNS = ((I32_MIN, I32_MAX, I32_MAX), (I32_MAX, I32_MAX, I32_MIN), (I32_MIN, I32_MIN, I32_MIN), (I32_MAX, -1, I32_MAX),
                (-1, I32_MIN, -1))


def target_inputs(n, d):
    """(vkL, vkR, c) [n][d] int32"""
    P = np.array(KEY_PATTERNS, dtype=np.int64)[np.arange(d) % len(KEY_PATTERNS)]
    rep = lambda v: np.ascontiguousarray(np.broadcast_to(v, (n, d)).astype(np.int32))      # noqa: E731
    return rep(P[:, 0]), rep(P[:, 2]), rep(P[:, 1])


def target_expected(n, d, q):
    """[d] centred: cent(sum_i (vkL_i * c_i + vkR_i) * alpha_i) with agg_inputs' alpha"""
    _, Al = agg_signer_values(n)
    asum = [sum(int(a) for a in Al[:, p]) for p in range(NPAT)]
    out = []
    for j in range(d):
        L, c, R = KEY_PATTERNS[j % len(KEY_PATTERNS)]
        out.append(cent((L * c + R) * asum[j % NPAT], q))
    return np.array(out, dtype=np.int64)


def sign_inputs(n, l, d, q):
    """fused signing: (sk_hat [n][2][l][d], c [n][d]) int32 of extremes and the signatures they make, cent(cent(L * c) + R):
    the vkL / vkR of target_inputs as the two key halves of every row, c from the same table"""
    L, R, c = target_inputs(n, d)
    sk = np.stack([np.broadcast_to(L[:, None, :], (n, l, d)), np.broadcast_to(R[:, None, :], (n, l, d))], axis=1)
    sig = cent_arr(cent_arr(L.astype(np.int64) * c, q) + R, q)
    return np.ascontiguousarray(sk.astype(np.int32)), c, np.broadcast_to(sig[:, None, :], (n, l, d)).astype(np.int32)


def sign_agg_expected(n, l, d, q):
    """[l][d]: the aggregate of sign_inputs' signatures with agg_inputs' alpha"""
    _, _, sig = sign_inputs(1, 1, d, q)
    _, Al = agg_signer_values(n)
    asum = [sum(int(a) for a in Al[:, p]) for p in range(NPAT)]
    row = [cent(int(sig[0, 0, j]) * asum[j % NPAT], q) for j in range(d)]
    return np.broadcast_to(np.array(row, dtype=np.int64), (l, d)).copy()


# ---- the aggregation kernels' per-lane sums (fz_launch_aggregate, fz_aggregate.hip) --------------------------------------
AGG_WAVES, AGG_DEPTH, AGG_R, AGG_FOLD = 8, 3, 4, 16


def direct_taken(knob, groups, N, d, target=False, sign=False):
    """does fz_launch_aggregate take aggregate_direct (FZ_AGG_DIRECT = knob)?"""
    return not sign and d // 4 >= 16 and knob >= 0 and (knob > 0 or (not target and groups * N <= 128)) and groups <= 65535


def onepass_shape(num_cu, groups, N, l, d, target=False, sig=True):
    """-> (AR, nsl): int4 columns per lane and signer slices per aggregate, as the launcher picks them (N: the largest group)"""
    cols_a = l * (d // 4)
    ar, nsl, best = 0, 1, 0
    for cand in (4, 3, 2):
        na = -(-cols_a // (64 * cand)) if sig else 0
        blocks_min = (na + (1 if target else 0)) * groups
        ns = min(num_cu // blocks_min, N // (AGG_WAVES * AGG_DEPTH))
        ns = min(max(ns, 1), 512)
        if N > 0 and ns > N:
            ns = N
        if N == 0:
            ns = 1
        tiles = blocks_min * ns
        if ar == 0 or (best <= num_cu and tiles <= num_cu and tiles * 16 >= best * 17):
            ar, nsl, best = cand, ns, tiles
    na4 = -(-cols_a // (64 * AGG_R)) if sig else 0
    if (na4 + (1 if target else 0)) * groups > num_cu:
        ar, nsl = 2, 1
    return ar, nsl


def onepass_lanes(n, nsl):
    """signer indices (within the aggregate) of every lane sum of one coefficient: slice sb, wave w takes i0 + w, i0 + w + 8, .."""
    base, extra = n // nsl, n % nsl
    out = []
    for sb in range(nsl):
        i0 = sb * base + min(sb, extra)
        i1 = i0 + base + (1 if sb < extra else 0)
        out += [list(range(i0 + w, i1, AGG_WAVES)) for w in range(AGG_WAVES)]
    return [s for s in out if s]


def direct_lanes(n, waves=AGG_WAVES):
    """aggregate_direct: lane group `sub` of wave w takes signers w * 4 + sub + 32 t (16-column tiles, 4 signers per wave)"""
    step = 4 * waves
    return [list(range(w * 4 + s, n, step)) for w in range(waves) for s in range(4) if w * 4 + s < n]


def fp64_chain(products):
    """the value an fp64 FMA chain s = fma(x, a, s) ends with, exactly: every step rounds the exact s + x * a once"""
    s = 0.0
    for p in products:
        s = float(int(s) + int(p))        # Python's int -> float conversion rounds to nearest, ties to even
    return int(s)


def agg_fold_free_error(lanes, pattern, n):
    """the error a kernel WITHOUT its in-loop fold leaves in one coefficient of `pattern`'s columns: sum over the lane sums of
    (rounded - exact) of the hi and lo chains, hi weighted by 2^16 (the final fold and the combine are exact)"""
    X, Al = agg_signer_values(n)
    err = 0
    for idx in lanes:
        for part, w in ((0, 65536), (1, 1)):
            prods = [int(X[i, pattern]) * split(Al[i, pattern])[part] for i in idx]
            err += w * (fp64_chain(prods) - sum(prods))
    return err


def agg_max_lane_sum(lanes, pattern, n):
    """max over lanes of the exact unfolded |sum| of the hi and lo products (running sums included)"""
    X, Al = agg_signer_values(n)
    top = 0
    for idx in lanes:
        for part in (0, 1):
            s = 0
            for i in idx:
                s += int(X[i, pattern]) * split(Al[i, pattern])[part]
                top = max(top, abs(s))
    return top


# ---- matvec / keygen / verify: A (.) y over l rows -----------------------------------------------------------------------
# (A, y) per column: A's value in every row and y's (the signature's / the secret transform's) in every row but row 0, whose y
# is `y0` (parity: makes the column's total odd whatever l is); "mixed" negates y on odd rows of the first half
MV_PATTERNS = (
    ("lo_odd", -1, I32_MAX),              # lo = 0xffff, odd: the fp64 conversion of l > 64 products is inexact
    ("lo_min", -1, I32_MIN),              # |y * lo| = 2^47 - 2^31, the largest: its int64 sum leaves int64 at l = 65538
    ("both", I32_MAX, I32_MIN),           # hi = 32767, lo = 0xffff, same sign
    ("hi_min", I32_MIN, I32_MIN),         # hi = -2^15: y * hi = +2^46
    ("hi_odd", HI_ODD, I32_MAX),
    ("mixed", -1, I32_MAX),
)
NMV = len(MV_PATTERNS)


def mv_row_values(l):
    """(Acol [NMV], Y [l][NMV]) int64: A's value and y of every row in a column of each pattern"""
    A = np.array([p[1] for p in MV_PATTERNS], dtype=np.int64)
    y = np.array([p[2] for p in MV_PATTERNS], dtype=np.int64)
    Y = np.tile(y, (l, 1))
    Y[0, 0] = y[0] - (1 - l % 2)          # the odd column's total: odd for every l
    m = [p[0] for p in MV_PATTERNS].index("mixed")
    k = np.arange(l)
    Y[:, m] *= np.where((k % 2 == 1) & (k < l // 2), -1, 1)
    return A, Y


def mv_inputs(l, d, batch=1):
    """(A [l][d], S [batch][l][d]) int32: column j follows pattern j % NMV"""
    Acol, Y = mv_row_values(l)
    cols = np.arange(d) % NMV
    A = np.ascontiguousarray(np.broadcast_to(Acol[cols], (l, d)).astype(np.int32))
    S = np.ascontiguousarray(np.broadcast_to(Y[:, cols], (batch, l, d)).astype(np.int32))
    return A, S


def mv_totals(l):
    """[NMV] (hi_total, lo_total): sum_k y_k * hi(A), sum_k y_k * lo(A) over all l rows, exact"""
    Acol, Y = mv_row_values(l)
    out = []
    for p in range(NMV):
        hi, lo = split(Acol[p])
        s = int(Y[:, p].sum())            # |s| <= l * 2^31 < 2^63
        out.append((s * hi, s * lo))
    return out


def mv_expected(l, d, q):
    """[d] centred: cent(sum_k A_k * y_k) per column"""
    per = [cent(h * 65536 + lo, q) for h, lo in mv_totals(l)]
    return np.array([per[j % NMV] for j in range(d)], dtype=np.int64)


def inexact_in_fp64(v):
    return float(int(v)) != v


def outside_int64(v):
    return not I64_MIN <= v <= I64_MAX


# the `small` flag and the imad guards, as the launchers derive them
def matvec_sliced_taken(knob, batch, l, d, num_cu, guard=True):
    """does fz_launch_matvec take matvec_sliced_kernel (FZ_MATVEC_SLICES = knob; guard=False: without `l <= 32768`)?"""
    split_k = batch * (d // 4) < num_cu * 256 if knob < 0 else (knob == 0 and batch <= num_cu * 2)
    return not split_k and (l <= 32768 or not guard) and knob >= 0


def matvec_route(knob, batch, l, d, num_cu, aligned=True):
    """the kernel fz_launch_matvec takes (FZ_MATVEC_SLICES = knob; aligned: A, S and out all 16-byte aligned) ->
    "split" | ("sliced", KS) | "kernel" | "scalar"; KS as the launcher settles it: the knob's 1 | 2 | 4 | 8 | 16 (any other value:
    by the number of waves), then halved while a slice would hold fewer than eight rows"""
    if d % 4 or not aligned:
        return "scalar"
    pow2 = d & (d - 1) == 0
    if 16 <= d <= 4096 and pow2 and (batch * (d // 4) < num_cu * 256 if knob < 0 else (knob == 0 and batch <= num_cu * 2)):
        return "split"
    if l <= 32768 and knob >= 0:
        ks = knob
        if ks not in (1, 2, 4, 8, 16):
            waves1 = -(-batch * (d // 4) // 64)
            ks = 1
            while ks < 16 and waves1 * ks < num_cu * 8:
                ks <<= 1
        while ks > 1 and l // ks < 8:
            ks >>= 1
        return ("sliced", ks)
    return "kernel"


KEYGEN_WAVES, VERIFY_WAVES = 4, 4


def keygen_lanes(l, d):
    """keygen_fused: per (wave, row slot p) the rows whose products enter that lane's sums (PPW = 256 / d row slots per wave,
    task t holds rows t * PPW + p, wave w takes tasks w, w + 4, ..)"""
    ppw = 256 // d
    tasks = -(-l // ppw)
    return tasks, [[t * ppw + p for t in range(w, tasks, KEYGEN_WAVES) if t * ppw + p < l]
                   for w in range(KEYGEN_WAVES) for p in range(ppw)]


def keygen_small(l, d):
    tasks, _ = keygen_lanes(l, d)
    return tasks <= 32 * KEYGEN_WAVES


def verify_shape(l, d, groups, num_cu, no_imad=False):
    """-> (R, imad, small, lanes): workgroups per aggregate, the integer form's choice, its `small` flag, and the rows of
    every lane sum of one coefficient (workgroup r, wave w, row slot p: tasks r * 4 + w + t * 4R)"""
    ppw = 256 // d
    tasks = -(-l // ppw)
    R = -(-tasks // VERIFY_WAVES)
    R = max(1, min(R, num_cu * 2 // groups, 64))
    step = R * VERIFY_WAVES
    imad = not no_imad and l <= 2 ** 15 and -(-tasks // step) >= 4
    lanes = [[t * ppw + p for t in range(r * VERIFY_WAVES + w, tasks, step) if t * ppw + p < l]
             for r in range(R) for w in range(VERIFY_WAVES) for p in range(ppw)]
    return R, imad, tasks <= 32 * step, lanes


def imad_small_error(lanes, l, pattern):
    """the error `small = true` leaves in one coefficient of `pattern`'s columns when the lane sums are in fact longer:
    fz_imad_total converts hi and lo to fp64 as they are (the folds after it are exact)"""
    Acol, Y = mv_row_values(l)
    hi, lo = split(Acol[pattern])
    err = 0
    for rows in lanes:
        s = int(Y[rows, pattern].sum()) if rows else 0
        err += 65536 * (int(float(s * hi)) - s * hi) + (int(float(s * lo)) - s * lo)
    return err


def max_lane_products(lanes):
    return max(len(r) for r in lanes)


# ---- keygen: secrets whose transform is a constant -------------------------------------------------------------------
def impulse_rows(n, l, d, v):
    """coef [n][2][l][d] int32: every row of half 0 is [v, 0, .., 0], of half 1 [-v, 0, .., 0] -- the transform of a scaled unit
    impulse is v in every coefficient, so y saturates the centred range in every row of the A (.) y sum"""
    c = np.zeros((n, 2, l, d), dtype=np.int32)
    c[:, 0, :, 0] = v
    c[:, 1, :, 0] = -v
    return c


def keygen_A(l, d):
    """A [l][d] for keygen: mv_inputs' A (any int32)"""
    return mv_inputs(l, d)[0]


def keygen_expected(l, d, q, v):
    """vk [2][d] for impulse_rows(.., v) and keygen_A: cent(l * A_j * (+-v))"""
    Acol, _ = mv_row_values(1)
    row = np.array([cent(l * int(Acol[j % NMV]) * v, q) for j in range(d)], dtype=np.int64)
    return np.stack([row, cent_arr(-row, q)])


def keygen_lane_error(l, d, q, v, pattern):
    """keygen_fused with `small = true` at this l: the error in a column of `pattern` (half 0), the secret rows impulse_rows'"""
    _, lanes = keygen_lanes(l, d)
    hi, lo = split(mv_row_values(1)[0][pattern])
    err = 0
    for rows in lanes:
        s = len(rows) * v
        err += 65536 * (int(float(s * hi)) - s * hi) + (int(float(s * lo)) - s * lo)
    return err


def odd_half_q(q):
    """the largest odd y <= (q - 1) / 2: (q - 1) / 2 itself is even for the scheme's prime (a multiple of 2^8), and sums of
    its products stay exact in fp64 long after 2^53"""
    h = (q - 1) // 2
    return h if h % 2 else h - 1


# ---- verification from int64 partial sums -----------------------------------------------------------------------------
I64_PATTERNS = (I64_MIN, I64_MAX, I64_MIN + 1, I64_MAX - 1, -(2 ** 62), 2 ** 53 + 1, -1, 0)


def i64_rows(l, d):
    """[l][d] int64 signature partial sums: pattern j % 8 of I64_PATTERNS (what an all-reduce may leave: any int64)"""
    row = np.array(I64_PATTERNS, dtype=np.int64)[np.arange(d) % len(I64_PATTERNS)]
    return np.ascontiguousarray(np.broadcast_to(row, (l, d)))


def i64_expected(A, l, d, q):
    """[d]: cent(sum_k A_k * cent(s_k)) for i64_rows (every row alike; A's rows alike as mv_inputs makes them)"""
    s = [cent(int(v), q) for v in i64_rows(1, d)[0]]
    return np.array([cent(l * int(A[0, j]) * s[j], q) for j in range(d)], dtype=np.int64)


def far_representative(t, q, top=True):
    """an int64 congruent to t mod q within q of INT64_MAX (top) or INT64_MIN"""
    t = int(t)
    return t + ((I64_MAX - t) // q) * q if top else t - ((t - I64_MIN) // q) * q
