"""Verification inputs whose norm and weight are known exactly, for pinning the verdict predicates of fusion/fusion.py:718-728
(norm("infty") > beta_vf, weight() > omega_vf: algebra/polynomials.py:221-227) at the point where they flip.

The signature is built in the coefficient domain -- rows z [l][d], centred, with max |z| = M at a chosen (row, position) and a
chosen row of exactly W non-zero coefficients -- and transformed with the oracle, so that INTT(sig_hat) == z.  The targets are
made consistent with it: target = A . sig_hat (the target form), and keys with cent(vkL * c + vkR) == target (the keyed form,
and verify_core with alpha_hat == 1).  tests/test_verdict_edges_host.py checks the builder against both oracles."""
import numpy as np

from oracle import oracle as O

I32_MIN, I32_MAX = -(2 ** 31), 2 ** 31 - 1


def lazy_beta_max(q):
    """the largest beta for which verify_fused skips centring: beta < q/2 - q/4096 (launch_verify_fused, exact in fp64 for
    q < 2^32), i.e. 4096 * beta < 2047 * q"""
    return (2047 * q - 1) // 4096


def coef_rows(rng, l, d, M, W, heavy=0, extreme=0, pos=0, sign=1, spread=None):
    """[l][d] int64 centred rows: z[extreme][pos] = sign * M and max |z| = M; row `heavy` holds exactly W non-zero
    coefficients, every other row fewer (W - 1 at most; at least 1 in row `extreme`).  The other non-zero values are
    uniform on +-[1, spread] (spread defaults to M)."""
    assert 0 <= M and 0 <= W <= d and (M == 0) == (W == 0), (M, W)
    assert W >= 2 or extreme == heavy or M == 0, "a second non-zero row needs W >= 2"
    s = M if spread is None else min(spread, M)
    z = np.zeros((l, d), dtype=np.int64)
    if M == 0:
        return z
    for k in range(l):
        if k == heavy:
            w = W
        elif k == extreme:
            w = int(rng.integers(1, W)) if W > 2 else 1
        else:
            w = int(rng.integers(0, W))
        others = np.setdiff1d(np.arange(d), [pos]) if k == extreme else np.arange(d)
        idx = rng.choice(others, size=w - (k == extreme), replace=False)
        z[k, idx] = rng.integers(1, s + 1, size=idx.size) * rng.choice(np.array([-1, 1]), size=idx.size)
    z[extreme, pos] = sign * M
    return z


def measure(z, q):
    """-> (max |z| per aggregate, max row weight per aggregate) of coefficient rows [..][l][d]: the reference's norm("infty")
    over stored values and weight() = #{x : x mod q != 0}"""
    z = np.asarray(z, dtype=np.int64)
    return np.abs(z).max(axis=(-2, -1)), (z % q != 0).sum(axis=-1).max(axis=-1)


def expect(M, W, mismatch, beta, omega):
    """the reference's verdict (fusion.py:718-727) in its order: target, norm, weight -> codes 3, 4, 5, else 0"""
    M, W, mismatch = np.broadcast_arrays(np.asarray(M), np.asarray(W), np.asarray(mismatch, dtype=bool))
    return np.where(mismatch, 3, np.where(M > beta, 4, np.where(W > omega, 5, 0))).astype(np.int32).tolist()


def public_matrix(rng, l, d):
    """any int32 values, the extremes included"""
    A = rng.integers(I32_MIN, I32_MAX, size=(l, d), dtype=np.int64, endpoint=True).astype(np.int32)
    A[0, : d // 2] = I32_MIN
    A[l - 1, d // 2:] = I32_MAX
    return A


def keys_for(rng, target, q):
    """(vkL, vkR, c) [G][d] int32 with cent(vkL * c + vkR) == target (centred int32 [G][d]), covering the int32 extremes: half
    the columns take a free vkL and c (INT32_MIN / MAX among them) and solve vkR = cent(target - vkL * c); the other half
    take a free vkR (non-centred extremes among them) and an invertible c and solve vkL = cent((target - vkR) / c)"""
    G, d = target.shape
    ext = np.array([I32_MIN, I32_MAX, I32_MIN + 1, -1, 1, 0], dtype=np.int64)

    def draw(size):
        v = rng.integers(I32_MIN, I32_MAX, size=size, dtype=np.int64, endpoint=True)
        m = rng.random(size) < 0.3
        v[m] = rng.choice(ext, size=int(m.sum()))
        return v
    t = target.astype(np.int64)
    vkL, c, vkR = draw((G, d)), draw((G, d)), draw((G, d))
    free_r = rng.random((G, d)) < 0.5
    c[free_r & (c % q == 0)] = I32_MIN                          # invertible: q is odd, 2^31 is not a multiple of it
    half = q // 2

    def cent(v):
        v = v % q
        return np.where(v > half, v - q, v)
    vkR = np.where(free_r, vkR, cent(t - cent(vkL * c)))        # |vkL * c| < 2^62: exact in int64
    cinv = np.array([pow(int(x) % q, -1, q) if r else 0 for x, r in zip(c.ravel(), free_r.ravel())], dtype=np.int64).reshape(G, d)
    lhs = cent(t - vkR)
    vkL = np.where(free_r, cent(lhs * cinv), vkL)               # |lhs| < 2^31, cinv < 2^32: exact in int64
    return vkL.astype(np.int32), vkR.astype(np.int32), c.astype(np.int32)


class Fixture:
    """G aggregates of l rows at one parameter set: z [G][l][d] coefficient rows, sig [G][l][d] = NTT(z), A [l][d],
    target [G][d] = A . sig, keys (vkL, vkR, c) [G][d] with cent(vkL * c + vkR) == target, M / W [G] measured from z"""

    def __init__(self, P, A, z, rng, coracle):
        q, d = P["q"], P["d"]
        self.P, self.q, self.d = P, q, d
        self.A = A
        self.z = np.asarray(z, dtype=np.int64)
        self.G, self.l = self.z.shape[0], self.z.shape[1]
        assert np.abs(self.z).max() <= (q - 1) // 2
        self.sig = coracle.ntt_forward(self.z.astype(np.int32), q, P["root"]).reshape(self.z.shape)
        self.target = coracle.matvec(A, self.sig, q).reshape(self.G, d)
        self.vkL, self.vkR, self.c = keys_for(rng, self.target, q)
        self.M, self.W = measure(self.z, q)

    def tampered(self, groups):
        """(target, vkR) with one coefficient of each listed aggregate's target moved by 1 mod q"""
        t, r = self.target.copy(), self.vkR.copy()
        j = (7 * self.l) % self.d
        for g in groups:
            t[g, j] = t[g, j] - 1 if t[g, j] > 0 else t[g, j] + 1
            r[g, j] = r[g, j] - 1 if r[g, j] > 0 else r[g, j] + 1
        return t, r


def build(P, l, specs, seed, coracle, A=None):
    """specs: one dict per aggregate of coef_rows' keyword arguments (M, W, heavy, extreme, pos, sign, spread) -> Fixture"""
    rng = np.random.default_rng(seed)
    d = P["d"]
    z = np.stack([coef_rows(rng, l, d, **s) for s in specs])
    return Fixture(P, public_matrix(rng, l, d) if A is None else A, z, rng, coracle)


# ---- small moduli: norm / weight of stored int32 values ------------------------------------------------------------------
# the int32 contexts take every odd q from 3 to 2^32 - 1, ring-only ones (root 0) included: primes across that range, on
# both sides of 2^30 (below it an int32 holds multiples k * q with |k| >= 2) and of 2^31
SMALL_MODULI = (3, 17, 257, 7681, 12289, 65537, 1073741789, 1073741827, O.PRIME, 4294967291)


def small_modulus_rows(q, d, seed, max_multiples=4096):
    """[n][d] int32 rows of stored values for modulus q: every int32 multiple k * q (a sample of them, its extremes kept, when
    there are more than max_multiples), 0, +-1, INT32_MIN / MAX, and rows mixing those -- all-multiple rows among them (weight
    0 whatever their magnitude)"""
    rng = np.random.default_rng(seed)
    kmin, kmax = -(2 ** 31 // q), (2 ** 31 - 1) // q
    if kmax - kmin + 1 <= max_multiples:
        mult = np.arange(kmin, kmax + 1, dtype=np.int64) * q
    else:
        ks = np.unique(np.concatenate([[kmin, kmin + 1, -3, -2, -1, 0, 1, 2, 3, kmax - 1, kmax],
                                       rng.integers(kmin, kmax, size=max_multiples, endpoint=True)]))
        mult = ks * q
    pad = (-mult.size) % d
    rows = [np.concatenate([mult, rng.choice(mult, size=pad)]).reshape(-1, d)]      # multiples only
    special = np.array([0, 1, -1, I32_MIN, I32_MAX], dtype=np.int64)
    mixed = rng.choice(mult, size=(6, d))
    mixed[0, :5] = special
    mixed[1, d - 1] = 1                                        # one non-multiple, last
    mixed[2, 0] = -1                                           # ... first
    mixed[3] = rng.choice(special, size=d)
    mixed[4] = rng.integers(I32_MIN, I32_MAX, size=d, dtype=np.int64, endpoint=True)
    mixed[5, ::2] = mult.max()
    mixed[5, 1::2] = mult.min()
    rows.append(mixed)
    return np.concatenate(rows).astype(np.int32)


def py_norm_weight(rows, q):
    """the reference's norm("infty") and weight() per row, in Python integers"""
    return ([max(abs(int(x)) for x in r) for r in rows], [sum(1 for x in r if int(x) % q) for r in rows])
