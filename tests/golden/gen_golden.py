#!/usr/bin/env python3
"""Generate the golden vectors under tests/golden/ by RUNNING THE REFERENCE.

Run only in the development container, where the reference checkout is mounted read-only:

    PYTHONPATH=/root/reference PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/gen_golden.py

Everything written here is data (inputs + the reference's outputs); no reference source is
copied.  The GPU box never sees the reference -- tests read only these fixtures.

Files
  algebra.npz   twiddle tables, NTT/INTT, pointwise ops, schoolbook product, matrix product for
                (PRIME, 64), (PRIME, 256) and a few small (q, d) pairs          [SURVEY G1,G2,G4,G5,G8]
  generic.npz   the same for parameters beyond the scheme's: a prime in [2^31, 2^32) at d = 256 / 2048, a prime just below 2^62
                at d = 64 / 1024, the scheme's prime with tables that are no root's powers; int64 arrays
  bulk.json     SHA-256 digests of B=4096 batches (fwd, inv, fwd.square.inv) + sample rows      [G3]
  scheme_128.npz / scheme_256.npz / scheme.json
                end-to-end setup/keygen/sign/aggregate/verify with every intermediate array [G6]
  kat.json      compact replay data extracted from the reference's own reproducible KAT CSVs  [G7]
  reference_tests.json
                the names of the reference's test functions, per test file, in file order (tests/test_reference_case_map.py)
  challenge_edges.npz
                the reference's coefficient rows (hash_vk_and_int_to_bytes + decode_bytes_to_polynomial_coefficients) for the
                fixtures of tests/_challenge_edges.py at the two scheme parameter sets (argument "challenge_edges")
"""
import csv
import hashlib
import json
import os
import re
import sys
import time

import numpy as np

REF = os.environ.get("FUSION_REFERENCE", "/root/reference")
if REF not in sys.path:
    sys.path.insert(0, REF)
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from algebra.matrices import GeneralMatrix  # noqa: E402  (reference)
from algebra.ntt import (bit_reverse_copy, cooley_tukey_ntt, find_primitive_root,  # noqa: E402
                         gentleman_sande_intt, ntt_poly_mult)
from algebra.polynomials import (PolynomialCoefficientRepresentation as PolyC,  # noqa: E402
                                 PolynomialNTTRepresentation as PolyN, transform)
import fusion.fusion as F  # noqa: E402

from oracle.oracle import splitmix_centered  # noqa: E402  (input generator only)

PRIME = 2147465729
sys.setrecursionlimit(10000)
csv.field_size_limit(1 << 30)


def sha_i32(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype="<i4").tobytes()).hexdigest()


def sha_str(s):
    return hashlib.sha256(s.encode("utf-8")).hexdigest()


def edge_rows(d, q):
    h = (q - 1) // 2
    lim_hi, lim_lo = 2 ** 31 - 1, -(2 ** 31)
    rows = [
        [0] * d, [1] + [0] * (d - 1), [0, 1] + [0] * (d - 2), [0] * (d - 1) + [1],
        [h] * d, [-h] * d, [h if j % 2 == 0 else -h for j in range(d)],
        [j - d // 2 for j in range(d)],
        # non-centred int32 inputs: outputs of the reference's __neg__ and raw int32 extremes
        [-(j * ((q - 1) // d)) for j in range(d)], [-(q - 1)] * d,
        [lim_hi] * d, [lim_lo] * d, [lim_hi if j % 3 == 0 else lim_lo for j in range(d)],
    ]
    return rows


def algebra_case(out, tag, q, d, root, n_seeded, rank):
    inv_root = pow(root, q - 2, q)
    tw = bit_reverse_copy([pow(root, i, q) for i in range(d)])
    itw = bit_reverse_copy([pow(inv_root, i, q) for i in range(d)])
    out[f"{tag}_params"] = np.array([q, d, root, inv_root], dtype=np.int64)
    out[f"{tag}_tw"] = np.array(tw, dtype=np.uint32)
    out[f"{tag}_itw"] = np.array(itw, dtype=np.uint32)
    seeded = splitmix_centered(1000 + d + q % 997, n_seeded * d, q).reshape(n_seeded, d)
    if q < PRIME:   # small primes: also exercise arbitrary int32 inputs
        rng = np.random.default_rng(q * 31 + d)
        seeded = np.concatenate([seeded, rng.integers(-2**31, 2**31, size=(4, d), dtype=np.int64).astype(np.int32)])
    rows = edge_rows(d, q) + [[int(v) for v in r] for r in seeded]
    x = np.array(rows, dtype=np.int64)
    assert x.min() >= -2**31 and x.max() < 2**31
    fwd = [cooley_tukey_ntt(list(r), q, 2 * d, tw) for r in rows]
    inv = [gentleman_sande_intt(list(r), q, 2 * d, itw) for r in rows]
    out[f"{tag}_x"] = x.astype(np.int32)
    out[f"{tag}_fwd"] = np.array(fwd, dtype=np.int32)
    out[f"{tag}_inv"] = np.array(inv, dtype=np.int32)

    # pointwise ops through the reference's classes (operands: every row against the next)
    def P(vals):
        return PolyN(modulus=q, degree=d, root=root, inv_root=inv_root, root_order=2 * d, values=list(vals))
    # the all-zero row is never the right operand: `x * zero_poly` returns the int 0 and
    # `x + zero_poly` returns x itself in the reference (polynomials.py:283-284, :342-343); those
    # quirks are covered by object-level tests, not by the kernel vectors
    a_rows, b_rows = rows, rows[1:] + rows[1:2]
    def vals(r):
        return [0] * d if isinstance(r, int) else r.values       # `x * zero_poly` is the int 0
    out[f"{tag}_pw_mul"] = np.array([vals(P(a) * P(b)) for a, b in zip(a_rows, b_rows)], dtype=np.int32)
    out[f"{tag}_pw_add"] = np.array([(P(a) + P(b)).values for a, b in zip(a_rows, b_rows)], dtype=np.int32)
    out[f"{tag}_pw_sub"] = np.array([(P(a) - P(b)).values for a, b in zip(a_rows, b_rows)], dtype=np.int32)
    # rows whose right operand is == 0 mod q: add/sub return the LEFT operand object unchanged there
    out[f"{tag}_pw_b_is_zero"] = np.array([all(v % q == 0 for v in b) for b in b_rows])
    out[f"{tag}_pw_neg"] = np.array([(-P(a)).values for a in a_rows], dtype=np.int64)

    # coefficient-domain schoolbook product == NTT product (G8)
    def C(vals):
        return PolyC(modulus=q, degree=d, root=root, inv_root=inv_root, root_order=2 * d, coefficients=list(vals))
    npair = 4
    f_rows = [[int(v) for v in r] for r in seeded[:npair]]
    g_rows = [[int(v) for v in r] for r in seeded[npair:2 * npair]]
    sb = [(C(f) * C(g)).coefficients for f, g in zip(f_rows, g_rows)]
    viantt = [ntt_poly_mult(list(f), list(g), q, root, inv_root, 2 * d) for f, g in zip(f_rows, g_rows)]
    assert sb == viantt
    out[f"{tag}_sb_f"] = np.array(f_rows, dtype=np.int32)
    out[f"{tag}_sb_g"] = np.array(g_rows, dtype=np.int32)
    out[f"{tag}_sb_fg"] = np.array(sb, dtype=np.int32)

    # (1 x l).(l x 1) through GeneralMatrix (G5)
    if rank:
        A = splitmix_centered(77 + d, rank * d, q).reshape(rank, d)
        S = splitmix_centered(99 + d, 2 * rank * d, q).reshape(2, rank, d)
        outs = []
        for b in range(2):
            Am = GeneralMatrix(matrix=[[P([int(v) for v in A[k]]) for k in range(rank)]])
            Sm = GeneralMatrix(matrix=[[P([int(v) for v in S[b, k]])] for k in range(rank)])
            outs.append((Am * Sm).matrix[0][0].values)
        out[f"{tag}_mv_A"] = A
        out[f"{tag}_mv_S"] = S
        out[f"{tag}_mv_out"] = np.array(outs, dtype=np.int32)


def gen_algebra():
    out = {}
    algebra_case(out, "p128", PRIME, 64, F.ROOT_128, 8, F.RANK_128)
    algebra_case(out, "p256", PRIME, 256, F.ROOT_256, 8, F.RANK_256)
    small = [(5, 2), (17, 8), (97, 16), (257, 64), (7681, 32), (12289, 256), (65537, 128), (40961, 4)]
    tags = []
    for q, d in small:
        root = find_primitive_root(modulus=q, root_order=2 * d)
        tag = f"s{q}_{d}"
        tags.append(tag)
        algebra_case(out, tag, q, d, root, 8, 3)
    out["small_tags"] = np.array(tags)
    np.savez_compressed(os.path.join(HERE, "algebra.npz"), **out)
    print("algebra.npz written:", len(out), "arrays")


# ---- the parameter space beyond the scheme's two sets (round 5's generic paths) -------------------------
# Numbers the REFERENCE produced for: a prime in [2^31, 2^32) at d = 256 and d = 2048 (the int32 kernels' widened range and the
# one-workgroup-per-polynomial kernels), the scheme's prime with tables that are not the powers of any root (contexts built
# from tables), a prime just below 2^62 at d = 64 and d = 1024 (the generic int64 path).  int64 arrays throughout.
Q32 = 4294828033          # 2^32 - 139263 = 1 (mod 8192)
Q62 = 4611686018427322369  # the last prime = 1 (mod 2^15) below 2^62 (tests/test_gpu_wide.py derives the same number)


def _root(q, n):
    for g in range(2, 5000):
        r = pow(g, (q - 1) // (2 * n), q)
        if pow(r, n, q) == q - 1:
            return r
    raise AssertionError("no root")


def generic_case(out, tag, q, d, tw, itw, root, raw32, classes):
    half = (q - 1) // 2
    rng = np.random.default_rng(q % 100003 + d)
    rows = [[0] * d, [half] * d, [-half] * d, [half if j % 2 == 0 else -half for j in range(d)], [1] + [0] * (d - 1)]
    rows += [[int(v) for v in rng.integers(-half, half + 1, size=d)] for _ in range(5)]
    if raw32:             # inputs the int32 kernels accept unreduced
        rows += [[int(v) for v in rng.integers(-2**31, 2**31, size=d)], [2**31 - 1 if j % 2 else -2**31 for j in range(d)]]
    out[f"{tag}_params"] = np.array([q, d, root or 0], dtype=np.int64)
    out[f"{tag}_tw"] = np.array(tw, dtype=np.int64)
    out[f"{tag}_itw"] = np.array(itw, dtype=np.int64)
    out[f"{tag}_x"] = np.array(rows, dtype=np.int64)
    out[f"{tag}_fwd"] = np.array([cooley_tukey_ntt(list(r), q, 2 * d, tw) for r in rows], dtype=np.int64)
    out[f"{tag}_inv"] = np.array([gentleman_sande_intt(list(r), q, 2 * d, itw) for r in rows], dtype=np.int64)
    if not classes:
        return
    inv_root = pow(root, q - 2, q)

    def P(vals):
        return PolyN(modulus=q, degree=d, root=root, inv_root=inv_root, root_order=2 * d, values=list(vals))
    a_rows, b_rows = rows[1:10], rows[2:10] + rows[1:2]          # (never the all-zero row: see algebra_case)
    out[f"{tag}_pw_a"] = np.array(a_rows, dtype=np.int64)
    out[f"{tag}_pw_b"] = np.array(b_rows, dtype=np.int64)
    out[f"{tag}_pw_mul"] = np.array([(P(a) * P(b)).values for a, b in zip(a_rows, b_rows)], dtype=np.int64)
    out[f"{tag}_pw_add"] = np.array([(P(a) + P(b)).values for a, b in zip(a_rows, b_rows)], dtype=np.int64)
    out[f"{tag}_pw_sub"] = np.array([(P(a) - P(b)).values for a, b in zip(a_rows, b_rows)], dtype=np.int64)
    out[f"{tag}_pw_neg"] = np.array([(-P(a)).values for a in a_rows], dtype=np.int64)
    rank = 3
    A = [[int(v) for v in rng.integers(-half, half + 1, size=d)] for _ in range(rank)]
    S = [[[int(v) for v in rng.integers(-half, half + 1, size=d)] for _ in range(rank)] for _ in range(2)]
    outs = []
    for b in range(2):
        Am = GeneralMatrix(matrix=[[P(A[k]) for k in range(rank)]])
        Sm = GeneralMatrix(matrix=[[P(S[b][k])] for k in range(rank)])
        outs.append((Am * Sm).matrix[0][0].values)
    out[f"{tag}_mv_A"] = np.array(A, dtype=np.int64)
    out[f"{tag}_mv_S"] = np.array(S, dtype=np.int64)
    out[f"{tag}_mv_out"] = np.array(outs, dtype=np.int64)
    # transform() both ways through the classes (the constructor checks run on these parameters too)
    c = PolyC(modulus=q, degree=d, root=root, inv_root=inv_root, root_order=2 * d, coefficients=list(rows[5]))
    ch = transform(c)
    assert ch.values == [int(v) for v in out[f"{tag}_fwd"][5]] and transform(ch).coefficients == rows[5]


def gen_generic():
    out, tags = {}, []
    t0 = time.time()
    for q, d, raw32 in ((Q32, 256, True), (Q32, 2048, True), (Q62, 64, False), (Q62, 1024, False)):
        root = _root(q, d)
        inv_root = pow(root, q - 2, q)
        tw = bit_reverse_copy([pow(root, i, q) for i in range(d)])
        itw = bit_reverse_copy([pow(inv_root, i, q) for i in range(d)])
        tag = f"g{q}_{d}"
        tags.append(tag)
        generic_case(out, tag, q, d, tw, itw, root, raw32, True)
        print(tag, "done", round(time.time() - t0, 1), "s", flush=True)
    for d in (64, 256):                                   # the scheme's prime, tables that are no root's powers
        rng = np.random.default_rng(4242 + d)
        tw = [int(v) for v in rng.integers(0, PRIME, size=d)]
        itw = [int(v) for v in rng.integers(0, PRIME, size=d)]
        tag = f"t{PRIME}_{d}"
        tags.append(tag)
        generic_case(out, tag, PRIME, d, tw, itw, None, True, False)
    out["tags"] = np.array(tags)
    np.savez_compressed(os.path.join(HERE, "generic.npz"), **out)
    print("generic.npz written:", len(out), "arrays")


def gen_bulk():
    res = {"generator": "oracle.oracle.splitmix_centered(seed=20261003, count=B*d)", "B": 4096, "cases": {}}
    for secpar, d, root in ((128, 64, F.ROOT_128), (256, 256, F.ROOT_256)):
        q = PRIME
        inv_root = pow(root, q - 2, q)
        tw = bit_reverse_copy([pow(root, i, q) for i in range(d)])
        itw = bit_reverse_copy([pow(inv_root, i, q) for i in range(d)])
        B = 4096
        x = splitmix_centered(20261003, B * d, q).reshape(B, d)
        t0 = time.time()
        fwd = np.array([cooley_tukey_ntt([int(v) for v in r], q, 2 * d, tw) for r in x], dtype=np.int32)
        inv = np.array([gentleman_sande_intt([int(v) for v in r], q, 2 * d, itw) for r in x], dtype=np.int32)
        half, logmod = q // 2, q.bit_length() - 1
        sq = [[F.PolynomialNTTRepresentation.__mul__.__globals__["cent"](int(v) * int(v), q, half, logmod) for v in r] for r in fwd]
        conv = np.array([gentleman_sande_intt(r, q, 2 * d, itw) for r in sq], dtype=np.int32)
        back = np.array([gentleman_sande_intt([int(v) for v in r], q, 2 * d, itw) for r in fwd], dtype=np.int32)
        assert np.array_equal(back, x)
        res["cases"][str(secpar)] = {
            "q": q, "d": d, "root": root, "inv_root": inv_root,
            "sha256_input": sha_i32(x), "sha256_fwd": sha_i32(fwd), "sha256_inv": sha_i32(inv),
            "sha256_fwd_square_inv": sha_i32(conv),
            "rows": {str(i): {"fwd": fwd[i].tolist(), "inv": inv[i].tolist(), "fwd_square_inv": conv[i].tolist()}
                     for i in (0, 1, 4095)},
        }
        print(f"bulk secpar={secpar}: {time.time()-t0:.1f}s")
    with open(os.path.join(HERE, "bulk.json"), "w") as f:
        json.dump(res, f)


def mat_values(m):
    """GeneralMatrix of NTT polys -> int32 array [rows*cols][d] (the scheme only uses vectors)."""
    return np.array([z.values for y in m.matrix for z in y], dtype=np.int32)


def gen_scheme():
    meta = {}
    for secpar, setup_seed, nkeys in ((128, 42, 4), (256, 2026, 4)):
        t0 = time.time()
        params = F.fusion_setup(secpar, setup_seed)
        d, l, q = params.degree, params.num_rows_sk, params.modulus
        A = mat_values(params.public_challenge)
        key_seeds = [1000 * secpar + 17 * i for i in range(nkeys)]
        msgs = [f"message number {i:04d} !!" for i in range(nkeys)]
        keys = [F.keygen(params, s) for s in key_seeds]
        coef = []
        for s in key_seeds:
            halves = []
            for sd in (s, s + 1):
                m = F.sample_coefficient_matrix(seed=sd, modulus=q, degree=d, root_order=params.root_order,
                                                root=params.root, inv_root=params.inv_root, num_rows=l, num_cols=1,
                                                norm_bound=params.beta_sk, weight_bound=params.omega_sk)
                halves.append(np.array([z.coefficients for y in m.matrix for z in y], dtype=np.int32))
            coef.append(np.stack(halves))
        coef = np.stack(coef)                                   # [N][2][l][d]
        sk_hat = np.stack([np.stack([mat_values(sk.left_sk_hat), mat_values(sk.right_sk_hat)]) for sk, _ in keys])
        vk = np.stack([np.stack([mat_values(v.left_vk_hat)[0], mat_values(v.right_vk_hat)[0]]) for _, v in keys])
        vks = [k[1] for k in keys]
        prehash = [F.hash_message_to_int(params, m) for m in msgs]
        challs = [F.hash_ch(params, v, m) for v, m in zip(vks, msgs)]
        c_hat = np.array([c.c_hat.values for c in challs], dtype=np.int32)
        sigs = [F.sign(params, k, m) for k, m in zip(keys, msgs)]
        sig = np.stack([mat_values(s.signature_hat) for s in sigs])      # [N][l][d]
        arrays = dict(A=A, coef=coef, sk_hat=sk_hat, vk=vk, c_hat=c_hat, sig=sig)
        info = dict(secpar=secpar, setup_seed=setup_seed, key_seeds=key_seeds, messages=msgs,
                    prehash=[str(p) for p in prehash],
                    sha256_str_params=sha_str(str(params)),
                    sha256_str_vk=[sha_str(str(v)) for v in vks],
                    sha256_str_sk=[sha_str(str(k[0])) for k in keys],
                    sha256_str_sig=[sha_str(str(s)) for s in sigs],
                    sha256_str_chall=[sha_str(str(c)) for c in challs],
                    beta_vf=params.beta_vf, omega_vf=params.omega_vf, capacity=params.capacity, agg={})
        for n in (1, 2, 4):
            sub_v, sub_m, sub_s = vks[:n], msgs[:n], sigs[:n]
            order = sorted(range(n), key=lambda i: str(sub_v[i]))
            alphas = F.hash_ag(params, [sub_v[i] for i in order], [sub_m[i] for i in order])
            agg = F.aggregate(params, sub_v, sub_m, sub_s)
            verdict = F.verify(params, sub_v, sub_m, agg)
            assert verdict == (True, ""), verdict
            arrays[f"alpha_hat_{n}"] = np.array([a.alpha_hat.values for a in alphas], dtype=np.int32)
            arrays[f"agg_{n}"] = mat_values(agg.signature_hat)
            # tamper exactly like tests/test_fusion.py:860-873 does (flip one value)
            agg.signature_hat.matrix[0][0].values[0] += 1
            bad = F.verify(params, sub_v, sub_m, agg)
            agg.signature_hat.matrix[0][0].values[0] -= 1
            info["agg"][str(n)] = dict(order=order, sha256_str_agg=sha_str(str(agg)), verdict=list(verdict),
                                       tampered_verdict=list(bad))
        # norm failure: an "aggregate" with a huge coefficient but consistent target cannot be built
        # from the reference flow; norm/weight branches are covered at the algebra level instead.
        np.savez_compressed(os.path.join(HERE, f"scheme_{secpar}.npz"), **arrays)
        meta[str(secpar)] = info
        print(f"scheme secpar={secpar}: {time.time()-t0:.1f}s")

    # BASELINE config 1 / misc/demo.py flow: secpar=128, 2 keys from the SAME seed
    params = F.fusion_setup(128, 42)
    keys = [F.keygen(params, 42) for _ in range(2)]
    msgs = ["first demo message 01", "second demo message 2"]
    sigs = [F.sign(params, k, m) for k, m in zip(keys, msgs)]
    vks = [k[1] for k in keys]
    agg = F.aggregate(params, vks, msgs, sigs)
    meta["demo128"] = dict(setup_seed=42, key_seed=42, messages=msgs,
                           sha256_str_sig=[sha_str(str(s)) for s in sigs], sha256_str_agg=sha_str(str(agg)),
                           verdict=list(F.verify(params, vks, msgs, agg)))
    with open(os.path.join(HERE, "scheme.json"), "w") as f:
        json.dump(meta, f)


def gen_scheme_many():
    """Many DISTINCT signers (VERDICT r02 task 2a): the reference's whole flow for N = 32 keys at secpar 128 and
    N = 16 at secpar 256 -- everything that depends on the ORDER of many keys (sorted(key=str(vk)) on signed decimals,
    the hash_ag text over N tuples, the aggregation coefficients in sorted order) -- plus nested sub-aggregates of
    mixed sizes (a many-aggregates call) and the tamper verdicts.  Signatures and keys are stored as digests (they are
    regenerated from the seeds by the build and compared by SHA-256); alpha_hat, aggregates and orders are stored whole."""
    meta = {}
    for secpar, setup_seed, nkeys, subsets in ((128, 4242, 32, ((0, 32), (0, 5), (5, 17), (17, 32))),
                                               (256, 777, 16, ((0, 16), (0, 3), (3, 9), (9, 16)))):
        t0 = time.time()
        params = F.fusion_setup(secpar, setup_seed)
        key_seeds = [31337 * secpar + 1009 * i * i + 7 * i for i in range(nkeys)]
        msgs = [f"signer {i}: pay {100 + 13 * i} units to account #{(i * 7919) % 1000:03d}" for i in range(nkeys)]
        keys = [F.keygen(params, s) for s in key_seeds]
        vks = [k[1] for k in keys]
        sigs = [F.sign(params, k, m) for k, m in zip(keys, msgs)]
        vk = np.stack([np.stack([mat_values(v.left_vk_hat)[0], mat_values(v.right_vk_hat)[0]]) for v in vks])
        sig = np.stack([mat_values(s.signature_hat) for s in sigs])
        arrays = dict(vk=vk, A=mat_values(params.public_challenge))
        info = dict(secpar=secpar, setup_seed=setup_seed, key_seeds=key_seeds, messages=msgs,
                    sha256_sig_rows=[sha_i32(s) for s in sig], sha256_str_vk=[sha_str(str(v)) for v in vks],
                    sha256_str_sig=[sha_str(str(s)) for s in sigs], subsets=[list(s) for s in subsets], agg={})
        for lo, hi in subsets:
            sub_v, sub_m, sub_s = vks[lo:hi], msgs[lo:hi], sigs[lo:hi]
            n = hi - lo
            order = sorted(range(n), key=lambda i: str(sub_v[i]))
            alphas = F.hash_ag(params, [sub_v[i] for i in order], [sub_m[i] for i in order])
            agg = F.aggregate(params, sub_v, sub_m, sub_s)
            verdict = F.verify(params, sub_v, sub_m, agg)
            assert verdict == (True, ""), verdict
            tag = f"{lo}_{hi}"
            arrays[f"alpha_hat_sorted_{tag}"] = np.array([a.alpha_hat.values for a in alphas], dtype=np.int32)
            arrays[f"agg_{tag}"] = mat_values(agg.signature_hat)
            agg.signature_hat.matrix[n % params.num_rows_sk][0].values[3] += 1
            bad = F.verify(params, sub_v, sub_m, agg)
            agg.signature_hat.matrix[n % params.num_rows_sk][0].values[3] -= 1
            swapped = list(sub_m)
            swapped[0], swapped[-1] = swapped[-1], swapped[0]
            info["agg"][tag] = dict(order=order, sha256_str_agg=sha_str(str(agg)), verdict=list(verdict),
                                    tampered_verdict=list(bad), tampered_at=[n % params.num_rows_sk, 3],
                                    swapped_messages_verdict=list(F.verify(params, sub_v, swapped, agg)) if n > 1 else None)
        np.savez_compressed(os.path.join(HERE, f"scheme_many_{secpar}.npz"), **arrays)
        meta[str(secpar)] = info
        print(f"scheme_many secpar={secpar}: {nkeys} signers, {time.time()-t0:.1f}s")
    with open(os.path.join(HERE, "scheme_many.json"), "w") as f:
        json.dump(meta, f)


def _full_worker(job):
    """one process of gen_scheme_full: the reference's keygen + sign for a block of signers -> (vk rows, signature rows)"""
    secpar, setup_seed, seeds, msgs = job
    params = F.fusion_setup(secpar, setup_seed)
    vks, sigs = [], []
    for s_, m_ in zip(seeds, msgs):
        k = F.keygen(params, s_)
        vks.append(np.stack([mat_values(k[1].left_vk_hat)[0], mat_values(k[1].right_vk_hat)[0]]))
        sigs.append(mat_values(F.sign(params, k, m_).signature_hat))
    return np.stack(vks), np.stack(sigs)


def gen_scheme_full(secpar=256, n=1024, setup_seed=31415, procs=8, tag=None):
    """BASELINE configs[3] AT ITS STATED SIZE through the reference: 1024 distinct signers at secpar 256 -- keygen and sign in
    `procs` processes (the reference is single-threaded: ~0.8 s per signer), then ONE aggregate() and ONE verify() over all of
    them.  Stored: the sorted order, SHA-256 of every verification key / signature row (the build regenerates them from the
    seeds), SHA-256 of the aggregation coefficients in sorted order, the aggregate itself, verdict and tamper verdict."""
    from multiprocessing import Pool
    t0 = time.time()
    seeds = [7_000_003 + 104_729 * i for i in range(n)]
    msgs = [f"transfer #{i:05d}: {1000 + (i * 37) % 9000} units" for i in range(n)]
    blocks = [(secpar, setup_seed, seeds[i::procs], msgs[i::procs]) for i in range(procs)]
    with Pool(procs) as pool:
        parts = pool.map(_full_worker, blocks)
    vk = np.empty((n, 2, parts[0][0].shape[-1]), dtype=np.int32)
    sig = np.empty((n,) + parts[0][1].shape[1:], dtype=np.int32)
    for i, (v_, s_) in enumerate(parts):
        vk[i::procs], sig[i::procs] = v_, s_
    print(f"scheme_full: {n} keygen + sign in {time.time() - t0:.0f} s")
    params = F.fusion_setup(secpar, setup_seed)

    def poly(v):
        return PolyN(modulus=params.modulus, degree=params.degree, root=params.root, inv_root=params.inv_root,
                     root_order=params.root_order, values=[int(x) for x in v])
    first = poly(vk[0, 0])

    def like(v):                    # the reference re-proves the primitive root in every constructor: clone instead
        import copy
        z = copy.copy(first)
        z.values = [int(x) for x in v]
        return z
    vks = [F.OneTimeVerificationKey(left_vk_hat=GeneralMatrix(matrix=[[like(vk[i, 0])]]),
                                    right_vk_hat=GeneralMatrix(matrix=[[like(vk[i, 1])]])) for i in range(n)]
    sigs = [F.Signature(signature_hat=GeneralMatrix(matrix=[[like(r)] for r in sig[i]])) for i in range(n)]
    order = sorted(range(n), key=lambda i: str(vks[i]))
    t1 = time.time()
    alphas = F.hash_ag(params, [vks[i] for i in order], [msgs[i] for i in order])
    agg = F.aggregate(params, vks, msgs, sigs)
    print(f"scheme_full: hash_ag + aggregate in {time.time() - t1:.0f} s")
    t1 = time.time()
    verdict = F.verify(params, vks, msgs, agg)
    assert verdict == (True, ""), verdict
    agg.signature_hat.matrix[11][0].values[7] += 1
    bad = F.verify(params, vks, msgs, agg)
    agg.signature_hat.matrix[11][0].values[7] -= 1
    print(f"scheme_full: 2 x verify in {time.time() - t1:.0f} s")
    alpha_sorted = np.array([a.alpha_hat.values for a in alphas], dtype=np.int32)
    tag = tag or str(secpar)
    np.savez_compressed(os.path.join(HERE, f"scheme_full_{tag}.npz"), agg=mat_values(agg.signature_hat),
                        order=np.array(order, dtype=np.int32))
    meta_path = os.path.join(HERE, "scheme_full.json")
    meta = json.load(open(meta_path)) if os.path.exists(meta_path) else {}
    too_many = None
    if n == params.capacity:                    # one signer more than the capacity: the reference refuses before any arithmetic
        too_many = list(F.verify(params, vks + [vks[0]], msgs + [msgs[0]], agg))
    with open(meta_path, "w") as f:
        json.dump({**meta, tag: dict(too_many_verdict=too_many, capacity=params.capacity, secpar=secpar, setup_seed=setup_seed, n=n, key_seeds=seeds, messages=msgs,
                                     sha256_vk=sha_i32(vk), sha256_sig=sha_i32(sig), sha256_sig_rows_first8=[sha_i32(r) for r in sig[:8]],
                                     sha256_alpha_hat_sorted=sha_i32(alpha_sorted), verdict=list(verdict), tampered_verdict=list(bad),
                                     tampered_at=[11, 7], sha256_str_agg=sha_str(str(agg)))}, f)
    print(f"scheme_full secpar={secpar}: {n} signers, {time.time() - t0:.0f} s in all")


def gen_kat_flow(seed=20261004, sigs=8):
    """VERDICT r02 task 2b: SHA-256 of every row (`str(inputs)`, `str(outputs)`) the flow of the reference's
    KATs/generate_KAT_values.py:36-147 produces, run through the REFERENCE's functions in the reference's order, with
    the seeds drawn from random.Random(seed) in the order tools/generate_kat_values.py draws them (the reference's
    script draws from the process-global generator, which its own samplers re-seed: not reproducible by design)."""
    import random
    from math import ceil, log2
    rng = random.Random(seed)
    out = {"seed": seed, "sigs": sigs, "rows": {}}

    def put(name, secpar, inputs, outputs):
        out["rows"].setdefault(f"{name}_KAT_{secpar}", []).append([sha_str(str(inputs)), sha_str(str(outputs))])
    for secpar in (128, 256):
        t0 = time.time()
        seed_a = rng.randint(0, 2**32 - 1)
        params = F.fusion_setup(secpar, seed_a)
        put("fusion_setup", secpar, (secpar, seed_a), params)
        seeds, msgs, otks, pre, challs, sgs = [], [], [], [], [], []
        for i in range(sigs):
            seeds.append(rng.randint(0, 2**32 - 1))
            msgs.append(str(i))
            otks.append(F.keygen(params, seeds[i]))
            put("fusion_keygen", secpar, (params, seeds[i]), otks[-1])
            vk = otks[i][1]
            pre.append(F.hash_message_to_int(params, msgs[i]))
            put("intermediate_hash_message_to_int", secpar, (params, msgs[i]), pre[-1])
            num_coefs = max(0, min(params.degree, params.omega_ch))
            bound = max(0, min(params.modulus // 2, params.beta_ch))
            n = ceil(params.omega_ch / 8) + ceil((log2(bound) + 1 + params.secpar) / 8) * num_coefs + \
                params.degree * ceil((log2(params.degree) + params.secpar) / 8)
            put("intermediate_hash_vk_and_int_to_bytes_to_int", secpar, (params, vk, pre[i], n),
                F.hash_vk_and_int_to_bytes(params, vk, pre[i], n))
            challs.append(F.hash_ch(params, vk, msgs[i]))
            put("intermediate_hash_ch", secpar, (params, vk, msgs[i]), challs[-1])
            sgs.append(F.sign(params, otks[i], msgs[i]))
            put("fusion_sign", secpar, (params, otks[i], pre[i]), sgs[-1])
        vks = [k[1] for k in otks]
        # the reference's script passes the (sk, vk) TUPLES to these two (generate_KAT_values.py:115, :127)
        put("intermediate_hash_vks_and_ints_and_challs_to_bytes", secpar, (params, otks, pre, challs),
            F.hash_vks_and_ints_and_challs_to_bytes(params, otks, pre, challs))
        put("intermediate_hash_ag", secpar, (params, otks, msgs), F.hash_ag(params, otks, msgs))
        agg = F.aggregate(params, vks, msgs, sgs)
        put("fusion_aggregate", secpar, (params, vks, msgs, sgs), agg)
        assert F.verify(params, vks, msgs, agg) == (True, "")
        print(f"kat_flow secpar={secpar}: {time.time()-t0:.1f}s")
    with open(os.path.join(HERE, "kat_flow.json"), "w") as f:
        json.dump(out, f)


_VAL = re.compile(r"values=\[([^\]]*)\]")


def _lists(s):
    return [[int(t) for t in m.split(",")] for m in _VAL.findall(s)]


def gen_kat():
    """Compact replay data from the reference's reproducible KAT CSVs (KATs/KAT_values)."""
    kdir = os.path.join(REF, "KATs", "KAT_values")
    out = {"source": "KATs/KAT_values/*.csv of the reference checkout", "setup": [], "hash_message_to_int": [],
           "hash_vk_and_int_to_bytes": [], "hash_ch": []}
    for secpar in (128, 256):
        with open(os.path.join(kdir, f"fusion_setup_KAT_{secpar}.csv"), newline="") as f:
            for inp, exp in csv.reader(f):
                sp, seed = eval(inp)
                assert str(F.fusion_setup(sp, seed)) == exp          # reproduces from the reference
                lists = _lists(exp)
                out["setup"].append(dict(secpar=sp, seed=seed, sha256_str_params=sha_str(exp),
                                         first_poly=lists[0], n_polys=len(lists)))
    with open(os.path.join(kdir, "intermediate_hash_message_to_int_KAT_128.csv"), newline="") as f:
        for inp, exp in csv.reader(f):
            msg = re.search(r", '([^']*)'\)$", inp).group(1)
            out["hash_message_to_int"].append(dict(secpar=128, message=msg, expected=exp))
    with open(os.path.join(kdir, "intermediate_hash_vk_and_int_to_bytes_to_int_KAT_128.csv"), newline="") as f:
        for inp, exp in csv.reader(f):
            m = re.search(r"\), (\d+), (\d+)\)$", inp)
            lists = _lists(inp)
            out["hash_vk_and_int_to_bytes"].append(dict(secpar=128, vk_left=lists[-2], vk_right=lists[-1],
                                                        i=m.group(1), n=int(m.group(2)),
                                                        sha256_expected_bytes=hashlib.sha256(eval(exp)).hexdigest()))
    with open(os.path.join(kdir, "intermediate_hash_ch_KAT_128.csv"), newline="") as f:
        for inp, exp in csv.reader(f):
            msg = re.search(r", '([^']*)'\)$", inp).group(1)
            lists = _lists(inp)
            out["hash_ch"].append(dict(secpar=128, vk_left=lists[-2], vk_right=lists[-1], message=msg,
                                       c_hat=_lists(exp)[0]))
    # replay all three through the reference to make sure the extraction is faithful
    params = F.fusion_setup(128, 1)
    for row in out["hash_message_to_int"]:
        assert str(F.hash_message_to_int(params, row["message"])) == row["expected"]

    def mkvk(row):
        def P(v):
            return PolyN(modulus=params.modulus, degree=params.degree, root=params.root, inv_root=params.inv_root,
                         root_order=params.root_order, values=list(v))
        return F.OneTimeVerificationKey(left_vk_hat=GeneralMatrix(matrix=[[P(row["vk_left"])]]),
                                        right_vk_hat=GeneralMatrix(matrix=[[P(row["vk_right"])]]))
    for row in out["hash_vk_and_int_to_bytes"]:
        b = F.hash_vk_and_int_to_bytes(params, mkvk(row), int(row["i"]), row["n"])
        assert hashlib.sha256(b).hexdigest() == row["sha256_expected_bytes"]
    for row in out["hash_ch"]:
        assert F.hash_ch(params, mkvk(row), row["message"]).c_hat.values == row["c_hat"]
    out["note"] = ("fusion_aggregate_KAT_128.csv does not reproduce from the current reference code "
                   "(stale; SURVEY.md 8c) and is therefore not replayed; 12 further KAT files are absent "
                   "from the checkout (.MISSING_LARGE_BLOBS).")
    with open(os.path.join(HERE, "kat.json"), "w") as f:
        json.dump(out, f)
    print("kat.json written:", {k: len(v) for k, v in out.items() if isinstance(v, list)})


def gen_reference_tests():
    """the names only (`def test_...(` at the start of a line), per file of the reference's tests/, in file order"""
    out = {}
    for name in sorted(os.listdir(os.path.join(REF, "tests"))):
        if name.startswith("test_") and name.endswith(".py"):
            with open(os.path.join(REF, "tests", name)) as fh:
                out["tests/" + name] = re.findall(r"^def (test_\w+)\(", fh.read(), flags=re.M)
    with open(os.path.join(HERE, "reference_tests.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("reference_tests.json written:", {k: len(v) for k, v in out.items()})


def gen_challenge_edges():
    """tests/_challenge_edges.py's key / digest fixtures and message fixtures through the reference's own functions: the rows
    before the transform (ternary: int8), and a SHA-256 of the fixture arrays so that a changed builder cannot meet stale rows"""
    sys.path.insert(0, os.path.dirname(HERE))
    import _challenge_edges as E
    out = {}
    for name in E.SCHEME_SETS:
        ps = E.SETS[name]
        params = F.fusion_setup(ps.secpar, 1)
        assert (params.degree, params.omega_ch, params.root, params.sign_hash_dst) == (ps.degree, ps.omega_ch, ps.root, ps.sign_hash_dst)
        sb, cb, ib = E.decode_shape(ps)
        n = sb + cb * min(ps.degree, ps.omega_ch) + ps.degree * ib           # as hash_ch asks for

        def key_of(vk):
            def P(v):
                return PolyN(modulus=params.modulus, degree=params.degree, root=params.root, inv_root=params.inv_root,
                             root_order=params.root_order, values=[int(t) for t in v])
            return F.OneTimeVerificationKey(left_vk_hat=GeneralMatrix(matrix=[[P(vk[0])]]),
                                            right_vk_hat=GeneralMatrix(matrix=[[P(vk[1])]]))

        def row_of(vk, i):
            b = F.hash_vk_and_int_to_bytes(params, key_of(vk), i, n)
            return F.decode_bytes_to_polynomial_coefficients(b, params.secpar, params.modulus, params.degree, params.beta_ch,
                                                             params.omega_ch)
        fx = E.fixtures(name)
        rows = np.array([row_of(fx.vk[k], fx.ints[k]) for k in range(len(fx))], dtype=np.int64)
        mvk = E.message_keys(ps)
        msgs = [m for _, m in E.message_fixtures()]
        mrows = np.array([row_of(mvk[k], F.hash_message_to_int(params, m)) for k, m in enumerate(msgs)], dtype=np.int64)
        assert np.abs(rows).max() <= 1 and np.abs(mrows).max() <= 1
        out[f"rows_{name}"] = rows.astype(np.int8)
        out[f"message_rows_{name}"] = mrows.astype(np.int8)
        out[f"fixtures_sha256_{name}"] = np.array(fx.sha256())
        out[f"messages_sha256_{name}"] = np.array(E.messages_sha256(ps))
    np.savez_compressed(os.path.join(HERE, "challenge_edges.npz"), **out)
    print("challenge_edges.npz written:", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    which = sys.argv[1:] or ["algebra", "bulk", "scheme", "kat", "many", "kat_flow", "reference_tests"]
    if "full" in sys.argv[1:]:                  # ~5 minutes on 8 cores: only on request
        gen_scheme_full()
    if "full128" in sys.argv[1:]:               # secpar 128 AT ITS CAPACITY (1796 signers, fusion.py:24)
        gen_scheme_full(secpar=128, n=1796, setup_seed=27182)
    if "full256cap" in sys.argv[1:]:            # secpar 256 AT ITS CAPACITY (2818 signers, fusion.py:25): ~15 minutes
        gen_scheme_full(secpar=256, n=2818, setup_seed=16180, tag="256cap")
    if "many" in which:
        gen_scheme_many()
    if "kat_flow" in which:
        gen_kat_flow()
    if "algebra" in which:
        gen_algebra()
    if "generic" in which:
        gen_generic()
    if "bulk" in which:
        gen_bulk()
    if "scheme" in which:
        gen_scheme()
    if "kat" in which:
        gen_kat()
    if "reference_tests" in which:
        gen_reference_tests()
    if "challenge_edges" in which:
        gen_challenge_edges()
