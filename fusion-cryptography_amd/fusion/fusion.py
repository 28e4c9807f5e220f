"""Drop-in for the reference's ``fusion.fusion``: the same parameter tables, key / signature
types and the ``fusion_setup / keygen / sign / aggregate / verify`` surface, with the algebra
executed by the fused MI355X cores of libfusion_hip.so.

Reference surface mirrored (file:line in the reference checkout):
  constants & PREFIX_PARAMETERS :16-141 · sample_coefficient_matrix :144 · sample_ntt_matrix :176 ·
  Params :204 · fusion_setup :294 · OneTimeSigningKey :298 · OneTimeVerificationKey :320 ·
  keygen :338 · SignatureChallenge :376 · Signature :392 · hash_message_to_int :405 ·
  hash_vk_and_int_to_bytes :412 · decode_bytes_to_polynomial_coefficients :422 · parse_challenge :484 ·
  hash_ch :511 · sign :534 · AggregationCoefficient :560 · hash_vks_and_ints_and_challs_to_bytes :573 ·
  decode_bytes_to_agg_coefs :594 · hash_ag :632 · aggregate :655 · verify :680

What runs where
  * host (Python stdlib, byte-for-byte the reference's formats): seeding/sampling with ``random``,
    SHA3-256 / SHAKE-256 over ``str()`` of the key objects, the byte -> sparse-ternary decoder.
  * device: every NTT/INTT and all ring arithmetic -- keygen (NTT of 2*rank rows + two
    matrix-vector products) = fz_keygen_core, sign = fz_sign_core, aggregate = fz_aggregate_core,
    verify = fz_verify_core (target sum, A.sigma, rank INTTs, norm/weight, verdict).
"""
from hashlib import sha3_256, shake_256
from math import ceil, log2
from typing import List, Optional, Tuple

import numpy as np

from algebra import _backend
from fusion_hip import hostpipe
from algebra.matrices import GeneralMatrix
from algebra.polynomials import (PolynomialCoefficientRepresentation, PolynomialNTTRepresentation, _check_transformable,
                                 sample_polynomial_coefficient_representation,
                                 sample_polynomial_ntt_representation, transform)
from fusion_hip import VERDICT_REASONS

# Toy prototype of a research scheme, like the reference: not for production use.

PREFIX_PARAMETERS: dict = {}
PRIME: int = 2147465729
DEGREE_128: int = 2 ** 6
DEGREE_256: int = 2 ** 8
ROOT_ORDER_128: int = 2 * DEGREE_128
ROOT_ORDER_256: int = 2 * DEGREE_256
RANK_128: int = 195
RANK_256: int = 83
CAPACITY_128: int = 1796
CAPACITY_256: int = 2818
CH_WEIGHT_128: int = 27
CH_WEIGHT_256: int = 60
AG_WEIGHT_128: int = 35
AG_WEIGHT_256: int = 60
SK_BD_128: int = 52
SK_BD_256: int = 52
CH_BD_128: int = 3
CH_BD_256: int = 1
AG_BD_128: int = 2
AG_BD_256: int = 1
ROOT_128: int = 23584283
ROOT_256: int = 3337519
# two-byte domain-separation tags: (security level id, usage id)
SIGN_PRE_HASH_DST_128: bytes = bytes([1, 0])
SIGN_PRE_HASH_DST_256: bytes = bytes([3, 0])
SIGN_HASH_DST_128: bytes = bytes([1, 1])
SIGN_HASH_DST_256: bytes = bytes([3, 1])
AGG_XOF_DST_128: bytes = bytes([1, 2])
AGG_XOF_DST_256: bytes = bytes([3, 2])

VF_BD_INTERMEDIATE_128: int = SK_BD_128 * (1 + min(DEGREE_128, CH_WEIGHT_128) * CH_BD_128)
VF_BD_INTERMEDIATE_256: int = SK_BD_256 * (1 + min(DEGREE_256, CH_WEIGHT_256) * CH_BD_256)
VF_BD_128: int = CAPACITY_128 * min(DEGREE_128, AG_WEIGHT_128) * AG_BD_128 * VF_BD_INTERMEDIATE_128
VF_BD_256: int = CAPACITY_256 * min(DEGREE_256, AG_WEIGHT_256) * AG_BD_256 * VF_BD_INTERMEDIATE_256


def _parameter_set(capacity, degree, root, rank, dsts, ch_weight, ag_weight, sk_bd, vf_bd):
    return {
        "capacity": capacity, "modulus": PRIME, "degree": degree, "root_order": 2 * degree, "root": root,
        "inv_root": pow(root, PRIME - 2, PRIME),
        "num_rows_pub_challenge": 1, "num_rows_sk": rank, "num_rows_vk": 1,
        "num_cols_pub_challenge": rank, "num_cols_sk": 1, "num_cols_vk": 1,
        "sign_pre_hash_dst": dsts[0], "sign_hash_dst": dsts[1], "agg_xof_dst": dsts[2],
        # the live challenge / aggregation-coefficient bounds are 1 for both sets (fusion.py:88-89, :114-115)
        "beta_sk": sk_bd, "beta_ch": 1, "beta_ag": 1,
        "omega_sk": degree, "omega_ch": ch_weight, "omega_ag": ag_weight,
        "beta_vf": vf_bd, "omega_vf": degree,
    }


PREFIX_PARAMETERS[128] = _parameter_set(CAPACITY_128, DEGREE_128, ROOT_128, RANK_128,
                                        (SIGN_PRE_HASH_DST_128, SIGN_HASH_DST_128, AGG_XOF_DST_128),
                                        CH_WEIGHT_128, AG_WEIGHT_128, SK_BD_128, VF_BD_128)
PREFIX_PARAMETERS[256] = _parameter_set(CAPACITY_256, DEGREE_256, ROOT_256, RANK_256,
                                        (SIGN_PRE_HASH_DST_256, SIGN_HASH_DST_256, AGG_XOF_DST_256),
                                        CH_WEIGHT_256, AG_WEIGHT_256, SK_BD_256, VF_BD_256)

for _secpar, _set in PREFIX_PARAMETERS.items():
    # XOF byte budgets (fusion.py:123-141): a coefficient needs its bits plus `secpar` bias bits
    _set["bytes_for_one_coef_bdd_by_beta_ch"] = ceil(ceil(log2(2 * _set["beta_ch"] + 1) / 8) + _secpar / 8)
    _set["bytes_for_one_coef_bdd_by_beta_ag"] = ceil(ceil(log2(2 * _set["beta_ag"] + 1) / 8) + _secpar / 8)
    _set["bytes_for_poly_shuffle"] = _set["degree"] * ceil(ceil(log2(_set["degree"]) / 8) + _secpar / 8)

_PARAM_FIELDS = ("capacity", "modulus", "degree", "root_order", "root", "inv_root", "num_rows_pub_challenge",
                 "num_rows_sk", "num_rows_vk", "num_cols_pub_challenge", "num_cols_sk", "num_cols_vk",
                 "sign_pre_hash_dst", "sign_hash_dst", "agg_xof_dst", "bytes_for_one_coef_bdd_by_beta_ch",
                 "bytes_for_one_coef_bdd_by_beta_ag", "bytes_for_poly_shuffle", "beta_sk", "beta_ch", "beta_ag",
                 "beta_vf", "omega_sk", "omega_ch", "omega_ag", "omega_vf")


def _replicated(sample_one, num_rows: int, num_cols: int, seed) -> list:
    """num_rows x num_cols entries from a sampler that is re-seeded on every call.  With a seed every call returns
    the same polynomial and leaves the process-global `random` in the same state, so one call plus fresh copies
    (the entries must stay independent objects: callers mutate them) is indistinguishable from num_rows * num_cols
    calls -- and 166x cheaper for a secret key.  Without a seed every entry is a fresh draw, as in the reference."""
    if seed is None or num_rows * num_cols <= 1:
        return [[sample_one() for _ in range(num_cols)] for _ in range(num_rows)]
    first = sample_one()
    data = first._data()
    if all(_backend.INT32_MIN <= v <= _backend.INT32_MAX for v in data):
        row = np.array(data, dtype=np.int32)      # the copies share this row until somebody asks one of them for its list
        return [[first if (i == 0 and j == 0) else first._like_arr(row) for j in range(num_cols)] for i in range(num_rows)]
    # (a modulus the kernels do not implement: plain copies of the list, as before)
    return [[first if (i == 0 and j == 0) else first._like(list(data)) for j in range(num_cols)] for i in range(num_rows)]


def sample_coefficient_matrix(seed: Optional[int], modulus: int, degree: int, root_order: int, root: int,
                              inv_root: int, num_rows: int, num_cols: int, norm_bound: int,
                              weight_bound: int) -> GeneralMatrix:
    """Every entry is sampled with the SAME seed (fusion.py:156-173), so all entries are equal."""
    return GeneralMatrix(matrix=_replicated(lambda: sample_polynomial_coefficient_representation(
        modulus=modulus, degree=degree, root_order=root_order, root=root, inv_root=inv_root,
        norm_bound=norm_bound, weight_bound=weight_bound, seed=seed), num_rows, num_cols, seed))


def sample_ntt_matrix(seed: Optional[int], modulus: int, degree: int, root_order: int, root: int, inv_root: int,
                      num_rows: int, num_cols: int) -> GeneralMatrix:
    return GeneralMatrix(matrix=_replicated(lambda: sample_polynomial_ntt_representation(
        modulus=modulus, degree=degree, root_order=root_order, root=root, inv_root=inv_root, seed=seed),
        num_rows, num_cols, seed))


class Params(object):
    def __init__(self, secpar: int, seed: Optional[int]):
        # an unknown secpar silently yields an attribute-less object, as in the reference (:235)
        if secpar in PREFIX_PARAMETERS:
            self.secpar = secpar
            table = PREFIX_PARAMETERS[secpar]
            for name in _PARAM_FIELDS:
                setattr(self, name, table[name])
            self.public_challenge = sample_ntt_matrix(
                seed=seed, modulus=self.modulus, degree=self.degree, root_order=self.root_order, root=self.root,
                inv_root=self.inv_root, num_rows=self.num_rows_pub_challenge, num_cols=self.num_cols_pub_challenge)

    def __str__(self) -> str:
        order = ("secpar", "capacity", "modulus", "degree", "root_order", "root", "inv_root",
                 "num_rows_pub_challenge", "num_rows_sk", "num_rows_vk", "num_cols_pub_challenge", "num_cols_sk",
                 "num_cols_vk", "beta_sk", "beta_ch", "beta_ag", "beta_vf", "omega_sk", "omega_ch", "omega_ag",
                 "omega_vf", "public_challenge", "sign_pre_hash_dst", "sign_hash_dst", "agg_xof_dst",
                 "bytes_for_one_coef_bdd_by_beta_ch", "bytes_for_one_coef_bdd_by_beta_ag", "bytes_for_poly_shuffle")
        return "Params(" + ", ".join(f"{k}={str(getattr(self, k))}" for k in order) + ")"

    def __repr__(self) -> str:
        return self.__str__()

    def __eq__(self, other):
        return self.__dict__ == other.__dict__


def fusion_setup(secpar: int, seed: Optional[int]) -> Params:
    return Params(secpar=secpar, seed=seed)


class OneTimeSigningKey(object):
    def __init__(self, seed: Optional[int], left_sk_hat: GeneralMatrix, right_sk_hat: GeneralMatrix):
        self.seed = seed
        self.left_sk_hat = left_sk_hat
        self.right_sk_hat = right_sk_hat

    def __str__(self):
        return (f"OneTimeSigningKey(seed={self.seed}, left_sk_hat={str(self.left_sk_hat)}, "
                f"right_sk_hat={str(self.right_sk_hat)})")

    def __repr__(self):
        return self.__str__()


class OneTimeVerificationKey(object):
    def __init__(self, left_vk_hat: GeneralMatrix, right_vk_hat: GeneralMatrix):
        self.left_vk_hat = left_vk_hat
        self.right_vk_hat = right_vk_hat

    def __str__(self):
        return f"OneTimeVerificationKey(left_vk_hat={self.left_vk_hat}, right_vk_hat={self.right_vk_hat})"

    def __repr__(self):
        return self.__str__()


OneTimeKeyTuple = Tuple[OneTimeSigningKey, OneTimeVerificationKey]


# ---- array <-> object marshalling ----------------------------------------------------------------
def _ctx(params):
    return _backend.ntt_ctx(params.modulus, params.degree, params.root, params.inv_root)


def _ntt_poly(params, values):
    return PolynomialNTTRepresentation(modulus=params.modulus, degree=params.degree, root=params.root,
                                       inv_root=params.inv_root, root_order=params.root_order, values=values)


_TEMPLATES = {}


def _template(params):
    """an NTT-domain polynomial of the parameter set's ring, validated once (its data is never used)"""
    key = (params.modulus, params.degree, params.root, params.inv_root, params.root_order)
    if key not in _TEMPLATES:
        t = _ntt_poly(params, [0] * params.degree)
        _check_transformable(t, params.degree)       # what transform() would object to, once per ring instead of per call
        _TEMPLATES[key] = t
    return _TEMPLATES[key]


def _column(params, arr):
    """[rows][d] int32 -> rows x 1 GeneralMatrix of NTT-domain polynomials, each backed by its row of `arr` (the lists of
    Python ints are built when somebody reads `.values`: algebra/polynomials.py, storage note)"""
    if not len(arr):
        return GeneralMatrix(matrix=[])
    t = _template(params)
    return GeneralMatrix(matrix=[[t._like_arr(row)] for row in arr])


def _rows_of(matrix: GeneralMatrix, q):
    """GeneralMatrix of polynomials -> [rows*cols][d] int32 (row-major)"""
    return _backend.stack_polys([z for row in matrix.matrix for z in row], q)


def _sample_half(params, s):
    """The polynomial sample_polynomial_coefficient_representation(..., seed=s) returns, as an int32 row, with the process-global
    `random` left exactly where that function leaves it.  512 randrange() calls in Python are 0.6 ms per polynomial -- most
    of a keygen() call; the C clone of CPython's generator (fz_sample_coefficients_state, pinned to `random` by the tests) takes
    microseconds and hands back the generator's state for random.setstate().  Only for what it reproduces bit for bit: a
    plain non-negative int seed below 2^64 - 1 (random.seed takes abs() of negative ints and hashes other types) and the stock
    sampler and generator functions (nobody patched them)."""
    import random as _random
    import algebra.polynomials as _P
    if (type(s) is int and 0 <= s < 2 ** 64 - 1 and _pristine("sample_polynomial_coefficient_representation")
            and _P.sample_polynomial_coefficient_representation is _ORIGINALS["sample_polynomial_coefficient_representation"]
            and _P.randrange == _random.randrange and _P.random_seed == _random.seed):
        try:
            row, state = hostpipe.sample_coefficients_with_state(s, params.modulus, params.degree, params.beta_sk, params.omega_sk)
            _random.setstate((3, state, None))
            return row
        except Exception:
            pass
    return sample_polynomial_coefficient_representation(
        modulus=params.modulus, degree=params.degree, root_order=params.root_order, root=params.root, inv_root=params.inv_root,
        norm_bound=params.beta_sk, weight_bound=params.omega_sk, seed=s)._i32()


def keygen(params: Params, seed: Optional[int]) -> OneTimeKeyTuple:
    """fusion.py:338-373: two coefficient-domain secret vectors (seeds `seed`, `seed + 1`), their
    NTTs, and vk = public_challenge * sk_hat -- the arithmetic is ONE fz_keygen_core call."""
    q = params.modulus
    A = _rows_of(params.public_challenge, q)
    if seed is not None and _pristine("sample_coefficient_matrix", "transform"):
        # every entry of a half is sampled with the same seed (fusion.py:156-173), i.e. IS the same polynomial, and each
        # call leaves the process-global `random` where one call leaves it: sample it once, let the kernel read it for
        # all l rows (fz_keygen_core_bcast)
        halves = [_sample_half(params, s) for s in (seed, seed + 1)]
        sk_hat, vk = _ctx(params).keygen_core_bcast(A, np.stack(halves)[None])
    else:
        halves = []
        for s in (seed, seed + 1):       # (raises TypeError on None + 1, as the reference does)
            coefs = sample_coefficient_matrix(
                seed=s, modulus=q, degree=params.degree, root_order=params.root_order, root=params.root,
                inv_root=params.inv_root, num_rows=params.num_rows_sk, num_cols=params.num_cols_sk,
                norm_bound=params.beta_sk, weight_bound=params.omega_sk)
            halves.append(_rows_of(coefs, q))
        sk_hat, vk = _ctx(params).keygen_core(A, np.stack(halves)[None])
    sk = OneTimeSigningKey(seed=seed, left_sk_hat=_column(params, sk_hat[0, 0]),
                           right_sk_hat=_column(params, sk_hat[0, 1]))
    vkey = OneTimeVerificationKey(left_vk_hat=_column(params, vk[0, 0:1]), right_vk_hat=_column(params, vk[0, 1:2]))
    return sk, vkey


def keygen_to_bytes(params: Params, seed: Optional[int]) -> Tuple[bytes, OneTimeVerificationKey]:
    """NOT in the reference: (to_bytes(params, keygen(params, seed)[0]), keygen(params, seed)[1]) without the signing key's
    rows in between -- the secret polynomials sampled exactly as keygen() samples them (and the process-global `random` left
    where it leaves it), then one fz_keygen_records_async call that packs them into the "secret" record and transforms them for
    the verification key alone.  Raises ValueError with the reason when the key is over beta_sk, as to_bytes does."""
    from fusion_hip import ENCODING_REASONS
    q = params.modulus
    A = _rows_of(params.public_challenge, q)
    if seed is not None and _pristine("sample_coefficient_matrix", "transform"):
        coef = np.stack([_sample_half(params, s) for s in (seed, seed + 1)])[None]            # [1][2][d]: see keygen()
    else:
        halves = []
        for s in (seed, seed + 1):       # (raises TypeError on None + 1, as the reference does)
            coefs = sample_coefficient_matrix(
                seed=s, modulus=q, degree=params.degree, root_order=params.root_order, root=params.root,
                inv_root=params.inv_root, num_rows=params.num_rows_sk, num_cols=params.num_cols_sk,
                norm_bound=params.beta_sk, weight_bound=params.omega_sk)
            halves.append(_rows_of(coefs, q))
        coef = np.stack(halves)[None]                                                         # [1][2][l][d]
    data, vk, codes = _ctx(params).keygen_records(A, coef, int(params.beta_sk))
    if codes[0]:
        raise ValueError(ENCODING_REASONS[int(codes[0])])
    vkey = OneTimeVerificationKey(left_vk_hat=_column(params, vk[0, 0:1]), right_vk_hat=_column(params, vk[0, 1:2]))
    return data.tobytes(), vkey


class SignatureChallenge(object):
    def __init__(self, c_hat: PolynomialNTTRepresentation):
        self.c_hat = c_hat

    def __str__(self):
        return f"SignatureChallenge(c_hat={str(self.c_hat)})"

    def __repr__(self):
        return self.__str__()

    def __eq__(self, other):
        return self.c_hat == other.c_hat


class Signature(object):
    def __init__(self, signature_hat: GeneralMatrix):
        self.signature_hat = signature_hat

    def __str__(self):
        return f"Signature(signature_hat={str(self.signature_hat)})"

    def __repr__(self):
        return self.__str__()


# ---- hash -> challenge pipeline (host; formats are part of the scheme) --------------------------------
def hash_message_to_int(params: Params, message: str) -> int:
    salted = (params.sign_pre_hash_dst.decode("utf-8") + "," + message).encode()
    return int.from_bytes(sha3_256(salted).digest(), byteorder="little")


def hash_vk_and_int_to_bytes(params: Params, key: OneTimeVerificationKey, i: int, n: int) -> bytes:
    x = (params.sign_hash_dst.decode("utf-8") + "," + str(key) + "," + str(i)).encode("utf-8")
    return shake_256(x).digest(n)


def decode_bytes_to_polynomial_coefficients(b: bytes, log2_bias: int, modulus: int, degree: int, norm_bound: int,
                                            weight_bound: int) -> List[int]:
    """XOF bytes -> sparse signed coefficient list (fusion.py:422-481): sign bits, then
    `weight_bound` magnitudes, then a partial Fisher-Yates driven by big-endian index draws."""
    num_coefs = max(1, min(degree, weight_bound))
    bound = max(1, min(modulus // 2, norm_bound))
    coef_bytes = ceil((log2(bound) + 1 + log2_bias) / 8)
    index_bytes = ceil((log2(degree) + log2_bias) / 8)
    sign_bytes = ceil(weight_bound / 8)
    needed = sign_bytes + (coef_bytes + index_bytes) * weight_bound
    if len(b) < needed:
        raise ValueError(f"Too few bytes to decode polynomial. Expected {needed} but got {len(b)}")
    # sign i is bit i (LSB first) of the big-endian integer in the leading bytes; 1 -> +1, 0 -> -1
    sign_word = int.from_bytes(b[:sign_bytes], byteorder="big")
    pos = sign_bytes
    coefficients: List[int] = []
    for i in range(weight_bound):
        magnitude = int.from_bytes(b[pos:pos + coef_bytes], byteorder="big") % bound + 1
        pos += coef_bytes
        coefficients.append(magnitude if (sign_word >> i) & 1 else -magnitude)
    coefficients.extend([0] * (degree - len(coefficients)))
    if num_coefs < degree:
        for i in range(degree - 1, weight_bound, -1):
            j = int.from_bytes(b[pos:pos + index_bytes], byteorder="big") % (i + 1)
            pos += index_bytes
            coefficients[i], coefficients[j] = coefficients[j], coefficients[i]
    return coefficients


def _challenge_bytes_needed(params: Params) -> int:
    num_coefs = max(0, min(params.degree, params.omega_ch))
    bound = max(0, min(params.modulus // 2, params.beta_ch))
    coef_bytes = ceil((log2(bound) + 1 + params.secpar) / 8)
    index_bytes = ceil((log2(params.degree) + params.secpar) / 8)
    return ceil(params.omega_ch / 8) + coef_bytes * num_coefs + params.degree * index_bytes


_ORIGINALS = {}


def _pristine(*names):
    """True while the module-level functions a shortcut bypasses are the ones defined here.  The reference's tests replace
    `fusion.fusion.decode_bytes_to_polynomial_coefficients` (tests/test_fusion.py:596, :644, :652) and expect parse_challenge
    and hash_ch to call the replacement: a shortcut must step aside for whoever patches the function it stands in for."""
    g = globals()
    return all(g.get(n) is _ORIGINALS.get(n) for n in names)


def _decode_row(params, b, norm_bound, weight_bound):
    """decode_bytes_to_polynomial_coefficients through the library's C decoder (fz_decode_coefficients; pinned to the Python
    function above by tests/test_host_pipeline.py) -> int32 row, or None when it declines: the Python function then
    produces the result or the reference's error"""
    try:
        return hostpipe.decode_coefficients(b, params.secpar, params.modulus, params.degree, norm_bound, weight_bound)
    except Exception:
        return None


def _coef_poly(params, coefficients):
    return PolynomialCoefficientRepresentation(modulus=params.modulus, degree=params.degree, root=params.root,
                                               inv_root=params.inv_root, root_order=params.root_order,
                                               coefficients=coefficients)


def parse_challenge(params: Params, b: bytes) -> PolynomialNTTRepresentation:
    if len(b) < params.omega_ch * params.bytes_for_one_coef_bdd_by_beta_ch + params.bytes_for_poly_shuffle:
        raise ValueError("hashed_vk_and_pre_hashed_message is too short")
    row = _decode_row(params, b, params.beta_ch, params.omega_ch) if _pristine("decode_bytes_to_polynomial_coefficients") else None
    if row is not None:
        return _template(params)._like_arr(_ctx(params).ntt_forward(row))       # one forward NTT on the device
    coefs = decode_bytes_to_polynomial_coefficients(b=b, log2_bias=params.secpar, modulus=params.modulus,
                                                    degree=params.degree, norm_bound=params.beta_ch,
                                                    weight_bound=params.omega_ch)
    return transform(_coef_poly(params, coefs))


def hash_ch(params: Params, key: OneTimeVerificationKey, message: str) -> SignatureChallenge:
    pre_hashed = hash_message_to_int(params=params, message=message)
    xof = hash_vk_and_int_to_bytes(params=params, key=key, i=pre_hashed, n=_challenge_bytes_needed(params))
    return SignatureChallenge(c_hat=parse_challenge(params=params, b=xof))


def _challenges(params: Params, pairs) -> List[SignatureChallenge]:
    """[hash_ch(params, key, message) for key, message in pairs] with ONE batched forward transform for all of them
    instead of a launch per signer; anything the C decoder declines goes through hash_ch itself"""
    pairs = list(pairs)
    if not _pristine("hash_ch", "parse_challenge", "decode_bytes_to_polynomial_coefficients", "transform"):
        return [hash_ch(params=params, key=k, message=m) for k, m in pairs]
    n = _challenge_bytes_needed(params)
    rows = []
    for k, m in pairs:
        b = hash_vk_and_int_to_bytes(params=params, key=k, i=hash_message_to_int(params=params, message=m), n=n)
        row = None
        if len(b) >= params.omega_ch * params.bytes_for_one_coef_bdd_by_beta_ch + params.bytes_for_poly_shuffle:
            row = _decode_row(params, b, params.beta_ch, params.omega_ch)
        if row is None:
            return [hash_ch(params=params, key=k, message=m) for k, m in pairs]
        rows.append(row)
    if not rows:
        return []
    t = _template(params)
    return [SignatureChallenge(c_hat=t._like_arr(r)) for r in _ctx(params).ntt_forward(np.stack(rows))]


def sign(params: Params, key: OneTimeKeyTuple, message: str) -> Signature:
    """sigma = left_sk_hat * c_hat + right_sk_hat (fusion.py:534-557) as one fz_sign_core call."""
    sk, vk = key
    c_hat = hash_ch(params=params, key=vk, message=message).c_hat
    q = params.modulus
    sk_hat = np.stack([_rows_of(sk.left_sk_hat, q), _rows_of(sk.right_sk_hat, q)])[None]
    sig = _ctx(params).sign_core(sk_hat, c_hat._i32()[None])
    return Signature(signature_hat=_column(params, sig[0]))


class AggregationCoefficient(object):
    def __init__(self, alpha_hat: PolynomialNTTRepresentation):
        self.alpha_hat = alpha_hat

    def __str__(self):
        return f"AggregationCoefficient(alpha_hat={self.alpha_hat})"

    def __repr__(self):
        return self.__str__()


def _agg_coef_bytes(params: Params) -> int:
    bound = max(0, min(params.modulus // 2, params.beta_ag))
    coef_bytes = ceil((log2(bound) + 1 + params.secpar) / 8)
    index_bytes = ceil((log2(params.degree) + params.secpar) / 8)
    return ceil(params.omega_ag / 8) + (coef_bytes + index_bytes) * params.omega_ag


def hash_vks_and_ints_and_challs_to_bytes(params: Params, keys: List[OneTimeVerificationKey],
                                          prehashed_messages: List[int],
                                          challenges: List[SignatureChallenge]) -> bytes:
    n = len(keys) * _agg_coef_bytes(params)
    salted = str.encode(params.agg_xof_dst.decode("utf-8") + ","
                        + str(list(zip(keys, prehashed_messages, challenges))))
    return shake_256(salted).digest(n)


def decode_bytes_to_agg_coefs(params: Params, b: bytes) -> List[AggregationCoefficient]:
    n = _agg_coef_bytes(params)
    count = len(b) // n
    if not count:
        return []
    fast = _pristine("decode_bytes_to_polynomial_coefficients")
    rows = [_decode_row(params, b[i * n:(i + 1) * n], params.beta_ag, params.omega_ag) if fast else None for i in range(count)]
    if any(r is None for r in rows):
        rows = _backend.to_i32([decode_bytes_to_polynomial_coefficients(
            b=b[i * n:(i + 1) * n], log2_bias=params.secpar, modulus=params.modulus, degree=params.degree,
            norm_bound=params.beta_ag, weight_bound=params.omega_ag) for i in range(count)], params.modulus)
    # all `count` forward transforms in one batched launch
    hats = _ctx(params).ntt_forward(np.stack(rows))
    t = _template(params)
    return [AggregationCoefficient(alpha_hat=t._like_arr(row)) for row in hats]


def hash_ag(params: Params, keys: List[OneTimeVerificationKey], messages: List[str],
            _challs: Optional[List[SignatureChallenge]] = None) -> List[AggregationCoefficient]:
    """fusion.py:632-652.  `_challs` (not in the reference): the challenges of exactly these (key, message) pairs when the
    caller has them already -- verify() needs them itself, and hash_ch is a pure function of its arguments."""
    pairs = list(zip(keys, messages))
    pre_hashed = [hash_message_to_int(params=params, message=m) for _, m in pairs]
    challs = _challs if _challs is not None else _challenges(params, pairs)
    b = hash_vks_and_ints_and_challs_to_bytes(params=params, keys=keys, prehashed_messages=pre_hashed,
                                              challenges=challs)
    return decode_bytes_to_agg_coefs(params=params, b=b)


def aggregate(params: Params, keys: List[OneTimeVerificationKey], messages: List[str],
              signatures: List[Signature]) -> Signature:
    """sum_i sigma_i * alpha_i over the key-sorted inputs (fusion.py:655-677): one fz_aggregate_core."""
    triples = sorted(list(zip(keys, messages, signatures)), key=lambda x: str(x[0]))
    alphas = hash_ag(params=params, keys=[t[0] for t in triples], messages=[t[1] for t in triples])
    q = params.modulus
    sig = np.stack([_rows_of(t[2].signature_hat, q) for t in triples])
    alpha = _backend.stack_polys([a.alpha_hat for a in alphas], q)
    out = _ctx(params).aggregate_core(sig, alpha)
    return Signature(signature_hat=_column(params, out))


def verify(params: Params, keys: List[OneTimeVerificationKey], messages: List[str],
           aggregate_signature: Signature) -> Tuple[bool, str]:
    """fusion.py:680-728.  Never raises for a bad signature: (False, reason) with the reference's
    reason strings, checked in the reference's order (target, then norm, then weight)."""
    if len(keys) > params.capacity:
        return False, VERDICT_REASONS[1]
    if len(keys) != len(messages):
        return False, VERDICT_REASONS[2]
    pairs = sorted(zip(keys, messages), key=lambda x: str(x[0]))
    sorted_vks = [p[0] for p in pairs]
    challs = _challenges(params, pairs)
    if _pristine("hash_ag"):
        alphas = hash_ag(params=params, keys=sorted_vks, messages=[p[1] for p in pairs], _challs=challs)
    else:
        alphas = hash_ag(params=params, keys=sorted_vks, messages=[p[1] for p in pairs])
    q = params.modulus
    code = _ctx(params).verify_core(
        _rows_of(params.public_challenge, q), _rows_of(aggregate_signature.signature_hat, q),
        _backend.stack_polys([v.left_vk_hat.matrix[0][0] for v in sorted_vks], q),
        _backend.stack_polys([v.right_vk_hat.matrix[0][0] for v in sorted_vks], q),
        _backend.stack_polys([c.c_hat for c in challs], q),
        _backend.stack_polys([a.alpha_hat for a in alphas], q),
        params.beta_vf, params.omega_vf)
    return (code == 0), VERDICT_REASONS[code]


def verify_signatures(params: Params, keys: List[OneTimeVerificationKey], messages: List[str],
                      signatures: List[Signature]) -> List[Tuple[bool, str]]:
    """NOT in the reference (an extension of the object face): is each single signature valid?  -> one (ok, reason) per signer,
    reasons from fusion_hip.SIGNATURE_REASONS.  Signer i passes when A . sigma_i == vkL_i * c_i + vkR_i (c_i = hash_ch(vk_i,
    m_i)), ||INTT(sigma_i)||_inf <= VF_BD_INTERMEDIATE_{secpar} (the bound of ONE honest signature) and every row's weight
    <= omega_vf -- verify() of a one-signer aggregate with alpha == 1, but against the single-signature bound.  Screen
    untrusted contributions with it before aggregate(): one bad signature makes the aggregate fail verify() without saying
    whose it was.  Batched exactly as fusion_hip.scheme.BatchScheme.verify_signatures (one challenge pass, one launch).
    Unequal numbers of keys, messages and signatures raise fusion_hip.FusionHipError(FZ_E_BADARG)."""
    from fusion_hip import FusionHipError, SIGNATURE_REASONS
    from fusion_hip._lib import FZ_E_BADARG
    from fusion_hip.scheme import BatchScheme, signature_from_object, vk_from_object
    if not (len(keys) == len(messages) == len(signatures)):
        raise FusionHipError(FZ_E_BADARG, f"{len(keys)} keys, {len(messages)} messages, {len(signatures)} signatures")
    n, d, l = len(keys), params.degree, params.num_rows_sk
    vk = np.stack([vk_from_object(params, k) for k in keys]) if n else np.zeros((0, 2, d), dtype=np.int32)
    sig = np.stack([signature_from_object(params, s) for s in signatures]) if n else np.zeros((0, l, d), dtype=np.int32)
    bs = BatchScheme(params)
    try:
        codes = bs.verify_signatures(vk, list(messages), sig)
    finally:
        bs.close()
    return [(int(c) == 0, SIGNATURE_REASONS[int(c)]) for c in codes]


def to_bytes(params: Params, obj, aggregate: bool = False) -> bytes:
    """NOT in the reference (an extension of the object face): the canonical compact bytes of a OneTimeVerificationKey, a
    OneTimeSigningKey (a "secret" record) or a Signature; aggregate=True encodes a Signature under
    the aggregate bound beta_vf instead of the single-signature one.  Raises ValueError with the reason when the object cannot
    be encoded (its norm is over the bound)."""
    from fusion_hip import ENCODING_REASONS
    from fusion_hip.scheme import BatchScheme, signature_from_object, vk_from_object
    if isinstance(obj, OneTimeVerificationKey):
        kind, rows = "vk", vk_from_object(params, obj)[None]
    elif isinstance(obj, Signature):
        kind, rows = ("aggregate" if aggregate else "signature"), signature_from_object(params, obj)[None]
    elif isinstance(obj, OneTimeSigningKey):
        q = params.modulus
        kind, rows = "secret", np.stack([_rows_of(obj.left_sk_hat, q), _rows_of(obj.right_sk_hat, q)])[None]
    else:
        raise TypeError(f"to_bytes takes a OneTimeVerificationKey, a OneTimeSigningKey or a Signature, not {type(obj).__name__}")
    bs = BatchScheme(params)
    try:
        data, codes = bs.encode(kind, rows)
    finally:
        bs.close()
    if codes[0]:
        raise ValueError(ENCODING_REASONS[int(codes[0])])
    return data.tobytes()


def sign_to_bytes(params: Params, key: OneTimeKeyTuple, message: str) -> bytes:
    """NOT in the reference: to_bytes(params, sign(params, key, message)) without the Signature in between -- the challenge as
    sign() takes it (hash_ch, whoever stands behind that name), then one fz_sign_encoded_async call that signs and packs.  Raises
    ValueError with the reason when the signature is over the bound of one signature, as to_bytes does."""
    from fusion_hip import ENCODING_REASONS
    from fusion_hip.scheme import signature_bound
    sk, vk = key
    bound = signature_bound(params)
    c_hat = hash_ch(params=params, key=vk, message=message).c_hat
    q = params.modulus
    sk_hat = np.stack([_rows_of(sk.left_sk_hat, q), _rows_of(sk.right_sk_hat, q)])[None]
    data, codes = _ctx(params).sign_encoded(sk_hat, c_hat._i32()[None], bound)
    if codes[0]:
        raise ValueError(ENCODING_REASONS[int(codes[0])])
    return data.tobytes()


def sign_from_bytes(params: Params, secret_record: bytes, vk: OneTimeVerificationKey, message: str) -> bytes:
    """NOT in the reference: sign_to_bytes(params, (from_bytes(params, "secret", secret_record), vk), message) without the key's
    rows in between -- the challenge as sign() takes it, then one fz_sign_records_async call that signs from the record and
    packs.  Raises ValueError for a record of the wrong length, and with the reason for a record that is not canonical (6) or a
    signature over the bound of one signature (4)."""
    from fusion_hip import ENCODING_REASONS
    from fusion_hip.scheme import encoded_size, signature_bound
    size = encoded_size(params, "secret")
    if len(secret_record) != size:
        raise ValueError(f"a 'secret' record is {size} bytes, not {len(secret_record)}")
    c_hat = hash_ch(params=params, key=vk, message=message).c_hat
    data, codes = _ctx(params).sign_records(bytes(secret_record), int(params.beta_sk), c_hat._i32()[None], params.num_rows_sk,
                                            signature_bound(params))
    if codes[0]:
        raise ValueError(ENCODING_REASONS[int(codes[0])])
    return data.tobytes()


def vk_of_secret_bytes(params: Params, secret_record: bytes) -> OneTimeVerificationKey:
    """NOT in the reference: the verification key of one "secret" record, keygen(params, seed)[1] for the record
    keygen_to_bytes(params, seed) returned, without the key's rows in between -- one fz_vk_records_async call that unpacks the
    record, transforms it and multiplies by the public challenge.  Raises ValueError for a record of the wrong length, and
    with the reason for a record that is not canonical (6)."""
    from fusion_hip import ENCODING_REASONS
    from fusion_hip.scheme import encoded_size
    size = encoded_size(params, "secret")
    if len(secret_record) != size:
        raise ValueError(f"a 'secret' record is {size} bytes, not {len(secret_record)}")
    vk, codes = _ctx(params).vk_records(bytes(secret_record), int(params.beta_sk), _rows_of(params.public_challenge, params.modulus),
                                        params.num_rows_sk)
    if codes[0]:
        raise ValueError(ENCODING_REASONS[int(codes[0])])
    return OneTimeVerificationKey(left_vk_hat=_column(params, vk[0, 0:1]), right_vk_hat=_column(params, vk[0, 1:2]))


def sign_from_secret_bytes(params: Params, secret_record: bytes, message: str) -> Tuple[bytes, OneTimeVerificationKey]:
    """NOT in the reference: sign_from_bytes from the record alone -> (the signature's bytes, the verification key the record
    belongs to): vk_of_secret_bytes, then sign_from_bytes with that key -- the challenge through hash_ch, whoever stands behind
    that name.  Raises ValueError as those two do."""
    vk = vk_of_secret_bytes(params, secret_record)
    return sign_from_bytes(params, secret_record, vk, message), vk


def from_bytes(params: Params, kind: str, data: bytes):
    """NOT in the reference: the inverse of to_bytes for one record of `kind` ("vk", "signature", "aggregate" or "secret") -> a
    OneTimeVerificationKey, a Signature or a OneTimeSigningKey (seed=None: the record does not hold it).  Raises ValueError for
    a wrong length or a record that is not canonical."""
    from fusion_hip import ENCODING_REASONS
    from fusion_hip.scheme import BatchScheme, encoded_size, signature_to_object, sk_to_object, vk_to_object
    size = encoded_size(params, kind)
    if len(data) != size:
        raise ValueError(f"a {kind!r} record is {size} bytes, not {len(data)}")
    bs = BatchScheme(params)
    try:
        rows, codes = bs.decode(kind, data)
    finally:
        bs.close()
    if codes[0]:
        raise ValueError(ENCODING_REASONS[int(codes[0])])
    if kind == "secret":
        return sk_to_object(params, None, rows[0])
    return vk_to_object(params, rows[0]) if kind == "vk" else signature_to_object(params, rows[0])


def _aggregate_from_bytes(params, keys, messages, blobs, verify):
    """aggregate_from_bytes (verify=False: no verdict, None) and aggregate_verify_from_bytes: -> (Signature, verdict)"""
    from fusion_hip import ENCODING_REASONS
    from fusion_hip.scheme import BatchScheme, encoded_size, vk_from_object
    if not (len(keys) == len(messages) == len(blobs)):
        raise ValueError(f"{len(keys)} keys, {len(messages)} messages, {len(blobs)} records")
    size = encoded_size(params, "signature")
    for i, b in enumerate(blobs):
        if len(b) != size:
            raise ValueError(f"record {i}: a 'signature' record is {size} bytes, not {len(b)}")
    if not blobs:
        raise ValueError("no records to aggregate")
    vk = np.stack([vk_from_object(params, k) for k in keys])
    bs = BatchScheme(params)
    try:
        call = bs.aggregate_verify_encoded if verify else bs.aggregate_encoded
        out, codes, *verdict = call(vk, list(messages), b"".join(bytes(b) for b in blobs))
    finally:
        bs.close()
    bad = np.flatnonzero(codes)
    if bad.size:
        raise ValueError(f"record {int(bad[0])}: {ENCODING_REASONS[int(codes[bad[0]])]}")
    return Signature(signature_hat=_column(params, out)), (verdict[0] if verify else None)


def aggregate_from_bytes(params: Params, keys: List[OneTimeVerificationKey], messages: List[str],
                         blobs: List[bytes]) -> Signature:
    """NOT in the reference: aggregate() of signatures given as their compact bytes (one "signature" record of to_bytes
    each), without ever expanding them -- the Signature that aggregate(params, keys, messages, [from_bytes(params,
    "signature", b) for b in blobs]) returns (BatchScheme.aggregate_encoded: one fused pass over the bytes).  Raises
    ValueError for unequal numbers of keys, messages and blobs, for a blob of the wrong length, and for a record that is not
    canonical (with the index of the first one and the reason).  The target equation of a signature is NOT checked, as
    aggregate() does not check it either: verify() the result, or call aggregate_verify_from_bytes."""
    return _aggregate_from_bytes(params, keys, messages, blobs, False)[0]


def aggregate_verify_from_bytes(params: Params, keys: List[OneTimeVerificationKey], messages: List[str],
                                blobs: List[bytes]) -> Tuple[Signature, Tuple[bool, str]]:
    """NOT in the reference: aggregate_from_bytes and verify() of its result in one pass, as an aggregator that checks its own
    output does -> (Signature, (ok, reason)): the Signature of aggregate_from_bytes and what verify(params, keys, messages,
    that Signature) returns (BatchScheme.aggregate_verify_encoded: the challenges and hash_ag are computed once, not twice).
    Raises ValueError as aggregate_from_bytes does."""
    return _aggregate_from_bytes(params, keys, messages, blobs, True)


def verify_signatures_from_bytes(params: Params, keys: List[OneTimeVerificationKey], messages: List[str],
                                 blobs: List[bytes]) -> List[Tuple[bool, str]]:
    """NOT in the reference: verify_signatures() of signatures given as their compact bytes (one "signature" record of
    to_bytes each), without ever expanding them -> [(ok, reason)] per signer (BatchScheme.verify_signatures_encoded).  A record
    that is not canonical reports (False, "Encoding is not canonical."), a signature that misses its key's target (False,
    "Target doesn't match image of signature.").  Raises ValueError for unequal numbers of keys, messages and blobs and for a
    blob of the wrong length (with its index)."""
    from fusion_hip import ENCODING_REASONS, SIGNATURE_REASONS
    from fusion_hip.scheme import BatchScheme, encoded_size, vk_from_object
    if not (len(keys) == len(messages) == len(blobs)):
        raise ValueError(f"{len(keys)} keys, {len(messages)} messages, {len(blobs)} records")
    size = encoded_size(params, "signature")
    for i, b in enumerate(blobs):
        if len(b) != size:
            raise ValueError(f"record {i}: a 'signature' record is {size} bytes, not {len(b)}")
    if not blobs:
        return []
    vk = np.stack([vk_from_object(params, k) for k in keys])
    bs = BatchScheme(params)
    try:
        codes = bs.verify_signatures_encoded(vk, list(messages), b"".join(bytes(b) for b in blobs))
    finally:
        bs.close()
    return [(int(c) == 0, ENCODING_REASONS[6] if int(c) == 6 else SIGNATURE_REASONS[int(c)]) for c in codes]


def verify_from_bytes(params: Params, keys: List[OneTimeVerificationKey], messages: List[str], blob: bytes) -> Tuple[bool, str]:
    """NOT in the reference: verify() of an aggregate given as its compact bytes (the "aggregate" record of to_bytes(...,
    aggregate=True)), without expanding it -> (ok, reason) as verify(params, keys, messages, from_bytes(params, "aggregate",
    blob)) gives it (BatchScheme.verify_encoded); a record that is not canonical reports (False, "Encoding is not
    canonical.").  Raises ValueError for a blob of the wrong length."""
    from fusion_hip.scheme import BatchScheme, encoded_size, vk_from_object
    size = encoded_size(params, "aggregate")
    if len(blob) != size:
        raise ValueError(f"an 'aggregate' record is {size} bytes, not {len(blob)}")
    d = params.degree
    vk = np.stack([vk_from_object(params, k) for k in keys]) if len(keys) else np.zeros((0, 2, d), dtype=np.int32)
    bs = BatchScheme(params)
    try:
        return bs.verify_encoded(vk, list(messages), bytes(blob))
    finally:
        bs.close()


def _groups_for_many(params: Params, keys_per_group, messages_per_group):
    """the concatenated key rows, messages and sizes of G groups of signers; ValueError (naming the group) for unequal numbers of
    groups, a group without signers and a group with unequal numbers of keys and messages"""
    from fusion_hip.scheme import vk_from_object
    if len(keys_per_group) != len(messages_per_group):
        raise ValueError(f"{len(keys_per_group)} groups of keys, {len(messages_per_group)} groups of messages")
    for g, (k, m) in enumerate(zip(keys_per_group, messages_per_group)):
        if len(k) != len(m):
            raise ValueError(f"group {g}: {len(k)} keys, {len(m)} messages")
        if not len(k):
            raise ValueError(f"group {g}: no signers")
    return (lambda: np.stack([vk_from_object(params, k) for ks in keys_per_group for k in ks]),
            [m for ms in messages_per_group for m in ms], [len(ks) for ks in keys_per_group])


def _aggregate_many_from_bytes(params, keys_per_group, messages_per_group, blobs_per_group, verify, hash_ag="host", key_sort="host"):
    """aggregate_many_from_bytes (verify=False: no verdicts, None) and aggregate_verify_many_from_bytes: -> ([Signature] * G, verdicts);
    hash_ag: BatchScheme's, where the committees' aggregation coefficients are hashed ("host", "device" or "auto"); key_sort:
    BatchScheme's, where the device form sorts the committees' keys ("host" or "device")"""
    from fusion_hip import ENCODING_REASONS
    from fusion_hip.scheme import BatchScheme, encoded_size
    if len(blobs_per_group) != len(keys_per_group):
        raise ValueError(f"{len(keys_per_group)} groups of keys, {len(blobs_per_group)} groups of records")
    vk_rows, messages, sizes = _groups_for_many(params, keys_per_group, messages_per_group)
    size = encoded_size(params, "signature")
    for g, blobs in enumerate(blobs_per_group):
        if len(blobs) != sizes[g]:
            raise ValueError(f"group {g}: {sizes[g]} keys, {len(blobs)} records")
        for i, b in enumerate(blobs):
            if len(b) != size:
                raise ValueError(f"group {g} record {i}: a 'signature' record is {size} bytes, not {len(b)}")
    if not sizes:
        return [], ([] if verify else None)
    bs = BatchScheme(params, hash_ag=hash_ag, key_sort=key_sort)
    try:
        call = bs.aggregate_verify_many_encoded if verify else bs.aggregate_many_encoded
        out, codes, *verdicts = call(vk_rows(), messages, b"".join(bytes(b) for blobs in blobs_per_group for b in blobs), sizes)
    finally:
        bs.close()
    bad = np.flatnonzero(codes)
    if bad.size:
        off = np.concatenate([[0], np.cumsum(sizes)])
        g = int(np.searchsorted(off, bad[0], side="right")) - 1
        raise ValueError(f"group {g} record {int(bad[0] - off[g])}: {ENCODING_REASONS[int(codes[bad[0]])]}")
    return [Signature(signature_hat=_column(params, rows)) for rows in out], (verdicts[0] if verify else None)


def aggregate_many_from_bytes(params: Params, keys_per_group: List[List[OneTimeVerificationKey]], messages_per_group: List[List[str]],
                              blobs_per_group: List[List[bytes]], hash_ag: str = "host", key_sort: str = "host") -> List[Signature]:
    """NOT in the reference: aggregate_from_bytes for G committees at once -> [Signature] * G, entry g what
    aggregate_from_bytes(params, keys_per_group[g], messages_per_group[g], blobs_per_group[g]) returns
    (BatchScheme.aggregate_many_encoded: one launch over all committees' bytes).  Raises ValueError, naming the group and the
    record, for unequal numbers of groups, of keys, messages and blobs of a group, for a group without signers, for a blob of
    the wrong length and for a record that is not canonical (the first one, with the reason).  hash_ag: where the committees'
    aggregation coefficients are hashed, "host" (the default), "device" or "auto" (BatchScheme's option; the result is the same).
    key_sort: where the device form sorts each committee's keys, "host" (the default) or "device" (BatchScheme's option; the
    result is the same)."""
    return _aggregate_many_from_bytes(params, keys_per_group, messages_per_group, blobs_per_group, False, hash_ag, key_sort)[0]


def aggregate_verify_many_from_bytes(params: Params, keys_per_group: List[List[OneTimeVerificationKey]],
                                     messages_per_group: List[List[str]],
                                     blobs_per_group: List[List[bytes]],
                                     hash_ag: str = "host",
                                     key_sort: str = "host") -> Tuple[List[Signature], List[Tuple[bool, str]]]:
    """NOT in the reference: aggregate_verify_from_bytes for G committees at once -> ([Signature] * G, [(ok, reason)] * G), entry g
    of each what aggregate_verify_from_bytes(params, keys_per_group[g], messages_per_group[g], blobs_per_group[g]) returns
    (BatchScheme.aggregate_verify_many_encoded: one launch for all committees' aggregates and verification targets, one for all
    verdicts).  Raises ValueError as aggregate_many_from_bytes does; hash_ag and key_sort as there."""
    return _aggregate_many_from_bytes(params, keys_per_group, messages_per_group, blobs_per_group, True, hash_ag, key_sort)


def verify_many_from_bytes(params: Params, keys_per_group: List[List[OneTimeVerificationKey]], messages_per_group: List[List[str]],
                           blobs: List[bytes], hash_ag: str = "host", key_sort: str = "host") -> List[Tuple[bool, str]]:
    """NOT in the reference: verify_from_bytes for G aggregates at once (blobs[g]: the "aggregate" record of group g) ->
    [(ok, reason)] * G, entry g what verify_from_bytes(params, keys_per_group[g], messages_per_group[g], blobs[g]) returns
    (BatchScheme.verify_many_encoded).  Raises ValueError, naming the group, for unequal numbers of groups, of keys and messages
    of a group, for a group without signers and for a blob of the wrong length.  hash_ag and key_sort as aggregate_many_from_bytes
    takes them."""
    from fusion_hip.scheme import BatchScheme, encoded_size
    if len(blobs) != len(keys_per_group):
        raise ValueError(f"{len(keys_per_group)} groups of keys, {len(blobs)} records")
    vk_rows, messages, sizes = _groups_for_many(params, keys_per_group, messages_per_group)
    size = encoded_size(params, "aggregate")
    for g, b in enumerate(blobs):
        if len(b) != size:
            raise ValueError(f"group {g} record 0: an 'aggregate' record is {size} bytes, not {len(b)}")
    if not sizes:
        return []
    bs = BatchScheme(params, hash_ag=hash_ag, key_sort=key_sort)
    try:
        return bs.verify_many_encoded(vk_rows(), messages, b"".join(bytes(b) for b in blobs), sizes)
    finally:
        bs.close()


_ORIGINALS.update({name: globals()[name] for name in (
    "decode_bytes_to_polynomial_coefficients", "hash_ch", "parse_challenge", "transform", "sample_coefficient_matrix", "hash_ag",
    "sample_polynomial_coefficient_representation")})
