"""Fixtures that put the per-signer challenge pipeline (csrc/fz_challenge.hip, csrc/fz_keccak_wave.h, csrc/fz_host.cpp: text
of str(vk) -> SHAKE-256 -> decoder) exactly on the edges its code depends on, and a model of the operation in plain Python.

What the code depends on, and the family that pins it:
- str(int(prehash)) is written three times (u256_to_base1e9 on one lane, the systolic array of challenge_wave_kernel,
  u256_decimal on the host): a 256-bit integer in 1..9 chunks of base 10^9, the top chunk 1..9 digits wide, every inner
  chunk zero-padded to nine.  digest_fixtures(): 10^k and 10^k - 1 for every digit count 1..78, the limb boundaries
  2^(32t) - 1 / 2^(32t) / 2^(32t) + 1, 2^255, 2^256 - 1, and for every inner chunk position one integer whose chunk there
  is 0, one where it is 999999999 and one where it has fewer than nine digits.
- the serialiser places characters by a wave prefix scan over dec_len() of the lanes' values (vpl = 2 * degree / 64 values per
  lane, one with idle lanes below degree 32) and drops the separator after the last value of each row.  key_fixtures(): the
  41 values [0, +-(10^k - 1), +-10^k (k = 1..9), +-(q // 2), 2^31 - 1, -2^31] rotated through every position, so that each
  occurs in every slot of a lane and at indices 0, degree - 1, degree and 2 * degree - 1; the all-zero key (shortest text)
  and keys of 2 * degree values of eleven characters (longest text).
- the SHAKE padding lands where the text length puts it: buf[len] ^= 0x1f, buf[nb * 136 - 1] ^= 0x80, nb = len // 136 + 1.
  sweep_fixtures(): texts of 136 consecutive lengths, i.e. every residue mod 136 (135: both suffix bits in one byte; 0: a
  whole extra block).
- message_fixtures(): every byte length 0..280, the block boundaries len + 4 = 0 (mod 136) up to eight blocks, multi-byte
  UTF-8 on them, and two long messages (20 000 and 200 000 bytes) that share a wave with short ones.

The model: text() is Python's str() of the integers between the fixed pieces, row() is hashlib.shake_256 and the decoder of
fusion.py:422-481 restated on int.from_bytes.  It calls nothing of this project.  mech_blocks() states the same text the way
the kernels build it (lengths by comparisons, positions by prefix sums, digits written backwards, chunks of base 10^9, the
two pad bytes), with a switch per plausible fault; sponge() is a plain Keccak-f[1600] that absorbs whatever blocks it is
given, so that a wrong pad byte or block count can be followed to the row it would produce.
tests/test_challenge_edges_host.py shows that the fixtures reach every edge and that every fault changes a fixture's row."""
import bisect
import functools
import hashlib
import types
from math import ceil, log2

import numpy as np

from oracle.oracle import splitmix_centered

PRIME = 2147465729
RATE = 136
I32_MIN, I32_MAX = -(2 ** 31), 2 ** 31 - 1
_ROOT_256 = 3337519                            # a primitive 512th root of unity mod PRIME (the scheme's at secpar 256)


def _param_set(name, secpar, degree, weight, weight_ag, root, dst, scheme):
    return types.SimpleNamespace(
        name=name, secpar=secpar, modulus=PRIME, degree=degree, root=root, inv_root=pow(root, PRIME - 2, PRIME),
        root_order=2 * degree, omega_ch=weight, omega_ag=weight_ag, beta_ch=1, beta_ag=1, scheme=scheme,
        bytes_for_one_coef_bdd_by_beta_ch=0, bytes_for_poly_shuffle=0,
        sign_pre_hash_dst=bytes([dst, 0]), sign_hash_dst=bytes([dst, 1]), agg_xof_dst=bytes([dst, 2]))


# the two scheme sets (fusion.py:24-118) and three beyond them: four values per lane, and fewer values than lanes
SETS = {p.name: p for p in (
    _param_set("s128", 128, 64, 27, 35, 23584283, 1, True),
    _param_set("s256", 256, 256, 60, 60, _ROOT_256, 3, True),
    _param_set("d128w64", 256, 128, 64, 64, pow(_ROOT_256, 2, PRIME), 9, False),
    _param_set("d16", 128, 16, 5, 5, pow(_ROOT_256, 16, PRIME), 9, False),
    _param_set("d4", 40, 4, 1, 1, pow(_ROOT_256, 64, PRIME), 9, False),
)}
SCHEME_SETS = ("s128", "s256")
EXTRA_SETS = ("d128w64", "d16", "d4")


def vpl(ps):
    """values per lane of the serialiser's wave (vk_text_wave)"""
    return max(1, 2 * ps.degree // 64)


# ---- fixtures -----------------------------------------------------------------------------------------------------------------
THRESHOLDS = [0] + [s * v for k in range(1, 10) for v in (10 ** k - 1, 10 ** k) for s in (1, -1)] + \
    [PRIME // 2, -(PRIME // 2), I32_MAX, I32_MIN]
BASE_DIGEST = 3 ** 161                          # 77 digits, no chunk trivial
_G = 1000000000


def from_chunks(chunks):
    """the integer whose base-10^9 chunks (least significant first) are `chunks`"""
    return sum(c * _G ** j for j, c in enumerate(chunks))


def chunks_of(x):
    out = []
    while True:
        x, r = divmod(x, _G)
        out.append(r)
        if not x:
            return out


def digest_fixtures():
    """[(name, integer < 2^256)]"""
    out = []
    for k in range(78):
        out.append((f"10^{k}", 10 ** k))
        out.append((f"10^{k}-1", 10 ** k - 1))
    for t in range(1, 8):
        out += [(f"2^{32 * t}-1", 2 ** (32 * t) - 1), (f"2^{32 * t}", 2 ** (32 * t)), (f"2^{32 * t}+1", 2 ** (32 * t) + 1)]
    out += [("2^255", 2 ** 255), ("2^256-1", 2 ** 256 - 1)]
    full = [(123456789 + 98765432 * j) % _G for j in range(8)] + [98765]       # nine chunks; every inner one has nine digits
    assert all(c >= 10 ** 8 for c in full[:8])
    for j in range(8):
        for tag, c in (("zero", 0), ("nines", _G - 1), ("short", 10 ** (j % 8) + j)):     # short: 1..8 digits
            ch = list(full)
            ch[j] = c
            out.append((f"chunk{j}-{tag}", from_chunks(ch)))
    assert all(0 <= v < 2 ** 256 for _, v in out)
    return out


def key_fixtures(ps):
    """[(name, [2][degree] int32)]"""
    d = ps.degree
    n, T = 2 * d, THRESHOLDS
    out = []
    for r in range(len(T)):                     # value T[i] at every flat index k with k + r = i (mod 41)
        out.append((f"rot{r}", np.array([T[(k + r) % len(T)] for k in range(n)], dtype=np.int64)))
    out.append(("zero", np.zeros(n, dtype=np.int64)))
    out.append(("longest-halfq", np.full(n, -(PRIME // 2), dtype=np.int64)))
    out.append(("longest-min", np.full(n, I32_MIN, dtype=np.int64)))
    mixed = np.where(np.arange(n) % 2 == 0, I32_MIN, -(10 ** 9))
    out.append(("longest-mixed", mixed.astype(np.int64)))
    return [(name, v.astype(np.int32).reshape(2, d)) for name, v in out]


def base_key(ps):
    return splitmix_centered(0xC4A11E6E + ps.degree, 2 * ps.degree).reshape(2, ps.degree)


def sweep_fixtures(ps):
    """[(name, key, digest)]: texts of 136 consecutive lengths.  Step e has e more characters than step 0 (2 * degree values of
    one digit, a digest of one digit): the first e values have two digits, or the first e - 10 with a digest of eleven digits
    (every other step, and every step past 2 * degree); where a key has too few values even for that, a longer digest and
    then wider values"""
    d = ps.degree
    n = 2 * d
    out = []
    for e in range(RATE):
        widths = [1] * n
        digits = 1
        if 10 <= e <= n + 10 and (e > n or e % 2):       # both digests wherever both fit
            m, digits = e - 10, 11
        elif e <= n:
            m = e
        else:
            m = n
            rest = e - n
            digits += min(rest, 77)
            rest -= digits - 1
            k = 0
            while rest:                          # values of three to ten digits
                add = min(rest, 8)
                widths[k] = 2 + add
                rest -= add
                k += 1
        for k in range(m):
            widths[k] = max(widths[k], 2)
        key = np.array([7 if w == 1 else 10 ** (w - 1) + w for w in widths], dtype=np.int64)
        assert [len(str(int(v))) for v in key] == widths and key.max() <= I32_MAX
        out.append((f"sweep{e}", key.astype(np.int32).reshape(2, d), 7 if digits == 1 else 10 ** (digits - 1) + 7))
    return out


class Fixtures:
    """the key / digest fixtures of one parameter set: names [n], family [n], vk [n][2][degree] int32, ints [n], pre [n][32] uint8"""

    def __init__(self, ps, drop=()):
        d = ps.degree
        rows = []                               # (family, name, key, digest)
        bk = base_key(ps)
        if "digest" not in drop:
            rows += [("digest", "digest:" + name, bk, v) for name, v in digest_fixtures()]
        keys = dict(key_fixtures(ps))
        if "key" not in drop:
            rows += [("key", "key:" + name, k, BASE_DIGEST) for name, k in keys.items()]
            # the shortest and the longest text there is
            rows += [("key", "key:zero/digest:0", keys["zero"], 0), ("key", "key:longest-min/digest:2^256-1", keys["longest-min"], 2 ** 256 - 1),
                     ("key", "key:longest-halfq/digest:2^256-1", keys["longest-halfq"], 2 ** 256 - 1)]
        if "sweep" not in drop:
            rows += [("sweep", "sweep:" + name[5:], k, v) for name, k, v in sweep_fixtures(ps)]
        self.ps = ps
        self.family = [r[0] for r in rows]
        self.names = [r[1] for r in rows]
        self.vk = np.stack([r[2] for r in rows]).astype(np.int32).reshape(len(rows), 2, d)
        self.ints = [int(r[3]) for r in rows]
        self.pre = np.frombuffer(b"".join(v.to_bytes(32, "little") for v in self.ints), dtype=np.uint8).reshape(len(rows), 32).copy()

    def __len__(self):
        return len(self.names)

    def sha256(self):
        """of everything the expected rows depend on (tests/golden/challenge_edges.npz carries it)"""
        h = hashlib.sha256()
        h.update("\n".join(self.names).encode())
        h.update(np.ascontiguousarray(self.vk, dtype="<i4").tobytes())
        h.update(self.pre.tobytes())
        return h.hexdigest()


@functools.lru_cache(maxsize=None)
def fixtures(set_name):
    return Fixtures(SETS[set_name])


def message_lengths():
    return list(range(0, 281)) + [RATE * k - 4 + t for k in range(3, 9) for t in (-1, 0, 1)]


LONG_MESSAGES = {100: 20000, 200: 200000}       # index in message_fixtures() -> byte length


@functools.lru_cache(maxsize=None)
def message_fixtures():
    """[(name, message str)] -- the digest is SHA3-256 of dst + "," + the message's UTF-8 bytes"""
    def ascii_of(i, n):
        return bytes(33 + (7 * i + k) % 90 for k in range(n)).decode("ascii")
    out = [(f"len{n}", ascii_of(i, n)) for i, n in enumerate(message_lengths())]
    # UTF-8 of two, three and four bytes per character with the byte length on and around len + 4 = 0 (mod 136)
    out += [("utf8-2x66", "ü" * 66), ("utf8-2x134", "ü" * 134), ("utf8-3x44", "✓" * 44), ("utf8-4x33", "\U0001f511" * 33),
            ("utf8-4x67", "\U0001f511" * 67), ("utf8-2x66-1", "ü" * 65 + "a"), ("utf8-2x66+1", "ü" * 66 + "a"),
            ("utf8-3x44+1", "✓" * 44 + "a"), ("utf8-mixed", "café ✓ \U0001f511" * 9), ("utf8-4x33-1", "\U0001f511" * 32 + "abc")]
    for at, n in sorted(LONG_MESSAGES.items()):  # among short ones: in the lane-pair forms a wave holds 32 messages
        out.insert(at, (f"long{n}", ascii_of(at, n)))
    return out


def message_keys(ps):
    n = len(message_fixtures())
    return splitmix_centered(0x5EED0000 + ps.degree, n * 2 * ps.degree).reshape(n, 2, ps.degree)


def messages_sha256(ps):
    """of the messages and their keys (tests/golden/challenge_edges.npz carries it)"""
    msgs = [m for _, m in message_fixtures()]
    return hashlib.sha256("\n".join(msgs).encode("utf-8") + np.ascontiguousarray(message_keys(ps), dtype="<i4").tobytes()).hexdigest()


def message_digest(ps, message):
    return hashlib.sha3_256(ps.sign_pre_hash_dst + b"," + message.encode("utf-8")).digest()


# ---- the model: plain Python integers and hashlib ---------------------------------------------------------------------------
def poly_text(ps, values):
    return (f"PolynomialNTTRepresentation(modulus={ps.modulus}, degree={ps.degree}, root={ps.root}, inv_root={ps.inv_root}, "
            f"root_order={ps.root_order}, values={[int(v) for v in values]})")


def vk_text(ps, left, right):
    m = "GeneralMatrix(elem_class=<class 'algebra.polynomials.PolynomialNTTRepresentation'>, matrix=[[{}]])"
    return f"OneTimeVerificationKey(left_vk_hat={m.format(poly_text(ps, left))}, right_vk_hat={m.format(poly_text(ps, right))})"


def text(ps, left, right, i):
    """what hash_vk_and_int_to_bytes hashes (fusion.py:412-419)"""
    return (ps.sign_hash_dst.decode("utf-8") + "," + vk_text(ps, left, right) + "," + str(int(i))).encode("utf-8")


def decode_shape(ps, weight=None):
    """(sign bytes, bytes per coefficient, bytes per index) of the decoder for norm bound 1"""
    w = ps.omega_ch if weight is None else weight
    return ceil(w / 8), ceil((log2(1) + 1 + ps.secpar) / 8), ceil((log2(ps.degree) + ps.secpar) / 8)


def challenge_bytes(ps):
    """the n of hash_ch (fusion.py:511-524)"""
    sb, cb, ib = decode_shape(ps)
    return sb + cb * min(ps.degree, ps.omega_ch) + ps.degree * ib


def decode(ps, b, weight=None, fault=None):
    """decode_bytes_to_polynomial_coefficients (fusion.py:422-481) for norm bound 1.  fault: "sign-bits-reversed" | "mod-i" """
    d = ps.degree
    w = ps.omega_ch if weight is None else weight
    sb, cb, ib = decode_shape(ps, w)
    assert len(b) >= sb + (cb + ib) * w
    s = int.from_bytes(b[:sb], "big")
    pos = sb
    coefs = []
    for i in range(w):
        bit = (i & ~7) | (7 - (i & 7)) if fault == "sign-bits-reversed" else i
        sign = 2 * ((s >> bit) & 1) - 1
        coefs.append(((int.from_bytes(b[pos:pos + cb], "big") % 1) + 1) * sign)
        pos += cb
    coefs += [0] * (d - len(coefs))
    if max(1, min(d, w)) < d:
        for i in range(d - 1, w, -1):
            j = int.from_bytes(b[pos:pos + ib], "big") % (i if fault == "mod-i" else i + 1)
            pos += ib
            coefs[i], coefs[j] = coefs[j], coefs[i]
    return coefs


def row(ps, left, right, i):
    """the coefficient row of hash_ch before its transform"""
    return decode(ps, hashlib.shake_256(text(ps, left, right, i)).digest(challenge_bytes(ps)))


@functools.lru_cache(maxsize=None)
def model_rows(set_name):
    """[n][degree] int32 for fixtures(set_name)"""
    ps, fx = SETS[set_name], fixtures(set_name)
    return np.array([row(ps, fx.vk[k, 0], fx.vk[k, 1], fx.ints[k]) for k in range(len(fx))], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def message_model(set_name):
    """(digests [n][32] uint8, rows [n][degree] int32) for message_fixtures() with message_keys()"""
    ps = SETS[set_name]
    vk = message_keys(ps)
    dig = [message_digest(ps, m) for _, m in message_fixtures()]
    rows = [row(ps, vk[k, 0], vk[k, 1], int.from_bytes(dg, "little")) for k, dg in enumerate(dig)]
    return np.frombuffer(b"".join(dig), dtype=np.uint8).reshape(len(dig), 32).copy(), np.array(rows, dtype=np.int32)


def aggregation_rows(ps, vk, ints, c_hat):
    """hash_vks_and_ints_and_challs_to_bytes + decode_bytes_to_agg_coefs without the transform (fusion.py:574-629): ONE stream
    over str(list(zip(keys, prehashed, challs))), cut into one piece per signer"""
    sb, cb, ib = decode_shape(ps, ps.omega_ag)
    per = sb + (cb + ib) * ps.omega_ag
    items = ", ".join(f"({vk_text(ps, k[0], k[1])}, {int(i)}, SignatureChallenge(c_hat={poly_text(ps, c)}))"
                      for k, i, c in zip(vk, ints, c_hat))
    b = hashlib.shake_256((ps.agg_xof_dst.decode("utf-8") + "," + "[" + items + "]").encode("utf-8")).digest(len(vk) * per)
    return [decode(ps, b[k * per:(k + 1) * per], ps.omega_ag) for k in range(len(vk))]


# ---- the text as the kernels build it, with a switch per fault ----------------------------------------------------------------
def _cdiv(a, b):                                # C's truncating division and remainder
    q = abs(a) // abs(b) * (1 if (a < 0) == (b < 0) else -1)
    return q, a - q * b


_P10 = [10 ** k for k in range(1, 10)]


def dec_len(v, fault=None):
    """len(str(v)) by nine comparisons u >= 10^k (dec_len of fz_challenge.hip).  fault ("dec-len-gt", k): the k-th one with > for
    >=; "abs-wraps": the magnitude kept in an int32, so that -(-2^31) stays negative"""
    u = -v if v < 0 else v
    if fault == "abs-wraps" and u > I32_MAX:
        u -= 2 ** 32
    n = (2 if v < 0 else 1) + bisect.bisect_right(_P10, u)           # how many of the nine thresholds are <= u
    if isinstance(fault, tuple) and fault[0] == "dec-len-gt" and u == 10 ** fault[1]:
        n -= 1
    return n


def u256_text(x, fault=None):
    """str(x) through chunks of base 10^9.  fault: "no-zero-padding" (inner chunks as they are), "count-nonzero-chunks",
    "top-chunk-9-wide" """
    ch = chunks_of(x)
    nch = len(ch)
    if fault == "count-nonzero-chunks":
        nch = max(1, sum(1 for c in ch if c))
    top = 9 if fault == "top-chunk-9-wide" else dec_len(ch[nch - 1])
    out = str(ch[nch - 1]).rjust(top, "0")[-top:]
    for c in range(nch - 2, -1, -1):
        out += str(ch[c]) if fault == "no-zero-padding" else str(ch[c]).rjust(9, "0")
    return out


def text_pieces(ps):
    """the fixed pieces: before the left values, between the rows, after the right values (with the "," before the digest)"""
    head = poly_text(ps, [])[:-2]               # "...values=["
    mopen = "GeneralMatrix(elem_class=<class 'algebra.polynomials.PolynomialNTTRepresentation'>, matrix=[["
    s0 = ps.sign_hash_dst.decode("utf-8") + ",OneTimeVerificationKey(left_vk_hat=" + mopen + head
    s1 = "])]]), right_vk_hat=" + mopen + head
    return s0.encode(), s1.encode(), b"])]])),"


def mech_blocks(ps, left, right, i, fault=None):
    """the padded 136-byte blocks the sponge absorbs, built as vk_text_wave builds them.  Further faults: "separator-after-left",
    "separator-after-right" (kept after the last value of that row), "pad-assigned" (the two suffix bytes stored instead of
    xor-ed), "blocks-ceil" (nb = ceil(len / 136))"""
    d = ps.degree
    vals = [int(v) for v in left] + [int(v) for v in right]
    s0, s1, s2 = text_pieces(ps)

    def sep(k):
        if (k == d - 1 and fault == "separator-after-left") or (k == 2 * d - 1 and fault == "separator-after-right"):
            return True
        return (k + 1) % d != 0
    lens = [dec_len(v, fault) + (2 if sep(k) else 0) for k, v in enumerate(vals)]
    left_total, total = sum(lens[:d]), sum(lens)
    ds = u256_text(i, fault).encode()
    at1, at2 = len(s0) + left_total, len(s0) + len(s1) + total
    at3 = at2 + len(s2)
    length = at3 + len(ds)
    buf = bytearray((length // RATE + 2) * RATE)
    pos = len(s0)
    for k, v in enumerate(vals):                # characters, last digit first
        if k == d:
            pos += len(s1)
        n = dec_len(v, fault)
        u = -v if v < 0 else v
        if fault == "abs-wraps" and u > I32_MAX:
            u -= 2 ** 32
        p = pos + n
        while True:
            u, r = _cdiv(u, 10)
            p -= 1
            buf[p] = (48 + r) & 0xff
            if not u:
                break
        if v < 0:
            p -= 1
            buf[p] = 45
        pos += n
        if sep(k):
            buf[pos:pos + 2] = b", "
            pos += 2
    buf[0:len(s0)] = s0
    buf[at1:at1 + len(s1)] = s1
    buf[at2:at2 + len(s2)] = s2
    buf[at3:at3 + len(ds)] = ds
    nb = -(-length // RATE) if fault == "blocks-ceil" else length // RATE + 1
    if fault == "pad-assigned":
        buf[length] = 0x1f
        buf[nb * RATE - 1] = 0x80
    else:
        buf[length] ^= 0x1f
        buf[nb * RATE - 1] ^= 0x80
    return bytes(buf[:nb * RATE])


def padded(t):
    """pad10*1 with SHAKE's suffix (FIPS 202): what a correct serialiser hands to the sponge for the text t"""
    nb = len(t) // RATE + 1
    buf = bytearray(t) + bytearray(nb * RATE - len(t))
    buf[len(t)] ^= 0x1f
    buf[-1] ^= 0x80
    return bytes(buf)


def _keccak_tables():
    rc, r = [], 1
    for _ in range(24):
        c = 0
        for j in range(7):
            r = ((r << 1) ^ ((r >> 7) * 0x71)) % 256
            if r & 2:
                c ^= 1 << ((1 << j) - 1)
        rc.append(c)
    rot = [[0] * 5 for _ in range(5)]
    x, y = 1, 0
    for t in range(24):
        rot[x][y] = ((t + 1) * (t + 2) // 2) % 64
        x, y = y, (2 * x + 3 * y) % 5
    return rc, rot


_RC, _ROT = _keccak_tables()
_M64 = 2 ** 64 - 1


def _rol(v, n):
    return ((v << n) | (v >> (64 - n))) & _M64 if n else v


def keccak_f(s):
    """Keccak-f[1600] on 25 lanes, lane (x, y) at s[x + 5 * y] (FIPS 202, section 3.2)"""
    for rc in _RC:
        c = [s[x] ^ s[x + 5] ^ s[x + 10] ^ s[x + 15] ^ s[x + 20] for x in range(5)]
        dd = [c[(x + 4) % 5] ^ _rol(c[(x + 1) % 5], 1) for x in range(5)]
        b = [0] * 25
        for x in range(5):
            for y in range(5):
                b[y + 5 * ((2 * x + 3 * y) % 5)] = _rol(s[x + 5 * y] ^ dd[x], _ROT[x][y])
        s = [b[k] ^ (~b[(k % 5 + 1) % 5 + 5 * (k // 5)] & _M64 & b[(k % 5 + 2) % 5 + 5 * (k // 5)]) for k in range(25)]
        s[0] ^= rc
    return s


def sponge(blocks, n):
    """absorb whole 136-byte blocks as they are (no padding added), squeeze n bytes"""
    assert len(blocks) % RATE == 0
    s = [0] * 25
    for o in range(0, len(blocks), RATE):
        for k in range(17):
            s[k] ^= int.from_bytes(blocks[o + 8 * k:o + 8 * k + 8], "little")
        s = keccak_f(s)
    out = b""
    while True:
        out += b"".join(v.to_bytes(8, "little") for v in s[:17])
        if len(out) >= n:
            return out[:n]
        s = keccak_f(s)


def mech_row(ps, left, right, i, fault=None):
    """the row a pipeline with `fault` would return"""
    dfault = fault if fault in ("sign-bits-reversed", "mod-i") else None
    return decode(ps, sponge(mech_blocks(ps, left, right, i, fault), challenge_bytes(ps)), fault=dfault)


FAULTS = ["no-zero-padding", "count-nonzero-chunks", "top-chunk-9-wide", "pad-assigned", "blocks-ceil"] + \
    [("dec-len-gt", k) for k in range(1, 10)] + \
    ["separator-after-left", "separator-after-right", "abs-wraps", "sign-bits-reversed", "mod-i"]
