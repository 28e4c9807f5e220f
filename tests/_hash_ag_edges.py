"""Fixtures that put hash_ag for many committees on the device (csrc/fz_hash_ag.hip, its entry csrc/fz_hash_ag_capi.hip) on the
edges its code depends on, and a model of the operation in plain Python.

What the code depends on, and the family that pins it:
- the committee's text is absorbed in PIECES (the fixed text in front of a polynomial and its values) written behind the tail
  the last piece left over; the SHAKE padding lands where the whole text's length puts it.  residue_cases(): committee texts of
  length 0, 1, 134 and 135 mod 136 (a whole pad block; the two ordinary ends; both suffix bits in one byte), made by changing
  the digit counts of a few c_hat values; boundary_cases(): the end of the first signer's left key values, of its right key
  values and of its whole item on a block boundary (no tail to carry).
- integers are formatted where they are stored.  value_cases(): c_hat values 0, +-1 and the centred extremes +-(q - 1) / 2 (11
  characters); pre-hashes of all-zero bytes ("0", one chunk), of 32 bytes 0xff (78 digits), and one whose decimal has an all-zero
  base-10^9 chunk in the middle.
- the stream is squeezed block by block and decoded section by section; sections are not block-aligned.  stream_cases():
  committees of 1, 2 and 3 signers; 17 and 18 signers at secpar 256 (17 * 3968 = 496 * 136: the stream ends on a block boundary)
  and 136 signers at secpar 128 (136 * 1195 is the first multiple of 136).
- layout_call(): one ragged call with groups of different sizes, one more group than a multiple of the four waves of a workgroup,
  an order list that permutes the whole row range, and rows that no group names.

The model: committee_text() is Python's str() of the integers between the fixed pieces, model_rows() is hashlib.shake_256 and the
decoder of fusion.py:422-481 restated on int.from_bytes (tests/_challenge_edges.py: a chunk sliced past the section is b"", i.e. 0).
It calls nothing of this project.  tests/test_hash_ag_edges_host.py shows that every fixture sits on the edge it claims and that
the host pipeline agrees with the model on all of them."""
import functools
import hashlib
import types

import numpy as np

from _challenge_edges import PRIME, RATE, SETS, decode, decode_shape, from_chunks, poly_text, vk_text
from oracle.oracle import splitmix_centered

WAVES = 4                                       # committees per workgroup of hash_ag_wave_kernel
HALF = (PRIME - 1) // 2


def section_bytes(ps):
    """agg_coef_bytes (fusion.py:579-585): the bytes of one signer's section"""
    sb, cb, ib = decode_shape(ps, ps.omega_ag)
    return sb + (cb + ib) * ps.omega_ag


def item_text(ps, vk, pre, c):
    return f"({vk_text(ps, vk[0], vk[1])}, {int.from_bytes(bytes(pre), 'little')}, SignatureChallenge(c_hat={poly_text(ps, c)}))"


def committee_text(ps, vk, pre, c):
    """what hash_vks_and_ints_and_challs hashes (fusion.py:632-640) for the signers in the order given"""
    items = ", ".join(item_text(ps, vk[k], pre[k], c[k]) for k in range(len(vk)))
    return (ps.agg_xof_dst.decode("utf-8") + ",[" + items + "]").encode("utf-8")


def piece_ends(ps, vk, pre, c):
    """the text lengths at which the kernel's pieces of the FIRST signer end: after the left key values, the right key values,
    the item"""
    t = committee_text(ps, vk, pre, c).decode("utf-8")
    a = t.index("values=[") + 8
    a = t.index("]", a)
    b = t.index("values=[", a) + 8
    b = t.index("]", b)
    e = len(ps.agg_xof_dst.decode("utf-8") + ",[" + item_text(ps, vk[0], pre[0], c[0]))
    return a, b, e


def model_rows(ps, vk, pre, c):
    """[N][degree] int32: the coefficient rows of hash_ag before their transform, signers in the order given"""
    n = section_bytes(ps)
    b = hashlib.shake_256(committee_text(ps, vk, pre, c)).digest(n * len(vk))
    return np.array([decode(ps, b[k * n:(k + 1) * n], weight=ps.omega_ag) for k in range(len(vk))], dtype=np.int32)


def base_rows(ps, n, seed):
    """(vk [n][2][d], pre [n][32], c [n][d]): centred rows of full width and digests with no trivial chunk"""
    d = ps.degree
    vk = splitmix_centered(0xA66 + seed, n * 2 * d).reshape(n, 2, d)
    c = splitmix_centered(0xC4A7 + seed, n * d).reshape(n, d)
    pre = np.frombuffer(hashlib.shake_256(b"hash_ag edges %d" % seed).digest(32 * n), dtype=np.uint8).reshape(n, 32).copy()
    return vk, pre, c


def _case(name, set_name, vk, pre, c, **claims):
    return types.SimpleNamespace(name=name, set=set_name, vk=np.ascontiguousarray(vk, dtype=np.int32),
                                 pre=np.ascontiguousarray(pre, dtype=np.uint8), c=np.ascontiguousarray(c, dtype=np.int32), **claims)


def _stretch(ps, vk, pre, c, row, want, length_of):
    """widen the leading values of `row` (a view into vk or c: they start as 1, one character) until length_of() = want mod 136"""
    row[:24] = 1
    delta = (want - length_of()) % RATE
    for k in range(min(24, len(row))):
        add = min(9, delta)
        row[k] = 10 ** add                      # add + 1 characters
        delta -= add
    assert delta == 0 and length_of() % RATE == want
    return vk, pre, c


@functools.lru_cache(maxsize=None)
def residue_cases(set_name):
    """committees of two signers whose whole text has length r mod 136, r = 0, 1, 134, 135"""
    ps = SETS[set_name]
    out = []
    for r in (0, 1, 134, 135):
        vk, pre, c = base_rows(ps, 2, 10 + r)
        _stretch(ps, vk, pre, c, c[1], r, lambda: len(committee_text(ps, vk, pre, c)))
        out.append(_case(f"len%136={r}", set_name, vk, pre, c, residue=r))
    return out


@functools.lru_cache(maxsize=None)
def boundary_cases(set_name):
    """committees of two signers where piece `which` of the first signer (0: left key values, 1: right key values, 2: the item)
    ends on a block boundary"""
    ps = SETS[set_name]
    out = []
    for which in range(3):
        vk, pre, c = base_rows(ps, 2, 20 + which)
        row = (vk[0, 0], vk[0, 1], c[0])[which]
        _stretch(ps, vk, pre, c, row, 0, lambda: piece_ends(ps, vk, pre, c)[which])
        out.append(_case(f"piece{which}-on-block", set_name, vk, pre, c, piece=which))
    return out


@functools.lru_cache(maxsize=None)
def value_cases(set_name):
    ps = SETS[set_name]
    d = ps.degree
    out = []
    vk, pre, c = base_rows(ps, 3, 30)
    pat = np.array([0, 1, -1, HALF, -HALF], dtype=np.int64)
    c[0] = pat[np.arange(d) % 5]
    c[1] = pat[(np.arange(d) + 2) % 5]
    c[2] = 0
    vk[1, 0] = -HALF                            # the longest left row: 11 characters everywhere
    vk[2, 1] = 0
    out.append(_case("c-extremes", set_name, vk, pre, c))
    vk, pre, c = base_rows(ps, 3, 31)
    pre[0] = 0                                  # "0": one chunk of one digit
    pre[1] = 0xff                               # 2^256 - 1: 78 digits
    ch = [(123456789 + 98765432 * j) % 10 ** 9 for j in range(8)] + [98765]
    ch[4] = 0                                   # an all-zero chunk in the middle
    pre[2] = np.frombuffer(from_chunks(ch).to_bytes(32, "little"), dtype=np.uint8)
    out.append(_case("prehash-digits", set_name, vk, pre, c, zero_chunk=4))
    return out


STREAM_SIZES = {"s128": (1, 2, 3, 136), "s256": (1, 2, 3, 17, 18), "d128w64": (1, 3), "d16": (1, 5), "d4": (1, 7)}


@functools.lru_cache(maxsize=None)
def stream_cases(set_name):
    ps = SETS[set_name]
    return [_case(f"{n}-signers", set_name, *base_rows(ps, n, 40 + n), signers=n) for n in STREAM_SIZES[set_name]]


def all_cases(set_name):
    """every committee fixture of the set (the text edges need 16 values to widen: not at degree 4)"""
    edges = residue_cases(set_name) + boundary_cases(set_name) if SETS[set_name].degree >= 16 else []
    return edges + value_cases(set_name) + stream_cases(set_name)


@functools.lru_cache(maxsize=None)
def case_rows(set_name):
    """{case name: model_rows of the case, signers in the order given}"""
    ps = SETS[set_name]
    return {k.name: model_rows(ps, k.vk, k.pre, k.c) for k in all_cases(set_name)}


@functools.lru_cache(maxsize=None)
def layout_call(set_name):
    """ONE ragged call: -> (vk [N][2][d], pre [N][32], c [N][d], order [M], off [G + 1], want [N][d]).  G = 2 * WAVES + 1 groups of
    sizes 1..4 (different sizes, the last workgroup with one wave), their rows scattered over the whole row range by a fixed
    permutation, five rows named by no group; want: the model's row for every named row, zero for the others."""
    ps = SETS[set_name]
    sizes = [3, 1, 4, 2, 1, 3, 2, 4, 1]
    assert len(sizes) == 2 * WAVES + 1
    m = sum(sizes)
    n = m + 5
    vk, pre, c = base_rows(ps, n, 50)
    perm = (np.arange(n) * 7 + 3) % n               # 7 and n = 26 are coprime
    assert sorted(perm) == list(range(n)) and not np.array_equal(perm, np.arange(n))
    order = perm[:m].astype(np.uint32)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    want = np.zeros((n, ps.degree), dtype=np.int32)
    for g in range(len(sizes)):
        rows = order[int(off[g]):int(off[g + 1])]
        want[rows] = model_rows(ps, vk[rows], pre[rows], c[rows])
    return vk, pre, c, order, off, want
