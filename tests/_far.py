"""Operands past 4 GiB: the case table, the sample sets and the fault models shared by tests/test_far_offsets_host.py (CPU) and
tests/test_gpu_far_offsets.py (GPU).  Importing this module needs no GPU and no library.

Every kernel in csrc indexes with size_t, and many narrow part of the address arithmetic by hand (a scalar base plus a 32-bit
lane offset, 32-bit signer indices, `unsigned` offsets).  A byte offset kept in 32 bits, an element index kept in int or unsigned
and a count truncated on its way into the library all compute the right answer while every operand stays below 2^32 bytes.  The
thresholds an operand can cross:

    T1 = 2^32 bytes                      (a byte offset in uint32 wraps)
    T2 = 2^31 int32 elements =  8 GiB    (an element index in int32 goes negative)
    T3 = 2^32 elements       = 16 GiB    (an element index in uint32 wraps; a count in uint32 loses its top bit)

A CASE is one entry point on one route with one operand that is the SMALLEST that crosses its thresholds: the threshold plus a
ragged remainder (three rows, which at 1024-value chunks is a partial last chunk and a last workgroup with idle waves; a count
that is no multiple of 4 for the pointwise entries).  Its SAMPLE SET is the first rows, the last rows, the rows on both sides of
each crossed threshold, and for each of those the ALIAS rows a wrapped offset would land on (byte offset - 2^32, element index
- 2^31, element index - 2^32).  A FAULT MODEL maps an element index to the index a narrowed computation would use; applied to the
loads it says which input row an output row is computed from, applied to the stores which output row receives the result.

Indices no device can reach are named here once and tested nowhere: a transform task index of 2^42 (2^52 elements), a record
number of 2^32 (every record is at least 16 bytes long: 64 GiB of them, and the aggregating entries refuse N >= 2^22 long
before), a radix-4 wave-task count of 2^31 (2 TiB of degree-256 rows), a wide-path row count of 2^31 (the refusal in
fz_wide.hip; fz_wide_pw_host and fz_wide_matvec_host state no count limit at all), a group count above 65535 (the refusal in fz_capi.hip).  UNREACHABLE lists the crossings an entry's own refusal
rules out, with the refusal that proves it; tests/test_far_offsets_host.py pins those refusals on both sides of their limit."""
from collections import namedtuple

import numpy as np

GAMMA = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1
PRIME = 2147465729                 # oracle.PRIME: restated so that importing this file needs nothing (asserted equal in the CPU test)

T1_BYTES = 1 << 32
T2_ELEMS = 1 << 31
T3_ELEMS = 1 << 32
THRESHOLDS = ("T1", "T2", "T3")
CHUNK = 1024                        # int32 values per wave-task of the chunked kernels (fz_ntt_dev.h kChunk)
WAVES_PER_BLOCK = 4                 # fz_ntt_dev.h kWavesPerBlock
WINDOW_ELEMS = 4096                 # a sample window: this many elements (four chunks), at least two rows
PIECE_BYTES = 0x70000000            # the piecewise pass: no offset inside a piece reaches 2^31 bytes, and no multiple of
#                                     7 * 2^28 is 2^32, 2^33 or 2^34, so no piece boundary falls on a threshold


# ---- the synthetic stream at arbitrary element indices ---------------------------------------------------------------------------
def stream_at(seed, idx, q=PRIME):
    """values of the fz_fill_synthetic stream `seed` at the element indices `idx` (any shape, any order, up to 2^64 - 2): value i
    is SplitMix64(seed + (i + 1) * GAMMA) mod q, centred -- oracle.splitmix_centered(seed, n)[i] for i < n"""
    idx = np.asarray(idx, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed & M64) + (idx + np.uint64(1)) * np.uint64(GAMMA)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return ((z % np.uint64(q)).astype(np.int64) - (q - 1) // 2).astype(np.int32)


def stream_run(seed, first, n, q=PRIME):
    """n consecutive values from element `first` on"""
    return stream_at(seed, np.arange(first, first + n, dtype=np.uint64), q)


WIDE_Q = (1 << 61) - 1               # the wide cases' modulus (odd, below 2^63)


def wide_run(first, n):
    """n consecutive values of the wide cases' host stream from element `first` on: ((i + 1) * GAMMA mod 2^64) >> 4, less 2^59 --
    int64 in [-2^59, 2^59), inside the centred range of WIDE_Q; three passes over the array, so that 2^29 values are made in
    seconds, and indexable like stream_at"""
    i = np.arange(first + 1, first + n + 1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        i *= np.uint64(GAMMA)
    i >>= np.uint64(4)
    return i.view(np.int64) - np.int64(1 << 59)


def shifted_seed(seed, first):
    """the seed under which fz_fill_synthetic writes, from index 0 on, what stream `seed` holds from element `first` on (the rule of
    test_gpu_fullsize.py's host_rows)"""
    return (seed + first * GAMMA) & M64


# ---- the case table ---------------------------------------------------------------------------------------------------------------
# name      unique; the GPU test's parametrize id
# entry     the Context method (or module function) under test
# route     environment knobs read at context creation that choose the kernel
# degree    ring degree of the context
# operand   the argument that crosses
# unit      elements per ROW of that operand (a row is what one output row is computed from: a polynomial, a signer's key, ...)
# esize     bytes per element of that operand
# rows      rows of that operand
# count     the count handed to the C entry for that operand, and how many elements one count stands for (per_count)
# kind      "stream": output row r depends on input row r alone; "accumulate": every output value sums over all rows
# chunked   the kernel walks 1024-value chunks (a ragged remainder ends in a partial chunk and idle waves)
Case = namedtuple("Case", "name entry route degree operand unit esize rows count per_count kind chunked")


def _smallest(threshold_elems, unit, extra_rows=3):
    return -(-threshold_elems // unit) + extra_rows


def _case(name, entry, degree, operand, unit, top, route=None, kind="stream", chunked=False, per_count=None, esize=4, rows=None):
    """top: the highest threshold the operand crosses; rows default to the smallest count that crosses it"""
    elems = {"T1": T1_BYTES // esize, "T2": T2_ELEMS, "T3": T3_ELEMS}[top]
    rows = _smallest(elems, unit) if rows is None else rows
    per_count = unit if per_count is None else per_count
    assert rows * unit % per_count == 0
    return Case(name, entry, dict(route or {}), degree, operand, unit, esize, rows, rows * unit // per_count, per_count, kind, chunked)


K16 = {"FZ_NTT_KERNEL": "16"}
K4 = {"FZ_NTT_KERNEL": "4"}
PW_T3 = T3_ELEMS + 1027            # a count that is no multiple of 4 (and no multiple of the degree)
PW_T1 = (T1_BYTES // 4) + 1027

CASES = [
    # ---- crossing T1, T2 and T3 ----
    _case("fill_synthetic", "fill_synthetic_dev", 256, "out", 1, "T3", rows=PW_T3),
    _case("ntt_forward16_d256", "ntt_forward_dev", 256, "in/out", 256, "T3", K16, chunked=True, per_count=256),
    _case("ntt_inverse16_d256", "ntt_inverse_dev", 256, "in/out", 256, "T3", K16, chunked=True, per_count=256),
    _case("ntt_forward16_d64", "ntt_forward_dev", 64, "in/out", 64, "T3", K16, chunked=True, per_count=64),
    _case("ntt_inverse16_d64", "ntt_inverse_dev", 64, "in/out", 64, "T3", K16, chunked=True, per_count=64),
    _case("pw_mul", "pw_dev:OP_MUL", 256, "a/b/out", 1, "T3", rows=PW_T3),
    _case("pw_add", "pw_dev:OP_ADD", 256, "a/b/out", 1, "T3", rows=PW_T3),
    _case("pw_sub", "pw_dev:OP_SUB", 256, "a/b/out", 1, "T3", rows=PW_T3),
    _case("pw_neg", "pw_neg_dev", 256, "a/out", 1, "T3", rows=PW_T3),
    # ---- the same entries with the operand that crosses T1 alone: the quick half of each (a 16 GiB operand costs seconds) ----
    _case("fill_synthetic_t1", "fill_synthetic_dev", 256, "out", 1, "T1", rows=PW_T1),
    _case("ntt_forward16_d256_t1", "ntt_forward_dev", 256, "in/out", 256, "T1", K16, chunked=True, per_count=256),
    _case("ntt_inverse16_d256_t1", "ntt_inverse_dev", 256, "in/out", 256, "T1", K16, chunked=True, per_count=256),
    _case("ntt_forward16_d64_t1", "ntt_forward_dev", 64, "in/out", 64, "T1", K16, chunked=True, per_count=64),
    _case("ntt_inverse16_d64_t1", "ntt_inverse_dev", 64, "in/out", 64, "T1", K16, chunked=True, per_count=64),
    _case("pw_mul_t1", "pw_dev:OP_MUL", 256, "a/b/out", 1, "T1", rows=PW_T1),
    _case("pw_add_t1", "pw_dev:OP_ADD", 256, "a/b/out", 1, "T1", rows=PW_T1),
    _case("pw_sub_t1", "pw_dev:OP_SUB", 256, "a/b/out", 1, "T1", rows=PW_T1),
    _case("pw_neg_t1", "pw_neg_dev", 256, "a/out", 1, "T1", rows=PW_T1),
    # ---- crossing T1 only ----
    _case("ntt_forward4_d256", "ntt_forward_dev", 256, "in/out", 256, "T1", K4),
    _case("ntt_inverse4_d256", "ntt_inverse_dev", 256, "in/out", 256, "T1", K4),
    _case("ntt_multi_planned", "ntt_multi_dev", 256, "job 0 in/out", 256, "T1", {"FZ_MULTI_ORDER": "1"}, chunked=True),
    _case("ntt_multi_table_order", "ntt_multi_dev", 256, "job 0 in/out", 256, "T1", {"FZ_MULTI_ORDER": "0"}, chunked=True),
    _case("poly_mul_radix4", "poly_mul_dev", 256, "f/g/out", 256, "T1", {"FZ_POLYMUL_FORM": "1"}),
    _case("poly_mul_16", "poly_mul_dev", 256, "f/g/out", 256, "T1", {"FZ_POLYMUL_FORM": "2"}, chunked=True),
    _case("pw_mulacc", "pw_mulacc_dev", 256, "acc/a/b", 1, "T1", rows=PW_T1),
    _case("pw_mul_bcast", "pw_mul_bcast_dev", 256, "a/out", 256, "T1"),
    _case("matvec_sliced", "matvec_dev", 256, "S", 4 * 256, "T1"),                       # the default route at this size
    _case("matvec_fp64", "matvec_dev", 256, "S", 4 * 256, "T1", {"FZ_MATVEC_SLICES": "-1"}),
    _case("sign_core", "sign_core_dev", 256, "sk_hat", 2 * 4 * 256, "T1"),
    _case("keygen_core", "keygen_core_dev", 256, "sk_hat out", 2 * 4 * 256, "T1"),
    _case("keygen_core_bcast", "keygen_core_bcast_dev", 256, "sk_hat out", 2 * 4 * 256, "T1"),
    # compact bytes, verification-key kind (2 rows of degree 256, B = (q - 1) / 2, 31-bit fields): 2048 bytes of int32 rows and 1984
    # bytes of record per key; one case with the rows the smallest that cross, one with the bytes
    _case("encode_records_rows", "encode_records_async_dev", 256, "rows in", 512, "T1", chunked=True),
    _case("decode_records_rows", "decode_records_async_dev", 256, "rows out", 512, "T1", chunked=True),
    _case("encode_records_bytes", "encode_records_async_dev", 256, "bytes out", 1984, "T1", esize=1),
    _case("decode_records_bytes", "decode_records_async_dev", 256, "bytes in", 1984, "T1", esize=1),
    _case("check_records_bytes", "check_records_async_dev", 256, "bytes in", 1984, "T1", esize=1),
    _case("sign_encoded", "sign_encoded_async_dev", 256, "sk_hat", 2 * 3 * 256, "T1"),      # l = 3: the output's last chunk is partial
    _case("sample_secret_polys", "sample_secret_polys_dev", 256, "out", 2 * 256, "T1"),
    _case("aggregate_onepass", "aggregate_core_dev", 256, "sig", 4 * 256, "T1", {"FZ_AGG_DIRECT": "-1"}, kind="accumulate"),
    _case("aggregate_direct4", "aggregate_core_dev", 256, "sig", 4 * 256, "T1", {"FZ_AGG_DIRECT": "4"}, kind="accumulate"),
    # signature records of l = 4 rows at the widest bound: 31-bit fields, 3968 bytes per record
    _case("aggregate_encoded", "aggregate_encoded_async_dev", 256, "bytes", 3968, "T1", esize=1, kind="accumulate"),
    _case("verify_encoded", "verify_encoded_async_dev", 256, "bytes", 3968, "T1", esize=1),
    # the wide path: 8-byte values, entries that take HOST arrays (2^29 values are 4 GiB on the host and on the device)
    _case("wide_ntt", "WideContext.ntt_forward", 256, "in/out", 256, "T1", esize=8),
    _case("wide_pw", "WideContext.pw_mul", 256, "a/b/out", 1, "T1", esize=8, rows=(T1_BYTES // 8) + 1027),
]
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)

# the quick half of a three-threshold case: <name>_t1 beside <name>
QUICK = {c.name: c.name[:-3] for c in CASES if c.name.endswith("_t1")}
assert all(v in CASE for v in QUICK.values())

# crossings an entry's own refusal keeps out of reach: (entry, what would have to be crossed, the refusal that rules it out)
UNREACHABLE = [
    ("aggregate_core_dev", "a signer index of 2^21 (T2 at l = 4, degree 256 is exactly 2^21 signers)", "fz_aggregate_core: N < 2^21"),
    ("aggregate_encoded_async_dev", "a signer index past 2^22", "fz_aggregate_encoded_async: N < 2^22 (FZ_E_UNSUPPORTED)"),
    ("aggregate_encoded_ragged_async_dev", "a 32-bit signer index wrapping", "fz_aggregate_encoded_ragged_async: total < 0xffffffc0"),
    ("encode/decode/check_records_async_dev", "an element offset inside one record past 2^31", "records_args: rows * degree <= 0x7fffffff"),
    ("ntt_multi_dev", "a job of 2^31 rows (the row count shares its word with the direction bit)", "fz_ntt_multi: rows < 2^31"),
    ("*_batch_dev", "a group index past the grid's y/z limit", "groups <= 65535"),
    ("keygen_core_dev (fused)", "a segment count past int32", "batch * 2 <= 0x7fffffff, else the two-launch form"),
]


def elems(case):
    return case.rows * case.unit


def nbytes(case):
    return elems(case) * case.esize


def crossed(case):
    """the thresholds the operand crosses, as {name: first element index at or past it}"""
    out = {}
    if nbytes(case) > T1_BYTES:
        out["T1"] = T1_BYTES // case.esize
    if elems(case) > T2_ELEMS:
        out["T2"] = T2_ELEMS
    if elems(case) > T3_ELEMS:
        out["T3"] = T3_ELEMS
    return out


def excess(case):
    """by how many elements the operand exceeds each crossed threshold"""
    return {t: elems(case) - e for t, e in crossed(case).items()}


# ---- the sample set ---------------------------------------------------------------------------------------------------------------
def windows(case):
    """-> sorted, disjoint (first_row, n_rows): the first and last rows, the rows on both sides of each crossed threshold, and the
    alias rows of all of those (byte offset - 2^32, element index - 2^31, element index - 2^32) wherever such a row exists"""
    w = max(2, WINDOW_ELEMS // case.unit)
    rows = case.rows
    base = [(0, w), (rows - w, rows)]
    for e in crossed(case).values():
        r = e // case.unit
        base.append((max(0, r - w), min(rows, r + w)))
    spans = list(base)
    for lo, hi in base:
        for shift in (T1_BYTES // case.esize, T2_ELEMS, T3_ELEMS):
            a_lo, a_hi = lo - -(-shift // case.unit), hi - shift // case.unit      # (every row the shifted window touches)
            if a_hi > 0 and a_lo < rows:
                spans.append((max(0, a_lo), min(rows, a_hi)))
    spans.sort()
    merged = []
    for lo, hi in spans:
        if hi <= lo:
            continue
        if merged and lo <= merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], hi)
        else:
            merged.append([lo, hi])
    return [(lo, hi - lo) for lo, hi in merged]


def sampled_rows(case):
    return np.concatenate([np.arange(lo, lo + n, dtype=np.int64) for lo, n in windows(case)])


def pieces(case, unit=None):
    """-> (first_row, n_rows) of the piecewise pass over the crossing operand: whole rows, at most PIECE_BYTES each"""
    unit = case.unit if unit is None else unit
    per = PIECE_BYTES // (unit * case.esize)
    return [(lo, min(per, case.rows - lo)) for lo in range(0, case.rows, per)]


# ---- fault models ---------------------------------------------------------------------------------------------------------------
OUTSIDE = -1          # the narrowed index points outside the buffer (a negative int32 index)
UNTOUCHED = -2        # the element is never reached (a truncated count)
MODELS = ("u32_bytes", "i32_elems", "u32_elems", "count_u32")


def applies(model, case):
    """can the narrowing change anything for this operand?"""
    if model == "u32_bytes":
        return nbytes(case) > T1_BYTES
    if model == "i32_elems":
        return elems(case) > T2_ELEMS
    if model == "u32_elems":
        return elems(case) > T3_ELEMS
    if model == "count_u32":
        return case.count >= 1 << 32
    raise KeyError(model)


def narrowed(model, case, e):
    """element indices e (int64 array) -> the index the narrowed computation uses (or OUTSIDE / UNTOUCHED)"""
    e = np.asarray(e, dtype=np.int64)
    if model == "u32_bytes":
        return (e * case.esize % (1 << 32)) // case.esize
    if model == "i32_elems":
        low = e % (1 << 32)
        return np.where(low >= 1 << 31, OUTSIDE, low)
    if model == "u32_elems":
        return e % (1 << 32)
    if model == "count_u32":
        return np.where(e < (case.count % (1 << 32)) * case.per_count, e, UNTOUCHED)
    raise KeyError(model)


def row_map(model, case, rows):
    """rows (int64 array) -> for each, the row its first element is narrowed to (OUTSIDE / UNTOUCHED kept).  With the model on the
    LOADS, output row r is computed from input row row_map(r); on the STORES, the result of row r lands in row row_map(r) and
    row r keeps its poison."""
    rows = np.asarray(rows, dtype=np.int64)
    f = narrowed(model, case, rows * case.unit)
    return np.where(f >= 0, f // case.unit, f)


def wrong_rows(model, case, rows, side):
    """which of `rows` hold something other than their own result under the model applied to `side` ("load" or "store")?
    load: every row whose source is not itself.  store: those rows (they keep their poison) and the rows that receive another
    row's result."""
    rows = np.asarray(rows, dtype=np.int64)
    moved = row_map(model, case, rows) != rows
    if side == "load":
        return rows[moved]
    assert side == "store"
    # a sampled row a receives a foreign result if some row r != a of the operand narrows to it: r = a + k * period
    hit = np.zeros(rows.shape, bool)
    if model != "count_u32":
        for shift in ((T1_BYTES // case.esize,) if model == "u32_bytes" else (T3_ELEMS,)):
            for k in range(1, elems(case) // shift + 1):
                src = rows * case.unit + k * shift
                ok = src < elems(case)
                f = narrowed(model, case, np.where(ok, src, 0))
                hit |= ok & (f == rows * case.unit)
    return rows[moved | hit]


def accumulate_column(case, seed_sig, seed_alpha, k, j, l, q=PRIME, model=None, keep=None):
    """one coefficient of an aggregate over ALL signers with the indexable stream: sum_i sig[i][k][j] * alpha[i][j] mod q, centred;
    int64, reduced after every product.  With a model, the signature row index is narrowed as a load would narrow it; keep
    [signers] bool: the signers that count (a skip mask's complement)."""
    d = case.degree
    i = np.arange(case.rows, dtype=np.int64)
    e = i * case.unit + k * d + j
    if model is not None:
        f = narrowed(model, case, i * case.unit)
        e = np.where(f >= 0, f + k * d + j, 0)
    s = stream_at(seed_sig, e.astype(np.uint64), q).astype(np.int64)
    a = stream_at(seed_alpha, (i * d + j).astype(np.uint64), q).astype(np.int64)
    prod = (s * a) % q
    t = int((prod if keep is None else prod[np.asarray(keep, bool)]).sum() % q)
    return t - q if t > q // 2 else t
