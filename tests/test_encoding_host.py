"""The compact byte encoding of keys, signatures and aggregates, on the CPU: the record lengths and
field widths of the format table, a numpy restatement of the format (the spec the device kernels are held to in
tests/test_gpu_encoding.py) checked on random fields and against the digests of the golden objects in tests/golden/encoding.json,
and the register budget of the new kernels."""
import hashlib
import json
import os
import re
import types

import numpy as np
import pytest

G = os.path.join(os.path.dirname(__file__), "golden")

# kind -> secpar -> (rows, B, w, record bytes), the table of INTEGRATION.md section G
TABLE = {
    "vk": {128: (2, 1073732864, 31, 496), 256: (2, 1073732864, 31, 1984)},
    "signature": {128: (195, 4264, 14, 21840), 256: (83, 3172, 13, 34528)},
    "aggregate": {128: (195, 536070080, 30, 46800), 256: (83, 536321760, 30, 79680)},
}


def params_of(secpar):
    """the attributes the encoding reads, without a device (fusion_setup samples its public challenge on the GPU)"""
    from oracle.oracle import PARAMS
    P = PARAMS[secpar]
    return types.SimpleNamespace(secpar=secpar, modulus=P["q"], degree=P["d"], num_rows_sk=P["rank"], beta_vf=P["beta_vf"])


# ---- the spec: numpy, no device ------------------------------------------------------------------------------------------
def spec_kind(secpar, kind):
    rows, B, w, rb = TABLE[kind][secpar]
    return rows, B, w, rb


def spec_values(secpar, kind, rows):
    """the centred integers z of every record: [N][rows][d] int64 (vk: the stored values mod q, centred; else cent(INTT(row)))"""
    from oracle.oracle import PARAMS, py_cent, py_ntt_inverse, py_twiddles
    P = PARAMS[secpar]
    q = P["q"]
    rows = np.asarray(rows, dtype=np.int64)
    if kind == "vk":
        return (rows + q // 2) % q - q // 2
    itw = py_twiddles(P["inv_root"], q, P["d"])
    flat = rows.reshape(-1, P["d"])
    out = np.array([py_ntt_inverse([py_cent(int(v), q) for v in r], q, itw) for r in flat], dtype=np.int64)
    return out.reshape(rows.shape)


def spec_pack(z, B, w):
    """[N][rows][d] centred integers -> [N][record bytes] uint8: fields u = z + B of w bits, row-major, LSB first"""
    z = np.asarray(z, dtype=np.int64)
    n = z.shape[0]
    u = z.reshape(n, -1) + B
    if (u < 0).any() or (u > 2 * B).any():
        raise ValueError("a value is outside [-B, B]")
    bits = ((u[..., None] >> np.arange(w, dtype=np.int64)) & 1).astype(np.uint8)          # [N][fields][w], bit 0 first
    return np.packbits(bits.reshape(n, -1), axis=1, bitorder="little")


def spec_unpack(b, B, w, shape):
    """[N][record bytes] uint8 -> [N][rows][d] int64, or ValueError when a field is above 2B"""
    b = np.asarray(b, dtype=np.uint8)
    n = b.shape[0]
    bits = np.unpackbits(b, axis=1, bitorder="little").reshape(n, -1, w).astype(np.int64)
    u = bits @ (np.int64(1) << np.arange(w, dtype=np.int64))
    if (u > 2 * B).any():
        raise ValueError("a field is above 2B")
    return (u - B).reshape((n,) + tuple(shape))


def spec_encode(secpar, kind, rows):
    _, B, w, _ = spec_kind(secpar, kind)
    return spec_pack(spec_values(secpar, kind, rows), B, w)


GOLDEN_OBJECTS = {"vk": ("vk", "vk"), "sig": ("signature", "sig"), "agg_4": ("aggregate", "agg_4")}


def golden_rows(secpar, name):
    S = np.load(os.path.join(G, f"scheme_{secpar}.npz"))
    a = S[name]
    return a[None] if name.startswith("agg") else a


# ---- tests -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("secpar", [128, 256])
def test_encoded_size_reproduces_the_format_table(secpar):
    from fusion_hip.scheme import _encoding, encoded_size
    p = params_of(secpar)
    for kind, by in TABLE.items():
        rows, B, w, rb = by[secpar]
        assert encoded_size(p, kind) == rb
        assert _encoding(p, kind)[:5] == (rows, kind != "vk", B, w, rb)
        assert (2 * B).bit_length() == w and rows * p.degree * w % 8 == 0 and rb % 16 == 0
    # 13 of the 32 bits of an int32 value at secpar 256: the 2.46x of the issue
    assert round(p.num_rows_sk * p.degree * 4 / encoded_size(p, "signature"), 2) == (2.29 if secpar == 128 else 2.46)


def test_encoded_size_refuses_unknown_kinds_and_secpars():
    from fusion_hip import FusionHipError
    from fusion_hip._lib import FZ_E_BADARG
    from fusion_hip.scheme import encoded_size
    for kind in ("sk", "Signature", "", None):
        with pytest.raises(FusionHipError) as e:
            encoded_size(params_of(256), kind)
        assert e.value.code == FZ_E_BADARG
    other = params_of(256)
    other.secpar = 192
    for kind in TABLE:
        with pytest.raises(FusionHipError) as e:
            encoded_size(other, kind)
        assert e.value.code == FZ_E_BADARG


@pytest.mark.parametrize("secpar", [128, 256])
@pytest.mark.parametrize("kind", sorted(TABLE))
def test_spec_round_trips_in_range_fields_and_refuses_the_rest(secpar, kind):
    rows, B, w, rb = TABLE[kind][secpar]
    d = params_of(secpar).degree
    rng = np.random.default_rng(secpar + len(kind))
    z = rng.integers(-B, B + 1, size=(3, rows, d), dtype=np.int64)
    z[0, 0, 0], z[1, -1, -1], z[2, 0, 1] = B, -B, 0
    b = spec_pack(z, B, w)
    assert b.shape == (3, rb)
    assert np.array_equal(spec_unpack(b, B, w, (rows, d)), z)
    assert np.array_equal(spec_pack(spec_unpack(b, B, w, (rows, d)), B, w), b)
    # the first and the last field of a record sit in its first and last bits
    assert (int(b[0, 0]) | int(b[0, 1]) << 8 | int(b[0, 2]) << 16 | int(b[0, 3]) << 24) & ((1 << w) - 1) == 2 * B
    for bad in (B + 1, -B - 1):
        zz = z.copy()
        zz[1, 0, 0] = bad
        with pytest.raises(ValueError):
            spec_pack(zz, B, w)
    # every field value above 2B is refused, wherever it sits: 2B + 1, 2^w - 1 and one between
    for u in sorted({2 * B + 1, (2 * B + 1 + (1 << w) - 1) // 2, (1 << w) - 1}):
        for j in (0, rows * d // 2, rows * d - 1):
            bits = np.unpackbits(b[1:2], bitorder="little").reshape(-1, w)
            bits[j] = (u >> np.arange(w)) & 1
            bb = np.packbits(bits.reshape(1, -1), axis=1, bitorder="little")
            with pytest.raises(ValueError):
                spec_unpack(bb, B, w, (rows, d))


@pytest.mark.parametrize("secpar", [128, 256])
def test_spec_digests_of_the_golden_objects(secpar):
    with open(os.path.join(G, "encoding.json")) as fh:
        want = json.load(fh)[str(secpar)]
    assert sorted(want) == sorted(GOLDEN_OBJECTS)
    for name, (kind, key) in GOLDEN_OBJECTS.items():
        rows, B, w, rb = TABLE[kind][secpar]
        r = golden_rows(secpar, key)
        b = spec_encode(secpar, kind, r)
        assert b.shape == (r.shape[0], rb)
        assert hashlib.sha3_256(b.tobytes()).hexdigest() == want[name], (secpar, name)
        # the stored rows come back: NTT(z) == rows (mod q) -- decode's half, checked through the forward transform
        if kind == "vk":
            from oracle.oracle import PARAMS
            q = PARAMS[secpar]["q"]
            assert np.array_equal(spec_unpack(b, B, w, (rows, r.shape[-1])), (r.astype(np.int64) + q // 2) % q - q // 2)


def test_spec_decode_is_the_forward_transform_of_the_fields():
    from oracle.oracle import PARAMS, py_cent, py_ntt_forward, py_twiddles
    P = PARAMS[256]
    q, d = P["q"], P["d"]
    r = golden_rows(256, "sig")[:1, :3]
    z = spec_values(256, "signature", r)
    tw = py_twiddles(P["root"], q, d)
    back = np.array([py_ntt_forward([int(v) for v in row], q, tw) for row in z.reshape(-1, d)]).reshape(r.shape)
    assert np.array_equal(back, r)
    assert all(py_cent(int(v), q) == int(v) for v in back.ravel()[:64])


def test_record_kernels_compile_without_spills():
    """records_encode / records_decode / records_zero_failed: degrees 64 and 256 x both multiplies for the coefficient kinds, one
    instantiation each for keys; no spill, no scratch, and no more LDS than the transforms (lds16_doubles)"""
    from _isa import asm, assert_fits_transforms, metadata
    records = metadata(asm("fz_records"), "records_")
    assert len([k for k in records if "records_encode" in k]) == 5, sorted(records)
    assert len([k for k in records if "records_decode" in k]) == 5, sorted(records)
    assert len([k for k in records if "records_zero_failed" in k]) == 1, sorted(records)
    assert_fits_transforms(records, r"records_(?:encode|decode)ILi(\d)E", "ntt_inv16|ntt_fwd16")
