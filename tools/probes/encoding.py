"""The compact byte encoding (BatchScheme.encode / decode): the kernels against the transforms they
contain, and what the smaller form saves on the host link.

  kernel  encode ("signature") against fz_ntt_inverse over the same rows, decode against fz_ntt_forward, at secpar 256 with
          N = 1024 and 4096 signatures and at secpar 128 with N = 1024.  Cold operands: each launch reads one of enough rotating
          copies that their sum exceeds the caches (512 MiB).  Event-timed over REPS calls, the minimum per call over ROUNDS
          rounds, the four operations alternating within a round.  An encode or decode CALL is three launches (the status
          memset, the records kernel, records_zero_failed); the transforms are one.  Bytes moved per call (rows read + bytes
          written, or the reverse) over that time, and its fraction of 8 TB/s.
  e2e     host bytes -> device rows (upload of the encoded batch + decode) against the upload of the same rows as int32, both
          synchronised, wall clock, the minimum over ROUNDS * 5 runs.
  summary the kernel durations of a `rocprofv3 --kernel-trace --output-format csv` run of ONE size
          (`kernel SECPAR N`): per kernel the number of dispatches, the median and the minimum, records kernels, transforms
          (ntt_inv16 / ntt_fwd16, or the radix-4 ntt_inv4 / ntt_fwd4 fz_ntt_* picks below 2^19 rows of degree 64) and the
          memset, and the kernel-only ratios.
Run from the repository root on a GPU box: python tools/probes/encoding.py [all | kernel SECPAR N | e2e | summary TRACE_CSV]."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "fusion-cryptography_amd"), ROOT):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import fusion.fusion as F  # noqa: E402
from fusion_hip import DeviceArray  # noqa: E402
from fusion_hip.scheme import BatchScheme, _encoding  # noqa: E402

REPS = 20
ROUNDS = 3
PEAK = 8.0e12
COLD_BYTES = 512 << 20


def kernel(bs, secpar, n):
    ctx, l, d = bs.ctx, bs.l, bs.d
    rows, coef, bound, w, rb = _encoding(bs.params, "signature")
    vals = n * l * d
    copies = max(2, -(-COLD_BYTES // (vals * 4)))
    rng = np.random.default_rng(n)
    z = rng.integers(-bound, bound + 1, size=(n * l, d), dtype=np.int64).astype(np.int32)
    x = ctx.ntt_forward(z)
    src = [DeviceArray.from_numpy(ctx, x) for _ in range(copies)]
    dst = [DeviceArray(ctx, (n * l, d)) for _ in range(copies)]
    enc = [DeviceArray(ctx, (n, rb), np.uint8) for _ in range(copies)]
    st = DeviceArray(ctx, (n,))
    for k in range(copies):
        ctx.encode_records_async_dev(src[k].ptr, n, l, True, bound, enc[k].ptr, st.ptr)
    ctx.synchronize()
    assert not st.numpy().any()
    ops = {                                                  # encode / decode: the whole call, three launches (see the header)
        "ntt_inverse": (lambda k: ctx.ntt_inverse_dev(src[k].ptr, dst[k].ptr, n * l), 8 * vals),
        "encode": (lambda k: ctx.encode_records_async_dev(src[k].ptr, n, l, True, bound, enc[k].ptr, st.ptr), 4 * vals + n * rb),
        "ntt_forward": (lambda k: ctx.ntt_forward_dev(src[k].ptr, dst[k].ptr, n * l), 8 * vals),
        "decode": (lambda k: ctx.decode_records_async_dev(enc[k].ptr, n, l, True, bound, dst[k].ptr, st.ptr), 4 * vals + n * rb),
    }
    best = {}
    for _ in range(ROUNDS):
        for name, (fn, _) in ops.items():
            fn(0)
            ctx.synchronize()
            ctx.timer_start()
            for r in range(REPS):
                fn((r + 1) % copies)
            us = ctx.timer_stop_ms() * 1e3 / REPS
            best[name] = min(best.get(name, 1e30), us)
    print(f"secpar {secpar}  N {n} signatures  ({n * l} rows of degree {d}, w = {w}, {n * rb} encoded bytes against "
          f"{4 * vals} int32 bytes: {4 * vals / (n * rb):.2f}x; {copies} rotating copies)")
    for name, (_, nbytes) in ops.items():
        print(f"  {name:12s} {best[name]:9.2f} us per call   {nbytes / 1e6:8.1f} MB   {nbytes / best[name] / 1e6:7.3f} TB/s "
              f"= {nbytes / best[name] / 1e-6 / PEAK:5.1%} of 8 TB/s")
    print(f"  ratio encode / ntt_inverse {best['encode'] / best['ntt_inverse']:.3f}   decode / ntt_forward "
          f"{best['decode'] / best['ntt_forward']:.3f}")
    for b in src + dst + enc + [st]:
        b.free()


def e2e(bs, secpar, n):
    ctx, l, d = bs.ctx, bs.l, bs.d
    rows, coef, bound, w, rb = _encoding(bs.params, "signature")
    rng = np.random.default_rng(7)
    z = rng.integers(-bound, bound + 1, size=(n * l, d), dtype=np.int64).astype(np.int32)
    x = ctx.ntt_forward(z).reshape(n, l, d)
    data, codes = bs.encode("signature", x)
    assert not codes.any()
    blob = data.tobytes()
    dR, dB, st = DeviceArray(ctx, (n, l, d)), DeviceArray(ctx, (n, rb), np.uint8), DeviceArray(ctx, (n,))
    t_int, t_bytes = 1e30, 1e30
    for _ in range(ROUNDS * 5):
        t0 = time.perf_counter()
        ctx.h2d(dR.ptr, x)                                   # h2d synchronises
        t_int = min(t_int, time.perf_counter() - t0)
        t0 = time.perf_counter()
        ctx.h2d(dB.ptr, np.frombuffer(blob, dtype=np.uint8))
        ctx.decode_records_async_dev(dB.ptr, n, l, True, bound, dR.ptr, st.ptr)
        ctx.synchronize()
        t_bytes = min(t_bytes, time.perf_counter() - t0)
    assert np.array_equal(dR.numpy(), x)
    print(f"secpar {secpar}  N {n}: host -> device rows  int32 upload {t_int * 1e3:8.3f} ms ({x.nbytes / 1e6:.1f} MB)   "
          f"bytes upload + decode {t_bytes * 1e3:8.3f} ms ({len(blob) / 1e6:.1f} MB)   {t_int / t_bytes:.2f}x")
    for b in (dR, dB, st):
        b.free()


def summary(path):
    import csv
    import re
    times = {}
    with open(path) as fh:
        for r in csv.DictReader(fh):
            name = r["Kernel_Name"]
            m = re.search(r"::(\w+(?:<[^>]*>)?)\(", name)
            key = m.group(1) if m else name.split("(")[0]
            times.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    med = {}
    for key in sorted(times):
        if not re.search(r"records_|ntt_inv|ntt_fwd|fillBuffer", key):
            continue
        t = np.array(times[key])
        med[key] = float(np.median(t))
        print(f"  {key:40s} {len(t):5d} dispatches   median {np.median(t):9.2f} us   min {t.min():9.2f} us")
    def pick(pat):                              # the instantiation dispatched most often (set-up transforms take others)
        keys = [k for k in med if re.search(pat, k)]
        return med[max(keys, key=lambda k: len(times[k]))] if keys else None
    for a, b in ((r"records_encode<\d, \w+, true>", r"ntt_inv"), (r"records_decode<\d, \w+, true>", r"ntt_fwd")):
        ta, tb = pick(a), pick(b)
        if ta and tb:
            print(f"  kernel-only median ratio {a.split('<')[0]} / {b}: {ta / tb:.3f}")


def main(argv):
    mode = argv[0] if argv else "all"
    if mode == "summary":
        summary(argv[1])
        return
    if mode == "kernel" and len(argv) == 3:
        secpar, n = int(argv[1]), int(argv[2])
        bs = BatchScheme(F.fusion_setup(secpar, 2026))
        kernel(bs, secpar, n)
        bs.close()
        return
    for secpar, sizes in ((256, (1024, 4096)), (128, (1024,))):
        bs = BatchScheme(F.fusion_setup(secpar, 2026))
        if mode in ("all", "kernel"):
            for n in sizes:
                kernel(bs, secpar, n)
        if mode in ("all", "e2e"):
            for n in sizes:
                e2e(bs, secpar, n)
        bs.close()


if __name__ == "__main__":
    main(sys.argv[1:])
