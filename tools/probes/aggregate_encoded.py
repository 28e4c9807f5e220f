"""Aggregation straight from the compact bytes (fz_aggregate_encoded_async, BatchScheme.aggregate_encoded) against the two-call
path it replaces, fz_decode_records_async followed by fz_aggregate_core, on the same box and in the same process.

  kernel  device-resident bytes, cold operands: each call reads one of enough rotating copies of the encoded batch (and of
          alpha_hat) that their sum exceeds the caches (512 MiB).  Event-timed over REPS calls, the minimum per call over ROUNDS
          rounds, the operations alternating within a round; `spread` = (max - min) / min of the per-round times of the same
          operation.  The fused CALL is four launches (the memset of the partial, aggregate_encoded, the centring pass; with
          `check` the status memset and encoded_check as well); the two-call path is decode's three and aggregate_core's.
          HBM bytes each moves per call by the byte model (records read, rows written and read again, alpha_hat read), their
          rate over that time as a fraction of 8 TB/s, and the shader clock held while the timed loop runs.
  e2e     host bytes -> aggregate on the host: aggregate_encoded(vk, msgs, bytes) against decode(device=True) + aggregate, wall
          clock, the minimum over ROUNDS runs; hash_ag's serial sponge is in both.  Device memory each holds at its peak: the sum
          of the arrays live at once, from the shapes.
Run from the repository root on a GPU box: python tools/probes/aggregate_encoded.py [all | kernel SECPAR N | e2e SECPAR N]."""
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
ROUNDS = 4
PEAK = 8.0e12
COLD_BYTES = 512 << 20


def kernel(bs, secpar, n):
    ctx, l, d = bs.ctx, bs.l, bs.d
    rows, coef, bound, w, rb = _encoding(bs.params, "signature")
    vals = n * l * d
    copies = max(2, -(-COLD_BYTES // (n * rb)))
    rng = np.random.default_rng(n)
    z = rng.integers(-bound, bound + 1, size=(n * l, d), dtype=np.int64).astype(np.int32)
    x = DeviceArray.from_numpy(ctx, ctx.ntt_forward(z))
    h = (bs.q - 1) // 2
    alpha = rng.integers(-h, h + 1, size=(n, d), dtype=np.int64).astype(np.int32)
    enc = [DeviceArray(ctx, (n, rb), np.uint8) for _ in range(copies)]
    al = [DeviceArray.from_numpy(ctx, alpha) for _ in range(copies)]
    st, rowsbuf = DeviceArray(ctx, (n,)), DeviceArray(ctx, (n * l, d))
    part, out, out2 = DeviceArray(ctx, (l, d), np.int64), DeviceArray(ctx, (l, d)), DeviceArray(ctx, (l, d))
    for k in range(copies):
        ctx.encode_records_async_dev(x.ptr, n, l, True, bound, enc[k].ptr, st.ptr)
    ctx.synchronize()
    assert not st.numpy().any()
    x.free()

    def two_call(k):
        ctx.decode_records_async_dev(enc[k].ptr, n, l, True, bound, rowsbuf.ptr, st.ptr)
        ctx.aggregate_core_dev(rowsbuf.ptr, al[k].ptr, out2.ptr, n, l)

    def fused(k):
        ctx.aggregate_encoded_async_dev(enc[k].ptr, al[k].ptr, 0, n, l, bound, part.ptr, out.ptr)

    def checked(k):
        ctx.check_records_async_dev(enc[k].ptr, n, l, bound, st.ptr)
        ctx.aggregate_encoded_async_dev(enc[k].ptr, al[k].ptr, st.ptr, n, l, bound, part.ptr, out.ptr)

    a_bytes = 4 * n * d
    ops = {
        "decode": (lambda k: ctx.decode_records_async_dev(enc[k].ptr, n, l, True, bound, rowsbuf.ptr, st.ptr), n * rb + 4 * vals),
        "decode + aggregate_core": (two_call, n * rb + 8 * vals + a_bytes),
        "aggregate_encoded": (fused, n * rb + a_bytes),
        "check + aggregate_encoded": (checked, 2 * n * rb + a_bytes),
    }
    two_call(0)
    fused(0)
    ctx.synchronize()
    assert np.array_equal(out.numpy(), out2.numpy()), "the fused entry and the two-call path disagree"
    seen = {name: [] for name in ops}
    clock = {}
    for _ in range(ROUNDS):
        for name, (fn, _) in ops.items():
            fn(0)
            ctx.synchronize()
            ctx.timer_start()
            for r in range(REPS):
                fn((r + 1) % copies)
            seen[name].append(ctx.timer_stop_ms() * 1e3 / REPS)
    for name, (fn, _) in ops.items():                     # the clock under the same loop, in a pass of its own (the probe is a launch too)
        for r in range(4 * REPS):
            fn(r % copies)
        clock[name] = ctx.diag_shader_clock(200)
        ctx.synchronize()
    print(f"secpar {secpar}  N {n} signatures  ({n * l} rows of degree {d}, w = {w}, {n * rb} encoded bytes, {copies} rotating copies)")
    for name, (_, nbytes) in ops.items():
        t = seen[name]
        best = min(t)
        print(f"  {name:26s} {best:9.2f} us per call  (spread {(max(t) - best) / best:5.1%})  {nbytes / 1e6:8.1f} MB  "
              f"{nbytes / best / 1e6:6.3f} TB/s = {nbytes / best / 1e-6 / PEAK:5.1%} of 8 TB/s   shader clock {clock[name]:6.0f} MHz")
    two, one, dec = min(seen["decode + aggregate_core"]), min(seen["aggregate_encoded"]), min(seen["decode"])
    print(f"  two-call / fused {two / one:.3f}   fused / decode alone {one / dec:.3f}   two-call / (check + fused) "
          f"{two / min(seen['check + aggregate_encoded']):.3f}")
    for b in enc + al + [st, rowsbuf, part, out, out2]:
        b.free()


def e2e(bs, secpar, n):
    l, d = bs.l, bs.d
    rows, coef, bound, w, rb = _encoding(bs.params, "signature")
    seeds = [5000 + k for k in range(n)]
    msgs = [f"probe-{k}" for k in range(n)]
    sk, vk = bs.keygen_batch(seeds)
    sig = bs.sign_batch(sk, vk, msgs)
    data, codes = bs.encode("signature", sig)
    assert not codes.any()
    blob = data.tobytes()

    def old():
        dS, c = bs.decode("signature", blob, device=True)
        try:
            return bs.aggregate(vk, msgs, dS)
        finally:
            dS.free()

    new = lambda: bs.aggregate_encoded(vk, msgs, blob)[0]
    assert np.array_equal(old(), new())
    t_old, t_new = 1e30, 1e30
    for _ in range(ROUNDS):
        t0 = time.perf_counter()
        old()
        t_old = min(t_old, time.perf_counter() - t0)
        t0 = time.perf_counter()
        new()
        t_new = min(t_new, time.perf_counter() - t0)
    t0 = time.perf_counter()
    bs.hash_ag_dev(vk, msgs)
    bs.ctx.synchronize()
    t_hash = time.perf_counter() - t0
    common = 4 * n + 4 * n * d + 4 * l * d                 # status / codes, alpha_hat, the aggregate
    m_old = n * rb + 4 * n * l * d + common + 4 * n * d    # ... + the int32 rows + c_hat (aggregate keeps it to the end)
    m_new = n * rb + common + 8 * l * d
    print(f"secpar {secpar}  N {n}: host bytes -> aggregate   decode(device=True) + aggregate {t_old * 1e3:8.2f} ms   "
          f"aggregate_encoded {t_new * 1e3:8.2f} ms   {t_old / t_new:.3f}x   (hash_ag_dev alone, one run: {t_hash * 1e3:.2f} ms)")
    print(f"  device memory live at the peak (from the shapes): {m_old / 1e6:.1f} MB against {m_new / 1e6:.1f} MB = {m_old / m_new:.2f}x")


def main(argv):
    mode = argv[0] if argv else "all"
    if mode in ("kernel", "e2e") and len(argv) == 3:
        secpar, n = int(argv[1]), int(argv[2])
        bs = BatchScheme(F.fusion_setup(secpar, 2026))
        (kernel if mode == "kernel" else e2e)(bs, secpar, n)
        bs.close()
        return
    for secpar, sizes in ((256, (64, 256, 1024, 2048)), (128, (1024,))):
        bs = BatchScheme(F.fusion_setup(secpar, 2026))
        for n in sizes:
            kernel(bs, secpar, n)
        if secpar == 256:
            e2e(bs, secpar, 1024)
        bs.close()


if __name__ == "__main__":
    main(sys.argv[1:])
