"""Many committees aggregated straight from the compact bytes in ONE launch (fz_aggregate_encoded_ragged_async,
BatchScheme.aggregate_many_encoded) against the two ways there were, on the same box and in the same process:

  A   one fz_aggregate_encoded_ragged_async call over all G groups
  B1  G calls of fz_aggregate_encoded_async, one per group
  B2  fz_decode_records_async over all records, then fz_aggregate_core_ragged on the int32 rows

  kernel  device-resident bytes, cold operands: each call reads one of enough rotating copies of the encoded batch (and of
          alpha_hat) that their sum exceeds the caches (512 MiB).  Event-timed over REPS whole calls, the minimum per call over
          ROUNDS rounds, the operations alternating within a round; `spread` = (max - min) / min of the per-round times of the
          same operation.  Every operation leaves the centred int32 aggregates of all groups.  With one group, B1 is the
          control: A should match it within its spread.
  e2e     host bytes -> aggregates on the host: aggregate_many_encoded against G calls of aggregate_encoded, wall clock, the
          minimum over ROUNDS runs; and the device memory live at the peak, from the array shapes, against decode + aggregate_many.
Run from the repository root on a GPU box: python tools/probes/aggregate_many_encoded.py [all | kernel SECPAR SHAPE | e2e SECPAR
SHAPE], SHAPE = GxN or `mix`; `all` runs every step in a process of its own and writes profiles/r16_aggregate_many_encoded.txt."""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "fusion-cryptography_amd"), ROOT):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402

REPS = 20
ROUNDS = 4
COLD_BYTES = 512 << 20
SHAPES = ("64x64", "64x16", "16x256", "mix", "1x1024")
OUT = os.path.join(ROOT, "profiles", "r16_aggregate_many_encoded.txt")


def sizes_of(shape):
    """GxN: G groups of N signers; mix: 70 groups of 1 .. 200 signers"""
    if shape == "mix":
        return [int(x) for x in np.random.default_rng(70).integers(1, 201, size=70)]
    g, n = shape.split("x")
    return [int(n)] * int(g)


def kernel(bs, secpar, shape):
    from fusion_hip import DeviceArray
    from fusion_hip.scheme import _encoding
    ctx, l, d = bs.ctx, bs.l, bs.d
    rows, coef, bound, w, rb = _encoding(bs.params, "signature")
    sizes = sizes_of(shape)
    g, n = len(sizes), sum(sizes)
    off = [0] + [int(x) for x in np.cumsum(sizes)]
    copies = max(2, -(-COLD_BYTES // (n * rb)))
    rng = np.random.default_rng(n)
    z = rng.integers(-bound, bound + 1, size=(n * l, d), dtype=np.int64).astype(np.int32)
    x = DeviceArray.from_numpy(ctx, ctx.ntt_forward(z))
    h = (bs.q - 1) // 2
    alpha = rng.integers(-h, h + 1, size=(n, d), dtype=np.int64).astype(np.int32)
    enc = [DeviceArray(ctx, (n, rb), np.uint8) for _ in range(copies)]
    al = [DeviceArray.from_numpy(ctx, alpha) for _ in range(copies)]
    st, rowsbuf = DeviceArray(ctx, (n,)), DeviceArray(ctx, (n * l, d))
    part = DeviceArray(ctx, (g, l, d), np.int64)
    outs = {name: DeviceArray(ctx, (g, l, d)) for name in ("A", "B1", "B2")}
    for k in range(copies):
        ctx.encode_records_async_dev(x.ptr, n, l, True, bound, enc[k].ptr, st.ptr)
    ctx.synchronize()
    assert not st.numpy().any()
    x.free()
    per = l * d

    def a(k):
        ctx.aggregate_encoded_ragged_async_dev(enc[k].ptr, al[k].ptr, 0, off, l, bound, part.ptr, per, outs["A"].ptr)

    def b1(k):
        for i in range(g):
            ctx.aggregate_encoded_async_dev(enc[k].ptr + off[i] * rb, al[k].ptr + off[i] * d * 4, 0, sizes[i], l, bound,
                                            part.ptr + i * per * 8, outs["B1"].ptr + i * per * 4)

    def b2(k):
        ctx.decode_records_async_dev(enc[k].ptr, n, l, True, bound, rowsbuf.ptr, st.ptr)
        ctx.aggregate_core_ragged_dev(rowsbuf.ptr, al[k].ptr, off, l, outs["B2"].ptr)

    ops = {"A  ragged, one call": a, f"B1 {g} single calls": b1, "B2 decode + core_ragged": b2}
    for fn in ops.values():
        fn(0)
    ctx.synchronize()
    want = outs["A"].numpy()
    assert np.array_equal(want, outs["B1"].numpy()) and np.array_equal(want, outs["B2"].numpy()), "the three paths disagree"
    seen = {name: [] for name in ops}
    for _ in range(ROUNDS):
        for name, fn in ops.items():
            fn(0)
            ctx.synchronize()
            ctx.timer_start()
            for r in range(REPS):
                fn((r + 1) % copies)
            seen[name].append(ctx.timer_stop_ms() * 1e3 / REPS)
    print(f"secpar {secpar}  {shape}: {g} groups, {n} signatures (sizes {min(sizes)} .. {max(sizes)}), {n * rb} encoded bytes, "
          f"{copies} rotating copies")
    best = {name: min(t) for name, t in seen.items()}
    for name, t in seen.items():
        print(f"  {name:26s} {best[name]:10.2f} us per call  (spread {(max(t) - best[name]) / best[name]:5.1%})  "
              f"{(n * rb + 4 * n * d) / best[name] / 1e6:6.3f} TB/s of records + alpha_hat")
    names = list(ops)
    rival = min(names[1:], key=lambda k: best[k])
    slack = (max(seen[rival]) - best[rival])
    print(f"  B1 / A {best[names[1]] / best[names[0]]:.3f}   B2 / A {best[names[2]] / best[names[0]]:.3f}   "
          f"A - min(B1, B2) = {best[names[0]] - best[rival]:+.2f} us against that operation's spread of {slack:.2f} us: "
          f"{'within' if best[names[0]] - best[rival] <= slack else 'SLOWER'}")
    for b in enc + al + [st, rowsbuf, part] + list(outs.values()):
        b.free()


def e2e(bs, secpar, shape):
    from fusion_hip.scheme import _encoding
    l, d = bs.l, bs.d
    rows, coef, bound, w, rb = _encoding(bs.params, "signature")
    sizes = sizes_of(shape)
    g, n = len(sizes), sum(sizes)
    off = [0] + [int(x) for x in np.cumsum(sizes)]
    seeds = [5000 + k for k in range(n)]
    msgs = [f"probe-{k}" for k in range(n)]
    sk, vk = bs.keygen_batch(seeds)
    data, codes = bs.sign_batch_encoded(sk, vk, msgs)
    assert not codes.any()
    blob = data.tobytes()
    blobs = [data[a:b].tobytes() for a, b in zip(off, off[1:])]

    def old():
        return np.stack([bs.aggregate_encoded(vk[a:b], msgs[a:b], blobs[i])[0] for i, (a, b) in enumerate(zip(off, off[1:]))])

    new = lambda: bs.aggregate_many_encoded(vk, msgs, blob, sizes)[0]
    assert np.array_equal(old(), new())
    t_old, t_new = 1e30, 1e30
    for _ in range(ROUNDS):
        t0 = time.perf_counter()
        old()
        t_old = min(t_old, time.perf_counter() - t0)
        t0 = time.perf_counter()
        new()
        t_new = min(t_new, time.perf_counter() - t0)
    common = 4 * n + 4 * n * d + 4 * g * l * d              # status / codes, alpha_hat, the aggregates
    m_rows = n * rb + 4 * n * l * d + common + 4 * n * d    # decode + aggregate_many: ... + the int32 rows + c_hat (kept to the end)
    m_new = n * rb + common + 8 * g * l * d                 # ... + the int64 partials
    print(f"secpar {secpar}  {shape}: host bytes -> {g} aggregates   {g} calls of aggregate_encoded {t_old * 1e3:8.2f} ms   "
          f"aggregate_many_encoded {t_new * 1e3:8.2f} ms   {t_old / t_new:.3f}x")
    print(f"  device memory live at the peak (from the shapes): decode + aggregate_many {m_rows / 1e6:.1f} MB against "
          f"{m_new / 1e6:.1f} MB = {m_rows / m_new:.2f}x")


def main(argv):
    mode = argv[0] if argv else "all"
    if mode in ("kernel", "e2e") and len(argv) == 3:
        import fusion.fusion as F
        from fusion_hip.scheme import BatchScheme
        secpar = int(argv[1])
        bs = BatchScheme(F.fusion_setup(secpar, 2026))
        (kernel if mode == "kernel" else e2e)(bs, secpar, argv[2])
        bs.close()
        return
    steps = [("kernel", s, shape) for s in (256, 128) for shape in SHAPES] + [("e2e", s, "64x64") for s in (256, 128)]
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        for what, secpar, shape in steps:                   # one process per step: each starts from a fresh context and a cold chip
            r = subprocess.run([sys.executable, os.path.abspath(__file__), what, str(secpar), shape], capture_output=True, text=True,
                               timeout=300)
            text = r.stdout if r.returncode == 0 else f"{what} {secpar} {shape}: exit {r.returncode}\n{r.stderr[-2000:]}\n"
            sys.stdout.write(text)
            sys.stdout.flush()
            fh.write(text)
            fh.flush()
            if r.returncode != 0:                           # nothing more on a device that a step left in an unknown state
                raise SystemExit(r.returncode)


if __name__ == "__main__":
    main(sys.argv[1:])
