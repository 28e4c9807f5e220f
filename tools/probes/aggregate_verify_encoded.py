"""Aggregates AND verification targets of many committees straight from the compact bytes in ONE launch
(fz_aggregate_target_encoded_ragged_async; BatchScheme.aggregate_verify_encoded / aggregate_verify_many_encoded) against what there
was, on the same box and in the same process:

  kernel  A  one fz_aggregate_target_encoded_ragged_async call: both kinds of int64 partials and the centred aggregates
          P  the pair it replaces: fz_aggregate_encoded_ragged_async, then fz_aggregate_target_partial_ragged(d_sig = NULL)
          Device-resident operands, cold: each call reads one of enough rotating copies of the encoded batch, alpha_hat, the keys
          and c_hat that their sum exceeds the caches (512 MiB).  Event-timed over REPS whole calls, ROUNDS rounds, the two
          operations alternating within a round; reported per operation: the minimum, and the spread max - min of its rounds.
          Requirement: A's minimum is not above P's by more than P's own spread.  Both leave the same sums, bit for bit.
  e2e     host bytes -> aggregates and verdicts on the host, wall clock, the minimum of ROUNDS runs:
          aggregate_verify_encoded against aggregate_encoded + verify (one committee), aggregate_verify_many_encoded against
          aggregate_many_encoded + verify_many (many); beside the saving, what one hash_ag per committee and one challenge pass
          cost alone in the same process (the expected saving), and the device memory live at the peak, from the array shapes.
Run from the repository root on a GPU box: python tools/probes/aggregate_verify_encoded.py [all | kernel SECPAR SHAPE | e2e SECPAR
SHAPE], SHAPE = GxN or `mix`; `all` runs every step in a process of its own and writes profiles/r23_aggregate_verify_encoded.txt."""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "fusion-cryptography_amd"), ROOT):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402

REPS = 20
ROUNDS = 5
E2E_ROUNDS = 4
COLD_BYTES = 512 << 20
SHAPES = ("1x1024", "16x256", "64x64", "64x16", "mix")
E2E_SHAPES = ("1x1024", "64x64", "64x16")
OUT = os.path.join(ROOT, "profiles", "r23_aggregate_verify_encoded.txt")


def sizes_of(shape):
    """GxN: G groups of N signers; mix: 70 groups of 1 .. 194 signers (DESIGN.md section 5.16's)"""
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
    copies = max(2, -(-COLD_BYTES // (n * (rb + 16 * d))))
    rng = np.random.default_rng(n)
    z = rng.integers(-bound, bound + 1, size=(n * l, d), dtype=np.int64).astype(np.int32)
    x = DeviceArray.from_numpy(ctx, ctx.ntt_forward(z))
    h = (bs.q - 1) // 2
    alpha, chal = (rng.integers(-h, h + 1, size=(n, d), dtype=np.int64).astype(np.int32) for _ in range(2))
    vk = rng.integers(-h, h + 1, size=(n, 2, d), dtype=np.int64).astype(np.int32)
    enc = [DeviceArray(ctx, (n, rb), np.uint8) for _ in range(copies)]
    al, ch, kk = ([DeviceArray.from_numpy(ctx, a) for _ in range(copies)] for a in (alpha, chal, vk))
    kl, kr = ([DeviceArray.from_numpy(ctx, np.ascontiguousarray(vk[:, i])) for _ in range(copies)] for i in (0, 1))      # the pair's split keys
    st = DeviceArray(ctx, (n,))
    per = l * d
    res = {name: (DeviceArray(ctx, (g, per), np.int64), DeviceArray(ctx, (g, d), np.int64), DeviceArray(ctx, (g, per))) for name in "AP"}
    for k in range(copies):
        ctx.encode_records_async_dev(x.ptr, n, l, True, bound, enc[k].ptr, st.ptr)
    ctx.synchronize()
    assert not st.numpy().any()
    x.free()

    def a(k):
        p, t, o = res["A"]
        ctx.aggregate_target_encoded_ragged_async_dev(enc[k].ptr, al[k].ptr, 0, kk[k].ptr, ch[k].ptr, off, l, bound, p.ptr, per, t.ptr, d, o.ptr)

    def pair(k):
        p, t, o = res["P"]
        ctx.aggregate_encoded_ragged_async_dev(enc[k].ptr, al[k].ptr, 0, off, l, bound, p.ptr, per, o.ptr)
        ctx.aggregate_target_partial_ragged_dev(0, al[k].ptr, kl[k].ptr, kr[k].ptr, ch[k].ptr, off, l, 0, 0, t.ptr, d)

    ops = {"A  one launch": a, "P  the pair": pair}
    for fn in ops.values():
        fn(0)
    ctx.synchronize()
    for u, v in zip(res["A"], res["P"]):
        assert np.array_equal(u.numpy(), v.numpy()), "the two paths disagree"
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
          f"{copies} rotating copies, {ROUNDS} rounds of {REPS} calls")
    best = {name: min(t) for name, t in seen.items()}
    for name, t in seen.items():
        print(f"  {name:16s} {best[name]:10.2f} us per call  (spread max - min {max(t) - best[name]:7.2f} us)")
    na, npair = list(ops)
    slack = max(seen[npair]) - best[npair]
    diff = best[na] - best[npair]
    print(f"  P / A {best[npair] / best[na]:.3f}   A - P = {diff:+.2f} us against P's spread of {slack:.2f} us: "
          f"{'not slower' if diff <= 0 else 'within' if diff <= slack else 'SLOWER'}")
    for b in enc + al + ch + kk + kl + kr + [st] + [y for r in res.values() for y in r]:
        b.free()


def e2e(bs, secpar, shape):
    from fusion_hip.context import DeviceScope
    from fusion_hip.scheme import _Committees, _encoding
    l, d = bs.l, bs.d
    rows, coef, bound, w, rb = _encoding(bs.params, "signature")
    sizes = sizes_of(shape)
    g, n = len(sizes), sum(sizes)
    seeds = [5000 + k for k in range(n)]
    msgs = [f"probe-{k}" for k in range(n)]
    sk, vk = bs.keygen_batch(seeds)
    data, codes = bs.sign_batch_encoded(sk, vk, msgs)
    assert not codes.any()
    blob = data.tobytes()
    if g == 1:
        def old():
            agg, c = bs.aggregate_encoded(vk, msgs, blob)
            return agg[None], [bs.verify(vk, msgs, agg)]

        def new():
            agg, c, v = bs.aggregate_verify_encoded(vk, msgs, blob)
            return agg[None], [v]
        names = "aggregate_encoded + verify", "aggregate_verify_encoded"
    else:
        def old():
            aggs, c = bs.aggregate_many_encoded(vk, msgs, blob, sizes)
            return aggs, bs.verify_many(vk, msgs, aggs, sizes)

        def new():
            aggs, c, v = bs.aggregate_verify_many_encoded(vk, msgs, blob, sizes)
            return aggs, v
        names = "aggregate_many_encoded + verify_many", "aggregate_verify_many_encoded"
    (a0, v0), (a1, v1) = old(), new()
    assert np.array_equal(a0, a1) and v0 == v1 == [(True, "")] * g, "the two flows disagree"

    # what the second call repeats: one challenge pass over all signers, one hash_ag per committee (on aggregate_many's pool)
    def repeated():
        with DeviceScope() as s:
            m = _Committees(bs, s, vk, msgs, sizes)           # (hash_ag="host": the host form)
            t0 = time.perf_counter()
            m.challenges()
            t1 = time.perf_counter()
            m.keys_host()
            m.alpha_hat()
            bs.ctx.synchronize()
            return t1 - t0, time.perf_counter() - t1
    t_old = t_new = t_ch = t_ag = 1e30
    for _ in range(E2E_ROUNDS):
        t0 = time.perf_counter()
        old()
        t_old = min(t_old, time.perf_counter() - t0)
        t0 = time.perf_counter()
        new()
        t_new = min(t_new, time.perf_counter() - t0)
        c, a = repeated()
        t_ch, t_ag = min(t_ch, c), min(t_ag, a)
    m_agg = n * rb + 4 * n + 4 * n * d + 12 * g * l * d                  # call 1: bytes, status, alpha_hat, partials + aggregates
    m_ver = 4 * n * d + 4 * n * d + 8 * n * d + 4 * g * l * d + 12 * g * d + 4 * g      # call 2: c_hat, alpha_hat, vkL + vkR, aggregates, targets, verdicts
    m_old = max(m_agg, m_ver)
    m_new = m_agg + 8 * n * d + 4 * n * d + 8 * g * d + 4 * g            # call 1's + vk, c_hat, the targets' partials, the verdicts
    print(f"secpar {secpar}  {shape}: host bytes -> {g} aggregate(s) and verdict(s), minimum of {E2E_ROUNDS}")
    print(f"  {names[0]:38s} {t_old * 1e3:9.2f} ms")
    print(f"  {names[1]:38s} {t_new * 1e3:9.2f} ms   {t_old / t_new:.3f}x   {'faster' if t_new < t_old else 'NOT FASTER'}")
    print(f"  saved {(t_old - t_new) * 1e3:8.2f} ms; expected: one challenge pass {t_ch * 1e3:.2f} ms + hash_ag per committee with its "
          f"upload and transform {t_ag * 1e3:.2f} ms = {(t_ch + t_ag) * 1e3:.2f} ms")
    print(f"  device memory live at the peak (from the shapes): the two calls {m_old / 1e6:.1f} MB (the larger), the one pass {m_new / 1e6:.1f} MB")


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
    steps = [("kernel", s, shape) for s in (256, 128) for shape in SHAPES] + [("e2e", s, shape) for s in (256, 128) for shape in E2E_SHAPES]
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        for what, secpar, shape in steps:                   # one process per step: each starts from a fresh context and a cold chip
            r = subprocess.run([sys.executable, os.path.abspath(__file__), what, str(secpar), shape], capture_output=True, text=True,
                               timeout=240)
            text = r.stdout if r.returncode == 0 else f"{what} {secpar} {shape}: exit {r.returncode}\n{r.stderr[-2000:]}\n"
            sys.stdout.write(text)
            sys.stdout.flush()
            fh.write(text)
            fh.flush()
            if r.returncode != 0:                           # nothing more on a device that a step left in an unknown state
                raise SystemExit(r.returncode)


if __name__ == "__main__":
    main(sys.argv[1:])
