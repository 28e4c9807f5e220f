"""Signing straight to the compact bytes (fz_sign_encoded_async, BatchScheme.sign_batch_encoded) against the pair of calls it
replaces, fz_sign_core followed by fz_encode_records_async, on the same box and in the same process.

  kernel     device-resident sk_hat and c_hat of N honest keys (64 generated ones, tiled), cold operands: each call reads one of
             enough rotating copies of sk_hat that their sum exceeds the caches (512 MiB).  A = the new entry, B = sign_core +
             encode_records (the int32 signatures written by the one and read back by the other).  Event-timed over REPS calls,
             the minimum per call over ROUNDS rounds, A and B alternating within a round; `spread` = (max - min) / min of the
             per-round times of the same operation.  HBM bytes each moves per call by the byte model (both key halves read, the
             records written; B also writes the rows and reads them back; c_hat, shared by a signer's l rows, is left to the
             L2 in both), and their rate over that time as a fraction of 8 TB/s.
  e2e        host sk_hat -> host bytes: sign_batch_encoded(sk_hat, vk, msgs) against sign_batch(device=True) + encode, wall
             clock, the minimum over ROUNDS runs (the challenge pass is in both).  Device memory each holds at its peak: the sum
             of the arrays live at once, from the shapes.

Without arguments every step runs as a process of its own under its own time limit, the first failure ends the probe, and
the steps' output is collected in profiles/r15_sign_encoded.txt (--out PATH: elsewhere).  Run from the repository root on
a GPU box: python tools/probes/sign_encoded.py [--out PATH] | kernel SECPAR N | e2e SECPAR N."""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "fusion-cryptography_amd"), ROOT):
    sys.path.insert(0, p)

REPS = 20
ROUNDS = 4
PEAK = 8.0e12
COLD_BYTES = 512 << 20
BASE = 64
STEPS = [(["kernel", str(s), str(n)], 240) for s in (256, 128) for n in (64, 1024, 8192)] + \
        [(["e2e", str(s), "1024"], 240) for s in (256, 128)]


def setup(secpar):
    import fusion.fusion as F
    from fusion_hip.scheme import BatchScheme
    return BatchScheme(F.fusion_setup(secpar, 2026))


def keys(bs, n):
    seeds = [5000 + k for k in range(n)]
    msgs = [f"probe-{k}" for k in range(n)]
    sk, vk = bs.keygen_batch(seeds)
    return sk, vk, msgs


def alternate(ctx, ops, copies):
    """{name: fn(copy index)} -> {name: per-call microseconds of every round}"""
    seen = {name: [] for name in ops}
    for _ in range(ROUNDS):
        for name, fn in ops.items():
            fn(0)
            ctx.synchronize()
            ctx.timer_start()
            for r in range(REPS):
                fn((r + 1) % copies)
            seen[name].append(ctx.timer_stop_ms() * 1e3 / REPS)
    return seen


def report(seen, nbytes):
    for name, t in seen.items():
        best = min(t)
        print(f"  {name:34s} {best:9.2f} us per call  (spread {(max(t) - best) / best:5.1%})  {nbytes[name] / 1e6:8.1f} MB  "
              f"{nbytes[name] / best / 1e6:6.3f} TB/s = {nbytes[name] / best / 1e-6 / PEAK:5.1%} of 8 TB/s")


def kernel(secpar, n):
    import numpy as np
    from fusion_hip import DeviceArray
    from fusion_hip.scheme import _encoding
    bs = setup(secpar)
    ctx, l, d = bs.ctx, bs.l, bs.d
    _, _, bound, w, rb = _encoding(bs.params, "signature")
    sk, vk, msgs = keys(bs, BASE)
    c_hat, _ = bs.challenges(vk, msgs)
    idx = np.arange(n) % BASE
    key_bytes = n * 2 * l * d * 4
    copies = max(2, -(-COLD_BYTES // key_bytes))
    tiled = np.ascontiguousarray(sk[idx])
    dK = [DeviceArray.from_numpy(ctx, tiled) for _ in range(copies)]
    del tiled
    dC = DeviceArray.from_numpy(ctx, c_hat[idx])
    ba, bb = DeviceArray(ctx, (n, rb), np.uint8), DeviceArray(ctx, (n, rb), np.uint8)
    sa, sb, rows = DeviceArray(ctx, (n,)), DeviceArray(ctx, (n,)), DeviceArray(ctx, (n * l, d))

    def new(k):
        ctx.sign_encoded_async_dev(dK[k].ptr, dC.ptr, n, l, bound, ba.ptr, sa.ptr)

    def pair(k):
        ctx.sign_core_dev(dK[k].ptr, dC.ptr, rows.ptr, n, l)
        ctx.encode_records_async_dev(rows.ptr, n, l, True, bound, bb.ptr, sb.ptr)

    new(0)
    pair(0)
    assert not sa.numpy().any() and not sb.numpy().any(), "honest signatures were refused"
    assert np.array_equal(ba.numpy(), bb.numpy()), "the fused pass and the pair differ"
    ops = {"A fz_sign_encoded_async": new, "B sign_core + encode_records": pair}
    seen = alternate(ctx, ops, copies)
    print(f"secpar {secpar}  N {n} signers  ({n * l} rows of degree {d}, w = {w}, {n * rb} encoded bytes, {copies} rotating copies of sk_hat)")
    report(seen, {"A fz_sign_encoded_async": key_bytes + n * rb, "B sign_core + encode_records": key_bytes + 8 * n * l * d + n * rb})
    a, b = (min(seen[k]) for k in ops)
    sp = (max(seen["B sign_core + encode_records"]) - b) / b
    print(f"  B / A {b / a:.3f}   (A is {'not ' if a <= b * (1 + sp) else ''}slower than B by more than B's spread)")


def e2e(secpar, n):
    import numpy as np
    from fusion_hip.scheme import _encoding
    bs = setup(secpar)
    l, d = bs.l, bs.d
    _, _, bound, w, rb = _encoding(bs.params, "signature")
    sk, vk, msgs = keys(bs, n)

    def old():
        dS = bs.sign_batch(sk, vk, msgs, device=True)
        try:
            return bs.encode("signature", dS)
        finally:
            dS.free()

    new = lambda: bs.sign_batch_encoded(sk, vk, msgs)
    (ob, oc), (nb, nc) = old(), new()
    assert np.array_equal(ob, nb) and not oc.any() and not nc.any()
    t_old, t_new = 1e30, 1e30
    for _ in range(ROUNDS):
        t0 = time.perf_counter()
        old()
        t_old = min(t_old, time.perf_counter() - t0)
        t0 = time.perf_counter()
        new()
        t_new = min(t_new, time.perf_counter() - t0)
    keyb, chal, sig = 8 * n * l * d, 4 * n * d, 4 * n * l * d
    m_old = max(keyb + chal + sig, sig + n * rb + 4 * n)         # while signing; while encoding
    m_new = keyb + chal + n * rb + 4 * n
    print(f"secpar {secpar}  N {n}: host sk_hat -> host bytes   sign_batch(device=True) + encode {t_old * 1e3:8.2f} ms   "
          f"sign_batch_encoded {t_new * 1e3:8.2f} ms   {t_old / t_new:.3f}x")
    print(f"  device memory live at the peak (from the shapes): {m_old / 1e6:.1f} MB against {m_new / 1e6:.1f} MB = {m_old / m_new:.2f}x")


def drive(out):
    """every step in a process of its own, under its own limit; the first failure ends the probe"""
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("# python tools/probes/sign_encoded.py   (one process per step; see the file's docstring for what is measured)\n")
        for args, limit in STEPS:
            fh.flush()
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, cwd=ROOT, timeout=limit, stdout=subprocess.PIPE,
                                   stderr=subprocess.STDOUT, text=True)
            except subprocess.TimeoutExpired:
                fh.write(f"step {' '.join(args)}: no result within {limit} s; the probe ends here\n")
                return 124
            lines = [ln for ln in r.stdout.splitlines() if "amdgpu.ids" not in ln]
            fh.write("\n".join(lines) + "\n")
            print("\n".join(lines), flush=True)
            if r.returncode != 0:
                fh.write(f"step {' '.join(args)}: exit status {r.returncode}; the probe ends here\n")
                return r.returncode
    return 0


def main(argv):
    if argv and argv[0] == "kernel" and len(argv) == 3:
        kernel(int(argv[1]), int(argv[2]))
    elif argv and argv[0] == "e2e" and len(argv) == 3:
        e2e(int(argv[1]), int(argv[2]))
    elif not argv or (argv[0] == "--out" and len(argv) == 2):
        return drive(argv[1] if argv else os.path.join(ROOT, "profiles", "r15_sign_encoded.txt"))
    else:
        print(__doc__)
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
