"""Signing straight from compact secret-key records (fz_sign_records_async, BatchScheme.sign_batch_records) against the pair of
calls that was the only way to sign from records before, fz_decode_records_async(rows = 2 l) followed by fz_sign_encoded_async,
and beside fz_sign_encoded_async on keys already resident as int32 -- on the same box and in the same process.

  kernel     device-resident "secret" records, sk_hat and c_hat of N honest keys (64 generated ones, tiled), cold operands: each
             call reads one of enough rotating copies of its key input that their sum exceeds the caches (512 MiB).  A = the new
             entry, B = decode_records + sign_encoded (the int32 key written by the one and read back by the other), C =
             sign_encoded on resident int32 keys (reported, no requirement).  Event-timed over REPS calls, the minimum per call
             over ROUNDS rounds, A, B and C alternating within a round; `spread` = (max - min) / min of the per-round times of
             the same operation.  HBM bytes each moves per call by the byte model (the key read in its form, the records
             written; B also writes the int32 key and reads it back; c_hat, shared by a signer's l rows, is left to the L2 in
             all), and their rate over that time as a fraction of 8 TB/s.
  e2e        host records -> host bytes: sign_batch_records(records, vk, msgs) against sign_batch_encoded(sk_hat, vk, msgs)
             from host int32 keys, wall clock, the minimum over ROUNDS runs (the challenge pass is in both).  Device memory
             each holds at its peak: the sum of the arrays live at once, from the shapes.

Without arguments every step runs as a process of its own under its own time limit, the first failure ends the probe, and
the steps' output is collected in profiles/r17_sign_records.txt (--out PATH: elsewhere).  Run from the repository root on
a GPU box: python tools/probes/sign_records.py [--out PATH] | kernel SECPAR N | e2e SECPAR N."""
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
STEPS = [(["kernel", str(s), str(n)], 120 if n < 8192 else 300) for s in (256, 128) for n in (64, 1024, 8192)] + \
        [(["e2e", str(s), "1024"], 120) for s in (256, 128)]


def setup(secpar):
    import fusion.fusion as F
    from fusion_hip.scheme import BatchScheme
    return BatchScheme(F.fusion_setup(secpar, 2026))


def keys(bs, n):
    seeds = [5000 + k for k in range(n)]
    msgs = [f"probe-{k}" for k in range(n)]
    sk, vk = bs.keygen_batch(seeds)
    return sk, vk, msgs


def alternate(ctx, ops):
    """{name: fn(call index; it picks its own rotating copy)} -> {name: per-call microseconds of every round}"""
    seen = {name: [] for name in ops}
    for _ in range(ROUNDS):
        for name, fn in ops.items():
            fn(0)
            ctx.synchronize()
            ctx.timer_start()
            for r in range(REPS):
                fn(r + 1)
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
    krows, _, kbound, wk, kb = _encoding(bs.params, "secret")
    sk, vk, msgs = keys(bs, BASE)
    recs, codes = bs.encode("secret", sk)
    assert not codes.any(), "honest keys were refused"
    c_hat, _ = bs.challenges(vk, msgs)
    idx = np.arange(n) % BASE
    rec_bytes, key_bytes = n * kb, n * 2 * l * d * 4
    rcopies, kcopies = max(2, -(-COLD_BYTES // rec_bytes)), max(2, -(-COLD_BYTES // key_bytes))
    tiled = np.ascontiguousarray(recs[idx])
    dR = [DeviceArray.from_numpy(ctx, tiled) for _ in range(rcopies)]
    tiled = np.ascontiguousarray(sk[idx])
    dK = [DeviceArray.from_numpy(ctx, tiled) for _ in range(kcopies)]
    del tiled
    dC = DeviceArray.from_numpy(ctx, c_hat[idx])
    ba, bb, bc = (DeviceArray(ctx, (n, rb), np.uint8) for _ in range(3))
    sa, sb, sc, sd = (DeviceArray(ctx, (n,)) for _ in range(4))
    rows = DeviceArray(ctx, (n, 2, l, d))

    def new(k):
        ctx.sign_records_async_dev(dR[k % rcopies].ptr, kbound, dC.ptr, n, l, bound, ba.ptr, sa.ptr)

    def pair(k):
        ctx.decode_records_async_dev(dR[k % rcopies].ptr, n, krows, True, kbound, rows.ptr, sd.ptr)
        ctx.sign_encoded_async_dev(rows.ptr, dC.ptr, n, l, bound, bb.ptr, sb.ptr)

    def resident(k):
        ctx.sign_encoded_async_dev(dK[k % kcopies].ptr, dC.ptr, n, l, bound, bc.ptr, sc.ptr)

    new(0)
    pair(0)
    resident(0)
    assert not sa.numpy().any() and not sb.numpy().any() and not sc.numpy().any() and not sd.numpy().any(), "honest keys were refused"
    assert np.array_equal(ba.numpy(), bb.numpy()) and np.array_equal(ba.numpy(), bc.numpy()), "the fused pass and the others differ"
    names = ("A fz_sign_records_async", "B decode_records + sign_encoded", "C sign_encoded, resident int32")
    ops = dict(zip(names, (new, pair, resident)))
    seen = alternate(ctx, ops)
    print(f"secpar {secpar}  N {n} signers  ({n * l} rows of degree {d}, wk = {wk}, w = {w}, {rec_bytes} key bytes, {n * rb} encoded bytes, "
          f"{rcopies} / {kcopies} rotating copies of the records / of sk_hat)")
    report(seen, dict(zip(names, (rec_bytes + n * rb, rec_bytes + 2 * key_bytes + n * rb, key_bytes + n * rb))))
    a, b, c = (min(seen[k]) for k in names)
    sp = (max(seen[names[1]]) - b) / b
    print(f"  B / A {b / a:.3f}   (A is {'not ' if a <= b * (1 + sp) else ''}slower than B by more than B's spread)   C / A {c / a:.3f}"
          f"   ({'resident int32 keys remain the faster input' if c < a else 'records are the faster input even against resident int32 keys'})")


def e2e(secpar, n):
    import numpy as np
    from fusion_hip.scheme import _encoding
    bs = setup(secpar)
    l, d = bs.l, bs.d
    _, _, bound, w, rb = _encoding(bs.params, "signature")
    kb = _encoding(bs.params, "secret")[4]
    sk, vk, msgs = keys(bs, n)
    recs, codes = bs.encode("secret", sk)
    assert not codes.any()
    old = lambda: bs.sign_batch_encoded(sk, vk, msgs)
    new = lambda: bs.sign_batch_records(recs, vk, msgs)
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
    keyb, chal = 8 * n * l * d, 4 * n * d
    m_old = keyb + chal + n * rb + 4 * n
    m_new = n * kb + chal + n * rb + 4 * n
    print(f"secpar {secpar}  N {n}: host keys -> host bytes   sign_batch_encoded (int32 keys, {keyb / 1e6:.1f} MB up) {t_old * 1e3:8.2f} ms   "
          f"sign_batch_records (records, {n * kb / 1e6:.1f} MB up) {t_new * 1e3:8.2f} ms   {t_old / t_new:.3f}x")
    print(f"  device memory live at the peak (from the shapes): {m_old / 1e6:.1f} MB against {m_new / 1e6:.1f} MB = {m_old / m_new:.2f}x")


def drive(out):
    """every step in a process of its own, under its own limit; the first failure ends the probe"""
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("# python tools/probes/sign_records.py   (one process per step; see the file's docstring for what is measured)\n")
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
        return drive(argv[1] if argv else os.path.join(ROOT, "profiles", "r17_sign_records.txt"))
    else:
        print(__doc__)
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
