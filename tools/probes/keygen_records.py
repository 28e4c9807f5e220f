"""Key generation straight to compact secret-key records (fz_keygen_records_async, BatchScheme.keygen_batch_encoded) against the pair
of calls that was the only way to records before, fz_keygen_core_bcast followed by fz_encode_records_async(rows = 2 l), and
beside fz_keygen_core_bcast alone -- on the same box and in the same process.

  kernel     the device-resident secret polynomials [N][2][d] of N seeds (64 sampled ones, tiled), cold operands: each call
             reads one of enough rotating copies of the polynomials that their sum exceeds the caches (512 MiB).  A = the new
             entry (coef_rows = 1), B = keygen_core_bcast + encode_records (the int32 key written by the one and read back by
             the other: the device work of keygen_batch_encoded before), C = keygen_core_bcast alone (reported, no
             requirement).  Event-timed over REPS calls, the minimum per call over ROUNDS rounds, A, B and C alternating within
             a round; `spread` = (max - min) / min of the per-round times of the same operation.  HBM bytes each moves per call
             by the byte model (the polynomials read, the verification keys written, the records written; B also writes the
             int32 key and reads it back, C writes it; the public challenge is left to the L2 in all), and their rate over that
             time as a fraction of 8 TB/s.  The step fails when A is slower than B by more than B's spread.
  e2e        seeds -> host records: keygen_batch_encoded(seeds) against keygen_batch(seeds, device=True) + encode("secret"),
             wall clock, the minimum over ROUNDS runs (the sampler is in both).  Device memory each holds at its peak: the sum
             of the arrays live at once, from the shapes.

Without arguments every step runs as a process of its own under its own time limit, the first failure ends the probe, and
the steps' output is collected in profiles/r19_keygen_records.txt (--out PATH: elsewhere).  Run from the repository root on
a GPU box: python tools/probes/keygen_records.py [--out PATH] | kernel SECPAR N | e2e SECPAR N."""
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
        print(f"  {name:38s} {best:9.2f} us per call  (spread {(max(t) - best) / best:5.1%})  {nbytes[name] / 1e6:8.1f} MB  "
              f"{nbytes[name] / best / 1e6:6.3f} TB/s = {nbytes[name] / best / 1e-6 / PEAK:5.1%} of 8 TB/s")


def kernel(secpar, n):
    import numpy as np
    from fusion_hip import DeviceArray, hostpipe
    from fusion_hip.scheme import _encoding
    bs = setup(secpar)
    ctx, l, d, p = bs.ctx, bs.l, bs.d, bs.params
    krows, _, kbound, wk, kb = _encoding(p, "secret")
    polys = hostpipe.sample_secret_polys(np.arange(5000, 5000 + BASE, dtype=np.uint64), p.modulus, d, p.beta_sk, p.omega_sk)
    coef_bytes, key_bytes, vk_bytes, rec_bytes = n * 2 * d * 4, n * 2 * l * d * 4, n * 2 * d * 4, n * kb
    copies = max(2, -(-COLD_BYTES // coef_bytes))
    dC = DeviceArray.from_numpy(ctx, np.ascontiguousarray(np.tile(polys[np.arange(n) % BASE], (copies, 1, 1, 1))))
    dA = bs._A_dev()
    ba, bb = (DeviceArray(ctx, (n, kb), np.uint8) for _ in range(2))
    va, vb, vc = (DeviceArray(ctx, (n, 2, d)) for _ in range(3))
    sa, sb = (DeviceArray(ctx, (n,)) for _ in range(2))
    rows, rows_c = (DeviceArray(ctx, (n, 2, l, d)) for _ in range(2))

    def new(k):
        ctx.keygen_records_async_dev(dA.ptr, dC.ptr + (k % copies) * coef_bytes, 1, n, l, kbound, ba.ptr, va.ptr, sa.ptr)

    def pair(k):
        ctx.keygen_core_bcast_dev(dA.ptr, dC.ptr + (k % copies) * coef_bytes, rows.ptr, vb.ptr, n, l)
        ctx.encode_records_async_dev(rows.ptr, n, krows, True, kbound, bb.ptr, sb.ptr)

    def alone(k):
        ctx.keygen_core_bcast_dev(dA.ptr, dC.ptr + (k % copies) * coef_bytes, rows_c.ptr, vc.ptr, n, l)

    new(0)
    pair(0)
    alone(0)
    assert not sa.numpy().any() and not sb.numpy().any(), "honest keys were refused"
    assert np.array_equal(ba.numpy(), bb.numpy()), "the fused pass and the pair differ in the records"
    assert np.array_equal(va.numpy(), vb.numpy()) and np.array_equal(va.numpy(), vc.numpy()), "the fused pass and the others differ in vk"
    names = ("A fz_keygen_records_async", "B keygen_core_bcast + encode_records", "C keygen_core_bcast alone")
    ops = dict(zip(names, (new, pair, alone)))
    seen = alternate(ctx, ops)
    print(f"secpar {secpar}  N {n} keys  (l = {l}, degree {d}, wk = {wk}, {coef_bytes} bytes of polynomials, {key_bytes} bytes of int32 key, "
          f"{rec_bytes} record bytes, {copies} rotating copies of the polynomials)")
    report(seen, dict(zip(names, (coef_bytes + vk_bytes + rec_bytes, coef_bytes + vk_bytes + 2 * key_bytes + rec_bytes,
                                  coef_bytes + vk_bytes + key_bytes))))
    a, b, c = (min(seen[k]) for k in names)
    sp = (max(seen[names[1]]) - b) / b
    ok = a <= b * (1 + sp)
    print(f"  B / A {b / a:.3f}   (A is {'not ' if ok else ''}slower than B by more than B's spread)   C / A {c / a:.3f}")
    return 0 if ok else 1


def e2e(secpar, n):
    import numpy as np
    from fusion_hip.scheme import _encoding
    bs = setup(secpar)
    l, d = bs.l, bs.d
    kb = _encoding(bs.params, "secret")[4]
    seeds = [5000 + k for k in range(n)]

    def old():
        dK, vk = bs.keygen_batch(seeds, device=True)
        try:
            data, codes = bs.encode("secret", dK)
        finally:
            dK.free()
        return data, vk, codes

    new = lambda: bs.keygen_batch_encoded(seeds)
    (ob, ov, oc), (nb, nv) = old(), new()
    assert np.array_equal(ob, nb) and np.array_equal(ov, nv) and not oc.any()
    t_old, t_new = 1e30, 1e30
    for _ in range(ROUNDS):
        t0 = time.perf_counter()
        old()
        t_old = min(t_old, time.perf_counter() - t0)
        t0 = time.perf_counter()
        new()
        t_new = min(t_new, time.perf_counter() - t0)
    coef, keyb, vkb = 8 * n * d, 8 * n * l * d, 8 * n * d
    m_old = coef + keyb + vkb + n * kb + 4 * n
    m_new = coef + vkb + n * kb + 4 * n
    print(f"secpar {secpar}  N {n}: seeds -> host records   keygen_batch(device=True) + encode ({keyb / 1e6:.1f} MB of int32 key on the device) "
          f"{t_old * 1e3:8.2f} ms   keygen_batch_encoded ({n * kb / 1e6:.1f} MB of records) {t_new * 1e3:8.2f} ms   {t_old / t_new:.3f}x")
    print(f"  device memory live at the peak (from the shapes): {m_old / 1e6:.1f} MB against {m_new / 1e6:.1f} MB = {m_old / m_new:.2f}x")
    return 0


def drive(out):
    """every step in a process of its own, under its own limit; the first failure ends the probe"""
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("# python tools/probes/keygen_records.py   (one process per step; see the file's docstring for what is measured)\n")
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
        return kernel(int(argv[1]), int(argv[2]))
    if argv and argv[0] == "e2e" and len(argv) == 3:
        return e2e(int(argv[1]), int(argv[2]))
    if not argv or (argv[0] == "--out" and len(argv) == 2):
        return drive(argv[1] if argv else os.path.join(ROOT, "profiles", "r19_keygen_records.txt"))
    print(__doc__)
    return 2


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
