"""Verification keys straight from compact secret-key records (fz_vk_records_async, BatchScheme.sign_batch_secret) against the pair
of calls that was the only way from a record to its key before, fz_decode_records_async(rows = 2 l, coef = 1, key_bound) followed
by fz_matvec over the 2 N halves -- on the same box and in the same process.

  kernel     device-resident honest "secret" records of N keys (64 generated ones, tiled), cold operands: each call reads one of
             enough rotating copies of the records that their sum exceeds the caches (512 MiB).  A = the new entry, B =
             decode_records + matvec (the int32 key written by the one and read back by the other).  Event-timed over REPS whole
             calls, the minimum per call over ROUNDS rounds, A and B alternating within a round; `spread` = (max - min) / min of
             the per-round times of the same operation.  HBM bytes each moves per call by the byte model (the records read, the
             verification keys written; B also writes the int32 key and reads it back; the public challenge is left to the L2 in
             both), and their rate over that time as a fraction of 8 TB/s.  At N = 1024 and 8192 the step's exit status is 3
             when A is slower than B by more than B's spread; N = 64 is launch latency on both sides and is reported only.
  e2e        host records + messages -> host signature records and keys: sign_batch_secret against decode("secret",
             device=True) + matvec + sign_batch_records, wall clock, the minimum over ROUNDS runs.  Device memory each holds at its
             peak: the sum of the arrays live at once, from the shapes.

Without arguments every step runs as a process of its own under its own time limit and the steps' output is collected in
profiles/r22_vk_records.txt (--out PATH: elsewhere).  A step that misses the requirement (exit status 3) is recorded and the
probe goes on; any other failure ends the probe.  Run from the repository root on a GPU box:
python tools/probes/vk_records.py [--out PATH] | kernel SECPAR N | e2e SECPAR N."""
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
REQUIRED = (1024, 8192)
MISSED = 3
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
    from fusion_hip import DeviceArray
    from fusion_hip.scheme import _encoding
    bs = setup(secpar)
    ctx, l, d = bs.ctx, bs.l, bs.d
    krows, _, kbound, wk, kb = _encoding(bs.params, "secret")
    base, base_vk = bs.keygen_batch_encoded([5000 + k for k in range(BASE)])
    key_bytes, vk_bytes, rec_bytes = n * 2 * l * d * 4, n * 2 * d * 4, n * kb
    copies = max(2, -(-COLD_BYTES // rec_bytes))
    dK = DeviceArray.from_numpy(ctx, np.ascontiguousarray(np.tile(base[np.arange(n) % BASE], (copies, 1))))
    dA = bs._A_dev()
    va, vb = (DeviceArray(ctx, (n, 2, d)) for _ in range(2))
    sa, sb = (DeviceArray(ctx, (n,)) for _ in range(2))
    rows = DeviceArray(ctx, (n, 2, l, d))

    def new(k):
        ctx.vk_records_async_dev(dA.ptr, dK.ptr + (k % copies) * rec_bytes, kbound, n, l, va.ptr, sa.ptr)

    def pair(k):
        ctx.decode_records_async_dev(dK.ptr + (k % copies) * rec_bytes, n, krows, True, kbound, rows.ptr, sb.ptr)
        ctx.matvec_dev(dA.ptr, rows.ptr, vb.ptr, 2 * n, l)

    new(0)
    pair(0)
    assert not sa.numpy().any() and not sb.numpy().any(), "honest records were refused"
    assert np.array_equal(va.numpy(), vb.numpy()), "the fused pass and the pair differ in vk"
    assert np.array_equal(va.numpy(), base_vk[np.arange(n) % BASE]), "the derived keys are not the generated ones"
    names = ("A fz_vk_records_async", "B decode_records + matvec")
    seen = alternate(ctx, dict(zip(names, (new, pair))))
    print(f"secpar {secpar}  N {n} keys  (l = {l}, degree {d}, wk = {wk}, {rec_bytes} record bytes, {key_bytes} bytes of int32 key, "
          f"{vk_bytes} bytes of vk, {copies} rotating copies of the records)")
    report(seen, dict(zip(names, (rec_bytes + vk_bytes, rec_bytes + 2 * key_bytes + vk_bytes))))
    a, b = (min(seen[k]) for k in names)
    sp = (max(seen[names[1]]) - b) / b
    ok = a <= b * (1 + sp)
    need = "required" if n in REQUIRED else "reported, not required: launch latency on both sides"
    print(f"  B / A {b / a:.3f}   (A is {'not ' if ok else ''}slower than B by more than B's spread; {need})")
    return 0 if ok or n not in REQUIRED else MISSED


def e2e(secpar, n):
    import numpy as np
    from fusion_hip import DeviceArray
    from fusion_hip.scheme import _encoding
    bs = setup(secpar)
    ctx, l, d = bs.ctx, bs.l, bs.d
    kb, rb = _encoding(bs.params, "secret")[4], _encoding(bs.params, "signature")[4]
    base, _ = bs.keygen_batch_encoded([5000 + k for k in range(BASE)])
    recs = np.ascontiguousarray(base[np.arange(n) % BASE])
    msgs = [f"vk-records-probe-{k}" for k in range(n)]

    def old():
        dR, codes = bs.decode("secret", recs, device=True)
        dV = DeviceArray(ctx, (n, 2, d))
        try:
            ctx.matvec_dev(bs._A_dev().ptr, dR.ptr, dV.ptr, 2 * n, l)
            vk = dV.numpy()
        finally:
            dR.free()
            dV.free()
        data, scodes = bs.sign_batch_records(recs, vk, msgs)
        return data, scodes | codes, vk

    new = lambda: bs.sign_batch_secret(recs, msgs)
    (ob, oc, ov), (nb, nc, nv) = old(), new()
    assert np.array_equal(ob, nb) and np.array_equal(ov, nv) and not oc.any() and not nc.any()
    t_old, t_new = 1e30, 1e30
    for _ in range(ROUNDS):
        t0 = time.perf_counter()
        old()
        t_old = min(t_old, time.perf_counter() - t0)
        t0 = time.perf_counter()
        new()
        t_new = min(t_new, time.perf_counter() - t0)
    keyb, vkb, chal = 8 * n * l * d, 8 * n * d, 4 * n * d
    m_old = max(n * kb + keyb + vkb + 4 * n, n * kb + vkb + chal + n * rb + 4 * n)      # the decode + matvec, or the signing after it
    m_new = n * kb + vkb + chal + n * rb + 8 * n
    print(f"secpar {secpar}  N {n}: host records + messages -> host signature records and keys   decode(device=True) + matvec + "
          f"sign_batch_records ({keyb / 1e6:.1f} MB of int32 key on the device) {t_old * 1e3:8.2f} ms   sign_batch_secret "
          f"({n * kb / 1e6:.1f} MB of records) {t_new * 1e3:8.2f} ms   {t_old / t_new:.3f}x")
    print(f"  device memory live at the peak (from the shapes): {m_old / 1e6:.1f} MB against {m_new / 1e6:.1f} MB = {m_old / m_new:.2f}x")
    return 0


def drive(out):
    """every step in a process of its own, under its own limit; a missed requirement is recorded, any other failure ends the probe"""
    os.makedirs(os.path.dirname(out), exist_ok=True)
    missed = 0
    with open(out, "w") as fh:
        fh.write("# python tools/probes/vk_records.py   (one process per step; see the file's docstring for what is measured)\n")
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
            if r.returncode == MISSED:
                missed += 1
                fh.write(f"step {' '.join(args)}: the requirement is missed\n")
            elif r.returncode != 0:
                fh.write(f"step {' '.join(args)}: exit status {r.returncode}; the probe ends here\n")
                return r.returncode
    return MISSED if missed else 0


def main(argv):
    if argv and argv[0] == "kernel" and len(argv) == 3:
        return kernel(int(argv[1]), int(argv[2]))
    if argv and argv[0] == "e2e" and len(argv) == 3:
        return e2e(int(argv[1]), int(argv[2]))
    if not argv or (argv[0] == "--out" and len(argv) == 2):
        return drive(argv[1] if argv else os.path.join(ROOT, "profiles", "r22_vk_records.txt"))
    print(__doc__)
    return 2


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
