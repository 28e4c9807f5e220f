"""Verification straight from the compact bytes (fz_verify_encoded_async, BatchScheme.verify_signatures_encoded / verify_encoded)
against the pair of calls it replaces, fz_decode_records_async followed by fz_verify_signatures_async (signatures) or
fz_verify_with_target_batch_async (one aggregate), on the same box and in the same process.

  kernel     device-resident bytes of N honest signatures (64 signed ones, tiled), cold operands: each call reads one of enough
             rotating copies of the encoded batch that their sum exceeds the caches (512 MiB).  A = the new entry in its keyed
             form, B = decode + verify_signatures.  Event-timed over REPS calls, the minimum per call over ROUNDS rounds, A and B
             alternating within a round; `spread` = (max - min) / min of the per-round times of the same operation.  HBM bytes
             each moves per call by the byte model (records read; B also writes the rows and reads them back), and their rate
             over that time as a fraction of 8 TB/s.
  aggregate  one "aggregate" record against its target array, A = the new entry (several workgroups per record, the clear of
             the shared area and the finish kernel included), B = decode + verify_with_target_batch.  The copies of ONE record
             that fit a probe stay inside the Infinity Cache: warm, for both.
  e2e        host bytes -> verdicts on the host: verify_signatures_encoded(vk, msgs, bytes) against decode(device=True) +
             verify_signatures, wall clock, the minimum over ROUNDS runs (the challenge pass is in both).  Device memory each
             holds at its peak: the sum of the arrays live at once, from the shapes.

Without arguments every step runs as a process of its own under its own time limit, the first failure ends the probe, and
the steps' output is collected in profiles/r11_verify_encoded.txt (--out PATH: elsewhere).  Run from the repository root on
a GPU box: python tools/probes/verify_encoded.py [--out PATH] | kernel SECPAR N | aggregate SECPAR | e2e SECPAR N."""
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
        [(["aggregate", str(s)], 120) for s in (256, 128)] + [(["e2e", str(s), "1024"], 240) for s in (256, 128)]


def setup(secpar):
    import fusion.fusion as F
    from fusion_hip.scheme import BatchScheme
    return BatchScheme(F.fusion_setup(secpar, 2026))


def signed(bs, n):
    seeds = [5000 + k for k in range(n)]
    msgs = [f"probe-{k}" for k in range(n)]
    sk, vk = bs.keygen_batch(seeds)
    return vk, msgs, bs.sign_batch(sk, vk, msgs)


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
    vk, msgs, sig = signed(bs, BASE)
    c_hat, _ = bs.challenges(vk, msgs)
    data, codes = bs.encode("signature", sig)
    assert not codes.any()
    idx = np.arange(n) % BASE
    copies = max(2, -(-COLD_BYTES // (n * rb)))
    enc = [DeviceArray.from_numpy(ctx, data[idx]) for _ in range(copies)]
    dK, dC, dA = DeviceArray.from_numpy(ctx, vk[idx]), DeviceArray.from_numpy(ctx, c_hat[idx]), bs._A_dev()
    st, rows = DeviceArray(ctx, (n,)), DeviceArray(ctx, (n * l, d))
    va, vb = DeviceArray(ctx, (n,)), DeviceArray(ctx, (n,))

    def new(k):
        ctx.verify_encoded_async_dev(dA.ptr, enc[k].ptr, n, l, bound, 0, dK.ptr, dC.ptr, va.ptr)

    def pair(k):
        ctx.decode_records_async_dev(enc[k].ptr, n, l, True, bound, rows.ptr, st.ptr)
        ctx.verify_signatures_async_dev(dA.ptr, rows.ptr, dK.ptr, dC.ptr, n, l, bound, d, vb.ptr)

    new(0)
    pair(0)
    assert not va.numpy().any() and not vb.numpy().any(), "honest signatures were rejected"
    ops = {"A fz_verify_encoded_async (keyed)": new, "B decode + verify_signatures": pair}
    seen = alternate(ctx, ops, copies)
    keys = 12 * n * d
    print(f"secpar {secpar}  N {n} signatures  ({n * l} rows of degree {d}, w = {w}, {n * rb} encoded bytes, {copies} rotating copies)")
    report(seen, {"A fz_verify_encoded_async (keyed)": n * rb + keys, "B decode + verify_signatures": n * rb + 8 * n * l * d + keys})
    a, b = (min(seen[k]) for k in ops)
    print(f"  B / A {b / a:.3f}")


def aggregate(secpar):
    import numpy as np
    from fusion_hip import DeviceArray
    from fusion_hip.scheme import _encoding
    bs = setup(secpar)
    ctx, l, d, q = bs.ctx, bs.l, bs.d, bs.q
    _, _, bound, w, rb = _encoding(bs.params, "aggregate")
    vk, msgs, sig = signed(bs, 4)
    agg = bs.aggregate(vk, msgs, sig)
    rec, codes = bs.encode("aggregate", agg)
    assert not codes.any() and bs.verify_encoded(vk, msgs, rec) == (True, "") == bs.verify(vk, msgs, agg)
    # the target the scheme call forms, here on the host: A (.) aggregate itself (the record is valid)
    A = bs.A.reshape(l, d).astype(object)
    target = ((A * agg.astype(object)).sum(axis=0) % q).astype(np.int64)
    target = ((target + q // 2) % q - q // 2).astype(np.int32)
    copies = 256
    enc = [DeviceArray.from_numpy(ctx, rec) for _ in range(copies)]
    dT, dA = DeviceArray.from_numpy(ctx, target), bs._A_dev()
    st, rows, va, vb = DeviceArray(ctx, (1,)), DeviceArray(ctx, (l, d)), DeviceArray(ctx, (1,)), DeviceArray(ctx, (1,))
    beta, omega = int(bs.params.beta_vf), int(bs.params.omega_vf)

    def new(k):
        ctx.verify_encoded_async_dev(dA.ptr, enc[k].ptr, 1, l, bound, dT.ptr, 0, 0, va.ptr)

    def pair(k):
        ctx.decode_records_async_dev(enc[k].ptr, 1, l, True, bound, rows.ptr, st.ptr)
        ctx.verify_with_target_batch_async_dev(dA.ptr, rows.ptr, dT.ptr, 1, l, beta, omega, vb.ptr)

    new(0)
    pair(0)
    assert va.numpy().tolist() == [0] == vb.numpy().tolist(), "the valid aggregate was rejected"
    ops = {"A fz_verify_encoded_async (target)": new, "B decode + verify_with_target": pair}
    seen = alternate(ctx, ops, copies)
    print(f"secpar {secpar}  one aggregate record  ({l} rows of degree {d}, w = {w}, {rb} encoded bytes, {copies} rotating copies: warm)")
    report(seen, {"A fz_verify_encoded_async (target)": rb + 8 * d, "B decode + verify_with_target": rb + 8 * l * d + 4 * d})
    a, b = (min(seen[k]) for k in ops)
    print(f"  B / A {b / a:.3f}")


def e2e(secpar, n):
    import numpy as np
    from fusion_hip.scheme import _encoding
    bs = setup(secpar)
    l, d = bs.l, bs.d
    _, _, bound, w, rb = _encoding(bs.params, "signature")
    vk, msgs, sig = signed(bs, n)
    data, codes = bs.encode("signature", sig)
    assert not codes.any()
    blob = data.tobytes()

    def old():
        dS, _ = bs.decode("signature", blob, device=True)
        try:
            return bs.verify_signatures(vk, msgs, dS)
        finally:
            dS.free()

    new = lambda: bs.verify_signatures_encoded(vk, msgs, blob)
    assert np.array_equal(old(), new()) and not new().any()
    t_old, t_new = 1e30, 1e30
    for _ in range(ROUNDS):
        t0 = time.perf_counter()
        old()
        t_old = min(t_old, time.perf_counter() - t0)
        t0 = time.perf_counter()
        new()
        t_new = min(t_new, time.perf_counter() - t0)
    common = 4 * n + 12 * n * d + 4 * l * d                 # verdicts, keys and challenges, A
    m_old, m_new = n * rb + 4 * n * l * d + 4 * n + common, n * rb + common      # ... + the int32 rows and decode's codes
    print(f"secpar {secpar}  N {n}: host bytes -> verdicts   decode(device=True) + verify_signatures {t_old * 1e3:8.2f} ms   "
          f"verify_signatures_encoded {t_new * 1e3:8.2f} ms   {t_old / t_new:.3f}x")
    print(f"  device memory live at the peak (from the shapes): {m_old / 1e6:.1f} MB against {m_new / 1e6:.1f} MB = {m_old / m_new:.2f}x")


def drive(out):
    """every step in a process of its own, under its own limit; the first failure ends the probe"""
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("# python tools/probes/verify_encoded.py   (one process per step; see the file's docstring for what is measured)\n")
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
    elif argv and argv[0] == "aggregate" and len(argv) == 2:
        aggregate(int(argv[1]))
    elif argv and argv[0] == "e2e" and len(argv) == 3:
        e2e(int(argv[1]), int(argv[2]))
    elif not argv or (argv[0] == "--out" and len(argv) == 2):
        return drive(argv[1] if argv else os.path.join(ROOT, "profiles", "r11_verify_encoded.txt"))
    else:
        print(__doc__)
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
