"""Per-signature verification (BatchScheme.verify_signatures): the kernel and the call end to end.

  kernel  verify_fused with the target formed from the key (fz_verify_signatures_async) beside verify_fused with a target
          array (fz_verify_with_target_batch_async) at G = N, secpar 128 and 256, N = 1024 and 8192, in the same process,
          the two forms alternating over ROUNDS rounds: event-timed over REPS launches each, the minimum over rounds.  Under
          `rocprofv3 --kernel-trace --stats` the two forms are the same kernel (one instantiation serves both), so each
          timed block is fenced by a diag_empty_launch and listed ("block k: ..."); `split <kernel_trace.csv>` gives the
          profiler's durations per block.
  e2e     verify_signatures at N = 64, 1024, 4096, 16384 with device-resident keys and signatures and from host arrays, and
          the workaround it replaces (aggregate_many + verify_many with sizes = [1] * N) at N = 1024.
Run from the repository root on a GPU box: python tools/probes/signature_screening.py [kernel|e2e|all | split TRACE_CSV]."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "fusion-cryptography_amd"), ROOT):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import fusion.fusion as F  # noqa: E402
from fusion_hip import DeviceArray  # noqa: E402
from fusion_hip.scheme import BatchScheme, signature_bound  # noqa: E402

REPS = 50
ROUNDS = 3
_BLOCKS = []        # kernel mode: the timed blocks in launch order (block k follows the k-th diag_empty_kernel of a trace)


def signers(bs, n, seed=1):
    seeds = [seed + 3 * i for i in range(n)]
    msgs = [f"probe message {i:07d}" for i in range(n)]
    dsk, _, dvk = bs.keygen_batch(seeds, device=True, keep_vk=True)
    dsig = bs.sign_batch(dsk, dvk, msgs, device=True)
    dsk.free()
    return dvk, msgs, dsig


def kernel(secpar):
    params = F.fusion_setup(secpar, 2026)
    bs = BatchScheme(params)
    ctx, l, d = bs.ctx, bs.l, bs.d
    beta = signature_bound(params)
    for n in (1024, 8192):
        dvk, msgs, dsig = signers(bs, n)
        dC, _ = bs.challenges_dev(dvk, msgs, want_prehash=False)
        dT = DeviceArray.from_numpy(ctx, np.zeros((n, d), dtype=np.int32))      # any target: the time does not depend on it
        dV = DeviceArray(ctx, (n,))
        dA = bs._A_dev()
        forms = {
            "target array (verify_with_target_batch_async)":
                lambda: ctx.verify_with_target_batch_async_dev(dA.ptr, dsig.ptr, dT.ptr, n, l, params.beta_vf, params.omega_vf, dV.ptr),
            "target from the key (verify_signatures_async)":
                lambda: ctx.verify_signatures_async_dev(dA.ptr, dsig.ptr, dvk.ptr, dC.ptr, n, l, beta, params.omega_vf, dV.ptr),
        }
        res = {}
        for rnd in range(ROUNDS):                   # the forms alternate: clock and placement drift falls on both alike
            for name, fn in forms.items():
                ctx.diag_empty_launch()             # the fence between blocks in a kernel trace
                _BLOCKS.append(f"secpar {secpar} N {n} {name} (round {rnd})")
                for _ in range(5):
                    fn()
                ctx.synchronize()
                ctx.timer_start()
                for _ in range(REPS):
                    fn()
                us = ctx.timer_stop_ms() * 1e3 / REPS
                res[name] = min(res.get(name, us), us)
                ctx.synchronize()
        assert (dV.numpy() == 0).all()
        byts = n * (l + 3) * 4 * d
        base = res["target array (verify_with_target_batch_async)"]
        for name, us in res.items():
            print(f"secpar {secpar}  N {n:5d}  {name:<48s} {us:8.1f} us/launch  {us * 1e3 / n:7.1f} ns/signer  "
                  f"{byts / us / 1e6:5.2f} TB/s of (l+3)*4*d per signer  x{us / base:.3f}", flush=True)
        for b in (dvk, dsig, dC, dT, dV):
            b.free()
    bs.close()


def stat(fn, reps=10):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts) * 1e3, statistics.median(ts) * 1e3


def e2e(secpar):
    params = F.fusion_setup(secpar, 2026)
    bs = BatchScheme(params)
    for n in (64, 1024, 4096, 16384):
        dvk, msgs, dsig = signers(bs, n)
        vk, sig = dvk.numpy(), dsig.numpy()
        assert (bs.verify_signatures(dvk, msgs, dsig) == 0).all()
        for name, args in (("device-resident", (dvk, msgs, dsig)), ("host arrays", (vk, msgs, sig))):
            lo, med = stat(lambda: bs.verify_signatures(*args))
            print(f"secpar {secpar}  N {n:5d}  verify_signatures, {name:<16s} min {lo:8.2f} ms  median {med:8.2f} ms  "
                  f"{n / lo / 1e3:6.2f} M signatures/s  (host form moves {sig.nbytes / 1e6:.0f} MB of signatures)", flush=True)
        if n == 1024:
            def workaround():
                aggs = bs.aggregate_many(dvk, msgs, dsig, [1] * n)
                return bs.verify_many(dvk, msgs, aggs, [1] * n)
            lo, med = stat(workaround, reps=3)
            print(f"secpar {secpar}  N {n:5d}  aggregate_many + verify_many, sizes=[1]*N     min {lo:8.2f} ms  median {med:8.2f} ms",
                  flush=True)
        dvk.free()
        dsig.free()
    bs.close()


def split(trace_csv):
    """a rocprofv3 kernel_trace.csv of `kernel` mode -> per block (k-th fence onwards): verify_fused dispatches and their
    median / min duration.  Block k is the k-th `block` line kernel mode printed."""
    import csv
    rows = sorted(csv.DictReader(open(trace_csv)), key=lambda r: int(r["Start_Timestamp"]))
    blocks = []
    for r in rows:
        if "diag_empty_kernel" in r["Kernel_Name"]:
            blocks.append([])
        elif "verify_fused" in r["Kernel_Name"] and blocks:
            blocks[-1].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)
    for k, v in enumerate(blocks):
        if v:
            print(f"block {k:2d}: {len(v):3d} verify_fused dispatches, median {statistics.median(v):8.2f} us, min {min(v):8.2f} us")


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    if what == "split":
        split(sys.argv[2])
        sys.exit(0)
    for secpar in (128, 256):
        if what in ("kernel", "all"):
            kernel(secpar)
    for k, label in enumerate(_BLOCKS):
        print(f"block {k:2d}: {label}")
    for secpar in (128, 256):
        if what in ("e2e", "all"):
            e2e(secpar)
