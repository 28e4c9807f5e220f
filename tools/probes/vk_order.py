"""The key sort of hash_ag for many committees: on the device (BatchScheme(key_sort="device"): fz_hash_ag_ragged_sorted_dev, the
digests kept on the device) against on the host (the "device" form of hash_ag as it was: fz_sort_by_vk_string_ragged over a host
copy of the keys, the digests downloaded and uploaded again), on the same box and in the same process.

The cells and the method are tools/probes/hash_ag_many.py's: G committees of n signers, both parameter sets, medians of REPS
repetitions on fresh inputs, the forms alternating; spread = (max - min) / median.
  step   the hash_ag step alone, from what the challenge pass leaves to alpha_hat on the device, wall clock to a synchronise:
           host sort      fusion_hip.scheme._Committees.alpha_hat under key_sort="host": the ragged sort of host-resident keys, the upload
                          of the digests, the entry
           + key download the same when the keys live on the device: the download of [N][2][d] in front of it
           device sort    ... under key_sort="device": the entry alone (keys and digests are where the challenge pass left them)
           entry          fz_hash_ag_ragged_sorted_dev by device events (memset, sort kernel, hash kernel, transform)
         on synthetic centred rows, a fresh window of a larger pool for every repetition.
  call   aggregate_verify_many_encoded on real keys and records under hash_ag="device", wall clock: key_sort="host" and "device",
         each with the keys handed over as a host array and as a DeviceArray; cells of up to CALL_MAX signers.
Run from the repository root on a GPU box: python tools/probes/vk_order.py [all | step SECPAR | call SECPAR]; `all` runs every part
in a process of its own and writes profiles/r26_vk_order.txt."""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "fusion-cryptography_amd"), ROOT):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402

REPS = 5
THREADS = 16
GS, NS = (64, 256, 1024, 4096), (4, 16, 64)
CALL_MAX = 16384
OUT = os.path.join(ROOT, "profiles", "r26_vk_order.txt")


def med(xs):
    m = statistics.median(xs)
    return m, (max(xs) - min(xs)) / m


def scheme(secpar, key_sort):
    import fusion.fusion as F
    from fusion_hip.scheme import BatchScheme
    return BatchScheme(F.fusion_setup(secpar, 7), threads=THREADS, hash_ag="device", key_sort=key_sort)


def pool(bs, n, windows):
    rng = np.random.default_rng(n)
    h = (bs.q - 1) // 2
    m = n + windows * 16
    return (rng.integers(-h, h + 1, size=(m, 2, bs.d), dtype=np.int32), rng.integers(0, 256, size=(m, 32), dtype=np.uint8),
            rng.integers(-h, h + 1, size=(m, bs.d), dtype=np.int32))


def step_cell(host, dev, sizes):
    from fusion_hip.context import DeviceScope
    from fusion_hip.scheme import _Committees
    ctx = host.ctx
    n = sum(sizes)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    VK, PRE, C = pool(host, n, REPS + 1)
    forms = ("host sort", "+ key download", "device sort", "entry")
    t = {f: [] for f in forms}
    for r in range(REPS + 1):                               # repetition 0 warms up
        vk, pre, c = (np.ascontiguousarray(a[16 * r:16 * r + n]) for a in (VK, PRE, C))
        L, R = np.ascontiguousarray(vk[:, 0]), np.ascontiguousarray(vk[:, 1])
        with DeviceScope() as s:
            dK, dC, dP = host._up(s, vk), host._up(s, c), host._up(s, pre)
            outs = {}
            for f in forms if r % 2 else forms[::-1]:
                ctx.synchronize()
                if f == "entry":
                    dAl = dev._new(s, (n, dev.d))
                    ctx.timer_start()
                    ctx.hash_ag_ragged_sorted_dev(dev.P, dK.ptr, dP.ptr, dC.ptr, n, off, None, dAl.ptr)
                    ms = ctx.timer_stop_ms()
                else:
                    # the call's inputs as its challenge pass leaves them: the digests on the device under the device sort, else on
                    # the host beside a host copy of the keys -- which "+ key download" leaves alpha_hat to fetch from the device
                    m = _Committees(dev if f == "device sort" else host, s, dK, None, sizes)
                    m.dK, m.dC = dK, dC
                    if f == "device sort":
                        m.dP = dP
                    else:
                        m.pre = pre
                    if f == "host sort":
                        m.L, m.R = L, R
                    t0 = time.perf_counter()
                    dAl = m.alpha_hat()
                    ctx.synchronize()
                    ms = (time.perf_counter() - t0) * 1e3
                outs[f] = dAl
                if r:
                    t[f].append(ms)
            if r == 0 and n <= 16384:
                assert np.array_equal(outs["host sort"].numpy(), outs["device sort"].numpy()), "the two sorts differ"
    return {f: med(v) for f, v in t.items()}


def part_step(secpar):
    host, dev = scheme(secpar, "host"), scheme(secpar, "device")
    print(f"secpar {secpar}: the hash_ag step under hash_ag=\"device\", ms (median of {REPS}, spread); threads={THREADS}")
    print(f"{'G x n':>10} {'host sort':>16} {'+ key download':>16} {'device sort':>16} {'entry':>16} {'host/device':>11}")
    for g in GS:
        for n in NS:
            res = step_cell(host, dev, [n] * g)
            a, b, c, e = res["host sort"], res["+ key download"], res["device sort"], res["entry"]
            print(f"{g:>5}x{n:<4} {a[0]:>9.3f} {a[1]:>5.0%} {b[0]:>9.3f} {b[1]:>5.0%} {c[0]:>9.3f} {c[1]:>5.0%} {e[0]:>9.3f} {e[1]:>5.0%} "
                  f"{a[0] / c[0]:>11.2f}", flush=True)
    host.close()
    dev.close()


def part_call(secpar):
    host, dev = scheme(secpar, "host"), scheme(secpar, "device")
    print(f"secpar {secpar}: aggregate_verify_many_encoded under hash_ag=\"device\", ms (median of {REPS}, spread); threads={THREADS}")
    print(f"{'G x n':>10} {'host sort':>16} {'host sort, keys':>16} {'device sort':>16} {'device sort, keys':>17} {'ratio':>6} {'ratio':>6}")
    print(f"{'':>10} {'':>16} {'on the device':>16} {'':>16} {'on the device':>17} {'host':>6} {'device':>6}")
    for g in GS:
        for n in NS:
            if g * n > CALL_MAX:
                continue
            N, sizes = g * n, [n] * g
            forms = (("host sort", host, False), ("host sort, dev", host, True), ("device sort", dev, False), ("device sort, dev", dev, True))
            t = {f[0]: [] for f in forms}
            for r in range(REPS + 1):                       # fresh keys and messages every repetition; repetition 0 warms up
                seeds = [1_000_003 * (r + 1) + 7 * i for i in range(N)]
                msgs = [f"probe {r} {i}" for i in range(N)]
                sk, vk, vk_dev = host.keygen_batch(seeds, device=True, keep_vk=True)
                data, codes = host.sign_batch_encoded(sk, vk_dev, msgs, device=True)
                sk.free()
                assert not codes.any()
                out = {}
                for f, bs, on_device in forms if r % 2 else forms[::-1]:
                    bs.ctx.synchronize()
                    t0 = time.perf_counter()
                    out[f] = bs.aggregate_verify_many_encoded(vk_dev if on_device else vk, msgs, data, sizes)
                    ms = (time.perf_counter() - t0) * 1e3
                    if r:
                        t[f].append(ms)
                for f in out:
                    assert np.array_equal(out[f][0], out["host sort"][0]) and out[f][2] == [(True, "")] * g, f
                vk_dev.free()
                data.free()
            m = {f: med(v) for f, v in t.items()}
            a, b, c, e = m["host sort"], m["host sort, dev"], m["device sort"], m["device sort, dev"]
            print(f"{g:>5}x{n:<4} {a[0]:>9.3f} {a[1]:>5.0%} {b[0]:>9.3f} {b[1]:>5.0%} {c[0]:>9.3f} {c[1]:>5.0%} {e[0]:>10.3f} {e[1]:>5.0%} "
                  f"{a[0] / c[0]:>6.2f} {b[0] / e[0]:>6.2f}", flush=True)
    host.close()
    dev.close()


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    if what == "step":
        return part_step(int(sys.argv[2]))
    if what == "call":
        return part_call(int(sys.argv[2]))
    lines = []
    for part in ("step", "call"):
        for secpar in ("128", "256"):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), part, secpar], capture_output=True, text=True, timeout=600)
            print(r.stdout + r.stderr[-2000:], flush=True)
            if r.returncode:                                # after a failed part nothing more is started on the device
                sys.exit(f"part {part} {secpar} failed with status {r.returncode}")
            lines.append(r.stdout)
    with open(OUT, "w") as fh:
        fh.write("the key sort of hash_ag for many committees, device against host (python tools/probes/vk_order.py all; the columns: its "
                 "docstring)\n\n")
        fh.write("\n".join(lines))


if __name__ == "__main__":
    main()
