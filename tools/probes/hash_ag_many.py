"""hash_ag for many committees: the device form (fz_hash_ag_ragged_dev, a wave per committee) against the host form
(the host form of fusion_hip.scheme._Committees.alpha_hat, on the scheme's thread pool), on the same box and in the same process.

Per cell G x n (G committees of n signers) and parameter set:
  step   the hash_ag step alone, from what the challenge pass leaves (keys, pre-hashes, c_hat) to alpha_hat on the device:
           entry   fz_hash_ag_ragged_dev by device events (memset, kernel, transform), order list given
           device  _Committees.alpha_hat in its device form, wall clock to a synchronise: the ragged key sort, the upload of the pre-hashes, the entry
           host    _Committees.alpha_hat under hash_ag="host" with threads=THREADS, wall clock to a synchronise (the c_hat
                   download before it is not counted; the upload and transform of the coefficients are: they are its own)
         on synthetic centred rows (the entry takes any), a fresh window of a larger pool for every repetition; medians of REPS
         repetitions, the forms alternating; spread = (max - min) / median.
         perm/s: the kernel's permutations (text blocks absorbed + stream blocks squeezed, from the mean item length of a sample
         of 64 signers) over the entry's time.
         order   the entry again under FZ_HASH_AG_ORDER=0 (the caller's order) on committees of MIXED sizes: the launch-order A/B.
  call   aggregate_verify_many_encoded on real keys and records, hash_ag="host" against "device", wall clock, medians of REPS;
         cells of up to CALL_MAX signers (the keys of larger ones do not fit a probe's minutes), "auto"'s choice beside them.
Run from the repository root on a GPU box: python tools/probes/hash_ag_many.py [all | step SECPAR | call SECPAR | order SECPAR];
`all` runs every part in a process of its own and writes profiles/r25_hash_ag_many.txt."""
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
OUT = os.path.join(ROOT, "profiles", "r25_hash_ag_many.txt")


def med(xs):
    m = statistics.median(xs)
    return m, (max(xs) - min(xs)) / m


def scheme(secpar, hash_ag="host"):
    import fusion.fusion as F
    from fusion_hip.scheme import BatchScheme
    return BatchScheme(F.fusion_setup(secpar, 7), threads=THREADS, hash_ag=hash_ag)


def perms_per_signer(bs, vk, pre, c):
    """blocks absorbed + squeezed per signer, from the exact item text of up to 64 signers"""
    from fusion_hip import hostpipe
    wrap = len("GeneralMatrix(elem_class=<class 'algebra.polynomials.PolynomialNTTRepresentation'>, matrix=[[]])")
    key = len("OneTimeVerificationKey(left_vk_hat=, right_vk_hat=)")
    k = min(64, len(vk))
    text = 0
    for i in range(k):
        poly = (len(hostpipe.format_vk(bs.P, c[i], c[i])) - key) // 2 - wrap
        text += len(hostpipe.format_vk(bs.P, vk[i, 0], vk[i, 1])) + len(str(int.from_bytes(bytes(pre[i]), "little"))) + poly
        text += len("(, , SignatureChallenge(c_hat=)), ")
    p = bs.params
    section = (p.omega_ag + 7) // 8 + (-(-(1 + p.secpar) // 8) + -(-(int(np.log2(bs.d)) + p.secpar) // 8)) * p.omega_ag
    return (text / k + section) / 136.0


def pool(bs, n, windows):
    rng = np.random.default_rng(n)
    h = (bs.q - 1) // 2
    m = n + windows * 16
    vk = rng.integers(-h, h + 1, size=(m, 2, bs.d), dtype=np.int32)
    c = rng.integers(-h, h + 1, size=(m, bs.d), dtype=np.int32)
    pre = rng.integers(0, 256, size=(m, 32), dtype=np.uint8)
    return vk, pre, c


def step_cell(bs, sizes, reps=REPS, forms=("entry", "device", "host")):
    from fusion_hip.context import DeviceScope
    from fusion_hip import hostpipe
    from fusion_hip.scheme import _Committees
    ctx = bs.ctx
    n = sum(sizes)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    VK, PRE, C = pool(bs, n, reps + 1)
    t = {f: [] for f in forms}
    for r in range(reps + 1):                               # repetition 0 warms up
        vk, pre, c = (np.ascontiguousarray(a[16 * r:16 * r + n]) for a in (VK, PRE, C))
        L, R = np.ascontiguousarray(vk[:, 0]), np.ascontiguousarray(vk[:, 1])
        with DeviceScope() as s:
            dK, dC = bs._up(s, vk), bs._up(s, c)
            for f in forms:
                ctx.synchronize()
                if f == "entry":
                    order = hostpipe.sort_by_vk_string_ragged(bs.P, L, R, off, THREADS)
                    dP, dAl = bs._up(s, pre), bs._new(s, (n, bs.d))
                    ctx.timer_start()
                    ctx.hash_ag_ragged_dev(bs.P, dK.ptr, dP.ptr, dC.ptr, n, order, off, dAl.ptr)
                    ms = ctx.timer_stop_ms()
                    a_dev = dAl
                else:
                    # the call's inputs as the challenge pass leaves them; bs has hash_ag="host": device_only picks the device form
                    m = _Committees(bs, s, vk, None, sizes, device_only=f == "device")
                    m.dK, m.dC, m.L, m.R, m.pre, m.c_hat = dK, dC, L, R, pre, c
                    t0 = time.perf_counter()
                    a = m.alpha_hat()
                    if f == "host":
                        a_host = a
                    ctx.synchronize()
                    ms = (time.perf_counter() - t0) * 1e3
                if r:
                    t[f].append(ms)
            if r == 0 and "host" in forms and "entry" in forms and n <= 4096:
                assert np.array_equal(a_dev.numpy(), a_host.numpy()), "the two forms differ"
    return {f: med(v) for f, v in t.items()}, perms_per_signer(bs, VK[:64], PRE[:64], C[:64]) * n


def part_step(secpar):
    bs = scheme(secpar)
    print(f"secpar {secpar}: the hash_ag step, ms (median of {REPS}, spread); threads={THREADS}")
    print(f"{'G x n':>10} {'entry':>16} {'device':>16} {'host':>16} {'host/device':>11} {'Mperm/s':>8} {'auto':>7}")
    auto = scheme(secpar, "auto")
    for g in GS:
        for n in NS:
            res, perms = step_cell(bs, [n] * g)
            e, dv, h = res["entry"], res["device"], res["host"]
            pick = auto._hash_ag_form([n] * g)
            print(f"{g:>5}x{n:<4} {e[0]:>9.3f} {e[1]:>5.0%} {dv[0]:>9.3f} {dv[1]:>5.0%} {h[0]:>9.3f} {h[1]:>5.0%} {h[0] / dv[0]:>11.2f} "
                  f"{perms / e[0] / 1e3:>8.1f} {pick:>7}{'' if (pick == 'device') == (dv[0] < h[0]) else '  (slower form)'}", flush=True)
    auto.close()
    bs.close()


def part_order(secpar):
    bs = scheme(secpar)
    sizes = [int(x) for x in np.random.default_rng(5).integers(1, 65, size=4096 + 512)]
    sizes[-3:] = [256, 256, 256]                            # three long committees that the caller lists last
    res, _ = step_cell(bs, sizes, forms=("entry",))
    print(f"secpar {secpar}: {len(sizes)} committees of 1..64 signers and three of 256 at the end of the list, "
          f"FZ_HASH_AG_ORDER={os.environ.get('FZ_HASH_AG_ORDER', '1')}: entry {res['entry'][0]:.3f} ms (spread {res['entry'][1]:.0%})", flush=True)
    bs.close()


def part_call(secpar):
    host, dev, auto = scheme(secpar, "host"), scheme(secpar, "device"), scheme(secpar, "auto")
    print(f"secpar {secpar}: aggregate_verify_many_encoded, ms (median of {REPS}, spread); threads={THREADS}")
    print(f"{'G x n':>10} {'host':>16} {'device':>16} {'host/device':>11} {'auto':>7}")
    for g in GS:
        for n in NS:
            if g * n > CALL_MAX:
                continue
            N, sizes = g * n, [n] * g
            t = {"host": [], "device": []}
            for r in range(REPS + 1):                       # fresh keys and messages every repetition; repetition 0 warms up
                seeds = [1_000_003 * (r + 1) + 7 * i for i in range(N)]
                msgs = [f"probe {r} {i}" for i in range(N)]
                sk, vk, vk_dev = host.keygen_batch(seeds, device=True, keep_vk=True)
                data, codes = host.sign_batch_encoded(sk, vk_dev, msgs, device=True)
                sk.free()
                assert not codes.any()
                out = {}
                for f, bs in (("host", host), ("device", dev)) if r % 2 else (("device", dev), ("host", host)):
                    bs.ctx.synchronize()
                    t0 = time.perf_counter()
                    out[f] = bs.aggregate_verify_many_encoded(vk, msgs, data, sizes)
                    ms = (time.perf_counter() - t0) * 1e3
                    if r:
                        t[f].append(ms)
                assert np.array_equal(out["host"][0], out["device"][0]) and out["host"][2] == out["device"][2] == [(True, "")] * g
                vk_dev.free()
                data.free()
            h, dv = med(t["host"]), med(t["device"])
            pick = auto._hash_ag_form(sizes)
            print(f"{g:>5}x{n:<4} {h[0]:>9.3f} {h[1]:>5.0%} {dv[0]:>9.3f} {dv[1]:>5.0%} {h[0] / dv[0]:>11.2f} {pick:>7}"
                  f"{'' if (pick == 'device') == (dv[0] < h[0]) else '  (slower form)'}", flush=True)
    for bs in (host, dev, auto):
        bs.close()


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    if what == "step":
        return part_step(int(sys.argv[2]))
    if what == "call":
        return part_call(int(sys.argv[2]))
    if what == "order":
        return part_order(int(sys.argv[2]))
    lines = []
    for part in ("step", "order", "order0", "call"):
        for secpar in ("128", "256"):
            env = dict(os.environ, FZ_HASH_AG_ORDER="0") if part == "order0" else dict(os.environ)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), part.rstrip("0"), secpar], capture_output=True, text=True, env=env,
                               timeout=900)
            print(r.stdout + r.stderr[-2000:], flush=True)
            if r.returncode:                                # after a failed part nothing more is started on the device
                sys.exit(f"part {part} {secpar} failed with status {r.returncode}")
            lines.append(r.stdout)
    with open(OUT, "w") as fh:
        fh.write("hash_ag of many committees, device against host (python tools/probes/hash_ag_many.py all; the columns: its docstring)\n\n")
        fh.write("\n".join(lines))


if __name__ == "__main__":
    main()
