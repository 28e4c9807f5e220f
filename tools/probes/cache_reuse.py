"""Does a multi-job launch find the previous launch's outputs in the 256 MiB Infinity Cache, and what is a hit worth?
Launch A = J forward jobs x -> y (4096 rows each), launch B = the J inverse jobs y -> z.  B is timed (HIP events on the kernels'
stream) directly after A, after A plus F MiB of filler traffic (fz_diag_copy: F/2 read + F/2 written, non-temporal stores) and
cold (F = 1024), for J = 16 and J = 4; operand sets rotate through a pool of more than 1 GiB and the filler through 2 GiB, so
nothing but A's output can be resident when B starts.  "B never faster than cold": the lines do not stay; "faster only at small
F": they stay and the distance decides.  Control: B timed a second time after B itself (input lines that were LOADED a launch
earlier): if that is faster than cold and B after A is not, a hit pays and it is the stored lines that do not stay.
FZ_MULTI_ORDER (0 | unset) is the launcher's layout of B: the context's record of A makes B's jobs consumers; A
itself has none, so its stores are streaming ones either way.  Output: profiles/r08_cache_reuse.txt"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "fusion-cryptography_amd"))
sys.path.insert(0, ROOT)
import fusion_hip
from fusion_hip._lib import NttJob
from fusion_hip.numa import pin_to_gpu_node
pin_to_gpu_node(0)          # host threads on the GPU's NUMA node (before the first HIP call)
from oracle import oracle as O      # parameters only (tools/ is not product code)

P = O.PARAMS[256]
ctx = fusion_hip.Context(P["q"], P["d"], P["root"], P["inv_root"])
ctx.set_stream(ctx.stream_create())
lib, h = ctx._lib, ctx._h
ROWS, JOB = 4096, 4096 * 1024                 # a job: 4096 rows of 256 int32 = 4 MiB
SETS, JMAX = 8, 16                            # 8 sets x (x, y, z) x 64 MiB = 1.5 GiB
pool = fusion_hip.DeviceBuffer(ctx, SETS * 3 * JMAX * JOB)
FILL = 1 << 30
fsrc, fdst = fusion_hip.DeviceBuffer(ctx, FILL), fusion_hip.DeviceBuffer(ctx, FILL)
ctx.fill_synthetic_dev(pool.ptr, SETS * 3 * JMAX * JOB // 4, 5)
ctx.fill_synthetic_dev(fsrc.ptr, FILL // 4, 6)
ctx.synchronize()


def tables(s, jobs):
    base = pool.ptr + s * 3 * JMAX * JOB
    x, y, z = base, base + JMAX * JOB, base + 2 * JMAX * JOB
    a = (NttJob * jobs)(*[NttJob(x + j * JOB, y + j * JOB, ROWS, 0) for j in range(jobs)])
    b = (NttJob * jobs)(*[NttJob(y + j * JOB, z + j * JOB, ROWS, 1) for j in range(jobs)])
    return a, b


state = {"set": 0, "fill": 0}


def one(jobs, filler_mib, reread=False):
    """A, filler, then B timed -> microseconds of B; reread: A, B, filler, then B again timed (its input was LOADED one launch ago)"""
    a, b = tables(state["set"] % SETS, jobs)
    state["set"] += 1
    assert lib.fz_ntt_multi(h, a, jobs) == 0
    if reread:
        assert lib.fz_ntt_multi(h, b, jobs) == 0
    left = filler_mib << 19                     # bytes to read = bytes to write
    while left > 0:
        n = min(left, 128 << 20)
        if state["fill"] + n > FILL:
            state["fill"] = 0
        ctx.diag_copy_dev(fsrc.ptr + state["fill"], fdst.ptr + state["fill"], n)
        state["fill"] += n
        left -= n
    ctx.timer_start()
    assert lib.fz_ntt_multi(h, b, jobs) == 0
    return ctx.timer_stop_ms() * 1e3


print(f"FZ_MULTI_ORDER={os.environ.get('FZ_MULTI_ORDER', '(unset)')}  library {os.environ.get('FUSION_HIP_LIB', fusion_hip.LIB_PATH)}")
print("B = J inverse jobs of 4096 rows reading what A (J forward jobs) wrote; F MiB of copy traffic between A and B; us = median of 9 (min .. max)")
for jobs in (16, 4):
    for _ in range(20):                         # clocks up, code resident
        one(jobs, 0)
    for f in (0, 64, 128, 192, 256, 384, 1024):
        us = [one(jobs, f) for _ in range(9)]
        moved = 2 * jobs * JOB
        print(f"J={jobs:2d}  F={f:4d} MiB: B {statistics.median(us):7.2f} us ({min(us):7.2f} .. {max(us):7.2f})   "
              f"{moved / statistics.median(us) / 1e3:7.1f} GB/s", flush=True)
    # the control: B run twice, the second timed -- its input lines were loaded (not stored) one launch of 2 J x 4 MiB earlier
    for f in (0, 64, 128, 1024):
        us = [one(jobs, f, reread=True) for _ in range(9)]
        print(f"J={jobs:2d}  F={f:4d} MiB: B again after B {statistics.median(us):7.2f} us ({min(us):7.2f} .. {max(us):7.2f})", flush=True)
