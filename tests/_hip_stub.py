"""A stub HIP runtime for host-only builds of the library's host logic, shared by tests/test_context_host.py and
tests/test_queue_host.py: STUB is C++ text that a driver program starts with.  Device and pinned memory are malloc / free (so
AddressSanitizer sees a read of a block that was released too early, and leak detection a block that never was), streams, events
and graphs are small heap objects.  Every call is logged under a mutex with its pointer, size, stream, source pointer and copy
kind, a global sequence number (stub_seq(): a driver may stamp records of its own from the same counter) and a small integer
naming the calling thread (stub_tid()).  Controls: "the stream is capturing", "the k-th allocation (or event creation)
fails", "hipMemcpy touches nothing" and "a large hipMalloc is backed by one byte" (drivers that hand over dummy pointers).
build_driver() compiles units of csrc host-only with a sanitizer and links them with a driver into a stand-alone program."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fusion-cryptography_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HOSTCXX = os.environ.get("HOSTCXX", "/opt/rocm/lib/llvm/bin/clang++")

STUB = r'''
#include "fz_internal.h"
#include "fusion_hip.h"
#include "fusion_hip_diag.h"
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <set>
#include <string>
#include <vector>

// ---- the stub runtime ------------------------------------------------------------------------------------------------
struct ihipStream_t { int capturing; };
struct ihipEvent_t { int recorded; };
struct ihipGraph { int nodes; };
struct hipGraphExec { int nodes; };
// kind: the hipMemcpyKind of a copy (-1 otherwise); src: its source; seq: position among ALL records of the process; tid: the caller
struct Call { std::string fn; const void *p; size_t n; const void *stream; const void *src; int kind; unsigned long seq; int tid; };
static std::mutex g_log_mu;                            // guards the log, the sequence counter and the controls' counters
static std::vector<Call> g_log;
static unsigned long g_seq = 0;
static long g_live_allocs = 0, g_live_events = 0, g_live_streams = 0;      // what exists now (device + pinned blocks; events; streams)
static bool g_report_capture = false;                 // control: hipStreamIsCapturing reports an active capture
static long g_fail_at = -1, g_allocs = 0;             // control: allocations [g_fail_at, g_fail_at + g_fail_n) fail
static int g_fail_n = 1;
static long g_fail_event_at = -1, g_events = 0;       // ... and this event creation
static bool g_copy_nothing = false;                   // control: hipMemcpy and hipMemcpyAsync log and touch no memory (a driver whose pointers are dummies)
static size_t g_fake_above = 0;                       // control: a hipMalloc of more bytes than this (0: never) is logged with its size, backed by 1 byte
static int stub_tid() {
    static std::atomic<int> next(0);
    static thread_local int id = next++;
    return id;
}
static unsigned long stub_seq() { std::lock_guard<std::mutex> g(g_log_mu); return g_seq++; }
static void rec(const char *fn, const void *p = nullptr, size_t n = 0, const void *stream = nullptr, const void *src = nullptr, int kind = -1,
                long d_allocs = 0, long d_events = 0, long d_streams = 0) {
    const int tid = stub_tid();
    std::lock_guard<std::mutex> g(g_log_mu);
    g_log.push_back({fn, p, n, stream, src, kind, g_seq++, tid});
    g_live_allocs += d_allocs;
    g_live_events += d_events;
    g_live_streams += d_streams;
}
static std::vector<Call> stub_log(size_t mark = 0) {            // a copy of the records from `mark` on (other threads may be logging)
    std::lock_guard<std::mutex> g(g_log_mu);
    return std::vector<Call>(g_log.begin() + (long)std::min(mark, g_log.size()), g_log.end());
}
static size_t stub_mark() { std::lock_guard<std::mutex> g(g_log_mu); return g_log.size(); }
static void stub_live(long *allocs, long *events, long *streams) {
    std::lock_guard<std::mutex> g(g_log_mu);
    *allocs = g_live_allocs; *events = g_live_events; *streams = g_live_streams;
}
static bool alloc_fails() {
    std::lock_guard<std::mutex> g(g_log_mu);
    const long k = g_allocs++;
    return g_fail_at >= 0 && k >= g_fail_at && k < g_fail_at + g_fail_n;
}
static hipError_t new_event(hipEvent_t *e) {
    {
        std::lock_guard<std::mutex> g(g_log_mu);
        if (g_events++ == g_fail_event_at) { *e = nullptr; return hipErrorOutOfMemory; }
    }
    *e = new ihipEvent_t{0};
    rec("hipEventCreate", *e, 0, nullptr, nullptr, -1, 0, 1);
    return hipSuccess;
}
static hipError_t new_stream(hipStream_t *s) { *s = new ihipStream_t{0}; rec("hipStreamCreate", *s, 0, nullptr, nullptr, -1, 0, 0, 1); return hipSuccess; }
extern "C" {
const char *hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : "stub error"; }
hipError_t hipGetLastError(void) { return hipSuccess; }
hipError_t hipGetDeviceCount(int *n) { *n = 1; return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipRuntimeGetVersion(int *v) { *v = HIP_VERSION; return hipSuccess; }
hipError_t hipGetDeviceProperties(hipDeviceProp_t *p, int) {
    memset(p, 0, sizeof(*p));
    p->multiProcessorCount = 256;
    snprintf(p->gcnArchName, sizeof(p->gcnArchName), "gfx950:sramecc+:xnack-");
    return hipSuccess;
}
hipError_t hipMalloc(void **p, size_t n) {
    if (alloc_fails()) { rec("hipMalloc failed", nullptr, n); return hipErrorOutOfMemory; }
    *p = malloc(g_fake_above && n > g_fake_above ? 1 : (n ? n : 1));
    rec("hipMalloc", *p, n, nullptr, nullptr, -1, 1);
    return hipSuccess;
}
hipError_t hipFree(void *p) { rec("hipFree", p, 0, nullptr, nullptr, -1, p ? -1 : 0); free(p); return hipSuccess; }
hipError_t hipHostMalloc(void **p, size_t n, unsigned) {
    if (alloc_fails()) { rec("hipHostMalloc failed", nullptr, n); return hipErrorOutOfMemory; }
    *p = malloc(n ? n : 1);
    rec("hipHostMalloc", *p, n, nullptr, nullptr, -1, 1);
    return hipSuccess;
}
hipError_t hipHostFree(void *p) { rec("hipHostFree", p, 0, nullptr, nullptr, -1, p ? -1 : 0); free(p); return hipSuccess; }
hipError_t hipMemcpy(void *d, const void *s, size_t n, hipMemcpyKind k) { rec("hipMemcpy", d, n, nullptr, s, (int)k); if (!g_copy_nothing) memcpy(d, s, n); return hipSuccess; }
hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, hipMemcpyKind k, hipStream_t st) { rec("hipMemcpyAsync", d, n, st, s, (int)k); if (!g_copy_nothing) memcpy(d, s, n); return hipSuccess; }
hipError_t hipMemsetAsync(void *d, int v, size_t n, hipStream_t st) { rec("hipMemsetAsync", d, n, st); if (n) memset(d, v, n); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t st) { rec("hipStreamSynchronize", nullptr, 0, st); return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) { return new_stream(s); }
hipError_t hipStreamCreateWithPriority(hipStream_t *s, unsigned, int) { return new_stream(s); }
hipError_t hipDeviceGetStreamPriorityRange(int *least, int *greatest) { *least = 0; *greatest = -1; return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t s) { rec("hipStreamDestroy", s, 0, nullptr, nullptr, -1, 0, 0, -1); delete s; return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t st, hipEvent_t e, unsigned) { rec("hipStreamWaitEvent", e, 0, st); return hipSuccess; }
hipError_t hipStreamBeginCapture(hipStream_t st, hipStreamCaptureMode) { rec("hipStreamBeginCapture", nullptr, 0, st); st->capturing = 1; return hipSuccess; }
hipError_t hipStreamEndCapture(hipStream_t st, hipGraph_t *g) { rec("hipStreamEndCapture", nullptr, 0, st); st->capturing = 0; *g = new ihipGraph{1}; return hipSuccess; }
hipError_t hipStreamIsCapturing(hipStream_t st, hipStreamCaptureStatus *out) {
    *out = (g_report_capture || st->capturing) ? hipStreamCaptureStatusActive : hipStreamCaptureStatusNone;
    return hipSuccess;
}
hipError_t hipGraphInstantiate(hipGraphExec_t *ex, hipGraph_t, hipGraphNode_t *, char *, size_t) { *ex = new hipGraphExec{1}; return hipSuccess; }
hipError_t hipGraphLaunch(hipGraphExec_t, hipStream_t st) { rec("hipGraphLaunch", nullptr, 0, st); return hipSuccess; }
hipError_t hipGraphExecDestroy(hipGraphExec_t ex) { delete ex; return hipSuccess; }
hipError_t hipGraphDestroy(hipGraph_t g) { delete g; return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t *e) { return new_event(e); }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { return new_event(e); }
hipError_t hipEventDestroy(hipEvent_t e) { rec("hipEventDestroy", e, 0, nullptr, nullptr, -1, 0, -1); delete e; return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t st) { rec("hipEventRecord", e, 0, st); e->recorded = 1; return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t e) { rec("hipEventSynchronize", e); return hipSuccess; }
hipError_t hipEventElapsedTime(float *ms, hipEvent_t, hipEvent_t) { *ms = 1.0f; return hipSuccess; }
}
// what fz_context.hip and fz_diag.hip take from the kernel units: the setup of each unit (none is linked), and fz_ntt.hip's helpers
int fz_ntt_query_grid(fz_ctx *) { return FZ_OK; }
int fz_records_query_grid(fz_ctx *) { return FZ_OK; }
int fz_aggregate_encoded_query_grid(fz_ctx *) { return FZ_OK; }
int fz_verify_encoded_setup(fz_ctx *) { return FZ_OK; }
int fz_sign_encoded_query_grid(fz_ctx *) { return FZ_OK; }
int fz_aggregate_many_encoded_query_grid(fz_ctx *) { return FZ_OK; }
int fz_sign_records_query_grid(fz_ctx *) { return FZ_OK; }
int fz_keygen_records_query_grid(fz_ctx *) { return FZ_OK; }
int fz_launch_diag(fz_ctx *, int, const void *, void *, size_t) { return FZ_OK; }
int fz_launch_diag_clock(hipStream_t, unsigned long long, unsigned long long *) { return FZ_OK; }
unsigned fz_multi_plan(const FzMultiJobs &, int, const FzProduced *, int, bool, unsigned, int *, unsigned *, int *, int *) { return 0; }
'''


def toolchain():
    """-> (hipcc, host compiler, ROCm root); skips when hipcc is missing"""
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not available")
    hostcxx = HOSTCXX if os.path.exists(HOSTCXX) else "clang++"
    return HIPCC, hostcxx, os.path.dirname(os.path.dirname(shutil.which(HIPCC) or HIPCC))


def sanitizer_links(tmp_path, san):
    """does an empty program link with this sanitizer (its runtime is installed)?  A real build failure is then an error, not a skip."""
    _, hostcxx, _ = toolchain()
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    return subprocess.run([hostcxx, san, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode == 0


def fatbin_definitions(objs):
    """C++ text that defines the fat-binary symbol each host-only object of a unit WITH kernels refers to (its registration code
    takes the symbol's address; a stub runtime never reads it)"""
    _, hostcxx, _ = toolchain()
    nm = os.path.join(os.path.dirname(hostcxx), "llvm-nm")
    names = set()
    for obj in objs:
        out = subprocess.check_output([nm if os.path.exists(nm) else "nm", "-u", obj], text=True)
        names.update(line.split()[-1] for line in out.splitlines() if "__hip_fatbin_" in line)
    return "".join('extern "C" { extern const char %s[16]; const char %s[16] = {0}; }\n' % (n, n) for n in sorted(names))


def build_driver(tmp_path, units, driver_text, san, name="driver", sources=(), flags=(), late_text=None):
    """units of csrc compiled host-only (hipcc) with `san`, linked with the driver (STUB + the test's own code) and `sources`
    (plain C++ files of csrc) -> path of the program.  late_text(objects) -> C++ text appended to the driver once the units are
    compiled (fatbin_definitions, for units that hold kernels)."""
    hipcc, hostcxx, rocm = toolchain()
    objs = []
    for unit in units:
        objs.append(str(tmp_path / ("%s_%s.o" % (name, unit))))
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-Xarch_host", san,
                               "-c", os.path.join(CSRC, unit + ".hip"), "-o", objs[-1]])
    src = tmp_path / (name + ".cpp")
    src.write_text(driver_text + (late_text(objs) if late_text else ""))
    exe = tmp_path / name
    subprocess.check_call([hostcxx, "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                           "-std=c++17", "-O1", "-g", san, "-pthread"] + list(flags) + [str(src)] + [str(s) for s in sources] + objs + ["-o", str(exe)])
    return exe
