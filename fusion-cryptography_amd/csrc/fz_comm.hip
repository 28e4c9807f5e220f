// fz_comm.hip -- the exchange steps of the path in the C ABI (include/fusion_hip.h): the RCCL binding and the collectives on
// the context's stream.
#include "fz_internal.h"
#include "../../include/fusion_hip.h"
#include "../../include/fusion_hip_diag.h"

#include <cstdio>
#include <cstring>
#include <new>
#include <algorithm>
#include <vector>
#include <string>
#include <dlfcn.h>
#include <mutex>

extern "C" {

// ---- the one exchange step of the path, in the C ABI: RCCL all-reduce of the int64 partial sums ---------------------
// RCCL is bound lazily (dlopen): the library loads and every other entry point works on a machine without it.
// WHICH copy is bound is an ownership question (VERDICT / ADVICE r04: an abort at process exit): a torch wheel ships its
// own librccl.so under the soname librccl.so.1 but asks for it by the unversioned file name, so a process that bound
// /opt/rocm's copy by soname first and imported torch afterwards carried TWO RCCLs of different ROCm releases -- and with
// RTLD_GLOBAL (rounds 2-4) the first copy's nccl* symbols interposed on the second's callers.  The rule now:
//   1. a copy already mapped under the soname serves (RTLD_NOLOAD): whoever loaded it owns it, we share it;
//   2. otherwise the copy that ships BESIDE THE HIP RUNTIME THIS PROCESS RUNS ON (dladdr of a HIP entry point: torch/lib when
//      fusion_hip mapped the wheel's runtime first, /opt/rocm/lib otherwise), opened by path -- a later `import torch` then finds
//      the same file (same device / inode) already mapped instead of adding a second copy;
//   3. otherwise the soname on the default search path.
// Always RTLD_LOCAL (nothing of RCCL enters the global scope), never dlclose'd (RCCL's own teardown runs at exit, after ours).
namespace {
struct RcclApi {
    void *handle;
    int (*GetUniqueId)(void *);
    int (*CommInitRank)(void **, int, fz_unique_id, int);
    int (*CommDestroy)(void *);
    int (*AllReduce)(const void *, void *, size_t, int, int, void *, hipStream_t);
    const char *(*GetErrorString)(int);
    int (*CommCount)(void *, int *);
    int (*GetVersion)(int *);
    int (*Broadcast)(const void *, void *, size_t, int, int, void *, hipStream_t);
    int (*ReduceScatter)(const void *, void *, size_t, int, int, void *, hipStream_t);
    char path[512];      // the file the symbols came from
    char how[64];        // which of the three rules found it
};
RcclApi g_rccl = {};
std::mutex g_rccl_mu;                       // binding and the registry of live communicators
std::vector<fz_comm *> g_live_comms;

void *rccl_open(char *how, size_t how_cap) {
    void *h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL | RTLD_NOLOAD);
    if (h) { snprintf(how, how_cap, "already mapped (shared)"); return h; }
    Dl_info di;
    if (dladdr((const void *)&hipGetDeviceCount, &di) && di.dli_fname) {
        std::string dir(di.dli_fname);
        const size_t cut = dir.rfind('/');
        if (cut != std::string::npos) {
            dir.resize(cut + 1);
            for (const char *n : {"librccl.so.1", "librccl.so"}) {
                h = dlopen((dir + n).c_str(), RTLD_NOW | RTLD_LOCAL);
                if (h) { snprintf(how, how_cap, "beside the HIP runtime"); return h; }
            }
        }
    }
    for (const char *n : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
        h = dlopen(n, RTLD_NOW | RTLD_LOCAL);
        if (h) { snprintf(how, how_cap, "default search path"); return h; }
    }
    return nullptr;
}

int rccl_bind() {
    std::lock_guard<std::mutex> lk(g_rccl_mu);
    if (g_rccl.handle) return FZ_OK;
    RcclApi a = {};
    void *h = nullptr;
    try {
        h = rccl_open(a.how, sizeof a.how);
    } catch (const std::bad_alloc &) {
        return fz_set_error(FZ_E_HIP, "out of host memory");
    }
    if (!h) return fz_set_error(FZ_E_RCCL, "RCCL not found (librccl.so.1): %s", dlerror());
    a.GetUniqueId = (int (*)(void *))dlsym(h, "ncclGetUniqueId");
    a.CommInitRank = (int (*)(void **, int, fz_unique_id, int))dlsym(h, "ncclCommInitRank");
    a.CommDestroy = (int (*)(void *))dlsym(h, "ncclCommDestroy");
    a.AllReduce = (int (*)(const void *, void *, size_t, int, int, void *, hipStream_t))dlsym(h, "ncclAllReduce");
    a.GetErrorString = (const char *(*)(int))dlsym(h, "ncclGetErrorString");
    a.CommCount = (int (*)(void *, int *))dlsym(h, "ncclCommCount");
    a.GetVersion = (int (*)(int *))dlsym(h, "ncclGetVersion");
    a.Broadcast = (int (*)(const void *, void *, size_t, int, int, void *, hipStream_t))dlsym(h, "ncclBroadcast");
    a.ReduceScatter = (int (*)(const void *, void *, size_t, int, int, void *, hipStream_t))dlsym(h, "ncclReduceScatter");
    if (!a.GetUniqueId || !a.CommInitRank || !a.CommDestroy || !a.AllReduce || !a.GetErrorString)
        return fz_set_error(FZ_E_RCCL, "librccl.so.1 lacks an expected symbol");      // (the handle stays open: never dlclose)
    Dl_info di;
    snprintf(a.path, sizeof a.path, "%s", dladdr((const void *)a.AllReduce, &di) && di.dli_fname ? di.dli_fname : "?");
    a.handle = h;
    g_rccl = a;
    return FZ_OK;
}

int rccl_check(int rc, const char *what) {
    if (rc == 0) return FZ_OK;
    return fz_set_error(FZ_E_RCCL, "%s: %s", what, g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "RCCL error");
}
}  // namespace

struct fz_comm {
    void *comm;          // ncclComm_t
    int nranks, rank, device;
};

int fz_comm_unique_id(fz_unique_id *out_id) {
    FZ_REQUIRE(out_id, "out_id is NULL");
    FZ_TRY(rccl_bind());
    return rccl_check(g_rccl.GetUniqueId(out_id), "ncclGetUniqueId");
}

int fz_comm_create(fz_ctx *ctx, int nranks, int rank, const fz_unique_id *id, fz_comm **out) {
    FZ_REQUIRE(ctx && id && out && nranks >= 1 && rank >= 0 && rank < nranks, "bad argument");
    *out = nullptr;
    FZ_DEV(ctx);                                          // the communicator binds to the CURRENT device
    FZ_TRY(rccl_bind());
    void *c = nullptr;
    FZ_TRY(rccl_check(g_rccl.CommInitRank(&c, nranks, *id, rank), "ncclCommInitRank"));
    fz_comm *C = new (std::nothrow) fz_comm();
    if (!C) { g_rccl.CommDestroy(c); return fz_set_error(FZ_E_HIP, "out of host memory"); }
    C->comm = c; C->nranks = nranks; C->rank = rank; C->device = ctx->device;
    try {
        std::lock_guard<std::mutex> lk(g_rccl_mu);
        g_live_comms.push_back(C);
    } catch (const std::bad_alloc &) {
        g_rccl.CommDestroy(c);
        delete C;
        return fz_set_error(FZ_E_HIP, "out of host memory");
    }
    *out = C;
    return FZ_OK;
}

// Idempotent: a handle that is not (or no longer) in the registry of live communicators is left alone -- a second destroy
// of the same handle returns FZ_OK without touching RCCL or the freed wrapper.  Communicators still alive when the
// process ends are NOT destroyed by this library (no static destructor, no atexit hook: ncclCommDestroy talks to the
// device, and by then the HIP runtime's own teardown may have begun); RCCL's teardown owns them.
int fz_comm_destroy(fz_comm *comm) {
    if (!comm) return FZ_OK;
    {
        std::lock_guard<std::mutex> lk(g_rccl_mu);
        auto it = std::find(g_live_comms.begin(), g_live_comms.end(), comm);
        if (it == g_live_comms.end()) return FZ_OK;
        g_live_comms.erase(it);
    }
    int rc = FZ_OK;
    if (comm->comm && g_rccl.CommDestroy) {
        (void)hipSetDevice(comm->device);
        (void)hipDeviceSynchronize();                    // nothing of ours may still be using the communicator's streams
        rc = rccl_check(g_rccl.CommDestroy(comm->comm), "ncclCommDestroy");
    }
    comm->comm = nullptr;
    delete comm;
    return rc;
}

// which RCCL serves this process: the file the symbols were bound from, the rule that found it ("already mapped (shared)" |
// "beside the HIP runtime" | "default search path"), and how many DIFFERENT files named librccl* the process has mapped
// (more than one = two copies, the state the binding rule exists to avoid)
int fz_rccl_library(char *out_path, size_t path_cap, char *out_how, size_t how_cap, int *out_copies_mapped) {
    FZ_TRY(rccl_bind());
    if (out_path && path_cap) snprintf(out_path, path_cap, "%s", g_rccl.path);
    if (out_how && how_cap) snprintf(out_how, how_cap, "%s", g_rccl.how);
    if (out_copies_mapped) try {
        std::vector<std::string> seen;
        if (FILE *f = fopen("/proc/self/maps", "r")) {
            char line[1024];
            while (fgets(line, sizeof line, f)) {
                const char *p = strchr(line, '/');
                if (!p || !strstr(p, "librccl")) continue;
                std::string path(p);
                while (!path.empty() && (path.back() == '\n' || path.back() == ' ')) path.pop_back();
                if (std::find(seen.begin(), seen.end(), path) == seen.end()) seen.push_back(path);
            }
            fclose(f);
        }
        *out_copies_mapped = (int)seen.size();
    } catch (const std::bad_alloc &) {
        return fz_set_error(FZ_E_HIP, "out of host memory");
    }
    return FZ_OK;
}

int fz_comm_info(fz_comm *comm, int *out_nranks, int *out_rank) {
    FZ_REQUIRE(comm, "comm is NULL");
    int n = comm->nranks;
    if (g_rccl.CommCount) FZ_TRY(rccl_check(g_rccl.CommCount(comm->comm, &n), "ncclCommCount"));   // what RCCL itself reports
    if (out_nranks) *out_nranks = n;
    if (out_rank) *out_rank = comm->rank;
    return FZ_OK;
}

int fz_rccl_version(int *out_version) {
    FZ_REQUIRE(out_version, "out_version is NULL");
    *out_version = 0;
    FZ_TRY(rccl_bind());
    if (!g_rccl.GetVersion) return fz_set_error(FZ_E_RCCL, "librccl.so.1 lacks ncclGetVersion");
    return rccl_check(g_rccl.GetVersion(out_version), "ncclGetVersion");
}

int fz_broadcast_i32(fz_ctx *ctx, fz_comm *comm, int32_t *d_buf, size_t count, int root) {
    FZ_REQUIRE(ctx && comm && (count == 0 || d_buf), "NULL argument");
    FZ_REQUIRE(root >= 0 && root < comm->nranks, "root outside the communicator");
    if (comm->device != ctx->device) return fz_set_error(FZ_E_BADARG, "communicator was created on device %d", comm->device);
    FZ_DEV(ctx);
    if (count == 0) return FZ_OK;
    if (!g_rccl.Broadcast) return fz_set_error(FZ_E_RCCL, "librccl.so.1 lacks ncclBroadcast");
    // in place, ncclInt32 (= 2), on the context's stream like the all-reduce
    return rccl_check(g_rccl.Broadcast(d_buf, d_buf, count, 2, root, comm->comm, ctx->stream), "ncclBroadcast");
}

int fz_reduce_scatter_i64(fz_ctx *ctx, fz_comm *comm, int64_t *d_buf, size_t count_per_rank) {
    FZ_REQUIRE(ctx && comm && (count_per_rank == 0 || d_buf), "NULL argument");
    if (comm->device != ctx->device) return fz_set_error(FZ_E_BADARG, "communicator was created on device %d", comm->device);
    FZ_DEV(ctx);
    if (count_per_rank == 0) return FZ_OK;
    if (!g_rccl.ReduceScatter) return fz_set_error(FZ_E_RCCL, "librccl.so.1 lacks ncclReduceScatter");
    // in place (NCCL's convention: the receive buffer is this rank's block of the send buffer), ncclInt64 (= 4), ncclSum (= 0)
    return rccl_check(g_rccl.ReduceScatter(d_buf, d_buf + (size_t)comm->rank * count_per_rank, count_per_rank, 4, 0, comm->comm, ctx->stream),
                      "ncclReduceScatter");
}

int fz_allreduce_i64(fz_ctx *ctx, fz_comm *comm, int64_t *d_buf, size_t count) {
    FZ_REQUIRE(ctx && comm && (count == 0 || d_buf), "NULL argument");
    if (comm->device != ctx->device) return fz_set_error(FZ_E_BADARG, "communicator was created on device %d", comm->device);
    FZ_DEV(ctx);
    if (count == 0) return FZ_OK;
    // in place, ncclInt64 (= 4), ncclSum (= 0), on the context's stream: ordered with the kernels around it and
    // capturable by fz_graph_* like them
    return rccl_check(g_rccl.AllReduce(d_buf, d_buf, count, 4, 0, comm->comm, ctx->stream), "ncclAllReduce");
}

}  // extern "C"
