// fz_diag.hip -- measuring and looking inside (include/fusion_hip.h, include/fusion_hip_diag.h): the event timer, per-dispatch
// profiling, what runtime serves the process, the launch-floor probes and the device-side stamp recorder.
#include "fz_internal.h"
#include "../../include/fusion_hip.h"
#include "../../include/fusion_hip_diag.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>

extern "C" {

int fz_timer_start(fz_ctx *ctx) {
    FZ_REQUIRE(ctx, "ctx is NULL");
    FZ_DEV(ctx);
    FZ_HIP(hipEventRecord(ctx->ev0, ctx->stream), "event record");
    return FZ_OK;
}

int fz_timer_stop_ms(fz_ctx *ctx, float *out_ms) {
    FZ_REQUIRE(ctx && out_ms, "NULL argument");
    FZ_DEV(ctx);
    if (fz_capturing(ctx)) return fz_set_error(FZ_E_BADARG, "the timer cannot be read during graph capture");
    FZ_HIP(hipEventRecord(ctx->ev1, ctx->stream), "event record");
    FZ_HIP(hipEventSynchronize(ctx->ev1), "event synchronize");
    FZ_HIP(hipEventElapsedTime(out_ms, ctx->ev0, ctx->ev1), "event elapsed");
    return FZ_OK;
}

int fz_profile_begin(fz_ctx *ctx, int max_launches, int sample_every) {
    FZ_REQUIRE(ctx && max_launches > 0 && max_launches <= (1 << 20) && sample_every >= 1, "bad argument");
    FZ_DEV(ctx);
    if (fz_capturing(ctx)) return fz_set_error(FZ_E_BADARG, "per-dispatch profiling cannot start during graph capture");
    if (max_launches > ctx->prof_cap) {
        // both arrays are replaced and prof_cap covers exactly the events that exist, or nothing changes
        hipEvent_t *ev = (hipEvent_t *)malloc(sizeof(hipEvent_t) * 2 * (size_t)max_launches);
        unsigned char *kind = (unsigned char *)malloc((size_t)max_launches);
        int made = 2 * ctx->prof_cap, rc = ev && kind ? FZ_OK : fz_set_error(FZ_E_HIP, "out of host memory");
        if (rc == FZ_OK && made) memcpy(ev, ctx->prof_ev, sizeof(hipEvent_t) * (size_t)made);
        for (; rc == FZ_OK && made < 2 * max_launches; ++made)
            if ((rc = fz_check_hip(hipEventCreate(&ev[made]), "event create")) != FZ_OK) break;
        if (rc != FZ_OK) {
            for (int i = 2 * ctx->prof_cap; ev && i < made; ++i) (void)hipEventDestroy(ev[i]);
            free(ev);
            free(kind);
            return rc;
        }
        free(ctx->prof_ev);
        free(ctx->prof_kind);
        ctx->prof_ev = ev;
        ctx->prof_kind = kind;
        ctx->prof_cap = max_launches;
    }
    ctx->prof_n = 0;
    ctx->prof_every = sample_every;
    ctx->prof_seen[0] = ctx->prof_seen[1] = 0;
    ctx->prof_on = 1;
    return FZ_OK;
}

int fz_profile_end(fz_ctx *ctx, double *fwd_avg_us, int *fwd_count, double *inv_avg_us, int *inv_count) {
    FZ_REQUIRE(ctx && fwd_avg_us && fwd_count && inv_avg_us && inv_count, "NULL argument");
    FZ_DEV(ctx);
    ctx->prof_on = 0;
    FZ_HIP(hipStreamSynchronize(ctx->stream), "profile sync");
    double sum[3] = {0, 0, 0};                  // kind 2 (multi-job launches) is reported by fz_profile_end_samples only
    int cnt[3] = {0, 0, 0};
    for (int i = 0; i < ctx->prof_n; ++i) {
        float ms = 0;
        FZ_HIP(hipEventElapsedTime(&ms, ctx->prof_ev[2 * i], ctx->prof_ev[2 * i + 1]), "event elapsed");
        sum[ctx->prof_kind[i]] += ms * 1e3;
        cnt[ctx->prof_kind[i]]++;
    }
    *fwd_avg_us = cnt[0] ? sum[0] / cnt[0] : 0.0;
    *inv_avg_us = cnt[1] ? sum[1] / cnt[1] : 0.0;
    *fwd_count = cnt[0];
    *inv_count = cnt[1];
    ctx->prof_n = 0;
    return FZ_OK;
}

int fz_profile_end_samples(fz_ctx *ctx, double *us, int *kind, int cap, int *n) {
    FZ_REQUIRE(ctx && us && kind && n && cap >= 0, "bad argument");
    FZ_DEV(ctx);
    ctx->prof_on = 0;
    FZ_HIP(hipStreamSynchronize(ctx->stream), "profile sync");
    int k = 0;
    for (int i = 0; i < ctx->prof_n && k < cap; ++i, ++k) {
        float ms = 0;
        FZ_HIP(hipEventElapsedTime(&ms, ctx->prof_ev[2 * i], ctx->prof_ev[2 * i + 1]), "event elapsed");
        us[k] = ms * 1e3;
        kind[k] = ctx->prof_kind[i];
    }
    *n = k;
    ctx->prof_n = 0;
    return FZ_OK;
}

int fz_runtime_info(fz_ctx *ctx, int *out_build, int *out_runtime, char *out_arch, size_t arch_cap) {
    FZ_REQUIRE(ctx, "ctx is NULL");
    if (out_build) *out_build = HIP_VERSION;
    if (out_runtime) {
        int v = 0;
        FZ_HIP(hipRuntimeGetVersion(&v), "hipRuntimeGetVersion");
        *out_runtime = v;
    }
    if (out_arch && arch_cap) {
        hipDeviceProp_t prop;
        FZ_HIP(hipGetDeviceProperties(&prop, ctx->device), "hipGetDeviceProperties");
        snprintf(out_arch, arch_cap, "%s", prop.gcnArchName);
    }
    return FZ_OK;
}

// ---- launch-floor diagnostics ------------------------------------------------------------------------------
int fz_diag_empty_launch(fz_ctx *ctx) {
    FZ_REQUIRE(ctx, "ctx is NULL");
    FZ_DEV(ctx);
    return fz_launch_diag(ctx, 0, nullptr, nullptr, 0);
}

int fz_diag_copy(fz_ctx *ctx, const void *d_src, void *d_dst, size_t bytes) {
    FZ_REQUIRE(ctx && (bytes == 0 || (d_src && d_dst)), "NULL argument");
    FZ_REQUIRE((((uintptr_t)d_src | (uintptr_t)d_dst) & 15) == 0 && bytes % 16 == 0, "16-byte aligned buffers and size");
    FZ_DEV(ctx);
    return fz_launch_diag(ctx, 1, d_src, d_dst, bytes);
}

int fz_diag_ntt_schedule(fz_ctx *ctx, size_t rows, int *family) {
    FZ_REQUIRE(ctx && family, "NULL argument");
    *family = 0;
    if (ctx->logd < 5 || ctx->logd > 8) return FZ_OK;
    const bool radix4_exists = ctx->logd == 6 || ctx->logd == 8;           // (degrees 32 and 128 only have the 16-per-lane kernels)
    if (!radix4_exists || ctx->force_kernel == 16) *family = 16;
    else if (ctx->force_kernel == 4) *family = 4;
    else *family = rows >= (size_t)ctx->small_batch_rows ? 16 : 4;
    return FZ_OK;
}

int fz_diag_multi_order(const fz_ntt_job *h_jobs, size_t n_jobs, const fz_ntt_job *h_prev, size_t n_prev, int degree,
                        unsigned resident_workgroups, int ordered, int *h_order, uint32_t *h_end, int *out_consumers, int *out_keep) {
    FZ_REQUIRE((n_jobs == 0 || (h_jobs && h_order && h_end)) && (n_prev == 0 || h_prev), "NULL argument");
    FZ_REQUIRE(n_jobs <= (size_t)kFzMultiMax && n_prev <= (size_t)kFzMultiMax, "at most %d jobs per launch", kFzMultiMax);
    FZ_REQUIRE(degree >= 32 && degree <= 256 && (degree & (degree - 1)) == 0 && resident_workgroups >= 1, "degree 32 .. 256, at least one workgroup");
    FzMultiJobs J;
    memset(&J, 0, sizeof(J));
    FzProduced prev[kFzMultiMax];
    for (size_t j = 0; j < n_jobs; ++j) {
        FZ_REQUIRE(h_jobs[j].rows > 0 && h_jobs[j].rows < ((size_t)1 << 31), "job %zu: rows", j);
        J.in[j] = h_jobs[j].d_in; J.out[j] = h_jobs[j].d_out;
        J.rows[j] = (unsigned)h_jobs[j].rows | (h_jobs[j].inverse ? 0x80000000u : 0u);
    }
    J.n = (int)n_jobs;
    for (size_t k = 0; k < n_prev; ++k) prev[k] = FzProduced{h_prev[k].d_out, (unsigned)h_prev[k].rows};
    int consumers = 0, keep = 0;
    (void)fz_multi_plan(J, degree, prev, (int)n_prev, ordered != 0, resident_workgroups, h_order, h_end, &consumers, &keep);
    if (out_consumers) *out_consumers = consumers;
    if (out_keep) *out_keep = keep;
    return FZ_OK;
}

int fz_diag_multi_last(fz_ctx *ctx, int *h_order, size_t cap, size_t *n, int *out_consumers, int *out_keep) {
    FZ_REQUIRE(ctx && n && (cap == 0 || h_order), "NULL argument");
    *n = (size_t)ctx->last_n;
    for (size_t k = 0; k < cap && k < (size_t)ctx->last_n; ++k) h_order[k] = ctx->last_order[k];
    if (out_consumers) *out_consumers = ctx->last_consumers;
    if (out_keep) *out_keep = ctx->last_keep;
    return FZ_OK;
}

int fz_diag_shader_clock(fz_ctx *ctx, unsigned microseconds, double *out_mhz) {
    FZ_REQUIRE(ctx && out_mhz, "NULL argument");
    FZ_REQUIRE(microseconds >= 1 && microseconds <= 1000000, "between 1 us and 1 s");
    FZ_DEV(ctx);
    // its own stream: the probe runs BESIDE whatever the caller queued on the context's stream (that is the point).  Stream
    // and result word live as long as the context: hipMalloc / hipFree here would synchronise the device with that work.
    if (!ctx->diag_stream) FZ_HIP(hipStreamCreateWithFlags(&ctx->diag_stream, hipStreamNonBlocking), "diag stream");
    if (!ctx->d_diag) FZ_HIP(hipMalloc((void **)&ctx->d_diag, 2 * sizeof(unsigned long long)), "diag alloc");
    unsigned long long h[2] = {0, 0};
    FZ_TRY(fz_launch_diag_clock(ctx->diag_stream, (unsigned long long)microseconds * 100ull, ctx->d_diag));
    FZ_HIP(hipMemcpyAsync(h, ctx->d_diag, sizeof(h), hipMemcpyDeviceToHost, ctx->diag_stream), "diag read");
    FZ_HIP(hipStreamSynchronize(ctx->diag_stream), "diag sync");
    *out_mhz = h[1] ? 100.0 * (double)h[0] / (double)h[1] : 0.0;
    return FZ_OK;
}

int fz_diag_delay(fz_ctx *ctx, unsigned microseconds) {
    FZ_REQUIRE(ctx, "ctx is NULL");
    FZ_REQUIRE(microseconds >= 1 && microseconds <= 100000, "between 1 us and 100 ms");
    FZ_DEV(ctx);
    return fz_launch_diag_clock(ctx->stream, (unsigned long long)microseconds * 100ull, nullptr);
}

// ---- device-side launch timestamps of the multi-job transform (diagnostics: include/fusion_hip_diag.h) -----------------
// rocprofv3 --kernel-trace serialises the dispatches of all streams, and HIP events are host-visible markers between
// dispatches: neither shows WHEN launches of different streams ran relative to each other.  While stamps are on, every
// workgroup of every fz_ntt_multi launch of this context stores the 100 MHz reference counter (s_memrealtime: one counter
// for the whole chip) at entry and -- after its stores have been acknowledged -- at exit; launch k of the recording is the
// interval [min entry, max exit] over its workgroups.  Slots are assigned when a launch is ISSUED (or captured: the slot is
// part of the recorded kernel arguments), so a captured graph is replayed ONCE between fz_diag_stamps_reset and
// fz_diag_stamps_read.
int fz_diag_stamps_begin(fz_ctx *ctx, size_t max_launches, size_t max_workgroups) {
    FZ_REQUIRE(ctx && max_launches >= 1 && max_launches <= (1u << 20) && max_workgroups >= 1 && max_workgroups <= ((size_t)1 << 26), "bad argument");
    FZ_DEV(ctx);
    if (fz_capturing(ctx)) return fz_set_error(FZ_E_BADARG, "stamps cannot be set up during graph capture");
    // a recording that is still on is switched OFF and taken apart first: if anything below fails, no recording is left
    // half-built and no launch takes a slot in a buffer that is gone
    ctx->stamp_on = 0;
    ctx->stamp_n = 0;
    ctx->stamp_used = 0;
    ctx->stamp_launch_cap = 0;
    ctx->stamp_wg_cap = 0;
    free(ctx->stamp_first); free(ctx->stamp_count);
    ctx->stamp_first = nullptr; ctx->stamp_count = nullptr;
    size_t *first = (size_t *)malloc(sizeof(size_t) * max_launches);
    unsigned *count = (unsigned *)malloc(sizeof(unsigned) * max_launches);
    int rc = first && count ? FZ_OK : fz_set_error(FZ_E_HIP, "out of host memory");
    if (rc == FZ_OK) rc = fz_area_replace(ctx, FZ_A_STAMP, 16 * max_workgroups);
    if (rc == FZ_OK) rc = fz_check_hip(hipMemsetAsync(ctx->area[FZ_A_STAMP].p, 0, 16 * max_workgroups, ctx->stream), "stamp reset");
    if (rc != FZ_OK) { free(first); free(count); return rc; }
    ctx->stamp_first = first;
    ctx->stamp_count = count;
    ctx->stamp_launch_cap = (int)max_launches;
    ctx->stamp_wg_cap = max_workgroups;
    ctx->stamp_on = 1;
    return FZ_OK;
}

// stop assigning slots (launches issued from now on carry no stamps); the recording stays readable
int fz_diag_stamps_stop(fz_ctx *ctx) {
    FZ_REQUIRE(ctx, "ctx is NULL");
    ctx->stamp_on = 0;
    return FZ_OK;
}

// zero every slot (asynchronous on the context's stream): before the ONE replay of a captured recording that is to be read
int fz_diag_stamps_reset(fz_ctx *ctx) {
    FZ_REQUIRE(ctx && ctx->area[FZ_A_STAMP].p, "no stamp buffer");
    FZ_DEV(ctx);
    FZ_HIP(hipMemsetAsync(ctx->area[FZ_A_STAMP].p, 0, 16 * ctx->stamp_used, ctx->stream), "stamp reset");
    return FZ_OK;
}

// synchronises the context's stream; per recorded launch k < *n: h_start[k] / h_end[k] = min entry / max exit over its
// workgroups (ticks of the 100 MHz counter; 0 / 0 when no workgroup of the launch has run since the reset), h_workgroups[k]
// (optional) = how many of its workgroups stamped, h_last_start[k] (optional) = the latest entry (when the dispatcher had
// handed out the launch's last workgroup)
int fz_diag_stamps_read(fz_ctx *ctx, uint64_t *h_start, uint64_t *h_end, uint64_t *h_last_start, uint32_t *h_workgroups, size_t cap, size_t *n) {
    FZ_REQUIRE(ctx && h_start && h_end && n, "NULL argument");
    FZ_REQUIRE(ctx->area[FZ_A_STAMP].p, "no stamp buffer");
    FZ_DEV(ctx);
    if (fz_capturing(ctx)) return fz_set_error(FZ_E_BADARG, "stamps cannot be read during graph capture");
    FZ_HIP(hipStreamSynchronize(ctx->stream), "stamp sync");
    unsigned long long *h = (unsigned long long *)malloc(16 * (ctx->stamp_used ? ctx->stamp_used : 1));      // (no C++ exception crosses the C ABI)
    if (!h) return fz_set_error(FZ_E_HIP, "out of host memory");
    if (ctx->stamp_used) {
        const int rc = fz_check_hip(hipMemcpy(h, ctx->area[FZ_A_STAMP].p, 16 * ctx->stamp_used, hipMemcpyDeviceToHost), "stamp read");
        if (rc != FZ_OK) { free(h); return rc; }
    }
    size_t k = 0;
    for (; k < (size_t)ctx->stamp_n && k < cap; ++k) {
        unsigned long long lo = ~0ull, hi = 0, last = 0;
        unsigned seen = 0;
        for (size_t w = ctx->stamp_first[k]; w < ctx->stamp_first[k] + ctx->stamp_count[k]; ++w) {
            const unsigned long long a = h[2 * w], b = h[2 * w + 1];
            if (!a && !b) continue;
            ++seen;
            lo = std::min(lo, a); hi = std::max(hi, b); last = std::max(last, a);
        }
        h_start[k] = seen ? lo : 0;
        h_end[k] = hi;
        if (h_last_start) h_last_start[k] = last;
        if (h_workgroups) h_workgroups[k] = seen;
    }
    *n = k;
    free(h);
    return FZ_OK;
}

}  // extern "C"
