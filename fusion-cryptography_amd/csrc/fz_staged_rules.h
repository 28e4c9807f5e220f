// fz_staged_rules.h -- what the host units that take small host inputs through the context's pinned staging slots share
// (fz_staged_capi.hip, fz_hash_ag_capi.hip, fz_vk_order_capi.hip), written once: the slots' protocol and the challenge decoder's cached weight table.
// Host code only; everything is private to the unit that includes it.
#ifndef FZ_STAGED_RULES_H
#define FZ_STAGED_RULES_H

#include "fz_internal.h"

#include <algorithm>
#include <vector>

// ---- the pinned staging slots (fz_internal.h), shared by the challenge pipeline's wave form, the sampler and the device hash_ag ---
// The protocol: stage_take, fill the slot, the launches that read it, stage_release with what they returned.
// stage_take: the next slot, at least `bytes` long and no longer read by any launch
static int stage_take(fz_ctx *ctx, size_t bytes, fz_ctx::FzStage **out) {
    fz_ctx::FzStage &st = ctx->chal_stage[ctx->chal_stage_next];
    ctx->chal_stage_next ^= 1;
    if (!st.ev) FZ_HIP(hipEventCreateWithFlags(&st.ev, hipEventDisableTiming), "staging event");
    if (st.busy) { FZ_HIP(hipEventSynchronize(st.ev), "staging slot still in use"); st.busy = 0; }
    if (st.bytes < bytes) {
        if (st.h) { FZ_HIP(hipHostFree(st.h), "staging free"); st.h = nullptr; st.bytes = 0; }
        const size_t want = std::max<size_t>((bytes + 65535) & ~(size_t)65535, 256 << 10);
        FZ_HIP(hipHostMalloc((void **)&st.h, want, hipHostMallocDefault), "staging alloc");
        st.bytes = want;
    }
    *out = &st;
    return FZ_OK;
}
// stage_release: the slot's event is recorded and the slot marked in use BEFORE the launches' code `rc` is looked at (a sequence that
// failed half-way may have queued a reader); -> rc, or the record's own error
static int stage_release(fz_ctx *ctx, fz_ctx::FzStage *st, int rc) {
    FZ_HIP(hipEventRecord(st->ev, ctx->stream), "staging event record");
    st->busy = 1;
    return rc;
}

// the decoder's weight table, cached in FZ_A_CHAL_TAB for the (index bytes, degree) it was built for
static int challenge_table_fit(fz_ctx *ctx, int ib, int degree, const uint32_t **d_tab) {
    if (!ctx->area[FZ_A_CHAL_TAB].p || ctx->chal_tab_ib != ib || ctx->chal_tab_degree != degree) {
        std::vector<uint32_t> tab((size_t)(degree + 1) * 16);
        fz_challenge_weight_table(ib, degree, tab.data());
        ctx->chal_tab_degree = 0;                            // (no table is built for degree 0: a failure below leaves none that counts)
        FZ_TRY(fz_area_replace(ctx, FZ_A_CHAL_TAB, tab.size() * 4));
        FZ_HIP(hipMemcpy(ctx->area[FZ_A_CHAL_TAB].p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice), "table upload");
        ctx->chal_tab_ib = ib;
        ctx->chal_tab_degree = degree;
    }
    *d_tab = (const uint32_t *)ctx->area[FZ_A_CHAL_TAB].p;
    return FZ_OK;
}

#endif
