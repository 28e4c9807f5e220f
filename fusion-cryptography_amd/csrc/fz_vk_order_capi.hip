// fz_vk_order_capi.hip -- the entries of the C ABI (include/fusion_hip.h) behind the device key sort of hash_ag for many committees:
// their rules, the pinned staging of the group tables and the mask, and the launch sequences; with them the challenge entry that
// leaves the digests on the device for these entries (its rules and forms: challenge_dev, fz_staged_capi.hip).  The kernels: fz_vk_order.hip (the
// sort) and fz_hash_ag.hip (the hash, through fz_launch_hash_ag as fz_hash_ag_capi.hip launches it).  No kernel here.
#include "fz_capi_rules.h"
#include "fz_staged_rules.h"

#include <cstring>
#include <algorithm>
#include <numeric>
#include <vector>

namespace {

// what both entries are handed, and their shared rules in fz_hash_ag_ragged_dev's order (the caller has checked its own pointers)
struct OrdCall {
    fz_ctx *ctx; const fz_scheme_params *P; const int32_t *d_vk; size_t N; const size_t *h_off; size_t G; const uint8_t *h_valid;
};

int order_rules(const OrdCall &c, uintptr_t aligned16, uintptr_t aligned4, bool whole, bool no_empty) {
    fz_ctx *ctx = c.ctx;
    const fz_scheme_params *P = c.P;
    FZ_DEV(ctx);
    if (!fz_host_params_ok(P)) return fz_set_error(FZ_E_BADARG, "bad scheme parameters");
    if (P->degree != ctx->degree || P->modulus != (int64_t)ctx->q)
        return fz_set_error(FZ_E_BADARG, "scheme parameters (degree %d) do not belong to this context (degree %d)", P->degree, ctx->degree);
    FZ_REQUIRE(!(aligned16 & 15) && !(aligned4 & 3), "misaligned device pointer");
    if (fz_capturing(ctx)) return fz_set_error(FZ_E_BADARG, "the device key sort stages its group table: not during graph capture");
    FZ_REQUIRE(c.N < ((size_t)1 << 31) && c.G < ((size_t)1 << 31), "N = %zu, G = %zu: fewer than 2^31 each", c.N, c.G);
    if (c.G) {
        FZ_REQUIRE(c.h_off[0] == 0, "offsets must start at 0 (got %zu)", c.h_off[0]);
        for (size_t g = 0; g < c.G; ++g) {
            FZ_REQUIRE(c.h_off[g] <= c.h_off[g + 1], "offsets must not decrease (group %zu)", g);
            FZ_REQUIRE(!no_empty || c.h_off[g] < c.h_off[g + 1], "group %zu is empty", g);
        }
        if (whole) FZ_REQUIRE(c.h_off[c.G] == c.N, "offsets end at %zu for %zu rows", c.h_off[c.G], c.N);
        else FZ_REQUIRE(c.h_off[c.G] <= c.N, "offsets end at %zu for %zu rows", c.h_off[c.G], c.N);
    }
    return FZ_OK;
}

// The sort's staging: the groups with a valid row as (first row, rows, first entry of the order list, 0), the order list
// compacted group after group; then the mask.  counts[k] = valid rows of the k-th group KEPT, *M their sum.
struct OrdLayout { size_t o_grp, o_valid, end; };
OrdLayout order_layout(const OrdCall &c, size_t at) {
    OrdLayout L;
    L.o_grp = at;
    L.o_valid = at + c.G * 16;
    L.end = L.o_valid + (((c.h_valid ? c.h_off[c.G] : 0) + 15) & ~(size_t)15);
    return L;
}
size_t order_fill(const OrdCall &c, const OrdLayout &L, uint8_t *h, std::vector<uint32_t> *counts, size_t *M) {
    uint32_t *grp = reinterpret_cast<uint32_t *>(h + L.o_grp);
    size_t kept = 0, m = 0;
    for (size_t g = 0; g < c.G; ++g) {
        const size_t a = c.h_off[g], b = c.h_off[g + 1];
        size_t cnt = b - a;
        if (c.h_valid) {
            cnt = 0;
            for (size_t i = a; i < b; ++i) {
                const uint8_t v = c.h_valid[i] ? 1 : 0;
                h[L.o_valid + i] = v;
                cnt += v;
            }
        }
        if (!cnt) continue;
        grp[4 * kept] = (uint32_t)a;
        grp[4 * kept + 1] = (uint32_t)(b - a);
        grp[4 * kept + 2] = (uint32_t)m;
        grp[4 * kept + 3] = 0;
        if (counts) counts->push_back((uint32_t)cnt);
        m += cnt;
        ++kept;
    }
    *M = m;
    return kept;
}

bool order_degree_ok(int d) { return d >= 4 && d <= 256 && !(d & (d - 1)); }

}  // namespace

extern "C" {

int fz_sort_by_vk_string_ragged_dev(fz_ctx *ctx, const fz_scheme_params *P, const int32_t *d_vk, size_t N, const size_t *h_off, size_t G,
                                    const uint8_t *h_valid, uint32_t *d_order) {
    FZ_REQUIRE(ctx && P, "NULL argument");
    FZ_REQUIRE(N == 0 || (d_vk && d_order), "NULL argument");
    FZ_REQUIRE(G == 0 || h_off, "NULL argument");
    const OrdCall c{ctx, P, d_vk, N, h_off, G, h_valid};
    FZ_TRY(order_rules(c, (uintptr_t)d_vk, (uintptr_t)d_order, true, false));
    if (!order_degree_ok(P->degree))
        return fz_set_error(FZ_E_UNSUPPORTED, "device key sort: degree 4..256, a power of two, only; use fz_sort_by_vk_string_ragged (host)");
    if (N == 0 || G == 0) return FZ_OK;
    const OrdLayout L = order_layout(c, 0);
    fz_ctx::FzStage *st = nullptr;
    FZ_TRY(stage_take(ctx, L.end + 64, &st));
    size_t M = 0;
    const size_t kept = order_fill(c, L, st->h, nullptr, &M);
    return stage_release(ctx, st, fz_launch_vk_order(ctx, d_vk, P->degree, st->h + L.o_grp, kept, h_valid ? st->h + L.o_valid : nullptr, d_order));
}

int fz_hash_ag_ragged_sorted_dev(fz_ctx *ctx, const fz_scheme_params *P, const int32_t *d_vk, const uint8_t *d_pre, const int32_t *d_c_hat,
                                 size_t N, const size_t *h_off, size_t G, const uint8_t *h_valid, int32_t *d_alpha_hat) {
    FZ_REQUIRE(ctx && P, "NULL argument");
    FZ_REQUIRE(N == 0 || (d_vk && d_pre && d_c_hat && d_alpha_hat), "NULL argument");
    FZ_REQUIRE(G == 0 || h_off, "NULL argument");
    const OrdCall c{ctx, P, d_vk, N, h_off, G, h_valid};
    FZ_TRY(order_rules(c, (uintptr_t)d_vk | (uintptr_t)d_c_hat | (uintptr_t)d_alpha_hat, (uintptr_t)d_pre, false, true));
    const char *why = nullptr;
    if (!fz_hash_ag_wave_ok(P, &why)) return fz_set_error(FZ_E_UNSUPPORTED, "%s", why);
    FZ_TRY(needs_transforms(ctx));
    if (N == 0) return FZ_OK;
    const int d = P->degree;
    size_t most = 0;                                             // (an upper bound of the order list: the mask is counted while it is staged)
    if (G) most = h_off[G];
    if (most == 0) return fz_check_hip(hipMemsetAsync(d_alpha_hat, 0, N * (size_t)d * 4, ctx->stream), "alpha clear");
    int ib = 0;
    (void)fz_host_agg_section_bytes(P, nullptr, nullptr, &ib);
    const uint32_t *d_tab = nullptr;
    FZ_TRY(challenge_table_fit(ctx, ib, d, &d_tab));
    void *d_ord = nullptr;                                       // the order list: context-owned scratch, written and read on the stream
    FZ_TRY(fz_scratch(ctx, most * 4 + 256, &d_ord));
    // one staging slot for both kernels: the hash kernel's group table (first entry of the order list, signers), LONGEST FIRST as
    // fz_hash_ag_ragged_dev hands it out, then the sort's table and the mask
    const size_t o_hgrp = 0;
    const OrdLayout L = order_layout(c, (G * 8 + 15) & ~(size_t)15);
    fz_ctx::FzStage *st = nullptr;
    FZ_TRY(stage_take(ctx, L.end + 64, &st));
    std::vector<uint32_t> counts;
    counts.reserve(G);
    size_t M = 0;
    const size_t kept = order_fill(c, L, st->h, &counts, &M);
    const uint32_t *sgrp = reinterpret_cast<const uint32_t *>(st->h + L.o_grp);
    std::vector<uint32_t> by(kept);
    std::iota(by.begin(), by.end(), 0u);
    if (ctx->knob_hash_ag_order)
        std::stable_sort(by.begin(), by.end(), [&](uint32_t a, uint32_t b) { return counts[a] > counts[b]; });
    uint32_t *hgrp = reinterpret_cast<uint32_t *>(st->h + o_hgrp);
    for (size_t k = 0; k < kept; ++k) {
        hgrp[2 * k] = sgrp[4 * by[k] + 2];
        hgrp[2 * k + 1] = counts[by[k]];
    }
    int rc = fz_check_hip(hipMemsetAsync(d_alpha_hat, 0, N * (size_t)d * 4, ctx->stream), "alpha clear");
    if (rc == FZ_OK && kept) rc = fz_launch_vk_order(ctx, d_vk, d, st->h + L.o_grp, kept, h_valid ? st->h + L.o_valid : nullptr, (uint32_t *)d_ord);
    if (rc == FZ_OK && kept) rc = fz_launch_hash_ag(ctx, P, d_vk, d_pre, d_c_hat, (const uint32_t *)d_ord, st->h + o_hgrp, kept, d_tab, d_alpha_hat);
    if (rc == FZ_OK && kept) rc = fz_launch_ntt(ctx, d_alpha_hat, d_alpha_hat, N, false);      // (no valid signer at all: N zero rows)
    return stage_release(ctx, st, rc);
}

int fz_challenge_hat_msgs_keep_dev(fz_ctx *ctx, const fz_scheme_params *P, const int32_t *d_vk, const char *h_msgs, const size_t *h_msg_off,
                                   size_t N, int32_t *d_c_hat, uint8_t *d_prehash_out) {
    FZ_REQUIRE((h_msg_off && d_prehash_out) || N == 0, "NULL argument");
    FZ_REQUIRE(!((uintptr_t)d_prehash_out & 15), "misaligned device pointer");
    return challenge_msgs_keep_dev(ctx, P, d_vk, h_msgs, h_msg_off, N, d_c_hat, d_prehash_out);
}

int fz_vk_halves_async(fz_ctx *ctx, const int32_t *d_vk, size_t N, int32_t *d_left, int32_t *d_right) {
    FZ_ENTER(ctx, N == 0 || (d_vk && d_left && d_right), "NULL argument");
    FZ_REQUIRE(!(((uintptr_t)d_vk | (uintptr_t)d_left | (uintptr_t)d_right) & 15), "misaligned device pointer");
    if (ctx->degree < 4 || (ctx->degree & (ctx->degree - 1)))
        return fz_set_error(FZ_E_UNSUPPORTED, "key halves: a power-of-two degree of at least 4 only");
    return fz_launch_vk_halves(ctx, d_vk, N, ctx->degree, d_left, d_right);
}

}  // extern "C"
