// fz_hash_ag_capi.hip -- the entry of the C ABI (include/fusion_hip.h) behind hash_ag for many committees on the device: its rules,
// the pinned staging of the order list and the group table, and the launch sequence.  The kernel: fz_hash_ag.hip.  No kernel here.
#include "fz_capi_rules.h"
#include "fz_staged_rules.h"

#include <cstring>
#include <algorithm>
#include <numeric>
#include <vector>

// What the wave-per-committee kernel takes (fz_hash_ag.hip); *why (optional): the message of the refusal.  44 bytes: what the
// decoder's chunk words hold at any alignment (kChunkWords of fz_challenge_decode_dev.h).
bool fz_hash_ag_wave_ok(const fz_scheme_params *P, const char **why) {
    const char *w = nullptr;
    const long long bound = std::max<long long>(1, std::min<long long>((long long)P->modulus / 2, P->beta_ag));
    int sb = 0, cb = 0, ib = 0;
    const size_t n = fz_host_agg_section_bytes(P, &sb, &cb, &ib);
    const long long pos0 = (long long)sb + (long long)cb * P->omega_ag;
    if (bound != 1) w = "device hash_ag: ternary aggregation coefficients (norm bound 1) only; use fz_aggregation_coefficients (host)";
    else if (P->degree > 256 || P->degree < 4 || (P->degree & (P->degree - 1)))
        w = "device hash_ag: degree 4..256, a power of two, only; use fz_aggregation_coefficients (host)";
    else if (P->omega_ag > 64 || P->omega_ag > P->degree || ib > 44)
        w = "device hash_ag: weight <= min(64, degree) and index chunks of at most 44 bytes only; use fz_aggregation_coefficients (host)";
    else if ((long long)n < pos0 || ((long long)n - pos0) % ib)
        w = "device hash_ag: a section that cuts an index chunk; use fz_aggregation_coefficients (host)";
    else if (!fz_challenge_wave_ok(P))
        w = "device hash_ag: outside the wave form of the challenge pipeline; use fz_aggregation_coefficients (host)";
    if (why) *why = w;
    return w == nullptr;
}

extern "C" {

int fz_hash_ag_ragged_dev(fz_ctx *ctx, const fz_scheme_params *P, const int32_t *d_vk, const uint8_t *d_pre, const int32_t *d_c_hat,
                          size_t N, const uint32_t *h_order, const size_t *h_off, size_t G, int32_t *d_alpha_hat) {
    FZ_REQUIRE(ctx && P, "NULL argument");
    FZ_REQUIRE(N == 0 || (d_vk && d_pre && d_c_hat && d_alpha_hat), "NULL argument");
    FZ_REQUIRE(G == 0 || h_off, "NULL argument");
    const size_t M = G ? h_off[G] : 0;
    FZ_REQUIRE(M == 0 || h_order, "NULL argument");
    FZ_DEV(ctx);
    if (!fz_host_params_ok(P)) return fz_set_error(FZ_E_BADARG, "bad scheme parameters");
    if (P->degree != ctx->degree || P->modulus != (int64_t)ctx->q)
        return fz_set_error(FZ_E_BADARG, "scheme parameters (degree %d) do not belong to this context (degree %d)", P->degree, ctx->degree);
    FZ_REQUIRE(!(((uintptr_t)d_vk | (uintptr_t)d_c_hat | (uintptr_t)d_alpha_hat) & 15) && !((uintptr_t)d_pre & 3), "misaligned device pointer");
    if (fz_capturing(ctx)) return fz_set_error(FZ_E_BADARG, "the device hash_ag stages its order list: not during graph capture");
    FZ_REQUIRE(N < ((size_t)1 << 31) && G < ((size_t)1 << 31), "N = %zu, G = %zu: fewer than 2^31 each", N, G);
    // ---- the groups: offsets from 0, never decreasing, no empty group, at most N entries; every entry a row, none twice ----
    if (G) {
        FZ_REQUIRE(h_off[0] == 0, "offsets must start at 0 (got %zu)", h_off[0]);
        for (size_t g = 0; g < G; ++g) {
            FZ_REQUIRE(h_off[g] <= h_off[g + 1], "offsets must not decrease (group %zu)", g);
            FZ_REQUIRE(h_off[g] < h_off[g + 1], "group %zu is empty", g);
        }
        FZ_REQUIRE(M <= N, "%zu order entries for %zu rows", M, N);
        std::vector<bool> seen(N, false);
        for (size_t i = 0; i < M; ++i) {
            FZ_REQUIRE(h_order[i] < N, "order entry %zu names row %u of %zu", i, h_order[i], N);
            FZ_REQUIRE(!seen[h_order[i]], "order entry %zu names row %u a second time", i, h_order[i]);
            seen[h_order[i]] = true;
        }
    }
    const char *why = nullptr;
    if (!fz_hash_ag_wave_ok(P, &why)) return fz_set_error(FZ_E_UNSUPPORTED, "%s", why);
    FZ_TRY(needs_transforms(ctx));
    if (N == 0) return FZ_OK;
    const int d = P->degree;
    if (M == 0) return fz_check_hip(hipMemsetAsync(d_alpha_hat, 0, N * (size_t)d * 4, ctx->stream), "alpha clear");
    int ib = 0;
    (void)fz_host_agg_section_bytes(P, nullptr, nullptr, &ib);
    const uint32_t *d_tab = nullptr;
    FZ_TRY(challenge_table_fit(ctx, ib, d, &d_tab));          // (the challenge decoder's: index bytes depend on degree and secpar alone)
    // The group table: (first entry of the order list, signers) per committee, LONGEST FIRST -- a committee is one serial chain of
    // ~100 permutations per signer, and a long one handed out last would be the tail of the launch (FZ_HASH_AG_ORDER=0: the
    // caller's order, for A/B runs).  Pinned staging: the kernel reads table and order list in place, nothing is uploaded.
    std::vector<uint32_t> by(G);
    std::iota(by.begin(), by.end(), 0u);
    if (ctx->knob_hash_ag_order)
        std::stable_sort(by.begin(), by.end(), [&](uint32_t a, uint32_t b) { return h_off[a + 1] - h_off[a] > h_off[b + 1] - h_off[b]; });
    const size_t o_grp = 0, o_ord = (G * 8 + 15) & ~(size_t)15;
    fz_ctx::FzStage *st = nullptr;
    FZ_TRY(stage_take(ctx, o_ord + M * 4 + 64, &st));
    uint32_t *grp = reinterpret_cast<uint32_t *>(st->h + o_grp);
    for (size_t k = 0; k < G; ++k) {
        grp[2 * k] = (uint32_t)h_off[by[k]];
        grp[2 * k + 1] = (uint32_t)(h_off[by[k] + 1] - h_off[by[k]]);
    }
    memcpy(st->h + o_ord, h_order, M * 4);
    int rc = fz_check_hip(hipMemsetAsync(d_alpha_hat, 0, N * (size_t)d * 4, ctx->stream), "alpha clear");
    if (rc == FZ_OK)
        rc = fz_launch_hash_ag(ctx, P, d_vk, d_pre, d_c_hat, reinterpret_cast<const uint32_t *>(st->h + o_ord), st->h + o_grp, G, d_tab, d_alpha_hat);
    if (rc == FZ_OK) rc = fz_launch_ntt(ctx, d_alpha_hat, d_alpha_hat, N, false);
    return stage_release(ctx, st, rc);
}

}  // extern "C"
