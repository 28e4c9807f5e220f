// fz_staged_capi.hip -- the entries of the C ABI (include/fusion_hip.h) that take small host inputs through the pinned staging slots
// and therefore refuse graph capture: the host side of the device challenge pipeline (fz_challenge.hip) and of the device sampler
// (fz_sample.hip).  No kernel.
#include "fz_capi_rules.h"
#include "fz_staged_rules.h"      // the pinned staging slots' protocol and the decoder's cached weight table

#include <cstring>
#include <algorithm>
#include <vector>

// ---- the challenge pipeline on the device (device half) ---------------------------------------------
// the pre-hashed messages come either as h_prehash [N][32] (computed by the caller, fz_hash_messages) or are computed here,
// on the device, from the messages themselves (h_msgs back to back, h_msg_off [N + 1]); h_prehash_out (optional, with
// messages only) receives them
struct ChalCall {
    fz_ctx *ctx; const fz_scheme_params *P; const int32_t *d_vk; const uint8_t *h_prehash; const char *h_msgs; const size_t *h_msg_off;
    uint8_t *h_prehash_out; size_t N; int32_t *d_out; bool transform;         // what the entry was handed
    uint8_t *d_prehash_out;                              // ... (with messages only) the digests stay in DEVICE memory: nothing waits for them
    size_t text_stride; int out_blocks, index_bytes;     // challenge_geometry: bytes of a signer's text row, blocks of SHAKE output, the decoder's index bytes
    const uint32_t *d_tab;                               // challenge_table
};
static_assert(sizeof(size_t) == sizeof(unsigned long long), "offsets travel as 64-bit words");

static int challenge_checks(const ChalCall &c) {
    fz_ctx *ctx = c.ctx;
    const fz_scheme_params *P = c.P;
    FZ_REQUIRE(ctx && P && (c.N == 0 || (c.d_vk && (c.h_prehash || c.h_msg_off) && c.d_out)), "NULL argument");
    if (!c.h_prehash && c.N) {
        FZ_REQUIRE(c.h_msg_off[c.N] == c.h_msg_off[0] || c.h_msgs, "NULL argument");
        for (size_t i = 0; i < c.N; ++i) FZ_REQUIRE(c.h_msg_off[i] <= c.h_msg_off[i + 1], "message offsets must not decrease");
    }
    FZ_DEV(ctx);
    if (!fz_host_params_ok(P)) return fz_set_error(FZ_E_BADARG, "bad scheme parameters");
    if (P->degree != ctx->degree || P->modulus != (int64_t)ctx->q)
        return fz_set_error(FZ_E_BADARG, "scheme parameters (degree %d) do not belong to this context (degree %d)", P->degree, ctx->degree);
    if (fz_capturing(ctx)) return fz_set_error(FZ_E_BADARG, "the challenge pipeline uploads the pre-hashed messages: not during graph capture");
    const long long bound = std::max<long long>(1, std::min<long long>((long long)P->modulus / 2, P->beta_ch));
    if (bound != 1 || P->degree > 256 || P->degree < 4 || (P->degree & (P->degree - 1)) || P->omega_ch > P->degree ||
        (((uintptr_t)c.d_vk | (uintptr_t)c.d_out) & 15))
        return fz_set_error(FZ_E_UNSUPPORTED, "device challenge pipeline: ternary challenges (norm bound 1), degree 4..256 and "
                                              "16-byte aligned rows only; use fz_challenge_coefficients (host)");
    if (c.transform) FZ_TRY(needs_transforms(ctx));
    return FZ_OK;
}

static int challenge_geometry(ChalCall &c) {
    int sb = 0, cb = 0;
    const size_t needed = fz_host_challenge_needed_bytes(c.P, &sb, &cb, &c.index_bytes);
    c.out_blocks = (int)((needed + kFzShakeRate - 1) / kFzShakeRate);
    // longest possible text: fixed pieces + 2*degree values of up to 11 characters + separators + 78 digits
    char t0[384], t1[384], t2[16];
    int n0, n1, n2;
    fz_host_vk_text_parts(c.P, t0, &n0, t1, &n1, t2, &n2, 384);
    if (n0 < 0) return fz_set_error(FZ_E_UNSUPPORTED, "verification-key text pieces do not fit");
    const size_t max_len = (size_t)n0 + n1 + n2 + (size_t)2 * c.P->degree * 13 + 78;
    size_t blocks = max_len / kFzShakeRate + 1;
    blocks += blocks & 1;                                   // even: rows stay 16-byte aligned
    c.text_stride = blocks * kFzShakeRate;
    return FZ_OK;
}

static int challenge_table(ChalCall &c) { return challenge_table_fit(c.ctx, c.index_bytes, c.P->degree, &c.d_tab); }

// One launch, nothing uploaded: the kernel reads the messages (or digests) from pinned host memory and leaves the
// digests there.  The call returns without synchronising unless the caller wants the digests.
static int challenge_wave_form(const ChalCall &c) {
    fz_ctx *ctx = c.ctx;
    const size_t N = c.N, msg_bytes = c.h_prehash ? 0 : c.h_msg_off[N] - c.h_msg_off[0];
    const size_t o_pre = 0, o_off = N * 32, o_msg = o_off + (N + 1) * 8;
    const bool digests_out = !c.h_prehash && c.h_prehash_out;
    fz_ctx::FzStage *st = nullptr;
    FZ_TRY(stage_take(ctx, o_msg + msg_bytes + 64, &st));
    if (c.h_prehash) {
        memcpy(st->h + o_pre, c.h_prehash, N * 32);
    } else {
        memcpy(st->h + o_off, c.h_msg_off, (N + 1) * 8);
        if (msg_bytes) memcpy(st->h + o_msg, c.h_msgs + c.h_msg_off[0], msg_bytes);
    }
    int rc = fz_launch_challenge_wave(ctx, c.P, c.d_vk, c.h_prehash ? st->h + o_pre : nullptr, st->h + o_msg, (const unsigned long long *)(st->h + o_off),
                                      c.d_prehash_out ? c.d_prehash_out : digests_out ? st->h + o_pre : nullptr, N, c.text_stride, c.out_blocks, c.d_tab,
                                      c.d_out);
    if (rc == FZ_OK && c.transform) rc = fz_launch_ntt(ctx, c.d_out, c.d_out, N, false);
    FZ_TRY(stage_release(ctx, st, rc));
    if (digests_out) {
        FZ_HIP(hipStreamSynchronize(ctx->stream), "digest sync");
        memcpy(c.h_prehash_out, st->h + o_pre, N * 32);
    }
    return FZ_OK;
}

// The three-kernel pipeline in passes of 65536 signers = two waves of 32 signers on each of the chip's 1024 SIMDs (a second wave per
// SIMD fills the issue slots one wave alone leaves empty); bounds the scratch at ~16 KB per signer
static int challenge_chunked_form(const ChalCall &c) {
    fz_ctx *ctx = c.ctx;
    const size_t chunk = 65536;
    for (size_t base = 0; base < c.N; base += chunk) {
        const size_t n = std::min(chunk, c.N - base);
        const size_t xstride = (n + 63) & ~(size_t)63;
        const size_t msg_bytes = c.h_prehash ? 0 : c.h_msg_off[base + n] - c.h_msg_off[base];
        FzCarve s;
        const size_t o_pre = s.take(n * 32), o_nb = s.take(n * 4), o_text = s.take(n * c.text_stride);
        const size_t o_xof = s.take(((size_t)c.out_blocks * (kFzShakeRate / 4) + 1) * xstride * 4);     // + one spare word row (decoder)
        const size_t with_digests = s.next;                   // digests: the three segments below are not allocated
        const size_t o_off = s.take((n + 1) * 8);
        const size_t o_dec = s.take(n * 64);                  // [n][16] words: the integers in base 10^9
        const size_t o_msg = s.take_packed(msg_bytes);        // (64-aligned)
        FZ_TRY(s.fit(ctx, c.h_prehash ? with_digests : s.next));
        uint8_t *sp = s.at<uint8_t>(0);
        uint8_t *pre = c.d_prehash_out ? c.d_prehash_out + 32 * base : sp + o_pre;      // (the caller's digests are written where they stay)
        if (c.h_prehash) {
            FZ_HIP(hipMemcpyAsync(pre, c.h_prehash + 32 * base, n * 32, hipMemcpyHostToDevice, ctx->stream), "upload of the pre-hashed messages");
        } else {
            FZ_HIP(hipMemcpyAsync(sp + o_off, c.h_msg_off + base, (n + 1) * 8, hipMemcpyHostToDevice, ctx->stream), "upload of the message offsets");
            if (msg_bytes)
                FZ_HIP(hipMemcpyAsync(sp + o_msg, c.h_msgs + c.h_msg_off[base], msg_bytes, hipMemcpyHostToDevice, ctx->stream), "upload of the messages");
            FZ_TRY(fz_launch_prehash(ctx, c.P, sp + o_msg, (const unsigned long long *)(sp + o_off), n, pre, (uint32_t *)(sp + o_dec)));
            if (c.h_prehash_out)
                FZ_HIP(hipMemcpyAsync(c.h_prehash_out + 32 * base, pre, n * 32, hipMemcpyDeviceToHost, ctx->stream), "download of the pre-hashed messages");
        }
        FZ_HIP(hipStreamSynchronize(ctx->stream), "upload sync");      // the caller's buffers have been consumed when this returns
        FZ_TRY(fz_launch_challenge(ctx, c.P, c.d_vk + base * 2 * (size_t)c.P->degree, pre,
                                   c.h_prehash ? nullptr : (const uint32_t *)(sp + o_dec), n, sp + o_text, c.text_stride,
                                   (int *)(sp + o_nb), (uint32_t *)(sp + o_xof), xstride, c.out_blocks, c.d_tab,
                                   c.d_out + base * (size_t)c.P->degree));
    }
    if (c.transform) return fz_launch_ntt(ctx, c.d_out, c.d_out, c.N, false);
    return FZ_OK;
}

static int challenge_dev(fz_ctx *ctx, const fz_scheme_params *P, const int32_t *d_vk, const uint8_t *h_prehash, const char *h_msgs,
                         const size_t *h_msg_off, uint8_t *h_prehash_out, size_t N, int32_t *d_out, bool transform, uint8_t *d_prehash_out = nullptr) {
    ChalCall c{ctx, P, d_vk, h_prehash, h_msgs, h_msg_off, h_prehash_out, N, d_out, transform, d_prehash_out, 0, 0, 0, nullptr};
    FZ_TRY(challenge_checks(c));
    if (N == 0) return FZ_OK;
    FZ_TRY(challenge_geometry(c));
    FZ_TRY(challenge_table(c));
    // Which form.  Up to kWaveFormMax signers per call every signer gets a WAVE (fz_launch_challenge_wave: the chain of ~108
    // permutations at 24 instructions + 4 gathers per round, text and stream in LDS); beyond, the three-kernel pipeline with 32
    // or 64 signers per wave has the higher throughput (profiles/r06_challenge_pipeline.txt).
    constexpr size_t kWaveFormMax = 4608;                    // 4096 signers: 0.67 ms against 0.77; 5120: 0.85 against 0.79
    const bool wave_form = fz_challenge_wave_ok(P) && (ctx->knob_shake_full == 3 || (ctx->knob_shake_full == 0 && N <= kWaveFormMax));
    return wave_form ? challenge_wave_form(c) : challenge_chunked_form(c);
}

// fz_challenge_hat_msgs_dev with the digests left in DEVICE memory (d_prehash_out [N][32]): what fz_challenge_hat_msgs_keep_dev
// (fz_vk_order_capi.hip, with the entries that read the digests there) runs -- the one copy of the rules above serves it too
int challenge_msgs_keep_dev(fz_ctx *ctx, const fz_scheme_params *P, const int32_t *d_vk, const char *h_msgs, const size_t *h_msg_off, size_t N,
                            int32_t *d_c_hat, uint8_t *d_prehash_out) {
    return challenge_dev(ctx, P, d_vk, nullptr, h_msgs, h_msg_off, nullptr, N, d_c_hat, true, d_prehash_out);
}

extern "C" {

int fz_challenge_coefficients_dev(fz_ctx *ctx, const fz_scheme_params *P, const int32_t *d_vk, const uint8_t *h_prehash,
                                  size_t N, int32_t *d_coefs) {
    FZ_REQUIRE(h_prehash || N == 0, "NULL argument");
    return challenge_dev(ctx, P, d_vk, h_prehash, nullptr, nullptr, nullptr, N, d_coefs, false);
}

int fz_challenge_hat_dev(fz_ctx *ctx, const fz_scheme_params *P, const int32_t *d_vk, const uint8_t *h_prehash, size_t N,
                         int32_t *d_c_hat) {
    FZ_REQUIRE(h_prehash || N == 0, "NULL argument");
    return challenge_dev(ctx, P, d_vk, h_prehash, nullptr, nullptr, nullptr, N, d_c_hat, true);
}

int fz_challenge_hat_msgs_dev(fz_ctx *ctx, const fz_scheme_params *P, const int32_t *d_vk, const char *h_msgs, const size_t *h_msg_off,
                              size_t N, int32_t *d_c_hat, uint8_t *h_prehash_out) {
    FZ_REQUIRE(h_msg_off || N == 0, "NULL argument");
    return challenge_dev(ctx, P, d_vk, nullptr, h_msgs, h_msg_off, h_prehash_out, N, d_c_hat, true);
}

// ---- the reference's seeded secret-key sampler on the device (fz_sample.hip) --------------------------------------------
int fz_sample_secret_polys_dev(fz_ctx *ctx, const uint64_t *h_seeds, size_t N, int64_t modulus, int degree, int64_t norm_bound,
                               int64_t weight_bound, int32_t *d_out) {
    FZ_REQUIRE(ctx && (N == 0 || (h_seeds && d_out)), "NULL argument");
    FZ_REQUIRE(degree >= 1 && modulus >= 2, "bad degree / modulus");
    FZ_DEV(ctx);
    if (fz_capturing(ctx)) return fz_set_error(FZ_E_BADARG, "the sampler uploads the seeds: not during graph capture");
    const int64_t bound = std::max<int64_t>(0, std::min<int64_t>(modulus / 2, norm_bound));
    if (bound < 1 || bound >= (1ll << 32)) return fz_set_error(FZ_E_BADARG, "empty range for randrange()");
    // a coefficient is stored as an int32: magnitudes run up to the bound, and from 2^31 on they would wrap silently
    if (bound > INT32_MAX)
        return fz_set_error(FZ_E_UNSUPPORTED, "sampler: a norm bound above 2^31 - 1 does not fit the int32 coefficients");
    if (weight_bound < degree)
        return fz_set_error(FZ_E_UNSUPPORTED, "device sampler: weight bound = degree only (no shuffle); use fz_sample_secret_polys");
    // the right half of a key is seeded with seed + 1: at seed = 2^64 - 1 that is 2^64, a THREE-word key for CPython's
    // init_by_array, not the wrapped 0 -- outside what this entry (and the host clone) takes
    for (size_t i = 0; i < N; ++i)
        if (h_seeds[i] == UINT64_MAX)
            return fz_set_error(FZ_E_UNSUPPORTED, "seed %zu is 2^64 - 1: seed + 1 needs a wider key than this sampler takes", i);
    if (N == 0) return FZ_OK;
    if (!ctx->d_mt_init) {
        uint32_t tab[624];
        fz_mt_init_table(tab);
        FZ_HIP(hipMalloc((void **)&ctx->d_mt_init, sizeof(tab)), "sampler table alloc");
        FZ_HIP(hipMemcpy(ctx->d_mt_init, tab, sizeof(tab), hipMemcpyHostToDevice), "sampler table upload");
    }
    int kbits = 0;
    for (uint64_t t = (uint64_t)bound; t; t >>= 1) ++kbits;            // bound.bit_length()
    // Up to 4096 keys (8192 generators: a seeding wave on every other CU): two kernels -- seeding on a lane per generator,
    // everything after it on a wave per generator, the states (20 MiB at most) through scratch: 54 + 29 us per 1024 keys
    // against 190 in one kernel.  Beyond, the one lane-per-polynomial kernel already has a wave on every CU and the two
    // forms take the same time (16 384 keys: 0.47 ms one kernel, 0.56 ms in four chunks of two).
    const bool two_kernels = bound < (1ll << 31) && N <= 4096;
    const size_t state_bytes = two_kernels ? N * 2 * 624 * sizeof(uint32_t) : 0;
    void *scr = nullptr;
    FZ_TRY(fz_scratch(ctx, state_bytes + 256, &scr));
    uint32_t *d_state = two_kernels ? (uint32_t *)scr : nullptr;
    // the seeds and the "ran out of output" flag live in the pinned staging slot the challenge pipeline uses: the kernels read the
    // seeds in place and store the flag there, so the call is two launches and one synchronisation -- no memset, no pageable upload,
    // no download (0.098 -> 0.078 ms per 1024 keys: most of what was left beside the two kernels' 57 us)
    fz_ctx::FzStage *st = nullptr;
    FZ_TRY(stage_take(ctx, 64 + N * 8, &st));
    volatile int *h_fail = reinterpret_cast<volatile int *>(st->h);
    *h_fail = 0;
    memcpy(st->h + 64, h_seeds, N * 8);
    FZ_TRY(stage_release(ctx, st, fz_launch_mt_sample(ctx, reinterpret_cast<const unsigned long long *>(st->h + 64), N, degree, (uint32_t)bound, kbits,
                                                      ctx->d_mt_init, d_out, reinterpret_cast<int *>(st->h), d_state)));
    FZ_HIP(hipStreamSynchronize(ctx->stream), "sampler sync");
    const int fail = *h_fail;
    if (fail) return fz_set_error(FZ_E_UNSUPPORTED, "device sampler ran out of generator output for a seed; use fz_sample_secret_polys");
    return FZ_OK;
}

}  // extern "C"
