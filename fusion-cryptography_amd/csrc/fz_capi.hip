// fz_capi.hip -- the C ABI of libfusion_hip.so (include/fusion_hip.h): the thin wrappers that check arguments and enqueue the
// transform, pointwise and scheme kernels on int32 rows.  (The challenge pipeline's and the sampler's entries: fz_staged_capi.hip; the
// compact-bytes entries: fz_records_capi.hip.)
#include "fz_capi_rules.h"
#include "../../include/fusion_hip_diag.h"

#include <cassert>
#include <cstring>
#include <algorithm>

// ---- the rules the entries share, each written once (an entry keeps its own order of checks and its own wording) -----------------
// (FZ_ENTER and needs_transforms, which fz_staged_capi.hip shares: fz_capi_rules.h)
// degree 64 or 256: the degrees of the fused kernels
static bool fused_degree(const fz_ctx *ctx) { return ctx->logd == 6 || ctx->logd == 8; }
static int needs_fused(const fz_ctx *ctx, const char *what) {
    return fused_degree(ctx) ? FZ_OK : fz_set_error(FZ_E_UNSUPPORTED, "%s needs the fused kernel (degree 64 or 256)", what);
}
// the reference's __neg__ is -(x mod q) in [-(q-1), 0] (polynomials.py:155-163): the one value of the path that is NOT centred,
// and for q >= 2^31 not an int32 either.  fz_pw_sub from a zero row gives the centred negation for every modulus.
static int negation_fits(const fz_ctx *ctx) {
    return ctx->q < 0x80000000u ? FZ_OK : fz_set_error(FZ_E_UNSUPPORTED, "-(x mod q) does not fit int32 for q >= 2^31: use fz_pw_sub(0, x), the centred negation");
}
// sums of N products are exact in int64 / fp64 below this many signers; `wording` (one %zu) is the entry's own
constexpr size_t kExactSumLimit = (size_t)1 << 21;
#define REQUIRE_EXACT_SUM(N, wording, shown) FZ_REQUIRE((N) < kExactSumLimit, wording, shown)
// the aggregates of one launch (its grid's z), and the strides between their results: one aggregate needs none, more need at least a
// result's length (need == 0: that result is not asked for)
static bool groups_ok(size_t groups) { return groups <= 65535; }
static bool strides_ok(size_t groups, size_t stride0, size_t need0, size_t stride1 = 0, size_t need1 = 0) {
    return groups <= 1 || (stride0 >= need0 && stride1 >= need1);
}
// A host-pointer wrapper of a DEVICE entry that carves FZ_A_SCRATCH itself stages its operands in this area: the inner entry's
// request may replace the first scratch, never the area under the operands.  (fz_poly_mul_host around fz_poly_mul.)
constexpr int kHostStagingArea = FZ_A_SCRATCH2;

// scratch of fz_verify_with_target_batch: observed [G][D] i32 | coef [G][l][D] i32 | max_abs [G][l] i64 | weight [G][l] i32.
// fz_verify_core carves its own segments on top of the layout for one aggregate, which its inner call requests again.
struct VerifyLayout { FzCarve c; size_t observed, coef, max_abs, weight; };
static VerifyLayout verify_layout(const fz_ctx *ctx, size_t groups, int l) {
    const size_t row = (size_t)ctx->degree * sizeof(int32_t), rows = groups * (size_t)l;
    VerifyLayout v;
    v.observed = v.c.take(groups * row), v.coef = v.c.take(rows * row);
    v.max_abs = v.c.take(rows * sizeof(int64_t)), v.weight = v.c.take(rows * sizeof(int32_t));
    return v;
}

// the five binary pointwise entries (fz_pw_neg: b = a)
static int pw_binary(fz_ctx *ctx, int op, const int32_t *a, const int32_t *b, int32_t *out, size_t count) {
    FZ_REQUIRE(ctx && (count == 0 || (a && b && out)), "NULL argument");
    if (op == FZ_OP_NEG) FZ_TRY(negation_fits(ctx));
    FZ_DEV(ctx);
    return fz_launch_pw(ctx, op, a, b, out, count);
}

// sk_hat = NTT(every secret row); vk_{L,R} = A . sk_hat_{L,R}   (fusion/fusion.py:363-370); bcast: d_coef holds one polynomial per half
static int keygen_core(fz_ctx *ctx, const int32_t *d_A, const int32_t *d_coef, int32_t *d_sk_hat, int32_t *d_vk, size_t batch, int l, bool bcast) {
    FZ_ENTER(ctx, l >= 1 && (batch == 0 || (d_A && d_coef && d_sk_hat && d_vk)), "bad argument");
    if (batch == 0) return FZ_OK;
    if (fused_degree(ctx) && batch * 2 <= 0x7fffffffu && !ctx->knob_unfused &&
        ((((uintptr_t)d_A | (uintptr_t)d_coef | (uintptr_t)d_sk_hat) & 15) == 0))
        return fz_launch_keygen_fused(ctx, d_A, d_coef, d_sk_hat, d_vk, batch * 2, l, bcast);   // one launch, sk_hat not re-read
    // generic degrees: (bcast: expand the rows in sk_hat, transform in place,) then the products
    if (bcast) FZ_TRY(fz_launch_bcast_rows(ctx, d_coef, d_sk_hat, batch * 2, l));
    FZ_TRY(fz_launch_ntt(ctx, bcast ? d_sk_hat : d_coef, d_sk_hat, batch * 2 * (size_t)l, false));
    return fz_launch_matvec(ctx, d_A, d_sk_hat, d_vk, batch * 2, l);
}

extern "C" {

// ---- transforms ----------------------------------------------------------------------------
static int ntt_dev(fz_ctx *ctx, const int32_t *d_in, int32_t *d_out, size_t batch, bool inverse) {
    FZ_ENTER(ctx, batch == 0 || (d_in && d_out), "NULL argument");
    return fz_launch_ntt(ctx, d_in, d_out, batch, inverse);
}
int fz_ntt_forward(fz_ctx *ctx, const int32_t *d_in, int32_t *d_out, size_t batch) { return ntt_dev(ctx, d_in, d_out, batch, false); }
int fz_ntt_inverse(fz_ctx *ctx, const int32_t *d_in, int32_t *d_out, size_t batch) { return ntt_dev(ctx, d_in, d_out, batch, true); }

static int ntt_host(fz_ctx *ctx, int32_t *h_data, size_t batch, bool inverse) {
    FZ_ENTER(ctx, batch == 0 || h_data, "NULL argument");
    if (batch == 0) return FZ_OK;
    const size_t bytes = batch * (size_t)ctx->degree * sizeof(int32_t);
    void *d = nullptr;
    FZ_TRY(fz_scratch(ctx, bytes, &d));
    FZ_TRY(fz_memcpy_h2d(ctx, d, h_data, bytes));
    FZ_TRY(fz_launch_ntt(ctx, (const int32_t *)d, (int32_t *)d, batch, inverse));
    return fz_memcpy_d2h(ctx, h_data, d, bytes);
}
int fz_ntt_forward_host(fz_ctx *ctx, int32_t *h_data, size_t batch) { return ntt_host(ctx, h_data, batch, false); }
int fz_ntt_inverse_host(fz_ctx *ctx, int32_t *h_data, size_t batch) { return ntt_host(ctx, h_data, batch, true); }

// ---- pointwise -------------------------------------------------------------------------------
int fz_pw_mul(fz_ctx *ctx, const int32_t *a, const int32_t *b, int32_t *out, size_t count) { return pw_binary(ctx, FZ_OP_MUL, a, b, out, count); }
int fz_pw_add(fz_ctx *ctx, const int32_t *a, const int32_t *b, int32_t *out, size_t count) { return pw_binary(ctx, FZ_OP_ADD, a, b, out, count); }
int fz_pw_sub(fz_ctx *ctx, const int32_t *a, const int32_t *b, int32_t *out, size_t count) { return pw_binary(ctx, FZ_OP_SUB, a, b, out, count); }
int fz_pw_neg(fz_ctx *ctx, const int32_t *a, int32_t *out, size_t count) { return pw_binary(ctx, FZ_OP_NEG, a, a, out, count); }
int fz_pw_mulacc(fz_ctx *ctx, int32_t *acc, const int32_t *a, const int32_t *b, size_t count) { return pw_binary(ctx, FZ_OP_MULACC, a, b, acc, count); }
int fz_pw_mul_bcast(fz_ctx *ctx, const int32_t *a, const int32_t *s, int32_t *out, size_t rows) {
    FZ_ENTER(ctx, rows == 0 || (a && s && out), "NULL argument");
    return fz_launch_pw_bcast(ctx, a, s, out, rows);
}

int fz_pw_binary_host(fz_ctx *ctx, int op, const int32_t *h_a, const int32_t *h_b, int32_t *h_out, size_t count) {
    FZ_ENTER(ctx, op >= FZ_OP_MUL && op <= FZ_OP_NEG, "bad op %d", op);
    FZ_REQUIRE(count == 0 || (h_a && h_out && (op == FZ_OP_NEG || h_b)), "NULL argument");
    if (op == FZ_OP_NEG) FZ_TRY(negation_fits(ctx));
    if (count == 0) return FZ_OK;
    const size_t bytes = count * sizeof(int32_t);
    FzCarve c;
    const size_t oa = c.take(bytes), ob = c.take(bytes), oout = c.take(bytes);
    FZ_TRY(c.fit(ctx, c.next));
    int32_t *da = c.at<int32_t>(oa), *db = c.at<int32_t>(ob), *dout = c.at<int32_t>(oout);
    FZ_TRY(fz_memcpy_h2d(ctx, da, h_a, bytes));
    if (op != FZ_OP_NEG) FZ_TRY(fz_memcpy_h2d(ctx, db, h_b, bytes));
    FZ_TRY(fz_launch_pw(ctx, op, da, op == FZ_OP_NEG ? da : db, dout, count));
    return fz_memcpy_d2h(ctx, h_out, dout, bytes);
}

// ---- synthetic batches ----------------------------------------------------------------------------
int fz_fill_synthetic(fz_ctx *ctx, int32_t *d_out, size_t count, uint64_t seed) {
    FZ_ENTER(ctx, count == 0 || d_out, "NULL argument");
    return fz_launch_fill_synthetic(ctx, d_out, count, (unsigned long long)seed);
}

// ---- negacyclic product -------------------------------------------------------------------------
int fz_poly_mul(fz_ctx *ctx, const int32_t *d_f, const int32_t *d_g, int32_t *d_out, size_t batch) {
    FZ_ENTER(ctx, batch == 0 || (d_f && d_g && d_out), "NULL argument");
    FZ_TRY(needs_transforms(ctx));
    if (batch == 0) return FZ_OK;
    if ((((uintptr_t)d_f | (uintptr_t)d_g | (uintptr_t)d_out) & 3) != 0)
        return fz_set_error(FZ_E_BADARG, "buffers must be 4-byte aligned");
    if (!ctx->knob_unfused && (fused_degree(ctx) || fz_polymul16_ok(ctx, d_f, d_g, d_out, batch)))
        return fz_launch_polymul_fused(ctx, d_f, d_g, d_out, batch);
    // generic degrees: NTT(f), NTT(g) into scratch, product in place, inverse into out
    const size_t n = batch * (size_t)ctx->degree;
    FzCarve c;
    const size_t of = c.take(n * sizeof(int32_t)), og = c.take(n * sizeof(int32_t));
    FZ_TRY(c.fit(ctx, c.next));
    int32_t *fh = c.at<int32_t>(of), *gh = c.at<int32_t>(og);
    FZ_TRY(fz_launch_ntt(ctx, d_f, fh, batch, false));
    FZ_TRY(fz_launch_ntt(ctx, d_g, gh, batch, false));
    FZ_TRY(fz_launch_pw(ctx, FZ_OP_MUL, fh, gh, fh, n));
    return fz_launch_ntt(ctx, fh, d_out, batch, true);
}

int fz_poly_mul_host(fz_ctx *ctx, const int32_t *h_f, const int32_t *h_g, int32_t *h_out, size_t batch) {
    FZ_ENTER(ctx, batch == 0 || (h_f && h_g && h_out), "NULL argument");
    FZ_TRY(needs_transforms(ctx));
    if (batch == 0) return FZ_OK;
    const size_t bytes = batch * (size_t)ctx->degree * sizeof(int32_t);
    FzCarve c;
    const size_t of = c.take(bytes), og = c.take(bytes);
    FZ_TRY(c.fit(ctx, c.next, kHostStagingArea));
    int32_t *df = c.at<int32_t>(of), *dg = c.at<int32_t>(og);
    FZ_TRY(fz_memcpy_h2d(ctx, df, h_f, bytes));
    FZ_TRY(fz_memcpy_h2d(ctx, dg, h_g, bytes));
    FZ_TRY(fz_poly_mul(ctx, df, dg, df, batch));
    return fz_memcpy_d2h(ctx, h_out, df, bytes);
}

// ---- matrix-vector ------------------------------------------------------------------------------
int fz_matvec(fz_ctx *ctx, const int32_t *A, const int32_t *S, int32_t *out, size_t batch, int l) {
    FZ_ENTER(ctx, l >= 1 && (batch == 0 || (A && S && out)), "bad argument");
    return fz_launch_matvec(ctx, A, S, out, batch, l);
}

int fz_matvec_host(fz_ctx *ctx, const int32_t *h_A, const int32_t *h_S, int32_t *h_out, size_t batch, int l) {
    FZ_ENTER(ctx, l >= 1 && (batch == 0 || (h_A && h_S && h_out)), "bad argument");
    if (batch == 0) return FZ_OK;
    const size_t row = (size_t)ctx->degree * sizeof(int32_t);
    const size_t bA = (size_t)l * row, bS = batch * (size_t)l * row, bO = batch * row;
    FzCarve c;
    const size_t oA = c.take(bA), oS = c.take(bS), oO = c.take(bO);
    FZ_TRY(c.fit(ctx, c.end));
    FZ_TRY(fz_memcpy_h2d(ctx, c.at<void>(oA), h_A, bA));
    FZ_TRY(fz_memcpy_h2d(ctx, c.at<void>(oS), h_S, bS));
    FZ_TRY(fz_launch_matvec(ctx, c.at<const int32_t>(oA), c.at<const int32_t>(oS), c.at<int32_t>(oO), batch, l));
    return fz_memcpy_d2h(ctx, h_out, c.at<void>(oO), bO);
}

// ---- fused scheme cores ---------------------------------------------------------------------------
int fz_keygen_core(fz_ctx *ctx, const int32_t *d_A, const int32_t *d_coef, int32_t *d_sk_hat, int32_t *d_vk, size_t batch, int l) {
    return keygen_core(ctx, d_A, d_coef, d_sk_hat, d_vk, batch, l, false);
}
int fz_keygen_core_bcast(fz_ctx *ctx, const int32_t *d_A, const int32_t *d_coef, int32_t *d_sk_hat, int32_t *d_vk, size_t batch, int l) {
    return keygen_core(ctx, d_A, d_coef, d_sk_hat, d_vk, batch, l, true);
}

int fz_sign_core(fz_ctx *ctx, const int32_t *d_sk_hat, const int32_t *d_c_hat, int32_t *d_sig, size_t batch, int l) {
    FZ_ENTER(ctx, l >= 1 && (batch == 0 || (d_sk_hat && d_c_hat && d_sig)), "bad argument");
    return fz_launch_sign(ctx, d_sk_hat, d_c_hat, d_sig, batch, l);
}

int fz_aggregate_partial_batch(fz_ctx *ctx, const int32_t *d_sig, const int32_t *d_alpha_hat, int64_t *d_partial,
                               size_t partial_stride, size_t groups, size_t N, int l) {
    FZ_ENTER(ctx, l >= 1 && d_partial && (N == 0 || groups == 0 || (d_sig && d_alpha_hat)), "bad argument");
    REQUIRE_EXACT_SUM(N, "N=%zu too large for exact int64/fp64 accumulation (< 2^21)", N);
    FZ_REQUIRE(groups_ok(groups) && strides_ok(groups, partial_stride, (size_t)l * ctx->degree), "bad groups / stride");
    return fz_launch_aggregate(ctx, d_sig, d_alpha_hat, d_partial, partial_stride, nullptr, groups, N, l);
}

int fz_aggregate_target_partial_batch(fz_ctx *ctx, const int32_t *d_sig, const int32_t *d_alpha_hat, const int32_t *d_vkL,
                                      const int32_t *d_vkR, const int32_t *d_c_hat, int64_t *d_partial, size_t partial_stride,
                                      int64_t *d_target_partial, size_t target_stride, size_t groups, size_t N, int l) {
    FZ_ENTER(ctx, l >= 1 && d_partial && d_target_partial, "bad argument");
    FZ_REQUIRE(N == 0 || groups == 0 || (d_sig && d_alpha_hat && d_vkL && d_vkR && d_c_hat), "NULL argument");
    REQUIRE_EXACT_SUM(N, "N=%zu too large for exact int64/fp64 accumulation (< 2^21)", N);
    FZ_REQUIRE(groups_ok(groups) && strides_ok(groups, partial_stride, (size_t)l * ctx->degree, target_stride, (size_t)ctx->degree),
               "bad groups / strides");
    FZ_REQUIRE((((uintptr_t)d_vkL | (uintptr_t)d_vkR | (uintptr_t)d_c_hat | (uintptr_t)d_alpha_hat | (uintptr_t)d_sig) & 15) == 0,
               "inputs must be 16-byte aligned");
    return fz_launch_aggregate(ctx, d_sig, d_alpha_hat, d_partial, partial_stride, nullptr, groups, N, l, d_vkL, d_vkR, d_c_hat,
                               d_target_partial, target_stride);
}

int fz_sign_aggregate_target_partial_batch(fz_ctx *ctx, const int32_t *d_sk_hat, const int32_t *d_c_hat, const int32_t *d_alpha_hat,
                                           const int32_t *d_vkL, const int32_t *d_vkR, int32_t *d_sig, int64_t *d_partial,
                                           size_t partial_stride, int64_t *d_target_partial, size_t target_stride, size_t groups,
                                           size_t N, int l) {
    FZ_ENTER(ctx, l >= 1 && d_partial, "bad argument");
    FZ_REQUIRE((d_vkL != nullptr) == (d_vkR != nullptr) && (d_vkL != nullptr) == (d_target_partial != nullptr),
               "verification keys and the target's partials come together or not at all");
    FZ_REQUIRE(N == 0 || groups == 0 || (d_sk_hat && d_c_hat && d_alpha_hat && d_sig), "NULL argument");
    REQUIRE_EXACT_SUM(N, "N=%zu too large for exact int64/fp64 accumulation (< 2^21)", N);
    FZ_REQUIRE(groups_ok(groups) && strides_ok(groups, partial_stride, (size_t)l * ctx->degree, target_stride, d_vkL ? (size_t)ctx->degree : 0),
               "bad groups / strides");
    if (N == 0 || groups == 0) return FZ_OK;
    const int d = ctx->degree;
    const uintptr_t align = (uintptr_t)d_sk_hat | (uintptr_t)d_c_hat | (uintptr_t)d_alpha_hat | (uintptr_t)d_vkL | (uintptr_t)d_vkR | (uintptr_t)d_sig;
    if (!ctx->knob_unfused && d % 4 == 0 && (d & (d - 1)) == 0 && d <= 256 && (align & 15) == 0)
        // one launch: sigma is written as it is computed and aggregated from registers (aggregate_onepass<.., SIGN>)
        return fz_launch_aggregate(ctx, nullptr, d_alpha_hat, d_partial, partial_stride, nullptr, groups, N, l, d_vkL, d_vkR, d_c_hat,
                                   d_target_partial, target_stride, nullptr, d_sk_hat, d_sig);
    // any other degree or alignment (and FZ_UNFUSED=1): the two launches this call stands for
    FZ_TRY(fz_launch_sign(ctx, d_sk_hat, d_c_hat, d_sig, groups * N, l));
    return fz_launch_aggregate(ctx, d_sig, d_alpha_hat, d_partial, partial_stride, nullptr, groups, N, l, d_vkL, d_vkR, d_c_hat,
                               d_target_partial, target_stride);
}

int fz_aggregate_partial(fz_ctx *ctx, const int32_t *d_sig, const int32_t *d_alpha_hat, int64_t *d_partial, size_t N, int l) {
    return fz_aggregate_partial_batch(ctx, d_sig, d_alpha_hat, d_partial, 0, 1, N, l);
}

// many aggregates of different sizes: chunks of kFzRaggedMax groups per launch
static int aggregate_ragged(fz_ctx *ctx, const int32_t *d_sig, const int32_t *d_alpha_hat, const int32_t *d_vkL, const int32_t *d_vkR,
                            const int32_t *d_c_hat, const size_t *h_offsets, size_t groups, int l, int32_t *d_out32,
                            int64_t *d_partial, size_t partial_stride, int64_t *d_target_partial, size_t target_stride) {
    const size_t per = (size_t)l * ctx->degree;
    for (size_t g = 0; g < groups; ++g) {
        FZ_REQUIRE(h_offsets[g] <= h_offsets[g + 1], "offsets must not decrease");
        REQUIRE_EXACT_SUM(h_offsets[g + 1] - h_offsets[g], "aggregate %zu: too many signers for exact accumulation (< 2^21)", g);
    }
    FZ_REQUIRE(h_offsets[groups] < 0xffffffffull, "too many signers in one call");
    for (size_t g0 = 0; g0 < groups; g0 += (size_t)kFzRaggedMax) {
        const size_t n = std::min<size_t>(kFzRaggedMax, groups - g0);
        size_t nmax = 0;
        for (size_t g = g0; g < g0 + n; ++g) nmax = std::max(nmax, h_offsets[g + 1] - h_offsets[g]);
        FZ_TRY(fz_launch_aggregate(ctx, d_sig, d_alpha_hat, d_partial ? d_partial + g0 * partial_stride : nullptr, partial_stride,
                                   d_out32 ? d_out32 + g0 * per : nullptr, n, nmax, l, d_vkL, d_vkR, d_c_hat,
                                   d_target_partial ? d_target_partial + g0 * target_stride : nullptr, target_stride, h_offsets + g0));
    }
    return FZ_OK;
}

int fz_aggregate_core_ragged(fz_ctx *ctx, const int32_t *d_sig, const int32_t *d_alpha_hat, const size_t *h_offsets, size_t groups,
                             int l, int32_t *d_out) {
    FZ_ENTER(ctx, l >= 1 && h_offsets && (groups == 0 || (d_sig && d_alpha_hat && d_out)), "bad argument");
    if (groups == 0) return FZ_OK;
    return aggregate_ragged(ctx, d_sig, d_alpha_hat, nullptr, nullptr, nullptr, h_offsets, groups, l, d_out, nullptr, 0, nullptr, 0);
}

int fz_aggregate_target_partial_ragged(fz_ctx *ctx, const int32_t *d_sig, const int32_t *d_alpha_hat, const int32_t *d_vkL,
                                       const int32_t *d_vkR, const int32_t *d_c_hat, const size_t *h_offsets, size_t groups, int l,
                                       int64_t *d_partial, size_t partial_stride, int64_t *d_target_partial, size_t target_stride) {
    FZ_REQUIRE(ctx && l >= 1 && h_offsets && d_target_partial && d_alpha_hat && d_vkL && d_vkR && d_c_hat, "bad argument");
    FZ_REQUIRE((d_sig == nullptr) == (d_partial == nullptr), "d_sig and d_partial go together (both NULL: verification targets only)");
    FZ_DEV(ctx);
    if (groups == 0) return FZ_OK;
    FZ_REQUIRE(strides_ok(groups, partial_stride, d_partial ? (size_t)l * ctx->degree : 0, target_stride, (size_t)ctx->degree), "bad strides");
    return aggregate_ragged(ctx, d_sig, d_alpha_hat, d_vkL, d_vkR, d_c_hat, h_offsets, groups, l, nullptr, d_partial, partial_stride,
                            d_target_partial, target_stride);
}

int fz_reduce_i64(fz_ctx *ctx, const int64_t *d_in, int32_t *d_out, size_t count) {
    FZ_ENTER(ctx, count == 0 || (d_in && d_out), "NULL argument");
    return fz_launch_reduce_i64(ctx, d_in, d_out, count);
}

int fz_aggregate_core(fz_ctx *ctx, const int32_t *d_sig, const int32_t *d_alpha_hat, int32_t *d_out, size_t N, int l) {
    FZ_ENTER(ctx, l >= 1 && N >= 1 && d_sig && d_alpha_hat && d_out, "bad argument");
    REQUIRE_EXACT_SUM(N, "N=%zu too large for exact fp64 accumulation (< 2^21)", N);
    return fz_launch_aggregate(ctx, d_sig, d_alpha_hat, nullptr, 0, d_out, 1, N, l);
}

int fz_target_partial_batch(fz_ctx *ctx, const int32_t *d_vkL, const int32_t *d_vkR, const int32_t *d_c_hat,
                            const int32_t *d_alpha_hat, int64_t *d_partial, size_t partial_stride, size_t groups,
                            size_t N) {
    FZ_ENTER(ctx, d_partial && (N == 0 || groups == 0 || (d_vkL && d_vkR && d_c_hat && d_alpha_hat)), "bad argument");
    REQUIRE_EXACT_SUM(N, "N=%zu too large (< 2^21)", N);
    FZ_REQUIRE(groups_ok(groups) && strides_ok(groups, partial_stride, (size_t)ctx->degree), "bad groups / stride");
    return fz_launch_target_partial(ctx, d_vkL, d_vkR, d_c_hat, d_alpha_hat, d_partial, partial_stride, groups, N);
}

int fz_target_partial(fz_ctx *ctx, const int32_t *d_vkL, const int32_t *d_vkR, const int32_t *d_c_hat,
                      const int32_t *d_alpha_hat, int64_t *d_partial, size_t N) {
    return fz_target_partial_batch(ctx, d_vkL, d_vkR, d_c_hat, d_alpha_hat, d_partial, 0, 1, N);
}

int fz_norm_weight(fz_ctx *ctx, const int32_t *d_coef, size_t batch, int64_t *d_max_abs, int32_t *d_weight) {
    FZ_ENTER(ctx, batch == 0 || (d_coef && d_max_abs && d_weight), "NULL argument");
    return fz_launch_norm_weight(ctx, d_coef, batch, d_max_abs, d_weight);
}

int fz_norm_weight_host(fz_ctx *ctx, const int32_t *h_coef, size_t batch, int64_t *h_max_abs, int32_t *h_weight) {
    FZ_ENTER(ctx, batch == 0 || (h_coef && h_max_abs && h_weight), "NULL argument");
    if (batch == 0) return FZ_OK;
    const size_t bC = batch * (size_t)ctx->degree * sizeof(int32_t), bM = batch * sizeof(int64_t), bW = batch * sizeof(int32_t);
    FzCarve c;
    const size_t oC = c.take(bC), oM = c.take(bM), oW = c.take(bW);
    FZ_TRY(c.fit(ctx, c.end));
    FZ_TRY(fz_memcpy_h2d(ctx, c.at<void>(oC), h_coef, bC));
    FZ_TRY(fz_launch_norm_weight(ctx, c.at<const int32_t>(oC), batch, c.at<int64_t>(oM), c.at<int32_t>(oW)));
    FZ_TRY(fz_memcpy_d2h(ctx, h_max_abs, c.at<void>(oM), bM));
    return fz_memcpy_d2h(ctx, h_weight, c.at<void>(oW), bW);
}

int fz_verify_with_target_batch(fz_ctx *ctx, const int32_t *d_A, const int32_t *d_sig, const int32_t *d_target,
                                size_t groups, int l, int64_t beta_vf, int64_t omega_vf, int *h_verdicts) {
    FZ_ENTER(ctx, l >= 1 && groups >= 1 && groups_ok(groups) && d_A && d_sig && d_target && h_verdicts, "bad argument");
    VerifyLayout v = verify_layout(ctx, groups, l);
    FZ_TRY(v.c.fit(ctx, v.c.end));                 // (the fused path below requests it too and never reads it)
    int *d_verdict = nullptr;
    FZ_TRY(fz_verdict_area(ctx, groups, &d_verdict));
    if (fused_degree(ctx) && !ctx->knob_unfused) {
        // one launch: sigma read once (matvec + inverse transforms + norm/weight + verdict fused)
        FZ_TRY(fz_launch_verify_fused(ctx, d_A, d_sig, d_target, groups, l, beta_vf, omega_vf, d_verdict));
    } else {
        int32_t *observed = v.c.at<int32_t>(v.observed), *coef = v.c.at<int32_t>(v.coef), *wt = v.c.at<int32_t>(v.weight);
        int64_t *mx = v.c.at<int64_t>(v.max_abs);
        FZ_TRY(fz_launch_matvec(ctx, d_A, d_sig, observed, groups, l));               // fusion.py:715-717
        FZ_TRY(fz_launch_ntt(ctx, d_sig, coef, groups * (size_t)l, true));            // fusion.py:690-692
        FZ_TRY(fz_launch_norm_weight(ctx, coef, groups * (size_t)l, mx, wt));         // fusion.py:722-727
        FZ_TRY(fz_launch_verdict(ctx, d_target, observed, mx, wt, groups, l, beta_vf, omega_vf, d_verdict));
    }
    return fz_memcpy_d2h(ctx, h_verdicts, d_verdict, groups * sizeof(int));
}

int fz_verify_with_target_batch_async(fz_ctx *ctx, const int32_t *d_A, const int32_t *d_sig, const int32_t *d_target,
                                      size_t groups, int l, int64_t beta_vf, int64_t omega_vf, int *d_verdicts) {
    FZ_ENTER(ctx, l >= 1 && groups >= 1 && groups_ok(groups) && d_A && d_sig && d_target && d_verdicts, "bad argument");
    FZ_TRY(needs_fused(ctx, "asynchronous verification"));
    return fz_launch_verify_fused(ctx, d_A, d_sig, d_target, groups, l, beta_vf, omega_vf, d_verdicts);
}

int fz_verify_signatures_async(fz_ctx *ctx, const int32_t *d_A, const int32_t *d_sig, const int32_t *d_vk,
                               const int32_t *d_c_hat, size_t N, int l, int64_t beta, int64_t omega, int *d_verdicts) {
    FZ_REQUIRE(ctx && l >= 1 && beta >= 0 && omega >= 0, "bad argument");
    if (N == 0) return FZ_OK;
    FZ_REQUIRE(d_A && d_sig && d_vk && d_c_hat && d_verdicts, "NULL argument");
    FZ_REQUIRE((((uintptr_t)d_A | (uintptr_t)d_sig) & 15) == 0, "A and the signatures must be 16-byte aligned");
    FZ_TRY(needs_fused(ctx, "per-signature verification"));
    FZ_DEV(ctx);
    return fz_launch_verify_signatures(ctx, d_A, d_sig, d_vk, d_c_hat, N, l, beta, omega, d_verdicts);
}

int fz_verify_partials_batch_async(fz_ctx *ctx, const int32_t *d_A, const int64_t *d_partial, size_t partial_stride,
                                   const int64_t *d_target_partial, size_t target_stride, size_t groups, int l,
                                   int64_t beta_vf, int64_t omega_vf, int *d_verdicts) {
    FZ_ENTER(ctx, l >= 1 && groups >= 1 && groups_ok(groups) && d_A && d_partial && d_target_partial && d_verdicts, "bad argument");
    FZ_REQUIRE(strides_ok(groups, partial_stride, (size_t)l * ctx->degree, target_stride, (size_t)ctx->degree), "bad strides");
    FZ_REQUIRE((((uintptr_t)d_partial | (uintptr_t)d_target_partial | (uintptr_t)d_A) & 15) == 0 && (partial_stride & 1) == 0,
               "partials must be 16-byte aligned");
    FZ_TRY(needs_fused(ctx, "verification from int64 partials"));
    return fz_launch_verify_fused_i64(ctx, d_A, d_partial, partial_stride, d_target_partial, target_stride, groups, l, beta_vf,
                                      omega_vf, d_verdicts);
}

int fz_verify_with_target(fz_ctx *ctx, const int32_t *d_A, const int32_t *d_sig, const int32_t *d_target, int l,
                          int64_t beta_vf, int64_t omega_vf, int *h_verdict) {
    return fz_verify_with_target_batch(ctx, d_A, d_sig, d_target, 1, l, beta_vf, omega_vf, h_verdict);
}

int fz_verify_core(fz_ctx *ctx, const int32_t *d_A, const int32_t *d_sig, const int32_t *d_vkL, const int32_t *d_vkR,
                   const int32_t *d_c_hat, const int32_t *d_alpha_hat, size_t N, int l,
                   int64_t beta_vf, int64_t omega_vf, int *h_verdict) {
    FZ_ENTER(ctx, l >= 1 && N >= 1 && d_A && d_sig && d_vkL && d_vkR && d_c_hat && d_alpha_hat && h_verdict, "bad argument");
    // the int64 sums and the target live behind the layout of fz_verify_with_target, carved on top of it: both allocated up front
    VerifyLayout v = verify_layout(ctx, 1, l);
    const size_t inner = v.c.end;                  // what the call at the end requests
    const size_t oP = v.c.take((size_t)ctx->degree * sizeof(int64_t)), oT = v.c.take((size_t)ctx->degree * sizeof(int32_t));
    assert(v.c.end >= inner);                      // so that request fits the area sized here: it never replaces the area under the target
    FZ_TRY(v.c.fit(ctx, v.c.end));
    int64_t *partial = v.c.at<int64_t>(oP);
    int32_t *target = v.c.at<int32_t>(oT);
    FZ_TRY(fz_target_partial(ctx, d_vkL, d_vkR, d_c_hat, d_alpha_hat, partial, N));   // fusion.py:706-714
    FZ_TRY(fz_launch_reduce_i64(ctx, partial, target, (size_t)ctx->degree));
    return fz_verify_with_target(ctx, d_A, d_sig, target, l, beta_vf, omega_vf, h_verdict);
}


// ---- many independent transforms in one dispatch -------------------------------------------------------
int fz_ntt_multi(fz_ctx *ctx, const fz_ntt_job *h_jobs, size_t n_jobs) {
    FZ_ENTER(ctx, n_jobs == 0 || h_jobs, "NULL argument");
    FZ_TRY(needs_transforms(ctx));
    for (size_t j = 0; j < n_jobs; ++j) {
        const fz_ntt_job &jb = h_jobs[j];
        FZ_REQUIRE(jb.rows == 0 || (jb.d_in && jb.d_out), "job %zu: NULL buffer", j);
        FZ_REQUIRE(jb.rows < ((size_t)1 << 31), "job %zu: too many rows", j);
        if ((((uintptr_t)jb.d_in | (uintptr_t)jb.d_out) & 15) != 0 && ctx->logd >= 2)
            return fz_set_error(FZ_E_BADARG, "job %zu: transform buffers must be 16-byte aligned", j);
    }
    if (!fused_degree(ctx)) {                            // other degrees: one launch per job (same results)
        for (size_t j = 0; j < n_jobs; ++j)
            FZ_TRY(fz_launch_ntt(ctx, h_jobs[j].d_in, h_jobs[j].d_out, h_jobs[j].rows, h_jobs[j].inverse != 0));
        return FZ_OK;
    }
    const unsigned ppw = 64u / (unsigned)(ctx->degree / 4);
    FzMultiJobs J;
    memset(&J, 0, sizeof(J));
    unsigned long long total = 0;
    for (size_t j = 0; j < n_jobs; ++j) {
        const fz_ntt_job &jb = h_jobs[j];
        if (jb.rows == 0) continue;
        const unsigned long long tasks = (jb.rows + ppw - 1) / ppw;
        if (J.n == kFzMultiMax || total + tasks > 0x7fffffffull) {      // table full: flush
            FZ_TRY(fz_launch_ntt_multi(ctx, J));
            memset(&J, 0, sizeof(J));
            total = 0;
        }
        total += tasks;
        J.in[J.n] = jb.d_in;
        J.out[J.n] = jb.d_out;
        J.rows[J.n] = (unsigned)jb.rows | (jb.inverse ? 0x80000000u : 0u);
        ++J.n;
    }
    return fz_launch_ntt_multi(ctx, J);
}

}  // extern "C"
