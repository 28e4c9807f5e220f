// fz_pointwise.hip -- the small streaming kernels: pointwise ring ops, the (1 x l).(l x 1) product, signing, and the target /
// reduce / norm-weight / verdict steps of verification, row broadcast and synthetic fill (aggregation has its own unit,
// fz_aggregate.hip).  All are HBM-bound (one modular multiply-add per 4..12 bytes moved): 16-byte-per-lane coalesced accesses,
// grid-stride loops over a grid capped at a few blocks per CU, fp64 exact arithmetic from fz_arith.h.
//
// Reference formulas: algebra/polynomials.py:303-385 (pointwise), algebra/matrices.py:108-131
// (scalar and matrix products), fusion/fusion.py:557 (sign), :706-727 (verify).  Every partial result the reference centres is
// congruent mod q to the lazily accumulated value here, and the final value is centred once -- identical output.
#include "fz_stream_dev.h"
#include "../../include/fusion_hip.h"

namespace {

template <int OP>
__device__ __forceinline__ int pw_op(int a, int b, int acc, const FzMod m) {
    if (OP == FZ_OP_MUL) return (int)fz_mulmod_cent((double)a, (double)b, m);
    if (OP == FZ_OP_ADD) return cent_i32((double)a + (double)b, m);
    if (OP == FZ_OP_SUB) return cent_i32((double)a - (double)b, m);
    if (OP == FZ_OP_NEG) {   // -(x mod q), x mod q in [0,q): reference __neg__ (polynomials.py:325-333)
        double c = fz_cent((double)a, m);
        double y = c < 0.0 ? c + m.q : c;
        return (int)(-y);
    }
    // MULACC
    return cent_i32((double)acc + fz_mulmod((double)a, (double)b, m), m);
}

template <int OP>
__global__ __launch_bounds__(kBlock) void pw_kernel(const int32_t *a, const int32_t *b, int32_t *out,
                                                    size_t count, int vec, FzMod m) {
    const size_t n4 = vec ? count / 4 : 0;   // vec == 0: pointers not 16-byte aligned, all scalar
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int4 *a4 = reinterpret_cast<const int4 *>(a);
    const int4 *b4 = reinterpret_cast<const int4 *>(b);
    int4 *o4 = reinterpret_cast<int4 *>(out);
    for (size_t i = gid; i < n4; i += stride) {
        int4 x = a4[i];
        int4 y = (OP == FZ_OP_NEG) ? x : b4[i];
        int4 z = (OP == FZ_OP_MULACC) ? o4[i] : x;
        int4 o;
        o.x = pw_op<OP>(x.x, y.x, z.x, m);
        o.y = pw_op<OP>(x.y, y.y, z.y, m);
        o.z = pw_op<OP>(x.z, y.z, z.z, m);
        o.w = pw_op<OP>(x.w, y.w, z.w, m);
        o4[i] = o;        // a normal store: the consumer usually follows at once (streaming stores: +2.5 % cold, measured in round 2)
    }
    // ragged tail (count not a multiple of 4) or the whole range when unaligned
    for (size_t i = n4 * 4 + gid; i < count; i += stride) {
        int x = a[i];
        int y = (OP == FZ_OP_NEG) ? x : b[i];
        int z = (OP == FZ_OP_MULACC) ? out[i] : x;
        out[i] = pw_op<OP>(x, y, z, m);
    }
}

// out[row][j] = cent(a[row][j] * s[j]); d4 = degree/4 (degree >= 4) or scalar path
__global__ __launch_bounds__(kBlock) void pw_bcast_kernel(const int32_t *a, const int32_t *s, int32_t *out,
                                                          size_t total, int degree, FzMod m) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int j = (int)(i % (size_t)degree);
        out[i] = (int)fz_mulmod_cent((double)a[i], (double)s[j], m);
    }
}

// s0..s3 += x * y mod q over the four lanes of an int4 (the operands by value, the sums by reference: the form under which its
// callers compile to the code they had with the four lines written out)
__device__ __forceinline__ void mulmod_acc4(int4 x, int4 y, double &s0, double &s1, double &s2, double &s3, FzMod m) {
    s0 += fz_mulmod((double)x.x, (double)y.x, m);
    s1 += fz_mulmod((double)x.y, (double)y.y, m);
    s2 += fz_mulmod((double)x.z, (double)y.z, m);
    s3 += fz_mulmod((double)x.w, (double)y.w, m);
}

// out[b][j] = cent(sum_k A[k][j] * S[b][k][j]); one thread per (b, 4 coefficients).  The rows of a product are a
// sequential chain for its thread: eight rows (16 loads of 16 bytes) are requested together before any arithmetic
// (one row at a time the kernel ran at 39 % of HBM peak on cold operands: latency, not bandwidth).
__global__ __launch_bounds__(kBlock) void matvec_kernel(const int32_t *A, const int32_t *S, int32_t *out,
                                                        size_t batch, int l, int degree, FzMod m) {
    constexpr int U = 8;
    const int d4 = degree / 4;
    const size_t total = batch * (size_t)d4;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const size_t b = i / d4;
        const int j4 = (int)(i % d4);
        const int4 *Ap = reinterpret_cast<const int4 *>(A) + j4;
        const int4 *Sp = reinterpret_cast<const int4 *>(S + b * (size_t)l * degree) + j4;
        double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
        int k = 0;
        for (; k + U <= l; k += U) {
            int4 x[U], y[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                x[u] = Ap[(size_t)(k + u) * d4];
                y[u] = Sp[(size_t)(k + u) * d4];
            }
            // written out: with mulmod_acc4 here, 24 v_mul_f64 of this kernel come out with their sources exchanged (docs/HISTORY.md §O)
#pragma unroll
            for (int u = 0; u < U; ++u) {
                s0 += fz_mulmod((double)x[u].x, (double)y[u].x, m);
                s1 += fz_mulmod((double)x[u].y, (double)y[u].y, m);
                s2 += fz_mulmod((double)x[u].z, (double)y[u].z, m);
                s3 += fz_mulmod((double)x[u].w, (double)y[u].w, m);
            }
        }
        for (; k < l; ++k) mulmod_acc4(Ap[(size_t)k * d4], Sp[(size_t)k * d4], s0, s1, s2, s3, m);
        int4 o;
        o.x = cent_i32(s0, m); o.y = cent_i32(s1, m); o.z = cent_i32(s2, m); o.w = cent_i32(s3, m);
        reinterpret_cast<int4 *>(out + b * (size_t)degree)[j4] = o;
    }
}
// The same product as (CX, KS) workgroups, CX = max(64, 256 / KS) columns (product, 4 coefficients) by KS slices of the k
// range: the waves with threadIdx.y = y take slice y -- KS times the rows in flight when one wave per 64 columns would leave
// the chip short of waves (2048 products of degree 64 are 512 of them) -- and accumulate in INTEGERS: A
// split into 16-bit halves on the fly, hi += s * (A >> 16), lo += s * (A & 0xffff) (v_mad_i64_i32), exact for any int32
// operands while l <= 2^15 (fz_arith.h).  Every iteration requests eight rows whether the slice still has eight or not (the
// row index is clamped, the surplus is not accumulated: the slice bounds are wave-uniform) -- a tail of single-row iterations
// is a chain of dependent round trips (five of them at four slices of 83 rows: 37.9 us against 33.6 with two slices).  The
// slices' sums meet in LDS; slice 0 reduces them to the centred row.
template <int KS>
__global__ __launch_bounds__(KS <= 4 ? 256 : 64 * KS) void matvec_sliced_kernel(const int32_t *A, const int32_t *S, int32_t *out,
                                                                                size_t batch, int l, int degree, FzMod m) {
    constexpr int U = 8, CX = KS <= 4 ? 256 / KS : 64;
    __shared__ long long red[(KS > 1 ? KS - 1 : 1) * 8 * CX];
    const int d4 = degree / 4;
    const size_t total = batch * (size_t)d4;
    const size_t i_raw = (size_t)blockIdx.x * CX + threadIdx.x;
    const bool live = i_raw < total;
    const size_t i = live ? i_raw : total - 1;          // idle lanes of the last workgroup shadow the last column and store nothing
    const int sl = threadIdx.y;
    const size_t b = i / d4;
    const int j4 = (int)(i % d4);
    const int per = (l + KS - 1) / KS;
    const int k1 = (sl + 1) * per < l ? (sl + 1) * per : l;
    const int4 *Ap = reinterpret_cast<const int4 *>(A) + j4;
    const int4 *Sp = reinterpret_cast<const int4 *>(S + b * (size_t)l * degree) + j4;
    long long h0 = 0, h1 = 0, h2 = 0, h3 = 0, l0 = 0, l1 = 0, l2 = 0, l3 = 0;
#define FZ_MV_ACC(XA, YS) \
    h0 += (long long)(YS).x * ((XA).x >> 16); l0 += (long long)(YS).x * ((XA).x & 0xffff); \
    h1 += (long long)(YS).y * ((XA).y >> 16); l1 += (long long)(YS).y * ((XA).y & 0xffff); \
    h2 += (long long)(YS).z * ((XA).z >> 16); l2 += (long long)(YS).z * ((XA).z & 0xffff); \
    h3 += (long long)(YS).w * ((XA).w >> 16); l3 += (long long)(YS).w * ((XA).w & 0xffff);
    for (int k = sl * per; k < k1; k += U) {
        int4 x[U], y[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int kk = k + u < k1 ? k + u : k1 - 1;
            x[u] = Ap[(size_t)kk * d4];
            y[u] = ld_stream4(Sp + (size_t)kk * d4);        // the vectors are read once (A is every product's: from the L2)
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (k + u < k1) { FZ_MV_ACC(x[u], y[u]) }
    }
#undef FZ_MV_ACC
    if (KS > 1) {
        if (sl > 0) {
            long long *mine = red + (size_t)(sl - 1) * 8 * CX + threadIdx.x;
            mine[0] = h0; mine[CX] = h1; mine[2 * CX] = h2; mine[3 * CX] = h3;
            mine[4 * CX] = l0; mine[5 * CX] = l1; mine[6 * CX] = l2; mine[7 * CX] = l3;
        }
        __syncthreads();
        if (sl > 0) return;
#pragma unroll
        for (int t = 0; t < KS - 1; ++t) {
            const long long *o = red + (size_t)t * 8 * CX + threadIdx.x;
            h0 += o[0]; h1 += o[CX]; h2 += o[2 * CX]; h3 += o[3 * CX];
            l0 += o[4 * CX]; l1 += o[5 * CX]; l2 += o[6 * CX]; l3 += o[7 * CX];
        }
    }
    if (!live) return;
    const bool small = l <= 32;
    int4 o;
    o.x = cent_i32(fz_imad_total(h0, l0, small, m), m); o.y = cent_i32(fz_imad_total(h1, l1, small, m), m);
    o.z = cent_i32(fz_imad_total(h2, l2, small, m), m); o.w = cent_i32(fz_imad_total(h3, l3, small, m), m);
    reinterpret_cast<int4 *>(out + b * (size_t)degree)[j4] = o;
}
// Few products (verify: one per aggregate): one 1024-thread block per product, the k-loop split over
// 1024/(degree/4) slices and reduced through LDS -- 83 dependent-latency iterations become 6.
__global__ __launch_bounds__(1024) void matvec_split_kernel(const int32_t *A, const int32_t *S, int32_t *out,
                                                            int l, int degree, FzMod m) {
    __shared__ double red[1024 * 4];
    const int d4 = degree / 4, slices = 1024 / d4;
    const int j4 = threadIdx.x % d4, sl = threadIdx.x / d4;
    const size_t b = blockIdx.x;
    const int4 *Ap = reinterpret_cast<const int4 *>(A) + j4;
    const int4 *Sp = reinterpret_cast<const int4 *>(S + b * (size_t)l * degree) + j4;
    double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    for (int k = sl; k < l; k += slices) mulmod_acc4(Ap[(size_t)k * d4], Sp[(size_t)k * d4], s0, s1, s2, s3, m);
    double *mine = red + (size_t)threadIdx.x * 4;
    mine[0] = s0; mine[1] = s1; mine[2] = s2; mine[3] = s3;
    __syncthreads();
    if (sl == 0) {
        for (int t = 1; t < slices; ++t) {
            const double *o = red + (size_t)(t * d4 + j4) * 4;
            s0 += o[0]; s1 += o[1]; s2 += o[2]; s3 += o[3];
        }
        int4 r;
        r.x = cent_i32(s0, m); r.y = cent_i32(s1, m); r.z = cent_i32(s2, m); r.w = cent_i32(s3, m);
        reinterpret_cast<int4 *>(out + b * (size_t)degree)[j4] = r;
    }
}
// any degree (degree % 4 != 0, or rows that are not 16-byte aligned): scalar
__global__ __launch_bounds__(kBlock) void matvec_scalar_kernel(const int32_t *A, const int32_t *S, int32_t *out,
                                                               size_t batch, int l, int degree, FzMod m) {
    const size_t total = batch * (size_t)degree;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const size_t b = i / degree;
        const int j = (int)(i % degree);
        double s = 0;
        for (int k = 0; k < l; ++k)
            s += fz_mulmod((double)A[(size_t)k * degree + j], (double)S[(b * l + k) * (size_t)degree + j], m);
        out[i] = cent_i32(s, m);
    }
}

// sig[b][k][j] = cent(cent(L[b][k][j] * c[b][j]) + R[b][k][j]); sk_hat = [batch][2][l][degree]
__global__ __launch_bounds__(kBlock) void sign_kernel(const int32_t *sk_hat, const int32_t *c_hat, int32_t *sig,
                                                      size_t batch, int l, int degree, FzMod m) {
    const int d4 = degree / 4;
    const size_t per_sig = (size_t)l * d4;
    const size_t total = batch * per_sig;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const size_t b = i / per_sig;
        const size_t rem = i % per_sig;          // k*d4 + j4
        const int j4 = (int)(rem % d4);
        const int4 *Lp = reinterpret_cast<const int4 *>(sk_hat + b * 2 * (size_t)l * degree);
        const int4 *Rp = Lp + per_sig;
        const int4 x = ld_stream4(Lp + rem), y = ld_stream4(Rp + rem);      // the key halves are read once
        int4 c = reinterpret_cast<const int4 *>(c_hat + b * (size_t)degree)[j4];
        int4 o;
        o.x = cent_i32(fz_mulmod((double)x.x, (double)c.x, m) + (double)y.x, m);
        o.y = cent_i32(fz_mulmod((double)x.y, (double)c.y, m) + (double)y.y, m);
        o.z = cent_i32(fz_mulmod((double)x.z, (double)c.z, m) + (double)y.z, m);
        o.w = cent_i32(fz_mulmod((double)x.w, (double)c.w, m) + (double)y.w, m);
        // a normal store: the aggregation usually reads the signatures next, and finds most of them in the caches -- sign 44.0 us
        // + aggregate 8.8 us chained (aggregate alone, cold: 17.6); a streaming store makes sign 40.9 us and the pair 58.2
        // (profiles/r05_keygen_sign_pair.txt, tools/probes/keygen_sign_pair.py)
        reinterpret_cast<int4 *>(sig)[i] = o;
    }
}

// any degree (degree % 4 != 0 included): one thread per coefficient
__global__ __launch_bounds__(kBlock) void sign_scalar_kernel(const int32_t *sk_hat, const int32_t *c_hat, int32_t *sig,
                                                             size_t batch, int l, int degree, FzMod m) {
    const size_t per_sig = (size_t)l * degree, total = batch * per_sig;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const size_t b = i / per_sig, rem = i % per_sig;
        const int32_t *Lp = sk_hat + b * 2 * per_sig;
        const double cj = (double)c_hat[b * (size_t)degree + rem % degree];
        sig[i] = cent_i32(fz_mulmod((double)Lp[rem], cj, m) + (double)Lp[per_sig + rem], m);
    }
}

__device__ __forceinline__ void atomic_add_i64(int64_t *p, double v) {
    atomicAdd(reinterpret_cast<unsigned long long *>(p), (unsigned long long)(long long)v);
}

// partial[g][j] += sum_i ((vkL_i*c_i + vkR_i) * alpha_i)[j]; one thread per coefficient, grid.y splits N
__global__ __launch_bounds__(kBlock) void target_kernel(const int32_t *vkL, const int32_t *vkR, const int32_t *c,
                                                        const int32_t *alpha, int64_t *partial, size_t pstride,
                                                        size_t N, int degree, FzMod m) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= degree) return;
    const size_t g = blockIdx.z, goff = g * N * (size_t)degree;
    const size_t per = (N + gridDim.y - 1) / gridDim.y;
    const size_t i0 = (size_t)blockIdx.y * per;
    const size_t i1 = (i0 + per < N) ? i0 + per : N;
    double s = 0;
#pragma unroll 4
    for (size_t i = i0; i < i1; ++i) {
        const size_t o = goff + i * (size_t)degree + j;
        double t = fz_mulmod((double)vkL[o], (double)c[o], m) + (double)vkR[o];   // |t| < 2^32
        s += fz_mulmod(t, (double)alpha[o], m);
    }
    if (i1 > i0) atomic_add_i64(partial + g * pstride + j, s);
}

// zero `count` int64 at partial + g*pstride for every group (one launch instead of G memsets)
__global__ __launch_bounds__(kBlock) void zero_i64_kernel(int64_t *partial, size_t pstride, size_t count) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    int64_t *p = partial + (size_t)blockIdx.z * pstride;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) p[i] = 0;
}

__global__ __launch_bounds__(kBlock) void reduce_i64_kernel(const int64_t *in, int32_t *out, size_t count, FzMod m) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride)
        out[i] = (int)fz_cent_i64(in[i], m);         // exact for ANY int64 (sums that crossed an all-reduce)
}

// one wave per row: max |x| over stored values, #{x : x mod q != 0}
__global__ __launch_bounds__(64) void norm_weight_kernel(const int32_t *coef, size_t batch, int degree, uint32_t q,
                                                         int64_t *max_abs, int32_t *weight) {
    for (size_t row = blockIdx.x; row < batch; row += gridDim.x) {
        long long mx = 0;
        int w = 0;
        for (int j = threadIdx.x; j < degree; j += 64) {
            long long x = coef[row * (size_t)degree + j];
            long long ax = x < 0 ? -x : x;
            mx = ax > mx ? ax : mx;
            // x mod q == 0 iff |x| mod q == 0; |x| <= 2^31 fits a uint32, so one exact 32-bit remainder serves every odd
            // q < 2^32 (an unreduced multiple such as 2q or -3q of a small modulus counts as zero, as in the reference)
            w += ((uint32_t)ax % q != 0u) ? 1 : 0;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            long long o = __shfl_xor(mx, off);
            mx = o > mx ? o : mx;
            w += __shfl_xor(w, off);
        }
        if (threadIdx.x == 0) {
            max_abs[row] = mx;
            weight[row] = w;
        }
    }
}

// verdict of fusion/fusion.py:718-728, evaluated in the reference's order; one block per aggregate
__global__ __launch_bounds__(256) void verdict_kernel(const int32_t *target, const int32_t *observed, int degree,
                                                      const int64_t *max_abs, const int32_t *weight, int l,
                                                      int64_t beta, int64_t omega, int *verdict) {
    __shared__ int s_mis, s_norm, s_wt;
    const size_t g = blockIdx.x;
    target += g * degree;
    observed += g * degree;
    max_abs += g * l;
    weight += g * l;
    if (threadIdx.x == 0) { s_mis = 0; s_norm = 0; s_wt = 0; }
    __syncthreads();
    for (int j = threadIdx.x; j < degree; j += blockDim.x)
        if (target[j] != observed[j]) atomicOr(&s_mis, 1);      // both centred: equal ints <=> equal mod q
    for (int k = threadIdx.x; k < l; k += blockDim.x) {
        if (max_abs[k] > beta) atomicOr(&s_norm, 1);
        if ((int64_t)weight[k] > omega) atomicOr(&s_wt, 1);
    }
    __syncthreads();
    if (threadIdx.x == 0)
        verdict[g] = s_mis ? FZ_VERDICT_TARGET_MISMATCH : (s_norm ? FZ_VERDICT_NORM : (s_wt ? FZ_VERDICT_WEIGHT : FZ_VERDICT_OK));
}

}  // namespace

int fz_launch_pw(fz_ctx *ctx, int op, const int32_t *a, const int32_t *b, int32_t *out, size_t count) {
    if (count == 0) return FZ_OK;
    const int vec = ((((uintptr_t)a | (uintptr_t)b | (uintptr_t)out) & 15) == 0) ? 1 : 0;
    const unsigned grid = grid_for(ctx, vec ? count / 4 + 4 : count);
    auto launch = [&](auto o) {                       // FZ_OP_NEG has no second operand: it is handed `a` again
        hipLaunchKernelGGL(pw_kernel<o()>, dim3(grid), dim3(kBlock), 0, ctx->stream, a, o() == FZ_OP_NEG ? a : b, out, count, vec, ctx->mod);
    };
    switch (op) {
        case FZ_OP_MUL: launch(std::integral_constant<int, FZ_OP_MUL>()); break;
        case FZ_OP_ADD: launch(std::integral_constant<int, FZ_OP_ADD>()); break;
        case FZ_OP_SUB: launch(std::integral_constant<int, FZ_OP_SUB>()); break;
        case FZ_OP_NEG: launch(std::integral_constant<int, FZ_OP_NEG>()); break;
        case FZ_OP_MULACC: launch(std::integral_constant<int, FZ_OP_MULACC>()); break;
        default: return fz_set_error(FZ_E_BADARG, "unknown pointwise op %d", op);
    }
    return fz_check_hip(hipGetLastError(), "pointwise launch");
}

int fz_launch_pw_bcast(fz_ctx *ctx, const int32_t *a, const int32_t *s, int32_t *out, size_t rows) {
    if (rows == 0) return FZ_OK;
    const size_t total = rows * (size_t)ctx->degree;
    hipLaunchKernelGGL(pw_bcast_kernel, dim3(grid_for(ctx, total)), dim3(kBlock), 0, ctx->stream, a, s, out, total,
                       ctx->degree, ctx->mod);
    return fz_check_hip(hipGetLastError(), "pw_bcast launch");
}

int fz_launch_matvec(fz_ctx *ctx, const int32_t *A, const int32_t *S, int32_t *out, size_t batch, int l) {
    if (batch == 0) return FZ_OK;
    const bool vec = ctx->degree % 4 == 0 && ((((uintptr_t)A | (uintptr_t)S | (uintptr_t)out) & 15) == 0);   // int4 rows
    if (vec && ctx->degree >= 16 && ctx->degree <= 4096 && (ctx->degree & (ctx->degree - 1)) == 0 &&
        (ctx->knob_matvec_slices < 0 ? batch * (size_t)(ctx->degree / 4) < (size_t)ctx->num_cu * 256
                                     : ctx->knob_matvec_slices == 0 && batch <= (size_t)ctx->num_cu * 2))
        // one 1024-thread workgroup per product while all of them are resident at once (two per CU); measured on cold operands
        // (profiles/r03_matvec_ab.txt): 512 products 11.1 us against 12.0 for the sliced kernel at degree 256, 8.7 against
        // 10.5 at degree 64; 1024 products 19.3 (sliced) against 26.2 / 12.5 against 14.0
        hipLaunchKernelGGL(matvec_split_kernel, dim3((unsigned)batch), dim3(1024), 0, ctx->stream, A, S, out, l,
                           ctx->degree, ctx->mod);
    else if (vec && l <= 32768 && ctx->knob_matvec_slices >= 0) {
        // slices of the k range per column: waves for every SIMD several times over, at least 8 rows per slice
        const size_t cols = batch * (size_t)(ctx->degree / 4), waves1 = (cols + 63) / 64;
        int ks = ctx->knob_matvec_slices;                                  // FZ_MATVEC_SLICES = 1 | 2 | 4 | 8 | 16 (A/B runs), -1: the fp64 kernels
        if (ks != 1 && ks != 2 && ks != 4 && ks != 8 && ks != 16) {
            ks = 1;
            while (ks < 16 && waves1 * ks < (size_t)ctx->num_cu * 8) ks <<= 1;
        }
        while (ks > 1 && l / ks < 8) ks >>= 1;
        const int cx = ks <= 4 ? 256 / ks : 64;
        const size_t blocks = (cols + cx - 1) / cx;
        if (blocks > 0x7fffffffull) return fz_set_error(FZ_E_UNSUPPORTED, "batch too large for one matvec launch");
        const dim3 grid((unsigned)blocks), block(cx, ks);
#define FZ_MVS(K) hipLaunchKernelGGL(matvec_sliced_kernel<K>, grid, block, 0, ctx->stream, A, S, out, batch, l, ctx->degree, ctx->mod)
        if (ks == 16) FZ_MVS(16);
        else if (ks == 8) FZ_MVS(8);
        else if (ks == 4) FZ_MVS(4);
        else if (ks == 2) FZ_MVS(2);
        else FZ_MVS(1);
#undef FZ_MVS
    }
    else if (vec)
        hipLaunchKernelGGL(matvec_kernel, dim3(grid_for(ctx, batch * (size_t)(ctx->degree / 4))), dim3(kBlock), 0,
                           ctx->stream, A, S, out, batch, l, ctx->degree, ctx->mod);
    else
        hipLaunchKernelGGL(matvec_scalar_kernel, dim3(grid_for(ctx, batch * (size_t)ctx->degree)), dim3(kBlock), 0,
                           ctx->stream, A, S, out, batch, l, ctx->degree, ctx->mod);
    return fz_check_hip(hipGetLastError(), "matvec launch");
}

int fz_launch_sign(fz_ctx *ctx, const int32_t *sk_hat, const int32_t *c_hat, int32_t *sig, size_t batch, int l) {
    if (batch == 0) return FZ_OK;
    if (ctx->degree % 4 != 0 || ((((uintptr_t)sk_hat | (uintptr_t)c_hat | (uintptr_t)sig) & 15) != 0)) {
        const size_t n = batch * (size_t)l * ctx->degree;
        hipLaunchKernelGGL(sign_scalar_kernel, dim3(grid_for(ctx, n)), dim3(kBlock), 0, ctx->stream, sk_hat, c_hat, sig, batch, l,
                           ctx->degree, ctx->mod);
        return fz_check_hip(hipGetLastError(), "sign (scalar) launch");
    }
    const size_t total = batch * (size_t)l * (ctx->degree / 4);
    hipLaunchKernelGGL(sign_kernel, dim3(grid_for(ctx, total)), dim3(kBlock), 0, ctx->stream, sk_hat, c_hat, sig, batch,
                       l, ctx->degree, ctx->mod);
    return fz_check_hip(hipGetLastError(), "sign launch");
}

// out[seg][k][:] = in[seg][:] for k < l (generic-degree path of fz_keygen_core_bcast)
__global__ __launch_bounds__(kBlock) void bcast_rows_kernel(const int32_t *in, int32_t *out, size_t segments, int l, int degree) {
    const size_t total = segments * (size_t)l * degree, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride)
        out[i] = in[(i / ((size_t)l * degree)) * degree + i % degree];
}

int fz_launch_bcast_rows(fz_ctx *ctx, const int32_t *in, int32_t *out, size_t segments, int l) {
    const size_t total = segments * (size_t)l * ctx->degree;
    if (total == 0) return FZ_OK;
    hipLaunchKernelGGL(bcast_rows_kernel, dim3(grid_for(ctx, total)), dim3(kBlock), 0, ctx->stream, in, out, segments, l, ctx->degree);
    return fz_check_hip(hipGetLastError(), "bcast_rows launch");
}

// synthetic input generator ("device-side sampling for synthetic batches"): value i of the stream is
// SplitMix64(seed + (i + 1) * golden) mod q, centred -- the same sequence as the host generator the tests and the
// bench use (oracle.splitmix_centered), so device-filled and host-filled batches are interchangeable
__global__ __launch_bounds__(kBlock) void fill_synthetic_kernel(int32_t *out, size_t count, unsigned long long seed, uint32_t q) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
        unsigned long long z = seed + (unsigned long long)(i + 1) * 0x9E3779B97F4A7C15ull;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        out[i] = (int32_t)((long long)(z % q) - (long long)((q - 1) / 2));
    }
}

int fz_launch_fill_synthetic(fz_ctx *ctx, int32_t *out, size_t count, unsigned long long seed) {
    if (count == 0) return FZ_OK;
    hipLaunchKernelGGL(fill_synthetic_kernel, dim3(grid_for(ctx, count)), dim3(kBlock), 0, ctx->stream, out, count, seed, ctx->q);
    return fz_check_hip(hipGetLastError(), "fill_synthetic launch");
}

static unsigned split_count(fz_ctx *ctx, size_t N, unsigned gx, size_t groups, size_t min_per_thread) {
    // enough blocks to fill the chip (~8 per CU over all groups) but at least `min_per_thread` items each
    size_t want = ((size_t)ctx->num_cu * 8 + gx * groups - 1) / (gx * groups);
    const size_t most = (N + min_per_thread - 1) / min_per_thread;
    if (want > most) want = most;
    if (want < 1) want = 1;
    if (want > 65535) want = 65535;
    return (unsigned)want;
}

int fz_launch_target_partial(fz_ctx *ctx, const int32_t *vkL, const int32_t *vkR, const int32_t *c, const int32_t *alpha,
                             int64_t *partial, size_t pstride, size_t groups, size_t N) {
    if (groups == 0) return FZ_OK;
    hipLaunchKernelGGL(zero_i64_kernel, dim3(1, 1, (unsigned)groups), dim3(kBlock), 0, ctx->stream, partial, pstride,
                       (size_t)ctx->degree);
    int rc = fz_check_hip(hipGetLastError(), "zero target");
    if (rc != FZ_OK || N == 0) return rc;
    const unsigned gx = (unsigned)((ctx->degree + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(target_kernel, dim3(gx, split_count(ctx, N, gx, groups, 8), (unsigned)groups), dim3(kBlock), 0,
                       ctx->stream, vkL, vkR, c, alpha, partial, pstride, N, ctx->degree, ctx->mod);
    return fz_check_hip(hipGetLastError(), "target launch");
}

int fz_launch_reduce_i64(fz_ctx *ctx, const int64_t *in, int32_t *out, size_t count) {
    if (count == 0) return FZ_OK;
    hipLaunchKernelGGL(reduce_i64_kernel, dim3(grid_for(ctx, count)), dim3(kBlock), 0, ctx->stream, in, out, count, ctx->mod);
    return fz_check_hip(hipGetLastError(), "reduce_i64 launch");
}

int fz_launch_norm_weight(fz_ctx *ctx, const int32_t *coef, size_t batch, int64_t *max_abs, int32_t *weight) {
    if (batch == 0) return FZ_OK;
    size_t cap = (size_t)ctx->num_cu * 16;
    const unsigned grid = (unsigned)(batch < cap ? batch : cap);
    hipLaunchKernelGGL(norm_weight_kernel, dim3(grid), dim3(64), 0, ctx->stream, coef, batch, ctx->degree, ctx->q, max_abs, weight);
    return fz_check_hip(hipGetLastError(), "norm_weight launch");
}

int fz_launch_verdict(fz_ctx *ctx, const int32_t *target, const int32_t *observed, const int64_t *max_abs,
                      const int32_t *weight, size_t groups, int l, int64_t beta, int64_t omega, int *d_verdict) {
    hipLaunchKernelGGL(verdict_kernel, dim3((unsigned)groups), dim3(256), 0, ctx->stream, target, observed, ctx->degree, max_abs, weight,
                       l, beta, omega, d_verdict);
    return fz_check_hip(hipGetLastError(), "verdict launch");
}
