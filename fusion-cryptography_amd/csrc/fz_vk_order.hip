// fz_vk_order.hip -- the key sort of hash_ag for MANY committees ON THE DEVICE: one wave per committee.
//
// aggregate() and verify() hash a committee's keys in the order sorted(keys, key=str) (fusion/fusion.py:661-663, :693).  The text of a
// key is 11 KB, but its order is that of the first coefficient whose values differ (fz_vk_order_key.h: an integer key per
// coefficient whose plain comparison is the text's), so the sort needs no text.  A committee is sorted by COUNTING: the rank of
// row i is the number of rows that compare less plus the number of equal rows with a smaller index -- stable by construction, every
// output written once, no atomics and no scratch.  The schedule is hash_ag_wave_kernel's (fz_hash_ag.hip): W committees per
// workgroup, waves never synchronising with each other.  Per block of 64 rows i (one per lane, its first coefficient's key in two
// registers) the wave walks the committee in tiles of 64 rows j: lane t computes row jb + t's key, and the 64 keys reach every lane
// as SCALARS (v_readlane with a wave-uniform index): the inner loop is two scalar reads and a 64-bit compare, with no LDS and
// therefore no bound on the committee's size.  O(n^2 / 64) compares per lane: 124 000 for the largest committee the parameter
// sets allow (2818 signers), beside a hash chain of 100 permutations per signer.  Only rows whose FIRST coefficients are equal walk
// further coefficients (fz_vk_text_cmp, sixteen values of each row per step, from L2): identical keys, in practice.
// The second kernel splits keys [N][2][d] into their halves [N][d], [N][d] for the launches that take them apart.
#include "fz_internal.h"
#include "fz_vk_order_key.h"

namespace {

// grp[slot] = (first row, rows, first entry of `order`, -): committee `slot` owns rows x .. x + y - 1 of vk [.][2][d] and of valid
// (NULL: all), and writes its rows with valid set, sorted, to order[z ..): GLOBAL row indices.  Nothing else is written.
template <int W>
__global__ __launch_bounds__(64 * W) void vk_order_wave_kernel(const int32_t *vk, int d, const uint4 *grp, size_t G, const uint8_t *valid,
                                                               uint32_t *order) {
    const int lane = threadIdx.x & 63;
    const size_t slot = (size_t)blockIdx.x * W + (threadIdx.x >> 6);
    if (slot >= G) return;                                       // waves of a workgroup never synchronise with each other
    const uint4 g = grp[slot];
    const uint32_t first = g.x, n = g.y;
    const size_t row = (size_t)2 * d;
    const int32_t *base = vk + (size_t)first * row;
    const uint8_t *ok = valid ? valid + first : nullptr;
#pragma unroll 1
    for (uint32_t ib = 0; ib < n; ib += 64) {
        const uint32_t i = ib + lane, ic = i < n ? i : n - 1;
        const bool mine = i < n && (!ok || ok[ic]);
        const uint64_t ki = fz_vk_text_key(base[ic * row], false);
        uint32_t rank = 0;
#pragma unroll 1
        for (uint32_t jb = 0; jb < n; jb += 64) {
            const uint32_t j = jb + lane, jc = j < n ? j : n - 1;
            const uint64_t kj = fz_vk_text_key(base[jc * row], false);
            const uint32_t klo = (uint32_t)kj, khi = (uint32_t)(kj >> 32);
            unsigned long long live = __ballot(j < n && (!ok || ok[jc]));
            while (live) {                                       // (wave-uniform)
                const int t = __builtin_ctzll(live);
                live &= live - 1;
                const uint64_t k = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)klo, t) |
                                   ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)khi, t) << 32);
                const uint32_t jt = jb + (uint32_t)t;
                if (k < ki) {
                    ++rank;
                } else if (k == ki && mine && jt != i) {         // equal first coefficients: the rest of the two keys decides
                    const int c = fz_vk_text_cmp(base + jt * row, base + i * row, d);
                    rank += (c < 0 || (c == 0 && jt < i)) ? 1u : 0u;
                }
            }
        }
        if (mine) order[g.z + rank] = first + i;
    }
}

__global__ __launch_bounds__(256) void vk_halves_kernel(const int4 *vk, size_t total, int logq, int4 *left, int4 *right) {
    const size_t q = (size_t)1 << logq;                          // 16-byte units per half
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t r = e >> (logq + 1), c = e & (2 * q - 1);
        (c < q ? left : right)[r * q + (c & (q - 1))] = vk[e];
    }
}

}  // namespace

// d_vk [.][2][degree]; grp [G] uint4 (first row, rows >= 1, first entry of d_order, 0) and valid (one byte per row of d_vk, or NULL:
// all), both device-visible (pinned host memory does); d_order receives, per committee, the global indices of its rows with valid
// set in the text order of str(vk), stable.  degree: a power of two, 4..256 (the entry sees to it)
int fz_launch_vk_order(fz_ctx *ctx, const int32_t *d_vk, int degree, const void *grp, size_t G, const uint8_t *valid, uint32_t *d_order) {
    if (G == 0) return FZ_OK;
    constexpr int W = 4;
    hipLaunchKernelGGL((vk_order_wave_kernel<W>), dim3((unsigned)((G + W - 1) / W)), dim3(64 * W), 0, ctx->stream, d_vk, degree,
                       (const uint4 *)grp, G, valid, d_order);
    return fz_check_hip(hipGetLastError(), "vk order launch");
}

// d_vk [N][2][degree] -> d_left [N][degree], d_right [N][degree]; 16-byte aligned rows (degree a multiple of 4, a power of two)
int fz_launch_vk_halves(fz_ctx *ctx, const int32_t *d_vk, size_t N, int degree, int32_t *d_left, int32_t *d_right) {
    if (N == 0) return FZ_OK;
    int logq = 0;
    while ((4 << logq) < degree) ++logq;
    const size_t total = N * 2 * ((size_t)degree / 4);
    const size_t blocks = (total + 255) / 256;
    hipLaunchKernelGGL(vk_halves_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, ctx->stream, (const int4 *)d_vk, total, logq,
                       (int4 *)d_left, (int4 *)d_right);
    return fz_check_hip(hipGetLastError(), "vk halves launch");
}
