// fz_keygen_records.hip -- key generation straight to compact "secret" records: the secret polynomials
// are range-checked and packed as they are read, their transform serves the verification key alone, and no int32 row of the
// key ever reaches memory.  keygen_records_bcast (one polynomial per (key, half), the scheme's seeded keys: a resident grid
// that sums A once per workgroup and then walks the (key, half) units) and keygen_records_rows (l polynomials per (key, half):
// keygen_fused with the row's fields packed instead of its transform stored); their launcher and the resident-grid query
// (the entry fz_keygen_records_async: fz_records_capi.hip).  Both kernels stand on the radix-4 structure of keygen_bcast_fused / keygen_fused
// (fz_scheme_fused.hip) and take its LDS: a 2 KiB transform region per wave and 8 KiB where the workgroup's waves meet.
#include "fz_records_dev.h"
#include "../../include/fusion_hip.h"

namespace {

// A wave's region once its transform is done: the fields of its 256 values (64 / (D/4) polynomials of D) in natural order as
// an int32 image in the first KiB, their packed form (32 wk <= 992 bytes: polynomial p's row at p * D / 8 * wk) in the second.
constexpr int kFieldImageBytes = 1024;

// the image -> the packed rows: lanes 0 .. 15 take 16 consecutive fields each, i.e. wk 16-bit words (fields_pack).  A polynomial
// is a multiple of 16 values, so no lane straddles two.
__device__ __forceinline__ void image_pack(uint8_t *region, int wk, int lane) {
    if (lane < 16) {
        uint32_t u[16];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int4 t = *reinterpret_cast<const int4 *>(region + 64 * lane + 16 * k);
            u[4 * k + 0] = (uint32_t)t.x;
            u[4 * k + 1] = (uint32_t)t.y;
            u[4 * k + 2] = (uint32_t)t.z;
            u[4 * k + 3] = (uint32_t)t.w;
        }
        fields_pack(reinterpret_cast<uint16_t *>(region + kFieldImageBytes) + lane * wk, u, wk);
    }
}

// a lane's 4 coefficients (any int32) -> s = cent(x mod q) and their fields s + B in f; the range check's two halves move on
__device__ __forceinline__ void coef_fields(const int (&x)[4], const FieldBounds &B, const FzMod &m, uint32_t (&f)[4], uint32_t &hi,
                                            uint32_t &mx) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long long s = (long long)(int)fz_cent((double)x[k], m);      // |x| < 2^31 is inside fz_cent's bound; |s| <= (q-1)/2
        f[k] = range_field(s, B, hi, mx);
    }
}

// `bytes` bytes at dst (both multiples of 8; dst 8-byte aligned and no more) = the packed row of rb bytes at `row` (LDS, a multiple
// of 8 bytes) repeated: an 8-byte store in front where dst is 8 mod 16, 16-byte streaming stores from there on, an 8-byte store
// behind them where 8 bytes are left.  A 16-byte unit may wrap around the row's end (rb is 8 mod 16 when D / 8 * wk is): its
// two halves are read on their own.  pos = the unit's place in the row, stepped by 1024 mod rb per round of the wave.
__device__ __forceinline__ void row_stream(uint8_t *dst, size_t bytes, const uint8_t *row, unsigned rb, unsigned step, int lane) {
    const unsigned head = (unsigned)(reinterpret_cast<uintptr_t>(dst) & 8);
    if (head && lane == 0) {
        const fz_v2i t = *reinterpret_cast<const fz_v2i *>(row);
        __builtin_nontemporal_store(t, reinterpret_cast<fz_v2i *>(dst));
    }
    const size_t body = (bytes - head) >> 4;
    uint8_t *d16 = dst + head;
    unsigned pos = (head + 16u * (unsigned)lane) % rb;
    for (size_t i = (size_t)lane; i < body; i += 64) {
        unsigned p2 = pos + 8;
        if (p2 >= rb) p2 -= rb;
        const fz_v2i lo = *reinterpret_cast<const fz_v2i *>(row + pos), hi = *reinterpret_cast<const fz_v2i *>(row + p2);
        fz_v4i t = {lo.x, lo.y, hi.x, hi.y};
        __builtin_nontemporal_store(t, reinterpret_cast<fz_v4i *>(d16 + 16 * i));
        pos += step;
        if (pos >= rb) pos -= rb;
    }
    if (((bytes - head) & 8) && lane == 63) {                 // the last 8 bytes of a stream of whole rows are a row's last
        const fz_v2i t = *reinterpret_cast<const fz_v2i *>(row + rb - 8);
        __builtin_nontemporal_store(t, reinterpret_cast<fz_v2i *>(dst + bytes - 8));
    }
}

// One polynomial per (key, half) (the reference's seeded keys: fusion.py:156-173).  A workgroup first sums the l rows of A in
// integers -- once, whatever number of units it goes on to walk -- and centres the sums: a lane keeps the four that meet its
// outputs.  A wave-task is then 64 / (D/4) consecutive units (key, half) = seg: the lane (p, mm) reads coefficients mm + (D/4) k
// of unit task * PPW + p, makes their fields and range-checks them, transforms (for vk alone: vk = cent((sum A) (.) FWD(s)),
// keygen_bcast_fused's arithmetic with the sum taken whole), and the wave packs each unit's row once and streams it out l times.
// Units past the end (a ragged last task at degree 64) read unit 0, store nothing and flag nothing.
template <int LOGD, bool FAST>
__global__ __launch_bounds__(64 * kWavesPerBlock) void keygen_records_bcast(const int32_t *A, const int32_t *coef, uint8_t *out, int32_t *vk,
                                                                            int *status, size_t units, int l, int wk, int key_bound,
                                                                            const double2 *__restrict__ tw2, FzTwA twA, FzMod m) {
    constexpr int D = 1 << LOGD, LP = D / 4, PPW = 64 / LP;
    __shared__ __attribute__((aligned(16))) double lds[kWavesPerBlock * 256 * 2];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int p = lane / LP, mm = lane % LP;
    double *wregion = lds + wave * 256;
    double *region = wregion + p * D;
    double2 twl[LOGD / 2 - 1][3];
    fwd4_load_twiddles<LOGD, double2>(twl, tw2, mm);

    // sum_k A_k, the rows this lane's row slot covers first (|A| <= 2^31, l < 2^31 rows: no overflow of int64)
    double asc[4];
    {
        long long *accbuf = reinterpret_cast<long long *>(lds + kWavesPerBlock * 256);
        long long asum[4] = {0, 0, 0, 0};
        for (int row = wave * PPW + p; row < l; row += kWavesPerBlock * PPW) {
            const int4 ak = *reinterpret_cast<const int4 *>(A + (size_t)row * D + 4 * mm);
            asum[0] += ak.x; asum[1] += ak.y; asum[2] += ak.z; asum[3] += ak.w;
        }
        long long *mine = accbuf + wave * 256 + p * D + 4 * mm;
#pragma unroll
        for (int k = 0; k < 4; ++k) mine[k] = asum[k];
        __syncthreads();
        long long sum = 0;
        if (threadIdx.x < D) {
#pragma unroll
            for (int w = 0; w < kWavesPerBlock; ++w)
#pragma unroll
                for (int q = 0; q < PPW; ++q) sum += accbuf[w * 256 + q * D + threadIdx.x];
        }
        __syncthreads();
        double *total = lds + kWavesPerBlock * 256;
        if (threadIdx.x < D) total[threadIdx.x] = fz_cent_i64(sum, m);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) asc[k] = total[4 * mm + k];
    }

    const FieldBounds B(wk, key_bound);
    const unsigned rb = (unsigned)(D / 8) * (unsigned)wk, step = 1024u % rb;
    const size_t half_bytes = (size_t)l * rb;
    const size_t tasks = (units + PPW - 1) / PPW;
    uint8_t *bytes = reinterpret_cast<uint8_t *>(wregion);
    for (size_t task = (size_t)blockIdx.x * kWavesPerBlock + wave; task < tasks; task += (size_t)gridDim.x * kWavesPerBlock) {
        const size_t seg = task * PPW + p;
        const bool valid = seg < units;
        const int32_t *src = coef + (valid ? seg : (size_t)0) * D + mm;
        int x[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = __builtin_nontemporal_load(src + k * LP);
        uint32_t f[4], hi = 0, mx = 0;
        coef_fields(x, B, m, f, hi, mx);
        const bool bad = hi != 0 || mx > B.two_b;
        double a[1][4];
#pragma unroll
        for (int k = 0; k < 4; ++k) a[0][k] = (double)x[k];
        wave_sync();                                      // the rows of the task before have been read out of the region
        fwd4_passes_n<LOGD, FAST, 1, double2>(a, region, twl, twA, m, mm);
        if (valid) {
            int4 v;
            v.x = (int)fz_cent(fz_mulmod(asc[0], (double)(int)fz_cent(a[0][0], m), m), m);
            v.y = (int)fz_cent(fz_mulmod(asc[1], (double)(int)fz_cent(a[0][1], m), m), m);
            v.z = (int)fz_cent(fz_mulmod(asc[2], (double)(int)fz_cent(a[0][2], m), m), m);
            v.w = (int)fz_cent(fz_mulmod(asc[3], (double)(int)fz_cent(a[0][3], m), m), m);
            *reinterpret_cast<int4 *>(vk + seg * D + 4 * mm) = v;
        }
        wave_sync();                                      // the transform has read the region: the fields' image now
#pragma unroll
        for (int k = 0; k < 4; ++k) reinterpret_cast<uint32_t *>(bytes)[p * D + mm + k * LP] = f[k];
        wave_sync();
        image_pack(bytes, wk, lane);
        wave_sync();
#pragma unroll
        for (int u = 0; u < PPW; ++u) {
            const size_t sg = task * PPW + u;             // uniform
            if (sg < units)
                row_stream(out + (sg >> 1) * (2 * half_bytes) + (sg & 1) * half_bytes, half_bytes, bytes + kFieldImageBytes + u * rb, rb, step,
                           lane);
        }
        records_flag(status, seg >> 1, bad && valid, FZ_VERDICT_NORM, lane);
    }
}

// l polynomials per (key, half), a workgroup per (key, half) as keygen_fused: per row the fields are made and range-checked
// before the transform, the transformed row is multiplied by its row of A and the canonical products are summed in integers
// (exact for every l), and the packed rows of a wave's task -- consecutive rows of the half -- go out as one run of 8-byte
// stores.  The waves' sums meet in LDS as keygen_fused's do.
template <int LOGD, bool FAST>
__global__ __launch_bounds__(64 * kWavesPerBlock) void keygen_records_rows(const int32_t *A, const int32_t *coef, uint8_t *out, int32_t *vk,
                                                                           int *status, int l, int wk, int key_bound,
                                                                           const double2 *__restrict__ tw2, FzTwA twA, FzMod m) {
    constexpr int D = 1 << LOGD, LP = D / 4, PPW = 64 / LP;
    __shared__ __attribute__((aligned(16))) double lds[kWavesPerBlock * 256 * 2];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int p = lane / LP, mm = lane % LP;
    double *wregion = lds + wave * 256;
    double *region = wregion + p * D;
    long long *accbuf = reinterpret_cast<long long *>(lds + kWavesPerBlock * 256);
    const size_t seg = blockIdx.x;                        // (key, half)
    coef += seg * (size_t)l * D;
    double2 twl[LOGD / 2 - 1][3];
    fwd4_load_twiddles<LOGD, double2>(twl, tw2, mm);

    const FieldBounds B(wk, key_bound);
    const unsigned rb = (unsigned)(D / 8) * (unsigned)wk;
    uint8_t *bytes = reinterpret_cast<uint8_t *>(wregion);
    uint8_t *half = out + (seg >> 1) * (2 * (size_t)l * rb) + (seg & 1) * ((size_t)l * rb);
    long long acc[4] = {0, 0, 0, 0};
    uint32_t hi = 0, mx = 0;
    const int tasks = (l + PPW - 1) / PPW;
    for (int task = wave; task < tasks; task += kWavesPerBlock) {
        const int row = task * PPW + p;
        const bool valid = row < l;
        const size_t rowc = (size_t)(valid ? row : l - 1);
        const int32_t *src = coef + rowc * D + mm;
        int x[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = __builtin_nontemporal_load(src + k * LP);
        const int4 ak = *reinterpret_cast<const int4 *>(A + rowc * D + 4 * mm);
        uint32_t f[4], h1 = 0, m1 = 0;
        coef_fields(x, B, m, f, h1, m1);
        if (valid) {
            hi |= h1;
            mx = max(mx, m1);
        }
        double a[1][4];
#pragma unroll
        for (int k = 0; k < 4; ++k) a[0][k] = (double)x[k];
        wave_sync();
        fwd4_passes_n<LOGD, FAST, 1, double2>(a, region, twl, twA, m, mm);
        if (valid) {
            const int av[4] = {ak.x, ak.y, ak.z, ak.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] += (long long)(int)fz_cent(fz_mulmod(fz_cent(a[0][k], m), (double)av[k], m), m);
        }
        wave_sync();
#pragma unroll
        for (int k = 0; k < 4; ++k) reinterpret_cast<uint32_t *>(bytes)[p * D + mm + k * LP] = f[k];
        wave_sync();
        image_pack(bytes, wk, lane);
        wave_sync();
        const int left = l - task * PPW;
        const unsigned words = (unsigned)(left < PPW ? left : PPW) * (rb >> 3);
        uint8_t *dst = half + (size_t)task * PPW * rb;
        for (unsigned i = (unsigned)lane; i < words; i += 64) {
            const fz_v2i t = *reinterpret_cast<const fz_v2i *>(bytes + kFieldImageBytes + 8 * i);
            __builtin_nontemporal_store(t, reinterpret_cast<fz_v2i *>(dst + 8 * (size_t)i));
        }
    }
    records_flag(status, seg >> 1, hi != 0 || mx > B.two_b, FZ_VERDICT_NORM, lane);
    long long *mine = accbuf + wave * 256 + p * D + 4 * mm;
#pragma unroll
    for (int k = 0; k < 4; ++k) mine[k] = acc[k];
    __syncthreads();
    if (threadIdx.x < D) {
        long long sum = 0;
#pragma unroll
        for (int w = 0; w < kWavesPerBlock; ++w)
#pragma unroll
            for (int q = 0; q < PPW; ++q) sum += accbuf[w * 256 + q * D + threadIdx.x];
        vk[seg * D + threadIdx.x] = (int)fz_cent_i64(sum, m);
    }
}

}  // namespace

// the seeded kernel's own resident grid (context creation; degrees 64 / 256, nothing to query at the others)
int fz_keygen_records_query_grid(fz_ctx *ctx) {
    return fz_dispatch<6, 8>(ctx, FZ_OK, [&](auto logd, auto fast) {
        return fz_resident_grid(ctx, keygen_records_bcast<logd(), fast()>, 64 * kWavesPerBlock, "occupancy query (keygen_records)",
                                &ctx->grid_keyrec);
    });
}

// fz_keygen_records_async: either kernel over the batch as a fz_records_pass
int fz_launch_keygen_records(fz_ctx *ctx, const int32_t *A, const int32_t *coef, bool rows, size_t n, int l, int wk, int64_t key_bound,
                             uint8_t *d_bytes, int32_t *d_vk, int *d_status) {
    const size_t units = 2 * n;
    const dim3 block(64 * kWavesPerBlock);
    const auto launch = [&]() {
        return fz_dispatch<6, 8>(ctx, FZ_E_UNSUPPORTED, [&](auto logd, auto fast) {
            constexpr int LOGD = logd();
            if (rows) {
                hipLaunchKernelGGL((keygen_records_rows<LOGD, fast()>), dim3((unsigned)units), block, 0, ctx->stream, A, coef, d_bytes, d_vk,
                                   d_status, l, wk, (int)key_bound, (const double2 *)ctx->d_tw2, ctx->twA, ctx->mod);
            } else {
                constexpr size_t per_block = (size_t)kWavesPerBlock * (64 / ((1 << LOGD) / 4));      // units of a workgroup's round
                const size_t blocks = (units + per_block - 1) / per_block, cap = (size_t)(ctx->grid_keyrec > 0 ? ctx->grid_keyrec : 1);
                hipLaunchKernelGGL((keygen_records_bcast<LOGD, fast()>), dim3((unsigned)(blocks < cap ? blocks : cap)), block, 0, ctx->stream,
                                   A, coef, d_bytes, d_vk, d_status, units, l, wk, (int)key_bound, (const double2 *)ctx->d_tw2, ctx->twA,
                                   ctx->mod);
            }
            return FZ_OK;
        });
    };
    return fz_records_pass(ctx, d_status, n, "keygen_records launch", launch, d_bytes, fz_record_bytes(ctx->degree, 2 * l, wk));
}
