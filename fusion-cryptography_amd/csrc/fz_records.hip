// fz_records.hip -- the compact byte encoding of keys, signatures and aggregates: the records_* kernels on the chunk walk and
// the passes of the 16-per-lane transforms (fz_ntt_dev.h), their launcher and their resident-grid query.
#include "fz_records_dev.h"
#include "../../include/fusion_hip.h"

namespace {
// the format of the records, the packed chunk and its loads and stores, the field packing and unpacking, the status flag and the
// record walk: fz_records_dev.h

// encode: rows [records][rec_values] int32 -> the byte stream; status word of a record |= FZ_VERDICT_NORM where some |z| > B
template <int LOGD, bool FAST, bool COEF>
__global__ __launch_bounds__(64 * kWavesPerBlock) void records_encode(const int32_t *in, uint8_t *out, size_t total, unsigned rec_values,
                                                                      int w, int bound, int *status, const double2 *__restrict__ itwB,
                                                                      const FzTwA *tab, FzMod m) {
    constexpr int L = Geom<LOGD>::L;
    __shared__ __attribute__((aligned(16))) double lds[lds16_doubles<LOGD>()];
    const int lane = threadIdx.x & 63, p = lane / L, r = lane % L;
    const ChunkTasks T(total);
    Chunk raw0 = {};
    if (T.first < T.tasks) raw0 = chunk_load(in, T.first, total, lane);      // before the table: see fwd16_run
    const double2 *s_tw = nullptr;
    if constexpr (COEF) s_tw = twiddles_to_lds<LOGD>(lds, itwB);
    const WaveLds W = wave_lds<LOGD>(lds, T.wave, p);
    if (T.first >= T.tasks) return;
    chunk_to_lds(W.stage, lane, raw0);
    RecWalk walk(T.first, T.stride, rec_values, lane);
    const FieldBounds B(w, bound);

    auto iteration = [&](const size_t task, auto more_tag) __attribute__((always_inline)) {       // pipeline and peeling: see fwd16_run
        constexpr bool more = decltype(more_tag)::value;
        Chunk raw = {};
        if (more) raw = chunk_load(in, task + T.stride, total, lane);
        int wl = w;
        asm volatile("" : "+s"(wl));                      // what depends on w alone (the bit offsets of the packing, the stream's
        const size_t total_bytes = total / 8 * (size_t)wl;      // length) is recomputed per chunk, not held across the loop
        wave_sync();
        if constexpr (COEF) {
            double a[16];
            image_to_doubles(W.stage, lane, a);
            wave_sync();
            inv16_to_image<LOGD, FAST>(a, W, p, r, s_tw, (TabPtr)tab, m);
            wave_sync();
        }
        // the lane's 16 consecutive values: centred (the transform's outputs already are), range-checked, packed
        // |z + B| < 2^32: the high word is all ones exactly when z < -B, the low word exceeds 2B exactly when z > B
        uint32_t u[16], hi = 0, mx = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int4 t = *reinterpret_cast<const int4 *>(W.stage + pad4(16 * lane + 4 * k));
            const int v[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const long long z = COEF ? (long long)v[i] : (long long)fz_cent((double)v[i], m);
                u[4 * k + i] = range_field(z, B, hi, mx);
            }
        }
        const bool bad = hi != 0 || mx > B.two_b;
        // (fields_pack and the read-back stay written out: inside a helper the packing comes out longer, docs/HISTORY.md section V)
        fields_pack(reinterpret_cast<uint16_t *>(W.pk) + lane * wl, u, wl);
        wave_sync();
        const Packed o = packed_from_lds(W.pk, wl, lane);
        wave_sync();
        if (more) chunk_to_lds(W.stage, lane, raw);       // waits for the prefetched loads (no store is younger)
        store_and_flag(out, task, total, total_bytes, wl, lane, o, status, walk.rec, bad, FZ_VERDICT_NORM);
        walk.step();
    };
    size_t task = T.first;
    for (; task + T.stride < T.tasks; task += T.stride) iteration(task, std::true_type());
    iteration(task, std::false_type());
}

// decode: the byte stream -> rows [records][rec_values] int32 (NTT(z) for COEF, z otherwise); status |= FZ_VERDICT_ENCODING where
// some field > 2B
template <int LOGD, bool FAST, bool COEF>
__global__ __launch_bounds__(64 * kWavesPerBlock) void records_decode(const uint8_t *in, int32_t *out, size_t total, unsigned rec_values,
                                                                      int w, int bound, int *status, const double2 *__restrict__ twB,
                                                                      const FzTwA *tab, FzMod m) {
    constexpr int D = Geom<LOGD>::D, L = Geom<LOGD>::L;
    __shared__ __attribute__((aligned(16))) double lds[lds16_doubles<LOGD>()];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int p = lane / L, r = lane % L;
    const size_t tasks = (total + kChunk - 1) / kChunk;
    const size_t total_bytes = total / 8 * (size_t)w;      // (ChunkTasks' text, kept here: with the length in front of it or behind
    const size_t first = (size_t)blockIdx.x * kWavesPerBlock + wave;      // it this kernel's prologue changes, docs/HISTORY.md section V)
    const size_t stride = (size_t)gridDim.x * kWavesPerBlock;
    Packed raw0 = {};
    if (first < tasks) raw0 = packed_load(in, first, total_bytes, w, lane);
    const double2 *s_tw = nullptr;
    if constexpr (COEF) s_tw = twiddles_to_lds<LOGD>(lds, twB);
    const WaveLds W = wave_lds<LOGD>(lds, wave, p);
    if (first >= tasks) return;
    packed_to_lds(W.pk, raw0, w, lane);
    RecWalk walk(first, stride, rec_values, lane);
    const uint32_t two_b = 2u * (unsigned)bound;

    auto iteration = [&](const size_t task, auto more_tag) __attribute__((always_inline)) {       // pipeline and peeling: see fwd16_run
        constexpr bool more = decltype(more_tag)::value;
        Packed raw = {};
        if (more) raw = packed_load(in, task + stride, total_bytes, w, lane);
        wave_sync();
        uint32_t u[16];
        const bool bad = fields_to_image(W.pk, W.stage, w, (uint32_t)bound, lane, u) > two_b;
        wave_sync();
        if constexpr (COEF) {
            double a[16];
            {                                             // image_fwd16's text, kept here: its call changes this kernel's schedule
                int x[16];                                // (docs/HISTORY.md section M)
#pragma unroll
                for (int k = 0; k < 16; ++k) x[k] = W.stage[pad4(p * D + r + L * k)];
#pragma unroll
                for (int k = 0; k < 16; ++k) a[k] = (double)x[k];
            }
            wave_sync();
            TabPtr t = (TabPtr)tab;
            asm volatile("" : "+s"(t));
            fwd16_passes<LOGD, FAST>(a, W.row, r, s_tw, t[0], m);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                int4 o;
                o.x = (int)fz_cent(a[4 * k + 0], m);
                o.y = (int)fz_cent(a[4 * k + 1], m);
                o.z = (int)fz_cent(a[4 * k + 2], m);
                o.w = (int)fz_cent(a[4 * k + 3], m);
                *reinterpret_cast<int4 *>(W.stage + pad4(16 * lane + 4 * k)) = o;
            }
            wave_sync();
        }
        const int4 o0 = *reinterpret_cast<const int4 *>(W.stage + pad4(4 * lane));
        const int4 o1 = *reinterpret_cast<const int4 *>(W.stage + pad4(256 + 4 * lane));
        const int4 o2 = *reinterpret_cast<const int4 *>(W.stage + pad4(512 + 4 * lane));
        const int4 o3 = *reinterpret_cast<const int4 *>(W.stage + pad4(768 + 4 * lane));
        wave_sync();
        if (more) packed_to_lds(W.pk, raw, w, lane);      // waits for the prefetched loads (no store is younger)
        chunk_store(out, task, total, lane, o0, o1, o2, o3);
        const bool valid = task * kChunk + 16 * lane < total;
        records_flag(status, walk.rec, bad && valid, FZ_VERDICT_ENCODING, lane);
        walk.step();
    };
    size_t task = first;
    for (; task + stride < tasks; task += stride) iteration(task, std::true_type());
    iteration(task, std::false_type());
}

// the follow-up of both: a record whose status word is set gets all-zero output (bytes or rows), so what a launch leaves is a
// function of its input alone.  Records are 8-byte multiples; a workgroup per record, striding.
__global__ __launch_bounds__(256) void records_zero_failed(const int *status, size_t n, uint8_t *dst, size_t rec_bytes) {
    for (size_t rec = blockIdx.x; rec < n; rec += gridDim.x) {
        if (status[rec] == 0) continue;
        fz_v2i *p = reinterpret_cast<fz_v2i *>(dst + rec * rec_bytes);
        const fz_v2i zero = {0, 0};
        for (size_t i = threadIdx.x; i < rec_bytes / 8; i += blockDim.x) p[i] = zero;
    }
}

}  // namespace

// compact byte encoding (fz_encode_records_async / fz_decode_records_async): the records kernel over the batch as a
// fz_records_pass.  Verification keys (no transform) take one instantiation.  The grid is capped at the kernel's OWN resident grid
// (fz_records_query_grid), as launch16f caps the transforms at theirs: the FAST encode holds more registers than ntt_inv16 (3
// workgroups per CU against 4), and a grid sized for the transform would leave a quarter of its workgroups for a second round of
// the grid-stride walk.
template <int LOGD, bool FAST, bool COEF>
static void launch_records_k(fz_ctx *ctx, bool decode, const void *src, void *dst, size_t total, unsigned rv, int w, int bound,
                             int *d_status) {
    const dim3 grid = chunk_grid(total, ctx->grid_rec[(decode ? 1 : 0) + (COEF ? 0 : 2)]), block(64 * kWavesPerBlock);
    if (decode)
        hipLaunchKernelGGL((records_decode<LOGD, FAST, COEF>), grid, block, 0, ctx->stream, (const uint8_t *)src, (int32_t *)dst, total, rv,
                           w, bound, d_status, (const double2 *)ctx->d_twB, (const FzTwA *)ctx->d_twAB, ctx->mod);
    else
        hipLaunchKernelGGL((records_encode<LOGD, FAST, COEF>), grid, block, 0, ctx->stream, (const int32_t *)src, (uint8_t *)dst, total, rv,
                           w, bound, d_status, (const double2 *)ctx->d_itwB, (const FzTwA *)ctx->d_twAB + 1, ctx->mod);
}

// resident grids of the records kernels this context launches: [encode, decode] x [coefficient kinds, keys]
template <int LOGD, bool FAST>
static int query_records(fz_ctx *ctx) {
    const void *k[4] = {(const void *)records_encode<LOGD, FAST, true>, (const void *)records_decode<LOGD, FAST, true>,
                        (const void *)records_encode<8, true, false>, (const void *)records_decode<8, true, false>};
    int rc = FZ_OK;
    for (int i = 0; i < 4 && rc == FZ_OK; ++i) rc = fz_resident_grid(ctx, k[i], 64 * kWavesPerBlock, "occupancy query (records)", &ctx->grid_rec[i]);
    return rc;
}

int fz_records_query_grid(fz_ctx *ctx) {
    return fz_dispatch<6, 8>(ctx, FZ_OK, [&](auto logd, auto fast) { return query_records<logd(), fast()>(ctx); });
}

int fz_launch_records(fz_ctx *ctx, bool decode, const void *src, void *dst, size_t n, int rows, bool coef, int w, int64_t bound,
                      int *d_status) {
    const unsigned rv = (unsigned)rows * (unsigned)ctx->degree;
    const size_t total = n * rv;
    const int b = (int)bound;
    const auto launch = [&]() {
        if (coef)
            return fz_dispatch<6, 8>(ctx, FZ_E_UNSUPPORTED, [&](auto logd, auto fast) {
                launch_records_k<logd(), fast(), true>(ctx, decode, src, dst, total, rv, w, b, d_status);
                return FZ_OK;
            });
        launch_records_k<8, true, false>(ctx, decode, src, dst, total, rv, w, b, d_status);
        return (int)FZ_OK;
    };
    return fz_records_pass(ctx, d_status, n, "records launch", launch, dst,
                           decode ? (size_t)rv * sizeof(int32_t) : fz_record_bytes(ctx->degree, rows, w));
}

int fz_launch_records_zero(fz_ctx *ctx, const int *d_status, size_t n, void *dst, size_t rec_bytes) {
    const size_t zcap = (size_t)ctx->num_cu * 4;
    hipLaunchKernelGGL(records_zero_failed, dim3((unsigned)(n < zcap ? n : zcap)), dim3(256), 0, ctx->stream, d_status, n, (uint8_t *)dst,
                       rec_bytes);
    return fz_check_hip(hipGetLastError(), "records zeroing launch");
}
