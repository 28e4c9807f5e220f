// fz_sign_records.hip -- signing straight from compact secret-key records to compact signature records:
// sign_records unpacks the two halves of a chunk of the key, transforms the left half, multiplies by the challenge, transforms
// back, adds the right half in the coefficient domain, range-checks and packs, so that no int32 row of the key or of the
// signature ever reaches memory; its launcher and its resident-grid query.
#include "fz_records_dev.h"
#include "../../include/fusion_hip.h"

namespace {

// Where a lane's 16 key fields lie.  A "secret" record is [2][rv] fields of wk bits, left half first; a lane owns 16 consecutive
// values of the output chunk, which never straddle a record or a polynomial, so its 16 fields of either half are wk 16-bit words
// = 2 wk bytes that start at a multiple of 2 wk bytes of the half.  The halves (rv / 8 * wk bytes, rv a multiple of 64) and the
// records begin on multiples of 4 bytes, so the words are 2-byte aligned and no more when wk is odd.  They are read as the
// (wk + 1) / 2 ALIGNED dwords that cover them: `p` is the first of these, `h` (0 or 1) the 16-bit words of it in front of the
// lane's own.  The covering dwords end where the half ends at the latest (its end is 4-byte aligned), so nothing past the key
// bytes is read.
struct KeyAddr {
    const uint8_t *p;
    unsigned h;
};
__device__ __forceinline__ KeyAddr key_addr(const uint8_t *key, size_t rec, unsigned off, unsigned rv, int wk) {
    const size_t g = (size_t)(off >> 4) * (size_t)wk;              // the lane's first 16-bit word of the half
    return {key + rec * ((size_t)(rv >> 2) * (size_t)wk) + 2 * (g & ~(size_t)1), (unsigned)(g & 1)};
}
__device__ __forceinline__ size_t key_half_bytes(unsigned rv, int wk) { return (size_t)(rv >> 3) * (size_t)wk; }

// the covering dwords of a lane's LEFT fields straight into LDS: dword i of lane `lane` lands at word 64 i + lane of `land` (one
// global_load_lds_dword per i: 256 bytes per wave instruction, the lanes' words side by side, which is what the instruction
// does).  One LDS base and the dword's place as the instruction offset (a base per dword costs sixteen scalar registers); the
// offset advances the global address as well, so that one is handed over 252 i bytes short -- as an integer: see sign_encode's
// key_request.  No register is held while the words are in flight; the reader waits itself (chunk_landed).  ndw = (wk + 1) / 2
// <= 16: the 4 KiB landing area.  Streaming loads: a key is read once.
__device__ __forceinline__ void key_request_lds(const KeyAddr &ka, int ndw, int32_t *land) {
    typedef const __attribute__((address_space(1))) void *gptr;
    typedef __attribute__((address_space(3))) void *lptr;
    const lptr l = (lptr)land;
    static_for<16>([&](auto i_tag) __attribute__((always_inline)) {
        constexpr int i = decltype(i_tag)::value;
        const gptr g = (gptr)(reinterpret_cast<uintptr_t>(ka.p) - (uintptr_t)(252 * i));
        if (i < ndw) __builtin_amdgcn_global_load_lds(g, l, 4, 256 * i, 2);      // aux 2: nt
    });
}

// the covering dwords of a lane's RIGHT fields into registers (the landing area is taken while they are in flight); only the
// first ndw are touched, here and below
struct KeyWords { uint32_t d[16]; };
__device__ __forceinline__ void key_request(const KeyAddr &ka, size_t half_bytes, int ndw, KeyWords &k) {
    typedef const __attribute__((address_space(1))) uint32_t *gptr;
    const gptr p = (gptr)reinterpret_cast<uintptr_t>(ka.p + half_bytes);
#pragma unroll
    for (int i = 0; i < 16; ++i)
        if (i < ndw) k.d[i] = __builtin_nontemporal_load(p + i);
}
// ... and into the layout the left ones land in (the count pinned anew: compared once for both, the sixteen outcomes wait in
// scalar registers across the strided pass)
__device__ __forceinline__ void key_to_lds(int32_t *land, int lane, int ndw, const KeyWords &k) {
    asm volatile("" : "+s"(ndw));
#pragma unroll
    for (int i = 0; i < 16; ++i)
        if (i < ndw) land[64 * i + lane] = (int32_t)k.d[i];
}

// a lane's 16 fields out of its covering dwords in the landing area: fields_unpack with 16-bit word o of the lane taken from
// word o + h of its dwords.  The misalignment is taken out here, at the LDS read; 16-bit reads of words that lie in the lane's own
// bank (dword i of lane at bank `lane`): no conflicts.  Exactly wk words are read.  -> the lane's largest field.
__device__ __forceinline__ uint32_t key_unpack(const int32_t *land, int lane, unsigned h, int wk, uint32_t (&u)[16]) {
    const uint8_t *base = reinterpret_cast<const uint8_t *>(land) + 4 * lane;
    const unsigned long long mask = (1ull << wk) - 1;
    unsigned long long acc = 0;
    int nb = 0, o = 0;
    uint32_t mx = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
#pragma unroll
        for (int e = 0; e < 2; ++e)
            if (nb < wk) {
                const unsigned x = (unsigned)(o++) + h;
                acc |= (unsigned long long)*reinterpret_cast<const uint16_t *>(base + (x >> 1) * 256 + (x & 1) * 2) << nb;
                nb += 16;
            }
        u[k] = (uint32_t)(acc & mask);
        mx = max(mx, u[k]);
        acc >>= wk;
        nb -= wk;
    }
    return mx;
}

// sign from records and encode: the byte stream of the signatures [N][l][D] of the key records [N][2][l][D] (wk-bit fields,
// bound kb) under c_hat [N][D]:  z = cent(INV(cent(FWD(sL) (.) c)) + sR).  Status word of a record |= FZ_VERDICT_ENCODING where
// some field of its key is above 2 kb, |= FZ_VERDICT_NORM where some |z| > B (4 | 6 == 6: the encoding comes first).
// A wave-task is one 1024-value chunk of the OUTPUT stream, as in sign_encode: lane `lane` = (p, r) owns values 16 lane ..
// 16 lane + 15 of it, which are outputs 16 r .. of polynomial p after the forward passes, inputs 16 r .. of the inverse passes and
// the lane's fields of the packed chunk -- the product with the challenge needs no exchange.  An iteration (1) transforms the
// image of the left half, (2) multiplies by the lane's 16 challenge words, (3) transforms back up to the transpose, (4) requests
// this chunk's right fields into registers and the NEXT chunk's left fields into the landing area (inv16_passes' hook: the region
// is free from there until the fields are packed), (5) runs the strided pass and centres into the image, (6) takes its 16
// values back, (7) waits, unpacks the next chunk's left fields into the image, (8) puts the right fields where the left ones
// were, unpacks, adds, centres and range-checks, (9) packs into the same area and stores.  The last iteration is peeled off.
// The per-lane twiddles of the inverse's contiguous pass are in LDS, those of the forward's come from memory (L2): the LDS is
// that of the transforms, which has room for one table.
// A non-canonical key record cannot fault: u - kb is just an integer, nothing is indexed by it.
template <int LOGD, bool FAST>
__global__ __launch_bounds__(64 * kWavesPerBlock) void sign_records(const uint8_t *key, const int32_t *c_hat, uint8_t *out, size_t total,
                                                                    unsigned rec_values, int wk, int key_bound, int w, int bound,
                                                                    int *status, const double2 *__restrict__ twB,
                                                                    const double2 *__restrict__ itwB, const FzTwA *tabs, FzMod m) {
    constexpr int D = Geom<LOGD>::D, L = Geom<LOGD>::L;
    __shared__ __attribute__((aligned(16))) double lds[lds16_doubles<LOGD>()];
    const int lane = threadIdx.x & 63, p = lane / L, r = lane % L;
    const ChunkTasks T(total);
    // what only the lanes' own address arithmetic uses: VALU operands, out of the scalar file (see RecWalk) -- and the walk's
    // own counters with them: two transforms' tables pass through the scalar file per chunk, and what is live across both is
    // saved around each
    asm volatile("" : "+v"(key), "+v"(c_hat), "+v"(status), "+v"(twB), "+v"(out), "+v"(total));
    RecWalk walk(T.first, T.stride, rec_values, lane);
    const WaveLds W = wave_lds<LOGD>(lds, T.wave, p);
    unsigned kb = (unsigned)key_bound, two_kb = 2u * (unsigned)key_bound;
    asm volatile("" : "+v"(kb), "+v"(two_kb));
    // the lane's fields of a chunk it has no value in (a ragged last chunk's) are the batch's first: read, transformed in
    // polynomials of their own, never stored and never flagged
    unsigned h0 = 0;
    if (T.first < T.tasks) {                              // before the table: see fwd16_run
        const bool in = T.first * kChunk + 16 * lane < total;
        const KeyAddr ka = key_addr(key, in ? walk.rec : (size_t)0, in ? walk.off : 0u, walk.rv, wk);
        h0 = ka.h;
        key_request_lds(ka, (wk + 1) >> 1, W.land);
    }
    const double2 *s_tw = twiddles_to_lds<LOGD>(lds, itwB);
    if (T.first >= T.tasks) return;
    // the left fields -> the image (chunk_to_lds' layout), -> is one of them above 2 kb?
    auto left_image = [&](unsigned h, int wkl) __attribute__((always_inline)) {
        uint32_t u[16];
        const uint32_t mx = key_unpack(W.land, lane, h, wkl, u);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int4 t;
            t.x = (int)(u[4 * k + 0] - kb);
            t.y = (int)(u[4 * k + 1] - kb);
            t.z = (int)(u[4 * k + 2] - kb);
            t.w = (int)(u[4 * k + 3] - kb);
            *reinterpret_cast<int4 *>(W.stage + pad4(16 * lane + 4 * k)) = t;
        }
        return mx;
    };
    chunk_landed<0>();
    uint32_t key_mx = left_image(h0, wk);                 // the largest key field of the lane's 16 values: a register, not a lane mask
    const FieldBounds B(w, bound);

    auto iteration = [&](const size_t task, auto more_tag) __attribute__((always_inline)) {
        constexpr bool more = decltype(more_tag)::value;
        int wl = w, wkl = wk;
        asm volatile("" : "+s"(wl), "+s"(wkl));           // recomputed per chunk, not held across the loop: see records_encode
        const size_t total_bytes = total / 8 * (size_t)wl;
        const int ndw = (wkl + 1) >> 1;
        // (recomputed where it is used: held across the transforms a lane mask is two scalar registers)
        auto is_valid = [&]() __attribute__((always_inline)) { return task * kChunk + 16 * lane < total; };
        KeyWords right;
        unsigned hn = 0, hc = 0;
        int v[16];
        {
            // the lane's 16 challenge words: outputs 16 r .. of the signer's polynomial (L2: shared by the signer's l rows)
            int4 c[4];
            {
                const bool valid = is_valid();
                const int32_t *pc = c_hat + (valid ? walk.rec : (size_t)0) * D + ((valid ? walk.off : 0u) & (unsigned)(D - 1));
#pragma unroll
                for (int k = 0; k < 4; ++k) c[k] = *reinterpret_cast<const int4 *>(pc + 4 * k);
            }
            // the image is complete (every lane's writes of it, by the preamble or the iteration before), and the reads of
            // `land` that made it have retired: in a wave's FIRST iteration those are the preamble's left_image, which has
            // just unpacked the landing area that the forward transpose is about to overwrite
            wave_sync();
            double a[16];
            image_fwd16<LOGD, FAST>(W.stage, a, W.row, p, r, twB, tabs, m);
            {
                // |a| < 2^38 times any int32 is inside fz_mulmod's bound; made canonical: an input the inverse accepts
                const int x[16] = {c[0].x, c[0].y, c[0].z, c[0].w, c[1].x, c[1].y, c[1].z, c[1].w,
                                   c[2].x, c[2].y, c[2].z, c[2].w, c[3].x, c[3].y, c[3].z, c[3].w};
#pragma unroll
                for (int k = 0; k < 16; ++k) a[k] = fz_cent(fz_mulmod(a[k], (double)x[k], m), m);
            }
            wave_sync();
            inv16_to_image<LOGD, FAST>(a, W, p, r, s_tw, (TabPtr)tabs + 1, m, [&]() __attribute__((always_inline)) {
                const bool valid = is_valid();
                const KeyAddr ka = key_addr(key, valid ? walk.rec : (size_t)0, valid ? walk.off : 0u, walk.rv, wkl);
                hc = ka.h;
                key_request(ka, key_half_bytes(walk.rv, wkl), ndw, right);
                if constexpr (more) {
                    const RecPos n = walk.next();
                    const bool in = (task + T.stride) * kChunk + 16 * lane < total;
                    const KeyAddr kn = key_addr(key, in ? n.rec : (size_t)0, in ? n.off : 0u, walk.rv, wkl);
                    hn = kn.h;
                    key_request_lds(kn, ndw, W.land);
                }
            });
            if constexpr (more) wave_sync_inflight();     // not a wait for the words in flight
            else wave_sync();
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int4 t = *reinterpret_cast<const int4 *>(W.stage + pad4(16 * lane + 4 * k));
            v[4 * k + 0] = t.x;
            v[4 * k + 1] = t.y;
            v[4 * k + 2] = t.z;
            v[4 * k + 3] = t.w;
        }
        uint32_t next_mx = 0;
        if constexpr (more) {
            wave_sync_inflight();                         // the image has been read: it is the next chunk's now
            chunk_landed<0>();
            next_mx = left_image(hn, wkl);
        }
        wave_sync();                                      // the landing area has been read: the right fields' now
        key_to_lds(W.land, lane, ndw, right);
        wave_sync();
        // z = cent(INV(..) + sR): |.| < 2^32 is inside fz_cent's bound whatever the field held.  Range-checked, packed
        uint32_t u[16], hi = 0, mx = 0;
        {
            uint32_t ur[16];
            key_mx = max(key_mx, key_unpack(W.land, lane, hc, wkl, ur));
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const long long z = (int)fz_cent((double)v[k] + (double)(int)(ur[k] - kb), m);
                u[k] = range_field(z, B, hi, mx);
            }
        }
        const bool bad = hi != 0 || mx > B.two_b;
        wave_sync();                                      // the landing area has been read: it is the packed chunk's now
        // (fields_pack and the read-back stay written out: inside a helper the packing comes out longer, docs/HISTORY.md section V)
        fields_pack(reinterpret_cast<uint16_t *>(W.pk) + lane * wl, u, wl);
        wave_sync();
        const Packed o = packed_from_lds(W.pk, wl, lane);
        wave_sync();
        // store_and_flag's two steps with the key's verdict between them: the encoding comes first
        packed_store(out, task, total_bytes, wl, lane, o);
        const bool valid = is_valid();
        records_flag(status, walk.rec, key_mx > two_kb && valid, FZ_VERDICT_ENCODING, lane);
        records_flag(status, walk.rec, bad && valid, FZ_VERDICT_NORM, lane);
        walk.step();
        key_mx = next_mx;
    };
    size_t task = T.first;
    for (; task + T.stride < T.tasks; task += T.stride) iteration(task, std::true_type());
    iteration(task, std::false_type());
}

template <int LOGD, bool FAST>
void launch_sign_records(fz_ctx *ctx, const uint8_t *key, const int32_t *c_hat, uint8_t *bytes, size_t total, unsigned rv, int wk,
                         int key_bound, int w, int bound, int *d_status) {
    hipLaunchKernelGGL((sign_records<LOGD, FAST>), chunk_grid(total, ctx->grid_signrec), dim3(64 * kWavesPerBlock), 0, ctx->stream,
                       key, c_hat, bytes, total, rv, wk, key_bound, w, bound, d_status, (const double2 *)ctx->d_twB,
                       (const double2 *)ctx->d_itwB, (const FzTwA *)ctx->d_twAB, ctx->mod);
}

}  // namespace

// the kernel's own resident grid (context creation; degrees 64 / 256, nothing to query at the others)
int fz_sign_records_query_grid(fz_ctx *ctx) {
    return fz_dispatch<6, 8>(ctx, FZ_OK, [&](auto logd, auto fast) {
        return fz_resident_grid(ctx, sign_records<logd(), fast()>, 64 * kWavesPerBlock, "occupancy query (sign_records)", &ctx->grid_signrec);
    });
}

// fz_sign_records_async: the fused pass over the batch as a fz_records_pass
int fz_launch_sign_records(fz_ctx *ctx, const uint8_t *key_bytes, int wk, int64_t key_bound, const int32_t *c_hat, size_t n, int l,
                           int w, int64_t bound, uint8_t *d_bytes, int *d_status) {
    const unsigned rv = (unsigned)l * (unsigned)ctx->degree;
    const size_t total = n * rv;
    const auto launch = [&]() {
        return fz_dispatch<6, 8>(ctx, FZ_E_UNSUPPORTED, [&](auto logd, auto fast) {
            launch_sign_records<logd(), fast()>(ctx, key_bytes, c_hat, d_bytes, total, rv, wk, (int)key_bound, w, (int)bound, d_status);
            return FZ_OK;
        });
    };
    return fz_records_pass(ctx, d_status, n, "sign_records launch", launch, d_bytes, fz_record_bytes(ctx->degree, l, w));
}
