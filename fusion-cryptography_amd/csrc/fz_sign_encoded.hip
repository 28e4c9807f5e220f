// fz_sign_encoded.hip -- signing straight to the compact byte encoding: sign_encode makes a chunk of
// the signature from the key and the challenge, inverse-transforms, range-checks and packs it, so that no int32 row of the
// signature ever reaches memory; its launcher and its resident-grid query.
#include "fz_records_dev.h"
#include "../../include/fusion_hip.h"

namespace {

// The signer of each of a lane's four 16-byte pieces.  chunk_load's lane mapping: piece j of a lane holds values 256 j + 4 lane ..
// + 3 of the chunk, so a lane's pieces lie 256 values apart and -- a record of l rows is 20.75 chunks at secpar 256, as little as
// a sixteenth of one at l = 1 and degree 64 -- in up to four different records.  The walk keeps (record, offset inside it) of the
// lane's piece 0 along the wave's chunks, stepped as RecWalk steps and with RecWalk's uniform operands (the chunk stride is the
// same); pieces 1 .. 3 follow from piece 0 by the same step with the stride of 256 values.  The divisions run once per wave, here.
struct PieceWalk {
    size_t rec;
    unsigned off, prec, poff;
    __device__ __forceinline__ PieceWalk(size_t first, unsigned rec_values, int lane) {
        const size_t e = first * kChunk + 4 * lane;
        rec = e / rec_values;
        off = (unsigned)(e - rec * rec_values);
        prec = 256u / rec_values;
        poff = 256u % rec_values;
        asm volatile("" : "+v"(prec), "+v"(poff));       // uniform, but VALU operands only (see RecWalk)
    }
    __device__ __forceinline__ void step(const RecWalk &w) { rec_advance(rec, off, w.srec, w.soff, w.rv); }
    // f(j, record, offset) for the lane's pieces j = 0 .. 3 of chunk `task`, the chunk the walk stands at; a piece past the end of
    // the batch (a ragged last chunk's) is given the batch's first values instead: read, transformed in polynomials of their own
    // and never stored
    template <class F>
    __device__ __forceinline__ void pieces(size_t task, size_t total, unsigned rv, int lane, const F &f) const {
        size_t pr = rec;
        unsigned po = off;
        const size_t e = task * kChunk + 4 * lane;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool in = e + 256 * j < total;
            f(j, in ? pr : (size_t)0, in ? po : 0u);
            rec_advance(pr, po, prec, poff, rv);
        }
    }
};

// the two key halves of a chunk in registers, piece j in l[j] and r[j]
struct KeyChunk { int4 l[4], r[4]; };

// sk_hat is [N][2][rv]: the halves of signer b lie rv values apart.  A piece never straddles a record or a polynomial: records
// are multiples of 16 values, offsets multiples of 4.
__device__ __forceinline__ const int32_t *key_piece(const int32_t *sk_hat, size_t rec, unsigned off, unsigned rv) {
    return sk_hat + rec * 2 * (size_t)rv + off;
}

// the wave's FIRST chunk: its 8 coalesced streaming 16-byte loads into registers
__device__ __forceinline__ KeyChunk key_load(const int32_t *sk_hat, const PieceWalk &pw, size_t task, size_t total, unsigned rv, int lane) {
    KeyChunk k;
    pw.pieces(task, total, rv, lane, [&](int j, size_t rec, unsigned off) __attribute__((always_inline)) {
        const int32_t *pl = key_piece(sk_hat, rec, off, rv);
        k.l[j] = nt_load4(pl);
        k.r[j] = nt_load4(pl + rv);
    });
    return k;
}

// every later chunk: the same 8 loads, the right halves into registers and the left halves straight into LDS (chunk_load_lds'
// instruction, here with a global address per piece: lane i's 16 bytes of piece j land at words 256 j + 4 i of
// `land`, the lane's own slots).  The left half costs no register while in flight; the reader waits itself (key_landed).
__device__ __forceinline__ void key_request(const int32_t *sk_hat, const PieceWalk &pw, size_t task, size_t total, unsigned rv, int lane,
                                            int32_t *land, KeyChunk &k) {
    typedef const __attribute__((address_space(1))) void *gptr;
    typedef __attribute__((address_space(3))) void *lptr;
    const lptr l = (lptr)land;
    pw.pieces(task, total, rv, lane, [&](int j, size_t rec, unsigned off) __attribute__((always_inline)) {
        const int32_t *pl = key_piece(sk_hat, rec, off, rv);
        // one LDS base and the piece's place as the instruction offset (a base per piece costs four scalar registers the FAST forms
        // do not have); the offset advances the global address as well, so that one is handed over 1024 j bytes short -- as an
        // integer: for a piece near the start of sk_hat the short address lies in front of the array, only address + offset is one
        const gptr g = (gptr)(reinterpret_cast<uintptr_t>(pl) - (uintptr_t)(1024 * j));
        if (j == 0) __builtin_amdgcn_global_load_lds(g, l, 16, 0, 2);          // aux 2: nt
        if (j == 1) __builtin_amdgcn_global_load_lds(g, l, 16, 1024, 2);
        if (j == 2) __builtin_amdgcn_global_load_lds(g, l, 16, 2048, 2);
        if (j == 3) __builtin_amdgcn_global_load_lds(g, l, 16, 3072, 2);
        k.r[j] = nt_load4(pl + rv);
    });
}
// ... landed (every vector memory operation of the wave has retired: the right halves, requested with them, are needed next
// anyway): the left halves out of the lane's slots
__device__ __forceinline__ void key_landed(const int32_t *land, int lane, KeyChunk &k) {
    chunk_landed<0>();
#pragma unroll
    for (int j = 0; j < 4; ++j) k.l[j] = *reinterpret_cast<const int4 *>(land + 256 * j + 4 * lane);
}

// the challenge pieces that go with a chunk's key pieces: shared by the signer's l rows and L2-resident, normal loads
template <int D>
__device__ __forceinline__ void chal_load(const int32_t *c_hat, const PieceWalk &pw, size_t task, size_t total, unsigned rv, int lane,
                                          int4 (&c)[4]) {
    pw.pieces(task, total, rv, lane, [&](int j, size_t rec, unsigned off) __attribute__((always_inline)) {
        c[j] = *reinterpret_cast<const int4 *>(c_hat + rec * D + (off & (unsigned)(D - 1)));
    });
}

// the chunk's int32 image in chunk_to_lds' layout: sigma = cent(cent(L * c) + R), exactly sign_kernel's arithmetic (any int32
// operands: |L * c| < 2^62 is inside fz_mulmod's bound, |. + R| < 2^32 inside fz_cent's).  Piece by piece, nothing crossing from
// one to the next: sixteen products interleaved hold more registers than the transform does.
__device__ __forceinline__ void sign_image(int32_t *stage, int lane, const KeyChunk &k, const int4 (&c)[4], const FzMod &m) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int4 o;
        o.x = (int)fz_cent(fz_mulmod((double)k.l[j].x, (double)c[j].x, m) + (double)k.r[j].x, m);
        o.y = (int)fz_cent(fz_mulmod((double)k.l[j].y, (double)c[j].y, m) + (double)k.r[j].y, m);
        o.z = (int)fz_cent(fz_mulmod((double)k.l[j].z, (double)c[j].z, m) + (double)k.r[j].z, m);
        o.w = (int)fz_cent(fz_mulmod((double)k.l[j].w, (double)c[j].w, m) + (double)k.r[j].w, m);
        *reinterpret_cast<int4 *>(stage + pad4(256 * j + 4 * lane)) = o;
        __builtin_amdgcn_sched_barrier(0);
    }
}

// sign and encode: the byte stream of the signatures [N][l][D] of sk_hat [N][2][l][D] under c_hat [N][D]; status word of a record
// |= FZ_VERDICT_NORM where some |z| > B.  records_encode<LOGD, FAST, true> with the chunk's int32 image computed instead of loaded.
// A wave-task is one 1024-value chunk of the OUTPUT stream.  The key pieces of the wave's next chunk are requested once the
// transpose buffer has been read back (inv16_passes' hook), the right halves into registers, the left halves into the 4 KiB of
// the wave's region behind the image: the landing area of the transforms, which is also where the packed chunk goes -- free from
// the hook until the fields are packed.  So an iteration (1) transforms its image up to the transpose, (2) requests the next
// chunk's key pieces, (3) runs the strided pass, centres into the image and range-checks, (4) waits for the pieces, takes the
// left halves out of the landing area and requests the challenge pieces, (5) packs into the same area, (6) makes the next image
// and (7) stores the packed chunk: the kernel holds one chunk of prefetch in registers across the strided pass, as records_encode
// does, and none across the contiguous pass.  The last iteration is peeled off (see fwd16_run).
template <int LOGD, bool FAST>
__global__ __launch_bounds__(64 * kWavesPerBlock) void sign_encode(const int32_t *sk_hat, const int32_t *c_hat, uint8_t *out, size_t total,
                                                                   unsigned rec_values, int w, int bound, int *status,
                                                                   const double2 *__restrict__ itwB, const FzTwA *tab, FzMod m) {
    constexpr int D = Geom<LOGD>::D, L = Geom<LOGD>::L;
    __shared__ __attribute__((aligned(16))) double lds[lds16_doubles<LOGD>()];
    const int lane = threadIdx.x & 63, p = lane / L, r = lane % L;
    const ChunkTasks T(total);
    // the three pointers only the lanes' own address arithmetic uses: VALU operands, out of the scalar file (see RecWalk) -- with
    // them there the FAST forms spill scalar registers beside the strided pass's table
    asm volatile("" : "+v"(sk_hat), "+v"(c_hat), "+v"(status));
    RecWalk walk(T.first, T.stride, rec_values, lane);    // the addresses need the walks: before the first loads here
    PieceWalk pw(T.first, rec_values, lane);
    KeyChunk raw0 = {};
    if (T.first < T.tasks) raw0 = key_load(sk_hat, pw, T.first, total, walk.rv, lane);      // before the table: see fwd16_run
    const double2 *s_tw = twiddles_to_lds<LOGD>(lds, itwB);
    const WaveLds W = wave_lds<LOGD>(lds, T.wave, p);
    if (T.first >= T.tasks) return;
    {
        int4 c[4];
        chal_load<D>(c_hat, pw, T.first, total, walk.rv, lane, c);
        sign_image(W.stage, lane, raw0, c, m);
    }
    pw.step(walk);                                        // from here on the walk stands at the chunk that is requested next
    const FieldBounds B(w, bound);

    auto iteration = [&](const size_t task, auto more_tag) __attribute__((always_inline)) {
        constexpr bool more = decltype(more_tag)::value;
        KeyChunk raw = {};
        int wl = w;
        asm volatile("" : "+s"(wl));                      // recomputed per chunk, not held across the loop: see records_encode
        const size_t total_bytes = total / 8 * (size_t)wl;
        wave_sync();
        {
            double a[16];
            image_to_doubles(W.stage, lane, a);
            wave_sync();
            inv16_to_image<LOGD, FAST>(a, W, p, r, s_tw, (TabPtr)tab, m, [&]() __attribute__((always_inline)) {
                if constexpr (more) key_request(sk_hat, pw, task + T.stride, total, walk.rv, lane, W.land, raw);
            });
            if constexpr (more) wave_sync_inflight();     // not a wait for the pieces in flight
            else wave_sync();
        }
        // the lane's 16 consecutive values, centred by the transform: range-checked, packed
        uint32_t u[16], hi = 0, mx = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int4 t = *reinterpret_cast<const int4 *>(W.stage + pad4(16 * lane + 4 * k));
            const int v[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const long long z = v[i];
                u[4 * k + i] = range_field(z, B, hi, mx);
            }
        }
        const bool bad = hi != 0 || mx > B.two_b;
        int4 c[4];
        if constexpr (more) {
            key_landed(W.land, lane, raw);
            chal_load<D>(c_hat, pw, task + T.stride, total, walk.rv, lane, c);
            wave_sync();                                  // the landing area has been read: it is the packed chunk's now
        }
        // (fields_pack and the read-back stay written out: inside a helper the packing comes out longer, docs/HISTORY.md section V)
        fields_pack(reinterpret_cast<uint16_t *>(W.pk) + lane * wl, u, wl);
        wave_sync();
        const Packed o = packed_from_lds(W.pk, wl, lane);
        wave_sync();
        if constexpr (more) {                             // waits for the challenge pieces (no store is younger)
            sign_image(W.stage, lane, raw, c, m);
            pw.step(walk);
        }
        store_and_flag(out, task, total, total_bytes, wl, lane, o, status, walk.rec, bad, FZ_VERDICT_NORM);
        walk.step();
    };
    size_t task = T.first;
    for (; task + T.stride < T.tasks; task += T.stride) iteration(task, std::true_type());
    iteration(task, std::false_type());
}

template <int LOGD, bool FAST>
void launch_sign_encode(fz_ctx *ctx, const int32_t *sk_hat, const int32_t *c_hat, uint8_t *bytes, size_t total, unsigned rv, int w,
                        int bound, int *d_status) {
    hipLaunchKernelGGL((sign_encode<LOGD, FAST>), chunk_grid(total, ctx->grid_signenc), dim3(64 * kWavesPerBlock), 0, ctx->stream,
                       sk_hat, c_hat, bytes, total, rv, w, bound, d_status, (const double2 *)ctx->d_itwB, (const FzTwA *)ctx->d_twAB + 1,
                       ctx->mod);
}

}  // namespace

// the kernel's own resident grid (context creation; degrees 64 / 256, nothing to query at the others): two workgroups per
// CU (176 - 185 VGPRs) against records_encode's three, whose grid would leave a third of the workgroups for a second round of
// the walk (see launch_records_k)
int fz_sign_encoded_query_grid(fz_ctx *ctx) {
    return fz_dispatch<6, 8>(ctx, FZ_OK, [&](auto logd, auto fast) {
        return fz_resident_grid(ctx, sign_encode<logd(), fast()>, 64 * kWavesPerBlock, "occupancy query (sign_encode)", &ctx->grid_signenc);
    });
}

// fz_sign_encoded_async: the fused pass over the batch as a fz_records_pass
int fz_launch_sign_encoded(fz_ctx *ctx, const int32_t *sk_hat, const int32_t *c_hat, size_t n, int l, int w, int64_t bound,
                           uint8_t *d_bytes, int *d_status) {
    const unsigned rv = (unsigned)l * (unsigned)ctx->degree;
    const size_t total = n * rv;
    const auto launch = [&]() {
        return fz_dispatch<6, 8>(ctx, FZ_E_UNSUPPORTED, [&](auto logd, auto fast) {
            launch_sign_encode<logd(), fast()>(ctx, sk_hat, c_hat, d_bytes, total, rv, w, (int)bound, d_status);
            return FZ_OK;
        });
    };
    return fz_records_pass(ctx, d_status, n, "sign_encode launch", launch, d_bytes, fz_record_bytes(ctx->degree, l, w));
}
