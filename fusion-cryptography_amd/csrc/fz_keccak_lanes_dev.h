// fz_keccak_lanes_dev.h -- stage 2 of the device challenge pipeline: Keccak-f[1600] on a lane PAIR per state (shake_kernel,
// prehash_kernel) and with a WHOLE state per lane (shake_full_kernel).  (The state spread over a wave: fz_keccak_wave.h.)  Device
// code of fz_challenge.hip, which includes it behind fz_challenge_text_dev.h.
#ifndef FZ_KECCAK_LANES_DEV_H
#define FZ_KECCAK_LANES_DEV_H

namespace {

// ---- Keccak-f[1600] on two lanes per state (low halves in the even lane, high halves in the odd lane) ----------------------------
// (the wave form keeps a copy of its own, fzkw::kRoundConst: served from that one the five lane kernels name another symbol in
// their address computations, which the kernel-by-kernel comparison counts as different: profiles/r24_challenge_units_isa.txt)
__constant__ uint32_t kRC[24][2] = {
    {0x00000001u, 0x00000000u}, {0x00008082u, 0x00000000u}, {0x0000808au, 0x80000000u}, {0x80008000u, 0x80000000u},
    {0x0000808bu, 0x00000000u}, {0x80000001u, 0x00000000u}, {0x80008081u, 0x80000000u}, {0x00008009u, 0x80000000u},
    {0x0000008au, 0x00000000u}, {0x00000088u, 0x00000000u}, {0x80008009u, 0x00000000u}, {0x8000000au, 0x00000000u},
    {0x8000808bu, 0x00000000u}, {0x0000008bu, 0x80000000u}, {0x00008089u, 0x80000000u}, {0x00008003u, 0x80000000u},
    {0x00008002u, 0x80000000u}, {0x00000080u, 0x80000000u}, {0x0000800au, 0x00000000u}, {0x8000000au, 0x80000000u},
    {0x80008081u, 0x80000000u}, {0x00008080u, 0x80000000u}, {0x80000001u, 0x00000000u}, {0x80008008u, 0x80000000u}};

__device__ __forceinline__ uint32_t partner(uint32_t x) {       // the other half of the same 64-bit lane: quad_perm [1,0,3,2]
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0xB1, 0xF, 0xF, true);
}

// this lane's half of rotl64(X, R), X = (own half, partner's half):  R < 32: (x << R) | (px >> (32 - R)) for BOTH lanes
// (low lane: lo' = lo << R | hi >> (32-R); high lane: hi' = hi << R | lo >> (32-R)); R >= 32 swaps the roles first
template <int R>
__device__ __forceinline__ uint32_t rotl64_half(uint32_t x, uint32_t px) {
    if (R == 0) return x;
    if (R == 32) return px;
    if (R < 32) return __builtin_amdgcn_alignbit(x, px, 32 - R);
    return __builtin_amdgcn_alignbit(px, x, 64 - R);
}

// three-input XOR in ONE instruction (v_bitop3_b32, truth table 0x96; the compiler keeps two v_xor otherwise)
#define FZ_X3(a, b, c) ((uint32_t)__builtin_amdgcn_bitop3_b32((a), (b), (c), 0x96))
// five rotated lanes of one output row: the five inputs first, then their five partner fetches, then the five
// rotations -- a DPP read of a register written by the previous instruction costs two wait states, and the compiler fills
// them with s_nop (36 per round pair in the first version) unless independent work sits in between
#define FZ_ROW(A0_, R0, A1_, R1, A2_, R2, A3_, R3, A4_, R4) \
    { const uint32_t t0 = (A0_), t1 = (A1_), t2 = (A2_), t3 = (A3_), t4 = (A4_); \
      const uint32_t p0 = partner(t0), p1 = partner(t1), p2 = partner(t2), p3 = partner(t3), p4 = partner(t4); \
      b0 = rotl64_half<R0>(t0, p0); b1 = rotl64_half<R1>(t1, p1); b2 = rotl64_half<R2>(t2, p2); \
      b3 = rotl64_half<R3>(t3, p3); b4 = rotl64_half<R4>(t4, p4); }
// one round A -> E (theta, rho + pi, chi, iota); every index a compile-time constant.  theta's column parities take two
// 3-input XORs each, and A ^ D = A ^ C[x-1] ^ rot(C[x+1], 1) is one more, so D is never formed: 119 vector operations per
// round and lane (10 parities, 10 for the five rotated parities, 25 + 48 for rho and pi, 25 chi, 1 iota)
#define FZ_KROUND32(A, E, rc) { \
    const uint32_t c0 = FZ_X3(FZ_X3(A##0, A##5, A##10), A##15, A##20), c1 = FZ_X3(FZ_X3(A##1, A##6, A##11), A##16, A##21), \
                   c2 = FZ_X3(FZ_X3(A##2, A##7, A##12), A##17, A##22), c3 = FZ_X3(FZ_X3(A##3, A##8, A##13), A##18, A##23), \
                   c4 = FZ_X3(FZ_X3(A##4, A##9, A##14), A##19, A##24); \
    uint32_t r0, r1, r2, r3, r4; \
    { const uint32_t q0 = partner(c0), q1 = partner(c1), q2 = partner(c2), q3 = partner(c3), q4 = partner(c4); \
      r0 = rotl64_half<1>(c0, q0); r1 = rotl64_half<1>(c1, q1); r2 = rotl64_half<1>(c2, q2); r3 = rotl64_half<1>(c3, q3); \
      r4 = rotl64_half<1>(c4, q4); } \
    /* d0 = c4 ^ r1, d1 = c0 ^ r2, d2 = c1 ^ r3, d3 = c2 ^ r4, d4 = c3 ^ r0 */ \
    uint32_t b0, b1, b2, b3, b4; \
    FZ_ROW(FZ_X3(A##0, c4, r1), 0, FZ_X3(A##6, c0, r2), 44, FZ_X3(A##12, c1, r3), 43, FZ_X3(A##18, c2, r4), 21, FZ_X3(A##24, c3, r0), 14) \
    E##0 = b0 ^ (~b1 & b2) ^ (rc); E##1 = b1 ^ (~b2 & b3); E##2 = b2 ^ (~b3 & b4); E##3 = b3 ^ (~b4 & b0); E##4 = b4 ^ (~b0 & b1); \
    FZ_ROW(FZ_X3(A##3, c2, r4), 28, FZ_X3(A##9, c3, r0), 20, FZ_X3(A##10, c4, r1), 3, FZ_X3(A##16, c0, r2), 45, FZ_X3(A##22, c1, r3), 61) \
    E##5 = b0 ^ (~b1 & b2); E##6 = b1 ^ (~b2 & b3); E##7 = b2 ^ (~b3 & b4); E##8 = b3 ^ (~b4 & b0); E##9 = b4 ^ (~b0 & b1); \
    FZ_ROW(FZ_X3(A##1, c0, r2), 1, FZ_X3(A##7, c1, r3), 6, FZ_X3(A##13, c2, r4), 25, FZ_X3(A##19, c3, r0), 8, FZ_X3(A##20, c4, r1), 18) \
    E##10 = b0 ^ (~b1 & b2); E##11 = b1 ^ (~b2 & b3); E##12 = b2 ^ (~b3 & b4); E##13 = b3 ^ (~b4 & b0); E##14 = b4 ^ (~b0 & b1); \
    FZ_ROW(FZ_X3(A##4, c3, r0), 27, FZ_X3(A##5, c4, r1), 36, FZ_X3(A##11, c0, r2), 10, FZ_X3(A##17, c1, r3), 15, FZ_X3(A##23, c2, r4), 56) \
    E##15 = b0 ^ (~b1 & b2); E##16 = b1 ^ (~b2 & b3); E##17 = b2 ^ (~b3 & b4); E##18 = b3 ^ (~b4 & b0); E##19 = b4 ^ (~b0 & b1); \
    FZ_ROW(FZ_X3(A##2, c1, r3), 62, FZ_X3(A##8, c2, r4), 55, FZ_X3(A##14, c3, r0), 39, FZ_X3(A##15, c4, r1), 41, FZ_X3(A##21, c0, r2), 2) \
    E##20 = b0 ^ (~b1 & b2); E##21 = b1 ^ (~b2 & b3); E##22 = b2 ^ (~b3 & b4); E##23 = b3 ^ (~b4 & b0); E##24 = b4 ^ (~b0 & b1); }

struct KState {
    uint32_t a0, a1, a2, a3, a4, a5, a6, a7, a8, a9, a10, a11, a12, a13, a14, a15, a16, a17, a18, a19, a20, a21, a22, a23, a24;
};

__device__ __forceinline__ void keccak_f_half(KState &S, int half) {
    uint32_t a0 = S.a0, a1 = S.a1, a2 = S.a2, a3 = S.a3, a4 = S.a4, a5 = S.a5, a6 = S.a6, a7 = S.a7, a8 = S.a8, a9 = S.a9,
             a10 = S.a10, a11 = S.a11, a12 = S.a12, a13 = S.a13, a14 = S.a14, a15 = S.a15, a16 = S.a16, a17 = S.a17,
             a18 = S.a18, a19 = S.a19, a20 = S.a20, a21 = S.a21, a22 = S.a22, a23 = S.a23, a24 = S.a24;
    uint32_t e0, e1, e2, e3, e4, e5, e6, e7, e8, e9, e10, e11, e12, e13, e14, e15, e16, e17, e18, e19, e20, e21, e22, e23, e24;
    // both halves of a round constant by SCALAR loads (the round index is uniform), the lane's half by a bitwise select (a
    // per-lane load put a vector-memory wait inside every round pair); the next pair's constants are requested before
    // this pair's rounds, so their latency is covered
    const uint32_t hmask = 0u - (uint32_t)half;
    uint32_t lo0 = kRC[0][0], hi0 = kRC[0][1], lo1 = kRC[1][0], hi1 = kRC[1][1];
#pragma unroll 1
    for (int r = 0; r < 24; r += 2) {
        const uint32_t rc0 = lo0 ^ ((lo0 ^ hi0) & hmask), rc1 = lo1 ^ ((lo1 ^ hi1) & hmask);
        const int rn = (r + 2) % 24;
        lo0 = kRC[rn][0]; hi0 = kRC[rn][1]; lo1 = kRC[rn + 1][0]; hi1 = kRC[rn + 1][1];
        FZ_KROUND32(a, e, rc0)
        FZ_KROUND32(e, a, rc1)
    }
    S.a0 = a0; S.a1 = a1; S.a2 = a2; S.a3 = a3; S.a4 = a4; S.a5 = a5; S.a6 = a6; S.a7 = a7; S.a8 = a8; S.a9 = a9;
    S.a10 = a10; S.a11 = a11; S.a12 = a12; S.a13 = a13; S.a14 = a14; S.a15 = a15; S.a16 = a16; S.a17 = a17; S.a18 = a18;
    S.a19 = a19; S.a20 = a20; S.a21 = a21; S.a22 = a22; S.a23 = a23; S.a24 = a24;
}

#define FZ_FOR17(M) M(0) M(1) M(2) M(3) M(4) M(5) M(6) M(7) M(8) M(9) M(10) M(11) M(12) M(13) M(14) M(15) M(16)
constexpr int kRateWords = kFzShakeRate / 4;        // 32-bit words of a block: the rows of the transposed stream a block takes

// text rows [N][text_stride] (padded blocks), nblocks [N]  ->  xof words, transposed: word k (32 bits: 64-bit lane k/2 of
// the stream, half k%2) of signer s at xof[k * xstride + s]
// Workgroups of WAVES independent waves.  More waves than CUs: four per workgroup -- they go to the four SIMDs of a CU,
// whereas four one-wave workgroups on a CU may share a SIMD (1024 of them ran at twice the time of 256: two chains on one
// issue port).  Fewer: one per workgroup, so that every chain has a CU (and its instruction fetch) to itself (669 us
// against 693 us).
template <int kShakeWaves>
__global__ __launch_bounds__(64 * kShakeWaves) void shake_kernel(const uint8_t *text, size_t text_stride, const int *nblocks, size_t N,
                                                                 int max_blocks, int out_blocks, uint32_t *xof, size_t xstride) {
    const int lane = threadIdx.x & 63, half = lane & 1;
    const size_t s_raw = ((size_t)blockIdx.x * kShakeWaves + (threadIdx.x >> 6)) * 32 + (lane >> 1);
    if (s_raw - (lane >> 1) >= N) return;                        // a whole wave past the end (the waves never synchronise)
    const bool live = s_raw < N;
    const size_t s = live ? s_raw : N - 1;                       // idle pairs shadow the last signer and store nothing
    const uint32_t *row = reinterpret_cast<const uint32_t *>(text + s * text_stride) + half;
    const int nb = nblocks[s];
    KState S = {};
    // the next block's 17 words are requested before this block's permutation: an absorbed block is otherwise one memory
    // round trip (the rows are 7 KB apart: nothing coalesces) in front of every one of the ~47 permutations
    uint32_t m0, m1, m2, m3, m4, m5, m6, m7, m8, m9, m10, m11, m12, m13, m14, m15, m16;
#define FZ_LD(i) m##i = row[2 * i];
    FZ_FOR17(FZ_LD)
#undef FZ_LD
#pragma unroll 1
    for (int b = 0; b < max_blocks; ++b) {
        if (b < nb) {                                            // both lanes of a pair agree; pairs of a wave may differ by a block
#define FZ_ABS(i) S.a##i ^= m##i;
            FZ_FOR17(FZ_ABS)
#undef FZ_ABS
            const uint32_t *w = row + (b + 1 < nb ? b + 1 : b) * kRateWords;
#define FZ_LD(i) m##i = w[2 * i];
            FZ_FOR17(FZ_LD)
#undef FZ_LD
            keccak_f_half(S, half);
        }
    }
    uint32_t *out = xof + s + (size_t)half * xstride;
#pragma unroll 1
    for (int m = 0; m < out_blocks; ++m) {
        if (live) {
            uint32_t *o = out + (size_t)m * kRateWords * xstride;
#define FZ_SQ(i) o[(size_t)(2 * i) * xstride] = S.a##i;
            FZ_FOR17(FZ_SQ)
#undef FZ_SQ
        }
        if (m + 1 < out_blocks) keccak_f_half(S, half);
    }
}

// ---- Keccak-f[1600] with a WHOLE state per lane (both 32-bit halves of every 64-bit lane in registers) ---------------------------
// For batches that fill the chip: a 64-bit rotation is two v_alignbit of the lane's own halves -- no partner fetch -- so a state
// costs ~180 vector operations per round instead of 2 x 119.  A single state takes 1.5x as long as on a lane pair, so this form
// pays only when the pair form would need more than one wave per SIMD (> 32 768 signers per pass): 65 536 signers are
// 1024 waves, one per SIMD.
struct W2 {
    uint32_t l, h;
};
__device__ __forceinline__ W2 w2_x3(W2 a, W2 b, W2 c) { return W2{FZ_X3(a.l, b.l, c.l), FZ_X3(a.h, b.h, c.h)}; }
__device__ __forceinline__ W2 w2_chi(W2 a, W2 b, W2 c) { return W2{a.l ^ (~b.l & c.l), a.h ^ (~b.h & c.h)}; }
template <int R>
__device__ __forceinline__ W2 w2_rotl(W2 x) {
    if (R == 0) return x;
    if (R == 32) return W2{x.h, x.l};
    if (R < 32) return W2{__builtin_amdgcn_alignbit(x.l, x.h, 32 - R), __builtin_amdgcn_alignbit(x.h, x.l, 32 - R)};
    return W2{__builtin_amdgcn_alignbit(x.h, x.l, 64 - R), __builtin_amdgcn_alignbit(x.l, x.h, 64 - R)};
}
// one output row y' of rho + pi + chi: B[x'] = rot(A[x][y] ^ D[x]) for the five (x, y) that land in row y' (x' = y,
// y' = 2x + 3y), the same (index, rotation) table as FZ_KROUND32 above
#define FZ_ROW64(E, O, I0, R0, I1, R1, I2, R2, I3, R3, I4, R4) \
    { const W2 b0 = w2_rotl<R0>(w2_x3(A[I0], C[(I0 + 4) % 5], Q[(I0 + 1) % 5])), b1 = w2_rotl<R1>(w2_x3(A[I1], C[(I1 + 4) % 5], Q[(I1 + 1) % 5])), \
               b2 = w2_rotl<R2>(w2_x3(A[I2], C[(I2 + 4) % 5], Q[(I2 + 1) % 5])), b3 = w2_rotl<R3>(w2_x3(A[I3], C[(I3 + 4) % 5], Q[(I3 + 1) % 5])), \
               b4 = w2_rotl<R4>(w2_x3(A[I4], C[(I4 + 4) % 5], Q[(I4 + 1) % 5])); \
      E[O] = w2_chi(b0, b1, b2); E[O + 1] = w2_chi(b1, b2, b3); E[O + 2] = w2_chi(b2, b3, b4); E[O + 3] = w2_chi(b3, b4, b0); \
      E[O + 4] = w2_chi(b4, b0, b1); }
__device__ __forceinline__ void keccak_round_full(const W2 (&A)[25], W2 (&E)[25], uint32_t rcl, uint32_t rch) {
    W2 C[5], Q[5];
#pragma unroll
    for (int x = 0; x < 5; ++x) C[x] = w2_x3(w2_x3(A[x], A[x + 5], A[x + 10]), A[x + 15], A[x + 20]);
#pragma unroll
    for (int x = 0; x < 5; ++x) Q[x] = w2_rotl<1>(C[x]);
    FZ_ROW64(E, 0, 0, 0, 6, 44, 12, 43, 18, 21, 24, 14)
    FZ_ROW64(E, 5, 3, 28, 9, 20, 10, 3, 16, 45, 22, 61)
    FZ_ROW64(E, 10, 1, 1, 7, 6, 13, 25, 19, 8, 20, 18)
    FZ_ROW64(E, 15, 4, 27, 5, 36, 11, 10, 17, 15, 23, 56)
    FZ_ROW64(E, 20, 2, 62, 8, 55, 14, 39, 15, 41, 21, 2)
    E[0].l ^= rcl;
    E[0].h ^= rch;
}
__device__ __forceinline__ void keccak_f_full(W2 (&A)[25]) {
    W2 E[25];
    uint32_t lo0 = kRC[0][0], hi0 = kRC[0][1], lo1 = kRC[1][0], hi1 = kRC[1][1];
#pragma unroll 1
    for (int r = 0; r < 24; r += 2) {
        const uint32_t a0 = lo0, b0 = hi0, a1 = lo1, b1 = hi1;
        const int rn = (r + 2) % 24;
        lo0 = kRC[rn][0]; hi0 = kRC[rn][1]; lo1 = kRC[rn + 1][0]; hi1 = kRC[rn + 1][1];
        keccak_round_full(A, E, a0, b0);
        keccak_round_full(E, A, a1, b1);
    }
}

// the same contract as shake_kernel, one lane per signer
template <int kShakeWaves>
__global__ __launch_bounds__(64 * kShakeWaves) void shake_full_kernel(const uint8_t *text, size_t text_stride, const int *nblocks,
                                                                      size_t N, int max_blocks, int out_blocks, uint32_t *xof,
                                                                      size_t xstride) {
    const int lane = threadIdx.x & 63;
    const size_t s_raw = ((size_t)blockIdx.x * kShakeWaves + (threadIdx.x >> 6)) * 64 + lane;
    if (s_raw - lane >= N) return;                               // a whole wave past the end (the waves never synchronise)
    const bool live = s_raw < N;
    const size_t s = live ? s_raw : N - 1;                       // idle lanes shadow the last signer and store nothing
    const uint2 *row = reinterpret_cast<const uint2 *>(text + s * text_stride);
    const int nb = nblocks[s];
    W2 A[25];
#pragma unroll
    for (int i = 0; i < 25; ++i) A[i] = W2{0u, 0u};
    uint2 m[17];
#pragma unroll
    for (int i = 0; i < 17; ++i) m[i] = row[i];
#pragma unroll 1
    for (int b = 0; b < max_blocks; ++b) {
        if (b < nb) {
#pragma unroll
            for (int i = 0; i < 17; ++i) { A[i].l ^= m[i].x; A[i].h ^= m[i].y; }
            const uint2 *w = row + (size_t)(b + 1 < nb ? b + 1 : b) * (kFzShakeRate / 8);
#pragma unroll
            for (int i = 0; i < 17; ++i) m[i] = w[i];
            keccak_f_full(A);
        }
    }
    uint32_t *out = xof + s;
#pragma unroll 1
    for (int q = 0; q < out_blocks; ++q) {
        if (live) {
            uint32_t *o = out + (size_t)q * kRateWords * xstride;
#pragma unroll
            for (int i = 0; i < 17; ++i) {
                o[(size_t)(2 * i) * xstride] = A[i].l;
                o[(size_t)(2 * i + 1) * xstride] = A[i].h;
            }
        }
        if (q + 1 < out_blocks) keccak_f_full(A);
    }
}

// byte p of what SHA3-256 absorbs for dst + "," + message (hash_message_to_int, fusion.py:405-409): the 3 prefix bytes, the
// message's `len` bytes at m, the suffix 0x06 and zeros, with 0x80 into position `last`, the end of the last block
__device__ __forceinline__ uint32_t sha3_msg_byte(unsigned long long p, unsigned long long len, const uint8_t *m, uint32_t dst0, uint32_t dst1,
                                                  unsigned long long last) {
    uint32_t v;
    if (p < 3) {
        v = p == 0 ? dst0 : (p == 1 ? dst1 : 0x2cu);
    } else {
        const unsigned long long k = p - 3;
        v = k < len ? (uint32_t)m[k] : (k == len ? 0x06u : 0u);
    }
    return p == last ? (v | 0x80u) : v;
}

// hash_message_to_int (fusion.py:405-409): SHA3-256 of dst + "," + message, one lane pair per message as above.  The
// stream is read byte by byte where it is absorbed -- messages are short (one block below 133 bytes) and start at any
// byte offset; its padding (0x06 ... 0x80) is part of the same byte function.  pre [N][32]: the digests, i.e. the
// pre-hashed integers, little-endian, exactly what vk_text_kernel prints in decimal.
__global__ __launch_bounds__(64) void prehash_kernel(const uint8_t *msgs, const unsigned long long *off, size_t N, uint32_t dst0,
                                                     uint32_t dst1, uint8_t *pre, uint32_t *dec) {
    const int lane = threadIdx.x & 63, half = lane & 1;
    const size_t s_raw = (size_t)blockIdx.x * 32 + (lane >> 1);
    const bool live = s_raw < N;
    const size_t s = live ? s_raw : N - 1;                       // idle pairs shadow the last message and store nothing
    const unsigned long long len = off[s + 1] - off[s];
    const uint8_t *m = msgs + (off[s] - off[0]);
    const unsigned long long nb = (len + 4 + kFzShakeRate - 1) / kFzShakeRate;        // 3 prefix bytes + message + the suffix byte
    const unsigned long long last = nb * kFzShakeRate - 1;
    unsigned long long nbmax = nb;                               // the wave's loop bound
#pragma unroll
    for (int w = 2; w < 64; w <<= 1) {
        const unsigned long long o = __shfl_xor(nbmax, w);
        nbmax = o > nbmax ? o : nbmax;
    }
    auto byte_at = [&](unsigned long long p) -> uint32_t { return sha3_msg_byte(p, len, m, dst0, dst1, last); };
    KState S = {};
#pragma unroll 1
    for (unsigned long long b = 0; b < nbmax; ++b) {
        if (b < nb) {                                            // both lanes of a pair agree
            const unsigned long long base = b * kFzShakeRate + 4 * half;
#define FZ_ABSB(i) { const unsigned long long q_ = base + 8 * i; \
                     S.a##i ^= byte_at(q_) | (byte_at(q_ + 1) << 8) | (byte_at(q_ + 2) << 16) | (byte_at(q_ + 3) << 24); }
            FZ_FOR17(FZ_ABSB)
#undef FZ_ABSB
            keccak_f_half(S, half);
        }
    }
    if (live) {
        uint32_t *o = reinterpret_cast<uint32_t *>(pre + s * 32) + half;
        o[0] = S.a0; o[2] = S.a1; o[4] = S.a2; o[6] = S.a3;
    }
    // the integer's decimal chunks for vk_text_kernel, by the even lane of the pair (limb 2k = its own half of lane k, limb
    // 2k + 1 = the partner's)
    const uint32_t p0 = partner(S.a0), p1 = partner(S.a1), p2 = partner(S.a2), p3 = partner(S.a3);
    if (dec && live && half == 0) {
        uint32_t limb[8] = {S.a0, p0, S.a1, p1, S.a2, p2, S.a3, p3};
        uint32_t *d = dec + s * kDecStride;
        d[9] = (uint32_t)u256_to_base1e9(limb, d);
    }
}

}  // namespace

#endif
