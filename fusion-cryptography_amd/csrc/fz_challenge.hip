// fz_challenge.hip -- the per-signer challenge pipeline ON THE DEVICE (device half).
//
// hash_ch (fusion/fusion.py:511-531) for N independent (key, message) pairs:
//     x  = sign_hash_dst + "," + str(vk) + "," + str(int(prehash))                      fusion.py:412-419
//     b  = SHAKE-256(x), as many bytes as the decoder consumes                          fusion.py:515-524
//     c  = decode_bytes_to_polynomial_coefficients(b, ...)                              fusion.py:422-481
//     c^ = NTT(c)                                                                       fusion.py:499-507
// The text of str(vk) is the one the reference hashes (fusion.py:328-329 -> algebra/matrices.py:40-41 ->
// algebra/polynomials.py:257-258).  Verification keys never leave the device as text: three kernels, each stage a source of its own,
//   1. vk_text_kernel      one wave per signer: the exact ASCII text (the decimal of the 256-bit pre-hashed message
//      (fz_challenge_      included), padded (SHAKE suffix 0x1f ... 0x80) to whole 136-byte blocks, written to a scratch
//       text_dev.h)        row; integers are formatted where they are stored
//   2. shake_kernel        TWO lanes per signer, one holding the low and one the high 32 bits of every Keccak lane:
//      (fz_keccak_         bitwise steps are independent 32-bit operations, a 64-bit rotation is one v_alignbit of
//       lanes_dev.h)       (own half, partner's half) with the partner's half fetched by a DPP quad swap -- the same
//                          instruction stream for both lanes.  119 vector operations per round and lane instead of
//                          ~200 for a whole state per lane: the chain of ~108 permutations per signer (47 absorbed
//                          blocks + 61 squeezed) is the latency of the whole pipeline, and Keccak offers no more
//                          parallelism inside a permutation without bit-slicing overheads that cancel it.
//                          Output words leave transposed ([word][signer]) so that every access is coalesced.
//   3. decode_kernel       one lane per signer: bit-string of signs, then the partial Fisher-Yates shuffle driven by
//      (fz_challenge_      33-byte big-endian integers reduced mod (i + 1) -- as byte dot products with a weight table
//       decode_dev.h)      (v_dot4_u32_u8), all indices first (independent, loads three iterations ahead), then the
//                          swaps; stream positions are the same for every signer (scalar registers), shuffle state
//                          and indices in LDS ([position][lane]).
// then the ordinary forward transform (fz_ntt.hip).  Here: the fused form, one wave per signer through all of it
// (challenge_wave_kernel), the launchers and the decoder's weight table.  Supported: the scheme's parameter sets (norm bound 1,
// i.e. ternary challenges; degree <= 256); anything else returns FZ_E_UNSUPPORTED and callers use the host pipeline (fz_host.cpp).
#include "fz_internal.h"
#include "../../include/fusion_hip.h"
#include "fz_keccak_wave.h"
#include "fz_challenge_text_dev.h"
#include "fz_keccak_lanes_dev.h"
#include "fz_challenge_decode_dev.h"
#include <algorithm>

namespace {

// ---- the whole pipeline of ONE signer on ONE wave (fz_keccak_wave.h): pre-hash, text, absorb, squeeze, decode --------------------
// With a batch of BASELINE configs[2]'s size (1024 signers) the three kernels of the stages run 32 (lane pairs) or 16 (decoder)
// waves on a chip with 1024 SIMDs and the call is the latency of one signer's chain.  Here a signer has a wave to itself:
//   * SHA3-256 of the message and SHAKE-256 of the key text run on the wave-wide Keccak state (24 instructions + 4 gathers
//     per round instead of 119 instructions): the ~108 permutations take ~0.25 ms instead of 0.64;
//   * the text is written to LDS and absorbed from there, the stream is squeezed into the same LDS bytes and decoded from
//     there: nothing but the key row, the message and the 4 d bytes of the challenge touches memory;
//   * the decoder's two phases are the wave's: the shuffle indices 64 at a time (a lane per draw, the byte dot product of
//     decode_kernel with the table row of the lane's own modulus), then the swaps -- not as swaps at all: the k-th non-zero
//     coefficient (weight <= 64) ends where the FIRST draw that names its original position sends it (see phase 2 below),
//     one LDS minimum per draw instead of 195 dependent steps.
// LDS per wave: max(text row, stream, 4 d) + 64 bytes.
constexpr int kWaveAux = 64;

template <int W, int NW>      // signers (waves) per workgroup; stream words per index chunk
__global__ __launch_bounds__(64 * W) void challenge_wave_kernel(const int32_t *vk, size_t vk_stride, const uint8_t *pre, const uint8_t *msgs,
                                                                const unsigned long long *off, uint8_t *pre_out, uint32_t dst0, uint32_t dst1,
                                                                size_t N, VkTextParts T, DecodeShapeDev D, const uint32_t *tab, int out_blocks,
                                                                size_t region, int32_t *coefs) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int lane = threadIdx.x & 63;
    const size_t s = (size_t)blockIdx.x * W + (threadIdx.x >> 6);
    if (s >= N) return;                                          // waves of a workgroup never synchronise with each other
    uint8_t *buf = smem + (size_t)(threadIdx.x >> 6) * (region + kWaveAux);
    uint32_t *aux = reinterpret_cast<uint32_t *>(buf + region);
    VkTextIn tin;                                                // the key row and the fixed pieces: requested now, used after the message's
    vk_text_load(tin, vk + s * vk_stride, D.degree, T, lane);    // digest (a memory latency of ~2.5 us under the ~8 us before they are needed)
    fzkw::Wave K;
    K.init(lane);
    const bool ab = K.word < 17;                                 // the rate's 17 words (their owners and the halos)
    // ---- the pre-hashed message: SHA3-256(dst + "," + message) (fusion.py:405-409), or the caller's digest ----
    if (pre) {
        if (lane < 8) aux[lane] = reinterpret_cast<const uint32_t *>(pre + s * 32)[lane];
    } else {
        const unsigned long long len = off[s + 1] - off[s];
        const uint8_t *m = msgs + (off[s] - off[0]);
        const unsigned long long nb = (len + 4 + kFzShakeRate - 1) / kFzShakeRate, last = nb * kFzShakeRate - 1;      // 3 prefix bytes + message + the suffix byte
        // a block's 136 bytes are put together in LDS by the whole wave -- byte p of the stream by lane p mod 64, so that the
        // message is read in three coalesced requests per block (it may sit in pinned HOST memory: fz_staged_capi.hip) -- and
        // taken from there as the rate's 17 words
#pragma unroll 1
        for (unsigned long long b = 0; b < nb; ++b) {
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                const int idx = lane + 64 * t;
                if (idx < kFzShakeRate) buf[idx] = (uint8_t)sha3_msg_byte(b * kFzShakeRate + (unsigned)idx, len, m, dst0, dst1, last);
            }
            wave_sync();
            if (ab) {
                const uint2 w = *reinterpret_cast<const uint2 *>(buf + 8 * K.word);
                K.lo ^= w.x;
                K.hi ^= w.y;
            }
            wave_sync();
            K.permute();
        }
        if (K.main && K.word < 4) {
            aux[2 * K.word] = K.lo;
            aux[2 * K.word + 1] = K.hi;
            if (pre_out) *reinterpret_cast<uint2 *>(pre_out + s * 32 + 8 * K.word) = make_uint2(K.lo, K.hi);
        }
        K.lo = K.hi = 0u;
    }
    wave_sync();
    // str(int.from_bytes(digest, "little")): base 10^9 chunks.  The nine rounds of the eight-limb short division as a
    // systolic array: lane t owns limb t, the remainder travels from lane t + 1 to lane t (one DPP read), so lane t runs
    // round r at step r + 7 - t and the 72 dependent divisions of one lane become 16 steps of the wave (4.6 -> ~1 us).
    {
        uint32_t limb = lane < 8 ? aux[lane] : 0u, rem = 0u;
        wave_sync();                                             // every limb has been read before aux is rewritten
#pragma unroll 1
        for (int step = 0; step < 16; ++step) {
            const int r = step - (7 - lane);                     // this lane's round
            const uint32_t rin = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)rem, 0x101, 0xf, 0xf, true);       // lane t + 1's remainder
            const unsigned long long cur = ((unsigned long long)rin << 32) | limb;
            const uint32_t q = (uint32_t)(cur / 1000000000ull);
            const bool on = lane < 8 && r >= 0 && r < 9;
            rem = on ? (uint32_t)(cur - (unsigned long long)q * 1000000000ull) : 0u;
            if (on) limb = q;
            if (on && lane == 0) aux[r] = rem;
        }
        wave_sync();
        const uint32_t mine = lane < 9 ? aux[lane] : 0u;
        const unsigned long long nz = __ballot(mine != 0u);
        if (lane == 0) aux[9] = nz ? (uint32_t)(64 - __builtin_clzll(nz)) : 1u;
    }
    wave_sync();
    // ---- the text, absorbed from LDS ----
    const int nb = vk_text_wave(buf, region, aux, tin, D.degree, T, lane);
    {
        const uint8_t *src = buf + 8 * (ab ? K.word : 0);
        uint2 m = ab ? *reinterpret_cast<const uint2 *>(src) : make_uint2(0u, 0u);
#pragma unroll 1
        for (int b = 0; b < nb; ++b) {
            K.lo ^= m.x;
            K.hi ^= m.y;
            if (ab) m = *reinterpret_cast<const uint2 *>(src + (size_t)(b + 1 < nb ? b + 1 : b) * kFzShakeRate);        // the next block, under the permutation
            K.permute();
        }
    }
    wave_sync();
    // ---- the stream, squeezed into the same bytes ----
#pragma unroll 1
    for (int q = 0; q < out_blocks; ++q) {
        if (ab && K.main) *reinterpret_cast<uint2 *>(buf + (size_t)q * kFzShakeRate + 8 * K.word) = make_uint2(K.lo, K.hi);
        if (q + 1 < out_blocks) K.permute();
    }
    wave_sync();
    // ---- decoder (fusion.py:422-481), norm bound 1 ----
    const int d = D.degree, wt = D.weight < d ? D.weight : d;
    const int draws = d - 1 - D.weight > 0 ? d - 1 - D.weight : 0;
    // sign k = bit k (LSB first) of the big-endian integer in the leading sign_bytes bytes; magnitudes are 1 + (chunk mod 1) = 1
    int sgn = 0, pos = lane;
    if (lane < wt) sgn = ((buf[D.sign_bytes - 1 - (lane >> 3)] >> (lane & 7)) & 1) ? 1 : -1;
    // phase 1: j_n = int.from_bytes(chunk_n, "big") % (d - n), a lane per draw
    const int ib = D.index_bytes, pos0 = D.sign_bytes + D.coef_bytes * D.weight;
    const uint32_t *xs = reinterpret_cast<const uint32_t *>(buf);
    uint32_t jv[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (c * 64 < draws) {                                    // (uniform)
            const int n = c * 64 + lane, nn = n < draws ? n : draws - 1;
            const int o = pos0 + nn * ib, sh = o & 3;
            const uint32_t *pw = xs + (o >> 2);
            uint32_t w[NW];
#pragma unroll
            for (int t = 0; t < NW; ++t) w[t] = pw[t];
            const uint32_t mod = (uint32_t)(d - nn);
            const uint32_t *Tm = tab + (size_t)mod * kTabStride;
            const uint4 t0 = *reinterpret_cast<const uint4 *>(Tm), t1 = *reinterpret_cast<const uint4 *>(Tm + 4), t2 = *reinterpret_cast<const uint4 *>(Tm + 8);
            const uint32_t recip = Tm[12];
            const uint32_t tw[12] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w, t2.x, t2.y, t2.z, t2.w};
            uint32_t sum = 0;                                    // (decode_kernel's dot product, written out in both: see there)
#pragma unroll
            for (int g = 0; g < NW; ++g) {
                const uint32_t hi = g + 1 < NW ? w[g + 1 < NW ? g + 1 : g] : 0u;
                sum = __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(hi, w[g], sh), tw[g], sum, false);
            }
            jv[c] = sum - __umulhi(sum, recip) * mod;            // sum mod (d - n), exact (fz_challenge_weight_table)
        }
    }
    // phase 2: for i = d-1 down to weight+1: swap(c[i], c[j]).  Before step i the positions weight .. i hold zeros (induction
    // from the top: a step writes position i only), so a step either exchanges two zeros or lifts the non-zero coefficient k = j
    // from its ORIGINAL position (< weight) to i, where no later step reaches it (their i and j are smaller) -- and leaves a
    // zero at k, so later draws of k do nothing.  The k-th coefficient therefore ends at the i of the FIRST draw with j = k, or
    // stays: 195 dependent swaps (6.2 us of the kernel: a compare pair and two selects each) become one LDS minimum per draw.
    wave_sync();                                                 // every lane has read its index chunks: the stream's first words become scratch
    uint32_t *first = reinterpret_cast<uint32_t *>(buf);         // first[k], k < weight: the smallest draw number n with j_n = k
    if (lane < wt) first[lane] = 0xffffffffu;                    // (4 * weight <= 4 * degree bytes: inside the region whatever the parameters)
    wave_sync();
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int n = c * 64 + lane;
        if (n < draws && jv[c] < (uint32_t)wt) atomicMin(&first[jv[c]], (uint32_t)n);
    }
    wave_sync();
    if (lane < wt) {
        const uint32_t n1 = first[lane];
        pos = n1 != 0xffffffffu ? d - 1 - (int)n1 : lane;
    }
    wave_sync();                                                 // the stream has been read: its bytes become the coefficient row
    int32_t *out = reinterpret_cast<int32_t *>(buf);
    for (int j = lane; j < d; j += 64) out[j] = 0;
    wave_sync();
    if (lane < wt) out[pos] = sgn;
    wave_sync();
    int32_t *dst = coefs + s * (size_t)d;
    for (int j = lane * 4; j < d; j += 256) *reinterpret_cast<int4 *>(dst + j) = *reinterpret_cast<const int4 *>(out + j);
}

// What both launchers hand their kernels, built from the parameters once: the fixed pieces of the text (from the host serialiser,
// so both pipelines share one definition), the decoder's shape, and the stream words of an index chunk.
struct ChalLaunch { VkTextParts T; DecodeShapeDev D; int nw; };
int challenge_launch_prep(const fz_scheme_params *P, ChalLaunch &L) {
    fz_host_vk_text_parts(P, L.T.s0, &L.T.n0, L.T.s1, &L.T.n1, L.T.s2, &L.T.n2, 384);
    if (L.T.n0 < 0) return fz_set_error(FZ_E_UNSUPPORTED, "verification-key text pieces do not fit");
    L.D.degree = P->degree;
    L.D.weight = P->omega_ch;
    (void)fz_host_challenge_needed_bytes(P, &L.D.sign_bytes, &L.D.coef_bytes, &L.D.index_bytes);
    if (L.D.index_bytes > 4 * (kChunkWords - 1)) return fz_set_error(FZ_E_UNSUPPORTED, "index chunks of %d bytes", L.D.index_bytes);
    L.nw = (3 + L.D.index_bytes + 3) / 4;
    return FZ_OK;
}
// the instantiations of the two decoders: M(NW) for the smallest NW of 5, 9, 12 stream words that holds a chunk of nw
#define FZ_FOR_NW(nw, M) do { if ((nw) <= 5) M(5); else if ((nw) <= 9) M(9); else M(12); } while (0)

}  // namespace

// d_vk [N][2][degree] int32 (left row, right row), d_pre [N][32] (SHA3-256 digests of the messages = the pre-hashed
// integers, little-endian), d_text / d_nblocks / d_xof scratch; d_coefs [N][degree] out
int fz_launch_challenge(fz_ctx *ctx, const fz_scheme_params *P, const int32_t *d_vk, const uint8_t *d_pre, const uint32_t *d_dec, size_t N,
                        uint8_t *d_text, size_t text_stride, int *d_nblocks, uint32_t *d_xof, size_t xstride, int out_blocks,
                        const uint32_t *d_tab, int32_t *d_coefs) {
    ChalLaunch L;
    FZ_TRY(challenge_launch_prep(P, L));
    const int d = P->degree;
    const size_t lds_text = (size_t)kTextWaves * text_stride + kTextWaves * 64;
    if (lds_text > 160 * 1024) return fz_set_error(FZ_E_UNSUPPORTED, "text row too long for the serialiser");
    if (lds_text > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void *)vk_text_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_text);
        if (e != hipSuccess) return fz_check_hip(e, "text kernel LDS attribute");
    }
    hipLaunchKernelGGL(vk_text_kernel, dim3((unsigned)((N + kTextWaves - 1) / kTextWaves)), dim3(64 * kTextWaves), lds_text, ctx->stream,
                       d_vk, (size_t)2 * d, d_pre, d_dec, N, d, L.T, d_text, text_stride, d_nblocks);
    int rc = fz_check_hip(hipGetLastError(), "vk_text launch");
    if (rc != FZ_OK) return rc;
    const int max_blocks = (int)(text_stride / kFzShakeRate);
    // lane pairs while they fit one wave per SIMD (the latency-optimal form), whole states per lane beyond
    const int shake_mode = ctx->knob_shake_full ? ctx->knob_shake_full : ((N + 31) / 32 > (size_t)ctx->num_cu * 4 ? 2 : 1);
    const size_t per_wave = shake_mode == 2 ? 64 : 32, waves = (N + per_wave - 1) / per_wave;
#define FZ_SHK(KERNEL, W) hipLaunchKernelGGL((KERNEL<W>), dim3((unsigned)((waves + W - 1) / W)), dim3(64 * W), 0, ctx->stream, d_text, \
                                             text_stride, d_nblocks, N, max_blocks, out_blocks, d_xof, xstride)
    if (shake_mode == 2) { if (waves > (size_t)ctx->num_cu) FZ_SHK(shake_full_kernel, 4); else FZ_SHK(shake_full_kernel, 1); }
    else { if (waves > (size_t)ctx->num_cu) FZ_SHK(shake_kernel, 4); else FZ_SHK(shake_kernel, 1); }
#undef FZ_SHK
    rc = fz_check_hip(hipGetLastError(), "shake launch");
    if (rc != FZ_OK) return rc;
    const int kmax = out_blocks * kRateWords - 1;
    const dim3 dgrid((unsigned)((N + 63) / 64));
    const size_t dlds = (size_t)d * 64 + (size_t)(d > L.D.weight ? d - 1 - L.D.weight : 0) * 64 + 64;
#define FZ_DEC(NWV) hipLaunchKernelGGL(decode_kernel<NWV>, dgrid, dim3(64), dlds, ctx->stream, d_xof, xstride, N, L.D, d_tab, kmax, d_coefs)
    FZ_FOR_NW(L.nw, FZ_DEC);
#undef FZ_DEC
    return fz_check_hip(hipGetLastError(), "decode launch");
}

// the fused form: one wave per signer.  d_pre [N][32] (digests) or, when null, d_msgs / d_off (the messages back to back and
// their N + 1 offsets) with d_pre_out [N][32] (optional) receiving the digests; d_coefs [N][degree] out
bool fz_challenge_wave_ok(const fz_scheme_params *P) { return P->omega_ch <= 64 && P->degree <= 256 && P->degree >= 4; }

int fz_launch_challenge_wave(fz_ctx *ctx, const fz_scheme_params *P, const int32_t *d_vk, const uint8_t *d_pre, const uint8_t *d_msgs,
                             const unsigned long long *d_off, uint8_t *d_pre_out, size_t N, size_t text_stride, int out_blocks,
                             const uint32_t *d_tab, int32_t *d_coefs) {
    if (N == 0) return FZ_OK;
    ChalLaunch L;
    FZ_TRY(challenge_launch_prep(P, L));
    if (!fz_challenge_wave_ok(P)) return fz_set_error(FZ_E_UNSUPPORTED, "wave form: weight <= 64 and degree 4..256 only");
    // one region for the text row, then the stream (a chunk's NW words may end up to 12 bytes past it), then the coefficients
    size_t region = text_stride;
    region = std::max(region, (size_t)out_blocks * kFzShakeRate + 16);
    region = std::max(region, (size_t)P->degree * 4);
    region = (region + 15) & ~(size_t)15;
    constexpr int W = 4;
    const size_t lds = (size_t)W * (region + kWaveAux);
    if (lds > 160 * 1024) return fz_set_error(FZ_E_UNSUPPORTED, "text row too long for the fused challenge kernel");
    const dim3 grid((unsigned)((N + W - 1) / W)), block(64 * W);
#define FZ_CW(NWV) do { \
        if (lds > 64 * 1024) { \
            hipError_t e = hipFuncSetAttribute((const void *)challenge_wave_kernel<W, NWV>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
            if (e != hipSuccess) return fz_check_hip(e, "challenge kernel LDS attribute"); \
        } \
        hipLaunchKernelGGL((challenge_wave_kernel<W, NWV>), grid, block, lds, ctx->stream, d_vk, (size_t)2 * P->degree, d_pre, d_msgs, d_off, d_pre_out, \
                           (uint32_t)P->sign_pre_hash_dst[0], (uint32_t)P->sign_pre_hash_dst[1], N, L.T, L.D, d_tab, out_blocks, region, d_coefs); \
    } while (0)
    FZ_FOR_NW(L.nw, FZ_CW);
#undef FZ_CW
    return fz_check_hip(hipGetLastError(), "challenge (wave form) launch");
}

// SHA3-256 of dst + "," + message for N messages: d_msgs the message bytes back to back, d_off [N + 1] their offsets (any
// origin: off[0] is subtracted), d_pre [N][32] out
int fz_launch_prehash(fz_ctx *ctx, const fz_scheme_params *P, const uint8_t *d_msgs, const unsigned long long *d_off, size_t N,
                      uint8_t *d_pre, uint32_t *d_dec) {
    if (N == 0) return FZ_OK;
    hipLaunchKernelGGL(prehash_kernel, dim3((unsigned)((N + 31) / 32)), dim3(64), 0, ctx->stream, d_msgs, d_off, N,
                       (uint32_t)P->sign_pre_hash_dst[0], (uint32_t)P->sign_pre_hash_dst[1], d_pre, d_dec);
    return fz_check_hip(hipGetLastError(), "prehash launch");
}

// the decoder's weight table for (index_bytes, degree): tab[m][g] (g < 12) packs 256^(ib-1-(4g+t)) mod m for t = 0..3 (zero
// past the chunk), tab[m][12] = ceil(2^32 / m); m = 1 .. degree.  Host array of (degree + 1) * 16 words.
void fz_challenge_weight_table(int index_bytes, int degree, uint32_t *h_tab) {
    for (int m = 0; m <= degree; ++m) {
        uint32_t *T = h_tab + (size_t)m * kTabStride;
        for (int g = 0; g < kTabStride; ++g) T[g] = 0;
        if (m == 0) continue;
        uint32_t pw = 1u % (uint32_t)m;                          // 256^0 mod m, then upwards from the chunk's LAST byte
        for (int k = index_bytes - 1; k >= 0; --k) {
            T[k >> 2] |= pw << (8 * (k & 3));
            pw = (pw * 256u) % (uint32_t)m;
        }
        T[12] = (uint32_t)((0x100000000ull + (unsigned)m - 1) / (unsigned)m);      // ceil(2^32 / m); m = 1: 0 (2^32 wraps) ...
        if (m == 1) T[12] = 0xffffffffu;                         // ... any sum mod 1 = 0: with q = sum - 1 the weights are all 0 anyway
    }
}
