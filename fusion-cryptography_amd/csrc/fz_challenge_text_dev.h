// fz_challenge_text_dev.h -- stage 1 of the device challenge pipeline: the exact ASCII text of one signer by one wave (vk_text_wave,
// also the fused kernel's) and the kernel that writes the rows (vk_text_kernel).  Device code of fz_challenge.hip, which includes it.
#ifndef FZ_CHALLENGE_TEXT_DEV_H
#define FZ_CHALLENGE_TEXT_DEV_H

#include "fz_wave_text_dev.h"         // wave_sync, dec_len: shared with fz_hash_ag.hip

namespace {

struct VkTextParts {                         // the fixed pieces of the text, built on the host once per call
    char s0[384], s1[384], s2[16];           // before the left values / between left and right / after the right values
    int n0, n1, n2;
};

// str(int) of a 256-bit integer (eight 32-bit limbs, least significant first) in base 10^9: chunks out[0..n-1], least
// significant first; returns n (1..9).  Nine rounds of an eight-limb short division: a sequential chain, one LANE's work.
__device__ __forceinline__ int u256_to_base1e9(uint32_t (&limb)[8], uint32_t *out) {
    int n = 0;
    bool nz = true;
    while (nz && n < 9) {
        unsigned long long rem = 0;
        nz = false;
#pragma unroll
        for (int t = 7; t >= 0; --t) {
            const unsigned long long cur = (rem << 32) | limb[t];
            limb[t] = (uint32_t)(cur / 1000000000ull);
            rem = cur % 1000000000ull;
            nz |= limb[t] != 0;
        }
        out[n++] = (uint32_t)rem;
    }
    return n;
}
constexpr int kDecStride = 16;               // uint32 per signer in the decimal scratch: 9 chunks, the chunk count at [9]

// The text of ONE signer by ONE wave, into `buf` (LDS, `cap` bytes, a multiple of 16): the exact characters, the SHAKE
// suffix (0x1f ... 0x80) and zeros up to the end of the last 136-byte block; returns the number of blocks (all lanes).
// aux[0..9]: the pre-hashed integer in base 10^9 (chunks, least significant first) and the chunk count at [9].
// What the text of one signer needs from memory, per lane: its values of the key row (2 * degree of them over the wave, at
// most 8 per lane) and its bytes of the three fixed pieces.  Requested by the caller as early as it can: a load where the byte
// is written is a round trip per loop iteration (most of the 9 us the text took for one signer in round 5's first form).
struct VkTextIn {
    int32_t vals[8];
    uint8_t f0[6], f1[6], f2;
};
__device__ __forceinline__ void vk_text_load(VkTextIn &in, const int32_t *row, int degree, const VkTextParts &T, int lane) {
    const int nvals = 2 * degree;
    const int vpl = nvals >= 64 ? nvals / 64 : 1;
    const int k0 = lane * vpl;
#pragma unroll
    for (int t = 0; t < 8; ++t) in.vals[t] = (t < vpl && k0 + t < nvals) ? row[k0 + t] : 0;
#pragma unroll
    for (int t = 0; t < 6; ++t) {
        in.f0[t] = lane + 64 * t < T.n0 ? (uint8_t)T.s0[lane + 64 * t] : (uint8_t)0;
        in.f1[t] = lane + 64 * t < T.n1 ? (uint8_t)T.s1[lane + 64 * t] : (uint8_t)0;
    }
    in.f2 = lane < T.n2 ? (uint8_t)T.s2[lane] : (uint8_t)0;
}

__device__ __forceinline__ int vk_text_wave(uint8_t *buf, size_t cap, const uint32_t *aux, const VkTextIn &in, int degree, const VkTextParts &T,
                                            int lane) {
    const int nvals = 2 * degree;
    const int vpl = nvals >= 64 ? nvals / 64 : 1;               // values per lane, at most 8 (a lane never straddles the two halves)
    const int k0 = lane * vpl;
    const int32_t (&vals)[8] = in.vals;
    const uint8_t (&f0)[6] = in.f0, (&f1)[6] = in.f1;
    const uint8_t f2 = in.f2;
    for (size_t o = (size_t)lane * 16; o < cap; o += 64 * 16) *reinterpret_cast<int4 *>(buf + o) = make_int4(0, 0, 0, 0);
    // pass 1: lengths (digits + ", " unless last of its half)
    int mine = 0;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int k = k0 + t;
        if (t < vpl && k < nvals) mine += dec_len(vals[t]) + (((k + 1) % degree) ? 2 : 0);
    }
    int incl = mine;                                            // inclusive scan over the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(incl, off);
        if (lane >= off) incl += o;
    }
    const int total_vals = __shfl(incl, 63);
    const int left_total = (nvals >= 64) ? __shfl(incl, 31) : __shfl(incl, degree - 1);
    int pos = T.n0 + (incl - mine) + ((k0 >= degree) ? T.n1 : 0);
    wave_sync();                                                // the zero fill above before the byte writes below
    // pass 2: characters, last digit first
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int k = k0 + t;
        if (t < vpl && k < nvals) {
            const int v = vals[t];
            const int n = dec_len(v);
            unsigned u = v < 0 ? 0u - (unsigned)v : (unsigned)v;
            int p = pos + n;
            do {
                buf[--p] = (uint8_t)('0' + u % 10u);
                u /= 10u;
            } while (u);
            if (v < 0) buf[--p] = '-';
            pos += n;
            if ((k + 1) % degree) { buf[pos] = ','; buf[pos + 1] = ' '; pos += 2; }
        }
    }
    // fixed pieces and the decimal of the pre-hashed message (lane c writes chunk c: 9 digits, the leading chunk as many
    // as it has)
    const int nch = (int)aux[9];
    const int top = dec_len((int)aux[nch - 1]);                  // < 10^9: fits an int
    const int tl = top + 9 * (nch - 1);
    const int at1 = T.n0 + left_total, at2 = T.n0 + T.n1 + total_vals, at3 = at2 + T.n2;
#pragma unroll
    for (int t = 0; t < 6; ++t) {
        const int c = lane + 64 * t;
        if (c < T.n0) buf[c] = f0[t];
        if (c < T.n1) buf[at1 + c] = f1[t];
    }
    if (lane < T.n2) buf[at2 + lane] = f2;
    if (lane < nch) {
        unsigned u = aux[lane];
        const int nd = (lane == nch - 1) ? top : 9;
        int p = at3 + tl - 9 * lane;                             // one past this chunk's last digit
        for (int k = 0; k < nd; ++k) {
            buf[--p] = (uint8_t)('0' + u % 10u);
            u /= 10u;
        }
    }
    const int len = at3 + tl;
    const int nb = len / kFzShakeRate + 1;                      // pad10*1 always adds at least one byte
    wave_sync();
    if (lane == 0) {
        buf[len] ^= 0x1f;                                       // SHAKE domain bits + first pad bit (FIPS 202)
        buf[nb * kFzShakeRate - 1] ^= 0x80;
    }
    wave_sync();
    return nb;
}

// one wave per signer, kTextWaves signers per workgroup.  text row i: blocks * 136 bytes, *nblocks = blocks.
// dec (optional): the pre-hashed integers already in base 10^9 (prehash_kernel converts them with a lane per message; done
// here it is one lane of the signer's wave while 63 wait: a third of this kernel's time)
constexpr int kTextWaves = 4;
__global__ __launch_bounds__(64 * kTextWaves) void vk_text_kernel(const int32_t *vk, size_t vk_stride, const uint8_t *pre,
                                                                  const uint32_t *dec, size_t N, int degree, VkTextParts T,
                                                                  uint8_t *text, size_t text_stride, int *nblocks) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t i = (size_t)blockIdx.x * kTextWaves + wave;
    if (i >= N) return;
    uint8_t *buf = smem + (size_t)wave * text_stride;
    uint32_t *aux = reinterpret_cast<uint32_t *>(smem + (size_t)kTextWaves * text_stride) + wave * 16;
    // str(int.from_bytes(prehash, "little")) (fusion.py:405-409, :416-418): the 256-bit integer in base 10^9, least
    // significant chunk first (one lane: 9 rounds of an 8-limb short division), digits written by lanes 0..8
    if (dec) {
        if (lane < 10) aux[lane] = dec[i * kDecStride + lane];
    } else if (lane == 0) {
        uint32_t limb[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const uint8_t *b = pre + i * 32 + 4 * t;
            limb[t] = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
        }
        aux[9] = (uint32_t)u256_to_base1e9(limb, aux);
    }
    VkTextIn tin;
    vk_text_load(tin, vk + i * vk_stride, degree, T, lane);
    const int nb = vk_text_wave(buf, text_stride, aux, tin, degree, T, lane);
    if (lane == 0) nblocks[i] = nb;
    uint8_t *dst = text + i * text_stride;
    for (int o = lane * 8; o < nb * kFzShakeRate; o += 64 * 8) *reinterpret_cast<uint2 *>(dst + o) = *reinterpret_cast<const uint2 *>(buf + o);
}

}  // namespace

#endif
