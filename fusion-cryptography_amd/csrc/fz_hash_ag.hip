// fz_hash_ag.hip -- hash_ag's aggregation coefficients for MANY committees ON THE DEVICE: one wave per committee.
//
// hash_ag (fusion/fusion.py:573-652) of one committee is ONE serial SHAKE-256:
//     x     = agg_xof_dst + "," + str(list(zip(sorted keys, pre-hashed messages, challenges)))             fusion.py:632-640
//     b     = SHAKE-256(x), N * n bytes, n = agg_coef_bytes                                                fusion.py:579-585, :641-645
//     a_i   = decode_bytes_to_polynomial_coefficients(b[i n : (i + 1) n], beta_ag, omega_ag)                fusion.py:646-651, :422-481
// about 100 permutations per signer, which nothing parallelises for one committee.  The sponges of DIFFERENT committees are
// independent: here each has a wave to itself (fz_keccak_wave.h: one Keccak state per wave), W committees per workgroup, waves never
// synchronising with each other -- the structure of challenge_wave_kernel (fz_challenge.hip), with three differences:
//   * the text has no bound (about 10 KB per signer), so it is STREAMED: one piece -- the fixed text in front of one polynomial and
//     that polynomial's values, at most 3.9 KB -- is written into LDS behind the bytes the last piece left over, the whole 136-byte
//     blocks are absorbed, and the tail of fewer than 136 bytes moves to the front.  The next piece's values are requested from
//     memory before the current piece's blocks are absorbed;
//   * the stream has no bound either: it is squeezed block by block into an LDS buffer of one section plus two blocks, section i is
//     decoded as soon as it is complete, and the block that holds the next section's first bytes moves to the front.  Sections are
//     not block-aligned: section i starts (i n) mod 136 bytes into its first block;
//   * the section is SHORTER than the decoder's walk where degree - 1 - omega_ag > omega_ag (degree 256: 195 draws, index bytes for
//     60): the reference then slices b"" and int.from_bytes(b"") is 0 (fusion.py:473-480), so a draw past the section takes j = 0.
// The decoder is challenge_wave_kernel's (signs, then "the first draw that names k"), written a second time with the section's
// offset and that rule: behind one helper the challenge kernels' generated code changes (fz_challenge_decode_dev.h).
// The fixed pieces of the text come from the host serialiser (fz_host_agg_text_parts), so both pipelines share one definition.
#include "fz_internal.h"
#include "../../include/fusion_hip.h"
#include "fz_keccak_wave.h"
#include "fz_wave_text_dev.h"               // wave_sync, dec_len
#include "fz_challenge_decode_dev.h"        // kChunkWords, kTabStride: the weight table is the challenge decoder's
#include <algorithm>

namespace {

constexpr int kAgPiece = 384;                // longest fixed piece in front of a list of values
constexpr int kAgFix = 3 * kAgPiece + 32;    // the fixed pieces in LDS: q0, q1, q2b (kAgPiece each), q2a, q3 (16 each)
constexpr int kAgAux = 64;                   // the pre-hashed integer in base 10^9
constexpr int kAgDigits = 78;                // longest decimal of a 256-bit integer

struct AgTextParts {                         // fz_host_agg_text_parts' pieces and the text's first four bytes: dst, ",", "["
    char q0[kAgPiece], q1[kAgPiece], q2b[kAgPiece], q2a[16], q3[16];
    int n0, n1, n2a, n2b, n3;
    uint32_t head;
};
struct AgShape {
    int degree, weight, sign_bytes, index_bytes;
    int pos0;                                // where a section's index chunks begin: sign bytes + the magnitudes' chunks
    int avail;                               // index chunks INSIDE a section; draws from this one on take j = 0
    int section;                             // n = agg_coef_bytes
};

// A wave-uniform pointer parked in two vector registers, and taken out where it is used: the absorb loop of the kernel below is short
// of scalar registers (lane masks of the wave-wide Keccak state, the loops' own state), and what a pointer costs there is two
// v_readfirstlane per use.  (The empty asm keeps the compiler from hoisting the read out of the loop, back into the scalar file.)
struct AgParked { uint32_t lo, hi; };
template <class T> __device__ __forceinline__ AgParked ag_park(T *p) {
    AgParked k{(uint32_t)(uintptr_t)p, (uint32_t)((uintptr_t)p >> 32)};
    asm volatile("" : "+v"(k.lo), "+v"(k.hi));
    return k;
}
template <class T> __device__ __forceinline__ T *ag_take(AgParked &k) {
    asm volatile("" : "+v"(k.lo), "+v"(k.hi));
    return reinterpret_cast<T *>((uintptr_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)k.lo) |
                                 ((uintptr_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)k.hi) << 32));
}

__device__ __forceinline__ uint32_t ag_take32(uint32_t &k) {
    asm volatile("" : "+v"(k));
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)k);
}

__device__ __forceinline__ void ag_load(int32_t (&v)[4], const int32_t *row, int degree, int lane) {
    const int vpl = degree >= 64 ? degree / 64 : 1, k0 = lane * vpl;
#pragma unroll
    for (int t = 0; t < 4; ++t) v[t] = (t < vpl && k0 + t < degree) ? row[k0 + t] : 0;
}

__device__ __forceinline__ int ag_put_fixed(uint8_t *buf, int at, const uint8_t *src, int n, int lane) {
    for (int c = lane; c < n; c += 64) buf[at + c] = src[c];
    return at + n;
}

// "v0, v1, ..., v_{d-1}" of one polynomial at buf[at ..): lane t writes its degree / 64 values (vk_text_wave's two passes); -> the length
__device__ __forceinline__ int ag_put_values(uint8_t *buf, int at, const int32_t (&vals)[4], int degree, int lane) {
    const int vpl = degree >= 64 ? degree / 64 : 1, k0 = lane * vpl;
    int mine = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int k = k0 + t;
        if (t < vpl && k < degree) mine += dec_len(vals[t]) + (k + 1 < degree ? 2 : 0);
    }
    int incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(incl, off);
        if (lane >= off) incl += o;
    }
    const int total = __shfl(incl, 63);
    int pos = at + incl - mine;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int k = k0 + t;
        if (t < vpl && k < degree) {
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
            if (k + 1 < degree) { buf[pos] = ','; buf[pos + 1] = ' '; pos += 2; }
        }
    }
    return total;
}

// str(int.from_bytes(digest, "little")) in base 10^9: challenge_wave_kernel's systolic short division (lane t owns limb t, the
// remainder travels from lane t + 1 to lane t), written a second time for the same reason as the decoder.  limb: the digest's
// word `lane` on lanes 0..7.  -> aux[0..8] the chunks, least significant first, aux[9] their number
__device__ __forceinline__ void ag_base1e9(uint32_t *aux, uint32_t limb, int lane) {
    uint32_t rem = 0u;
    wave_sync();                                                 // the last signer's chunks have been read
#pragma unroll 1
    for (int step = 0; step < 16; ++step) {
        const int r = step - (7 - lane);
        const uint32_t rin = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)rem, 0x101, 0xf, 0xf, true);
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
    wave_sync();
}

// the decimal of aux's integer at buf[at ..), lane c writing chunk c; -> its length
__device__ __forceinline__ int ag_put_u256(uint8_t *buf, int at, const uint32_t *aux, int lane) {
    const int nch = (int)aux[9];
    const int top = dec_len((int)aux[nch - 1]);                  // < 10^9: fits an int
    const int tl = top + 9 * (nch - 1);
    if (lane < nch) {
        unsigned u = aux[lane];
        const int nd = (lane == nch - 1) ? top : 9;
        int p = at + tl - 9 * lane;
        for (int k = 0; k < nd; ++k) {
            buf[--p] = (uint8_t)('0' + u % 10u);
            u /= 10u;
        }
    }
    return tl;
}

// Committee grp[slot] = (first entry of ord, signers) hashes rows ord[first], ord[first + 1], ... of vk [.][2][d], pre [.][32], chat [.][d]
// in that order; alpha[ord[first + i]] = the i-th decoded polynomial.  LDS per wave: region (the text pieces, then the stream) +
// 4 d (the decoder's row) + kAgFix + kAgAux.
template <int W, int NW>      // committees (waves) per workgroup; stream words per index chunk
__global__ __launch_bounds__(64 * W) void hash_ag_wave_kernel(const int32_t *vk, const uint8_t *pre, const int32_t *chat, const uint32_t *ord,
                                                              const uint2 *grp, size_t G, AgTextParts T, AgShape D, const uint32_t *tab,
                                                              size_t region, int32_t *alpha) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int lane = threadIdx.x & 63;
    const size_t slot = (size_t)blockIdx.x * W + (threadIdx.x >> 6);
    if (slot >= G) return;                                       // waves of a workgroup never synchronise with each other
    const int d = D.degree;
    uint8_t *buf = smem + (size_t)(threadIdx.x >> 6) * (region + (size_t)d * 4 + kAgFix + kAgAux);
    int32_t *out = reinterpret_cast<int32_t *>(buf + region);
    uint8_t *fix = buf + region + (size_t)d * 4;
    uint32_t *aux = reinterpret_cast<uint32_t *>(fix + kAgFix);
    const uint2 gr = grp[slot];
    uint32_t k_first = gr.x, k_cnt = gr.y;                       // (fewer than 2^31 rows: the entry sees to it; parked as the pointers are)
    uint32_t r = ord[gr.x], rn = r;                         // this signer's row and the next one's
    int32_t cur[4], nxt[4];
    ag_load(cur, vk + (size_t)r * 2 * d, d, lane);
#pragma unroll
    for (int t = 0; t < kAgPiece / 64; ++t) {
        const int c = lane + 64 * t;
        if (c < T.n0) fix[c] = (uint8_t)T.q0[c];
        if (c < T.n1) fix[kAgPiece + c] = (uint8_t)T.q1[c];
        if (c < T.n2b) fix[2 * kAgPiece + c] = (uint8_t)T.q2b[c];
    }
    if (lane < T.n2a) fix[3 * kAgPiece + lane] = (uint8_t)T.q2a[lane];
    if (lane < T.n3) fix[3 * kAgPiece + 16 + lane] = (uint8_t)T.q3[lane];
    // The pieces' lengths stay in vector registers although they are wave-uniform, the pointers are parked (AgParked), and so is
    // what only the second half of the kernel needs: the decoder's shape.
    int n0 = T.n0, n1 = T.n1, n2a = T.n2a, n2b = T.n2b, n3 = T.n3;
    asm volatile("" : "+v"(n0), "+v"(n1), "+v"(n2a), "+v"(n2b), "+v"(n3));
    int k_section = D.section, k_weight = D.weight, k_sign = D.sign_bytes, k_ib = D.index_bytes, k_pos0 = D.pos0, k_avail = D.avail;
    asm volatile("" : "+v"(k_section), "+v"(k_weight), "+v"(k_sign), "+v"(k_ib), "+v"(k_pos0), "+v"(k_avail));
    AgParked k_vk = ag_park(vk), k_pre = ag_park(pre), k_chat = ag_park(chat), k_ord = ag_park(ord), k_alpha = ag_park(alpha), k_tab = ag_park(tab);
    fzkw::Wave K;
    K.init(lane);
    const bool ab = K.word < 17;                                 // the rate's 17 words (their owners and the halos)
    wave_sync();
    // ---- absorb: the text piece by piece ----
    int have = 0;                                                // bytes at the front of buf that no block has taken yet (< 136)
    uint32_t limb = 0u;
#pragma unroll 1
    for (uint32_t i = 0; i < ag_take32(k_cnt); ++i) {
#pragma unroll 1
        for (int p = 0; p < 3; ++p) {                            // left key values, right key values, challenge values
            const uint32_t cnt = ag_take32(k_cnt);
            const bool last = p == 2 && i + 1 == cnt;
            int at = have;
            if (p == 0) {
                rn = ag_take<const uint32_t>(k_ord)[ag_take32(k_first) + (i + 1 < cnt ? i + 1 : i)];
                limb = lane < 8 ? reinterpret_cast<const uint32_t *>(ag_take<const uint8_t>(k_pre) + (size_t)r * 32)[lane] : 0u;
                if (i == 0) {
                    if (lane < 4) buf[at + lane] = (uint8_t)(T.head >> (8 * lane));
                    at += 4;
                } else {
                    if (lane < 2) buf[at + lane] = lane ? ' ' : ',';
                    at += 2;
                }
                at = ag_put_fixed(buf, at, fix, n0, lane);
            } else if (p == 1) {
                at = ag_put_fixed(buf, at, fix + kAgPiece, n1, lane);
            } else {
                at = ag_put_fixed(buf, at, fix + 3 * kAgPiece, n2a, lane);
                ag_base1e9(aux, limb, lane);
                at += ag_put_u256(buf, at, aux, lane);
                at = ag_put_fixed(buf, at, fix + 2 * kAgPiece, n2b, lane);
            }
            at += ag_put_values(buf, at, cur, d, lane);
            if (p == 2) {
                at = ag_put_fixed(buf, at, fix + 3 * kAgPiece + 16, n3, lane);
                if (last) {
                    if (lane == 0) buf[at] = ']';
                    at += 1;
                }
            }
            // the next piece's values, requested before this piece's blocks are absorbed
            ag_load(nxt, p == 1 ? ag_take<const int32_t>(k_chat) + (size_t)r * d : ag_take<const int32_t>(k_vk) + (p == 0 ? (size_t)r * 2 + 1 : (size_t)rn * 2) * d, d, lane);
            int nb = at / kFzShakeRate;
            if (last) {                                          // pad10*1 with SHAKE's domain bits: at least one byte, a whole block when
                nb += 1;                                         // the text ends on a block boundary, 0x9f when one byte is left
                const int end = nb * kFzShakeRate;
#pragma unroll
                for (int t = 0; t < 3; ++t)
                    if (at + lane + 64 * t < end) buf[at + lane + 64 * t] = 0;
                wave_sync();
                if (lane == 0) {
                    buf[at] ^= 0x1f;
                    buf[end - 1] ^= 0x80;
                }
            }
            wave_sync();
            {
                const uint8_t *src = buf + 8 * (ab ? K.word : 0);
                uint2 m = (ab && nb > 0) ? *reinterpret_cast<const uint2 *>(src) : make_uint2(0u, 0u);
#pragma unroll 1
                for (int b = 0; b < nb; ++b) {
                    K.lo ^= m.x;
                    K.hi ^= m.y;
                    if (ab) m = *reinterpret_cast<const uint2 *>(src + (size_t)(b + 1 < nb ? b + 1 : b) * kFzShakeRate);        // the next block, under the permutation
                    K.permute();
                }
            }
            have = last ? 0 : at - nb * kFzShakeRate;
            if (nb > 0 && have > 0) {                            // the tail moves to the front
                const uint8_t *s = buf + (size_t)nb * kFzShakeRate;
                uint8_t tl[3];
#pragma unroll
                for (int t = 0; t < 3; ++t) tl[t] = lane + 64 * t < have ? s[lane + 64 * t] : (uint8_t)0;
                wave_sync();
#pragma unroll
                for (int t = 0; t < 3; ++t)
                    if (lane + 64 * t < have) buf[lane + 64 * t] = tl[t];
            }
            wave_sync();
#pragma unroll
            for (int t = 0; t < 4; ++t) cur[t] = nxt[t];
            if (p == 2) r = rn;
        }
    }
    // ---- squeeze and decode, section by section ----
    const int n = __builtin_amdgcn_readfirstlane(k_section), weight = __builtin_amdgcn_readfirstlane(k_weight);
    const int sign_bytes = __builtin_amdgcn_readfirstlane(k_sign), ib = __builtin_amdgcn_readfirstlane(k_ib);
    const int pos0 = __builtin_amdgcn_readfirstlane(k_pos0), avail = __builtin_amdgcn_readfirstlane(k_avail);
    const int wt = weight < d ? weight : d;
    const int draws = d - 1 - weight > 0 ? d - 1 - weight : 0;
    const int lim = draws < avail ? draws : avail;               // draws whose chunk lies inside the section
    const uint32_t *xs = reinterpret_cast<const uint32_t *>(buf);
    int o = 0, held = 0;                                         // the section's offset in block 0; whole blocks already in buf
    bool stale = false;                                          // the state's block has been written out: permute before the next
#pragma unroll 1
    for (uint32_t i = 0; i < ag_take32(k_cnt); ++i) {
        const int need = (o + n + kFzShakeRate - 1) / kFzShakeRate;
#pragma unroll 1
        for (int q = held; q < need; ++q) {
            if (stale) K.permute();
            if (ab && K.main) *reinterpret_cast<uint2 *>(buf + (size_t)q * kFzShakeRate + 8 * K.word) = make_uint2(K.lo, K.hi);
            stale = true;
        }
        const uint32_t row = ag_take<const uint32_t>(k_ord)[ag_take32(k_first) + i];
        wave_sync();
        // decoder (fusion.py:422-481), norm bound 1: sign k = bit k (LSB first) of the big-endian integer in the leading sign bytes
        int sgn = 0, pos = lane;
        if (lane < wt) sgn = ((buf[o + sign_bytes - 1 - (lane >> 3)] >> (lane & 7)) & 1) ? 1 : -1;
        // phase 1: j_m = int.from_bytes(chunk_m, "big") % (d - m), a lane per draw; a chunk past the section is b"": j_m = 0
        uint32_t jv[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (c * 64 < lim) {                                  // (uniform)
                const int m = c * 64 + lane, mm = m < lim ? m : lim - 1;
                const int bo = o + pos0 + mm * ib, sh = bo & 3;
                const uint32_t *pw = xs + (bo >> 2);
                uint32_t w[NW];
#pragma unroll
                for (int t = 0; t < NW; ++t) w[t] = pw[t];
                const uint32_t mod = (uint32_t)(d - mm);
                const uint32_t *Tm = ag_take<const uint32_t>(k_tab) + (size_t)mod * kTabStride;
                const uint4 t0 = *reinterpret_cast<const uint4 *>(Tm), t1 = *reinterpret_cast<const uint4 *>(Tm + 4), t2 = *reinterpret_cast<const uint4 *>(Tm + 8);
                const uint32_t recip = Tm[12];
                const uint32_t tw[12] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w, t2.x, t2.y, t2.z, t2.w};
                uint32_t sum = 0;
#pragma unroll
                for (int g = 0; g < NW; ++g) {
                    const uint32_t hi = g + 1 < NW ? w[g + 1 < NW ? g + 1 : g] : 0u;
                    sum = __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(hi, w[g], sh), tw[g], sum, false);
                }
                jv[c] = m < lim ? sum - __umulhi(sum, recip) * mod : 0u;       // sum mod (d - m), exact (fz_challenge_weight_table)
            }
        }
        // phase 2 (challenge_wave_kernel's): coefficient k ends at d - 1 - (the FIRST draw with j = k), or stays
        uint32_t *first = reinterpret_cast<uint32_t *>(out);
        if (lane < wt) first[lane] = 0xffffffffu;
        wave_sync();
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int m = c * 64 + lane;
            if (m < draws && jv[c] < (uint32_t)wt) atomicMin(&first[jv[c]], (uint32_t)m);
        }
        wave_sync();
        if (lane < wt) {
            const uint32_t n1 = first[lane];
            pos = n1 != 0xffffffffu ? d - 1 - (int)n1 : lane;
        }
        wave_sync();
        for (int j = lane; j < d; j += 64) out[j] = 0;
        wave_sync();
        if (lane < wt) out[pos] = sgn;
        wave_sync();
        int32_t *dst = ag_take<int32_t>(k_alpha) + (size_t)row * d;
        for (int j = lane * 4; j < d; j += 256) *reinterpret_cast<int4 *>(dst + j) = *reinterpret_cast<const int4 *>(out + j);
        // the block that holds the next section's first bytes moves to the front
        const int e = o + n, lb = e / kFzShakeRate;
        o = e - lb * kFzShakeRate;
        held = o ? 1 : 0;
        if (o && lb) {
            uint2 v = make_uint2(0u, 0u);
            if (lane < kFzShakeRate / 8) v = *reinterpret_cast<const uint2 *>(buf + (size_t)lb * kFzShakeRate + 8 * lane);
            wave_sync();
            if (lane < kFzShakeRate / 8) *reinterpret_cast<uint2 *>(buf + 8 * lane) = v;
        }
        wave_sync();
    }
}

struct AgLaunch { AgTextParts T; AgShape D; int nw; size_t region; };

}  // namespace

// d_vk [.][2][degree], d_pre [.][32], d_c_hat [.][degree], ord [M] row indices and grp [G] = (first entry of ord, signers >= 1) --
// ord and grp device-visible (pinned host memory does) --; d_tab the challenge decoder's weight table; d_alpha [.][degree]
// receives one coefficient row per entry of ord, nothing else is written.  P: what fz_hash_ag_wave_ok (fz_hash_ag_capi.hip) takes
int fz_launch_hash_ag(fz_ctx *ctx, const fz_scheme_params *P, const int32_t *d_vk, const uint8_t *d_pre, const int32_t *d_c_hat,
                      const uint32_t *ord, const void *grp, size_t G, const uint32_t *d_tab, int32_t *d_alpha) {
    if (G == 0) return FZ_OK;
    AgLaunch L;                                                  // (the parameters are what fz_hash_ag_wave_ok takes: the entry's rule)
    int np[5];
    fz_host_agg_text_parts(P, L.T.q0, L.T.q1, L.T.q2a, L.T.q2b, L.T.q3, np, kAgPiece);
    if (np[0] < 0) return fz_set_error(FZ_E_UNSUPPORTED, "device hash_ag: text pieces do not fit");
    L.T.n0 = np[0]; L.T.n1 = np[1]; L.T.n2a = np[2]; L.T.n2b = np[3]; L.T.n3 = np[4];
    L.T.head = (uint32_t)P->agg_xof_dst[0] | ((uint32_t)P->agg_xof_dst[1] << 8) | ((uint32_t)',' << 16) | ((uint32_t)'[' << 24);
    int sb = 0, cb = 0, ib = 0;
    const size_t n = fz_host_agg_section_bytes(P, &sb, &cb, &ib);
    const int d = P->degree;
    L.D.degree = d;
    L.D.weight = P->omega_ag;
    L.D.sign_bytes = sb;
    L.D.index_bytes = ib;
    L.D.pos0 = sb + cb * P->omega_ag;
    L.D.avail = (int)((n - (size_t)L.D.pos0) / (size_t)ib);
    L.D.section = (int)n;
    L.nw = (3 + ib + 3) / 4;
    // the region holds the longest piece behind a tail of 135 bytes, with room for the final pad block: 13 bytes per value (11
    // characters and ", "); then the stream: the blocks a section touches at any offset, and the 4 kChunkWords bytes a chunk's
    // words may reach past it (they meet zero weights)
    const size_t piece = (size_t)std::max(std::max(4 + L.T.n0, L.T.n1), L.T.n2a + kAgDigits + L.T.n2b + L.T.n3 + 1) + (size_t)13 * d;
    const size_t text = (kFzShakeRate - 1) + piece + kFzShakeRate;
    const size_t stream = (kFzShakeRate - 1 + n + kFzShakeRate - 1) / kFzShakeRate * kFzShakeRate + 4 * kChunkWords;
    L.region = (std::max(text, stream) + 15) & ~(size_t)15;
    constexpr int W = 4;
    const size_t lds = (size_t)W * (L.region + (size_t)d * 4 + kAgFix + kAgAux);
    if (lds > 160 * 1024) return fz_set_error(FZ_E_UNSUPPORTED, "device hash_ag: section too long for the kernel's LDS");
    const dim3 grid((unsigned)((G + W - 1) / W)), block(64 * W);
#define FZ_AG(NWV) do { \
        if (lds > 64 * 1024) { \
            hipError_t e = hipFuncSetAttribute((const void *)hash_ag_wave_kernel<W, NWV>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
            if (e != hipSuccess) return fz_check_hip(e, "hash_ag kernel LDS attribute"); \
        } \
        hipLaunchKernelGGL((hash_ag_wave_kernel<W, NWV>), grid, block, lds, ctx->stream, d_vk, d_pre, d_c_hat, ord, (const uint2 *)grp, G, L.T, L.D, \
                           d_tab, L.region, d_alpha); \
    } while (0)
    if (L.nw <= 5) FZ_AG(5); else if (L.nw <= 9) FZ_AG(9); else FZ_AG(12);
#undef FZ_AG
    return fz_check_hip(hipGetLastError(), "hash_ag launch");
}
