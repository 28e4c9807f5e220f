// fz_records_dev.h -- the device building blocks of the compact byte encoding that more than one unit uses (fz_records.hip: the
// records_* kernels; fz_aggregate_encoded.hip: the range check and the aggregation straight from the bytes): the packed chunk of
// the chunk walk, the field unpacking, the per-record status flag and the record walk.  No kernels and no host code here;
// everything is private to the unit that includes it.
#ifndef FZ_RECORDS_DEV_H
#define FZ_RECORDS_DEV_H

#include "fz_ntt_dev.h"

namespace {
// ------------------------------------------------------------------------------------------
// Compact byte encoding of records (not in the reference).  A record is `rows` rows of D values; each
// value becomes a w-bit field u = z + B (z centred, B the kind's bound, w = bit_length(2B)), fields row-major and LSB first.
// Coefficient-domain kinds (COEF: signatures, aggregates) carry z = cent(INTT(row)); verification keys z = cent(row).
// The transform kernels' chunk walk: one wave-task is one 1024-value chunk of the batch, i.e. 1024 fields = 128 * w bytes = 8 * w
// 16-byte units of the byte stream (the chunk of task t starts at byte 128 * w * t, always 16-byte aligned).  Lane `lane` owns the
// chunk's values 16 * lane .. 16 * lane + 15, i.e. w consecutive 16-bit words of the packed chunk; a record is a multiple of 16
// values, so a lane's fields never straddle two records.  Staging per wave: the int32 image of chunk_load at the start of the
// wave's transpose region, the packed chunk (at most 4 KiB, w <= 32) right behind it: together exactly the region, so the LDS of
// a workgroup is that of the transforms (lds16_doubles).  w and B are kernel arguments: every branch on them is wave-uniform.
// ------------------------------------------------------------------------------------------
constexpr int kPackOff = kStageWords * 4;            // byte offset of the packed chunk inside a wave's region
constexpr int kPackBytes = 128 * 32;                 // 1024 fields of at most 32 bits
static_assert(kPackOff + kPackBytes <= Geom<6>::PPW * Geom<6>::PS * 8 && kPackOff + kPackBytes <= Geom<8>::PPW * Geom<8>::PS * 8,
              "the packed chunk must fit behind the int32 image in a wave's region");

typedef int fz_v2i __attribute__((ext_vector_type(2)));
// the wave-uniform table of the transform is read from constant memory where it is used, as polymul16 does: held in scalar
// registers across the loop (72 of them) it leaves too few for the record walk and the field width
typedef const __attribute__((address_space(4))) FzTwA *TabPtr;

// a packed chunk in registers: unit 64 * j + lane in u[j] (8 * w <= 256 units)
struct Packed { int4 u[4]; };

// the packed chunk of `task`: units past the end of the stream are not read; the stream's last unit may be 8 bytes (a record
// of degree 64 with rows * w odd), then it is read as such
__device__ __forceinline__ Packed packed_load(const uint8_t *in, size_t task, size_t total_bytes, int w, int lane) {
    Packed c;
    const size_t base = task * 128 * (size_t)w;
    const size_t left = total_bytes - base;
    const unsigned cb = (unsigned)(left < (size_t)128 * w ? left : (size_t)128 * w);      // the chunk's bytes (uniform)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        c.u[j] = make_int4(0, 0, 0, 0);
        if (64u * 16u * j < cb) {
            const unsigned off = 16u * (64u * j + lane);
            if (off + 16 <= cb) {
                const fz_v4i t = __builtin_nontemporal_load(reinterpret_cast<const fz_v4i *>(in + base + off));
                c.u[j] = make_int4(t.x, t.y, t.z, t.w);
            } else if (off < cb) {
                const fz_v2i t = __builtin_nontemporal_load(reinterpret_cast<const fz_v2i *>(in + base + off));
                c.u[j] = make_int4(t.x, t.y, 0, 0);
            }
        }
    }
    return c;
}

__device__ __forceinline__ void packed_to_lds(uint8_t *pk, const Packed &c, int w, int lane) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (64 * j < 8 * w && 64 * j + lane < 8 * w) *reinterpret_cast<int4 *>(pk + 16 * (64 * j + lane)) = c.u[j];
}

__device__ __forceinline__ Packed packed_from_lds(const uint8_t *pk, int w, int lane) {
    Packed c;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        c.u[j] = make_int4(0, 0, 0, 0);
        if (64 * j < 8 * w && 64 * j + lane < 8 * w) c.u[j] = *reinterpret_cast<const int4 *>(pk + 16 * (64 * j + lane));
    }
    return c;
}

// ... and back: the lane's w words at src -> its 16 fields (exactly w words are read)
__device__ __forceinline__ void fields_unpack(const uint16_t *src, uint32_t (&u)[16], int w) {
    const unsigned long long mask = (1ull << w) - 1;
    unsigned long long acc = 0;
    int nb = 0, o = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
#pragma unroll
        for (int e = 0; e < 2; ++e)
            if (nb < w) {
                acc |= (unsigned long long)src[o++] << nb;
                nb += 16;
            }
        u[k] = (uint32_t)(acc & mask);
        acc >>= w;
        nb -= w;
    }
}

// Per-record status: every (wave, record) with a failing lane sets its record's word with ONE atomic (at most 16 records meet
// in a chunk)
__device__ __forceinline__ void records_flag(int *status, size_t rec, bool bad, int code, int lane) {
    unsigned long long fail = __ballot(bad);
    while (fail) {                                        // uniform: one round per failing record of the wave
        const int first = __builtin_ctzll(fail);
        const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)rec, first);
        const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(rec >> 32), first);
        const size_t r = ((size_t)hi << 32) | lo;
        if (lane == first) atomicOr(status + r, code);
        fail &= ~__ballot(rec == r);
    }
}

// the record of a lane's first value, walked along the wave's chunks: the divisions run once per wave (constructor), a step is
// an add, a compare and a select (per lane: the uniform state would compete with the transform's scalar operands)
struct RecWalk {
    size_t rec, srec;
    unsigned off, soff, rv;
    __device__ __forceinline__ RecWalk(size_t first, size_t stride, unsigned rec_values, int lane) : rv(rec_values) {
        const size_t e = first * kChunk + 16 * lane, s = stride * kChunk;
        rec = e / rv;
        off = (unsigned)(e - rec * rv);
        srec = s / rv;
        soff = (unsigned)(s - srec * rv);
        asm volatile("" : "+v"(srec), "+v"(soff), "+v"(rv));      // uniform, but VALU operands only: out of the scalar file
    }
    __device__ __forceinline__ void step() {
        off += soff;                                      // < 2 * rv: no overflow, rv < 2^31
        const unsigned c = off >= rv ? 1u : 0u;
        rec += srec + c;
        off -= c * rv;
    }
};

}  // namespace

#endif
