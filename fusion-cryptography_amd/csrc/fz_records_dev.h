// fz_records_dev.h -- the device building blocks of the compact byte encoding that more than one unit uses (fz_records.hip: the
// records_* kernels; fz_aggregate_encoded.hip and fz_aggregate_many_encoded.hip, through fz_aggregate_encoded_dev.h: the range check
// and the aggregation straight from the bytes, of one committee and of many; fz_verify_encoded.hip:
// the verification straight from the bytes; fz_sign_encoded.hip: signing straight to the bytes; fz_sign_records.hip: signing
// straight from the key's bytes to the signature's; fz_keygen_records.hip: key generation straight to the key's bytes, which
// takes the field packing, the range check's step and the status flag; fz_vk_records.hip: the verification key straight from the
// key's bytes, on the consumers' steps): the packed chunk of the chunk
// walk with its loads and stores, the field packing and unpacking, the consumers' steps from the packed chunk to the transform's
// outputs and their sums, the per-record status flag, the record walk, the chunk walk's opening, and the producers' steps from
// the int32 image to the stored chunk (the range check's operands and its per-value step, the inverse transform centred into the
// image, store and flag).  No kernels here, and of host code only chunk_grid, the launch grid of the chunk walk; everything is
// private to the unit that includes it.
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

// the chunk's units to the stream (streaming stores; an 8-byte last unit as such, nothing past the end)
__device__ __forceinline__ void packed_store(uint8_t *out, size_t task, size_t total_bytes, int w, int lane, const Packed &c) {
    const size_t base = task * 128 * (size_t)w;
    const size_t left = total_bytes - base;
    const unsigned cb = (unsigned)(left < (size_t)128 * w ? left : (size_t)128 * w);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (64u * 16u * j < cb) {
            const unsigned off = 16u * (64u * j + lane);
            if (off + 16 <= cb) {
                fz_v4i t = {c.u[j].x, c.u[j].y, c.u[j].z, c.u[j].w};
                __builtin_nontemporal_store(t, reinterpret_cast<fz_v4i *>(out + base + off));
            } else if (off < cb) {
                fz_v2i t = {c.u[j].x, c.u[j].y};
                __builtin_nontemporal_store(t, reinterpret_cast<fz_v2i *>(out + base + off));
            }
        }
    }
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

// a lane's 16 fields (u < 2^w) -> its w 16-bit words at dst.  The bit count `nb` depends on w only: the emits are uniform branches.
__device__ __forceinline__ void fields_pack(uint16_t *dst, const uint32_t (&u)[16], int w) {
    unsigned long long acc = 0;
    int nb = 0, o = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        acc |= (unsigned long long)u[k] << nb;      // nb < 16: at most 47 bits held
        nb += w;
#pragma unroll
        for (int e = 0; e < 2; ++e)
            if (nb >= 16) {
                dst[o++] = (uint16_t)acc;
                acc >>= 16;
                nb -= 16;
            }
    }
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

// The steps every consumer of the bytes takes between its prefetch and its own work on the transform's outputs.  `pk`, `stage`
// and `row` are the packed chunk, the int32 image and the lane's polynomial p in the wave's region; (p, r) = (lane / L, lane % L).

// the lane's w words of the packed chunk -> its 16 fields, in u and as u - B in the int32 image (chunk_to_lds' layout: the low 32
// bits are z whenever u <= 2B, just an integer otherwise); -> the lane's largest field, for the range test u <= 2B of those who
// make it.  What depends on w alone (the bit offsets of the unpacking) is recomputed per chunk, not held across the loop: w is
// pinned in a scalar register here, as records_encode pins it for the packing.
// The form is the one that leaves every caller's code as it was with the text in place (docs/HISTORY.md section M): arguments
// by reference, as a kernel's iteration lambda holds them, and the fields in an array of the caller's.
__device__ __forceinline__ uint32_t fields_to_image(const uint8_t *const &pk, int32_t *const &stage, const int &w, const uint32_t &bound,
                                                    const int &lane, uint32_t (&u)[16]) {
    uint32_t mx = 0;
    int wl = w;
    asm volatile("" : "+s"(wl));
    fields_unpack(reinterpret_cast<const uint16_t *>(pk) + lane * wl, u, wl);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int4 t;
        t.x = (int)(u[4 * k + 0] - bound);
        t.y = (int)(u[4 * k + 1] - bound);
        t.z = (int)(u[4 * k + 2] - bound);
        t.w = (int)(u[4 * k + 3] - bound);
        mx = max(max(mx, max(u[4 * k + 0], u[4 * k + 1])), max(u[4 * k + 2], u[4 * k + 3]));
        *reinterpret_cast<int4 *>(stage + pad4(16 * lane + 4 * k)) = t;
    }
    return mx;
}

// the image (complete: the caller's wave_sync lies behind its last write) read transposed, a[k] = element r + L * k of polynomial
// p, and the forward passes on it: -> a[k] = output 16 r + k of polynomial p, not reduced (|a| < 2^38).  The wave-uniform table
// is taken from constant memory here, its pointer pinned in scalar registers (TabPtr).  The image is free once this returns.
template <int LOGD, bool FAST>
__device__ __forceinline__ void image_fwd16(const int32_t *stage, double (&a)[16], double *row, int p, int r, const double2 *s_tw,
                                            const FzTwA *tab, const FzMod &m) {
    constexpr int D = Geom<LOGD>::D, L = Geom<LOGD>::L;
    {
        int x[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) x[k] = stage[pad4(p * D + r + L * k)];
#pragma unroll
        for (int k = 0; k < 16; ++k) a[k] = (double)x[k];
    }
    wave_sync();
    TabPtr t = (TabPtr)tab;
    asm volatile("" : "+s"(t));
    fwd16_passes<LOGD, FAST>(a, row, r, s_tw, t[0], m);
}

// acc[k] += cent(a[k] * x[k]) for the 16 outputs image_fwd16 leaves and the 16 multipliers x = al[0].x .. al[3].w.  The
// multipliers are any int32: |a * x| < 2^69 is inside fz_mulmod's bound, its result within 2^18 of q/2, and fz_cent makes it
// canonical, |p| <= (q-1)/2 < 2^31 -- so fp64 sums of fewer than 2^22 of them are exact.
__device__ __forceinline__ void mulacc16(double (&acc)[16], const double (&a)[16], const int4 (&al)[4], const FzMod &m) {
    const int x[16] = {al[0].x, al[0].y, al[0].z, al[0].w, al[1].x, al[1].y, al[1].z, al[1].w,
                       al[2].x, al[2].y, al[2].z, al[2].w, al[3].x, al[3].y, al[3].z, al[3].w};
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[k] += fz_cent(fz_mulmod(a[k], (double)x[k], m), m);
}

// a lane's 16 sums to LDS, where a workgroup's waves meet: doubles 18 * lane .. 18 * lane + 15 of the wave's region, i.e. element
// e = 16 * lane + k of the chunk at pad16(e), coefficient i of the wave's polynomial q at q * PS + pad16(i); the two pad doubles
// behind them are left alone
static_assert(Geom<6>::PPW * Geom<6>::PS == 18 * 64 && Geom<8>::PPW * Geom<8>::PS == 18 * 64,
              "a lane's 16 sums and their pad are a wave's region");
__device__ __forceinline__ void sums_to_lds(double *region, const double (&acc)[16], int lane) {
    double2 *blk = reinterpret_cast<double2 *>(region + 18 * lane);
#pragma unroll
    for (int k = 0; k < 8; ++k) blk[k] = make_double2(acc[2 * k], acc[2 * k + 1]);
}

// A kernel's opening on the transforms' LDS (lds16_doubles<LOGD>() doubles: a region per wave, then the per-lane twiddle table):
// the table copied in behind a workgroup barrier, and the wave's region with the pieces the steps above work on
template <int LOGD>
__device__ __forceinline__ const double2 *twiddles_to_lds(double *lds, const double2 *__restrict__ twB) {
    using G = Geom<LOGD>;
    double2 *s_tw = reinterpret_cast<double2 *>(lds + kWavesPerBlock * G::PPW * G::PS);
    for (int i = threadIdx.x; i < G::NE * G::L; i += 64 * kWavesPerBlock) s_tw[i] = twB[i];
    __syncthreads();
    return s_tw;
}
struct WaveLds {
    double *region;      // the wave's transpose region
    int32_t *stage;      // the int32 image at its start
    uint8_t *pk;         // the packed chunk behind the image
    int32_t *land;       // the same place as the landing area of a chunk requested straight into LDS
    double *row;         // the transpose buffer of the lane's polynomial p
};
template <int LOGD>
__device__ __forceinline__ WaveLds wave_lds(double *lds, int wave, int p) {
    using G = Geom<LOGD>;
    static_assert(landing_fits<LOGD>() && kLandOff * 4 == kPackOff, "the landing area is the packed chunk's place");
    double *region = lds + wave * G::PPW * G::PS;
    int32_t *stage = reinterpret_cast<int32_t *>(region);
    return {region, stage, reinterpret_cast<uint8_t *>(region) + kPackOff, stage + kLandOff, region + p * G::PS};
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

// (record, offset inside it) moved on by srec records and soff < rv values: an add, a compare and a select.  S is the caller's
// type of srec (size_t or unsigned): widened here, the sum srec + c comes out as other instructions in sign_encode.
template <class S>
__device__ __forceinline__ void rec_advance(size_t &rec, unsigned &off, S srec, unsigned soff, unsigned rv) {
    off += soff;                                          // < 2 * rv: no overflow, rv < 2^31
    const unsigned c = off >= rv ? 1u : 0u;
    rec += srec + c;
    off -= c * rv;
}

// the record of a lane's first value, walked along the wave's chunks: the divisions run once per wave (constructor), a step is
// rec_advance (per lane: the uniform state would compete with the transform's scalar operands)
struct RecPos {
    size_t rec;
    unsigned off;
};
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
    __device__ __forceinline__ void step() { rec_advance(rec, off, srec, soff, rv); }
    // where the walk stands after its next step, without stepping it
    __device__ __forceinline__ RecPos next() const {
        RecPos n = {rec, off};
        rec_advance(n.rec, n.off, srec, soff, rv);
        return n;
    }
};

// The chunk walk of a kernel whose wave-task is one chunk of a stream of `total` values: the wave's tasks are first, first +
// stride, .. below `tasks`.  The kernel takes its lane first (held here, sign_encode's prologue comes out in another order) and
// writes the peeled loop over the tasks itself, as fwd16_run explains it: run by a function here, the loop and the iteration no
// longer share their task + stride (docs/HISTORY.md section V).
struct ChunkTasks {
    int wave;                                             // uniform: readfirstlane says so (scalar address arithmetic)
    size_t tasks, first, stride;
    __device__ __forceinline__ explicit ChunkTasks(size_t total)
        : wave(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)), tasks((total + kChunk - 1) / kChunk),
          first((size_t)blockIdx.x * kWavesPerBlock + wave), stride((size_t)gridDim.x * kWavesPerBlock) {}
};
// its grid (host): a workgroup per kWavesPerBlock tasks, at most `cap` of them (the kernel's resident grid)
inline dim3 chunk_grid(size_t total, int cap) {
    const size_t tasks = (total + kChunk - 1) / kChunk, blocks = (tasks + kWavesPerBlock - 1) / kWavesPerBlock;
    return dim3((unsigned)(blocks < (size_t)cap ? blocks : (size_t)cap));
}

// The steps every producer of the bytes takes once its chunk's int32 image stands in the wave's region.  Each has the form that
// leaves its callers' code as it was with the text in place, or the callers say why not (docs/HISTORY.md section V).  Three
// steps stay with the kernels, each a few lines: the field width pinned per chunk with the stream's length, `bad` from the two
// halves, and fields_pack with the read-back of the packed chunk -- every form of a helper for them changes the callers' code.

// the operands of the range check: uniform, but VALU operands only (see RecWalk)
struct FieldBounds {
    unsigned two_b, wmask, bnd;
    __device__ __forceinline__ FieldBounds(int w, int bound)
        : two_b(2u * (unsigned)bound), wmask((unsigned)((1ull << w) - 1)), bnd((unsigned)bound) {
        asm volatile("" : "+v"(two_b), "+v"(wmask), "+v"(bnd));
    }
};

// a centred value z -> its field u = z + B, range-checked in the two-halves form: |z + B| < 2^32, the high word is all ones
// exactly when z < -B and the low word exceeds 2B exactly when z > B, so the lane's values are out of range exactly when
// hi != 0 || mx > two_b after the last of them.  A refused field stays inside its own w bits.
__device__ __forceinline__ uint32_t range_field(const long long &z, const FieldBounds &b, uint32_t &hi, uint32_t &mx) {
    const unsigned long long s = (unsigned long long)(z + (long long)b.bnd);
    hi |= (uint32_t)(s >> 32);
    mx = max(mx, (uint32_t)s);
    return (uint32_t)s & b.wmask;
}

// the inverse passes on a[k] = value 16 * lane + k of the image (image_to_doubles; the caller's wave_sync lies behind the read)
// and their outputs, element r + L * k of polynomial p, centred into the image.  The wave-uniform table is taken from constant
// memory, its pointer pinned (TabPtr); `transposed` is inv16_passes' hook.
template <int LOGD, bool FAST, class HOOK = NoHook>
__device__ __forceinline__ void inv16_to_image(double (&a)[16], const WaveLds &W, int p, int r, const double2 *s_tw, TabPtr t,
                                               const FzMod &m, const HOOK &transposed = HOOK()) {
    constexpr int D = Geom<LOGD>::D, L = Geom<LOGD>::L;
    asm volatile("" : "+s"(t));
    inv16_passes<LOGD, FAST>(a, W.row, r, s_tw, t[0], m, transposed);
#pragma unroll
    for (int k = 0; k < 16; ++k) W.stage[pad4(p * D + r + L * k)] = (int)fz_cent(a[k], m);
}

// the packed chunk to the stream, and `code` to the status word of the lane's record where `bad` (lanes with values only)
__device__ __forceinline__ void store_and_flag(uint8_t *out, size_t task, size_t total, size_t total_bytes, int w, int lane,
                                               const Packed &o, int *status, size_t rec, bool bad, int code) {
    packed_store(out, task, total_bytes, w, lane, o);
    const bool valid = task * kChunk + 16 * lane < total;
    records_flag(status, rec, bad && valid, code, lane);
}

}  // namespace

#endif
