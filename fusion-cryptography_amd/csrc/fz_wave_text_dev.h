// fz_wave_text_dev.h -- what the kernels that write decimal text with one wave share (fz_challenge_text_dev.h, fz_hash_ag.hip): the
// wave's own barrier and the length of an integer's decimal.  Device code; private to the unit that includes it.
#ifndef FZ_WAVE_TEXT_DEV_H
#define FZ_WAVE_TEXT_DEV_H

namespace {

// what one lane wrote to LDS before, every lane of the WAVE reads after (the waves of a workgroup never synchronise with each other)
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ int dec_len(int v) {          // len(str(v)) for an int32
    unsigned u = v < 0 ? 0u - (unsigned)v : (unsigned)v;
    int n = (v < 0) ? 2 : 1;
    n += u >= 10u; n += u >= 100u; n += u >= 1000u; n += u >= 10000u; n += u >= 100000u; n += u >= 1000000u;
    n += u >= 10000000u; n += u >= 100000000u; n += u >= 1000000000u;
    return n;
}

}  // namespace

#endif
