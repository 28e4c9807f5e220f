// fz_vk_order_key.h -- the text order of str(OneTimeVerificationKey) WITHOUT the text, written once for the device sort
// (fz_vk_order.hip) and for host code that checks it (tests/test_vk_order_host.py).
//
// Every str(vk) (put_vk, fz_host.cpp) is fixed text, the left row's "v0, v1, ..., v(d-1)]", fixed text, the right row's values in
// the same form, fixed text.  Two keys therefore compare like the FIRST coefficient (left row first) whose values differ -- the
// decimal of an int32 names it, so equal texts are equal values -- and two different decimals compare by code point:
//   * '-' (0x2d) is below every digit: a negative value sorts first, and two negative values by their DIGITS, not by value;
//   * where one decimal is a prefix of the other, what follows the shorter one decides: ", " inside a row (',' = 0x2c is below
//     every digit: "12" before "123"), "]" behind a row's last value (']' = 0x5d is above every digit: "123" before "12").
// fz_vk_text_key packs that into an integer whose plain comparison is the text's: bit 40 = "not negative", then the digits, most
// significant first, as nibbles 1..10 from bit 36 down, the unused nibbles 0 (inside a row) or 11 (a row's last value).
#ifndef FZ_VK_ORDER_KEY_H
#define FZ_VK_ORDER_KEY_H

#include <stdint.h>

#if defined(__HIPCC__)
#define FZ_VK_HD __host__ __device__ __forceinline__
#else
#define FZ_VK_HD inline
#endif

FZ_VK_HD uint64_t fz_vk_text_key(int32_t v, bool last) {
    uint32_t u = v < 0 ? 0u - (uint32_t)v : (uint32_t)v;
    uint64_t k = 0;
    int n = 0;
    do {                                                     // the least significant digit first: it ends at nibble 10 - n
        const uint32_t q = u / 10u;
        k = (k >> 4) | ((uint64_t)(u - q * 10u + 1u) << 36);
        u = q;
        ++n;
    } while (u);
    if (last) k |= 0xbbbbbbbbbbull & (((uint64_t)1 << (4 * (10 - n))) - 1);
    return k | ((uint64_t)(v >= 0) << 40);
}

// keys a and b as rows [2][d] (left row, right row; 16-byte aligned, d a power of two >= 4): -1, 0 or 1 as str(a) <, ==, > str(b)
FZ_VK_HD int fz_vk_text_cmp(const int32_t *a, const int32_t *b, int d) {
    a = (const int32_t *)__builtin_assume_aligned(a, 16);
    b = (const int32_t *)__builtin_assume_aligned(b, 16);
    const int n = 2 * d;
    int c = 0, pos = -1;
    int32_t va = 0, vb = 0;
    for (; pos < 0 && c + 16 <= n; c += 16) {                // sixteen values of each row in flight
        int32_t x[16], y[16];
#pragma unroll
        for (int t = 0; t < 16; ++t) { x[t] = a[c + t]; y[t] = b[c + t]; }
#pragma unroll
        for (int t = 15; t >= 0; --t)
            if (x[t] != y[t]) { pos = c + t; va = x[t]; vb = y[t]; }
    }
    for (; pos < 0 && c < n; c += 4) {                       // (degree 4: rows of eight values)
        int32_t x[4], y[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) { x[t] = a[c + t]; y[t] = b[c + t]; }
#pragma unroll
        for (int t = 3; t >= 0; --t)
            if (x[t] != y[t]) { pos = c + t; va = x[t]; vb = y[t]; }
    }
    if (pos < 0) return 0;
    const bool last = (pos & (d - 1)) == d - 1;
    return fz_vk_text_key(va, last) < fz_vk_text_key(vb, last) ? -1 : 1;
}

#endif
