// reduce128.h -- (hi 2^64 + lo) mod q for ANY 64-bit hi and lo: the 128-bit draws of the seeded expansion (encrypt.hip k_seed_expand /
// k_enc_sym_fused).  Host and device, and no HIP header: a plain C++ compiler builds the host side, which is how
// tests/test_seeded_cpu.py drives the reduction at its operands' edges against unsigned __int128 -- the cipher's outputs cannot be prescribed.
#pragma once
#include <stdint.h>

typedef unsigned long long u64;
typedef unsigned int u32;

struct Modulus {
    u64 q;      // prime < 2^61
    u64 mu;     // floor(2^(2b) / q), b = bit length of q  (b <= 61, so mu < 2^62)
    u32 s1;     // b - 1
    u32 s2;     // b + 1
};

#if defined(__HIPCC__)
#define FHE_HD __host__ __device__ __forceinline__
#else
#define FHE_HD inline
#endif

FHE_HD u64 fhe_mulhi64(u64 a, u64 b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (u64)(((unsigned __int128)a * b) >> 64);
#endif
}
// z mod q for z = hi 2^64 + lo < 2^(2b): the reduction of mul_barrett (modarith.h) on a given z.  x = floor(z / 2^(b-1)) < 2^(b+1) -- hi is
// below 2^(2b-64) <= 2^(b-3), so the shift loses no bit --, qhat = floor(x mu / 2^(b+1)) in [Q - 2, Q], z - qhat q in [0, 3q).
FHE_HD u64 barrett128(u64 hi, u64 lo, const Modulus &m) {
    const u64 x = (hi << (64 - m.s1)) | (lo >> m.s1);
    const u64 plo = x * m.mu, phi = fhe_mulhi64(x, m.mu);
    const u64 qhat = (phi << (64 - m.s2)) | (plo >> m.s2);
    u64 r = lo - qhat * m.q;
    r = r >= 2 * m.q ? r - 2 * m.q : r;
    return r >= m.q ? r - m.q : r;
}
// any hi, lo; result in [0, q).  Needs q >= 2^32 (b >= 33; the entry points refuse smaller primes): three values below 2^(2b) go through
// barrett128 -- hi itself (2^64 <= 2^(2b)), then twice r 2^32 + (32 bits of lo) with r < q (below 2^(b+32) <= 2^(2b)).
FHE_HD u64 reduce128(u64 hi, u64 lo, const Modulus &m) {
    u64 r = barrett128(0, hi, m);
    r = barrett128(r >> 32, (r << 32) | (lo >> 32), m);
    return barrett128(r >> 32, (r << 32) | (lo & 0xffffffffULL), m);
}
