// packed_arith.h -- what the integer linear maps across slot-packed ciphertexts share (packed.hip: fhe_block8x8_scalar, fhe_channel_mix;
// planemap.hip: fhe_plane_map): the scalar rule, the Shoup pairs of a scalar, the lazy / canonical product and the host checks.
#pragma once
#include "internal.h"

struct PkMods { u64 q[FHE_MAX_K]; };                               // by value (wave-uniform)

template <bool LAZY>
struct PkArith {
    u64 q, nq;
    u32 zero;
    __device__ __forceinline__ PkArith(u64 q_) : q(q_), nq(0 - q_), zero(LAZY ? fhe_opaque_zero : 0) {}
    // x w mod q + {0 .. 3} q (LAZY) or canonical, for any 64-bit x
    __device__ __forceinline__ u64 mul(u64 x, ulonglong2 w) const {
        if constexpr (LAZY) return mul_shoup_lazy4(x, w.x, w.y, nq, zero);
        else return mul_shoup(x, w.x, w.y, q);
    }
    // [0, 4q) -> [0, q).  Behind post every interval up to the product's largest excess occurs.  Behind the product by 1 of a sum
    // below 32q the subtraction is still needed: a sum that is a multiple of q comes back as exactly q (every j q, j = 1 .. 31, on
    // every prime: whenever an output is 0), and on the 36/37-bit primes other sums come back in [q, 2q) too; on the 54- to 58-bit
    // primes a seeded search of 2^18 sums per prime found the product by 1 canonical everywhere else (observed, not proved).
    // DESIGN.md 3.12.1 has the table.
    __device__ __forceinline__ u64 canon(u64 x) const {
        if constexpr (LAZY) return csub(csub(x, 2 * q), q);
        else return x;
    }
};

// The table reads are scalar loads with a wave-uniform address.  Left alone, the compiler shares and clusters them across a whole pass
// (64 pairs = 256 SGPRs per matrix: hundreds of spills); adding a zero it cannot see through to the pointer before each output makes every
// output load the eight pairs it uses, next to their use -- 16 KiB of scalar-cache traffic per wave against 64 KiB of vector traffic.
template <typename P>
__device__ __forceinline__ const P *fresh(const P *p) {
    int off = 0;
    asm volatile("" : "+v"(off));
    return p + __builtin_amdgcn_readfirstlane(off);
}

// |w| <= min((t - 1) / 2, 2^31 - 1): the centred lift of w mod t is w itself
static inline bool scalar_ok(const fhe_ctx *c, int64_t w) {
    const u64 a = w < 0 ? (u64)0 - (u64)w : (u64)w;
    return a <= (c->t - 1) / 2 && a <= 0x7fffffffULL;
}
static inline ulonglong2 lift_pair(int64_t w, u64 q) {
    const u64 a = (w < 0 ? (u64)0 - (u64)w : (u64)w) % q;
    const u64 r = (w < 0 && a) ? q - a : a;
    return make_ulonglong2(r, (u64)(((unsigned __int128)r << 64) / q));
}
static inline bool lazy_ok(const fhe_ctx *c) { return c->max_prime_bits <= 58 && !c->opt.ntt_nopm; }
static inline PkMods pk_mods(const fhe_ctx *c) {
    PkMods M{};
    for (u32 i = 0; i < c->k; i++) M.q[i] = c->qb.primes[i];
    return M;
}
