// ksp_core.h -- what keyswitch_sp.hip and rotsum.hip share of the key switch with a special prime: the per-call constant table, the index
// map of sigma_g, the reduction of a 64-bit value and the drop of the special prime on one coefficient.  Moved here from keyswitch_sp.hip
// as they were; the entry points below are keyswitch_sp.hip's own kernels behind host functions, for rotsum.hip.
#pragma once
#include "internal.h"

// per-call constants by value (wave-uniform): every prime with floor(2^64 / q), and for r < L the pair (m = k - 1, r) of ctx->modswitch
struct KspTab {
    u64 q[FHE_MAX_K], r64[FHE_MAX_K];
    ulonglong2 inv[FHE_MAX_K];      // p^-1 mod q_r with its Shoup companion
    u64 add[FHE_MAX_K];             // (h mod q_r) + the smallest multiple of q_r that is >= p
    u64 p, h;                       // the special prime, floor(p / 2)
};

__device__ __forceinline__ u32 gal_src(u32 j, u32 ginv, u32 n, bool &neg) {      // j < n <= 2^14, ginv < 2n: no overflow
    const u32 s = (j * ginv) & (2 * n - 1);
    neg = s >= n;
    return s & (n - 1);
}
__device__ __forceinline__ u64 gal_load(const u64 *__restrict__ p, u32 j, u32 ginv, u32 n, u64 q) {
    bool neg;
    const u64 v = p[gal_src(j, ginv, n, neg)];
    return neg ? negmod(v, q) : v;
}
__device__ __forceinline__ u64 reduce64(u64 x, u64 q, u64 r64) {   // x mod q for any x < 2^64
    u64 r = x - __umul64hi(x, r64) * q;
    r = csub(r, 2 * q);
    return csub(r, q);
}
// one drop of fhe_mod_switch on one coefficient: x = acc_r in [0, q_r), cp = acc_p in [0, p); x + A - rr < 2^63 for primes below 2^61
__device__ __forceinline__ u64 ksp_drop(u64 x, u64 cp, const KspTab &T, u32 r) {
    const u64 rr = csub(cp + T.h, T.p);
    return mul_shoup(x + T.add[r] - rr, T.inv[r].x, T.inv[r].y, T.q[r]);
}
static inline dim3 ksp_grid2(u32 n, u64 rows) { return dim3((n + 255) / 256, (unsigned)(rows < 32768 ? (rows ? rows : 1) : 32768)); }

static inline KspTab ksp_tab(const fhe_ctx *c) {
    KspTab T{};
    const u32 k = c->k, m = k - 1;
    for (u32 i = 0; i < k; i++) {
        T.q[i] = c->qb.primes[i];
        T.r64[i] = (u64)(((unsigned __int128)1 << 64) / T.q[i]);
    }
    for (u32 r = 0; r < m; r++) {
        T.inv[r] = c->modswitch.inv[m * (m - 1) / 2 + r];
        T.add[r] = c->modswitch.add[m * (m - 1) / 2 + r];
    }
    T.p = T.q[m];
    T.h = T.p >> 1;
    return T;
}

// keyswitch_sp.hip, for rotsum.hip.  fhe_ksp_pm_ok: do the pseudo-Mersenne kernels run for `count` ciphertexts of this context.
bool fhe_ksp_pm_ok(const fhe_ctx *c, u64 count);
// dig [count][L][k][n] = NTT_(q_r)([c_(src_poly),i]_(q_r)): the first step of a relinearisation (k_ksp_fwd_pm<L, C, false>, or k_ksp_digits
// and the base's own transforms), on the path fhe_ksp_pm_ok names
int fhe_ksp_forward(const fhe_ctx *c, const u64 *ct, u64 stride, u32 src_poly, u64 *dig, u64 count, hipStream_t st);
// pseudo-Mersenne path only.  acc [rows][k][n] (NTT form, below PM_FOLDED / 16 q): the special prime's row in canonical coefficients -> sp [rows][n]
int fhe_ksp_inv_sp(const fhe_ctx *c, const u64 *acc, u64 *sp, u64 rows, hipStream_t st);
// pseudo-Mersenne path only: k_ksp_inv_down_add_pm<L, C, true> on acc [count][2][k][n] and sp [count][2][n]
int fhe_ksp_inv_down_add_galois(const fhe_ctx *c, const u64 *ct, u64 stride, u64 *out, u64 out_stride, const u64 *acc, const u64 *sp, u32 ginv, u64 count,
                                hipStream_t st);
