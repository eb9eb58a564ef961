// rotdiag_core.h -- what rotsum.hip, rotdiag.hip and rotbsgs.hip share of the hoisted special-prime rotations: the arithmetic policy of
// their two paths, the inner term of every accumulation kernel, the bounds of its lazy sums, and the steps that rotdiag.hip defines once
// behind host functions (the pattern of ksp_core.h): the forward and the drop step of the diagonal and baby-step / giant-step maps, and
// the two halves of plan creation.
#pragma once
#include "ksp_core.h"

// ---- the arithmetic of one path: the same members, canonical Barrett residues or lazy pseudo-Mersenne sums over class C --------------
struct ArBarrett {
    using Mod = Modulus;
    using Tab = const Modulus *;
    static __device__ __forceinline__ Mod mod(Tab t, u32 r) { return t[r]; }
    static __device__ __forceinline__ u64 mul(u64 a, u64 b, const Mod &m) { return mul_barrett(a, b, m); }
    static __device__ __forceinline__ u64 add(u64 a, u64 b, const Mod &m) { return addmod(a, b, m.q); }
    static __device__ __forceinline__ u64 fold(u64 a, const Mod &) { return a; }
};
template <typename C> struct ArPm {
    using Mod = PmMod;
    using Tab = RnsBase;
    static __device__ __forceinline__ Mod mod(const Tab &t, u32 r) { return t.pm[r]; }
    static __device__ __forceinline__ u64 mul(u64 a, u64 b, const Mod &m) { return mulvv_pm(a, b, m); }      // below RQ / 16 q
    static __device__ __forceinline__ u64 add(u64 a, u64 b, const Mod &) { return a + b; }
    static __device__ __forceinline__ u64 fold(u64 a, const Mod &m) { return fold_pm(a, m); }               // below PM_FOLDED / 16 q
};

// The lazy sums of ArPm, in sixteenths of q (4 LIM = 2^64 / q rounded down to a power of two).  A term is a mulvv_pm result below RQ; a
// sum is folded every ROT_FOLD_TERMS terms at the latest.  RQ is the figure the host checks mulvv_pm's result against, and it is what the
// kernels' range proofs rest on.
constexpr int ROT_FOLD_TERMS = 32;
template <typename C> constexpr bool rot_bounds_ok() {
    return FHE_MAX_K * C::RQ <= 4 * C::LIM                       // a tap's L + 1 <= FHE_MAX_K terms (L digit products, the C0 product) fit 64 bits
           && PM_FOLDED <= 32                                    // a folded value is a valid first operand of mulvv_pm (below 2^(b+1))
           && PM_FOLDED + ROT_FOLD_TERMS * C::RQ <= 4 * C::LIM;  // a folded sum and ROT_FOLD_TERMS more products fit 64 bits
}
static_assert(rot_bounds_ok<PmA>() && rot_bounds_ok<PmB>(), "lazy tap sums");

// a0 / a1 += sum_(l < L) dig[l][r][src] * key[l][pp][r][s].  dig: word src of row r of the first digit, [L][k][n]; key: word s of row r
// of the first key polynomial, [L][2][k][n]; kn = k n <= FHE_MAX_K 2^14, so every row offset fits 32 bits (and k_bs_baby keeps its 8
// waves per SIMD).  Gathered 8-byte reads of rows that stay in L2 across the taps.
template <typename A>
__device__ __forceinline__ void rot_digit_sum(const u64 *__restrict__ dig, const u64 *__restrict__ key, u32 Lq, u32 kn, const typename A::Mod &m, u64 &a0, u64 &a1) {
    for (u32 l = 0; l < Lq; l++) {
        const u64 x = dig[l * kn];
        const u64 *e = key + l * 2 * kn;
        a0 = A::add(a0, A::mul(x, e[0], m), m);
        a1 = A::add(a1, A::mul(x, e[kn], m), m);
    }
}
// T_j,pp,r[s] of one tap (rotdiag.hip), unfolded: the digit sum (key non-null: word s of row r), for r < L the gathered C0 word against
// pr = [p]_(q_r) (pp = 0) and, on the tap with g = 1 (key null), [p] D_r,r (pp = 1).  dig: row r of the ciphertext's first digit;
// c0: row r of its C0.  At most L + 1 terms below RQ each: rot_bounds_ok.
template <typename A>
__device__ __forceinline__ void rot_tap_term(const u64 *__restrict__ dig, const u64 *__restrict__ c0, const u64 *__restrict__ key, u32 src, u32 r, u32 Lq, u32 kn,
                                             u64 pr, const typename A::Mod &m, u64 &a0, u64 &a1) {
    a0 = a1 = 0;
    if (key) rot_digit_sum<A>(dig + src, key, Lq, kn, m, a0, a1);      // uniform: every tap but the one with g = 1
    if (r < Lq) {                                                      // uniform per row
        a0 = A::add(a0, A::mul(c0[src], pr, m), m);
        if (!key) a1 = A::mul(dig[r * kn + src], pr, m);
    }
}

// ---- rotdiag.hip, for rotbsgs.hip and rotsum.hip ----------------------------------------------------------------------------------------
// The path of a call: the call checks bound every launch size below fhe_ksp_pm_ok's own limit, so the context alone decides, and every
// step of a call and fhe_ksp_forward inside it agree
static inline bool fhe_rot_pm(const fhe_ctx *c) { return fhe_ksp_pm_ok(c, 1); }
// The forward step: dig [count][L][k][n] = the digit transforms of c_1, c0h [count][k][n] = NTT_(q_r)(c_0,r) (the special prime's row is
// written, as zeros, by the general path alone).  k_rd_fwd_pm, or k_rd_stage_c0, the base's own transform and fhe_ksp_forward.
int fhe_rot_forward(const fhe_ctx *c, const u64 *ct, u64 stride, u64 *dig, u64 *c0h, u64 count, hipStream_t st);
// The drop step on acc [rows][k][n] in NTT form: row = c * 2 + pp goes to out + c * out_stride + (pp L + r) n, one drop of fhe_mod_switch.
// fhe_ksp_inv_sp into sp [rows][n] and k_rd_inv_down_pm (acc is only read), or fhe_qbase_ntt(true) IN PLACE and k_rd_down (sp unused).
int fhe_rot_drop(const fhe_ctx *c, u64 *acc, u64 *sp, u64 *out, u64 out_stride, u64 rows, hipStream_t st);
// Plan creation.  d [rows + 1][k][n] on the device, rows 0 .. rows - 1 the caller's: X goes into the last row, ONE run of the context's own
// forward transform over all of them (null stream), and the last row gives f [n], the slot exponents relative to slot 0, cross-checked over
// every prime.  what: the rows' name in the two HIP failure messages
int fhe_rot_slot_exponents(const fhe_ctx *c, u64 *d, u32 rows, const char *what, std::vector<u32> &f);
// perm [count][n]: slot s of pi_(g_j) reads slot perm[j][s]; keys [count]: the device pointer of the key of g_j, 0 for g_j = 1
int fhe_rot_perm_keys(const std::vector<u32> &f, u32 count, const u32 *elts, const uint64_t *const *d_keys, u32 *perm, u64 *keys);
