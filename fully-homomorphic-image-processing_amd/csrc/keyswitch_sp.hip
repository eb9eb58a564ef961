// keyswitch_sp.hip -- key switching with a special prime (the RNS-only decomposition SEAL moved to after 2.3): fhe_relinearize_sp_poly and
// fhe_apply_galois_sp on gfx950.  include/fhe_hip.h states the operations; DESIGN.md 3.14 has the resource table and the measurements.
//
// The context has k primes; the last one, p = q_(k-1), is the special prime.  Ciphertexts live on the first L = k - 1 primes, keys on all k.
// With d the source polynomial (c_src_poly, or sigma_g(c_1)) and K = [L][2][k][n] the key in NTT form:
//     acc_pp,r = sum_(i < L) [d_i]_(q_r) (*) K_i,pp,r  mod q_r           for every r < k  ([d_i]_(q_r): the integer d_i in [0, q_i) reduced modulo q_r)
//     u_pp     = one drop of fhe_mod_switch (k -> k - 1) of acc_pp       (modswitch.hip: rr = (acc_p + h) mod p, (acc_r + A - rr) p^-1 mod q_r)
//     out      = (c_0 + u_0, c_1 + u_1)   or   (sigma_g(c_0) + u_0, u_1)
// L k forward transforms and 2 k inverse ones where the bit decomposition takes k nd k and 2 k; no digit width, the added noise is that of
// one rounding plus L n B q_max / p.
//
// Pseudo-Mersenne bases (the hot path), four launches:
//   k_ksp_fwd_pm       workgroup (c, i, r): d_i (through sigma_g for a rotation), folded below (17/16) q_r when r != i, forward transform mod q_r
//   k_ksp_accum_pm     per (c, r, slot): two integer sums of L mulvv_pm terms, one fold each
//   k_ksp_inv_sp_pm    workgroup (c, pp): the special prime's accumulator back to canonical coefficients ([count][2][n] of scratch)
//   k_ksp_inv_down_add_pm  workgroup (c, pp, r < L): inverse transform, the drop with the special prime's coefficients of the thread's own
//                      sixteen positions, the addition of c_pp / sigma_g(c_0), the store into the [2][L][n] output: u_pp never exists in memory
// General path (FP64-transform bases, 61-bit primes, FHE_NTT_NOPM=1): k_ksp_digits, fhe_qbase_ntt, k_ksp_accum, fhe_qbase_ntt, k_ksp_down_add --
// element-wise grids around the base's own transforms.  Every quantity is the canonical residue of the same integer on both paths: the same bits.
//
// In place (out2 == ct, same stride): the source polynomial is consumed by the first kernel; the last one reads c_pp,r at exactly the words
// it then writes (relinearise), or takes sigma_g(c_0,r) through LDS AFTER its transform, as k_galois_inv_add_pm does: every global read of
// the polynomial has landed before the barrier in front of the first store, and no other workgroup writes that polynomial.
//
// The index map of sigma_g and reduce64 are galois.hip's (file-local there); they are restated in ksp_core.h, which rotsum.hip shares, so
// that galois.hip stays as it is.
#include "ksp_core.h"

#include "host_math.h"

namespace {

// ---- general path -------------------------------------------------------------------------------------------------------------------
// dig [count][L][k][n]: d_i reduced to every q_r; a rotation also stores sigma(c0_i) beside the digits (a block's gathered reads cross other
// blocks' writes on an element-wise grid, so the last kernel cannot read c0 itself when the call runs in place)
template <bool GAL>
__global__ __launch_bounds__(256) void k_ksp_digits(const u64 *__restrict__ ct, u64 stride, u64 *__restrict__ dig, u64 *__restrict__ s0, KspTab T, u32 k, u32 n,
                                                    u32 src_poly, u32 ginv, u64 count) {
    const u32 Lq = k - 1;
    for (u64 u = blockIdx.y; u < count * Lq; u += gridDim.y) {
        const u32 i = (u32)(u % Lq);
        const u64 c = u / Lq;
        const u64 *src = ct + c * stride + ((u64)src_poly * Lq + i) * n, *c0 = ct + c * stride + (u64)i * n;
        for (u32 j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
            const u64 v = GAL ? gal_load(src, j, ginv, n, T.q[i]) : src[j];
            for (u32 r = 0; r < k; r++) dig[(u * k + r) * n + j] = reduce64(v, T.q[r], T.r64[r]);
            if (GAL) s0[u * n + j] = gal_load(c0, j, ginv, n, T.q[i]);
        }
    }
}
// acc[c][pp][r][s] = sum_i dig[c][i][r][s] * key[i][pp][r][s], canonical Barrett products
__global__ __launch_bounds__(256) void k_ksp_accum(const u64 *__restrict__ dig, const u64 *__restrict__ key, u64 *__restrict__ acc, const Modulus *__restrict__ mod,
                                                   u32 k, u32 n, u64 count) {
    const u32 Lq = k - 1;
    for (u64 u = blockIdx.y; u < count * k; u += gridDim.y) {
        const u32 r = (u32)(u % k);
        const u64 c = u / k;
        const Modulus m = mod[r];
        for (u32 s = blockIdx.x * blockDim.x + threadIdx.x; s < n; s += gridDim.x * blockDim.x) {
            u64 a0 = 0, a1 = 0;
            for (u32 i = 0; i < Lq; i++) {
                const u64 x = dig[((c * Lq + i) * k + r) * n + s];
                const u64 *e = key + (((u64)i * 2) * k + r) * n + s;
                a0 = addmod(a0, mul_barrett(x, e[0], m), m.q);
                a1 = addmod(a1, mul_barrett(x, e[(u64)k * n], m), m.q);
            }
            acc[((c * 2 + 0) * k + r) * n + s] = a0;
            acc[((c * 2 + 1) * k + r) * n + s] = a1;
        }
    }
}
// acc in coefficient form: the drop of the special prime and the addition; each thread reads and writes the same words of ct / out
template <bool GAL>
__global__ __launch_bounds__(256) void k_ksp_down_add(const u64 *ct, u64 stride, u64 *out, u64 out_stride, const u64 *__restrict__ acc, const u64 *__restrict__ s0,
                                                      KspTab T, u32 k, u32 n, u64 count) {
    const u32 Lq = k - 1;
    for (u64 u = blockIdx.y; u < count * 2 * Lq; u += gridDim.y) {
        const u32 r = (u32)(u % Lq), pp = (u32)((u / Lq) & 1);
        const u64 c = u / (2 * Lq);
        const u64 *a = acc + ((c * 2 + pp) * k + r) * n, *ap = acc + ((c * 2 + pp) * k + Lq) * n;
        const u64 *src = GAL ? s0 + (c * Lq + r) * n : ct + c * stride + ((u64)pp * Lq + r) * n;
        u64 *dst = out + c * out_stride + ((u64)pp * Lq + r) * n;
        for (u32 j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
            const u64 v = ksp_drop(a[j], ap[j], T, r);
            dst[j] = (GAL && pp) ? v : addmod(v, src[j], T.q[r]);
        }
    }
}

// ---- pseudo-Mersenne path -------------------------------------------------------------------------------------------------------------
// (1) workgroup (c, i, r): dig[c][i][r] = NTT_(q_r)([d_i]_(q_r)).  r == i: d_i < q_i is below PM_FOLDED / 16 q_i as it is.  r != i: d_i is any
// value below 2^61 (the base may mix prime sizes in both directions); fold_pm brings ANY 64-bit value to d_i mod q_r + {0, 1} q_r, below
// (17/16) q_r = PM_FOLDED (fhe_build_base checks 2^b + 2^(64-b) delta against that bound for every prime of a pseudo-Mersenne base), which is
// ntt_fwd_regs_pm's entry bound E0 <= C::LIM.  The negation of sigma_g is modulo the SOURCE prime q_i, before the fold.
template <int L, typename C, bool GAL>
__global__ __launch_bounds__(NttShape<L>::TP, 4) void k_ksp_fwd_pm(const u64 *__restrict__ ct, u64 stride, u64 *__restrict__ dig, RnsBase base, u32 src_poly, u32 ginv) {
    __shared__ u64 lds[NttShape<L>::LDS_WORDS];
    constexpr int N = NttShape<L>::N, TP = NttShape<L>::TP;
    const int tid = threadIdx.x;
    const u32 k = base.count, Lq = k - 1, r = blockIdx.x % k, i = (blockIdx.x / k) % Lq;
    const u64 c = blockIdx.x / (k * Lq);
    const PmMod m = base.pm[r];
    const u64 *src = ct + c * stride + ((u64)src_poly * Lq + i) * N;
    u64 x[1][16];
    if constexpr (GAL) {
        const u64 qi = base.pm[i].q;
#pragma unroll
        for (int e = 0; e < 16; e++) x[0][e] = gal_load(src, (u32)(e * TP + tid), ginv, N, qi);
    } else {
        load_coeff<L>(x[0], src, tid);
    }
    if (r != i) {                                  // uniform per workgroup
#pragma unroll
        for (int e = 0; e < 16; e++) x[0][e] = fold_pm(x[0][e], m);
    }
    ntt_fwd_regs_pm<L, 1, PM_FOLDED, C::LIM, C::CS>(x, base.tw_pm + (size_t)r * N, m, lds, tid);
#pragma unroll
    for (int e = 0; e < 16; e++) x[0][e] = canon_pm(x[0][e], m);
    store_slots<L>(x[0], dig + (u64)blockIdx.x * N, tid);
}
// (2) acc[c][pp][r][s] = sum_(i < L) dig * key as integers, one fold: L <= 7 terms below RQ each (42 q < 2^61 on class A, 10.5 q < 2^62 on
// class B), inside k_relin_accum_pm's 20-term bound
template <typename C>
__global__ __launch_bounds__(256) void k_ksp_accum_pm(const u64 *__restrict__ dig, const u64 *__restrict__ key, u64 *__restrict__ acc, RnsBase base, u32 n, u64 count) {
    const u32 k = base.count, Lq = k - 1;
    for (u64 u = blockIdx.y; u < count * k; u += gridDim.y) {
        const u32 r = (u32)(u % k);
        const u64 c = u / k;
        const PmMod m = base.pm[r];
        for (u32 s = blockIdx.x * blockDim.x + threadIdx.x; s < n; s += gridDim.x * blockDim.x) {
            u64 a0 = 0, a1 = 0;
            for (u32 i = 0; i < Lq; i++) {
                const u64 x = dig[((c * Lq + i) * k + r) * n + s];
                const u64 *e = key + (((u64)i * 2) * k + r) * n + s;
                a0 += mulvv_pm(x, e[0], m);
                a1 += mulvv_pm(x, e[(u64)k * n], m);
            }
            acc[((c * 2 + 0) * k + r) * n + s] = fold_pm(a0, m);
            acc[((c * 2 + 1) * k + r) * n + s] = fold_pm(a1, m);
        }
    }
}
// (3) workgroup (c, pp): the special prime's accumulator, coefficient form, canonical -> sp[c][pp][n]
template <int L, typename C>
__global__ __launch_bounds__(NttShape<L>::TP, 4) void k_ksp_inv_sp_pm(const u64 *__restrict__ acc, u64 *__restrict__ sp, RnsBase base) {
    __shared__ u64 lds[NttShape<L>::LDS_WORDS];
    constexpr int N = NttShape<L>::N;
    const int tid = threadIdx.x;
    const u32 k = base.count;
    const PmMod m = base.pm[k - 1];
    u64 x[1][16];
    load_slots<L>(x[0], acc + ((u64)blockIdx.x * k + (k - 1)) * N, tid);
    ntt_inv_regs_pm<L, 1, PM_FOLDED, C::XB, C::LIM, C::RQ>(x, base.itw_pm + (size_t)(k - 1) * N, m, lds, tid);
#pragma unroll
    for (int e = 0; e < 16; e++) x[0][e] = canon_rq_pm<C::RQ>(x[0][e], m);
    store_coeff<L>(x[0], sp + (u64)blockIdx.x * N, tid);
}
// (4) workgroup (c, pp, r < L): inverse transform of acc_pp,r, the drop, the addition, the store.  Everything beside the accumulator is
// loaded AFTER the transform (sixteen registers less are live through it).
template <int L, typename C, bool GAL>
__global__ __launch_bounds__(NttShape<L>::TP, 4) void k_ksp_inv_down_add_pm(const u64 *ct, u64 stride, u64 *out, u64 out_stride, const u64 *__restrict__ acc,
                                                                             const u64 *__restrict__ sp, RnsBase base, KspTab T, u32 ginv) {
    __shared__ u64 lds[NttShape<L>::LDS_WORDS];
    constexpr int N = NttShape<L>::N, TP = NttShape<L>::TP;
    const int tid = threadIdx.x;
    const u32 k = base.count, Lq = k - 1, r = blockIdx.x % Lq, pp = (blockIdx.x / Lq) & 1;
    const u64 cpp = blockIdx.x / Lq;               // c * 2 + pp
    const u64 c = cpp >> 1;
    const PmMod m = base.pm[r];
    u64 x[1][16], y[16];
    load_slots<L>(x[0], acc + (cpp * k + r) * N, tid);
    ntt_inv_regs_pm<L, 1, PM_FOLDED, C::XB, C::LIM, C::RQ>(x, base.itw_pm + (size_t)r * N, m, lds, tid);
    load_coeff<L>(y, sp + cpp * N, tid);
#pragma unroll
    for (int e = 0; e < 16; e++) x[0][e] = ksp_drop(canon_rq_pm<C::RQ>(x[0][e], m), y[e], T, r);
    if constexpr (GAL) {
        if (pp == 0) {                             // uniform per workgroup
            const u64 *c0 = ct + c * stride + (u64)r * N;
            __syncthreads();                       // the transform's last transpose has read the array
#pragma unroll
            for (int e = 0; e < 16; e++) lds[e * TP + tid] = c0[e * TP + tid];
            __syncthreads();                       // every global read of c0_r has landed: the store below may write it (in place)
#pragma unroll
            for (int e = 0; e < 16; e++) {
                bool neg;
                const u64 v = lds[gal_src((u32)elem_index<L - 4>(tid, e), ginv, N, neg)];
                x[0][e] = addmod(x[0][e], neg ? negmod(v, m.q) : v, m.q);
            }
        }
    } else {
        load_coeff<L>(y, ct + c * stride + ((u64)pp * Lq + r) * N, tid);
#pragma unroll
        for (int e = 0; e < 16; e++) x[0][e] = addmod(x[0][e], y[e], m.q);
    }
    store_coeff<L>(x[0], out + c * out_stride + ((u64)pp * Lq + r) * N, tid);
}

// the pseudo-Mersenne kernels run when the base has a class, the switch is off, the base's own transforms are not the FP64 ones
// (fhe_qbase_ntt) and the grid of the first kernel fits one launch
bool ksp_pm_ok(const fhe_ctx *c, u64 count) {
    const bool f64 = fhe_rgb_f64_supported(c) && !c->opt.force_u64;
    return c->qb.pm_class && !c->opt.ntt_nopm && !f64 && count * (c->k - 1) * c->k <= 0x7fffffffULL;
}

// src_poly: the source polynomial of a relinearisation step; 0 = a rotation (source sigma_g(c_1))
int key_switch(const fhe_ctx *c, const u64 *ct, u64 stride, u32 src_poly, u32 ginv, u64 *out2, u64 out_stride, u64 count, const u64 *key, u64 *scratch, hipStream_t st) {
    const u32 k = c->k, Lq = k - 1, n = c->n;
    const bool gal = src_poly == 0;
    const u32 sp_poly = gal ? 1 : src_poly;
    u64 *dig = scratch, *acc = dig + count * Lq * k * n, *aux = acc + count * 2 * k * n;      // aux: sp [count][2][n] or sigma(c0) [count][L][n]
    const KspTab T = ksp_tab(c);
    if (ksp_pm_ok(c, count)) {
        const RnsBase base = c->qb.dev();
#define GO_PM(CC)                                                                                                                                      \
    DISPATCH_L(c->logn, {                                                                                                                              \
        const unsigned g1 = (unsigned)(count * Lq * k), g3 = (unsigned)(count * 2), g4 = (unsigned)(count * 2 * Lq);                                   \
        if (gal) k_ksp_fwd_pm<L, CC, true><<<g1, NttShape<L>::TP, 0, st>>>(ct, stride, dig, base, sp_poly, ginv);                                     \
        else k_ksp_fwd_pm<L, CC, false><<<g1, NttShape<L>::TP, 0, st>>>(ct, stride, dig, base, sp_poly, ginv);                                        \
        k_ksp_accum_pm<CC><<<ksp_grid2(n, count * k), 256, 0, st>>>(dig, key, acc, base, n, count);                                                       \
        k_ksp_inv_sp_pm<L, CC><<<g3, NttShape<L>::TP, 0, st>>>(acc, aux, base);                                                                       \
        if (gal) k_ksp_inv_down_add_pm<L, CC, true><<<g4, NttShape<L>::TP, 0, st>>>(ct, stride, out2, out_stride, acc, aux, base, T, ginv);           \
        else k_ksp_inv_down_add_pm<L, CC, false><<<g4, NttShape<L>::TP, 0, st>>>(ct, stride, out2, out_stride, acc, aux, base, T, ginv);              \
    })
        if (c->qb.pm_class == 1) { GO_PM(PmA); } else { GO_PM(PmB); }
#undef GO_PM
        KERNEL_CHECK();
        return FHE_OK;
    }
    int rc;
    if (gal) k_ksp_digits<true><<<ksp_grid2(n, count * Lq), 256, 0, st>>>(ct, stride, dig, aux, T, k, n, sp_poly, ginv, count);
    else k_ksp_digits<false><<<ksp_grid2(n, count * Lq), 256, 0, st>>>(ct, stride, dig, aux, T, k, n, sp_poly, ginv, count);
    if ((rc = fhe_qbase_ntt(false, c, dig, dig, count * Lq, st))) return rc;
    k_ksp_accum<<<ksp_grid2(n, count * k), 256, 0, st>>>(dig, key, acc, c->qb.d_mod, k, n, count);
    if ((rc = fhe_qbase_ntt(true, c, acc, acc, count * 2, st))) return rc;
    if (gal) k_ksp_down_add<true><<<ksp_grid2(n, count * 2 * Lq), 256, 0, st>>>(ct, stride, out2, out_stride, acc, aux, T, k, n, count);
    else k_ksp_down_add<false><<<ksp_grid2(n, count * 2 * Lq), 256, 0, st>>>(ct, stride, out2, out_stride, acc, aux, T, k, n, count);
    KERNEL_CHECK();
    return FHE_OK;
}

// the checks both entry points share, in the order include/fhe_hip.h lists them; in_polys: polynomials of one input ciphertext that are read
int check_operands(const fhe_ctx *c, const void *ct, u64 stride, u32 in_polys, const void *out2, u64 out_stride, u64 count, const void *scratch, size_t scratch_bytes) {
    const u64 Ln = (u64)(c->k - 1) * c->n;
    if (stride < in_polys * Ln) return fail(FHE_ERR_PARAM, "ciphertext stride smaller than a size-%u ciphertext of %u primes", in_polys, c->k - 1);
    if (out_stride < 2 * Ln) return fail(FHE_ERR_PARAM, "output stride smaller than a size-2 ciphertext of %u primes", c->k - 1);
    if (!count) return FHE_OK;
    const size_t need = fhe_key_switch_sp_scratch_bytes(c, count);
    if (!scratch || scratch_bytes < need) return fail(FHE_ERR_PARAM, "scratch too small");
    const u64 in_words = (count - 1) * stride + in_polys * Ln, out_words = (count - 1) * out_stride + 2 * Ln;
    if (!(out2 == ct && out_stride == stride) && overlap(ct, in_words, out2, out_words))
        return fail(FHE_ERR_PARAM, "output range overlaps the input range (only out2 == ct with out_stride == stride may alias)");
    if (overlap(scratch, need / 8, ct, in_words) || overlap(scratch, need / 8, out2, out_words)) return fail(FHE_ERR_PARAM, "scratch overlaps the input or the output");
    return FHE_OK;
}

}  // namespace

// the pieces rotsum.hip runs as they are (ksp_core.h)
bool fhe_ksp_pm_ok(const fhe_ctx *c, u64 count) { return ksp_pm_ok(c, count); }
int fhe_ksp_forward(const fhe_ctx *c, const u64 *ct, u64 stride, u32 src_poly, u64 *dig, u64 count, hipStream_t st) {
    const u32 k = c->k, Lq = k - 1, n = c->n;
    if (ksp_pm_ok(c, count)) {
        const RnsBase base = c->qb.dev();
        const unsigned g1 = (unsigned)(count * Lq * k);
        if (c->qb.pm_class == 1) { DISPATCH_L(c->logn, (k_ksp_fwd_pm<L, PmA, false><<<g1, NttShape<L>::TP, 0, st>>>(ct, stride, dig, base, src_poly, 0))); }
        else { DISPATCH_L(c->logn, (k_ksp_fwd_pm<L, PmB, false><<<g1, NttShape<L>::TP, 0, st>>>(ct, stride, dig, base, src_poly, 0))); }
        KERNEL_CHECK();
        return FHE_OK;
    }
    k_ksp_digits<false><<<ksp_grid2(n, count * Lq), 256, 0, st>>>(ct, stride, dig, nullptr, ksp_tab(c), k, n, src_poly, 0, count);
    KERNEL_CHECK();
    return fhe_qbase_ntt(false, c, dig, dig, count * Lq, st);
}
int fhe_ksp_inv_sp(const fhe_ctx *c, const u64 *acc, u64 *sp, u64 rows, hipStream_t st) {
    const RnsBase base = c->qb.dev();
    if (c->qb.pm_class == 1) { DISPATCH_L(c->logn, (k_ksp_inv_sp_pm<L, PmA><<<(unsigned)rows, NttShape<L>::TP, 0, st>>>(acc, sp, base))); }
    else { DISPATCH_L(c->logn, (k_ksp_inv_sp_pm<L, PmB><<<(unsigned)rows, NttShape<L>::TP, 0, st>>>(acc, sp, base))); }
    KERNEL_CHECK();
    return FHE_OK;
}
int fhe_ksp_inv_down_add_galois(const fhe_ctx *c, const u64 *ct, u64 stride, u64 *out, u64 out_stride, const u64 *acc, const u64 *sp, u32 ginv, u64 count,
                                hipStream_t st) {
    const RnsBase base = c->qb.dev();
    const KspTab T = ksp_tab(c);
    const unsigned g4 = (unsigned)(count * 2 * (c->k - 1));
    if (c->qb.pm_class == 1) { DISPATCH_L(c->logn, (k_ksp_inv_down_add_pm<L, PmA, true><<<g4, NttShape<L>::TP, 0, st>>>(ct, stride, out, out_stride, acc, sp, base, T, ginv))); }
    else { DISPATCH_L(c->logn, (k_ksp_inv_down_add_pm<L, PmB, true><<<g4, NttShape<L>::TP, 0, st>>>(ct, stride, out, out_stride, acc, sp, base, T, ginv))); }
    KERNEL_CHECK();
    return FHE_OK;
}

extern "C" size_t fhe_ksk_sp_words(const fhe_ctx *c) {
    if (!c || c->k < 2) return 0;
    return (size_t)(c->k - 1) * 2 * c->k * c->n;
}

// the transformed source [L][k][n], the accumulators [2][k][n], and the larger of the special prime's coefficients [2][n] (pseudo-Mersenne
// path) and sigma(c0) [L][n] (general path, rotations) per ciphertext: enough for either path and either operation
extern "C" size_t fhe_key_switch_sp_scratch_bytes(const fhe_ctx *c, uint64_t count) {
    if (!c || c->k < 2) return 0;
    const u64 k = c->k, Lq = k - 1;
    return (size_t)(count * (Lq * k + 2 * k + (Lq > 2 ? Lq : 2)) * c->n * sizeof(u64));
}

extern "C" int fhe_relinearize_sp_poly(const fhe_ctx *c, const uint64_t *ct, uint64_t stride, uint32_t src_poly, uint64_t *out2, uint64_t out_stride, uint64_t count,
                                       const uint64_t *key, void *scratch, size_t scratch_bytes, fhe_stream s) {
    if (!c || !ct || !key || !out2) return fail(FHE_ERR_PARAM, "null argument");
    if (c->k < 2) return fail(FHE_ERR_PARAM, "a special-prime key switch needs a context of at least 2 primes (the last one is the special prime)");
    if (src_poly < 2 || src_poly >= FHE_MAX_POLYS) return fail(FHE_ERR_PARAM, "key-switch source polynomial %u out of range", src_poly);
    if (int rc = check_operands(c, ct, stride, src_poly + 1, out2, out_stride, count, scratch, scratch_bytes)) return rc;
    if (!count) return FHE_OK;
    return key_switch(c, (const u64 *)ct, stride, src_poly, 0, (u64 *)out2, out_stride, count, (const u64 *)key, (u64 *)scratch, (hipStream_t)s);
}

extern "C" int fhe_apply_galois_sp(const fhe_ctx *c, const uint64_t *ct2, uint64_t stride, uint64_t *out2, uint64_t out_stride, uint64_t count, uint32_t g,
                                   const uint64_t *key, void *scratch, size_t scratch_bytes, fhe_stream s) {
    if (!c || !ct2 || !key || !out2) return fail(FHE_ERR_PARAM, "null argument");
    if (c->k < 2) return fail(FHE_ERR_PARAM, "a special-prime key switch needs a context of at least 2 primes (the last one is the special prime)");
    const u32 n = c->n;
    if (!(g & 1) || g >= 2 * n || g == 1) return fail(FHE_ERR_PARAM, "Galois element %u: must be odd and in (1, 2n = %u)", g, 2 * n);
    if (int rc = check_operands(c, ct2, stride, 2, out2, out_stride, count, scratch, scratch_bytes)) return rc;
    if (!count) return FHE_OK;
    const u32 ginv = (u32)hostmath::powmod(g, n / 2 - 1, 2 * (u64)n);      // the units modulo 2n have exponent n / 2
    return key_switch(c, (const u64 *)ct2, stride, 0, ginv, (u64 *)out2, out_stride, count, (const u64 *)key, (u64 *)scratch, (hipStream_t)s);
}
