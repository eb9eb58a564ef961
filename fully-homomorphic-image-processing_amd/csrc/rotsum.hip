// rotsum.hip -- hoisted special-prime rotations of ONE ciphertext: fhe_rotate_sum_sp (a weighted sum of rotations, one key-switch tail for
// all of them) and fhe_rotate_each_sp (the rotations as separate ciphertexts, one set of forward transforms for all of them) on gfx950.
// include/fhe_hip.h states the operations; DESIGN.md 3.15 has the range proofs, the resource table and the measurements.
//
// With D_i,r = NTT_(q_r)([c_1,i]_(q_r)) (keyswitch_sp.hip's forward kernel, as it is) and pi_g the slot permutation with
// pi_g(NTT(a)) = NTT(sigma_g(a)), the taps (g_j, w_j, K_j) give
//     acc_pp,r = sum_(j: g_j != 1) w'_j sum_(i < L) pi_(g_j)(D_i,r) (*) K_j,i,pp,r  mod q_r      for every r < k
//     u_pp     = one drop of fhe_mod_switch (k -> k - 1) of acc_pp
//     out      = (u_0 + sum_j w'_j sigma_(g_j)(c_0),  u_1 + sum_(j: g_j = 1) w'_j c_1)
// The digit pi_g(D_i,r) is the transform of sigma_g(d_i) taken over the integers, coefficients in (-q_i, q_i), reduced to q_r: NOT the
// digit of fhe_apply_galois_sp, which negates modulo q_i and then reduces ((q_i - x) mod q_r against (-x) mod q_r).  Both are valid
// decompositions of sigma_g(c_1); the ciphertext bits differ, the plaintext and the noise bound do not.
//
// Pseudo-Mersenne bases, four launches whatever the number of taps:
//   k_ksp_fwd_pm<L, C, false>   src_poly = 1 (keyswitch_sp.hip)
//   k_rs_accum_pm               per (c, r, slot): per tap L gathered digits against both key polynomials (rotdiag_core.h's rot_digit_sum,
//                               the one rotdiag.hip and rotbsgs.hip use), folded, times w'_j,r; lazy sum over taps
//   k_ksp_inv_sp_pm             (keyswitch_sp.hip)
//   k_rs_final_pm               workgroup (c, pp, r < L): inverse transform, the drop, then c_0,r through LDS once and one gather per tap
//                               (pp = 0) or w' c_1,r at the words it then writes (pp = 1): u never exists in memory
// fhe_rotate_each_sp: the accumulation kernel writes acc[j][c] without weights and k_ksp_inv_down_add_pm<GAL = true> runs per tap.
// General path (FP64-transform bases, 61-bit primes, FHE_NTT_NOPM=1): element-wise kernels around fhe_qbase_ntt; sum_j w'_j sigma(c_0) and
// w' c_1 are staged in scratch BEFORE anything is written (a block's gathered reads cross other blocks' writes when the call runs in
// place).  Every quantity is the canonical residue of the same integer on both paths: the same bits.
// The call check is rotsum_host.h's, and the slot exponents and the permutation / key tables of the plan come from rotdiag_core.h's two
// plan helpers: both are shared with rotdiag.hip and rotbsgs.hip.
#include "rotdiag_core.h"
#include "rotsum_host.h"

#include <cstring>
#include <memory>

#include "host_math.h"

struct fhe_rotsum_plan {
    const fhe_ctx *ctx = nullptr;
    u32 taps = 0, rotations = 0;    // rotations: taps with g != 1
    int id = -1;                    // the tap with g = 1, or -1
    std::vector<u32> elts, ginv;
    void *d_block = nullptr;        // one allocation: perm [taps][n] u32, ginv [taps] u32, w [taps][k] u64, w1 [taps][k] u64 (ones), keys [taps]
    u32 *d_perm = nullptr, *d_ginv = nullptr;
    u64 *d_w = nullptr, *d_w1 = nullptr;
    const u64 **d_keys = nullptr;
    ~fhe_rotsum_plan() {
        if (d_block) (void)hipFree(d_block);
    }
};

namespace {

struct RsTaps {
    const u32 *perm;            // [taps][n]: slot s of pi_(g_j) reads slot perm[j][s]
    const u32 *ginv;            // [taps]: g_j^-1 mod 2n
    const u64 *w;               // [taps][k]: w'_j mod q_r, canonical
    const u64 *const *keys;     // [taps]: [L][2][k][n] NTT form, null for g_j = 1
    u32 taps;
    int id;
};

// Lazy sums over taps fold every RS_FOLD_TAPS terms.  A term is a mulvv_pm result, below RQ / 16 q; a folded sum is below PM_FOLDED / 16 q;
// 2^64 >= 4 LIM / 16 q (LIM = 2^62 / q rounded down to a power of two).  Class B with 64 taps needs the fold: 64 * 1.5 q = 96 q against
// 2^64 / q >= 64 on a 58-bit prime; class A (64 * 6 q = 384 q against 512) would just fit without it.
// RQ is the figure the host checks mulvv_pm's result against, and it is what this proof rests on.  The products themselves stay far below it:
// for a second operand below 2^43 (every weight is below t / 2) the two folds inside mulvv_pm leave tau + q with tau < delta = 2^b - q, so
// a term is at most 2^b - 1 and 64 unfolded terms at most 2^64 - 64: with real products the unfolded sum would not wrap on a 58-bit prime
// either (tests/test_rotsum_cpu.py reaches 0.999999 * 2^64 with every term crafted above q, and shows the wrap with the terms AT RQ).  The
// fold stays because the kernel's ranges are proved from the checked bounds, not from that finer argument.
// The conditions themselves are rot_bounds_ok (rotdiag_core.h), shared with rotdiag.hip and rotbsgs.hip; this file's own is the last one.
constexpr int RS_FOLD_TAPS = ROT_FOLD_TERMS;
static_assert(PM_FOLDED + rotsum::MAX_TAPS * PmB::RQ > 4 * PmB::LIM, "class B: the fold every RS_FOLD_TAPS taps is what keeps 64 taps inside 64 bits");

// ---- general path -------------------------------------------------------------------------------------------------------------------
// s0[c][r] = sum_(j0 <= j < j1) w'_j sigma_(g_j)(c_0,r) (weights 1 when !weighted); s1[c][r] = w'_id c_1,r (zero without an identity tap in range)
__global__ __launch_bounds__(256) void k_rs_stage(const u64 *__restrict__ ct, u64 stride, u64 *__restrict__ s0, u64 *__restrict__ s1, RsTaps P,
                                                  const Modulus *__restrict__ mod, u32 k, u32 n, u64 count, u32 j0, u32 j1) {
    const u32 Lq = k - 1;
    for (u64 u = blockIdx.y; u < count * Lq; u += gridDim.y) {
        const u32 r = (u32)(u % Lq);
        const u64 c = u / Lq;
        const Modulus m = mod[r];
        const u64 *c0 = ct + c * stride + (u64)r * n, *c1 = c0 + (u64)Lq * n;
        const bool id = s1 && P.id >= (int)j0 && P.id < (int)j1;
        for (u32 x = blockIdx.x * blockDim.x + threadIdx.x; x < n; x += gridDim.x * blockDim.x) {
            u64 a = 0;
            for (u32 j = j0; j < j1; j++) a = addmod(a, mul_barrett(gal_load(c0, x, P.ginv[j], n, m.q), P.w[j * k + r], m), m.q);
            s0[u * n + x] = a;
            if (s1) s1[u * n + x] = id ? mul_barrett(c1[x], P.w[(u32)P.id * k + r], m) : 0;
        }
    }
}
// acc[c][pp][r][s] = sum_(j0 <= j < j1, g_j != 1) w'_j sum_i dig[c][i][r][perm_j[s]] * key_j[i][pp][r][s], canonical Barrett products
__global__ __launch_bounds__(256) void k_rs_accum(const u64 *__restrict__ dig, RsTaps P, u64 *__restrict__ acc, const Modulus *__restrict__ mod, u32 k, u32 n,
                                                  u64 count, u32 j0, u32 j1) {
    const u32 Lq = k - 1;
    const u32 kn = k * n;
    for (u64 u = blockIdx.y; u < count * k; u += gridDim.y) {
        const u32 r = (u32)(u % k);
        const u64 c = u / k;
        const Modulus m = mod[r];
        const u64 *dr = dig + c * Lq * kn + (u64)r * n;
        for (u32 s = blockIdx.x * blockDim.x + threadIdx.x; s < n; s += gridDim.x * blockDim.x) {
            u64 s0 = 0, s1 = 0;
            for (u32 j = j0; j < j1; j++) {
                const u64 *key = P.keys[j];
                if (!key) continue;
                u64 a0 = 0, a1 = 0;
                rot_digit_sum<ArBarrett>(dr + P.perm[(u64)j * n + s], key + (u64)r * n + s, Lq, kn, m, a0, a1);
                const u64 w = P.w[j * k + r];
                s0 = addmod(s0, mul_barrett(a0, w, m), m.q);
                s1 = addmod(s1, mul_barrett(a1, w, m), m.q);
            }
            acc[((c * 2 + 0) * k + r) * n + s] = s0;
            acc[((c * 2 + 1) * k + r) * n + s] = s1;
        }
    }
}
// acc in coefficient form: the drop of the special prime and the addition of the staged terms (s1 null: nothing is added to u_1)
__global__ __launch_bounds__(256) void k_rs_down_add(u64 *__restrict__ out, u64 out_stride, const u64 *__restrict__ acc, const u64 *__restrict__ s0,
                                                     const u64 *__restrict__ s1, KspTab T, u32 k, u32 n, u64 count) {
    const u32 Lq = k - 1;
    for (u64 u = blockIdx.y; u < count * 2 * Lq; u += gridDim.y) {
        const u32 r = (u32)(u % Lq), pp = (u32)((u / Lq) & 1);
        const u64 c = u / (2 * Lq);
        const u64 *a = acc + ((c * 2 + pp) * k + r) * n, *ap = acc + ((c * 2 + pp) * k + Lq) * n;
        const u64 *src = pp ? s1 : s0;
        if (src) src += (c * Lq + r) * n;
        u64 *dst = out + c * out_stride + ((u64)pp * Lq + r) * n;
        for (u32 j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
            const u64 v = ksp_drop(a[j], ap[j], T, r);
            dst[j] = src ? addmod(v, src[j], T.q[r]) : v;
        }
    }
}

// ---- pseudo-Mersenne path -------------------------------------------------------------------------------------------------------------
// (2) per (c, r, slot).  Per tap: L gathered digits (canonical; gathered 8-byte reads of rows that stay in L2 across the taps, the choice
// DESIGN.md 3.10 measured for the Galois digits) against both key polynomials: L <= 7 mulvv_pm terms below RQ each in a 64-bit sum, as
// k_ksp_accum_pm forms them; one fold (below PM_FOLDED / 16 q < 2^(b+1): a valid first operand of mulvv_pm); the product with the canonical
// w'_j,r is below RQ again.  The sum over taps holds a folded value and at most RS_FOLD_TAPS such products: rs_bounds_ok.
// EACH: acc[jj][c][pp][r] = the folded digit sum of rotation jj alone, no weight.
template <typename C, bool EACH>
__global__ __launch_bounds__(256) void k_rs_accum_pm(const u64 *__restrict__ dig, RsTaps P, u64 *__restrict__ acc, RnsBase base, u32 n, u64 count) {
    const u32 k = base.count, Lq = k - 1;
    const u32 kn = k * n;
    for (u64 u = blockIdx.y; u < count * k; u += gridDim.y) {
        const u32 r = (u32)(u % k);
        const u64 c = u / k;
        const PmMod m = base.pm[r];
        const u64 *dr = dig + c * Lq * kn + (u64)r * n;
        for (u32 s = blockIdx.x * blockDim.x + threadIdx.x; s < n; s += gridDim.x * blockDim.x) {
            u64 s0 = 0, s1 = 0;
            u32 since = 0;
            u64 jj = 0;
            for (u32 j = 0; j < P.taps; j++) {
                const u64 *key = P.keys[j];
                if (!key) continue;                                    // uniform: the tap with g = 1
                u64 a0 = 0, a1 = 0;
                rot_digit_sum<ArPm<C>>(dr + P.perm[(u64)j * n + s], key + (u64)r * n + s, Lq, kn, m, a0, a1);
                a0 = fold_pm(a0, m);
                a1 = fold_pm(a1, m);
                if constexpr (EACH) {
                    acc[(((jj * count + c) * 2 + 0) * k + r) * n + s] = a0;
                    acc[(((jj * count + c) * 2 + 1) * k + r) * n + s] = a1;
                    jj++;
                } else {
                    const u64 w = P.w[j * k + r];
                    s0 += mulvv_pm(a0, w, m);
                    s1 += mulvv_pm(a1, w, m);
                    if (++since == RS_FOLD_TAPS) {
                        s0 = fold_pm(s0, m);
                        s1 = fold_pm(s1, m);
                        since = 0;
                    }
                }
            }
            if constexpr (!EACH) {
                acc[((c * 2 + 0) * k + r) * n + s] = fold_pm(s0, m);
                acc[((c * 2 + 1) * k + r) * n + s] = fold_pm(s1, m);
            }
        }
    }
}
// (4) workgroup (c, pp, r < L): k_ksp_inv_down_add_pm's transform and drop.  pp = 0: c_0,r goes through LDS once, AFTER the transform; per
// tap one gather with sigma's negation modulo q_r and a mulvv_pm with w'_j,r (canonical operands: below RQ), the sum over taps under
// rs_bounds_ok, canon_pm, one addmod.  Every global read of c_0,r has landed before the barrier in front of the store, and no other
// workgroup reads or writes that polynomial: out2 may be ct.  pp = 1: the tap with g = 1 adds w' c_1,r, read at the words the thread writes.
template <int L, typename C>
__global__ __launch_bounds__(NttShape<L>::TP, 4) void k_rs_final_pm(const u64 *ct, u64 stride, u64 *out, u64 out_stride, const u64 *__restrict__ acc,
                                                                     const u64 *__restrict__ sp, RnsBase base, KspTab T, RsTaps P) {
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
    if (pp == 0) {                                 // uniform per workgroup
        const u64 *c0 = ct + c * stride + (u64)r * N;
        __syncthreads();                           // the transform's last transpose has read the array
#pragma unroll
        for (int e = 0; e < 16; e++) lds[e * TP + tid] = c0[e * TP + tid];
        __syncthreads();                           // every global read of c0_r has landed: the store below may write it (in place)
#pragma unroll
        for (int e = 0; e < 16; e++) y[e] = 0;
        u32 since = 0;
        for (u32 j = 0; j < P.taps; j++) {
            const u32 ginv = P.ginv[j];
            const u64 w = P.w[j * k + r];
#pragma unroll
            for (int e = 0; e < 16; e++) {
                bool neg;
                const u64 v = lds[gal_src((u32)(e * TP + tid), ginv, N, neg)];
                y[e] += mulvv_pm(neg ? negmod(v, m.q) : v, w, m);
            }
            if (++since == RS_FOLD_TAPS) {
#pragma unroll
                for (int e = 0; e < 16; e++) y[e] = fold_pm(y[e], m);
                since = 0;
            }
        }
#pragma unroll
        for (int e = 0; e < 16; e++) x[0][e] = addmod(x[0][e], canon_pm(y[e], m), m.q);
    } else if (P.id >= 0) {
        const u64 w = P.w[(u32)P.id * k + r];
        load_coeff<L>(y, ct + c * stride + ((u64)Lq + r) * N, tid);
#pragma unroll
        for (int e = 0; e < 16; e++) x[0][e] = addmod(x[0][e], canon_pm(mulvv_pm(y[e], w, m), m), m.q);
    }
    store_coeff<L>(x[0], out + c * out_stride + ((u64)pp * Lq + r) * N, tid);
}

size_t scratch_words(const fhe_rotsum_plan *p, u64 count, bool each) {
    const u64 k = p->ctx->k, Lq = k - 1, n = p->ctx->n;
    if (!each) return (size_t)(count * (Lq * k + 2 * k + 2 * Lq) * n);           // dig, acc, the larger of sp [2][n] and the staged (s0, s1) [2][L][n]
    const u64 R = p->rotations ? p->rotations : 1;
    return (size_t)(count * (Lq * k + R * 2 * k + (2 * R > Lq ? 2 * R : Lq)) * n);   // dig, acc [R], the larger of sp [R][2][n] and the staged s0 [L][n]
}

template <bool EACH> void accum_pm(const fhe_ctx *c, const u64 *dig, const RsTaps &P, u64 *acc, u64 count, hipStream_t st) {
    const RnsBase base = c->qb.dev();
    if (c->qb.pm_class == 1) k_rs_accum_pm<PmA, EACH><<<ksp_grid2(c->n, count * c->k), 256, 0, st>>>(dig, P, acc, base, c->n, count);
    else k_rs_accum_pm<PmB, EACH><<<ksp_grid2(c->n, count * c->k), 256, 0, st>>>(dig, P, acc, base, c->n, count);
}

int rotate(const fhe_rotsum_plan *p, const u64 *ct, u64 stride, u64 *out, u64 out_stride, u64 tap_stride, u64 count, u64 *scratch, hipStream_t st, bool each) {
    const fhe_ctx *c = p->ctx;
    const u32 k = c->k, Lq = k - 1, n = c->n;
    const u64 R = p->rotations;
    u64 *dig = scratch, *acc = dig + count * Lq * k * n;
    const KspTab T = ksp_tab(c);
    RsTaps P{p->d_perm, p->d_ginv, each ? p->d_w1 : p->d_w, p->d_keys, p->taps, p->id};
    int rc;
    if (fhe_ksp_pm_ok(c, count)) {
        const RnsBase base = c->qb.dev();
        const bool A = c->qb.pm_class == 1;
        if (R && (rc = fhe_ksp_forward(c, ct, stride, 1, dig, count, st))) return rc;
        if (each) {
            u64 *sp = acc + R * count * 2 * k * n;
            if (R) {
                accum_pm<true>(c, dig, P, acc, count, st);
                KERNEL_CHECK();
                if ((rc = fhe_ksp_inv_sp(c, acc, sp, R * count * 2, st))) return rc;
            }
            u64 jj = 0;
            for (u32 j = 0; j < p->taps; j++) {
                u64 *o = out + j * tap_stride;
                if (p->elts[j] == 1) {
                    HIP_TRY(hipMemcpy2DAsync(o, out_stride * 8, ct, stride * 8, (size_t)2 * Lq * n * 8, count, hipMemcpyDeviceToDevice, st));
                    continue;
                }
                if ((rc = fhe_ksp_inv_down_add_galois(c, ct, stride, o, out_stride, acc + jj * count * 2 * k * n, sp + jj * count * 2 * n, p->ginv[j], count, st))) return rc;
                jj++;
            }
            return FHE_OK;
        }
        u64 *sp = acc + count * 2 * k * n;
        if (R) {
            accum_pm<false>(c, dig, P, acc, count, st);
        } else {
            HIP_TRY(hipMemsetAsync(acc, 0, count * 2 * k * n * 8, st));          // the identity alone: u = the drop of 0 = 0
        }
        KERNEL_CHECK();
        if ((rc = fhe_ksp_inv_sp(c, acc, sp, count * 2, st))) return rc;
        const unsigned g4 = (unsigned)(count * 2 * Lq);
        if (A) { DISPATCH_L(c->logn, (k_rs_final_pm<L, PmA><<<g4, NttShape<L>::TP, 0, st>>>(ct, stride, out, out_stride, acc, sp, base, T, P))); }
        else { DISPATCH_L(c->logn, (k_rs_final_pm<L, PmB><<<g4, NttShape<L>::TP, 0, st>>>(ct, stride, out, out_stride, acc, sp, base, T, P))); }
        KERNEL_CHECK();
        return FHE_OK;
    }
    const Modulus *mod = c->qb.d_mod;
    u64 *s0 = acc + count * 2 * k * n, *s1 = s0 + count * Lq * n;
    if (!each) {
        k_rs_stage<<<ksp_grid2(n, count * Lq), 256, 0, st>>>(ct, stride, s0, s1, P, mod, k, n, count, 0, p->taps);      // before anything is written
        if (R && (rc = fhe_ksp_forward(c, ct, stride, 1, dig, count, st))) return rc;
        if (R) k_rs_accum<<<ksp_grid2(n, count * k), 256, 0, st>>>(dig, P, acc, mod, k, n, count, 0, p->taps);
        else HIP_TRY(hipMemsetAsync(acc, 0, count * 2 * k * n * 8, st));
        KERNEL_CHECK();
        if (R && (rc = fhe_qbase_ntt(true, c, acc, acc, count * 2, st))) return rc;
        k_rs_down_add<<<ksp_grid2(n, count * 2 * Lq), 256, 0, st>>>(out, out_stride, acc, s0, p->id >= 0 ? s1 : nullptr, T, k, n, count);
        KERNEL_CHECK();
        return FHE_OK;
    }
    if (R && (rc = fhe_ksp_forward(c, ct, stride, 1, dig, count, st))) return rc;
    for (u32 j = 0; j < p->taps; j++) {
        u64 *o = out + j * tap_stride;
        if (p->elts[j] == 1) {
            HIP_TRY(hipMemcpy2DAsync(o, out_stride * 8, ct, stride * 8, (size_t)2 * Lq * n * 8, count, hipMemcpyDeviceToDevice, st));
            continue;
        }
        k_rs_stage<<<ksp_grid2(n, count * Lq), 256, 0, st>>>(ct, stride, s0, nullptr, P, mod, k, n, count, j, j + 1);
        k_rs_accum<<<ksp_grid2(n, count * k), 256, 0, st>>>(dig, P, acc, mod, k, n, count, j, j + 1);
        KERNEL_CHECK();
        if ((rc = fhe_qbase_ntt(true, c, acc, acc, count * 2, st))) return rc;
        k_rs_down_add<<<ksp_grid2(n, count * 2 * Lq), 256, 0, st>>>(o, out_stride, acc, s0, nullptr, T, k, n, count);
        KERNEL_CHECK();
    }
    return FHE_OK;
}

// the call check (rotsum_host.h) of both entry points; `each`: fhe_rotate_each_sp
int check_call(const fhe_rotsum_plan *p, const void *ct, u64 stride, const void *out, u64 out_stride, u64 tap_stride, u64 count, const void *scratch,
               size_t scratch_bytes, bool each) {
    const fhe_ctx *c = p->ctx;
    const std::string why = rotsum::check_call(c->k, c->n, ct, stride, out, out_stride, count, count * p->taps * 2 * c->k, scratch_words(p, count, each) * sizeof(u64),
                                               scratch, scratch_bytes, each ? p->taps : 0, tap_stride);
    return why.empty() ? FHE_OK : fail(FHE_ERR_PARAM, "%s", why.c_str());
}

}  // namespace

extern "C" int fhe_rotsum_plan_create(const fhe_ctx *c, uint32_t taps, const uint32_t *elts, const uint64_t *weights, const uint64_t *const *d_keys,
                                      fhe_rotsum_plan **out) {
    if (!c || !out || !elts || !d_keys) return fail(FHE_ERR_PARAM, "null argument");
    const u32 n = c->n, k = c->k;
    std::vector<uint64_t> w(taps && taps <= rotsum::MAX_TAPS ? taps : 0, 1);
    if (weights) std::copy(weights, weights + w.size(), w.begin());
    const std::string why = rotsum::check_taps(n, c->t, k, taps, elts, w.data(), (const void *const *)d_keys);
    if (!why.empty()) return fail(FHE_ERR_PARAM, "%s", why.c_str());
    // the context's own forward transform of X, in a buffer of its own
    u64 *d_x = nullptr;
    HIP_TRY(hipMalloc(&d_x, (size_t)k * n * 8));
    std::vector<u32> f;
    int rc = fhe_rot_slot_exponents(c, d_x, 0, "X", f);
    (void)hipFree(d_x);
    if (rc) return rc;
    std::unique_ptr<fhe_rotsum_plan> p(new fhe_rotsum_plan);
    p->ctx = c;
    p->taps = taps;
    p->elts.assign(elts, elts + taps);
    std::vector<u32> perm((size_t)taps * n);
    std::vector<u64> wr((size_t)taps * k), keys(taps);
    for (u32 j = 0; j < taps; j++) {
        const u32 g = elts[j];
        p->ginv.push_back((u32)hostmath::powmod(g, n / 2 - 1, 2 * (u64)n));      // the units modulo 2n have exponent n / 2
        if (g == 1) p->id = (int)j;
        else p->rotations++;
        for (u32 r = 0; r < k; r++) wr[(size_t)j * k + r] = rotsum::weight_residue(w[j], c->t, c->qb.primes[r]);
    }
    if ((rc = fhe_rot_perm_keys(f, taps, elts, d_keys, perm.data(), keys.data()))) return rc;
    const size_t b_perm = perm.size() * 4, b_ginv = ((size_t)taps * 4 + 7) & ~(size_t)7, b_w = wr.size() * 8, b_keys = (size_t)taps * 8;
    std::vector<unsigned char> blob(b_perm + b_ginv + 2 * b_w + b_keys);
    std::vector<u64> ones(wr.size(), 1);
    memcpy(blob.data(), perm.data(), b_perm);
    memcpy(blob.data() + b_perm, p->ginv.data(), (size_t)taps * 4);
    memcpy(blob.data() + b_perm + b_ginv, wr.data(), b_w);
    memcpy(blob.data() + b_perm + b_ginv + b_w, ones.data(), b_w);
    memcpy(blob.data() + b_perm + b_ginv + 2 * b_w, keys.data(), b_keys);
    if (hipMalloc(&p->d_block, blob.size()) != hipSuccess) {
        p->d_block = nullptr;
        return fail(FHE_ERR_NOMEM, "device allocation of %zu bytes for the rotate-sum plan", blob.size());
    }
    if (hipMemcpy(p->d_block, blob.data(), blob.size(), hipMemcpyHostToDevice) != hipSuccess) return fail(FHE_ERR_HIP, "upload of the rotate-sum plan");
    unsigned char *d = (unsigned char *)p->d_block;
    p->d_perm = (u32 *)d;
    p->d_ginv = (u32 *)(d + b_perm);
    p->d_w = (u64 *)(d + b_perm + b_ginv);
    p->d_w1 = (u64 *)(d + b_perm + b_ginv + b_w);
    p->d_keys = (const u64 **)(d + b_perm + b_ginv + 2 * b_w);
    *out = p.release();
    return FHE_OK;
}

extern "C" int fhe_rotsum_plan_destroy(fhe_rotsum_plan *p) {
    delete p;
    return FHE_OK;
}

extern "C" size_t fhe_rotsum_scratch_bytes(const fhe_rotsum_plan *p, uint64_t count, int each) {
    if (!p) return 0;
    return scratch_words(p, count, each != 0) * sizeof(u64);
}

extern "C" int fhe_rotate_sum_sp(const fhe_rotsum_plan *p, const uint64_t *ct2, uint64_t stride, uint64_t *out2, uint64_t out_stride, uint64_t count,
                                 void *scratch, size_t scratch_bytes, fhe_stream s) {
    if (!p || !ct2 || !out2) return fail(FHE_ERR_PARAM, "null argument");
    if (int rc = check_call(p, ct2, stride, out2, out_stride, 0, count, scratch, scratch_bytes, false)) return rc;
    if (!count) return FHE_OK;
    return rotate(p, (const u64 *)ct2, stride, (u64 *)out2, out_stride, 0, count, (u64 *)scratch, (hipStream_t)s, false);
}

extern "C" int fhe_rotate_each_sp(const fhe_rotsum_plan *p, const uint64_t *ct2, uint64_t stride, uint64_t *out, uint64_t out_stride, uint64_t tap_stride,
                                  uint64_t count, void *scratch, size_t scratch_bytes, fhe_stream s) {
    if (!p || !ct2 || !out) return fail(FHE_ERR_PARAM, "null argument");
    if (int rc = check_call(p, ct2, stride, out, out_stride, tap_stride, count, scratch, scratch_bytes, true)) return rc;
    if (!count) return FHE_OK;
    return rotate(p, (const u64 *)ct2, stride, (u64 *)out, out_stride, tap_stride, count, (u64 *)scratch, (hipStream_t)s, true);
}
