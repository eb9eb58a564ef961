// rotbsgs.hip -- a baby-step / giant-step linear map on the slots of ONE ciphertext: fhe_rotate_bsgs_sp on gfx950,
//     out = sum_i rot_(h_i)( sum_j p_(i,j) * rot_(g_j)(ct) )
// with G1 baby elements g_j, G2 giant elements h_i and a plaintext POLYNOMIAL per present pair: G1 + G2 keys where the diagonal method of
// rotdiag.hip needs G1 G2.  include/fhe_hip.h states the operation; DESIGN.md 3.17 has the range proof and the resource table.
//
// With D_l,r, C0_r, pi_g and P_(i,j),r as in rotdiag.hip:
//     A(i)_pp,r = sum_(j present) P_(i,j),r (*) T_j,pp,r                                          rotdiag.hip's accumulator, one per giant step
//     T_j,pp,r  = sum_l pi_(g_j)(D_l,r) (*) K_(g_j),l,pp,r + [pp = 0, r < L] [p] pi_(g_j)(C0_r) + [pp = 1, g_j = 1, r < L] [p] D_r,r
//     v(i)      = one drop of A(i)_1 (h_i != 1),   E(i)_l,r = NTT_(q_r)([v(i)_l]_(q_r))            the hoisted digits of the giant step
//     B_pp,r    = sum_(i: h_i != 1) [ sum_l pi_(h_i)(E(i)_l,r) (*) K_(h_i),l,pp,r + [pp = 0] pi_(h_i)(A(i)_0,r) ] + sum_(i: h_i = 1) A(i)_pp,r
//     out_pp    = one drop of B_pp
// A(i)_0 keeps its factor p through the giant step (all k primes, never rounded on its own): c_0 is rounded once, at the end.
//
// Pseudo-Mersenne bases, eight launches whatever G1 and G2 are:
//   k_rd_fwd_pm        (rotdiag_core.h) the digit transforms of c_1 and the transform of c_0
//   k_bs_baby_pm       per (c, group of BS_GG giant steps, r, slot): per baby step the gathered key sums T_j,0 and T_j,1 ONCE, fanned out to
//                      the group's accumulators through the coalesced P_(i,j),r[slot] reads
//   k_ksp_inv_sp_pm    (keyswitch_sp.hip) the special prime's row of every A(i)_1
//   k_rd_inv_down_pm   (rotdiag_core.h) inverse transform of A(i)_1 and the drop: v(i)
//   k_ksp_fwd_pm       (keyswitch_sp.hip) the L k digit transforms of every v(i)
//   k_bs_giant_pm      per (c, r, slot): the gathered E(i) against the giant keys, the gathered A(i)_0 word, the identity giant's own words
//   k_ksp_inv_sp_pm, k_rd_inv_down_pm  the last drop
// General path (FP64-transform bases, 61-bit primes, FHE_NTT_NOPM=1): element-wise Barrett kernels around fhe_qbase_ntt / fhe_ksp_forward.
// Every quantity is the canonical residue of the same integer on both paths: the same bits.
#include "rotdiag_core.h"
#include "rotbsgs_host.h"

struct fhe_rotbsgs_plan {
    const fhe_ctx *ctx = nullptr;
    u32 G1 = 0, G2 = 0, pairs = 0;
    std::vector<u32> baby, giant;
    void *d_block = nullptr;        // one allocation: P [pairs][k][n] u64, the tables below
    u64 *d_P = nullptr;
    u32 *d_permB = nullptr, *d_permG = nullptr;
    const u64 **d_keysB = nullptr, **d_keysG = nullptr;
    uint2 *d_pgrp = nullptr;
};

namespace {

constexpr int BS_GG = (int)rotbsgs::GIANT_GROUP;

struct BsDev {
    const u32 *permB, *permG;       // [G1][n], [G2][n]: slot s of pi_g reads slot perm[s] (the identity for g = 1)
    const u64 *P;                   // [pairs][k][n]: NTT_(q_r)(p'_(i,j)), canonical, the context's slot order
    const u64 *const *keysB;        // [G1]: [L][2][k][n] NTT form, null for g_j = 1
    const u64 *const *keysG;        // [G2]: the same, null for h_i = 1
    const uint2 *pgrp;              // [groups of BS_GG giant steps][G1]: (x = the row in P of the group's first present pair with baby step j, y = bit g set:
                                    // pair (group BS_GG + g, j) is present); the present pairs of one (group, j) are consecutive rows of P
    u64 pr[FHE_MAX_K];              // the special prime modulo q_r, r < L
    u32 G1, G2;
};

// The lazy sums, in sixteenths of q (4 LIM = 2^64 / q rounded down to a power of two):
//   T_j:   rotdiag.hip's: at most L + 1 <= FHE_MAX_K mulvv_pm results below RQ each, one fold (below PM_FOLDED: a valid first operand)
//   A(i):  one mulvv_pm(T_j, P_(i,j)) below RQ per PRESENT baby step; the fold counter counts every baby step, present or not, so a
//          register holds a folded value and at most BS_FOLD_BABY products
//   B:     per giant step L products below RQ and the folded word of A(i)_0 (below PM_FOLDED <= RQ): L + 1 <= FHE_MAX_K terms, one fold;
//          the sum over giant steps holds a folded value and at most BS_FOLD_GIANT folded terms (the identity giant adds one folded word)
constexpr int BS_FOLD_BABY = 32, BS_FOLD_GIANT = 32;
template <typename C> constexpr bool bs_bounds_ok() {
    return PM_FOLDED + BS_FOLD_BABY * C::RQ <= 4 * C::LIM        // A(i): a folded sum and BS_FOLD_BABY more products fit 64 bits
           && FHE_MAX_K * C::RQ <= 4 * C::LIM                    // T_j and the per-giant sum: L + 1 <= 8 terms
           && PM_FOLDED <= C::RQ                                 // the folded word of A(i)_0 counts as one of those terms
           && PM_FOLDED * (1 + BS_FOLD_GIANT) <= 4 * C::LIM      // B: a folded sum and BS_FOLD_GIANT folded terms
           && PM_FOLDED <= 32;                                   // a folded value is a valid first operand of mulvv_pm (below 2^(b+1))
}
static_assert(bs_bounds_ok<PmA>() && bs_bounds_ok<PmB>(), "lazy baby-step / giant-step sums");
static_assert(rotbsgs::MAX_STEPS <= 64 && BS_GG >= 1, "plan limits");

// ---- general path -------------------------------------------------------------------------------------------------------------------
// c0h [count][k][n]: c_0,r for r < L, zeros at the special prime, for the base's own forward transforms
__global__ __launch_bounds__(256) void k_bs_stage_c0(const u64 *__restrict__ ct, u64 stride, u64 *__restrict__ c0h, u32 k, u32 n, u64 count) {
    for (u64 u = blockIdx.y; u < count * k; u += gridDim.y) {
        const u32 r = (u32)(u % k);
        const u64 c = u / k;
        const u64 *src = ct + c * stride + (u64)r * n;
        for (u32 x = blockIdx.x * blockDim.x + threadIdx.x; x < n; x += gridDim.x * blockDim.x) c0h[u * n + x] = r < k - 1 ? src[x] : 0;
    }
}
// A0 / A1 [c][i][r][s] = sum_(j present) P_(i,j),r[s] T_j,pp,r[s], canonical Barrett products; per (c, i, r) row
__global__ __launch_bounds__(256) void k_bs_baby(const u64 *__restrict__ dig, const u64 *__restrict__ c0h, BsDev P, u64 *__restrict__ A0, u64 *__restrict__ A1,
                                                 const Modulus *__restrict__ mod, u32 k, u32 n, u64 count) {
    const u32 Lq = k - 1;
    for (u64 u = blockIdx.y; u < count * P.G2 * k; u += gridDim.y) {
        const u32 r = (u32)(u % k), i = (u32)((u / k) % P.G2);
        const u64 c = u / ((u64)k * P.G2);
        const Modulus m = mod[r];
        const bool low = r < Lq;
        const u64 pr = P.pr[r];
        for (u32 s = blockIdx.x * blockDim.x + threadIdx.x; s < n; s += gridDim.x * blockDim.x) {
            u64 s0 = 0, s1 = 0;
            for (u32 j = 0; j < P.G1; j++) {
                const uint2 pg = P.pgrp[(u64)(i / BS_GG) * P.G1 + j];
                if (!(pg.y >> (i % BS_GG) & 1)) continue;              // uniform: an absent pair
                const u32 idx = pg.x + __popc(pg.y & ((1u << (i % BS_GG)) - 1));
                const u64 *key = P.keysB[j];
                const u32 src = P.permB[(u64)j * n + s];
                u64 a0 = 0, a1 = 0;
                if (key) {
                    for (u32 l = 0; l < Lq; l++) {
                        const u64 x = dig[((c * Lq + l) * k + r) * n + src];
                        const u64 *e = key + (((u64)l * 2) * k + r) * n + s;
                        a0 = addmod(a0, mul_barrett(x, e[0], m), m.q);
                        a1 = addmod(a1, mul_barrett(x, e[(u64)k * n], m), m.q);
                    }
                }
                if (low) {
                    a0 = addmod(a0, mul_barrett(c0h[(c * k + r) * n + src], pr, m), m.q);
                    if (!key) a1 = mul_barrett(dig[((c * Lq + r) * k + r) * n + src], pr, m);
                }
                const u64 w = P.P[((u64)idx * k + r) * n + s];
                s0 = addmod(s0, mul_barrett(a0, w, m), m.q);
                s1 = addmod(s1, mul_barrett(a1, w, m), m.q);
            }
            A0[u * n + s] = s0;
            A1[u * n + s] = s1;
        }
    }
}
// acc [rows][k][n] in coefficient form -> the drop of the special prime; row = c * 2 + pp goes to out + c * out_stride + (pp L + r) n
__global__ __launch_bounds__(256) void k_bs_down(u64 *__restrict__ out, u64 out_stride, const u64 *__restrict__ acc, KspTab T, u32 k, u32 n, u64 rows) {
    const u32 Lq = k - 1;
    for (u64 u = blockIdx.y; u < rows * Lq; u += gridDim.y) {
        const u32 r = (u32)(u % Lq);
        const u64 row = u / Lq;
        const u64 *a = acc + (row * k + r) * n, *ap = acc + (row * k + Lq) * n;
        u64 *dst = out + (row >> 1) * out_stride + ((row & 1) * Lq + r) * n;
        for (u32 j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) dst[j] = ksp_drop(a[j], ap[j], T, r);
    }
}
// B [c][pp][r][s]: the giant steps.  E [c][i][l][r][n] the digits of v(i), A0 / A1 [c][i][r][n] in NTT form
__global__ __launch_bounds__(256) void k_bs_giant(const u64 *__restrict__ E, const u64 *__restrict__ A0, const u64 *__restrict__ A1, BsDev P, u64 *__restrict__ B,
                                                  const Modulus *__restrict__ mod, u32 k, u32 n, u64 count) {
    const u32 Lq = k - 1;
    for (u64 u = blockIdx.y; u < count * k; u += gridDim.y) {
        const u32 r = (u32)(u % k);
        const u64 c = u / k;
        const Modulus m = mod[r];
        for (u32 s = blockIdx.x * blockDim.x + threadIdx.x; s < n; s += gridDim.x * blockDim.x) {
            u64 s0 = 0, s1 = 0;
            for (u32 i = 0; i < P.G2; i++) {
                const u64 *key = P.keysG[i];
                const u64 ci = c * P.G2 + i;
                if (!key) {                                            // uniform: the identity giant step
                    s0 = addmod(s0, A0[(ci * k + r) * n + s], m.q);
                    s1 = addmod(s1, A1[(ci * k + r) * n + s], m.q);
                    continue;
                }
                const u32 src = P.permG[(u64)i * n + s];
                s0 = addmod(s0, A0[(ci * k + r) * n + src], m.q);
                for (u32 l = 0; l < Lq; l++) {
                    const u64 x = E[((ci * Lq + l) * k + r) * n + src];
                    const u64 *e = key + (((u64)l * 2) * k + r) * n + s;
                    s0 = addmod(s0, mul_barrett(x, e[0], m), m.q);
                    s1 = addmod(s1, mul_barrett(x, e[(u64)k * n], m), m.q);
                }
            }
            B[((c * 2 + 0) * k + r) * n + s] = s0;
            B[((c * 2 + 1) * k + r) * n + s] = s1;
        }
    }
}

// ---- pseudo-Mersenne path -------------------------------------------------------------------------------------------------------------
// per (c, group, r, slot): the group's BS_GG giant accumulators (2 BS_GG 64-bit registers) live through the loop over the baby steps.
// T_j is k_rd_accum_pm's a0 / a1 (the gather-bound part), computed once per baby step and group; the fan-out reads P_(i,j),r[s]
// coalesced.  A giant step past G2 has no bit in the group's mask, so the unrolled fan-out needs no bound on i.
template <typename C>
__global__ __launch_bounds__(256) void k_bs_baby_pm(const u64 *__restrict__ dig, const u64 *__restrict__ c0h, BsDev P, u64 *__restrict__ A0, u64 *__restrict__ A1,
                                                    RnsBase base, u32 n, u64 count) {
    const u32 k = base.count, Lq = k - 1, NG = (P.G2 + BS_GG - 1) / BS_GG;
    const u64 kn = (u64)k * n;
    for (u64 u = blockIdx.y; u < count * NG * k; u += gridDim.y) {
        const u32 r = (u32)(u % k), i0 = (u32)((u / k) % NG) * BS_GG;
        const u64 c = u / ((u64)k * NG);
        const PmMod m = base.pm[r];
        const bool low = r < Lq;
        const u64 pr = P.pr[r];
        for (u32 s = blockIdx.x * blockDim.x + threadIdx.x; s < n; s += gridDim.x * blockDim.x) {
            const u64 *Ps = P.P + (u64)r * n + s;                      // this thread's word of row 0; row idx is idx k n words further
            u64 s0[BS_GG], s1[BS_GG];
#pragma unroll
            for (int g = 0; g < BS_GG; g++) s0[g] = s1[g] = 0;
            u32 since = 0;
            for (u32 j = 0; j < P.G1; j++) {
                const u64 *key = P.keysB[j];
                const u32 src = P.permB[(u64)j * n + s];
                u64 a0 = 0, a1 = 0;
                if (key) {                                             // uniform: every baby step but the one with g = 1
                    for (u32 l = 0; l < Lq; l++) {
                        const u64 x = dig[((c * Lq + l) * k + r) * n + src];
                        const u64 *e = key + (((u64)l * 2) * k + r) * n + s;
                        a0 += mulvv_pm(x, e[0], m);
                        a1 += mulvv_pm(x, e[(u64)k * n], m);
                    }
                }
                if (low) {                                             // uniform per row
                    a0 += mulvv_pm(c0h[(c * k + r) * n + src], pr, m);
                    if (!key) a1 = mulvv_pm(dig[((c * Lq + r) * k + r) * n + src], pr, m);
                }
                a0 = fold_pm(a0, m);
                a1 = fold_pm(a1, m);
                const uint2 pg = P.pgrp[(u64)(i0 / BS_GG) * P.G1 + j];    // uniform
#pragma unroll
                for (int g = 0; g < BS_GG; g++) {
                    if (pg.y >> g & 1) {
                        const u64 w = Ps[(u64)(pg.x + __popc(pg.y & ((1u << g) - 1))) * kn];
                        s0[g] += mulvv_pm(a0, w, m);
                        s1[g] += mulvv_pm(a1, w, m);
                    }
                }
                if (++since == BS_FOLD_BABY) {
#pragma unroll
                    for (int g = 0; g < BS_GG; g++) {
                        s0[g] = fold_pm(s0[g], m);
                        s1[g] = fold_pm(s1[g], m);
                    }
                    since = 0;
                }
            }
#pragma unroll
            for (int g = 0; g < BS_GG; g++) {
                if (i0 + g < P.G2) {
                    const u64 at = (((c * P.G2 + i0 + g) * k + r) * n) + s;
                    A0[at] = fold_pm(s0[g], m);
                    A1[at] = fold_pm(s1[g], m);
                }
            }
        }
    }
}
// per (c, r, slot): see the bounds above
template <typename C>
__global__ __launch_bounds__(256) void k_bs_giant_pm(const u64 *__restrict__ E, const u64 *__restrict__ A0, const u64 *__restrict__ A1, BsDev P, u64 *__restrict__ B,
                                                     RnsBase base, u32 n, u64 count) {
    const u32 k = base.count, Lq = k - 1;
    for (u64 u = blockIdx.y; u < count * k; u += gridDim.y) {
        const u32 r = (u32)(u % k);
        const u64 c = u / k;
        const PmMod m = base.pm[r];
        for (u32 s = blockIdx.x * blockDim.x + threadIdx.x; s < n; s += gridDim.x * blockDim.x) {
            u64 s0 = 0, s1 = 0;
            u32 since = 0;
            for (u32 i = 0; i < P.G2; i++) {
                const u64 *key = P.keysG[i];
                const u64 ci = c * P.G2 + i;
                if (!key) {                                            // uniform: the identity giant step, folded words
                    s0 += A0[(ci * k + r) * n + s];
                    s1 += A1[(ci * k + r) * n + s];
                } else {
                    const u32 src = P.permG[(u64)i * n + s];
                    u64 a0 = A0[(ci * k + r) * n + src], a1 = 0;
                    for (u32 l = 0; l < Lq; l++) {
                        const u64 x = E[((ci * Lq + l) * k + r) * n + src];
                        const u64 *e = key + (((u64)l * 2) * k + r) * n + s;
                        a0 += mulvv_pm(x, e[0], m);
                        a1 += mulvv_pm(x, e[(u64)k * n], m);
                    }
                    s0 += fold_pm(a0, m);
                    s1 += fold_pm(a1, m);
                }
                if (++since == BS_FOLD_GIANT) {
                    s0 = fold_pm(s0, m);
                    s1 = fold_pm(s1, m);
                    since = 0;
                }
            }
            B[((c * 2 + 0) * k + r) * n + s] = fold_pm(s0, m);
            B[((c * 2 + 1) * k + r) * n + s] = fold_pm(s1, m);
        }
    }
}

struct Scratch {
    u64 *dig, *c0h, *A0, *A1, *spA, *v, *E, *B, *spB;
};
Scratch carve(const fhe_rotbsgs_plan *p, u64 count, u64 *s) {
    const u64 k = p->ctx->k, Lq = k - 1, n = p->ctx->n, G2 = p->G2;
    Scratch x;
    x.dig = s;
    x.c0h = x.dig + count * Lq * k * n;
    x.A0 = x.c0h + count * k * n;
    x.A1 = x.A0 + count * G2 * k * n;
    x.spA = x.A1 + count * G2 * k * n;
    x.v = x.spA + count * G2 * n;
    x.E = x.v + count * G2 * Lq * n;
    x.B = x.E + count * G2 * Lq * k * n;
    x.spB = x.B + count * 2 * k * n;
    return x;
}
size_t scratch_words(const fhe_rotbsgs_plan *p, u64 count) { return (size_t)rotbsgs::scratch_words(count, p->ctx->k, p->ctx->n, p->G2); }

int run(const fhe_rotbsgs_plan *p, const u64 *ct, u64 stride, u64 *out, u64 out_stride, u64 count, u64 *scratch, hipStream_t st) {
    const fhe_ctx *c = p->ctx;
    const u32 k = c->k, Lq = k - 1, n = c->n, G2 = p->G2;
    const u64 rows = count * G2;                   // one inner accumulator pair per ciphertext and giant step
    const Scratch S = carve(p, count, scratch);
    const KspTab T = ksp_tab(c);
    BsDev P{p->d_permB, p->d_permG, p->d_P, p->d_keysB, p->d_keysG, p->d_pgrp, {0}, p->G1, G2};
    for (u32 r = 0; r < Lq; r++) P.pr[r] = T.p % T.q[r];
    int rc;
    if (fhe_ksp_pm_ok(c, rows)) {
        const RnsBase base = c->qb.dev();
        const u64 NG = (G2 + BS_GG - 1) / BS_GG;
        const unsigned g1 = (unsigned)(count * (Lq * k + Lq)), gv = (unsigned)(rows * Lq), g4 = (unsigned)(count * 2 * Lq);
        const dim3 gb = ksp_grid2(n, count * NG * k), gg = ksp_grid2(n, count * k);
        const bool a = c->qb.pm_class == 1;
        if (a) {
            DISPATCH_L(c->logn, (k_rd_fwd_pm<L, PmA><<<g1, NttShape<L>::TP, 0, st>>>(ct, stride, S.dig, S.c0h, base)));
            k_bs_baby_pm<PmA><<<gb, 256, 0, st>>>(S.dig, S.c0h, P, S.A0, S.A1, base, n, count);
        } else {
            DISPATCH_L(c->logn, (k_rd_fwd_pm<L, PmB><<<g1, NttShape<L>::TP, 0, st>>>(ct, stride, S.dig, S.c0h, base)));
            k_bs_baby_pm<PmB><<<gb, 256, 0, st>>>(S.dig, S.c0h, P, S.A0, S.A1, base, n, count);
        }
        KERNEL_CHECK();
        // v(i): A1 [rows][k][n] read as pairs of rows, written as contiguous [rows][L][n] (row = c' * 2 + pp, "stride" 2 L n)
        if ((rc = fhe_ksp_inv_sp(c, S.A1, S.spA, rows, st))) return rc;
        if (a) { DISPATCH_L(c->logn, (k_rd_inv_down_pm<L, PmA><<<gv, NttShape<L>::TP, 0, st>>>(S.v, 2 * (u64)Lq * n, S.A1, S.spA, base, T))); }
        else { DISPATCH_L(c->logn, (k_rd_inv_down_pm<L, PmB><<<gv, NttShape<L>::TP, 0, st>>>(S.v, 2 * (u64)Lq * n, S.A1, S.spA, base, T))); }
        KERNEL_CHECK();
        if ((rc = fhe_ksp_forward(c, S.v, (u64)Lq * n, 0, S.E, rows, st))) return rc;
        if (a) k_bs_giant_pm<PmA><<<gg, 256, 0, st>>>(S.E, S.A0, S.A1, P, S.B, base, n, count);
        else k_bs_giant_pm<PmB><<<gg, 256, 0, st>>>(S.E, S.A0, S.A1, P, S.B, base, n, count);
        KERNEL_CHECK();
        if ((rc = fhe_ksp_inv_sp(c, S.B, S.spB, count * 2, st))) return rc;
        if (a) { DISPATCH_L(c->logn, (k_rd_inv_down_pm<L, PmA><<<g4, NttShape<L>::TP, 0, st>>>(out, out_stride, S.B, S.spB, base, T))); }
        else { DISPATCH_L(c->logn, (k_rd_inv_down_pm<L, PmB><<<g4, NttShape<L>::TP, 0, st>>>(out, out_stride, S.B, S.spB, base, T))); }
        KERNEL_CHECK();
        return FHE_OK;
    }
    k_bs_stage_c0<<<ksp_grid2(n, count * k), 256, 0, st>>>(ct, stride, S.c0h, k, n, count);
    KERNEL_CHECK();
    if ((rc = fhe_qbase_ntt(false, c, S.c0h, S.c0h, count, st))) return rc;
    if ((rc = fhe_ksp_forward(c, ct, stride, 1, S.dig, count, st))) return rc;
    k_bs_baby<<<ksp_grid2(n, rows * k), 256, 0, st>>>(S.dig, S.c0h, P, S.A0, S.A1, c->qb.d_mod, k, n, count);
    KERNEL_CHECK();
    // the identity giant step reads A1 in NTT form, so a COPY is transformed and dropped: the first [rows][k][n] words of E hold it until
    // v is written; the digits of v then overwrite them
    u64 *A1c = S.E;
    if (hipMemcpyAsync(A1c, S.A1, rows * k * n * sizeof(u64), hipMemcpyDeviceToDevice, st) != hipSuccess) return fail(FHE_ERR_HIP, "copy of the inner accumulators");
    if ((rc = fhe_qbase_ntt(true, c, A1c, A1c, rows, st))) return rc;
    k_bs_down<<<ksp_grid2(n, rows * Lq), 256, 0, st>>>(S.v, 2 * (u64)Lq * n, A1c, T, k, n, rows);
    KERNEL_CHECK();
    if ((rc = fhe_ksp_forward(c, S.v, (u64)Lq * n, 0, S.E, rows, st))) return rc;
    k_bs_giant<<<ksp_grid2(n, count * k), 256, 0, st>>>(S.E, S.A0, S.A1, P, S.B, c->qb.d_mod, k, n, count);
    KERNEL_CHECK();
    if ((rc = fhe_qbase_ntt(true, c, S.B, S.B, count * 2, st))) return rc;
    k_bs_down<<<ksp_grid2(n, count * 2 * Lq), 256, 0, st>>>(out, out_stride, S.B, T, k, n, count * 2);
    KERNEL_CHECK();
    return FHE_OK;
}

// in the order include/fhe_hip.h lists them (fhe_rotate_diag_sum_sp's)
int check_call(const fhe_rotbsgs_plan *p, const void *ct, u64 stride, const void *out, u64 out_stride, u64 count, const void *scratch, size_t scratch_bytes) {
    const fhe_ctx *c = p->ctx;
    const u64 Ln = (u64)(c->k - 1) * c->n;
    if (stride < 2 * Ln) return fail(FHE_ERR_PARAM, "ciphertext stride smaller than a size-2 ciphertext of %u primes", c->k - 1);
    if (out_stride < 2 * Ln) return fail(FHE_ERR_PARAM, "output stride smaller than a size-2 ciphertext of %u primes", c->k - 1);
    if (!count) return FHE_OK;
    if (count > 0x7fffffffULL || count * p->G2 * c->k * c->k > 0x7fffffffULL) return fail(FHE_ERR_PARAM, "too many ciphertexts for one call");
    const size_t need = scratch_words(p, count) * sizeof(u64);
    if (!scratch || scratch_bytes < need) return fail(FHE_ERR_PARAM, "scratch too small");
    const u64 in_words = (count - 1) * stride + 2 * Ln, out_words = (count - 1) * out_stride + 2 * Ln;
    if (!(out == ct && out_stride == stride) && overlap(ct, in_words, out, out_words))
        return fail(FHE_ERR_PARAM, "output range overlaps the input range (only out2 == ct2 with out_stride == stride may alias)");
    if (overlap(scratch, need / 8, ct, in_words) || overlap(scratch, need / 8, out, out_words)) return fail(FHE_ERR_PARAM, "scratch overlaps the input or the output");
    return FHE_OK;
}

}  // namespace

extern "C" int fhe_rotbsgs_plan_create(const fhe_ctx *c, uint32_t G1, const uint32_t *baby, uint32_t G2, const uint32_t *giant, const uint64_t *plains,
                                       const uint64_t *const *d_baby_keys, const uint64_t *const *d_giant_keys, fhe_rotbsgs_plan **out) {
    if (!c || !out || !baby || !giant || !plains || !d_baby_keys || !d_giant_keys) return fail(FHE_ERR_PARAM, "null argument");
    const u32 n = c->n, k = c->k;
    const std::string why = rotbsgs::check_plan(n, c->t, k, G1, baby, G2, giant, plains, (const void *const *)d_baby_keys, (const void *const *)d_giant_keys);
    if (!why.empty()) return fail(FHE_ERR_PARAM, "%s", why.c_str());
    std::vector<int32_t> idx;
    std::vector<uint32_t> grp;
    const u32 pairs = rotbsgs::group_rows(n, G1, G2, plains, idx, grp);
    // rows 0 .. pairs - 1: the centred lifts of the present pairs; row `pairs`: the monomial X (rotdiag.hip's way to the slot exponents)
    const size_t row = (size_t)k * n, b_P = (size_t)(pairs + 1) * row * 8;
    const size_t b_permB = (((size_t)G1 * n * 4) + 7) & ~(size_t)7, b_permG = (((size_t)G2 * n * 4) + 7) & ~(size_t)7;
    const size_t b_keysB = (size_t)G1 * 8, b_keysG = (size_t)G2 * 8, b_pgrp = grp.size() * 4;
    std::vector<uint64_t> h((size_t)(pairs + 1) * row, 0);
    const std::vector<uint64_t> primes(c->qb.primes.begin(), c->qb.primes.end());
    for (size_t u = 0; u < (size_t)G1 * G2; u++)
        if (idx[u] >= 0) rotdiag::lift(plains + u * n, n, c->t, primes.data(), k, h.data() + (size_t)idx[u] * row);
    for (u32 r = 0; r < k; r++) h[(size_t)pairs * row + (size_t)r * n + 1] = 1;
    fhe_rotbsgs_plan *p = new fhe_rotbsgs_plan;
    p->ctx = c;
    p->G1 = G1;
    p->G2 = G2;
    p->pairs = pairs;
    p->baby.assign(baby, baby + G1);
    p->giant.assign(giant, giant + G2);
    auto bail = [&](int rc) {
        if (p->d_block) (void)hipFree(p->d_block);
        delete p;
        return rc;
    };
    const size_t bytes = b_P + b_permB + b_permG + b_keysB + b_keysG + b_pgrp;
    if (hipMalloc(&p->d_block, bytes) != hipSuccess) {
        p->d_block = nullptr;
        return bail(fail(FHE_ERR_NOMEM, "device allocation of %zu bytes for the rotate-bsgs plan", bytes));
    }
    u64 *d = (u64 *)p->d_block;
    if (hipMemcpy(d, h.data(), h.size() * 8, hipMemcpyHostToDevice) != hipSuccess) return bail(fail(FHE_ERR_HIP, "upload of the plaintexts"));
    if (int rc = fhe_qbase_ntt(false, c, d, d, pairs + 1, nullptr)) return bail(rc);
    std::vector<uint64_t> x(row);
    if (hipStreamSynchronize(nullptr) != hipSuccess || hipMemcpy(x.data(), d + (size_t)pairs * row, row * 8, hipMemcpyDeviceToHost) != hipSuccess)
        return bail(fail(FHE_ERR_HIP, "transform of the plaintexts"));
    std::vector<u32> f, fr;
    if (!rotsum::slot_exponents(x.data(), n, c->qb.primes[0], f)) return bail(fail(FHE_ERR_PARAM, "the context's transform of X is not a set of odd powers of one root"));
    for (u32 r = 1; r < k; r++)
        if (!rotsum::slot_exponents(x.data() + (size_t)r * n, n, c->qb.primes[r], fr) || fr != f)
            return bail(fail(FHE_ERR_PARAM, "the context's transforms order their slots differently from prime to prime"));
    std::vector<unsigned char> tail(bytes - b_P, 0);
    u32 *permB = (u32 *)tail.data(), *permG = (u32 *)(tail.data() + b_permB);
    u64 *keysB = (u64 *)(tail.data() + b_permB + b_permG), *keysG = keysB + G1;
    std::copy(grp.begin(), grp.end(), (uint32_t *)(tail.data() + b_permB + b_permG + b_keysB + b_keysG));
    for (u32 j = 0; j < G1; j++) {
        if (!rotsum::slot_perm(f, baby[j], permB + (size_t)j * n)) return bail(fail(FHE_ERR_PARAM, "no slot permutation for Galois element %u", baby[j]));
        keysB[j] = baby[j] == 1 ? 0 : (u64)(uintptr_t)d_baby_keys[j];
    }
    for (u32 i = 0; i < G2; i++) {
        if (!rotsum::slot_perm(f, giant[i], permG + (size_t)i * n)) return bail(fail(FHE_ERR_PARAM, "no slot permutation for Galois element %u", giant[i]));
        keysG[i] = giant[i] == 1 ? 0 : (u64)(uintptr_t)d_giant_keys[i];
    }
    unsigned char *base = (unsigned char *)p->d_block + b_P;
    if (hipMemcpy(base, tail.data(), tail.size(), hipMemcpyHostToDevice) != hipSuccess) return bail(fail(FHE_ERR_HIP, "upload of the rotate-bsgs plan"));
    p->d_P = d;
    p->d_permB = (u32 *)base;
    p->d_permG = (u32 *)(base + b_permB);
    p->d_keysB = (const u64 **)(base + b_permB + b_permG);
    p->d_keysG = p->d_keysB + G1;
    p->d_pgrp = (uint2 *)(base + b_permB + b_permG + b_keysB + b_keysG);
    *out = p;
    return FHE_OK;
}

extern "C" int fhe_rotbsgs_plan_destroy(fhe_rotbsgs_plan *p) {
    if (!p) return FHE_OK;
    if (p->d_block) (void)hipFree(p->d_block);
    delete p;
    return FHE_OK;
}

extern "C" size_t fhe_rotbsgs_scratch_bytes(const fhe_rotbsgs_plan *p, uint64_t count) {
    if (!p) return 0;
    return scratch_words(p, count) * sizeof(u64);
}

extern "C" int fhe_rotate_bsgs_sp(const fhe_rotbsgs_plan *p, const uint64_t *ct2, uint64_t stride, uint64_t *out2, uint64_t out_stride, uint64_t count,
                                  void *scratch, size_t scratch_bytes, fhe_stream s) {
    if (!p || !ct2 || !out2) return fail(FHE_ERR_PARAM, "null argument");
    if (int rc = check_call(p, ct2, stride, out2, out_stride, count, scratch, scratch_bytes)) return rc;
    if (!count) return FHE_OK;
    return run(p, (const u64 *)ct2, stride, (u64 *)out2, out_stride, count, (u64 *)scratch, (hipStream_t)s);
}
