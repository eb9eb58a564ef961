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
// The steps of a call, on either path (T_j and the digit sum are rotdiag_core.h's rot_tap_term and rot_digit_sum):
//   fhe_rot_forward    (rotdiag_core.h) the digit transforms of c_1 and the transform of c_0
//   k_bs_baby(_pm)     the inner accumulators A(i) of every giant step
//   fhe_rot_drop       (rotdiag_core.h) v(i), the drop of every A(i)_1
//   fhe_ksp_forward    (ksp_core.h) the L k digit transforms of every v(i)
//   k_bs_giant         the gathered E(i) against the giant keys, the gathered A(i)_0 word, the identity giant's own words
//   fhe_rot_drop       the last drop
// Pseudo-Mersenne bases, eight launches whatever G1 and G2 are: k_rd_fwd_pm, k_bs_baby_pm (per (c, group of BS_GG giant steps, r, slot):
// per baby step the gathered key sums T_j,0 and T_j,1 ONCE, fanned out to the group's accumulators through the coalesced P_(i,j),r[slot]
// reads), k_ksp_inv_sp_pm, k_rd_inv_down_pm, k_ksp_fwd_pm, k_bs_giant, k_ksp_inv_sp_pm, k_rd_inv_down_pm.
// General path (FP64-transform bases, 61-bit primes, FHE_NTT_NOPM=1): element-wise Barrett kernels around fhe_qbase_ntt / fhe_ksp_forward.
// Every quantity is the canonical residue of the same integer on both paths: the same bits.
#include "rotdiag_core.h"
#include "rotbsgs_host.h"

#include <memory>

struct fhe_rotbsgs_plan {
    const fhe_ctx *ctx = nullptr;
    u32 G1 = 0, G2 = 0, pairs = 0;
    std::vector<u32> baby, giant;
    void *d_block = nullptr;        // one allocation: P [pairs][k][n] u64, the tables below
    u64 *d_P = nullptr;
    u32 *d_permB = nullptr, *d_permG = nullptr;
    const u64 **d_keysB = nullptr, **d_keysG = nullptr;
    uint2 *d_pgrp = nullptr;
    ~fhe_rotbsgs_plan() {
        if (d_block) (void)hipFree(d_block);
    }
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
//   T_j:   rot_tap_term's: at most L + 1 <= FHE_MAX_K mulvv_pm results below RQ each, one fold (below PM_FOLDED: a valid first operand)
//   A(i):  one mulvv_pm(T_j, P_(i,j)) below RQ per PRESENT baby step; the fold counter counts every baby step, present or not, so a
//          register holds a folded value and at most BS_FOLD_BABY products
//   B:     per giant step L products below RQ and the folded word of A(i)_0 (below PM_FOLDED <= RQ): L + 1 <= FHE_MAX_K terms, one fold;
//          the sum over giant steps holds a folded value and at most BS_FOLD_GIANT folded terms (the identity giant adds one folded word)
// rot_bounds_ok (rotdiag_core.h) has T_j, the first operand and A(i); the giant step's own conditions are here.
constexpr int BS_FOLD_BABY = ROT_FOLD_TERMS, BS_FOLD_GIANT = 32;
template <typename C> constexpr bool bs_bounds_ok() {
    return rot_bounds_ok<C>()
           && PM_FOLDED <= C::RQ                                 // the folded word of A(i)_0 counts as one of the per-giant sum's L + 1 terms
           && PM_FOLDED * (1 + BS_FOLD_GIANT) <= 4 * C::LIM;     // B: a folded sum and BS_FOLD_GIANT folded terms
}
static_assert(bs_bounds_ok<PmA>() && bs_bounds_ok<PmB>(), "lazy baby-step / giant-step sums");
static_assert(rotbsgs::MAX_STEPS <= 64 && BS_GG >= 1, "plan limits");

// ---- the baby steps ---------------------------------------------------------------------------------------------------------------------
// general path.  A0 / A1 [c][i][r][s] = sum_(j present) P_(i,j),r[s] T_j,pp,r[s], canonical Barrett products; per (c, i, r) row
__global__ __launch_bounds__(256) void k_bs_baby(const u64 *__restrict__ dig, const u64 *__restrict__ c0h, BsDev P, u64 *__restrict__ A0, u64 *__restrict__ A1,
                                                 const Modulus *__restrict__ mod, u32 k, u32 n, u64 count) {
    using A = ArBarrett;
    const u32 Lq = k - 1;
    const u32 kn = k * n;
    for (u64 u = blockIdx.y; u < count * P.G2 * k; u += gridDim.y) {
        const u32 r = (u32)(u % k), i = (u32)((u / k) % P.G2);
        const u64 c = u / ((u64)k * P.G2);
        const Modulus m = mod[r];
        const u64 pr = P.pr[r];
        const u64 *dr = dig + c * Lq * kn + (u64)r * n, *c0r = c0h + (c * k + r) * n;
        for (u32 s = blockIdx.x * blockDim.x + threadIdx.x; s < n; s += gridDim.x * blockDim.x) {
            u64 s0 = 0, s1 = 0;
            for (u32 j = 0; j < P.G1; j++) {
                const uint2 pg = P.pgrp[(u64)(i / BS_GG) * P.G1 + j];
                if (!(pg.y >> (i % BS_GG) & 1)) continue;              // uniform: an absent pair
                const u32 idx = pg.x + __popc(pg.y & ((1u << (i % BS_GG)) - 1));
                const u64 *key = P.keysB[j];
                u64 a0, a1;
                rot_tap_term<A>(dr, c0r, key ? key + (u64)r * n + s : nullptr, P.permB[(u64)j * n + s], r, Lq, kn, pr, m, a0, a1);
                const u64 w = P.P[((u64)idx * k + r) * n + s];
                s0 = A::add(s0, A::mul(a0, w, m), m);
                s1 = A::add(s1, A::mul(a1, w, m), m);
            }
            A0[u * n + s] = s0;
            A1[u * n + s] = s1;
        }
    }
}
// pseudo-Mersenne path, per (c, group, r, slot): the group's BS_GG giant accumulators (2 BS_GG 64-bit registers) live through the loop over
// the baby steps.  T_j (the gather-bound part) is computed once per baby step and group; the fan-out reads P_(i,j),r[s] coalesced.  A giant
// step past G2 has no bit in the group's mask, so the unrolled fan-out needs no bound on i.
template <typename C>
__global__ __launch_bounds__(256) void k_bs_baby_pm(const u64 *__restrict__ dig, const u64 *__restrict__ c0h, BsDev P, u64 *__restrict__ A0, u64 *__restrict__ A1,
                                                    RnsBase base, u32 n, u64 count) {
    using A = ArPm<C>;
    const u32 k = base.count, Lq = k - 1, NG = (P.G2 + BS_GG - 1) / BS_GG;
    const u32 kn = k * n;
    for (u64 u = blockIdx.y; u < count * NG * k; u += gridDim.y) {
        const u32 r = (u32)(u % k), i0 = (u32)((u / k) % NG) * BS_GG;
        const u64 c = u / ((u64)k * NG);
        const PmMod m = base.pm[r];
        const u64 pr = P.pr[r];
        const u64 *dr = dig + c * Lq * kn + (u64)r * n, *c0r = c0h + (c * k + r) * n;
        for (u32 s = blockIdx.x * blockDim.x + threadIdx.x; s < n; s += gridDim.x * blockDim.x) {
            const u64 *Ps = P.P + (u64)r * n + s;                      // this thread's word of row 0; row idx is idx k n words further
            u64 s0[BS_GG], s1[BS_GG];
#pragma unroll
            for (int g = 0; g < BS_GG; g++) s0[g] = s1[g] = 0;
            u32 since = 0;
            for (u32 j = 0; j < P.G1; j++) {
                const u64 *key = P.keysB[j];
                u64 a0, a1;
                rot_tap_term<A>(dr, c0r, key ? key + (u64)r * n + s : nullptr, P.permB[(u64)j * n + s], r, Lq, kn, pr, m, a0, a1);
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

// ---- the giant steps, one kernel for both paths -----------------------------------------------------------------------------------------
// B [c][pp][r][s] per (c, r, slot).  E [c][i][l][r][n] the digits of v(i), A0 / A1 [c][i][r][n] in NTT form.  ArBarrett: canonical residues,
// the folds and their counter vanish.  ArPm: see the bounds above.
template <typename A>
__global__ __launch_bounds__(256) void k_bs_giant(const u64 *__restrict__ E, const u64 *__restrict__ A0, const u64 *__restrict__ A1, BsDev P, u64 *__restrict__ B,
                                                  typename A::Tab tab, u32 k, u32 n, u64 count) {
    const u32 Lq = k - 1;
    const u32 kn = k * n;
    for (u64 u = blockIdx.y; u < count * k; u += gridDim.y) {
        const u32 r = (u32)(u % k);
        const u64 c = u / k;
        const typename A::Mod m = A::mod(tab, r);
        for (u32 s = blockIdx.x * blockDim.x + threadIdx.x; s < n; s += gridDim.x * blockDim.x) {
            u64 s0 = 0, s1 = 0;
            u32 since = 0;
            for (u32 i = 0; i < P.G2; i++) {
                const u64 *key = P.keysG[i];
                const u64 ci = c * P.G2 + i;
                if (!key) {                                            // uniform: the identity giant step, folded words
                    s0 = A::add(s0, A0[(ci * k + r) * n + s], m);
                    s1 = A::add(s1, A1[(ci * k + r) * n + s], m);
                } else {
                    const u32 src = P.permG[(u64)i * n + s];
                    u64 a0 = A0[(ci * k + r) * n + src], a1 = 0;
                    rot_digit_sum<A>(E + (ci * Lq * k + r) * n + src, key + (u64)r * n + s, Lq, kn, m, a0, a1);
                    s0 = A::add(s0, A::fold(a0, m), m);
                    s1 = A::add(s1, A::fold(a1, m), m);
                }
                if (++since == BS_FOLD_GIANT) {
                    s0 = A::fold(s0, m);
                    s1 = A::fold(s1, m);
                    since = 0;
                }
            }
            B[((c * 2 + 0) * k + r) * n + s] = A::fold(s0, m);
            B[((c * 2 + 1) * k + r) * n + s] = A::fold(s1, m);
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
    const bool pm = fhe_rot_pm(c), a = c->qb.pm_class == 1;
    const dim3 gb = ksp_grid2(n, count * ((G2 + BS_GG - 1) / BS_GG) * k), gg = ksp_grid2(n, count * k);
    int rc;
    if ((rc = fhe_rot_forward(c, ct, stride, S.dig, S.c0h, count, st))) return rc;
    if (!pm) k_bs_baby<<<ksp_grid2(n, rows * k), 256, 0, st>>>(S.dig, S.c0h, P, S.A0, S.A1, c->qb.d_mod, k, n, count);
    else if (a) k_bs_baby_pm<PmA><<<gb, 256, 0, st>>>(S.dig, S.c0h, P, S.A0, S.A1, c->qb.dev(), n, count);
    else k_bs_baby_pm<PmB><<<gb, 256, 0, st>>>(S.dig, S.c0h, P, S.A0, S.A1, c->qb.dev(), n, count);
    KERNEL_CHECK();
    // v(i): A1 [rows][k][n] read as pairs of rows, written as contiguous [rows][L][n] (row = c' * 2 + pp, "stride" 2 L n).  The identity giant
    // step reads A1 in NTT form and the general path's drop transforms in place, so there a COPY is dropped: the first [rows][k][n] words of
    // E hold it until v is written; the digits of v then overwrite them
    u64 *A1d = S.A1;
    if (!pm) {
        A1d = S.E;
        if (hipMemcpyAsync(A1d, S.A1, rows * k * n * sizeof(u64), hipMemcpyDeviceToDevice, st) != hipSuccess) return fail(FHE_ERR_HIP, "copy of the inner accumulators");
    }
    if ((rc = fhe_rot_drop(c, A1d, S.spA, S.v, 2 * (u64)Lq * n, rows, st))) return rc;
    if ((rc = fhe_ksp_forward(c, S.v, (u64)Lq * n, 0, S.E, rows, st))) return rc;
    if (!pm) k_bs_giant<ArBarrett><<<gg, 256, 0, st>>>(S.E, S.A0, S.A1, P, S.B, c->qb.d_mod, k, n, count);
    else if (a) k_bs_giant<ArPm<PmA>><<<gg, 256, 0, st>>>(S.E, S.A0, S.A1, P, S.B, c->qb.dev(), k, n, count);
    else k_bs_giant<ArPm<PmB>><<<gg, 256, 0, st>>>(S.E, S.A0, S.A1, P, S.B, c->qb.dev(), k, n, count);
    KERNEL_CHECK();
    return fhe_rot_drop(c, S.B, S.spB, out, out_stride, count * 2, st);
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
    // rows 0 .. pairs - 1 of the block: the centred lifts of the present pairs, transformed with the row of X behind them (fhe_rot_slot_exponents)
    const size_t row = (size_t)k * n, b_P = (size_t)(pairs + 1) * row * 8;
    const size_t b_permB = (((size_t)G1 * n * 4) + 7) & ~(size_t)7, b_permG = (((size_t)G2 * n * 4) + 7) & ~(size_t)7;
    const size_t b_keysB = (size_t)G1 * 8, b_keysG = (size_t)G2 * 8, b_pgrp = grp.size() * 4;
    std::vector<uint64_t> h((size_t)pairs * row, 0);
    const std::vector<uint64_t> primes(c->qb.primes.begin(), c->qb.primes.end());
    for (size_t u = 0; u < (size_t)G1 * G2; u++)
        if (idx[u] >= 0) rotdiag::lift(plains + u * n, n, c->t, primes.data(), k, h.data() + (size_t)idx[u] * row);
    std::unique_ptr<fhe_rotbsgs_plan> p(new fhe_rotbsgs_plan);
    p->ctx = c;
    p->G1 = G1;
    p->G2 = G2;
    p->pairs = pairs;
    p->baby.assign(baby, baby + G1);
    p->giant.assign(giant, giant + G2);
    const size_t bytes = b_P + b_permB + b_permG + b_keysB + b_keysG + b_pgrp;
    if (hipMalloc(&p->d_block, bytes) != hipSuccess) {
        p->d_block = nullptr;
        return fail(FHE_ERR_NOMEM, "device allocation of %zu bytes for the rotate-bsgs plan", bytes);
    }
    u64 *d = (u64 *)p->d_block;
    if (hipMemcpy(d, h.data(), h.size() * 8, hipMemcpyHostToDevice) != hipSuccess) return fail(FHE_ERR_HIP, "upload of the plaintexts");
    std::vector<u32> f;
    if (int rc = fhe_rot_slot_exponents(c, d, pairs, "the plaintexts", f)) return rc;
    std::vector<unsigned char> tail(bytes - b_P, 0);
    u32 *permB = (u32 *)tail.data(), *permG = (u32 *)(tail.data() + b_permB);
    u64 *keysB = (u64 *)(tail.data() + b_permB + b_permG), *keysG = keysB + G1;
    std::copy(grp.begin(), grp.end(), (uint32_t *)(tail.data() + b_permB + b_permG + b_keysB + b_keysG));
    if (int rc = fhe_rot_perm_keys(f, G1, baby, d_baby_keys, permB, keysB)) return rc;
    if (int rc = fhe_rot_perm_keys(f, G2, giant, d_giant_keys, permG, keysG)) return rc;
    unsigned char *base = (unsigned char *)p->d_block + b_P;
    if (hipMemcpy(base, tail.data(), tail.size(), hipMemcpyHostToDevice) != hipSuccess) return fail(FHE_ERR_HIP, "upload of the rotate-bsgs plan");
    p->d_P = d;
    p->d_permB = (u32 *)base;
    p->d_permG = (u32 *)(base + b_permB);
    p->d_keysB = (const u64 **)(base + b_permB + b_permG);
    p->d_keysG = p->d_keysB + G1;
    p->d_pgrp = (uint2 *)(base + b_permB + b_permG + b_keysB + b_keysG);
    *out = p.release();
    return FHE_OK;
}

extern "C" int fhe_rotbsgs_plan_destroy(fhe_rotbsgs_plan *p) {
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
    const fhe_ctx *c = p->ctx;
    const u64 launch = count > 0x7fffffffULL ? ~0ULL : count * p->G2 * c->k * c->k;      // the product itself must not wrap
    const std::string why = rotsum::check_call(c->k, c->n, ct2, stride, out2, out_stride, count, launch, scratch_words(p, count) * sizeof(u64), scratch, scratch_bytes);
    if (!why.empty()) return fail(FHE_ERR_PARAM, "%s", why.c_str());
    if (!count) return FHE_OK;
    return run(p, (const u64 *)ct2, stride, (u64 *)out2, out_stride, count, (u64 *)scratch, (hipStream_t)s);
}
