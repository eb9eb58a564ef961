// rotdiag.hip -- a diagonal linear map on the slots of ONE ciphertext under one special-prime key switch: fhe_rotate_diag_sum_sp on gfx950,
// out = sum_j p_j * rot_(g_j)(ct) with a plaintext POLYNOMIAL p_j per tap (a vector of slot values, through the batch encoder).
// include/fhe_hip.h states the operation; DESIGN.md 3.16 has the range proof and the resource table.
//
// With D_i,r and pi_g as in rotsum.hip, p'_j the centred lift of p_j and P_j,r = NTT_(q_r)(p'_j) in the context's own slot order:
//     acc_pp,r = sum_(j: g_j != 1) P_j,r (*) sum_(i < L) pi_(g_j)(D_i,r) (*) K_j,i,pp,r  mod q_r      for every r < k
//     u_pp     = one drop of fhe_mod_switch (k -> k - 1) of acc_pp
//     out      = (u_0 + sum_j p'_j sigma_(g_j)(c_0),  u_1 + sum_(j: g_j = 1) p'_j c_1)                   (products in R_(q_r))
// The products with p'_j are polynomial products, so c_0 is transformed too (C0_r = NTT_(q_r)(c_0,r), r < L) and joins the accumulation as one
// more digit whose "key" is the constant [p]_(q_r) (p the special prime): with z = sum_j p'_j sigma_(g_j)(c_0),
//     acc'_0,r = acc_0,r + [p]_(q_r) sum_j P_j,r (*) pi_(g_j)(C0_r)   for r < L,   acc'_0,p = acc_0,p
// and the drop of acc'_0 is u_0 + z EXACTLY: the drop subtracts a value that depends on the special prime's residue alone, which is unchanged,
// and multiplies by p^-1 mod q_r.  The identity tap's c_1 term is [p]_(q_r) P_id,r (*) D_r,r in acc'_1,r in the same way.  The tail is then an
// inverse transform and the drop, with no read of the input: every input word is in scratch before the first store, so out2 may be ct2.
//
// Pseudo-Mersenne bases, four launches whatever the number of taps:
//   k_rd_fwd_pm        workgroup (c, i, r): k_ksp_fwd_pm's digit transforms of c_1, and (c, r < L): the transform of c_0,r
//   k_rd_accum_pm      per (c, r, slot): per tap L gathered digits against both key polynomials plus the gathered C0 word against [p]_(q_r),
//                      folded, times P_j,r[slot]; lazy sum over taps
//   k_ksp_inv_sp_pm    (keyswitch_sp.hip)
//   k_rd_inv_down_pm   workgroup (c, pp, r < L): inverse transform, the drop, the store
// General path (FP64-transform bases, 61-bit primes, FHE_NTT_NOPM=1): element-wise Barrett kernels around fhe_qbase_ntt.  Every quantity is
// the canonical residue of the same integer on both paths: the same bits.
#include "rotdiag_core.h"
#include "rotdiag_host.h"

struct fhe_rotdiag_plan {
    const fhe_ctx *ctx = nullptr;
    u32 taps = 0;
    std::vector<u32> elts;
    void *d_block = nullptr;        // one allocation: P [taps][k][n] u64, perm [taps][n] u32 (the identity for g = 1), keys [taps]
    u64 *d_P = nullptr;
    u32 *d_perm = nullptr;
    const u64 **d_keys = nullptr;
};

namespace {

struct RdTaps {
    const u32 *perm;            // [taps][n]: slot s of pi_(g_j) reads slot perm[j][s]
    const u64 *P;               // [taps][k][n]: NTT_(q_r)(p'_j), canonical, the context's slot order
    const u64 *const *keys;     // [taps]: [L][2][k][n] NTT form, null for g_j = 1
    u64 pr[FHE_MAX_K];          // the special prime modulo q_r, r < L
    u32 taps;
};

// rotsum.hip's lazy tap sum (a term is a mulvv_pm result below RQ / 16 q, folded every RD_FOLD_TAPS terms), with one more term in the sum of
// a tap: the L digit products and the C0 product, L + 1 <= FHE_MAX_K terms below RQ each in 64 bits (48 q of 512 on class A, 12 q of 64 on
// class B).  The diagonal word P_j,r[s] is canonical, as the scalar weight was: the product bound RQ is the same.
constexpr int RD_FOLD_TAPS = 32;
template <typename C> constexpr bool rd_bounds_ok() {
    return PM_FOLDED + RD_FOLD_TAPS * C::RQ <= 4 * C::LIM        // a folded sum and RD_FOLD_TAPS more terms fit 64 bits
           && FHE_MAX_K * C::RQ <= 4 * C::LIM                    // the L + 1 <= 8 products of one tap do
           && PM_FOLDED <= 32;                                   // a folded value is a valid first operand of mulvv_pm (below 2^(b+1))
}
static_assert(rd_bounds_ok<PmA>() && rd_bounds_ok<PmB>(), "lazy tap sums");

// ---- general path -------------------------------------------------------------------------------------------------------------------
// c0h [count][k][n]: c_0,r for r < L, zeros at the special prime, for the base's own forward transforms
__global__ __launch_bounds__(256) void k_rd_stage_c0(const u64 *__restrict__ ct, u64 stride, u64 *__restrict__ c0h, u32 k, u32 n, u64 count) {
    for (u64 u = blockIdx.y; u < count * k; u += gridDim.y) {
        const u32 r = (u32)(u % k);
        const u64 c = u / k;
        const u64 *src = ct + c * stride + (u64)r * n;
        for (u32 x = blockIdx.x * blockDim.x + threadIdx.x; x < n; x += gridDim.x * blockDim.x) c0h[u * n + x] = r < k - 1 ? src[x] : 0;
    }
}
// acc[c][pp][r][s] = sum_j P_j,r[s] (sum_i dig[c][i][r][perm_j[s]] key_j[i][pp][r][s] + [p]_(q_r) (pp = 0: c0h[c][r][perm_j[s]]; pp = 1 and
// g_j = 1: dig[c][r][r][s])), canonical Barrett products
__global__ __launch_bounds__(256) void k_rd_accum(const u64 *__restrict__ dig, const u64 *__restrict__ c0h, RdTaps P, u64 *__restrict__ acc,
                                                  const Modulus *__restrict__ mod, u32 k, u32 n, u64 count) {
    const u32 Lq = k - 1;
    for (u64 u = blockIdx.y; u < count * k; u += gridDim.y) {
        const u32 r = (u32)(u % k);
        const u64 c = u / k;
        const Modulus m = mod[r];
        const bool low = r < Lq;
        const u64 pr = P.pr[r];
        for (u32 s = blockIdx.x * blockDim.x + threadIdx.x; s < n; s += gridDim.x * blockDim.x) {
            u64 s0 = 0, s1 = 0;
            for (u32 j = 0; j < P.taps; j++) {
                const u64 *key = P.keys[j];
                const u32 src = P.perm[(u64)j * n + s];
                u64 a0 = 0, a1 = 0;
                if (key) {
                    for (u32 i = 0; i < Lq; i++) {
                        const u64 x = dig[((c * Lq + i) * k + r) * n + src];
                        const u64 *e = key + (((u64)i * 2) * k + r) * n + s;
                        a0 = addmod(a0, mul_barrett(x, e[0], m), m.q);
                        a1 = addmod(a1, mul_barrett(x, e[(u64)k * n], m), m.q);
                    }
                }
                if (low) {
                    a0 = addmod(a0, mul_barrett(c0h[(c * k + r) * n + src], pr, m), m.q);
                    if (!key) a1 = mul_barrett(dig[((c * Lq + r) * k + r) * n + src], pr, m);
                }
                const u64 w = P.P[((u64)j * k + r) * n + s];
                s0 = addmod(s0, mul_barrett(a0, w, m), m.q);
                s1 = addmod(s1, mul_barrett(a1, w, m), m.q);
            }
            acc[((c * 2 + 0) * k + r) * n + s] = s0;
            acc[((c * 2 + 1) * k + r) * n + s] = s1;
        }
    }
}
// acc in coefficient form: the drop of the special prime
__global__ __launch_bounds__(256) void k_rd_down(u64 *__restrict__ out, u64 out_stride, const u64 *__restrict__ acc, KspTab T, u32 k, u32 n, u64 count) {
    const u32 Lq = k - 1;
    for (u64 u = blockIdx.y; u < count * 2 * Lq; u += gridDim.y) {
        const u32 r = (u32)(u % Lq), pp = (u32)((u / Lq) & 1);
        const u64 c = u / (2 * Lq);
        const u64 *a = acc + ((c * 2 + pp) * k + r) * n, *ap = acc + ((c * 2 + pp) * k + Lq) * n;
        u64 *dst = out + c * out_stride + ((u64)pp * Lq + r) * n;
        for (u32 j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) dst[j] = ksp_drop(a[j], ap[j], T, r);
    }
}

// ---- pseudo-Mersenne path -------------------------------------------------------------------------------------------------------------
// (1) k_rd_fwd_pm (rotdiag_core.h)
// (2) per (c, r, slot).  Per tap: k_rs_accum_pm's L gathered digits against both key polynomials, and for r < L the gathered C0 word (pp = 0)
// or, on the identity tap, D_r,r (pp = 1) against the canonical [p]_(q_r): at most L + 1 <= 8 mulvv_pm terms below RQ each in a 64-bit sum
// (rd_bounds_ok); one fold (below PM_FOLDED / 16 q < 2^(b+1): a valid first operand of mulvv_pm); the product with the canonical P_j,r[s] is
// below RQ again.  The sum over taps holds a folded value and at most RD_FOLD_TAPS such products.
template <typename C>
__global__ __launch_bounds__(256) void k_rd_accum_pm(const u64 *__restrict__ dig, const u64 *__restrict__ c0h, RdTaps P, u64 *__restrict__ acc, RnsBase base,
                                                     u32 n, u64 count) {
    const u32 k = base.count, Lq = k - 1;
    for (u64 u = blockIdx.y; u < count * k; u += gridDim.y) {
        const u32 r = (u32)(u % k);
        const u64 c = u / k;
        const PmMod m = base.pm[r];
        const bool low = r < Lq;
        const u64 pr = P.pr[r];
        for (u32 s = blockIdx.x * blockDim.x + threadIdx.x; s < n; s += gridDim.x * blockDim.x) {
            u64 s0 = 0, s1 = 0;
            u32 since = 0;
            for (u32 j = 0; j < P.taps; j++) {
                const u64 *key = P.keys[j];
                const u32 src = P.perm[(u64)j * n + s];
                u64 a0 = 0, a1 = 0;
                if (key) {                                             // uniform: every tap but the one with g = 1
                    for (u32 i = 0; i < Lq; i++) {
                        const u64 x = dig[((c * Lq + i) * k + r) * n + src];
                        const u64 *e = key + (((u64)i * 2) * k + r) * n + s;
                        a0 += mulvv_pm(x, e[0], m);
                        a1 += mulvv_pm(x, e[(u64)k * n], m);
                    }
                }
                if (low) {                                             // uniform per row
                    a0 += mulvv_pm(c0h[(c * k + r) * n + src], pr, m);
                    if (!key) a1 = mulvv_pm(dig[((c * Lq + r) * k + r) * n + src], pr, m);
                }
                const u64 w = P.P[((u64)j * k + r) * n + s];
                s0 += mulvv_pm(fold_pm(a0, m), w, m);
                s1 += mulvv_pm(fold_pm(a1, m), w, m);
                if (++since == RD_FOLD_TAPS) {
                    s0 = fold_pm(s0, m);
                    s1 = fold_pm(s1, m);
                    since = 0;
                }
            }
            acc[((c * 2 + 0) * k + r) * n + s] = fold_pm(s0, m);
            acc[((c * 2 + 1) * k + r) * n + s] = fold_pm(s1, m);
        }
    }
}
// (4) k_rd_inv_down_pm (rotdiag_core.h)

// the digits [L][k][n], C0 [k][n] (the special prime's row is used by the general path alone), the accumulators [2][k][n] and the special
// prime's coefficients [2][n] (pseudo-Mersenne path) per ciphertext
size_t scratch_words(const fhe_rotdiag_plan *p, u64 count) {
    const u64 k = p->ctx->k, Lq = k - 1, n = p->ctx->n;
    return (size_t)(count * (Lq * k + k + 2 * k + 2) * n);
}

int run(const fhe_rotdiag_plan *p, const u64 *ct, u64 stride, u64 *out, u64 out_stride, u64 count, u64 *scratch, hipStream_t st) {
    const fhe_ctx *c = p->ctx;
    const u32 k = c->k, Lq = k - 1, n = c->n;
    u64 *dig = scratch, *c0h = dig + count * Lq * k * n, *acc = c0h + count * k * n, *sp = acc + count * 2 * k * n;
    const KspTab T = ksp_tab(c);
    RdTaps P{p->d_perm, p->d_P, p->d_keys, {0}, p->taps};
    for (u32 r = 0; r < Lq; r++) P.pr[r] = T.p % T.q[r];
    int rc;
    if (fhe_ksp_pm_ok(c, count)) {
        const RnsBase base = c->qb.dev();
        const unsigned g1 = (unsigned)(count * (Lq * k + Lq)), g4 = (unsigned)(count * 2 * Lq);
        const dim3 g2 = ksp_grid2(n, count * k);
        if (c->qb.pm_class == 1) {
            DISPATCH_L(c->logn, (k_rd_fwd_pm<L, PmA><<<g1, NttShape<L>::TP, 0, st>>>(ct, stride, dig, c0h, base)));
            k_rd_accum_pm<PmA><<<g2, 256, 0, st>>>(dig, c0h, P, acc, base, n, count);
        } else {
            DISPATCH_L(c->logn, (k_rd_fwd_pm<L, PmB><<<g1, NttShape<L>::TP, 0, st>>>(ct, stride, dig, c0h, base)));
            k_rd_accum_pm<PmB><<<g2, 256, 0, st>>>(dig, c0h, P, acc, base, n, count);
        }
        KERNEL_CHECK();
        if ((rc = fhe_ksp_inv_sp(c, acc, sp, count * 2, st))) return rc;
        if (c->qb.pm_class == 1) { DISPATCH_L(c->logn, (k_rd_inv_down_pm<L, PmA><<<g4, NttShape<L>::TP, 0, st>>>(out, out_stride, acc, sp, base, T))); }
        else { DISPATCH_L(c->logn, (k_rd_inv_down_pm<L, PmB><<<g4, NttShape<L>::TP, 0, st>>>(out, out_stride, acc, sp, base, T))); }
        KERNEL_CHECK();
        return FHE_OK;
    }
    k_rd_stage_c0<<<ksp_grid2(n, count * k), 256, 0, st>>>(ct, stride, c0h, k, n, count);
    KERNEL_CHECK();
    if ((rc = fhe_qbase_ntt(false, c, c0h, c0h, count, st))) return rc;
    if ((rc = fhe_ksp_forward(c, ct, stride, 1, dig, count, st))) return rc;
    k_rd_accum<<<ksp_grid2(n, count * k), 256, 0, st>>>(dig, c0h, P, acc, c->qb.d_mod, k, n, count);
    KERNEL_CHECK();
    if ((rc = fhe_qbase_ntt(true, c, acc, acc, count * 2, st))) return rc;
    k_rd_down<<<ksp_grid2(n, count * 2 * Lq), 256, 0, st>>>(out, out_stride, acc, T, k, n, count);
    KERNEL_CHECK();
    return FHE_OK;
}

// in the order include/fhe_hip.h lists them (fhe_rotate_sum_sp's)
int check_call(const fhe_rotdiag_plan *p, const void *ct, u64 stride, const void *out, u64 out_stride, u64 count, const void *scratch, size_t scratch_bytes) {
    const fhe_ctx *c = p->ctx;
    const u64 Ln = (u64)(c->k - 1) * c->n;
    if (stride < 2 * Ln) return fail(FHE_ERR_PARAM, "ciphertext stride smaller than a size-2 ciphertext of %u primes", c->k - 1);
    if (out_stride < 2 * Ln) return fail(FHE_ERR_PARAM, "output stride smaller than a size-2 ciphertext of %u primes", c->k - 1);
    if (!count) return FHE_OK;
    if (count * c->k * c->k > 0x7fffffffULL) return fail(FHE_ERR_PARAM, "too many ciphertexts for one call");
    const size_t need = scratch_words(p, count) * sizeof(u64);
    if (!scratch || scratch_bytes < need) return fail(FHE_ERR_PARAM, "scratch too small");
    const u64 in_words = (count - 1) * stride + 2 * Ln, out_words = (count - 1) * out_stride + 2 * Ln;
    if (!(out == ct && out_stride == stride) && overlap(ct, in_words, out, out_words))
        return fail(FHE_ERR_PARAM, "output range overlaps the input range (only out2 == ct2 with out_stride == stride may alias)");
    if (overlap(scratch, need / 8, ct, in_words) || overlap(scratch, need / 8, out, out_words)) return fail(FHE_ERR_PARAM, "scratch overlaps the input or the output");
    return FHE_OK;
}

}  // namespace

extern "C" int fhe_rotdiag_plan_create(const fhe_ctx *c, uint32_t taps, const uint32_t *elts, const uint64_t *plains, const uint64_t *const *d_keys,
                                       fhe_rotdiag_plan **out) {
    if (!c || !out || !elts || !plains || !d_keys) return fail(FHE_ERR_PARAM, "null argument");
    const u32 n = c->n, k = c->k;
    const std::vector<uint64_t> ones(taps && taps <= rotsum::MAX_TAPS ? taps : 0, 1);      // the weights' check is the plaintexts', below
    std::string why = rotsum::check_taps(n, c->t, k, taps, elts, ones.data(), (const void *const *)d_keys);
    if (why.empty()) why = rotdiag::check_plains(n, c->t, taps, plains);
    if (!why.empty()) return fail(FHE_ERR_PARAM, "%s", why.c_str());
    // rows 0 .. taps - 1: the centred lifts; row taps: the monomial X.  One run of the context's own forward transform: slot s of X holds psi_r^(e_s)
    const size_t row = (size_t)k * n, b_P = (size_t)taps * row * 8, b_perm = (((size_t)taps * n * 4) + 7) & ~(size_t)7, b_keys = (size_t)taps * 8;
    std::vector<uint64_t> h((taps + 1) * row, 0);
    const std::vector<uint64_t> primes(c->qb.primes.begin(), c->qb.primes.end());
    for (u32 j = 0; j < taps; j++) rotdiag::lift(plains + (size_t)j * n, n, c->t, primes.data(), k, h.data() + j * row);
    for (u32 r = 0; r < k; r++) h[taps * row + (size_t)r * n + 1] = 1;
    fhe_rotdiag_plan *p = new fhe_rotdiag_plan;
    p->ctx = c;
    p->taps = taps;
    p->elts.assign(elts, elts + taps);
    auto bail = [&](int rc) {
        if (p->d_block) (void)hipFree(p->d_block);
        delete p;
        return rc;
    };
    // the block is sized for the transform's input (taps + 1 rows); the permutations and the keys then take the place of the row of X and what follows
    const size_t bytes = b_P + (row * 8 > b_perm + b_keys ? row * 8 : b_perm + b_keys);
    if (hipMalloc(&p->d_block, bytes) != hipSuccess) {
        p->d_block = nullptr;
        return bail(fail(FHE_ERR_NOMEM, "device allocation of %zu bytes for the rotate-diag plan", bytes));
    }
    u64 *d = (u64 *)p->d_block;
    if (hipMemcpy(d, h.data(), h.size() * 8, hipMemcpyHostToDevice) != hipSuccess) return bail(fail(FHE_ERR_HIP, "upload of the plaintexts"));
    if (int rc = fhe_qbase_ntt(false, c, d, d, taps + 1, nullptr)) return bail(rc);
    std::vector<uint64_t> x(row);
    if (hipStreamSynchronize(nullptr) != hipSuccess || hipMemcpy(x.data(), d + taps * row, row * 8, hipMemcpyDeviceToHost) != hipSuccess)
        return bail(fail(FHE_ERR_HIP, "transform of the plaintexts"));
    std::vector<u32> f, fr;
    if (!rotsum::slot_exponents(x.data(), n, c->qb.primes[0], f)) return bail(fail(FHE_ERR_PARAM, "the context's transform of X is not a set of odd powers of one root"));
    for (u32 r = 1; r < k; r++)
        if (!rotsum::slot_exponents(x.data() + (size_t)r * n, n, c->qb.primes[r], fr) || fr != f)
            return bail(fail(FHE_ERR_PARAM, "the context's transforms order their slots differently from prime to prime"));
    std::vector<unsigned char> tail(b_perm + b_keys, 0);
    u32 *perm = (u32 *)tail.data();
    u64 *keys = (u64 *)(tail.data() + b_perm);
    for (u32 j = 0; j < taps; j++) {
        const u32 g = elts[j];
        if (!rotsum::slot_perm(f, g, perm + (size_t)j * n)) return bail(fail(FHE_ERR_PARAM, "no slot permutation for Galois element %u", g));
        keys[j] = g == 1 ? 0 : (u64)(uintptr_t)d_keys[j];
    }
    if (hipMemcpy((unsigned char *)p->d_block + b_P, tail.data(), tail.size(), hipMemcpyHostToDevice) != hipSuccess)
        return bail(fail(FHE_ERR_HIP, "upload of the rotate-diag plan"));
    p->d_P = d;
    p->d_perm = (u32 *)((unsigned char *)p->d_block + b_P);
    p->d_keys = (const u64 **)((unsigned char *)p->d_block + b_P + b_perm);
    *out = p;
    return FHE_OK;
}

extern "C" int fhe_rotdiag_plan_destroy(fhe_rotdiag_plan *p) {
    if (!p) return FHE_OK;
    if (p->d_block) (void)hipFree(p->d_block);
    delete p;
    return FHE_OK;
}

extern "C" size_t fhe_rotdiag_scratch_bytes(const fhe_rotdiag_plan *p, uint64_t count) {
    if (!p) return 0;
    return scratch_words(p, count) * sizeof(u64);
}

extern "C" int fhe_rotate_diag_sum_sp(const fhe_rotdiag_plan *p, const uint64_t *ct2, uint64_t stride, uint64_t *out2, uint64_t out_stride, uint64_t count,
                                      void *scratch, size_t scratch_bytes, fhe_stream s) {
    if (!p || !ct2 || !out2) return fail(FHE_ERR_PARAM, "null argument");
    if (int rc = check_call(p, ct2, stride, out2, out_stride, count, scratch, scratch_bytes)) return rc;
    if (!count) return FHE_OK;
    return run(p, (const u64 *)ct2, stride, (u64 *)out2, out_stride, count, (u64 *)scratch, (hipStream_t)s);
}
