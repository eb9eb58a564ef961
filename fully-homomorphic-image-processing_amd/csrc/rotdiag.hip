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
// The steps of a call, on either path:
//   fhe_rot_forward    the digit transforms of c_1 and the transform of c_0
//   k_rd_accum         per (c, r, slot): per tap L gathered digits against both key polynomials plus the gathered C0 word against [p]_(q_r)
//                      (rotdiag_core.h's rot_tap_term), times P_j,r[slot]; the sum over taps
//   fhe_rot_drop       inverse transform, the drop, the store
// Pseudo-Mersenne bases, four launches whatever the number of taps: k_rd_fwd_pm (workgroup (c, i, r): k_ksp_fwd_pm's digit transforms of
// c_1, and (c, r < L): the transform of c_0,r), k_rd_accum<ArPm<C>> (lazy sums), k_ksp_inv_sp_pm (keyswitch_sp.hip), k_rd_inv_down_pm.
// General path (FP64-transform bases, 61-bit primes, FHE_NTT_NOPM=1), seven: k_rd_stage_c0, the base's transform and fhe_ksp_forward;
// k_rd_accum<ArBarrett>; fhe_qbase_ntt and k_rd_down.  Every quantity is the canonical residue of the same integer on both paths: the
// same bits.
// This file also defines, once, what rotdiag_core.h declares for rotbsgs.hip and rotsum.hip: the forward and the drop step with their
// kernels and dispatches, and the two halves of plan creation (the slot exponents from the transform of X; the permutation and key tables).
#include "rotdiag_core.h"
#include "rotdiag_host.h"

#include <memory>

struct fhe_rotdiag_plan {
    const fhe_ctx *ctx = nullptr;
    u32 taps = 0;
    std::vector<u32> elts;
    void *d_block = nullptr;        // one allocation: P [taps][k][n] u64, perm [taps][n] u32 (the identity for g = 1), keys [taps]
    u64 *d_P = nullptr;
    u32 *d_perm = nullptr;
    const u64 **d_keys = nullptr;
    ~fhe_rotdiag_plan() {
        if (d_block) (void)hipFree(d_block);
    }
};

namespace {

struct RdTaps {
    const u32 *perm;            // [taps][n]: slot s of pi_(g_j) reads slot perm[j][s]
    const u64 *P;               // [taps][k][n]: NTT_(q_r)(p'_j), canonical, the context's slot order
    const u64 *const *keys;     // [taps]: [L][2][k][n] NTT form, null for g_j = 1
    u64 pr[FHE_MAX_K];          // the special prime modulo q_r, r < L
    u32 taps;
};

// The lazy tap sum of the pseudo-Mersenne path is rotdiag_core.h's (rot_bounds_ok): per tap the L digit products and the C0 product, L + 1 <=
// FHE_MAX_K terms below RQ each in 64 bits (48 q of 512 on class A, 12 q of 64 on class B), one fold, and the product with the canonical
// diagonal word P_j,r[s], below RQ again; the sum over taps is folded every ROT_FOLD_TERMS products.

// ---- the shared steps (rotdiag_core.h) --------------------------------------------------------------------------------------------------
// general path: c0h [count][k][n] = c_0,r for r < L, zeros at the special prime, for the base's own forward transforms
__global__ __launch_bounds__(256) void k_rd_stage_c0(const u64 *__restrict__ ct, u64 stride, u64 *__restrict__ c0h, u32 k, u32 n, u64 count) {
    for (u64 u = blockIdx.y; u < count * k; u += gridDim.y) {
        const u32 r = (u32)(u % k);
        const u64 c = u / k;
        const u64 *src = ct + c * stride + (u64)r * n;
        for (u32 x = blockIdx.x * blockDim.x + threadIdx.x; x < n; x += gridDim.x * blockDim.x) c0h[u * n + x] = r < k - 1 ? src[x] : 0;
    }
}
// general path: acc [rows][k][n] in coefficient form -> the drop of the special prime; row = c * 2 + pp goes to out + c * out_stride + (pp L + r) n
__global__ __launch_bounds__(256) void k_rd_down(u64 *__restrict__ out, u64 out_stride, const u64 *__restrict__ acc, KspTab T, u32 k, u32 n, u64 rows) {
    const u32 Lq = k - 1;
    for (u64 u = blockIdx.y; u < rows * Lq; u += gridDim.y) {
        const u32 r = (u32)(u % Lq);
        const u64 row = u / Lq;
        const u64 *a = acc + (row * k + r) * n, *ap = acc + (row * k + Lq) * n;
        u64 *dst = out + (row >> 1) * out_stride + ((row & 1) * Lq + r) * n;
        for (u32 j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) dst[j] = ksp_drop(a[j], ap[j], T, r);
    }
}
// pseudo-Mersenne path, per ciphertext L k + L workgroups.  The first L k are k_ksp_fwd_pm's (c, i, r): dig[c][i][r] = NTT_(q_r)([c_1,i]_(q_r)),
// folded below PM_FOLDED when r != i.  The last L are (c, r): c0h[c][r] = NTT_(q_r)(c_0,r), canonical input.
template <int L, typename C>
__global__ __launch_bounds__(NttShape<L>::TP, 4) void k_rd_fwd_pm(const u64 *__restrict__ ct, u64 stride, u64 *__restrict__ dig, u64 *__restrict__ c0h, RnsBase base) {
    __shared__ u64 lds[NttShape<L>::LDS_WORDS];
    constexpr int N = NttShape<L>::N;
    const int tid = threadIdx.x;
    const u32 k = base.count, Lq = k - 1, per = Lq * k + Lq, w = blockIdx.x % per;
    const u64 c = blockIdx.x / per;
    const bool d = w < Lq * k;                     // uniform per workgroup
    const u32 r = d ? w % k : w - Lq * k, i = d ? w / k : r;
    const PmMod m = base.pm[r];
    u64 x[1][16];
    load_coeff<L>(x[0], ct + c * stride + ((u64)(d ? Lq : 0) + i) * N, tid);
    if (r != i) {
#pragma unroll
        for (int e = 0; e < 16; e++) x[0][e] = fold_pm(x[0][e], m);
    }
    ntt_fwd_regs_pm<L, 1, PM_FOLDED, C::LIM, C::CS>(x, base.tw_pm + (size_t)r * N, m, lds, tid);
#pragma unroll
    for (int e = 0; e < 16; e++) x[0][e] = canon_pm(x[0][e], m);
    store_slots<L>(x[0], d ? dig + ((c * Lq + i) * k + r) * N : c0h + (c * k + r) * N, tid);
}
// pseudo-Mersenne path, workgroup (row = c * 2 + pp, r < L): k_ksp_inv_down_add_pm's transform and drop, nothing added: the input's terms
// went through the accumulator
template <int L, typename C>
__global__ __launch_bounds__(NttShape<L>::TP, 4) void k_rd_inv_down_pm(u64 *__restrict__ out, u64 out_stride, const u64 *__restrict__ acc, const u64 *__restrict__ sp,
                                                                        RnsBase base, KspTab T) {
    __shared__ u64 lds[NttShape<L>::LDS_WORDS];
    constexpr int N = NttShape<L>::N;
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
    store_coeff<L>(x[0], out + c * out_stride + ((u64)pp * Lq + r) * N, tid);
}

// ---- the accumulation, one kernel for both paths ----------------------------------------------------------------------------------------
// acc[c][pp][r][s] = sum_j P_j,r[s] T_j,pp,r[s] per (c, r, slot), T_j rot_tap_term's.  ArBarrett: canonical residues throughout, the folds
// and their counter vanish.  ArPm: T_j is folded once (below PM_FOLDED / 16 q < 2^(b+1): a valid first operand of mulvv_pm), the product
// with the canonical P_j,r[s] is below RQ again, and the sum over taps holds a folded value and at most ROT_FOLD_TERMS such products.
template <typename A>
__global__ __launch_bounds__(256) void k_rd_accum(const u64 *__restrict__ dig, const u64 *__restrict__ c0h, RdTaps P, u64 *__restrict__ acc, typename A::Tab tab,
                                                  u32 k, u32 n, u64 count) {
    const u32 Lq = k - 1;
    const u32 kn = k * n;
    for (u64 u = blockIdx.y; u < count * k; u += gridDim.y) {
        const u32 r = (u32)(u % k);
        const u64 c = u / k;
        const typename A::Mod m = A::mod(tab, r);
        const u64 pr = P.pr[r];
        const u64 *dr = dig + c * Lq * kn + (u64)r * n, *c0r = c0h + u * n;
        for (u32 s = blockIdx.x * blockDim.x + threadIdx.x; s < n; s += gridDim.x * blockDim.x) {
            u64 s0 = 0, s1 = 0;
            u32 since = 0;
            for (u32 j = 0; j < P.taps; j++) {
                const u64 *key = P.keys[j];
                u64 a0, a1;
                rot_tap_term<A>(dr, c0r, key ? key + (u64)r * n + s : nullptr, P.perm[(u64)j * n + s], r, Lq, kn, pr, m, a0, a1);
                const u64 w = P.P[((u64)j * k + r) * n + s];
                s0 = A::add(s0, A::mul(A::fold(a0, m), w, m), m);
                s1 = A::add(s1, A::mul(A::fold(a1, m), w, m), m);
                if (++since == ROT_FOLD_TERMS) {
                    s0 = A::fold(s0, m);
                    s1 = A::fold(s1, m);
                    since = 0;
                }
            }
            acc[((c * 2 + 0) * k + r) * n + s] = A::fold(s0, m);
            acc[((c * 2 + 1) * k + r) * n + s] = A::fold(s1, m);
        }
    }
}

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
    if (int rc = fhe_rot_forward(c, ct, stride, dig, c0h, count, st)) return rc;
    const dim3 g2 = ksp_grid2(n, count * k);
    if (!fhe_rot_pm(c)) k_rd_accum<ArBarrett><<<g2, 256, 0, st>>>(dig, c0h, P, acc, c->qb.d_mod, k, n, count);
    else if (c->qb.pm_class == 1) k_rd_accum<ArPm<PmA>><<<g2, 256, 0, st>>>(dig, c0h, P, acc, c->qb.dev(), k, n, count);
    else k_rd_accum<ArPm<PmB>><<<g2, 256, 0, st>>>(dig, c0h, P, acc, c->qb.dev(), k, n, count);
    KERNEL_CHECK();
    return fhe_rot_drop(c, acc, sp, out, out_stride, count * 2, st);
}

}  // namespace

int fhe_rot_forward(const fhe_ctx *c, const u64 *ct, u64 stride, u64 *dig, u64 *c0h, u64 count, hipStream_t st) {
    const u32 k = c->k, Lq = k - 1;
    if (fhe_rot_pm(c)) {
        const RnsBase base = c->qb.dev();
        const unsigned g1 = (unsigned)(count * (Lq * k + Lq));
        if (c->qb.pm_class == 1) { DISPATCH_L(c->logn, (k_rd_fwd_pm<L, PmA><<<g1, NttShape<L>::TP, 0, st>>>(ct, stride, dig, c0h, base))); }
        else { DISPATCH_L(c->logn, (k_rd_fwd_pm<L, PmB><<<g1, NttShape<L>::TP, 0, st>>>(ct, stride, dig, c0h, base))); }
        KERNEL_CHECK();
        return FHE_OK;
    }
    k_rd_stage_c0<<<ksp_grid2(c->n, count * k), 256, 0, st>>>(ct, stride, c0h, k, c->n, count);
    KERNEL_CHECK();
    if (int rc = fhe_qbase_ntt(false, c, c0h, c0h, count, st)) return rc;
    return fhe_ksp_forward(c, ct, stride, 1, dig, count, st);
}

int fhe_rot_drop(const fhe_ctx *c, u64 *acc, u64 *sp, u64 *out, u64 out_stride, u64 rows, hipStream_t st) {
    const u32 k = c->k, Lq = k - 1;
    const KspTab T = ksp_tab(c);
    if (fhe_rot_pm(c)) {
        const RnsBase base = c->qb.dev();
        const unsigned g4 = (unsigned)(rows * Lq);
        if (int rc = fhe_ksp_inv_sp(c, acc, sp, rows, st)) return rc;
        if (c->qb.pm_class == 1) { DISPATCH_L(c->logn, (k_rd_inv_down_pm<L, PmA><<<g4, NttShape<L>::TP, 0, st>>>(out, out_stride, acc, sp, base, T))); }
        else { DISPATCH_L(c->logn, (k_rd_inv_down_pm<L, PmB><<<g4, NttShape<L>::TP, 0, st>>>(out, out_stride, acc, sp, base, T))); }
        KERNEL_CHECK();
        return FHE_OK;
    }
    if (int rc = fhe_qbase_ntt(true, c, acc, acc, rows, st)) return rc;
    k_rd_down<<<ksp_grid2(c->n, rows * Lq), 256, 0, st>>>(out, out_stride, acc, T, k, c->n, rows);
    KERNEL_CHECK();
    return FHE_OK;
}

int fhe_rot_slot_exponents(const fhe_ctx *c, u64 *d, u32 rows, const char *what, std::vector<u32> &f) {
    const u32 n = c->n, k = c->k;
    const size_t row = (size_t)k * n;
    std::vector<uint64_t> x(row, 0);
    for (u32 r = 0; r < k; r++) x[(size_t)r * n + 1] = 1;
    if (hipMemcpy(d + rows * row, x.data(), row * 8, hipMemcpyHostToDevice) != hipSuccess) return fail(FHE_ERR_HIP, "upload of %s", what);
    if (int rc = fhe_qbase_ntt(false, c, d, d, rows + 1, nullptr)) return rc;
    if (hipStreamSynchronize(nullptr) != hipSuccess || hipMemcpy(x.data(), d + rows * row, row * 8, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(FHE_ERR_HIP, "transform of %s", what);
    // slot s of the transform of X holds psi_r^(e_s)
    std::vector<u32> fr;
    if (!rotsum::slot_exponents(x.data(), n, c->qb.primes[0], f)) return fail(FHE_ERR_PARAM, "the context's transform of X is not a set of odd powers of one root");
    for (u32 r = 1; r < k; r++)
        if (!rotsum::slot_exponents(x.data() + (size_t)r * n, n, c->qb.primes[r], fr) || fr != f)
            return fail(FHE_ERR_PARAM, "the context's transforms order their slots differently from prime to prime");
    return FHE_OK;
}

int fhe_rot_perm_keys(const std::vector<u32> &f, u32 count, const u32 *elts, const uint64_t *const *d_keys, u32 *perm, u64 *keys) {
    for (u32 j = 0; j < count; j++) {
        const u32 g = elts[j];
        if (!rotsum::slot_perm(f, g, perm + j * f.size())) return fail(FHE_ERR_PARAM, "no slot permutation for Galois element %u", g);
        keys[j] = g == 1 ? 0 : (u64)(uintptr_t)d_keys[j];
    }
    return FHE_OK;
}

extern "C" int fhe_rotdiag_plan_create(const fhe_ctx *c, uint32_t taps, const uint32_t *elts, const uint64_t *plains, const uint64_t *const *d_keys,
                                       fhe_rotdiag_plan **out) {
    if (!c || !out || !elts || !plains || !d_keys) return fail(FHE_ERR_PARAM, "null argument");
    const u32 n = c->n, k = c->k;
    const std::vector<uint64_t> ones(taps && taps <= rotsum::MAX_TAPS ? taps : 0, 1);      // the weights' check is the plaintexts', below
    std::string why = rotsum::check_taps(n, c->t, k, taps, elts, ones.data(), (const void *const *)d_keys);
    if (why.empty()) why = rotdiag::check_plains(n, c->t, taps, plains);
    if (!why.empty()) return fail(FHE_ERR_PARAM, "%s", why.c_str());
    // rows 0 .. taps - 1 of the block: the centred lifts, transformed with the row of X behind them (fhe_rot_slot_exponents); the block is sized
    // for that, and the permutations and the keys then take the place of the row of X and what follows
    const size_t row = (size_t)k * n, b_P = (size_t)taps * row * 8, b_perm = (((size_t)taps * n * 4) + 7) & ~(size_t)7, b_keys = (size_t)taps * 8;
    std::vector<uint64_t> h(taps * row, 0);
    const std::vector<uint64_t> primes(c->qb.primes.begin(), c->qb.primes.end());
    for (u32 j = 0; j < taps; j++) rotdiag::lift(plains + (size_t)j * n, n, c->t, primes.data(), k, h.data() + j * row);
    std::unique_ptr<fhe_rotdiag_plan> p(new fhe_rotdiag_plan);
    p->ctx = c;
    p->taps = taps;
    p->elts.assign(elts, elts + taps);
    const size_t bytes = b_P + (row * 8 > b_perm + b_keys ? row * 8 : b_perm + b_keys);
    if (hipMalloc(&p->d_block, bytes) != hipSuccess) {
        p->d_block = nullptr;
        return fail(FHE_ERR_NOMEM, "device allocation of %zu bytes for the rotate-diag plan", bytes);
    }
    u64 *d = (u64 *)p->d_block;
    if (hipMemcpy(d, h.data(), b_P, hipMemcpyHostToDevice) != hipSuccess) return fail(FHE_ERR_HIP, "upload of the plaintexts");
    std::vector<u32> f;
    if (int rc = fhe_rot_slot_exponents(c, d, taps, "the plaintexts", f)) return rc;
    std::vector<unsigned char> tail(b_perm + b_keys, 0);
    if (int rc = fhe_rot_perm_keys(f, taps, elts, d_keys, (u32 *)tail.data(), (u64 *)(tail.data() + b_perm))) return rc;
    if (hipMemcpy((unsigned char *)p->d_block + b_P, tail.data(), tail.size(), hipMemcpyHostToDevice) != hipSuccess)
        return fail(FHE_ERR_HIP, "upload of the rotate-diag plan");
    p->d_P = d;
    p->d_perm = (u32 *)((unsigned char *)p->d_block + b_P);
    p->d_keys = (const u64 **)((unsigned char *)p->d_block + b_P + b_perm);
    *out = p.release();
    return FHE_OK;
}

extern "C" int fhe_rotdiag_plan_destroy(fhe_rotdiag_plan *p) {
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
    const fhe_ctx *c = p->ctx;
    const std::string why = rotsum::check_call(c->k, c->n, ct2, stride, out2, out_stride, count, count * c->k * c->k, scratch_words(p, count) * sizeof(u64), scratch, scratch_bytes);
    if (!why.empty()) return fail(FHE_ERR_PARAM, "%s", why.c_str());
    if (!count) return FHE_OK;
    return run(p, (const u64 *)ct2, stride, (u64 *)out2, out_stride, count, (u64 *)scratch, (hipStream_t)s);
}
