// idct.hip -- the way back from the JPEG path: dequantisation + 8x8 inverse DCT (fhe_idct8x8_dequant) and the JFIF
// YCbCr -> RGB step (fhe_ycc_to_rgb_blocks), the inverses of fhe_dct8x8_quant and fhe_rgb_to_ycc_blocks.
//
// Per block of 64 size-2 ciphertexts (include/fhe_hip.h states the op-by-op specification):
//   c[i] *= encode(Q[i]);  idct_line on every row, then on every column;  c[i] *= encode(0.125)
// idct_line is the transpose of the forward LL&M line: IJG's jidctint dataflow on the same twelve constants (kDctConst).
// Every step is an exact operation in R_q, so the plan folds the two per-ciphertext products into one input product
// encode(Q[i]) * encode(0.125) (fhe_plain_ntt_mul: the same ring element, not encode(Q[i] / 8)) and the kernels transform
// each input polynomial once, evaluate the whole linear circuit per NTT slot and transform back: the ciphertexts are
// bit-identical to the op-at-a-time evaluation.
//
// Where fhe_dct_path(ctx) == 1 (primes < 2^47, n <= 8192) the fused exact-FP64 pair k_idct_rows + k_idct_cols runs
// (dct_fused.hip); every other context, and FHE_DCT_FORCE_U64=1, takes the general path: k_ntt_fwd, the slot kernels
// below, k_ntt_inv (as fhe_dct8x8_quant's general path).
#include "internal.h"

#include "host_math.h"

#include <vector>

struct fhe_idct_plan {
    ulonglong2 *d_consts = nullptr;   // [DCT_NCONST][k][n] Shoup pairs, slot order: cid 0..11 kDctConst, 12 + i the input scale of ciphertext i
    double *d_consts_f64 = nullptr;   // the same as centred doubles in the fused FP64 kernels' order, or null
    u32 k = 0, n = 0;
    bool has_quant = false;
};

namespace {

// One 1-D inverse line on eight fully reduced residues (jidctint: even part from d0 d2 d4 d6, odd part from d1 d3 d5 d7,
// butterfly on the output side).  C(cid) yields the Shoup pair of constant cid at this thread's slot.
template <typename CF>
__device__ __forceinline__ void idct_line_u64(u64 (&d)[8], const u64 q, CF C) {
    auto MUL = [&](u64 x, int cid) { const ulonglong2 w = C(cid); return mul_shoup(x, w.x, w.y, q); };
    u64 z1 = MUL(addmod(d[2], d[6], q), 0);
    const u64 t2 = addmod(z1, MUL(d[6], 2), q), t3 = addmod(z1, MUL(d[2], 1), q);
    const u64 t0 = addmod(d[0], d[4], q), t1 = submod(d[0], d[4], q);
    const u64 t10 = addmod(t0, t3, q), t13 = submod(t0, t3, q), t11 = addmod(t1, t2, q), t12 = submod(t1, t2, q);
    u64 u0 = d[7], u1 = d[5], u2 = d[3], u3 = d[1];
    z1 = addmod(u0, u3, q);
    u64 z2 = addmod(u1, u2, q), z3 = addmod(u0, u2, q), z4 = addmod(u1, u3, q);
    const u64 z5 = MUL(addmod(z3, z4, q), 3);
    u0 = MUL(u0, 4);
    u1 = MUL(u1, 5);
    u2 = MUL(u2, 6);
    u3 = MUL(u3, 7);
    z1 = MUL(z1, 8);
    z2 = MUL(z2, 9);
    z3 = addmod(MUL(z3, 10), z5, q);
    z4 = addmod(MUL(z4, 11), z5, q);
    u0 = addmod(u0, addmod(z1, z3, q), q);
    u1 = addmod(u1, addmod(z2, z4, q), q);
    u2 = addmod(u2, addmod(z2, z3, q), q);
    u3 = addmod(u3, addmod(z1, z4, q), q);
    d[0] = addmod(t10, u3, q);
    d[7] = submod(t10, u3, q);
    d[1] = addmod(t11, u2, q);
    d[6] = submod(t11, u2, q);
    d[2] = addmod(t12, u1, q);
    d[5] = submod(t12, u1, q);
    d[3] = addmod(t13, u0, q);
    d[4] = submod(t13, u0, q);
}

// Slot kernel (Shoup / Harvey bases, FHE_NTT_NOPM=1): one thread owns one NTT slot of one (block, poly, prime) unit:
// 64 values in, input scale, row pass, column pass, 64 values out (in place).
__global__ __launch_bounds__(256) void k_idct_slots(u64 *__restrict__ data, const ulonglong2 *__restrict__ consts,
                                                    const Modulus *__restrict__ mods, u32 k, u32 n) {
    const u32 unit = blockIdx.y;             // (block * 2 + poly) * k + prime
    const u32 prime = unit % k;
    const u32 bp = unit / k;
    const u32 blk = bp >> 1, poly = bp & 1;
    const u32 slot = blockIdx.x * blockDim.x + threadIdx.x;
    const u64 q = mods[prime].q;
    const size_t ct_stride = (size_t)2 * k * n;
    u64 *p = data + (size_t)blk * 64 * ct_stride + ((size_t)poly * k + prime) * n + slot;
    const ulonglong2 *cp = consts + (size_t)prime * n + slot;
    const size_t cstride = (size_t)k * n;
    auto C = [&](int cid) { return cp[(size_t)cid * cstride]; };
    u64 v[8][8];
#pragma unroll
    for (int i = 0; i < 64; i++) {
        const ulonglong2 w = C(12 + i);
        v[i >> 3][i & 7] = mul_shoup(p[(size_t)i * ct_stride], w.x, w.y, q);
    }
#pragma unroll
    for (int r = 0; r < 8; r++) idct_line_u64(v[r], q, C);
#pragma unroll
    for (int col = 0; col < 8; col++) {
        u64 l[8];
#pragma unroll
        for (int i = 0; i < 8; i++) l[i] = v[i][col];
        idct_line_u64(l, q, C);
#pragma unroll
        for (int i = 0; i < 8; i++) v[i][col] = l[i];
    }
#pragma unroll
    for (int i = 0; i < 64; i++) p[(size_t)i * ct_stride] = v[i >> 3][i & 7];
}

// Pseudo-Mersenne bases (class PmA, every prime <= 55 bits) take the slot step as two launches of 8 values per thread, on
// lazy arithmetic as k_dct_lines_pm: sums stay unreduced, a difference a - b gets a power-of-two multiple of q at or above
// b's bound added, every product is mulvv_pm(fold_pm(x), c) -- any 64-bit x in, below 6 q out.
//
// Bounds in units of q, for inputs below I q (IP = the power of two at or above I):
//   even part   d2 + d6 < 2I, z1 < 6;  t2, t3 < 12;  t0 < 2I, t1 < I + IP
//               t10 < 2I + 12, t13 < 2I + 16, t11 < I + IP + 12, t12 < I + IP + 16
//   odd part    z3 + z4 < 4I (the largest product operand);  every product < 6;  z3, z4 < 12;  u0 .. u3 < 6 + 6 + 12 = 24
//   outputs     sums < I + IP + 40, differences (+ 32 q) < I + IP + 48 = idct_pm_out(I)
// Rows: the input scale brings the canonical inputs below 6 q, so I = 6 and row outputs are below 62 q (stored as they
// are); columns: I = 62, the largest value met is 4 I = 248 q, the outputs are below 174 q.  256 q < 2^63 for q < 2^55.
__host__ __device__ constexpr int idct_pow2_at_least(int v) { int p = 1; while (p < v) p <<= 1; return p; }
__host__ __device__ constexpr int idct_pm_out(int I) { return I + idct_pow2_at_least(I) + 48; }
constexpr int IDCT_PM_PROD = 6;                                   // mulvv_pm's result bound for class PmA (ntt_core.h)
constexpr int IDCT_PM_ROW_OUT = idct_pm_out(IDCT_PM_PROD);        // 62
template <int I, typename CF>
__device__ __forceinline__ void idct_line_pm(u64 (&d)[8], const PmMod &m, CF C) {
    constexpr int IP = idct_pow2_at_least(I);
    static_assert(4 * I <= 256 && 2 * I + 48 <= 256 && idct_pm_out(I) <= 256, "a sum would pass 256 q");
    const u64 oi = m.q * IP, o16 = m.q * 16, o32 = m.q * 32;
    auto MUL = [&](u64 x, int cid) { return mulvv_pm(fold_pm(x, m), C(cid).x, m); };
    u64 z1 = MUL(d[2] + d[6], 0);
    const u64 t2 = z1 + MUL(d[6], 2), t3 = z1 + MUL(d[2], 1);
    const u64 t0 = d[0] + d[4], t1 = d[0] - d[4] + oi;
    const u64 t10 = t0 + t3, t13 = t0 - t3 + o16, t11 = t1 + t2, t12 = t1 - t2 + o16;
    u64 u0 = d[7], u1 = d[5], u2 = d[3], u3 = d[1];
    z1 = u0 + u3;
    u64 z2 = u1 + u2, z3 = u0 + u2, z4 = u1 + u3;
    const u64 z5 = MUL(z3 + z4, 3);
    u0 = MUL(u0, 4);
    u1 = MUL(u1, 5);
    u2 = MUL(u2, 6);
    u3 = MUL(u3, 7);
    z1 = MUL(z1, 8);
    z2 = MUL(z2, 9);
    z3 = MUL(z3, 10) + z5;
    z4 = MUL(z4, 11) + z5;
    u0 = u0 + z1 + z3;
    u1 = u1 + z2 + z4;
    u2 = u2 + z2 + z3;
    u3 = u3 + z1 + z4;
    d[0] = t10 + u3;
    d[7] = t10 - u3 + o32;
    d[1] = t11 + u2;
    d[6] = t11 - u2 + o32;
    d[2] = t12 + u1;
    d[5] = t12 - u1 + o32;
    d[3] = t13 + u0;
    d[4] = t13 - u0 + o32;
}
// COLS = false: line `l` = row l of the block (ciphertexts 8 l .. 8 l + 7), input scale first; true: column l (ciphertexts
// l, l + 8, ...), canonical residues out
template <bool COLS>
__global__ __launch_bounds__(256) void k_idct_lines_pm(u64 *__restrict__ data, const ulonglong2 *__restrict__ consts,
                                                       const PmMod *__restrict__ pm, u32 k, u32 n) {
    const u32 line = blockIdx.y & 7, unit = blockIdx.y >> 3;      // unit = (block * 2 + poly) * k + prime
    const u32 prime = unit % k;
    const u32 bp = unit / k;
    const u32 blk = bp >> 1, poly = bp & 1;
    const u32 slot = blockIdx.x * blockDim.x + threadIdx.x;
    const PmMod m = pm[prime];
    const size_t ct_stride = (size_t)2 * k * n, step = COLS ? 8 * ct_stride : ct_stride;
    u64 *p = data + ((size_t)blk * 64 + (COLS ? line : 8 * line)) * ct_stride + ((size_t)poly * k + prime) * n + slot;
    const ulonglong2 *cp = consts + (size_t)prime * n + slot;
    const size_t cstride = (size_t)k * n;
    auto C = [&](int cid) { return cp[(size_t)cid * cstride]; };
    u64 v[8];
    if constexpr (!COLS) {
#pragma unroll
        for (int i = 0; i < 8; i++) v[i] = mulvv_pm(fold_pm(p[(size_t)i * step], m), C(12 + 8 * line + i).x, m);
        idct_line_pm<IDCT_PM_PROD>(v, m, C);
#pragma unroll
        for (int i = 0; i < 8; i++) p[(size_t)i * step] = v[i];
    } else {
#pragma unroll
        for (int i = 0; i < 8; i++) v[i] = p[(size_t)i * step];
        idct_line_pm<IDCT_PM_ROW_OUT>(v, m, C);
#pragma unroll
        for (int i = 0; i < 8; i++) p[(size_t)i * step] = canon_pm(v[i], m);    // fold_pm takes any 64-bit value and returns one below 17/16 q
    }
}

// ------------------------------------------------------------------------------------------------
// JFIF YCbCr -> RGB (the inverse of rgb_to_ycc_fhe), one launch per call, every context
// ------------------------------------------------------------------------------------------------
// Y is never multiplied: R = Y' + Cr 1.402, G = Y' - Cb .344136 - Cr .714136, B = Y' + Cb 1.772 with Y' = Y + Delta encode(128).
// The kernel transforms Cb and Cr, forms the three products per slot, transforms them back and adds Y and the precomputed
// Delta encode(128) (on polynomial 0): exact in R_q, so the same bits as the op-by-op sequence.
// consts: [4][k][n] Shoup pairs (1.402, .344136, .714136, 1.772); y_off: [k][len] = Delta * encode(128.0) lifted.
template <int L>
__global__ __launch_bounds__(NttShape<L>::TP) void k_ycc2rgb(u64 *__restrict__ Y, u64 *__restrict__ Cb, u64 *__restrict__ Cr,
                                                              const ulonglong2 *__restrict__ consts, const u64 *__restrict__ yoff, u32 yoff_len,
                                                              RnsBase base, u32 group, u64 gstride) {
    __shared__ u64 lds[NttShape<L>::LDS_WORDS];
    constexpr int N = NttShape<L>::N, TP = NttShape<L>::TP;
    const int tid = threadIdx.x;
    const u64 rp0 = blockIdx.x;                // (pixel * 2 + poly) * k + prime
    const u32 prime = (u32)(rp0 % base.count);
    const u32 poly = (u32)((rp0 / base.count) & 1);
    const u64 pix = rp0 / (2 * base.count);
    const u64 rp = ((pix / group) * gstride + (pix % group) * 2 * base.count * N) / N + (u64)poly * base.count + prime;
    const u64 q = base.mod[prime].q;
    const ulonglong2 *tw = base.tw + (size_t)prime * N, *itw = base.itw + (size_t)prime * N;
    const size_t cstride = (size_t)base.count * N;
    const ulonglong2 *cp = consts + (size_t)prime * N;
    u64 cb[16], cr[16];
    load_coeff<L>(cb, Cb + rp * N, tid);
    ntt_fwd_regs<L>(cb, tw, q, lds, tid);
    load_coeff<L>(cr, Cr + rp * N, tid);
    ntt_fwd_regs<L>(cr, tw, q, lds, tid);
    u64 r[16], g[16], b[16];
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const int pos = i * TP + tid;
        auto M = [&](u64 x, int cid) { const ulonglong2 w = cp[cid * cstride + pos]; return mul_shoup(x, w.x, w.y, q); };
        r[i] = M(cr[i], 0);
        g[i] = submod(submod(0, M(cb[i], 1), q), M(cr[i], 2), q);
        b[i] = M(cb[i], 3);
    }
    ntt_inv_regs<L>(r, itw, q, lds, tid);
    ntt_lds_release();                         // the inverse transform's last transpose reads across waves (ntt_core.h, CONTRACT)
    ntt_inv_regs<L>(g, itw, q, lds, tid);
    ntt_lds_release();
    ntt_inv_regs<L>(b, itw, q, lds, tid);
    u64 y[16];
    load_coeff<L>(y, Y + rp * N, tid);
#pragma unroll
    for (int i = 0; i < 16; i++) {
        u64 yy = y[i];
        if (poly == 0) {
            const int j = elem_index<L - 4>(tid, i);
            if ((u32)j < yoff_len) yy = addmod(yy, yoff[(size_t)prime * yoff_len + j], q);
        }
        r[i] = addmod(yy, csub(r[i], q), q);
        g[i] = addmod(yy, csub(g[i], q), q);
        b[i] = addmod(yy, csub(b[i], q), q);
    }
    store_coeff<L>(r, Y + rp * N, tid);
    store_coeff<L>(g, Cb + rp * N, tid);
    store_coeff<L>(b, Cr + rp * N, tid);
}

static int prep_plain(const fhe_ctx *c, double v, int int_coeffs, int frac_coeffs, std::vector<uint64_t> &plain, ulonglong2 *dst, fhe_stream s) {
    const int len = fhe_frac_encode(c->n, c->t, v, int_coeffs, frac_coeffs, plain.data());
    if (len < 0) return len;
    return fhe_plain_prepare(c, plain.data(), (uint32_t)len, (uint64_t *)dst, s);
}

}  // namespace

// Encode, lift and transform the four factors and Delta encode(128) once per context and (int_coeffs, frac_coeffs) pair
// (synchronous, first call only); kept until the context is destroyed, as the rgb_to_ycc constants.
static int ycc_consts(const fhe_ctx *c, int int_coeffs, int frac_coeffs, hipStream_t st, const fhe_ctx::RgbConsts **out) {
    using namespace hostmath;
    std::lock_guard<std::mutex> lock(c->rgb_mutex);
    for (const fhe_ctx::RgbConsts *r : c->ycc)
        if (r->int_coeffs == int_coeffs && r->frac_coeffs == frac_coeffs) { *out = r; return FHE_OK; }
    static const double cc[4] = {1.402, 0.344136, 0.714136, 1.772};
    const size_t pw = (size_t)c->k * c->n;
    std::vector<uint64_t> plain(c->n);
    fhe_ctx::RgbConsts t;
    auto drop = [&](int code) { if (t.d_c) (void)hipFree(t.d_c); if (t.d_off) (void)hipFree(t.d_off); return code; };
    int rc = fhe_dev_alloc(sizeof(ulonglong2) * pw * 4, (void **)&t.d_c);
    if (rc) return rc;
    for (int i = 0; i < 4; ++i)
        if ((rc = prep_plain(c, cc[i], int_coeffs, frac_coeffs, plain, t.d_c + pw * i, st))) return drop(rc);
    int len = fhe_frac_encode(c->n, c->t, 128.0, int_coeffs, frac_coeffs, plain.data());
    if (len < 0) return drop(len);
    std::vector<u64> off((size_t)c->k * len);
    for (u32 i = 0; i < c->k; ++i)
        for (int j = 0; j < len; ++j) {
            const u64 qi = c->qb.primes[i], m = plain[j];
            u64 v = mulmod(c->delta_mod[i], m % qi, qi);
            if (m >= c->upper_half_threshold) v = addmod(v, c->upper_half_increment[i], qi);
            off[(size_t)i * len + j] = v;
        }
    if ((rc = fhe_dev_alloc(off.size() * sizeof(u64) + 8, (void **)&t.d_off))) return drop(rc);
    if (hipMemcpy(t.d_off, off.data(), off.size() * sizeof(u64), hipMemcpyHostToDevice) != hipSuccess) return drop(fail(FHE_ERR_HIP, "upload failed"));
    t.off_len = (u32)len;
    if (hipStreamSynchronize(st) != hipSuccess) return drop(fail(FHE_ERR_HIP, "stream sync failed"));
    t.int_coeffs = int_coeffs;
    t.frac_coeffs = frac_coeffs;
    c->ycc.push_back(new fhe_ctx::RgbConsts(t));
    *out = c->ycc.back();
    return FHE_OK;
}

extern "C" int fhe_ycc_to_rgb_blocks(const fhe_ctx *c, uint64_t *blocks, uint64_t n_blocks, int int_coeffs, int frac_coeffs, fhe_stream s) {
    if (!c || !blocks) return fail(FHE_ERR_PARAM, "null argument");
    if (!n_blocks) return FHE_OK;
    hipStream_t st = (hipStream_t)s;
    const fhe_ctx::RgbConsts *k4 = nullptr;
    int rc = ycc_consts(c, int_coeffs, frac_coeffs, st, &k4);
    if (rc) return rc;
    const u64 plane = (u64)64 * 2 * c->k * c->n;           // words of one channel of one block
    const u64 nrp = n_blocks * 64 * 2 * c->k;
    if (nrp > 0x7fffffffULL) return fail(FHE_ERR_PARAM, "too many blocks for one launch");
    u64 *y = (u64 *)blocks;
    const RnsBase base = c->qb.dev();
    DISPATCH_L(c->logn, (k_ycc2rgb<L><<<(unsigned)nrp, NttShape<L>::TP, 0, st>>>(y, y + plane, y + 2 * plane, k4->d_c, k4->d_off, k4->off_len,
                                                                                 base, 64, 3 * plane)));
    KERNEL_CHECK();
    return FHE_OK;
}

// ------------------------------------------------------------------------------------------------
// plan + entry point
// ------------------------------------------------------------------------------------------------
extern "C" int fhe_idct_plan_create(const fhe_ctx *c, const double *quant64, int int_coeffs, int frac_coeffs, fhe_stream s, fhe_idct_plan **out) {
    if (!c || !out) return fail(FHE_ERR_PARAM, "null argument");
    *out = nullptr;
    if (quant64)
        for (int i = 0; i < 64; ++i)
            if (!(quant64[i] != 0.0)) return fail(FHE_ERR_PARAM, "quant[%d] is zero", i);
    fhe_idct_plan *p = new fhe_idct_plan();
    p->k = c->k;
    p->n = c->n;
    p->has_quant = quant64 != nullptr;
    const size_t pw = (size_t)c->k * c->n;   // pairs per constant
    int rc = fhe_dev_alloc(sizeof(ulonglong2) * pw * DCT_NCONST, (void **)&p->d_consts);
    if (rc) { delete p; return rc; }
    std::vector<uint64_t> plain(c->n);
    ulonglong2 *d_eighth = nullptr, *d_tmp = nullptr;
    auto cleanup = [&](int code) {
        if (d_eighth) (void)hipFree(d_eighth);
        if (d_tmp) (void)hipFree(d_tmp);
        if (code) { (void)hipFree(p->d_consts); if (p->d_consts_f64) (void)hipFree(p->d_consts_f64); delete p; }
        return code;
    };
    for (int i = 0; i < 12; ++i)
        if ((rc = prep_plain(c, kDctConst[i], int_coeffs, frac_coeffs, plain, p->d_consts + pw * i, s))) return cleanup(rc);
    if (!quant64) {
        for (int i = 0; i < 64; ++i)
            if ((rc = prep_plain(c, 0.125, int_coeffs, frac_coeffs, plain, p->d_consts + pw * (12 + i), s))) return cleanup(rc);
    } else {
        // dequantisation and the final scale as one product: encode(Q[i]) * encode(0.125), the ring product of the two lifted plaintexts
        if ((rc = fhe_dev_alloc(sizeof(ulonglong2) * pw, (void **)&d_eighth))) return cleanup(rc);
        if ((rc = fhe_dev_alloc(sizeof(ulonglong2) * pw, (void **)&d_tmp))) return cleanup(rc);
        if ((rc = prep_plain(c, 0.125, int_coeffs, frac_coeffs, plain, d_eighth, s))) return cleanup(rc);
        for (int i = 0; i < 64; ++i) {
            if ((rc = prep_plain(c, quant64[i], int_coeffs, frac_coeffs, plain, d_tmp, s))) return cleanup(rc);
            if ((rc = fhe_plain_ntt_mul(c, (const uint64_t *)d_eighth, (const uint64_t *)d_tmp, (uint64_t *)(p->d_consts + pw * (12 + i)), s)))
                return cleanup(rc);
        }
    }
    if (fhe_dct_f64_supported(c) && (rc = fhe_idct_f64_make_consts(c, p->d_consts, &p->d_consts_f64, (hipStream_t)s))) return cleanup(rc);
    if (hipStreamSynchronize((hipStream_t)s) != hipSuccess) return cleanup(fail(FHE_ERR_HIP, "stream sync failed"));
    *out = p;
    return cleanup(FHE_OK);
}
extern "C" int fhe_idct_plan_destroy(fhe_idct_plan *p) {
    if (!p) return FHE_OK;
    if (p->d_consts) (void)hipFree(p->d_consts);
    if (p->d_consts_f64) (void)hipFree(p->d_consts_f64);
    delete p;
    return FHE_OK;
}
// The fused pair keeps one row-transformed copy of a wave of blocks (FP64, as fhe_dct8x8_scratch_bytes); the general path works
// in place on `out` and needs none.
extern "C" size_t fhe_idct8x8_scratch_bytes(const fhe_ctx *c, uint64_t n_blocks) {
    if (!c || !fhe_dct_f64_supported(c)) return 0;
    const u64 wave = c->opt.dct_wave_blocks < n_blocks ? c->opt.dct_wave_blocks : n_blocks;
    return (size_t)wave * 64 * 2 * c->k * c->n * sizeof(double);
}

extern "C" int fhe_idct8x8_dequant(const fhe_ctx *c, const fhe_idct_plan *plan, const uint64_t *in, uint64_t *out, uint64_t n_blocks,
                                   void *scratch, size_t scratch_bytes, fhe_stream s) {
    if (!c || !plan || !in || !out) return fail(FHE_ERR_PARAM, "null argument");
    if (plan->k != c->k || plan->n != c->n) return fail(FHE_ERR_PARAM, "plan was built for another context");
    if (n_blocks == 0) return FHE_OK;
    hipStream_t st = (hipStream_t)s;
    if (plan->d_consts_f64 && fhe_dct_f64_supported(c) && !c->opt.force_u64) {
        const size_t per_block = (size_t)64 * 2 * c->k * c->n;
        const u64 fit = scratch ? scratch_bytes / (per_block * sizeof(double)) : 0;
        if (fit == 0) return fail(FHE_ERR_PARAM, "scratch too small: need fhe_idct8x8_scratch_bytes()");
        const u64 wave = fit < c->opt.dct_wave_blocks ? fit : c->opt.dct_wave_blocks;
        for (u64 b0 = 0; b0 < n_blocks; b0 += wave) {
            const u64 nb = (n_blocks - b0) < wave ? (n_blocks - b0) : wave;
            int rc = fhe_idct_f64_launch(c, plan->d_consts_f64, (const u64 *)in + b0 * per_block, (u64 *)out + b0 * per_block, nb, (double *)scratch, st);
            if (rc) return rc;
        }
        return FHE_OK;
    }
    const u64 polys_per_block = 64 * 2;   // RNS polynomials (of k residues) per block
    const u64 max_blocks = 4096;
    for (u64 b0 = 0; b0 < n_blocks; b0 += max_blocks) {
        const u64 nb = (n_blocks - b0) < max_blocks ? (n_blocks - b0) : max_blocks;
        const size_t off = (size_t)b0 * polys_per_block * c->k * c->n;
        int rc = fhe_ntt_launch(false, c, c->qb, (const u64 *)in + off, (u64 *)out + off, nb * polys_per_block * c->k, st);
        if (rc) return rc;
        if (c->qb.pm_class == 1 && !c->opt.ntt_nopm) {
            dim3 grid8(c->n / 256, (unsigned)(nb * 2 * c->k * 8));
            k_idct_lines_pm<false><<<grid8, 256, 0, st>>>((u64 *)out + off, plan->d_consts, c->qb.d_pm, c->k, c->n);
            k_idct_lines_pm<true><<<grid8, 256, 0, st>>>((u64 *)out + off, plan->d_consts, c->qb.d_pm, c->k, c->n);
        } else {
            dim3 grid(c->n / 256, (unsigned)(nb * 2 * c->k));
            k_idct_slots<<<grid, 256, 0, st>>>((u64 *)out + off, plan->d_consts, c->qb.d_mod, c->k, c->n);
        }
        KERNEL_CHECK();
        rc = fhe_ntt_launch(true, c, c->qb, (const u64 *)out + off, (u64 *)out + off, nb * polys_per_block * c->k, st);
        if (rc) return rc;
    }
    return FHE_OK;
}
