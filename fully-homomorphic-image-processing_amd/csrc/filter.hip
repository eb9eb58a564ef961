// filter.hip -- encrypted 2-D convolution with a public kernel (fhe_filter2d): per output ciphertext
//     out = sum over the kernel positions p with encode(w[p]) != 0 of multiply_plain(src[tap[p]], encode(w[p]))
// (include/fhe_hip.h states the op-by-op specification).  multiply_plain is linear and everything is exact arithmetic mod q, so
//     INTT( sum_p NTT(src[tap[p]]) . NTT(lift(encode(w[p]))) )
// is the same ring element and therefore the same canonical residues: every source polynomial is transformed ONCE however many
// outputs read it, every output polynomial is transformed back ONCE however many taps it has, and the taps that share a weight
// are summed before they are multiplied (a box filter costs one product per slot, Gauss 3x3 three).
//
// Launches per call:
//   1. fhe_ntt_forward over all n_src * size polynomials into scratch (skipped with src_is_ntt);
//   2. pseudo-Mersenne bases (fhe_filter_path 1 / 2): k_filter_acc_inv_pm, one workgroup per output residue polynomial -- gather of the
//      taps' slot vectors, lazy sums, one product per distinct weight, inverse transform in the same kernel, canonical store.  No
//      NTT-form accumulator goes through HBM;
//      every other base (fhe_filter_path 0 / 4): k_filter_mac (canonical Shoup arithmetic, one thread per slot) into `out`, then
//      fhe_ntt_inverse in place.
// The tap table travels through the staging ring in chunks of FHE_STAGE_SLOT_BYTES / (4 * non-zero taps) outputs (1024 .. 4096).
#include "internal.h"

#include "host_math.h"

#include <vector>

struct fhe_filter_plan {
    u32 k = 0, n = 0, kw = 0, kh = 0;
    u32 nt = 0, nd = 0;               // non-zero taps, distinct non-zero weights
    u32 pos[FHE_FILTER_MAX_TAPS];     // kernel position (row-major) of sorted tap i; sorted by weight id, then by position
    ulonglong2 *d_w = nullptr;        // [nd][k][n] Shoup pairs, slot order (fhe_plain_prepare)
    u64 *d_wx = nullptr;              // [nd][k][n] the values alone (the pseudo-Mersenne kernel needs no companion)
    u32 *d_wid = nullptr;             // [nt] weight id of sorted tap i, non-decreasing
};

namespace {

__global__ void k_pairs_first(const ulonglong2 *__restrict__ in, u64 *__restrict__ out, u64 count) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) out[i] = in[i].x;
}

// Workgroup -> (prime, output, poly).  `prime` is the slowest index: every workgroup in flight reads the same few weight vectors,
// and neighbouring workgroups are neighbouring outputs of one residue, whose taps overlap (a 3x3 window shares six of its nine
// source polynomials with the next one).  Workgroups are handed to the eight XCDs round robin; with `xcd_span` != 0 workgroup b
// works on item (b % 8) * xcd_span + b / 8, so that each XCD -- each L2 -- walks its own contiguous run of outputs instead of
// every eighth one (items at or beyond `total` do nothing).
struct FilterItem { u32 prime, poly; u64 o; bool live; };
__device__ __forceinline__ FilterItem filter_item(u64 b, u64 total, u64 xcd_span, u32 size, u64 cnt) {
    const u64 it = xcd_span ? (b & 7) * xcd_span + (b >> 3) : b;
    FilterItem r;
    r.live = it < total && (!xcd_span || (b >> 3) < xcd_span);
    const u64 per_prime = cnt * size;
    r.prime = (u32)(it / per_prime);
    const u64 rem = it % per_prime;
    r.o = rem / size;
    r.poly = (u32)(rem % size);
    return r;
}

// Lazy sums, in units of q (q < 2^58 for class PmB, < 2^55 for class PmA; fold_pm takes ANY 64-bit value to below 17/16 q):
//   s  sum of the source slots of one weight.  Sources are canonical (< q; what fhe_ntt_forward writes).  s is folded after every
//      FILTER_SUM_FOLD = 16 summands: s < 17/16 + 16 < 18 q < 2^63.
//   y  sum of the products mulvv_pm(fold_pm(s), w) < RQ (6 q class A, 1.5 q class B).  y is folded after every FILTER_PROD_FOLD = 8
//      products, as k_sum_inv_pm does: y < 17/16 + 8 RQ <= 49.1 q < 2^61 (class A), 13.1 q < 2^62 (class B).
// Both counters are compile-time constants, so the bounds hold for every kernel up to FHE_FILTER_MAX_TAPS taps and any weights; the
// largest summands (every slot q - 1, 49 and 64 equal weights, 64 taps) are a GPU test (tests/test_gpu_filter.py).
constexpr u32 FILTER_SUM_FOLD = 16, FILTER_PROD_FOLD = 8;
constexpr u64 FILTER_CHUNK_MAX = 4096;

template <int L, typename C>
__global__ __launch_bounds__(NttShape<L>::TP, 4) void k_filter_acc_inv_pm(const u64 *__restrict__ src, const u32 *__restrict__ taps,
                                                                          const u64 *__restrict__ wx, const u32 *__restrict__ wid, u32 nt,
                                                                          u64 *__restrict__ out, u32 size, u64 cnt, u64 total, u64 xcd_span,
                                                                          RnsBase base) {
    __shared__ u64 lds[NttShape<L>::LDS_WORDS];
    constexpr int N = NttShape<L>::N, TP = NttShape<L>::TP;
    const int tid = threadIdx.x;
    const FilterItem it = filter_item(blockIdx.x, total, xcd_span, size, cnt);
    if (!it.live) return;                                   // uniform over the workgroup
    const PmMod m = base.pm[it.prime];
    const u32 *tp = taps + it.o * nt;
    const u64 *wp = wx + (size_t)it.prime * N;
    const size_t wstride = (size_t)base.count * N;
    u64 y[1][16], s[16];
#pragma unroll
    for (int r = 0; r < 16; r++) { y[0][r] = 0; s[r] = 0; }
    u32 cur = wid[0], nsum = 0, nprod = 0;
    auto flush = [&]() {
        if (nprod == FILTER_PROD_FOLD) {
            nprod = 0;
#pragma unroll
            for (int r = 0; r < 16; r++) y[0][r] = fold_pm(y[0][r], m);
        }
        const u64 *w = wp + cur * wstride;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            y[0][r] += mulvv_pm(fold_pm(s[r], m), w[r * TP + tid], m);
            s[r] = 0;
        }
        nprod++;
        nsum = 0;
    };
    for (u32 i = 0; i < nt; i++) {
        const u32 w = wid[i];
        if (w != cur) { flush(); cur = w; }
        u64 x[16];
        load_slots<L>(x, src + (((size_t)tp[i] * size + it.poly) * base.count + it.prime) * N, tid);
        if (nsum == FILTER_SUM_FOLD) {
            nsum = 0;
#pragma unroll
            for (int r = 0; r < 16; r++) s[r] = fold_pm(s[r], m);
        }
#pragma unroll
        for (int r = 0; r < 16; r++) s[r] += x[r];
        nsum++;
    }
    flush();
#pragma unroll
    for (int r = 0; r < 16; r++) y[0][r] = fold_pm(y[0][r], m);
    ntt_inv_regs_pm<L, 1, C::RQ, C::XB, C::LIM, C::RQ>(y, base.itw_pm + (size_t)it.prime * N, m, lds, tid);
#pragma unroll
    for (int r = 0; r < 16; r++) y[0][r] = canon_rq_pm<C::RQ>(y[0][r], m);
    store_coeff<L>(y[0], out + ((it.o * size + it.poly) * base.count + it.prime) * N, tid);
}

// General path: one thread per NTT slot, canonical arithmetic throughout (sources below q, addmod sums, one Shoup product per
// distinct weight).  Writes the slot-form sum to `out`; fhe_ntt_inverse follows in place.
__global__ __launch_bounds__(256) void k_filter_mac(const u64 *__restrict__ src, const u32 *__restrict__ taps, const ulonglong2 *__restrict__ wv,
                                                    const u32 *__restrict__ wid, u32 nt, u64 *__restrict__ out, u32 size, u64 cnt, u64 total,
                                                    u64 xcd_span, const Modulus *__restrict__ mods, u32 k, u32 n) {
    const u32 per = n / 256;
    const FilterItem it = filter_item(blockIdx.x / per, total, xcd_span, size, cnt);
    if (!it.live) return;
    const u32 slot = (blockIdx.x % per) * 256 + threadIdx.x;
    const u64 q = mods[it.prime].q;
    const u32 *tp = taps + it.o * nt;
    const ulonglong2 *wp = wv + (size_t)it.prime * n + slot;
    const size_t wstride = (size_t)k * n;
    u64 acc = 0, s = 0;
    u32 cur = wid[0];
    for (u32 i = 0; i < nt; i++) {
        const u32 w = wid[i];
        if (w != cur) {
            const ulonglong2 c = wp[cur * wstride];
            acc = addmod(acc, mul_shoup(s, c.x, c.y, q), q);
            s = 0;
            cur = w;
        }
        s = addmod(s, src[(((size_t)tp[i] * size + it.poly) * k + it.prime) * n + slot], q);
    }
    const ulonglong2 c = wp[cur * wstride];
    acc = addmod(acc, mul_shoup(s, c.x, c.y, q), q);
    out[((it.o * size + it.poly) * k + it.prime) * n + slot] = acc;
}

inline bool filter_pm(const fhe_ctx *c) { return c->qb.pm_class && !c->opt.ntt_nopm; }
inline size_t ct_words(const fhe_ctx *c, u32 size) { return (size_t)size * c->k * c->n; }
inline int clampi(long long v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : (int)v; }

}  // namespace

extern "C" int fhe_filter_path(const fhe_ctx *c) {
    if (!c) return fail(FHE_ERR_PARAM, "null argument");
    if (filter_pm(c)) return c->qb.pm_class & 3;
    return (fhe_rgb_f64_supported(c) && !c->opt.force_u64) ? 4 : 0;
}

extern "C" int fhe_filter_plan_create(const fhe_ctx *c, const double *weights, uint32_t kw, uint32_t kh, int int_coeffs, int frac_coeffs,
                                      fhe_stream s, fhe_filter_plan **out) {
    if (!c || !weights || !out) return fail(FHE_ERR_PARAM, "null argument");
    *out = nullptr;
    if (!kw || !kh || (u64)kw * kh > FHE_FILTER_MAX_TAPS)
        return fail(FHE_ERR_PARAM, "filter kernel of %u x %u positions (1 .. FHE_FILTER_MAX_TAPS = %d)", kw, kh, FHE_FILTER_MAX_TAPS);
    const u32 np = kw * kh;
    std::vector<uint64_t> plain(c->n);
    std::vector<double> distinct;
    std::vector<std::vector<uint64_t>> enc;
    int id_of[FHE_FILTER_MAX_TAPS];
    for (u32 p = 0; p < np; ++p) {
        id_of[p] = -1;
        u32 d = 0;
        for (; d < distinct.size(); ++d)
            if (distinct[d] == weights[p]) break;
        if (d < distinct.size()) { id_of[p] = (int)d; continue; }
        const int len = fhe_frac_encode(c->n, c->t, weights[p], int_coeffs, frac_coeffs, plain.data());
        if (len < 0) return len;                               // a weight the encoder cannot hold (fhe_last_error has the text)
        if (len == 0) continue;                                // the zero plaintext: this position is skipped, as the specification says
        id_of[p] = (int)distinct.size();
        distinct.push_back(weights[p]);
        enc.emplace_back(plain.begin(), plain.begin() + len);
    }
    if (distinct.empty()) return fail(FHE_ERR_PARAM, "every weight of the filter kernel encodes to the zero plaintext");
    fhe_filter_plan *p = new fhe_filter_plan();
    p->k = c->k;
    p->n = c->n;
    p->kw = kw;
    p->kh = kh;
    p->nd = (u32)distinct.size();
    u32 wid[FHE_FILTER_MAX_TAPS];
    for (u32 d = 0; d < p->nd; ++d)
        for (u32 q = 0; q < np; ++q)
            if (id_of[q] == (int)d) { p->pos[p->nt] = q; wid[p->nt++] = d; }
    const size_t pw = (size_t)c->k * c->n;
    auto cleanup = [&](int code) {
        if (code) { (void)fhe_filter_plan_destroy(p); }
        return code;
    };
    int rc;
    if ((rc = fhe_dev_alloc(sizeof(ulonglong2) * pw * p->nd, (void **)&p->d_w))) return cleanup(rc);
    if ((rc = fhe_dev_alloc(sizeof(u64) * pw * p->nd, (void **)&p->d_wx))) return cleanup(rc);
    if ((rc = fhe_dev_alloc(sizeof(u32) * FHE_FILTER_MAX_TAPS, (void **)&p->d_wid))) return cleanup(rc);
    hipStream_t st = (hipStream_t)s;
    for (u32 d = 0; d < p->nd; ++d)
        if ((rc = fhe_plain_prepare(c, enc[d].data(), (uint32_t)enc[d].size(), (uint64_t *)(p->d_w + pw * d), s))) return cleanup(rc);
    const u64 total = (u64)pw * p->nd;
    k_pairs_first<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(p->d_w, p->d_wx, total);
    if (hipGetLastError() != hipSuccess) return cleanup(fail(FHE_ERR_HIP, "kernel launch failed"));
    if (hipMemcpyAsync(p->d_wid, wid, sizeof(u32) * p->nt, hipMemcpyHostToDevice, st) != hipSuccess) return cleanup(fail(FHE_ERR_HIP, "upload failed"));
    if (hipStreamSynchronize(st) != hipSuccess) return cleanup(fail(FHE_ERR_HIP, "stream sync failed"));
    *out = p;
    return FHE_OK;
}

extern "C" int fhe_filter_plan_destroy(fhe_filter_plan *p) {
    if (!p) return FHE_OK;
    if (p->d_w) (void)hipFree(p->d_w);
    if (p->d_wx) (void)hipFree(p->d_wx);
    if (p->d_wid) (void)hipFree(p->d_wid);
    delete p;
    return FHE_OK;
}

extern "C" int fhe_filter_plan_taps(const fhe_filter_plan *p) {
    if (!p) return fail(FHE_ERR_PARAM, "null argument");
    return (int)p->nt;
}

// ---- index arithmetic (host only) ------------------------------------------------------------------------------------------------
static int filter_geometry(uint32_t src_w, uint32_t src_h, uint32_t channels, uint32_t kw, uint32_t kh, int ax, int ay, uint32_t sx, uint32_t sy) {
    if (!src_w || !src_h || !channels) return fail(FHE_ERR_PARAM, "empty image");
    if (!kw || !kh || (u64)kw * kh > FHE_FILTER_MAX_TAPS) return fail(FHE_ERR_PARAM, "filter kernel of %u x %u positions (1 .. %d)", kw, kh, FHE_FILTER_MAX_TAPS);
    if (!sx || !sy) return fail(FHE_ERR_PARAM, "strides must be positive");
    if (ax < 0 || ay < 0 || (u32)ax >= kw || (u32)ay >= kh) return fail(FHE_ERR_PARAM, "anchor (%d, %d) outside the %u x %u kernel", ax, ay, kw, kh);
    if ((u64)src_w * src_h * channels > 0xffffffffULL) return fail(FHE_ERR_PARAM, "image too large");
    return FHE_OK;
}

extern "C" int fhe_filter_source_rows(uint32_t src_h, uint32_t kh, int anchor_y, uint32_t stride_y, uint32_t row0, uint32_t row1, uint32_t *first,
                                      uint32_t *count) {
    if (!first || !count) return fail(FHE_ERR_PARAM, "null argument");
    if (!src_h || !kh || kh > FHE_FILTER_MAX_TAPS || !stride_y || anchor_y < 0 || (u32)anchor_y >= kh) return fail(FHE_ERR_PARAM, "bad filter geometry");
    const u32 dst_h = (src_h + stride_y - 1) / stride_y;
    if (row0 >= row1 || row1 > dst_h) return fail(FHE_ERR_PARAM, "destination rows [%u, %u) are not a range of the %u output rows", row0, row1, dst_h);
    const int lo = clampi((long long)row0 * stride_y - anchor_y, 0, (int)src_h - 1);
    const int hi = clampi((long long)(row1 - 1) * stride_y + (kh - 1) - anchor_y, 0, (int)src_h - 1);
    *first = (u32)lo;
    *count = (u32)(hi - lo + 1);
    return FHE_OK;
}

extern "C" int fhe_filter_tap_plan(uint32_t src_w, uint32_t src_h, uint32_t channels, uint32_t kw, uint32_t kh, int anchor_x, int anchor_y,
                                   uint32_t stride_x, uint32_t stride_y, uint32_t row0, uint32_t row1, uint32_t src_row0, uint32_t *dst_w,
                                   uint32_t *dst_h, uint32_t *taps) {
    int rc = filter_geometry(src_w, src_h, channels, kw, kh, anchor_x, anchor_y, stride_x, stride_y);
    if (rc) return rc;
    const u32 dw = (src_w + stride_x - 1) / stride_x, dh = (src_h + stride_y - 1) / stride_y;
    if (dst_w) *dst_w = dw;
    if (dst_h) *dst_h = dh;
    if (!taps) return FHE_OK;
    if (row0 >= row1 || row1 > dh) return fail(FHE_ERR_PARAM, "destination rows [%u, %u) are not a range of the %u output rows", row0, row1, dh);
    u32 first = 0, cnt = 0;
    if ((rc = fhe_filter_source_rows(src_h, kh, anchor_y, stride_y, row0, row1, &first, &cnt))) return rc;
    if (src_row0 > first) return fail(FHE_ERR_PARAM, "the resident window starts at source row %u, rows [%u, %u) read from row %u", src_row0, row0, row1, first);
    const u32 np = kw * kh;
    for (u32 y = row0; y < row1; ++y)
        for (u32 x = 0; x < dw; ++x)
            for (u32 ch = 0; ch < channels; ++ch) {
                u32 *tp = taps + (((size_t)(y - row0) * dw + x) * channels + ch) * np;
                for (u32 j = 0; j < kh; ++j) {
                    const u32 yy = (u32)clampi((long long)y * stride_y + j - anchor_y, 0, (int)src_h - 1) - src_row0;
                    for (u32 i = 0; i < kw; ++i) {
                        const u32 xx = (u32)clampi((long long)x * stride_x + i - anchor_x, 0, (int)src_w - 1);
                        tp[j * kw + i] = (yy * src_w + xx) * channels + ch;
                    }
                }
            }
    return FHE_OK;
}

// ---- the call -------------------------------------------------------------------------------------------------------------------
extern "C" size_t fhe_filter2d_scratch_bytes(const fhe_ctx *c, const fhe_filter_plan *plan, uint32_t size, uint64_t n_src, uint64_t count, int src_is_ntt) {
    (void)count;
    if (!c || !plan || src_is_ntt) return 0;
    return (size_t)n_src * ct_words(c, size) * sizeof(u64);
}

extern "C" int fhe_filter2d(const fhe_ctx *c, const fhe_filter_plan *plan, const uint64_t *src, uint64_t n_src, uint32_t size, int src_is_ntt,
                            const uint32_t *taps, uint64_t *out, uint64_t count, void *scratch, size_t scratch_bytes, fhe_stream s) {
    if (!c || !plan || !src || !out || !taps) return fail(FHE_ERR_PARAM, "null argument");
    if (plan->k != c->k || plan->n != c->n) return fail(FHE_ERR_PARAM, "plan was built for another context");
    if (size == 0 || size > FHE_MAX_POLYS) return fail(FHE_ERR_PARAM, "ciphertext size %u (1 .. %d)", size, FHE_MAX_POLYS);
    if (count == 0) return FHE_OK;
    if (n_src == 0 || n_src > 0xffffffffULL) return fail(FHE_ERR_PARAM, "%llu source ciphertexts", (unsigned long long)n_src);
    const size_t cw = ct_words(c, size);
    const u64 *src_end = (const u64 *)src + n_src * cw, *out_end = (const u64 *)out + count * cw;
    if ((const u64 *)out < src_end && (const u64 *)src < out_end) return fail(FHE_ERR_PARAM, "out overlaps src");
    const size_t need = fhe_filter2d_scratch_bytes(c, plan, size, n_src, count, src_is_ntt);
    if (need) {
        if (!scratch || scratch_bytes < need) return fail(FHE_ERR_PARAM, "scratch too small: need fhe_filter2d_scratch_bytes() = %zu bytes", need);
        const char *sb = (const char *)scratch, *se = sb + need;
        if ((sb < (const char *)out_end && (const char *)out < se) || (sb < (const char *)src_end && (const char *)src < se))
            return fail(FHE_ERR_PARAM, "scratch overlaps src or out");
    }
    const u32 np = plan->kw * plan->kh, nt = plan->nt;
    for (u64 i = 0; i < count * np; ++i)
        if (taps[i] >= n_src) return fail(FHE_ERR_PARAM, "tap %llu of output %llu is %u, the batch has %llu sources", (unsigned long long)(i % np),
                                          (unsigned long long)(i / np), taps[i], (unsigned long long)n_src);
    hipStream_t st = (hipStream_t)s;
    const u64 *xs = (const u64 *)src;
    if (!src_is_ntt) {
        const u64 step = (u64)1 << 20;                          // polynomials per forward launch (even, far below the launch limit)
        const u64 np_src = n_src * size;
        for (u64 d = 0; d < np_src; d += step) {
            const u64 part = np_src - d < step ? np_src - d : step;
            int rc = fhe_ntt_forward(c, src + d * c->k * c->n, (uint64_t *)scratch + d * c->k * c->n, part, s);
            if (rc) return rc;
        }
        xs = (const u64 *)scratch;
    }
    const bool pm = filter_pm(c);
    const RnsBase base = c->qb.dev();
    // outputs per launch: what one staging slot holds of the compacted tap table, at most FILTER_CHUNK_MAX (keeps the grid of k_filter_mac below 2^31)
    const u64 fit = FHE_STAGE_SLOT_BYTES / (sizeof(u32) * nt), per_slot = fit < FILTER_CHUNK_MAX ? fit : FILTER_CHUNK_MAX;
    std::vector<u32> buf;
    for (u64 done = 0; done < count; done += per_slot) {
        const u64 part = count - done < per_slot ? count - done : per_slot;
        buf.resize(part * nt);
        for (u64 o = 0; o < part; ++o)
            for (u32 i = 0; i < nt; ++i) buf[o * nt + i] = taps[(done + o) * np + plan->pos[i]];
        const u64 total = part * size * c->k;
        // one contiguous run of outputs per XCD for the one-workgroup-per-polynomial kernel only: k_filter_mac splits a polynomial over
        // n / 256 workgroups, so consecutive workgroups already share their taps, and the remapping measured 3-11 % slower there
        const u64 xcd_span = (pm && c->opt.filter_xcd) ? (total + 7) / 8 : 0;
        const u64 groups = xcd_span ? xcd_span * 8 : total;
        u64 *po = (u64 *)out + done * cw;
        FheStage sg;
        int rc = fhe_stage_acquire(buf.data(), buf.size() * sizeof(u32), st, &sg);
        if (rc) return rc;
        if (pm) {
#define GO_PM(CC) DISPATCH_L(c->logn, (k_filter_acc_inv_pm<L, CC><<<(unsigned)groups, NttShape<L>::TP, 0, st>>>(xs, (const u32 *)sg.dev, plan->d_wx, plan->d_wid, nt, po, size, part, total, xcd_span, base)))
            if (c->qb.pm_class == 1) { GO_PM(PmA); }
            else { GO_PM(PmB); }
#undef GO_PM
        } else {
            k_filter_mac<<<(unsigned)(groups * (c->n / 256)), 256, 0, st>>>(xs, (const u32 *)sg.dev, plan->d_w, plan->d_wid, nt, po, size, part, total, xcd_span,
                                                                             c->qb.d_mod, c->k, c->n);
        }
        const hipError_t le = hipGetLastError();
        rc = fhe_stage_release(sg, st);
        if (le != hipSuccess) return fail(FHE_ERR_HIP, "kernel launch: %s", hipGetErrorString(le));
        if (rc) return rc;
        if (!pm && (rc = fhe_ntt_inverse(c, (const uint64_t *)po, (uint64_t *)po, part * size, s))) return rc;
    }
    return FHE_OK;
}
