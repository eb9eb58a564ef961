// filter.hip -- encrypted 2-D convolution with a public kernel (fhe_filter2d): per output ciphertext
//     out = sum over the kernel positions p with encode(w[p]) != 0 of multiply_plain(src[tap[p]], encode(w[p]))
// (include/fhe_hip.h states the op-by-op specification).  multiply_plain is linear and everything is exact arithmetic mod q, so
//     INTT( sum_p NTT(src[tap[p]]) . NTT(lift(encode(w[p]))) )
// is the same ring element and therefore the same canonical residues: every source polynomial is transformed ONCE however many
// outputs read it, every output polynomial is transformed back ONCE however many taps it has, and the taps that share a weight
// are summed before they are multiplied (a box filter costs one product per slot, Gauss 3x3 three).
//
// This file holds the plan, the index arithmetic and the call's own checks; the kernels and the launch sequence are tap_sum.h's, which
// fhe_remap shares.  Launches per call:
//   1. fhe_ntt_forward over all n_src * size polynomials into scratch (skipped with src_is_ntt);
//   2. pseudo-Mersenne bases (fhe_filter_path 1 / 2): k_tap_sum_pm<L, C, true, SharedIdRows>, one workgroup per output residue
//      polynomial, one contiguous run of outputs per XCD (FHE_FILTER_XCD=0: plain order);
//      every other base (fhe_filter_path 0 / 4): k_tap_sum_mac<SharedIdRows> into `out`, then fhe_ntt_inverse in place.
// The tap table travels through the staging ring in chunks of FHE_STAGE_SLOT_BYTES / (4 * non-zero taps) outputs (1024 .. 4096).
#include "tap_sum.h"

#include "host_math.h"

#include <cstring>
#include <map>
#include <vector>

struct fhe_filter_plan {
    u32 k = 0, n = 0, kw = 0, kh = 0;
    u32 nt = 0, nd = 0;               // non-zero taps, distinct non-zero weights
    u32 pos[FHE_FILTER_MAX_TAPS];     // kernel position (row-major) of sorted tap i; sorted by weight id, then by position
    ulonglong2 *d_w = nullptr;        // [nd][k][n] Shoup pairs, slot order (fhe_plain_prepare)
    u64 *d_wx = nullptr;              // [nd][k][n] the values alone: both forms are kept, so a plan also serves the context's FHE_NTT_NOPM twin
    u32 *d_wid = nullptr;             // [nt] weight id of sorted tap i, non-decreasing
};

extern "C" int fhe_filter_path(const fhe_ctx *c) { return tap_sum_path(c); }

extern "C" int fhe_filter_plan_create(const fhe_ctx *c, const double *weights, uint32_t kw, uint32_t kh, int int_coeffs, int frac_coeffs,
                                      fhe_stream s, fhe_filter_plan **out) {
    if (!c || !weights || !out) return fail(FHE_ERR_PARAM, "null argument");
    *out = nullptr;
    if (!kw || !kh || (u64)kw * kh > FHE_FILTER_MAX_TAPS)
        return fail(FHE_ERR_PARAM, "filter kernel of %u x %u positions (1 .. FHE_FILTER_MAX_TAPS = %d)", kw, kh, FHE_FILTER_MAX_TAPS);
    const u32 np = kw * kh;
    std::vector<uint64_t> plain(c->n);
    std::map<u64, int> seen;                                   // bit pattern of the weight -> id (-1: encodes to zero)
    std::vector<std::vector<uint64_t>> enc;
    int id_of[FHE_FILTER_MAX_TAPS];
    for (u32 p = 0; p < np; ++p) {
        u64 bits;
        memcpy(&bits, &weights[p], sizeof bits);
        const auto hit = seen.find(bits);
        if (hit != seen.end()) { id_of[p] = hit->second; continue; }
        const int len = fhe_frac_encode(c->n, c->t, weights[p], int_coeffs, frac_coeffs, plain.data());
        if (len < 0) return len;                               // a weight the encoder cannot hold (fhe_last_error has the text)
        id_of[p] = len ? (int)enc.size() : -1;                 // the zero plaintext: this position is skipped, as the specification says
        if (len) enc.emplace_back(plain.begin(), plain.begin() + len);
        seen.emplace(bits, id_of[p]);
    }
    if (enc.empty()) return fail(FHE_ERR_PARAM, "every weight of the filter kernel encodes to the zero plaintext");
    fhe_filter_plan *p = new fhe_filter_plan();
    p->k = c->k;
    p->n = c->n;
    p->kw = kw;
    p->kh = kh;
    p->nd = (u32)enc.size();
    u32 wid[FHE_FILTER_MAX_TAPS];
    for (u32 d = 0; d < p->nd; ++d)
        for (u32 q = 0; q < np; ++q)
            if (id_of[q] == (int)d) { p->pos[p->nt] = q; wid[p->nt++] = d; }
    int rc = tap_sum_weights(c, enc, &p->d_w, &p->d_wx, s);
    if (!rc) rc = fhe_dev_alloc(sizeof(u32) * FHE_FILTER_MAX_TAPS, (void **)&p->d_wid);
    if (!rc && hipMemcpyAsync(p->d_wid, wid, sizeof(u32) * p->nt, hipMemcpyHostToDevice, (hipStream_t)s) != hipSuccess) rc = fail(FHE_ERR_HIP, "upload failed");
    if (!rc && hipStreamSynchronize((hipStream_t)s) != hipSuccess) rc = fail(FHE_ERR_HIP, "stream sync failed");   // `wid` is on the stack
    if (rc) {
        (void)fhe_filter_plan_destroy(p);
        return rc;
    }
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
    const int lo = (int)clampll((long long)row0 * stride_y - anchor_y, 0, (int)src_h - 1);
    const int hi = (int)clampll((long long)(row1 - 1) * stride_y + (kh - 1) - anchor_y, 0, (int)src_h - 1);
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
                    const u32 yy = (u32)clampll((long long)y * stride_y + j - anchor_y, 0, (int)src_h - 1) - src_row0;
                    for (u32 i = 0; i < kw; ++i) {
                        const u32 xx = (u32)clampll((long long)x * stride_x + i - anchor_x, 0, (int)src_w - 1);
                        tp[j * kw + i] = (yy * src_w + xx) * channels + ch;
                    }
                }
            }
    return FHE_OK;
}

// ---- the call -------------------------------------------------------------------------------------------------------------------
extern "C" size_t fhe_filter2d_scratch_bytes(const fhe_ctx *c, const fhe_filter_plan *plan, uint32_t size, uint64_t n_src, uint64_t count, int src_is_ntt) {
    (void)count;
    return tap_sum_scratch_bytes(c, plan, size, n_src, src_is_ntt);
}

extern "C" int fhe_filter2d(const fhe_ctx *c, const fhe_filter_plan *plan, const uint64_t *src, uint64_t n_src, uint32_t size, int src_is_ntt,
                            const uint32_t *taps, uint64_t *out, uint64_t count, void *scratch, size_t scratch_bytes, fhe_stream s) {
    if (!c || !plan || !src || !out || !taps) return fail(FHE_ERR_PARAM, "null argument");
    if (plan->k != c->k || plan->n != c->n) return fail(FHE_ERR_PARAM, "plan was built for another context");
    int rc = tap_sum_check("fhe_filter2d", c, plan, src, n_src, size, src_is_ntt, out, count, scratch, scratch_bytes);
    if (rc || count == 0) return rc;
    const u32 np = plan->kw * plan->kh, nt = plan->nt;
    for (u64 i = 0; i < count * np; ++i)
        if (taps[i] >= n_src) return fail(FHE_ERR_PARAM, "tap %llu of output %llu is %u, the batch has %llu sources", (unsigned long long)(i % np),
                                          (unsigned long long)(i / np), taps[i], (unsigned long long)n_src);
    // everything is checked before anything is enqueued
    if (!src_is_ntt && (rc = tap_sum_forward(c, src, n_src, size, scratch, s))) return rc;
    // the non-zero taps in the plan's order.  One contiguous run of outputs per XCD for the one-workgroup-per-polynomial kernel only:
    // k_tap_sum_mac splits a polynomial over n / 256 consecutive workgroups, and the remapping measured 3-11 % slower there
    const auto fill = [&](u64 o, u32 *row) {
        for (u32 i = 0; i < nt; ++i) row[i] = taps[o * np + plan->pos[i]];
    };
    return tap_sum_launch<false>(c, tap_sum_pm(c), c->opt.filter_xcd, src_is_ntt ? (const u64 *)src : (const u64 *)scratch, size,
                                 SharedIdRows{nullptr, plan->d_wid, nt}, plan->d_w, plan->d_wx, fill, out, false, count, s);
}
