// resample.hip -- encrypted resampling with public weights (fhe_remap): per output ciphertext o
//     out[o] = sum over the live slots p of multiply_plain(src[taps[o][p]], encode(w[wids[o][p]]))
// (include/fhe_hip.h states the op-by-op specification).  It is fhe_filter2d with the weights chosen PER OUTPUT: resizing by any
// factor, rotating and warping are linear maps whose weights depend on the geometry alone, which is public.  As in filter.hip,
// everything is exact arithmetic mod q, so
//     INTT( sum_p NTT(src[taps[o][p]]) . NTT(lift(encode(w[wids[o][p]]))) )
// holds the same canonical residues as the op-by-op sequence; with out_is_ntt the sum is stored before the inverse transform, which
// is what fhe_ntt_forward of the specified output holds, and a second fhe_remap reads it with src_is_ntt (the two passes of a
// separable resize share ONE transform pair per ciphertext).
//
// This file holds the weight table, the axis plans and the call's own checks; the kernels and the launch sequence are tap_sum.h's, which
// fhe_filter2d shares.  Launches per call:
//   1. fhe_ntt_forward over all n_src * size polynomials into scratch (skipped with src_is_ntt);
//   2. pseudo-Mersenne bases (fhe_remap_path 1 / 2): k_tap_sum_pm<L, C, INV, OwnIdRows>, one workgroup per output residue polynomial
//      in plain order, with INV the inverse transform in the same kernel;
//      every other base (fhe_remap_path 0 / 4): k_tap_sum_mac<OwnIdRows> into `out`, then fhe_ntt_inverse in place unless out_is_ntt.
// The (tap, weight id) table travels through the staging ring in chunks of FHE_STAGE_SLOT_BYTES / (8 T) outputs (512 .. 4096).
#include "tap_sum.h"

#include "host_math.h"

#include <cmath>
#include <cstring>
#include <map>
#include <vector>

struct fhe_weight_table {
    const fhe_ctx *ctx = nullptr;
    u32 k = 0, n = 0;
    u32 nd = 0;                       // distinct values whose encoding is not the zero plaintext
    bool pm = false;                  // which of the two device forms is held
    std::vector<u32> id;              // [count] entry -> distinct id, FHE_REMAP_SKIP for an entry that encodes to zero
    ulonglong2 *d_w = nullptr;        // [nd][k][n] Shoup pairs, slot order (fhe_plain_prepare): the general path
    u64 *d_wx = nullptr;              // [nd][k][n] the values alone: the pseudo-Mersenne kernels need no companion
};

extern "C" int fhe_remap_path(const fhe_ctx *c) { return tap_sum_path(c); }

// ---- the weight table ------------------------------------------------------------------------------------------------------------
extern "C" int fhe_weight_table_create(const fhe_ctx *c, const double *weights, uint32_t count, int int_coeffs, int frac_coeffs, fhe_stream s,
                                       fhe_weight_table **out) {
    if (!c || !weights || !out) return fail(FHE_ERR_PARAM, "null argument");
    *out = nullptr;
    if (!count) return fail(FHE_ERR_PARAM, "empty weight table");
    std::vector<uint64_t> plain(c->n);
    std::map<u64, u32> seen;                                   // bit pattern of the value -> id (FHE_REMAP_SKIP: encodes to zero)
    std::vector<std::vector<uint64_t>> enc;
    std::vector<u32> id(count);
    for (u32 e = 0; e < count; ++e) {
        if (!std::isfinite(weights[e])) return fail(FHE_ERR_PARAM, "weight %u is not finite", e);
        u64 bits;
        memcpy(&bits, &weights[e], sizeof bits);
        const auto hit = seen.find(bits);
        if (hit != seen.end()) { id[e] = hit->second; continue; }
        const int len = fhe_frac_encode(c->n, c->t, weights[e], int_coeffs, frac_coeffs, plain.data());
        if (len < 0) return len;                               // a weight the encoder cannot hold (fhe_last_error has the text)
        u32 d = FHE_REMAP_SKIP;
        if (len > 0) {
            if (enc.size() >= FHE_REMAP_MAX_WEIGHTS)
                return fail(FHE_ERR_PARAM, "more than FHE_REMAP_MAX_WEIGHTS = %d distinct weights (round them: fhe_resample_axis_plan's weight_bits)", FHE_REMAP_MAX_WEIGHTS);
            d = (u32)enc.size();
            enc.emplace_back(plain.begin(), plain.begin() + len);
        }
        seen.emplace(bits, d);
        id[e] = d;
    }
    fhe_weight_table *t = new fhe_weight_table();
    t->ctx = c;
    t->k = c->k;
    t->n = c->n;
    t->nd = (u32)enc.size();
    t->pm = tap_sum_pm(c);
    t->id.swap(id);
    // only the form the context's kernels read is kept: bare values on the pseudo-Mersenne paths, Shoup pairs otherwise
    const int rc = tap_sum_weights(c, enc, t->pm ? nullptr : &t->d_w, t->pm ? &t->d_wx : nullptr, s);
    if (rc) {
        (void)fhe_weight_table_destroy(t);
        return rc;
    }
    *out = t;
    return FHE_OK;
}

extern "C" int fhe_weight_table_destroy(fhe_weight_table *t) {
    if (!t) return FHE_OK;
    if (t->d_w) (void)hipFree(t->d_w);
    if (t->d_wx) (void)hipFree(t->d_wx);
    delete t;
    return FHE_OK;
}

extern "C" int fhe_weight_table_count(const fhe_weight_table *t) {
    if (!t) return fail(FHE_ERR_PARAM, "null argument");
    return (int)t->id.size();
}

extern "C" int fhe_weight_table_distinct(const fhe_weight_table *t) {
    if (!t) return fail(FHE_ERR_PARAM, "null argument");
    return (int)t->nd;
}

// ---- index and weight arithmetic of one axis (host only) --------------------------------------------------------------------------
namespace {

// the kernel as a function of the signed distance d = (tap position - sample position) / filter scale
double resample_kernel(int kernel, double d) {
    const double a = std::fabs(d);
    switch (kernel) {
        case FHE_RESAMPLE_TRIANGLE: return a < 1.0 ? 1.0 - a : 0.0;
        case FHE_RESAMPLE_CATMULL_ROM:
            if (a <= 1.0) return (1.5 * a - 2.5) * a * a + 1.0;
            if (a < 2.0) return ((-0.5 * a + 2.5) * a - 4.0) * a + 2.0;
            return 0.0;
        case FHE_RESAMPLE_REFERENCE_CUBIC: {
            // homo/fhe_resize.h:150-185 with t3 = t * t: weights (t^2 - t)/2, 1 - t^2, (t^2 + t)/2, 0 of the taps at -1, 0, 1, 2 from
            // the integer position, t the offset: the tap at distance d has t = -1 - d, -d, 1 - d, 2 - d
            if (d <= -2.0 || d > 1.0) return 0.0;
            if (d <= -1.0) { const double t = -1.0 - d; return (t * t - t) / 2.0; }
            if (d <= 0.0) { const double t = -d; return 1.0 - t * t; }
            const double t = 1.0 - d;
            return (t * t + t) / 2.0;
        }
        case FHE_RESAMPLE_LANCZOS3: {
            if (a >= 3.0) return 0.0;
            if (a == 0.0) return 1.0;
            const double px = M_PI * d;
            return 3.0 * std::sin(px) * std::sin(px / 3.0) / (px * px);
        }
        case FHE_RESAMPLE_BOX: return (d >= -0.5 && d < 0.5) ? 1.0 : 0.0;
    }
    return 0.0;
}

}  // namespace

extern "C" int fhe_resample_axis_plan(uint32_t src_len, uint32_t dst_len, int kernel, int antialias, int convention, int weight_bits, uint32_t *T,
                                      uint32_t *taps, double *weights) {
    if (!T) return fail(FHE_ERR_PARAM, "null argument");
    if (!src_len || !dst_len || src_len > 0x7fffffffu || dst_len > 0x7fffffffu) return fail(FHE_ERR_PARAM, "axis of %u -> %u samples", src_len, dst_len);
    if (kernel < FHE_RESAMPLE_TRIANGLE || kernel > FHE_RESAMPLE_BOX) return fail(FHE_ERR_PARAM, "unknown resampling kernel %d", kernel);
    if (convention != FHE_RESAMPLE_HALF_PIXEL && convention != FHE_RESAMPLE_REFERENCE) return fail(FHE_ERR_PARAM, "unknown coordinate convention %d", convention);
    if (convention == FHE_RESAMPLE_REFERENCE && dst_len < 2) return fail(FHE_ERR_PARAM, "the reference's coordinates divide by dst_len - 1");
    if (weight_bits < 0 || weight_bits > 30) return fail(FHE_ERR_PARAM, "weight_bits %d (0 = unrounded, 1 .. 30)", weight_bits);
    if ((taps == nullptr) != (weights == nullptr)) return fail(FHE_ERR_PARAM, "taps and weights come together");
    const bool identity = convention == FHE_RESAMPLE_HALF_PIXEL && src_len == dst_len;
    const bool widen = antialias && src_len > dst_len;
    // c = ceil(radius * filter scale): radius 1 (triangle), 2 (the cubics), 3 (Lanczos-3), 1/2 (box); T = 2 c taps from floor(u) - c + 1 on
    const u64 r2 = kernel == FHE_RESAMPLE_TRIANGLE ? 2 : kernel == FHE_RESAMPLE_BOX ? 1 : kernel == FHE_RESAMPLE_LANCZOS3 ? 6 : 4;   // twice the radius
    const u64 c = widen ? (r2 * src_len + 2 * (u64)dst_len - 1) / (2 * (u64)dst_len) : (r2 + 1) / 2;
    const u64 nt = identity ? 1 : 2 * c;
    if (nt > FHE_REMAP_MAX_TAPS) return fail(FHE_ERR_PARAM, "the widened kernel has %llu taps (at most FHE_REMAP_MAX_TAPS = %d)", (unsigned long long)nt, FHE_REMAP_MAX_TAPS);
    *T = (u32)nt;
    if (!taps) return FHE_OK;
    const double fs = widen ? (double)src_len / (double)dst_len : 1.0;
    const double S = (double)((u64)1 << weight_bits);
    std::vector<long long> m(nt);
    for (u32 x = 0; x < dst_len; ++x) {
        u32 *tp = taps + (size_t)x * nt;
        double *wp = weights + (size_t)x * nt;
        if (identity) { tp[0] = x; wp[0] = 1.0; continue; }
        long long first;
        double off = 0.0;                                      // sample position - floor position (reference convention)
        double u = 0.0;
        if (convention == FHE_RESAMPLE_HALF_PIXEL) {
            u = ((double)x + 0.5) * (double)src_len / (double)dst_len - 0.5;
            first = (long long)std::floor(u) - (long long)c + 1;
        } else {
            const float uf = fhe_resize_ref_coord(x, dst_len, src_len);
            first = (long long)(int)uf - (long long)c + 1;      // int(): towards zero (homo/fhe_resize.h:228,260), floor in the offset (:230,262)
            off = (double)(uf - floorf(uf));
        }
        double sum = 0.0;
        for (u64 i = 0; i < nt; ++i) {
            const long long j = first + (long long)i;
            const double d = convention == FHE_RESAMPLE_HALF_PIXEL ? (double)j - u : (double)((long long)i - (long long)c + 1) - off;
            tp[i] = (u32)clampll(j, 0, (long long)src_len - 1);
            wp[i] = resample_kernel(kernel, d / fs);
            sum += wp[i];
        }
        if (!(std::fabs(sum) > 1e-12)) return fail(FHE_ERR_PARAM, "the weights of output %u sum to zero", x);
        for (u64 i = 0; i < nt; ++i) wp[i] /= sum;
        if (weight_bits) {
            long long tot = 0;
            u64 big = 0;
            for (u64 i = 0; i < nt; ++i) {
                m[i] = (long long)std::floor(wp[i] * S + 0.5);
                tot += m[i];
                if (wp[i] > wp[big]) big = i;
            }
            m[big] += (long long)S - tot;
            for (u64 i = 0; i < nt; ++i) wp[i] = (double)m[i] / S;
        }
    }
    return FHE_OK;
}

// ---- the call ---------------------------------------------------------------------------------------------------------------------
extern "C" size_t fhe_remap_scratch_bytes(const fhe_ctx *c, const fhe_weight_table *table, uint32_t size, uint64_t n_src, uint64_t count, int src_is_ntt) {
    (void)count;
    return tap_sum_scratch_bytes(c, table, size, n_src, src_is_ntt);
}

extern "C" int fhe_remap(const fhe_ctx *c, const fhe_weight_table *table, const uint64_t *src, uint64_t n_src, uint32_t size, int src_is_ntt,
                         const uint32_t *taps, const uint32_t *wids, uint32_t T, uint64_t *out, int out_is_ntt, uint64_t count, void *scratch,
                         size_t scratch_bytes, fhe_stream s) {
    if (!c || !table || !src || !out || !taps || !wids) return fail(FHE_ERR_PARAM, "null argument");
    if (table->ctx != c) return fail(FHE_ERR_PARAM, "weight table was built for another context");
    if (T == 0 || T > FHE_REMAP_MAX_TAPS) return fail(FHE_ERR_PARAM, "%u taps per output (1 .. FHE_REMAP_MAX_TAPS = %d)", T, FHE_REMAP_MAX_TAPS);
    int rc = tap_sum_check("fhe_remap", c, table, src, n_src, size, src_is_ntt, out, count, scratch, scratch_bytes);
    if (rc || count == 0) return rc;
    const u64 n_entries = table->id.size();
    for (u64 o = 0; o < count; ++o) {
        u32 live = 0;
        for (u32 p = 0; p < T; ++p) {
            const u32 w = wids[o * T + p];
            if (w == FHE_REMAP_SKIP) continue;
            if (w >= n_entries) return fail(FHE_ERR_PARAM, "weight id %u in slot %u of output %llu, the table has %llu entries", w, p, (unsigned long long)o,
                                            (unsigned long long)n_entries);
            if (taps[o * T + p] >= n_src) return fail(FHE_ERR_PARAM, "tap %u of output %llu is %u, the batch has %llu sources", p, (unsigned long long)o,
                                                      taps[o * T + p], (unsigned long long)n_src);
            if (table->id[w] != FHE_REMAP_SKIP) live++;
        }
        if (!live) return fail(FHE_ERR_PARAM, "output %llu has no live term (every slot is skipped or multiplies by the zero plaintext)", (unsigned long long)o);
    }
    // everything is checked before anything is enqueued
    if (!src_is_ntt && (rc = tap_sum_forward(c, src, n_src, size, scratch, s))) return rc;
    // the live (tap, distinct id) pairs of an output first, the rest of its row marked unused
    const auto fill = [&](u64 o, uint2 *row) {
        u32 live = 0;
        for (u32 p = 0; p < T; ++p) {
            const u32 w = wids[o * T + p];
            if (w == FHE_REMAP_SKIP || table->id[w] == FHE_REMAP_SKIP) continue;
            row[live++] = make_uint2(taps[o * T + p], table->id[w]);
        }
        for (; live < T; ++live) row[live] = make_uint2(0, FHE_REMAP_SKIP);
    };
    return tap_sum_launch<true>(c, table->pm, false, src_is_ntt ? (const u64 *)src : (const u64 *)scratch, size, OwnIdRows{nullptr, T}, table->d_w,
                                table->d_wx, fill, out, out_is_ntt != 0, count, s);
}
