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
// Launches per call:
//   1. fhe_ntt_forward over all n_src * size polynomials into scratch (skipped with src_is_ntt);
//   2. pseudo-Mersenne bases (fhe_remap_path 1 / 2): k_remap_acc_pm<L, C, INV>, one workgroup per output residue polynomial -- gather
//      of the taps' slot vectors, one product per run of taps with one weight id, lazy sums, and with INV the inverse transform in
//      the same kernel;
//      every other base (fhe_remap_path 0 / 4): k_remap_mac (canonical Shoup arithmetic, one thread per slot) into `out`, then
//      fhe_ntt_inverse in place unless out_is_ntt.
// The (tap, weight id) table travels through the staging ring in chunks of FHE_STAGE_SLOT_BYTES / (8 T) outputs (512 .. 4096).
#include "internal.h"

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

namespace {

__global__ void k_pairs_first(const ulonglong2 *__restrict__ in, u64 *__restrict__ out, u64 count) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) out[i] = in[i].x;
}

// Workgroup b -> (prime, output, poly) in plain order, `prime` slowest: the workgroups in flight read the weight vectors of ONE residue,
// and neighbouring workgroups are neighbouring outputs, which share sources (a horizontal pass: columns x, x + 1 read overlapping
// pixels of one row) or weights (a vertical pass: the outputs of one row).  fhe_filter2d's order -- one contiguous run of outputs per
// XCD -- measured 1-10 % slower for the two passes of a resize and is not built in (profiles/EXPERIMENTS.md 16).
struct RemapItem { u32 prime, poly; u64 o; };
__device__ __forceinline__ RemapItem remap_item(u64 b, u32 size, u64 cnt) {
    const u64 per_prime = cnt * size, rem = b % per_prime;
    RemapItem r;
    r.prime = (u32)(b / per_prime);
    r.o = rem / size;
    r.poly = (u32)(rem % size);
    return r;
}

// One table row per output: T (tap, weight id) pairs, the live ones first, FHE_REMAP_SKIP in the id of the first unused pair.
// Lazy sums, in units of q (q < 2^58 for class PmB, < 2^55 for class PmA; fold_pm takes ANY 64-bit value to below 17/16 q):
//   s  sum of the source slots of one run of taps with one weight id.  Sources are canonical (< q: what fhe_ntt_forward and a
//      remap with out_is_ntt write).  s is folded after every REMAP_SUM_FOLD = 16 summands: s < 17/16 + 16 < 18 q < 2^63.  A run
//      of ONE tap is multiplied as it is (canonical, below the 2^(b+1) mulvv_pm asks for); longer runs are folded first.
//   y  sum of the products mulvv_pm(., w) < RQ (6 q class A, 1.5 q class B).  y is folded after every REMAP_PROD_FOLD = 8
//      products: y < 17/16 + 8 RQ <= 49.1 q < 2^61 (class A), 13.1 q < 2^62 (class B).
// Both counters are compile-time constants, so the bounds hold for any T <= FHE_REMAP_MAX_TAPS, any ids and any weights; the
// largest summands (every slot q - 1; 64 distinct ids, 64 equal ids) are a GPU test (tests/test_gpu_resample.py).
constexpr u32 REMAP_SUM_FOLD = 16, REMAP_PROD_FOLD = 8;
constexpr u64 REMAP_CHUNK_MAX = 4096;

template <int L, typename C, bool INV>
__global__ __launch_bounds__(NttShape<L>::TP, 4) void k_remap_acc_pm(const u64 *__restrict__ src, const uint2 *__restrict__ table, u32 T,
                                                                     const u64 *__restrict__ wx, u64 *__restrict__ out, u32 size, u64 cnt, RnsBase base) {
    __shared__ u64 lds[INV ? NttShape<L>::LDS_WORDS : 1];
    constexpr int N = NttShape<L>::N, TP = NttShape<L>::TP;
    const int tid = threadIdx.x;
    const RemapItem it = remap_item(blockIdx.x, size, cnt);          // the grid is exactly cnt * size * primes workgroups
    const PmMod m = base.pm[it.prime];
    const uint2 *row = table + it.o * T;
    const u64 *wp = wx + (size_t)it.prime * N;
    const size_t wstride = (size_t)base.count * N;
    u64 y[1][16], s[16];
#pragma unroll
    for (int r = 0; r < 16; r++) { y[0][r] = 0; s[r] = 0; }
    u32 cur = row[0].y, nsum = 0, nrun = 0, nprod = 0;
    auto flush = [&]() {
        if (nprod == REMAP_PROD_FOLD) {
            nprod = 0;
#pragma unroll
            for (int r = 0; r < 16; r++) y[0][r] = fold_pm(y[0][r], m);
        }
        const u64 *w = wp + cur * wstride;
        if (nrun == 1) {
#pragma unroll
            for (int r = 0; r < 16; r++) {
                y[0][r] += mulvv_pm(s[r], w[r * TP + tid], m);
                s[r] = 0;
            }
        } else {
#pragma unroll
            for (int r = 0; r < 16; r++) {
                y[0][r] += mulvv_pm(fold_pm(s[r], m), w[r * TP + tid], m);
                s[r] = 0;
            }
        }
        nprod++;
        nsum = 0;
        nrun = 0;
    };
    for (u32 i = 0; i < T; i++) {
        const uint2 e = row[i];
        if (e.y == FHE_REMAP_SKIP) break;
        if (e.y != cur) { flush(); cur = e.y; }
        u64 x[16];
        load_slots<L>(x, src + (((size_t)e.x * size + it.poly) * base.count + it.prime) * N, tid);
        if (nsum == REMAP_SUM_FOLD) {
            nsum = 0;
#pragma unroll
            for (int r = 0; r < 16; r++) s[r] = fold_pm(s[r], m);
        }
#pragma unroll
        for (int r = 0; r < 16; r++) s[r] += x[r];
        nsum++;
        nrun++;
    }
    flush();
    u64 *po = out + ((it.o * size + it.poly) * base.count + it.prime) * N;
    if constexpr (INV) {
#pragma unroll
        for (int r = 0; r < 16; r++) y[0][r] = fold_pm(y[0][r], m);
        ntt_inv_regs_pm<L, 1, C::RQ, C::XB, C::LIM, C::RQ>(y, base.itw_pm + (size_t)it.prime * N, m, lds, tid);
#pragma unroll
        for (int r = 0; r < 16; r++) y[0][r] = canon_rq_pm<C::RQ>(y[0][r], m);
        store_coeff<L>(y[0], po, tid);
    } else {
#pragma unroll
        for (int r = 0; r < 16; r++) y[0][r] = canon_pm(y[0][r], m);
        store_slots<L>(y[0], po, tid);
    }
}

// General path: one thread per NTT slot, canonical arithmetic throughout (sources below q, addmod sums, one Shoup product per run of
// taps with one weight id).  Writes the canonical slot-form sum to `out`.
__global__ __launch_bounds__(256) void k_remap_mac(const u64 *__restrict__ src, const uint2 *__restrict__ table, u32 T, const ulonglong2 *__restrict__ wv,
                                                   u64 *__restrict__ out, u32 size, u64 cnt, const Modulus *__restrict__ mods, u32 k, u32 n) {
    const u32 per = n / 256;
    const RemapItem it = remap_item(blockIdx.x / per, size, cnt);    // the grid is exactly cnt * size * primes * per workgroups
    const u32 slot = (blockIdx.x % per) * 256 + threadIdx.x;
    const u64 q = mods[it.prime].q;
    const uint2 *row = table + it.o * T;
    const ulonglong2 *wp = wv + (size_t)it.prime * n + slot;
    const size_t wstride = (size_t)k * n;
    u64 acc = 0, s = 0;
    u32 cur = row[0].y;
    for (u32 i = 0; i < T; i++) {
        const uint2 e = row[i];
        if (e.y == FHE_REMAP_SKIP) break;
        if (e.y != cur) {
            const ulonglong2 c = wp[cur * wstride];
            acc = addmod(acc, mul_shoup(s, c.x, c.y, q), q);
            s = 0;
            cur = e.y;
        }
        s = addmod(s, src[(((size_t)e.x * size + it.poly) * k + it.prime) * n + slot], q);
    }
    const ulonglong2 c = wp[cur * wstride];
    acc = addmod(acc, mul_shoup(s, c.x, c.y, q), q);
    out[((it.o * size + it.poly) * k + it.prime) * n + slot] = acc;
}

inline bool remap_pm(const fhe_ctx *c) { return c->qb.pm_class && !c->opt.ntt_nopm; }
inline size_t ct_words(const fhe_ctx *c, u32 size) { return (size_t)size * c->k * c->n; }
inline long long clampll(long long v, long long lo, long long hi) { return v < lo ? lo : v > hi ? hi : v; }

}  // namespace

extern "C" int fhe_remap_path(const fhe_ctx *c) {
    if (!c) return fail(FHE_ERR_PARAM, "null argument");
    if (remap_pm(c)) return c->qb.pm_class & 3;
    return (fhe_rgb_f64_supported(c) && !c->opt.force_u64) ? 4 : 0;
}

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
    t->pm = remap_pm(c);
    t->id.swap(id);
    const size_t pw = (size_t)c->k * c->n;
    ulonglong2 *d_tmp = nullptr;
    auto cleanup = [&](int code) {
        if (d_tmp) (void)hipFree(d_tmp);
        if (code) (void)fhe_weight_table_destroy(t);
        return code;
    };
    hipStream_t st = (hipStream_t)s;
    int rc;
    if (t->nd && t->pm) {
        // the pseudo-Mersenne kernels read bare values: each entry is prepared into one temporary pair vector and its first halves kept
        if ((rc = fhe_dev_alloc(sizeof(u64) * pw * t->nd, (void **)&t->d_wx))) return cleanup(rc);
        if ((rc = fhe_dev_alloc(sizeof(ulonglong2) * pw, (void **)&d_tmp))) return cleanup(rc);
        for (u32 d = 0; d < t->nd; ++d) {
            if ((rc = fhe_plain_prepare(c, enc[d].data(), (uint32_t)enc[d].size(), (uint64_t *)d_tmp, s))) return cleanup(rc);
            k_pairs_first<<<(unsigned)((pw + 255) / 256), 256, 0, st>>>(d_tmp, t->d_wx + pw * d, pw);
            if (hipGetLastError() != hipSuccess) return cleanup(fail(FHE_ERR_HIP, "kernel launch failed"));
        }
    } else if (t->nd) {
        if ((rc = fhe_dev_alloc(sizeof(ulonglong2) * pw * t->nd, (void **)&t->d_w))) return cleanup(rc);
        for (u32 d = 0; d < t->nd; ++d)
            if ((rc = fhe_plain_prepare(c, enc[d].data(), (uint32_t)enc[d].size(), (uint64_t *)(t->d_w + pw * d), s))) return cleanup(rc);
    }
    if (hipStreamSynchronize(st) != hipSuccess) return cleanup(fail(FHE_ERR_HIP, "stream sync failed"));
    *out = t;
    return cleanup(FHE_OK);
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
    if (!c || !table || src_is_ntt) return 0;
    return (size_t)n_src * ct_words(c, size) * sizeof(u64);
}

extern "C" int fhe_remap(const fhe_ctx *c, const fhe_weight_table *table, const uint64_t *src, uint64_t n_src, uint32_t size, int src_is_ntt,
                         const uint32_t *taps, const uint32_t *wids, uint32_t T, uint64_t *out, int out_is_ntt, uint64_t count, void *scratch,
                         size_t scratch_bytes, fhe_stream s) {
    if (!c || !table || !src || !out || !taps || !wids) return fail(FHE_ERR_PARAM, "null argument");
    if (table->ctx != c) return fail(FHE_ERR_PARAM, "weight table was built for another context");
    if (size == 0 || size > FHE_MAX_POLYS) return fail(FHE_ERR_PARAM, "ciphertext size %u (1 .. %d)", size, FHE_MAX_POLYS);
    if (T == 0 || T > FHE_REMAP_MAX_TAPS) return fail(FHE_ERR_PARAM, "%u taps per output (1 .. FHE_REMAP_MAX_TAPS = %d)", T, FHE_REMAP_MAX_TAPS);
    if (count == 0) return FHE_OK;
    if (n_src == 0 || n_src > 0xffffffffULL) return fail(FHE_ERR_PARAM, "%llu source ciphertexts", (unsigned long long)n_src);
    const size_t cw = ct_words(c, size);
    const u64 *src_end = (const u64 *)src + n_src * cw, *out_end = (const u64 *)out + count * cw;
    if ((const u64 *)out < src_end && (const u64 *)src < out_end) return fail(FHE_ERR_PARAM, "out overlaps src");
    const size_t need = fhe_remap_scratch_bytes(c, table, size, n_src, count, src_is_ntt);
    if (need) {
        if (!scratch || scratch_bytes < need) return fail(FHE_ERR_PARAM, "scratch too small: need fhe_remap_scratch_bytes() = %zu bytes", need);
        const char *sb = (const char *)scratch, *se = sb + need;
        if ((sb < (const char *)out_end && (const char *)out < se) || (sb < (const char *)src_end && (const char *)src < se))
            return fail(FHE_ERR_PARAM, "scratch overlaps src or out");
    }
    // everything is checked before anything is enqueued
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
    const bool pm = table->pm;
    const RnsBase base = c->qb.dev();
    // outputs per launch: what one staging slot holds of the compacted table, at most REMAP_CHUNK_MAX (keeps the grid of k_remap_mac below 2^31)
    const u64 fit = FHE_STAGE_SLOT_BYTES / (sizeof(uint2) * T), per_slot = fit < REMAP_CHUNK_MAX ? fit : REMAP_CHUNK_MAX;
    std::vector<uint2> buf;
    for (u64 done = 0; done < count; done += per_slot) {
        const u64 part = count - done < per_slot ? count - done : per_slot;
        buf.resize(part * T);
        for (u64 o = 0; o < part; ++o) {
            u32 live = 0;
            uint2 *row = buf.data() + o * T;
            for (u32 p = 0; p < T; ++p) {
                const u32 w = wids[(done + o) * T + p];
                if (w == FHE_REMAP_SKIP || table->id[w] == FHE_REMAP_SKIP) continue;
                row[live++] = make_uint2(taps[(done + o) * T + p], table->id[w]);
            }
            for (; live < T; ++live) row[live] = make_uint2(0, FHE_REMAP_SKIP);
        }
        const u64 total = part * size * c->k;                  // output residue polynomials of this launch
        u64 *po = (u64 *)out + done * cw;
        FheStage sg;
        int rc = fhe_stage_acquire(buf.data(), buf.size() * sizeof(uint2), st, &sg);
        if (rc) return rc;
        if (pm) {
#define GO_PM(CC, INV) DISPATCH_L(c->logn, (k_remap_acc_pm<L, CC, INV><<<(unsigned)total, NttShape<L>::TP, 0, st>>>(xs, (const uint2 *)sg.dev, T, table->d_wx, po, size, part, base)))
            if (c->qb.pm_class == 1) {
                if (out_is_ntt) { GO_PM(PmA, false); }
                else { GO_PM(PmA, true); }
            } else {
                if (out_is_ntt) { GO_PM(PmB, false); }
                else { GO_PM(PmB, true); }
            }
#undef GO_PM
        } else {
            k_remap_mac<<<(unsigned)(total * (c->n / 256)), 256, 0, st>>>(xs, (const uint2 *)sg.dev, T, table->d_w, po, size, part, c->qb.d_mod, c->k, c->n);
        }
        const hipError_t le = hipGetLastError();
        rc = fhe_stage_release(sg, st);
        if (le != hipSuccess) return fail(FHE_ERR_HIP, "kernel launch: %s", hipGetErrorString(le));
        if (rc) return rc;
        if (!pm && !out_is_ntt && (rc = fhe_ntt_inverse(c, (const uint64_t *)po, (uint64_t *)po, part * size, s))) return rc;
    }
    return FHE_OK;
}
