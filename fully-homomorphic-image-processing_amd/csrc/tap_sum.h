// tap_sum.h -- what fhe_filter2d (filter.hip) and fhe_remap (resample.hip) share: per output ciphertext o
//     out[o] = INTT( sum_i NTT(src[tap(o, i)]) . NTT(lift(encode(w[id(o, i)]))) )
// over the live slots i of the output's table row.  The two calls differ only in where id(o, i) comes from (the row types below);
// the kernels, the operand checks, the forward pass, the weight preparation and the launch loop are here once.
#pragma once
#include "internal.h"

#include <vector>

// ---- table rows: (tap, weight id) of slot i of output o, uniform over the workgroup (scalar loads) -----------------------------------
// Shared ids (fhe_filter2d): u32 table[o * width + i] names the source, the plan's wid[i] (non-decreasing) the weight: 4 bytes per tap
// in the staging slot.  Every slot is live, so the kernels' loops have no exit but their end (TERMINATED = false), and the plan sorts
// the taps by weight, so runs of one tap are the exception and every run is folded (SINGLE_TAP_UNFOLDED = false): with the remap's two
// rules the filter measured 1.0-1.4 % (general kernel) and 0.4-0.7 % (pseudo-Mersenne kernel) slower on Gauss 5x5.
struct SharedIdRows {
    typedef u32 Entry;
    static constexpr bool TERMINATED = false, SINGLE_TAP_UNFOLDED = false;
    const u32 *table, *wid;
    u32 width;
    struct Row {
        const u32 *tp, *wid;
        __device__ __forceinline__ uint2 operator[](u32 i) const { return make_uint2(tp[i], wid[i]); }
    };
    __device__ __forceinline__ Row row(u64 o) const { return Row{table + o * width, wid}; }
};
// Own ids (fhe_remap): uint2 table[o * width + i] = (tap, weight id), the live pairs first, FHE_REMAP_SKIP in the id of the first
// unused pair: 8 bytes per tap.
struct OwnIdRows {
    typedef uint2 Entry;
    static constexpr bool TERMINATED = true, SINGLE_TAP_UNFOLDED = true;
    const uint2 *table;
    u32 width;
    struct Row {
        const uint2 *p;
        __device__ __forceinline__ uint2 operator[](u32 i) const { return p[i]; }
    };
    __device__ __forceinline__ Row row(u64 o) const { return Row{table + o * width}; }
};

// Workgroup -> (prime, output, poly).  `prime` is the slowest index: every workgroup in flight reads the weight vectors of one residue,
// and neighbouring workgroups are neighbouring outputs, whose taps overlap (a 3x3 window shares six of its nine source polynomials with
// the next one).  Workgroups are handed to the eight XCDs round robin; with `xcd_span` != 0 workgroup b works on item
// (b % 8) * xcd_span + b / 8, so that each XCD -- each L2 -- walks its own contiguous run of outputs instead of every eighth one (items
// at or beyond `total` do nothing).  fhe_filter2d asks for that order on the pseudo-Mersenne path (FHE_FILTER_XCD=0: plain order);
// fhe_remap always passes 0: the XCD order measured 1-10 % slower for the two passes of a resize (profiles/EXPERIMENTS.md 16).
struct TapItem { u32 prime, poly; u64 o; bool live; };
__device__ __forceinline__ TapItem tap_item(u64 b, u64 total, u64 xcd_span, u32 size, u64 cnt) {
    const u64 it = xcd_span ? (b & 7) * xcd_span + (b >> 3) : b;
    TapItem r;
    r.live = it < total && (!xcd_span || (b >> 3) < xcd_span);
    const u64 per_prime = cnt * size;
    r.prime = (u32)(it / per_prime);
    const u64 rem = it % per_prime;
    r.o = rem / size;
    r.poly = (u32)(rem % size);
    return r;
}

// Lazy sums, in units of q (q < 2^58 for class PmB, < 2^55 for class PmA; fold_pm takes ANY 64-bit value to below 17/16 q):
//   s  sum of the source slots of one run of taps with one weight id.  Sources MUST be canonical (< q): what fhe_ntt_forward and a
//      remap with out_is_ntt write, and what both calls' src_is_ntt contracts ask for.  s is folded after every TAP_SUM_FOLD = 16
//      summands: s < 17/16 + 16 < 18 q < 2^63.  Where the row type says so (SINGLE_TAP_UNFOLDED), a run of ONE tap is multiplied as it
//      is (canonical, below the 2^(b+1) mulvv_pm asks for); every other run is folded first.
//   y  sum of the products mulvv_pm(., w) < RQ (6 q class A, 1.5 q class B).  y is folded after every TAP_PROD_FOLD = 8 products, as
//      k_sum_inv_pm does: y < 17/16 + 8 RQ <= 49.1 q < 2^61 (class A), 13.1 q < 2^62 (class B).
// Both counters are compile-time constants, so the bounds hold for any row of up to 64 taps, any ids and any weights; the largest
// summands (every slot q - 1; 49 and 64 equal weights, 64 distinct ids) are GPU tests (tests/test_gpu_filter.py, test_gpu_resample.py).
constexpr u32 TAP_SUM_FOLD = 16, TAP_PROD_FOLD = 8;
constexpr u64 TAP_CHUNK_MAX = 4096;

// One workgroup per output residue polynomial, 16 slots per thread: gather of the taps' slot vectors, one product per run of taps with
// one weight id and, with INV, the inverse transform in the same kernel (canonical coefficients); without INV the canonical slot-form
// sum is stored and no LDS is used.  No NTT-form accumulator goes through HBM.
template <int L, typename C, bool INV, typename Rows>
__global__ __launch_bounds__(NttShape<L>::TP, 4) void k_tap_sum_pm(const u64 *__restrict__ src, const Rows rows, const u64 *__restrict__ wx,
                                                                   u64 *__restrict__ out, u32 size, u64 cnt, u64 total, u64 xcd_span, RnsBase base) {
    __shared__ u64 lds[INV ? NttShape<L>::LDS_WORDS : 1];
    constexpr int N = NttShape<L>::N, TP = NttShape<L>::TP;
    const int tid = threadIdx.x;
    const TapItem it = tap_item(blockIdx.x, total, xcd_span, size, cnt);
    if (!it.live) return;                                   // uniform over the workgroup
    const PmMod m = base.pm[it.prime];
    const typename Rows::Row row = rows.row(it.o);
    const u64 *wp = wx + (size_t)it.prime * N;
    const size_t wstride = (size_t)base.count * N;
    u64 y[1][16], s[16];
#pragma unroll
    for (int r = 0; r < 16; r++) { y[0][r] = 0; s[r] = 0; }
    u32 cur = row[0].y, nsum = 0, nrun = 0, nprod = 0;
    auto flush = [&]() {
        if (nprod == TAP_PROD_FOLD) {
            nprod = 0;
#pragma unroll
            for (int r = 0; r < 16; r++) y[0][r] = fold_pm(y[0][r], m);
        }
        const u64 *w = wp + cur * wstride;
        if (Rows::SINGLE_TAP_UNFOLDED && nrun == 1) {
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
    for (u32 i = 0; i < rows.width; i++) {
        const uint2 e = row[i];
        if (Rows::TERMINATED && e.y == FHE_REMAP_SKIP) break;
        if (e.y != cur) { flush(); cur = e.y; }
        u64 x[16];
        load_slots<L>(x, src + (((size_t)e.x * size + it.poly) * base.count + it.prime) * N, tid);
        if (nsum == TAP_SUM_FOLD) {
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
// taps with one weight id), n / 256 consecutive workgroups per polynomial in plain order.  Writes the canonical slot-form sum to `out`.
template <typename Rows>
__global__ __launch_bounds__(256) void k_tap_sum_mac(const u64 *__restrict__ src, const Rows rows, const ulonglong2 *__restrict__ wv,
                                                     u64 *__restrict__ out, u32 size, u64 cnt, u64 total, const Modulus *__restrict__ mods, u32 k, u32 n) {
    const u32 per = n / 256;
    const TapItem it = tap_item(blockIdx.x / per, total, 0, size, cnt);
    if (!it.live) return;
    const u32 slot = (blockIdx.x % per) * 256 + threadIdx.x;
    const u64 q = mods[it.prime].q;
    const typename Rows::Row row = rows.row(it.o);
    const ulonglong2 *wp = wv + (size_t)it.prime * n + slot;
    const size_t wstride = (size_t)k * n;
    u64 acc = 0, s = 0;
    u32 cur = row[0].y;
    for (u32 i = 0; i < rows.width; i++) {
        const uint2 e = row[i];
        if (Rows::TERMINATED && e.y == FHE_REMAP_SKIP) break;
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

static __global__ void k_pairs_first(const ulonglong2 *__restrict__ in, u64 *__restrict__ out, u64 count) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) out[i] = in[i].x;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------
static inline long long clampll(long long v, long long lo, long long hi) { return v < lo ? lo : v > hi ? hi : v; }
static inline size_t ct_words(const fhe_ctx *c, u32 size) { return (size_t)size * c->k * c->n; }
static inline bool tap_sum_pm(const fhe_ctx *c) { return c->qb.pm_class && !c->opt.ntt_nopm; }

// fhe_filter_path / fhe_remap_path
static inline int tap_sum_path(const fhe_ctx *c) {
    if (!c) return fail(FHE_ERR_PARAM, "null argument");
    if (tap_sum_pm(c)) return c->qb.pm_class & 3;
    return (fhe_rgb_f64_supported(c) && !c->opt.force_u64) ? 4 : 0;
}

// the transformed sources, unless the caller brings them
static inline size_t tap_sum_scratch_bytes(const fhe_ctx *c, const void *owner, u32 size, u64 n_src, int src_is_ntt) {
    if (!c || !owner || src_is_ntt) return 0;
    return (size_t)n_src * ct_words(c, size) * sizeof(u64);
}

// The operands both calls take; `entry` names the call in the scratch message.  An empty batch (count == 0) is checked for its size
// only: the caller returns FHE_OK next.
static inline int tap_sum_check(const char *entry, const fhe_ctx *c, const void *owner, const uint64_t *src, u64 n_src, u32 size, int src_is_ntt,
                                const uint64_t *out, u64 count, const void *scratch, size_t scratch_bytes) {
    if (size == 0 || size > FHE_MAX_POLYS) return fail(FHE_ERR_PARAM, "ciphertext size %u (1 .. %d)", size, FHE_MAX_POLYS);
    if (count == 0) return FHE_OK;
    if (n_src == 0 || n_src > 0xffffffffULL) return fail(FHE_ERR_PARAM, "%llu source ciphertexts", (unsigned long long)n_src);
    const size_t cw = ct_words(c, size);
    if (overlap(out, count * cw, src, n_src * cw)) return fail(FHE_ERR_PARAM, "out overlaps src");
    const size_t need = tap_sum_scratch_bytes(c, owner, size, n_src, src_is_ntt);
    if (need) {
        if (!scratch || scratch_bytes < need) return fail(FHE_ERR_PARAM, "scratch too small: need %s_scratch_bytes() = %zu bytes", entry, need);
        if (overlap(scratch, need / 8, out, count * cw) || overlap(scratch, need / 8, src, n_src * cw)) return fail(FHE_ERR_PARAM, "scratch overlaps src or out");
    }
    return FHE_OK;
}

// fhe_ntt_forward of all n_src * size source polynomials into scratch
static inline int tap_sum_forward(const fhe_ctx *c, const uint64_t *src, u64 n_src, u32 size, void *scratch, fhe_stream s) {
    const u64 step = (u64)1 << 20;                              // polynomials per forward launch (even, far below the launch limit)
    const u64 np_src = n_src * size;
    for (u64 d = 0; d < np_src; d += step) {
        const u64 part = np_src - d < step ? np_src - d : step;
        int rc = fhe_ntt_forward(c, src + d * c->k * c->n, (uint64_t *)scratch + d * c->k * c->n, part, s);
        if (rc) return rc;
    }
    return FHE_OK;
}

// The encoded distinct plaintexts `enc`, lifted and transformed (fhe_plain_prepare), as [nd][k][n] Shoup pairs (*pairs) and / or their
// bare values (*values: the pseudo-Mersenne kernel needs no companion); a null pointer = that form is not kept, and the pairs then pass
// through one temporary vector.  Synchronises the stream.  On failure the caller frees what was allocated.
static inline int tap_sum_weights(const fhe_ctx *c, const std::vector<std::vector<uint64_t>> &enc, ulonglong2 **pairs, u64 **values, fhe_stream s) {
    const size_t pw = (size_t)c->k * c->n, nd = enc.size();
    hipStream_t st = (hipStream_t)s;
    ulonglong2 *tmp = nullptr;
    int rc = FHE_OK;
    if (nd && values) rc = fhe_dev_alloc(sizeof(u64) * pw * nd, (void **)values);
    if (nd && !rc) rc = pairs ? fhe_dev_alloc(sizeof(ulonglong2) * pw * nd, (void **)pairs) : fhe_dev_alloc(sizeof(ulonglong2) * pw, (void **)&tmp);
    for (size_t d = 0; d < nd && !rc; ++d) {
        ulonglong2 *w = pairs ? *pairs + pw * d : tmp;
        if ((rc = fhe_plain_prepare(c, enc[d].data(), (uint32_t)enc[d].size(), (uint64_t *)w, s)) || !values) continue;
        k_pairs_first<<<(unsigned)((pw + 255) / 256), 256, 0, st>>>(w, *values + pw * d, pw);
        if (hipGetLastError() != hipSuccess) rc = fail(FHE_ERR_HIP, "kernel launch failed");
    }
    if (!rc && hipStreamSynchronize(st) != hipSuccess) rc = fail(FHE_ERR_HIP, "stream sync failed");
    if (tmp) (void)hipFree(tmp);
    return rc;
}

// The launches after the forward pass.  `rows` comes without its table: fill(o, row) writes output o's compacted row of rows.width
// entries, and the table travels through the staging ring in chunks of FHE_STAGE_SLOT_BYTES / (entry bytes * width) outputs, at most
// TAP_CHUNK_MAX (keeps the grid of k_tap_sum_mac below 2^31).  pm: k_tap_sum_pm on `values` (xcd: one contiguous run of outputs per XCD),
// else k_tap_sum_mac on `pairs`.  slot_form: the canonical slot-form sum stays in `out` (fhe_remap's out_is_ntt); otherwise the inverse
// transform runs, inside k_tap_sum_pm or as fhe_ntt_inverse in place.  HAS_SLOT_FORM only says whether the caller ever asks for slot
// form: fhe_filter2d does not, and so does not instantiate the ten INV = false kernels.
template <bool HAS_SLOT_FORM, typename Rows, typename Fill>
static int tap_sum_launch(const fhe_ctx *c, bool pm, bool xcd, const u64 *xs, u32 size, Rows rows, const ulonglong2 *pairs, const u64 *values, Fill fill,
                          uint64_t *out, bool slot_form, u64 count, fhe_stream s) {
    typedef typename Rows::Entry Entry;
    hipStream_t st = (hipStream_t)s;
    const RnsBase base = c->qb.dev();
    const u64 fit = FHE_STAGE_SLOT_BYTES / (sizeof(Entry) * rows.width), per_slot = fit < TAP_CHUNK_MAX ? fit : TAP_CHUNK_MAX;
    std::vector<Entry> buf;
    for (u64 done = 0; done < count; done += per_slot) {
        const u64 part = count - done < per_slot ? count - done : per_slot;
        buf.resize(part * rows.width);
        for (u64 o = 0; o < part; ++o) fill(done + o, buf.data() + o * rows.width);
        const u64 total = part * size * c->k;                  // output residue polynomials of this launch
        const u64 xcd_span = (pm && xcd) ? (total + 7) / 8 : 0;
        const u64 groups = xcd_span ? xcd_span * 8 : total;
        u64 *po = (u64 *)out + done * ct_words(c, size);
        FheStage sg;
        int rc = fhe_stage_acquire(buf.data(), buf.size() * sizeof(Entry), st, &sg);
        if (rc) return rc;
        rows.table = (const Entry *)sg.dev;
        if (pm) {
#define GO_PM(CC, INV) DISPATCH_L(c->logn, (k_tap_sum_pm<L, CC, INV, Rows><<<(unsigned)groups, NttShape<L>::TP, 0, st>>>(xs, rows, values, po, size, part, total, xcd_span, base)))
            const bool a = c->qb.pm_class == 1;
            if constexpr (HAS_SLOT_FORM) {
                if (slot_form && a) { GO_PM(PmA, false); }
                else if (slot_form) { GO_PM(PmB, false); }
            }
            if (!slot_form && a) { GO_PM(PmA, true); }
            else if (!slot_form) { GO_PM(PmB, true); }
#undef GO_PM
        } else {
            k_tap_sum_mac<Rows><<<(unsigned)(total * (c->n / 256)), 256, 0, st>>>(xs, rows, pairs, po, size, part, total, c->qb.d_mod, c->k, c->n);
        }
        const hipError_t le = hipGetLastError();
        rc = fhe_stage_release(sg, st);
        if (le != hipSuccess) return fail(FHE_ERR_HIP, "kernel launch: %s", hipGetErrorString(le));
        if (rc) return rc;
        if (!pm && !slot_form && (rc = fhe_ntt_inverse(c, (const uint64_t *)po, (uint64_t *)po, part * size, s))) return rc;
    }
    return FHE_OK;
}
