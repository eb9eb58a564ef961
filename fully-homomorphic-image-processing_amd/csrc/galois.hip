// galois.hip -- seal::PolyCRTBuilder (batched plaintext slots) and seal::Evaluator::rotate_rows / rotate_columns (Galois
// automorphisms of size-2 ciphertexts followed by a key switch) on gfx950.  include/fhe_hip.h states the operations.
//
// apply_galois(ct, g, key_g) = key switch of [sigma_g(c0), 0, sigma_g(c1)] with the keys for sigma_g(s).  The key switch is
// behz.hip's (digits -> forward transforms -> accumulate against the key -> inverse transforms -> add); what is new is that its
// source polynomials are read THROUGH the automorphism.  sigma_g as a gather: output coefficient j comes from source
// coefficient s = j g^-1 mod 2n, negated modulo the residue's prime when s >= n (x^n = -1; the negation of 0 is 0).
//
// Two paths, the same bits:
//   staged (FHE_GALOIS_STAGED=1): k_galois_stage writes [sigma(c0), 0, sigma(c1)] to scratch (gathered loads, coalesced stores) and
//       fhe_relinearize_poly runs on it unchanged -- the correctness baseline;
//   fused (default): the digit kernel loads c1 through the index map (k_galois_fwd_pm on the pseudo-Mersenne bases,
//       k_galois_digits on the general path), behz.hip's accumulation runs unchanged, and the last kernel adds sigma(c0) to
//       polynomial 0 and nothing to polynomial 1 (k_galois_inv_add_pm / k_galois_add): 3 k n words per ciphertext are neither
//       written nor read back.
// The gather is a permutation with stride g^-1 of 8-byte words.  The pseudo-Mersenne kernels own a whole residue polynomial per
// workgroup (32-64 KiB at the presets), so every line a wave touches is used completely by the workgroup, and the k workgroups of one
// digit sit next to each other: the permuted addresses are served by L2 / the vector cache.  The digit kernel -- which reads the same
// source k digits times -- therefore gathers straight from global memory; loading the polynomial with coalesced reads into the
// transform's LDS array and taking the permuted values from there (an odd stride in 8-byte units is conflict-free) costs two barriers
// and 32 LDS accesses per thread and measured 2-4 % slower per rotation at P8192 (FHE_GALOIS_GATHER_LDS=1 keeps it for A/B runs;
// DESIGN.md 3.10).  The LAST kernel always takes sigma(c0) through LDS, after its transform: that makes in place (out2 == ct2) safe by
// construction -- every global read of the workgroup's source polynomial has landed in LDS before the barrier that precedes its first
// store, and no other workgroup writes that polynomial -- and keeps sixteen registers out of the transform (no spills).
// The general path's kernels are element-wise grids, where a block's gathered reads cross other blocks' writes: its first kernel
// therefore stores sigma(c0) beside the digits (k n words per ciphertext) and the last one adds from there.
#include "internal.h"

#include <cstdlib>
#include <vector>

#include "host_math.h"

namespace {

struct GalMods { u64 q[FHE_MAX_K], r64[FHE_MAX_K]; };      // q_i and floor(2^64 / q_i), by value (wave-uniform)

// source of output coefficient j under sigma_g: index and whether it is negated.  j < n <= 2^14 and ginv < 2n <= 2^15: no overflow
__device__ __forceinline__ u32 gal_src(u32 j, u32 ginv, u32 n, bool &neg) {
    const u32 s = (j * ginv) & (2 * n - 1);
    neg = s >= n;
    return s & (n - 1);
}
__device__ __forceinline__ u64 gal_load(const u64 *__restrict__ p, u32 j, u32 ginv, u32 n, u64 q) {
    bool neg;
    const u64 v = p[gal_src(j, ginv, n, neg)];
    return neg ? negmod(v, q) : v;
}
__device__ __forceinline__ u64 reduce64(u64 x, u64 q, u64 r64) {   // x mod q for any x < 2^64
    u64 r = x - __umul64hi(x, r64) * q;
    r = csub(r, 2 * q);
    return csub(r, q);
}
inline dim3 grid2(u32 n, u64 rows) { return dim3((n + 255) / 256, (unsigned)(rows < 32768 ? (rows ? rows : 1) : 32768)); }

// staged path: stage [count][3][k][n] = [sigma(c0), 0, sigma(c1)]
__global__ __launch_bounds__(256) void k_galois_stage(const u64 *__restrict__ ct, u64 stride, u64 *__restrict__ stage, GalMods M, u32 k, u32 n, u32 ginv, u64 count) {
    for (u64 u = blockIdx.y; u < count * 3 * k; u += gridDim.y) {
        const u32 i = (u32)(u % k), pp = (u32)((u / k) % 3);
        const u64 c = u / (3 * k);
        const u64 *src = ct + c * stride + ((u64)(pp >> 1) * k + i) * n;
        u64 *dst = stage + u * n;
        for (u32 j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) dst[j] = pp == 1 ? 0 : gal_load(src, j, ginv, n, M.q[i]);
    }
}

// general path (1): k_relin_digits with sigma(c1) as its source; the unit of digit 0 also stores sigma(c0_i) for the last kernel
__global__ __launch_bounds__(256) void k_galois_digits(const u64 *__restrict__ ct, u64 stride, u64 *__restrict__ dig, u64 *__restrict__ s0, GalMods M, u32 k, u32 n,
                                                       u32 nd, u32 dbc, u32 ginv, u64 count) {
    const u64 mask = (1ULL << dbc) - 1;            // dbc <= 60
    for (u64 u = blockIdx.y; u < count * k * nd; u += gridDim.y) {
        const u32 d = (u32)(u % nd), i = (u32)((u / nd) % k);
        const u64 c = u / ((u64)nd * k);
        const u64 *c0 = ct + c * stride + (u64)i * n, *c1 = c0 + (u64)k * n;
        for (u32 j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
            const u64 v = (gal_load(c1, j, ginv, n, M.q[i]) >> (dbc * d)) & mask;
            for (u32 ii = 0; ii < k; ii++) dig[(u * k + ii) * n + j] = reduce64(v, M.q[ii], M.r64[ii]);
            if (d == 0) s0[(c * k + i) * n + j] = gal_load(c0, j, ginv, n, M.q[i]);
        }
    }
}
// general path (last): out0 = sigma(c0) + acc0, out1 = acc1
__global__ __launch_bounds__(256) void k_galois_add(u64 *__restrict__ out, u64 out_stride, const u64 *__restrict__ acc, const u64 *__restrict__ s0, GalMods M, u32 k, u32 n,
                                                    u64 count) {
    for (u64 u = blockIdx.y; u < count * 2 * k; u += gridDim.y) {
        const u32 ii = (u32)(u % k), pp = (u32)((u / k) & 1);
        const u64 c = u / (2 * k);
        u64 *dst = out + c * out_stride + ((u64)pp * k + ii) * n;
        const u64 *a = acc + u * n, *s = s0 + (c * k + ii) * n;
        for (u32 j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) dst[j] = pp ? a[j] : addmod(s[j], a[j], M.q[ii]);
    }
}

// sigma_g of one residue polynomial into the registers of load_coeff's mapping (element r TP + tid): through LDS (coalesced global
// reads, permuted LDS reads; both barriers are part of it: the second frees the array for the transform) or straight from global memory
template <int L, bool VIA_LDS>
__device__ __forceinline__ void gal_load_coeff(u64 (&x)[16], const u64 *__restrict__ p, u32 ginv, u64 q, u64 *lds, int tid) {
    constexpr int N = NttShape<L>::N, TP = NttShape<L>::TP;
    if constexpr (VIA_LDS) {
#pragma unroll
        for (int r = 0; r < 16; r++) lds[r * TP + tid] = p[r * TP + tid];
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 16; r++) {
            bool neg;
            const u64 v = lds[gal_src((u32)(r * TP + tid), ginv, N, neg)];
            x[r] = neg ? negmod(v, q) : v;
        }
        __syncthreads();
    } else {
#pragma unroll
        for (int r = 0; r < 16; r++) x[r] = gal_load(p, (u32)(r * TP + tid), ginv, N, q);
    }
}

// pseudo-Mersenne path (1): k_relin_fwd_pm with sigma(c1_i) as its source.  Workgroup (c, i, d, ii): digit d of sigma(c1_i), transformed
// modulo q_ii; the negation is modulo the SOURCE prime q_i, before the digit is taken.
template <int L, typename C, bool VIA_LDS>
__global__ __launch_bounds__(NttShape<L>::TP, 4) void k_galois_fwd_pm(const u64 *__restrict__ ct, u64 stride, u64 *__restrict__ dig, RnsBase base, u32 nd, u32 dbc, u32 ginv) {
    __shared__ u64 lds[NttShape<L>::LDS_WORDS];
    constexpr int N = NttShape<L>::N;
    const int tid = threadIdx.x;
    const u32 k = base.count, ii = blockIdx.x % k;
    const u64 u = blockIdx.x / k;                  // (c * k + i) * nd + d
    const u32 d = (u32)(u % nd), i = (u32)((u / nd) % k);
    const u64 c = u / ((u64)nd * k);
    const u64 mask = (1ULL << dbc) - 1;            // dbc <= 60
    const PmMod m = base.pm[ii];
    u64 x[1][16];
    gal_load_coeff<L, VIA_LDS>(x[0], ct + c * stride + ((u64)k + i) * N, ginv, base.pm[i].q, lds, tid);
    const bool wide = dbc >= m.sh + 32;            // the digit may reach q_ii
#pragma unroll
    for (int r = 0; r < 16; r++) {
        x[0][r] = (x[0][r] >> (dbc * d)) & mask;
        if (wide) x[0][r] = fold_pm(x[0][r], m);
    }
    ntt_fwd_regs_pm<L, 1, PM_FOLDED, C::LIM, C::CS>(x, base.tw_pm + (size_t)ii * N, m, lds, tid);
#pragma unroll
    for (int r = 0; r < 16; r++) x[0][r] = canon_pm(x[0][r], m);
    store_slots<L>(x[0], dig + (u * k + ii) * N, tid);
}
// pseudo-Mersenne path (3): k_relin_inv_add_pm with sigma(c0) added to polynomial 0 and nothing to polynomial 1.  sigma(c0_ii) always
// comes through LDS: every global read of the polynomial is complete at the barrier, so the store may land on it (in place).
template <int L, typename C>
__global__ __launch_bounds__(NttShape<L>::TP, 4) void k_galois_inv_add_pm(const u64 *ct, u64 stride, u64 *out, u64 out_stride, const u64 *__restrict__ acc, RnsBase base, u32 ginv) {
    __shared__ u64 lds[NttShape<L>::LDS_WORDS];
    constexpr int N = NttShape<L>::N;
    const int tid = threadIdx.x;
    const u32 k = base.count, ii = blockIdx.x % k, pp = (blockIdx.x / k) & 1;
    const u64 c = blockIdx.x / (2 * k);
    const PmMod m = base.pm[ii];
    u64 x[1][16];
    u64 *dst = out + c * out_stride + ((u64)pp * k + ii) * N;
    load_slots<L>(x[0], acc + (u64)blockIdx.x * N, tid);
    ntt_inv_regs_pm<L, 1, PM_FOLDED, C::XB, C::LIM, C::RQ>(x, base.itw_pm + (size_t)ii * N, m, lds, tid);
#pragma unroll
    for (int r = 0; r < 16; r++) x[0][r] = canon_rq_pm<C::RQ>(x[0][r], m);
    if (pp == 0) {                                 // uniform per workgroup; after the transform: sixteen registers less are live through it (no spills)
        u64 y[16];
        __syncthreads();                           // the transform's last transpose has read the array
        gal_load_coeff<L, true>(y, ct + c * stride + (u64)ii * N, ginv, m.q, lds, tid);
#pragma unroll
        for (int r = 0; r < 16; r++) x[0][r] = addmod(x[0][r], y[r], m.q);
    }
    store_coeff<L>(x[0], dst, tid);
}

GalMods gal_mods(const fhe_ctx *c) {
    GalMods M{};
    for (u32 i = 0; i < c->k; i++) {
        M.q[i] = c->qb.primes[i];
        M.r64[i] = (u64)(((unsigned __int128)1 << 64) / M.q[i]);
    }
    return M;
}

int fused_pm(const fhe_ctx *c, const u64 *ct, u64 stride, u64 *out2, u64 out_stride, u64 count, u32 ginv, const u64 *evk, u32 dbc, u64 *scratch, hipStream_t st) {
    const u32 k = c->k, nd = fhe_evk_digits(c, dbc);
    u64 *dig = scratch, *acc = dig + count * k * nd * k * c->n;
    const RnsBase base = c->qb.dev();
    const bool via_lds = c->opt.galois_gather_lds;
#define GO_PM(CC)                                                                                                                       \
    DISPATCH_L(c->logn, {                                                                                                               \
        if (via_lds) k_galois_fwd_pm<L, CC, true><<<(unsigned)(count * k * nd * k), NttShape<L>::TP, 0, st>>>(ct, stride, dig, base, nd, dbc, ginv); \
        else k_galois_fwd_pm<L, CC, false><<<(unsigned)(count * k * nd * k), NttShape<L>::TP, 0, st>>>(ct, stride, dig, base, nd, dbc, ginv);        \
        if (int rc = fhe_relin_accum(c, dig, evk, acc, nd, count, st)) return rc;                                                       \
        k_galois_inv_add_pm<L, CC><<<(unsigned)(count * 2 * k), NttShape<L>::TP, 0, st>>>(ct, stride, out2, out_stride, acc, base, ginv); \
    })
    if (c->qb.pm_class == 1) { GO_PM(PmA); } else { GO_PM(PmB); }
#undef GO_PM
    KERNEL_CHECK();
    return FHE_OK;
}

int fused_general(const fhe_ctx *c, const u64 *ct, u64 stride, u64 *out2, u64 out_stride, u64 count, u32 ginv, const u64 *evk, u32 dbc, u64 *scratch, hipStream_t st) {
    const u32 k = c->k, n = c->n, nd = fhe_evk_digits(c, dbc);
    u64 *dig = scratch, *acc = dig + count * k * nd * k * n, *s0 = acc + count * 2 * k * n;
    const GalMods M = gal_mods(c);
    int rc;
    k_galois_digits<<<grid2(n, count * k * nd), 256, 0, st>>>(ct, stride, dig, s0, M, k, n, nd, dbc, ginv, count);
    if ((rc = fhe_qbase_ntt(false, c, dig, dig, count * k * nd, st))) return rc;
    if ((rc = fhe_relin_accum(c, dig, evk, acc, nd, count, st))) return rc;
    if ((rc = fhe_qbase_ntt(true, c, acc, acc, count * 2, st))) return rc;
    k_galois_add<<<grid2(n, count * 2 * k), 256, 0, st>>>(out2, out_stride, acc, s0, M, k, n, count);
    KERNEL_CHECK();
    return FHE_OK;
}

}  // namespace

// [sigma(c0), 0, sigma(c1)] for every ciphertext, then the key switch's own digits and accumulators: enough for either path
extern "C" size_t fhe_apply_galois_scratch_bytes(const fhe_ctx *c, uint32_t dbc, uint64_t count) {
    if (!c || !dbc) return 0;
    return (size_t)count * 3 * c->k * c->n * sizeof(u64) + fhe_relinearize_scratch_bytes(c, dbc, count);
}

extern "C" int fhe_apply_galois(const fhe_ctx *c, const uint64_t *ct2, uint64_t stride, uint64_t *out2, uint64_t out_stride, uint64_t count, uint32_t g,
                                const uint64_t *evk, uint32_t dbc, void *scratch, size_t scratch_bytes, fhe_stream s) {
    if (!c || !ct2 || !evk || !out2) return fail(FHE_ERR_PARAM, "null argument");
    if (dbc < 1 || dbc > 60) return fail(FHE_ERR_PARAM, "decomposition bit count out of range");
    const u32 k = c->k, n = c->n;
    if (!(g & 1) || g >= 2 * n || g == 1) return fail(FHE_ERR_PARAM, "Galois element %u: must be odd and in (1, 2n = %u)", g, 2 * n);
    const u64 ctw = (u64)2 * k * n;
    if (stride < ctw || out_stride < ctw) return fail(FHE_ERR_PARAM, "stride smaller than a size-2 ciphertext");
    if (count && (!scratch || scratch_bytes < fhe_apply_galois_scratch_bytes(c, dbc, count))) return fail(FHE_ERR_PARAM, "scratch too small");
    if (!count) return FHE_OK;
    const uintptr_t i0 = (uintptr_t)ct2, i1 = i0 + ((count - 1) * stride + ctw) * sizeof(u64);
    const uintptr_t o0 = (uintptr_t)out2, o1 = o0 + ((count - 1) * out_stride + ctw) * sizeof(u64);
    if (!(out2 == ct2 && out_stride == stride) && o0 < i1 && i0 < o1)
        return fail(FHE_ERR_PARAM, "output range overlaps the input range (only out2 == ct2 with out_stride == stride may alias)");
    const uintptr_t s0 = (uintptr_t)scratch, s1 = s0 + fhe_apply_galois_scratch_bytes(c, dbc, count);
    if ((s0 < i1 && i0 < s1) || (s0 < o1 && o0 < s1)) return fail(FHE_ERR_PARAM, "scratch overlaps the input or the output");
    if (int rc = fhe_behz_ensure(c)) return rc;
    hipStream_t st = (hipStream_t)s;
    const u32 nd = fhe_evk_digits(c, dbc);
    const u32 ginv = (u32)hostmath::powmod(g, n / 2 - 1, 2 * (u64)n);      // the units modulo 2n have exponent n / 2
    u64 *scr = (u64 *)scratch;
    if (c->opt.galois_staged) {
        k_galois_stage<<<grid2(n, count * 3 * k), 256, 0, st>>>((const u64 *)ct2, stride, scr, gal_mods(c), k, n, ginv, count);
        KERNEL_CHECK();
        u64 *rest = scr + count * 3 * k * n;
        return fhe_relinearize_poly(c, (const uint64_t *)scr, (u64)3 * k * n, 2, out2, out_stride, count, evk, dbc, rest, scratch_bytes - (size_t)count * 3 * k * n * sizeof(u64), s);
    }
    if (fhe_relin_pm_ok(c, nd, count)) return fused_pm(c, (const u64 *)ct2, stride, (u64 *)out2, out_stride, count, ginv, (const u64 *)evk, dbc, scr, st);
    return fused_general(c, (const u64 *)ct2, stride, (u64 *)out2, out_stride, count, ginv, (const u64 *)evk, dbc, scr, st);
}

// ---- host only: Galois elements and the slot encoder ---------------------------------------------------------------------------
extern "C" int fhe_galois_element(uint32_t n, int steps, int swap_rows, uint32_t *g) {
    if (!g) return fail(FHE_ERR_PARAM, "null argument");
    if (n < 4 || (n & (n - 1)) || n > (1u << 16)) return fail(FHE_ERR_PARAM, "n = %u is not a power of two in 4 .. 65536", n);
    const long long half = n / 2;                                   // slots per row = order of 3 modulo 2n
    long long sred = (long long)steps % half;
    if (sred < 0) sred += half;                                     // left by s == left by s mod n/2; 3^(n/2 - s) is the inverse of 3^s
    u64 e = hostmath::powmod(3, (u64)sred, 2 * (u64)n);
    if (swap_rows) e = hostmath::mulmod(e, 2 * (u64)n - 1, 2 * (u64)n);
    *g = (uint32_t)e;
    return FHE_OK;
}

namespace {
// zeta: the smallest primitive 2n-th root of unity modulo t; 0 (with the error set) when t does not support batching
u64 batch_root(u32 n, u64 t) {
    if (n < 4 || (n & (n - 1)) || n > (1u << 16)) { fail(FHE_ERR_PARAM, "n = %u is not a power of two in 4 .. 65536", n); return 0; }
    if (t >> 61 || !hostmath::is_prime(t) || (t - 1) % (2 * (u64)n)) {
        fail(FHE_ERR_PARAM, "batching needs a prime plain modulus t = 1 (mod 2n) below 2^61; t = %llu, n = %u", (unsigned long long)t, n);
        return 0;
    }
    u64 root = 0;
    for (u64 b = 2; !root && b < t; ++b) {
        const u64 c = hostmath::powmod(b, (t - 1) / (2 * (u64)n), t);
        if (hostmath::powmod(c, n, t) == t - 1) root = c;
    }
    u64 best = root, p = root;
    const u64 sq = hostmath::mulmod(root, root, t);
    for (u32 e = 3; e < 2 * n; e += 2) {                             // the primitive roots are the odd powers of any one of them
        p = hostmath::mulmod(p, sq, t);
        if (p < best) best = p;
    }
    return best;
}
// a[j] <- sum_i a[i] w^(i j) mod t, w a primitive len-th root of unity (radix 2, in place, natural order in and out)
void cyclic_ntt(std::vector<u64> &a, u64 w, u64 t) {
    const size_t len = a.size();
    int bits = 0;
    while (((size_t)1 << bits) < len) ++bits;
    for (size_t i = 0; i < len; ++i) {
        const size_t j = hostmath::bit_reverse((uint32_t)i, bits);
        if (i < j) std::swap(a[i], a[j]);
    }
    for (size_t h = 1; h < len; h <<= 1) {
        const u64 wh = hostmath::powmod(w, len / (2 * h), t);
        for (size_t b = 0; b < len; b += 2 * h) {
            u64 f = 1;
            for (size_t i = b; i < b + h; ++i) {
                const u64 x = a[i], y = hostmath::mulmod(a[i + h], f, t);
                a[i] = hostmath::addmod(x, y, t);
                a[i + h] = hostmath::submod(x, y, t);
                f = hostmath::mulmod(f, wh, t);
            }
        }
    }
}
// exponent e of slot (row, j): 3^j for row 0, 2n - 3^j for row 1; the evaluation at zeta^e sits at index (e - 1) / 2 of the cyclic transform
// of the twisted coefficients (m(zeta^(2 i + 1)) = sum_c m_c zeta^c (zeta^2)^(c i))
std::vector<u32> slot_index(u32 n) {
    std::vector<u32> idx(n);
    u64 p = 1;
    for (u32 j = 0; j < n / 2; ++j) {
        idx[j] = (u32)((p - 1) / 2);
        idx[n / 2 + j] = (u32)((2 * (u64)n - p - 1) / 2);
        p = p * 3 % (2 * (u64)n);
    }
    return idx;
}
}  // namespace

extern "C" int fhe_batch_encode(uint32_t n, uint64_t t, const uint64_t *slots, uint64_t count, uint64_t *plain) {
    if (!slots || !plain) return fail(FHE_ERR_PARAM, "null argument");
    const u64 zeta = batch_root(n, t);
    if (!zeta) return FHE_ERR_PARAM;
    for (u64 i = 0; i < count * n; ++i)
        if (slots[i] >= t) return fail(FHE_ERR_PARAM, "slot %llu of plaintext %llu holds %llu >= t", (unsigned long long)(i % n), (unsigned long long)(i / n), (unsigned long long)slots[i]);
    const std::vector<u32> idx = slot_index(n);
    const u64 izeta = hostmath::invmod(zeta, t), iw = hostmath::mulmod(izeta, izeta, t), ninv = hostmath::invmod(n, t);
    std::vector<u64> a(n);
    for (u64 p = 0; p < count; ++p) {
        for (u32 j = 0; j < n; ++j) a[idx[j]] = slots[p * n + j];
        cyclic_ntt(a, iw, t);                                        // n m_c zeta^c = sum_i A_i (zeta^-2)^(c i)
        u64 f = ninv;
        for (u32 c = 0; c < n; ++c) {
            plain[p * n + c] = hostmath::mulmod(a[c], f, t);
            f = hostmath::mulmod(f, izeta, t);
        }
    }
    return FHE_OK;
}

extern "C" int fhe_batch_decode(uint32_t n, uint64_t t, const uint64_t *plain, uint64_t count, uint64_t *slots) {
    if (!slots || !plain) return fail(FHE_ERR_PARAM, "null argument");
    const u64 zeta = batch_root(n, t);
    if (!zeta) return FHE_ERR_PARAM;
    for (u64 i = 0; i < count * n; ++i)
        if (plain[i] >= t) return fail(FHE_ERR_PARAM, "coefficient %llu of plaintext %llu holds %llu >= t", (unsigned long long)(i % n), (unsigned long long)(i / n), (unsigned long long)plain[i]);
    const std::vector<u32> idx = slot_index(n);
    const u64 w = hostmath::mulmod(zeta, zeta, t);
    std::vector<u64> a(n);
    for (u64 p = 0; p < count; ++p) {
        u64 f = 1;
        for (u32 c = 0; c < n; ++c) {
            a[c] = hostmath::mulmod(plain[p * n + c], f, t);
            f = hostmath::mulmod(f, zeta, t);
        }
        cyclic_ntt(a, w, t);
        for (u32 j = 0; j < n; ++j) slots[p * n + j] = a[idx[j]];
    }
    return FHE_OK;
}
