// modswitch.hip -- fhe_mod_switch: BFV modulus switching on gfx950; drops the last primes of the RNS base of every polynomial.
// include/fhe_hip.h states the operation; fhe_ctx_create_level (fhe_hip.hip) makes the context the result lives in.
//
// One drop removes the last prime p = q_m of a base q_0 .. q_m.  Per coefficient, with c the canonical representative in [0, q), h = floor(p / 2):
//     c' = floor((c + h) / p) mod (q / p)
// which in residues, with r = (c_m + h) mod p, is for every i < m
//     c'_i = (c_i + (h mod q_i) - (r mod q_i)) * p^-1 mod q_i
// (SEAL 3.x divide_and_round_q_last).  fhe_mod_switch to k_out applies it k - k_out times, last prime first: the iteration is the definition.
//
// k_mod_switch<K_IN, K_OUT, LAZY>: one thread owns two adjacent coefficients of one polynomial (16-byte accesses, as k_eltwise), loads their
// K_IN residues, runs the drops in registers and stores K_OUT words per coefficient: one launch, each input word read once, each output
// word written once.  K_IN and K_OUT are template arguments so that every register array has constant indices (28 pairs, nothing in scratch)
// and every constant is a scalar load from the kernel-argument segment at a fixed offset.
//
// Arithmetic.  The bases may mix prime sizes (a 61-bit prime dropped over a 36-bit one): r is NOT below 2 q_i.  The host folds the subtraction
// into one unsigned addend per pair: A = (h mod q_i) + M with M the smallest multiple of q_i that is >= p, so that
//     x = c_i + A - r        is >= 0, below c_i + 2 q_i + p, and = c_i + h - r (mod q_i)
// and the Shoup product x * p^-1 mod q_i takes any 64-bit x: one product per (drop, kept prime), k (k - 1) / 2 = 28 at 8 -> 1.
// Canonical (LAZY = false; a 61-bit prime in the base, or FHE_NTT_NOPM): mul_shoup, x < 3 * 2^61.  LAZY (packed_arith.h lazy_ok: primes of at
// most 58 bits): mul_shoup_lazy4 leaves c_i in [0, 4 q_i) between drops -- x < 4 q_i + 2 q_i + p < 2^61 -- and a residue is made canonical
// exactly once: before it is the dropped prime (r needs c_m in [0, p)), or before the store.
#include "packed_arith.h"
#include "host_math.h"

namespace {

template <int K_IN, int K_OUT, bool LAZY>
__global__ __launch_bounds__(256) void k_mod_switch(const ulonglong2 *__restrict__ in, ulonglong2 *__restrict__ out, ModSwitchTab T, u32 half_n, u64 n_polys) {
    static_assert(1 <= K_OUT && K_OUT < K_IN && K_IN <= FHE_MAX_K, "drops at least one prime, keeps at least one");
    const u32 j = blockIdx.x * 256 + threadIdx.x;
    if (j >= half_n) return;
    const u32 zero = LAZY ? fhe_opaque_zero : 0;
    const u64 p = (u64)blockIdx.z * gridDim.y + blockIdx.y;          // one polynomial per workgroup row: a loop over polynomials keeps all 28 pairs live across it
    if (p < n_polys) {
        const ulonglong2 *src = in + p * K_IN * half_n + j;
        u64 a[K_IN], b[K_IN];                                        // the two coefficients' residues
#pragma unroll
        for (int i = 0; i < K_IN; i++) {
            const ulonglong2 v = src[(u64)i * half_n];
            a[i] = v.x;
            b[i] = v.y;
        }
#pragma unroll
        for (int m = K_IN - 1; m >= K_OUT; m--) {
            const u64 pm = T.q[m], h = pm >> 1;
            if (LAZY && m < K_IN - 1) {
                a[m] = csub(csub(a[m], 2 * pm), pm);
                b[m] = csub(csub(b[m], 2 * pm), pm);
            }
            const u64 ra = csub(a[m] + h, pm), rb = csub(b[m] + h, pm);
#pragma unroll
            for (int i = 0; i < m; i++) {
                const int e = m * (m - 1) / 2 + i;
                const u64 xa = a[i] + T.add[e] - ra, xb = b[i] + T.add[e] - rb;
                if constexpr (LAZY) {
                    a[i] = mul_shoup_lazy4(xa, T.inv[e].x, T.inv[e].y, 0 - T.q[i], zero);
                    b[i] = mul_shoup_lazy4(xb, T.inv[e].x, T.inv[e].y, 0 - T.q[i], zero);
                } else {
                    a[i] = mul_shoup(xa, T.inv[e].x, T.inv[e].y, T.q[i]);
                    b[i] = mul_shoup(xb, T.inv[e].x, T.inv[e].y, T.q[i]);
                }
            }
        }
        ulonglong2 *dst = out + p * K_OUT * half_n + j;
#pragma unroll
        for (int i = 0; i < K_OUT; i++) {
            const u64 qi = T.q[i];
            dst[(u64)i * half_n] = LAZY ? make_ulonglong2(csub(csub(a[i], 2 * qi), qi), csub(csub(b[i], 2 * qi), qi)) : make_ulonglong2(a[i], b[i]);
        }
    }
}

template <int K_IN, int K_OUT>
void launch(bool lazy, dim3 grid, hipStream_t st, const ulonglong2 *in, ulonglong2 *out, const ModSwitchTab &T, u32 half_n, u64 n_polys) {
    if (lazy) k_mod_switch<K_IN, K_OUT, true><<<grid, 256, 0, st>>>(in, out, T, half_n, n_polys);
    else k_mod_switch<K_IN, K_OUT, false><<<grid, 256, 0, st>>>(in, out, T, half_n, n_polys);
}
template <int K_IN>
void launch_in(u32 k_out, bool lazy, dim3 grid, hipStream_t st, const ulonglong2 *in, ulonglong2 *out, const ModSwitchTab &T, u32 half_n, u64 n_polys) {
#define GO(KO)                                                                              \
    case KO:                                                                                \
        if constexpr (KO < K_IN) launch<K_IN, KO>(lazy, grid, st, in, out, T, half_n, n_polys);   \
        break
    switch (k_out) { GO(1); GO(2); GO(3); GO(4); GO(5); GO(6); GO(7); }
#undef GO
}

}  // namespace

// the per-pair constants of every drop of the context's base, once, on the host (fhe_ctx_create): entry m (m - 1) / 2 + i for q_m dropped over q_i
void fhe_modswitch_build(fhe_ctx *c) {
    ModSwitchTab &T = c->modswitch;
    for (u32 m = 0; m < c->k; m++) T.q[m] = c->qb.primes[m];
    for (u32 m = 1; m < c->k; m++)
        for (u32 i = 0; i < m; i++) {
            const u64 p = T.q[m], qi = T.q[i], inv = hostmath::invmod(p % qi, qi);
            const u32 e = m * (m - 1) / 2 + i;
            T.inv[e] = make_ulonglong2(inv, hostmath::shoup(inv, qi));
            T.add[e] = (p >> 1) % qi + (p + qi - 1) / qi * qi;
        }
}

extern "C" int fhe_mod_switch(const fhe_ctx *c, uint32_t k_out, const uint64_t *in, uint64_t *out, uint64_t n_polys, fhe_stream s) {
    if (!c || !in || !out) return fail(FHE_ERR_PARAM, "null argument");
    if (k_out == 0 || k_out >= c->k) return fail(FHE_ERR_PARAM, "mod_switch: k_out = %u, a context of %u primes switches to 1 .. %u", k_out, c->k, c->k - 1);
    if (!n_polys) return FHE_OK;
    if (n_polys > 32768ull * 65535) return fail(FHE_ERR_PARAM, "n_polys %llu: more polynomials than one grid holds", (unsigned long long)n_polys);
    if (overlap(in, n_polys * c->k * c->n, out, n_polys * k_out * c->n))
        return fail(FHE_ERR_PARAM, "output range overlaps the input range (fhe_mod_switch has no in-place form: the strides differ)");
    const u32 half_n = c->n / 2;
    const bool lazy = lazy_ok(c);
    hipStream_t st = (hipStream_t)s;
    const unsigned gy = (unsigned)(n_polys < 32768 ? n_polys : 32768);
    const dim3 grid((half_n + 255) / 256, gy, (unsigned)((n_polys + gy - 1) / gy));
    auto I = (const ulonglong2 *)in;
    auto O = (ulonglong2 *)out;
#define GO(KI) case KI: launch_in<KI>(k_out, lazy, grid, st, I, O, c->modswitch, half_n, n_polys); break
    switch (c->k) { GO(2); GO(3); GO(4); GO(5); GO(6); GO(7); GO(8); }
#undef GO
    KERNEL_CHECK();
    return FHE_OK;
}
