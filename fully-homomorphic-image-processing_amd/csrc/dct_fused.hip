// dct_fused.hip -- the headline kernels: encrypted_dct + quantize_fhe (homo/fhe_image.h:196-305)
// as two fused launches per wave of blocks, with exact FP64-FMA modular arithmetic.
//
// Why FP64.  gfx950 has no 64-bit integer multiplier; a Shoup modular product costs ~10 quarter/half
// rate 32-bit multiplies (measured 4.6 lane-products/clk/CU, profiles/r01_ubench_*).  For primes
// below 2^48 the same residue can be computed EXACTLY with five double-precision operations
//     h = y*w;  l = fma(y,w,-h);  q = rint(h/p);  r = fma(-q,p,h) + l          (|r| <= p/2 + eps)
// (h+l is the exact 106-bit product, q p is exact, so r is the exact centred remainder), measured
// at 10.1 lane-products/clk/CU.  Values stay integers of magnitude < 2^53 throughout, additions
// need no reduction at all, and the final residues are bit-identical to the u64 path.  This is
// integer modular arithmetic carried by the FP64 FMA pipe, not floating-point approximation.
//
// Dataflow per (block, polynomial j, prime i):
//   kernel A (rows):    for each row: x_m = d_m +- d_(7-m) on coefficients, forward NTT of the
//                       four sums (even half) or differences (odd half), the even/odd part of the
//                       LL&M row pass per NTT slot, store the four row outputs (NTT form; packed to
//                       40 bytes per thread and polynomial for primes <= 37 bits, FP64 otherwise)
//   kernel B (columns): same for columns on the NTT-form intermediates, per-output scale
//                       encode(0.125)*encode(1/quant) folded into one product, inverse NTT, store.
// The public u64 ciphertexts are read and written 16 bytes per lane as well, in the shapes with 8 coefficients per thread
// (n = 2048, 4096, 8192): in the ordinary pass-0 layout a thread owns coefficients r*TP + tid, never two neighbours, but
// pass 0 is column-independent, so the wide kernels (WIDE) carry two neighbouring columns of two polynomials through it
// instead of one column of four -- coefficients r*TP + 2u + {0, 1} of polynomials 2h + {0, 1}, h = tid / (TP/2) -- and
// the exchange between pass 0 and pass 1 converts between the two layouts (exchange_pairs_fwd / _inv).  The arithmetic
// per value is unchanged.  The 8-byte bodies remain: 16 coefficients per thread, n = 1024, k_dct_one_launch, a call
// whose `in` or `out` is only 8-byte aligned (fhe_dct_f64_launch) and FHE_DCT_WIDE_IO=0.
// The private formats are laid out so that the column kernel moves 16 bytes per lane (`buffer_load_dwordx4`,
// 1 KiB contiguous per wave): the packed intermediate as two 16-byte planes of low words and one 8-byte plane of high
// bytes (store_packed), the FP64 intermediate as planes of value pairs, the packed column kernel's constants as tables of
// pairs (k_consts_to_pairs).  Slot ownership, the transforms and every arithmetic operation are those of the 8-byte layout.
// Each workgroup carries 4 polynomials x 2^LE coefficients per thread in registers (n = 4096: LE = 3,
// 512 threads, 64 data VGPRs, two workgroups = four waves per SIMD) and shares every twiddle across
// the four; the even and odd workgroup of a line read the same eight inputs and are placed on the
// same XCD (blockIdx = 16g+u and 16g+8+u) so the second
// read is an L2 hit.  All 832 Evaluator calls of the reference are exact ring operations, so this
// evaluation order yields bit-identical ciphertexts.
#include "internal.h"

#include <cstdlib>

#include "fp64_core.h"

#pragma clang fp contract(off)

namespace {
using namespace fp64;

// Register-pass geometry with 2^LE coefficients per thread (LE = 3: 512 threads per 4096-point
// polynomial, 64 data VGPRs for four polynomials -> 4 waves/SIMD; LE = 4: 256 threads, 128 VGPRs).
template <int L, int LE> struct Shape {
    static constexpr int N = 1 << L, E = 1 << LE, TP = N >> LE, NP = (L + LE - 1) / LE, LDS_WORDS = N + (N >> LE);
};
__host__ __device__ constexpr int g_lo(int L, int LE, int p) { return (L - LE * p - LE) < 0 ? 0 : (L - LE * p - LE); }
__host__ __device__ constexpr int g_stages(int L, int LE, int p) { return (L - LE * p) > LE ? LE : (L - LE * p); }
template <int LO, int LE> __device__ __forceinline__ int g_index(int tid, int r) {
    return ((tid >> LO) << (LO + LE)) | (r << LO) | (tid & ((1 << LO) - 1));
}
template <int LO, int LE> __device__ __forceinline__ int g_pad(int j) { return j + ((j >> (LO + LE)) << LO); }
// paired pass-0 layout (exchange_pairs_fwd): h = tid / (TP/2).  The halves of a workgroup are whole waves, so h is the same
// for every lane of a wave and lives in a scalar register: what depends on it costs scalar instructions only.
template <int TP> __device__ __forceinline__ int pair_half(int tid) { return __builtin_amdgcn_readfirstlane(tid) / (TP / 2); }

// twiddles of one register pass, fetched ahead of use (before the preceding LDS barrier) so that
// their L2 latency is hidden behind the previous pass: 2^(LE-1-rb) values per stage, < 2^LE in all.
template <int L, int LE, int P> struct PassTw {
    static constexpr int LO = g_lo(L, LE, P), S = g_stages(L, LE, P), NTW = (1 << LE) - 1;
    static constexpr int rb(int u) { return (L - 1 - (LE * P + u)) - LO; }
    static constexpr int count(int u) { return 1 << (LE - 1 - rb(u)); }
    static constexpr int offset(int u) { int o = 0; for (int v = 0; v < u; v++) o += count(v); return o; }
};
template <int L, int LE, int P>
__device__ __forceinline__ void load_tw(double (&w)[(1 << LE) - 1], const double *__restrict__ tw, int tid) {
    using T = PassTw<L, LE, P>;
    const int th = (P == 0) ? 0 : (tid >> T::LO);
#pragma unroll
    for (int u = 0; u < T::S; u++) {
#pragma unroll
        for (int i = 0; i < T::count(u); i++) w[T::offset(u) + i] = tw[(1 << (LE * P + u)) + ((th << (LE - 1 - T::rb(u))) | i)];
    }
}

template <int L, int LE, int P, int M>
__device__ __forceinline__ void fwd_pass(double (&x)[M][1 << LE], const double (&w)[(1 << LE) - 1], double p, double pinv) {
    using T = PassTw<L, LE, P>;
    constexpr int E = 1 << LE, KB = (LE == 3) ? 2 : 1;     // butterflies batched per product group
#pragma unroll
    for (int u = 0; u < T::S; u++) {
        const int rb = T::rb(u);
        // enumerate the E/2 butterflies of this stage: index b -> r0 = b with a zero inserted at bit rb
#pragma unroll
        for (int b0 = 0; b0 < E / 2; b0 += KB) {
            double t[KB * M], wm[KB * M];
#pragma unroll
            for (int kb = 0; kb < KB; kb++) {
                const int b = b0 + kb, r0 = ((b >> rb) << (rb + 1)) | (b & ((1 << rb) - 1)), r1 = r0 | (1 << rb);
                const double wv = w[T::offset(u) + (r0 >> (rb + 1))];
#pragma unroll
                for (int m = 0; m < M; m++) { t[kb * M + m] = x[m][r1]; wm[kb * M + m] = wv; }
            }
            mmv<KB * M>(t, wm, p, pinv);
#pragma unroll
            for (int kb = 0; kb < KB; kb++) {
                const int b = b0 + kb, r0 = ((b >> rb) << (rb + 1)) | (b & ((1 << rb) - 1)), r1 = r0 | (1 << rb);
#pragma unroll
                for (int m = 0; m < M; m++) {
                    const double X = x[m][r0];
                    x[m][r0] = X + t[kb * M + m];
                    x[m][r1] = X - t[kb * M + m];
                }
            }
        }
    }
}

template <int L, int LE, int P, int M>
__device__ __forceinline__ void inv_pass(double (&x)[M][1 << LE], const double (&w)[(1 << LE) - 1], double ninv, double p, double pinv) {
    using T = PassTw<L, LE, P>;
    constexpr int E = 1 << LE, KB = (LE == 3) ? 2 : 1;
#pragma unroll
    for (int u = T::S - 1; u >= 0; u--) {
        const int sigma = LE * P + u, rb = T::rb(u);
        if (sigma == 0) {          // last stage of the whole transform: both outputs carry n^-1
#pragma unroll
            for (int b = 0; b < E / 2; b++) {
                const int r0 = ((b >> rb) << (rb + 1)) | (b & ((1 << rb) - 1)), r1 = r0 | (1 << rb);
                const double wv = w[T::offset(u) + (r0 >> (rb + 1))];
                double t[2 * M], wm[2 * M];
#pragma unroll
                for (int m = 0; m < M; m++) {
                    const double X = x[m][r0], Y = x[m][r1];
                    t[m] = X + Y; wm[m] = ninv;
                    t[M + m] = X - Y; wm[M + m] = wv;
                }
                mmv<2 * M>(t, wm, p, pinv);
#pragma unroll
                for (int m = 0; m < M; m++) { x[m][r0] = t[m]; x[m][r1] = t[M + m]; }
            }
        } else {
#pragma unroll
            for (int b0 = 0; b0 < E / 2; b0 += KB) {
                double t[KB * M], wm[KB * M];
#pragma unroll
                for (int kb = 0; kb < KB; kb++) {
                    const int b = b0 + kb, r0 = ((b >> rb) << (rb + 1)) | (b & ((1 << rb) - 1)), r1 = r0 | (1 << rb);
                    const double wv = w[T::offset(u) + (r0 >> (rb + 1))];
#pragma unroll
                    for (int m = 0; m < M; m++) {
                        const double X = x[m][r0], Y = x[m][r1];
                        x[m][r0] = X + Y;
                        t[kb * M + m] = X - Y; wm[kb * M + m] = wv;
                    }
                }
                mmv<KB * M>(t, wm, p, pinv);
#pragma unroll
                for (int kb = 0; kb < KB; kb++) {
                    const int b = b0 + kb, r0 = ((b >> rb) << (rb + 1)) | (b & ((1 << rb) - 1)), r1 = r0 | (1 << rb);
#pragma unroll
                    for (int m = 0; m < M; m++) x[m][r1] = t[kb * M + m];
                }
            }
        }
    }
}

// M polynomials through two alternating LDS buffers: one barrier per polynomial.
// When both layouts keep the wave bits of the thread id (tid >> 6) on the same index bits -- every
// exchange except the one next to pass 0 -- a wave reads only what it wrote itself: no workgroup
// barrier is needed (LDS operations of one wave complete in order), and the eight waves of a
// workgroup are free to drift apart instead of meeting twelve times per transform.
template <int L, int LE, int LO_FROM, int LO_TO, int M>
__device__ __forceinline__ void transpose(double (&x)[M][1 << LE], double *lds, int tid, int &phase) {
    constexpr int PL = imin(LO_FROM, LO_TO), E = 1 << LE;
    constexpr bool WAVE_LOCAL = (Shape<L, LE>::TP <= 64) || (LO_FROM <= 6 && LO_TO <= 6);
#pragma unroll
    for (int m = 0; m < M; m++) {
        double *buf = lds + (phase & 1) * Shape<L, LE>::LDS_WORDS;
        phase++;
#pragma unroll
        for (int r = 0; r < E; r++) buf[g_pad<PL, LE>(g_index<LO_FROM, LE>(tid, r))] = x[m][r];
        if constexpr (WAVE_LOCAL) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        } else {
            __syncthreads();
        }
#pragma unroll
        for (int r = 0; r < E; r++) x[m][r] = buf[g_pad<PL, LE>(g_index<LO_TO, LE>(tid, r))];
    }
}

// The paired pass-0 layout (PAIRED transforms: the wide row and column kernels).  Pass 0 is column-independent and its
// twiddles are the same for every thread, so the 4 x 2^LE values a thread carries through it need not be one column of
// four polynomials: with h = tid / (TP/2), u = tid % (TP/2) a thread holds, for j = 0, 1 and c = 0, 1,
//     x[2j + c][r] = coefficient r*TP + 2u + c of polynomial 2h + j
// -- two neighbouring columns of two polynomials, which it reads from / writes to a public ciphertext 16 bytes at a time.
// The exchange next to pass 0, the one that crosses waves and needs workgroup barriers anyway, converts between this
// and the ordinary pass-1 layout (x[m][r] = coefficient g_index<LO1>(tid, r) of polynomial m) through BOTH buffers at
// once: in step j polynomial j travels through buffer 0 and polynomial 2 + j through buffer 1, so on the paired side
// threads with h = 0 touch buffer 0 and threads with h = 1 buffer 1, 16 bytes per access (the pair is adjacent and 16-byte
// aligned under g_pad<LO1>: the padding is 2^LO1 words every TP).  Three barriers where four transposes have four.
// Hazards.  Step 1 reuses both buffers: one barrier between the steps.  Towards the neighbouring exchange (pass 1 <-> 2)
// there is none when that exchange is wave-local: on the ordinary side a wave touches only words of the region
// [576 w, 576 (w + 1)) that the same wave -- and no other -- uses in the wave-local exchanges, under either padding
// (tests/test_dct_paired_layout.py), and LDS operations of one wave complete in order.  Where the neighbour crosses waves
// itself (n = 8192: LO1 = 7) its last / first access to a buffer is separated from ours by one more barrier.
template <int L, int LE>
__device__ __forceinline__ void exchange_pairs_fwd(double (&x)[4][1 << LE], double *lds, int tid) {
    using SH = Shape<L, LE>;
    constexpr int TP = SH::TP, E = 1 << LE, LO1 = g_lo(L, LE, 1), LO2 = g_lo(L, LE, 2);
    constexpr bool NEIGHBOUR_WAVE_LOCAL = (TP <= 64) || (LO1 <= 6 && LO2 <= 6);
    static_assert(LE == 3 && TP >= 128 && g_lo(L, LE, 0) == LO1 + LE, "paired layout: 8 values per thread, halves of whole waves");
    const int h = pair_half<TP>(tid), u = tid % (TP / 2);
    double *wr = lds + h * SH::LDS_WORDS + 2 * u;                      // + r * (TP + 2^LO1) = g_pad<LO1>(r*TP + 2u)
    const double *rd = lds + g_pad<LO1, LE>(g_index<LO1, LE>(tid, 0));  // + r * 2^LO1
#pragma unroll
    for (int j = 0; j < 2; j++) {
        if (j) __syncthreads();                 // every wave has read step 0
#pragma unroll
        for (int r = 0; r < E; r++) *(double2 *)(wr + r * (TP + (1 << LO1))) = make_double2(x[2 * j][r], x[2 * j + 1][r]);
        __syncthreads();
#pragma unroll
        for (int r = 0; r < E; r++) {
            x[2 * j][r] = rd[r << LO1];                                // polynomial j
            x[2 * j + 1][r] = rd[SH::LDS_WORDS + (r << LO1)];          // polynomial 2 + j
        }
    }
    if constexpr (!NEIGHBOUR_WAVE_LOCAL) __syncthreads();
    // x[0], x[1], x[2], x[3] hold polynomials 0, 2, 1, 3: put them in order (register renaming, the loops are unrolled)
#pragma unroll
    for (int r = 0; r < E; r++) { const double t = x[1][r]; x[1][r] = x[2][r]; x[2][r] = t; }
}
// the mirror image: ordinary pass-1 layout in, paired layout out
template <int L, int LE>
__device__ __forceinline__ void exchange_pairs_inv(double (&x)[4][1 << LE], double *lds, int tid) {
    using SH = Shape<L, LE>;
    constexpr int TP = SH::TP, E = 1 << LE, LO1 = g_lo(L, LE, 1), LO2 = g_lo(L, LE, 2);
    constexpr bool NEIGHBOUR_WAVE_LOCAL = (TP <= 64) || (LO1 <= 6 && LO2 <= 6);
    static_assert(LE == 3 && TP >= 128 && g_lo(L, LE, 0) == LO1 + LE, "paired layout: 8 values per thread, halves of whole waves");
    const int h = pair_half<TP>(tid), u = tid % (TP / 2);
    double *wr = lds + g_pad<LO1, LE>(g_index<LO1, LE>(tid, 0));
    const double *rd = lds + h * SH::LDS_WORDS + 2 * u;
    if constexpr (!NEIGHBOUR_WAVE_LOCAL) __syncthreads();
#pragma unroll
    for (int r = 0; r < E; r++) { const double t = x[1][r]; x[1][r] = x[2][r]; x[2][r] = t; }      // polynomials 0, 2, 1, 3
#pragma unroll
    for (int j = 0; j < 2; j++) {
        if (j) __syncthreads();
#pragma unroll
        for (int r = 0; r < E; r++) {
            wr[r << LO1] = x[2 * j][r];                                // polynomial j
            wr[SH::LDS_WORDS + (r << LO1)] = x[2 * j + 1][r];          // polynomial 2 + j
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < E; r++) {
            const double2 v = *(const double2 *)(rd + r * (TP + (1 << LO1)));
            x[2 * j][r] = v.x;
            x[2 * j + 1][r] = v.y;
        }
    }
}

// forward transform; `w` holds the pass-0 twiddles on entry.  `pre()` is invoked once, right
// before the last transpose, so that the caller can start fetching what it needs after the NTT.
// PAIRED: x enters in the paired pass-0 layout (exchange_pairs_fwd) and leaves in the ordinary last-pass layout.
template <int L, int LE, int M, bool PAIRED = false, typename PRE, int P = 0>
__device__ __forceinline__ void ntt_fwd(double (&x)[M][1 << LE], double (&w)[(1 << LE) - 1], const double *__restrict__ tw, double p, double pinv,
                                        double *lds, int tid, int &phase, PRE pre) {
    if constexpr (P + 1 < Shape<L, LE>::NP) {
        double wn[(1 << LE) - 1];
        if (LE >= 4) load_tw<L, LE, P + 1>(wn, tw, tid);   // in flight during this pass and the transpose
        fwd_pass<L, LE, P, M>(x, w, p, pinv);
        if (LE < 4) load_tw<L, LE, P + 1>(wn, tw, tid);    // four waves/SIMD: the transpose alone hides it
        if constexpr (P + 2 == Shape<L, LE>::NP) pre();
        if constexpr (PAIRED && P == 0) exchange_pairs_fwd<L, LE>(x, lds, tid);
        else transpose<L, LE, g_lo(L, LE, P), g_lo(L, LE, P + 1), M>(x, lds, tid, phase);
        ntt_fwd<L, LE, M, PAIRED, PRE, P + 1>(x, wn, tw, p, pinv, lds, tid, phase, pre);
    } else {
        fwd_pass<L, LE, P, M>(x, w, p, pinv);
    }
}
// PAIRED: x enters in the ordinary last-pass layout and leaves in the paired pass-0 layout (exchange_pairs_inv).
template <int L, int LE, int M, bool BIG, bool PAIRED = false, int P = Shape<L, LE>::NP - 1>
__device__ __forceinline__ void ntt_inv(double (&x)[M][1 << LE], double (&w)[(1 << LE) - 1], const double *__restrict__ itw, double p, double pinv,
                                        double *lds, int tid, int &phase) {
    if constexpr (P > 0) {
        double wn[(1 << LE) - 1];
        if (LE >= 4) load_tw<L, LE, P - 1>(wn, itw, tid);
        inv_pass<L, LE, P, M>(x, w, 0.0, p, pinv);
        if (LE < 4) load_tw<L, LE, P - 1>(wn, itw, tid);
        if constexpr (BIG) {
#pragma unroll
            for (int m = 0; m < M; m++)
#pragma unroll
                for (int r = 0; r < (1 << LE); r++) x[m][r] = red(x[m][r], p, pinv);
        }
        if constexpr (PAIRED && P == 1) exchange_pairs_inv<L, LE>(x, lds, tid);
        else transpose<L, LE, g_lo(L, LE, P), g_lo(L, LE, P - 1), M>(x, lds, tid, phase);
        ntt_inv<L, LE, M, BIG, PAIRED, P - 1>(x, wn, itw, p, pinv, lds, tid, phase);
    } else {
        inv_pass<L, LE, P, M>(x, w, itw[0], p, pinv);
    }
}

// Packed intermediate (primes <= 37 bits): a row output is an integer |v| < 2^39, so it travels as
// its low 32 bits plus one signed high byte -- 40 bytes per thread and polynomial instead of 64.
// t = v + (2^52 + 2^51) has bits(t) = (0x43380000 + floor(v / 2^32)) : (v mod 2^32), so packing is one
// FP64 add and byte picks, unpacking (cols_body) rebuilds t from (low word, 0x43380000 + sign-extended byte:
// one `v_add_u32_sdwa`), and the column kernel's first butterfly works on the biased values directly:
//   t_a - t_b = a - b,   t_a + (t_b - 2 (2^52 + 2^51)) = a + b
// (all exact: every operand and result is an integer below 2^53).
// Layout of a thread's 40 bytes per polynomial (a private format; TP threads): low words 0..3 at tid * 16, low words
// 4..7 at TP * 16 + tid * 16, the eight high bytes at 2 * TP * 16 + tid * 8 -- so the column kernel fetches a polynomial
// with two 16-byte loads and one 8-byte load (a wave reads 1 KiB contiguously per 16-byte load).
constexpr double PACK_BIAS = 6755399441055744.0;
// `ob` is the workgroup's uniform base, `vo` the thread's byte offset tid * 8 and `so` the uniform byte offset.  This one
// access keeps a plain pointer and 8-byte stores (hipcc merges some of them): with buffer stores, or with the four low words
// of a plane gathered for one 16-byte store, hipcc spills 39-58 VGPRs of the row kernel in every arrangement tried
// (profiles/EXPERIMENTS.md sections 15 and 19), this form none.
template <int E, int TP>
__device__ __forceinline__ void store_packed(char *__restrict__ ob, u32 vo, u32 so, const double (&x)[E]) {
    static_assert(E == 8, "packed layout is defined for 8 values per thread");
    u32 lo[8], hi[8];
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const double t = x[r] + PACK_BIAS;
        lo[r] = (u32)__double2loint(t);
        hi[r] = (u32)__double2hiint(t);
    }
    u32 h[2];
#pragma unroll
    for (int g = 0; g < 2; g++) {
        const u32 p01 = __builtin_amdgcn_perm(hi[4 * g + 1], hi[4 * g + 0], 0x0c0c0400u);
        const u32 p23 = __builtin_amdgcn_perm(hi[4 * g + 3], hi[4 * g + 2], 0x0c0c0400u);
        h[g] = __builtin_amdgcn_perm(p23, p01, 0x05040100u);
    }
#pragma unroll
    for (int q = 0; q < 4; q++) *(u64 *)(ob + (size_t)(so + (q >> 1) * TP * 16 + (q & 1) * 8) + 2 * vo) = (u64)lo[2 * q] | ((u64)lo[2 * q + 1] << 32);
    *(u64 *)(ob + (size_t)(so + 4 * TP * 8) + vo) = (u64)h[0] | ((u64)h[1] << 32);
}
// Circuit constants through LDS (gfx950 `buffer_load_dwordx4 ... lds`): the per-slot constants of a wave -- NT tables x 64
// doubles -- are brought straight from L2 into that wave's own LDS region without passing through VGPRs, one slot
// ahead (two regions per wave, used alternately): the request for slot r+1 is issued before slot r is evaluated, so
// the L2 round trip that each of the eight per-slot rounds used to expose runs behind the products of the current
// slot, and no prefetch registers are needed (the 128-VGPR budget is what defeated every register prefetch,
// DESIGN.md 5c).  Requests of one wave complete in order, so `s_waitcnt vmcnt(<requests of slot r+1>)` means slot r
// has landed; the waits are written by hand (hipcc does not order a ds_read behind an LDS-DMA request).
// One instruction moves 1 KiB: lanes 0..31 fetch the wave's 64 values (two per lane) of table i, lanes 32..63 those of
// table i+1; LDS destination = M0 base + 16 * lane, i.e. table i at doubles [0, 64), table i+1 at [64, 128).
// (A divergent `if (lane < 32)` for an odd last table would split the basic block, and hipcc then sinks the slots'
// arithmetic below all eight fetches: 351 spilled VGPRs.)
typedef __attribute__((address_space(3))) void lc_lptr;
// `w` is the window of this prime's tables from table FIRST (gwin, fp64_core.h), `soff` the slot's uniform byte offset,
// `voff` the lane's: `buffer_load_dwordx4 ... lds` takes the three as they are, so the eight slots' addresses never
// occupy VGPRs (the flat form held a 64-bit pair per request and spilled some of them).
template <int NT>
__device__ __forceinline__ void stage_consts(gwin_t w, u32 voff, u32 soff, u32 cstride_bytes, double *stg) {
#pragma unroll
    for (int i0 = 0; i0 < NT; i0 += 2) {
        const int i = (i0 + 1 < NT) ? i0 : NT - 2;      // odd count: the last instruction fetches tables NT-2 (again) and NT-1 --
        // no divergent branch, no spare table, no extra LDS
        __builtin_amdgcn_raw_ptr_buffer_load_lds(w, (lc_lptr *)(stg + i * 64), 16, voff, soff + (u32)i * cstride_bytes, 0, 0);
    }
}

// WIDE: the public inputs 16 bytes per lane, in the paired pass-0 layout (exchange_pairs_fwd); `in` must be 16-byte aligned
template <int L, int LE, bool BIG, int HALF, bool PACK, bool LDSC, bool WIDE = false>
__device__ __forceinline__ void rows_body(const u64 *__restrict__ in, double *__restrict__ mid, const double *__restrict__ consts,
                                          const double *__restrict__ tw, const Work &wk, double p, double pinv, u32 k, double *lds) {
    using SH = Shape<L, LE>;
    constexpr int N = SH::N, TP = SH::TP, E = SH::E, NC = HalfC<HALF>::NC, FIRST = HalfC<HALF>::FIRST;
    const int tid = threadIdx.x;
    const size_t poly_words = (size_t)k * N, ct_words = 2 * poly_words;
    const size_t base = ((size_t)wk.blk * 64 + 8 * wk.line) * ct_words + (size_t)wk.poly * poly_words + (size_t)wk.prime * N;
    // this workgroup's window of each tensor (gwin, fp64_core.h): eight ciphertexts from `base`; byte offsets inside it
    // are  vo + uniform  and stay below 2^31 (checked by fhe_dct_f64_launch)
    const gwin_t win_in = gwin(in + base), win_mid = gwin(mid + base);
    const u32 vo = (u32)tid * 8u, ctb = (u32)(ct_words * 8);
    double w0[E - 1];
    load_tw<L, LE, 0>(w0, tw, tid);
    double x[4][E];
    // d_m + d_(7-m) in integers (inputs are < 2^47), then one exact move to double; d_m - d_(7-m) as the difference
    // of the two biased doubles.  Two line pairs are kept in flight; the compiler fences stop it from hoisting every
    // load to the top.
    u64 ra[2][E], rb[2][E];
    auto issue = [&](int m) {
#pragma unroll
        for (int r = 0; r < E; r++) {       // pass-0 mapping: coefficient r*TP + tid
            ra[m & 1][r] = gld_u64(win_in, vo, (u32)m * ctb + r * TP * 8);
            rb[m & 1][r] = gld_u64(win_in, vo, (u32)(7 - m) * ctb + r * TP * 8);
        }
    };
    auto combine = [&](int m) {
#pragma unroll
        for (int r = 0; r < E; r++) {
            const u64 A = ra[m & 1][r], B = rb[m & 1][r];
            x[m][r] = HALF ? u52_biased(A) - u52_biased(B) : u52_to_f64(A + B);
        }
    };
    if constexpr (WIDE) {
        // paired pass-0 mapping: polynomial 2h + j (= d_(2h+j) +- d_(7-2h-j)), coefficients r*TP + 2u + {0, 1}.  The two
        // ciphertext offsets that depend on h are wave-uniform (pair_half); a wave reads 1 KiB contiguously per instruction.
        // Staging stays at 32 VGPRs, and three groups of eight requests are in flight before the first wait instead of one
        // (in this phase x[][] is not live yet, so its own registers receive half of the loads; profiles/EXPERIMENTS.md 24).
        const u32 h = (u32)pair_half<TP>(tid), vw = 16u * ((u32)tid % (TP / 2));
        const u32 soa = h ? 2u * ctb : 0u, sob = h ? 4u * ctb : 6u * ctb;
        // Request i = j * E + r is the pair of row r: qa -> x[2j][r], x[2j+1][r].  The two doubles formed from a pair take the
        // four registers its `a` side arrived in, so all 2E `a` requests cost what x costs anyway; the `b` side goes
        // through a ring of E quadruples.  Order a0 b0 .. a(E-1) b(E-1) a(E) .. a(2E-1): 3E requests before the first wait.
        u64x2 qa[2 * E], qb[E];
        auto lda = [&](int i) { return gld_u64x2(win_in, vw, soa + (u32)(i / E) * ctb + (i % E) * TP * 8); };
        auto ldb = [&](int i) { return gld_u64x2(win_in, vw, sob + (u32)(1 - i / E) * ctb + (i % E) * TP * 8); };
#pragma unroll
        for (int i = 0; i < E; i++) {
            qa[i] = lda(i);
            qb[i] = ldb(i);
        }
#pragma unroll
        for (int i = E; i < 2 * E; i++) qa[i] = lda(i);
#pragma unroll
        for (int i = 0; i < 2 * E; i++) {
            const u64x2 a = qa[i], b = qb[i % E];
            double &xa = x[2 * (i / E)][i % E], &xb = x[2 * (i / E) + 1][i % E];
            xa = HALF ? u52_biased(a.a) - u52_biased(b.a) : u52_to_f64(a.a + b.a);
            xb = HALF ? u52_biased(a.b) - u52_biased(b.b) : u52_to_f64(a.b + b.b);
            // the pair is consumed here, so it is formed (and its ring slot free) before b(E+i) is requested into that
            // slot: a bare fence keeps the loads in order but lets hipcc sink every combine below them
            asm volatile("" ::"v"(xa), "v"(xb) : "memory");
            if (i < E) qb[i] = ldb(E + i);
        }
    } else if constexpr (LE >= 4) {
        issue(0);
        issue(1);
        asm volatile("" ::: "memory");
        combine(0);
        issue(2);
        asm volatile("" ::: "memory");
        combine(1);
        issue(3);
        asm volatile("" ::: "memory");
        combine(2);
        combine(3);
    } else {   // four waves per SIMD hide the round trips; keep the staging registers small
#pragma unroll
        for (int m = 0; m < 4; m++) {
            issue(m);
            combine(m);
            asm volatile("" ::: "memory");
        }
    }
    const size_t cstride = (size_t)k * N;
    const gwin_t win_c = gwin(consts + (size_t)FIRST * cstride + (size_t)wk.prime * N);
    const u32 csb = (u32)(cstride * 8);
    double cn[9];
    auto fetch = [&](int r) {
#pragma unroll
        for (int i = 0; i < NC; i++) cn[i] = gld_f64(win_c, vo, (u32)i * csb + r * TP * 8);
    };
    int phase = 0;
    ntt_fwd<L, LE, 4, WIDE>(x, w0, tw, p, pinv, lds, tid, phase, [&] { if (LE >= 4) fetch(0); });
    // LDSC: two staging buffers of NC x 64 doubles per wave (9 x 512 B x 2 x 8 waves = the two exchange buffers exactly)
    const int lane = tid & 63;
    double *stg = lds + (tid >> 6) * (2 * NC * 64);
    const u32 svoff = (u32)(((size_t)(lane >> 5) * cstride + (tid & ~63) + 2 * (lane & 31)) * sizeof(double));
    constexpr int NDMA = (NC + 1) / 2;      // instructions per slot
    if constexpr (LDSC) {
        // keep the slots' arithmetic below the barrier: hoisted into the last transform pass it costs registers there
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();                    // every wave is done with the exchange buffers
        stage_consts<NC>(win_c, svoff, 0, csb, stg);
    }
#pragma unroll
    for (int r = 0; r < E; r++) {
        double c[9];
        if constexpr (LDSC) {
            // slot r+1 on its way into the other buffer (last read in slot r-1) while slot r is evaluated
            if (r + 1 < E) stage_consts<NC>(win_c, svoff, (r + 1) * TP * 8, csb, stg + ((r + 1) & 1) * NC * 64);
            if (r + 1 < E) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NDMA) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const double *sr = stg + (r & 1) * NC * 64 + lane;
#pragma unroll
            for (int i = 0; i < NC; i++) c[i] = sr[i * 64];
        } else {
        if (LE < 4) fetch(r);               // four waves per SIMD: no software prefetch, fewer registers
#pragma unroll
        for (int i = 0; i < NC; i++) c[i] = cn[i];
        if (LE >= 4 && r + 1 < E) fetch(r + 1);
        }
        line_half<HALF>(x[0][r], x[1][r], x[2][r], x[3][r], c, p, pinv);
        if (BIG) {
#pragma unroll
            for (int m = 0; m < 4; m++) x[m][r] = red(x[m][r], p, pinv);
        } else if (PACK && HALF == 0) {   // outputs 0 and 4 carry no product: bring them below 2^39 too
            x[0][r] = red(x[0][r], p, pinv);
            x[2][r] = red(x[2][r], p, pinv);
        }
        // pin the slot's arithmetic between its own constant reads and the next slot's fetch: without a consumer here
        // hipcc orders all eight fetch / wait / read groups first and the arithmetic after them (constants spilled)
        if constexpr (LDSC) asm volatile("" ::"v"(x[0][r]), "v"(x[1][r]), "v"(x[2][r]), "v"(x[3][r]) : "memory");
    }
#pragma unroll
    for (int m = 0; m < 4; m++) {
        const u32 so = (u32)(2 * m + HALF) * ctb;
        if constexpr (PACK) {
            store_packed<E, TP>((char *)(mid + base), vo, so, x[m]);
        } else {
            // plane j holds values 2j, 2j + 1 of every thread.  16 coefficients per thread: the same layout 8 bytes at a time (the
            // pair of registers a 16-byte store needs costs this register-bound shape 129 spilled VGPRs instead of 91)
            if constexpr (LE >= 4) {
#pragma unroll
                for (int r = 0; r < E; r++) gst_f64(win_mid, 2 * vo, so + (r >> 1) * TP * 16 + (r & 1) * 8, x[m][r]);
            } else {
#pragma unroll
                for (int j = 0; j < E / 2; j++) gst_f64x2(win_mid, 2 * vo, so + j * TP * 16, x[m][2 * j], x[m][2 * j + 1]);
            }
        }
    }
}

// waves per SIMD requested from the register allocator = what LDS lets be resident (at most two workgroups)
__host__ __device__ constexpr int occ_waves(int tp, int lds_words) {
    return ((2 * lds_words * 16 <= 160 * 1024) ? 2 : 1) * tp / 256 < 1 ? 1 : ((2 * lds_words * 16 <= 160 * 1024) ? 2 : 1) * tp / 256;
}
template <int L, int LE> struct Occ { static constexpr int W = occ_waves(Shape<L, LE>::TP, Shape<L, LE>::LDS_WORDS); };

template <int L, int LE, bool BIG, bool PACK, bool LDSC, bool WIDE = false>
__global__ __launch_bounds__((Shape<L, LE>::TP), (Occ<L, LE>::W)) void k_dct_rows(const u64 *__restrict__ in, double *__restrict__ mid,
                                                                  const double *__restrict__ consts, const double *__restrict__ tw_all,
                                                                  const Modulus *__restrict__ mods, u32 k) {
    __shared__ __attribute__((aligned(16))) double lds[2 * Shape<L, LE>::LDS_WORDS];
    const Work wk = decode(blockIdx.x, k);
    const double p = (double)mods[wk.prime].q, pinv = 1.0 / p;
    const double *tw = tw_all + (size_t)wk.prime * Shape<L, LE>::N;
    if (wk.half) rows_body<L, LE, BIG, 1, PACK, LDSC, WIDE>(in, mid, consts, tw, wk, p, pinv, k, lds);
    else rows_body<L, LE, BIG, 0, PACK, LDSC, WIDE>(in, mid, consts, tw, wk, p, pinv, k, lds);
}

// WIDE: the public outputs 16 bytes per lane, in the paired pass-0 layout (exchange_pairs_inv); `out` must be 16-byte aligned
template <int L, int LE, bool BIG, int HALF, bool PACK, bool WIDE = false>
__device__ __forceinline__ void cols_body(const double *__restrict__ mid, u64 *__restrict__ out, const double *__restrict__ consts,
                                          const double *__restrict__ cpairs, const double *__restrict__ itw, const Work &wk, double p, double pinv, u32 k, double *lds) {
    using SH = Shape<L, LE>;
    constexpr int N = SH::N, TP = SH::TP, E = SH::E, NC = HalfC<HALF>::NC, FIRST = HalfC<HALF>::FIRST;
    constexpr int LASTP = SH::NP - 1;
    const int tid = threadIdx.x;
    const size_t poly_words = (size_t)k * N, ct_words = 2 * poly_words;
    const size_t base = ((size_t)wk.blk * 64 + wk.line) * ct_words + (size_t)wk.poly * poly_words + (size_t)wk.prime * N;
    const size_t cstride = (size_t)k * N;
    // windows as in rows_body: a column spans 57 ciphertexts from `base` (rows 8 ciphertexts apart), the constants
    // of this prime 76 tables; all offsets below 2^31 (fhe_dct_f64_launch)
    const gwin_t win_mid = gwin(mid + base), win_out = gwin(out + base);
    // constants.  FP64-intermediate variants: win_c = the half's line constants in the plain table, win_s = the per-output
    // scales (row 2m+HALF, column wk.line -> constant 12 + 8*row + col).  Packed variant: win_c = the half's line pairs in
    // the paired table (k_consts_to_pairs) from its first one, win_s = the two scale pairs of (column, half), win_1 = the last
    // line constant of the half (2 or 11), which has no partner and comes from the plain table.
    const gwin_t win_c = PACK ? gwin(cpairs + 2 * ((size_t)(HALF ? 1 : 0) * cstride + (size_t)wk.prime * N))
                              : gwin(consts + (size_t)FIRST * cstride + (size_t)wk.prime * N);
    const gwin_t win_s = PACK ? gwin(cpairs + 2 * ((size_t)(DCT_NPAIR_LINE + 2 * (2 * wk.line + HALF)) * cstride + (size_t)wk.prime * N))
                              : gwin(consts + (size_t)(12 + 8 * HALF + wk.line) * cstride + (size_t)wk.prime * N);
    const gwin_t win_1 = gwin(consts + (size_t)(FIRST + NC - 1) * cstride + (size_t)wk.prime * N);
    const u32 vo = (u32)tid * 8u, rsb = (u32)(ct_words * 64), csb = (u32)(cstride * 8);     // bytes per row / per table
    const double pbias = p + 4503599627370496.0;
    double cn[9], sn[4];
    auto fetch = [&](int r) {
        if constexpr (PACK) {
#pragma unroll
            for (int i = 0; i < NC / 2; i++) {
                const f64x2 v = gld_f64x2(win_c, 2 * vo, (u32)i * 2 * csb + r * TP * 16);
                cn[2 * i] = v.a;
                cn[2 * i + 1] = v.b;
            }
            cn[NC - 1] = gld_f64(win_1, vo, r * TP * 8);
#pragma unroll
            for (int g = 0; g < 2; g++) {
                const f64x2 v = gld_f64x2(win_s, 2 * vo, (u32)g * 2 * csb + r * TP * 16);
                sn[2 * g] = v.a;
                sn[2 * g + 1] = v.b;
            }
        } else {
#pragma unroll
            for (int i = 0; i < NC; i++) cn[i] = gld_f64(win_c, vo, (u32)i * csb + r * TP * 8);
#pragma unroll
            for (int m = 0; m < 4; m++) sn[m] = gld_f64(win_s, vo, (u32)(16 * m) * csb + r * TP * 8);
        }
    };
    double wl[E - 1];
    if constexpr (!PACK) {           // in flight behind the bulk loads
        fetch(0);
        load_tw<L, LE, LASTP>(wl, itw, tid);
    }
    double x[4][E];
    if constexpr (PACK) {
        // rebuild the biased doubles t = 2^52 + 2^51 + v from (0x43380000 + sign-extended byte : low
        // word) and let the first butterfly remove the bias.  All 80 packed words are requested
        // before the first is used (x is not live yet).
        u32x4 qa[4][2], qb[4][2];
        u64 ha[4], hb[4];
#pragma unroll
        for (int m = 0; m < 4; m++) {
#pragma unroll
            for (int g = 0; g < 2; g++) {
                qa[m][g] = gld_b128(win_mid, 2 * vo, (u32)m * rsb + g * TP * 16);
                qb[m][g] = gld_b128(win_mid, 2 * vo, (u32)(7 - m) * rsb + g * TP * 16);
            }
            ha[m] = gld_u64(win_mid, vo, (u32)m * rsb + 4 * TP * 8);
            hb[m] = gld_u64(win_mid, vo, (u32)(7 - m) * rsb + 4 * TP * 8);
        }
#pragma unroll
        for (int m = 0; m < 4; m++) {
#pragma unroll
            for (int r = 0; r < E; r++) {
                const u32 hwa = (r & 4) ? (u32)(ha[m] >> 32) : (u32)ha[m], hwb = (r & 4) ? (u32)(hb[m] >> 32) : (u32)hb[m];
                const double ta = __hiloint2double((int)(0x43380000u + (u32)(int)(signed char)(hwa >> (8 * (r & 3)))), (int)qa[m][r >> 2][r & 3]);
                const double tb = __hiloint2double((int)(0x43380000u + (u32)(int)(signed char)(hwb >> (8 * (r & 3)))), (int)qb[m][r >> 2][r & 3]);
                x[m][r] = HALF ? ta - tb : ta + (tb - 2.0 * PACK_BIAS);
            }
        }
    } else {
#pragma unroll
        for (int m = 0; m < 4; m++) {
#pragma unroll
            for (int j = 0; j < E / 2; j++) {
                const f64x2 A = gld_f64x2(win_mid, 2 * vo, (u32)m * rsb + j * TP * 16), B = gld_f64x2(win_mid, 2 * vo, (u32)(7 - m) * rsb + j * TP * 16);
                x[m][2 * j] = HALF ? A.a - B.a : A.a + B.a;
                x[m][2 * j + 1] = HALF ? A.b - B.b : A.b + B.b;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < E; r++) {
        double c[9], sc[4];
        if (PACK) fetch(r);
#pragma unroll
        for (int i = 0; i < NC; i++) c[i] = cn[i];
#pragma unroll
        for (int m = 0; m < 4; m++) sc[m] = sn[m];
        if (!PACK && r + 1 < E) fetch(r + 1);
        line_half<HALF>(x[0][r], x[1][r], x[2][r], x[3][r], c, p, pinv);
        double y[4] = {x[0][r], x[1][r], x[2][r], x[3][r]};
        mmv<4>(y, sc, p, pinv);
#pragma unroll
        for (int m = 0; m < 4; m++) x[m][r] = y[m];
    }
    // packed variant: the last pass's twiddles are requested only now -- 14 registers that the slots need for the paired
    // constants (requested before the slots, the kernel spills 4 VGPRs); four waves per SIMD hide the round trip
    if constexpr (PACK) load_tw<L, LE, LASTP>(wl, itw, tid);
    int phase = 0;
    ntt_inv<L, LE, 4, BIG, WIDE>(x, wl, itw, p, pinv, lds, tid, phase);
    if constexpr (WIDE) {
        // paired pass-0 mapping: x[2j + c][r] = coefficient r*TP + 2u + c of output row 2 (2h + j) + HALF; the row offset
        // that depends on h is wave-uniform (pair_half)
        const u32 vw = 16u * ((u32)tid % (TP / 2)), sow = pair_half<TP>(tid) ? 4u * rsb : 0u;
#pragma unroll
        for (int j = 0; j < 2; j++) {
#pragma unroll
            for (int r = 0; r < E; r++)
                gst_u64x2(win_out, vw, sow + (u32)(2 * j + HALF) * rsb + r * TP * 8, f64_to_residue(x[2 * j][r], pbias), f64_to_residue(x[2 * j + 1][r], pbias));
        }
    } else {
#pragma unroll
        for (int m = 0; m < 4; m++) {
#pragma unroll
            for (int r = 0; r < E; r++) gst_u64(win_out, vo, (u32)(2 * m + HALF) * rsb + r * TP * 8, f64_to_residue(x[m][r], pbias));
        }
    }
}

template <int L, int LE, bool BIG, bool PACK, bool WIDE = false>
__global__ __launch_bounds__((Shape<L, LE>::TP), (Occ<L, LE>::W)) void k_dct_cols(const double *__restrict__ mid, u64 *__restrict__ out,
                                                                  const double *__restrict__ consts, const double *__restrict__ cpairs, const double *__restrict__ itw_all,
                                                                  const Modulus *__restrict__ mods, u32 k) {
    __shared__ __attribute__((aligned(16))) double lds[2 * Shape<L, LE>::LDS_WORDS];
    const Work wk = decode(blockIdx.x, k);   // line = column index
    const double p = (double)mods[wk.prime].q, pinv = 1.0 / p;
    const double *itw = itw_all + (size_t)wk.prime * Shape<L, LE>::N;
    if (wk.half) cols_body<L, LE, BIG, 1, PACK, WIDE>(mid, out, consts, cpairs, itw, wk, p, pinv, k, lds);
    else cols_body<L, LE, BIG, 0, PACK, WIDE>(mid, out, consts, cpairs, itw, wk, p, pinv, k, lds);
}

// EXPERIMENT (round 4, FHE_DCT_ONE_LAUNCH=D; off by default): rows and columns in ONE launch.  A unit is (prime, block,
// polynomial): 16 row workgroups write its 1.25 MB packed intermediate, 16 column workgroups read it.  All 32 sit on one
// XCD (blockIdx = 8 * sequence + xcd) and the XCD's sequence alternates [16 row workgroups of unit j + D][16 column
// workgroups of unit j], so a unit's intermediate is consumed D units after it was produced -- while it is still in that
// XCD's L2 / the Infinity Cache -- instead of a whole 256-block wave (3 GiB) later.  Workgroups are dispatched in blockIdx
// order, so the rows a column workgroup waits for were dispatched before it and never wait themselves: no deadlock; the
// wait is a bounded spin on a per-unit arrival counter (release: __threadfence + atomicAdd by every row workgroup;
// acquire: atomic load + __threadfence), and a spin that runs out raises *err instead of hanging the device.
template <int L, int LE>
__global__ __launch_bounds__((Shape<L, LE>::TP), (Occ<L, LE>::W)) void k_dct_one_launch(const u64 *__restrict__ in, double *__restrict__ mid, u64 *__restrict__ out,
                                                                        const double *__restrict__ consts, const double *__restrict__ cpairs, const double *__restrict__ tw_all,
                                                                        const double *__restrict__ itw_all, const Modulus *__restrict__ mods, u32 k,
                                                                        u32 n_blocks, u32 dist, u32 *__restrict__ arrived, u32 *__restrict__ err) {
    __shared__ double lds[2 * Shape<L, LE>::LDS_WORDS];
    const u32 xcd = blockIdx.x & 7, seq = blockIdx.x >> 3, chunk = seq >> 5, r = seq & 31;
    const bool is_row = r < 16;
    const long j = is_row ? (long)chunk : (long)chunk - (long)(dist & 0xffffu);
    const u32 n_units = n_blocks * 2 * k;
    if (j < 0) return;
    const u64 g = (u64)j * 8 + xcd;
    if (g >= n_units) return;
    Work wk;
    wk.prime = (u32)(g / (n_blocks * 2));
    const u32 rem = (u32)(g - (u64)wk.prime * n_blocks * 2);
    wk.blk = rem >> 1;
    wk.poly = rem & 1;
    wk.line = (r & 15) >> 1;
    wk.half = r & 1;
    const double p = (double)mods[wk.prime].q, pinv = 1.0 / p;
    if (is_row) {
        const double *tw = tw_all + (size_t)wk.prime * Shape<L, LE>::N;
        if (wk.half) rows_body<L, LE, false, 1, true, true>(in, mid, consts, tw, wk, p, pinv, k, lds);
        else rows_body<L, LE, false, 0, true, true>(in, mid, consts, tw, wk, p, pinv, k, lds);
        if (dist & 0x10000u) return;                       // timing-only switch of the experiment: no hand-over at all (results invalid)
        __syncthreads();                                   // every thread's stores are issued ...
        if (threadIdx.x == 0) {
            __threadfence();                               // ... and visible device-wide before the unit counts this workgroup
            atomicAdd(arrived + g, 1u);
        }
    } else {
        if (!(dist & 0x10000u) && threadIdx.x == 0) {
            u32 spins = 0;
            while (__hip_atomic_load(arrived + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 16u) {
                __builtin_amdgcn_s_sleep(8);
                if (++spins > (1u << 24)) { atomicExch(err, 1u); break; }
            }
            __threadfence();
        }
        __syncthreads();
        const double *itw = itw_all + (size_t)wk.prime * Shape<L, LE>::N;
        if (wk.half) cols_body<L, LE, false, 1, true>(mid, out, consts, cpairs, itw, wk, p, pinv, k, lds);
        else cols_body<L, LE, false, 0, true>(mid, out, consts, cpairs, itw, wk, p, pinv, k, lds);
    }
}

// Shoup-pair table in the u64 kernels' slot order (16 slots per thread) -> centred doubles in the
// fused kernels' slot order: bit-reversed index j = (t << LE) + r lives at r * (n >> LE) + t.
__global__ void k_consts_to_f64(const ulonglong2 *__restrict__ in, double *__restrict__ out, const Modulus *__restrict__ mods, u32 k, u32 n, u32 le, u32 total) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const u32 pos = i % n, rowbase = i - pos;          // destination position within its [n] row
    const u32 tp = n >> le, r = pos / tp, t = pos % tp;
    const u32 j = (t << le) + r;
    const u32 src = (j & 15) * (n >> 4) + (j >> 4);
    const u64 q = mods[(i / n) % k].q;
    const u64 w = in[rowbase + src].x;
    out[i] = w > q / 2 ? -(double)(q - w) : (double)w;
}

// The column kernel's tables: two constants that a thread uses in the same slot as ONE 16-byte element, [pair table][prime][position]
// of double2, so a lane reads both with one `buffer_load_dwordx4` and a wave 1 KiB contiguously.  Pair tables 0..4 are the line
// constants {0,1} {3,4} {5,6} {7,8} {9,10} (2 and 11 have no partner and stay in the plain table); 5 + 2 (2 col + half) + g holds the
// output scales of column `col`, half `half`: rows (half, 2 + half) for g = 0 and (4 + half, 6 + half) for g = 1.
__global__ void k_consts_to_pairs(const ulonglong2 *__restrict__ in, double *__restrict__ out, const Modulus *__restrict__ mods, u32 k, u32 n, u32 le, u32 total) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const u32 pos = i % n, prime = (i / n) % k, pt = i / (n * k);
    const u32 tp = n >> le, r = pos / tp, t = pos % tp;
    const u32 j = (t << le) + r;
    const u32 src = (j & 15) * (n >> 4) + (j >> 4);
    u32 ca, cb;
    if (pt < DCT_NPAIR_LINE) {
        ca = pt ? 2 * pt + 1 : 0;
        cb = ca + 1;
    } else {
        const u32 u = pt - DCT_NPAIR_LINE, g = u & 1, half = (u >> 1) & 1, col = u >> 2;
        ca = 12 + 8 * (4 * g + half) + col;
        cb = ca + 16;
    }
    const u64 q = mods[prime].q;
    const u64 wa = in[((size_t)ca * k + prime) * n + src].x, wb = in[((size_t)cb * k + prime) * n + src].x;
    out[2 * (size_t)i] = wa > q / 2 ? -(double)(q - wa) : (double)wa;
    out[2 * (size_t)i + 1] = wb > q / 2 ? -(double)(q - wb) : (double)wb;
}

// rgb_to_ycc_fhe (homo/fhe_image.h:310-325) for one residue polynomial of one pixel: three joint
// forward transforms, the nine constant products per slot, three joint inverse transforms, in
// place.  No intermediate leaves the workgroup: global traffic is the compulsory 3 in + 3 out.
template <int L, int LE>
__global__ __launch_bounds__((Shape<L, LE>::TP), (Occ<L, LE>::W)) void k_rgb2ycc_f64(u64 *__restrict__ R, u64 *__restrict__ G, u64 *__restrict__ Bc,
                                                                     const double *__restrict__ consts, const double *__restrict__ tw_all,
                                                                     const double *__restrict__ itw_all, const Modulus *__restrict__ mods,
                                                                     const u64 *__restrict__ yoff, u32 yoff_len, u32 k, u32 group, u64 gstride) {
    using SH = Shape<L, LE>;
    constexpr int N = SH::N, TP = SH::TP, E = SH::E, LASTP = SH::NP - 1;
    __shared__ double lds[2 * SH::LDS_WORDS];
    const int tid = threadIdx.x;
    // prime-major like the DCT kernels: resident workgroups share one prime's tables
    const u32 per_prime = gridDim.x / k;
    const u32 prime = blockIdx.x / per_prime;
    const u32 pp = blockIdx.x - prime * per_prime;           // pixel * 2 + poly
    const u32 poly = pp & 1, pix = pp >> 1;
    const u64 q = mods[prime].q;
    const double p = (double)q, pinv = 1.0 / p;
    const double *tw = tw_all + (size_t)prime * N, *itw = itw_all + (size_t)prime * N;
    // pixel `pix` of a plane: contiguous (group == 0), or `group` pixels every gstride words (the block layout of the
    // ciphertext streams, [block][R G B][64]: fhe_rgb_to_ycc_blocks)
    const size_t pix_off = group ? (size_t)(pix / group) * gstride + (size_t)(pix % group) * 2 * k * N : (size_t)pix * 2 * k * N;
    const size_t off = pix_off + ((size_t)poly * k + prime) * N + tid;
    double w0[E - 1];
    load_tw<L, LE, 0>(w0, tw, tid);
    double x[3][E];
    {
        const u64 *src[3] = {R + off, G + off, Bc + off};
#pragma unroll
        for (int m = 0; m < 3; m++)
#pragma unroll
            for (int r = 0; r < E; r++) x[m][r] = u52_to_f64(src[m][r * TP]);
    }
    int phase = 0;
    ntt_fwd<L, LE, 3>(x, w0, tw, p, pinv, lds, tid, phase, [] {});
    double wl[E - 1];
    load_tw<L, LE, LASTP>(wl, itw, tid);
    const double *cp = consts + (size_t)prime * N + tid;
    const size_t cstride = (size_t)k * N;
#pragma unroll
    for (int r = 0; r < E; r++) {
        double c[9], y[9];
#pragma unroll
        for (int i = 0; i < 9; i++) { c[i] = cp[(size_t)i * cstride + r * TP]; y[i] = x[i % 3][r]; }
        mmv<9>(y, c, p, pinv);
        x[0][r] = y[0] + y[1] + y[2];          // Y  =  0.299 R + 0.587 G + 0.114 B      (- 128 below)
        x[1][r] = y[3] - y[4] + y[5];          // Cb = (-0.168736) R - 0.331264 G + 0.5 B
        x[2][r] = y[6] - y[7] - y[8];          // Cr =  0.5 R - 0.418688 G - 0.081312 B
    }
    ntt_inv<L, LE, 3, false>(x, wl, itw, p, pinv, lds, tid, phase);
    u64 *dst[3] = {R + off, G + off, Bc + off};
#pragma unroll
    for (int m = 0; m < 3; m++)
#pragma unroll
        for (int r = 0; r < E; r++) {
            double v = x[m][r];
            v = v < 0.0 ? v + p : v;
            u64 o = f64_to_u52(v);
            if (m == 0 && poly == 0) {
                const u32 j = (u32)(r * TP + tid);
                if (j < yoff_len) o = submod(o, yoff[(size_t)prime * yoff_len + j], q);
            }
            dst[m][r * TP] = o;
        }
}

// Standalone transforms and multiply_plain on the FP64 machinery, reading and writing the library's
// NTT-form order (the u64 kernels' 16-slots-per-thread order, include/fhe_hip.h layout note):
// bit-reversed index j = (t << LE) + r lives at (j & 15) * (n / 16) + (j >> 4).
// MODE 0: forward NTT; 1: inverse NTT; 2: multiply_plain (NTT, product with the prepared plaintext,
// inverse NTT).  M polynomials of one prime per workgroup share every twiddle.
template <int L, int LE, int M, int MODE>
__global__ __launch_bounds__((Shape<L, LE>::TP), (Occ<L, LE>::W)) void k_poly_f64(const u64 *__restrict__ in, u64 *__restrict__ out,
                                                                  const ulonglong2 *__restrict__ plain, const double *__restrict__ tw_all,
                                                                  const double *__restrict__ itw_all, const Modulus *__restrict__ mods, u32 k) {
    using SH = Shape<L, LE>;
    constexpr int N = SH::N, TP = SH::TP, E = SH::E, LASTP = SH::NP - 1;
    static_assert(LE == 3, "slot-order mapping below is written for 8 values per thread");
    __shared__ double lds[2 * SH::LDS_WORDS];
    const int tid = threadIdx.x;
    const u32 per_prime = gridDim.x / k;
    const u32 prime = blockIdx.x / per_prime;
    const u32 g = blockIdx.x - prime * per_prime;
    const double p = (double)mods[prime].q, pinv = 1.0 / p;
    const double *tw = tw_all + (size_t)prime * N, *itw = itw_all + (size_t)prime * N;
    const int slot0 = ((tid & 1) << 3) * (N >> 4) + (tid >> 1);        // + r * (N >> 4)
    double x[M][E];
    int phase = 0;
    if constexpr (MODE != 1) {
        double w0[E - 1];
        load_tw<L, LE, 0>(w0, tw, tid);
#pragma unroll
        for (int m = 0; m < M; m++) {
            const u64 *src = in + ((size_t)(g * M + m) * k + prime) * N + tid;
#pragma unroll
            for (int r = 0; r < E; r++) x[m][r] = u52_to_f64(src[r * TP]);
        }
        ntt_fwd<L, LE, M>(x, w0, tw, p, pinv, lds, tid, phase, [] {});
    } else {
#pragma unroll
        for (int m = 0; m < M; m++) {
            const u64 *src = in + ((size_t)(g * M + m) * k + prime) * N + slot0;
#pragma unroll
            for (int r = 0; r < E; r++) x[m][r] = u52_to_f64(src[r * (N >> 4)]);
        }
    }
    if constexpr (MODE == 0) {
#pragma unroll
        for (int m = 0; m < M; m++) {
            u64 *dst = out + ((size_t)(g * M + m) * k + prime) * N + slot0;
#pragma unroll
            for (int r = 0; r < E; r++) {
                double v = red(x[m][r], p, pinv);
                v = v < 0.0 ? v + p : v;
                dst[r * (N >> 4)] = f64_to_u52(v);
            }
        }
        return;
    }
    double wl[E - 1];
    load_tw<L, LE, LASTP>(wl, itw, tid);
    if constexpr (MODE == 2) {
        const ulonglong2 *pp = plain + (size_t)prime * N + slot0;
#pragma unroll
        for (int r = 0; r < E; r++) {
            const double w = u52_to_f64(pp[r * (N >> 4)].x);
            double y[M], wm[M];
#pragma unroll
            for (int m = 0; m < M; m++) { y[m] = x[m][r]; wm[m] = w; }
            mmv<M>(y, wm, p, pinv);
#pragma unroll
            for (int m = 0; m < M; m++) x[m][r] = y[m];
        }
    }
    ntt_inv<L, LE, M, false>(x, wl, itw, p, pinv, lds, tid, phase);
#pragma unroll
    for (int m = 0; m < M; m++) {
        u64 *dst = out + ((size_t)(g * M + m) * k + prime) * N + tid;
#pragma unroll
        for (int r = 0; r < E; r++) {
            double v = x[m][r];
            v = v < 0.0 ? v + p : v;
            dst[r * TP] = f64_to_u52(v);
        }
    }
}

}  // namespace


// coefficients per thread = 2^LE of the fused pair for this context: 8 (four waves per SIMD) at n = 4096 with primes
// <= 40 bits and at n = 8192 (1024-thread workgroups, one per CU); 16 otherwise
static u32 dct_shape_le(const fhe_ctx *c) {
    if (c->opt.dct_le != 3) return 4;      // coefficients per thread = 2^LE; 3 keeps four waves per SIMD resident
    if (c->logn == 12 && c->max_prime_bits <= 40) return 3;
    if (c->logn == 13 || c->logn == 11) return 3;
    return 4;
}

bool fhe_dct_f64_supported(const fhe_ctx *c) {
    return c && c->qb.d_tw_f64 && c->max_prime_bits <= 47 && (c->logn >= 10 && c->logn <= 13);
}

int fhe_dct_f64_make_consts(const fhe_ctx *c, fhe_dct_plan *plan, hipStream_t st) {
    const u32 total = DCT_NCONST * c->k * c->n, pairs = DCT_NPAIR * c->k * c->n;
    const u32 le = dct_shape_le(c);
    const bool packed = c->max_prime_bits <= 37 && le == 3 && c->opt.dct_pack;      // the contexts launch_pair runs the packed column kernel for
    HIP_TRY(hipMalloc(&plan->d_consts_f64, sizeof(double) * total));
    if (packed) { HIP_TRY(hipMalloc(&plan->d_consts_pair, 2 * sizeof(double) * pairs)); }
    k_consts_to_f64<<<(total + 255) / 256, 256, 0, st>>>(plan->d_consts, plan->d_consts_f64, c->qb.d_mod, c->k, c->n, le, total);
    KERNEL_CHECK();
    if (packed) {
        k_consts_to_pairs<<<(pairs + 255) / 256, 256, 0, st>>>(plan->d_consts, plan->d_consts_pair, c->qb.d_mod, c->k, c->n, le, pairs);
        KERNEL_CHECK();
    }
    return FHE_OK;
}


// row kernel: circuit constants through LDS (stage_consts); FheOptions::dct_ldsc = false reads them into registers as before.
// (The column kernel has four more constants per slot and no register to spare: the same staging spills 36-56 VGPRs
// there and measured 68 k blocks/s against 80 k, so it keeps its loads.)

// The wide kernels (16-byte public accesses, paired pass-0 layout) exist for 8 coefficients per thread and workgroups of at
// least two waves (n = 2048, 4096, 8192); everything else, and a call that does not ask for them, runs the 8-byte bodies.
template <int L, int LE, bool BIG, bool PACK, bool LDSC>
static void launch_rows(bool wide, const fhe_ctx *c, const fhe_dct_plan *plan, const u64 *in, double *mid, unsigned grid, hipStream_t st) {
    constexpr int TP = Shape<L, LE>::TP;
    if constexpr (LE == 3 && TP >= 128 && !(L == 12 && BIG)) {      // n = 4096 takes 16 coefficients per thread above 40 bits
        if (wide) {
            k_dct_rows<L, LE, BIG, PACK, LDSC, true><<<grid, TP, 0, st>>>(in, mid, plan->d_consts_f64, c->qb.d_tw_f64, c->qb.d_mod, c->k);
            return;
        }
    }
    k_dct_rows<L, LE, BIG, PACK, LDSC><<<grid, TP, 0, st>>>(in, mid, plan->d_consts_f64, c->qb.d_tw_f64, c->qb.d_mod, c->k);
}
template <int L, int LE, bool BIG, bool PACK>
static void launch_cols(bool wide, const fhe_ctx *c, const fhe_dct_plan *plan, const double *mid, u64 *out, unsigned grid, hipStream_t st) {
    constexpr int TP = Shape<L, LE>::TP;
    if constexpr (LE == 3 && TP >= 128 && !(L == 12 && BIG)) {      // n = 4096 takes 16 coefficients per thread above 40 bits
        if (wide) {
            k_dct_cols<L, LE, BIG, PACK, true><<<grid, TP, 0, st>>>(mid, out, plan->d_consts_f64, plan->d_consts_pair, c->qb.d_itw_f64, c->qb.d_mod, c->k);
            return;
        }
    }
    k_dct_cols<L, LE, BIG, PACK><<<grid, TP, 0, st>>>(mid, out, plan->d_consts_f64, plan->d_consts_pair, c->qb.d_itw_f64, c->qb.d_mod, c->k);
}

// wide_in / wide_out: run the wide row / column kernel where the shape has one
template <int L, int LE>
static void launch_pair(const fhe_ctx *c, const fhe_dct_plan *plan, const u64 *in, u64 *out, double *mid, unsigned grid, bool big, hipStream_t st, int which,
                        bool wide_in, bool wide_out) {
    if (big) {
        if (which & 1) launch_rows<L, LE, true, false, false>(wide_in, c, plan, in, mid, grid, st);
        if (which & 2) launch_cols<L, LE, true, false>(wide_out, c, plan, mid, out, grid, st);
        return;
    }
    if constexpr (LE == 3) {
        if (c->max_prime_bits <= 37 && c->opt.dct_pack) {      // packed intermediate, 40 instead of 64 bytes
            if (which & 1) {
                if (c->opt.dct_ldsc) launch_rows<L, LE, false, true, true>(wide_in, c, plan, in, mid, grid, st);
                else launch_rows<L, LE, false, true, false>(wide_in, c, plan, in, mid, grid, st);
            }
            if (which & 2) launch_cols<L, LE, false, true>(wide_out, c, plan, mid, out, grid, st);
            return;
        }
    }
    if (which & 1) launch_rows<L, LE, false, false, false>(wide_in, c, plan, in, mid, grid, st);
    if (which & 2) launch_cols<L, LE, false, false>(wide_out, c, plan, mid, out, grid, st);
}

int fhe_dct_f64_launch(const fhe_ctx *c, const fhe_dct_plan *plan, const u64 *in, u64 *out, u64 n_blocks, double *mid, hipStream_t st, int which) {
    const u64 items = n_blocks * 8 * 2 * c->k;   // (block, line, poly, prime), multiple of 8
    const u64 grid = items * 2;
    if (grid > 0x7fffffffULL) return fail(FHE_ERR_PARAM, "too many blocks for one launch");
    // the kernels address each tensor through 32-bit byte offsets inside a per-workgroup window (gwin): at most one
    // block of 64 ciphertexts (2 k n words each) or the 76 constant tables (k n doubles each) -- both below 2^31 bytes
    // for k n < 2^21, far beyond any context this path accepts (n <= 8192)
    if ((u64)c->k * c->n >= (1ULL << 21)) return fail(FHE_ERR_PARAM, "fused FP64 path: a block of ciphertexts exceeds the 2 GiB addressing window");
    const bool big = c->max_prime_bits > 40;
    // the packed column kernel reads the paired tables: a plan without them (made for a context with FHE_DCT_PACK=0) is refused
    if (!big && dct_shape_le(c) == 3 && c->max_prime_bits <= 37 && c->opt.dct_pack && !plan->d_consts_pair)
        return fail(FHE_ERR_PARAM, "fused FP64 path: the plan has no paired constant tables (it was created for a context without the packed intermediate)");
    if (c->opt.dct_one_launch && which == 3 && c->logn == 12 && dct_shape_le(c) == 3 && c->max_prime_bits <= 37 && c->opt.dct_pack && c->d_arrived) {
        const u64 n_units = n_blocks * 2 * c->k;
        if (n_units > c->arrived_cap) return fail(FHE_ERR_PARAM, "one-launch experiment: wave too large for the arrival counters");
        HIP_TRY(hipMemsetAsync(c->d_arrived, 0, (n_units + 1) * sizeof(u32), st));
        const u32 dist = c->opt.dct_one_launch;
        const u64 chunks = (n_units + 7) / 8 + (dist & 0xffffu);
        k_dct_one_launch<12, 3><<<(unsigned)(chunks * 32 * 8), Shape<12, 3>::TP, 0, st>>>(in, mid, out, plan->d_consts_f64, plan->d_consts_pair, c->qb.d_tw_f64, c->qb.d_itw_f64, c->qb.d_mod,
                                                                                       c->k, (u32)n_blocks, dist, c->d_arrived + 1, c->d_arrived);
        KERNEL_CHECK();
        // EXPERIMENT path (FHE_DCT_ONE_LAUNCH; profiles/EXPERIMENTS.md section 1; never a default, never in a parity path other than its
        // own test): a column workgroup that gives up waiting for its rows sets d_arrived[0] and goes on with an incomplete
        // intermediate, so the flag is read back before the call reports success.  That makes this path synchronous -- acceptable
        // for a measurement switch, and the only way the caller cannot receive a silently wrong result.  (The no-deadlock argument
        // also rests on workgroups being dispatched in blockIdx order, which HIP does not promise: one more reason it stays off.)
        u32 timed_out = 0;
        HIP_TRY(hipMemcpyAsync(&timed_out, c->d_arrived, sizeof(u32), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (timed_out) return fail(FHE_ERR_HIP, "one-launch experiment: a column workgroup timed out waiting for its row transforms; the output is incomplete");
        return FHE_OK;
    }
    // the wide kernels move 16 bytes per lane to and from the public ciphertexts, and every offset inside a block is a multiple
    // of 16: they need `in` and `out` on 16-byte boundaries.  The C ABI promises 8, so a call with either pointer only 8-byte
    // aligned runs the 8-byte kernels -- it is neither refused nor run wide.  FHE_DCT_WIDE_IO: bit 0 inputs, bit 1 outputs.
    const bool aligned = !(((uintptr_t)in | (uintptr_t)out) & 15);
    const bool wi = aligned && (c->opt.dct_wide_io & 1), wo = aligned && (c->opt.dct_wide_io & 2);
    switch (c->logn) {   // LE = 3 is only built for the headline size
        case 10: launch_pair<10, 4>(c, plan, in, out, mid, (unsigned)grid, big, st, which, wi, wo); break;
        case 11: launch_pair<11, 3>(c, plan, in, out, mid, (unsigned)grid, big, st, which, wi, wo); break;
        case 12: if (dct_shape_le(c) == 3) launch_pair<12, 3>(c, plan, in, out, mid, (unsigned)grid, false, st, which, wi, wo); else launch_pair<12, 4>(c, plan, in, out, mid, (unsigned)grid, big, st, which, wi, wo); break;
        case 13: if (dct_shape_le(c) == 3) launch_pair<13, 3>(c, plan, in, out, mid, (unsigned)grid, big, st, which, wi, wo); else launch_pair<13, 4>(c, plan, in, out, mid, (unsigned)grid, big, st, which, wi, wo); break;
        default: return fail(FHE_ERR_PARAM, "fused FP64 path supports n in {1024, 2048, 4096, 8192}");
    }
    KERNEL_CHECK();
    return FHE_OK;
}

// ------------------------------------------------------------------------------------------------
// rgb_to_ycc_fhe on the FP64 kernels (n = 4096, primes <= 40 bits: the P4096 preset)
// ------------------------------------------------------------------------------------------------
bool fhe_rgb_f64_supported(const fhe_ctx *c) {
    return fhe_dct_f64_supported(c) && c->logn == 12 && c->max_prime_bits <= 40;
}

int fhe_rgb_f64_make_consts(const fhe_ctx *c, const ulonglong2 *d_c, double **out, hipStream_t st) {
    const u32 total = 9 * c->k * c->n;
    HIP_TRY(hipMalloc(out, sizeof(double) * total));
    k_consts_to_f64<<<(total + 255) / 256, 256, 0, st>>>(d_c, *out, c->qb.d_mod, c->k, c->n, 3, total);
    KERNEL_CHECK();
    return FHE_OK;
}

int fhe_rgb_f64_launch(const fhe_ctx *c, u64 *r, u64 *g, u64 *b, u64 count, const double *consts, const u64 *yoff, u32 yoff_len, hipStream_t st, u32 group, u64 gstride) {
    const u64 grid = count * 2 * c->k;
    if (grid > 0x7fffffffULL) return fail(FHE_ERR_PARAM, "too many pixels for one launch");
    k_rgb2ycc_f64<12, 3><<<(unsigned)grid, Shape<12, 3>::TP, 0, st>>>(r, g, b, consts, c->qb.d_tw_f64, c->qb.d_itw_f64, c->qb.d_mod, yoff, yoff_len, c->k, group, gstride);
    KERNEL_CHECK();
    return FHE_OK;
}

// mode 0 forward NTT, 1 inverse NTT, 2 multiply_plain; n_polys RNS polynomials of k residues each
int fhe_poly_f64_launch(int mode, const fhe_ctx *c, const u64 *in, u64 *out, u64 n_polys, const ulonglong2 *plain, hipStream_t st) {
    const u64 grid2 = (n_polys / 2) * c->k, grid1 = n_polys * c->k;
    if (grid1 > 0x7fffffffULL) return fail(FHE_ERR_PARAM, "too many polynomials for one launch");
    constexpr int TP = Shape<12, 3>::TP;
#define LAUNCH_POLY(M, GRID)                                                                                                          \
    switch (mode) {                                                                                                                   \
        case 0: k_poly_f64<12, 3, M, 0><<<(unsigned)(GRID), TP, 0, st>>>(in, out, plain, c->qb.d_tw_f64, c->qb.d_itw_f64, c->qb.d_mod, c->k); break; \
        case 1: k_poly_f64<12, 3, M, 1><<<(unsigned)(GRID), TP, 0, st>>>(in, out, plain, c->qb.d_tw_f64, c->qb.d_itw_f64, c->qb.d_mod, c->k); break; \
        default: k_poly_f64<12, 3, M, 2><<<(unsigned)(GRID), TP, 0, st>>>(in, out, plain, c->qb.d_tw_f64, c->qb.d_itw_f64, c->qb.d_mod, c->k); break; \
    }
    if (n_polys % 2 == 0) { LAUNCH_POLY(2, grid2) } else { LAUNCH_POLY(1, grid1) }
#undef LAUNCH_POLY
    KERNEL_CHECK();
    return FHE_OK;
}

// ------------------------------------------------------------------------------------------------
// The inverse: dequantisation + 8x8 IDCT (fhe_idct8x8_dequant, idct.hip) as the same two fused launches
// ------------------------------------------------------------------------------------------------
// The butterfly of an inverse line sits on the OUTPUT side (out[m] = E[m] + O[m], out[7-m] = E[m] - O[m]; E from the even
// inputs d0 d2 d4 d6, O from the odd ones d1 d3 d5 d7), so the halves split on the inputs:
//   k_idct_rows: the even workgroup of a row takes inputs 0, 2, 4, 6, the odd one 1, 3, 5, 7 (8 apart in blockIdx, one
//                XCD); four joint forward NTTs, per slot the input product (encode(Q[i]) * encode(0.125), folded by the
//                plan) and the half line; E[0..3] / O[0..3] stored in NTT form at ciphertexts 8 row + 0..3 / 8 row + 4..7
//   k_idct_cols: each of the two workgroups of a column forms the column's eight inputs as E +- O while it loads (exact
//                adds in the NTT domain), evaluates the whole line per slot, keeps outputs 0..3 or 4..7 and runs four
//                joint inverse NTTs.
// Bounds (units of p; every product mm(y, w) below has |y| <= 4 p and a centred |w| <= p/2, so |r| <= p/2 + 6 p^2 2^-53 < 0.6 p
// for p < 2^47; red(x) returns |x - round(x / p) p| <= p/2 up to the same kind of term):
//   rows:  after the forward NTT each value is reduced (red: |x| <= p/2); input products < 0.6 p; even part t0, t1 < 1.2 p,
//          t2, t3 < 1.2 p, E < 2.4 p; odd part: up to three products summed after the fourth, O < 2.4 p; both reduced again
//          before the store (|.| <= p/2)
//   cols:  inputs E +- O < p; even part: d2 + d6 < 2 p, t0 < 2 p, t3 < 1.2 p, E' < 3.2 p; odd part: z3 + z4 < 4 p (the
//          largest product operand), O' < 2.4 p; outputs < 5.6 p, reduced before the inverse NTT (|.| <= p/2), whose
//          passes reduce between them for primes above 40 bits as the forward columns do.
// Everything stays far below 2^53: the arithmetic is exact and the residues equal the op-by-op evaluation.
namespace {
using namespace fp64;

// Half of an inverse line on one NTT slot.  HALF 0: v = d0 d2 d4 d6 -> E0..E3 (t10 t11 t12 t13);  HALF 1: v = d1 d3 d5 d7 ->
// O0..O3 (u3 u2 u1 u0 of the specification).  c[] = the twelve line constants at this slot.
template <int HALF>
__device__ __forceinline__ void idct_half(double (&v)[4], const double (&c)[12], double p, double pinv) {
    if constexpr (HALF == 0) {
        double y[3] = {v[1] + v[3], v[3], v[1]};
        const double w[3] = {c[0], c[2], c[1]};
        mmv<3>(y, w, p, pinv);
        const double t2 = y[0] + y[1], t3 = y[0] + y[2], t0 = v[0] + v[2], t1 = v[0] - v[2];
        v[0] = t0 + t3;
        v[1] = t1 + t2;
        v[2] = t1 - t2;
        v[3] = t0 - t3;
    } else {
        const double u0 = v[3], u1 = v[2], u2 = v[1], u3 = v[0];
        const double z1 = u0 + u3, z2 = u1 + u2, z3 = u0 + u2, z4 = u1 + u3;
        double ya[5] = {z3 + z4, u0, u1, u2, u3}, yb[4] = {z1, z2, z3, z4};
        const double wa[5] = {c[3], c[4], c[5], c[6], c[7]}, wb[4] = {c[8], c[9], c[10], c[11]};
        mmv<5>(ya, wa, p, pinv);
        mmv<4>(yb, wb, p, pinv);
        const double z3b = yb[2] + ya[0], z4b = yb[3] + ya[0];
        v[0] = ya[4] + yb[0] + z4b;        // O0 = u3' + z1' + z4'
        v[1] = ya[3] + yb[1] + z3b;        // O1 = u2' + z2' + z3'
        v[2] = ya[2] + yb[1] + z4b;        // O2 = u1' + z2' + z4'
        v[3] = ya[1] + yb[0] + z3b;        // O3 = u0' + z1' + z3'
    }
}

template <int L, int LE, int HALF>
__device__ __forceinline__ void irows_body(const u64 *__restrict__ in, double *__restrict__ mid, const double *__restrict__ consts,
                                           const double *__restrict__ tw, const Work &wk, double p, double pinv, u32 k, double *lds) {
    using SH = Shape<L, LE>;
    constexpr int N = SH::N, TP = SH::TP, E = SH::E;
    const int tid = threadIdx.x;
    const size_t poly_words = (size_t)k * N, ct_words = 2 * poly_words, cstride = (size_t)k * N;
    const size_t base = ((size_t)wk.blk * 64 + 8 * wk.line) * ct_words + (size_t)wk.poly * poly_words + (size_t)wk.prime * N + tid;
    double w0[E - 1];
    load_tw<L, LE, 0>(w0, tw, tid);
    double x[4][E];
#pragma unroll
    for (int m = 0; m < 4; m++) {
        const u64 *a = in + base + (size_t)(2 * m + HALF) * ct_words;
#pragma unroll
        for (int r = 0; r < E; r++) x[m][r] = u52_to_f64(a[r * TP]);
        asm volatile("" ::: "memory");
    }
    int phase = 0;
    ntt_fwd<L, LE, 4>(x, w0, tw, p, pinv, lds, tid, phase, [] {});
    const double *cp = consts + (size_t)wk.prime * N + tid;
#pragma unroll
    for (int r = 0; r < E; r++) {
        double c[12], s[4], v[4];
#pragma unroll
        for (int i = 0; i < 12; i++) c[i] = cp[(size_t)i * cstride + r * TP];
#pragma unroll
        for (int m = 0; m < 4; m++) {
            s[m] = cp[(size_t)(12 + 8 * wk.line + 2 * m + HALF) * cstride + r * TP];
            v[m] = red(x[m][r], p, pinv);
        }
        mmv<4>(v, s, p, pinv);
        idct_half<HALF>(v, c, p, pinv);
#pragma unroll
        for (int m = 0; m < 4; m++) x[m][r] = red(v[m], p, pinv);
    }
#pragma unroll
    for (int m = 0; m < 4; m++) {
        double *o = mid + base + (size_t)(4 * HALF + m) * ct_words;
#pragma unroll
        for (int r = 0; r < E; r++) o[r * TP] = x[m][r];
    }
}

template <int L, int LE>
__global__ __launch_bounds__((Shape<L, LE>::TP), (Occ<L, LE>::W)) void k_idct_rows(const u64 *__restrict__ in, double *__restrict__ mid,
                                                                   const double *__restrict__ consts, const double *__restrict__ tw_all,
                                                                   const Modulus *__restrict__ mods, u32 k) {
    __shared__ double lds[2 * Shape<L, LE>::LDS_WORDS];
    const Work wk = decode(blockIdx.x, k);   // line = row index
    const double p = (double)mods[wk.prime].q, pinv = 1.0 / p;
    const double *tw = tw_all + (size_t)wk.prime * Shape<L, LE>::N;
    if (wk.half) irows_body<L, LE, 1>(in, mid, consts, tw, wk, p, pinv, k, lds);
    else irows_body<L, LE, 0>(in, mid, consts, tw, wk, p, pinv, k, lds);
}

template <int L, int LE, bool BIG, int HALF>
__device__ __forceinline__ void icols_body(const double *__restrict__ mid, u64 *__restrict__ out, const double *__restrict__ consts,
                                           const double *__restrict__ itw, const Work &wk, double p, double pinv, u32 k, double *lds) {
    using SH = Shape<L, LE>;
    constexpr int N = SH::N, TP = SH::TP, E = SH::E, LASTP = SH::NP - 1;
    const int tid = threadIdx.x;
    const size_t poly_words = (size_t)k * N, ct_words = 2 * poly_words, cstride = (size_t)k * N;
    const size_t base = (size_t)wk.blk * 64 * ct_words + (size_t)wk.poly * poly_words + (size_t)wk.prime * N + tid;
    const u32 col = wk.line, m = col < 4 ? col : 7 - col;      // row output `col` = E[m] + O[m] (col < 4) or E[m] - O[m]
    const bool neg = col >= 4;
    const double *cp = consts + (size_t)wk.prime * N + tid;
    double x[4][E];
#pragma unroll
    for (int r = 0; r < E; r++) {
        double d[8], c[12];
#pragma unroll
        for (int rr = 0; rr < 8; rr++) {
            const double A = mid[base + (size_t)(8 * rr + m) * ct_words + r * TP], B = mid[base + (size_t)(8 * rr + 4 + m) * ct_words + r * TP];
            d[rr] = neg ? A - B : A + B;
        }
#pragma unroll
        for (int i = 0; i < 12; i++) c[i] = cp[(size_t)i * cstride + r * TP];
        double ev[4] = {d[0], d[2], d[4], d[6]}, od[4] = {d[1], d[3], d[5], d[7]};
        idct_half<0>(ev, c, p, pinv);
        idct_half<1>(od, c, p, pinv);
#pragma unroll
        for (int j = 0; j < 4; j++) x[j][r] = red(HALF ? ev[3 - j] - od[3 - j] : ev[j] + od[j], p, pinv);
    }
    double wl[E - 1];
    load_tw<L, LE, LASTP>(wl, itw, tid);
    int phase = 0;
    ntt_inv<L, LE, 4, BIG>(x, wl, itw, p, pinv, lds, tid, phase);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        u64 *o = out + base + (size_t)(8 * (4 * HALF + j) + col) * ct_words;
#pragma unroll
        for (int r = 0; r < E; r++) {
            double v = x[j][r];
            v = v < 0.0 ? v + p : v;
            o[r * TP] = f64_to_u52(v);
        }
    }
}

template <int L, int LE, bool BIG>
__global__ __launch_bounds__((Shape<L, LE>::TP), (Occ<L, LE>::W)) void k_idct_cols(const double *__restrict__ mid, u64 *__restrict__ out,
                                                                   const double *__restrict__ consts, const double *__restrict__ itw_all,
                                                                   const Modulus *__restrict__ mods, u32 k) {
    __shared__ double lds[2 * Shape<L, LE>::LDS_WORDS];
    const Work wk = decode(blockIdx.x, k);   // line = column index
    const double p = (double)mods[wk.prime].q, pinv = 1.0 / p;
    const double *itw = itw_all + (size_t)wk.prime * Shape<L, LE>::N;
    if (wk.half) icols_body<L, LE, BIG, 1>(mid, out, consts, itw, wk, p, pinv, k, lds);
    else icols_body<L, LE, BIG, 0>(mid, out, consts, itw, wk, p, pinv, k, lds);
}

template <int L, int LE>
void launch_ipair(const fhe_ctx *c, const double *consts, const u64 *in, u64 *out, double *mid, unsigned grid, bool big, hipStream_t st) {
    constexpr int TP = Shape<L, LE>::TP;
    k_idct_rows<L, LE><<<grid, TP, 0, st>>>(in, mid, consts, c->qb.d_tw_f64, c->qb.d_mod, c->k);
    if (big) k_idct_cols<L, LE, true><<<grid, TP, 0, st>>>(mid, out, consts, c->qb.d_itw_f64, c->qb.d_mod, c->k);
    else k_idct_cols<L, LE, false><<<grid, TP, 0, st>>>(mid, out, consts, c->qb.d_itw_f64, c->qb.d_mod, c->k);
}
}  // namespace

int fhe_idct_f64_make_consts(const fhe_ctx *c, const ulonglong2 *d_consts, double **out, hipStream_t st) {
    const u32 total = DCT_NCONST * c->k * c->n;
    HIP_TRY(hipMalloc(out, sizeof(double) * total));
    k_consts_to_f64<<<(total + 255) / 256, 256, 0, st>>>(d_consts, *out, c->qb.d_mod, c->k, c->n, dct_shape_le(c), total);
    KERNEL_CHECK();
    return FHE_OK;
}

int fhe_idct_f64_launch(const fhe_ctx *c, const double *consts, const u64 *in, u64 *out, u64 n_blocks, double *mid, hipStream_t st) {
    const u64 grid = n_blocks * 8 * 2 * c->k * 2;   // (block, line, poly, prime) x two halves
    if (grid > 0x7fffffffULL) return fail(FHE_ERR_PARAM, "too many blocks for one launch");
    const bool big = c->max_prime_bits > 40;
    switch (c->logn) {   // the forward pair's shapes (dct_shape_le)
        case 10: launch_ipair<10, 4>(c, consts, in, out, mid, (unsigned)grid, big, st); break;
        case 11: launch_ipair<11, 3>(c, consts, in, out, mid, (unsigned)grid, big, st); break;
        case 12: if (dct_shape_le(c) == 3) launch_ipair<12, 3>(c, consts, in, out, mid, (unsigned)grid, big, st); else launch_ipair<12, 4>(c, consts, in, out, mid, (unsigned)grid, big, st); break;
        case 13: if (dct_shape_le(c) == 3) launch_ipair<13, 3>(c, consts, in, out, mid, (unsigned)grid, big, st); else launch_ipair<13, 4>(c, consts, in, out, mid, (unsigned)grid, big, st); break;
        default: return fail(FHE_ERR_PARAM, "fused FP64 path supports n in {1024, 2048, 4096, 8192}");
    }
    KERNEL_CHECK();
    return FHE_OK;
}
