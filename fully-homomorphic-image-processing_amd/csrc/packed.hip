// packed.hip -- integer linear maps ACROSS slot-packed ciphertexts on gfx950: fhe_block8x8_scalar (an 8x8 separable transform of a
// group of 64 ciphertexts: the packed JPEG DCT / IDCT with quantisation) and fhe_channel_mix (a small matrix across planes: the colour
// conversion).  include/fhe_hip.h states the operations.
//
// A scalar weight is the constant polynomial: multiply_plain by it multiplies every residue by w mod q_i -- no transform, no rotation.
// The maps are therefore element-wise in the coefficient index: a thread owns ONE word position (polynomial, prime, coefficient) of all
// 64 ciphertexts of a group, reads its 64 words (lanes run along the coefficient index: 64 coalesced streams), runs the row pass
// (R, with pre folded in front) and the column pass (L, with post behind) and writes its 64 words.  Nothing in between touches global
// memory, and a thread reads every word it owns before it writes one, so in place is safe by construction.
//
// The 64 intermediate words of a thread live in LDS: the thread's column of a [64][64] u64 array (32 KiB per 64-thread workgroup) used as
// an indexed private file -- no barrier; word w of thread t sits at [w][t], conflict-free -- with the two passes as loops of eight lines.
// No scratch, no spills (DESIGN.md 3.11 has the resource figures; profiles/EXPERIMENTS.md 18 the register-resident alternative).
//
// Arithmetic.  Every constant is stored as (w mod q_i, floor((w mod q_i) 2^64 / q_i)) in the plan's device table (4 x 64 pairs per prime)
// and applied with a Shoup product, which takes ANY 64-bit operand.  Lazy accumulation: a term is below 4 q_i (mul_shoup_lazy4), eight of
// them below 32 q_i <= 2^63 for primes of at most 58 bits -- every class the presets use -- and go unreduced into the next product.
// Eight lazy products of a 61-bit prime do not fit 64 bits: contexts with a wider prime, and contexts created with FHE_NTT_NOPM=1, take
// canonical products (below q_i; eight below 2^64 for q_i < 2^61).  The last product (post, or 1) is reduced to [0, q_i).
#include "packed_arith.h"

#include <cmath>
#include <vector>

namespace {

struct B8Tab { ulonglong2 pre[64], L[64], R[64], post[64]; };      // per prime: (w mod q, Shoup companion)
// one line of eight: o[v] = sum_y i[y] M[v][y], each sum below 32 q (LAZY) or 8 q.  The eight pairs of output v + 1 are requested before
// the products of output v, so their scalar-load latency is covered by about a hundred vector instructions (two sets of 32 SGPRs).
template <bool LAZY>
__device__ __forceinline__ void line8(u64 (&o)[8], const u64 (&i)[8], const ulonglong2 *M, const PkArith<LAZY> &A) {
    ulonglong2 cur[8], nxt[8];
    const ulonglong2 *M0 = fresh(M);
#pragma unroll
    for (int y = 0; y < 8; y++) cur[y] = M0[y];
#pragma unroll
    for (int v = 0; v < 8; v++) {
        if (v < 7) {
            const ulonglong2 *Mv = fresh(M + 8 * (v + 1));
#pragma unroll
            for (int y = 0; y < 8; y++) nxt[y] = Mv[y];
        }
        __builtin_amdgcn_sched_barrier(0);                           // the requests stay in front, and nothing of one output is scheduled into another's
        u64 acc = A.mul(i[0], cur[0]);
#pragma unroll
        for (int y = 1; y < 8; y++) acc += A.mul(i[y], cur[y]);
        o[v] = acc;
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int y = 0; y < 8; y++) cur[y] = nxt[y];
    }
}

// grid: x = word position / 64 within a ciphertext (size * k * n words; n is a multiple of 64, so a workgroup has ONE prime and the
// table reads are scalar), y = group.  Group g, ciphertext p, word e: in[(g * 64 + p) * ctw + e].  in / out are not __restrict__: they may
// be the same buffer; the first store of a thread follows its last load through the data dependence of the column pass on every row.
// The loads of row x + 1 are issued before the arithmetic of row x (about a thousand vector instructions), so one wave per SIMD hides
// its own memory latency: the 32 KiB of LDS per workgroup allow five workgroups per CU.
template <bool LAZY, bool PRE>
__global__ __launch_bounds__(64, 2) void k_block8x8(const u64 *in, u64 *out, const B8Tab *__restrict__ tab, PkMods M, u32 n, u32 k, u64 ctw) {
    __shared__ u64 mid[64][64];                                                      // [word of the thread][thread]: conflict-free, private, no barrier
    const u64 e = (u64)blockIdx.x * 64 + threadIdx.x;
    const u32 i = (u32)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * 64u / n) % k));      // ctw <= 2^26 words; the division runs on the vector unit
    const B8Tab *T = tab + i;
    const PkArith<LAZY> A(M.q[i]);
    const u64 *src = in + (u64)blockIdx.y * 64 * ctw + e;
    u64 *dst = out + (u64)blockIdx.y * 64 * ctw + e;
    u64 r[8];
#pragma unroll
    for (int y = 0; y < 8; y++) r[y] = src[(u64)y * ctw];
#pragma unroll 1
    for (int x = 0; x < 8; x++) {
        u64 nx[8], o[8];
#pragma unroll
        for (int y = 0; y < 8; y++) nx[y] = x < 7 ? src[(u64)(8 * (x + 1) + y) * ctw] : 0;       // wave-uniform: the last row prefetches nothing
        if constexpr (PRE) {
            const ulonglong2 *P = fresh(T->pre + 8 * x);
#pragma unroll
            for (int y = 0; y < 8; y++) r[y] = A.mul(r[y], P[y]);
        }
        line8<LAZY>(o, r, T->R, A);
#pragma unroll
        for (int v = 0; v < 8; v++) mid[8 * x + v][threadIdx.x] = o[v];
#pragma unroll
        for (int y = 0; y < 8; y++) r[y] = nx[y];
    }
#pragma unroll 1
    for (int v = 0; v < 8; v++) {
        u64 o[8];
#pragma unroll
        for (int x = 0; x < 8; x++) r[x] = mid[8 * x + v][threadIdx.x];
        line8<LAZY>(o, r, T->L, A);
        ulonglong2 P[8];                                                             // post[u][v], u = 0 .. 7: a column of the table
#pragma unroll
        for (int u = 0; u < 8; u++) P[u] = fresh(T->post + v)[8 * u];
#pragma unroll
        for (int u = 0; u < 8; u++) dst[(u64)(8 * u + v) * ctw] = A.canon(A.mul(o[u], P[u]));
    }
}

// fhe_channel_mix: out_i = sum_j M[i][j] in_j on every word of every ciphertext.  tab: [k][m * c] pairs; a zero entry is (0, 0) and
// contributes 0.  The sum of at most eight terms obeys the bounds above; the last step is a product with 1 that reduces it.
struct MixTab { ulonglong2 w[FHE_MAX_K][64]; ulonglong2 one[FHE_MAX_K]; u64 q[FHE_MAX_K]; };
template <bool LAZY>
__global__ __launch_bounds__(256) void k_channel_mix(const u64 *in, u64 in_cs, u64 in_ps, u64 *out, u64 out_cs, u64 out_ps, const MixTab *__restrict__ tab,
                                                     u32 c, u32 m, u32 n, u32 k, u64 ctw, u64 count) {
    const u64 e = (u64)blockIdx.x * 256 + threadIdx.x;             // ctw is a multiple of 256 (n >= 1024)
    const u32 i = (u32)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * 256u / n) % k));
    const PkArith<LAZY> A(tab->q[i]);
    const ulonglong2 *W = tab->w[i];
    const ulonglong2 one = tab->one[i];
    for (u64 g = blockIdx.y; g < count; g += gridDim.y) {
        u64 v[8];
#pragma unroll
        for (u32 j = 0; j < 8; j++) v[j] = j < c ? in[g * in_cs + j * in_ps + e] : 0;      // every read before the first write (in place)
#pragma unroll
        for (u32 o = 0; o < 8; o++) {
            if (o < m) {
                const ulonglong2 *Wo = fresh(W + o * c);
                u64 acc = 0;
#pragma unroll
                for (u32 j = 0; j < 8; j++)
                    if (j < c) acc += A.mul(v[j], Wo[j]);
                out[g * out_cs + o * out_ps + e] = A.canon(A.mul(acc, one));
            }
        }
    }
}

}  // namespace

struct fhe_block8x8_plan {
    const fhe_ctx *ctx = nullptr;
    B8Tab *d_tab = nullptr;       // [k]
    bool has_pre = false;
};

extern "C" int fhe_block8x8_plan_create(const fhe_ctx *c, const int64_t *L, const int64_t *R, const int64_t *pre, const int64_t *post, fhe_stream s,
                                        fhe_block8x8_plan **out) {
    if (!c || !L || !R || !out) return fail(FHE_ERR_PARAM, "null argument");
    *out = nullptr;
    for (int j = 0; j < 64; j++) {
        if (!scalar_ok(c, L[j]) || !scalar_ok(c, R[j]) || (pre && !scalar_ok(c, pre[j])) || (post && !scalar_ok(c, post[j])))
            return fail(FHE_ERR_PARAM, "scalar %d out of range: |w| <= min((t - 1) / 2, 2^31 - 1) with t = %llu", j, (unsigned long long)c->t);
        if ((pre && !pre[j]) || (post && !post[j])) return fail(FHE_ERR_PARAM, "entry %d of pre / post is zero (multiply_plain by the zero plaintext is refused)", j);
    }
    for (int u = 0; u < 8; u++) {
        bool lz = true, rz = true;
        for (int x = 0; x < 8; x++) { lz = lz && !L[8 * u + x]; rz = rz && !R[8 * u + x]; }
        if (lz || rz) return fail(FHE_ERR_PARAM, "row %d of %s is all zero: the output would be the transparent zero", u, lz ? "L" : "R");
    }
    std::vector<B8Tab> tab(c->k);
    for (u32 i = 0; i < c->k; i++) {
        const u64 q = c->qb.primes[i];
        for (int j = 0; j < 64; j++) {
            tab[i].pre[j] = lift_pair(pre ? pre[j] : 1, q);
            tab[i].L[j] = lift_pair(L[j], q);
            tab[i].R[j] = lift_pair(R[j], q);
            tab[i].post[j] = lift_pair(post ? post[j] : 1, q);
        }
    }
    fhe_block8x8_plan *p = new fhe_block8x8_plan;
    p->ctx = c;
    p->has_pre = pre != nullptr;
    const size_t bytes = tab.size() * sizeof(B8Tab);
    hipError_t e = hipMalloc((void **)&p->d_tab, bytes);
    if (e == hipSuccess) e = hipMemcpyAsync(p->d_tab, tab.data(), bytes, hipMemcpyHostToDevice, (hipStream_t)s);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)s);                     // `tab` leaves scope
    if (e != hipSuccess) {
        if (p->d_tab) (void)hipFree(p->d_tab);
        delete p;
        return fail(e == hipErrorOutOfMemory ? FHE_ERR_NOMEM : FHE_ERR_HIP, "block8x8 plan table: %s", hipGetErrorString(e));
    }
    *out = p;
    return FHE_OK;
}

extern "C" int fhe_block8x8_plan_destroy(fhe_block8x8_plan *p) {
    if (!p) return FHE_OK;
    if (p->d_tab) (void)hipFree(p->d_tab);
    delete p;
    return FHE_OK;
}

extern "C" int fhe_block8x8_scalar(const fhe_ctx *c, const fhe_block8x8_plan *plan, const uint64_t *in, uint64_t *out, uint32_t size, uint64_t count,
                                   fhe_stream s) {
    if (!c || !plan || !in || !out) return fail(FHE_ERR_PARAM, "null argument");
    if (plan->ctx != c) return fail(FHE_ERR_PARAM, "the plan was built for another context");
    if (size < 2 || size > FHE_MAX_POLYS) return fail(FHE_ERR_PARAM, "size %u: 2 .. FHE_MAX_POLYS polynomials per ciphertext", size);
    if (!count) return FHE_OK;
    const u64 ctw = (u64)size * c->k * c->n, total = count * 64 * ctw;
    if (count >> 34) return fail(FHE_ERR_PARAM, "count %llu: more groups than 2^60 words hold", (unsigned long long)count);      // ctw <= 2^26: total cannot wrap
    if (out != in && overlap(in, total, out, total)) return fail(FHE_ERR_PARAM, "output range overlaps the input range (only out == in may alias)");
    hipStream_t st = (hipStream_t)s;
    const PkMods M = pk_mods(c);
    for (u64 g0 = 0; g0 < count; g0 += 65535) {                                       // grid.y holds 65535 groups
        const dim3 grid((unsigned)(ctw / 64), (unsigned)(count - g0 < 65535 ? count - g0 : 65535));
        const u64 *pi = (const u64 *)in + g0 * 64 * ctw;
        u64 *po = (u64 *)out + g0 * 64 * ctw;
#define GO(LAZY, PRE) k_block8x8<LAZY, PRE><<<grid, 64, 0, st>>>(pi, po, plan->d_tab, M, c->n, c->k, ctw)
        if (lazy_ok(c)) { if (plan->has_pre) GO(true, true); else GO(true, false); }
        else { if (plan->has_pre) GO(false, true); else GO(false, false); }
#undef GO
    }
    KERNEL_CHECK();
    return FHE_OK;
}

// the two extents (count, ct stride) and (planes, plane stride) of a channel_mix operand tile without overlap: the smaller stride holds a
// ciphertext, the larger one holds the whole inner extent (an extent of 1 has no stride to check)
static bool mix_layout_ok(u64 ctw, u64 count, u64 cs, u32 planes, u64 ps) {
    if (count > 1 && planes > 1) {
        const bool ct_inner = cs <= ps;
        const u64 s_in = ct_inner ? cs : ps, n_in = ct_inner ? count : planes, s_out = ct_inner ? ps : cs;
        return s_in >= ctw && s_out / n_in >= s_in;                 // s_out >= n_in * s_in without the product
    }
    if (count > 1) return cs >= ctw;
    if (planes > 1) return ps >= ctw;
    return true;
}
// words from the first word of an operand to its last + 1; 0 when that does not fit 2^60 words (strides or counts no allocation can have)
static u64 mix_extent(u64 ctw, u64 count, u64 cs, u32 planes, u64 ps) {
    const unsigned __int128 x = (unsigned __int128)(count - 1) * cs + (unsigned __int128)(planes - 1) * ps + ctw;
    return x >> 60 ? 0 : (u64)x;
}

extern "C" int fhe_channel_mix(const fhe_ctx *c, const int64_t *Mx, const int64_t *bias, uint32_t ch, uint32_t m, const uint64_t *in, uint64_t in_cs,
                               uint64_t in_ps, uint64_t *out, uint64_t out_cs, uint64_t out_ps, uint32_t size, uint64_t count, fhe_stream s) {
    if (!c || !Mx || !in || !out) return fail(FHE_ERR_PARAM, "null argument");
    if (ch < 1 || ch > 8 || m < 1 || m > 8) return fail(FHE_ERR_PARAM, "channel_mix: 1 <= c, m <= 8 (got c = %u, m = %u)", ch, m);
    if (size < 2 || size > FHE_MAX_POLYS) return fail(FHE_ERR_PARAM, "size %u: 2 .. FHE_MAX_POLYS polynomials per ciphertext", size);
    for (u32 o = 0; o < m; o++) {
        bool zero = true;
        for (u32 j = 0; j < ch; j++) {
            if (!scalar_ok(c, Mx[o * ch + j])) return fail(FHE_ERR_PARAM, "scalar M[%u][%u] out of range: |w| <= min((t - 1) / 2, 2^31 - 1)", o, j);
            zero = zero && !Mx[o * ch + j];
        }
        if (zero) return fail(FHE_ERR_PARAM, "row %u of M is all zero: the output would be the transparent zero", o);
        if (bias && !scalar_ok(c, bias[o])) return fail(FHE_ERR_PARAM, "bias %u out of range: |w| <= min((t - 1) / 2, 2^31 - 1)", o);
    }
    if (!count) return FHE_OK;
    const u64 ctw = (u64)size * c->k * c->n;
    if (!mix_layout_ok(ctw, count, in_cs, ch, in_ps) || !mix_layout_ok(ctw, count, out_cs, m, out_ps))
        return fail(FHE_ERR_PARAM, "channel_mix: strides let ciphertexts of one operand overlap");
    const u64 in_words = mix_extent(ctw, count, in_cs, ch, in_ps), out_words = mix_extent(ctw, count, out_cs, m, out_ps);
    if (!in_words || !out_words) return fail(FHE_ERR_PARAM, "channel_mix: count and strides describe more than 2^60 words");
    const bool same = (const uint64_t *)out == in && in_cs == out_cs && in_ps == out_ps && m == ch;
    if (!same && overlap(in, in_words, out, out_words))
        return fail(FHE_ERR_PARAM, "output range overlaps the input range (in place needs identical pointers and strides and m == c)");
    MixTab tab{};
    for (u32 i = 0; i < c->k; i++) {
        for (u32 j = 0; j < m * ch; j++) tab.w[i][j] = lift_pair(Mx[j], c->qb.primes[i]);
        tab.one[i] = lift_pair(1, c->qb.primes[i]);
        tab.q[i] = c->qb.primes[i];
    }
    hipStream_t st = (hipStream_t)s;
    FheStage sg;
    int rc = fhe_stage_acquire(&tab, sizeof tab, st, &sg);
    if (rc) return rc;
    const dim3 grid((unsigned)(ctw / 256), (unsigned)(count < 65535 ? count : 65535));
    if (lazy_ok(c)) k_channel_mix<true><<<grid, 256, 0, st>>>((const u64 *)in, in_cs, in_ps, (u64 *)out, out_cs, out_ps, (const MixTab *)sg.dev, ch, m, c->n, c->k, ctw, count);
    else k_channel_mix<false><<<grid, 256, 0, st>>>((const u64 *)in, in_cs, in_ps, (u64 *)out, out_cs, out_ps, (const MixTab *)sg.dev, ch, m, c->n, c->k, ctw, count);
    const hipError_t le = hipGetLastError();
    rc = fhe_stage_release(sg, st);
    if (le != hipSuccess) return fail(FHE_ERR_HIP, "kernel launch: %s", hipGetErrorString(le));
    if (rc) return rc;
    if (bias) {                                                       // add_plain of the one-coefficient plaintext [bias mod t], sign +1, per output plane
        for (u32 o = 0; o < m; o++) {
            if (!bias[o]) continue;
            const uint64_t p = bias[o] < 0 ? c->t - ((u64)0 - (u64)bias[o]) : (u64)bias[o];
            if ((rc = fhe_add_plain(c, out + o * out_ps, out_cs, count, &p, 1, 1, s))) return rc;
        }
    }
    return FHE_OK;
}

// D[u][x] = round-half-away(2^bits c_u / 2 cos((2 x + 1) u pi / 16)), c_0 = 1 / sqrt 2: the orthonormal 8-point DCT-II scaled by 2^bits
extern "C" int fhe_dct8_matrix(int bits, int64_t *D) {
    if (!D) return fail(FHE_ERR_PARAM, "null argument");
    if (bits < 1 || bits > 20) return fail(FHE_ERR_PARAM, "dct8_matrix: bits = %d (1 .. 20)", bits);
    const long double pi = 3.14159265358979323846264338327950288L;
    for (int u = 0; u < 8; u++)
        for (int x = 0; x < 8; x++) {
            const long double v = ldexpl((u ? 1.0L : sqrtl(0.5L)) * 0.5L * cosl((2 * x + 1) * u * pi / 16), bits);
            D[8 * u + x] = (int64_t)(v < 0 ? -floorl(-v + 0.5L) : floorl(v + 0.5L));
        }
    return FHE_OK;
}
