// planemap.hip -- fhe_plane_map: a sparse integer linear map ACROSS position-packed ciphertexts on gfx950 (packed resize, warps, strided
// tile filters, chroma subsampling).  include/fhe_hip.h states the operation; packed.hip has the dense 8x8 and channel maps.
//
// Ciphertext p of a frame holds pixel p of n independent frames in its slots, so output plane o = sum over its live slots of
// w * in[tap]: scalar weights (packed_arith.h), element-wise in the coefficient index, no transform, no rotation, no key.
//
// k_plane_map<LAZY, W>.  The plan cuts the outputs into GROUPS whose live sources, taken together, number at most W (plan_create, below;
// the same cut on every host).  A 64-thread workgroup owns 64 consecutive word positions of one (ciphertext, group): one prime, so every
// table read is a scalar load at a wave-uniform address.  It loads the group's sources into the thread's column of a [W][64] u64 LDS
// array -- coalesced, eight loads in flight, no barrier: word w of thread t sits at [w][t] and only thread t touches it -- then walks the
// group's outputs: a term is one LDS read at a wave-uniform row and one Shoup product, an output word is written once.  A source that two
// groups use is read by both (plan_info: source_reads); inside a group it is read once however many outputs use it.
//
// k_plane_map_direct<LAZY>: one thread per (output plane, word) reads its sources straight from global memory, the same term lists with
// plane ids where the windowed kernel has LDS rows.  It is the correctness baseline AND the default: measured on the same resident batch
// it was faster than the best window in two of six cases, and the adoption rule asked for "not slower in every case".
// The windowed kernel runs for a plan created with an explicit window, or in a context created with FHE_PLANEMAP_WINDOW=16|32|64;
// FHE_PLANEMAP_DIRECT=1 forces the direct kernel everywhere.
//
// Term lists are padded to a multiple of four with (row 0, pair (0, 0)) entries -- a product with the pair (0, 0) is 0 in both
// arithmetics -- so the inner step is four reads and four products without a branch.
//
// Arithmetic.  Lazy (packed_arith.h lazy_ok: primes of at most 58 bits, no FHE_NTT_NOPM): a term is below 4 q, a chunk of at most eight
// below 32 q <= 2^63; an output of more than eight terms reduces each chunk with the product by 1 (below 4 q) and sums at most eight
// chunks (below 32 q); the last product by 1 and canon() give [0, q).  Otherwise canonical products: eight below 8 q < 2^64 for
// q < 2^61, chunks reduced to [0, q), eight of them below 8 q again.
#include "packed_arith.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace {

struct PmGroup { u32 src_off, n_src, out_off, n_out; };            // into PmTab::src / PmTab::outs
struct PmOut { u32 plane, n_quads, term_off, live; };               // term_off (a multiple of 4) into rows / planes / pairs
struct PmTab {
    const PmGroup *groups;
    const u32 *src;                // source plane ids of the groups, one run per group
    const PmOut *outs;             // in group order
    const u32 *rows;               // per term: row of the source in its group's window
    const u32 *planes;             // per term: the source plane id (direct kernel)
    const ulonglong2 *pairs;       // [k][n_terms]: (w mod q_i, Shoup companion)
    u32 n_terms;
};
struct PmOne { ulonglong2 v[FHE_MAX_K]; };                          // (1, floor(2^64 / q_i)), by value

// one output word: `rd(j)` is the operand of term j, `pw` its pairs; n_quads >= 1 groups of four terms
template <bool LAZY, typename Read>
__device__ __forceinline__ u64 pm_output(const PkArith<LAZY> &A, ulonglong2 one, u32 n_quads, const ulonglong2 *pw, Read rd) {
    const bool multi = n_quads > 2;
    u64 total = 0;
#pragma unroll 1
    for (u32 qd = 0; qd < n_quads; qd += 2) {
        u64 x[4];
#pragma unroll
        for (u32 j = 0; j < 4; j++) x[j] = rd(4 * qd + j);
        u64 acc = A.mul(x[0], pw[4 * qd]);
#pragma unroll
        for (u32 j = 1; j < 4; j++) acc += A.mul(x[j], pw[4 * qd + j]);
        if (qd + 1 < n_quads) {
#pragma unroll
            for (u32 j = 0; j < 4; j++) x[j] = rd(4 * qd + 4 + j);
#pragma unroll
            for (u32 j = 0; j < 4; j++) acc += A.mul(x[j], pw[4 * qd + 4 + j]);
        }
        total += multi ? A.mul(acc, one) : acc;
    }
    return A.canon(A.mul(total, one));
}

// grid: x = word position / 64 within a ciphertext (n is a multiple of 64: one prime per workgroup), y = group of [g0, g1) (strided),
// z = ciphertext.  in [count][n_in][ctw], out [count][n_out][ctw] do not overlap (the host refuses it).
template <bool LAZY, int W>
__global__ __launch_bounds__(64) void k_plane_map(const u64 *__restrict__ in, u64 *__restrict__ out, PmTab T, PkMods M, PmOne O, u32 g0, u32 g1, u32 n, u32 k,
                                                  u64 ctw, u32 n_in, u32 n_out) {
    __shared__ u64 win[W][64];                                       // [source of the group][thread]: conflict-free, private, no barrier
    const u32 tid = threadIdx.x;
    const u64 e = (u64)blockIdx.x * 64 + tid;
    const u32 i = (u32)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * 64u / n) % k));
    const PkArith<LAZY> A(M.q[i]);
    const ulonglong2 one = O.v[i];
    const ulonglong2 *pairs = T.pairs + (u64)i * T.n_terms;
    const u64 *src = in + (u64)blockIdx.z * n_in * ctw + e;
    u64 *dst = out + (u64)blockIdx.z * n_out * ctw + e;
#pragma unroll 1
    for (u32 g = g0 + blockIdx.y; g < g1; g += gridDim.y) {
        const PmGroup G = T.groups[g];
        const u32 *sp = T.src + G.src_off;
#pragma unroll 1
        for (u32 s = 0; s < G.n_src; s += 8) {                        // n_src <= W: the plan launches the instance that holds its groups
            u64 r[8];
#pragma unroll
            for (u32 j = 0; j < 8; j++) r[j] = s + j < G.n_src ? src[(u64)sp[s + j] * ctw] : 0;
#pragma unroll
            for (u32 j = 0; j < 8; j++)
                if (s + j < G.n_src) win[s + j][tid] = r[j];
        }
        const PmOut *op = T.outs + G.out_off;
#pragma unroll 1
        for (u32 o = 0; o < G.n_out; o++) {
            const PmOut D = op[o];
            const u32 *rw = T.rows + D.term_off;
            dst[(u64)D.plane * ctw] = pm_output<LAZY>(A, one, D.n_quads, pairs + D.term_off, [&](u32 j) { return win[rw[j]][tid]; });
        }
    }
}

// grid: x = word position / 256, y = output (strided over the plan's n_out descriptors), z = ciphertext
template <bool LAZY>
__global__ __launch_bounds__(256) void k_plane_map_direct(const u64 *__restrict__ in, u64 *__restrict__ out, PmTab T, PkMods M, PmOne O, u32 n, u32 k, u64 ctw,
                                                          u32 n_in, u32 n_out) {
    const u64 e = (u64)blockIdx.x * 256 + threadIdx.x;              // ctw is a multiple of 256 (n >= 1024)
    const u32 i = (u32)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * 256u / n) % k));
    const PkArith<LAZY> A(M.q[i]);
    const ulonglong2 one = O.v[i];
    const ulonglong2 *pairs = T.pairs + (u64)i * T.n_terms;
    const u64 *src = in + (u64)blockIdx.z * n_in * ctw + e;
    u64 *dst = out + (u64)blockIdx.z * n_out * ctw + e;
#pragma unroll 1
    for (u32 o = blockIdx.y; o < n_out; o += gridDim.y) {
        const PmOut D = T.outs[o];
        const u32 *pl = T.planes + D.term_off;
        dst[(u64)D.plane * ctw] = pm_output<LAZY>(A, one, D.n_quads, pairs + D.term_off, [&](u32 j) { return src[(u64)pl[j] * ctw]; });
    }
}

u32 window_class(u32 n_src) { return n_src <= 16 ? 0 : n_src <= 32 ? 1 : 2; }

}  // namespace

// The window of the cut when neither the caller nor FHE_PLANEMAP_WINDOW names one: the fastest of 16, 32, 64 on the resize case
#define FHE_PLANE_DEFAULT_WINDOW 16

struct fhe_plane_map_plan {
    const fhe_ctx *ctx = nullptr;
    void *d_blob = nullptr;
    PmTab tab{};
    u32 n_in = 0, n_out = 0, n_groups = 0, window = 0;
    bool windowed = false;            // the caller or FHE_PLANEMAP_WINDOW named a window: k_plane_map runs, not the default direct kernel
    u32 class_end[3] = {0, 0, 0};     // groups [0, class_end[0]) fit 16 rows, [class_end[0], class_end[1]) 32, the rest 64
    u64 source_reads = 0;
};

extern "C" int fhe_plane_map_plan_create(const fhe_ctx *c, uint32_t n_in, uint32_t n_out, uint32_t T, const uint32_t *taps, const int64_t *weights,
                                         const uint32_t *order, uint32_t window, fhe_stream s, fhe_plane_map_plan **out) {
    if (!c || !taps || !weights || !out) return fail(FHE_ERR_PARAM, "null argument");
    *out = nullptr;
    if (!n_in || n_in > FHE_PLANE_MAX_PLANES || !n_out || n_out > FHE_PLANE_MAX_PLANES)
        return fail(FHE_ERR_PARAM, "plane_map: 1 <= n_in, n_out <= %d (got %u, %u)", FHE_PLANE_MAX_PLANES, n_in, n_out);
    if (T < 1 || T > FHE_PLANE_MAX_TAPS) return fail(FHE_ERR_PARAM, "plane_map: T = %u slots per output (1 .. %d)", T, FHE_PLANE_MAX_TAPS);
    if (window != 0 && window != 16 && window != 32 && window != 64) return fail(FHE_ERR_PARAM, "plane_map: window %u (0 = default, 16, 32 or 64)", window);
    const bool windowed = window != 0 || c->opt.planemap_window != 0;
    if (!window) window = c->opt.planemap_window ? c->opt.planemap_window : FHE_PLANE_DEFAULT_WINDOW;
    for (u32 o = 0; o < n_out; o++) {
        bool live = false;
        for (u32 p = 0; p < T; p++) {
            const int64_t w = weights[(size_t)o * T + p];
            if (!scalar_ok(c, w))
                return fail(FHE_ERR_PARAM, "scalar [%u][%u] out of range: |w| <= min((t - 1) / 2, 2^31 - 1) with t = %llu", o, p, (unsigned long long)c->t);
            if (!w) continue;
            live = true;
            if (taps[(size_t)o * T + p] >= n_in) return fail(FHE_ERR_PARAM, "plane_map: tap [%u][%u] = %u of a live slot is not below n_in = %u", o, p, taps[(size_t)o * T + p], n_in);
        }
        if (!live) return fail(FHE_ERR_PARAM, "plane_map: output %u has no live term: it would be the transparent zero", o);
    }
    if (order) {
        std::vector<bool> seen(n_out, false);
        for (u32 j = 0; j < n_out; j++) {
            if (order[j] >= n_out || seen[order[j]]) return fail(FHE_ERR_PARAM, "plane_map: order is not a permutation of 0 .. %u (entry %u)", n_out - 1, j);
            seen[order[j]] = true;
        }
    }
    // the groups: walk the outputs in `order`; an output joins the open group while the union of live sources stays within the window
    std::vector<PmGroup> groups;
    std::vector<u32> src, rows, planes, in_group(n_in, 0xffffffffu), row_of(n_in, 0), fresh_src;
    std::vector<PmOut> outs;
    std::vector<int64_t> wts;                                        // per term, padding = 0
    fresh_src.reserve(T);
    PmGroup G{0, 0, 0, 0};
    for (u32 j = 0; j < n_out; j++) {
        const u32 o = order ? order[j] : j;
        const u32 *tp = taps + (size_t)o * T;
        const int64_t *wp = weights + (size_t)o * T;
        auto collect = [&](u32 gid) {                                  // the live sources of `o` the group does not hold yet, each once
            fresh_src.clear();
            for (u32 p = 0; p < T; p++)
                if (wp[p] && in_group[tp[p]] != gid && std::find(fresh_src.begin(), fresh_src.end(), tp[p]) == fresh_src.end()) fresh_src.push_back(tp[p]);
        };
        collect((u32)groups.size());
        if (G.n_out && G.n_src + fresh_src.size() > window) {        // close the group; an output wider than the window gets one of its own
            groups.push_back(G);
            G = PmGroup{(u32)src.size(), 0, (u32)outs.size(), 0};
            collect((u32)groups.size());
        }
        const u32 gid = (u32)groups.size();
        for (u32 sp : fresh_src) {
            in_group[sp] = gid;
            row_of[sp] = G.n_src++;
            src.push_back(sp);
        }
        PmOut D{o, 0, (u32)rows.size(), 0};
        u32 first = 0;
        for (u32 p = 0; p < T; p++) {
            if (!wp[p]) continue;
            if (!D.live) first = tp[p];
            rows.push_back(row_of[tp[p]]);
            planes.push_back(tp[p]);
            wts.push_back(wp[p]);
            D.live++;
        }
        while (rows.size() % 4) { rows.push_back(0); planes.push_back(first); wts.push_back(0); }
        D.n_quads = (u32)(rows.size() - D.term_off) / 4;
        outs.push_back(D);
        G.n_out++;
    }
    groups.push_back(G);
    // groups by the kernel instance that holds them (stable: the walk's order inside a class)
    std::stable_sort(groups.begin(), groups.end(), [](const PmGroup &a, const PmGroup &b) { return window_class(a.n_src) < window_class(b.n_src); });
    fhe_plane_map_plan *p = new fhe_plane_map_plan;
    p->ctx = c;
    p->n_in = n_in;
    p->n_out = n_out;
    p->window = window;
    p->windowed = windowed;
    p->n_groups = (u32)groups.size();
    for (const PmGroup &g : groups) {
        p->source_reads += g.n_src;
        for (u32 cl = window_class(g.n_src); cl < 3; cl++) p->class_end[cl]++;
    }
    const size_t n_terms = rows.size();
    std::vector<ulonglong2> pairs((size_t)c->k * n_terms);
    for (u32 i = 0; i < c->k; i++)
        for (size_t j = 0; j < n_terms; j++) pairs[i * n_terms + j] = wts[j] ? lift_pair(wts[j], c->qb.primes[i]) : make_ulonglong2(0, 0);
    // one device blob: pairs (16-byte aligned) first, then the 32-bit tables
    const size_t off_pairs = 0, off_groups = off_pairs + pairs.size() * sizeof(ulonglong2), off_outs = off_groups + groups.size() * sizeof(PmGroup),
                 off_src = off_outs + outs.size() * sizeof(PmOut), off_rows = off_src + src.size() * 4, off_planes = off_rows + n_terms * 4,
                 bytes = off_planes + n_terms * 4;
    std::vector<unsigned char> blob(bytes);
    std::memcpy(blob.data() + off_pairs, pairs.data(), pairs.size() * sizeof(ulonglong2));
    std::memcpy(blob.data() + off_groups, groups.data(), groups.size() * sizeof(PmGroup));
    std::memcpy(blob.data() + off_outs, outs.data(), outs.size() * sizeof(PmOut));
    std::memcpy(blob.data() + off_src, src.data(), src.size() * 4);
    std::memcpy(blob.data() + off_rows, rows.data(), n_terms * 4);
    std::memcpy(blob.data() + off_planes, planes.data(), n_terms * 4);
    hipError_t e = hipMalloc(&p->d_blob, bytes);
    if (e == hipSuccess) e = hipMemcpyAsync(p->d_blob, blob.data(), bytes, hipMemcpyHostToDevice, (hipStream_t)s);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)s);                     // `blob` leaves scope
    if (e != hipSuccess) {
        if (p->d_blob) (void)hipFree(p->d_blob);
        delete p;
        return fail(e == hipErrorOutOfMemory ? FHE_ERR_NOMEM : FHE_ERR_HIP, "plane_map plan tables: %s", hipGetErrorString(e));
    }
    const unsigned char *d = (const unsigned char *)p->d_blob;
    p->tab = PmTab{(const PmGroup *)(d + off_groups), (const u32 *)(d + off_src), (const PmOut *)(d + off_outs), (const u32 *)(d + off_rows),
                   (const u32 *)(d + off_planes), (const ulonglong2 *)(d + off_pairs), (u32)n_terms};
    *out = p;
    return FHE_OK;
}

extern "C" int fhe_plane_map_plan_destroy(fhe_plane_map_plan *p) {
    if (!p) return FHE_OK;
    if (p->d_blob) (void)hipFree(p->d_blob);
    delete p;
    return FHE_OK;
}

extern "C" int fhe_plane_map_plan_info(const fhe_plane_map_plan *p, uint32_t *groups, uint64_t *source_reads, uint32_t *window) {
    if (!p) return fail(FHE_ERR_PARAM, "null argument");
    if (groups) *groups = p->n_groups;
    if (source_reads) *source_reads = p->source_reads;
    if (window) *window = p->window;
    return FHE_OK;
}

extern "C" int fhe_plane_map(const fhe_ctx *c, const fhe_plane_map_plan *plan, const uint64_t *in, uint64_t *out, uint32_t size, uint64_t count,
                             fhe_stream s) {
    if (!c || !plan || !in || !out) return fail(FHE_ERR_PARAM, "null argument");
    if (plan->ctx != c) return fail(FHE_ERR_PARAM, "the plan was built for another context");
    if (size < 2 || size > FHE_MAX_POLYS) return fail(FHE_ERR_PARAM, "size %u: 2 .. FHE_MAX_POLYS polynomials per ciphertext", size);
    if (!count) return FHE_OK;
    const u64 ctw = (u64)size * c->k * c->n;
    if (count >> 18) return fail(FHE_ERR_PARAM, "count %llu: more frames than 2^60 words hold", (unsigned long long)count);      // planes <= 2^16, ctw <= 2^26
    if (overlap(in, count * plan->n_in * ctw, out, count * plan->n_out * ctw))
        return fail(FHE_ERR_PARAM, "output range overlaps the input range (fhe_plane_map has no in-place form)");
    hipStream_t st = (hipStream_t)s;
    const PkMods M = pk_mods(c);
    PmOne O{};
    for (u32 i = 0; i < c->k; i++) O.v[i] = lift_pair(1, c->qb.primes[i]);
    const bool lazy = lazy_ok(c);
    for (u64 f0 = 0; f0 < count; f0 += 65535) {                                       // grid.z holds 65535 frames
        const unsigned nz = (unsigned)(count - f0 < 65535 ? count - f0 : 65535);
        const u64 *pi = (const u64 *)in + f0 * plan->n_in * ctw;
        u64 *po = (u64 *)out + f0 * plan->n_out * ctw;
        if (c->opt.planemap_direct || !plan->windowed) {
            const dim3 grid((unsigned)(ctw / 256), plan->n_out < 65535 ? plan->n_out : 65535, nz);
            if (lazy) k_plane_map_direct<true><<<grid, 256, 0, st>>>(pi, po, plan->tab, M, O, c->n, c->k, ctw, plan->n_in, plan->n_out);
            else k_plane_map_direct<false><<<grid, 256, 0, st>>>(pi, po, plan->tab, M, O, c->n, c->k, ctw, plan->n_in, plan->n_out);
            continue;
        }
        for (u32 cl = 0, g0 = 0; cl < 3; g0 = plan->class_end[cl++]) {
            const u32 g1 = plan->class_end[cl];
            if (g1 == g0) continue;
            const dim3 grid((unsigned)(ctw / 64), g1 - g0 < 65535 ? g1 - g0 : 65535, nz);
#define GO(W)                                                                                                                          \
    do {                                                                                                                               \
        if (lazy) k_plane_map<true, W><<<grid, 64, 0, st>>>(pi, po, plan->tab, M, O, g0, g1, c->n, c->k, ctw, plan->n_in, plan->n_out);  \
        else k_plane_map<false, W><<<grid, 64, 0, st>>>(pi, po, plan->tab, M, O, g0, g1, c->n, c->k, ctw, plan->n_in, plan->n_out);      \
    } while (0)
            if (cl == 0) GO(16);
            else if (cl == 1) GO(32);
            else GO(64);
#undef GO
        }
    }
    KERNEL_CHECK();
    return FHE_OK;
}
