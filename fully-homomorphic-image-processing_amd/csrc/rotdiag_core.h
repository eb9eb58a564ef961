// rotdiag_core.h -- the two transform kernels of the pseudo-Mersenne path that rotdiag.hip and rotbsgs.hip share, moved here from rotdiag.hip
// as they were: the forward transforms of the digits of c_1 and of c_0, and the inverse transform with the drop of the special prime.
// Internal linkage: each translation unit compiles its own copy.
#pragma once
#include "ksp_core.h"

namespace {

// (1) per ciphertext L k + L workgroups.  The first L k are k_ksp_fwd_pm's (c, i, r): dig[c][i][r] = NTT_(q_r)([c_1,i]_(q_r)), folded below
// PM_FOLDED when r != i.  The last L are (c, r): c0h[c][r] = NTT_(q_r)(c_0,r), canonical input.
template <int L, typename C>
__global__ __launch_bounds__(NttShape<L>::TP, 4) void k_rd_fwd_pm(const u64 *__restrict__ ct, u64 stride, u64 *__restrict__ dig, u64 *__restrict__ c0h, RnsBase base) {
    __shared__ u64 lds[NttShape<L>::LDS_WORDS];
    constexpr int N = NttShape<L>::N;
    const int tid = threadIdx.x;
    const u32 k = base.count, Lq = k - 1, per = Lq * k + Lq, w = blockIdx.x % per;
    const u64 c = blockIdx.x / per;
    const bool d = w < Lq * k;                     // uniform per workgroup
    const u32 r = d ? w % k : w - Lq * k, i = d ? w / k : r;
    const PmMod m = base.pm[r];
    u64 x[1][16];
    load_coeff<L>(x[0], ct + c * stride + ((u64)(d ? Lq : 0) + i) * N, tid);
    if (r != i) {
#pragma unroll
        for (int e = 0; e < 16; e++) x[0][e] = fold_pm(x[0][e], m);
    }
    ntt_fwd_regs_pm<L, 1, PM_FOLDED, C::LIM, C::CS>(x, base.tw_pm + (size_t)r * N, m, lds, tid);
#pragma unroll
    for (int e = 0; e < 16; e++) x[0][e] = canon_pm(x[0][e], m);
    store_slots<L>(x[0], d ? dig + ((c * Lq + i) * k + r) * N : c0h + (c * k + r) * N, tid);
}
// (4) workgroup (c, pp, r < L): k_ksp_inv_down_add_pm's transform and drop, nothing added: the input's terms went through the accumulator
template <int L, typename C>
__global__ __launch_bounds__(NttShape<L>::TP, 4) void k_rd_inv_down_pm(u64 *__restrict__ out, u64 out_stride, const u64 *__restrict__ acc, const u64 *__restrict__ sp,
                                                                        RnsBase base, KspTab T) {
    __shared__ u64 lds[NttShape<L>::LDS_WORDS];
    constexpr int N = NttShape<L>::N;
    const int tid = threadIdx.x;
    const u32 k = base.count, Lq = k - 1, r = blockIdx.x % Lq, pp = (blockIdx.x / Lq) & 1;
    const u64 cpp = blockIdx.x / Lq;               // c * 2 + pp
    const u64 c = cpp >> 1;
    const PmMod m = base.pm[r];
    u64 x[1][16], y[16];
    load_slots<L>(x[0], acc + (cpp * k + r) * N, tid);
    ntt_inv_regs_pm<L, 1, PM_FOLDED, C::XB, C::LIM, C::RQ>(x, base.itw_pm + (size_t)r * N, m, lds, tid);
    load_coeff<L>(y, sp + cpp * N, tid);
#pragma unroll
    for (int e = 0; e < 16; e++) x[0][e] = ksp_drop(canon_rq_pm<C::RQ>(x[0][e], m), y[e], T, r);
    store_coeff<L>(x[0], out + c * out_stride + ((u64)pp * Lq + r) * N, tid);
}

}  // namespace
