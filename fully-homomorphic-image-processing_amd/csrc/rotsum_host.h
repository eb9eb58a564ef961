// rotsum_host.h -- the host arithmetic of a rotate-sum plan (rotsum.hip, include/fhe_hip.h fhe_rotsum_plan_create): the checks on the taps
// and the slot permutations pi_g, from a given transform of the monomial X; and the check on the operands of a call that rotsum.hip,
// rotdiag.hip and rotbsgs.hip share.  No device, no HIP header: tools/rotsum_host_check.cpp builds it alone, under the host sanitizers.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

namespace rotsum {

constexpr uint32_t MAX_TAPS = 64;

inline uint64_t mulmod(uint64_t a, uint64_t b, uint64_t q) { return (uint64_t)((unsigned __int128)a * b % q); }

// "" when the taps are admissible, otherwise the reason.  elts [taps], weights [taps] (any 64-bit value, taken modulo t), keys [taps]
// (only compared with null; null itself = the caller checks no keys, the Python model of the checks)
inline std::string check_taps(uint32_t n, uint64_t t, uint32_t k, uint32_t taps, const uint32_t *elts, const uint64_t *weights, const void *const *keys) {
    if (k < 2) return "a special-prime key switch needs a context of at least 2 primes (the last one is the special prime)";
    if (taps == 0 || taps > MAX_TAPS) return "tap count " + std::to_string(taps) + ": 1 .. " + std::to_string(MAX_TAPS);
    if (!elts || !weights) return "null argument";
    for (uint32_t j = 0; j < taps; j++) {
        const uint32_t g = elts[j];
        if (!(g & 1) || g >= 2 * n) return "Galois element " + std::to_string(g) + ": must be odd and in [1, 2n = " + std::to_string(2 * n) + ")";
        for (uint32_t i = 0; i < j; i++)
            if (elts[i] == g) return "Galois element " + std::to_string(g) + " is repeated";
        if (weights[j] % t == 0) return "weight of tap " + std::to_string(j) + " is 0 modulo t";
        if (keys && g != 1 && !keys[j]) return "null key for Galois element " + std::to_string(g);
    }
    return "";
}

// the centred lift of w mod t, in (-t/2, t/2], reduced modulo q
inline uint64_t weight_residue(uint64_t w, uint64_t t, uint64_t q) {
    w %= t;
    return 2 * w > t ? (q - (t - w) % q) % q : w % q;
}

// xhat [n]: the forward transform modulo q of the monomial X, so slot s holds psi^(e_s) for a primitive 2n-th root psi and odd e_s.
// f [n]: e_s / e_0 mod 2n (odd, pairwise distinct), whatever psi is.  false when xhat is no such transform.
inline bool slot_exponents(const uint64_t *xhat, uint32_t n, uint64_t q, std::vector<uint32_t> &f) {
    const uint64_t rho = xhat[0];
    if (n < 2 || rho == 0 || rho >= q) return false;
    // powers of rho, sorted by value: rho^j for odd j < 2n must be pairwise distinct and cover every slot
    std::vector<std::pair<uint64_t, uint32_t>> pw;
    pw.reserve(n);
    const uint64_t rho2 = mulmod(rho, rho, q);
    uint64_t cur = rho;
    for (uint32_t j = 1; j < 2 * n; j += 2) {
        pw.emplace_back(cur, j);
        cur = mulmod(cur, rho2, q);
    }
    if (cur != rho) return false;                       // rho^(2n) != 1
    std::sort(pw.begin(), pw.end());
    for (uint32_t j = 1; j < n; j++)
        if (pw[j].first == pw[j - 1].first) return false;   // the order of rho is below 2n
    f.assign(n, 0);
    std::vector<char> seen(2 * (size_t)n, 0);
    for (uint32_t s = 0; s < n; s++) {
        auto it = std::lower_bound(pw.begin(), pw.end(), std::make_pair(xhat[s], (uint32_t)0));
        if (it == pw.end() || it->first != xhat[s] || seen[it->second]) return false;
        seen[it->second] = 1;
        f[s] = it->second;
    }
    return true;
}

// perm [n]: pi_g reads slot s from the slot that holds psi^(e_s g mod 2n), i.e. the one whose relative exponent is f_s g mod 2n
inline bool slot_perm(const std::vector<uint32_t> &f, uint32_t g, uint32_t *perm) {
    const uint32_t n = (uint32_t)f.size();
    if (!n || (n & (n - 1)) || !(g & 1) || g >= 2 * n) return false;
    std::vector<uint32_t> where(2 * (size_t)n, n);
    for (uint32_t s = 0; s < n; s++) {
        if (f[s] >= 2 * n || where[f[s]] != n) return false;
        where[f[s]] = s;
    }
    for (uint32_t s = 0; s < n; s++) {
        const uint32_t src = where[(uint32_t)(((uint64_t)f[s] * g) & (2 * n - 1))];
        if (src == n) return false;
        perm[s] = src;
    }
    return true;
}

// do [a, a + a_words) and [b, b + b_words) share a 64-bit word (internal.h's overlap, for a header without the device's)
inline bool overlap(const void *a, uint64_t a_words, const void *b, uint64_t b_words) {
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + a_words * 8, b0 = (uintptr_t)b, b1 = b0 + b_words * 8;
    return a0 < b1 && b0 < a1;
}

// "" when fhe_rotate_sum_sp, fhe_rotate_each_sp, fhe_rotate_diag_sum_sp or fhe_rotate_bsgs_sp may run on these operands, otherwise the
// reason, in the order include/fhe_hip.h lists the checks.  Nothing is dereferenced.  launch: the family's largest launch-size product;
// need: the bytes of scratch the call takes; taps != 0: fhe_rotate_each_sp, out [taps] batches tap_stride words apart and no in-place form
inline std::string check_call(uint32_t k, uint32_t n, const void *ct, uint64_t stride, const void *out, uint64_t out_stride, uint64_t count, uint64_t launch,
                              size_t need, const void *scratch, size_t scratch_bytes, uint32_t taps = 0, uint64_t tap_stride = 0) {
    const uint64_t Ln = (uint64_t)(k - 1) * n;
    if (stride < 2 * Ln) return "ciphertext stride smaller than a size-2 ciphertext of " + std::to_string(k - 1) + " primes";
    if (out_stride < 2 * Ln) return "output stride smaller than a size-2 ciphertext of " + std::to_string(k - 1) + " primes";
    if (!count) return "";
    if (launch > 0x7fffffffULL) return "too many ciphertexts for one call";
    const uint64_t out_batch = (count - 1) * out_stride + 2 * Ln;
    if (taps && tap_stride < out_batch) return "tap stride smaller than one batch of outputs";
    if (!scratch || scratch_bytes < need) return "scratch too small";
    const uint64_t in_words = (count - 1) * stride + 2 * Ln, out_words = taps ? (taps - 1) * tap_stride + out_batch : out_batch;
    if (taps) {
        if (overlap(ct, in_words, out, out_words)) return "output range overlaps the input range (fhe_rotate_each_sp has no in-place form)";
    } else if (!(out == ct && out_stride == stride) && overlap(ct, in_words, out, out_words)) {
        return "output range overlaps the input range (only out2 == ct2 with out_stride == stride may alias)";
    }
    if (overlap(scratch, need / 8, ct, in_words) || overlap(scratch, need / 8, out, out_words)) return "scratch overlaps the input or the output";
    return "";
}

}  // namespace rotsum
