// rotbsgs_host.h -- the host arithmetic a baby-step / giant-step plan adds to rotdiag_host.h (rotbsgs.hip, include/fhe_hip.h
// fhe_rotbsgs_plan_create): the checks on the two element lists, on the plaintexts [G2][G1][n] and their keys, the table of the present
// pairs and the scratch formula.  The centred lift, the slot permutations and the check on a call's operands are rotdiag_host.h's and rotsum_host.h's.
// No device, no HIP header: tools/rotbsgs_host_check.cpp builds it alone, under the host sanitizers.
#pragma once
#include "rotdiag_host.h"

namespace rotbsgs {

constexpr uint32_t MAX_STEPS = 64;      // per list: at most 64 baby and 64 giant elements
constexpr uint32_t GIANT_GROUP = 4;     // giant accumulators one thread of the baby accumulation keeps in registers (rotbsgs.hip)

// "" when the list is admissible, otherwise the reason.  what: "baby" or "giant"
inline std::string check_elts(uint32_t n, uint32_t count, const uint32_t *elts, const char *what) {
    if (count == 0 || count > MAX_STEPS) return std::string(what) + " step count " + std::to_string(count) + ": 1 .. " + std::to_string(MAX_STEPS);
    if (!elts) return "null argument";
    for (uint32_t j = 0; j < count; j++) {
        const uint32_t g = elts[j];
        if (!(g & 1) || g >= 2 * n) return std::string(what) + " Galois element " + std::to_string(g) + ": must be odd and in [1, 2n = " + std::to_string(2 * n) + ")";
        for (uint32_t i = 0; i < j; i++)
            if (elts[i] == g) return std::string(what) + " Galois element " + std::to_string(g) + " is repeated";
    }
    return "";
}

// idx [G2][G1]: the rank of pair (i, j) among the present pairs in row-major order, -1 for an absent (all-zero) pair.  Returns the
// number of present pairs.  plains [G2][G1][n]
inline uint32_t present_pairs(uint32_t n, uint32_t G1, uint32_t G2, const uint64_t *plains, std::vector<int32_t> &idx) {
    idx.assign((size_t)G1 * G2, -1);
    uint32_t pairs = 0;
    for (uint32_t u = 0; u < G1 * G2; u++) {
        const uint64_t *p = plains + (size_t)u * n;
        bool zero = true;
        for (uint32_t x = 0; x < n && zero; x++) zero = p[x] == 0;
        if (!zero) idx[u] = (int32_t)pairs++;
    }
    return pairs;
}

// The order rotbsgs.hip keeps the present pairs in: by (group of GIANT_GROUP giant steps, baby step, giant step within the group), so the
// present pairs of one (group, baby step) are consecutive rows.  idx [G2][G1]: the row of pair (i, j), -1 for an absent pair;
// grp [groups][G1][2]: (the row of the first present pair of (group, j), the mask of the group's giant steps present with j).
// Returns the number of present pairs
inline uint32_t group_rows(uint32_t n, uint32_t G1, uint32_t G2, const uint64_t *plains, std::vector<int32_t> &idx, std::vector<uint32_t> &grp) {
    std::vector<int32_t> rank;
    present_pairs(n, G1, G2, plains, rank);
    const uint32_t groups = (G2 + GIANT_GROUP - 1) / GIANT_GROUP;
    idx.assign((size_t)G1 * G2, -1);
    grp.assign((size_t)groups * G1 * 2, 0);
    uint32_t rows = 0;
    for (uint32_t g = 0; g < groups; g++)
        for (uint32_t j = 0; j < G1; j++) {
            grp[((size_t)g * G1 + j) * 2] = rows;
            for (uint32_t b = 0; b < GIANT_GROUP && g * GIANT_GROUP + b < G2; b++) {
                const size_t u = (size_t)(g * GIANT_GROUP + b) * G1 + j;
                if (rank[u] < 0) continue;
                idx[u] = (int32_t)rows++;
                grp[((size_t)g * G1 + j) * 2 + 1] |= 1u << b;
            }
        }
    return rows;
}

// "" when the plan is admissible, otherwise the reason.  baby_keys [G1] / giant_keys [G2] are only compared with null; a null ARRAY =
// the caller checks no keys (the Python model of the checks)
inline std::string check_plan(uint32_t n, uint64_t t, uint32_t k, uint32_t G1, const uint32_t *baby, uint32_t G2, const uint32_t *giant, const uint64_t *plains,
                              const void *const *baby_keys, const void *const *giant_keys) {
    if (k < 2) return "a special-prime key switch needs a context of at least 2 primes (the last one is the special prime)";
    std::string why = check_elts(n, G1, baby, "baby");
    if (why.empty()) why = check_elts(n, G2, giant, "giant");
    if (!why.empty()) return why;
    if (!plains) return "null argument";
    for (size_t u = 0; u < (size_t)G1 * G2; u++)
        for (uint32_t x = 0; x < n; x++)
            if (plains[u * n + x] >= t)
                return "plaintext of pair (" + std::to_string(u / G1) + ", " + std::to_string(u % G1) + "): coefficient " + std::to_string(x) + " is not below t";
    std::vector<int32_t> idx;
    present_pairs(n, G1, G2, plains, idx);
    for (uint32_t i = 0; i < G2; i++) {
        bool any = false;
        for (uint32_t j = 0; j < G1; j++) any = any || idx[(size_t)i * G1 + j] >= 0;
        if (!any) return "giant step " + std::to_string(i) + " has no present pair (every plaintext of its row is the zero polynomial)";
    }
    for (uint32_t j = 0; j < G1; j++) {
        bool any = false;
        for (uint32_t i = 0; i < G2; i++) any = any || idx[(size_t)i * G1 + j] >= 0;
        if (!any) return "baby step " + std::to_string(j) + " has no present pair (every plaintext of its column is the zero polynomial)";
    }
    if (baby_keys)
        for (uint32_t j = 0; j < G1; j++)
            if (baby[j] != 1 && !baby_keys[j]) return "null key for baby Galois element " + std::to_string(baby[j]);
    if (giant_keys)
        for (uint32_t i = 0; i < G2; i++)
            if (giant[i] != 1 && !giant_keys[i]) return "null key for giant Galois element " + std::to_string(giant[i]);
    return "";
}

// words of scratch for `count` ciphertexts of a context of k primes (L = k - 1) and G2 giant steps: rotdiag's (the digits of c_1
// [L][k][n], C0 [k][n], the outer accumulators B [2][k][n] and their special-prime rows [2][n]) and per giant step the inner accumulators
// A(i) [2][k][n], the special-prime row of A(i)_1 [n], v(i) [L][n] and its digits E(i) [L][k][n]
inline uint64_t scratch_words(uint64_t count, uint32_t k, uint32_t n, uint32_t G2) {
    const uint64_t L = k - 1;
    return count * ((L * k + 3 * (uint64_t)k + 2) + (uint64_t)G2 * (2 * (uint64_t)k + 1 + L + L * k)) * n;
}

}  // namespace rotbsgs
