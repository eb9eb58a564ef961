// rotdiag_host.h -- the host arithmetic a rotate-diag plan adds to rotsum_host.h (rotdiag.hip, include/fhe_hip.h fhe_rotdiag_plan_create):
// the checks on the plaintexts and their centred lift to every prime.  The checks on the elements and keys, the slot permutations and the
// check on a call's operands are rotsum_host.h's.  No device, no HIP header: tools/rotdiag_host_check.cpp builds it alone, under the host sanitizers.
#pragma once
#include "rotsum_host.h"

namespace rotdiag {

// "" when the plaintexts are admissible, otherwise the reason.  plains [taps][n], coefficients modulo t
inline std::string check_plains(uint32_t n, uint64_t t, uint32_t taps, const uint64_t *plains) {
    if (!plains) return "null argument";
    for (uint32_t j = 0; j < taps; j++) {
        const uint64_t *p = plains + (size_t)j * n;
        bool zero = true;
        for (uint32_t x = 0; x < n; x++) {
            if (p[x] >= t) return "plaintext of tap " + std::to_string(j) + ": coefficient " + std::to_string(x) + " is not below t";
            zero = zero && p[x] == 0;
        }
        if (zero) return "plaintext of tap " + std::to_string(j) + " is the zero polynomial";
    }
    return "";
}

// out [k][n]: the centred lift of p [n] (coefficients in (-t/2, t/2]) reduced to every prime, canonical
inline void lift(const uint64_t *p, uint32_t n, uint64_t t, const uint64_t *primes, uint32_t k, uint64_t *out) {
    for (uint32_t r = 0; r < k; r++)
        for (uint32_t x = 0; x < n; x++) out[(size_t)r * n + x] = rotsum::weight_residue(p[x], t, primes[r]);
}

}  // namespace rotdiag
