// rotdiag_host_check.cpp -- the host arithmetic a rotate-diag plan adds to a rotate-sum plan's (csrc/rotdiag_host.h: the checks on the
// plaintexts, their centred lift to every prime) in a program of its own, for a CPU build under the host sanitizers:
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/rotdiag_host_check.cpp -o rotdiag_host_check
// No device, no library.  Exit status 0 and "ok" when everything holds.
#include <cstdio>
#include <random>

#include "../fully-homomorphic-image-processing_amd/csrc/rotdiag_host.h"

static int fails = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); fails++; } \
    } while (0)

int main() {
    const uint64_t t = 65537;
    const uint64_t primes[3] = {0x3fffffffd8001ULL, (1ULL << 61) - 20479, 65537 * 2 + 1};      // a 50-bit one, a 61-bit one, one just above t
    for (uint32_t n : {2u, 64u, 1024u}) {
        for (uint32_t taps : {1u, 3u, 64u}) {
            std::mt19937_64 rng(n * 131 + taps);
            std::vector<uint64_t> p((size_t)taps * n);
            for (auto &v : p) v = rng() % t;
            p[0] = 1;                                                   // no tap is all zero whatever the draw
            for (uint32_t j = 0; j < taps; j++) p[(size_t)j * n + n - 1] = t - 1;
            CHECK(rotdiag::check_plains(n, t, taps, p.data()).empty());
            CHECK(!rotdiag::check_plains(n, t, taps, nullptr).empty());
            // the last coefficient of the last tap at t: refused, and named
            std::vector<uint64_t> bad = p;
            bad.back() = t;
            CHECK(rotdiag::check_plains(n, t, taps, bad.data()).find("not below t") != std::string::npos);
            bad.back() = ~0ULL;
            CHECK(rotdiag::check_plains(n, t, taps, bad.data()).find("not below t") != std::string::npos);
            // the last tap all zero
            bad = p;
            for (uint32_t x = 0; x < n; x++) bad[(size_t)(taps - 1) * n + x] = 0;
            CHECK(rotdiag::check_plains(n, t, taps, bad.data()).find("zero polynomial") != std::string::npos);
            // the lift: canonical, congruent to the centred value, on every prime
            std::vector<uint64_t> out((size_t)3 * n, ~0ULL);
            for (uint32_t j = 0; j < taps; j++) {
                rotdiag::lift(p.data() + (size_t)j * n, n, t, primes, 3, out.data());
                for (uint32_t r = 0; r < 3; r++)
                    for (uint32_t x = 0; x < n; x++) {
                        const uint64_t v = p[(size_t)j * n + x], got = out[(size_t)r * n + x], q = primes[r];
                        CHECK(got < q);
                        if (2 * v > t) CHECK((got + (t - v)) % q == 0);
                        else CHECK(got == v % q);
                    }
            }
        }
    }
    // the edges of the centred lift: (t - 1) / 2 stays, (t + 1) / 2 becomes negative
    uint64_t edge[4] = {0, (t - 1) / 2, (t + 1) / 2, t - 1}, out[4];
    rotdiag::lift(edge, 4, t, primes, 1, out);
    CHECK(out[0] == 0 && out[1] == (t - 1) / 2 && out[2] == primes[0] - (t - 1) / 2 && out[3] == primes[0] - 1);
    if (fails) return 1;
    std::printf("ok\n");
    return 0;
}
