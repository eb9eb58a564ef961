// rotbsgs_host_check.cpp -- the host arithmetic a baby-step / giant-step plan adds to a rotate-diag plan's (csrc/rotbsgs_host.h: the checks
// on the two element lists, the plaintexts and the keys, the table of the present pairs, the scratch formula) in a program of its own, for a
// CPU build under the host sanitizers:
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/rotbsgs_host_check.cpp -o rotbsgs_host_check
// No device, no library.  Exit status 0 and "ok" when everything holds.
#include <cstdio>
#include <random>

#include "../fully-homomorphic-image-processing_amd/csrc/rotbsgs_host.h"

static int fails = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); fails++; } \
    } while (0)

static bool has(const std::string &s, const std::string &what) { return s.find(what) != std::string::npos; }

int main() {
    const uint64_t t = 65537;
    const uint32_t shapes[][2] = {{1, 1}, {3, 1}, {1, 2}, {4, 3}, {16, 8}, {64, 64}, {5, 9}};
    for (uint32_t n : {8u, 64u, 256u}) {
        for (const auto &sh : shapes) {
            const uint32_t G1 = sh[0], G2 = sh[1];
            if (G1 > n || G2 > n) continue;                             // n odd elements below 2n
            std::mt19937_64 rng(n * 131 + G1 * 7 + G2);
            std::vector<uint32_t> baby(G1), giant(G2);
            for (uint32_t j = 0; j < G1; j++) baby[j] = 2 * j + 1;      // 1 first
            for (uint32_t i = 0; i < G2; i++) giant[i] = 2 * n - 1 - 2 * i;
            std::vector<uint64_t> p((size_t)G1 * G2 * n);
            for (auto &v : p) v = rng() % t;
            for (size_t u = 0; u < (size_t)G1 * G2; u++) p[u * n + n - 1] = t - 1;
            std::vector<const void *> kb(G1, &fails), kg(G2, &fails);
            kb[0] = nullptr;                                            // the element 1 needs no key
            CHECK(rotbsgs::check_plan(n, t, 3, G1, baby.data(), G2, giant.data(), p.data(), kb.data(), kg.data()).empty());
            CHECK(rotbsgs::check_plan(n, t, 3, G1, baby.data(), G2, giant.data(), p.data(), nullptr, nullptr).empty());
            CHECK(has(rotbsgs::check_plan(n, t, 1, G1, baby.data(), G2, giant.data(), p.data(), nullptr, nullptr), "at least 2 primes"));
            CHECK(has(rotbsgs::check_plan(n, t, 3, 0, baby.data(), G2, giant.data(), p.data(), nullptr, nullptr), "baby step count"));
            CHECK(has(rotbsgs::check_plan(n, t, 3, G1, baby.data(), 65, giant.data(), p.data(), nullptr, nullptr), "giant step count"));
            CHECK(has(rotbsgs::check_plan(n, t, 3, G1, nullptr, G2, giant.data(), p.data(), nullptr, nullptr), "null"));
            CHECK(has(rotbsgs::check_plan(n, t, 3, G1, baby.data(), G2, giant.data(), nullptr, nullptr, nullptr), "null"));
            // a null key for a non-identity element, in either list
            if (G1 > 1) {
                auto bad = kb;
                bad[G1 - 1] = nullptr;
                CHECK(has(rotbsgs::check_plan(n, t, 3, G1, baby.data(), G2, giant.data(), p.data(), bad.data(), kg.data()), "null key for baby"));
            }
            {
                auto bad = kg;
                bad[0] = nullptr;                                       // giant[0] = 2n - 1 is never the element 1
                CHECK(has(rotbsgs::check_plan(n, t, 3, G1, baby.data(), G2, giant.data(), p.data(), kb.data(), bad.data()), "null key for giant"));
            }
            // elements: even, out of range, repeated
            for (uint32_t g : {0u, 4u, 2 * n, 2 * n + 1}) {
                auto bad = giant;
                bad[G2 - 1] = g;
                CHECK(has(rotbsgs::check_plan(n, t, 3, G1, baby.data(), G2, bad.data(), p.data(), nullptr, nullptr), "giant Galois element"));
            }
            if (G1 > 1) {
                auto bad = baby;
                bad[G1 - 1] = bad[0];
                CHECK(has(rotbsgs::check_plan(n, t, 3, G1, bad.data(), G2, giant.data(), p.data(), nullptr, nullptr), "repeated"));
            }
            // the last coefficient of the last pair at t and above
            std::vector<uint64_t> bad = p;
            bad.back() = t;
            CHECK(has(rotbsgs::check_plan(n, t, 3, G1, baby.data(), G2, giant.data(), bad.data(), nullptr, nullptr), "not below t"));
            bad.back() = ~0ULL;
            CHECK(has(rotbsgs::check_plan(n, t, 3, G1, baby.data(), G2, giant.data(), bad.data(), nullptr, nullptr), "not below t"));
            // a whole giant row absent; a whole baby column absent
            bad = p;
            for (size_t x = 0; x < (size_t)G1 * n; x++) bad[(size_t)(G2 - 1) * G1 * n + x] = 0;
            CHECK(has(rotbsgs::check_plan(n, t, 3, G1, baby.data(), G2, giant.data(), bad.data(), nullptr, nullptr), "giant step " + std::to_string(G2 - 1) + " has no present pair"));
            if (G1 > 1) {
                bad = p;
                for (uint32_t i = 0; i < G2; i++)
                    for (uint32_t x = 0; x < n; x++) bad[((size_t)i * G1 + G1 - 1) * n + x] = 0;
                CHECK(has(rotbsgs::check_plan(n, t, 3, G1, baby.data(), G2, giant.data(), bad.data(), nullptr, nullptr), "baby step " + std::to_string(G1 - 1) + " has no present pair"));
            }
            // absent pairs on a checkerboard (when both lists have more than one entry every row and column keeps a pair)
            bad = p;
            uint32_t want = 0;
            for (uint32_t i = 0; i < G2; i++)
                for (uint32_t j = 0; j < G1; j++) {
                    const bool gone = G1 > 1 && G2 > 1 && ((i + j) & 1);
                    if (gone) for (uint32_t x = 0; x < n; x++) bad[((size_t)i * G1 + j) * n + x] = 0;
                    want += !gone;
                }
            CHECK(rotbsgs::check_plan(n, t, 3, G1, baby.data(), G2, giant.data(), bad.data(), nullptr, nullptr).empty());
            std::vector<int32_t> rank, idx;
            std::vector<uint32_t> grp;
            CHECK(rotbsgs::present_pairs(n, G1, G2, bad.data(), rank) == want);
            CHECK(rotbsgs::group_rows(n, G1, G2, bad.data(), idx, grp) == want);
            const uint32_t GG = rotbsgs::GIANT_GROUP, groups = (G2 + GG - 1) / GG;
            CHECK(grp.size() == (size_t)groups * G1 * 2 && idx.size() == (size_t)G1 * G2);
            std::vector<char> seen(want, 0);
            for (uint32_t i = 0; i < G2; i++)
                for (uint32_t j = 0; j < G1; j++) {
                    const size_t u = (size_t)i * G1 + j;
                    const uint32_t base = grp[((size_t)(i / GG) * G1 + j) * 2], mask = grp[((size_t)(i / GG) * G1 + j) * 2 + 1];
                    CHECK((rank[u] >= 0) == (idx[u] >= 0) && (idx[u] >= 0) == (bool)(mask >> (i % GG) & 1));
                    if (idx[u] < 0) continue;
                    CHECK((uint32_t)idx[u] < want && !seen[idx[u]]);
                    if ((uint32_t)idx[u] < want) seen[idx[u]] = 1;
                    CHECK((uint32_t)idx[u] == base + (uint32_t)__builtin_popcount(mask & ((1u << (i % GG)) - 1)));      // the kernels' way to the row
                }
            for (uint32_t g = 0; g < groups; g++)
                for (uint32_t j = 0; j < G1; j++) CHECK((grp[((size_t)g * G1 + j) * 2 + 1] >> GG) == 0 && grp[((size_t)g * G1 + j) * 2] <= want);
        }
    }
    // the scratch formula: rotdiag's words and per giant step A [2][k][n], the special row [n], v [L][n], E [L][k][n]
    CHECK(rotbsgs::scratch_words(1, 4, 1024, 1) == (uint64_t)1024 * ((12 + 12 + 2) + (8 + 1 + 3 + 12)));
    CHECK(rotbsgs::scratch_words(3, 2, 8, 64) == (uint64_t)3 * 8 * ((2 + 6 + 2) + 64 * (4 + 1 + 1 + 2)));
    CHECK(rotbsgs::scratch_words(0, 4, 1024, 8) == 0);
    CHECK(rotbsgs::scratch_words(1u << 20, 8, 16384, 64) == ((uint64_t)1 << 20) * 16384 * ((56 + 24 + 2) + 64 * (16 + 1 + 7 + 56)));
    if (fails) return 1;
    std::printf("ok\n");
    return 0;
}
