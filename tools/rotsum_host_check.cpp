// rotsum_host_check.cpp -- the host arithmetic of a rotate-sum plan (csrc/rotsum_host.h: the checks on the taps and on a call, the slot permutations
// from a transform of X, the weights' residues) in a program of its own, for a CPU build under the host sanitizers:
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/rotsum_host_check.cpp -o rotsum_host_check
// No device, no library.  It builds the transform of X itself, in two slot orders, and compares every permutation with the definition:
// pi_g(NTT(a)) = NTT(sigma_g(a)) on a random polynomial, by direct evaluation.  Exit status 0 and "ok" when everything holds.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../fully-homomorphic-image-processing_amd/csrc/rotsum_host.h"

using rotsum::mulmod;

static uint64_t powmod(uint64_t a, uint64_t e, uint64_t q) {
    uint64_t r = 1;
    for (a %= q; e; e >>= 1, a = mulmod(a, a, q))
        if (e & 1) r = mulmod(r, a, q);
    return r;
}
static int fails = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); fails++; } \
    } while (0)

static uint32_t bitrev(uint32_t v, int bits) {
    uint32_t r = 0;
    for (int i = 0; i < bits; i++) r |= ((v >> i) & 1u) << (bits - 1 - i);
    return r;
}

// a(psi^e) for every slot's exponent e
static std::vector<uint64_t> evaluate(const std::vector<uint64_t> &a, const std::vector<uint32_t> &expo, uint64_t psi, uint64_t q) {
    std::vector<uint64_t> out(expo.size());
    for (size_t s = 0; s < expo.size(); s++) {
        const uint64_t x = powmod(psi, expo[s], q);
        uint64_t acc = 0;
        for (size_t j = a.size(); j-- > 0;) acc = (mulmod(acc, x, q) + a[j]) % q;
        out[s] = acc;
    }
    return out;
}

static void one_order(uint32_t n, uint64_t q, uint64_t psi, const std::vector<uint32_t> &expo, std::mt19937_64 &rng) {
    std::vector<uint64_t> X(n, 0), a(n);
    X[1] = 1;
    for (auto &v : a) v = rng() % q;
    const std::vector<uint64_t> xhat = evaluate(X, expo, psi, q), ahat = evaluate(a, expo, psi, q);
    std::vector<uint32_t> f;
    CHECK(rotsum::slot_exponents(xhat.data(), n, q, f));
    CHECK(f.size() == n && f[0] == 1);
    const uint32_t gs[] = {1, 3, 2 * n - 1, (uint32_t)powmod(3, n / 8, 2 * n), (uint32_t)powmod(3, n / 2 - 1, 2 * n), 5, 2 * n - 3};
    for (uint32_t g : gs) {
        std::vector<uint32_t> perm(n, n);
        CHECK(rotsum::slot_perm(f, g, perm.data()));
        std::vector<uint64_t> sa(n, 0);                                   // sigma_g(a)
        for (uint32_t j = 0; j < n; j++) {
            const uint32_t e = (uint32_t)(((uint64_t)j * g) % (2 * n));
            sa[e % n] = e >= n ? (q - a[j]) % q : a[j];
        }
        const std::vector<uint64_t> want = evaluate(sa, expo, psi, q);
        bool same = true, bijective = true;
        std::vector<char> hit(n, 0);
        for (uint32_t s = 0; s < n; s++) {
            if (perm[s] >= n || hit[perm[s]]) { bijective = false; break; }
            hit[perm[s]] = 1;
            same = same && ahat[perm[s]] == want[s];
        }
        CHECK(bijective);
        CHECK(same);
        if (g == 1)
            for (uint32_t s = 0; s < n; s++) CHECK(perm[s] == s);
    }
    std::vector<uint32_t> perm(n);
    CHECK(!rotsum::slot_perm(f, 2, perm.data()));                         // even
    CHECK(!rotsum::slot_perm(f, 2 * n + 1, perm.data()));                 // out of range
    // not a transform of X: a repeated value, a value that is no power of the first one, zero
    std::vector<uint64_t> bad = xhat;
    bad[n - 1] = bad[1];
    CHECK(!rotsum::slot_exponents(bad.data(), n, q, f));
    bad = xhat;
    bad[2] = mulmod(bad[2], 2, q);                                        // an even power, a value another slot holds, or no power at all
    CHECK(!rotsum::slot_exponents(bad.data(), n, q, f));
    bad = xhat;
    bad[0] = 0;
    CHECK(!rotsum::slot_exponents(bad.data(), n, q, f));
    bad.assign(n, 1);                                                     // the order of rho is 1
    CHECK(!rotsum::slot_exponents(bad.data(), n, q, f));
}

int main() {
    std::mt19937_64 rng(7);
    // q = 1 (mod 2n) for n = 16, 64: 12289 = 3 * 2^12 + 1; 65537
    const uint64_t qs[] = {12289, 65537};
    for (uint64_t q : qs)
        for (uint32_t n : {16u, 64u}) {
            uint64_t psi = 0;
            for (uint64_t z = 2; z < q && !psi; z++) {
                const uint64_t c = powmod(z, (q - 1) / (2 * n), q);
                if (powmod(c, n, q) == q - 1) psi = c;
            }
            CHECK(psi != 0);
            int bits = 0;
            while ((1u << bits) < n) bits++;
            std::vector<uint32_t> br(n), grouped(n);
            for (uint32_t s = 0; s < n; s++) br[s] = 2 * bitrev(s, bits) + 1;                       // the bit-reversed order
            for (uint32_t s = 0; s < n; s++) grouped[s] = (uint32_t)powmod(3, s % (n / 2), 2 * n);  // rows of 3^j and -3^j
            for (uint32_t s = n / 2; s < n; s++) grouped[s] = 2 * n - grouped[s];
            one_order(n, q, psi, br, rng);
            one_order(n, q, psi, grouped, rng);
        }
    // the checks on the taps
    const uint32_t n = 1024;
    const uint64_t t = 65537;
    const int dummy = 0;
    const void *key = &dummy;
    {
        const uint32_t e[] = {1, 3, 2 * n - 1};
        const uint64_t w[] = {1, t - 1, (t + 1) / 2};
        const void *k[] = {nullptr, key, key};
        CHECK(rotsum::check_taps(n, t, 2, 3, e, w, k).empty());
        CHECK(rotsum::check_taps(n, t, 2, 3, e, w, nullptr).empty());
        CHECK(!rotsum::check_taps(n, t, 1, 3, e, w, k).empty());          // k < 2
        CHECK(!rotsum::check_taps(n, t, 2, 0, e, w, k).empty());          // no tap
        CHECK(!rotsum::check_taps(n, t, 2, 65, e, w, k).empty());         // refused before anything is read
        CHECK(!rotsum::check_taps(n, t, 2, 3, nullptr, w, k).empty());
        const void *k0[] = {nullptr, nullptr, key};
        CHECK(!rotsum::check_taps(n, t, 2, 3, e, w, k0).empty());         // null key for g = 3
        const uint64_t w0[] = {1, 2 * t, 5};
        CHECK(!rotsum::check_taps(n, t, 2, 3, e, w0, k).empty());         // weight 0 modulo t
        const uint32_t even[] = {1, 4, 5}, big[] = {1, 3, 2 * n + 1}, twice[] = {3, 5, 3};
        CHECK(!rotsum::check_taps(n, t, 2, 3, even, w, k).empty());
        CHECK(!rotsum::check_taps(n, t, 2, 3, big, w, k).empty());
        CHECK(!rotsum::check_taps(n, t, 2, 3, twice, w, k).empty());
    }
    {
        std::vector<uint32_t> e(64);
        std::vector<uint64_t> w(64, 1);
        for (uint32_t j = 0; j < 64; j++) e[j] = 2 * j + 1;
        CHECK(rotsum::check_taps(n, t, 2, 64, e.data(), w.data(), nullptr).empty());
    }
    // the call check of the four rotation entry points: made-up addresses, nothing is dereferenced.  k = 3 primes of n = 1024: a size-2
    // ciphertext is ctw = 4096 words; 2 ciphertexts in, 2 out, 1000 words (8000 bytes) of scratch
    {
        const uint32_t ck = 3;
        const uint64_t ctw = 2 * (uint64_t)(ck - 1) * n, count = 2, launch = count * ck * ck;
        const size_t need = 8000;
        const auto at = [](uint64_t word) { return (const void *)(uintptr_t)(0x10000000ULL + 8 * word); };
        const void *ct = at(0), *out = at(100000), *scr = at(200000);
        const auto has = [](const std::string &why, const char *word) { return why.find(word) != std::string::npos; };
        const auto sum = [&](const void *c, uint64_t stride, const void *o, uint64_t ostride, uint64_t cnt, uint64_t lnch, const void *s, size_t bytes) {
            return rotsum::check_call(ck, n, c, stride, o, ostride, cnt, lnch, need, s, bytes);
        };
        const auto each = [&](const void *c, const void *o, uint64_t tap_stride, const void *s) {
            return rotsum::check_call(ck, n, c, ctw, o, ctw, count, launch, need, s, need, 3, tap_stride);
        };
        CHECK(sum(ct, ctw, out, ctw, count, launch, scr, need).empty());
        CHECK(sum(ct, ctw + 8, out, ctw + 24, count, launch, scr, need + 1).empty());                 // padded strides, a larger buffer
        CHECK(each(ct, out, count * ctw, scr).empty());
        // every refusal, one at a time, by the word the callers' tests look for
        std::string why = sum(ct, ctw - 1, out, ctw, count, launch, scr, need);
        CHECK(has(why, "ciphertext stride") && has(why, "of 2 primes"));
        why = sum(ct, ctw, out, ctw - 1, count, launch, scr, need);
        CHECK(has(why, "output stride") && has(why, "of 2 primes"));
        CHECK(has(sum(ct, ctw, out, ctw, count, 0x80000000ULL, scr, need), "too many"));
        CHECK(sum(ct, ctw, out, ctw, count, 0x7fffffffULL, scr, need).empty());
        CHECK(has(each(ct, out, count * ctw - 1, scr), "tap stride"));
        CHECK(has(sum(ct, ctw, out, ctw, count, launch, scr, need - 1), "scratch too small"));
        CHECK(has(sum(ct, ctw, out, ctw, count, launch, nullptr, need), "scratch too small"));
        why = sum(ct, ctw, at(2 * ctw - 1), ctw, count, launch, scr, need);                           // the last input word is the first output word
        CHECK(has(why, "overlaps") && !has(why, "scratch overlaps") && has(why, "only out2 == ct2"));
        CHECK(sum(ct, ctw, at(2 * ctw), ctw, count, launch, scr, need).empty());                      // adjacent ranges share no word
        CHECK(has(sum(ct, ctw, out, ctw, count, launch, at(2 * ctw - 1), need), "scratch overlaps"));     // scratch on the input's last word
        CHECK(has(sum(ct, ctw, out, ctw, count, launch, at(100000 - 1000 + 1), need), "scratch overlaps"));   // scratch's last word on the output's first
        CHECK(sum(ct, ctw, out, ctw, count, launch, at(100000 - 1000), need).empty());
        // the order of the refusals: strides, the launch size, the tap stride, scratch, the operands' overlap, scratch's overlap
        CHECK(has(sum(ct, ctw - 1, out, ctw - 1, count, 0x80000000ULL, nullptr, 0), "ciphertext stride"));
        CHECK(has(sum(ct, ctw, out, ctw - 1, count, 0x80000000ULL, nullptr, 0), "output stride"));
        CHECK(has(sum(ct, ctw, ct, ctw + 8, count, 0x80000000ULL, nullptr, 0), "too many"));
        CHECK(has(rotsum::check_call(ck, n, ct, ctw, ct, ctw, count, launch, need, nullptr, 0, 3, 1), "tap stride"));
        CHECK(has(sum(ct, ctw, ct, ctw + 8, count, launch, nullptr, 0), "scratch too small"));
        why = sum(ct, ctw, ct, ctw + 8, count, launch, ct, need);
        CHECK(has(why, "overlaps") && !has(why, "scratch overlaps"));
        // no ciphertext: clean after the strides, whatever the rest is
        CHECK(sum(ct, ctw, ct, ctw + 8, 0, ~0ULL, nullptr, 0).empty());
        CHECK(rotsum::check_call(ck, n, ct, ctw, ct, ctw, 0, ~0ULL, need, nullptr, 0, 3, 0).empty());
        CHECK(has(sum(ct, ctw - 1, out, ctw, 0, launch, scr, need), "ciphertext stride"));
        // in place: out == ct with equal strides for the sums, never for fhe_rotate_each_sp; the same pointer with another stride is refused
        CHECK(sum(ct, ctw, ct, ctw, count, launch, scr, need).empty());
        CHECK(sum(ct, ctw + 8, ct, ctw + 8, count, launch, scr, need).empty());
        why = each(ct, ct, count * ctw, scr);
        CHECK(has(why, "overlaps") && has(why, "no in-place form"));
        why = sum(ct, ctw, ct, ctw + 8, count, launch, scr, need);
        CHECK(has(why, "overlaps") && has(why, "only out2 == ct2"));
        CHECK(each(at(3 * count * ctw), at(0), count * ctw, scr).empty());                            // the LAST tap's batch ends just before the input
        CHECK(has(each(at(3 * count * ctw - 1), at(0), count * ctw, scr), "overlaps"));               // ... and on its first word
    }
    // centred lifts
    const uint64_t q = 0x3FFFFFFF000001ULL;
    CHECK(rotsum::weight_residue(1, t, q) == 1);
    CHECK(rotsum::weight_residue(t - 1, t, q) == q - 1);
    CHECK(rotsum::weight_residue((t - 1) / 2, t, q) == (t - 1) / 2);
    CHECK(rotsum::weight_residue((t + 1) / 2, t, q) == q - (t - 1) / 2);
    CHECK(rotsum::weight_residue(t + 3, t, q) == 3);
    CHECK(rotsum::weight_residue(t - 1, t, 3) == 2);                      // q below t: -1 mod 3
    if (fails) {
        std::printf("%d check(s) failed\n", fails);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
