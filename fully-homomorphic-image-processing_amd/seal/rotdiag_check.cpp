// Diagonal linear maps on encrypted slots through the SEAL facade: loads <count> size-2 ciphertexts over the first k - 1 of the primes given
// (the records Ciphertext::save writes, in the level context), a set of special-prime Galois keys and a list of taps with their diagonals
// (both written by the Python test), runs seal::hip::rotate_diag_sum_sp (in place) on the batch, saves the results and prints a digest of
// what it saved:
//     digest = sum over the output words w_i of w_i * (2 i + 1)  mod 2^64
// tests/test_gpu_rotdiag_hosts.py compares file and digest with the Python host on the same input.
//   galois keys file: per element u32 element, u32 reserved, then the words of [k - 1][2][k][n]
//   taps file:        per tap u32 element, u32 reserved, then n u64 slot values (flat row order)
//   rotdiag_check <in> <out> <count> <galois keys> <taps> <n> <t> <q0> <q1> [q2 ...]
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "seal/hip_circuits.h"

int main(int argc, char **argv) {
    if (argc < 10) {
        std::fprintf(stderr, "usage: %s <in> <out> <count> <galois keys> <taps> <n> <t> <q0> <q1> [q2 ...]\n", argv[0]);
        return 2;
    }
    const size_t count = (size_t)std::strtoull(argv[3], nullptr, 10);
    const size_t n = (size_t)std::strtoull(argv[6], nullptr, 10);
    seal::EncryptionParameters params;
    params.set_poly_modulus("1x^" + std::string(argv[6]) + " + 1");
    std::vector<seal::SmallModulus> q;
    for (int i = 8; i < argc; ++i) q.push_back(seal::SmallModulus(std::strtoull(argv[i], nullptr, 0)));
    params.set_coeff_modulus(q);
    params.set_plain_modulus(std::strtoull(argv[7], nullptr, 0));
    seal::SEALContext parent(params);
    seal::SEALContext level = seal::hip::level_context(parent, (uint32_t)q.size() - 1);
    const size_t kw = fhe_ksk_sp_words(parent.state()->h);
    seal::hip::CiphertextBatch cts;
    {
        std::ifstream is(argv[1], std::ios::binary);
        if (!is) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 1; }
        cts.load(level, is, count, 2);
    }
    seal::hip::SpecialGaloisKeys gkeys;
    {
        std::ifstream is(argv[4], std::ios::binary);
        if (!is) { std::fprintf(stderr, "cannot open %s\n", argv[4]); return 1; }
        uint32_t hdr[2];
        std::vector<uint64_t> words(kw);
        while (is.read((char *)hdr, sizeof hdr)) {
            is.read((char *)words.data(), (std::streamsize)(kw * 8));
            if (!is) { std::fprintf(stderr, "truncated Galois key in %s\n", argv[4]); return 1; }
            gkeys.add(hdr[0], seal::hip::SpecialKeys(parent, words, 1));
        }
    }
    std::vector<uint32_t> elements;
    std::vector<uint64_t> diagonals;
    {
        std::ifstream is(argv[5], std::ios::binary);
        if (!is) { std::fprintf(stderr, "cannot open %s\n", argv[5]); return 1; }
        uint32_t hdr[2];
        std::vector<uint64_t> row(n);
        while (is.read((char *)hdr, sizeof hdr)) {
            is.read((char *)row.data(), (std::streamsize)(n * 8));
            if (!is) { std::fprintf(stderr, "truncated diagonal in %s\n", argv[5]); return 1; }
            elements.push_back(hdr[0]);
            diagonals.insert(diagonals.end(), row.begin(), row.end());
        }
    }
    seal::hip::RotDiagPlan plan(parent, gkeys, elements, diagonals);
    seal::hip::rotate_diag_sum_sp(parent, level, cts, plan);
    std::ofstream out(argv[2], std::ios::binary);
    cts.save(out);
    out.close();
    if (!out) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 1; }
    const std::vector<uint64_t> words = cts.to_host();
    uint64_t digest = 0;
    for (size_t i = 0; i < words.size(); ++i) digest += words[i] * (2 * (uint64_t)i + 1);
    std::printf("rotdiag_check: %zu ciphertexts, %zu taps digest=%016llx\n", count, elements.size(), (unsigned long long)digest);
    return 0;
}
