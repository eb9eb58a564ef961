// Baby-step / giant-step linear maps on encrypted slots through the SEAL facade: loads <count> size-2 ciphertexts over the first k - 1 of the
// primes given (the records Ciphertext::save writes, in the level context), a set of special-prime Galois keys and a plan (both written by
// the Python test), runs seal::hip::rotate_bsgs_sp (in place) on the batch, saves the results and prints a digest of what it saved:
//     digest = sum over the output words w_i of w_i * (2 i + 1)  mod 2^64
// tests/test_gpu_rotbsgs_hosts.py compares file and digest with the Python host on the same input.
//   galois keys file: per element u32 element, u32 reserved, then the words of [k - 1][2][k][n]
//   plan file:        u32 G1, u32 G2, G1 u32 baby elements, G2 u32 giant elements, then [G2][G1][n] u64 slot values (flat row order)
//   rotbsgs_check <in> <out> <count> <galois keys> <plan> <n> <t> <q0> <q1> [q2 ...]
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "seal/hip_circuits.h"

int main(int argc, char **argv) {
    if (argc < 10) {
        std::fprintf(stderr, "usage: %s <in> <out> <count> <galois keys> <plan> <n> <t> <q0> <q1> [q2 ...]\n", argv[0]);
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
    std::vector<uint32_t> baby, giant;
    std::vector<uint64_t> diagonals;
    {
        std::ifstream is(argv[5], std::ios::binary);
        if (!is) { std::fprintf(stderr, "cannot open %s\n", argv[5]); return 1; }
        uint32_t hdr[2];
        if (!is.read((char *)hdr, sizeof hdr) || hdr[0] > 64 || hdr[1] > 64) { std::fprintf(stderr, "bad plan header in %s\n", argv[5]); return 1; }
        baby.resize(hdr[0]);
        giant.resize(hdr[1]);
        diagonals.resize((size_t)hdr[0] * hdr[1] * n);
        is.read((char *)baby.data(), (std::streamsize)(baby.size() * 4));
        is.read((char *)giant.data(), (std::streamsize)(giant.size() * 4));
        is.read((char *)diagonals.data(), (std::streamsize)(diagonals.size() * 8));
        if (!is) { std::fprintf(stderr, "truncated plan in %s\n", argv[5]); return 1; }
    }
    seal::hip::RotBsgsPlan plan(parent, gkeys, baby, giant, diagonals);
    seal::hip::rotate_bsgs_sp(parent, level, cts, plan);
    std::ofstream out(argv[2], std::ios::binary);
    cts.save(out);
    out.close();
    if (!out) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 1; }
    const std::vector<uint64_t> words = cts.to_host();
    uint64_t digest = 0;
    for (size_t i = 0; i < words.size(); ++i) digest += words[i] * (2 * (uint64_t)i + 1);
    std::printf("rotbsgs_check: %zu ciphertexts, %zu x %zu steps digest=%016llx\n", count, baby.size(), giant.size(), (unsigned long long)digest);
    return 0;
}
