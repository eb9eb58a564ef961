// Modulus switching through the SEAL facade: loads <count> ciphertexts of <size> polynomials (the records Ciphertext::save writes) in the
// context of all the primes given, runs seal::hip::mod_switch to the first <k_out> of them (seal::hip::level_context), saves the results
// as records of the level context and prints a digest of the output:
//     digest = sum over the output words w_i (i counted through the whole stream) of w_i * (2 i + 1)  mod 2^64
// tests/test_gpu_modswitch.py compares file and digest with the Python path (Evaluator.mod_switch) on the same input.
//   modswitch_check <in> <out> <count> <size> <k_out> <n> <t> <q0> <q1> [q2 ...]
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "seal/hip_circuits.h"

int main(int argc, char **argv) {
    if (argc < 10) {
        std::fprintf(stderr, "usage: %s <in> <out> <count> <size> <k_out> <n> <t> <q0> <q1> [q2 ...]\n", argv[0]);
        return 2;
    }
    const size_t count = (size_t)std::strtoull(argv[3], nullptr, 10);
    const uint32_t size = (uint32_t)std::strtoul(argv[4], nullptr, 10), k_out = (uint32_t)std::strtoul(argv[5], nullptr, 10);
    seal::EncryptionParameters params;
    params.set_poly_modulus("1x^" + std::string(argv[6]) + " + 1");
    std::vector<seal::SmallModulus> q;
    for (int i = 8; i < argc; ++i) q.push_back(seal::SmallModulus(std::strtoull(argv[i], nullptr, 0)));
    params.set_coeff_modulus(q);
    params.set_plain_modulus(std::strtoull(argv[7], nullptr, 0));
    seal::SEALContext context(params);
    seal::SEALContext level = seal::hip::level_context(context, k_out);
    seal::hip::CiphertextBatch in;
    {
        std::ifstream is(argv[1], std::ios::binary);
        if (!is) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 1; }
        in.load(context, is, count, size);
    }
    seal::hip::CiphertextBatch res = seal::hip::mod_switch(context, level, in);
    std::ofstream out(argv[2], std::ios::binary);
    res.save(out);
    out.close();
    if (!out) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 1; }
    const std::vector<uint64_t> words = res.to_host();
    uint64_t digest = 0;
    for (size_t i = 0; i < words.size(); ++i) digest += words[i] * (2 * (uint64_t)i + 1);
    std::printf("modswitch_check: %zu ciphertexts of %u polynomials, %zu -> %u primes digest=%016llx\n", count, size, q.size(), k_out, (unsigned long long)digest);
    return 0;
}
