// Galois rotations through the SEAL facade: loads <count> size-2 ciphertexts (the records Ciphertext::save writes) and a Galois key record
// (seal::hip::GaloisKeys::save; the Python host's GaloisKeys.save writes the same), rotates the rows of every ciphertext left by <steps>
// through seal::hip::rotate_rows, swaps them through seal::hip::rotate_columns if <swap> is 1, saves the results in the same order and
// prints a digest of them:
//     digest = sum over the output words w_i (i counted through the whole stream) of w_i * (2 i + 1)  mod 2^64
// tests/test_gpu_galois.py compares file and digest with the Python path (Evaluator.rotate_rows / rotate_columns) on the same input.
//   galois_check <in> <out> <count> <keys> <steps> <swap 0|1> <n> <t> <q0> [q1 ...]
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "seal/seal.h"

int main(int argc, char **argv) {
    if (argc < 10) {
        std::fprintf(stderr, "usage: %s <in> <out> <count> <keys> <steps> <swap 0|1> <n> <t> <q0> [q1 ...]\n", argv[0]);
        return 2;
    }
    const size_t count = (size_t)std::strtoull(argv[3], nullptr, 10);
    const int steps = std::atoi(argv[5]);
    const bool swap = std::atoi(argv[6]) != 0;
    seal::EncryptionParameters params;
    params.set_poly_modulus("1x^" + std::string(argv[7]) + " + 1");
    std::vector<seal::SmallModulus> q;
    for (int i = 9; i < argc; ++i) q.push_back(seal::SmallModulus(std::strtoull(argv[i], nullptr, 0)));
    params.set_coeff_modulus(q);
    params.set_plain_modulus(std::strtoull(argv[8], nullptr, 0));
    seal::SEALContext context(params);
    std::vector<seal::Ciphertext> cts(count);
    {
        std::ifstream in(argv[1], std::ios::binary);
        if (!in) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 1; }
        for (seal::Ciphertext &c : cts) c.load(in);
    }
    seal::hip::GaloisKeys keys;
    {
        std::ifstream in(argv[4], std::ios::binary);
        if (!in) { std::fprintf(stderr, "cannot open %s\n", argv[4]); return 1; }
        keys.load(in);
    }
    seal::hip::rotate_rows(context, cts, steps, keys);
    if (swap) seal::hip::rotate_columns(context, cts, keys);
    std::ofstream out(argv[2], std::ios::binary);
    uint64_t digest = 0, index = 0;
    for (const seal::Ciphertext &c : cts) {
        c.save(out);
        const uint64_t *p = c.pointer();
        const size_t words = (size_t)c.size() * c.coeff_mod_count() * (c.poly_coeff_count() - 1);
        for (size_t i = 0; i < words; ++i, ++index) digest += p[i] * (2 * index + 1);
    }
    out.close();
    if (!out) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 1; }
    std::printf("galois_check: %zu ciphertexts steps=%d swap=%d digest=%016llx\n", count, steps, (int)swap, (unsigned long long)digest);
    return 0;
}
