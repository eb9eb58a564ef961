// Key switching with a special prime through the SEAL facade: loads <count> ciphertexts of <size> polynomials over the first k - 1 of the
// primes given (the records Ciphertext::save writes, in the level context), the special-prime evaluation keys for s^2 .. s^(size-1) and a
// set of special-prime Galois keys (both written by the Python test from KeyGenerator's tensors), relinearises every ciphertext through
// seal::hip::relinearize_sp when <size> is above 2, rotates the rows left by <steps> through seal::hip::rotate_rows_sp, swaps them through
// seal::hip::rotate_columns_sp if <swap> is 1, saves the results and prints a digest of them:
//     digest = sum over the output words w_i (i counted through the whole stream) of w_i * (2 i + 1)  mod 2^64
// tests/test_gpu_keyswitch_sp_hosts.py compares file and digest with the Python path on the same input.
//   relin keys file:  the words of [size - 2][k - 1][2][k][n], NTT form (absent sets: an empty file)
//   galois keys file: per element u32 element, u32 reserved, then the words of [k - 1][2][k][n]
//   keyswitch_sp_check <in> <out> <count> <size> <relin keys> <galois keys> <steps> <swap 0|1> <n> <t> <q0> <q1> [q2 ...]
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "seal/hip_circuits.h"

int main(int argc, char **argv) {
    if (argc < 13) {
        std::fprintf(stderr, "usage: %s <in> <out> <count> <size> <relin keys> <galois keys> <steps> <swap 0|1> <n> <t> <q0> <q1> [q2 ...]\n", argv[0]);
        return 2;
    }
    const size_t count = (size_t)std::strtoull(argv[3], nullptr, 10);
    const uint32_t size = (uint32_t)std::strtoul(argv[4], nullptr, 10);
    const int steps = std::atoi(argv[7]);
    const bool swap = std::atoi(argv[8]) != 0;
    seal::EncryptionParameters params;
    params.set_poly_modulus("1x^" + std::string(argv[9]) + " + 1");
    std::vector<seal::SmallModulus> q;
    for (int i = 11; i < argc; ++i) q.push_back(seal::SmallModulus(std::strtoull(argv[i], nullptr, 0)));
    params.set_coeff_modulus(q);
    params.set_plain_modulus(std::strtoull(argv[10], nullptr, 0));
    seal::SEALContext parent(params);
    seal::SEALContext level = seal::hip::level_context(parent, (uint32_t)q.size() - 1);
    const size_t kw = fhe_ksk_sp_words(parent.state()->h);
    seal::hip::CiphertextBatch cts;
    {
        std::ifstream is(argv[1], std::ios::binary);
        if (!is) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 1; }
        cts.load(level, is, count, size);
    }
    if (size > 2) {
        std::ifstream is(argv[5], std::ios::binary);
        std::vector<uint64_t> words((size_t)(size - 2) * kw);
        is.read((char *)words.data(), (std::streamsize)(words.size() * 8));
        if (!is) { std::fprintf(stderr, "cannot read %u key sets from %s\n", size - 2, argv[5]); return 1; }
        cts = seal::hip::relinearize_sp(parent, level, cts, seal::hip::SpecialKeys(parent, words, size - 2));
    }
    seal::hip::SpecialGaloisKeys gkeys;
    {
        std::ifstream is(argv[6], std::ios::binary);
        if (!is) { std::fprintf(stderr, "cannot open %s\n", argv[6]); return 1; }
        uint32_t hdr[2];
        std::vector<uint64_t> words(kw);
        while (is.read((char *)hdr, sizeof hdr)) {
            is.read((char *)words.data(), (std::streamsize)(kw * 8));
            if (!is) { std::fprintf(stderr, "truncated Galois key in %s\n", argv[6]); return 1; }
            gkeys.add(hdr[0], seal::hip::SpecialKeys(parent, words, 1));
        }
    }
    seal::hip::rotate_rows_sp(parent, level, cts, steps, gkeys);
    if (swap) seal::hip::rotate_columns_sp(parent, level, cts, gkeys);
    std::ofstream out(argv[2], std::ios::binary);
    cts.save(out);
    out.close();
    if (!out) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 1; }
    const std::vector<uint64_t> words = cts.to_host();
    uint64_t digest = 0;
    for (size_t i = 0; i < words.size(); ++i) digest += words[i] * (2 * (uint64_t)i + 1);
    std::printf("keyswitch_sp_check: %zu ciphertexts of %u polynomials steps=%d swap=%d digest=%016llx\n", count, size, steps, (int)swap, (unsigned long long)digest);
    return 0;
}
