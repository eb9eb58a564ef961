// The inverse JPEG steps through the SEAL facade: loads n_blocks x 192 ciphertexts (per block 64 Y, 64 Cb, 64 Cr, the order
// server_jpeg writes), runs seal::hip::idct8x8_dequant over them (dequantised by the JPEG luminance table when quant = 1) and
// seal::hip::ycc_to_rgb_blocks, and saves the 64 R, 64 G, 64 B per block.  tests/test_gpu_idct.py compares its output with the
// Python Evaluator's on the same input.
//   idct_check <in> <out> <n_blocks> <quant 0|1> <n> <t> <q0> [q1 ...]
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "seal/seal.h"

int main(int argc, char **argv) {
    if (argc < 8) {
        std::fprintf(stderr, "usage: %s <in> <out> <n_blocks> <quant 0|1> <n> <t> <q0> [q1 ...]\n", argv[0]);
        return 2;
    }
    const size_t n_blocks = std::strtoull(argv[3], nullptr, 10);
    const bool quant = std::atoi(argv[4]) != 0;
    seal::EncryptionParameters params;
    params.set_poly_modulus("1x^" + std::string(argv[5]) + " + 1");
    std::vector<seal::SmallModulus> q;
    for (int i = 7; i < argc; ++i) q.push_back(seal::SmallModulus(std::strtoull(argv[i], nullptr, 0)));
    params.set_coeff_modulus(q);
    params.set_plain_modulus(std::strtoull(argv[6], nullptr, 0));
    seal::SEALContext context(params);
    static const std::vector<double> yqt = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                                            14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                                            49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
    std::vector<seal::Ciphertext> cts(n_blocks * 192);
    {
        std::ifstream in(argv[1], std::ios::binary);
        if (!in) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 1; }
        for (seal::Ciphertext &c : cts) c.load(in);
    }
    seal::hip::idct8x8_dequant(context, cts, quant ? &yqt : nullptr);
    seal::hip::ycc_to_rgb_blocks(context, cts);
    std::ofstream out(argv[2], std::ios::binary);
    for (const seal::Ciphertext &c : cts) c.save(out);
    out.close();
    if (!out) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 1; }
    std::printf("idct_check: %zu blocks\n", n_blocks);
    return 0;
}
