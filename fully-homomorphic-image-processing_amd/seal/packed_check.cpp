// The packed JPEG transform through the SEAL facade: loads 3 * <groups> * 64 size-2 ciphertexts (the records Ciphertext::save writes), the
// position-packed R, G and B planes one after the other ([3][groups][64]: ciphertext 8 r + c of a group holds pixel (r, c) of its blocks),
// runs the colour mix with the level shift (seal::hip::channel_mix: the JFIF matrix in 8 fractional bits, bias -128 * 2^8 on Y) and the forward
// block plan (seal::hip::block8x8_scalar: L = R = dct8_matrix(<dct_bits>), post = round(2^<quant_bits> / Q) for the luminance table of
// homo/fhe_image.h:99), saves the results in the same order and prints a digest of them:
//     digest = sum over the output words w_i (i counted through the whole stream) of w_i * (2 i + 1)  mod 2^64
// tests/test_gpu_packed.py compares file and digest with the Python path (circuits.packed_jpeg_compress) on the same input.
//   packed_check <in> <out> <groups> <dct_bits> <quant_bits> <n> <t> <q0> [q1 ...]
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "seal/hip_circuits.h"

static const int64_t YQT[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                                18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};

int main(int argc, char **argv) {
    if (argc < 9) {
        std::fprintf(stderr, "usage: %s <in> <out> <groups> <dct_bits> <quant_bits> <n> <t> <q0> [q1 ...]\n", argv[0]);
        return 2;
    }
    const size_t groups = (size_t)std::strtoull(argv[3], nullptr, 10);
    const int dct_bits = std::atoi(argv[4]), quant_bits = std::atoi(argv[5]);
    seal::EncryptionParameters params;
    params.set_poly_modulus("1x^" + std::string(argv[6]) + " + 1");
    std::vector<seal::SmallModulus> q;
    for (int i = 8; i < argc; ++i) q.push_back(seal::SmallModulus(std::strtoull(argv[i], nullptr, 0)));
    params.set_coeff_modulus(q);
    params.set_plain_modulus(std::strtoull(argv[7], nullptr, 0));
    seal::SEALContext context(params);
    seal::hip::CiphertextBatch planes;
    {
        std::ifstream in(argv[1], std::ios::binary);
        if (!in) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 1; }
        planes.load(context, in, 3 * groups * 64, 2);
    }
    const std::vector<int64_t> M = {77, 150, 29, -43, -85, 128, 128, -107, -21}, bias = {-(128 << 8), 0, 0};
    seal::hip::CiphertextBatch ycc = seal::hip::channel_mix(context, M, 3, 3, planes, bias);
    const std::vector<int64_t> D = seal::hip::dct8_matrix(dct_bits);
    std::vector<int64_t> post(64);
    for (int i = 0; i < 64; ++i) post[i] = (((int64_t)1 << (quant_bits + 1)) + YQT[i]) / (2 * YQT[i]);
    seal::hip::Block8x8Plan plan(context, D, D, std::vector<int64_t>(), post);
    seal::hip::block8x8_scalar(plan, ycc);
    std::ofstream out(argv[2], std::ios::binary);
    ycc.save(out);
    out.close();
    if (!out) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 1; }
    const std::vector<uint64_t> words = ycc.to_host();
    uint64_t digest = 0;
    for (size_t i = 0; i < words.size(); ++i) digest += words[i] * (2 * (uint64_t)i + 1);
    std::printf("packed_check: %zu groups dct_bits=%d quant_bits=%d digest=%016llx\n", groups, dct_bits, quant_bits, (unsigned long long)digest);
    return 0;
}
