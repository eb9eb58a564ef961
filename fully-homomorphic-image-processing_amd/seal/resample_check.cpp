// A separable resize with public weights through the SEAL facade: loads width * height * 3 ciphertexts (R, G, B per pixel, row by row: the
// stream client.send_resize writes), resizes all three channels through seal::hip::resize_plain (axis plans from fhe_resample_axis_plan,
// clamp-to-edge borders), saves the dst_w * dst_h * 3 results in the same order and prints a digest of them:
//     digest = sum over the output words w_i (i counted through the whole stream) of w_i * (2 i + 1)  mod 2^64
// tests/test_gpu_resample.py compares file and digest with the Python path (server.server_resize_plain) on the same input.
//   resample_check <in> <out> <width> <height> <dst_w> <dst_h> <triangle|catmull_rom|reference_cubic|lanczos3|box> <half_pixel|reference>
//                  <antialias 0|1> <weight_bits> <n> <t> <q0> [q1 ...]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "seal/seal.h"

int main(int argc, char **argv) {
    if (argc < 14) {
        std::fprintf(stderr, "usage: %s <in> <out> <width> <height> <dst_w> <dst_h> <kernel> <convention> <antialias> <weight_bits> <n> <t> <q0> [q1 ...]\n", argv[0]);
        return 2;
    }
    const uint32_t width = (uint32_t)std::strtoul(argv[3], nullptr, 10), height = (uint32_t)std::strtoul(argv[4], nullptr, 10);
    const uint32_t dw = (uint32_t)std::strtoul(argv[5], nullptr, 10), dh = (uint32_t)std::strtoul(argv[6], nullptr, 10);
    static const char *const kernels[] = {"triangle", "catmull_rom", "reference_cubic", "lanczos3", "box"};
    int kernel = -1;
    for (int i = 0; i < 5; ++i)
        if (!std::strcmp(argv[7], kernels[i])) kernel = i;
    const int convention = !std::strcmp(argv[8], "reference") ? FHE_RESAMPLE_REFERENCE : !std::strcmp(argv[8], "half_pixel") ? FHE_RESAMPLE_HALF_PIXEL : -1;
    if (kernel < 0 || convention < 0) { std::fprintf(stderr, "unknown kernel %s or convention %s\n", argv[7], argv[8]); return 2; }
    const bool antialias = std::atoi(argv[9]) != 0;
    const int weight_bits = std::atoi(argv[10]);
    seal::EncryptionParameters params;
    params.set_poly_modulus("1x^" + std::string(argv[11]) + " + 1");
    std::vector<seal::SmallModulus> q;
    for (int i = 13; i < argc; ++i) q.push_back(seal::SmallModulus(std::strtoull(argv[i], nullptr, 0)));
    params.set_coeff_modulus(q);
    params.set_plain_modulus(std::strtoull(argv[12], nullptr, 0));
    seal::SEALContext context(params);
    std::vector<seal::Ciphertext> cts((size_t)width * height * 3);
    {
        std::ifstream in(argv[1], std::ios::binary);
        if (!in) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 1; }
        for (seal::Ciphertext &c : cts) c.load(in);
    }
    const std::vector<seal::Ciphertext> res = seal::hip::resize_plain(context, cts, width, height, dw, dh, kernel, 3, antialias, convention, weight_bits);
    std::ofstream out(argv[2], std::ios::binary);
    uint64_t digest = 0, index = 0;
    for (const seal::Ciphertext &c : res) {
        c.save(out);
        const uint64_t *p = c.pointer();
        const size_t words = (size_t)c.size() * c.coeff_mod_count() * (c.poly_coeff_count() - 1);
        for (size_t i = 0; i < words; ++i, ++index) digest += p[i] * (2 * index + 1);
    }
    out.close();
    if (!out) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 1; }
    std::printf("resample_check: %s %ux%u -> %ux%u digest=%016llx\n", argv[7], width, height, dw, dh, (unsigned long long)digest);
    return 0;
}
