// A 2-D convolution through the SEAL facade: loads width * height * 3 ciphertexts (R, G, B per pixel, row by row: the stream
// client.send_resize writes), filters all three channels with a named kernel through seal::hip::filter2d (taps from
// fhe_filter_tap_plan, clamp-to-edge borders), saves the dst_w * dst_h * 3 results in the same order and prints a digest of them:
//     digest = sum over the output words w_i (i counted through the whole stream) of w_i * (2 i + 1)  mod 2^64
// tests/test_gpu_filter.py compares file and digest with the Python path (server.server_filter / Evaluator.filter2d) on the same input.
//   filter_check <in> <out> <width> <height> <box3|gauss3|gauss5|sobel_x|sharpen|chroma420> <n> <t> <q0> [q1 ...]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "seal/seal.h"

int main(int argc, char **argv) {
    if (argc < 9) {
        std::fprintf(stderr, "usage: %s <in> <out> <width> <height> <kernel> <n> <t> <q0> [q1 ...]\n", argv[0]);
        return 2;
    }
    const uint32_t width = (uint32_t)std::strtoul(argv[3], nullptr, 10), height = (uint32_t)std::strtoul(argv[4], nullptr, 10);
    const std::string name = argv[5];
    std::vector<double> w;
    uint32_t kw = 3, kh = 3, stride = 1;
    int anchor = 1;
    if (name == "box3") w.assign(9, 1.0 / 9.0);
    else if (name == "gauss3") { for (int j = 0; j < 3; ++j) for (int i = 0; i < 3; ++i) w.push_back((j == 1 ? 2 : 1) * (i == 1 ? 2 : 1) / 16.0); }
    else if (name == "gauss5") {
        static const int b[5] = {1, 4, 6, 4, 1};
        kw = kh = 5; anchor = 2;
        for (int j = 0; j < 5; ++j) for (int i = 0; i < 5; ++i) w.push_back(b[j] * b[i] / 256.0);
    }
    else if (name == "sobel_x") w = {-1, 0, 1, -2, 0, 2, -1, 0, 1};
    else if (name == "sharpen") w = {0, -1, 0, -1, 5, -1, 0, -1, 0};
    else if (name == "chroma420") { kw = kh = 2; anchor = 0; stride = 2; w.assign(4, 0.25); }
    else { std::fprintf(stderr, "unknown kernel %s\n", name.c_str()); return 2; }
    seal::EncryptionParameters params;
    params.set_poly_modulus("1x^" + std::string(argv[6]) + " + 1");
    std::vector<seal::SmallModulus> q;
    for (int i = 8; i < argc; ++i) q.push_back(seal::SmallModulus(std::strtoull(argv[i], nullptr, 0)));
    params.set_coeff_modulus(q);
    params.set_plain_modulus(std::strtoull(argv[7], nullptr, 0));
    seal::SEALContext context(params);
    std::vector<seal::Ciphertext> cts((size_t)width * height * 3);
    {
        std::ifstream in(argv[1], std::ios::binary);
        if (!in) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 1; }
        for (seal::Ciphertext &c : cts) c.load(in);
    }
    uint32_t dw = 0, dh = 0;
    if (fhe_filter_tap_plan(width, height, 3, kw, kh, anchor, anchor, stride, stride, 0, 0, 0, &dw, &dh, nullptr)) {
        std::fprintf(stderr, "tap plan: %s\n", fhe_last_error());
        return 1;
    }
    std::vector<uint32_t> taps((size_t)dw * dh * 3 * kw * kh);
    if (fhe_filter_tap_plan(width, height, 3, kw, kh, anchor, anchor, stride, stride, 0, dh, 0, &dw, &dh, taps.data())) {
        std::fprintf(stderr, "tap plan: %s\n", fhe_last_error());
        return 1;
    }
    const std::vector<seal::Ciphertext> res = seal::hip::filter2d(context, cts, w, kw, kh, taps);
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
    std::printf("filter_check: %s %ux%u -> %ux%u digest=%016llx\n", name.c_str(), width, height, dw, dh, (unsigned long long)digest);
    return 0;
}
