// A sparse integer map across position-packed ciphertexts through the SEAL facade: reads a plan (text: n_in n_out T window n_order, then
// n_out * T taps, n_out * T weights, n_order order entries), loads <frames> * n_in size-2 ciphertexts (the records Ciphertext::save
// writes, frame after frame), runs seal::hip::plane_map, saves the <frames> * n_out results in the same order and prints the plan's cut
// and a digest of the output:
//     digest = sum over the output words w_i (i counted through the whole stream) of w_i * (2 i + 1)  mod 2^64
// tests/test_gpu_planemap.py compares file, cut and digest with the Python path (Evaluator.plane_map) on the same input.
//   planemap_check <plan> <in> <out> <frames> <n> <t> <q0> [q1 ...]
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "seal/hip_circuits.h"

int main(int argc, char **argv) {
    if (argc < 8) {
        std::fprintf(stderr, "usage: %s <plan> <in> <out> <frames> <n> <t> <q0> [q1 ...]\n", argv[0]);
        return 2;
    }
    const size_t frames = (size_t)std::strtoull(argv[4], nullptr, 10);
    seal::EncryptionParameters params;
    params.set_poly_modulus("1x^" + std::string(argv[5]) + " + 1");
    std::vector<seal::SmallModulus> q;
    for (int i = 7; i < argc; ++i) q.push_back(seal::SmallModulus(std::strtoull(argv[i], nullptr, 0)));
    params.set_coeff_modulus(q);
    params.set_plain_modulus(std::strtoull(argv[6], nullptr, 0));
    seal::SEALContext context(params);
    unsigned long n_in = 0, n_out = 0, T = 0, window = 0, n_order = 0;
    std::vector<uint32_t> taps, order;
    std::vector<int64_t> weights;
    {
        std::ifstream pf(argv[1]);
        pf >> n_in >> n_out >> T >> window >> n_order;
        if (!pf || n_out > 65536 || T > 64 || n_order > 65536) { std::fprintf(stderr, "cannot read the plan %s\n", argv[1]); return 1; }
        taps.resize(n_out * T);
        weights.resize(n_out * T);
        order.resize(n_order);
        for (size_t i = 0; i < taps.size(); ++i) pf >> taps[i];
        for (size_t i = 0; i < weights.size(); ++i) { long long w; pf >> w; weights[i] = w; }
        for (size_t i = 0; i < order.size(); ++i) pf >> order[i];
        if (!pf) { std::fprintf(stderr, "the plan %s is short\n", argv[1]); return 1; }
    }
    seal::hip::CiphertextBatch in;
    {
        std::ifstream is(argv[2], std::ios::binary);
        if (!is) { std::fprintf(stderr, "cannot open %s\n", argv[2]); return 1; }
        in.load(context, is, frames * n_in, 2);
    }
    seal::hip::PlaneMapPlan plan(context, (uint32_t)n_in, (uint32_t)T, taps, weights, order, (uint32_t)window);
    seal::hip::CiphertextBatch res = seal::hip::plane_map(plan, in);
    std::ofstream out(argv[3], std::ios::binary);
    res.save(out);
    out.close();
    if (!out) { std::fprintf(stderr, "cannot write %s\n", argv[3]); return 1; }
    const std::vector<uint64_t> words = res.to_host();
    uint64_t digest = 0;
    for (size_t i = 0; i < words.size(); ++i) digest += words[i] * (2 * (uint64_t)i + 1);
    std::printf("planemap_check: %zu frames groups=%u source_reads=%llu window=%u digest=%016llx\n", frames, plan.groups(), (unsigned long long)plan.source_reads(),
                plan.window(), (unsigned long long)digest);
    return 0;
}
