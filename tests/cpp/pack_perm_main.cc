// pack_perm_main.cc — packs the weights of one act-order matrix on the host through tmac_amd/csrc/tmac_pack.h, with the arithmetic the
// permuted pack kernels (k_pack_gptq_weights_perm, k_pack_codes_weights_perm in tmac_pack.hip) use: table t takes its four codes from the
// source columns perm[4 t .. 4 t + 3].  Plain g++, no HIP.  (Scales and zeros do not pass through the permutation: tests/cpp/pack_main.cc.)
//   pack_perm_main gptq|codes Mw K bits bm kfactor weights.bin perm.bin A.bin
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../tmac_amd/csrc/tmac_pack.h"

namespace pk = tmac_pack;

static std::vector<uint8_t> slurp(const char* path, size_t bytes) {
    FILE* f = fopen(path, "rb");
    std::vector<uint8_t> v(bytes);
    if (!f || fread(v.data(), 1, bytes, f) != bytes || fgetc(f) != EOF) { fprintf(stderr, "%s: not %zu bytes\n", path, bytes); exit(2); }
    fclose(f);
    return v;
}

int main(int argc, char** argv) {
    if (argc != 10) { fprintf(stderr, "usage: see the head of pack_perm_main.cc\n"); return 2; }
    const bool gptq = std::string(argv[1]) == "gptq";
    const int Mw = atoi(argv[2]), K = atoi(argv[3]), bits = atoi(argv[4]), bm = atoi(argv[5]), kf = atoi(argv[6]);
    const int T = K / 4, M = Mw * bits;
    const std::vector<uint8_t> src = slurp(argv[7], gptq ? (size_t)(K / (32 / bits)) * Mw * 4 : (size_t)Mw * K);
    const std::vector<uint8_t> praw = slurp(argv[8], (size_t)K * 4);
    std::vector<int32_t> perm((size_t)K);
    memcpy(perm.data(), praw.data(), praw.size());

    std::vector<uint8_t> A((size_t)M * T / 2, 0);
    for (int o = 0; o < Mw; ++o)
        for (int t = 0; t < T; ++t) {
            uint32_t c[4];
            for (int ig = 0; ig < 4; ++ig) {
                const int k = perm[(size_t)4 * t + ig];
                if (gptq) {
                    uint32_t word;
                    memcpy(&word, src.data() + 4 * ((size_t)pk::gptq_word_row(k, bits) * Mw + o), 4);
                    c[ig] = pk::gptq_code(word, k, bits);
                } else {
                    c[ig] = src[(size_t)o * K + k];
                }
            }
            const uint32_t four = pk::codes_four(c[0], c[1], c[2], c[3]);
            for (int p = 0; p < bits; ++p) {
                const int r = pk::mrow(o, p, bits);
                A[pk::blob_byte(r, t, bm, kf, T)] |= (uint8_t)(pk::codes_nibble(four, p) << (pk::blob_high(r, bm) ? 4 : 0));
            }
        }
    FILE* f = fopen(argv[9], "wb");
    if (!f || fwrite(A.data(), 1, A.size(), f) != A.size()) { fprintf(stderr, "cannot write %s\n", argv[9]); return 2; }
    fclose(f);
    return 0;
}
