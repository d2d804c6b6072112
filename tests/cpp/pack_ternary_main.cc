// pack_ternary_main.cc — packs one matrix of PACKED ternary BitNet weights (uint8 [Mw / 4][K], four weight rows per byte) on the host through
// tmac_amd/csrc/tmac_pack.h: the format's arithmetic (ternary_packed_row, ternary_field, ternary_four) and the blob's index arithmetic the
// pack kernels (tmac_pack.hip: k_pack_ternary_weights, k_pack_ternary_weights_x4) share.  Plain g++, no HIP; tests/test_bitnet_packed_cpu.py
// builds it with -fsanitize=address,undefined.
//   pack_ternary_main form Mw K bm kfactor packed.bin A.bin
// form 0: per weight row, as the general kernel walks the matrix -- weight row o takes field o / R4 of packed row o % R4.
// form 1: four fields per byte, as the read-once kernel walks it -- every packed row feeds the four weight rows i R4 + pr; needs R4 % 16 == 0
//         there, not here: the arithmetic holds for every R4.
// Output: A.bin, the weight half of the reference blob (bits = 2).  stdout: the number of fields of value 3.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../tmac_amd/csrc/tmac_pack.h"

namespace pk = tmac_pack;

static std::vector<uint8_t> slurp(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    std::vector<uint8_t> v;
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}
static void dump(const char* path, const void* p, size_t n) {
    FILE* f = fopen(path, "wb");
    if (!f || fwrite(p, 1, n, f) != n) { fprintf(stderr, "cannot write %s\n", path); exit(2); }
    fclose(f);
}

int main(int argc, char** argv) {
    if (argc != 8) { fprintf(stderr, "usage: see the head of pack_ternary_main.cc\n"); return 2; }
    const int form = atoi(argv[1]), Mw = atoi(argv[2]), K = atoi(argv[3]), bm = atoi(argv[4]), kf = atoi(argv[5]);
    const int bits = 2, T = K / 4, M = Mw * bits, R4 = Mw / 4;
    const std::vector<uint8_t> P = slurp(argv[6]);
    if (Mw % 4 || P.size() != (size_t)R4 * K) { fprintf(stderr, "packed: %zu bytes\n", P.size()); return 2; }

    std::vector<uint8_t> A((size_t)M * T / 2, 0);
    long invalid = 0;
    auto put = [&](int o, int t, uint32_t four) {
        for (int p = 0; p < bits; ++p) {
            const int r = pk::mrow(o, p, bits);
            A[pk::blob_byte(r, t, bm, kf, T)] |= (uint8_t)(pk::codes_nibble(four, p) << (pk::blob_high(r, bm) ? 4 : 0));
        }
    };
    auto bytes_of = [&](int pr, int t) {
        uint32_t b;
        memcpy(&b, P.data() + (size_t)pr * K + 4 * (size_t)t, 4);      // little endian: column i in byte i
        return b;
    };
    if (form == 0) {
        for (int o = 0; o < Mw; ++o)
            for (int t = 0; t < T; ++t) {
                int n;
                put(o, t, pk::ternary_four(bytes_of(pk::ternary_packed_row(o, R4), t), pk::ternary_field(o, R4), &n));
                invalid += n;
            }
    } else {
        for (int pr = 0; pr < R4; ++pr)
            for (int t = 0; t < T; ++t) {
                const uint32_t b = bytes_of(pr, t);
                for (int i = 0; i < 4; ++i) {
                    int n;
                    put(i * R4 + pr, t, pk::ternary_four(b, i, &n));
                    invalid += n;
                }
            }
    }
    dump(argv[7], A.data(), A.size());
    printf("%ld\n", invalid);
    return 0;
}
