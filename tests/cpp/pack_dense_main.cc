// pack_dense_main.cc — quantises and packs one matrix of BitNet master weights on the host through tmac_amd/csrc/tmac_pack.h: the absmean
// rule (absmean_scale, absmean_inv, absmean_four) and the index arithmetic the pack kernels (tmac_pack.hip: k_absmean, k_pack_dense_weights)
// share.  Plain g++, no HIP; tests/test_pack_dense_cpu.py builds it with -fsanitize=address,undefined.
//   pack_dense_main src Mw K bm kfactor m_groups eps scales_given W.bin scales_in.bin A.bin S.bin
// src: 0 fp32, 1 fp16, 2 bf16 (tmac_src_dtype_t); W.bin: the masters' bytes, [Mw][K] row-major; scales_in.bin: fp32 [m_groups], read when
// scales_given is 1.  Outputs: A.bin, the weight half of the reference blob (bits = 2), and S.bin, the fp32 [m_groups] scales.
// The block sum is taken in the device's order: chunks of ABSMEAN_CHUNK elements, each chunk lane by lane as k_absmean deals it, the lanes
// of a wave through the xor butterfly, the waves and then the chunks in index order.
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

struct Masters {
    std::vector<uint8_t> raw;
    int src;
    float get(size_t i) const {
        if (src == pk::SRC_F32) { float v; memcpy(&v, raw.data() + 4 * i, 4); return v; }
        uint16_t h;
        memcpy(&h, raw.data() + 2 * i, 2);
        return src == pk::SRC_F16 ? pk::f16_bits_to_f32(h) : pk::bf16_bits_to_f32(h);
    }
};

// sum of |w| over elements [base, base + n) as k_absmean and k_absmean_scales take it
static double block_sum(const Masters& W, size_t base, size_t n) {
    double total = 0.0;
    for (size_t c = 0; c < pk::absmean_chunks(n); ++c) {
        double lane[pk::ABSMEAN_THREADS];
        for (int t = 0; t < pk::ABSMEAN_THREADS; ++t) {
            lane[t] = 0.0;
            for (int i = 0; i < pk::ABSMEAN_STEPS; ++i) {
                const size_t e = c * pk::ABSMEAN_CHUNK + ((size_t)i * pk::ABSMEAN_THREADS + t) * pk::ABSMEAN_VEC;
                if (e < n)
                    for (int j = 0; j < pk::ABSMEAN_VEC; ++j) lane[t] += (double)fabsf(W.get(base + e + j));
            }
        }
        double chunk = 0.0;
        for (int wv = 0; wv < pk::ABSMEAN_THREADS / 64; ++wv) {
            double v[64], u[64];
            memcpy(v, lane + 64 * wv, sizeof v);
            for (int off = 32; off >= 1; off >>= 1) {
                for (int l = 0; l < 64; ++l) u[l] = v[l] + v[l ^ off];
                memcpy(v, u, sizeof v);
            }
            chunk = wv == 0 ? v[0] : chunk + v[0];
        }
        total += chunk;
    }
    return total;
}

int main(int argc, char** argv) {
    if (argc != 13) { fprintf(stderr, "usage: see the head of pack_dense_main.cc\n"); return 2; }
    const int src = atoi(argv[1]), Mw = atoi(argv[2]), K = atoi(argv[3]), bm = atoi(argv[4]), kf = atoi(argv[5]), mg = atoi(argv[6]);
    const float eps = (float)atof(argv[7]);
    const int given = atoi(argv[8]);
    const int bits = 2, T = K / 4, M = Mw * bits, R = Mw / mg;
    const Masters W{slurp(argv[9]), src};
    if (W.raw.size() != (size_t)Mw * K * (src == pk::SRC_F32 ? 4 : 2)) { fprintf(stderr, "W: %zu bytes\n", W.raw.size()); return 2; }

    std::vector<float> s((size_t)mg);
    if (given) {
        const std::vector<uint8_t> in = slurp(argv[10]);
        if (in.size() != 4 * (size_t)mg) { fprintf(stderr, "scales_in: %zu bytes\n", in.size()); return 2; }
        memcpy(s.data(), in.data(), in.size());
    } else {
        for (int g = 0; g < mg; ++g) s[g] = pk::absmean_scale(block_sum(W, (size_t)g * R * K, (size_t)R * K), (double)((size_t)R * K), eps);
    }

    std::vector<uint8_t> A((size_t)M * T / 2, 0);
    for (int o = 0; o < Mw; ++o) {
        const float inv = pk::absmean_inv(s[o / R]);
        for (int t = 0; t < T; ++t) {
            const size_t e = (size_t)o * K + 4 * (size_t)t;
            const uint32_t four = pk::absmean_four(W.get(e), W.get(e + 1), W.get(e + 2), W.get(e + 3), inv);
            for (int p = 0; p < bits; ++p) {
                const int r = pk::mrow(o, p, bits);
                A[pk::blob_byte(r, t, bm, kf, T)] |= (uint8_t)(pk::codes_nibble(four, p) << (pk::blob_high(r, bm) ? 4 : 0));
            }
        }
    }
    dump(argv[11], A.data(), A.size());
    dump(argv[12], s.data(), 4 * s.size());
    return 0;
}
