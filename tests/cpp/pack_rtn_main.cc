// pack_rtn_main.cc — quantises (per-group round to nearest) and packs one dense matrix on the host through tmac_amd/csrc/tmac_pack.h: the
// rule (rtn_scale_zq, rtn_four, rtn_zero), the index of a (row, group) parameter and the index arithmetic the pack kernels (tmac_pack.hip:
// k_rtn_params, k_pack_rtn_weights, k_pack_codes_scales) share.  Plain g++, no HIP; tests/test_pack_rtn_cpu.py builds it with
// -fsanitize=address,undefined.
//   pack_rtn_main src Mw K bits gs zero_point scale_f16 bm kfactor W.bin A.bin S.bin P.bin
// src: 0 fp32, 1 fp16, 2 bf16 (tmac_src_dtype_t); W.bin: the masters' bytes, [Mw][K] row-major.  Outputs: A.bin, the weight half of the
// reference blob; S.bin, its fp32 scales half (scales and, with zero points, zeros, interleaved by octets); P.bin, fp32 [3][Mw][K / gs] --
// scales, zq, and 1.0 where the group is invalid.
// The minimum and maximum are taken in the device's order -- a lane's loads in turn, then the xor butterfly over the group's lanes -- though
// being exact, no order could show.
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

int main(int argc, char** argv) {
    if (argc != 14) { fprintf(stderr, "usage: see the head of pack_rtn_main.cc\n"); return 2; }
    const int src = atoi(argv[1]), Mw = atoi(argv[2]), K = atoi(argv[3]), bits = atoi(argv[4]), gs = atoi(argv[5]), zp = atoi(argv[6]),
              f16 = atoi(argv[7]), bm = atoi(argv[8]), kf = atoi(argv[9]);
    const int T = K / 4, M = Mw * bits, SG = K / gs;
    const Masters W{slurp(argv[10]), src};
    if (W.raw.size() != (size_t)Mw * K * (src == pk::SRC_F32 ? 4 : 2)) { fprintf(stderr, "W: %zu bytes\n", W.raw.size()); return 2; }

    const size_t items = (size_t)Mw * SG;
    std::vector<float> P(3 * items), zeros(items);
    float *scales = P.data(), *zq = scales + items, *bad = zq + items;
    const int epl = src != pk::SRC_F32 && gs % 8 == 0 ? 8 : 4, vecs = gs / epl;
    int seg = 1;
    while (seg < vecs && seg < 64) seg <<= 1;
    for (int o = 0; o < Mw; ++o)
        for (int sg = 0; sg < SG; ++sg) {
            const size_t item = pk::rtn_param_index(o, sg, SG);
            float lo[64], hi[64];
            bool fin[64];
            for (int sub = 0; sub < seg; ++sub) {
                lo[sub] = hi[sub] = 0.0f;
                fin[sub] = true;
                for (int v = sub; v < vecs; v += seg)
                    for (int j = 0; j < epl; ++j) {
                        const float w = W.get(item * gs + (size_t)v * epl + j);
                        lo[sub] = fminf(lo[sub], w);
                        hi[sub] = fmaxf(hi[sub], w);
                        fin[sub] = fin[sub] && pk::rtn_finite(w);
                    }
            }
            for (int off = seg / 2; off >= 1; off >>= 1)
                for (int l = 0; l < off; ++l) {      // lane 0 ends with what the butterfly leaves in every lane
                    lo[l] = fminf(lo[l], lo[l + off]);
                    hi[l] = fmaxf(hi[l], hi[l + off]);
                    fin[l] = fin[l] && fin[l + off];
                }
            bad[item] = pk::rtn_scale_zq(lo[0], hi[0], fin[0], bits, zp, f16, &scales[item], &zq[item]) ? 0.0f : 1.0f;
            zeros[item] = pk::rtn_zero(scales[item], zq[item], bits);
        }

    std::vector<uint8_t> A((size_t)M * T / 2, 0);
    for (int o = 0; o < Mw; ++o)
        for (int t = 0; t < T; ++t) {
            const size_t e = (size_t)o * K + 4 * (size_t)t, pi = pk::rtn_param_index(o, 4 * t / gs, SG);
            const uint32_t four = pk::rtn_four(W.get(e), W.get(e + 1), W.get(e + 2), W.get(e + 3), scales[pi], zq[pi], bits);
            for (int p = 0; p < bits; ++p) {
                const int r = pk::mrow(o, p, bits);
                A[pk::blob_byte(r, t, bm, kf, T)] |= (uint8_t)(pk::codes_nibble(four, p) << (pk::blob_high(r, bm) ? 4 : 0));
            }
        }
    std::vector<float> S(items * (zp ? 2 : 1));
    for (int o = 0; o < Mw; ++o)
        for (int sg = 0; sg < SG; ++sg) {
            const size_t item = pk::rtn_param_index(o, sg, SG);
            S[pk::scale_index(o, sg, 0, bm, bits, SG, zp)] = scales[item];
            if (zp) S[pk::scale_index(o, sg, 1, bm, bits, SG, zp)] = zeros[item];
        }
    dump(argv[11], A.data(), A.size());
    dump(argv[12], S.data(), 4 * S.size());
    dump(argv[13], P.data(), 4 * P.size());
    return 0;
}
