// asan_main.hip -- TEST INFRASTRUCTURE ONLY: the network core's host build (net_host.hip) under
// AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program. It drives every function of
// the core on exactly-sized heap buffers -- bf16 rounding of edge values, the folding, the pack and
// unpack of F = 32, 96, 256 (a round trip, and every index hit once), the tap map at the board's edges
// and past the batch's end, and the stem on boards that hold every int8 value -- and checks the
// invariants it can state itself. Any sanitizer report or failed check exits non-zero.
#include "net_host.hip"

#include <stdio.h>
#include <stdlib.h>

#define CHECK(c)                                                 \
    do {                                                         \
        if (!(c)) {                                              \
            printf("net_host asan: check failed: %s\n", #c);     \
            return 1;                                            \
        }                                                        \
    } while (0)

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }
static float unit(uint32_t& s) { return (float)(lcg(s) >> 8) / (float)(1 << 24); }

int main() {
    uint32_t seed = 12345u;
    // bf16: exact values stay, ties go to even, NaN stays NaN, one rounding from float64
    CHECK(net_bf16_round(1.0f) == 0x3f80 && net_bf16_widen(0x3f80) == 1.0f);
    CHECK(net_bf16_round(net_bits_f32(0x3f808000u)) == 0x3f80 && net_bf16_round(net_bits_f32(0x3f818000u)) == 0x3f82);
    CHECK((net_bf16_round(net_bits_f32(0x7fc00001u)) & 0x7fc0) == 0x7fc0);
    CHECK(net_bf16_round(net_bits_f32(0x7f800000u)) == 0x7f80 && net_bf16_round(net_bits_f32(0x7f7fffffu)) == 0x7f80);
    const double above_tie = (double)net_bits_f32(0x3f808000u) + 1e-12, below_tie = (double)net_bits_f32(0x3f808000u) - 1e-12;
    CHECK(net_bf16_round_f64(above_tie) == 0x3f81 && net_bf16_round_f64(below_tie) == 0x3f80);
    for (int i = 0; i < 100000; ++i) {
        const float x = net_bits_f32(lcg(seed));
        const uint16_t h = net_bf16_round(x);
        if (x == x) CHECK(net_bf16_round(net_bf16_widen(h)) == h);
    }
    int packs = 0;
    for (int F : {32, 96, 256}) {
        CHECK(net_features_ok(F));
        const int64_t K = 9 * (int64_t)F, E = net_pack_elems(F);
        std::vector<float> w(K * F), b(F), scale(F), bias(F), mean(F), var(F), wf(K * F), bo(F);
        std::vector<uint16_t> wh(K * F), packed(E), back(K * F);
        std::vector<uint8_t> hit(E, 0);
        for (auto& x : w) x = unit(seed) - 0.5f;
        for (int o = 0; o < F; ++o) {
            b[o] = unit(seed) - 0.5f;
            scale[o] = 0.5f + unit(seed);
            bias[o] = unit(seed) - 0.5f;
            mean[o] = unit(seed) - 0.5f;
            var[o] = 0.5f + unit(seed);
        }
        nt_fold(w.data(), b.data(), scale.data(), bias.data(), mean.data(), var.data(), 1e-5, K, F, wf.data(), wh.data(),
                bo.data());
        for (int64_t k = 0; k < K; ++k)
            for (int n = 0; n < F; ++n) {
                const int64_t idx = net_pack_index(F, k, n);
                CHECK(idx >= 0 && idx < E && !hit[idx]);
                hit[idx] = 1;
                int64_t k2;
                int n2;
                net_unpack_index(F, idx, &k2, &n2);
                CHECK(k2 == k && n2 == n);
            }
        nt_pack(F, wh.data(), packed.data());
        nt_unpack(F, packed.data(), back.data());
        CHECK(back == wh);
        ++packs;
    }
    CHECK(!net_features_ok(0) && !net_features_ok(48) && !net_features_ok(544));
    // the tap map: 7 x 5 boards, 3 of them, and rows past the end
    {
        const int R = 7, C = 5, P = R * C;
        const int64_t M = 3 * P;
        for (int64_t m = 0; m < M + 70; ++m)
            for (int tap = 0; tap < 9; ++tap) {
                const int64_t src = net_tap_row(m, M, R, C, tap);
                CHECK(src >= -1 && src < M);
                if (m >= M) CHECK(src == -1);
                if (src >= 0) CHECK(src / P == m / P);  // never another board's cell
                if (tap == 4 && m < M) CHECK(src == m);
            }
        CHECK(net_tap_row(0, M, R, C, 0) == -1 && net_tap_row(P - 1, M, R, C, 8) == -1);
    }
    for (int lane = 0; lane < 64; ++lane)
        for (int reg = 0; reg < 16; ++reg) CHECK(net_acc_row(lane, reg) >= 0 && net_acc_row(lane, reg) < 32);
    // the stem on boards that hold every int8 value: no read outside w [9][CH][F]
    int stems = 0;
    for (int CH : {8, 32, 128}) {
        const int R = 4, C = 3, F = 32, P = R * C;
        const int64_t n = 24;
        std::vector<int8_t> boards(n * P);
        for (size_t i = 0; i < boards.size(); ++i) boards[i] = (int8_t)(i - 128);
        std::vector<float> w((size_t)9 * CH * F), b(F);
        for (auto& x : w) x = unit(seed) - 0.5f;
        for (auto& x : b) x = unit(seed) - 0.5f;
        std::vector<uint16_t> out(n * P * F);
        nt_stem(boards.data(), n, R, C, CH, F, w.data(), b.data(), out.data());
        for (uint16_t h : out) CHECK(!(h & 0x8000) || h == 0x8000);  // after the ReLU
        ++stems;
    }
    CHECK(net_blob_len(81, 144, 32, 0, 32) == 9 * 32 * 32 + 5 * 32 + (32 + 5 + 81 * 32 + 32 + 32 + 1) + (64 + 10 + 162 * 144 + 144));
    printf("net_host asan: %d packs, %d stems: checks ok\n", packs, stems);
    return 0;
}
