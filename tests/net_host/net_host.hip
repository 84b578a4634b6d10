// net_host.hip -- TEST INFRASTRUCTURE ONLY: the host build of the policy/value network's launch-free core
// (csrc/m3_net_core.hpp) behind a C face, for tests/test_net_cpu.py (ctypes, net_host.py) and for the
// sanitized stand-alone program asan_main.hip.
#include <stdint.h>

#include <vector>

#include "../../element-crush-gym_amd/csrc/m3_net_core.hpp"

using namespace m3n;

extern "C" {

int nt_features_ok(int F) { return net_features_ok(F); }

void nt_bf16_round(const float* x, int64_t n, uint16_t* out) {
    for (int64_t i = 0; i < n; ++i) out[i] = net_bf16_round(x[i]);
}

void nt_bf16_round_f64(const double* x, int64_t n, uint16_t* out) {
    for (int64_t i = 0; i < n; ++i) out[i] = net_bf16_round_f64(x[i]);
}

void nt_bf16_widen(const uint16_t* h, int64_t n, float* out) {
    for (int64_t i = 0; i < n; ++i) out[i] = net_bf16_widen(h[i]);
}

// a convolution [rows][out] with its BN folded: w' as float32 and as bf16, b' as float32
void nt_fold(const float* w, const float* b, const float* scale, const float* bias, const float* mean, const float* var,
             double eps, int64_t rows, int out, float* w_f32, uint16_t* w_bf16, float* b_out) {
    net_fold_conv_f32(w, b, scale, bias, mean, var, eps, rows, out, w_f32, b_out);
    net_fold_conv_bf16(w, b, scale, bias, mean, var, eps, rows, out, w_bf16, b_out);
}

int64_t nt_pack_elems(int F) { return net_pack_elems(F); }
int64_t nt_pack_index(int F, int64_t k, int n) { return net_pack_index(F, k, n); }
void nt_pack(int F, const uint16_t* w, uint16_t* packed) { net_pack(F, w, packed); }
void nt_unpack(int F, const uint16_t* packed, uint16_t* w) { net_unpack(F, packed, w); }

int64_t nt_tap_row(int64_t m, int64_t M, int R, int C, int tap) { return net_tap_row(m, M, R, C, tap); }
int nt_acc_row(int lane, int reg) { return net_acc_row(lane, reg); }
int64_t nt_blob_len(int P, int A, int CH, int L, int F) { return net_blob_len(P, A, CH, L, F); }

// the stem of n boards: out [n][P][F] bf16
void nt_stem(const int8_t* boards, int64_t n, int R, int C, int CH, int F, const float* w, const float* b, uint16_t* out) {
    const int P = R * C;
    for (int64_t g = 0; g < n; ++g)
        for (int p = 0; p < P; ++p)
            for (int o = 0; o < F; ++o) out[(g * P + p) * F + o] = net_stem_at(boards + g * P, R, C, CH, F, p, o, w, b);
}

}  // extern "C"
