// m3_net_core.hpp -- the launch-free parts of the policy/value ResNet (m3_net.hip holds the kernels,
// DESIGN.md §4.4 the arithmetic model): bf16 rounding, the BatchNorm folding, the pre-pack of a tower
// convolution's weights into the MFMA's B-operand fragment order, the index maps of the implicit GEMM
// and the order of the weight blob. Host-includable like the other *_core.hpp files: the test-only host
// build (tests/net_host) compiles exactly this text.
//
// The network (the reference's ElementCrush in inference form), for a board of R x C cells, P = R * C:
//   one_hot(cell, CH)                      a cell < 0 or >= CH is the zero vector
//   stem   3x3 SAME conv CH -> F, BN, ReLU
//   tower  L x (conv, BN, ReLU, conv, BN, + residual, ReLU), every conv 3x3 SAME F -> F
//   value  1x1 conv F -> 1, BN, ReLU, flatten, dense [P -> F], ReLU, dense [F -> 1], ReLU
//   policy 1x1 conv F -> 2, BN, ReLU, flatten (NHWC: p * 2 + ch), dense [2P -> A]
// Every BN is folded in float64 into the convolution before it (net_fold). The tower's folded
// weights are rounded once to bf16, its activations are stored as bf16, everything else is float32.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#ifndef M3_HD
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define M3_HD __host__ __device__ __forceinline__
#else
#define M3_HD inline
#endif
#endif

namespace m3n {

constexpr int NET_MIN_F = 32, NET_MAX_F = 512;
constexpr int NET_TILE = 32;    // rows and columns of one MFMA tile (v_mfma_f32_32x32x16_bf16)
constexpr int NET_KSTEP = 16;   // its K
constexpr int NET_FRAG = 8;     // bf16 elements of an operand fragment per lane

M3_HD bool net_features_ok(int F) { return F >= NET_MIN_F && F <= NET_MAX_F && F % 32 == 0; }

// ---- bf16 ------------------------------------------------------------------------------------------
M3_HD uint32_t net_f32_bits(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    return u;
}

M3_HD float net_bits_f32(uint32_t u) {
    float x;
    memcpy(&x, &u, 4);
    return x;
}

// float32 -> bf16, round to nearest even; a NaN stays a (quiet) NaN
M3_HD uint16_t net_bf16_round(float x) {
    const uint32_t u = net_f32_bits(x);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x0040u);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

M3_HD float net_bf16_widen(uint16_t h) { return net_bits_f32((uint32_t)h << 16); }

// float64 -> bf16 in ONE rounding to nearest even. Through float32 the value would be rounded twice;
// that differs from one rounding only where the float32 lands exactly on a bf16 tie that the double
// was not on, and there the side the double lay on decides.
M3_HD uint16_t net_bf16_round_f64(double x) {
    const float f = (float)x;
    const uint32_t u = net_f32_bits(f);
    if ((u & 0xffffu) == 0x8000u && (u & 0x7f800000u) != 0x7f800000u && (double)f != x)
        return (uint16_t)((u >> 16) + (fabs(x) > fabs((double)f) ? 1u : 0u));
    return net_bf16_round(f);
}

// ---- BatchNorm folding (float64) ---------------------------------------------------------------------
// y = (conv(x) + b - mean) * scale / sqrt(var + eps) + bias  ==  conv'(x) + b' with
//   k = scale / sqrt(var + eps),  w' = w * k,  b' = (b - mean) * k + bias
M3_HD double net_fold_k(float scale, float var, double eps) { return (double)scale / sqrt((double)var + eps); }
M3_HD double net_fold_w(float w, double k) { return (double)w * k; }
M3_HD double net_fold_b(float b, float mean, float bias, double k) { return ((double)b - (double)mean) * k + (double)bias; }

// a convolution [taps][in][out] (+ bias [out], BN [out] x 4) folded: w' as float32 or as bf16, b' as float32
inline void net_fold_conv_f32(const float* w, const float* b, const float* scale, const float* bias, const float* mean,
                              const float* var, double eps, int64_t rows, int out, float* w_out, float* b_out) {
    for (int o = 0; o < out; ++o) {
        const double k = net_fold_k(scale[o], var[o], eps);
        for (int64_t r = 0; r < rows; ++r) w_out[r * out + o] = (float)net_fold_w(w[r * out + o], k);
        b_out[o] = (float)net_fold_b(b[o], mean[o], bias[o], k);
    }
}

inline void net_fold_conv_bf16(const float* w, const float* b, const float* scale, const float* bias, const float* mean,
                               const float* var, double eps, int64_t rows, int out, uint16_t* w_out, float* b_out) {
    for (int o = 0; o < out; ++o) {
        const double k = net_fold_k(scale[o], var[o], eps);
        for (int64_t r = 0; r < rows; ++r) w_out[r * out + o] = net_bf16_round_f64(net_fold_w(w[r * out + o], k));
        b_out[o] = (float)net_fold_b(b[o], mean[o], bias[o], k);
    }
}

// ---- the implicit GEMM of a tower convolution ---------------------------------------------------------
// out[m][n] = sum_k A[m][k] * B[k][n],  m = (board * P + r * C + c),  n = output feature,
// k = tap * F + ci with tap = ky * 3 + kx: A[m][k] is the activation at (r + ky - 1, c + kx - 1),
// feature ci, zero outside the board; B[k][n] = w'[ky][kx][ci][n].
// One v_mfma_f32_32x32x16_bf16 takes, in lane l (r = l & 31, h = l >> 5), element j = 0..7:
// A[row r][k = 8h + j] and B[k = 8h + j][col r]. The pre-pack stores B so that a lane's fragment is
// 16 consecutive bytes: [n tile][k step][lane][j].
M3_HD int64_t net_pack_ksteps(int F) { return (int64_t)9 * F / NET_KSTEP; }
M3_HD int64_t net_pack_elems(int F) { return (int64_t)9 * F * F; }

M3_HD int64_t net_pack_index(int F, int64_t k, int n) {
    const int64_t ks = k / NET_KSTEP;
    const int kk = (int)(k % NET_KSTEP), lane = (kk / NET_FRAG) * NET_TILE + n % NET_TILE;
    return (((int64_t)(n / NET_TILE) * net_pack_ksteps(F) + ks) * 64 + lane) * NET_FRAG + kk % NET_FRAG;
}

// the inverse: position in the packed image -> (k, n)
M3_HD void net_unpack_index(int F, int64_t idx, int64_t* k, int* n) {
    const int j = (int)(idx % NET_FRAG), lane = (int)(idx / NET_FRAG % 64);
    const int64_t t = idx / NET_FRAG / 64, ks = t % net_pack_ksteps(F);
    *k = ks * NET_KSTEP + (lane / NET_TILE) * NET_FRAG + j;
    *n = (int)(t / net_pack_ksteps(F)) * NET_TILE + lane % NET_TILE;
}

inline void net_pack(int F, const uint16_t* w /*[9 F][F]*/, uint16_t* packed) {
    for (int64_t k = 0; k < (int64_t)9 * F; ++k)
        for (int n = 0; n < F; ++n) packed[net_pack_index(F, k, n)] = w[k * F + n];
}

inline void net_unpack(int F, const uint16_t* packed, uint16_t* w) {
    for (int64_t i = 0; i < net_pack_elems(F); ++i) {
        int64_t k;
        int n;
        net_unpack_index(F, i, &k, &n);
        w[k * F + n] = packed[i];
    }
}

// Row m of the GEMM and tap -> the row its activation is read from, or -1 for a tap outside the board
// (SAME zero padding) or a row past the batch's end.
M3_HD int64_t net_tap_row(int64_t m, int64_t M, int R, int C, int tap) {
    if (m >= M) return -1;
    const int P = R * C, p = (int)(m % P);
    const int r = p / C + tap / 3 - 1, c = p % C + tap % 3 - 1;
    if (r < 0 || r >= R || c < 0 || c >= C) return -1;
    return m - p + (int64_t)r * C + c;
}

// accumulator register `reg` (0..15) of lane l of a 32x32 result tile: its row; its column is l & 31
M3_HD int net_acc_row(int lane, int reg) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }

// ---- the stem: a gather, bit-exact by its fixed order -------------------------------------------------
// acc = b'[o]; acc += w'[tap][cell][o] over the taps in ascending order that lie on the board and
// whose cell is in [0, CH); ReLU; bf16.
M3_HD uint16_t net_stem_at(const int8_t* board, int R, int C, int CH, int F, int p, int o, const float* w,
                           const float* b) {
    float acc = b[o];
    const int r0 = p / C, c0 = p % C;
    for (int tap = 0; tap < 9; ++tap) {
        const int r = r0 + tap / 3 - 1, c = c0 + tap % 3 - 1;
        if (r < 0 || r >= R || c < 0 || c >= C) continue;
        const int cell = board[r * C + c];
        if (cell < 0 || cell >= CH) continue;
        acc += w[((int64_t)tap * CH + cell) * F + o];
    }
    return net_bf16_round(acc > 0.0f ? acc : 0.0f);
}

// ---- the weight blob ---------------------------------------------------------------------------------
// m3_net_create takes the arrays as one float32 blob in this order (shapes as in include/m3.h):
//   conv.conv.kernel, conv.conv.bias, conv.bn.{scale, bias, mean, var},
//   per residual layer i: conv1.kernel, conv1.bias, bn1.{scale, bias, mean, var},
//                         conv2.kernel, conv2.bias, bn2.{scale, bias, mean, var},
//   value_head.conv.kernel, value_head.conv.bias, value_head.bn.{scale, bias, mean, var},
//   value_head.dense1.{kernel, bias}, value_head.dense2.{kernel, bias},
//   policy_head.conv.kernel, policy_head.conv.bias, policy_head.bn.{scale, bias, mean, var},
//   policy_head.dense.{kernel, bias}
M3_HD int64_t net_blob_len(int P, int A, int CH, int L, int F) {
    const int64_t stem = (int64_t)9 * CH * F + 5 * F, conv = (int64_t)9 * F * F + 5 * F;
    const int64_t value = F + 1 + 4 + (int64_t)P * F + F + F + 1, policy = 2 * F + 2 + 8 + (int64_t)2 * P * A + A;
    return stem + 2 * L * conv + value + policy;
}

}  // namespace m3n
