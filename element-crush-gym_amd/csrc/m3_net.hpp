// m3_net.hpp -- launchers of the policy/value network's kernels (m3_net.hip) as m3_api.hip calls them.
// The network sees the board as R x C int8 cells, so nothing here is a template over the board
// configurations.
#pragma once

#include <hip/hip_runtime.h>

#include "m3_net_core.hpp"

namespace m3n {

// the board and network shape every kernel takes
struct NetShape {
    int R, C, P, A, CH, F;
};

// the heads' weights (device, float32), folded
struct NetHeads {
    const float* v_w;    // [F]      value 1x1 conv
    const float* v_b;    // [1]
    const float* d1_w;   // [P][F]
    const float* d1_b;   // [F]
    const float* d2_w;   // [F]
    const float* d2_b;   // [1]
    const float* p_w;    // [F][2]   policy 1x1 conv
    const float* p_b;    // [2]
    const float* pd_w;   // [2P][A]
    const float* pd_b;   // [A]
};

// boards [n][P] -> act [n * P][F] bf16
hipError_t launch_net_stem(hipStream_t st, const NetShape& s, int64_t n, const int8_t* boards, const float* w,
                           const float* b, uint16_t* act);
// out = relu(conv3x3(in) + b (+ res)), all [M][F] bf16 with M = n * P; out may be res, never in
hipError_t launch_net_conv(hipStream_t st, const NetShape& s, int64_t n, const uint16_t* in, const uint16_t* packed,
                           const float* b, const uint16_t* res, uint16_t* out);
// act [n * P][F] -> values [n], logits [n][A]; need (nullable): rows with need == 0 are not written
hipError_t launch_net_heads(hipStream_t st, const NetShape& s, int64_t n, const uint16_t* act, const NetHeads& h,
                            const uint8_t* need, float* values, float* logits);
// act [count] bf16 -> out [count] float32
hipError_t launch_net_widen(hipStream_t st, int64_t count, const uint16_t* act, float* out);

}  // namespace m3n
