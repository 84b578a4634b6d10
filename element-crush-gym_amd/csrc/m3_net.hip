// m3_net.hip -- the kernels of the policy/value ResNet (m3_net_core.hpp holds the arithmetic and the
// index maps, DESIGN.md §4.4 the model). Plain launches on the context stream (m3_api.hip):
//   k_net_stem   the one-hot 3x3 stem as a gather (VALU), bit-exact by its fixed order of additions
//   k_net_conv   a tower convolution as an implicit GEMM on v_mfma_f32_32x32x16_bf16: M = positions of
//                the batch, N = F, K = 9F; bias, residual, ReLU and the bf16 rounding in the epilogue
//   k_net_heads  the value and policy heads of one board per block (VALU, float32)
// Activations are NHWC bf16 without a halo: a tap outside the board, and a row past the batch's end,
// is a zero fragment (net_tap_row), so there is no halo that could stop being zero, and an M tile may
// straddle boards: every row of the GEMM finds its own board. No reduction depends on the batch: a
// result element is one lane's accumulator over the K steps in ascending order.
#include "m3_net.hpp"

namespace m3n {
namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int NET_BLOCK = 256;
constexpr int CONV_WAVES = NET_BLOCK / 64;  // waves of a block, along M
constexpr int CONV_MT = 2, CONV_NT = 2;     // 32x32 tiles of a wave: 64 rows x 64 features

__global__ void __launch_bounds__(NET_BLOCK) k_net_stem(NetShape s, int64_t total, const int8_t* boards,
                                                        const float* w, const float* b, uint16_t* act) {
    const int64_t t = (int64_t)blockIdx.x * NET_BLOCK + threadIdx.x;
    if (t >= total) return;
    const int64_t m = t / s.F;
    const int o = (int)(t % s.F), p = (int)(m % s.P);
    act[t] = net_stem_at(boards + (m - p), s.R, s.C, s.CH, s.F, p, o, w, b);
}

__device__ __forceinline__ bf16x8 frag_load(const uint4* p) {
    const uint4 v = p ? *p : make_uint4(0u, 0u, 0u, 0u);
    return __builtin_bit_cast(bf16x8, v);
}

__global__ void __launch_bounds__(NET_BLOCK) k_net_conv(NetShape s, int64_t M, const uint16_t* in,
                                                        const uint16_t* packed, const float* bias,
                                                        const uint16_t* res, uint16_t* out) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t m0 = ((int64_t)blockIdx.x * CONV_WAVES + wave) * (CONV_MT * NET_TILE);
    if (m0 >= M) return;  // (the whole wave)
    const int F = s.F, nt0 = blockIdx.y * CONV_NT;
    const bool second = nt0 + 1 < F / NET_TILE;  // an odd count of N tiles: the last wave column has one
    const int64_t KS = net_pack_ksteps(F);
    const int row = lane & 31, half = lane >> 5;
    const uint4* wp = reinterpret_cast<const uint4*>(packed) + (int64_t)nt0 * KS * 64 + lane;
    f32x16 acc[CONV_MT][CONV_NT];
#pragma unroll
    for (int i = 0; i < CONV_MT; ++i)
#pragma unroll
        for (int j = 0; j < CONV_NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
    for (int tap = 0; tap < 9; ++tap) {
        const uint4* ap[CONV_MT];
#pragma unroll
        for (int i = 0; i < CONV_MT; ++i) {
            const int64_t src = net_tap_row(m0 + i * NET_TILE + row, M, s.R, s.C, tap);
            ap[i] = src < 0 ? nullptr : reinterpret_cast<const uint4*>(in + src * F + half * NET_FRAG);
        }
        const uint4* wt = wp + (int64_t)tap * (F / NET_KSTEP) * 64;
        for (int ks = 0; ks < F / NET_KSTEP; ++ks) {
            const bf16x8 a0 = frag_load(ap[0] ? ap[0] + 2 * ks : nullptr);
            const bf16x8 a1 = frag_load(ap[1] ? ap[1] + 2 * ks : nullptr);
            const bf16x8 b0 = frag_load(wt + (int64_t)ks * 64);
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc[0][0], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, acc[1][0], 0, 0, 0);
            if (second) {
                const bf16x8 b1 = frag_load(wt + (KS + ks) * 64);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc[1][1], 0, 0, 0);
            }
        }
    }
    // float32 epilogue: + b', + residual (the bf16 activation widened), ReLU, one rounding to bf16
#pragma unroll
    for (int j = 0; j < CONV_NT; ++j) {
        if (j && !second) continue;
        const int n = (nt0 + j) * NET_TILE + row;
        const float bn = bias[n];
#pragma unroll
        for (int i = 0; i < CONV_MT; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t m = m0 + i * NET_TILE + net_acc_row(lane, r);
                if (m >= M) continue;
                float v = acc[i][j][r] + bn;
                if (res) v += net_bf16_widen(res[m * F + n]);
                out[m * F + n] = net_bf16_round(v > 0.0f ? v : 0.0f);
            }
    }
}

// One block per board. LDS: hv [P] (value 1x1), hp [2P] (policy 1x1, NHWC flat), h1 [F] (dense1).
__global__ void __launch_bounds__(NET_BLOCK) k_net_heads(NetShape s, const uint16_t* act, NetHeads h,
                                                         const uint8_t* need, float* values, float* logits) {
    extern __shared__ float lds[];
    const int64_t b = blockIdx.x;
    if (need && !need[b]) return;  // (the whole block)
    const int P = s.P, F = s.F, A = s.A;
    float *hv = lds, *hp = lds + P, *h1 = lds + 3 * P;
    const uint16_t* x = act + b * P * F;
    for (int p = threadIdx.x; p < P; p += NET_BLOCK) {
        float v = h.v_b[0], p0 = h.p_b[0], p1 = h.p_b[1];
        for (int f = 0; f < F; ++f) {
            const float a = net_bf16_widen(x[(int64_t)p * F + f]);
            v += a * h.v_w[f];
            p0 += a * h.p_w[2 * f];
            p1 += a * h.p_w[2 * f + 1];
        }
        hv[p] = v > 0.0f ? v : 0.0f;
        hp[2 * p] = p0 > 0.0f ? p0 : 0.0f;
        hp[2 * p + 1] = p1 > 0.0f ? p1 : 0.0f;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < F; j += NET_BLOCK) {
        float v = h.d1_b[j];
        for (int p = 0; p < P; ++p) v += hv[p] * h.d1_w[(int64_t)p * F + j];
        h1[j] = v > 0.0f ? v : 0.0f;
    }
    for (int a = threadIdx.x; a < A; a += NET_BLOCK) {
        float v = h.pd_b[a];
        for (int q = 0; q < 2 * P; ++q) v += hp[q] * h.pd_w[(int64_t)q * A + a];
        logits[b * A + a] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float v = h.d2_b[0];
        for (int j = 0; j < F; ++j) v += h1[j] * h.d2_w[j];
        values[b] = v > 0.0f ? v : 0.0f;
    }
}

__global__ void __launch_bounds__(NET_BLOCK) k_net_widen(int64_t count, const uint16_t* act, float* out) {
    const int64_t t = (int64_t)blockIdx.x * NET_BLOCK + threadIdx.x;
    if (t < count) out[t] = net_bf16_widen(act[t]);
}

unsigned blocks_for(int64_t items) { return (unsigned)((items + NET_BLOCK - 1) / NET_BLOCK); }

}  // namespace

hipError_t launch_net_stem(hipStream_t st, const NetShape& s, int64_t n, const int8_t* boards, const float* w,
                           const float* b, uint16_t* act) {
    const int64_t total = n * s.P * s.F;
    if (!total) return hipSuccess;
    hipLaunchKernelGGL(k_net_stem, dim3(blocks_for(total)), dim3(NET_BLOCK), 0, st, s, total, boards, w, b, act);
    return hipGetLastError();
}

hipError_t launch_net_conv(hipStream_t st, const NetShape& s, int64_t n, const uint16_t* in, const uint16_t* packed,
                           const float* b, const uint16_t* res, uint16_t* out) {
    const int64_t M = n * s.P;
    if (!M) return hipSuccess;
    const int64_t rows = CONV_WAVES * CONV_MT * NET_TILE;
    const int nt = s.F / NET_TILE;
    hipLaunchKernelGGL(k_net_conv, dim3((unsigned)((M + rows - 1) / rows), (unsigned)((nt + CONV_NT - 1) / CONV_NT)),
                       dim3(NET_BLOCK), 0, st, s, M, in, packed, b, res, out);
    return hipGetLastError();
}

hipError_t launch_net_heads(hipStream_t st, const NetShape& s, int64_t n, const uint16_t* act, const NetHeads& h,
                            const uint8_t* need, float* values, float* logits) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_net_heads, dim3((unsigned)n), dim3(NET_BLOCK), (size_t)(3 * s.P + s.F) * sizeof(float), st, s,
                       act, h, need, values, logits);
    return hipGetLastError();
}

hipError_t launch_net_widen(hipStream_t st, int64_t count, const uint16_t* act, float* out) {
    if (!count) return hipSuccess;
    hipLaunchKernelGGL(k_net_widen, dim3(blocks_for(count)), dim3(NET_BLOCK), 0, st, count, act, out);
    return hipGetLastError();
}

}  // namespace m3n
