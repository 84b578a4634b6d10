// m3_lookahead.hpp -- device one-ply lookahead (BoardV2.greedy_action, boardv2.py:209-218): the step
// reward of EVERY legal action of every board, and the greedy pick. Included at the end of
// m3_kernels.hpp; the logic that needs no wave is in m3_lookahead_core.hpp (also built for the host,
// tests/lookahead_host).
//
// k_lookahead: a one-wave workgroup stages LookK::BPW boards HBM -> LDS as k_apply does, one lane per
// board derives the legal set (as k_legal) into LDS, and a wave prefix sum of the popcounts numbers
// the group's (board, legal action) candidates. Rounds of 64: lane j of a round finds its board in
// the prefix, selects its k-th set bit and runs the whole apply_action -- dead-board shuffle and all
// -- on a private copy, on the register chain reseeded from (seed, mt[397]). The lanes fold into one
// LDS record per board: a 64-bit atomicMax on the packed key (reward, then lower id), the OR of the
// flags, the draws of the highest id. A per-board loop over its actions would hold the wave to its
// fullest board (legal counts run 6..32 at 9x9x6 and 19..60 at 16x16x8).
//
// Exact pass: a candidate whose first scan forms more groups than KS::GCAP, or whose chain runs past
// its limit, voids its board: the board's index goes to a list (one entry per board, O(n)), and
// k_lookahead_fix redoes ALL candidates of a listed board -- one board per wave, a candidate per
// lane, FullMT + ArrayStore in scratch -- and rewrites the board's outputs. It is exact whatever
// share of the candidates overflows.
//
// The 32 x 32-frame configurations run one board per wave and take ~13 minutes per kernel to
// compile: launch_lookahead<CF> returns M3_ERR_UNSUPPORTED for them without instantiating a kernel.
#pragma once

#include "m3_lookahead_core.hpp"

namespace m3k {
struct LookArgs {
    Shape shape;
    int64_t n;
    const int8_t* boards;
    const uint32_t* seeds;
    const int32_t* n_actions;  // nullable: num_moves - moves[b] (the env)
    const int32_t* moves;
    int num_moves;
    int32_t* best_action;      // every output nullable
    int32_t* best_reward;
    int32_t* values;           // [n][A]: the reward of a legal id, -1 otherwise
    uint32_t* last_draws;
    uint32_t* flags;
    uint32_t* ovf_count;       // zeroed by the caller
    uint32_t* ovf_list;        // [n]
    uint32_t* bad_cells;       // nullable: set to 1 if a cell value lies outside [0, 127]
};
}  // namespace m3k
using m3k::LookArgs;

namespace {

// Boards per wave. More boards fill the last round of 64 better (the mean group has BPW x 17 / x 39
// candidates) and cost LDS for their staging and one lane each in the legal phase; with too many the
// legal phase, which runs one lane per board, and the longest candidate of more rounds hold the wave.
// A/B on the MI355X (65,536 boards of 9x9x6 / 16,384 of 16x16x8, min-max of five repeats, ms;
// profiles/lookahead_bench.json): 9x9x6 16 / 32 / 64 boards: 0.908-0.967 / 0.879-0.892 / 1.256-1.261;
// 16x16x8 4 / 8 / 16 boards: 1.189-1.261 / 1.216-1.243 / 1.483-1.506 (4 and 8 within noise).
// At 32 boards the 9x9x6 kernel's 13.8 KB of LDS caps it at 2 waves per SIMD: 242 VGPRs, nothing spilled
// (16 boards: bounded for 4 waves, 128 VGPRs, 436 B of scratch).
#ifndef M3_LOOK_BPW
#define M3_LOOK_BPW 32
#endif
#ifndef M3_LOOK_BPW16
#define M3_LOOK_BPW16 8
#endif
template <class CF>
struct LookK {
    // (frame configurations: 16, so that a group's bytes start 16-byte aligned for every board size)
    static constexpr int BPW = CF::DYN ? 16 : (CF::N <= 128 ? M3_LOOK_BPW : M3_LOOK_BPW16);
    static_assert(BPW >= 1 && BPW <= 64, "one lane per board in the legal phase");
    static_assert(CF::DYN ? BPW % 16 == 0 : (BPW * CF::N) % 16 == 0, "the staging copy loads 16-byte chunks");
    // waves per SIMD the registers are bounded for: the frame configurations 1 as in every kernel that
    // runs their cascade (nothing may reach scratch); the specialised shapes as k_env_step
    static constexpr int WPS = KS<CF>::STEP_WPS;
};

__device__ __forceinline__ void look_store(const LookArgs& a, int64_t b, uint64_t key, uint32_t flags,
                                           uint32_t last_draws) {
    if (a.best_action) a.best_action[b] = look_key_action(key);
    if (a.best_reward) a.best_reward[b] = look_key_reward(key);
    if (a.last_draws) a.last_draws[b] = last_draws;
    if (a.flags) a.flags[b] = flags;
}

__device__ __forceinline__ int look_n_actions(const LookArgs& a, int64_t b) {
    return a.n_actions ? a.n_actions[b] : a.num_moves - a.moves[b];
}

template <class CF>
__global__ void __launch_bounds__(KS<CF>::B, LookK<CF>::WPS) k_lookahead(LookArgs a) {
    using K = KS<CF>;
    constexpr int G = LookK<CF>::BPW;
    constexpr int AWS = CF::AW;  // row stride of the legal sets in LDS
    __shared__ __attribute__((aligned(16))) uint8_t lds[G * CF::N + 16];
    __shared__ uint32_t gtab[LdsTable<CF, K::GCAP, K::B>::WORDS];
    __shared__ uint32_t act_s[G * AWS];
    __shared__ uint32_t pre_s[G + 1];
    __shared__ uint32_t seed_s[G], m397_s[G];
    __shared__ int32_t nact_s[G];
    __shared__ LookAcc acc_s[G];
    const typename CF::Dim dm(a.shape);
    const int NC = dm.cells(), A = dm.actions(), AW = dm.aw();
    const int64_t b0 = (int64_t)blockIdx.x * G;
    const int nb = (int)((a.n - b0) < G ? (a.n - b0) : G);
    flag_bad_cells(block_copy_in_checked<K::B>(a.boards + b0 * NC, lds, nb * NC), a.bad_cells);
    lds_sync();
    const int t = threadIdx.x;
    uint32_t cnt = 0u;
    if (t < nb) {  // the legal set of board t, as k_legal
        typename CF::Bd P[CF::NP], HL, VL;
        lds_to_planes<CF>(lds, t, P, dm);
        legal_masks<CF>(P, special_mask<CF, CF::NP>(P), HL, VL, dm);
        uint32_t act[CF::AW];
        action_bits<CF>(HL, VL, act, dm);
#pragma unroll
        for (int i = 0; i < CF::AW; ++i) {
            const uint32_t w = i < AW ? act[i] : 0u;
            act_s[t * AWS + i] = w;
            cnt += (uint32_t)__builtin_popcount(w);
        }
        const uint32_t s = a.seeds[b0 + t];
        const int na = look_n_actions(a, b0 + t);
        seed_s[t] = s;
        m397_s[t] = mt_state397(s);
        nact_s[t] = na;
        LookAcc acc;
        look_acc_init(acc, na, cnt);
        acc_s[t] = acc;
    }
    uint32_t inc = cnt;  // wave inclusive prefix sum (lanes past nb add 0)
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t v = __shfl_up(inc, d);
        if (t >= d) inc += v;
    }
    if (t < nb) pre_s[t] = inc - cnt;
    if (t == nb - 1) pre_s[nb] = inc;
    lds_sync();
    const uint32_t total = pre_s[nb];
    if (a.values) {  // -1 for every id that is not legal; the candidates write the others
        for (int i = t; i < nb * A; i += K::B) {
            const int g = i / A, id = i - g * A;
            if (!((act_s[g * AWS + (id >> 5)] >> (id & 31)) & 1u)) a.values[(b0 + g) * A + id] = -1;
        }
    }
    LdsTable<CF, K::GCAP, K::B> st{as_lds(gtab + t)};  // overflow -> k_lookahead_fix
    for (uint32_t base = 0u; base < total; base += (uint32_t)K::B) {
        const uint32_t j = base + (uint32_t)t;
        if (j < total) {  // (a lane without a candidate in the last round is inactive)
            const int g = look_find_board(pre_s, nb, j);
            const int action = look_kth_bit(act_s + g * AWS, AW, j - pre_s[g]);
            typename CF::Bd P[CF::NP];
            lds_to_planes<CF>(lds, g, P, dm);
            const LookCand c =
                look_eval<CF, typename K::Chain>(P, seed_s[g], m397_s[g], nact_s[g], action, st, dm);
            if (a.values && !c.redo) a.values[(b0 + g) * A + action] = c.reward;
            look_fold(&acc_s[g], c, action, j + 1u == pre_s[g + 1]);
        }
    }
    lds_sync();
    if (t < nb) {
        const LookAcc acc = acc_s[t];
        if (acc.redo) {
            const uint32_t slot = atomicAdd(a.ovf_count, 1u);
            a.ovf_list[slot] = (uint32_t)(b0 + t);
        } else {
            look_store(a, b0 + t, acc.key, acc.flags, acc.last_draws);
        }
    }
}

// redo the listed boards whole: one board per wave, a candidate per lane (FullMT and the full group
// table in lane-private scratch, as k_apply_fix)
template <class CF>
__global__ void __launch_bounds__(FIX_BLOCK) k_lookahead_fix(LookArgs a) {
    static_assert(FIX_BLOCK == 64, "one wave: the reduction below is a wave's");
    const uint32_t cnt = *a.ovf_count;
    const typename CF::Dim dm(a.shape);
    const int A = dm.actions(), AW = dm.aw();
    const uint32_t t = threadIdx.x;
    for (uint32_t i = blockIdx.x; i < cnt; i += gridDim.x) {
        const int64_t b = a.ovf_list[i];
        typename CF::Bd P[CF::NP], HL, VL;
        bytes_to_planes<CF>(a.boards + b * dm.cells(), P, dm);
        legal_masks<CF>(P, special_mask<CF, CF::NP>(P), HL, VL, dm);
        uint32_t act[CF::AW];
        action_bits<CF>(HL, VL, act, dm);
#pragma unroll
        for (int w = 0; w < CF::AW; ++w)
            if (w >= AW) act[w] = 0u;
        const int na = look_n_actions(a, b);
        uint64_t key = LOOK_KEY_NONE;
        uint32_t fl = 0u, ld = 0u;
        FullMT mt;
        ArrayStore<CF> st;
        look_exact<CF>(P, act, a.seeds[b], na, t, (uint32_t)FIX_BLOCK, key, fl, ld,
                       a.values ? a.values + b * A : nullptr, mt, st, dm);
#pragma unroll
        for (int d = 32; d; d >>= 1) {  // (every lane is back: the loop above is over uniform bounds)
            const unsigned long long k2 = __shfl_xor((unsigned long long)key, d);
            if (look_key_better(k2, key)) key = k2;
            fl |= __shfl_xor(fl, d);
            const uint32_t l2 = __shfl_xor(ld, d);  // (only the lane of the highest id holds draws)
            ld = l2 > ld ? l2 : ld;
        }
        if (t == 0u) {
            LookAcc acc;
            look_acc_init(acc, na, look_count(act, AW));
            look_store(a, b, key, fl | acc.flags, ld);
        }
    }
}

}  // namespace

namespace m3k {

template <class CF>
int launch_lookahead(hipStream_t stream, const LookArgs& a) {
    if constexpr (CF::W > 8) {
        return set_err(M3_ERR_UNSUPPORTED, "lookahead is not built for boards with a side above 16 (the 32 x 32 frame)");
    } else {
        if (a.n == 0) return M3_OK;
        constexpr int G = LookK<CF>::BPW;
        hipLaunchKernelGGL(k_lookahead<CF>, dim3((unsigned)((a.n + G - 1) / G)), dim3(KS<CF>::B), 0, stream, a);
        HIP_TRY(hipGetLastError());
        // grid-strides over the device-side count of listed boards; blocks past it exit at once
        const int64_t gf = std::min<int64_t>(std::max<int64_t>(a.n / 16, 16), 2048);
        hipLaunchKernelGGL(k_lookahead_fix<CF>, dim3((unsigned)gf), dim3(FIX_BLOCK), 0, stream, a);
        HIP_TRY(hipGetLastError());
        return M3_OK;
    }
}

}  // namespace m3k
