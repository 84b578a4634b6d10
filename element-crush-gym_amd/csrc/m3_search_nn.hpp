// m3_search_nn.hpp -- launchers of the network-guided tree kernels (m3_search_nn.hip) as m3_api.hip
// calls them. Like m3_search.hpp: the tree sees the board as N bytes and AW action words, so nothing
// here is a template over the board configurations.
#pragma once

#include <hip/hip_runtime.h>

#include "m3_search.hpp"
#include "m3_search_nn_core.hpp"

namespace m3s {

// One round's buffers, all [n] or [n][..] device arrays of the search object.
struct NNRound {
    NTree T;
    // rows of the apply launch (its seeds are the games' cfg seeds, its actions T.action)
    int8_t* row_boards;  // [n][N]
    int32_t* row_na;
    // what the apply launch wrote
    const int8_t* out_boards;
    const int32_t* out_reward;
    const uint32_t* out_flags;
    const uint32_t* out_legal;  // [n][AW]
    // the evaluation batch: fixed size, one row per game
    int8_t* ev_boards;   // [n][N]
    uint8_t* ev_need;    // [n] 1: the game created a non-terminal node this round
    uint32_t* apply_ovf;  // the apply launch's exact-pass count: zeroed by select, read by attach
    uint64_t* stats;      // [0] max nodes used, [1] simulation rounds, [2] apply exact-pass count
};

hipError_t launch_nn_init(hipStream_t st, const NNRound& r, const int8_t* boards, const int32_t* n_actions,
                          const int32_t* rewards, const uint32_t* legal);
hipError_t launch_nn_select(hipStream_t st, const NNRound& r);
hipError_t launch_nn_attach(hipStream_t st, const NNRound& r);
// values [n], logits [n][A] (device): the evaluator's answer to the batch; backup = 0 for the construction
hipError_t launch_nn_commit(hipStream_t st, const NNRound& r, const float* values, const float* logits, int backup);
// the built-in linear evaluator of the batch: W [N][CH][A + 1] (device)
hipError_t launch_nn_linear(hipStream_t st, const NNRound& r, int CH, const float* W, float* values, float* logits);
hipError_t launch_nn_finish(hipStream_t st, const NTree& T, const NResult& r, int32_t* keep_best, uint64_t* stats);
hipError_t launch_nn_advance(hipStream_t st, const NTree& T, const int32_t* actions, int8_t* out_boards,
                             int32_t* out_rewards, int32_t* out_n_actions, uint32_t* out_flags);

}  // namespace m3s
