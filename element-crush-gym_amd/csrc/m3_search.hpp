// m3_search.hpp -- launchers of the tree kernels (m3_search.hip) as m3_api.hip calls them. The tree
// depends on the board only through the cell count N and the action words AW, so nothing here is a
// template over the board configurations: one small translation unit, compiled once.
#pragma once

#include <hip/hip_runtime.h>

#include "m3_search_core.hpp"

namespace m3s {

// One simulation round's buffers, all [n] or [n][..] device arrays of the search object.
struct SearchRound {
    STree T;
    // rows of the apply launch (its seeds are the games' cfg seeds, its actions T.action)
    int8_t* row_boards;  // [n][N]
    int32_t* row_na;
    // what the apply launch wrote
    const int8_t* out_boards;
    const int32_t* out_reward;
    const uint32_t* out_flags;
    const uint32_t* out_legal;  // [n][AW]
    // rows of the rollout launch and what it wrote
    int8_t* ro_boards;
    int32_t* ro_na;
    const int32_t* ro_gain;
    const uint32_t* ro_flags;
    uint32_t* apply_ovf;    // the apply launch's exact-pass count: zeroed by select, read by attach
    uint32_t* ro_counters;  // the rollout launch's 4 counter words: zeroed by attach, read by backup
    uint64_t* stats;        // [0] max nodes used, [1] rounds, [2] apply / [3] rollout exact-pass counts
};

constexpr int SEARCH_BLOCK = 64;  // threads per workgroup: one wave
// Games per workgroup. The tree walk is one lane per game and bound by the latency of its dependent
// loads, not by lanes, so a wave takes few games: 4,096 games then spread over 256 waves instead of
// 64, and each wave moves 16 boards, not 64, behind its walk (DESIGN.md §6.0.1 has the A/B).
constexpr int SEARCH_GAMES = 16;

// ---- what the tree kernels of m3_search.hip and m3_search_nn.hip share --------------------------
__device__ __forceinline__ int64_t game0() { return (int64_t)blockIdx.x * SEARCH_GAMES; }
__device__ __forceinline__ int games_here(int64_t n) {
    const int64_t left = n - game0();
    return left < SEARCH_GAMES ? (int)left : SEARCH_GAMES;
}

// The workgroup's boards, one after the other, the lanes across a board's bytes: dst(j) / src(j)
// are the addresses of game j's board. The loads of a few boards are in flight together.
template <class Dst, class Src>
__device__ __forceinline__ void copy_boards(int nb, int N, Dst dst, Src src) {
#pragma unroll 4
    for (int j = 0; j < nb; ++j) {
        int8_t* d = dst(j);  // nullptr: nothing to copy for this game
        if (d) search_copy_board(d, src(j), N, threadIdx.x, SEARCH_BLOCK);
    }
}
// kernels without a board to move: one lane per game, every lane of the wave in use
__device__ __forceinline__ int64_t lane_game() { return (int64_t)blockIdx.x * SEARCH_BLOCK + threadIdx.x; }

inline unsigned grid_for(int64_t n) { return (unsigned)((n + SEARCH_GAMES - 1) / SEARCH_GAMES); }
inline unsigned grid_flat(int64_t n) { return (unsigned)((n + SEARCH_BLOCK - 1) / SEARCH_BLOCK); }

hipError_t launch_search_init(hipStream_t st, const STree& T, const int8_t* boards, const int32_t* n_actions,
                              const int32_t* rewards, const uint32_t* legal);
hipError_t launch_search_select(hipStream_t st, const SearchRound& r);
hipError_t launch_search_attach(hipStream_t st, const SearchRound& r);
hipError_t launch_search_backup(hipStream_t st, const SearchRound& r);
// keep_best [n]: best_action once more, for a later advance (r.best_action may be null)
hipError_t launch_search_finish(hipStream_t st, const STree& T, const SResult& r, int32_t* keep_best, uint64_t* stats);
// actions [n] (device); the new roots' boards, rewards and n_actions go to out_* (device), out_flags
// gets the game's flag word, with M3_FLAG_BAD_ACTION where the action had no child
hipError_t launch_search_advance(hipStream_t st, const STree& T, const int32_t* actions, int8_t* out_boards,
                                 int32_t* out_rewards, int32_t* out_n_actions, uint32_t* out_flags);
// test hook: search_ucb1 of n (reward_sum, visits, parent_visits, c) tuples
hipError_t launch_search_ucb1(hipStream_t st, int64_t n, const int64_t* reward_sum, const int32_t* visits,
                              const int32_t* parent_visits, const double* c, const double* log_tab, double* out);

}  // namespace m3s
