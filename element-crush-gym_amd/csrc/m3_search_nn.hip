// m3_search_nn.hip -- the tree kernels of the network-guided device MCTS (m3_search_nn_core.hpp holds
// the logic). One round is k_nn_select -> launch_apply -> k_nn_attach, which leaves the evaluation
// batch (one board per game and a `need` byte), then -- after the evaluator -- k_nn_commit: plain
// launches on the context stream (m3_api.hip). As in m3_search.hip one lane per game walks the tree
// (SEARCH_GAMES games per wave), and the 64 lanes of the wave then move those games' boards and logits
// rows, consecutive lanes on consecutive bytes or floats.
#include "m3_search_nn.hpp"

namespace m3s {
namespace {

__global__ void __launch_bounds__(SEARCH_BLOCK) k_nn_init(NNRound r, const int8_t* boards, const int32_t* n_actions,
                                                          const int32_t* rewards, const uint32_t* legal) {
    const NTree& T = r.T;
    const int64_t g0 = game0(), g = g0 + threadIdx.x;
    const int nb = games_here(T.n);
    if ((int)threadIdx.x < nb) r.ev_need[g] = (uint8_t)nn_init_root(T, g, n_actions[g], rewards[g], legal + g * T.AW);
    copy_boards(nb, T.N, [&](int j) { return nn_board(T, g0 + j, 0); }, [&](int j) { return boards + (g0 + j) * T.N; });
    copy_boards(nb, T.N, [&](int j) { return r.ev_boards + (g0 + j) * T.N; },
                [&](int j) { return boards + (g0 + j) * T.N; });
}

__global__ void __launch_bounds__(SEARCH_BLOCK) k_nn_select(NNRound r) {
    __shared__ int32_t s_leaf[SEARCH_GAMES];
    const NTree& T = r.T;
    const int64_t g0 = game0(), g = g0 + threadIdx.x;
    const int nb = games_here(T.n);
    if (blockIdx.x == 0 && threadIdx.x == 0) *r.apply_ovf = 0u;
    if ((int)threadIdx.x < nb) {
        r.row_na[g] = nn_select(T, g);
        s_leaf[threadIdx.x] = T.leaf[g];
    }
    __syncthreads();
    // the leaf's board is the row of the apply launch; a game that does not expand keeps it as a
    // terminal row (n_actions = 0)
    copy_boards(nb, T.N, [&](int j) { return r.row_boards + (g0 + j) * T.N; },
                [&](int j) { return (const int8_t*)nn_board(T, g0 + j, s_leaf[j]); });
}

__global__ void __launch_bounds__(SEARCH_BLOCK) k_nn_attach(NNRound r) {
    __shared__ int32_t s_child[SEARCH_GAMES];
    const NTree& T = r.T;
    const int64_t g0 = game0(), g = g0 + threadIdx.x;
    const int nb = games_here(T.n);
    if (blockIdx.x == 0 && threadIdx.x == 0) r.stats[2] += *r.apply_ovf;
    if ((int)threadIdx.x < nb) {
        r.ev_need[g] = (uint8_t)nn_attach(T, g, r.out_reward[g], r.out_flags[g], r.out_legal + g * T.AW);
        s_child[threadIdx.x] = T.pending[g];
    }
    __syncthreads();
    // the batch row: the new child's board (also kept in its node), or the leaf's from the apply row
    copy_boards(nb, T.N, [&](int j) { return r.ev_boards + (g0 + j) * T.N; },
                [&](int j) { return (s_child[j] >= 0 ? r.out_boards : (const int8_t*)r.row_boards) + (g0 + j) * T.N; });
    copy_boards(nb, T.N, [&](int j) { return s_child[j] >= 0 ? nn_board(T, g0 + j, s_child[j]) : (int8_t*)nullptr; },
                [&](int j) { return r.out_boards + (g0 + j) * T.N; });
}

__global__ void __launch_bounds__(SEARCH_BLOCK) k_nn_commit(NNRound r, const float* values, const float* logits,
                                                            int backup) {
    __shared__ int32_t s_node[SEARCH_GAMES];  // the node whose row this round evaluated; -1 without
    __shared__ int32_t s_bad[SEARCH_GAMES];
    const NTree& T = r.T;
    const int64_t g0 = game0(), g = g0 + threadIdx.x;
    const int nb = games_here(T.n);
    if (blockIdx.x == 0 && threadIdx.x == 0 && backup) r.stats[1] += 1;
    if ((int)threadIdx.x < nb) {
        const int32_t node = T.gflags[g] ? -1 : T.pending[g];
        const bool need = node >= 0 && T.link[nn_base(T, g) + node].n_actions >= 1;
        s_node[threadIdx.x] = need ? node : -1;
        s_bad[threadIdx.x] = need && !nn_finite(values[g]);
    }
    __syncthreads();
    // the needed rows go into their nodes, the lanes across a row's floats; each lane looks at the
    // legal logits among its own
    for (int j = 0; j < nb; ++j) {
        const int32_t node = s_node[j];
        if (node < 0) continue;
        const uint32_t* legal = T.untried + (nn_base(T, g0 + j) + node) * T.AW;  // (untouched since the node was made)
        if (nn_store_row(nn_row(T, g0 + j, node), logits + (g0 + j) * T.A, legal, T.A, threadIdx.x, SEARCH_BLOCK))
            s_bad[j] = 1;  // (every writer stores the same value)
    }
    __syncthreads();
    if ((int)threadIdx.x < nb) nn_commit(T, g, values[g], s_bad[threadIdx.x] != 0, backup != 0);
}

// a wave per board, the lanes across the A + 1 outputs: a row of W is read by consecutive lanes
__global__ void __launch_bounds__(SEARCH_BLOCK) k_nn_linear(int64_t n, int N, int CH, int A, const int8_t* boards,
                                                            const uint8_t* need, const float* W, float* values,
                                                            float* logits) {
    const int64_t b = blockIdx.x;
    if (b >= n || !need[b]) return;
    nn_linear_row(boards + b * N, W, N, CH, A, values + b, logits + b * A, threadIdx.x, SEARCH_BLOCK);
}

__global__ void __launch_bounds__(SEARCH_BLOCK) k_nn_finish(NTree T, NResult r, int32_t* keep_best, uint64_t* stats) {
    const int64_t g = lane_game();
    if (g >= T.n) return;
    keep_best[g] = nn_finish(T, g, r);
    atomicMax((unsigned long long*)&stats[0], (unsigned long long)T.used[g]);
}

__global__ void __launch_bounds__(SEARCH_BLOCK) k_nn_advance(NTree T, const int32_t* actions, int8_t* out_boards,
                                                             int32_t* out_rewards, int32_t* out_n_actions,
                                                             uint32_t* out_flags) {
    __shared__ int32_t s_root[SEARCH_GAMES];
    const int64_t g0 = game0(), g = g0 + threadIdx.x;
    const int nb = games_here(T.n);
    if ((int)threadIdx.x < nb) {
        int32_t root = nn_advance(T, g, actions[g]);
        out_flags[g] = T.gflags[g] | (root < 0 ? SF_BAD_ACTION : 0u);
        if (root < 0) root = T.root[g];
        const SNodeLink l = T.link[nn_base(T, g) + root];
        out_rewards[g] = l.state_reward;
        out_n_actions[g] = l.n_actions;
        s_root[threadIdx.x] = root;
    }
    __syncthreads();
    copy_boards(nb, T.N, [&](int j) { return out_boards + (g0 + j) * T.N; },
                [&](int j) { return (const int8_t*)nn_board(T, g0 + j, s_root[j]); });
}

}  // namespace

hipError_t launch_nn_init(hipStream_t st, const NNRound& r, const int8_t* boards, const int32_t* n_actions,
                          const int32_t* rewards, const uint32_t* legal) {
    hipLaunchKernelGGL(k_nn_init, dim3(grid_for(r.T.n)), dim3(SEARCH_BLOCK), 0, st, r, boards, n_actions, rewards, legal);
    return hipGetLastError();
}

hipError_t launch_nn_select(hipStream_t st, const NNRound& r) {
    hipLaunchKernelGGL(k_nn_select, dim3(grid_for(r.T.n)), dim3(SEARCH_BLOCK), 0, st, r);
    return hipGetLastError();
}

hipError_t launch_nn_attach(hipStream_t st, const NNRound& r) {
    hipLaunchKernelGGL(k_nn_attach, dim3(grid_for(r.T.n)), dim3(SEARCH_BLOCK), 0, st, r);
    return hipGetLastError();
}

hipError_t launch_nn_commit(hipStream_t st, const NNRound& r, const float* values, const float* logits, int backup) {
    hipLaunchKernelGGL(k_nn_commit, dim3(grid_for(r.T.n)), dim3(SEARCH_BLOCK), 0, st, r, values, logits, backup);
    return hipGetLastError();
}

hipError_t launch_nn_linear(hipStream_t st, const NNRound& r, int CH, const float* W, float* values, float* logits) {
    hipLaunchKernelGGL(k_nn_linear, dim3((unsigned)r.T.n), dim3(SEARCH_BLOCK), 0, st, r.T.n, r.T.N, CH, r.T.A,
                       (const int8_t*)r.ev_boards, (const uint8_t*)r.ev_need, W, values, logits);
    return hipGetLastError();
}

hipError_t launch_nn_finish(hipStream_t st, const NTree& T, const NResult& r, int32_t* keep_best, uint64_t* stats) {
    hipLaunchKernelGGL(k_nn_finish, dim3(grid_flat(T.n)), dim3(SEARCH_BLOCK), 0, st, T, r, keep_best, stats);
    return hipGetLastError();
}

hipError_t launch_nn_advance(hipStream_t st, const NTree& T, const int32_t* actions, int8_t* out_boards,
                             int32_t* out_rewards, int32_t* out_n_actions, uint32_t* out_flags) {
    hipLaunchKernelGGL(k_nn_advance, dim3(grid_for(T.n)), dim3(SEARCH_BLOCK), 0, st, T, actions,
                       out_boards, out_rewards, out_n_actions, out_flags);
    return hipGetLastError();
}

}  // namespace m3s
