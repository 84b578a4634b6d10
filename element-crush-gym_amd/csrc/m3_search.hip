// m3_search.hip -- the tree kernels of the device-resident MCTS (m3_search_core.hpp holds the logic).
// One simulation round is k_search_select -> launch_apply -> k_search_attach -> launch_rollouts ->
// k_search_backup, plain launches on the context stream (m3_api.hip, m3_search_run). One lane per
// game walks the tree (SEARCH_GAMES games per wave); the 64 lanes of the wave then move those games' boards, with
// consecutive lanes on consecutive bytes of a board.
#include "m3_search.hpp"

namespace m3s {
namespace {

__global__ void __launch_bounds__(SEARCH_BLOCK) k_search_init(STree T, const int8_t* boards, const int32_t* n_actions,
                                                              const int32_t* rewards, const uint32_t* legal) {
    const int64_t g0 = game0(), g = g0 + threadIdx.x;
    const int nb = games_here(T.n);
    if ((int)threadIdx.x < nb) search_init_root(T, g, n_actions[g], rewards[g], legal + g * T.AW);
    copy_boards(nb, T.N, [&](int j) { return node_board(T, g0 + j, 0); },
                [&](int j) { return boards + (g0 + j) * T.N; });
}

__global__ void __launch_bounds__(SEARCH_BLOCK) k_search_select(SearchRound r) {
    __shared__ int32_t s_leaf[SEARCH_GAMES];
    const STree& T = r.T;
    const int64_t g0 = game0(), g = g0 + threadIdx.x;
    const int nb = games_here(T.n);
    if (blockIdx.x == 0 && threadIdx.x == 0) *r.apply_ovf = 0u;
    if ((int)threadIdx.x < nb) {
        r.row_na[g] = search_select(T, g);
        s_leaf[threadIdx.x] = T.leaf[g];
    }
    __syncthreads();
    // the leaf's board is the row of the apply launch; a game that does not expand keeps it as a
    // terminal row (n_actions = 0), and k_search_attach takes its rollout row from there
    copy_boards(nb, T.N, [&](int j) { return r.row_boards + (g0 + j) * T.N; },
                [&](int j) { return (const int8_t*)node_board(T, g0 + j, s_leaf[j]); });
}

__global__ void __launch_bounds__(SEARCH_BLOCK) k_search_attach(SearchRound r) {
    __shared__ int32_t s_child[SEARCH_GAMES];
    const STree& T = r.T;
    const int64_t g0 = game0(), g = g0 + threadIdx.x;
    const int nb = games_here(T.n);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        r.stats[2] += *r.apply_ovf;
        for (int w = 0; w < 4; ++w) r.ro_counters[w] = 0u;
    }
    if ((int)threadIdx.x < nb) {
        const int32_t before = T.used[g];
        r.ro_na[g] = search_attach(T, g, r.out_reward[g], r.out_flags[g], r.out_legal + g * T.AW);
        s_child[threadIdx.x] = T.used[g] != before ? T.leaf[g] : -1;
    }
    __syncthreads();
    // the rollout row: the new child's board (also kept in its node), or the leaf's from the apply row
    copy_boards(nb, T.N, [&](int j) { return r.ro_boards + (g0 + j) * T.N; },
                [&](int j) { return (s_child[j] >= 0 ? r.out_boards : (const int8_t*)r.row_boards) + (g0 + j) * T.N; });
    copy_boards(nb, T.N, [&](int j) { return s_child[j] >= 0 ? node_board(T, g0 + j, s_child[j]) : (int8_t*)nullptr; },
                [&](int j) { return r.out_boards + (g0 + j) * T.N; });
}

__global__ void __launch_bounds__(SEARCH_BLOCK) k_search_backup(SearchRound r) {
    const int64_t g = lane_game();
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        r.stats[1] += 1;
        r.stats[3] += r.ro_counters[0];
    }
    if (g < r.T.n) search_backup(r.T, g, r.ro_gain[g], r.ro_flags[g]);
}

__global__ void __launch_bounds__(SEARCH_BLOCK) k_search_finish(STree T, SResult r, int32_t* keep_best, uint64_t* stats) {
    const int64_t g = lane_game();
    if (g >= T.n) return;
    keep_best[g] = search_finish(T, g, r);
    atomicMax((unsigned long long*)&stats[0], (unsigned long long)T.used[g]);
}

__global__ void __launch_bounds__(SEARCH_BLOCK) k_search_advance(STree T, const int32_t* actions, int8_t* out_boards,
                                                                 int32_t* out_rewards, int32_t* out_n_actions,
                                                                 uint32_t* out_flags) {
    __shared__ int32_t s_root[SEARCH_GAMES];
    const int64_t g0 = game0(), g = g0 + threadIdx.x;
    const int nb = games_here(T.n);
    if ((int)threadIdx.x < nb) {
        int32_t root = search_advance(T, g, actions[g]);
        out_flags[g] = T.gflags[g] | (root < 0 ? SF_BAD_ACTION : 0u);
        if (root < 0) root = T.root[g];
        const SNodeLink l = T.link[node_base(T, g) + root];
        out_rewards[g] = l.state_reward;
        out_n_actions[g] = l.n_actions;
        s_root[threadIdx.x] = root;
    }
    __syncthreads();
    copy_boards(nb, T.N, [&](int j) { return out_boards + (g0 + j) * T.N; },
                [&](int j) { return (const int8_t*)node_board(T, g0 + j, s_root[j]); });
}

__global__ void __launch_bounds__(SEARCH_BLOCK) k_search_ucb1(int64_t n, const int64_t* reward_sum, const int32_t* visits,
                                                              const int32_t* parent_visits, const double* c,
                                                              const double* log_tab, double* out) {
    const int64_t i = lane_game();
    if (i < n) out[i] = search_ucb1(reward_sum[i], visits[i], log_tab[parent_visits[i]], c[i]);
}

}  // namespace

hipError_t launch_search_init(hipStream_t st, const STree& T, const int8_t* boards, const int32_t* n_actions,
                              const int32_t* rewards, const uint32_t* legal) {
    hipLaunchKernelGGL(k_search_init, dim3(grid_for(T.n)), dim3(SEARCH_BLOCK), 0, st, T, boards, n_actions, rewards, legal);
    return hipGetLastError();
}

hipError_t launch_search_select(hipStream_t st, const SearchRound& r) {
    hipLaunchKernelGGL(k_search_select, dim3(grid_for(r.T.n)), dim3(SEARCH_BLOCK), 0, st, r);
    return hipGetLastError();
}

hipError_t launch_search_attach(hipStream_t st, const SearchRound& r) {
    hipLaunchKernelGGL(k_search_attach, dim3(grid_for(r.T.n)), dim3(SEARCH_BLOCK), 0, st, r);
    return hipGetLastError();
}

hipError_t launch_search_backup(hipStream_t st, const SearchRound& r) {
    hipLaunchKernelGGL(k_search_backup, dim3(grid_flat(r.T.n)), dim3(SEARCH_BLOCK), 0, st, r);
    return hipGetLastError();
}

hipError_t launch_search_finish(hipStream_t st, const STree& T, const SResult& r, int32_t* keep_best, uint64_t* stats) {
    hipLaunchKernelGGL(k_search_finish, dim3(grid_flat(T.n)), dim3(SEARCH_BLOCK), 0, st, T, r, keep_best, stats);
    return hipGetLastError();
}

hipError_t launch_search_advance(hipStream_t st, const STree& T, const int32_t* actions, int8_t* out_boards,
                                 int32_t* out_rewards, int32_t* out_n_actions, uint32_t* out_flags) {
    hipLaunchKernelGGL(k_search_advance, dim3(grid_for(T.n)), dim3(SEARCH_BLOCK), 0, st, T, actions, out_boards,
                       out_rewards, out_n_actions, out_flags);
    return hipGetLastError();
}

hipError_t launch_search_ucb1(hipStream_t st, int64_t n, const int64_t* reward_sum, const int32_t* visits,
                              const int32_t* parent_visits, const double* c, const double* log_tab, double* out) {
    hipLaunchKernelGGL(k_search_ucb1, dim3(grid_flat(n)), dim3(SEARCH_BLOCK), 0, st, n, reward_sum, visits, parent_visits,
                       c, log_tab, out);
    return hipGetLastError();
}

}  // namespace m3s
