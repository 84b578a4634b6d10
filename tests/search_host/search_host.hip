// search_host.hip -- TEST INFRASTRUCTURE ONLY: the search-tree core (csrc/m3_search_core.hpp) built for
// the host. The node pool lives in host memory, every kernel of m3_search.hip is restated as a serial
// loop over the games calling the same M3_HD functions, and the step and the playout between them
// are the caller's (tests/test_search_cpu.py hands in the C oracle's). Driven through ctypes
// (search_host.py) and, under ASan + UBSan, by asan_main.hip.
#include "../../element-crush-gym_amd/csrc/m3_search_core.hpp"

#include <string.h>

#include <vector>

using namespace m3s;

struct SH {
    STree T{};
    std::vector<SNodeHot> hot;
    std::vector<SNodeLink> link;
    std::vector<uint32_t> untried, gflags;
    std::vector<int8_t> boards, row_boards;
    std::vector<int32_t> root, used, leaf, expanded, action;
    std::vector<double> log_tab;
    int64_t used_bound = 0;  // as m3_search keeps it (m3_api.hip)
    bool ready = false;
};

extern "C" {

SH* sh_create(long n, int cap, int N, int AW, int A) {
    SH* h = new SH;
    const size_t nodes = (size_t)n * cap;
    h->hot.resize(nodes);
    h->link.resize(nodes);
    h->untried.resize(nodes * AW);
    h->boards.resize(nodes * N);
    h->row_boards.resize((size_t)n * N);
    for (auto* v : {&h->root, &h->used, &h->leaf, &h->expanded, &h->action}) v->resize(n);
    h->gflags.resize(n);
    h->log_tab.resize((size_t)cap + 1);
    search_log_table(cap, h->log_tab.data());
    h->T = STree{n, cap, N, AW, A, h->hot.data(), h->link.data(), h->untried.data(), h->boards.data(),
                 h->root.data(), h->used.data(), h->leaf.data(), h->expanded.data(), h->action.data(),
                 h->gflags.data(), h->log_tab.data()};
    return h;
}

void sh_destroy(SH* h) { delete h; }

// k_search_init (the constructor's expansion is the caller's next select / attach)
void sh_set_roots(SH* h, const int8_t* boards, const int32_t* n_actions, const int32_t* rewards, const uint32_t* legal) {
    const STree& T = h->T;
    for (int64_t g = 0; g < T.n; ++g) {
        search_init_root(T, g, n_actions[g], rewards[g], legal + g * T.AW);
        search_copy_board(node_board(T, g, 0), boards + g * T.N, T.N, 0, 1);
    }
    h->used_bound = 1;
    h->ready = true;
}

// m3_search_run's checks: 0 and the rounds are accounted for, -6 before sh_set_roots, -7 if they do not fit
int sh_run_begin(SH* h, int simulations) {
    if (!h->ready) return -6;
    if (!search_run_fits(h->used_bound, simulations, h->T.cap)) return -7;
    h->used_bound += simulations;
    return 0;
}

// k_search_select: the rows of the apply launch
void sh_select(SH* h, int8_t* row_boards, int32_t* row_na, int32_t* row_action) {
    const STree& T = h->T;
    for (int64_t g = 0; g < T.n; ++g) {
        row_na[g] = search_select(T, g);
        row_action[g] = T.action[g];
        search_copy_board(h->row_boards.data() + g * T.N, node_board(T, g, T.leaf[g]), T.N, 0, 1);
    }
    memcpy(row_boards, h->row_boards.data(), h->row_boards.size());
}

// k_search_attach: the apply launch's outputs in, the rows of the rollout launch out
void sh_attach(SH* h, const int8_t* out_boards, const int32_t* out_reward, const uint32_t* out_flags,
               const uint32_t* out_legal, int8_t* ro_boards, int32_t* ro_na) {
    const STree& T = h->T;
    for (int64_t g = 0; g < T.n; ++g) {
        const int32_t before = T.used[g];
        ro_na[g] = search_attach(T, g, out_reward[g], out_flags[g], out_legal + g * T.AW);
        const bool grew = T.used[g] != before;
        const int8_t* src = grew ? out_boards + g * T.N : h->row_boards.data() + g * T.N;
        search_copy_board(ro_boards + g * T.N, src, T.N, 0, 1);
        if (grew) search_copy_board(node_board(T, g, T.leaf[g]), src, T.N, 0, 1);
    }
}

void sh_backup(SH* h, const int32_t* gain, const uint32_t* flags) {
    for (int64_t g = 0; g < h->T.n; ++g) search_backup(h->T, g, gain[g], flags[g]);
}

void sh_finish(SH* h, int32_t* best_action, int32_t* value, int32_t* root_visits, int32_t* n_children,
               int32_t* child_action, int32_t* child_visits, int64_t* child_reward, uint32_t* flags) {
    const SResult r{best_action, value, root_visits, n_children, child_action, child_visits, child_reward, flags};
    for (int64_t g = 0; g < h->T.n; ++g) search_finish(h->T, g, r);
}

// k_search_advance; returns the number of games whose action had no child
int sh_advance(SH* h, const int32_t* actions, int8_t* out_boards, int32_t* out_rewards, int32_t* out_n_actions) {
    const STree& T = h->T;
    int bad = 0;
    for (int64_t g = 0; g < T.n; ++g) {
        int32_t root = search_advance(T, g, actions[g]);
        if (root < 0) {
            ++bad;
            root = T.root[g];
        }
        const SNodeLink l = T.link[node_base(T, g) + root];
        out_rewards[g] = l.state_reward;
        out_n_actions[g] = l.n_actions;
        search_copy_board(out_boards + g * T.N, node_board(T, g, root), T.N, 0, 1);
    }
    return bad;
}

int sh_nodes_used(SH* h, long g) { return h->T.used[g]; }

void sh_log_table(int n, double* out) {
    std::vector<double> tab((size_t)n + 1);
    search_log_table(n, tab.data());
    for (int v = 1; v <= n; ++v) out[v - 1] = tab[v];
}

double sh_ucb1(long long reward_sum, int visits, int parent_visits, double c) {
    return search_ucb1(reward_sum, visits, ::log((double)parent_visits), c);
}

}  // extern "C"
