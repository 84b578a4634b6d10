// search_nn_host.hip -- TEST INFRASTRUCTURE ONLY: the network-guided tree core
// (csrc/m3_search_nn_core.hpp) built for the host. The node pool lives in host memory, every kernel of
// m3_search_nn.hip is restated as a serial loop over the games calling the same M3_HD functions, and the
// step and the evaluator between them are the caller's (tests/test_search_nn_cpu.py hands in the C
// oracle's step and a Python evaluator). Driven through ctypes (search_nn_host.py) and, under ASan +
// UBSan, by asan_main.hip.
#include "../../element-crush-gym_amd/csrc/m3_search_nn_core.hpp"

#include <string.h>

#include <vector>

using namespace m3s;

struct NH {
    NTree T{};
    std::vector<NNodeHot> hot;
    std::vector<SNodeLink> link;
    std::vector<uint32_t> untried, gflags;
    std::vector<int8_t> boards, row_boards;
    std::vector<float> logits;
    std::vector<int32_t> root, used, leaf, expanded, action, pending;
    std::vector<double> log_tab;
    int64_t used_bound = 0;  // as m3_search_nn keeps it (m3_api.hip)
    bool ready = false;
};

extern "C" {

NH* nh_create(long n, int cap, int N, int AW, int A) {
    NH* h = new NH;
    const size_t nodes = (size_t)n * cap;
    h->hot.resize(nodes);
    h->link.resize(nodes);
    h->untried.resize(nodes * AW);
    h->boards.resize(nodes * N);
    h->logits.resize(nodes * A);
    h->row_boards.resize((size_t)n * N);
    for (auto* v : {&h->root, &h->used, &h->leaf, &h->expanded, &h->action, &h->pending}) v->resize(n);
    h->gflags.resize(n);
    h->log_tab.resize((size_t)cap + 1);
    search_log_table(cap, h->log_tab.data());
    h->T = NTree{n, cap, N, AW, A, h->hot.data(), h->link.data(), h->untried.data(), h->boards.data(),
                 h->logits.data(), h->root.data(), h->used.data(), h->leaf.data(), h->expanded.data(),
                 h->action.data(), h->pending.data(), h->gflags.data(), h->log_tab.data()};
    return h;
}

void nh_destroy(NH* h) { delete h; }

// k_nn_init: the roots and their evaluation batch
void nh_set_roots(NH* h, const int8_t* boards, const int32_t* n_actions, const int32_t* rewards, const uint32_t* legal,
                  int8_t* ev_boards, uint8_t* ev_need) {
    const NTree& T = h->T;
    for (int64_t g = 0; g < T.n; ++g) {
        ev_need[g] = (uint8_t)nn_init_root(T, g, n_actions[g], rewards[g], legal + g * T.AW);
        search_copy_board(nn_board(T, g, 0), boards + g * T.N, T.N, 0, 1);
        search_copy_board(ev_boards + g * T.N, boards + g * T.N, T.N, 0, 1);
    }
    h->used_bound = 1;
    h->ready = true;
}

// m3_search_nn_batch's checks for a run of `simulations`: 0, -6 before nh_set_roots, -7 if they do not fit
int nh_fits(NH* h, int simulations) {
    if (!h->ready) return -6;
    return search_run_fits(h->used_bound, simulations, h->T.cap) ? 0 : -7;
}

// k_nn_select: the rows of the apply launch
void nh_select(NH* h, int8_t* row_boards, int32_t* row_na, int32_t* row_action) {
    const NTree& T = h->T;
    for (int64_t g = 0; g < T.n; ++g) {
        row_na[g] = nn_select(T, g);
        row_action[g] = T.action[g];
        search_copy_board(h->row_boards.data() + g * T.N, nn_board(T, g, T.leaf[g]), T.N, 0, 1);
    }
    memcpy(row_boards, h->row_boards.data(), h->row_boards.size());
}

// k_nn_attach: the apply launch's outputs in, the evaluation batch out
void nh_attach(NH* h, const int8_t* out_boards, const int32_t* out_reward, const uint32_t* out_flags,
               const uint32_t* out_legal, int8_t* ev_boards, uint8_t* ev_need) {
    const NTree& T = h->T;
    for (int64_t g = 0; g < T.n; ++g) {
        ev_need[g] = (uint8_t)nn_attach(T, g, out_reward[g], out_flags[g], out_legal + g * T.AW);
        const int32_t child = T.pending[g];
        const int8_t* src = child >= 0 ? out_boards + g * T.N : h->row_boards.data() + g * T.N;
        search_copy_board(ev_boards + g * T.N, src, T.N, 0, 1);
        if (child >= 0) search_copy_board(nn_board(T, g, child), src, T.N, 0, 1);
    }
}

// k_nn_commit
void nh_commit(NH* h, const float* values, const float* logits, int backup) {
    const NTree& T = h->T;
    for (int64_t g = 0; g < T.n; ++g) {
        const int32_t node = T.gflags[g] ? -1 : T.pending[g];
        const bool need = node >= 0 && T.link[nn_base(T, g) + node].n_actions >= 1;
        bool bad = need && !nn_finite(values[g]);
        if (need)
            bad |= nn_store_row(nn_row(T, g, node), logits + g * T.A, T.untried + (nn_base(T, g) + node) * T.AW, T.A, 0, 1);
        nn_commit(T, g, values[g], bad, backup != 0);
    }
    if (backup) h->used_bound += 1;
}

void nh_finish(NH* h, int32_t* best_action, int32_t* value, int32_t* root_visits, int32_t* n_children,
               int32_t* child_action, int32_t* child_visits, float* child_value_sum, float* child_prior, uint32_t* flags) {
    const NResult r{best_action, value, root_visits, n_children, child_action, child_visits, child_value_sum, child_prior,
                    flags};
    for (int64_t g = 0; g < h->T.n; ++g) nn_finish(h->T, g, r);
}

// k_nn_advance; returns the number of games whose action had no child
int nh_advance(NH* h, const int32_t* actions, int8_t* out_boards, int32_t* out_rewards, int32_t* out_n_actions) {
    const NTree& T = h->T;
    int bad = 0;
    for (int64_t g = 0; g < T.n; ++g) {
        int32_t root = nn_advance(T, g, actions[g]);
        if (root < 0) {
            ++bad;
            root = T.root[g];
        }
        const SNodeLink l = T.link[nn_base(T, g) + root];
        out_rewards[g] = l.state_reward;
        out_n_actions[g] = l.n_actions;
        search_copy_board(out_boards + g * T.N, nn_board(T, g, root), T.N, 0, 1);
    }
    return bad;
}

int nh_nodes_used(NH* h, long g) { return h->T.used[g]; }

float nh_score(float sum, int visits, int parent_visits, float c, float prior) {
    return nn_score(sum, visits, ::log((double)parent_visits), c, prior);
}

int nh_onehot_width(int types) { return nn_onehot_width(types); }

// k_nn_linear of one board
void nh_linear(const int8_t* board, const float* W, int N, int CH, int A, float* value, float* logits) {
    nn_linear_row(board, W, N, CH, A, value, logits, 0, 1);
}

}  // extern "C"
