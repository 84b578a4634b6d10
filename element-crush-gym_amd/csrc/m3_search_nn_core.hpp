// m3_search_nn_core.hpp -- the network-guided search tree of mctslib (nn/mcts.py: NNNode,
// NeuralNetworkMCTS, over abc/mcts.py:33-128) on the node pool of m3_search_core.hpp, without the
// kernels around it and without the network: prior-weighted selection, one expansion per game per
// round, and an evaluator's value backed up instead of a playout. Everything is M3_HD: the kernels
// of m3_search_nn.hip (one lane per game) and the host harness (tests/search_nn_host) run this code.
//
// The evaluator maps a board to (value: f32, logits: f32[A]) and lives outside: a round stops at an
// evaluation batch (one board per game and a `need` byte), and what comes back is handed to
// nn_commit. Every node that is created and is not terminal is evaluated once (NNNode.__init__ and
// rollout() call the model on the same state: one call serves both). The logits stay raw, as the
// reference keeps them (nn/mcts.py:20-21): no softmax, negative values allowed, entries of illegal
// actions never read.
//
// Node pool: as m3_search_core.hpp (game-major, children in expansion order), with
//   - a 16-byte hot record {f32 sum, i32 visits, i32 next, f32 prior}: one load per child of a score,
//   - the link record of the UCB1 tree (SNodeLink),
//   - the untried set as AW words, the board as N bytes,
//   - the node's row of A logits: a child's prior is its parent's logit at the child's action
//     (nn/mcts.py:39), so a row is read once per expansion of that node.
//   bytes per node = 16 + 32 + 4 * AW + N + 4 * A   (9x9x6: 725; 16x16x8: 2,288)
//
// Score of a child (NNNode.ucb1 = BaseNode.ucb1(c * policy)), in float32 with every operation
// rounded on its own -- nn_score is compiled under `#pragma clang fp contract(off)` for the device and
// the host (see m3_search_core.hpp on why not the __f*_rn intrinsics):
//     mean  = sum / (f32)visits                                  (f32 division, correctly rounded)
//     e     = (f32) sqrt( log_tab[parent.visits] / (double)(1 + visits) )   (double, rounded to f32 once)
//     w     = (f32)c * prior
//     score = mean + w * e
//   visits == 0 gives +inf and nothing else is evaluated; c == 0 (the greedy line) still evaluates the
//   product. First maximum in expansion order, strict `>`.
//   The trees are pinned to the reference's own tree code. It is executed with numpy standing in for
//   `jax.numpy` and with integer rewards handed over as Python ints, so that numpy promotes as JAX does
//   with x64 off. JAX itself has still not been run. (tests/golden/gen_golden_search_nn.py)
//
// Backup: ret = the evaluator's value for a new non-terminal child, (f32)state_reward for a terminal
// leaf or a terminal new child (nn/mcts.py:52-56) -- not reward plus value; sum += ret in f32 from
// leaf to root. (The reference keeps an all-integer sum as a Python int until a float arrives; here
// the sum is always f32, exact while visits * reward < 2^24.)
//
// A round is nn_select -> the step -> nn_attach (the child's records exist, unlinked; the batch is
// written) -> the evaluator -> nn_commit (finiteness, link the child, backup). The child is linked
// only once its evaluation is in: NNNode.__init__ calls the model before expand() inserts the child,
// so a game that freezes on a bad evaluation keeps its tree as it stood.
#pragma once

#include "m3_search_core.hpp"

namespace m3s {

constexpr uint32_t SF_BAD_EVAL = 0x400u;  // M3_FLAG_BAD_EVAL: a needed value or legal logit is not finite

struct NNodeHot {
    float sum;       // Node.reward
    int32_t visits;  // Node.visits
    int32_t next;    // next sibling in expansion order, -1 at the end
    float prior;     // NNNode.policy: the parent's logit at this node's action (the root: 1.0)
};
static_assert(sizeof(NNodeHot) == 16, "the hot record is 16 bytes");

struct NTree {
    int64_t n;    // games
    int32_t cap;  // node slots per game
    int32_t N, AW, A;
    NNodeHot* hot;      // [n][cap]
    SNodeLink* link;    // [n][cap]
    uint32_t* untried;  // [n][cap][AW]
    int8_t* boards;     // [n][cap][N]
    float* logits;      // [n][cap][A]
    int32_t* root;      // [n]
    int32_t* used;      // [n] slots taken
    int32_t* leaf;      // [n] the node this round selected
    int32_t* expanded;  // [n] 1: this round expands `leaf` with action[g]
    int32_t* action;    // [n]
    int32_t* pending;   // [n] the child nn_attach made this round, not linked yet; -1 without
    uint32_t* gflags;   // [n] non-zero: the game is frozen
    const double* log_tab;  // [cap + 1]
};

M3_HD int64_t nn_base(const NTree& T, int64_t g) { return g * (int64_t)T.cap; }
M3_HD int8_t* nn_board(const NTree& T, int64_t g, int32_t k) { return T.boards + (nn_base(T, g) + k) * T.N; }
M3_HD float* nn_row(const NTree& T, int64_t g, int32_t k) { return T.logits + (nn_base(T, g) + k) * T.A; }

M3_HD bool nn_finite(float x) {
    uint32_t u;
    __builtin_memcpy(&u, &x, 4);
    return (u & 0x7f800000u) != 0x7f800000u;
}

// log_pv: log_tab[parent.visits]
M3_HD float nn_score(float sum, int32_t visits, double log_pv, float c, float prior) {
#pragma clang fp contract(off)
    if (visits == 0) return INFINITY;
    const float mean = sum / (float)visits;
    const double q = log_pv / (double)(1 + visits);
    const float e = (float)__builtin_sqrt(q);
    const float w = c * prior;
    const float x = w * e;
    return mean + x;
}

// best_child(c): the first maximum of the score over the children in expansion order; -1 without children
M3_HD int32_t nn_best_child(const NTree& T, int64_t base, int32_t node, float c) {
    const int32_t pv = T.hot[base + node].visits;
    const double lp = pv >= 1 ? T.log_tab[pv] : 0.0;  // (children of an unvisited node are unvisited: +inf)
    int32_t best = -1, ch = T.link[base + node].first;
    float bv = 0.0f;
    if (ch < 0) return -1;
    NNodeHot h = T.hot[base + ch];
    for (;;) {
        // the next sibling's record is requested before this child's score is evaluated: the walk is a
        // chain of dependent loads, and the divisions and the square root run in its shadow
        const int32_t nx = h.next;
        NNodeHot hn = h;
        if (nx >= 0) hn = T.hot[base + nx];
        const float v = nn_score(h.sum, h.visits, lp, c, h.prior);
        if (best < 0 || v > bv) {
            best = ch;
            bv = v;
        }
        if (nx < 0) break;
        ch = nx;
        h = hn;
    }
    return best;
}

// the highest untried action of a node, removed from the set (untried_actions.pop()); -1 if none
M3_HD int32_t nn_pop_untried(const NTree& T, int64_t base, int32_t node) {
    uint32_t* u = T.untried + (base + node) * T.AW;
    for (int w = T.AW - 1; w >= 0; --w)
        if (u[w]) {
            const int b = 31 - __builtin_clz(u[w]);
            u[w] &= ~(1u << b);
            return w * 32 + b;
        }
    return -1;
}

// The root, unevaluated: returns 1 if the root's row is needed (the root is not terminal).
M3_HD int32_t nn_init_root(const NTree& T, int64_t g, int32_t n_actions, int32_t reward, const uint32_t* legal) {
    const int64_t base = nn_base(T, g);
    T.hot[base] = NNodeHot{0.0f, 0, -1, 1.0f};
    T.link[base] = SNodeLink{-1, -1, -1, -1, n_actions, reward, 0u, 0};
    for (int w = 0; w < T.AW; ++w) T.untried[base * T.AW + w] = legal[w];
    T.root[g] = 0;
    T.used[g] = 1;
    T.gflags[g] = 0u;
    T.leaf[g] = 0;
    T.expanded[g] = 0;
    T.action[g] = -1;
    T.pending[g] = n_actions >= 1 ? 0 : -1;  // the root's evaluation is the first batch
    return n_actions >= 1;
}

// Selection (abc/mcts.py:94-101), as search_select: returns the n_actions of the row for the step.
M3_HD int32_t nn_select(const NTree& T, int64_t g) {
    const int64_t base = nn_base(T, g);
    int32_t node = T.root[g];
    T.expanded[g] = 0;
    T.action[g] = -1;
    T.pending[g] = -1;
    T.leaf[g] = node;
    if (T.gflags[g]) return 0;
    for (;;) {
        const int32_t na = T.link[base + node].n_actions;
        if (na < 1) break;  // terminal: its state reward is backed up again
        const int32_t a = nn_pop_untried(T, base, node);
        if (a >= 0) {
            T.leaf[g] = node;
            T.expanded[g] = 1;
            T.action[g] = a;
            return na;
        }
        const int32_t ch = nn_best_child(T, base, node, (float)na);
        if (ch < 0) {  // not terminal, no legal action: the reference's max() of no children raises
            T.gflags[g] |= SF_NO_LEGAL;
            break;
        }
        node = ch;
    }
    T.leaf[g] = node;
    return 0;
}

// After the step: the child's records (NNNode.__init__ up to the model call), not linked to its parent
// yet. Returns the game's `need` byte: 1 if the child exists and is not terminal.
M3_HD int32_t nn_attach(const NTree& T, int64_t g, int32_t step_reward, uint32_t step_flags, const uint32_t* legal) {
    const int64_t base = nn_base(T, g);
    if (T.gflags[g] || !T.expanded[g]) return 0;
    if (step_flags & SF_STEP_FREEZE) {
        T.gflags[g] |= step_flags & SF_STEP_FREEZE;
        return 0;
    }
    const int32_t leaf = T.leaf[g], a = T.action[g];
    const int32_t child = T.used[g]++;  // (the host checked the capacity before the round)
    const SNodeLink p = T.link[base + leaf];
    T.link[base + child] = SNodeLink{leaf, -1, -1, a, p.n_actions - 1, p.state_reward + step_reward, step_flags, 0};
    T.hot[base + child] = NNodeHot{0.0f, 0, -1, T.logits[(base + leaf) * T.A + a]};
    for (int w = 0; w < T.AW; ++w) T.untried[(base + child) * T.AW + w] = legal[w];
    T.pending[g] = child;
    return p.n_actions - 1 >= 1;
}

// lanes `lane`, lane + nl, ... store one evaluated row into a node and report whether a logit of a
// legal action (bit set in `legal`) among theirs is not finite
M3_HD bool nn_store_row(float* dst, const float* src, const uint32_t* legal, int A, int lane, int nl) {
    bool bad = false;
    for (int i = lane; i < A; i += nl) {
        const float x = src[i];
        dst[i] = x;
        bad |= ((legal[i >> 5] >> (i & 31)) & 1u) && !nn_finite(x);
    }
    return bad;
}

// What the evaluator's answer does to the game: `bad` = the game's needed value or one of its legal
// logits is not finite (the caller looked, nn_store_row). backup = false: the two batches of the
// construction (abc/mcts.py:82), which back nothing up.
M3_HD void nn_commit(const NTree& T, int64_t g, float value, bool bad, bool backup) {
    const int64_t base = nn_base(T, g);
    if (T.gflags[g]) return;
    const int32_t child = T.pending[g];
    int32_t node = T.leaf[g];
    float ret;
    if (child >= 0) {
        const bool need = T.link[base + child].n_actions >= 1;
        if (need && bad) {
            T.gflags[g] |= SF_BAD_EVAL;
            return;
        }
        T.pending[g] = -1;
        if (child == T.root[g]) return;  // the root's own evaluation: nothing to link
        const int32_t last = T.link[base + node].last;
        if (last < 0) T.link[base + node].first = child;
        else T.hot[base + last].next = child;
        T.link[base + node].last = child;
        ret = need ? value : (float)T.link[base + child].state_reward;
        node = child;
    } else {
        ret = (float)T.link[base + node].state_reward;
    }
    if (!backup) return;
    while (node >= 0) {
        T.hot[base + node].visits += 1;
        T.hot[base + node].sum += ret;
        node = T.link[base + node].parent;
    }
}

// The result of a search (abc/mcts.py:113-120), as search_finish with the f32 sums and the priors.
struct NResult {
    int32_t *best_action, *value, *root_visits, *n_children;  // [n]
    int32_t *child_action, *child_visits;                    // [n][A]
    float *child_value_sum, *child_prior;                    // [n][A]
    uint32_t* flags;                                         // [n]
};

M3_HD int32_t nn_finish(const NTree& T, int64_t g, const NResult& r) {
    const int64_t base = nn_base(T, g);
    const int32_t root = T.root[g];
    int32_t best = -1, bestv = 0, k = 0;
    for (int32_t ch = T.link[base + root].first; ch >= 0; ch = T.hot[base + ch].next, ++k) {
        const NNodeHot h = T.hot[base + ch];
        if (best < 0 || h.visits > bestv) {
            best = ch;
            bestv = h.visits;
        }
        if (k < T.A) {  // (a node has at most A children: one per action)
            if (r.child_action) r.child_action[g * T.A + k] = T.link[base + ch].action;
            if (r.child_visits) r.child_visits[g * T.A + k] = h.visits;
            if (r.child_value_sum) r.child_value_sum[g * T.A + k] = h.sum;
            if (r.child_prior) r.child_prior[g * T.A + k] = h.prior;
        }
    }
    const int32_t best_action = best >= 0 ? T.link[base + best].action : -1;
    if (r.n_children) r.n_children[g] = k;
    if (r.root_visits) r.root_visits[g] = T.hot[base + root].visits;
    if (r.best_action) r.best_action[g] = best_action;
    int32_t node = root;
    if (!T.gflags[g])
        for (;;) {
            if (T.link[base + node].n_actions < 1) break;
            const uint32_t* u = T.untried + (base + node) * T.AW;
            uint32_t any = 0u;
            for (int w = 0; w < T.AW; ++w) any |= u[w];
            if (any) break;
            const int32_t ch = nn_best_child(T, base, node, 0.0f);
            if (ch < 0) {
                T.gflags[g] |= SF_NO_LEGAL;
                break;
            }
            node = ch;
        }
    if (r.value) r.value[g] = T.link[base + node].state_reward;
    if (r.flags) r.flags[g] = T.gflags[g];
    return best_action;
}

// Re-root at the child reached by `action`, as search_advance.
M3_HD int32_t nn_advance(const NTree& T, int64_t g, int32_t action) {
    const int64_t base = nn_base(T, g);
    const int32_t root = T.root[g];
    if (T.gflags[g]) return root;
    for (int32_t ch = T.link[base + root].first; ch >= 0; ch = T.hot[base + ch].next)
        if (T.link[base + ch].action == action) {
            T.link[base + ch].parent = -1;
            T.root[g] = ch;
            return ch;
        }
    return -1;
}

// The built-in baseline evaluator: a linear map of the one-hot board. W is f32 [N][CH][A + 1], CH the
// reference's one-hot width (elementCrush.py:66, :92); a cell whose value is >= CH contributes
// nothing, like one_hot out of range.
//   out[j] = (((W[0][x0][j] + W[1][x1][j]) + W[2][x2][j]) + ...)  over the cells in ascending order,
// float32, no bias; logits = out[0 .. A), value = out[A]. Lanes `lane`, lane + nl, ... take the j.
M3_HD int nn_onehot_width(int types) {
    int b = 0;
    while ((1 << b) < types) ++b;
    return 1 << (b + 2);
}

M3_HD void nn_linear_row(const int8_t* board, const float* W, int N, int CH, int A, float* value, float* logits, int lane,
                         int nl) {
#pragma clang fp contract(off)
    const int J = A + 1;
    for (int j = lane; j < J; j += nl) {
        float acc = 0.0f;
        bool have = false;
        for (int i = 0; i < N; ++i) {
            const int x = board[i];
            if (x < 0 || x >= CH) continue;
            const float w = W[((int64_t)i * CH + x) * J + j];
            acc = have ? acc + w : w;
            have = true;
        }
        if (j < A) logits[j] = acc;
        else *value = acc;
    }
}

}  // namespace m3s
