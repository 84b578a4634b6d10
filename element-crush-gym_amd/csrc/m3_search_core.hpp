// m3_search_core.hpp -- the UCB1 search tree of mctslib (abc/mcts.py:33-128, standard/mcts.py:22-43)
// over a fixed node pool, without the kernels around it: selection, the bookkeeping of an expansion,
// backup, the result of a search and the re-rooting, one game at a time. Everything is M3_HD, so the
// kernels of m3_search.hip (one lane per game) and the host harness (tests/search_host) run the same
// code. The rules of the game are not here: a board is N opaque bytes, the step (launch_apply) and the
// playout (launch_rollouts) run between these functions and hand their results in.
//
// Node pool. Every game owns `cap` node slots; node k of game g is element g * cap + k of each array
// ("game-major" structure of arrays). Selection and backup are pointer chases of one lane per game:
// no layout makes them coalesce, so the fields they read per child sit together in one 16-byte record
// (SNodeHot: reward sum, visits, next sibling -- one load per child of best_child), the rest of a
// node in a 32-byte record (SNodeLink), the untried set as AW words and the board as N contiguous
// bytes, which the kernels copy with the lanes across a board's bytes. A game's early nodes (the
// root's neighbourhood, read by every simulation) are neighbours in memory.
//   bytes per node = 16 + 32 + 4 * AW + N  (9x9x6: 149; 16x16x8: 368)
// Children are a singly linked list in expansion order (first / last in the parent, next in the
// child): every `max()` of the reference breaks ties by that order.
//
// UCB1, bit for bit as CPython evaluates Node.ucb1 (standard/mcts.py:33-37):
//     ucb1 = reward_sum / visits + c * sqrt(log(parent.visits) / (1 + visits))
//   - doubles, every operation rounded on its own (IEEE round-to-nearest): search_ucb1 is compiled
//     under `#pragma clang fp contract(off)`, for the device and for the host, and uses the plain
//     operators and __builtin_sqrt (division and square root of doubles are correctly rounded on
//     gfx950). Not the __dmul_rn / __dadd_rn intrinsics: HIP's headers define them as the plain
//     operators inside functions compiled with hipcc's default -ffp-contract=fast, so they carry the
//     permission to fuse with them. A fused multiply-add rounds c * sqrt(..) + mean once and
//     reorders near-ties.
//   - visits == 0 gives +inf and nothing else is evaluated; c == 0 still evaluates the product
//     (0 * finite = 0).
//   - the maximum is taken with a strict `>` over the children in expansion order: the first
//     maximum wins, like max().
//   - log is never computed on the device: log_tab[v] = std::log((double)v) is filled on the host
//     (search_log_table; CPython's math.log calls the same libm) for v = 1 .. cap and uploaded.
//     Every visit count is below cap: the host refuses a run that could pass it (search_run_fits).
//   - reward_sum (int64) and visits are exact integers below 2^53, so (double)reward_sum /
//     (double)visits is Python's int / int.
#pragma once

#include <math.h>
#include <stdint.h>

#ifndef M3_HD
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define M3_HD __host__ __device__ __forceinline__
#else
#define M3_HD inline
#endif
#endif

namespace m3s {

// (the values of include/m3.h's M3_FLAG_*)
constexpr uint32_t SF_BAD_ACTION = 0x02u, SF_SHUFFLE_CAP = 0x04u, SF_NO_LEGAL = 0x08u, SF_CASCADE_CAP = 0x100u;
// what freezes a game: the reference raises (max() of no children, np.random.choice([])) or never returns
constexpr uint32_t SF_FREEZE = SF_SHUFFLE_CAP | SF_NO_LEGAL | SF_CASCADE_CAP;
// what freezes a game in an expansion's step: the caps only. The apply launch also samples the action
// after the step and sets NO_LEGAL when the board it left has none (m3_apply_actions' next_action);
// the search samples nothing there -- the reference is still shuffling -- so that bit is not the game's.
constexpr uint32_t SF_STEP_FREEZE = SF_SHUFFLE_CAP | SF_CASCADE_CAP;

struct SNodeHot {
    int64_t reward_sum;  // Node.reward
    int32_t visits;      // Node.visits
    int32_t next;        // next sibling in expansion order, -1 at the end
};
struct SNodeLink {
    int32_t parent;        // -1: the root (backup stops here)
    int32_t first, last;   // children in expansion order, -1 without
    int32_t action;        // the action that led here
    int32_t n_actions;     // state.n_actions (< 1: terminal)
    int32_t state_reward;  // state.reward
    uint32_t flags;        // M3_FLAG_* of the step that made the node
    int32_t pad;
};
static_assert(sizeof(SNodeHot) == 16 && sizeof(SNodeLink) == 32, "node records are 16 and 32 bytes");

struct STree {
    int64_t n;      // games
    int32_t cap;    // node slots per game
    int32_t N, AW, A;
    SNodeHot* hot;        // [n][cap]
    SNodeLink* link;      // [n][cap]
    uint32_t* untried;    // [n][cap][AW]
    int8_t* boards;       // [n][cap][N]
    int32_t* root;        // [n]
    int32_t* used;        // [n] slots taken
    int32_t* leaf;        // [n] the node this round selected / attached
    int32_t* expanded;    // [n] 1: this round expands `leaf` with action[g]
    int32_t* action;      // [n]
    uint32_t* gflags;     // [n] non-zero: the game is frozen (SF_FREEZE bits)
    const double* log_tab;  // [cap + 1]
};

M3_HD int64_t node_base(const STree& T, int64_t g) { return g * (int64_t)T.cap; }
M3_HD int8_t* node_board(const STree& T, int64_t g, int32_t k) { return T.boards + (node_base(T, g) + k) * T.N; }

// `used` counts the nodes below the root that were ever attached (an upper bound kept on the host: one
// per simulation, one for the constructor's expansion). A run of `simulations` rounds fits if the
// root, those nodes and one new node per round have a slot; no device-side overflow path exists.
inline bool search_run_fits(int64_t used, int64_t simulations, int64_t cap) { return used + simulations + 1 <= cap; }

// log_tab[0] = 0 (never read), log_tab[v] = log(v)
inline void search_log_table(int32_t n, double* out) {
    out[0] = 0.0;
    for (int32_t v = 1; v <= n; ++v) out[v] = ::log((double)v);
}

// Node.ucb1 with log(parent.visits) looked up by the caller (see the head of this file)
M3_HD double search_ucb1(int64_t reward_sum, int32_t visits, double log_pv, double c) {
#pragma clang fp contract(off)
    if (visits == 0) return (double)INFINITY;
    const double mean = (double)reward_sum / (double)visits;
    const double q = log_pv / (double)(1 + visits);
    const double e = __builtin_sqrt(q);
    const double x = c * e;
    return mean + x;
}

// Node.best_child(c): the first maximum of ucb1 over the children in expansion order; -1 without children
M3_HD int32_t search_best_child(const STree& T, int64_t base, int32_t node, double c) {
    const int32_t pv = T.hot[base + node].visits;
    const double lp = pv >= 1 ? T.log_tab[pv] : 0.0;  // (children of an unvisited node are unvisited: +inf)
    int32_t best = -1, ch = T.link[base + node].first;
    double bv = 0.0;
    if (ch < 0) return -1;
    SNodeHot h = T.hot[base + ch];
    for (;;) {
        // the next sibling's record is requested before this child's UCB1 is evaluated: the walk is a
        // chain of dependent loads, and the divisions and the square root run in its shadow
        const int32_t nx = h.next;
        SNodeHot hn = h;
        if (nx >= 0) hn = T.hot[base + nx];
        const double v = search_ucb1(h.reward_sum, h.visits, lp, c);
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
M3_HD int32_t search_pop_untried(const STree& T, int64_t base, int32_t node) {
    uint32_t* u = T.untried + (base + node) * T.AW;
    for (int w = T.AW - 1; w >= 0; --w)
        if (u[w]) {
            const int b = 31 - __builtin_clz(u[w]);
            u[w] &= ~(1u << b);
            return w * 32 + b;
        }
    return -1;
}

M3_HD void search_init_root(const STree& T, int64_t g, int32_t n_actions, int32_t reward, const uint32_t* legal) {
    const int64_t base = node_base(T, g);
    T.hot[base] = SNodeHot{0, 0, -1};
    T.link[base] = SNodeLink{-1, -1, -1, -1, n_actions, reward, 0u, 0};
    for (int w = 0; w < T.AW; ++w) T.untried[base * T.AW + w] = legal[w];
    T.root[g] = 0;
    T.used[g] = 1;
    T.gflags[g] = 0u;
    T.leaf[g] = 0;
    T.expanded[g] = 0;
    T.action[g] = -1;
}

// Selection (abc/mcts.py:94-101): descend while the node is not terminal and fully expanded; a
// non-terminal node with untried actions expands its highest one. Sets leaf / expanded / action of
// the game and returns the n_actions of the row for the apply launch: the leaf's when the game
// expands, 0 (a terminal row, its output ignored) otherwise.
M3_HD int32_t search_select(const STree& T, int64_t g) {
    const int64_t base = node_base(T, g);
    int32_t node = T.root[g];
    T.expanded[g] = 0;
    T.action[g] = -1;
    T.leaf[g] = node;
    if (T.gflags[g]) return 0;
    for (;;) {
        const int32_t na = T.link[base + node].n_actions;
        if (na < 1) break;  // terminal: rolled out again as it is
        const int32_t a = search_pop_untried(T, base, node);
        if (a >= 0) {
            T.leaf[g] = node;
            T.expanded[g] = 1;
            T.action[g] = a;
            return na;
        }
        const int32_t ch = search_best_child(T, base, node, (double)na);
        if (ch < 0) {  // not terminal, no legal action: the reference's max() of no children raises
            T.gflags[g] |= SF_NO_LEGAL;
            break;
        }
        node = ch;
    }
    T.leaf[g] = node;
    return 0;
}

// After the apply launch: append the child to the leaf (Node.expand). leaf[g] becomes the node to roll
// out; returns its n_actions for the rollout row (0 for a frozen game: a terminal row plays nothing).
M3_HD int32_t search_attach(const STree& T, int64_t g, int32_t step_reward, uint32_t step_flags, const uint32_t* legal) {
    const int64_t base = node_base(T, g);
    if (T.gflags[g]) return 0;
    const int32_t leaf = T.leaf[g];
    if (!T.expanded[g]) return T.link[base + leaf].n_actions;
    if (step_flags & SF_STEP_FREEZE) {
        T.gflags[g] |= step_flags & SF_STEP_FREEZE;
        return 0;
    }
    const int32_t child = T.used[g]++;  // (the host checked the capacity before the run)
    const SNodeLink p = T.link[base + leaf];
    T.link[base + child] = SNodeLink{leaf, -1, -1, T.action[g], p.n_actions - 1, p.state_reward + step_reward, step_flags, 0};
    T.hot[base + child] = SNodeHot{0, 0, -1};
    for (int w = 0; w < T.AW; ++w) T.untried[(base + child) * T.AW + w] = legal[w];
    if (p.last < 0) T.link[base + leaf].first = child;
    else T.hot[base + p.last].next = child;
    T.link[base + leaf].last = child;
    T.leaf[g] = child;
    return p.n_actions - 1;
}

// Backup (abc/mcts.py:106-109) of ret = leaf.state.reward + the rollout's gain, leaf to root.
M3_HD void search_backup(const STree& T, int64_t g, int32_t gain, uint32_t rollout_flags) {
    if (T.gflags[g]) return;
    if (rollout_flags & SF_FREEZE) {
        T.gflags[g] |= rollout_flags & SF_FREEZE;
        return;
    }
    const int64_t base = node_base(T, g);
    int32_t node = T.leaf[g];
    const int64_t ret = (int64_t)T.link[base + node].state_reward + gain;
    while (node >= 0) {
        T.hot[base + node].visits += 1;
        T.hot[base + node].reward_sum += ret;
        node = T.link[base + node].parent;
    }
}

// The result of a search (abc/mcts.py:113-120): the first most-visited root child, the reward of the
// state at the end of the greedy line (best_child(0) while not terminal and fully expanded), and the
// root's children (action, visits, reward sum) in expansion order. best_action -1: no child. Every
// output is nullable; returns best_action.
struct SResult {
    int32_t *best_action, *value, *root_visits, *n_children;  // [n]
    int32_t *child_action, *child_visits;                    // [n][A]
    int64_t* child_reward;                                   // [n][A]
    uint32_t* flags;                                         // [n]
};

M3_HD int32_t search_finish(const STree& T, int64_t g, const SResult& r) {
    const int64_t base = node_base(T, g);
    const int32_t root = T.root[g];
    int32_t best = -1, bestv = 0, k = 0;
    for (int32_t ch = T.link[base + root].first; ch >= 0; ch = T.hot[base + ch].next, ++k) {
        const int32_t v = T.hot[base + ch].visits;
        if (best < 0 || v > bestv) {
            best = ch;
            bestv = v;
        }
        if (k < T.A) {  // (a node has at most A children: one per action)
            if (r.child_action) r.child_action[g * T.A + k] = T.link[base + ch].action;
            if (r.child_visits) r.child_visits[g * T.A + k] = v;
            if (r.child_reward) r.child_reward[g * T.A + k] = T.hot[base + ch].reward_sum;
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
            const int32_t ch = search_best_child(T, base, node, 0.0);
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

// Re-root at the child reached by `action` (abc/mcts.py:123-124): the subtree and its statistics stay,
// the new root has no parent. Returns the new root; -1 (the root stays) if no child of the root was
// reached by that action. A frozen game stays as it is and returns its root.
M3_HD int32_t search_advance(const STree& T, int64_t g, int32_t action) {
    const int64_t base = node_base(T, g);
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

// lanes `lane`, lane + nl, ... copy the bytes of one board
M3_HD void search_copy_board(int8_t* dst, const int8_t* src, int N, int lane, int nl) {
    for (int i = lane; i < N; i += nl) dst[i] = src[i];
}

}  // namespace m3s
