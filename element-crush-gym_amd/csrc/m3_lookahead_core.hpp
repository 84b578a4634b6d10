// m3_lookahead_core.hpp -- the one-ply lookahead (BoardV2.greedy_action, boardv2.py:209-218) without
// the kernel around it: candidate enumeration, the packed (reward, action) key, one candidate's
// apply_action and the per-board fold with its hand-over to the exact pass. Everything is M3_HD, so
// k_lookahead (m3_lookahead.hpp) and the host harness (tests/lookahead_host) run the same code.
//
// A wave handles a group of boards. Their legal sets (action_bits) sit side by side as act[g][AW],
// pre[g] is the number of legal actions of the boards before g (pre[nb] the total), and candidate j
// of the group -- lane j % 64 of round j / 64 -- is action number j - pre[g] of board g.
#pragma once

#include "m3_rules.hpp"

namespace m3 {

// The board of candidate j: the g with pre[g] <= j < pre[g + 1] (boards without a legal action have
// an empty range and are never returned). j < pre[nb].
M3_HD int look_find_board(const uint32_t* pre, int nb, uint32_t j) {
    int lo = 0, hi = nb;  // pre[lo] <= j < pre[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (pre[mid] <= j) lo = mid;
        else hi = mid;
    }
    return lo;
}

// id of the k-th (0-based, ascending) set bit of act[0 .. aw); -1 if there are not that many
M3_HD int look_kth_bit(const uint32_t* act, int aw, uint32_t k) {
    for (int i = 0; i < aw; ++i) {
        const uint32_t c = (uint32_t)__builtin_popcount(act[i]);
        if (k < c) return i * 32 + select_bit(act[i], (int)k);
        k -= c;
    }
    return -1;
}

M3_HD uint32_t look_count(const uint32_t* act, int aw) {
    uint32_t c = 0;
    for (int i = 0; i < aw; ++i) c += (uint32_t)__builtin_popcount(act[i]);
    return c;
}

// The key orders candidates as the reference's loop does (legal ids ascending, the first strict
// maximum wins): a larger reward first, then the LOWER id. The reward's sign bit is flipped so that
// unsigned order is int32 order; the id is stored complemented. Every int32 reward and every id
// below 2^32 - 1 fit, and no candidate packs to 0, which stands for "no legal action".
constexpr uint64_t LOOK_KEY_NONE = 0ull;
M3_HD uint64_t look_key(int32_t reward, int action) {
    return ((uint64_t)((uint32_t)reward ^ 0x80000000u) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)action);
}
M3_HD int32_t look_key_reward(uint64_t key) {
    return key == LOOK_KEY_NONE ? -1 : (int32_t)((uint32_t)(key >> 32) ^ 0x80000000u);
}
M3_HD int32_t look_key_action(uint64_t key) {
    return key == LOOK_KEY_NONE ? -1 : (int32_t)(0xFFFFFFFFu - (uint32_t)key);
}
M3_HD bool look_key_better(uint64_t a, uint64_t b) { return a > b; }

// One candidate: the whole apply_action on a private copy of the board, the chain reseeded from
// (seed, mt[397]) as in every step. redo: the fast path gave up (more first-scan groups than the
// table holds, or the chain ran past its limit) and the reward is void.
struct LookCand {
    int32_t reward;
    uint32_t draws;  // raw draws of this apply (0 on a terminal board)
    uint32_t flags;  // M3_FLAG_* without the internal recompute bits
    bool redo;
};

template <class CF, class RNG, class Store>
M3_HD LookCand look_eval(const typename CF::Bd* P0, uint32_t seed, uint32_t m397, int n_actions, int action,
                         Store& st, const typename CF::Dim& dm) {
    typename CF::Bd P[CF::NP], HL, VL;
#pragma unroll
    for (int p = 0; p < CF::NP; ++p) P[p] = P0[p];
    RNG rng;
    rng.init(seed, m397);
    uint32_t f;
    LookCand c;
    c.reward = apply_action<CF>(P, n_actions, action, rng, f, HL, VL, st, dm);
    c.redo = (f & FLAG_RECOMPUTE) != 0u;
    c.draws = (f & (FLAG_TERMINAL | FLAG_BAD_ACTION)) ? 0u : rng.draws();
    c.flags = f & ~(uint32_t)FLAG_RECOMPUTE;
    return c;
}

// What a group's candidates fold into, one per board (LDS in the kernel).
struct LookAcc {
    unsigned long long key;  // best (reward, lowest id) so far
    uint32_t flags;          // OR of the candidates' flags
    uint32_t last_draws;     // draws of the highest legal id's apply
    uint32_t redo;           // some candidate needs the exact pass: the board is handed over whole
};

M3_HD void look_acc_init(LookAcc& a, int n_actions, uint32_t count) {
    a.key = LOOK_KEY_NONE;
    a.flags = (n_actions < 1 ? (uint32_t)FLAG_TERMINAL : 0u) | (count == 0u ? (uint32_t)FLAG_NO_LEGAL : 0u);
    a.last_draws = 0u;
    a.redo = 0u;
}

// Fold candidate `action` (is_last: the board's highest legal id) into its board. In the kernel the
// lanes of a round fold concurrently: the key by a 64-bit maximum, which no order of arrival changes.
M3_HD void look_fold(LookAcc* a, const LookCand& c, int action, bool is_last) {
#ifdef __HIP_DEVICE_COMPILE__
    if (c.redo) {
        atomicOr(&a->redo, 1u);
        return;
    }
    atomicMax(&a->key, (unsigned long long)look_key(c.reward, action));
    if (c.flags) atomicOr(&a->flags, c.flags);
    if (is_last) a->last_draws = c.draws;
#else
    if (c.redo) {
        a->redo = 1u;
        return;
    }
    const uint64_t k = look_key(c.reward, action);
    if (look_key_better(k, a->key)) a->key = k;
    a->flags |= c.flags;
    if (is_last) a->last_draws = c.draws;
#endif
}

// The exact pass: every candidate of one handed-over board with the full 624-word generator and the
// full group table. `lane`/`lanes`: candidates lane, lane + lanes, .. are this caller's (the kernel:
// one board per wave, 64 lanes; the host: 0 / 1). values (nullable): the board's row of the table.
template <class CF>
M3_HD void look_exact(const typename CF::Bd* P0, const uint32_t* act, uint32_t seed, int n_actions,
                      uint32_t lane, uint32_t lanes, uint64_t& key, uint32_t& flags, uint32_t& last_draws,
                      int32_t* values, FullMT& mt, ArrayStore<CF>& st, const typename CF::Dim& dm) {
    const uint32_t total = look_count(act, dm.aw());
    for (uint32_t base = 0; base < total; base += lanes) {
        const uint32_t j = base + lane;
        if (j < total) {
            const int action = look_kth_bit(act, dm.aw(), j);
            typename CF::Bd P[CF::NP], HL, VL;
#pragma unroll
            for (int p = 0; p < CF::NP; ++p) P[p] = P0[p];
            mt.init(seed, 0u);
            uint32_t f;
            const int32_t r = apply_action<CF>(P, n_actions, action, mt, f, HL, VL, st, dm);
            const uint64_t k = look_key(r, action);
            if (look_key_better(k, key)) key = k;
            flags |= f & ~(uint32_t)FLAG_RECOMPUTE;
            if (j + 1u == total) last_draws = (f & (FLAG_TERMINAL | FLAG_BAD_ACTION)) ? 0u : mt.draws();
            if (values) values[action] = r;
        }
    }
}

}  // namespace m3
