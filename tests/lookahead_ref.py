"""The "oracle lookahead" the lookahead tests compare against, and the states they share.

Written from Oracle.legal_actions + Oracle.apply_action only (the reference's loop,
boardv2.py:209-218): every legal id ascending, each applied to the board on its own, the first
strict maximum kept. About 1 ms per board; results are cached per call site and read-only.
"""
from __future__ import annotations

import numpy as np

from oracle import Oracle

FLAG_TERMINAL, FLAG_BAD_ACTION, FLAG_NO_LEGAL = 0x01, 0x02, 0x08

_cache = {}


def oracle_lookahead(shape, boards, seeds, n_actions):
    """dict(values [n, A] (-1 where illegal), best_action, best_reward, last_draws, flags, counts,
    draw_table [n, A]: the raw draws of each candidate's apply)."""
    o = Oracle(*shape)
    boards = np.asarray(boards).reshape(-1, o.R, o.C).astype(np.int32)
    n = len(boards)
    seeds = np.broadcast_to(np.asarray(seeds, dtype=np.uint32), (n,))
    na = np.broadcast_to(np.asarray(n_actions, dtype=np.int32), (n,))
    res = dict(values=np.full((n, o.A), -1, np.int32), best_action=np.full(n, -1, np.int32),
               best_reward=np.full(n, -1, np.int32), last_draws=np.zeros(n, np.uint32), flags=np.zeros(n, np.uint32),
               counts=np.zeros(n, np.int32), draw_table=np.zeros((n, o.A), np.int32))
    for i in range(n):
        legal = o.legal_actions(boards[i])
        res["counts"][i] = len(legal)
        fl = (FLAG_TERMINAL if na[i] < 1 else 0) | (0 if legal else FLAG_NO_LEGAL)
        best, best_r, draws = -1, -1, 0
        for a in legal:  # ascending ids; the first strict maximum wins
            _, r, d, f = o.apply_action(boards[i], int(seeds[i]), a, int(na[i]))
            res["values"][i, a] = r
            res["draw_table"][i, a] = d
            fl |= f
            draws = 0 if f & (FLAG_TERMINAL | FLAG_BAD_ACTION) else d
            if r > best_r:
                best, best_r = a, r
        res["best_action"][i], res["best_reward"][i] = best, best_r
        res["last_draws"][i], res["flags"][i] = draws, fl
    for a in res.values():
        a.setflags(write=False)
    return res


def cached_lookahead(key, shape, boards, seeds, n_actions):
    k = ("la", key)
    if k not in _cache:
        _cache[k] = oracle_lookahead(shape, boards, seeds, n_actions)
    return _cache[k]


def mid_episode_states(shape, n, first_seed=1, moves=20):
    """n states of oracle random episodes (seeded random play, samplerTasks.py:9-14): state i is
    episode first_seed + i after i % moves steps, so specials are present and the depths spread.
    dict(boards int8 [n, R, C], seeds uint32, n_actions int32)."""
    k = ("mid", tuple(shape), n, first_seed, moves)
    if k in _cache:
        return _cache[k]
    o = Oracle(*shape)
    boards = np.zeros((n, o.R, o.C), np.int8)
    seeds = np.arange(first_seed, first_seed + n, dtype=np.uint32)
    na = np.zeros(n, np.int32)
    for i in range(n):
        s, depth = int(seeds[i]), i % moves
        b, _ = o.init_board(s)
        a, _ = o.random_action(b, s)
        left = moves
        for _ in range(depth):
            if a < 0:
                break
            b, _, _, _, a, _ = o.apply_action_next(b, s, a, left)
            left -= 1
        boards[i], na[i] = b, left
    res = dict(boards=boards, seeds=seeds, n_actions=na)
    for a in res.values():
        a.setflags(write=False)
    _cache[k] = res
    return res


def greedy_states(golden_mcts, shape=(9, 9, 6)):
    """The 32 mcts.npz gr_* states at depth seed % 7 of the reference's greedy episodes."""
    k = ("gr",)
    if k in _cache:
        return _cache[k]
    o = Oracle(*shape)
    g = golden_mcts
    n = len(g["gr_seed"])
    boards = np.zeros((n, o.R, o.C), np.int8)
    na = np.zeros(n, np.int32)
    for i, (seed, acts) in enumerate(zip(g["gr_seed"], g["gr_actions"])):
        b, _ = o.init_board(int(seed))
        left = 20
        for a in acts[: int(seed) % 7]:
            b, _, _, _ = o.apply_action(b, int(seed), int(a), left)
            left -= 1
        boards[i], na[i] = b, left
    res = dict(boards=boards, seeds=np.asarray(g["gr_seed"], dtype=np.uint32), n_actions=na)
    for a in res.values():
        a.setflags(write=False)
    _cache[k] = res
    return res


def assert_equal(got, want, what=""):
    """Values table (when present), best action, best reward, last draws and flags all equal."""
    for k in ("values", "best_action", "best_reward", "last_draws", "flags"):
        if k in got and got[k] is not None:
            bad = np.flatnonzero((np.asarray(got[k]) != np.asarray(want[k])).reshape(len(want[k]), -1).any(axis=1))
            assert len(bad) == 0, (what, k, bad[:8], np.asarray(got[k])[bad[:2]], np.asarray(want[k])[bad[:2]])
