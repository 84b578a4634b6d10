"""Episode scorers of the reference's ``samplerTasks.py`` over the device step, and batched greedy.

``random_task`` / ``greedy_test`` / ``mcts_task`` / ``nn_mcts_task`` restate samplerTasks.py:9-42
(the NN variant takes any ``model(array[1, R, C]) -> (value, policy)``; the JAX net itself is out of
scope), and ``nn_mcts_episodes`` plays many such episodes in lockstep on the device trees. The
reference functions take no arguments and draw the board seed from numpy's
global RNG (``BoardConfig()``, boardConfig.py:34); here ``seed`` may be given
to make an episode reproducible, and ``None`` keeps the reference behaviour.

``greedy_actions_device(states)`` is the same list from ONE ``m3_lookahead`` call: the states go up
once (no host legal sets, no board per candidate) and the device evaluates every legal action;
``greedy_episodes(seeds)`` plays whole greedy episodes in one batched env.

``greedy_actions(states)`` is ``[s.greedy_action for s in states]``
(boardv2.py:209-218) for many boards in ONE launch: every legal action of
every state is applied by one ``m3_apply_actions`` call and each state keeps
its first maximum, as the reference loop does.
"""
from __future__ import annotations

from typing import List, Sequence

import numpy as np

from . import _native
from .boardConfig import BoardConfig
from .boardv2 import BoardV2, _ids_past_board, _sync_global_rng
from .mcts import MCTS, NeuralNetworkMCTS


def _start(seed, moves=20):
    state = BoardV2(moves, BoardConfig(seed=seed))
    np.random.seed(state.cfg.seed)                                # samplerTasks.py:11
    return state


def random_task(seed=None) -> int:
    """samplerTasks.py:9-14: seeded random actions until terminal; returns the episode reward."""
    state = _start(seed)
    while not state.is_terminal:
        state = state.apply_action(np.random.choice(state.legal_actions))
    return state.reward


def greedy_test(seed=None) -> int:
    """samplerTasks.py:17-22: the best one-step action every move."""
    state = _start(seed)
    while not state.is_terminal:
        state = state.apply_action(state.greedy_action)
    return state.reward


def mcts_task(seed=None, exploration_weight=2, simulations=100) -> int:
    """samplerTasks.py:25-32: MCTS(state, 2, 100) every move, device rollouts."""
    state = _start(seed)
    search = MCTS(state, exploration_weight, simulations, False, deterministic=False)
    while not state.is_terminal:
        action, _, _ = search()
        state = state.apply_action(action)
    return state.reward


def nn_mcts_task(model, seed=None, exploration_weight=3, simulations=100, moves=20) -> int:
    """samplerTasks.py:35-42: NeuralNetworkMCTS(model, state, 3, 100) every move, trees on the device."""
    state = _start(seed, moves)
    search = NeuralNetworkMCTS(model, state, exploration_weight, simulations, verbose=False)
    while not state.is_terminal:
        action, _, _ = search()
        state = state.apply_action(action)
    return state.reward


def nn_mcts_episodes(seeds, evaluator=None, weights=None, moves: int = 20, simulations: int = 100, rows: int = 9,
                     columns: int = 9, types: int = 6, net=None):
    """``nn_mcts_task`` for every seed at once, in lockstep: one ``DeviceSearchNN`` over all games, one
    search and one re-rooting per move. ``evaluator`` / ``weights`` / ``net`` as ``DeviceSearchNN`` takes
    them (a batch evaluator on the host, or the built-in linear evaluator or an ``ElementCrushNet`` on the
    device). Returns the episode scores [len(seeds)]."""
    from .search import DeviceSearchNN

    seeds = [int(s) for s in np.atleast_1d(seeds)]
    states = [BoardV2(moves, BoardConfig(rows=rows, columns=columns, types=types, seed=s)) for s in seeds]
    ds = DeviceSearchNN(states, simulations, evaluator=evaluator, weights=weights, net=net)
    try:
        for _ in range(moves):
            ds()
        return np.array([s.reward for s in ds.states()], dtype=np.int64)
    finally:
        ds.close()


def greedy_actions(states: Sequence[BoardV2], sync_rng: bool = False) -> List:
    """``greedy_action`` of every state (one board shape) with all candidates in one launch.

    sync_rng=True leaves numpy's global RNG as the LAST state's greedy_action would."""
    states = list(states)
    if not states:
        return []
    cfg = states[0].cfg
    shape = (cfg.rows, cfg.columns, cfg.types)
    if any((s.cfg.rows, s.cfg.columns, s.cfg.types) != shape for s in states):
        raise ValueError("greedy_actions() needs states of one board shape")
    legal = [s.legal_actions for s in states]
    counts = np.array([len(x) for x in legal])
    owner = np.repeat(np.arange(len(states)), counts)
    if len(owner) == 0:
        return [None] * len(states)
    acts = np.concatenate([np.asarray(x, dtype=np.int32) for x in legal if len(x)])
    boards = np.stack([np.asarray(states[i].array) for i in owner])
    seeds = np.array([int(states[i].cfg.seed) & 0xFFFFFFFF for i in owner], dtype=np.uint32)
    n_act = np.array([states[i].n_actions for i in owner], dtype=np.int32)
    res = _native.context(*shape).apply_actions(boards, seeds, n_act, acts)
    out, pos = [], 0
    for i, s in enumerate(states):
        k = int(counts[i])
        if k == 0:
            out.append(None)
            continue
        totals = s.reward + res["reward"][pos:pos + k].astype(np.int64)
        out.append(int(acts[pos + int(np.argmax(totals))]))   # argmax = first maximum, as the loop
        pos += k
    if sync_rng and counts[-1] and not states[-1].is_terminal:
        _sync_global_rng(states[-1].cfg.seed, int(res["draws"][-1]))
    return out


def greedy_actions_device(states: Sequence[BoardV2], sync_rng: bool = False) -> List:
    """``greedy_actions`` over the device lookahead (m3_lookahead): one board per state goes up,
    the legal sets and every candidate stay on the device. Same contract: None for a state without
    a legal action; sync_rng=True leaves numpy's global RNG as the LAST state's greedy_action would."""
    states = list(states)
    if not states:
        return []
    cfg = states[0].cfg
    shape = (cfg.rows, cfg.columns, cfg.types)
    if any((s.cfg.rows, s.cfg.columns, s.cfg.types) != shape for s in states):
        raise ValueError("greedy_actions_device() needs states of one board shape")
    _ids_past_board(cfg)  # rows < columns: IndexError, as legal_actions / apply_action raise
    boards = np.stack([np.asarray(s.array) for s in states])
    seeds = np.array([int(s.cfg.seed) & 0xFFFFFFFF for s in states], dtype=np.uint32)
    n_act = np.array([s.n_actions for s in states], dtype=np.int32)
    res = _native.context(*shape).lookahead(boards, seeds, n_act)
    out = [None if a < 0 else int(a) for a in res["best_action"]]
    if sync_rng and out[-1] is not None and not states[-1].is_terminal:
        _sync_global_rng(states[-1].cfg.seed, int(res["last_draws"][-1]))
    return out


def greedy_episodes(seeds, moves: int = 20, rows: int = 9, columns: int = 9, types: int = 6, device: int = 0):
    """``greedy_test`` (samplerTasks.py:17-22) for every seed at once: one batched env, autoreset off
    and no score goal, ``moves`` greedy steps on the device. Returns the episode scores [len(seeds)]."""
    from .batched import BatchedMatch3Env

    seeds = np.ascontiguousarray(np.atleast_1d(seeds), dtype=np.uint32)
    env = BatchedMatch3Env(len(seeds), rows, columns, types, num_moves=moves, env_goal=2**31 - 1, device=device,
                           seeds=seeds, autoreset=False)
    try:
        for _ in range(moves):
            env.step_greedy()
        return env.scores().astype(np.int64)
    finally:
        env.close()
