"""Device-resident MCTS: the search trees of many games in GPU memory, searched in lockstep.

``match3tile.mcts.search_lockstep`` keeps every tree in Python: a simulation round walks each game's
tree on the host, expands one node per game with a batch-1 ``apply_action`` and makes one blocking
rollout call. ``DeviceSearch`` holds the trees in device memory (``m3_search_*``, include/m3.h): a
round is selection, the expansions' ``apply_action``, the attach, the rollouts and the backup as five
launches for all games at once, and a whole ``__call__`` -- ``simulations`` rounds -- is enqueued
without a host round trip.

The search is the reference's (mctslib/abc/mcts.py:71-128, standard/mcts.py), node for node: expansion
order, UCB1 with the node's ``n_actions`` as the exploration weight, evaluated bit for bit as CPython
evaluates it, one ``random.randint(0, 2**31 - 1)`` rollout seed per simulation from each game's own
generator, root re-use between calls. So game g returns what ``MCTS(states[g], c, simulations,
rng=rngs[g])()`` returns. (The reference's ``exploration_weight`` argument is not read by its
selection, abc/mcts.py:96, and has no counterpart here.)

One departure, kept on purpose: a root that is already terminal (``n_actions < 1``) when the trees are
built. The reference's constructor expands unconditionally (abc/mcts.py:82), ``apply_action`` of a
terminal state returns the state itself, and ``MCTS(...)()`` answers with an unplayable action and
the policy ``[0.0]``. Here such a root keeps no child: ``result()`` reports ``best_action`` -1, no
children, ``value`` = the root's reward, and the simulations in ``root_visits``; ``__call__`` raises
``ValueError``, as it does -- there like the reference, whose last lines raise -- for a root that
became terminal by re-rooting. ``dataset.play_games`` never builds such a root.

A game freezes (include/m3.h) where the reference raises or never returns; ``result()["flags"]`` holds
its ``M3_FLAG_*`` word, its tree stays as it stood, and the games beside it go on. Board shapes with a
side above 16 (the 32 x 32 frame of the kernels) are searched like any other.

``leaf_rollouts > 1`` and ``deterministic=True`` stay on the host path (``match3tile.mcts.MCTS``).

``DeviceSearchNN`` (below) is the network-guided search of the reference (mctslib/nn/mcts.py) on the same
kind of trees: priors from an evaluator's logits, the evaluator's value backed up instead of a playout,
the evaluator behind one batched call per round or, for the built-in linear one, on the device.

numpy's global RNG: the reference leaves it where the last rollout's last ``apply_action`` left it.
After a device search its state is unspecified (nothing is replayed into it); nothing in
``dataset.play_games`` reads it.

Memory: ``node_capacity`` node slots per game, 16 + 32 + 4 * ceil(A / 32) + rows * columns bytes each
(9x9x6: 149 bytes, so the default ``2 + n_actions * simulations`` slots of a 20-move, 256-simulation
game are 763 KB per game, 3.1 GB for 4,096 games). Slots are not reclaimed on re-rooting.
"""
from __future__ import annotations

import ctypes
import random
from typing import List, Optional, Sequence

import numpy as np

from . import _native
from .boardv2 import BoardV2
from .mcts import SEED_BOUND

_CAPS = _native.FLAG_SHUFFLE_CAP | _native.FLAG_CASCADE_CAP


class DeviceSearch:
    """``DeviceSearch(states, simulations, rngs=None, node_capacity=None)``: one tree per BoardV2 state.

    All states share a board shape and ``simulations``. ``rngs[g]`` (default: the ``random`` module for
    every game, drawn game by game) is the source of game g's rollout seeds. ``node_capacity``
    defaults to ``2 + max(n_actions) * simulations``: enough for one ``__call__`` per remaining move."""

    def __init__(self, states: Sequence, simulations: int, rngs: Optional[Sequence] = None,
                 node_capacity: Optional[int] = None):
        states = list(states)
        if not states:
            raise ValueError("DeviceSearch needs at least one state")
        cfg = states[0].cfg
        shape = (cfg.rows, cfg.columns, cfg.types)
        if any((s.cfg.rows, s.cfg.columns, s.cfg.types) != shape for s in states):
            raise ValueError("DeviceSearch needs states of one board shape")
        if rngs is not None and len(rngs) != len(states):
            raise ValueError("one rng per state")
        self._ctx = _native.context(*shape)
        self._cfgs = [s.cfg for s in states]
        self._rngs = [random] * len(states) if rngs is None else list(rngs)
        self.simulations = int(simulations)
        self.n = len(states)
        if node_capacity is None:
            node_capacity = 2 + max(1, max(s.n_actions for s in states)) * self.simulations
        self.node_capacity = int(node_capacity)
        h = ctypes.c_void_p()
        _native.check(_native.lib().m3_search_create(self._ctx.handle, self.n, self.node_capacity, ctypes.byref(h)))
        self._h = h
        boards = self._ctx._boards(np.stack([np.asarray(s.array) for s in states]))
        seeds = np.array([int(s.cfg.seed) & 0xFFFFFFFF for s in states], dtype=np.uint32)
        na = np.array([s.n_actions for s in states], dtype=np.int32)
        rew = np.array([int(s.reward) for s in states], dtype=np.int32)
        with self._ctx._lock:
            _native.check(_native.lib().m3_search_set_roots(self._h, _native.ptr(boards), _native.ptr(seeds),
                                                            _native.ptr(na), _native.ptr(rew)))
        self._states = [s.clone() for s in states]

    def close(self):
        if getattr(self, "_h", None):
            _native.lib().m3_search_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- the raw calls -------------------------------------------------------------
    def run(self, rollout_seeds) -> None:
        """Enqueue len(rollout_seeds) rounds; rollout_seeds [rounds][n]. Does not wait for the kernels.
        Raises M3Error (M3_ERR_CAP) if the rounds do not fit node_capacity; nothing is run then."""
        rs = np.ascontiguousarray(rollout_seeds, dtype=np.uint32).reshape(-1, self.n)
        with self._ctx._lock:
            _native.check(_native.lib().m3_search_run(self._h, len(rs), _native.ptr(rs)))

    def result(self, children: bool = True) -> dict:
        """m3_search_result: best_action, value, root_visits, n_children, flags and, with children, the
        root's child_action / child_visits / child_reward [n, A] in expansion order. Blocks."""
        n, A = self.n, self._ctx.A
        out = dict(best_action=np.empty(n, np.int32), value=np.empty(n, np.int32), root_visits=np.empty(n, np.int32),
                   n_children=np.empty(n, np.int32), child_action=np.empty((n, A), np.int32) if children else None,
                   child_visits=np.empty((n, A), np.int32), child_reward=np.empty((n, A), np.int64) if children else None,
                   flags=np.empty(n, np.uint32))
        order = ("best_action", "value", "root_visits", "n_children", "child_action", "child_visits", "child_reward",
                 "flags")
        with self._ctx._lock:
            _native.check(_native.lib().m3_search_result(self._h, *[_native.ptr(out[k]) for k in order]))
        return out

    def stats(self) -> dict:
        out = np.zeros(4, np.uint64)
        with self._ctx._lock:
            _native.check(_native.lib().m3_search_stats(self._h, _native.ptr(out)))
        return dict(nodes_used=int(out[0]), rounds=int(out[1]), apply_exact=int(out[2]), rollout_exact=int(out[3]))

    def advance(self, actions=None) -> List[BoardV2]:
        """Re-root every game at the child ``actions[g]`` leads to (None: the last result's best
        action) and return the new roots. The subtrees keep their statistics."""
        n, ctx = self.n, self._ctx
        act = None if actions is None else np.ascontiguousarray(actions, dtype=np.int32).reshape(n)
        boards = np.empty((n, ctx.N), np.int8)
        rew, na = np.empty(n, np.int32), np.empty(n, np.int32)
        legal = np.empty((n, ctx.words), np.uint32)
        with ctx._lock:
            _native.check(_native.lib().m3_search_advance(self._h, _native.ptr(act), _native.ptr(boards), _native.ptr(rew),
                                                          _native.ptr(na), _native.ptr(legal)))
        states = []
        for g in range(n):
            st = BoardV2(int(na[g]), self._cfgs[g], boards[g].astype(np.int64).reshape(ctx.rows, ctx.columns))
            st._reward = int(rew[g])
            st._actions = _native.bits_to_actions(legal[g], ctx.A)
            states.append(st)
        self._states = states
        return self.states()

    def states(self) -> List[BoardV2]:
        """The current roots."""
        return [s.clone() for s in self._states]

    # ---- MCTS.__call__ ----------------------------------------------------------------
    def __call__(self):
        """``simulations`` rounds for every game, then re-root at the best action, as ``MCTS.__call__``.
        Returns [(action, value, policies)] per game; policies = child visits / root visits in
        expansion order. ValueError where ``rollouts()`` raises (a state without a legal action),
        RuntimeError where a step or a rollout stopped at a shuffle or cascade cap (the cap decides for
        a game that holds both; a game of the first kind anywhere in the batch is reported first)."""
        if any(s.is_terminal for s in self._states):
            raise ValueError("search of a terminal state (after a re-rooting the reference's MCTS.__call__ raises in its "
                             "last lines; a root that was terminal from the start has no child here: see the module docstring)")
        seeds = np.empty((self.simulations, self.n), np.uint32)
        for g, rng in enumerate(self._rngs):  # game by game: each game's seeds in order from its own generator
            seeds[:, g] = [rng.randint(0, SEED_BOUND) for _ in range(self.simulations)]
        self.run(seeds)
        res = self.result(children=False)
        fl = res["flags"]
        # (a playout that stopped at a cap finds no legal action at its next move: that game's
        # M3_FLAG_NO_LEGAL comes from the cap, where the reference is still shuffling)
        if ((fl & _native.FLAG_NO_LEGAL != 0) & (fl & _CAPS == 0)).any():
            raise ValueError("a search reached a board with no legal action (np.random.choice of an empty list)")
        if (fl & _CAPS).any():
            raise RuntimeError("a step or a rollout of the search stopped at a shuffle or cascade cap "
                               "(M3_FLAG_SHUFFLE_CAP / M3_FLAG_CASCADE_CAP): the reference would not return")
        out = []
        for g in range(self.n):
            k, rv = int(res["n_children"][g]), int(res["root_visits"][g])
            out.append((int(res["best_action"][g]), int(res["value"][g]),
                        [int(v) / rv for v in res["child_visits"][g][:k]]))
        self.advance(None)
        return out


def onehot_width(types: int) -> int:
    """The reference's one-hot width of a cell (elementCrush.py:66): 2 ** (ceil(log2(types)) + 2)."""
    return 2 ** ((int(types) - 1).bit_length() + 2)


def linear_evaluator(weights):
    """The built-in linear evaluator (m3_search_nn_run_linear) as a host evaluator for
    ``DeviceSearchNN(evaluator=...)``, bit for bit: out[j] is the float32 sum, cell after cell in
    ascending order, of ``weights[cell, board[cell], j]`` over the cells whose value is below CH;
    logits = out[:A], value = out[A]."""
    W = np.ascontiguousarray(weights, dtype=np.float32)
    N, CH, J = W.shape

    def run(boards, need):
        n = len(boards)
        out = np.zeros((n, J), np.float32)
        for g in np.flatnonzero(need):
            acc = None
            for i, x in enumerate(np.asarray(boards[g]).reshape(-1)):
                if 0 <= x < CH:
                    acc = W[i, x].copy() if acc is None else acc + W[i, x]
            if acc is not None:
                out[g] = acc
        return out[:, J - 1].copy(), out[:, :J - 1].copy()
    return run


class DeviceSearchNN:
    """``DeviceSearchNN(states, simulations, evaluator=None, weights=None, node_capacity=None, net=None)``: the
    network-guided search of the reference (mctslib/nn/mcts.py: NNNode, NeuralNetworkMCTS), one tree per
    BoardV2 state in device memory (``m3_search_nn_*``, include/m3.h), all games in lockstep.

    One of ``evaluator`` / ``weights`` / ``net`` is given:

    - ``evaluator(boards: np.int8 [n, R, C], need: np.bool_ [n]) -> (values f32 [n], logits f32 [n, A])``
      is called once per round with every game's batch row on the host; rows with ``need`` False are
      ignored. Every created, non-terminal node is evaluated exactly once.
    - ``weights``: f32 ``[N, CH, A + 1]`` (``CH = onehot_width(types)``) of the built-in linear
      evaluator, which runs on the device: a whole ``__call__`` is enqueued without a host round trip.
    - ``net``: a ``match3tile.net.ElementCrushNet`` of the states' board shape, the reference's
      policy/value network on the device (``m3_search_nn_run_net``): as with ``weights`` a whole
      ``__call__`` is enqueued without a host round trip. The search does not own the net.
    - ``evaluator=False``: the caller drives the rounds itself with ``batch`` and ``feed`` /
      ``feed_device``, the two construction batches included (``run`` and ``__call__`` are not for it).

    The logits stay raw (no softmax; they may be negative); a child's prior is its parent's logit at
    the child's action; the value of a new non-terminal child -- the state reward of a terminal one --
    is backed up as float32. The arithmetic is in csrc/m3_search_nn_core.hpp. The trees are pinned to
    the reference's own tree code. It is executed with numpy standing in for ``jax.numpy`` and with
    integer rewards handed over as Python ints, so that numpy promotes as JAX does with x64 off. JAX
    itself has still not been run.

    An already-terminal root behaves as documented for ``DeviceSearch``. ``node_capacity`` defaults to
    ``2 + max(n_actions) * simulations``; a slot is 16 + 32 + 4 * ceil(A / 32) + rows * columns + 4 * A
    bytes (9x9x6: 725)."""

    def __init__(self, states: Sequence, simulations: int, evaluator=None, weights=None,
                 node_capacity: Optional[int] = None, net=None):
        states = list(states)
        if not states:
            raise ValueError("DeviceSearchNN needs at least one state")
        if (evaluator is not None) + (weights is not None) + (net is not None) != 1:
            raise ValueError("DeviceSearchNN needs exactly one of evaluator=, weights= and net=")
        cfg = states[0].cfg
        shape = (cfg.rows, cfg.columns, cfg.types)
        if any((s.cfg.rows, s.cfg.columns, s.cfg.types) != shape for s in states):
            raise ValueError("DeviceSearchNN needs states of one board shape")
        if net is not None and (net.cfg.rows, net.cfg.columns, net.cfg.types) != shape:
            raise ValueError(f"net= of board shape {(net.cfg.rows, net.cfg.columns, net.cfg.types)}, the states are "
                             f"{shape}")
        self._net = net
        self._ctx = ctx = _native.context(*shape)
        self._cfgs = [s.cfg for s in states]
        self._evaluator = evaluator
        self.simulations = int(simulations)
        self.n = len(states)
        if node_capacity is None:
            node_capacity = 2 + max(1, max(s.n_actions for s in states)) * self.simulations
        self.node_capacity = int(node_capacity)
        self._w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float32)
            want = (ctx.N, onehot_width(cfg.types), ctx.A + 1)
            if w.shape != want:
                raise ValueError(f"weights of shape {w.shape}, expected {want}")
            self._w = ctx.device_array(w)
        h = ctypes.c_void_p()
        _native.check(_native.lib().m3_search_nn_create(ctx.handle, self.n, self.node_capacity, ctypes.byref(h)))
        self._h = h
        boards = ctx._boards(np.stack([np.asarray(s.array) for s in states]))
        seeds = np.array([int(s.cfg.seed) & 0xFFFFFFFF for s in states], dtype=np.uint32)
        na = np.array([s.n_actions for s in states], dtype=np.int32)
        rew = np.array([int(s.reward) for s in states], dtype=np.int32)
        with ctx._lock:
            _native.check(_native.lib().m3_search_nn_set_roots(self._h, _native.ptr(boards), _native.ptr(seeds),
                                                               _native.ptr(na), _native.ptr(rew)))
        self._states = [s.clone() for s in states]
        self._construction = 2  # batches of the construction still to be fed (abc/mcts.py:82)
        if evaluator is not False:
            self.run(0)

    def close(self):
        if getattr(self, "_h", None):
            _native.lib().m3_search_nn_destroy(self._h)
            self._h = None
        if getattr(self, "_w", None) is not None:
            self._w.free()
            self._w = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- the raw calls -------------------------------------------------------------
    def batch(self, remaining: int = 1):
        """m3_search_nn_batch, read back: (boards int8 [n, R, C], need bool [n]). Blocks."""
        ctx, L = self._ctx, _native.lib()
        pb, pn = ctypes.c_void_p(), ctypes.c_void_p()
        boards, need = np.empty((self.n, ctx.rows, ctx.columns), np.int8), np.empty(self.n, np.uint8)
        with ctx._lock:
            _native.check(L.m3_search_nn_batch(self._h, int(remaining), ctypes.byref(pb), ctypes.byref(pn)))
            _native.check(L.m3_ctx_synchronize(ctx.handle))
            _native.check(L.m3_dev_copy(ctx.handle, _native.ptr(boards), pb, boards.nbytes, 2))
            _native.check(L.m3_dev_copy(ctx.handle, _native.ptr(need), pn, need.nbytes, 2))
        return boards, need.astype(np.bool_)

    def feed(self, values, logits) -> None:
        """m3_search_nn_feed: the evaluator's answer to the pending batch, from host arrays."""
        v = np.ascontiguousarray(values, dtype=np.float32).reshape(self.n)
        lg = np.ascontiguousarray(logits, dtype=np.float32).reshape(self.n, self._ctx.A)
        with self._ctx._lock:
            _native.check(_native.lib().m3_search_nn_feed(self._h, _native.ptr(v), _native.ptr(lg)))

    def feed_device(self, d_values, d_logits) -> None:
        """m3_search_nn_feed_device: the answer in device memory (``_native.DeviceArray`` or pointers), f32
        [n] and f32 [n, A]. The caller's own stream must have finished writing them; the arrays must
        stay valid until the context stream has passed this round. Does not wait."""
        pv, pl = (getattr(d, "ptr", d) for d in (d_values, d_logits))
        with self._ctx._lock:
            _native.check(_native.lib().m3_search_nn_feed_device(self._h, pv, pl))
        if self._construction:
            self._construction -= 1

    def run(self, simulations: Optional[int] = None) -> None:
        """The construction batches still to come, then ``simulations`` rounds (default: the object's).
        Raises M3Error (M3_ERR_CAP) if the rounds do not fit node_capacity; nothing is run then."""
        sims = self.simulations if simulations is None else int(simulations)
        if self._w is not None:
            with self._ctx._lock:
                _native.check(_native.lib().m3_search_nn_run_linear(self._h, sims, self._w.ptr))
            self._construction = 0
            return
        if self._net is not None:
            with self._ctx._lock:
                _native.check(_native.lib().m3_search_nn_run_net(self._h, sims, self._net.handle))
            self._construction = 0
            return
        while self._construction or sims:
            boards, need = self.batch(max(1, sims))  # (a run that does not fit is refused at its first batch)
            values, logits = self._evaluator(boards, need)
            self.feed(values, logits)
            if self._construction:
                self._construction -= 1
            else:
                sims -= 1

    def result(self, children: bool = True) -> dict:
        """m3_search_nn_result: best_action, value, root_visits, n_children, flags and, with children,
        the root's child_action / child_visits / child_value_sum / child_prior [n, A] in expansion
        order. Blocks."""
        n, A = self.n, self._ctx.A
        out = dict(best_action=np.empty(n, np.int32), value=np.empty(n, np.int32), root_visits=np.empty(n, np.int32),
                   n_children=np.empty(n, np.int32), child_action=np.empty((n, A), np.int32) if children else None,
                   child_visits=np.empty((n, A), np.int32),
                   child_value_sum=np.empty((n, A), np.float32) if children else None,
                   child_prior=np.empty((n, A), np.float32) if children else None, flags=np.empty(n, np.uint32))
        order = ("best_action", "value", "root_visits", "n_children", "child_action", "child_visits", "child_value_sum",
                 "child_prior", "flags")
        with self._ctx._lock:
            _native.check(_native.lib().m3_search_nn_result(self._h, *[_native.ptr(out[k]) for k in order]))
        return out

    def stats(self) -> dict:
        out = np.zeros(6, np.uint64)
        with self._ctx._lock:
            _native.check(_native.lib().m3_search_nn_stats(self._h, _native.ptr(out)))
        return dict(nodes_used=int(out[0]), rounds=int(out[1]), apply_exact=int(out[2]), host_feeds=int(out[3]),
                    device_feeds=int(out[4]), linear_evals=int(out[5]))

    def advance(self, actions=None) -> List[BoardV2]:
        """Re-root every game at the child ``actions[g]`` leads to (None: the last result's best
        action) and return the new roots. The subtrees keep their statistics."""
        n, ctx = self.n, self._ctx
        act = None if actions is None else np.ascontiguousarray(actions, dtype=np.int32).reshape(n)
        boards = np.empty((n, ctx.N), np.int8)
        rew, na = np.empty(n, np.int32), np.empty(n, np.int32)
        legal = np.empty((n, ctx.words), np.uint32)
        with ctx._lock:
            _native.check(_native.lib().m3_search_nn_advance(self._h, _native.ptr(act), _native.ptr(boards),
                                                             _native.ptr(rew), _native.ptr(na), _native.ptr(legal)))
        states = []
        for g in range(n):
            st = BoardV2(int(na[g]), self._cfgs[g], boards[g].astype(np.int64).reshape(ctx.rows, ctx.columns))
            st._reward = int(rew[g])
            st._actions = _native.bits_to_actions(legal[g], ctx.A)
            states.append(st)
        self._states = states
        return self.states()

    def states(self) -> List[BoardV2]:
        """The current roots."""
        return [s.clone() for s in self._states]

    # ---- NeuralNetworkMCTS.__call__ ---------------------------------------------------
    def __call__(self):
        """``simulations`` rounds for every game, then re-root at the best action. Returns
        [(action, value, policies)] per game. Raises like ``DeviceSearch.__call__`` (ValueError for a
        terminal root or a state without a legal action, RuntimeError for a step that stopped at a
        cap), and RuntimeError where an evaluation was not finite (M3_FLAG_BAD_EVAL)."""
        if any(s.is_terminal for s in self._states):
            raise ValueError("search of a terminal state (see the DeviceSearch module docstring)")
        self.run()
        res = self.result(children=False)
        fl = res["flags"]
        if (fl & _native.FLAG_BAD_EVAL).any():
            raise RuntimeError("an evaluator returned a value or a legal logit that is not finite (M3_FLAG_BAD_EVAL)")
        if ((fl & _native.FLAG_NO_LEGAL != 0) & (fl & _CAPS == 0)).any():
            raise ValueError("a search reached a board with no legal action")
        if (fl & _CAPS).any():
            raise RuntimeError("a step of the search stopped at a shuffle or cascade cap "
                               "(M3_FLAG_SHUFFLE_CAP / M3_FLAG_CASCADE_CAP): the reference would not return")
        out = []
        for g in range(self.n):
            k, rv = int(res["n_children"][g]), int(res["root_visits"][g])
            out.append((int(res["best_action"][g]), int(res["value"][g]),
                        [int(v) / rv for v in res["child_visits"][g][:k]]))
        self.advance(None)
        return out
