#!/usr/bin/env python3
"""Golden vectors for the network-guided search (m3_search_nn_*, DeviceSearchNN), from the REAL
reference's tree code: ``NNNode`` / ``NeuralNetworkMCTS`` (mctslib/nn/mcts.py) over ``BaseNode.ucb1``
and ``BaseMCTS.__call__`` (mctslib/abc/mcts.py), on the reference's own ``BoardV2``.

    M3_REFERENCE=<path to the reference> python3 -B tests/golden/gen_golden_search_nn.py

Runs where the reference is (it never travels). Writes ``tests/golden/search_nn.npz``; only data is
committed -- no reference source.

How the reference's code is made to run without JAX and without its network:

  stand-ins  ``mctslib/nn/mcts.py`` uses ``jax.numpy`` for ``jnp.array([state.array])`` alone and
             ``elementCrush`` for one annotation. Two modules written here take their names in
             ``sys.modules`` before the import: ``jax.numpy.array = numpy.array`` and an empty
             ``ElementCrush``.
  adapter    the reference's ``BoardV2.apply_action`` hands ``reward`` over as ``numpy.int64``. Under
             numpy 2 ``float32 + int64`` is float64; JAX with x64 off (the reference's setting)
             promotes that pair to float32. ``_State`` hands ``reward`` and ``n_actions`` over as
             Python ints, which numpy 2 treats as weakly typed -- exactly as JAX treats the int64.
             That JAX promotes this way is taken from JAX's promotion rules; JAX itself is not run.
  evaluators the functions of tests/nn_evaluators.py, the very ones the tests use.

Per case ``X`` (A, C, D, E, Fc, Fn, M, W; and ``A_numpy``: case A without the adapter, i.e. what a
plain numpy execution computes):

  X_shape (R, C, T)  X_sims  X_calls  X_c (the exploration weight handed over; the reference's
  selection uses the state's n_actions instead)  X_wseed (RandomState seed of the linear
  evaluator's weights, -1 without)  X_evname ("linear", "constant", "negative")
  X_board [n, R, C]  X_seed [n]  X_n_actions [n]  X_reward [n]                 the roots
  X_action  X_value  X_root_visits  X_n_children  [n, calls]
  X_policies f64 [n, calls, K] (padded with -1)
  X_child_action / X_child_visits i32, X_child_sum / X_child_prior u32 (float32 bit patterns)
  [n, calls, K], in the dict order of ``root.children``

and one ``ev_<RxCxT>_<wseed>_{board, value_bits, logits_crc}`` triple per linear evaluator: what
``nn_evaluators.linear_eval`` gave for one root board when the file was made.
"""
from __future__ import annotations

import os
import signal
import sys
import time
import types
import zlib

sys.dont_write_bytecode = True
REF = os.environ.get("M3_REFERENCE") or sys.exit("set M3_REFERENCE to the reference's directory")
if REF not in sys.path:
    sys.path.insert(0, REF)

import numpy as np  # noqa: E402

_jax, _jnp, _ec = types.ModuleType("jax"), types.ModuleType("jax.numpy"), types.ModuleType("elementCrush")
_jnp.array = np.array
_jax.numpy = _jnp
_ec.ElementCrush = type("ElementCrush", (), {})
sys.modules.update({"jax": _jax, "jax.numpy": _jnp, "elementCrush": _ec})

from match3tile.boardConfig import BoardConfig  # noqa: E402
from match3tile.boardv2 import BoardV2  # noqa: E402
from mctslib.nn.mcts import NeuralNetworkMCTS  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import nn_evaluators as nev  # noqa: E402

C_WEIGHT = 3
GAME_SECONDS = 120


class _State:
    """The reference's state with its integers handed over as Python ints (see the module docstring)."""

    def __init__(self, inner):
        self._s = inner

    reward = property(lambda self: int(self._s.reward))
    n_actions = property(lambda self: int(self._s.n_actions))
    legal_actions = property(lambda self: self._s.legal_actions)
    is_terminal = property(lambda self: self._s.is_terminal)
    array = property(lambda self: self._s.array)

    def apply_action(self, action):
        return _State(self._s.apply_action(action))

    def clone(self):
        return _State(self._s.clone())


def _alarm(signum, frame):
    raise TimeoutError


def f32_bits(x):
    return int(np.asarray(x, dtype=np.float32).reshape(()).view(np.uint32))


def search(root, model, sims, calls, adapter):
    """[per call: (action, value, policies, root visits, [(action, visits, sum bits, prior bits)])]"""
    m = NeuralNetworkMCTS(model, _State(root) if adapter else root, C_WEIGHT, sims, False)
    out = []
    for _ in range(calls):
        node = m._root  # (the call re-roots; the root it searched keeps its children and visits)
        a, v, p = m()
        kids = [(int(k), int(ch.visits), f32_bits(ch.reward), f32_bits(ch.policy)) for k, ch in node.children.items()]
        out.append((int(a), int(v), [float(x) for x in p], int(node.visits), kids))
    return out


def mid_roots():
    """Case M: 9x9x6, seeds 1001..1008, BoardV2(7, ...) after 1 + g % 4 random legal moves."""
    roots = []
    for g, seed in enumerate(range(1001, 1009)):
        st = BoardV2(7, BoardConfig(seed=seed))
        rs = np.random.RandomState(seed)
        for _ in range(1 + g % 4):
            legal = st.legal_actions
            st = st.apply_action(int(legal[rs.randint(len(legal))]))
        roots.append(st)
    return roots


def reset_roots(shape, seeds, n_actions):
    return [BoardV2(n_actions, BoardConfig(seed=int(s), rows=shape[0], columns=shape[1], types=shape[2])) for s in seeds]


def d_seeds():
    """Case D: the first 8 seeds of 1..39 whose 7x5x4 reset board has a legal action."""
    out = [s for s in range(1, 40) if reset_roots((7, 5, 4), [s], 5)[0].legal_actions][:8]
    assert len(out) == 8
    return out


# name, shape, roots, sims, calls, weight seed (None: a named evaluator), evaluator name
def cases():
    return [
        ("A", (9, 9, 6), reset_roots((9, 9, 6), range(601, 619), 4), 20, 3, 1, "linear"),
        ("C", (16, 16, 8), reset_roots((16, 16, 8), range(701, 705), 5), 12, 1, 3, "linear"),
        ("D", (7, 5, 4), reset_roots((7, 5, 4), d_seeds(), 5), 12, 1, 4, "linear"),
        ("E", (9, 9, 6), reset_roots((9, 9, 6), range(801, 817), 2), 40, 2, 5, "linear"),
        ("Fc", (9, 9, 6), reset_roots((9, 9, 6), range(901, 909), 3), 40, 2, None, "constant"),
        ("Fn", (9, 9, 6), reset_roots((9, 9, 6), range(901, 909), 3), 40, 2, None, "negative"),
        ("M", (9, 9, 6), mid_roots(), 16, 2, 9, "linear"),
        ("W", (20, 20, 6), reset_roots((20, 20, 6), range(1101, 1105), 5), 8, 1, 12, "linear"),
    ]


def model_of(shape, wseed, evname):
    if evname == "linear":
        W = nev.weights(shape, wseed)
        return lambda x: nev.linear_eval(W, x[0])
    ev = nev.constant_ev if evname == "constant" else nev.negative_ev
    return lambda x: ev(x[0], 0, 0)


def run(name, shape, roots, sims, calls, wseed, evname, adapter=True):
    model = model_of(shape, wseed, evname)
    res = []
    signal.signal(signal.SIGALRM, _alarm)
    for g, root in enumerate(roots):
        signal.alarm(GAME_SECONDS)  # a dead board whose shuffle cycles hangs the reference
        try:
            res.append(search(root, model, sims, calls, adapter))
        except TimeoutError:
            raise SystemExit(f"case {name}: game {g} (seed {root.cfg.seed}) did not return in {GAME_SECONDS} s; "
                             "choose another seed and write it into the case list")
        finally:
            signal.alarm(0)
    n = len(roots)
    assert len(res) == n and all(len(r) == calls for r in res), name  # every game finished every call
    K = max(len(c[4]) for r in res for c in r)
    out = {
        "shape": np.array(shape, np.int32), "sims": np.int32(sims), "calls": np.int32(calls), "c": np.int32(C_WEIGHT),
        "wseed": np.int32(-1 if wseed is None else wseed), "evname": np.array(evname),
        "board": np.stack([np.asarray(r.array) for r in roots]).astype(np.int8),
        "seed": np.array([r.cfg.seed for r in roots], np.int64),
        "n_actions": np.array([r.n_actions for r in roots], np.int32),
        "reward": np.array([r.reward for r in roots], np.int64),
        "action": np.array([[c[0] for c in r] for r in res], np.int32),
        "value": np.array([[c[1] for c in r] for r in res], np.int64),
        "root_visits": np.array([[c[3] for c in r] for r in res], np.int32),
        "n_children": np.array([[len(c[4]) for c in r] for r in res], np.int32),
        "policies": np.full((n, calls, K), -1.0, np.float64),
        "child_action": np.full((n, calls, K), -1, np.int32), "child_visits": np.zeros((n, calls, K), np.int32),
        "child_sum": np.zeros((n, calls, K), np.uint32), "child_prior": np.zeros((n, calls, K), np.uint32),
    }
    for g, r in enumerate(res):
        for call, (_, _, pol, _, kids) in enumerate(r):
            assert len(pol) == len(kids)
            out["policies"][g, call, :len(pol)] = pol
            for j, (a, v, s, p) in enumerate(kids):
                out["child_action"][g, call, j], out["child_visits"][g, call, j] = a, v
                out["child_sum"][g, call, j], out["child_prior"][g, call, j] = s, p
    return out


def main():
    out = {}
    for name, shape, roots, sims, calls, wseed, evname in cases():
        t0 = time.perf_counter()
        res = run(name, shape, roots, sims, calls, wseed, evname)
        dt = time.perf_counter() - t0
        out.update({f"{name}_{k}": v for k, v in res.items()})
        print(f"case {name}: {len(roots)} games x {calls} calls x {sims} simulations, reference wall time {dt:.2f} s")
        if evname == "linear":
            value, logits = nev.linear_eval(nev.weights(shape, wseed), res["board"][0])
            tag = f"ev_{shape[0]}x{shape[1]}x{shape[2]}_{wseed}"
            out[f"{tag}_board"] = res["board"][0]
            out[f"{tag}_value_bits"] = np.uint32(f32_bits(value))
            out[f"{tag}_logits_crc"] = np.uint32(zlib.crc32(np.ascontiguousarray(logits, np.float32).tobytes()))
        if name == "A":  # the same run as numpy executes it: int64 rewards turn the sums float64
            t0 = time.perf_counter()
            res = run("A_numpy", shape, roots, sims, calls, wseed, evname, adapter=False)
            out.update({f"A_numpy_{k}": v for k, v in res.items()})
            print(f"case A_numpy: reference wall time {time.perf_counter() - t0:.2f} s")
    path = os.path.join(OUT, "search_nn.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
