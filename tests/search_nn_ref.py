"""Expected side of the network-guided device trees (``m3_search_nn_*``, ``DeviceSearchNN``): a Python
model written from the semantics of include/m3.h and DESIGN.md §4.9 -- not from the library's code --
over the C oracle's step (``search_ref.FreezingBoard``), with ``np.float32`` arithmetic, ``math.log``
and ``math.sqrt``. Values are compared as bit patterns. The model itself is held to the reference's own
tree code by tests/test_search_nn_golden_cpu.py (tests/golden/search_nn.npz); it stays the expected
side where the reference raises or never returns: frozen games (case G) and evaluations that are not
finite (cases H, P, Q, R). The evaluators live in tests/nn_evaluators.py and are re-exported here.

An evaluator here is ``ev(board[R, C], game, round) -> (value f32, logits f32[A])``; round 0 is the
roots' batch, round 1 the construction's expansion, round 2 + k simulation k since the roots were set.
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "element-crush-gym_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import search_ref  # noqa: E402
from nn_evaluators import constant_ev, linear_eval, negative_ev, onehot_width, weights  # noqa: E402,F401
from search_ref import F_NO_LEGAL, Freeze  # noqa: E402

F_BAD_EVAL = 0x400
f32 = np.float32
INF = f32(np.inf)


def bits(x):
    return int(np.asarray(x, dtype=np.float32).reshape(()).view(np.uint32))


def linear_evaluator(W):
    return lambda board, game, rnd: linear_eval(W, board)


def batch_evaluator(ev, n, A, first_round=0):
    """``ev`` as DeviceSearchNN's host evaluator: called once per batch, counts the rounds itself. Rows
    without need are filled with NaN: the library must not read them."""
    state = dict(round=first_round, calls=0)

    def run(boards, need):
        values, logits = np.full(n, np.nan, np.float32), np.full((n, A), np.nan, np.float32)
        for g in range(n):
            if need[g]:
                values[g], logits[g] = ev(boards[g], g, state["round"])
        state["round"] += 1
        state["calls"] += 1
        return values, logits
    run.state = state
    return run


def score(total, visits, parent_visits, c, prior):
    """The score of a child, float32 with every operation rounded on its own."""
    if visits == 0:
        return INF
    with np.errstate(all="ignore"):
        mean = f32(total) / f32(visits)
        e = f32(math.sqrt(math.log(parent_visits) / (1 + visits)))
        w = f32(c) * f32(prior)
        return mean + w * e


class BadEval(Exception):
    pass


class NNNode:
    def __init__(self, state, ev, parent=None, policy=1.0):
        self.state, self.parent, self.children = state.clone(), parent, {}
        self.visits, self.total, self.policy = 0, f32(0.0), f32(policy)
        self.untried = list(state.legal_actions) if not state.is_terminal else []
        self.value, self.logits = None, None
        if not state.is_terminal:  # one evaluation serves the node's priors and its rollout value
            value, logits = ev(state.array)
            value, logits = f32(value), np.asarray(logits, np.float32)
            if not np.isfinite(value) or not all(np.isfinite(logits[a]) for a in self.untried):
                raise BadEval()
            self.value, self.logits = value, logits

    @property
    def fully_expanded(self):
        return not self.untried

    def expand(self, ev):
        action = self.untried.pop()  # the highest untried legal id (IndexError: none)
        child = NNNode(self.state.apply_action(action), ev, self, self.logits[action])
        self.children[action] = child
        return child

    def best_child(self, c):
        best, bv = None, None
        for ch in self.children.values():
            v = score(ch.total, ch.visits, self.visits, c, ch.policy)
            if best is None or v > bv:
                best, bv = ch, v
        if best is None:
            raise IndexError("no children")
        return best


class NNSearch:
    """One game. ev(board, round). Freezes as the library does; `frozen` then holds the result dict."""

    def __init__(self, state, ev):
        self.round, self.frozen, self.root = 0, None, None
        self._ev = lambda board: ev(board, self.round)
        self.terminal_root = state.is_terminal
        self.root_reward = state.reward
        self.sim_count = 0
        self._guard(self._construct, state)

    def _construct(self, state):
        self.root = NNNode(state, self._ev)
        self.round = 1
        if not state.is_terminal:
            self.root.expand(self._ev)

    def _guard(self, fn, *args):
        fl = 0
        try:
            fn(*args)
        except Freeze as e:
            fl = e.flags
        except IndexError:
            fl = F_NO_LEGAL
        except BadEval:
            fl = F_BAD_EVAL
        if fl:
            self.frozen = dict(children=self._children(), root_visits=self.root.visits if self.root else 0, flags=fl)

    def _children(self):
        if self.root is None:
            return []
        return [(a, ch.visits, bits(ch.total), bits(ch.policy)) for a, ch in self.root.children.items()]

    def _simulate(self):
        node = self.root
        while not node.state.is_terminal and node.fully_expanded:
            node = node.best_child(node.state.n_actions)
        if not node.state.is_terminal:
            node = node.expand(self._ev)
        ret = f32(node.state.reward) if node.state.is_terminal else node.value
        while node is not None:
            node.visits += 1
            node.total = f32(node.total + ret)
            node = node.parent

    def simulate(self, rnd):
        self.round = rnd
        if self.frozen is None:
            self._guard(self._simulate)

    def result(self):
        if self.frozen is not None:
            return self.frozen
        root = self.root
        res = dict(children=self._children(), root_visits=root.visits, flags=0)
        if self.terminal_root:
            res.update(action=-1, value=int(root.state.reward), policies=[])
            return res
        best_a, best = None, None
        for a, ch in root.children.items():
            if best is None or ch.visits > best.visits:
                best_a, best = a, ch
        node = root
        try:
            while not node.state.is_terminal and node.fully_expanded:
                node = node.best_child(0)
        except IndexError:
            self.frozen = dict(children=res["children"], root_visits=root.visits, flags=F_NO_LEGAL)
            return self.frozen
        res.update(action=best_a, value=int(node.state.reward),
                   policies=[ch.visits / root.visits for ch in root.children.values()])
        return res

    def advance(self, action):
        if self.frozen is None and not self.terminal_root:
            self.root = self.root.children[action]
            self.root.parent = None


_cache = {}


def run_case(key, shape, roots, sims, calls, ev):
    """roots: search_ref root dicts. ev(board, game, round). Returns want[game][call]; cached by `key`."""
    if key in _cache:
        return _cache[key]
    want = []
    for g, r in enumerate(roots):
        st = search_ref.state(shape, r["board"], r["seed"], r["n_actions"], r["reward"])
        s = NNSearch(st, lambda board, rnd, g=g: ev(board, g, rnd))
        out, rnd = [], 2
        for _ in range(calls):
            for _ in range(sims):
                s.simulate(rnd)
                rnd += 1
            res = s.result()
            out.append(res)
            if not res["flags"] and res.get("action", -1) >= 0:
                s.advance(res["action"])
        want.append(out)
    _cache[key] = want
    return want


def assert_game(res, g, want, tag=""):
    """res: the arrays of m3_search_nn_result (or the host core's); want: one call of one game."""
    k = len(want["children"])
    assert int(res["flags"][g]) == want["flags"], (tag, g, hex(int(res["flags"][g])), hex(want["flags"]))
    assert res["root_visits"][g] == want["root_visits"], (tag, g)
    assert res["n_children"][g] == k, (tag, g)
    cs, cp = res["child_value_sum"].view(np.uint32), res["child_prior"].view(np.uint32)
    got = [(int(res["child_action"][g][j]), int(res["child_visits"][g][j]), int(cs[g][j]), int(cp[g][j])) for j in range(k)]
    assert got == [tuple(int(x) for x in c) for c in want["children"]], (tag, g, got, want["children"])
    if want["flags"]:
        return
    assert res["best_action"][g] == want["action"], (tag, g)
    assert res["value"][g] == want["value"], (tag, g)
    rv = int(res["root_visits"][g])
    assert [int(res["child_visits"][g][j]) / rv for j in range(k)] == list(want["policies"]), (tag, g)


# ---- the cases the CPU and the GPU tests share -------------------------------------------------
def case_a():
    """9x9x6, 18 games, n_actions 4, 20 simulations, 3 calls, the linear evaluator of RandomState(1)."""
    shape = (9, 9, 6)
    roots = search_ref.reset_roots(range(601, 619), 4)
    W = weights(shape, 1)
    return dict(shape=shape, roots=roots, sims=20, calls=3, W=W, ev=linear_evaluator(W),
                want=run_case("A", shape, roots, 20, 3, linear_evaluator(W)))


def case_c():
    shape = (16, 16, 8)
    roots = search_ref.reset_roots(range(701, 705), 5)
    W = weights(shape, 3)
    return dict(shape=shape, roots=roots, sims=12, calls=1, W=W, ev=linear_evaluator(W),
                want=run_case("C", shape, roots, 12, 1, linear_evaluator(W)))


def case_d(seeds):
    shape = (7, 5, 4)
    roots = search_ref.reset_roots(seeds, 5)
    W = weights(shape, 4)
    return dict(shape=shape, roots=roots, sims=12, calls=1, W=W, ev=linear_evaluator(W),
                want=run_case(("D", tuple(seeds)), shape, roots, 12, 1, linear_evaluator(W)))


def case_e():
    shape = (9, 9, 6)
    roots = search_ref.reset_roots(range(801, 817), 2)
    W = weights(shape, 5)
    return dict(shape=shape, roots=roots, sims=40, calls=2, W=W, ev=linear_evaluator(W),
                want=run_case("E", shape, roots, 40, 2, linear_evaluator(W)))


def case_f(which):
    shape = (9, 9, 6)
    roots = search_ref.reset_roots(range(901, 909), 3)
    ev = constant_ev if which == "constant" else negative_ev
    return dict(shape=shape, roots=roots, sims=40, calls=2, ev=ev, want=run_case(("F", which), shape, roots, 40, 2, ev))


def case_g():
    """The freezing roots of search_ref.freeze_case(): 5x5x6, 64 games, 6 moves, 12 simulations."""
    shape = (5, 5, 6)
    roots = search_ref.reset_roots(range(1, 65), 6)
    W = weights(shape, 7)
    return dict(shape=shape, roots=roots, sims=12, calls=2, W=W, ev=linear_evaluator(W),
                want=run_case("G", shape, roots, 12, 2, linear_evaluator(W)))


H_GAME, H_ROUND = 7, 2 + 4  # the fifth simulation round


def case_h():
    a = case_a()
    base = a["ev"]

    def ev(board, game, rnd):
        value, logits = base(board, game, rnd)
        return (f32(np.nan), logits) if (game == H_GAME and rnd == H_ROUND) else (value, logits)
    return dict(a, ev=ev, want=run_case("H", a["shape"], a["roots"], a["sims"], a["calls"], ev))


# ---- non-finite logits: cases P (one poisoned legal logit per game), Q (every illegal logit) and R
# (an infinite weight of the linear evaluator), all on the roots of case A --------------------------
NAN, FLT_MAX, DENORMAL = f32(np.nan), np.finfo(np.float32).max, f32(1e-45)


def trace_case_a():
    """The clean run of case A again, with every evaluation written down:
    {(game, round): (board, legal ids ascending)}. The model's own record: nothing of the library."""
    if "A-trace" in _cache:
        return _cache["A-trace"][1]
    a = case_a()
    o = search_ref.capped_oracle(a["shape"])
    trace = {}

    def ev(board, game, rnd):
        assert (game, rnd) not in trace
        trace[(game, rnd)] = (np.array(board, np.int32), sorted(int(x) for x in o.legal_actions(np.array(board, np.int32))))
        return a["ev"](board, game, rnd)
    want = run_case("A-trace-run", a["shape"], a["roots"], a["sims"], a["calls"], ev)
    assert want == a["want"]
    _cache["A-trace"] = (want, trace)
    return trace


def _first(pred):
    return lambda legal: next((x for x in legal if pred(x)), None)


# kind: (rounds searched, games searched, the legal id poisoned, the value written, freezes)
_SIMS_A, _CALLS_A = 20, 3
POISON_KINDS = {
    "nan_lowest": (range(2 + 4, 2 + _SIMS_A), range(18), lambda legal: legal[0], NAN, True),
    "pinf_highest": (range(2 + _SIMS_A + 2, 2 + 2 * _SIMS_A), range(18), lambda legal: legal[-1], INF, True),  # in call 1
    "ninf_ge128": (range(2 + 2, 2 + _SIMS_A), range(18), _first(lambda x: x >= 128), -INF, True),
    "nan_mod31": (range(2 + 5, 2 + _SIMS_A * _CALLS_A), range(18), _first(lambda x: x % 32 == 31), NAN, True),
    "nan_mod0": (range(2 + 7, 2 + _SIMS_A * _CALLS_A), range(18), _first(lambda x: x % 32 == 0), NAN, True),
    "nan_roots": ([0], range(16, -1, -1), lambda legal: legal[len(legal) // 2], NAN, True),      # (the ragged workgroup)
    "ninf_construction": ([1], range(17, -1, -1), lambda legal: legal[0], -INF, True),
    "fltmax": ([0], range(18), lambda legal: legal[-1], FLT_MAX, False),       # the root's highest legal id: the first
    "denormal": ([0], range(18), lambda legal: legal[-1], DENORMAL, False),    # child's prior, read in every selection
}


def pick_poisons():
    """{kind: (game, round, id, value)}: for every kind the first game (one game per kind) and round of
    the clean run whose evaluated node has such a legal id. A kind without one is missing."""
    trace, taken, out = trace_case_a(), set(), {}
    for kind, (rounds, games, pick, value, _) in POISON_KINDS.items():
        for g in games:
            hit = next(((rnd, pick(trace[(g, rnd)][1])) for rnd in rounds
                        if (g, rnd) in trace and trace[(g, rnd)][1] and pick(trace[(g, rnd)][1]) is not None), None)
            if g not in taken and hit is not None:
                out[kind] = (g, hit[0], hit[1], value)
                taken.add(g)
                break
    return out


def case_p():
    """Case A with one legal logit of one evaluated row poisoned in each of nine games."""
    a, poisons = case_a(), pick_poisons()
    at = {(g, rnd): (i, v) for g, rnd, i, v in poisons.values()}

    def ev(board, game, rnd):
        value, logits = a["ev"](board, game, rnd)
        if (game, rnd) in at:
            logits = logits.copy()
            logits[at[(game, rnd)][0]] = at[(game, rnd)][1]
        return value, logits
    return dict(a, ev=ev, poisons=poisons, want=run_case("P", a["shape"], a["roots"], a["sims"], a["calls"], ev))


def case_q():
    """Case A with NaN, +inf and -inf written to every illegal id of every evaluated row: never read."""
    a = case_a()
    o = search_ref.capped_oracle(a["shape"])
    junk = np.array([NAN, INF, -INF], np.float32)

    def ev(board, game, rnd):
        value, logits = a["ev"](board, game, rnd)
        legal = set(int(x) for x in o.legal_actions(np.array(board, np.int32)))
        illegal = np.array([i for i in range(len(logits)) if i not in legal])
        logits = logits.copy()
        logits[illegal] = junk[(illegal + game + rnd) % 3]
        return value, logits
    return dict(a, ev=ev, want=run_case("Q", a["shape"], a["roots"], a["sims"], a["calls"], ev))


def pick_infinite_weight():
    """(cell, cell value, logit id, games frozen, games hit only where the id is illegal, games never hit)
    for W[cell][value][id] = +inf: the first choice, from the clean run's record, that freezes some
    games, leaves some whose boards hit the weight only where the id is illegal, and misses some."""
    trace = trace_case_a()
    for cell in (72, 76, 80, 36, 40, 44, 0):
        for x in range(1, 7):
            hits = [(g, legal) for (g, _), (board, legal) in trace.items() if board.reshape(-1)[cell] == x]
            hit_games = {g for g, _ in hits}
            for j in range(144):
                frozen = {g for g, legal in hits if j in legal}
                if 3 <= len(frozen) <= 12 and len(hit_games - frozen) >= 2 and 18 - len(hit_games) >= 2:
                    return cell, x, j, sorted(frozen), sorted(hit_games - frozen), sorted(set(range(18)) - hit_games)
    return None


def case_r():
    """Case A with one weight of the linear evaluator +inf: the device's own evaluator produces the
    infinite logit (and NaN where the sum goes on to add -inf: it does not here, one weight only)."""
    a = case_a()
    cell, x, j = pick_infinite_weight()[:3]
    W = a["W"].copy()
    W[cell, x, j] = INF
    ev = linear_evaluator(W)
    return dict(a, W=W, ev=ev, want=run_case("R", a["shape"], a["roots"], a["sims"], a["calls"], ev))
