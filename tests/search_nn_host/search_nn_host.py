"""ctypes face of the TEST-ONLY host build of the network-guided tree core (search_nn_host.hip), and the
driver that plays the kernels' rounds with the C oracle's step and a Python evaluator in between."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from hostbuild import build  # noqa: E402

LIB = os.path.join(HERE, "libsearch_nn_host.so")
_lib = None


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def lib():
    global _lib
    if _lib is None:
        build(LIB, os.path.join(HERE, "search_nn_host.hip"), ["--offload-host-only", "-O1"])
        L = ctypes.CDLL(LIB)
        vp, i32, lg, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float
        L.nh_create.argtypes, L.nh_create.restype = [lg, i32, i32, i32, i32], vp
        L.nh_destroy.argtypes, L.nh_destroy.restype = [vp], None
        L.nh_set_roots.argtypes, L.nh_set_roots.restype = [vp] * 7, None
        L.nh_fits.argtypes, L.nh_fits.restype = [vp, i32], i32
        L.nh_select.argtypes, L.nh_select.restype = [vp] * 4, None
        L.nh_attach.argtypes, L.nh_attach.restype = [vp] * 7, None
        L.nh_commit.argtypes, L.nh_commit.restype = [vp, vp, vp, i32], None
        L.nh_finish.argtypes, L.nh_finish.restype = [vp] * 10, None
        L.nh_advance.argtypes, L.nh_advance.restype = [vp] * 5, i32
        L.nh_nodes_used.argtypes, L.nh_nodes_used.restype = [vp, lg], i32
        L.nh_score.argtypes, L.nh_score.restype = [f32, i32, i32, f32, f32], f32
        L.nh_onehot_width.argtypes, L.nh_onehot_width.restype = [i32], i32
        L.nh_linear.argtypes, L.nh_linear.restype = [vp, vp, i32, i32, i32, vp, vp], None
        _lib = L
    return _lib


def actions_to_bits(actions, words):
    bits = np.zeros(words, np.uint32)
    for a in actions:
        bits[a // 32] |= np.uint32(1 << (a % 32))
    return bits


RESULT_KEYS = ("best_action", "value", "root_visits", "n_children", "child_action", "child_visits", "child_value_sum",
               "child_prior", "flags")


class HostSearchNN:
    """DeviceSearchNN's rounds on the host core. states: objects with array / cfg.seed / n_actions /
    reward; evaluator(boards int8 [n, R, C], need bool [n]) -> (values, logits), called once per batch.
    `record`: a list that receives the scenario (integers) asan_main replays."""

    def __init__(self, oracle, states, node_capacity, evaluator, record=None):
        self.o, self.n, self.cap = oracle, len(states), int(node_capacity)
        self.N, self.A = oracle.R * oracle.C, oracle.A
        self.AW = (self.A + 31) // 32
        self.h = lib().nh_create(self.n, self.cap, self.N, self.AW, self.A)
        self.ev, self.rec = evaluator, record
        self._rec([self.n, self.cap, self.N, self.AW, self.A])
        self.set_roots(states)

    def set_roots(self, states, evaluator=None):
        """nh_set_roots (again: the trees the object held are dropped), then the two construction batches."""
        assert len(states) == self.n
        if evaluator is not None:
            self.ev = evaluator
        oracle = self.o
        self.seeds = [int(s.cfg.seed) for s in states]
        boards = np.ascontiguousarray(np.stack([np.asarray(s.array).reshape(-1) for s in states]), dtype=np.int8)
        na = np.array([s.n_actions for s in states], np.int32)
        rew = np.array([s.reward for s in states], np.int32)
        legal = np.stack([actions_to_bits(oracle.legal_actions(np.asarray(s.array)), self.AW) for s in states])
        self._rec([1], boards, na, rew, legal)
        evb, need = np.zeros((self.n, self.N), np.int8), np.zeros(self.n, np.uint8)
        lib().nh_set_roots(self.h, _p(boards), _p(na), _p(rew), _p(legal), _p(evb), _p(need))
        self._feed(evb, need, 0)   # the roots' batch
        self._round(0)             # the construction's expansion

    def __del__(self):
        if getattr(self, "h", None):
            lib().nh_destroy(self.h)
            self.h = None

    def _rec(self, *parts):
        if self.rec is not None:
            for p in parts:
                self.rec.extend(int(x) for x in np.asarray(p).reshape(-1))

    def _feed(self, evb, need, backup):
        values, logits = self.ev(evb.reshape(self.n, self.o.R, self.o.C), need.astype(np.bool_))
        values = np.ascontiguousarray(values, np.float32).reshape(self.n)
        logits = np.ascontiguousarray(logits, np.float32).reshape(self.n, self.A)
        self._rec([3, backup], values.view(np.uint32), logits.view(np.uint32))
        lib().nh_commit(self.h, _p(values), _p(logits), backup)

    def _round(self, backup):
        n, N = self.n, self.N
        rows = np.zeros((n, N), np.int8)
        row_na, row_act = np.zeros(n, np.int32), np.zeros(n, np.int32)
        lib().nh_select(self.h, _p(rows), _p(row_na), _p(row_act))
        ob = np.zeros((n, N), np.int8)
        rew, fl = np.zeros(n, np.int32), np.ones(n, np.uint32)  # (flags 1: a terminal row)
        lg = np.zeros((n, self.AW), np.uint32)
        for g in range(n):
            if row_na[g] >= 1:
                nb, r, _, f = self.o.apply_action(rows[g].astype(np.int32).reshape(self.o.R, self.o.C), self.seeds[g],
                                                  int(row_act[g]), int(row_na[g]))
                legal = self.o.legal_actions(nb)
                if not legal:  # as k_apply: it samples the action after the step, and flags an empty set
                    f |= 0x08
                ob[g], rew[g], fl[g] = np.asarray(nb).reshape(-1), r, f
                lg[g] = actions_to_bits(legal, self.AW)
        evb, need = np.zeros((n, N), np.int8), np.zeros(n, np.uint8)
        self._rec([2], ob, rew, fl, lg)
        lib().nh_attach(self.h, _p(ob), _p(rew), _p(fl), _p(lg), _p(evb), _p(need))
        self._feed(evb, need, backup)

    def run(self, simulations):
        """Returns m3_search_nn_batch's code for the run's first batch (0, -7)."""
        rc = lib().nh_fits(self.h, int(simulations))
        self._rec([4 if rc == 0 else 7, simulations])
        if rc:
            return rc
        for _ in range(simulations):
            self._round(1)
        return 0

    def result(self):
        n, A = self.n, self.A
        out = dict(best_action=np.zeros(n, np.int32), value=np.zeros(n, np.int32), root_visits=np.zeros(n, np.int32),
                   n_children=np.zeros(n, np.int32), child_action=np.zeros((n, A), np.int32),
                   child_visits=np.zeros((n, A), np.int32), child_value_sum=np.zeros((n, A), np.float32),
                   child_prior=np.zeros((n, A), np.float32), flags=np.zeros(n, np.uint32))
        self._rec([5])
        lib().nh_finish(self.h, *[_p(out[k]) for k in RESULT_KEYS])
        return out

    def advance(self, actions):
        actions = np.ascontiguousarray(actions, np.int32)
        ob = np.zeros((self.n, self.N), np.int8)
        rew, na = np.zeros(self.n, np.int32), np.zeros(self.n, np.int32)
        self._rec([6], actions)
        bad = lib().nh_advance(self.h, _p(actions), _p(ob), _p(rew), _p(na))
        return bad, ob, rew, na

    def nodes_used(self, g=0):
        return lib().nh_nodes_used(self.h, g)


def result_lines(res):
    """The text asan_main prints for one result."""
    cs, cp = res["child_value_sum"].view(np.uint32), res["child_prior"].view(np.uint32)
    out = []
    for g in range(len(res["best_action"])):
        k = int(res["n_children"][g])
        kids = " ".join(f"{res['child_action'][g][j]}:{res['child_visits'][g][j]}:{cs[g][j]}:{cp[g][j]}" for j in range(k))
        out.append(f"{g} {res['best_action'][g]} {res['value'][g]} {res['root_visits'][g]} {k} {res['flags'][g]} {kids}"
                   .rstrip())
    return out
