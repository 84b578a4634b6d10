"""ctypes face of the TEST-ONLY host build of the search-tree core (search_host.hip), and the driver
that plays the kernels' rounds with the C oracle's step and playout in between."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from hostbuild import build  # noqa: E402

LIB = os.path.join(HERE, "libsearch_host.so")
_lib = None


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def lib():
    global _lib
    if _lib is None:
        build(LIB, os.path.join(HERE, "search_host.hip"), ["--offload-host-only", "-O1"])
        L = ctypes.CDLL(LIB)
        vp, i32, lg = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
        L.sh_create.argtypes, L.sh_create.restype = [lg, i32, i32, i32, i32], vp
        L.sh_destroy.argtypes, L.sh_destroy.restype = [vp], None
        L.sh_set_roots.argtypes, L.sh_set_roots.restype = [vp] * 5, None
        L.sh_run_begin.argtypes, L.sh_run_begin.restype = [vp, i32], i32
        L.sh_select.argtypes, L.sh_select.restype = [vp] * 4, None
        L.sh_attach.argtypes, L.sh_attach.restype = [vp] * 7, None
        L.sh_backup.argtypes, L.sh_backup.restype = [vp] * 3, None
        L.sh_finish.argtypes, L.sh_finish.restype = [vp] * 9, None
        L.sh_advance.argtypes, L.sh_advance.restype = [vp] * 5, i32
        L.sh_nodes_used.argtypes, L.sh_nodes_used.restype = [vp, lg], i32
        L.sh_log_table.argtypes, L.sh_log_table.restype = [i32, vp], None
        L.sh_ucb1.argtypes, L.sh_ucb1.restype = [ctypes.c_longlong, i32, i32, ctypes.c_double], ctypes.c_double
        _lib = L
    return _lib


def actions_to_bits(actions, words):
    bits = np.zeros(words, np.uint32)
    for a in actions:
        bits[a // 32] |= np.uint32(1 << (a % 32))
    return bits


class HostSearch:
    """DeviceSearch's rounds on the host core. states: objects with array / cfg.seed / n_actions /
    reward (tests/test_mcts_cpu.OracleBoard); every result is what m3_search_result returns.
    `record`: a list that receives the scenario (integers) asan_main replays."""

    def __init__(self, oracle, states, node_capacity, record=None):
        self.o, self.n, self.cap = oracle, len(states), int(node_capacity)
        self.N, self.A = oracle.R * oracle.C, oracle.A
        self.AW = (self.A + 31) // 32
        self.h = lib().sh_create(self.n, self.cap, self.N, self.AW, self.A)
        self.rec = record
        self._rec([self.n, self.cap, self.N, self.AW, self.A])
        self.set_roots(states)

    def set_roots(self, states):
        """m3_search_set_roots: as many states as the object has games; the trees it held are dropped."""
        oracle = self.o
        assert len(states) == self.n
        self.seeds = [int(s.cfg.seed) for s in states]
        boards = np.ascontiguousarray(np.stack([np.asarray(s.array).reshape(-1) for s in states]), dtype=np.int8)
        na = np.array([s.n_actions for s in states], np.int32)
        rew = np.array([s.reward for s in states], np.int32)
        legal = np.stack([actions_to_bits(oracle.legal_actions(np.asarray(s.array)), self.AW) for s in states])
        self._rec([1], boards, na, rew, legal)
        lib().sh_set_roots(self.h, _p(boards), _p(na), _p(rew), _p(legal))
        self._round(None)  # MCTS.__init__'s expansion

    def __del__(self):
        if getattr(self, "h", None):
            lib().sh_destroy(self.h)
            self.h = None

    def _rec(self, *parts):
        if self.rec is not None:
            for p in parts:
                self.rec.extend(int(x) for x in np.asarray(p).reshape(-1))

    def _round(self, rseeds):
        n, N = self.n, self.N
        rows = np.zeros((n, N), np.int8)
        row_na, row_act = np.zeros(n, np.int32), np.zeros(n, np.int32)
        lib().sh_select(self.h, _p(rows), _p(row_na), _p(row_act))
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
        ro = np.zeros((n, N), np.int8)
        ro_na = np.zeros(n, np.int32)
        self._rec([2 if rseeds is None else 4], ob, rew, fl, lg)
        lib().sh_attach(self.h, _p(ob), _p(rew), _p(fl), _p(lg), _p(ro), _p(ro_na))
        if rseeds is None:
            return
        res = self.o.rollouts(ro.astype(np.int32), self.seeds, ro_na, rseeds, threads=1)
        gain, rfl = np.ascontiguousarray(res["gain"], np.int32), np.ascontiguousarray(res["flags"], np.uint32)
        self._rec(gain, rfl)
        lib().sh_backup(self.h, _p(gain), _p(rfl))

    def run(self, simulations, rollout_seeds):
        """rollout_seeds [simulations][n]. Returns m3_search_run's code (0, -6, -7)."""
        rc = lib().sh_run_begin(self.h, int(simulations))
        self._rec([3 if rc == 0 else 7, simulations])
        if rc:
            return rc
        for k in range(simulations):
            self._round(np.asarray(rollout_seeds[k], dtype=np.uint32))
        return 0

    def result(self):
        n, A = self.n, self.A
        out = dict(best_action=np.zeros(n, np.int32), value=np.zeros(n, np.int32), root_visits=np.zeros(n, np.int32),
                   n_children=np.zeros(n, np.int32), child_action=np.zeros((n, A), np.int32),
                   child_visits=np.zeros((n, A), np.int32), child_reward=np.zeros((n, A), np.int64),
                   flags=np.zeros(n, np.uint32))
        self._rec([5])
        lib().sh_finish(self.h, *[_p(out[k]) for k in ("best_action", "value", "root_visits", "n_children",
                                                       "child_action", "child_visits", "child_reward", "flags")])
        return out

    def advance(self, actions):
        actions = np.ascontiguousarray(actions, np.int32)
        ob = np.zeros((self.n, self.N), np.int8)
        rew, na = np.zeros(self.n, np.int32), np.zeros(self.n, np.int32)
        self._rec([6], actions)
        bad = lib().sh_advance(self.h, _p(actions), _p(ob), _p(rew), _p(na))
        return bad, ob, rew, na

    def nodes_used(self, g=0):
        return lib().sh_nodes_used(self.h, g)


def result_lines(res):
    """The text asan_main prints for one m3_search_result."""
    out = []
    for g in range(len(res["best_action"])):
        k = int(res["n_children"][g])
        kids = " ".join(f"{res['child_action'][g][j]}:{res['child_visits'][g][j]}:{res['child_reward'][g][j]}"
                        for j in range(k))
        out.append(f"{g} {res['best_action'][g]} {res['value'][g]} {res['root_visits'][g]} {k} {res['flags'][g]} {kids}"
                   .rstrip())
    return out
