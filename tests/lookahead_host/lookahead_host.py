"""ctypes face of the TEST-ONLY host build of the lookahead core (lookahead_host.hip)."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from hostbuild import build  # noqa: E402

LIB = os.path.join(HERE, "liblookahead_host.so")
_lib = None
CFG_ID = {(9, 9, 6): 0, (16, 16, 8): 1}
FRAME = 2  # any other shape with sides up to 16, in the 16 x 16 frame (lh_set_frame)


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def lib():
    global _lib
    if _lib is None:
        # -O0, as tests/hostcore (the frame instantiations optimise slowly on the host)
        build(LIB, os.path.join(HERE, "lookahead_host.hip"), ["-O0"])
        L = ctypes.CDLL(LIB)
        vp, i32, u32, u64, lg = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_long
        L.lh_lookahead.argtypes = [i32, i32, lg] + [vp] * 9
        L.lh_lookahead.restype = i32
        L.lh_key.argtypes, L.lh_key.restype = [ctypes.c_int32, i32], u64
        L.lh_key_reward.argtypes, L.lh_key_reward.restype = [u64], ctypes.c_int32
        L.lh_key_action.argtypes, L.lh_key_action.restype = [u64], ctypes.c_int32
        L.lh_find_board.argtypes, L.lh_find_board.restype = [vp, i32, u32], i32
        L.lh_kth_bit.argtypes, L.lh_kth_bit.restype = [vp, i32, u32], i32
        L.lh_fold.argtypes, L.lh_fold.restype = [i32, vp, vp], u64
        _lib = L
    return _lib


class LookaheadHost:
    def __init__(self, R=9, C=9, T=6):
        self.shape = (R, C, T)
        self.cfg = CFG_ID.get(self.shape, FRAME)
        self.N, self.A = R * C, R * (C - 1) * 2

    def _sel(self):
        if self.cfg == FRAME:
            assert lib().lh_set_frame(*self.shape) == 0, self.shape

    def gcap(self):
        self._sel()
        return lib().lh_gcap(self.cfg)

    def chain_limit(self):
        self._sel()
        return lib().lh_chain_limit(self.cfg)

    def lookahead(self, boards, seeds, n_actions, bpw=16):
        """The emulated wave: groups of bpw boards, rounds of 64 candidates. Returns the dict of
        m3_lookahead's outputs plus stats = (candidates, given up by the fast path, boards redone)."""
        b = np.ascontiguousarray(np.asarray(boards).reshape(-1, self.N), dtype=np.int8)
        n = len(b)
        seeds = np.ascontiguousarray(np.broadcast_to(np.asarray(seeds, dtype=np.uint32), (n,)))
        na = np.ascontiguousarray(np.broadcast_to(np.asarray(n_actions, dtype=np.int32), (n,)))
        best = np.full(n, -7, np.int32)
        rew = np.full(n, -7, np.int32)
        tab = np.full((n, self.A), -7, np.int32)
        draws = np.full(n, 7, np.uint32)
        flags = np.full(n, 7, np.uint32)
        stats = np.zeros(3, np.int64)
        self._sel()
        rc = lib().lh_lookahead(self.cfg, int(bpw), n, _p(b), _p(seeds), _p(na), _p(best), _p(rew), _p(tab),
                                _p(draws), _p(flags), _p(stats))
        assert rc == 0, rc
        return dict(best_action=best, best_reward=rew, values=tab, last_draws=draws, flags=flags,
                    stats=tuple(int(x) for x in stats))
