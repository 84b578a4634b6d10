"""ctypes face of the TEST-ONLY host build of the 9x9x6 refill (refill_host.hip)."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from hostbuild import build  # noqa: E402

LIB = os.path.join(HERE, "librefill_host.so")
_lib = None
R = C = 9
NP, W = 7, 3


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def lib():
    global _lib
    if _lib is None:
        build(LIB, os.path.join(HERE, "refill_host.hip"), ["--offload-host-only", "-O1"])
        L = ctypes.CDLL(LIB)
        vp, i32, lg = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
        L.rf_refill.argtypes = [i32, i32, lg] + [vp] * 6
        L.rf_refill.restype = i32
        L.rf_step_refills.argtypes = [lg, vp, vp, vp, i32, vp]
        L.rf_step_refills.restype = i32
        L.rf_episode_refills.argtypes = [lg, vp, i32, i32, vp]
        L.rf_episode_refills.restype = lg
        _lib = L
    return _lib


def em_words(heights):
    """(n, 9) column heights -> (n, 3) words of the top-aligned hole set (cell (r, c) is bit 9 r + c)."""
    h = np.asarray(heights).reshape(-1, C)
    cells = (np.arange(R)[None, :, None] < h[:, None, :]).reshape(len(h), R * C)
    bits = np.zeros((len(h), 32 * W), np.uint64)
    bits[:, :R * C] = cells
    return (bits.reshape(len(h), W, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)


def refill(which, limit, heights, seeds, k0):
    """which: 'new' (refill) or 'loop' (refill_loop). Returns planes (n, 7, 3), k, overflow."""
    em = np.ascontiguousarray(em_words(heights))
    n = len(em)
    seeds = np.ascontiguousarray(np.broadcast_to(np.asarray(seeds, dtype=np.uint32), (n,)))
    k0 = np.ascontiguousarray(np.broadcast_to(np.asarray(k0, dtype=np.uint32), (n,)))
    planes = np.zeros((n, NP, W), np.uint32)
    k = np.zeros(n, np.uint32)
    ovf = np.zeros(n, np.uint32)
    rc = lib().rf_refill({"new": 0, "loop": 1}[which], int(limit), n, _p(em), _p(seeds), _p(k0), _p(planes), _p(k),
                         _p(ovf))
    assert rc == 0, rc
    return planes, k, ovf


def episode_refills(seeds, moves, cap=24):
    """Tiles of every refill of seeded episodes: (n, moves, cap), 0 = no such refill; and the steps redone."""
    seeds = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint32))
    need = np.zeros((len(seeds), moves, cap), np.uint32)
    redone = lib().rf_episode_refills(len(seeds), _p(seeds), int(moves), int(cap), _p(need))
    return need, int(redone)


def step_refills(boards, seeds, actions, cap=4):
    """Tiles of the first `cap` refills of one step per board: (n, cap), 0 = no such refill."""
    b = np.ascontiguousarray(np.asarray(boards).reshape(-1, R * C), dtype=np.int8)
    seeds = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint32))
    actions = np.ascontiguousarray(np.asarray(actions, dtype=np.int32))
    need = np.zeros((len(b), cap), np.uint32)
    assert lib().rf_step_refills(len(b), _p(b), _p(seeds), _p(actions), int(cap), _p(need)) == 0
    return need
