#!/usr/bin/env python3
"""Dead boards that never come alive: the dead-board shuffle's cap on the headline shapes.

    M3_REFERENCE=<reference checkout> python3 -B tests/golden/gen_golden_cycling.py

BoardV2.apply_action shuffles a settled board without a legal move until it has one
(boardv2.py:188-194), and every shuffle reseeds (boardFunctions.py:17): the same row permutation
again and again. A board that stays dead under every power of that permutation hangs the
reference; the kernels and the oracle stop after 1024 shuffles and flag M3_FLAG_SHUFFLE_CAP.
shuffle.npz has no such board at 9x9x6 or 16x16x8 (all of its rows terminate).

Search (oracle only): boards whose rows are one colour sequence of period 5 or 6 under 2..6
different cyclic shifts -- every row permutation of such a board is a board of the same kind -- that
are dead, with a swap that leaves them dead as action, kept if the oracle's apply_action at
shuffle_cap = 1024 ends with the cap flag. A minute per shape at most; a shape where the search
finds none is recorded with zero rows. The committed run: 9x9x6 16 hits among 1,710 dead boards
in 54 s; 16x16x8 none among 949 dead boards in 60 s.

Each hit is then confirmed with the REAL reference: apply_action does not return within a 3 s
alarm (as gen_golden.py's gen_shuffle records it). Only data is committed -- no reference source:
``cycling.npz`` holds board, seed, action and the oracle's capped result (next, reward, draws,
flags) per shape.
"""
from __future__ import annotations

import os
import signal
import sys
import time

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ["M3_REFERENCE"]
for p in (REF, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

from match3tile.boardConfig import BoardConfig  # noqa: E402
from match3tile.boardv2 import BoardV2  # noqa: E402
from oracle import FLAG_SHUFFLE_CAP, Oracle  # noqa: E402

SHAPES = [(9, 9, 6), (16, 16, 8)]
BUDGET_S = 60
KEEP = 16


class _Timeout(Exception):
    pass


def _alarm(signum, frame):
    raise _Timeout()


def reference_hangs(shape, board, seed, action) -> bool:
    R, C, T = shape
    cfg = BoardConfig(seed=int(seed), rows=R, columns=C, types=T)
    signal.signal(signal.SIGALRM, _alarm)
    signal.alarm(3)
    try:
        BoardV2(20, cfg, np.array(board, dtype=np.int64)).apply_action(int(action))
        signal.alarm(0)
        return False
    except _Timeout:
        return True


def search(shape, rng):
    R, C, T = shape
    o = Oracle(R, C, T, shuffle_cap=1024)
    hits, dead, t0 = [], 0, time.time()
    while time.time() - t0 < BUDGET_S and len(hits) < KEEP:
        p = int(rng.integers(5, 7))
        if p > T:
            continue
        base = rng.permutation(T)[:p] + 1
        shifts = rng.choice(p, size=int(rng.integers(2, 7)), replace=True)
        rowshift = rng.choice(shifts, size=R)
        board = np.array([[base[(c + s) % p] for c in range(C)] for s in rowshift], np.int32)
        if o.get_matches(board)[2] or o.legal_actions(board):
            continue
        dead += 1
        seed = int(rng.integers(1, 2**31))
        for action in rng.permutation(o.A)[:4]:
            nb, r, d, f = o.apply_action(board, seed, int(action), 20)
            if f & FLAG_SHUFFLE_CAP and reference_hangs(shape, board, seed, action):
                hits.append((board.astype(np.int8), seed, int(action), nb.astype(np.int8), r, d, f))
                break
    print(f"{R}x{C}x{T}: {dead} dead boards searched in {time.time() - t0:.0f} s, {len(hits)} reach the cap")
    return hits


def main():
    rng = np.random.default_rng(20240)
    out = {}
    for shape in SHAPES:
        R, C, T = shape
        hits = search(shape, rng)
        tag = f"{R}x{C}x{T}"
        out[f"board_{tag}"] = np.array([h[0] for h in hits], np.int8).reshape(-1, R, C)
        out[f"seed_{tag}"] = np.array([h[1] for h in hits], np.uint32)
        out[f"action_{tag}"] = np.array([h[2] for h in hits], np.int32)
        out[f"next_{tag}"] = np.array([h[3] for h in hits], np.int8).reshape(-1, R, C)
        out[f"reward_{tag}"] = np.array([h[4] for h in hits], np.int32)
        out[f"draws_{tag}"] = np.array([h[5] for h in hits], np.int32)
        out[f"flags_{tag}"] = np.array([h[6] for h in hits], np.int32)
    np.savez_compressed(os.path.join(HERE, "cycling.npz"), **out)


if __name__ == "__main__":
    main()
