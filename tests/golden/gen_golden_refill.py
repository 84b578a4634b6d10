"""Writes tests/golden/refill.npz: 9x9x6 boards whose first move clears a chosen number of cells,
for the refill sizes around the 32-tile stream of the two-part refill (m3_rules.hpp refill): exactly
32, 33 and all 81, and some sizes next to them.

Reset boards with a bomb + bomb, bomb + line, line + line or mega + mega pair under the swap and a
few more line specials and bombs sprinkled on, kept when the host build of the rule code
(tests/refill_host) reports a first refill of a wanted size. Data only: boards, seeds, actions and
that size (`need`); tests/test_refill_cpu.py pins `need` to the rule code, tests/test_gpu_refill.py
plays the rows on the device against the oracle.

    python tests/golden/gen_golden_refill.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests", "refill_host"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import crafted  # noqa: E402
import refill_host as rf  # noqa: E402
from oracle import Oracle  # noqa: E402

WANT = {30: 20, 31: 40, 32: 100, 33: 100, 34: 40, 36: 20, 81: 60}  # first refill size: rows at most
BATCHES = 6


def main():
    o = Oracle(9, 9, 6)
    cfg = o.cfg
    dec = crafted.decode_table(o)
    rng = np.random.default_rng(81)
    base = [o.init_board(s)[0].astype(np.int8) for s in range(1, 65)]
    pairs = [(cfg.B, cfg.B), (cfg.B, cfg.H), (cfg.B, cfg.V), (cfg.H, cfg.V), (cfg.M, cfg.M)]
    kept = {k: [] for k in WANT}

    def token(t):  # line specials carry a tile type
        return int(t) | int(rng.integers(1, 7)) if t in (cfg.H, cfg.V) else int(t)

    for _ in range(BATCHES):
        n = 20000
        boards = np.stack([base[i] for i in rng.integers(0, len(base), n)])
        actions = rng.integers(0, o.A, n).astype(np.int32)
        seeds = rng.integers(1, 2**32, n, dtype=np.uint64).astype(np.uint32)
        for i in range(n):
            sr, sc, tr, tc = dec[actions[i]]
            a, b = pairs[int(rng.integers(0, len(pairs)))]
            boards[i, sr, sc], boards[i, tr, tc] = token(a), token(b)
            for _ in range(int(rng.integers(0, 6))):
                r, c = (int(x) for x in rng.integers(0, 9, 2))
                if (r, c) in ((sr, sc), (tr, tc)):
                    continue
                u = rng.random()
                boards[i, r, c] = cfg.B if u > 0.9 else (int(boards[i, r, c]) & cfg.TM) | (cfg.H if u < 0.45 else cfg.V)
        need = rf.step_refills(boards, seeds, actions, cap=1)[:, 0]
        for k in WANT:
            for i in np.flatnonzero(need == k)[:WANT[k] - len(kept[k])]:
                kept[k].append((boards[i].copy(), seeds[i], actions[i], k))
    assert all(kept[k] for k in (32, 33, 81)), {k: len(kept[k]) for k in WANT}
    rows = [r for k in WANT for r in kept[k]]
    np.savez_compressed(os.path.join(HERE, "refill.npz"),
                        boards=np.array([r[0] for r in rows], np.int8), seeds=np.array([r[1] for r in rows], np.uint32),
                        actions=np.array([r[2] for r in rows], np.int32), need=np.array([r[3] for r in rows], np.int32))
    print({k: len(kept[k]) for k in WANT})


if __name__ == "__main__":
    main()
