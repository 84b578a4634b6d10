#!/usr/bin/env python3
"""Simulations per second of the network-guided device trees, beside the UCB1 rollout trees.

    python3 tools/search_nn_rate.py [--games 4096] [--simulations 100] [--repeats 5] [--out FILE.json]

Two searches over the same roots (9x9x6 reset boards of seeds 1..games, 20 moves left):
  nn_linear   DeviceSearchNN(weights=...): prior-weighted trees, every batch evaluated on the device by
              the built-in linear evaluator, a whole run enqueued without a host round trip;
  rollout     DeviceSearch: UCB1 trees with one random playout per simulation.
They answer different questions (a playout of up to 20 steps against one evaluation), so the two figures
are context for each other, not a race. Host clock around run + result(children=False), which ends in
a blocking download; the trees are built (roots set, construction done, stream idle) before the clock
starts. One warm-up run of each path at the timed size first, then --repeats timed runs, the two paths
alternating. simulations/s = games x simulations / seconds; median, min and max are printed.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "element-crush-gym_amd"))

import numpy as np  # noqa: E402

from match3tile import _native  # noqa: E402
from match3tile.boardConfig import BoardConfig  # noqa: E402
from match3tile.boardv2 import BoardV2  # noqa: E402
from match3tile.search import DeviceSearch, DeviceSearchNN, onehot_width  # noqa: E402

MOVES = 20


def timed(make, run):
    ds = make()
    ds.result(children=False)  # (blocks: the construction is done before the clock starts)
    t0 = time.perf_counter()
    run(ds)
    ds.result(children=False)
    dt = time.perf_counter() - t0
    st = ds.stats()
    ds.close()
    return dt, st


def spread(xs):
    xs = np.asarray(xs, float)
    return {"median": float(np.median(xs)), "min": float(xs.min()), "max": float(xs.max()), "repeats": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--simulations", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if _native.device_count() == 0:
        sys.exit("search_nn_rate.py needs the GPU")
    n, sims = a.games, a.simulations
    roots = [BoardV2(MOVES, BoardConfig(seed=s)) for s in range(1, n + 1)]
    W = np.random.RandomState(1).standard_normal((81, onehot_width(6), 145)).astype(np.float32)
    seeds = np.random.default_rng(n).integers(0, 2**31 - 1, (sims, n)).astype(np.uint32)
    paths = {
        "nn_linear": (lambda: DeviceSearchNN(roots, sims, weights=W, node_capacity=2 + sims), lambda ds: ds.run()),
        "rollout": (lambda: DeviceSearch(roots, sims, node_capacity=2 + sims), lambda ds: ds.run(seeds)),
    }
    times = {p: [] for p in paths}
    stats = {}
    for rep in range(a.repeats + 1):  # (the first pass is the warm-up: code objects, staging, allocations)
        for p, (make, run) in paths.items():
            dt, st = timed(make, run)
            print(f"# {'warm-up' if rep == 0 else 'repeat ' + str(rep)} {p}: {dt:.4f} s", file=sys.stderr, flush=True)
            if rep:
                times[p].append(dt)
                stats[p] = st
    out = {"what": "simulations/s, network-guided trees (device linear evaluator) beside UCB1 rollout trees, MI355X "
                   "(tools/search_nn_rate.py)",
           "shape": "9x9x6", "games": n, "moves_left": MOVES, "simulations": sims}
    for p in paths:
        out[p + "_s"] = spread(times[p])
        out[p + "_simulations_per_s"] = n * sims / out[p + "_s"]["median"]
        out[p + "_stats"] = stats[p]
    s = json.dumps(out, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s)


if __name__ == "__main__":
    main()
