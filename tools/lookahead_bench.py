#!/usr/bin/env python3
"""Device one-ply lookahead against what the library offered before it, on the same states.

    python3 tools/lookahead_bench.py [--out lookahead_bench.json] [--label "bpw 32 / 8"]

Two paths, one process, alternating, after a warm-up, five repeats each:
  device    m3_lookahead_device on device-resident boards / seeds / n_actions (best action and best
            reward out; a second row adds the [n][A] table), HIP events around it (m3_ctx_timer);
  baseline  the host loop of samplers.greedy_actions at array level: m3_legal_actions to the host,
            every board replicated once per legal action, ONE m3_apply_actions call over the
            expanded list, first maximum per board in numpy -- host clock around the whole of it,
            and around its two synchronising library calls alone.
States: 65,536 boards of 9x9x6 and 16,384 of 16x16x8, mid-game (seven seeded random moves into
20-move episodes, played on the device). Both paths must pick the same actions.
M3_LIB selects an A/B build of the library (make variant-fast ...); --label names the row.
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
from match3tile._native import check, lib, ptr  # noqa: E402
from match3tile.batched import BatchedMatch3Env  # noqa: E402

SIZES = (((9, 9, 6), 65536), ((16, 16, 8), 16384))
REPEATS, WARM = 5, 2


def mid_game(shape, n, depth=7):
    env = BatchedMatch3Env(n, *shape, num_moves=20, env_goal=2**31 - 1, autoreset=False)
    for _ in range(depth):
        env.step()
    out = env.observations().reshape(n, -1), env.seeds(), (20 - env.moves()).astype(np.int32)
    env.close()
    return out


def baseline(ctx, boards, seeds, n_act):
    """(picks, seconds inside the two library calls, candidates)"""
    n = len(boards)
    bits = np.empty((n, ctx.words), np.uint32)
    t0 = time.perf_counter()
    check(lib().m3_legal_actions(ctx.handle, n, ptr(boards), ptr(bits)))
    t1 = time.perf_counter()
    legal = np.unpackbits(bits.view(np.uint8), axis=1, bitorder="little")[:, :ctx.A].astype(bool)
    owner, acts = np.nonzero(legal)
    counts = legal.sum(axis=1)
    assert counts.min() > 0
    m = len(owner)
    xb, xs, xn = np.ascontiguousarray(boards[owner]), np.ascontiguousarray(seeds[owner]), np.ascontiguousarray(n_act[owner])
    xa = np.ascontiguousarray(acts, dtype=np.int32)
    ob, orw, od, of = np.empty_like(xb), np.empty(m, np.int32), np.empty(m, np.uint32), np.empty(m, np.uint32)
    t2 = time.perf_counter()
    check(lib().m3_apply_actions(ctx.handle, m, ptr(xb), ptr(xs), ptr(xn), ptr(xa), ptr(ob), ptr(orw), ptr(od),
                                 ptr(of), None, None))
    t3 = time.perf_counter()
    start = np.concatenate([[0], np.cumsum(counts)[:-1]])
    best = np.maximum.reduceat(orw, start)
    first = np.full(n, m, np.int64)
    hit = np.flatnonzero(orw == best[owner])
    np.minimum.at(first, owner[hit], hit)
    return xa[first], (t1 - t0) + (t3 - t2), m


def spread(xs):
    xs = np.asarray(xs, float)
    return {"median": float(np.median(xs)), "min": float(xs.min()), "max": float(xs.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="default")
    ap.add_argument("--device-only", action="store_true", help="A/B rows of library variants: skip the baseline")
    a = ap.parse_args()
    rows = []
    for shape, n in SIZES:
        boards, seeds, n_act = mid_game(shape, n)
        assert (boards > 0).all()
        ctx = _native.Context(*shape)
        d_b, d_s, d_na = ctx.device_array(boards), ctx.device_array(seeds), ctx.device_array(n_act)
        d_a, d_r, d_v = ctx.device_empty(4 * n), ctx.device_empty(4 * n), ctx.device_empty(4 * n * ctx.A)

        def device(table):
            ms = np.zeros(1, np.float32)
            check(lib().m3_ctx_timer(ctx.handle, 0, None))
            check(lib().m3_lookahead_device(ctx.handle, n, d_b.ptr, d_s.ptr, d_na.ptr, d_a.ptr, d_r.ptr,
                                            d_v.ptr if table else None, None, None))
            check(lib().m3_ctx_timer(ctx.handle, 1, ptr(ms)))
            return float(ms[0]) * 1e-3

        dev, dev_tab, base, base_calls = [], [], [], []
        cands = None
        for it in range(WARM + REPEATS):
            td, tt = device(False), device(True)
            if not a.device_only:
                t0 = time.perf_counter()
                picks, in_calls, cands = baseline(ctx, boards, seeds, n_act)
                tb = time.perf_counter() - t0
                got = d_a.to_host(np.int32, (n,))
                assert (got == picks).all(), "device and baseline picks differ"
            if it >= WARM:
                dev.append(td)
                dev_tab.append(tt)
                if not a.device_only:
                    base.append(tb)
                    base_calls.append(in_calls)
        if cands is None:
            cands = int((d_v.to_host(np.int32, (n, ctx.A)) >= 0).sum())
        row = {"shape": "x".join(map(str, shape)), "boards": n, "candidates": int(cands), "label": a.label,
               "device_s": spread(dev), "device_with_table_s": spread(dev_tab),
               "device_boards_per_s": n / float(np.median(dev)), "device_candidates_per_s": cands / float(np.median(dev))}
        if not a.device_only:
            row.update({"baseline_s": spread(base), "baseline_library_calls_s": spread(base_calls),
                        "baseline_boards_per_s": n / float(np.median(base)),
                        "baseline_candidates_per_s": cands / float(np.median(base)),
                        "speedup_vs_baseline": float(np.median(base) / np.median(dev)),
                        "speedup_vs_baseline_library_calls": float(np.median(base_calls) / np.median(dev))})
        rows.append(row)
        for d in (d_b, d_s, d_na, d_a, d_r, d_v):
            d.free()
        ctx.close()
    out = {"what": "one-ply lookahead, device vs host-expanded baseline, MI355X (tools/lookahead_bench.py)",
           "repeats": REPEATS, "warmup": WARM, "lib": os.environ.get("M3_LIB", "build/libm3.so"), "rows": rows}
    s = json.dumps(out, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s)


if __name__ == "__main__":
    main()
