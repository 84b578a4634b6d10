#!/usr/bin/env python3
"""Throughput of the policy/value network on the device, beside torch on the same card.

    python3 tools/net_bench.py [--boards 4096] [--repeats 5] [--search-simulations 50] [--out profiles/net_bench.json]

For (layers, features) = (4, 64), (10, 128), (40, 256) on `--boards` boards of 9x9x6:
  evaluations_per_s   boards / device time of one m3_net_forward_device (HIP events on the context stream,
                      m3_ctx_timer), median of --repeats after one warm-up call;
  tower_share         1 - t(the same net with layers = 0) / t: the stem and the heads are what a net without
                      a tower runs, so the difference is the tower convolutions' time (events, not a trace);
  tower_tflops, tower_fraction_of_peak
                      2 * positions * 9 F * F * 2 layers FLOP over that tower time, and over the 2.5 PFLOP/s
                      dense bf16 MFMA peak of the MI355X (spec): compute-bound by count, so the FLOP bound is
                      the one named;
  torch_*             the same stack (one-hot, 3x3 convs with folded BN as bias, ReLU, residual adds, the two
                      heads) in torch, bf16 and channels_last, random weights, timed with torch events in a
                      CHILD process (`--torch-child`), the yardstick. torch's forward is not compared for
                      results here (tests/net_torch_ref.py does that on the CPU in float64).
And simulations/s of a `--boards`-game guided search (DeviceSearchNN) with the (4, 64) net beside the
built-in linear evaluator's: host clock around run + result(children=False), which blocks.
A run without a GPU fails; nothing here falls back.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "element-crush-gym_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

CONFIGS = [(4, 64), (10, 128), (40, 256)]
SHAPE = (9, 9, 6)
PEAK_BF16 = 2.5e15  # dense bf16 MFMA, MI355X spec


def spread(xs):
    xs = np.asarray(xs, float)
    return {"median": float(np.median(xs)), "min": float(xs.min()), "max": float(xs.max()), "repeats": len(xs)}


def tower_flop(n, layers, F):
    return 2.0 * n * 81 * 9 * F * F * 2 * layers


def torch_child(n, repeats):
    """Prints one JSON line: ms per forward for every configuration."""
    import torch
    import torch.nn.functional as Fn

    dev = torch.device("cuda:0")
    out = {}
    g = torch.Generator(device="cpu").manual_seed(0)
    boards = torch.randint(0, 6, (n, 9, 9), generator=g).to(dev)
    for layers, F in CONFIGS:
        def conv(cin, cout, k):
            w = (torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5).to(dev, torch.bfloat16)
            return w.contiguous(memory_format=torch.channels_last), (0.1 * torch.randn(cout, generator=g)).to(dev, torch.bfloat16)
        stem = conv(32, F, 3)
        tower = [(conv(F, F, 3), conv(F, F, 3)) for _ in range(layers)]
        vconv, pconv = conv(F, 1, 1), conv(F, 2, 1)
        d1 = (torch.randn(81, F, generator=g) / 9).to(dev, torch.bfloat16)
        d2 = (torch.randn(F, 1, generator=g) / F ** 0.5).to(dev, torch.bfloat16)
        pd = (torch.randn(162, 144, generator=g) / 12).to(dev, torch.bfloat16)

        def forward():
            x = Fn.one_hot(boards, 32).to(torch.bfloat16).permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last)
            x = torch.relu(Fn.conv2d(x, *stem, padding=1))
            for (a, b) in tower:
                t = torch.relu(Fn.conv2d(x, *a, padding=1))
                x = torch.relu(Fn.conv2d(t, *b, padding=1) + x)
            v = torch.relu(Fn.conv2d(x, *vconv)).permute(0, 2, 3, 1).reshape(n, -1)
            v = torch.relu(torch.relu(v @ d1) @ d2)
            p = torch.relu(Fn.conv2d(x, *pconv)).permute(0, 2, 3, 1).reshape(n, -1) @ pd
            return v, p
        with torch.no_grad():
            forward()
            forward()
            torch.cuda.synchronize()
            ms = []
            for _ in range(repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                forward()
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1))
        out[f"{layers}x{F}"] = ms
    print(json.dumps({"torch": torch.__version__, "ms": out}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boards", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--search-simulations", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--torch-child", action="store_true")
    a = ap.parse_args()
    if a.torch_child:
        return torch_child(a.boards, a.repeats)

    import net_ref
    from match3tile import _native
    from match3tile.boardConfig import BoardConfig
    from match3tile.boardv2 import BoardV2
    from match3tile.net import ElementCrushNet
    from match3tile.search import DeviceSearchNN, onehot_width

    if _native.device_count() == 0:
        sys.exit("net_bench.py needs the GPU")
    n, L = a.boards, _native.lib()
    cfg = BoardConfig(rows=9, columns=9, types=6)
    ctx = _native.context(*SHAPE)
    boards = np.random.default_rng(1).integers(0, 6, (n, 81)).astype(np.int8)
    d_b, d_v, d_l = ctx.device_array(boards), ctx.device_empty(n * 4), ctx.device_empty(n * ctx.A * 4)

    def device_ms(net):
        ms = ctypes.c_float()
        _native.check(L.m3_ctx_timer(ctx.handle, 0, None))
        net.forward_device(d_b, n, d_v, d_l, sync=False)
        _native.check(L.m3_ctx_timer(ctx.handle, 1, ctypes.byref(ms)))
        return ms.value

    out = {"what": "policy/value network forward on the device, MI355X (tools/net_bench.py)", "shape": "9x9x6",
           "boards": n, "peak_bf16_flops_spec": PEAK_BF16, "configs": {}}
    nets = {}
    for layers, F in CONFIGS:
        full = ElementCrushNet(cfg, layers, F, net_ref.make_weights(SHAPE + (layers, F)))
        bare = ElementCrushNet(cfg, 0, F, net_ref.make_weights(SHAPE + (0, F)))
        device_ms(full), device_ms(bare)  # warm-up
        t_full, t_bare = [], []
        for _ in range(a.repeats):  # alternating
            t_full.append(device_ms(full))
            t_bare.append(device_ms(bare))
        tf, tb = float(np.median(t_full)), float(np.median(t_bare))
        tower_s = max(tf - tb, 1e-9) / 1e3
        flop = tower_flop(n, layers, F)
        out["configs"][f"{layers}x{F}"] = {
            "layers": layers, "features": F, "forward_ms": spread(t_full), "without_tower_ms": spread(t_bare),
            "evaluations_per_s": n / (tf / 1e3), "tower_share": 1.0 - tb / tf, "tower_flop": flop,
            "tower_tflops": flop / tower_s / 1e12, "tower_fraction_of_peak": flop / tower_s / PEAK_BF16}
        print(f"# {layers}x{F}: {tf:.3f} ms, {n / (tf / 1e3):.0f} evaluations/s", file=sys.stderr, flush=True)
        bare.close()
        nets[(layers, F)] = full
    # the guided search: the (4, 64) net beside the linear evaluator
    sims = a.search_simulations
    roots = [BoardV2(20, BoardConfig(seed=s)) for s in range(1, n + 1)]
    W = np.random.RandomState(1).standard_normal((81, onehot_width(6), 145)).astype(np.float32)
    paths = {"net_4x64": dict(net=nets[(4, 64)]), "linear": dict(weights=W)}
    times = {p: [] for p in paths}
    for rep in range(a.repeats + 1):
        for p, kw in paths.items():
            ds = DeviceSearchNN(roots, sims, node_capacity=2 + sims, **kw)
            ds.result(children=False)
            t0 = time.perf_counter()
            ds.run()
            ds.result(children=False)
            dt = time.perf_counter() - t0
            ds.close()
            if rep:
                times[p].append(dt)
    out["search"] = {"games": n, "simulations": sims}
    for p in paths:
        out["search"][p + "_s"] = spread(times[p])
        out["search"][p + "_simulations_per_s"] = n * sims / float(np.median(times[p]))
    for net in nets.values():
        net.close()
    for d in (d_b, d_v, d_l):
        d.free()
    ctx.close()
    if not a.no_torch:  # a fresh child process: torch brings its own HIP runtime state
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--torch-child", "--boards", str(n), "--repeats",
                            str(a.repeats)], capture_output=True, text=True)
        if r.returncode:
            out["torch_error"] = (r.stderr or r.stdout)[-400:]
        else:
            t = json.loads(r.stdout.strip().splitlines()[-1])
            out["torch_version"] = t["torch"]
            for key, ms in t["ms"].items():
                c = out["configs"][key]
                c["torch_bf16_channels_last_ms"] = spread(ms)
                c["torch_evaluations_per_s"] = n / (float(np.median(ms)) / 1e3)
                c["speed_vs_torch"] = float(np.median(ms)) / c["forward_ms"]["median"]
    s = json.dumps(out, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s)


if __name__ == "__main__":
    main()
