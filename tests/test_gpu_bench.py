"""bench.py end to end on the MI355X at reduced size: the bench attests its own run.

After the clock stops, bench.py replays boards spread over the env through the C
oracle (from their first episode through every same-step autoreset to the last
timed step) and reports parity.oracle_match; nranks comes from the RCCL
communicator (1 without one)."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape,boards", [("9x9x6", 65536), ("16x16x8", 16384)])
def test_bench_line_attests_parity(shape, boards):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--shape", shape, "--boards", str(boards),
           "--steps", "6", "--warmup", "3", "--full", "--no-cpu-baseline", "--check-boards", "384"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    d = json.loads(out.stdout.strip().splitlines()[-1])
    assert d["value"] > 0 and d["n_gpus"] == 1 and d["nranks"] == 1 and d["gather_ok"] is None
    assert d["parity"]["oracle_match"] is True, d["parity"]
    assert d["parity"]["oracle_sample"]["boards"] == 384 and len(d["parity"]["digest"]) == 8


def test_plain_run_is_lean_and_dumps_its_last_step(tmp_path):
    """Without --full the line holds the headline figure only (no parity, roofline or CPU baseline);
    --dump-outputs writes the last timed step's outputs as float .npy files, and a board the oracle
    replays over the same warmup + steps ends where the dump says."""
    import numpy as np

    from oracle import Oracle

    boards, steps, warmup = 4096, 5, 2
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--boards", str(boards),
           "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(tmp_path / "out")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    d = json.loads(out.stdout.strip().splitlines()[-1])
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["steps"] == steps and d["full"] is False
    assert d["unit"] == "env-steps/s" and d["higher_is_better"] is True and d["dtype"] == "int8"
    assert abs(d["value"] - boards * steps / (d["ms_per_step"] * steps / 1e3)) <= 1e-6 * d["value"]
    assert not {"parity", "roofline", "cpu_baseline", "gather_ok", "path_stats"} & set(d)
    got = {f[:-4]: np.load(tmp_path / "out" / f) for f in sorted(os.listdir(tmp_path / "out"))}
    assert set(got) == {"observations", "rewards", "dones", "truncateds", "flags", "scores", "moves",
                        "next_actions", "seeds", "board_index"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    assert got["observations"].shape == (boards, 9, 9) and (got["board_index"] == np.arange(boards)).all()
    # boards still inside their first episode (seed 1 + b) after warmup + steps moves, as bench.py's own replay
    o = Oracle(9, 9, 6, episode_shuffle_cap=1024)
    rem, checked = steps + warmup, 0
    for b in (0, 1, 1777, 2048, boards - 2, boards - 1):
        if o.random_episode(1 + b, 20, 500)["n"] <= rem:
            continue
        ep = o.random_episode(1 + b, rem, 500)
        assert (got["observations"][b].reshape(-1) == ep["final"].reshape(-1)).all()
        assert got["scores"][b] == ep["rewards"].sum() and got["rewards"][b] == ep["rewards"][-1]
        assert got["seeds"][b] == 1 + b and got["moves"][b] == rem
        checked += 1
    assert checked >= 3


def test_more_gpus_than_the_box_has_fails_loudly():
    """`python bench.py --gpus N` with N above the visible GPUs: the rank whose GPU index is not
    visible fails before any device work and the whole job exits non-zero -- no 1-GPU line
    printed under an N-GPU command (the driver's scaling run uses this command form)."""
    from match3tile import _native

    n = _native.device_count()
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n + 1), "--boards", "4096",
           "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--check-boards", "0"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode != 0
    assert not [x for x in out.stdout.splitlines() if x.startswith("{")], out.stdout[-2000:]
