"""The search-tree core (csrc/m3_search_core.hpp) on the CPU, before a GPU sees it.

tests/search_host builds the M3_HD functions the tree kernels call -- selection, the attach, backup,
the result, the re-rooting -- for the host; the step and the playout between them come from the C
oracle. Expected side: ``match3tile.mcts.MCTS`` over the same oracle (search_ref.py), which
tests/test_mcts_cpu.py holds to the real reference's outputs, and those outputs themselves
(tests/golden/mcts.npz, the se_* cases).
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "search_host"))
import search_host as sh  # noqa: E402
import search_ref as ref  # noqa: E402

SHAPE = (9, 9, 6)


def run_group(roots, sims, calls, record=None, capacity=None):
    """The roots as one lockstep HostSearch; yields (call, result arrays) and re-roots at best_action."""
    o = ref.oracle(SHAPE)
    states = [ref.root_state(SHAPE, r["seed"], r["n_actions"]) for r in roots]
    hs = sh.HostSearch(o, states, capacity or 2 + calls * sims, record)
    seeds = [ref.rollout_seeds(r["pyseed"], sims, calls) for r in roots]
    for call in range(calls):
        assert hs.run(sims, [[seeds[g][call][k] for g in range(len(roots))] for k in range(sims)]) == 0
        res = hs.result()
        yield call, res, hs
        bad, _, _, na = hs.advance(res["best_action"])
        assert bad == 0
        assert list(na) == [r["n_actions"] - call - 1 for r in roots]


def test_golden_searches(golden):
    """The real reference's (action, value, policies), two consecutive calls, and the whole root of
    the Python search over the oracle."""
    g = golden("mcts")
    for i in range(len(g["se_seed"])):
        sims = int(g["se_sims"][i])
        root = dict(seed=int(g["se_seed"][i]), n_actions=20, pyseed=int(g["se_pyseed"][i]))
        want = ref.reference_search(SHAPE, root["seed"], 20, sims, root["pyseed"], 2, float(g["se_c"][i]))
        for call, res, _ in run_group([root], sims, 2):
            n = int(g[f"se{call}_npol"][i])
            assert res["best_action"][0] == g[f"se{call}_action"][i], (i, call)
            assert res["value"][0] == g[f"se{call}_value"][i], (i, call)
            pol = res["child_visits"][0][:res["n_children"][0]] / res["root_visits"][0]
            assert np.array_equal(pol, g[f"se{call}_policies"][i][:n]), (i, call)
            ref.assert_result(res, 0, want[call], ("golden", i, call))


@pytest.mark.parametrize("key", sorted(ref.extra_groups()), ids=lambda k: f"na{k[0]}-sims{k[1]}")
def test_extra_roots(key):
    """32 roots off the golden file's seeds, in lockstep groups, at exactly the capacity they need."""
    n_actions, sims = key
    roots = ref.extra_groups()[key]
    calls = ref.calls_possible(n_actions, ref.EXTRA_CALLS)
    want = [ref.reference_search(SHAPE, r["seed"], n_actions, sims, r["pyseed"], calls) for r in roots]
    for call, res, hs in run_group(roots, sims, calls):
        for g in range(len(roots)):
            ref.assert_result(res, g, want[g][call], (key, call))
    assert max(hs.nodes_used(g) for g in range(len(roots))) <= 2 + calls * sims
    if (n_actions, sims) in ((1, 40), (2, 40)):  # saturated: simulations that rolled a terminal leaf out again
        assert max(hs.nodes_used(g) for g in range(len(roots))) < 2 + calls * sims


def test_every_extra_pairing_is_covered():
    assert len(ref.EXTRA) == 32 and len(ref.extra_groups()) == 12
    assert not {r["seed"] for r in ref.EXTRA} & {3, 11, 29, 101}


def test_terminal_root_and_order_of_calls():
    """A search whose root is terminal has no child (-1), where the reference's finish raises; a run
    before the roots are set, and one past the capacity, are refused with nothing done."""
    o = ref.oracle(SHAPE)
    st = ref.root_state(SHAPE, 77, 1)
    hs = sh.HostSearch(o, [st], 2 + 2 * 3)
    assert hs.run(3, [[5], [6], [7]]) == 0
    res = hs.result()
    assert res["n_children"][0] == min(len(st.legal_actions), 1 + 3)  # every child is terminal: one more per round
    assert hs.advance(res["best_action"])[0] == 0
    assert hs.run(3, [[8], [9], [10]]) == 0
    res2 = hs.result()
    assert res2["best_action"][0] == -1 and res2["n_children"][0] == 0 and res2["root_visits"][0] >= 3
    assert hs.advance([0])[0] == 1  # no such child: the root stays
    assert hs.run(1, [[1]]) == -7  # 1 + 6 simulations run: a 7th does not fit 8 slots
    L = sh.lib()
    h = L.sh_create(1, 8, 81, 5, 144)
    assert L.sh_run_begin(h, 1) == -6
    L.sh_destroy(h)


def test_log_table_is_libm_log():
    """m3_search_log_table (host only) and the core's table: math.log, compared as bits."""
    want = np.array([math.log(v) for v in range(1, 65537)])
    got = np.zeros(65536)
    sh.lib().sh_log_table(65536, sh._p(got))
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    from match3tile import _native
    got2 = np.zeros(65536)
    _native.check(_native.lib().m3_search_log_table(65536, _native.ptr(got2)))
    assert np.array_equal(got2.view(np.uint64), want.view(np.uint64))


def test_host_ucb1_is_pythons():
    """The host build of search_ucb1 against Node.ucb1's expression, as bits."""
    rng = np.random.default_rng(11)
    L = sh.lib()
    for _ in range(2000):
        v = int(rng.integers(1, 300))
        pv = v + int(rng.integers(0, 3000))
        rs = int(rng.integers(0, 400 * v))
        c = float(rng.integers(0, 21))
        want = rs / v + c * math.sqrt(math.log(pv) / (1 + v))
        assert L.sh_ucb1(rs, v, pv, c) == want
    assert L.sh_ucb1(5, 0, 1, 3.0) == math.inf


def test_search_core_under_asan_ubsan(tmp_path):
    """The stand-alone program replays the recorded scenario of one group (n_actions 5, 7 simulations,
    three calls, run at exactly node_capacity, then one request beyond it) and must print the results
    of the Python run above it."""
    roots = ref.extra_groups()[(5, 7)]
    rec, lines = [], []
    for call, res, hs in run_group(roots, 7, 3, record=rec):
        lines += sh.result_lines(res)
    assert hs.run(1, [[1] * len(roots)]) == -7
    lines.append("refused 1")
    path = tmp_path / "scenario.txt"
    path.write_text(" ".join(map(str, rec)) + "\n")
    d = os.path.join(ROOT, "tests", "search_host")
    subprocess.run(["make", "-C", d, "asan"], check=True, capture_output=True)
    r = subprocess.run([os.path.join(d, "build", "search_asan"), str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and "checks ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    out = r.stdout.strip().splitlines()
    assert out[:-1] == lines
    assert f"3 results, 1 refused, {2 + 3 * 7} of {2 + 3 * 7} nodes" in out[-1]
