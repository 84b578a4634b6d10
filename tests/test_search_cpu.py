"""The search-tree core (csrc/m3_search_core.hpp) on the CPU, before a GPU sees it.

tests/search_host builds the M3_HD functions the tree kernels call -- selection, the attach, backup,
the result, the re-rooting -- for the host; the step and the playout between them come from the C
oracle. Expected side: ``match3tile.mcts.MCTS`` over the same oracle (search_ref.py), which
tests/test_mcts_cpu.py holds to the real reference's outputs, and those outputs themselves
(tests/golden/mcts.npz, the se_* cases).

The cases of search_ref.general_search -- games that freeze beside games that go on, roots that are no
reset boards (two of them terminal from the start), re-rooting at a chosen child, a second set of
roots on a live object -- run here first and on the device in tests/test_gpu_search.py. The driver
hands the core the step flags k_apply would (search_host.py, _round): M3_FLAG_NO_LEGAL beside a cap.
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


RESULT_KEYS = ("best_action", "value", "root_visits", "n_children", "child_action", "child_visits", "child_reward", "flags")


def run_case(cs, record=None):
    """A case of search_ref as one lockstep HostSearch at exactly the capacity its calls need; yields
    (call, result arrays, HostSearch). The caller re-roots."""
    hs = sh.HostSearch(ref.capped_oracle(cs["shape"]), cs["states"], 2 + cs["calls"] * cs["sims"], record)
    for call in range(cs["calls"]):
        assert hs.run(cs["sims"], ref.round_seeds(cs, call)) == 0
        yield call, hs.result(), hs


def check_freeze_counts(cs):
    dead, step, playout, live = ref.freeze_kinds(cs)
    print(f"freeze case: {len(dead)} dead roots, {len(step)} frozen in a step, {len(playout)} in a playout, "
          f"{len(live)} never; flag words {sorted({hex(w[-1]['flags']) for w in cs['want'] if w[-1]['flags']})}")
    assert len(dead) >= 1 and len(step) >= 1 and len(playout) >= 1 and len(live) >= 40
    return dead, step, playout, live


def test_frozen_games_freeze_alone():
    """5x5x6, 64 games in lockstep: dead roots, caps in an expansion's step and in a playout. A frozen
    game reports its tree as it stood and its flag word; the games beside it go on as if alone."""
    cs = ref.freeze_case()
    check_freeze_counts(cs)
    n = len(cs["roots"])
    for call, res, hs in run_case(cs):
        for g in range(n):
            ref.assert_game(res, g, cs["want"][g][call], ("freeze", call))
        if call == 0:
            first = {k: res[k].copy() for k in RESULT_KEYS}
        else:
            for g in (g for g in range(n) if cs["want"][g][0]["flags"]):
                for k in RESULT_KEYS:
                    assert np.array_equal(res[k][g], first[k][g]), (g, k)
        bad, _, _, na = hs.advance(res["best_action"])  # (a frozen game keeps its root: not a bad action)
        assert bad == 0
        for g in range(n):
            assert na[g] == 6 - sum(not w["flags"] for w in cs["want"][g][:call + 1]), (g, call)  # one move per unfrozen call


def test_heterogeneous_roots():
    """Mid-episode roots with specials, 20 different n_actions in one batch, non-zero root rewards, and
    two roots that are terminal when they are set: those keep no child (include/m3.h,
    m3_search_set_roots -- the reference's constructor would attach the state to itself)."""
    cs = ref.hetero_case()
    assert sorted({r["n_actions"] for r in cs["roots"]}) == list(range(0, 21))
    (_, res, hs), = run_case(cs)
    for g in range(40):
        ref.assert_game(res, g, cs["want"][g][0], "hetero")
    for g in (36, 37):
        assert cs["roots"][g]["reward"] > 0
        assert (res["best_action"][g], res["n_children"][g], res["root_visits"][g], res["flags"][g]) == (-1, 0, 10, 0)
        assert res["value"][g] == cs["roots"][g]["reward"]
        assert hs.nodes_used(g) == 1


def test_advance_with_explicit_actions():
    """Three calls, each re-rooted at the last of the least-visited root children instead of the best."""
    cs = ref.advance_case()
    n = len(cs["roots"])
    for call, res, hs in run_case(cs):
        for g in range(n):
            ref.assert_game(res, g, cs["want"][g][call], ("advance", call))
        actions = [ref.least_visited_last(call, cs["want"][g][call]) for g in range(n)]
        first = [cs["want"][g][call]["children"][0][0] for g in range(n)]
        assert any(a != cs["want"][g][call]["action"] for g, a in enumerate(actions))  # not the default re-rooting
        assert any(a != f for a, f in zip(actions, first))                             # nor the first child
        bad, _, rew, na = hs.advance(actions)
        assert bad == 0
        assert [(int(a), int(b)) for a, b in zip(na, rew)] == [cs["want"][g][call]["next"] for g in range(n)], call


def test_second_set_roots_drops_the_trees():
    """One object at capacity 2 + 12: a search that freezes some games, then other roots and a second
    search of 12 rounds, which fits only because the slots were given back; the flag words start again."""
    first = ref.freeze_case()
    second = ref.case((5, 5, 6), ref.reset_roots(range(101, 165), 6), 12, 1)
    assert [g for g in range(64) if first["want"][g][0]["flags"] and not second["want"][g][0]["flags"]]
    hs = sh.HostSearch(ref.capped_oracle((5, 5, 6)), first["states"], 2 + 12)
    for cs in (first, second):
        if cs is second:
            hs.set_roots(cs["states"])
        assert hs.run(12, ref.round_seeds(cs, 0)) == 0
        res = hs.result()
        for g in range(64):
            ref.assert_game(res, g, cs["want"][g][0], ("set_roots", cs["roots"][0]["seed"]))
        assert hs.run(1, [[1] * 64]) == -7  # the object is full again


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


def test_freeze_scenario_under_asan_ubsan(tmp_path):
    """The 64 games of test_frozen_games_freeze_alone (both calls at exactly node_capacity, frozen games
    among them) replayed by the stand-alone program: it must print the Python run's results."""
    cs = ref.freeze_case()
    rec, lines, used = [], [], 0
    for call, res, hs in run_case(cs, record=rec):
        lines += sh.result_lines(res)
        assert hs.advance(res["best_action"])[0] == 0
        used = max(hs.nodes_used(g) for g in range(len(cs["roots"])))
    assert any(line.split()[5] != "0" for line in lines)  # (flags: frozen games are in the text)
    path = tmp_path / "scenario.txt"
    path.write_text(" ".join(map(str, rec)) + "\n")
    d = os.path.join(ROOT, "tests", "search_host")
    subprocess.run(["make", "-C", d, "asan"], check=True, capture_output=True)
    r = subprocess.run([os.path.join(d, "build", "search_asan"), str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and "checks ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    out = r.stdout.strip().splitlines()
    assert out[:-1] == lines
    assert f"2 results, 0 refused, {used} of {2 + 2 * 12} nodes" in out[-1]
