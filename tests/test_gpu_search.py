"""Device-resident MCTS trees (m3_search_*, match3tile.search.DeviceSearch) on the MI355X.

Bar: the device search returns what the reference's search returns -- the real reference's
(action, value, policies) of tests/golden/mcts.npz, and, against ``match3tile.mcts.MCTS`` over the C
oracle (search_ref.py), every root child's action, visits and reward sum and the root's visits, for
every game of a lockstep batch over consecutive calls. UCB1 on the device is compared with CPython's
evaluation as bits.

The frame-shape case is 7 rows x 5 columns x 4 types: a board of 5 rows x 7 columns has action ids
that decode past its last row, the reference raises IndexError on every step of it, and the library
refuses it (M3_ERR_INVALID) -- which the last test checks.
"""
import math
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import search_ref as ref  # noqa: E402
from match3tile import _native  # noqa: E402
from match3tile.boardConfig import BoardConfig  # noqa: E402
from match3tile.boardv2 import BoardV2  # noqa: E402
from match3tile.dataset import play_games  # noqa: E402
from match3tile.search import DeviceSearch  # noqa: E402


def device_states(shape, seeds, n_actions):
    """BoardV2 roots holding the oracle's initial boards (the boards of search_ref.root_state)."""
    out = []
    for s in seeds:
        cfg = BoardConfig(rows=shape[0], columns=shape[1], types=shape[2], seed=int(s))
        out.append(BoardV2(n_actions, cfg, ref.oracle(shape).init_board(int(s))[0].astype(np.int64)))
    return out


def check_against_python(shape, seeds, n_actions, sims, calls, with_advance=True):
    pyseeds = [9000 + int(s) for s in seeds]
    want = [ref.reference_search(shape, int(s), n_actions, sims, ps, calls) for s, ps in zip(seeds, pyseeds)]
    ds = DeviceSearch(device_states(shape, seeds, n_actions), sims, node_capacity=2 + calls * sims)
    rs = [ref.rollout_seeds(ps, sims, calls) for ps in pyseeds]
    for call in range(calls):
        ds.run([[rs[g][call][k] for g in range(len(seeds))] for k in range(sims)])
        res = ds.result()
        for g in range(len(seeds)):
            ref.assert_result(res, g, want[g][call], (shape, call))
        states = ds.advance(None)
        for g, st in enumerate(states):
            assert st.n_actions == n_actions - call - 1
    st = ds.stats()
    assert st["rounds"] == calls * sims and 2 <= st["nodes_used"] <= 2 + calls * sims
    ds.close()
    return st


def test_golden_searches(golden):
    """The four se_* cases of the real reference, one game each, two calls through __call__."""
    g = golden("mcts")
    for i in range(len(g["se_seed"])):
        root = BoardV2(20, BoardConfig(seed=int(g["se_seed"][i])))
        ds = DeviceSearch([root], int(g["se_sims"][i]), rngs=[random.Random(int(g["se_pyseed"][i]))])
        for call in range(2):
            (a, v, p), = ds()
            n = int(g[f"se{call}_npol"][i])
            assert a == g[f"se{call}_action"][i], (i, call)
            assert v == g[f"se{call}_value"][i], (i, call)
            assert np.array_equal(np.array(p), g[f"se{call}_policies"][i][:n]), (i, call)
        assert ds.states()[0].n_actions == 18
        ds.close()


def test_130_games_three_calls():
    """Two full waves and a ragged third, re-rooted twice."""
    check_against_python((9, 9, 6), range(1, 131), 4, 20, 3)


def test_16x16x8():
    check_against_python((16, 16, 8), range(1, 9), 20, 12, 2)


def test_frame_shape_7x5x4():
    o = ref.oracle((7, 5, 4))
    seeds = [s for s in range(1, 40) if o.legal_actions(o.init_board(s)[0])][:8]
    assert len(seeds) == 8
    check_against_python((7, 5, 4), seeds, 20, 12, 1)


def test_saturated_trees():
    """n_actions = 2, 40 simulations: selection ends on terminal leaves and rolls them out again."""
    st = check_against_python((9, 9, 6), range(301, 317), 2, 40, 2)
    assert st["nodes_used"] < 2 + 2 * 40


def test_caps_and_order():
    ctx = _native.context(9, 9, 6)
    L = _native.lib()
    import ctypes
    h = ctypes.c_void_p()
    _native.check(L.m3_search_create(ctx.handle, 1, 8, ctypes.byref(h)))
    one = np.ones((1, 1), np.uint32)
    assert L.m3_search_run(h, 1, _native.ptr(one)) == -6          # M3_ERR_STATE before set_roots
    assert L.m3_search_result(h, *[None] * 8) == -6
    L.m3_search_destroy(h)
    sims = 10
    states = device_states((9, 9, 6), [5, 6, 7], 20)
    ds = DeviceSearch(states, sims, node_capacity=2 + 2 * sims - 1)  # one short of two runs
    seeds = np.arange(sims * 3, dtype=np.uint32).reshape(sims, 3) + 17
    ds.run(seeds)
    first = ds.result()
    with pytest.raises(_native.M3Error) as e:
        ds.run(seeds)
    assert e.value.code == -7                                     # M3_ERR_CAP, nothing enqueued
    again = ds.result()                                           # the previous run is still readable
    for k in first:
        for g in range(3):  # (child arrays: the root's n_children entries)
            a, b = (x[k][g][:first["n_children"][g]] if x[k].ndim == 2 else x[k][g] for x in (first, again))
            assert np.array_equal(a, b), k
    assert ds.stats()["rounds"] == sims and (again["root_visits"] == sims).all()
    ds.run(seeds[:sims - 1])                                      # what still fits, runs
    assert (ds.result()["root_visits"] == 2 * sims - 1).all()
    with pytest.raises(_native.M3Error) as e:                     # an action without an expanded child
        ds.advance([10000, 10000, 10000])
    assert e.value.code == -1
    ds.close()


def test_play_games_device_tree_equals_host_trees():
    cfgs = [BoardConfig(seed=s) for s in (2, 3, 5, 8, 13)]
    pyseeds = [101, 102, 103, 104, 105]
    host = play_games(cfgs, 3, pyseeds, simulations=16)
    dev = play_games(cfgs, 3, pyseeds, simulations=16, device_tree=True)
    assert host.keys() == dev.keys()
    for k in host:
        assert len(host[k]) == len(dev[k]) == 15, k
        for a, b in zip(host[k], dev[k]):
            assert np.array_equal(np.asarray(a), np.asarray(b)), k
    with pytest.raises(ValueError):
        play_games(cfgs, 3, pyseeds, simulations=16, leaf_rollouts=2, device_tree=True)


def ucb1_python(rs, v, pv, c):
    """Node.ucb1 (standard/mcts.py:33-37) as CPython evaluates it."""
    if v == 0:
        return float("inf")
    return rs / v + c * math.sqrt(math.log(pv) / (1 + v))


def ucb1_table():
    """~4,096 (reward_sum, visits, parent_visits, c) tuples: values a search meets, unvisited children,
    c = 0, and near-ties -- neighbours (reward_sum, reward_sum + d) at means near 2^35 with ~2^16
    visits (reward sums below 2^53, as the core requires), where one more reward moves the value by about one unit in the last place; only pairs
    whose CPython values differ by exactly one such unit are kept."""
    rng = np.random.default_rng(2024)
    rows = []
    for _ in range(2600):
        v = int(rng.integers(1, 400))
        rows.append((int(rng.integers(0, 500 * v)), v, v + int(rng.integers(0, 5000)), float(rng.integers(1, 21))))
    for _ in range(200):
        rows.append((int(rng.integers(0, 1000)), 0, int(rng.integers(1, 5000)), float(rng.integers(1, 21))))
        v = int(rng.integers(1, 400))
        rows.append((int(rng.integers(0, 500 * v)), v, v + int(rng.integers(0, 5000)), 0.0))
    pairs = 0
    while pairs < 450:
        v = int(rng.integers(1 << 16, 1 << 17))
        pv = v + int(rng.integers(0, 1 << 16))
        rs = (1 << 35) * v + int(rng.integers(0, 1 << 30))
        c = float(rng.integers(1, 21))
        a = ucb1_python(rs, v, pv, c)
        for d in (1, 2, 3, 4):
            b = ucb1_python(rs + d, v, pv, c)
            if int(np.float64(b).view(np.uint64)) - int(np.float64(a).view(np.uint64)) == 1:
                rows += [(rs, v, pv, c), (rs + d, v, pv, c)]
                pairs += 1
                break
    return rows, pairs


def test_ucb1_bits_on_the_device():
    rows, pairs = ucb1_table()
    assert pairs == 450 and 3900 <= len(rows) <= 4200
    rs = np.array([r[0] for r in rows], np.int64)
    v = np.array([r[1] for r in rows], np.int32)
    pv = np.array([r[2] for r in rows], np.int32)
    c = np.array([r[3] for r in rows], np.float64)
    out = np.zeros(len(rows), np.float64)
    ctx = _native.context(9, 9, 6)
    _native.check(_native.lib().m3_search_ucb1(ctx.handle, len(rows), _native.ptr(rs), _native.ptr(v), _native.ptr(pv),
                                               _native.ptr(c), _native.ptr(out)))
    want = np.array([ucb1_python(*r) for r in rows], np.float64)
    diff = np.flatnonzero(out.view(np.uint64) != want.view(np.uint64))
    print("ucb1: tuples whose bits differ:", len(diff), [(rows[i], out[i].hex(), want[i].hex()) for i in diff[:5]])
    assert len(diff) == 0
    assert np.isinf(out).sum() == 200


def test_rows_below_columns_is_refused():
    """5 rows x 7 columns: the reference raises IndexError on every step (boardConfig.py:27,45-59)."""
    import ctypes
    ctx = _native.context(5, 7, 4)
    h = ctypes.c_void_p()
    assert _native.lib().m3_search_create(ctx.handle, 4, 16, ctypes.byref(h)) == -1
