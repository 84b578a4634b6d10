"""Network-guided device MCTS trees (m3_search_nn_*, DeviceSearchNN) on the MI355X against the
reference's own tree code.

Expected side: tests/golden/search_nn.npz alone -- what ``NNNode`` / ``BaseNode.ucb1`` /
``BaseMCTS.__call__`` of the reference computed (gen_golden_search_nn.py) -- with the evaluators of
tests/nn_evaluators.py. No oracle and no Python model of the search is involved: the device shares
nothing with the expected side but the evaluator. Every field of every game and call is compared,
floats as bit patterns. tests/test_search_nn_golden_cpu.py asks the same of the host build first.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import search_nn_golden as gold  # noqa: E402
from match3tile import _native  # noqa: E402
from match3tile.boardConfig import BoardConfig  # noqa: E402
from match3tile.boardv2 import BoardV2  # noqa: E402
from match3tile.search import DeviceSearchNN  # noqa: E402


@pytest.fixture(scope="module")
def data(golden):
    return golden("search_nn")


def states_of(shape, roots):
    out = []
    for r in roots:
        st = BoardV2(r["n_actions"], BoardConfig(seed=r["seed"], rows=shape[0], columns=shape[1], types=shape[2]),
                     np.array(r["board"], np.int64))
        st._reward = r["reward"]
        out.append(st)
    return out


def check_calls(ds, cs, run_call, games=None, tag=""):
    """Every call of the case on `ds`: run_call(call) runs its simulations; every game against the file;
    re-rooted with advance(None). games[g]: the case's game that object game g plays (default: g)."""
    games = list(range(ds.n)) if games is None else games
    for call in range(cs["calls"]):
        run_call(call)
        res = ds.result()
        for g, src in enumerate(games):
            gold.assert_game(res, g, cs["want"][src][call], (cs["name"], tag, call))
        states = ds.advance(None)
        for g, src in enumerate(games):
            assert states[g].n_actions == cs["roots"][src]["n_actions"] - call - 1
            assert states[g].reward >= cs["roots"][src]["reward"]


def run_case(cs, mode):
    """mode "host": the evaluator fed from host arrays; "linear": the device's linear evaluator;
    "device": the caller drives every batch and hands the answers over as device pointers."""
    n, shape = len(cs["roots"]), cs["shape"]
    A = 2 * shape[0] * (shape[1] - 1)
    rounds = cs["calls"] * cs["sims"]
    cap = 2 + rounds
    ev = gold.batch_evaluator(cs["ev"], n, A)
    states = states_of(shape, cs["roots"])
    if mode == "linear":
        ds = DeviceSearchNN(states, cs["sims"], weights=cs["W"], node_capacity=cap)
        check_calls(ds, cs, lambda call: ds.run(), tag=mode)
    elif mode == "host":
        ds = DeviceSearchNN(states, cs["sims"], evaluator=ev, node_capacity=cap)
        check_calls(ds, cs, lambda call: ds.run(), tag=mode)
    else:
        ds = DeviceSearchNN(states, cs["sims"], evaluator=False, node_capacity=cap)
        d_v, d_l = ds._ctx.device_empty(n * 4), ds._ctx.device_empty(n * A * 4)
        check_calls(ds, cs, lambda call: gold.feed_device_rounds(ds, ev, d_v, d_l, cs["sims"], call == 0), tag=mode)
    st = ds.stats()
    assert st["rounds"] == rounds and 1 <= st["nodes_used"] <= cap
    feeds = dict(host=("host_feeds", ev), linear=("linear_evals", None), device=("device_feeds", ev))[mode]
    for k in ("host_feeds", "linear_evals", "device_feeds"):
        assert st[k] == (2 + rounds if k == feeds[0] else 0), (k, st)
    if feeds[1] is not None:
        assert ev.state["calls"] == 2 + rounds
    ds.close()
    if mode == "device":
        d_v.free()
        d_l.free()


@pytest.mark.parametrize("name", ["A", "C", "D", "E", "M"])
def test_linear_cases_host_fed_and_on_the_device(data, name):
    cs = gold.load_case(data, name)
    run_case(cs, "host")
    run_case(cs, "linear")


@pytest.mark.parametrize("name", ["Fc", "Fn"])
def test_named_evaluators_host_fed(data, name):
    """Ties (constant logits) and negative priors; no weights: host-fed only."""
    run_case(gold.load_case(data, name), "host")


def test_case_m_mid_episode_roots_through_feed_device(data):
    """Roots with a reward, both calls with the answers handed over as device pointers."""
    run_case(gold.load_case(data, "M"), "device")


def test_case_w_wide_frame_20x20x6(data):
    """The 32x32 frame: A = 760, AW = 24, twelve lane passes per logits row."""
    cs = gold.load_case(data, "W")
    run_case(cs, "host")
    run_case(cs, "linear")


@pytest.mark.parametrize("mode", ["host", "linear"])
def test_second_set_roots_on_a_live_object(data, mode):
    """Two calls of case A, then m3_search_nn_set_roots with case M's roots (its 8 roots repeated over
    the 18 games) on the same object: equal to the file bit for bit -- and so to a fresh object, which
    test_linear_cases_host_fed_and_on_the_device holds to the same file. The node pool keeps the old
    trees' bytes."""
    a, m = gold.load_case(data, "A"), gold.load_case(data, "M")
    n, A, L = 18, 144, _native.lib()
    cap = 2 + 3 * a["sims"]
    if mode == "linear":
        ds = DeviceSearchNN(states_of(a["shape"], a["roots"]), a["sims"], weights=a["W"], node_capacity=cap)
    else:
        ds = DeviceSearchNN(states_of(a["shape"], a["roots"]), a["sims"], evaluator=gold.batch_evaluator(a["ev"], n, A),
                            node_capacity=cap)
    check_calls(ds, dict(a, calls=2), lambda call: ds.run(), tag="before")
    assert ds.stats()["rounds"] == 2 * a["sims"]
    games = [g % 8 for g in range(n)]
    roots = [m["roots"][src] for src in games]
    ctx = ds._ctx
    boards = ctx._boards(np.stack([r["board"] for r in roots]))
    seeds = np.array([r["seed"] for r in roots], np.uint32)
    na, rew = np.array([r["n_actions"] for r in roots], np.int32), np.array([r["reward"] for r in roots], np.int32)
    with ctx._lock:
        _native.check(L.m3_search_nn_set_roots(ds._h, _native.ptr(boards), _native.ptr(seeds), _native.ptr(na),
                                               _native.ptr(rew)))
    if mode == "linear":
        d_w = ctx.device_array(np.ascontiguousarray(m["W"], np.float32))

        def run_call(call):  # (pending construction batches are part of the first run)
            with ctx._lock:
                _native.check(L.m3_search_nn_run_linear(ds._h, m["sims"], d_w.ptr))
    else:
        ev = gold.batch_evaluator(m["ev"], n, A)

        def run_call(call):
            for k in range(-2 if call == 0 else 0, m["sims"]):
                boards_k, need = ds.batch(max(1, m["sims"] - max(0, k)))
                ds.feed(*ev(boards_k, need))
    check_calls(ds, m, run_call, games=games, tag="again")
    st = ds.stats()
    assert st["rounds"] == m["calls"] * m["sims"] and st["nodes_used"] <= 2 + m["calls"] * m["sims"]
    ds.close()
    if mode == "linear":
        d_w.free()
