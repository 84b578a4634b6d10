"""Network-guided device MCTS trees (m3_search_nn_*, match3tile.search.DeviceSearchNN) on the MI355X.

Bar: for every game of a lockstep batch and every call, the device trees hold what the Python model of
search_nn_ref.py holds -- every root child's action, visits, value sum and prior (floats as bit
patterns), the root's visits, the action, the value and the policies -- with the evaluator fed from
the host (cases A, C..H, and P, Q, R: rows with a logit that is not finite) and with the built-in
linear evaluator on the device (case B, which must equal case A bit for bit), and with the answer
handed over as device pointers.
tests/test_search_nn_cpu.py runs the same cases on the host build first.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import search_nn_ref as ref  # noqa: E402
import search_ref  # noqa: E402
from match3tile import _native  # noqa: E402
from match3tile.search import DeviceSearchNN, onehot_width  # noqa: E402


def roots_of(cs):
    return [search_ref.state(cs["shape"], r["board"], r["seed"], r["n_actions"], r["reward"]) for r in cs["roots"]]


def run_case(cs, device_linear=False, spare=0):
    """The case through DeviceSearchNN at exactly the capacity its calls need (+ spare): every game of
    every call against the model, re-rooted at the best action. Returns (DeviceSearchNN, stats)."""
    n, shape = len(cs["roots"]), cs["shape"]
    A = 2 * shape[0] * (shape[1] - 1)
    cap = 2 + cs["calls"] * cs["sims"] + spare
    if device_linear:
        ds = DeviceSearchNN(roots_of(cs), cs["sims"], weights=cs["W"], node_capacity=cap)
    else:
        ev = ref.batch_evaluator(cs["ev"], n, A)
        ds = DeviceSearchNN(roots_of(cs), cs["sims"], evaluator=ev, node_capacity=cap)
    for call in range(cs["calls"]):
        ds.run()
        res = ds.result()
        for g in range(n):
            ref.assert_game(res, g, cs["want"][g][call], (call,))
        states = ds.advance(None)
        for g, st in enumerate(states):
            w = cs["want"][g][call]
            if not w["flags"] and w["action"] >= 0:
                assert st.n_actions == cs["roots"][g]["n_actions"] - call - 1
    st = ds.stats()
    assert st["rounds"] == cs["calls"] * cs["sims"] and 1 <= st["nodes_used"] <= cap
    if device_linear:
        assert st["host_feeds"] == 0 and st["device_feeds"] == 0 and st["linear_evals"] == 2 + cs["calls"] * cs["sims"]
    else:
        assert st["host_feeds"] == 2 + cs["calls"] * cs["sims"] == ev.state["calls"] and st["linear_evals"] == 0
    return ds, st


def same_result(a, b):
    """Two results agree in everything a result defines (the child arrays up to n_children)."""
    if any(not np.array_equal(a[k], b[k]) for k in ("best_action", "value", "root_visits", "n_children", "flags")):
        return False
    return all(np.array_equal(a[k][g][:c].view(np.uint32), b[k][g][:c].view(np.uint32))
               for k in ("child_action", "child_visits", "child_value_sum", "child_prior")
               for g, c in enumerate(a["n_children"]))


def test_case_a_host_fed_linear_evaluator():
    """18 games: one full 16-game workgroup plus a ragged 2; A = 144, three lane passes per logits row."""
    cs = ref.case_a()
    assert all(not w[-1]["flags"] for w in cs["want"])
    run_case(cs)[0].close()


def test_case_b_device_linear_path_equals_case_a():
    """The same want as case A, bit for bit, with no host feed."""
    ds, st = run_case(ref.case_a(), device_linear=True)
    assert st["host_feeds"] == 0
    ds.close()


def test_case_c_16x16x8():
    """A = 480, AW = 15; host-fed and on the device."""
    cs = ref.case_c()
    run_case(cs)[0].close()
    run_case(cs, device_linear=True)[0].close()


def test_case_d_frame_shape_7x5x4():
    """A = 56: a partial lane pass."""
    o = search_ref.oracle((7, 5, 4))
    seeds = [s for s in range(1, 40) if o.legal_actions(o.init_board(s)[0])][:8]
    assert len(seeds) == 8
    cs = ref.case_d(seeds)
    run_case(cs)[0].close()
    run_case(cs, device_linear=True)[0].close()


def test_case_e_saturated_trees():
    """n_actions 2, 40 simulations: terminal leaves visited again (need = 0, return = state reward) and
    terminal new children."""
    cs = ref.case_e()
    ds, st = run_case(cs)
    assert st["nodes_used"] < 2 + 2 * 40
    ds.close()
    run_case(cs, device_linear=True)[0].close()


@pytest.mark.parametrize("which", ["constant", "negative"])
def test_case_f_ties_and_negative_logits(which):
    run_case(ref.case_f(which))[0].close()


def test_case_g_freezing_roots():
    cs = ref.case_g()
    dead = [g for g, w in enumerate(cs["want"]) if w[-1]["flags"] == ref.F_NO_LEGAL and w[-1]["root_visits"] == 0
            and not w[-1]["children"]]
    step = [g for g, w in enumerate(cs["want"]) if w[-1]["flags"] & search_ref.F_STEP_FREEZE]
    live = [g for g, w in enumerate(cs["want"]) if not w[-1]["flags"]]
    assert len(dead) >= 1 and len(step) >= 1 and len(live) >= 32, (dead, step, len(live))
    run_case(cs)[0].close()
    run_case(cs, device_linear=True)[0].close()


def test_case_h_bad_evaluation_freezes_one_game():
    a, h = ref.case_a(), ref.case_h()
    for call in range(3):
        assert h["want"][ref.H_GAME][call]["flags"] == ref.F_BAD_EVAL == _native.FLAG_BAD_EVAL
        assert all(h["want"][g][call] == a["want"][g][call] for g in range(18) if g != ref.H_GAME)
    run_case(h)[0].close()
    ev = ref.batch_evaluator(h["ev"], 18, 144)
    ds = DeviceSearchNN(roots_of(h), h["sims"], evaluator=ev)
    with pytest.raises(RuntimeError, match="BAD_EVAL"):
        ds()
    ds.close()


def test_case_p_one_poisoned_legal_logit_freezes_exactly_that_game():
    """nn_store_row on the device: lanes stride the row by 64, lanes 0..15 make a third pass over ids
    128..143, and a lane reads bit id & 31 of word id >> 5 of the node's legal set. One game each with NaN
    / +inf / -inf at its lowest, its highest, a third-pass and two word-edge legal ids, in the roots'
    batch and in the construction's, freezes with exactly M3_FLAG_BAD_EVAL; FLT_MAX and a denormal do
    not. (tests/test_search_nn_cpu.py asserts that the model's games hold these conditions.)"""
    p = ref.case_p()
    assert set(p["poisons"]) == set(ref.POISON_KINDS)
    for kind, (g, rnd, i, v) in p["poisons"].items():
        assert p["want"][g][-1]["flags"] == (ref.F_BAD_EVAL if ref.POISON_KINDS[kind][4] else 0), kind
    run_case(p)[0].close()


def test_case_p_through_feed_device():
    """The same poisoned rows handed over as device pointers (m3_search_nn_feed_device)."""
    import search_nn_golden as gold
    p = ref.case_p()
    n, A, rounds = 18, 144, p["calls"] * p["sims"]
    ev = ref.batch_evaluator(p["ev"], n, A)
    ds = DeviceSearchNN(roots_of(p), p["sims"], evaluator=False, node_capacity=2 + rounds)
    d_v, d_l = ds._ctx.device_empty(n * 4), ds._ctx.device_empty(n * A * 4)
    for call in range(p["calls"]):
        gold.feed_device_rounds(ds, ev, d_v, d_l, p["sims"], call == 0)
        res = ds.result()
        for g in range(n):
            ref.assert_game(res, g, p["want"][g][call], ("feed_device", call))
        ds.advance(None)
    st = ds.stats()
    assert st["device_feeds"] == 2 + rounds and st["host_feeds"] == 0 and st["rounds"] == rounds
    ds.close()
    d_v.free()
    d_l.free()


def test_case_q_illegal_logits_are_never_read():
    """NaN and +-inf at every illegal id of every needed row of every round: equal to clean case A."""
    a, q = ref.case_a(), ref.case_q()
    assert q["want"] == a["want"]
    run_case(q)[0].close()


def test_case_r_infinite_weight_on_the_device_linear_path():
    """One weight +inf: k_nn_linear itself produces the infinite logit. The games whose evaluated boards
    meet it where the id is legal freeze, on the device's evaluator and host-fed alike."""
    r = ref.case_r()
    frozen = ref.pick_infinite_weight()[3]
    assert [g for g in range(18) if r["want"][g][-1]["flags"] == ref.F_BAD_EVAL] == frozen and 3 <= len(frozen) <= 12
    run_case(r, device_linear=True)[0].close()
    run_case(r)[0].close()


def test_feed_device_equals_host_feed():
    """Case D with the evaluator's answer handed over as device pointers (m3_search_nn_feed_device): the
    caller drives every batch itself, the two construction batches included."""
    o = search_ref.oracle((7, 5, 4))
    cs = ref.case_d([s for s in range(1, 40) if o.legal_actions(o.init_board(s)[0])][:8])
    n, A = 8, 56
    ev = ref.batch_evaluator(cs["ev"], n, A)
    ds = DeviceSearchNN(roots_of(cs), cs["sims"], evaluator=False, node_capacity=2 + cs["sims"])
    d_v, d_l = ds._ctx.device_empty(n * 4), ds._ctx.device_empty(n * A * 4)
    for k in range(2 + cs["sims"]):
        boards, need = ds.batch(max(1, cs["sims"] - max(0, k - 2)))
        values, logits = ev(boards, need)
        d_v.upload(values)   # (blocks on the context stream: the round before has read the arrays)
        d_l.upload(logits)
        ds.feed_device(d_v, d_l)
    res = ds.result()
    for g in range(n):
        ref.assert_game(res, g, cs["want"][g][0], ("feed_device",))
    st = ds.stats()
    assert st["device_feeds"] == 2 + cs["sims"] and st["host_feeds"] == 0 and st["rounds"] == cs["sims"]
    ds.close()
    d_v.free()
    d_l.free()


def test_case_i_protocol_and_capacity():
    L = _native.lib()
    ctx = _native.context(9, 9, 6)
    cs = ref.case_a()
    n, A = 18, 144
    h = ctypes.c_void_p()
    _native.check(L.m3_search_nn_create(ctx.handle, n, 8, ctypes.byref(h)))
    pb, pn = ctypes.c_void_p(), ctypes.c_void_p()
    v, lg = np.zeros(n, np.float32), np.zeros((n, A), np.float32)
    assert L.m3_search_nn_batch(h, 1, ctypes.byref(pb), ctypes.byref(pn)) == -6   # before set_roots
    assert L.m3_search_nn_feed(h, _native.ptr(v), _native.ptr(lg)) == -6
    assert L.m3_search_nn_result(h, *[None] * 9) == -6
    states = roots_of(cs)
    boards = ctx._boards(np.stack([np.asarray(s.array) for s in states]))
    seeds = np.array([s.cfg.seed for s in states], np.uint32)
    na, rew = np.full(n, 4, np.int32), np.zeros(n, np.int32)
    _native.check(L.m3_search_nn_set_roots(h, _native.ptr(boards), _native.ptr(seeds), _native.ptr(na), _native.ptr(rew)))
    assert L.m3_search_nn_feed(h, _native.ptr(v), _native.ptr(lg)) == -6          # a feed without a pending batch
    assert L.m3_search_nn_batch(h, 1, ctypes.byref(pb), ctypes.byref(pn)) == 0
    assert L.m3_search_nn_batch(h, 1, ctypes.byref(pb), ctypes.byref(pn)) == -6   # a second batch before a feed
    assert L.m3_search_nn_result(h, *[None] * 9) == -6
    assert L.m3_search_nn_feed(h, _native.ptr(v), _native.ptr(lg)) == 0
    L.m3_search_nn_destroy(h)
    # a capacity one short of two runs, on both paths
    sims = cs["sims"]
    one = dict(cs, calls=1, want=[w[:1] for w in cs["want"]])
    for device_linear in (False, True):
        ds, _ = run_case(one, device_linear=device_linear, spare=sims - 1)
        first = ds.result()
        with pytest.raises(_native.M3Error) as e:
            ds.run()
        assert e.value.code == -7
        again = ds.result()
        assert same_result(first, again)                                 # the previous result is still readable
        assert ds.stats()["rounds"] == sims
        ds.run(sims - 1)                                                 # what does fit still runs
        assert ds.stats()["rounds"] == 2 * sims - 1
        ds.close()


def test_onehot_width():
    assert [onehot_width(t) for t in (2, 3, 4, 5, 6, 8, 9, 16, 17)] == [ref.onehot_width(t) for t in (2, 3, 4, 5, 6, 8, 9, 16, 17)]
    assert onehot_width(6) == 32 and onehot_width(8) == 32 and onehot_width(4) == 16


def test_batch1_dropin_and_lockstep_episodes():
    """NeuralNetworkMCTS (one game, model(array[1, R, C])) returns the model's (action, value, policies)
    call after call; nn_mcts_episodes scores the same episodes on the device-linear path, on the host
    path and game by game through nn_mcts_task."""
    from match3tile.boardConfig import BoardConfig
    from match3tile.boardv2 import BoardV2
    from match3tile.mcts import NeuralNetworkMCTS
    from match3tile.samplers import nn_mcts_episodes, nn_mcts_task
    from match3tile.search import linear_evaluator

    cs = ref.case_a()
    W = cs["W"]
    calls = []

    def model(x):
        assert x.shape == (1, 9, 9)
        calls.append(1)
        return ref.linear_eval(W, x[0])
    g = 3
    r = cs["roots"][g]
    root = BoardV2(r["n_actions"], BoardConfig(seed=r["seed"]), search_ref.oracle(cs["shape"]).init_board(r["seed"])[0].astype(np.int64))
    m = NeuralNetworkMCTS(model, root, 3, cs["sims"], verbose=False)
    for call in range(cs["calls"]):
        w = cs["want"][g][call]
        assert m() == (w["action"], w["value"], list(w["policies"])), call
    assert m.state.n_actions == r["n_actions"] - cs["calls"] and len(calls) >= 2
    seeds = [11, 12, 13]
    dev = nn_mcts_episodes(seeds, weights=W, moves=3, simulations=8)
    host = nn_mcts_episodes(seeds, evaluator=linear_evaluator(W), moves=3, simulations=8)
    assert np.array_equal(dev, host)

    def model3(x):
        return ref.linear_eval(W, x[0])
    assert [nn_mcts_task(model3, s, simulations=8, moves=3) for s in seeds[:2]] == [int(v) for v in dev[:2]]
