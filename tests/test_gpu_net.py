"""The policy/value network on the MI355X (m3_net_*, match3tile.net.ElementCrushNet) against the CPU
restatements of tests/net_ref.py.

The error measure is e(x) = max |x - f64| / max |f64| over a whole output tensor. The device differs from
the written model only in the order of the float32 accumulation and in the rare bf16 rounding that this
flips, so it must sit closer to the model than the model sits to the true network:
d = max |device - model| / max |f64| <= e(model). A wrong tap, channel or flatten order gives d of order 1.
Measured d / e(model) per case: DESIGN.md §6.0.3.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import net_ref  # noqa: E402
from net_ref import CASES, case_id  # noqa: E402

from match3tile import _native  # noqa: E402
from match3tile.boardConfig import BoardConfig  # noqa: E402
from match3tile.boardv2 import BoardV2  # noqa: E402
from match3tile.net import ElementCrushNet  # noqa: E402
from match3tile.search import DeviceSearchNN  # noqa: E402

_cache = {}


def cfg_of(case):
    return BoardConfig(rows=case[0], columns=case[1], types=case[2])


def setup(case):
    """Weights, boards, the two CPU forwards, the net and its device outputs: computed once per case."""
    if case not in _cache:
        n = 3 if case[4] == 256 else 130
        w, b = net_ref.make_weights(case), net_ref.make_boards(case, n)
        net = ElementCrushNet(cfg_of(case), case[3], case[4], w)
        values, logits = net.forward(b)
        _cache[case] = dict(w=w, boards=b, n=n, f64=net_ref.forward_f64(case, w, b), model=net_ref.forward_model(case, w, b),
                            net=net, values=values, logits=logits)
    return _cache[case]


@pytest.fixture(scope="module", autouse=True)
def close_nets():
    yield
    for s in _cache.values():
        s["net"].close()
    _cache.clear()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def device_forward(net, boards, need=None, fill=None):
    """forward_device on freshly uploaded arrays; the outputs start as `fill` where given."""
    ctx, n = net._ctx, len(boards)
    b = np.ascontiguousarray(np.asarray(boards).reshape(n, -1), dtype=np.int8)
    v0 = np.full(n, np.nan if fill is None else fill, np.float32)
    l0 = np.full((n, net.A), np.nan if fill is None else fill, np.float32)
    d_b, d_v, d_l = ctx.device_array(b), ctx.device_array(v0), ctx.device_array(l0)
    d_n = ctx.device_array(np.ascontiguousarray(need, dtype=np.uint8)) if need is not None else None
    net.forward_device(d_b, n, d_v, d_l, d_need=d_n)
    out = d_v.to_host(np.float32, (n,)), d_l.to_host(np.float32, (n, net.A))
    for d in (d_b, d_v, d_l, d_n):
        if d is not None:
            d.free()
    return out


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_stem_bit_for_bit(case):
    s = setup(case)
    got = s["net"].trunk(s["boards"], 0)
    assert got.shape == s["boards"].shape + (case[4],)
    assert np.array_equal(bits(got), bits(net_ref.stem_model(case, s["w"], s["boards"])))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_forward_against_the_model(case):
    s = setup(case)
    for key in ("values", "logits"):
        scale = np.max(np.abs(s["f64"][key]))
        e = net_ref.err(s["model"][key], s["f64"][key])
        d = float(np.max(np.abs(s[key].astype(np.float64) - s["model"][key])) / scale)
        print(f"{case_id(case)} {key}: d = {d:.3e}, e(model) = {e:.3e}, d / e(model) = {d / e:.4f}")
        assert np.isfinite(s[key]).all()
        assert d <= e, (key, d, e)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_trunk_after_every_layer(case):
    s = setup(case)
    for k in range(case[3] + 1):
        got = s["net"].trunk(s["boards"], k).astype(np.float64)
        f64, model = s["f64"]["trunk"][k], s["model"]["trunk"][k]
        e = net_ref.err(model, f64)
        d = float(np.max(np.abs(got - model)) / np.max(np.abs(f64)))
        print(f"{case_id(case)} trunk {k}: d = {d:.3e}, e(model) = {e:.3e}")
        assert d <= e, (f"layer {k}", d, e)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_batch_invariance_bit_for_bit(case):
    s = setup(case)
    net, b, n = s["net"], s["boards"], s["n"]
    i = 77 if n > 77 else n - 1
    want_v, want_l = bits(s["values"][i]), bits(s["logits"][i])
    v, lg = net.forward(b[i:i + 1])                       # alone
    assert np.array_equal(bits(v[0]), want_v) and np.array_equal(bits(lg[0]), want_l)
    v, lg = net.forward(np.stack([b[i], b[0], b[1]]))     # first of three
    assert np.array_equal(bits(v[0]), want_v) and np.array_equal(bits(lg[0]), want_l)
    assert np.array_equal(bits(v[1]), bits(s["values"][0])) and np.array_equal(bits(lg[2]), bits(s["logits"][1]))
    # a need mask: the needed rows are what they are without one
    need = (np.arange(n) % 3 != 1).astype(np.uint8)
    mv, ml = device_forward(net, b, need=need, fill=-7.0)
    on = need.astype(bool)
    assert np.array_equal(bits(mv[on]), bits(s["values"][on])) and np.array_equal(bits(ml[on]), bits(s["logits"][on]))
    # two calls in a row
    v2, l2 = net.forward(b)
    assert np.array_equal(bits(v2), bits(s["values"])) and np.array_equal(bits(l2), bits(s["logits"]))


@pytest.mark.parametrize("case", [CASES[0], CASES[3]], ids=case_id)
def test_forward_equals_forward_device(case):
    s = setup(case)
    dv, dl = device_forward(s["net"], s["boards"])
    assert np.array_equal(bits(dv), bits(s["values"])) and np.array_equal(bits(dl), bits(s["logits"]))
    v, lg = s["net"].forward(np.zeros((0, case[0], case[1]), np.int8))
    assert v.shape == (0,) and lg.shape == (0, s["net"].A)
    assert s["net"].trunk(np.zeros((0, case[0], case[1]), np.int8), 0).shape == (0, case[0], case[1], case[4])
    value, policy = s["net"](s["boards"][:2])  # the reference model's calling convention
    assert value.shape == (2, 1) and policy.shape == (2, s["net"].A)
    assert np.array_equal(bits(value[:, 0]), bits(s["values"][:2])) and np.array_equal(bits(policy), bits(s["logits"][:2]))


def test_unsupported_features_is_refused_by_the_library():
    import ctypes
    ctx = _native.context(9, 9, 6)
    blob, h = np.zeros(16, np.float32), ctypes.c_void_p()
    rc = _native.lib().m3_net_create(ctx.handle, 9, 9, 6, 0, 48, 1e-5, _native.ptr(blob), blob.size, ctypes.byref(h))
    assert rc == -2 and not h.value
    rc = _native.lib().m3_net_create(ctx.handle, 9, 9, 6, 0, 32, 1e-5, _native.ptr(blob), blob.size, ctypes.byref(h))
    assert rc == -1 and not h.value  # a blob of the wrong length


# ---- the guided search with the network as its evaluator ---------------------------------------------------------
RESULT_INT = ("best_action", "value", "root_visits", "n_children", "flags")
RESULT_CHILD = ("child_action", "child_visits", "child_value_sum", "child_prior")


def assert_same_result(a, b, what):
    for k in RESULT_INT:
        assert np.array_equal(a[k], b[k]), (what, k)
    for k in RESULT_CHILD:
        for g, c in enumerate(a["n_children"]):
            assert np.array_equal(a[k][g][:c].view(np.uint32), b[k][g][:c].view(np.uint32)), (what, k, g)


def roots(case, count, moves=6):
    out, seed = [], 1
    while len(out) < count:
        st = BoardV2(moves, BoardConfig(rows=case[0], columns=case[1], types=case[2], seed=seed))
        if st.legal_actions:
            out.append(st)
        seed += 1
    return out


def run_both(net, states, sims=12):
    """net= against evaluator=net.forward: every result field, then after advance() and a second run."""
    dev = DeviceSearchNN(states, sims, net=net, node_capacity=2 + 2 * sims)
    fed = DeviceSearchNN(states, sims, evaluator=lambda boards, need: net.forward(boards), node_capacity=2 + 2 * sims)
    results = []
    for call in range(2):
        dev.run()
        fed.run()
        a, b = dev.result(), fed.result()
        assert_same_result(a, b, f"call {call}")
        results.append(a)
        if (a["flags"] != 0).any():
            break
        sa, sb = dev.advance(None), fed.advance(None)
        assert all(np.array_equal(x.array, y.array) and x.n_actions == y.n_actions for x, y in zip(sa, sb))
    st = dev.stats()
    assert st["host_feeds"] == 0 and st["linear_evals"] == 0 and st["device_feeds"] == 2 + st["rounds"]
    dev.close()
    fed.close()
    return results


@pytest.mark.parametrize("case,games", [(CASES[0], 8), (CASES[3], 4)], ids=["9x9x6", "7x5x4"])
def test_search_with_the_net_equals_the_host_fed_search(case, games):
    s = setup(case)
    results = run_both(s["net"], roots(case, games))
    assert len(results) == 2 and (results[0]["root_visits"] > 0).all()
    assert not (results[0]["flags"] & _native.FLAG_BAD_EVAL).any()


def test_search_freezes_on_an_infinite_weight_as_the_host_fed_path_does():
    case = CASES[0]
    s = setup(case)
    states = roots(case, 8)
    a = states[0].legal_actions[0]
    w = dict(s["w"])
    k = w["policy_head.dense.kernel"].copy()
    k[5, a] = np.inf
    w["policy_head.dense.kernel"] = k
    net = ElementCrushNet(cfg_of(case), case[3], case[4], w)
    try:
        results = run_both(net, states)
        fl = results[0]["flags"]
        assert fl[0] & _native.FLAG_BAD_EVAL  # the root of game 0 has action a legal
    finally:
        net.close()


def test_search_refuses_a_net_of_another_shape():
    import ctypes
    s9, s7 = setup(CASES[0]), setup(CASES[3])
    with pytest.raises(ValueError, match="board shape"):
        DeviceSearchNN(roots(CASES[0], 2), 4, net=s7["net"])
    ds = DeviceSearchNN(roots(CASES[0], 2), 4, net=s9["net"])  # (and the library itself)
    assert _native.lib().m3_search_nn_run_net(ds._h, 1, s7["net"].handle) == -1
    assert _native.lib().m3_search_nn_run_net(ds._h, 1, ctypes.c_void_p()) == -1
    ds.close()


def test_batch1_facade_with_a_net():
    """NeuralNetworkMCTS with a net returns what it returns with the equivalent host evaluator."""
    from match3tile.mcts import NeuralNetworkMCTS
    from match3tile.samplers import nn_mcts_episodes

    case = CASES[0]
    net = setup(case)["net"]
    root = roots(case, 1, moves=4)[0]
    calls = []

    def model(x):
        calls.append(x.shape)
        return net(x)
    dev, host = NeuralNetworkMCTS(net, root, 3, 10), NeuralNetworkMCTS(model, root, 3, 10)
    for call in range(2):
        assert dev() == host(), call
    assert calls and all(c == (1, 9, 9) for c in calls)
    seeds = [21, 22, 23]
    a = nn_mcts_episodes(seeds, net=net, moves=2, simulations=6)
    b = nn_mcts_episodes(seeds, evaluator=lambda boards, need: net.forward(boards), moves=2, simulations=6)
    assert np.array_equal(a, b)
