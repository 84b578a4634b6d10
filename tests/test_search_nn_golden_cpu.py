"""The network-guided search against the reference's own tree code.

tests/golden/search_nn.npz holds what ``NNNode`` / ``BaseNode.ucb1`` / ``BaseMCTS.__call__`` of the
reference computed over its own ``BoardV2`` (gen_golden_search_nn.py: numpy standing in for
``jax.numpy``, integer rewards handed over as Python ints so that numpy promotes as JAX does with x64
off; JAX itself was not run). Here the Python model of search_nn_ref.py and the host build of
csrc/m3_search_nn_core.hpp must equal that file in every field of every game and call, bit for bit;
tests/test_gpu_search_nn_golden.py asks the same of the device.
"""
import numpy as np
import pytest

import search_nn_golden as gold
import search_nn_ref as ref
import search_ref
from test_search_nn_cpu import nh, run_case

MODEL_KEYS = ("children", "root_visits", "flags", "action", "value", "policies")


@pytest.fixture(scope="module")
def data(golden):
    return golden("search_nn")


@pytest.mark.parametrize("name", gold.CASES)
def test_model_equals_the_reference_trees(data, name):
    cs = gold.load_case(data, name)
    got = ref.run_case(("golden", name), cs["shape"], cs["roots"], cs["sims"], cs["calls"], cs["ev"])
    assert len(got) == len(cs["want"])
    for g, (gw, ww) in enumerate(zip(got, cs["want"])):
        for call in range(cs["calls"]):
            a = {k: gw[call].get(k) for k in MODEL_KEYS}
            a["children"] = [tuple(int(x) for x in c) for c in a["children"]]
            assert a == ww[call], (name, g, call)


@pytest.mark.parametrize("name", gold.CASES)
def test_host_core_equals_the_reference_trees(data, name):
    """(The wide frame included: the host harness takes any N and A.)"""
    cs = gold.load_case(data, name)
    run_case(cs)


def test_cases_are_the_ones_of_the_model_module(data):
    """The file's cases A, C, D, E, F carry the constants of search_nn_ref.py, on the same roots."""
    o = search_ref.oracle((7, 5, 4))
    d_seeds = [s for s in range(1, 40) if o.legal_actions(o.init_board(s)[0])][:8]
    pairs = (("A", ref.case_a()), ("C", ref.case_c()), ("D", ref.case_d(d_seeds)), ("E", ref.case_e()),
             ("Fc", ref.case_f("constant")), ("Fn", ref.case_f("negative")))
    for name, mine in pairs:
        cs = gold.load_case(data, name)
        assert (cs["shape"], cs["sims"], cs["calls"]) == (mine["shape"], mine["sims"], mine["calls"]), name
        assert [(r["seed"], r["n_actions"], r["reward"]) for r in cs["roots"]] == \
               [(r["seed"], r["n_actions"], r["reward"]) for r in mine["roots"]], name
        so = search_ref.oracle(cs["shape"])
        assert all(np.array_equal(r["board"], so.init_board(r["seed"])[0]) for r in cs["roots"]), name
        if "W" in mine:
            assert np.array_equal(cs["W"], mine["W"]), name
    m, w = gold.load_case(data, "M"), gold.load_case(data, "W")
    assert [r["seed"] for r in m["roots"]] == list(range(1001, 1009)) and m["sims"] == 16 and m["calls"] == 2
    assert [7 - r["n_actions"] for r in m["roots"]] == [1 + g % 4 for g in range(8)]
    assert all(r["reward"] > 0 for r in m["roots"]) and len({r["reward"] for r in m["roots"]}) >= 6
    assert w["shape"] == (20, 20, 6) and len(w["roots"]) == 4 and (w["sims"], w["calls"]) == (8, 1)
    assert all(r["n_actions"] == 5 for r in w["roots"])


def test_mid_episode_roots_back_up_the_absolute_reward(data):
    """Case M holds what it is for: terminal leaves under roots with a reward, whose return is the
    state's reward and not the gain since the root."""
    cs = gold.load_case(data, "M")
    assert min(r["reward"] for r in cs["roots"]) > 0 and max(r["reward"] for r in cs["roots"]) > 100
    assert sorted({r["n_actions"] for r in cs["roots"]}) == [3, 4, 5, 6]
    for g, r in enumerate(cs["roots"]):  # the value is a state's reward: the root's own is in it
        assert all(w["value"] >= r["reward"] for w in cs["want"][g])
    assert any(w["value"] > cs["roots"][g]["reward"] for g in range(8) for w in cs["want"][g])
    # a child that terminal leaves were backed up into: its mean is beyond the root's reward, far beyond
    # what the evaluator's values (a sum of 81 standard normals) or the gain since the root could give
    heavy = [(g, call, c) for g in range(8) for call, w in enumerate(cs["want"][g]) for c in w["children"]
             if c[1] >= 2 and float(np.uint32(c[2]).view(np.float32)) / c[1] > cs["roots"][g]["reward"] > 100]
    assert heavy


def ulps(a, b):
    """|a - b| in units of the last place of float32 bit patterns of one sign."""
    return abs(int(a) - int(b))


def test_numpy_departs_from_float32_only_in_late_sums(data):
    """``A_numpy_*``: the same run with the reference's states as they are (rewards numpy.int64), which
    numpy 2 promotes to float64 where JAX keeps float32. The file documents where the two part ways:
    nowhere but in child sums, by one ulp, and only under roots with at most 2 moves left (where
    terminal leaves -- integer rewards -- have been backed up)."""
    keys = [k[len("A_numpy_"):] for k in data.files if k.startswith("A_numpy_")]
    assert "child_sum" in keys and len(keys) == len([k for k in data.files if k.startswith("A_") and
                                                     not k.startswith("A_numpy_")])
    for k in keys:
        if k != "child_sum":
            assert np.array_equal(data["A_" + k], data["A_numpy_" + k]), k
    a, b = data["A_child_sum"], data["A_numpy_child_sum"]
    nc, na = data["A_n_children"], data["A_n_actions"]
    differing = set()
    for g in range(a.shape[0]):
        for call in range(a.shape[1]):
            for j in range(int(nc[g, call])):
                x, y = a[g, call, j], b[g, call, j]
                assert (x >> 31) == (y >> 31) and ulps(x, y) <= 1, (g, call, j)
                if x != y:
                    differing.add((g, call))
                    assert int(na[g]) - call <= 2, (g, call)  # the root of call k has n_actions - k moves left
    assert differing, "the file no longer holds a departure: regenerate, and restate this test"
    assert len(differing) < a.shape[0]  # a few games, not a systematic shift


def test_linear_evaluator_is_the_one_the_file_was_made_with(data):
    triples = gold.evaluator_triples(data)
    assert {t[0] for t in triples} == {(9, 9, 6), (16, 16, 8), (7, 5, 4), (20, 20, 6)}
    for shape, wseed, board, value_bits, crc in triples:
        value, logits = ref.linear_eval(ref.weights(shape, wseed), board)
        assert ref.bits(value) == value_bits and gold.logits_crc(logits) == crc, (shape, wseed)
        assert logits.shape == (2 * shape[0] * (shape[1] - 1),)


def test_second_set_roots_on_a_live_host_tree(data):
    """Two calls of case A, then case M's roots (its 8 roots repeated over the 18 games) on the same
    pool: equal to the file -- and so to a fresh object -- bit for bit. The pool keeps the old trees' bytes."""
    a, m = gold.load_case(data, "A"), gold.load_case(data, "M")
    two = dict(a, calls=2, want=[w[:2] for w in a["want"]])
    hs, _ = run_case(two, spare=20)  # (capacity of the three calls case A has)
    n = len(a["roots"])
    roots = [m["roots"][g % 8] for g in range(n)]
    states = [search_ref.state(m["shape"], r["board"], r["seed"], r["n_actions"], r["reward"]) for r in roots]
    ev = ref.batch_evaluator(m["ev"], n, 144)
    hs.set_roots(states, ev)
    assert max(hs.nodes_used(g) for g in range(n)) <= 2
    for call in range(m["calls"]):
        assert hs.run(m["sims"]) == 0
        res = hs.result()
        for g in range(n):
            gold.assert_game(res, g, m["want"][g % 8][call], ("again", call))
        assert hs.advance([m["want"][g % 8][call]["action"] for g in range(n)])[0] == 0
    assert ev.state["calls"] == 2 + m["calls"] * m["sims"]
    assert nh.lib().nh_fits(hs.h, 62 - 1 - m["calls"] * m["sims"] - 1) == 0  # the bound restarted at the new roots
    assert nh.lib().nh_fits(hs.h, 62 - 1 - m["calls"] * m["sims"]) == -7
