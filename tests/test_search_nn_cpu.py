"""The network-guided tree core (csrc/m3_search_nn_core.hpp) on the CPU, before a GPU sees it.

tests/search_nn_host builds the M3_HD functions the tree kernels call for the host; the step between
them is the C oracle's, the evaluator a Python function. Expected side: the Python model of
search_nn_ref.py, written from the documented semantics (tests/test_search_nn_golden_cpu.py holds the
model and this host build to the reference's own tree code). Every case of tests/test_gpu_search_nn.py
runs here first, compared as bit patterns; the score and the linear evaluator are checked on their own.
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "search_nn_host"))
import search_nn_host as nh  # noqa: E402
import search_nn_ref as ref  # noqa: E402
import search_ref  # noqa: E402

f32 = np.float32


def run_case(cs, record=None, spare=0):
    """A case as one lockstep HostSearchNN at exactly the capacity its calls need; checks every game of
    every call and re-roots at the best action. Returns (HostSearchNN, result lines)."""
    shape, n = cs["shape"], len(cs["roots"])
    o = search_ref.capped_oracle(shape)
    states = [search_ref.state(shape, r["board"], r["seed"], r["n_actions"], r["reward"]) for r in cs["roots"]]
    ev = ref.batch_evaluator(cs["ev"], n, o.A)
    hs = nh.HostSearchNN(o, states, 2 + cs["calls"] * cs["sims"] + spare, ev, record)
    lines = []
    for call in range(cs["calls"]):
        assert hs.run(cs["sims"]) == 0
        res = hs.result()
        lines += nh.result_lines(res)
        for g in range(n):
            ref.assert_game(res, g, cs["want"][g][call], (call,))
        act = [w[call].get("action", 0) if not w[call]["flags"] else 0 for w in cs["want"]]
        live = [g for g, w in enumerate(cs["want"]) if not w[call]["flags"] and w[call]["action"] >= 0]
        bad = hs.advance(act)[0]
        assert bad == n - len(live) - sum(1 for w in cs["want"] if w[call]["flags"])
    assert ev.state["calls"] == 2 + cs["calls"] * cs["sims"]
    return hs, lines


def test_case_a_ragged_workgroup():
    cs = ref.case_a()
    hs, _ = run_case(cs)
    assert all(not w[-1]["flags"] for w in cs["want"])
    assert max(hs.nodes_used(g) for g in range(18)) <= 2 + 3 * 20


def test_case_c_16x16x8():
    run_case(ref.case_c())


def test_case_d_frame_shape_7x5x4():
    o = search_ref.oracle((7, 5, 4))
    seeds = [s for s in range(1, 40) if o.legal_actions(o.init_board(s)[0])][:8]
    assert len(seeds) == 8
    run_case(ref.case_d(seeds))


def test_case_e_saturated_trees():
    cs = ref.case_e()
    hs, _ = run_case(cs)
    # terminal leaves were visited again (no node made in those rounds) and terminal children were made
    assert max(hs.nodes_used(g) for g in range(16)) < 2 + 2 * 40
    assert any(v > 1 for w in cs["want"] for _, v, _, _ in w[-1]["children"])


@pytest.mark.parametrize("which", ["constant", "negative"])
def test_case_f_ties_and_negative_logits(which):
    cs = ref.case_f(which)
    run_case(cs)
    if which == "negative":
        assert all(np.array(p, np.uint32).view(np.float32) < 0 for w in cs["want"] for _, _, _, p in w[-1]["children"])


def count_freezes(cs):
    """(dead roots, games frozen in a step, never frozen) from the Python model alone."""
    dead = [g for g, w in enumerate(cs["want"]) if w[-1]["flags"] == ref.F_NO_LEGAL and w[-1]["root_visits"] == 0
            and not w[-1]["children"]]
    step = [g for g, w in enumerate(cs["want"]) if w[-1]["flags"] & search_ref.F_STEP_FREEZE]
    live = [g for g, w in enumerate(cs["want"]) if not w[-1]["flags"]]
    return dead, step, live


def test_case_g_freezing_roots():
    cs = ref.case_g()
    dead, step, live = count_freezes(cs)
    assert len(dead) >= 1 and len(step) >= 1 and len(live) >= 32, (dead, step, len(live))
    run_case(cs)


def test_case_h_bad_evaluation_freezes_one_game():
    a, h = ref.case_a(), ref.case_h()
    for call in range(3):
        assert h["want"][ref.H_GAME][call]["flags"] == ref.F_BAD_EVAL
        for g in range(18):
            if g != ref.H_GAME:
                assert h["want"][g][call] == a["want"][g][call]
    # the tree as it stood: four simulations backed up, the fifth's node not linked
    assert h["want"][ref.H_GAME][0]["root_visits"] == 4
    run_case(h)


# ---- the legal-logit finiteness check (nn_store_row, the `bad` of nn_commit) ---------------------
def test_case_p_one_poisoned_legal_logit_freezes_exactly_that_game():
    """NaN / +inf / -inf at the lowest and the highest legal id, at a legal id >= 128 (the third pass
    over the row), at legal ids with id % 32 == 31 and == 0 (the word edges of the legal bits), in the
    roots' batch and in the construction's; FLT_MAX and a denormal, which are finite."""
    a, p = ref.case_a(), ref.case_p()
    poisons = p["poisons"]
    assert set(poisons) == set(ref.POISON_KINDS), sorted(set(ref.POISON_KINDS) - set(poisons))  # every condition exists
    trace = ref.trace_case_a()
    assert len({g for g, _, _, _ in poisons.values()}) == len(poisons)
    for kind, (g, rnd, i, v) in poisons.items():
        legal = trace[(g, rnd)][1]
        assert i in legal and p["ev"](trace[(g, rnd)][0], g, rnd)[1].view(np.uint32)[i] == ref.bits(v), kind
        freezes = ref.POISON_KINDS[kind][4]
        assert freezes == (not np.isfinite(v)), kind
        call0 = max(0, rnd - 2) // p["sims"]  # the call whose result first shows it
        for call in range(3):
            w = p["want"][g][call]
            if call < call0:
                assert w == a["want"][g][call], (kind, call)
            else:
                assert w["flags"] == (ref.F_BAD_EVAL if freezes else 0), (kind, call, hex(w["flags"]))
    g, rnd, i, _ = poisons["nan_lowest"]
    assert i == trace[(g, rnd)][1][0] and rnd >= 2
    g, rnd, i, _ = poisons["pinf_highest"]
    assert i == trace[(g, rnd)][1][-1] and rnd >= 2 + p["sims"]  # in the second call: the first is clean
    assert p["want"][g][0]["flags"] == 0 and p["want"][g][1]["root_visits"] >= 1
    assert poisons["ninf_ge128"][2] >= 128 and poisons["ninf_ge128"][1] >= 2
    assert poisons["nan_mod31"][2] % 32 == 31 and poisons["nan_mod0"][2] % 32 == 0
    assert poisons["nan_mod31"][1] >= 2 and poisons["nan_mod0"][1] >= 2
    # the roots' batch: no child, no visit; the construction's: the child never linked, the tree as it stood
    for kind, rnd in (("nan_roots", 0), ("ninf_construction", 1)):
        g = poisons[kind][0]
        assert poisons[kind][1] == rnd and g >= 16, kind  # (in the ragged second workgroup of the device)
        assert all(w == dict(children=[], root_visits=0, flags=ref.F_BAD_EVAL) for w in p["want"][g]), kind
    # a simulation round: the tree as it stood, the rounds before it backed up
    g, rnd = poisons["nan_lowest"][:2]
    assert p["want"][g][0]["root_visits"] == rnd - 2 and len(p["want"][g][0]["children"]) >= 1
    # finite, however large or small: the tree goes on (and is the model's, not case A's)
    assert any(p["want"][poisons[k][0]] != a["want"][poisons[k][0]] for k in ("fltmax", "denormal"))
    # every other game is untouched
    others = set(range(18)) - {g for g, _, _, _ in poisons.values()}
    assert len(others) == 9 and all(p["want"][g] == a["want"][g] for g in others)
    run_case(p)


def test_case_q_illegal_logits_are_never_read():
    """NaN and +-inf at every illegal id of every needed row of every round: nothing freezes and every
    tree equals clean case A bit for bit."""
    a, q = ref.case_a(), ref.case_q()
    trace = ref.trace_case_a()
    (g, rnd), (board, legal) = next(iter(trace.items()))
    row = q["ev"](board, g, rnd)[1]
    assert all(np.isfinite(row[i]) == (i in legal) for i in range(144)) and 0 < len(legal) < 144
    assert q["want"] == a["want"] and all(not w[-1]["flags"] for w in q["want"])
    run_case(q)


def test_case_r_infinite_weight_of_the_linear_evaluator():
    """W[cell][x][j] = +inf: the games whose evaluated boards hold x at the cell where j is legal freeze,
    the ones that hold it only where j is illegal and the ones that never hold it equal case A."""
    a, r = ref.case_a(), ref.case_r()
    cell, x, j, frozen, hit_only, missed = ref.pick_infinite_weight()
    assert len(frozen) >= 3 and len(hit_only) >= 2 and len(missed) >= 2
    assert [g for g in range(18) if r["want"][g][-1]["flags"]] == frozen
    assert all(r["want"][g][-1]["flags"] == ref.F_BAD_EVAL for g in frozen)
    assert all(r["want"][g] == a["want"][g] for g in hit_only + missed)
    run_case(r)
    # the host build of the device's evaluator gives the model's infinity (and NaN once -inf is added to it)
    L = nh.lib()
    W = r["W"].copy()
    board = np.full(81, x, np.int8)
    for trial in range(2):
        value, logits = np.zeros(1, np.float32), np.zeros(144, np.float32)
        L.nh_linear(nh._p(board), nh._p(W), 81, W.shape[1], 144, nh._p(value), nh._p(logits))
        wv, wl = ref.linear_eval(W, board)
        assert ref.bits(value[0]) == ref.bits(wv) and np.array_equal(logits.view(np.uint32), wl.view(np.uint32))
        assert (np.isnan(wl[j]) if trial else wl[j] == np.inf) and np.isfinite(np.delete(wl, j)).all()
        W[cell + 1, x, j] = -np.inf


def test_capacity_and_order_of_calls():
    cs = ref.case_a()
    hs, _ = run_case(dict(cs, calls=1, want=[w[:1] for w in cs["want"]]), spare=19)  # one short of two runs
    assert hs.run(20) == -7
    res = hs.result()
    for g in range(18):  # (re-rooted: the previous root's best child is the root now)
        assert res["root_visits"][g] >= 1
    assert hs.run(19) == 0
    L = nh.lib()
    h = L.nh_create(1, 8, 81, 5, 144)
    assert L.nh_fits(h, 1) == -6
    L.nh_destroy(h)


# ---- the score, as bits ------------------------------------------------------------------------
def host_score(total, v, pv, c, prior):
    return f32(nh.lib().nh_score(float(f32(total)), int(v), int(pv), float(f32(c)), float(f32(prior))))


def fused_score(total, v, pv, c, prior):
    """What a fused multiply-add of w * e + mean would give (one rounding, from exact double arithmetic:
    the product of two f32 is exact in double, and the sum's double rounding is harmless for a search
    of pairs that differ)."""
    mean = f32(total) / f32(v)
    e = f32(math.sqrt(math.log(pv) / (1 + v)))
    w = f32(c) * f32(prior)
    return f32(float(w) * float(e) + float(mean))


def test_score_bits_on_crafted_triples():
    assert host_score(5.0, 0, 1, 3.0, 1.0) == np.inf            # v = 0: nothing else is evaluated
    assert host_score(np.nan, 0, 1, 3.0, np.nan) == np.inf
    rng = np.random.default_rng(5)
    fused_differs = negative = zero_c = 0
    for i in range(4000):
        v = int(rng.integers(1, 300))
        pv = v + int(rng.integers(0, 3000))
        total = f32(rng.standard_normal() * 37.0) * f32(v)
        c = f32(0.0) if i % 10 == 0 else f32(rng.integers(1, 21))
        prior = f32(rng.standard_normal() * 2.0)
        want = ref.score(total, v, pv, c, prior)
        got = host_score(total, v, pv, c, prior)
        assert ref.bits(got) == ref.bits(want), (total, v, pv, c, prior)
        negative += prior < 0
        zero_c += c == 0
        if c == 0:  # the product is still evaluated: a signed zero times e, added to the mean
            assert ref.bits(got) == ref.bits(f32(total) / f32(v) + f32(0.0) * prior * f32(1.0))
        fused_differs += ref.bits(fused_score(total, v, pv, c, prior)) != ref.bits(want)
    # the crafted set holds what it must: negative priors, c = 0, and triples a fused w * e + mean misrounds
    assert negative > 1000 and zero_c == 400 and fused_differs > 100, (negative, zero_c, fused_differs)


def test_score_pair_ordered_differently_when_fused():
    """Two siblings whose order under the separate roundings is the reverse of their order under a
    fused multiply-add: found by search from the model alone, then asked of the host core."""
    rng = np.random.default_rng(9)
    found = 0
    for _ in range(200000):
        v = int(rng.integers(1, 50))
        pv = v + int(rng.integers(1, 500))
        c, prior = f32(rng.integers(1, 21)), f32(rng.standard_normal())
        t1 = f32(rng.standard_normal() * 11.0) * f32(v)
        s1, f1 = ref.score(t1, v, pv, c, prior), fused_score(t1, v, pv, c, prior)
        if ref.bits(s1) == ref.bits(f1):
            continue
        # a sibling with prior 0 and the mean at the separate result: ties it exactly, not the fused one
        t2 = f32(s1) * f32(v)
        if f32(t2) / f32(v) != s1:
            continue
        s2 = ref.score(t2, v, pv, c, f32(0.0))
        assert ref.bits(s2) == ref.bits(s1)
        assert ref.bits(host_score(t1, v, pv, c, prior)) == ref.bits(host_score(t2, v, pv, c, 0.0))
        found += 1
        if found == 20:
            break
    assert found == 20


def test_linear_evaluator_bits():
    L = nh.lib()
    for shape, k in (((9, 9, 6), 1), ((7, 5, 4), 4), ((16, 16, 8), 3)):
        R, C, T = shape
        W = ref.weights(shape, k)
        N, CH, A = W.shape[0], W.shape[1], W.shape[2] - 1
        assert L.nh_onehot_width(T) == CH == ref.onehot_width(T)
        rng = np.random.default_rng(k)
        for trial in range(3):
            board = rng.integers(0, CH + 6 if trial else T, size=N).astype(np.int8)  # cells >= CH contribute nothing
            if trial == 2:
                board[:3] = 127  # the first cells among them: the sum starts at the first cell that counts
            value, logits = np.zeros(1, np.float32), np.zeros(A, np.float32)
            L.nh_linear(nh._p(board), nh._p(W), N, CH, A, nh._p(value), nh._p(logits))
            wv, wl = ref.linear_eval(W, board)
            assert ref.bits(value[0]) == ref.bits(wv)
            assert np.array_equal(logits.view(np.uint32), wl.view(np.uint32))


def test_search_nn_core_under_asan_ubsan(tmp_path):
    """The stand-alone program (its own main, ASan + UBSan, nothing preloaded) replays the recorded
    scenario of case A at exactly node_capacity, then one request beyond it, and must print the results
    of the Python run."""
    cs = ref.case_a()
    rec = []
    hs, lines = run_case(cs, record=rec)
    assert hs.run(1) == -7
    lines.append("refused 1")
    path = tmp_path / "scenario.txt"
    path.write_text(" ".join(map(str, rec)) + "\n")
    d = os.path.join(ROOT, "tests", "search_nn_host")
    subprocess.run(["make", "-C", d, "asan"], check=True, capture_output=True)
    r = subprocess.run([os.path.join(d, "build", "search_nn_asan"), str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and "checks ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    out = r.stdout.strip().splitlines()
    assert out[:-1] == lines
    assert f"3 results, 1 refused, " in out[-1] and f" of {2 + 3 * 20} nodes" in out[-1]


def test_new_translation_unit_recorded_with_the_pass_off():
    """m3_search_nn.hip is in the shipped library, compiled like m3_search.o: its recorded command line
    carries the flag that turns SIOptimizeVGPRLiveRange off."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import spill_audit
    from match3tile import _native
    dev, host = spill_audit.command_lines(_native.LIB_PATH)
    mine = [x for x in dev + host if "m3_search_nn.hip" in x]
    assert mine, "no command line of m3_search_nn.hip recorded in libm3.so"
    assert all(spill_audit.SAFETY_FLAG in x for x in mine), mine[:1]
