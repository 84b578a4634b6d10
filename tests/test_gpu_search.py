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
    """Eight workgroups of 16 games and a ragged ninth of 2, re-rooted twice."""
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


# ---- frozen games, the exact pass inside a round, roots that are no reset boards -----------------
# Expected side: search_ref.general_search, the reference's search over the oracle from any root,
# freezing where include/m3.h says a game freezes.
RESULT_KEYS = ("best_action", "value", "root_visits", "n_children", "child_action", "child_visits", "child_reward", "flags")


def device_roots(cs, games=None):
    """BoardV2 roots of a search_ref case: its boards, cfg seeds, n_actions and rewards."""
    R, C, T = cs["shape"]
    out = []
    for g in range(len(cs["roots"])) if games is None else games:
        r, st = cs["roots"][g], cs["states"][g]
        b = BoardV2(r["n_actions"], BoardConfig(rows=R, columns=C, types=T, seed=r["seed"]), np.asarray(st.array).astype(np.int64))
        b._reward = r["reward"]
        out.append(b)
    return out


def device_search(cs, games=None, rngs=None):
    """One DeviceSearch over the games of a case, at exactly the capacity its calls need."""
    return DeviceSearch(device_roots(cs, games), cs["sims"], rngs=rngs, node_capacity=2 + cs["calls"] * cs["sims"])


def run_call(ds, cs, call, games=None):
    games = list(range(len(cs["roots"])) if games is None else games)
    ds.run(ref.round_seeds(cs, call, games))
    res = ds.result()
    for j, g in enumerate(games):
        ref.assert_game(res, j, cs["want"][g][call], (cs["shape"], call, g))
    return res


def test_frozen_games_freeze_alone():
    """5x5x6, 64 games: 2 dead roots, 2 games frozen by a cap in an expansion's step and 8 in a playout
    (flag words 0x8, 0x4, and 0x4 / 0xc), 52 never. Every game on both calls; a game frozen in call 0
    reports the same arrays after call 1."""
    cs = ref.freeze_case()
    dead, step, playout, live = ref.freeze_kinds(cs)
    print(f"freeze case: {len(dead)} dead roots, {len(step)} frozen in a step, {len(playout)} in a playout, "
          f"{len(live)} never; flag words {sorted({hex(w[-1]['flags']) for w in cs['want'] if w[-1]['flags']})}")
    assert len(dead) >= 1 and len(step) >= 1 and len(playout) >= 1 and len(live) >= 40
    n = len(cs["roots"])
    ds = device_search(cs)
    for call in range(2):
        res = run_call(ds, cs, call)
        if call == 0:
            first = {k: res[k].copy() for k in RESULT_KEYS}
        else:
            for g in (g for g in range(n) if cs["want"][g][0]["flags"]):
                k = first["n_children"][g]
                for key in RESULT_KEYS:  # (child arrays: the root's n_children entries)
                    a, b = (x[key][g][:k] if x[key].ndim == 2 else x[key][g] for x in (first, res))
                    assert np.array_equal(a, b), (g, key)
        states = ds.advance(None)  # (a frozen game keeps its root: no bad action)
        for g, st in enumerate(states):
            assert st.n_actions == 6 - sum(not w["flags"] for w in cs["want"][g][:call + 1]), (g, call)
    assert ds.stats()["rounds"] == 24
    ds.close()


def test_call_maps_frozen_games_to_exceptions():
    """DeviceSearch.__call__: ValueError with a dead root in the batch, RuntimeError with a game frozen
    by a cap alone, the reference's tuples otherwise."""
    cs = ref.freeze_case()
    dead, _, _, live = ref.freeze_kinds(cs)
    capped = [g for g, w in enumerate(cs["want"]) if w[0]["flags"] == ref.F_SHUFFLE_CAP]
    both = [g for g, w in enumerate(cs["want"]) if w[0]["flags"] == ref.F_SHUFFLE_CAP | ref.F_NO_LEGAL]
    assert dead and capped and both and len(live) >= 5  # (both: a playout that went on past its cap)

    def rngs(games):
        return [random.Random(9000 + cs["roots"][g]["seed"]) for g in games]

    for games, error in ((live[:3] + dead[:1] + live[3:5], ValueError), (live[:3] + capped[:1] + live[3:5], RuntimeError),
                         (both[:1] + live[:3], RuntimeError)):
        ds = device_search(cs, games, rngs(games))
        with pytest.raises(error):
            ds()
        ds.close()
    games = live[:5]
    ds = device_search(cs, games, rngs(games))
    for call in range(2):
        assert ds() == [(cs["want"][g][call]["action"], cs["want"][g][call]["value"], cs["want"][g][call]["policies"])
                        for g in games], call
    ds.close()


@pytest.mark.parametrize("shape", [(9, 9, 6), (16, 16, 8)], ids=lambda s: "x".join(map(str, s)))
def test_exact_pass_inside_a_round(shape):
    """Roots painted with more match groups than the table holds: the expansions of their children
    leave k_apply for the exact pass, whose count k_search_attach adds up from a word k_search_select
    zeroes in front of every apply launch.

    Lower bound of apply_exact: the root children whose first scan has more groups than the table
    holds and goes through the table at all. The group count alone is no bound: get_matches fills the
    table only with a crossing cell or a run of six on the board, and a root's own legal swaps can take
    a cell out of the painted plus (9x9x6: 454 children with more than 6 groups, apply_exact 437)."""
    import crafted
    rw = crafted.rows(shape, n=64)
    idx = np.flatnonzero(rw["layout"] != crafted.PLAIN)[:40]
    assert len(idx) == 40
    roots = [dict(board=rw["boards"][i], seed=int(rw["seeds"][i]), n_actions=3, reward=0) for i in idx]
    cs = ref.case(shape, roots, 12, 1)
    ds = device_search(cs)
    res = run_call(ds, cs, 0)
    o, dec = ref.capped_oracle(shape), crafted.decode_table(ref.capped_oracle(shape))
    kids = [(rw["boards"][i], int(res["child_action"][g][j])) for g, i in enumerate(idx) for j in range(res["n_children"][g])]
    groups = sum(crafted.first_scan_groups(o, b, a, dec) > crafted.lcap(shape) for b, a in kids)
    over = sum(crafted.first_scan_groups(o, b, a, dec) > crafted.lcap(shape) and crafted.first_scan_takes_table(o, b, a, dec)
               for b, a in kids)
    st = ds.stats()
    print(f"{shape}: apply_exact {st['apply_exact']} (root children: {len(kids)}, with a first scan of more groups than "
          f"the table holds: {groups}, of those through the table: {over}), rollout_exact {st['rollout_exact']}")
    assert over > 0
    assert over <= st["apply_exact"] <= 40 * 13  # (one expansion per game and round, and the constructor's)
    assert st["rounds"] == 12
    ds.close()


def test_heterogeneous_roots():
    """Mid-episode roots with specials, n_actions 20..1 in one batch, non-zero root rewards, and two
    roots that are terminal when they are set: those keep no child (include/m3.h, m3_search_set_roots)."""
    cs = ref.hetero_case()
    ds = device_search(cs)
    res = run_call(ds, cs, 0)
    for g in (36, 37):
        assert (res["best_action"][g], res["n_children"][g], res["root_visits"][g], res["flags"][g]) == (-1, 0, 10, 0)
        assert res["value"][g] == cs["roots"][g]["reward"] > 0
    with pytest.raises(ValueError):  # __call__ refuses a terminal root
        ds()
    ds.close()


def test_advance_with_explicit_actions():
    """Three calls, each re-rooted at the last of the least-visited root children instead of the best."""
    cs = ref.advance_case()
    n = len(cs["roots"])
    o = ref.capped_oracle(cs["shape"])
    ds = device_search(cs)
    for call in range(3):
        run_call(ds, cs, call)
        want = [cs["want"][g][call] for g in range(n)]
        actions = [ref.least_visited_last(call, w) for w in want]
        assert any(a != w["action"] for a, w in zip(actions, want))
        states = ds.advance(actions)
        for g, st in enumerate(states):
            assert (st.n_actions, st.reward) == want[g]["next"], (call, g)
            assert np.array_equal(st.array, want[g]["next_board"]), (call, g)
            assert list(st._actions) == o.legal_actions(want[g]["next_board"]), (call, g)
    ds.close()


def raw_roots(cs):
    n = len(cs["roots"])
    boards = np.ascontiguousarray(np.stack([np.asarray(s.array).reshape(-1) for s in cs["states"]]), dtype=np.int8)
    return (boards, np.array([r["seed"] for r in cs["roots"]], np.uint32), np.array([r["n_actions"] for r in cs["roots"]], np.int32),
            np.array([r["reward"] for r in cs["roots"]], np.int32)), n


def raw_result(h, n, A, null=None):
    """m3_search_result into sentinel-filled buffers, output `null` (an index into RESULT_KEYS) absent."""
    out = dict(best_action=np.full(n, -77, np.int32), value=np.full(n, -77, np.int32), root_visits=np.full(n, -77, np.int32),
               n_children=np.full(n, -77, np.int32), child_action=np.full((n, A), -77, np.int32),
               child_visits=np.full((n, A), -77, np.int32), child_reward=np.full((n, A), -77, np.int64),
               flags=np.full(n, 0xABCD, np.uint32))
    _native.check(_native.lib().m3_search_result(h, *[None if j == null else _native.ptr(out[k])
                                                    for j, k in enumerate(RESULT_KEYS)]))
    return out


def untouched(a):
    """Every element still the sentinel raw_result and the advance buffers are filled with."""
    return bool((a == (0xABCD if a.dtype == np.uint32 else -77)).all())


def test_second_set_roots_drops_the_trees():
    """One m3_search, 64 games of 5x5x6 at capacity 2 + 12: a search that freezes some games, then
    m3_search_set_roots with other roots and a second search of 12 rounds, which fits only because the
    slots were given back; flags, statistics and the round count start again."""
    import ctypes
    first = ref.freeze_case()
    second = ref.case((5, 5, 6), ref.reset_roots(range(101, 165), 6), 12, 1)
    thawed = [g for g in range(64) if first["want"][g][0]["flags"] and not second["want"][g][0]["flags"]]
    assert thawed
    ctx, L = _native.context(5, 5, 6), _native.lib()
    h = ctypes.c_void_p()
    _native.check(L.m3_search_create(ctx.handle, 64, 2 + 12, ctypes.byref(h)))
    stats = np.zeros(4, np.uint64)
    for cs in (first, second):
        args, n = raw_roots(cs)
        _native.check(L.m3_search_set_roots(h, *[_native.ptr(a) for a in args]))
        seeds = np.ascontiguousarray(ref.round_seeds(cs, 0), dtype=np.uint32)
        _native.check(L.m3_search_run(h, 12, _native.ptr(seeds)))
        res = raw_result(h, n, ctx.A)
        for g in range(n):
            ref.assert_game(res, g, cs["want"][g][0], ("set_roots", cs["roots"][0]["seed"]))
        _native.check(L.m3_search_stats(h, _native.ptr(stats)))
        assert stats[1] == 12
        assert L.m3_search_run(h, 1, _native.ptr(seeds)) == -7  # the object is full again
    L.m3_search_destroy(h)


@pytest.mark.parametrize("shape,cuts", [((10, 8, 9), (0, 1, 16, 33)), ((12, 12, 7), (0, 16, 17))],
                         ids=["10x8x9-1+15+17", "12x12x7-16+1"])
def test_batch_composition_does_not_matter(shape, cuts):
    """A game's result does not depend on the games beside it or on its place in a workgroup of 16:
    the batch as a whole, and cut into separate searches of one game, a partial and a ragged group."""
    o = ref.capped_oracle(shape)
    seeds = [s for s in range(1, 80) if o.legal_actions(o.init_board(s)[0])][:cuts[-1]]
    assert len(seeds) == cuts[-1]
    cs = ref.case(shape, ref.reset_roots(seeds, 4), 10, 1)
    ds = device_search(cs)
    whole = run_call(ds, cs, 0)
    ds.close()
    for lo, hi in zip(cuts, cuts[1:]):
        games = list(range(lo, hi))
        ds = device_search(cs, games)
        part = run_call(ds, cs, 0, games)
        ds.close()
        for j, g in enumerate(games):
            k = whole["n_children"][g]
            for key in RESULT_KEYS:
                a, b = (x[key][i][:k] if x[key].ndim == 2 else x[key][i] for x, i in ((whole, g), (part, j)))
                assert np.array_equal(a, b), (g, key)


def test_wide_frame_20x20x6():
    """The 32 x 32 frame (a side above 16) under the tree kernels: 3 games against the reference."""
    cs = ref.case((20, 20, 6), ref.reset_roots([1, 2, 3], 2), 6, 1)
    ds = device_search(cs)
    run_call(ds, cs, 0)
    assert ds.stats()["rounds"] == 6
    ds.close()


def test_nullable_outputs():
    """m3_search_result with each of its eight outputs absent in turn, m3_search_advance on explicit
    actions with each of its four: what is present equals the call with everything present."""
    cs = ref.advance_case()
    n = len(cs["roots"])
    ctx = _native.context(*cs["shape"])
    actions = np.array([ref.least_visited_last(0, cs["want"][g][0]) for g in range(n)], np.int32)
    names = ("boards", "rewards", "n_actions", "legal")

    def advance(null):
        ds = device_search(cs)
        ds.run(ref.round_seeds(cs, 0))
        if null is None:
            full = raw_result(ds._h, n, ctx.A)
            for g in range(n):
                ref.assert_game(full, g, cs["want"][g][0], "nullable")
            for j in range(8):
                got = raw_result(ds._h, n, ctx.A, null=j)
                for i, k in enumerate(RESULT_KEYS):
                    if i == j:
                        assert untouched(got[k]), (j, k)
                    elif got[k].ndim == 2:  # (child arrays: the root's n_children entries are the contract)
                        assert all(np.array_equal(got[k][g][:c], full[k][g][:c]) for g, c in enumerate(full["n_children"])), (j, k)
                    else:
                        assert np.array_equal(got[k], full[k]), (j, k)
        out = dict(boards=np.full((n, ctx.N), -77, np.int8), rewards=np.full(n, -77, np.int32),
                   n_actions=np.full(n, -77, np.int32), legal=np.full((n, ctx.words), 0xABCD, np.uint32))
        _native.check(_native.lib().m3_search_advance(ds._h, _native.ptr(actions),
                                                      *[None if k == null else _native.ptr(out[k]) for k in names]))
        ds.run(ref.round_seeds(cs, 1))  # the search goes on from the new roots, whatever was asked for
        res = ds.result()
        for g in range(n):
            ref.assert_game(res, g, cs["want"][g][1], ("nullable", null))
        ds.close()
        return out

    full = advance(None)
    o = ref.capped_oracle(cs["shape"])
    for g in range(n):
        w = cs["want"][g][0]
        assert (full["n_actions"][g], full["rewards"][g]) == w["next"]
        assert np.array_equal(full["boards"][g], w["next_board"].reshape(-1))
        assert _native.bits_to_actions(full["legal"][g], ctx.A) == o.legal_actions(w["next_board"])
    for null in names:
        got = advance(null)
        for k in names:
            assert untouched(got[k]) if k == null else np.array_equal(got[k], full[k]), (null, k)
