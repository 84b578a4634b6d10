"""Device one-ply lookahead (m3_lookahead, m3_env_lookahead, m3_env_step_greedy) on the MI355X.

Expected side of every test: the oracle lookahead of lookahead_ref.py (Oracle.legal_actions +
Oracle.apply_action, the reference's loop boardv2.py:209-218), the reference's greedy episodes
(mcts.npz gr_*), or a twin env stepped with the same actions from the host.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import crafted  # noqa: E402
import lookahead_ref as ref  # noqa: E402
from match3tile import _native  # noqa: E402
from match3tile.batched import BatchedMatch3Env  # noqa: E402
from match3tile.boardConfig import BoardConfig  # noqa: E402
from match3tile.boardv2 import BoardV2  # noqa: E402
from match3tile.samplers import greedy_actions, greedy_actions_device, greedy_episodes  # noqa: E402
from oracle import Oracle  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if _native.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")


def ids(s):
    return "x".join(map(str, s))


# ---- 1. stateless against the oracle, full tables ---------------------------------------------
def states_for(shape, golden):
    if shape == (9, 9, 6):  # 301 mid-episode states + the 32 gr_* states: 333, a ragged tail
        a, b = ref.mid_episode_states(shape, 301), ref.greedy_states(golden("mcts"))
        return {k: np.concatenate([a[k], b[k]]) for k in a}
    if shape == (16, 16, 8):
        return ref.mid_episode_states(shape, 96)
    if shape == (5, 5, 6):  # seeds 1..128 hold boards without a legal action: all of them, then the others
        st = ref.mid_episode_states(shape, 128)
        w = ref.cached_lookahead(("all", shape), shape, st["boards"], st["seeds"], st["n_actions"])
        dead = np.flatnonzero(w["counts"] == 0)
        assert 0 < len(dead) < 64
        pick = np.sort(np.concatenate([dead, np.flatnonzero(w["counts"] > 0)[: 64 - len(dead)]]))
        return {k: v[pick] for k, v in st.items()}
    return ref.mid_episode_states(shape, 64)


STATELESS = [(9, 9, 6), (16, 16, 8), (7, 7, 4), (10, 8, 5), (12, 12, 7), (6, 5, 15), (5, 5, 6)]


@pytest.mark.parametrize("shape", STATELESS, ids=ids)
def test_stateless_matches_oracle(shape, golden):
    st = states_for(shape, golden)
    assert len(st["seeds"]) == {(9, 9, 6): 333, (16, 16, 8): 96}.get(shape, 64)
    want = ref.cached_lookahead(("st", shape), shape, st["boards"], st["seeds"], st["n_actions"])
    if shape == (5, 5, 6):
        assert (want["counts"] == 0).any()
    ctx = _native.Context(*shape)
    try:
        got = ctx.lookahead(st["boards"], st["seeds"], st["n_actions"], values=True)
        ref.assert_equal(got, want, shape)
        dead = want["counts"] == 0
        assert (got["best_action"][dead] == -1).all() and (got["best_reward"][dead] == -1).all()
        assert (got["flags"][dead] & _native.FLAG_NO_LEGAL).all()
        # terminal states: every legal action is worth 0, the lowest id wins, nothing is drawn
        wt = ref.cached_lookahead(("term", shape), shape, st["boards"][:40], st["seeds"][:40], 0)
        gt = ctx.lookahead(st["boards"][:40], st["seeds"][:40], 0, values=True)
        ref.assert_equal(gt, wt, (shape, "terminal"))
        assert (gt["flags"] & _native.FLAG_TERMINAL).all() and (gt["last_draws"] == 0).all()
        live = wt["counts"] > 0
        assert (gt["best_reward"][live] == 0).all()
        assert (gt["best_action"][live] == np.argmax(wt["values"][live] >= 0, axis=1)).all()
        # n = 1 (every board alone equals its row of the batch: done for all in test_lane_position)
        g1 = ctx.lookahead(st["boards"][5:6], st["seeds"][5:6], st["n_actions"][5:6], values=True)
        ref.assert_equal(g1, {k: v[5:6] for k, v in want.items()}, (shape, "n=1"))
    finally:
        ctx.close()


def test_n0_and_every_output_null(golden):
    shape = (9, 9, 6)
    st = states_for(shape, golden)
    want = ref.cached_lookahead(("st", shape), shape, st["boards"], st["seeds"], st["n_actions"])
    ctx = _native.Context(*shape)
    L = _native.lib()
    try:
        assert L.m3_lookahead(ctx.handle, 0, None, None, None, None, None, None, None, None) == 0
        assert ctx.lookahead(np.zeros((0, 9, 9), np.int8), np.zeros(0, np.uint32), np.zeros(0, np.int32),
                             values=True)["values"].shape == (0, ctx.A)
        for n in (333, 40):  # the staged path and the zero-copy path
            b = np.ascontiguousarray(st["boards"][:n].reshape(n, -1))
            s = np.ascontiguousarray(st["seeds"][:n])
            na = np.ascontiguousarray(st["n_actions"][:n])
            names = ("best_action", "best_reward", "values", "last_draws", "flags")
            for skip in names + (None,):
                out = dict(best_action=np.full(n, -9, np.int32), best_reward=np.full(n, -9, np.int32),
                           values=np.full((n, ctx.A), -9, np.int32), last_draws=np.full(n, 9, np.uint32),
                           flags=np.full(n, 9, np.uint32))
                args = [None if k == skip else _native.ptr(out[k]) for k in names]
                _native.check(L.m3_lookahead(ctx.handle, n, _native.ptr(b), _native.ptr(s), _native.ptr(na), *args))
                for k in names:
                    if k != skip:
                        assert (out[k] == want[k][:n]).all(), (n, skip, k)
    finally:
        ctx.close()


# ---- 2. the exact pass ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(9, 9, 6), (16, 16, 8), (7, 7, 4)], ids=ids)
def test_fallback_on_crafted_boards(shape):
    rw = crafted.rows(shape)
    o = Oracle(*shape)
    want = ref.cached_lookahead(("crafted", shape), shape, rw["boards"], rw["seeds"], 20)
    dec = crafted.decode_table(o)
    cand = over = 0
    for i in range(len(rw["seeds"])):
        for a in np.flatnonzero(want["values"][i] >= 0):
            cand += 1
            over += crafted.first_scan_groups(o, rw["boards"][i], int(a), dec) > crafted.lcap(shape)
    past = int((want["draw_table"] > crafted.chain_limit(shape)).sum())
    at_max = ((want["values"] == want["best_reward"][:, None]) & (want["values"] >= 0)).sum(axis=1)
    tied = int((at_max > 1).sum())
    print(f"{ids(shape)}: {cand} candidates, {over} over the table, {past} past the chain, {tied} tied boards")
    assert cand == int(want["counts"].sum()) and over * 2 > cand
    if shape == (16, 16, 8):
        assert past >= 500
    assert tied > 0
    ctx = _native.Context(*shape)
    try:
        got = ctx.lookahead(rw["boards"], rw["seeds"], 20, values=True)  # all 400 boards in one call
    finally:
        ctx.close()
    ref.assert_equal(got, want, shape)


# ---- 3. the reference's greedy episodes ------------------------------------------------------------
def env_state(env):
    return dict(boards=env.observations(), reward=env.rewards(), done=env.dones(), trunc=env.truncateds(),
                score=env.scores(), moves=env.moves(), seeds=env.seeds(), flags=env.flags())


def assert_same_state(a, b, what):
    for k in a:
        assert (a[k] == b[k]).all(), (what, k, np.flatnonzero((a[k] != b[k]).reshape(len(a[k]), -1).any(axis=1))[:8])


def test_greedy_episodes_match_reference(golden):
    g = golden("mcts")
    seeds = np.asarray(g["gr_seed"], dtype=np.uint32)
    assert len(seeds) == 32
    kw = dict(num_moves=20, env_goal=2**31 - 1, seeds=seeds, autoreset=False)
    env, twin = BatchedMatch3Env(32, **kw), BatchedMatch3Env(32, **kw)
    try:
        for t in range(20):
            la = env.lookahead()
            assert (la["best_action"] == g["gr_actions"][:, t]).all(), t
            env.step_greedy()
            twin.step(g["gr_actions"][:, t])
            assert_same_state(env_state(env), env_state(twin), t)
        assert (env.scores() == g["gr_reward"]).all()
    finally:
        env.close()
        twin.close()
    assert (greedy_episodes(seeds) == g["gr_reward"]).all()


def test_greedy_actions_device_equals_host_loop(golden):
    g = golden("mcts")
    states = []
    for seed, acts in zip(g["gr_seed"], g["gr_actions"]):
        s = BoardV2(20, BoardConfig(seed=int(seed)))
        for a in acts[: int(seed) % 7]:
            s = s.apply_action(int(a))
        states.append(s)
    states.append(BoardV2(0, BoardConfig(seed=5)))  # terminal: the first legal action wins
    assert greedy_actions_device(states) == greedy_actions(states)
    live = states[:-1]
    np.random.seed(1)
    want = greedy_actions(live, sync_rng=True)
    want_next = np.random.randint(0, 2**31 - 1)
    np.random.seed(1)
    got = greedy_actions_device(live, sync_rng=True)
    assert got == want and np.random.randint(0, 2**31 - 1) == want_next
    assert greedy_actions_device([]) == []
    with pytest.raises(IndexError):
        greedy_actions_device([BoardV2(20, BoardConfig(rows=5, columns=7, seed=3))])


# ---- 4. autoreset and shards ---------------------------------------------------------------------
@pytest.mark.parametrize("shape,n,steps,sample", [((9, 9, 6), 1000, 12, 128), ((16, 16, 8), 200, 6, 128)],
                         ids=["9x9x6", "16x16x8"])
def test_autoreset_and_shards(shape, n, steps, sample):
    """num_moves = 5: at 9x9x6 every board resets twice through the prefetched episode slots."""
    pick = np.sort(np.random.default_rng(11).permutation(n)[:sample])
    runs = {}
    for shards in (1, 2):
        kw = dict(rows=shape[0], columns=shape[1], types=shape[2], num_moves=5, autoreset=True, shards=shards)
        env, twin = BatchedMatch3Env(n, **kw), BatchedMatch3Env(n, **kw)
        trace = []
        try:
            for t in range(steps):
                la = env.lookahead()
                obs, seeds, moves = env.observations(), env.seeds(), env.moves()
                want = ref.cached_lookahead(("env", shape, t), shape, obs[pick], seeds[pick], 5 - moves[pick])
                assert (la["best_action"][pick] == want["best_action"]).all(), (shards, t)
                assert (la["best_reward"][pick] == want["best_reward"]).all(), (shards, t)
                env.step_greedy()
                twin.step(la["best_action"])
                st = env_state(env)
                assert_same_state(st, env_state(twin), (shards, t))
                trace.append((la["best_action"], st))
            if shape == (9, 9, 6):
                assert env.stats()["autoresets"] >= 2 * n
        finally:
            env.close()
            twin.close()
        runs[shards] = trace
    for t, ((a1, s1), (a2, s2)) in enumerate(zip(runs[1], runs[2])):
        assert (a1 == a2).all(), t
        assert_same_state(s1, s2, ("shards", t))


# ---- 5. lane position ----------------------------------------------------------------------------
def test_lane_position_10x8x9():
    """The lane-interference repro shape: a board's result must not depend on the
    candidates that share its wave."""
    shape = (10, 8, 9)
    st = ref.mid_episode_states(shape, 64)
    want = ref.cached_lookahead(("st", shape), shape, st["boards"], st["seeds"], st["n_actions"])
    ctx = _native.Context(*shape)
    try:
        together = ctx.lookahead(st["boards"], st["seeds"], st["n_actions"], values=True)
        ref.assert_equal(together, want, "together")
        for i in range(64):
            alone = ctx.lookahead(st["boards"][i:i + 1], st["seeds"][i:i + 1], st["n_actions"][i:i + 1], values=True)
            for k in alone:
                assert (alone[k][0] == together[k][i]).all(), (i, k)
    finally:
        ctx.close()


# ---- 6. errors -----------------------------------------------------------------------------------
def test_errors():
    L = _native.lib()
    ctx = _native.Context(9, 9, 6)
    try:
        for n in (3, 300):  # zero-copy and staged
            b = np.ones((n, 81), np.int8)
            b[n - 1, 80] = -128  # a cell of 128
            s, na, out = np.ones(n, np.uint32), np.full(n, 20, np.int32), np.zeros(n, np.int32)
            rc = L.m3_lookahead(ctx.handle, n, _native.ptr(b), _native.ptr(s), _native.ptr(na), _native.ptr(out),
                                None, None, None, None)
            assert rc == -1, rc  # M3_ERR_INVALID
        h = ctypes.c_void_p()
        _native.check(L.m3_env_create(ctx.handle, 8, 20, 500, ctypes.byref(h)))
        assert L.m3_env_lookahead(h, None, None, None) == -6  # M3_ERR_STATE: before reset
        assert L.m3_env_step_greedy(h) == -6
        _native.check(L.m3_env_destroy(h))
    finally:
        ctx.close()
    wide = _native.Context(20, 20, 6)
    try:
        with pytest.raises(_native.M3Error) as e:
            wide.lookahead(np.ones((2, 20, 20), np.int8), [1, 2], 20)
        assert e.value.code == -2  # M3_ERR_UNSUPPORTED
    finally:
        wide.close()
