"""The kernels' second ways to a result, made to run in known numbers (libm3.so on the MI355X).

Every step, rollout and stateless kernel keeps the first LCAP match groups of a scan in LDS, takes
a record of a global spill pool for more (LdsStore::put, an atomicAdd on the pool counter; 4096
records per shard and step, max(4096, n / 8) per rollout launch), and hands a board whose lane
finds the pool full -- or runs past its register MT19937 chain -- to k_env_fix / k_apply_fix /
k_rollout_fix, which recompute it with the full table in scratch and overwrite the row the first
kernel left behind. The stateless k_apply has no pool: every board past its table is recomputed.
The fixtures never fill the table and seeded play spills once in a thousand steps, so the boards
here are painted to (tests/crafted.py; what they are is checked on the CPU from the oracle alone,
tests/test_crafted_cpu.py). Replication makes the counts: a few hundred unique rows, the oracle
evaluated once per row, tiled to thousands -- which copy is recomputed depends on atomic order,
and every copy must equal the oracle bit for bit whatever the order.
"""
import numpy as np
import pytest

import crafted
from conftest import SHAPES

pytestmark = pytest.mark.gpu

from match3tile import _native  # noqa: E402
from match3tile.batched import BatchedMatch3Env  # noqa: E402
from oracle import Oracle  # noqa: E402

BIG = 2**31 - 1
MOVES = 3           # episode length of the env cases: a third of the rows finish on the crafted step
STRIDE = 1 << 20    # autoreset seed increment
POOL = crafted.POOL            # KS::SPILL_RECORDS per shard and step; rollout_spill_cap for n <= 32768
FIX_LANES = crafted.FIX_LANES  # the fix kernels' lanes; more work takes their grid-stride loop
EXTRA = crafted.NSLOT          # steps after the crafted one: one more than the prefetch queues are deep

ALL = dict(SHAPES, **{"8x8x5": (8, 8, 5)})  # (8x8x5: a frame shape -- the 16x16x8 table and chain)


@pytest.fixture(scope="module")
def ctxs():
    if _native.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    return {tag: _native.Context(*shape) for tag, shape in ALL.items()}


def _mix(shape, n_over, n_under, seed=1):
    """Row indices into crafted.rows(shape): n_over copies of rows with more first-scan groups than
    the LDS table holds, n_under of rows within it (plain and crafted), shuffled together."""
    rw = crafted.rows(shape)
    over = np.flatnonzero(rw["groups"] > crafted.lcap(shape))
    under = np.flatnonzero(rw["groups"] <= crafted.lcap(shape))
    idx = np.concatenate([crafted.replicate(rw, -(-k // len(ix)), ix, k)["src"] for ix, k in ((over, n_over), (under, n_under))])
    return np.random.default_rng(seed).permutation(idx)


# ---- stateless: k_apply -> k_apply_fix ---------------------------------------------------------
APPLY_CASES = {"wave+1": (65, 0), "1023": (1023, 257), "1024": (1024, 256), "1025": (1025, 255), "6144": (4700, 1444)}


@pytest.mark.parametrize("case", list(APPLY_CASES))
@pytest.mark.parametrize("tag", list(ALL))
def test_apply_over_the_table(ctxs, tag, case):
    """m3_apply_actions with legal sets and next actions on crafted rows. k_apply's table is LDS
    only (LdsTable, no pool), so EVERY row with more than LCAP groups in its first scan reaches
    k_apply_fix (FullMT + ArrayStore in scratch) -- by construction, the ABI exposes no counter:
    65 such rows (a full wave of overflowing lanes plus one), then exactly 1023 / 1024 / 1025
    among ordinary rows -- the fix kernel's 1024 lanes just not filled, filled, and one board into
    the second turn of its grid-stride loop -- and 6144 rows with 4700 (five turns)."""
    shape = ALL[tag]
    rw = crafted.rows(shape)
    st = crafted.oracle_steps(shape, rw)
    src = _mix(shape, *APPLY_CASES[case])
    L = crafted.lcap(shape)
    assert int((rw["groups"][src] > L).sum()) == APPLY_CASES[case][0]
    res = ctxs[tag].apply_actions(rw["boards"][src], rw["seeds"][src], 20, rw["actions"][src], legal=True,
                                  next_action=True)
    assert (res["boards"] == st["next"][src]).all()
    assert (res["reward"] == st["reward"][src]).all()
    assert (res["draws"] == st["draws"][src]).all()
    assert ((res["flags"] & 0x1F) == st["flags"][src]).all()
    assert (res["legal"] == crafted.legal_words(st["legal"])[src]).all()
    assert (res["next_action"] == st["next_action"][src]).all()


# ---- env: k_env_step / k_env_cont_grid -> k_env_fix --------------------------------------------
_traj = {}


def _trajectory(shape, i, mv0):
    """Row i of crafted.rows(shape), loaded with moves = mv0, over the crafted step and EXTRA
    seeded random steps of a 3-move autoreset env, by the oracle: per step a dict(reward, draws,
    flags, done, obs, next_action, seed, moves, score) of the env's state AFTER it (the next episode's on
    a finished step). Cached: every copy of a row shares it."""
    key = (shape, int(i), int(mv0))
    if key in _traj:
        return _traj[key]
    o = Oracle(*shape)
    rw = crafted.rows(shape)
    board, seed, mv, score = rw["boards"][i].astype(np.int32), int(rw["seeds"][i]), int(mv0), 0
    action = int(rw["actions"][i])
    out = []
    for _ in range(1 + EXTRA):
        nb, r, d, f, nx, _ = o.apply_action_next(board, seed, action, MOVES - mv)
        assert not f & 0x0F
        f |= 0x08 if nx < 0 else 0  # (M3_FLAG_NO_LEGAL: the env flags a step that leaves no move)
        mv, score = mv + 1, score + r
        done = mv == MOVES
        if done:  # same-step autoreset: BoardV2.__init__ of seed + stride and its first action
            seed = (seed + STRIDE) & 0xFFFFFFFF
            nb, mv, score = o.init_board(seed)[0], 0, 0
            ep = o.batch_episodes([seed], MOVES, BIG, threads=1)
            nx = int(ep["actions"][0, 0])
            assert nx == o.random_action(nb, seed)[0]
        out.append(dict(reward=r, draws=d, flags=f, done=done, obs=nb, next_action=nx, seed=seed, moves=mv, score=score))
        board, action = nb, nx
    _traj[key] = out
    return out


def _run_env(ctx, shape, src, shards, eager):
    """Load the rows src (moves 0, 1, 2 by position), play the crafted step with the rows' actions
    and EXTRA steps on the device-drawn ones, check every step against _trajectory. Returns the
    step_recomputes of the crafted step and everything read back (for the shards comparison)."""
    rw = crafted.rows(shape)
    st = crafted.oracle_steps(shape, rw)
    n = len(src)
    mv0 = (np.arange(n) % MOVES).astype(np.int32)
    keys, inv = np.unique(np.stack([src, mv0], 1), axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    tr = [_trajectory(shape, i, m) for i, m in keys]

    def want(t, field, dtype=np.int64):
        return np.array([x[t][field] for x in tr], dtype)[inv]

    env = BatchedMatch3Env(n, *shape, num_moves=MOVES, env_goal=BIG, seeds=False, autoreset=True,
                           seed_stride=STRIDE, shards=shards)
    s0 = env.state_dict()
    s0.update(boards=rw["boards"][src], seeds=rw["seeds"][src], score=np.zeros(n, np.int32), moves=mv0,
              next_action=np.full(n, -1, np.int32))
    env.load_state_dict(s0)
    if eager:
        assert env.device_ptr(_native.ENV_LEGAL) != 0
    # (a loaded env that has not stepped yet reports zeroed counters, not what its allocation held)
    assert env.stats() == dict(step_recomputes=0, reset_recomputes=0, autoresets=0, shards=shards)
    before = env.stats()["step_recomputes"]
    env.step(rw["actions"][src])
    rec = env.stats()["step_recomputes"] - before
    got = []
    for t in range(1 + EXTRA):
        if t:
            env.step()
        g = dict(reward=env.rewards(), draws=env.draws(), done=env.dones(), flags=env.flags(), obs=env.observations(),
                 next_action=env.next_actions(), seeds=env.seeds(), moves=env.moves(), scores=env.scores(),
                 legal=env.legal_bits(), trunc=env.truncateds())
        got.append(g)
        assert (g["reward"] == want(t, "reward")).all(), t
        assert (g["draws"] == want(t, "draws")).all(), t
        assert (g["done"] == want(t, "done", bool)).all(), t
        assert not g["trunc"].any() and ((g["flags"] & 0x1F) == want(t, "flags")).all(), t
        assert (g["scores"] == want(t, "score")).all(), t
        assert (g["moves"] == want(t, "moves")).all(), t
        assert (g["seeds"] == want(t, "seed")).all(), t
        assert (g["obs"] == np.array([x[t]["obs"] for x in tr])[inv]).all(), t
        assert (g["next_action"] == want(t, "next_action")).all(), t
        assert (g["legal"] == ctx.legal_bits(g["obs"])).all(), t
    # the crafted step once more, from the per-row oracle results (not through _trajectory)
    g, done = got[0], mv0 == MOVES - 1
    assert done.sum() > n // 4 and (~done).sum() > n // 2
    assert (g["reward"] == st["reward"][src]).all() and (g["draws"] == st["draws"][src]).all()
    assert (g["obs"][~done] == st["next"][src][~done]).all()
    assert (g["next_action"][~done] == st["next_action"][src][~done]).all()
    assert (g["legal"][~done] == crafted.legal_words(st["legal"])[src][~done]).all()
    s2 = (rw["seeds"][src][done] + np.uint32(STRIDE)).astype(np.uint32)
    fb, _, ff = ctx.init_boards(s2)
    assert (g["seeds"][done] == s2).all() and (g["obs"][done] == fb).all() and (g["next_action"][done] == ff).all()
    env.close()
    return rec, got


def _per_shard(shape, src, shards):
    """(S, chain): per shard the rows with more first-scan groups than LCAP, and in all the rows
    whose draws -- the next action's included -- pass the step kernel's chain
    (test_crafted_rows_and_the_rng_chain states the rule). Shards are m3_env_set_shards' ranges."""
    rw = crafted.rows(shape)
    st = crafted.oracle_steps(shape, rw)
    n = len(src)
    per = ((n + shards - 1) // shards + 255) // 256 * 256
    over = rw["groups"][src] > crafted.lcap(shape)
    S = [int(over[s * per:(s + 1) * per].sum()) for s in range(shards)]
    chain = int((st["draws_after"][src] > crafted.chain_limit(shape)).sum())
    return S, chain


@pytest.mark.parametrize("eager", [False, True], ids=["lazy_legal", "eager_legal"])
@pytest.mark.parametrize("tag", list(ALL))
def test_env_below_the_pool(ctxs, tag, eager):
    """2048 rows, about 1300 of them past the LDS table, with 1 and with 2 shards: every such row
    takes a spill record in k_env_step (its first scan) and keeps it through the cascade -- put and
    get for g >= LCAP with most lanes of a wave spilling at once, the merge of the plus' arm into a
    spill record -- and no lane finds the pool full (records, the continuations' included, stay
    below 4096 a shard). step_recomputes of the crafted step is therefore exactly the number of
    rows past the RNG chain: none at 9x9x6 (624 draws), the oracle's count at 16x16x8 and 8x8x5
    (227), where those rows go k_env_step -> ovf_list -> k_env_fix with table words in their staging
    row. A third of the rows finish on the crafted step (in k_env_step, in k_env_cont_grid or in
    k_env_fix: env_finish without a staging row); EXTRA more steps consume every prefetch queue
    entry those kernels wrote. The shard settings must agree on everything read back."""
    shape = ALL[tag]
    src = _mix(shape, 1300, 748)
    runs = {}
    for shards in (1, 2):
        S, chain = _per_shard(shape, src, shards)
        assert max(S) <= 2048 and sum(S) == 1300
        if crafted.chain_limit(shape) == 624:
            assert chain == 0
        elif tag in SHAPES:
            assert chain >= 20
        rec, got = _run_env(ctxs[tag], shape, src, shards, eager)
        print(f"{tag} below the pool, shards={shards}, eager={eager}: S={S} chain={chain} step_recomputes={rec}")
        assert rec == chain, (rec, chain)
        runs[shards] = got
    for a, b in zip(runs[1], runs[2]):
        for k in a:
            assert (a[k] == b[k]).all(), k


@pytest.mark.parametrize("eager", [False, True], ids=["lazy_legal", "eager_legal"])
@pytest.mark.parametrize("tag", list(ALL))
def test_env_pool_exhausted(ctxs, tag, eager):
    """One shard of 8192 rows, 6144 of them past the LDS table: the pool's 4096 records run out in
    k_env_step, every later lane gets rec >= pool_cap from LdsStore::put and appends itself to
    ovf_list, and k_env_fix's 1024 lanes take its grid-stride loop at least twice. At least
    S - 4096 rows are recomputed (more when continuations or later scans ask for a record too,
    plus the rows past the chain), at most all."""
    shape = ALL[tag]
    src = _mix(shape, 6144, 2048)
    S, chain = _per_shard(shape, src, 1)
    assert S == [6144]
    rec, _ = _run_env(ctxs[tag], shape, src, 1, eager)
    print(f"{tag} pool exhausted, eager={eager}: S={S} chain={chain} step_recomputes={rec} (bound {S[0] - POOL}..{len(src)})")
    assert S[0] - POOL >= 2 * FIX_LANES
    assert S[0] - POOL <= rec <= len(src), rec


@pytest.mark.parametrize("eager", [False, True], ids=["lazy_legal", "eager_legal"])
@pytest.mark.parametrize("tag", list(ALL))
def test_env_pool_boundary(ctxs, tag, eager):
    """Two shards with exactly 4096 rows past the LDS table each: k_env_step takes exactly the last
    record of each shard's pool, and a continuation (or a later scan of an ordinary row) that needs
    one finds the pool full. No bound on the counter below; the results are exact."""
    shape = ALL[tag]
    rw = crafted.rows(shape)
    half = [_mix(shape, 4096, 1024, seed=s) for s in (2, 3)]
    src = np.concatenate(half)
    S, chain = _per_shard(shape, src, 2)
    assert S == [POOL, POOL]
    rec, _ = _run_env(ctxs[tag], shape, src, 2, eager)
    print(f"{tag} at the boundary, eager={eager}: S={S} chain={chain} step_recomputes={rec}")
    assert chain <= rec <= len(src), rec


# ---- rollouts: k_rollout -> k_rollout_fix ------------------------------------------------------
def _first_scan_after_rollout_action(shape, src, rs):
    """Groups of the first scan of each rollout: the first action is drawn from the rollout seed
    (mcts.py:17) and changes two cells of the painted board."""
    o = Oracle(*shape)
    rw = crafted.rows(shape)
    dec = crafted.decode_table(o)
    g = np.zeros(len(src), np.int32)
    for j, (i, s) in enumerate(zip(src, rs)):
        a, _ = o.random_action(rw["boards"][i].astype(np.int32), int(s))
        g[j] = crafted.first_scan_groups(o, rw["boards"][i], a, dec)
    return g


def _check_rollouts(ctx, shape, src, rs, n_actions):
    rw = crafted.rows(shape)
    o = Oracle(*shape, episode_shuffle_cap=1024)
    got = ctx.rollouts(rw["boards"][src], rw["seeds"][src], n_actions, rs, final_boards=True)
    want = o.rollouts(rw["boards"][src].astype(np.int32), rw["seeds"][src], n_actions, rs)
    assert (got["gain"] == want["gain"]).all()
    assert (got["steps"] == want["steps"]).all()
    assert (got["draws"].astype(np.int64) == want["draws"]).all()
    assert ((got["flags"] & 0x1F) == (want["flags"] & 0x1F)).all()
    assert (got["final"].reshape(len(src), -1) == want["final"]).all()


@pytest.mark.parametrize("n_actions", [1, 3, 20])
@pytest.mark.parametrize("tag", list(SHAPES))
def test_rollouts_pool_exhausted(ctxs, tag, n_actions):
    """8192 rollouts from crafted boards, random rollout seeds, pool of 4096 records
    (rollout_spill_cap): more than 4096 of them still have more than LCAP groups in their first
    scan after the rollout's own first action (counted with the oracle), so at least that many
    less 4096 lanes find the pool full and are replayed from their first move by k_rollout_fix
    (FullMT x 2 + ArrayStore), through several turns of its grid-stride loop; a lane keeps its
    record for the whole rollout."""
    shape = SHAPES[tag]
    src = _mix(shape, 7000, 1192)
    rs = np.random.default_rng(5).integers(0, 2**31, size=len(src)).astype(np.uint32)
    g = _first_scan_after_rollout_action(shape, src, rs)
    spill = int((g > crafted.lcap(shape)).sum())
    print(f"{tag} rollouts n={len(src)}: {spill} first scans past the table")
    assert spill - POOL >= FIX_LANES
    _check_rollouts(ctxs[tag], shape, src, rs, n_actions)


@pytest.mark.parametrize("tag", list(SHAPES))
def test_rollouts_every_lane_spills(ctxs, tag):
    """1100 rollouts (18 waves, the last ragged), every first scan past the table after the
    rollout's first action: every lane of every wave takes a pool record at once; none is
    exhausted (pool 4096), so only rows past the chain reach k_rollout_fix."""
    shape = SHAPES[tag]
    rw = crafted.rows(shape)
    L = crafted.lcap(shape)
    cand = np.resize(np.flatnonzero(rw["groups"] > L + 1), 4000)
    rs = np.random.default_rng(6).integers(0, 2**31, size=len(cand)).astype(np.uint32)
    keep = np.flatnonzero(_first_scan_after_rollout_action(shape, cand, rs) > L)[:1100]
    assert len(keep) == 1100
    for n_actions in (1, 3, 20):
        _check_rollouts(ctxs[tag], shape, cand[keep], rs[keep], n_actions)


# ---- the dead-board shuffle's cap (tests/golden/cycling.npz) -----------------------------------
CAPPED = 0x04 | 0x10 | 0x08  # M3_FLAG_SHUFFLE_CAP | M3_FLAG_SHUFFLED, and M3_FLAG_NO_LEGAL: still dead


def _cycling(golden, times):
    g = golden("cycling")
    idx = np.tile(np.arange(len(g["seed_9x9x6"])), times)
    return {k[:-len("_9x9x6")]: g[k][idx] for k in g.files if k.endswith("_9x9x6")}


def test_cycling_boards_stateless_and_rollouts(ctxs, golden):
    """Dead boards that no shuffle revives (the reference hangs on them) through m3_apply_actions:
    the step stops after 1024 reseeded shuffles like the oracle (m3_rules.hpp SHUFFLE_CAP,
    m3_oracle.c:505-507) -- same board, reward and draws, FLAG_SHUFFLE_CAP | FLAG_SHUFFLED, no
    legal move and next action -1. This is the `~t` expectation that test_shuffle_golden leaves
    empty. A rollout from such a board stops where the oracle's does (no legal first action)."""
    c = _cycling(golden, 5)  # (more rows than a wave)
    n = len(c["seed"])
    assert n > 64
    ctx = ctxs["9x9x6"]
    res = ctx.apply_actions(c["board"], c["seed"], 20, c["action"], legal=True, next_action=True)
    assert (res["boards"] == c["next"]).all()
    assert (res["reward"] == c["reward"]).all() and (res["draws"] == c["draws"]).all()
    assert ((res["flags"] & 0x1F) == CAPPED).all()
    assert (res["next_action"] == -1).all() and not res["legal"].any()
    o = Oracle(9, 9, 6, episode_shuffle_cap=1024)
    rs = np.arange(11, 11 + n, dtype=np.uint32)
    for boards in (c["board"], c["next"]):
        got = ctx.rollouts(boards, c["seed"], 20, rs, final_boards=True)
        want = o.rollouts(boards.astype(np.int32), c["seed"], 20, rs)
        for k in ("gain", "steps", "draws"):
            assert (got[k].astype(np.int64) == want[k]).all(), k
        assert ((got["flags"] & 0x1F) == (want["flags"] & 0x1F)).all() and (got["flags"] & 0x08).all()
        assert (got["final"].reshape(n, -1) == want["final"]).all()


@pytest.mark.parametrize("shards", [1, 2])
def test_cycling_boards_in_the_env(ctxs, golden, shards):
    """The same boards loaded into an env: k_env_step pauses at the dead board and k_env_cont_grid
    runs the shuffle loop to its cap. Flags, board, reward and draws are the oracle's; the env is
    not stuck: it has no next action (-1, the oracle's: no legal move), and stepping on flags the
    bad action and leaves the board as it is, as the oracle's apply_action does."""
    c = _cycling(golden, 5)
    n = len(c["seed"])
    o = Oracle(9, 9, 6, shuffle_cap=1024)
    env = BatchedMatch3Env(n, 9, 9, 6, num_moves=20, env_goal=BIG, seeds=False, autoreset=True, seed_stride=STRIDE,
                           shards=shards)
    s0 = env.state_dict()
    s0.update(boards=c["board"], seeds=c["seed"], score=np.zeros(n, np.int32), moves=np.zeros(n, np.int32),
              next_action=np.full(n, -1, np.int32))
    env.load_state_dict(s0)
    env.step(c["action"])
    assert ((env.flags() & 0x1F) == CAPPED).all()
    assert (env.observations() == c["next"]).all()
    assert (env.rewards() == c["reward"]).all() and (env.draws() == c["draws"]).all()
    assert not env.dones().any() and (env.scores() == c["reward"]).all() and (env.seeds() == c["seed"]).all()
    want_next = np.array([o.random_action(b.astype(np.int32), int(s))[0] for b, s in zip(c["next"], c["seed"])])
    assert (want_next == -1).all() and (env.next_actions() == want_next).all()
    assert not env.legal_bits().any()
    for _ in range(2):
        env.step()
        nb, r, d, f = o.apply_action(c["next"][0].astype(np.int32), int(c["seed"][0]), -1, 19)
        assert f == 0x02 and r == 0 and (nb == c["next"][0]).all()
        assert ((env.flags() & 0x1F) == 0x02).all()
        assert (env.observations() == c["next"]).all() and (env.rewards() == 0).all()
        assert (env.next_actions() == -1).all() and (env.scores() == c["reward"]).all()
    env.close()
