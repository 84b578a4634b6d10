"""The golden step and shuffle fixtures through the ENV kernels (libm3.so on the MI355X).

tests/golden/steps.npz and shuffle.npz hold the hard boards -- mega and bomb combos, near-full
refills, 1,200 / 1,680 dead boards -- and test_gpu_parity.py runs them through the stateless
k_apply only. The env's step has code of its own for exactly those boards: k_env_step pauses a
cascade at CASCADE_LIMIT and at a dead board, k_env_cont_grid resumes it from a continuation
record (its own staging and the dead-board shuffle), k_env_fix redoes what ran past the RNG chain
or the group table. Here every fixture row is loaded into a BatchedMatch3Env (m3_env_set) and
stepped once with the fixture's action as a host action; the bar is the stateless tests' own:
bit-exact boards, rewards, raw-draw counts and flags, plus the env's pre-drawn next action and
legal set against the stateless kernels on the resulting board.
"""
import numpy as np
import pytest

from conftest import SHAPES

pytestmark = pytest.mark.gpu

from match3tile import _native  # noqa: E402
from match3tile.batched import BatchedMatch3Env  # noqa: E402
from oracle import FLAG_SHUFFLE_CAP, Oracle  # noqa: E402

BIG = 2**31 - 1
MOVES = 20
STRIDE = 1 << 20  # autoreset seed increment (keeps the next episodes' seeds apart from the fixture's)


@pytest.fixture(scope="module")
def ctxs():
    if _native.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    return {tag: _native.Context(*shape) for tag, shape in SHAPES.items()}


def _rows(g, name, tag):
    """The fixture's rows as (boards, seeds, n_actions, actions, next, reward, draws); rows with
    n_actions < 1 (2 of the step rows: a terminal board does not step) are left out -- an env
    has no such board; the stateless test keeps them."""
    seeds = g["seed_" + tag].astype(np.uint32)
    na = g["n_actions_" + tag].astype(np.int32) if "n_actions_" + tag in g else np.full(len(seeds), MOVES, np.int32)
    keep = na >= 1
    assert (~keep).sum() <= 2 and (na <= MOVES).all()
    if name == "steps":
        assert (na == 1).any()  # the last move of an episode stays in
    return tuple(a[keep] for a in (g["board_" + tag], seeds, na, g["action_" + tag].astype(np.int32),
                                   g["next_" + tag], g["reward_" + tag], g["draws_" + tag]))


@pytest.mark.parametrize("shards", [1, 2])
@pytest.mark.parametrize("autoreset", [False, True], ids=["noreset", "autoreset"])
@pytest.mark.parametrize("name", ["steps", "shuffle"])
@pytest.mark.parametrize("tag", list(SHAPES))
def test_env_step_on_golden_fixture(golden, ctxs, tag, name, autoreset, shards):
    g = golden(name)
    ctx = ctxs[tag]
    boards, seeds, na, acts, nxt, reward, draws = _rows(g, name, tag)
    n = len(seeds)
    env = BatchedMatch3Env(n, *SHAPES[tag], num_moves=MOVES, env_goal=BIG, seeds=False, autoreset=autoreset,
                           seed_stride=STRIDE, shards=shards)
    st = env.state_dict()  # (never reset: zeros)
    st.update(boards=boards, seeds=seeds, score=np.zeros(n, np.int32), moves=(MOVES - na).astype(np.int32),
              next_action=np.full(n, -1, np.int32))
    env.load_state_dict(st)
    assert (env.legal_bits() == ctx.legal_bits(boards)).all()
    env.step(acts)
    done = na == 1
    assert (env.dones() == done).all()
    assert not env.truncateds().any()
    assert (env.rewards() == reward).all()
    live = draws >= 0
    assert (env.draws()[live] == draws[live]).all()
    flags = env.flags()
    if name == "shuffle":
        # (every dead board of the fixture comes alive within the device's shuffle cap: no row is
        # set apart as in test_shuffle_golden, whose FLAG_SHUFFLE_CAP branch is empty too)
        assert (g["terminates_" + tag] == 1).all()
        assert not (flags & FLAG_SHUFFLE_CAP).any()
        assert (flags & _native.FLAG_SHUFFLED).sum() > 100
    # the stateless kernel on the same rows: the env's pre-drawn next action and legal set
    want = ctx.apply_actions(boards, seeds, na, acts, next_action=True)
    assert (want["boards"] == nxt).all() and (want["reward"] == reward).all()  # (test_apply_action_golden's bar)
    obs = env.observations()
    swapped = done & autoreset  # same-step autoreset: the observation is the next episode's board
    assert (obs[~swapped] == nxt[~swapped]).all()
    assert (env.next_actions()[~swapped] == want["next_action"][~swapped]).all()
    assert (env.legal_bits()[~swapped] == ctx.legal_bits(nxt)[~swapped]).all()
    assert (env.scores()[~swapped] == reward[~swapped]).all()
    assert (env.moves()[~swapped] == (MOVES - na + 1)[~swapped]).all()
    assert (env.seeds()[~swapped] == seeds[~swapped]).all()
    if swapped.any():
        # the finished rows (n_actions == 1) swapped in their next episode: seed + stride, fresh
        # board (the oracle's BoardV2.__init__), first action, zeroed counters
        s2 = (seeds[swapped] + np.uint32(STRIDE)).astype(np.uint32)
        fb, _, ff = ctx.init_boards(s2)
        o = Oracle(*SHAPES[tag])
        assert (env.seeds()[swapped] == s2).all()
        assert (obs[swapped] == fb).all()
        for i, s in zip(np.flatnonzero(swapped), s2):
            assert (obs[i] == o.init_board(int(s))[0]).all()
        assert (env.next_actions()[swapped] == ff).all()
        assert (env.legal_bits()[swapped] == ctx.legal_bits(fb)).all()
        assert (env.scores()[swapped] == 0).all() and (env.moves()[swapped] == 0).all()
    env.close()
