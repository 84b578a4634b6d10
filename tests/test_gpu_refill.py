"""The two-part 9x9x6 refill (m3_rules.hpp refill) on the device against the oracle: seeded
episodes move by move, crafted boards whose first move clears 32, 33 and all 81 cells (the sizes
around the 32-tile stream: 33 and more take refill_loop), and rollouts."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from match3tile import _native  # noqa: E402
from match3tile.batched import BatchedMatch3Env  # noqa: E402
from oracle import FLAG_SHUFFLE_CAP, Oracle  # noqa: E402

BIG = 2**31 - 1
N, MOVES = 4096, 20
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refill.npz")


def test_seeded_episodes_move_by_move():
    """4,096 boards, seeds 1..4096, 20 seeded moves, no autoreset: board, reward, score, draws and
    next action after every move. Every board is compared (none of these episodes reaches the
    oracle's shuffle cap: asserted)."""
    if _native.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    seeds = np.arange(1, N + 1, dtype=np.uint32)
    o = Oracle(9, 9, 6)
    env = BatchedMatch3Env(N, 9, 9, 6, num_moves=MOVES, env_goal=BIG, seeds=seeds, autoreset=False)
    boards = env.observations().reshape(N, 9, 9).astype(np.int32)
    actions = env.next_actions().copy()
    score = np.zeros(N, np.int64)
    for mv in range(MOVES):
        want = [o.apply_action_next(boards[i], int(seeds[i]), int(actions[i]), MOVES - mv) for i in range(N)]
        assert not any(w[3] & FLAG_SHUFFLE_CAP for w in want), mv
        env.step()
        boards = np.array([w[0] for w in want], np.int32)
        score += np.array([w[1] for w in want])
        last = mv == MOVES - 1
        assert (env.observations().reshape(N, 9, 9) == boards).all(), mv
        assert (env.rewards() == np.array([w[1] for w in want])).all(), mv
        assert (env.scores() == score).all(), mv
        assert (env.draws() == np.array([w[2] for w in want])).all(), mv
        actions = np.array([w[4] for w in want], np.int32)
        if not last:  # (a finished episode without autoreset draws no further action)
            assert (env.next_actions() == actions).all(), mv
    env.close()


def test_crafted_first_moves_around_32_tiles():
    """tests/golden/refill.npz: 304 boards with first refills of 30..36 and 81 tiles, 100 of exactly
    32, 38 of exactly 33, 60 of all 81 (tests/test_refill_cpu.py pins the sizes to the rule code)."""
    g = np.load(GOLDEN)
    assert {32, 33, 81} <= set(g["need"].tolist()) and len(g["need"]) >= 300
    o = Oracle(9, 9, 6)
    ctx = _native.Context(9, 9, 6)
    res = ctx.apply_actions(g["boards"], g["seeds"], 20, g["actions"], next_action=True)
    for i in range(len(g["need"])):
        nb, r, d, f, nx, _ = o.apply_action_next(g["boards"][i].astype(np.int32), int(g["seeds"][i]),
                                                 int(g["actions"][i]), 20)
        assert (res["boards"][i] == nb).all(), i
        assert (res["reward"][i], res["draws"][i], res["next_action"][i]) == (r, d, nx), i
        assert (res["flags"][i] & 0x1F) == f, i
    ctx.close()


def test_rollouts():
    """4,096 rollouts of stepped boards against the oracle's."""
    seeds = np.arange(1, N + 1, dtype=np.uint32)
    ctx = _native.Context(9, 9, 6)
    boards, _, first = ctx.init_boards(seeds)
    res = ctx.apply_actions(boards, seeds, 20, first)
    rs = (np.arange(N, dtype=np.uint64) * 2654435761 + 7).astype(np.uint32)
    got = ctx.rollouts(res["boards"], seeds, 19, rs)
    want = Oracle(9, 9, 6).rollouts(res["boards"].astype(np.int32), seeds, 19, rs)
    assert (got["gain"] == want["gain"]).all()
    assert (got["steps"] == want["steps"]).all()
    assert (got["draws"] == want["draws"]).all()
    ctx.close()
