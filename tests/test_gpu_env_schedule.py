"""The batched env reconfigured while it runs, call by call against the host model (env_model.py).

Every other test fixes shards, autoreset, stride and the way of stepping when the env is built. The
env keeps state between steps that is keyed by exactly those settings -- per-shard counter blocks
rotated by step % CBLOCKS, shard-local prefetch queues, episode slots filled NSLOT - 1 steps ahead
with seed + k * stride, per-shard stats words -- so here they change mid-run:

  schedule 1  the shard count changes (m3_env_set_shards between steps);
  schedule 2  autoreset goes on and off and the stride changes, with seeds that wrap past 2^32;
  schedule 3  every way to step in turn, and m3_env_set, a reset, the stateless calls, the eager
              legal buffer and the timing ring between steps.

After every step every board's observation, reward, done, truncated, score, moves, seed, next
action, flags and draws equal the model's, and the legal sets every fourth step: bit for bit, no
tolerance anywhere. test_env_model_cpu.py pins the model and shows, from the model alone, that each
schedule reaches what it is meant to reach.
"""
import time

import numpy as np
import pytest

import env_model as em
import lookahead_ref
from conftest import SHAPES

pytestmark = pytest.mark.gpu

from match3tile import _native  # noqa: E402
from match3tile._native import check, lib, ptr  # noqa: E402
from match3tile.batched import BatchedMatch3Env  # noqa: E402

# the M3_FLAG_* bits of include/m3.h (bits 0x20..0x80 are the kernels' own: which pass computed a step)
PUBLIC_FLAGS = 0x1F | _native.FLAG_CASCADE_CAP | _native.FLAG_RESET_CAP
SET_IDS = {"score": _native.ENV_SCORE, "moves": _native.ENV_MOVES}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if _native.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")


def _ids(shape):
    return "x".join(map(str, shape))


class Run:
    """One env and one model fed the same calls; the model's CPU time is kept apart."""

    def __init__(self, shape, cfg):
        self.shape, self.cfg = shape, cfg
        self.model_s = 0.0
        self.t0 = time.perf_counter()
        self.env = BatchedMatch3Env(cfg["n"], *shape, num_moves=cfg["num_moves"], env_goal=cfg["env_goal"],
                                    seeds=cfg["seeds"], autoreset=cfg["autoreset"], seed_stride=cfg["seed_stride"],
                                    shards=cfg["shards"])
        self.model = em.EnvModel(cfg["n"], shape, num_moves=cfg["num_moves"], env_goal=cfg["env_goal"],
                                 autoreset=cfg["autoreset"], seed_stride=cfg["seed_stride"])
        self.timed(self.model.reset, cfg["seeds"])
        self.eager = False
        self.steps = 0
        self.compare("after the reset", legal=True)

    def timed(self, f, *a):
        t = time.perf_counter()
        r = f(*a)
        self.model_s += time.perf_counter() - t
        return r

    def compare(self, what, legal=False):
        env, m = self.env, self.model
        got = dict(board=env.observations(), reward=env.rewards(), done=env.dones(), trunc=env.truncateds(),
                   score=env.scores(), moves=env.moves(), seed=env.seeds(), next_action=env.next_actions(),
                   flags=env.flags() & PUBLIC_FLAGS, draws=env.draws())
        for k, g in got.items():
            w = getattr(m, k)
            bad = np.flatnonzero((g != w).reshape(m.n, -1).any(1))
            assert len(bad) == 0, (f"{what}: {k} of {len(bad)} boards, first {bad[:6]}: "
                                   f"got {g[bad[0]].tolist()}, want {w[bad[0]].tolist()}")
        if legal or self.eager:
            want = self.timed(m.legal_words)
            bad = np.flatnonzero((env.legal_bits() != want).any(1))
            assert len(bad) == 0, f"{what}: legal set of {len(bad)} boards, first {bad[:6]}"

    def step(self, op):
        env, m = self.env, self.model
        t = self.steps
        if op[0] == "step":
            env.step()
            self.timed(m.step)
        elif op[0] == "step_host":
            a = em.s3_actions(m, op)
            env.step(a)
            self.timed(m.step, a)
        elif op[0] == "step_device":
            a = em.s3_actions(m, op)
            d = env.ctx.device_array(a)
            env.step_device(d.ptr)
            env.synchronize()
            d.free()
            self.timed(m.step, a)
        elif op[0] == "step_greedy":
            la = env.lookahead()
            idx = np.arange(em.S3_SAMPLE) * (m.n // em.S3_SAMPLE)
            t1 = time.perf_counter()
            want = lookahead_ref.cached_lookahead(("schedule3", self.shape, t), self.shape, m.board[idx], m.seed[idx],
                                                  m.num_moves - m.moves[idx])
            self.model_s += time.perf_counter() - t1
            assert (la["best_action"][idx] == want["best_action"]).all(), f"step {t}: lookahead best_action"
            assert (la["best_reward"][idx] == want["best_reward"]).all(), f"step {t}: lookahead best_reward"
            env.step_greedy()
            self.timed(m.step, la["best_action"])
        else:
            raise ValueError(op)
        self.steps += 1
        self.compare(f"step {t} ({op[0]})", legal=t % 4 == 3)

    def stats_hold(self, what):
        st = self.env.stats()
        assert st["autoresets"] == self.model.resets, (what, st, self.model.resets)
        return st

    def finish(self, name):
        self.stats_hold("at the end")
        self.env.close()
        wall = time.perf_counter() - self.t0
        print(f"{name} {_ids(self.shape)}: {self.steps} steps of {self.model.n} boards, wall {wall:.2f} s = "
              f"model {self.model_s:.2f} s + rest {wall - self.model_s:.2f} s; {self.model.resets} autoresets")


@pytest.mark.parametrize("shape", list(em.S1_CASES), ids=_ids)
def test_schedule1_shards_change_mid_run(shape):
    """m3_env_set_shards between steps: 2, 1, 2, 1, 3, 1, 8, 2, 1, 2 shards over 32 steps of the
    staggered settings (3-move episodes, env_goal 20, stride n). Shard slot 1 sits out 1, 2, 3 and 4
    steps in turn; before the fix it came back with the counter blocks of its last steps unzeroed
    in all but the last case (stale continuation, overflow and prefetch counts), and its autoresets
    and recomputes dropped out of m3_env_stats while it sat out. Around every call the stats hold:
    autoresets equal the model's count, the recompute counts never decrease, shards is the new count."""
    cfg, ops = em.schedule1(shape)
    run = Run(shape, cfg)
    last = run.env.stats()
    for op in ops:
        if op[0] == "shards":
            before = run.stats_hold(f"before set_shards({op[1]}) at step {run.steps}")
            run.env.set_shards(op[1])
            after = run.stats_hold(f"after set_shards({op[1]}) at step {run.steps}")
            assert after["shards"] == op[1]
            for k in ("step_recomputes", "reset_recomputes"):
                assert last[k] <= before[k] <= after[k], (k, run.steps, last, before, after)
            last = after
        else:
            run.step(op)
    run.finish("schedule 1")


@pytest.mark.parametrize("tag", list(SHAPES))
def test_schedule2_autoreset_and_stride_change_mid_run(tag):
    """Built with autoreset off; 3 steps, autoreset on at stride n, 6 steps, stride 3n + 1, 6 steps,
    autoreset off (3 steps in which done boards are stepped on), on again, 8 steps -- on two shards,
    6-move episodes that end at every length, seeds 2^32 - 3n/2 + i: every board's seed wraps and board
    n/2 resets onto seed 0. A reset takes the seed plus the stride in force at that step, so each
    change has to rebuild the episodes queued ahead."""
    shape = SHAPES[tag]
    cfg, ops = em.schedule2(shape)
    run = Run(shape, cfg)
    for op in ops:
        if op[0] == "autoreset":
            run.env.set_autoreset(op[1], op[2])
            run.model.set_autoreset(op[1], op[2])
            run.stats_hold(f"after set_autoreset{op[1:]} at step {run.steps}")
            run.compare(f"after set_autoreset{op[1:]} at step {run.steps}")
        else:
            run.step(op)
    run.finish("schedule 2")


@pytest.mark.parametrize("tag", list(SHAPES))
def test_schedule3_every_step_kind_and_the_calls_between(tag):
    """step(), step(host actions in [-1, A]), step_device, step_greedy in turn for 36 steps of 5-move
    episodes (env_goal 60, autoreset on, two shards); before a greedy step the lookahead of 64 boards
    against the oracle, and the model is fed the device's picks. Between steps, each at a fixed step:
    the stateless apply_actions / legal_bits on the env's own context (checked against the oracle,
    the env unchanged), device_ptr(ENV_LEGAL) (from then on the eager legal buffer is compared every
    step), enable_timing(3), set_shards(3), m3_env_set of the scores alone (+ 7), of the moves alone
    (zeros; then every seventh board at num_moves: terminal no-op steps), and a reset with new seeds
    after an odd number of steps. The autoreset count holds through all of them and restarts at the
    reset."""
    shape = SHAPES[tag]
    cfg, ops = em.schedule3(shape)
    run = Run(shape, cfg)
    env, m = run.env, run.model
    for op in ops:
        what = f"{op[0]} before step {run.steps}"
        if op[0].startswith("step"):
            run.step(op)
            continue
        if op[0] == "stateless":
            idx = np.arange(0, m.n, 8)
            na = m.num_moves - m.moves[idx]
            r = env.ctx.apply_actions(m.board[idx], m.seed[idx], na, m.next_action[idx], legal=True, next_action=True)
            t1 = time.perf_counter()
            for j, i in enumerate(idx):
                nb, rew, d, f, nxt, _ = m.o.apply_action_next(m.board[i], int(m.seed[i]), int(m.next_action[i]), int(na[j]))
                assert (r["boards"][j] == nb).all() and r["reward"][j] == rew and r["draws"][j] == d, (what, i)
                assert r["flags"][j] & PUBLIC_FLAGS == f and r["next_action"][j] == nxt, (what, i)
            want = m.legal_words()
            run.model_s += time.perf_counter() - t1
            assert (env.ctx.legal_bits(m.board) == want).all(), what
        elif op[0] == "eager_legal":
            assert env.device_ptr(_native.ENV_LEGAL) != 0
            run.eager = True
        elif op[0] == "timing":
            env.enable_timing(op[1])
        elif op[0] == "shards":
            env.set_shards(op[1])
            assert env.stats()["shards"] == op[1]
        elif op[0] == "set":
            v = em.s3_set_values(m, op[2])
            check(lib().m3_env_set(env.handle, SET_IDS[op[1]], ptr(v)))
            m.set_field(op[1], v)
        elif op[0] == "reset":
            assert m.resets > 0
            run.stats_hold(what)
            env.reset(seeds=op[1])
            run.timed(m.reset, op[1])
            assert env.stats()["autoresets"] == 0
        else:
            raise ValueError(op)
        run.stats_hold("after " + what)
        run.compare("after " + what, legal=True)
    ms = env.kernel_ms()
    assert len(ms) == 3 and (ms > 0).all(), ms  # the timing ring took its three shard-steps and no more
    run.finish("schedule 3")
