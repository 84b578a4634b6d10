"""The host env model (env_model.py) pinned before it judges the kernels -- no GPU needed.

1. The reference's recorded env runs (tests/golden/env.npz, every tag, run and step).
2. The staggered autoreset walk of Oracle.batch_episodes (test_autoreset_staggered_trace_vs_oracle).
3. The three schedules of test_gpu_env_schedule.py through the model alone: the preconditions that
   make the GPU runs mean something (queues non-empty in every shard range at every step, seeds that
   wrap and land on 0, every step kind, bad actions and terminal boards), from the model only.
"""
import os

import numpy as np
import pytest

import crafted
import env_model as em
from conftest import GOLDEN, SHAPES
from oracle import FLAG_BAD_ACTION, FLAG_SHUFFLE_CAP, FLAG_TERMINAL, Oracle

with np.load(os.path.join(GOLDEN, "env.npz")) as _g:
    ENV_TAGS = sorted({k[len("moves_"):] for k in _g.files if k.startswith("moves_")})


@pytest.mark.parametrize("tag", ENV_TAGS)
def test_model_replays_reference_env_runs(golden, tag):
    """Every run and step of the fixture: the README loop over the real reference (gen_golden.py,
    gen_env), autoreset off, a reset with the recorded argument at every done step (-1: reset()
    without a seed starts the same seed again, env.py:62)."""
    g = golden("env")
    shape = tuple(int(x) for x in tag.split("x"))
    act, obs, rew = g["action_" + tag], g["obs_" + tag], g["reward_" + tag]
    done, trunc = g["done_" + tag], g["trunc_" + tag]
    arg, robs, after = g["reset_arg_" + tag], g["reset_obs_" + tag], g["seed_after_" + tag]
    resets = 0
    for i in range(len(g["seed_" + tag])):
        m = em.EnvModel(1, shape, num_moves=int(g["moves_" + tag][i]), env_goal=int(g["goal_" + tag][i]),
                        autoreset=False)
        m.reset([g["seed_" + tag][i]])
        assert (m.board[0] == g["init_" + tag][i]).all(), i
        fresh = True
        for t in range(act.shape[1]):
            # the loop plays np.random.choice(legal) from the global stream: behind a step that is
            # the model's pre-drawn action (behind a reset the stream stands after the board's
            # draws, where the env's first action reseeds: samplerTasks.py:11-13)
            assert fresh or m.next_action[0] == act[i, t], (i, t)
            fresh = False
            m.step(act[i, t:t + 1])
            assert (m.board[0] == obs[i, t]).all(), (i, t)
            assert m.reward[0] == rew[i, t] and m.done[0] == bool(done[i, t]) and m.trunc[0] == bool(trunc[i, t]), (i, t)
            assert (arg[i, t] != -2) == bool(m.done[0])
            if m.done[0]:
                m.reset([m.seed[0] if arg[i, t] < 0 else arg[i, t]])
                assert (m.board[0] == robs[i, t]).all(), (i, t)
                assert m.score[0] == 0 and m.moves[0] == 0
                resets += 1
                fresh = True
            assert int(m.seed[0]) == int(after[i, t]), (i, t)
    assert resets > 0


@pytest.mark.parametrize("tag", list(SHAPES))
def test_model_equals_staggered_batch_episodes(tag):
    """Random policy, autoreset on, 3-move episodes with env_goal 20, stride n: the walk of
    test_autoreset_staggered_trace_vs_oracle over Oracle.batch_episodes, 256 boards, 12 steps."""
    shape = SHAPES[tag]
    n, base, moves, goal, steps = 256, 100, 3, 20, 12
    o = Oracle(*shape, episode_shuffle_cap=1024)
    eps = [o.batch_episodes(np.arange(base + e * n, base + (e + 1) * n, dtype=np.uint32), moves, goal)
           for e in range(steps)]
    A, R, D = (np.stack([ep[k] for ep in eps]) for k in ("actions", "rewards", "draws"))  # [episode, board, move]
    assert not (np.stack([ep["flags"] for ep in eps]) & FLAG_SHUFFLE_CAP).any()
    model = em.EnvModel(n, shape, num_moves=moves, env_goal=goal, autoreset=True, seed_stride=n)
    model.reset(np.arange(base, base + n, dtype=np.uint32))
    b = np.arange(n)
    e = np.zeros(n, np.int64)
    m = np.zeros(n, np.int64)
    score = np.zeros(n, np.int64)
    for t in range(steps):
        assert (model.next_action == A[e, b, m]).all(), f"step {t}: actions"
        model.step()
        r = R[e, b, m]
        score += r
        tr = score >= goal
        dn = tr | (m + 1 == moves)
        assert (model.reward == r).all(), f"step {t}: rewards"
        assert (model.draws == D[e, b, m]).all(), f"step {t}: draws"
        assert (model.done == dn).all() and (model.trunc == tr).all(), f"step {t}: done / truncated"
        e, m, score = e + dn, np.where(dn, 0, m + 1), np.where(dn, 0, score)
        assert (model.score == score).all() and (model.moves == m).all(), f"step {t}: score / moves"
        assert (model.seed == (base + b + e * n).astype(np.uint32)).all(), f"step {t}: seeds"
    assert model.resets == e.sum() and e.min() >= steps // moves and e.max() > e.min()


def _run(cfg, ops, shape, on_step=None, on_call=None):
    """A schedule through the model alone. on_step(t, model, op) after every step, on_call(model, op,
    before) around every other call (before = True ahead of it)."""
    model = em.EnvModel(cfg["n"], shape, num_moves=cfg["num_moves"], env_goal=cfg["env_goal"],
                        autoreset=cfg["autoreset"], seed_stride=cfg["seed_stride"])
    model.reset(cfg["seeds"])
    t = 0
    for op in ops:
        if op[0].startswith("step"):
            # (a greedy step plays the pre-drawn action here: the lookahead of every board on the host
            # costs minutes, and nothing below depends on which legal action such a step plays)
            model.step(em.s3_actions(model, op) if len(op) > 1 else None)
            if on_step:
                on_step(t, model, op)
            t += 1
            continue
        if on_call:
            on_call(model, op, True)
        if op[0] == "autoreset":
            model.set_autoreset(op[1], op[2])
        elif op[0] == "set":
            model.set_field(op[1], em.s3_set_values(model, op[2]))
        elif op[0] == "reset":
            model.reset(op[1])
        if on_call:
            on_call(model, op, False)
    return model, t


S1_MIN_SHARE = 0.05


@pytest.mark.parametrize("shape", list(em.S1_CASES), ids=lambda s: "x".join(map(str, s)))
def test_schedule1_preconditions(shape):
    """Shards change mid-run. (a) Some shard slot >= 1 sits out 1, 2 and 3 steps modulo CBLOCKS
    (its counter blocks come back stale) and once a multiple of it. (b) At every step at least 5 %
    of the boards of every current shard range finish, so each stale prefetch count of (a) would
    have been non-zero."""
    cblocks = crafted.NSLOT  # CBLOCKS = PF_LAG + 1 = NSLOT (m3_kernels.hpp)
    assert cblocks == 4
    n, _, _, _, shards_at = em.S1_CASES[shape]
    gaps = em.s1_absences(n, shards_at)
    assert any({1, 2, 3} <= {g % cblocks for g in gs} and any(g % cblocks == 0 for g in gs) for gs in gaps.values()), gaps
    timeline = em.s1_timeline(shards_at)
    assert all(cnt > 0 for k in set(timeline) for _, cnt in em.shard_ranges(n, k))
    cfg, ops = em.schedule1(shape)
    low = [1.0]

    def on_step(t, model, op):
        for off, cnt in em.shard_ranges(n, timeline[t]):
            share = model.done[off:off + cnt].mean()
            low[0] = min(low[0], share)
            assert share >= S1_MIN_SHARE, (t, off, cnt, share)

    model, steps = _run(cfg, ops, shape, on_step)
    assert steps == em.S1_STEPS and model.reset_flags == 0
    print(f"schedule 1 {shape}: lowest share of finished boards in a shard range {low[0]:.3f}, "
          f"{model.resets} resets, slot gaps {gaps}")


@pytest.mark.parametrize("tag", list(SHAPES))
def test_schedule2_preconditions(tag):
    """Autoreset and stride change mid-run: a seed wraps past 2^32, a reset lands on seed 0, boards
    are done at the step before and the step after every set_autoreset call, every board is
    mid-episode or freshly reset at the stride change, done boards are stepped on while autoreset
    is off, and the episodes end at every length."""
    shape = SHAPES[tag]
    cfg, ops = em.schedule2(shape)
    seen = dict(wrap=0, zero=0, stepped_done=0, lengths=set(), after=[], before=[], pending=False)
    prev = {}

    def on_step(t, model, op):
        if prev:
            reset = model.done & model.autoreset
            seen["wrap"] += int((reset & (model.seed < prev["seed"])).sum())
            seen["zero"] += int((reset & (model.seed == 0)).sum())
            if not model.autoreset:
                seen["stepped_done"] += int(prev["done"].sum())
            seen["lengths"] |= set((prev["moves"][reset] + 1).tolist())
        if seen["pending"]:
            seen["after"].append(int(model.done.sum()))
            seen["pending"] = False
        prev.update(seed=model.seed.copy(), done=model.done.copy(), moves=model.moves.copy())

    def on_call(model, op, before):
        if before:
            seen["before"].append(int(model.done.sum()))
            seen["pending"] = True
            if model.autoreset and op[1] and op[2] != model.stride:  # the stride change
                assert ((model.moves >= 0) & (model.moves < model.num_moves)).all()
                assert (model.moves[model.done] == 0).all()

    model, steps = _run(cfg, ops, shape, on_step, on_call)
    assert steps == sum(em.S2_TIMELINE)
    assert len(seen["before"]) == 4 and len(seen["after"]) == 4
    assert min(seen["before"]) > 0 and min(seen["after"]) > 0, seen
    assert seen["wrap"] >= 1 and seen["zero"] >= 1 and seen["stepped_done"] >= 1, seen
    assert seen["lengths"] >= set(range(1, em.S2_MOVES + 1)), seen["lengths"]
    assert model.reset_flags == 0
    print(f"schedule 2 {tag}: {seen['wrap']} wraps, {seen['zero']} resets onto seed 0, done before the calls "
          f"{seen['before']} and after {seen['after']}, {seen['stepped_done']} steps of done boards, "
          f"episode lengths {sorted(seen['lengths'])}, {model.resets} resets")


@pytest.mark.parametrize("tag", list(SHAPES))
def test_schedule3_preconditions(tag):
    """Every way to step at least twice, bad actions, terminal no-op steps, and every call between
    steps at its place."""
    shape = SHAPES[tag]
    cfg, ops = em.schedule3(shape)
    kinds = [op[0] for op in ops if op[0].startswith("step")]
    assert all(kinds.count(k) >= 2 for k in em.S3_KINDS), kinds
    calls = [op[0] for op in ops if not op[0].startswith("step")]
    assert calls == ["stateless", "eager_legal", "timing", "shards", "set", "set", "set", "reset"]
    reset_at = [i for i, op in enumerate(ops) if op[0] == "reset"][0]
    assert sum(op[0].startswith("step") for op in ops[:reset_at]) % 2 == 1  # an odd number of steps
    seen = dict(bad=0, terminal=0, resets_before=0)

    def on_step(t, model, op):
        seen["bad"] += int(((model.flags & FLAG_BAD_ACTION) != 0).sum())
        seen["terminal"] += int(((model.flags & FLAG_TERMINAL) != 0).sum())

    def on_call(model, op, before):
        if op[0] == "reset" and before:
            seen["resets_before"] = model.resets

    model, steps = _run(cfg, ops, shape, on_step, on_call)
    assert steps == em.S3_STEPS
    assert seen["bad"] >= 1 and seen["terminal"] >= 1 and seen["resets_before"] > 0 and model.resets > 0, seen
    assert model.reset_flags == 0
    print(f"schedule 3 {tag}: {seen['bad']} bad-action steps, {seen['terminal']} terminal steps, "
          f"{seen['resets_before']} resets before the mid-run reset, {model.resets} after")
