"""A stepwise host model of the batched env: n x Match3Env with same-step autoreset.

numpy and the C oracle only -- never the native library. Where Oracle.batch_episodes can only
say "seeded random policy, fixed stride, from reset", this model is stepped call by call, so a
run that mixes policies, changes the stride, overwrites one field or resets in the middle still has
something to be compared against. It restates env.py:48-56 as env_fin_begin / env_fin_store
(csrc/m3_kernels.hpp) do:

    n_actions = num_moves - moves;  apply_action + the seeded random action behind it
    score += reward;  moves += 1 (always: a terminal board and a bad action count too)
    trunc = score >= goal;  done = trunc or moves == num_moves
    autoreset and done:  seed += stride (mod 2^32), a fresh board of that seed, its first seeded
        action, score = moves = 0; reward, done, trunc and draws still show the finished step

test_env_model_cpu.py holds the model to the reference's recorded env runs and to
Oracle.batch_episodes before test_gpu_env_schedule.py lets it judge the kernels. The scripted
schedules both files run are defined at the end.
"""
from __future__ import annotations

import numpy as np

import crafted
from oracle import FLAG_BAD_ACTION, FLAG_NO_LEGAL, FLAG_TERMINAL, Oracle

FIELDS = ("board", "seed", "score", "moves", "next_action", "reward", "done", "trunc", "flags", "draws")
BLOCK = 256  # m3_env_set_shards cuts shards on multiples of the 256-board workgroup


class EnvModel:
    def __init__(self, n, shape, num_moves=20, env_goal=500, autoreset=True, seed_stride=None):
        self.n, self.shape = int(n), tuple(shape)
        self.o = Oracle(*shape)
        self.num_moves, self.goal = int(num_moves), int(env_goal)
        self.set_autoreset(autoreset, self.n if seed_stride is None else seed_stride)
        R, C = self.o.R, self.o.C
        self.board = np.zeros((n, R, C), np.int32)
        self.seed = np.zeros(n, np.uint32)
        self.score = np.zeros(n, np.int32)
        self.moves = np.zeros(n, np.int32)
        self.next_action = np.zeros(n, np.int32)
        self.reward = np.zeros(n, np.int32)
        self.done = np.zeros(n, bool)
        self.trunc = np.zeros(n, bool)
        self.flags = np.zeros(n, np.uint32)
        self.draws = np.zeros(n, np.uint32)
        self.resets = 0          # autoresets since the last reset()
        self.reset_flags = 0     # OR of the flags the resets of the run gave (0 for the shapes in use)

    def set_autoreset(self, enabled, stride):
        self.autoreset, self.stride = bool(enabled), int(stride) & 0xFFFFFFFF

    def _fresh(self, i, seed):
        """Match3Env.reset of board i; returns (draws of the board's reset, its reset flags)."""
        b, d = self.o.init_board(seed)
        first, _ = self.o.random_action(b, seed)
        self.board[i], self.seed[i], self.next_action[i] = b, seed, first
        self.score[i] = self.moves[i] = 0
        return d, (FLAG_NO_LEGAL if first < 0 else 0)

    def reset(self, seeds):
        seeds = np.asarray(seeds, dtype=np.uint32)
        assert seeds.shape == (self.n,)
        for i in range(self.n):
            self.draws[i], self.flags[i] = self._fresh(i, int(seeds[i]))
        self.reward[:] = 0
        self.done[:] = False
        self.trunc[:] = False
        self.resets = 0
        return self

    def step(self, actions=None):
        """One step of every board; actions None: each board's pre-drawn seeded action."""
        acts = self.next_action.copy() if actions is None else np.asarray(actions).astype(np.int64)
        assert acts.shape == (self.n,)
        o = self.o
        for i in range(self.n):
            seed = int(self.seed[i])
            nb, r, d, f, nxt, _ = o.apply_action_next(self.board[i], seed, int(acts[i]),
                                                      self.num_moves - int(self.moves[i]))
            stepped = not f & (FLAG_TERMINAL | FLAG_BAD_ACTION)
            if stepped and nxt < 0:
                f |= FLAG_NO_LEGAL
            score = int(self.score[i]) + r
            moves = int(self.moves[i]) + 1
            tr = score >= self.goal
            dn = tr or moves == self.num_moves
            self.reward[i], self.done[i], self.trunc[i] = r, dn, tr
            self.draws[i] = d if stepped else 0
            if dn and self.autoreset:
                _, rf = self._fresh(i, (seed + self.stride) & 0xFFFFFFFF)
                self.resets += 1
                self.reset_flags |= rf
                f |= rf
            else:
                self.board[i], self.score[i], self.moves[i], self.next_action[i] = nb, score, moves, nxt
            self.flags[i] = f
        return self

    def set_field(self, name, array):
        """m3_env_set: overwrite one field of every board."""
        assert name in FIELDS, name
        dst = getattr(self, name)
        dst[...] = np.asarray(array).reshape(dst.shape)

    def legal_bool(self):
        out = np.zeros((self.n, self.o.A), bool)
        for i in range(self.n):
            out[i, self.o.legal_actions(self.board[i])] = True
        return out

    def legal_words(self):
        return crafted.legal_words(self.legal_bool())


def shard_ranges(n, k):
    """[(offset, count)] of the k shards as m3_env_set_shards cuts them."""
    per = -(-(-(-n // k)) // BLOCK) * BLOCK
    offs = [min(n, s * per) for s in range(k)]
    return [(o, min(n, o + per) - o) for o in offs]


# ------------------------------------------------------------------------------------ schedules
# A schedule is a list of calls: the GPU test makes each on a BatchedMatch3Env and on the model, the
# CPU test on the model alone.
#   ("step",) ("step_host", actions) ("step_device", actions) ("step_greedy",)
#   ("shards", k) ("autoreset", enabled, stride) ("set", field, None or values) ("reset", seeds)
#   ("stateless",) ("eager_legal",) ("timing", capacity)
N_HEADLINE = 1992  # 8 * 256 - 56: eight non-empty shards, a ragged last shard, a ragged last wave

# Schedule 1: the shard count before step t (0-based; shards 2 from construction)
S1_STEPS = 32
S1_SHARDS = {5: 1, 6: 2, 10: 1, 12: 3, 15: 1, 18: 8, 20: 2, 24: 1, 28: 2}
S1_SHARDS_WIDE = {t: min(k, 2) for t, k in S1_SHARDS.items()}  # the 32 x 32 frame: one board per wave
# shape -> (n, num_moves, env_goal, seed_base, shard list)
S1_CASES = {
    (9, 9, 6): (N_HEADLINE, 3, 20, 100, S1_SHARDS),
    (16, 16, 8): (N_HEADLINE, 3, 20, 100, S1_SHARDS),
    (8, 8, 5): (N_HEADLINE, 3, 20, 100, S1_SHARDS),
    (20, 20, 6): (300, 3, 20, 100, S1_SHARDS_WIDE),
}


def s1_timeline(shards_at, steps=S1_STEPS, first=2):
    """The shard count in force at every step."""
    out, k = [], first
    for t in range(steps):
        k = shards_at.get(t, k)
        out.append(k)
    return out


def s1_absences(n, shards_at, steps=S1_STEPS, first=2):
    """For every shard slot >= 1: the lengths of the runs of steps it sat out between two steps it
    ran (a slot runs a step when the shard count gives it boards)."""
    tl = s1_timeline(shards_at, steps, first)
    out = {}
    for s in range(1, max(tl)):
        ran = [t for t, k in enumerate(tl) if s < k and shard_ranges(n, k)[s][1] > 0]
        gaps = [b - a - 1 for a, b in zip(ran, ran[1:]) if b - a > 1]
        if gaps:
            out[s] = gaps
    return out


def schedule1(shape):
    n, moves, goal, base, shards_at = S1_CASES[tuple(shape)]
    ops = []
    for t in range(S1_STEPS):
        if t in shards_at:
            ops.append(("shards", shards_at[t]))
        ops.append(("step",))
    cfg = dict(n=n, num_moves=moves, env_goal=goal, autoreset=True, seed_stride=n, shards=2,
               seeds=np.arange(base, base + n, dtype=np.uint32))
    return cfg, ops


# Schedule 2: autoreset and stride change mid-run, seeds wrap. Seeds 2^32 - 3n/2 + i: board n/2's
# first reset (stride n) lands on seed 0, the boards from n/2 on wrap at their first reset and the
# ones below at their second. (With the 2^32 - n/2 + i first thought of, no reset can land on 0:
# the seed after a resets of stride n and b of stride 3n + 1 is i - n/2 + a n + b (3n + 1) > 0.)
S2_MOVES = 6
S2_GOAL = {(9, 9, 6): 45, (16, 16, 8): 45}
S2_TIMELINE = (3, 6, 6, 3, 8)  # steps before, between and after the four set_autoreset calls


def schedule2(shape):
    n = N_HEADLINE
    seeds = ((2**32 - 3 * n // 2 + np.arange(n, dtype=np.int64)) % 2**32).astype(np.uint32)
    calls = [("autoreset", True, n), ("autoreset", True, 3 * n + 1), ("autoreset", False, 3 * n + 1),
             ("autoreset", True, 3 * n + 1)]
    ops = []
    for k, steps in enumerate(S2_TIMELINE):
        ops += [("step",)] * steps
        if k < len(calls):
            ops.append(calls[k])
    cfg = dict(n=n, num_moves=S2_MOVES, env_goal=S2_GOAL[tuple(shape)], autoreset=False, seed_stride=n, shards=2,
               seeds=seeds)
    return cfg, ops


# Schedule 3: every way to step, and the calls between steps (before step t, 0-based).
S3_STEPS = 36
S3_MOVES, S3_GOAL = 5, 60
S3_KINDS = ("step", "step_host", "step_device", "step_greedy")
S3_SAMPLE = 64  # boards whose lookahead is checked against the oracle before a greedy step
# The terminal boards: autoreset keeps moves below num_moves, so no board of this schedule would ever
# be stepped with n_actions < 1. One more m3_env_set of M3_ENV_MOVES, five steps ahead of the
# reset and one ahead of a greedy step, puts every seventh board at num_moves.
S3_CALLS = {3: ("stateless",), 6: ("eager_legal",), 9: ("timing", 3), 13: ("shards", 3), 17: ("set", "score", "plus7"),
            20: ("set", "moves", "zeros"), 22: ("set", "moves", "terminal7"), 27: ("reset", None)}


def schedule3(shape):
    n = N_HEADLINE
    A = Oracle(*shape).A
    rng = np.random.default_rng(303)
    ops = []
    for t in range(S3_STEPS):
        if t in S3_CALLS:
            c = S3_CALLS[t]
            if c[0] == "reset":
                c = ("reset", rng.integers(1, 2**32, size=n, dtype=np.uint64).astype(np.uint32))
            ops.append(c)
        kind = S3_KINDS[t % 4]
        if kind in ("step_host", "step_device"):
            # ids in [-1, A]: both ends are bad ids, most of the rest illegal swaps; "own" marks the
            # boards that play their pre-drawn legal action instead, so episodes keep scoring
            ops.append((kind, rng.integers(-1, A + 1, size=n).astype(np.int32), rng.random(n) < 0.5))
        else:
            ops.append((kind,))
    cfg = dict(n=n, num_moves=S3_MOVES, env_goal=S3_GOAL, autoreset=True, seed_stride=n, shards=2,
               seeds=np.arange(7000, 7000 + n, dtype=np.uint32))
    return cfg, ops


def s3_actions(model, op):
    """The action array of a step_host / step_device call: the scripted ids, or the board's own."""
    return np.where(op[2], model.next_action, op[1]).astype(np.int32)


def s3_set_values(model, what):
    if what == "plus7":
        return (model.score + 7).astype(np.int32)
    if what == "zeros":
        return np.zeros(model.n, np.int32)
    if what == "terminal7":
        return np.where(np.arange(model.n) % 7 == 0, model.num_moves, model.moves).astype(np.int32)
    raise ValueError(what)
