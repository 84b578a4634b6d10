"""The one-ply lookahead core (csrc/m3_lookahead_core.hpp) on the CPU, before a GPU sees it.

tests/lookahead_host builds the M3_HD functions k_lookahead / k_lookahead_fix call -- candidate
enumeration, the packed key, the per-board fold and the hand-over to the exact pass -- for the
host and emulates a wave's rounds serially. Expected side: the oracle lookahead (lookahead_ref.py:
Oracle.legal_actions + Oracle.apply_action, the reference's loop boardv2.py:209-218).
"""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

import crafted
import lookahead_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "lookahead_host"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import lookahead_host as lh  # noqa: E402

CRAFTED_SHAPES = [(9, 9, 6), (16, 16, 8), (7, 7, 4)]


@pytest.mark.parametrize("shape", CRAFTED_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_host_core_matches_oracle_on_crafted_boards(shape):
    """crafted.rows: most candidates overflow the group table, so the hand-over to the exact pass
    and its fold carry most boards."""
    rw = crafted.rows(shape)
    h = lh.LookaheadHost(*shape)
    assert h.gcap() == crafted.lcap(shape) and h.chain_limit() == crafted.chain_limit(shape)
    want = ref.cached_lookahead(("crafted", shape), shape, rw["boards"], rw["seeds"], 20)
    got = h.lookahead(rw["boards"], rw["seeds"], 20, bpw=32 if shape == (9, 9, 6) else 8)
    cand, redo, boards_redone = got["stats"]
    assert cand == int(want["counts"].sum())
    assert redo * 2 > cand and boards_redone > 0, got["stats"]
    ref.assert_equal(got, want, shape)


@pytest.mark.parametrize("bpw", [1, 7, 16, 64])
def test_host_core_matches_oracle_on_greedy_states(golden, bpw):
    st = ref.greedy_states(golden("mcts"))
    want = ref.cached_lookahead("gr", (9, 9, 6), st["boards"], st["seeds"], st["n_actions"])
    got = lh.LookaheadHost(9, 9, 6).lookahead(st["boards"], st["seeds"], st["n_actions"], bpw=bpw)
    ref.assert_equal(got, want, bpw)
    g = golden("mcts")  # the picks continue the reference's greedy episodes
    for i, (seed, acts) in enumerate(zip(g["gr_seed"], g["gr_actions"])):
        assert got["best_action"][i] == acts[int(seed) % 7]


def test_terminal_and_dead_boards():
    """n_actions < 1: every legal action is worth 0, the lowest id wins, nothing is drawn. 5x5x6
    seeds 1..128 hold boards without a legal action: -1 / -1."""
    shape = (5, 5, 6)
    o = ref.Oracle(*shape)
    boards = np.array([o.init_board(s)[0] for s in range(1, 129)], np.int8)
    na = np.where(np.arange(128) % 3 == 0, 0, 20).astype(np.int32)
    want = ref.cached_lookahead("5x5x6", shape, boards, np.arange(1, 129), na)
    assert (want["counts"] == 0).any() and (want["counts"] > 0).any()
    got = lh.LookaheadHost(*shape).lookahead(boards, np.arange(1, 129), na, bpw=8)
    ref.assert_equal(got, want)
    dead = want["counts"] == 0
    assert (got["best_action"][dead] == -1).all() and (got["best_reward"][dead] == -1).all()
    term = (na == 0) & ~dead
    assert (got["best_reward"][term] == 0).all() and (got["last_draws"][term] == 0).all()


def test_key_orders_reward_then_lower_id():
    L = lh.lib()
    assert L.lh_key_action(0) == -1 and L.lh_key_reward(0) == -1  # "no legal action"
    rewards = [-2**31, -5, -1, 0, 1, 17, 2**31 - 2, 2**31 - 1]
    ids = [0, 1, 31, 32, 143, 479, 2**20]
    keys = [(L.lh_key(r, a), r, a) for r in rewards for a in ids]
    for k, r, a in keys:
        assert k != 0 and L.lh_key_reward(k) == r and L.lh_key_action(k) == a
    for k1, r1, a1 in keys:
        for k2, r2, a2 in keys:
            assert (k1 > k2) == ((r1, -a1) > (r2, -a2))
    # the fold is a maximum: any order of arrival gives the lowest id among the maxima
    rng = np.random.default_rng(3)
    for _ in range(50):
        n = int(rng.integers(1, 40))
        r = (rng.integers(0, 4, n).astype(np.int64) * ((2**31 - 2) // 3)).astype(np.int32)  # 0 .. 2**31 - 2
        a = rng.permutation(480)[:n].astype(np.int32)
        want_a = int(a[r == r.max()].min())
        for _ in range(3):
            p = rng.permutation(n)
            rp, ap = np.ascontiguousarray(r[p]), np.ascontiguousarray(a[p])  # (kept alive across the call)
            k = L.lh_fold(n, lh._p(rp), lh._p(ap))
            assert L.lh_key_action(k) == want_a and L.lh_key_reward(k) == int(r.max())


def test_enumeration_prefix_search_and_kth_bit():
    L = lh.lib()
    rng = np.random.default_rng(7)
    for _ in range(40):
        nb = int(rng.integers(1, 65))
        aw = int(rng.integers(1, 16))
        act = rng.integers(0, 2**32, (nb, aw), dtype=np.uint64).astype(np.uint32)
        act[rng.random(nb) < 0.2] = 0  # boards without a legal action: an empty range
        act &= rng.integers(0, 2**32, (nb, aw), dtype=np.uint64).astype(np.uint32)
        ids = [np.flatnonzero(np.unpackbits(row.view(np.uint8), bitorder="little")) for row in act]
        pre = np.concatenate([[0], np.cumsum([len(x) for x in ids])]).astype(np.uint32)
        for j in range(int(pre[-1])):
            g = L.lh_find_board(lh._p(pre), nb, j)
            assert pre[g] <= j < pre[g + 1]
            row = np.ascontiguousarray(act[g])  # (kept alive across the call)
            assert L.lh_kth_bit(lh._p(row), aw, j - int(pre[g])) == ids[g][j - pre[g]]
        row = np.ascontiguousarray(act[0])
        assert L.lh_kth_bit(lh._p(row), aw, len(ids[0])) == -1


def test_lookahead_core_under_asan_ubsan():
    """The stand-alone program beside the harness (host code only, run as a program)."""
    d = os.path.join(ROOT, "tests", "lookahead_host")
    subprocess.run(["make", "-C", d, "asan"], check=True, capture_output=True)
    r = subprocess.run([os.path.join(d, "build", "lookahead_asan")], capture_output=True, text=True)
    assert r.returncode == 0 and "checks ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


OBJS = sorted(glob.glob(os.path.join(ROOT, "element-crush-gym_amd", "build", "m3_inst_*.o")))


@pytest.mark.skipif(len(OBJS) < 10, reason="library objects not built (make -C element-crush-gym_amd)")
def test_frame16_lookahead_kernels_stay_out_of_scratch():
    """DESIGN.md §4 "Lane interference": a frame kernel that runs the cascade with several boards per
    wave must not reach scratch."""
    import spill_audit

    census = spill_audit.census(OBJS)
    checked = 0
    for name, v in census.items():
        if "frame16/" in name and name.startswith("k_lookahead<"):
            assert v.get("private_segment_fixed_size", 0) == 0, (name, v)
            checked += 1
    assert checked == 4
    for tag in ("9x9x6", "16x16x8"):
        assert any(tag in k and k.startswith("k_lookahead<") for k in census), tag
