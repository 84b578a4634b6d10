"""tests/crafted.py on the CPU: what the GPU fallback tests (test_gpu_fallbacks.py) presuppose about
their input, from the oracle alone -- so that none of them can pass because its boards went soft --
and the host build of the device rule code (tests/hostcore) on the same rows: many-group scans,
merges into late groups and full-board refills before any of it runs on a GPU."""
import os
import sys

import numpy as np
import pytest

import crafted
from conftest import ROOT, SHAPES
from oracle import FLAG_SHUFFLED, Oracle

sys.path.insert(0, os.path.join(ROOT, "tests", "hostcore"))
from hostcore import HostCore  # noqa: E402

ALL = dict(SHAPES, **{"8x8x5": (8, 8, 5)})  # (the frame shape of the GPU tests)


def test_constants_match_the_kernel_source():
    """Every kernel constant that tests/crafted.py restates for the GPU tests -- KS::GCAP, the reach of
    KS::Chain, the pool sizes, the fix kernels' lanes, NSLOT, RESET_KCAP -- against the value compiled
    into the host harness from the kernels' own header (hc_geometry), for each kind of configuration:
    the two specialised shapes, the 16 x 16 frame and the 32 x 32 frame."""
    # (8, 8, 5) and (9, 9, 5) run in FCfg, whose N is the frame's 256 cells whatever the board's: a
    # table or chain sized by the board's own cells (9x9x5: 81, as 9x9x6) would show in these two rows
    shapes = ((9, 9, 6), (16, 16, 8), (8, 8, 5), (9, 9, 5), (20, 20, 6))
    for shape in shapes:
        hc = HostCore(*shape)
        g = hc.geometry()
        assert crafted.lcap(shape) == g["GCAP"], shape
        assert crafted.chain_limit(shape) == g["CHAIN_LIMIT"], shape
        assert crafted.pool(shape) == g["SPILL_RECORDS"], shape
        assert crafted.fix_lanes(shape) == g["FIX_LANES"], shape
        assert crafted.NSLOT == g["NSLOT"], shape
        assert crafted.RESET_KCAP_9 == g["RESET_KCAP"], shape
        assert g["BPW"] == (1 if shape == (20, 20, 6) else 64), shape
        assert g["CASCADE_LIMIT"] == (2 if shape == (9, 9, 6) else -1), shape  # (test_hostcore_cpu's pauses)
        for n in (8192, 65536):
            budget = (256 << 20) // (4 * g["SPILL_WORDS"])
            want = crafted.rollout_pool(n) if shape != (20, 20, 6) else min(crafted.rollout_pool(n), budget)
            assert hc.rollout_spill_cap(n) == want, (shape, n)
            assert shape == (20, 20, 6) or budget > want, (shape, n)  # (rollout_pool's premise)
    # what the GPU tests use outright, for the shapes they run
    for shape in ALL.values():
        assert (crafted.pool(shape), crafted.fix_lanes(shape)) == (crafted.POOL, crafted.FIX_LANES)
    assert crafted.rollout_pool(8192) == crafted.POOL
    assert [crafted.lcap(s) for s in shapes[:4]] == [6, 4, 4, 4]
    assert [crafted.chain_limit(s) for s in shapes[:3]] == [624, 227, 227]


@pytest.mark.parametrize("tag", list(ALL))
def test_crafted_rows_fill_the_table(tag):
    """Preconditions on the group counts (first scan of the step, the oracle's get_matches)."""
    shape = ALL[tag]
    rw = crafted.rows(shape)
    L = crafted.lcap(shape)
    cr = rw["layout"] != crafted.PLAIN
    assert 0.15 < (~cr).mean() < 0.35                      # about a quarter of ordinary rows
    assert (rw["groups"][~cr] <= L).all()                  # ... none of which fills the table
    assert (rw["groups"][cr] > L).mean() >= 0.60
    for g in range(L - 1, L + 7):
        assert (rw["groups"][cr] == g).any(), g
    last = rw["layout"] == crafted.LAST
    assert (rw["above"][last] >= L + 1).sum() >= 30       # the plus merges into a spill record
    assert ((rw["above"][last] >= 0) & (rw["above"][last] < L)).sum() >= 5  # ... and into LDS
    assert (rw["groups"][last] == rw["above"][last] + 1).all()  # the plus is the last group
    assert (rw["layout"] == crafted.FIRST).sum() >= 50
    # the action is a swap of two equal cells: the first scan runs on the board as painted
    o = Oracle(*shape)
    dec = crafted.decode_table(o)
    b, a = rw["boards"][cr], rw["actions"][cr]
    i = np.arange(len(a))
    assert (b[i, dec[a, 0], dec[a, 1]] == b[i, dec[a, 2], dec[a, 3]]).all()
    # every crafted row has a cell in both a horizontal and a vertical run (the scan, not the
    # loop-free path): the plus' centre
    for bd in b[:50]:
        t = bd.astype(np.int32) & o.cfg.TM
        h = np.zeros(t.shape, bool)
        v = np.zeros(t.shape, bool)
        eh = (t[:, :-2] == t[:, 1:-1]) & (t[:, 1:-1] == t[:, 2:]) & (t[:, :-2] > 0)
        ev = (t[:-2] == t[1:-1]) & (t[1:-1] == t[2:]) & (t[:-2] > 0)
        for k in range(3):
            h[:, k:k + eh.shape[1]] |= eh
            v[k:k + ev.shape[0]] |= ev
        assert (h & v).any()


@pytest.mark.parametrize("tag", list(ALL))
def test_crafted_rows_and_the_rng_chain(tag):
    """Preconditions on the draw counts. The step kernels draw from the register chain
    ChainMTT<LIMIT> (m3_rng.hpp): next32 with k raw outputs behind it serves the draw iff k < LIMIT
    (below 227 by the fast level, up to LIMIT by slow()), else it raises `overflow` -- so a step is
    within the chain's reach iff it draws at most LIMIT times between two reseeds, the pre-drawn
    next action's draws included (env_fin_begin draws it for every row that stepped, finished or
    not), and is recomputed by k_env_fix iff that count is LIMIT + 1 or more. LIMIT is 624 at
    9x9x6 and 227 at 16x16x8 and in the frames (8x8x5: its 64 cells seldom get there, so no
    count is asked of it). No crafted row shuffles (the only reseed inside a step), so the oracle's
    draws_after is that count."""
    shape = ALL[tag]
    rw = crafted.rows(shape)
    st = crafted.oracle_steps(shape, rw)
    assert not (st["flags"] & FLAG_SHUFFLED).any() and not st["flags"].any()
    assert (st["next_action"] >= 0).all()
    assert (st["draws_after"] > st["draws"]).all()
    assert (st["draws_after"] < 624).all()
    if crafted.chain_limit(shape) == 624:
        pass  # every recompute at this shape is one of the group table / spill pool
    elif tag in SHAPES:
        over = st["draws_after"] > 227
        assert over.sum() >= 10 and (~over & (st["draws_after"] > 150)).sum() >= 10
        # (below 624, above: k_env_fix' three-level chain serves them)
        assert (over & (rw["groups"] > 4)).sum() >= 5     # past the table and past the chain at once
    assert (rw["heavy"] & (st["draws_after"] > 100)).sum() >= 10


def _words(legal_bool):
    return crafted.legal_words(legal_bool)


@pytest.mark.parametrize("small", [False, True, 4, 32], ids=["full", "table1", "table4", "envstep16"])
@pytest.mark.parametrize("tag", list(ALL))
def test_hostcore_apply_on_crafted_rows(tag, small):
    """HostCore.apply (apply_action + legal set + next action of m3_rules.hpp on the host) on the
    crafted rows against the oracle: boards, reward, draws, flags, legal set and next action, with
    the full group table, with a 1- and a 4-group table and with the 16x16 env step's pair (4
    groups, one-level chain), each with the exact recompute behind it."""
    shape = ALL[tag]
    rw = crafted.rows(shape)
    st = crafted.oracle_steps(shape, rw)
    hc = HostCore(*shape)
    out, rew, drw, flg, legal, nxt = hc.apply(rw["boards"], rw["seeds"], 20, rw["actions"], small=small)
    n = len(rew)
    assert (out == st["next"].reshape(n, -1)).all()
    assert (rew == st["reward"]).all() and (drw == st["draws"]).all()
    assert ((flg & 0x1F) == st["flags"]).all()
    assert (legal == _words(st["legal"])).all()
    assert (nxt == st["next_action"]).all()
    if small is True:
        assert hc.recomputed > 0.6 * n
    elif small == 4:
        assert hc.recomputed >= int((rw["groups"] > 4).sum())


@pytest.mark.parametrize("tag", list(ALL))
def test_hostcore_rollouts_on_crafted_rows(tag):
    """rollout_one on the host from the crafted boards (the first action comes from the rollout
    seed, so most first scans keep their painted groups) against Oracle.rollouts."""
    shape = ALL[tag]
    rw = crafted.rows(shape)
    hc, o = HostCore(*shape), Oracle(*shape, episode_shuffle_cap=1024)
    n = len(rw["seeds"])
    rs = (np.arange(n, dtype=np.uint64) * 2654435761 % (2**31)).astype(np.uint32)
    for k in (1, 3, 20):
        g = hc.rollouts(rw["boards"], rw["seeds"], k, rs)
        w = o.rollouts(rw["boards"].astype(np.int32), rw["seeds"], k, rs, threads=4)
        ok = g["gain"] >= 0  # (chain overflow: replayed on the GPU by k_rollout_fix)
        assert ok.mean() > 0.8
        assert (g["gain"][ok] == w["gain"][ok]).all() and (g["steps"][ok] == w["steps"][ok]).all()
        assert (g["draws"][ok].astype(np.int64) == w["draws"][ok]).all()
        assert ((g["flags"][ok] & 0x1F) == (w["flags"][ok] & 0x1F)).all()


def test_cycling_dead_boards_stop_at_the_cap(golden):
    """tests/golden/cycling.npz: dead 9x9x6 boards that stay dead under every power of the
    reseeded row shuffle (the reference never returns from apply_action on them; the generator
    confirmed that under an alarm). The oracle and the host build stop after the same 1024
    shuffles (m3_oracle.c:505-507, m3_rules.hpp apply_cascade_ex) with FLAG_SHUFFLE_CAP |
    FLAG_SHUFFLED and the same board, reward and draws -- the branch test_shuffle_golden's `~t`
    rows would take, had shuffle.npz any. The search found no such board at 16x16x8 (recorded
    with zero rows)."""
    g = golden("cycling")
    assert len(g["seed_9x9x6"]) >= 8 and len(g["seed_16x16x8"]) == 0
    shape = SHAPES["9x9x6"]
    o, hc = Oracle(*shape, shuffle_cap=1024), HostCore(*shape)
    b, s, a = g["board_9x9x6"], g["seed_9x9x6"], g["action_9x9x6"]
    assert (g["flags_9x9x6"] == 0x14).all()
    for i in range(len(s)):
        assert not o.legal_actions(b[i]) and not o.get_matches(b[i].astype(np.int32))[2]
        nb, r, d, f = o.apply_action(b[i].astype(np.int32), int(s[i]), int(a[i]), 20)
        assert (nb == g["next_9x9x6"][i]).all() and (r, d, f) == (g["reward_9x9x6"][i], g["draws_9x9x6"][i], 0x14)
        assert not o.legal_actions(nb)
    for small in (False, True):
        out, rew, drw, flg, legal, nxt = hc.apply(b, s, 20, a, small=small)
        assert (out == g["next_9x9x6"].reshape(len(s), -1)).all()
        assert (rew == g["reward_9x9x6"]).all() and (drw == g["draws_9x9x6"]).all()
        assert ((flg & 0x17) == 0x14).all() and (nxt == -1).all() and not legal.any()


def test_first_scan_takes_table_against_the_host_build():
    """crafted.first_scan_takes_table (a restatement of get_matches' way past the table) on painted
    16x16x8 boards under every one of their own legal swaps: where the first scan goes through the table
    with more groups than it holds, the host build of the step (a 4-group table, KS::GCAP there) leaves
    for the exact pass; and some swaps do break the plus, so that the group count alone says nothing."""
    shape = (16, 16, 8)
    o, hc = Oracle(*shape), HostCore(*shape)
    assert crafted.lcap(shape) == 4
    dec = crafted.decode_table(o)
    rw = crafted.rows(shape, n=64)
    idx = np.flatnonzero(rw["layout"] != crafted.PLAIN)[:8]
    through, past = 0, 0
    for i in idx:
        assert crafted.first_scan_takes_table(o, rw["boards"][i], int(rw["actions"][i]), dec)  # the painted swap
        for a in o.legal_actions(rw["boards"][i].astype(np.int32)):
            many = crafted.first_scan_groups(o, rw["boards"][i], a, dec) > 4
            if many and crafted.first_scan_takes_table(o, rw["boards"][i], a, dec):
                hc.apply(rw["boards"][i:i + 1], rw["seeds"][i:i + 1], 3, [a], small=4)
                assert hc.recomputed == 1, (i, a)
                through += 1
            past += many and not crafted.first_scan_takes_table(o, rw["boards"][i], a, dec)
    assert through >= 50 and past >= 1
    assert not crafted.first_scan_takes_table(o, o.init_board(5)[0])  # a reset board: no match at all
