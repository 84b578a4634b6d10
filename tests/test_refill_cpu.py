"""The two-part 9x9x6 refill (m3_rules.hpp refill: generation loop + refill_place) against the
tile-by-tile refill_loop it replaced, on the CPU (tests/refill_host: a host build of the same
header). Equal planes, generator position and overflow flag; the planes only where the refill did
not overflow (an overflowed step is recomputed from scratch). Both chain depths: 624 (ChainMT, the
9x9x6 kernels' generator) and 227 (ChainMT1: the same loop with the overflow at its exit)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "refill_host"))
import refill_host as rf  # noqa: E402


def both(limit, heights, seeds, k0):
    heights = np.asarray(heights).reshape(-1, 9)
    new = rf.refill("new", limit, heights, seeds, k0)
    old = rf.refill("loop", limit, heights, seeds, k0)
    return heights, new, old


def assert_equal(limit, heights, seeds, k0):
    heights, (pn, kn, on), (po, ko, oo) = both(limit, heights, seeds, k0)
    assert (kn == ko).all(), np.flatnonzero(kn != ko)[:5]
    assert (on == oo).all(), np.flatnonzero(on != oo)[:5]
    ok = on == 0
    bad = np.flatnonzero((pn != po).any(axis=(1, 2)) & ok)
    assert bad.size == 0, (bad[:5], heights[bad[:5]])
    return heights.sum(axis=1), on


def spread(n, first=0):
    """n holes, dealt to the columns one at a time from column `first`."""
    h = [0] * 9
    c = first
    while n:
        if h[c] < 9:
            h[c] += 1
            n -= 1
        c = (c + 1) % 9
    return h


@pytest.mark.parametrize("limit", [227, 624])
def test_random_hole_sets(limit):
    rng = np.random.default_rng(limit)
    n = 100_000
    heights = rng.integers(0, 10, size=(n, 9))
    heights[::4] = np.where(heights[::4] > 3, 0, heights[::4])  # a quarter small, as most refills on the GPU
    seeds = rng.integers(1, 2**32, size=n, dtype=np.uint64).astype(np.uint32)
    k0 = rng.integers(0, 201, size=n)
    holes, ovf = assert_equal(limit, heights, seeds, k0)
    assert (holes > 32).any() and (holes <= 32).sum() > n // 4 and (holes == 0).any()
    if limit == 227:
        assert ovf.any()


@pytest.mark.parametrize("limit", [227, 624])
@pytest.mark.parametrize("holes", [0, 1, 32, 33, 81])
def test_exact_hole_counts(limit, holes):
    rows = [spread(holes, first) for first in range(9)]
    if holes == 32:
        rows += [[4, 4, 4, 4, 4, 3, 0, 0, 9], [0, 0, 0, 0, 0, 5, 9, 9, 9], [9, 9, 9, 5, 0, 0, 0, 0, 0],
                 [9, 0, 0, 7, 0, 0, 7, 0, 9]]
    if holes == 33:
        rows += [[4, 4, 4, 4, 4, 4, 0, 0, 9], [0, 0, 0, 0, 0, 6, 9, 9, 9]]
    heights = np.repeat(np.array(rows), 50, axis=0)
    seeds = np.arange(1, len(heights) + 1, dtype=np.uint32) * 7919
    got, _ = assert_equal(limit, heights, seeds, np.arange(len(heights)) % 13)
    assert (got == holes).all()


@pytest.mark.parametrize("limit", [227, 624])
def test_one_full_column(limit):
    heights = np.repeat(np.eye(9, dtype=np.int64) * 9, 40, axis=0)
    below = np.repeat(np.triu(np.ones((9, 9), np.int64)) * 9, 10, axis=0)  # the columns from c on full
    heights = np.concatenate([heights, below])
    seeds = np.arange(1, len(heights) + 1, dtype=np.uint32) * 104729
    assert_equal(limit, heights, seeds, np.arange(len(heights)) % 50)


@pytest.mark.parametrize("limit", [227, 624])
def test_refills_that_cross_draw_227(limit):
    k0 = np.repeat(np.arange(180, 228), 30)
    heights = np.array([spread(20 + i % 13, i % 9) for i in range(len(k0))])
    seeds = np.arange(1, len(k0) + 1, dtype=np.uint32) * 31
    _, (pn, kn, on), _ = both(limit, heights, seeds, k0)
    assert_equal(limit, heights, seeds, k0)
    if limit == 227:
        assert on.any() and not on.all()
    else:
        assert not on.any() and (kn > 227).any() and (kn <= 227).any()


def test_refills_that_reach_the_624_draw_limit():
    k0 = np.repeat(np.arange(560, 625), 20)
    heights = np.array([spread(8 + i % 25, i % 9) for i in range(len(k0))])
    seeds = np.arange(1, len(k0) + 1, dtype=np.uint32) * 2053
    _, (pn, kn, on), _ = both(624, heights, seeds, k0)
    assert_equal(624, heights, seeds, k0)
    assert on.any() and not on.all()
    # and across the second level change (draw 454)
    k0 = np.repeat(np.arange(420, 455), 20)
    heights = np.array([spread(16 + i % 17, i % 9) for i in range(len(k0))])
    _, ovf = assert_equal(624, heights, seeds[:len(k0)], k0)
    assert not ovf.any()


def test_fallback_share_of_seeded_episodes():
    """The share of refills that go to refill_loop (more than 32 tiles), over the episodes of
    tests/test_gpu_refill.py: seeds 1..4096, 20 seeded moves. A wave of the step kernel (64
    consecutive boards, one move, the j-th refill of the cascade) falls back when any of its lanes
    does. DESIGN.md §4 quotes the figures this prints."""
    need, redone = rf.episode_refills(np.arange(1, 4097), 20)
    assert need[:, :, -1].max() == 0, "more refills in a step than the table holds"
    lanes = need[need > 0]
    lane_share = (lanes > 32).mean()
    waves = need.reshape(64, 64, 20, -1).max(axis=1)  # (wave, move, refill): the largest lane
    wave_share = (waves[waves > 0] > 32).mean()
    print(f"refills {lanes.size}, mean tiles {lanes.mean():.2f}, over 32 tiles: {lane_share:.5f} of the refills, "
          f"{wave_share:.4f} of the wave-level refills; steps redone with the full generator: {redone}")
    assert lanes.size > 4096 * 20 and redone < 4096  # every step refills at least once


def test_crafted_fixture_has_the_refill_sizes_it_names():
    """tests/golden/refill.npz (the device test's crafted boards): the first refill of every row has
    the size the fixture records, and both sides of the 32-tile stream are there."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "refill.npz"))
    need = rf.step_refills(g["boards"], g["seeds"], g["actions"], cap=1)[:, 0]
    assert (need == g["need"]).all()
    count = {k: int((need == k).sum()) for k in (32, 33, 81)}
    assert min(count.values()) >= 30 and len(need) >= 300, count


def test_refill_under_asan_ubsan():
    """The stand-alone program beside the harness (host code only, run as a program)."""
    d = os.path.join(ROOT, "tests", "refill_host")
    subprocess.run(["make", "-C", d, "asan"], check=True, capture_output=True)
    r = subprocess.run([os.path.join(d, "build", "refill_asan")], capture_output=True, text=True)
    assert r.returncode == 0 and "checks ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
