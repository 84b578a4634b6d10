"""Boards crafted to fill the match-group table (numpy and the oracle only; shape-generic).

The kernels keep the first LCAP match groups of a scan in LDS (KS::GCAP, m3_batch_core.hpp: 6 at
9x9x6, 4 at 16x16x8 and in the frames), further groups in a record of a global spill pool, and hand a
board over to an exact recompute when the pool is full or the register MT19937 chain runs out.
Seeded play gets there about once in a thousand steps and the fixtures never do, so these boards
are painted: a reset board (no matches) with k straight runs and one plus on it, and as action a
swap of two equal neighbouring cells, which leaves the board as painted -- the step's first scan
(boardv2.py:133-136) then sees every painted group at once.

The table is only used when the scan is (m3_rules.hpp, get_matches): a cell lying in both a
horizontal and a vertical run sends the whole board through match_scan, and the plus has one. Its
vertical run comes first in scan order and its horizontal arm starts left of it, so the arm is
merged into the vertical run's group (add_to_matches, boardFunctions.py:126-131) -- a
read-modify-write of that group's table entry. Two layouts:

  FIRST  the plus tops row 0 and is group 0: the merge goes to the LDS part of the table;
  LAST   the plus fills the bottom three rows and every other run lies above them, so its group
         index is the number of groups above: from LCAP on, the merge rewrites a spill record.

A few boards also carry a T or an L whose second arm the reference drops (its start is already in
the first arm, boardFunctions.py:136): one group, two cells less in the mask.

Every painted shape gets a colour that differs from all its outside neighbours, so it neither grows
nor touches another run; still, every number a test relies on (group counts, draws) is taken from
the oracle, never from what was meant to be painted.
"""
from __future__ import annotations

import numpy as np

from oracle import Oracle

PLAIN, FIRST, LAST = 0, 1, 2


SPECIALISED = {(9, 9, 6), (16, 16, 8)}  # M3_SHAPES (m3_kernels.hpp); every other shape runs in a frame


def _kernel_cells(shape):
    """CF::N of the configuration a shape runs in: its own cells if specialised, else its frame's
    (FCfg: 16 x 16, or 32 x 32 with a side above 16) -- what KS<CF> sizes itself by."""
    R, C, _ = shape
    return R * C if tuple(shape) in SPECIALISED else (256 if max(R, C) <= 16 else 1024)


# The kernels' constants that the tests restate (KS<CF> and its neighbours in m3_batch_core.hpp), as
# literals: the GPU tests need no host build. test_crafted_cpu holds every one of them to the values
# compiled into the host harness (hostcore's hc_geometry).
POOL = 4096          # KS::SPILL_RECORDS per shard and step, and rollout_pool(n) for n <= 32768
FIX_LANES = 1024     # FIX_GRID x 64: the fix kernels' lanes; more work takes their grid-stride loop
NSLOT = 4            # episode slots per board: a freed slot takes the episode NSLOT - 1 ahead
RESET_KCAP_9 = 454   # k_init<CF, false> gives up a prefetched 9x9x6 reset past this many draws


def _wide(shape):
    """the 32 x 32 frame: one board per wave, and a spill record of 86 KB"""
    return tuple(shape) not in SPECIALISED and max(shape[0], shape[1]) > 16


def pool(shape):
    """KS<CF>::SPILL_RECORDS: spill-pool records per shard and step"""
    return 256 if _wide(shape) else POOL


def fix_lanes(shape):
    """FIX_GRID x lanes_for<CF>(): boards one turn of a fix kernel's grid-stride loop takes"""
    return 16 if _wide(shape) else FIX_LANES


def rollout_pool(n):
    """rollout_spill_cap below its 256 MB budget (every shape outside the 32 x 32 frame, where the
    budget is the smaller): records of the spill pool of a launch of n rollouts"""
    return max(POOL, n // 8)


def lcap(shape):
    """KS<CF>::GCAP (m3_batch_core.hpp): match groups per lane in LDS -- 6 for 9x9x6, 4 for 16x16x8
    and for every frame shape (held to the compiled value by test_crafted_cpu)."""
    return 6 if _kernel_cells(shape) <= 128 else 4


def chain_limit(shape):
    """Raw draws since the last reseed that the step kernels' register chain can serve
    (KS::Chain: ChainMTT<624> for 9x9x6, ChainMTT<227> for 16x16x8 and the frames; m3_rng.hpp
    next32 / slow: with k outputs behind it the chain serves one more iff k < LIMIT, else it
    raises `overflow`)."""
    return 624 if _kernel_cells(shape) <= 128 else 227


def decode_table(o: Oracle):
    """[A, 4] (source row, column, target row, column) of every action id."""
    return np.array([sum(o.decode(a), ()) for a in range(o.A)], np.int32)


def first_scan_groups(o: Oracle, board, action=None, dec=None):
    """Groups of the step's first get_matches: the board after the swap, type bits only."""
    b = np.array(board, np.int32)
    if action is not None:
        sr, sc, tr, tc = (dec if dec is not None else decode_table(o))[action]
        b[sr, sc], b[tr, tc] = b[tr, tc], b[sr, sc]
    return o.get_matches(b & o.cfg.TM)[2]


def first_scan_takes_table(o: Oracle, board, action=None, dec=None):
    """Whether the step's first get_matches goes through the sequential scan and its group table at
    all (m3_rules.hpp, get_matches): only with a cell in both a horizontal and a vertical run of three
    or more, or with a run of six or more. Without either every maximal run is its own group and no
    table is filled, however many groups there are -- a swap that takes a cell out of the painted
    plus leaves such a board."""
    b = np.array(board, np.int32)
    if action is not None:
        sr, sc, tr, tc = (dec if dec is not None else decode_table(o))[action]
        b[sr, sc], b[tr, tc] = b[tr, tc], b[sr, sc]
    b &= o.cfg.TM
    R, C = b.shape
    h3 = (b[:, :-2] != 0) & (b[:, :-2] == b[:, 1:-1]) & (b[:, 1:-1] == b[:, 2:])  # a horizontal triple starts here
    v3 = (b[:-2] != 0) & (b[:-2] == b[1:-1]) & (b[1:-1] == b[2:])
    hc, vc = np.zeros((R, C), bool), np.zeros((R, C), bool)
    for k in range(3):
        hc[:, k:C - 2 + k] |= h3
        vc[k:R - 2 + k] |= v3
    six = ((h3[:, :-3] & h3[:, 1:-2] & h3[:, 2:-1] & h3[:, 3:]).any() if C >= 6 else False) or \
          ((v3[:-3] & v3[1:-2] & v3[2:-1] & v3[3:]).any() if R >= 6 else False)
    return bool((hc & vc).any() or six)


def _paint(board, used, cells, rng, T):
    """Paint `cells` in one colour that no outside neighbour has; False if they are taken or no
    colour is left."""
    R, C = board.shape
    if any(not (0 <= r < R and 0 <= c < C) or used[r, c] for r, c in cells):
        return False
    inside = set(cells)
    ban = set()
    for r, c in cells:
        for rr, cc in ((r + 1, c), (r - 1, c), (r, c + 1), (r, c - 1)):
            if 0 <= rr < R and 0 <= cc < C and (rr, cc) not in inside:
                ban.add(int(board[rr, cc]))
    free = [t for t in range(1, T + 1) if t not in ban]
    if not free:
        return False
    col = free[int(rng.integers(len(free)))]
    for r, c in cells:
        board[r, c] = col
        used[r, c] = True
    return True


def _shape(kind, r, c):
    if kind == "h3":
        return [(r, c), (r, c + 1), (r, c + 2)]
    if kind == "h4":
        return [(r, c), (r, c + 1), (r, c + 2), (r, c + 3)]
    if kind == "v3":
        return [(r, c), (r + 1, c), (r + 2, c)]
    if kind == "plus":  # vertical run through column c, horizontal run through its middle row
        return [(r, c), (r + 1, c), (r + 2, c), (r + 1, c - 1), (r + 1, c + 1)]
    if kind == "T":     # h-run first, the v-run hangs from its middle cell: dropped
        return [(r, c), (r, c + 1), (r, c + 2), (r + 1, c + 1), (r + 2, c + 1)]
    if kind == "L":     # ... from its last cell: dropped too
        return [(r, c), (r, c + 1), (r, c + 2), (r + 1, c + 2), (r + 2, c + 2)]
    raise ValueError(kind)


def craft(o: Oracle, rng, layout, k, dec=None):
    """One painted board of `layout` (FIRST / LAST) with up to k runs besides the plus.
    Returns (board int8 [R, C], action, meta) with meta = dict(layout, groups, above, heavy): groups
    of the first scan, for LAST the groups of the rows above the plus (-1 for FIRST), and whether
    the runs carry line specials (three rows in ten: H / V bits on a random share of the run
    cells, so the matched runs clear whole rows and columns -- draw counts up to a full-board
    refill and beyond, the other way into a recompute on boards of more than 128 cells)."""
    R, C, T = o.R, o.C, o.T
    dec = decode_table(o) if dec is None else dec
    while True:
        board = o.init_board(int(rng.integers(1, 2**32)))[0].copy()
        used = np.zeros((R, C), bool)
        pc = int(rng.integers(1, C - 1))
        top = 0 if layout == FIRST else R - 3
        if not _paint(board, used, _shape("plus", top, pc), rng, T):
            continue
        if layout == FIRST:
            used[0, :pc] = True          # nothing starts before the plus
            lo, hi = 0, R
        else:
            used[R - 3:, :] = True       # everything else lies above it
            lo, hi = 0, R - 3
        quirk = rng.random() < 0.15
        done = 0
        runs = []
        for _ in range(60 * (k + 1)):
            if done >= k:
                break
            u = rng.random()
            kind = ("T" if u < 0.5 else "L") if quirk else ("h3" if u < 0.45 else "v3" if u < 0.85 else "h4")
            r, c = int(rng.integers(lo, hi)), int(rng.integers(0, C))
            cells = _shape(kind, r, c)
            if max(rr for rr, _ in cells) >= hi:
                continue
            if _paint(board, used, cells, rng, T):
                done += 1
                quirk = False
                runs += cells
        heavy = rng.random() < 0.3
        if heavy:  # line specials in the runs: each clears its row / column when its run is matched
            dens = rng.random()
            for r, c in runs:
                if rng.random() < dens:
                    board[r, c] |= o.cfg.H if rng.random() < 0.5 else o.cfg.V
        eq = np.flatnonzero(board[dec[:, 0], dec[:, 1]] == board[dec[:, 2], dec[:, 3]])
        action = int(eq[int(rng.integers(len(eq)))])  # (the plus alone gives four such swaps)
        above = -1
        if layout == LAST:
            upper = board.astype(np.int32) & o.cfg.TM
            upper[R - 3:] = 0
            above = o.get_matches(upper)[2]
        meta = dict(layout=layout, groups=first_scan_groups(o, board, action, dec), above=above, heavy=heavy)
        return board.astype(np.int8), action, meta


def plain(o: Oracle, rng, dec=None):
    """An ordinary row: a reset board that plays one of its own legal actions."""
    board = o.init_board(int(rng.integers(1, 2**32)))[0]
    legal = o.legal_actions(board)
    action = legal[int(rng.integers(len(legal)))]
    meta = dict(layout=PLAIN, groups=first_scan_groups(o, board, action, dec), above=-1, heavy=False)
    return board.astype(np.int8), action, meta


_cache = {}


def rows(shape, n=400, seed=2024):
    """n rows for `shape`, about a quarter of them plain, the rest split between the two layouts:
    dict(boards [n, R, C] int8, seeds uint32, actions int32, layout, groups, above, heavy). Cached and
    read-only: every test of a shape shares them."""
    key = (tuple(shape), n, seed)
    if key in _cache:
        return _cache[key]
    o = Oracle(*shape)
    rng = np.random.default_rng(seed)
    dec = decode_table(o)
    L = lcap(shape)
    out = []
    for _ in range(n):
        u = rng.random()
        if u < 0.25:
            out.append(plain(o, rng, dec))
        elif u < 0.6:
            out.append(craft(o, rng, FIRST, int(rng.integers(L - 2, L + 9)), dec))
        else:
            out.append(craft(o, rng, LAST, int(rng.integers(L - 1, L + 8)), dec))
    res = dict(boards=np.array([b for b, _, _ in out], np.int8),
               seeds=rng.integers(1, 2**32, size=n, dtype=np.uint64).astype(np.uint32),
               actions=np.array([a for _, a, _ in out], np.int32),
               layout=np.array([m["layout"] for _, _, m in out], np.int8),
               groups=np.array([m["groups"] for _, _, m in out], np.int32),
               above=np.array([m["above"] for _, _, m in out], np.int32),
               heavy=np.array([m["heavy"] for _, _, m in out], bool))
    for a in res.values():
        a.setflags(write=False)
    _cache[key] = res
    return res


def oracle_steps(shape, rw, n_actions=20):
    """The oracle's apply_action and the seeded random action behind it for every row:
    dict(next [n, R, C], reward, draws, flags, next_action, draws_after, legal [n, A] bool).
    Cached on the identity of rw (use it on rows(), before replicate())."""
    key = ("steps", tuple(shape), id(rw), n_actions)
    if key in _cache:
        return _cache[key]
    o = Oracle(*shape)
    n = len(rw["seeds"])
    res = dict(next=np.zeros((n, o.R, o.C), np.int32), reward=np.zeros(n, np.int64), draws=np.zeros(n, np.int64),
               flags=np.zeros(n, np.int64), next_action=np.zeros(n, np.int32), draws_after=np.zeros(n, np.int64),
               legal=np.zeros((n, o.A), bool))
    for i in range(n):
        nb, r, d, f, nx, da = o.apply_action_next(rw["boards"][i].astype(np.int32), int(rw["seeds"][i]),
                                                  int(rw["actions"][i]), n_actions)
        res["next"][i], res["reward"][i], res["draws"][i], res["flags"][i] = nb, r, d, f
        res["next_action"][i], res["draws_after"][i] = nx, da
        res["legal"][i, o.legal_actions(nb)] = True
    for a in res.values():
        a.setflags(write=False)
    _cache[key] = res
    _cache[("keep", id(rw))] = rw  # (keeps id(rw) from being reused)
    return res


def replicate(rw, times, index=None, total=None):
    """The rows `index` of rw (default: all) tiled `times` times, cut to `total` rows if given:
    the same dict plus src, each copy's row in rw. The oracle is evaluated once per unique row
    (take its results with src); the copies may take different paths on the device -- which of
    them finds the pool full depends on atomic order -- and must still agree bit for bit."""
    index = np.arange(len(rw["seeds"])) if index is None else np.asarray(index, np.int64)
    src = np.tile(index, times)[:total]
    out = {k: v[src] for k, v in rw.items()}
    out["src"] = src
    return out


def legal_words(legal_bool):
    """[n, A] bool -> [n, ceil(A / 32)] uint32, bit a of word a // 32 (the ABI's legal set)."""
    n, A = legal_bool.shape
    pad = np.zeros((n, (A + 31) // 32 * 32), np.uint8)
    pad[:, :A] = legal_bool
    return np.packbits(pad, axis=1, bitorder="little").view("<u4").astype(np.uint32)
