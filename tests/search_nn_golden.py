"""tests/golden/search_nn.npz (written by tests/golden/gen_golden_search_nn.py from the reference's own
NNNode / BaseMCTS code) as cases the CPU and the GPU tests share. Reads the file and
tests/nn_evaluators.py only: no oracle, no Python model of the search."""
import zlib

import numpy as np

import nn_evaluators as nev

CASES = ("A", "C", "D", "E", "Fc", "Fn", "M", "W")
_cases = {}


def load_case(data, name):
    """dict(shape, sims, calls, wseed, evname, W (None without weights), ev(board, game, round),
    roots=[dict(board [R, C], seed, n_actions, reward)], want=[game][call] -> dict(children=[(action,
    visits, sum bits, prior bits)], root_visits, flags=0, action, value, policies)). `data`: the loaded
    npz. Cached by name; nothing in it is to be changed."""
    if name in _cases:
        return _cases[name]
    d = {k[len(name) + 1:]: data[k] for k in data.files if k.startswith(name + "_") and
         not (name == "A" and k.startswith("A_numpy_"))}
    shape = tuple(int(x) for x in d["shape"])
    wseed, evname = int(d["wseed"]), str(d["evname"])
    W = nev.weights(shape, wseed) if evname == "linear" else None
    if W is not None:
        ev = lambda board, game, rnd: nev.linear_eval(W, board)  # noqa: E731
    else:
        ev = nev.constant_ev if evname == "constant" else nev.negative_ev
    n, calls = d["action"].shape
    roots = [dict(board=d["board"][g].astype(np.int32), seed=int(d["seed"][g]), n_actions=int(d["n_actions"][g]),
                  reward=int(d["reward"][g])) for g in range(n)]
    want = []
    for g in range(n):
        per_call = []
        for c in range(calls):
            k = int(d["n_children"][g, c])
            kids = [(int(d["child_action"][g, c, j]), int(d["child_visits"][g, c, j]), int(d["child_sum"][g, c, j]),
                     int(d["child_prior"][g, c, j])) for j in range(k)]
            per_call.append(dict(children=kids, root_visits=int(d["root_visits"][g, c]), flags=0,
                                 action=int(d["action"][g, c]), value=int(d["value"][g, c]),
                                 policies=[float(x) for x in d["policies"][g, c, :k]]))
        want.append(per_call)
    _cases[name] = dict(name=name, shape=shape, sims=int(d["sims"]), calls=int(calls), c=int(d["c"]), wseed=wseed,
                        evname=evname, W=W, ev=ev, roots=roots, want=want)
    return _cases[name]


def assert_game(res, g, want, tag=""):
    """res: the arrays of m3_search_nn_result (or the host core's); want: one call of one game of the
    file. Every field; floats as bit patterns."""
    k = len(want["children"])
    assert int(res["flags"][g]) == 0, (tag, g, hex(int(res["flags"][g])))
    assert int(res["root_visits"][g]) == want["root_visits"], (tag, g)
    assert int(res["n_children"][g]) == k, (tag, g)
    cs, cp = res["child_value_sum"].view(np.uint32), res["child_prior"].view(np.uint32)
    got = [(int(res["child_action"][g][j]), int(res["child_visits"][g][j]), int(cs[g][j]), int(cp[g][j])) for j in range(k)]
    assert got == want["children"], (tag, g, got, want["children"])
    assert int(res["best_action"][g]) == want["action"], (tag, g)
    assert int(res["value"][g]) == want["value"], (tag, g)
    rv = int(res["root_visits"][g])
    assert [int(res["child_visits"][g][j]) / rv for j in range(k)] == want["policies"], (tag, g)


def batch_evaluator(ev, n, A):
    """``ev`` as a host evaluator (boards, need) -> (values, logits), counting the rounds itself. Rows
    without need are filled with NaN: the library must not read them."""
    state = dict(round=0, calls=0)

    def run(boards, need):
        values, logits = np.full(n, np.nan, np.float32), np.full((n, A), np.nan, np.float32)
        for g in range(n):
            if need[g]:
                values[g], logits[g] = ev(boards[g], g, state["round"])
        state["round"] += 1
        state["calls"] += 1
        return values, logits
    run.state = state
    return run


def evaluator_triples(data):
    """[(shape, wseed, board, value bits, crc32 of the logits' bytes)] as recorded in the file."""
    out = []
    for k in data.files:
        if k.startswith("ev_") and k.endswith("_board"):
            tag = k[:-len("_board")]
            dims, wseed = tag.split("_")[1:]
            shape = tuple(int(x) for x in dims.split("x"))
            out.append((shape, int(wseed), data[k], int(data[tag + "_value_bits"]), int(data[tag + "_logits_crc"])))
    return out


def logits_crc(logits):
    return zlib.crc32(np.ascontiguousarray(logits, np.float32).tobytes())


def feed_device_rounds(ds, ev, d_values, d_logits, rounds, construction):
    """Drive a ``DeviceSearchNN(evaluator=False)`` by hand: the two construction batches (if asked), then
    `rounds` simulation rounds, every answer handed over in the device arrays d_values / d_logits."""
    for k in range(-2 if construction else 0, rounds):
        boards, need = ds.batch(max(1, rounds - max(0, k)))
        values, logits = ev(boards, need)
        d_values.upload(values)  # (blocks on the context stream: the round before has read the arrays)
        d_logits.upload(logits)
        ds.feed_device(d_values, d_logits)
