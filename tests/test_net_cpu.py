"""The policy/value network without a GPU: the two CPU restatements against each other, the validity of
the seeded fixtures, the Python class's argument checking, and the host build of csrc/m3_net_core.hpp
(folding, bf16 rounding, the weight pre-pack, the index maps) against numpy bit for bit and as a
stand-alone ASan + UBSan program."""
import os
import subprocess
import sys

import numpy as np
import pytest

import net_ref
from net_ref import CASES, case_id

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "net_host"))
import net_host  # noqa: E402
from net_host import p  # noqa: E402

from match3tile.boardConfig import BoardConfig  # noqa: E402

N_CPU = 12  # boards per case here (the GPU tests use 130)
_cache = {}


def reference(case):
    """(weights, boards, f64, model) of a case, computed once."""
    if case not in _cache:
        w = net_ref.make_weights(case)
        b = net_ref.make_boards(case, 3 if case[4] == 256 else N_CPU)
        _cache[case] = (w, b, net_ref.forward_f64(case, w, b), net_ref.forward_model(case, w, b))
    return _cache[case]


@pytest.fixture(scope="module")
def torch_outputs(tmp_path_factory):
    """The torch float64 forward of every case, from ONE child process (this module does not import torch)."""
    path = str(tmp_path_factory.mktemp("net") / "torch.npz")
    here = os.path.dirname(os.path.abspath(__file__))
    subprocess.run([sys.executable, os.path.join(here, "net_torch_ref.py"), path, str(N_CPU)], check=True, cwd=here)
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_numpy_f64_equals_torch_f64(case, torch_outputs):
    _, _, f64, _ = reference(case)
    i = CASES.index(case)
    for key in ("values", "logits"):
        e = net_ref.err(f64[key], torch_outputs[f"{i}.{key}"])
        print(case_id(case), key, "numpy vs torch:", e)
        assert e <= 1e-9, (key, e)
    for k, a in enumerate(f64["trunk"]):
        assert net_ref.err(a, torch_outputs[f"{i}.trunk{k}"]) <= 1e-9, ("trunk", k)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_fixtures_are_valid(case):
    """Conditions, not measurements: the heads are alive and the model is close to the true network."""
    _, _, f64, model = reference(case)
    assert (f64["values"] > 0).all()
    alive = (f64["policy_1x1"] != 0).any(axis=-1)  # per position
    assert alive.mean() > 0.5
    for key in ("values", "logits"):
        e = net_ref.err(model[key], f64[key])
        print(case_id(case), key, "e(model):", e)
        assert e <= 0.05, (key, e)


def test_boards_hold_the_edge_values():
    b = net_ref.make_boards(CASES[0], 130)
    assert (b == -1).any() and (b == 127).any() and (b == 32).any() and ((b > 6) & (b < 32)).any()
    assert abs(((b > 6) | (b < 0)).mean() - 0.05) < 0.02


def test_class_argument_checking():
    from match3tile.net import ElementCrushNet, weight_spec

    case = CASES[0]
    cfg = BoardConfig(rows=9, columns=9, types=6)
    w = net_ref.make_weights(case)
    assert [(k, s) for k, s in weight_spec(cfg, 2, 32)] == [(k, s) for k, s in net_ref.weight_keys(*case)]
    missing = dict(w)
    del missing["residual_block.residual_layers.1.bn2.var"]
    with pytest.raises(ValueError, match=r"residual_block\.residual_layers\.1\.bn2\.var"):
        ElementCrushNet(cfg, 2, 32, missing)
    extra = dict(w, **{"value_head.dense3.kernel": np.zeros(3, np.float32)})
    with pytest.raises(ValueError, match=r"value_head\.dense3\.kernel"):
        ElementCrushNet(cfg, 2, 32, extra)
    shape = dict(w, **{"policy_head.dense.kernel": np.zeros((162, 143), np.float32)})
    with pytest.raises(ValueError, match=r"policy_head\.dense\.kernel"):
        ElementCrushNet(cfg, 2, 32, shape)
    for F in (48, 0, 544):
        with pytest.raises(ValueError, match="multiple of 32"):
            ElementCrushNet(cfg, 2, F, w)


# ---- the host build of m3_net_core.hpp against numpy, bit for bit ---------------------------------------------
def edge_floats():
    rng = np.random.default_rng(3)
    bits = rng.integers(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32)
    edges = np.array([0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x7F7FFFFF, 0x7F800000, 0xFF800000, 0x00000001,
                      0x80000000, 0x00008000, 0x7F7F8000], np.uint32)
    x = np.concatenate([bits, edges]).view(np.float32)
    return x[~np.isnan(x)]


def test_core_bf16_rounding_bits():
    L = net_host.lib()
    x = edge_floats()
    out = np.zeros(len(x), np.uint16)
    L.nt_bf16_round(p(x), len(x), p(out))
    want = (net_ref.bf16_round_f32(x).view(np.uint32) >> 16).astype(np.uint16)
    assert (out == want).all()
    back = np.zeros(len(x), np.float32)
    L.nt_bf16_widen(p(out), len(out), p(back))
    assert (back.view(np.uint32) == net_ref.bf16_round_f32(x).view(np.uint32)).all()
    # one rounding from float64: doubles a hair off a float32 that sits on a bf16 tie
    with np.errstate(over="ignore", invalid="ignore"):
        f = x[np.isfinite(x)][:50000].astype(np.float64)
        tie = ((x[np.isfinite(x)][:20000].view(np.uint32) & 0xFFFF0000) | 0x8000).view(np.float32).astype(np.float64)
        tie = tie[np.isfinite(tie)]
        d = np.concatenate([f * (1 + 1e-9), tie, np.nextafter(tie, np.inf), np.nextafter(tie, -np.inf)])
    out = np.zeros(len(d), np.uint16)
    L.nt_bf16_round_f64(p(d), len(d), p(out))
    want = (net_ref.bf16_round_f64(d).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    assert (out == want).all()
    # and against exact arithmetic on the ties' neighbours: above a tie rounds up, below rounds down
    t = np.float64(np.array([0x3F808000], np.uint32).view(np.float32)[0])
    d = np.array([np.nextafter(t, 2.0), np.nextafter(t, 0.0), t], np.float64)
    out = np.zeros(3, np.uint16)
    L.nt_bf16_round_f64(p(d), 3, p(out))
    assert out.tolist() == [0x3F81, 0x3F80, 0x3F80]


@pytest.mark.parametrize("F", [32, 96])
def test_core_folding_bits(F):
    L = net_host.lib()
    rng = np.random.default_rng(F)
    rows = 9 * F
    w = {"c.conv.kernel": rng.normal(0, 0.1, (3, 3, F, F)).astype(np.float32),
         "c.conv.bias": rng.normal(0, 0.2, F).astype(np.float32),
         "c.bn.scale": rng.uniform(0.5, 1.5, F).astype(np.float32), "c.bn.bias": rng.normal(0, 0.2, F).astype(np.float32),
         "c.bn.mean": rng.normal(0, 0.2, F).astype(np.float32), "c.bn.var": rng.uniform(0.5, 1.5, F).astype(np.float32)}
    wk, bk = net_ref._fold(w, "c", "conv", "bn", 1e-5)
    wf, wh, bo = np.zeros((rows, F), np.float32), np.zeros((rows, F), np.uint16), np.zeros(F, np.float32)
    L.nt_fold(p(w["c.conv.kernel"]), p(w["c.conv.bias"]), p(w["c.bn.scale"]), p(w["c.bn.bias"]), p(w["c.bn.mean"]),
              p(w["c.bn.var"]), 1e-5, rows, F, p(wf), p(wh), p(bo))
    assert (wf.view(np.uint32) == wk.reshape(rows, F).astype(np.float32).view(np.uint32)).all()
    assert (bo.view(np.uint32) == bk.astype(np.float32).view(np.uint32)).all()
    want = (net_ref.bf16_round_f64(wk.reshape(rows, F)).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    assert (wh == want).all()


@pytest.mark.parametrize("F", [32, 96, 256])
def test_core_pack_round_trip(F):
    """pack then unpack gives the weights back; the packed image is the B operand's fragment order: lane l
    of k step s of N tile t holds B[16 s + 8 (l >> 5) + j][32 t + (l & 31)], j = 0..7, in 16 consecutive bytes."""
    L = net_host.lib()
    K = 9 * F
    w = np.random.default_rng(F).integers(0, 2 ** 16, (K, F), dtype=np.uint16)
    packed, back = np.zeros(K * F, np.uint16), np.zeros((K, F), np.uint16)
    assert L.nt_pack_elems(F) == K * F
    L.nt_pack(F, p(w), p(packed))
    L.nt_unpack(F, p(packed), p(back))
    assert (back == w).all()
    want = w.reshape(K // 16, 2, 8, F // 32, 32).transpose(3, 0, 1, 4, 2)  # [t][s][h][r][j]
    assert (packed == want.reshape(-1)).all()
    assert L.nt_pack_index(F, 16 * 5 + 8 + 3, 32 + 7) == (((1 * (K // 16) + 5) * 64) + 32 + 7) * 8 + 3


def test_core_index_maps():
    L = net_host.lib()
    R, C = 7, 5
    P, n = R * C, 3
    M = n * P
    for m in range(M + 40):
        b, pos = divmod(m, P)
        r, c = divmod(pos, C)
        for tap in range(9):
            rr, cc = r + tap // 3 - 1, c + tap % 3 - 1
            want = b * P + rr * C + cc if m < M and 0 <= rr < R and 0 <= cc < C else -1
            assert L.nt_tap_row(m, M, R, C, tap) == want
    # the accumulator map of v_mfma_f32_32x32x16: every (row, column) of the tile exactly once
    seen = {(L.nt_acc_row(lane, reg), lane & 31) for lane in range(64) for reg in range(16)}
    assert seen == {(r, c) for r in range(32) for c in range(32)}
    assert [L.nt_acc_row(0, g) for g in range(16)] == [0, 1, 2, 3, 8, 9, 10, 11, 16, 17, 18, 19, 24, 25, 26, 27]
    assert L.nt_acc_row(32, 0) == 4
    for case in CASES:
        r, c, t, layers, F = case
        total = sum(int(np.prod(s)) for _, s in net_ref.weight_keys(*case))
        assert L.nt_blob_len(r * c, net_ref.action_space(r, c), net_ref.onehot_width(t), layers, F) == total
    assert [L.nt_features_ok(F) for F in (32, 96, 512, 0, 16, 48, 544)] == [1, 1, 1, 0, 0, 0, 0]


@pytest.mark.parametrize("case", [CASES[3], CASES[6]], ids=case_id)
def test_core_stem_bits(case):
    """The core's stem (the text the kernel compiles) equals the numpy model's bit for bit."""
    L = net_host.lib()
    r, c, t, _, F = case
    w = net_ref.make_weights(case)
    b = net_ref.make_boards(case, 6)
    sw, sb = net_ref._fold(w, "conv", "conv", "bn", 1e-5)
    sw, sb = np.ascontiguousarray(sw, dtype=np.float32), sb.astype(np.float32)
    out = np.zeros((6, r, c, F), np.uint16)
    L.nt_stem(p(b), 6, r, c, net_ref.onehot_width(t), F, p(sw), p(sb), p(out))
    want = (net_ref.stem_model(case, w, b).view(np.uint32) >> 16).astype(np.uint16)
    assert (out == want).all()


def test_net_core_under_asan_ubsan():
    d = os.path.dirname(os.path.abspath(net_host.__file__))
    subprocess.run(["make", "-C", d, "asan"], check=True, capture_output=True)
    r = subprocess.run([os.path.join(d, "build", "net_asan")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checks ok" in r.stdout


def test_net_translation_unit_in_the_makefile_with_the_safety_flags():
    mk = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "element-crush-gym_amd",
                           "Makefile")).read()
    assert "$(OUT)/m3_net.o" in mk.split("OBJS :=")[1].split("all:")[0]
    assert "$(HIPCC) $(HIPFLAGS) $(SAFETY) -c -o $@ csrc/m3_net.hip" in mk
