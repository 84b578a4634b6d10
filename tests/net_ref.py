"""TEST INFRASTRUCTURE ONLY: CPU restatements of the policy/value network (include/m3.h "the policy/value
network") in numpy, the seeded weights and boards the network tests share, and the
error measure.

- ``forward_f64``: the network in plain float64, no rounding anywhere (BN folded in float64).
- ``forward_model``: the written arithmetic model of the device: BN folded in float64; the stem a
  float32 gather in ascending tap order; the tower's folded weights rounded once to bf16 and its
  activations stored as bf16, accumulated here in float64 (the device accumulates in float32 on the
  matrix cores); float32 head weights over the bf16 trunk output.

tests/net_torch_ref.py holds an independent float64 forward in torch (unfolded BN, NCHW conv2d)."""
import numpy as np

# (rows, columns, types, layers, features) of the GPU cases
CASES = [(9, 9, 6, 2, 32), (9, 9, 6, 2, 96), (16, 16, 8, 1, 32), (7, 5, 4, 1, 32), (6, 6, 2, 0, 32),
         (20, 20, 6, 1, 32), (9, 9, 20, 1, 32), (9, 9, 6, 1, 256)]
BN_EPS = 1e-5


def case_id(case):
    r, c, t, L, F = case
    return f"{r}x{c}x{t}-L{L}-F{F}"


def onehot_width(types):
    return 2 ** ((int(types) - 1).bit_length() + 2)


def action_space(rows, columns):
    return 2 * rows * (columns - 1)


# ---- bf16 ------------------------------------------------------------------------------------------------
def bf16_round_f32(x):
    """float32 -> the nearest bf16 (ties to even), returned as float32."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    r = np.where(nan, ((u >> 16) | 0x40) << 16, r)
    return r.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def bf16_round_f64(x):
    """float64 -> the nearest bf16 in ONE rounding (ties to even), returned as float64. Through float32
    the value would be rounded twice; where that float32 sits exactly on a bf16 tie the double was not
    on, the side the double lay on decides."""
    x = np.asarray(x, dtype=np.float64)
    f = x.astype(np.float32)
    u = f.view(np.uint32)
    tie = ((u & 0xFFFF) == 0x8000) & np.isfinite(f) & (f.astype(np.float64) != x)
    up = np.abs(x) > np.abs(f.astype(np.float64))
    hi = (u >> 16).astype(np.uint32) + (tie & up).astype(np.uint32)
    fixed = (hi << 16).astype(np.uint32).view(np.float32)
    return np.where(tie, fixed, bf16_round_f32(f)).astype(np.float64)


# ---- weights and boards -----------------------------------------------------------------------------------
def weight_keys(rows, columns, types, layers, features):
    """(key, shape, fan_in or None) in the order of m3_net_create's blob."""
    P, A, F, CH = rows * columns, action_space(rows, columns), features, onehot_width(types)
    bn = ("scale", "bias", "mean", "var")

    def conv(prefix, cname, bname, kh, cin, cout):
        return [(f"{prefix}.{cname}.kernel", (kh, kh, cin, cout)), (f"{prefix}.{cname}.bias", (cout,))] + \
               [(f"{prefix}.{bname}.{k}", (cout,)) for k in bn]

    spec = conv("conv", "conv", "bn", 3, CH, F)
    for i in range(layers):
        base = f"residual_block.residual_layers.{i}"
        spec += conv(base, "conv1", "bn1", 3, F, F) + conv(base, "conv2", "bn2", 3, F, F)
    spec += conv("value_head", "conv", "bn", 1, F, 1)
    spec += [("value_head.dense1.kernel", (P, F)), ("value_head.dense1.bias", (F,)),
             ("value_head.dense2.kernel", (F, 1)), ("value_head.dense2.bias", (1,))]
    spec += conv("policy_head", "conv", "bn", 1, F, 2)
    spec += [("policy_head.dense.kernel", (2 * P, A)), ("policy_head.dense.bias", (A,))]
    return spec


def make_weights(case, seed=0):
    """Seeded float32 weights: kernels N(0, 1 / fan_in), BN scale and var U(0.5, 1.5), every bias and
    mean N(0, 0.2^2). A random tower has dead heads -- the value head's last ReLU returns 0 for every
    board and the policy head's 1x1 ReLU can be all zero, so a test would see only biases -- hence the
    heads' BN bias is |N(0, 0.2^2)| + 0.5 and dense2's bias |.| + 1."""
    rng = np.random.default_rng(seed)
    w = {}
    for key, shape in weight_keys(*case):
        leaf = key.rsplit(".", 1)[1]
        if leaf == "kernel":
            fan_in = int(np.prod(shape[:-1]))
            a = rng.normal(0.0, np.sqrt(1.0 / fan_in), shape)
        elif leaf in ("scale", "var"):
            a = rng.uniform(0.5, 1.5, shape)
        else:
            a = rng.normal(0.0, 0.2, shape)
        if key in ("value_head.bn.bias", "policy_head.bn.bias"):
            a = np.abs(a) + 0.5
        if key == "value_head.dense2.bias":
            a = np.abs(a) + 1.0
        w[key] = a.astype(np.float32)
    return w


def make_boards(case, n, seed=1):
    """n boards of random tiles; 5 % of the cells replaced by values in (types, 40): in-range specials,
    out-of-range values and 32 itself; a few cells -1 and 127."""
    rows, columns, types = case[:3]
    rng = np.random.default_rng(seed)
    b = rng.integers(0, types, (n, rows, columns))
    special = rng.random(b.shape) < 0.05
    b = np.where(special, rng.integers(types + 1, 40, b.shape), b)
    flat = b.reshape(-1)
    flat[rng.choice(flat.size, 4, replace=False)] = -1
    flat[rng.choice(flat.size, 4, replace=False)] = 127
    flat[rng.choice(flat.size, 2, replace=False)] = 32
    return b.astype(np.int8)


# ---- the network ------------------------------------------------------------------------------------------
def _fold(w, prefix, cname, bname, eps):
    """float64 (w', b') of a convolution and the BN behind it."""
    k = w[f"{prefix}.{bname}.scale"].astype(np.float64) / np.sqrt(w[f"{prefix}.{bname}.var"].astype(np.float64) + eps)
    wk = w[f"{prefix}.{cname}.kernel"].astype(np.float64) * k
    b = (w[f"{prefix}.{cname}.bias"].astype(np.float64) - w[f"{prefix}.{bname}.mean"].astype(np.float64)) * k \
        + w[f"{prefix}.{bname}.bias"].astype(np.float64)
    return wk, b


def _conv3x3(x, w):
    """SAME 3x3 convolution, NHWC float64: x [n, R, C, I], w [3, 3, I, O]."""
    n, R, C, _ = x.shape
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    out = np.zeros((n, R, C, w.shape[3]))
    for ky in range(3):
        for kx in range(3):
            out += xp[:, ky:ky + R, kx:kx + C, :] @ w[ky, kx]
    return out


def _onehot(boards, CH):
    b = np.asarray(boards).astype(np.int64)
    return ((b[..., None] == np.arange(CH)) & (b[..., None] >= 0)).astype(np.float64)


def _heads(x, w, eps, cast):
    """The two heads over the trunk output x [n, R, C, F] (float64 accumulation); cast: the dtype the
    folded 1x1 weights and the dense weights are held in."""
    n = x.shape[0]
    out = {}
    vw, vb = _fold(w, "value_head", "conv", "bn", eps)
    v1 = np.maximum(x @ vw[0, 0].astype(cast).astype(np.float64) + vb.astype(cast).astype(np.float64), 0.0)
    h1 = np.maximum(v1.reshape(n, -1) @ w["value_head.dense1.kernel"].astype(np.float64)
                    + w["value_head.dense1.bias"].astype(np.float64), 0.0)
    out["values"] = np.maximum(h1 @ w["value_head.dense2.kernel"].astype(np.float64)
                               + w["value_head.dense2.bias"].astype(np.float64), 0.0).reshape(n)
    pw, pb = _fold(w, "policy_head", "conv", "bn", eps)
    p1 = np.maximum(x @ pw[0, 0].astype(cast).astype(np.float64) + pb.astype(cast).astype(np.float64), 0.0)
    out["policy_1x1"] = p1
    out["logits"] = p1.reshape(n, -1) @ w["policy_head.dense.kernel"].astype(np.float64) \
        + w["policy_head.dense.bias"].astype(np.float64)
    return out


def forward_f64(case, w, boards, eps=BN_EPS):
    """Plain float64. Returns values [n], logits [n, A], trunk [L + 1] x [n, R, C, F], policy_1x1."""
    layers = case[3]
    sw, sb = _fold(w, "conv", "conv", "bn", eps)
    x = np.maximum(_conv3x3(_onehot(boards, sw.shape[2]), sw) + sb, 0.0)
    trunk = [x]
    for i in range(layers):
        base = f"residual_block.residual_layers.{i}"
        w1, b1 = _fold(w, base, "conv1", "bn1", eps)
        w2, b2 = _fold(w, base, "conv2", "bn2", eps)
        t = np.maximum(_conv3x3(x, w1) + b1, 0.0)
        x = np.maximum(_conv3x3(t, w2) + b2 + x, 0.0)
        trunk.append(x)
    out = _heads(x, w, eps, np.float64)
    out["trunk"] = trunk
    return out


def stem_model(case, w, boards, eps=BN_EPS):
    """The stem exactly as the device computes it: float32, acc = b'; acc += w'[ky][kx][cell] over the taps
    in ascending (ky, kx) order that lie on the board with a cell in [0, CH); ReLU; bf16. float32 out."""
    rows, columns = case[:2]
    sw, sb = _fold(w, "conv", "conv", "bn", eps)
    sw, sb = sw.astype(np.float32), sb.astype(np.float32)
    CH = sw.shape[2]
    b = np.asarray(boards).astype(np.int64)
    n = len(b)
    bp = np.full((n, rows + 2, columns + 2), -1, np.int64)
    bp[:, 1:-1, 1:-1] = b
    acc = np.broadcast_to(sb, (n, rows, columns, sb.size)).astype(np.float32)
    for ky in range(3):
        for kx in range(3):
            cell = bp[:, ky:ky + rows, kx:kx + columns]
            ok = (cell >= 0) & (cell < CH)
            add = sw[ky, kx][np.where(ok, cell, 0)]
            acc = np.where(ok[..., None], (acc + add).astype(np.float32), acc)
    return bf16_round_f32(np.maximum(acc, np.float32(0.0)))


def forward_model(case, w, boards, eps=BN_EPS):
    """The arithmetic model of the device (module docstring). Same fields as forward_f64."""
    layers = case[3]
    x = stem_model(case, w, boards, eps).astype(np.float64)
    trunk = [x]
    for i in range(layers):
        base = f"residual_block.residual_layers.{i}"
        w1, b1 = _fold(w, base, "conv1", "bn1", eps)
        w2, b2 = _fold(w, base, "conv2", "bn2", eps)
        w1, w2 = bf16_round_f64(w1), bf16_round_f64(w2)
        b1, b2 = b1.astype(np.float32).astype(np.float64), b2.astype(np.float32).astype(np.float64)
        t = bf16_round_f64(np.maximum(_conv3x3(x, w1) + b1, 0.0))
        x = bf16_round_f64(np.maximum(_conv3x3(t, w2) + b2 + x, 0.0))
        trunk.append(x)
    out = _heads(x, w, eps, np.float32)
    out["trunk"] = trunk
    return out


def err(x, ref):
    """e(x) = max |x - ref| / max |ref| over the whole tensor."""
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(np.asarray(x, dtype=np.float64) - ref)) / np.max(np.abs(ref)))
