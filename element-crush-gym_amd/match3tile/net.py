"""The reference's policy/value network (``ElementCrush``, elementCrush.py:51-97, elementGOModules.py) in
inference form on the device: ``m3_net_*`` of include/m3.h, kernels in csrc/m3_net.hip. No ML framework
is loaded: the weights are a flat dict of float32 numpy arrays named by the flax state paths
(INTEGRATION.md has the lines that flatten ``nnx.state(model)`` into it), and ``np.savez`` / ``np.load``
of that dict is the file format.

BatchNorm runs on the stored running statistics (the reference never switches its
model to evaluation mode, which is not reproduced)."""
from __future__ import annotations

import ctypes
from typing import Dict, List, Tuple

import numpy as np

from . import _native
from .search import onehot_width

# flax.nnx.BatchNorm's documented default epsilon. Flax is not installed where this was written and has
# not been run: pass the value your model was built with if it differs.
BN_EPSILON = 1e-5

_BN = ("scale", "bias", "mean", "var")


def weight_spec(cfg, layers: int, features: int) -> List[Tuple[str, tuple]]:
    """(key, shape) of every weight array, in the order of m3_net_create's blob."""
    P, A, F = cfg.rows * cfg.columns, cfg.action_space, int(features)
    CH = onehot_width(cfg.types)

    def conv(prefix, conv_name, bn_name, kh, cin, cout):
        out = [(f"{prefix}.{conv_name}.kernel", (kh, kh, cin, cout)), (f"{prefix}.{conv_name}.bias", (cout,))]
        return out + [(f"{prefix}.{bn_name}.{k}", (cout,)) for k in _BN]

    spec = conv("conv", "conv", "bn", 3, CH, F)
    for i in range(int(layers)):
        base = f"residual_block.residual_layers.{i}"
        spec += conv(base, "conv1", "bn1", 3, F, F) + conv(base, "conv2", "bn2", 3, F, F)
    spec += conv("value_head", "conv", "bn", 1, F, 1)
    spec += [("value_head.dense1.kernel", (P, F)), ("value_head.dense1.bias", (F,)),
             ("value_head.dense2.kernel", (F, 1)), ("value_head.dense2.bias", (1,))]
    spec += conv("policy_head", "conv", "bn", 1, F, 2)
    spec += [("policy_head.dense.kernel", (2 * P, A)), ("policy_head.dense.bias", (A,))]
    return spec


class ElementCrushNet:
    """``ElementCrushNet(cfg, layers, features, weights, bn_epsilon=1e-5)``: the network of
    ``ElementCrush(cfg, layers, features)`` with the given weights, on the device.

    ``weights``: dict of float32 arrays (``weight_spec`` lists keys and shapes); a missing key, an extra
    key or a wrong shape is a ValueError that names the key. ``features`` must be a multiple of 32 in
    32..512.

    - ``forward(boards [n, R, C]) -> (values f32 [n], logits f32 [n, A])``: raw logits, no softmax.
    - ``trunk(boards, upto) -> f32 [n, R, C, F]``: the activations after the stem (``upto = 0``) or
      after residual layer ``upto``.
    - ``net(x [B, R, C]) -> (value [B, 1], policy [B, A])``: the reference model's calling convention,
      so a net can stand where the reference passes ``model``.

    Any int8 cell is accepted: a cell < 0 or >= the one-hot width is the zero vector. A board's outputs
    do not depend on the batch it is evaluated in."""

    def __init__(self, cfg, layers: int, features: int, weights: Dict[str, np.ndarray], bn_epsilon: float = BN_EPSILON):
        self.cfg, self.layers, self.features = cfg, int(layers), int(features)
        if self.layers < 0:
            raise ValueError(f"layers = {layers}: must be >= 0")
        if self.features % 32 or not 32 <= self.features <= 512:
            raise ValueError(f"features = {features}: a multiple of 32 in 32..512 is supported")
        spec = weight_spec(cfg, self.layers, self.features)
        names = {k for k, _ in spec}
        parts = []
        for key, shape in spec:
            if key not in weights:
                raise ValueError(f"weights: missing key {key!r}")
            a = np.asarray(weights[key])
            if a.shape != shape:
                raise ValueError(f"weights: {key!r} has shape {a.shape}, expected {shape}")
            parts.append(np.ascontiguousarray(a, dtype=np.float32).reshape(-1))
        for key in weights:
            if key not in names:
                raise ValueError(f"weights: unexpected key {key!r}")
        blob = np.concatenate(parts)
        self._ctx = ctx = _native.context(cfg.rows, cfg.columns, cfg.types)
        self.rows, self.columns, self.A = cfg.rows, cfg.columns, ctx.A
        h = ctypes.c_void_p()
        with ctx._lock:
            _native.check(_native.lib().m3_net_create(ctx.handle, cfg.rows, cfg.columns, cfg.types, self.layers,
                                                      self.features, float(bn_epsilon), _native.ptr(blob), blob.size,
                                                      ctypes.byref(h)))
        self._h = h

    @classmethod
    def from_npz(cls, path, cfg, layers: int, features: int, bn_epsilon: float = BN_EPSILON):
        """The net of a ``np.savez`` file of the weight dict."""
        with np.load(path) as z:
            return cls(cfg, layers, features, {k: z[k] for k in z.files}, bn_epsilon)

    def close(self):
        if getattr(self, "_h", None):
            _native.lib().m3_net_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def _boards(self, boards):
        b = np.asarray(boards)
        if b.size and (b.min() < -128 or b.max() > 127):
            raise ValueError("cell values must fit int8")
        return np.ascontiguousarray(b.reshape(-1, self._ctx.N), dtype=np.int8)

    def forward(self, boards):
        b = self._boards(boards)
        n = len(b)
        values, logits = np.empty(n, np.float32), np.empty((n, self.A), np.float32)
        with self._ctx._lock:
            _native.check(_native.lib().m3_net_forward(self._h, _native.ptr(b), n, _native.ptr(values),
                                                       _native.ptr(logits)))
        return values, logits

    def forward_device(self, d_boards, n: int, d_values, d_logits, d_need=None, sync: bool = True):
        """m3_net_forward_device on ``_native.DeviceArray``s (or pointers) of this net's context."""
        pb, pn, pv, pl = (getattr(d, "ptr", d) for d in (d_boards, d_need, d_values, d_logits))
        with self._ctx._lock:
            _native.check(_native.lib().m3_net_forward_device(self._h, pb, pn, int(n), pv, pl))
            if sync:
                _native.check(_native.lib().m3_ctx_synchronize(self._ctx.handle))

    def trunk(self, boards, upto: int):
        b = self._boards(boards)
        n = len(b)
        out = np.empty((n, self.rows, self.columns, self.features), np.float32)
        with self._ctx._lock:
            _native.check(_native.lib().m3_net_trunk(self._h, _native.ptr(b), n, int(upto), _native.ptr(out)))
        return out

    def __call__(self, x):
        values, logits = self.forward(np.asarray(x).reshape(-1, self.rows, self.columns))
        return values.reshape(-1, 1), logits
