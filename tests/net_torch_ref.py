"""TEST INFRASTRUCTURE ONLY: the policy/value network in torch on the CPU, float64, written from the layer
list (include/m3.h) and independent of tests/net_ref.py: one_hot, ``conv2d`` in NCHW with the kernels
permuted from [kh][kw][in][out], ``batch_norm`` in evaluation mode (unfolded), NHWC flatten. It checks
the numpy restatement's layout conventions and its folding. torch is a test-only import, and it is
imported in a child process only (``python net_torch_ref.py OUT.npz N``, started once by
tests/test_net_cpu.py): torch brings its own HIP runtime library, which these tests do not load into
the process that runs the library's own."""
import numpy as np
import torch
import torch.nn.functional as Fn


def _t(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


def _conv_bn(x, w, prefix, cname, bname, eps, pad):
    k = _t(w[f"{prefix}.{cname}.kernel"]).permute(3, 2, 0, 1).contiguous()  # [out][in][kh][kw]
    y = Fn.conv2d(x, k, _t(w[f"{prefix}.{cname}.bias"]), padding=pad)
    return Fn.batch_norm(y, _t(w[f"{prefix}.{bname}.mean"]), _t(w[f"{prefix}.{bname}.var"]),
                         _t(w[f"{prefix}.{bname}.scale"]), _t(w[f"{prefix}.{bname}.bias"]), training=False, eps=eps)


def forward_torch(case, w, boards, eps=1e-5):
    rows, columns, types, layers, _ = case
    CH = 2 ** ((types - 1).bit_length() + 2)
    b = torch.from_numpy(np.asarray(boards).astype(np.int64))
    n = b.shape[0]
    ok = (b >= 0) & (b < CH)
    x = Fn.one_hot(torch.where(ok, b, torch.zeros_like(b)), CH).to(torch.float64) * ok[..., None]
    x = x.permute(0, 3, 1, 2)  # NCHW
    x = torch.relu(_conv_bn(x, w, "conv", "conv", "bn", eps, 1))
    trunk = [x.permute(0, 2, 3, 1).numpy().copy()]
    for i in range(layers):
        base = f"residual_block.residual_layers.{i}"
        t = torch.relu(_conv_bn(x, w, base, "conv1", "bn1", eps, 1))
        x = torch.relu(_conv_bn(t, w, base, "conv2", "bn2", eps, 1) + x)
        trunk.append(x.permute(0, 2, 3, 1).numpy().copy())
    v = torch.relu(_conv_bn(x, w, "value_head", "conv", "bn", eps, 0)).permute(0, 2, 3, 1).reshape(n, -1)
    v = torch.relu(v @ _t(w["value_head.dense1.kernel"]) + _t(w["value_head.dense1.bias"]))
    v = torch.relu(v @ _t(w["value_head.dense2.kernel"]) + _t(w["value_head.dense2.bias"]))
    p = torch.relu(_conv_bn(x, w, "policy_head", "conv", "bn", eps, 0)).permute(0, 2, 3, 1).reshape(n, -1)
    p = p @ _t(w["policy_head.dense.kernel"]) + _t(w["policy_head.dense.bias"])
    return dict(values=v.reshape(n).numpy(), logits=p.numpy(), trunk=trunk)


if __name__ == "__main__":
    import sys

    import net_ref

    out = {}
    for i, case in enumerate(net_ref.CASES):
        w = net_ref.make_weights(case)
        b = net_ref.make_boards(case, 3 if case[4] == 256 else int(sys.argv[2]))
        t = forward_torch(case, w, b)
        out[f"{i}.values"], out[f"{i}.logits"] = t["values"], t["logits"]
        for k, x in enumerate(t["trunk"]):
            out[f"{i}.trunk{k}"] = x
    np.savez(sys.argv[1], **out)
