"""Plain-torch statement of PointNetCls(k, feature_transform=True) in eval mode, written from the math and generic in
dtype and device. It is the same-device comparator of tests/test_pointnet_ft_gpu.py and tools/bench_pointnet_ft.py,
and tests/test_pointnet_ft_cpu.py checks it in float64 against the reference's own float64 outputs.

    x'  = T3^T x                      T3 = I + head3(max_n relu-tower_{3->64->128->1024}(x))
    h   = relu(W1 x' + b1)            [64, N]
    Tf  = I + headk(max_n relu-tower_{64->64->128->1024}(h))
    u   = Tf^T h
    z2  = relu(W2 u + b2)
    pooled = max_n (W3 z2 + b3)       logp = log_softmax(head(pooled))

Every (W, b) is a 1x1 conv / linear with its eval-mode BatchNorm applied as the affine map it is."""
import torch


def _affine(sd, prefix, lin, bn, x, dtype):
    """bn(lin(x)) for x [B, C, N] (conv1d, kernel 1) or [B, C] (linear); bn None: the bare layer."""
    w = sd[f"{prefix}{lin}.weight"].to(dtype).reshape(sd[f"{prefix}{lin}.weight"].shape[0], -1)
    b = sd[f"{prefix}{lin}.bias"].to(dtype)
    y = torch.einsum("oc,bc...->bo...", w, x) + b.reshape((1, -1) + (1,) * (x.dim() - 2))
    if bn is None:
        return y
    g, beta = sd[f"{prefix}{bn}.weight"].to(dtype), sd[f"{prefix}{bn}.bias"].to(dtype)
    mean, var = sd[f"{prefix}{bn}.running_mean"].to(dtype), sd[f"{prefix}{bn}.running_var"].to(dtype)
    shape = (1, -1) + (1,) * (x.dim() - 2)
    return (y - mean.reshape(shape)) / torch.sqrt(var.reshape(shape) + 1e-5) * g.reshape(shape) + beta.reshape(shape)


def _stn(sd, prefix, x, k, dtype):
    """I + head(max_n relu-tower(x)) -> [B, k, k]  (STN3d: k = 3, STNkd: k = 64)."""
    y = torch.relu(_affine(sd, prefix, "conv1", "bn1", x, dtype))
    y = torch.relu(_affine(sd, prefix, "conv2", "bn2", y, dtype))
    y = torch.relu(_affine(sd, prefix, "conv3", "bn3", y, dtype))
    y = y.max(dim=2)[0]
    y = torch.relu(_affine(sd, prefix, "fc1", "bn4", y, dtype))
    y = torch.relu(_affine(sd, prefix, "fc2", "bn5", y, dtype))
    y = _affine(sd, prefix, "fc3", None, y, dtype)
    return y.reshape(-1, k, k) + torch.eye(k, dtype=dtype, device=x.device)


def forward(sd, x, dtype=None):
    """sd: a PointNetCls(k, feature_transform=True) state_dict (tensors on x's device); x [B,3,N].
    Returns (logp [B,k], trans [B,3,3], trans_feat [B,64,64]); differentiable in x."""
    dtype = dtype or x.dtype
    x = x.to(dtype)
    trans = _stn(sd, "feat.stn.", x, 3, dtype)
    xp = torch.einsum("bcd,bcn->bdn", trans, x)                 # x' = T3^T x
    h = torch.relu(_affine(sd, "feat.", "conv1", "bn1", xp, dtype))
    tf = _stn(sd, "feat.fstn.", h, 64, dtype)
    u = torch.einsum("bij,bin->bjn", tf, h)                     # u = Tf^T h
    z2 = torch.relu(_affine(sd, "feat.", "conv2", "bn2", u, dtype))
    pooled = _affine(sd, "feat.", "conv3", "bn3", z2, dtype).max(dim=2)[0]
    y = torch.relu(_affine(sd, "", "fc1", "bn1", pooled, dtype))
    y = torch.relu(_affine(sd, "", "fc2", "bn2", y, dtype))     # dropout is the identity in eval mode
    y = _affine(sd, "", "fc3", None, y, dtype)
    return torch.log_softmax(y, dim=1), trans, tf
