"""TEST INFRASTRUCTURE: a plain-torch restatement of the reference's shape_invariant_ifgm (attack/SIadv/SIadv_attack.py:
205-340), batched, for any device and dtype. It is the checker of tests/test_siadv_*.py and the same-GPU baseline of
tools/bench_siadv.py; the product never imports it. Points and normals are [B,N,3] here, as in the reference.

The normals are the definition the fixture's open3d stand-in uses (tests/golden/make_golden_siadv.py): the K = 20
nearest points including the point itself, their covariance about their mean, the eigenvector of the smallest
eigenvalue by `eigh`, (0,0,1) for a zero covariance. The sign is whatever `eigh` returns: the step does not depend on it.
"""
import numpy as np
import torch

KNN = 20


def knn_lists(P, k=KNN, extra=0):
    """idx [B,N,k] of the k nearest points (self included), and the squared distances [B,N,k+extra] ascending."""
    d2 = ((P[:, :, None, :] - P[:, None, :, :]) ** 2).sum(-1)
    d, idx = torch.topk(d2, min(k + extra, P.shape[1]), dim=2, largest=False, sorted=True)
    return idx[:, :, :k], d


def pca_normals(P, idx):
    """Smallest eigenvector [B,N,3] of the covariance of the listed points; (0,0,1) where the covariance is zero."""
    B, N, K = idx.shape
    nb = torch.gather(P[:, None].expand(B, N, N, 3), 2, idx[..., None].expand(B, N, K, 3).long())
    d = nb - nb.mean(2, keepdim=True)
    cov = d.transpose(2, 3) @ d / K
    w, v = torch.linalg.eigh(cov)
    n = v[..., 0]
    default = torch.zeros_like(n)
    default[..., 2] = 1
    return torch.where((cov.abs().amax((2, 3)) == 0)[..., None], default, n)


def estimate_normals(P):
    return pca_normals(P, knn_lists(P)[0])


def spin_axis_matrix(n):
    """get_spin_axis_matrix (:217-247) for normals [B,N,3]: U [B,N,3,3], the |z^2 - 1| < 1e-4 rows included."""
    x, y, z = n[..., 0], n[..., 1], n[..., 2]
    den = torch.sqrt(1 - z ** 2)
    zero = torch.zeros_like(z)
    u = torch.stack([torch.stack([y / den, -x / den, zero], -1),
                     torch.stack([x * z / den, y * z / den, -den], -1), n], -2)
    r = 1 / np.sqrt(2)
    bound = torch.stack([torch.stack([zero + r, zero - r, zero], -1),
                         torch.stack([z / np.sqrt(2), z / np.sqrt(2), zero], -1),
                         torch.stack([zero, zero, z], -1)], -2)
    return torch.where((abs(z ** 2 - 1) < 1e-4)[..., None, None], bound, u)


def round_trip(P, n):
    """The cloud the reference shows the victim (:293-298): U^T (U (P + t)) - t. At the rewritten rows of U it is not P."""
    U = spin_axis_matrix(n)
    t = (P * n).sum(-1, keepdim=True) * n
    Pp = (U @ (P + t)[..., None])[..., 0]
    return (U.transpose(-1, -2) @ Pp[..., None])[..., 0] - t


def si_step(P, ori, g, n, step_size, eps):
    """One step (:293-320) from the gradient g = dL/d(round_trip(P, n)) [B,N,3]: the literal formulas, g' = U g by the
    chain rule."""
    U = spin_axis_matrix(n)
    t = (P * n).sum(-1, keepdim=True) * n
    Pp = (U @ (P + t)[..., None])[..., 0]
    gp = (U @ g[..., None])[..., 0].clone()
    gp[..., 2] = 0.
    norm = torch.sum(gp ** 2, dim=[1, 2]) ** 0.5
    Pp = Pp - step_size * np.sqrt(3 * 1024) * gp / (norm[:, None, None] + 1e-9)
    P = (U.transpose(-1, -2) @ Pp[..., None])[..., 0] - t
    return ori + torch.clamp(P - ori, min=-eps, max=eps)


def tangent_projection_step(P, ori, g, n, step_size, eps):
    """The shortcut the product must NOT take: g - (n.g) n in place of U^T (U g with g'_z = 0)."""
    gt = g - (n * g).sum(-1, keepdim=True) * n
    norm = torch.sum(gt ** 2, dim=[1, 2]) ** 0.5
    P = P - step_size * np.sqrt(3 * 1024) * gt / (norm[:, None, None] + 1e-9)
    return ori + torch.clamp(P - ori, min=-eps, max=eps)


def cw_loss(logits, target, top5=False):
    """CWLoss (:142-164) with kappa 0, untargeted, summed over the batch."""
    onehot = torch.eye(logits.shape[1], dtype=logits.dtype, device=logits.device)[target.long()]
    real = torch.sum(onehot * logits, 1)
    masked = (1 - onehot) * logits - onehot * 10000
    other = torch.topk(masked, 5)[0][:, 4] if top5 else torch.max(masked, 1)[0]
    return torch.sum(torch.max(real - other, torch.zeros_like(other)))


def point_grad(model, P, target, top5=False, pre_head=None):
    """(dL/dP [B,N,3], loss) of the surrogate at P [B,N,3]."""
    Pc = P.detach().transpose(1, 2).contiguous().requires_grad_()
    inp = pre_head(Pc) if pre_head is not None else Pc
    out = model(inp)
    loss = cw_loss(out[0] if isinstance(out, (tuple, list)) else out, target, top5)
    (g,) = torch.autograd.grad(loss, Pc)
    return g.transpose(1, 2), loss.detach()


def run_loop(model, points, target, eps, step_size, max_steps, top5=False, normals=estimate_normals, record=None):
    """The whole loop from points [B,N,6]; returns the coordinates [B,N,3]. record: a dict that receives the lists
    P (P_0 ... P_max_steps), n and g (the normals and the gradient used by each step)."""
    n = points[:, :, 3:]
    n = n / torch.sqrt(torch.sum(n ** 2, dim=-1, keepdim=True))
    P = points[:, :, :3]
    ori = P
    if record is not None:
        record.update(P=[P], n=[], g=[])
    for i in range(max_steps):
        g, _ = point_grad(model, round_trip(P, n), target, top5)
        Pn = si_step(P, ori, g, n, step_size, eps)
        if record is not None:
            record["P"].append(Pn), record["n"].append(n), record["g"].append(g)
        P = Pn
        if i + 1 < max_steps:
            n = normals(P)
    return P
