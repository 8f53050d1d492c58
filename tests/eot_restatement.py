"""The two kernels of csrc/eot.hip (pc3d_eot_prepare_f32, pc3d_eot_update_f32) restated as plain torch formulas — no
autograd, no package code. Everything is evaluated in `dtype` (float64 for the reference; float32 on the GPU gives the
"same-device fp32 restatement" whose distance from float64 sets the tests' bands).

Tie rule of the renormalisation's maximum norm: the LOWEST index. tests/test_eot_cpu.py holds this file's gradient to
autograd through torch's own max(dim) on the CPU, on a cloud with two points tied for the maximum: torch's CPU
max(dim) returns — and its backward routes the gradient to — the first of the tied entries, so that is what the kernel
implements.

Shapes: adv / ori [B,3,K]; rot [E,3,3] and idx [E,K] / inv [E,K,2] are ONE iteration's row of the tables.
"""
import torch

LR = 1e-2
BETAS = (0.9, 0.999)
EPS = 1e-8


def inverse_table(idx, K):
    """inv [E,K,2] (int64, -1 = none): the at most two columns j with idx[e,j] mod K == i, ascending."""
    E = idx.shape[0]
    inv = torch.full((E, K, 2), -1, dtype=torch.int64)
    for e in range(E):
        for j in range(K):
            i = int(idx[e, j]) % K
            inv[e, i, 0 if inv[e, i, 0] < 0 else 1] = j
    return inv


def slots(adv, ori, rot):
    """p [S,B,3,K]: slot 0 the iterate, slot e >= 1 = R_e ori + (adv - ori)."""
    out = [adv]
    if rot is not None:
        for e in range(rot.shape[0]):
            R = rot[e].to(adv.dtype).to(adv.device)
            out.append((R[None, :, :, None] * ori[:, None, :, :]).sum(2) + (adv - ori))
    return torch.stack(out)


def centre_scale(p):
    """centroid [S,B,3], scale [S,B], arg [S,B] (lowest index of the maximum norm) of p [S,B,3,K]."""
    K = p.shape[-1]
    c = p.sum(-1) / K
    q = p - c[..., None]
    n = torch.sqrt((q * q).sum(2))
    s = n.max(-1)[0]
    ar = torch.arange(K, device=p.device).expand_as(n)
    arg = torch.where(n == s[..., None], ar, torch.full_like(ar, K)).min(-1)[0]
    return c, s, arg


def prepare(adv, ori, rot=None, idx=None, renorm=False, dtype=torch.float64):
    """(X [(1+E) B,3,K], centroid [S,B,3], scale [S,B], arg [S,B])."""
    adv, ori = adv.to(dtype), ori.to(dtype)
    B, _, K = adv.shape
    p = slots(adv, ori, rot)
    S = p.shape[0]
    if renorm:
        c, s, arg = centre_scale(p)
        y = (p - c[..., None]) / s[..., None, None]
    else:
        c = torch.zeros((S, B, 3), dtype=dtype, device=adv.device)
        s = torch.ones((S, B), dtype=dtype, device=adv.device)
        arg = torch.zeros((S, B), dtype=torch.int64, device=adv.device)
        y = p
    if idx is not None:
        cols = (idx.long() % K).to(adv.device)
        y = torch.stack([y[0]] + [y[e][:, :, cols[e - 1]] for e in range(1, S)])
    return y.reshape(S * B, 3, K), c, s, arg


def adv_gradient(adv, ori, gx, rot=None, inv=None, renorm=False, dtype=torch.float64):
    """d (sum over the views of <gx_e, x_e>) / d adv, [B,3,K]: without views, slot 0's gradient."""
    adv, ori, gx = adv.to(dtype), ori.to(dtype), gx.to(dtype)
    B, _, K = adv.shape
    p = slots(adv, ori, rot)
    E = p.shape[0] - 1
    if renorm:
        c, s, arg = centre_scale(p)
    G = torch.zeros_like(adv)
    for e in (range(1, E + 1) if E else [0]):
        g = gx[e * B:(e + 1) * B]
        if inv is not None and e >= 1:
            iv = inv[e - 1].to(adv.device)
            j, has = iv.clamp(min=0), (iv >= 0).to(dtype)
            g = g[:, :, j[:, 0]] * has[:, 0] + g[:, :, j[:, 1]] * has[:, 1]
        if renorm:
            q = p[e] - c[e][..., None]
            se = s[e]
            ds = -(g * q).sum((1, 2)) / (se * se)
            gq = g / se[:, None, None]
            for b in range(B):
                qa = q[b, :, arg[e, b]]
                gq[b, :, arg[e, b]] = gq[b, :, arg[e, b]] + ds[b] * qa / torch.sqrt((qa * qa).sum())
            g = gq - gq.sum(-1, keepdim=True) / K
        G = G + g
    return G


def distance(adv, ori, dist_kind, w, nn_idx=None, batch_mean=None, dtype=torch.float64):
    """(dist [B], its gradient [B,3,K] inside a mean over batch_mean clouds). dist_kind 'chamfer' (adv -> ori on nn_idx) / 'l2'."""
    adv, ori, w = adv.to(dtype), ori.to(dtype), w.to(dtype)
    B, _, K = adv.shape
    bm = batch_mean if batch_mean is not None else B
    if dist_kind == "chamfer":
        near = torch.gather(ori, 2, nn_idx.long()[:, None, :].expand(B, 3, K))
        d = adv - near
        return w * ((d * d).sum(1).sum(1) / K), (2.0 * w / (bm * K))[:, None, None] * d
    if dist_kind == "l2":
        d = adv - ori
        nrm = torch.sqrt((d * d).sum((1, 2)))
        return w * nrm, (w / bm)[:, None, None] * d / nrm[:, None, None]
    return torch.zeros_like(w), torch.zeros_like(adv)


def update(adv, ori, gx, m, v, step, pred, goal, untarget, bestdist, bestscore, o_bestdist, o_bestscore, o_bestattack,
           rot=None, inv=None, renorm=False, dist_kind="chamfer", w=None, nn_idx=None, batch_mean=None, one_d=True, box=0.4,
           lr=LR, dtype=torch.float64):
    """One pc3d_eot_update_f32 launch; returns a dict of every output (inputs are left alone)."""
    adv0, ori0 = adv.to(dtype), ori.to(dtype)
    B = adv.shape[0]
    dist, gd = distance(adv, ori, dist_kind, w, nn_idx, batch_mean, dtype)
    succ = (pred[:B] != goal) if untarget else (pred[:B] == goal)
    bd, obd = bestdist.to(dtype), o_bestdist.to(dtype)
    upd, upd_o = succ & (dist < bd), succ & (dist < obd)          # a NaN distance compares false
    out = dict(dist=dist, upd=upd, upd_o=upd_o,
               bestdist=torch.where(upd, dist, bd), bestscore=torch.where(upd, pred[:B], bestscore),
               o_bestdist=torch.where(upd_o, dist, obd), o_bestscore=torch.where(upd_o, pred[:B], o_bestscore),
               o_bestattack=torch.where(upd_o[:, None, None], adv0, o_bestattack.to(dtype)), input_val=adv0.clone())
    g = adv_gradient(adv, ori, gx, rot, inv, renorm, dtype) + gd
    b1, b2 = BETAS
    m1 = m.to(dtype) + (g - m.to(dtype)) * (1.0 - b1)
    v1 = v.to(dtype) * b2 + (1.0 - b2) * g * g
    denom = torch.sqrt(v1) / (1.0 - b2 ** step) ** 0.5 + EPS
    x = adv0 - (lr / (1.0 - b1 ** step)) * (m1 / denom)
    if one_d:
        z = torch.maximum(torch.minimum(x[:, 2], ori0[:, 2] + box), ori0[:, 2] - box)
        x = torch.stack([ori0[:, 0], ori0[:, 1], z], 1)
    out.update(g=g, m=m1, v=v1, adv=x)
    return out
