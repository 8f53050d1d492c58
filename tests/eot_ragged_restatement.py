"""The ragged twins of csrc/eot.hip (pc3d_eot_prepare_ragged_f32, pc3d_eot_update_ragged_f32, pc3d_eot_draw_ragged_f32)
restated: tests/eot_restatement.py's formulas applied to every cloud's own [1,3,L] slice and padded the way include/pc3d.h
says, and tests/eot_draw_restatement.py's draw at K = L. No package code.

Shapes: adv / ori [B,3,K] (K the capacity), lengths a list of B ints; rot [E,3,3], idx [E,B,K] and inv [E,B,K,2] are ONE
iteration's row of the per-cloud tables.
"""
import numpy as np
import torch

import eot_draw_restatement as dr
import eot_restatement as rs


def _pad(x, K):
    """x [..., L] -> [..., K]: the columns from L on are copies of column 0."""
    L = x.shape[-1]
    return torch.cat([x, x[..., :1].expand(*x.shape[:-1], K - L)], -1) if L < K else x


def prepare(adv, ori, lengths, rot=None, idx=None, renorm=False, dtype=torch.float64):
    """(X [(1+E) B,3,K] padded with every slot's column 0, centroid [S,B,3], scale [S,B], arg [S,B])."""
    B, _, K = adv.shape
    X, c, s, arg = [], [], [], []
    for b, L in enumerate(lengths):
        ib = None if idx is None else idx[:, b, :L]
        x, cb, sb, ab = rs.prepare(adv[b:b + 1, :, :L], ori[b:b + 1, :, :L], rot, ib, renorm, dtype)
        X.append(_pad(x, K)), c.append(cb), s.append(sb), arg.append(ab)        # x [S,3,L]
    S = X[0].shape[0]
    return torch.stack(X, 1).reshape(S * B, 3, K), torch.cat(c, 1), torch.cat(s, 1), torch.cat(arg, 1)


def update(adv, ori, lengths, gx, m, v, step, pred, goal, untarget, bestdist, bestscore, o_bestdist, o_bestscore, o_bestattack,
           rot=None, inv=None, renorm=False, dist_kind="chamfer", w=None, nn_idx=None, batch_mean=None, one_d=True, box=0.4,
           lr=rs.LR, dtype=torch.float64):
    """One pc3d_eot_update_ragged_f32 launch as a dict of every output, [B, ...] each. adv and input_val are padded with
    their row 0, o_bestattack where it was copied (elsewhere it is the input); g, m, v hold the rows < L and zeros behind
    (the launch leaves those rows alone). batch_mean None: B, the whole batch."""
    B, _, K = adv.shape
    S = gx.shape[0] // B
    bm = B if batch_mean is None else batch_mean
    outs = []
    for b, L in enumerate(lengths):
        one = rs.update(adv[b:b + 1, :, :L], ori[b:b + 1, :, :L], gx.reshape(S, B, 3, K)[:, b, :, :L], m[b:b + 1, :, :L],
                        v[b:b + 1, :, :L], step, pred[b:b + 1], goal[b:b + 1], untarget, bestdist[b:b + 1], bestscore[b:b + 1],
                        o_bestdist[b:b + 1], o_bestscore[b:b + 1], o_bestattack[b:b + 1, :, :L], rot=rot,
                        inv=None if inv is None else inv[:, b, :L], renorm=renorm, dist_kind=dist_kind, w=w[b:b + 1],
                        nn_idx=None if nn_idx is None else nn_idx[b:b + 1, :L], batch_mean=bm, one_d=one_d, box=box, lr=lr,
                        dtype=dtype)
        for k in ("adv", "input_val"):
            one[k] = _pad(one[k], K)
        one["o_bestattack"] = _pad(one["o_bestattack"], K) if bool(one["upd_o"][0]) else o_bestattack[b:b + 1].to(dtype)
        for k in ("g", "m", "v"):
            one[k] = torch.cat([one[k], torch.zeros((1, 3, K - L), dtype=dtype, device=adv.device)], -1)
        outs.append(one)
    return {k: torch.cat([o[k] for o in outs]) for k in outs[0]}


def draw(seed, n, e, lengths, K):
    """(rot float64 [3,3], idx int64 [B,K], inv int32 [B,K,2]) of draw index n, view e: cloud b's rows < L are the dense
    draw's at K = L; behind them idx repeats the cloud's idx[0] and inv is -1. The rotation does not know a length."""
    B = len(lengths)
    idx = np.empty((B, K), dtype=np.int64)
    inv = np.full((B, K, 2), -1, dtype=np.int32)
    for b, L in enumerate(lengths):
        _, ib, vb = dr.draw(seed, n, e, L)
        idx[b, :L], idx[b, L:], inv[b, :L] = ib, ib[0], vb
    return dr.rotation(seed, n, e), idx, inv
