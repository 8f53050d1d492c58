"""TEST INFRASTRUCTURE: one iteration of the CW loop on a batch of clouds of different sizes, in numpy, for any float dtype,
written from the reference's statements (attack/CW/CW_attack.py:121-174) and the definition of the ragged batch — cloud b
counts lengths[b] points, its further rows are copies of its point 0 — and not from the kernel. It is the checker of
tests/test_cw_ragged_cpu.py and tests/test_cw_ragged_gpu.py; the product never imports it.

Everything is channel-first, [B,3,K]. `step` slices every cloud by its length and hands the slice to `step_cloud`, which
knows nothing of padding; what it returns is written back and the padding rows are filled in:

* norm            dist_val = sqrt(sum((adv-ori)^2)) over the cloud's own points                  (:129-131)
* decision        cw_step_restatement.bookkeep, the reference's per-sample loop                  (:136-153)
* gradient        g_model + w/batch (adv-ori)/dist_val (L2Dist) or + 2 w/(batch L) (adv - ori[nn]) (ChamferDist adv2ori)
* Adam            torch.optim.Adam's statements with weight_decay 0 and bias corrections for step t
* clip            ClipPointsLinf(budget): per point, diff * min(budget / (|diff| + 1e-9), 1); budget 0: none
* re-padding      adv rows >= L take the new point 0; input_val (always) and o_bestattack (where copied) take the iterate the
                  pass started from, padding rows = its point 0; m and v of the padding rows stay as they were

Rows at and beyond a length are never read (the CPU test fills them with NaN), with one exception the issue names: a
searched index of the Chamfer term may point at a padding row of ori, which holds ori's point 0.
"""
import numpy as np

import cw_step_restatement as rs

POINT_OUT = ("adv", "m", "v", "input_val", "o_bestattack")
VEC_OUT = ("dist_val", "bestdist", "o_bestdist", "bestscore", "o_bestscore")


def step_cloud(dtype, adv, ori, g_model, m, v, t, w, batch, dist_kind, nn_idx, lr, budget, betas=rs.BETAS, eps=rs.EPS):
    """One cloud [3,L] alone: returns (dist_val, new adv, new m, new v) in `dtype`. batch: the size of the batch whose mean the
    loss is (the 1/B of dist_func(...).mean()); nn_idx [L] with every entry in [0, L)."""
    adv, ori, g_model, m, v = (np.asarray(x, dtype=dtype) for x in (adv, ori, g_model, m, v))
    one = dtype(1)
    L = adv.shape[1]
    diff = adv - ori
    dist_val = np.sqrt(np.sum(diff * diff, dtype=dtype))
    wb = dtype(w) / dtype(batch)
    if dist_kind == 1:
        g = g_model + wb * (diff / dist_val)
    elif dist_kind == 2:
        g = g_model + (dtype(2) * wb / dtype(L)) * (adv - ori[:, nn_idx])
    else:
        g = g_model
    b1, b2 = dtype(betas[0]), dtype(betas[1])
    m = b1 * m + (one - b1) * g
    v = b2 * v + (one - b2) * g * g
    # the bias corrections are scalars of the step number: in double whatever dtype is (as torch computes them)
    step_size = dtype(lr / (1. - betas[0] ** t))
    bc2_sqrt = dtype(np.sqrt(1. - betas[1] ** t))
    p = adv - step_size * (m / (np.sqrt(v) / bc2_sqrt + dtype(eps)))
    if budget > 0:
        d = p - ori
        norm = np.sqrt(np.sum(d * d, axis=0, dtype=dtype))
        scale = np.minimum(dtype(budget) / (norm + dtype(1e-9)), one)
        p = ori + d * scale[None, :]
    return dist_val, p.astype(dtype), m.astype(dtype), v.astype(dtype)


def step(dtype, s, lengths, t, untarget, dist_kind, nn_idx=None, lr=rs.LR, budget=rs.BUDGET, batch=None):
    """One iteration on the padded batch. s: dict of numpy arrays — adv, ori, g, m, v, o_bestattack, input_val [B,3,K]; pred,
    label, bestscore, o_bestscore int64 [B]; bestdist, o_bestdist, w [B]. Returns a dict of new arrays (POINT_OUT in `dtype`,
    the distances in `dtype`, the scores int64) plus "copied" [B] bool; s is not modified."""
    B = len(lengths)
    batch = B if batch is None else batch
    out = {k: np.array(s[k], dtype=dtype) for k in POINT_OUT + ("bestdist", "o_bestdist")}
    out["bestscore"], out["o_bestscore"] = s["bestscore"].copy(), s["o_bestscore"].copy()
    out["dist_val"] = np.zeros(B, dtype=dtype)
    before = np.array(s["adv"], dtype=dtype)
    for b, L in enumerate(int(n) for n in lengths):
        nn = None
        if dist_kind == 2:
            nn = np.asarray(nn_idx[b, :L]).astype(np.int64)
            nn = np.where(nn >= L, 0, nn)              # a padding row of ori holds ori's point 0
        # a contiguous copy: numpy's summation order then depends on the values alone, not on the array the slice came from
        cut = lambda x: np.ascontiguousarray(np.asarray(x)[b, :, :L])        # noqa: E731
        d, p, m, v = step_cloud(dtype, cut(s["adv"]), cut(s["ori"]), cut(s["g"]), cut(s["m"]), cut(s["v"]), t, s["w"][b], batch,
                                dist_kind, nn, lr, budget)
        out["dist_val"][b] = d
        out["adv"][b, :, :L], out["adv"][b, :, L:] = p, p[:, :1]
        out["m"][b, :, :L], out["v"][b, :, :L] = m, v
        out["input_val"][b, :, :L], out["input_val"][b, :, L:] = before[b, :, :L], before[b, :, :1]
    # the decisions on the distances just computed; the copy takes the padded iterate of before the update
    keep = out["o_bestattack"]
    out["copied"] = rs.bookkeep(out["dist_val"], s["pred"], s["label"], untarget, out["bestdist"], out["bestscore"],
                                out["o_bestdist"], out["o_bestscore"], keep, out["input_val"])
    return out


def inputs(lengths, K, seed=0):
    """A padded case in the style of cw_step_restatement.inputs: float32 arrays [B,3,K], a mix of improving, non-improving and
    failing samples (factors 2 and 0.5 around the true distance), the padding rows of ori and adv proper copies of point 0,
    those of g zero (what the victim gives them), of m and v zero. rand_idx [B,K] int32 in [0,K) (it may name padding rows)."""
    B = len(lengths)
    rng = np.random.default_rng(1000 * seed + 31 * K + B)
    f = np.float32
    ori = (rng.random((B, 3, K)) - 0.5).astype(f)
    adv = (ori + 0.1 * rng.standard_normal((B, 3, K))).astype(f)
    g = (1e-3 * rng.standard_normal((B, 3, K))).astype(f)
    m = (1e-3 * rng.standard_normal((B, 3, K))).astype(f)
    v = (1e-6 * rng.random((B, 3, K))).astype(f)
    for b, L in enumerate(lengths):
        ori[b, :, L:], adv[b, :, L:] = ori[b, :, :1], adv[b, :, :1]
        g[b, :, L:] = m[b, :, L:] = v[b, :, L:] = 0
    label = rng.integers(0, 40, B)
    pred = label.copy()
    differs = np.arange(B) % 3 != 2
    pred[differs] = (pred[differs] + 1) % 40
    dist = np.array([np.sqrt(np.sum((adv[b, :, :L].astype(np.float64) - ori[b, :, :L]) ** 2)) for b, L in enumerate(lengths)])
    sel = np.arange(B)
    return dict(adv=adv, ori=ori, g=g, m=m, v=v, label=label.astype(np.int64), pred=pred.astype(np.int64),
                bestdist=np.where(sel % 2 == 0, dist * 2, dist * 0.5).astype(f),
                o_bestdist=np.where(sel % 4 < 2, dist * 2, dist * 0.5).astype(f),
                bestscore=np.full(B, -1, dtype=np.int64), o_bestscore=np.full(B, -1, dtype=np.int64),
                w=(rng.random(B) * 20 + 1).astype(f), o_bestattack=np.zeros((B, 3, K), dtype=f),
                input_val=np.zeros((B, 3, K), dtype=f), rand_idx=rng.integers(0, K, (B, K)).astype(np.int32))
