"""TEST INFRASTRUCTURE: one iteration step of the CW loop in plain torch, for any dtype, written from the reference's own
statements (attack/CW/CW_attack.py:121-174 as oracle.ref_torch.cw_attack has them) and not from the kernels. It is the
checker of tests/test_cw_step_cpu.py (which ties it to the oracle's loop bit for bit) and of tests/test_cw_step_gpu.py
(which holds every form of the device-side update to it in float64); the product never imports it.

Everything is channel-first, [B,3,K], on the CPU, as the reference's loop has it:

* distance        dist_val = sqrt(sum((adv-ori)^2, [1,2]))                                   (:129-131)
* bookkeeping     the per-sample Python loop of :136-153, both comparisons strict
* gradient        g_model + autograd of the reference's distance functor, batch mean included
* Adam            a real torch.optim.Adam whose state (step = t-1, exp_avg = m, exp_avg_sq = v) is injected
* clip            oracle.ref_torch.ClipPointsLinf(budget); budget 0: none

`adam_clip` restates ops.adam_clip_step the same way. `inputs`, `tie_inputs` and `adam_clip_inputs` build the cases both
test files use, `nn_f64` the arg-min the Chamfer term is given, `bands` the tolerance rule.
"""
import functools
import operator

import numpy as np
import torch

from oracle import ref_torch as ort

LR, BUDGET, BETAS, EPS, T = 0.01, 0.18, (0.9, 0.999), 1e-8, 5
FLOAT_OUT = ("adv", "m", "v", "dist_val", "bestdist", "o_bestdist")
INT_OUT = ("bestscore", "o_bestscore")


def dist_value(adv, ori):
    return torch.sqrt(torch.sum((adv - ori) ** 2, dim=[1, 2]))


def bookkeep(dist_val, pred, label, untarget, bestdist, bestscore, o_bestdist, o_bestscore, o_bestattack, input_val,
             overall_lt=operator.lt):
    """CW_attack.py:136-153 on numpy arrays, in place; returns the samples whose iterate was copied. overall_lt exists for
    the teeth test alone (tests/test_cw_step_cpu.py replaces it by <=)."""
    copied = np.zeros(len(dist_val), dtype=bool)
    for e in range(len(dist_val)):
        ok = (pred[e] != label[e]) if untarget else (pred[e] == label[e])
        if dist_val[e] < bestdist[e] and ok:
            bestdist[e], bestscore[e] = dist_val[e], pred[e]
        if overall_lt(dist_val[e], o_bestdist[e]) and ok:
            o_bestdist[e], o_bestscore[e] = dist_val[e], pred[e]
            o_bestattack[e] = input_val[e]
            copied[e] = True
    return copied


def dist_loss(adv, ori, w, dist_kind, nn_idx=None, spelling="gather"):
    """The scalar the reference adds to the adversarial loss (:161-163). dist_kind 1: L2Dist; 2: ChamferDist adv2ori, as the
    reference spells it (spelling "min": through the [B,K,K] matrix) or on the given neighbours (spelling "gather")."""
    if dist_kind == 1:
        return ort.L2Dist()(adv, ori, w).mean()
    if dist_kind != 2:
        raise ValueError(dist_kind)
    if spelling == "min":
        return ort.ChannelFirst(ort.ChamferDist())(adv, ori, w).mean()
    a, o = adv.transpose(1, 2), ori.transpose(1, 2)
    q = torch.gather(o, 1, nn_idx.long()[:, :, None].expand(-1, -1, 3))
    return (torch.mean(torch.sum((a - q) ** 2, dim=2), dim=1) * w.float()).mean()


def dist_grad(dtype, adv, ori, w, dist_kind, nn_idx=None, spelling="gather"):
    if dist_kind == 0:
        return torch.zeros_like(adv, dtype=dtype)
    a = adv.detach().to(dtype).clone().requires_grad_()
    dist_loss(a, ori.to(dtype), w, dist_kind, nn_idx, spelling).backward()
    return a.grad


def adam(p, g, m, v, t, lr, betas, eps):
    """One step of torch.optim.Adam from the injected state; returns (p, m, v) as new tensors."""
    p = p.detach().clone().requires_grad_()
    opt = torch.optim.Adam([p], lr=lr, betas=betas, eps=eps, weight_decay=0.)
    opt.state[p] = {"step": torch.tensor(float(t - 1)), "exp_avg": m.detach().clone(), "exp_avg_sq": v.detach().clone()}
    p.grad = g.detach().clone()
    opt.step()
    st = opt.state[p]
    assert int(st["step"]) == t
    return p.detach(), st["exp_avg"], st["exp_avg_sq"]


def clip(p, ori, budget):
    return ort.ClipPointsLinf(budget)(p.clone().detach(), ori) if budget > 0 else p


def step(dtype, adv, ori, g_model, m, v, t, w, pred, label, untarget, bestdist, bestscore, o_bestdist, o_bestscore,
         o_bestattack, dist_kind, nn_idx, lr, budget, betas=BETAS, eps=EPS, spelling="gather", overall_lt=operator.lt):
    """One iteration. Returns a dict of every tensor the kernels write (FLOAT_OUT, INT_OUT, o_bestattack, input_val) in
    `dtype` / int64, plus "copied" [B] bool. w keeps its own dtype: the functors take it as it comes (ref_torch._w)."""
    adv, ori, g_model, m, v = (x.detach().to(dtype) for x in (adv, ori, g_model, m, v))
    dist_val = dist_value(adv, ori)
    bk = dict(bestdist=bestdist.to(dtype).numpy().copy(), bestscore=bestscore.numpy().copy(),
              o_bestdist=o_bestdist.to(dtype).numpy().copy(), o_bestscore=o_bestscore.numpy().copy(),
              o_bestattack=o_bestattack.to(dtype).numpy().copy())
    input_val = adv.numpy().copy()
    copied = bookkeep(dist_val.numpy(), pred.numpy(), label.numpy(), untarget, input_val=input_val, overall_lt=overall_lt, **bk)
    g = g_model + dist_grad(dtype, adv, ori, w, dist_kind, nn_idx, spelling)
    p, m, v = adam(adv, g, m, v, t, lr, betas, eps)
    out = {k: torch.from_numpy(a) for k, a in bk.items()}
    out.update(adv=clip(p, ori, budget), m=m, v=v, dist_val=dist_val, input_val=torch.from_numpy(input_val),
               copied=torch.from_numpy(copied))
    return out


def project(p, ori, normal, budget):
    """The clip of ops.adam_clip_step: none (ori None), ClipPointsLinf, or ProjectInnerClipLinf (budget 0: projection only)."""
    if ori is None:
        return p
    if normal is None:
        return clip(p, ori, budget)
    fn = ort.ProjectInnerClipLinf(budget) if budget > 0 else ort.ProjectInnerPoints()
    return fn(p.clone().detach(), ori, normal)


def adam_clip(dtype, p, g, g2, m, v, t, lr, ori=None, normal=None, budget=0., betas=BETAS, eps=EPS):
    """ops.adam_clip_step restated: g + g2, the injected Adam, the clip. Returns dict(p, m, v, stepped): `stepped` is the
    iterate before the clip (what the projection's branches look at)."""
    c = lambda x: None if x is None else x.detach().to(dtype)      # noqa: E731
    p, g, g2, m, v, ori, normal = (c(x) for x in (p, g, g2, m, v, ori, normal))
    q, m, v = adam(p, g if g2 is None else g + g2, m, v, t, lr, betas, eps)
    return dict(p=project(q, ori, normal, budget), m=m, v=v, stepped=q)


# ----------------------------------------------------------------------------------------------------------------------
# the tolerance rule
# ----------------------------------------------------------------------------------------------------------------------
def bands(ref64, ref32, names=FLOAT_OUT, keep=None):
    """Per output: 16 x the largest deviation of the fp32 restatement from the float64 one on this very input, floor
    16 x 2^-24 x max|ref|. keep: a mask of the entries that count (same shape as the output), or None."""
    out = {}
    for k in names:
        a, b = ref64[k].double(), ref32[k].double()
        if keep is not None and a.shape == keep.shape:
            a, b = a[keep], b[keep]
        dev = float((a - b).abs().max()) if a.numel() else 0.
        out[k] = 16. * max(dev, 2. ** -24 * (float(a.abs().max()) if a.numel() else 0.))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------------------------------------
def nn_f64(adv, ori, chunk=256):
    """int32 [B,K]: the arg-min over ori of the float64 direct-difference distances of every adv point, in row chunks (no
    [B,K,K] matrix). adv / ori [B,3,K], any device."""
    a, o = adv.double(), ori.double()
    out = []
    for i in range(0, a.shape[2], chunk):
        d = sum((a[:, c, i:i + chunk, None] - o[:, c, None, :]) ** 2 for c in range(3))
        out.append(d.argmin(2))
    return torch.cat(out, 1).to(torch.int32)


FAR = (6e5, -5e5, 7e5)      # the far point of inputs(far=True): |adv - ori| = 1.05e6


@functools.lru_cache(maxsize=None)
def inputs(K, B=3, far=False):
    """The case both test files run at K points (fp32, [B,3,K]); never modified by its users. ori uniform in [-0.5, 0.5],
    adv = ori + 0.1 randn, small gradient and moments, w in [1, 21], and — the recipe of test_cw_riders_gpu._book_state —
    a mix of improving, non-improving and failing samples with factors 2 and 0.5 around the true distance, so that no
    decision sits at rounding distance. far: the last point of sample 0 lies 1e6 away from its original. The clip's
    scale is then 1.7e-7, the one place where its `+ 1e-9` is visible in the result at all; everything else about the
    case is unchanged."""
    g = torch.Generator().manual_seed(31 * K + B)
    ori = torch.rand(B, 3, K, generator=g) - 0.5
    adv = ori + torch.randn(B, 3, K, generator=g) * 0.1
    if far:
        adv[0, :, K - 1] = ori[0, :, K - 1] + torch.tensor(FAR)
    label = torch.randint(0, 40, (B,), generator=g)
    pred = label.clone()
    differs = torch.arange(B) % 3 != 2
    pred[differs] = (pred[differs] + 1) % 40
    dist = dist_value(adv, ori)
    sel = torch.arange(B)
    return dict(adv=adv, ori=ori, label=label, pred=pred,
                bestdist=torch.where(sel % 2 == 0, dist * 2, dist * 0.5).contiguous(),
                o_bestdist=torch.where(sel % 4 < 2, dist * 2, dist * 0.5).contiguous(),
                bestscore=torch.full((B,), -1), o_bestscore=torch.full((B,), -1),
                g=torch.randn(B, 3, K, generator=g) * 1e-3, m=torch.randn(B, 3, K, generator=g) * 1e-3,
                v=torch.rand(B, 3, K, generator=g) * 1e-6, w=torch.rand(B, generator=g) * 20 + 1,
                rand_idx=torch.randint(0, K, (B, K), generator=g).to(torch.int32))


def clipped_share(inp, untarget=True, dist_kind=1):
    """Share of the points of `inp` that lie past BUDGET after Adam and before the clip, on the float64 restatement."""
    r = run(torch.float64, inp, untarget, dist_kind, nn_idx=inp["rand_idx"], budget=0.)
    return float((torch.sum((r["adv"] - inp["ori"].double()) ** 2, dim=1).sqrt() > BUDGET).double().mean())


def run(dtype, inp, untarget, dist_kind, nn_idx=None, t=T, budget=BUDGET, **over):
    """step() on a case of inputs() / tie_inputs(); `over` replaces single inputs."""
    a = {k: over.get(k, inp[k]) for k in inp}
    return step(dtype, a["adv"], a["ori"], a["g"], a["m"], a["v"], t, a["w"], a["pred"], a["label"], untarget, a["bestdist"],
                a["bestscore"], a["o_bestdist"], a["o_bestscore"], over.get("o_bestattack", torch.zeros_like(a["adv"])),
                dist_kind, nn_idx, LR, budget, **{k: over[k] for k in ("spelling", "overall_lt") if k in over})


TIE_DIST = 5 * 2. ** -10


@functools.lru_cache(maxsize=None)
def tie_inputs(K, untarget):
    """Five samples whose distance is EXACT in any summation order: ori and adv - ori are multiples of 2^-10, one point per
    sample moved by (3,4,0) x 2^-10, the rest unmoved, so dist = 5 x 2^-10. Per sample: bestdist = dist (no update);
    bestdist = nextafter(dist) (update); o_bestdist = dist under a larger bestdist (per-step best only, no copy);
    o_bestdist = 0; a failing sample with everything above (nothing happens)."""
    B = 5
    g = torch.Generator().manual_seed(977 + K)
    ori = torch.randint(-512, 513, (B, 3, K), generator=g).float() / 1024
    adv = ori.clone()
    for b in range(B):
        k = (K - 1 - 211 * b) % K          # sample 0: the last lane of the last register tile
        adv[b, :, k] += torch.tensor([3., 4., 0.]) / 1024
    label = torch.randint(0, 40, (B,), generator=g)
    succeeds = torch.tensor([True, True, True, True, False])
    pred = torch.where(succeeds == bool(untarget), (label + 1) % 40, label)
    d = np.float32(TIE_DIST)
    up = float(np.nextafter(d, np.float32(np.inf)))
    return dict(adv=adv, ori=ori, label=label, pred=pred, bestdist=torch.tensor([float(d), up, 1., 1., 1.]),
                o_bestdist=torch.tensor([1., 1., float(d), 0., 1.]), bestscore=torch.full((B,), -1),
                o_bestscore=torch.full((B,), -1), g=torch.randn(B, 3, K, generator=g) * 1e-3,
                m=torch.randn(B, 3, K, generator=g) * 1e-3, v=torch.rand(B, 3, K, generator=g) * 1e-6,
                w=torch.rand(B, generator=g) * 20 + 1)


N_OPPOSITE = 7


@functools.lru_cache(maxsize=None)
def adam_clip_inputs(K, B=3):
    """p, ori, g, g2, m, v, normal [B,3,K + 7] for ops.adam_clip_step: random unit normals against a random offset of 0.1
    randn, and 7 constructed rows at the end of every cloud with g = g2 = m = v = 0 — Adam then moves them by exactly 0 —
    whose offset d is a multiple of 2^-10 and whose normal is -3 d: the projection's "opposite" branch (inner < 0 and
    n x d = 0), which puts them back onto ori."""
    g = torch.Generator().manual_seed(4243 + K)
    n = K + N_OPPOSITE
    ori = torch.randint(-512, 513, (B, 3, n), generator=g).float() / 1024
    p = ori + torch.randn(B, 3, n, generator=g) * 0.1
    normal = torch.randn(B, 3, n, generator=g)
    normal = normal / normal.norm(dim=1, keepdim=True)
    t = dict(g=torch.randn(B, 3, n, generator=g) * 1e-3, g2=torch.randn(B, 3, n, generator=g) * 1e-3,
             m=torch.randn(B, 3, n, generator=g) * 1e-3, v=torch.rand(B, 3, n, generator=g) * 1e-6)
    d = torch.randint(1, 9, (B, 3, N_OPPOSITE), generator=g).float() / 1024
    d = d * (torch.randint(0, 2, (B, 3, N_OPPOSITE), generator=g).float() * 2 - 1)
    p[:, :, K:] = ori[:, :, K:] + d
    normal[:, :, K:] = -3 * d
    for x in t.values():
        x[:, :, K:] = 0
    return dict(p=p, ori=ori, normal=normal, **t)


def projection_keep(stepped, ori, normal):
    """bool [B,K]: the points whose projection branch is decided beyond rounding, on float64 values: `inner` farther than
    1e-6 |d||n| from 0, and |n x d| not within a factor 2 of the 1e-6 threshold."""
    d = stepped.double() - ori.double()
    n = normal.double()
    inner = torch.sum(d * n, dim=1)
    cr = torch.cross(n, d, dim=1).norm(dim=1)
    return (inner.abs() > 1e-6 * d.norm(dim=1) * n.norm(dim=1)) & ~((cr >= 0.5e-6) & (cr <= 2e-6))
