"""TEST INFRASTRUCTURE: one whole iteration update of GeoA3 in plain torch, for any dtype, on GIVEN index arrays, written
from the reference's own statements (attack/GeoA3/GeoA3_attack.py:92-102 lp_clip, :139-181 the terms, :321-351 record and
optimiser, loss_utils.py:36-105) and not from the kernel. It is the checker of tests/test_geoa3_step_cpu.py (which ties it to
oracle.ref_torch.GeoA3Oracle.forward_step + torch.optim.Adam in float64) and of tests/test_geoa3_step_gpu.py (which holds
ops.geoa3_update to it); the product never imports it.

Everything is channel-first, [B,3,N], on the CPU:

* record     the per-sample loop of :321-330 on the given prediction, the PREVIOUS iteration's constraint value and the
             iterate as it stands; both comparisons strict
* terms      dis (Chamfer two- / single-sided, or the L2 sum), hd (max, torch.max's first index), kappa_adv on the normal of
             the nearest ori point (clamp 1e-12, mean of |<v,n>| over idx[:, :, 1:]), curv, constrain, loss_n
* gradient   autograd of sum_b gval * scale_b * constrain_b on these formulas, + the victim's gradient g
* update     a real torch.optim.Adam on the offset (state injected), lr * 0.9990 with the scheduler, lp_clip, x = ori + offset

`inputs` builds the cases both test files use, `neighbours_f64` their float64 neighbours, cw_step_restatement.bands the
tolerance.
"""
import functools

import numpy as np
import torch

from cw_step_restatement import adam, bands, nn_f64  # noqa: F401  (bands: re-exported for the two test files)
from helpers import unit_cloud
from knn_step_restatement import knn_f64
from oracle import ref_torch as ort

BETAS, EPS, GAMMA = (0.9, 0.999), 1e-8, 0.9990
NCLS = 40
DEFAULTS = dict(cls_loss_type="CE", targeted=False, confidence=0., dis_loss_type="CD", two_sided=True, w_dis=1.0, w_hd=0.1,
                w_curv=1.0, scheduler=False, cc_linf=0., t=0, search_step=1)
TERM_OUT = ("dis", "hd", "curv", "constrain", "loss_n")
FLOAT_OUT = ("x", "offset", "m", "v", "g") + TERM_OUT          # held to the band
EXACT_OUT = ("best_loss", "iter_best_loss", "best_attack")     # copies of inputs: exact in fp32
INT_OUT = ("best_step", "best_bs", "iter_best_score", "hd_arg")

# (N, B, k): fewer points than two waves, several hundred, one past a multiple of 256, more points than threads
CASES = [(67, 3, 2), (200, 3, 16), (257, 1, 16), (1031, 1, 16)]


# ----------------------------------------------------------------------------------------------------------------------
# the terms
# ----------------------------------------------------------------------------------------------------------------------
def _rows(t, idx):
    """t [B,M,C] gathered at idx [B,N] -> [B,N,C]."""
    return torch.gather(t, 1, idx.long()[:, :, None].expand(-1, -1, t.shape[2]))


def kappa(x, normal, knn_idx):
    """loss_utils.py:63-70 / :83-90 on given neighbour lists (self first, dropped): [B,N]. Also returns |<v,n>| [B,N,k]."""
    a = x.transpose(1, 2)
    B, N, _ = a.shape
    k = knn_idx.shape[2] - 1
    nb = _rows(a, knn_idx.long()[:, :, 1:].reshape(B, N * k)).view(B, N, k, 3)
    vec = nb - a[:, :, None, :]
    vec = vec / vec.norm(2, 3, keepdim=True).clamp(min=1e-12)
    inner = torch.abs((vec * normal.transpose(1, 2)[:, :, None, :]).sum(3))
    return inner.mean(2), inner


def terms(x, ori, normal_ori, kappa_ori, nn_ao, nn_oa, knn_idx, c):
    """dict(dis, hd, hd_arg, curv, constrain, d_ao, inner) per sample, :139-181."""
    a, o = x.transpose(1, 2), ori.transpose(1, 2)
    B = x.shape[0]
    zero = torch.zeros(B, dtype=x.dtype)
    d_ao = inner = None
    if nn_ao is not None:
        d_ao = ((a - _rows(o, nn_ao)) ** 2).sum(2)
    if c["dis_loss_type"] == "CD":
        dis = d_ao.mean(1)
        if c["two_sided"]:
            dis = dis + ((o - _rows(a, nn_oa)) ** 2).sum(2).mean(1)
    else:
        dis = ((x - ori) ** 2).sum(1).sum(1)
    constrain = c["w_dis"] * dis
    hd, hd_arg = zero, torch.zeros(B, dtype=torch.int64)
    if c["dis_loss_type"] == "CD":
        hd, hd_arg = d_ao.max(1)
        if c["w_hd"] != 0:
            constrain = constrain + c["w_hd"] * hd
    curv = zero
    if c["w_curv"] != 0 and knn_idx is not None:
        nrm = _rows(normal_ori.transpose(1, 2), nn_ao).transpose(1, 2)
        ka, inner = kappa(x, nrm, knn_idx)
        curv = ((ka - torch.gather(kappa_ori, 1, nn_ao.long())) ** 2).mean(1)
        constrain = constrain + c["w_curv"] * curv
    return dict(dis=dis, hd=hd, hd_arg=hd_arg, curv=curv, constrain=constrain, d_ao=d_ao, inner=inner)


def cls_loss(logp, target, c):
    """:123-134 on the victim's OUTPUT, the log-probabilities."""
    if c["cls_loss_type"] == "Margin":
        oh = torch.zeros(target.size() + (logp.shape[1],), dtype=logp.dtype).scatter_(1, target.unsqueeze(1), 1.)
        fake = (oh * logp).sum(1)
        other = ((1. - oh) * logp - oh * 10000.).max(1)[0]
        return torch.clamp((other - fake if c["targeted"] else fake - other) + c["confidence"], min=0.)
    ce = torch.nn.CrossEntropyLoss(reduction="none")(logp, target.long())
    return ce if c["targeted"] else -ce


def lp_clip(offset, cc_linf):
    """:92-102."""
    lengths = (offset ** 2).sum(1, keepdim=True).sqrt().expand_as(offset)
    scaled = torch.where(lengths > 1e-6, offset / lengths * cc_linf, torch.zeros_like(offset))
    return torch.where(lengths < cc_linf, offset, scaled)


def record(pred, target, targeted, metric, x, step, search_step, st):
    """:321-330 per sample on numpy copies of the state; returns the new state."""
    st = {k: v.clone() for k, v in st.items()}
    for e in range(len(pred)):
        ok = (pred[e] == target[e]) if targeted else (pred[e] != target[e])
        if ok and metric[e] < st["best_loss"][e]:
            st["best_loss"][e], st["best_step"][e], st["best_bs"][e] = metric[e], step, search_step
            st["best_attack"][e] = x[e]
        if ok and metric[e] < st["iter_best_loss"][e]:
            st["iter_best_loss"][e], st["iter_best_score"][e] = metric[e], pred[e]
    return st


# ----------------------------------------------------------------------------------------------------------------------
# one iteration
# ----------------------------------------------------------------------------------------------------------------------
def step(dtype, inp, nbrs, **over):
    """One whole update of a case of inputs() on the neighbours nbrs = dict(nn_ao, nn_oa, knn_idx). `over` replaces single
    inputs or entries of DEFAULTS. Returns every tensor the kernel writes plus "lr" (a Python float), "pred", "d_ao", "inner"."""
    c = dict(DEFAULTS)
    c.update({k: over.pop(k) for k in list(over) if k in DEFAULTS})
    a = {k: over.get(k, v) for k, v in inp.items()}
    f = lambda t: t.detach().to(dtype)      # noqa: E731
    B = a["x"].shape[0]
    gval = a["gval"]
    logp = torch.log_softmax(f(a["logits"]), dim=1)
    pred = torch.argmax(a["logits"], dim=1)
    st = record(pred, a["target"], c["targeted"], f(a["constrain"]), f(a["x"]), c["t"], c["search_step"],
                dict(best_loss=f(a["best_loss"]), iter_best_loss=f(a["iter_best_loss"]), best_attack=f(a["best_attack"]),
                     best_step=a["best_step"], best_bs=a["best_bs"], iter_best_score=a["iter_best_score"]))
    knn_idx = nbrs.get("knn_idx") if c["w_curv"] != 0 else None
    need_ao = c["dis_loss_type"] == "CD" or knn_idx is not None
    two = c["two_sided"] and c["dis_loss_type"] == "CD" and nbrs.get("nn_oa") is not None
    x = f(a["x"]).clone().requires_grad_()
    tm = terms(x, f(a["ori"]), f(a["normal"]), f(a["kappa_ori"]), nbrs["nn_ao"] if need_ao else None,
               nbrs["nn_oa"] if two else None, knn_idx, dict(c, two_sided=two))
    scale = f(a["scale"])
    (gval * scale * tm["constrain"]).sum().backward()
    g = f(a["g"]) + x.grad
    loss_n = cls_loss(logp, a["target"], c) + scale * tm["constrain"].detach()
    off, m, v = adam(f(a["offset"]), g, f(a["m"]), f(a["v"]), c["t"] + 1, a["lr"], BETAS, EPS)
    if c["cc_linf"] != 0:
        off = lp_clip(off, c["cc_linf"])
    out = dict(st)
    out.update(x=f(a["ori"]) + off, offset=off, m=m, v=v, g=g, loss_n=loss_n, pred=pred,
               lr=a["lr"] * GAMMA if c["scheduler"] else a["lr"],
               **{k: tm[k].detach() for k in ("dis", "hd", "curv", "constrain", "hd_arg")},
               d_ao=None if tm["d_ao"] is None else tm["d_ao"].detach(), inner=None if tm["inner"] is None else tm["inner"].detach())
    return out


def run(dtype, case, **over):
    return step(dtype, inputs(*case), neighbours_f64(*case), **over)


# ----------------------------------------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(N, B, k):
    """The case both test files run at (N, B, k), fp32, never modified by its users. ori: helpers.unit_cloud clouds (rng seed
    = the case's position + 1); x = ori + offset with offsets N(0, s_b), s_b from 1e-3 to 1e-2 over the batch; normals by the
    oracle's estimate_normal(k = 3), kappa_ori by its _kappa on float64 neighbours; a small random "victim" gradient and Adam
    state; random logits; and a record state in which sample 0 improves both bests, sample 1 only the step's best, and sample
    2 fails (its label is its prediction)."""
    seed = {c[0]: i + 1 for i, c in enumerate(CASES)}.get(N, 5 + N)
    rng = np.random.default_rng(seed)
    g = torch.Generator().manual_seed(1000 + seed)
    ori = torch.from_numpy(np.stack([unit_cloud(rng, N) for _ in range(B)])).transpose(1, 2).contiguous()
    sig = torch.tensor([1e-3 * 10. ** (b / max(B - 1, 1)) for b in range(B)])
    offset = torch.randn(B, 3, N, generator=g) * sig[:, None, None]
    orc = ort.GeoA3Oracle(as_written=False, dtype=torch.float64, direct=True)
    normal = orc.estimate_normal(ori, 3).contiguous()
    # utility.py:73-75 multiplies by -sign(<n, sum>), and torch.sign(0) = 0: a point whose centred neighbours sum to exactly 0
    # gets the zero normal, whose inner products are exactly 0 in every precision. Such points get the z axis here, so that
    # every inner product of the cases is a decision with a margin (tests/test_geoa3_step_cpu.py checks it)
    dead = (normal.abs().sum(1, keepdim=True) == 0).expand_as(normal)
    normal = torch.where(dead, torch.tensor([0., 0., 1.])[None, :, None].expand_as(normal), normal).contiguous()
    kappa_ori = orc._kappa(ori, normal, k).float().contiguous()
    logits = torch.randn(B, NCLS, generator=g)
    pred = logits.argmax(1)
    sel = torch.arange(B)
    target = torch.where(sel % 3 == 2, pred, (pred + 1) % NCLS)
    constrain = torch.rand(B, generator=g) + 0.5
    return dict(ori=ori, offset=offset, x=ori + offset, normal=normal, kappa_ori=kappa_ori, logits=logits, target=target,
                g=torch.randn(B, 3, N, generator=g) * 1e-3, m=torch.randn(B, 3, N, generator=g) * 1e-3,
                v=torch.rand(B, 3, N, generator=g) * 1e-6, scale=torch.tensor([10., 20., 5.])[sel % 3].contiguous(),
                constrain=constrain, best_loss=torch.where(sel % 3 == 1, constrain * 0.5, constrain * 2).contiguous(),
                iter_best_loss=(constrain * 2).contiguous(), best_attack=torch.ones(B, 3, N),
                best_step=torch.full((B,), -1), best_bs=torch.full((B,), -1), iter_best_score=torch.full((B,), -1),
                lr=0.01, gval=float(np.float32(1.0) / np.float32(B)))


@functools.lru_cache(maxsize=None)
def neighbours_f64(N, B, k):
    """dict(nn_ao, nn_oa [B,N] int32, knn_idx [B,N,k+1] int32) of a case of inputs() on float64 direct differences."""
    inp = inputs(N, B, k)
    return dict(nn_ao=nn_f64(inp["x"], inp["ori"]), nn_oa=nn_f64(inp["ori"], inp["x"]), knn_idx=knn_f64(inp["x"], k)[1])
