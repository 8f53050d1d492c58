"""TEST INFRASTRUCTURE: one iteration's update of the kNN attack in plain torch, for any dtype, written from the reference's
own statements (attack/KNN/KNN_attack.py:117-136, attack/CW/CW_utils/dist_utils.py:125-160 and 189-223, clip_utils.py:67-136
as oracle.ref_torch has them) and not from the kernel. It is the checker of tests/test_knn_step_cpu.py (which ties it to
oracle.ref_torch.knn_attack bit for bit) and of tests/test_knn_step_gpu.py (which holds ops.knn_attack_update to it in
float64); the product never imports it.

Everything is channel-first, [B,3,N], on the CPU, as the reference's loop has it:

* distance   dist_func(adv^T, ori^T).mean() * N with dist_func = ChamferkNNDist(adv2ori) (w2 given) or ChamferDist(adv2ori)
             (w2 None), differentiated by autograd. Two spellings of the neighbour terms: "matrix" — through the [B,N,N]
             matrices, topk and min, as the reference writes them — and "gather" — on given knn_idx [B,N,k+1] (self first) and
             nn_idx [B,N]. The outlier mask is a constant of the graph (torch.no_grad, dist_utils.py:145-151).
* gradient   g_model + that
* Adam       a real torch.optim.Adam whose state (step = t-1, exp_avg = m, exp_avg_sq = v) is injected
* clip       ProjectInnerClipLinf(budget)(p, ori, normal) or ClipPointsLinf(budget)(p, ori)

`mut` names ONE deliberate mistake (tests/test_knn_step_cpu.py shows that each leaves the band). `inputs` builds the cases
both test files use, `knn_f64` / cw_step_restatement.nn_f64 the float64 neighbours, cw_step_restatement.bands the tolerance.
"""
import functools

import torch

from cw_step_restatement import adam, bands, nn_f64  # noqa: F401  (bands / nn_f64: re-exported for the two test files)
from oracle import ref_torch as ort

LR, BUDGET, BETAS, EPS, T = 0.01, 0.18, (0.9, 0.999), 1e-8, 5
K_NN, ALPHA, W1, W2 = 5, 1.05, 5., 3.
FLOAT_OUT = ("adv", "m", "v")
MUTATIONS = ("biased_std", "ge_mask", "no_scatter", "no_times_K", "weights_swapped", "no_projection", "clip_first")


# ----------------------------------------------------------------------------------------------------------------------
# the two distance terms, per sample, on [B,N,3] tensors as the functors receive them
# ----------------------------------------------------------------------------------------------------------------------
def knn_values(pc, k, knn_idx=None, scatter=True):
    """value [B,N] = mean squared distance to the k nearest other points (dist_utils.py:133-143). knn_idx None: the
    reference's expansion matrix and topk; else on the given neighbours, columns 1..k (scatter=False: no gradient to them)."""
    if knn_idx is None:
        pc = pc.transpose(2, 1)
        inner = -2. * torch.matmul(pc.transpose(2, 1), pc)
        xx = torch.sum(pc ** 2, dim=1, keepdim=True)
        dist = xx + inner + xx.transpose(2, 1)
        neg_value, _ = (-dist).topk(k=k + 1, dim=-1)
        return torch.mean(-(neg_value[..., 1:]), dim=-1)
    B, N, _ = pc.shape
    idx = knn_idx.long()[:, :, 1:k + 1].reshape(B, N * k, 1).expand(-1, -1, 3)
    nb = torch.gather(pc if scatter else pc.detach(), 1, idx).view(B, N, k, 3)
    return torch.mean(torch.sum((pc[:, :, None, :] - nb) ** 2, dim=3), dim=2)


def knn_mask(value, alpha, mut=None):
    """(mask [B,N] bool, threshold [B]): dist_utils.py:145-151, torch.std's default (unbiased), strict >."""
    with torch.no_grad():
        thr = torch.mean(value, dim=-1) + alpha * torch.std(value, dim=-1, unbiased=mut != "biased_std")
        return (value >= thr[:, None]) if mut == "ge_mask" else (value > thr[:, None]), thr


def knn_term(pc, k, alpha, knn_idx=None, mut=None):
    value = knn_values(pc, k, knn_idx, scatter=mut != "no_scatter")
    mask, _ = knn_mask(value, alpha, mut)
    return torch.mean(value * mask.to(value.dtype), dim=1)


def chamfer_term(adv, ori, nn_idx=None):
    """adv2ori [B]: distance.py:40-50 through the reference's expansion matrix, or on the given arg-mins."""
    if nn_idx is None:
        return torch.mean(torch.min(ort.batch_pairwise_dist(ori, adv), 1)[0], dim=1)
    q = torch.gather(ori, 1, nn_idx.long()[:, :, None].expand(-1, -1, 3))
    return torch.mean(torch.sum((adv - q) ** 2, dim=2), dim=1)


def dist_loss(adv, ori, k, alpha, w1, w2, knn_idx=None, nn_idx=None, mut=None):
    """KNN_attack.py:119-123 for channel-first adv / ori: dist_func(adv^T, ori^T).mean() * N."""
    a, o = adv.transpose(1, 2).contiguous(), ori.transpose(1, 2).contiguous()
    ones = torch.ones((a.shape[0],), dtype=torch.float32)          # ref_torch._w: the functors' default weights
    cd = (chamfer_term(a, o, nn_idx) * ones).mean()
    if w2 is None:
        loss = cd
    else:
        kd = (knn_term(a, k, alpha, knn_idx, mut) * ones).mean()
        loss = cd * w2 + kd * w1 if mut == "weights_swapped" else cd * w1 + kd * w2
    return loss.mean() if mut == "no_times_K" else loss.mean() * adv.shape[2]


def dist_grad(dtype, adv, ori, k, alpha, w1, w2, knn_idx=None, nn_idx=None, mut=None):
    a = adv.detach().to(dtype).clone().requires_grad_()
    dist_loss(a, ori.to(dtype), k, alpha, w1, w2, knn_idx, nn_idx, mut).backward()
    return a.grad


def clip(p, ori, normal, budget, project, mut=None):
    p = p.clone().detach()
    if not project or mut == "no_projection":
        return ort.ClipPointsLinf(budget)(p, ori)
    if mut == "clip_first":
        return ort.ProjectInnerPoints()(ort.ClipPointsLinf(budget)(p, ori), ori, normal)
    return ort.ProjectInnerClipLinf(budget)(p, ori, normal)


def step(dtype, adv, ori, normal, g_model, m, v, t, lr=LR, budget=BUDGET, k=K_NN, alpha=ALPHA, w1=W1, w2=W2, project=True,
         knn_idx=None, nn_idx=None, mut=None, betas=BETAS, eps=EPS):
    """One iteration's update. normal None: the positions double as normals (KNN_attack.py:68-73). knn_idx / nn_idx None:
    the "matrix" spelling, else "gather". Returns dict(adv, m, v, stepped, g_dist): `stepped` is the iterate before the clip."""
    adv, ori, g_model, m, v = (x.detach().to(dtype) for x in (adv, ori, g_model, m, v))
    normal = ori if normal is None else normal.detach().to(dtype)
    g_dist = dist_grad(dtype, adv, ori, k, alpha, w1, w2, knn_idx, nn_idx, mut)
    q, m, v = adam(adv, g_model + g_dist, m, v, t, lr, betas, eps)
    return dict(adv=clip(q, ori, normal, budget, project, mut), m=m, v=v, stepped=q, g_dist=g_dist)


# ----------------------------------------------------------------------------------------------------------------------
# float64 neighbours and the inputs
# ----------------------------------------------------------------------------------------------------------------------
def knn_f64(pts, k, chunk=256):
    """(d float64 [B,N,k+1] ascending, idx int32 [B,N,k+1]) of the self-kNN of pts [B,3,N] on float64 direct differences,
    the point itself first, in row chunks (no [B,N,N] matrix)."""
    x = pts.double()
    ds, ids = [], []
    for i in range(0, x.shape[2], chunk):
        d = sum((x[:, c, i:i + chunk, None] - x[:, c, None, :]) ** 2 for c in range(3))
        rows = torch.arange(i, min(i + chunk, x.shape[2]))
        d[:, rows - i, rows] = -1.                                  # the point itself sorts first whatever else is at 0
        dv, di = (-d).topk(k + 1, dim=-1)
        dv = -dv
        dv[:, :, 0] = 0.
        ds.append(dv), ids.append(di)
    return torch.cat(ds, 1), torch.cat(ids, 1).to(torch.int32)


def mask_margin(adv, k, alpha):
    """(value, thr, mask, rel) in float64 on direct differences: rel [B,N] = |value - thr| / thr."""
    d, _ = knn_f64(adv, k)
    value = d[:, :, 1:].mean(-1)
    mask, thr = knn_mask(value, alpha)
    return value, thr, mask, (value - thr[:, None]).abs() / thr[:, None]


N_PLANT = 2          # far points per cloud (masked by construction); one in a cloud of fewer than 16 points
MARGIN = 1e-4        # every point's |value - thr| exceeds MARGIN * thr in float64: the fp32 mask cannot legitimately differ


@functools.lru_cache(maxsize=None)
def inputs(N, B=3, k=K_NN, with_normal=True, alpha=ALPHA):
    """The case both test files run at N points (fp32, [B,3,N]); never modified by its users. ori uniform in [-0.5, 0.5], adv
    = ori + 0.1 randn (so the clip at BUDGET shortens some points and not others), small gradient and moments, and per cloud:
      * N_PLANT points of adv moved 1 and 1.5 outwards, away from the cloud: masked whatever the rest does;
      * the last point is an "opposite" point of the projection — the normal it is given has length 1e-6 and points against
        its offset, so that inner < 0 and |n x d| < 1e-6 by a factor 9 after any Adam step (with_normal False: its POSITION
        is that tiny vector, the positions being the normals then);
      * points closer than MARGIN to the outlier threshold are redrawn (bounded) until none is left.
    with_normal: random unit normals as a separate tensor, else None. alpha: the threshold's factor the margins are made for."""
    g = torch.Generator().manual_seed(7919 * N + 31 * B + k)
    ori = torch.rand(B, 3, N, generator=g) - 0.5
    u = torch.randn(B, 3, generator=g)
    u = u / u.norm(dim=1, keepdim=True)
    normal = None
    if with_normal:
        normal = torch.randn(B, 3, N, generator=g)
        normal = normal / normal.norm(dim=1, keepdim=True)
        normal[:, :, N - 1] = -1e-6 * u
    else:
        ori[:, :, N - 1] = -1e-6 * u
    adv = ori + torch.randn(B, 3, N, generator=g) * 0.1
    adv[:, :, N - 1] = ori[:, :, N - 1] + 0.1 * u
    for p in range(N_PLANT if N >= 16 else 1):
        adv[:, :, p] = ori[:, :, p] + (1.0 + 0.5 * p) * ori[:, :, p] / ori[:, :, p].norm(dim=1, keepdim=True)
    for _ in range(20):
        close = mask_margin(adv, k, alpha)[3] <= 2 * MARGIN
        if not close.any():
            break
        nudge = torch.randn(B, 3, N, generator=g) * 0.02
        adv = torch.where(close[:, None, :], adv + nudge, adv)
    return dict(adv=adv.contiguous(), ori=ori, normal=normal, g=torch.randn(B, 3, N, generator=g) * 1e-3,
                m=torch.randn(B, 3, N, generator=g) * 1e-3, v=torch.rand(B, 3, N, generator=g) * 1e-6)


def run(dtype, inp, t=T, **over):
    """step() on a case of inputs(); `over` replaces single inputs or keywords of step()."""
    names = ("adv", "ori", "normal", "g", "m", "v")
    a = {n: over.pop(n, inp[n]) for n in names}
    return step(dtype, a["adv"], a["ori"], a["normal"], a["g"], a["m"], a["v"], t, **over)


def lattice(n_side, B=1, spacing=1. / 16):
    """A cubic lattice of n_side^3 points, spacing a power of two: every point, the corners included, has at least three
    neighbours at exactly `spacing`, so for k <= 3 every value_i is spacing^2 exactly, the std is 0, thr = mean and the
    strict mask is empty."""
    ax = torch.arange(n_side, dtype=torch.float32) * spacing
    pts = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij")).reshape(3, -1)
    return pts[None].repeat(B, 1, 1).contiguous()


@functools.lru_cache(maxsize=None)
def lattice_case(B=2):
    """(inputs, k): adv is a 4 x 4 x 4 lattice, k = 3 — all value_i equal: `>` masks nothing, `>=` everything."""
    g = torch.Generator().manual_seed(3)
    adv = lattice(4, B=B)
    n = torch.randn(adv.shape, generator=g)
    return dict(adv=adv, ori=adv + 0.05 * torch.randn(adv.shape, generator=g), normal=n / n.norm(dim=1, keepdim=True),
                g=torch.randn(adv.shape, generator=g) * 1e-3, m=torch.randn(adv.shape, generator=g) * 1e-3,
                v=torch.rand(adv.shape, generator=g) * 1e-6), 3


# (N, B, k, with_normal) of the step cases both test files run: fewer points than a wave, the wave boundary, several points
# per thread, an odd count, and the cap of the update kernel (one cloud: its float64 neighbours cost the most)
CAP = 4096
CASES = [(N, B, k, wn) for N in (7, 64, 65, 200, 1024, 1031) for (B, k, wn) in ((3, 5, True), (1, 1, False))] + \
    [(200, 1, 5, False), (200, 3, 1, True), (CAP, 1, 5, True)]
# ... and with alpha = 0 (the threshold is the mean, which the far points raise: about a fifth of the points are masked), so that the masked list is long
# and the edges fill several staging trips of the kernel (2048 edges each)
HEAVY_ALPHA = 0.0
HEAVY = [(2049, 3, 5, True), (CAP, 1, 5, True)]


@functools.lru_cache(maxsize=None)
def neighbours_f64(N, B, k, with_normal, alpha=ALPHA):
    """(knn_idx, nn_idx) of a case of inputs() on float64 direct differences."""
    inp = inputs(N, B, k, with_normal, alpha)
    return knn_f64(inp["adv"], k)[1], nn_f64(inp["adv"], inp["ori"])
