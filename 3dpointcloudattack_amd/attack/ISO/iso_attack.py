"""The isometry attack (TSI + CTRI) — MI355X mirror of the reference's ``attack/ISO/iso_attack.py``.

A cloud is attacked by a 3x3 matrix W in front of the frozen victim, x' = W x:
  TSI   Thompson sampling over a grid of Euler-angle intervals draws rotations until one fools the victim
        (``thompson_sample_attack``); the draw with the smallest true-class probability is kept;
  CTRI  Adam on the 9 entries of W against a CW / cross-entropy loss until the prediction flips (``gradient_attack``).

The reference runs one cloud at a time with ``.item()`` / ``.cpu()`` in every step. ``ISOAttack`` runs a batch: TSI is
host-driven by necessity (the bandit needs a reward before its next draw) with one batched forward and one device-to-host
copy per round; CTRI is a device-side loop — the victim's fused passes plus ONE ``pc3d_iso_update_f32`` launch per step
(latch instead of `break`, record, weight gradient, Adam, next iterate), replayed from a hipGraph, no host round trip.

Kept on purpose: the softmax taken on the victim's log-probabilities; the spectral penalty that is
computed every step on ``W.data`` and therefore never reaches the gradient (LAMBDA does not influence the trajectory);
its fresh normal draw from torch's CPU generator on every call; the evaluation BEFORE the last update being the one a
cloud that never breaks reports. Not kept: import-time side effects (open3d, the terminal-size query, a ``device`` global).
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import graphed as _graphed
from ... import ops
from . import isometry_init  # noqa: F401  (reference-style drivers reach it through this module)
from . import thompson_sample as ts
from .thompson_sample import logits_info

POWER_ITERS = 30


def _penalty_with(W, v, iters=POWER_ITERS):
    """|v^T M v| after `iters` power iterations on M = W^T W - I from the start vector v (fp32, W's device)."""
    v = F.normalize(v, dim=0, eps=1e-12).to(W.device)
    matrix = torch.mm(W.t(), W) - torch.eye(3, device=W.device)
    penalty = torch.zeros((), device=W.device)
    for _ in range(iters):
        v = F.normalize(torch.matmul(matrix, v), dim=0, eps=1e-12)
        penalty = torch.dot(v, torch.matmul(matrix, v))
    return penalty.abs()


def spectral_penalty(W, iters=30):
    """Spectral norm of W^T W - I by power iteration (iso_attack.py:58-65). Draws its start vector from torch's CPU
    generator on EVERY call, as the reference does."""
    return _penalty_with(W, torch.empty(3).normal_(0, 1), iters)


def iso_penalty(W, p=2):
    """Schatten p-norm of M = W^T W - I in the reference's form (iso_attack.py:68-73)."""
    matrix = torch.mm(W.t(), W) - torch.eye(3, device=W.device)
    return (torch.mm(matrix.t(), matrix)).pow(p / 2.).trace().pow(1. / p).abs()


class ISOnet(nn.Module):
    """The victim behind a bias-free 3 -> 3 linear layer on the coordinates (iso_attack.py:89-101). `iso.weight` is
    [3,3], or [B,3,3] to give every sample of the batch its own matrix; the product runs in pc3d_iso_apply_f32."""

    def __init__(self, model):
        super(ISOnet, self).__init__()
        self.model = model
        for p in self.parameters():
            p.requires_grad = False
        self.iso = nn.Linear(3, 3, bias=False)

    def forward(self, x):
        W = self.iso.weight
        if W.dim() == 2:
            W = W.unsqueeze(0).expand(x.shape[0], 3, 3)
        return self.model(ops.IsoTransform.apply(x, W))


def _rates(out):
    return F.softmax(out, dim=1).sort(1, descending=True)


def _tsi(thompson, victim, x, label, clouds, num_init, tsi_batch):
    """TSI for the listed clouds of x [B,3,N], `tsi_batch` of them sharing each round. Per round and cloud still drawing,
    in cloud order: one posterior draw (get_action) and one rotation (three uniforms); then ONE batched forward, ONE
    device-to-host copy (flag and true-class probability per cloud) and the posterior updates in cloud order.
    Returns {cloud: (float64 matrix with the smallest true-class probability, number of draws, last drawn matrix)}."""
    env = thompson.environment
    res = {}
    for g0 in range(0, len(clouds), tsi_batch):
        group = list(clouds[g0:g0 + tsi_batch])
        mats, probs = {b: [] for b in group}, {b: [] for b in group}
        active = group
        for _ in range(num_init):
            if not active:
                break
            arms = []
            for b in active:
                arm = thompson.get_action()
                mats[b].append(isometry_init.rotation_xyz(*env.arm_to_interval(arm)))
                arms.append(arm)
            W = torch.as_tensor(np.stack([mats[b][-1] for b in active]), dtype=torch.float32).to(x.device)
            sel = x[active[0]:active[0] + 1] if len(active) == 1 else x[torch.as_tensor(active, device=x.device)]
            lab = label[torch.as_tensor(active, device=x.device)]
            with torch.no_grad():
                rates, indices = _rates(victim(ops.iso_apply(sel, W))[0])
                tp = (rates * (indices == lab[:, None])).sum(1)
                host = torch.stack([(indices[:, 0] == lab).float(), tp], 1).cpu()
            still = []
            for j, b in enumerate(active):
                reward = env.reward_of(int(host[j, 0]))
                thompson._update_params(arms[j], reward)
                probs[b].append(float(host[j, 1]))
                if reward != 1:
                    still.append(b)
            active = still
        for b in group:
            res[b] = (mats[b][int(np.argmin(probs[b]))], len(probs[b]), mats[b][-1])
    return res


def thompson_sample_attack(thompson, obj, label, model, num_init=1):
    """TSI on one cloud obj [1,3,N] behind `model` (an ISOnet): (the drawn matrix with the smallest true-class
    probability as a float32 tensor, thompson). At most num_init rounds, stops at the first reward 1 (iso_attack.py:104-118).
    `model.iso.weight` is left at the last drawn matrix, as in the reference."""
    chosen, _, last = _tsi(thompson, model.model, obj.detach().float(), label.reshape(-1), [0], num_init, 1)[0]
    model.iso.weight.data = torch.as_tensor(last, dtype=torch.float32).to(obj.device)
    return torch.as_tensor(chosen, dtype=torch.float32).to(obj.device), thompson


class _Ctri(_graphed.DeviceLoop):
    """The CTRI loop on B clouds: static buffers, one step as the body, captured (fast path) as one step. Clouds that take
    no part (not attacked, or already fooled by TSI) are latched as done before the first step: their W, steps and kept_*
    never change, and the loop's shape — hence its captured graph — depends on the batch alone."""

    def __init__(self, victim, B, N, dev, fast, kind, kappa, lr, key=None):
        # the graph bakes in the addresses of the folded weights: it holds what it points at (LoopGraph.keep)
        super().__init__(key, dev, owners=(victim,), counts=(1,), warmup=2)
        self.victim, self.fast, self.kind, self.kappa, self.lr = victim, fast, kind, float(kappa), float(lr)
        f32 = dict(dtype=torch.float32, device=dev)
        b = self.bufs
        b["x"], b["xo"] = torch.zeros((B, 3, N), **f32), torch.zeros((B, 3, N), **f32)
        b["W"], b["m"], b["v"] = (torch.zeros((B, 3, 3), **f32) for _ in range(3))
        b["label"] = torch.zeros((B,), dtype=torch.int64, device=dev)
        b["kept_pred"] = torch.zeros((B,), dtype=torch.int64, device=dev)
        b["done"] = torch.zeros((B,), dtype=torch.int32, device=dev)
        b["steps"] = torch.zeros((B,), dtype=torch.int32, device=dev)
        b["kept_out"] = None                   # [B, ncls], allocated by the first step from the victim's output

    def load(self, x, label, W, active=None):
        """active: bool [B], the clouds that run (default: all)."""
        b = self.bufs
        b["x"].copy_(x), b["label"].copy_(label), b["W"].copy_(W.reshape(-1, 3, 3))
        for t in (b["m"], b["v"], b["steps"], b["kept_out"], b["kept_pred"]):
            if t is not None:
                t.zero_()
        if active is None:
            b["done"].zero_()
        else:
            b["done"].copy_((~active).to(torch.int32))
        ops.iso_apply(b["x"], b["W"], out=b["xo"])

    def _update(self, pred, row, **grad):
        b = self.bufs
        if b["kept_out"] is None:
            b["kept_out"] = torch.zeros_like(row)
        ops.iso_update(b["x"], b["xo"], b["W"], b["m"], b["v"], pred, b["label"], row, b["done"], b["steps"],
                       b["kept_out"], b["kept_pred"], self.lr, **grad)

    def step(self):
        b = self.bufs
        if self.fast:     # the victim's fused passes (no autograd) + ONE launch for everything else
            logp, pred, _, gx = self.victim.fused_loss_and_grad(b["xo"], b["label"], self.kind, self.kappa, scale=1.0)
            self._update(pred, logp, g=gx)
            return
        # any victim: autograd through IsoTransform. The loss is taken on what the victim returns: the margin on the
        # output as given (kind + 4); the cross-entropy applies its own log-softmax to it, as F.cross_entropy does
        Wp = b["W"].detach().requires_grad_()
        with torch.enable_grad():
            out = self.victim(ops.IsoTransform.apply(b["x"], Wp))[0]
        _, pred, _, g_out = ops.cls_loss(out.detach(), b["label"], self.kind + 4 if self.kind == 0 else self.kind, self.kappa,
                                         scale=1.0)
        (gW,) = torch.autograd.grad(out, Wp, g_out)
        self._update(pred, out.detach().contiguous(), gW=gW.contiguous())

    body = step


_MAX_CTRI_CACHE = 4


def _ctri_loop(victim, x, label, W, active, target, kappa, step_size, fused=True, graph=True, cache=None):
    """A loaded _Ctri for x [B,3,N] from the matrices W [B,3,3], ready to run(). cache: a graphed.LoopCache (or any
    dict) that keeps captured loops per (shape, settings, weights); None: nothing is captured."""
    B, _, N = x.shape
    fast = bool(fused and hasattr(victim, "fused_loss_and_grad"))
    kind = 0 if target != 0 else 3          # pc3d_cls_loss_f32: the CW margin (+ kappa), or minus the cross-entropy
    cached = fast and graph and cache is not None
    key = _graphed.loop_key(victim, x.device, B, N, kind, float(kappa), float(step_size)) if cached else None
    c = cache.get(key) if cached else None
    if c is None:
        c = _Ctri(victim, B, N, x.device, fast, kind, kappa, step_size, key)
        if cached:
            cache[key] = c
            c.load(x, label, W, active)
            c.capture()
    c.load(x, label, W, active)
    return c


def _penalties(W, steps):
    """Host, cloud order: cloud b draws steps[b] start vectors from torch's CPU generator, as one spectral_penalty call
    per step does in the reference, and the last one gives its penalty on W[b] (fp32, the reference's formula). Leaves
    the generator where the reference's function calls leave it after attacking the clouds one by one."""
    out = []
    for Wb, n in zip(W.cpu(), steps.tolist()):
        v = None
        for _ in range(n):
            v = torch.empty(3).normal_(0, 1)
        out.append(float(_penalty_with(Wb, v)) if v is not None else 0.0)
    return out


class ISOAttack:
    """Batched TSI + CTRI. ``attack(pc [B,3,N], label [B])`` returns (adversarial clouds [B,3,N], matrices [B,3,3], info):
    info holds, per cloud, the columns the reference logs — attacked, init_success, correct, true_prob_before,
    true_prob_after, pred_after, pred_prob_after (probabilities as fractions, not per cent), penalty, steps — and
    tsi_draws, tsi_W (the matrices TSI handed on). The Thompson posterior (`self.thompson`) persists across calls, as it
    does across the objects of a reference run.

    tsi_batch: clouds that draw from the shared posterior per TSI round; 1 is the reference's order exactly for any B
    (numpy's global generator and the posterior end where the reference leaves them), larger values trade that for fewer,
    wider forwards. fused: use the victim's fused_loss_and_grad when it has one (PointNet); otherwise, and for any other
    victim, autograd through ops.IsoTransform. graph: replay the fused step from a hipGraph, captured once per batch
    shape. The loop runs on all B clouds, those that take no part latched as done from the start, and the per-cloud stop
    is the same latch, so it always runs num_steps steps. LAMBDA is accepted and, as in the reference, has no effect."""

    def __init__(self, model, num_steps=50, step_size=5e-4, LAMBDA=1000, target=1, kappa=0, num_init=50, d=4, a=-np.pi,
                 b=np.pi, attack_type='combine', thompson=None, tsi_batch=1, fused=True, graph=True):
        if num_steps < 1 or tsi_batch < 1:
            raise ValueError("ISOAttack: num_steps and tsi_batch must be >= 1")
        self.model = model.eval()
        self.num_steps, self.step_size, self.LAMBDA, self.target, self.kappa = num_steps, step_size, LAMBDA, target, kappa
        self.num_init, self.attack_type, self.tsi_batch, self.fused, self.graph = num_init, attack_type, tsi_batch, fused, graph
        self.thompson = thompson if thompson is not None else ts.BernThompson(ts.environment(d=d, a0=a, b0=b))
        self._ctri_cache = _graphed.LoopCache(_MAX_CTRI_CACHE)

    def attack(self, pc, label):
        with torch.cuda.device(pc.device):
            return self._attack(pc, label)

    def _attack(self, pc, label):
        x = pc.detach().float().contiguous()
        label = label.detach().reshape(-1).long().to(x.device)
        B, dev = x.shape[0], x.device
        with torch.no_grad():
            rates, indices = _rates(self.model(x)[0])
        attacked_t = indices[:, 0] == label
        true_before = (rates * (indices == label[:, None])).sum(1)
        attacked = attacked_t.cpu().numpy()
        clouds = [int(b) for b in np.nonzero(attacked)[0]]        # misclassified clouds are not attacked (iso_attack.py:385)

        tsi = _tsi(self.thompson, self.model, x, label, clouds, self.num_init, self.tsi_batch)
        W64 = np.tile(np.eye(3), (B, 1, 1))
        draws = np.zeros(B, dtype=np.int64)
        for b, (mat, n, _) in tsi.items():
            W64[b], draws[b] = mat, n
        tsi_W = torch.as_tensor(W64, dtype=torch.float32)          # the float32 values the reference hands on
        W = tsi_W.to(dev, copy=True)
        with torch.no_grad():                                      # the re-evaluation with the chosen matrix (:394)
            rates, indices = _rates(self.model(ops.iso_apply(x, W))[0])
        pred_after, pred_prob = indices[:, 0].clone(), rates[:, 0].clone()
        true_after = (rates * (indices == label[:, None])).sum(1)
        correct_t = (pred_after == label) & attacked_t
        still_np = correct_t.cpu().numpy()
        init_success = attacked & ~still_np
        steps = np.zeros(B, dtype=np.int64)
        penalty = np.zeros(B)

        if still_np.any() and self.attack_type == 'combine':
            run = correct_t.clone()                                # the clouds TSI left correct
            c = _ctri_loop(self.model, x, label, W, run, self.target, self.kappa, self.step_size, self.fused, self.graph,
                           self._ctri_cache)
            c.run(self.num_steps)
            r, i = _rates(c.kept_out)                              # the evaluation each cloud reports (see pc3d_iso_update_f32)
            W = c.W.clone()
            pred_after, pred_prob = torch.where(run, c.kept_pred, pred_after), torch.where(run, r[:, 0], pred_prob)
            true_after = torch.where(run, (r * (i == label[:, None])).sum(1), true_after)
            correct_t = torch.where(run, c.kept_pred == label, correct_t)
            st = c.steps.cpu()
            steps = st.numpy().astype(np.int64)
            failed = correct_t.cpu().numpy()
            penalty = np.where(failed, 0.0, np.array(_penalties(W, st)))   # a failed CTRI reports penalty 0 (:402-403)
        adv = ops.iso_apply(x, W)
        info = dict(attacked=torch.as_tensor(attacked), init_success=torch.as_tensor(init_success),
                    correct=correct_t.cpu().long(), true_prob_before=true_before.cpu(), true_prob_after=true_after.cpu(),
                    pred_after=pred_after.cpu(), pred_prob_after=pred_prob.cpu(), penalty=torch.as_tensor(penalty),
                    steps=torch.as_tensor(steps), tsi_draws=torch.as_tensor(draws), tsi_W=tsi_W)
        return adv, W, info


def gradient_attack(obj, label, model, args):
    """CTRI on one cloud obj [1,3,N] behind `model` (an ISOnet), from its current `iso.weight`; args carries step_size,
    num_steps, target, kappa (and LAMBDA, without effect). Returns (correct, rates, indices, model, penalty, steps) as
    iso_attack.py:121-159: the values of the breaking evaluation, or of the evaluation before the last update; the model
    keeps the final matrix. `penalty` is the last spectral_penalty call's: at the break on the final matrix, and for a
    cloud that never breaks on the matrix BEFORE the last update (the reference calls it ahead of optimizer.step())."""
    model.eval()
    x, lab = obj.detach().float().contiguous(), label.reshape(-1).long()
    with torch.cuda.device(x.device), torch.no_grad():
        c = _ctri_loop(model.model, x, lab, model.iso.weight.data.reshape(1, 3, 3), None, args.target, args.kappa,
                       args.step_size, graph=False)
        c.run(args.num_steps - 1)
        W_pen = c.W.clone()              # a cloud that broke earlier keeps this matrix; one that never breaks was last
        c.run(1)                         # penalised on it, before the final update
    model.iso.weight.data = c.W[0].clone()
    rates, indices = _rates(c.kept_out)
    steps = c.steps.cpu()
    return (int((c.kept_pred[0] == lab[0]).item()), rates[0], indices[0], model, _penalties(W_pen, steps)[0], int(steps[0]))
