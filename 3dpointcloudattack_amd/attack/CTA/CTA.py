"""The critical-point attack — MI355X mirror of the reference's ``attack/CTA/CTA.py`` (and, through ``variant='sumloss'``,
of ``CTA_sumloss.py``).

The reference ranks the points of a set of clouds by integrated gradients, then runs an optimiser that may move only the
top-ranked points, one more level of them whenever a pass of 25-step windows stops improving, until the victim's
prediction for the first cloud changes. It does so one set at a time, from Python, with one forward and one backward per
step and five or more device-to-host copies in each. Here ``cta_attack`` advances G sets together and stays on the device:

  saliency   ``pc3d_ig_steps_f32`` writes all steps x S interpolated clouds of a set, the victim runs on them in one batch
             (fused passes for a PointNet, autograd otherwise), ``pc3d_ig_cotangent_f32`` forms the cotangent and
             ``pc3d_ig_reduce_f64`` the float64 mask and both contribution tables;
  ranking    on the host: ``np.argsort(kind='quicksort')`` of the float64 contributions, copied back once — the order of
             exact ties is numpy's — turned into a selection table sel[G,P,W] of (sample, point) slots per level;
  loop       per step the victim's forward, ``pc3d_cta_cotangent_f32`` (loss cotangent, records, windows, success flag),
             the victim's backward and ``pc3d_cta_update_f32`` (mask, Adam / Momentum, counters, latch). For a PointNet
             victim without the Chamfer penalty 25 steps are one hipGraph replay; the host then reads the windows and
             latches in one copy, takes ``np.mean`` as the reference does, decides per set and writes control words.

What the reference does is kept as written, not as commented: the saliency differentiates the
log-softmax output with a cotangent in rows j < 2 only; a falsy class (0, None) selects the multi-hot of every row's
top-1; CTA.py's ranking is over [3,B] (it sums the mask over the points) and unmasks points ``contr_index[pa][:]`` of
sample 0 for pa <= 2; CTA_sumloss.py's is over [B,N]; Adam has no bias correction, its epsilon inside the root and step
size 1; the optimiser state survives a level change, the iterate does not; the original class's logit is negated, not
excluded, in ``max_other_logits``. Departures: ``cta_attack`` reports 'Exhausted' where ``act_max`` returns None (the
reference falls off its end); the prints are not kept.
"""
import random

import numpy as np
import torch

from ... import graphed as _graphed
from ... import ops
from ...model import pointnet as _pointnet
from .utils import dis_utils_torch
from .utils.integrated_gradients import IntegratedGradients

stop_threshold = 5e-1
noise_weight = 1e-2

WINDOW = 25              # steps per stop window, and per graph replay
PASS_MAX = 1500          # a pass breaks at cur_step >= 1500
TOTAL_MAX = 15000        # 'Fail' once a pass ends with step >= 15000
IG_SET_SIZE = 2          # VanillaGradient.get_mask's default, which IntegratedGradients never overrides
MAX_ROWS = 4096          # clouds per victim pass of the saliency: a chunk size chosen for memory, not a limit of the kernels
_LOOPS = _graphed.LoopCache(4)
_P_LATCH, _P_CUR, _P_STEP, _P_NPP = 50, 51, 52, 53


def get_IG(input_tensor, ori_cls, network, IG_steps=25, baseline='black'):
    """The float64 [3,N,B] integrated-gradients mask of one set [B,3,N] for class ori_cls (CTA.py:30-33)."""
    return IntegratedGradients(network.eval()).get_mask(input_tensor, ori_cls, baseline, IG_steps)


def layer_hook(act_dict, layer_name):
    """A forward hook that keeps its layer's latest output in act_dict[layer_name] (CTA.py:36-40)."""
    return lambda module, inputs, output: act_dict.__setitem__(layer_name, output)


def sampling(points, sample_size):
    """sample_size rows of points drawn with replacement from numpy's global generator reseeded to 1 (CTA.py:43-49):
    the same rows on every call."""
    np.random.seed(1)
    return points[np.random.choice(points.shape[0], size=sample_size)]


# ----------------------------------------------------------------------------------------------------------------------
# the victim
# ----------------------------------------------------------------------------------------------------------------------
def _is_pointnet(network):
    return isinstance(network, _pointnet.PointNetCls)


def _pointnet_logits(network, x):
    """z [B,k], the pre-softmax logits of a PointNetCls, with autograd history (the module's own forward up to fc3)."""
    head = network.folded()
    g = network.feat(x)[0]
    g = ops.linear_act(g, *head[0], "relu")
    g = ops.linear_act(g, *head[1], "relu")
    return ops.linear_act(g, *head[2])


def _generic_forward(network, x, layer_activation, layer_name):
    """(output, z): the victim's first output and the hooked layer's activation, by autograd. A PointNetCls computes fc3
    inside a fused launch, so no hook of it ever fires: its logits are taken from its own layers."""
    if _is_pointnet(network):
        z = _pointnet_logits(network, x)
        return torch.log_softmax(z, dim=1), z
    if layer_activation is not None:
        layer_activation.pop(layer_name, None)
    out = network(x)
    out = out[0] if isinstance(out, (tuple, list)) else out
    z = None if layer_activation is None else layer_activation.get(layer_name)
    if z is None:
        raise RuntimeError(f"CTA: no forward hook filled layer_activation[{layer_name!r}] during the victim's forward; "
                           "register CTA.layer_hook on the layer whose activation the attack optimises")
    return out, z


def _check_cuda(t, who):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise NotImplementedError(f"{who}: the critical-point attack runs on the GPU only (there is no CPU path); "
                                  "pass CUDA tensors")


def input_gradients(network, clouds, B, target_class, set_size=IG_SET_SIZE, fused=True, out=None, want_logits=False,
                    layer_activation=None, layer_name=None):
    """VanillaGradient.get_mask for R = steps x B clouds [R,3,N] at once: the victim's input gradient [R,3,N] for the
    cotangent on its log-softmax output that is zero except in rows j < set_size of every step. want_logits adds what
    the hooked layer holds after this forward: the pre-softmax logits of a PointNetCls, the hook's activation of any
    other victim when layer_activation / layer_name name one that fired (else the victim's first output)."""
    _check_cuda(clouds, "VanillaGradient.get_mask")
    if B < set_size:
        raise IndexError(f"index {B} is out of bounds for dimension 0 with size {B}")     # target[j] of the reference
    tc = int(target_class) if target_class else None
    clouds = clouds.float().contiguous()
    if fused and _is_pointnet(network):
        with torch.no_grad():
            logits, ctx = _pointnet.fused_forward(network, clouds)
            g = _pointnet.fused_input_grad(ctx, ops.ig_cotangent(logits, B, set_size, tc), out=out)
        return (g, logits) if want_logits else g
    x = clouds.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        if _is_pointnet(network) or (layer_activation is not None and layer_name is not None):
            logp, z = _generic_forward(network, x, layer_activation, layer_name)
        else:
            logp = network(x)
            logp = z = logp[0] if isinstance(logp, (tuple, list)) else logp
        R, k = logp.shape
        t = torch.zeros((R // B, B, k), dtype=logp.dtype, device=logp.device)
        if tc is None:
            top = logp.detach().view(R // B, B, k).argmax(2)
            multi = torch.zeros((R // B, k), dtype=logp.dtype, device=logp.device).scatter_(1, top, 1.0)
            t[:, :set_size] = multi[:, None, :]
        else:
            t[:, :set_size, tc] = 1.0
        (g,) = torch.autograd.grad(logp, x, t.view(R, k))
    if out is not None:
        out.copy_(g)
        g = out
    return (g.contiguous(), z.detach()) if want_logits else g.contiguous()


def saliency(network, sets, ori_cls, IG_steps=25, baseline='black', fused=True, keep_grads=False, layer_activation=None,
             layer_name=None):
    """Integrated gradients of G sets [G,S,3,N]: dict(mask float64 [G,3,N,S], contri_cn [G,3,S], contri_bn [G,S,N],
    base [G], last [G,S,k]: what the hooked layer holds for the last step's clouds, the last forward before the loop)."""
    _check_cuda(sets, "IntegratedGradients.get_mask")
    G, S, _, N = sets.shape
    sets = sets.float()
    alphas = np.linspace(0, 1, IG_steps)
    rows = IG_steps * S
    clouds = torch.empty((G * rows, 3, N), dtype=torch.float32, device=sets.device)
    bases = []
    for g in range(G):
        c, b = ops.ig_steps(sets[g], alphas, baseline)
        clouds[g * rows:(g + 1) * rows] = c
        bases.append(b)
    grads = torch.empty_like(clouds)
    last = []
    # whole steps of one set per victim pass
    per = max(1, MAX_ROWS // S) * S
    for g in range(G):
        for a in range(0, rows, per):
            lo, hi = g * rows + a, g * rows + min(a + per, rows)
            _, logits = input_gradients(network, clouds[lo:hi], S, ori_cls[g], IG_SET_SIZE, fused, out=grads[lo:hi], want_logits=True,
                                        layer_activation=layer_activation, layer_name=layer_name)
        last.append(logits[-S:])
    res = dict(mask=[], contri_cn=[], contri_bn=[], base=torch.cat(bases), last=torch.stack(last))
    for g in range(G):
        m, cn, bn = ops.ig_reduce(grads[g * rows:(g + 1) * rows], sets[g], bases[g])
        res["mask"].append(m), res["contri_cn"].append(cn), res["contri_bn"].append(bn)
    for key in ("mask", "contri_cn", "contri_bn"):
        res[key] = torch.stack(res[key])
    if keep_grads:
        res["grads"] = grads
    return res


# ----------------------------------------------------------------------------------------------------------------------
# ranking (host) and the selection table
# ----------------------------------------------------------------------------------------------------------------------
def selection_table(contr_index, variant, S, N, set_size=2):
    """The flat (sample * N + point) slots either variant unmasks per level, from its contr_index: (sel int32 [P,W], cap).
    'cta' (CTA.py:185-188): contr_index [3,B]; level pa <= 2 unmasks points contr_index[pa][:] of sample 0: P = 3, W = B,
    cap 3. 'sumloss' (CTA_sumloss.py:190-192): contr_index [B,N]; level pa unmasks point contr_index[j][pa] of every
    sample j < set_size: P = N, W = set_size, no cap."""
    ci = np.asarray(contr_index)
    if variant == "cta":
        if ci.shape != (3, S):
            raise ValueError(f"selection_table: 'cta' ranks a [3,{S}] table, got {ci.shape}")
        return np.ascontiguousarray(ci[:3], dtype=np.int32), 3
    if variant == "sumloss":
        if ci.shape != (S, N) or set_size > S:
            raise ValueError(f"selection_table: 'sumloss' ranks a [{S},{N}] table with set_size <= {S}, got {ci.shape}, {set_size}")
        j = np.arange(set_size, dtype=np.int64)[None, :]
        return np.ascontiguousarray(j * N + ci[:set_size].T, dtype=np.int32), 0x7fffffff
    raise ValueError(f"selection_table: unknown variant {variant!r}")


def rank(sal, g, variant):
    """(contri, contr_index) of set g as the reference forms them: float64, np.argsort(kind='quicksort')."""
    contri = sal["contri_cn" if variant == "cta" else "contri_bn"][g].cpu().numpy()
    return contri, np.argsort(contri, axis=-1, kind='quicksort', order=None)


# ----------------------------------------------------------------------------------------------------------------------
# the loop
# ----------------------------------------------------------------------------------------------------------------------
class _Loop(_graphed.DeviceLoop):
    """Static buffers of one problem shape (`s`), one step as the body, captured (graph=True) as ONE graph of a window's
    25 steps: run_window() is its only use."""

    def __init__(self, network, G, S, N, k, P, W, dev, mode, targeted, optimizer, fused, key=None):
        super().__init__(key, dev, owners=(network,), counts=(WINDOW,), warmup=1)
        f32 = dict(dtype=torch.float32, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        self.network, self.fused, self.G, self.S = network, fused, G, S
        self.s = self.bufs
        self.s.update(
            x=torch.zeros((G * S, 3, N), **f32), proto=torch.zeros((G * S, 3, N), **f32), v=torch.zeros((G * S, 3, N), **f32),
            s_adam=torch.zeros((G * S, 3, N), **f32) if optimizer == "Adam" else None,
            sel=torch.full((G, P, W), -1, **i32), cap=0, poll=torch.zeros((G, ops.CTA_POLL_WORDS), **i32),
            ctrl=torch.zeros((G,), **i32), ori=torch.zeros((G,), **i32), tar=torch.zeros((G,), **i32),
            w=torch.zeros((S,), **f32), hist_ori=torch.zeros((G, ops.CTA_HISTORY), **f32),
            hist_max=torch.zeros((G, ops.CTA_HISTORY), **f32), zlast=torch.zeros((G * S, k), **f32),
            mode=mode, targeted=targeted, optimizer=optimizer, S=S)
        self.layer_activation, self.layer_name = None, None
        self.penalty = None            # (beta, per-set levels on the host): the Chamfer term of CTA.py:165-174

    def load(self, sets, sel, cap, ori, tar, w, start, live):
        s = self.s
        G, S = self.G, self.S
        flat = sets.reshape(G * S, 3, -1)
        s["x"].copy_(flat), s["proto"].copy_(flat), s["v"].zero_()
        if s["s_adam"] is not None:
            s["s_adam"].zero_()
        s["sel"].copy_(torch.as_tensor(sel)), s["ori"].copy_(torch.as_tensor(ori, dtype=torch.int32))
        s["tar"].copy_(torch.as_tensor(tar, dtype=torch.int32)), s["w"].copy_(torch.as_tensor(w, dtype=torch.float32))
        s["cap"] = cap
        poll = np.zeros((G, ops.CTA_POLL_WORDS), dtype=np.int32)
        poll[:, _P_NPP] = start
        poll[:, _P_LATCH] = np.where(live, 0, 2)
        s["poll"].copy_(torch.from_numpy(poll)), s["ctrl"].zero_(), s["hist_ori"].zero_(), s["hist_max"].zero_(), s["zlast"].zero_()

    def step(self):
        s = self.s
        if self.fused:
            with torch.no_grad():
                logits, ctx = _pointnet.fused_forward(self.network, s["x"])
                g = _pointnet.fused_input_grad(ctx, ops.cta_cotangent(logits, s))
        else:
            x = s["x"].detach().clone().requires_grad_(True)
            with torch.enable_grad():
                _, z = _generic_forward(self.network, x, self.layer_activation, self.layer_name)
                gl = ops.cta_cotangent(z.detach().float().contiguous(), s)
                loss = (z * gl).sum()
                if self.penalty is not None:
                    beta, levels = self.penalty
                    for gi in range(self.G):
                        if levels[gi] > 0:     # `for pa in range(num_p_per): total_dis = chamfer(input, prototype)`
                            sl = slice(gi * self.S, (gi + 1) * self.S)
                            loss = loss + beta * dis_utils_torch.chamfer(x[sl], s["proto"][sl])
                (g,) = torch.autograd.grad(loss, x)
            g = g.float().contiguous()
        ops.cta_update(s, g)

    body = step

    def steps(self):
        for _ in range(WINDOW):
            self.step()

    def run_window(self):
        self.run(WINDOW)


def _loop_for(network, G, S, N, k, P, W, dev, mode, targeted, optimizer, fused, graph, loader):
    if not (fused and graph):
        c = _Loop(network, G, S, N, k, P, W, dev, mode, targeted, optimizer, fused)
        loader(c)
        return c
    key = _graphed.loop_key(network, dev, G, S, N, k, P, W, mode, targeted, optimizer)
    c = _LOOPS.get(key)
    if c is None:
        c = _LOOPS.put(key, _Loop(network, G, S, N, k, P, W, dev, mode, targeted, optimizer, fused, key))
        loader(c)
        c.capture()
    loader(c)
    return c


def _as_list(v, G, name):
    if isinstance(v, (list, tuple, np.ndarray)) or (torch.is_tensor(v) and v.dim() > 0):
        v = [int(e) for e in v]
        if len(v) != G:
            raise ValueError(f"cta_attack: {name} has {len(v)} entries for {G} sets")
        return v
    return [int(v)] * G


def cta_attack(network, sets, ori_cls, variant='cta', target_att=False, tar_cls=None, alpha=1e-6, beta=1e-4, IG_steps=25,
               n_points=1, verbose=False, using_softmax_neuron=False, penalize_dis=False, optimizer='Adam', set_size=2,
               layer_activation=None, layer_name=None, fused=True, graph=True, return_info=False):
    """The critical-point attack on G sets [G,S,3,N] at once; every set has its own level, counters, optimiser state and
    latch. ori_cls / tar_cls: one class or one per set. Returns (states, best_img [G,S,3,N], ori_logits, max_other_logits):
    per set 'Suc', 'Fail', 'Exhausted' (the reference's ``act_max`` returns None there) or 'IndexError' (``CTA_sumloss.py`` raises it
    when a level passes N; ``act_max`` raises it too, here the other sets of the batch keep their results) and the two record lists of its
    last pass (numpy 0-d float32 values). return_info adds a dict: mask, contri, contr_index, tar_cls, num_p_per, steps,
    cur_step, decisions and means per set."""
    _check_cuda(sets, "cta_attack")
    if variant not in ("cta", "sumloss"):
        raise ValueError(f"cta_attack: variant must be 'cta' or 'sumloss', got {variant!r}")
    if optimizer not in ("Adam", "Momentum"):
        raise ValueError(f"cta_attack: optimizer must be 'Adam' or 'Momentum', got {optimizer!r}")
    if sets.dim() != 4 or sets.shape[2] != 3:
        raise ValueError(f"cta_attack: sets must be [G,S,3,N], got {tuple(sets.shape)}")
    G, S, _, N = sets.shape
    dev = sets.device
    sets = sets.detach().float().contiguous()
    network.eval()
    ori = _as_list(ori_cls, G, "ori_cls")
    use_fused = bool(fused and _is_pointnet(network) and not (penalize_dis and variant == "cta"))
    targeted = target_att is not False
    if variant == "sumloss" and set_size > S:
        raise IndexError(f"index {S} is out of bounds for dimension 0 with size {S}")

    sal = saliency(network, sets, ori, IG_steps, 'black', fused=fused, layer_activation=layer_activation, layer_name=layer_name)
    k = sal["last"].shape[-1]
    z_last = sal["last"].cpu()
    # the target class: host code, as in the reference (random.randint / topk on the last forward's activation of sample 0)
    if tar_cls is not None:
        tar = _as_list(tar_cls, G, "tar_cls")
    elif target_att == 'random':
        tar = []
        for g in range(G):
            t = ori[g]
            while t == ori[g]:
                t = random.randint(0, 104)
            tar.append(t)
    elif target_att == 'second':
        tar = [int(torch.topk(z_last[g][0], 2).indices[-1]) for g in range(G)]
    elif target_att == 'least':
        tar = [int(torch.topk(z_last[g][0], 105).indices[-1]) for g in range(G)]
    elif targeted:
        raise NameError("name 'tar_cls' is not defined")          # the reference, for any other truthy target_att
    else:
        tar = [0] * G
    for c in ori + (tar if targeted else []):
        if not 0 <= c < k:
            raise IndexError(f"index {c} is out of bounds for dimension 0 with size {k}")

    sels, limits, info = [], [], dict(contri=[], contr_index=[])
    for g in range(G):
        contri, ci = rank(sal, g, variant)
        sel, cap = selection_table(ci, variant, S, N, set_size)
        sels.append(sel), limits.append(int(np.sum(contri > 0)))
        info["contri"].append(contri), info["contr_index"].append(ci)
    sel = np.stack(sels)
    start = n_points if variant == "sumloss" else 0
    # 'sumloss' reads contr_index[j][pa] for pa < level: a level above N is the reference's IndexError at its first step
    live = np.array([start < limits[g] and not (variant == "sumloss" and start > N) for g in range(G)])

    a32 = np.float32(float(alpha))
    w = np.zeros((S,), dtype=np.float32)
    if variant == "cta":
        w[0] = a32
        mode = "log_softmax" if using_softmax_neuron else ("ori_minus_tar" if targeted else "ori_minus_second")
    else:
        share = np.float32(a32 * np.float32(1.0 / set_size))
        if using_softmax_neuron or targeted:
            w[set_size - 1] = share                                # the reference's loop overwrites: the last sample only
            mode = "log_softmax" if using_softmax_neuron else "ori_minus_tar"
        else:
            w[:set_size] = share
            mode = "ori"

    loop = _loop_for(network, G, S, N, k, sel.shape[1], sel.shape[2], dev, mode, targeted, optimizer, use_fused, graph,
                     lambda c: c.load(sets, sel, cap, ori, tar, w, start, live))
    loop.layer_activation, loop.layer_name = layer_activation, layer_name
    levels = [start] * G
    loop.penalty = (float(beta), levels) if (penalize_dis and variant == "cta") else None
    s = loop.s

    states = [None if live[g] else ('IndexError' if start > N and start < limits[g] else 'Exhausted') for g in range(G)]
    last_ori, last_tar = [float('inf')] * G, [-float('inf')] * G
    decisions, means = [[] for _ in range(G)], [[] for _ in range(G)]
    while any(st is None for st in states):
        loop.run_window()
        p = s["poll"].cpu().numpy()                                # the one copy: windows, latches, counters
        ctrl = np.zeros((G,), dtype=np.int32)
        for g in range(G):
            if states[g] is not None:
                continue
            if p[g, _P_LATCH] == 1:
                states[g] = 'Suc'
                continue
            cur, step = int(p[g, _P_CUR]), int(p[g, _P_STEP])
            new_ori = np.mean(np.ascontiguousarray(p[g, 0:WINDOW]).view(np.float32))
            brk = bool(new_ori >= last_ori[g]) or cur >= PASS_MAX
            new_tar = np.nan
            if targeted:
                new_tar = np.mean(np.ascontiguousarray(p[g, WINDOW:2 * WINDOW]).view(np.float32))
                brk = brk or bool(new_tar <= last_tar[g])
            means[g].append((float(new_ori), float(new_tar))), decisions[g].append(int(brk))
            if not brk:
                last_ori[g], last_tar[g] = new_ori, new_tar
                continue
            if step >= TOTAL_MAX:
                states[g], ctrl[g] = 'Fail', 2
            elif levels[g] + 1 >= limits[g]:
                states[g], ctrl[g] = 'Exhausted', 2
            else:
                if variant == "sumloss" and levels[g] + 1 > N:
                    states[g], ctrl[g] = 'IndexError', 2                # contr_index[j][pa] with pa = N
                    continue
                levels[g] += 1
                last_ori[g], last_tar[g] = float('inf'), -float('inf')
                ctrl[g] = 1
        if ctrl.any():
            s["ctrl"].copy_(torch.from_numpy(ctrl))
            ops.cta_update(s, control=True)

    p = s["poll"].cpu().numpy()
    hist_o, hist_m = s["hist_ori"].cpu().numpy(), s["hist_max"].cpu().numpy()
    ori_logits = [[hist_o[g, i].copy() for i in range(min(int(p[g, _P_CUR]), ops.CTA_HISTORY))] for g in range(G)]
    max_other = [[hist_m[g, i].copy() for i in range(min(int(p[g, _P_CUR]), ops.CTA_HISTORY))] for g in range(G)]
    best = s["x"].detach().clone().view(G, S, 3, N)
    if layer_activation is not None and layer_name is not None:
        layer_activation[layer_name] = s["zlast"].detach().clone()      # the logits of every set's last forward
    res = (states, best, ori_logits, max_other)
    if return_info:
        info.update(mask=sal["mask"], tar_cls=tar if targeted else [-1] * G, num_p_per=[int(v) for v in p[:, _P_NPP]],
                    steps=[int(v) for v in p[:, _P_STEP]], cur_step=[int(v) for v in p[:, _P_CUR]], decisions=decisions,
                    means=means, fused=use_fused, loop=loop)
        return res + (info,)
    return res


def _act_max(variant, network, input, layer_activation, layer_name, ori_cls, alpha, beta, target_att, IG_steps, n_points,
             verbose, using_softmax_neuron, penalize_dis, optimizer, set_size=2):
    _check_cuda(input, "act_max")
    states, best, ori_logits, max_other = cta_attack(
        network, input.detach()[None], ori_cls, variant=variant, target_att=target_att, alpha=alpha, beta=beta,
        IG_steps=IG_steps, n_points=n_points, verbose=verbose, using_softmax_neuron=using_softmax_neuron,
        penalize_dis=penalize_dis, optimizer=optimizer, set_size=set_size, layer_activation=layer_activation,
        layer_name=layer_name)
    if states[0] == 'IndexError':
        raise IndexError(f"index {input.shape[2]} is out of bounds for axis 0 with size {input.shape[2]}")
    if states[0] == 'Exhausted':
        return None                     # the reference falls off the end of act_max
    return states[0], best[0], ori_logits[0], max_other[0]


def act_max(network,
            input,
            layer_activation,
            layer_name,
            ori_cls,
            alpha,
            beta,
            target_att=False,
            IG_steps=25,
            n_points=1,
            verbose=False,
            using_softmax_neuron=False,
            penalize_dis=False,
            optimizer='Adam'
            ):
    """CTA.py:58-286 for one set [S,3,N]: (state, best_img, ori_logits, max_other_logits), or None where the reference
    falls off its end. ``cta_attack`` with G = 1."""
    return _act_max("cta", network, input, layer_activation, layer_name, ori_cls, alpha, beta, target_att, IG_steps,
                    n_points, verbose, using_softmax_neuron, penalize_dis, optimizer)
