"""The critical-point attack (the reference's attack/CTA/CTA.py and CTA_sumloss.py with utils/{vanilla_gradient,
integrated_gradients}.py) restated in plain torch + numpy, on whatever device the cloud lives on. It follows the reference
statement by statement — the saliency's cotangent with its fancy-indexed multi-hot, the float64 accumulation, the
[3,B] / [B,N] ranking, the unmasking per level, Adam without bias correction, the records with the original logit
negated, the 25-step windows — and records what the reference only prints: every window mean, every decision and the
level at exit. tests/golden/make_golden_cta.py checks on the CPU that it reproduces the real reference bit for bit;
tests/test_cta_gpu.py and tools/bench_cta.py run it on the GPU next to the device loop.

`forward(x) -> (logp, z)`: the victim's first output (log-softmax, what VanillaGradient differentiates) and the hooked
layer's activation (the pre-softmax logits, what the loop reads), both with autograd history.
"""
import numpy as np
import torch


def hooked_forward(network, layer, device_dtype=None):
    """forward(x) for a victim whose `layer` (the last linear layer) is called in its forward: a forward hook catches z."""
    box = {}
    layer.register_forward_hook(lambda mod, inp, out: box.__setitem__("z", out))

    def forward(x):
        out = network(x)
        return (out[0] if isinstance(out, (tuple, list)) else out), box["z"]
    return forward


def vanilla_mask(forward, x, target_class, set_size=2):
    """VanillaGradient.get_mask (vanilla_gradient.py:11-25): [3,N,B] numpy, the input gradient with the batch axis last."""
    x = x.clone().requires_grad_(True)
    logp, _ = forward(x)
    target = torch.zeros_like(logp)
    for j in range(set_size):                      # B < set_size raises IndexError, as the reference does
        target[j][target_class if target_class else logp.topk(1, dim=1)[1]] = 1
    logp.backward(target)
    return np.moveaxis(x.grad.detach().cpu().numpy(), 0, -1)


def ig_mask(forward, x, target_class, steps=25, baseline="black", want_steps=False):
    """IntegratedGradients.get_mask (integrated_gradients.py:8-26): float64 [3,N,B]."""
    if baseline == "black":
        base = torch.ones_like(x) * torch.min(x).detach()
    elif baseline == "white":
        base = torch.ones_like(x) * torch.max(x).detach()
    else:
        base = torch.zeros_like(x)
    B, C, N = x.shape
    grad_sum = np.moveaxis(np.zeros((N, C, B)), 1, 0)
    diff = x - base
    per_step = []
    for alpha in np.linspace(0, 1, steps):
        g = vanilla_mask(forward, base + alpha * diff, target_class)
        per_step.append(g)
        grad_sum += g
    mask = grad_sum * np.moveaxis(diff.detach().cpu().numpy(), 0, -1) / steps
    return (mask, per_step) if want_steps else mask


def rank(mask, variant):
    """(contri, contr_index) as CTA.py:93-94 ([3,B]) or CTA_sumloss.py:87-91 ([B,N]) form them."""
    if variant == "sumloss":
        mask = np.moveaxis(mask, -1, 0)
    contri = np.sum(mask, axis=1)
    return contri, np.argsort(contri, axis=-1, kind="quicksort", order=None)


def run(forward, x, ori_cls, alpha, beta=0.0, variant="cta", target_att=False, tar_cls=None, IG_steps=25, n_points=1,
        using_softmax_neuron=False, penalize_dis=False, optimizer="Adam", set_size=2, chamfer=None, max_total=15000,
        mask=None):
    """act_max of either variant. target_att False, 'second', or anything else with tar_cls given. Returns a dict: state
    ('Suc' | 'Fail' | None where the reference falls off its end), best_img, ori_logits, max_other_logits (lists of numpy
    0-d values), mask, contri, contr_index, tar_cls, means (one row per window: new_ori, new_tar or nan), decisions (one
    int per window: 1 = break), num_p_per at exit, steps (total), cur_step, z0 (sample 0's logits of every step)."""
    prototype = x.detach().clone()
    if mask is None:
        mask = ig_mask(forward, prototype, ori_cls, IG_steps, "black")
    contri, contr_index = rank(mask, variant)
    with torch.no_grad():
        _, z_last = forward(_last_ig_cloud(prototype, IG_steps))     # what the hook holds when the target is chosen
    if target_att == "second":
        tar_cls = int(torch.topk(z_last[0], 2).indices[-1])
    res = dict(mask=mask, contri=contri, contr_index=contr_index, tar_cls=-1 if tar_cls is None else int(tar_cls),
               means=[], decisions=[], z0=[], state=None, num_p_per=-1, steps=0, cur_step=0)
    v = torch.zeros_like(prototype)
    v_adam = torch.zeros_like(prototype)
    s_adam = torch.zeros_like(prototype)
    step = 0
    inp = prototype.clone()
    ori_logits, max_other = [], []
    start = n_points if variant == "sumloss" else 0

    def done(state, npp, cur):
        res.update(state=state, best_img=inp.detach(), ori_logits=ori_logits, max_other_logits=max_other, num_p_per=npp,
                   steps=step, cur_step=cur)
        return res

    res.update(best_img=inp.detach(), ori_logits=ori_logits, max_other_logits=max_other)
    for num_p_per in range(start, int(np.sum(contri > 0))):
        cur_step = 0
        last_ori, last_tar = float("inf"), -float("inf")
        rec_ori, rec_tar = [], []
        ori_logits, max_other = [], []
        inp = prototype.clone().requires_grad_(True)
        while True:
            step += 1
            cur_step += 1
            _, z = forward(inp)
            if variant == "cta":
                if using_softmax_neuron:
                    loss = alpha * torch.log(torch.softmax(z[0], dim=0))[ori_cls]
                elif target_att is not False:
                    loss = alpha * (z[0][ori_cls] - z[0][tar_cls])
                else:
                    loss = alpha * (z[0][ori_cls] - z[0][torch.topk(z[0], 2).indices[-1]])
                if penalize_dis:
                    total = 0
                    for pa in range(num_p_per):
                        total = chamfer(inp, prototype)
                    loss = loss + beta * total
            else:
                loss = torch.zeros((), dtype=z.dtype, device=z.device)
                if using_softmax_neuron:
                    for j in range(set_size):
                        loss = alpha * torch.log(torch.softmax(z[j], dim=0))[ori_cls]
                    loss = loss / set_size
                elif target_att is not False:
                    for j in range(set_size):
                        loss = alpha * (z[j][ori_cls] - z[j][tar_cls])
                    loss = loss / set_size
                else:
                    for j in range(set_size):
                        loss = loss + alpha * z[j][ori_cls]
                    loss = loss / set_size
            (grad,) = torch.autograd.grad(loss, inp)
            masked = torch.zeros_like(grad)
            if variant == "cta":
                for pa in range(num_p_per):
                    if pa > 2:
                        continue
                    masked[0, :, contr_index[pa]] = grad[0, :, contr_index[pa]]
            else:
                for j in range(set_size):
                    for pa in range(num_p_per):
                        masked[j, :, contr_index[j][pa]] = grad[j, :, contr_index[j][pa]]
            with torch.no_grad():
                if optimizer == "Momentum":
                    v = 0.9 * v - masked
                    new = torch.add(inp, v)
                else:
                    b1, b2, xi = 0.9, 0.999, 1e-8
                    v_adam = b1 * v_adam + (1 - b1) * masked
                    s_adam = b2 * s_adam + (1 - b2) * torch.square(masked)
                    new = torch.add(inp, -1 * v_adam / torch.sqrt(s_adam + xi))
            inp = new.detach().requires_grad_(True)
            z0 = z[0].detach()
            res["z0"].append(z0.cpu().numpy().copy())
            ori_logits.append(z0[ori_cls].cpu().numpy())
            tmp = z0.clone()
            tmp[ori_cls] *= -1
            max_other.append(torch.max(tmp).cpu().numpy())
            rec_ori.append(z0[ori_cls].cpu().numpy())
            if target_att is not False:
                rec_tar.append(z0[tar_cls].cpu().numpy())
            cur_class = int(torch.argmax(z0))
            if (target_att is False and cur_class != ori_cls) or (target_att is not False and cur_class == tar_cls):
                return done("Suc", num_p_per, cur_step)
            if cur_step >= 25 and cur_step % 25 == 0:
                new_ori = np.mean(np.asarray(rec_ori[-25:]))
                new_tar = np.mean(np.asarray(rec_tar[-25:])) if target_att is not False else np.nan
                brk = bool(new_ori >= last_ori) or cur_step >= 1500
                if target_att is not False:
                    brk = brk or bool(new_tar <= last_tar)
                res["means"].append((float(new_ori), float(new_tar)))
                res["decisions"].append(int(brk))
                if brk:
                    break
                last_ori, last_tar = new_ori, new_tar
        if step >= max_total:
            return done("Fail", num_p_per, cur_step)
        res.update(num_p_per=num_p_per, steps=step, cur_step=cur_step, best_img=inp.detach(), ori_logits=ori_logits,
                   max_other_logits=max_other)
    res["steps"] = step
    return res


def _last_ig_cloud(x, steps):
    """The cloud of the last forward before the loop: integrated gradients' last step, baseline + 1.0 * (x - baseline)."""
    base = torch.ones_like(x) * torch.min(x).detach()
    return base + np.linspace(0, 1, steps)[-1] * (x - base)


def pointnet_ft_forward(sd):
    """forward(x) for a PointNetCls(k, feature_transform=True) given by its state_dict sd: tests/pointnet_ft_restatement.py's
    statement of the victim, with the logits handed out next to their log-softmax."""
    import pointnet_ft_restatement as pft

    def forward(x):
        dtype = x.dtype
        trans = pft._stn(sd, "feat.stn.", x, 3, dtype)
        xp = torch.einsum("bcd,bcn->bdn", trans, x)
        h = torch.relu(pft._affine(sd, "feat.", "conv1", "bn1", xp, dtype))
        tf = pft._stn(sd, "feat.fstn.", h, 64, dtype)
        u = torch.einsum("bij,bin->bjn", tf, h)
        z2 = torch.relu(pft._affine(sd, "feat.", "conv2", "bn2", u, dtype))
        pooled = pft._affine(sd, "feat.", "conv3", "bn3", z2, dtype).max(dim=2)[0]
        y = torch.relu(pft._affine(sd, "", "fc1", "bn1", pooled, dtype))
        y = torch.relu(pft._affine(sd, "", "fc2", "bn2", y, dtype))
        z = pft._affine(sd, "", "fc3", None, y, dtype)
        return torch.log_softmax(z, dim=1), z
    return forward


def ranking_agrees(ci, ref_ci, ref_contri, band):
    """Compare a ranking with the fixture's wherever it is decided: position p of a row is checked when the fixture's
    contribution there is more than `band` away from both of its sorted neighbours. Returns (all equal, number checked)."""
    ok, checked = True, 0
    for row in range(ref_contri.shape[0]):
        s = ref_contri[row][ref_ci[row]]
        d = np.diff(s)
        sure = (np.concatenate([[np.inf], d]) > band) & (np.concatenate([d, [np.inf]]) > band)
        ok = ok and np.array_equal(np.asarray(ci)[row][sure], ref_ci[row][sure])
        checked += int(sure.sum())
    return ok, checked
