"""TEST INFRASTRUCTURE: a plain-torch restatement of the reference's three query attacks (attack/SIadv/SIadv_attack.py:
343-624: simba_attack, simbapp_attack, shape_invariant_query_attack), batched, for any device and dtype, with the table
of every cloud as an input. It is the checker of tests/test_siadv_query_*.py and the same-device baseline of
tools/bench_siadv_query.py; the product never imports it. Clouds are [B,N,3] here, as in the reference.

All clouds advance in lock step (entry i of every table in step i); a cloud whose loop has ended is left alone. Both
tries of a step are evaluated (the reference skips the second one after an accepted first one; its loss is recorded as
the loss that would have been computed) and the decision is the reference's: try 0, and only if rejected, try 1.
"""
import numpy as np
import torch

import siadv_restatement as R


def sign_order(step_size):
    """The order in which the reference's `for eps in {step_size, -step_size}` visits the two signs."""
    return tuple({step_size, -step_size})


def first(out):
    return out[0] if isinstance(out, (tuple, list)) else out


def query_loss(logp, target, top5=False):
    """CWLoss(kappa=-999, tar=True) per cloud [B] (:142-164): max(other - real, -999)."""
    onehot = torch.eye(logp.shape[1], dtype=logp.dtype, device=logp.device)[target.long()]
    real = torch.sum(onehot * logp, 1)
    masked = (1 - onehot) * logp - onehot * 10000
    other = torch.topk(masked, 5)[0][:, 4] if top5 else torch.max(masked, 1)[0]
    return torch.max(other - real, torch.full_like(other, -999.))


def top5_rule(logp, target):
    return torch.where((logp.topk(5)[1] == target[:, None]).any(1), target, torch.full_like(target, -1))


def initial_query(victim, P, target, top5=False, pre_head=None):
    """(logp [B,k], adv_target [B]) of the clean clouds P [B,N,3]."""
    x = P.transpose(1, 2).contiguous()
    with torch.no_grad():
        logp = first(victim(pre_head(x) if pre_head is not None else x))
    adv_target = top5_rule(logp, target) if top5 else logp.argmax(1)
    return logp, adv_target


def simba_basis(N):
    """basis_list before the shuffle (:371-375): [3N,2] rows (channel, idx), the point index outermost."""
    return np.array([(i, j) for j in range(N) for i in range(3)])


def draw_simba_tables(N, active):
    """The reference's draws: one np.random.shuffle of the [3N,2] list per cloud that did not return early, in cloud
    order. Returns int32 [B,3N] of 3 * idx + channel (zeros for the clouds that returned early)."""
    tab = np.zeros((len(active), 3 * N), np.int32)
    for b, on in enumerate(active):
        if on:
            basis = simba_basis(N)
            np.random.shuffle(basis)
            tab[b] = 3 * basis[:, 1] + basis[:, 0]
    return tab


def surrogate_grad(surrogate, x_cf, target, top5=False):
    """d CWLoss(kappa=-999, tar=True) / dx of the surrogate at x_cf [B,3,N] (the loss is a sum over the clouds)."""
    x = x_cf.detach().clone().requires_grad_()
    loss = query_loss(first(surrogate(x)), target, top5).sum()
    (g,) = torch.autograd.grad(loss, x)
    return g


def simbapp_tables(surrogate, P, target, step_size, generator, top5=False):
    """The restated simbapp draws: choices [B,3N] = multinomial(|g|.reshape(-1)) (a choice c stands for channel c % 3 of
    point c // 3, as the reference unpacks it) and the amounts [B,3N,2] = sign + 0.1 randn."""
    B, N, _ = P.shape
    g = surrogate_grad(surrogate, P.transpose(1, 2).contiguous(), target, top5)
    w = g.abs().reshape(B, -1)
    tab = torch.multinomial(w, 3 * N, replacement=True, generator=generator).to(torch.int32)
    signs = torch.tensor(sign_order(step_size), dtype=P.dtype, device=P.device)
    eps = signs[None, None, :] + 0.1 * torch.randn((B, 3 * N, 2), generator=generator, dtype=P.dtype, device=P.device)
    return tab, eps


def ours_tables(surrogate, P, n, target, eps, top5=False):
    """The sensitivity map (:536-563) from clouds P and unit normals n [B,N,3]: (order [B,N] by ranking descending,
    stable; directions [B,N,3]; rankings [B,N])."""
    U = R.spin_axis_matrix(n)
    t = (P * n).sum(-1, keepdim=True) * n
    Pp = (U @ (P + t)[..., None])[..., 0].detach().requires_grad_()
    inputs = (U.transpose(-1, -2) @ Pp[..., None])[..., 0] - t
    inputs = torch.min(torch.max(inputs, P - eps), P + eps)
    loss = query_loss(first(surrogate(inputs.transpose(1, 2))), target, top5).sum()
    (g,) = torch.autograd.grad(loss, Pp)
    g = g.clone()
    g[..., 2] = 0.
    rank = torch.sqrt(g[..., 0] ** 2 + g[..., 1] ** 2)
    dirs = g / (rank[..., None] + 1e-16)
    order = torch.sort(rank, dim=1, descending=True, stable=True)[1]
    return order.to(torch.int32), dirs, rank


def run_query(victim, P, target, tab, eps, top5=False, frame=None, active=None, pre_head=None, init=None):
    """The query loop. P [B,N,3], tab [B,L] integer, eps [2] or [B,L,2] (the amount of each try).
    frame: None — coordinate mode, entry e is coordinate e % 3 of point e // 3 (simba, simbapp); or (n [B,N,3] unit
    normals, dirs [B,N,3]) — the shape-invariant mode, entry e is a point. active [B] bool: clouds whose loop runs (the
    others returned early). init: (logp, adv_target) of initial_query, computed here when None.
    Returns a dict: adv_points (the accepted state; in frame mode the last candidate evaluated), adv_target, query_costs,
    accepted [B,L] (0 / 1, -1 neither, -2 not reached), losses [B,L,2], best [B,L] (NaN where not reached)."""
    B, N, _ = P.shape
    L = tab.shape[1]
    dev, dt = P.device, P.dtype
    tab = torch.as_tensor(tab, device=dev).long()
    eps = torch.as_tensor(eps, device=dev).to(dt)
    if eps.dim() == 1:
        eps = eps[None, None, :].expand(B, L, 2)
    logp0, adv_target = init if init is not None else initial_query(victim, P, target, top5, pre_head)
    adv_target = adv_target.clone()
    active = torch.ones(B, dtype=torch.bool, device=dev) if active is None else torch.as_tensor(active, device=dev).bool()
    queries = torch.ones(B, dtype=torch.int64, device=dev)
    best = torch.full((B,), -999., dtype=dt, device=dev)
    accepted = torch.full((B, L), -2, dtype=torch.int64, device=dev)
    losses = torch.full((B, L, 2), float("nan"), dtype=dt, device=dev)
    bests = torch.full((B, L), float("nan"), dtype=dt, device=dev)
    last_logp = logp0.clone()
    ar = torch.arange(B, device=dev)
    if frame is None:
        state = P.clone()
    else:
        n, dirs = frame
        U = R.spin_axis_matrix(n)
        t = (P * n).sum(-1, keepdim=True) * n
        state = (U @ (P + t)[..., None])[..., 0]
    last_cand = P.clone()

    def show(s):
        return s if frame is None else (U.transpose(-1, -2) @ s[..., None])[..., 0] - t

    for i in range(L):
        live = active & (best < 0)
        if not bool(live.any()):
            break
        e = tab[:, i]
        cands = []
        for k in range(2):
            pert = torch.zeros_like(state)
            if frame is None:
                pert[ar, e // 3, e % 3] += eps[:, i, k]
            else:
                pert[ar, e] += eps[:, i, k, None] * dirs[ar, e]
            cands.append(state + pert)
        x = torch.cat([show(c) for c in cands]).transpose(1, 2).contiguous()
        with torch.no_grad():
            logp = first(victim(pre_head(x) if pre_head is not None else x))
        l0, l1 = query_loss(logp[:B], target, top5), query_loss(logp[B:], target, top5)
        a0 = l0 > best
        a1 = ~a0 & (l1 > best)
        acc = torch.where(a0, 0, torch.where(a1, 1, -1))
        take = live & (acc >= 0)
        pick1 = (acc == 1)
        new_state = torch.where(pick1[:, None, None], cands[1], cands[0])
        state = torch.where(take[:, None, None], new_state, state)
        new_loss = torch.where(pick1, l1, l0)
        best = torch.where(take, new_loss, best)
        lp_acc = torch.where(pick1[:, None], logp[B:], logp[:B])
        adv_target = torch.where(take, lp_acc.argmax(1), adv_target)
        last1 = ~a0                                            # the last try evaluated: try 1 unless try 0 was accepted
        last_logp = torch.where(live[:, None], torch.where(last1[:, None], logp[B:], logp[:B]), last_logp)
        shown = torch.where(last1[:, None, None], show(cands[1]), show(cands[0]))
        last_cand = torch.where(live[:, None, None], shown, last_cand)
        queries = queries + torch.where(live, torch.where(a0, 1, 2), 0)
        accepted[:, i] = torch.where(live, acc, accepted[:, i])
        losses[:, i, 0] = torch.where(live, l0, losses[:, i, 0])
        losses[:, i, 1] = torch.where(live, l1, losses[:, i, 1])
        bests[:, i] = torch.where(live, best, bests[:, i])
    if top5:
        adv_target = torch.where(active, top5_rule(last_logp, target), adv_target)
    adv_points = state if frame is None else last_cand
    return dict(adv_points=adv_points, adv_target=adv_target, query_costs=queries, accepted=accepted, losses=losses, best=bests,
                state=state, last_logp=last_logp)
