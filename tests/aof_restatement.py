"""A plain-torch restatement of the untargeted AOF attack (attack/AOF/Eval_AOF.py `attack`), written from its behaviour.

Not product code and not a test: tests/golden/make_golden_aof_untargeted.py checks that, on one CPU thread and in fp32, it
reproduces the real reference bit for bit; run in float64 it gives the deviation the tolerance bands of
tests/golden/aof_untargeted.npz are set from; tests/test_aof_untargeted_cpu.py re-runs the fp32 form against the fixture.

    run(model, trans_model, data [B,K,3], label [B], kappa, budget, lr, low_pass, step, epochs, dtype) -> dict

`model` / `trans_model`: callables on [B,3,K] returning the logits (or a tuple that starts with them). The loss is the
untargeted logits margin with `kappa`, the clip the per-point L2 clip with `budget`. Two generators are consumed in the
reference's order: torch's CPU generator (one randn((B,3,K)) per binary step) and numpy's global one (one shuffle per
batch).
"""
import hashlib

import numpy as np
import torch


def digest(a):
    """SHA-256 of an array's bytes (C order) with its dtype and shape: how the fixture stores the iterates."""
    a = np.ascontiguousarray(a)
    return hashlib.sha256(f"{a.dtype.str}{a.shape}".encode() + a.tobytes()).hexdigest()


def logits_of(out):
    return out[0] if isinstance(out, (tuple, list)) else out


def untargeted_margin_loss(logits, label, kappa):
    """mean_b max(logit_label - max_other + kappa, 0); the label's own entry is pushed down by 10000 before the max."""
    hot = torch.zeros(logits.shape, dtype=torch.float32, device=logits.device).scatter_(1, label.view(-1, 1), 1).float().to(logits.dtype)
    real = torch.sum(hot * logits, dim=1)
    other = torch.max((1. - hot) * logits - hot * 10000., dim=1)[0]
    return torch.clamp(real - other + kappa, min=0.).mean()


def margins(logits, label):
    """largest other logit - label logit, per cloud (negative: still classified as the label)."""
    hot = torch.zeros(logits.shape, dtype=torch.bool, device=logits.device).scatter_(1, label.view(-1, 1), True)
    return (logits.masked_fill(hot, -float("inf")).max(dim=1)[0] - logits[hot]).detach()


def clip_points(pc, ori, budget):
    with torch.no_grad():
        diff = pc - ori
        norm = torch.sum(diff ** 2, dim=1) ** 0.5
        scale = torch.clamp(budget / (norm + 1e-9), max=1.)
        return ori + diff * scale[:, None, :]


def knn_idx(x, k):
    """x [B,3,N] -> the k largest entries per row of -|xi|^2 + 2 xi.xj - |xj|^2 (the point itself included)."""
    inner = -2 * torch.matmul(x.transpose(2, 1), x)
    xx = torch.sum(x ** 2, dim=1, keepdim=True)
    return (-xx - inner - xx.transpose(2, 1)).topk(k=k, dim=-1)[1]


def laplace_basis(pc, basis_dtype=torch.double):
    """pc [B,3,N] -> the eigenvectors [B,N,N] (ascending eigenvalues) of L = D - A, A the Gaussian weights
    exp(-|pi - pj|^2) on the symmetrised 30-nearest-neighbour graph; computed in float64 (as the reference does; the
    fp32 form stands for an implementation whose graph and eigensolver are fp32), returned in pc's dtype."""
    p = pc.detach().clone().to(basis_dtype)
    idx = knn_idx(p, 30)
    p = p.transpose(2, 1).contiguous()
    A = torch.exp(-torch.sum((p.unsqueeze(2) - p.unsqueeze(1)).square(), dim=3))
    mask = torch.zeros_like(A)
    mask.scatter_(2, idx, 1)
    mask = mask + mask.transpose(2, 1)
    mask[mask > 1] = 1
    A = A * mask
    L = torch.diag_embed(torch.sum(A, dim=2)) - A
    _, v = torch.linalg.eigh(L)
    return v.to(pc)


def bands(x, V, lp):
    coeff = torch.bmm(x, V)
    hfc = torch.bmm(coeff[..., lp:], V[..., lp:].transpose(2, 1))
    lfc = torch.bmm(coeff[..., :lp], V[..., :lp].transpose(2, 1))
    return lfc, hfc


def shuffled_rows(array):
    seq = np.arange(array.shape[1])
    np.random.shuffle(seq)
    return array[:, seq, :]


def run(model, trans_model, data, label, kappa, budget, lr, low_pass, step, epochs, dtype=torch.float32, basis_dtype=torch.double):
    """Everything runs on data's device (the fixture: the CPU); the records are numpy arrays on the host."""
    ori = data.transpose(2, 1).to(dtype).detach().clone()
    label = label.long()
    B, _, K = ori.shape
    o_bestdist = np.array([1e10] * B)
    o_bestscore = np.array([-1] * B)
    o_bestattack = np.zeros((B, 3, K))
    label_np = label.cpu().numpy()
    iter_adv, iter_lfc, mar_adv, mar_lfc, dists = [], [], [], [], []
    cur = ori
    for _ in range(step):
        cur = ori.clone() + torch.randn((B, 3, K)).to(ori.device) * 1e-7          # rebinds the cloud every later distance / clip refers to
        V = laplace_basis(cur, basis_dtype)
        lfc, hfc = bands(cur, V, low_pass)
        lfc = lfc.detach().clone().requires_grad_()
        hfc = hfc.detach().clone()
        opt = torch.optim.Adam([lfc], lr=lr, weight_decay=0)
        for _ in range(epochs):
            adv = lfc + hfc
            logits = logits_of(model(adv))
            lfc_logits = logits_of(model(lfc))
            # record first, on the iterate that was just evaluated
            pred = torch.argmax(logits, dim=1).cpu().numpy()
            lfc_pred = torch.argmax(lfc_logits, dim=1).cpu().numpy()
            dist = torch.amax(torch.abs(adv - cur), dim=(1, 2)).detach().cpu().numpy()
            adv_np = adv.detach().cpu().numpy().copy()
            iter_adv.append(adv_np), iter_lfc.append(lfc.detach().cpu().numpy().copy()), dists.append(dist.copy())
            mar_adv.append(margins(logits, label).cpu().numpy()), mar_lfc.append(margins(lfc_logits, label).cpu().numpy())
            for e in range(B):
                if pred[e] != label_np[e] and dist[e] < o_bestdist[e] and lfc_pred[e] != label_np[e]:
                    o_bestdist[e], o_bestscore[e], o_bestattack[e] = dist[e], pred[e], adv_np[e]
            loss = 0.5 * untargeted_margin_loss(logits, label, kappa) + 0.5 * untargeted_margin_loss(lfc_logits, label, kappa)
            opt.zero_grad()
            loss.backward()
            opt.step()
            with torch.no_grad():
                clipped = clip_points(lfc + hfc, cur, budget)
                new_lfc, new_hfc = bands(clipped, V, low_pass)
                hfc.data = new_hfc
                lfc.data = new_lfc
    # a cloud that never succeeded is the ZERO cloud clipped towards the last noisy cloud
    adv_pc = clip_points(torch.tensor(o_bestattack).to(cur), cur, budget)
    with torch.no_grad():
        preds = torch.argmax(logits_of(model(adv_pc)), dim=-1)
        trans_preds = torch.argmax(logits_of(trans_model(adv_pc)), dim=-1)
        shuf = shuffled_rows(adv_pc.transpose(2, 1).float()).transpose(2, 1).to(dtype)
        shuffle_preds = torch.argmax(logits_of(model(shuf)), dim=-1)
        shuffle_trans_preds = torch.argmax(logits_of(trans_model(shuf)), dim=-1)
    host = lambda t: t.cpu().numpy()
    st = lambda a, dt: np.stack(a).astype(dt) if a else np.zeros((0,), dtype=dt)
    return dict(o_bestdist=o_bestdist, o_bestscore=o_bestscore, o_bestattack=o_bestattack, data_last=host(cur),
                preds=host(preds), trans_preds=host(trans_preds), shuffle_preds=host(shuffle_preds),
                shuffle_trans_preds=host(shuffle_trans_preds), at_num=float((preds != label).sum().item()),
                trans_num=float((trans_preds != label).sum().item()),
                best_pc=host(adv_pc.transpose(1, 2).contiguous()), iter_adv=st(iter_adv, host(adv_pc).dtype),
                iter_lfc=st(iter_lfc, host(adv_pc).dtype), dist=st(dists, host(adv_pc).dtype),
                margin_adv=st(mar_adv, np.float64), margin_lfc=st(mar_lfc, np.float64))
