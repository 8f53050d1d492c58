#!/usr/bin/env python3
"""Generate tests/golden/gen3dadv.npz: short runs of the REAL reference's point-adding attacks on the CPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_gen3dadv.py

B = 1 (the reference's prints / .item() calls need it), seeded PointNet weights, small sizes (K = 256, A = 64, clusters
3 x 16). Cases: CWAdd with Chamfer untargeted, Hausdorff untargeted, Chamfer targeted; CWAddClusters with FarChamfer.
Stored per case: the cloud and target, the critical-point scores and the indices the reference picked, the DBSCAN
labels and the initial clusters (CWAddClusters), every iterate (recorded through the dist_func the loop calls on it),
o_bestdist, the returned cloud, success_num and the fail counters.

The order of tied critical-point scores is unspecified for torch.topk; here torch.topk is made a stable descending sort
(ties to the lower index, the rule the mirror documents), as canonical_unsorted_topk does for CurveNet. Only data is
written — no reference source is copied.
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, _seeded_pointnet, install_cpu_shim, unit_cloud  # noqa: E402

SEED = 1000


def stable_topk(log):
    """torch.topk as a stable descending sort (ties to the lower index); calls on [B,K] scores are logged."""
    _orig_sort = torch.sort

    def topk(input, k, dim=-1, largest=True, sorted=True, **kw):
        vals, idx = _orig_sort(input, dim=dim, descending=largest, stable=True)
        vals, idx = vals.narrow(dim, 0, k), idx.narrow(dim, 0, k)
        log.append((input.detach().numpy().copy(), idx.numpy().copy()))
        return vals, idx
    torch.topk = topk
    torch.Tensor.topk = lambda self, k, dim=-1, largest=True, sorted=True: topk(self, k, dim, largest, sorted)


class Recorder(torch.nn.Module):
    """The loop calls dist_func(adv [B,A,3], ori [B,K,3], batch_avg=False) once per iteration for its bookkeeping,
    then again with the weights for the loss: the first call of every iteration logs the iterate as [B,3,A]."""

    def __init__(self, inner):
        super().__init__()
        self.inner, self.log = inner, []

    def forward(self, adv, ori, weights=None, batch_avg=True):
        if weights is None:
            self.log.append(adv.detach().numpy().transpose(0, 2, 1).copy())
        return self.inner(adv, ori, weights=weights, batch_avg=batch_avg)


def main():
    install_cpu_shim()
    topk_log = []
    stable_topk(topk_log)
    from model.pointnet import PointNetCls
    from attack.Gen3DAdv import IndpAdd_attack, ClusterAdd_attack
    from attack.Gen3DAdv.utils.adv_utils import UntargetedLogitsAdvLoss, LogitsAdvLoss
    from attack.Gen3DAdv.utils.dist_utils import ChamferDist, HausdorffDist, FarChamferDist

    db_log = []
    _DB = ClusterAdd_attack.DBSCAN

    class LoggedDBSCAN(_DB):
        def fit_predict(self, X, y=None, sample_weight=None):
            lab = super().fit_predict(X, y, sample_weight=sample_weight)
            db_log.append((np.asarray(X).copy(), lab.copy()))
            return lab
    ClusterAdd_attack.DBSCAN = LoggedDBSCAN

    model, sha = _seeded_pointnet(PointNetCls, 40, 0)
    trans_model, _ = _seeded_pointnet(PointNetCls, 40, 1)
    fx = {"sha256": np.array(sha)}
    cases = {
        "chamfer_untarget": dict(kind="add", dist="chamfer", method="untarget", kappa=0., w=(5e2, 4e3), seed=11),
        "hausdorff_untarget": dict(kind="add", dist="hausdorff", method="untarget", kappa=5., w=(2e2, 9e2), seed=12),
        "chamfer_target": dict(kind="add", dist="chamfer", method="target", kappa=0., w=(5e2, 4e3), seed=13),
        "clusters": dict(kind="cluster", dist="far", method="untarget", kappa=0., w=(0.05, 0.3), seed=14),
    }
    K, A, NC, P = 256, 64, 3, 16
    steps, iters = 3, 25
    fx["names"] = np.array(sorted(cases))
    for nm in sorted(cases):
        c = cases[nm]
        rng = np.random.default_rng(c["seed"])
        pc = unit_cloud(rng, K)[None]                                        # [1,K,3]
        x = torch.from_numpy(pc).transpose(1, 2).contiguous()
        with torch.no_grad():
            logits = model(x)[0]
        tgt = int(torch.argmax(logits, 1)) if c["method"] == "untarget" else int(_orig_topk2(logits)[0, 1])
        adv_func = UntargetedLogitsAdvLoss(kappa=c["kappa"]) if c["method"] == "untarget" else LogitsAdvLoss(kappa=c["kappa"])
        if c["dist"] == "far":
            rec = Recorder(FarChamferDist(NC, 'adv2ori', 0.1))
            atk = ClusterAdd_attack.CWAddClusters(model, trans_model, adv_func, rec, attack_lr=1e-2, init_weight=c["w"][0],
                                                  max_weight=c["w"][1], binary_step=steps, num_iter=iters, num_add=NC,
                                                  cl_num_p=P, attack_method=c["method"])
            inits = []
            _ic = atk._init_centers
            atk._init_centers = lambda pcs, lab: (lambda r: (inits.append(r.copy()), r)[1])(_ic(pcs, lab))
        else:
            rec = Recorder(ChamferDist('adv2ori') if c["dist"] == "chamfer" else HausdorffDist('adv2ori'))
            atk = IndpAdd_attack.CWAdd(model, trans_model, adv_func, rec, attack_lr=1e-2, init_weight=c["w"][0],
                                       max_weight=c["w"][1], binary_step=steps, num_iter=iters, num_add=A,
                                       attack_method=c["method"])
        topk_log.clear()
        db_log.clear()
        torch.manual_seed(SEED)
        np.random.seed(SEED)
        with contextlib.redirect_stdout(io.StringIO()):
            bd, ba, sn = atk.attack(torch.from_numpy(pc), torch.tensor([tgt]))
        scores, idx = next((s, i) for s, i in topk_log if s.shape == (1, K))
        fx[f"{nm}_pc"], fx[f"{nm}_target"] = pc, np.array([tgt])
        fx[f"{nm}_cfg"] = np.array([steps, iters, c["kappa"], c["w"][0], c["w"][1]])
        fx[f"{nm}_scores"], fx[f"{nm}_idx"] = scores.astype(np.float32), idx.astype(np.int64)
        fx[f"{nm}_bestdist"], fx[f"{nm}_bestattack"], fx[f"{nm}_success"] = bd, ba, np.array(sn)
        fx[f"{nm}_traj"] = np.stack(rec.log).astype(np.float32)[:, 0]         # [steps*iters, 3, A]
        if c["kind"] == "cluster":
            fx[f"{nm}_dbscan_points"], fx[f"{nm}_dbscan_labels"] = db_log[0]
            fx[f"{nm}_init"] = inits[0].astype(np.float32)                    # [1, NC, P, 3]
            counts = np.bincount(db_log[0][1][db_log[0][1] >= 0])
            print(nm, "cluster sizes", counts.tolist())
        else:
            fx[f"{nm}_fails"] = np.array([atk.attack_fail, atk.shuffle_fail, atk.trans_fail])
        print(nm, "bestdist", bd, "success", sn, flush=True)
    np.savez_compressed(os.path.join(OUT, "gen3dadv.npz"), **fx)
    print("gen3dadv.npz:", len(fx), "arrays")


_ORIG_TOPK = torch.topk


def _orig_topk2(logits):
    return _ORIG_TOPK(logits, 2, dim=1)[1]


if __name__ == "__main__":
    main()
