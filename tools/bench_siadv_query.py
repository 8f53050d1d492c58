"""SI-Adv's query attacks (attack/SIadv: simba, ours) on the GPU: what a step of the batched loop costs beside the target's
forward, and whole attacks against the plain-torch restatement run ONE CLOUD AT A TIME on the same GPU, which is how the
reference runs them. Shape: B = 32 clouds of N = 1024 points on an ellipsoid, PointNet with 40 classes (seeded weights 3 /
4) as surrogate and target, eps 0.16, step_size 0.32.

  step_us            one step of the fast path (the fused forward of the 2B candidate clouds, log-softmax,
                     pc3d_query_step_f32), replayed from a hipGraph, coordinate mode and frame mode
  forward_us         the fused forward of 2B clouds + log-softmax alone, same timing; step_own_cost_us is the difference
  kernels_us         pc3d_query_step_f32 (both modes) and pc3d_si_rank_f32 stand-alone, replayed
  launches           library launches per step and of the forward alone (counted at the ctypes shim)
  simba / ours       the whole attack, wall clock (first call: with the capture; then the median of 3), its query_costs,
                     and the restatement (tests/siadv_query_restatement.py with oracle/ref_torch's PointNetCls) on the
                     first --baseline-clouds clouds one at a time with the same tables; one_at_a_time_ms_per_cloud is
                     its mean, speedup the batch's per-cloud time against it
Replayed timings start after >= 150 ms of the same work. One JSON document on stdout; --json PATH also writes it."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

import siadv_query_restatement as Q
from bench_siadv import graph_us, med
from helpers import hip_pointnet, oracle_pointnet
from test_siadv_gpu import ellipsoid

M = importlib.import_module
ops = M("3dpointcloudattack_amd.ops")
_lib = M("3dpointcloudattack_amd._lib")
si = M("3dpointcloudattack_amd.attack.SIadv.SIadv_attack")
pointnet = M("3dpointcloudattack_amd.model.pointnet")
dev = torch.device("cuda:0")
EPS, STEP = 0.16, 0.32


def wall_ms(fn, n=3):
    torch.cuda.synchronize()
    t = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    first = (time.perf_counter() - t) * 1e3
    v = []
    for _ in range(n):
        t = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        v.append((time.perf_counter() - t) * 1e3)
    return dict(first_call=first, median=statistics.median(v), min=min(v), max=max(v)), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--N", type=int, default=1024)
    ap.add_argument("--baseline-clouds", type=int, default=2)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    B, N = a.B, a.N
    sur, tgt = hip_pointnet(3, dev)[0], hip_pointnet(4, dev)[0]
    P, _ = ellipsoid(B, N, 0)
    points = P.to(dev)
    x = points.transpose(1, 2).contiguous()
    with torch.no_grad():
        label = tgt(x)[0].argmax(1)

    def attack(method):
        args = types.SimpleNamespace(eps=EPS, step_size=STEP, max_steps=1, num_class=40, top5_attack=False, defense_method=None,
                                     transfer_attack_method=None, query_attack_method=method)
        return si.PointCloudAttack(args, wb_classifier=sur, classifier=tgt)

    out = {"what": "tools/bench_siadv_query.py on one MI355X, one process; step and kernel timings from replayed hipGraphs after "
                   "150 ms of the same work, whole attacks by wall clock",
           "shape": {"B": B, "N": N, "eps": EPS, "step_size": STEP, "victim": "PointNetCls(k=40)", "poll_every": si.POLL}}
    simba, ours = attack("simba"), attack("ours")
    np.random.seed(0)
    tab_simba = torch.from_numpy(si.draw_simba_tables(N, np.ones(B, bool))).to(dev)
    nrm, order, dirs, _ = ours.query_sensitivity(x, label)
    logp0 = tgt(x)[0].detach()
    eps = torch.tensor(si.sign_order(STEP), dtype=torch.float32)
    loops = {}
    for name, atk, tab, fr in (("coordinate", simba, tab_simba, None), ("frame", ours, order, (nrm, dirs))):
        c = si._QueryLoop(atk.classifier, atk.pre_head, atk.top5_attack, B, N, tab.shape[1], 40, dev, fr is not None, False, True)
        c.load(x, label, tab, eps.to(dev), torch.ones(B, dtype=torch.bool, device=dev), label.to(torch.int32), logp0,
               *(fr if fr else ()))
        loops[name] = c
    names, real = [], _lib.call

    def counted(name, *args_):
        names.append(name)
        return real(name, *args_)

    def forward():
        return torch.log_softmax(pointnet.fused_forward(tgt, loops["coordinate"].bufs["cand"])[0], dim=1)

    def hold(c):                       # a step that decides nothing new: the clouds stay live, the timing is a live step's
        c.bufs["pos"].zero_(), c.bufs["done"].zero_(), c.bufs["best"].fill_(-999.)
        c.step()
    _lib.call = counted
    try:
        forward()
        n_fwd = len(names)
        del names[:]
        loops["coordinate"].step()
        out["launches"] = {"forward": n_fwd, "step": len(names), "beside_the_forward": names[n_fwd:]}
    finally:
        _lib.call = real
    out["forward_us"] = med(lambda: graph_us(forward))
    out["step_us"] = {k: med(lambda c=c: graph_us(lambda: hold(c))) for k, c in loops.items()}
    out["step_own_cost_us"] = {k: v["median"] - out["forward_us"]["median"] for k, v in out["step_us"].items()}
    lp = torch.cat([logp0, logp0]).contiguous()
    g = torch.randn(B, 3, N, device=dev)
    out["kernels_us"] = {f"query_step_{k}": med(lambda c=c: graph_us(lambda: ops.query_step(c.bufs, lp))) for k, c in loops.items()}
    out["kernels_us"]["si_rank"] = med(lambda: graph_us(lambda: ops.si_rank(g, nrm)))

    plain_s, plain_t = oracle_pointnet(3)[0].to(dev).eval(), oracle_pointnet(4)[0].to(dev).eval()
    nb = min(a.baseline_clouds, B)
    for name, atk in (("simba", simba), ("ours", ours)):
        if name == "simba":
            t, (adv, adv_target, costs) = wall_ms(lambda: atk.simba_attack(points, label, table=tab_simba))
        else:
            t, (adv, adv_target, costs) = wall_ms(lambda: atk.shape_invariant_query_attack(points, label, table=(nrm, order, dirs)))
        rec = {"batched_ms": t, "query_costs": {"min": int(costs.min()), "median": float(costs.float().median()), "max": int(costs.max())},
               "misclassified": int((adv_target != label).sum())}
        per, same = [], 0
        for b in range(nb):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if name == "simba":
                q = Q.run_query(plain_t, points[b:b + 1], label[b:b + 1], tab_simba[b:b + 1], eps.to(dev))
            else:
                fr = (nrm[b:b + 1].transpose(1, 2).contiguous(), dirs[b:b + 1])
                q = Q.run_query(plain_t, points[b:b + 1], label[b:b + 1], order[b:b + 1], eps.to(dev), frame=fr)
            torch.cuda.synchronize()
            per.append((time.perf_counter() - t0) * 1e3)
            same += int(int(q["query_costs"][0]) == int(costs[b]))
        rec["one_at_a_time_ms_per_cloud"] = {"clouds": nb, "mean": statistics.mean(per), "min": min(per), "max": max(per),
                                             "same_query_costs_as_the_batch": same}
        rec["speedup_per_cloud"] = statistics.mean(per) / (t["median"] / B)
        out[name] = rec
    doc = json.dumps(out, indent=1)
    print(doc)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
