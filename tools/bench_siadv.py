"""The shape-invariant attack (attack/SIadv) on the GPU: what a step costs beside the surrogate's passes, and the loop
against its plain-torch restatement on the same GPU. Shape: B = 32 clouds of N = 1024 points on an ellipsoid with their
normals, PointNet with 40 classes (seeded weights) as surrogate and target, eps 0.16, step_size 0.07, max_steps 50.

  step_fast_us       one step of the fast path (search, pc3d_si_frame_f32, the surrogate's fused passes, pc3d_si_step_f32),
                     replayed from a hipGraph
  victim_us          the surrogate's fused forward + backward alone, same timing; step_own_cost_us is the difference
  kernels_us         the search (K = 20), pc3d_pca_normal_f32, pc3d_si_frame_f32 (idx mode), pc3d_si_step_f32 (nrm mode and
                     idx mode) stand-alone, replayed
  loop_fast_ms       PointCloudAttack.iterate, 50 steps, wall clock (first call: with the capture; then the median of 5)
  loop_generic_ms    the same on the generic path (autograd for dL/dP; host-driven, so wall clock is the fair timing)
  loop_restated_ms   tests/siadv_restatement.py::run_loop with oracle/ref_torch's PointNetCls on the same GPU: the
                     reference's algorithm in plain torch (autograd, cdist-style search, batched `eigh` for the normals)
  launches           library launches per fast step and of the surrogate's passes alone (counted at the ctypes shim)
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
import numpy as np
import torch

import siadv_restatement as R
from helpers import hip_pointnet, oracle_pointnet
from test_siadv_gpu import ellipsoid

M = importlib.import_module
ops = M("3dpointcloudattack_amd.ops")
_lib = M("3dpointcloudattack_amd._lib")
si = M("3dpointcloudattack_amd.attack.SIadv.SIadv_attack")
dev = torch.device("cuda:0")
EPS, STEP, STEPS = 0.16, 0.07, 50


def graph_us(fn, per=20, reps=50):
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        fn()
        side.synchronize()
        with torch.cuda.graph(g, stream=side):
            for _ in range(per):
                fn()
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.15:                   # the same work, before the clock starts
            for _ in range(5):
                g.replay()
            side.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(side)
        for _ in range(reps):
            g.replay()
        e1.record(side)
        e1.synchronize()
    return e0.elapsed_time(e1) / (per * reps) * 1e3


def med(f, n=3):
    v = [f() for _ in range(n)]
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def wall_ms(fn, n=5):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    first = (time.perf_counter() - t) * 1e3
    v = []
    for _ in range(n):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        v.append((time.perf_counter() - t) * 1e3)
    return dict(first_call=first, median=statistics.median(v), min=min(v), max=max(v), per_step_us=statistics.median(v) / STEPS * 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--N", type=int, default=1024)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    B, N = a.B, a.N
    victim, _ = hip_pointnet(3, dev)
    P, nrm = ellipsoid(B, N, 0)
    points = torch.cat([P, nrm], -1).to(dev)
    with torch.no_grad():
        label = victim(points[:, :, :3].transpose(1, 2).contiguous())[0].argmax(1)
    args = types.SimpleNamespace(eps=EPS, step_size=STEP, max_steps=STEPS, num_class=40, top5_attack=False, defense_method=None,
                                 transfer_attack_method="ifgm_ours", query_attack_method=None)
    out = {"what": "tools/bench_siadv.py on one MI355X, one process; step and kernel timings from replayed hipGraphs after 150 ms "
                   "of the same work, whole loops by wall clock",
           "shape": {"B": B, "N": N, "max_steps": STEPS, "eps": EPS, "step_size": STEP, "victim": "PointNetCls(k=40)"}}

    x = points[:, :, :3].transpose(1, 2).contiguous()
    loop = si._Loop(victim, B, N, dev, STEP, EPS)
    loop.load(x, x, label)
    loop.first(nrm.to(dev).transpose(1, 2).contiguous())
    loop.step()
    names, real = [], _lib.call

    def counted(name, *args_):
        names.append(name)
        return real(name, *args_)
    _lib.call = counted
    try:
        victim.fused_attack_grad(loop.xe, label, "untargeted_logits", 0.0, scale=1.0)
        n_victim = len(names)
        del names[:]
        loop.step()
        out["launches"] = {"victim_passes": n_victim, "fast_step": len(names), "beside_the_victim": [n for n in names if "si_" in n or "knn" in n]}
    finally:
        _lib.call = real

    out["step_fast_us"] = med(lambda: graph_us(loop.step))
    out["victim_us"] = med(lambda: graph_us(lambda: victim.fused_attack_grad(loop.xe, label, "untargeted_logits", 0.0, scale=1.0)))
    out["step_own_cost_us"] = out["step_fast_us"]["median"] - out["victim_us"]["median"]
    g = torch.randn(B, 3, N, device=dev)
    idx = ops.knn_raw(loop.x, loop.x, 20, q_cf=True, r_cf=True)[1]
    xs, xe, nb = loop.x.clone(), torch.empty_like(x), torch.empty_like(x)
    ops.si_frame(xs, idx=idx, out=xe, nrm_out=nb)
    out["kernels_us"] = {
        "knn_k20": med(lambda: graph_us(lambda: ops.knn_raw(xs, xs, 20, q_cf=True, r_cf=True))),
        "pca_normal": med(lambda: graph_us(lambda: ops.pca_normal(xs, idx, cf=True))),
        "si_frame_idx": med(lambda: graph_us(lambda: ops.si_frame(xs, idx=idx, out=xe, nrm_out=nb))),
        "si_step_nrm": med(lambda: graph_us(lambda: ops.si_step(xs, x, g, STEP, EPS, nrm=nb))),
        "si_step_idx": med(lambda: graph_us(lambda: ops.si_step(xs, x, g, STEP, EPS, idx=idx))),
    }

    fast = si.PointCloudAttack(args, wb_classifier=victim, classifier=victim)
    generic = si.PointCloudAttack(args, wb_classifier=victim, classifier=victim, fused=False)
    out["loop_fast_ms"] = wall_ms(lambda: fast.iterate(points, label))
    out["loop_generic_ms"] = wall_ms(lambda: generic.iterate(points, label))
    plain = oracle_pointnet(3)
    plain = (plain[0] if isinstance(plain, tuple) else plain).to(dev).eval()
    for p in plain.parameters():
        p.requires_grad_(False)
    out["loop_restated_ms"] = wall_ms(lambda: R.run_loop(plain, points, label, EPS, STEP, STEPS), n=3)
    out["restated_over_fast"] = out["loop_restated_ms"]["median"] / out["loop_fast_ms"]["median"]
    out["generic_over_fast"] = out["loop_generic_ms"]["median"] / out["loop_fast_ms"]["median"]
    # agreement with the restatement, cloud by cloud: a trajectory of this attack is not stable under rounding (one ulp of
    # noise in the victim moves an arg-max of its max-pool, the normalised step carries that to the clamp), so clouds
    # leave the restatement's run one by one; tests/golden/make_golden_siadv.py measures the same of the reference itself
    agree = {}
    for k in (1, 2, 5):
        d = (fast.iterate(points, label, steps=k).transpose(1, 2) - R.run_loop(plain, points, label, EPS, STEP, k)).abs().amax((1, 2))
        agree[f"after_{k}"] = {"clouds_within_1e-3": int((d <= 1e-3).sum()), "of": B, "median_deviation": float(d.median())}
    out["fast_vs_restated"] = agree
    dfast = fast.iterate(points, label).transpose(1, 2)
    out["finite_and_in_box_after_50"] = bool(torch.isfinite(dfast).all() and float((dfast - points[:, :, :3]).abs().max()) <= EPS + 1e-6)
    doc = json.dumps(out, indent=1)
    print(doc)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
