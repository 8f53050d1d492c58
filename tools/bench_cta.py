"""The critical-point attack (attack/CTA) on the GPU: what a step costs beside the victim's passes, the batched
integrated-gradients pass against sequential single-set passes, and a whole attack against the plain-torch restatement run
one set at a time on the same GPU. Shape: G = 16 sets of S = 2 clouds (B = 32) of N = 1024 points, PointNet with 40
classes (seeded weights), Adam, untargeted, alpha 1e-4.

  step_fused_us      one step of the fused loop (fused_forward, pc3d_cta_cotangent_f32, fused_input_grad,
                     pc3d_cta_update_f32), replayed from a hipGraph
  victim_us          the victim's fused forward + backward alone, fed the loop's own cotangent precomputed at the same
                     iterate (like for like), same timing; step_own_cost_us is the difference
  kernels_us         pc3d_cta_cotangent_f32 and pc3d_cta_update_f32 stand-alone, replayed; pc3d_ig_steps_f32 and
                     pc3d_ig_reduce_f64 for one set at 50 steps
  ig_batched_ms      saliency() of the G sets at steps = 50: one victim pass of all steps x B clouds per set
  ig_sequential_ms   the generic path (autograd) one step at a time, 50 passes per set, for the G sets
  attack_ms          cta_attack on the G sets, wall clock (first call: with the capture; then the median)
  attack_restated_ms tests/cta_restatement.py::run with oracle/ref_torch's PointNetCls on the same GPU, one set after the
                     other, on the first --restated-sets sets: the reference's algorithm in plain torch, timed once;
                     attack_same_sets_ms is cta_attack on those sets
  launches           library launches per fused step and of the victim's passes alone (counted at the ctypes shim)
Replayed timings start after >= 150 ms of the same work; every figure is a median of repetitions in this one process.
One JSON document on stdout; --json PATH also writes it."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import cta_restatement as R
from helpers import hip_pointnet, oracle_pointnet

M = importlib.import_module
ops = M("3dpointcloudattack_amd.ops")
_lib = M("3dpointcloudattack_amd._lib")
pointnet = M("3dpointcloudattack_amd.model.pointnet")
cta = M("3dpointcloudattack_amd.attack.CTA.CTA")
dev = torch.device("cuda:0")
ALPHA, IG_STEPS = 1e-4, 50


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


def wall_ms(fn, n=3):
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
    return dict(first_call=first, median=statistics.median(v), min=min(v), max=max(v))


def count_launches(fn):
    seen = []
    real = _lib.call

    def counting(name, *a):
        seen.append(name)
        return real(name, *a)
    _lib.call = counting
    try:
        fn()
    finally:
        _lib.call = real
    return seen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--G", type=int, default=16)
    ap.add_argument("--S", type=int, default=2)
    ap.add_argument("--N", type=int, default=1024)
    ap.add_argument("--restated-sets", type=int, default=4)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    G, S, N = a.G, a.S, a.N
    victim, _ = hip_pointnet(0, dev)
    rng = np.random.default_rng(0)
    pts = rng.standard_normal((G, S, 3, N)).astype(np.float32)
    pts /= np.linalg.norm(pts, axis=2, keepdims=True).max(axis=3, keepdims=True)
    sets = torch.from_numpy(pts).to(dev)
    with torch.no_grad():
        ori = [int(victim(sets[g])[0][0].argmax()) for g in range(G)]
    out = {"what": "tools/bench_cta.py on one MI355X, one process; step and kernel timings from replayed hipGraphs after 150 ms "
                   "of the same work, whole passes and attacks by wall clock",
           "shape": {"G": G, "S": S, "B": G * S, "N": N, "ig_steps": IG_STEPS, "alpha": ALPHA, "optimizer": "Adam",
                     "victim": "PointNetCls(k=40)"}}

    # one step and its parts
    res = cta.cta_attack(victim, sets, ori, alpha=ALPHA, IG_steps=2, graph=False, return_info=True)
    loop = res[4]["loop"]
    s = loop.s
    s["poll"].zero_()                                             # every set live at level 0: nothing is unmasked, no set latches
    x = s["x"]
    logits = pointnet.fused_forward(victim, x)[0]
    loop_g = ops.cta_cotangent(logits, s).clone()                 # the loop's own cotangent at this iterate, precomputed
    gl = torch.empty_like(logits)

    def victim_passes():
        ctx = pointnet.fused_forward(victim, x)[1]
        pointnet.fused_input_grad(ctx, loop_g)
    gx = torch.randn_like(x) * 1e-3
    out["launches"] = {"victim_passes": len(count_launches(victim_passes)), "fused_step": len(count_launches(loop.step)),
                       "beside_the_victim": ["pc3d_cta_cotangent_f32", "pc3d_cta_update_f32"]}
    keep = {k: s[k].clone() for k in ("x", "v", "s_adam", "poll")}

    def rewind():
        for k, v in keep.items():
            s[k].copy_(v)
    out["step_fused_us"] = med(lambda: graph_us(loop.step))
    rewind()
    out["victim_us"] = med(lambda: graph_us(victim_passes))
    out["step_own_cost_us"] = out["step_fused_us"]["median"] - out["victim_us"]["median"]
    out["kernels_us"] = {"cta_cotangent": med(lambda: graph_us(lambda: ops.cta_cotangent(logits, s, out=gl))),
                         "cta_update": med(lambda: graph_us(lambda: ops.cta_update(s, gx)))}
    al = torch.from_numpy(np.linspace(0, 1, IG_STEPS)).to(dev)
    clouds, base = ops.ig_steps(sets[0], al)
    grads = torch.randn_like(clouds)
    out["kernels_us"]["ig_steps_one_set"] = med(lambda: graph_us(lambda: ops.ig_steps(sets[0], al)))
    out["kernels_us"]["ig_reduce_one_set"] = med(lambda: graph_us(lambda: ops.ig_reduce(grads, sets[0], base)))
    rewind()

    # the saliency pass
    out["ig_batched_ms"] = wall_ms(lambda: cta.saliency(victim, sets, ori, IG_STEPS))

    def ig_sequential():
        alphas = np.linspace(0, 1, IG_STEPS)
        for g in range(G):
            clouds, _ = ops.ig_steps(sets[g], alphas)
            for st in range(IG_STEPS):
                cta.input_gradients(victim, clouds[st * S:(st + 1) * S], S, ori[g], fused=False)
    out["ig_sequential_ms"] = wall_ms(ig_sequential)
    out["ig_speedup"] = out["ig_sequential_ms"]["median"] / out["ig_batched_ms"]["median"]

    # a whole attack
    runs = []

    def attack():
        runs.append(cta.cta_attack(victim, sets, ori, alpha=ALPHA, IG_steps=IG_STEPS, return_info=True))
    out["attack_ms"] = wall_ms(attack)
    info = runs[-1][4]
    out["attack_outcome"] = {"states": runs[-1][0], "steps": info["steps"], "num_p_per": info["num_p_per"]}
    # the restatement, one set at a time, on the first R sets; the device loop on the same sets for the ratio
    Rn = min(a.restated_sets, G)
    out["attack_same_sets_ms"] = wall_ms(lambda: cta.cta_attack(victim, sets[:Rn], ori[:Rn], alpha=ALPHA, IG_steps=IG_STEPS))
    onet, _ = oracle_pointnet(0)
    onet = onet.to(dev)
    fwd = R.hooked_forward(onet, onet.fc3)
    rest = []
    torch.cuda.synchronize()
    t = time.perf_counter()
    for g in range(Rn):
        rest.append(R.run(fwd, sets[g], ori[g], torch.tensor(ALPHA, device=dev), IG_steps=IG_STEPS))
    torch.cuda.synchronize()
    out["attack_restated_ms"] = {"sets": Rn, "once": (time.perf_counter() - t) * 1e3}
    out["restated_outcome"] = {"states": [str(r["state"]) for r in rest], "steps": [r["steps"] for r in rest]}
    out["attack_speedup_same_sets"] = out["attack_restated_ms"]["once"] / out["attack_same_sets_ms"]["median"]
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.json:
        with open(a.json, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
