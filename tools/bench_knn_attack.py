"""The kNN attack (attack/KNN/KNN_attack.py, CWKNN) on a PointNet victim: what an iteration of the device loop
(device_loop=True) costs beside the victim's passes, the direct path (device_loop=False) in the same process, and whole
attacks. Shape: B = 32 clouds of N points (1024, then 2048 and 4096), PointNet with 40 classes (seeded weights),
UntargetedLogitsAdvLoss(15), ChamferkNNDist(), ProjectInnerClipLinf(0.18), lr 1e-3.

  loop_iter_us         one iteration of the device loop, from the attack's own 16-iteration hipGraph
  victim_us            fused_attack_grad alone on the loop's buffers (the same loss kind and scale, so the same cotangent);
                       own_cost_us is the difference
  kernels_us           the self-kNN search (hinted by its own last result), the adv -> ori search and
                       pc3d_knn_attack_update_f32 stand-alone, replayed
  direct_iter_ms       (attack with `--iters` iterations - attack with none) / iters for device_loop=False, wall clock;
                       loop_iter_wall_ms likewise for the device loop (its graph captured before the clock starts)
  attack_2500_*_ms     a whole attack() at the default 2500 iterations, wall clock, both ways (first call of the device
                       loop: with its capture)
  launches             library launches per device-loop iteration and of the victim's passes alone (counted at the ctypes shim)
Replayed timings start after >= 150 ms of the same work and stop on an event inside the clocked stream; every figure is a
median of repetitions in this one process. One JSON document on stdout; --json PATH also writes it."""
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

from helpers import hip_pointnet, unit_cloud

M = importlib.import_module
ops = M("3dpointcloudattack_amd.ops")
_lib = M("3dpointcloudattack_amd._lib")
knn = M("3dpointcloudattack_amd.attack.KNN.KNN_attack")
adv_utils = M("3dpointcloudattack_amd.attack.CW.CW_utils.adv_utils")
dist_utils = M("3dpointcloudattack_amd.attack.CW.CW_utils.dist_utils")
clip_utils = M("3dpointcloudattack_amd.attack.CW.CW_utils.clip_utils")
dev = torch.device("cuda:0")
KAPPA, BUDGET, LR = 15.0, 0.18, 1e-3


def graph_us(fn, per=10, reps=30):
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        fn()
        side.synchronize()
        with torch.cuda.graph(g, stream=side):
            for _ in range(per):
                fn()
        return replay_us(g.replay, per, reps, side)


def replay_us(replay, per, reps, stream):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.15:                   # the same work, before the clock starts
        for _ in range(5):
            replay()
        stream.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(reps):
        replay()
    e1.record(stream)
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


def one_size(victim, B, N, iters, whole, parts):
    rng = np.random.default_rng(0)
    pcs = torch.from_numpy(np.stack([unit_cloud(rng, N) for _ in range(B)]))
    with torch.no_grad():
        label = victim(pcs.transpose(1, 2).contiguous().to(dev))[0].argmax(1).cpu()

    def make(num_iter, **kw):
        return knn.CWKNN(victim, None, None, None, None, None, adv_func=adv_utils.UntargetedLogitsAdvLoss(KAPPA),
                         dist_func=dist_utils.ChamferkNNDist(), clip_func=clip_utils.ProjectInnerClipLinf(BUDGET),
                         attack_lr=LR, num_iter=num_iter, device=dev, **kw)

    def run(atk):
        def f():
            torch.manual_seed(0)
            np.random.seed(0)
            return atk.attack(pcs, label)
        return f
    out = {}
    atk = make(16, device_loop=True)
    run(atk)()
    assert atk.last_path == "device_loop"
    loop = next(iter(atk._loop_cache.values()))
    c = loop.bufs
    plan = c["plan"]
    kind, kappa = plan["kind"]

    def victim_pass():
        plan["victim"].fused_attack_grad(c["adv"], c["target"], kind, kappa, pred_out=c["pred"], step=c["step"], scale=plan["scale"])
    with torch.no_grad():
        names = count_launches(loop.body)
        out["launches"] = {"loop_iteration": len(names), "victim_passes": len(count_launches(victim_pass)),
                           "beside_the_victim": names[-3:]}
        cur = torch.cuda.current_stream(dev)
        out["loop_iter_us"] = med(lambda: replay_us(lambda: loop.graphs.replay(16), 16, 20, cur))
        out["victim_us"] = med(lambda: graph_us(victim_pass))
        out["own_cost_us"] = out["loop_iter_us"]["median"] - out["victim_us"]["median"]
        if parts:
            gx = torch.randn(B, 3, N, device=dev) * 1e-3
            one = torch.ones(1, dtype=torch.int32, device=dev)
            out["kernels_us"] = {
                "knn_search_hinted": med(lambda: graph_us(lambda: ops.knn_search_into(c["adv"], c["knn_d"], c["knn_idx"]))),
                "nn_search": med(lambda: graph_us(lambda: ops.nn_search_into(c["adv"], c["ori"], c["nn_d"], c["nn_idx"]))),
                "knn_attack_update": med(lambda: graph_us(lambda: ops.knn_attack_update(
                    c["adv"], c["ori"], gx, c["m"], c["v"], one, LR, c["knn_d"], c["knn_idx"], c["nn_idx"], plan["c_ch"],
                    plan["c_knn"], plan["alpha"], plan["budget"], plan["clip_mode"], c["normal"])))}
    # per iteration by wall clock, both ways
    for name, kw in (("loop", dict(device_loop=True)), ("direct", dict(device_loop=False))):
        a0, a1 = make(0, **kw), make(iters, **kw)
        w0, w1 = wall_ms(run(a0)), wall_ms(run(a1))
        out[f"{name}_attack_0_ms"], out[f"{name}_attack_{iters}_ms"] = w0, w1
        out["loop_iter_wall_ms" if name == "loop" else "direct_iter_ms"] = (w1["median"] - w0["median"]) / iters
    out["loop_faster_than_direct"] = bool(out["loop_iter_wall_ms"] < out["direct_iter_ms"])
    if whole:
        res = {}
        for name, kw in (("loop", dict(device_loop=True)), ("direct", dict(device_loop=False))):
            f = run(make(whole, **kw))
            out[f"attack_{whole}_{name}_ms"] = wall_ms(lambda: res.__setitem__(name, f()), n=2)
        out["attack_outcome"] = {n: {"success_num": r[1]} for n, r in res.items()}
        out["attack_max_abs_diff"] = float(np.abs(res["loop"][0] - res["direct"][0]).max())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 2048, 4096])
    ap.add_argument("--iters", type=int, default=200, help="iterations of the per-iteration wall-clock comparisons")
    ap.add_argument("--whole", type=int, default=2500, help="iterations of the whole attacks (0: none)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    victim, _ = hip_pointnet(0, dev)
    out = {"what": "tools/bench_knn_attack.py on one MI355X, one process; iteration and kernel timings from replayed hipGraphs "
                   "after 150 ms of the same work, whole attacks by wall clock",
           "shape": {"B": a.B, "kappa": KAPPA, "budget": BUDGET, "lr": LR, "victim": "PointNetCls(k=40)",
                     "dist_func": "ChamferkNNDist()", "clip_func": "ProjectInnerClipLinf(0.18)"}}
    for i, N in enumerate(a.sizes):
        out[f"N{N}"] = one_size(victim, a.B, N, a.iters, a.whole, parts=True)
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
