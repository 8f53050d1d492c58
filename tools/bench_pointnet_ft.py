"""The feature-transform PointNet victim on the GPU (B = 32, N = 1024 by default), all in ONE process:

1. fused_attack_grad per step for feature_transform True and False (the yardstick: three towers against two), alternated
   in rounds inside replayed hipGraphs, with the launches per step counted at the library boundary;
2. the plain-torch restatement (tests/pointnet_ft_restatement.py) forward + autograd on the same GPU;
3. the CW iteration (bench.py's settings) on the feature-transform victim and on the plain one.
Timing: a graph of `per` calls is replayed for >= 150 ms first, then HIP events bracket `reps` more replays.
--kernels-only runs the feature-transform step a few times and exits: the run to put under
`rocprofv3 --kernel-trace --stats` (no counters in that run) for the new kernels' own times.
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

import bench
import pointnet_ft_restatement as rst

M = importlib.import_module
ops = M("3dpointcloudattack_amd.ops")
_lib = M("3dpointcloudattack_amd._lib")
dev = torch.device("cuda:0")
PEAK_F32_MFMA_TFLOPS = 157.3        # MI355X, fp32 matrix (vendor figure)


def graph_us(fn, per=10, reps=30, warm_ms=150.0):
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        fn()
        side.synchronize()
        with torch.cuda.graph(g, stream=side):
            for _ in range(per):
                fn()
        t0 = time.perf_counter()
        while (time.perf_counter() - t0) * 1e3 < warm_ms:       # >= 150 ms of the same replays before the timing
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


def victim(ft, seed):
    m = M("3dpointcloudattack_amd.model.pointnet").PointNetCls(k=bench.NCLS, feature_transform=ft)
    m.load_state_dict(M("3dpointcloudattack_amd.seeding").seeded_state_dict(m, seed))
    return m.to(dev).eval()


def count_launches(fn):
    names, real = [], _lib.call

    def counted(name, *a):
        names.append(name)
        return real(name, *a)
    _lib.call = counted
    try:
        fn()
    finally:
        _lib.call = real
    return names


def tower_flops(B, N):
    """Shape-derived FLOPs per launch: the trunk 3->64->128->1024, STNkd's tower with its extra 64->64 layer."""
    l3 = 2.0 * B * N * 128 * 1024
    trunk = 2.0 * B * N * (3 * 64 + 64 * 128) + l3
    return {"trunk": trunk, "stnkd_tower": trunk + 2.0 * B * N * 64 * 64, "layer3": l3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--npts", type=int, default=bench.NPTS)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    B, N = args.batch, args.npts
    rng = np.random.default_rng(1235)
    data = torch.from_numpy(np.stack([bench.unit_cloud(rng, N) for _ in range(B)]))
    x = data.transpose(1, 2).contiguous().to(dev)
    models = {ft: victim(ft, 0) for ft in (True, False)}
    with torch.no_grad():
        tgt = {ft: m(x)[0].argmax(1) for ft, m in models.items()}
    steps = {ft: (lambda ft=ft: models[ft].fused_attack_grad(x, tgt[ft], "untargeted_logits", bench.KAPPA)) for ft in models}
    if args.kernels_only:
        for _ in range(20):
            steps[True]()
        torch.cuda.synchronize()
        return
    res = {"B": B, "N": N, "lib": _lib.LIB_PATH, "tower_flops_per_launch": tower_flops(B, N),
           "peak_f32_mfma_tflops": PEAK_F32_MFMA_TFLOPS}
    times = {ft: [] for ft in models}
    for _ in range(args.rounds):
        for ft in (True, False):
            times[ft].append(graph_us(steps[ft]))
    res["fused_attack_grad_us"] = {
        ("feature_transform" if ft else "plain"): {"us": t, "median": statistics.median(t), "min_max_spread": max(t) - min(t),
                                                    "launches": len(count_launches(steps[ft])),
                                                    "launch_names": count_launches(steps[ft])}
        for ft, t in times.items()}
    res["ratio_ft_over_plain"] = statistics.median(times[True]) / statistics.median(times[False])

    sd = models[True].state_dict()

    def restated():
        xa = x.clone().requires_grad_()
        logp = rst.forward(sd, xa)[0]
        M("3dpointcloudattack_amd.attack.CW.CW_utils.adv_utils").UntargetedLogitsAdvLoss(bench.KAPPA)(logp, tgt[True]).mean().backward()
        return xa.grad
    for _ in range(3):
        restated()
    torch.cuda.synchronize()
    t = []
    for _ in range(args.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            restated()
        e1.record()
        e1.synchronize()
        t.append(e0.elapsed_time(e1) / 10 * 1e3)
    res["restatement_autograd_us"] = {"us": t, "median": statistics.median(t)}

    CW = M("3dpointcloudattack_amd.attack.CW.CW_attack").CW
    adv_utils, dist_utils, clip_utils = (M(f"3dpointcloudattack_amd.attack.CW.CW_utils.{n}") for n in
                                         ("adv_utils", "dist_utils", "clip_utils"))
    runs = {}
    for ft in (True, False):
        trans_model = victim(ft, 1)
        with torch.no_grad():
            labels = models[ft](x)[0].argmax(1).cpu()
        atk = CW(models[ft], trans_model, adv_func=adv_utils.UntargetedLogitsAdvLoss(kappa=bench.KAPPA),
                 clip_func=clip_utils.ClipPointsLinf(budget=bench.BUDGET), dist_func=dist_utils.ChamferDist(),
                 attack_lr=bench.LR, binary_step=10, num_iter=500, device=dev)
        torch.manual_seed(1000)
        st = atk._begin(data, labels)
        atk._begin_binary_step(st)
        runs[ft] = atk._make_runner(st)
    it = {ft: [] for ft in runs}
    for _ in range(args.rounds):
        for ft, run in runs.items():
            for i in range(40):
                run(i)
            run.flush()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.steps):
                run(i)
            run.flush()
            torch.cuda.synchronize()
            it[ft].append((time.perf_counter() - t0) * 1e3 / args.steps)
    res["cw_iteration_ms"] = {("feature_transform" if ft else "plain"): {"ms_per_step": t, "median": statistics.median(t),
                                                                        "min_max_spread": max(t) - min(t)}
                              for ft, t in it.items()}
    print(json.dumps(res))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
