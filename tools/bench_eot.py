"""The additional-experiments CW (attack/additional_exp/CW_attack.py) with EOT + renormalisation + z-only box on a PointNet
victim: what an iteration of the device loop (device_loop=True) costs, against the autograd path (device_loop=False) in the
same process, with and without resampling. Shapes: B = 1, K = 4000 (the reference driver's, Test_CW.py) and B = 32,
K = 1024; PointNet with 40 classes (seeded weights), LogitsAdvLoss(0), PerSampleDist(ChamferDist()), lr 1e-2.

  iter_wall_ms         (attack with `--iters` iterations - attack with none) / iters by wall clock around a device
                       synchronise, device loop and autograd path alternating, median of repetitions (the loop's graph is
                       captured before the clock starts). This includes the host's draws.
  loop_gpu_us          one iteration of the device loop from its own 16-iteration hipGraph, device events: the chain alone
  victim_stacked_us    fused_attack_grad on the stacked [(1+10) B,3,K] input alone; nn_search_us, eot_prepare_us and
                       eot_update_us: the other three launches alone
  launches             library launches of one device-loop iteration (counted at the ctypes shim; the loop has no others)
  draw_block_ms        host time of one block's draws (16 iterations x 10 views: rotations, and with resampling
                       random.sample + the inverse table), and host_share: the draws' share of the device-loop attack's wall
                       time (CW.draw_seconds / wall)
  loop_rng_*           the device loop with device_rng=True (the tables drawn by pc3d_eot_draw_f32 in front of every block of
                       16 iterations), timed alternately with the two others in the same windows: iter_wall_ms as above,
                       speedup_over_host_draws = loop / loop_rng, loop_rng_gpu_us = (one draw launch + the 16-iteration
                       graph) / 16 by device events, draw_seconds = CW.draw_seconds (0: the host draws nothing)
  device_draws         per shape: the loop_rng iteration with resampling, the host-draw loop without (the chain's speed), the
                       gap between them and the draw launch's own time / 16
  draw_launch_us       pc3d_eot_draw_f32 alone for cnt = 16 rows, E = 10 views, per K, rotations + indices + inverse
Replayed timings start after >= 150 ms of the same work and stop on an event inside the clocked stream. One JSON document
on stdout; --json PATH also writes it."""
import argparse
import importlib
import json
import os
import random
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
cwm = M("3dpointcloudattack_amd.attack.additional_exp.CW_attack")
adv_utils = M("3dpointcloudattack_amd.attack.CW.CW_utils.adv_utils")
dist_utils = M("3dpointcloudattack_amd.attack.CW.CW_utils.dist_utils")
dev = torch.device("cuda:0")
LR = 1e-2
DRAW_SEED = 2000             # device_rng=True's seed


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


def med(f, n=3):
    v = [f() for _ in range(n)]
    return dict(median=statistics.median(v), min=min(v), max=max(v))


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


def one_config(victim, B, K, iters, resample, reps):
    rng = np.random.default_rng(0)
    pcs = torch.from_numpy(np.stack([unit_cloud(rng, K) for _ in range(B)]))
    with torch.no_grad():
        lg = victim(pcs.transpose(1, 2).contiguous().to(dev))[0]
    tgt, org = lg.topk(2, dim=1)[1][:, 1].cpu(), lg.argmax(1).cpu()

    def make(num_iter, name):
        return cwm.CW(victim, cwm.AdvLossAdapter(adv_utils.LogitsAdvLoss(0.), adv_utils.UntargetedLogitsAdvLoss(0.)),
                      cwm.PerSampleDist(dist_utils.ChamferDist()), attack_lr=LR, binary_step=1, num_iter=num_iter,
                      whether_target=True, whether_1d=True, whether_renormalization=True, whether_3Dtransform=True,
                      whether_resample=resample, device=dev, device_loop=name != "autograd", device_rng=name == "loop_rng",
                      seed=DRAW_SEED)

    def wall(atk):
        torch.manual_seed(0)
        random.seed(0)
        torch.cuda.synchronize()
        t = time.perf_counter()
        res = atk.attack(pcs, tgt, org)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, res

    out = {}
    paths = ("loop", "autograd", "loop_rng")
    atks = {(name, n): make(n, name) for name in paths for n in (0, iters)}
    for a in atks.values():                                  # warm-up: captures, code objects, the library's algorithms
        wall(a)
    assert atks[("loop", iters)].last_path == "device_loop" and atks[("autograd", iters)].last_path == "autograd"
    assert atks[("loop", iters)].last_draws == "host" and atks[("loop_rng", iters)].last_draws == "device"
    times = {k: [] for k in atks}
    shares, res, rng_draw_seconds = [], {}, []
    for _ in range(reps):                                    # alternating
        for k, a in atks.items():
            ms, r = wall(a)
            times[k].append(ms)
            res[k[0]] = r
            if k == ("loop", iters):
                shares.append(a.draw_seconds * 1e3 / ms)
            if k == ("loop_rng", iters):
                rng_draw_seconds.append(a.draw_seconds)
    for name in paths:
        per = [(t1 - t0) / iters for t0, t1 in zip(times[(name, 0)], times[(name, iters)])]
        out[f"{name}_iter_wall_ms"] = dict(median=statistics.median(per), min=min(per), max=max(per))
        out[f"{name}_attack_{iters}_ms"] = statistics.median(times[(name, iters)])
    out["speedup_wall"] = out["autograd_iter_wall_ms"]["median"] / out["loop_iter_wall_ms"]["median"]
    out["host_share_of_loop_attack"] = statistics.median(shares)
    out["max_abs_diff_of_results"] = float(np.abs(res["loop"][1] - res["autograd"][1]).max())
    out["loop_rng_speedup_over_host_draws"] = out["loop_iter_wall_ms"]["median"] / out["loop_rng_iter_wall_ms"]["median"]
    out["loop_rng_draw_seconds"] = max(rng_draw_seconds)

    atk = atks[("loop", iters)]
    loop = next(iter(atk._loop_cache.values()))
    c = loop.bufs
    plan = c["plan"]
    kind, kappa = plan["kind"]
    cur = torch.cuda.current_stream(dev)

    def victim_pass():
        plan["victim"].fused_attack_grad(c["X"], c["goal_s"], kind, kappa, pred_out=c["pred"], step=c["step"], scale=plan["scale"])
    with torch.no_grad():
        names = count_launches(loop.body)
        out["launches"] = {"loop_iteration": len(names), "victim_passes": len(count_launches(victim_pass)),
                           "beside_the_victim": [n for n in names if n.startswith("pc3d_eot") or n == "pc3d_nn_f32"]}
        out["loop_gpu_us"] = med(lambda: replay_us(lambda: loop.graphs.replay(16), 16, 10, cur))

        def block_with_draws():                              # what device_rng=True enqueues per block of 16 iterations
            ops.eot_draw(DRAW_SEED, 0, (0, 16), c["rot"], c["idx"], c["inv"])
            loop.graphs.replay(16)
        out["loop_rng_gpu_us"] = med(lambda: replay_us(block_with_draws, 16, 10, cur))
        out["victim_stacked_us"] = med(lambda: graph_us(victim_pass))
        gx = torch.randn_like(c["X"]) * 1e-3
        one = torch.ones(1, dtype=torch.int32, device=dev)
        out["eot_prepare_us"] = med(lambda: graph_us(lambda: ops.eot_prepare(
            c["adv"], c["ori"], c["rot"], c["idx"], plan["renorm"], one, out=c["X"], stats=c["stats"], arg=c["arg"])))
        out["nn_search_us"] = med(lambda: graph_us(lambda: ops.nn_search_into(c["adv"], c["ori"], c["nn_d"], c["nn_idx"])))
        out["eot_update_us"] = med(lambda: graph_us(lambda: ops.eot_update(
            c["adv"], c["ori"], gx, c["m"], c["v"], one, LR, c["pred"], c["goal"], plan["untarget"], c["bestdist"],
            c["bestscore"], c["o_bestdist"], c["o_bestscore"], c["o_bestattack"], rot=c["rot"], inv=c["inv"],
            renorm=plan["renorm"], stats=c["stats"], arg=c["arg"], input_val=c["input_val"], dist_kind=plan["dist_kind"],
            w=c["w"], nn_idx=c["nn_idx"], batch_mean=B, one_d=plan["one_d"], box=plan["box"])))

    def draw():
        t = time.perf_counter()
        atk._draw_block(c, 0, atk.LOOP_BLOCK, K)
        return (time.perf_counter() - t) * 1e3
    out["draw_block_ms"] = med(draw)
    out["draw_per_iteration_ms"] = out["draw_block_ms"]["median"] / atk.LOOP_BLOCK
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=int, nargs="+", default=[1, 4000, 32, 1024], help="B K pairs")
    ap.add_argument("--iters", type=int, default=48, help="iterations of the wall-clock comparisons (blocks of 16)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    victim, _ = hip_pointnet(0, dev)
    out = {"what": "tools/bench_eot.py on one MI355X, one process; wall-clock per-iteration figures by difference of two "
                   "attacks, chain and kernel timings from replayed hipGraphs after 150 ms of the same work",
           "config": {"lr": LR, "victim": "PointNetCls(k=40)", "dist_func": "PerSampleDist(ChamferDist())", "views": 10,
                      "whether_1d": True, "whether_renormalization": True, "whether_3Dtransform": True, "iters": a.iters}}
    out["draw_launch_us"] = {}
    for K in sorted(set(a.shapes[1::2]) | {1024, 4000, 8192}):
        rot = torch.zeros((16, 10, 3, 3), dtype=torch.float32, device=dev)
        idx = torch.zeros((16, 10, K), dtype=torch.int32, device=dev)
        inv = torch.zeros((16, 10, K, 2), dtype=torch.int32, device=dev)
        out["draw_launch_us"][f"K{K}"] = med(lambda: graph_us(lambda: ops.eot_draw(DRAW_SEED, 0, (0, 16), rot, idx, inv)))
    for B, K in zip(a.shapes[::2], a.shapes[1::2]):
        for resample in (False, True):
            key = f"B{B}_K{K}_{'resample' if resample else 'eot_renorm_1d'}"
            out[key] = one_config(victim, B, K, a.iters, resample, a.reps)
            print(f"{key}: done", file=sys.stderr, flush=True)
    out["device_draws"] = {}
    for B, K in zip(a.shapes[::2], a.shapes[1::2]):
        plain, res = out[f"B{B}_K{K}_eot_renorm_1d"], out[f"B{B}_K{K}_resample"]
        rng_ms, chain_ms = res["loop_rng_iter_wall_ms"]["median"], plain["loop_iter_wall_ms"]["median"]
        out["device_draws"][f"B{B}_K{K}"] = {
            "resample_loop_rng_iter_wall_ms": rng_ms, "resample_host_draw_loop_iter_wall_ms": res["loop_iter_wall_ms"]["median"],
            "no_resample_loop_iter_wall_ms": chain_ms, "gap_to_no_resample_ms": rng_ms - chain_ms,
            "draw_launch_per_iteration_ms": out["draw_launch_us"][f"K{K}"]["median"] / 16 * 1e-3,
            "chain_gpu_us_resample_vs_not": [res["loop_gpu_us"]["median"], plain["loop_gpu_us"]["median"]]}
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
