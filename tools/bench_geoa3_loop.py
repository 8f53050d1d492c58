"""GeoA3 (attack/GeoA3/GeoA3_attack.py, geoA3_attack) on a PointNet victim: what an iteration of the device loop
(cfg.device_loop = True) costs, its pieces, the autograd path (device_loop = False, unchanged code) in the same process, and
whole 2 x 100 attacks both ways. Shape: B = 32 clouds of N points (1024, then 2048), PointNet with 40 classes (seeded
weights), the default loss mix (CE, two-sided Chamfer 1.0, Hausdorff 0.1, curvature 1.0 on 16 neighbours), Adam, lr 0.01.

  loop_iter_us         one iteration of the device loop, from the attack's own 16-iteration hipGraph; the replays carry the
                       attack thousands of iterations past its end, and the update kernel's cost depends on the cloud, so
                       this figure drifts — loop_iter_wall_ms is the one of a real attack
  victim_us            fused_forward + cls_loss + fused_input_grad alone on the loop's buffers
  kernels_us           the adv -> ori and ori -> adv searches, the self-kNN search (hinted by its own last result) and
                       pc3d_geoa3_update_f32 (in full, without the curvature term, and single-sided without it) stand-alone,
                       replayed on the state a 2 x 16 attack ends in; largest_in_degree: of that state's two edge sets
  loop_iter_wall_ms    (attack with 2 x `--iters` iterations - attack with 2 x 0) / (2 x iters), wall clock, graphs captured
                       before the clock starts; autograd_iter_ms likewise for device_loop = False
  attack_2x100_*_ms    a whole attack, wall clock, both ways, with the number of successes
  launches             library launches per device-loop iteration (counted at the ctypes shim)
Replayed timings start after >= 150 ms of the same work and stop on an event inside the clocked stream; every figure is a
median of repetitions in this one process, with its minimum and maximum (the run-to-run spread a comparison has to beat).
One JSON document on stdout; --json PATH also writes it."""
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

from helpers import hip_pointnet, unit_cloud

M = importlib.import_module
ops = M("3dpointcloudattack_amd.ops")
_lib = M("3dpointcloudattack_amd._lib")
ga = M("3dpointcloudattack_amd.attack.GeoA3.GeoA3_attack")
pointnet = M("3dpointcloudattack_amd.model.pointnet")
dev = torch.device("cuda:0")


def cfg_of(N, steps, **over):
    base = dict(attack_method='untarget', curv_loss_weight=1.0, curv_loss_knn=16, initial_const=10, iter_max_steps=steps,
                binary_max_steps=2, is_partial_var=False, optim='adam', lr=0.01, npoint=N, is_subsample_opt=False,
                eval_num=1, is_pre_jitter_input=False, cls_loss_type='CE', classes=40, confidence=0, dis_loss_type='CD',
                is_cd_single_side=False, dis_loss_weight=1.0, hd_loss_weight=0.1, uniform_loss_weight=0.0,
                is_use_lr_scheduler=False, is_debug=False, is_pro_grad=False, cc_linf=0.0, is_real_offset=False, knn_range=3)
    base.update(over)
    return types.SimpleNamespace(**base)


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


def med(f, n=5):
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


def one_size(victim, B, N, iters, whole):
    rng = np.random.default_rng(0)
    pcs = torch.from_numpy(np.stack([unit_cloud(rng, N) for _ in range(B)]))
    with torch.no_grad():
        label = victim(pcs.transpose(1, 2).contiguous().to(dev))[0].argmax(1).cpu()
    res = {}

    def run(steps, loop, key=None):
        cfg = cfg_of(N, steps, device_loop=loop)

        def f():
            torch.manual_seed(0)
            np.random.seed(0)
            r = ga.geoA3_attack(victim, None, None, None, None, None, pcs, label, cfg, 0, 1)
            assert ga.geoA3_attack.last_path == ("device_loop" if loop else "autograd")
            if key:
                res[key] = r
        return f
    out = {}
    run(16, True)()
    loop = next(lp for lp in victim._geoa3_loop_cache.values() if lp.key[1] == N and lp.graphs is not None)
    s = loop.bufs
    tgt = s["target"]

    def victim_pass():
        logits, ctx = pointnet.fused_forward(victim, s["x"])
        _, _, _, g = ops.cls_loss(logits, tgt, 3, 0.0, scale=1.0 / B, pred_out=s["pred"])
        return pointnet.fused_input_grad(ctx, g)
    with torch.no_grad():
        names = count_launches(loop.body)
        out["launches"] = {"loop_iteration": len(names), "beside_the_victim": names[-4:]}
        cur = torch.cuda.current_stream(dev)
        out["loop_iter_us"] = med(lambda: replay_us(lambda: loop.graphs.replay(16), 16, 20, cur))
        out["victim_us"] = med(lambda: graph_us(victim_pass))
    # The replays above carried the attack thousands of iterations on. The stand-alone kernels are timed on the state a
    # 2 x 16 attack ends in, with lr = 0 so that the update kernel leaves the iterate where it is (its cost depends on the
    # cloud: the owner of a point sorts that point's incoming edges, and the largest in-degree sets the workgroup's time)
    run(16, True)()
    with torch.no_grad():
        s["lr"].zero_()
        gx = torch.randn(B, 3, N, device=dev) * 1e-3
        cls = torch.zeros(B, device=dev)

        def update(**kw):
            a = dict(nn_ao=s["ao_i"], nn_oa=s["oa_i"], knn_idx=s["knn_i"], normal_ori=s["normal"], kappa_ori=s["kappa_ori"],
                     gval=1.0 / B, w_dis=1.0, w_hd=0.1, w_curv=1.0)
            a.update(kw)
            return lambda: ops.geoa3_update(s["x"], s["ori"], s["offset"], gx, s["m"], s["v"], s["step"], s["search"], s["lr"],
                                            s["scale"], cls, s["pred"], s["target"], False, s["constrain"], s["loss_rows"],
                                            s["best_loss"], s["best_attack"], s["best_bs"], s["best_step"], s["iter_best_loss"],
                                            s["iter_best_score"], **a)
        out["kernels_us"] = {
            "nn_search_adv_ori": med(lambda: graph_us(lambda: ops.nn_search_into(s["x"], s["ori"], s["ao_d"], s["ao_i"]))),
            "nn_search_ori_adv": med(lambda: graph_us(lambda: ops.nn_search_into(s["ori"], s["x"], s["oa_d"], s["oa_i"]))),
            "knn_search_hinted": med(lambda: graph_us(lambda: ops.knn_search_into(s["x"], s["knn_d"], s["knn_i"]))),
            "geoa3_update": med(lambda: graph_us(update())),
            "geoa3_update_without_curvature": med(lambda: graph_us(update(w_curv=0.0))),
            "geoa3_update_single_sided_without_curvature": med(lambda: graph_us(update(w_curv=0.0, nn_oa=None)))}
        out["largest_in_degree"] = {
            "curvature_edges": int(max(int(torch.bincount(s["knn_i"][b, :, 1:].reshape(-1).long(), minlength=N).max()) for b in range(B))),
            "ori_adv_edges": int(max(int(torch.bincount(s["oa_i"][b].long(), minlength=N).max()) for b in range(B)))}
    for name, loop in (("loop", True), ("autograd", False)):
        w0, w1 = wall_ms(run(0, loop)), wall_ms(run(iters, loop))
        out[f"{name}_attack_2x0_ms"], out[f"{name}_attack_2x{iters}_ms"] = w0, w1
        out["loop_iter_wall_ms" if loop else "autograd_iter_ms"] = (w1["median"] - w0["median"]) / (2 * iters)
        out[f"{name}_iter_spread_ms"] = ((w1["max"] - w1["min"]) + (w0["max"] - w0["min"])) / (2 * iters)
    gain = out["autograd_iter_ms"] - out["loop_iter_wall_ms"]
    out["loop_faster_than_autograd_beyond_spread"] = bool(gain > out["loop_iter_spread_ms"] + out["autograd_iter_spread_ms"])
    if whole:
        for name, loop in (("loop", True), ("autograd", False)):
            out[f"attack_2x{whole}_{name}_ms"] = wall_ms(run(whole, loop, key=name), n=3)
        out["attack_outcome"] = {n: {"success": int(np.asarray(r[2]).sum())} for n, r in res.items()}
        out["attack_best_step_equal"] = bool(res["loop"][3] == res["autograd"][3])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 2048])
    ap.add_argument("--iters", type=int, default=48, help="iterations per search step of the per-iteration wall-clock comparisons")
    ap.add_argument("--whole", type=int, default=100, help="iterations per search step of the whole attacks (0: none)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    victim, _ = hip_pointnet(0, dev)
    out = {"what": "tools/bench_geoa3_loop.py on one MI355X, one process; iteration and kernel timings from replayed hipGraphs "
                   "after 150 ms of the same work, whole attacks by wall clock",
           "shape": {"B": a.B, "victim": "PointNetCls(k=40)", "loss": "CE + CD 1.0 (two-sided) + HD 0.1 + curvature 1.0 (k=16)",
                     "lr": 0.01, "binary_max_steps": 2}}
    for N in a.sizes:
        out[f"N{N}"] = one_size(victim, a.B, N, a.iters, a.whole)
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
