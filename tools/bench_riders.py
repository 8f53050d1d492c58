"""A/B of the CW iteration's riders (csrc/linear_riders.hip, the update epilogue of csrc/pointmlp.hip) on the GPU.

1. Every host launch with and without its rider, and the last backward with and without its epilogue, inside replayed
   hipGraphs (timing as bench.py::graph_ms: `per` calls per graph, HIP events around `reps` replays).
2. The whole iteration (bench.py's flagship: CW on PointNet, B=32, N=1024) for every choice of pieces — 17 launches,
   search rider only, bookkeeping rider + update epilogue only, all (15 launches) — alternated in rounds in ONE process,
   200 graph-replayed steps per timing; medians and min-max spreads per choice.
One JSON document on stdout; --json PATH also writes it. --dist l2 / --npts N select the other shapes of the sweep."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench

M = importlib.import_module
ops = M("3dpointcloudattack_amd.ops")
dev = torch.device("cuda:0")


def graph_us(fn, per=20, reps=50):
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        fn()
        side.synchronize()
        with torch.cuda.graph(g, stream=side):
            for _ in range(per):
                fn()
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


def launches(B, N):
    """us per call of every host with / without its rider (3 timings each, the median)."""
    torch.manual_seed(0)
    g = lambda *s: torch.randn(*s, device=dev)     # noqa: E731
    ori = torch.rand(B, 3, N, device=dev) - 0.5
    adv = ori + 0.01 * g(B, 3, N)
    pooled_s, w1s, b1s = g(B, 1024), g(512, 1024) / 32, g(512)
    g_c2, w2c_t, c1 = g(B, 256), g(512, 256) / 16, g(B, 512)
    label = torch.randint(0, 40, (B,), device=dev)
    pred = (label + 1) % 40
    f = lambda v: torch.full((B,), v, device=dev)     # noqa: E731
    bestdist, o_bestdist = f(1e10), f(1e10)
    bestscore, o_bestscore = torch.full((B,), -1, device=dev), torch.full((B,), -1, device=dev)
    o_bestattack, input_val, dist_val = torch.zeros_like(adv), torch.zeros_like(adv), torch.zeros(B, device=dev)
    m, v = torch.zeros_like(adv), torch.zeros_like(adv)
    step = torch.ones(1, dtype=torch.int32, device=dev)
    adam, wts = torch.zeros(2, device=dev), f(10.0)
    tw = tuple(t.to(dev) for t in (torch.randn(64, 3), torch.randn(64), torch.randn(128, 64) / 8, torch.randn(128),
                                   torch.randn(1024, 128) / 11, torch.randn(1024)))
    tw = tw + (tw[2].t().contiguous(),)
    pooled, argidx, masks = ops.pointmlp3_max_fwd_raw(adv, tw, True, want_masks=True)
    g_pooled, gx = g(B, 1024) * 1e-2, g(B, 3, N) * 1e-3
    _, nn_idx = ops.nn_raw(adv, ori, True, True)
    book = (pred, label, True, bestdist, bestscore, o_bestdist, o_bestscore, o_bestattack)

    def upd_launch():
        ops.cw_update(adv, ori, *book, gx, m, v, step, 0.01, 0.18, input_val=input_val, dist_val=dist_val, dist_kind=2, w=wts,
                      nn_idx=nn_idx)

    def book_rider(ride):
        ops.linear_book(g_c2, w2c_t, adv, ori, *book, gate=c1, input_val=input_val, dist_val=dist_val, step=step, lr=0.01,
                        adam=adam, ride=ride)

    def bwd_plain():
        ops.pointmlp3_max_bwd_raw(adv, tw, argidx, g_pooled, masks, out=gx, accumulate=True)

    def bwd_update():
        ops.pointmlp3_max_bwd_update(adv, tw, argidx, g_pooled, masks, gx, ori, m, v, adam, 0.18, dist_kind=2, w=wts,
                                     dist_val=dist_val, nn_idx=nn_idx)

    cases = {
        "linear_stn1": lambda: ops.linear(pooled_s, w1s, b1s, relu=True),
        "nn_search": lambda: ops.nn_raw(adv, ori, True, True),
        "linear_stn1+nn_two_launches": lambda: ops.linear_nn(pooled_s, w1s, b1s, relu=True, q=adv, r=ori, q_cf=True, r_cf=True,
                                                               ride=False),
        "linear_stn1+nn_rider": lambda: ops.linear_nn(pooled_s, w1s, b1s, relu=True, q=adv, r=ori, q_cf=True, r_cf=True),
        "linear_cls2_bwd": lambda: ops.linear(g_c2, w2c_t, gate=c1),
        "linear_cls2_bwd+book_two_launches": lambda: book_rider(False),
        "linear_cls2_bwd+book_rider": lambda: book_rider(True),
        "cw_update": upd_launch,
        "stn_bwd": bwd_plain,
        "stn_bwd+update_epilogue": bwd_update,
    }
    book_rider(True)        # the Adam factors the epilogue reads
    out = {}
    for name, fn in cases.items():
        out[name] = statistics.median(graph_us(fn) for _ in range(3))
    return out


def iteration(B, N, dname, rounds, steps, warmup):
    """ms per step of the whole iteration for every choice of riders, alternated `rounds` times."""
    PointNetCls = M("3dpointcloudattack_amd.model.pointnet").PointNetCls
    CW = M("3dpointcloudattack_amd.attack.CW.CW_attack").CW
    adv_utils = M("3dpointcloudattack_amd.attack.CW.CW_utils.adv_utils")
    dist_utils = M("3dpointcloudattack_amd.attack.CW.CW_utils.dist_utils")
    clip_utils = M("3dpointcloudattack_amd.attack.CW.CW_utils.clip_utils")
    model, trans_model = PointNetCls(k=bench.NCLS), PointNetCls(k=bench.NCLS)
    model.load_state_dict(bench.seeded_state(model, 0))
    trans_model.load_state_dict(bench.seeded_state(trans_model, 1))
    model, trans_model = model.to(dev).eval(), trans_model.to(dev).eval()
    rng = np.random.default_rng(1235)
    data = torch.from_numpy(np.stack([bench.unit_cloud(rng, N) for _ in range(B)]))
    with torch.no_grad():
        labels = model(data.transpose(1, 2).contiguous().to(dev))[0].argmax(1).cpu()
    choices = {"17_launches": False, "search_rider_only": {"search"}, "book_rider+update_epilogue_only": {"update"},
               "15_launches": True}
    runs = {}
    for name, riders in choices.items():
        atk = CW(model, trans_model, adv_func=adv_utils.UntargetedLogitsAdvLoss(kappa=bench.KAPPA),
                 clip_func=clip_utils.ClipPointsLinf(budget=bench.BUDGET),
                 dist_func=dist_utils.L2Dist() if dname == "l2" else dist_utils.ChamferDist(),
                 attack_lr=bench.LR, binary_step=10, num_iter=500, device=dev, riders=riders)
        torch.manual_seed(1000)
        st = atk._begin(data, labels)
        atk._begin_binary_step(st)
        runs[name] = (atk._make_runner(st), st)
    times = {name: [] for name in choices}
    for _ in range(rounds):
        for name, (run, _) in runs.items():
            for i in range(warmup):
                run(i)
            run.flush()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(steps):
                run(i)
            run.flush()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / steps)
    # every choice started from the same state and ran the same number of iterations: the same bits
    ref = runs["17_launches"][1]
    same = {name: all(torch.equal(st[k], ref[k]) for k in bench.DUMPED_STATE + ("exp_avg", "exp_avg_sq"))
            for name, (_, st) in runs.items()}
    return {name: {"ms_per_step": t, "median": statistics.median(t), "min_max_spread": max(t) - min(t),
                   "state_equals_17_launches": same[name]} for name, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--npts", type=int, default=bench.NPTS)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--dist", default="chamfer", choices=("chamfer", "l2"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--no-launches", action="store_true")
    ap.add_argument("--no-iteration", action="store_true")
    args = ap.parse_args()
    res = {"B": args.batch, "N": args.npts, "dist": args.dist, "lib": importlib.import_module("3dpointcloudattack_amd._lib").LIB_PATH}
    if not args.no_launches:
        res["launch_us_in_replayed_graphs"] = launches(args.batch, args.npts)
    if not args.no_iteration:
        res["iteration"] = iteration(args.batch, args.npts, args.dist, args.rounds, args.steps, args.warmup)
    print(json.dumps(res))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
