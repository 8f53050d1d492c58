"""The point-dropping defence heads (defense.py, csrc/defense.hip) at B = 32, K = 1024 / 2048 / 4096, k = 2, npoint = K:
us per call of SOR forward and forward + backward — the two-launch form (search + select) and the fused per-cloud launch,
replayed from hipGraphs and called eagerly — and of the SRS device draw (draw + counter + gather); beside each SOR figure
the same call through the plain-torch restatement of the reference's algorithm (float64 expansion matrix, topk,
per-sample mask loop; tests/test_defense_cpu.RestatedSOR) on the same GPU. Then ms per iteration of CW (autograd path,
fused=False) on PointNet, on Defended(PointNet, SORDefense) — the victim behind the head replayed from hipGraphs, and
launched eagerly — and on Defended(PointNet, restatement) at B = 32, K = 1024.
Every figure is taken after ~150 ms of the same work (the clocks ramp under load). Writes profiles/defense_bench.json.
Usage: python tools/bench_defense.py [--out FILE] [--iters N]"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from test_defense_cpu import RestatedSOR, outlier_cloud  # noqa: E402

M = importlib.import_module
dev = torch.device("cuda:0")
dfn = M("3dpointcloudattack_amd.defense")
seeded_state_dict = M("3dpointcloudattack_amd.seeding").seeded_state_dict


def ramp(fn, seconds=0.15):
    t_end = time.perf_counter() + seconds
    while time.perf_counter() < t_end:
        fn()
        torch.cuda.synchronize()


def eager_us(fn, reps=50):
    ramp(fn)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def graph_us(fn, reps=10, rounds=20):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    ramp(g.replay)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(rounds):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (reps * rounds)


def heads(B, K):
    rng = np.random.default_rng(K)
    x = torch.from_numpy(np.stack([outlier_cloud(rng, K) for _ in range(B)])).to(dev).transpose(1, 2).contiguous()
    x.requires_grad_()
    G = torch.rand((B, 3, K), device=dev) + 0.5
    row = dict(B=B, K=K, k=2, alpha=1.1, npoint=K)

    def fwd(head):
        return lambda: head(x.detach())

    def fwd_bwd(head):
        return lambda: torch.autograd.grad((head(x) * G).sum(), x)

    for name, fused in (("two_launch", False), ("fused", True)):
        head = dfn.SORDefense(npoint=K)
        head.fused = fused
        row[f"sor_{name}_fwd_us"] = round(graph_us(fwd(head)), 1)
        row[f"sor_{name}_fwd_bwd_us"] = round(graph_us(fwd_bwd(head)), 1)
        row[f"sor_{name}_fwd_eager_us"] = round(eager_us(fwd(head)), 1)
        row[f"sor_{name}_fwd_bwd_eager_us"] = round(eager_us(fwd_bwd(head)), 1)
    ref = RestatedSOR(2, 1.1, K)
    row["sor_torch_fwd_us"] = round(eager_us(fwd(ref), reps=10), 1)
    row["sor_torch_fwd_bwd_us"] = round(eager_us(fwd_bwd(ref), reps=10), 1)
    best = min(row["sor_two_launch_fwd_us"], row["sor_fused_fwd_us"])
    row["sor_fwd_speedup_vs_torch"] = round(row["sor_torch_fwd_us"] / best, 1)
    row["sor_fwd_bwd_speedup_vs_torch"] = round(row["sor_torch_fwd_bwd_us"] / min(row["sor_two_launch_fwd_bwd_us"],
                                                                                     row["sor_fused_fwd_bwd_us"]), 1)
    srs = dfn.SRSDefense(drop_num=500, device_rng=True, seed=1).to(dev)
    srs(x)
    row["srs_device_us"] = round(graph_us(lambda: srs(x)), 1)
    row["srs_device_eager_us"] = round(eager_us(lambda: srs(x)), 1)
    host = dfn.SRSDefense(drop_num=500)
    row["srs_host_draw_eager_us"] = round(eager_us(lambda: host(x), reps=10), 1)
    return row


def cw_ms(victim, trans, pcs, labels, iters):
    cwm = M("3dpointcloudattack_amd.attack.CW.CW_attack")
    u = "3dpointcloudattack_amd.attack.CW.CW_utils."
    atk = cwm.CW(victim, trans, adv_func=M(u + "adv_utils").UntargetedLogitsAdvLoss(5.),
                 clip_func=M(u + "clip_utils").ClipPointsLinf(0.18), dist_func=M(u + "dist_utils").ChamferDist(), fused=False)
    torch.manual_seed(0)
    st = atk._begin(pcs, labels)
    atk._begin_binary_step(st)
    run = atk._make_runner(st)
    ramp(run)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "defense_bench.json"))
    ap.add_argument("--iters", type=int, default=100)
    a = ap.parse_args()
    res = dict(device=torch.cuda.get_device_name(0), heads=[heads(32, K) for K in (1024, 2048, 4096)])

    def victim(seed):
        m = M("3dpointcloudattack_amd.model.pointnet").PointNetCls(k=40)
        m.load_state_dict(seeded_state_dict(m, seed))
        return m.to(dev).eval()

    B, K = 32, 1024
    rng = np.random.default_rng(0)
    pcs = torch.from_numpy(np.stack([outlier_cloud(rng, K) for _ in range(B)]))
    model, trans = victim(0), victim(1)
    with torch.no_grad():
        labels = model(pcs.transpose(1, 2).contiguous().to(dev))[0].argmax(1).cpu()
    cw = dict(B=B, K=K, path="autograd (fused=False)")
    cw["undefended_ms"] = round(cw_ms(model, trans, pcs, labels, a.iters), 4)
    cw["defended_sor_ms"] = round(cw_ms(dfn.Defended(model, dfn.SORDefense(npoint=K)), trans, pcs, labels, a.iters), 4)
    cw["defended_sor_eager_victim_ms"] = round(cw_ms(dfn.Defended(model, dfn.SORDefense(npoint=K), graph=False), trans, pcs,
                                                     labels, a.iters), 4)
    cw["defended_torch_sor_ms"] = round(cw_ms(dfn.Defended(model, RestatedSOR(2, 1.1, K)), trans, pcs, labels,
                                              max(10, a.iters // 5)), 4)
    cw["head_cost_ms"] = round(cw["defended_sor_ms"] - cw["undefended_ms"], 4)
    cw["torch_head_cost_ms"] = round(cw["defended_torch_sor_ms"] - cw["undefended_ms"], 4)
    res["cw_pointnet"] = cw
    print(json.dumps(res))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
