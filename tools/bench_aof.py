"""The untargeted AOF attack (attack/AOF/Eval_AOF.py) on the GPU: what an iteration costs beside the victim's pass, the
fused loop against the generic one and against the plain-torch restatement on the same GPU, and a whole attack. Shape:
B = 32 clouds of N = 1024 points, low_pass 100, PointNet with 40 classes (seeded weights), UntargetedLogitsAdvLoss(30),
ClipPointsLinf(0.18), lr 1e-2.

  fused_iter_us        one iteration of the fused loop (stacked victim pass, pc3d_aof_record_f32, pc3d_aof_update_f32,
                       pc3d_spectral_reproject_sum_f32), replayed from a hipGraph
  victim_stacked_us    fused_loss_and_grad on the loop's own [2B,3,N] buffer alone (the same loss, so the same
                       cotangent), same timing; own_cost_us is the difference
  victim_two_passes_us the same work as two passes of B clouds; stacked_equals_two_passes: the gradients bit for bit
  kernels_us           the three own launches stand-alone, replayed
  generic_iter_ms      (attack with `--epochs` iterations - attack with none) / epochs for the generic path (autograd, the
                       victim's passes replayed through GraphedVictim), step = 1, wall clock; fused_iter_wall_ms and
                       restated_iter_ms likewise for the fused loop and for tests/aof_restatement.py with
                       oracle/ref_torch's PointNetCls on the same GPU; basis_ms is the attack with no iteration (noise,
                       Laplacian, torch.linalg.eigh, first projection, final clip and the four closing forwards)
  attack_2x200_*_ms    AOF.attack with step = 2, epochs = 200, wall clock (first call: with the capture; then the median:
                       the AOF object keeps its graphs, as over the batches of a loader)
  launches             library launches per fused iteration and of the stacked victim pass alone (counted at the ctypes shim)
Replayed timings start after >= 150 ms of the same work; every figure is a median of repetitions in this one process.
One JSON document on stdout; --json PATH also writes it."""
import argparse
import contextlib
import importlib
import io
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

import aof_restatement as R
from helpers import hip_pointnet, oracle_pointnet, unit_cloud

M = importlib.import_module
ops = M("3dpointcloudattack_amd.ops")
_lib = M("3dpointcloudattack_amd._lib")
ea = M("3dpointcloudattack_amd.attack.AOF.Eval_AOF")
adv_utils = M("3dpointcloudattack_amd.attack.CW.CW_utils.adv_utils")
clip_utils = M("3dpointcloudattack_amd.attack.CW.CW_utils.clip_utils")
dev = torch.device("cuda:0")
KAPPA, BUDGET, LR = 30.0, 0.18, 1e-2


def graph_us(fn, per=10, reps=30):
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
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--N", type=int, default=1024)
    ap.add_argument("--low-pass", type=int, default=100)
    ap.add_argument("--epochs", type=int, default=40, help="iterations of the per-iteration wall-clock comparisons")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    B, N, lp = a.B, a.N, a.low_pass
    victim, _ = hip_pointnet(0, dev)
    trans, _ = hip_pointnet(1, dev)
    rng = np.random.default_rng(0)
    pcs = torch.from_numpy(np.stack([unit_cloud(rng, N) for _ in range(B)]))
    with torch.no_grad():
        label = victim(pcs.transpose(1, 2).contiguous().to(dev))[0].argmax(1).cpu()
    out = {"what": "tools/bench_aof.py on one MI355X, one process; iteration and kernel timings from replayed hipGraphs after "
                   "150 ms of the same work, whole attacks by wall clock",
           "shape": {"B": B, "N": N, "low_pass": lp, "kappa": KAPPA, "budget": BUDGET, "lr": LR, "victim": "PointNetCls(k=40)"}}

    def make(**kw):
        return ea.AOF(victim, trans, adv_utils.UntargetedLogitsAdvLoss(KAPPA), clip_utils.ClipPointsLinf(BUDGET), lr=LR,
                      low_pass=lp, device=dev, **kw)

    # one iteration and its parts
    atk = make(step=1, epochs=1)
    ori = pcs.float().to(dev).transpose(1, 2).contiguous()
    lab = label.to(dev)
    fk = atk._fused_kind()
    torch.manual_seed(0)
    loop = atk._fused_loop(B, N, fk)
    fl = st = loop.bufs
    atk._load(fl, ori, lab)
    atk._new_step(fl)
    buf, label2 = fl["buf"], fl["label2"]

    def stacked():
        victim.fused_loss_and_grad(buf, label2, *fk, scale=0.5 / B)

    def two_passes():
        victim.fused_loss_and_grad(buf[:B], lab, *fk, scale=0.5 / B)
        victim.fused_loss_and_grad(buf[B:], lab, *fk, scale=0.5 / B)
    with torch.no_grad():
        g2 = victim.fused_loss_and_grad(buf, label2, *fk, scale=0.5 / B)[3]
        ga = victim.fused_loss_and_grad(buf[:B], lab, *fk, scale=0.5 / B)[3]
        gb = victim.fused_loss_and_grad(buf[B:], lab, *fk, scale=0.5 / B)[3]
        out["stacked_equals_two_passes"] = bool(torch.equal(g2[:B], ga) and torch.equal(g2[B:], gb))
        names = count_launches(loop.body)
        out["launches"] = {"fused_iteration": len(names), "victim_stacked_pass": len(count_launches(stacked)),
                           "beside_the_victim": [n for n in names if "aof" in n or "spectral" in n]}
        ea._begin_step(fl)
        out["fused_iter_us"] = med(lambda: graph_us(loop.body))
        ea._begin_step(fl)
        out["victim_stacked_us"] = med(lambda: graph_us(stacked))
        out["victim_two_passes_us"] = med(lambda: graph_us(two_passes))
        out["own_cost_us"] = out["fused_iter_us"]["median"] - out["victim_stacked_us"]["median"]
        data, hfc, clipped, coeff = fl["data"], torch.randn(B, 3, N, device=dev) * 0.1, torch.empty(B, 3, N, device=dev), torch.empty(B, 3, N, device=dev)
        m, v, step = torch.zeros(B, 3, N, device=dev), torch.zeros(B, 3, N, device=dev), torch.ones(1, dtype=torch.int32, device=dev)
        lfc = buf[B:].clone()
        pred2 = torch.zeros(2 * B, dtype=torch.long, device=dev)
        Vb = torch.linalg.qr(torch.randn(B, N, N, device=dev))[0].contiguous()
        Vtb = Vb.transpose(1, 2).contiguous()
        out["kernels_us"] = {
            "aof_record": med(lambda: graph_us(lambda: ops.aof_record(buf[:B], data, pred2[:B], pred2[B:], lab, st["o_bestdist"],
                                                                     st["o_bestscore"], st["o_bestattack"]))),
            "aof_update": med(lambda: graph_us(lambda: ops.aof_update(lfc, g2[:B], g2[B:], m, v, hfc, data, step, LR, BUDGET, out=clipped))),
            "spectral_reproject_sum": med(lambda: graph_us(lambda: ops.spectral_reproject(data, Vb, Vtb, lp, lfc, hfc, coeff, sum=clipped))),
            "spectral_reproject": med(lambda: graph_us(lambda: ops.spectral_reproject(data, Vb, Vtb, lp, lfc, hfc, coeff)))}

    # per iteration by wall clock: the three loops, step = 1
    E = a.epochs

    def run(atk):
        def f():
            torch.manual_seed(0)
            np.random.seed(0)
            with contextlib.redirect_stdout(io.StringIO()):
                return atk.attack(pcs, label)
        return f
    out["basis_ms"] = wall_ms(run(make(step=1, epochs=0)))
    for name, kw in (("fused", dict(fused=True)), ("generic", dict(fused=False))):
        w = wall_ms(run(make(step=1, epochs=E, **kw)))
        out[f"{name}_attack_1x{E}_ms"] = w
        out[f"{name}_iter_wall_ms" if name == "fused" else "generic_iter_ms"] = (w["median"] - out["basis_ms"]["median"]) / E
    onet, otrans = oracle_pointnet(0)[0].to(dev), oracle_pointnet(1)[0].to(dev)

    def restated(epochs):
        def f():
            torch.manual_seed(0)
            np.random.seed(0)
            return R.run(onet, otrans, pcs.to(dev), label.to(dev), kappa=KAPPA, budget=BUDGET, lr=LR, low_pass=lp, step=1, epochs=epochs)
        return f
    r0 = wall_ms(restated(0), n=1)
    r1 = wall_ms(restated(E), n=1)
    out["restated_basis_ms"], out[f"restated_attack_1x{E}_ms"] = r0, r1
    out["restated_iter_ms"] = (r1["median"] - r0["median"]) / E
    out["fused_faster_than_generic"] = bool(out["fused_iter_wall_ms"] < out["generic_iter_ms"])

    # a whole attack of 2 x 200
    res = {}
    for name, kw in (("fused", dict(fused=True)), ("generic", dict(fused=False))):
        f = run(make(step=2, epochs=200, **kw))
        out[f"attack_2x200_{name}_ms"] = wall_ms(lambda: res.__setitem__(name, f()), n=2 if name == "generic" else 3)
    out["attack_outcome"] = {n: {"found": int((r[0] < 1e9).sum()), "success_num": r[2]} for n, r in res.items()}
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
