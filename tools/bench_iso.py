"""The isometry attack (attack/ISO) on the GPU: what a CTRI step costs beside the victim, and the whole attack against its
plain-torch restatement. Shape: B = 32 clouds of N = 1024 points, PointNet with 40 classes (seeded weights).

  step_fast_us      one CTRI step on the fast path (victim's fused passes + pc3d_iso_update_f32), replayed from a hipGraph
  victim_us         the victim's fused forward + backward alone, same timing: the attack's own cost is the difference
  step_generic_us   one CTRI step on the generic path (IsoTransform + autograd + iso_update with gW). Autograd's backward is
                    host-driven, so this one is timed eagerly (events around `reps` steps), not from a replayed graph
  kernels_us        pc3d_iso_apply_f32 / pc3d_iso_wgrad_f32 / pc3d_iso_update_f32 stand-alone, replayed
  attack_ms         a whole ISOAttack.attack with defaults, wall clock (first call: with the graph capture; second: without)
  restated_ms       tests/test_iso_cpu.py::RestatedISO with the same victim on the same GPU: the reference's algorithm at the
                    reference's granularity (eager autograd, host-side stop test), tsi_batch = 1 as the product's default
Timings start after ~1 s of replayed steps (clock ramp). The step timings use step_size = 0 so that no cloud stops while
the clock runs (a stopped cloud skips the weight gradient). One JSON document on stdout; --json PATH also writes it."""
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
from test_iso_cpu import RestatedISO

M = importlib.import_module
ops = M("3dpointcloudattack_amd.ops")
iso = M("3dpointcloudattack_amd.attack.ISO.iso_attack")
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


def eager_us(fn, reps=200):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def med(f, n=3):
    v = [f() for _ in range(n)]
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--N", type=int, default=1024)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    B, N = a.B, a.N
    victim, _ = hip_pointnet(0, dev)
    rng = np.random.default_rng(0)
    x = torch.from_numpy(np.stack([unit_cloud(rng, N) for _ in range(B)]).transpose(0, 2, 1).copy()).to(dev)
    with torch.no_grad():
        label = victim(x)[0].argmax(1)
    eye = torch.eye(3, device=dev).repeat(B, 1, 1)
    out = {"shape": {"B": B, "N": N, "victim": "PointNetCls(k=40)"}}

    fast = iso._Ctri(victim, B, N, dev, True, 0, 0.0, 0.0)
    fast.load(x, label, eye)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 1.0:                      # clock ramp
        for _ in range(50):
            fast.step()
        torch.cuda.synchronize()
    out["step_fast_us"] = med(lambda: graph_us(fast.step))
    out["victim_us"] = med(lambda: graph_us(lambda: victim.fused_loss_and_grad(fast.xo, label, 0, 0.0, scale=1.0)))
    out["attack_own_cost_us"] = out["step_fast_us"]["median"] - out["victim_us"]["median"]
    gen = iso._Ctri(victim, B, N, dev, False, 0, 0.0, 0.0)
    gen.load(x, label, eye)
    out["step_generic_us"] = dict(med(lambda: eager_us(gen.step)), timing="eager (autograd's backward is host-driven)")
    g = torch.randn(B, 3, N, device=dev)
    xo = torch.empty_like(x)
    st = iso._Ctri(victim, B, N, dev, True, 0, 0.0, 0.0)
    st.load(x, label, eye)
    row = torch.randn(B, 40, device=dev)
    st.kept_out = torch.zeros_like(row)
    out["kernels_us"] = {
        "iso_apply": med(lambda: graph_us(lambda: ops.iso_apply(x, eye, out=xo))),
        "iso_wgrad": med(lambda: graph_us(lambda: ops.iso_wgrad(g, x))),
        "iso_update": med(lambda: graph_us(lambda: ops.iso_update(x, st.xo, st.W, st.m, st.v, label, label, row, st.done, st.steps,
                                                                    st.kept_out, st.kept_pred, 0.0, g=g))),
    }

    def whole(cls, **kw):
        np.random.seed(0), torch.manual_seed(0)
        atk = cls(victim, **kw)
        ts = []
        for _ in range(2):
            torch.cuda.synchronize()
            t = time.perf_counter()
            _, _, info = atk.attack(x, label)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t) * 1e3)
        steps = np.asarray(info["steps"])
        return dict(first_call_ms=ts[0], second_call_ms=ts[1], clouds_in_ctri=int((steps > 0).sum()),
                    init_success=int(np.asarray(info["init_success"]).sum()), tsi_draws=int(np.asarray(info["tsi_draws"]).sum()))
    out["attack_ms"] = whole(iso.ISOAttack)
    out["attack_tsi_batch_B_ms"] = whole(iso.ISOAttack, tsi_batch=B)
    out["restated_ms"] = whole(RestatedISO)
    out["restated_over_attack"] = out["restated_ms"]["second_call_ms"] / out["attack_ms"]["second_call_ms"]
    out["note"] = ("the two calls of a whole attack draw different rotations (the posterior and numpy's generator move on), so "
                   "clouds_in_ctri / tsi_draws are those of the second call; TSI is host-driven in both implementations")
    doc = json.dumps(out, indent=1)
    print(doc)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
