"""The low-band spectral basis of AOF (csrc/lowband.hip) against the dense decomposition it replaces, on one GPU, at
B = 32, low_pass = 100, k = 30 and N = 1024, 2048 (--N):

  full_basis_ms       what a binary step of basis="full" computes: dense Laplacian, torch.linalg.eigh, the V^T copy
  lowband_basis_ms    ops.lowband_basis: kNN, CSR Laplacian, the filtered block iteration; `split` gives the CSR build alone,
                      the iteration without outer iterations (start block, two orthonormalisations, one Rayleigh-Ritz), and
                      the cost of the filter steps (the default schedule minus the same schedule with degree 1)
  reproject_us        ops.spectral_reproject (V and V^T) against ops.band_reproject (U), 10 calls per replayed hipGraph
  attack_2x200_ms     CWTAOF.attack with the reference's defaults (2 binary steps of 200 iterations) on a PointNet victim, wall
                      clock, with each basis (first call: with the graph capture; then the median)
The two bases are timed with events around eager calls after a warm-up (torch.linalg.eigh synchronises with the host and
cannot be captured); lowband_basis_graph_ms is ops.lowband_basis_csr replayed from a hipGraph where the capture succeeds.
One JSON document on stdout; --json PATH also writes it."""
import argparse
import contextlib
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
ta = M("3dpointcloudattack_amd.attack.AOF.TAOF_attack")
adv_utils = M("3dpointcloudattack_amd.attack.CW.CW_utils.adv_utils")
dist_utils = M("3dpointcloudattack_amd.attack.CW.CW_utils.dist_utils")
clip_utils = M("3dpointcloudattack_amd.attack.CW.CW_utils.clip_utils")
dev = torch.device("cuda:0")


def eager_ms(fn, n=5):
    fn()
    torch.cuda.synchronize()
    v = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        v.append(e0.elapsed_time(e1))
    return dict(median=statistics.median(v), min=min(v), max=max(v))


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
            g.replay()
            side.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(side)
        for _ in range(reps):
            g.replay()
        e1.record(side)
        e1.synchronize()
    return e0.elapsed_time(e1) / (per * reps) * 1e3


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


@contextlib.contextmanager
def schedule(**kw):
    old = dict(ops.LOWBAND_DEFAULTS)
    ops.LOWBAND_DEFAULTS.update(kw)
    try:
        yield
    finally:
        ops.LOWBAND_DEFAULTS.update(old)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--N", type=int, default=1024)
    ap.add_argument("--low-pass", type=int, default=100)
    ap.add_argument("--no-attack", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    B, N, lp = a.B, a.N, a.low_pass
    rng = np.random.default_rng(0)
    pcs = torch.from_numpy(np.stack([unit_cloud(rng, N) for _ in range(B)]))
    x = pcs.to(dev).transpose(1, 2).contiguous()
    out = {"what": "tools/bench_lowband.py on one MI355X, one process", "shape": {"B": B, "N": N, "low_pass": lp, "k": 30},
           "schedule": dict(ops.LOWBAND_DEFAULTS), "block": ops.lowband_block(N, lp)}

    def full():
        L = ops.graph_laplacian(x, 30, cf=True)
        _, V = torch.linalg.eigh(L)
        return V.contiguous(), V.transpose(2, 1).contiguous()

    out["full_basis_ms"] = eager_ms(full, n=3)
    out["lowband_basis_ms"] = eager_ms(lambda: ops.lowband_basis(x, lp, 30, cf=True))
    csr = ops.graph_laplacian_csr(x, 30, cf=True)
    split = {"csr_build_ms": eager_ms(lambda: ops.graph_laplacian_csr(x, 30, cf=True)),
             "iteration_ms": eager_ms(lambda: ops.lowband_basis_csr(*csr, lp))}
    with schedule(iters=0):
        split["no_outer_iteration_ms"] = eager_ms(lambda: ops.lowband_basis_csr(*csr, lp))
    with schedule(degree=1):
        split["degree_1_ms"] = eager_ms(lambda: ops.lowband_basis_csr(*csr, lp))
    d = ops.LOWBAND_DEFAULTS
    split["filter_steps_ms"] = split["iteration_ms"]["median"] - split["degree_1_ms"]["median"]
    split["per_outer_iteration_without_filter_ms"] = (split["degree_1_ms"]["median"] - split["no_outer_iteration_ms"]["median"]) / d["iters"]
    out["split"] = split
    try:
        out["lowband_basis_graph_ms"] = graph_us(lambda: ops.lowband_basis_csr(*csr, lp), per=2, reps=5) / 1e3
    except Exception as e:      # a capture that the runtime refuses is reported, not fatal
        out["lowband_basis_graph_ms"] = f"not captured: {type(e).__name__}: {str(e)[:200]}"
    print(json.dumps({k: out[k] for k in ("full_basis_ms", "lowband_basis_ms", "split", "lowband_basis_graph_ms")}), file=sys.stderr, flush=True)
    out["lowband_faster_than_full"] = bool(out["lowband_basis_ms"]["median"] < out["full_basis_ms"]["median"])

    # the per-iteration re-projection
    V, Vt = full()
    U, theta, resid = ops.lowband_basis(x, lp, 30, cf=True)
    out["resid_max"] = float(resid.max())
    adv = x + 0.01 * torch.randn_like(x)
    lfc, hfc, co, s = (torch.empty_like(adv) for _ in range(4))
    rp = {"spectral_reproject": statistics.median(graph_us(lambda: ops.spectral_reproject(adv, V, Vt, lp, lfc, hfc, co)) for _ in range(3)),
          "spectral_reproject_sum": statistics.median(graph_us(lambda: ops.spectral_reproject(adv, V, Vt, lp, lfc, hfc, co, sum=s)) for _ in range(3))}
    lf, hf = lfc.clone(), hfc.clone()
    rp["band_reproject"] = statistics.median(graph_us(lambda: ops.band_reproject(adv, U, lfc, hfc)) for _ in range(3))
    rp["band_reproject_sum"] = statistics.median(graph_us(lambda: ops.band_reproject(adv, U, lfc, hfc, sum=s)) for _ in range(3))
    rp["bytes_full"], rp["bytes_band"] = 2 * B * N * N * 4, 2 * B * N * lp * 4
    rp["lfc_max_abs_difference_between_the_bases"] = float((lf - lfc).abs().max())
    out["reproject_us"] = rp
    print(json.dumps(rp), file=sys.stderr, flush=True)
    del V, Vt

    if not a.no_attack:
        victim, _ = hip_pointnet(0, dev)
        with torch.no_grad():
            lo = victim(x)[0]
        y, tgt = lo.argmax(1).cpu(), lo.topk(2)[1][:, 1].cpu()
        res = {}
        for basis in ("full", "lowband"):
            atk = ta.CWTAOF(victim, adv_utils.LogitsAdvLoss(0.), dist_utils.L2Dist(), low_pass=lp,
                            clip_func=clip_utils.ClipPointsLinf(0.18), device=dev, basis=basis)

            def run():
                torch.manual_seed(0)
                res[basis] = atk.attack(pcs, tgt, y)
            out[f"attack_2x200_{basis}_ms"] = wall_ms(run, n=2)
        out["attack_outcome"] = {n: {"found": int((r[0] < 1e9).sum()), "success_num": r[2]} for n, r in res.items()}
        out["attack_faster_with_lowband"] = bool(out["attack_2x200_lowband_ms"]["median"] < out["attack_2x200_full_ms"]["median"])
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
