"""defense.FusedDefended on the GPU: what the SOR head costs inside the device-side attack loops, and which search it
should use. B = 32, PointNet with 40 classes (seeded weights), SORDefense(k = 2, alpha = 1.1, npoint = K).

  search           pc3d_knn_small_f32 (ops.knn_small_dists) against ops.knn_raw (the wave-per-query kernel, with the hint
                   of its own last call, as sor_select calls it) on the same clouds, self-search, channel-first, replayed
                   from hipGraphs: k1 = 3 at K = 1024 / 2048 / 4096 and k1 = 9 at K = 1024. The two are timed alternately,
                   `--repeats` times each; median and the spread (max - min) of both are recorded, and `adopt` says
                   whether the new kernel is faster at K = 1024, k1 = 3 by more than the larger spread — the rule
                   defense.SOR_SMALL_SEARCH is set by. The outputs are compared bit for bit first.
  head_us          the SOR pieces alone, replayed: search + select (forward) and the backward launch, per search
  cw_ms            one CW iteration (Chamfer, ClipPointsLinf), K = 1024: FusedDefended in the fused loop (replayed), with
                   either search; Defended on the autograd path (fused=False; tools/bench_defense.py's figure); the
                   undefended victim in the same fused pass FusedDefended's loop takes (riders=None) and in the default
                   loop. head_cost_ms = FusedDefended - undefended (same pass).
  siadv_step_us    SI-Adv's white-box step (search, frame, victim passes, step) with and without the head, replayed
Replayed timings start after >= 150 ms of the same work. Writes profiles/fused_defended_bench.json.
Usage: python tools/bench_fused_defended.py [--out FILE] [--repeats N]"""
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
import numpy as np  # noqa: E402
import torch  # noqa: E402

from test_defense_cpu import outlier_cloud  # noqa: E402

M = importlib.import_module
dev = torch.device("cuda:0")
ops = M("3dpointcloudattack_amd.ops")
dfn = M("3dpointcloudattack_amd.defense")
si = M("3dpointcloudattack_amd.attack.SIadv.SIadv_attack")
seeded_state_dict = M("3dpointcloudattack_amd.seeding").seeded_state_dict


class Replayed:
    """fn captured `per` times back to back; us() = one timed window of `reps` replays after 150 ms of the same work."""

    def __init__(self, fn, per=20):
        self.per, self.side, self.g = per, torch.cuda.Stream(), torch.cuda.CUDAGraph()
        with torch.cuda.stream(self.side):
            for _ in range(2):
                fn()
            self.side.synchronize()
            with torch.cuda.graph(self.g, stream=self.side):
                for _ in range(per):
                    fn()

    def us(self, reps=50):
        with torch.cuda.stream(self.side):
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < 0.15:
                for _ in range(5):
                    self.g.replay()
                self.side.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(self.side)
            for _ in range(reps):
                self.g.replay()
            e1.record(self.side)
            e1.synchronize()
        return e0.elapsed_time(e1) / (self.per * reps) * 1e3


def alternate(fns, repeats):
    """{name: dict(median, min, max, spread)} in us, the candidates timed in turn `repeats` times."""
    rep = {k: Replayed(f) for k, f in fns.items()}
    v = {k: [] for k in fns}
    for _ in range(repeats):
        for k in fns:
            v[k].append(rep[k].us())
    return {k: dict(median=round(statistics.median(t), 2), min=round(min(t), 2), max=round(max(t), 2),
                    spread=round(max(t) - min(t), 2)) for k, t in v.items()}


def clouds(B, K, seed=0):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(np.stack([outlier_cloud(rng, K) for _ in range(B)]))           # [B,K,3]


def victim(seed):
    m = M("3dpointcloudattack_amd.model.pointnet").PointNetCls(k=40)
    m.load_state_dict(seeded_state_dict(m, seed))
    return m.to(dev).eval()


def search_rows(B, repeats):
    rows = []
    for K, k1 in ((1024, 3), (2048, 3), (4096, 3), (1024, 9)):
        x = clouds(B, K, K).to(dev).transpose(1, 2).contiguous()
        a, b = ops.knn_small_dists(x, x, k1, True, True), ops.knn_raw(x, x, k1, True, True)[0]
        same = bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))
        t = alternate({"knn_small": lambda: ops.knn_small_dists(x, x, k1, True, True),
                       "knn_raw": lambda: ops.knn_raw(x, x, k1, True, True)}, repeats)
        rows.append(dict(B=B, K=K, k1=k1, bit_equal=same, knn_small_us=t["knn_small"], knn_raw_us=t["knn_raw"],
                         speedup=round(t["knn_raw"]["median"] / t["knn_small"]["median"], 2)))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def head_rows(B, K, repeats):
    x = clouds(B, K, 1).to(dev).transpose(1, 2).contiguous()
    g = torch.rand((B, 3, K), device=dev)
    sel = dfn.sor_select(x, 2, 1.1, K)
    return alternate({"fwd_knn_raw": lambda: dfn.sor_select(x, 2, 1.1, K),
                      "fwd_knn_small": lambda: dfn.sor_select(x, 2, 1.1, K, search="small"),
                      "bwd": lambda: dfn.sor_backward(g, sel["count"], sel["rank"])}, repeats)


def cw_runner(vic, trans, pcs, labels, **kw):
    cwm = M("3dpointcloudattack_amd.attack.CW.CW_attack")
    u = "3dpointcloudattack_amd.attack.CW.CW_utils."
    atk = cwm.CW(vic, trans, adv_func=M(u + "adv_utils").UntargetedLogitsAdvLoss(5.),
                 clip_func=M(u + "clip_utils").ClipPointsLinf(0.18), dist_func=M(u + "dist_utils").ChamferDist(), **kw)
    torch.manual_seed(0)
    st = atk._begin(pcs, labels)
    atk._begin_binary_step(st)
    return atk._make_runner(st), atk._capturable()


def cw_ms(run, iters=96):
    def window(n):
        for _ in range(n):
            run()
        if hasattr(run, "flush"):
            run.flush()
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.15:
        window(16)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    window(iters)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def cw_rows(B, K, repeats):
    pcs = clouds(B, K, 0)
    model, trans = victim(0), victim(1)
    with torch.no_grad():
        labels = model(pcs.transpose(1, 2).contiguous().to(dev))[0].argmax(1).cpu()
    runs, captured = {}, {}
    for name, small in (("fused_defended_knn_raw", False), ("fused_defended_knn_small", True)):
        dfn.SOR_SMALL_SEARCH = small               # read at call time; the capture below bakes the launch in
        runs[name], captured[name] = cw_runner(dfn.FusedDefended(model, dfn.SORDefense(2, 1.1, K)), trans, pcs, labels)
    runs["undefended_same_pass"], captured["undefended_same_pass"] = cw_runner(model, trans, pcs, labels, riders=None)
    runs["undefended_default"], captured["undefended_default"] = cw_runner(model, trans, pcs, labels)
    runs["defended_autograd"], captured["defended_autograd"] = cw_runner(dfn.Defended(model, dfn.SORDefense(2, 1.1, K)), trans,
                                                                         pcs, labels, fused=False)
    v = {k: [] for k in runs}
    for _ in range(repeats):
        for k, r in runs.items():
            v[k].append(cw_ms(r, 32 if k == "defended_autograd" else 96))
    out = {k: dict(median=round(statistics.median(t), 4), min=round(min(t), 4), max=round(max(t), 4), captured=captured[k])
           for k, t in v.items()}
    base = out["undefended_same_pass"]["median"]
    out["head_cost_ms"] = {k: round(out[k]["median"] - base, 4) for k in ("fused_defended_knn_raw", "fused_defended_knn_small")}
    out["autograd_over_fused"] = round(out["defended_autograd"]["median"] / min(out["fused_defended_knn_raw"]["median"],
                                                                                 out["fused_defended_knn_small"]["median"]), 2)
    return out


def siadv_rows(B, N, repeats):
    pcs = clouds(B, N, 2)
    x = pcs.to(dev).transpose(1, 2).contiguous()
    model = victim(3)
    with torch.no_grad():
        label = model(x)[0].argmax(1)
    fns = {}
    loops = []
    for name, vic, small in (("undefended", model, False),
                             ("fused_defended_knn_raw", dfn.FusedDefended(model, dfn.SORDefense(2, 1.1, N)), False),
                             ("fused_defended_knn_small", dfn.FusedDefended(model, dfn.SORDefense(2, 1.1, N)), True)):
        loop = si._Loop(vic, B, N, dev, 0.07, 0.16)
        loop.load(x, x, label)
        loops.append(loop)

        def step(loop=loop, small=small):
            dfn.SOR_SMALL_SEARCH = small
            loop.step()
        fns[name] = step
    out = alternate(fns, repeats)
    out["head_cost_us"] = {k: round(out[k]["median"] - out["undefended"]["median"], 2)
                           for k in ("fused_defended_knn_raw", "fused_defended_knn_small")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fused_defended_bench.json"))
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    default_search = dfn.SOR_SMALL_SEARCH
    B = 32
    res = {"what": "tools/bench_fused_defended.py on one MI355X, one process; replayed hipGraphs after 150 ms of the same work, "
                   f"candidates timed alternately, {a.repeats} windows each (median, min, max; spread = max - min)",
           "device": torch.cuda.get_device_name(0), "SOR_SMALL_SEARCH_as_committed": bool(default_search)}
    res["search"] = search_rows(B, a.repeats)
    r0 = res["search"][0]
    gain = r0["knn_raw_us"]["median"] - r0["knn_small_us"]["median"]
    spread = max(r0["knn_raw_us"]["spread"], r0["knn_small_us"]["spread"])
    res["adopt"] = dict(rule="knn_small faster than knn_raw at B=32, K=1024, k1=3 by more than the larger run-to-run spread",
                        gain_us=round(gain, 2), spread_us=spread, adopt=bool(gain > spread and all(r["bit_equal"] for r in res["search"])))
    res["head_us"] = head_rows(B, 1024, a.repeats)
    print(json.dumps(res["head_us"]), flush=True)
    res["cw_ms"] = cw_rows(B, 1024, a.repeats)
    print(json.dumps(res["cw_ms"]), flush=True)
    res["siadv_step_us"] = siadv_rows(B, 1024, a.repeats)
    dfn.SOR_SMALL_SEARCH = default_search
    doc = json.dumps(res, indent=1)
    print(doc)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(doc + "\n")


if __name__ == "__main__":
    main()
