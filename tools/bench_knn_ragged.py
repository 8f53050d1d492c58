"""Clouds of different sizes in the kNN attack's device loop on the GPU: what the ragged iteration costs and what it saves.
B = 32, Kmax = 1024, lengths uniform in [256, 1024] from a fixed seed, PointNet with 40 classes (seeded weights),
UntargetedLogitsAdvLoss(15), ChamferkNNDist(), ProjectInnerClipLinf(0.18).

  iter_us          one iteration of CWKNN(device_loop=True), replayed from the attack's own 16-iteration hipGraph: `ragged`
                   (attack(data, target, lengths)), `dense` (32 clouds of K = 1024 points, the yardstick) and `alone_sum` (the
                   same 32 clouds as 32 attacks at B = 1, each at its own size: the sum of their iterations, what a user does
                   without lengths). The candidates are timed alternately, `--repeats` windows each; median, min, max, spread.
  victim_us        fused_attack_grad alone on the ragged loop's padded buffers (`padded_data`: without lengths; `lengths`:
                   given them) and on the dense loop's: what the padded DATA costs the victim's
                   data-dependent tower forward, apart from the two new kernels
  --towers         iter_us `ragged` and `dense` and victim_us only (no runs alone, no search / update rows): the measurement
                   of §8.19, taken on this tree and on its parent in alternated processes (a tree whose victim takes no
                   lengths has no `lengths` candidate)
  search_us        the self-kNN search alone: pc3d_knn_ragged_f32 on the padded batch, the same kernel with all lengths = Kmax
                   on the dense clouds, and its dense twin pc3d_knn_hint_f32 on the dense clouds (all hinted by their own result)
  update_us        the update launch alone, likewise
Replayed timings start after >= 150 ms of the same work. Writes profiles/knn_ragged_bench.json.
Usage: python tools/bench_knn_ragged.py [--out FILE] [--repeats N]"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_fused_defended import alternate, dev, victim  # noqa: E402
from helpers import unit_cloud  # noqa: E402

M = importlib.import_module
ops = M("3dpointcloudattack_amd.ops")
cloud_io = M("3dpointcloudattack_amd.dataset.cloud_io")
knn = M("3dpointcloudattack_amd.attack.KNN.KNN_attack")
KAPPA, BUDGET, LR = 15.0, 0.18, 1e-3


def attacker(model, **kw):
    u = "3dpointcloudattack_amd.attack.CW.CW_utils."
    return knn.CWKNN(model, None, None, None, None, None, adv_func=M(u + "adv_utils").UntargetedLogitsAdvLoss(KAPPA),
                     dist_func=M(u + "dist_utils").ChamferkNNDist(), clip_func=M(u + "clip_utils").ProjectInnerClipLinf(BUDGET),
                     attack_lr=LR, num_iter=16, device=dev, device_loop=True, **kw)


def captured_loop(atk, *args):
    """The attack's own loop after one 16-iteration attack(): its buffers hold the clouds, its graphs are captured."""
    torch.manual_seed(0)
    atk.attack(*args)
    assert atk.last_path == "device_loop"
    loop = next(iter(atk._loop_cache.values()))
    assert loop.graphs is not None
    return loop


def loop_us(loop, reps=6):
    """One iteration in us: `reps` replays of the 16-iteration graph after >= 150 ms of the same replays."""
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.15:
        loop.graphs.replay(16)
        torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        loop.graphs.replay(16)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (16 * reps) * 1e3


def stats(t, nd=2):
    return dict(median=round(statistics.median(t), nd), min=round(min(t), nd), max=round(max(t), nd),
                spread=round(max(t) - min(t), nd))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_ragged_bench.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--towers", action="store_true", help="the ragged and dense iteration and the victim alone, nothing else")
    a = ap.parse_args()
    B, K = 32, 1024
    rng = np.random.default_rng(2024)
    lengths = rng.integers(256, K + 1, B)
    clouds = [unit_cloud(rng, int(n)) for n in lengths]
    data, lens = cloud_io.stack_ragged(clouds)
    if data.shape[1] < K:        # the capacity is Kmax = K whatever the largest draw (rows behind a length are ignored)
        data = np.concatenate([data, np.repeat(data[:, :1], K - data.shape[1], axis=1)], axis=1)
    dense = torch.from_numpy(np.stack([unit_cloud(np.random.default_rng(100 + b), K) for b in range(B)]))
    model = victim(0)
    with torch.no_grad():
        labels = model(torch.from_numpy(data).transpose(1, 2).contiguous().to(dev))[0].argmax(1).cpu()
        dense_labels = model(dense.transpose(1, 2).contiguous().to(dev))[0].argmax(1).cpu()
    res = {"what": "tools/bench_knn_ragged.py on one MI355X, one process; replayed hipGraphs after 150 ms of the same work, "
                   f"candidates timed alternately, {a.repeats} windows each (median, min, max; spread = max - min)",
           "device": torch.cuda.get_device_name(0), "B": B, "Kmax": K, "lengths": [int(n) for n in lengths],
           "points_counted_share": round(float(np.sum(lengths)) / (B * K), 3)}

    ragged = captured_loop(attacker(model, sample_seeds=list(range(B))), torch.from_numpy(data), labels, lens)
    full = captured_loop(attacker(model), dense, dense_labels)
    alone = [] if a.towers else [
        captured_loop(attacker(model, sample_seeds=[b], global_batch=B), torch.from_numpy(c)[None], labels[b:b + 1])
        for b, c in enumerate(clouds)]
    v = {"ragged": [], "dense": []}
    if alone:
        v["alone_sum"] = []
    for _ in range(a.repeats):
        v["ragged"].append(loop_us(ragged))
        v["dense"].append(loop_us(full))
        if alone:
            v["alone_sum"].append(sum(loop_us(lp, 2) for lp in alone))
    it = {k: stats(t) for k, t in v.items()}
    it["ragged_minus_dense"] = round(it["ragged"]["median"] - it["dense"]["median"], 2)
    it["larger_spread"] = max(it["ragged"]["spread"], it["dense"]["spread"])
    if alone:
        it["alone_over_ragged"] = round(it["alone_sum"]["median"] / it["ragged"]["median"], 2)
    res["iter_us"] = it
    print(json.dumps(it), flush=True)

    r, d = ragged.bufs, full.bufs
    plan = d["plan"]
    kind, kappa = plan["kind"]
    lens_full = torch.full((B,), K, dtype=torch.int32, device=dev)
    host_full = np.full(B, K)
    c_ch_full, c_knn_full = (torch.full((B,), plan[n], dtype=torch.float32, device=dev) for n in ("c_ch", "c_knn"))
    one = torch.ones(1, dtype=torch.int32, device=dev)
    gx = torch.randn(B, 3, K, device=dev) * 1e-3
    gx_r = ops.pad_ragged(gx.clone(), r["lens"])

    def vpass(c, **kw):
        return lambda: plan["victim"].fused_attack_grad(c["adv"], c["target"], kind, kappa, pred_out=c["pred"], step=c["step"],
                                                        scale=plan["scale"], **kw)

    def update(c, g, **kw):
        return lambda: ops.knn_attack_update(c["adv"], c["ori"], g, c["m"], c["v"], one, LR, c["knn_d"], c["knn_idx"],
                                             c["nn_idx"], alpha=plan["alpha"], budget=plan["budget"], clip_mode=plan["clip_mode"],
                                             normal=c["normal"], **kw)
    with torch.no_grad():
        vp = {"padded_data": vpass(r), "dense_data": vpass(d)}
        if getattr(plan["victim"], "fused_lengths", False):
            vp["lengths"] = vpass(r, lengths=r["lens"])
        res["victim_us"] = alternate(vp, a.repeats)
        if a.towers:
            return finish(res, a.out)
        res["search_us"] = alternate({
            "ragged": lambda: ops.knn_search_into(r["adv"], r["knn_d"], r["knn_idx"], lengths=r["lens"], lengths_host=r["lens_host"]),
            "ragged_kernel_full_lengths": lambda: ops.knn_search_into(d["adv"], d["knn_d"], d["knn_idx"], lengths=lens_full,
                                                                      lengths_host=host_full),
            "dense": lambda: ops.knn_search_into(d["adv"], d["knn_d"], d["knn_idx"])}, a.repeats)
        res["update_us"] = alternate({
            "ragged": update(r, gx_r, c_chamfer=r["c_ch"], c_knn=r["c_knn"], lengths=r["lens"]),
            "ragged_kernel_full_lengths": update(d, gx, c_chamfer=c_ch_full, c_knn=c_knn_full, lengths=lens_full),
            "dense": update(d, gx, c_chamfer=plan["c_ch"], c_knn=plan["c_knn"])}, a.repeats)
    finish(res, a.out)


def finish(res, out):
    doc = json.dumps(res, indent=1)
    print(doc)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(doc + "\n")


if __name__ == "__main__":
    main()
