"""Clouds of different sizes in the shape-invariant white-box attack's device loop on the GPU: what the ragged step costs and
what it saves. B = 32, Kmax = 1024, lengths uniform in [256, 1024] from a fixed seed (the draw of tools/bench_knn_ragged.py),
clouds on an ellipsoid, PointNet with 40 classes (seeded weights) as surrogate, eps 0.16, step_size 0.07.

  step_us          one step of PointCloudAttack's fast path, replayed from the attack's own hipGraph: `ragged`
                   (iterate(points, target, lengths=...)), `dense` (32 clouds of K = 1024 points, the yardstick) and
                   `alone_sum` (the same 32 clouds as 32 device-loop attacks at B = 1, each at its own size: the sum of their
                   steps, what a user does without lengths). The candidates are timed alternately, `--repeats` windows each;
                   median, min, max, spread.
  search_us        the self-kNN search alone (K = 20, hinted by its own result): pc3d_knn_ragged_f32 on the padded batch, the
                   same kernel with all lengths = Kmax on the dense clouds, and its dense twin pc3d_knn_hint_f32 on them
  frame_us         pc3d_si_frame_ragged_f32 / pc3d_si_frame_f32 alone, from the neighbour lists, likewise
  step_kernel_us   pc3d_si_step_ragged_f32 / pc3d_si_step_f32 alone (normals given, as the loop calls it), likewise
  pca_normal_us    pc3d_pca_normal_ragged_f32 / pc3d_pca_normal_f32 alone, likewise
  --dense-only     the dense step alone (step_us `dense`), nothing else, importing the package from --root: the measurement
                   that is taken on this tree and on its parent in alternated processes
Replayed timings start after >= 150 ms of the same work. Writes profiles/siadv_ragged_bench.json.
Usage: python tools/bench_siadv_ragged.py [--out FILE] [--repeats N] [--dense-only] [--root DIR]"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time
import types


def _root():
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    return os.path.abspath(ap.parse_known_args()[0].root)


ROOT = _root()
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_fused_defended import alternate, dev, victim  # noqa: E402
from test_siadv_gpu import ellipsoid  # noqa: E402

M = importlib.import_module
ops = M("3dpointcloudattack_amd.ops")
si = M("3dpointcloudattack_amd.attack.SIadv.SIadv_attack")
EPS, STEP, KNN = 0.16, 0.07, 20


def attacker(model):
    args = types.SimpleNamespace(eps=EPS, step_size=STEP, max_steps=2, num_class=40, top5_attack=False, defense_method=None,
                                 transfer_attack_method="ifgm_ours", query_attack_method=None)
    return si.PointCloudAttack(args, wb_classifier=model, classifier=model)


def captured_loop(atk, points, target, **kw):
    """The attack's own loop after a two-step iterate(): its buffers hold the clouds, its graph is captured."""
    atk.iterate(points, target, **kw)
    loop = next(iter(atk._loops.values()))
    assert loop.graphs is not None
    return loop


def loop_us(loop, reps=6, per=16):
    """One step in us: `reps` rounds of `per` replays of the one-step graph after >= 150 ms of the same replays."""
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.15:
        loop.run(per)
        torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        loop.run(per)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (per * reps) * 1e3


def stats(t, nd=2):
    return dict(median=round(statistics.median(t), nd), min=round(min(t), nd), max=round(max(t), nd),
                spread=round(max(t) - min(t), nd))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "siadv_ragged_bench.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--dense-only", action="store_true", help="the dense step alone, nothing else")
    ap.add_argument("--root", default=ROOT, help="the tree whose package is measured (default: this file's)")
    a = ap.parse_args()
    B, K = 32, 1024
    rng = np.random.default_rng(2024)
    lengths = rng.integers(256, K + 1, B)
    model = victim(0)
    dense = ellipsoid(B, K, 1)[0].to(dev)                                  # [B,K,3]: every step estimates its normals
    with torch.no_grad():
        dense_labels = model(dense.transpose(1, 2).contiguous())[0].argmax(1)
    full = captured_loop(attacker(model), dense, dense_labels)
    res = {"what": "tools/bench_siadv_ragged.py on one MI355X, one process; replayed hipGraphs after 150 ms of the same work, "
                   f"candidates timed alternately, {a.repeats} windows each (median, min, max; spread = max - min)",
           "device": torch.cuda.get_device_name(0), "root": os.path.relpath(ROOT), "B": B, "Kmax": K,
           "lengths": [int(n) for n in lengths], "points_counted_share": round(float(np.sum(lengths)) / (B * K), 3)}
    if a.dense_only:
        res["step_us"] = {"dense": stats([loop_us(full) for _ in range(a.repeats)])}
        return finish(res, a.out)

    clouds = [ellipsoid(1, int(n), 100 + b)[0][0] for b, n in enumerate(lengths)]            # [n,3] each
    data = torch.full((B, K, 3), float("nan"))                             # the rows behind a length are only written
    for b, c in enumerate(clouds):
        data[b, :c.shape[0]] = c
    data = data.to(dev)
    with torch.no_grad():
        labels = torch.cat([model(c[None].transpose(1, 2).contiguous().to(dev))[0].argmax(1) for c in clouds])
    ragged = captured_loop(attacker(model), data, labels, lengths=lengths)
    assert ragged.ragged and not full.ragged
    alone = [captured_loop(attacker(model), c[None].to(dev), labels[b:b + 1]) for b, c in enumerate(clouds)]
    v = {"ragged": [], "dense": [], "alone_sum": []}
    for _ in range(a.repeats):
        v["ragged"].append(loop_us(ragged))
        v["dense"].append(loop_us(full))
        v["alone_sum"].append(sum(loop_us(lp, 2) for lp in alone))
    it = {k: stats(t) for k, t in v.items()}
    it["ragged_minus_dense"] = round(it["ragged"]["median"] - it["dense"]["median"], 2)
    it["larger_spread"] = max(it["ragged"]["spread"], it["dense"]["spread"])
    it["alone_over_ragged"] = round(it["alone_sum"]["median"] / it["ragged"]["median"], 2)
    res["step_us"] = it
    print(json.dumps(it), flush=True)

    r = ragged.bufs
    lens_full = torch.full((B,), K, dtype=torch.int32, device=dev)
    host_full = np.full(B, K)
    xd, xr = full.bufs["x"].clone(), r["x"].clone()
    dd, di = torch.zeros((B, K, KNN), device=dev), torch.zeros((B, K, KNN), dtype=torch.int32, device=dev)
    g = torch.randn(B, 3, K, device=dev)
    xe, nb_d, nb_r = torch.empty_like(xd), torch.empty_like(xd), torch.empty_like(xd)
    with torch.no_grad():
        ops.knn_search_into(xd, dd, di)
        ops.si_frame(xd, idx=di, out=xe, nrm_out=nb_d)
        ops.si_frame(xr, idx=r["idx"], out=xe, nrm_out=nb_r, lengths=r["lens"])
        res["search_us"] = alternate({
            "ragged": lambda: ops.knn_search_into(xr, r["d"], r["idx"], lengths=r["lens"], lengths_host=r["lens_host"]),
            "ragged_kernel_full_lengths": lambda: ops.knn_search_into(xd, dd, di, lengths=lens_full, lengths_host=host_full),
            "dense": lambda: ops.knn_search_into(xd, dd, di)}, a.repeats)
        res["frame_us"] = alternate({
            "ragged": lambda: ops.si_frame(xr, idx=r["idx"], out=xe, nrm_out=nb_r, lengths=r["lens"]),
            "ragged_kernel_full_lengths": lambda: ops.si_frame(xd, idx=di, out=xe, nrm_out=nb_d, lengths=lens_full),
            "dense": lambda: ops.si_frame(xd, idx=di, out=xe, nrm_out=nb_d)}, a.repeats)
        res["pca_normal_us"] = alternate({
            "ragged": lambda: ops.pca_normal(xr, r["idx"], cf=True, lengths=r["lens"]),
            "ragged_kernel_full_lengths": lambda: ops.pca_normal(xd, di, cf=True, lengths=lens_full),
            "dense": lambda: ops.pca_normal(xd, di, cf=True)}, a.repeats)
        # last: the step moves its cloud (inside the eps box of ori)
        od, orr = full.bufs["ori"], r["ori"]
        res["step_kernel_us"] = alternate({
            "ragged": lambda: ops.si_step(xr, orr, g, STEP, EPS, nrm=nb_r, lengths=r["lens"]),
            "ragged_kernel_full_lengths": lambda: ops.si_step(xd, od, g, STEP, EPS, nrm=nb_d, lengths=lens_full),
            "dense": lambda: ops.si_step(xd, od, g, STEP, EPS, nrm=nb_d)}, a.repeats)
    for k in ("search_us", "frame_us", "pca_normal_us", "step_kernel_us"):
        t = res[k]
        t["full_lengths_minus_dense"] = round(t["ragged_kernel_full_lengths"]["median"] - t["dense"]["median"], 2)
        t["larger_spread"] = max(t["ragged_kernel_full_lengths"]["spread"], t["dense"]["spread"])
    finish(res, a.out)


def finish(res, out):
    doc = json.dumps(res, indent=1)
    print(doc)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(doc + "\n")


if __name__ == "__main__":
    main()
