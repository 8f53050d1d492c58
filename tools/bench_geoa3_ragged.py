"""Clouds of different sizes in GeoA3's device loop on the GPU: what the ragged iteration costs and what it saves.
B = 32, Kmax = 1024, lengths uniform in [256, 1024] from a fixed seed, PointNet with 40 classes (seeded weights), the default
loss mix (CE, two-sided Chamfer + 0.1 Hausdorff + curvature at k = 16), cfg.device_loop = True.

  iter_us          one iteration of geoA3_attack(cfg.device_loop = True), replayed from the attack's own 16-iteration hipGraph:
                   `ragged` (lengths given), `dense` (32 clouds of K = 1024 points, the yardstick) and `alone_sum` (the same 32
                   clouds as 32 attacks at B = 1, each at its own size: the sum of their iterations, what a user does without
                   lengths). The candidates are timed alternately, `--repeats` windows each; median, min, max, spread.
  search_us        the self-kNN search alone: pc3d_knn_ragged_f32 on the padded batch, the same kernel with all lengths = Kmax
                   on the dense clouds, and its dense twin pc3d_knn_hint_f32 on the dense clouds (all hinted by their own result)
  update_us        the update launch alone, likewise: pc3d_geoa3_update_ragged_f32 / pc3d_geoa3_update_f32
Replayed timings start after >= 150 ms of the same work. Writes profiles/geoa3_ragged_bench.json.
Usage: python tools/bench_geoa3_ragged.py [--out FILE] [--repeats N]"""
import argparse
import importlib
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_fused_defended import alternate, dev, victim  # noqa: E402
from bench_knn_ragged import finish, loop_us, stats  # noqa: E402
from helpers import unit_cloud  # noqa: E402

M = importlib.import_module
ops = M("3dpointcloudattack_amd.ops")
cloud_io = M("3dpointcloudattack_amd.dataset.cloud_io")
ga = M("3dpointcloudattack_amd.attack.GeoA3.GeoA3_attack")


def config(**over):
    base = dict(attack_method='untarget', curv_loss_weight=1.0, curv_loss_knn=16, initial_const=10, iter_max_steps=16,
                binary_max_steps=1, is_partial_var=False, optim='adam', lr=0.01, npoint=1024, is_subsample_opt=False, eval_num=1,
                is_pre_jitter_input=False, cls_loss_type='CE', classes=40, confidence=0, dis_loss_type='CD',
                is_cd_single_side=False, dis_loss_weight=1.0, hd_loss_weight=0.1, uniform_loss_weight=0.0,
                is_use_lr_scheduler=False, is_debug=False, is_pro_grad=False, cc_linf=0.0, device_loop=True)
    base.update(over)
    return types.SimpleNamespace(**base)


def captured_loop(model, pcs, labels, lengths=None, **over):
    """The attack's own loop after one 16-iteration attack: its buffers hold the clouds, its graphs are captured. The victim
    keeps a few loops only: the caller holds on to this one."""
    ga.geoA3_attack(model, None, None, None, None, None, pcs, labels, config(lengths=lengths, **over), 0, 1)
    assert ga.geoA3_attack.last_path == "device_loop"
    loop = list(model._geoa3_loop_cache.values())[-1]
    assert loop.graphs is not None and (loop.bufs.get("lens") is not None) == (lengths is not None)
    return loop


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geoa3_ragged_bench.json"))
    ap.add_argument("--repeats", type=int, default=5)
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
    res = {"what": "tools/bench_geoa3_ragged.py on one MI355X, one process; replayed hipGraphs after 150 ms of the same work, "
                   f"candidates timed alternately, {a.repeats} windows each (median, min, max; spread = max - min)",
           "device": torch.cuda.get_device_name(0), "B": B, "Kmax": K, "k": 16, "lengths": [int(n) for n in lengths],
           "points_counted_share": round(float(np.sum(lengths)) / (B * K), 3)}

    ragged = captured_loop(model, torch.from_numpy(data), labels, lens, sample_seeds=list(range(B)), global_batch=B)
    full = captured_loop(model, dense, dense_labels)
    alone = [captured_loop(model, torch.from_numpy(c)[None], labels[b:b + 1], sample_seeds=[b], global_batch=B)
             for b, c in enumerate(clouds)]
    v = {"ragged": [], "dense": [], "alone_sum": []}
    for _ in range(a.repeats):
        v["ragged"].append(loop_us(ragged))
        v["dense"].append(loop_us(full))
        v["alone_sum"].append(sum(loop_us(lp, 2) for lp in alone))
    it = {k: stats(t) for k, t in v.items()}
    it["ragged_minus_dense"] = round(it["ragged"]["median"] - it["dense"]["median"], 2)
    it["larger_spread"] = max(it["ragged"]["spread"], it["dense"]["spread"])
    it["alone_over_ragged"] = round(it["alone_sum"]["median"] / it["ragged"]["median"], 2)
    res["iter_us"] = it
    print(it, flush=True)

    r, d = ragged.bufs, full.bufs
    plan = ga._device_loop_plan(model, config(), B, K, False)
    lens_full = torch.full((B,), K, dtype=torch.int32, device=dev)
    host_full = np.full(B, K)
    cls = torch.zeros(B, device=dev)
    gx = torch.randn(B, 3, K, device=dev) * 1e-3

    def update(c, **kw):
        return lambda: ops.geoa3_update(c["x"], c["ori"], c["offset"], gx, c["m"], c["v"], c["step"], c["search"], c["lr"],
                                        c["scale"], cls, c["pred"], c["target"], False, c["constrain"], c["loss_rows"],
                                        c["best_loss"], c["best_attack"], c["best_bs"], c["best_step"], c["iter_best_loss"],
                                        c["iter_best_score"], nn_ao=c["ao_i"], nn_oa=c["oa_i"], knn_idx=c["knn_i"],
                                        normal_ori=c["normal"], kappa_ori=c["kappa_ori"], dis_kind="CD", gval=plan["gval"],
                                        w_dis=plan["w_dis"], w_hd=plan["w_hd"], w_curv=plan["w_curv"], **kw)
    with torch.no_grad():
        res["search_us"] = alternate({
            "ragged": lambda: ops.knn_search_into(r["x"], r["knn_d"], r["knn_i"], lengths=r["lens"], lengths_host=r["lens_host"]),
            "ragged_kernel_full_lengths": lambda: ops.knn_search_into(d["x"], d["knn_d"], d["knn_i"], lengths=lens_full,
                                                                      lengths_host=host_full),
            "dense": lambda: ops.knn_search_into(d["x"], d["knn_d"], d["knn_i"])}, a.repeats)
        res["update_us"] = alternate({
            "ragged": update(r, lengths=r["lens"]),
            "ragged_kernel_full_lengths": update(d, lengths=lens_full),
            "dense": update(d)}, a.repeats)
    for nm in ("search_us", "update_us"):
        t = res[nm]
        t["full_lengths_minus_dense"] = round(t["ragged_kernel_full_lengths"]["median"] - t["dense"]["median"], 2)
        t["larger_spread"] = max(t["ragged_kernel_full_lengths"]["spread"], t["dense"]["spread"])
    finish(res, a.out)


if __name__ == "__main__":
    main()
