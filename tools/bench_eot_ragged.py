"""Clouds of different sizes in the additional-experiments CW device loop (EOT over ten views + renormalisation + z-only
box, Chamfer) on the GPU: what the ragged iteration costs and what it saves. B = 32, Kmax = 4096, lengths uniform in
[2048, 4096] from a fixed seed — the face-scan workload of the reference driver, which runs one cloud at a time — PointNet
with 40 classes (seeded weights), device draws; every figure with and without resampling.

  iteration_us     one iteration replayed from the attack's own hipGraph (the draw launch is outside it): `ragged`
                   (attack(..., lengths=...)), `dense` (32 clouds of K = 4096, the yardstick) and `alone_sum` (the same 32
                   clouds as 32 device-loop attacks at B = 1, each at its own size: the sum of their iterations, what a user
                   does without lengths). Timed alternately, `--repeats` windows each; median, min, max, spread.
  draw_block_us    the launch in front of every block of 16 iterations: pc3d_eot_draw_ragged_f32 (B tables a view) against
                   pc3d_eot_draw_f32 (one); `share` = its part of block + 16 iterations
  prepare_us / update_us / draw_us
                   the three launches alone: `ragged` on the ragged batch, `ragged_kernel_full_lengths` and `dense` on the
                   full clouds
  --dense-only     the dense iteration alone, importing the package from --root: what --pairs runs
  --pairs DIR      five alternated pairs of fresh processes, this tree's dense iteration against the tree at DIR (its parent
                   commit, named by --parent-name), with resampling; the dense device code is unchanged, so the two must lie
                   inside each other's spread
Replayed timings start after >= 150 ms of the same work (50 ms for each of the 32 loops of alone_sum). Writes
profiles/eot_ragged_bench.json.
Usage: python tools/bench_eot_ragged.py [--out FILE] [--repeats N] [--pairs DIR --parent-name NAME] [--dense-only] [--root DIR]"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time


def _root():
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    return os.path.abspath(ap.parse_known_args()[0].root)


HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = _root()
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_fused_defended import alternate, dev, victim  # noqa: E402
from helpers import unit_cloud  # noqa: E402

M = importlib.import_module
ops = M("3dpointcloudattack_amd.ops")
cwm = M("3dpointcloudattack_amd.attack.additional_exp.CW_attack")
adv_u = M("3dpointcloudattack_amd.attack.CW.CW_utils.adv_utils")
dist_u = M("3dpointcloudattack_amd.attack.CW.CW_utils.dist_utils")
B, KMAX, E, SEED = 32, 4096, 10, 11


def captured_loop(model, data, target, resample, **kw):
    """The attack's own loop after one binary step of 16 iterations: its buffers hold the clouds and the tables of the last
    block, its graphs are captured. (sample_seeds / global_batch exist on the tree that has `lengths`.)"""
    extra = dict(sample_seeds=list(range(data.shape[0])), global_batch=data.shape[0]) if kw else {}
    atk = cwm.CW(model, cwm.AdvLossAdapter(adv_u.LogitsAdvLoss(0.), adv_u.UntargetedLogitsAdvLoss(0.)),
                 cwm.PerSampleDist(dist_u.ChamferDist()), binary_step=1, num_iter=16, whether_target=True, whether_1d=True,
                 whether_3Dtransform=True, whether_renormalization=True, whether_resample=resample, graph=True,
                 device_loop=True, device_rng=True, seed=SEED, **extra)
    torch.manual_seed(0)
    atk.attack(data, target, target, **kw)
    assert atk.last_path == "device_loop" and atk.last_draws == "device"
    loop = next(iter(atk._loop_cache.values()))
    assert loop.graphs is not None
    return loop


def loop_us(loop, reps=4, per=16, warm=0.15):
    """One iteration in us: `reps` replays of the 16-iteration graph after >= `warm` s of the same replays."""
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < warm:
        loop.run(per)
        torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        loop.run(per)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (per * reps) * 1e3


def launches_us(fns, repeats, per=20):
    """{name: stats} of plain launches on the current stream (the draw runs outside the loop's graph), in turn."""
    v = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < 0.15:
                fn()
                torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(per):
                fn()
            e1.record()
            torch.cuda.synchronize()
            v[k].append(e0.elapsed_time(e1) / per * 1e3)
    return {k: stats(t) for k, t in v.items()}


def stats(t, nd=2):
    return dict(median=round(statistics.median(t), nd), min=round(min(t), nd), max=round(max(t), nd),
                spread=round(max(t) - min(t), nd))


def labels_of(model, clouds):
    with torch.no_grad():
        return torch.cat([model(torch.from_numpy(c).t().contiguous()[None].to(dev))[0].topk(2, dim=1)[1][:, 1] for c in clouds]).cpu()


def pairs(a):
    """Five alternated pairs of fresh processes: this tree's dense iteration, the parent's."""
    v = {"this_tree": [], a.parent_name: []}
    for _ in range(5):
        for name, root in (("this_tree", HERE), (a.parent_name, os.path.abspath(a.pairs))):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--dense-only", "--root", root, "--repeats", "3",
                                  "--out", os.devnull], check=True, capture_output=True, text=True).stdout
            v[name].append(json.loads(out.strip().splitlines()[-1])["dense_iteration_us"]["median"])
            print(name, v[name][-1], flush=True)
    res = {k: dict(stats(t), runs=t) for k, t in v.items()}
    res["difference_of_medians"] = round(res["this_tree"]["median"] - res[a.parent_name]["median"], 2)
    res["larger_spread"] = max(res["this_tree"]["spread"], res[a.parent_name]["spread"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "eot_ragged_bench.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--dense-only", action="store_true", help="the dense iteration (with resampling) alone, nothing else")
    ap.add_argument("--root", default=ROOT, help="the tree whose package is measured (default: this file's)")
    ap.add_argument("--pairs", default=None, help="a checkout of the parent commit to compare the dense iteration against")
    ap.add_argument("--parent-name", default="parent", help="how the JSON names that checkout")
    a = ap.parse_args()
    rng = np.random.default_rng(2024)
    lengths = rng.integers(2048, KMAX + 1, B)
    model = victim(0)
    full_clouds = [unit_cloud(rng, KMAX) for _ in range(B)]
    dense_data, dense_tgt = torch.from_numpy(np.stack(full_clouds)), labels_of(model, full_clouds)
    if a.dense_only:
        loop = captured_loop(model, dense_data, dense_tgt, True)
        print(json.dumps({"dense_iteration_us": stats([loop_us(loop) for _ in range(a.repeats)])}))
        return
    res = {"what": "tools/bench_eot_ragged.py on one MI355X; replayed hipGraphs after 150 ms of the same work, candidates timed "
                   f"alternately, {a.repeats} windows each (median, min, max; spread = max - min)",
           "device": torch.cuda.get_device_name(0), "B": B, "Kmax": KMAX, "E": E, "lengths": [int(n) for n in lengths],
           "points_counted_share": round(float(np.sum(lengths)) / (B * KMAX), 3)}
    clouds = [unit_cloud(rng, int(n)) for n in lengths]
    data = torch.full((B, KMAX, 3), float("nan"))                          # the rows behind a length are only written
    for b, c in enumerate(clouds):
        data[b, :c.shape[0]] = torch.from_numpy(c)
    tgt = labels_of(model, clouds)
    for resample in (False, True):
        tag = "resample" if resample else "views"
        ragged = captured_loop(model, data, tgt, resample, lengths=lengths)
        dense = captured_loop(model, dense_data, dense_tgt, resample)
        alone = [captured_loop(model, torch.from_numpy(c)[None], tgt[b:b + 1], resample) for b, c in enumerate(clouds)]
        assert ragged.bufs["lens"] is not None and dense.bufs.get("lens") is None
        v = {"ragged": [], "dense": [], "alone_sum": []}
        for _ in range(a.repeats):
            v["ragged"].append(loop_us(ragged))
            v["dense"].append(loop_us(dense))
            v["alone_sum"].append(sum(loop_us(lp, 2, warm=0.05) for lp in alone))
        it = {k: stats(t) for k, t in v.items()}
        it["alone_over_ragged"] = round(it["alone_sum"]["median"] / it["ragged"]["median"], 2)
        it["ragged_over_dense"] = round(it["ragged"]["median"] / it["dense"]["median"], 3)
        res[f"iteration_us_{tag}"] = it
        print(tag, json.dumps(it), flush=True)
        r, d = ragged.bufs, dense.bufs
        lens_full = torch.full((B,), KMAX, dtype=torch.int32, device=dev)
        with torch.no_grad():
            if resample:
                idx_f, inv_f = torch.zeros_like(r["idx"]), torch.zeros_like(r["inv"])
                ops.eot_draw(SEED, 0, (0, 32), d["rot"], idx_f, inv_f, lengths=lens_full)
                blk = launches_us({
                    "ragged": lambda: ops.eot_draw(SEED, 0, (0, 16), r["rot"], r["idx"], r["inv"], lengths=r["lens"]),
                    "ragged_kernel_full_lengths": lambda: ops.eot_draw(SEED, 0, (0, 16), d["rot"], idx_f, inv_f, lengths=lens_full),
                    "dense": lambda: ops.eot_draw(SEED, 0, (0, 16), d["rot"], d["idx"], d["inv"])}, a.repeats)
                blk["share_of_ragged_block"] = round(blk["ragged"]["median"] / (blk["ragged"]["median"] + 16 * it["ragged"]["median"]), 3)
                blk["share_of_dense_block"] = round(blk["dense"]["median"] / (blk["dense"]["median"] + 16 * it["dense"]["median"]), 3)
                res["draw_block_us"] = blk
                print("draw", json.dumps(blk), flush=True)
            else:
                idx_f = inv_f = None
            Xf = torch.empty_like(d["X"])
            res[f"prepare_us_{tag}"] = alternate({
                "ragged": lambda: ops.eot_prepare(r["adv"], r["ori"], r["rot"], r["idx"], True, r["step"], out=r["X"],
                                                  stats=r["stats"], arg=r["arg"], lengths=r["lens"]),
                "ragged_kernel_full_lengths": lambda: ops.eot_prepare(d["adv"], d["ori"], d["rot"], idx_f, True, d["step"], out=Xf,
                                                                      stats=d["stats"], arg=d["arg"], lengths=lens_full),
                "dense": lambda: ops.eot_prepare(d["adv"], d["ori"], d["rot"], d["idx"], True, d["step"], out=Xf,
                                                 stats=d["stats"], arg=d["arg"])}, a.repeats)
            gx = torch.randn((1 + E) * B, 3, KMAX, device=dev) * 1e-3

            def upd(c, inv, **kw):
                # (the step word stands still: every launch reads the same rows)
                ops.eot_update(c["adv"], c["ori"], gx, c["m"], c["v"], c["step"], 1e-2, c["pred"], c["goal"], False,
                               c["bestdist"], c["bestscore"], c["o_bestdist"], c["o_bestscore"], c["o_bestattack"], rot=c["rot"],
                               inv=inv, renorm=True, stats=c["stats"], arg=c["arg"], input_val=c["input_val"],
                               dist_kind="chamfer", w=c["w"], nn_idx=c["nn_idx"], batch_mean=B, one_d=True, **kw)
            res[f"update_us_{tag}"] = alternate({
                "ragged": lambda: upd(r, r["inv"], lengths=r["lens"]),
                "ragged_kernel_full_lengths": lambda: upd(d, inv_f, lengths=lens_full),
                "dense": lambda: upd(d, d["inv"])}, a.repeats)
        for k in (f"prepare_us_{tag}", f"update_us_{tag}"):
            t = res[k]
            t["full_lengths_minus_dense"] = round(t["ragged_kernel_full_lengths"]["median"] - t["dense"]["median"], 2)
            t["larger_spread"] = max(t["ragged_kernel_full_lengths"]["spread"], t["dense"]["spread"])
            print(k, json.dumps(t), flush=True)
        del ragged, dense, alone
    if a.pairs:
        res["dense_iteration_us_against_" + a.parent_name] = pairs(a)
    doc = json.dumps(res, indent=1)
    print(doc)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(doc + "\n")


if __name__ == "__main__":
    main()
