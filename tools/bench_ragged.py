"""Clouds of different sizes in one batch on the GPU: what the ragged CW iteration costs and what it saves. B = 32,
Kmax = 1024, lengths uniform in [256, 1024] from a fixed seed, PointNet with 40 classes (seeded weights), Chamfer,
ClipPointsLinf.

  cw_ms            one CW iteration, replayed from hipGraphs: `ragged` (CW.attack's pass with lengths: the 17-launch pass whose
                   update launch is pc3d_cw_update_ragged_f32), `dense_riders_off` (K = 1024, riders=False: the same pass with the
                   dense update launch, the yardstick) and `alone_sum` (the same 32 clouds as 32 attacks at B = 1, each at its
                   own size: the sum of their iterations, what a user does today); `dense_pass_on_padded_data` (the dense pass
                   on the padded batch, lengths ignored: timing only) and `tower_forwards_us` (the victim's two tower forwards
                   on the padded and on the dense clouds) separate what the padded DATA costs the victim's data-dependent
                   forward from what the masked update costs. The candidates are timed alternately,
                   `--repeats` windows each; median, min, max, and the difference ragged - dense against the larger spread.
  update_us        the update launch alone, ragged against dense, on the same state
  pad_us           the padding launch alone
  --towers         the measurement of the towers that take lengths and nothing else: cw_ms `ragged` and
                   `dense_riders_off`, `tower_forwards_us` and `tower_backwards_us` — the victim's two tower forwards /
                   backwards on the padded batch without lengths (`padded_data`), with them (`lengths`) and on the dense
                   clouds (`dense_data`). Run from a checkout whose ops take no lengths (the parent of 8.19) it measures
                   that tree: `ragged` is then the padded pass and there is no `lengths` candidate; the two trees are run
                   alternated in pairs, a process each (profiles/ragged_tower_bench.json).
Replayed timings start after >= 150 ms of the same work. Writes profiles/ragged_bench.json.
Usage: python tools/bench_ragged.py [--out FILE] [--repeats N] [--towers]"""
import argparse
import importlib
import inspect
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_fused_defended import alternate, cw_ms, dev, victim  # noqa: E402
from helpers import unit_cloud  # noqa: E402

M = importlib.import_module
ops = M("3dpointcloudattack_amd.ops")
cloud_io = M("3dpointcloudattack_amd.dataset.cloud_io")


def attacker(model, trans, **kw):
    cwm = M("3dpointcloudattack_amd.attack.CW.CW_attack")
    u = "3dpointcloudattack_amd.attack.CW.CW_utils."
    return cwm.CW(model, trans, adv_func=M(u + "adv_utils").UntargetedLogitsAdvLoss(5.),
                  clip_func=M(u + "clip_utils").ClipPointsLinf(0.18), dist_func=M(u + "dist_utils").ChamferDist(), **kw)


def runner(atk, pcs, labels, lengths=None):
    torch.manual_seed(0)
    st = atk._begin(pcs, labels, lengths)
    atk._begin_binary_step(st)
    assert atk._capturable()
    return atk._make_runner(st), st


def stats(t, nd=4):
    return dict(median=round(statistics.median(t), nd), min=round(min(t), nd), max=round(max(t), nd),
                spread=round(max(t) - min(t), nd))


def tower_rows(model, xp, xd, lengths, repeats):
    """The victim's two tower forwards and its two tower backwards alone, in us: on the padded batch without lengths, with
    them (where ops takes them) and on the dense clouds."""
    pk = M("3dpointcloudattack_amd.model.pointnet").fused_pack(model)
    have_lengths = "lengths" in inspect.signature(ops.pointmlp3_max_fwd_raw).parameters
    lens = torch.from_numpy(np.asarray(lengths, dtype=np.int32)).to(dev)
    B = xp.shape[0]
    g_c, g_s = torch.randn(B, 1024, device=dev), torch.randn(B, 1024, device=dev)

    def forwards(x, **kw):
        s = ops.pointmlp3_max_fwd_raw(x, pk["tower_s"], True, want_masks=True, **kw)
        c = ops.pointmlp3_max_fwd_raw(x, pk["tower_c"], False, want_masks=True, **kw)
        return s, c

    def backwards(x, state, **kw):
        (_, idx_s, masks_s), (_, idx, masks), T, gx = state
        ops.pointmlp3_max_bwd_raw(x, pk["tower_c"], idx, g_c, masks, T=T, want_gT=True, out=gx, **kw)
        ops.pointmlp3_max_bwd_raw(x, pk["tower_s"], idx_s, g_s, masks_s, out=gx, accumulate=True, **kw)

    cands = {"padded_data": (xp, {}), "dense_data": (xd, {})}
    if have_lengths:
        cands["lengths"] = (xp, dict(lengths=lens))
    T = torch.eye(3, device=dev).repeat(B, 1, 1) + 0.1 * torch.randn(B, 3, 3, device=dev)
    fwd, bwd = {}, {}
    for name, (x, kw) in cands.items():
        state = forwards(x, **kw) + (T, torch.empty_like(x))
        fwd[name] = lambda x=x, kw=kw: forwards(x, **kw)
        bwd[name] = lambda x=x, kw=kw, state=state: backwards(x, state, **kw)
    return dict(tower_forwards_us=alternate(fwd, repeats), tower_backwards_us=alternate(bwd, repeats))


def towers_only(B, K, lengths, clouds, repeats):
    """--towers: the ragged and the dense CW iteration and the towers alone."""
    model, trans = victim(0), victim(1)
    data, lens = cloud_io.stack_ragged(clouds)
    dense = torch.from_numpy(np.stack([unit_cloud(np.random.default_rng(100 + b), K) for b in range(B)]))
    with torch.no_grad():
        labels = model(torch.from_numpy(data).transpose(1, 2).contiguous().to(dev))[0].argmax(1).cpu()
        dense_labels = model(dense.transpose(1, 2).contiguous().to(dev))[0].argmax(1).cpu()
    runs = {"ragged": runner(attacker(model, trans, sample_seeds=list(range(B))), torch.from_numpy(data), labels, lens)[0],
            "dense_riders_off": runner(attacker(model, trans, riders=False), dense, dense_labels)[0]}
    v = {k: [] for k in runs}
    for _ in range(repeats):
        for k, r in runs.items():
            v[k].append(cw_ms(r))
    out = dict(cw_ms={k: stats(t) for k, t in v.items()})
    xp, xd = torch.from_numpy(data).transpose(1, 2).contiguous().to(dev), dense.transpose(1, 2).contiguous().to(dev)
    out.update(tower_rows(model, xp, xd, lengths, repeats))
    return out


def cw_rows(B, K, lengths, clouds, repeats):
    model, trans = victim(0), victim(1)
    data, lens = cloud_io.stack_ragged(clouds)
    dense = torch.from_numpy(np.stack([unit_cloud(np.random.default_rng(100 + b), K) for b in range(B)]))
    with torch.no_grad():
        labels = model(torch.from_numpy(data).transpose(1, 2).contiguous().to(dev))[0].argmax(1).cpu()
        dense_labels = model(dense.transpose(1, 2).contiguous().to(dev))[0].argmax(1).cpu()
    runs = {"ragged": runner(attacker(model, trans, sample_seeds=list(range(B))), torch.from_numpy(data), labels, lens)[0],
            "dense_riders_off": runner(attacker(model, trans, riders=False), dense, dense_labels)[0],
            # the dense pass on the PADDED data (lengths ignored: wrong means, timing only): what the data itself costs
            "dense_pass_on_padded_data": runner(attacker(model, trans, riders=False), torch.from_numpy(data), labels)[0]}
    alone = [runner(attacker(model, trans, sample_seeds=[b], global_batch=B), torch.from_numpy(c)[None], labels[b:b + 1])[0]
             for b, c in enumerate(clouds)]
    v = {"ragged": [], "dense_riders_off": [], "dense_pass_on_padded_data": [], "alone_sum": []}
    for _ in range(repeats):
        for k, r in runs.items():
            v[k].append(cw_ms(r))
        v["alone_sum"].append(sum(cw_ms(r, 32) for r in alone))
    out = {k: stats(t) for k, t in v.items()}
    diff = out["ragged"]["median"] - out["dense_riders_off"]["median"]
    out["ragged_minus_dense_ms"] = round(diff, 4)
    out["larger_spread_ms"] = max(out["ragged"]["spread"], out["dense_riders_off"]["spread"])
    out["alone_over_ragged"] = round(out["alone_sum"]["median"] / out["ragged"]["median"], 2)
    out["points_counted_share"] = round(float(np.sum(lengths)) / (B * K), 3)
    # the victim's tower forward is data dependent (candidates of the screened max: every exact tie is rechecked, and a tile of
    # copies is nothing but ties): the two towers of the plain victim on the padded and on the dense clouds
    xp, xd = torch.from_numpy(data).transpose(1, 2).contiguous().to(dev), dense.transpose(1, 2).contiguous().to(dev)

    out.update(tower_rows(model, xp, xd, lengths, repeats))
    return out


def launch_rows(B, K, lengths, repeats):
    g = torch.Generator().manual_seed(1)
    ori = (torch.rand(B, 3, K, generator=g) - 0.5).to(dev)
    lens = torch.from_numpy(np.asarray(lengths, dtype=np.int32)).to(dev)
    ops.pad_ragged(ori, lens)

    def state():
        adv = ori + 0.05 * torch.randn(B, 3, K, generator=g).to(dev)
        ops.pad_ragged(adv, lens)
        z = lambda: torch.zeros(B, 3, K, device=dev)      # noqa: E731
        return dict(adv=adv, g=1e-3 * torch.randn(B, 3, K, generator=g).to(dev), m=z(), v=z(), oba=z(), iv=z(),
                    pred=torch.ones(B, dtype=torch.long, device=dev), label=torch.zeros(B, dtype=torch.long, device=dev),
                    bd=torch.full((B,), 1e10, device=dev), bs=torch.full((B,), -1, dtype=torch.long, device=dev),
                    obd=torch.full((B,), 1e10, device=dev), obs=torch.full((B,), -1, dtype=torch.long, device=dev),
                    w=torch.full((B,), 10., device=dev), dv=torch.zeros(B, device=dev),
                    nn=torch.randint(0, 256, (B, K), generator=g).to(torch.int32).to(dev),
                    step=torch.ones(1, dtype=torch.int32, device=dev))

    def update(s, ln):
        ops.cw_update(s["adv"], ori, s["pred"], s["label"], True, s["bd"], s["bs"], s["obd"], s["obs"], s["oba"], s["g"], s["m"],
                      s["v"], s["step"], 0.01, 0.18, input_val=s["iv"], dist_val=s["dv"], dist_kind=2, w=s["w"], nn_idx=s["nn"],
                      lengths=ln)

    sr, sd, x = state(), state(), ori.clone()
    t = alternate({"update_ragged": lambda: update(sr, lens), "update_dense": lambda: update(sd, None),
                   "pad": lambda: ops.pad_ragged(x, lens)}, repeats)
    return dict(update_us=dict(ragged=t["update_ragged"], dense=t["update_dense"],
                               ragged_minus_dense=round(t["update_ragged"]["median"] - t["update_dense"]["median"], 2)),
                pad_us=t["pad"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_bench.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--towers", action="store_true", help="the ragged and dense iteration and the towers alone, nothing else")
    a = ap.parse_args()
    B, K = 32, 1024
    rng = np.random.default_rng(2024)
    lengths = rng.integers(256, K + 1, B)
    clouds = [unit_cloud(rng, int(n)) for n in lengths]
    res = {"what": "tools/bench_ragged.py on one MI355X, one process; replayed hipGraphs after 150 ms of the same work, candidates "
                   f"timed alternately, {a.repeats} windows each (median, min, max; spread = max - min)",
           "device": torch.cuda.get_device_name(0), "B": B, "Kmax": K, "lengths": [int(n) for n in lengths]}
    if a.towers:
        res.update(towers_only(B, K, lengths, clouds, a.repeats))
    else:
        res.update(launch_rows(B, K, lengths, a.repeats))
        print(json.dumps({k: res[k] for k in ("update_us", "pad_us")}), flush=True)
        res["cw_ms"] = cw_rows(B, K, lengths, clouds, a.repeats)
    doc = json.dumps(res, indent=1)
    print(doc)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(doc + "\n")


if __name__ == "__main__":
    main()
