#!/usr/bin/env python3
"""Generate tests/golden/siadv_query.npz: the REAL reference's simba_attack and shape_invariant_query_attack
(attack/SIadv/SIadv_attack.py:343-414, 503-624) on the CPU, one cloud at a time.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_siadv_query.py

The reference module is loaded by make_golden_siadv.py's load_reference() (the CPU shims and the open3d STAND-IN described
there; the stand-in is handed the coordinates [1,N,3], which is what `points` is for the shape-invariant query attack
here). Nothing of the reference is edited; it is observed from outside:

  * np.random.shuffle is wrapped to keep the shuffled [3N,2] basis list of simba_attack (the table);
  * the module-level name `sorted` is wrapped to keep the ranked point list of shape_invariant_query_attack;
  * CWLoss is wrapped to keep every loss in call order; the steps are rebuilt from them by the loop's own rule and the
    rebuild is checked against the query_costs the reference returns;
  * in the float64 run `Tensor.float` keeps float64 (the two re-evaluations at the end of the shape-invariant attack call
    .float() on the cloud before the float64 victim); stdout of the reference's prints is discarded.
The loss of a second try the reference never evaluated (its first try was accepted) is filled in from
tests/siadv_query_restatement.py run on the same table, after that restatement has matched every loss the reference
did compute to within band_loss.

Clouds: B = 4 ellipsoid clouds (make_golden_siadv.ellipsoid_clouds) cut to N = 64; seeded PointNets 3 (surrogate) and 4
(target), 40 classes. Labels: the target model's own prediction, except the cloud with the smallest top-1 / top-2 gap of
the batch, which gets its runner-up class (it returns early). Cases: simba (L = 192), ours, ours_top5 (L = 64).

Every case searches its own seed (the seed of its clouds and of np.random). Stored: step_size, eps, signs (tuple({s, -s})
as evaluated here), and per case <c>: points, target, np_seed (np.random.seed before the clouds, run in order), tab [B,L] int32 (simba: 3 * idx + channel; zeros for a cloud that returned
early), early [B], loss [B,L,2], accepted [B,L] (0 / 1, -1 neither, -2 not reached), best [B,L], query_costs, adv_target,
adv_points, band_loss, band_P; for ours also nrm, dir, key (the normals, directions and rankings the reference used).

band_loss / band_P: 16x the largest deviation between the fp32 run and the same run in float64 (both models and all
tensor types in double), the multiple every golden generator here uses. A seed is REFUSED, and the next one tried, unless
every decision loss - best_loss is farther from 0 than band_loss, fp32 and float64 take the same accept sequence, and
among the simba clouds one returns early, one succeeds before its table ends after at least one rejected first try,
and one exhausts its table. Only data is written.
"""
import contextlib
import copy
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import OUT, _seeded_pointnet  # noqa: E402
import make_golden_siadv as G  # noqa: E402
import siadv_query_restatement as Q  # noqa: E402

NCLS, B, N = 40, 4, 64
STEP, EPS = 4.0, 0.16
CASES = {"simba": dict(method="simba", top5=False), "ours": dict(method="ours", top5=False),
         "ours_top5": dict(method="ours", top5=True)}


def rebuild_steps(losses, L):
    """(accepted [L], loss [L,2], best [L], consumed) from the losses in call order, by the loop's own rule."""
    acc, ls, bs = np.full(L, -2, np.int64), np.full((L, 2), np.nan), np.full(L, np.nan)
    best, i, k = -999., 0, 0
    while best < 0 and i < L:
        acc[i] = -1
        for t in range(2):
            ls[i, t] = losses[k]
            k += 1
            if ls[i, t] > best:
                best, acc[i] = ls[i, t], t
                break
        bs[i] = best
        i += 1
    return acc, ls, bs, k


def run_reference(mod, surrogate, target_model, points, target, case, double, np_seed):
    dt = torch.float64 if double else torch.float32
    real_float, real_cuda_float, real_tfloat = torch.FloatTensor, torch.cuda.FloatTensor, torch.Tensor.float
    real_shuffle = np.random.shuffle
    torch.set_default_dtype(dt)
    if double:
        torch.FloatTensor = torch.cuda.FloatTensor = torch.DoubleTensor
        torch.Tensor.float = lambda self, *a, **k: self.double()
    tables, ranked = [], []

    def shuffle(a):
        real_shuffle(a)
        if getattr(a, "ndim", 0) == 2:
            tables.append(np.array(a))

    def sorted_(it, **kw):
        out = sorted(it, **kw)
        ranked.append(out)
        return out

    np.random.shuffle, mod.sorted = shuffle, sorted_
    try:
        atk = object.__new__(mod.PointCloudAttack)
        atk.args, atk.device = None, torch.device("cpu")
        atk.eps, atk.step_size, atk.max_steps = EPS, STEP, 0
        atk.num_class, atk.top5_attack, atk.normal = NCLS, case["top5"], False
        atk.attack_method, atk.defense_method = case["method"], None
        atk.wb_classifier, atk.classifier = surrogate, target_model
        real_l = atk.CWLoss
        frame = case["method"] == "ours"
        L = N if frame else 3 * N
        r = dict(tab=[], early=[], loss=[], accepted=[], best=[], query_costs=[], adv_target=[], adv_points=[], nrm=[], dir=[], key=[])
        np.random.seed(np_seed)
        for b in range(B):
            losses = []

            def cwloss(*a, **kw):
                out = real_l(*a, **kw)
                losses.append(float(out.detach()))
                return out

            atk.CWLoss = cwloss
            del tables[:], ranked[:]
            pts = torch.from_numpy(points[b:b + 1]).to(dt)
            nrm = []
            real_n = atk.get_normal_vector
            atk.get_normal_vector = lambda p: nrm.append(real_n(p)) or nrm[-1]
            with contextlib.redirect_stdout(io.StringIO()):
                adv, adv_target, cost = atk.run(pts, torch.from_numpy(target[b:b + 1]))
            atk.get_normal_vector = real_n
            if frame:
                losses = losses[1:]                                  # the first call is the surrogate's loss
                order = np.array([c[0] for c in ranked[0]], np.int32)
                dirs = np.zeros((N, 3))
                key = np.zeros(N)
                for c in ranked[0]:
                    dirs[c[0]], key[c[0]] = c[1][0].numpy(), c[2]
                n0 = nrm[0] / torch.sqrt(torch.sum(nrm[0] ** 2, dim=-1, keepdim=True))
                r["tab"].append(order), r["dir"].append(dirs), r["key"].append(key), r["nrm"].append(n0[0].numpy())
                early = False
            else:
                early = not tables
                tab = np.zeros(L, np.int32) if early else (3 * tables[0][:, 1] + tables[0][:, 0]).astype(np.int32)
                r["tab"].append(tab)
            acc, ls, bs, used = rebuild_steps(losses, L) if not early else (np.full(L, -2), np.full((L, 2), np.nan), np.full(L, np.nan), 0)
            assert used == len(losses) == int(cost) - 1, (used, len(losses), cost)
            r["early"].append(early), r["loss"].append(ls), r["accepted"].append(acc), r["best"].append(bs)
            r["query_costs"].append(int(cost)), r["adv_target"].append(int(adv_target)), r["adv_points"].append(adv[0].detach().numpy())
        return {k: np.stack(v) for k, v in r.items() if v}
    finally:
        torch.set_default_dtype(torch.float32)
        torch.FloatTensor, torch.cuda.FloatTensor, torch.Tensor.float = real_float, real_cuda_float, real_tfloat
        np.random.shuffle = real_shuffle
        del mod.sorted


def restate(surrogate, target_model, points, target, case, r, dt):
    P, tg = torch.from_numpy(points).to(dt), torch.from_numpy(target)
    signs = torch.tensor(Q.sign_order(STEP), dtype=dt)
    frame = None
    if case["method"] == "ours":
        frame = (torch.from_numpy(r["nrm"]).to(dt), torch.from_numpy(r["dir"]).to(dt))
    return Q.run_query(target_model, P, tg, r["tab"], signs, case["top5"], frame, active=~r["early"])


def generate(mod, sur, tgt, sur64, tgt64, name, seed):
    """The arrays of case `name` for the clouds of one seed, or None when the seed is refused."""
    case = CASES[name]
    rng = np.random.default_rng(seed)
    points = np.ascontiguousarray(G.ellipsoid_clouds(rng)[:, :N, :3])
    with torch.no_grad():
        logp = tgt(torch.from_numpy(points).transpose(1, 2).contiguous())[0]
    top2 = logp.topk(2)
    target = top2[1][:, 0].numpy().astype(np.int64)
    b_early = int((top2[0][:, 0] - top2[0][:, 1]).argmin())
    target[b_early] = int(top2[1][b_early, 1])
    r32 = run_reference(mod, sur, tgt, points, target, case, False, seed)
    r64 = run_reference(mod, sur64, tgt64, points, target, case, True, seed)
    try:
        assert np.array_equal(r32["tab"], r64["tab"]), "fp32 and float64 rank / draw different tables"
        assert np.array_equal(r32["accepted"], r64["accepted"]), "fp32 and float64 take different accept sequences"
        both = ~np.isnan(r32["loss"])
        dev_loss = float(np.abs(r32["loss"][both] - r64["loss"][both]).max()) if both.any() else 0.0
        dev_P = float(np.abs(r32["adv_points"].astype(np.float64) - r64["adv_points"]).max())
        band_loss, band_P = 16.0 * max(dev_loss, 2.0 ** -24), 16.0 * max(dev_P, 2.0 ** -24)
        prev = np.concatenate([np.full((B, 1), -999.), r32["best"][:, :-1]], 1)      # best_loss before each step
        m = float(np.nanmin(np.abs(r32["loss"] - prev[:, :, None])))
        assert m > band_loss, f"a decision sits {m:.3e} from best_loss (band_loss {band_loss:.3e})"
        if name == "simba":
            acc, early = r32["accepted"], r32["early"]
            ends = (acc != -2).sum(1)
            mid = [bool((not early[b]) and ends[b] < 3 * N and r32["best"][b, ends[b] - 1] >= 0 and (acc[b, :ends[b]] != 0).any())
                   for b in range(B)]
            full = [bool((not early[b]) and ends[b] == 3 * N and r32["best"][b, -1] < 0) for b in range(B)]
            assert early.any() and any(mid) and any(full), f"early {early.tolist()} mid {mid} exhausted {full}"
        for dt, s, t, rr in ((torch.float32, sur, tgt, r32), (torch.float64, sur64, tgt64, r64)):
            q = restate(s, t, points, target, case, rr, dt)
            assert np.array_equal(q["accepted"].numpy(), rr["accepted"]), f"the restatement ({dt}) takes another accept sequence"
            d = np.abs(q["losses"].double().numpy() - rr["loss"])
            assert float(np.nanmax(d, initial=0.0)) <= band_loss, f"restatement losses off by {np.nanmax(d):.3e}"
            if dt == torch.float32:
                filled = np.where(np.isnan(rr["loss"]), q["losses"].double().numpy(), rr["loss"])
    except AssertionError as e:
        print(f"seed {seed}: {name} refused: {e}")
        return None
    r32["loss"] = filled
    fx = {f"{name}_points": points, f"{name}_target": target, f"{name}_np_seed": np.int64(seed)}
    for k, v in r32.items():
        fx[f"{name}_{k}"] = v.astype(np.float32) if v.dtype == np.float64 and k in ("adv_points", "nrm", "dir", "key") else v
    fx[f"{name}_band_loss"], fx[f"{name}_band_P"] = np.float64(band_loss), np.float64(band_P)
    print(f"{name} (seed {seed}): dev_loss {dev_loss:.3e} band_loss {band_loss:.3e} band_P {band_P:.3e} margin {m:.3e} "
          f"costs {r32['query_costs'].tolist()} adv_target {r32['adv_target'].tolist()} target {target.tolist()} "
          f"early {r32['early'].tolist()}")
    return fx


def main():
    from model.pointnet import PointNetCls
    mod = G.load_reference()
    sur, sha_s = _seeded_pointnet(PointNetCls, NCLS, 3)
    tgt, sha_t = _seeded_pointnet(PointNetCls, NCLS, 4)
    sur64, tgt64 = copy.deepcopy(sur).double().eval(), copy.deepcopy(tgt).double().eval()
    fx = {"cases": np.array(list(CASES)), "step_size": np.float64(STEP), "eps": np.float64(EPS),
          "signs": np.array(Q.sign_order(STEP), np.float64)}
    for name in CASES:                       # every case searches its own seed: the clouds and the np.random seed
        for seed in range(20, 420):
            part = generate(mod, sur, tgt, sur64, tgt64, name, seed)
            if part is not None:
                fx.update(part)
                break
        else:
            raise SystemExit(f"{name}: no seed passed")
    fx.update({"sha256_surrogate": np.array(sha_s), "sha256_target": np.array(sha_t), "weights_seeds": np.array([3, 4])})
    path = os.path.join(OUT, "siadv_query.npz")
    np.savez_compressed(path, **fx)
    print("siadv_query.npz:", len(fx), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
