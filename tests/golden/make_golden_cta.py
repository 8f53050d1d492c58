#!/usr/bin/env python3
"""Generate tests/golden/cta.npz: the REAL reference's critical-point attack (attack/CTA/CTA.py, CTA_sumloss.py and their
utils) run on the CPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_cta.py

The reference modules are imported as they are. `torchvision` (imported by CTA.py, never used) is an inert stand-in in
sys.modules. CTA_sumloss.py calls `.cuda()` unconditionally (:150); while it runs, `torch.Tensor.cuda` is an identity
stand-in — no reference text is edited. The module-level name `np` of either module is a pass-through proxy that records
the arguments and results of `argsort` (contri, contr_index) and `mean` (the window means), which the reference only
prints. The victims are the reference's PointNetCls(k=40) with the project's seeded weights; a forward hook on fc3 fills
the activation dictionary, as Eval_CTA.py does.

Every case is also run through tests/cta_restatement.py, which must reproduce the reference bit for bit (mask, ranking,
records, window means, state, best_img); the per-step logits of sample 0 and the decisions are then taken from it.

Bands. The same run is repeated with the victim and the cloud in float64. band_x = 16 x the largest deviation of the
fp32 run from the float64 run in x (16: the multiple make_golden_iso.py and make_golden_defense.py use for a different
summation order on the device), for x in mask, contri (the ranked contributions), rec (the records), img (best_img), gap (the top-1/top-2 gap of sample 0's
logits at every step) — each with a floor of 16 x 2^-24 x the largest magnitude.
A case is REFUSED, and the next seed tried (at most 32 per case), when
  * any step's top-1/top-2 gap (which decides success and `second`) lies inside band_gap,
  * any window comparison has a margin inside band_rec — unless both windows hold one and the same value 50 times (a
    pass whose iterate does not move: level 0 of CTA.py unmasks nothing; every deterministic implementation then
    compares a number with itself),
  * the float64 run disagrees on a discrete outcome (state, level at exit, step counts, decisions, target class, which
    entries of the mask are exactly zero),
  * the fp32 run itself is not reproducible under another rounding: its mask leaves the float64 one by more than
    MASK_REL of the largest entry (a pooling winner changed inside the victim at some step), or its best_img by more
    than IMG_ABS (the trajectories parted) — the bands would then be wide enough to pass anything,
  * any max-pool channel of the victim (STN3d, STNkd, trunk; channels a ReLU zeroes left out) has, at any saliency step
    with alpha > 0, its winner less than POOL_REL = 16 x 2^-24 of the channel's largest magnitude ahead of the runner-up
    (float64 victim): which point wins, and so receives the channel's whole gradient, is then decided by the order
    in which an fp32 implementation sums a layer's 128 products, and a second fp32 implementation need not agree with
    the first (the float64 run agreeing with the CPU's fp32 run does not show that it would). At alpha = 0 every
    channel is an exact N-way tie, which the tie rule decides: that step is not looked at,
  * the case does not show what it is there for (`want`: a success, at least one break).
Only data is written.
"""
import contextlib
import copy
import importlib.util
import inspect
import io
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))                     # tests/: the restatement
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))    # oracle.ref_torch
from make_golden import OUT, REF, unit_cloud  # noqa: E402
import cta_restatement as rs  # noqa: E402

CTA_DIR = os.path.join(REF, "attack", "CTA")
MULT = 16.0
MASK_REL, IMG_ABS = 1e-4, 1e-3
POOL_REL = MULT * 2.0 ** -24         # 16 ulps of a channel's largest activation
MAX_SEEDS = 32


class Refused(Exception):
    pass


class NpProxy:
    """`np` for the reference module: numpy itself, with argsort and mean recorded."""

    def __init__(self, log):
        self._log = log

    def __getattr__(self, name):
        return getattr(np, name)

    def argsort(self, a, *args, **kw):
        r = np.argsort(a, *args, **kw)
        self._log["contri"], self._log["contr_index"] = np.array(a), np.array(r)
        return r

    def mean(self, a, *args, **kw):
        r = np.mean(a, *args, **kw)
        self._log["means"].append(r)
        return r


def load_reference():
    tv = types.ModuleType("torchvision")
    tv.models, tv.transforms = types.ModuleType("torchvision.models"), types.ModuleType("torchvision.transforms")
    sys.modules["torchvision"], sys.modules["torchvision.models"], sys.modules["torchvision.transforms"] = tv, tv.models, tv.transforms
    sys.path.insert(0, os.path.join(CTA_DIR, "utils"))       # CTA_sumloss.py: `import dis_utils_torch`
    mods = {}
    for name in ("CTA", "CTA_sumloss"):
        spec = importlib.util.spec_from_file_location("ref_" + name, os.path.join(CTA_DIR, name + ".py"))
        mods[name] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mods[name])
    return mods


@contextlib.contextmanager
def cuda_identity():
    had = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        yield
    finally:
        torch.Tensor.cuda = had


def victim(ft, seed, dtype):
    from model.pointnet import PointNetCls
    from oracle.ref_torch import seeded_state_dict
    m = PointNetCls(k=40, feature_transform=ft)
    m.load_state_dict(seeded_state_dict(m, seed))
    return m.eval().to(dtype)


def reference_run(mods, case, x, ori_cls, dtype):
    """The real act_max on a fresh victim; returns (result or None, log, mask)."""
    mod = mods["CTA" if case["variant"] == "cta" else "CTA_sumloss"]
    net = victim(case["ft"], case["wseed"], dtype)
    act, log = {}, dict(means=[])
    net.fc3.register_forward_hook(mod.layer_hook(act, "fc3"))
    mod.np = NpProxy(log)
    kw = dict(network=net, input=x.to(dtype).clone().requires_grad_(True), layer_activation=act, layer_name="fc3",
              ori_cls=ori_cls, alpha=torch.tensor(case["alpha"], dtype=dtype), beta=torch.tensor(0.0, dtype=dtype),
              target_att=case["target_att"], IG_steps=case["ig_steps"], n_points=case["n_points"], verbose=False,
              using_softmax_neuron=False, penalize_dis=False, optimizer=case["optimizer"])
    try:
        with contextlib.redirect_stdout(io.StringIO()), cuda_identity():
            out = mod.act_max(**kw)
            mask = mod.get_IG(x.to(dtype).clone(), ori_cls, net, case["ig_steps"], baseline="black")
    finally:
        mod.np = np
    return out, log, mask


def replay_decisions(means, targeted):
    """The reference's stop rule replayed on its own window means: (decisions, margins)."""
    dec, mar = [], []
    it = iter(means)
    last_o, last_t, windows = float("inf"), -float("inf"), 0
    for new_o in it:
        new_t = next(it) if targeted else None
        windows += 1
        brk = bool(new_o >= last_o) or windows * 25 >= 1500
        m = abs(float(new_o) - float(last_o))
        if targeted:
            brk = brk or bool(new_t <= last_t)
            m = min(m, abs(float(new_t) - float(last_t)))
        dec.append(int(brk)), mar.append(m)
        last_o, last_t = new_o, new_t
        if brk:
            last_o, last_t, windows = float("inf"), -float("inf"), 0
    return dec, mar


def pool_margin(case, x, steps):
    """The smallest relative top-2 margin of any live max-pool channel over the saliency steps with alpha > 0 (float64)."""
    net = victim(case["ft"], case["wseed"], torch.float64)
    seen = []
    towers = [(net.feat.stn.bn3, True), (net.feat.bn3, False)] + ([(net.feat.fstn.bn3, True)] if case["ft"] else [])
    for mod, relu in towers:
        mod.register_forward_hook(lambda m, i, o, relu=relu: seen.append((o.detach(), relu)))
    x = x.double()
    base = torch.ones_like(x) * torch.min(x)
    worst = np.inf
    for alpha in np.linspace(0, 1, steps)[1:]:
        seen.clear()
        with torch.no_grad():
            net(base + alpha * (x - base))
        for act, relu in seen:
            act = act[:2]                                    # rows >= set_size carry no cotangent
            top = act.topk(2, dim=2).values
            rel = (top[..., 0] - top[..., 1]) / act.abs().amax(dim=2).clamp_min(1e-300)
            live = top[..., 0] > 0 if relu else torch.ones_like(rel, dtype=torch.bool)
            if live.any():
                worst = min(worst, float(rel[live].min()))
    return worst


def top2_gap(z0):
    s = np.sort(np.asarray(z0, dtype=np.float64), axis=1)
    return s[:, -1] - s[:, -2]


def one_case(mods, case, seed):
    rng = np.random.default_rng(seed)
    B, N = case["B"], case["N"]
    x = torch.from_numpy((case.get("scale", 1.0) * np.stack([unit_cloud(rng, N).T for _ in range(B)])).astype(np.float32))
    net = victim(case["ft"], case["wseed"], torch.float32)
    with torch.no_grad():
        pred0 = int(net(x)[0][0].argmax())
    ori_cls = 0 if case.get("ori0") else pred0
    if not case.get("ori0") and ori_cls == 0:
        raise Refused("the cloud's class is 0, which is the falsy-branch case's business")
    out, log, mask = reference_run(mods, case, x, ori_cls, torch.float32)
    out64, log64, mask64 = reference_run(mods, case, x, ori_cls, torch.float64)
    targeted = case["target_att"] is not False
    # the restatement must be the reference, bit for bit
    fwd = rs.hooked_forward(net, net.fc3)
    r = rs.run(fwd, x, ori_cls, torch.tensor(case["alpha"]), variant=case["variant"], target_att=case["target_att"],
               IG_steps=case["ig_steps"], n_points=case["n_points"], optimizer=case["optimizer"])
    assert np.array_equal(r["mask"], mask) and np.array_equal(r["contri"], log["contri"])
    if r["steps"] == 0:
        raise Refused("no positive contribution: the loop never runs")
    assert np.array_equal(r["contr_index"], log["contr_index"])
    means = np.array([float(m) for m in log["means"]])
    rmeans = np.array([v for row in r["means"] for v in (row if targeted else row[:1])])
    assert np.array_equal(means, rmeans), (means, rmeans)
    dec, margins = replay_decisions(log["means"], targeted)
    assert dec == r["decisions"]
    if out is None:
        assert r["state"] is None
        state, best, ol, ml = "None", r["best_img"], r["ori_logits"], r["max_other_logits"]
    else:
        state, best, ol, ml = out[0], out[1].detach(), out[2], out[3]
        assert r["state"] == state and torch.equal(r["best_img"], best)
    assert np.array_equal(np.array(ol), np.array(r["ori_logits"])) and np.array_equal(np.array(ml), np.array(r["max_other_logits"]))
    # the float64 run: discrete outcomes and deviations
    net64 = victim(case["ft"], case["wseed"], torch.float64)
    r64 = rs.run(rs.hooked_forward(net64, net64.fc3), x.double(), ori_cls, torch.tensor(case["alpha"], dtype=torch.float64),
                 variant=case["variant"], target_att=case["target_att"], IG_steps=case["ig_steps"], n_points=case["n_points"],
                 optimizer=case["optimizer"])
    st64 = "None" if out64 is None else out64[0]
    dec64, _ = replay_decisions(log64["means"], targeted)
    if (st64, dec64, r64["num_p_per"], r64["steps"], r64["cur_step"], r64["tar_cls"]) != \
            (state, dec, r["num_p_per"], r["steps"], r["cur_step"], r["tar_cls"]):
        raise Refused(f"float64 disagrees: {st64} {r64['num_p_per']} {r64['steps']} vs {state} {r['num_p_per']} {r['steps']}")
    if not np.array_equal(log64["contr_index"], log["contr_index"]) and case["variant"] == "cta":
        raise Refused("float64 ranks the [3,B] table differently")
    z0, z064 = np.array(r["z0"]), np.array(r64["z0"])

    def band(a, b):
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        return MULT * max(float(np.max(np.abs(a - b))), 2.0 ** -24 * float(np.max(np.abs(b))))
    ol64 = out64[2] if out64 is not None else r64["ori_logits"]
    ml64 = out64[3] if out64 is not None else r64["max_other_logits"]
    best64 = out64[1].detach() if out64 is not None else r64["best_img"]
    bands = dict(band_mask=band(mask, mask64), band_rec=max(band(z0, z064), band(ol, ol64), band(ml, ml64)),
                 band_img=band(best.numpy(), best64.numpy()), band_gap=band(top2_gap(z0), top2_gap(z064)),
                 band_contri=band(log["contri"], log64["contri"]))
    if not np.array_equal(mask == 0.0, mask64 == 0.0):
        raise Refused("float64 has other exact zeros in the mask")
    if bands["band_mask"] > MULT * MASK_REL * np.max(np.abs(mask64)) or bands["band_img"] > MULT * IMG_ABS:
        raise Refused(f"not reproducible: band_mask {bands['band_mask']:.2e} (largest entry {np.max(np.abs(mask64)):.2e}), "
                      f"band_img {bands['band_img']:.2e}")
    pm = pool_margin(case, x, case["ig_steps"])
    if pm <= POOL_REL:
        raise Refused(f"a max-pool channel's winner leads by {pm:.2e} of the channel's magnitude (POOL_REL {POOL_REL:.2e})")
    gaps = top2_gap(z0)
    if gaps.min() <= bands["band_gap"]:
        raise Refused(f"a step has top-2 gap {gaps.min():.3e} inside band_gap {bands['band_gap']:.3e}")
    # window margins; a pass that did not move compares a number with itself
    pos = 0
    lvl_start = 0
    for i, (d, m) in enumerate(zip(dec, margins)):
        hi = pos + 25
        still = np.all(z0[lvl_start:hi] == z0[lvl_start])
        if np.isfinite(m) and m <= bands["band_rec"] and not still:
            raise Refused(f"window {i}: margin {m:.3e} inside band_rec {bands['band_rec']:.3e}")
        pos = hi
        if d:
            lvl_start = pos
    want = case.get("want", "Suc")
    if state != want or (case.get("want_break", True) and sum(dec) == 0):
        raise Refused(f"state {state}, {sum(dec)} breaks: not the regime the case is there for")
    fx = dict(x=x.numpy(), ori_cls=np.int64(ori_cls), seed=np.int64(seed), mask=mask, mask64=mask64, contri=log["contri"],
              contr_index=log["contr_index"], tar_cls=np.int64(r["tar_cls"]), ori_logits=np.array(ol, dtype=np.float32),
              max_other_logits=np.array(ml, dtype=np.float32), z0=z0.astype(np.float32), means=np.array(r["means"]),
              decisions=np.array(dec, dtype=np.int64), margins=np.array(margins), num_p_per=np.int64(r["num_p_per"]),
              steps=np.int64(r["steps"]), cur_step=np.int64(r["cur_step"]), state=np.array(state), best_img=best.numpy(),
              ori_logits64=np.array(ol64, dtype=np.float64), best_img64=best64.numpy(), gap_min=np.float64(gaps.min()), pool_margin=np.float64(pm),
              alpha=np.float64(case["alpha"]), ig_steps=np.int64(case["ig_steps"]), n_points=np.int64(case["n_points"]),
              ft=np.int64(case["ft"]), wseed=np.int64(case["wseed"]), variant=np.array(case["variant"]),
              optimizer=np.array(case["optimizer"]), target_att=np.array(str(case["target_att"])),
              zero_points=np.all(mask == 0.0, axis=0), **{k: np.float64(v) for k, v in bands.items()})
    # the alpha = 0 step on its own: which point receives the tie's gradient
    g0 = rs.vanilla_mask(fwd, torch.ones_like(x) * torch.min(x), ori_cls)
    fx["tie_receivers"] = np.flatnonzero(np.any(g0 != 0.0, axis=(0, 2)))
    return fx


CASES = {
    "cta_adam": dict(variant="cta", B=2, N=64, ig_steps=5, alpha=1e-4, optimizer="Adam", target_att=False, n_points=1, ft=0, wseed=0),
    "cta_momentum_tar": dict(variant="cta", B=2, N=100, ig_steps=2, alpha=0.05, optimizer="Momentum", target_att="second", n_points=1,
                             ft=0, wseed=0),
    # scale 0.5: at unit scale this seeded feature-transform victim's logits reach several hundred, where one fp32 ulp
    # of a logit is already 6e-5 (tests/test_pointnet_ft_gpu.py scales its clouds the same way)
    "cta_ft": dict(variant="cta", B=2, N=64, ig_steps=5, alpha=1e-4, optimizer="Adam", target_att=False, n_points=1, ft=1, wseed=1,
                   scale=0.5),
    "cta_b3": dict(variant="cta", B=3, N=64, ig_steps=5, alpha=1e-4, optimizer="Adam", target_att=False, n_points=1, ft=0, wseed=0),
    # ori_cls = 0 takes the saliency's falsy branch (the multi-hot of every row's top-1); the victim does not predict
    # class 0 for the cloud, so the loop succeeds at its first step
    "cta_ori0": dict(variant="cta", B=2, N=256, ig_steps=2, alpha=1e-4, optimizer="Adam", target_att=False, n_points=1, ft=0, wseed=0,
                     ori0=True, want_break=False),
    # (at alpha = 1e-4 this case's long passes part from their float64 twins; at 1e-3 level 1 succeeds within its first
    # window, so the level changes of this variant are pinned by the Momentum case)
    # N = 256 sits with 2 steps (cta_ori0) and 25 steps with N = 64: at N = 256 and 25 steps together no seed among 32 is
    # admissible — among 25 x 2 x 2048 pooled channels of 256 nearly coincident points one always sits on a near-tie
    "sumloss_adam": dict(variant="sumloss", B=2, N=64, ig_steps=25, alpha=1e-3, optimizer="Adam", target_att=False, n_points=1,
                         ft=0, wseed=0, want_break=False),
    # CTA_sumloss.py's targeted loss depends on the LAST sample only while success is read from sample 0, which therefore
    # never moves: a targeted run ends in the reference's IndexError. The Momentum case of this variant is untargeted.
    "sumloss_momentum": dict(variant="sumloss", B=2, N=100, ig_steps=5, alpha=0.3, optimizer="Momentum", target_att=False, n_points=1,
                             ft=0, wseed=0),
}


def signatures(mods):
    from attack.CTA.utils.integrated_gradients import IntegratedGradients
    from attack.CTA.utils.saliency_mask import SaliencyMask
    from attack.CTA.utils.vanilla_gradient import VanillaGradient
    fns = {"CTA.act_max": mods["CTA"].act_max, "CTA.get_IG": mods["CTA"].get_IG, "CTA.layer_hook": mods["CTA"].layer_hook,
           "CTA.sampling": mods["CTA"].sampling, "CTA_sumloss.act_max": mods["CTA_sumloss"].act_max,
           "CTA_sumloss.get_IG": mods["CTA_sumloss"].get_IG, "SaliencyMask.__init__": SaliencyMask.__init__,
           "SaliencyMask.get_mask": SaliencyMask.get_mask, "VanillaGradient.get_mask": VanillaGradient.get_mask,
           "IntegratedGradients.get_mask": IntegratedGradients.get_mask}
    sig = {k: str(inspect.signature(v)) for k, v in fns.items()}
    sig["CTA.stop_threshold"], sig["CTA.noise_weight"] = repr(mods["CTA"].stop_threshold), repr(mods["CTA"].noise_weight)
    return sig


def main():
    only = [a.split(":")[0] for a in sys.argv[1:]]          # name or name:alpha — a trial run, nothing is written
    for a in sys.argv[1:]:
        if ":" in a:
            CASES[a.split(":")[0]]["alpha"] = float(a.split(":")[1])
    mods = load_reference()
    fx = {}
    for name, case in CASES.items():
        if only and name not in only:
            continue
        for seed in range(MAX_SEEDS):
            try:
                r = one_case(mods, case, 1000 * (1 + list(CASES).index(name)) + seed)
            except IndexError as e:              # CTA_sumloss.py runs past its table when no level succeeds
                print(f"{name}: seed {seed} refused: the reference raises IndexError: {e}")
                continue
            except Refused as e:
                print(f"{name}: seed {seed} refused: {e}")
                continue
            print(f"{name}: seed {seed}: {r['state']} level {r['num_p_per']} steps {r['steps']} cur {r['cur_step']} "
                  f"decisions {r['decisions'].tolist()} tar {r['tar_cls']} gap_min {r['gap_min']:.3e} bands "
                  + " ".join(f"{k[5:]} {float(r[k]):.2e}" for k in sorted(r) if k.startswith("band_"))
                  + f" tie_receivers {r['tie_receivers'].tolist()} zero points {int(r['zero_points'].sum())}")
            fx.update({f"{name}/{k}": v for k, v in r.items()})
            break
        else:
            raise SystemExit(f"{name}: no seed among {MAX_SEEDS} gives an admissible case")
    sig = signatures(mods)
    fx["cases"] = np.array([n for n in CASES if not only or n in only])
    fx["signatures"] = np.array([f"{k}{v}" if v.startswith("(") else f"{k}={v}" for k, v in sorted(sig.items())])
    if not only:
        path = os.path.join(OUT, "cta.npz")
        np.savez_compressed(path, **fx)
        print("cta.npz:", len(fx), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
