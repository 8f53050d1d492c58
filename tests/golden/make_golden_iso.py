#!/usr/bin/env python3
"""Generate tests/golden/iso.npz: the REAL reference's isometry attack (attack/ISO: TSI + CTRI) run on the CPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_iso.py

The reference's iso_attack / thompson_sample / isometry_init modules are imported as they are. Inert stand-ins for
`open3d` and `iso_utils` (a progress bar and two log helpers, none of which computes anything) sit in sys.modules while
they load, and iso_attack's `device` global, which exists only under its `__main__`, is set to the CPU. The victim is the
reference's PointNetCls(k=40) with the project's seeded weights. Each case processes its clouds in order the way the
reference's `__main__` does (pre-check, TSI, re-evaluation, CTRI), with one shared Thompson posterior. The ISOnet wrapper
is built once per case BEFORE torch is seeded: its nn.Linear initialisation draws from the same generator and is
overwritten by TSI's matrix before any use, so a cloud consumes exactly `steps` normal draws.

Stored per case <c> (clouds of N = 64 and N = 256, 6 each): x, label, args (num_steps, step_size, LAMBDA, target, kappa,
num_init, d, a, b), seed (numpy and torch); attacked, true_prob_before, tsi_all (every float64 matrix TSI drew, in
order), tsi_W (the chosen matrices: float32 values, as the reference hands them on), tsi_draws, init_success,
alpha / beta after the case, W after CTRI, steps, correct, rates2 / indices2 (first two sorted entries), true_prob_after, penalty, next_np / next_torch (the next draw of either generator) and the band. `signatures` lists the
reference functions' signatures as strings.

  band_W, band_gap   the same trajectories are run with the reference in float64 (the victim and W in double; the
      spectral penalty, which the reference cannot evaluate in double and which never reaches the gradient, replaced by
      a stand-in that makes the same draw). dev_W is the largest deviation of the fp32 run's final W, dev_gap that of its
      top-1/top-2 gap over every evaluation; the bands are 16x those (the multiple make_golden_defense.py uses for a
      different summation order on the device).

A case is REFUSED — the next seed is tried — if any evaluation of the run has a top-1/top-2 gap inside band_gap, if any Adam
step sees a gradient component with |g| < 1e-4 max|g|, if the float64 run disagrees on a discrete outcome, if the
reference's own fp32 trajectory leaves band_W (or changes its outcome) when every layer output of the victim carries one
ulp of relative noise (PROBES repetitions: such a run sits on a tie inside the victim, which the two rules above do not
see, and is not reproducible under any other rounding), or if the case does not show the regime it is there for. Only data is written.
"""
import copy
import importlib.util
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, REF, _seeded_pointnet, unit_cloud  # noqa: E402

ISO_DIR = os.path.join(REF, "attack", "ISO")
NCLOUD = 6


def load_reference():
    o3d = types.ModuleType("open3d")
    utils = types.ModuleType("iso_utils")
    utils.progress_bar = lambda *a, **k: None
    utils.adjust_lr_steep = lambda *a, **k: None
    utils.log_row = lambda *a, **k: None
    sys.modules["open3d"], sys.modules["iso_utils"] = o3d, utils
    sys.path.insert(0, ISO_DIR)
    import thompson_sample
    import isometry_init
    # by file path: a directory of the same name sits next to iso_attack.py and would win a plain import
    spec = importlib.util.spec_from_file_location("ref_iso_attack", os.path.join(ISO_DIR, "iso_attack.py"))
    iso_attack = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(iso_attack)
    iso_attack.device = torch.device("cpu")
    thompson_sample.device = torch.device("cpu")
    real = isometry_init.rotation_xyz

    def recording(a, b):                                   # every float64 matrix TSI draws, in order
        m = real(a, b)
        DRAWN.append(m.copy())
        return m
    recording.__wrapped_real__ = real
    isometry_init.rotation_xyz = recording
    return iso_attack, thompson_sample


DRAWN = []


class Rec(torch.nn.Module):
    """The victim, recording the top-1/top-2 gap of every evaluation (and the float64 twin's on the same input)."""

    def __init__(self, model, twin=None):
        super().__init__()
        self.model, self.twin, self.gaps, self.gaps64 = model, [twin], [], []

    def forward(self, x):
        out = self.model(x)
        if PROBE["on"]:
            return out
        s = out[0].detach().sort(1, descending=True)[0]
        self.gaps.append(float(s[0, 0] - s[0, 1]))
        if self.twin[0] is not None:
            with torch.no_grad():
                s = self.twin[0](x.detach().double())[0].sort(1, descending=True)[0]
            self.gaps64.append(float(s[0, 0] - s[0, 1]))
        return out


class Refused(Exception):
    pass


PROBE = {"on": False, "gen": None, "rel": 2.0 ** -23}
PROBES = 16


def _round_off(mod, inp, out):
    """Forward hook of the fp32 victim's conv / linear layers while a probe runs: one ulp of relative noise on every
    output, from a generator of its own — what another summation order inside the victim amounts to."""
    if not PROBE["on"]:
        return None
    return out + PROBE["rel"] * out.abs() * torch.randn(out.shape, generator=PROBE["gen"])


def run_case(iso, ts, model, model64, x, label, a, seed):
    """One pass over the clouds as the reference's __main__ makes it. a: dict of args."""
    args = types.SimpleNamespace(**a)
    rec = Rec(model, model64)
    model_v = iso.ISOnet(model=rec)
    model_v.eval()
    rec64 = Rec(model64)
    model_v64 = iso.ISOnet(model=rec64).double()
    model_v64.eval()
    grads, grads64 = [], []
    model_v.iso.weight.register_hook(lambda g: grads.append(g.detach().clone()))
    model_v64.iso.weight.register_hook(lambda g: grads64.append(g.detach().clone()))
    del DRAWN[:]
    np.random.seed(seed)
    torch.manual_seed(seed)
    thompson = ts.BernThompson(ts.environment(d=args.d, a0=args.a, b0=args.b))
    n = x.shape[0]
    r = dict(attacked=np.zeros(n, bool), true_prob_before=np.zeros(n, np.float32), tsi_W=np.tile(np.eye(3), (n, 1, 1)),
             tsi_draws=np.zeros(n, np.int64), init_success=np.zeros(n, bool), W=np.tile(np.eye(3, dtype=np.float32), (n, 1, 1)),
             steps=np.zeros(n, np.int64), correct=np.zeros(n, np.int64), rates2=np.zeros((n, 2), np.float32),
             indices2=np.zeros((n, 2), np.int64), true_prob_after=np.zeros(n, np.float32), penalty=np.zeros(n))
    dev_W = 0.0
    gap_pairs = []                                       # (fp32 gap, float64 gap) of corresponding CTRI evaluations
    ctri = []                                            # (cloud, start W, final W, correct, steps) of every CTRI run
    for i in range(n):
        obj, lab = torch.from_numpy(x[i:i + 1]), torch.from_numpy(label[i:i + 1])
        _, correct, rates, indices = iso.logits_info(obj, lab, rec)
        r["true_prob_before"][i] = rates[(indices == lab.item()).nonzero().item()].item()
        r["rates2"][i], r["indices2"][i] = rates[:2].detach().numpy(), indices[:2].numpy()
        r["true_prob_after"][i] = r["true_prob_before"][i]
        if correct == 0:
            continue
        r["attacked"][i] = True
        before = thompson.alpha.sum() + thompson.beta.sum()
        model_v.iso.weight.data, thompson = iso.thompson_sample_attack(thompson, obj, lab, model_v, args.num_init)
        r["tsi_draws"][i] = int(round(thompson.alpha.sum() + thompson.beta.sum() - before))
        r["tsi_W"][i] = model_v.iso.weight.data.double().numpy()        # float32 values (torch.Tensor(matrix)), exactly
        _, correct, rates, indices = iso.logits_info(obj, lab, model_v)
        W0 = model_v.iso.weight.data.clone()
        penalty, steps = 0, 0
        if correct == 0:
            r["init_success"][i] = True
        elif args.attack_type == 'combine':
            k0, g0 = len(rec.gaps), len(grads)
            correct, rates, indices, model_v, penalty, steps = iso.gradient_attack(obj, lab, model_v, args)
            if correct == 1:
                penalty = 0
            # the same trajectory in float64, torch's generator put back afterwards
            state = torch.get_rng_state()
            real = iso.spectral_penalty
            iso.spectral_penalty = lambda W, iters=30: (torch.empty(3).normal_(0, 1).sum() * 0).double()
            try:
                model_v64.iso.weight.data = W0.double()
                k64, g64 = len(rec64.gaps), len(grads64)
                c64, _, i64, _, _, s64 = iso.gradient_attack(obj.double(), lab, model_v64, args)
            finally:
                iso.spectral_penalty = real
                torch.set_rng_state(state)
            if (c64, s64, int(i64[0])) != (correct, steps, int(indices[0])):
                raise Refused(f"cloud {i}: the float64 run ends differently ({c64}, {s64}) vs ({correct}, {steps})")
            dev_W = max(dev_W, float((model_v.iso.weight.data.double() - model_v64.iso.weight.data).abs().max()))
            ctri.append((i, W0, model_v.iso.weight.data.clone(), correct, steps))
            # gradient_attack evaluates twice per step when target != 0: compare evaluation by evaluation
            a32, a64 = rec.gaps[k0:], rec64.gaps[k64:]
            assert len(a32) == len(a64), (len(a32), len(a64))
            gap_pairs += list(zip(a32, a64))
            for g in grads[g0:] + grads64[g64:]:
                g = g.abs()
                if float(g.min()) < 1e-4 * float(g.max()):
                    raise Refused(f"cloud {i}: an Adam step sees |g| = {float(g.min()):.3e} < 1e-4 * {float(g.max()):.3e}")
        r["W"][i] = model_v.iso.weight.data.numpy()
        r["steps"][i], r["correct"][i], r["penalty"][i] = steps, correct, penalty
        r["rates2"][i], r["indices2"][i] = rates[:2].detach().numpy(), indices[:2].numpy()
        r["true_prob_after"][i] = rates[(indices == lab.item()).nonzero().item()].item()
    dev_gap = max([abs(p - q) for p, q in gap_pairs] + [abs(p - q) for p, q in zip(rec.gaps, rec.gaps64)])
    r["band_W"], r["band_gap"] = np.float64(16.0 * max(dev_W, 2.0 ** -24)), np.float64(16.0 * dev_gap)
    if min(rec.gaps) <= r["band_gap"]:
        raise Refused(f"an evaluation has gap {min(rec.gaps):.3e} inside band_gap {r['band_gap']:.3e}")
    # stability probe: the reference's own fp32 trajectory, repeated with one ulp of noise on every layer output of the
    # victim, must stay inside band_W and keep its outcome — a trajectory that sits on a discrete tie INSIDE the victim (an
    # arg-max of the max-pool, a ReLU) jumps to another branch under any other rounding, and no implementation can follow it
    state = torch.get_rng_state()
    n_hook = len(grads)
    try:
        PROBE["on"] = True
        for k in range(PROBES):
            PROBE["gen"] = torch.Generator().manual_seed(1000 + k)
            for i, W0, W1, correct, steps in ctri:
                model_v.iso.weight.data = W0.clone()
                c, _, _, _, _, st = iso.gradient_attack(torch.from_numpy(x[i:i + 1]), torch.from_numpy(label[i:i + 1]), model_v, args)
                d = float((model_v.iso.weight.data - W1).abs().max())
                if (c, st) != (correct, steps) or d > r["band_W"]:
                    raise Refused(f"cloud {i}: probe {k} moves the reference's own fp32 run by {d:.3e} (band_W {r['band_W']:.3e}), "
                                  f"outcome ({c}, {st}) vs ({correct}, {steps}): a tie inside the victim")
    finally:
        PROBE["on"] = False
        torch.set_rng_state(state)
        del grads[n_hook:]
    r["alpha"], r["beta"] = thompson.alpha.copy(), thompson.beta.copy()
    r["tsi_all"] = np.stack(DRAWN) if DRAWN else np.zeros((0, 3, 3))
    r["next_np"], r["next_torch"] = np.float64(np.random.uniform()), torch.rand(1).double().numpy()[0]
    return r


BASE = dict(num_steps=50, step_size=5e-4, LAMBDA=1000, target=1, kappa=0, num_init=50, d=4, a=-np.pi, b=np.pi,
            attack_type='combine')
CASES = {
    "a": dict(a=-0.05, b=0.05, step_size=5e-3, num_steps=30),                  # TSI fails, CTRI breaks mid-loop
    "b": dict(a=-0.05, b=0.05, step_size=5e-4, num_steps=8),                   # clouds that never break
    "c": dict(num_init=50),                                                    # TSI successes and its early break
    "d": dict(num_init=50, target=0),
    "e": dict(a=-0.05, b=0.05, step_size=5e-3, num_steps=30),                  # + one cloud with a wrong label
}


def regime(name, r):
    """What the case is there to show; a seed that does not show it is passed over."""
    ctri = r["attacked"] & ~r["init_success"]
    if name in ("a", "e"):
        ok = ctri.sum() >= 4 and (r["correct"][ctri] == 0).sum() >= 2 and ((r["steps"][ctri] > 1) & (r["correct"][ctri] == 0)).any()
        if name == "e":
            ok = ok and not r["attacked"][2]
        return ok
    if name == "b":
        return ctri.sum() >= 4 and (r["correct"][ctri] == 1).sum() >= 3
    ok = r["init_success"].sum() >= 3 and (r["tsi_draws"][r["init_success"]] > 1).any()
    if name == "d":                       # target = 0 is there for the cross-entropy loss IN CTRI: a cloud must get there and break
        ok = ok and ctri.sum() >= 1 and (r["correct"][ctri] == 0).any()
    return ok


SIGNED = {"iso_attack": ["spectral_penalty", "iso_penalty", "logits_info", "ISOnet.__init__", "ISOnet.forward",
                         "thompson_sample_attack", "gradient_attack"],
          "thompson_sample": ["logits_info", "environment.__init__", "environment.generate_thetas", "environment.arm_to_interval",
                              "environment.get_reward_matrix", "BetaAlgo.__init__", "BetaAlgo.get_reward_matrix",
                              "BetaAlgo._update_params", "BernThompson.__init__", "BernThompson.get_action"],
          "isometry_init": ["rotation_xyz", "rotation_axis_angle", "rotation", "reflection", "ref_rot"]}


def sig_string(f):
    """'(name, name=default, ...)' with array defaults written as lists (numpy's print options must not matter)."""
    import inspect
    out = []
    for p in inspect.signature(f).parameters.values():
        d = p.default
        out.append(p.name if d is inspect.Parameter.empty else f"{p.name}={np.asarray(d).tolist()!r}" if isinstance(d, np.ndarray)
                   else f"{p.name}={d!r}")
    return "(" + ", ".join(out) + ")"


def signatures(iso, ts):
    """'module:qualified name:signature' of every function the mirror package restates (names only, no code)."""
    mods = {"iso_attack": iso, "thompson_sample": ts, "isometry_init": sys.modules["isometry_init"]}
    out = []
    for m, names in SIGNED.items():
        for q in names:
            f = mods[m]
            for part in q.split("."):
                f = getattr(f, part)
            f = getattr(f, "__wrapped_real__", f)
            out.append(f"{m}:{q}:{sig_string(f)}")
    return out


def main():
    from model.pointnet import PointNetCls
    iso, ts = load_reference()
    model, sha = _seeded_pointnet(PointNetCls, 40, 3)
    model64 = copy.deepcopy(model).double().eval()
    for p in list(model.parameters()) + list(model64.parameters()):
        p.requires_grad_(False)                                     # the victim is frozen; only iso.weight is optimised
    for m in model.modules():                                       # after the float64 twin was copied: fp32 victim only
        if isinstance(m, (torch.nn.Conv1d, torch.nn.Linear)):
            m.register_forward_hook(_round_off)
    fx = {"sha256": np.array(sha), "weights_seed": np.int64(3), "cases": np.array([f"{c}_n{N}" for N in (64, 256) for c in CASES])}
    for N in (64, 256):
        for ci, (name, over) in enumerate(CASES.items()):
            a = dict(BASE, **over)
            for seed in range(1000 * N + 100 * ci, 1000 * N + 100 * ci + 99):
                rng = np.random.default_rng(seed)
                x = np.stack([unit_cloud(rng, N) for _ in range(NCLOUD)]).transpose(0, 2, 1).copy()
                with torch.no_grad():
                    logp = model(torch.from_numpy(x))[0]
                label = logp.argmax(1).numpy().astype(np.int64)
                if name == "e":
                    label[2] = int(logp[2].argsort(descending=True)[1])       # the runner-up: a wrong label
                try:
                    r = run_case(iso, ts, model, model64, x, label, a, seed)
                except Refused as e:
                    print(f"{name}_n{N} seed {seed}: refused: {e}")
                    continue
                if not regime(name, r):
                    print(f"{name}_n{N} seed {seed}: passed over (steps {r['steps'].tolist()} correct {r['correct'].tolist()} "
                          f"init {r['init_success'].astype(int).tolist()} draws {r['tsi_draws'].tolist()})")
                    continue
                break
            else:
                raise SystemExit(f"{name}_n{N}: no seed passed")
            key = f"{name}_n{N}"
            fx[f"{key}_x"], fx[f"{key}_label"], fx[f"{key}_seed"] = x, label, np.int64(seed)
            fx[f"{key}_args"] = np.array([a["num_steps"], a["step_size"], a["LAMBDA"], a["target"], a["kappa"], a["num_init"],
                                          a["d"], a["a"], a["b"]], dtype=np.float64)
            for k, v in r.items():
                fx[f"{key}_{k}"] = v
            print(f"{key}: seed {seed} attacked {r['attacked'].astype(int).tolist()} draws {r['tsi_draws'].tolist()} init "
                  f"{r['init_success'].astype(int).tolist()} steps {r['steps'].tolist()} correct {r['correct'].tolist()} "
                  f"band_W {r['band_W']:.2e} band_gap {r['band_gap']:.2e}")
    fx["signatures"] = np.array(signatures(iso, ts))
    np.savez_compressed(os.path.join(OUT, "iso.npz"), **fx)
    print("iso.npz:", len(fx), "arrays")


if __name__ == "__main__":
    main()
