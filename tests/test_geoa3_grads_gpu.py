"""The gradient of GeoA3's `_forward_step` loss (attack/GeoA3/GeoA3_attack.py:103-183) on the iterates the REAL reference's
loop visits at N = 1024 — the size, the nominal-batch plans and the shared victim graph the benchmark runs with — against
float64 gradients computed on the reference's model (tests/golden/geoa3_grads*.npz, make_golden_geoa3_grads.py). The loop
tests next door (test_config_sizes_gpu.py) pin these cases by 20 % - 100 % bands on the loss curve only.

Three gradients per iterate: g_con (distance / Hausdorff / curvature terms: the two nearest-neighbour searches, the kappa
gather, pc3d_geoa3_terms_f32 and their backward), g_cls (the victim's forward and backward under the classification loss)
and g_total. Every band is the reference's OWN fp32-against-float64 deviation on the same iterate, times the project's
band factor 4; nothing here is derived from what the HIP code gives. The victims are piecewise (arg-max pools, kNN graphs,
walks), so the reference's own fp32 run is off by 1e-3 .. 1e-1 on a few iterates where one such decision is a near-tie:
g_cls and g_total are therefore held to 4 x the THIRD-largest band of the case on all but 2 of the 24 CurveNet iterates
(6 DGCNN iterates: the second-largest, all but 1), and half of the
iterates the reference itself resolves cleanly (b_cls <= 1e-5) to 4 x the largest band among those. g_con has no victim
in it and is held to 4 x its own band on every iterate.

MEASURED (MI355X, deterministic build; the same on two runs), per case in the order cngeo margin_l2 / cngeo ce_cd_hd_curv /
dgcnn margin_l2 / dgcnn ce_cd_hd_curv:
    g_con, largest multiple of its own band (limit 4):                 0.18 / 1.33 / 0.07 / 1.27
    term values, largest multiple of 4 x their own deviation:          0.45 / 0.59 / 0.32 / 0.42
    g_cls, largest multiple of the wide band, iterates outside it:     0.59 none / 3.71 iterate 13 / 0.25 none / 20.7 iterate 12
    g_total, the same (direct and general form are bit-identical):     0.83 none / 3.71 iterate 13 / 0.25 none / 20.8 iterate 12
    clean iterates inside the tight band (need half):                  8 of 13 / 6 of 10 / the reference has none / 1 of 2
Iterate 13 of cngeo ce_cd_hd_curv is the reference's own worst (9.5e-3, the HIP victim lands on the same side: 9.5e-3);
iterate 12 of dgcnn ce_cd_hd_curv is 6.3e-2 off: one re-wired feature-space edge. With the output of geoa3_terms' backward
scaled by 1.05 the terms and total tests of both ce_cd_hd_curv cases fail; with the replayed victim's input gradient scaled
by 1.05 the victim and total tests of both CurveNet cases fail."""
import importlib
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle import ref_torch as ort
import test_configs_gpu as tc

pytestmark = pytest.mark.gpu
M = importlib.import_module
FACTOR = 4.0
KEYS = [f"{v}_n1024_{nm}" for v in ("cngeo", "dgcnn") for nm in ("margin_l2", "ce_cd_hd_curv")]


@pytest.fixture(scope="module")
def fx():
    out = dict(np.load(os.path.join(GOLDEN, "geoa3_grads.npz")))
    cs = np.load(os.path.join(GOLDEN, "config_sizes.npz"))
    for k in KEYS:
        out[f"{k}_pc"] = cs[f"{k}_pc"]
        if k.startswith("cngeo"):
            out[f"{k}_iter_inputs"] = cs[f"{k}_iter_inputs"]
            out.update(np.load(os.path.join(GOLDEN, f"geoa3_grads_{k}.npz")))
    return out


@pytest.fixture(scope="module")
def victims(dev, fx):
    dg, sha = tc._hip_dgcnn(dev)
    assert sha == str(fx["dgcnn_sha256"])
    cn = tc._hip_curvenet(dev, np.load(os.path.join(GOLDEN, "cw_curvenet.npz"))["conv2_bias"])
    assert ort.state_sha256(cn.state_dict()) == str(fx["cngeo_sha256"])
    gr = M("3dpointcloudattack_amd.graphed")
    return {"dgcnn": gr.wrap(dg, enable=None), "cngeo": gr.wrap(cn, enable=None)}     # as geoA3_attack wraps its victim


def _rel_l2(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


class _Case:
    def __init__(self, dev, fx, victims, key):
        self.key, self.dev, self.fx = key, dev, fx
        self.nm = key.split("n1024_")[1]
        self.net = victims[key.split("_")[0]]
        self.cfg = tc._geo_cfg(host_rng=True, npoint=1024, **tc.GEO_CASES[self.nm])
        self.xs = fx[f"{key}_iter_inputs"]
        self.n = self.xs.shape[0]
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.ori = t(fx[f"{key}_pc"].transpose(0, 2, 1))
        self.normal = t(fx[f"{key}_normal_ori"])
        self.kappa = t(fx[f"{key}_ori_kappa"]) if f"{key}_ori_kappa" in fx else None
        self.target = t(fx[f"{key}_target"])
        self.scale, self.targeted = fx[f"{key}_scale_const"], fx[f"{key}_targeted"]
        assert self.n == len(fx[f"{key}_iter_index"]) == (24 if key.startswith("cngeo") else 6)
        # the stored arguments span both binary steps: the reference's untargeted run, initial_const 10, then its update
        assert not self.targeted.any() and self.scale.shape == (self.n, 1)
        half = self.n // 2
        assert (self.scale[:half] == 10.0).all() and (self.scale[half:] == self.scale[half]).all()
        assert self.scale[half, 0] in (5.0, 20.0)
        assert (self.kappa is None) == (self.cfg.curv_loss_weight == 0)

    def step(self, i, cfg=None, direct=False):
        ga = M("3dpointcloudattack_amd.attack.GeoA3.GeoA3_attack")
        x = torch.from_numpy(self.xs[i:i + 1].copy()).to(self.dev).requires_grad_()
        out = ga._forward_step(self.net, self.ori, x, self.normal, self.kappa, self.target,
                               torch.from_numpy(self.scale[i]).to(self.dev), cfg or self.cfg, bool(self.targeted[i]), direct=direct)
        return x, out

    def band(self, name):
        return self.fx[f"{self.key}_{name}"]

    def two_tier(self, what, devs, band):
        """All but `cap` iterates (2 of 24, 1 of 6) inside 4 x the (cap + 1)-th largest reference band — the rule the
        reference's own fp32 run passes with factor 1 by construction; half of the clean ones inside 4 x the clean set's
        largest band."""
        devs = np.asarray(devs)
        cap = 2 if self.n == 24 else 1
        clean = self.band("clean")
        wide, tight = FACTOR * np.sort(band)[-(cap + 1)], FACTOR * (band[clean].max() if clean.any() else 0.0)   # dgcnn margin_l2: the reference has no clean iterate
        out = np.nonzero(devs > wide)[0]
        inside = int((devs[clean] <= tight).sum())
        print(f"{self.key} {what}: max {devs.max() / wide:.3f} x the wide band ({wide:.2e}); outside it: {out.tolist()}; "
              f"clean iterates inside the tight band ({tight:.2e}): {inside} of {int(clean.sum())}")
        for i in range(self.n):
            print(f"    iterate {int(self.band('iter_index')[i]):2d}  dev {devs[i]:.3e}  reference's own {band[i]:.3e}"
                  f"{'  clean' if clean[i] else ''}")
        assert np.isfinite(devs).all()
        assert len(out) <= cap, (self.key, what, out.tolist(), devs[out].tolist(), wide)
        assert 2 * inside >= int(clean.sum()), (self.key, what, inside, int(clean.sum()), tight)


@pytest.mark.parametrize("key", KEYS)
def test_terms_gradient_on_reference_iterates(dev, fx, victims, key):
    """cls_loss_type 'None' (ce_cd_hd_curv stays on the fused-terms path; margin_l2's only term is the L2 distance): the
    gradient of (scale_const * constrain_loss).mean() and the term values, on EVERY iterate, no exclusions.
    MEASURED: the module docstring's table; DESIGN.md §4.6."""
    c = _Case(dev, fx, victims, key)
    cfg = tc._geo_cfg(host_rng=True, npoint=1024, **{**tc.GEO_CASES[c.nm], "cls_loss_type": 'None'})
    devs, worst = [], {}
    for i in range(c.n):
        x, out = c.step(i, cfg)
        _, _, loss, loss_n, cls_loss, dis, hd, curv, con, _ = out
        loss.backward()
        devs.append(_rel_l2(x.grad.cpu().numpy(), fx[f"{key}_g_con"][i:i + 1]))
        assert float(cls_loss) == 0.0
        for nm_, v in (("dis", dis), ("hd", hd), ("curv", curv), ("con", con)):
            ref, got = float(fx[f"{key}_{nm_}"][i]), float(v)
            bound = FACTOR * float(fx[f"{key}_dev_{nm_}"][i]) * abs(ref)
            worst[nm_] = max(worst.get(nm_, 0.0), abs(got - ref) / bound if bound > 0 else float(got != ref))
        sc = float(c.scale[i, 0])
        assert abs(float(loss_n) - sc * float(fx[f"{key}_con"][i])) <= (FACTOR * float(fx[f"{key}_dev_con"][i]) + 2.0 ** -23) * abs(sc * float(fx[f"{key}_con"][i]))
    devs, band = np.array(devs), c.band("b_con")
    print(f"{key} g_con: largest multiple of the reference's own band {np.max(devs / band):.3f}; term values, largest "
          f"multiple of 4 x their own deviation: " + ", ".join(f"{k_} {v:.3f}" for k_, v in worst.items()))
    for i in range(c.n):
        print(f"    iterate {int(c.band('iter_index')[i]):2d}  dev {devs[i]:.3e}  reference's own {band[i]:.3e} "
              f"(its expansion form: {c.band('b_con_expansion')[i]:.3e})")
    assert (devs <= FACTOR * band).all(), (key, np.nonzero(devs > FACTOR * band)[0].tolist(), (devs / band).max())
    assert all(v <= 1.0 for v in worst.values()), (key, worst)


@pytest.mark.parametrize("key", KEYS)
def test_victim_gradient_on_reference_iterates(dev, fx, victims, key):
    """The gradient of cls_loss.mean() through the HIP victim (forward and backward, graph-replayed as in the loop).
    MEASURED: the module docstring's table; DESIGN.md §4.6."""
    c = _Case(dev, fx, victims, key)
    devs = []
    for i in range(c.n):
        x, out = c.step(i)
        cls_loss = out[4]
        ref = fx[f"{key}_g_cls"][i:i + 1]
        assert abs(float(cls_loss) - float(fx[f"{key}_cls"][i])) <= 2e-2 + 1e-3 * abs(float(fx[f"{key}_cls"][i]))   # logits: pinned next door
        if cls_loss.requires_grad and cls_loss.grad_fn is not None:
            cls_loss.mean().backward()
            g = x.grad.cpu().numpy() if x.grad is not None else np.zeros_like(ref)
        else:
            g = np.zeros_like(ref)
        devs.append(_rel_l2(g, ref))
    c.two_tier("g_cls", devs, c.band("b_cls"))


@pytest.mark.parametrize("key", KEYS)
def test_total_gradient_on_reference_iterates(dev, fx, victims, key):
    """g_total from a plain `_forward_step`, once through `loss.backward()` and once in the direct form (the loss never
    formed: backward through `roots` / `grads`, what the loop runs by default). Both must pass the two-tier rule.
    MEASURED: the module docstring's table; DESIGN.md §4.6."""
    c = _Case(dev, fx, victims, key)
    devs = {False: [], True: []}
    mutual = []
    for i in range(c.n):
        g = {}
        for direct in (False, True):
            x, out = c.step(i, direct=direct)
            if isinstance(out[-1], dict):
                assert direct and out[2] is None
                torch.autograd.backward(out[-1]["roots"], out[-1]["grads"])
            else:
                out[2].backward()
            g[direct] = x.grad.cpu().numpy()
            devs[direct].append(_rel_l2(g[direct], fx[f"{key}_g_total"][i:i + 1]))
            assert abs(float(out[3]) - float(fx[f"{key}_loss_n"][i])) <= 2e-2 + 1e-3 * abs(float(fx[f"{key}_loss_n"][i]))
        mutual.append(_rel_l2(g[True], g[False]))
    print(f"{key}: direct against general form, relative L2 per iterate: max {max(mutual):.3e}")
    for direct in (False, True):
        c.two_tier(f"g_total (direct={direct})", devs[direct], c.band("b_total"))
