"""CPU: the shape-invariant attack's plain-torch side against tests/golden/siadv.npz (the real reference's
shape_invariant_ifgm run on the CPU with a stand-in for open3d, see tests/golden/make_golden_siadv.py).

  * the restatement of the loop (tests/siadv_restatement.py), in fp32 and in float64, reproduces every stored P_i, the
    gradients and the ending within the bands stored with the case;
  * the mirror's four geometry helpers and CWLoss, which are device-agnostic torch, match the stored intermediates;
  * the step does not depend on the sign of the normals; run() refuses the query attacks by name; the drop-in imports.
"""
import importlib
import os
import types

import numpy as np
import pytest
import torch

import siadv_restatement as R
from conftest import GOLDEN

CASES = ("s1", "s5", "s5_top5")


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "siadv.npz"))


@pytest.fixture(scope="module")
def models():
    from oracle import ref_torch as ort
    out = []
    for seed in (3, 4):
        m = ort.PointNetCls(k=40)
        m.load_state_dict(ort.seeded_state_dict(m, seed))
        out.append(m.eval())
    return out


def _args(fx, case, **over):
    eps, step_size, max_steps, top5 = fx[f"{case}_args"]
    a = dict(eps=float(eps), step_size=float(step_size), max_steps=int(max_steps), num_class=40, top5_attack=bool(top5),
             defense_method=None, transfer_attack_method="ifgm_ours", query_attack_method=None)
    a.update(over)
    return types.SimpleNamespace(**a)


def _mirror():
    return importlib.import_module("3dpointcloudattack_amd.attack.SIadv.SIadv_attack")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_fixture(fx, models, case, dtype):
    import copy
    a = _args(fx, case)
    sur, tgt = (copy.deepcopy(m).to(dtype) for m in models)
    points, target = torch.from_numpy(fx["points"]).to(dtype), torch.from_numpy(fx["target"])
    rec = {}
    P = R.run_loop(sur, points, target, a.eps, a.step_size, a.max_steps, a.top5_attack, record=rec)
    band_P, band_gap = float(fx[f"{case}_band_P"]), float(fx[f"{case}_band_gap"])
    for i, Pi in enumerate(rec["P"]):
        dev = float((Pi.double() - torch.from_numpy(fx[f"{case}_P"][i]).double()).abs().max())
        print(f"{case} {dtype} P_{i}: deviation {dev:.3e} (band_P {band_P:.3e})")
        assert dev <= band_P
    # the stored gradient is dL/dP' = U dL/dP before its third component is dropped
    U0 = R.spin_axis_matrix(rec["n"][0])
    gp0 = (U0 @ rec["g"][0][..., None])[..., 0]
    ref_g = torch.from_numpy(fx[f"{case}_g"][0]).double()
    assert float((gp0.double() - ref_g).abs().max()) <= 1e-3 * float(ref_g.abs().max())
    with torch.no_grad():
        logits = tgt(P.transpose(1, 2).contiguous())[0]
    s = logits.sort(1, descending=True)[0]
    gap = (s[:, 0] - s[:, 1]).double().numpy()
    assert np.abs(gap - fx[f"{case}_gap"]).max() <= band_gap
    sure = fx[f"{case}_gap"] > band_gap
    assert sure.sum() * 2 >= len(sure)
    pred = logits.argmax(1)
    adv_target = pred
    if a.top5_attack:
        adv_target = torch.where((logits.topk(5)[1] == target[:, None]).any(1), target, torch.full_like(target, -1))
    assert np.array_equal(adv_target.numpy()[sure], fx[f"{case}_adv_target"][sure])
    assert np.array_equal((pred != target).numpy()[sure].astype(np.int64), fx[f"{case}_count"][sure])


@pytest.mark.parametrize("case", ["s5", "s5_top5"])
def test_mirror_helpers_match_the_fixture(fx, models, case):
    si = _mirror()
    atk = si.PointCloudAttack(_args(fx, case), wb_classifier=models[0], classifier=models[1])
    points = torch.from_numpy(fx["points"])
    P0, n0 = torch.from_numpy(fx[f"{case}_P"][0]), torch.from_numpy(fx[f"{case}_n"][0])
    assert torch.equal(P0, points[:, :, :3])
    U = atk.get_spin_axis_matrix(n0)
    assert U.shape == (4, 256, 3, 3) and torch.isfinite(U).all()
    np.testing.assert_allclose(U.numpy(), fx[f"{case}_U0"], rtol=1e-6, atol=1e-7)
    bound = (n0[..., 2] ** 2 - 1).abs() < 1e-4
    assert 4 <= int(bound[0].sum()) <= 8                     # the rewritten rows are exercised ...
    assert float((U[bound] @ U[bound].transpose(-1, -2) - torch.eye(3)).abs().max()) < 1e-3
    assert float((U[bound][:, 2] - n0[bound]).abs().max()) > 5e-3      # ... and are NOT the frame of n there
    Pp, U2, t = atk.get_transformed_point_cloud(P0, n0)
    assert torch.equal(U2, U)
    np.testing.assert_allclose(t.numpy(), fx[f"{case}_t0"], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(Pp.numpy(), fx[f"{case}_Pp0"], rtol=1e-5, atol=1e-6)
    back = atk.get_original_point_cloud(torch.from_numpy(fx[f"{case}_Pp0"]), U, t)
    ref_back = (torch.from_numpy(fx[f"{case}_U0"]).transpose(-1, -2) @ torch.from_numpy(fx[f"{case}_Pp0"])[..., None])[..., 0] \
        - torch.from_numpy(fx[f"{case}_t0"])
    np.testing.assert_allclose(back.numpy(), ref_back.numpy(), rtol=1e-6, atol=1e-7)
    target = torch.from_numpy(fx["target"])
    with torch.no_grad():
        logits = models[0](P0.transpose(1, 2).contiguous())[0]
    for b in range(4):                                       # the reference's loss is one cloud's (B = 1) ...
        loss = atk.CWLoss(logits[b:b + 1], target[b:b + 1], kappa=0., tar=False, num_classes=40)
        assert abs(float(loss) - float(fx[f"{case}_loss0"][b])) <= 1e-4
    total = atk.CWLoss(logits, target, kappa=0., tar=False, num_classes=40)
    assert abs(float(total) - float(fx[f"{case}_loss0"].sum())) <= 4e-4      # ... and the batch's is their sum
    assert float(total) == pytest.approx(float(R.cw_loss(logits, target, atk.top5_attack)), abs=1e-6)


def test_step_does_not_depend_on_the_sign_of_the_normals(fx):
    g = torch.Generator().manual_seed(0)
    P0 = torch.from_numpy(fx["s5_P"][2]).double()
    ori = torch.from_numpy(fx["s5_P"][0]).double()
    grad = torch.randn(P0.shape, generator=g, dtype=torch.float64)
    for n in (torch.from_numpy(fx["s5_n"][0]).double(), torch.from_numpy(fx["s5_n"][2]).double()):
        a = R.si_step(P0, ori, grad, n, 0.07, 0.16)
        b = R.si_step(P0, ori, grad, -n, 0.07, 0.16)
        flip = torch.where(torch.rand(n.shape[:2], generator=g) < 0.5, -1.0, 1.0).double()[..., None]
        c = R.si_step(P0, ori, grad, n * flip, 0.07, 0.16)
        assert float((a - b).abs().max()) == 0.0 and float((a - c).abs().max()) == 0.0


def test_literal_step_differs_from_the_tangent_projection_at_the_boundary_rows(fx):
    """Why the product keeps U as written: well away from |z| = 1 the two forms agree to the rounding of the stored fp32
    normals (which 1 / sqrt(1 - z^2) magnifies near the poles), at the rewritten rows they do not."""
    P0, n0 = torch.from_numpy(fx["s5_P"][0]).double(), torch.from_numpy(fx["s5_n"][0]).double()
    grad = torch.randn(P0.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    a = R.si_step(P0, P0, grad, n0, 0.07, 10.0)
    b = R.tangent_projection_step(P0, P0, grad, n0, 0.07, 10.0)
    bound = (n0[..., 2] ** 2 - 1).abs() < 1e-4
    exact = n0[..., 2].abs() == 1
    away, at = float((a - b)[n0[..., 2].abs() < 0.99].abs().max()), float((a - b)[bound & ~exact].abs().max())
    print(f"literal vs tangent projection: {away:.3e} away from the poles, {at:.3e} at the rewritten rows")
    assert at > 1e-4 and away < 0.2 * at        # (away: the clouds' norms differ through the rewritten rows, and rounding)


@pytest.mark.parametrize("method", ["simba", "simbapp", "ours"])
def test_query_attacks_are_refused_by_name(fx, models, method):
    si = _mirror()
    atk = si.PointCloudAttack(_args(fx, "s1", query_attack_method=method), wb_classifier=models[0], classifier=models[1])
    assert atk.attack_method == method
    with pytest.raises(NotImplementedError, match=method):
        atk.run(torch.from_numpy(fx["points"]), torch.from_numpy(fx["target"]))


def test_models_come_from_args_and_small_clouds_are_refused(fx, models):
    si = _mirror()
    atk = si.PointCloudAttack(_args(fx, "s5", wb_classifier=models[0], classifier=models[1]))
    assert atk.wb_classifier is models[0] and atk.classifier is models[1] and atk.pre_head is None
    for name in ("eps", "step_size", "max_steps", "num_class", "top5_attack", "attack_method", "defense_method",
                 "wb_classifier", "classifier", "pre_head", "CWLoss", "run", "get_defense_head", "get_normal_vector",
                 "get_spin_axis_matrix", "get_transformed_point_cloud", "get_original_point_cloud", "shape_invariant_ifgm"):
        assert hasattr(atk, name), name
    with pytest.raises(ValueError, match="N >= 20"):
        atk.get_normal_vector(torch.zeros(1, 19, 3))
    with pytest.raises(ValueError):
        si.PointCloudAttack(_args(fx, "s5"))


DROPIN = r'''
import importlib, sys
sys.path.insert(0, %r)
pc3d = importlib.import_module("3dpointcloudattack_amd")
pc3d.install_dropin()
from attack.SIadv.SIadv_attack import PointCloudAttack
from attack.SIadv.baselines import *
from attack.SIadv.baselines.attack.util.clip_utils import ClipPointsLinf as C
assert C is ClipPointsLinf and SORDefense and SRSDefense and DUPNet
assert PointCloudAttack is importlib.import_module("3dpointcloudattack_amd.attack.SIadv.SIadv_attack").PointCloudAttack
print("siadv dropin ok")
'''


def test_reference_import_paths_resolve():
    import subprocess
    import sys
    from conftest import ROOT
    out = subprocess.run([sys.executable, "-c", DROPIN % ROOT], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "siadv dropin ok" in out.stdout, out.stderr[-2000:]


def test_drop_in_imports():
    base = importlib.import_module("3dpointcloudattack_amd.attack.SIadv.baselines")
    star = {k: getattr(base, k) for k in dir(base) if not k.startswith("_")}
    for name in ("ClipPointsLinf", "SORDefense", "SRSDefense", "DUPNet"):
        assert name in star, name
    cw_clip = importlib.import_module("3dpointcloudattack_amd.attack.CW.CW_utils.clip_utils")
    assert base.ClipPointsL2 is cw_clip.ClipPointsL2                   # identical in the reference: re-exported
    assert base.ClipPointsLinf is not cw_clip.ClipPointsLinf           # SI-Adv's is a true per-coordinate clamp
    pc, ori = torch.tensor([[[0.5, -0.5, 0.05]]]), torch.zeros(1, 1, 3)
    assert torch.equal(base.ClipPointsLinf(0.16)(pc, ori), torch.tensor([[[0.16, -0.16, 0.05]]]))
    si = _mirror()
    assert si.ClipPointsLinf is base.ClipPointsLinf and si.SORDefense is base.SORDefense
    heads = si.PointCloudAttack.get_defense_head
    assert isinstance(heads(None, "sor"), base.SORDefense) and isinstance(heads(None, "srs"), base.SRSDefense)
    with pytest.raises(NotImplementedError):
        heads(None, "none")
