"""GPU: geoA3_attack(cfg.device_loop = True) — GeoA3's iteration as a captured chain of own kernels on PointNet victims.

The base case: 3 clouds of 200 points (helpers.unit_cloud, rng seed 3), labels from oracle_pointnet(0), the configuration of
tests/golden/make_golden.py's GeoA3 fixtures with 2 x 12 steps, cfg.host_rng = True, seed 77. Yardsticks that exist without
the device loop, against GeoA3Oracle(as_written=False, dtype=float64) (float64 searches) on the same case: the fp32 oracle's
deviation and the autograd path's deviation. Measured on an MI355X (relative on the loss curves, absolute on the best
clouds; printed by test_base_case_against_the_oracles):
    fp32 oracle      loss 2.37e-06   clouds 3.65e-07
    autograd path    loss 1.82e-06   clouds 1.99e-05
    device loop      loss 2.31e-06   clouds 1.99e-05

The feature-transform victim is held to test_knn_loop_gpu's bands against the double oracle (median < 1e-6, 90 % within 1e-4,
q99 < 1e-2), not to the rule above, and the reason is in the victim, not in the update kernel: with the seeded weights its
logits reach 320 and 1 - p_target lies between 1e-13 and 2e-3, and the loss launch of the launch-minimal passes
(pc3d_cls_loss_f32) forms the log-probabilities as z - (max + log sum), which keeps eps x |z| = 3e-5 of absolute error where
the CE gradient needs 1 - p_target: its input gradient is 4e-3 relative from a float64 evaluation there (autograd through
forward(): 2.5e-5; the plain victim: 4.5e-7 either way). Measured: one coordinate of the 1800 takes the other sign in Adam's
first step (clouds 0.02 = 2 lr apart there, loss curves 8.0e-3 relative; the autograd path 3.6e-07 / 2.3e-04), same success
mask and best steps; median 0, 99.94 % within 1e-4, q99 3.7e-08.
"""
import importlib

import numpy as np
import pytest
import torch

import pointnet_ft_restatement as rst
from conftest import GOLDEN
from helpers import hip_pointnet, oracle_pointnet, unit_cloud
from oracle import ref_torch as ort
from test_oracle_golden import GEO_CASES, _geo_cfg

pytestmark = pytest.mark.gpu
M = importlib.import_module


def _ga():
    return M("3dpointcloudattack_amd.attack.GeoA3.GeoA3_attack")


def _clouds(seed, B, N):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(np.stack([unit_cloud(rng, N) for _ in range(B)]))


def _attack(victim, pcs, labels, seed=77, **over):
    ga = _ga()
    cfg = _geo_cfg(host_rng=True, **over)
    torch.manual_seed(seed)
    np.random.seed(seed)
    best, tgt, mask, steps, losses = ga.geoA3_attack(victim, None, None, None, None, None, pcs, labels, cfg, 0, 1)
    return dict(best=best.cpu().numpy(), mask=np.asarray(mask), steps=list(steps), losses=np.array(losses), path=ga.geoA3_attack.last_path)


def _same(a, b):
    return (np.array_equal(a["best"], b["best"]) and np.array_equal(a["mask"], b["mask"]) and a["steps"] == b["steps"]
            and np.array_equal(a["losses"], b["losses"]))


def _oracle(net, pcs, labels, seed=77, **kw):
    torch.manual_seed(seed)
    np.random.seed(seed)
    best, _, mask, steps, losses = ort.GeoA3Oracle(as_written=False, **kw).attack(net, pcs, labels, _geo_cfg(), per_sample_label=True)
    return dict(best=best.detach().numpy(), mask=np.asarray(mask), steps=list(steps), losses=np.array(losses))


@pytest.fixture(scope="module")
def pn(dev):
    return hip_pointnet(0, dev)[0]


@pytest.fixture(scope="module")
def case():
    opn, _ = oracle_pointnet(0)
    pcs = _clouds(3, 3, 200)
    with torch.no_grad():
        labels = opn(pcs.transpose(1, 2).contiguous())[0].argmax(1)
    return dict(opn=opn, pcs=pcs, labels=labels, o64=_oracle(opn, pcs, labels, dtype=torch.float64),
                o32=_oracle(opn, pcs, labels))


def _deviation(r, ref):
    return (float(np.max(np.abs(r["losses"] - ref["losses"]) / np.abs(ref["losses"]))), float(np.abs(r["best"] - ref["best"]).max()))


def test_base_case_against_the_oracles(dev, pn, case):
    loop = _attack(pn, case["pcs"], case["labels"], device_loop=True)
    assert loop["path"] == "device_loop"
    plain = _attack(pn, case["pcs"], case["labels"], device_loop=False)
    assert plain["path"] == "autograd"
    o64, o32 = case["o64"], case["o32"]
    for r in (loop, plain, o32):
        assert np.array_equal(r["mask"], o64["mask"]) and r["steps"] == o64["steps"]
    assert o64["mask"].all() and o64["steps"] == [4, 4, 2]
    d32, dplain, dloop = _deviation(o32, o64), _deviation(plain, o64), _deviation(loop, o64)
    print(f"fp32 oracle: loss {d32[0]:.3g} clouds {d32[1]:.3g}; autograd path: loss {dplain[0]:.3g} clouds {dplain[1]:.3g}; "
          f"device loop: loss {dloop[0]:.3g} clouds {dloop[1]:.3g}")
    assert dloop[0] <= 4 * max(d32[0], dplain[0]) and dloop[1] <= 4 * max(d32[1], dplain[1])


def test_golden_cases_on_the_device_loop(dev, pn):
    """The assertions of test_geoa3_gpu.test_geoa3_attack_vs_reference_and_oracle with cfg.device_loop = True."""
    import os
    ga = _ga()
    fx = np.load(os.path.join(GOLDEN, "geoa3.npz"))
    onet, _ = oracle_pointnet(0)
    for nm in fx["names"]:
        cfg = _geo_cfg(device_loop=True, **GEO_CASES[str(nm)])
        torch.manual_seed(77)
        np.random.seed(77)
        best, tgt, mask, steps, losses = ga.geoA3_attack(pn, None, None, None, None, None, torch.from_numpy(fx[f"{nm}_pc"]),
                                                         torch.from_numpy(fx[f"{nm}_label"]), cfg, 0, 1)
        assert ga.geoA3_attack.last_path == "device_loop", nm
        assert best.shape == fx[f"{nm}_best"].shape and len(steps) == 1 and len(losses) == cfg.iter_max_steps
        assert np.array_equal(mask, fx[f"{nm}_mask"]), nm
        L, Lr = np.array(losses), fx[f"{nm}_losses"]
        assert np.all(np.isfinite(L)) and L.shape == Lr.shape
        np.testing.assert_allclose(L[0], Lr[0], rtol=0.2, atol=0.05)
        if mask.any():
            with torch.no_grad():
                lab = pn(best)[0].argmax(1).cpu()
                lab_ref = onet(torch.from_numpy(fx[f"{nm}_best"]))[0].argmax(1)
            assert torch.equal(lab != tgt.cpu(), lab_ref != torch.from_numpy(fx[f"{nm}_label"]))


@pytest.mark.parametrize("steps", [20, 37])
def test_graph_replay_equals_eager_and_run_equals_run(dev, pn, case, steps):
    g = _attack(pn, case["pcs"], case["labels"], device_loop=True, iter_max_steps=steps)
    e = _attack(pn, case["pcs"], case["labels"], device_loop=True, iter_max_steps=steps, graph_victim=False)
    g2 = _attack(pn, case["pcs"], case["labels"], device_loop=True, iter_max_steps=steps)
    assert g["path"] == e["path"] == "device_loop" and g["mask"].any()
    assert _same(g, e) and _same(g, g2)


def test_batch_of_three_equals_three_alone(dev, pn, case):
    seeds = [41, 42, 43]
    out = _attack(pn, case["pcs"], case["labels"], device_loop=True, sample_seeds=seeds, global_batch=3)
    assert out["mask"].any()
    for i in range(3):
        one = _attack(pn, case["pcs"][i:i + 1], case["labels"][i:i + 1], device_loop=True, sample_seeds=[seeds[i]], global_batch=3)
        assert one["path"] == "device_loop"
        assert np.array_equal(one["best"][0], out["best"][i]) and one["steps"][0] == out["steps"][i]
        assert np.array_equal(one["losses"][:, 0], out["losses"][:, i]), i


def test_second_call_reuses_the_graphs(dev, case):
    pn1, pn2 = hip_pointnet(0, dev)[0], hip_pointnet(0, dev)[0]
    first = _attack(pn1, case["pcs"], case["labels"], device_loop=True)
    states = list(pn1._geoa3_loop_cache.values())
    assert len(states) == 1 and states[0].graphs is not None
    graphs = states[0].graphs
    other = _clouds(9, 3, 200)
    second = _attack(pn1, other, case["labels"], device_loop=True)
    assert list(pn1._geoa3_loop_cache.values())[0].graphs is graphs and second["path"] == "device_loop"
    fresh = _attack(pn2, other, case["labels"], device_loop=True)
    assert _same(second, fresh) and not np.array_equal(second["losses"], first["losses"])


def test_feature_transform_victim(dev):
    pnm, seeding = M("3dpointcloudattack_amd.model.pointnet"), M("3dpointcloudattack_amd.seeding")
    m = pnm.PointNetCls(k=40, feature_transform=True)
    sd = seeding.seeded_state_dict(m, 0)
    m.load_state_dict(sd, strict=True)
    m = m.eval().to(dev)
    sd_cpu = {k: v.float() for k, v in sd.items()}

    def oracle_victim(x):
        return rst.forward(sd_cpu, x)

    pcs = _clouds(5, 3, 200)
    with torch.no_grad():
        labels = oracle_victim(pcs.transpose(1, 2).contiguous())[0].argmax(1)
    o64 = _oracle(oracle_victim, pcs, labels, dtype=torch.float64)
    loop = _attack(m, pcs, labels, device_loop=True)
    assert loop["path"] == "device_loop"
    plain = _attack(m, pcs, labels, device_loop=False)
    dplain, dloop = _deviation(plain, o64), _deviation(loop, o64)
    print(f"feature-transform victim. autograd path: loss {dplain[0]:.3g} clouds {dplain[1]:.3g}; device loop: loss {dloop[0]:.3g} "
          f"clouds {dloop[1]:.3g}")
    assert np.array_equal(loop["mask"], o64["mask"]) and loop["steps"] == o64["steps"]
    assert _in_double_oracle_bands(loop["best"], o64["best"])


def _in_double_oracle_bands(hadv, oadv):
    """test_knn_loop_gpu's bands for a trajectory on the launch-minimal passes against a double oracle's."""
    dev_abs = np.abs(hadv - oadv)
    print("median", np.median(dev_abs), "share <= 1e-4", (dev_abs <= 1e-4).mean(), "q99", np.quantile(dev_abs, 0.99))
    return np.median(dev_abs) < 1e-6 and (dev_abs <= 1e-4).mean() > 0.9 and np.quantile(dev_abs, 0.99) < 1e-2


def _falls_back(victim, pcs, labels, **over):
    a1 = _attack(victim, pcs, labels, device_loop=True, iter_max_steps=3, **over)
    a0 = _attack(victim, pcs, labels, device_loop=False, iter_max_steps=3, **over)
    assert a1["path"] == "autograd" and a0["path"] == "autograd"
    assert _same(a1, a0)


def test_falls_back_on_an_ssg_victim(dev):
    ssg = M("3dpointcloudattack_amd.model.pointnet2_SSG").PointNet_Ssg(40)
    ssg.load_state_dict(ort.seeded_state_dict(ssg, 3))
    ssg = ssg.eval().to(dev)
    _falls_back(ssg, _clouds(6, 2, 600), torch.tensor([3, 7]), npoint=600)


@pytest.mark.parametrize("over", [dict(is_partial_var=True, knn_range=8), dict(is_pre_jitter_input=True),
                                  dict(uniform_loss_weight=0.1, curv_loss_weight=0, hd_loss_weight=0), dict(is_pro_grad=True)],
                         ids=["partial_var", "pre_jitter", "uniform", "pro_grad"])
def test_falls_back_on_a_configuration_outside_the_plan(dev, pn, case, over):
    _falls_back(pn, case["pcs"], case["labels"], npoint=200, **over)


def test_falls_back_above_the_cap(dev, pn, ops):
    n = ops.GEOA3_LOOP_MAX_POINTS + 4
    _falls_back(pn, _clouds(7, 1, n), torch.tensor([5]), npoint=n)


def test_keyword_absent_equals_false(dev, pn, case):
    a = _attack(pn, case["pcs"], case["labels"])
    b = _attack(pn, case["pcs"], case["labels"], device_loop=False)
    assert a["path"] == b["path"] == "autograd" and _same(a, b)
