"""GPU: CWKNN(device_loop=True) — the kNN attack's iteration as a captured chain of own kernels on PointNet victims."""
import importlib
import os

import numpy as np
import pytest
import torch

import pointnet_ft_restatement as rst
from conftest import GOLDEN
from helpers import hip_pointnet, oracle_pointnet, unit_cloud
from oracle import ref_torch as ort

pytestmark = pytest.mark.gpu
M = importlib.import_module


def _mods():
    return (M("3dpointcloudattack_amd.attack.KNN.KNN_attack"), M("3dpointcloudattack_amd.attack.CW.CW_utils.adv_utils"),
            M("3dpointcloudattack_amd.attack.CW.CW_utils.dist_utils"), M("3dpointcloudattack_amd.attack.CW.CW_utils.clip_utils"))


def _clouds(seed, B, N):
    rng = np.random.default_rng(seed)
    return np.stack([unit_cloud(rng, N) for _ in range(B)])


class _KNNDist64(ort.KNNDist):
    def __call__(self, pc, weights=None, batch_avg=True):
        return super().__call__(pc.double(), weights, batch_avg).float()


class _CK64:
    """The reference's ChamferkNNDist with both terms evaluated in double (see test_knn_attack_gpu)."""

    def __init__(self):
        self.cd, self.kd = ort.ChamferDist(dtype=torch.float64), _KNNDist64()

    def __call__(self, a, o, weights=None, batch_avg=True):
        return self.cd(a, o, weights, batch_avg) * 5. + self.kd(a, weights, batch_avg) * 3.


def _attack(victim, data, labels, seed=8, num_iter=10, dist_func=None, clip_func=None, adv_func=None, **kw):
    knn, adv, dist, clip = _mods()
    atk = knn.CWKNN(victim, None, None, None, None, None, adv_func=adv_func or adv.UntargetedLogitsAdvLoss(5.),
                    dist_func=dist_func or dist.ChamferkNNDist(), clip_func=clip_func or clip.ProjectInnerClipLinf(0.18),
                    attack_lr=1e-2, num_iter=num_iter, **kw)
    torch.manual_seed(seed)
    np.random.seed(seed)
    out, sn = atk.attack(torch.from_numpy(data), labels)
    return atk, out, sn


def _in_double_oracle_bands(hadv, oadv):
    dev_abs = np.abs(hadv - oadv)
    print("median", np.median(dev_abs), "share <= 1e-4", (dev_abs <= 1e-4).mean(), "q99", np.quantile(dev_abs, 0.99))
    return np.median(dev_abs) < 1e-6 and (dev_abs <= 1e-4).mean() > 0.9 and np.quantile(dev_abs, 0.99) < 1e-2


@pytest.fixture(scope="module")
def pn(dev):
    return hip_pointnet(0, dev)[0]


@pytest.fixture(scope="module")
def case():
    """3 clouds of 200 points, their labels, and the double oracle's 10 iterations (test_knn_attack_vs_double_oracle)."""
    opn, _ = oracle_pointnet(0)
    pcs = _clouds(4, 3, 200)
    with torch.no_grad():
        labels = opn(torch.from_numpy(pcs).transpose(1, 2).contiguous())[0].argmax(1)
    torch.manual_seed(8)
    oadv, osn = ort.knn_attack(opn, torch.from_numpy(pcs), labels, ort.UntargetedLogitsAdvLoss(5.), _CK64(),
                               ort.ProjectInnerClipLinf(0.18), attack_lr=1e-2, num_iter=10)
    return dict(opn=opn, pcs=pcs, labels=labels, oadv=oadv, osn=osn)


def test_golden_pointnet_chamferknn(dev, pn):
    """The real reference's run: the assertions of test_knn_attack_vs_reference_golden."""
    knn, adv, dist, clip = _mods()
    fx = np.load(os.path.join(GOLDEN, "knn.npz"))
    nm = "pointnet_chamferknn"
    iters, lr, kappa = fx[f"{nm}_cfg"]
    atk = knn.CWKNN(pn, pn, None, None, None, None, adv_func=adv.UntargetedLogitsAdvLoss(kappa), dist_func=dist.ChamferkNNDist(),
                    clip_func=clip.ProjectInnerClipLinf(budget=0.18), attack_lr=float(lr), num_iter=int(iters), device_loop=True)
    torch.manual_seed(1000)
    np.random.seed(1000)
    out, sn = atk.attack(torch.from_numpy(fx[f"{nm}_pc"]), torch.from_numpy(fx[f"{nm}_target"]))
    assert atk.last_path == "device_loop"
    assert out.dtype == np.float32 and out.shape == fx[f"{nm}_adv"].shape
    assert sn == int(fx[f"{nm}_success"])
    assert [atk.attack_fail, atk.pt_fail] == fx[f"{nm}_fails"].tolist()
    dev_abs = np.abs(out - fx[f"{nm}_adv"])
    assert np.median(dev_abs) < 5e-3 and dev_abs.max() <= 0.36 + 1e-5


def test_vs_double_oracle(dev, pn, case):
    atk, hadv, hsn = _attack(pn, case["pcs"], case["labels"], device_loop=True)
    assert atk.last_path == "device_loop"
    assert hsn == case["osn"]
    assert _in_double_oracle_bands(hadv, case["oadv"])
    with torch.no_grad():
        hl = pn(torch.from_numpy(hadv).transpose(1, 2).contiguous().to(dev))[0].argmax(1).cpu()
        ol = case["opn"](torch.from_numpy(case["oadv"]).transpose(1, 2).contiguous())[0].argmax(1)
    assert torch.equal(hl, ol)


def test_default_path_is_recorded_and_unchanged_by_the_keyword(dev, pn, case):
    a0, out0, _ = _attack(pn, case["pcs"], case["labels"])
    a1, out1, _ = _attack(pn, case["pcs"], case["labels"], device_loop=False)
    assert a0.last_path == a1.last_path == "direct" and np.array_equal(out0, out1)


@pytest.mark.parametrize("num_iter", [20, 37])
def test_graph_replay_equals_eager_and_run_equals_run(dev, pn, case, num_iter):
    _, g, gs = _attack(pn, case["pcs"], case["labels"], num_iter=num_iter, device_loop=True)
    _, e, es = _attack(pn, case["pcs"], case["labels"], num_iter=num_iter, device_loop=True, graph=False)
    _, g2, _ = _attack(pn, case["pcs"], case["labels"], num_iter=num_iter, device_loop=True)
    assert np.array_equal(g, e) and gs == es, float(np.abs(g - e).max())
    assert np.array_equal(g, g2)
    assert np.abs(g - case["pcs"]).max() > 1e-3


def test_zero_iterations_capture_nothing_and_return_the_start(dev, pn, case):
    """num_iter = 0 (what tools/bench_knn_attack.py times as the attack's fixed cost): no graph is captured, none is run."""
    a, g, gs = _attack(pn, case["pcs"], case["labels"], num_iter=0, device_loop=True)
    _, e, es = _attack(pn, case["pcs"], case["labels"], num_iter=0, device_loop=True, graph=False)
    assert a.last_path == "device_loop" and next(iter(a._loop_cache.values())).graphs is None
    assert np.array_equal(g, e) and gs == es


def test_batch_of_three_equals_three_alone(dev, pn, case):
    seeds = [41, 42, 43]
    _, out, _ = _attack(pn, case["pcs"], case["labels"], device_loop=True, sample_seeds=seeds, global_batch=3)
    for i in range(3):
        a, one, _ = _attack(pn, case["pcs"][i:i + 1], case["labels"][i:i + 1], device_loop=True, sample_seeds=[seeds[i]],
                            global_batch=3)
        assert a.last_path == "device_loop"
        assert np.array_equal(one[0], out[i]), (i, float(np.abs(one[0] - out[i]).max()))


def test_second_attack_reuses_the_graph(dev, pn, case):
    atk, first, _ = _attack(pn, case["pcs"], case["labels"], num_iter=20, device_loop=True)
    graphs = next(iter(atk._loop_cache.values())).graphs
    assert graphs is not None
    other = _clouds(9, 3, 200)
    torch.manual_seed(8)
    second, _ = atk.attack(torch.from_numpy(other), case["labels"])
    assert next(iter(atk._loop_cache.values())).graphs is graphs and atk.last_path == "device_loop"
    _, fresh, _ = _attack(pn, other, case["labels"], num_iter=20, device_loop=True)
    assert np.array_equal(second, fresh)
    assert not np.array_equal(second, first)


def test_against_the_direct_path(dev, pn, case):
    """device_loop=True against device_loop=False on the same seed. The two paths differ in how the victim's gradient is
    computed (launch-minimal passes against autograd through the graphed victim), so the clouds are held to the double
    oracle's bands against each other; the measured deviation is printed (and recorded in DESIGN.md §8.10)."""
    _, loop, ls = _attack(pn, case["pcs"], case["labels"], device_loop=True)
    _, direct, ds = _attack(pn, case["pcs"], case["labels"], device_loop=False)
    print("bit-equal:", np.array_equal(loop, direct), "max |diff|:", float(np.abs(loop - direct).max()))
    assert ls == ds
    assert _in_double_oracle_bands(loop, direct)


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
        labels = oracle_victim(torch.from_numpy(pcs).transpose(1, 2).contiguous())[0].argmax(1)
    torch.manual_seed(8)
    oadv, osn = ort.knn_attack(oracle_victim, torch.from_numpy(pcs), labels, ort.UntargetedLogitsAdvLoss(5.), _CK64(),
                               ort.ProjectInnerClipLinf(0.18), attack_lr=1e-2, num_iter=10)
    atk, hadv, hsn = _attack(m, pcs, labels, device_loop=True)
    assert atk.last_path == "device_loop" and hsn == osn
    assert _in_double_oracle_bands(hadv, oadv)


def test_six_channel_input(dev, pn, case):
    rng = np.random.default_rng(12)
    nrm = rng.standard_normal(case["pcs"].shape).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=2, keepdims=True)
    data = np.concatenate([case["pcs"], nrm], axis=2)
    torch.manual_seed(8)
    oadv, osn = ort.knn_attack(case["opn"], torch.from_numpy(data), case["labels"], ort.UntargetedLogitsAdvLoss(5.), _CK64(),
                               ort.ProjectInnerClipLinf(0.18), attack_lr=1e-2, num_iter=10)
    atk, hadv, hsn = _attack(pn, data, case["labels"], device_loop=True)
    assert atk.last_path == "device_loop" and hsn == osn and hadv.shape == case["pcs"].shape
    assert _in_double_oracle_bands(hadv, oadv)
    assert not np.array_equal(hadv, _attack(pn, case["pcs"], case["labels"], device_loop=True)[1])      # the normals were used


def _falls_back(victim, data, labels, **kw):
    a1, out1, s1 = _attack(victim, data, labels, device_loop=True, **kw)
    a0, out0, s0 = _attack(victim, data, labels, device_loop=False, **kw)
    assert a1.last_path != "device_loop" and a1.last_path == a0.last_path
    assert np.array_equal(out1, out0) and s1 == s0


def test_falls_back_on_an_ssg_victim(dev):
    knn, adv, dist, clip = _mods()
    ssg = M("3dpointcloudattack_amd.model.pointnet2_SSG").PointNet_Ssg(40)
    ssg.load_state_dict(ort.seeded_state_dict(ssg, 3))
    ssg = ssg.eval().to(dev)
    _falls_back(ssg, _clouds(6, 2, 600), torch.tensor([3, 7]), num_iter=3, dist_func=dist.ChamferDist())


def test_falls_back_on_a_hausdorff_functor(dev, pn, case):
    knn, adv, dist, clip = _mods()
    _falls_back(pn, case["pcs"], case["labels"], num_iter=4, dist_func=dist.HausdorffDist())


def test_falls_back_above_the_cap(dev, pn, ops):
    n = ops.KNN_LOOP_MAX_POINTS + 4
    _falls_back(pn, _clouds(7, 1, n), torch.tensor([5]), num_iter=2)
