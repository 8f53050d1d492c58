"""GPU: attack/additional_exp CW with device_loop=True — the fused loop around one stacked victim pass — on the golden runs
of the real reference (tests/golden/cw_additional.npz, the bands of tests/test_cw_additional_gpu.py unchanged), on a batch,
and its fall-backs to the autograd path."""
import importlib
import os
import random

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from helpers import hip_pointnet, oracle_pointnet, unit_cloud
from oracle import ref_torch as ort
from test_oracle_golden import ADDL_CASES, _AddlAdv

pytestmark = pytest.mark.gpu
M = importlib.import_module

# max |z_device_loop - z_autograd| over the coordinates of the clouds the batched case returns after 10 iterations (all
# three succeed on both paths, at the same iterations), measured on the MI355X: the two paths round the
# views and the gradient differently.
AGREEMENT_MEASURED = 1.49e-7


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "cw_additional.npz"))


def _mods():
    return (M("3dpointcloudattack_amd.attack.additional_exp.CW_attack"), M("3dpointcloudattack_amd.attack.CW.CW_utils.adv_utils"),
            M("3dpointcloudattack_amd.attack.CW.CW_utils.dist_utils"))


class _F64:
    """The oracle's distance functor evaluated in float64 (tests/test_cw_additional_gpu.py)."""

    def __init__(self, inner, per_sample):
        self.inner, self.per_sample = inner, per_sample

    def __call__(self, adv, ori, w):
        return self.inner(adv.double(), ori.double(), w, batch_avg=not self.per_sample).float()


def _seed():
    torch.manual_seed(2000)
    random.seed(2000)
    np.random.seed(2000)


def _attack(nm, dev, dist_func, **kw):
    cwm, adv, _ = _mods()
    c = ADDL_CASES[nm]
    net, _ = hip_pointnet(0, dev)
    return cwm.CW(net, cwm.AdvLossAdapter(adv.LogitsAdvLoss(c["kappa"]), adv.UntargetedLogitsAdvLoss(c["kappa"])), dist_func,
                  attack_lr=1e-2, binary_step=c["steps"], num_iter=c["iters"], whether_target=c["target"], whether_1d=c["d1"],
                  whether_renormalization=c["renorm"], whether_3Dtransform=c["eot"], whether_resample=c["resample"], **kw)


@pytest.mark.parametrize("nm", ["z_chamfer_target", "resample_chamfer_target", "free_l2_untarget"])
def test_golden_cases_on_the_device_loop(dev, fx, nm):
    cwm, _, dist = _mods()
    c = ADDL_CASES[nm]
    onet, _ = oracle_pointnet(0)
    pc, tgt, org = torch.from_numpy(fx[f"{nm}_pc"]), torch.from_numpy(fx[f"{nm}_target"]), torch.from_numpy(fx[f"{nm}_origin"])
    df = {"chamfer": dist.ChamferDist(), "l2": dist.L2Dist()}[c["dist"]]
    per_sample = not c["target"]
    # B = 1: the bare functor and PerSampleDist are both recognised
    atk = _attack(nm, dev, cwm.PerSampleDist(df) if per_sample else df, device_loop=True)
    _seed()
    bd, ba, sn = atk.attack(pc, tgt, org)
    assert atk.last_path == "device_loop"
    assert bd.shape == (1,) and ba.shape == fx[f"{nm}_bestattack"].shape and ba.dtype == np.float64
    assert sn == int(fx[f"{nm}_success"]), nm
    oi = {"chamfer": ort.ChamferDist(), "l2": ort.L2Dist()}[c["dist"]]
    _seed()
    obd, oba, osn = ort.cw_additional_attack(onet, pc, tgt, org, _AddlAdv(ort, c["kappa"]), _F64(oi, per_sample),
                                             attack_lr=1e-2, binary_step=c["steps"], num_iter=c["iters"],
                                             whether_target=c["target"], whether_1d=c["d1"],
                                             whether_renormalization=c["renorm"], whether_3Dtransform=c["eot"],
                                             whether_resample=c["resample"])
    assert sn == osn
    if sn:
        # the bands of tests/test_cw_additional_gpu.py, set there from two valid fp32 evaluations of the victim's heads
        np.testing.assert_allclose(bd, obd, rtol=5e-2, err_msg=nm)
        np.testing.assert_allclose(bd, fx[f"{nm}_bestdist"], rtol=0.15, err_msg=nm)
        frac = np.mean(np.abs(ba - oba) <= 2e-3)
        print(f"\n  {nm}: bestdist {bd} oracle {obd} fixture {fx[f'{nm}_bestdist']}  within 2e-3: {frac:.4f}")
        assert frac > (0.85 if c["eot"] else 0.97), nm
        with torch.no_grad():
            lab = onet(torch.from_numpy(ba).float().transpose(1, 2).contiguous())[0].argmax(1)
            lab_ref = onet(torch.from_numpy(fx[f"{nm}_bestattack"]).transpose(1, 2).contiguous())[0].argmax(1)
        assert torch.equal(lab, lab_ref), nm
    if c["d1"]:
        assert np.array_equal(ba[..., :2].astype(np.float32), fx[f"{nm}_pc"][..., :2])
        assert np.all(np.abs(ba[..., 2] - fx[f"{nm}_pc"][..., 2]) <= 0.4 + 1e-6)


def test_chamferknn_case_takes_the_autograd_path(dev, fx):
    """ChamferkNNDist is not in the device loop: the flag changes nothing, bit for bit."""
    _, _, dist = _mods()
    nm = "eot_renorm_chamferknn_target"
    pc, tgt, org = torch.from_numpy(fx[f"{nm}_pc"]), torch.from_numpy(fx[f"{nm}_target"]), torch.from_numpy(fx[f"{nm}_origin"])
    res = []
    for flag in (True, False):
        atk = _attack(nm, dev, dist.ChamferkNNDist(), device_loop=flag)
        _seed()
        res.append(atk.attack(pc, tgt, org))
        assert atk.last_path == "autograd"
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1]) and res[0][2] == res[1][2]


# ---------------------------------------------------------------------------------------------------------------------
# the batched case of test_additional_cw_batched: B = 3, K = 192, EOT + renorm, z-only
# ---------------------------------------------------------------------------------------------------------------------
_BATCH = {}


def _batched(dev):
    if not _BATCH:
        net, _ = hip_pointnet(0, dev)
        rng = np.random.default_rng(9)
        pcs = torch.from_numpy(np.stack([unit_cloud(rng, 192) for _ in range(3)]))
        with torch.no_grad():
            lg = net(pcs.transpose(1, 2).contiguous().to(dev))[0]
        _BATCH.update(net=net, pcs=pcs, tgt=lg.topk(2, dim=1)[1][:, 1].cpu(), org=lg.argmax(1).cpu())
    return _BATCH


def _run_batched(dev, device_loop, graph=True, resample=False, binary_step=2, num_iter=10, dist_func=None, pcs=None,
                 device=None, eot=True, block=None):
    cwm, adv, dist = _mods()
    b = _batched(dev)
    df = cwm.PerSampleDist(dist.ChamferDist()) if dist_func is None else dist_func
    atk = cwm.CW(b["net"], cwm.AdvLossAdapter(adv.LogitsAdvLoss(0.), adv.UntargetedLogitsAdvLoss(0.)), df,
                 binary_step=binary_step, num_iter=num_iter, whether_target=True, whether_1d=True, whether_3Dtransform=eot,
                 whether_renormalization=True, whether_resample=resample, graph=graph, device_loop=device_loop, device=device)
    if block is not None:
        atk.LOOP_BLOCK = block               # iterations per replay and per block of draws (the tables hold two blocks)
    _seed()
    pcs = b["pcs"] if pcs is None else pcs
    n = pcs.shape[0]
    out = atk.attack(pcs, b["tgt"][:n], b["org"][:n])
    return atk, out, (torch.get_rng_state(), random.getstate())


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


@pytest.mark.parametrize("resample", [False, True])
def test_batched_runs_agree_and_leave_the_generators_alike(dev, resample):
    # 18 iterations: one block of 16 draws and a remainder of two single-iteration replays
    atk, first, rng_first = _run_batched(dev, True, resample=resample, num_iter=18)
    assert atk.last_path == "device_loop"
    bd, ba, sn = first
    pcs = _batched(dev)["pcs"].numpy()
    assert bd.shape == (3,) and ba.shape == (3, 192, 3) and 0 <= sn <= 3 and np.isfinite(ba).all()
    assert np.array_equal(ba[..., :2].astype(np.float32), pcs[..., :2])
    assert np.all(np.abs(ba[..., 2] - pcs[..., 2]) <= 0.4 + 1e-6)
    _, again, rng_again = _run_batched(dev, True, resample=resample, num_iter=18)
    assert _same(first, again)                                            # run == run, same seeds
    _, eager, rng_eager = _run_batched(dev, True, graph=False, resample=resample, num_iter=18)
    assert _same(first, eager)                                            # graph replay == eager launches
    _, small, rng_small = _run_batched(dev, True, resample=resample, num_iter=18, block=4)
    assert _same(first, small)                                            # five blocks of draws == two: every row is the right one
    ref, _, rng_ref = _run_batched(dev, False, resample=resample, num_iter=18)
    assert ref.last_path == "autograd"
    for got in (rng_first, rng_again, rng_eager, rng_small):
        assert torch.equal(got[0], rng_ref[0]) and got[1] == rng_ref[1]


def test_fallbacks_take_the_autograd_path(dev):
    cwm, _, dist = _mods()
    df = dist.ChamferDist()
    b = _batched(dev)
    # a lambda as dist_func
    atk, _, _ = _run_batched(dev, True, binary_step=1, num_iter=1, dist_func=lambda a, o, w: df(a, o, w, batch_avg=False))
    assert atk.last_path == "autograd"
    # a bare functor at B = 3 (its batch mean is not the per-sample distance) — and the same functor at B = 1 is taken
    atk, _, _ = _run_batched(dev, True, binary_step=1, num_iter=1, dist_func=df)
    assert atk.last_path == "autograd"
    atk, _, _ = _run_batched(dev, True, binary_step=1, num_iter=1, dist_func=df, pcs=b["pcs"][:1])
    assert atk.last_path == "device_loop"
    # ChamferkNNDist inside the adapter
    atk, _, _ = _run_batched(dev, True, binary_step=1, num_iter=1, dist_func=cwm.PerSampleDist(dist.ChamferkNNDist()))
    assert atk.last_path == "autograd"
    # K above the cap
    ops = M("3dpointcloudattack_amd.ops")
    rng = np.random.default_rng(2)
    big = torch.from_numpy(unit_cloud(rng, ops.EOT_MAX_POINTS + 1)[None])
    atk, _, _ = _run_batched(dev, True, binary_step=1, num_iter=1, pcs=big, eot=False)
    assert atk.last_path == "autograd"
    # a CPU device (a plain-torch victim and the pure-torch L2Dist: this package's own victims and set distances are GPU only)
    _, adv, _ = _mods()
    onet, _ = oracle_pointnet(0)
    cpu = cwm.CW(onet, cwm.AdvLossAdapter(adv.LogitsAdvLoss(0.), adv.UntargetedLogitsAdvLoss(0.)), cwm.PerSampleDist(dist.L2Dist()),
                 binary_step=1, num_iter=1, device="cpu", device_loop=True)
    _seed()
    bd, ba, _ = cpu.attack(b["pcs"][:2, :64], b["tgt"][:2], b["org"][:2])
    assert cpu.last_path == "autograd" and ba.shape == (2, 64, 3)


def test_agreement_with_the_autograd_path(dev):
    """10 iterations of the batched case on both paths, same seeds: to rounding, not bit for bit."""
    dl, a, _ = _run_batched(dev, True, binary_step=1, num_iter=10)
    ag, b, _ = _run_batched(dev, False, binary_step=1, num_iter=10)
    assert dl.last_path == "device_loop" and ag.last_path == "autograd"
    diff = np.abs(a[1] - b[1])
    print(f"\n  success {a[2]} / {b[2]}  bestdist {a[0]} / {b[0]}  max |diff| {diff.max():.3e}  mean {diff.mean():.3e}"
          f"  within 1e-5: {np.mean(diff <= 1e-5):.4f}")
    assert a[2] == b[2]
    assert diff.max() <= 4 * AGREEMENT_MEASURED
