"""GPU: the untargeted AOF attack (attack/AOF/Eval_AOF.py) — its three kernels against torch bit for bit, the victim's
stacked pass, and the loop against the real reference's run (tests/golden/aof_untargeted.npz), its generic twin and its
eager twin."""
import importlib
import os
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from helpers import hip_pointnet, unit_cloud

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "aof_untargeted.npz"))


def _mods():
    m = importlib.import_module
    return (m("3dpointcloudattack_amd.attack.AOF.Eval_AOF"), m("3dpointcloudattack_amd.attack.CW.CW_utils.adv_utils"),
            m("3dpointcloudattack_amd.attack.CW.CW_utils.clip_utils"))


def _clouds(seed, B, N, scale=1.0):
    rng = np.random.default_rng(seed)
    return torch.from_numpy((scale * np.stack([unit_cloud(rng, N) for _ in range(B)])).astype(np.float32))


def _labels(net, pcs, dev):
    with torch.no_grad():
        return net(pcs.transpose(1, 2).contiguous().to(dev))[0].argmax(1).cpu()


# ---- pc3d_aof_record_f32 -----------------------------------------------------------------------------------------------
def _record_reference(adv, data, pred, lfc_pred, label, obd, obs, oba):
    dist = torch.amax(torch.abs(adv - data), dim=(1, 2))
    upd = (pred != label) & (dist < obd) & (lfc_pred != label)
    return dist, torch.where(upd, dist, obd), torch.where(upd, pred, obs), torch.where(upd[:, None, None], adv, oba), upd


@pytest.mark.parametrize("N", [130, 1024])
def test_record_kernel_equals_torch(ops, dev, N):
    """Two batches of B = 5. First: all three conditions true with the maximum in the cloud's last element; each condition
    false alone; dist == o_bestdist exactly. Second: a NaN coordinate; all true; all false; an improvement of an earlier
    best; a failure after an earlier best."""
    B = 5
    gen = torch.Generator().manual_seed(N)
    data = torch.randn(B, 3, N, generator=gen)
    adv = data + 0.01 * torch.randn(B, 3, N, generator=gen)
    adv[0, 2, N - 1] = data[0, 2, N - 1] + 0.5                       # the maximum sits in the last element
    label = torch.tensor([3, 3, 3, 3, 3])
    dist = torch.amax(torch.abs(adv - data), dim=(1, 2))
    batches = [dict(pred=torch.tensor([7, 3, 7, 7, 7]), lfc=torch.tensor([8, 8, 8, 3, 8]),
                    obd=torch.stack([torch.tensor(1e10), torch.tensor(1e10), dist[2] * 0.5, torch.tensor(1e10), dist[4]]),
                    want=[True, False, False, False, False], adv=adv)]
    adv2 = adv.clone()
    adv2[0, 1, N // 2] = float("nan")
    batches.append(dict(pred=torch.tensor([7, 7, 3, 9, 3]), lfc=torch.tensor([8, 8, 3, 8, 8]),
                        obd=torch.stack([torch.tensor(1e10), torch.tensor(1e10), torch.tensor(1e10), dist[3] * 2, dist[4] * 2]),
                        want=[False, True, False, True, False], adv=adv2))
    for bt in batches:
        a = bt["adv"].to(dev)
        d = data.to(dev)
        both = torch.cat([bt["pred"], bt["lfc"]]).to(dev)            # the two predictions as the halves of one [2B] tensor
        lab = label.to(dev)
        obd, obs = bt["obd"].clone().to(dev), torch.full((B,), -1, dtype=torch.long, device=dev)
        oba = torch.full((B, 3, N), 0.25, device=dev)
        dist_ref, obd_ref, obs_ref, oba_ref, upd = _record_reference(a, d, both[:B], both[B:], lab, obd, obs, oba)
        assert upd.tolist() == bt["want"]
        dv = torch.full((B,), -1.0, device=dev)
        step = torch.tensor([4], dtype=torch.int32, device=dev)
        ops.aof_record(a, d, both[:B], both[B:], lab, obd, obs, oba, dist_val=dv, step=step)
        assert torch.equal(obd, obd_ref) and torch.equal(obs, obs_ref) and torch.equal(oba, oba_ref)
        assert torch.equal(torch.isnan(dv), torch.isnan(dist_ref))
        assert torch.equal(torch.nan_to_num(dv, nan=-1.0), torch.nan_to_num(dist_ref, nan=-1.0))
        assert int(step.item()) == 5
        # without the optional outputs: the same bests
        obd2, obs2, oba2 = bt["obd"].clone().to(dev), torch.full((B,), -1, dtype=torch.long, device=dev), torch.full((B, 3, N), 0.25, device=dev)
        ops.aof_record(a, d, both[:B], both[B:], lab, obd2, obs2, oba2)
        assert torch.equal(obd2, obd_ref) and torch.equal(obs2, obs_ref) and torch.equal(oba2, oba_ref)


# ---- pc3d_aof_update_f32 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [130, 1024])
@pytest.mark.parametrize("t", [1, 7])
@pytest.mark.parametrize("budget", [0.05, 0.0])
def test_update_kernel_equals_the_three_launch_composition(ops, dev, N, t, budget):
    """Adam (ops.adam_clip_step with g2) + torch.add + this package's ClipPointsLinf against the one launch: the same bits
    in lfc, m, v and the clipped cloud. The displacements straddle the budget; the first points do not move at all."""
    clip = _mods()[2]
    B, lr = 3, 1e-2
    gen = torch.Generator().manual_seed(1000 * N + t)
    r = lambda s=1.0: (s * torch.randn(B, 3, N, generator=gen)).to(dev)
    lfc, hfc, g1, g2 = r(0.5), r(0.1), r(1e-3), r(1e-3)
    m = r(1e-3) if t > 1 else torch.zeros(B, 3, N, device=dev)
    v = r(1e-3).square() if t > 1 else torch.zeros(B, 3, N, device=dev)
    still = slice(0, 9)                                  # zero gradient, zero momentum: these points stay where they are
    g1[:, :, still] = 0
    g2[:, :, still] = 0
    m[:, :, still] = 0
    delta = r()
    delta = delta / delta.norm(dim=1, keepdim=True) * (0.1 * torch.rand(B, 1, N, generator=gen)).to(dev)     # norms in [0, 0.1)
    data = torch.add(lfc, hfc) - delta
    data[:, :, still] = torch.add(lfc, hfc)[:, :, still]            # ... and coincide with the data: zero displacement
    step = torch.tensor([t], dtype=torch.int32, device=dev)
    # the composition
    lfc_c, m_c, v_c = lfc.clone(), m.clone(), v.clone()
    ops.adam_clip_step(lfc_c, g1, m_c, v_c, step, lr, g2=g2)
    out_c = clip.ClipPointsLinf(budget)(torch.add(lfc_c, hfc), data)
    # the launch
    lfc_k, m_k, v_k = lfc.clone(), m.clone(), v.clone()
    out_k = ops.aof_update(lfc_k, g1, g2, m_k, v_k, hfc, data, step, lr, budget)
    assert torch.equal(lfc_k, lfc_c) and torch.equal(m_k, m_c) and torch.equal(v_k, v_c) and torch.equal(out_k, out_c)
    assert torch.equal(out_k[:, :, still], data[:, :, still])
    moved = (out_k - data).norm(dim=1)
    if budget > 0:
        scaled = (torch.add(lfc_c, hfc) - data).norm(dim=1) > budget
        assert scaled.any() and (~scaled).any()                     # some points clipped, some not
        assert float(moved.max()) <= budget * (1 + 1e-5)
    # the host step number gives the same bits as the device word
    lfc_h, m_h, v_h = lfc.clone(), m.clone(), v.clone()
    out_h = ops.aof_update(lfc_h, g1, g2, m_h, v_h, hfc, data, t, lr, budget)
    assert torch.equal(out_h, out_k) and torch.equal(lfc_h, lfc_k)


# ---- pc3d_spectral_reproject_sum_f32 -----------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,lp", [(1, 130, 7), (2, 256, 0), (2, 256, 256), (2, 1000, 101), (2, 1024, 100)])
def test_reproject_sum_keeps_the_bands_and_adds_exactly(ops, dev, B, N, lp):
    gen = torch.Generator().manual_seed(N + lp)
    V = (torch.randn(B, N, N, generator=gen) / N ** 0.5).to(dev)
    Vt = V.transpose(1, 2).contiguous()
    adv = (0.4 * torch.randn(B, 3, N, generator=gen)).to(dev)
    lfc0, hfc0 = ops.spectral_reproject(adv, V, Vt, lp)
    lfc, hfc, coeff, s = (torch.full((B, 3, N), 7.0, device=dev) for _ in range(4))
    ops.spectral_reproject(adv, V, Vt, lp, lfc, hfc, coeff, sum=s)
    assert torch.equal(lfc, lfc0) and torch.equal(hfc, hfc0)
    assert torch.equal(s, lfc + hfc)
    # the loop's layout: lfc and the sum are the two halves of one [2B,3,N] buffer
    buf = torch.full((2 * B, 3, N), 7.0, device=dev)
    hfc2 = torch.empty_like(hfc)
    ops.spectral_reproject(adv, V, Vt, lp, buf[B:], hfc2, coeff, sum=buf[:B])
    assert torch.equal(buf[B:], lfc0) and torch.equal(hfc2, hfc0) and torch.equal(buf[:B], s)


# ---- the victim's stacked pass -----------------------------------------------------------------------------------------
def test_stacked_pass_equals_two_passes(dev):
    """fused_loss_and_grad on [2B] clouds with scale = 0.5 / B against one call per half: a cloud's prediction and gradient
    do not depend on what else is in the batch."""
    B, N = 3, 160
    net, _ = hip_pointnet(0, dev)
    a = _clouds(21, B, N).transpose(1, 2).contiguous().to(dev)
    b = (a + 0.01 * torch.randn(B, 3, N, generator=torch.Generator().manual_seed(2)).to(dev)).contiguous()
    label = _labels(net, a.transpose(1, 2).cpu(), dev).to(dev)
    with torch.no_grad():
        _, pred2, loss2, g2 = net.fused_loss_and_grad(torch.cat([a, b]).contiguous(), label.repeat(2), "untargeted_logits", 30.0,
                                                      scale=0.5 / B)
        _, pa, la, ga = net.fused_loss_and_grad(a, label, "untargeted_logits", 30.0, scale=0.5 / B)
        _, pb, lb, gb = net.fused_loss_and_grad(b, label, "untargeted_logits", 30.0, scale=0.5 / B)
    assert torch.equal(pred2[:B], pa) and torch.equal(pred2[B:], pb)
    assert torch.equal(loss2[:B], la) and torch.equal(loss2[B:], lb)
    assert float(g2.abs().max()) > 0
    assert torch.equal(g2[:B], ga) and torch.equal(g2[B:], gb)


# ---- the loop ----------------------------------------------------------------------------------------------------------
def _case(fx, case):
    return {k.split("/", 1)[1]: fx[k] for k in fx.files if k.startswith(case + "/")}


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("case", ["mixed", "long"])
def test_attack_vs_reference(dev, fx, case, fused):
    """AOF.attack against the REAL reference's run. Discrete outcomes are equal (the fixture's margins keep every decision
    1e-2 away from a tie); o_bestdist of the found clouds and the final clouds lie inside the fixture's bands (2.5 x the
    deviation of an fp32 run from the float64 run, see tests/golden/make_golden_aof_untargeted.py); a never-found cloud is
    clip(0, data). Measured on MI355X, generic and fused alike: mixed — distance 2.0e-6 of band 6.7e-6, clouds q90 8.1e-7 / q99
    1.8e-6 of 1.6e-6 / 4.4e-6; long — distance 2.4e-6 of 2.2e-5, clouds median 1.1e-6 / q90 2.8e-6 / q99 4.7e-6 of 3.1e-6 / 8.1e-6 / 1.3e-5."""
    ea, adv, clip = _mods()
    f = _case(fx, case)
    net, _ = hip_pointnet(0, dev)
    trans, _ = hip_pointnet(1, dev)
    atk = ea.AOF(net, trans, adv.UntargetedLogitsAdvLoss(kappa=float(f["kappa"])), clip.ClipPointsLinf(budget=float(f["budget"])),
                 lr=float(f["lr"]), low_pass=int(f["low_pass"]), step=int(f["step"]), epochs=int(f["epochs"]),
                 batch_size=int(f["batch_size"]), fused=fused)
    assert (atk._fused_kind() is not None) == fused
    torch.manual_seed(int(f["torch_seed"]))
    np.random.seed(int(f["torch_seed"]))
    bd, out, sn = atk.attack(torch.from_numpy(f["data"]), torch.from_numpy(f["label"]))
    assert out.shape == f["best_pc"].shape and out.dtype == np.float32 and bd.dtype == np.float64
    found = f["o_bestscore"] >= 0
    dev_abs = np.abs(out.astype(np.float64) - f["best_pc"])
    ddist = np.abs(bd[found] - f["o_bestdist"][found])
    print(f"{case} fused={fused}: found {(bd < 1e9).astype(int).tolist()} o_bestdist {ddist.max() if found.any() else 0:.2e} "
          f"(band {float(f['band_dist_abs']):.2e}; relative {(ddist / f['o_bestdist'][found]).max():.2e}) clouds median {np.median(dev_abs):.2e} q90 {np.quantile(dev_abs, 0.9):.2e} "
          f"q99 {np.quantile(dev_abs, 0.99):.2e} max {dev_abs.max():.2e} (bands {float(f['band_pc_q50']):.2e} "
          f"{float(f['band_pc_q90']):.2e} {float(f['band_pc_q99']):.2e})")
    assert np.array_equal(bd < 1e9, found)
    assert np.array_equal(atk.o_bestscore.cpu().numpy(), f["o_bestscore"])
    assert np.array_equal(atk.preds.cpu().numpy(), f["preds"]) and np.array_equal(atk.trans_preds.cpu().numpy(), f["trans_preds"])
    assert np.array_equal(atk.shuffle_preds.cpu().numpy(), f["shuffle_preds"])
    assert np.array_equal(atk.shuffle_trans_preds.cpu().numpy(), f["shuffle_trans_preds"])
    assert sn == int(f["at_num"]) and atk.trans_num == int(f["trans_num"])
    assert np.all(bd[~found] == 1e10)
    # a never-found cloud: the zero cloud clipped towards the last noisy cloud, exactly
    if (~found).any():
        last = torch.from_numpy(f["data_last"]).to(dev)
        want = clip.ClipPointsLinf(float(f["budget"]))(torch.zeros_like(last), last).transpose(1, 2).cpu().numpy()
        assert np.array_equal(out[~found], want[~found])
    assert ddist.max() <= float(f["band_dist_abs"])
    assert np.median(dev_abs) <= float(f["band_pc_q50"]) and (dev_abs <= float(f["band_pc_q90"])).mean() >= 0.9 \
        and np.quantile(dev_abs, 0.99) <= float(f["band_pc_q99"])


def _run(ea, adv, clip, net, trans, pcs, y, seed, **kw):
    atk = ea.AOF(net, trans, adv.UntargetedLogitsAdvLoss(kappa=kw.pop("kappa", 30.)), clip.ClipPointsLinf(0.18), **kw)
    torch.manual_seed(seed)
    np.random.seed(seed)
    bd, out, sn = atk.attack(pcs, y)
    return atk, bd, out, sn


def _assert_twins(a, b):
    (atk0, bd0, out0, sn0), (atk1, bd1, out1, sn1) = a, b
    found = bd0 < 1e9
    assert found.any(), "the case must exercise the best-so-far update"
    assert np.array_equal(found, bd1 < 1e9) and sn0 == sn1 and atk0.trans_num == atk1.trans_num
    assert torch.equal(atk0.o_bestscore, atk1.o_bestscore) and torch.equal(atk0.preds, atk1.preds)
    np.testing.assert_allclose(bd1[found], bd0[found], rtol=1e-3)
    d = np.abs(out1 - out0)      # autograd vs the fused backward over the Adam steps; one step off would show as ~1e-2 (= lr)
    assert d.max() < 1e-3 and np.median(d) < 1e-5


def test_fused_equals_generic(dev):
    ea, adv, clip = _mods()
    net, _ = hip_pointnet(0, dev)
    trans, _ = hip_pointnet(1, dev)
    pcs = _clouds(FUSED_SEED, 6, 192)
    y = _labels(net, pcs, dev)
    res = [_run(ea, adv, clip, net, trans, pcs, y, 6, lr=1e-2, low_pass=30, step=2, epochs=12, fused=fused) for fused in (False, True)]
    assert res[0][0]._fused_kind() is None and res[1][0]._fused_kind() is not None
    _assert_twins(*res)


FUSED_SEED = 51     # chosen with tests/aof_restatement.py on the CPU: clouds found and not found, every in-loop margin >= 1.7e-2


def test_graph_replay_equals_eager(dev):
    """The replayed iteration (graphs of GRAPH_BLOCK iterations and of one) reproduces the eager fused path bit for bit;
    epochs = GRAPH_BLOCK + 1 runs both graph sizes."""
    ea, adv, clip = _mods()
    assert ea.GRAPH_BLOCK == 8
    net, _ = hip_pointnet(0, dev)
    trans, _ = hip_pointnet(1, dev)
    pcs = _clouds(15, 3, 160)
    y = _labels(net, pcs, dev)
    outs = [_run(ea, adv, clip, net, trans, pcs, y, 4, low_pass=30, step=2, epochs=9, graph=graph) for graph in (False, True)]
    (a0, bd0, out0, sn0), (a1, bd1, out1, sn1) = outs
    assert np.array_equal(bd0, bd1) and np.array_equal(out0, out1) and sn0 == sn1
    assert torch.equal(a0.o_bestscore, a1.o_bestscore) and torch.equal(a0.shuffle_preds, a1.shuffle_preds)


def test_module_level_attack_counts(dev, capsys):
    """Two batches of B = 2 with args.batch_size = 5: total_num follows the argument, the counts add up across batches."""
    ea, adv, clip = _mods()
    net, _ = hip_pointnet(0, dev)
    trans, _ = hip_pointnet(1, dev)
    pcs = _clouds(60, 4, 128)
    y = _labels(net, pcs, dev)
    loader = [(pcs[:2], y[:2]), (pcs[2:], y[2:])]
    args = types.SimpleNamespace(step=1, low_pass=20, lr=1e-2, epochs=3, batch_size=5)
    kw = dict(args=args, model=net, trans_model=trans, test_loader=loader, adv_func=adv.UntargetedLogitsAdvLoss(30.),
              clip_func=clip.ClipPointsLinf(0.18))
    torch.manual_seed(5)
    np.random.seed(5)
    all_pc, all_lbl, at_num, trans_num, total_num = ea.attack(device=dev, **kw)
    printed = capsys.readouterr().out
    assert total_num == 10.0 and all_pc.shape == (4, 128, 3) and np.array_equal(all_lbl, y.numpy())
    with torch.no_grad():
        x = torch.from_numpy(all_pc).transpose(1, 2).contiguous().to(dev)
        want_at = int((net(x)[0].argmax(1).cpu() != y).sum())
        want_tr = int((trans(x)[0].argmax(1).cpu() != y).sum())
    assert at_num == want_at and trans_num == want_tr
    assert f"attack success rate:{at_num / total_num}, trans success rate: {trans_num / total_num}, consuming time:" in printed
    # the same through the module's globals, as the reference's driver sets them
    saved = {k: getattr(ea, k) for k in kw}
    try:
        for k, v in kw.items():
            setattr(ea, k, v)
        torch.manual_seed(5)
        np.random.seed(5)
        again = ea.attack(device=dev)
    finally:
        for k, v in saved.items():
            setattr(ea, k, v)
    capsys.readouterr()
    assert np.array_equal(again[0], all_pc) and again[2:] == (at_num, trans_num, total_num)


def test_feature_transform_victim_takes_the_fused_path(dev):
    ea, adv, clip = _mods()
    pn = importlib.import_module("3dpointcloudattack_amd.model.pointnet")
    seeding = importlib.import_module("3dpointcloudattack_amd.seeding")
    nets = []
    for seed in (0, 1):
        m = pn.PointNetCls(k=40, feature_transform=True)
        m.load_state_dict(seeding.seeded_state_dict(m, seed), strict=True)
        nets.append(m.eval().to(dev))
    pcs = _clouds(FT_SEED, 4, 128, scale=0.5)       # half scale: this seeded victim's logits reach several hundred at unit scale
    y = _labels(nets[0], pcs, dev)
    res = [_run(ea, adv, clip, nets[0], nets[1], pcs, y, 3, kappa=FT_KAPPA, lr=1e-2, low_pass=20, step=2, epochs=6, fused=fused)
           for fused in (False, True)]
    assert res[0][0]._fused_kind() is None and res[1][0]._fused_kind() is not None
    _assert_twins(*res)


FT_SEED, FT_KAPPA = 70, 30.     # chosen on the CPU likewise (feature-transform victim): all four found, margins >= 4e-2
