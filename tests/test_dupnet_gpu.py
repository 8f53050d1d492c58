"""GPU: PU-Net / DUP-Net on the device (csrc/punet.hip, ops.three_interp, ops.pcd_tail, defense.DUPNet) against float64 torch,
against the reference fixture (tests/golden/dupnet.npz, dupnet_stages.npz — every tolerance is a band read from there) and
against the plain-torch restatement (test_dupnet_cpu.RestatedPUNet) on the same device."""
import importlib
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from helpers import hip_pointnet
from test_dupnet_cpu import WEIGHT_PARTS, RestatedPUNet, case_input, cases, grad_for_compare, load_state, restated_sor

pytestmark = pytest.mark.gpu
ops = importlib.import_module("3dpointcloudattack_amd.ops")
dfn = importlib.import_module("3dpointcloudattack_amd.defense")
pum = importlib.import_module("3dpointcloudattack_amd.attack.SIadv.baselines.defense.DUP_Net.pu_modules")
pun = importlib.import_module("3dpointcloudattack_amd.attack.SIadv.baselines.defense.DUP_Net.pu_net")
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "dupnet.npz"))


@pytest.fixture(scope="module")
def stages():
    return np.load(os.path.join(GOLDEN, "dupnet_stages.npz"))


def _punet(dev, fps_start=None):
    net = dfn.PUNet(npoint=1024, up_ratio=4, fps_start=fps_start)
    net.load_state_dict(load_state(), strict=True)
    return net.eval().to(dev)


def _interp64(u, k, F, bias=None, relu=False):
    """float64 torch: the reference's interpolation with direct-difference distances."""
    d = ((u[:, :, None, :] - k[:, None, :, :]) ** 2).sum(-1)
    dd, idx = d.topk(3, dim=-1, largest=False)
    w = 1.0 / (dd + 1e-8)
    w = w / w.sum(-1, keepdim=True)
    B = u.shape[0]
    y = (F[torch.arange(B, device=u.device).view(B, 1, 1), idx] * w.unsqueeze(-1)).sum(2)
    if bias is not None:
        y = y + bias
    return torch.relu(y) if relu else y


@pytest.mark.parametrize("B,N,M,C,cf,col,fused", [(2, 200, 3, 64, False, 0, False), (3, 1024, 128, 128, True, 0, True),
                                                   (2, 333, 512, 512, False, 0, False), (2, 256, 128, 64, True, 67, True),
                                                   (1, 64, 17, 64, False, 3, False)])
def test_three_interp_against_float64(dev, B, N, M, C, cf, col, fused):
    """Forward and the three gradients against float64 torch; an unknown point that coincides with a known one (d = 0); both
    coordinate layouts; the column-offset output with bias + ReLU in the epilogue. Tolerance from the fp32 summation length:
    3 products forward, C products per dot and up to N contributions per known row backward."""
    g = torch.Generator().manual_seed(B * 1000 + N + M + C)
    u = torch.rand(B, N, 3, generator=g) * 2 - 1
    k = torch.rand(B, M, 3, generator=g) * 2 - 1
    u[:, 5] = k[:, 1]                                                     # d = 0
    F = torch.randn(B, M, C, generator=g)
    bias = torch.randn(C, generator=g) if fused else None
    G = torch.rand(B, N, C, generator=g) + 0.5
    ud, kd, Fd = [(t.to(dev).transpose(1, 2).contiguous().transpose(1, 2) if (cf and t.shape[2] == 3) else t.to(dev)).requires_grad_()
                  for t in (u, k, F)]
    u_in, k_in = (ud.transpose(1, 2), kd.transpose(1, 2)) if cf else (ud, kd)
    if col or fused:
        buf = torch.full((B, N, col + C + 5), 7.0, device=dev)
        res = ops.three_interp(u_in, k_in, Fd, out=buf, col=col, bias=bias.to(dev) if fused else None, relu=fused, u_cf=cf, k_cf=cf)
        assert res.data_ptr() == buf.data_ptr()
        y = res[:, :, col:col + C]
        assert bool((res[:, :, :col] == 7.0).all()) and bool((res[:, :, col + C:] == 7.0).all())        # nothing else written
    else:
        y = ops.three_interp(u_in, k_in, Fd, u_cf=cf, k_cf=cf)
    u6, k6, F6 = [t.double().to(dev).requires_grad_() for t in (u, k, F)]
    y6 = _interp64(u6, k6, F6, bias.double().to(dev) if fused else None, False)
    if fused:       # ReLU: where the two disagree about the sign the value must sit within rounding of zero; the float64 gradient
        flip = (y.detach() > 0) != (y6.detach() > 0)                                  # is then taken with the device's mask
        assert float((y6.detach().abs() * flip).max()) <= 16 * EPS * float(y6.detach().abs().max())
        y6 = y6 * (y.detach() > 0)
    (y * G.to(dev)).sum().backward()
    (y6 * G.double().to(dev)).sum().backward()
    scale_y = float(y6.detach().abs().max())
    dy = float((y.detach().double() - y6.detach()).abs().max())
    assert dy <= 16 * EPS * max(scale_y, 1.0), dy
    for name, a, b, terms in (("feats", Fd.grad, F6.grad, N), ("unknown", ud.grad, u6.grad, C), ("known", kd.grad, k6.grad, N)):
        d = float((a.double() - b).abs().max())
        tol = 16 * EPS * math.sqrt(terms + C) * float(b.abs().max())
        print(f"three_interp B={B} N={N} M={M} C={C} {name}: dev {d:.2e} tol {tol:.2e}")
        assert d <= tol, (name, d, tol)
    assert bool(torch.isfinite(ud.grad).all()) and bool(torch.isfinite(kd.grad).all())


def test_pcd_tail_against_float64(dev):
    """The fused head against float64 torch, including the branch-major output order, and its backward."""
    g = torch.Generator().manual_seed(5)
    for B, N, r in ((2, 100, 4), (1, 1024, 2), (3, 77, 1)):
        h = torch.randn(r * B * N, 128, generator=g)
        w3, b3 = torch.randn(64, 128, generator=g) / 8, torch.randn(64, generator=g)
        w4, b4 = torch.randn(3, 64, generator=g) / 4, torch.randn(3, generator=g)
        G = torch.rand(B, r * N, 3, generator=g) + 0.5
        hd = h.to(dev).requires_grad_()
        out = ops.pcd_tail(hd, w3.to(dev), b3.to(dev), w4.to(dev), b4.to(dev), B, N, r)
        assert out.shape == (B, r * N, 3)
        h6 = h.double().to(dev).requires_grad_()
        y6 = torch.relu(h6 @ w3.double().to(dev).t() + b3.double().to(dev)) @ w4.double().to(dev).t() + b4.double().to(dev)
        o6 = y6.view(r, B, N, 3).permute(1, 0, 2, 3).reshape(B, r * N, 3)             # branch k at the points k*N .. (k+1)*N - 1
        (out * G.to(dev)).sum().backward()
        (o6 * G.double().to(dev)).sum().backward()
        do = float((out.detach().double() - o6.detach()).abs().max())
        dg = float((hd.grad.double() - h6.grad).abs().max())
        tol_o = 16 * EPS * math.sqrt(128 + 64) * float(o6.detach().abs().max())
        tol_g = 16 * EPS * math.sqrt(64 + 3) * float(h6.grad.abs().max())
        print(f"pcd_tail B={B} N={N} r={r}: out dev {do:.2e} tol {tol_o:.2e}; grad dev {dg:.2e} tol {tol_g:.2e}")
        assert do <= tol_o and dg <= tol_g


def _run(net, x, starts, G, pre=None, stages=False):
    x = x.detach().clone().requires_grad_()
    net.fps_start = starts
    pts = x if pre is None else pre(x).transpose(1, 2)
    res = net(pts, return_stages=stages)
    out, st = res if stages else (res, None)
    (out * G).sum().backward()
    return out.detach(), x.grad, st


def test_punet_matches_the_reference_fixture(dev, fx, stages):
    """FPS picks and ball tables equal, 3-NN lists equal as sets, stages / output / gradient inside the stored bands."""
    net = _punet(dev)
    sor = dfn.SORDefense(k=2, alpha=1.1, npoint=1024)
    for name in cases(fx):
        x, starts, G = [t.to(dev) for t in case_input(fx, name)]
        out, grad, st = _run(net, x, starts, G, pre=sor if name == "e2e" else None, stages=True)
        for k in range(4):
            assert np.array_equal(st["fps"][k].cpu().numpy(), fx[f"{name}_fps{k + 1}"].astype(np.int32)), (name, k)
        do = float((out.cpu() - torch.from_numpy(fx[f"{name}_out"])).abs().max())
        dg = float((grad_for_compare(name, grad.cpu()) - grad_for_compare(name, torch.from_numpy(fx[f"{name}_grad"]))).abs().max())
        print(f"{name}: out dev {do:.2e} band {float(fx[f'{name}_out_band']):.2e}; grad dev {dg:.2e} band "
              f"{float(fx[f'{name}_grad_band']):.2e}")
        if name == "syn":
            rows = int(stages["rows"])
            for k in range(4):
                assert np.array_equal(st["ball"][k][0].cpu().numpy(), stages[f"ball{k + 1}"].astype(np.int32)), k
            for k in range(3):
                _, idx = ops.knn_raw(st["l_xyz"][0].detach(), st["l_xyz"][k + 2].detach(), 3)
                assert np.array_equal(np.sort(idx[0].cpu().numpy(), -1), np.sort(stages[f"nn{k + 1}"].astype(np.int32), -1)), k
            for key, val in [(f"l{k}_feats", st["l_feats"][k][0, ::rows]) for k in (2, 3, 4)] + \
                    [("cat", st["cat"][0, ::rows, :259])]:
                d = float((val.detach().cpu() - torch.from_numpy(stages[key])).abs().max())
                print(f"  {key}: dev {d:.2e} band {float(stages[key + '_band']):.2e}")
                assert d <= float(stages[key + "_band"]), (key, d)
        assert do <= float(fx[f"{name}_out_band"]), (name, do)
        assert dg <= float(fx[f"{name}_grad_band"]), (name, dg)


def test_switches_agree_within_the_band(dev, fx, stages):
    """conv-before-interp == interp-before-conv and the fused tail == the layer-by-layer tail, inside the stored bands."""
    net = _punet(dev)
    x, starts, G = [t.to(dev) for t in case_input(fx, "syn")]
    ref_out, ref_grad, ref_st = _run(net, x, starts, G, stages=True)
    for mod, flag in ((pum, "CONV_BEFORE_INTERP"), (pun, "EXPAND_FUSED")):
        old = getattr(mod, flag)
        setattr(mod, flag, not old)
        try:
            out, grad, st = _run(net, x, starts, G, stages=True)
        finally:
            setattr(mod, flag, old)
        dc = float((st["cat"].detach() - ref_st["cat"].detach()).abs().max())
        do, dg = float((out - ref_out).abs().max()), float((grad - ref_grad).abs().max())
        print(f"{flag}={not old}: cat dev {dc:.2e}, out dev {do:.2e}, grad dev {dg:.2e}")
        assert dc <= float(stages["cat_band"]) and do <= float(fx["syn_out_band"]) and dg <= float(fx["syn_grad_band"]), flag


def test_dupnet_end_to_end_and_defended_logits(dev, fx):
    """DUPNet against the fixture's e2e case, and Defended(PointNet, DUPNet) logits against the restatement + the same victim."""
    x, starts, G = [t.to(dev) for t in case_input(fx, "e2e")]
    head = dfn.DUPNet(weights=WEIGHT_PARTS, fps_start=starts).to(dev)
    xg = x.clone().requires_grad_()
    out = head(xg)
    assert out.shape == (x.shape[0], 3, 4096)
    (out.transpose(1, 2) * G).sum().backward()
    do = float((out.detach().transpose(1, 2).cpu() - torch.from_numpy(fx["e2e_out"])).abs().max())
    dg = float((xg.grad.cpu() - torch.from_numpy(fx["e2e_grad"])).abs().max())
    print(f"DUPNet e2e: out dev {do:.2e} band {float(fx['e2e_out_band']):.2e}; grad dev {dg:.2e} band {float(fx['e2e_grad_band']):.2e}")
    assert do <= float(fx["e2e_out_band"]) and dg <= float(fx["e2e_grad_band"])
    victim, _ = hip_pointnet(0, dev)
    logits = dfn.Defended(victim, head)(x)[0]
    rest = RestatedPUNet(load_state(), device=dev)
    with torch.no_grad():
        up, _ = rest.forward(restated_sor(x).transpose(1, 2), starts)
        ref_logits = victim(up.transpose(1, 2).contiguous())[0]
    d = float((logits - ref_logits).abs().max())
    print(f"Defended(PointNet, DUPNet) logits dev {d:.2e} (|logit| <= {float(ref_logits.abs().max()):.2f})")
    assert torch.equal(logits.argmax(1), ref_logits.argmax(1))
    # the victim is a max over 4096 points of an MLP with Lipschitz-bounded layers: the logits move by rounding of the
    # upsampled points (band) times the MLP's gain, measured here on the restatement itself by a band-sized perturbation
    with torch.no_grad():
        bump = victim((up + float(fx["e2e_out_band"]) * torch.sign(torch.randn_like(up))).transpose(1, 2).contiguous())[0]
    gain = float((bump - ref_logits).abs().max())
    assert d <= max(16 * gain, 16 * EPS * float(ref_logits.abs().max())), (d, gain)


@pytest.mark.parametrize("det", [True, False])
def test_reproducible_run_batch_and_graph(dev, fx, det):
    """Fixed starts: run == run, a cloud in the batch == the cloud alone, eager == hipGraph replay (torch.equal, forward and
    backward) in deterministic mode; with deterministic=False agreement inside the band is all that is asked."""
    x, starts, G = [t.to(dev) for t in case_input(fx, "e2e")]
    ob, gb = float(fx["e2e_out_band"]), float(fx["e2e_grad_band"])

    def same(a, b):
        if det:
            return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        return float((a[0] - b[0]).abs().max()) <= ob and float((a[1] - b[1]).abs().max()) <= gb

    def fwd_bwd(head, xin, Gin):
        xin = xin.detach().clone().requires_grad_()
        out = head(xin)
        g, = torch.autograd.grad((out.transpose(1, 2) * Gin).sum(), xin)
        return out.detach(), g

    with ops.deterministic(det):
        head = dfn.DUPNet(weights=WEIGHT_PARTS, fps_start=starts).to(dev)
        a = fwd_bwd(head, x, G)
        assert same(a, fwd_bwd(head, x, G))
        for i in range(x.shape[0]):
            one = dfn.DUPNet(weights=WEIGHT_PARTS, fps_start=starts[:, i:i + 1]).to(dev)
            assert same((a[0][i:i + 1], a[1][i:i + 1]), fwd_bwd(one, x[i:i + 1], G[i:i + 1])), i
        sx = x.clone().requires_grad_()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                o = head(sx)
                torch.autograd.grad((o.transpose(1, 2) * G).sum(), sx)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            so = head(sx)
            sg, = torch.autograd.grad((so.transpose(1, 2) * G).sum(), sx)
        for perm in ([0, 1, 2, 3], [3, 2, 1, 0]):
            xin = x[perm]
            head_e = dfn.DUPNet(weights=WEIGHT_PARTS, fps_start=starts).to(dev)
            with torch.no_grad():
                sx.copy_(xin)
            graph.replay()
            assert same((so, sg), fwd_bwd(head_e, xin, G)), perm


def test_short_cw_run_on_the_defended_victim(dev, fx):
    """A handful of CW iterations (fused=False) through Defended(PointNet, DUPNet(fps_start=0)): finite results, and the same
    success flags as the same loop through the plain-torch restatement on this device."""
    M = importlib.import_module
    CW = M("3dpointcloudattack_amd.attack.CW.CW_attack").CW
    adv_u = M("3dpointcloudattack_amd.attack.CW.CW_utils.adv_utils")
    dist_u = M("3dpointcloudattack_amd.attack.CW.CW_utils.dist_utils")
    clip_u = M("3dpointcloudattack_amd.attack.CW.CW_utils.clip_utils")
    victim, _ = hip_pointnet(0, dev)
    head = dfn.DUPNet(weights=WEIGHT_PARTS, fps_start=0).to(dev)
    net = dfn.Defended(victim, head)
    x = torch.from_numpy(fx["e2e_x"][:2]).transpose(1, 2).contiguous()          # [B,K,3]
    with torch.no_grad():
        labels = net(x.to(dev).transpose(1, 2).contiguous())[0].argmax(1).cpu()

    class Restated(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.rest = RestatedPUNet(load_state(), device=dev)
            self.starts = torch.zeros(4, 2, dtype=torch.int32)

        def forward(self, pc):
            up, _ = self.rest.forward(restated_sor(pc).transpose(1, 2), self.starts)
            return victim(up.transpose(1, 2).contiguous())

    res = []
    for model in (net, Restated()):
        atk = CW(model, model, adv_func=adv_u.UntargetedLogitsAdvLoss(0.), clip_func=clip_u.ClipPointsLinf(0.18),
                 dist_func=dist_u.ChamferDist(), binary_step=1, num_iter=4, device=dev, fused=False)
        torch.manual_seed(0)
        bd, ba, sn = atk.attack(x, labels)
        assert np.all(np.isfinite(ba)) and ba.shape[0] == 2
        res.append((np.asarray(bd) < 1e9, sn))
    assert np.array_equal(res[0][0], res[1][0]) and res[0][1] == res[1][1], res
