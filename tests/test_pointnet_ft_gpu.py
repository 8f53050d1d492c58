"""PointNetCls(k, feature_transform=True) on the GPU: parity with the real reference (tests/golden/pointnet_ft.npz), the
fused entry points against forward() + autograd, dL/dTf on its own, the bit-for-bit properties, and the attacks that
reach the victim through the fused entry points (CW, ISO, SI-Adv)."""
import importlib
import os
import types

import numpy as np
import pytest
import torch

import pointnet_ft_restatement as rst
from conftest import GOLDEN
from helpers import unit_cloud
from test_iso_cpu import case_args

pytestmark = pytest.mark.gpu
M = importlib.import_module
ops = M("3dpointcloudattack_amd.ops")
pn = M("3dpointcloudattack_amd.model.pointnet")
seeding = M("3dpointcloudattack_amd.seeding")

NAMES = ["b1_n1", "b2_n130", "b3_n200", "b2_n1024", "k7_b2_n130", "ties_b1_n144"]
TIE = 16
U = 2.0 ** -24


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "pointnet_ft.npz"))


@pytest.fixture(scope="module")
def victim(dev):
    """victim(k, seed) -> the seeded feature-transform PointNetCls on the GPU (one instance per (k, seed))."""
    cache = {}

    def get(k=40, seed=0):
        if (k, seed) not in cache:
            m = pn.PointNetCls(k=k, feature_transform=True)
            m.load_state_dict(seeding.seeded_state_dict(m, seed), strict=True)
            cache[(k, seed)] = m.eval().to(dev)
        return cache[(k, seed)]
    return get


def clouds(seed, B, N, dev):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(np.stack([unit_cloud(rng, N) for _ in range(B)])).transpose(1, 2).contiguous().to(dev)


def fold_ties(g):
    g = g.copy()
    g[:, :, :TIE] += g[:, :, -TIE:]
    return g[:, :, :-TIE]


def test_fixture_lists_the_cases(fx):
    assert [str(n) for n in fx["names"]] == NAMES


@pytest.mark.parametrize("nm", NAMES)
def test_parity_with_the_reference(dev, fx, victim, nm):
    """logp, trans, trans_feat and gx against the reference's FLOAT64 arrays. Band: 4x the reference's own
    fp32-vs-float64 deviation (the largest absolute one of the quantity in the case); the factor is for the two 64-term
    sums that folding Tf into W2 and the MFMA K order re-associate. gx: >= 99.5 % of the elements inside the band and a
    global relative L2 < 2e-3 (a max-pool route or a ReLU within rounding of a tie may resolve differently and moves a
    channel's gradient; the generator refused cases in which the reference itself does that). The tie case compares
    the total of each tied pair.

    Measured on MI355X (largest deviation from float64 as a multiple of the reference's own; gx: share inside the band,
    relative L2 of the mirror / of the reference):
      b1_n1         logp 0.90  trans 1.65  trans_feat 1.19   gx 100 %  4.9e-7 / 3.3e-7
      b2_n130       logp 1.07  trans 1.42  trans_feat 1.00   gx 100 %  5.8e-7 / 5.7e-7
      b3_n200       logp 1.43  trans 0.90  trans_feat 1.12   gx 100 %  5.4e-7 / 5.0e-7
      b2_n1024      logp 1.03  trans 1.47  trans_feat 1.15   gx 100 %  6.9e-7 / 6.4e-7
      k7_b2_n130    logp 0.73  trans 1.63  trans_feat 1.19   gx 100 %  4.2e-7 / 4.6e-7
      ties_b1_n144  logp 1.15  trans 1.58  trans_feat 1.06   gx 100 %  5.2e-7 / 6.8e-7
    b1_n1 is the case that needs the blocked gather of pc3d_pointnet_ft_tower_bwd_f32 in all three towers: its one point
    wins all 1024 channels of every tower, and summed as one fma chain (as pointmlp3_max_bwd_kernel sums them) the
    largest gx element was off by 2.4e-5 against a band of 1.8e-5 (relative L2 1.4e-6); in blocks of 32 it is 8.3e-6."""
    k, seed = (int(v) for v in fx[f"{nm}_model"])
    model = victim(k, seed)
    assert seeding.state_sha256(model.state_dict()) == str(fx[f"sha256_k{k}_s{seed}"])
    x = torch.from_numpy(fx[f"{nm}_x"]).to(dev).requires_grad_()
    logp, trans, tf = model(x)
    assert tf.shape == (x.shape[0], 64, 64) and not tf.requires_grad
    (logp * torch.from_numpy(fx[f"{nm}_w"]).to(dev)).sum().backward()
    fails = []
    for got, q in ((logp, "logp"), (trans, "trans"), (tf, "trans_feat")):
        ref32, ref64 = fx[f"{nm}_{q}"], fx[f"{nm}_{q}64"]
        own = np.abs(ref32 - ref64).max()
        dev_ = np.abs(got.detach().cpu().numpy().astype(np.float64) - ref64).max()
        print(f"{nm} {q}: mirror-vs-f64 {dev_:.3e}, reference fp32-vs-f64 {own:.3e}, ratio {dev_ / own:.2f}")
        if not dev_ <= 4.0 * own:
            fails.append((q, dev_, own))
    assert np.array_equal(logp.argmax(1).cpu().numpy(), fx[f"{nm}_logp64"].argmax(1))
    got, g32, g64 = x.grad.cpu().numpy().astype(np.float64), fx[f"{nm}_gx"], fx[f"{nm}_gx64"]
    if nm.startswith("ties"):
        got, g32, g64 = fold_ties(got), fold_ties(g32), fold_ties(g64)
    own = np.abs(g32 - g64).max()
    inside = (np.abs(got - g64) <= 4.0 * own).mean()
    rel = np.linalg.norm(got - g64) / np.linalg.norm(g64)
    print(f"{nm} gx: {inside:.4f} inside 4 x {own:.3e}, largest {np.abs(got - g64).max():.3e}, relative L2 {rel:.3e} "
          f"(reference {np.linalg.norm(g32 - g64) / np.linalg.norm(g64):.3e})")
    assert not fails, fails
    assert inside >= 0.995 and rel < 2e-3


def test_restatement_on_the_device_brackets_the_mirror(dev, fx, victim):
    """The plain-torch restatement (the bench's comparator) on the same GPU: in float64 it reproduces the reference's
    float64 logp, and the mirror sits inside the fixture's band around it."""
    nm = "b3_n200"
    model = victim()
    sd = {k: v.double() for k, v in model.state_dict().items()}
    x = torch.from_numpy(fx[f"{nm}_x"]).to(dev)
    with torch.no_grad():
        logp64 = rst.forward(sd, x, torch.float64)[0]
        logp = model(x)[0]
    ref = fx[f"{nm}_logp64"]
    np.testing.assert_allclose(logp64.cpu().numpy(), ref, rtol=1e-9, atol=1e-10 * np.abs(ref).max())
    assert float((logp.double() - logp64).abs().max()) <= 4.0 * np.abs(fx[f"{nm}_logp"] - ref).max()


@pytest.mark.parametrize("kind,kappa", [("untargeted_logits", 5.0), ("logits", 0.0), ("cross_entropy", 0.0)])
def test_fused_entry_points_equal_autograd_path(dev, victim, kind, kappa):
    """fused_loss_and_grad and fused_attack_grad against forward() + autograd, with the tolerances of
    test_fused_loss_and_grad_equals_autograd_path (the two paths run the 3x3 STN's and the classifier's heads on
    different kernels: one hidden unit within rounding of its ReLU may flip in one sample).
    The clouds are scaled by 0.5: at unit scale this seeded victim's logits reach 700, where ONE fp32 ulp of a logit is
    6e-5 — and the cross-entropy gradient is proportional to exp(logit differences), so the two paths' roundings of the
    logits alone separate it by 3e-5 ... 1.2e-4 (measured), above the cited tolerance of 2e-5. At half scale the
    logits stay below 64 (ulp 4e-6) and the tolerance means what it meant for the plain victim."""
    adv = M("3dpointcloudattack_amd.attack.CW.CW_utils.adv_utils")
    model = victim()
    x = 0.5 * clouds(8, 5, 300, dev)
    with torch.no_grad():
        tgt = model(x)[0].argmax(1)
    if kind == "logits":
        tgt = (tgt + 3) % 40
    fn = {"untargeted_logits": adv.UntargetedLogitsAdvLoss(kappa), "logits": adv.LogitsAdvLoss(kappa),
          "cross_entropy": adv.CrossEntropyAdvLoss()}[kind]
    xa = x.clone().requires_grad_()
    logp_a = model(xa)[0]
    fn(logp_a, tgt).mean().backward()
    logp, pred, loss, gx = model.fused_loss_and_grad(x, tgt, kind, kappa)
    torch.testing.assert_close(logp, logp_a.detach(), rtol=1e-4, atol=2e-5)
    assert torch.equal(pred, logp_a.argmax(1))
    pred2, loss2, gx2 = model.fused_attack_grad(x, tgt, kind, kappa)
    assert torch.equal(pred2, pred)
    torch.testing.assert_close(loss2, loss, rtol=1e-5, atol=1e-6)
    ref = xa.grad
    for g in (gx, gx2):
        rel = torch.stack([(g[b] - ref[b]).norm() / ref[b].norm() for b in range(g.shape[0])])
        assert int((rel < 2e-5).sum()) >= g.shape[0] - 1, rel.tolist()
        assert float(rel.max()) < 0.3, rel.tolist()


def test_dLdTf_of_the_raw_backward_entries(dev, victim):
    """pc3d_pointnet_ft_tower_bwd_f32 (trunk form) + pc3d_pointnet_ft_dtf_f32 at N = 130 against a float64 evaluation
    that takes the SAME routes (the forward launch's arg-max indices and ReLU masks), so only rounding separates them:
    |got - ref| <= gamma * sum of the absolute values of every product, gamma = (1024 + 128 + N + 16) u for the gather
    over <= 1024 channels, the 128-term product with W2, the N-term sum and the recomputation of h."""
    B, N = 2, 130
    model = victim()
    W1, b1, W2, b2, W3, b3 = model.feat.folded()[:6]
    rng = np.random.default_rng(5)
    x = clouds(6, B, N, dev)
    T = (torch.eye(3) + 0.2 * torch.from_numpy(rng.standard_normal((B, 3, 3)).astype(np.float32))).to(dev).contiguous()
    Tf = (torch.eye(64) + 0.1 * torch.from_numpy(rng.standard_normal((B, 64, 64)).astype(np.float32))).to(dev).contiguous()
    g = torch.from_numpy(rng.standard_normal((B, 1024)).astype(np.float32)).to(dev)
    W2b = ops.pointnet_ft_fold_w2(W2, Tf)
    torch.testing.assert_close(W2b, torch.einsum("cj,bij->bci", W2, Tf), rtol=1e-5, atol=1e-5)
    pooled, idx, masks = ops.pointnet_ft_tower_fwd_raw(x, T, W1, b1, W2b, b2, W3, b3, False)
    part_gT, nt = ops.pointnet_ft_gT_workspace(B, N, dev)
    gx, q = ops.pointnet_ft_tower_bwd_raw(x, T, W1, W2b, W3, idx, g, masks, part_gT, 0, W2q=W2)
    got = ops.pointnet_ft_dtf_raw(x, T, W1, b1, q).view(B, 64, 64).double().cpu()
    d = lambda t: t.double().cpu()      # noqa: E731
    xp = torch.einsum("bcd,bcn->bdn", d(T), d(x))
    pre = torch.einsum("ic,bcn->bin", d(W1), xp) + d(b1)[None, :, None]
    h = torch.relu(pre)
    mag_h = torch.einsum("ic,bcn->bin", d(W1).abs(), xp.abs()) + d(b1).abs()[None, :, None]
    m2 = masks[1].cpu()                                                      # [B,N,4] int32 -> [B,N,128] bool
    on = ((m2[..., None] >> torch.arange(32)) & 1).bool().reshape(B, N, 128)
    route = torch.zeros(B, N, 1024, dtype=torch.float64)
    route.scatter_(1, idx.long().cpu()[:, None, :], d(g)[:, None, :])       # route[b, idx[b,c], c] = g[b,c]
    g_z2 = torch.einsum("bnc,ck->bnk", route, d(W3)) * on
    mag_z2 = torch.einsum("bnc,ck->bnk", route.abs(), d(W3).abs()) * on
    ref_q = torch.einsum("bnk,kj->bnj", g_z2, d(W2))
    mag_q = torch.einsum("bnk,kj->bnj", mag_z2, d(W2).abs())
    ref = torch.einsum("bin,bnj->bij", h, ref_q)
    mag = torch.einsum("bin,bnj->bij", mag_h, mag_q)
    gamma = (1024 + 128 + N + 16) * U
    assert float((d(q) - ref_q).abs().max()) > 0 or float(ref_q.abs().max()) > 0
    assert bool(((d(q) - ref_q).abs() <= (1024 + 128 + 8) * U * mag_q).all())
    worst = float(((got - ref).abs() / mag).max())
    print(f"dL/dTf: largest |got - ref| / magnitude {worst:.3e} (gamma {gamma:.3e}); largest |dL/dTf| {float(ref.abs().max()):.3e}")
    assert float(ref.abs().max()) > 0 and worst <= gamma


@pytest.mark.parametrize("B,N", [(1, 1), (2, 130)])
def test_plain_form_of_the_backward_equals_the_shipped_tower_backward(dev, victim, B, N):
    """pc3d_pointnet_ft_tower_bwd_f32 without a transform (the form STN3d's tower takes in this victim) against
    pc3d_pointmlp3_max_bwd_f32 on the same forward: the same routes and masks, only the order of the gather's sum
    differs (blocks of 32 against one chain of <= 1024 terms): gamma_1024 = 1024 u of the gradient's scale."""
    tower = victim().feat.stn.folded()[0]
    x = clouds(21, B, N, dev)
    g = torch.from_numpy(np.random.default_rng(3).standard_normal((B, 1024)).astype(np.float32)).to(dev)
    pooled, idx, masks = ops.pointmlp3_max_fwd_raw(x, tower, True, want_masks=True)
    g = g * (pooled > 0)
    ref = ops.pointmlp3_max_bwd_raw(x, tower, idx, g, masks)
    got, q = ops.pointnet_ft_tower_bwd_raw(x, None, tower[0], tower[2], tower[4], idx, g, masks, None, 0)
    assert q is None and float(ref.abs().max()) > 0
    assert float((got - ref).abs().max()) <= 1024 * U * float(ref.abs().max())
    acc = ops.pointnet_ft_tower_bwd_raw(x, None, tower[0], tower[2], tower[4], idx, g, masks, None, 0, out=ref.clone(),
                                        accumulate=True)[0]
    assert torch.equal(acc, ref + got)


def _bitwise_only():
    if os.environ.get("PC3D_DETERMINISTIC", "1") == "0":
        pytest.skip("asserts bit-equality: deterministic mode only")


def test_run_equals_run_and_cloud_in_batch_equals_cloud_alone(dev, fx, victim):
    _bitwise_only()
    model = victim()
    x = torch.from_numpy(fx["b3_n200_x"]).to(dev)
    with torch.no_grad():
        tgt = model(x)[0].argmax(1)              # the clean labels: the untargeted loss is active
    first = model.fused_loss_and_grad(x, tgt, "untargeted_logits", 5.0, scale=1.0)
    for _ in range(10):
        again = model.fused_loss_and_grad(x, tgt, "untargeted_logits", 5.0, scale=1.0)
        assert all(torch.equal(a, b) for a, b in zip(first, again))
    assert torch.isfinite(first[3]).all() and float(first[3].abs().max()) > 0
    for b in range(3):
        alone = model.fused_loss_and_grad(x[b:b + 1], tgt[b:b + 1], "untargeted_logits", 5.0, scale=1.0)
        assert all(torch.equal(a[b:b + 1], o) for a, o in zip(first, alone)), b
    xa = x.clone().requires_grad_()         # the autograd path: the same towers, deterministic too
    outs = []
    for _ in range(2):
        xa.grad = None
        model(xa)[0].sum().backward()
        outs.append(xa.grad.clone())
    assert torch.equal(outs[0], outs[1])


def test_tie_case_is_deterministic_and_keeps_the_total(dev, fx, victim):
    """A cloud whose first 16 points are repeated at its end (across a forward-tile boundary): every arg-max has a tied
    twin. The lowest index wins, every run; the gradient sits on the first copy only."""
    _bitwise_only()
    model = victim()
    x = torch.from_numpy(fx["ties_b1_n144_x"]).to(dev)
    w = torch.from_numpy(fx["ties_b1_n144_w"]).to(dev)
    grads = []
    for _ in range(3):
        xa = x.clone().requires_grad_()
        (model(xa)[0] * w).sum().backward()
        grads.append(xa.grad)
    assert torch.equal(grads[0], grads[1]) and torch.equal(grads[0], grads[2])
    g = grads[0]
    assert float(g[:, :, :TIE].abs().max()) > 0 and float(g[:, :, -TIE:].abs().max()) == 0.0
    # the same cloud without the repeated tail routes the same channels to the same points: the totals agree to rounding
    xb = x[:, :, :-TIE].clone().requires_grad_()
    (model(xb)[0] * w).sum().backward()
    torch.testing.assert_close(g[:, :, :-TIE], xb.grad, rtol=1e-4, atol=1e-5 * float(g.abs().max()))


def _cw_mods():
    return (M("3dpointcloudattack_amd.attack.CW.CW_attack"), M("3dpointcloudattack_amd.attack.CW.CW_utils.adv_utils"),
            M("3dpointcloudattack_amd.attack.CW.CW_utils.dist_utils"), M("3dpointcloudattack_amd.attack.CW.CW_utils.clip_utils"))


@pytest.mark.parametrize("fused", [False, True])
def test_cw_attack_matches_the_reference_run(dev, fx, victim, fused):
    """The real reference's CW.attack on the feature-transform victim (B = 1, L2Dist, untargeted): the assertions of
    test_cw_attack_matches_reference_golden's L2 branch. The adversarial label is compared with the one the reference
    gave its own best attack (stored in the fixture)."""
    cwm, adv, dist, clip = _cw_mods()
    nm = "cw_l2_untarget"
    model, trans_model = victim(40, 0), victim(40, 1)
    steps, iters, kappa = fx[f"{nm}_cfg"]
    traj = []

    class Rec(torch.nn.Module):
        def __init__(self, inner):
            super().__init__()
            self.inner = inner

        def forward(self, a, o, w=None, batch_avg=True):
            traj.append(a.detach().cpu().numpy()[0].copy())
            return self.inner(a, o, w, batch_avg)

    atk = cwm.CW(model, trans_model, adv_func=adv.UntargetedLogitsAdvLoss(kappa), clip_func=clip.ClipPointsLinf(budget=0.18),
                 dist_func=Rec(dist.L2Dist()), attack_lr=1e-2, binary_step=int(steps), num_iter=int(iters),
                 attack_method="untarget", fused=fused)
    torch.manual_seed(1000)
    np.random.seed(1000)
    bd, ba, sn = atk.attack(torch.from_numpy(fx[f"{nm}_pc"]), torch.from_numpy(fx[f"{nm}_target"]))
    traj = np.stack(traj)
    ref_traj, ref_bd = fx[f"{nm}_traj"], fx[f"{nm}_bestdist"]
    assert ba.dtype == np.float64 and bd.dtype == np.float64 and ba.shape == fx[f"{nm}_bestattack"].shape
    np.testing.assert_array_equal(traj[0], ref_traj[0])      # same RNG stream, same start
    assert sn == int(fx[f"{nm}_success"])
    assert np.array_equal(bd < 1e9, ref_bd < 1e9)
    assert [atk.attack_fail, atk.shuffle_fail, atk.trans_fail] == fx[f"{nm}_fails"].tolist()
    dev_abs = np.abs(traj - ref_traj).reshape(len(traj), -1)
    print(f"fused={fused}: trajectory median {np.median(dev_abs):.3e}, first 15 within 1e-4 {(dev_abs[:15] <= 1e-4).mean():.4f}, "
          f"q99 {np.quantile(dev_abs, 0.99):.3e}, first two {dev_abs[:2].max():.3e}, bestdist {bd} vs {ref_bd}")
    assert np.median(dev_abs) < 1e-6
    assert (dev_abs[:15] <= 1e-4).mean() > 0.90
    assert np.quantile(dev_abs, 0.99) < 1e-2
    assert dev_abs[:2].max() < 1e-6
    np.testing.assert_allclose(bd, ref_bd, rtol=2e-2)
    with torch.no_grad():
        lab = model(torch.from_numpy(ba).float().transpose(1, 2).contiguous().to(dev))[0].argmax(1).cpu().numpy()
    assert np.array_equal(lab, fx[f"{nm}_advlabel"])


def test_cw_takes_the_fused_update_pass_and_graph_equals_eager(dev, victim, monkeypatch):
    """The 15-launch riders iteration is not built for this victim: CW._iterate must send it to _pass_fused_update. The
    captured iteration (hipGraph) reproduces the eager one bit for bit, also in a second attack on the same victim."""
    _bitwise_only()
    cwm, adv, dist, clip = _cw_mods()
    model, trans_model = victim(40, 0), victim(40, 1)
    assert not model.has_fused_attack_update
    with pytest.raises(NotImplementedError):
        model.fused_attack_update(clouds(1, 1, 64, dev), None, "untargeted_logits")
    taken = []
    real = cwm.CW._pass_fused_update
    monkeypatch.setattr(cwm.CW, "_pass_riders", lambda self, *a: pytest.fail("the riders pass was taken"))
    monkeypatch.setattr(cwm.CW, "_pass_fused_update", lambda self, *a: (taken.append(1), real(self, *a))[1])
    rng = np.random.default_rng(31)
    pcs = torch.from_numpy(np.stack([unit_cloud(rng, 200) for _ in range(3)]))
    with torch.no_grad():
        labels = model(pcs.transpose(1, 2).contiguous().to(dev))[0].argmax(1).cpu()
    outs = []
    for graph in (False, True, True):
        atk = cwm.CW(model, trans_model, adv_func=adv.UntargetedLogitsAdvLoss(5.), clip_func=clip.ClipPointsLinf(0.18),
                     dist_func=dist.ChamferDist(), binary_step=2, num_iter=8, graph=graph)
        assert atk._capturable() == graph
        torch.manual_seed(77)
        np.random.seed(77)
        outs.append(atk.attack(pcs, labels) + (atk.attack_fail, atk.shuffle_fail, atk.trans_fail))
    assert taken
    for o in outs[1:]:
        assert np.array_equal(outs[0][0], o[0]) and np.array_equal(outs[0][1], o[1]) and outs[0][2:] == o[2:]


def test_iso_fast_path_equals_generic_path(dev, victim):
    """A short CTRI loop of the isometry attack on the victim, from the matrices and with the settings of iso.npz's case
    a_n256: the fast path (fused_loss_and_grad) against the generic one (IsoTransform + autograd), inside the band_W that
    fixture carries for a PointNet victim (16x the reference's fp32-vs-float64 deviation), same stops and predictions."""
    iso = M("3dpointcloudattack_amd.attack.ISO.iso_attack")
    fi = np.load(os.path.join(GOLDEN, "iso.npz"))
    key = "a_n256"
    a = case_args(fi, key)
    model = victim()
    x = torch.from_numpy(fi[f"{key}_x"]).to(dev)
    W0 = torch.from_numpy(fi[f"{key}_tsi_W"]).float().to(dev)
    with torch.no_grad():
        label = model(ops.iso_apply(x, W0))[0].argmax(1)         # every cloud starts unbroken: the loop has work to do

    def loop(**kw):
        c = iso._ctri_loop(model, x, label, W0, None, int(a["target"]), int(a["kappa"]), a["step_size"], cache={}, **kw)
        c.run(4)
        return [t.clone() for t in (c.W, c.steps, c.kept_pred)]
    fast, gen = loop(), loop(fused=False)
    dW = float((gen[0] - fast[0]).abs().max())
    print(f"ISO fast vs generic: max |dW| {dW:.3e} (band_W {float(fi[f'{key}_band_W']):.3e}), steps {fast[1].tolist()}")
    assert int(fast[1].sum()) > 0 and float((fast[0] - W0).abs().max()) > 0
    assert dW <= float(fi[f"{key}_band_W"])
    assert torch.equal(gen[1], fast[1]) and torch.equal(gen[2], fast[2])


def test_siadv_fast_path_equals_generic_path(dev, victim):
    """Two single steps of SI-Adv's ifgm_ours with the victim as the surrogate, on siadv.npz's clouds and settings: the fast
    path (fused_attack_grad) against the generic one, inside the band_P that fixture carries for a PointNet surrogate."""
    si = M("3dpointcloudattack_amd.attack.SIadv.SIadv_attack")
    fs = np.load(os.path.join(GOLDEN, "siadv.npz"))
    eps, step_size, max_steps, top5 = fs["s5_args"]
    args = dict(eps=float(eps), step_size=float(step_size), max_steps=int(max_steps), num_class=40, top5_attack=bool(top5),
                defense_method=None, transfer_attack_method="ifgm_ours", query_attack_method=None)
    nets = victim(40, 0), victim(40, 1)
    points = torch.from_numpy(fs["points"]).to(dev)
    with torch.no_grad():
        target = nets[0](points[:, :, :3].transpose(1, 2).contiguous())[0].argmax(1)
    fast = si.PointCloudAttack(types.SimpleNamespace(**args), wb_classifier=nets[0], classifier=nets[1])
    generic = si.PointCloudAttack(types.SimpleNamespace(**args), wb_classifier=nets[0], classifier=nets[1], fused=False)
    assert fast._fast() and not generic._fast()
    band = float(fs["s5_band_P"])
    ori = points[:, :, :3].contiguous()
    p1 = fast.iterate(points, target, steps=1)
    d1 = float((p1 - generic.iterate(points, target, steps=1)).abs().max())
    # the second step teacher-forced, as test_loop_teacher_forced does: both paths start from the SAME iterate (normals are
    # now estimated, not given), so a neighbour-list tie that 1e-6 of difference would resolve differently cannot compound
    start = p1.transpose(1, 2).contiguous()
    p2 = fast.iterate(start, target, steps=1, ori=ori)
    d2 = float((p2 - generic.iterate(start, target, steps=1, ori=ori)).abs().max())
    print(f"SI-Adv fast vs generic: first step {d1:.3e}, second step (teacher-forced) {d2:.3e} (band_P {band:.3e})")
    assert float((p1 - ori.transpose(1, 2)).abs().max()) > 0 and float((p2 - p1).abs().max()) > 0
    assert d1 <= band and d2 <= band
