"""GPU: defense.FusedDefended — a PointNet victim behind SOR with the fused entry points of the device-side attack loops.
Victim level: exact against the hand composition (sor_select, the inner victim's fused call, sor_backward) and against
Defended; then the loops that reach the victim through those methods (CW, SI-Adv white-box, the additional-experiments CW,
kNN, AOF, CWTAOF, ISO, CWAdd)."""
import importlib
import os
import random
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from helpers import hip_pointnet, unit_cloud
from oracle import ref_torch as ort
from test_defense_cpu import SWEEP_BAND, RestatedSOR
from test_defense_gpu import CW_SEED, run_cw_defended

pytestmark = pytest.mark.gpu
M = importlib.import_module
ops = M("3dpointcloudattack_amd.ops")
dfn = M("3dpointcloudattack_amd.defense")
_lib = M("3dpointcloudattack_amd._lib")
graphed = M("3dpointcloudattack_amd.graphed")
pointnet = M("3dpointcloudattack_amd.model.pointnet")

KINDS = ("untargeted_logits", "logits", "cross_entropy")


def _bitwise_only():
    if os.environ.get("PC3D_DETERMINISTIC", "1") == "0":
        pytest.skip("asserts bit-equality: deterministic mode only (the victim's backward uses float atomics otherwise)")


def _victim(ft, dev, seed=0):
    if not ft:
        return hip_pointnet(seed, dev)[0]
    m = pointnet.PointNetCls(k=40, feature_transform=True)
    m.load_state_dict(ort.seeded_state_dict(m, seed))
    return m.eval().to(dev)


def _clouds(B, K, seed, dev):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(np.stack([unit_cloud(rng, K) for _ in range(B)])).transpose(1, 2).contiguous().to(dev)


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "feature_transform"])
def victim(request, dev):
    return _victim(request.param, dev)


def _hand(model, x, k, alpha, npoint, target, kind, kappa, which, **kw):
    sel = dfn.sor_select(x, k, alpha, npoint)
    if which == "attack":
        pred, loss, g = model.fused_attack_grad(sel["out"], target, kind, kappa, scale=1.0 / x.shape[0], **kw)
        return (pred, loss, dfn.sor_backward(g, sel["count"], sel["rank"])), sel
    logp, pred, loss, g = model.fused_loss_and_grad(sel["out"], target, kind, kappa, scale=1.0 / x.shape[0])
    return (logp, pred, loss, dfn.sor_backward(g, sel["count"], sel["rank"])), sel


@pytest.mark.parametrize("K,npoint", [(100, 100), (100, 1024), (256, 256), (256, 1024)])
def test_fused_calls_equal_the_hand_composition(dev, victim, K, npoint, monkeypatch):
    _bitwise_only()
    B = 3
    x = _clouds(B, K, 10 + K, dev)
    target = torch.tensor([3, 17, 39], device=dev)
    fd = dfn.FusedDefended(victim, dfn.SORDefense(2, 1.1, npoint))
    for kind in KINDS:
        got = fd.fused_attack_grad(x, target, kind, 0.5)
        want, sel = _hand(victim, x, 2, 1.1, npoint, target, kind, 0.5, "attack")
        assert got[2].shape == (B, 3, K)
        assert all(torch.equal(a, b) for a, b in zip(got, want)), kind
        dropped = (sel["rank"] < 0)[:, None, :].expand(B, 3, K)
        assert int(dropped.sum()) > 0 and bool((got[2][dropped] == 0).all())
        if kind == "cross_entropy":                                  # (the hinge losses are flat where they are satisfied)
            assert bool((got[2][~dropped] != 0).any())
        got = fd.fused_loss_and_grad(x, target, kind, 0.5)
        want, _ = _hand(victim, x, 2, 1.1, npoint, target, kind, 0.5, "loss")
        assert all(torch.equal(a, b) for a, b in zip(got, want)), kind
    # pred_out / step / scale are handed through
    pred_a, pred_b = torch.zeros(B, dtype=torch.long, device=dev), torch.zeros(B, dtype=torch.long, device=dev)
    step_a, step_b = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    got = fd.fused_attack_grad(x, target, "logits", 0.0, pred_out=pred_a, step=step_a, scale=0.25)
    sel = dfn.sor_select(x, 2, 1.1, npoint)
    p, l, g = victim.fused_attack_grad(sel["out"], target, "logits", 0.0, pred_out=pred_b, step=step_b, scale=0.25)
    assert torch.equal(got[2], dfn.sor_backward(g, sel["count"], sel["rank"])) and torch.equal(pred_a, pred_b)
    assert int(step_a) == int(step_b) == 1
    # fused_forward / fused_input_grad, as methods and through the module-level functions (what CWTAOF, CTA and GeoA3 call)
    logits, ctx = fd.fused_forward(x)
    il, ictx = pointnet.fused_forward(victim, sel["out"])
    assert torch.equal(logits, il)
    gl = torch.randn(logits.shape, device=dev, generator=torch.Generator(dev).manual_seed(1))
    want = dfn.sor_backward(pointnet.fused_input_grad(ictx, gl), sel["count"], sel["rank"])
    assert torch.equal(fd.fused_input_grad(ctx, gl), want)
    l2, c2 = pointnet.fused_forward(fd, x)
    out = torch.empty_like(x)
    assert torch.equal(l2, il) and pointnet.fused_input_grad(c2, gl, out=out) is out and torch.equal(out, want)
    assert pointnet.fused_forward(fd, x, tail=False)[0] is None
    assert pointnet.fused_pack(fd) is pointnet.fused_pack(victim)
    # both searches: the same bits
    for small in (False, True):
        monkeypatch.setattr(dfn, "SOR_SMALL_SEARCH", small)
        r = fd.fused_attack_grad(x, target, "untargeted_logits", 0.5)
        w, _ = _hand(victim, x, 2, 1.1, npoint, target, "untargeted_logits", 0.5, "attack")
        assert all(torch.equal(a, b) for a, b in zip(r, w)), small


@pytest.mark.parametrize("K,npoint", [(100, 1024), (256, 256)])
def test_forward_equals_defended_and_its_autograd_gradient(dev, victim, K, npoint, monkeypatch):
    _bitwise_only()
    x = _clouds(3, K, 20 + K, dev)
    head = dfn.SORDefense(2, 1.1, npoint)
    target = torch.tensor([1, 2, 3], device=dev)
    for small in (False, True):
        monkeypatch.setattr(dfn, "SOR_SMALL_SEARCH", small)
        fd = dfn.FusedDefended(victim, head)
        xa, xb = x.clone().requires_grad_(), x.clone().requires_grad_()
        a, b = fd(xa), dfn.Defended(victim, head, graph=False)(xb)
        assert len(a) == len(b) == 3 and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        ga, = torch.autograd.grad(a[0][torch.arange(3), target].sum(), xa)
        gb, = torch.autograd.grad(b[0][torch.arange(3), target].sum(), xb)
        assert torch.equal(ga, gb) and float(ga.abs().max()) > 0
        with torch.no_grad():
            assert torch.equal(graphed.wrap(fd)(x)[0], b[0].detach())          # replayed as a deterministic victim
        # the fused logits are the forward's logits before the log-softmax
        assert torch.equal(torch.log_softmax(fd.fused_forward(x)[0], dim=1).argmax(1), a[0].argmax(1))


def test_batch_independence_graph_replay_no_sync_and_launch_names(dev, victim, monkeypatch):
    _bitwise_only()
    B, K, npoint = 3, 256, 1024
    fd = dfn.FusedDefended(victim, dfn.SORDefense(2, 1.1, npoint))
    x = _clouds(B, K, 31, dev)
    target = torch.tensor([5, 6, 7], device=dev)
    full = fd.fused_attack_grad(x, target, "untargeted_logits", 0.0, scale=1.0)
    for i in range(B):
        one = fd.fused_attack_grad(x[i:i + 1].contiguous(), target[i:i + 1], "untargeted_logits", 0.0, scale=1.0)
        assert all(torch.equal(a[i:i + 1], b) for a, b in zip(full, one)), i
    # one call without a host sync
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        fd.fused_attack_grad(x, target, "untargeted_logits", 0.0, scale=1.0)
        fd.fused_loss_and_grad(x, target, "logits", 0.0)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    # launch names: the inner call's plus one search, one select, one backward
    names, real = [], _lib.call

    def counted(name, *a):
        names.append(name)
        return real(name, *a)
    sel = dfn.sor_select(x, 2, 1.1, npoint)
    for small, search in ((False, "pc3d_knn_hint_f32"), (True, "pc3d_knn_small_f32")):
        monkeypatch.setattr(dfn, "SOR_SMALL_SEARCH", small)
        monkeypatch.setattr(_lib, "call", counted)
        del names[:]
        victim.fused_attack_grad(sel["out"], target, "untargeted_logits", 0.0, scale=1.0)
        inner = list(names)
        del names[:]
        fd.fused_attack_grad(x, target, "untargeted_logits", 0.0, scale=1.0)
        monkeypatch.setattr(_lib, "call", real)
        assert len(inner) >= 10 and names == [search, "pc3d_sor_select_f32"] + inner + ["pc3d_sor_bwd_f32"], names
    # eager == a captured replay on fresh inputs
    sx, out = x.clone(), [None] * 3

    def body():
        out[:] = fd.fused_attack_grad(sx, target, "untargeted_logits", 0.0, scale=1.0)
    loop = graphed.LoopGraph(body, dev, 2, owners=(fd,))
    for xin in (x.flip(0).contiguous(), _clouds(B, K, 32, dev)):
        sx.copy_(xin)
        loop.replay()
        e = fd.fused_attack_grad(xin, target, "untargeted_logits", 0.0, scale=1.0)
        assert all(torch.equal(a, b) for a, b in zip(out, e))


def test_construction(dev):
    net, _ = hip_pointnet(0, dev)
    dg = M("3dpointcloudattack_amd.model.dgcnn")
    head = dfn.SORDefense(3, 1.05, 512)
    with pytest.raises(TypeError, match="PointNetCls"):
        dfn.FusedDefended(dg.DGCNN(types.SimpleNamespace(k=20, emb_dims=1024, dropout=0.5), output_channels=40), head)
    with pytest.raises(TypeError, match="SORDefense"):
        dfn.FusedDefended(net, dfn.SRSDefense(10))
    with pytest.raises(TypeError, match="PointNetCls"):
        dfn.FusedDefended(dfn.Defended(net, head), head)
    a, b = dfn.FusedDefended(net, head).to(dev), dfn.FusedDefended(graphed.GraphedVictim(net), head).to(dev)
    assert b.model is net and (a.k, a.alpha, a.npoint) == (3, 1.05, 512)
    head.k = 5                                                     # read once, at construction
    assert a.k == 3
    for name in ("k", "alpha", "npoint"):
        with pytest.raises(AttributeError):
            setattr(a, name, 1)
    assert graphed.weights_key(a) != graphed.weights_key(b)
    assert list(a.state_dict().keys()) == list(net.state_dict().keys())
    assert a.deterministic_forward and a.has_fused_attack_update is False and not hasattr(a, "fused_attack_update")
    assert hasattr(a, "_require_fused") and not a.training
    with pytest.raises(ValueError):
        a.fused_attack_grad(torch.zeros((1, 3, 600), device=dev), torch.zeros(1, dtype=torch.long, device=dev), "logits")  # K > npoint


# ---------------------------------------------------------------------------------------------------------------
# CW
# ---------------------------------------------------------------------------------------------------------------
def _run_cw_fused(dev, graph, seed):
    """run_cw_defended's attack (same clouds, labels, arguments, seeds) on FusedDefended with the fused loop."""
    cwm = M("3dpointcloudattack_amd.attack.CW.CW_attack")
    adv, dist, clip = (M("3dpointcloudattack_amd.attack.CW.CW_utils." + n) for n in ("adv_utils", "dist_utils", "clip_utils"))
    model, _ = hip_pointnet(0, dev)
    trans, _ = hip_pointnet(1, dev)
    B, K, steps, iters = 4, 256, 2, 15
    rng = np.random.default_rng(seed)
    pcs = torch.from_numpy(np.stack([unit_cloud(rng, K) for _ in range(B)]))
    with torch.no_grad():
        labels = dfn.Defended(model, RestatedSOR(2, 1.1, K))(pcs.transpose(1, 2).contiguous().to(dev))[0].argmax(1).cpu()
    vic = dfn.FusedDefended(model, dfn.SORDefense(2, 1.1, K))
    atk = cwm.CW(vic, trans, adv_func=adv.UntargetedLogitsAdvLoss(5.), clip_func=clip.ClipPointsLinf(0.18),
                 dist_func=dist.ChamferDist(), binary_step=steps, num_iter=iters, graph=graph)
    assert atk._capturable() == graph and graphed.unwrap(atk.model) is vic
    taken, real = [], atk._pass_fused_update
    atk._pass_fused_update = lambda *a: (taken.append(1), real(*a))[1]
    torch.manual_seed(11)
    np.random.seed(11)
    res = atk.attack(pcs, labels) + (atk.attack_fail, atk.shuffle_fail, atk.trans_fail)
    assert len(taken) >= 1 if graph else len(taken) == steps * iters
    return res


def test_cw_fused_loop_against_the_autograd_path(dev):
    seed = CW_SEED
    ref, ref_head = run_cw_defended(dev, "ref", seed)
    margin = float(ref_head.min_margin)
    print(f"smallest tie margin over the restatement's run: {margin:.3e} (band {SWEEP_BAND:.3e})")
    assert margin > SWEEP_BAND, f"an iterate has a point inside the tie band ({margin:.3e}): choose another seed"
    hip, _ = run_cw_defended(dev, "hip", seed)
    fused = _run_cw_fused(dev, True, seed)
    (bd, ba, sn), (rbd, rba, rsn) = fused[:3], hip[:3]
    ok = (bd < 1e9) & (rbd < 1e9)
    print("successful in both:", int(ok.sum()), "of", len(bd), "best distances", bd, rbd,
          "max cloud deviation", float(np.abs(ba - rba).max()))
    assert sn == rsn and np.array_equal(bd < 1e9, rbd < 1e9)
    np.testing.assert_allclose(bd[ok], rbd[ok], rtol=2e-3)
    np.testing.assert_allclose(ba, rba, atol=2e-4)
    assert fused[3:] == hip[3:]


def test_cw_graph_equals_eager(dev):
    _bitwise_only()
    a, b = _run_cw_fused(dev, True, CW_SEED), _run_cw_fused(dev, False, CW_SEED)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


# ---------------------------------------------------------------------------------------------------------------
# SI-Adv white-box
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def si_fx():
    return np.load(os.path.join(GOLDEN, "siadv.npz"))


@pytest.fixture(scope="module")
def si_nets(dev):
    out = []
    for seed in (3, 4):
        m = pointnet.PointNetCls(k=40)
        m.load_state_dict(ort.seeded_state_dict(m, seed))
        out.append(m.eval().to(dev))
    return out


def test_siadv_white_box_fast_path(dev, si_fx, si_nets):
    from test_siadv_gpu import make_attack
    points, target = torch.from_numpy(si_fx["points"]).to(dev), torch.from_numpy(si_fx["target"]).to(dev)
    fast = make_attack(si_fx, "s5", si_nets, wb=dfn.FusedDefended(si_nets[0], dfn.SORDefense(2, 1.1)))
    generic = make_attack(si_fx, "s5", si_nets, wb=dfn.Defended(si_nets[0], dfn.SORDefense(2, 1.1)))
    assert fast._fast() and not generic._fast()
    band = float(si_fx["s5_band_P"])
    iterates = [points[:, :, :3]]
    for steps in (1, 2):
        f, g = fast.iterate(points, target, steps=steps), generic.iterate(points, target, steps=steps)
        iterates.append(g.transpose(1, 2) if g.shape[1] == 3 else g)
        d = float((f - g).abs().max())
        print(f"fused vs generic defended white-box after {steps} step(s): {d:.3e} (band_P {band:.3e})")
        assert d <= band
    # the comparison means something only while no point of an iterate sits inside SOR's tie band
    margin = np.inf
    for P in iterates[:2]:
        r = dfn.sor_select(P.transpose(1, 2).contiguous(), 2, 1.1, 1024, want_stats=True)
        margin = min(margin, float(((r["v"] - r["thr"][:, None]).abs() / r["thr"][:, None]).min()))
    print(f"smallest tie margin over the iterates: {margin:.3e} (band {SWEEP_BAND:.3e})")
    assert margin > SWEEP_BAND


def test_siadv_replay_equals_eager(dev, si_fx, si_nets):
    _bitwise_only()
    from test_siadv_gpu import make_attack
    points, target = torch.from_numpy(si_fx["points"]).to(dev), torch.from_numpy(si_fx["target"]).to(dev)
    wb = dfn.FusedDefended(si_nets[0], dfn.SORDefense(2, 1.1))
    a = make_attack(si_fx, "s5", si_nets, wb=wb).iterate(points, target, steps=50)
    b = make_attack(si_fx, "s5", si_nets, wb=wb, graph=False).iterate(points, target, steps=50)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())


# ---------------------------------------------------------------------------------------------------------------
# the additional-experiments CW (EOT) and the kNN loop: B = 3, K = 192, 20 iterations
# ---------------------------------------------------------------------------------------------------------------
def _np_clouds(B, K, seed):
    rng = np.random.default_rng(seed)
    return np.stack([unit_cloud(rng, K) for _ in range(B)])


def _labels(vic, pcs, dev):
    with torch.no_grad():
        return vic(torch.from_numpy(pcs).transpose(1, 2).contiguous().to(dev))[0].argmax(1).cpu()


def test_eot_cw_device_loop(dev):
    _bitwise_only()
    cwm = M("3dpointcloudattack_amd.attack.additional_exp.CW_attack")
    adv, dist = (M("3dpointcloudattack_amd.attack.CW.CW_utils." + n) for n in ("adv_utils", "dist_utils"))
    net, _ = hip_pointnet(0, dev)
    vic = dfn.FusedDefended(net, dfn.SORDefense(2, 1.1, 192))
    pcs = _np_clouds(3, 192, 41)
    labels = _labels(vic, pcs, dev)
    res = []
    for graph in (True, False):
        atk = cwm.CW(vic, cwm.AdvLossAdapter(adv.LogitsAdvLoss(0.), adv.UntargetedLogitsAdvLoss(0.)),
                     cwm.PerSampleDist(dist.ChamferDist()), attack_lr=1e-2, binary_step=1, num_iter=20, whether_target=False,
                     whether_1d=True, whether_3Dtransform=True, graph=graph, device_loop=True)
        torch.manual_seed(5), np.random.seed(5), random.seed(5)     # the views are drawn from all three streams
        res.append(atk.attack(torch.from_numpy(pcs), torch.zeros(3), labels))
        assert atk.last_path == "device_loop"
    (bd, ba, sn), (bd2, ba2, sn2) = res
    assert np.array_equal(bd, bd2) and np.array_equal(ba, ba2) and sn == sn2
    assert np.isfinite(ba).all() and ba.shape == (3, 192, 3)
    found = bd < 1e9
    assert float(np.abs(ba[found] - pcs[found].astype(np.float64)).max(initial=0.0)) <= 0.4 + 1e-6       # the z box


def test_knn_device_loop(dev):
    _bitwise_only()
    knn = M("3dpointcloudattack_amd.attack.KNN.KNN_attack")
    adv, dist, clip = (M("3dpointcloudattack_amd.attack.CW.CW_utils." + n) for n in ("adv_utils", "dist_utils", "clip_utils"))
    net, _ = hip_pointnet(0, dev)
    vic = dfn.FusedDefended(net, dfn.SORDefense(2, 1.1, 192))
    pcs = _np_clouds(3, 192, 42)
    labels = _labels(vic, pcs, dev)
    res = []
    for graph in (True, False):
        atk = knn.CWKNN(vic, None, None, None, None, None, adv_func=adv.UntargetedLogitsAdvLoss(5.), dist_func=dist.ChamferkNNDist(),
                        clip_func=clip.ProjectInnerClipLinf(0.18), attack_lr=1e-2, num_iter=20, graph=graph, device_loop=True)
        torch.manual_seed(8), np.random.seed(8)
        res.append(atk.attack(torch.from_numpy(pcs), labels))
        assert atk.last_path == "device_loop"
    (out, sn), (out2, sn2) = res
    assert np.array_equal(out, out2) and sn == sn2
    assert np.isfinite(out).all() and float(np.abs(out - pcs).max()) <= 0.18 + float(np.spacing(np.float32(1.2)))


# ---------------------------------------------------------------------------------------------------------------
# smoke: the loops that only call fused_loss_and_grad / fused_attack_grad — 3 iterations, B = 2, K = 128
# ---------------------------------------------------------------------------------------------------------------
def _smoke_attack(name, vic, trans, graph):
    adv, dist, clip = (M("3dpointcloudattack_amd.attack.CW.CW_utils." + n) for n in ("adv_utils", "dist_utils", "clip_utils"))
    if name == "AOF":
        ea = M("3dpointcloudattack_amd.attack.AOF.Eval_AOF")
        atk = ea.AOF(vic, trans, adv.UntargetedLogitsAdvLoss(kappa=5.), clip.ClipPointsLinf(budget=0.18), lr=1e-2, low_pass=20,
                     step=1, epochs=3, batch_size=2, graph=graph)
        return atk, lambda pcs, lab: atk.attack(pcs, lab), atk._fused_kind() is not None
    if name == "CWTAOF":
        ta = M("3dpointcloudattack_amd.attack.AOF.TAOF_attack")
        atk = ta.CWTAOF(vic, adv.LogitsAdvLoss(0.), dist.L2Dist(), attack_lr=1e-2, binary_step=1, num_iter=3, low_pass=20,
                        clip_func=clip.ClipPointsLinf(0.18), graph=graph)
        return atk, lambda pcs, lab: atk.attack(pcs, (lab + 1) % 40, lab), atk._fused_kind() is not None
    if name == "ISOAttack":
        iso = M("3dpointcloudattack_amd.attack.ISO.iso_attack")
        atk = iso.ISOAttack(vic, num_steps=3, step_size=5e-3, num_init=2, a=-0.05, b=0.05, graph=graph)
        dev = next(vic.parameters()).device
        return atk, lambda pcs, lab: atk.attack(pcs.transpose(1, 2).contiguous().to(dev), lab.to(dev))[:2], True
    ia = M("3dpointcloudattack_amd.attack.Gen3DAdv.IndpAdd_attack")
    atk = ia.CWAdd(vic, trans, adv.UntargetedLogitsAdvLoss(30.), dist.ChamferDist('adv2ori'), num_add=16, binary_step=1,
                   num_iter=3, graph=graph)
    return atk, lambda pcs, lab: atk.attack(pcs, lab), atk._path(16) == "fast"


@pytest.mark.parametrize("name", ["AOF", "CWTAOF", "ISOAttack", "CWAdd"])
def test_smoke_loops_with_a_fused_defended_victim(dev, name):
    _bitwise_only()
    net, _ = hip_pointnet(0, dev)
    trans, _ = hip_pointnet(1, dev)
    K = 128
    vic = dfn.FusedDefended(net, dfn.SORDefense(2, 1.1, K + 16 if name == "CWAdd" else K))
    pcs = torch.from_numpy(_np_clouds(2, K, 51))
    with torch.no_grad():
        lab = net(pcs.transpose(1, 2).contiguous().to(dev))[0].argmax(1).cpu()
    res = []
    for graph in (True, False):
        atk, run, fast = _smoke_attack(name, vic, trans, graph)
        assert fast, "the loop did not take its fused path"
        torch.manual_seed(13), np.random.seed(13)
        out = run(pcs, lab)
        res.append([o.detach().cpu().numpy() if torch.is_tensor(o) else np.asarray(o) for o in out])
    for a, b in zip(*res):
        assert np.array_equal(a, b)
    clouds = res[0][1]
    assert np.isfinite(clouds.astype(np.float64)).all()
