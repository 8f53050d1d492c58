"""GPU: the isometry attack's kernels (csrc/iso.hip), ops.IsoTransform and attack/ISO's batched loop.

Bounds: u = 2^-24, gamma_k = k u / (1 - k u). A 3-term product sum in fp32 is within gamma_3 sum|w||x| of the exact one; a sum
of N products in ANY order within gamma_{N+2} sum|g x| (the kernels use fused multiply-adds: fewer roundings, same bound).
The loop is checked against the reference's recorded runs (tests/golden/iso.npz) with the bands the fixture's generator
measured, and against the plain-torch restatement of tests/test_iso_cpu.py on the same device."""
import copy
import importlib
import os
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from helpers import hip_pointnet, unit_cloud
from oracle import ref_torch as ort
from test_iso_cpu import RestatedISO, case_args, cases, check_against_reference, seeded_attack

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def gamma(k):
    return k * U / (1 - k * U)


def _iso():
    return importlib.import_module("3dpointcloudattack_amd.attack.ISO.iso_attack")


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "iso.npz"))


@pytest.fixture(scope="module")
def victim(dev, fx):
    m, sha = hip_pointnet(int(fx["weights_seed"]), dev)
    assert sha == str(fx["sha256"])
    return m


SHAPES = [(B, R, N) for B in (1, 3) for R in (1, 4) for N in (1, 63, 64, 65, 300)]


def _cloud(rng, B, N, cf, dev):
    """A [B,3,N] (cf) or [B,N,3] fp32 cloud as a NON-contiguous view of a wider buffer: the kernels read through strides."""
    buf = torch.from_numpy(rng.standard_normal((B, N + 3, 4)).astype(np.float32)).to(dev)
    v = buf[:, 1:N + 1, :3]
    return v.transpose(1, 2) if cf else v


# ---------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("cf", [True, False])
def test_apply_vs_float64(dev, ops, cf, transpose):
    rng = np.random.default_rng(11)
    for B, R, N in SHAPES:
        x = _cloud(rng, B, N, cf, dev)
        W = torch.from_numpy(rng.standard_normal((B * R, 3, 3)).astype(np.float32)).to(dev)
        out = ops.iso_apply(x, W, R=R, transpose=transpose, cf=cf)
        assert out.shape == ((B * R, 3, N) if cf else (B * R, N, 3))
        x64 = (x if cf else x.transpose(1, 2)).double().cpu().repeat_interleave(R, 0)           # [BR,3,N]
        W64 = W.double().cpu()
        W64 = W64.transpose(1, 2) if transpose else W64
        ref, mag = torch.matmul(W64, x64), torch.matmul(W64.abs(), x64.abs())
        got = (out if cf else out.transpose(1, 2)).double().cpu()
        assert ((got - ref).abs() <= gamma(3) * mag).all(), (B, R, N, float(((got - ref).abs() - gamma(3) * mag).max()))


@pytest.mark.parametrize("cf", [True, False])
def test_wgrad_bound_and_bit_identities(dev, ops, cf):
    rng = np.random.default_rng(12)
    for B, R, N in SHAPES:
        x = _cloud(rng, B, N, cf, dev)
        g = _cloud(rng, B * R, N, cf, dev)
        gW = ops.iso_wgrad(g, x, R=R, cf=cf)
        x64 = (x if cf else x.transpose(1, 2)).double().cpu().repeat_interleave(R, 0)
        g64 = (g if cf else g.transpose(1, 2)).double().cpu()
        ref, mag = torch.matmul(g64, x64.transpose(1, 2)), torch.matmul(g64.abs(), x64.abs().transpose(1, 2))
        err = (gW.double().cpu() - ref).abs()
        assert (err <= gamma(N + 2) * mag).all(), (B, R, N, float((err - gamma(N + 2) * mag).max()))
        assert torch.equal(gW, ops.iso_wgrad(g, x, R=R, cf=cf)), "run to run"
        if R > 1:                                    # R matrices in one call == R calls with one matrix per cloud
            gv = g.reshape(B, R, *g.shape[1:])
            for r in range(R):
                assert torch.equal(gW.view(B, R, 3, 3)[:, r], ops.iso_wgrad(gv[:, r], x, R=1, cf=cf)), (B, R, N, r)


def _state(B, ncls, dev):
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)        # noqa: E731
    return dict(m=z(B, 3, 3), v=z(B, 3, 3), done=z(B, dt=torch.int32), steps=z(B, dt=torch.int32), kept_out=z(B, ncls),
                kept_pred=z(B, dt=torch.int64))


def _update(ops, x, xo, W, st, pred, label, row, lr, **kw):
    return ops.iso_update(x, xo, W, st["m"], st["v"], pred, label, row, st["done"], st["steps"], st["kept_out"],
                          st["kept_pred"], lr, **kw)


@pytest.mark.parametrize("N", [1, 65, 300, 1024])
def test_update_fused_wgrad_equals_standalone(dev, ops, N):
    """The launch that reduces g x^T itself leaves the bits of the launch that is handed pc3d_iso_wgrad_f32's result."""
    rng = np.random.default_rng(13 + N)
    B, ncls = 3, 7
    x, g = _cloud(rng, B, N, True, dev), _cloud(rng, B, N, True, dev)
    label = torch.arange(B, device=dev)
    row = torch.randn(B, ncls, device=dev)
    res = []
    for fused in (True, False):
        W = torch.eye(3, device=dev).repeat(B, 1, 1) + 0.01
        st, xo = _state(B, ncls, dev), torch.empty(B, 3, N, device=dev)
        kw = dict(g=g) if fused else dict(gW=ops.iso_wgrad(g, x))
        for _ in range(2):
            _update(ops, x, xo, W, st, label.clone(), label, row, 1e-2, **kw)
        res.append((W, st["m"], st["v"], xo))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert not torch.equal(res[0][0], torch.eye(3, device=dev).repeat(B, 1, 1) + 0.01)


def test_update_adam_three_steps_vs_torch(dev, ops):
    """|dW| <= 2^-22 against torch.optim.Adam on the CPU in fp32 after three steps: one rounding of W per step at |W| < 2
    (2^-24 each), with room for the update's own rounding (lr * 1e-7, of order 1e-10)."""
    rng = np.random.default_rng(14)
    B, N, ncls, lr = 4, 5, 3, 5e-3
    gs = rng.uniform(1e-3, 1.0, (3, B, 3, 3)).astype(np.float32) * rng.choice([-1.0, 1.0], (3, B, 3, 3)).astype(np.float32)
    W0 = (np.eye(3, dtype=np.float32) + 0.1 * rng.standard_normal((B, 3, 3)).astype(np.float32))
    p = torch.nn.Parameter(torch.from_numpy(W0.copy()))
    opt = torch.optim.Adam([p], lr=lr, betas=(0.9, 0.999))
    x = _cloud(rng, B, N, True, dev)
    W, st, xo = torch.from_numpy(W0.copy()).to(dev), _state(B, ncls, dev), torch.empty(B, 3, N, device=dev)
    label, row = torch.zeros(B, dtype=torch.int64, device=dev), torch.zeros(B, ncls, device=dev)
    for s in range(3):
        opt.zero_grad()
        p.grad = torch.from_numpy(gs[s].copy())
        opt.step()
        _update(ops, x, xo, W, st, label.clone(), label, row, lr, gW=torch.from_numpy(gs[s]).to(dev))
    err = float((W.cpu() - p.detach()).abs().max())
    print(f"adam: max |dW| after 3 steps {err:.3e} (bound {2.0 ** -22:.3e})")
    assert float(p.detach().abs().max()) < 2 and err <= 2.0 ** -22
    assert st["steps"].tolist() == [3] * B


def test_update_latch_record_and_epilogue(dev, ops):
    """Scripted predictions: cloud 0 is wrong at step 2 and stops there, cloud 1 never stops."""
    rng = np.random.default_rng(15)
    B, N, ncls = 2, 130, 5
    x = _cloud(rng, B, N, False, dev)                                   # channels-last in, channels-first out
    label = torch.tensor([1, 3], device=dev)
    preds = [[1, 3], [4, 3], [1, 3], [1, 3]]                            # cloud 0 "recovers" at step 3: a latch ignores that
    W = torch.eye(3, device=dev).repeat(B, 1, 1)
    st, xo = _state(B, ncls, dev), torch.empty(B, 3, N, device=dev)
    rows, frozen = [], None
    for s, pr in enumerate(preds, 1):
        g, row = _cloud(rng, B, N, False, dev), torch.randn(B, ncls, device=dev)
        rows.append(row)
        before = W.clone()
        _update(ops, x, xo.transpose(1, 2), W, st, torch.tensor(pr, device=dev), label, row, 1e-2, g=g, cf=False)
        assert torch.equal(xo, ops.iso_apply(x.transpose(1, 2), W)), "the epilogue's x' is iso_apply(W), bit for bit"
        assert not torch.equal(W[1], before[1])
        if s == 1:
            assert not torch.equal(W[0], before[0])
        if s == 2:
            assert torch.equal(W[0], before[0]), "the breaking evaluation takes no update"
            frozen = (W[0].clone(), st["m"][0].clone(), st["v"][0].clone())
        if s >= 2:
            assert st["done"].tolist() == [1, 0] and st["steps"].tolist() == [2, s]
            assert torch.equal(st["kept_out"][0], rows[1][0]) and torch.equal(st["kept_out"][1], row[1])
            assert st["kept_pred"].tolist() == [4, 3]
            for a, b in zip(frozen, (W[0], st["m"][0], st["v"][0])):
                assert torch.equal(a, b)


@pytest.mark.parametrize("R", [1, 2])
def test_isotransform_gradients(dev, ops, R):
    rng = np.random.default_rng(16)
    for B, N in ((1, 1), (3, 65), (2, 300)):
        x = _cloud(rng, B, N, True, dev).contiguous().requires_grad_()
        W = torch.from_numpy(rng.standard_normal((B * R, 3, 3)).astype(np.float32)).to(dev).requires_grad_()
        G = torch.from_numpy(rng.standard_normal((B * R, 3, N)).astype(np.float32)).to(dev)
        (ops.IsoTransform.apply(x, W) * G).sum().backward()
        x64, W64, G64 = x.detach().double().cpu().requires_grad_(), W.detach().double().cpu().requires_grad_(), G.double().cpu()
        (torch.matmul(W64, x64.repeat_interleave(R, 0)) * G64).sum().backward()
        xr = x64.detach().repeat_interleave(R, 0)
        mag_W = torch.matmul(G64.abs(), xr.abs().transpose(1, 2))
        assert ((W.grad.double().cpu() - W64.grad).abs() <= gamma(N + 2) * mag_W).all()
        # gx[b] = sum_r W_r^T G_r: gamma_3 per product sum, and R - 1 more additions
        mag_x = torch.matmul(W64.detach().abs().transpose(1, 2), G64.abs()).view(B, R, 3, N).sum(1)
        assert ((x.grad.double().cpu() - x64.grad).abs() <= gamma(3 + R - 1) * mag_x).all()


# ---------------------------------------------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------------------------------------------
def _run(fx, key, victim, dev, **kw):
    atk, a = seeded_attack(_iso().ISOAttack, victim, fx, key, **kw)
    adv, W, info = atk.attack(torch.from_numpy(fx[f"{key}_x"]).to(dev), torch.from_numpy(fx[f"{key}_label"]).to(dev))
    return atk, adv, W, info


@pytest.mark.parametrize("key", cases())
def test_loop_against_reference(dev, fx, victim, key):
    atk, adv, W, info = _run(fx, key, victim, dev, tsi_batch=1)
    assert np.array_equal(info["tsi_W"].double().numpy(), fx[f"{key}_tsi_W"]), "the matrices TSI hands on"
    check_against_reference(fx, key, W, info, atk.thompson)
    assert torch.equal(adv, importlib.import_module("3dpointcloudattack_amd.ops").iso_apply(
        torch.from_numpy(fx[f"{key}_x"]).to(dev), W))


def _same(a, b):
    (adv_a, W_a, i_a), (adv_b, W_b, i_b) = a, b
    assert torch.equal(adv_a, adv_b) and torch.equal(W_a, W_b)
    for k in i_a:
        assert torch.equal(torch.as_tensor(i_a[k]), torch.as_tensor(i_b[k])), k


@pytest.mark.parametrize("key", ["a_n64", "d_n64", "a_n256"])
def test_run_equals_run_and_graph_equals_eager(dev, fx, victim, key):
    runs = [_run(fx, key, victim, dev, graph=g)[1:] for g in (True, True, False)]
    _same(runs[0], runs[1])
    _same(runs[0], runs[2])
    assert int(runs[0][2]["steps"].sum()) > 0


def test_cloud_in_batch_equals_cloud_alone_and_paths_agree(dev, fx, victim):
    """The CTRI loop from the matrices the reference's TSI handed on: every cloud alone == the cloud in the batch, bit for
    bit; a batch in which a cloud is latched from the start leaves the others' bits alone; and the generic path
    (IsoTransform + autograd + iso_update with gW) lands within band_W of the fast path."""
    key = "a_n256"
    a = case_args(fx, key)
    x, label = torch.from_numpy(fx[f"{key}_x"]).to(dev), torch.from_numpy(fx[f"{key}_label"]).to(dev)
    W0 = torch.from_numpy(fx[f"{key}_tsi_W"]).float().to(dev)

    def loop(xs, ls, Ws, active=None, **kw):
        c = _iso()._ctri_loop(victim, xs, ls, Ws, active, a["target"], a["kappa"], a["step_size"], cache={}, **kw)
        c.run(a["num_steps"])
        return [t.clone() for t in (c.W, c.steps, c.kept_out, c.kept_pred, c.done)]
    fast = loop(x, label, W0)
    for b in range(x.shape[0]):
        one = loop(x[b:b + 1], label[b:b + 1], W0[b:b + 1])
        for t_all, t_one in zip(fast, one):
            assert torch.equal(t_all[b:b + 1], t_one), b
    active = torch.tensor([True, False, True, True, False, True], device=dev)
    part = loop(x, label, W0, active)
    for t_all, t_part in zip(fast[:4], part[:4]):
        assert torch.equal(t_all[active], t_part[active])
    assert torch.equal(part[0][~active], W0[~active]) and part[1][~active].tolist() == [0, 0]
    gen = loop(x, label, W0, fused=False)
    dW = float((gen[0] - fast[0]).abs().max())
    print(f"fast vs generic: max |dW| {dW:.3e} (band_W {float(fx[f'{key}_band_W']):.3e})")
    assert dW <= float(fx[f"{key}_band_W"])
    assert torch.equal(gen[1], fast[1]) and torch.equal(gen[3], fast[3])


def test_fast_step_is_one_launch_more_than_the_victim(dev, fx, victim, monkeypatch):
    """A fast-path CTRI step = the launches of fused_loss_and_grad + exactly one, pc3d_iso_update_f32."""
    _lib = importlib.import_module("3dpointcloudattack_amd._lib")
    names, real = [], _lib.call

    def counted(name, *a):
        names.append(name)
        return real(name, *a)
    key = "a_n64"
    x, label = torch.from_numpy(fx[f"{key}_x"]).to(dev), torch.from_numpy(fx[f"{key}_label"]).to(dev)
    c = _iso()._ctri_loop(victim, x, label, torch.eye(3, device=dev).repeat(x.shape[0], 1, 1), None, 1, 0, 5e-3, graph=False)
    c.step()                                              # folded-weight caches are built here, outside the count
    monkeypatch.setattr(_lib, "call", counted)
    victim.fused_loss_and_grad(c.xo, label, 0, 0.0, scale=1.0)
    n_victim = len(names)
    del names[:]
    c.step()
    assert n_victim >= 10 and len(names) == n_victim + 1, (n_victim, names)
    assert names.count("pc3d_iso_update_f32") == 1 and names[-1] == "pc3d_iso_update_f32"
    print(f"launches: victim forward+backward {n_victim}, CTRI step {len(names)}")


# ---------------------------------------------------------------------------------------------------------------
# the reference-named entry points, driven cloud by cloud as the reference's __main__ drives its own
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["e_n64", "d_n64"])
def test_dropin_functions_cloud_by_cloud(dev, fx, victim, key):
    """ISOnet, logits_info, thompson_sample_attack and gradient_attack in the reference's order, against the recorded run:
    discrete outcomes, draws and posterior exact, W within band_W, probabilities within band_gap, penalties of the
    clouds CTRI fooled within the corner bound, both generators' next draws."""
    from test_iso_cpu import penalty_tols
    iso = _iso()
    ts = importlib.import_module("3dpointcloudattack_amd.attack.ISO.thompson_sample")
    a = case_args(fx, key)
    args = types.SimpleNamespace(**a)
    g = lambda n: fx[f"{key}_{n}"]          # noqa: E731
    model_v = iso.ISOnet(model=victim).to(dev)          # built once, before the seeds: its init draws from torch's generator
    model_v.eval()
    seed = int(g("seed"))
    np.random.seed(seed), torch.manual_seed(seed)
    thompson = ts.BernThompson(ts.environment(d=a["d"], a0=a["a"], b0=a["b"]))
    band_W, band_gap, tols = float(g("band_W")), float(g("band_gap")), penalty_tols(fx, key)
    drawn = 0
    for i in range(g("x").shape[0]):
        obj, lab = torch.from_numpy(g("x")[i:i + 1]).to(dev), torch.from_numpy(g("label")[i:i + 1]).to(dev)
        _, correct, rates, indices = iso.logits_info(obj, lab, victim)
        assert bool(correct) == bool(g("attacked")[i])
        assert abs(float(rates[(indices == lab.item()).nonzero().item()]) - g("true_prob_before")[i]) <= band_gap
        if correct == 0:
            continue
        W_tsi, thompson = iso.thompson_sample_attack(thompson, obj, lab, model_v, a["num_init"])
        drawn += int(g("tsi_draws")[i])
        assert np.array_equal(W_tsi.cpu().double().numpy(), g("tsi_W")[i])
        last = torch.as_tensor(g("tsi_all")[drawn - 1], dtype=torch.float32)
        assert torch.equal(model_v.iso.weight.data.cpu(), last), "iso.weight is left at the LAST drawn matrix"
        model_v.iso.weight.data = W_tsi
        _, correct, rates, indices = iso.logits_info(obj, lab, model_v)
        assert (correct == 0) == bool(g("init_success")[i])
        penalty, steps = 0.0, 0
        if correct == 1:
            correct, rates, indices, model_v, penalty, steps = iso.gradient_attack(obj, lab, model_v, args)
            if correct == 1:
                penalty = 0.0
        assert (correct, steps, int(indices[0])) == (int(g("correct")[i]), int(g("steps")[i]), int(g("indices2")[i, 0])), i
        assert float((model_v.iso.weight.data.cpu().double() - torch.from_numpy(g("W")[i]).double()).abs().max()) <= band_W
        assert float((rates[:2].cpu() - torch.from_numpy(g("rates2")[i])).abs().max()) <= band_gap
        assert abs(penalty - float(g("penalty")[i])) <= tols[i], (i, penalty, g("penalty")[i], tols[i])
    assert np.array_equal(thompson.alpha, g("alpha")) and np.array_equal(thompson.beta, g("beta"))
    assert np.random.uniform() == float(g("next_np")) and float(torch.rand(1).double()[0]) == float(g("next_torch"))


def test_isonet_forward_and_reward_matrix(dev, fx, victim):
    """ISOnet.forward with one [3,3] matrix and with one matrix per sample equals the victim on iso_apply's output, bit for
    bit, and differentiates to iso.weight; the bandit's get_reward_matrix sets the matrix, evaluates and updates."""
    iso = _iso()
    ts = importlib.import_module("3dpointcloudattack_amd.attack.ISO.thompson_sample")
    ops = importlib.import_module("3dpointcloudattack_amd.ops")
    key = "c_n64"
    x, label = torch.from_numpy(fx[f"{key}_x"]).to(dev), torch.from_numpy(fx[f"{key}_label"]).to(dev)
    B = x.shape[0]
    net = iso.ISOnet(victim).to(dev).eval()
    W1 = torch.from_numpy(fx[f"{key}_tsi_W"][0]).float().to(dev)
    net.iso.weight.data = W1
    with torch.no_grad():
        assert torch.equal(net(x)[0], victim(ops.iso_apply(x, W1.expand(B, 3, 3).contiguous()))[0])
    WB = torch.from_numpy(fx[f"{key}_tsi_W"]).float().to(dev)
    net.iso.weight = torch.nn.Parameter(WB.clone())
    out = net(x)[0]
    with torch.no_grad():
        assert torch.equal(out.detach(), victim(ops.iso_apply(x, WB))[0])
    out.gather(1, label[:, None]).sum().backward()
    assert net.iso.weight.grad.shape == (B, 3, 3) and bool(torch.isfinite(net.iso.weight.grad).all())
    assert float(net.iso.weight.grad.abs().amax((1, 2)).min()) > 0
    state = np.random.get_state()
    try:
        np.random.seed(3)
        th = ts.BernThompson(ts.environment(d=4, a0=-np.pi, b0=np.pi))
        arm = th.get_action()
        net1 = iso.ISOnet(victim).to(dev).eval()
        reward, matrix = th.get_reward_matrix(arm, x[:1], label[:1], net1)
        assert torch.equal(net1.iso.weight.data.cpu(), torch.as_tensor(matrix, dtype=torch.float32))
        _, correct, _, _ = ts.logits_info(x[:1], label[:1], net1)
        assert reward == 1 - correct and th.alpha[arm] == 1 + reward and th.beta[arm] == 2 - reward
        assert th.alpha.sum() + th.beta.sum() == 2 * 64 + 1
    finally:
        np.random.set_state(state)


def test_batched_tsi_against_restatement(dev, fx, victim):
    """tsi_batch = B is a generalisation the reference does not have: the product against the restatement, same setting, same
    device. Discrete outcomes exact, W within the case's band."""
    key = "e_n64"
    B = fx[f"{key}_x"].shape[0]
    x, label = torch.from_numpy(fx[f"{key}_x"]).to(dev), torch.from_numpy(fx[f"{key}_label"]).to(dev)
    atk, _ = seeded_attack(_iso().ISOAttack, victim, fx, key, tsi_batch=B)
    _, W, info = atk.attack(x, label)
    nxt = (np.random.uniform(), float(torch.rand(1)))
    ref, _ = seeded_attack(RestatedISO, victim, fx, key, tsi_batch=B)
    _, Wr, iref = ref.attack(x, label)
    assert nxt == (np.random.uniform(), float(torch.rand(1))), "both generators end in the same state"
    for k in ("attacked", "init_success", "tsi_draws", "steps", "correct", "pred_after"):
        assert np.array_equal(np.asarray(info[k]).astype(np.int64), np.asarray(iref[k]).astype(np.int64)), k
    assert np.array_equal(atk.thompson.alpha, ref.thompson.alpha) and np.array_equal(atk.thompson.beta, ref.thompson.beta)
    assert np.array_equal(info["tsi_W"].numpy(), iref["tsi_W"])
    dW = float((W - Wr).abs().max())
    print(f"tsi_batch={B}: max |dW| {dW:.3e} (band_W {float(fx[f'{key}_band_W']):.3e})")
    assert dW <= float(fx[f"{key}_band_W"]) and min(ref.gaps) > float(fx[f"{key}_band_gap"])


def test_dgcnn_generic_path_against_restatement(dev):
    """A victim without fused_loss_and_grad: DGCNN (N = 128, k = 4) through IsoTransform + autograd + iso_update(gW), against
    the restatement driving the SAME victim on the same device. The band follows the fixture generator's rule for this
    run: 16x the deviation between the restatement in fp32 and in float64 on the oracle's DGCNN with the same weights
    (CPU), and the run is only meaningful if every evaluation's top-1/top-2 gap lies outside it."""
    dg = importlib.import_module("3dpointcloudattack_amd.model.dgcnn")
    cfg = types.SimpleNamespace(k=4, emb_dims=1024, dropout=0.5)
    m = dg.DGCNN(cfg, 40)
    sd = ort.seeded_state_dict(m, 21)
    m.load_state_dict(sd)
    m = m.eval().to(dev)
    rng = np.random.default_rng(2102)
    B, N = 2, 128
    x = torch.from_numpy(np.stack([unit_cloud(rng, N) for _ in range(B)]).transpose(0, 2, 1).copy())
    kw = dict(num_steps=4, step_size=5e-3, num_init=2, a=-0.05, b=0.05)
    om = ort.DGCNN(cfg, 40)
    om.load_state_dict(sd)
    om.eval()
    for p in om.parameters():
        p.requires_grad_(False)
    with torch.no_grad():
        label = m(x.to(dev))[0].argmax(1)
    assert torch.equal(label.cpu(), om(x)[0].argmax(1))
    outs = []
    for model, xx in ((om, x), (copy.deepcopy(om).double(), x.double())):
        np.random.seed(7), torch.manual_seed(7)
        r = RestatedISO(model, **kw)
        outs.append((r.attack(xx, label.cpu())[1], r.gaps))
    band_W = 16.0 * max(float((outs[0][0].double() - outs[1][0]).abs().max()), U)
    band_gap = 16.0 * max(abs(p - q) for p, q in zip(outs[0][1], outs[1][1]))
    np.random.seed(7), torch.manual_seed(7)
    ref = RestatedISO(m, **kw)
    _, Wr, iref = ref.attack(x.to(dev), label)
    np.random.seed(7), torch.manual_seed(7)
    atk = _iso().ISOAttack(m, **kw)
    _, W, info = atk.attack(x.to(dev), label)
    dW = float((W - Wr).abs().max())
    print(f"dgcnn: max |dW| {dW:.3e} band_W {band_W:.3e}; smallest gap {min(ref.gaps):.3e} band_gap {band_gap:.3e}; "
          f"steps {iref['steps'].tolist()}")
    assert min(ref.gaps) > band_gap
    for k in ("attacked", "init_success", "tsi_draws", "steps", "correct", "pred_after"):
        assert np.array_equal(np.asarray(info[k]).astype(np.int64), np.asarray(iref[k]).astype(np.int64)), k
    assert int(iref["steps"].sum()) > 0 and dW <= band_W
