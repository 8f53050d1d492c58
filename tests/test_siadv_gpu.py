"""GPU: the shape-invariant attack's kernels (pc3d_pca_normal_f32, pc3d_si_frame_f32, pc3d_si_step_f32) against float64
restatements of the literal formulas, and the loop (attack/SIadv/SIadv_attack.py) against tests/golden/siadv.npz — the
real reference's shape_invariant_ifgm run on the CPU with a stand-in for open3d (tests/golden/make_golden_siadv.py).

Bounds: a kernel is held to 16x the fp32-vs-float64 deviation of the restatement on the very input; the loop to the
bands stored with the fixture (16x the deviation of the reference's own fp32 run from its float64 run).
"""
import importlib
import os
import types

import numpy as np
import pytest
import torch

import siadv_restatement as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

M = importlib.import_module
AXES = np.array([1.0, 0.7, 0.5])
SHAPES = [(1, 20), (3, 20), (1, 65), (3, 65), (1, 256), (3, 256), (1, 257), (3, 257), (1, 1024), (3, 1024)]
EPS, STEP = 0.16, 0.07


def ellipsoid(B, N, seed):
    """(points, unit normals) [B,N,3] float32 on the ellipsoid with axes 1, 0.7, 0.5; the first 8 points of every cloud sit
    where the normal is (0,0,+-1) and just inside / outside |n_z^2 - 1| = 1e-4 (the rows get_spin_axis_matrix rewrites)."""
    rng = np.random.default_rng(seed)
    zs = []
    for s in (1.0, -1.0):
        zs += [(0.0, s), (0.3, s * np.sqrt(1 - 0.9e-4)), (1.1, s * np.sqrt(1 - 1.1e-4))]
    zs += [(2.0, np.sqrt(1 - 0.99e-4)), (4.0, -np.sqrt(1 - 1.01e-4))]
    P, Nn = np.zeros((B, N, 3)), np.zeros((B, N, 3))
    for b in range(B):
        d = rng.standard_normal((N, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        p = d * AXES
        n = p / AXES ** 2
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        for j, (az, nz) in enumerate(zs):
            r = np.sqrt(max(0.0, 1 - nz * nz))
            nj = np.array([r * np.cos(az + b), r * np.sin(az + b), nz])
            p[j], n[j] = AXES ** 2 * nj / np.sqrt((AXES ** 2 * nj * nj).sum()), nj
        P[b], Nn[b] = p, n
    n32 = Nn.astype(np.float32)
    n32 /= np.sqrt((n32.astype(np.float64) ** 2).sum(-1, keepdims=True)).astype(np.float32)
    return torch.from_numpy(P.astype(np.float32)), torch.from_numpy(n32)


def lay(t, cf, dev):
    """[B,N,3] host tensor -> the device tensor in the layout under test."""
    t = t.to(dev)
    return t.transpose(1, 2).contiguous() if cf else t.contiguous()


def unlay(t, cf):
    return (t.transpose(1, 2) if cf else t).contiguous().cpu()


def eigh_normals(P, idx):
    """float64 `eigh` on the same lists: (smallest eigenvector [B,N,3], eigenvalues [B,N,3] ascending)."""
    P = P.double()
    B, N, K = idx.shape
    nb = torch.gather(P[:, None].expand(B, N, N, 3), 2, idx.long()[..., None].expand(B, N, K, 3))
    d = nb - nb.mean(2, keepdim=True)
    w, v = torch.linalg.eigh(d.transpose(2, 3) @ d / K)
    return v[..., 0], w


# ------------------------------------------------------------------------------------------------------
# pc3d_pca_normal_f32
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cf", [False, True], ids=["cl", "cf"])
@pytest.mark.parametrize("B,N", SHAPES)
def test_pca_normal_vs_eigh(ops, dev, B, N, cf):
    P, _ = ellipsoid(B, N, 100 + N)
    x = lay(P, cf, dev)
    _, idx = ops.knn_raw(x, x, 20, q_cf=cf, r_cf=cf)
    n = ops.pca_normal(x, idx, cf=cf)
    assert n.shape == x.shape
    assert torch.equal(n, ops.pca_normal(x, idx, cf=cf))                 # bit-identical run to run
    n = unlay(n, cf).double()
    assert float((n.norm(dim=-1) - 1).abs().max()) < 1e-6
    assert bool((n[..., 2] >= 0).all())                                  # the sign rule: the hemisphere z >= 0
    ref, w = eigh_normals(P, idx.cpu())
    ok = (w[..., 1] - w[..., 0]) > 1e-3 * w[..., 2]                      # test_estimate_normal_closed_form_vs_eigh's criterion
    excluded = 1.0 - float(ok.double().mean())
    cos = (n * ref).sum(-1).abs()
    print(f"B={B} N={N}: excluded {excluded:.4f}, smallest ratio {float(((w[..., 1] - w[..., 0]) / w[..., 2]).min()):.3f}, "
          f"1 - min|cos| {float(1 - cos[ok].min()):.3e}")
    assert excluded <= 0.01
    assert bool((cos[ok] > 1 - 1e-4).all())


def test_pca_normal_degenerate_and_bad_index(ops, dev):
    P, _ = ellipsoid(2, 65, 7)
    x = P.to(dev)
    _, idx = ops.knn_raw(x, x, 20)
    two = ops.pca_normal(x, idx[:, :, :2].contiguous())                  # K = 2 < 3: open3d's default normal
    assert torch.equal(two, torch.tensor([0.0, 0.0, 1.0], device=dev).expand(2, 65, 3))
    same = torch.zeros((1, 20, 3), device=dev) + 0.25                    # zero covariance
    lists = torch.arange(20, dtype=torch.int32, device=dev).expand(1, 20, 20).contiguous()
    assert torch.equal(ops.pca_normal(same, lists), torch.tensor([0.0, 0.0, 1.0], device=dev).expand(1, 20, 3))
    good = ops.pca_normal(x, idx)
    bad = idx.clone()
    bad[0, 3, 5], bad[1, 64, 19], bad[1, 10, 0] = 65, -1, 2 ** 30
    out = ops.pca_normal(x, bad)
    torch.cuda.synchronize()
    hit = torch.zeros((2, 65), dtype=torch.bool, device=dev)
    hit[0, 3] = hit[1, 64] = hit[1, 10] = True
    assert bool(torch.isnan(out[hit]).all())
    assert torch.equal(out[~hit], good[~hit])                            # ... at that point only
    with pytest.raises(Exception):
        ops.pca_normal(x, idx.long())


# ------------------------------------------------------------------------------------------------------
# pc3d_si_frame_f32 / pc3d_si_step_f32 against the float64 restatement of the literal formulas
# ------------------------------------------------------------------------------------------------------
def step_inputs(B, N, seed):
    """P, ori, g, n [B,N,3] float32 (host). With B = 3: cloud 1 has g = 0, cloud 2 sits at the clip already."""
    ori, n = ellipsoid(B, N, seed)
    gen = torch.Generator().manual_seed(seed)
    P = ori + 0.05 * (2 * torch.rand(ori.shape, generator=gen) - 1)
    g = torch.randn(ori.shape, generator=gen) * torch.rand((B, N, 1), generator=gen) ** 4     # a few points dominate
    if B >= 3:
        g[1] = 0.0
        P[2] = ori[2] + EPS * torch.where(torch.rand(ori[2].shape, generator=gen) < 0.5, -1.0, 1.0)
    return P, ori, g, n


def bound_of(f32, f64):
    return 16.0 * max(float((f32.double() - f64).abs().max()), 2.0 ** -24)


@pytest.mark.parametrize("cf", [False, True], ids=["cl", "cf"])
@pytest.mark.parametrize("B,N", SHAPES)
def test_si_step_vs_float64_restatement(ops, dev, B, N, cf):
    P, ori, g, n = step_inputs(B, N, 200 + N)
    ref64 = R.si_step(P.double(), ori.double(), g.double(), n.double(), STEP, EPS)
    ref32 = R.si_step(P, ori, g, n, STEP, EPS)
    bound = bound_of(ref32, ref64)
    x = lay(P, cf, dev)
    nout = torch.empty_like(x)
    ret = ops.si_step(x, lay(ori, cf, dev), lay(g, cf, dev), STEP, EPS, nrm=lay(n, cf, dev), nrm_out=nout, cf=cf)
    assert ret is x                                                      # in place
    out = unlay(x, cf)
    dev_k = float((out.double() - ref64).abs().max())
    short = float((R.tangent_projection_step(P.double(), ori.double(), g.double(), n.double(), STEP, EPS) - ref64).abs().max())
    print(f"B={B} N={N}: kernel deviates {dev_k:.3e}, bound {bound:.3e}; the tangent-projection shortcut would deviate {short:.3e}")
    assert torch.isfinite(out).all()
    assert dev_k <= bound
    assert short > bound                                                 # the bound tells the two forms apart
    assert torch.equal(unlay(nout, cf), n)                               # the normals used
    # inside the eps box up to one ulp
    slack = np.spacing(np.float32(float(out.abs().max())))
    assert float((out.double() - ori.double()).abs().max()) <= float(np.float32(EPS)) + slack
    if B >= 3:
        # g = 0: the clamp of what the victim was shown (the input up to the rewritten rows), no NaN from 0 / (0 + 1e-9)
        shown = R.round_trip(P.double(), n.double())[1]
        want = ori[1].double() + torch.clamp(shown - ori[1].double(), -EPS, EPS)
        assert float((out[1].double() - want).abs().max()) <= bound
        far = n[1][:, 2].abs() < 0.99                                    # (1 / sqrt(1 - z^2) magnifies rounding near the poles)
        assert float((out[1] - P[1]).abs()[far].max()) <= bound          # away from the rewritten rows: the input itself
        # a cloud alone equals the cloud inside the batch, bit for bit
        for b in range(B):
            xb = lay(P[b:b + 1], cf, dev)
            ops.si_step(xb, lay(ori[b:b + 1], cf, dev), lay(g[b:b + 1], cf, dev), STEP, EPS, nrm=lay(n[b:b + 1], cf, dev), cf=cf)
            assert torch.equal(unlay(xb, cf)[0], out[b])


@pytest.mark.parametrize("cf", [False, True], ids=["cl", "cf"])
@pytest.mark.parametrize("B,N", [(1, 20), (3, 65), (3, 257), (3, 1024)])
def test_si_step_idx_mode_is_pca_normal_then_nrm_mode(ops, dev, B, N, cf):
    P, ori, g, _ = step_inputs(B, N, 300 + N)
    x0 = lay(P, cf, dev)
    _, idx = ops.knn_raw(x0, x0, 20, q_cf=cf, r_cf=cf)
    nrm = ops.pca_normal(x0, idx, cf=cf)
    o, gg = lay(ori, cf, dev), lay(g, cf, dev)
    a, b, c = x0.clone(), x0.clone(), x0.clone()
    nout = torch.empty_like(x0)
    ops.si_step(a, o, gg, STEP, EPS, nrm=nrm, cf=cf)
    ops.si_step(b, o, gg, STEP, EPS, idx=idx, nrm_out=nout, cf=cf)
    ops.si_step(c, o, gg, STEP, EPS, idx=idx, cf=cf)
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(nout, nrm)
    assert torch.isfinite(a).all()
    # the cloud the victim is shown: both modes the same bits, and the restatement's round trip within its own bound
    e1 = ops.si_frame(x0, nrm=nrm, cf=cf)
    n2 = torch.empty_like(x0)
    e2 = ops.si_frame(x0, idx=idx, nrm_out=n2, cf=cf)
    assert torch.equal(e1, e2) and torch.equal(n2, nrm)
    nh = unlay(nrm, cf)
    r64, r32 = R.round_trip(P.double(), nh.double()), R.round_trip(P, nh)
    assert float((unlay(e1, cf).double() - r64).abs().max()) <= bound_of(r32, r64)
    with pytest.raises(ValueError):
        ops.si_step(a, o, gg, STEP, EPS, cf=cf)
    with pytest.raises(ValueError):
        ops.si_step(a, o, gg, STEP, EPS, nrm=nrm, idx=idx, cf=cf)


def test_si_step_bad_index_stays_in_its_cloud(ops, dev):
    P, ori, g, _ = step_inputs(3, 65, 9)
    x = lay(P, True, dev)
    _, idx = ops.knn_raw(x, x, 20, q_cf=True, r_cf=True)
    good = x.clone()
    ops.si_step(good, lay(ori, True, dev), lay(g, True, dev), STEP, EPS, idx=idx)
    idx[1, 7, 3] = 65
    ops.si_step(x, lay(ori, True, dev), lay(g, True, dev), STEP, EPS, idx=idx)
    torch.cuda.synchronize()
    assert bool(torch.isnan(x[1, :, 7]).all())                           # the cloud's norm carries the NaN to its points ...
    assert torch.equal(x[0], good[0]) and torch.equal(x[2], good[2])     # ... and to no other cloud


# ------------------------------------------------------------------------------------------------------
# the loop against the fixture
# ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "siadv.npz"))


@pytest.fixture(scope="module")
def nets(dev):
    from oracle import ref_torch as ort
    PointNetCls = M("3dpointcloudattack_amd.model.pointnet").PointNetCls
    out = []
    for seed in (3, 4):
        m = PointNetCls(k=40)
        m.load_state_dict(ort.seeded_state_dict(m, seed))
        out.append(m.eval().to(dev))
    return out


def make_attack(fx, case, nets, **kw):
    eps, step_size, max_steps, top5 = fx[f"{case}_args"]
    over = {k: kw.pop(k) for k in list(kw) if k in ("max_steps", "defense_method")}
    a = dict(eps=float(eps), step_size=float(step_size), max_steps=int(max_steps), num_class=40, top5_attack=bool(top5),
             defense_method=None, transfer_attack_method="ifgm_ours", query_attack_method=None)
    a.update(over)
    si = M("3dpointcloudattack_amd.attack.SIadv.SIadv_attack")
    wb, tgt = kw.pop("wb", nets[0]), kw.pop("tgt", nets[1])
    return si.PointCloudAttack(types.SimpleNamespace(**a), wb_classifier=wb, classifier=tgt, **kw)


def near_ties(P, rel):
    """[B,N] bool: the 20th and 21st neighbour's squared distances within a relative `rel` of each other (float64)."""
    d = R.knn_lists(P.double(), 20, extra=1)[1]
    return (d[..., 20] - d[..., 19]) <= rel * d[..., 20]


@pytest.mark.parametrize("case", ["s5", "s5_top5"])
def test_loop_teacher_forced(fx, nets, dev, case):
    """From each stored P_i one product step lands within band_P of the stored P_{i+1} (top-1: the fast path; top-5: the
    generic path). i = 0 takes the stored normals, later steps estimate their own."""
    atk = make_attack(fx, case, nets)
    assert atk._fast() == (case == "s5")
    band = float(fx[f"{case}_band_P"])
    Ps, target = torch.from_numpy(fx[f"{case}_P"]), torch.from_numpy(fx["target"]).to(dev)
    ori = Ps[0].to(dev)
    for i in range(Ps.shape[0] - 1):
        pts = torch.cat([Ps[i], torch.from_numpy(fx[f"{case}_n"][0])], -1) if i == 0 else Ps[i]
        out = atk.iterate(pts.to(dev), target, steps=1, ori=ori).transpose(1, 2).cpu()
        tie = near_ties(Ps[i], float(fx["tie_rel"])) if i > 0 else torch.zeros(Ps[i].shape[:2], dtype=torch.bool)
        assert float(tie.double().mean()) <= 0.01
        dev_i = float((out.double() - Ps[i + 1].double()).abs()[~tie].max())
        print(f"{case} P_{i} -> P_{i + 1}: deviation {dev_i:.3e} (band_P {band:.3e}), {int(tie.sum())} near-tie points left out")
        assert dev_i <= band


@pytest.mark.parametrize("case", ["s1", "s5", "s5_top5"])
def test_loop_free_running(fx, nets, dev, case):
    atk = make_attack(fx, case, nets)
    points, target = torch.from_numpy(fx["points"]).to(dev), torch.from_numpy(fx["target"]).to(dev)
    band_P, band_gap = float(fx[f"{case}_band_P"]), float(fx[f"{case}_band_gap"])
    one = atk.iterate(points, target, steps=1).transpose(1, 2).cpu()
    d1 = float((one.double() - torch.from_numpy(fx[f"{case}_P"][1]).double()).abs().max())
    print(f"{case}: one step deviates {d1:.3e} (band_P {band_P:.3e})")
    assert d1 <= band_P
    adv, adv_target, count = atk.run(points, target)
    assert adv.shape == (4, 256, 3) and adv_target.shape == (4,) and isinstance(count, int)
    assert torch.isfinite(adv).all()
    slack = float(np.spacing(np.float32(1.2)))
    assert float((adv.cpu().double() - points[:, :, :3].cpu().double()).abs().max()) <= float(np.float32(atk.eps)) + slack
    sure = fx[f"{case}_gap"] > band_gap
    assert sure.sum() * 2 >= len(sure)
    assert np.array_equal(adv_target.cpu().numpy()[sure], fx[f"{case}_adv_target"][sure])
    with torch.no_grad():
        pred = nets[1](adv.transpose(1, 2).contiguous())[0].argmax(1)
    wrong = (pred != target).cpu().numpy().astype(np.int64)
    assert np.array_equal(wrong[sure], fx[f"{case}_count"][sure])
    if sure.all():
        assert count == int(fx[f"{case}_count"].sum())


def test_fast_path_vs_generic_path(fx, nets, dev):
    points, target = torch.from_numpy(fx["points"]).to(dev), torch.from_numpy(fx["target"]).to(dev)
    fast, generic = make_attack(fx, "s5", nets), make_attack(fx, "s5", nets, fused=False)
    assert fast._fast() and not generic._fast()
    band = float(fx["s5_band_P"])
    for steps in (1, 2):
        d = float((fast.iterate(points, target, steps=steps) - generic.iterate(points, target, steps=steps)).abs().max())
        print(f"fast vs generic after {steps} step(s): {d:.3e} (band_P {band:.3e})")
        assert d <= band


def test_fast_step_is_three_launches_more_than_the_victim(fx, nets, dev, monkeypatch):
    """A fast-path step = the launches of the surrogate's fused passes + the search, pc3d_si_frame_f32, pc3d_si_step_f32."""
    _lib = M("3dpointcloudattack_amd._lib")
    names, real = [], _lib.call

    def counted(name, *a):
        names.append(name)
        return real(name, *a)
    atk = make_attack(fx, "s5", nets, graph=False)
    points, target = torch.from_numpy(fx["points"]).to(dev), torch.from_numpy(fx["target"]).to(dev)
    x = points[:, :, :3].transpose(1, 2).contiguous()
    c = atk._loop(x, x, target)
    c.step()                                                             # folded-weight caches are built here, outside the count
    monkeypatch.setattr(_lib, "call", counted)
    nets[0].fused_attack_grad(c.xe, target, "untargeted_logits", 0.0, scale=1.0)
    n_victim = len(names)
    del names[:]
    c.step()
    print(f"launches: surrogate forward+backward {n_victim}, SI-Adv step {len(names)}")
    assert n_victim >= 10 and len(names) == n_victim + 3, (n_victim, names)
    assert [n for n in names if n.startswith("pc3d_si_")] == ["pc3d_si_frame_f32", "pc3d_si_step_f32"]
    assert names[-1] == "pc3d_si_step_f32" and names[0].startswith("pc3d_knn")


def _bitwise_only():
    if os.environ.get("PC3D_DETERMINISTIC", "1") == "0":
        pytest.skip("asserts bit-equality: deterministic mode only (the victim's backward uses float atomics otherwise)")


def test_graph_replay_equals_eager_and_run_equals_run(fx, nets, dev):
    _bitwise_only()
    points, target = torch.from_numpy(fx["points"]).to(dev), torch.from_numpy(fx["target"]).to(dev)
    graphed, eager = make_attack(fx, "s5", nets, max_steps=50), make_attack(fx, "s5", nets, max_steps=50, graph=False)
    a = graphed.iterate(points, target)
    assert len(graphed._loops) == 1 and next(iter(graphed._loops.values())).graphs is not None
    b = graphed.iterate(points, target)                                  # the captured graph again, reloaded
    c = eager.iterate(points, target)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b) and torch.equal(a, c)


def test_cloud_in_batch_equals_cloud_alone(fx, nets, dev):
    _bitwise_only()
    points, target = torch.from_numpy(fx["points"]).to(dev), torch.from_numpy(fx["target"]).to(dev)
    atk = make_attack(fx, "s5", nets, max_steps=50)
    whole = atk.iterate(points, target)
    for b in (0, 3):
        alone = atk.iterate(points[b:b + 1], target[b:b + 1])
        assert torch.equal(alone[0], whole[b])


def _clean_and_adv_loss(atk, points, target, adv):
    def loss(x):
        with torch.no_grad():
            inp = atk.pre_head(x) if atk.pre_head is not None else x
            out = atk.wb_classifier(inp)
            return float(atk.CWLoss(out[0] if isinstance(out, (tuple, list)) else out, target, 0., False, atk.num_class))
    return loss(points[:, :, :3].transpose(1, 2).contiguous()), loss(adv)


@pytest.mark.parametrize("victim", ["defended_sor", "dgcnn"])
def test_generic_path_on_other_surrogates(fx, nets, dev, victim):
    from oracle import ref_torch as ort
    if victim == "dgcnn":
        m = M("3dpointcloudattack_amd.model.dgcnn").DGCNN(types.SimpleNamespace(k=20, emb_dims=1024, dropout=0.5), output_channels=40)
        m.load_state_dict(ort.seeded_state_dict(m, 5))
        wb = m.eval().to(dev)
    else:
        D = M("3dpointcloudattack_amd.defense")
        wb = D.Defended(nets[0], D.SORDefense(k=2, alpha=1.1))
    atk = make_attack(fx, "s5", nets, wb=wb, max_steps=3)
    assert not atk._fast()
    points = torch.from_numpy(fx["points"]).to(dev)
    with torch.no_grad():
        target = wb(points[:, :, :3].transpose(1, 2).contiguous())[0].argmax(1)
    adv = atk.iterate(points, target)
    assert torch.isfinite(adv).all()
    slack = float(np.spacing(np.float32(1.2)))
    assert float((adv.transpose(1, 2) - points[:, :, :3]).abs().max()) <= float(np.float32(atk.eps)) + slack
    clean, after = _clean_and_adv_loss(atk, points, target, adv)
    print(f"{victim}: loss {clean:.4f} clean, {after:.4f} after 3 steps")
    assert after <= clean


def test_defense_head_in_front_of_both_models(fx, nets, dev):
    """defense_method = 'sor': get_defense_head's SORDefense(k=2, alpha=1.1) in front of the surrogate and the target."""
    atk = make_attack(fx, "s5", nets, defense_method="sor", max_steps=2)
    assert type(atk.pre_head).__name__ == "SORDefense" and not atk._fast()
    points, target = torch.from_numpy(fx["points"]).to(dev), torch.from_numpy(fx["target"]).to(dev)
    adv, adv_target, count = atk.run(points, target)
    assert torch.isfinite(adv).all() and adv.shape == (4, 256, 3) and 0 <= count <= 4
