"""GPU: the SOR / SRS defence heads (csrc/defense.hip) against the reference fixture (tests/golden/defense.npz) and against
the plain-torch restatement of the reference's algorithm (test_defense_cpu.RestatedSOR) on the same device."""
import importlib
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from helpers import hip_pointnet, unit_cloud
from test_defense_cpu import SWEEP, SWEEP_BAND, SWEEP_CAP, RestatedSOR, cases, sweep_clouds

pytestmark = pytest.mark.gpu
ops = importlib.import_module("3dpointcloudattack_amd.ops")
dfn = importlib.import_module("3dpointcloudattack_amd.defense")


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "defense.npz"))


def _layouts(x_cf):
    """The [B,3,K] tensor as given and as a channel-first VIEW of a [B,K,3] buffer (point stride 3, channel stride 1)."""
    return {"channel_first": x_cf.contiguous(), "channel_last_view": x_cf.transpose(1, 2).contiguous().transpose(1, 2)}


@pytest.mark.parametrize("fused", [False, True])
def test_sor_matches_the_reference_fixture(dev, fx, fused):
    """mask, count, src equal; output bit-equal to the points it copies; gradient of (out * G).sum() to fp32 summation
    tolerance (at most ceil(npoint / n_b) addends per point), exactly zero on dropped points; both layouts."""
    for name, k, alpha, npoint, band in cases(fx):
        x0 = torch.from_numpy(fx[f"{name}_x"]).to(dev)
        mask, n = fx[f"{name}_mask"], fx[f"{name}_n"]
        for lay, x in _layouts(x0).items():
            x = x.detach().requires_grad_()
            head = dfn.SORDefense(k=k, alpha=alpha, npoint=npoint)
            head.fused = fused
            out, count, src = head(x, return_info=True)
            assert out.shape == (x.shape[0], 3, npoint) and count.dtype == torch.int32 and src.dtype == torch.int32
            assert np.array_equal(count.cpu().numpy(), n), (name, lay)
            src_ref = np.stack([np.nonzero(mask[b])[0][np.arange(npoint) % n[b]] for b in range(len(n))])
            assert np.array_equal(src.cpu().numpy(), src_ref), (name, lay)
            assert np.array_equal(out.detach().cpu().numpy(), fx[f"{name}_out"]), (name, lay)       # bit-equal copies
            (out * torch.from_numpy(fx[f"{name}_G"]).to(dev)).sum().backward()
            g = x.grad.cpu().numpy()
            np.testing.assert_allclose(g, fx[f"{name}_grad"], rtol=1e-6, err_msg=f"{name} {lay}")
            assert np.all(g[~np.repeat(mask[:, None, :], 3, 1)] == 0.0), (name, lay)
        # the raw entry on a channel-last tensor: same selection, [B,npoint,3] output
        r = dfn.sor_select(x0.transpose(1, 2).contiguous(), k, alpha, npoint, cf=False, fused=fused)
        assert np.array_equal(r["out"].cpu().numpy().transpose(0, 2, 1), fx[f"{name}_out"]), name
        rank = r["rank"].cpu().numpy()
        assert np.array_equal(rank >= 0, mask) and all(
            np.array_equal(rank[b][mask[b]], np.arange(n[b])) for b in range(len(n))), name


@pytest.mark.parametrize("fused", [False, True])
def test_sor_v_and_thr_within_the_stored_band(dev, fx, fused):
    for name, k, alpha, npoint, band in cases(fx):
        x = torch.from_numpy(fx[f"{name}_x"]).to(dev)
        r = dfn.sor_select(x, k, alpha, npoint, fused=fused, want_stats=True)
        v, thr = r["v"].double().cpu().numpy(), r["thr"].double().cpu().numpy()
        rv, rthr = fx[f"{name}_v"], fx[f"{name}_thr"]
        dv = np.max(np.abs(v - rv) / np.maximum(rv, rthr[:, None]))
        dt = np.max(np.abs(thr - rthr) / rthr)
        print(f"{name} fused={fused}: v dev {dv:.2e} thr dev {dt:.2e} band {band:.2e}")
        assert dv <= band and dt <= band, (name, dv, dt, band)


def _fwd_bwd(x, k, alpha, npoint, G, fused=False):
    x = x.detach().clone().requires_grad_()
    head = dfn.SORDefense(k=k, alpha=alpha, npoint=npoint)
    head.fused = fused
    out, count, src = head(x, return_info=True)
    (out * G).sum().backward()
    return out.detach(), count, src, x.grad


@pytest.mark.parametrize("det", [True, False])
def test_sor_reproducible_run_batch_and_graph(dev, fx, det):
    """run == run, a cloud in a batch == the cloud alone, eager == graph replay — torch.equal, forward and backward."""
    k, alpha, npoint = 2, 1.1, 1024
    x = torch.from_numpy(fx["k1024_x"]).to(dev)
    G = torch.from_numpy(fx["k1024_G"]).to(dev)
    with ops.deterministic(det):
        a = _fwd_bwd(x, k, alpha, npoint, G)
        b = _fwd_bwd(x, k, alpha, npoint, G)
        assert all(torch.equal(p, q) for p, q in zip(a, b))
        for i in range(x.shape[0]):
            one = _fwd_bwd(x[i:i + 1], k, alpha, npoint, G[i:i + 1])
            assert all(torch.equal(p[i:i + 1], q) for p, q in zip(a, one)), i
        # graph: forward + backward captured once, replayed on fresh input values
        sx = x.clone().requires_grad_()
        head = dfn.SORDefense(k=k, alpha=alpha, npoint=npoint)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                o = head(sx)
                gx, = torch.autograd.grad((o * G).sum(), sx)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            so, sc, ss = head(sx, return_info=True)
            sg, = torch.autograd.grad((so * G).sum(), sx)
        for xin in (x, x.flip(0)):
            with torch.no_grad():
                sx.copy_(xin)
            graph.replay()
            e = _fwd_bwd(xin, k, alpha, npoint, G)
            assert torch.equal(so, e[0]) and torch.equal(sc, e[1]) and torch.equal(ss, e[2]) and torch.equal(sg, e[3])


def test_sor_random_shapes_against_the_restatement(dev):
    """The sweep of test_defense_cpu (K 64 .. 4096, npoint >= K, k 1 .. 8, B 1 / 3 / 32) against the float64 restatement on
    this device; ties inside SWEEP_BAND are excused, at most SWEEP_CAP of all points."""
    total = excused = 0
    for i, (B, K, k, npoint, alpha) in enumerate(SWEEP):
        x = torch.from_numpy(sweep_clouds(i)).to(dev).requires_grad_()
        ref = RestatedSOR(k, alpha, npoint)
        rout = ref(x)
        G = torch.rand(rout.shape, device=dev, generator=torch.Generator(dev).manual_seed(i)) + 0.5
        rgrad, = torch.autograd.grad((rout * G).sum(), x)
        inside = (ref.v - ref.thr[:, None]).abs() <= SWEEP_BAND * ref.thr[:, None]
        total += inside.numel()
        excused += int(inside.sum())
        for fused in (False, True) if k <= 8 else (False,):
            r = dfn.sor_select(x.detach(), k, alpha, npoint, fused=fused, want_stats=True)
            mask = r["rank"] >= 0
            assert torch.equal(mask[~inside], ref.mask[~inside]), (i, fused)
            clean = ~inside.any(1)                     # clouds without an excused point: everything must agree
            assert torch.equal(r["count"][clean].long(), ref.n[clean]), (i, fused)
            assert torch.equal(r["src"][clean].long(), ref.src[clean]), (i, fused)
            assert torch.equal(r["out"][clean], rout.detach()[clean]), (i, fused)
            np.testing.assert_allclose(r["v"].double().cpu().numpy(), ref.v.cpu().numpy(),
                                       atol=SWEEP_BAND * float(ref.thr.max()), rtol=SWEEP_BAND)
            g = dfn.sor_backward(G, r["count"], r["rank"])
            np.testing.assert_allclose(g[clean].cpu().numpy(), rgrad[clean].cpu().numpy(), rtol=1e-6, err_msg=str(i))
    print(f"sweep: {excused} of {total} points inside the band (excused)")
    assert excused <= SWEEP_CAP * total, (excused, total)


def test_srs_device_draw(dev):
    """Rows of K - drop_num distinct in-range indices; same (seed, counter) -> same table; successive calls and
    successive graph replays differ; inclusion counts within 6 sigma of Binomial(T * B, (K - drop_num) / K)."""
    B, K, drop = 8, 1024, 500
    M = K - drop
    a = dfn.srs_select(123, 7, B, K, M, dev)
    assert a.shape == (B, M) and a.dtype == torch.int32
    s = a.long().sort(1)[0]
    assert int(s.min()) >= 0 and int(s.max()) < K and bool((s[:, 1:] > s[:, :-1]).all())
    assert torch.equal(a, dfn.srs_select(123, 7, B, K, M, dev))
    ctr = torch.full((1,), 7, dtype=torch.int32, device=dev)
    assert torch.equal(a, dfn.srs_select(123, ctr, B, K, M, dev))             # device counter == host counter
    assert not torch.equal(a, dfn.srs_select(123, 8, B, K, M, dev))
    assert not torch.equal(a, dfn.srs_select(124, 7, B, K, M, dev))
    assert not torch.equal(a[0], a[1])
    for K2, M2 in ((64, 1), (100, 100), (777, 300), (4096, 3596), (2, 1)):       # padded sizes, M == K, the limits
        t = dfn.srs_select(5, 0, 3, K2, M2, dev).long().sort(1)[0]
        assert t.shape == (3, M2) and int(t.min()) >= 0 and int(t.max()) < K2 and bool((t[:, 1:] > t[:, :-1]).all())

    # the module: successive calls differ, output = the gathered points in drawn order
    head = dfn.SRSDefense(drop_num=drop, device_rng=True, seed=99).to(dev)
    x = torch.from_numpy(np.stack([unit_cloud(np.random.default_rng(b), K) for b in range(B)])).to(dev).transpose(1, 2).contiguous()
    o1, o2 = head(x), head(x)
    assert o1.shape == (B, 3, M) and not torch.equal(o1, o2) and not o1.requires_grad
    idx = dfn.srs_select(99, 0, B, K, M, dev)
    assert torch.equal(o1, torch.gather(x, 2, idx.long()[:, None, :].expand(B, 3, M)))
    assert int(head.calls.item()) == 2
    # graph replays advance the device counter
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        so = head(x)
    reps = []
    for _ in range(3):
        graph.replay()
        reps.append(so.clone())
    assert not torch.equal(reps[0], reps[1]) and not torch.equal(reps[1], reps[2])
    assert torch.equal(reps[0], torch.gather(x, 2, dfn.srs_select(99, 2, B, K, M, dev).long()[:, None, :].expand(B, 3, M)))
    assert int(head.calls.item()) == 5

    # uniformity: every point's inclusion count over T calls x B clouds
    T, p = 200, M / K
    cnt = torch.zeros((K,), dtype=torch.int64, device=dev)
    for t in range(T):
        cnt += torch.bincount(dfn.srs_select(2024, t, B, K, M, dev).long().flatten(), minlength=K)
    nn_, sigma = T * B, math.sqrt(T * B * p * (1 - p))
    dev_max = float((cnt.double() - nn_ * p).abs().max())
    print(f"inclusion counts: largest deviation {dev_max:.1f} = {dev_max / sigma:.2f} sigma")
    assert dev_max <= 6 * sigma
    assert int(cnt.sum()) == T * B * M


def test_srs_host_mode_matches_the_reference_tables(dev, fx):
    x = torch.from_numpy(fx["k1024_x"]).to(dev)
    for drop in fx["srs_drops"]:
        np.random.seed(int(fx["srs_seed"]))
        out = dfn.SRSDefense(drop_num=int(drop))(x)
        idx = torch.from_numpy(fx[f"srs{int(drop)}_idx"]).long().to(dev)
        assert torch.equal(out, torch.gather(x, 2, idx[:, None, :].expand(-1, 3, -1)))


def _cw_mods():
    m = importlib.import_module
    return (m("3dpointcloudattack_amd.attack.CW.CW_attack"), m("3dpointcloudattack_amd.attack.CW.CW_utils.adv_utils"),
            m("3dpointcloudattack_amd.attack.CW.CW_utils.dist_utils"), m("3dpointcloudattack_amd.attack.CW.CW_utils.clip_utils"))


CW_SEED = 409      # clouds of test_cw_through_defended_pointnet: no iterate of the restatement's run inside the tie band


def run_cw_defended(dev, which, seed=CW_SEED):
    """CW (B = 4, K = 256, 2 x 15 iterations, seeded weights, fused=False) on Defended(PointNet, head); which: "hip" / "ref".
    Returns (attack() result + fail counters, the restatement head or None)."""
    cwm, adv, dist, clip = _cw_mods()
    model, _ = hip_pointnet(0, dev)
    trans, _ = hip_pointnet(1, dev)
    B, K, steps, iters = 4, 256, 2, 15
    rng = np.random.default_rng(seed)
    pcs = torch.from_numpy(np.stack([unit_cloud(rng, K) for _ in range(B)]))
    ref_head = RestatedSOR(2, 1.1, K)
    with torch.no_grad():
        labels = dfn.Defended(model, ref_head)(pcs.transpose(1, 2).contiguous().to(dev))[0].argmax(1).cpu()
    ref_head.min_margin = None
    vic = dfn.Defended(model, dfn.SORDefense(k=2, alpha=1.1, npoint=K) if which == "hip" else ref_head)
    atk = cwm.CW(vic, trans, adv_func=adv.UntargetedLogitsAdvLoss(5.), clip_func=clip.ClipPointsLinf(0.18),
                 dist_func=dist.ChamferDist(), binary_step=steps, num_iter=iters, fused=False)
    assert atk.model is vic and not atk._capturable()                    # graphed.wrap leaves it eager
    torch.manual_seed(11)
    np.random.seed(11)
    return atk.attack(pcs, labels) + (atk.attack_fail, atk.shuffle_fail, atk.trans_fail), (ref_head if which == "ref" else None)


def test_cw_through_defended_pointnet(dev):
    """Defended(PointNet, SORDefense) as the victim of CW (autograd path) against the same attack on a Defended whose head is
    the plain-torch restatement: best distance rtol 2e-3 on samples successful in both, clouds atol 2e-4 (the figures of
    test_pointnet_cw_gpu's two-path comparison). CW_SEED is chosen so that no iterate of the restatement's run has a point
    inside the tie band; that is checked here, not assumed."""
    ref, ref_head = run_cw_defended(dev, "ref")
    margin = float(ref_head.min_margin)
    print(f"smallest tie margin over the restatement's run: {margin:.3e} (band {SWEEP_BAND:.3e})")
    assert margin > SWEEP_BAND, f"an iterate has a point inside the tie band ({margin:.3e}): choose another seed"
    hip, _ = run_cw_defended(dev, "hip")
    (bd, ba, sn), (rbd, rba, rsn) = hip[:3], ref[:3]
    assert sn == rsn and np.array_equal(bd < 1e9, rbd < 1e9)
    ok = (bd < 1e9) & (rbd < 1e9)
    print("successful in both:", int(ok.sum()), "of", len(bd), "best distances", bd, rbd)
    np.testing.assert_allclose(bd[ok], rbd[ok], rtol=2e-3)
    np.testing.assert_allclose(ba, rba, atol=2e-4)
    assert hip[3:] == ref[3:]


def test_defended_trans_model_changes_trans_fail_only(dev):
    cwm, adv, dist, clip = _cw_mods()
    model, _ = hip_pointnet(0, dev)
    trans, _ = hip_pointnet(1, dev)
    B, K = 4, 256
    rng = np.random.default_rng(405)
    pcs = torch.from_numpy(np.stack([unit_cloud(rng, K) for _ in range(B)]))
    with torch.no_grad():
        labels = model(pcs.transpose(1, 2).contiguous().to(dev))[0].argmax(1).cpu()
    outs = []
    for tm in (trans, dfn.Defended(trans, dfn.SORDefense(npoint=K)), dfn.Defended(trans, dfn.SRSDefense(drop_num=100, device_rng=True, seed=1))):
        atk = cwm.CW(model, tm, adv_func=adv.UntargetedLogitsAdvLoss(5.), clip_func=clip.ClipPointsLinf(0.18),
                     dist_func=dist.ChamferDist(), binary_step=2, num_iter=15)
        torch.manual_seed(3)
        np.random.seed(3)
        bd, ba, sn = atk.attack(pcs, labels)
        outs.append((bd, ba, sn, atk.attack_fail, atk.shuffle_fail))
        assert 0 <= atk.trans_fail <= B
    for o in outs[1:]:
        assert np.array_equal(o[0], outs[0][0]) and np.array_equal(o[1], outs[0][1]) and o[2:] == outs[0][2:]


def test_evaluate_defended_equals_argmax_of_composition(dev):
    model, _ = hip_pointnet(0, dev)
    rng = np.random.default_rng(8)
    B, K = 10, 512
    pcs = np.stack([unit_cloud(rng, K) for _ in range(B)])                        # [B,K,3]
    head = dfn.SORDefense(npoint=K)
    with torch.no_grad():
        want = model(head(torch.from_numpy(pcs).to(dev).transpose(1, 2).contiguous()))[0].argmax(1).cpu().numpy()
    labels = want.copy()
    labels[::3] = (labels[::3] + 1) % 40
    for clouds in (pcs, torch.from_numpy(pcs).transpose(1, 2), torch.from_numpy(pcs).to(dev)):
        r = dfn.evaluate_defended(model, head, clouds, labels, batch=4)
        assert np.array_equal(r["pred"], want) and r["pred"].dtype == np.int64
        assert np.array_equal(r["correct"], want == labels) and r["count"] == int((want == labels).sum())


def test_no_host_sync(dev, fx):
    """SOR forward + backward and the SRS device draw run with synchronising calls turned into errors."""
    x = torch.from_numpy(fx["k1024_x"]).to(dev).requires_grad_()
    G = torch.from_numpy(fx["k1024_G"]).to(dev)
    sor = dfn.SORDefense()
    srs = dfn.SRSDefense(drop_num=500, device_rng=True, seed=5).to(dev)
    sor(x), srs(x)                                                               # lazy initialisation outside the check
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for fused in (False, True):
            sor.fused = fused
            out, count, src = sor(x, return_info=True)
            g, = torch.autograd.grad((out * G).sum(), x)
        o = srs(x)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(g).all() and o.shape == (4, 3, 524)
