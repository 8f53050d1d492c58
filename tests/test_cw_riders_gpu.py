"""GPU parity, no tolerances: the CW iteration's riders against the launches they replace.

* ops.linear_nn (pc3d_linear_nn_f32: the adv -> ori search as extra workgroups of a head layer's launch) against
  ops.linear + ops.nn_raw;
* ops.linear_book (pc3d_linear_book_f32: the bookkeeping half of the update as extra workgroups) against ops.linear +
  the bookkeeping outputs of ops.cw_update (NOT cw_bookkeep, whose reduction tree differs);
* ops.pointmlp3_max_bwd_update (the update as the epilogue of the last backward launch) against
  pointmlp3_max_bwd_raw(accumulate=True) + ops.cw_update from the same state;
* whole CW iterations, 15 launches against 17, eager and graph-captured, across a binary-step boundary.
Everything is torch.equal; where an input holds a NaN, NaNs are compared by position."""
import importlib

import numpy as np
import pytest
import torch

from helpers import hip_pointnet, unit_cloud

pytestmark = pytest.mark.gpu
ops = importlib.import_module("3dpointcloudattack_amd.ops")


def _mods():
    m = importlib.import_module
    return (m("3dpointcloudattack_amd.attack.CW.CW_attack"), m("3dpointcloudattack_amd.attack.CW.CW_utils.adv_utils"),
            m("3dpointcloudattack_amd.attack.CW.CW_utils.dist_utils"), m("3dpointcloudattack_amd.attack.CW.CW_utils.clip_utils"))


def _same(a, b):
    """torch.equal with NaNs compared by position."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if not a.is_floating_point():
        return torch.equal(a, b)
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(a[~na], b[~nb])


# ---------------------------------------------------------------------------------------------------------------
# search rider
# ---------------------------------------------------------------------------------------------------------------
def _linear_nn_case(dev, K, O, B, N, seed=0, ties=False, nan_query=False, relu=True, gate=False, M=None):
    g = torch.Generator().manual_seed(seed * 7919 + K + 3 * O + 5 * B + 7 * N)
    X = torch.randn(B, K, generator=g).to(dev)
    W = (torch.randn(O, K, generator=g) / K ** 0.5).to(dev)
    bias = torch.randn(O, generator=g).to(dev)
    gt = torch.randn(B, O, generator=g).to(dev) if gate else None
    q = (torch.rand(B, 3, N, generator=g) - 0.5).to(dev)
    r = (torch.rand(B, 3, N if M is None else M, generator=g) - 0.5).to(dev)
    if ties:        # duplicated reference points: the lowest index must win, inside a chunk and across waves
        r[:, :, 1::2] = r[:, :, 0::2][:, :, :r[:, :, 1::2].shape[2]]
        r[:, :, N // 2:] = r[:, :, :N - N // 2]
    if nan_query:
        q[0, 1, 3] = float("nan")
        q[B - 1, :, N - 1] = float("nan")
    Y0 = ops.linear(X, W, bias, relu=relu, gate=gt)
    d0, i0 = ops.nn_raw(q, r, True, True)
    Y1, d1, i1 = ops.linear_nn(X, W, bias, relu=relu, gate=gt, q=q, r=r, q_cf=True, r_cf=True)
    torch.cuda.synchronize()
    assert torch.equal(Y1, Y0)
    assert _same(d1, d0)
    assert torch.equal(i1, i0)
    return d0, i0


@pytest.mark.parametrize("N", [512, 700, 1024])
@pytest.mark.parametrize("B", [5, 32, 37])
@pytest.mark.parametrize("O", [256, 512, 200])
@pytest.mark.parametrize("K", [256, 512, 1024])
def test_linear_nn_matches_linear_and_nn(dev, K, O, B, N):
    _linear_nn_case(dev, K, O, B, N)


@pytest.mark.parametrize("B,N,M", [(32, 2048, 2048),      # the largest reference cloud that rides
                                   (32, 1024, 2048),      # fewer queries than reference points
                                   (5, 700, 1500),
                                   (32, 1024, 4096),      # one tile, but past the rider's range: two launches
                                   (8, 2048, 512)])
def test_linear_nn_other_cloud_sizes(dev, B, N, M):
    _linear_nn_case(dev, 1024, 512, B, N, seed=5, M=M)
    _linear_nn_case(dev, 256, 200, B, N, seed=6, M=M, nan_query=True)


@pytest.mark.parametrize("K,O,B,N", [(1024, 512, 32, 64),     # search outside the rider's range (four-wave form)
                                     (1024, 512, 32, 4096),   # two queries per lane
                                     (200, 512, 8, 1024),     # layer outside the 32 x 16 tiling (K % 16 != 0)
                                     (1024, 32, 8, 1024)])    # ... (O < 64)
def test_linear_nn_fallback(dev, K, O, B, N):
    _linear_nn_case(dev, K, O, B, N, seed=1)


def test_linear_nn_ties_and_nan_query(dev):
    d, i = _linear_nn_case(dev, 1024, 512, 32, 1024, seed=2, ties=True, gate=True)
    assert int((i % 2).sum()) == 0 and int(i.max()) < 512      # ties went to the lowest index
    _linear_nn_case(dev, 1024, 512, 32, 1024, seed=3, nan_query=True)
    _linear_nn_case(dev, 512, 256, 5, 700, seed=4, ties=True, nan_query=True, relu=False)


def test_linear_nn_ride_off_is_two_launches_same_bits(dev):
    g = torch.Generator().manual_seed(11)
    X, W = torch.randn(32, 1024, generator=g).to(dev), torch.randn(512, 1024, generator=g).to(dev)
    q, r = torch.rand(32, 3, 1024, generator=g).to(dev), torch.rand(32, 3, 1024, generator=g).to(dev)
    a = ops.linear_nn(X, W, q=q, r=r, q_cf=True, r_cf=True, ride=True)
    b = ops.linear_nn(X, W, q=q, r=r, q_cf=True, r_cf=True, ride=False)
    assert all(torch.equal(u, v) for u, v in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------
# bookkeeping rider
# ---------------------------------------------------------------------------------------------------------------
def _book_state(dev, B, K, untarget, seed):
    g = torch.Generator().manual_seed(seed)
    ori = (torch.rand(B, 3, K, generator=g) - 0.5).to(dev)
    adv = ori + (torch.randn(B, 3, K, generator=g) * 0.01).to(dev)
    label = torch.randint(0, 40, (B,), generator=g).to(dev)
    pred = label.clone()
    differs = torch.arange(B, device=dev) % 3 != 2          # two of three samples predict another class
    pred[differs] = (pred[differs] + 1) % 40
    dist = torch.sqrt(((adv - ori) ** 2).sum((1, 2)))
    # a mix: per sample, the per-step best / the overall best is above or below the current distance
    sel = torch.arange(B, device=dev)
    bestdist = torch.where(sel % 2 == 0, dist * 2, dist * 0.5)
    o_bestdist = torch.where(sel % 4 < 2, dist * 2, dist * 0.5)
    return dict(adv=adv, ori=ori, pred=pred, label=label, bestdist=bestdist.contiguous(), bestscore=torch.full((B,), -1, device=dev),
                o_bestdist=o_bestdist.contiguous(), o_bestscore=torch.full((B,), -1, device=dev),
                o_bestattack=torch.zeros(B, 3, K, device=dev), input_val=torch.zeros(B, 3, K, device=dev),
                dist_val=torch.zeros(B, device=dev), m=torch.zeros(B, 3, K, device=dev), v=torch.zeros(B, 3, K, device=dev),
                g=(torch.randn(B, 3, K, generator=g) * 1e-3).to(dev), step=torch.full((1,), 3, dtype=torch.int32, device=dev),
                untarget=untarget)


_BOOK_OUT = ("bestdist", "bestscore", "o_bestdist", "o_bestscore", "o_bestattack", "input_val", "dist_val")


@pytest.mark.parametrize("untarget", [True, False])
@pytest.mark.parametrize("K", [333, 1024, 2048, 4096, 8192])
@pytest.mark.parametrize("ride", [True, False])
def test_linear_book_matches_cw_update_bookkeeping(dev, K, untarget, ride):
    B = 12
    ref = _book_state(dev, B, K, untarget, seed=K + int(untarget))
    new = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in ref.items()}
    g = torch.Generator().manual_seed(5)
    X, W = torch.randn(B, 256, generator=g).to(dev), torch.randn(512, 256, generator=g).to(dev)
    gate = torch.randn(B, 512, generator=g).to(dev)
    Y0 = ops.linear(X, W, gate=gate)
    ops.cw_update(ref["adv"], ref["ori"], ref["pred"], ref["label"], untarget, ref["bestdist"], ref["bestscore"],
                  ref["o_bestdist"], ref["o_bestscore"], ref["o_bestattack"], ref["g"], ref["m"], ref["v"], ref["step"], 0.01,
                  0.18, input_val=ref["input_val"], dist_val=ref["dist_val"], dist_kind=1,
                  w=torch.ones(B, device=dev))
    adam = torch.zeros(2, device=dev)
    adv_before = new["adv"].clone()
    Y1 = ops.linear_book(X, W, new["adv"], new["ori"], new["pred"], new["label"], untarget, new["bestdist"], new["bestscore"],
                         new["o_bestdist"], new["o_bestscore"], new["o_bestattack"], gate=gate, input_val=new["input_val"],
                         dist_val=new["dist_val"], step=new["step"], lr=0.01, adam=adam, ride=ride)
    torch.cuda.synchronize()
    assert torch.equal(Y1, Y0)
    assert torch.equal(new["adv"], adv_before)               # the bookkeeping only reads the iterate
    for k in _BOOK_OUT:
        assert torch.equal(new[k], ref[k]), k
    # the mix is really there: improving, non-improving and failing samples
    changed = new["o_bestscore"] != -1
    assert 0 < int(changed.sum()) < B
    assert bool(torch.isfinite(adam).all()) and float(adam[0]) > 0.01 and 0 < float(adam[1]) < 1


# ---------------------------------------------------------------------------------------------------------------
# update epilogue
# ---------------------------------------------------------------------------------------------------------------
def _tower(dev, C3, seed):
    g = torch.Generator().manual_seed(seed)

    def u(*s, k):
        return ((torch.rand(*s, generator=g) * 2 - 1) / k ** 0.5).to(dev)
    w = (u(64, 3, k=3), u(64, k=3), u(128, 64, k=64), u(128, k=64), u(C3, 128, k=128), u(C3, k=128))
    return w + (w[2].t().contiguous(),)


@pytest.mark.parametrize("hits", ["natural", "one_tile"])
@pytest.mark.parametrize("N", [256, 1024, 200, 77, 1025, 2048])     # past 1024: cw_update_kernel<2> on the other side
@pytest.mark.parametrize("dist_kind", [0, 1, 2])
def test_bwd_update_matches_bwd_then_cw_update(dev, dist_kind, N, hits):
    B, C3 = 6, 1024
    untarget = True
    st = _book_state(dev, B, N, untarget, seed=17 * N + dist_kind)
    w = _tower(dev, C3, 3)
    x = st["adv"]
    pooled, argidx, masks = ops.pointmlp3_max_fwd_raw(x, w, True, want_masks=True)
    if hits == "one_tile":       # every channel's arg-max in one tile: all the other tiles take the no-hit exit
        c = torch.arange(C3, device=dev)
        argidx = (32 * ((N // 32) // 2) + c % 32).clamp(max=N - 1).to(torch.int32)[None, :].expand(B, C3).contiguous()
    gen = torch.Generator().manual_seed(N)
    g_pooled = (torch.randn(B, C3, generator=gen) * 1e-2).to(dev)
    gx0 = st["g"]
    wts = (torch.rand(B, generator=gen) * 20 + 1).to(dev)
    st["m"].copy_((torch.randn(B, 3, N, generator=gen) * 1e-3).to(dev))
    st["v"].copy_((torch.rand(B, 3, N, generator=gen) * 1e-6).to(dev))
    _, nn_idx = ops.nn_raw(x, st["ori"], True, True)
    ref = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in st.items()}
    new = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in st.items()}
    # reference: backward in accumulate form, then the one-launch update
    gx_ref = gx0.clone()
    ops.pointmlp3_max_bwd_raw(ref["adv"], w, argidx, g_pooled, masks, out=gx_ref, accumulate=True)
    ops.cw_update(ref["adv"], ref["ori"], ref["pred"], ref["label"], untarget, ref["bestdist"], ref["bestscore"],
                  ref["o_bestdist"], ref["o_bestscore"], ref["o_bestattack"], gx_ref, ref["m"], ref["v"], ref["step"], 0.01,
                  0.18, input_val=ref["input_val"], dist_val=ref["dist_val"], dist_kind=dist_kind, w=wts, nn_idx=nn_idx)
    # new: bookkeeping rider (writes dist_val and the Adam factors), then the backward with the update as its epilogue
    adam = torch.zeros(2, device=dev)
    gen2 = torch.Generator().manual_seed(1)
    X, W = torch.randn(B, 256, generator=gen2).to(dev), torch.randn(512, 256, generator=gen2).to(dev)
    ops.linear_book(X, W, new["adv"], new["ori"], new["pred"], new["label"], untarget, new["bestdist"], new["bestscore"],
                    new["o_bestdist"], new["o_bestscore"], new["o_bestattack"], input_val=new["input_val"],
                    dist_val=new["dist_val"], step=new["step"], lr=0.01, adam=adam)
    gx_new = gx0.clone()
    ops.pointmlp3_max_bwd_update(new["adv"], w, argidx, g_pooled, masks, gx_new, new["ori"], new["m"], new["v"], adam, 0.18,
                                 dist_kind=dist_kind, w=wts, dist_val=new["dist_val"], nn_idx=nn_idx)
    torch.cuda.synchronize()
    assert torch.equal(gx_new, gx0)                          # gx is only read
    for k in ("adv", "m", "v") + _BOOK_OUT:
        assert torch.equal(new[k], ref[k]), k
    assert not torch.equal(new["adv"], st["adv"])


# ---------------------------------------------------------------------------------------------------------------
# whole iterations: 15 launches against 17
# ---------------------------------------------------------------------------------------------------------------
class _Calls:
    """Counts the calls of the three rider ops and of the launches they replace while a loop runs."""
    NAMES = ("linear_nn", "linear_book", "pointmlp3_max_bwd_update", "cw_update", "nn_raw")

    def __init__(self, monkeypatch):
        self.n = dict.fromkeys(self.NAMES, 0)
        for nm in self.NAMES:
            monkeypatch.setattr(ops, nm, self._wrap(nm, getattr(ops, nm)))

    def _wrap(self, nm, fn):
        def counted(*a, **k):
            self.n[nm] += 1
            return fn(*a, **k)
        return counted


def _drive(dev, B, N, dist_name, graph, riders, iters=22):
    from bench import DUMPED_STATE
    cwm, adv, dist, clip = _mods()
    model, _ = hip_pointnet(0, dev)
    trans_model, _ = hip_pointnet(1, dev)
    rng = np.random.default_rng(100 + B + N)
    pcs = torch.from_numpy(np.stack([unit_cloud(rng, N) for _ in range(B)]))
    with torch.no_grad():
        labels = model(pcs.transpose(1, 2).contiguous().to(dev))[0].argmax(1).cpu()
    dist_func = dist.ChamferDist() if dist_name == "chamfer" else dist.L2Dist()
    atk = cwm.CW(model, trans_model, adv_func=adv.UntargetedLogitsAdvLoss(5.), clip_func=clip.ClipPointsLinf(0.18),
                 dist_func=dist_func, binary_step=2, num_iter=iters, graph=graph, riders=riders)
    torch.manual_seed(5)
    st = atk._begin(pcs, labels)
    atk._begin_binary_step(st)
    if graph:
        run = atk._make_runner(st, warmup=3, unroll=4)      # its 3 warm-up passes are real iterations, in both runs
        assert hasattr(run, "flush")
    else:
        run = lambda: atk._iterate(st)                      # noqa: E731
    for _ in range(iters):
        run()
    if graph:
        run.flush()
    atk._end_binary_step(st)                                # the binary-step boundary: new weights, fresh start point
    atk._begin_binary_step(st)
    for _ in range(iters):
        run()
    if graph:
        run.flush()
    torch.cuda.synchronize()
    return {k: st[k].detach().clone() for k in DUMPED_STATE + ("exp_avg", "exp_avg_sq", "step")}


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("dist_name", ["chamfer", "l2"])
@pytest.mark.parametrize("B,N", [(4, 256), (32, 1024)])
def test_cw_15_launch_iteration_equals_17_launch(dev, B, N, dist_name, graph, monkeypatch):
    with monkeypatch.context() as mp:
        calls = _Calls(mp)
        new = _drive(dev, B, N, dist_name, graph, True)
    # the new path really ran: every queued iteration (eager: 44; captured: the warm-up passes and the graphs' bodies) went
    # through the riders, none through the launches they replace
    assert calls.n["linear_book"] == calls.n["pointmlp3_max_bwd_update"] >= (8 if graph else 44)
    assert calls.n["linear_nn"] == (calls.n["linear_book"] if dist_name == "chamfer" else 0)
    assert calls.n["cw_update"] == 0 and calls.n["nn_raw"] == 0
    with monkeypatch.context() as mp:
        calls = _Calls(mp)
        old = _drive(dev, B, N, dist_name, graph, False)
    assert calls.n["linear_nn"] == calls.n["linear_book"] == calls.n["pointmlp3_max_bwd_update"] == 0
    assert calls.n["cw_update"] >= (8 if graph else 44)
    assert int(new["step"]) == int(old["step"]) == 22
    for k in old:
        assert torch.equal(new[k], old[k]), k
    assert float(old["o_bestdist"].min()) < 1e9              # the attack got somewhere: the bookkeeping was exercised


@pytest.mark.parametrize("piece", ["search", "update"])
def test_cw_single_piece_equals_17_launch(dev, piece, monkeypatch):
    with monkeypatch.context() as mp:
        calls = _Calls(mp)
        new = _drive(dev, 4, 256, "chamfer", False, {piece}, iters=20)
    assert calls.n["linear_nn"] == 40 and calls.n["nn_raw"] == 0        # one call either way; `ride` decides the launches
    assert calls.n["linear_book"] == calls.n["pointmlp3_max_bwd_update"] == (40 if piece == "update" else 0)
    assert calls.n["cw_update"] == (0 if piece == "update" else 40)
    old = _drive(dev, 4, 256, "chamfer", False, False, iters=20)
    for k in old:
        assert torch.equal(new[k], old[k]), k
