"""GPU: hipGraph replay of a victim's forward/backward (3dpointcloudattack_amd/graphed.py) returns what the eager
launches return, and never lets a replay overwrite memory an earlier forward still needs."""
import gc
import importlib
import os
import types
import weakref

import numpy as np
import pytest
import torch

from oracle import ref_torch as ort

pytestmark = pytest.mark.gpu
graphed = importlib.import_module("3dpointcloudattack_amd.graphed")


def _victim(dev, name):
    if name == "curvenet":
        m = importlib.import_module("3dpointcloudattack_amd.model.curvenet").CurveNet(num_classes=40)
    elif name == "dgcnn":
        m = importlib.import_module("3dpointcloudattack_amd.model.dgcnn").DGCNN(
            types.SimpleNamespace(k=20, emb_dims=1024, dropout=0.5), output_channels=40)
    else:
        m = importlib.import_module("3dpointcloudattack_amd.model.pointnet").PointNetCls(k=40, feature_transform=False)
    m.load_state_dict(ort.seeded_state_dict(m, 3, gain=1.0))
    return m.eval().to(dev)


def _grad(model, x, w):
    xa = x.clone().requires_grad_()
    out = model(xa)
    logits = out[0]
    (logits * w).sum().backward()
    return logits.detach().clone(), xa.grad.clone(), out


@pytest.mark.parametrize("name", ["curvenet", "dgcnn", "pointnet"])
def test_replay_matches_eager(dev, name):
    m = _victim(dev, name)
    g = graphed.wrap(m)
    assert isinstance(g, graphed.GraphedVictim) and graphed.wrap(m) is g
    gen = torch.Generator().manual_seed(0)
    w = torch.randn(4, 40, generator=gen).to(dev)
    for trial in range(3):                                  # capture on the first call, replays after it
        x = (torch.rand(4, 3, 1024, generator=gen) - 0.5).to(dev)
        le, ge, oe = _grad(m, x, w)
        lg, gg, og = _grad(g, x, w)
        assert len(oe) == len(og)
        torch.testing.assert_close(lg, le, rtol=1e-4, atol=1e-5)
        assert (gg - ge).norm() <= 2e-3 * ge.norm() + 1e-12, (trial, g.stats)
        with torch.no_grad():
            torch.testing.assert_close(g(x)[0], m(x)[0], rtol=1e-4, atol=1e-5)
    assert g.stats["replayed"] >= 6 and g.stats["eager"] == 0 and g.stats["captures"] == 2, g.stats


def test_forwards_waiting_for_backward_keep_their_memory(dev):
    """Several forwards before one backward (expectation-over-transformation loops): each replays its own replica of
    the capture, beyond MAX_REPLICAS the call runs eagerly; the gradients are those of the eager victim. The first
    forward's OUTPUT tensor is dropped on purpose: what keeps a replica busy is its autograd node."""
    m = _victim(dev, "dgcnn")
    g = graphed.wrap(m)
    gen = torch.Generator().manual_seed(1)
    n = graphed.MAX_REPLICAS + 1
    xs = [(torch.rand(2, 3, 256, generator=gen) - 0.5).to(dev).requires_grad_() for _ in range(n)]
    w = torch.randn(2, 40, generator=gen).to(dev)
    loss = 0.
    for x in xs:
        loss = loss + (g(x)[0] * w).sum()
    assert g.stats["captures"] == graphed.MAX_REPLICAS and g.stats["eager"] == 1
    loss.backward()
    rs = [x.detach().clone().requires_grad_() for x in xs]
    sum((m(r)[0] * w).sum() for r in rs).backward()
    for x, r in zip(xs, rs):
        assert (x.grad - r.grad).norm() <= 2e-3 * r.grad.norm() + 1e-12
    before = dict(g.stats)
    g(xs[0].detach().clone().requires_grad_())[0].sum().backward()      # all replicas are free again: a replay
    assert g.stats["eager"] == before["eager"] and g.stats["captures"] == before["captures"]


def test_recaptures_when_weights_change(dev):
    m = _victim(dev, "pointnet")
    g = graphed.wrap(m)
    x = (torch.rand(2, 3, 128, generator=torch.Generator().manual_seed(2)) - 0.5).to(dev)
    with torch.no_grad():
        before = g(x)[0].clone()
        m.load_state_dict(ort.seeded_state_dict(m, 4, gain=1.0))
        after = g(x)[0]
        torch.testing.assert_close(after, m(x)[0], rtol=1e-4, atol=1e-5)
    assert not torch.allclose(before, after)


def test_non_deterministic_victims_are_left_alone(dev):
    ssg = importlib.import_module("3dpointcloudattack_amd.model.pointnet2_SSG").PointNet_Ssg(num_classes=40)
    assert graphed.wrap(ssg) is ssg


def test_capture_survives_cache_invalidation(dev):
    """.eval() / .to(device) drop the victims' folded-weight caches even when nothing changed; a capture made before
    must keep replaying correctly (it keeps the tensors it was captured with alive)."""
    m = _victim(dev, "pointnet")
    g = graphed.wrap(m)
    gen = torch.Generator().manual_seed(5)
    x = (torch.rand(3, 3, 200, generator=gen) - 0.5).to(dev)
    w = torch.randn(3, 40, generator=gen).to(dev)
    _grad(g, x, w)
    ref_l, ref_g, _ = _grad(m, x, w)
    for _ in range(3):
        m.train(True), m.eval(), m.to(dev), m._invalidate()
        junk = [torch.full((1 << 16,), float("nan"), device=dev) for _ in range(64)]    # reuse whatever was freed
        l, gr, _ = _grad(g, x, w)
        del junk
        torch.testing.assert_close(l, ref_l, rtol=1e-4, atol=1e-5)
        assert (gr - ref_g).norm() <= 2e-3 * ref_g.norm() + 1e-12
    assert g.stats["captures"] == 1


def test_leaf_grad_accumulates_across_replays(dev):
    """the replayed backward must not hand its static grad buffer to AccumulateGrad — two backward passes
    into the same leaf without clearing .grad give g1 + g2, as eager does."""
    m = _victim(dev, "pointnet")
    g = graphed.wrap(m)
    gen = torch.Generator().manual_seed(8)
    x = (torch.rand(2, 3, 160, generator=gen) - 0.5).to(dev)
    w1, w2 = torch.randn(2, 40, generator=gen).to(dev), torch.randn(2, 40, generator=gen).to(dev)
    xe, xg = x.clone().requires_grad_(), x.clone().requires_grad_()
    for model, leaf in ((m, xe), (g, xg)):
        (model(leaf)[0] * w1).sum().backward()
        (model(leaf)[0] * w2).sum().backward()
    assert g.stats["replayed"] >= 2
    assert (xg.grad - xe.grad).norm() <= 2e-3 * xe.grad.norm()


def test_mode_switch_recaptures(dev):
    """The backward kernel flavour (ordered sums / float atomics) is baked into a capture: a graphed victim used with
    deterministic=False must not hand that capture to a later deterministic call of the same shape. After an
    atomic-mode pass, deterministic passes through the SAME wrapper are bit-equal to each other and to the eager victim."""
    ops = importlib.import_module("3dpointcloudattack_amd.ops")
    m = _victim(dev, "dgcnn")
    g = graphed.wrap(m)
    gen = torch.Generator().manual_seed(5)
    w = torch.randn(4, 40, generator=gen).to(dev)
    x = (torch.rand(4, 3, 1024, generator=gen) - 0.5).to(dev)
    with ops.deterministic(False):
        _grad(g, x, w)
        _grad(g, x, w)
    caps = g.stats["captures"]
    with ops.deterministic(True):
        _, g1, _ = _grad(g, x, w)
        _, g2, _ = _grad(g, x, w)
        _, ge, _ = _grad(m, x, w)
    assert g.stats["captures"] == caps + 1, g.stats       # its own capture, not the atomic one's
    assert torch.equal(g1, g2) and torch.equal(g1, ge)


# -- LoopGraph: the one capture protocol of the package's loops. No victim: the body is x += 1 on 64 floats. ----------
def _counter(dev):
    x = torch.zeros(64, device=dev)
    return x, (lambda: x.add_(1))


def test_loop_graph_warmup_and_replay(dev):
    """The warm-up passes are real passes, capture itself executes nothing, and a graph of n passes advances by n."""
    x, body = _counter(dev)
    loop = graphed.LoopGraph(body, dev, warmup=2, counts=(1, 4))
    assert sorted(loop.graphs) == [1, 4]
    assert torch.equal(x, torch.full_like(x, 2.0))
    loop.replay(4)
    loop.replay()
    assert torch.equal(x, torch.full_like(x, 7.0))


def test_loop_graph_keeps_what_the_graphs_point_at(dev):
    """keep holds the tensors the caches hand out during the capture (note_captured) and the owners' cached tensors."""
    x, _ = _counter(dev)
    handed = torch.ones(64, device=dev)
    owner = torch.nn.Linear(2, 2).to(dev)
    owner.folded_cache = (torch.zeros(3, device=dev), [torch.zeros(5, device=dev)])      # plain attribute, not a buffer

    def body():
        graphed.note_captured(handed)
        x.add_(handed)
    loop = graphed.LoopGraph(body, dev, warmup=1, owners=(owner,))
    kept = {id(t) for t in loop.keep}
    assert id(handed) in kept
    assert id(owner.folded_cache[0]) in kept and id(owner.folded_cache[1][0]) in kept
    assert id(owner.weight) not in kept                    # parameters belong to the module, not to its caches
    assert not graphed.capturing()


@pytest.mark.parametrize("gc_on", [True, False])
def test_loop_graph_leaves_the_collector_as_it_was(dev, gc_on):
    _, body = _counter(dev)
    was = gc.isenabled()
    try:
        gc.enable() if gc_on else gc.disable()
        graphed.LoopGraph(body, dev, warmup=1, counts=(1, 2))
        assert gc.isenabled() == gc_on
    finally:
        gc.enable() if was else gc.disable()


def test_loop_graph_inside_an_open_guard(dev):
    """A LoopGraph built inside a capture_guard() (GraphedVictim's no-grad capture) takes its own list and leaves the
    outer guard open and intact: the outer list receives what is noted before, during the warm-up pass (which runs
    under the outer guard alone) and afterwards; the captured pass's tensors go to the LoopGraph's own list."""
    x, _ = _counter(dev)
    before, inner, after = (torch.ones(64, device=dev) for _ in range(3))

    def body():
        graphed.note_captured(inner)
        x.add_(inner)
    was = gc.isenabled()
    with graphed.capture_guard() as outer:
        graphed.note_captured(before)
        loop = graphed.LoopGraph(body, dev, warmup=1)
        assert graphed.capturing() and not gc.isenabled()
        graphed.note_captured(after)
        assert [id(t) for t in outer] == [id(before), id(inner), id(after)]
    assert [id(t) for t in loop.keep] == [id(inner)]
    assert not graphed.capturing() and gc.isenabled() == was
    loop.replay()
    assert torch.equal(x, torch.full_like(x, 2.0))


# -- DeviceLoop: one key's buffers, body and graphs. The body is x += 1 on one float. -------------------------------------
def test_device_loop_replay_equals_eager(dev):
    x = torch.zeros(1, device=dev)
    loop = graphed.DeviceLoop("k", dev, counts=(1, 16), warmup=2, body=lambda: x.add_(1), bufs=dict(x=x))
    assert loop.capture(rewind=lambda: x.zero_()) is True and float(x) == 0.0
    graphs = loop.graphs
    assert sorted(graphs.graphs) == [1, 16]
    x.fill_(5.0)
    assert loop.capture(rewind=lambda: x.zero_()) is False and loop.graphs is graphs and float(x) == 5.0
    y = torch.zeros(1, device=dev)
    twin = graphed.DeviceLoop("k", dev, counts=(1, 16), warmup=2, body=lambda: y.add_(1), bufs=dict(x=y))
    for n in (0, 1, 15, 16, 17, 33):
        x.zero_(), y.zero_()
        loop.run(n), twin.run(n)
        assert float(x) == n and float(y) == n and twin.graphs is None


def _knn_attack(dev):
    t = importlib.import_module("test_knn_loop_gpu")
    pcs = t._clouds(4, 3, 200)
    atk, _, _ = t._attack(t.hip_pointnet(0, dev)[0], pcs, torch.zeros(3, dtype=torch.long), num_iter=2, device_loop=True)
    assert atk.last_path == "device_loop"
    return atk, atk._loop_cache


def _eot_attack(dev):
    t = importlib.import_module("test_eot_device_rng_gpu")
    atk = t._make(dev, "B1_K64", True, binary_step=1, num_iter=2)
    t._attack(dev, "B1_K64", atk)
    assert atk.last_path == "device_loop"
    return atk, atk._loop_cache


def _iso_attack(dev):
    t = importlib.import_module("test_iso_gpu")
    fx = np.load(os.path.join(t.GOLDEN, "iso.npz"))
    victim, _ = t.hip_pointnet(int(fx["weights_seed"]), dev)
    atk = t._run(fx, "a_n64", victim, dev)[0]
    return atk, atk._ctri_cache


@pytest.mark.parametrize("make", [_knn_attack, _eot_attack, _iso_attack], ids=["cwknn", "eot_cw", "iso"])
def test_an_attacks_loop_dies_with_the_attack_without_the_cycle_collector(dev, make):
    """No reference cycle runs through a captured loop: dropping the attack frees it (and its graphs) by reference count,
    at once, not at whatever allocation wakes the cycle collector — which may be inside another capture."""
    atk, cache = make(dev)
    assert len(cache) == 1
    ref = weakref.ref(next(iter(cache.values())))
    assert ref().graphs is not None
    del cache
    torch.cuda.synchronize()
    was = gc.isenabled()
    gc.collect()
    gc.disable()
    try:
        assert ref() is not None
        del atk
        assert ref() is None
    finally:
        if was:
            gc.enable()
