"""GPU parity, no tolerances: the PointNet tower forward with layer 3 screened on bf16 MFMA and the survivors rechecked
exactly (the default of ops.pointmlp3_max_fwd_raw) against the exact fp32 kernel (exact=True). The screen only decides
WHICH (point, channel) pairs are recomputed; every value that leaves the kernel is the exact kernel's fmaf chain, so all
outputs must agree in every bit. NaNs are compared as positions (see test_pointmlp_bwd_balance_gpu.py).
The `stats` of the debug instantiation (candidates rechecked, channel blocks that ran the exact block instead) show that
a case passed THROUGH the screen and not around it."""
import importlib

import numpy as np
import pytest
import torch

from helpers import hip_pointnet

pytestmark = pytest.mark.gpu

TILE = 128


def _weights(dev, C3, seed):
    g = torch.Generator().manual_seed(seed)

    def u(*s, k):
        return ((torch.rand(*s, generator=g) * 2 - 1) / k ** 0.5).to(dev)
    return [u(64, 3, k=3), u(64, k=3), u(128, 64, k=64), u(128, k=64), u(C3, 128, k=128), u(C3, k=128)]


def _same_bits(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if not a.dtype.is_floating_point:
        return torch.equal(a, b)
    na, nb = torch.isnan(a).contiguous(), torch.isnan(b).contiguous()
    return torch.equal(na, nb) and torch.equal(a.contiguous().view(torch.int32)[~na], b.contiguous().view(torch.int32)[~nb])


def _flat(res):
    out = []
    for r in res:
        out.extend(r if isinstance(r, tuple) else [r])
    return out


def _run(ops, x, w, relu_last, exact, x_cf=True, **kw):
    """(part_val, part_idx[, T_out]) of fold=False and (pooled, argidx, mask1, mask2[, T_out]) of the folded launch."""
    a = ops.pointmlp3_max_fwd_raw(x, w, relu_last, x_cf=x_cf, fold=False, exact=exact, **kw)
    b = ops.pointmlp3_max_fwd_raw(x, w, relu_last, x_cf=x_cf, want_masks=True, exact=exact, **kw)
    return _flat(a) + _flat(b)


def _stats(ops, x, w, relu_last=False, **kw):
    dbg = {}
    ops.pointmlp3_max_fwd_raw(x, w, relu_last, fold=False, screen_dbg=dbg, **kw)
    return dbg["stats"].cpu().numpy().astype(np.int64)


def _assert_parity(ops, x, w, relu_last=False, x_cf=True, bitwise_nan=False, **kw):
    ex = _run(ops, x, w, relu_last, True, x_cf=x_cf, **kw)
    sc = _run(ops, x, w, relu_last, False, x_cf=x_cf, **kw)
    torch.cuda.synchronize()
    assert len(ex) == len(sc)
    for i, (e, s) in enumerate(zip(ex, sc)):
        if bitwise_nan:
            assert _same_bits(e, s), f"output {i} differs"
        else:
            assert torch.equal(e, s), f"output {i} differs"


SHAPES = [(2, 128, 1024), (3, 200, 256), (1, 1, 32), (1, 33, 64), (2, 1024, 1024), (1, 1500, 1024)]


@pytest.mark.parametrize("variant", ["plain", "T", "T_head"])
@pytest.mark.parametrize("B,N,C3", SHAPES)
def test_screened_equals_exact(ops, dev, B, N, C3, variant):
    torch.manual_seed(B * 100003 + N * 101 + C3)
    w = _weights(dev, C3, N + C3)
    x = torch.randn(B, 3, N, device=dev) * 0.5
    kw = {}
    if variant == "T":
        kw["T"] = torch.eye(3, device=dev)[None] + 0.3 * torch.randn(B, 3, 3, device=dev)
    elif variant == "T_head":
        K = 256
        kw["T_head"] = (torch.randn(B, K, device=dev), (torch.randn(9, K, device=dev) / K ** 0.5).contiguous(),
                        torch.eye(3, device=dev).reshape(9).contiguous())
    for relu_last in (False, True):
        _assert_parity(ops, x, w, relu_last, x_cf=True, **kw)
        _assert_parity(ops, x.transpose(1, 2).contiguous(), w, relu_last, x_cf=False, **kw)
    st = _stats(ops, x, w, **kw)
    ntiles = (N + TILE - 1) // TILE
    cand, fell = st[..., 0].sum(), st[..., 1].sum()
    print(f"[screen] B={B} N={N} C3={C3} {variant}: {cand / (B * ntiles * C3):.2f} candidates per (tile, channel), "
          f"{fell} of {B * ntiles * (C3 // 32)} channel blocks fell back")
    assert cand < 8 * B * ntiles * C3
    assert 32 * fell <= B * ntiles * (C3 // 32)
    assert cand >= B * ntiles * C3 - 32 * fell          # at least the winner of every screened (tile, channel)


def test_ties(ops, dev):
    """Exact ties and near-ties: the lowest index must win, whichever path a (tile, channel block) takes."""
    C3 = 256
    w = _weights(dev, C3, 5)
    g = torch.Generator().manual_seed(11)
    one = torch.randn(1, 3, 1, generator=g).to(dev) * 0.5
    # one point repeated: every value ties, point 0 of each tile wins
    x = one.expand(1, 3, 2 * TILE).contiguous()
    _assert_parity(ops, x, w)
    pv, pi = ops.pointmlp3_max_fwd_raw(x, w, False, fold=False)
    assert torch.equal(pi, (torch.arange(2, device=dev, dtype=torch.int32) * TILE)[None, :, None].expand(1, 2, C3))
    # each point duplicated at a higher index: the copy never wins
    half = torch.randn(2, 3, 64, generator=g).to(dev) * 0.5
    x = torch.cat([half, half], dim=2).contiguous()
    _assert_parity(ops, x, w)
    _, idx = ops.pointmlp3_max_fwd_raw(x, w, False)
    assert int(idx.max()) < 64
    st = _stats(ops, x, w)
    assert st[..., 0].sum() >= 2 * 2 * C3 - 64 * st[..., 1].sum()    # both copies of every screened winner were rechecked
    # one point plus 1e-7 jitter: hundreds of candidates per channel, more than a block's list holds
    x = (one + 1e-7 * torch.randn(1, 3, TILE, generator=g).to(dev)).contiguous()
    _assert_parity(ops, x, w)
    st = _stats(ops, x, w)
    print(f"[screen] jitter 1e-7: {st[..., 1].sum()} of {C3 // 32} channel blocks fell back, {st[..., 0].sum()} candidates rechecked")
    assert st[..., 1].sum() > 0


@pytest.mark.parametrize("case", ["nan_coord", "inf_coord", "huge_coord", "w3_nan", "w3_inf", "w3_tiny", "w3_huge",
                                  "all_negative"])
def test_non_finite_and_extreme(ops, dev, case):
    B, N, C3 = 2, 200, 256
    torch.manual_seed(7)
    w = _weights(dev, C3, 3)
    x = torch.randn(B, 3, N, device=dev) * 0.5
    relu_last = False
    ntiles = (N + TILE - 1) // TILE
    if case == "nan_coord":
        x[0, 1, 17] = float("nan")
    elif case == "inf_coord":
        x[1, 2, 150] = float("inf")
    elif case == "huge_coord":
        x[0, :, 5] = 1e30
        x[1, :, 140] = -1e30
    elif case == "w3_nan":
        w[4][37, 5] = float("nan")
    elif case == "w3_inf":
        w[4][200, 127] = float("-inf")
    elif case == "w3_tiny":
        w[4] = (w[4] * 1e-38).contiguous()
    elif case == "w3_huge":
        w[4] = (w[4] * 1e30).contiguous()
    elif case == "all_negative":
        w[5] = torch.full_like(w[5], -1e3)
        relu_last = True
    _assert_parity(ops, x, w, relu_last, bitwise_nan=True)
    _assert_parity(ops, x.transpose(1, 2).contiguous(), w, relu_last, x_cf=False, bitwise_nan=True)
    st = _stats(ops, x, w, relu_last)
    print(f"[screen] {case}: fell back {st[..., 1].tolist()} of {C3 // 32} blocks per tile, candidates {st[..., 0].tolist()}")
    if case in ("w3_nan", "w3_inf"):
        # the channel block that holds the non-finite row runs the exact block in every tile of every cloud
        assert (st[..., 1] >= 1).all()
    if case == "all_negative":
        pooled, _ = ops.pointmlp3_max_fwd_raw(x, w, True)
        assert float(pooled.abs().max()) == 0.0


def _host_h2(x, w, mask2):
    """h2 [B,N,128] in float64 from the launch's inputs, with the kernel's own layer-2 ReLU decisions (mask2): the fp32 h2
    the kernel holds differs from it by a few ulps (1e-7 relative), four orders below the bound under test."""
    W1, b1, W2, b2 = (t.double().cpu() for t in w[:4])
    p = x.double().cpu().transpose(1, 2)                                  # [B,N,3]
    h1 = torch.relu(p @ W1.t() + b1)
    pre = h1 @ W2.t() + b2
    bits = (mask2.cpu().to(torch.int64)[..., None] >> torch.arange(32)) & 1        # [B,N,4,32]
    on = bits.reshape(mask2.shape[0], mask2.shape[1], 128).bool()
    return torch.where(on, pre, torch.zeros_like(pre))


@pytest.mark.parametrize("B,N,C3", [(1, 128, 64), (1, 200, 1024)])
def test_bound_holds_on_the_hardware(ops, dev, B, N, C3):
    """|v - S| <= E for every (point, channel): S and E as the kernel formed them, v the exact product in float64. The
    printed ratio is the check of what pointmlp_screen_bound.h allows for the MFMA's undocumented accumulation."""
    torch.manual_seed(N + C3)
    w = _weights(dev, C3, 21)
    x = torch.randn(B, 3, N, device=dev) * 0.5
    dbg = {"dump": True}
    _, _, masks = ops.pointmlp3_max_fwd_raw(x, w, False, want_masks=True, screen_dbg=dbg)
    torch.cuda.synchronize()
    assert int(dbg["stats"][..., 1].sum()) == 0                           # every block went through the screen
    S, E = dbg["S"].double().cpu(), dbg["E"].double().cpu()
    assert torch.isfinite(S).all() and torch.isfinite(E).all()
    v = _host_h2(x, w, masks[1]) @ w[4].double().cpu().t()
    ratio = ((v - S).abs() / E).max().item()
    print(f"[screen] N={N} C3={C3}: max |v - S| / E = {ratio:.4f}")
    assert ((v - S).abs() <= E).all()


def test_capture_and_new_weights(ops, dev):
    """Captured and replayed; then the victim gets other weights: the screen follows them (its bf16 operands are made
    from the fp32 rows inside every launch, nothing is cached), and the old graph still replays its old result."""
    graphed = importlib.import_module("3dpointcloudattack_amd.graphed")
    pn = importlib.import_module("3dpointcloudattack_amd.model.pointnet")
    ort = importlib.import_module("oracle.ref_torch")
    model, _ = hip_pointnet(3, dev)
    torch.manual_seed(5)
    x = torch.randn(4, 3, 300, device=dev) * 0.5

    def run(exact=False):
        pk = pn.fused_pack(model)
        return ops.pointmlp3_max_fwd_raw(x, pk["tower_s"], True, want_masks=True, exact=exact), pk

    eager, _ = run()
    eager = [t.clone() for t in _flat(eager)]
    for e, s in zip(eager, _flat(run(exact=True)[0])):
        assert torch.equal(e, s)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with graphed.capture_guard() as keep:
        with torch.cuda.graph(graph):
            out, pk_old = run()
    out = _flat(out)
    for _ in range(2):
        for t in out:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for e, s in zip(eager, out):
            assert torch.equal(e, s)
    model.load_state_dict(ort.seeded_state_dict(model, 4))
    new = _flat(run()[0])
    for e, s in zip(_flat(run(exact=True)[0]), new):
        assert torch.equal(e, s)
    assert not torch.equal(new[0], eager[0])
    for t in out:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for e, s in zip(eager, out):
        assert torch.equal(e, s)
    del keep, pk_old
