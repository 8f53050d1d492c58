"""GPU parity, no tolerances: the screened PointNet tower forward fed from the PREPARED image of W3 (bf16 hi / lo operands
in MFMA order, row norms, a k-group-major fp32 copy for a recheck that goes by channel; csrc/pointmlp_screen.hip) against
the exact fp32 kernel and against the in-launch form that makes the same operands from W3 inside every launch. The
tests pass the image's holder explicitly: weights + [W2T, pack], pack a plain list that the first launch fills."""
import importlib

import numpy as np
import pytest
import torch

from helpers import hip_pointnet

pytestmark = pytest.mark.gpu

TILE = 128
PCAP = 8        # PMS_PCAP: candidates per (tile, channel) before the channel's block runs the exact block


def _weights(dev, C3, seed):
    g = torch.Generator().manual_seed(seed)

    def u(*s, k):
        return ((torch.rand(*s, generator=g) * 2 - 1) / k ** 0.5).to(dev)
    return [u(64, 3, k=3), u(64, k=3), u(128, 64, k=64), u(128, k=64), u(C3, 128, k=128), u(C3, k=128)]


def _packed(w):
    """The tower as the model folds it: the six tensors, W2^T and an empty list for the prepared image."""
    return list(w[:6]) + [w[2].t().contiguous(), []]


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


def _run(ops, x, w, relu_last, x_cf=True, **kw):
    """(part_val, part_idx[, T_out]) of fold=False and (pooled, argidx, mask1, mask2[, T_out]) of the folded launch."""
    a = ops.pointmlp3_max_fwd_raw(x, w, relu_last, x_cf=x_cf, fold=False, **kw)
    b = ops.pointmlp3_max_fwd_raw(x, w, relu_last, x_cf=x_cf, want_masks=True, **kw)
    return _flat(a) + _flat(b)


def _dbg(ops, x, w, relu_last=False, dump=False, **kw):
    dbg = {"dump": True} if dump else {}
    ops.pointmlp3_max_fwd_raw(x, w, relu_last, fold=False, screen_dbg=dbg, **kw)
    return dbg


def _stats(ops, x, w, relu_last=False, **kw):
    return _dbg(ops, x, w, relu_last, **kw)["stats"].cpu().numpy().astype(np.int64)


def _assert_same(ref, got, what, bitwise_nan=False):
    assert len(ref) == len(got)
    for i, (e, s) in enumerate(zip(ref, got)):
        assert (_same_bits(e, s) if bitwise_nan else torch.equal(e, s)), f"{what}: output {i} differs"


def _assert_parity(ops, x, wp, relu_last=False, x_cf=True, bitwise_nan=False, **kw):
    """prepared == exact and prepared == in-launch, all outputs; the pack must have been used (filled, key matching)."""
    pr = _run(ops, x, wp, relu_last, x_cf=x_cf, **kw)
    assert len(wp[7]) == 4 and wp[7][3] == (wp[4].data_ptr(), wp[4]._version)
    ex = _run(ops, x, wp, relu_last, x_cf=x_cf, exact=True, **kw)
    il = _run(ops, x, wp, relu_last, x_cf=x_cf, in_launch=True, **kw)
    torch.cuda.synchronize()
    _assert_same(ex, pr, "prepared vs exact", bitwise_nan)
    _assert_same(il, pr, "prepared vs in-launch", bitwise_nan)


# C3: 32 one block, seven idle waves; 64 both halves of one recheck trip; 96 a half-empty trip; 288 wave 0 has two
# slots, the others one; 1024 the victim's. N: one point, a ragged tile, a full tile, two tiles with a ragged second.
@pytest.mark.parametrize("variant", ["plain", "T", "T_head"])
@pytest.mark.parametrize("N", [1, 33, 128, 200])
@pytest.mark.parametrize("C3", [32, 64, 96, 288, 1024])
def test_prepared_equals_exact_and_in_launch(ops, dev, N, C3, variant):
    B = 1 + (N + C3 // 32) % 3
    torch.manual_seed(B * 100003 + N * 101 + C3)
    wp = _packed(_weights(dev, C3, N + C3))
    x = torch.randn(B, 3, N, device=dev) * 0.5
    kw = {}
    if variant == "T":
        kw["T"] = torch.eye(3, device=dev)[None] + 0.3 * torch.randn(B, 3, 3, device=dev)
    elif variant == "T_head":
        K = 256
        kw["T_head"] = (torch.randn(B, K, device=dev), (torch.randn(9, K, device=dev) / K ** 0.5).contiguous(),
                        torch.eye(3, device=dev).reshape(9).contiguous())
    for relu_last in (False, True):
        _assert_parity(ops, x, wp, relu_last, x_cf=True, **kw)
        _assert_parity(ops, x.transpose(1, 2).contiguous(), wp, relu_last, x_cf=False, **kw)
    dp = _dbg(ops, x, wp, dump=True, **kw)
    di = _dbg(ops, x, wp, dump=True, in_launch=True, **kw)
    torch.cuda.synchronize()
    assert _same_bits(dp["S"], di["S"]) and _same_bits(dp["E"], di["E"])      # NaN = not written (no such point)
    assert torch.equal(dp["stats"][..., 0], di["stats"][..., 0])
    assert int(dp["stats"][..., 1].abs().sum()) == 0
    assert int(dp["stats"][..., 0].sum()) >= B * ((N + TILE - 1) // TILE) * C3


def test_pack_against_torch(ops, dev):
    """The three arrays of the image, restated: hi = bf16(x), lo = bf16(x - hi) in the order the header documents."""
    C3 = 288
    g = torch.Generator().manual_seed(77)
    W3 = torch.randn(C3, 128, generator=g)
    W3[3] *= 1e-20
    W3[40] *= 1e10
    W3[41] = 0.0
    W3[100, ::3] = 0.0
    W3 = W3.to(dev).contiguous()
    bf, nw, q = ops.pointmlp3_w3_prepare(W3)
    torch.cuda.synchronize()
    hi = W3.to(torch.bfloat16)
    lo = (W3 - hi.float()).to(torch.bfloat16)

    def order(t):   # [C3,128] -> [block, k-step, lane r + 32 h, 8]: W3[32 cb + r][16 t + 8 h + i]
        return t.view(C3 // 32, 32, 8, 2, 8).permute(0, 2, 3, 1, 4).reshape(C3 // 32, 8, 64, 8).contiguous()
    assert bf.shape == (C3 // 32, 8, 2, 64, 8) and bf.dtype == torch.bfloat16
    assert torch.equal(bf[:, :, 0].contiguous().view(torch.int16), order(hi).view(torch.int16))
    assert torch.equal(bf[:, :, 1].contiguous().view(torch.int16), order(lo).view(torch.int16))
    assert q.shape == (32, C3, 4)
    assert torch.equal(q.permute(1, 0, 2).reshape(C3, 128), W3)              # w3_q[t][c] = W3[c][4t..4t+3]
    assert torch.isfinite(nw).all()
    assert (nw.double() >= W3.double().norm(dim=1)).all()


def test_channel_cap_edge_and_ties(ops, dev):
    """PCAP equal candidates in every channel fill the slots exactly; one more and every block runs the exact block.
    The lowest index wins on either path. Then the duplicated-half and the 1e-7-jitter clouds of test_ties."""
    C3 = 256
    w = _weights(dev, C3, 5)
    g = torch.Generator().manual_seed(11)
    one = torch.randn(1, 3, 1, generator=g).to(dev) * 0.5
    for n, fell in ((PCAP, 0), (PCAP + 1, C3 // 32)):
        wp = _packed(w)
        x = one.expand(1, 3, n).contiguous()
        _assert_parity(ops, x, wp)
        _, pi = ops.pointmlp3_max_fwd_raw(x, wp, False, fold=False)
        assert int(pi.abs().max()) == 0
        st = _stats(ops, x, wp)
        assert st[..., 1].sum() == fell
        assert st[..., 0].sum() == (C3 * PCAP if fell == 0 else 0)
    wp = _packed(w)
    half = torch.randn(2, 3, 64, generator=g).to(dev) * 0.5
    x = torch.cat([half, half], dim=2).contiguous()
    _assert_parity(ops, x, wp)
    _, idx = ops.pointmlp3_max_fwd_raw(x, wp, False)
    assert int(idx.max()) < 64
    st = _stats(ops, x, wp)
    assert st[..., 0].sum() >= 2 * 2 * C3 - 64 * st[..., 1].sum()    # both copies of every screened winner were rechecked
    x = (one + 1e-7 * torch.randn(1, 3, TILE, generator=g).to(dev)).contiguous()
    _assert_parity(ops, x, wp)
    st = _stats(ops, x, wp)
    print(f"[prepared] jitter 1e-7: {st[..., 1].sum()} of {C3 // 32} channel blocks fell back, {st[..., 0].sum()} candidates rechecked")
    assert st[..., 1].sum() > 0


@pytest.mark.parametrize("case", ["nan_coord", "inf_coord", "huge_coord", "w3_nan", "w3_inf", "w3_tiny", "w3_huge",
                                  "all_negative"])
def test_non_finite_and_extreme(ops, dev, case):
    B, N, C3 = 2, 200, 256
    torch.manual_seed(7)
    w = _weights(dev, C3, 3)
    x = torch.randn(B, 3, N, device=dev) * 0.5
    relu_last = False
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
    wp = _packed(w)                       # the image is made from the edited weights
    _assert_parity(ops, x, wp, relu_last, bitwise_nan=True)
    _assert_parity(ops, x.transpose(1, 2).contiguous(), wp, relu_last, x_cf=False, bitwise_nan=True)
    st = _stats(ops, x, wp, relu_last)
    print(f"[prepared] {case}: fell back {st[..., 1].tolist()} of {C3 // 32} blocks per tile, candidates {st[..., 0].tolist()}")
    if case in ("w3_nan", "w3_inf"):
        assert (st[..., 1] >= 1).all()
    if case == "all_negative":
        pooled, _ = ops.pointmlp3_max_fwd_raw(x, wp, True)
        assert float(pooled.abs().max()) == 0.0


def test_stale_image_is_not_read(ops, dev):
    """W3 written in place after the image was made: the key (storage, version) no longer matches, the launch makes its
    operands from the new W3 itself, and the list is left as it was."""
    B, N, C3 = 2, 200, 288
    torch.manual_seed(3)
    wp = _packed(_weights(dev, C3, 9))
    x = torch.randn(B, 3, N, device=dev) * 0.5
    before = _run(ops, x, wp, False)
    pack = wp[7]
    held = list(pack)
    assert len(held) == 4
    wp[4].mul_(-1.5)
    wp[4][5, 7] = 3.0
    after = _run(ops, x, wp, False)
    _assert_same(_run(ops, x, wp, False, exact=True), after, "after the in-place write vs exact")
    assert not torch.equal(before[0], after[0])
    assert wp[7] is pack and len(pack) == 4 and all(a is b for a, b in zip(pack, held))
    assert pack[3] != (wp[4].data_ptr(), wp[4]._version)


def test_capture_on_the_model_path(ops, dev):
    graphed = importlib.import_module("3dpointcloudattack_amd.graphed")
    pn = importlib.import_module("3dpointcloudattack_amd.model.pointnet")
    ort = importlib.import_module("oracle.ref_torch")
    torch.manual_seed(5)
    x = torch.randn(4, 3, 300, device=dev) * 0.5

    def run(model, **kw):
        pk = pn.fused_pack(model)
        return ops.pointmlp3_max_fwd_raw(x, pk["tower_s"], True, want_masks=True, **kw), pk

    def replay_equals(graph, out, ref):
        for t in out:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for e, s in zip(ref, out):
            assert torch.equal(e, s)

    def capture(model):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            run(model, in_launch=True)    # the in-launch instantiation's first use is not inside the capture
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with graphed.capture_guard() as keep:
            with torch.cuda.graph(graph):
                out, pk = run(model)
        return graph, _flat(out), pk, keep

    # the first call that could fill the list falls into a capture: the in-launch form, and the list stays empty
    model, _ = hip_pointnet(3, dev)
    ref = [t.clone() for t in _flat(run(model, exact=True)[0])]
    assert pn.fused_pack(model)["tower_s"][7] == []
    graph0, out0, pk0, keep0 = capture(model)
    assert pk0["tower_s"][7] == []
    replay_equals(graph0, out0, ref)

    # the normal order: eager (fills the list), capture, replays, new weights
    model, _ = hip_pointnet(3, dev)
    eager, pk = run(model)
    eager = [t.clone() for t in _flat(eager)]
    pack = pk["tower_s"][7]
    assert len(pack) == 4
    _assert_same(ref, eager, "eager prepared vs exact")
    graph, out, pk_old, keep = capture(model)
    assert pk_old["tower_s"][7] is pack and len(pack) == 4
    cached = {id(t) for t in graphed._cached_tensors(model)}
    assert all(id(t) in cached for t in pack[:3])
    for _ in range(2):
        replay_equals(graph, out, eager)
    model.load_state_dict(ort.seeded_state_dict(model, 4))
    new, pk_new = run(model)
    new = _flat(new)
    assert pk_new["tower_s"][7] is not pack and len(pk_new["tower_s"][7]) == 4
    _assert_same(_flat(run(model, exact=True)[0]), new, "new weights: prepared vs exact")
    assert not torch.equal(new[0], eager[0])
    replay_equals(graph, out, eager)
    assert len(pack) == 4
    del keep, pk_old, keep0, pk0
