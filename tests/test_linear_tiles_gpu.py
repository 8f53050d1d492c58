"""GPU parity, no tolerances: every tile form of the small-batch linear kernel (32x16, 16x16, 16x8, 8x8; include/pc3d.h)
computes the bits of the forced 32x16 form — NaN positions included — through all four entries that take the tile:
ops.linear, ops.linear_nn (layer + search), ops.linear_book (layer + bookkeeping) and ops.linear_pre.

Why it must hold: an output element depends on its own row of X and its own row of W only, and neither the k order,
nor the chunk -> wave assignment, nor the order in which the eight waves' partial sums are added depends on the tile."""
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu
ops = importlib.import_module("3dpointcloudattack_amd.ops")

REF = "32x16"
FORMS = ("16x16", "16x8", "8x8")


def _same(a, b):
    """torch.equal with NaNs compared by position."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if not a.is_floating_point():
        return torch.equal(a, b)
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(a[~na], b[~nb])


def _layer(dev, B, K, O, seed=0):
    g = torch.Generator().manual_seed(seed * 7919 + 3 * B + 5 * K + 7 * O)
    X = torch.randn(B, K, generator=g).to(dev)
    W = (torch.randn(O, K, generator=g) / K ** 0.5).to(dev)
    bias = torch.randn(O, generator=g).to(dev)
    gate = torch.randn(B, O, generator=g).to(dev)
    return X, W, bias, gate


def _epilogues(dev, X, W, bias, gate):
    """(name, kwargs) of the epilogue variants; the last one reads X and writes Y through row strides larger than the row."""
    B, K = X.shape
    O = W.shape[0]
    Xs = torch.full((B, K + 8), 7.0, device=dev)
    Xs[:, :K] = X
    return [("plain", dict(X=X)),
            ("bias+leaky", dict(X=X, bias=bias, relu=True, slope=0.2)),
            ("gate", dict(X=X, gate=gate, gate_slope=0.25)),
            ("all+strided", dict(X=Xs[:, :K], bias=bias, relu=True, slope=0.0, gate=gate, gate_slope=0.5, strided_out=O + 5))]


def _run_linear(dev, W, tile, X, strided_out=None, **kw):
    if strided_out is None:
        return ops.linear(X, W, tile=tile, **kw), None
    buf = torch.full((X.shape[0], strided_out), -3.0, device=dev)
    Y = ops.linear(X, W, out=buf[:, :W.shape[0]], tile=tile, **kw)
    return Y, buf


# K: one chunk; one chunk per wave; wave 0 holding two chunks; the upper limit of the tiled kernel
@pytest.mark.parametrize("K", [16, 128, 144, 1024])
@pytest.mark.parametrize("O", [64, 72, 520])
@pytest.mark.parametrize("B", [1, 15, 16, 17, 32, 33])
def test_linear_tile_forms_same_bits(dev, B, O, K):
    X, W, bias, gate = _layer(dev, B, K, O)
    for name, kw in _epilogues(dev, X, W, bias, gate):
        Y0, buf0 = _run_linear(dev, W, REF, **kw)
        Yr, _ = _run_linear(dev, W, None, **kw)                     # the rule picks one of the forms
        assert torch.equal(Yr, Y0), (name, "rule")
        for form in FORMS:
            Y1, buf1 = _run_linear(dev, W, form, **kw)
            assert torch.equal(Y1, Y0), (name, form)
            if buf0 is not None:                                    # nothing written between the rows
                assert torch.equal(buf1, buf0), (name, form)
    # the layer itself is right: the worst-case bound of a K-term fp32 dot product in any order, K u sum |x||w| with
    # u = 2^-24, doubled for the rounding of the products
    Xd, Wd = X.double(), W.double()
    bound = K * 2.0 ** -23 * (Xd.abs() @ Wd.abs().t())
    assert bool(((ops.linear(X, W, tile=REF).double() - Xd @ Wd.t()).abs() <= bound).all())


def test_linear_tile_forms_nan_inf_stay_in_their_row_and_column(dev):
    B, K, O = 33, 144, 72
    X, W, bias, gate = _layer(dev, B, K, O, seed=1)
    clean = ops.linear(X, W, bias, tile=REF)
    X[9, 5], X[9, 77], X[9, 130] = float("nan"), float("inf"), float("-inf")
    W[21, 0], W[21, 64], W[21, 143] = float("inf"), float("nan"), float("-inf")
    Y0 = ops.linear(X, W, bias, tile=REF)
    keep = torch.ones(B, O, dtype=torch.bool, device=dev)
    keep[9, :] = False
    keep[:, 21] = False
    assert torch.equal(Y0[keep], clean[keep])                       # no other row or column changes
    assert not bool(torch.isfinite(Y0[9]).any()) and not bool(torch.isfinite(Y0[:, 21]).any())
    for form in FORMS:
        for kw in (dict(), dict(relu=True, slope=0.1), dict(gate=gate, gate_slope=0.3)):
            assert _same(ops.linear(X, W, bias, tile=form, **kw), ops.linear(X, W, bias, tile=REF, **kw)), (form, kw)


def test_linear_tile_argument_is_checked(dev):
    X, W, _, _ = _layer(dev, 4, 64, 64)
    with pytest.raises(ValueError):
        ops.linear(X, W, tile="64x64")
    assert ops.linear_tile(32, 1024, 512) in ops.LINEAR_TILES
    # a shape outside the tiled kernel (K % 16 != 0) has one form: the argument changes nothing
    X2, W2, _, _ = _layer(dev, 4, 40, 64)
    assert torch.equal(ops.linear(X2, W2, tile="8x8"), ops.linear(X2, W2))


# ---------------------------------------------------------------------------------------------------------------
# the riders and the pre-layer
# ---------------------------------------------------------------------------------------------------------------
def _nn_inputs(dev, B, N, M, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, 3, N, generator=g) - 0.5).to(dev), (torch.rand(B, 3, M, generator=g) - 0.5).to(dev)


# N = M = 64: the search on its four-wave form, outside the rider's range, i.e. two launches with the tiled layer;
# N = 1024 / 700: one launch; K = 200: the layer outside the tiled kernel, two launches and one form
@pytest.mark.parametrize("B,K,O,N", [(5, 256, 200, 64), (32, 1024, 512, 64), (32, 1024, 512, 1024), (17, 144, 72, 700),
                                     (8, 200, 512, 1024)])
def test_linear_nn_tile_forms_same_bits(dev, B, K, O, N):
    X, W, bias, gate = _layer(dev, B, K, O, seed=2)
    q, r = _nn_inputs(dev, B, N, N, seed=N + B)
    kw = dict(relu=True, gate=gate, gate_slope=0.5, q=q, r=r, q_cf=True, r_cf=True)
    Y0, d0, i0 = ops.linear_nn(X, W, bias, tile=REF, **kw)
    da, ia = ops.nn_raw(q, r, True, True)
    assert torch.equal(d0, da) and torch.equal(i0, ia)
    for form in FORMS + (None,):
        Y1, d1, i1 = ops.linear_nn(X, W, bias, tile=form, **kw)
        assert torch.equal(Y1, Y0) and torch.equal(d1, d0) and torch.equal(i1, i0), form


def _book_state(dev, B, NK, seed):
    g = torch.Generator().manual_seed(seed)
    ori = (torch.rand(B, 3, NK, generator=g) - 0.5).to(dev)
    adv = ori + (torch.randn(B, 3, NK, generator=g) * 0.01).to(dev)
    label = torch.randint(0, 40, (B,), generator=g).to(dev)
    pred = label.clone()
    differs = torch.arange(B, device=dev) % 3 != 2
    pred[differs] = (pred[differs] + 1) % 40
    dist = torch.sqrt(((adv - ori) ** 2).sum((1, 2)))
    sel = torch.arange(B, device=dev)
    return dict(adv=adv, ori=ori, pred=pred, label=label,
                bestdist=torch.where(sel % 2 == 0, dist * 2, dist * 0.5).contiguous(), bestscore=torch.full((B,), -1, device=dev),
                o_bestdist=torch.where(sel % 4 < 2, dist * 2, dist * 0.5).contiguous(),
                o_bestscore=torch.full((B,), -1, device=dev), o_bestattack=torch.zeros(B, 3, NK, device=dev),
                input_val=torch.zeros(B, 3, NK, device=dev), dist_val=torch.zeros(B, device=dev))


_BOOK_OUT = ("bestdist", "bestscore", "o_bestdist", "o_bestscore", "o_bestattack", "input_val", "dist_val")


def _run_book(dev, X, W, gate, st, tile):
    s = {k: v.clone() for k, v in st.items()}
    adam = torch.zeros(2, device=dev)
    step = torch.full((1,), 3, dtype=torch.int32, device=dev)
    Y = ops.linear_book(X, W, s["adv"], s["ori"], s["pred"], s["label"], True, s["bestdist"], s["bestscore"], s["o_bestdist"],
                        s["o_bestscore"], s["o_bestattack"], gate=gate, input_val=s["input_val"], dist_val=s["dist_val"],
                        step=step, lr=0.01, adam=adam, tile=tile)
    return Y, s, adam


@pytest.mark.parametrize("B,K,O,NK", [(12, 256, 512, 333), (33, 144, 72, 1024)])
def test_linear_book_tile_forms_same_bits(dev, B, K, O, NK):
    X, W, _, gate = _layer(dev, B, K, O, seed=3)
    st = _book_state(dev, B, NK, seed=NK)
    Y0, s0, adam0 = _run_book(dev, X, W, gate, st, REF)
    assert 0 < int((s0["o_bestscore"] != -1).sum()) < B            # improving and non-improving samples are both there
    assert float(adam0[0]) > 0.01 and 0 < float(adam0[1]) < 1
    for form in FORMS + (None,):
        Y1, s1, adam1 = _run_book(dev, X, W, gate, st, form)
        assert torch.equal(Y1, Y0) and torch.equal(adam1, adam0), form
        for k in _BOOK_OUT:
            assert torch.equal(s1[k], s0[k]), (form, k)


def _pre_inputs(dev, B, P, K, O, J=9):
    g = torch.Generator().manual_seed(B + 3 * P + K)
    return (torch.randn(B, P, 16, generator=g).to(dev), J, torch.randn(J, K, generator=g).to(dev),
            torch.randn(B, K, generator=g).to(dev), (torch.randn(O, K, generator=g) / K ** 0.5).to(dev),
            torch.randn(B, O, generator=g).to(dev))


@pytest.mark.parametrize("P", [1, 8, 32])
@pytest.mark.parametrize("B,K,O", [(32, 256, 512), (17, 144, 72), (5, 16, 9)])
def test_linear_pre_tile_forms_same_bits(dev, B, K, O, P):
    parts, J, Wp, gate_pre, W, gate = _pre_inputs(dev, B, P, K, O)
    for gt in (gate, None):
        Y0 = ops.linear_pre(parts, J, Wp, gate_pre, W, gate=gt, tile=REF)
        for form in FORMS + (None,):
            assert torch.equal(ops.linear_pre(parts, J, Wp, gate_pre, W, gate=gt, tile=form), Y0), form
    S = parts.double().sum(1)[:, :J]
    Xd = torch.where(gate_pre > 0, S @ Wp.double(), torch.zeros((), dtype=torch.float64, device=dev))
    torch.testing.assert_close(ops.linear_pre(parts, J, Wp, gate_pre, W, tile=REF).double(), Xd @ W.double().t(),
                               rtol=1e-4, atol=1e-4)


def test_tile_forms_in_a_captured_graph_replayed_twice(dev):
    """Each entry in each form captured into one graph; both replays give the eager 32x16 bits."""
    B, K, O, N = 17, 144, 72, 700
    X, W, bias, gate = _layer(dev, B, K, O, seed=4)
    q, r = _nn_inputs(dev, B, N, N, seed=9)
    st = _book_state(dev, B, 333, seed=10)
    parts, J, Wp, gate_pre, Wq, gateq = _pre_inputs(dev, B, 8, K, O)
    eager = (ops.linear(X, W, bias, relu=True, tile=REF), ops.linear_nn(X, W, bias, q=q, r=r, q_cf=True, r_cf=True, tile=REF),
             _run_book(dev, X, W, gate, st, REF), ops.linear_pre(parts, J, Wp, gate_pre, Wq, gate=gateq, tile=REF))
    torch.cuda.synchronize()
    for form in FORMS:
        s = {k: v.clone() for k, v in st.items()}
        adam = torch.zeros(2, device=dev)
        step = torch.full((1,), 3, dtype=torch.int32, device=dev)
        out = {}

        def body():
            out["lin"] = ops.linear(X, W, bias, relu=True, tile=form)
            out["nn"] = ops.linear_nn(X, W, bias, q=q, r=r, q_cf=True, r_cf=True, tile=form)
            out["book"] = ops.linear_book(X, W, s["adv"], s["ori"], s["pred"], s["label"], True, s["bestdist"], s["bestscore"],
                                          s["o_bestdist"], s["o_bestscore"], s["o_bestattack"], gate=gate,
                                          input_val=s["input_val"], dist_val=s["dist_val"], step=step, lr=0.01, adam=adam,
                                          tile=form)
            out["pre"] = ops.linear_pre(parts, J, Wp, gate_pre, Wq, gate=gateq, tile=form)

        side = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                body()
        for _ in range(2):
            for k, v in st.items():                                 # the bookkeeping's state back to its start
                s[k].copy_(v)
            for t in (out["lin"], out["nn"][0], out["nn"][1], out["book"], out["pre"]):
                t.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out["lin"], eager[0]), form
            assert all(torch.equal(u, v) for u, v in zip(out["nn"], eager[1])), form
            assert torch.equal(out["book"], eager[2][0]) and torch.equal(adam, eager[2][2]), form
            for k in _BOOK_OUT:
                assert torch.equal(s[k], eager[2][1][k]), (form, k)
            assert torch.equal(out["pre"], eager[3]), form
