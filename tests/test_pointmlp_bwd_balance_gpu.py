"""GPU parity, no tolerances: the balanced tower backward (pc3d_pointmlp3_max_bwd_f32: hits sorted by point, whole
points shared out over the four waves, rows accumulated in registers) against the two-list kernel it replaced
(the same entry's PC3D_PM_BWD_TWOLIST form). Both form every point's row by the same fma chain in ascending channel order, so
gx and part_gT must agree in every bit: they are compared as int32 words, which also pins the sign of zero and of
infinity. The one thing left open is WHICH NaN a NaN is: a NaN must sit where the other kernel has a NaN, but its sign
and payload may differ (x + y of two NaNs returns the payload of whichever operand the compiler put first; torch.equal
itself is false for any NaN, two runs of one kernel included).
The raw op takes argidx, g and the masks as inputs, so the hit distribution is whatever a case says."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _weights(dev, C3, seed):
    g = torch.Generator().manual_seed(seed)

    def u(*s, k):
        return ((torch.rand(*s, generator=g) * 2 - 1) / k ** 0.5).to(dev)
    w = (u(64, 3, k=3), u(64, k=3), u(128, 64, k=64), u(128, k=64), u(C3, 128, k=128), u(C3, k=128))
    return w + (w[2].t().contiguous(),)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    if a.shape != b.shape:
        return False
    na, nb = torch.isnan(a).contiguous(), torch.isnan(b).contiguous()
    return torch.equal(na, nb) and torch.equal(_bits(a)[~na], _bits(b)[~nb])


def _argidx(kind, B, N, C3, natural, dev):
    c = torch.arange(C3, device=dev, dtype=torch.int64)
    tile0 = 32 * ((N // 32) // 2)                         # a full tile when N >= 64, else tile 0
    if kind == "natural":
        return natural
    if kind == "one_point":                               # all C3 channels on one point
        idx = torch.full((C3,), min(tile0 + 21, N - 1), device=dev, dtype=torch.int64)
    elif kind == "one_tile":                              # all channels in one tile, split over both halves
        idx = (tile0 + c % 32).clamp(max=N - 1)
    elif kind == "one_half":                              # all channels in the upper half of one tile
        idx = (tile0 + 16 + c % 16).clamp(max=N - 1)
    elif kind == "one_per_point":                         # one hit per point (as far as the channels reach)
        idx = c % N
    elif kind == "skewed":                                # one point owns most of a tile's hits, the rest are spread
        idx = torch.where(c % 3 == 0, (c * 7) % N, torch.full_like(c, min(tile0 + 5, N - 1)))
    else:
        raise AssertionError(kind)
    return idx.to(torch.int32)[None, :].expand(B, C3).contiguous()


def _case(ops, dev, B, N, C3, kind="natural", g_kind="randn", seed=0):
    torch.manual_seed(1000 * seed + N + C3)
    x = torch.randn(B, 3, N, device=dev) * 0.5
    T = torch.randn(B, 3, 3, device=dev) * 0.5
    w = _weights(dev, C3, seed + 1)
    pooled, natural, masks = ops.pointmlp3_max_fwd_raw(x, w, False, T=T, want_masks=True)
    g = torch.randn(B, C3, device=dev)
    if g_kind == "zero":                                  # no hit at all
        g = torch.zeros_like(g)
    elif g_kind == "special":                             # +0, -0, NaN, +-inf among ordinary values
        sel = torch.arange(C3, device=dev) % 7
        g[:, sel == 1] = 0.0
        g[:, sel == 2] = -0.0
        g[:, sel == 3] = float("nan")
        g[:, sel == 4] = float("inf")
        g[:, sel == 5] = float("-inf")
    return x, T, w, _argidx(kind, B, N, C3, natural, dev), g, masks


def _both(ops, x, w, idx, g, masks, T=None, want_gT=False, accumulate=False, x_cf=True, init=None):
    res = []
    for twolist in (False, True):
        out = None
        if init is not None:                              # a fresh buffer with init's strides (gaps included) and values
            out = torch.empty_strided(init.shape, init.stride(), dtype=init.dtype, device=init.device).copy_(init)
        r = ops.pointmlp3_max_bwd_raw(x, w, idx, g, masks, T=T, x_cf=x_cf, out=out, accumulate=accumulate,
                                      want_gT=want_gT, twolist=twolist)
        res.append(r if want_gT else (r, None))
    (gx_new, gt_new), (gx_old, gt_old) = res
    assert _same_bits(gx_new, gx_old), "gx differs from the two-list kernel"
    if want_gT:
        assert _same_bits(gt_new, gt_old), "part_gT differs from the two-list kernel"
    return gx_new, gt_new


KINDS = ["natural", "one_point", "one_tile", "one_half", "one_per_point", "skewed"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N", [33, 1000, 1024, 4096])
@pytest.mark.parametrize("C3", [32, 256, 1024])
def test_hit_distributions(ops, dev, kind, N, C3):
    B = 2 if N == 4096 else 3
    x, T, w, idx, g, masks = _case(ops, dev, B, N, C3, kind)
    _both(ops, x, w, idx, g, masks)                                   # no T, no part_gT
    _both(ops, x, w, idx, g, masks, T=T, want_gT=True)                # the trunk's launch
    _both(ops, x, w, idx, g, masks, T=T)                              # T without part_gT


@pytest.mark.parametrize("kind", ["natural", "one_point", "one_tile", "skewed"])
@pytest.mark.parametrize("g_kind", ["zero", "special"])
@pytest.mark.parametrize("N,C3", [(33, 32), (1000, 256), (1024, 1024)])
def test_zero_and_non_finite_gradients(ops, dev, kind, g_kind, N, C3):
    x, T, w, idx, g, masks = _case(ops, dev, 2, N, C3, kind, g_kind)
    gx, gt = _both(ops, x, w, idx, g, masks, T=T, want_gT=True)
    if g_kind == "zero":
        assert not gx.any() and not gt.any()
    _both(ops, x, w, idx, g, masks, accumulate=True, init=torch.randn_like(x))


@pytest.mark.parametrize("kind", ["natural", "one_half", "skewed"])
@pytest.mark.parametrize("N,C3", [(33, 256), (1000, 1024), (1024, 1024), (4096, 1024)])
@pytest.mark.parametrize("with_T", [False, True])
def test_accumulate(ops, dev, kind, N, C3, with_T):
    x, T, w, idx, g, masks = _case(ops, dev, 2, N, C3, kind, seed=3)
    init = torch.randn_like(x)
    acc, _ = _both(ops, x, w, idx, g, masks, T=T if with_T else None, want_gT=with_T, accumulate=True, init=init)
    plain, _ = _both(ops, x, w, idx, g, masks, T=T if with_T else None, want_gT=with_T)
    assert _same_bits(acc, init + plain)


@pytest.mark.parametrize("N,C3", [(33, 32), (1000, 256), (1024, 1024)])
def test_strided_views(ops, dev, N, C3):
    """[B,3,N] and [B,N,3] views with non-trivial strides, for x and for gx: the same numbers as the contiguous call."""
    x, T, w, idx, g, masks = _case(ops, dev, 3, N, C3, seed=5)
    ref, ref_gT = _both(ops, x, w, idx, g, masks, T=T, want_gT=True)
    B = x.shape[0]
    # channel-first views of point-major storage, and of a wider buffer
    x_pm = x.transpose(1, 2).contiguous()                             # [B,N,3] storage
    big = torch.zeros(B, 5, N + 7, device=dev)
    big[:, 1:4, 3:N + 3] = x
    for xv in (x_pm.transpose(1, 2), big[:, 1:4, 3:N + 3]):
        assert not xv.is_contiguous()
        out = torch.full((B, 4, N + 2), 7.0, device=dev)[:, :3, 1:N + 1]
        gx, gT = _both(ops, xv, w, idx, g, masks, T=T, want_gT=True, init=out)
        assert _same_bits(gx, ref) and _same_bits(gT, ref_gT)
    # point-major call ([B,N,3]) on contiguous and on strided storage
    wide = torch.zeros(B, N, 6, device=dev)
    wide[:, :, 2:5] = x_pm
    for xv in (x_pm, wide[:, :, 2:5], x.transpose(1, 2)):
        out = torch.full((B, N, 5), 7.0, device=dev)[:, :, 1:4]
        gx, gT = _both(ops, xv, w, idx, g, masks, T=T, want_gT=True, x_cf=False, init=out)
        assert _same_bits(gx.transpose(1, 2), ref) and _same_bits(gT, ref_gT)
        acc, _ = _both(ops, xv, w, idx, g, masks, T=T, want_gT=True, x_cf=False, accumulate=True, init=out)
        assert _same_bits(acc, out + gx)


@pytest.mark.parametrize("kind", ["natural", "one_point", "skewed"])
def test_two_consecutive_calls_agree(ops, dev, kind):
    x, T, w, idx, g, masks = _case(ops, dev, 4, 1024, 1024, kind, seed=7)
    a, a_gT = ops.pointmlp3_max_bwd_raw(x, w, idx, g, masks, T=T, want_gT=True)
    b, b_gT = ops.pointmlp3_max_bwd_raw(x, w, idx, g, masks, T=T, want_gT=True)
    assert _same_bits(a, b) and _same_bits(a_gT, b_gT)


def test_balanced_backward_in_a_replayed_graph(ops, dev):
    """The kernel as the attack loops run it: captured once, replayed, against the eager two-list launch."""
    x, T, w, idx, g, masks = _case(ops, dev, 4, 1024, 1024, seed=9)
    ref, ref_gT = ops.pointmlp3_max_bwd_raw(x, w, idx, g, masks, T=T, want_gT=True, twolist=True)
    out = torch.empty_like(x)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.pointmlp3_max_bwd_raw(x, w, idx, g, masks, T=T, want_gT=True, out=out)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, gT = ops.pointmlp3_max_bwd_raw(x, w, idx, g, masks, T=T, want_gT=True, out=out)
    for _ in range(3):
        out.fill_(float("nan"))
        gT.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert _same_bits(out, ref) and _same_bits(gT, ref_gT)
