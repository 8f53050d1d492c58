"""GPU parity, no tolerances: the packed form of the tower backward (a workgroup per 128 points; the W2 product over
the rows of points that have a hit only, packed into blocks of 32 rows) against the tile32 form (a workgroup per 32
points, every row multiplied). MFMA rows are independent and every chain is stated the same way, so gx, part_gT and —
for the launch with the update epilogue — adv, m and v must agree in every bit; they are compared as
tests/test_pointmlp_bwd_balance_gpu.py compares (NaN positions, every other word as int32).
The cases are those that file's kinds do not pin: the number of live points of one 128-point tile around the 32-row
block boundaries, where in the tile they sit (a row slot taken for a point position shows there), ragged last tiles,
one point owning every channel with special values in g, strided views, a replayed graph."""
import pytest
import torch

pytestmark = pytest.mark.gpu

TP = 128        # points per workgroup of the packed form


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


def _special(g):
    """+0, -0, NaN, +-inf among ordinary values, by channel"""
    sel = torch.arange(g.shape[1], device=g.device) % 7
    g = g.clone()
    g[:, sel == 1] = 0.0
    g[:, sel == 2] = -0.0
    g[:, sel == 3] = float("nan")
    g[:, sel == 4] = float("inf")
    g[:, sel == 5] = float("-inf")
    return g


def _case(ops, dev, B, N, C3, seed=0):
    torch.manual_seed(1000 * seed + N + C3)
    x = torch.randn(B, 3, N, device=dev) * 0.5
    T = torch.randn(B, 3, 3, device=dev) * 0.5
    w = _weights(dev, C3, seed + 1)
    _, natural, masks = ops.pointmlp3_max_fwd_raw(x, w, False, T=T, want_masks=True)
    return x, T, w, natural, torch.randn(B, C3, device=dev), masks


def _fresh(init):
    return torch.empty_strided(init.shape, init.stride(), dtype=init.dtype, device=init.device).copy_(init)


def _raw(ops, x, w, idx, g, masks, T=None, want_gT=False, accumulate=False, x_cf=True, init=None):
    """gx (and part_gT) of both forms, compared; returns the packed form's"""
    res = []
    for tile32 in (False, True):
        r = ops.pointmlp3_max_bwd_raw(x, w, idx, g, masks, T=T, x_cf=x_cf, out=None if init is None else _fresh(init),
                                      accumulate=accumulate, want_gT=want_gT, tile32=tile32)
        res.append(r if want_gT else (r, None))
    (gx_p, gt_p), (gx_t, gt_t) = res
    assert _same_bits(gx_p, gx_t), "gx differs from the tile32 form"
    if want_gT:
        assert gt_p.shape == (x.shape[0], (idx_n(x, x_cf) + 31) // 32, 16)
        assert _same_bits(gt_p, gt_t), "part_gT differs from the tile32 form"
    return gx_p, gt_p


def idx_n(x, x_cf):
    return x.shape[2] if x_cf else x.shape[1]


def _update(ops, x, w, idx, g, masks, dist_kind=2, seed=0, x_cf=True):
    """the launch with the CW update as its epilogue: adv, m, v of both forms, compared"""
    dev = x.device
    B, N = x.shape[0], idx_n(x, x_cf)
    gen = torch.Generator().manual_seed(77 + seed)

    def r(*s):
        return torch.randn(*s, generator=gen).to(dev)
    shape = tuple(x.shape)
    state = dict(adv=x, ori=x + 0.05 * r(*shape), m=1e-3 * r(*shape), v=1e-6 * r(*shape).abs(), gx=r(*shape))
    wts = (torch.rand(B, generator=gen) * 20 + 1).to(dev)
    dist_val = (torch.rand(B, generator=gen) + 0.5).to(dev)
    nn_idx = torch.randint(0, N, (B, N), generator=gen).to(dev).to(torch.int32)
    adam = torch.tensor([0.01, 1.7], device=dev)
    res = []
    for tile32 in (False, True):
        s = {k: _fresh(v) for k, v in state.items()}
        ops.pointmlp3_max_bwd_update(s["adv"], w, idx, g, masks, s["gx"], s["ori"], s["m"], s["v"], adam, 0.18,
                                     dist_kind=dist_kind, w=wts, dist_val=dist_val, nn_idx=nn_idx, x_cf=x_cf,
                                     tile32=tile32)
        assert torch.equal(_bits(s["gx"]), _bits(state["gx"]))          # gx is only read
        res.append(s)
    for k in ("adv", "m", "v"):
        assert _same_bits(res[0][k], res[1][k]), k + " differs from the tile32 form"
    assert not torch.equal(res[0]["adv"], x)
    return res[0]


def _all_launches(ops, x, T, w, idx, g, masks, seed=0):
    _raw(ops, x, w, idx, g, masks)                                      # no T, no part_gT
    _raw(ops, x, w, idx, g, masks, T=T, want_gT=True)                   # the trunk's launch
    _raw(ops, x, w, idx, g, masks, accumulate=True, init=torch.randn_like(x))   # the STN tower's
    _raw(ops, x, w, idx, g, masks, T=T, want_gT=True, accumulate=True, init=torch.randn_like(x))
    for dist_kind in (0, 1, 2):
        _update(ops, x, w, idx, g, masks, dist_kind=dist_kind, seed=seed)


def _route(B, N, C3, live, sink, dev):
    """channel j -> live[j] while they last (one channel per chosen point), every other channel -> the point `sink`"""
    idx = torch.full((C3,), sink, dtype=torch.int64)
    k = min(len(live), C3)
    idx[:k] = torch.as_tensor(live[:k], dtype=torch.int64)
    assert int(idx.max()) < N
    return idx.to(torch.int32).to(dev)[None, :].expand(B, C3).contiguous()


N3 = 3 * TP     # three 128-point tiles: tile 0 without a hit, tile 1 under test, the sink in tile 2
PERM = torch.randperm(TP, generator=torch.Generator().manual_seed(5)).tolist()


@pytest.mark.parametrize("C3", [32, 1024])
@pytest.mark.parametrize("live", [0, 1, 31, 32, 33, 64, 65, 96, 97, 128])
def test_live_points_in_one_tile(ops, dev, live, C3):
    """exactly `live` points of tile 1 have a hit (C3 = 32: as many as the channels reach): 0 to 4 row blocks, full and
    ragged ones; tile 0 takes the no-hit exit, the sink point collects the rest of the channels"""
    x, T, w, _, g, masks = _case(ops, dev, 2, N3, C3, seed=live)
    pts = sorted(TP + p for p in PERM[:live])
    idx = _route(2, N3, C3, pts, 2 * TP + 44, dev)
    assert len(set(idx[0].tolist()) & set(range(TP, 2 * TP))) == min(live, C3)
    _all_launches(ops, x, T, w, idx, g, masks, seed=live)


POSITIONS = {
    "last_sub_tile": [96 + p for p in (0, 3, 4, 9, 17, 30, 31)],
    "first_sub_tile": [0, 1, 7, 16, 29, 31],
    "one_per_sub_tile": [5, 40, 77, 127],
    "second_and_fourth": [32, 63, 100, 126],
}


@pytest.mark.parametrize("C3", [32, 1024])
@pytest.mark.parametrize("where", sorted(POSITIONS))
def test_position_of_the_live_points(ops, dev, where, C3):
    """few live points, so row slot != point position almost everywhere; sub-tiles without a hit next to ones with"""
    x, T, w, _, g, masks = _case(ops, dev, 2, N3, C3, seed=len(where))
    pts = [TP + p for p in POSITIONS[where]]
    # the channels past the chosen points go to the LAST chosen point: no hit anywhere else
    idx = _route(2, N3, C3, pts, pts[-1], dev)
    gx, _ = _raw(ops, x, w, idx, g, masks, T=T, want_gT=True)
    dead = torch.ones(N3, dtype=torch.bool, device=dev)
    dead[torch.as_tensor(pts, device=dev)] = False
    assert not gx[:, :, dead].any()
    _all_launches(ops, x, T, w, idx, g, masks)


@pytest.mark.parametrize("N", [33, 129, 160, 1000])
@pytest.mark.parametrize("C3", [32, 1024])
def test_ragged_sizes(ops, dev, N, C3):
    """a last tile with fewer than 128, and a last sub-tile with fewer than 32, points; natural arg-max"""
    x, T, w, natural, g, masks = _case(ops, dev, 3, N, C3, seed=N)
    _all_launches(ops, x, T, w, natural, g, masks)
    last = torch.full_like(natural, N - 1)                              # every channel on the very last point
    _all_launches(ops, x, T, w, last, g, masks)


@pytest.mark.parametrize("g_kind", ["randn", "special"])
def test_one_point_owns_every_channel(ops, dev, g_kind):
    x, T, w, natural, g, masks = _case(ops, dev, 2, 1024, 1024, seed=11)
    if g_kind == "special":
        g = _special(g)
    idx = torch.full_like(natural, 5 * TP + 77)
    _all_launches(ops, x, T, w, idx, g, masks)


def test_special_gradients_on_live_and_dead_points(ops, dev):
    """zeros, +-inf and NaN in g: a point whose channels all carry g == 0 is dead, one with a NaN is live"""
    x, T, w, natural, g, masks = _case(ops, dev, 2, 1024, 1024, seed=13)
    g = _special(g)
    _all_launches(ops, x, T, w, natural, g, masks)
    c = torch.arange(1024, device=dev)
    by_seven = (TP + c % 7).to(torch.int32)[None, :].expand(2, 1024).contiguous()   # point 128 + k <- channels = k mod 7
    _all_launches(ops, x, T, w, by_seven, g, masks)


@pytest.mark.parametrize("N,C3", [(160, 32), (1000, 1024)])
def test_strided_views(ops, dev, N, C3):
    """[B,3,N] views of point-major and of wider storage, and point-major calls, for x and gx"""
    x, T, w, natural, g, masks = _case(ops, dev, 2, N, C3, seed=5)
    ref, ref_gT = _raw(ops, x, w, natural, g, masks, T=T, want_gT=True)
    B = x.shape[0]
    x_pm = x.transpose(1, 2).contiguous()
    big = torch.zeros(B, 5, N + 7, device=dev)
    big[:, 1:4, 3:N + 3] = x
    for xv in (x_pm.transpose(1, 2), big[:, 1:4, 3:N + 3]):
        out = torch.full((B, 4, N + 2), 7.0, device=dev)[:, :3, 1:N + 1]
        gx, gT = _raw(ops, xv, w, natural, g, masks, T=T, want_gT=True, init=out)
        assert _same_bits(gx, ref) and _same_bits(gT, ref_gT)
        acc, _ = _raw(ops, xv, w, natural, g, masks, T=T, want_gT=True, accumulate=True, init=out)
        assert _same_bits(acc, out + gx)
    wide = torch.zeros(B, N, 6, device=dev)
    wide[:, :, 2:5] = x_pm
    for xv in (x_pm, wide[:, :, 2:5]):
        out = torch.full((B, N, 5), 7.0, device=dev)[:, :, 1:4]
        gx, gT = _raw(ops, xv, w, natural, g, masks, T=T, want_gT=True, x_cf=False, init=out)
        assert _same_bits(gx.transpose(1, 2), ref) and _same_bits(gT, ref_gT)
    _update(ops, x, w, natural, g, masks)
    _update(ops, x_pm, w, natural, g, masks, x_cf=False)                # adv, m, v and gx point-major


def test_two_runs_agree_and_default_entry(ops, dev):
    x, T, w, natural, g, masks = _case(ops, dev, 3, 1024, 1024, seed=7)
    a, a_gT = ops.pointmlp3_max_bwd_raw(x, w, natural, g, masks, T=T, want_gT=True, tile32=False)
    b, b_gT = ops.pointmlp3_max_bwd_raw(x, w, natural, g, masks, T=T, want_gT=True, tile32=False)
    assert _same_bits(a, b) and _same_bits(a_gT, b_gT)
    d, d_gT = ops.pointmlp3_max_bwd_raw(x, w, natural, g, masks, T=T, want_gT=True)       # whichever form is the default
    assert _same_bits(a, d) and _same_bits(a_gT, d_gT)


def test_packed_backward_in_a_replayed_graph(ops, dev):
    x, T, w, natural, g, masks = _case(ops, dev, 3, 1024, 1024, seed=9)
    ref, ref_gT = ops.pointmlp3_max_bwd_raw(x, w, natural, g, masks, T=T, want_gT=True, tile32=True)
    out = torch.empty_like(x)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.pointmlp3_max_bwd_raw(x, w, natural, g, masks, T=T, want_gT=True, out=out, tile32=False)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, gT = ops.pointmlp3_max_bwd_raw(x, w, natural, g, masks, T=T, want_gT=True, out=out, tile32=False)
    for _ in range(3):
        out.fill_(float("nan"))
        gT.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert _same_bits(out, ref) and _same_bits(gT, ref_gT)
