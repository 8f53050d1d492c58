"""GPU: every entry point of the PointNet tower backward against its float64 reference, element by element.

ops.pointmlp3_max_bwd_raw (the default entry, the tile32, the packed and the two-list form), ops.pointnet_ft_tower_bwd_raw
(the plain form that pointmlp3_max(..., blocked_bwd=True) runs, and the trunk form with a per-cloud W2) and
ops.pointmlp3_max under autograd are held to tests/pointmlp_bwd_restatement.py: the statement of csrc/pointmlp.hip in
plain torch, tied to torch autograd in float64 by tests/test_pointmlp_bwd_ref_cpu.py. argidx, g and both ReLU masks are
inputs of the raw backward, so nothing is left to a tie or to a ReLU at zero: every word of gx and part_gT has to lie
within band = 16 M_REF 2^-24 A of the float64 value (A: the same statement on absolute values; M_REF: the error of the
fp32 restatements, measured on the CPU), the pad words 9..15 of a part_gT record and everything a dead point or a tile
without a hit owns are exact zeros, storage outside the views keeps its payload NaN, and a NaN or an infinity in g
stays in the rows of its own point: every other point and record keeps its finite band, the poisoned ones have the
reference's class (NaN, +inf, -inf, finite) word by word. No case needed narrowing: fp32 overflows nowhere here, and
the kernels' selects, chains and MFMA rows give a non-finite operand no way into another row.

This is the value anchor of the bit-parity chain (test_pointmlp_bwd_balance_gpu.py, test_pointmlp_bwd_packed_gpu.py,
test_cw_riders_gpu.py). Every case prints the kernel's largest err / band.

Largest kernel err / band measured on the MI355X over all cases and entries: 0.0624 for gx (case
32-N257-C1024-one_per_point-single_bit-randn-noT; the default, tile32, packed and two-list entries alike, 0.0614 on
the plain and 0.0570 on the trunk form of pointnet_ft_tower_bwd_raw) and 0.0623 for part_gT (case
17-N257-C64-skewed-single_bit-large-T, the same four entries; 0.0578 on the trunk form). Both are single-bit-mask cases
and sit at 1/16: the kernels are as far from float64 as the fp32 restatements are. With random masks no case is above
0.006.

What the test found: through T, a point without a hit that shares its 32-point sub-tile with a live one got -0 instead
of +0 in every coordinate whose row of T is negative throughout (g'[0] T[c][0] = -0 started the chain). The chain now
starts from +0 in all forms; no other bit changes.
"""
import importlib

import pytest
import torch

import pointmlp_bwd_restatement as rs

pytestmark = pytest.mark.gpu
ops = importlib.import_module("3dpointcloudattack_amd.ops")

CASES = rs.cases()
IDS = [c["name"] for c in CASES]
ENTRIES = ("default", "tile32", "packed", "twolist", "ft_plain", "ft_trunk")
RAW_KW = {"default": {}, "tile32": dict(tile32=True), "packed": dict(tile32=False), "twolist": dict(twolist=True)}
FORM = {"ft_plain": "plain", "ft_trunk": "trunk"}


def _nan_fill(shape, dev):
    return torch.full(shape, rs.NAN_WORD, dtype=torch.int32, device=dev).view(torch.float32)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _weights(case, dev):
    w = tuple(t.to(dev) for t in case["weights"])
    return w + (w[2].t().contiguous(),)


def _inputs(case, dev, **over):
    x, T, W1, W2, W3, argidx, g, mask1, mask2 = (None if t is None else t.to(dev) for t in rs.args_of(case, **over))
    return x, T, argidx, g, (mask1, mask2)


def _launch(entry, case, dev, i, **over):
    """(gx [B,3,N], part_gT or None) on the CPU, of the contiguous channel-first call"""
    x, T, argidx, g, masks = _inputs(case, dev, **over)
    w = _weights(case, dev)
    B, _, N = x.shape
    if entry in RAW_KW:
        r = ops.pointmlp3_max_bwd_raw(x, w, argidx, g, masks, T=T, want_gT=T is not None, **RAW_KW[entry])
        gx, gT = r if T is not None else (r, None)
    elif entry == "ft_plain":
        gx, q = ops.pointnet_ft_tower_bwd_raw(x, None, w[0], w[2], w[4], argidx, g, masks, None, 0)
        assert q is None
        gT = None
    else:
        ws, nt = ops.pointnet_ft_gT_workspace(B, N, dev, towers=2)
        assert ws.shape == (B, 2 * nt, 16) and nt == (N + 31) // 32
        ws.copy_(_nan_fill(ws.shape, dev))
        off = nt * (i % 2)                          # either tower's rows
        gx, q = ops.pointnet_ft_tower_bwd_raw(x, case["T_any"].to(dev), w[0], case["W2b"].to(dev), w[4], argidx, g, masks, ws,
                                              off, W2q=w[2])
        assert q.shape == (B, N, 64)
        other = ws[:, nt - off:2 * nt - off]
        assert bool((_bits(other) == rs.NAN_WORD).all()), "the other tower's part_gT rows were written"
        gT = ws[:, off:off + nt]
    torch.cuda.synchronize()
    return gx.cpu(), None if gT is None else gT.cpu()


def _dead(case):
    """bool [B,N]: points without a hit"""
    return rs.hit_counts(case["argidx"], case["g"], case["x"].shape[2]) == 0


def _check_zeros(case, gx, gT, what):
    """a dead point's gradient is exact +0, and so is the record of a tile without a hit"""
    dead = _dead(case)
    B, _, N = case["x"].shape
    assert not _bits(gx.transpose(1, 2)[dead]).any(), what + ": gx of a dead point is not +0 bit for bit"
    if gT is not None:
        nt = (N + 31) // 32
        empty = torch.cat([dead, torch.ones(B, nt * 32 - N, dtype=torch.bool)], 1).reshape(B, nt, 32).all(2)
        assert not _bits(gT[empty]).any(), what + ": the part_gT record of a tile without a hit is not +0"


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_entry_matches_float64(dev, entry, i):
    case = CASES[i]
    ref = rs.reference(i, FORM.get(entry, "raw"))
    what = "%s, %s" % (case["name"], entry)
    gx, gT = _launch(entry, case, dev, i)
    print("%s: err / band  gx %s" % (what, "  part_gT ".join("%.4f" % q for q in _ratios(case, gx, gT, ref))))
    rs.check(case, gx, gT, ref, what)
    _check_zeros(case, gx, gT, what)


def _ratios(case, gx, gT, ref):
    ok_pt, ok_tile = rs.clean_points(case)
    return (rs.ratio(gx, ref[0], ref[2], ok_pt),) + (() if gT is None or ref[1] is None else (rs.ratio(gT, ref[1], ref[3], ok_tile),))


# ----------------------------------------------------------------------------------------------------------------------
# layouts: point-major, views, accumulate, sentinels
# ----------------------------------------------------------------------------------------------------------------------
LAYOUT_CASES = [i for i, c in enumerate(CASES) if c["x"].shape[2] in (33, 129, 160, 257) and c["W3"].shape[0] >= 64][:12] \
    + [i for i, c in enumerate(CASES) if c["g_kind"] == "dead_point"]
LAYOUTS = ("pm", "cf_view_of_pm", "cf_wide", "pm_wide")


def _views(layout, x, dev, seed):
    """(x view, out view, out storage, x_cf): x inside random storage, out inside payload-NaN storage"""
    B, _, N = x.shape
    gen = torch.Generator().manual_seed(seed)
    if layout == "pm":
        return x.transpose(1, 2).contiguous(), _nan_fill((B, N, 3), dev), None, False
    if layout == "cf_view_of_pm":
        store = _nan_fill((B, N, 3), dev)
        return x.transpose(1, 2).contiguous().transpose(1, 2), store.transpose(1, 2), None, True
    if layout == "cf_wide":
        big = torch.randn(B, 5, N + 7, generator=gen).to(dev)
        big[:, 1:4, 3:N + 3] = x
        store = _nan_fill((B, 4, N + 2), dev)
        return big[:, 1:4, 3:N + 3], store[:, :3, 1:N + 1], store, True
    big = torch.randn(B, N + 2, 6, generator=gen).to(dev)
    big[:, 1:N + 1, 2:5] = x.transpose(1, 2)
    store = _nan_fill((B, N + 1, 5), dev)
    return big[:, 1:N + 1, 2:5], store[:, :N, 1:4], store, False


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("i", LAYOUT_CASES, ids=[IDS[i] for i in LAYOUT_CASES])
def test_layouts_and_accumulate(dev, i, layout, accumulate):
    case = CASES[i]
    ref = rs.reference(i)
    x, T, argidx, g, masks = _inputs(case, dev)
    w = _weights(case, dev)
    B, _, N = x.shape
    dead = _dead(case)
    for entry, kw in RAW_KW.items():
        what = "%s, %s, %s%s" % (case["name"], entry, layout, ", accumulate" if accumulate else "")
        xv, out, store, x_cf = _views(layout, x, dev, i)
        init = None
        if accumulate:
            init = torch.randn(B, 3, N, generator=torch.Generator().manual_seed(i)).to(dev)
            out.copy_(init if x_cf else init.transpose(1, 2))
        if store is not None:
            before = _bits(store).clone()
        r = ops.pointmlp3_max_bwd_raw(xv, w, argidx, g, masks, T=T, want_gT=T is not None, x_cf=x_cf, out=out,
                                      accumulate=accumulate, **kw)
        gx, gT = r if T is not None else (r, None)
        assert gx.data_ptr() == out.data_ptr()
        torch.cuda.synchronize()
        if store is not None:           # every word outside the view keeps its payload NaN
            inside = torch.zeros_like(store, dtype=torch.bool)
            (inside[:, :3, 1:N + 1] if x_cf else inside[:, :N, 1:4]).fill_(True)
            assert torch.equal(_bits(store)[~inside], before[~inside]), what + ": a word outside the out view was written"
            assert bool((_bits(store)[~inside] == rs.NAN_WORD).all())
        gx = (gx if x_cf else gx.transpose(1, 2)).cpu()
        gT = None if gT is None else gT.cpu()
        if not accumulate:
            rs.check(case, gx, gT, ref, what)
            _check_zeros(case, gx, gT, what)
            continue
        # init + gx, one more rounding: the band gains 2^-24 |init + gx|
        want = init.cpu().double() + ref[0]
        ref_acc = (want, ref[1], ref[2] + rs.EPS * want.abs(), ref[3])
        rs.check(case, gx, gT, ref_acc, what)
        kept = _bits(gx.transpose(1, 2)[dead]) == _bits(init.cpu().transpose(1, 2)[dead])
        assert bool(kept.all()), what + ": an accumulating launch changed the bits of a dead point"
        if gT is not None:
            _check_zeros(case, torch.zeros_like(gx), gT, what)


# ----------------------------------------------------------------------------------------------------------------------
# autograd
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blocked", [False, True])
@pytest.mark.parametrize("relu_last", [False, True])
@pytest.mark.parametrize("N,C3,B", [(33, 64, 3), (160, 1024, 2), (257, 1024, 3)])
def test_autograd_entry(dev, N, C3, B, relu_last, blocked):
    """ops.pointmlp3_max: the reference gets the forward kernel's own argidx, masks and pooled > 0"""
    gen = torch.Generator().manual_seed(17 * N + C3)
    w = rs._weights(gen, C3)
    x = torch.randn(B, 3, N, generator=gen) * 0.5
    up = torch.randn(B, C3, generator=gen)
    wd = tuple(t.to(dev) for t in w)
    wd = wd + (wd[2].t().contiguous(),)
    pooled, argidx, masks = ops.pointmlp3_max_fwd_raw(x.to(dev), wd, relu_last, want_masks=True)
    xr = x.to(dev).requires_grad_()
    y = ops.pointmlp3_max(xr, wd, relu_last, blocked_bwd=blocked)
    assert torch.equal(_bits(y.detach()), _bits(pooled))
    y.backward(up.to(dev))
    torch.cuda.synchronize()
    g = up * (pooled.cpu() > 0) if relu_last else up
    if relu_last:
        assert 0 < int((pooled > 0).sum()) < pooled.numel()
    args = (x, None, w[0], w[2], w[4], argidx.cpu(), g, masks[0].cpu(), masks[1].cpu())
    case = dict(x=x, argidx=argidx.cpu(), g=g)
    ref = rs.run(torch.float64, *args) + rs.bands(*args)
    what = "autograd N=%d C3=%d relu_last=%s blocked=%s" % (N, C3, relu_last, blocked)
    q = rs.check(case, xr.grad.cpu(), None, ref, what)
    print("%s: err / band gx %.4f" % (what, q[0]))
    _check_zeros(case, xr.grad.cpu(), None, what)


# ----------------------------------------------------------------------------------------------------------------------
# sensitivity on the device
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_checker_sees_every_mutation_on_the_device(dev, i):
    """the kernel gets the mutated (valid) inputs, the checker the unmutated reference: it must raise"""
    case = CASES[i]
    ref = rs.reference(i)
    for kind, over, _ in rs.mutations(i):
        if "argidx" in over:
            assert 0 <= int(over["argidx"].min()) and int(over["argidx"].max()) < case["x"].shape[2]
        for entry in ("default", "twolist"):
            gx, gT = _launch(entry, case, dev, i, **over)
            with pytest.raises(AssertionError):
                rs.check(case, gx, gT, ref, kind)


def test_want_gT_needs_T(dev):
    c = CASES[0]
    x, T, argidx, g, masks = _inputs(c, dev)
    with pytest.raises(ValueError, match="T and part_gT go together"):
        ops.pointmlp3_max_bwd_raw(x, _weights(c, dev), argidx, g, masks, T=None, want_gT=True)
