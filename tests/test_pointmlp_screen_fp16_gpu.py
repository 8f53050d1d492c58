"""GPU parity, no tolerances: the PointNet tower forward with layer 3 screened by ONE scaled fp16 product per k-step
(the H form of csrc/pointmlp_screen.hip, bound in csrc/pointmlp_screen_h_bound.h) against the exact fp32 kernel and
against the three-product bf16 form fed from the same prepared image; and that form's bound, measured on the hardware.
The tests name the form (form="fp16" / "bf16"), so they check the same thing whichever of the two is the default."""
import importlib

import numpy as np
import pytest
import torch

from helpers import hip_pointnet
from test_pointmlp_screen_gpu import _host_h2
from test_pointmlp_screen_prepared_gpu import _assert_same, _flat, _packed, _weights

pytestmark = pytest.mark.gpu

TILE = 128
PCAP = 16       # PMH_PCAP: candidates per (tile, channel) before the channel's block runs the exact block


def _run(ops, x, w, relu_last, x_cf=True, **kw):
    a = ops.pointmlp3_max_fwd_raw(x, w, relu_last, x_cf=x_cf, fold=False, **kw)
    b = ops.pointmlp3_max_fwd_raw(x, w, relu_last, x_cf=x_cf, want_masks=True, **kw)
    return _flat(a) + _flat(b)


def _stats(ops, x, w, relu_last=False, form="fp16", **kw):
    dbg = {}
    ops.pointmlp3_max_fwd_raw(x, w, relu_last, fold=False, screen_dbg=dbg, form=form, **kw)
    return dbg["stats"].cpu().numpy().astype(np.int64)


def _assert_parity(ops, x, wp, relu_last=False, x_cf=True, bitwise_nan=False, **kw):
    """fp16 == exact and fp16 == bf16-prepared, all outputs; the image must have been there (or fp16 was not what ran)."""
    hf = _run(ops, x, wp, relu_last, x_cf=x_cf, form="fp16", **kw)
    assert len(wp[7]) == 4 and wp[7][3] == (wp[4].data_ptr(), wp[4]._version) and ops._pm_w3_h(wp[7][0]) is not None
    ex = _run(ops, x, wp, relu_last, x_cf=x_cf, exact=True, **kw)
    bf = _run(ops, x, wp, relu_last, x_cf=x_cf, form="bf16", **kw)
    df = _run(ops, x, wp, relu_last, x_cf=x_cf, **kw)
    torch.cuda.synchronize()
    _assert_same(ex, hf, "fp16 vs exact", bitwise_nan)
    _assert_same(bf, hf, "fp16 vs bf16-prepared", bitwise_nan)
    _assert_same(df, hf, "fp16 vs the default form", bitwise_nan)


# C3: 32 one block, seven idle waves; 96 a half-empty recheck trip; 288 wave 0 has two slots, the others one; 1024 the
# victim's. N: one point, a ragged tile, a full tile, two tiles with a ragged second.
@pytest.mark.parametrize("variant", ["plain", "T", "T_head"])
@pytest.mark.parametrize("N", [1, 33, 128, 200])
@pytest.mark.parametrize("C3", [32, 96, 288, 1024])
def test_fp16_equals_exact_and_bf16(ops, dev, N, C3, variant):
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
    st, sb = _stats(ops, x, wp, **kw), _stats(ops, x, wp, form="bf16", **kw)
    ntiles = (N + TILE - 1) // TILE
    print(f"[fp16 screen] B={B} N={N} C3={C3} {variant}: {st[..., 0].sum() / (B * ntiles * C3):.3f} candidates per "
          f"(tile, channel) (bf16: {sb[..., 0].sum() / (B * ntiles * C3):.3f}), {st[..., 1].sum()} blocks fell back")
    assert st[..., 1].sum() == 0
    assert B * ntiles * C3 <= st[..., 0].sum() <= PCAP * B * ntiles * C3   # the winner of every (tile, channel) at least


def test_image_against_torch(ops, dev):
    """The fp16 image and its cw array, restated: W3 2^sw[c] rounded to nearest even, in the bf16 image's lane order."""
    C3 = 288
    g = torch.Generator().manual_seed(77)
    W3 = torch.randn(C3, 128, generator=g)
    W3[3] *= 1e-12
    W3[40] *= 1e10
    W3[41] = 0.0
    W3[100, ::3] = 0.0
    W3[7, 5] = float("nan")
    W3[9] *= 1e30
    W3 = W3.to(dev).contiguous()
    bf, nw, q = ops.pointmlp3_w3_prepare(W3)
    (h, cw), ptrs = ops._pm_w3_h(bf)
    torch.cuda.synchronize()
    assert h.shape == (C3 // 32, 8, 64, 8) and h.dtype == torch.float16 and cw.shape == (C3,)
    assert h.untyped_storage().data_ptr() == bf.untyped_storage().data_ptr() and ptrs[0] == h.data_ptr() and ptrs[1] == cw.data_ptr()
    ok = nw <= 2.0 ** 60
    assert not ok[7] and not ok[9] and int((~ok).sum()) == 2
    sw = 13 - torch.floor(torch.log2(nw.double()))
    scaled = (W3.double() * torch.exp2(sw)[:, None]).float()                 # exact: a power of two
    want = torch.where(ok[:, None], scaled, torch.zeros_like(scaled)).to(torch.float16)
    order = want.view(C3 // 32, 32, 8, 2, 8).permute(0, 2, 3, 1, 4).reshape(C3 // 32, 8, 64, 8).contiguous()
    assert torch.equal(h.view(torch.int16), order.view(torch.int16))
    assert torch.isinf(cw[~ok]).all() and (cw[~ok] > 0).all()
    ns = nw.double() * torch.exp2(sw)
    assert ((ns >= 2.0 ** 13) & (ns < 2.0 ** 14))[ok].all()
    assert torch.equal(cw[ok], (torch.tensor(1.0625 * 2.0 ** -10, dtype=torch.float32, device=dev) * ns.float())[ok])


def test_cap_edge(ops, dev):
    """PCAP equal candidates in every channel fill the slots exactly; one more and every block runs the exact block.
    The lowest index wins on either path."""
    C3 = 256
    w = _weights(dev, C3, 5)
    g = torch.Generator().manual_seed(11)
    one = torch.randn(1, 3, 1, generator=g).to(dev) * 0.5
    for n, fell in ((PCAP, 0), (PCAP + 1, C3 // 32)):
        wp = _packed(w)
        x = one.expand(1, 3, n).contiguous()
        _assert_parity(ops, x, wp)
        _, pi = ops.pointmlp3_max_fwd_raw(x, wp, False, fold=False, form="fp16")
        assert int(pi.abs().max()) == 0
        st = _stats(ops, x, wp)
        assert st[..., 1].sum() == fell
        assert st[..., 0].sum() == (C3 * PCAP if fell == 0 else 0)


def test_ties_and_jitter(ops, dev):
    C3 = 256
    wp = _packed(_weights(dev, C3, 5))
    g = torch.Generator().manual_seed(11)
    one = torch.randn(1, 3, 1, generator=g).to(dev) * 0.5
    half = torch.randn(2, 3, 64, generator=g).to(dev) * 0.5
    x = torch.cat([half, half], dim=2).contiguous()                     # each point duplicated at a higher index
    _assert_parity(ops, x, wp)
    _, idx = ops.pointmlp3_max_fwd_raw(x, wp, False, form="fp16")
    assert int(idx.max()) < 64
    st = _stats(ops, x, wp)
    assert st[..., 0].sum() >= 2 * 2 * C3 - 64 * st[..., 1].sum()        # both copies of every screened winner were rechecked
    x = (one + 1e-7 * torch.randn(1, 3, TILE, generator=g).to(dev)).contiguous()
    _assert_parity(ops, x, wp)
    st = _stats(ops, x, wp)
    print(f"[fp16 screen] jitter 1e-7: {st[..., 1].sum()} of {C3 // 32} channel blocks fell back, {st[..., 0].sum()} candidates rechecked")
    assert st[..., 1].sum() > 0


@pytest.mark.parametrize("case", ["nan_coord", "inf_coord", "huge_coord", "w3_nan", "w3_inf", "w3_tiny", "w3_huge",
                                  "w3_small_row", "w3_zero_column"])
def test_non_finite_and_extreme(ops, dev, case):
    B, N, C3 = 2, 200, 256
    torch.manual_seed(7)
    w = _weights(dev, C3, 3)
    x = torch.randn(B, 3, N, device=dev) * 0.5
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
    elif case == "w3_small_row":
        w[4][70] *= 1e-6
    elif case == "w3_zero_column":
        w[4][:, 9] = 0.0
    wp = _packed(w)                       # the images are made from the edited weights
    _assert_parity(ops, x, wp, bitwise_nan=True)
    _assert_parity(ops, x.transpose(1, 2).contiguous(), wp, x_cf=False, bitwise_nan=True)
    st = _stats(ops, x, wp)
    print(f"[fp16 screen] {case}: fell back {st[..., 1].tolist()} of {C3 // 32} blocks per tile, candidates {st[..., 0].tolist()}")
    if case in ("w3_nan", "w3_inf"):
        assert (st[..., 1] >= 1).all()
    if case in ("w3_small_row", "w3_zero_column"):
        assert st[..., 1].sum() == 0      # a channel's own exponent: a small row is screened like any other


@pytest.mark.parametrize("B,N,C3", [(1, 128, 64), (1, 200, 1024)])
def test_bound_holds_on_the_hardware(ops, dev, B, N, C3):
    """|v - S| <= E for every (point, channel): S and E as the kernel formed them (handed back in the unscaled domain:
    both times the same exact power of two), v the exact product in float64. The printed ratio is the check of what
    pointmlp_screen_h_bound.h allows for the fp16 conversions and the MFMA's undocumented accumulation.
    Measured on MI355X: see DESIGN.md 3.1."""
    torch.manual_seed(N + C3)
    wp = _packed(_weights(dev, C3, 21))
    x = torch.randn(B, 3, N, device=dev) * 0.5
    dbg = {"dump": True}
    _, _, masks = ops.pointmlp3_max_fwd_raw(x, wp, False, want_masks=True, screen_dbg=dbg, form="fp16")
    torch.cuda.synchronize()
    assert int(dbg["stats"][..., 1].sum()) == 0                           # every block went through the screen
    S, E = dbg["S"].double().cpu(), dbg["E"].double().cpu()
    assert torch.isfinite(S).all() and torch.isfinite(E).all()
    v = _host_h2(x, wp, masks[1]) @ wp[4].double().cpu().t()
    ratio = ((v - S).abs() / E).max().item()
    print(f"[fp16 screen] N={N} C3={C3}: max |v - S| / E = {ratio:.4f}")
    assert ratio < 1.0


def test_replayed_graph_and_weight_reload(ops, dev):
    """Eager (makes both images in one allocation), capture, replays; then new weights: a new image is made, and the old
    graph still replays on the old one, which the bf16 image's tensor keeps alive."""
    graphed = importlib.import_module("3dpointcloudattack_amd.graphed")
    pn = importlib.import_module("3dpointcloudattack_amd.model.pointnet")
    ort = importlib.import_module("oracle.ref_torch")
    torch.manual_seed(5)
    x = torch.randn(4, 3, 300, device=dev) * 0.5

    def run(model, **kw):
        pk = pn.fused_pack(model)
        return ops.pointmlp3_max_fwd_raw(x, pk["tower_s"], True, want_masks=True, **kw), pk

    model, _ = hip_pointnet(3, dev)
    ref = [t.clone() for t in _flat(run(model, exact=True)[0])]
    eager, pk = run(model, form="fp16")
    eager = [t.clone() for t in _flat(eager)]
    pack = pk["tower_s"][7]
    assert len(pack) == 4 and ops._pm_w3_h(pack[0]) is not None
    _assert_same(ref, eager, "eager fp16 vs exact")
    graph = torch.cuda.CUDAGraph()
    with graphed.capture_guard() as keep:
        with torch.cuda.graph(graph):
            out, pk_old = run(model, form="fp16")
    out = _flat(out)
    cached = {id(t) for t in graphed._cached_tensors(model)}
    assert id(pack[0]) in cached          # the one allocation: bf16 image, fp16 image and cw
    old_ptr = pack[0].untyped_storage().data_ptr()

    def replay_equals(want):
        for t in out:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        _assert_same(want, out, "replay")

    replay_equals(eager)
    model.load_state_dict(ort.seeded_state_dict(model, 4))
    new, pk_new = run(model, form="fp16")
    new = _flat(new)
    pack_new = pk_new["tower_s"][7]
    assert pack_new is not pack and len(pack_new) == 4
    assert pack_new[0].untyped_storage().data_ptr() != old_ptr and pack[0].untyped_storage().data_ptr() == old_ptr
    _assert_same(_flat(run(model, exact=True)[0]), new, "new weights: fp16 vs exact")
    assert not torch.equal(new[0], eager[0])
    replay_equals(eager)
    del keep, pk_old
