"""GPU: every form of the PointNet tower's three launch entries is reachable through ops, ops passes the form it was
asked for, and all forms of a launch write the same bits. B = 2, N = 130, C3 = 64: two forward tiles (and two packed
backward workgroups), the last with 2 valid points. No captures here: a form's first use inside one is
test_pointmlp_screen_pair_gpu's subject."""
import pytest
import torch

from test_pointmlp_screen_prepared_gpu import _flat, _packed, _weights

pytestmark = pytest.mark.gpu

B, N, C3 = 2, 130, 64
EXACT, SCREEN, PREP, H, H_PAIR = range(5)              # PC3D_PM_FWD_*
DEFAULT, PACKED, TILE32, TWOLIST = range(4)            # PC3D_PM_BWD_*
FWD_FORM_ARG = 28                                      # pc3d_pointmlp3_max_fwd_f32: x + 3 strides, B, N, T, 5 head, 6 weights,
                                                       # 3 widths, relu_last, 6 outputs, then form
BWD_FORM_ARG, UPD_FORM_ARG = -3, -2                    # ..., form, stop_after, stream / ..., form, stream


@pytest.fixture
def forms(ops, monkeypatch):
    """The arguments of every tower launch that ops makes, by entry."""
    seen = {}
    call = ops._lib.call

    def recording(name, *args):
        if name.startswith("pc3d_pointmlp3_max_"):
            seen.setdefault(name, []).append(args)
        return call(name, *args)
    monkeypatch.setattr(ops._lib, "call", recording)
    return seen


@pytest.fixture(scope="module")
def case(dev):
    torch.manual_seed(B * 100003 + N * 101 + C3)
    K = 256
    return dict(wp=_packed(_weights(dev, C3, N + C3)), x=torch.randn(B, 3, N, device=dev) * 0.5,
                T=torch.eye(3, device=dev)[None] + 0.3 * torch.randn(B, 3, 3, device=dev),
                T_head=(torch.randn(B, K, device=dev), (torch.randn(9, K, device=dev) / K ** 0.5).contiguous(),
                        torch.eye(3, device=dev).reshape(9).contiguous()),
                g=torch.randn(B, C3, device=dev))


def _same(ref, got, what):
    assert len(ref) == len(got), what
    for i, (e, s) in enumerate(zip(ref, got)):
        assert e.dtype == s.dtype and torch.equal(e, s), f"{what}: output {i} differs"


@pytest.mark.parametrize("variant", ["plain", "T", "T_head"])
def test_forward_forms(ops, dev, forms, case, variant):
    kw = {} if variant == "plain" else {variant: case[variant]}
    x, wp = case["x"], case["wp"]

    def run(**form_kw):
        """(pooled, argidx, mask1, mask2[, T_out]) and the form that ops passed"""
        res = _flat(ops.pointmlp3_max_fwd_raw(x, wp, False, want_masks=True, **form_kw, **kw))
        return res, forms["pc3d_pointmlp3_max_fwd_f32"][-1][FWD_FORM_ARG]

    ops.pointmlp3_max_fwd_raw(x, wp, False)               # fills the prepared image (outside any capture)
    assert len(wp[7]) == 4 and ops._pm_w3_h(wp[7][0]) is not None
    ref, form = run(exact=True)
    assert form == EXACT and len(ref) == (5 if variant == "T_head" else 4)
    for form_kw, want in [(dict(in_launch=True), SCREEN), (dict(form="bf16"), PREP), (dict(recheck="channel"), H),
                          (dict(form="fp16", recheck="channel"), H), (dict(recheck="pair"), H_PAIR),
                          (dict(), ops._pm_fwd_form(False, False, True, True, None, None, False))]:
        got, form = run(**form_kw)
        assert form == want, (form_kw, form)
        torch.cuda.synchronize()
        _same(ref, got, f"{variant} {form_kw} vs exact")
    assert ops.pointmlp3_pair_recheck_ready(dev)          # so recheck="pair" ran the pair kernel, not its fall-back
    dbg = {}
    ops.pointmlp3_max_fwd_raw(x, wp, False, screen_dbg=dbg, recheck="pair", **kw)
    assert forms["pc3d_pointmlp3_max_fwd_f32"][-1][FWD_FORM_ARG] == H_PAIR
    rechecked, fell = (int(v) for v in dbg["stats"].sum(dim=(0, 1)))       # a screened block rechecks >= 1 point per channel
    assert rechecked >= 32 * (B * 2 * (C3 // 32) - fell) and fell < B * 2 * (C3 // 32)
    assert set(forms) == {"pc3d_pointmlp3_max_fwd_f32"}


def _tower_state(ops, case, T):
    x, wp = case["x"], case["wp"]
    _, argidx, masks = ops.pointmlp3_max_fwd_raw(x, wp, False, T=T, want_masks=True, exact=True)
    return x, tuple(wp[:7]), argidx, masks


def test_backward_forms(ops, forms, case):
    x, w, argidx, masks = _tower_state(ops, case, case["T"])
    ref = None
    for form_kw, want in [(dict(), DEFAULT), (dict(tile32=True), TILE32), (dict(tile32=False), PACKED),
                          (dict(twolist=True), TWOLIST)]:
        got = ops.pointmlp3_max_bwd_raw(x, w, argidx, case["g"], masks, T=case["T"], want_gT=True, **form_kw)
        args = forms["pc3d_pointmlp3_max_bwd_f32"][-1]
        assert args[BWD_FORM_ARG] == want and args[BWD_FORM_ARG + 1] == 0, (form_kw, args[BWD_FORM_ARG:])
        torch.cuda.synchronize()
        assert got[1].shape == (B, (N + 31) // 32, 16)
        ref = ref or got
        _same(ref, got, f"backward {form_kw} vs the default form")
    assert float(ref[0].abs().max()) > 0 and float(ref[1].abs().max()) > 0


def test_backward_update_forms(ops, dev, forms, case):
    x, w, argidx, masks = _tower_state(ops, case, None)
    gen = torch.Generator().manual_seed(77)

    def r(*s):
        return torch.randn(*s, generator=gen).to(dev)
    state = dict(adv=x, ori=x + 0.05 * r(*x.shape), m=1e-3 * r(*x.shape), v=1e-6 * r(*x.shape).abs(), gx=r(*x.shape))
    wts = (torch.rand(B, generator=gen) * 20 + 1).to(dev)
    nn_idx = torch.randint(0, N, (B, N), generator=gen).to(dev).to(torch.int32)
    adam = torch.tensor([0.01, 1.7], device=dev)
    ref = None
    for tile32, want in [(None, DEFAULT), (True, TILE32), (False, PACKED)]:
        s = {k: v.clone() for k, v in state.items()}
        ops.pointmlp3_max_bwd_update(s["adv"], w, argidx, case["g"], masks, s["gx"], s["ori"], s["m"], s["v"], adam, 0.18,
                                     dist_kind=2, w=wts, nn_idx=nn_idx, tile32=tile32)
        assert forms["pc3d_pointmlp3_max_bwd_update_f32"][-1][UPD_FORM_ARG] == want, tile32
        torch.cuda.synchronize()
        got = [s["adv"], s["m"], s["v"]]
        ref = ref or got
        _same(ref, got, f"update tile32={tile32} vs the default form")
        assert torch.equal(s["gx"], state["gx"])                          # gx is only read
    assert not torch.equal(ref[0], x)
