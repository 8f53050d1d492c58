"""CPU: the PointNet tower's three launch entries take the kernel form as an argument (include/pc3d.h). Their argument
rules are checked before any HIP call — every data pointer below is NULL, so nothing here can reach a launch — and
ops chooses the forward's form by one pure function, checked here against the rules of pointmlp3_max_fwd_raw's docstring
over every combination of its inputs."""
import ctypes
import itertools

import pytest

EXACT, SCREEN, PREP, H, H_PAIR = range(5)              # PC3D_PM_FWD_*
DEFAULT, PACKED, TILE32, TWOLIST = range(4)            # PC3D_PM_BWD_*

_BUF = ctypes.create_string_buffer(64)
PTR = ctypes.addressof(_BUF)                           # a non-null optional pointer; no rule lets a launch read it


def _fwd(**kw):
    """pc3d_pointmlp3_max_fwd_f32's arguments: B = 1, N = 4, legal widths, every pointer NULL, the in-launch form."""
    a = dict(x=None, x_bs=0, x_ps=0, x_cs=0, B=1, N=4, T=None, th_in=None, th_W=None, th_b=None, th_K=0, T_out=None,
             W1=None, b1=None, W2=None, b2=None, W3=None, b3=None, C1=64, C2=128, C3=64, relu_last=0, part_val=None,
             part_idx=None, pooled=None, argidx=None, mask1=None, mask2=None, form=SCREEN, w3_bf=None, w3_nw=None,
             w3_q=None, w3_h=None, w3_cw=None, stats=None, dbg_S=None, dbg_E=None, stop_after=0, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return list(a.values())


def _bwd(**kw):
    a = dict(x=None, x_bs=0, x_ps=0, x_cs=0, B=1, N=4, T=None, W1=None, b1=None, W2=None, b2=None, W3=None, W2T=None,
             C1=64, C2=128, C3=64, argidx=None, mask1=None, mask2=None, g_pooled=None, grad_x=None, gx_bs=0, gx_ps=0,
             gx_cs=0, part_gT=None, accumulate=0, form=DEFAULT, stop_after=0, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return list(a.values())


def _upd(**kw):
    a = dict(x=None, x_bs=0, x_ps=0, x_cs=0, B=1, N=4, W1=None, b1=None, W2=None, b2=None, W3=None, W2T=None, C1=64,
             C2=128, C3=64, argidx=None, mask1=None, mask2=None, g_pooled=None, grad_x=None, gx_bs=0, gx_ps=0, gx_cs=0,
             ori=None, o_bs=0, o_ps=0, o_cs=0, m=None, v=None, beta1=0.9, beta2=0.999, eps=1e-8, budget=0.0, adam=None,
             dist_kind=0, w=None, dist_val=None, nn_idx=None, form=DEFAULT, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return list(a.values())


IMG3 = dict(w3_bf=PTR, w3_nw=PTR, w3_q=PTR)
IMG5 = dict(IMG3, w3_h=PTR, w3_cw=PTR)
HEAD = dict(th_in=PTR, th_W=PTR, th_b=PTR, th_K=8, T_out=PTR)


@pytest.mark.parametrize("kw, fragment", [
    (dict(form=5), b"unknown form 5"),
    (dict(form=-1), b"unknown form -1"),
    (dict(form=PREP, **dict(IMG3, w3_q=None)), b"w3_bf, w3_nw and w3_q"),
    (dict(form=H_PAIR, **dict(IMG5, w3_h=None)), b"both prepared images"),
    (dict(HEAD, T=PTR), b"not both"),
    (dict(HEAD, T_out=None), b"complete transform head"),
    (dict(stats=PTR, dbg_S=PTR), b"dbg_S and dbg_E go together"),
    (dict(dbg_S=PTR, dbg_E=PTR), b"which stats"),
    (dict(stats=PTR, stop_after=4), b"stop_after = 4"),
    (dict(stop_after=1), b"which stats"),
    (dict(form=EXACT, stats=PTR), b"stats belongs to a screened form"),
], ids=["form_5", "form_neg", "prep_without_w3_q", "h_pair_without_w3_h", "th_in_with_T", "th_in_without_T_out",
        "dbg_S_without_dbg_E", "dbg_S_without_stats", "stop_after_4", "stop_after_1_without_stats", "exact_with_stats"])
def test_forward_rules(pc3d, kw, fragment):
    lib = pc3d.load()
    assert lib.pc3d_pointmlp3_max_fwd_f32(*_fwd(**kw)) == -22
    assert fragment in lib.pc3d_last_error()


@pytest.mark.parametrize("kw", [dict(form=EXACT), dict(form=SCREEN), dict(form=PREP, **IMG3), dict(form=H, **IMG5),
                                dict(form=H_PAIR, **IMG5), dict(form=H_PAIR, stats=PTR, dbg_S=PTR, dbg_E=PTR, stop_after=3, **IMG5),
                                dict(HEAD), dict(T=PTR), dict(T=PTR, th_W=PTR, th_K=-3)])
def test_forward_legal_arguments_reach_the_data_pointers(pc3d, kw):
    """What the rules allow gets as far as the check of the data pointers (all NULL here), and, with B = 0, returns 0."""
    lib = pc3d.load()
    assert lib.pc3d_pointmlp3_max_fwd_f32(*_fwd(**kw)) == -22
    assert lib.pc3d_last_error().endswith(b"pc3d_pointmlp3_max_fwd_f32: null pointer")
    assert lib.pc3d_pointmlp3_max_fwd_f32(*_fwd(B=0, **kw)) == 0        # an empty batch is a no-op


def test_backward_rules(pc3d):
    lib = pc3d.load()
    for kw, fragment in [(dict(form=4), b"unknown form 4"), (dict(form=-1), b"unknown form -1"),
                         (dict(form=TILE32, stop_after=2), b"stop_after = 2"),
                         (dict(form=DEFAULT, stop_after=2), b"stop_after = 2"),
                         (dict(form=PACKED, stop_after=6), b"stop_after = 6"),
                         (dict(form=PACKED, stop_after=-1), b"stop_after = -1")]:
        assert lib.pc3d_pointmlp3_max_bwd_f32(*_bwd(**kw)) == -22, kw
        assert fragment in lib.pc3d_last_error(), kw
    for kw in [dict(form=f) for f in (DEFAULT, PACKED, TILE32, TWOLIST)] + [dict(form=PACKED, stop_after=s) for s in range(1, 6)]:
        assert lib.pc3d_pointmlp3_max_bwd_f32(*_bwd(**kw)) == -22, kw
        assert lib.pc3d_last_error().endswith(b"pc3d_pointmlp3_max_bwd_f32: null pointer"), kw
        assert lib.pc3d_pointmlp3_max_bwd_f32(*_bwd(B=0, **kw)) == 0, kw


def test_update_rules(pc3d):
    lib = pc3d.load()
    for form in (TWOLIST, 4, -1):
        assert lib.pc3d_pointmlp3_max_bwd_update_f32(*_upd(form=form)) == -22, form
        assert b"unknown form %d" % form in lib.pc3d_last_error(), form
    for form in (DEFAULT, PACKED, TILE32):
        assert lib.pc3d_pointmlp3_max_bwd_update_f32(*_upd(form=form)) == -22, form
        assert lib.pc3d_last_error().endswith(b"pc3d_pointmlp3_max_bwd_update_f32: null pointer"), form
        assert lib.pc3d_pointmlp3_max_bwd_update_f32(*_upd(form=form, B=0)) == 0, form


def _expected_form(exact, in_launch, image, form, recheck, dbg, default_form, default_recheck):
    """pointmlp3_max_fwd_raw's docstring, restated: the form, or the fragment of the ValueError's text."""
    if exact and dbg:
        return "screen_dbg belongs to the screened launch"
    if form == "bf16" and recheck is not None:
        return "recheck belongs to form='fp16'"
    if exact:
        return EXACT
    if in_launch or image == "none":                       # the image is not used / there is none
        return SCREEN
    if form is None:                                       # naming a recheck selects fp16; the debug figures are bf16's
        form = "fp16" if recheck is not None else "bf16" if dbg else default_form
    if form == "bf16" or image == "bf16 only":
        return PREP
    return {"pair": H_PAIR, "channel": H}[recheck or default_recheck]


@pytest.mark.parametrize("default_form, default_recheck", [("fp16", "pair"), ("fp16", "channel"), ("bf16", "pair")])
def test_forward_form_selector_table(ops, monkeypatch, default_form, default_recheck):
    monkeypatch.setattr(ops, "PM_FWD_DEFAULT_FORM", default_form)
    monkeypatch.setattr(ops, "PM_FWD_DEFAULT_RECHECK", default_recheck)
    assert (ops.PM_FWD_EXACT, ops.PM_FWD_SCREEN, ops.PM_FWD_SCREEN_PREP, ops.PM_FWD_SCREEN_H, ops.PM_FWD_SCREEN_H_PAIR) \
        == (EXACT, SCREEN, PREP, H, H_PAIR)
    seen = set()
    for exact, in_launch, image, form, recheck, dbg in itertools.product(
            (False, True), (False, True), ("none", "bf16 only", "both"), (None, "bf16", "fp16"), (None, "channel", "pair"),
            (False, True)):
        case = (exact, in_launch, image, form, recheck, dbg)
        want = _expected_form(*case, default_form, default_recheck)
        args = (exact, in_launch, image != "none", image == "both", form, recheck, dbg)
        if isinstance(want, str):
            with pytest.raises(ValueError) as ei:
                ops._pm_fwd_form(*args)
            assert want in str(ei.value), case
        else:
            assert ops._pm_fwd_form(*args) == want, case
        seen.add(want)
    assert {EXACT, SCREEN, PREP, H, H_PAIR} <= seen and len([s for s in seen if isinstance(s, str)]) == 2


def test_forward_form_selector_refuses_unknown_names(ops):
    for kw, fragment in [(dict(form="fp8", recheck=None), "form is None, 'bf16' or 'fp16'"),
                         (dict(form=None, recheck="lane"), "recheck is None, 'channel' or 'pair'")]:
        for exact in (False, True):                       # validated whichever form runs
            with pytest.raises(ValueError) as ei:
                ops._pm_fwd_form(exact, False, True, True, dbg=False, **kw)
            assert fragment in str(ei.value)


def test_backward_form_map(ops):
    assert (ops.PM_BWD_DEFAULT, ops.PM_BWD_PACKED, ops.PM_BWD_TILE32, ops.PM_BWD_TWOLIST) == (DEFAULT, PACKED, TILE32, TWOLIST)
    assert [ops._pm_bwd_form(False, t) for t in (None, True, False)] == [DEFAULT, TILE32, PACKED]
    assert ops._pm_bwd_form(True, None) == TWOLIST
