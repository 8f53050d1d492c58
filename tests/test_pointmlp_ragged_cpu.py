"""CPU: the two tower entries that take per-cloud lengths (include/pc3d.h: pc3d_pointmlp3_max_fwd_ragged_f32 and
pc3d_pointmlp3_max_bwd_ragged_f32). Their argument rules are checked before any HIP call — every data pointer below is
NULL, so nothing here can reach a launch —, ops chooses the ragged forward's form by one pure function, checked against a
restatement over every combination of its inputs, and the options that name a launch without a ragged twin are refused."""
import ctypes
import itertools

import pytest
import torch

from test_pointmlp_abi_cpu import _bwd, _fwd, DEFAULT, EXACT, H, H_PAIR, HEAD, IMG3, IMG5, PACKED, PREP, PTR, SCREEN, TILE32, \
    TWOLIST

FWD, BWD = "pc3d_pointmlp3_max_fwd_ragged_f32", "pc3d_pointmlp3_max_bwd_ragged_f32"


def _fwd_r(lengths=PTR, **kw):
    """The ragged forward's arguments: the dense entry's (test_pointmlp_abi_cpu._fwd, the exact form) with lengths in front
    of the stream."""
    a = _fwd(**dict(dict(form=EXACT), **kw))
    return a[:-1] + [lengths, a[-1]]


def _bwd_r(lengths=PTR, **kw):
    a = _bwd(**kw)
    return a[:-1] + [lengths, a[-1]]


@pytest.mark.parametrize("kw, fragment", [
    (dict(lengths=None), b"lengths [B] is required"),
    (dict(lengths=None, B=0), b"lengths [B] is required"),
    (dict(form=SCREEN), b"form 1 has no ragged twin"),
    (dict(form=PREP, **IMG3), b"form 2 has no ragged twin"),
    (dict(form=H, **IMG5), b"form 3 has no ragged twin"),
    (dict(form=5), b"form 5 has no ragged twin"),
    (dict(form=-1), b"form -1 has no ragged twin"),
    (dict(form=H_PAIR, **dict(IMG5, w3_h=None)), b"both prepared images"),
    (dict(form=H_PAIR, **dict(IMG5, w3_cw=None)), b"both prepared images"),
    (dict(form=H_PAIR, **dict(IMG5, w3_q=None)), b"both prepared images"),
    (dict(form=H_PAIR, **IMG3), b"both prepared images"),
    (dict(form=H_PAIR, stats=PTR, **IMG5), b"belong to the dense entry's debug launch"),
    (dict(form=H_PAIR, stats=PTR, dbg_S=PTR, dbg_E=PTR, **IMG5), b"belong to the dense entry's debug launch"),
    (dict(dbg_S=PTR, dbg_E=PTR), b"belong to the dense entry's debug launch"),
    (dict(stop_after=1), b"belong to the dense entry's debug launch"),
    (dict(form=H_PAIR, stop_after=3, **IMG5), b"belong to the dense entry's debug launch"),
    (dict(HEAD, T=PTR), b"not both"),
    (dict(HEAD, T_out=None), b"complete transform head"),
], ids=["no_lengths", "no_lengths_B0", "screen", "prep", "h", "form_5", "form_neg", "pair_without_w3_h", "pair_without_w3_cw",
        "pair_without_w3_q", "pair_bf16_image_only", "stats", "stats_dump", "dump", "stop_after_exact", "stop_after_pair",
        "th_in_with_T", "th_in_without_T_out"])
def test_forward_rules(pc3d, kw, fragment):
    lib = pc3d.load()
    assert lib.pc3d_pointmlp3_max_fwd_ragged_f32(*_fwd_r(**kw)) == -22
    err = lib.pc3d_last_error()
    assert FWD.encode() + b":" in err and fragment in err, err


@pytest.mark.parametrize("kw", [dict(form=EXACT), dict(form=EXACT, **IMG5), dict(form=H_PAIR, **IMG5), dict(HEAD), dict(T=PTR)])
def test_forward_legal_arguments_reach_the_data_pointers(pc3d, kw):
    """What the rules allow gets as far as the check of the data pointers (all NULL here), and, with B = 0, returns 0."""
    lib = pc3d.load()
    assert lib.pc3d_pointmlp3_max_fwd_ragged_f32(*_fwd_r(**kw)) == -22
    assert lib.pc3d_last_error().endswith(FWD.encode() + b": null pointer")
    assert lib.pc3d_pointmlp3_max_fwd_ragged_f32(*_fwd_r(B=0, **kw)) == 0        # an empty batch is a no-op


def test_backward_rules(pc3d):
    lib = pc3d.load()
    for kw, fragment in [(dict(lengths=None), b"lengths [B] is required"),
                         (dict(lengths=None, B=0), b"lengths [B] is required"),
                         (dict(form=TILE32), b"form 2 has no ragged twin"), (dict(form=TWOLIST), b"form 3 has no ragged twin"),
                         (dict(form=4), b"form 4 has no ragged twin"), (dict(form=-1), b"form -1 has no ragged twin"),
                         (dict(form=PACKED, stop_after=2), b"stop_after = 2"), (dict(form=DEFAULT, stop_after=5), b"stop_after = 5"),
                         (dict(stop_after=-1), b"stop_after = -1")]:
        assert lib.pc3d_pointmlp3_max_bwd_ragged_f32(*_bwd_r(**kw)) == -22, kw
        err = lib.pc3d_last_error()
        assert BWD.encode() + b":" in err and fragment in err, (kw, err)
    for kw in [dict(form=DEFAULT), dict(form=PACKED), dict(form=PACKED, accumulate=1, T=PTR, part_gT=PTR)]:
        assert lib.pc3d_pointmlp3_max_bwd_ragged_f32(*_bwd_r(**kw)) == -22, kw
        assert lib.pc3d_last_error().endswith(BWD.encode() + b": null pointer"), kw
        assert lib.pc3d_pointmlp3_max_bwd_ragged_f32(*_bwd_r(B=0, **kw)) == 0, kw


def test_signatures_are_the_dense_ones_with_lengths_before_the_stream(ops):
    sig = ops._lib.SIGNATURES
    for dense, ragged in (("pc3d_pointmlp3_max_fwd_f32", FWD), ("pc3d_pointmlp3_max_bwd_f32", BWD)):
        assert sig[ragged] == sig[dense][:-1] + [ctypes.c_void_p, sig[dense][-1]]


def _expected_ragged_form(exact, image):
    """pointmlp3_max_fwd_raw's docstring on lengths, restated."""
    if exact:
        return EXACT
    return H_PAIR if image == "both" else EXACT


def test_ragged_form_selector_table(ops):
    seen = set()
    for exact, image in itertools.product((False, True), ("none", "bf16 only", "both")):
        want = _expected_ragged_form(exact, image)
        assert ops._pm_fwd_form_ragged(exact, image != "none", image == "both") == want, (exact, image)
        seen.add(want)
    assert seen == {EXACT, H_PAIR}
    # (have_h_image without have_image does not occur: the fp16 image lies behind the bf16 one)
    assert ops._pm_fwd_form_ragged(False, False, True) == EXACT


LENS = torch.ones(2, dtype=torch.int32)
X = torch.zeros(2, 3, 8)       # a CPU tensor: a call that got past the refusal would fail on it with another error


@pytest.mark.parametrize("kw, named", [
    (dict(in_launch=True), ["in_launch"]), (dict(form="bf16"), ["form='bf16'"]), (dict(recheck="channel"), ["recheck='channel'"]),
    (dict(screen_dbg={}), ["screen_dbg"]), (dict(serial=True), ["serial"]),
    (dict(form="fp16", recheck="channel"), ["recheck='channel'"]), (dict(exact=True, serial=True), ["serial"]),
    (dict(in_launch=True, screen_dbg={"dump": True}), ["in_launch", "screen_dbg"])])
def test_forward_options_without_a_ragged_twin_are_refused(ops, kw, named):
    with pytest.raises(ValueError) as ei:
        ops.pointmlp3_max_fwd_raw(X, [None] * 6, False, lengths=LENS, **kw)
    assert "no ragged twin" in str(ei.value)
    assert str(ei.value).endswith(" for " + ", ".join(named)), str(ei.value)


@pytest.mark.parametrize("kw", [dict(twolist=True), dict(tile32=True), dict(tile32=False, stop_after=3)])
def test_backward_options_without_a_ragged_twin_are_refused(ops, kw):
    with pytest.raises(ValueError) as ei:
        ops.pointmlp3_max_bwd_raw(X, [None] * 7, None, None, (None, None), lengths=LENS, **kw)
    assert "lengths go with the packed form only" in str(ei.value)


def test_victim_declares_fused_lengths(pc3d):
    import importlib
    pn = importlib.import_module(pc3d.__name__ + ".model.pointnet")
    assert pn.PointNetCls(k=4).fused_lengths is True
    ft = pn.PointNetCls(k=4, feature_transform=True)
    assert ft.fused_lengths is False
    with pytest.raises(ValueError) as ei:           # refused before anything touches the device
        pn.fused_forward(ft, X, lengths=LENS)
    assert "fused_lengths" in str(ei.value)
