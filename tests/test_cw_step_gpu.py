"""GPU: every form of the CW iteration's device-side update against an independent float64 step.

ops.cw_update (pc3d_cw_update_f32, every cw_update_kernel<PER>), ops.cw_bookkeep + ops.cw_step (the two-launch path, the
only one past 8192 points) and ops.adam_clip_step are held to tests/cw_step_restatement.py — the reference's own
statements with a real torch.optim.Adam, tied to oracle.ref_torch.cw_attack bit for bit by tests/test_cw_step_cpu.py —
evaluated in float64 on the CPU. The riders (test_cw_riders_gpu.py) are bit-equal to cw_update, so this anchors them too.

Bound, per output and per case, from the reference alone: 16 x the largest deviation of the fp32 restatement from the
float64 one on the case's own inputs, floor 16 x 2^-24 x max|ref| (rs.bands). Integer state, the copies and the
sentinels are held to equality, bit for bit. Every case prints kernel error / band.

Largest kernel error / band measured on the MI355X over all cases: 0.145 for the CW step (v at K = 2048, L2 term,
cw_update; adv never above 0.07) and 0.070 for adam_clip_step. Most cases sit at 0.0625 = 1/16: the kernel is then as far
from float64 as the fp32 restatement is, which is what a build with -ffp-contract=off should give.
"""
import functools
import importlib

import pytest
import torch

import cw_step_restatement as rs

pytestmark = pytest.mark.gpu
ops = importlib.import_module("3dpointcloudattack_amd.ops")

KS = [1, 333, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192]     # both sides of every PER switch
FORMS = [(K, f) for K in KS for f in ("update", "two_launch")] + [(8193, "two_launch"), (9000, "two_launch")]
NAN_WORD = 0x7FC00ABC            # a quiet NaN with a payload: survives only if nobody writes the word
INT_PAD = -0x5A5A5A5A
POINTS = ("adv", "ori", "g", "m", "v", "o_bestattack", "input_val")
VECTORS = ("pred", "label", "bestdist", "bestscore", "o_bestdist", "o_bestscore", "w", "dist_val")
WRITTEN = ("adv", "m", "v", "dist_val", "bestdist", "bestscore", "o_bestdist", "o_bestscore", "o_bestattack", "input_val")


def _nan_fill(shape, dev):
    return torch.full(shape, NAN_WORD, dtype=torch.int32, device=dev).view(torch.float32)


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t.contiguous()


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _is_sentinel(t):
    return bool((_bits(t) == NAN_WORD).all())


@functools.lru_cache(maxsize=None)
def _nn(K, far, dev):
    inp = rs.inputs(K, far=far)
    return rs.nn_f64(inp["adv"].to(dev), inp["ori"].to(dev)).cpu()


@functools.lru_cache(maxsize=None)
def _reference(K, dist_kind, untarget, nn_kind, far, dev):
    """(nn_idx or None, float64 restatement, bands) of the case, computed once and shared by every layout and form."""
    inp = rs.inputs(K, far=far)
    nn = None
    if dist_kind == 2:
        nn = inp["rand_idx"] if nn_kind == "random" else _nn(K, far, dev)
    r64 = rs.run(torch.float64, inp, untarget, dist_kind, nn_idx=nn)
    r32 = rs.run(torch.float32, inp, untarget, dist_kind, nn_idx=nn)
    for k in rs.INT_OUT + ("copied",):
        assert torch.equal(r64[k], r32[k]), "a decision of the case sits at rounding distance"
    # the reference's own spelling, through min over [B,K,K] (not the far point: its |x|^2 + |y|^2 - 2xy cancels at 1e12)
    if dist_kind == 2 and nn_kind == "argmin" and K <= 1025 and not far:
        own = rs.run(torch.float64, inp, untarget, 2, spelling="min")
        for k in rs.FLOAT_OUT:
            assert float((own[k] - r64[k]).abs().max()) <= 1e-12, k
    return nn, r64, rs.bands(r64, r32)


def _lay(t, cf, dev):
    """[B,3,K] on the device as a fresh contiguous [B,3,K] (cf) or [B,K,3] tensor."""
    if t is None:
        return None
    t = t.to(dev)
    return t.clone() if cf else torch.empty(t.shape[0], t.shape[2], 3, device=dev).copy_(t.transpose(1, 2))


def _state(inp, dev, cf):
    """The case on the device in the given layout, outputs prefilled with the payload NaN."""
    s = {k: _lay(inp[k], cf, dev) for k in ("adv", "ori", "g", "m", "v")}
    s.update({k: inp[k].to(dev) for k in VECTORS if k != "dist_val"})
    s["o_bestattack"], s["input_val"] = _nan_fill(s["adv"].shape, dev), _nan_fill(s["adv"].shape, dev)
    s["dist_val"] = _nan_fill((s["adv"].shape[0],), dev)
    return {k: v.clone() for k, v in s.items()}


def _launch(s, form, untarget, dist_kind, nn_idx, cf, step_as, t=rs.T, budget=rs.BUDGET):
    """One iteration through `form`, in place on s. The step number reaches the update as the device word or as an int."""
    dev = s["adv"].device
    if nn_idx is not None:
        nn_idx = nn_idx.to(dev)
    if form == "update":
        word = torch.full((1,), t, dtype=torch.int32, device=dev)
        ops.cw_update(s["adv"], s["ori"], s["pred"], s["label"], untarget, s["bestdist"], s["bestscore"], s["o_bestdist"],
                      s["o_bestscore"], s["o_bestattack"], s["g"], s["m"], s["v"], word if step_as == "word" else t, rs.LR, budget,
                      input_val=s["input_val"], dist_val=s["dist_val"], dist_kind=dist_kind, w=s["w"], nn_idx=nn_idx,
                      betas=rs.BETAS, eps=rs.EPS, cf=cf)
    else:
        word = torch.full((1,), t - 1, dtype=torch.int32, device=dev)
        ops.cw_bookkeep(s["adv"], s["ori"], s["pred"], s["label"], untarget, s["bestdist"], s["bestscore"], s["o_bestdist"],
                        s["o_bestscore"], s["o_bestattack"], input_val=s["input_val"], dist_val=s["dist_val"], step=word, cf=cf)
        ops.cw_step(s["adv"], s["g"], s["m"], s["v"], word if step_as == "word" else t, rs.LR, s["ori"], budget,
                    dist_kind=dist_kind, w=s["w"], l2norm=s["dist_val"], nn_idx=nn_idx, betas=rs.BETAS, eps=rs.EPS, cf=cf)
    # cw_update only reads the word; cw_bookkeep advances it once per launch, whatever B is
    assert int(word) == t
    return s


def _cf_view(t, cf):
    return t if cf or t.dim() != 3 else t.transpose(1, 2)


def _check_copies(s, before, copied, cf):
    """input_val is the old iterate; o_bestattack is the old iterate on the copied samples and untouched elsewhere."""
    assert _same_bits(s["input_val"], before)
    for b, c in enumerate(copied.tolist()):
        if c:
            assert _same_bits(s["o_bestattack"][b], before[b]), b
        else:
            assert _is_sentinel(s["o_bestattack"][b]), b


def _check(s, before, r64, band, cf, tag):
    ratios = {}
    for k in rs.FLOAT_OUT:
        err = float((_cf_view(s[k], cf).double().cpu() - r64[k]).abs().max())
        ratios[k] = err / band[k] if band[k] > 0 else (0. if err == 0 else float("inf"))
    print(f"cw_step_band {tag}: " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()) + f" worst={max(ratios.values()):.3f}")
    for k, v in ratios.items():
        assert v <= 1., (k, v)            # also fails on NaN
    for k in rs.INT_OUT:
        assert torch.equal(s[k].cpu(), r64[k]), k
    _check_copies(s, before, r64["copied"], cf)


def _case(dev, K, dist_kind, untarget, cf, form, nn_kind="argmin", far=False):
    inp = rs.inputs(K, far=far)
    nn, r64, band = _reference(K, dist_kind, untarget, nn_kind, far, dev)
    s = _state(inp, dev, cf)
    before = s["adv"].clone()
    _launch(s, form, untarget, dist_kind, nn, cf, "word")
    _check(s, before, r64, band, cf, f"K={K} kind={dist_kind} untarget={int(untarget)} cf={int(cf)} {form} nn={nn_kind} far={int(far)}")
    host = _launch(_state(inp, dev, cf), form, untarget, dist_kind, nn, cf, "int")
    for k in WRITTEN:
        assert _same_bits(host[k], s[k]), k        # the step number as a host int: the same bits
    for k in ("ori", "g", "pred", "label", "w"):
        assert _same_bits(s[k], _state(inp, dev, cf)[k]), k          # inputs are only read


# that 20 % .. 80 % of every case's points lie past the budget before the clip, and that its decisions are a mix, is
# asserted on the reference alone by test_cw_step_cpu.py::test_inputs_are_not_tame (no GPU needed)
@pytest.mark.parametrize("cf", [True, False])
@pytest.mark.parametrize("untarget", [True, False])
@pytest.mark.parametrize("dist_kind", [0, 1, 2])
@pytest.mark.parametrize("K,form", FORMS)
def test_step_against_float64(dev, K, form, dist_kind, untarget, cf):
    _case(dev, K, dist_kind, untarget, cf, form)


@pytest.mark.parametrize("cf", [True, False])
@pytest.mark.parametrize("K,form", [(333, "update"), (2049, "update"), (2049, "two_launch"), (8192, "update"), (9000, "two_launch")])
def test_chamfer_term_uses_the_index_it_is_given(dev, K, form, cf):
    _case(dev, K, 2, True, cf, form, nn_kind="random")


@pytest.mark.parametrize("dist_kind", [0, 1, 2])
@pytest.mark.parametrize("K,form", [(333, "update"), (2049, "update"), (2049, "two_launch")])
def test_far_point_clip(dev, K, form, dist_kind):
    """One point 1e6 away from its original: the clip's scale is 1.7e-7, the only place where the `+ 1e-9` inside its
    division shows in the result (test_cw_step_cpu.py: the misplaced epsilon is 700 bands away on this case)."""
    _case(dev, K, dist_kind, True, True, form, far=True)


# ----------------------------------------------------------------------------------------------------------------------
# windows of larger buffers
# ----------------------------------------------------------------------------------------------------------------------
def _window(t, left, pad, dev):
    buf = _nan_fill(t.shape[:2] + (t.shape[2] + pad,), dev)
    win = buf[:, :, left:left + t.shape[2]]
    win.copy_(t)
    return buf, win


def _vec_window(t, dev):
    if t.dtype == torch.float32:
        buf = _nan_fill((t.shape[0] + 2,), dev)
    else:
        buf = torch.full((t.shape[0] + 2,), INT_PAD, dtype=t.dtype, device=dev)
    buf[1:1 + t.shape[0]].copy_(t)
    return buf, buf[1:1 + t.shape[0]]


@pytest.mark.parametrize("form", ["update", "two_launch"])
@pytest.mark.parametrize("dist_kind", [1, 2])
@pytest.mark.parametrize("K", [333, 1025, 4097])
def test_windows_of_larger_buffers(dev, K, dist_kind, form):
    """Every tensor a window of a sentinel-filled buffer, g and ori with strides of their own: the same bits as the
    contiguous run, and no pad word touched."""
    inp = rs.inputs(K)
    nn = _nn(K, False, dev) if dist_kind == 2 else None
    ref = _launch(_state(inp, dev, True), form, True, dist_kind, nn, True, "word")
    plain = _state(inp, dev, True)
    bufs, s = {}, {}
    for k in POINTS:
        left, pad = {"g": (5, 16), "ori": (7, 12)}.get(k, (3, 8))
        bufs[k], s[k] = _window(plain[k], left, pad, dev)
        bufs[k] = (bufs[k], left)
    for k in VECTORS:
        buf, s[k] = _vec_window(plain[k], dev)
        bufs[k] = (buf, 1)
    assert s["g"].stride() != s["adv"].stride() != s["ori"].stride() and s["m"].stride() == s["adv"].stride()
    _launch(s, form, True, dist_kind, nn, True, "word")
    for k in WRITTEN:
        assert _same_bits(s[k], ref[k]), k
    for k, (buf, left) in bufs.items():
        n = s[k].shape[-1]
        pads = torch.cat([buf[..., :left].reshape(-1), buf[..., left + n:].reshape(-1)])
        assert bool((_bits(pads) == (NAN_WORD if buf.dtype == torch.float32 else INT_PAD)).all()), k


def test_cw_update_refuses_state_with_other_strides(dev):
    inp = rs.inputs(333)
    s = _state(inp, dev, True)
    for k in ("m", "v", "o_bestattack", "input_val"):
        t = dict(s)
        t[k] = _window(s[k], 3, 8, dev)[1]
        with pytest.raises(ValueError, match=f"{k} must share adv's shape and strides"):
            _launch(t, "update", True, 1, None, True, "word")


# ----------------------------------------------------------------------------------------------------------------------
# batch order, NaN cloud
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["update", "two_launch"])
@pytest.mark.parametrize("dist_kind", [1, 2])
def test_batch_order(dev, dist_kind, form):
    """B enters the arithmetic through w / B, so the invariant is: permuting the samples permutes the outputs, bit for bit."""
    K = 2049
    inp = rs.inputs(K)
    nn = _nn(K, False, dev) if dist_kind == 2 else None
    a = _launch(_state(inp, dev, True), form, True, dist_kind, nn, True, "word")
    perm = torch.tensor([2, 0, 1], device=dev)
    b = {k: v[perm].contiguous() for k, v in _state(inp, dev, True).items()}
    _launch(b, form, True, dist_kind, None if nn is None else nn[perm.cpu()].contiguous(), True, "word")
    for k in WRITTEN:
        assert _same_bits(b[k], a[k][perm]), k


@pytest.mark.parametrize("form", ["update", "two_launch"])
@pytest.mark.parametrize("dist_kind", [1, 2])
def test_nan_cloud(dev, dist_kind, form):
    """One sample's iterate all NaN: its bests and its best attack stay, its distance is NaN, and the other samples get the
    bits of the run without it."""
    K = 2049
    inp = rs.inputs(K)
    nn = _nn(K, False, dev) if dist_kind == 2 else None
    clean = _launch(_state(inp, dev, True), form, True, dist_kind, nn, True, "word")
    assert bool(rs.run(torch.float64, inp, True, dist_kind, nn_idx=nn)["copied"][1])      # sample 1 would have been copied
    s = _state(inp, dev, True)
    s["adv"][1] = float("nan")
    start = {k: v.clone() for k, v in s.items()}
    _launch(s, form, True, dist_kind, nn, True, "word")
    for k in ("bestdist", "bestscore", "o_bestdist", "o_bestscore", "o_bestattack"):
        assert _same_bits(s[k][1], start[k][1]), k
    assert bool(torch.isnan(s["dist_val"][1])) and bool(torch.isnan(s["adv"][1]).all())
    others = torch.tensor([0, 2], device=dev)
    for k in WRITTEN:
        assert _same_bits(s[k][others], clean[k][others]), k


# ----------------------------------------------------------------------------------------------------------------------
# decisions at exact ties
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["update", "two_launch"])
@pytest.mark.parametrize("untarget", [True, False])
@pytest.mark.parametrize("K", [333, 2049, 8192])
def test_decisions_at_exact_ties(dev, K, untarget, form):
    """The distance is exact in any summation order (rs.tie_inputs), so `<` against an equal best must not fire."""
    inp = rs.tie_inputs(K, untarget)
    r64 = rs.run(torch.float64, inp, untarget, 0)
    s = _state(inp, dev, True)
    before = s["adv"].clone()
    _launch(s, form, untarget, 0, None, True, "word")
    assert s["dist_val"].cpu().tolist() == [rs.TIE_DIST] * 5
    for k in ("bestdist", "o_bestdist"):
        assert torch.equal(s[k].double().cpu(), r64[k]), k
    for k in rs.INT_OUT:
        assert torch.equal(s[k].cpu(), r64[k]), k
    assert r64["copied"].tolist() == [True, True, False, False, False]
    assert (r64["bestscore"] != -1).tolist() == [False, True, True, True, False]
    _check_copies(s, before, r64["copied"], True)


# ----------------------------------------------------------------------------------------------------------------------
# adam_clip_step
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["none", "linf", "normal", "normal_budget0"])
@pytest.mark.parametrize("with_g2", [False, True])
@pytest.mark.parametrize("cf", [True, False])
@pytest.mark.parametrize("K", [1, 300, 1025])
def test_adam_clip_step_against_float64(dev, K, cf, with_g2, mode):
    inp = rs.adam_clip_inputs(K)
    budget = rs.BUDGET if mode in ("linf", "normal") else 0.
    ori = None if mode == "none" else inp["ori"]
    normal = inp["normal"] if mode.startswith("normal") else None
    g2 = inp["g2"] if with_g2 else None
    r64, r32 = (rs.adam_clip(dt, inp["p"], inp["g"], g2, inp["m"], inp["v"], rs.T, rs.LR, ori, normal, budget)
                for dt in (torch.float64, torch.float32))
    keep = None
    if normal is not None:      # the projection's two branches: only the points the float64 reference decides beyond rounding
        keep = rs.projection_keep(r64["stepped"], ori, normal)
        assert float((~keep).double().mean()) <= 0.01
        assert bool(keep[:, K:].all())
        keep = keep[:, None, :].expand(-1, 3, -1)
    band = rs.bands(r64, r32, names=("p", "m", "v"), keep=keep)

    def lay(t):
        return _lay(t, cf, dev)

    outs = []
    for step in (torch.full((1,), rs.T, dtype=torch.int32, device=dev), rs.T):
        p, m, v = lay(inp["p"]), lay(inp["m"]), lay(inp["v"])
        ops.adam_clip_step(p, lay(inp["g"]), m, v, step, rs.LR, betas=rs.BETAS, eps=rs.EPS, ori=lay(ori), normal=lay(normal),
                           budget=budget, cf=cf, g2=lay(g2))
        outs.append((p, m, v))
    for a, b in zip(*outs):
        assert _same_bits(a, b)
    ratios = {}
    for k, t in zip(("p", "m", "v"), outs[0]):
        d = (_cf_view(t, cf).double().cpu() - r64[k]).abs()
        if keep is not None and k == "p":
            d = d[keep]
        ratios[k] = float(d.max()) / band[k]
    print(f"adam_clip_band K={K} cf={int(cf)} g2={int(with_g2)} {mode}: " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items())
          + f" worst={max(ratios.values()):.3f}")
    for k, r in ratios.items():
        assert r <= 1., (k, r)
    # the constructed rows: Adam moves them by exactly 0; the "opposite" branch then puts them onto ori, anything else
    # leaves them where they were
    tail = _cf_view(outs[0][0], cf)[:, :, K:].cpu()
    assert _same_bits(tail, (inp["ori"] if normal is not None else inp["p"])[:, :, K:])
