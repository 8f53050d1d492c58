"""GPU: the PointNet tower with per-cloud lengths (pc3d_pointmlp3_max_fwd_ragged_f32 / _bwd_ragged_f32, include/pc3d.h),
from the two kernels up to the ragged CW and kNN loops. No tolerances: a launch given lengths reads no row at or beyond a
length and writes, on the rows below it, the bits of the dense launch on that cloud.

Kernel-level shapes: Kmax = 300 (forward tiles of 128, 128 and 44 points, three packed backward workgroups), B = 8, lengths
300, 257, 256, 129, 128, 33, 32, 1: a full cloud, one point into the last tile, the tile edge, the backward's 32-point
sub-tile edges, a single point. Widths 3 -> 64 -> 128 -> C3 with C3 = 64 and 1024."""
import functools
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import hip_pointnet, unit_cloud
from oracle import ref_torch as ort
from test_pointmlp_screen_prepared_gpu import _packed, _weights

pytestmark = pytest.mark.gpu
M = importlib.import_module
ops = M("3dpointcloudattack_amd.ops")
pointnet = M("3dpointcloudattack_amd.model.pointnet")
graphed = M("3dpointcloudattack_amd.graphed")
cloud_io = M("3dpointcloudattack_amd.dataset.cloud_io")
cwm = M("3dpointcloudattack_amd.attack.CW.CW_attack")
knnm = M("3dpointcloudattack_amd.attack.KNN.KNN_attack")
adv_u = M("3dpointcloudattack_amd.attack.CW.CW_utils.adv_utils")
dist_u = M("3dpointcloudattack_amd.attack.CW.CW_utils.dist_utils")
clip_u = M("3dpointcloudattack_amd.attack.CW.CW_utils.clip_utils")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KMAX, B = 300, 8
LENGTHS = [300, 257, 256, 129, 128, 33, 32, 1]
PERM = [5, 0, 7, 2, 1, 6, 3, 4]
TILE, SUB = 128, 32
SENTINEL = 7.25
EXACT, H_PAIR = 0, 4
FWD, BWD = "pc3d_pointmlp3_max_fwd_ragged_f32", "pc3d_pointmlp3_max_bwd_ragged_f32"
FWD_FORM_ARG = 28
VARIANTS = ("plain", "T", "T_head")


def _lens(lengths, dev):
    return torch.tensor(lengths, dtype=torch.int32, device=dev)


def _eq(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


@functools.lru_cache(maxsize=None)
def _case(C3, n, dev):
    """Weights (with an empty list for the prepared image, filled by the first eager launch), a batch [B,3,n], T, the
    transform head's operands and an upstream gradient: shared, never modified."""
    g = torch.Generator().manual_seed(1000 * C3 + n)
    hk = 256
    c = dict(wp=_packed(_weights(dev, C3, n + C3)), x=(torch.randn(B, 3, n, generator=g) * 0.5).to(dev),
             T=(torch.eye(3)[None] + 0.3 * torch.randn(B, 3, 3, generator=g)).to(dev),
             T_head=(torch.randn(B, hk, generator=g).to(dev), (torch.randn(9, hk, generator=g) / hk ** 0.5).to(dev),
                     torch.eye(3).reshape(9).to(dev)),
             g=torch.randn(B, C3, generator=g).to(dev))
    ops.pointmlp3_max_fwd_raw(c["x"], c["wp"], False)       # one eager call before any capture: the prepared image
    assert len(c["wp"][7]) == 4
    return c


def _nan_beyond(x, lengths):
    x = x.clone()
    for b, L in enumerate(lengths):
        x[b, :, L:] = float("nan")
    return x


def _rows(idx, c, variant):
    """The per-cloud operands of `variant` for the clouds idx (a slice or an index list)."""
    if variant == "T":
        return dict(T=c["T"][idx].contiguous())
    if variant == "T_head":
        h, W, b = c["T_head"]
        return dict(T_head=(h[idx].contiguous(), W, b))
    return {}


def _run(x, c, relu_last, variant, exact, lengths=None, idx=slice(None), partials=False):
    """Forward and both backwards (store and accumulate into a sentinel) of the tower on x. A dict of every output."""
    kw = dict(_rows(idx, c, variant), exact=exact)
    if lengths is not None:
        kw["lengths"] = lengths
    wp, g = c["wp"], c["g"][idx].contiguous()
    out = {}
    res = ops.pointmlp3_max_fwd_raw(x, wp, relu_last, want_masks=True, **kw)
    out["pooled"], out["argidx"], (out["mask1"], out["mask2"]) = res[:3]
    T = kw.get("T")
    if variant == "T_head":
        out["T_out"] = res[3]
        T = res[3].view(-1, 3, 3)
    if partials:
        out["part_val"], out["part_idx"] = ops.pointmlp3_max_fwd_raw(x, wp, relu_last, fold=False, **kw)[:2]
    if relu_last:
        g = g * (out["pooled"] > 0)
    bkw = dict(T=T, want_gT=T is not None) if T is not None else {}
    if lengths is not None:
        bkw["lengths"] = lengths
    masks = (out["mask1"], out["mask2"])
    r = ops.pointmlp3_max_bwd_raw(x, tuple(wp[:7]), out["argidx"], g, masks, **bkw)
    out["gx"], out["part_gT"] = r if T is not None else (r, None)
    acc = torch.full_like(x, SENTINEL)
    ops.pointmlp3_max_bwd_raw(x, tuple(wp[:7]), out["argidx"], g, masks, out=acc, accumulate=True,
                              **{k: v for k, v in bkw.items() if k != "want_gT"})
    out["gx_acc"] = acc
    torch.cuda.synchronize()
    return out


@pytest.fixture
def calls(monkeypatch):
    """Every library call that ops makes: (name, args), in order."""
    seen = []
    call = ops._lib.call

    def recording(name, *args):
        seen.append((name, args))
        return call(name, *args)
    monkeypatch.setattr(ops._lib, "call", recording)
    return seen


def _tower_calls(calls):
    return [n for n, _ in calls if n.startswith("pc3d_pointmlp3_max_")]


FORMS = pytest.mark.parametrize("exact", [True, False], ids=["exact", "pair"])
GRID = [pytest.mark.parametrize("C3", [64, 1024]), pytest.mark.parametrize("relu_last", [False, True], ids=["norelu", "relu"]),
        pytest.mark.parametrize("variant", VARIANTS), FORMS]


def _grid(f):
    for m in GRID:
        f = m(f)
    return f


# ----------------------------------------------------------------------------------------------------------------------
# 1. rows beyond a length are never read
# ----------------------------------------------------------------------------------------------------------------------
@_grid
def test_rows_beyond_a_length_are_never_read(dev, calls, C3, relu_last, variant, exact):
    """x holds NaN at and beyond every length; the dense entries on the batch padded with copies of point 0 (ops.pad_ragged)
    are the reference."""
    c = _case(C3, KMAX, dev)
    lens = _lens(LENGTHS, dev)
    del calls[:]
    got = _run(_nan_beyond(c["x"], LENGTHS), c, relu_last, variant, exact, lengths=lens)
    fwd = [a for n, a in calls if n == FWD]
    assert _tower_calls(calls) == [FWD, BWD, BWD] and fwd[0][FWD_FORM_ARG] == (EXACT if exact else H_PAIR)
    ref = _run(ops.pad_ragged(c["x"].clone(), lens), c, relu_last, variant, False)
    for k in ("pooled", "argidx") + (("T_out",) if variant == "T_head" else ()):
        assert _eq(got[k], ref[k]), k
    assert int(got["argidx"].max()) < KMAX and all(int(got["argidx"][b].max()) < L for b, L in enumerate(LENGTHS))
    for b, L in enumerate(LENGTHS):
        for k in ("mask1", "mask2", ):
            assert _eq(got[k][b, :L], ref[k][b, :L]), (k, b)
            assert not got[k][b, L:].any(), (k, b)
        for k in ("gx", "gx_acc"):
            assert _eq(got[k][b, :, :L], ref[k][b, :, :L]), (k, b)
        assert _eq(got["gx"][b, :, L:], torch.zeros(3, KMAX - L, device=dev)), b
        assert _eq(got["gx_acc"][b, :, L:], torch.full((3, KMAX - L), SENTINEL, device=dev)), b
    assert not torch.isnan(got["gx"]).any() and float(got["gx"].abs().max()) > 0
    if variant != "plain":
        assert _eq(got["part_gT"].sum(1), ref["part_gT"].sum(1))
        assert float(got["part_gT"].abs().max()) > 0
        for b, L in enumerate(LENGTHS):
            assert not got["part_gT"][b, (L + SUB - 1) // SUB:].any(), b       # records at and beyond L are zero


# ----------------------------------------------------------------------------------------------------------------------
# 2. each cloud against its own run
# ----------------------------------------------------------------------------------------------------------------------
@_grid
def test_each_cloud_equals_the_dense_entries_on_that_cloud_alone(dev, C3, relu_last, variant, exact):
    c = _case(C3, KMAX, dev)
    got = _run(_nan_beyond(c["x"], LENGTHS), c, relu_last, variant, exact, lengths=_lens(LENGTHS, dev))
    for b, L in enumerate(LENGTHS):
        one = _run(c["x"][b:b + 1, :, :L].contiguous(), c, relu_last, variant, False, idx=slice(b, b + 1))
        for k in ("pooled", "argidx") + (("T_out",) if variant == "T_head" else ()):
            assert _eq(got[k][b:b + 1], one[k]), (k, b)
        for k in ("mask1", "mask2"):
            assert _eq(got[k][b:b + 1, :L], one[k]), (k, b)
        for k in ("gx", "gx_acc"):
            assert _eq(got[k][b:b + 1, :, :L], one[k]), (k, b)
        if variant != "plain":
            assert _eq(got["part_gT"][b:b + 1].sum(1), one["part_gT"].sum(1)), b


# ----------------------------------------------------------------------------------------------------------------------
# 3. full lengths
# ----------------------------------------------------------------------------------------------------------------------
@FORMS
@pytest.mark.parametrize("C3", [64, 1024])
@pytest.mark.parametrize("n", [127, 128, 129, 300])
def test_full_lengths_equal_the_dense_entries_in_every_output(dev, n, C3, exact):
    c = _case(C3, n, dev)
    for relu_last, variant in [(False, "plain"), (True, "T"), (False, "T_head")]:
        got = _run(c["x"], c, relu_last, variant, exact, lengths=_lens([n] * B, dev), partials=True)
        ref = _run(c["x"], c, relu_last, variant, exact, partials=True)
        assert set(got) == set(ref)
        for k, v in ref.items():
            assert (v is None and got[k] is None) or _eq(got[k], v), (k, variant)


# ----------------------------------------------------------------------------------------------------------------------
# 4. skipped tiles
# ----------------------------------------------------------------------------------------------------------------------
@FORMS
@pytest.mark.parametrize("C3", [64, 1024])
@pytest.mark.parametrize("relu_last", [False, True], ids=["norelu", "relu"])
def test_skipped_tiles_hold_partials_that_no_fold_takes(dev, C3, relu_last, exact):
    c = _case(C3, KMAX, dev)
    got = _run(_nan_beyond(c["x"], LENGTHS), c, relu_last, "T_head", exact, lengths=_lens(LENGTHS, dev), partials=True)
    pv, pi = got["part_val"], got["part_idx"]
    assert pv.shape == (B, 3, C3)
    skipped = 0
    for b, L in enumerate(LENGTHS):
        for t in range(3):
            if t * TILE >= L:
                assert bool((pv[b, t] == float("-inf")).all()) and not pi[b, t].any(), (b, t)
                skipped += 1
            else:
                assert bool(torch.isfinite(pv[b, t]).all()), (b, t)
    assert skipped == 2 * 4 + 2      # lengths <= 128: two tiles; 256, 129: one; 300, 257: none
    for serial in (False, True):
        pooled, argidx = ops.pointmlp3_fold_raw(pv, pi, relu_last, serial=serial)
        assert _eq(pooled, got["pooled"]) and _eq(argidx, got["argidx"]), serial


# ----------------------------------------------------------------------------------------------------------------------
# 5. capture
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C3", [64, 1024])
def test_one_captured_pair_serves_other_lengths(dev, C3):
    """A forward + backward pair captured once, replayed after the lengths buffer (and the NaN rows of x) were overwritten
    with a permutation: the lengths are data of the launches."""
    c = _case(C3, KMAX, dev)
    lens, x = _lens(LENGTHS, dev), _nan_beyond(c["x"], LENGTHS)
    keys = ("pooled", "argidx", "mask1", "mask2", "T_out", "gx", "gx_acc", "part_gT")
    eager = _run(x, c, True, "T_head", False, lengths=lens)                   # (also: the instantiation's first use)
    graph = torch.cuda.CUDAGraph()
    with graphed.capture_guard() as keep:
        with torch.cuda.graph(graph):
            out = _run_captured(x, c, lens)
    graph.replay()
    torch.cuda.synchronize()
    for k in keys:
        assert _eq(out[k], eager[k]), k
    permuted = [LENGTHS[i] for i in PERM]
    assert permuted != LENGTHS
    want = _run(_nan_beyond(c["x"], permuted), c, True, "T_head", False, lengths=_lens(permuted, dev))
    lens.copy_(_lens(permuted, dev))
    x.copy_(_nan_beyond(c["x"], permuted))
    graph.replay()
    torch.cuda.synchronize()
    for k in keys:
        assert _eq(out[k], want[k]), k
    assert not _eq(want["pooled"], eager["pooled"])
    del keep


def _run_captured(x, c, lens):
    """_run(x, c, True, "T_head", False, lengths=lens) without its synchronize."""
    wp, out = c["wp"], {}
    out["pooled"], out["argidx"], (out["mask1"], out["mask2"]), out["T_out"] = ops.pointmlp3_max_fwd_raw(
        x, wp, True, want_masks=True, T_head=c["T_head"], lengths=lens)
    g = c["g"] * (out["pooled"] > 0)
    T, masks = out["T_out"].view(-1, 3, 3), (out["mask1"], out["mask2"])
    out["gx"], out["part_gT"] = ops.pointmlp3_max_bwd_raw(x, tuple(wp[:7]), out["argidx"], g, masks, T=T, want_gT=True, lengths=lens)
    out["gx_acc"] = torch.full_like(x, SENTINEL)
    ops.pointmlp3_max_bwd_raw(x, tuple(wp[:7]), out["argidx"], g, masks, T=T, out=out["gx_acc"], accumulate=True, lengths=lens)
    return out


FRESH = r'''
import importlib, sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import torch
ops = importlib.import_module("3dpointcloudattack_amd.ops")
from test_pointmlp_screen_prepared_gpu import _flat, _packed, _weights
dev = torch.device("cuda:0")
torch.manual_seed(3)
wp = _packed(_weights(dev, 288, 9))
x = torch.randn(4, 3, 300, device=dev) * 0.5
lengths = [300, 257, 128, 3]
lens = torch.tensor(lengths, dtype=torch.int32, device=dev)
for b, L in enumerate(lengths):
    x[b, :, L:] = float("nan")
calls = []
call = ops._lib.call
ops._lib.call = lambda name, *a: (calls.append((name, a[28])) if name.endswith("fwd_ragged_f32") else None, call(name, *a))[1]
run = lambda **kw: _flat(ops.pointmlp3_max_fwd_raw(x, wp, False, want_masks=True, lengths=lens, **kw))
ops.pointmlp3_max_fwd_raw(torch.randn(4, 3, 300, device=dev), wp, False)   # a DENSE launch makes the images; no ragged launch yet
assert len(wp[7]) == 4 and ops.pointmlp3_pair_recheck_ready(dev)
side = torch.cuda.Stream()
side.wait_stream(torch.cuda.current_stream())
graph = torch.cuda.CUDAGraph()
with torch.cuda.stream(side):
    with torch.cuda.graph(graph, stream=side):
        out = run()                                   # the ragged pair instantiation's first use: inside a capture
assert calls == [("pc3d_pointmlp3_max_fwd_ragged_f32", 4)]      # ops asked for the production form; the entry stepped aside
graph.replay()
torch.cuda.synchronize()
exact = run(exact=True)                               # the ragged exact kernel, eager
torch.cuda.synchronize()
assert all(torch.equal(a, b) for a, b in zip(exact, out))
after = run()                                         # outside a capture: now the ragged pair instantiation
torch.cuda.synchronize()
assert [c[1] for c in calls] == [4, 0, 4]
assert all(torch.equal(a, b) for a, b in zip(exact, after))
assert not torch.isnan(out[0]).any()
print("fresh ragged capture ok")
'''


def test_first_use_inside_a_capture_takes_the_ragged_exact_kernel():
    out = subprocess.run([sys.executable, "-c", FRESH % (ROOT, os.path.join(ROOT, "tests"))], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0 and "fresh ragged capture ok" in out.stdout, out.stdout[-1000:] + out.stderr[-3000:]


# ----------------------------------------------------------------------------------------------------------------------
# 6. the victim
# ----------------------------------------------------------------------------------------------------------------------
VB, VLENGTHS = 4, [300, 257, 128, 3]
_MODELS = {}


def _victim(dev):
    if "m" not in _MODELS:
        _MODELS["m"], _MODELS["t"] = hip_pointnet(0, dev)[0], hip_pointnet(1, dev)[0]
    return _MODELS["m"]


@functools.lru_cache(maxsize=None)
def _clouds():
    rng = np.random.default_rng(78)
    return [unit_cloud(rng, n) for n in VLENGTHS]


@pytest.mark.parametrize("nan_padding", [False, True], ids=["padded", "nan"])
@pytest.mark.parametrize("kind", ["untargeted_logits", "cross_entropy"])
def test_victim_with_lengths_equals_the_padded_pass(dev, calls, kind, nan_padding):
    victim = _victim(dev)
    assert victim.fused_lengths
    data, lengths = cloud_io.stack_ragged(_clouds())
    xpad = torch.from_numpy(data).transpose(1, 2).contiguous().to(dev)
    x = _nan_beyond(xpad, VLENGTHS) if nan_padding else xpad
    lens = _lens(VLENGTHS, dev)
    target = _labels(dev).to(dev)                   # the clean predictions: the untargeted hinge is active
    with torch.no_grad():
        ref = [t.clone() for t in victim.fused_loss_and_grad(xpad, target, kind, 0.5, scale=1.0 / VB)]
        ref_a = [t.clone() for t in victim.fused_attack_grad(xpad, target, kind, 0.5, scale=1.0 / VB)]
        del calls[:]
        got = victim.fused_loss_and_grad(x, target, kind, 0.5, scale=1.0 / VB, lengths=lens)
        assert _tower_calls(calls) == [FWD, FWD, BWD, BWD]
        got_a = victim.fused_attack_grad(x, target, kind, 0.5, scale=1.0 / VB, lengths=lens)
    torch.cuda.synchronize()
    assert _tower_calls(calls) == [FWD, FWD, BWD, BWD] * 2
    for i, name in enumerate(("logp", "pred", "loss")):
        assert _eq(got[i], ref[i]), name
    assert _eq(got_a[0], ref_a[0]) and _eq(got_a[1], ref_a[1])
    for g, r in ((got[3], ref[3]), (got_a[2], ref_a[2])):
        for b, L in enumerate(VLENGTHS):
            assert _eq(g[b, :, :L], r[b, :, :L]), b
            assert _eq(g[b, :, L:], torch.zeros(3, KMAX - L, device=dev)), b
        assert float(g.abs().max()) > 0


def test_feature_transform_victim_refuses_lengths(dev):
    ft = pointnet.PointNetCls(k=40, feature_transform=True)
    ft.load_state_dict(ort.seeded_state_dict(ft, 0))
    ft = ft.eval().to(dev)
    assert ft.fused_lengths is False and ft.pad_invariant
    x, lens, target = torch.randn(VB, 3, 64, device=dev), _lens([64, 3, 1, 17], dev), torch.zeros(VB, dtype=torch.long, device=dev)
    for f in (lambda: ft.fused_loss_and_grad(x, target, "cross_entropy", lengths=lens),
              lambda: ft.fused_attack_grad(x, target, "cross_entropy", lengths=lens),
              lambda: pointnet.fused_forward(ft, x, lengths=lens)):
        with pytest.raises(ValueError, match="fused_lengths"):
            f()
    with torch.no_grad():
        ft.fused_loss_and_grad(x, target, "cross_entropy")                  # without lengths: its padded pass, as before


# ----------------------------------------------------------------------------------------------------------------------
# 7. the loops
# ----------------------------------------------------------------------------------------------------------------------
SEEDS = [3000 + i for i in range(VB)]
ORDER = [2, 0, 3, 1]
COUNTERS = ("attack_fail", "shuffle_fail", "trans_fail")
DENSE_FWD = "pc3d_pointmlp3_max_fwd_f32"


def _labels(dev):
    data, _ = cloud_io.stack_ragged(_clouds())
    with torch.no_grad():
        return _victim(dev)(torch.from_numpy(data).transpose(1, 2).contiguous().to(dev))[0].argmax(1).cpu()


def _cw(dev, **kw):
    _victim(dev)
    return cwm.CW(_MODELS["m"], _MODELS["t"], adv_func=adv_u.UntargetedLogitsAdvLoss(5.), clip_func=clip_u.ClipPointsLinf(0.18),
                  dist_func=dist_u.ChamferDist(), binary_step=2, num_iter=6, **kw)


def _knn(dev, **kw):
    _victim(dev)
    return knnm.CWKNN(_MODELS["m"], _MODELS["t"], None, None, None, None, adv_func=adv_u.UntargetedLogitsAdvLoss(5.),
                      dist_func=dist_u.ChamferDist(), clip_func=clip_u.ProjectInnerClipLinf(0.18), attack_lr=1e-2, num_iter=19,
                      device_loop=True, **kw)


def _iteration_calls(calls):
    """The tower launches that fall between two update launches: the iterations' (warm-up and capture passes included)."""
    upd = [i for i, (n, _) in enumerate(calls) if n in ("pc3d_cw_update_ragged_f32", "pc3d_knn_attack_update_ragged_f32")]
    assert len(upd) >= 2
    return [n for n, _ in calls[upd[0]:upd[-1]] if n.startswith("pc3d_pointmlp3_max_")]


def test_ragged_cw_hands_the_lengths_to_the_victim(dev, calls):
    labels, clouds = _labels(dev), _clouds()
    np.random.seed(3)
    alone = []
    for b, c in enumerate(clouds):
        atk = _cw(dev, sample_seeds=[SEEDS[b]], global_batch=VB, graph=False)
        alone.append(atk.attack(torch.from_numpy(c)[None], labels[b:b + 1]) + ({k: getattr(atk, k) for k in COUNTERS},))
    assert FWD not in _tower_calls(calls)                        # a run alone is a dense run
    atk = _cw(dev, sample_seeds=SEEDS, graph=True)
    for order in (list(range(VB)), ORDER):                       # the second call: permuted lengths, the same attack object
        data, lengths = cloud_io.stack_ragged([clouds[s] for s in order])
        atk.sample_seeds = [SEEDS[s] for s in order]
        for k in COUNTERS:
            setattr(atk, k, 0)
        del calls[:]
        np.random.seed(3)
        bd, ba, sn = atk.attack(torch.from_numpy(data), labels[order], lengths)
        its = _iteration_calls(calls)
        assert set(its) == {FWD, BWD} and its.count(FWD) == its.count(BWD) >= 2, its[:12]
        print(f"ragged CW order {order}: success {sn}/{VB} bestdist {bd}")
        if order == list(range(VB)):     # (numpy's global stream, consumed in batch order, matches the runs alone in order)
            assert {k: getattr(atk, k) for k in COUNTERS} == {k: sum(a[3][k] for a in alone) for k in COUNTERS}
        for b, s in enumerate(order):
            L = VLENGTHS[s]
            assert bd[b] == alone[s][0][0], (b, s)
            assert np.array_equal(ba[b, :L], alone[s][1][0]), (b, s)
            assert np.array_equal(ba[b, L:], np.broadcast_to(ba[b, 0], (KMAX - L, 3))), b
        assert sn == sum(a[2] for a in alone)


def test_ragged_knn_loop_hands_the_lengths_to_the_victim(dev, calls):
    labels, clouds = _labels(dev), _clouds()
    alone = []
    for b, c in enumerate(clouds):
        atk = _knn(dev, sample_seeds=[SEEDS[b]], global_batch=VB, graph=False)
        adv, sn = atk.attack(torch.from_numpy(c)[None], labels[b:b + 1])
        assert atk.last_path == "device_loop"
        alone.append((adv[0], sn, atk.attack_fail, atk.pt_fail))
    assert FWD not in _tower_calls(calls)
    atk = _knn(dev, sample_seeds=SEEDS, global_batch=VB, graph=True)
    loop = graphs = None
    for order in (list(range(VB)), ORDER):
        data, lengths = cloud_io.stack_ragged([clouds[s] for s in order])
        atk.sample_seeds = [SEEDS[s] for s in order]
        atk.attack_fail = atk.pt_fail = 0
        del calls[:]
        adv, sn = atk.attack(torch.from_numpy(data), labels[order], lengths)
        assert atk.last_path == "device_loop" and len(atk._loop_cache) == 1
        if loop is None:
            loop = next(iter(atk._loop_cache.values()))
            graphs = loop.graphs
            its = _iteration_calls(calls)                        # the loop's warm-up and capture passes
            assert graphs is not None and set(its) == {FWD, BWD} and its.count(FWD) == its.count(BWD) >= 2, its[:12]
        else:                                                    # the same loop, the same graphs: nothing is launched by hand
            assert next(iter(atk._loop_cache.values())) is loop and loop.graphs is graphs
            assert not [n for n, _ in calls if n == "pc3d_knn_attack_update_ragged_f32"]
        print(f"ragged kNN order {order}: success {sn}/{VB}")
        for b, s in enumerate(order):
            L = VLENGTHS[s]
            assert np.array_equal(adv[b, :L], alone[s][0]), (b, s, float(np.abs(adv[b, :L] - alone[s][0]).max()))
            assert np.array_equal(adv[b, L:], np.broadcast_to(adv[b, 0], (KMAX - L, 3))), b
        assert sn == sum(a[1] for a in alone)
        assert atk.attack_fail == sum(a[2] for a in alone) and atk.pt_fail == sum(a[3] for a in alone)
