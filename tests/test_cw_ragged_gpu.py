"""GPU: clouds of different sizes in one batch — ops.pad_ragged, PointNet's padding invariance (logits, gradient),
ops.cw_update(lengths=...) against the float64 restatement and against the dense launch, and CW.attack(data, target, lengths)
against the same clouds attacked alone.

The lengths sit on both sides of the tower's point tile (a multiple of it: 1024; 1025, 513, 65, 3 are not) and of the update
kernel's 1024-thread stride (1024 | 1025, 1030: one and two points per thread)."""
import functools
import importlib

import numpy as np
import pytest
import torch

import cw_ragged_restatement as rr
import cw_step_restatement as rs
from helpers import hip_pointnet, unit_cloud
from oracle import ref_torch as ort

pytestmark = pytest.mark.gpu
M = importlib.import_module
ops = M("3dpointcloudattack_amd.ops")
pointnet = M("3dpointcloudattack_amd.model.pointnet")
dfn = M("3dpointcloudattack_amd.defense")
graphed = M("3dpointcloudattack_amd.graphed")
cloud_io = M("3dpointcloudattack_amd.dataset.cloud_io")
cwm = M("3dpointcloudattack_amd.attack.CW.CW_attack")
adv_u = M("3dpointcloudattack_amd.attack.CW.CW_utils.adv_utils")
dist_u = M("3dpointcloudattack_amd.attack.CW.CW_utils.dist_utils")
clip_u = M("3dpointcloudattack_amd.attack.CW.CW_utils.clip_utils")

LENGTHS = [1030, 1025, 1024, 513, 65, 3]
KMAX = 1030
NAN_WORD = 0x7FC00ABC            # a quiet NaN with a payload: survives only if nobody writes the word


def _nan_fill(shape, dev):
    return torch.full(shape, NAN_WORD, dtype=torch.int32, device=dev).view(torch.float32)


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t.contiguous()


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _lens(lengths, dev):
    return torch.tensor(lengths, dtype=torch.int32, device=dev)


def _victim(ft, dev, seed=0):
    if not ft:
        return hip_pointnet(seed, dev)[0]
    m = pointnet.PointNetCls(k=40, feature_transform=True)
    m.load_state_dict(ort.seeded_state_dict(m, seed))
    return m.eval().to(dev)


@functools.lru_cache(maxsize=None)
def _clouds():
    """(data [B,Kmax,3] float32 numpy, lengths int32 numpy, the list of clouds): shared, never modified."""
    rng = np.random.default_rng(77)
    clouds = [unit_cloud(rng, n) for n in LENGTHS]
    data, lengths = cloud_io.stack_ragged(clouds)
    return data, lengths, clouds


# ----------------------------------------------------------------------------------------------------------------------
# 1. the padding kernel
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cf", [True, False])
def test_pad_ragged_equals_indexing(dev, cf):
    lengths = [KMAX, 1, 513, 256, 257, 3]            # untouched cloud, a single point, both sides of the launch's 256 block
    B = len(lengths)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(B, 3, KMAX, generator=g).to(dev)
    for b, L in enumerate(lengths):
        x[b, :, L:] = _nan_fill((3, KMAX - L), dev)     # the ignored rows: NaN
    want = x.clone()
    for b, L in enumerate(lengths):
        want[b, :, L:] = want[b, :, :1]
    if not cf:
        x, want = (torch.empty(B, KMAX, 3, device=dev).copy_(t.transpose(1, 2)) for t in (x, want))
    start = x.clone()
    lens = _lens(lengths, dev)
    got = ops.pad_ragged(x, lens, cf=cf)
    assert got is x and _same_bits(x, want)
    assert not torch.isnan(x).any()
    assert _same_bits(x[0], start[0]), "a cloud with L = Kmax is untouched"
    # eager equals a replay from a captured graph (the lengths are read as data: other lengths, the same graph)
    y = start.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.pad_ragged(y, lens, cf=cf)
    torch.cuda.current_stream().wait_stream(side)
    y.copy_(start)
    graph = torch.cuda.CUDAGraph()
    with graphed.capture_guard():
        with torch.cuda.graph(graph):
            ops.pad_ragged(y, lens, cf=cf)
    y.copy_(start)
    graph.replay()
    torch.cuda.synchronize()
    assert _same_bits(y, want)
    lens.copy_(_lens([KMAX] * B, dev))
    y.copy_(start)
    graph.replay()
    torch.cuda.synchronize()
    assert _same_bits(y, start)


def test_pad_ragged_refuses_other_lengths(dev):
    x = torch.zeros(2, 3, 8, device=dev)
    for bad in (torch.tensor([1, 2], device=dev), torch.tensor([1, 2, 3], dtype=torch.int32, device=dev),
                torch.tensor([1, 2], dtype=torch.int32), [1, 2]):
        with pytest.raises(ValueError, match="lengths must be a contiguous int32"):
            ops.pad_ragged(x, bad)


# ----------------------------------------------------------------------------------------------------------------------
# 2. / 3. the victim does not see the padding
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[False, True], ids=["plain", "feature_transform"])
def victim(request, dev):
    return _victim(request.param, dev)


def test_logits_of_the_padded_batch_equal_every_cloud_alone(dev, victim):
    data, lengths, clouds = _clouds()
    x = torch.from_numpy(data).transpose(1, 2).contiguous().to(dev)
    with torch.no_grad():
        logits = pointnet.fused_forward(victim, x)[0].clone()
        for b, c in enumerate(clouds):
            alone = pointnet.fused_forward(victim, torch.from_numpy(c).t().contiguous()[None].to(dev))[0]
            assert torch.equal(logits[b:b + 1], alone), b


@pytest.mark.parametrize("kind", ["untargeted_logits", "cross_entropy"])
def test_gradient_of_the_padded_batch_equals_every_cloud_alone(dev, victim, kind):
    """Rows at and beyond the length: exactly zero. Rows below: the values of the cloud alone (== : a signed zero passes)."""
    data, lengths, clouds = _clouds()
    B = len(clouds)
    x = torch.from_numpy(data).transpose(1, 2).contiguous().to(dev)
    target = torch.tensor([3, 17, 39, 0, 21, 8], device=dev)
    with torch.no_grad():
        pred, loss, g = victim.fused_attack_grad(x, target, kind, 0.5, scale=1.0 / B)
        pred, loss, g = pred.clone(), loss.clone(), g.clone()
        for b, c in enumerate(clouds):
            L = len(c)
            p1, l1, g1 = victim.fused_attack_grad(torch.from_numpy(c).t().contiguous()[None].to(dev), target[b:b + 1], kind,
                                                  0.5, scale=1.0 / B)
            assert torch.equal(pred[b:b + 1], p1) and torch.equal(loss[b:b + 1], l1), b
            assert bool((g[b, :, L:] == 0).all()), b
            assert bool((g[b, :, :L] == g1[0]).all()), (b, float((g[b, :, :L] - g1[0]).abs().max()))


# ----------------------------------------------------------------------------------------------------------------------
# 4. the update kernel
# ----------------------------------------------------------------------------------------------------------------------
POINTS = ("adv", "ori", "g", "m", "v", "o_bestattack", "input_val")
WRITTEN = ("adv", "m", "v", "dist_val", "bestdist", "bestscore", "o_bestdist", "o_bestscore", "o_bestattack", "input_val")


def _device_state(s, lengths, dev, cf, nan_padding=True):
    """The case of rr.inputs on the device; outputs prefilled with the payload NaN, and so are the rows at and beyond every
    length of adv, g, m and v (never read). ori keeps its padding."""
    d = {k: torch.from_numpy(s[k]).to(dev) for k in ("adv", "ori", "g", "m", "v", "pred", "label", "bestdist", "o_bestdist",
                                                      "bestscore", "o_bestscore", "w")}
    if nan_padding:
        for b, L in enumerate(lengths):
            for k in ("adv", "g", "m", "v"):
                d[k][b, :, L:] = _nan_fill((3, d[k].shape[2] - L), dev)
    d["o_bestattack"], d["input_val"] = _nan_fill(d["adv"].shape, dev), _nan_fill(d["adv"].shape, dev)
    d["dist_val"] = _nan_fill((len(lengths),), dev)
    if not cf:
        for k in POINTS:
            d[k] = torch.empty(d[k].shape[0], d[k].shape[2], 3, device=dev).copy_(d[k].transpose(1, 2))
    return d


def _update(d, untarget, dist_kind, nn_idx, cf, lens):
    word = torch.full((1,), rs.T, dtype=torch.int32, device=d["adv"].device)
    ops.cw_update(d["adv"], d["ori"], d["pred"], d["label"], untarget, d["bestdist"], d["bestscore"], d["o_bestdist"],
                  d["o_bestscore"], d["o_bestattack"], d["g"], d["m"], d["v"], word, rs.LR, rs.BUDGET, input_val=d["input_val"],
                  dist_val=d["dist_val"], dist_kind=dist_kind, w=d["w"], nn_idx=nn_idx, betas=rs.BETAS, eps=rs.EPS, cf=cf,
                  lengths=lens)
    return d


def _cf(t, cf):
    return t if cf or t.dim() != 3 else t.transpose(1, 2)


@functools.lru_cache(maxsize=None)
def _ragged_reference(dist_kind, untarget, nn_kind):
    s = rr.inputs(LENGTHS, KMAX)
    nn = None
    if dist_kind == 2:
        nn = s["rand_idx"] if nn_kind == "random" else rs.nn_f64(torch.from_numpy(s["adv"]), torch.from_numpy(s["ori"])).numpy()
    r64 = rr.step(np.float64, s, LENGTHS, rs.T, untarget, dist_kind, nn_idx=nn)
    r32 = rr.step(np.float32, s, LENGTHS, rs.T, untarget, dist_kind, nn_idx=nn)
    for k in rs.INT_OUT + ("copied",):
        assert np.array_equal(r64[k], r32[k]), "a decision of the case sits at rounding distance"
    t64, t32 = ({k: torch.from_numpy(np.asarray(v)) for k, v in r.items()} for r in (r64, r32))
    return s, nn, t64, rs.bands(t64, t32)


@pytest.mark.parametrize("cf", [True, False])
@pytest.mark.parametrize("untarget", [True, False])
@pytest.mark.parametrize("dist_kind,nn_kind", [(1, None), (2, "argmin"), (2, "random")])
def test_ragged_update_against_float64(dev, dist_kind, nn_kind, untarget, cf):
    """The tolerance rule of tests/test_cw_step_gpu.py (rs.bands: 16 x the fp32 restatement's own deviation from float64,
    floor 16 x 2^-24 max|ref|) on the counted rows; integer state, copies, padding and sentinels bit for bit. nn "random": the
    index names padding rows of ori too."""
    s, nn, r64, band = _ragged_reference(dist_kind, untarget, nn_kind)
    d = _device_state(s, LENGTHS, dev, cf)
    before = _cf(d["adv"], cf).clone()
    _update(d, untarget, dist_kind, None if nn is None else torch.from_numpy(nn).to(dev), cf, _lens(LENGTHS, dev))
    out = {k: _cf(d[k], cf) for k in WRITTEN}
    ratios = {}
    for k in rs.FLOAT_OUT:
        err = 0.
        for b, L in enumerate(LENGTHS):
            a, r = (out[k][b, :, :L], r64[k][b, :, :L]) if out[k].dim() == 3 else (out[k][b], r64[k][b])
            err = max(err, float((a.double().cpu() - r).abs().max()))
        ratios[k] = err / band[k]
    print(f"cw_ragged_band kind={dist_kind} nn={nn_kind} untarget={int(untarget)} cf={int(cf)}: "
          + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    for k, v in ratios.items():
        assert v <= 1., (k, v)
    for k in rs.INT_OUT:
        assert torch.equal(out[k].cpu(), r64[k]), k
    for b, L in enumerate(LENGTHS):
        pad = KMAX - L
        assert _same_bits(out["adv"][b, :, L:], out["adv"][b, :, :1].expand(3, pad)), b          # the NEW point 0
        assert _same_bits(out["input_val"][b, :, :L], before[b, :, :L]), b
        assert _same_bits(out["input_val"][b, :, L:], before[b, :, :1].expand(3, pad)), b        # the old one
        for k in ("m", "v"):
            assert bool((_bits(out[k][b, :, L:]) == NAN_WORD).all()), (k, b)                      # not written
        if bool(r64["copied"][b]):
            assert _same_bits(out["o_bestattack"][b], out["input_val"][b]), b
        else:
            assert bool((_bits(out["o_bestattack"][b]) == NAN_WORD).all()), b
    assert not torch.isnan(out["adv"]).any()


@pytest.mark.parametrize("untarget", [True, False])
@pytest.mark.parametrize("dist_kind", [1, 2])
@pytest.mark.parametrize("K", [1023, 1024, 1025, 2049])
def test_full_lengths_equal_the_dense_launch(dev, K, dist_kind, untarget):
    B = 3
    s = rr.inputs([K] * B, K)
    nn = torch.from_numpy(s["rand_idx"]).to(dev) if dist_kind == 2 else None
    dense = _update(_device_state(s, [K] * B, dev, True), untarget, dist_kind, nn, True, None)
    ragged = _update(_device_state(s, [K] * B, dev, True), untarget, dist_kind, nn, True, _lens([K] * B, dev))
    for k in WRITTEN:
        assert _same_bits(ragged[k], dense[k]), k


@pytest.mark.parametrize("dist_kind", [1, 2])
def test_ragged_update_equals_the_dense_launch_on_every_cloud_alone(dev, dist_kind):
    """The kernel's own promise: a cloud in the padded batch gets the bits of the dense launch at K = L on that cloud. The
    dense launch divides w by its own B, so it is given B copies of the cloud: the same w, the same B."""
    s = rr.inputs(LENGTHS, KMAX)
    B = len(LENGTHS)
    nn = None
    if dist_kind == 2:       # every index below the cloud's own length, so that the cloud alone can take it as it is
        nn = torch.from_numpy(np.minimum(s["rand_idx"], np.array(LENGTHS, dtype=np.int32)[:, None] - 1).astype(np.int32)).to(dev)
    d = _update(_device_state(s, LENGTHS, dev, True), True, dist_kind, nn, True, _lens(LENGTHS, dev))
    for b, L in enumerate(LENGTHS):
        one = {k: np.repeat(v[b:b + 1, :, :L] if v.ndim == 3 else v[b:b + 1], B, axis=0) for k, v in s.items() if k != "rand_idx"}
        nn1 = nn[b:b + 1, :L].repeat(B, 1).contiguous() if nn is not None else None
        a = _update(_device_state(one, [L] * B, dev, True), True, dist_kind, nn1, True, None)
        for k in WRITTEN:
            got = d[k][b, :, :L] if d[k].dim() == 3 else d[k][b]
            if k == "o_bestattack" and bool((_bits(d[k][b]) == NAN_WORD).all()):
                assert bool((_bits(a[k][0]) == NAN_WORD).all())
                continue
            assert _same_bits(got, a[k][0]), (k, b)


# ----------------------------------------------------------------------------------------------------------------------
# 5. the whole attack
# ----------------------------------------------------------------------------------------------------------------------
SEEDS = [1000 + i for i in range(len(LENGTHS))]
COUNTERS = ("attack_fail", "shuffle_fail", "trans_fail")


class _NoPadInvariance(torch.nn.Module):
    """A transfer model that does not declare pad_invariant: the attack must hand it every cloud alone."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner
        self.sizes = []

    def forward(self, x):
        self.sizes.append(tuple(x.shape))
        return self.inner(x)


def _dist(name):
    return dist_u.L2Dist() if name == "l2" else dist_u.ChamferDist()


def _attacker(model, trans, dist, **kw):
    return cwm.CW(model, trans, adv_func=adv_u.UntargetedLogitsAdvLoss(5.), clip_func=clip_u.ClipPointsLinf(0.18),
                  dist_func=_dist(dist), binary_step=2, num_iter=12, **kw)


_MODELS = {}


def _models(dev):
    if not _MODELS:
        _MODELS["m"], _MODELS["t"] = hip_pointnet(0, dev)[0], hip_pointnet(1, dev)[0]
    return _MODELS["m"], _MODELS["t"]


def _labels(dev):
    data, _, _ = _clouds()
    with torch.no_grad():
        return _models(dev)[0](torch.from_numpy(data).transpose(1, 2).contiguous().to(dev))[0].argmax(1).cpu()


@functools.lru_cache(maxsize=None)
def _alone(dist, dev):
    """The B attacks alone: B = 1, K = lengths[b], sample_seeds = [seed_b], global_batch = B; numpy's global stream seeded once
    and consumed in batch order. Returns (bestdist [B], list of best attacks, success_num, counters)."""
    model, trans = _models(dev)
    _, _, clouds = _clouds()
    labels = _labels(dev)
    np.random.seed(3)
    bd, ba, sn, cnt = [], [], 0, dict.fromkeys(COUNTERS, 0)
    for b, c in enumerate(clouds):
        atk = _attacker(model, trans, dist, sample_seeds=[SEEDS[b]], global_batch=len(clouds), graph=False)
        d, a, n = atk.attack(torch.from_numpy(c)[None], labels[b:b + 1])
        bd.append(d[0]), ba.append(a[0])
        sn += n
        for k in COUNTERS:
            cnt[k] += getattr(atk, k)
    return np.array(bd), ba, sn, cnt


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("dist", ["l2", "chamfer"])
def test_ragged_attack_equals_the_attacks_alone(dev, dist, graph):
    model, trans = _models(dev)
    data, lengths, clouds = _clouds()
    bd1, ba1, sn1, cnt1 = _alone(dist, dev)
    # Chamfer run: the transfer model without pad_invariant, evaluated cloud by cloud
    tm = _NoPadInvariance(trans) if dist == "chamfer" else trans
    atk = _attacker(model, tm, dist, sample_seeds=SEEDS, graph=graph)
    np.random.seed(3)
    bd, ba, sn = atk.attack(torch.from_numpy(data), _labels(dev), lengths)
    print(f"ragged attack {dist} graph={graph}: success {sn}/{len(clouds)} bestdist {bd} counters "
          f"{[getattr(atk, k) for k in COUNTERS]}")
    assert bd.dtype == np.float64 and ba.dtype == np.float64 and ba.shape == (len(clouds), KMAX, 3)
    assert np.array_equal(bd, bd1)
    for b, L in enumerate(LENGTHS):
        assert np.array_equal(ba[b, :L], ba1[b]), b
        assert np.array_equal(ba[b, L:], np.broadcast_to(ba[b, 0], (KMAX - L, 3))), b
    assert sn == sn1
    assert {k: getattr(atk, k) for k in COUNTERS} == cnt1
    if dist == "chamfer":
        assert tm.sizes == [(1, 3, L) for L in LENGTHS]


# ----------------------------------------------------------------------------------------------------------------------
# 6. errors and the default
# ----------------------------------------------------------------------------------------------------------------------
class _NoPadPointNet(pointnet.PointNetCls):
    pad_invariant = False


def test_lengths_raise_where_there_is_no_ragged_pass(dev):
    model, trans = _models(dev)
    data, lengths, _ = _clouds()
    x, y = torch.from_numpy(data), _labels(dev)
    nopad = _NoPadPointNet(k=40)
    nopad.load_state_dict(model.state_dict())
    cases = [
        (_attacker(dfn.FusedDefended(model, dfn.SORDefense(2, 1.1, 1024)), trans, "l2"), "pad_invariant"),
        (_attacker(nopad.eval().to(dev), trans, "l2"), "pad_invariant"),
        (_attacker(model, trans, "l2", fused=False), "fused=False"),
        (cwm.CW(model, trans, adv_func=adv_u.UntargetedLogitsAdvLoss(5.), clip_func=clip_u.ClipPointsLinf(0.18),
                dist_func=dist_u.HausdorffDist(), binary_step=2, num_iter=12), "dist_func HausdorffDist"),
        (cwm.CW(model, trans, adv_func=adv_u.UntargetedLogitsAdvLoss(5.), clip_func=clip_u.ClipPointsL2(0.18),
                dist_func=dist_u.L2Dist(), binary_step=2, num_iter=12), "clip_func ClipPointsL2"),
        (cwm.CW(model, trans, adv_func=lambda lg, t: lg.sum(1), clip_func=clip_u.ClipPointsLinf(0.18),
                dist_func=dist_u.L2Dist(), binary_step=2, num_iter=12), "adv_func"),
    ]
    for atk, word in cases:
        with pytest.raises(ValueError, match=word):
            atk.attack(x, y, lengths)
    atk = _attacker(model, trans, "l2")
    for bad in ([1] * 5, [0] + [1] * 5, [KMAX + 1] + [1] * 5, [1.5] * 6):
        with pytest.raises(ValueError, match="lengths must"):
            atk.attack(x, y, bad)
    with pytest.raises(ValueError, match="CW_UPDATE_MAX_POINTS"):
        atk.attack(torch.zeros(1, ops.CW_UPDATE_MAX_POINTS + 1, 3), y[:1], [5])


def test_no_lengths_is_the_dense_attack(dev):
    model, trans = _models(dev)
    rng = np.random.default_rng(52)
    pcs = torch.from_numpy(np.stack([unit_cloud(rng, 300) for _ in range(3)]))
    with torch.no_grad():
        labels = model(pcs.transpose(1, 2).contiguous().to(dev))[0].argmax(1).cpu()
    outs = []
    for kw in ({}, {"lengths": None}):
        atk = _attacker(model, trans, "chamfer", sample_seeds=[5, 6, 7])
        np.random.seed(3)
        outs.append(atk.attack(pcs, labels, **kw) + tuple(getattr(atk, k) for k in COUNTERS))
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_perturb_attack_cw_inherits_the_ragged_pass(dev):
    """Gen3DAdv's Perturb_attack.CW: the same search, five transfer checks; a transfer model without pad_invariant sees every
    cloud alone."""
    pert = M("3dpointcloudattack_amd.attack.Gen3DAdv.Perturb_attack")
    model, trans = _models(dev)
    data, lengths, clouds = _clouds()
    kw = dict(adv_func=adv_u.UntargetedLogitsAdvLoss(5.), clip_func=clip_u.ClipPointsLinf(0.18), dist_func=dist_u.ChamferDist(),
              binary_step=2, num_iter=12, sample_seeds=SEEDS)
    seen = _NoPadInvariance(trans)
    atk = pert.CW(model, trans, seen, None, None, None, **kw)
    np.random.seed(3)
    bd, ba, sn = atk.attack(torch.from_numpy(data), _labels(dev), lengths)
    bd1, ba1, sn1, _ = _alone("chamfer", dev)
    assert np.array_equal(bd, bd1) and sn == sn1
    for b, L in enumerate(LENGTHS):
        assert np.array_equal(ba[b, :L], ba1[b]) and np.array_equal(ba[b, L:], np.broadcast_to(ba[b, 0], (KMAX - L, 3))), b
    assert seen.sizes == [(1, 3, L) for L in LENGTHS]
