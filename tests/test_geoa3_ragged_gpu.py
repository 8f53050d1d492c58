"""GPU: clouds of different sizes in GeoA3's device loop — the ragged update
(pc3d_geoa3_update_ragged_f32) against the dense launch, bit for bit, and against the float64 restatement
(tests/geoa3_step_restatement.py) within the bands tests/test_geoa3_step_gpu.py uses; the ragged normals and kappa_ori
against the dense calls on every cloud alone; and geoA3_attack with cfg.lengths against the same clouds attacked alone.

Launch-level cases run at the cap (Kmax = 2048, k = 16: 140.5 KiB of LDS) with the lengths of tests/geoa3_ragged_cases.py,
and once at k = 2 with a cloud of L = 4; whole attacks at Kmax = 1025 with 2 binary steps x 19 iterations (one block of 16
and three single replays). Behind every length the float buffers hold a payload NaN and the index buffers 0x7fffffff.
tests/test_geoa3_ragged_cpu.py shows that no decision of the float64 comparison's inputs sits at rounding distance."""
import functools
import importlib
import itertools

import numpy as np
import pytest
import torch

import geoa3_ragged_cases as gc
import geoa3_step_restatement as rs
from helpers import hip_pointnet, unit_cloud
from oracle import ref_torch as ort
from test_oracle_golden import _geo_cfg

pytestmark = pytest.mark.gpu
M = importlib.import_module
ops = M("3dpointcloudattack_amd.ops")
ga = M("3dpointcloudattack_amd.attack.GeoA3.GeoA3_attack")
utility = M("3dpointcloudattack_amd.attack.GeoA3.utility")
loss_utils = M("3dpointcloudattack_amd.attack.GeoA3.loss_utils")
pointnet = M("3dpointcloudattack_amd.model.pointnet")
dfn = M("3dpointcloudattack_amd.defense")
cloud_io = M("3dpointcloudattack_amd.dataset.cloud_io")

NAN_WORD = 0x7FC00ABC            # the payload NaN of tests/test_cw_ragged_gpu.py: survives only if nobody writes the word
BAD_INDEX = 0x7FFFFFFF
KINDS = {("CE", True): 2, ("CE", False): 3, ("Margin", True): 1, ("Margin", False): 0}
POINTS = ("x", "ori", "offset", "g", "m", "v", "normal", "best_attack")
WORDS = ("target", "scale", "constrain", "best_loss", "iter_best_loss", "best_step", "best_bs", "iter_best_score", "logits")
POINT_OUT = ("x", "offset", "m", "v", "g", "best_attack")
WORD_OUT = ("best_loss", "iter_best_loss", "constrain_word", "best_step", "best_bs", "iter_best_score", "step", "lr", "hd_arg", "pred")


def _nan_fill(shape, dev, dtype=torch.float32):
    t = torch.full(shape, NAN_WORD, dtype=torch.int32, device=dev)
    return t.view(torch.float32) if dtype == torch.float32 else t


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t.contiguous()


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _untouched(t):
    return bool((_bits(t) == NAN_WORD).all())


def _lens(lengths, dev):
    return torch.tensor([int(n) for n in lengths], dtype=torch.int32, device=dev)


# ----------------------------------------------------------------------------------------------------------------------
# the update launch
# ----------------------------------------------------------------------------------------------------------------------
def _search(dev, x, ori, k):
    """The product's own searches on dense [B,3,N] device clouds: dict(nn_ao, nn_oa [B,N], knn_idx [B,N,k+1])."""
    B, _, N = x.shape
    out = {}
    for nm, q, r in (("nn_ao", x, ori), ("nn_oa", ori, x)):
        d, i = torch.zeros((B, N), device=dev), torch.zeros((B, N), dtype=torch.int32, device=dev)
        ops.nn_search_into(q, r, d, i)
        out[nm] = i
    d, i = torch.zeros((B, N, k + 1), device=dev), torch.zeros((B, N, k + 1), dtype=torch.int32, device=dev)
    ops.knn_search_into(x, d, i)
    out["knn_idx"] = i
    return out


def _to_dev(inp, dev):
    return {k: (v.to(dev).contiguous() if torch.is_tensor(v) else v) for k, v in inp.items()}


def _launch(case, found, lens=None, **over):
    """One launch on copies of the device tensors of `case` (rs.inputs' names, any batch); returns what it writes, on the
    device. g_out starts as the payload NaN."""
    c = dict(rs.DEFAULTS)
    c.update(over)
    a = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in case.items()}
    dev = a["x"].device
    B = a["x"].shape[0]
    pred = torch.zeros((B,), dtype=torch.int64, device=dev)
    _, _, cls, _ = ops.cls_loss(a["logits"], a["target"], KINDS[(c["cls_loss_type"], c["targeted"])], c["confidence"],
                                scale=a["gval"], pred_out=pred)
    step = torch.full((B,), c["t"], dtype=torch.int32, device=dev)
    search = torch.tensor([c["search_step"]], dtype=torch.int32, device=dev)
    lr = torch.full((B,), a["lr"], dtype=torch.float64, device=dev)
    rows = torch.zeros((c["t"] + 2, B), device=dev)
    terms, hd_arg = torch.zeros((5, B), device=dev), torch.zeros((B,), dtype=torch.int32, device=dev)
    g_out = _nan_fill(tuple(a["x"].shape), dev)
    cd, curv = c["dis_loss_type"] == "CD", c["w_curv"] != 0
    ops.geoa3_update(a["x"], a["ori"], a["offset"], a["g"], a["m"], a["v"], step, search, lr, a["scale"], cls, pred, a["target"],
                     c["targeted"], a["constrain"], rows, a["best_loss"], a["best_attack"], a["best_bs"], a["best_step"],
                     a["iter_best_loss"], a["iter_best_score"], nn_ao=found["nn_ao"] if cd or curv else None,
                     nn_oa=found["nn_oa"] if cd and c["two_sided"] else None, knn_idx=found["knn_idx"] if curv else None,
                     normal_ori=a["normal"] if curv else None, kappa_ori=a["kappa_ori"] if curv else None,
                     dis_kind=c["dis_loss_type"], gval=a["gval"], w_dis=c["w_dis"], w_hd=c["w_hd"], w_curv=c["w_curv"],
                     scheduler=c["scheduler"], cc_linf=c["cc_linf"], terms_out=terms, hd_arg_out=hd_arg, g_out=g_out, lengths=lens)
    torch.cuda.synchronize(dev)
    out = {k: a[k] for k in ("x", "offset", "m", "v", "best_attack", "best_loss", "iter_best_loss", "best_step", "best_bs",
                             "iter_best_score")}
    out.update(g=g_out, constrain_word=a["constrain"], hd_arg=hd_arg, pred=pred, lr=lr, step=step, rows=rows, terms=terms)
    return out


# L2 has no Hausdorff term: (kind, curvature, Hausdorff weight, scheduler)
MIXES = [m for m in itertools.product(("two", "single", "l2"), (True, False), (True, False), (True, False))
         if not (m[0] == "l2" and m[2])]


def _mix(kind, curv, hd, sched):
    return dict(dis_loss_type="L2" if kind == "l2" else "CD", two_sided=kind == "two", w_curv=1.0 if curv else 0.,
                w_hd=0.1 if hd else 0., scheduler=sched, t=2)


@pytest.mark.parametrize("N", [1023, 1024, 1025, 2048])
def test_full_lengths_equal_the_dense_launch(dev, N):
    t = _to_dev(rs.inputs(N, 2, gc.K), dev)
    found = _search(dev, t["x"], t["ori"], gc.K)
    lens = _lens([N, N], dev)
    for mix in MIXES:
        c = _mix(*mix)
        dense, ragged = _launch(t, found, **c), _launch(t, found, lens, **c)
        for n in POINT_OUT + WORD_OUT + ("rows", "terms"):
            assert _same_bits(ragged[n], dense[n]), (n, mix)
        assert not _same_bits(dense["x"], t["x"]) and not _untouched(dense["g"])
        assert dense["step"].tolist() == [3, 3] and (dense["lr"].tolist() == [0.01 * 0.9990] * 2) == mix[3]


@functools.lru_cache(maxsize=None)
def _padded_case(name, dev, clip=False):
    """The clouds of gc.LENGTHS (name "cap": Kmax = 2048, k = 16) or gc.SMALL_LENGTHS ("small": k = 2) as one padded batch on
    the device, shared and never modified: every float buffer holds the payload NaN behind a length — ori too, whose padding
    the kernel does not read either —, every index buffer 0x7fffffff. Returns (t, found, alone, lengths, k): alone[b] = (the
    cloud's own tensors [1, ..], its own search results)."""
    lengths, k = (gc.LENGTHS, gc.K) if name == "cap" else (gc.SMALL_LENGTHS, gc.SMALL_K)
    B, kmax = len(lengths), max(lengths)
    cases = [_to_dev(gc.inputs(L, k, b, clip), dev) for b, L in enumerate(lengths)]
    t = {n: _nan_fill((B, 3, kmax), dev) for n in POINTS}
    t["kappa_ori"] = _nan_fill((B, kmax), dev)
    found = dict(nn_ao=torch.full((B, kmax), BAD_INDEX, dtype=torch.int32, device=dev),
                 nn_oa=torch.full((B, kmax), BAD_INDEX, dtype=torch.int32, device=dev),
                 knn_idx=torch.full((B, kmax, k + 1), BAD_INDEX, dtype=torch.int32, device=dev))
    alone = []
    for b, (L, inp) in enumerate(zip(lengths, cases)):
        for n in POINTS:
            t[n][b, :, :L] = inp[n][0]
        t["kappa_ori"][b, :L] = inp["kappa_ori"][0]
        f1 = _search(dev, inp["x"], inp["ori"], k)
        for n in found:
            found[n][b, :L] = f1[n][0]
        alone.append((inp, f1))
    for n in WORDS:
        t[n] = torch.cat([inp[n] for inp in cases]).contiguous()
    t["lr"], t["gval"] = cases[0]["lr"], cases[0]["gval"]
    return t, found, alone, lengths, k


def _check_against_alone(dev, name, clip=False, **c):
    t, found, alone, lengths, k = _padded_case(name, dev, clip)
    kmax = max(lengths)
    out = _launch(t, found, _lens(lengths, dev), **c)
    cd_or_curv = c.get("dis_loss_type", "CD") == "CD" or c.get("w_curv", 1.0) != 0
    for b, L in enumerate(lengths):
        one = _launch(*alone[b], **c)
        for n in POINT_OUT:
            assert _same_bits(out[n][b, :, :L], one[n][0]), (n, b)
            assert bool(torch.isfinite(one[n]).all()), (n, b)
        for n in WORD_OUT:
            assert _same_bits(out[n][b:b + 1], one[n]), (n, b)
        assert _same_bits(out["rows"][:, b], one["rows"][:, 0]) and _same_bits(out["terms"][:, b], one["terms"][:, 0]), b
        assert bool(torch.isfinite(out["rows"][:, b]).all()) and bool(torch.isfinite(out["terms"][:, b]).all()), b
        # behind the length: x holds the NEW row 0, m / v / offset / g_out are untouched
        assert _same_bits(out["x"][b, :, L:], out["x"][b, :, :1].expand(3, kmax - L)), b
        assert not _same_bits(out["x"][b, :, 0], t["x"][b, :, 0]), b
        for n in ("m", "v", "offset", "g"):
            assert _untouched(out[n][b, :, L:]), (n, b)
        # the record (clouds 0, 3, 6: b % 3 == 0) copies the iterate as it arrived, its padding as copies of ITS row 0
        if b % 3 == 0:
            assert int(out["best_step"][b]) == c.get("t", 0) and _same_bits(out["best_attack"][b, :, :L], t["x"][b, :, :L]), b
            assert _same_bits(out["best_attack"][b, :, L:], t["x"][b, :, :1].expand(3, kmax - L)), b
        else:
            assert int(out["best_step"][b]) == -1 and _untouched(out["best_attack"][b, :, L:]), b
        if cd_or_curv and c.get("dis_loss_type", "CD") == "CD":
            assert 0 <= int(out["hd_arg"][b]) < L, b
    assert not torch.isnan(out["x"]).any()
    for n in ("best_loss", "iter_best_loss", "constrain_word", "lr"):
        assert bool(torch.isfinite(out[n]).all()), n


@pytest.mark.parametrize("mix", [("two", True, True, False), ("single", False, True, True), ("l2", False, False, False),
                                 ("two", True, False, True)], ids=lambda m: "-".join(str(v) for v in m))
def test_every_cloud_of_the_padded_batch_equals_the_dense_launch_alone(dev, mix):
    _check_against_alone(dev, "cap", **_mix(*mix))


def test_padded_batch_with_lp_clip_and_the_small_cloud(dev):
    _check_against_alone(dev, "cap", clip=True, **gc.CONFIGS["clip_scheduler"])
    _check_against_alone(dev, "small", **gc.CONFIGS["default"])          # k = 2, a cloud of L = 4 = the normals' minimum
    _check_against_alone(dev, "small", **_mix("single", True, True, True))


@pytest.mark.parametrize("name,config", [("cap", "default"), ("cap", "clip_scheduler"), ("small", "default")])
def test_ragged_launch_against_float64(dev, name, config):
    """rs.step per cloud on its own L rows and index arrays (the product's own searches, so ties cannot matter), held to the
    bands of tests/test_geoa3_step_gpu.py: cw_step_restatement.bands — 16 x the fp32 restatement's own deviation from float64
    on the same input, floor 16 x 2^-24 max|ref| —, per cloud; the copies and every integer output exact."""
    clip = config == "clip_scheduler"
    over = gc.CONFIGS[config]
    t, found, alone, lengths, k = _padded_case(name, dev, clip)
    out = {n: v.cpu() for n, v in _launch(t, found, _lens(lengths, dev), **over).items()}
    for b, L in enumerate(lengths):
        inp = gc.inputs(L, k, b, clip)
        nb = {n: v.cpu() for n, v in alone[b][1].items()}
        ref64, ref32 = rs.step(torch.float64, inp, nb, **dict(over)), rs.step(torch.float32, inp, nb, **dict(over))
        band = rs.bands(ref64, ref32, names=rs.FLOAT_OUT)
        got = {n: out[n][b:b + 1, :, :L] for n in ("x", "offset", "m", "v", "g", "best_attack")}
        got.update({n: out["terms"][i, b:b + 1] for i, n in enumerate(rs.TERM_OUT)})
        got.update({n: out[n][b:b + 1] for n in ("best_loss", "iter_best_loss", "best_step", "best_bs", "iter_best_score", "pred")})
        got["hd_arg"] = out["hd_arg"][b:b + 1].long()
        for n in rs.FLOAT_OUT:
            err = float((got[n].double() - ref64[n]).abs().max())
            print(f"{config} L={L} {n}: deviation {err:.3g}, band {band[n]:.3g}")
            assert err <= band[n], (n, b)
        for n in rs.EXACT_OUT:
            assert torch.equal(got[n], ref32[n]), (n, b)
        for n in rs.INT_OUT + ("pred",):
            assert torch.equal(got[n], ref64[n]), (n, b, got[n], ref64[n])
        assert float(out["lr"][b]) == ref64["lr"] and int(out["step"][b]) == over["t"] + 1, b
        assert torch.equal(out["rows"][over["t"], b:b + 1], got["loss_n"]) and float(out["rows"][over["t"] + 1, b]) == 0., b
        if clip and L >= 64:
            ln = got["offset"].norm(dim=1)
            assert int((ln > 0.0499).sum()) > 0 and int((ln < 0.049).sum()) > 0, b


def test_update_wrapper_refuses_bad_lengths(dev):
    t = _to_dev(rs.inputs(67, 3, 2), dev)
    found = _search(dev, t["x"], t["ori"], 2)
    for bad in ([67, 67, 67], _lens([67, 67], dev), _lens([67, 67, 67], dev).long(), torch.tensor([67, 67, 67], dtype=torch.int32)):
        with pytest.raises(ValueError, match="lengths must be a contiguous int32"):
            _launch(t, found, bad)


# ----------------------------------------------------------------------------------------------------------------------
# the original cloud's normals and curvature
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cap", "small"])
def test_ragged_normals_and_kappa_ori(dev, name):
    t, _, alone, lengths, k = _padded_case(name, dev)
    kmax = max(lengths)
    pc = t["ori"]                        # the payload NaN behind every length: not read
    lens = _lens(lengths, dev)
    normal = utility.estimate_normal_ragged(pc, 3, lens, lengths)
    again = utility.estimate_normal_ragged(pc, 3, lens)                  # the lengths read back
    kap = loss_utils._get_kappa_ori_ragged(pc, normal, k, lens, lengths)
    assert tuple(normal.shape) == (len(lengths), 3, kmax) and tuple(kap.shape) == (len(lengths), kmax)
    assert _same_bits(normal, again) and not torch.isnan(normal).any() and not torch.isnan(kap).any()
    assert _untouched(pc[0, :, lengths[0]:]) and _untouched(pc[-1, :, lengths[-1]:])      # the input is left alone
    for b, L in enumerate(lengths):
        one = alone[b][0]["ori"]
        n1 = utility.estimate_normal(one, k=3)
        assert _same_bits(normal[b, :, :L], n1[0]), b
        assert _same_bits(normal[b, :, L:], normal[b, :, :1].expand(3, kmax - L)), b
        assert _same_bits(kap[b, :L], loss_utils._get_kappa_ori(one, n1, k)[0]), b
        assert not kap[b, L:].any(), b
    short = list(lengths[:-1]) + [3]
    with pytest.raises(ValueError, match="exceeds the reference length"):
        utility.estimate_normal_ragged(pc, 3, _lens(short, dev), short)


# ----------------------------------------------------------------------------------------------------------------------
# the whole attack
# ----------------------------------------------------------------------------------------------------------------------
ATTACK_LENGTHS = [1025, 1024, 1023, 257, 65, 64, 17]
AB = len(ATTACK_LENGTHS)
SEEDS = [3000 + i for i in range(AB)]
ORDER = [3, 6, 0, 5, 1, 4, 2]
LOSS_MIXES = {"default": {}, "l2_no_curv": dict(dis_loss_type="L2", hd_loss_weight=0, curv_loss_weight=0)}
_MODELS = {}


class _NoPadInvariance(torch.nn.Module):
    """A transfer model that does not declare pad_invariant: the attack must hand it every cloud alone."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner
        self.sizes = []

    def forward(self, x):
        self.sizes.append(tuple(x.shape))
        return self.inner(x)


def _victim(ft, dev):
    if ("v", ft) not in _MODELS:
        if ft:
            m = pointnet.PointNetCls(k=40, feature_transform=True)
            m.load_state_dict(ort.seeded_state_dict(m, 0))
            _MODELS["v", ft] = m.eval().to(dev)
        else:
            _MODELS["v", ft] = hip_pointnet(0, dev)[0]
    return _MODELS["v", ft]


def _transfer(dev):
    if "t" not in _MODELS:
        _MODELS["t"] = hip_pointnet(1, dev)[0]
    return _MODELS["t"]


@functools.lru_cache(maxsize=None)
def _clouds():
    rng = np.random.default_rng(91)
    return [unit_cloud(rng, n) for n in ATTACK_LENGTHS]


@functools.lru_cache(maxsize=None)
def _labels(ft, dev):
    data, _ = cloud_io.stack_ragged(_clouds())
    with torch.no_grad():
        return _victim(ft, dev)(torch.from_numpy(data).transpose(1, 2).contiguous().to(dev))[0].argmax(1).cpu()


def _run(victim, pc, labels, seeds, lengths=None, pt=None, **over):
    if lengths is not None:
        over = dict(over, lengths=lengths)
    cfg = _geo_cfg(device_loop=True, iter_max_steps=19, binary_max_steps=2, sample_seeds=list(seeds), global_batch=AB, **over)
    best, _, mask, steps, losses = ga.geoA3_attack(victim, pt, None, None, None, None, pc, labels, cfg, 0, 1)
    assert ga.geoA3_attack.last_path == "device_loop"
    return dict(best=best.cpu().numpy(), mask=np.asarray(mask), steps=list(steps), losses=np.array(losses),
                pt_fail=ga.geoA3_attack.last_transfer_fails["pt"])


@functools.lru_cache(maxsize=None)
def _alone(mix, ft, dev):
    """Every cloud attacked alone: B = 1, N = its length, its own seed, global_batch = B, eager."""
    victim, labels = _victim(ft, dev), _labels(ft, dev)
    return [_run(victim, torch.from_numpy(c)[None], labels[b:b + 1], [SEEDS[b]], pt=_transfer(dev), graph_victim=False,
                 **LOSS_MIXES[mix]) for b, c in enumerate(_clouds())]


def _check_attack(r, order, mix, ft, dev):
    alone = _alone(mix, ft, dev)
    kmax = max(ATTACK_LENGTHS)
    assert r["best"].dtype == np.float32 and r["best"].shape == (AB, 3, kmax) and r["losses"].shape == (19, AB)
    for b, src in enumerate(order):
        L, one = ATTACK_LENGTHS[src], alone[src]
        assert np.array_equal(r["best"][b, :, :L], one["best"][0]), (b, float(np.abs(r["best"][b, :, :L] - one["best"][0]).max()))
        assert np.array_equal(r["best"][b, :, L:], np.broadcast_to(r["best"][b, :, :1], (3, kmax - L))), b
        assert r["mask"][b] == one["mask"][0] and r["steps"][b] == one["steps"][0], b
        assert np.array_equal(r["losses"][:, b], one["losses"][:, 0]), b
    assert np.isfinite(r["losses"]).all() and not np.isnan(r["best"]).any()
    assert r["pt_fail"] == sum(a["pt_fail"] for a in alone)
    return sum(bool(a["mask"][0]) for a in alone)


def _ragged_loops(victim):
    return [lp for lp in victim._geoa3_loop_cache.values() if lp.bufs.get("lens") is not None]


@pytest.mark.parametrize("mix,ft,graph", [("default", False, True), ("default", False, False), ("l2_no_curv", False, True),
                                          ("l2_no_curv", False, False), ("default", True, True)],
                         ids=["default-graph", "default-eager", "l2-graph", "l2-eager", "feature_transform-graph"])
def test_ragged_attack_equals_the_attacks_alone(dev, mix, ft, graph):
    victim, labels = _victim(ft, dev), _labels(ft, dev)
    _alone(mix, ft, dev)                       # first: its dense loops pass through the victim's loop cache
    data, lengths = cloud_io.stack_ragged(_clouds())
    # the L2 runs: the transfer model without pad_invariant, evaluated cloud by cloud
    tm = _NoPadInvariance(_transfer(dev)) if mix == "l2_no_curv" else _transfer(dev)
    kw = dict(LOSS_MIXES[mix], **({} if graph else {"graph_victim": False}))
    r = _run(victim, torch.from_numpy(data), labels, SEEDS, lengths=lengths, pt=tm, **kw)
    found = _check_attack(r, list(range(AB)), mix, ft, dev)
    print(f"ragged GeoA3 {mix} ft={ft} graph={graph}: found {found}/{AB}, steps {r['steps']}, pt_fail {r['pt_fail']}")
    if mix == "l2_no_curv":
        assert tm.sizes == [(1, 3, L) for L in ATTACK_LENGTHS]
    # a second call with permuted lengths (a tensor this time): the same loop, and nothing new is captured
    loops = _ragged_loops(victim)
    loop = loops[-1]
    graphs = loop.graphs
    assert (graphs is not None) == graph
    n_loops = len(victim._geoa3_loop_cache)
    data2, lengths2 = cloud_io.stack_ragged([_clouds()[s] for s in ORDER])
    r2 = _run(victim, torch.from_numpy(data2), labels[ORDER], [SEEDS[s] for s in ORDER], lengths=torch.from_numpy(lengths2), pt=tm,
              **kw)
    assert len(victim._geoa3_loop_cache) == n_loops and _ragged_loops(victim)[-1] is loop and loop.graphs is graphs
    assert loop.bufs["lens"].tolist() == [ATTACK_LENGTHS[s] for s in ORDER]
    _check_attack(r2, ORDER, mix, ft, dev)


def test_nan_behind_the_lengths_equals_the_padded_input(dev):
    victim, labels = _victim(False, dev), _labels(False, dev)
    data, lengths = cloud_io.stack_ragged(_clouds())
    holes = np.full(data.shape, NAN_WORD, dtype=np.int32).view(np.float32)
    for b, c in enumerate(_clouds()):
        holes[b, :len(c)] = c
    a = _run(victim, torch.from_numpy(data), labels, SEEDS, lengths=lengths)
    given = torch.from_numpy(holes).to(dev)
    b_ = _run(victim, given, labels, SEEDS, lengths=[int(n) for n in lengths])
    for n in ("best", "mask", "losses"):
        assert np.array_equal(a[n], b_[n]), n
    assert a["steps"] == b_["steps"] and not np.isnan(b_["best"]).any()
    assert np.array_equal(given.cpu().numpy().view(np.int32), holes.view(np.int32))          # the caller's tensor is left alone


def test_no_lengths_is_the_dense_attack(dev):
    victim = _victim(False, dev)
    pcs = torch.from_numpy(np.stack([unit_cloud(np.random.default_rng(53 + i), 300) for i in range(3)]))
    with torch.no_grad():
        labels = victim(pcs.transpose(1, 2).contiguous().to(dev))[0].argmax(1).cpu()
    outs = []
    for kw in ({}, {"lengths": None}):           # the attribute absent, and None
        cfg = _geo_cfg(device_loop=True, sample_seeds=[5, 6, 7], **kw)
        plan = ga._device_loop_plan(victim, cfg, 3, 300, False)
        assert plan is not None and "ragged" not in plan
        best, _, mask, steps, losses = ga.geoA3_attack(victim, None, None, None, None, None, pcs, labels, cfg, 0, 1)
        outs.append((best.cpu().numpy(), mask, steps, np.array(losses)))
    assert all(np.array_equal(x, y) for x, y in zip(outs[0], outs[1]))
    assert not _ragged_loops(victim) or all(lp.bufs["x"].shape[2] != 300 for lp in _ragged_loops(victim))


class _NoPadPointNet(pointnet.PointNetCls):
    pad_invariant = False


def test_lengths_raise_where_there_is_no_ragged_loop(dev):
    victim = hip_pointnet(0, dev)[0]
    rng = np.random.default_rng(2)
    data, lengths = cloud_io.stack_ragged([unit_cloud(rng, n) for n in (70, 64, 17)])
    x, y = torch.from_numpy(data), torch.tensor([1, 2, 3])

    def call(model=victim, lens=lengths, **over):
        cfg = _geo_cfg(**{"device_loop": True, "lengths": lens, **over})
        return ga.geoA3_attack(model, None, None, None, None, None, x, y, cfg, 0, 1)

    nopad = _NoPadPointNet(k=40)
    nopad.load_state_dict(victim.state_dict())
    training = hip_pointnet(0, dev)[0].train()
    ga.geoA3_attack.last_path = None
    cases = [(dict(model=nopad.eval().to(dev)), "pad_invariant"),
             (dict(model=dfn.FusedDefended(victim, dfn.SORDefense(2, 1.1, 70))), "pad_invariant|refuses"),
             (dict(model=training), "refuses"), (dict(uniform_loss_weight=0.1), "refuses"), (dict(optim='sgd'), "refuses"),
             (dict(is_pro_grad=True), "refuses"), (dict(cls_loss_type='None'), "refuses"),
             (dict(dis_loss_type='L2'), "refuses"),                      # L2 with the Hausdorff weight on
             (dict(device_loop=False), "device_loop"), (dict(lens=[70, 64]), "lengths must"),
             (dict(lens=[70, 64, 16]), "lengths must"), (dict(lens=[71, 64, 17]), "lengths must")]
    for kw, word in cases:
        with pytest.raises(ValueError, match=word):
            call(**kw)
    assert ga.geoA3_attack.last_path is None and "_geoa3_loop_cache" not in victim.__dict__
