"""GPU: clouds of different sizes in the kNN attack's device loop — the ragged search (pc3d_knn_ragged_f32) against the dense
search of every cloud alone, the ragged update (pc3d_knn_attack_update_ragged_f32) against the dense launch and against the
float64 restatement, and CWKNN.attack(data, target, lengths) against the same clouds attacked alone.

The lengths sit on both sides of the search's 2048-candidate tile (2049 | 2048), of its 64-candidate step (65 | 64), of the
update kernel's 1024-thread stride (1025 | 1024), and at L = k + 1 (6). Rows at and beyond a length hold a payload NaN."""
import functools
import importlib

import numpy as np
import pytest
import torch

import knn_step_restatement as rs
from helpers import hip_pointnet, unit_cloud
from oracle import ref_torch as ort

pytestmark = pytest.mark.gpu
M = importlib.import_module
ops = M("3dpointcloudattack_amd.ops")
lib = M("3dpointcloudattack_amd._lib")
pointnet = M("3dpointcloudattack_amd.model.pointnet")
dfn = M("3dpointcloudattack_amd.defense")
graphed = M("3dpointcloudattack_amd.graphed")
cloud_io = M("3dpointcloudattack_amd.dataset.cloud_io")
knnm = M("3dpointcloudattack_amd.attack.KNN.KNN_attack")
adv_u = M("3dpointcloudattack_amd.attack.CW.CW_utils.adv_utils")
dist_u = M("3dpointcloudattack_amd.attack.CW.CW_utils.dist_utils")
clip_u = M("3dpointcloudattack_amd.attack.CW.CW_utils.clip_utils")

LENGTHS = [2049, 2048, 1025, 1024, 65, 64, 6]
KMAX = 2049
K_NN = 5
K1 = K_NN + 1
B = len(LENGTHS)
NAN_WORD = 0x7FC00ABC            # the payload NaN of tests/test_cw_ragged_gpu.py: survives only if nobody writes the word


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
    return torch.tensor(lengths, dtype=torch.int32, device=dev)


@functools.lru_cache(maxsize=None)
def _clouds():
    rng = np.random.default_rng(78)
    return [unit_cloud(rng, n) for n in LENGTHS]


def _padded(dev, nan=True):
    """x [B,3,KMAX]: cloud b in its first LENGTHS[b] columns, the payload NaN (or copies of point 0) behind them."""
    data, _ = cloud_io.stack_ragged(_clouds())
    x = torch.from_numpy(data).transpose(1, 2).contiguous().to(dev)
    if nan:
        for b, L in enumerate(LENGTHS):
            x[b, :, L:] = _nan_fill((3, KMAX - L), dev)
    return x


# ----------------------------------------------------------------------------------------------------------------------
# 1. the search
# ----------------------------------------------------------------------------------------------------------------------
def _dense_knn(x, K, hint=None, entry="pc3d_knn_f32"):
    """pc3d_knn_f32 (or pc3d_knn_hint_f32) of the contiguous [B,3,N] clouds x on themselves."""
    Bx, _, N = x.shape
    d = torch.zeros((Bx, N, K), dtype=torch.float32, device=x.device)
    i = torch.zeros((Bx, N, K), dtype=torch.int32, device=x.device)
    pts = (x.data_ptr(), 3 * N, 1, N)
    extra = () if entry == "pc3d_knn_f32" else (hint.data_ptr() if hint is not None else 0,)
    with torch.cuda.device(x.device):
        lib.call(entry, *pts, *pts, Bx, N, N, K, d.data_ptr(), i.data_ptr(), *extra, torch.cuda.current_stream().cuda_stream)
    return d, i


@functools.lru_cache(maxsize=None)
def _alone_knn(dev):
    """(d, idx) of every cloud alone from pc3d_knn_f32: computed once, never modified."""
    x = _padded(dev)
    return [_dense_knn(x[b:b + 1, :, :L].contiguous(), K1) for b, L in enumerate(LENGTHS)]


def _check_search(d, idx, dev):
    for b, L in enumerate(LENGTHS):
        d1, i1 = _alone_knn(dev)[b]
        assert _same_bits(d[b, :L], d1[0]) and torch.equal(idx[b, :L], i1[0]), b
        assert _untouched(d[b, L:]) and _untouched(idx[b, L:]), b


def _search_into(x, d, idx, lengths, dev):
    ops.knn_search_into(x, d, idx, lengths=_lens(lengths, dev), lengths_host=lengths)
    torch.cuda.synchronize()
    return d, idx


def test_ragged_search_equals_the_dense_search_of_every_cloud_alone(dev):
    x = _padded(dev)
    lens = _lens(LENGTHS, dev)
    # no hint
    d, idx = ops.knn_ragged(x, x, K1, lens, q_cf=True, r_cf=True)
    for b, L in enumerate(LENGTHS):
        d1, i1 = _alone_knn(dev)[b]
        assert _same_bits(d[b, :L], d1[0]) and torch.equal(idx[b, :L], i1[0]), b
        assert not d[b, L:].any() and not idx[b, L:].any(), b        # the wrapper's zeros: never written
    # hint == idx: the first call finds no usable hint (the payload NaN is out of range), the second one its own result
    assert ops.KNN_HINTS and KMAX >= ops.KNN_HINT_MIN_M
    d, idx = _nan_fill((B, KMAX, K1), dev), _nan_fill((B, KMAX, K1), dev, torch.int32)
    _check_search(*_search_into(x, d, idx, LENGTHS, dev), dev)
    d.copy_(_nan_fill((B, KMAX, K1), dev))
    _check_search(*_search_into(x, d, idx, LENGTHS, dev), dev)
    # a hint of out-of-range entries (negative, beyond the capacity) and duplicates; every other run of 16 rows (a
    # workgroup's queries) names the last K1 rows of the capacity: a usable, poor hint for the full cloud, beyond the cloud
    # for every other one
    g = torch.Generator().manual_seed(5)
    bad = torch.randint(-4, KMAX + 4, (B, KMAX, K1), generator=g, dtype=torch.int32)
    bad[:, ::3, 1] = bad[:, ::3, 0]
    bad[:, (torch.arange(KMAX) // 16) % 2 == 1] = KMAX - 1 - torch.arange(K1, dtype=torch.int32)
    idx.copy_(bad.to(dev))
    for b, L in enumerate(LENGTHS):
        idx[b, L:] = _nan_fill((KMAX - L, K1), dev, torch.int32)
    _check_search(*_search_into(x, d, idx, LENGTHS, dev), dev)
    # ... as an explicit hint buffer too
    d2, i2 = ops.knn_ragged(x, x, K1, lens, q_cf=True, r_cf=True, hint=bad.to(dev))
    for b, L in enumerate(LENGTHS):
        assert _same_bits(d2[b, :L], d[b, :L]) and torch.equal(i2[b, :L], idx[b, :L]), b


@pytest.mark.parametrize("N", [64, 65, 2048, 2049])
def test_full_lengths_search_equals_the_dense_launch(dev, N):
    rng = np.random.default_rng(N)
    x = torch.from_numpy(np.stack([unit_cloud(rng, N) for _ in range(2)])).transpose(1, 2).contiguous().to(dev)
    lens = _lens([N, N], dev)
    for K in (1, K1):
        want = _dense_knn(x, K, None, "pc3d_knn_hint_f32")
        got = ops.knn_ragged(x, x, K, lens, q_cf=True, r_cf=True)
        assert _same_bits(got[0], want[0]) and torch.equal(got[1], want[1]), K
    moved = x + 1e-3 * torch.randn(x.shape, generator=torch.Generator().manual_seed(1)).to(dev)
    want = _dense_knn(moved, K1, got[1], "pc3d_knn_hint_f32")
    hinted = ops.knn_ragged(moved, moved, K1, lens, q_cf=True, r_cf=True, hint=got[1])
    assert _same_bits(hinted[0], want[0]) and torch.equal(hinted[1], want[1])


def test_one_captured_search_serves_other_lengths(dev):
    x = _padded(dev, nan=False)
    for b in range(B):                       # every row a point of its own: any length is a cloud
        x[b] = torch.from_numpy(unit_cloud(np.random.default_rng(100 + b), KMAX)).t().to(dev)
    other = LENGTHS[::-1]
    lens = _lens(LENGTHS, dev)
    host = np.array(LENGTHS)
    d, idx = _nan_fill((B, KMAX, K1), dev), _nan_fill((B, KMAX, K1), dev, torch.int32)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.knn_search_into(x, d, idx, lengths=lens, lengths_host=host)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with graphed.capture_guard():
        with torch.cuda.graph(graph):
            ops.knn_search_into(x, d, idx, lengths=lens, lengths_host=host)
    for lengths in (LENGTHS, other):
        lens.copy_(_lens(lengths, dev))
        d.copy_(_nan_fill(d.shape, dev)), idx.copy_(_nan_fill(idx.shape, dev, torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        for b, L in enumerate(lengths):
            d1, i1 = _dense_knn(x[b:b + 1, :, :L].contiguous(), K1)
            assert _same_bits(d[b, :L], d1[0]) and torch.equal(idx[b, :L], i1[0]), (lengths, b)
            assert _untouched(d[b, L:]) and _untouched(idx[b, L:]), (lengths, b)


def test_search_refuses_a_cloud_with_fewer_points_than_k(dev):
    x = _padded(dev, nan=False)
    d, idx = torch.zeros((B, KMAX, K1), device=dev), torch.zeros((B, KMAX, K1), dtype=torch.int32, device=dev)
    short = LENGTHS[:-1] + [K1 - 1]
    with pytest.raises(ValueError, match="exceeds the cloud length"):
        ops.knn_search_into(x, d, idx, lengths=_lens(short, dev), lengths_host=short)
    with pytest.raises(ValueError, match="exceeds the cloud length"):
        ops.knn_search_into(x, d, idx, lengths=_lens(short, dev))                       # read back
    with pytest.raises(ValueError, match="exceeds the reference length"):
        ops.knn_ragged(x, x, K1, _lens(short, dev), q_cf=True, r_cf=True)
    with pytest.raises(ValueError, match="lengths must be a contiguous int32"):
        ops.knn_search_into(x, d, idx, lengths=LENGTHS)


# ----------------------------------------------------------------------------------------------------------------------
# 2. the update
# ----------------------------------------------------------------------------------------------------------------------
POINTS = ("adv", "ori", "normal", "g", "m", "v")


@functools.lru_cache(maxsize=None)
def _cases(alpha):
    """One case of rs.inputs per length (B = 1, k = 5, with normals): shared, never modified."""
    cases = [rs.inputs(L, 1, K_NN, True, alpha) for L in LENGTHS]
    for L, inp in zip(LENGTHS, cases):       # the outlier decisions are farther from the threshold than fp32 can move them
        assert float(rs.mask_margin(inp["adv"], K_NN, alpha)[3].min()) > rs.MARGIN, L
    return cases


def _padded_case(alpha, dev):
    """The cases as one padded batch on the device: rows at and beyond a length hold the payload NaN (ori: copies of its
    point 0, as the attack pads it), and so do the two search results there. Returns (tensors, found, per-cloud found)."""
    t = {n: _nan_fill((B, 3, KMAX), dev) for n in POINTS}
    knn_d, knn_idx = _nan_fill((B, KMAX, K1), dev), _nan_fill((B, KMAX, K1), dev, torch.int32)
    nn_idx = _nan_fill((B, KMAX), dev, torch.int32)
    for b, (L, inp) in enumerate(zip(LENGTHS, _cases(alpha))):
        for n in POINTS:
            t[n][b, :, :L] = inp[n][0].to(dev)
        t["ori"][b, :, L:] = t["ori"][b, :, :1]
    lens = _lens(LENGTHS, dev)
    ops.knn_search_into(t["adv"], knn_d, knn_idx, lengths=lens, lengths_host=LENGTHS)
    alone = []
    for b, L in enumerate(LENGTHS):
        a1, o1 = t["adv"][b:b + 1, :, :L].contiguous(), t["ori"][b:b + 1, :, :L].contiguous()
        nn1 = ops.nn_raw(a1, o1, True, True)[1]
        nn_idx[b, :L] = nn1[0]
        alone.append((knn_d[b:b + 1, :L].contiguous(), knn_idx[b:b + 1, :L].contiguous(), nn1))
    return t, (knn_d, knn_idx, nn_idx), alone


def _scales(lengths, with_knn=True):
    return ops.knn_attack_scales_ragged(lengths, K_NN if with_knn else 0, 1, rs.W1, rs.W2 if with_knn else None)


def _launch(t, found, c_ch, c_knn, alpha, project, lens=None):
    a = {n: t[n].clone() for n in POINTS}
    step = torch.tensor([rs.T], dtype=torch.int32, device=a["adv"].device)
    ops.knn_attack_update(a["adv"], a["ori"], a["g"], a["m"], a["v"], step, rs.LR, found[0], found[1], found[2], c_ch, c_knn,
                          alpha, rs.BUDGET, "project_clip" if project else "clip", a["normal"], lengths=lens)
    torch.cuda.synchronize()
    return {n: a[n] for n in rs.FLOAT_OUT}


@pytest.mark.parametrize("project", [True, False])
@pytest.mark.parametrize("with_knn", [True, False])
@pytest.mark.parametrize("N", [1023, 1024, 1025, 2049])
def test_full_lengths_update_equals_the_dense_launch(dev, N, with_knn, project):
    inp = rs.inputs(N, 2, K_NN, True)
    t = {n: inp[n].to(dev) for n in POINTS}
    knn_d = torch.zeros((2, N, K1), dtype=torch.float32, device=dev)
    knn_idx = torch.zeros((2, N, K1), dtype=torch.int32, device=dev)
    ops.knn_search_into(t["adv"], knn_d, knn_idx)
    found = (knn_d, knn_idx, ops.nn_raw(t["adv"], t["ori"], True, True)[1])
    up = np.float32(N)
    c_ch, c_knn = ops.knn_attack_scales(N, K_NN if with_knn else 0, 2, up * np.float32(rs.W1),
                                        up * np.float32(rs.W2) if with_knn else None)
    dense = _launch(t, found, c_ch, c_knn, rs.ALPHA, project)
    ragged = _launch(t, found, np.full(2, c_ch, np.float32), np.full(2, c_knn, np.float32), rs.ALPHA, project, _lens([N, N], dev))
    for n in rs.FLOAT_OUT:
        assert _same_bits(ragged[n], dense[n]), n
    assert not _same_bits(dense["adv"], t["adv"])


@pytest.mark.parametrize("with_knn", [True, False])
def test_ragged_update_equals_the_dense_launch_on_every_cloud_alone(dev, with_knn):
    t, found, alone = _padded_case(rs.ALPHA, dev)
    c_ch, c_knn = _scales(LENGTHS, with_knn)
    out = _launch(t, found, c_ch, c_knn, rs.ALPHA, True, _lens(LENGTHS, dev))
    assert not torch.isnan(out["adv"]).any()
    for b, L in enumerate(LENGTHS):
        one = _launch({n: t[n][b:b + 1, :, :L].contiguous() for n in POINTS}, alone[b], c_ch[b], c_knn[b], rs.ALPHA, True)
        for n in rs.FLOAT_OUT:
            assert _same_bits(out[n][b, :, :L], one[n][0]), (n, b)
        assert _same_bits(out["adv"][b, :, L:], out["adv"][b, :, :1].expand(3, KMAX - L)), b      # the NEW point 0
        assert not _same_bits(out["adv"][b, :, 0], t["adv"][b, :, 0]), b
        assert _untouched(out["m"][b, :, L:]) and _untouched(out["v"][b, :, L:]), b


@pytest.mark.parametrize("alpha", [rs.ALPHA, rs.HEAVY_ALPHA], ids=["alpha1.05", "alpha0"])
def test_ragged_update_against_float64(dev, alpha):
    """rs.step per cloud on the [:L] slices, on the indices the product's own searches found; the bands of
    tests/test_knn_step_gpu.py (cw_step_restatement.bands: 16 x the fp32 restatement's own deviation from float64, floor
    16 x 2^-24 max|ref|), per cloud. alpha = 0: about a fifth of the points are masked, so the edges of the large clouds fill
    more than one staging trip."""
    t, found, alone = _padded_case(alpha, dev)
    c_ch, c_knn = _scales(LENGTHS)
    out = _launch(t, found, c_ch, c_knn, alpha, True, _lens(LENGTHS, dev))
    for b, (L, inp) in enumerate(zip(LENGTHS, _cases(alpha))):
        idx = dict(knn_idx=alone[b][1].cpu(), nn_idx=alone[b][2].cpu())
        ref64 = rs.run(torch.float64, inp, k=K_NN, alpha=alpha, **idx)
        band = rs.bands(ref64, rs.run(torch.float32, inp, k=K_NN, alpha=alpha, **idx), names=rs.FLOAT_OUT)
        for n in rs.FLOAT_OUT:
            err = float((out[n][b:b + 1, :, :L].double().cpu() - ref64[n]).abs().max())
            print(f"alpha={alpha} L={L} {n}: deviation {err:.3g}, band {band[n]:.3g}")
            assert err <= band[n], (n, b)
    assert not torch.isnan(out["adv"]).any()


# ----------------------------------------------------------------------------------------------------------------------
# 3. the whole attack
# ----------------------------------------------------------------------------------------------------------------------
SEEDS = [2000 + i for i in range(B)]
NUM_ITER = 19          # one block of 16 and three single-iteration replays
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


def _dist(name):
    return dist_u.ChamferkNNDist() if name == "chamfer_knn" else dist_u.ChamferDist()


def _attacker(victim, trans, dist, **kw):
    kw.setdefault("device_loop", True)
    return knnm.CWKNN(victim, trans, None, None, None, None, adv_func=adv_u.UntargetedLogitsAdvLoss(5.), dist_func=_dist(dist),
                      clip_func=clip_u.ProjectInnerClipLinf(0.18), attack_lr=1e-2, num_iter=NUM_ITER, **kw)


@functools.lru_cache(maxsize=None)
def _labels(ft, dev):
    data, _ = cloud_io.stack_ragged(_clouds())
    with torch.no_grad():
        return _victim(ft, dev)(torch.from_numpy(data).transpose(1, 2).contiguous().to(dev))[0].argmax(1).cpu()


@functools.lru_cache(maxsize=None)
def _alone(dist, ft, dev):
    """Every cloud attacked alone: B = 1, K = lengths[b], its own seed, global_batch = B. (clouds, success, attack_fail,
    pt_fail) per cloud."""
    victim, labels = _victim(ft, dev), _labels(ft, dev)
    out = []
    for b, c in enumerate(_clouds()):
        atk = _attacker(victim, _transfer(dev), dist, sample_seeds=[SEEDS[b]], global_batch=B, graph=False)
        adv, sn = atk.attack(torch.from_numpy(c)[None], labels[b:b + 1])
        assert atk.last_path == "device_loop"
        out.append((adv[0], sn, atk.attack_fail, atk.pt_fail))
    return out


def _check_attack(adv, sn, atk, order, dist, ft, dev):
    alone = _alone(dist, ft, dev)
    assert adv.dtype == np.float32 and adv.shape == (B, KMAX, 3) and atk.last_path == "device_loop"
    for b, src in enumerate(order):
        L = LENGTHS[src]
        assert np.array_equal(adv[b, :L], alone[src][0]), (b, float(np.abs(adv[b, :L] - alone[src][0]).max()))
        assert np.array_equal(adv[b, L:], np.broadcast_to(adv[b, 0], (KMAX - L, 3))), b
        assert np.abs(adv[b, :L] - _clouds()[src]).max() > 1e-3, b
    assert sn == sum(a[1] for a in alone)
    assert atk.attack_fail == sum(a[2] for a in alone) and atk.pt_fail == sum(a[3] for a in alone)


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("ft", [False, True], ids=["plain", "feature_transform"])
@pytest.mark.parametrize("dist", ["chamfer", "chamfer_knn"])
def test_ragged_attack_equals_the_attacks_alone(dev, dist, ft, graph):
    victim, labels = _victim(ft, dev), _labels(ft, dev)
    data, lengths = cloud_io.stack_ragged(_clouds())
    # plain Chamfer runs: the transfer model without pad_invariant, evaluated cloud by cloud
    tm = _NoPadInvariance(_transfer(dev)) if dist == "chamfer" else _transfer(dev)
    atk = _attacker(victim, tm, dist, sample_seeds=SEEDS, global_batch=B, graph=graph)
    adv, sn = atk.attack(torch.from_numpy(data), labels, lengths)
    print(f"ragged kNN attack {dist} ft={ft} graph={graph}: success {sn}/{B}, attack_fail {atk.attack_fail}, pt_fail {atk.pt_fail}")
    _check_attack(adv, sn, atk, list(range(B)), dist, ft, dev)
    if dist == "chamfer":
        assert tm.sizes == [(1, 3, L) for L in LENGTHS]
    # a second call with permuted lengths: the same loop, the same graphs
    loop = next(iter(atk._loop_cache.values()))
    graphs = loop.graphs
    assert (graphs is not None) == graph
    order = [3, 6, 0, 5, 1, 4, 2]
    data2, lengths2 = cloud_io.stack_ragged([_clouds()[s] for s in order])
    atk.sample_seeds = [SEEDS[s] for s in order]
    atk.attack_fail = atk.pt_fail = 0
    adv2, sn2 = atk.attack(torch.from_numpy(data2), labels[order], lengths2)
    assert len(atk._loop_cache) == 1 and next(iter(atk._loop_cache.values())) is loop and loop.graphs is graphs
    _check_attack(adv2, sn2, atk, order, dist, ft, dev)


def test_ragged_attack_with_normals_equals_the_attacks_alone(dev):
    """[B, Kmax, 6] input: the positions are a slice of the upload that the attack makes contiguous and pads, the normals go
    to the projection as they are. Rows at and beyond a length hold the payload NaN in all six channels: never read."""
    victim, labels = _victim(False, dev), _labels(False, dev)
    rng = np.random.default_rng(14)
    six = []
    for c in _clouds():
        n = rng.standard_normal(c.shape).astype(np.float32)
        six.append(np.concatenate([c, n / np.linalg.norm(n, axis=1, keepdims=True)], axis=1))
    data = np.full((B, KMAX, 6), NAN_WORD, dtype=np.int32).view(np.float32)
    for b, c in enumerate(six):
        data[b, :len(c)] = c
    atk = _attacker(victim, _transfer(dev), "chamfer_knn", sample_seeds=SEEDS, global_batch=B)
    adv, sn = atk.attack(torch.from_numpy(data), labels, LENGTHS)
    assert atk.last_path == "device_loop" and adv.shape == (B, KMAX, 3) and not np.isnan(adv).any()
    assert next(iter(atk._loop_cache.values())).bufs["normal"] is not None
    total, xyz_only = 0, _alone("chamfer_knn", False, dev)
    for b, c in enumerate(six):
        one = _attacker(victim, _transfer(dev), "chamfer_knn", sample_seeds=[SEEDS[b]], global_batch=B, graph=False)
        adv1, sn1 = one.attack(torch.from_numpy(c)[None], labels[b:b + 1])
        total += sn1
        L = LENGTHS[b]
        assert np.array_equal(adv[b, :L], adv1[0]), (b, float(np.abs(adv[b, :L] - adv1[0]).max()))
        assert np.array_equal(adv[b, L:], np.broadcast_to(adv[b, 0], (KMAX - L, 3))), b
        assert not np.array_equal(adv1[0], xyz_only[b][0]), b            # the normals were used
    assert sn == total


def test_no_lengths_is_the_dense_attack(dev):
    victim = _victim(False, dev)
    rng = np.random.default_rng(53)
    pcs = torch.from_numpy(np.stack([unit_cloud(rng, 300) for _ in range(3)]))
    with torch.no_grad():
        labels = victim(pcs.transpose(1, 2).contiguous().to(dev))[0].argmax(1).cpu()
    outs = []
    for kw in ({}, {"lengths": None}):
        atk = _attacker(victim, None, "chamfer_knn", sample_seeds=[5, 6, 7])
        outs.append(atk.attack(pcs, labels, **kw))
    assert np.array_equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1]


# ----------------------------------------------------------------------------------------------------------------------
# 4. refusals
# ----------------------------------------------------------------------------------------------------------------------
class _NoPadPointNet(pointnet.PointNetCls):
    pad_invariant = False


def test_lengths_raise_where_there_is_no_ragged_loop(dev):
    victim = _victim(False, dev)
    rng = np.random.default_rng(2)
    data, lengths = cloud_io.stack_ragged([unit_cloud(rng, n) for n in (70, 64, 6)])
    x, y = torch.from_numpy(data), torch.tensor([1, 2, 3])
    nopad = _NoPadPointNet(k=40)
    nopad.load_state_dict(victim.state_dict())
    kw = dict(adv_func=adv_u.UntargetedLogitsAdvLoss(5.), dist_func=dist_u.ChamferkNNDist(),
              clip_func=clip_u.ProjectInnerClipLinf(0.18), attack_lr=1e-2, num_iter=2, device_loop=True)

    def make(model=victim, **over):
        return knnm.CWKNN(model, None, None, None, None, None, **{**kw, **over})

    cases = [
        (make(device_loop=False), "device_loop=False"),
        (make(dfn.FusedDefended(victim, dfn.SORDefense(2, 1.1, 70))), "pad_invariant"),
        (make(nopad.eval().to(dev)), "pad_invariant"),
        (make(adv_func=lambda lg, t: lg.sum(1)), "adv_func"),
        (make(dist_func=dist_u.HausdorffDist()), "dist_func HausdorffDist"),
        (make(clip_func=clip_u.ClipPointsL2(0.18)), "clip_func ClipPointsL2"),
        (make(fused=False), "clip_func"),
        (make(dist_func=dist_u.ChamferkNNDist(knn_k=0)), "k=0 out of range"),
        (make(dist_func=dist_u.ChamferkNNDist(knn_k=64)), "k=64 out of range"),
    ]
    moved = pointnet.PointNetCls(k=40)
    moved.load_state_dict(victim.state_dict())
    cases.append((make(moved.eval()), "not on the GPU"))
    moved.cpu()                               # after the attack object put it on the device
    for atk, word in cases:
        with pytest.raises(ValueError, match=word):
            atk.attack(x, y, lengths)
        assert atk.last_path is None and len(atk._loop_cache) == 0
    atk = make()
    for bad in ([70, 64], [70, 64, 5], [71, 64, 6], [0, 64, 6], [70.5, 64., 6.]):
        with pytest.raises(ValueError, match="lengths must"):
            atk.attack(x, y, bad)
    with pytest.raises(ValueError, match="KNN_LOOP_MAX_POINTS"):
        atk.attack(torch.zeros(1, ops.KNN_LOOP_MAX_POINTS + 1, 3), y[:1], [70])
    # plain ChamferDist has k = 0: a single point is a cloud
    one = make(dist_func=dist_u.ChamferDist())
    adv, _ = one.attack(x, y, [70, 64, 1])
    assert one.last_path == "device_loop" and np.array_equal(adv[2], np.broadcast_to(adv[2, 0], adv[2].shape))
