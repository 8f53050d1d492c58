"""GPU: the shape-invariant white-box attack on a batch of clouds of different sizes. The contract is the
other ragged loops': every cloud equals its run alone in every bit, and every padding row of an output is a copy of that
output's row 0. The kernels (pc3d_pca_normal_ragged_f32, pc3d_si_frame_ragged_f32, pc3d_si_step_ragged_f32) are held to
the dense entries on each cloud alone, the attack to eager dense attacks on each cloud alone.

The lengths sit on both sides of every stride in the kernels: si_step's 1024 threads, si_frame's 256-thread blocks, the
wave of 64, and the minimum of 20 (KNN). Rows at and beyond a length are pre-filled with NaN wherever the contract says they
are never read, so a read shows as a NaN in an output.
"""
import importlib

import numpy as np
import pytest
import torch

import siadv_restatement as R
from test_siadv_gpu import (EPS, STEP, _bitwise_only, bound_of, ellipsoid, fx, lay, make_attack, nets,  # noqa: F401
                            step_inputs, unlay)

pytestmark = pytest.mark.gpu

M = importlib.import_module
KNN = 20
LENGTHS = (1100, 1025, 1024, 1023, 65, 64, 20)
KMAX = 1100
LAYOUTS = pytest.mark.parametrize("cf", [False, True], ids=["cl", "cf"])


def rows(t, cf):
    """The device tensor under test as [B,N,3] (a view)."""
    return t.transpose(1, 2) if cf else t


def nan_behind(t, lengths):
    """A copy of the host tensor [B,N,3] with every row at and beyond the cloud's length NaN."""
    t = t.clone()
    for b, L in enumerate(lengths):
        t[b, L:] = float("nan")
    return t


def lens_of(lengths, dev):
    return torch.tensor(lengths, dtype=torch.int32, device=dev)


def check_against_alone(out, alone, b, L, cf, what):
    """Rows < L of cloud b equal the dense entry on the cloud alone, rows >= L equal row 0, everything is finite."""
    o, a = rows(out, cf)[b], rows(alone, cf)[0]
    assert a.shape[0] == L
    assert torch.isfinite(o).all(), (what, b, L)
    assert torch.equal(o[:L], a), (what, b, L)
    assert torch.equal(o[L:], o[:1].expand(o.shape[0] - L, 3)), (what, b, L)


class Batch:
    """Seeded ellipsoid clouds as test_siadv_gpu.step_inputs builds them, on the device in one layout, the padding rows of
    x, ori, g and nrm NaN; the neighbour lists from ops.knn_ragged; and every cloud alone with its own dense search."""

    def __init__(self, ops, dev, lengths, kmax, seed, cf, nan=True):
        self.lengths, self.cf, self.lens = lengths, cf, lens_of(lengths, dev)
        self.host = step_inputs(len(lengths), kmax, seed)                  # P, ori, g, n
        fill = (lambda t: nan_behind(t, lengths)) if nan else (lambda t: t)
        self.x, self.ori, self.g, self.nrm = (lay(fill(t), cf, dev) for t in self.host)
        self.idx = ops.knn_ragged(self.x, self.x, KNN, self.lens, q_cf=cf, r_cf=cf, lengths_host=np.array(lengths))[1]
        self.alone = []
        for b, L in enumerate(lengths):
            xb, ob, gb, nb = (lay(t[b:b + 1, :L], cf, dev) for t in self.host)
            ib = ops.knn_raw(xb, xb, KNN, q_cf=cf, r_cf=cf)[1]
            assert torch.equal(self.idx[b, :L], ib[0])                     # the ragged search's own contract
            self.alone.append((xb, ob, gb, nb, ib))


# ------------------------------------------------------------------------------------------------------
# 1. the kernels against the clouds alone
# ------------------------------------------------------------------------------------------------------
@LAYOUTS
def test_kernels_equal_the_clouds_alone(ops, dev, cf):
    t = Batch(ops, dev, LENGTHS, KMAX, 500, cf)
    pn = ops.pca_normal(t.x, t.idx, cf=cf, lengths=t.lens)
    e_n, no_n = torch.empty_like(t.x), torch.empty_like(t.x)
    ops.si_frame(t.x, nrm=t.nrm, out=e_n, nrm_out=no_n, cf=cf, lengths=t.lens)
    e_i, no_i = torch.empty_like(t.x), torch.empty_like(t.x)
    ops.si_frame(t.x, idx=t.idx, out=e_i, nrm_out=no_i, cf=cf, lengths=t.lens)
    s_n, so_n = t.x.clone(), torch.empty_like(t.x)
    ops.si_step(s_n, t.ori, t.g, STEP, EPS, nrm=t.nrm, nrm_out=so_n, cf=cf, lengths=t.lens)
    s_i, so_i = t.x.clone(), torch.empty_like(t.x)
    ops.si_step(s_i, t.ori, t.g, STEP, EPS, idx=t.idx, nrm_out=so_i, cf=cf, lengths=t.lens)
    s_j = t.x.clone()
    ops.si_step(s_j, t.ori, t.g, STEP, EPS, idx=t.idx, cf=cf, lengths=t.lens)                # the LDS stage alone
    assert torch.equal(s_j, s_i)
    for b, L in enumerate(LENGTHS):
        xb, ob, gb, nb, ib = t.alone[b]
        check_against_alone(pn, ops.pca_normal(xb, ib, cf=cf), b, L, cf, "pca_normal")
        a_no = torch.empty_like(xb)
        check_against_alone(e_n, ops.si_frame(xb, nrm=nb, nrm_out=a_no, cf=cf), b, L, cf, "si_frame nrm: xe")
        check_against_alone(no_n, a_no, b, L, cf, "si_frame nrm: nrm_out")
        a_no = torch.empty_like(xb)
        check_against_alone(e_i, ops.si_frame(xb, idx=ib, nrm_out=a_no, cf=cf), b, L, cf, "si_frame idx: xe")
        check_against_alone(no_i, a_no, b, L, cf, "si_frame idx: nrm_out")
        a, a_no = xb.clone(), torch.empty_like(xb)
        ops.si_step(a, ob, gb, STEP, EPS, nrm=nb, nrm_out=a_no, cf=cf)
        check_against_alone(s_n, a, b, L, cf, "si_step nrm: x")
        check_against_alone(so_n, a_no, b, L, cf, "si_step nrm: nrm_out")
        a, a_no = xb.clone(), torch.empty_like(xb)
        ops.si_step(a, ob, gb, STEP, EPS, idx=ib, nrm_out=a_no, cf=cf)
        check_against_alone(s_i, a, b, L, cf, "si_step idx: x")
        check_against_alone(so_i, a_no, b, L, cf, "si_step idx: nrm_out")


# ------------------------------------------------------------------------------------------------------
# 2. full lengths: the dense launch on all rows
# ------------------------------------------------------------------------------------------------------
@LAYOUTS
@pytest.mark.parametrize("N", [1023, 1024, 1025])
def test_full_lengths_equal_the_dense_launch(ops, dev, N, cf):
    P, ori, g, n = (lay(t, cf, dev) for t in step_inputs(3, N, 600 + N))
    lens = lens_of((N, N, N), dev)
    idx = ops.knn_raw(P, P, KNN, q_cf=cf, r_cf=cf)[1]
    assert torch.equal(ops.pca_normal(P, idx, cf=cf, lengths=lens), ops.pca_normal(P, idx, cf=cf))
    for mode in (dict(nrm=n), dict(idx=idx)):
        rn, dn = torch.empty_like(P), torch.empty_like(P)
        assert torch.equal(ops.si_frame(P, nrm_out=rn, cf=cf, lengths=lens, **mode), ops.si_frame(P, nrm_out=dn, cf=cf, **mode))
        assert torch.equal(rn, dn)
        r, d = P.clone(), P.clone()
        ops.si_step(r, ori, g, STEP, EPS, nrm_out=rn, cf=cf, lengths=lens, **mode)
        ops.si_step(d, ori, g, STEP, EPS, nrm_out=dn, cf=cf, **mode)
        assert torch.equal(r, d) and torch.equal(rn, dn) and torch.isfinite(r).all()


# ------------------------------------------------------------------------------------------------------
# 3. the LDS stage boundary: decided by the capacity, not by the lengths
# ------------------------------------------------------------------------------------------------------
def test_lds_stage_boundary(ops, dev):
    lengths = (5200, 5121, 5120, 20)
    t = Batch(ops, dev, lengths, 5200, 700, True)
    x, nout = t.x.clone(), torch.empty_like(t.x)
    ops.si_step(x, t.ori, t.g, STEP, EPS, idx=t.idx, nrm_out=nout, lengths=t.lens)          # 5200 > 5120: through nrm_out
    for b, L in enumerate(lengths):
        xb, ob, gb, _, ib = t.alone[b]
        a, a_no = xb.clone(), torch.empty_like(xb)
        ops.si_step(a, ob, gb, STEP, EPS, idx=ib, nrm_out=a_no)
        if L <= 5120:                                                      # alone it is staged in LDS: nrm_out is optional
            a2 = xb.clone()
            ops.si_step(a2, ob, gb, STEP, EPS, idx=ib)
            assert torch.equal(a2, a)
        check_against_alone(x, a, b, L, True, "si_step idx beyond the LDS stage: x")
        check_against_alone(nout, a_no, b, L, True, "si_step idx beyond the LDS stage: nrm_out")
    _lib = M("3dpointcloudattack_amd._lib")
    for kw in (dict(lengths=t.lens), dict()):                              # without nrm_out: refused, as the dense entry does
        with pytest.raises(_lib.Pc3dError, match="needs nrm_out"):
            ops.si_step(t.x.clone(), t.ori, t.g, STEP, EPS, idx=t.idx, **kw)


# ------------------------------------------------------------------------------------------------------
# 4. float64
# ------------------------------------------------------------------------------------------------------
@LAYOUTS
def test_ragged_si_step_vs_float64_restatement(ops, dev, cf):
    """Per cloud, the existing test's own rule: 16x the fp32-vs-float64 deviation of the restatement on that cloud's first L
    rows, floor 2^-24. No point is left out."""
    t = Batch(ops, dev, LENGTHS, KMAX, 800, cf)
    x = t.x.clone()
    ops.si_step(x, t.ori, t.g, STEP, EPS, nrm=t.nrm, cf=cf, lengths=t.lens)
    out = unlay(x, cf)
    assert torch.isfinite(out).all()
    for b, L in enumerate(LENGTHS):
        P, ori, g, n = (h[b:b + 1, :L] for h in t.host)
        ref64 = R.si_step(P.double(), ori.double(), g.double(), n.double(), STEP, EPS)
        bound = bound_of(R.si_step(P, ori, g, n, STEP, EPS), ref64)
        dev_k = float((out[b:b + 1, :L].double() - ref64).abs().max())
        print(f"cloud {b} L={L}: kernel deviates {dev_k:.3e}, bound {bound:.3e}")
        assert dev_k <= bound


# ------------------------------------------------------------------------------------------------------
# 5. a bad index stays in its cloud
# ------------------------------------------------------------------------------------------------------
def test_index_beyond_the_length_stays_in_its_cloud(ops, dev):
    """An index >= L but < Kmax is out of range for its cloud: the range check is against L. The padding rows hold finite
    values here, so the NaN can only come from the check."""
    lengths = (65, 40, 64)
    t = Batch(ops, dev, lengths, 65, 9, True, nan=False)
    good = t.x.clone()
    ops.si_step(good, t.ori, t.g, STEP, EPS, idx=t.idx, lengths=t.lens)
    bad = t.idx.clone()
    bad[1, 7, 3] = 50
    x = t.x.clone()
    ops.si_step(x, t.ori, t.g, STEP, EPS, idx=bad, lengths=t.lens)
    n_bad = ops.pca_normal(t.x, bad, cf=True, lengths=t.lens)
    n_good = ops.pca_normal(t.x, t.idx, cf=True, lengths=t.lens)
    e_bad, e_good = ops.si_frame(t.x, idx=bad, lengths=t.lens), ops.si_frame(t.x, idx=t.idx, lengths=t.lens)
    torch.cuda.synchronize()
    assert torch.isfinite(good).all()
    assert bool(torch.isnan(x[1]).all())                                 # the cloud's norm carries the NaN to all its points
    assert torch.equal(x[0], good[0]) and torch.equal(x[2], good[2])     # ... and to no other cloud
    hit = torch.zeros((3, 65), dtype=torch.bool, device=dev)
    hit[1, 7] = True
    for o_bad, o_good in ((n_bad, n_good), (e_bad, e_good)):             # per point: that point alone
        assert bool(torch.isnan(o_bad.transpose(1, 2)[hit]).all())
        assert torch.equal(o_bad.transpose(1, 2)[~hit], o_good.transpose(1, 2)[~hit])
    # the same index is in range for the dense launch of the full batch
    d = t.x.clone()
    ops.si_step(d, t.ori, t.g, STEP, EPS, idx=bad)
    assert torch.isfinite(d).all()


# ------------------------------------------------------------------------------------------------------
# 6. - 10. the attack
# ------------------------------------------------------------------------------------------------------
A_LENGTHS = (1100, 1025, 1024, 65, 20)
STEPS = 5
_alone = {}


@pytest.fixture(scope="module")
def surrogates(nets, dev):
    from oracle import ref_torch as ort
    ft = M("3dpointcloudattack_amd.model.pointnet").PointNetCls(k=40, feature_transform=True)
    ft.load_state_dict(ort.seeded_state_dict(ft, 3))
    return {"plain": nets[0], "ft": ft.eval().to(dev)}


def ragged_points(lengths, kmax, seed, C, dev):
    """points [B,kmax,C] on the device, rows at and beyond a length NaN; C = 6 carries the ellipsoid's normals."""
    P, n = ellipsoid(len(lengths), kmax, seed)
    pts = torch.cat([P, n], -1) if C == 6 else P
    return nan_behind(pts, lengths).to(dev)


def labels_alone(wb, points, lengths):
    """The surrogate's clean prediction of every cloud alone: the label the untargeted loss starts from."""
    with torch.no_grad():
        return torch.cat([wb(points[b:b + 1, :L, :3].transpose(1, 2).contiguous())[0].argmax(1) for b, L in enumerate(lengths)])


def alone_runs(fx, nets, wb, points, target, lengths, steps, key=None):
    """[(adv [L,3], adv_target, count)] of an eager dense attack on every cloud alone; computed once per key."""
    if key is not None and key in _alone:
        return _alone[key]
    atk = make_attack(fx, "s5", nets, wb=wb, max_steps=steps, graph=False)
    out = []
    for b, L in enumerate(lengths):
        adv, lab, count = atk.shape_invariant_ifgm(points[b:b + 1, :L], target[b:b + 1])
        out.append((adv[0].clone(), int(lab), count))
    if key is not None:
        _alone[key] = out
    return out


def check_attack(x, ref, lengths):
    """x [B,3,Kmax] against the clouds alone: the columns below a length in every bit, the others equal to column 0."""
    assert torch.isfinite(x).all()
    for b, L in enumerate(lengths):
        assert torch.equal(x[b, :, :L], ref[b][0].t()), (b, L)
        assert torch.equal(x[b, :, L:], x[b, :, :1].expand(3, x.shape[2] - L)), (b, L)


@pytest.mark.parametrize("C", [6, 3])
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("victim", ["plain", "ft"])
def test_attack_equals_the_attacks_alone(fx, nets, surrogates, dev, victim, graph, C):
    _bitwise_only()
    wb = surrogates[victim]
    points = ragged_points(A_LENGTHS, KMAX, 900, C, dev)
    target = labels_alone(wb, points, A_LENGTHS)
    ref = alone_runs(fx, nets, wb, points, target, A_LENGTHS, STEPS, key=(victim, C))
    atk = make_attack(fx, "s5", nets, wb=wb, max_steps=STEPS, graph=graph)
    assert atk._fast()
    x = atk.iterate(points, target, lengths=A_LENGTHS)
    assert x.shape == (len(A_LENGTHS), 3, KMAX)
    check_attack(x, ref, A_LENGTHS)
    adv, adv_target, count = atk.run(points, target, lengths=np.array(A_LENGTHS))
    assert adv.shape == (len(A_LENGTHS), KMAX, 3) and torch.equal(adv, x.transpose(1, 2))
    assert adv_target.tolist() == [r[1] for r in ref]
    assert count == sum(r[2] for r in ref)
    cloud_io = M("3dpointcloudattack_amd.dataset.cloud_io")
    for b, c in enumerate(cloud_io.unstack_ragged(adv, A_LENGTHS)):
        assert torch.equal(c, ref[b][0])
    if graph:
        assert len(atk._loops) == 1 and next(iter(atk._loops.values())).graphs is not None


def test_one_captured_loop_serves_other_lengths(fx, nets, dev):
    _bitwise_only()
    first, second, kmax, steps = (1100, 1025, 700), (600, 64, 20), 1100, 3
    wb = nets[0]
    points = ellipsoid(3, kmax, 910)[0].to(dev)                          # [B,Kmax,3]: every step searches
    atk = make_attack(fx, "s5", nets, max_steps=steps)
    for lengths in (first, second):        # the shorter lengths second: the hint buffer then holds indices beyond them
        pts = nan_behind(points, lengths)
        target = labels_alone(wb, pts, lengths)
        check_attack(atk.iterate(pts, target, lengths=torch.tensor(lengths)), alone_runs(fx, nets, wb, pts, target, lengths, steps),
                     lengths)
        assert len(atk._loops) == 1
    (loop,) = atk._loops.values()
    assert loop.ragged and loop.graphs is not None and loop.lens.tolist() == list(second)
    target = labels_alone(wb, points, (kmax,) * 3)
    dense = atk.iterate(points, target)
    assert len(atk._loops) == 2 and [c.ragged for c in atk._loops.values()] == [True, False]
    assert torch.equal(dense, make_attack(fx, "s5", nets, max_steps=steps, graph=False).iterate(points, target))


def test_reference_clouds_inside_a_ragged_batch(fx, nets, dev):
    """The fixture's four clouds (L = 256), which the existing tests hold to the reference's bands, ride with a fifth of
    L = 300 = Kmax: their rows equal the dense 4-cloud run in every bit."""
    _bitwise_only()
    points, target = torch.from_numpy(fx["points"]).to(dev), torch.from_numpy(fx["target"]).to(dev)
    dense = make_attack(fx, "s5", nets).iterate(points, target)
    P5, n5 = ellipsoid(1, 300, 920)
    batch = torch.full((5, 300, 6), float("nan"), device=dev)
    batch[:4, :256] = points
    batch[4] = torch.cat([P5, n5], -1)[0].to(dev)
    lengths = [256, 256, 256, 256, 300]
    x = make_attack(fx, "s5", nets).iterate(batch, torch.cat([target, target[:1]]), lengths=lengths)
    assert torch.isfinite(x).all()
    assert torch.equal(x[:4, :, :256], dense)
    assert torch.equal(x[:4, :, 256:], x[:4, :, :1].expand(4, 3, 44))


def record_step(monkeypatch, atk, x, target, lens):
    """The entry names of one step of the loop (every launch goes through _lib.call), after one unrecorded step that builds
    the folded-weight caches."""
    _lib = M("3dpointcloudattack_amd._lib")
    names, real = [], _lib.call

    def counted(name, *a):
        names.append(name)
        return real(name, *a)
    c = atk._loop(x, x, target, None, lens)
    c.step()
    with monkeypatch.context() as mp:
        mp.setattr(_lib, "call", counted)
        c.step()
    return names


@pytest.mark.parametrize("victim", ["plain", "ft"])
def test_ragged_step_is_the_dense_step_launch_for_launch(fx, nets, surrogates, dev, monkeypatch, victim):
    lengths = np.array([600, 300, 20])
    x = ellipsoid(3, 600, 930)[0].to(dev).transpose(1, 2).contiguous()
    target = torch.tensor([1, 2, 3], device=dev)
    atk = make_attack(fx, "s5", nets, wb=surrogates[victim], graph=False)
    dense = record_step(monkeypatch, atk, x, target, None)
    ragged = record_step(monkeypatch, atk, x, target, lengths)
    print(f"{victim}: {len(dense)} launches a step\n  dense  {dense}\n  ragged {ragged}")
    assert not [n for n in dense if "_ragged" in n]                      # lengths=None: today's entries
    swap = {dense[0]: "pc3d_knn_ragged_f32", "pc3d_si_frame_f32": "pc3d_si_frame_ragged_f32",
            "pc3d_si_step_f32": "pc3d_si_step_ragged_f32"}
    assert dense[0].startswith("pc3d_knn") and dense[-1] == "pc3d_si_step_f32" and dense.count(dense[0]) == 1
    if victim == "plain":                                                # the two-tower victim's towers skip the padding
        swap.update({"pc3d_pointmlp3_max_fwd_f32": "pc3d_pointmlp3_max_fwd_ragged_f32",
                     "pc3d_pointmlp3_max_bwd_f32": "pc3d_pointmlp3_max_bwd_ragged_f32"})
        assert "pc3d_pointmlp3_max_fwd_f32" in dense and "pc3d_pointmlp3_max_bwd_f32" in dense
    assert ragged == [swap.get(n, n) for n in dense]
    assert len([n for n in ragged if "_ragged" in n]) == len([n for n in dense if n in swap]) >= 3


def test_gates_on_the_gpu_call_no_entry(fx, nets, dev, monkeypatch):
    _lib = M("3dpointcloudattack_amd._lib")
    D = M("3dpointcloudattack_amd.defense")
    lengths = (64, 40, 20)
    points = ragged_points(lengths, 64, 940, 6, dev)
    target = torch.tensor([1, 2, 3], device=dev)
    cases = [make_attack(fx, "s5", nets, wb=D.FusedDefended(nets[0], D.SORDefense(k=2, alpha=1.1, npoint=64))),
             make_attack(fx, "s5", nets, defense_method="sor"),
             make_attack(fx, "s5_top5", nets),
             make_attack(fx, "s5", nets, fused=False)]
    for method in ("simba", "simbapp", "ours"):
        q = make_attack(fx, "s5", nets)
        q.attack_method = method
        cases.append(q)
    assert cases[2].top5_attack
    names, real = [], _lib.call

    def counted(name, *a):
        names.append(name)
        return real(name, *a)
    monkeypatch.setattr(_lib, "call", counted)
    for atk in cases:
        for call in (atk.run, atk.shape_invariant_ifgm, atk.iterate):
            with pytest.raises(ValueError, match="shape_invariant_ifgm"):
                call(points, target, lengths=lengths)
    with pytest.raises(ValueError, match="lengths must"):
        make_attack(fx, "s5", nets).run(points, target, lengths=(64, 40, 19))
    assert names == []
