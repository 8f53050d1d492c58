"""GPU: ops.knn_attack_update (pc3d_knn_attack_update_f32) against tests/knn_step_restatement.py in float64.

The kernel is fed the product's own search results (ops.knn_search_into / ops.nn_raw) and the restatement gathers on the
same indices, so ties cannot matter. Tolerance per output: cw_step_restatement.bands — 16 x the fp32-vs-float64 deviation
of the restatement on the same input, floor 16 x 2^-24 x max|ref|. tests/test_knn_step_cpu.py shows that every point's
outlier decision is farther than 1e-4 x thr from its threshold on these inputs: nothing is excluded here.
"""
import numpy as np
import pytest
import torch

import knn_step_restatement as rs

pytestmark = pytest.mark.gpu


def _scales(ops, N, k, B, w2):
    up = np.float32(N)                                                  # the reference's `* K`
    if w2 is None:
        return ops.knn_attack_scales(N, 0, B, up, None)
    return ops.knn_attack_scales(N, k, B, up * np.float32(rs.W1), up * np.float32(w2))


def _search(ops, dev, inp, k):
    adv, ori = inp["adv"].to(dev), inp["ori"].to(dev)
    B, _, N = adv.shape
    knn_d = torch.zeros((B, N, k + 1), dtype=torch.float32, device=dev)
    knn_idx = torch.zeros((B, N, k + 1), dtype=torch.int32, device=dev)
    ops.knn_search_into(adv, knn_d, knn_idx)
    _, nn_idx = ops.nn_raw(adv, ori, True, True)
    return knn_d, knn_idx, nn_idx


def _product(ops, dev, inp, k, found, w2=rs.W2, project=True, t=rs.T, device_word=True, scales=None, alpha=rs.ALPHA, **over):
    """One launch on a copy of the case; returns the tensors it writes, on the CPU."""
    a = {n: (over[n] if n in over else inp[n]) for n in ("adv", "ori", "normal", "g", "m", "v")}
    a = {n: (None if x is None else x.to(dev).clone()) for n, x in a.items()}
    B, _, N = a["adv"].shape
    knn_d, knn_idx, nn_idx = found
    c_ch, c_knn = scales if scales is not None else _scales(ops, N, k, B, w2)
    step = torch.tensor([t], dtype=torch.int32, device=dev) if device_word else t
    ops.knn_attack_update(a["adv"], a["ori"], a["g"], a["m"], a["v"], step, rs.LR, knn_d, knn_idx, nn_idx, c_ch, c_knn,
                          alpha, rs.BUDGET, "project_clip" if project else "clip", a["normal"])
    return {n: a[n].cpu() for n in rs.FLOAT_OUT}


def _check(got, inp, k, found, **kw):
    idx = dict(knn_idx=found[1].cpu(), nn_idx=found[2].cpu())
    ref64 = rs.run(torch.float64, inp, k=k, **idx, **kw)
    band = rs.bands(ref64, rs.run(torch.float32, inp, k=k, **idx, **kw), names=rs.FLOAT_OUT)
    for name in rs.FLOAT_OUT:
        dev_ = float((got[name].double() - ref64[name]).abs().max())
        print(f"{name}: deviation {dev_:.3g}, band {band[name]:.3g}")
        assert dev_ <= band[name], name


@pytest.mark.parametrize("case", rs.CASES)
def test_update_vs_float64_restatement(ops, dev, case):
    N, B, k, wn = case
    inp = rs.inputs(*case)
    found = _search(ops, dev, inp, k)
    _check(_product(ops, dev, inp, k, found), inp, k, found)


@pytest.mark.parametrize("case", rs.HEAVY)
def test_update_with_many_masked_points(ops, dev, case):
    """alpha = 0: about a fifth of the points are masked and the edges fill several staging trips."""
    N, B, k, wn = case
    inp = rs.inputs(*case, rs.HEAVY_ALPHA)
    found = _search(ops, dev, inp, k)
    _check(_product(ops, dev, inp, k, found, alpha=rs.HEAVY_ALPHA), inp, k, found, alpha=rs.HEAVY_ALPHA)


@pytest.mark.parametrize("device_word", [True, False])
@pytest.mark.parametrize("t", [1, 5])
def test_step_word(ops, dev, t, device_word):
    case = (200, 3, 5, True)
    inp = rs.inputs(*case)
    found = _search(ops, dev, inp, 5)
    _check(_product(ops, dev, inp, 5, found, t=t, device_word=device_word), inp, 5, found, t=t)


@pytest.mark.parametrize("case", [(200, 3, 5, True), (1031, 1, 1, False)])
def test_clip_only_and_no_knn_term(ops, dev, case):
    N, B, k, wn = case
    inp = rs.inputs(*case)
    found = _search(ops, dev, inp, k)
    _check(_product(ops, dev, inp, k, found, project=False), inp, k, found, project=False)
    plain = _product(ops, dev, inp, k, found, w2=None)                                   # c_knn = 0: plain ChamferDist
    _check(plain, inp, k, found, w2=None)
    bare = _product(ops, dev, inp, k, (None, None, found[2]), w2=None)                   # ... and without a kNN result at all
    assert all(torch.equal(plain[name], bare[name]) for name in rs.FLOAT_OUT)


@pytest.mark.parametrize("k", [1, 3])
def test_lattice_has_zero_knn_gradient(ops, dev, k):
    """All value_i equal: the strict mask is empty, so the kNN term must not change a bit of the update."""
    inp, _ = rs.lattice_case()
    found = _search(ops, dev, inp, k)
    N, B = inp["adv"].shape[2], inp["adv"].shape[0]
    with_knn = _product(ops, dev, inp, k, found)
    c_ch, _ = _scales(ops, N, k, B, rs.W2)
    without = _product(ops, dev, inp, k, found, scales=(c_ch, 0.0))
    for name in rs.FLOAT_OUT:
        assert torch.equal(with_knn[name], without[name]), name


def test_planted_far_points_are_masked(ops, dev):
    """The kNN term reaches exactly the masked points and their neighbours: the planted far points among them."""
    case = (200, 3, 5, True)
    N, B, k, _ = case
    inp = rs.inputs(*case)
    found = _search(ops, dev, inp, k)
    c_ch, _ = _scales(ops, N, k, B, rs.W2)
    with_knn = _product(ops, dev, inp, k, found)
    without = _product(ops, dev, inp, k, found, scales=(c_ch, 0.0))
    mask = rs.mask_margin(inp["adv"], k, rs.ALPHA)[2]
    assert mask[:, :rs.N_PLANT].all()
    touched = mask.clone()
    nb = found[1].cpu().long()[:, :, 1:]
    for b in range(B):
        touched[b, nb[b][mask[b]].reshape(-1)] = True
    differs = (with_knn["m"] != without["m"]).any(1)
    assert torch.equal(differs, touched)


def test_chamfer_term_uses_the_given_index(ops, dev):
    case = (200, 3, 5, True)
    inp = rs.inputs(*case)
    knn_d, knn_idx, nn_idx = _search(ops, dev, inp, 5)
    perm = torch.stack([torch.randperm(200, generator=torch.Generator().manual_seed(b)) for b in range(3)]).to(dev)
    permuted = (knn_d, knn_idx, torch.gather(nn_idx, 1, perm).contiguous())
    got = _product(ops, dev, inp, 5, permuted)
    _check(got, inp, 5, permuted)
    assert not torch.equal(got["m"], _product(ops, dev, inp, 5, (knn_d, knn_idx, nn_idx))["m"])


def test_bitwise_properties(ops, dev):
    """Run == run; a sample inside a batch == the sample alone; a NaN sample leaves its neighbours' bits alone."""
    case = (1031, 3, 5, True)
    N, B, k, _ = case
    inp = rs.inputs(*case)
    found = _search(ops, dev, inp, k)
    scales = _scales(ops, N, k, B, rs.W2)
    base = _product(ops, dev, inp, k, found, scales=scales)
    again = _product(ops, dev, inp, k, found, scales=scales)
    for name in rs.FLOAT_OUT:
        assert torch.equal(base[name], again[name]), name
    for b in range(B):
        one = {n: (None if x is None else x[b:b + 1].contiguous()) for n, x in inp.items()}
        alone = _product(ops, dev, one, k, tuple(f[b:b + 1].contiguous() for f in found), scales=scales)
        for name in rs.FLOAT_OUT:
            assert torch.equal(alone[name][0], base[name][b]), (name, b)
    bad = inp["adv"].clone()
    bad[1] = float("nan")
    nan = _product(ops, dev, inp, k, found, scales=scales, adv=bad)
    for name in rs.FLOAT_OUT:
        assert torch.equal(nan[name][0], base[name][0]) and torch.equal(nan[name][2], base[name][2]), name
    assert torch.isnan(nan["adv"][1]).all()


def test_refusals(ops, dev, pc3d):
    inp = rs.inputs(64, 3, 5, True)
    found = _search(ops, dev, inp, 5)
    a = {n: inp[n].to(dev).clone() for n in ("adv", "ori", "g", "m", "v")}
    strided = torch.zeros((3, 64, 3), device=dev).transpose(1, 2)          # adv's shape, other strides
    with pytest.raises(ValueError, match="strides"):
        ops.knn_attack_update(a["adv"], a["ori"], a["g"], strided, a["v"], 1, rs.LR, *found)
    with pytest.raises(Exception, match="GPU only"):
        ops.knn_attack_update(inp["adv"].clone(), inp["ori"], inp["g"], inp["m"].clone(), inp["v"].clone(), 1, rs.LR)
    with pytest.raises(TypeError):
        ops.knn_attack_update(a["adv"].double(), a["ori"], a["g"], a["m"].double(), a["v"].double(), 1, rs.LR, *found)
    # N above the cap: the library's error code, before any launch
    n = ops.KNN_LOOP_MAX_POINTS + 1
    big = torch.zeros((1, 3, n), device=dev)
    lib = pc3d.load()
    p = big.data_ptr()
    rc = lib.pc3d_knn_attack_update_f32(p, 3 * n, 1, n, p, 3 * n, 1, n, None, 0, 0, 0, p, 3 * n, 1, n, p, p, 1, n, 0, None, None,
                                        None, 0.01, 0.9, 0.999, 1e-8, 0.18, 0, 1.05, 0.0, 0.0, None, 1, None)
    assert rc == -22 and b"N <=" in lib.pc3d_last_error()
    with pytest.raises(Exception, match="rc=-22"):
        ops.knn_attack_update(big, big.clone(), big.clone(), big.clone(), big.clone(), 1, rs.LR)
