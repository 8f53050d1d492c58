"""CPU: tests/knn_step_restatement.py IS the reference's algorithm, and the band of tests/test_knn_step_gpu.py has teeth.

* Trajectory: oracle.ref_torch.knn_attack on a toy victim in fp32, with ChamferkNNDist and with ChamferDist, with
  ProjectInnerClipLinf and with ClipPointsLinf, the three adversarial functors, 3- and 6-channel input; the restatement
  iterated in fp32 from the oracle's own start point reproduces every iterate its `record` hook sees, and the returned
  cloud, bit for bit.
* The two spellings of the neighbour terms agree in float64.
* The step cases are not tame, and no point's outlier decision sits near its threshold.
* Teeth: each mistake the GPU file exists to catch, made on the float64 restatement, leaves the band the GPU file
  computes for the same inputs on at least one output.
"""
import numpy as np
import pytest
import torch

import knn_step_restatement as rs
from oracle import ref_torch as ort


class _Toy:
    """log_softmax of a fixed random linear map of the flattened cloud to 5 classes, as a tuple like the oracle's victims:
    the iterate enters it once, so the gradient at the leaf is g_model + g_dist whatever order autograd sums in."""

    def __init__(self, K, seed):
        self.W = torch.randn(5, 3 * K, generator=torch.Generator().manual_seed(seed))

    def __call__(self, x):
        return (torch.log_softmax(x.reshape(x.shape[0], -1) @ self.W.t(), dim=1),)


ADV = {"untargeted": lambda: ort.UntargetedLogitsAdvLoss(0.5), "logits": lambda: ort.LogitsAdvLoss(0.5),
       "cross_entropy": lambda: ort.CrossEntropyAdvLoss()}


@pytest.mark.parametrize("channels", [3, 6])
@pytest.mark.parametrize("adv_name", sorted(ADV))
@pytest.mark.parametrize("project", [True, False])
@pytest.mark.parametrize("knn_term", [True, False])
def test_restatement_reproduces_the_oracle_loop_bit_for_bit(knn_term, project, adv_name, channels):
    B, K, iters, lr, budget = 3, 48, 6, 0.02, 0.03
    gen = torch.Generator().manual_seed(17 + channels + 2 * int(knn_term))
    data = torch.rand(B, K, 3, generator=gen) - 0.5
    if channels == 6:
        n = torch.randn(B, K, 3, generator=gen)
        data = torch.cat([data, n / n.norm(dim=2, keepdim=True)], dim=2)
    model = _Toy(K, 3)
    target = torch.randint(0, 5, (B,), generator=gen)
    adv_func = ADV[adv_name]()
    dist_func = ort.ChamferkNNDist() if knn_term else ort.ChamferDist()
    clip_func = ort.ProjectInnerClipLinf(budget) if project else (lambda pc, ori, normal: ort.ClipPointsLinf(budget)(pc, ori))
    seen = []
    torch.manual_seed(5)
    out, _ = ort.knn_attack(model, data, target, adv_func, dist_func, clip_func, attack_lr=lr, num_iter=iters,
                            attack_method="untarget" if adv_name == "untargeted" else "target",
                            record=lambda it, a: seen.append(torch.from_numpy(a)))
    assert len(seen) == iters
    seen.append(torch.from_numpy(out).transpose(1, 2).contiguous())

    cf = data.float().transpose(1, 2).contiguous()
    ori, normal = cf[:, :3].contiguous(), (cf[:, 3:].contiguous() if channels == 6 else None)
    adv = seen[0].clone()                                            # the oracle's own start point
    m, v = torch.zeros_like(adv), torch.zeros_like(adv)
    clipped = projected = 0
    for it in range(iters):
        x = adv.clone().requires_grad_()
        adv_func(model(x)[0], target).mean().backward()
        r = rs.step(torch.float32, adv, ori, normal, x.grad, m, v, it + 1, lr=lr, budget=budget,
                    w2=rs.W2 if knn_term else None, project=project)
        assert torch.equal(r["adv"], seen[it + 1]), it
        d = r["stepped"] - ori
        clipped += int((d.norm(dim=1) > budget).sum())
        projected += int((torch.sum(d * (ori if normal is None else normal), dim=1) < 0).sum())
        adv, m, v = r["adv"], r["m"], r["v"]
    # the run exercised the clip and both sides of the projection's first test, and moved
    assert clipped > 0 and 0 < projected < B * K * iters
    assert not torch.equal(adv, seen[0])


@pytest.mark.parametrize("case", [(64, 3, 5, True), (200, 3, 5, True), (200, 1, 1, False)])
def test_spellings_agree_in_float64(case):
    N, B, k, wn = case
    inp = rs.inputs(*case)
    knn_idx, nn_idx = rs.neighbours_f64(*case)
    for w2 in (rs.W2, None):
        a = rs.run(torch.float64, inp, k=k, w2=w2)
        b = rs.run(torch.float64, inp, k=k, w2=w2, knn_idx=knn_idx, nn_idx=nn_idx)
        for name in rs.FLOAT_OUT:
            assert float((a[name] - b[name]).abs().max()) <= 1e-10, (name, w2)


@pytest.mark.parametrize("case", rs.CASES + [c + (rs.HEAVY_ALPHA,) for c in rs.HEAVY])
def test_inputs_are_not_tame(case):
    """Masked and unmasked points, points the projection moves, an "opposite" point, points the clip shortens and points
    it leaves — and every point's |value - thr| exceeds MARGIN x thr in float64, so the fp32 mask cannot legitimately differ."""
    N, B, k, wn = case[:4]
    alpha = case[4] if len(case) > 4 else rs.ALPHA
    inp = rs.inputs(*case)
    knn_idx, nn_idx = rs.neighbours_f64(*case)
    value, thr, mask, rel = rs.mask_margin(inp["adv"], k, alpha)
    assert float(rel.min()) > rs.MARGIN
    assert 0 < int(mask.sum()) < mask.numel()
    assert mask[:, :(rs.N_PLANT if N >= 16 else 1)].all()                # the planted far points are masked
    if len(case) > 4:
        assert int(mask.sum(1).min()) * k > 2048                         # more edges than one staging trip of the kernel
    a = rs.run(torch.float64, inp, k=k, alpha=alpha, knn_idx=knn_idx, nn_idx=nn_idx)
    b = rs.run(torch.float32, inp, k=k, alpha=alpha, knn_idx=knn_idx, nn_idx=nn_idx)
    ori = inp["ori"].double()
    nrm = ori if inp["normal"] is None else inp["normal"].double()
    d = a["stepped"] - ori
    inner = torch.sum(d * nrm, dim=1)
    cross = torch.cross(nrm, d, dim=1).norm(dim=1)
    # the projection's branches are decided beyond rounding (same decisions in fp32), and all three occur
    assert float((inner.abs() / (d.norm(dim=1) * nrm.norm(dim=1))).min()) > 1e-6
    assert not ((cross >= 0.5e-6) & (cross <= 2e-6)).any()
    d32 = b["stepped"].double() - ori
    assert torch.equal(torch.sum(d32 * nrm, dim=1) < 0, inner < 0)
    opposite = (inner < 0) & (cross < 1e-6)
    assert int(opposite.sum()) >= B and 0 < int((inner < 0).sum()) < inner.numel()
    assert float((a["adv"] - ori)[:, :, N - 1].abs().max()) == 0.       # the opposite point is put back onto ori
    moved = (inner < 0) & ~opposite
    assert float((a["adv"] - a["stepped"]).abs().amax(1)[moved].min()) > 0.
    # the clip shortens some points and leaves others
    after = (a["adv"] - ori).norm(dim=1)
    assert int((after > rs.BUDGET * (1 - 1e-6)).sum()) > 0 and int((after < 0.99 * rs.BUDGET).sum()) > 0


# ----------------------------------------------------------------------------------------------------------------------
# teeth
# ----------------------------------------------------------------------------------------------------------------------
def _separation(base, mutated, band):
    worst = 0.
    for name, bd in band.items():
        d = (mutated[name].double() - base[name].double()).abs()
        d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
        worst = max(worst, float(d.max()) / bd)
    return worst


def _teeth_case(name):
    if name == "ge_mask":
        inp, k = rs.lattice_case()
    elif name == "biased_std":
        # many small clouds: the two thresholds lie 7 % of alpha x std apart at N = 8, and some cloud has a point in between
        inp, k = rs.inputs(8, B=256, k=3), 3
    else:
        inp, k = rs.inputs(200, 3, 5, True), 5
    return inp, k, rs.knn_f64(inp["adv"], k)[1], rs.nn_f64(inp["adv"], inp["ori"])


@pytest.mark.parametrize("name", rs.MUTATIONS)
def test_band_separates_mutation(name):
    inp, k, knn_idx, nn_idx = _teeth_case(name)
    kw = dict(k=k, knn_idx=knn_idx, nn_idx=nn_idx)
    base = rs.run(torch.float64, inp, **kw)
    band = rs.bands(base, rs.run(torch.float32, inp, **kw), names=rs.FLOAT_OUT)
    sep = _separation(base, rs.run(torch.float64, inp, mut=name, **kw), band)
    print(f"{name}: separation {sep:.3g} x band")
    assert sep > 1


def test_lattice_has_no_outliers_in_either_precision():
    inp, k = rs.lattice_case()
    for dtype in (torch.float32, torch.float64):
        d = rs.knn_f64(inp["adv"], k)[0].to(dtype)
        mask, thr = rs.knn_mask(d[:, :, 1:].mean(-1), rs.ALPHA)
        assert not mask.any() and np.allclose(thr.numpy(), 1. / 256, rtol=0, atol=0)
