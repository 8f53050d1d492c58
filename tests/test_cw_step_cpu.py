"""CPU: tests/cw_step_restatement.py IS the reference's algorithm, and the band of tests/test_cw_step_gpu.py has teeth.

* Trajectory: oracle.ref_torch.cw_attack on a toy victim, one binary step of 6 iterations in fp32, with L2Dist and with
  ChannelFirst(ChamferDist()); the restatement iterated in fp32 from the same start reproduces the iterate, the bests
  and the best attack of every iteration bit for bit. What the oracle's loop does not return (bestdist, o_bestscore, the
  state of every iteration) is read from its own local variables at the one call it makes right after the bookkeeping,
  the adversarial loss.
* The two spellings of the Chamfer term agree in float64 to 1e-12.
* Teeth: each mistake the GPU file exists to catch, made on the float64 restatement, moves at least one output by more
  than 100 x the band the GPU file computes for the same inputs.
"""
import operator
import sys

import numpy as np
import pytest
import torch

import cw_step_restatement as rs
from oracle import ref_torch as ort


# ----------------------------------------------------------------------------------------------------------------------
# the restatement against the oracle's loop
# ----------------------------------------------------------------------------------------------------------------------
class _Toy:
    """A fixed random linear map of the flattened cloud to 5 logits, returned as a tuple as the oracle expects."""

    def __init__(self, K, seed):
        self.W = torch.randn(5, 3 * K, generator=torch.Generator().manual_seed(seed))

    def __call__(self, x):
        return (x.reshape(x.shape[0], -1) @ self.W.t(),)


class _Spy:
    """The adversarial loss, called by the oracle right after its bookkeeping (:160): keeps a copy of the loop's state."""
    KEEP = ("bestdist", "bestscore", "o_bestdist", "o_bestscore", "o_bestattack", "dist_val", "pred_val", "input_val", "cur_w")

    def __init__(self, fn):
        self.fn, self.seen = fn, []

    def __call__(self, logits, target):
        loc = sys._getframe(1).f_locals
        self.seen.append({k: np.array(loc[k], copy=True) for k in self.KEEP})
        return self.fn(logits, target)


@pytest.mark.parametrize("dist_kind", [1, 2])
@pytest.mark.parametrize("untarget", [True, False])
def test_restatement_reproduces_the_oracle_loop_bit_for_bit(dist_kind, untarget):
    B, K, iters = 4, 64, 6
    gen = torch.Generator().manual_seed(11 + dist_kind)
    data = torch.rand(B, K, 3, generator=gen) - 0.5
    model = _Toy(K, 3)
    clean = model(data.transpose(1, 2).contiguous())[0]
    # untargeted: the true class for two samples, a wrong one for the others; targeted: the runner-up / the current class
    order = clean.argsort(1, descending=True)
    target = torch.where(torch.arange(B) % 2 == 0, order[:, 0], order[:, 1]) if untarget else \
        torch.where(torch.arange(B) % 2 == 0, order[:, 1], order[:, 0])
    adv_func = _Spy(ort.UntargetedLogitsAdvLoss(0.) if untarget else ort.LogitsAdvLoss(0.))
    dist_func = ort.L2Dist() if dist_kind == 1 else ort.ChannelFirst(ort.ChamferDist())
    new_adv = []

    def clip_func(pc, ori):
        out = ort.ClipPointsLinf(rs.BUDGET)(pc, ori)
        new_adv.append(out.clone())          # the loop goes on updating the returned tensor in place
        return out

    torch.manual_seed(5)
    o_bestdist, o_bestattack, _, _ = ort.cw_attack(model, data, target, adv_func, dist_func, clip_func, attack_lr=rs.LR,
                                                   binary_step=1, num_iter=iters,
                                                   attack_method="untarget" if untarget else "target")
    assert len(adv_func.seen) == len(new_adv) == iters

    ori = data.float().transpose(1, 2).contiguous()
    adv = torch.from_numpy(adv_func.seen[0]["input_val"].copy())            # the oracle's own start point
    st = dict(bestdist=torch.full((B,), 1e10), bestscore=torch.full((B,), -1), o_bestdist=torch.full((B,), 1e10),
              o_bestscore=torch.full((B,), -1), o_bestattack=torch.zeros(B, 3, K))
    m, v = torch.zeros_like(adv), torch.zeros_like(adv)
    flips = 0
    for it in range(iters):
        seen = adv_func.seen[it]
        x = adv.clone().requires_grad_()
        logits = model(x)[0]
        adv_func.fn(logits, target).mean().backward()
        pred = logits.argmax(1)
        assert np.array_equal(pred.numpy(), seen["pred_val"])
        r = rs.step(torch.float32, adv, ori, x.grad, m, v, it + 1, torch.from_numpy(seen["cur_w"]), pred, target, untarget,
                    st["bestdist"], st["bestscore"], st["o_bestdist"], st["o_bestscore"], st["o_bestattack"], dist_kind, None,
                    rs.LR, rs.BUDGET, spelling="min")
        assert np.array_equal(r["input_val"].numpy(), seen["input_val"])
        assert np.array_equal(r["dist_val"].numpy(), seen["dist_val"])
        for k in st:
            assert np.array_equal(r[k].numpy().astype(np.float64), seen[k].astype(np.float64)), (it, k)
        assert torch.equal(r["adv"], new_adv[it]), it
        flips += int(r["copied"].sum())
        adv, m, v = r["adv"], r["m"], r["v"]
        st = {k: r[k] for k in st}
    assert np.array_equal(st["o_bestdist"].numpy().astype(np.float64), o_bestdist)
    assert np.array_equal(st["o_bestattack"].numpy().transpose(0, 2, 1).astype(np.float64), o_bestattack)
    # the run exercised the decisions: some sample was copied, some sample never succeeded or stopped improving
    assert 0 < flips < B * iters
    assert not torch.equal(adv, ori)


@pytest.mark.parametrize("K", [64, 333, 1025])
def test_chamfer_spellings_agree_in_float64(K):
    inp = rs.inputs(K)
    nn = rs.nn_f64(inp["adv"], inp["ori"])
    a = rs.run(torch.float64, inp, True, 2, spelling="min")
    b = rs.run(torch.float64, inp, True, 2, nn_idx=nn)
    for k in rs.FLOAT_OUT:
        assert float((a[k] - b[k]).abs().max()) <= 1e-12, k
    for k in rs.INT_OUT:
        assert torch.equal(a[k], b[k])


@pytest.mark.parametrize("K", [1, 333, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193, 9000])
def test_inputs_are_not_tame(K):
    """Between 20 % and 80 % of the points lie past the budget before the clip; both restatements take the same decisions,
    and those are a mix."""
    inp = rs.inputs(K)
    assert 0.2 <= rs.clipped_share(inp) <= 0.8
    for untarget in (True, False):
        a = rs.run(torch.float64, inp, untarget, 1)
        b = rs.run(torch.float32, inp, untarget, 1)
        for k in rs.INT_OUT + ("copied",):
            assert torch.equal(a[k], b[k])
        assert 0 < int((a["bestscore"] != -1).sum()) < 3
    assert int(rs.run(torch.float64, inp, True, 1)["copied"].sum()) == 2


# ----------------------------------------------------------------------------------------------------------------------
# teeth
# ----------------------------------------------------------------------------------------------------------------------
K_TEETH = 2049


def _separation(base, mutated, band):
    """The largest |mutated - base| / band over the float outputs (NaN-safe: a NaN on one side only counts as inf)."""
    worst = 0.
    for k, bd in band.items():
        d = (mutated[k].double() - base[k].double()).abs()
        d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
        worst = max(worst, float(d.max()) / bd)
    return worst


def _case(dist_kind, far=False):
    inp = rs.inputs(K_TEETH, far=far)
    nn = rs.nn_f64(inp["adv"], inp["ori"]) if dist_kind == 2 else None
    base = rs.run(torch.float64, inp, True, dist_kind, nn_idx=nn)
    band = rs.bands(base, rs.run(torch.float32, inp, True, dist_kind, nn_idx=nn))
    return inp, nn, base, band


def _swap_1024(x):
    """Rows k and k - 1024 exchanged for k >= 1024 (what a wrong register tile would read)."""
    y = x.clone()
    n = x.shape[2] - 1024
    y[:, :, 1024:1024 + n], y[:, :, :n] = x[:, :, :n], x[:, :, 1024:1024 + n]
    return y


def _mut_gradient_rows(dist_kind):
    inp, nn, base, band = _case(dist_kind)
    g = inp["g"].double() + rs.dist_grad(torch.float64, inp["adv"], inp["ori"], inp["w"], dist_kind, nn)
    return base, rs.run(torch.float64, inp, True, 0, g=_swap_1024(g)), band


def _mut_moments(dist_kind):
    inp, nn, base, band = _case(dist_kind)
    return base, rs.run(torch.float64, inp, True, dist_kind, nn_idx=nn, m=_swap_1024(inp["m"]), v=_swap_1024(inp["v"])), band


def _mut_batch_mean(dist_kind):
    inp, nn, base, band = _case(dist_kind)
    return base, rs.run(torch.float64, inp, True, dist_kind, nn_idx=nn, w=inp["w"] * inp["w"].numel()), band


def _mut_chamfer_mean(dist_kind):
    inp, nn, base, band = _case(2)
    return base, rs.run(torch.float64, inp, True, 2, nn_idx=nn, w=inp["w"] * K_TEETH), band


def _mut_l2norm_neighbour(dist_kind):
    inp, nn, base, band = _case(1)
    adv, ori = inp["adv"].double(), inp["ori"].double()
    wrong = torch.roll(rs.dist_value(adv, ori), 1)
    g = inp["g"].double() + (inp["w"].double() / 3 / wrong)[:, None, None] * (adv - ori)
    return base, rs.run(torch.float64, inp, True, 0, g=g), band


def _mut_clip_eps(dist_kind):
    # the + 1e-9 changes the scale by 1e-9 absolute: on |adv - ori| ~ 0.1 that is 1e-10, below fp32 itself — the only input
    # on which ANY arithmetic can tell the two clips apart is a point so far out that its scale is of the order of 1e-9
    inp, nn, base, band = _case(dist_kind, far=True)
    mut = rs.run(torch.float64, inp, True, dist_kind, nn_idx=nn, budget=0.)
    ori = inp["ori"].double()
    diff = mut["adv"] - ori
    scale = torch.clamp(rs.BUDGET / torch.sum(diff ** 2, dim=1) ** 0.5 + 1e-9, max=1.)
    mut["adv"] = ori + diff * scale[:, None, :]
    return base, mut, band


def _mut_step_number(dist_kind):
    inp, nn, base, band = _case(dist_kind)
    return base, rs.run(torch.float64, inp, True, dist_kind, nn_idx=nn, t=rs.T + 1), band


MUTATIONS = {"gradient_rows_swapped": _mut_gradient_rows, "moments_swapped": _mut_moments, "batch_mean_dropped": _mut_batch_mean,
             "chamfer_mean_dropped": _mut_chamfer_mean, "l2norm_of_neighbour": _mut_l2norm_neighbour,
             "clip_eps_outside": _mut_clip_eps, "step_off_by_one": _mut_step_number}


@pytest.mark.parametrize("dist_kind", [1, 2])
@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_band_separates_mutation(name, dist_kind):
    if (name == "chamfer_mean_dropped" and dist_kind != 2) or (name == "l2norm_of_neighbour" and dist_kind != 1):
        dist_kind = 3 - dist_kind          # these two belong to one distance: the other parameter repeats it
    base, mut, band = MUTATIONS[name](dist_kind)
    sep = _separation(base, mut, band)
    print(f"{name} dist_kind={dist_kind}: separation {sep:.3g} x band")
    assert sep > 100


def test_far_point_leaves_the_adv_band_as_it_was():
    """The far point does not blow the band up: the adv band of the far case is that of the plain case."""
    for dist_kind in (0, 1):
        _, _, _, plain = _case(dist_kind)
        _, _, _, far = _case(dist_kind, far=True)
        assert far["adv"] <= 2 * plain["adv"]


@pytest.mark.parametrize("untarget", [True, False])
def test_tie_case_separates_le_from_lt(untarget):
    """On the tie case (o_bestdist == dist exactly) `<=` in the overall-best decision copies a sample that `<` leaves."""
    inp = rs.tie_inputs(333, untarget)
    base = rs.run(torch.float64, inp, untarget, 0)
    f32 = rs.run(torch.float32, inp, untarget, 0)
    mut = rs.run(torch.float64, inp, untarget, 0, overall_lt=operator.le)
    assert base["dist_val"].tolist() == [rs.TIE_DIST] * 5 and f32["dist_val"].tolist() == [rs.TIE_DIST] * 5
    assert base["copied"].tolist() == [True, True, False, False, False]
    assert (base["bestscore"] != -1).tolist() == [False, True, True, True, False]
    assert mut["copied"].tolist() == [True, True, True, False, False]
    assert int(mut["o_bestscore"][2]) == int(inp["pred"][2]) and int(base["o_bestscore"][2]) == -1
    band = rs.bands(base, f32)
    assert float((mut["o_bestattack"] - base["o_bestattack"]).abs().max()) > 100 * band["adv"]
