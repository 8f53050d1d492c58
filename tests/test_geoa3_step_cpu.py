"""CPU: tests/geoa3_step_restatement.py IS the reference's iteration, and the band of tests/test_geoa3_step_gpu.py has teeth.

* (a) In float64 its terms and gradient equal oracle.ref_torch.GeoA3Oracle(as_written=False, dtype=float64, keep_dtype=True,
  direct=True).forward_step, and its update a torch.optim.Adam step on that gradient.
* (b) On every case the two largest adv -> ori distances differ by more than 1e-4 relative and every |<v,n>| that enters a
  kappa exceeds 1e-6: no decision (Hausdorff arg-max, sign of an inner product) sits at rounding distance, so the
  fp32-vs-float64 band is not inflated by a flipped one.
* (c) The band on the gradient, 16 x (fp32 - float64), stays below 1e-3 x max|g|: it can fail.
* (d) The band on the constraint terms stays below 1e-4 relative.
"""
import types

import pytest
import torch

import geoa3_step_restatement as rs
from oracle import ref_torch as ort

CONFIGS = {"default": {}, "single_sided": dict(two_sided=False), "no_curv": dict(w_curv=0.),
           "margin_l2": dict(cls_loss_type="Margin", confidence=5., dis_loss_type="L2", w_hd=0., w_curv=0.),
           "targeted_ce": dict(targeted=True)}


def _oracle_step(case, over):
    c = dict(rs.DEFAULTS, **over)
    inp, nb = rs.inputs(*case), rs.neighbours_f64(*case)
    d = lambda t: t.double()      # noqa: E731
    orc = ort.GeoA3Oracle(as_written=False, dtype=torch.float64, keep_dtype=True, direct=True)
    cfg = types.SimpleNamespace(cls_loss_type=c["cls_loss_type"], classes=rs.NCLS, confidence=c["confidence"],
                                dis_loss_type=c["dis_loss_type"], is_cd_single_side=not c["two_sided"],
                                dis_loss_weight=c["w_dis"], hd_loss_weight=c["w_hd"], curv_loss_weight=c["w_curv"],
                                curv_loss_knn=case[2])
    logp = torch.log_softmax(d(inp["logits"]), dim=1)
    # the iterate is the leaf (d x / d offset = 1): inputs()'s x is ori + offset rounded to fp32, which is what both sides see
    offset, x = d(inp["offset"]), d(inp["x"]).clone().requires_grad_()
    _, loss,loss_n, _, dis, hd, curv, constrain = orc.forward_step(lambda _: (logp,), d(inp["ori"]), x, d(inp["normal"]),
                                                                    d(inp["kappa_ori"]), inp["target"], inp["scale"], cfg,
                                                                    c["targeted"])
    loss.backward()
    g = x.grad + d(inp["g"])
    off, m, v = rs.adam(offset, g, d(inp["m"]), d(inp["v"]), c["t"] + 1, inp["lr"], rs.BETAS, rs.EPS)
    return dict(g=g, loss_n=loss_n.detach(), dis=dis.detach(), hd=hd, curv=curv, constrain=constrain.detach(), offset=off,
                m=m, v=v, x=d(inp["ori"]) + off)


@pytest.mark.parametrize("name", sorted(CONFIGS))
@pytest.mark.parametrize("case", rs.CASES[:3])
def test_float64_restatement_equals_the_oracle_step(case, name):
    over = CONFIGS[name]
    ref = _oracle_step(case, over)
    got = rs.run(torch.float64, case, gval=1.0 / case[1], **over)      # the oracle's batch mean: 1 / B in float64
    for k, want in ref.items():
        if not torch.is_tensor(want):
            continue                      # a term the oracle leaves at 0 when its weight is 0
        want = want.detach()
        scale = max(float(want.abs().max()), 1e-30)
        assert float((got[k] - want).abs().max()) <= 1e-11 * scale, (k, name)


@pytest.mark.parametrize("case", rs.CASES)
def test_no_decision_sits_at_rounding_distance(case):
    r = rs.run(torch.float64, case)
    top = r["d_ao"].topk(2, dim=1)[0]
    assert float(((top[:, 0] - top[:, 1]) / top[:, 0]).min()) > 1e-4
    assert float(r["inner"].min()) > 1e-6
    r32 = rs.run(torch.float32, case)
    assert torch.equal(r32["hd_arg"], r["hd_arg"])


@pytest.mark.parametrize("case", rs.CASES)
def test_bands_can_fail(case):
    r64, r32 = rs.run(torch.float64, case), rs.run(torch.float32, case)
    band = rs.bands(r64, r32, names=rs.FLOAT_OUT)
    print({k: f"{v:.3g}" for k, v in band.items()})
    assert band["g"] < 1e-3 * float(r64["g"].abs().max())
    for k in ("dis", "hd", "curv", "constrain"):
        assert band[k] < 1e-4 * float(r64[k].abs().max()), k


def test_record_and_clip_branches_occur():
    """The record state of the cases takes all three branches, and lp_clip at 0.05 shortens some offsets and leaves others."""
    case = rs.CASES[1]
    inp = rs.inputs(*case)
    r = rs.run(torch.float32, case, t=3, search_step=1)
    assert r["best_step"].tolist() == [3, -1, -1] and r["best_bs"].tolist() == [1, -1, -1]
    assert r["iter_best_score"].tolist() == [int(r["pred"][0]), int(r["pred"][1]), -1]
    assert torch.equal(r["best_attack"][0], inp["x"][0]) and bool((r["best_attack"][1:] == 1).all())
    big = inp["offset"] * 20
    c = rs.run(torch.float64, case, offset=big, x=inp["ori"] + big, cc_linf=0.05)
    ln = c["offset"].norm(dim=1)
    assert int((ln > 0.05 * (1 - 1e-9)).sum()) > 0 and int((ln < 0.049).sum()) > 0 and float(ln.max()) <= 0.05 * (1 + 1e-9)
    s = rs.run(torch.float64, case, scheduler=True)
    assert s["lr"] == inp["lr"] * 0.9990
