"""GPU: ops.geoa3_update (pc3d_geoa3_update_f32) against tests/geoa3_step_restatement.py.

The kernel is fed the product's own search results (ops.nn_search_into / ops.knn_search_into) and the restatement gathers on
the same indices, so ties cannot matter. Every float output, the total gradient included, is held to
cw_step_restatement.bands — 16 x the fp32-vs-float64 deviation of the restatement on the same input, floor 16 x 2^-24 x
max|ref|; the copies (best_loss, iter_best_loss, best_attack) and every integer output must be exact.
tests/test_geoa3_step_cpu.py shows that no decision of these inputs sits at rounding distance.
"""
import pytest
import torch

import geoa3_step_restatement as rs

pytestmark = pytest.mark.gpu
KINDS = {("CE", True): 2, ("CE", False): 3, ("Margin", True): 1, ("Margin", False): 0}


def _search(ops, dev, x, ori, k):
    x, ori = x.to(dev).contiguous(), ori.to(dev).contiguous()
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


def _product(ops, dev, inp, found, pass_knn=True, **over):
    """One launch on a copy of the case; returns every tensor it writes, on the CPU."""
    c = dict(rs.DEFAULTS)
    c.update({k: over.pop(k) for k in list(over) if k in rs.DEFAULTS})
    a = {k: over.get(k, v) for k, v in inp.items()}
    t = {k: v.to(dev).clone().contiguous() for k, v in a.items() if torch.is_tensor(v)}
    B, _, N = t["x"].shape
    pred = torch.zeros((B,), dtype=torch.int64, device=dev)
    _, _, cls, _ = ops.cls_loss(t["logits"], t["target"], KINDS[(c["cls_loss_type"], c["targeted"])], c["confidence"],
                                scale=a["gval"], pred_out=pred)
    step = torch.full((B,), c["t"], dtype=torch.int32, device=dev)
    search = torch.tensor([c["search_step"]], dtype=torch.int32, device=dev)
    lr = torch.full((B,), a["lr"], dtype=torch.float64, device=dev)
    rows = torch.zeros((c["t"] + 2, B), device=dev)
    terms, hd_arg, g_out = torch.zeros((5, B), device=dev), torch.zeros((B,), dtype=torch.int32, device=dev), torch.zeros_like(t["x"])
    cd = c["dis_loss_type"] == "CD"
    curv = c["w_curv"] != 0
    ops.geoa3_update(t["x"], t["ori"], t["offset"], t["g"], t["m"], t["v"], step, search, lr, t["scale"], cls, pred, t["target"],
                     c["targeted"], t["constrain"], rows, t["best_loss"], t["best_attack"], t["best_bs"], t["best_step"],
                     t["iter_best_loss"], t["iter_best_score"],
                     nn_ao=found["nn_ao"] if found and (cd or curv) else None,
                     nn_oa=found["nn_oa"] if found and cd and c["two_sided"] else None,
                     knn_idx=found["knn_idx"] if found and pass_knn else None,
                     normal_ori=t["normal"] if pass_knn else None, kappa_ori=t["kappa_ori"] if pass_knn else None,
                     dis_kind=c["dis_loss_type"], gval=a["gval"], w_dis=c["w_dis"], w_hd=c["w_hd"], w_curv=c["w_curv"],
                     scheduler=c["scheduler"], cc_linf=c["cc_linf"], terms_out=terms, hd_arg_out=hd_arg, g_out=g_out)
    torch.cuda.synchronize(dev)
    out = {k: t[k].cpu() for k in ("x", "offset", "m", "v", "best_loss", "iter_best_loss", "best_attack", "best_step", "best_bs",
                                   "iter_best_score")}
    out.update(g=g_out.cpu(), constrain_word=t["constrain"].cpu(), hd_arg=hd_arg.cpu().long(), pred=pred.cpu(), lr=lr.cpu(), step=step.cpu(), rows=rows.cpu(),
               **{k: terms[i].cpu() for i, k in enumerate(rs.TERM_OUT)})
    return out


def _check(got, inp, found, **over):
    nb = {k: v.cpu() for k, v in found.items()} if found else {}
    ref64, ref32 = rs.step(torch.float64, inp, nb, **dict(over)), rs.step(torch.float32, inp, nb, **dict(over))
    band = rs.bands(ref64, ref32, names=rs.FLOAT_OUT)
    for name in rs.FLOAT_OUT:
        dev_ = float((got[name].double() - ref64[name]).abs().max())
        print(f"{name}: deviation {dev_:.3g}, band {band[name]:.3g}")
        assert dev_ <= band[name], name
    for name in rs.EXACT_OUT:
        assert torch.equal(got[name], ref32[name]), name
    for name in rs.INT_OUT + ("pred",):
        assert torch.equal(got[name], ref64[name]), (name, got[name], ref64[name])
    t = over.get("t", rs.DEFAULTS["t"])
    assert torch.equal(got["constrain_word"], got["constrain"])            # what the next record reads
    assert torch.equal(got["rows"][t], got["loss_n"]) and float(got["rows"][t + 1].abs().max()) == 0.
    assert got["step"].tolist() == [t + 1] * len(got["step"])
    return ref64


@pytest.mark.parametrize("case", rs.CASES)
def test_update_vs_float64_restatement(ops, dev, case):
    inp = rs.inputs(*case)
    found = _search(ops, dev, inp["x"], inp["ori"], case[2])
    got = _product(ops, dev, inp, found)
    _check(got, inp, found)


@pytest.mark.parametrize("case", [rs.CASES[0], rs.CASES[1]])
def test_single_sided_and_no_curvature(ops, dev, case):
    inp = rs.inputs(*case)
    found = _search(ops, dev, inp["x"], inp["ori"], case[2])
    _check(_product(ops, dev, inp, found, two_sided=False), inp, found, two_sided=False)
    with_w0 = _product(ops, dev, inp, found, w_curv=0.)
    _check(with_w0, inp, found, w_curv=0.)
    bare = _product(ops, dev, inp, found, pass_knn=False, w_curv=0.)           # ... and without a kNN result at all
    for name in rs.FLOAT_OUT + rs.EXACT_OUT + rs.INT_OUT:
        assert torch.equal(with_w0[name], bare[name]), name


@pytest.mark.parametrize("targeted", [False, True])
def test_l2_with_margin_needs_no_search(ops, dev, targeted):
    inp = rs.inputs(*rs.CASES[1])
    over = dict(cls_loss_type="Margin", confidence=5., dis_loss_type="L2", w_hd=0., w_curv=0., targeted=targeted)
    _check(_product(ops, dev, inp, None, pass_knn=False, **over), inp, None, **over)


def test_lp_clip(ops, dev):
    case = rs.CASES[1]
    inp = rs.inputs(*case)
    big = inp["offset"] * 20                     # lengths around 0.03 ... 0.3: the clip at 0.05 shortens some and leaves others
    x = inp["ori"] + big
    found = _search(ops, dev, x, inp["ori"], case[2])
    over = dict(offset=big, x=x, cc_linf=0.05)
    got = _product(ops, dev, inp, found, **over)
    _check(got, inp, found, **over)
    ln = got["offset"].norm(dim=1)
    assert int((ln > 0.0499).sum()) > 0 and int((ln < 0.049).sum()) > 0


@pytest.mark.parametrize("t", [0, 4])
def test_scheduler_and_step_word(ops, dev, t):
    """Adam steps 1 and 5; the lr word after the launch is the host's product lr * 0.9990 * ... bit for bit."""
    case = rs.CASES[1]
    inp = rs.inputs(*case)
    found = _search(ops, dev, inp["x"], inp["ori"], case[2])
    lr = inp["lr"]
    for _ in range(t):
        lr *= 0.9990
    over = dict(scheduler=True, t=t, lr=lr)
    got = _product(ops, dev, inp, found, **over)
    ref = _check(got, inp, found, **over)
    assert got["lr"].tolist() == [lr * 0.9990] * case[1] and ref["lr"] == lr * 0.9990
    plain = _product(ops, dev, inp, found, t=t, lr=lr)
    assert plain["lr"].tolist() == [lr] * case[1]


@pytest.mark.parametrize("targeted", [False, True])
def test_record_with_a_tie_in_the_logits(ops, dev, targeted):
    """Classes 5 and 17 share the maximum: the prediction is 5 (first index). Sample 0 improves both bests, sample 1 the
    step's best only, sample 2 fails."""
    case = rs.CASES[1]
    inp = rs.inputs(*case)
    logits = inp["logits"].clone()
    logits[:, 5] = logits[:, 17] = logits.max() + 1
    hit, miss = torch.tensor([5, 5, 17]), torch.tensor([17, 17, 5])
    target = hit if targeted else miss
    found = _search(ops, dev, inp["x"], inp["ori"], case[2])
    over = dict(logits=logits, target=target, targeted=targeted, t=3, search_step=1)
    got = _product(ops, dev, inp, found, **over)
    _check(got, inp, found, **over)
    assert got["pred"].tolist() == [5, 5, 5]
    assert got["best_step"].tolist() == [3, -1, -1] and got["best_bs"].tolist() == [1, -1, -1]
    assert got["iter_best_score"].tolist() == [5, 5, -1]
    assert torch.equal(got["best_attack"][0], inp["x"][0]) and bool((got["best_attack"][1:] == 1).all())


def test_coincident_points(ops, dev):
    """Two points of every cloud coincide: their difference vector has length 0, below the 1e-12 clamp."""
    case = rs.CASES[1]
    inp = rs.inputs(*case)
    offset = inp["offset"].clone()
    offset[:, :, 1] = inp["x"][:, :, 0] - inp["ori"][:, :, 1]
    x = inp["x"].clone()
    x[:, :, 1] = x[:, :, 0]
    found = _search(ops, dev, x, inp["ori"], case[2])
    knn = found["knn_idx"].cpu()
    assert bool((knn[:, 0, :2].sort(1)[0] == torch.tensor([0, 1])).all())
    got = _product(ops, dev, inp, found, x=x, offset=offset)
    _check(got, inp, found, x=x, offset=offset)
    assert bool(torch.isfinite(got["g"]).all())


def test_cap_and_refusal(ops, dev):
    n = ops.GEOA3_LOOP_MAX_POINTS
    assert n >= 2048 and ops.geoa3_update_fits(n, 16) and not ops.geoa3_update_fits(n + 4, 16)
    case = (n, 1, 16)
    inp = rs.inputs(*case)
    found = _search(ops, dev, inp["x"], inp["ori"], 16)
    _check(_product(ops, dev, inp, found), inp, found)
    big = {k: (torch.zeros((1, 3, n + 4)) if torch.is_tensor(v) and v.dim() == 3 else v) for k, v in inp.items()}
    big["kappa_ori"] = torch.zeros((1, n + 4))
    with pytest.raises(Exception, match="rc=-22"):
        _product(ops, dev, big, None, pass_knn=False, dis_loss_type="L2", w_hd=0., w_curv=0.)


def test_bitwise_properties(ops, dev):
    """Run == run; a sample inside a batch == the sample alone (same gval)."""
    case = rs.CASES[1]
    inp = rs.inputs(*case)
    found = _search(ops, dev, inp["x"], inp["ori"], case[2])
    base, again = _product(ops, dev, inp, found), _product(ops, dev, inp, found)
    names = rs.FLOAT_OUT + rs.EXACT_OUT + rs.INT_OUT
    for name in names:
        assert torch.equal(base[name], again[name]), name
    for b in range(case[1]):
        one = {k: (v[b:b + 1].contiguous() if torch.is_tensor(v) else v) for k, v in inp.items()}
        alone = _product(ops, dev, one, {k: v[b:b + 1].contiguous() for k, v in found.items()})
        for name in names:
            assert torch.equal(alone[name][0], base[name][b]), (name, b)
