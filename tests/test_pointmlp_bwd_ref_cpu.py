"""CPU: tests/pointmlp_bwd_restatement.py, the float64 reference of the tower backward, checked on its own.

* it is right: on natural inputs (arg-max and ReLU decisions of a float64 torch forward) run(float64) equals torch
  autograd's x.grad and T.grad to 1e-12, with and without T, with and without the ReLU after the pool;
* the mask format round-trips, bit 63 and bit 31 included;
* every fp32 summation order stays inside 1/16 of the band on every case (that is what M_REF says), and
* every mutation of every case leaves the band of the unmutated reference, so the band can see the errors it is for.
The argument check of ops.pointmlp3_max_bwd_raw (T None with want_gT) is tested here too: it needs no GPU.
"""
import functools
import importlib

import pytest
import torch

import pointmlp_bwd_restatement as rs

CASES = rs.cases()
IDS = [c["name"] for c in CASES]


@pytest.mark.parametrize("relu_last", [False, True])
@pytest.mark.parametrize("with_T", [False, True])
@pytest.mark.parametrize("N,C3,B", [(1, 32, 2), (33, 64, 3), (160, 1024, 2)])
def test_restatement_equals_autograd(N, C3, B, with_T, relu_last):
    gen = torch.Generator().manual_seed(100 * N + C3 + with_T)
    w = tuple(t.double() for t in rs._weights(gen, C3))
    x = (torch.randn(B, 3, N, generator=gen) * 0.5).double().requires_grad_()
    T = (torch.randn(B, 3, 3, generator=gen) * 0.5).double().requires_grad_() if with_T else None
    g = torch.randn(B, C3, generator=gen).double()
    pooled, argidx, mask1, mask2, _ = rs.forward(torch.float64, x, T, w, relu_last)
    pooled.backward(g)
    if relu_last:
        assert 0 < int((pooled.detach() > 0).sum()) < pooled.numel()      # the mask of g does something
        g = g * (pooled.detach() > 0)
    gx, gT = rs.run(torch.float64, x.detach(), None if T is None else T.detach(), w[0], w[2], w[4], argidx, g, mask1, mask2)
    scale = float(x.grad.abs().max())
    assert scale > 0 and float((gx - x.grad).abs().max()) <= 1e-12 * scale
    if with_T:
        assert gT.shape == (B, (N + 31) // 32, 16) and not gT[:, :, 9:].any()
        got = gT.sum(1)[:, :9].reshape(B, 3, 3)
        assert float((got - T.grad).abs().max()) <= 1e-12 * float(T.grad.abs().max())
    else:
        assert gT is None


def test_per_cloud_w2_equals_autograd():
    gen = torch.Generator().manual_seed(5)
    B, N, C3 = 3, 70, 64
    w = [t.double() for t in rs._weights(gen, C3)]
    w[2] = (w[2][None] @ (torch.eye(64) + 0.2 * torch.randn(B, 64, 64, generator=gen)).double()).contiguous()
    x = torch.randn(B, 3, N, generator=gen).double().requires_grad_()
    T = torch.randn(B, 3, 3, generator=gen).double()
    g = torch.randn(B, C3, generator=gen).double()
    pooled, argidx, mask1, mask2, _ = rs.forward(torch.float64, x, T, w)
    pooled.backward(g)
    gx, _ = rs.run(torch.float64, x.detach(), T, w[0], w[2], w[4], argidx, g, mask1, mask2)
    assert float((gx - x.grad).abs().max()) <= 1e-12 * float(x.grad.abs().max())


def test_mask_round_trip():
    gen = torch.Generator().manual_seed(1)
    m1 = torch.rand(3, 50, 64, generator=gen) < 0.5
    m2 = torch.rand(3, 50, 128, generator=gen) < 0.5
    m1[0, 0], m1[0, 1] = False, True
    m1[0, 2] = torch.arange(64) == 63                       # the sign bit alone
    m2[0, 2] = torch.arange(128) % 32 == 31                 # every word's sign bit alone
    mask1, mask2 = rs.pack_masks(m1, m2)
    assert mask1.dtype == torch.int64 and mask2.dtype == torch.int32 and mask2.shape == (3, 50, 4)
    assert int(mask1[0, 0]) == 0 and int(mask1[0, 1]) == -1 and int(mask1[0, 2]) == -2 ** 63
    assert mask2[0, 2].tolist() == [-2 ** 31] * 4
    u1, u2 = rs.unpack_masks(mask1, mask2)
    assert torch.equal(u1, m1) and torch.equal(u2, m2)
    one = rs.pack_masks(torch.arange(64)[None, :] == torch.arange(64)[:, None],
                        torch.arange(128)[None, :] == torch.arange(64)[:, None] * 2 + 1)
    for j in range(64):                                     # bit j <-> channel j; word k // 32, bit k % 32 <-> channel k
        assert int(one[0][j]) & 0xFFFFFFFFFFFFFFFF == 1 << j
        k = 2 * j + 1
        assert [int(v) & 0xFFFFFFFF for v in one[1][j]] == [(1 << (k % 32)) if q == k // 32 else 0 for q in range(4)]


def test_case_list_covers_what_it_should():
    sizes = {c["x"].shape[2] for c in CASES}
    assert {1, 31, 32, 33, 127, 128, 129, 160, 257, 384, 1024} == sizes
    assert {c["W3"].shape[0] for c in CASES} == {32, 64, 1024}
    assert sum(c["x"].shape[2] == 1024 for c in CASES) == 1
    assert {c["hit"] for c in CASES} == {"natural", "one_owner", "one_per_point", "skewed", "last_sub_tile", "last_point",
                                         "live_in_tile", "empty_tiles"}
    assert {c["mask"] for c in CASES} == {"own", "random", "single_bit", "off_on_live", "all_on"}
    assert {c["g_kind"] for c in CASES} == {"randn", "small", "large", "dead_point", "nonfinite"}
    assert {c["x"].shape[0] for c in CASES} == {2, 3}
    for c in CASES:
        assert 0 <= int(c["argidx"].min()) and int(c["argidx"].max()) < c["x"].shape[2]
    live = sorted(int((rs.hit_counts(c["argidx"], c["g"], 384)[0, 128:256] > 0).sum()) for c in CASES
                  if c["hit"] == "live_in_tile" and not c["poisoned"])
    assert live == [1, 31, 32, 33, 64, 65, 96, 97, 128]


@functools.lru_cache(maxsize=None)
def _fp32_ratios(i):
    """{output: largest err / band over rs.ORDERS} of case i; the classes and pad words are checked on the way"""
    case = CASES[i]
    ref = rs.reference(i)
    ok_pt, ok_tile = rs.clean_points(case)
    q = {"gx": 0., "gT": 0.}
    for order in rs.ORDERS:
        gx, gT = rs.run(torch.float32, *rs.args_of(case), order=order)
        rs.check(case, gx, gT, ref, "%s, fp32 %s" % (case["name"], order))
        q["gx"] = max(q["gx"], rs.ratio(gx, ref[0], ref[2], ok_pt))
        if gT is not None:
            q["gT"] = max(q["gT"], rs.ratio(gT, ref[1], ref[3], ok_tile))
    return q


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_fp32_orders_stay_inside_the_band(i):
    """err / band <= 1 / 16 for every order: the band is 16 M_REF 2^-24 A, and M_REF bounds the fp32 restatements"""
    q = _fp32_ratios(i)
    print("%s: fp32 restatements at %.4f (gx) and %.4f (part_gT) of the band" % (CASES[i]["name"], q["gx"], q["gT"]))
    for k in q:
        assert q[k] <= 1. / rs.MARGIN, "%s %s: M_REF is too small" % (CASES[i]["name"], k)


def test_m_ref_is_the_measured_one():
    """the constant is the measurement rounded up, not a number with room in it"""
    for k in ("gx", "gT"):
        worst = max(range(len(CASES)), key=lambda i: _fp32_ratios(i)[k])
        m = _fp32_ratios(worst)[k] * rs.MARGIN * rs.M_REF[k]
        print("m_ref measured for %s: %.4f (%s); M_REF %.2f" % (k, m, CASES[worst]["name"], rs.M_REF[k]))
        assert 0.9 * rs.M_REF[k] <= m <= rs.M_REF[k]


@functools.lru_cache(maxsize=None)
def _mutation_ratios(i):
    """[(kind, err / band of the fp32 restatement on the mutated inputs against the unmutated reference)]"""
    case = CASES[i]
    ref = rs.reference(i)
    ok_pt, ok_tile = rs.clean_points(case)
    out = []
    for kind, over, exact in rs.mutations(i):
        assert exact > rs.SMALLEST_MARGIN
        gx, gT = rs.run(torch.float32, *rs.args_of(case, **over), order="fma")
        r = rs.ratio(gx, ref[0], ref[2], ok_pt)
        if gT is not None:
            r = max(r, rs.ratio(gT, ref[1], ref[3], ok_tile))
        with pytest.raises(AssertionError):
            rs.check(case, gx, gT, ref, kind)
        out.append((kind, r))
    return out


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_band_sees_every_mutation(i):
    rows = _mutation_ratios(i)
    print("%s: %s" % (CASES[i]["name"], ", ".join("%s %.3g" % r for r in rows)))
    for kind, r in rows:
        assert r > rs.SMALLEST_MARGIN - 1., "%s: %s stands only %.3g x the band" % (CASES[i]["name"], kind, r)


def test_every_mutation_kind_occurs():
    rows = [(r, kind, CASES[i]["name"]) for i in range(len(CASES)) for kind, r in _mutation_ratios(i)]
    assert {k for _, k, _ in rows} == set(rs.MUTATIONS)
    print("smallest mutation margin: %.3g x the band (%s, %s)" % min(rows))
    for kind in rs.MUTATIONS:                # and not in one lucky case only
        assert sum(k == kind for _, k, _ in rows) >= 5, kind


def test_want_gT_without_T_is_refused():
    """the balanced and packed kernels write part_gT only with T: the combination would return uninitialised memory"""
    ops = importlib.import_module("3dpointcloudattack_amd.ops")
    c = CASES[0]
    w = c["weights"]
    with pytest.raises(ValueError, match="T and part_gT go together"):
        ops.pointmlp3_max_bwd_raw(c["x"], w, c["argidx"], c["g"], (c["mask1"], c["mask2"]), T=None, want_gT=True)
