"""GPU parity, no tolerances: the two small kernels of the CW step that issue their global loads together at entry
(the tower's fold and the classifier tail) against the earlier form of each, kept behind a template flag and reached
with serial=True (pc3d_pointmlp3_fold_f32 with serial = 1, pc3d_cls_tail_serial_f32). Only WHERE the loads are
issued differs: arithmetic, comparison order and NaN behaviour are the same statements, so every returned array must
agree in every bit. Arrays are compared as int32 words (which pins the sign of zero and of infinity); a NaN must sit
where the other form has a NaN."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")


def _same_bits(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if not a.dtype.is_floating_point:
        return torch.equal(a, b)
    na, nb = torch.isnan(a).contiguous(), torch.isnan(b).contiguous()
    return torch.equal(na, nb) and torch.equal(a.contiguous().view(torch.int32)[~na], b.contiguous().view(torch.int32)[~nb])


# ------------------------------------------------------------------------------------------------------------
# fold
# ------------------------------------------------------------------------------------------------------------
def _fold_inputs(B, ntiles, C3, dev, seed):
    """Column c takes pattern c % 6: 0 random; 1 the same maximum in several tiles (the first must win); 2 a later tile
    strictly larger than everything before it; 3 a whole column of -inf; 4 NaN in the first tile; 5 NaN in a later tile."""
    g = torch.Generator().manual_seed(seed)
    val = torch.randn(B, ntiles, C3, generator=g)
    idx = torch.randint(0, 1 << 20, (B, ntiles, C3), generator=g, dtype=torch.int32)
    pat = torch.arange(C3) % 6
    last, mid = ntiles - 1, ntiles // 2
    val[:, :, pat == 1] = val[:, :, pat == 1].clamp(max=1.0)
    for t in {0, mid, last} if ntiles > 2 else set(range(ntiles)):
        val[:, t, pat == 1] = 3.0
    val[:, last, pat == 2] = 7.0
    if ntiles > 9:
        val[:, 8, pat == 2] = 6.0                      # the first tile of the second chunk beats the first chunk, then loses
    val[:, :, pat == 3] = -INF
    val[:, 0, pat == 4] = NAN
    val[:, last, pat == 5] = NAN                       # ntiles = 1: the first tile
    if ntiles > 2:
        val[:, 1, pat == 5] = NAN
    return val.to(dev), idx.to(dev)


@pytest.mark.parametrize("C3", [64, 1000, 1024])
@pytest.mark.parametrize("ntiles", [1, 2, 7, 8, 9, 16, 33])
def test_fold_matches_serial_form(ops, dev, ntiles, C3):
    for B, relu_last in itertools.product((1, 3), (False, True)):
        val, idx = _fold_inputs(B, ntiles, C3, dev, seed=ntiles * 7 + B)
        p0, i0 = ops.pointmlp3_fold_raw(val, idx, relu_last, serial=True)
        p1, i1 = ops.pointmlp3_fold_raw(val, idx, relu_last)
        assert _same_bits(p1, p0) and torch.equal(i1, i0), (B, ntiles, C3, relu_last)
        # the kept form is the definition: first tile unless a later one is strictly larger
        if not relu_last:
            pat = torch.arange(C3, device=dev) % 6
            assert torch.equal(i0[:, pat == 1], idx[:, 0, pat == 1]) and (p0[:, pat == 1] == 3.0).all()
            assert torch.equal(i0[:, pat == 2], idx[:, ntiles - 1, pat == 2])
            assert torch.equal(i0[:, pat == 3], idx[:, 0, pat == 3]) and (p0[:, pat == 3] == -INF).all()
            assert torch.isnan(p0[:, pat == 4]).all() and torch.equal(i0[:, pat == 4], idx[:, 0, pat == 4])
            if ntiles > 1:
                assert not torch.isnan(p0[:, pat == 5]).any()


def test_fold_keyword_of_the_tower_forward(ops, dev):
    """serial=True on pointmlp3_max_fwd_raw folds the same partials with the kept kernel (N = 300: 3 tiles, one partial)."""
    torch.manual_seed(5)
    x = torch.randn(2, 3, 300, device=dev) * 0.5
    w = tuple(t.to(dev) for t in (torch.randn(64, 3), torch.randn(64), torch.randn(128, 64) / 8, torch.randn(128),
                                  torch.randn(96, 128) / 11, torch.randn(96)))
    for relu_last in (False, True):
        p0, i0, m0 = ops.pointmlp3_max_fwd_raw(x, w, relu_last, want_masks=True, serial=True)
        p1, i1, m1 = ops.pointmlp3_max_fwd_raw(x, w, relu_last, want_masks=True)
        assert _same_bits(p1, p0) and torch.equal(i1, i0) and torch.equal(m1[0], m0[0]) and torch.equal(m1[1], m0[1])


# ------------------------------------------------------------------------------------------------------------
# classifier tail
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncls", [2, 40, 64])
@pytest.mark.parametrize("K2", [4, 128, 256])
def test_cls_tail_matches_serial_form(ops, dev, K2, ncls):
    g = torch.Generator().manual_seed(K2 * 64 + ncls)
    steps = [torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(2)]
    calls = 0
    for B in (1, 4, 5, 32):
        c2 = torch.randn(B, K2, generator=g).clamp(min=0).to(dev)
        w3 = (torch.randn(ncls, K2, generator=g) / K2 ** 0.5).to(dev)
        b3 = torch.randn(ncls, generator=g).to(dev)
        pred = ops.cls_tail(c2, w3, b3, torch.zeros(B, dtype=torch.int64, device=dev), 0, serial=True)[1]
        hit = torch.arange(B, device=dev) % 2 == 0        # even samples: target = arg-max; odd: another class
        target = torch.where(hit, pred, (pred + 1) % ncls)
        for kind, want_logp in itertools.product((0, 1, 2), (True, False)):
            r0 = ops.cls_tail(c2, w3, b3, target, kind, kappa=0.5, scale=1.0 / B, step=steps[0], want_logp=want_logp,
                              serial=True)
            r1 = ops.cls_tail(c2, w3, b3, target, kind, kappa=0.5, scale=1.0 / B, step=steps[1], want_logp=want_logp)
            calls += 1
            assert (r0[0] is None) == (r1[0] is None) == (not want_logp)
            for a0, a1 in zip(r0, r1):
                assert a0 is None or _same_bits(a1, a0), (B, K2, ncls, kind, want_logp)
            assert torch.equal(r0[1], pred)
            assert int(steps[0]) == calls and int(steps[1]) == calls      # up by exactly one per call
