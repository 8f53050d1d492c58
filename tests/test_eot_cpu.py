"""CPU: tests/eot_restatement.py (the float64 formulas csrc/eot.hip is held to on the GPU) against autograd through the
mirror's own composition — _renormalize, bmm, cat + index_select — in float64, and the C-ABI / ctypes declarations of the
two entries.

The tie case decides the kernel's rule: torch's CPU max(dim) returns the FIRST of two equal maxima and its backward sends
the whole gradient there; eot_restatement.centre_scale (and pc3d_eot_prepare_f32) take the lowest index accordingly. A
restatement with any other rule misses test_gradient_matches_autograd[tie-*] by the full size of the scale's gradient."""
import importlib
import os
import re

import numpy as np
import pytest
import torch

import eot_restatement as rs
from conftest import ROOT

cwm = importlib.import_module("3dpointcloudattack_amd.attack.additional_exp.CW_attack")


def _cloud(gen, B, K):
    ori = torch.randn((B, 3, K), generator=gen, dtype=torch.float64) * 0.4
    adv = ori + torch.randn((B, 3, K), generator=gen, dtype=torch.float64) * 0.02
    return adv, ori


def _rot(gen, E):
    out = []
    for e in range(E):
        th = float(torch.randn(1, generator=gen)) * 1e-2
        c, s = np.cos(th), np.sin(th)
        out.append([[[c, s, 0], [-s, c, 0], [0, 0, 1]], [[1, 0, 0], [0, c, s], [0, -s, c]], [[c, 0, s], [0, 1, 0], [-s, 0, c]],
                    [[1, 0, 0], [0, 1, 0], [0, 0, 1]]][e % 4])
    return torch.tensor(out, dtype=torch.float64)


def _autograd(adv, ori, gx, rot, idx, renorm):
    """d sum_e <gx_e, x_e> / d adv through the mirror's composition (CW_attack.py, the EOT branch and the plain one)."""
    B, _, K = adv.shape
    a = adv.clone().requires_grad_()
    if rot is None:
        x = cwm._renormalize(a) if renorm else a
        loss = (gx[:B] * x).sum()
    else:
        diff = a - ori
        loss = 0.
        for e in range(rot.shape[0]):
            x = torch.bmm(rot[e][None].expand(B, -1, -1), ori) + diff
            if renorm:
                x = cwm._renormalize(x)
            if idx is not None:
                x = torch.index_select(torch.cat((x, x), 2), 2, idx[e].long())
            loss = loss + (gx[(e + 1) * B:(e + 2) * B] * x).sum()
    loss.backward()
    return a.grad


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


# renorm x resample x EOT; the reference resamples views only, so there is no (resample, E = 0)
COMBOS = [(rn, rsm, E) for rn in (False, True) for rsm in (False, True) for E in (0, 1, 10) if E or not rsm]


@pytest.mark.parametrize("renorm,resample,E", COMBOS)
def test_gradient_matches_autograd(renorm, resample, E):
    gen = torch.Generator().manual_seed(11 + E)
    B, K = 2, 37
    adv, ori = _cloud(gen, B, K)
    rot = _rot(gen, E) if E else None
    idx = inv = None
    if resample:
        # columns of cat((x, x), 2) as the reference draws them (1 .. 2K-1, without replacement); view 0 is built by hand:
        # point 3 is drawn twice (3 and 3 + K), point 5 never
        rows = [torch.randperm(2 * K - 1, generator=gen)[:K] + 1 for _ in range(E)]
        rest = [j for j in range(1, 2 * K) if j % K not in (3, 5)]
        rows[0] = torch.tensor([3, 3 + K] + rest[:K - 2])
        idx = torch.stack(rows)
        inv = rs.inverse_table(idx, K)
        assert (inv[0, 3] >= 0).all() and (inv[0, 5] < 0).all()
    gx = torch.randn(((1 + E) * B, 3, K), generator=gen, dtype=torch.float64)
    want = _autograd(adv, ori, gx, rot, idx, renorm)
    got = rs.adv_gradient(adv, ori, gx, rot, inv, renorm)
    assert _rel(got, want) <= 1e-10
    # the forward half: the restatement's views are the composition's
    X = rs.prepare(adv, ori, rot, idx, renorm)[0]
    for e in range(E):
        x = torch.bmm(rot[e][None].expand(B, -1, -1), ori) + (adv - ori)
        x = cwm._renormalize(x) if renorm else x
        if resample:
            x = torch.index_select(torch.cat((x, x), 2), 2, idx[e].long())
        assert _rel(X[(e + 1) * B:(e + 2) * B], x) <= 1e-12
    x0 = cwm._renormalize(adv) if renorm else adv
    assert _rel(X[:B], x0) <= 1e-12


@pytest.mark.parametrize("E", [0, 1])
def test_gradient_matches_autograd_on_a_tie(E):
    """Two points tied for the largest norm (mirror images through the centroid, every coordinate a small dyadic number so
    that the centroid is exactly zero and the two norms are the same bits): torch's CPU max(dim) picks one of them, and
    the restatement's rule — the lowest index — must be that one."""
    B, K = 2, 12
    half = torch.tensor([[0.25, 0.5, -0.125], [1.5, 0.0, 0.0], [0.5, -0.75, 0.25], [-0.25, 0.125, 0.5], [0.0, 0.5, 0.5],
                         [0.375, 0.25, -0.5]], dtype=torch.float64)
    pts = torch.cat([half, -half])                                    # the maximum norm 1.5 at rows 1 and 7
    adv = torch.stack([pts.t(), pts.flip(0).t()]).contiguous()        # second cloud: the tie at 4 and 10
    ori = adv.clone()
    n = torch.sqrt((adv ** 2).sum(1))
    assert torch.equal(adv.sum(2), torch.zeros(2, 3, dtype=torch.float64)) and int((n[0] == n[0].max()).sum()) == 2
    rot = torch.eye(3, dtype=torch.float64)[None] if E else None
    gx = torch.randn(((1 + E) * B, 3, K), generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    want = _autograd(adv, ori, gx, rot, None, True)
    got = rs.adv_gradient(adv, ori, gx, rot, None, True)
    assert rs.prepare(adv, ori, rot, None, True)[3][E].tolist() == [1, 4]
    assert _rel(got, want) <= 1e-10


def test_host_inverse_table_matches_the_restatement():
    rng = np.random.default_rng(5)
    K = 130
    idx = np.stack([rng.permutation(np.arange(1, 2 * K))[:K] for _ in range(3)]).astype(np.int32)
    want = rs.inverse_table(torch.from_numpy(idx), K).numpy()
    for e in range(3):
        out = np.empty((K, 2), dtype=np.int32)
        cwm._inverse_columns(idx[e] % K, K, out)
        assert np.array_equal(out, want[e])


def test_entries_are_declared_and_bound():
    """include/pc3d.h declares pc3d_eot_prepare_f32 / pc3d_eot_update_f32 and _lib.py binds them with as many arguments."""
    lib = importlib.import_module("3dpointcloudattack_amd._lib")
    header = open(os.path.join(ROOT, "include", "pc3d.h")).read()
    for name in ("pc3d_eot_prepare_f32", "pc3d_eot_update_f32"):
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert decl is not None, name
        assert name in lib.SIGNATURES, name
        assert len(lib.SIGNATURES[name]) == len(decl.group(1).split(",")), name
    ops = importlib.import_module("3dpointcloudattack_amd.ops")
    assert callable(ops.eot_prepare) and callable(ops.eot_update)
    assert ops.EOT_MAX_POINTS == int(re.search(r"#define\s+PC3D_EOT_MAX_POINTS\s+(\d+)", header).group(1))
    assert ops.EOT_MAX_VIEWS == int(re.search(r"#define\s+PC3D_EOT_MAX_VIEWS\s+(\d+)", header).group(1))
