"""GPU: pc3d_eot_draw_f32 through ops.eot_draw against the restatement of its header text (tests/eot_draw_restatement.py):
idx and inv exactly, rot to the rounding of float32, rows outside the range untouched, bad arguments refused."""
import importlib

import numpy as np
import pytest
import torch

import eot_draw_restatement as rs

pytestmark = pytest.mark.gpu
M = importlib.import_module

# (K, E, cnt, T, row0, n0, seed): every K of {1, 2, 3, 33, 64, 192, 1000, 4096, 8192 (the LDS cap)}, E of {1, 10, 16}, cnt of
# {1, 3, 16}, row0 0 and 16 of T = 32 and T = 37 (once with the range ending at T), n0 of {0, 7, 2^31 + 5}, a negative seed
BIG = 2 ** 31 + 5
CASES = [
    (1, 1, 1, 32, 0, 0, 0),
    (2, 10, 3, 32, 16, 7, -5),
    (3, 16, 16, 32, 16, BIG, 2000),
    (33, 10, 3, 37, 5, 7, 123456789),
    (64, 16, 16, 32, 0, 0, -5),
    (192, 10, 16, 32, 16, BIG, 2000),
    (1000, 10, 3, 37, 34, 0, -5),
    (4096, 10, 16, 32, 0, 7, 2000),
    (8192, 16, 16, 32, 16, BIG, -5),
    (8192, 1, 1, 1, 0, 0, -(2 ** 63)),
]
IDS = ["K{}_E{}_cnt{}_T{}_row{}_n{}_seed{}".format(*c) for c in CASES]
ROT_FILL, INT_FILL = 7.0, -7
_RUNS = {}


def _tables(dev, T, E, K):
    return (torch.full((T, E, 3, 3), ROT_FILL, dtype=torch.float32, device=dev),
            torch.full((T, E, K), INT_FILL, dtype=torch.int32, device=dev),
            torch.full((T, E, K, 2), INT_FILL, dtype=torch.int32, device=dev))


def _run(dev, case):
    """Two launches into pre-filled tables (read back) and the restatement of the rows asked for, computed once."""
    if case not in _RUNS:
        ops = M("3dpointcloudattack_amd.ops")
        K, E, cnt, T, row0, n0, seed = case
        got = []
        for rows in (slice(row0, row0 + cnt), (row0, cnt)):      # both spellings of the rows
            rot, idx, inv = _tables(dev, T, E, K)
            ops.eot_draw(seed, n0, rows, rot, idx, inv)
            got.append((rot.cpu().numpy(), idx.cpu().numpy(), inv.cpu().numpy()))
        ref = [[rs.draw(seed, n0 + r, e, K) for e in range(E)] for r in range(cnt)]
        want = tuple(np.stack([np.stack([ref[r][e][k] for e in range(E)]) for r in range(cnt)]) for k in range(3))
        _RUNS[case] = (got, want)
    return _RUNS[case]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_indices_and_inverse_equal_the_restatement(dev, case):
    K, E, cnt, T, row0, n0, seed = case
    (first, _), (_, idx, inv) = _run(dev, case)
    assert np.array_equal(first[1][row0:row0 + cnt], idx)
    assert np.array_equal(first[2][row0:row0 + cnt], inv)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_rotations_equal_the_restatement(dev, case):
    K, E, cnt, T, row0, n0, seed = case
    (first, _), (rot, _, _) = _run(dev, case)
    got = first[0][row0:row0 + cnt].astype(np.float64)
    fixed = (rot == 0.0) | (rot == 1.0)                      # the exact entries of the case's matrix
    assert np.array_equal(got[fixed], rot[fixed])
    err = np.abs(got - rot).max()
    print(f"\n  max |rot - restatement| = {err:.3e}")
    assert err <= 2.0 ** -23


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_other_rows_keep_their_contents_and_launches_repeat(dev, case):
    K, E, cnt, T, row0, n0, seed = case
    (first, second), _ = _run(dev, case)
    outside = np.ones(T, dtype=bool)
    outside[row0:row0 + cnt] = False
    assert np.all(first[0][outside] == ROT_FILL) and np.all(first[1][outside] == INT_FILL) and np.all(first[2][outside] == INT_FILL)
    assert np.all(first[0][~outside] != ROT_FILL) and np.all(first[1][~outside] != INT_FILL)
    for a, b in zip(first, second):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))      # bit for bit


def test_rot_alone(dev):
    ops = M("3dpointcloudattack_amd.ops")
    case = CASES[5]
    K, E, cnt, T, row0, n0, seed = case
    (first, _), _ = _run(dev, case)
    rot, _, _ = _tables(dev, T, E, K)
    out = ops.eot_draw(seed, n0, (row0, cnt), rot)
    assert out[0] is rot and out[1] is None and out[2] is None
    assert np.array_equal(rot.cpu().numpy().view(np.int32), first[0].view(np.int32))
    # no rows: nothing is written
    rot, idx, inv = _tables(dev, T, E, K)
    ops.eot_draw(seed, n0, (row0, 0), rot, idx, inv)
    ops.eot_draw(seed, n0, slice(T, T), rot, idx, inv)
    assert bool((rot == ROT_FILL).all()) and bool((idx == INT_FILL).all()) and bool((inv == INT_FILL).all())


def test_bad_arguments_are_errors_without_a_launch(dev):
    ops, lib = M("3dpointcloudattack_amd.ops"), M("3dpointcloudattack_amd._lib")
    T, E, K = 8, 3, 16
    rot, idx, inv = _tables(dev, T, E, K)
    bad = [
        dict(rows=(0, T + 1)), dict(rows=(-1, 2)), dict(rows=(T, 1)), dict(rows=slice(6, 10)), dict(rows=slice(0, 4, 2)),
        dict(rows=(2, -1)), dict(n0=-1), dict(seed=2 ** 63), dict(inv=None), dict(idx=None),
        dict(idx=idx.long()), dict(inv=inv[:, :, :, :1]), dict(idx=idx[:, :, :8]), dict(rot=rot[:, :, :2]), dict(rot=rot.double()),
        dict(idx=idx.transpose(0, 1)), dict(rot=torch.zeros((T, 17, 3, 3), device=dev)),
    ]
    for kw in bad:
        a = dict(seed=1, n0=0, rows=(0, 2), rot=rot, idx=idx, inv=inv)
        a.update(kw)
        with pytest.raises((ValueError, TypeError)):
            ops.eot_draw(a["seed"], a["n0"], a["rows"], a["rot"], a["idx"], a["inv"])
    with pytest.raises(lib.Pc3dError):
        ops.eot_draw(1, 0, (0, 2), rot.cpu(), idx.cpu(), inv.cpu())
    with pytest.raises(lib.Pc3dError):
        ops.eot_draw(1, 0, (0, 2), rot, idx.cpu(), inv)
    # the C entry point itself: its own checks, before any HIP call
    p = (rot.data_ptr(), idx.data_ptr(), inv.data_ptr())
    st = torch.cuda.current_stream().cuda_stream
    for args in [(1, 0, 0, T + 1, T, E, K) + p, (1, 0, -1, 1, T, E, K) + p, (1, 0, 7, 2, T, E, K) + p, (1, 0, 0, -1, T, E, K) + p,
                 (1, -1, 0, 1, T, E, K) + p, (1, 0, 0, 1, T, 0, K) + p, (1, 0, 0, 1, T, ops.EOT_MAX_VIEWS + 1, K) + p,
                 (1, 0, 0, 1, T, E, 0) + p, (1, 0, 0, 1, T, E, ops.EOT_MAX_POINTS + 1) + p,
                 (1, 0, 0, 1, T, E, K, p[0], p[1], 0), (1, 0, 0, 1, T, E, K, p[0], 0, p[2]), (1, 0, 0, 1, T, E, K, 0, p[1], p[2]),
                 (1, 0, 2 ** 31 - 1, 2, T, E, K) + p]:
        with pytest.raises(lib.Pc3dError):
            lib.call("pc3d_eot_draw_f32", *args, st)
    torch.cuda.synchronize()
    assert bool((rot == ROT_FILL).all()) and bool((idx == INT_FILL).all()) and bool((inv == INT_FILL).all())
