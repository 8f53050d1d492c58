"""CPU: batches of clouds of different sizes — dataset.cloud_io.stack_ragged / unstack_ragged, and the float64 restatement of
the ragged CW update (tests/cw_ragged_restatement.py) on a padded batch against the same restatement cloud by cloud."""
import importlib

import numpy as np
import pytest
import torch

import cw_ragged_restatement as rr
import cw_step_restatement as rs

cloud_io = importlib.import_module("3dpointcloudattack_amd.dataset.cloud_io")

LENGTHS = [1030, 1025, 1024, 513, 65, 3, 1]
KMAX = 1030


def test_stack_unstack_round_trip():
    rng = np.random.default_rng(5)
    clouds = [rng.standard_normal((n, 3)).astype(np.float32) for n in (7, 1, 12, 3)]
    data, lengths = cloud_io.stack_ragged(clouds)
    assert data.shape == (4, 12, 3) and data.dtype == np.float32
    assert lengths.dtype == np.int32 and lengths.tolist() == [7, 1, 12, 3]
    for b, c in enumerate(clouds):
        assert np.array_equal(data[b, :len(c)], c)
        assert np.array_equal(data[b, len(c):], np.broadcast_to(c[0], (12 - len(c), 3)))
    back = cloud_io.unstack_ragged(data, lengths)
    assert len(back) == 4 and all(np.array_equal(a, c) for a, c in zip(back, clouds))
    # tensors and float64 lists go in too; tensors come out as tensors
    data_t, lengths_t = cloud_io.stack_ragged([torch.from_numpy(c).double() for c in clouds])
    assert np.array_equal(data_t, data) and np.array_equal(lengths_t, lengths)
    back_t = cloud_io.unstack_ragged(torch.from_numpy(data), lengths)
    assert all(torch.is_tensor(a) and np.array_equal(a.numpy(), c) for a, c in zip(back_t, clouds))


@pytest.mark.parametrize("bad,word", [([], "empty"), ([np.zeros((4, 3)), np.zeros((0, 3))], "no points"),
                                      ([np.zeros((4, 3)), np.zeros((4, 2))], r"\[K, 3\]")])
def test_stack_ragged_rejections(bad, word):
    with pytest.raises(ValueError, match=word):
        cloud_io.stack_ragged(bad)


def _nan_padding(s, lengths):
    """The rows at and beyond every length of what the update must not read: NaN. ori keeps its padding (a searched index may
    name one of those rows)."""
    s = {k: v.copy() for k, v in s.items()}
    for b, L in enumerate(lengths):
        for k in ("adv", "g", "m", "v", "o_bestattack", "input_val"):
            s[k][b, :, L:] = np.nan
    return s


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("untarget", [True, False])
@pytest.mark.parametrize("dist_kind", [0, 1, 2])
def test_padded_batch_equals_cloud_by_cloud(dist_kind, untarget, dtype):
    """Exact: the restatement slices by length, so a cloud in the padded batch and the cloud alone see the same numbers."""
    B = len(LENGTHS)
    s = rr.inputs(LENGTHS, KMAX)
    padded = rr.step(dtype, _nan_padding(s, LENGTHS), LENGTHS, rs.T, untarget, dist_kind, nn_idx=s["rand_idx"])
    assert padded["copied"].any() and not padded["copied"].all()
    for b, L in enumerate(LENGTHS):
        one = {k: v[b:b + 1, :, :L].copy() if v.ndim == 3 else v[b:b + 1].copy() for k, v in s.items() if k != "rand_idx"}
        nn = np.where(s["rand_idx"][b:b + 1, :L] >= L, 0, s["rand_idx"][b:b + 1, :L])
        alone = rr.step(dtype, one, [L], rs.T, untarget, dist_kind, nn_idx=nn, batch=B)
        for k in rr.POINT_OUT:
            if k == "o_bestattack" and not padded["copied"][b]:
                continue                      # not written: the padded run still holds its NaN rows there
            assert np.array_equal(padded[k][b, :, :L], alone[k][0]), (k, b)
        for k in rr.VEC_OUT + ("copied",):
            assert np.array_equal(padded[k][b:b + 1], alone[k]), (k, b)
        # re-padding: the new point 0 in the iterate, the old one in the copies; m / v of the padding rows are not written
        assert np.array_equal(padded["adv"][b, :, L:], np.broadcast_to(padded["adv"][b, :, :1], (3, KMAX - L)))
        assert np.array_equal(padded["input_val"][b, :, L:], np.broadcast_to(s["adv"][b, :, :1].astype(dtype), (3, KMAX - L)))
        if padded["copied"][b]:
            assert np.array_equal(padded["o_bestattack"][b], padded["input_val"][b])
        assert np.isnan(padded["m"][b, :, L:]).all() and np.isnan(padded["v"][b, :, L:]).all()
        assert not np.isnan(padded["adv"][b]).any() and not np.isnan(padded["input_val"][b]).any()


@pytest.mark.parametrize("dist_kind", [0, 1, 2])
def test_full_lengths_equal_the_dense_restatement(dist_kind):
    """With every length = K the ragged restatement states what tests/cw_step_restatement.py (torch, autograd, a real
    torch.optim.Adam) states for the dense step: float64, to rounding."""
    K, B = 333, 3
    s = rr.inputs([K] * B, K, seed=1)
    nn = s["rand_idx"]
    got = rr.step(np.float64, s, [K] * B, rs.T, True, dist_kind, nn_idx=nn)
    t = {k: torch.from_numpy(v) for k, v in s.items()}
    want = rs.step(torch.float64, t["adv"], t["ori"], t["g"], t["m"], t["v"], rs.T, t["w"], t["pred"], t["label"], True,
                   t["bestdist"], t["bestscore"], t["o_bestdist"], t["o_bestscore"], t["o_bestattack"], dist_kind,
                   t["rand_idx"] if dist_kind == 2 else None, rs.LR, rs.BUDGET)
    for k in rs.FLOAT_OUT + ("input_val", "o_bestattack"):
        np.testing.assert_allclose(got[k], want[k].numpy(), rtol=1e-12, atol=1e-15, err_msg=k)
    for k in rs.INT_OUT + ("copied",):
        assert np.array_equal(got[k], want[k].numpy()), k
