"""GPU: the three ragged attacks launch what they launched before their host code moved into ragged.py — the names of the
library entries a dense and a ragged call go through, in order, against the lists recorded on the parent commit
(tests/ragged_launch_cases.py). Equality of the lists: no launch added, removed or reordered. What the launches compute is
pinned bit for bit by the ragged suites of the three attacks; this file only counts and orders."""
import importlib

import numpy as np
import pytest
import torch

import ragged_launch_cases as rc
from helpers import unit_cloud
from test_oracle_golden import _geo_cfg

pytestmark = pytest.mark.gpu
M = importlib.import_module
_lib = M("3dpointcloudattack_amd._lib")
seeding = M("3dpointcloudattack_amd.seeding")
pointnet = M("3dpointcloudattack_amd.model.pointnet")
cloud_io = M("3dpointcloudattack_amd.dataset.cloud_io")
cwm = M("3dpointcloudattack_amd.attack.CW.CW_attack")
knnm = M("3dpointcloudattack_amd.attack.KNN.KNN_attack")
ga = M("3dpointcloudattack_amd.attack.GeoA3.GeoA3_attack")
adv_u = M("3dpointcloudattack_amd.attack.CW.CW_utils.adv_utils")
dist_u = M("3dpointcloudattack_amd.attack.CW.CW_utils.dist_utils")
clip_u = M("3dpointcloudattack_amd.attack.CW.CW_utils.clip_utils")

B, KMAX, LENGTHS = 3, 40, [40, 33, 17]
SEEDS = [5, 6, 7]


def _victim(dev):
    m = pointnet.PointNetCls(k=40)
    m.load_state_dict(seeding.seeded_state_dict(m, 0))
    return m.eval().to(dev)


def _batch(lengths):
    rng = np.random.default_rng(31)
    data, lens = cloud_io.stack_ragged([unit_cloud(rng, n) for n in lengths])
    return torch.from_numpy(data), torch.tensor([1, 2, 3]), lens


def _cw(dev, lengths):
    victim = _victim(dev)
    atk = cwm.CW(victim, victim, adv_func=adv_u.UntargetedLogitsAdvLoss(5.), clip_func=clip_u.ClipPointsLinf(0.18),
                 dist_func=dist_u.ChamferDist(), binary_step=1, num_iter=2, graph=False, device=dev, sample_seeds=SEEDS,
                 global_batch=B)
    data, target, lens = _batch(lengths or [KMAX] * B)
    return lambda: atk.attack(data, target, *([lens] if lengths else []))


def _knn(dev, lengths):
    victim = _victim(dev)
    atk = knnm.CWKNN(victim, victim, None, None, None, None, adv_func=adv_u.UntargetedLogitsAdvLoss(5.),
                     dist_func=dist_u.ChamferkNNDist(), clip_func=clip_u.ProjectInnerClipLinf(0.18), attack_lr=1e-2, num_iter=2,
                     device=dev, graph=False, device_loop=True, sample_seeds=SEEDS, global_batch=B)
    data, target, lens = _batch(lengths or [KMAX] * B)

    def run():
        atk.attack(data, target, *([lens] if lengths else []))
        assert atk.last_path == "device_loop"
    return run


def _geoa3(dev, lengths):
    victim = _victim(dev)
    data, target, lens = _batch(lengths or [KMAX] * B)
    cfg = _geo_cfg(device_loop=True, graph_victim=False, binary_max_steps=1, iter_max_steps=2, sample_seeds=SEEDS,
                   global_batch=B, **(dict(lengths=lens) if lengths else {}))

    def run():
        ga.geoA3_attack(victim, victim, None, None, None, None, data, target.to(dev), cfg, 0, 1)
        assert ga.geoA3_attack.last_path == "device_loop"
    return run


CASES = {"cw_dense": (_cw, None), "cw_ragged": (_cw, LENGTHS), "cw_ragged_single_point": (_cw, [40, 1, 17]),
         "knn_dense": (_knn, None), "knn_ragged": (_knn, LENGTHS),
         "geoa3_dense": (_geoa3, None), "geoa3_ragged": (_geoa3, LENGTHS)}


def record(name, dev):
    """The entry names of the case's SECOND call on the same attacker and victim: the first call's preparation launches
    (weight folds, the screened tower's first-use fall-back) stay out of the list."""
    make, lengths = CASES[name]
    run = make(dev, lengths)
    run()
    names, call = [], _lib.call

    def recorder(entry, *args):
        names.append(entry)
        return call(entry, *args)

    _lib.call = recorder
    try:
        run()
    finally:
        _lib.call = call
    return names


@pytest.mark.parametrize("name", list(CASES))
def test_launches_are_the_parent_commits(dev, name):
    got = record(name, dev)
    print(f"{name}: {len(got)} launches")
    assert got == rc.EXPECTED[name]

