"""The launch lists tests/test_eot_ragged_gpu.py holds the dense additional-experiments CW loop to: for each case, the names
of the library entries (every launch goes through _lib.call) of the second attack() on one attacker and victim, in order, the
way tests/ragged_launch_cases.py keeps them for the other loops.

EXPECTED was recorded with record() below on the parent commit 3e08dcf ("SI-Adv white-box loop: clouds of different sizes in
one batch"), which has no `lengths` keyword and no `_ragged` entries in this loop — not on the tree that carries this file:
the test asks whether `lengths=None` still launches what it launched, so its expectation must not come from the changed
code. A change that alters a list on purpose records it again on ITS parent and says so here.

Every name is written without its "pc3d_" prefix and "_f32" suffix."""
import importlib
import random

import numpy as np
import torch

B, K = 3, 40
# (renorm, views, resample, device_rng)
CASES = {"plain": (False, False, False, False), "renorm": (True, False, False, False),
         "eot_renorm_host": (True, True, False, False), "eot_renorm_resample_host": (True, True, True, False),
         "eot_renorm_resample_device": (True, True, True, True)}


def _names(text):
    return ["pc3d_" + w + "_f32" for w in text.split()]


def record(name, dev):
    """The entry names of the case's SECOND attack() on the same attacker and victim (the first one's preparation launches
    stay out), eager (graph=False: a replay makes no call), one binary step of two iterations."""
    M = importlib.import_module
    _lib = M("3dpointcloudattack_amd._lib")
    cwm = M("3dpointcloudattack_amd.attack.additional_exp.CW_attack")
    adv = M("3dpointcloudattack_amd.attack.CW.CW_utils.adv_utils")
    dist = M("3dpointcloudattack_amd.attack.CW.CW_utils.dist_utils")
    from helpers import hip_pointnet, unit_cloud
    renorm, views, resample, device_rng = CASES[name]
    net, _ = hip_pointnet(0, dev)
    rng = np.random.default_rng(31)
    pcs = torch.from_numpy(np.stack([unit_cloud(rng, K) for _ in range(B)]))
    atk = cwm.CW(net, cwm.AdvLossAdapter(adv.LogitsAdvLoss(0.), adv.UntargetedLogitsAdvLoss(0.)),
                 cwm.PerSampleDist(dist.ChamferDist()), binary_step=1, num_iter=2, whether_target=True, whether_1d=True,
                 whether_3Dtransform=views, whether_renormalization=renorm, whether_resample=resample, graph=False,
                 device_loop=True, device_rng=device_rng, seed=7)

    def run():
        torch.manual_seed(1)
        random.seed(1)
        atk.attack(pcs, torch.tensor([1, 2, 3]), torch.tensor([4, 5, 6]))
        assert atk.last_path == "device_loop"

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


_CLEAN = "pointmlp3_max_fwd linear linear linear pointmlp3_max_fwd linear linear linear"        # the clean prediction
_PASS = ("pointmlp3_max_fwd linear linear pointmlp3_max_fwd linear linear cls_tail linear linear pointmlp3_max_bwd linear_pre "
         "linear pointmlp3_max_bwd nn eot_update")                                            # the victim's passes, search, update

EXPECTED = {
    "plain": _names(f"{_CLEAN} {_PASS} {_PASS}"),
    "renorm": _names(f"{_CLEAN} eot_prepare {_PASS} eot_prepare {_PASS}"),
    "eot_renorm_host": _names(f"{_CLEAN} eot_prepare {_PASS} eot_prepare {_PASS}"),
    "eot_renorm_resample_host": _names(f"{_CLEAN} eot_prepare {_PASS} eot_prepare {_PASS}"),
    "eot_renorm_resample_device": _names(f"{_CLEAN} eot_draw eot_prepare {_PASS} eot_prepare {_PASS}"),
}
