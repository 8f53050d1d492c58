"""Every kernel that carries the optimiser step (csrc/update_body.h: Adam, the per-point clips, the best-attack decision)
against the bits recorded in tests/golden/update_bits.npz by tests/golden/make_update_bits.py. The inputs are regenerated
from the same module the recorder used (tests/update_bits_cases.py); every output is compared as integers, so one ulp, a
NaN or a signed zero that differs is a failure. A band against float64 (the other tests of these kernels) cannot see that.

cw_point_update also runs inside the tower-backward epilogue and behind the linear rider; they are held bit-equal to the
stand-alone kernels recorded here by tests/test_cw_riders_gpu.py (test_bwd_update_matches_bwd_then_cw_update,
test_linear_book_matches_cw_update_bookkeeping, test_cw_15_launch_iteration_equals_17_launch) and
tests/test_pointnet_cw_gpu.py (test_cw_update_equals_bookkeep_plus_step, test_launch_minimal_iteration_equals_generic_path),
so they need no entry of their own.
"""
import hashlib
import os

import numpy as np
import pytest
import torch

import update_bits_cases as ubc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    return np.load(os.path.join(GOLDEN, "update_bits.npz"))


@pytest.mark.parametrize("entry", list(ubc.ENTRIES))
def test_update_bits(entry, ops, dev, recorded):
    got = ubc.ENTRIES[entry](ops, dev)
    torch.cuda.synchronize()
    keys = {k[len(entry) + 1:] for k in recorded.files if k.startswith(entry + "/")}
    assert keys == set(got), "the cases and the record differ"
    bad = []
    for key, t in got.items():
        want, have = recorded[f"{entry}/{key}"], ubc.bits(t)
        if want.dtype == np.uint8:      # a large output: the sha256 of its integer view
            same = hashlib.sha256(have.numpy().tobytes()).digest() == want.tobytes()
        else:
            same = torch.equal(have, torch.from_numpy(want))
        if not same:
            bad.append(key)
    assert not bad, f"{entry}: {len(bad)} of {len(got)} outputs differ from the recorded bits: {bad[:8]}"
