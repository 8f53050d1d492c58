"""Every kernel that calls the wave / workgroup primitives of csrc/pc3d_common.h (arg-max with the lower index on a tie,
inclusive scans over 64, 32 and 16 lanes, sums / maxima / minima over groups of lanes, the two workgroup sums) and is not
already pinned by tests/test_update_bits_gpu.py, against the bits recorded in tests/golden/wave_bits.npz by
tests/golden/make_wave_bits.py on the commit before the primitives existed. The inputs are regenerated from the module the
recorder used (tests/wave_bits_cases.py); every output is compared as integers. DESIGN.md ("Wave primitives") maps each
call site to its entry here.
"""
import hashlib
import os

import numpy as np
import pytest
import torch

import wave_bits_cases as wbc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    return np.load(os.path.join(GOLDEN, "wave_bits.npz"))


@pytest.mark.parametrize("entry", list(wbc.ENTRIES))
def test_wave_bits(entry, ops, dev, recorded):
    got = wbc.ENTRIES[entry](ops, dev)
    torch.cuda.synchronize()
    keys = {k[len(entry) + 1:] for k in recorded.files if k.startswith(entry + "/")}
    assert keys == set(got), "the cases and the record differ"
    bad = []
    for key, t in got.items():
        want, have = recorded[f"{entry}/{key}"], wbc.bits(t)
        if want.dtype == np.uint8:      # a large output: the sha256 of its integer view
            same = hashlib.sha256(have.numpy().tobytes()).digest() == want.tobytes()
        else:
            same = torch.equal(have, torch.from_numpy(want))
        if not same:
            bad.append(key)
    assert not bad, f"{entry}: {len(bad)} of {len(got)} outputs differ from the recorded bits: {bad[:8]}"
