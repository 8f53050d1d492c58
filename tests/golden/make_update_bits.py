#!/usr/bin/env python3
"""Record tests/golden/update_bits.npz: the bits the optimiser-update kernels compute on the seeded cases of
tests/update_bits_cases.py (Adam, the per-point clips and the best-attack bookkeeping of adam_clip_step, clip, cw_update,
cw_step, add_update, aof_update, iso_update, knn_attack_update and geoa3_update).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_update_bits.py [output.npz]

Needs the GPU and the built library. The kernels that run ARE the definition of the right bits: the file was recorded
on the commit before csrc/update_body.h gathered these statements into one place, and it is re-recorded ONLY by a change
that means to alter the arithmetic — never to make tests/test_update_bits_gpu.py pass. None of these kernels uses float
atomics and every sum runs in a fixed order; the recorder runs every case twice and refuses to write unless the two runs
agree bit for bit. Outputs of at most 4 KiB are stored as integer views, larger ones as the sha256 of that view.
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                       # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))      # the repository root
import update_bits_cases as ubc  # noqa: E402


def main(cases=ubc, name="update_bits.npz"):
    """Record the ENTRIES of `cases` (a module like update_bits_cases; make_wave_bits.py passes wave_bits_cases)."""
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, name)
    ops = importlib.import_module("3dpointcloudattack_amd.ops")
    dev = torch.device("cuda:0")
    rec = {}
    for entry, fn in cases.ENTRIES.items():
        first, second = fn(ops, dev), fn(ops, dev)
        torch.cuda.synchronize()
        for key, t in first.items():
            if not torch.equal(ubc.bits(t), ubc.bits(second[key])):
                raise SystemExit(f"{entry}/{key}: two runs disagree; nothing written")
            rec[f"{entry}/{key}"] = ubc.stored(t)
        print(f"{entry}: {len(first)} outputs")
    np.savez_compressed(out_path, **rec)
    print(f"{out_path}: {len(rec)} entries, {os.path.getsize(out_path)} bytes")


if __name__ == "__main__":
    main()
