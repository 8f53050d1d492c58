#!/usr/bin/env python3
"""Record tests/golden/wave_bits.npz: the bits of the kernels that reduce, scan or take an arg-max over a wavefront or a
workgroup, on the seeded cases of tests/wave_bits_cases.py.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_wave_bits.py [output.npz]

Needs the GPU and the built library. The file was recorded on commit b51b7c4 ("One Adam/clip/decision device body and one
loop-replay helper"), the parent of the change that gathered these loops into the primitives of csrc/pc3d_common.h: the
kernels of that commit ARE the definition of the right bits, and the file is re-recorded only by a change that means to
alter the arithmetic, never to make tests/test_wave_bits_gpu.py pass. The recorder is make_update_bits.py's: every case
runs twice and nothing is written unless the two runs agree bit for bit; outputs of at most 4 KiB are stored as integer
views, larger ones as the sha256 of that view.

One entry has been re-recorded since: pointnet_tower/N333-C1024-thK256/gx, with the change that starts the tower
backward's chain through T from +0 (tests/test_pointmlp_bwd_ref_gpu.py). Cloud 2 of that case has a row of T that is
negative throughout, and its 224 words of points without a hit were -0; they are +0 now. With -0 put back the new
output has the old hash, and the other 402 entries came out as they were.
"""
import make_update_bits          # puts tests/ and the repository root on sys.path
import wave_bits_cases

if __name__ == "__main__":
    make_update_bits.main(wave_bits_cases, "wave_bits.npz")
