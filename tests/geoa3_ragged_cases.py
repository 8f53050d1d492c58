"""TEST INFRASTRUCTURE: the cases of tests/test_geoa3_ragged_cpu.py and tests/test_geoa3_ragged_gpu.py — clouds of different
sizes for pc3d_geoa3_update_ragged_f32, built from tests/geoa3_step_restatement.py's own inputs (one case of B = 1 per
length; the input seed of a length N is geoa3_step_restatement.inputs' rule, 5 + N, or the position in its CASES).

The launch-level lengths sit on both sides of the update's 1024-thread stride (1025 | 1024 | 1023), of the search's
64-candidate step (65 | 64), at its 2048 tile, which is the update's cap, and at L = k + 1 (17); the small batch holds a
cloud of L = 4 at k = 2. The CPU file checks, before any GPU run, that on every one of them the float32 and the float64
restatement take the same decisions — the Hausdorff arg-max, the sign of every curvature inner product, the lp_clip branch
and the record — with a margin; the GPU file then holds the kernel to the restatement's bands.
"""
import functools

import torch

import geoa3_step_restatement as rs
from cw_step_restatement import nn_f64
from knn_step_restatement import knn_f64

LENGTHS = [2048, 1025, 1024, 1023, 65, 64, 17]
KMAX, K = 2048, 16
SMALL_LENGTHS, SMALL_K = [4, 67], 2
CC_LINF = 0.05
# the configurations of the float64 comparison: the default loss mix, and the scheduler with lp_clip on offsets 20 x as long
# (lengths 0.03 ... 0.3 around the clip at 0.05, tests/test_geoa3_step_gpu.py::test_lp_clip's construction)
CONFIGS = {"default": dict(t=3), "clip_scheduler": dict(cc_linf=CC_LINF, scheduler=True, t=3)}


@functools.lru_cache(maxsize=None)
def inputs(L, k, b, clip=False):
    """rs.inputs(L, 1, k) as cloud b of a batch: the record state takes a branch by b % 3 (0: improves both bests, 1: the
    step's best only, 2: fails — its label is its prediction), the scale constant follows; clip: the offsets 20 x as long.
    Never modified by its users."""
    inp = dict(rs.inputs(L, 1, k))
    mode = b % 3
    inp["scale"] = torch.tensor([[10., 20., 5.][mode]])
    if mode == 1:
        inp["best_loss"] = (inp["constrain"] * 0.5).contiguous()
    if mode == 2:
        inp["target"] = inp["logits"].argmax(1)
    if clip:
        inp["offset"] = inp["offset"] * 20
        inp["x"] = inp["ori"] + inp["offset"]
    return inp


@functools.lru_cache(maxsize=None)
def neighbours_f64(L, k, clip=False):
    inp = inputs(L, k, 0, clip)
    return dict(nn_ao=nn_f64(inp["x"], inp["ori"]), nn_oa=nn_f64(inp["ori"], inp["x"]), knn_idx=knn_f64(inp["x"], k)[1])


def signed_inner(dtype, inp, nb):
    """<normalize(p_j - p_i), n_i> [B,N,k] with its sign, rs.kappa's steps."""
    a = inp["x"].to(dtype).transpose(1, 2)
    B, N, _ = a.shape
    knn_idx = nb["knn_idx"]
    k = knn_idx.shape[2] - 1
    nrm = rs._rows(inp["normal"].to(dtype).transpose(1, 2), nb["nn_ao"])
    vec = rs._rows(a, knn_idx.long()[:, :, 1:].reshape(B, N * k)).view(B, N, k, 3) - a[:, :, None, :]
    vec = vec / vec.norm(2, 3, keepdim=True).clamp(min=1e-12)
    return (vec * nrm[:, :, None, :]).sum(3)
