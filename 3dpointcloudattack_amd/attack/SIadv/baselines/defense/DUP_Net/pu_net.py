"""PU-Net (CVPR'18), the upsampler of DUP-Net — DUP_Net/pu_net.py of the reference with the same constructor, the same
``state_dict`` keys and shapes (the reference checkpoint loads strictly) and the same [B,N,3] -> [B,up_ratio*N,3] forward.

What runs where: four set-abstraction levels on the PointNet++ kernels with the sampling / grouping chain
run ahead on the geometry stream; three feature-propagation levels as convolution-then-``ops.three_interp`` written straight
into the [B,N,260] concatenation [xyz | l1 | up1 | up2 | up3 | 0] (259 columns + one zero column so that the GEMM's K is a
multiple of four); the expansion as ONE GEMM with the branches' first layers stacked, one GEMM per branch, and the coordinate
head as one launch (``ops.pcd_tail``) that writes the reference's branch-major point order.

FPS start indices: the reference draws ``torch.randint(0, N_level, (B,))`` once per level and forward; so does this module,
through the start source of ``model.pointnet2_utils`` (``set_fps_start_source``). ``fps_start`` (an int, or an int tensor
[4,B]) fixes them: the module is then a pure function of its input and declares ``deterministic_forward``."""
import torch
import torch.nn as nn

from ...... import ops
from ......model import pointnet2_utils as _pn2
from ......model.pointnet import _FrozenFusedMixin
from .pu_modules import PointnetSAModule, PointnetFPModule
from .pytorch_modules import SharedMLP

# The expansion + reconstruction tail as one autograd node around the stacked GEMM, the per-branch GEMMs and the fused
# coordinate head (True), or composed from ops.linear_act layer by layer as the reference writes it (False: A/B timing and
# the parity fallback).
EXPAND_FUSED = True


class _ExpandFn(torch.autograd.Function):
    """X [B*N, 260] -> [B, r*N, 3]: relu(W1_k x + b1_k) for the r branches as one GEMM (W1 stacked, [r*256, 260]), relu(W2_k . +
    b2_k) per branch into one [r*B*N, 128] tensor, then the coordinate head (pc3d_pcd_tail_f32). Backward: the head's launch,
    one GEMM per branch on W2_k^T with the ReLU mask applied on load, one GEMM on the stacked W1^T."""

    @staticmethod
    def forward(ctx, X, B, N, r, w1, b1, w3, b3, w4, b4, *w2b2):
        BN, C1 = B * N, w1.shape[0] // r
        H1 = ops.gemm_nt(X, w1, b1, "relu", unit_rows=N)
        H2 = torch.empty((r * BN, w2b2[0].shape[0]), dtype=torch.float32, device=X.device)
        for k in range(r):
            ops.gemm_nt(H1[:, k * C1:(k + 1) * C1], w2b2[2 * k], w2b2[2 * k + 1], "relu", out=H2[k * BN:(k + 1) * BN], unit_rows=N)
        out, mask = ops.pcd_tail_raw(H2, w3, b3, w4, b4, B, N, r)
        ctx.save_for_backward(H1, H2, mask, w1, w3, w4, *w2b2[0::2])
        ctx.dims = (B, N, r, C1)
        return out

    @staticmethod
    def backward(ctx, g):
        H1, H2, mask, w1, w3, w4, *w2 = ctx.saved_tensors
        B, N, r, C1 = ctx.dims
        BN = B * N
        gH2 = ops.pcd_tail_bwd_raw(g, mask, w3, w4, B, N, r)
        gH1 = torch.empty_like(H1)
        for k in range(r):
            ops.gemm_nt(gH2[k * BN:(k + 1) * BN], ops._w_transposed(w2[k]), gate=H2[k * BN:(k + 1) * BN],
                        out=gH1[:, k * C1:(k + 1) * C1], unit_rows=N)
        gX = ops.gemm_nt(gH1, ops._w_transposed(w1), gate=H1, unit_rows=N)
        return (gX,) + (None,) * (9 + 2 * r)


class PUNet(_FrozenFusedMixin, nn.Module):

    def __init__(self, npoint=1024, up_ratio=2, use_normal=False, use_bn=False, use_res=False, fps_start=None):
        """npoint: input point number; up_ratio: the output has npoint * up_ratio points; use_normal / use_bn / use_res as in
        the reference (the device path runs the plain variant DUP-Net uses); fps_start: None (drawn per forward), an int, or
        an int tensor [4,B] — the start index of every level's farthest-point sampling."""
        super(PUNet, self).__init__()
        self.npoint = npoint
        self.use_normal = use_normal
        self.up_ratio = up_ratio
        self.npoints = [npoint, npoint // 2, npoint // 4, npoint // 8]
        mlps = [[32, 32, 64], [64, 64, 128], [128, 128, 256], [256, 256, 512]]
        radius = [0.05, 0.1, 0.2, 0.3]
        nsamples = [32, 32, 32, 32]

        in_ch = 0 if not use_normal else 3
        self.SA_modules = nn.ModuleList()
        for k in range(len(self.npoints)):
            self.SA_modules.append(PointnetSAModule(npoint=self.npoints[k], radius=radius[k], nsample=nsamples[k],
                                                    mlp=[in_ch] + mlps[k], use_xyz=True, use_res=use_res, bn=use_bn))
            in_ch = mlps[k][-1]

        self.FP_Modules = nn.ModuleList()
        for k in range(len(self.npoints) - 1):
            self.FP_Modules.append(PointnetFPModule(mlp=[mlps[k + 1][-1], 64], bn=use_bn))

        in_ch = len(self.npoints) * 64 + 3
        self.FC_Modules = nn.ModuleList()
        for k in range(up_ratio):
            self.FC_Modules.append(SharedMLP([in_ch, 256, 128], bn=use_bn))

        self.pcd_layer = nn.Sequential(SharedMLP([128, 64], bn=use_bn), SharedMLP([64, 3], activation=None, bn=False))
        self.fps_start = fps_start
        self.geometry_stream = True
        self._folded_cache = None

    @property
    def deterministic_forward(self):
        """A pure function of the input (fit for hipGraph capture / replay) once the FPS starts are fixed."""
        return self.fps_start is not None

    def _fold(self):
        """The expansion's weights in the layout the launches take: W1 of the branches stacked with a zero column (K = 260)."""
        fc = [m.layers() for m in self.FC_Modules]
        w1 = torch.cat([l[0][0] for l in fc], dim=0)
        w1 = torch.cat([w1, torch.zeros_like(w1[:, :1])], dim=1).contiguous()
        b1 = torch.cat([l[0][1] for l in fc], dim=0).contiguous()
        w2b2 = [t.contiguous() for l in fc for t in l[1][:2]]
        (w3, b3, _), = self.pcd_layer[0].layers()
        (w4, b4, _), = self.pcd_layer[1].layers()
        return dict(w1=w1, b1=b1, w2b2=w2b2, w3=w3.contiguous(), b3=b3.contiguous(), w4=w4.contiguous(), b4=b4.contiguous())

    def _starts(self, B, sizes, device):
        """Per level the int32 [B] start indices, or None where the level draws its own."""
        fs = self.fps_start
        if fs is None:
            return [None] * len(sizes)
        if isinstance(fs, int):
            if not 0 <= fs < min(sizes):
                raise ValueError(f"PUNet: fps_start={fs} is not an index of every level's cloud (sizes {sizes})")
            return [torch.full((B,), fs, dtype=torch.int32, device=device)] * len(sizes)
        fs = torch.as_tensor(fs)
        if tuple(fs.shape) != (len(sizes), B):
            raise ValueError(f"PUNet: fps_start must be an int or an int tensor [{len(sizes)},B={B}], got {tuple(fs.shape)}")
        fs = fs.to(device=device, dtype=torch.int32)
        return [fs[k].contiguous() for k in range(len(sizes))]

    def expand(self, feats, B, N):
        """[B,N,260] concatenation -> [B, up_ratio*N, 3]: expansion branches and coordinate reconstruction."""
        f = self.folded()
        r = self.up_ratio
        if EXPAND_FUSED and tuple(f["w3"].shape) == ops.PCD_TAIL_WIDTHS[:2][::-1]:
            return _ExpandFn.apply(feats.view(B * N, -1), B, N, r, f["w1"], f["b1"], f["w3"], f["b3"], f["w4"], f["b4"],
                                   *f["w2b2"])
        C1 = f["w1"].shape[0] // r
        h1 = ops.linear_act(feats, f["w1"], f["b1"], "relu")
        outs = []
        for k in range(r):
            h2 = ops.linear_act(h1[:, :, k * C1:(k + 1) * C1], f["w2b2"][2 * k], f["w2b2"][2 * k + 1], "relu")
            outs.append(ops.linear_act(ops.linear_act(h2, f["w3"], f["b3"], "relu"), f["w4"], f["b4"], None))
        return torch.cat(outs, dim=1)

    def forward(self, points, npoint=None, return_stages=False):
        """points [B,N,3] fp32 on the GPU -> [B, up_ratio*N, 3]. return_stages: also a dict of the intermediate tensors
        (fps / ball / nn index tables, l_feats channels-last, the concatenation)."""
        if not isinstance(points, torch.Tensor) or points.dim() != 3 or points.shape[2] != (6 if self.use_normal else 3):
            raise ValueError(f"PUNet: expected a [B,N,{6 if self.use_normal else 3}] tensor, got "
                             f"{tuple(getattr(points, 'shape', ()))}")
        if self.use_normal:
            raise NotImplementedError("PU-Net on the device path: use_normal is not implemented")
        npoints = list(self.npoints) if npoint is None else [npoint // 2 ** k for k in range(len(self.npoints))]
        B, N, _ = points.shape
        sizes = [N] + npoints[:-1]
        if any(s > n for s, n in zip(npoints, sizes)) or npoints[-1] < 3:
            raise ValueError(f"PUNet: a cloud of N={N} points cannot be sampled to {npoints}")
        self._require_fused(points)
        xyz = points.float()
        for m, s, st in zip(self.SA_modules, npoints, self._starts(B, sizes, points.device)):
            m.npoint, m.fps_start = s, st
        geos = _pn2.geometry_chain(self, xyz.permute(0, 2, 1), list(self.SA_modules))

        l_xyz, l_feats = [xyz], [None]
        for k, m in enumerate(self.SA_modules):
            lk_xyz, lk_feats = m.forward_cl(l_xyz[k], l_feats[k], geos[k])
            l_xyz.append(lk_xyz)
            l_feats.append(lk_feats)
        _pn2.geometry_join(self, xyz)

        C = l_feats[1].shape[2]
        width = 3 + C * (1 + len(self.FP_Modules))
        feats = torch.empty((B, N, (width + 3) // 4 * 4), dtype=torch.float32, device=points.device)
        feats[:, :, :3] = xyz
        feats[:, :, 3:3 + C] = l_feats[1]
        if feats.shape[2] > width:
            feats[:, :, width:] = 0.0
        for k, fp in enumerate(self.FP_Modules):
            feats = fp.forward_cl(xyz, l_xyz[k + 2], l_feats[k + 2], out=feats, col=3 + C * (k + 1))
        out = self.expand(feats, B, N)
        if return_stages:
            return out, dict(fps=[g[0] for g in geos], ball=[g[2] for g in geos], l_xyz=l_xyz, l_feats=l_feats, cat=feats)
        return out
