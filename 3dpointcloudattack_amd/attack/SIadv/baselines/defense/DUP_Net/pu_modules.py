"""Set-abstraction and feature-propagation modules of PU-Net (DUP_Net/pu_modules.py of the reference) on the kernels the
PointNet++ victims run on: the same class names, constructor arguments, tensor layouts and ``state_dict`` keys
(``mlps.0.layer{i}.conv.*``, ``mlp.layer{i}.conv.*``).

A set-abstraction level is farthest-point sampling + ball query (run ahead on the geometry stream, they depend on the
coordinates only), the per-point / per-centre form of the first layer (``ops.sa_front``) and the remaining layers + group max
(``ops.grouped_mlp_max``, or ``group_act`` + ``mlp_relu_max`` for the widths the chain launch does not take), with the
convolutions' biases where the classifiers have folded batch norm. A feature-propagation level is the 3-NN search and
``ops.three_interp``; its 1x1 convolution runs BEFORE the interpolation on the known rows (the weights sum to one, so
relu(W interp(F) + b) = relu(interp(F W^T) + b) up to rounding; CONV_BEFORE_INTERP = False keeps the order as written).
Only what DUP-Net uses runs here: single scale, max pooling, no batch norm, no residual blocks."""
from typing import List

import torch
import torch.nn as nn

from ...... import ops
from ......model import pointnet2_utils as _pn2
from .pytorch_modules import SharedMLP

# The level's convolution on the M known rows, then 64 interpolated channels (True), or C2 interpolated channels, then the
# convolution on the N unknown rows as the reference writes it (False; kept for A/B timing and as the parity fallback).
CONV_BEFORE_INTERP = True


class QueryAndGroup(nn.Module):
    """Holds a grouping's radius and sample count (the search itself is ops.ball_query)."""

    def __init__(self, radius: float, nsample: int, use_xyz: bool = True):
        super(QueryAndGroup, self).__init__()
        self.radius, self.nsample, self.use_xyz = radius, nsample, use_xyz


class _PointnetSAModuleBase(nn.Module):
    def __init__(self):
        super(_PointnetSAModuleBase, self).__init__()
        self.npoint = None
        self.groupers = None
        self.mlps = None
        self.pool_method = 'max_pool'
        self.fps_start = None        # int32 [B] start indices of the next geometry() call (None: the start source's draw)

    def _single(self):
        if self.npoint is None or len(self.groupers) != 1 or self.pool_method != 'max_pool' or not self.groupers[0].use_xyz:
            raise NotImplementedError("PU-Net on the device path: single-scale grouping with use_xyz and max_pool only")
        return self.groupers[0]

    def split_layers(self):
        """([(W, b), ...], (Wx [C1,3], Wf [C1,D] or None, b1)) of the level's MLP in the kernels' [xyz(3), feat(D)] order,
        which is the order the reference concatenates in (pu_utils.py: grouped_xyz first)."""
        layers = [(w.contiguous(), b.contiguous()) for w, b, relu in self.mlps[0].layers()]
        return layers, _pn2._split_first(layers)

    def geometry(self, xyz_t, with_rev=True):
        """Centre indices, centres, group indices (+ unit table, reverse index) from detached coordinates [B,N,3]: the entry
        format of pointnet2_utils.geometry_chain."""
        grouper = self._single()
        B, N, _ = xyz_t.shape
        start = self.fps_start if self.fps_start is not None else _pn2._fps_start(B, N, xyz_t.device)
        fps_idx = ops.fps(xyz_t, self.npoint, start)
        centres = ops.group_gather(xyz_t, None, fps_idx.view(B, self.npoint, 1)).view(B, self.npoint, 3)
        idx = ops.ball_query(grouper.radius, grouper.nsample, xyz_t, centres)
        ev = torch.cuda.Event()
        ev.record()
        blocks = None
        widths = [w.shape[0] for w, _ in self.split_layers()[0]]
        if grouper.nsample in (32, 64, 128) and len(widths) == 3:
            unit = ops.sa_chain_table_unit(self.npoint, grouper.nsample, *widths)
            tbl = ops.sa_blocks(idx, unit) if unit else None
            if tbl is not None:
                ev_tb = torch.cuda.Event()
                blocks = tbl + (ev_tb,)
                ev_tb.record()
        g = [fps_idx, centres, idx, ev, None, None, N, blocks]
        if with_rev:
            self.geometry_rev(g)
        return g

    geometry_rev = staticmethod(_pn2.PointNetSetAbstraction.geometry_rev)

    def forward_cl(self, xyz_t, feats, geo=None):
        """xyz_t [B,N,3] (any strides), feats [B,N,D] channels-last or None -> (new_xyz [B,S,3], new_feats [B,S,C'])."""
        grouper = self._single()
        if not xyz_t.is_cuda:
            raise ops._lib.Pc3dError(f"{type(self).__name__}: input is on {xyz_t.device}; PU-Net runs on the GPU only")
        layers, first = self.split_layers()
        if not _pn2._front_supported(first, layers, grouper.nsample):
            raise NotImplementedError("PU-Net on the device path: this MLP shape is not covered by the grouped kernels")
        if geo is None:
            with torch.no_grad():
                geo = self.geometry(xyz_t.detach())
        fps_idx, _, idx, ev, rev = geo[:5]
        torch.cuda.current_stream(xyz_t.device).wait_event(ev)
        new_xyz, P, Bc = ops.sa_front(xyz_t, feats, fps_idx, *first)
        return new_xyz, _pn2._grouped_tail(P, Bc, idx, layers, rev, geo[7])

    def forward(self, xyz: torch.Tensor, features: torch.Tensor = None, npoint=None, new_xyz=None):
        """xyz [B,N,3], features [B,C,N] or None -> (new_xyz [B,npoint,3], new_features [B,C',npoint])."""
        if new_xyz is not None:
            raise NotImplementedError("PU-Net on the device path: the centres are sampled inside the level")
        if npoint is not None:
            self.npoint = npoint
        feats = None if features is None else features.permute(0, 2, 1).contiguous().float()
        new_xyz, new_feats = self.forward_cl(xyz.float(), feats)
        return new_xyz, new_feats.permute(0, 2, 1)


class PointnetSAModuleMSG(_PointnetSAModuleBase):
    """Pointnet set abstraction layer with multiscale grouping (the parameters of every scale; one scale runs)."""

    def __init__(self, *, npoint: int, radii: List[float], nsamples: List[int], mlps: List[List[int]], bn: bool = True,
                 use_xyz: bool = True, use_res=False, pool_method='max_pool', instance_norm=False):
        super(PointnetSAModuleMSG, self).__init__()
        assert len(radii) == len(nsamples) == len(mlps)
        if use_res:
            raise NotImplementedError
        self.npoint = npoint
        self.groupers = nn.ModuleList()
        self.mlps = nn.ModuleList()
        for radius, nsample, spec in zip(radii, nsamples, mlps):
            self.groupers.append(QueryAndGroup(radius, nsample, use_xyz=use_xyz))
            spec = list(spec)
            if use_xyz:
                spec[0] += 3
            self.mlps.append(SharedMLP(spec, bn=bn, instance_norm=instance_norm))
        self.pool_method = pool_method


class PointnetSAModule(PointnetSAModuleMSG):
    """Pointnet set abstraction layer"""

    def __init__(self, *, mlp: List[int], npoint: int = None, radius: float = None, nsample: int = None, bn: bool = True,
                 use_xyz: bool = True, use_res=False, pool_method='max_pool', instance_norm=False):
        super(PointnetSAModule, self).__init__(mlps=[mlp], npoint=npoint, radii=[radius], nsamples=[nsample], bn=bn,
                                               use_xyz=use_xyz, use_res=use_res, pool_method=pool_method,
                                               instance_norm=instance_norm)


class PointnetFPModule(nn.Module):
    """Propagates the features of one set to another: 3-NN inverse-distance interpolation + shared MLP."""

    def __init__(self, *, mlp: List[int], bn: bool = True):
        super(PointnetFPModule, self).__init__()
        self.mlp = SharedMLP(mlp, bn=bn)

    def forward_cl(self, unknown, known, known_feats, unknown_feats=None, out=None, col=0, conv_first=None):
        """unknown [B,n,3], known [B,m,3], known_feats [B,m,C2], unknown_feats [B,n,C1] or None (all channels-last) ->
        [B,n,mlp[-1]], or the caller's [B,n,ld] buffer with the columns [col, col + mlp[-1]) written."""
        layers = self.mlp.layers()
        B, n = unknown.shape[0], unknown.shape[1]
        conv_first = CONV_BEFORE_INTERP if conv_first is None else conv_first
        (w0, b0, relu0), rest = layers[0], layers[1:]
        todo = layers
        if known.shape[1] == 1:                                   # the reference's repeat branch
            y = known_feats.repeat(1, n, 1)
        elif conv_first and unknown_feats is None and w0.shape[0] % 4 == 0:
            g = ops.linear_act(known_feats, w0.contiguous(), None, None)            # the convolution on the m known rows
            if not rest and out is not None:
                return ops.three_interp(unknown, known, g, out=out, col=col, bias=b0, relu=relu0)
            y = ops.three_interp(unknown, known, g, bias=b0, relu=relu0)
            todo = rest
        else:
            y = ops.three_interp(unknown, known, known_feats)
        if unknown_feats is not None:
            y = torch.cat([unknown_feats, y], dim=-1)
        for w, b, relu in todo:
            y = ops.linear_act(y, w.contiguous(), b, "relu" if relu else None)
        if out is None:
            return y
        out[:, :, col:col + y.shape[2]] = y
        return out

    def forward(self, unknown: torch.Tensor, known: torch.Tensor, unknow_feats: torch.Tensor,
                known_feats: torch.Tensor) -> torch.Tensor:
        """unknown [B,n,3], known [B,m,3], unknow_feats [B,C1,n] or None, known_feats [B,C2,m] -> [B,mlp[-1],n]."""
        uf = None if unknow_feats is None else unknow_feats.permute(0, 2, 1).contiguous().float()
        y = self.forward_cl(unknown.float(), known.float(), known_feats.permute(0, 2, 1).contiguous().float(), uf)
        return y.permute(0, 2, 1)
