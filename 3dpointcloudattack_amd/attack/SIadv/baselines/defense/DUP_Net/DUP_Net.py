"""DUP-Net (ICCV'19): statistical outlier removal followed by the PU-Net upsampler, as a head in front of a victim —
DUP_Net/DUP_Net.py of the reference: [B,3,K] -> [B,3,npoint*up_ratio], differentiable in the input.

The SOR stage is ``defense.SORDefense`` (one search + one launch, fixed output shape), the upsampler ``pu_net.PUNet``. The
reference reads ``pu-in_1024-up_4.pth`` beside its module; here ``weights`` names the checkpoint (see ``load_punet_weights``)
and a missing one is an error — never random weights silently."""
import glob
import os

import numpy as np
import torch
import torch.nn as nn

from ......defense import SORDefense
from .pu_net import PUNet

BASE_DIR = os.path.dirname(os.path.abspath(__file__))
CHECKPOINT = 'pu-in_1024-up_4.pth'
WEIGHTS_ENV = 'PC3D_PUNET_WEIGHTS'


def _read_weights(path):
    if path.endswith('.npz'):
        with np.load(path) as z:
            return {k: torch.from_numpy(z[k]) for k in z.files}
    return dict(torch.load(path, map_location='cpu', weights_only=True))


def load_punet_weights(weights=None):
    """A PU-Net ``state_dict`` from: a ``state_dict``; a path to a ``.pth`` (read with ``weights_only=True``) or ``.npz`` file
    (arrays named by the ``state_dict`` keys); a glob pattern or a list of such files whose keys are merged (a checkpoint
    split into parts). None: the environment variable PC3D_PUNET_WEIGHTS (a path, a glob or several joined by the path
    separator), then ``pu-in_1024-up_4.pth`` beside this module; otherwise FileNotFoundError."""
    if isinstance(weights, dict):
        return weights
    tried = []
    if weights is None:
        env = os.environ.get(WEIGHTS_ENV)
        if env:
            weights = env.split(os.pathsep)
        else:
            tried.append(f"${WEIGHTS_ENV} (not set)")
            weights = [os.path.join(BASE_DIR, CHECKPOINT)]
    if isinstance(weights, (str, os.PathLike)):
        weights = [os.fspath(weights)]
    paths = []
    for w in weights:
        hits = sorted(glob.glob(os.fspath(w))) if glob.has_magic(os.fspath(w)) else [os.fspath(w)]
        paths += hits
        tried.append(os.fspath(w))
    missing = [p for p in paths if not os.path.isfile(p)]
    if not paths or missing:
        raise FileNotFoundError("DUPNet: no PU-Net checkpoint found (looked at " + ", ".join(tried) + "); pass weights=<path to "
                                f"{CHECKPOINT}, .npz parts or a state_dict> or set {WEIGHTS_ENV}")
    state = {}
    for p in paths:
        state.update(_read_weights(p))
    return state


class DUPNet(nn.Module):

    def __init__(self, sor_k=2, sor_alpha=1.1, npoint=1024, up_ratio=4, weights=None, fps_start=None):
        super(DUPNet, self).__init__()
        self.npoint = npoint
        self.sor = SORDefense(k=sor_k, alpha=sor_alpha)
        self.pu_net = PUNet(npoint=self.npoint, up_ratio=up_ratio, use_normal=False, use_bn=False, use_res=False,
                            fps_start=fps_start)
        self.pu_net.load_state_dict(load_punet_weights(weights), strict=True)
        self.pu_net.eval()

    @property
    def deterministic_forward(self):
        return self.pu_net.deterministic_forward

    def train(self, mode=True):
        """The upsampler is frozen (the reference calls ``.eval()`` once and never trains it)."""
        super(DUPNet, self).train(mode)
        self.pu_net.eval()
        return self

    def forward(self, x):
        if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.shape[1] != 3:
            raise ValueError(f"DUPNet: expected a [B,3,K] tensor, got {tuple(getattr(x, 'shape', ()))}")
        with torch.enable_grad():
            x = self.sor(x)
            x = x.transpose(1, 2)
            x = self.pu_net(x)
            x = x.transpose(1, 2)
        return x
