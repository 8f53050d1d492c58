"""Mirror of attack/SIadv/baselines/attack/util/clip_utils.py. Three of its four functors are line for line those of
attack/CW/CW_utils/clip_utils.py and are re-exported from there. ClipPointsLinf is not: here it is a true per-coordinate
clamp (clip_utils.py:46-61), where CW's class of the same name bounds each point's L2 norm."""
import torch
import torch.nn as nn

from ......attack.CW.CW_utils.clip_utils import ClipPointsL2, ProjectInnerClipLinf, ProjectInnerPoints  # noqa: F401

__all__ = ["ClipPointsL2", "ClipPointsLinf", "ProjectInnerPoints", "ProjectInnerClipLinf"]


class ClipPointsLinf(nn.Module):
    """pc clamped to ori_pc +- budget in every coordinate; plain torch, any device and layout. Inside the attack loop
    the same clamp is the last stage of pc3d_si_step_f32."""

    def __init__(self, budget):
        super(ClipPointsLinf, self).__init__()
        self.budget = budget

    def forward(self, pc, ori_pc):
        with torch.no_grad():
            diff = pc - ori_pc
            diff = torch.clamp(diff, min=-self.budget, max=self.budget)
            pc = ori_pc + diff
        return pc
