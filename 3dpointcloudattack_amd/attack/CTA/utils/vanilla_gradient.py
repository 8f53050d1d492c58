"""attack/CTA/utils/vanilla_gradient.py of the reference: the victim's input gradient for the cotangent that is zero
except in rows j < set_size, where it is one-hot at target_class or — target_class falsy: None and class 0 alike — the
multi-hot of EVERY row's top-1 class (the reference's fancy-indexed assignment). Returned as numpy [3,N,B]. The
reference's image-only helpers (get_smoothed_mask, apply_region), which no point-cloud caller can reach, are not mirrored."""
import numpy as np

from .saliency_mask import SaliencyMask


class VanillaGradient(SaliencyMask):
    def __init__(self, model):
        super(VanillaGradient, self).__init__(model)

    def get_mask(self, image_tensor, target_class=None, set_size=2):
        from .. import CTA as _cta
        g = _cta.input_gradients(self.model, image_tensor.detach(), image_tensor.shape[0], target_class, set_size)
        return np.moveaxis(g.cpu().numpy(), 0, -1)
