"""attack/CTA/utils/integrated_gradients.py of the reference: integrated gradients of a set of clouds [B,3,N] -> float64
numpy [3,N,B]. All steps x B interpolated clouds are written by one launch and go through the victim together; the
sum over the steps (step order, double) and the product with (x - baseline) / steps are one more launch. A `process`
other than the default identity is applied per step on the host, as the reference applies it."""
import numpy as np

from .vanilla_gradient import VanillaGradient


class IntegratedGradients(VanillaGradient):
    def get_mask(self, image_tensor, target_class=None, baseline='black', steps=25, process=lambda x: x):
        from .. import CTA as _cta
        sal = _cta.saliency(self.model, image_tensor.detach()[None], [target_class], steps, baseline,
                            keep_grads=process is not _DEFAULT_PROCESS)
        if process is _DEFAULT_PROCESS:
            return sal["mask"][0].cpu().numpy()
        B, C, N = image_tensor.shape
        grad_sum = np.moveaxis(np.zeros((N, C, B)), 1, 0)
        g = sal["grads"].view(steps, B, C, N).cpu().numpy()
        for s in range(steps):
            grad_sum += process(np.moveaxis(g[s], 0, -1))
        diff = (image_tensor.detach() - sal["base"][0]).cpu().numpy()
        return grad_sum * np.moveaxis(diff, 0, -1) / steps


_DEFAULT_PROCESS = IntegratedGradients.get_mask.__defaults__[-1]
