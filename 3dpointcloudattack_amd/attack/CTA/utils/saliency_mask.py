"""Base class of the saliency methods (the reference's attack/CTA/utils/saliency_mask.py): it holds the victim, put into
eval mode, and the list of hooks a subclass may have registered. The reference also moves the victim to the GPU when
there is one; here the caller has done that."""


class SaliencyMask(object):
    def __init__(self, model):
        model.eval()
        self.model, self.gradient, self.hooks = model, None, []

    def get_mask(self, image_tensor, target_class=None):
        raise NotImplementedError(f"{type(self).__name__} does not define get_mask; use VanillaGradient or IntegratedGradients")

    def remove_hooks(self):
        while self.hooks:
            self.hooks.pop().remove()
