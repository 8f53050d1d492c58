"""attack/CTA of the reference: the critical-point attack — integrated-gradients saliency of a set of clouds, then an
optimiser loop on its most salient points (CTA.py, CTA_sumloss.py), batched over sets and run on the device
(DESIGN.md §8.8)."""
