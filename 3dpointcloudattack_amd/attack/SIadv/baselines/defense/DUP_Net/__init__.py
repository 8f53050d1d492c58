"""DUP-Net (SOR + the PU-Net upsampler) in front of a victim — attack/SIadv/baselines/defense/DUP_Net of the reference."""
from .DUP_Net import DUPNet  # noqa: F401
from .pu_net import PUNet  # noqa: F401
