"""attack/SIadv/baselines of the reference: ``from baselines import *`` yields what SIadv_attack.py uses — ClipPointsLinf
and the three defence heads (SORDefense, SRSDefense, DUPNet)."""
from .attack import *  # noqa: F401,F403
from .defense import *  # noqa: F401,F403
