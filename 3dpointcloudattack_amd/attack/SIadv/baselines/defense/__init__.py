"""The three pre-processing defences of attack/SIadv/baselines/defense, as device-side heads (``defense.py``)."""
from .drop_points import SRSDefense, SORDefense  # noqa: F401
from .DUP_Net import DUPNet  # noqa: F401
