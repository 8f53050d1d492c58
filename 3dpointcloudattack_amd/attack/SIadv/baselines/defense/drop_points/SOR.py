"""Grad-enable SOR defense (attack/SIadv/baselines/defense/drop_points/SOR.py) — the device-side head of ``defense.py``."""
from ......defense import SORDefense  # noqa: F401
