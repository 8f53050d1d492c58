"""SRS defense (attack/SIadv/baselines/defense/drop_points/SRS.py) — the device-side head of ``defense.py``."""
from ......defense import SRSDefense  # noqa: F401
