"""attack/SIadv/baselines/attack of the reference: the clip functors (util/clip_utils.py). Its adv_utils / dist_utils are
variants of attack/CW/CW_utils that the SI-Adv attack never calls; they are not mirrored."""
from .util import *  # noqa: F401,F403
