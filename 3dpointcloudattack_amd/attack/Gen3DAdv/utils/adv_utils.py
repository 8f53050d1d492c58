"""attack/Gen3DAdv/utils/adv_utils.py mirror. The reference's file is a copy of attack/CW/CW_utils/adv_utils.py (whitespace
aside), so this re-exports that mirror: the same classes, which the attacks' fast-path type checks recognise."""
from ...CW.CW_utils.adv_utils import *  # noqa: F401,F403
