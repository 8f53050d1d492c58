"""attack/Gen3DAdv/utils/basic_util.py mirror. The reference's file is a copy of attack/CW/CW_utils/basic_util.py (whitespace
aside), so this re-exports that mirror: the same classes, which the attacks' fast-path type checks recognise."""
from ...CW.CW_utils.basic_util import *  # noqa: F401,F403
