from .clip_utils import *  # noqa: F401,F403
