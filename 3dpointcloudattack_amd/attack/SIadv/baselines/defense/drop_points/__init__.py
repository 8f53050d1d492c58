from .SOR import SORDefense  # noqa: F401
from .SRS import SRSDefense  # noqa: F401
