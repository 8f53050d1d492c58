"""attack/CTA/utils/dis_utils_numpy.py of the reference: the same functions as utils/dis_utils_numpy.py, re-exported."""
from ....utils.dis_utils_numpy import bid_hausdorff_dis, chamfer, pairwise_distances, sgd_hausdorff_dis  # noqa: F401
