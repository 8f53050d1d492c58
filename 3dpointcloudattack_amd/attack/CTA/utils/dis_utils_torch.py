"""attack/CTA/utils/dis_utils_torch.py of the reference: the same functions as utils/dis_utils_torch.py, re-exported
(the reference's copy differs by a debug print in pairwise_distances, which is not kept)."""
from ....utils.dis_utils_torch import bid_hausdorff_dis, chamfer, euclidean_distances, pairwise_distances, sgd_hausdorff_dis  # noqa: F401
