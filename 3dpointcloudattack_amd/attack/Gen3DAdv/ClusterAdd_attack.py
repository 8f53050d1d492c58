"""Cluster-adding C&W attack (Xiang et al., CVPR'19) — MI355X mirror of attack/Gen3DAdv/ClusterAdd_attack.py.

The loop is CWAdd's (IndpAdd_attack.py in this package: persistent [ori | adv] buffer, fused victim, one update launch
whose distance term is FarChamferDist's farthest intra-cluster pair + Chamfer). What differs is the start cloud
(:80-126): 128 critical points, DBSCAN(eps=0.2, min_samples=3) per cloud, the `num_add` largest clusters resampled to
`cl_num_p` points each (with replacement, hence duplicate points, when a cluster has <= cl_num_p points), kNN clusters
of random points when there are too few clusters. DBSCAN runs on the host (once per attack) as a numpy restatement of
scikit-learn's semantics (dbscan_labels below), so nothing depends on scikit-learn; the selection around it makes the
reference's np.unique / np.argsort / np.random.choice calls in the reference's order, so numpy's global stream advances
exactly as the reference's does. There are no post-attack checks (the reference has none).
"""
import numpy as np
import torch

from .IndpAdd_attack import CWAdd as _CWAdd
from .IndpAdd_attack import get_critical_points  # noqa: F401  (the reference defines the same function, :12-39)


def dbscan_labels(points, eps=0.2, min_samples=3):
    """scikit-learn's DBSCAN(eps, min_samples).fit_predict on points [N,3] (Euclidean), restated:
    * a core point has >= min_samples points within eps (distance <= eps, the point itself counted);
    * clusters are the connected components of core points (neighbours within eps), labelled 0, 1, ... in the order
      of the smallest core index in each;
    * a border point (not core, within eps of a core point) takes the smallest label among the core points next to it;
    * every other point is -1 (noise)."""
    p = np.asarray(points, dtype=np.float64)
    n = p.shape[0]
    dist = np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(-1))
    near = dist <= eps
    core = near.sum(1) >= min_samples
    labels = np.full(n, -1, dtype=np.int64)
    nxt = 0
    for seed in range(n):
        if not core[seed] or labels[seed] != -1:
            continue
        # grow the component of `seed`: core points spread the label, border points only receive it (first come —
        # components are grown in increasing label order, so that is the smallest adjacent label)
        labels[seed] = nxt
        frontier = [seed]
        while frontier:
            i = frontier.pop()
            for j in np.nonzero(near[i] & (labels == -1))[0]:
                labels[j] = nxt
                if core[j]:
                    frontier.append(j)
        nxt += 1
    return labels


def select_clusters(points, labels, num_add, cl_num_p):
    """The reference's selection from one cloud's clustered critical points (:104-126) -> [num_add, cl_num_p, 3]."""
    keep = labels > -0.5
    labels, points = labels[keep], points[keep]
    if len(points) == 0:
        raise ValueError("CWAddClusters: DBSCAN found no cluster among the critical points")
    uniq, counts = np.unique(labels, return_counts=True)
    out = []
    for lab in uniq[np.argsort(counts)[-num_add:]]:
        members = points[labels == lab]
        pick = np.random.choice(len(members), cl_num_p, replace=not (len(members) > cl_num_p))
        out.append(members[pick])
    while len(out) < num_add:
        centre = points[np.random.choice(len(points), 1)[0]]
        order = np.argsort(np.sum((points - centre[None, :]) ** 2, axis=1))[:cl_num_p]
        out.append(points[order])
    return np.array(out)


class CWAddClusters(_CWAdd):
    """Class for CW attack."""

    def __init__(self, model, trans_model, adv_func, dist_func, attack_lr=1e-2, init_weight=5., max_weight=30.,
                 binary_step=5, num_iter=500, num_add=3, cl_num_p=32, attack_method='untarget', device=None,
                 verbose=False, fused=True, graph=True, sample_seeds=None, global_batch=None, deterministic=None):
        """Arguments as attack/Gen3DAdv/ClusterAdd_attack.py:47-49 (num_add clusters of cl_num_p points); the extra
        keywords are the CW mirror's. `init_points` (attribute, default None): a [B,3,num_add*cl_num_p] start cloud
        used instead of the clustering."""
        super().__init__(model, trans_model, adv_func, dist_func, attack_lr=attack_lr, init_weight=init_weight,
                         max_weight=max_weight, binary_step=binary_step, num_iter=num_iter, num_add=num_add,
                         attack_method=attack_method, device=device, verbose=verbose, fused=fused, graph=graph,
                         sample_seeds=sample_seeds, global_batch=global_batch, deterministic=deterministic)
        self.cl_num_p = cl_num_p

    def _init_centers(self, pc, label):
        """Clusters of critical points as start points (:80-126) -> np.ndarray [B, num_add, cl_num_p, 3]."""
        cri = get_critical_points(self.model, pc, label, 128)
        pts = cri.transpose(1, 2).cpu().numpy()      # [B, 128, 3]
        return np.array([select_clusters(p, dbscan_labels(p, 0.2, 3), self.num_add, self.cl_num_p) for p in pts])

    def _initial_points(self, ori, label):
        clusters = torch.from_numpy(self._init_centers(ori, label)).float().to(self.device)
        B = clusters.shape[0]
        return clusters.view(B, self.num_add * self.cl_num_p, 3).transpose(1, 2).contiguous()

    def _attack(self, data, target):
        """Returns (o_bestdist [B] float64, concat(ori, added) [B,K+A,3] float64, success_num) like the reference
        (:288); no post-attack checks."""
        st = self._begin(data, target)
        self._search(st)
        o_bestdist, o_bestattack, success_num = self._finish(st)
        if self.verbose:
            print('Successfully attack {}/{}'.format(success_num, st["B"]))
        return o_bestdist, self._result(st, o_bestattack), success_num
