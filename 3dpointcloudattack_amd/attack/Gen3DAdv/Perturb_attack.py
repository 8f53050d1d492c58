"""C&W point-perturbation attack with five transfer models — MI355X mirror of attack/Gen3DAdv/Perturb_attack.py.

The reference is the CW loop (attack/CW/CW_attack.py) with five transfer victims (PointNet, PointNet++ MSG / SSG, DGCNN,
CurveNet) checked after the search, as the kNN attack does. So this is the CW mirror (device-resident loop, fused update,
hipGraph replay) with the kNN mirror's transfer checks; transfer models may be None (skipped). The shuffled cloud is
classified as in the reference (numpy's global RNG advances) but, as there, no counter records it.
"""
import torch

from ..CW.CW_attack import CW as _CW
from ..CW.CW_attack import rand_row, rand_row_ragged
from ..KNN.KNN_attack import TRANSFER_MODELS, count_transfer_fails


class CW(_CW):
    """Class for CW attack."""

    def __init__(self, model, pt_model, ptm_model, pts_model, dgcnn_model, cur_model, adv_func, clip_func, dist_func,
                 attack_lr=1e-2, init_weight=10., max_weight=80., binary_step=10, num_iter=500, attack_method="untarget",
                 device=None, verbose=False, fused=True, graph=True, sample_seeds=None, global_batch=None,
                 deterministic=None):
        """Arguments as attack/Gen3DAdv/Perturb_attack.py:25-26; the extra keywords are the CW mirror's."""
        super().__init__(model, model, adv_func, clip_func, dist_func, attack_lr=attack_lr, init_weight=init_weight,
                         max_weight=max_weight, binary_step=binary_step, num_iter=num_iter, attack_method=attack_method,
                         device=device, verbose=verbose, fused=fused, graph=graph, sample_seeds=sample_seeds,
                         global_batch=global_batch, deterministic=deterministic)
        for (counter, attr), m in zip(TRANSFER_MODELS, (pt_model, ptm_model, pts_model, dgcnn_model, cur_model)):
            if m is not None:
                m = m.to(self.device)
                m.eval()
            setattr(self, attr, m)
            setattr(self, counter, 0)

    def _attack(self, data, target, lengths=None):
        """Returns (o_bestdist [B] float64, o_bestattack [B,K,3] float64, success_num) like the reference. lengths: the
        CW mirror's ragged batch; a transfer model that does not declare pad_invariant then sees every cloud alone, on
        its own [1,3,lengths[b]] slice."""
        st = self._begin(data, target, lengths)
        target, lens = st["target"], st["lengths_host"]
        self._search(st)
        success_num, o_bestattack = self._outcome(st)
        with torch.no_grad():
            count_transfer_fails(self, o_bestattack, target, lens)
            best_np = o_bestattack.double().cpu().numpy()
            if lens is None:
                shuffled = rand_row(best_np.transpose((0, 2, 1)))
            else:
                shuffled = rand_row_ragged(best_np.transpose((0, 2, 1)).copy(), lens)
            self.model(torch.from_numpy(shuffled.transpose((0, 2, 1)).copy()).float().to(self.device))
        return st["o_bestdist"].double().cpu().numpy(), best_np.transpose((0, 2, 1)), success_num
