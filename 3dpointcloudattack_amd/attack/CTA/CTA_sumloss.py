"""The critical-point attack with the loss summed over the set — MI355X mirror of the reference's
``attack/CTA/CTA_sumloss.py``. It differs from ``CTA.py`` in what it ranks and what it unmasks (CTA.py documents both;
DESIGN.md §8.8): the mask is moved to [B,3,N] first, so the contributions are per (sample, point) and level ``pa``
unmasks point ``contr_index[j][pa]`` of every sample j < set_size, with no cap; the levels start at ``n_points``; the
untargeted loss is ``alpha / set_size * sum_j z[j][ori]`` with nothing subtracted, the targeted and the softmax-neuron
losses are those of the LAST sample only (the reference's loop overwrites), divided by set_size; there is no distance
penalty (the block is commented out there). The device loop is ``CTA.cta_attack(variant='sumloss')``."""
from .CTA import _act_max, cta_attack, get_IG, layer_hook, sampling  # noqa: F401

stop_threshold = 5e-1
noise_weight = 1e-2


def act_max(network,
            input,
            layer_activation,
            layer_name,
            ori_cls,
            alpha,
            beta,
            target_att=False,
            IG_steps=25,
            n_points=1,
            verbose=False,
            using_softmax_neuron=False,
            penalize_dis=False,
            optimizer='Adam',
            set_size=2):
    """CTA_sumloss.py:57-290 for one set [S,3,N]: (state, best_img, ori_logits, max_other_logits), or None where the
    reference falls off its end."""
    return _act_max("sumloss", network, input, layer_activation, layer_name, ori_cls, alpha, beta, target_att, IG_steps,
                    n_points, verbose, using_softmax_neuron, penalize_dis, optimizer, set_size)
