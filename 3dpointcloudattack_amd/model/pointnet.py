"""PointNet classifier — MI355X mirror of the reference's ``model/pointnet.py`` (same class names, constructor
arguments, sub-module names and ``state_dict`` keys, so reference checkpoints load unchanged).

The attack path runs the victim in eval mode with frozen weights (attack/CW/CW_attack.py:40-41). In that mode
``forward`` does not run Conv1d/BatchNorm/max as separate ops: eval BatchNorm is folded into the conv/linear
weights once, and each tower (3 -> 64 -> 128 -> 1024 + max over points) is ONE fused HIP launch pair
(``pc3d_pointmlp3_max_{fwd,bwd}_f32``, fp32 MFMA) that never writes the [B,C,N] activations.

``feature_transform=True`` adds STNkd (the 64 x 64 feature transform). Its tower and the trunk then run on the
``pc3d_pointnet_ft_*`` kernels: the transform is folded into the trunk's layer-2 weight per cloud instead of being
applied to every point. The ``feature_transform=False`` path launches exactly what it did before.

Reference: STN3d model/pointnet.py:14-48, STNkd :51-87, PointNetfeat :89-128, PointNetCls :130-148.
"""

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops


def _fold_bn(weight, bias, bn):
    """Fold eval-mode BatchNorm1d into the preceding 1x1 conv / linear: y = s*(Wx+b-mean)+beta."""
    w = weight.detach().reshape(weight.shape[0], -1).float()
    s = bn.weight.detach().float() / torch.sqrt(bn.running_var.detach().float() + bn.eps)
    b = bias.detach().float() if bias is not None else torch.zeros_like(s)
    return (w * s[:, None]).contiguous(), ((b - bn.running_mean.detach().float()) * s + bn.bias.detach().float()).contiguous()


def _plain(weight, bias):
    """Snapshot (never a view of the parameter: a captured graph keeps replaying the weights it was captured with)."""
    return weight.detach().reshape(weight.shape[0], -1).float().clone(), bias.detach().float().clone()


class _FrozenFusedMixin:
    """Shared machinery: the folded-weight cache of a frozen module. The cache is keyed on (data_ptr, version) of every
    parameter / buffer it was folded from (the module's own and those of plain sub-modules; sub-modules that carry this
    mixin key their own caches), so ``load_state_dict`` on ANY ancestor, in-place weight updates and real device moves
    re-fold, while a no-op ``.to()`` / ``.eval()`` keeps the tensors a captured hipGraph may point at."""

    def _own_tensors(self):
        stack = [self]
        while stack:
            m = stack.pop()
            for t in m._parameters.values():
                if t is not None:
                    yield t
            for t in m._buffers.values():
                if t is not None:
                    yield t
            for c in m._modules.values():
                if c is not None and not isinstance(c, _FrozenFusedMixin):
                    stack.append(c)

    def _source_key(self):
        return tuple((t.data_ptr(), t._version) for t in self._own_tensors())

    def folded(self):
        """The module's folded weights (built by ``_fold``), re-folded when a source tensor changed."""
        key = self._source_key()
        d = self.__dict__
        if d.get("_folded_cache") is None or d.get("_folded_key") != key:
            object.__setattr__(self, "_folded_cache", self._fold())
            object.__setattr__(self, "_folded_key", key)
        return d["_folded_cache"]

    def _invalidate(self):
        object.__setattr__(self, "_folded_cache", None)
        object.__setattr__(self, "_fused_cache", None)

    def _require_fused(self, x):
        if self.training:
            raise NotImplementedError(
                f"{type(self).__name__}: only the eval-mode (frozen-weight) attack path is implemented on MI355X; "
                "training the victim is out of scope (SURVEY §2.1 train.py)")
        if not x.is_cuda:
            raise ops._lib.Pc3dError(f"{type(self).__name__}: input is on {x.device}; the fused path runs on the GPU only")


class STN3d(_FrozenFusedMixin, nn.Module):
    """Input transform net (model/pointnet.py:14-48)."""

    def __init__(self):
        super(STN3d, self).__init__()
        self.conv1 = torch.nn.Conv1d(3, 64, 1)
        self.conv2 = torch.nn.Conv1d(64, 128, 1)
        self.conv3 = torch.nn.Conv1d(128, 1024, 1)
        self.fc1 = nn.Linear(1024, 512)
        self.fc2 = nn.Linear(512, 256)
        self.fc3 = nn.Linear(256, 9)
        self.relu = nn.ReLU()

        self.bn1 = nn.BatchNorm1d(64)
        self.bn2 = nn.BatchNorm1d(128)
        self.bn3 = nn.BatchNorm1d(1024)
        self.bn4 = nn.BatchNorm1d(512)
        self.bn5 = nn.BatchNorm1d(256)
        self._folded_cache = None

    def _fold(self):
        tower = _fold_bn(self.conv1.weight, self.conv1.bias, self.bn1) + \
            _fold_bn(self.conv2.weight, self.conv2.bias, self.bn2) + \
            _fold_bn(self.conv3.weight, self.conv3.bias, self.bn3)
        tower = tower + (tower[2].t().contiguous(), [])  # W2^T for the backward kernel; the holder of W3's prepared image (PointNetfeat._fold)
        head = (_fold_bn(self.fc1.weight, self.fc1.bias, self.bn4),
                _fold_bn(self.fc2.weight, self.fc2.bias, self.bn5),
                _plain(self.fc3.weight, self.fc3.bias))
        iden = torch.eye(3, dtype=torch.float32, device=self.fc3.weight.device).reshape(1, 9)
        return tower, head, iden

    def forward(self, x, blocked_bwd=False):
        self._require_fused(x)
        tower, head, iden = self.folded()
        g = ops.pointmlp3_max(x, tower, True, blocked_bwd)    # relu(bn3(conv3)) then max == max then relu
        g = ops.linear_act(g, *head[0], "relu")
        g = ops.linear_act(g, *head[1], "relu")
        g = ops.linear_act(g, *head[2]) + iden
        return g.view(-1, 3, 3)


class STNkd(_FrozenFusedMixin, nn.Module):
    """Feature transform net (model/pointnet.py:51-87). It has no forward of its own here: its tower recomputes the
    trunk's first layer from the points, so it only runs inside PointNetfeat (ops.pointnet_ft_feat_fwd)."""

    def __init__(self, k=64):
        super(STNkd, self).__init__()
        if k != 64:
            raise NotImplementedError("STNkd: only k=64 (the PointNetfeat feature transform) is implemented on MI355X")
        self.conv1 = torch.nn.Conv1d(k, 64, 1)
        self.conv2 = torch.nn.Conv1d(64, 128, 1)
        self.conv3 = torch.nn.Conv1d(128, 1024, 1)
        self.fc1 = nn.Linear(1024, 512)
        self.fc2 = nn.Linear(512, 256)
        self.fc3 = nn.Linear(256, k * k)
        self.relu = nn.ReLU()

        self.bn1 = nn.BatchNorm1d(64)
        self.bn2 = nn.BatchNorm1d(128)
        self.bn3 = nn.BatchNorm1d(1024)
        self.bn4 = nn.BatchNorm1d(512)
        self.bn5 = nn.BatchNorm1d(256)

        self.k = k
        self._folded_cache = None

    def _fold(self):
        WA, bA = _fold_bn(self.conv1.weight, self.conv1.bias, self.bn1)
        W2, b2 = _fold_bn(self.conv2.weight, self.conv2.bias, self.bn2)
        W3, b3 = _fold_bn(self.conv3.weight, self.conv3.bias, self.bn3)
        w1, b1 = _fold_bn(self.fc1.weight, self.fc1.bias, self.bn4)
        w2, b2h = _fold_bn(self.fc2.weight, self.fc2.bias, self.bn5)
        w3, b3h = _plain(self.fc3.weight, self.fc3.bias)
        iden = torch.eye(self.k, dtype=torch.float32, device=w3.device).reshape(-1)
        return dict(WA=WA, bA=bA, W2=W2, b2=b2, W3=W3, b3=b3,
                    head=((w1, b1), (w2, b2h), (w3, (b3h + iden).contiguous())),    # + identity (:82-86)
                    head_t=(_t(w1), _t(w2), _t(w3)))

    def forward(self, x):
        raise NotImplementedError("STNkd runs inside PointNetfeat(feature_transform=True) only: its fused tower starts "
                                  "from the points, not from a [B,64,N] activation")


class PointNetfeat(_FrozenFusedMixin, nn.Module):
    """Global feature trunk (model/pointnet.py:89-128), global_feat=True. With feature_transform=True, forward returns
    trans_feat [B,64,64] DETACHED: the gradient that reaches x through the transform's use inside the trunk is
    complete, but a loss term on the returned trans_feat itself (the training regulariser) gets no gradient."""

    def __init__(self, global_feat=True, feature_transform=False):
        super(PointNetfeat, self).__init__()
        self.stn = STN3d()
        self.conv1 = torch.nn.Conv1d(3, 64, 1)
        self.conv2 = torch.nn.Conv1d(64, 128, 1)
        self.conv3 = torch.nn.Conv1d(128, 1024, 1)
        self.bn1 = nn.BatchNorm1d(64)
        self.bn2 = nn.BatchNorm1d(128)
        self.bn3 = nn.BatchNorm1d(1024)
        self.global_feat = global_feat
        self.feature_transform = feature_transform
        if not self.global_feat:
            raise NotImplementedError(
                "PointNetfeat: global_feat=False (the PointNetDenseCls segmentation trunk) is not on the attack path "
                "(every attack driver builds PointNetCls: attack/CW/Eval_CW.py:97)")
        if self.feature_transform:
            self.fstn = STNkd(k=64)
        self._folded_cache = None

    def _fold(self):
        tower = _fold_bn(self.conv1.weight, self.conv1.bias, self.bn1) + \
            _fold_bn(self.conv2.weight, self.conv2.bias, self.bn2) + \
            _fold_bn(self.conv3.weight, self.conv3.bias, self.bn3)
        # W2^T for the backward kernel, and an empty list that ops.pointmlp3_max_fwd_raw fills once, on its first launch,
        # with the prepared image of this W3 (nothing is launched here). A plain list on purpose: graphed._cached_tensors
        # walks tuples, lists and dicts, which is what keeps the image alive next to a captured graph after a re-fold.
        return tower + (tower[2].t().contiguous(), [])

    def forward(self, x):
        self._require_fused(x)
        trans = self.stn(x, blocked_bwd=self.feature_transform)
        if self.feature_transform:
            g, trans_feat = ops.pointnet_ft_feat(x, trans, self.folded(), self.fstn.folded())
            return g, trans, trans_feat
        xt = torch.bmm(x.transpose(2, 1), trans).transpose(2, 1)   # [B,3,N] strided view; kernel takes strides
        g = ops.pointmlp3_max(xt, self.folded(), False)            # bn3(conv3) has no ReLU (:121)
        return g, trans, None


class PointNetCls(_FrozenFusedMixin, nn.Module):
    """model/pointnet.py:130-148 — returns (log_softmax logits [B,k], trans [B,3,3], trans_feat): None, or with
    feature_transform=True the [B,64,64] feature transform, detached (see PointNetfeat)."""
    deterministic_forward = True   # forward is a pure function of its input (no RNG): attack loops may share it
    # Copies of a cloud's point 0 appended behind the cloud change neither the logits nor the gradient of the other rows,
    # and receive a gradient of exactly zero: every pooled value is a max over points whose ties go to the lowest index
    # (csrc/pointmlp.hip). Both variants; CW.attack(data, target, lengths) asks for it. Nothing else declares it.
    pad_invariant = True

    def __init__(self, k=2, feature_transform=False):
        super(PointNetCls, self).__init__()
        self.feature_transform = feature_transform
        # the 15-launch riders iteration exists for the two-tower victim only; attack loops ask the instance
        self.has_fused_attack_update = not feature_transform
        # the fused passes take per-cloud lengths (fused_forward(..., lengths=)): the two-tower victim's tower kernels
        # have ragged twins, the feature-transform victim's (csrc/pointmlp_ft.hip) do not and keep the padded pass
        self.fused_lengths = not feature_transform
        self.feat = PointNetfeat(global_feat=True, feature_transform=feature_transform)
        self.fc1 = nn.Linear(1024, 512)
        self.fc2 = nn.Linear(512, 256)
        self.fc3 = nn.Linear(256, k)
        self.dropout = nn.Dropout(p=0.3)
        self.bn1 = nn.BatchNorm1d(512)
        self.bn2 = nn.BatchNorm1d(256)
        self.relu = nn.ReLU()
        self._folded_cache = None

    def _fold(self):
        return (_fold_bn(self.fc1.weight, self.fc1.bias, self.bn1),
                _fold_bn(self.fc2.weight, self.fc2.bias, self.bn2),   # dropout is identity in eval
                _plain(self.fc3.weight, self.fc3.bias))

    def fused_loss_and_grad(self, x, target, kind, kappa=0.0, scale=None, lengths=None):
        """Attack fast path (no autograd): (logp [B,k], pred [B], per-sample adv loss [B], d mean(loss)/dx).
        kind in ops.LOSS_KINDS. Numerically the same computation as forward() + autograd, in ~20 launches.
        lengths: see fused_forward; the gradient rows behind a cloud's length are zero."""
        logits, ctx = fused_forward(self, x, lengths=lengths)
        logp, pred, loss, g_logits = ops.cls_loss(logits, target, kind, kappa,
                                                  scale=1.0 / x.shape[0] if scale is None else scale)
        return logp, pred, loss, fused_input_grad(ctx, g_logits)

    def fused_attack_grad(self, x, target, kind, kappa=0.0, pred_out=None, step=None, scale=None, lengths=None):
        """fused_loss_and_grad for the attack loops: the classifier tail (fc3, loss, fc3 backward) is one launch that
        also writes the prediction into `pred_out` and advances the device step word. Returns (pred, loss, dL/dx)."""
        _, ctx = fused_forward(self, x, tail=False, lengths=lengths)
        c2, pk = ctx[9], ctx[1]
        _, pred, loss, g_c2 = ops.cls_tail(c2, pk["c"][4], pk["c"][5], target, kind, kappa,
                                           scale=1.0 / x.shape[0] if scale is None else scale,
                                           pred_out=pred_out, step=step, want_logp=False)
        return pred, loss, fused_input_grad(ctx, None, g_c2=g_c2)

    def fused_attack_update(self, x, target, kind, kappa=0.0, pred_out=None, step=None, scale=None, cw=None,
                            ride_search=True, epilogue=True):
        """A whole CW iteration on the iterate x ([B,3,N], updated IN PLACE) in 15 launches, one chain: fused_attack_grad's
        victim passes with the attack's independent pieces carried by launches that exist anyway —
          * the adv -> ori search (Chamfer) rides the STN head's first linear launch (ops.linear_nn);
          * the bookkeeping (||adv-ori||, best-distance decisions, input_val / o_bestattack copies) and Adam's two
            bias-correction factors ride the first launch after the classifier tail (ops.linear_book);
          * distance gradient + Adam + clip are the epilogue of the last backward launch (ops.pointmlp3_max_bwd_update).
        The same bits as fused_attack_grad + ops.nn_raw + ops.cw_update. cw: the loop's state — ori, label, untarget,
        bestdist, bestscore, o_bestdist, o_bestscore, o_bestattack, input_val, dist_val, m, v, w, adam (float32 [2]), lr,
        budget, dist_kind. ride_search / epilogue = False give that piece its own launch again (A/B switches). Returns pred."""
        self._require_fused(x)
        if self.feature_transform:
            raise NotImplementedError("PointNetCls.fused_attack_update: the riders iteration is not built for a "
                                      "feature-transform victim (has_fused_attack_update is False); use fused_attack_grad")
        pk = fused_pack(self)
        w1s, b1s, w2s, b2s, w3s, b3s = pk["s"]
        w1c, b1c, w2c, b2c, w3c, b3c = pk["c"]
        w1c_t, w2c_t, w3c_t = pk["c_t"]
        w1s_t, w2s_t, w3s_t = pk["s_t"]
        dk, ori = cw["dist_kind"], cw["ori"]
        pooled_s, idx_s, masks_s = ops.pointmlp3_max_fwd_raw(x, pk["tower_s"], True, want_masks=True)
        nn_idx = None
        if dk == 2:
            a1, _, nn_idx = ops.linear_nn(pooled_s, w1s, b1s, relu=True, q=x, r=ori, q_cf=True, r_cf=True, ride=ride_search)
        else:
            a1 = ops.linear(pooled_s, w1s, b1s, relu=True)
        a2 = ops.linear(a1, w2s, b2s, relu=True)
        pooled, idx, masks, trans = ops.pointmlp3_max_fwd_raw(x, pk["tower_c"], False, want_masks=True, T_head=(a2, w3s, b3s))
        c1 = ops.linear(pooled, w1c, b1c, relu=True)
        c2 = ops.linear(c1, w2c, b2c, relu=True)
        _, pred, _, g_c2 = ops.cls_tail(c2, w3c, b3c, target, kind, kappa, scale=1.0 / x.shape[0] if scale is None else scale,
                                        pred_out=pred_out, step=step, want_logp=False)
        if epilogue:
            g_c1 = ops.linear_book(g_c2, w2c_t, x, ori, pred, cw["label"], cw["untarget"], cw["bestdist"], cw["bestscore"],
                                   cw["o_bestdist"], cw["o_bestscore"], cw["o_bestattack"], gate=c1,
                                   input_val=cw["input_val"], dist_val=cw["dist_val"], step=step, lr=cw["lr"], adam=cw["adam"])
        else:
            g_c1 = ops.linear(g_c2, w2c_t, gate=c1)
        g_pooled = ops.linear(g_c1, w1c_t)
        gx, part_gT = ops.pointmlp3_max_bwd_raw(x, pk["tower_c"], idx, g_pooled, masks, T=trans, want_gT=True)
        g_a1 = ops.linear_pre(part_gT, 9, pk["s"][4], a2, w2s_t, gate=a1)
        g_pooled_s = ops.linear(g_a1, w1s_t, gate=pooled_s)
        if epilogue:
            ops.pointmlp3_max_bwd_update(x, pk["tower_s"], idx_s, g_pooled_s, masks_s, gx, ori, cw["m"], cw["v"], cw["adam"],
                                         cw["budget"], dist_kind=dk, w=cw["w"], dist_val=cw["dist_val"], nn_idx=nn_idx)
        else:
            ops.pointmlp3_max_bwd_raw(x, pk["tower_s"], idx_s, g_pooled_s, masks_s, out=gx, accumulate=True)
            ops.cw_update(x, ori, pred, cw["label"], cw["untarget"], cw["bestdist"], cw["bestscore"], cw["o_bestdist"],
                          cw["o_bestscore"], cw["o_bestattack"], gx, cw["m"], cw["v"], step, cw["lr"], cw["budget"],
                          input_val=cw["input_val"], dist_val=cw["dist_val"], dist_kind=dk, w=cw["w"], nn_idx=nn_idx)
        return pred

    def forward(self, x):
        self._require_fused(x)
        head = self.folded()
        g, trans, trans_feat = self.feat(x)
        g = ops.linear_act(g, *head[0], "relu")
        g = ops.linear_act(g, *head[1], "relu")
        g = ops.linear_act(g, *head[2])
        return F.log_softmax(g, dim=1), trans, trans_feat


def _t(w):
    return w.t().contiguous()


def _fused_sources(model):
    src = model.feat.stn.folded(), model.feat.folded(), model.folded()
    return src + (model.feat.fstn.folded(),) if model.feature_transform else src


def fused_pack(model):
    """The launch-minimal path's weight pack, rebuilt when any of the folded caches it was built from was re-folded.
    Callers that bake its pointers into a hipGraph keep the returned dict alive next to the graph."""
    if not isinstance(model, PointNetCls) and hasattr(model, "fused_pack"):
        return model.fused_pack()          # a wrapper around a PointNetCls (defense.FusedDefended): the inner victim's pack
    pk = model.__dict__.get("_fused_cache")
    if pk is None or any(a is not b for a, b in zip(pk["src"], _fused_sources(model))):
        pk = _fused_pack(model)
        object.__setattr__(model, "_fused_cache", pk)
    return pk


def _fused_pack(model):
    """Everything the launch-minimal path needs, built once from the folded weights: heads as (W, b) plus the
    transposed copies the backward launches read (weights are frozen, so W^T is a constant)."""
    src = _fused_sources(model)
    (tower_s, head_s, iden), tower_c, head_c = src[:3]
    (w1s, b1s), (w2s, b2s), (w3s, b3s) = head_s
    (w1c, b1c), (w2c, b2c), (w3c, b3c) = head_c
    w3s_t = torch.zeros((w3s.shape[1], 16), dtype=torch.float32, device=w3s.device)   # [256,16], 9 used
    w3s_t[:, :9] = w3s.t()
    return dict(src=src, tower_s=tower_s, tower_c=tower_c, fstn=src[3] if len(src) > 3 else None,
                s=(w1s, b1s, w2s, b2s, w3s, (b3s + iden.view(-1)).contiguous()),
                c=(w1c, b1c, w2c, b2c, w3c, b3c),
                s_t=(_t(w1s), _t(w2s), w3s_t.contiguous()), c_t=(_t(w1c), _t(w2c), _t(w3c)))


class _LengthsCtx(tuple):
    """fused_forward's ctx of a pass that was given lengths: the same twelve items, the lengths as an attribute."""
    lengths = None


def fused_forward(model, x, tail=True, lengths=None):
    """Launch-minimal forward of PointNetCls: 2 tower launches (+2 folds) + 5 head launches, no autograd graph.
    Returns (logits [B,k] PRE-softmax, ctx) — ctx feeds fused_input_grad.
    A feature-transform victim: 3 tower launches (+3 folds), the W2 fold, 9 head launches; ctx has a 13th item.
    A model that is not a PointNetCls but brings its own ``fused_forward`` (defense.FusedDefended) runs that one.
    lengths: None, or an int32 [B] device tensor — cloud b has lengths[b] points and both towers (and, through the ctx,
    both tower backwards) run their ragged launches: the rows behind a length are never read, the logits are those of the
    batch padded with copies of point 0, the gradient rows behind a length are zero. For a victim that declares
    fused_lengths only (the two-tower one); any other raises."""
    if lengths is not None and not (isinstance(model, PointNetCls) and model.fused_lengths):
        raise ValueError("fused_forward: lengths need a victim that declares fused_lengths (PointNetCls without the "
                         "feature transform); run the padded pass")
    if not isinstance(model, PointNetCls) and hasattr(model, "fused_forward"):
        return model.fused_forward(x, tail)
    model._require_fused(x)
    pk = fused_pack(model)
    w1s, b1s, w2s, b2s, w3s, b3s = pk["s"]
    w1c, b1c, w2c, b2c, w3c, b3c = pk["c"]
    pooled_s, idx_s, masks_s = ops.pointmlp3_max_fwd_raw(x, pk["tower_s"], True, want_masks=True, lengths=lengths)
    a1 = ops.linear(pooled_s, w1s, b1s, relu=True)
    a2 = ops.linear(a1, w2s, b2s, relu=True)
    ft = None
    if pk["fstn"] is not None:
        trans = ops.linear(a2, w3s, b3s)             # two towers read the transform: it gets a launch of its own
        pooled, _, ft = ops.pointnet_ft_feat_fwd(x, trans, pk["tower_c"], pk["fstn"])
        idx = masks = None
    else:
        # the transform (STN fc3 + identity, [B,9]) is computed in the trunk tower's prologue: no launch of its own
        pooled, idx, masks, trans = ops.pointmlp3_max_fwd_raw(x, pk["tower_c"], False, want_masks=True, T_head=(a2, w3s, b3s),
                                                              lengths=lengths)
    c1 = ops.linear(pooled, w1c, b1c, relu=True)
    c2 = ops.linear(c1, w2c, b2c, relu=True)
    logits = ops.linear(c2, w3c, b3c) if tail else None
    ctx = (x, pk, pooled_s, idx_s, a1, a2, trans, idx, c1, c2, masks_s, masks)
    if lengths is not None:
        ctx = _LengthsCtx(ctx)
        ctx.lengths = lengths
    return logits, ctx if ft is None else ctx + (ft,)


def fused_input_grad(ctx, g_logits, out=None, g_c2=None):
    """Backward-to-input of fused_forward for an upstream gradient on the logits: 5 head launches + 2 tower launches.
    A ctx that brings its own ``fused_input_grad`` (defense.FusedDefended's) runs that one."""
    if hasattr(ctx, "fused_input_grad"):
        return ctx.fused_input_grad(g_logits, out=out, g_c2=g_c2)
    x, pk, pooled_s, idx_s, a1, a2, trans, idx, c1, c2, masks_s, masks = ctx[:12]
    lengths = getattr(ctx, "lengths", None)   # a pass that was given lengths (the two-tower victim only)
    w1c_t, w2c_t, w3c_t = pk["c_t"]
    w1s_t, w2s_t, w3s_t = pk["s_t"]
    if g_c2 is None:
        g_c2 = ops.linear(g_logits, w3c_t, gate=c2)
    g_c1 = ops.linear(g_c2, w2c_t, gate=c1)
    g_pooled = ops.linear(g_c1, w1c_t)
    if len(ctx) > 12:   # feature transform: trunk, dL/dTf, STNkd head and tower; both towers' dL/dT partials in part_gT
        gx, part_gT = ops.pointnet_ft_feat_bwd(ctx[12], g_pooled, out=out)
    else:
        gx, part_gT = ops.pointmlp3_max_bwd_raw(x, pk["tower_c"], idx, g_pooled, masks, T=trans, want_gT=True, out=out,
                                                lengths=lengths)
    # fc3's backward (dL/dT partials summed, 9 -> 256, ReLU mask of a2) runs inside the launch of fc2's backward
    g_a1 = ops.linear_pre(part_gT, 9, pk["s"][4], a2, w2s_t, gate=a1)
    g_pooled_s = ops.linear(g_a1, w1s_t, gate=pooled_s)                 # ReLU after the STN max-pool
    if len(ctx) > 12:   # all three towers of this victim sum a point's channels in blocks
        ts = pk["tower_s"]
        ops.pointnet_ft_tower_bwd_raw(x, None, ts[0], ts[2], ts[4], idx_s, g_pooled_s, masks_s, None, 0, out=gx, accumulate=True)
    else:
        ops.pointmlp3_max_bwd_raw(x, pk["tower_s"], idx_s, g_pooled_s, masks_s, out=gx, accumulate=True, lengths=lengths)
    return gx


def feature_transform_regularizer(trans):
    """model/pointnet.py:178-185."""
    d = trans.size()[1]
    I = torch.eye(d, device=trans.device)[None, :, :]
    return torch.mean(torch.norm(torch.bmm(trans, trans.transpose(2, 1)) - I, dim=(1, 2)))
