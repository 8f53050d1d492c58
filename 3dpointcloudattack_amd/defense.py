"""Pre-processing defences in front of a victim — MI355X mirrors of the reference's point-dropping heads
(attack/SIadv/baselines/defense/drop_points/SOR.py, SRS.py; used there as ``classifier(pre_head(points))``,
attack/SIadv/SIadv_attack.py:189-202).

``SORDefense`` (statistical outlier removal) and ``SRSDefense`` (simple random sampling) keep the reference's class
names, constructor arguments, defaults and tensor layouts ([B,3,K] in, [B,3,npoint] / [B,3,K-drop_num] out). What
changes is where the work happens: the reference's SOR builds a [B,K,K] float64 matrix, calls ``.item()`` on it and
assembles its output with a Python loop over the batch; its SRS draws on the host one cloud at a time and uploads B index
tensors. Here SOR is the self-kNN search plus ONE launch (pc3d_sor_select_f32: statistics, mask, ordered compaction,
padding, gather) with a gather-form backward (pc3d_sor_bwd_f32), has a fixed output shape and never touches the host, so
a defended victim runs inside an attack loop and inside ``torch.cuda.graph``.

``DUPNet`` (SOR followed by the PU-Net upsampler, attack/SIadv/baselines/defense/DUP_Net) is exported from here too; it lives
under the reference's import path.

``Defended(model, head)`` is the composition as an ``nn.Module`` (any model, any head, autograd);
``FusedDefended(model, head)`` is a PointNet victim behind SOR that keeps the fused entry points, so the device-side
attack loops run on it; ``evaluate_defended`` is the after-the-attack table row. There is no CPU fallback: tensors must
live on the GPU.

Deviation from the reference (SOR): ``K > npoint`` raises ``ValueError`` from the shapes alone. The reference's
``process_data`` only survives that case when the number of kept points happens to be <= npoint (it asserts otherwise),
which depends on the data; a head whose output shape may not depend on the data cannot offer that.
"""
import numpy as np
import torch
import torch.nn as nn

from . import _lib
from . import graphed as _graphed
from . import ops

# Search + select as two launches (False) or one fused per-cloud launch (True). Measured on MI355X (tools/bench_defense.py,
# profiles/defense_bench.json): the fused form puts one workgroup on each of B compute units while the search
# of the two-launch form fills the chip, and loses from K = 1024 up at B = 32.
SOR_FUSED = False
# The search FusedDefended puts in front of pc3d_sor_select_f32: the list-per-lane kernel (pc3d_knn_small_f32, True; k <= 8)
# or the wave-per-query kernel of ops.knn_raw (False). The same bits either way. Measured on MI355X
# (tools/bench_fused_defended.py, profiles/fused_defended_bench.json): 9.3 against 21.3 us at B = 32,
# K = 1024, k1 = 3, run-to-run spread 0.08 us; faster at K = 2048 / 4096 and at k1 = 9 too.
SOR_SMALL_SEARCH = True
SOR_SMALL_MAX_K = 8
SOR_FUSED_MAX_POINTS = 4096
SOR_MAX_POINTS = 8192
SRS_DEVICE_MAX_POINTS = 4096


def _sor_shapes(K, k, npoint):
    if k < 1:
        raise ValueError(f"SORDefense: k={k} must be >= 1")
    if K < k + 1:
        raise ValueError(f"SORDefense: a cloud of K={K} points has no k={k} neighbours per point (K >= k + 1)")
    if K > npoint:
        raise ValueError(f"SORDefense: K={K} points exceed npoint={npoint}; the output holds every kept point, so "
                         "npoint >= K is required (the reference asserts when more than npoint points are kept)")
    if K > SOR_MAX_POINTS:
        raise ValueError(f"SORDefense: K={K} exceeds the limit of {SOR_MAX_POINTS} points")
    if k + 1 > 64:
        raise ValueError(f"SORDefense: k={k} exceeds the search's limit of 63 neighbours")


def sor_select(x, k=2, alpha=1.1, npoint=1024, cf=True, fused=None, want_stats=False, search=None):
    """SOR forward without autograd on x [B,3,K] (cf) or [B,K,3]: dict(out (same layout as x, npoint points), count [B]
    int32, rank [B,K] int32, src [B,npoint] int32) and with want_stats also v [B,K], thr [B] (fp32 copies of the fp64
    values the mask was taken with). search (two-launch form only): None / "knn" = ops.knn_raw, "small" = the values-only
    list-per-lane search ops.knn_small_dists (k <= 8) — the same distance bits, hence the same selection."""
    p, bs, ps, cs, B, K = ops._pts(x, cf, "x")
    _sor_shapes(K, int(k), int(npoint))
    k1 = int(k) + 1
    fused = SOR_FUSED if fused is None else bool(fused)
    if search not in (None, "knn", "small"):
        raise ValueError(f"sor_select: search={search!r} is not one of None, 'knn', 'small'")
    if search == "small" and (fused or int(k) > SOR_SMALL_MAX_K):
        raise ValueError(f"sor_select: search='small' takes the two-launch form and k <= {SOR_SMALL_MAX_K} (k={k}, fused={fused})")
    if fused and (K > SOR_FUSED_MAX_POINTS or k1 > 9):
        raise ValueError(f"the fused SOR launch takes K <= {SOR_FUSED_MAX_POINTS} and k <= 8 (K={K}, k={k})")
    dev = x.device
    out = torch.empty((B, 3, npoint) if cf else (B, npoint, 3), dtype=torch.float32, device=dev)
    count = torch.empty((B,), dtype=torch.int32, device=dev)
    rank = torch.empty((B, K), dtype=torch.int32, device=dev)
    src = torch.empty((B, npoint), dtype=torch.int32, device=dev)
    v = torch.empty((B, K), dtype=torch.float32, device=dev) if want_stats else None
    thr = torch.empty((B,), dtype=torch.float32, device=dev) if want_stats else None
    op, obs, opst, ocs, _, _ = ops._pts(out, cf, "out")
    if fused:
        d = torch.empty((B, K, k1), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.call("pc3d_sor_fused_f32", p, bs, ps, cs, B, K, k1, float(alpha), int(npoint), d.data_ptr(), ops._ptr(v),
                      ops._ptr(thr), count.data_ptr(), rank.data_ptr(), src.data_ptr(), op, obs, opst, ocs, ops._stream())
    else:
        d = ops.knn_small_dists(x, x, k1, cf, cf) if search == "small" else ops.knn_raw(x, x, k1, cf, cf)[0]
        with torch.cuda.device(dev):
            _lib.call("pc3d_sor_select_f32", d.data_ptr(), p, bs, ps, cs, B, K, k1, float(alpha), int(npoint), ops._ptr(v),
                      ops._ptr(thr), count.data_ptr(), rank.data_ptr(), src.data_ptr(), op, obs, opst, ocs, ops._stream())
    res = dict(out=out, count=count, rank=rank, src=src)
    if want_stats:
        res.update(v=v, thr=thr)
    return res


def sor_backward(g, count, rank, cf=True, out=None):
    """grad_x of the SOR copies for upstream g (layout of the output): [B,3,K] (cf) or [B,K,3]; written into `out` if given."""
    gp, gbs, gps, gcs, B, npoint = ops._pts(g, cf, "grad_out")
    K = rank.shape[1]
    grad = torch.empty((B, 3, K) if cf else (B, K, 3), dtype=torch.float32, device=g.device) if out is None else out
    if tuple(grad.shape) != ((B, 3, K) if cf else (B, K, 3)):
        raise ValueError(f"sor_backward: out has shape {tuple(grad.shape)}, the input cloud's is {(B, 3, K) if cf else (B, K, 3)}")
    rp, rbs, rps, rcs, _, _ = ops._pts(grad, cf, "grad_x")
    with torch.cuda.device(g.device):
        _lib.call("pc3d_sor_bwd_f32", gp, gbs, gps, gcs, count.data_ptr(), rank.data_ptr(), B, K, npoint, rp, rbs, rps, rcs,
                  ops._stream())
    return grad


class _SorFn(torch.autograd.Function):
    """The mask is a constant; the gradient flows back to x through the copies."""

    @staticmethod
    def forward(ctx, x, k, alpha, npoint, fused, search=None):
        r = sor_select(x, k, alpha, npoint, cf=True, fused=fused, search=search)
        ctx.n_extra = 4 if search is None else 5         # one gradient slot per argument apply() was given
        ctx.save_for_backward(r["count"], r["rank"])
        ctx.mark_non_differentiable(r["count"], r["src"])
        ctx.set_materialize_grads(False)
        return r["out"], r["count"], r["src"]

    @staticmethod
    def backward(ctx, g, _gc, _gs):
        if g is None:
            return (None,) * (1 + ctx.n_extra)
        count, rank = ctx.saved_tensors
        if g.dtype != torch.float32:
            g = g.float()
        return (sor_backward(g, count, rank, cf=True),) + (None,) * ctx.n_extra


class SORDefense(nn.Module):
    """Statistical outlier removal as defense (SOR.py:7-84): same constructor, same [B,3,K] -> [B,3,npoint] forward."""

    def __init__(self, k=2, alpha=1.1, npoint=1024):
        super(SORDefense, self).__init__()
        self.k = k
        self.alpha = alpha
        self.npoint = npoint
        self.fused = None          # None: the module default SOR_FUSED

    def forward(self, x, return_info=False):
        """x [B,3,K] fp32 on the GPU. With return_info also count [B] (points kept) and src [B,npoint] (the input index
        every output point copies), both int32 on the device."""
        if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.shape[1] != 3:
            raise ValueError(f"SORDefense: expected a [B,3,K] tensor, got {tuple(getattr(x, 'shape', ()))}")
        _sor_shapes(x.shape[2], int(self.k), int(self.npoint))
        if x.dtype != torch.float32:
            x = x.float()
        out, count, src = _SorFn.apply(x, int(self.k), float(self.alpha), int(self.npoint), self.fused)
        return (out, count, src) if return_info else out


def gather_points(x, idx, cf=True):
    """out[b,:,j] = x[b,:,idx[b,j]] (cf) for an int32 index table idx [B,M] on the device; one launch."""
    p, bs, ps, cs, B, K = ops._pts(x, cf, "x")
    if idx.dtype != torch.int32 or not idx.is_cuda or idx.dim() != 2 or idx.shape[0] != B or not idx.is_contiguous():
        raise ValueError("gather_points: idx must be a contiguous int32 [B,M] tensor on the GPU")
    M = idx.shape[1]
    out = torch.empty((B, 3, M) if cf else (B, M, 3), dtype=torch.float32, device=x.device)
    op, obs, opst, ocs, _, _ = ops._pts(out, cf, "out")
    with torch.cuda.device(x.device):
        _lib.call("pc3d_gather_points_f32", p, bs, ps, cs, idx.data_ptr(), B, K, M, op, obs, opst, ocs, ops._stream())
    return out


def srs_select(seed, counter, B, K, M, device):
    """idx [B,M] int32: the device-side draw (pc3d_srs_select_i32). counter: a 1-element int32 GPU tensor or an int."""
    if not (1 <= M <= K <= SRS_DEVICE_MAX_POINTS):
        raise ValueError(f"srs_select: need 1 <= M <= K <= {SRS_DEVICE_MAX_POINTS} (K={K}, M={M})")
    idx = torch.empty((B, M), dtype=torch.int32, device=device)
    dev_ctr, host_ctr = (counter.data_ptr(), 0) if isinstance(counter, torch.Tensor) else (0, int(counter))
    with torch.cuda.device(device):
        _lib.call("pc3d_srs_select_i32", int(seed), dev_ctr, host_ctr, B, K, M, idx.data_ptr(), ops._stream())
    return idx


class SRSDefense(nn.Module):
    """Random dropping points as defense (SRS.py:8-39): [B,3,K] -> [B,3,K-drop_num], no gradient.

    Default (device_rng=False): the subsets are drawn exactly as the reference draws them — ``np.random.choice(K,
    K - drop_num, replace=False)`` per cloud in batch order from numpy's global stream, so the same ``np.random.seed``
    gives the same subsets — then ONE [B,K-drop_num] upload and one gather launch. The host draw makes this mode
    unfit for ``torch.cuda.graph`` capture (a replay would repeat the captured subset).
    device_rng=True: the draw runs on the device (pc3d_srs_select_i32) from (seed, a call counter that lives on the
    device, cloud, point); nothing touches the host, and consecutive replays of a captured graph draw different subsets.
    Run one forward (or move the module to the device) before capturing. seed=None takes ``torch.initial_seed()``."""

    def __init__(self, drop_num=500, device_rng=False, seed=None):
        super(SRSDefense, self).__init__()
        self.drop_num = drop_num
        self.device_rng = device_rng
        self.seed = seed
        self.register_buffer("calls", torch.zeros((1,), dtype=torch.int32), persistent=False)

    def draw_host(self, B, K):
        """The reference's draws (SRS.py:30): [B,K-drop_num] indices from numpy's global stream."""
        if not 0 <= self.drop_num < K:
            raise ValueError(f"SRSDefense: drop_num={self.drop_num} leaves nothing of K={K} points")
        return np.stack([np.random.choice(K, K - self.drop_num, replace=False) for _ in range(B)])

    def random_drop_index(self, B, K, device):
        """idx [B,K-drop_num] int32 on the device for the next forward."""
        if not self.device_rng:
            return torch.from_numpy(self.draw_host(B, K).astype(np.int32)).to(device)
        if not 0 <= self.drop_num < K:
            raise ValueError(f"SRSDefense: drop_num={self.drop_num} leaves nothing of K={K} points")
        if self.calls.device != device:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("SRSDefense(device_rng=True): move the module to the device before capturing")
            self.calls = self.calls.to(device)
        if self.seed is None:
            self.seed = int(torch.initial_seed()) & 0x7FFFFFFFFFFFFFFF
        idx = srs_select(self.seed, self.calls, B, K, K - self.drop_num, device)
        ops.i32_add(self.calls, 1)
        return idx

    def forward(self, x):
        if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.shape[1] != 3:
            raise ValueError(f"SRSDefense: expected a [B,3,K] tensor, got {tuple(getattr(x, 'shape', ()))}")
        with torch.no_grad():
            x = x.detach()
            ops._check(x, "x")
            idx = self.random_drop_index(x.shape[0], x.shape[2], x.device)
            return gather_points(x, idx, cf=True)


class Defended(nn.Module):
    """``model`` behind a pre-processing head: forward(x) = model(head(x)), returning what the model returns (the victims'
    3-tuple). Accepted wherever the attack classes take ``model`` / ``trans_model``: it declares no deterministic forward
    and no fused entry points, so ``graphed.wrap`` leaves the composition eager and the attacks differentiate it through
    autograd (SORDefense passes the gradient to the kept points). The victim BEHIND the head is still a pure function of
    the head's output: with graph=True (default) its forward / backward replay from hipGraphs when it declares a
    deterministic forward (``graphed.wrap``; graph=None takes the victim's own default, False launches it eagerly).
    With an SRSDefense in host mode the composition as a whole cannot be captured into a hipGraph (the draw happens on
    the host)."""

    def __init__(self, model, head, graph=True):
        super().__init__()
        self.model = model
        self.head = head
        self.graph = graph

    def forward(self, x):
        return _graphed.wrap(self.model, enable=self.graph)(self.head(x))


class _DefendedCtx:
    """What FusedDefended.fused_forward hands to fused_input_grad: the inner victim's ctx and SOR's (count, rank)."""
    __slots__ = ("inner", "count", "rank")

    def __init__(self, inner, count, rank):
        self.inner, self.count, self.rank = inner, count, rank

    def fused_input_grad(self, g_logits, out=None, g_c2=None):
        from .model import pointnet as _pointnet
        g = _pointnet.fused_input_grad(self.inner, g_logits, g_c2=g_c2)
        return sor_backward(g, self.count, self.rank, cf=True, out=out)


class FusedDefended(nn.Module):
    """``PointNetCls`` behind a ``SORDefense`` WITH the fused entry points the device-side attack loops ask for, so a
    defended victim runs inside them (CW, the additional-experiments CW, kNN, SI-Adv's white-box loop, AOF, CWTAOF, ISO,
    CWAdd / CWAddClusters) instead of on their autograd paths. ``Defended`` stays the general composition (any model, any
    head, autograd); this class is the one pair with fixed shapes and no host round trip on both sides.

    model: a ``PointNetCls`` (plain or feature_transform=True; a GraphedVictim around one is unwrapped). head: a
    ``SORDefense``. Anything else raises TypeError: SRSDefense (a fresh draw per forward) and DUPNet (the upsampler's
    backward) are out of scope. The head's k, alpha and npoint are read ONCE, here, and are read-only afterwards (a
    captured loop bakes them in); they also sit in a non-persistent buffer, so ``graphed.weights_key`` tells two wrappers
    of one model apart while ``state_dict()`` is the inner model's.

    Every fused call is four steps — the search, pc3d_sor_select_f32, the inner victim's fused call on the [B,3,npoint]
    output, pc3d_sor_bwd_f32 — without a host sync and with every allocation from torch's pool, so it captures into a
    hipGraph. The mask is a constant of the backward, as in ``_SorFn``: the gradient is exactly zero on dropped points.
    ``forward`` is the differentiable composition, bit-equal to ``Defended(model, head)(x)``."""
    deterministic_forward = True
    has_fused_attack_update = False      # no riders iteration: CW takes fused_attack_grad + one update launch

    def __init__(self, model, head):
        super().__init__()
        from .model import pointnet as _pointnet
        model = _graphed.unwrap(model)
        if not isinstance(model, _pointnet.PointNetCls):
            raise TypeError(f"FusedDefended: model must be a PointNetCls (plain or feature_transform=True), got "
                            f"{type(model).__name__}; use Defended for any other victim")
        if not isinstance(head, SORDefense):
            raise TypeError(f"FusedDefended: head must be a SORDefense, got {type(head).__name__}; SRSDefense and DUPNet "
                            "heads run behind Defended (autograd path)")
        k, alpha, npoint = int(head.k), float(head.alpha), int(head.npoint)
        if not 1 <= k <= 63:
            raise ValueError(f"FusedDefended: k={k} out of range [1, 63]")
        self.model = model
        object.__setattr__(self, "_settings", (k, alpha, npoint))
        self.register_buffer("sor_settings", torch.tensor([k, alpha, npoint], dtype=torch.float64), persistent=False)
        self.train(model.training)

    k = property(lambda self: self._settings[0])
    alpha = property(lambda self: self._settings[1])
    npoint = property(lambda self: self._settings[2])

    def state_dict(self, *a, **kw):
        return self.model.state_dict(*a, **kw)

    def load_state_dict(self, *a, **kw):
        return self.model.load_state_dict(*a, **kw)

    def _require_fused(self, x):
        self.model._require_fused(x)

    def _search(self):
        return "small" if SOR_SMALL_SEARCH and self.k <= SOR_SMALL_MAX_K else None

    def _select(self, x):
        self._require_fused(x)
        if x.dim() != 3 or x.shape[1] != 3:
            raise ValueError(f"FusedDefended: expected a [B,3,K] tensor, got {tuple(x.shape)}")
        k, alpha, npoint = self._settings
        return sor_select(x, k, alpha, npoint, cf=True, fused=False, search=self._search())

    def fused_pack(self):
        """The inner victim's weight pack (what a loop compares to tell whether the weights it captured are current)."""
        from .model import pointnet as _pointnet
        return _pointnet.fused_pack(self.model)

    def forward(self, x):
        self._require_fused(x)
        if x.dim() != 3 or x.shape[1] != 3:
            raise ValueError(f"FusedDefended: expected a [B,3,K] tensor, got {tuple(x.shape)}")
        if x.dtype != torch.float32:
            x = x.float()
        k, alpha, npoint = self._settings
        out, _, _ = _SorFn.apply(x, k, alpha, npoint, False, self._search() or "knn")
        return self.model(out)

    def fused_forward(self, x, tail=True):
        """(logits [B,classes] PRE-softmax or None, ctx) of the defended victim; ctx feeds fused_input_grad."""
        from .model import pointnet as _pointnet
        sel = self._select(x)
        logits, inner = _pointnet.fused_forward(self.model, sel["out"], tail)
        return logits, _DefendedCtx(inner, sel["count"], sel["rank"])

    def fused_input_grad(self, ctx, g_logits, out=None, g_c2=None):
        """dL/dx [B,3,K] for an upstream gradient on the logits (or on the last hidden layer, g_c2)."""
        return ctx.fused_input_grad(g_logits, out=out, g_c2=g_c2)

    def fused_loss_and_grad(self, x, target, kind, kappa=0.0, scale=None):
        """PointNetCls.fused_loss_and_grad of the defended victim: (logp, pred, loss, dL/dx [B,3,K])."""
        sel = self._select(x)
        logp, pred, loss, g = self.model.fused_loss_and_grad(sel["out"], target, kind, kappa,
                                                             scale=1.0 / x.shape[0] if scale is None else scale)
        return logp, pred, loss, sor_backward(g, sel["count"], sel["rank"], cf=True)

    def fused_attack_grad(self, x, target, kind, kappa=0.0, pred_out=None, step=None, scale=None):
        """PointNetCls.fused_attack_grad of the defended victim: (pred, loss, dL/dx [B,3,K])."""
        sel = self._select(x)
        pred, loss, g = self.model.fused_attack_grad(sel["out"], target, kind, kappa, pred_out=pred_out, step=step,
                                                     scale=1.0 / x.shape[0] if scale is None else scale)
        return pred, loss, sor_backward(g, sel["count"], sel["rank"], cf=True)


def evaluate_defended(model, head, clouds, labels, batch=32):
    """Predictions of the defended victim on finished (adversarial) clouds: clouds [B,K,3] or [B,3,K] (tensor or
    array), labels [B]. Runs on the model's device in chunks of `batch`, ONE device-to-host copy at the end. Returns
    dict(pred [B] int64, correct [B] bool — pred == label —, count: how many are correct)."""
    clouds = torch.as_tensor(clouds)
    labels = torch.as_tensor(labels).long().view(-1)
    if clouds.dim() != 3 or 3 not in clouds.shape[1:]:
        raise ValueError(f"evaluate_defended: expected [B,K,3] or [B,3,K] clouds, got {tuple(clouds.shape)}")
    if clouds.shape[0] != labels.shape[0]:
        raise ValueError("evaluate_defended: one label per cloud")
    if clouds.shape[2] == 3 and clouds.shape[1] != 3:
        clouds = clouds.transpose(1, 2)
    p = next(iter(model.parameters()), None)
    dev = p.device if p is not None else torch.device("cuda", torch.cuda.current_device())
    net = Defended(model, head, graph=False).to(dev).eval()     # chunks of any size, each seen once: nothing to replay
    labels = labels.to(dev)
    res = torch.empty((2, clouds.shape[0]), dtype=torch.int64, device=dev)
    with torch.no_grad():
        for s in range(0, clouds.shape[0], int(batch)):
            x = clouds[s:s + int(batch)].to(dev).float().contiguous()
            out = net(x)
            pred = (out[0] if isinstance(out, tuple) else out).argmax(dim=1)
            res[0, s:s + pred.shape[0]] = pred
            res[1, s:s + pred.shape[0]] = (pred == labels[s:s + pred.shape[0]]).long()
    host = res.cpu().numpy()
    return dict(pred=host[0], correct=host[1].astype(bool), count=int(host[1].sum()))


def __getattr__(name):
    """``DUPNet`` / ``PUNet`` (the third head: SOR + the PU-Net upsampler) live under the reference's import path,
    attack/SIadv/baselines/defense/DUP_Net, which imports SORDefense from here: resolved on first use."""
    if name in ("DUPNet", "PUNet", "load_punet_weights"):
        from .attack.SIadv.baselines.defense.DUP_Net import DUP_Net as _dup
        return getattr(_dup, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
