"""kNN attack (AAAI'20) — MI355X mirror of attack/KNN/KNN_attack.py: one long Adam run (no binary search) with a
Chamfer (+ optional kNN-distance) regulariser and inner-point projection + per-point clip.

Same constructor / ``attack(data, target)`` signature and return values (attack/KNN/KNN_attack.py:19-20,56,244-246).
The loop (:99-141) runs on the device without host synchronisation: the per-iteration ``.item()`` success count
(:113-115) is dropped from the loop (it only fed a discarded local), Adam + ProjectInnerClipLinf are ONE HIP launch
when the clip functor is this package's own, and the regularisers are the fused NN / kNN kernels. B > 1 works; the
transfer / fail counters are sums over the batch. Transfer models may be ``None`` (skipped).

``device_loop=True`` (PointNet victims, see ``CWKNN._device_loop_plan``): the iteration is the victim's launch-minimal
passes, the two searches and ONE update launch (pc3d_knn_attack_update_f32), replayed from a hipGraph without autograd.
``attack(data, target, lengths)`` runs that loop on a batch of clouds of different sizes.
"""
import numpy as np
import torch
import torch.optim as optim

from ... import graphed as _graphed
from ... import ops
from ... import ragged as _ragged
from ... import streams as _streams
from ..CW.CW_utils import adv_utils as _adv_utils
from ..CW.CW_utils import clip_utils as _clip_utils
from ..CW.CW_utils import dist_utils as _dist_utils


def rand_row(array, dim_needed):
    """attack/KNN/KNN_attack.py:8-13."""
    row_total = array.shape[0]
    row_sequence = np.arange(row_total)
    np.random.shuffle(row_sequence)
    return array[row_sequence[0:dim_needed], :]


TRANSFER_MODELS = (("pt_fail", "pt_model"), ("ptm_fail", "ptm_model"), ("pts_fail", "pts_model"),
                   ("dgcnn_fail", "dgcnn_model"), ("cur_fail", "cur_model"))


def count_transfer_fails(attack, result, target, lens=None):
    """The five transfer checks (reference :160-240): every transfer model the attack holds (None: skipped) classifies
    `result` [B,3,K]; its counter grows by the samples on which the attack does not succeed there. lens (a ragged batch's
    sizes): a model that does not declare pad_invariant sees every cloud alone, on its own [1,3,lens[b]] slice."""
    for name, attr in TRANSFER_MODELS:
        m = getattr(attack, attr)
        if m is None:
            continue
        p = _ragged.predict(m, result, lens)
        setattr(attack, name, getattr(attack, name) + int((~attack._success(p, target)).sum().item()))


class CWKNN:
    """Class for CW attack."""

    def __init__(self, model, pt_model, ptm_model, pts_model, dgcnn_model, cur_model, adv_func, dist_func, clip_func,
                 attack_lr=1e-3, num_iter=2500, attack_method='untarget', device=None, verbose=False, fused=True,
                 graph=True, sample_seeds=None, global_batch=None, deterministic=None, device_loop=False):
        """Extra keywords (defaults = the reference's behaviour). For sharded runs: `sample_seeds` (one int
        per sample) draws every sample's start noise AND a PointNet++ victim's FPS start indices from that sample's own
        generator instead of the shared global stream, and `global_batch` is the size of the unsharded batch whose loss
        mean the shard is a part of — with both, a sample's trajectory does not depend on the batch or rank it runs in
        (bit for bit: the backward kernels sum in a fixed order, ops.DETERMINISTIC).
        `device_loop=True` runs the iteration as a captured chain of own kernels when the victim, the functors and the
        cloud size allow it (_device_loop_plan), and silently the usual path otherwise; `last_path` says which one the
        last attack() took: "device_loop", "direct" (own functors through autograd) or "generic"."""
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())

        def prep(m):
            if m is None:
                return None
            m = m.to(self.device)
            m.eval()
            return m

        # a victim with a deterministic forward replays its forward/backward from hipGraphs (graphed.py)
        self.model = _graphed.wrap(prep(model), enable=graph)
        self.pt_model = prep(pt_model)
        self.ptm_model = prep(ptm_model)
        self.pts_model = prep(pts_model)
        self.dgcnn_model = prep(dgcnn_model)
        self.cur_model = prep(cur_model)
        self.adv_func = adv_func
        self.dist_func = dist_func
        self.clip_func = clip_func
        self.attack_lr = attack_lr
        self.num_iter = num_iter
        self.attack_method = attack_method
        self.shuffle_fail = 0
        self.trans_fail = 0
        self.attack_fail = 0
        self.pt_fail = 0
        self.ptm_fail = 0
        self.pts_fail = 0
        self.dgcnn_fail = 0
        self.cur_fail = 0
        self.verbose = verbose
        self.fused = fused
        self.sample_seeds = sample_seeds
        self.global_batch = global_batch
        self.deterministic = deterministic     # None: ops.DETERMINISTIC; True / False: that mode during attack()
        self.graph = graph
        self.device_loop = device_loop
        self.last_path = None
        self._loop_cache = _graphed.LoopCache(1)    # the device loop (buffers and captured graphs), kept from call to call

    def _success(self, pred, target):
        return (pred != target) if self.attack_method == 'untarget' else (pred == target)

    def _fused_clip(self):
        """(budget, use_normal) for a recognised clip functor, else None."""
        cf = self.clip_func
        if not self.fused or cf is None:
            return None
        if type(cf) is _clip_utils.ProjectInnerClipLinf:
            return float(cf.budget), True
        if type(cf) in (_clip_utils.ClipPointsLinf, _dist_utils.ClipPointsLinf):
            return float(cf.budget), False
        return None

    # ---- device loop (PointNet victim + own functors): no autograd, every buffer updated IN PLACE, replayed from hipGraphs ----
    def _dist_plan(self):
        """(k, alpha, w1, w2) of a distance functor the device loop knows — ChamferkNNDist / ChamferDist with 'adv2ori'
        (w2 None: no kNN term) — else None."""
        df = self.dist_func
        if type(df) is _dist_utils.ChamferkNNDist and df.chamfer_dist.method == 'adv2ori':
            return int(df.knn_dist.k), float(df.knn_dist.alpha), float(df.w1), float(df.w2)
        if type(df) is _dist_utils.ChamferDist and df.method == 'adv2ori':
            return 0, 0.0, 1.0, None
        return None

    def _ragged_lengths(self, data, lengths):
        """lengths as int64 numpy [B] after every check of the ragged loop, or ValueError naming what does not fit, before
        any launch: there is no silent fall-back, since the direct and generic paths would count the padding copies of
        point 0 as neighbours and as outlier statistics."""
        who = "CWKNN.attack(lengths=...)"
        if not self.device_loop:
            raise ValueError(f"{who}: device_loop=False has no ragged pass")
        if data.dim() != 3 or data.shape[2] not in (3, 6):
            raise ValueError(f"{who}: data must be [B, Kmax, 3 or 6], got {tuple(data.shape)}")
        B, K = data.shape[:2]
        plan = self._device_loop_plan(B, K, data.shape[2] == 6, ragged=True)
        if isinstance(plan, str):
            raise ValueError(f"{who}: {plan}")
        return _ragged.check_lengths(who, lengths, B, K, max(1, plan["k"] + 1), "max(1, k + 1)")

    def _device_loop_plan(self, B, K, has_normal, ragged=False):
        """The one gate of the device loop: its constants when it applies — a GPU victim with fused_attack_grad (the two
        PointNetCls variants), an adversarial functor the CW loop maps to ops.LOSS_KINDS, ChamferkNNDist / ChamferDist
        with 'adv2ori', a clip functor _fused_clip() recognises, and a cloud the update kernel holds. Where it does not,
        the dense gate returns None (the caller takes the usual path) and the ragged one the reason, a string (the caller
        raises it). ragged: the victim must declare pad_invariant, and the two scales are per-cloud device data that
        every call prepares from its lengths, so the plan, and with it the loop's key, holds the functor's weights and
        the size of the whole batch in their place, and the flag."""
        victim = _graphed.unwrap(self.model)
        fc, dp = self._fused_clip(), self._dist_plan()
        kind = _adv_utils.own_adv_kind(self.adv_func)          # the CW loop's mapping of the adversarial functors
        if self.device.type != "cuda":
            why = f"the device {self.device} has no device loop"
        elif not hasattr(victim, "fused_attack_grad") or (ragged and not getattr(victim, "pad_invariant", False)):
            why = (f"the victim {type(victim).__name__} does not declare pad_invariant or lacks the fused entry points "
                   "(fused_attack_grad)")
        elif kind is None:
            why = f"adv_func {type(self.adv_func).__name__} is not one of this package's adversarial functors"
        elif dp is None:
            why = f"dist_func {type(self.dist_func).__name__} is neither ChamferkNNDist nor ChamferDist with 'adv2ori'"
        elif fc is None:
            why = (f"clip_func {type(self.clip_func).__name__} is neither ProjectInnerClipLinf nor ClipPointsLinf "
                   "(or fused=False)")
        elif K > ops.KNN_LOOP_MAX_POINTS:
            why = f"Kmax={K} exceeds KNN_LOOP_MAX_POINTS={ops.KNN_LOOP_MAX_POINTS}"
        elif dp[3] is not None and not 1 <= dp[0] <= 63:
            why = f"ChamferkNNDist's k={dp[0]} out of range [1, 63]"
        elif dp[0] + 1 > K:
            why = f"ChamferkNNDist's k + 1 = {dp[0] + 1} neighbours of Kmax={K} points"
        elif next(victim.parameters()).device.type != "cuda":
            why = "the victim's parameters are not on the GPU"
        else:
            why = None
        if why is not None:
            return why if ragged else None
        k, alpha, w1, w2 = dp
        # The batch mean and the shard ratio together are 1 / G, G the size of the whole batch: the constants are prepared
        # from G itself, so a sample's bits depend on neither the shard it runs in nor that shard's size. Without
        # global_batch (G = B) these are the float32 steps of the direct path's per_sample_terms / scaled_gvec.
        G = int(self.global_batch) if self.global_batch else B
        if ragged:
            scales = dict(w1=w1, w2=w2, G=G, ragged=True)
        else:
            up = np.float32(K)
            c_ch, c_knn = ops.knn_attack_scales(K, k, G, up * np.float32(w1), None if w2 is None else up * np.float32(w2))
            scales = dict(c_ch=float(c_ch), c_knn=float(c_knn))
        return dict(victim=victim, kind=kind, k=k, alpha=alpha, **scales, budget=fc[0],
                    clip_mode="project_clip" if fc[1] else "clip", scale=1.0 / G, has_normal=bool(has_normal and fc[1]))

    def _device_loop_state(self, plan, B, K):
        """The loop of this shape, these constants, this kernel flavour and these weights: its buffers (static: the graphs
        point at them), the iteration body and, once captured, the graphs — the last one is kept from call to call."""
        victim, dev, lr = plan["victim"], self.device, self.attack_lr
        key = _graphed.loop_key(victim, dev, B, K, float(lr), bool(self.graph),
                                tuple(sorted((n, v) for n, v in plan.items() if n != "victim")))
        loop = self._loop_cache.get(key)
        if loop is not None:
            return loop
        f32 = dict(dtype=torch.float32, device=dev)
        adv, ori, m, v = (torch.zeros((B, 3, K), **f32) for _ in range(4))
        normal = torch.zeros((B, 3, K), **f32) if plan["has_normal"] else None
        k = plan["k"]
        knn_d = torch.zeros((B, K, k + 1), **f32) if k else None
        knn_idx = torch.zeros((B, K, k + 1), dtype=torch.int32, device=dev) if k else None      # also the search's hint
        nn_d, nn_idx = torch.zeros((B, K), **f32), torch.zeros((B, K), dtype=torch.int32, device=dev)
        step = torch.zeros((1,), dtype=torch.int32, device=dev)
        pred = torch.zeros((B,), dtype=torch.long, device=dev)
        target = torch.zeros((B,), dtype=torch.long, device=dev)
        kind, kappa = plan["kind"]
        bufs = dict(adv=adv, ori=ori, normal=normal, target=target, plan=plan, m=m, v=v, step=step, pred=pred, knn_d=knn_d,
                    knn_idx=knn_idx, nn_d=nn_d, nn_idx=nn_idx)
        lens = lens_host = None
        c_ch, c_knn = plan.get("c_ch"), plan.get("c_knn")
        if plan.get("ragged"):
            # the lengths and the per-cloud scales are DATA of the captured launches: another call's lengths replay the
            # same graphs (_run_device_loop fills them in place)
            lens, lens_host = _ragged.loop_lengths(B, K, dev)
            c_ch, c_knn = torch.zeros((B,), **f32), torch.zeros((B,), **f32)
            bufs.update(lens=lens, lens_host=lens_host, c_ch=c_ch, c_knn=c_knn)
        vlens = _ragged.victim_kwargs(victim, lens)

        def body():
            # one chain on one stream: the victim's passes (the classifier tail advances the step word), the self-kNN
            # search hinted by its own last result, the adv -> ori search, the update. Ragged (lens: the lengths, else None
            # and every launch is the dense one): the same chain, launch for launch — the self-kNN search over every cloud's
            # own points, the adv -> ori search unchanged (ori's padding rows are copies of its point 0 and lose every tie
            # to it), the ragged update
            with torch.no_grad():
                _, _, gx = victim.fused_attack_grad(adv, target, kind, kappa, pred_out=pred, step=step, scale=plan["scale"],
                                                    **vlens)
                if k:
                    ops.knn_search_into(adv, knn_d, knn_idx, lengths=lens, lengths_host=lens_host)
                ops.nn_search_into(adv, ori, nn_d, nn_idx)
                ops.knn_attack_update(adv, ori, gx, m, v, step, lr, knn_d, knn_idx, nn_idx, c_ch, c_knn, plan["alpha"],
                                      plan["budget"], plan["clip_mode"], normal, lengths=lens)

        return self._loop_cache.put(key, _graphed.DeviceLoop(key, dev, owners=(victim,), counts=(1, self.LOOP_BLOCK),
                                                             warmup=2, body=body, bufs=bufs))

    LOOP_BLOCK = 16      # iterations per graph replay; the remainder replays single-iteration graphs

    def _run_device_loop(self, plan, adv_data, ori_data, normal, target, lens=None):
        B, _, K = adv_data.shape
        loop = self._device_loop_state(plan, B, K)
        c = loop.bufs
        if lens is not None:
            # what a run of every cloud alone prepares from its own point count (ops.knn_attack_scales_ragged)
            c_ch, c_knn = ops.knn_attack_scales_ragged(lens, plan["k"], plan["G"], plan["w1"], plan["w2"])
            _ragged.set_loop_lengths(c, lens)
            c["c_ch"].copy_(torch.from_numpy(c_ch)), c["c_knn"].copy_(torch.from_numpy(c_knn))

        def rewind():
            c["adv"].copy_(adv_data)
            c["m"].zero_(), c["v"].zero_(), c["step"].zero_()

        with torch.no_grad():
            c["ori"].copy_(ori_data)
            c["target"].copy_(target)
            if c["normal"] is not None:
                c["normal"].copy_(normal)
            rewind()
            if self.graph and self.num_iter > 0:
                loop.capture(rewind)
            loop.run(self.num_iter)
            adv_data.copy_(c["adv"])

    def attack(self, data, target, lengths=None):
        """Attack on given data to target.
        Args:
            data (torch.FloatTensor): victim data, [B, num_points, 3] (or 6 with normals)
            target (torch.LongTensor): target output, [B]
            lengths (default None: every cloud has data.shape[1] points, nothing changes): B ints, the sizes of a batch of
                clouds of different sizes as dataset.cloud_io.stack_ragged builds it, max(1, k + 1) <= lengths[b] <= Kmax =
                data.shape[1]; rows of data at and beyond a length are ignored. Runs the device loop only (device_loop=True,
                a pad_invariant PointNet victim, own functors, Kmax <= ops.KNN_LOOP_MAX_POINTS); anything else raises
                ValueError before any launch. With `sample_seeds` and `global_batch` every cloud gets the bits of its run
                alone; without seeds the start noise is one batch-shaped draw whose padding columns are ignored.
        Returns (adv [B,K,3] float32 numpy, success_num) like the reference (:244-246); with lengths, adv's rows at and
        beyond a cloud's length hold that cloud's row 0.
        """
        if lengths is not None:
            lengths = self._ragged_lengths(data, lengths)
        if self.deterministic is not None and self.deterministic != ops.DETERMINISTIC:
            with ops.deterministic(self.deterministic):
                return self.attack(data, target, lengths)
        if self.sample_seeds is None:
            return self._attack(data, target, None, lengths)
        from ...model import pointnet2_utils as _pn2
        assert len(self.sample_seeds) == data.shape[0], "sample_seeds needs one seed per sample"
        prev = _pn2.set_fps_start_source(_pn2.SeededFpsStarts([int(s) + 7919 for s in self.sample_seeds]))
        try:
            return self._attack(data, target, [torch.Generator().manual_seed(int(s)) for s in self.sample_seeds], lengths)
        finally:
            _pn2.set_fps_start_source(prev)

    def _attack(self, data, target, gens, lens=None):
        dev = self.device
        B, K = data.shape[:2]
        ratio = (float(B) / float(self.global_batch)) if self.global_batch else 1.0
        data = data.float().to(dev).detach()
        data = data.transpose(1, 2).contiguous()
        ori_data = data.clone().detach()
        ori_data.requires_grad = False

        # points and normals (:68-73; with xyz only the positions double as "normals", SURVEY A-11)
        if ori_data.shape[1] == 3:
            normal = ori_data
        else:
            normal = ori_data[:, 3:, :]
            ori_data = ori_data[:, :3, :]
        lens_dev = None
        if lens is not None:
            # ragged batch: every cloud's rows from its length on become copies of its point 0 (the normals' are never read)
            lens_dev = torch.from_numpy(lens.astype(np.int32)).to(dev)
            if normal is not ori_data:
                ori_data = ori_data.contiguous()
            ops.pad_ragged(ori_data, lens_dev)

        # clean forward (:76-78). Kept even when nothing is printed: a PointNet++ victim draws its FPS start indices
        # from the global RNG on every forward, so skipping it would shift the stream the reference sees.
        with torch.no_grad():
            clean_logits = _graphed.logits_of(self.model(ori_data))
            clean_pred = torch.argmax(clean_logits, dim=1)
        if self.verbose:
            print("ori label:", clean_pred.tolist())
        target = target.long().to(dev).detach().view(-1)

        # init variables with small perturbation (CPU generator like the reference, :84-85)
        if gens is None or lens is None:
            noise = torch.randn((B, 3, K)) if gens is None else torch.stack([torch.randn((3, K), generator=g) for g in gens])
        else:
            noise = _ragged.per_cloud_draw(B, 3, K, lens, lambda b, n: torch.randn((3, n), generator=gens[b]))
        adv_data = ori_data.clone().detach() + noise.to(dev) * 1e-7
        if lens is not None:
            ops.pad_ragged(adv_data, lens_dev)
        adv_data.requires_grad_()
        fc = self._fused_clip()
        if fc is None:
            opt = optim.Adam([adv_data], lr=self.attack_lr, weight_decay=0.)
        else:
            exp_avg, exp_avg_sq = torch.zeros_like(adv_data), torch.zeros_like(adv_data)
        # (with lens, _ragged_lengths has asked the gate already: a plan, never a reason)
        plan = self._device_loop_plan(B, K, normal is not ori_data, ragged=lens is not None) if self.device_loop else None
        if plan is not None:
            self.last_path = "device_loop"
            self._run_device_loop(plan, adv_data, ori_data, normal, target, lens)
            return self._finish(adv_data, target, B, lens)
        ori_t = ori_data.transpose(1, 2).contiguous()
        # Own functors on both sides: the loss is never assembled. Each functor hands back its per-sample terms with
        # d loss / d term built in (per_sample / per_sample_terms: the batch means, `* K`, the functor's own weights and the
        # shard ratio are constants), the backward starts from the terms, and the distance branch differentiates an ALIAS
        # of the iterate so that its gradient arrives in a buffer of its own, summed inside the Adam launch — none of the
        # ~25 mean / scale / add / accumulate launches of `loss = adv.mean() + dist.mean() * K; loss.backward()`.
        own_dist = (_dist_utils.ChamferDist, _dist_utils.HausdorffDist, _dist_utils.ChamferkNNDist)
        direct = (fc is not None and adv_data.is_cuda and type(self.dist_func) in own_dist
                  and hasattr(self.adv_func, "per_sample") and getattr(self, "direct_terms", True)
                  and clean_logits.dim() == 2 and 2 <= clean_logits.shape[1] <= 64 and clean_logits.dtype == torch.float32)
        self.last_path = "direct" if direct else "generic"
        if direct:
            adv_alias = adv_data.detach().requires_grad_()           # same storage: follows the in-place updates
            up_adv = np.float32(ratio)
            up_dist = np.float32(ratio) * np.float32(K) if ratio != 1.0 else np.float32(K)
            ones = ops.const_vec(dev, B, 1.0)

        # The distance term does not depend on the victim: its searches (kNN + Chamfer) run on a side stream beside the
        # victim's forward, whose first kernels (farthest-point sampling: one workgroup per cloud) leave most of the
        # chip idle. Autograd runs each node's backward on its forward's stream, so the two backwards overlap as well.
        cur = torch.cuda.current_stream(dev) if adv_data.is_cuda else None
        side = (_streams.side_stream(dev, _streams.TERMS)
                if cur is not None and getattr(self, "dist_stream", True) and getattr(self.model, "sampling_chain_front", False)
                else None)                      # ONE per process (see streams.py); only beside a sampling-chain victim
        # A PointNet++ victim draws an FPS start per sampling layer and forward from the CPU generator (SURVEY A-4): the
        # loop's draws are made here, in the same order, and uploaded once (pointnet2_utils.PredrawnFpsStarts)
        from ...model import pointnet2_utils as _pn2
        victim = _graphed.unwrap(self.model)
        predrawn = None
        if adv_data.is_cuda and hasattr(victim, "sampling_input_sizes") and getattr(self, "predraw_starts", True):
            predrawn = _pn2.PredrawnFpsStarts(victim.sampling_input_sizes(K), B, self.num_iter, dev, inner=_pn2.fps_start_source())
            prev_source = _pn2.set_fps_start_source(predrawn)
        try:
            for iteration in range(self.num_iter):
                if direct:
                    if side is not None:
                        side.wait_stream(cur)
                        with torch.cuda.stream(side):
                            terms = self.dist_func.per_sample_terms(adv_alias, ori_data, up_dist)   # channel-first, zero-copy
                    logits = _graphed.logits_of(self.model(adv_data))
                    a_term = self.adv_func.per_sample(logits.contiguous(), target, up_adv)
                    if a_term is None:
                        raise RuntimeError("CWKNN: the victim's logits changed shape / dtype between forwards")
                    if side is not None:
                        cur.wait_stream(side)
                    else:
                        terms = self.dist_func.per_sample_terms(adv_alias, ori_data, up_dist)
                    adv_data.grad = None
                    adv_alias.grad = None
                    torch.autograd.backward([a_term] + terms, [ones] * (1 + len(terms)))
                    ops.adam_clip_step(adv_data.data, adv_data.grad, exp_avg, exp_avg_sq, iteration + 1, self.attack_lr,
                                       ori=ori_data, normal=normal if fc[1] else None, budget=fc[0], g2=adv_alias.grad)
                    continue
                if side is not None:
                    side.wait_stream(cur)
                    with torch.cuda.stream(side):
                        # in the official tensorflow code they use sum instead of mean, hence * K (:119-123)
                        dist_loss = self.dist_func(adv_data.transpose(1, 2).contiguous(), ori_t).mean() * K
                logits = _graphed.logits_of(self.model(adv_data))  # [B, num_classes]
                adv_loss = self.adv_func(logits, target).mean()
                if side is not None:
                    cur.wait_stream(side)
                else:
                    dist_loss = self.dist_func(adv_data.transpose(1, 2).contiguous(), ori_t).mean() * K
                loss = adv_loss + dist_loss
                if ratio != 1.0:
                    loss = loss * ratio            # batch means (:117-123) of a shard of a larger batch
                if fc is None:
                    opt.zero_grad()
                    loss.backward()
                    opt.step()
                    adv_data.data = self.clip_func(adv_data.clone().detach(), ori_data, normal)
                else:
                    adv_data.grad = None
                    loss.backward()
                    ops.adam_clip_step(adv_data.data, adv_data.grad, exp_avg, exp_avg_sq, iteration + 1, self.attack_lr,
                                       ori=ori_data, normal=normal if fc[1] else None, budget=fc[0])
        finally:
            if predrawn is not None:
                _pn2.set_fps_start_source(prev_source)
        return self._finish(adv_data, target, B)

    def _finish(self, adv_data, target, B, lens=None):
        # end of CW attack (lens: a ragged batch — the victim is pad_invariant and sees the padded batch)
        with torch.no_grad():
            pred = torch.argmax(_graphed.logits_of(self.model(adv_data)), dim=-1)  # [B]
            success_num = int(self._success(pred, target).sum().item())
            if self.verbose:
                print('Successfully attack {}/{}'.format(success_num, B))
            result = adv_data.detach().float()
            # Test attack + transfer models (:160-240)
            self.attack_fail += int((~self._success(torch.argmax(_graphed.logits_of(self.model(result)), dim=1), target)).sum().item())
            count_transfer_fails(self, result, target, lens)

        adv_np = adv_data.detach().transpose(1, 2).contiguous().cpu().numpy()  # [B, K, 3]
        return adv_np, success_num
