"""C&W point-perturbation attack with binary search — MI355X mirror of attack/CW/CW_attack.py.

Same constructor / ``attack(data, target)`` signature and return values as the reference
(attack/CW/CW_attack.py:26-27,57,260). What changes is where the work happens:

* the hot loop (reference :111-178) never leaves the GPU: the per-iteration ``.cpu().numpy()`` of the whole
  adversarial cloud and the Python per-sample best-attack loop (:129-153) become device-side selects, so an
  iteration has no host synchronisation; the host is consulted once per binary-search step (:182-200);
* batches B > 1 work (the reference's prints / ``.item()`` calls at :84,:216-257 force B = 1; the fail counters
  are kept as attributes and become sums over the batch);
* when the functors are this package's own (``ClipPointsLinf`` / ``ProjectInnerClipLinf``), Adam + clip run as ONE
  fused HIP launch (pc3d_adam_clip_step_f32) instead of torch.optim.Adam + ~10 elementwise kernels. Arbitrary
  user callables still work through the generic path (same protocol as the reference:
  ``adv_func(logits, target)``, ``dist_func(adv[B,3,K], ori[B,3,K], weights[B])``, ``clip_func(pc, ori)``).
"""
import numpy as np
import torch
import torch.optim as optim

from ... import graphed as _graphed
from ... import ops
from ... import ragged as _ragged
from ... import streams as _streams
from .CW_utils import adv_utils as _adv_utils
from .CW_utils import clip_utils as _clip_utils
from .CW_utils import dist_utils as _dist_utils


def rand_row(array):
    """attack/CW/CW_attack.py:16-20 — shuffle the points of [B,K,3] with numpy's global RNG."""
    row_total = array.shape[1]
    row_sequence = np.arange(row_total)
    np.random.shuffle(row_sequence)
    return array[:, row_sequence, :]


def rand_row_ragged(array, lengths):
    """rand_row for clouds of different sizes, [B,Kmax,3] in place: cloud b's first lengths[b] rows are permuted — one
    permutation per cloud from numpy's global stream, in batch order, the draw rand_row makes for that cloud alone — and
    its further rows take the new row 0 again."""
    for b, n in enumerate(lengths):
        row_sequence = np.arange(int(n))
        np.random.shuffle(row_sequence)
        array[b, :int(n)] = array[b, row_sequence]
        array[b, int(n):] = array[b, 0]
    return array


def bisect_weights(lower, upper, current, ok):
    """The reference's weight adjustment (:182-200), sample by sample in float64, in place: an attack that succeeded
    (ok[e]) raises the lower bound to the weight it ran with, any other lowers the upper bound; the next weight is the
    midpoint."""
    for e in range(len(current)):
        if ok[e]:
            lower[e] = max(lower[e], current[e])
        else:
            upper[e] = min(upper[e], current[e])
        current[e] = (lower[e] + upper[e]) / 2.


class _GraphRunner:
    """Replays captured iterations; batches calls into unrolled graphs. The captured launches hold raw pointers
    into the state dict's tensors AND into the victim's folded / transposed weight caches, so the runner keeps both
    alive for as long as it lives — the former itself, the latter with the graphed.LoopGraph it holds (a later re-fold
    of the victim — other weights loaded, a device move — then leaves this runner replaying the weights it was captured
    with instead of reading freed memory).
    graphs: {iterations per launch: CUDAGraph}, always including 1. Calls accumulate until the largest graph is full;
    flush() runs what is pending with the largest graphs that fit. (A graph boundary costs ~17 us on this stack —
    single-iteration graphs replay at 308.7 us per iteration against 291.7 in a four-iteration graph — hence 16.)"""

    def __init__(self, st, loop):
        self._keep, self.loop, self.graphs, self.pending = st, loop, loop.graphs, 0
        self.sizes = sorted(self.graphs, reverse=True)
        self.g1, self.unroll = self.graphs[1], self.sizes[0]

    def __call__(self, i=None):
        self.pending += 1
        if self.pending == self.unroll:
            self.flush()

    def flush(self):
        self.loop.run(self.pending)
        self.pending = 0


class CW:
    """Class for CW attack."""
    ragged = True       # attack(data, target, lengths) exists; the point-adding subclasses switch it off

    def __init__(self, model, trans_model, adv_func, clip_func, dist_func, attack_lr=1e-2,
                 init_weight=10., max_weight=80., binary_step=10, num_iter=500, attack_method="untarget",
                 device=None, verbose=False, fused=True, graph=True, sample_seeds=None, global_batch=None,
                 deterministic=None, riders=True):
        """Arguments as attack/CW/CW_attack.py:26-38. Extra keyword-only style options (defaults keep the
        reference behaviour): device (default: current CUDA device), verbose (reference prints), fused (use the
        fused Adam+clip launch when clip_func is recognised). For sharded runs: `sample_seeds` (one int
        per sample of the batch handed to attack()) draws each sample's 1e-7 start noise (:94) from its own CPU
        generator instead of the shared global stream, and `global_batch` is the size of the unsharded batch whose
        `.mean()` (:160-165) this shard's losses belong to — with both, a sample's trajectory does not depend on the
        rank / batch it is attacked in. `riders`: the fused PointNet iteration in 15 launches (the search and the bookkeeping
        ride head launches, the update is the last backward's epilogue; True, the default) or in the 17 launches it replaced
        (False: the parity yardstick, bit-identical); a collection out of {"search", "update"} takes only those pieces."""
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.model = model.to(self.device)
        self.model.eval()
        # victims with a deterministic forward replay their forward/backward from hipGraphs (graphed.py); the fused
        # PointNet entry points are reached through the wrapper unchanged
        self.model = _graphed.wrap(self.model, enable=graph)
        self.trans_model = trans_model.to(self.device)
        self.trans_model.eval()
        self.adv_func = adv_func
        self.dist_func = dist_func
        self.attack_lr = attack_lr
        self.init_weight = init_weight
        self.max_weight = max_weight
        self.binary_step = binary_step
        self.num_iter = num_iter
        self.clip_func = clip_func
        self.attack_method = attack_method
        self.shuffle_fail = 0
        self.trans_fail = 0
        self.attack_fail = 0
        self.verbose = verbose
        # A/B switches of the autograd passes (on: the shipped behaviour): differentiate the functors' per-sample terms
        # directly (_direct_terms); run the distance term on the TERMS stream beside a sampling-chain victim (_dist_fork)
        self.direct_terms = True
        self.dist_stream = True
        self.fused = fused
        self.graph = graph
        self.riders = {"search", "update"} if riders is True else (set() if not riders else set(riders))
        if self.riders - {"search", "update"}:
            raise ValueError(f"riders: unknown piece(s) {sorted(self.riders - {'search', 'update'})}")
        self.sample_seeds = sample_seeds
        self.global_batch = global_batch
        # None: the process-wide setting (ops.DETERMINISTIC, default on: ordered backward sums, bit-reproducible runs);
        # True / False: that mode for the duration of attack()
        self.deterministic = deterministic

    # -- helpers ---------------------------------------------------------------------------------------
    def _success(self, pred, label):
        return (pred != label) if self.attack_method == 'untarget' else (pred == label)

    def _fused_clip_budget(self):
        """budget of a recognised per-point clip functor, else None (generic path)."""
        cf = self.clip_func
        if not self.fused or cf is None:
            return None
        if type(cf) in (_clip_utils.ClipPointsLinf, _dist_utils.ClipPointsLinf):
            return float(cf.budget)
        return None

    def _capturable(self):
        """hipGraph capture needs a body free of host syncs / allocations outside torch's pool. That is known for
        this package's own functors and victim mirrors; arbitrary user callables run eagerly instead."""
        own_adv = (_adv_utils.LogitsAdvLoss, _adv_utils.UntargetedLogitsAdvLoss, _adv_utils.CrossEntropyAdvLoss)
        own_dist = (_dist_utils.L2Dist, _dist_utils.ChamferDist, _dist_utils.HausdorffDist, _dist_utils.ChamferkNNDist)
        # Only the launch-minimal pass (a victim with fused_loss_and_grad) is captured whole. For the other victims
        # the iteration's bookkeeping copies become memcpy nodes, and a replay of that graph measured SLOWER than the
        # eager loop around a GraphedVictim (CurveNet, B=32 N=4096: 14.4 vs 10.7 ms per iteration).
        return (self.graph and self._fused_clip_budget() is not None and type(self.adv_func) in own_adv
                and type(self.dist_func) in own_dist and hasattr(self.model, "_require_fused")
                and self._fused_model_loss() is not None)

    def _fused_model_loss(self):
        """(kind, kappa) when the victim offers the launch-minimal fused_loss_and_grad AND the adversarial functor is
        one of this package's own (their gradients are built into pc3d_cls_loss_f32); else None (autograd path)."""
        if not self.fused or not hasattr(self.model, "fused_loss_and_grad"):
            return None
        return self._own_adv_kind()

    def _own_adv_kind(self):
        return _adv_utils.own_adv_kind(self.adv_func)

    def _direct_terms(self, st):
        """The autograd pass without the loss: own functors on both sides, a fused clip and a victim that goes through
        autograd. The iteration then differentiates the functors' per-sample terms (d loss / d term built in) and the logits
        (gradient from the loss kernel) directly — no mean / weight / sum / accumulate launches, see attack/KNN."""
        own_dist = (_dist_utils.ChamferDist, _dist_utils.HausdorffDist, _dist_utils.ChamferkNNDist)
        return (self.fused and self.direct_terms and st["budget"] is not None and st["adv"].is_cuda
                and type(self.dist_func) in own_dist and self._own_adv_kind() is not None
                and st["adv"].shape[1] == 3 and st["input_val"] is not None)

    def _fused_dist_kind(self):
        """1 / 2 when the distance functor's gradient is built into pc3d_cw_step_f32 (L2Dist, ChamferDist adv2ori),
        else 0 (its gradient then comes from autograd through the functor)."""
        df = self.dist_func
        if type(df) is _dist_utils.L2Dist:
            return 1
        if type(df) is _dist_utils.ChamferDist and df.method == 'adv2ori':
            return 2
        return 0

    # -- the hot loop, split so that bench.py / graph capture can drive single iterations ---------------
    def _ragged_lengths(self, data, lengths):
        """lengths as int64 numpy [B] after every check of the ragged path, or ValueError naming what does not fit: there is
        no silent fall-back, since a pass that does not know the lengths would average over the padding."""
        if not self.ragged:
            raise ValueError(f"CW.attack(lengths=...): {type(self).__name__} has no ragged pass")
        victim = _graphed.unwrap(self.model)
        if not getattr(victim, "pad_invariant", False) or not hasattr(victim, "fused_attack_grad"):
            raise ValueError(f"CW.attack(lengths=...): the victim {type(victim).__name__} does not declare pad_invariant or "
                             "lacks the fused entry points (fused_attack_grad)")
        if not self.fused:
            raise ValueError("CW.attack(lengths=...): fused=False has no ragged pass")
        if self._own_adv_kind() is None:
            raise ValueError(f"CW.attack(lengths=...): adv_func {type(self.adv_func).__name__} is not one of this package's "
                             "adversarial functors")
        if self._fused_dist_kind() == 0:
            raise ValueError(f"CW.attack(lengths=...): dist_func {type(self.dist_func).__name__} is neither L2Dist nor "
                             "ChamferDist('adv2ori')")
        if self._fused_clip_budget() is None:
            raise ValueError(f"CW.attack(lengths=...): clip_func {type(self.clip_func).__name__} is not ClipPointsLinf")
        if data.dim() != 3 or data.shape[2] != 3:
            raise ValueError(f"CW.attack(lengths=...): data must be [B, Kmax, 3], got {tuple(data.shape)}")
        B, K = data.shape[:2]
        if K > ops.CW_UPDATE_MAX_POINTS:
            raise ValueError(f"CW.attack(lengths=...): Kmax={K} exceeds CW_UPDATE_MAX_POINTS={ops.CW_UPDATE_MAX_POINTS}")
        return _ragged.check_lengths("CW.attack(lengths=...)", lengths, B, K)

    def _begin(self, data, target, lengths=None):
        """Upload + clean prediction (reference :63-89). Returns the state dict the iteration works on. lengths (checked by
        _ragged_lengths): the clouds' sizes; they live in an int32 device buffer of the state, which the kernels read as
        data, and ori is padded with copies of every cloud's point 0."""
        dev = self.device
        B, K = data.shape[:2]
        data = data.float().to(dev).detach()
        data = data.transpose(1, 2).contiguous()
        ori_data = data.clone().detach()
        lens_dev = None
        if lengths is not None:
            lens_dev = torch.from_numpy(np.asarray(lengths, dtype=np.int32)).to(dev)
            ops.pad_ragged(ori_data, lens_dev)
        target = target.long().to(dev).detach().view(-1)
        label = target
        with torch.no_grad():
            logits = _graphed.logits_of(self.model(ori_data))
            pred = torch.argmax(logits, dim=1)
        if self.verbose:
            print("ori label:", pred.tolist())
        if self.attack_method == 'top1_error':
            # reference (:86-89, B=1): target := runner-up class of the clean prediction
            target = label = logits.topk(2, dim=1, largest=True, sorted=True)[1][:, 1].detach()
        gens = None
        if self.sample_seeds is not None:
            assert len(self.sample_seeds) == B, "sample_seeds needs one seed per sample"
            gens = [torch.Generator().manual_seed(int(sd)) for sd in self.sample_seeds]
        return dict(
            B=B, K=K, ori=ori_data, target=target, label=label, budget=self._fused_clip_budget(), gens=gens,
            # ragged batch: the sizes on the host (start noise, final checks) and on the device (the update launch)
            lengths_host=None if lengths is None else [int(n) for n in lengths], lengths=lens_dev,
            # losses are batch means (:160-165): a shard of a larger batch scales its terms by B/global_batch
            ratio=(float(B) / float(self.global_batch)) if self.global_batch else 1.0,
            # weight factor for budget regularization (host, consulted once per binary step)
            lower_bound=np.zeros((B,)), upper_bound=np.ones((B,)) * self.max_weight,
            current_weight=np.ones((B,)) * self.init_weight,
            # best results over the whole binary search — device resident
            o_bestdist=torch.full((B,), 1e10, dtype=torch.float32, device=dev),
            o_bestscore=torch.full((B,), -1, dtype=torch.long, device=dev),
            o_bestattack=torch.zeros((B, 3, K), dtype=torch.float32, device=dev),
            input_val=ori_data.clone(), pred=torch.zeros((B,), dtype=torch.long, device=dev),
            step=torch.zeros((1,), dtype=torch.int32, device=dev), graph=None,
            dist_val=torch.zeros((B,), dtype=torch.float32, device=dev),
            # Adam's two bias-correction factors of the current step, written on the device by the bookkeeping rider
            adam=torch.zeros((2,), dtype=torch.float32, device=dev))

    def _begin_binary_step(self, st):
        """Fresh start point, Adam state and per-step bests (reference :94-100)."""
        dev, B, K = self.device, st["B"], st["K"]
        # same RNG stream as the reference: CPU generator, then upload (:94)
        if st["gens"] is None:
            # (ragged: the batch-shaped draw stays, its padding columns are overwritten below; a cloud's noise then depends
            # on the batch it is in, so this mode is not comparable cloud by cloud with runs alone)
            noise = torch.randn((B, 3, K))
        elif st.get("lengths") is None:
            noise = torch.stack([torch.randn((3, K), generator=g) for g in st["gens"]])
        else:
            noise = _ragged.per_cloud_draw(B, 3, K, st["lengths_host"],
                                           lambda b, n: torch.randn((3, n), generator=st["gens"][b]))
        adv_data = st["ori"].clone().detach() + noise.to(dev) * 1e-7
        if st.get("lengths") is not None:
            ops.pad_ragged(adv_data, st["lengths"])
        adv_data.requires_grad_()
        if "adv" not in st:
            # first binary step: allocate the per-step state once; later steps refill it IN PLACE so a captured
            # hipGraph of the iteration stays valid across binary steps
            st["adv"] = adv_data
            st["bestdist"] = torch.full((B,), 1e10, dtype=torch.float32, device=dev)
            st["bestscore"] = torch.full((B,), -1, dtype=torch.long, device=dev)
            st["weights"] = torch.from_numpy(st["current_weight"] * st["ratio"]).float().to(dev)
            # d loss / d (distance term of sample b) for `dist_func(adv, ori, weights).mean()`: weights[b] / B, what autograd
            # derives in two launches per iteration (the direct-terms pass below reads it from here)
            st["gdist"] = st["weights"] * float(np.float32(1.0) / np.float32(B))
            if st["budget"] is not None:
                st["exp_avg"] = torch.zeros_like(adv_data)
                st["exp_avg_sq"] = torch.zeros_like(adv_data)
        else:
            with torch.no_grad():
                st["adv"].copy_(adv_data)
                st["bestdist"].fill_(1e10)
                st["bestscore"].fill_(-1)
                st["weights"].copy_(torch.from_numpy(st["current_weight"] * st["ratio"]).float())
                torch.mul(st["weights"], float(np.float32(1.0) / np.float32(B)), out=st["gdist"])
                if st["budget"] is not None:
                    st["exp_avg"].zero_()
                    st["exp_avg_sq"].zero_()
        st["step"].zero_()
        if st["budget"] is None:
            st["opt"] = optim.Adam([st["adv"]], lr=self.attack_lr, weight_decay=0.)

    def _iterate(self, st, iteration=None, last=False):
        """One pass of the hot-loop body (reference :111-174), entirely on the device. The Adam step number lives
        in st["step"] on the device, so the body is identical every pass (hipGraph-replayable). Picks the pass."""
        fml = self._fused_model_loss() if st["budget"] is not None else None
        dk = self._fused_dist_kind() if fml is not None else 0
        if st.get("lengths") is not None:
            # ragged batch (attack() has checked everything): the 17-launch pass, its update launch given the lengths; the
            # riders do not apply, their epilogue does not know lengths
            return self._pass_fused_update(st, fml, dk)
        if dk:
            # launch-minimal passes: victim fwd/bwd (fused heads), bookkeeping, [NN search], one update launch
            if (self.riders and "adam" in st and hasattr(self.model, "fused_attack_update")
                    and getattr(self.model, "has_fused_attack_update", True) and st["K"] <= ops.CW_UPDATE_MAX_POINTS):
                return self._pass_riders(st, fml, dk)
            if hasattr(self.model, "fused_attack_grad") and st["K"] <= ops.CW_UPDATE_MAX_POINTS:
                return self._pass_fused_update(st, fml, dk)
            return self._pass_fused_steps(st, fml, dk)
        if fml is None and self._direct_terms(st):
            return self._pass_direct_terms(st)
        return self._pass_autograd(st, fml)

    def _pass_riders(self, st, fml, dk):
        """15 launches: the search, the bookkeeping and the update ride the victim's own launches."""
        with torch.no_grad():
            self.model.fused_attack_update(
                st["adv"].detach(), st["target"], *fml, pred_out=st["pred"], step=st["step"], scale=st["ratio"] / st["B"],
                cw=dict(ori=st["ori"], label=st["label"], untarget=self.attack_method == 'untarget',
                        bestdist=st["bestdist"], bestscore=st["bestscore"], o_bestdist=st["o_bestdist"],
                        o_bestscore=st["o_bestscore"], o_bestattack=st["o_bestattack"], input_val=st["input_val"],
                        dist_val=st["dist_val"], m=st["exp_avg"], v=st["exp_avg_sq"], w=st["weights"],
                        adam=st["adam"], lr=self.attack_lr, budget=st["budget"], dist_kind=dk),
                ride_search="search" in self.riders, epilogue="update" in self.riders)

    def _pass_fused_update(self, st, fml, dk):
        """17 launches: the classifier tail writes pred + advances the step word, [the search], one update launch."""
        ori_data = st["ori"]
        with torch.no_grad():
            cur = st["adv"].detach()
            _, _, gx_model = self.model.fused_attack_grad(cur, st["target"], *fml, pred_out=st["pred"], step=st["step"],
                                                          scale=st["ratio"] / st["B"],
                                                          **_ragged.victim_kwargs(self.model, st.get("lengths")))
            nn_idx = None
            if dk == 2:
                _, nn_idx = ops.nn_raw(cur, ori_data, True, True)
            ops.cw_update(cur, ori_data, st["pred"], st["label"], self.attack_method == 'untarget', st["bestdist"],
                          st["bestscore"], st["o_bestdist"], st["o_bestscore"], st["o_bestattack"], gx_model,
                          st["exp_avg"], st["exp_avg_sq"], st["step"], self.attack_lr, st["budget"],
                          input_val=st["input_val"], dist_val=st["dist_val"], dist_kind=dk, w=st["weights"],
                          nn_idx=nn_idx, lengths=st.get("lengths"))

    def _pass_fused_steps(self, st, fml, dk):
        """A victim with fused_loss_and_grad only (or a cloud too large for the update launch): bookkeeping, [the
        search] and the step are a launch each."""
        ori_data = st["ori"]
        with torch.no_grad():
            cur = st["adv"].detach()
            _, pred, _, gx_model = self.model.fused_loss_and_grad(cur, st["target"], *fml,
                                                                  scale=st["ratio"] / st["B"])
            ops.cw_bookkeep(cur, ori_data, pred, st["label"], self.attack_method == 'untarget', st["bestdist"],
                            st["bestscore"], st["o_bestdist"], st["o_bestscore"], st["o_bestattack"],
                            input_val=st["input_val"], dist_val=st["dist_val"], step=st["step"])
            st["pred"].copy_(pred)
            nn_idx = None
            if dk == 2:
                _, nn_idx = ops.nn_raw(cur, ori_data, True, True)
            ops.cw_step(cur, gx_model, st["exp_avg"], st["exp_avg_sq"], st["step"], self.attack_lr, ori_data,
                        st["budget"], dist_kind=dk, w=st["weights"], l2norm=st["dist_val"], nn_idx=nn_idx)

    def _dist_fork(self, adv_data):
        """(main, side) when the distance term is to run beside the victim, side already waiting on main; else None.
        The term depends on the iterate only: beside a victim whose forward starts with a sampling chain (most of the
        chip idle: CurveNet, PointNet++) it runs on the process-wide TERMS stream, and autograd runs its backward there
        too (as in attack/KNN/KNN_attack.py). Beside DGCNN the same move cost GeoA3 2 %, hence the victim's flag."""
        if not (adv_data.is_cuda and self.dist_stream and getattr(self.model, "sampling_chain_front", False)
                and not torch.cuda.is_current_stream_capturing()):
            return None
        main = torch.cuda.current_stream(adv_data.device)
        side = _streams.side_stream(adv_data.device, _streams.TERMS)
        side.wait_stream(main)
        return main, side

    def _pass_direct_terms(self, st):
        """The autograd pass without the loss (see _direct_terms)."""
        adv_data, ori_data, B = st["adv"], st["ori"], st["B"]
        alias = st.get("adv_alias")
        if alias is None or alias.data_ptr() != adv_data.data_ptr():
            alias = st["adv_alias"] = adv_data.detach().requires_grad_()      # same storage, its own .grad
        fork = self._dist_fork(adv_data)
        if fork:
            with torch.cuda.stream(fork[1]):
                terms = self.dist_func.per_sample_terms(alias, ori_data, st["gdist"], mean=False)
        logits = _graphed.logits_of(self.model(adv_data))
        kind, kappa = self._own_adv_kind()
        lg = logits if (logits.dtype == torch.float32 and logits.stride(1) == 1) else logits.float().contiguous()
        # the loss kernel in raw mode (+4: the functor's value on the logits as given): prediction into st["pred"],
        # gradient already scaled by ratio / B (the batch mean)
        _, pred, _, g_logits = ops.cls_loss(lg.detach(), st["target"], ops.LOSS_KINDS[kind] + 4, kappa,
                                            float(np.float32(st["ratio"]) / np.float32(B)), pred_out=st["pred"])
        with torch.no_grad():
            ops.cw_bookkeep(adv_data.detach(), ori_data, pred, st["label"], self.attack_method == 'untarget', st["bestdist"],
                            st["bestscore"], st["o_bestdist"], st["o_bestscore"], st["o_bestattack"],
                            input_val=st["input_val"], dist_val=st["dist_val"], step=st["step"])
        if fork:
            fork[0].wait_stream(fork[1])
        else:
            terms = self.dist_func.per_sample_terms(alias, ori_data, st["gdist"], mean=False)
        adv_data.grad = None
        alias.grad = None
        ones = ops.const_vec(adv_data.device, B, 1.0)
        torch.autograd.backward([lg] + terms, [g_logits] + [ones] * len(terms))
        ops.adam_clip_step(adv_data.data, adv_data.grad, st["exp_avg"], st["exp_avg_sq"], st["step"],
                           self.attack_lr, ori=ori_data, budget=st["budget"], g2=alias.grad)

    def _bookkeep_torch(self, st, cur, pred, dist_val):
        """The record of one pass (reference :129-153) in torch ops, for what pc3d_cw_bookkeep_f32 does not take."""
        with torch.no_grad():
            succ = self._success(pred, st["label"])
            upd = succ & (dist_val < st["bestdist"])
            st["bestdist"].copy_(torch.where(upd, dist_val, st["bestdist"]))
            st["bestscore"].copy_(torch.where(upd, pred, st["bestscore"]))
            upd_o = succ & (dist_val < st["o_bestdist"])
            st["o_bestdist"].copy_(torch.where(upd_o, dist_val, st["o_bestdist"]))
            st["o_bestscore"].copy_(torch.where(upd_o, pred, st["o_bestscore"]))
            st["o_bestattack"].copy_(torch.where(upd_o[:, None, None], cur, st["o_bestattack"]))
            st["input_val"].copy_(cur)     # the iterate the LAST pass started from (reference :133, :208-209)
            st["pred"].copy_(pred)

    def _pass_autograd(self, st, fml):
        """The generic protocol: the functors as given, gradients from autograd. With fml the victim's side (forward,
        adversarial loss, backward to the input) is its fused_loss_and_grad and autograd differentiates the distance only."""
        adv_data, ori_data, label = st["adv"], st["ori"], st["label"]
        gx_model = fork = None
        if fml is not None:
            with torch.no_grad():  # victim forward + adversarial loss + backward-to-input without autograd
                logits, pred, _, gx_model = self.model.fused_loss_and_grad(adv_data.detach(), st["target"], *fml,
                                                                           scale=st["ratio"] / st["B"])
        else:
            fork = self._dist_fork(adv_data)
            if fork:
                with torch.cuda.stream(fork[1]):
                    dist_loss = self.dist_func(adv_data, ori_data, st["weights"]).mean()
            logits = _graphed.logits_of(self.model(adv_data))
            pred = torch.argmax(logits, dim=1)  # [B]
        # record values (device side; reference :129-153)
        with torch.no_grad():
            cur = adv_data.detach()
        if (cur.is_cuda and cur.dtype == torch.float32 and ori_data.dtype == torch.float32 and pred.dtype == torch.int64
                and cur.dim() == 3 and cur.shape[1] == 3 and st["input_val"] is not None):
            # the same bookkeeping as ONE launch (pc3d_cw_bookkeep_f32, as on the fused-victim path) instead of ~16
            with torch.no_grad():
                ops.cw_bookkeep(cur, ori_data, pred.contiguous(), label, self.attack_method == 'untarget', st["bestdist"],
                                st["bestscore"], st["o_bestdist"], st["o_bestscore"], st["o_bestattack"],
                                input_val=st["input_val"], dist_val=st["dist_val"])
                st["pred"].copy_(pred)
        else:
            with torch.no_grad():
                dist_val = torch.sqrt(torch.sum((cur - ori_data) ** 2, dim=[1, 2]))  # [B]
            self._bookkeep_torch(st, cur, pred, dist_val)
        # compute loss and backward
        if fork:
            fork[0].wait_stream(fork[1])
        else:
            dist_loss = self.dist_func(adv_data, ori_data, st["weights"]).mean()
        if gx_model is not None:
            adv_data.grad = None
            dist_loss.backward()
            adv_data.grad.add_(gx_model)
            ops.i32_add(st["step"], 1)
            ops.adam_clip_step(adv_data.data, adv_data.grad, st["exp_avg"], st["exp_avg_sq"], st["step"],
                               self.attack_lr, ori=ori_data, budget=st["budget"])
            return
        adv_loss = self.adv_func(logits, st["target"]).mean()
        if st["ratio"] != 1.0:
            adv_loss = adv_loss * st["ratio"]
        loss = adv_loss + dist_loss
        if st["budget"] is None:
            opt = st["opt"]
            opt.zero_grad()
            loss.backward()
            opt.step()
            if self.clip_func is not None:
                adv_data.data = self.clip_func(adv_data.clone().detach(), ori_data)
        else:
            adv_data.grad = None
            loss.backward()
            ops.i32_add(st["step"], 1)
            ops.adam_clip_step(adv_data.data, adv_data.grad, st["exp_avg"], st["exp_avg_sq"], st["step"],
                               self.attack_lr, ori=ori_data, budget=st["budget"])

    def _make_runner(self, st, warmup=3, unroll=16):
        """Capture the iteration into hipGraphs (after `warmup` eager passes on a side stream, as torch requires) and
        return a callable that replays it. Only the fused path (recognised clip functor) is captured; the generic
        path with arbitrary user callables returns an eager runner. Replays are bit-identical to eager passes: same
        kernels, same order, same buffers. Graphs of 1, 4 and `unroll` iterations back to back are kept: the runner
        batches calls into the largest one (one graph launch per `unroll` iterations instead of one each) and `flush()`
        runs whatever is still pending with the largest graphs that fit; callers flush before they read results or
        stop a clock."""
        if not self._capturable():
            run = lambda i=None: self._iterate(st, i)    # noqa: E731
            return run
        if st["graph"] is not None:
            return st["graph_run"]
        victim = _graphed.unwrap(self.model)
        # warm-up passes are real iterations; account for them by NOT rolling anything back: callers start counting
        # after _make_runner (bench) or use _begin_binary_step to reset the state (attack()).
        loop = _graphed.LoopGraph(lambda: self._iterate(st), self.device, warmup,
                                  counts={1, min(4, max(1, unroll)), max(1, unroll)}, owners=(victim,))
        st["graph"] = loop.graphs[1]
        # the runner keeps the state's tensors alive, not the dict itself (st -> runner -> st would be a cycle that only
        # the cycle collector frees, at an arbitrary later time)
        st["graph_run"] = _GraphRunner([v for v in st.values() if torch.is_tensor(v)], loop)
        return st["graph_run"]

    def _end_binary_step(self, st):
        """Adjust the weight factor (reference :182-200) — one host round trip per binary step."""
        bs = st["bestscore"].cpu().numpy()
        bd = st["bestdist"].double().cpu().numpy()
        obd = st["o_bestdist"].double().cpu().numpy()
        lab = st["label"].cpu().numpy()
        hit = (bs != lab) if self.attack_method == 'untarget' else (bs == lab)
        bisect_weights(st["lower_bound"], st["upper_bound"], st["current_weight"], hit & (bs != -1) & (bd <= obd))

    def attack(self, data, target, lengths=None):
        """lengths (default None: every cloud has data.shape[1] points, nothing changes): a sequence, array or tensor of B
        ints, 1 <= lengths[b] <= Kmax = data.shape[1], the sizes of a batch of clouds of different sizes. Rows of data at and
        beyond a cloud's length are ignored (dataset.cloud_io.stack_ragged builds such a batch). Every cloud is attacked as
        it is — with `sample_seeds` and `global_batch` = B exactly as in a run of that cloud alone — in one batch, on a
        pad_invariant victim (PointNetCls) with own functors (L2Dist or ChamferDist('adv2ori'), ClipPointsLinf); anything
        else raises ValueError before any launch. Without `sample_seeds` the start noise is one batch-shaped draw whose
        padding columns are ignored, which is NOT comparable cloud by cloud with runs alone. In the returned
        o_bestattack [B,Kmax,3], rows at and beyond a cloud's length hold that cloud's row 0."""
        args = (data, target) if lengths is None else (data, target, self._ragged_lengths(data, lengths))
        if self.deterministic is None:
            return self._attack(*args)
        with ops.deterministic(self.deterministic):
            return self._attack(*args)

    def _search(self, st):
        """The binary search (reference :93-200): every step restarts from a fresh start point, runs num_iter iterations
        (captured into hipGraphs when the body allows) and adjusts the weights once on the host."""
        run = None
        self.weight_history = []          # [binary_step][B]: the distance weight every binary step ran with (reference :93-200)
        for binary_step in range(self.binary_step):
            self._begin_binary_step(st)
            self.weight_history.append(st["current_weight"].copy())
            if run is None and self._capturable() and self.num_iter >= 8:
                # capture once (its warm-up passes advance the state), then restart this binary step cleanly with
                # the SAME start point so results do not depend on whether a graph is used
                start = st["adv"].detach().clone()
                o_keep = (st["o_bestdist"].clone(), st["o_bestscore"].clone(), st["o_bestattack"].clone())
                run = self._make_runner(st)
                with torch.no_grad():
                    st["adv"].copy_(start)
                    st["bestdist"].fill_(1e10)
                    st["bestscore"].fill_(-1)
                    st["exp_avg"].zero_()
                    st["exp_avg_sq"].zero_()
                    st["step"].zero_()
                    st["o_bestdist"].copy_(o_keep[0])
                    st["o_bestscore"].copy_(o_keep[1])
                    st["o_bestattack"].copy_(o_keep[2])
            for iteration in range(self.num_iter):
                if run is not None:
                    run()
                else:
                    self._iterate(st, iteration)
            if hasattr(run, "flush"):
                run.flush()
            self._end_binary_step(st)

    def _outcome(self, st):
        """(success_num, o_bestattack [B,3,K]) after the search: success counted on the last prediction; samples that
        never succeeded take the last iterate (reference :205-209)."""
        pred = st["pred"] if self.num_iter > 0 and self.binary_step > 0 else None
        success_num = int(self._success(pred, st["label"]).sum().item()) if pred is not None else 0
        fail_idx = torch.from_numpy(st["lower_bound"] == 0.).to(self.device)
        return success_num, torch.where(fail_idx[:, None, None], st["input_val"], st["o_bestattack"])

    def _attack(self, data, target, lengths=None):
        """Attack on given data to target.
        Args:
            data (torch.FloatTensor): victim data, [B, num_points, 3]
            target (torch.LongTensor): target output, [B]
        Returns (o_bestdist [B] float64, o_bestattack [B,K,3] float64, success_num) like the reference (:260).
        """
        dev = self.device
        st = self._begin(data, target, lengths)
        target, lens = st["target"], st["lengths_host"]
        self._search(st)
        success_num, o_bestattack = self._outcome(st)
        o_bestdist = st["o_bestdist"]

        with torch.no_grad():
            # Test attack (:211-224)
            attack_pred = torch.argmax(_graphed.logits_of(self.model(o_bestattack)), dim=1)
            self.attack_fail += int((~self._success(attack_pred, target)).sum().item())
            # Test shuffle attack (:226-241) — numpy global RNG like the reference
            best_np = o_bestattack.double().cpu().numpy()  # [B,3,K]
            if lens is None:
                shuffled = rand_row(best_np.transpose((0, 2, 1)))
            else:
                shuffled = rand_row_ragged(best_np.transpose((0, 2, 1)).copy(), lens)
            shuffled = torch.from_numpy(shuffled.transpose((0, 2, 1)).copy()).float().to(dev)
            shuffle_pred = torch.argmax(_graphed.logits_of(self.model(shuffled)), dim=1)
            self.shuffle_fail += int((~self._success(shuffle_pred, target)).sum().item())
            # Test transfer attack (:244-257)
            trans_pred = _ragged.predict(self.trans_model, o_bestattack, lens)
            self.trans_fail += int((~self._success(trans_pred, target)).sum().item())
        if self.verbose:
            print('attack result: ', attack_pred.tolist(), 'shuffle result: ', shuffle_pred.tolist(),
                  'transfer result: ', trans_pred.tolist())

        return o_bestdist.double().cpu().numpy(), best_np.transpose((0, 2, 1)), success_num
