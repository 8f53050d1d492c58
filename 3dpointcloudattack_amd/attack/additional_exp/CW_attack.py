"""CW with the binary-searched point-set distance, z-only perturbation, renormalisation in the loop and expectation
over small random rotations / resampling — MI355X mirror of attack/additional_exp/CW_attack.py.

Same constructor and ``attack(data, target, origin_label)`` signature and return values as the reference (:14-18,
:47, :321). This is the caller that exercises the Chamfer / Chamfer+kNN regularisers as THE binary-searched distance
(:151-159): with this package's functors they are the fused nearest-neighbour / kNN HIP kernels, so no [B,K,K]
matrix is formed in any of the 1 + 10 forwards of an iteration.

Protocol kept from the reference:
  * ``adv_func(logits, label, whether_target=1|0)`` (:245-247,:254,:259) — note that no functor in the reference
    repository accepts that keyword; ``AdvLossAdapter`` below wraps the CW_utils.adv_utils functors;
  * ``dist_func(adv[B,K,3], ori[B,K,3], weights[B])`` (:151-153), scalar or per-sample result;
  * ``model(x[B,3,K]) -> (logits, _, _)`` (:75,:117);
  * random streams: the start noise and the rotation angles come from torch's global CPU generator (:88,:196), the
    rotation choice and the resampling indices from Python's ``random`` (:211,:238) — drawn here in the same order,
    so a seeded run consumes the same streams as the reference.
What changes: batches B > 1 work (the reference prints ``.item()`` and constrains only sample 0, :80-84,:268-275 —
here the z-only / box constraint applies to every sample); bookkeeping stays on the device (one host read per
binary-search step); the resampling draws ``K`` of ``2K`` indices (the reference hard-codes 4000 of 8000, :238).

``device_loop=True`` (PointNet victims, see ``CW._device_loop_plan``): the iteration is ONE stacked victim pass of the
iterate and its ten views between pc3d_eot_prepare_f32 and pc3d_eot_update_f32 (csrc/eot.hip), replayed from a hipGraph
without autograd; the rotations and resampling indices are still drawn on the host, in the same order, a block of
iterations ahead — or, with ``device_rng=True``, on the device by pc3d_eot_draw_f32 (a counter-based stream of its own, NOT
draw-for-draw comparable with the reference: see ``CW.__init__``).

``attack(..., lengths=...)``: clouds of different sizes in one batch on that device loop — the lengths reach
the three kernels of csrc/eot.hip through their ``_ragged_f32`` twins and, with resampling, the per-cloud tables the device
draws; every cloud comes out as from a run of that cloud alone.
"""
import random
import time

import numpy as np
import torch
import torch.optim as optim

from ... import graphed as _graphed
from ... import ops
from ... import ragged as _ragged
from ..CW.CW_attack import bisect_weights


class AdvLossAdapter:
    """Gives a CW_utils.adv_utils-style functor pair the ``whether_target`` keyword this attack calls with (:245-259)."""

    def __init__(self, targeted_func, untargeted_func=None):
        self.targeted_func = targeted_func
        self.untargeted_func = untargeted_func if untargeted_func is not None else targeted_func

    def __call__(self, logits, label, whether_target=1):
        return (self.targeted_func if whether_target else self.untargeted_func)(logits, label)


class PerSampleDist:
    """Gives a CW_utils.dist_utils functor the ``dist_func(adv, ori, weights)`` call of this attack with one distance per
    sample (``batch_avg=False``): what the per-sample bookkeeping of a batch B > 1 needs, and what the device loop
    recognises (``CW._device_loop_plan``)."""

    def __init__(self, functor):
        self.functor = functor

    def __call__(self, adv, ori, weights=None):
        return self.functor(adv, ori, weights, batch_avg=False)


def _inverse_columns(cols, K, out):
    """out [K,2] (int32): the at most two positions j with cols[j] == i, ascending, else -1 (K draws without replacement
    from the 2K - 1 columns of cat((x, x), 2) hit a point at most twice)."""
    out.fill(-1)
    order = np.argsort(cols, kind="stable")
    sc = cols[order]
    first = np.ones(K, dtype=bool)
    first[1:] = sc[1:] != sc[:-1]
    out[sc[first], 0] = order[first]
    out[sc[~first], 1] = order[~first]


def _renormalize(x):
    """:107-115 / :224-230 — centre and scale [B,3,K] to the unit sphere (differentiable, like the reference)."""
    p = x.permute(0, 2, 1)
    p = p - torch.mean(p, dim=1).unsqueeze(1)
    var = torch.max(torch.sqrt(torch.sum(p ** 2, dim=2)), dim=1, keepdim=True)[0]
    return (p / var.unsqueeze(1)).permute(0, 2, 1)


def _rotation_draw():
    """:195-219 — one draw of (theta ~ 1e-2 N(0,1), axis choice) as a 3 x 3 list: z / x / y rotation with probability 0.2
    each, else the identity. Consumes torch.randn(1) THEN random.random(), like the reference."""
    theta = torch.randn(1) * 1e-2
    c, s = float(torch.cos(theta)), float(torch.sin(theta))
    r = random.random()
    if r < 0.2:
        return [[c, s, 0], [-s, c, 0], [0, 0, 1]]
    if r < 0.4:
        return [[1, 0, 0], [0, c, s], [0, -s, c]]
    if r < 0.6:
        return [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    return [[1, 0, 0], [0, 1, 0], [0, 0, 1]]


def _small_rotation(dev):
    """The draw as a [1,3,3] device tensor (the autograd path: one upload per view)."""
    return ops.h2d(torch.tensor(_rotation_draw(), dtype=torch.float32), dev).unsqueeze(0)


class CW:
    """Class for CW attack (additional experiments)."""

    def __init__(self, model, adv_func, dist_func, attack_lr=1e-2,
                 init_weight=10., max_weight=80., binary_step=10, num_iter=500, whether_target=True, whether_1d=True,
                 whether_renormalization=False,
                 whether_3Dtransform=False, whether_resample=False, device=None, verbose=False, graph=True,
                 device_loop=False, device_rng=False, seed=None, sample_seeds=None, global_batch=None):
        """`device_loop=True` runs the iteration as a captured chain of own kernels around ONE stacked victim pass when
        the victim, the functors and the cloud size allow it (_device_loop_plan), and silently the usual path otherwise;
        `last_path` says which one the last attack() took: "device_loop" or "autograd".

        `device_rng=True` (off by default) lets the device loop draw its rotations and resampling tables on the device
        (ops.eot_draw) instead of on the host: one launch in front of every block of iterations, nothing consumed from
        Python's `random`, and from torch's CPU generator only the start noise. The stream is the library's own function
        of (seed, draw index, view) — the reference's distributions, not its draws — where iteration `it` of binary step
        `bs` has draw index `draw_base + bs * num_iter + it`; `draw_base` (public, 0 at construction) advances by
        binary_step * num_iter at the end of every device-drawn attack(), and setting it back reproduces a run.
        `seed=None` takes torch.initial_seed() at the first use. It takes effect only where the device loop runs with
        views; `last_draws` says what the last attack() did: "device", "host" or None (no views).

        `sample_seeds` (one int per sample of the batch handed to attack(); None: one batch-shaped draw from torch's global
        CPU generator, as the reference) draws each sample's 1e-7 start noise from its own CPU generator, and `global_batch`
        (None: the batch handed to attack()) is the size of the batch whose `.mean()` the losses belong to — it takes effect
        in the device loop; both as in attack/CW/CW_attack.py: with them a sample's trajectory does not depend on the batch
        it is attacked in."""
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.model = model.to(self.device)
        self.model.eval()
        self.model = _graphed.wrap(self.model, enable=graph)   # hipGraph replay for deterministic victims
        self.adv_func = adv_func
        self.dist_func = dist_func
        self.attack_lr = attack_lr
        self.init_weight = init_weight
        self.max_weight = max_weight
        self.binary_step = binary_step
        self.num_iter = num_iter
        self.whether_target = whether_target
        self.whether_1d = whether_1d
        self.whether_renormalization = whether_renormalization
        self.whether_3Dtransform = whether_3Dtransform
        self.box_constraint = 0.4
        self.whether_resample = whether_resample
        self.verbose = verbose
        self.graph = graph
        self.device_loop = device_loop
        self.device_rng = bool(device_rng)
        self.seed = seed
        self.sample_seeds = sample_seeds
        self.global_batch = global_batch
        self.draw_base = 0
        self.last_path = None
        self.last_draws = None                 # who drew the last attack()'s views: "device", "host" or None (no views)
        self.draw_seconds = 0.0                # host time the last device-loop attack() spent drawing rotations / indices
        self._loop_cache = _graphed.LoopCache(1)    # the device loop (buffers and captured graphs), kept from call to call

    def _forward(self, x):
        return _graphed.logits_of(self.model(x))

    # ---- device loop (PointNet victim + own functors): no autograd, ONE stacked victim pass, replayed from hipGraphs ----
    EOT_VIEWS = 10       # :193 — the expectation's ten views
    LOOP_BLOCK = 16      # iterations per graph replay = per block of host draws; the remainder replays single iterations

    def _device_loop_plan(self, B, K, ragged=False):
        """The constants of the device loop when it applies, else None: a GPU victim with fused_attack_grad (the two
        PointNetCls variants), an AdvLossAdapter around functors the CW loop maps to ops.LOSS_KINDS, ChamferDist('adv2ori')
        or L2Dist — inside PerSampleDist, or bare at B = 1 where the batch mean is the identity — and a cloud the kernels
        hold. ChamferkNNDist and arbitrary callables take the autograd path. `ragged`: the plan of a batch of clouds of
        different sizes (the flag enters the loop's key; the lengths never do). A `global_batch` adds the entry
        "batch_mean" and sets the tail's scale; without one the plan is what it always was."""
        from ..CW.CW_utils import adv_utils as _adv_utils
        from ..CW.CW_utils import dist_utils as _dist_utils
        victim = _graphed.unwrap(self.model)
        if self.device.type != "cuda" or not hasattr(victim, "fused_attack_grad") or K > ops.EOT_MAX_POINTS:
            return None
        if next(victim.parameters()).device.type != "cuda":
            return None
        if type(self.adv_func) is not AdvLossAdapter:
            return None
        af = self.adv_func.targeted_func if self.whether_target else self.adv_func.untargeted_func
        kind = _adv_utils.own_adv_kind(af)
        if kind is None:
            return None
        df = self.dist_func
        if type(df) is PerSampleDist:
            df = df.functor
        elif B != 1:
            return None
        if type(df) is _dist_utils.ChamferDist and df.method == 'adv2ori':
            dist_kind = "chamfer"
        elif type(df) is _dist_utils.L2Dist:
            dist_kind = "l2"
        else:
            return None
        E = self.EOT_VIEWS if self.whether_3Dtransform else 0
        renorm = bool(self.whether_renormalization)
        G = int(self.global_batch) if self.global_batch else B
        plan = dict(victim=victim, kind=kind, dist_kind=dist_kind, E=E, renorm=renorm,
                    resample=bool(E and self.whether_resample), prepare=bool(E or renorm), one_d=bool(self.whether_1d),
                    untarget=not self.whether_target, box=float(self.box_constraint), scale=1.0 / ((E if E else 1) * G))
        if self.global_batch:
            plan["batch_mean"] = G
        if ragged:
            plan["ragged"] = True
        return plan

    def _loop_key(self, plan, B, K):
        """The key of the loop of this shape, these constants, this kernel flavour and these weights. A ragged plan carries
        its flag, never the lengths: they are device data of the launches."""
        device_draws = bool(self.device_rng and plan["E"])
        return _graphed.loop_key(plan["victim"], self.device, B, K, float(self.attack_lr), device_draws,
                                 int(self.seed) if device_draws else None, bool(self.graph),
                                 tuple(sorted((n, v) for n, v in plan.items() if n != "victim")))

    def _device_loop_state(self, plan, B, K):
        """The loop of this shape, these constants, this kernel flavour and these weights: its buffers (static: the graphs
        point at them), the iteration body and, once captured, the graphs — the last one is kept from call to call."""
        victim, dev, lr = plan["victim"], self.device, self.attack_lr
        device_draws = bool(self.device_rng and plan["E"])
        if device_draws and self.seed is None:
            self.seed = int(torch.initial_seed()) & 0x7FFFFFFFFFFFFFFF
        key = self._loop_key(plan, B, K)
        loop = self._loop_cache.get(key)
        if loop is not None:
            return loop
        E, LB = plan["E"], self.LOOP_BLOCK
        S, T = 1 + E, 2 * LB
        f32, i32, i64 = (dict(dtype=t, device=dev) for t in (torch.float32, torch.int32, torch.long))
        adv, ori, m, v, o_bestattack, input_val = (torch.zeros((B, 3, K), **f32) for _ in range(6))
        X = torch.zeros((S * B, 3, K), **f32) if plan["prepare"] else None
        stats = torch.zeros((S * B, 4), **f32) if plan["prepare"] else None
        arg = torch.zeros((S * B,), **i32) if plan["prepare"] else None
        # the per-iteration tables: T = two blocks of rows on the device, two pinned blocks on the host (none of those when
        # the device draws)
        rot = torch.zeros((T, E, 3, 3), **f32) if E else None
        ragged = bool(plan.get("ragged"))
        # (ragged: a table per cloud, a cloud of another length draws other columns; attack() has refused host draws)
        idx = torch.zeros((T, E, B, K) if ragged else (T, E, K), **i32) if plan["resample"] else None
        inv = torch.zeros((T, E, B, K, 2) if ragged else (T, E, K, 2), **i32) if plan["resample"] else None
        host_draws = bool(E) and not device_draws
        rot_pin = torch.zeros((2, LB, E, 3, 3), dtype=torch.float32).pin_memory() if host_draws else None
        idx_pin = torch.zeros((2, LB, E, K), dtype=torch.int32).pin_memory() if host_draws and plan["resample"] else None
        inv_pin = torch.zeros((2, LB, E, K, 2), dtype=torch.int32).pin_memory() if host_draws and plan["resample"] else None
        chamfer = plan["dist_kind"] == "chamfer"
        nn_d = torch.zeros((B, K), **f32) if chamfer else None
        nn_idx = torch.zeros((B, K), **i32) if chamfer else None
        step = torch.zeros((1,), **i32)
        pred, goal_s, goal = torch.zeros((S * B,), **i64), torch.zeros((S * B,), **i64), torch.zeros((B,), **i64)
        w, bestdist, o_bestdist = (torch.zeros((B,), **f32) for _ in range(3))
        bestscore, o_bestscore = (torch.zeros((B,), **i64) for _ in range(2))
        kind, kappa = plan["kind"]
        # ragged: the lengths the launches read as data, and beside them the same lengths once per slot for the victim's
        # stacked pass; every call refills all three in place
        lens, lens_host = _ragged.loop_lengths(B, K, dev) if ragged else (None, None)
        lens_s = torch.full((S * B,), K, **i32) if ragged else None
        vkw = _ragged.victim_kwargs(victim, lens_s)
        batch_mean = plan.get("batch_mean", B)

        def body():
            # one chain on one stream: the stacked input, the victim's passes on it (the classifier tail advances the step
            # word), the adv -> ori search, the update
            with torch.no_grad():
                x_in = adv
                if plan["prepare"]:
                    ops.eot_prepare(adv, ori, rot, idx, plan["renorm"], step, out=X, stats=stats, arg=arg, lengths=lens)
                    x_in = X
                _, _, gx = victim.fused_attack_grad(x_in, goal_s, kind, kappa, pred_out=pred, step=step, scale=plan["scale"],
                                                    **vkw)
                if chamfer:
                    ops.nn_search_into(adv, ori, nn_d, nn_idx)
                ops.eot_update(adv, ori, gx, m, v, step, lr, pred, goal, plan["untarget"], bestdist, bestscore,
                               o_bestdist, o_bestscore, o_bestattack, rot=rot, inv=inv, renorm=plan["renorm"], stats=stats,
                               arg=arg, input_val=input_val, dist_kind=plan["dist_kind"], w=w, nn_idx=nn_idx,
                               batch_mean=batch_mean, one_d=plan["one_d"], box=plan["box"], lengths=lens)

        bufs = dict(plan=plan, device_draws=device_draws, adv=adv, ori=ori, m=m, v=v, o_bestattack=o_bestattack,
                    input_val=input_val, X=X, stats=stats, arg=arg, rot=rot, idx=idx, inv=inv, rot_pin=rot_pin, idx_pin=idx_pin,
                    inv_pin=inv_pin, nn_d=nn_d, nn_idx=nn_idx, step=step, pred=pred, goal_s=goal_s, goal=goal, w=w,
                    bestdist=bestdist, o_bestdist=o_bestdist, bestscore=bestscore, o_bestscore=o_bestscore,
                    lens=lens, lens_host=lens_host, lens_s=lens_s,
                    uploaded=[torch.cuda.Event(), torch.cuda.Event()])
        return self._loop_cache.put(key, _graphed.DeviceLoop(key, dev, owners=(victim,), counts=(1, self.LOOP_BLOCK),
                                                             warmup=2, body=body, bufs=bufs))

    def _draw_block(self, c, half, count, K):
        """`count` iterations' rotations (and resampling indices with their inverse tables) into pinned block `half`, in
        the order the autograd path draws them: per view torch.randn(1), random.random(), random.sample(range(1, 2K), K)."""
        t0 = time.perf_counter()
        rot = c["rot_pin"].numpy()
        idx = c["idx_pin"].numpy() if c["idx_pin"] is not None else None
        inv = c["inv_pin"].numpy() if c["inv_pin"] is not None else None
        for it in range(count):
            for e in range(c["plan"]["E"]):
                rot[half, it, e] = _rotation_draw()
                if idx is not None:
                    idx[half, it, e] = random.sample(range(1, K * 2), K)
                    _inverse_columns(idx[half, it, e] % K, K, inv[half, it, e])
        self.draw_seconds += time.perf_counter() - t0

    def _run_iterations(self, loop, K, binary_step=0):
        """One binary-search step's num_iter iterations: block n of LOOP_BLOCK iterations reads rows (n mod 2) LOOP_BLOCK ...
        of the tables (the step word counts from 0); its draws are uploaded in front of its replay, and the next block's
        are made while it runs — never more than num_iter * EOT_VIEWS sets per step. With device draws the block's rows
        are filled by ONE launch on the current stream in front of its replay (outside the graph: the host knows the draw
        index), and the host neither draws nor waits."""
        c = loop.bufs
        LB, E = self.LOOP_BLOCK, c["plan"]["E"]
        left = self.num_iter
        host_draws = bool(E) and not c["device_draws"]
        n0 = self.draw_base + binary_step * self.num_iter      # the block's first draw index (device draws)
        if host_draws and left:
            c["uploaded"][0].synchronize()
            self._draw_block(c, 0, min(LB, left), K)
        n = 0
        while left > 0:
            cnt, half = min(LB, left), n % 2
            if c["device_draws"]:
                # (the rotations do not depend on a length: without resampling a ragged loop takes the dense launch)
                ops.eot_draw(self.seed, n0, (half * LB, cnt), c["rot"], c["idx"], c["inv"],
                             lengths=c["lens"] if c["idx"] is not None else None)
                n0 += cnt
            elif E:
                rows = slice(half * LB, half * LB + cnt)
                for nm in ("rot", "idx", "inv"):
                    if c[nm] is not None:
                        c[nm][rows].copy_(c[nm + "_pin"][half, :cnt], non_blocking=True)
                c["uploaded"][half].record()
            loop.run(cnt)
            left -= cnt
            n += 1
            if host_draws and left:
                c["uploaded"][n % 2].synchronize()      # the pinned block about to be rewritten has been read
                self._draw_block(c, n % 2, min(LB, left), K)

    def _attack_device_loop(self, plan, adv_data, ori_data, goal, B, K, lens=None):
        dev = self.device
        loop = self._device_loop_state(plan, B, K)
        c = loop.bufs
        S = 1 + plan["E"]
        if lens is not None:
            _ragged.set_loop_lengths(c, lens)
            c["lens_s"].copy_(c["lens"].repeat(S))
        lower_bound = np.zeros((B,))
        upper_bound = np.ones((B,)) * self.max_weight
        current_weight = np.ones((B,)) * self.init_weight
        self.draw_seconds = 0.0

        def begin_step():
            c["bestdist"].fill_(1e10), c["bestscore"].fill_(-1)
            c["m"].zero_(), c["v"].zero_(), c["step"].zero_()

        def rewind():
            c["adv"].copy_(adv_data), c["input_val"].copy_(adv_data)
            c["o_bestdist"].fill_(1e10), c["o_bestscore"].fill_(-1), c["o_bestattack"].zero_()
            begin_step()

        with torch.no_grad():
            c["ori"].copy_(ori_data)
            c["goal"].copy_(goal)
            c["goal_s"].copy_(goal.repeat(S))
            c["w"].fill_(float(self.init_weight))
            rewind()
            if self.graph and self.num_iter > 0 and self.binary_step > 0:
                loop.capture(rewind)
            goal_np = goal.cpu().numpy()
            for binary_step in range(self.binary_step):
                begin_step()
                c["w"].copy_(ops.h2d(torch.from_numpy(current_weight).float(), dev))
                self._run_iterations(loop, K, binary_step)
                # adjust weight factor (:283-303) — one host read per binary-search step
                bs, bd, obd = c["bestscore"].cpu().numpy(), c["bestdist"].cpu().numpy(), c["o_bestdist"].cpu().numpy()
                hit = (bs == goal_np) if self.whether_target else (bs != goal_np)
                bisect_weights(lower_bound, upper_bound, current_weight, hit & (bs != -1) & (bd <= obd))
            fail_idx = torch.from_numpy(lower_bound == 0.).to(dev)
            o_bestattack = torch.where(fail_idx[:, None, None], c["input_val"], c["o_bestattack"])
            o_bestdist = c["o_bestdist"].double()
        if c["device_draws"]:
            self.draw_base += self.binary_step * self.num_iter      # the next batch sees other draws
        success_num = int((lower_bound > 0.).sum())
        if self.verbose:
            print('Successfully attack {}/{}   pred: {}'.format(success_num, B, c["pred"][:B].tolist()))
        return (o_bestdist.cpu().numpy(), o_bestattack.double().cpu().numpy().transpose((0, 2, 1)), success_num)

    def _ragged_lengths(self, data, lengths):
        """lengths as int64 numpy [B] after every check of the ragged pass, or ValueError naming what does not fit, before
        any launch: there is no silent fall-back, since a pass that does not know the lengths would centre, resample and
        average over the padding."""
        who = "CW.attack(lengths=...)"
        if not self.device_loop:
            raise ValueError(f"{who}: device_loop=False has no ragged pass (the autograd path does not know lengths)")
        victim = _graphed.unwrap(self.model)
        if not getattr(victim, "pad_invariant", False) or not hasattr(victim, "fused_attack_grad"):
            raise ValueError(f"{who}: the victim {type(victim).__name__} does not declare pad_invariant or lacks the fused "
                             "entry points (fused_attack_grad)")
        if self.whether_3Dtransform and self.whether_resample and not self.device_rng:
            raise ValueError(f"{who}: whether_resample needs device_rng=True (per-cloud tables drawn on the host would consume "
                             "`random` in an order the reference does not define)")
        if data.dim() != 3 or data.shape[2] != 3:
            raise ValueError(f"{who}: data must be [B, Kmax, 3], got {tuple(data.shape)}")
        B, K = data.shape[:2]
        if K > ops.EOT_MAX_POINTS:
            raise ValueError(f"{who}: Kmax={K} exceeds EOT_MAX_POINTS={ops.EOT_MAX_POINTS}")
        lens = _ragged.check_lengths(who, lengths, B, K, low=1)
        if self._device_loop_plan(B, K, ragged=True) is None:
            raise ValueError(f"{who}: no device-loop plan (it needs a GPU victim, an AdvLossAdapter around this package's "
                             "adversarial functors and PerSampleDist around ChamferDist('adv2ori') or L2Dist)")
        return lens

    def attack(self, data, target=torch.Tensor([0]), origin_label=torch.Tensor([105]), lengths=None):
        """data [B,K,3] (or [B,3,K]); target [B] (targeted) / origin_label [B] (untargeted).
        Returns (o_bestdist [B] float64, o_bestattack [B,K,3] float64, success_num) like the reference (:321).

        lengths (default None: every cloud has K points, nothing changes): a sequence, array or tensor of B ints,
        1 <= lengths[b] <= Kmax = data.shape[1], the sizes of a batch [B,Kmax,3] of clouds of different sizes; rows of data at
        and beyond a cloud's length are ignored (dataset.cloud_io.stack_ragged builds such a batch, unstack_ragged takes the
        result apart). It needs device_loop=True with a plan, a pad_invariant victim and, for whether_resample,
        device_rng=True; anything else raises ValueError before any launch. With `sample_seeds` and `global_batch` = B every
        cloud is attacked exactly as in a run of that cloud alone (same seed, draw_base and global_batch). In the returned
        o_bestattack [B,Kmax,3], rows at and beyond a cloud's length hold that cloud's row 0."""
        dev = self.device
        lens = None if lengths is None else self._ragged_lengths(data, lengths)
        if data.shape[2] == 3:
            data = data.transpose(1, 2).contiguous()
        B, _, K = data.shape
        data = data.float().to(dev).detach()
        ori_data = data.clone().detach()
        lens_dev = None
        if lens is not None:
            lens_dev = torch.from_numpy(lens.astype(np.int32)).to(dev)
            ops.pad_ragged(ori_data, lens_dev)
        target = target.long().to(dev).detach().view(-1)
        origin_label = origin_label.detach().to(dev).long().view(-1)
        if target.numel() == 1 and B > 1:
            target = target.expand(B)
        if origin_label.numel() == 1 and B > 1:
            origin_label = origin_label.expand(B)
        goal = target if self.whether_target else origin_label

        lower_bound = np.zeros((B,))
        upper_bound = np.ones((B,)) * self.max_weight
        current_weight = np.ones((B,)) * self.init_weight

        o_bestdist = torch.full((B,), 1e10, dtype=torch.float64, device=dev)
        o_bestscore = torch.full((B,), -1, dtype=torch.long, device=dev)
        o_bestattack = torch.zeros((B, 3, K), dtype=torch.float32, device=dev)

        with torch.no_grad():
            pred = torch.argmax(self._forward(ori_data), dim=1)
        if self.verbose:
            print('clean pred: {}  goal: {}'.format(pred.tolist(), goal.tolist()))

        # ONE start point for the whole search: later binary steps continue from the previous step's iterate (:88-93)
        if self.sample_seeds is None:
            # (ragged: the batch-shaped draw stays, its padding columns are overwritten below; a cloud's noise then depends
            # on the batch it is in, so this mode is not comparable cloud by cloud with runs alone)
            noise = torch.randn((B, 3, K))
        else:
            assert len(self.sample_seeds) == B, "sample_seeds needs one seed per sample"
            gens = [torch.Generator().manual_seed(int(sd)) for sd in self.sample_seeds]
            noise = _ragged.per_cloud_draw(B, 3, K, [K] * B if lens is None else lens,
                                           lambda b, n: torch.randn((3, n), generator=gens[b]))
        adv_data = ori_data.clone().detach() + noise.to(dev) * 1e-7
        if lens is not None:
            ops.pad_ragged(adv_data, lens_dev)
        plan = self._device_loop_plan(B, K, ragged=lens is not None) if self.device_loop else None
        self.last_path = "device_loop" if plan is not None else "autograd"
        if plan is not None:
            self.last_draws = ("device" if self.device_rng else "host") if plan["E"] else None
        else:
            self.last_draws = "host" if self.whether_3Dtransform else None
        if plan is not None:
            return self._attack_device_loop(plan, adv_data, ori_data, goal, B, K, lens)
        input_val = adv_data.detach().clone()
        for binary_step in range(self.binary_step):
            adv_data.requires_grad_()
            bestdist = torch.full((B,), 1e10, dtype=torch.float64, device=dev)
            bestscore = torch.full((B,), -1, dtype=torch.long, device=dev)
            opt = optim.Adam([adv_data], lr=self.attack_lr, weight_decay=0.)
            weights = torch.from_numpy(current_weight)

            for iteration in range(self.num_iter):
                logits = self._forward(_renormalize(adv_data) if self.whether_renormalization else adv_data)
                pred = torch.argmax(logits, dim=1)
                dist_loss = self.dist_func(adv_data.permute(0, 2, 1), ori_data.permute(0, 2, 1), weights)

                # record values (device side; reference :155-182)
                with torch.no_grad():
                    dist_val = dist_loss.detach().double().reshape(-1).expand(B)
                    succ = (pred == goal) if self.whether_target else (pred != goal)
                    upd = succ & (dist_val < bestdist)
                    bestdist = torch.where(upd, dist_val, bestdist)
                    bestscore = torch.where(upd, pred, bestscore)
                    upd_o = succ & (dist_val < o_bestdist)
                    o_bestdist = torch.where(upd_o, dist_val, o_bestdist)
                    o_bestscore = torch.where(upd_o, pred, o_bestscore)
                    input_val = adv_data.detach().clone()
                    o_bestattack = torch.where(upd_o[:, None, None], input_val, o_bestattack)
                dist_loss = dist_loss.mean()

                wt = 1 if self.whether_target else 0
                if self.whether_3Dtransform:
                    # expectation over 10 random small rotations of the CLEAN cloud carrying the same perturbation
                    diff = adv_data - ori_data.detach()
                    losses = []
                    for _ in range(10):
                        Tr = _small_rotation(dev)
                        x = torch.bmm(Tr.expand(B, -1, -1), ori_data.detach()) + diff
                        if self.whether_renormalization:
                            x = _renormalize(x)
                        if self.whether_resample:
                            # the cloud twice, K of its 2K columns drawn without replacement (:236-239: index 0 excluded)
                            indices = random.sample(range(1, K * 2), K)
                            x = torch.index_select(torch.cat((x, x), 2), 2, ops.h2d(torch.tensor(indices, dtype=torch.long), dev))
                        losses.append(self.adv_func(self._forward(x), goal, whether_target=wt).mean())
                    adv_loss = torch.mean(torch.stack(losses))
                else:
                    adv_loss = self.adv_func(logits, goal, whether_target=wt).mean()
                loss = adv_loss + dist_loss
                if self.verbose and iteration % 10 == 0:
                    print('Step {}, iteration {}, success {}/{}  adv_loss: {:.4f}, dist_loss: {:.4f}'.format(
                        binary_step, iteration, int(succ.sum()), B, float(adv_loss), float(dist_loss)))

                opt.zero_grad()
                loss.backward()
                opt.step()

                if self.whether_1d:
                    # attack on the z direction only, inside a +-0.4 box (:266-275)
                    with torch.no_grad():
                        adv_data[:, 0] = ori_data[:, 0]
                        adv_data[:, 1] = ori_data[:, 1]
                        adv_data[:, 2] = torch.max(torch.min(adv_data[:, 2], ori_data[:, 2] + self.box_constraint),
                                                   ori_data[:, 2] - self.box_constraint)

            # adjust weight factor (:283-303) — one host read per binary-search step
            bs, bd, obd = bestscore.cpu().numpy(), bestdist.cpu().numpy(), o_bestdist.cpu().numpy()
            goal_np = goal.cpu().numpy()
            hit = (bs == goal_np) if self.whether_target else (bs != goal_np)
            bisect_weights(lower_bound, upper_bound, current_weight, hit & (bs != -1) & (bd <= obd))

        # fail to attack some examples: assign them the iterate the last pass started from (:309-310)
        fail_idx = torch.from_numpy(lower_bound == 0.).to(dev)
        o_bestattack = torch.where(fail_idx[:, None, None], input_val, o_bestattack)
        success_num = int((lower_bound > 0.).sum())
        if self.verbose:
            print('Successfully attack {}/{}   pred: {}'.format(success_num, B, pred.tolist()))
        return (o_bestdist.cpu().numpy(), o_bestattack.double().cpu().numpy().transpose((0, 2, 1)), success_num)
