"""SI-Adv: the shape-invariant white-box attack (I-FGM) and the three query attacks — MI355X mirror of the reference's
``attack/SIadv/SIadv_attack.py``.

White box (``ifgm_ours``). Every point moves only inside its tangent plane: with the normal n the point is taken to the
frame P' = U (P + (P.n) n), the surrogate's gradient is taken there, its component along the normal is dropped, P' makes
an L2-normalised step and goes back, P = U^T P' - (P.n) n, followed by the clamp to the eps box; then the normals are
estimated again. The reference runs one cloud at a time and re-estimates the normals with open3d on the host in every
step. ``PointCloudAttack`` runs a batch and stays on the device: per step one self-kNN search (K = 20, hinted by the
previous step's lists), ``pc3d_si_frame_f32`` (the PCA normals from the lists and the cloud U^T (U (P + t)) - t the
reference shows the victim), the surrogate's passes, and ``pc3d_si_step_f32`` (the step). The loop has no data-dependent
exit, so with a PointNet surrogate (fused passes, no autograd) the step is captured into a hipGraph and replayed. Any
other surrogate, a defence head or the top-5 loss take autograd for the gradient and the same two kernels.
``run(points, target, lengths)`` runs the fast path on a batch of clouds of different sizes: every cloud
gets the bits of its run alone, launch for launch the dense step with the search, the frame and the step in their
``_ragged`` forms; anything but the fast path raises.

Black box (``simba``, ``simbapp``, ``ours``: ``simba_attack``, ``simbapp_attack``, ``shape_invariant_query_attack``). The
reference queries the target once per signed try of one table entry of one cloud and reads the loss back each time. Here
all clouds of a batch advance together: a step is ONE forward of the 2B candidate clouds (both signed tries of every
cloud) and one launch of ``pc3d_query_step_f32``, which takes the reference's decision per cloud (try 0, and only if it
was rejected try 1; strict >; query_costs + 1 or + 2), puts the accepted change into the state, latches the clouds whose
loop has ended and writes the candidates of the next entry. With a PointNet target and no defence head the step is
captured into a hipGraph; the host reads the latches back every 16 steps. The tables come first: ``simba``'s shuffled
basis lists are drawn on the host exactly as the reference draws them (``draw_simba_tables``); ``simbapp``'s choices and
amounts are drawn once per batch on the device from the caller's generator (parity unpinned: the reference's body cannot
run); ``ours`` ranks the points by the surrogate's gradient in the tangent frame (``pc3d_si_rank_f32``).

Kept on purpose: the spin-axis matrix as written, including its rows for |n_z^2 - 1| < 1e-4, which
are not the frame of n — so the victim sees those points displaced by up to 1e-4, which a PointNet's max-pool can
amplify; sqrt(3 * 1024) in the step whatever N is; the loss summed over the batch; in the query attacks the returned
cloud of ``ours`` (the last candidate evaluated, accepted or not), the top-5 rule on the last logits evaluated, strict >
and kappa = -999. Not kept: the checkpoint loading of ``build_models`` (the models are handed in), ``assert
abs(normal_vec).max() <= 1`` (a host round trip), the normal estimation after the last step (never used), and the two
shuffled re-evaluations with their prints at the end of ``shape_invariant_query_attack`` (they change no result).
"""
import numpy as np
import torch

from ... import graphed as _graphed
from ... import ops
from ... import ragged as _ragged
from ...model import pointnet as _pointnet
from .baselines import ClipPointsLinf, DUPNet, SORDefense, SRSDefense

KNN = 20                                  # open3d.geometry.KDTreeSearchParamKNN(knn=20), SIadv_attack.py:212
QUERY_METHODS = ("simba", "simbapp", "ours")
_MAX_LOOPS = 4
POLL = 16                                 # query loops: steps per graph replay, and between two reads of the latches
_QUERY_NAMES = {"simba": "simba_attack", "simbapp": "simbapp_attack", "ours": "shape_invariant_query_attack"}


def _first(out):
    return out[0] if isinstance(out, (tuple, list)) else out


class _Loop(_graphed.DeviceLoop):
    """The fast path's loop for one batch shape: static buffers, one step as the body, captured as one step.
    ragged: a batch of clouds of different sizes, N the capacity. The lengths are DATA of the launches (bufs "lens", and
    "lens_host" for the search wrapper's check; every call refills them), so one captured graph serves every set of
    lengths; the search writes the loop's own d / idx [B,N,KNN], idx also being its hint. The step is the dense step launch
    for launch: the search over every cloud's own points, the frame, whose xe repeats its row 0 in the padding rows (the
    surrogate is pad_invariant, or skips them: ragged.victim_kwargs), and the step, which pads the new iterate."""

    def __init__(self, victim, B, N, dev, step_size, eps, key=None, ragged=False):
        # the graph bakes in the addresses of the folded weights: it holds what it points at (LoopGraph.keep)
        super().__init__(key, dev, owners=(victim,), counts=(1,), warmup=2)
        self.victim, self.step_size, self.eps, self.ragged = victim, float(step_size), float(eps), bool(ragged)
        f32 = dict(dtype=torch.float32, device=dev)
        self.bufs.update({nm: torch.zeros((B, 3, N), **f32) for nm in ("x", "ori", "xe", "nrm")},
                         label=torch.zeros((B,), dtype=torch.int64, device=dev), lens=None, lens_host=None)
        if self.ragged:
            lens, lens_host = _ragged.loop_lengths(B, N, dev)
            self.bufs.update(lens=lens, lens_host=lens_host, d=torch.zeros((B, N, KNN), **f32),
                             idx=torch.zeros((B, N, KNN), dtype=torch.int32, device=dev))
        self.vlens = _ragged.victim_kwargs(victim, self.bufs["lens"])

    def load(self, x, ori, label, nrm=None, lens=None):
        """The call's state. Ragged (lens: int64 numpy [B]): the lengths first, then x, ori and the given normals (kept in
        the loop's own nrm) with their rows at and beyond a length made copies of row 0."""
        b = self.bufs
        b["x"].copy_(x), b["ori"].copy_(ori), b["label"].copy_(label)
        if self.ragged:
            _ragged.set_loop_lengths(b, lens)
            if nrm is not None:
                b["nrm"].copy_(nrm)
            for nm in ("x", "ori") + (("nrm",) if nrm is not None else ()):
                ops.pad_ragged(b[nm], b["lens"])

    def _move(self, nrm):
        # the victim is shown xe (si_frame), as in the reference; its loss is summed over the batch, not averaged: scale 1
        b = self.bufs
        g = self.victim.fused_attack_grad(b["xe"], b["label"], "untargeted_logits", 0.0, scale=1.0, **self.vlens)[2]
        ops.si_step(b["x"], b["ori"], g, self.step_size, self.eps, nrm=nrm, lengths=b["lens"])

    def first(self, nrm):
        """Step 0: the normals that came with the cloud (ragged: the loop's own copy of them, see load)."""
        nrm = self.bufs["nrm"] if self.ragged else nrm
        ops.si_frame(self.bufs["x"], nrm=nrm, out=self.bufs["xe"], lengths=self.bufs["lens"])
        self._move(nrm)

    def step(self):
        b = self.bufs
        if self.ragged:
            idx = ops.knn_search_into(b["x"], b["d"], b["idx"], lengths=b["lens"], lengths_host=b["lens_host"])[1]
        else:
            _, idx = ops.knn_raw(b["x"], b["x"], KNN, q_cf=True, r_cf=True)
        ops.si_frame(b["x"], idx=idx, out=b["xe"], nrm_out=b["nrm"], lengths=b["lens"])
        self._move(b["nrm"])

    body = step


def simba_basis(N):
    """basis_list of simba_attack before its shuffle (SIadv_attack.py:371-375): [3N,2] rows (channel, idx), in the
    reference's loop order (the point index outermost)."""
    basis_list = []
    for j in range(N):
        for i in range(3):
            basis_list.append((i, j))
    return np.array(basis_list)


def draw_simba_tables(N, active):
    """The tables of simba_attack for a batch, drawn as the reference draws them: one np.random.shuffle of the [3N,2]
    basis list per cloud, in cloud order, and only for the clouds that did not return early (active[b] true).
    Returns int32 [B,3N]: entry 3 * idx + channel (zeros for a cloud that returned early)."""
    tab = np.zeros((len(active), 3 * N), np.int32)
    for b, on in enumerate(active):
        if on:
            basis_list = simba_basis(N)
            np.random.shuffle(basis_list)
            tab[b] = 3 * basis_list[:, 1] + basis_list[:, 0]
    return tab


def sign_order(step_size):
    """The two signs in the order the reference's ``for eps in {step_size, -step_size}`` visits them."""
    return tuple({step_size, -step_size})


class _QueryLoop(_graphed.DeviceLoop):
    """The query loops' loop for one batch shape: static buffers, POLL steps as the body, captured as one such round.
    classifier / pre_head / top5: the attack's, handed in (the loop does not hold the attack, which holds the loop).
    frame: the shape-invariant mode (the state is P', a candidate is the whole cloud U^T (P' + pert) - t)."""

    def __init__(self, classifier, pre_head, top5, B, N, L, k, dev, frame, table_eps, fast, key=None):
        super().__init__(key, dev, owners=(classifier,), counts=(1,), warmup=1)
        self.classifier, self.pre_head, self.fast, self.L = classifier, pre_head, fast, L
        f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
        s = self.bufs
        s["top"] = 5 if top5 else 1
        s["st"], s["last"] = torch.zeros((B, 3, N), **f32), torch.zeros((B, 3, N), **f32)
        s["cand"] = torch.zeros((2 * B, 3, N), **f32)
        s["ori"], s["nrm"], s["dir"] = ((torch.zeros((B, 3, N), **f32), torch.zeros((B, 3, N), **f32),
                                         torch.zeros((B, N, 3), **f32)) if frame else (None, None, None))
        s["tab"] = torch.zeros((B, L), **i32)
        s["eps"] = torch.zeros((B, L, 2) if table_eps else (2,), **f32)
        for nm in ("pos", "done", "queries", "adv_target", "last_try"):
            s[nm] = torch.zeros((B,), **i32)
        s["best"] = torch.zeros((B,), **f32)
        s["label"] = torch.zeros((B,), dtype=torch.int64, device=dev)
        s["last_logp"] = torch.zeros((B, k), **f32)
        s["acc_trace"], s["loss_trace"] = torch.zeros((B, L), **i32), torch.zeros((B, L, 2), **f32)

    def load(self, x, label, tab, eps, active, adv_target0, logp0, nrm=None, dirs=None):
        """The clean clouds x [B,3,N], the tables, the clouds whose loop runs, and the initial query's outcome; then the
        first candidates."""
        s = self.bufs
        s["tab"].copy_(tab), s["eps"].copy_(eps), s["label"].copy_(label)
        s["pos"].zero_(), s["queries"].fill_(1), s["last_try"].zero_(), s["best"].fill_(-999.)
        s["done"].copy_(~active), s["adv_target"].copy_(adv_target0), s["last_logp"].copy_(logp0)
        s["acc_trace"].fill_(-2), s["loss_trace"].fill_(float("nan"))
        s["last"].copy_(x)
        if s["nrm"] is not None:
            s["ori"].copy_(x), s["nrm"].copy_(nrm), s["dir"].copy_(dirs)
        else:
            s["st"].copy_(x)
        ops.query_step(s, init=True)

    def step(self):
        cand = self.bufs["cand"]
        if self.fast:
            logp = torch.log_softmax(_pointnet.fused_forward(self.classifier, cand)[0], dim=1)
        else:
            logp = _first(self.classifier(self.pre_head(cand) if self.pre_head is not None else cand)).float().contiguous()
        ops.query_step(self.bufs, logp)

    def body(self):
        for _ in range(POLL):
            self.step()

    def run_polled(self):
        """Rounds of POLL steps until every cloud is latched; the latches come back to the host once per round. A latched
        cloud is left alone by the kernel, so a round may run past the end of the tables."""
        for _ in range((self.L + POLL - 1) // POLL):
            self.run(1)
            if bool(self.bufs["done"].all()):
                break


class PointCloudAttack(object):
    """``PointCloudAttack(args, wb_classifier=None, classifier=None)``: the surrogate and the target are handed in (or
    taken from ``args.wb_classifier`` / ``args.classifier``); args carries eps, step_size, max_steps, num_class,
    top5_attack, defense_method and the attack method (``transfer_attack_method`` or ``query_attack_method``).
    ``run(points [B,N,6], target [B])`` returns (adv_points [B,N,3], adv_target [B], number of misclassified clouds).
    With a query method, ``run(points [B,N,3 or 6], target [B])`` returns (adv_points [B,N,3], adv_target [B] int64,
    query_costs [B] int64).
    ``run(points [B,Kmax,6 or 3], target [B], lengths)`` (the white-box attack only): a batch of clouds of different sizes as
    dataset.cloud_io.stack_ragged builds it, see shape_invariant_ifgm.
    fused / graph: use the models' fused passes when they have them, and replay the step from a hipGraph."""

    def __init__(self, args, wb_classifier=None, classifier=None, fused=True, graph=True):
        self.args = args
        self.device = getattr(args, "device", None)
        self.eps = args.eps
        self.normal = getattr(args, "normal", False)
        self.step_size = args.step_size
        self.num_class = args.num_class
        self.max_steps = args.max_steps
        self.top5_attack = args.top5_attack
        query = getattr(args, "query_attack_method", None)
        self.attack_method = getattr(args, "transfer_attack_method", None) if query is None else query
        wb_classifier = wb_classifier if wb_classifier is not None else getattr(args, "wb_classifier", None)
        classifier = classifier if classifier is not None else getattr(args, "classifier", None)
        if wb_classifier is None or classifier is None:
            raise ValueError("PointCloudAttack: pass the surrogate (wb_classifier) and the target (classifier) models")
        self.wb_classifier = wb_classifier.eval()
        self.classifier = classifier.eval()
        self.defense_method = args.defense_method
        self.pre_head = None
        if self.defense_method is not None:
            self.pre_head = self.get_defense_head(self.defense_method)
        self.fused, self.graph = fused, graph
        self._loops = _graphed.LoopCache(_MAX_LOOPS)
        self._query_loops = _graphed.LoopCache(_MAX_LOOPS)
        self.generator = getattr(args, "generator", None)      # simbapp's draws (a torch.Generator on the clouds' device)
        self.last_query = None                                  # the last query loop's traces (see _query)

    def CWLoss(self, logits, target, kappa=0, tar=False, num_classes=40):
        """Carlini & Wagner loss, summed over the batch (SIadv_attack.py:142-164). logits [B,num_classes], target [B]."""
        target = torch.ones(logits.size(0), dtype=logits.dtype, device=logits.device).mul(target.to(logits.dtype))
        target_one_hot = torch.eye(num_classes, dtype=logits.dtype, device=logits.device)[target.long()]
        real = torch.sum(target_one_hot * logits, 1)
        if not self.top5_attack:
            other = torch.max((1 - target_one_hot) * logits - (target_one_hot * 10000), 1)[0]
        else:
            other = torch.topk((1 - target_one_hot) * logits - (target_one_hot * 10000), 5)[0][:, 4]
        kappa = torch.zeros_like(other).fill_(kappa)
        if tar:
            return torch.sum(torch.max(other - real, kappa))
        return torch.sum(torch.max(real - other, kappa))

    def run(self, points, target, lengths=None):
        """points [B,N,6] (coordinates and normals; the query attacks use the coordinates only), target [B].
        lengths (default None): the sizes of a ragged batch, for the white-box attack only (shape_invariant_ifgm)."""
        if self.attack_method == 'ifgm_ours' or (lengths is not None and self.attack_method in QUERY_METHODS):
            return self.shape_invariant_ifgm(points, target, lengths)
        if self.attack_method == 'simba':
            return self.simba_attack(points, target)
        if self.attack_method == 'simbapp':
            return self.simbapp_attack(points, target)
        if self.attack_method == 'ours':
            return self.shape_invariant_query_attack(points, target)
        raise NotImplementedError(f"PointCloudAttack: unknown attack method {self.attack_method!r}")

    def get_defense_head(self, method):
        """The pre-processing defence in front of both models (SIadv_attack.py:189-202)."""
        if method == 'sor':
            pre_head = SORDefense(k=2, alpha=1.1)
        elif method == 'srs':
            pre_head = SRSDefense(drop_num=500)
        elif method == 'dupnet':
            pre_head = DUPNet(sor_k=2, sor_alpha=1.1, npoint=1024, up_ratio=4)
        else:
            raise NotImplementedError
        return pre_head

    def get_normal_vector(self, points, lengths=None):
        """Normals [B,N,3] of points [B,N,3] on the GPU: the self-kNN search (K = 20, the point included) and the PCA
        normal of every list (pc3d_pca_normal_f32) — the definition open3d documents for
        estimate_normals(KDTreeSearchParamKNN(knn=20)); the sign is this library's.
        lengths (B ints, KNN <= lengths[b] <= N; default None: every cloud has N points): cloud b's first lengths[b] rows
        are searched and get the normals of the cloud alone, the rows behind them (never read) row 0's normal."""
        if points.shape[1] < KNN:
            raise ValueError(f"get_normal_vector: N = {points.shape[1]} points, the {KNN}-neighbour normals need N >= {KNN}")
        points = points.detach().float()
        if lengths is not None:
            lens = _ragged.check_lengths("get_normal_vector", lengths, points.shape[0], points.shape[1], low=KNN, low_text="KNN")
            lens_dev = torch.from_numpy(lens.astype(np.int32)).to(points.device)
            _, idx = ops.knn_ragged(points.contiguous(), points.contiguous(), KNN, lens_dev, lengths_host=lens)
            return ops.pca_normal(points, idx, lengths=lens_dev)
        _, idx = ops.knn_raw(points, points, KNN)
        return ops.pca_normal(points, idx)

    def get_spin_axis_matrix(self, normal_vec):
        """U [B,N,3,3] of normals [B,N,3] (SIadv_attack.py:217-247), the rows for |z^2 - 1| < 1e-4 included."""
        x, y, z = normal_vec[:, :, 0], normal_vec[:, :, 1], normal_vec[:, :, 2]
        u = torch.zeros(normal_vec.shape[:2] + (3, 3), dtype=normal_vec.dtype, device=normal_vec.device)
        denominator = torch.sqrt(1 - z ** 2)
        u[:, :, 0, 0] = y / denominator
        u[:, :, 0, 1] = - x / denominator
        u[:, :, 0, 2] = 0.
        u[:, :, 1, 0] = x * z / denominator
        u[:, :, 1, 1] = y * z / denominator
        u[:, :, 1, 2] = - denominator
        u[:, :, 2] = normal_vec
        # revision for |z| = 1, boundary case
        pos = abs(z ** 2 - 1) < 1e-4
        r = 1 / np.sqrt(2)
        zero = torch.zeros_like(z)
        bound = torch.stack([torch.stack([zero + r, zero - r, zero], -1),
                             torch.stack([z / np.sqrt(2), z / np.sqrt(2), zero], -1),
                             torch.stack([zero, zero, z], -1)], -2)
        return torch.where(pos[:, :, None, None], bound, u).data

    def get_transformed_point_cloud(self, points, normal_vec):
        """(P' = U (P + (P.N) N), U, (P.N) N) for points, normals [B,N,3] (SIadv_attack.py:250-263)."""
        intercept = torch.mul(points, normal_vec).sum(-1, keepdim=True)
        spin_axis_matrix = self.get_spin_axis_matrix(normal_vec)
        translation_matrix = torch.mul(intercept, normal_vec).data
        new_points = (points + translation_matrix).unsqueeze(-1)
        new_points = torch.matmul(spin_axis_matrix, new_points).squeeze(-1).data
        return new_points, spin_axis_matrix, translation_matrix

    def get_original_point_cloud(self, new_points, spin_axis_matrix, translation_matrix):
        """P = U^T P' - (P.N) N (SIadv_attack.py:266-276)."""
        inputs = torch.matmul(spin_axis_matrix.transpose(-1, -2), new_points.unsqueeze(-1))
        inputs = inputs - translation_matrix.unsqueeze(-1)
        return inputs.squeeze(-1)

    # ------------------------------------------------------------------------------------------------------
    def _fast(self):
        return bool(self.fused and self.pre_head is None and not self.top5_attack
                    and hasattr(self.wb_classifier, "fused_attack_grad"))

    def _loop_key(self, device, B, N, ragged=False):
        """The dense loop's key as it always was; a ragged loop's carries the flag, never the lengths."""
        consts = (B, N, float(self.step_size), float(self.eps)) + ((("ragged", True),) if ragged else ())
        return _graphed.loop_key(self.wb_classifier, device, *consts)

    def _loop(self, x, ori, target, nrm=None, lens=None):
        """A loaded _Loop for x [B,3,N]; with graph=True captured once per (shape, settings, weights). lens (int64 numpy
        [B]): the ragged loop of that shape, loaded with these lengths and the given normals nrm."""
        B, _, N = x.shape
        v = self.wb_classifier
        ragged = lens is not None
        state = dict(nrm=nrm, lens=lens) if ragged else {}
        key = self._loop_key(x.device, B, N, ragged) if self.graph else None
        c = self._loops.get(key) if self.graph else None
        if c is None:
            c = _Loop(v, B, N, x.device, self.step_size, self.eps, key, ragged=ragged)
            if self.graph:
                self._loops.put(key, c)
                c.load(x, ori, target, **state)
                c.capture()
        c.load(x, ori, target, **state)
        return c

    def _ragged_lengths(self, points, lengths):
        """lengths as int64 numpy [B] after every gate of the ragged pass, or ValueError naming what does not fit, before
        any launch. There is no silent fall-back: the generic path would count the padding copies of row 0 as neighbours
        (a degenerate covariance and the default normal for row 0 and every point near it), and a surrogate that is not
        pad_invariant would see them as points."""
        who = "shape_invariant_ifgm"
        sur = _graphed.unwrap(self.wb_classifier)
        if self.attack_method in QUERY_METHODS:
            raise ValueError(f"{who}: lengths go with the white-box attack only, not with the query attack "
                             f"'{self.attack_method}'")
        if not self._fast():
            why = ("fused=False" if not self.fused else f"the defence head '{self.defense_method}'" if self.pre_head is not None
                   else "top5_attack" if self.top5_attack
                   else f"the surrogate {type(sur).__name__} has no fused entry points (fused_attack_grad)")
            raise ValueError(f"{who}: lengths run the fast path only ({why} takes the generic path, which has no ragged pass)")
        if not getattr(sur, "pad_invariant", False):
            raise ValueError(f"{who}: the surrogate {type(sur).__name__} does not declare pad_invariant")
        if not isinstance(points, torch.Tensor) or points.dim() != 3 or points.shape[2] not in (3, 6):
            raise ValueError(f"{who}: points must be [B,Kmax,6] (or [B,Kmax,3]), got "
                             f"{tuple(points.shape) if isinstance(points, torch.Tensor) else type(points)}")
        return _ragged.check_lengths(who, lengths, points.shape[0], points.shape[1], low=KNN, low_text="KNN")

    def _generic_grad(self, xe, target):
        """dL/dxe [B,3,N] by autograd through the defence head and the surrogate, at the cloud xe = U^T P' - t that
        si_frame hands over. The reference takes the gradient at P'; the chain rule gives dL/dP' = U dL/dxe, which the
        step kernel forms."""
        P = xe.detach().clone().requires_grad_()
        with torch.enable_grad():
            inp = self.pre_head(P) if self.pre_head is not None else P
            logits = _first(self.wb_classifier(inp))
            loss = self.CWLoss(logits, target, kappa=0., tar=False, num_classes=self.num_class)
            if not loss.requires_grad:           # nothing of the loss depends on the points
                return torch.zeros_like(xe), loss.detach()
            (g,) = torch.autograd.grad(loss, P)
        return g.contiguous(), loss.detach()

    def iterate(self, points, target, steps=None, ori=None, lengths=None):
        """The loop alone: the coordinates [B,3,N] after `steps` (default max_steps) steps from points [B,N,6]. With
        points [B,N,3] (no normals) the first step estimates them like the later ones do. ori [B,N,3]: the clean cloud the
        clamp refers to when the run continues from an iterate (default: the coordinates given).
        lengths (B ints, KNN <= lengths[b] <= N; default None: every cloud has N points): a ragged batch, see
        shape_invariant_ifgm. Columns below a length have the bits of that cloud's run alone, the others equal column 0."""
        lens = self._ragged_lengths(points, lengths) if lengths is not None else None
        steps = self.max_steps if steps is None else steps
        points = points.detach().float()
        B, N, C = points.shape
        if C not in (3, 6):
            raise ValueError(f"shape_invariant_ifgm: points must be [B,N,6] (or [B,N,3]), got {tuple(points.shape)}")
        if N < KNN and (steps > 1 or C == 3):
            raise ValueError(f"shape_invariant_ifgm: N = {N} points, the {KNN}-neighbour normals need N >= {KNN}")
        target = target.detach().reshape(-1).long().to(points.device)
        nrm = None
        if C == 6:
            normal_vec = points[:, :, -3:]
            normal_vec = normal_vec / torch.sqrt(torch.sum(normal_vec ** 2, dim=-1, keepdim=True))
            nrm = normal_vec.transpose(1, 2).contiguous()
        x = points[:, :, :3].transpose(1, 2).contiguous()
        ori = x.clone() if ori is None else ori.detach().float().transpose(1, 2).contiguous()
        if steps < 1:
            return x if lens is None else ops.pad_ragged(x, torch.from_numpy(lens.astype(np.int32)).to(x.device))
        with torch.cuda.device(x.device), torch.no_grad():
            if self._fast():
                c = self._loop(x, ori, target, nrm, lens)
                if nrm is not None:
                    c.first(nrm)
                c.run(steps - (nrm is not None))
                return c.x.clone()
            xe = torch.empty_like(x)
            for i in range(steps):
                if i > 0 or nrm is None:
                    _, idx = ops.knn_raw(x, x, KNN, q_cf=True, r_cf=True)
                    nrm = torch.empty_like(x)
                    ops.si_frame(x, idx=idx, out=xe, nrm_out=nrm)
                else:
                    ops.si_frame(x, nrm=nrm, out=xe)
                g, _ = self._generic_grad(xe, target)
                ops.si_step(x, ori, g, self.step_size, self.eps, nrm=nrm)
        return x

    def shape_invariant_ifgm(self, points, target, lengths=None):
        """White-box I-FGM on shape-invariant sensitivity maps, transferred to the target model.
        points [B,N,6], target [B] -> (adv_points [B,N,3], adv_target [B], number of clouds the target misclassifies).
        lengths (default None: every cloud has N points, nothing changes): B ints (sequence, array or tensor), the sizes of
        a batch of clouds of different sizes, KNN <= lengths[b] <= Kmax = N. Rows of points at and beyond a length may hold
        anything (they are only written); adv_points' are copies of the cloud's row 0 (dataset.cloud_io.unstack_ragged drops
        them). Every cloud gets the bits of its run alone. The fast path only — fused, no defence head, no top-5 loss, a
        surrogate with fused_attack_grad that declares pad_invariant — anything else raises ValueError before any launch.
        A target model that does not declare pad_invariant sees every cloud alone (ragged.predict)."""
        if lengths is not None:
            lens = self._ragged_lengths(points, lengths)
            x = self.iterate(points, target, lengths=lens)
            target = target.detach().reshape(-1).long().to(x.device)
            with torch.no_grad():
                pred = _ragged.predict(self.classifier, x, lens)
            return x.transpose(1, 2).contiguous(), pred, (pred != target).sum().item()
        x = self.iterate(points, target)
        target = target.detach().reshape(-1).long().to(x.device)
        with torch.no_grad():
            inp = self.pre_head(x) if self.pre_head is not None else x
            adv_logits = _first(self.classifier(inp))
            pred = adv_logits.max(1)[1]
            adv_target = pred
            if self.top5_attack:
                in_top5 = (adv_logits.topk(5)[1] == target[:, None]).any(1)
                adv_target = torch.where(in_top5, target, torch.full_like(target, -1))
        return x.transpose(1, 2).contiguous(), adv_target, (pred != target).sum().item()

    # ------------------------------------------------------------------------------------------------------
    # the query attacks
    def _query_prepare(self, points, target, method):
        """Checks, the coordinates x [B,3,N], the labels, and the initial query: (x, target, logp0, adv_target0)."""
        if not isinstance(points, torch.Tensor) or not points.is_cuda:
            raise NotImplementedError(f"PointCloudAttack.{_QUERY_NAMES[method]}: the query attack '{method}' runs on the GPU "
                                      "only (no CPU fallback)")
        points = points.detach().float()
        if points.dim() != 3 or points.shape[2] not in (3, 6):
            raise ValueError(f"{_QUERY_NAMES[method]}: points must be [B,N,3] or [B,N,6], got {tuple(points.shape)}")
        if method == "ours" and points.shape[1] < KNN:
            raise ValueError(f"{_QUERY_NAMES[method]}: N = {points.shape[1]} points, the {KNN}-neighbour normals need N >= {KNN}")
        x = points[:, :, :3].transpose(1, 2).contiguous()
        target = target.detach().reshape(-1).long().to(x.device)
        with torch.no_grad():
            logp0 = _first(self.classifier(self.pre_head(x) if self.pre_head is not None else x)).float()
        adv_target0 = logp0.max(1)[1]
        if self.top5_attack:
            adv_target0 = self._top5_rule(logp0, target)
        return x, target, logp0, adv_target0

    @staticmethod
    def _top5_rule(logits, target):
        in_top5 = (logits.topk(5)[1] == target[:, None]).any(1)
        return torch.where(in_top5, target, torch.full_like(target, -1))

    def _wb_grad(self, x, target):
        """d CWLoss(kappa=-999, tar=True) / dx [B,3,N] of the surrogate at x [B,3,N] (no defence head: the reference hands
        the surrogate the cloud itself). The loss is max(other - real, -999) per cloud, so its gradient on the
        log-probabilities is +1 at `other` and -1 at the label — a row that sums to zero, which the log-softmax's backward
        passes on unchanged: with a fused surrogate the row goes straight into its backward-to-input."""
        sur = self.wb_classifier
        if self.fused and isinstance(sur, _pointnet.PointNetCls):
            with torch.no_grad():
                logits, ctx = _pointnet.fused_forward(sur, x)
                masked = torch.log_softmax(logits, dim=1)
                real = masked.gather(1, target[:, None])[:, 0]
                masked.scatter_(1, target[:, None], -10000.)
                if self.top5_attack:
                    ov, oi = masked.topk(5)
                    ov, oi = ov[:, 4], oi[:, 4]
                else:
                    ov, oi = masked.max(1)
                g = torch.zeros_like(logits)
                g.scatter_(1, oi[:, None], 1.0)
                g.scatter_add_(1, target[:, None], torch.full_like(real, -1.0)[:, None])
                g = (g * ((ov - real) > -999.)[:, None]).contiguous()
                return _pointnet.fused_input_grad(ctx, g)
        P = x.detach().clone().requires_grad_()
        with torch.enable_grad():
            loss = self.CWLoss(_first(sur(P)), target, kappa=-999., tar=True, num_classes=self.num_class)
            if not loss.requires_grad:
                return torch.zeros_like(x)
            (g,) = torch.autograd.grad(loss, P)
        return g.contiguous()

    def _query_fast(self):
        return bool(self.fused and self.pre_head is None and isinstance(self.classifier, _pointnet.PointNetCls))

    def _query_loop(self, B, N, L, k, dev, frame, table_eps):
        fast = self._query_fast()
        cached = fast and self.graph
        key = _graphed.loop_key(self.classifier, dev, B, N, L, k, frame, table_eps, bool(self.top5_attack)) if cached else None
        c = self._query_loops.get(key) if cached else None
        if c is None:
            c = _QueryLoop(self.classifier, self.pre_head, self.top5_attack, B, N, L, k, dev, frame, table_eps, fast, key)
            if cached:
                self._query_loops.put(key, c)
                c.capture()                 # on the zeroed buffers (every table entry 0 is in range); load() follows
        return c

    def _query(self, method, x, target, logp0, adv_target0, active, tab, eps, nrm=None, dirs=None):
        """The loop for prepared tables. tab int32 [B,L], eps float32 [2] or [B,L,2]; active [B] bool: the clouds whose
        loop runs. self.last_query keeps the traces: accepted [B,L] (0 / 1, -1 neither, -2 not reached), losses [B,L,2],
        best [B]."""
        B, _, N = x.shape
        dev = x.device
        tab = torch.as_tensor(tab).to(device=dev, dtype=torch.int32).contiguous()
        eps = torch.as_tensor(eps).to(device=dev, dtype=torch.float32).contiguous()
        L, frame = tab.shape[1], nrm is not None
        if tab.shape[0] != B or L < 1:
            raise ValueError(f"{_QUERY_NAMES[method]}: the table must be [B,L], got {tuple(tab.shape)}")
        with torch.cuda.device(dev), torch.no_grad():
            c = self._query_loop(B, N, L, logp0.shape[1], dev, frame, eps.dim() == 3)
            c.load(x, target, tab, eps, active, adv_target0.to(torch.int32), logp0, nrm, dirs)
            c.run_polled()
            s = c.bufs
            adv_target = s["adv_target"].long()
            if bool((adv_target == -2).any()):
                raise ValueError(f"{_QUERY_NAMES[method]}: a table entry or a label is out of range")
            if self.top5_attack:                  # on the logits of the last candidate evaluated (:406-411, :599-604)
                adv_target = torch.where(active, self._top5_rule(s["last_logp"], target), adv_target)
            out = (s["last"] if frame else s["st"]).transpose(1, 2).contiguous()
            self.last_query = dict(accepted=s["acc_trace"].clone(), losses=s["loss_trace"].clone(), best=s["best"].clone(),
                                   table=tab, eps=eps)
            return out, adv_target, s["queries"].long()

    def simba_attack(self, points, target, table=None):
        """Black-box query-based SimBA attack, batched. points [B,N,3 or 6], target [B] -> (adv_points [B,N,3],
        adv_target [B] int64, query_costs [B] int64). table: int32 [B,3N] of 3 * idx + channel in place of the draw."""
        x, target, logp0, adv_target0 = self._query_prepare(points, target, "simba")
        active = adv_target0 == target                          # the others return the clean cloud at once
        if table is None:
            table = draw_simba_tables(x.shape[2], active.cpu().numpy())
        eps = torch.tensor(sign_order(self.step_size), dtype=torch.float32)
        return self._query("simba", x, target, logp0, adv_target0, active, table, eps)

    def simbapp_attack(self, points, target, table=None, generator=None):
        """Black-box query-based SimBA++ attack, batched (mirrored against its restatement only: the reference's body
        cannot run). The choices Categorical(|g|).sample() and the amounts eps + 0.1 randn are drawn up front, once per
        batch, on the device from `generator` (default: self.generator). table: (choices int32 [B,3N], amounts
        float32 [B,3N,2]) in place of the draw."""
        x, target, logp0, adv_target0 = self._query_prepare(points, target, "simbapp")
        active = adv_target0 == target
        if table is None:
            B, _, N = x.shape
            gen = generator if generator is not None else self.generator
            w = self._wb_grad(x, target).abs().reshape(B, -1)
            w = torch.where(active[:, None], w, torch.ones_like(w))        # a cloud that returned early draws nothing it uses
            choice = torch.multinomial(w, 3 * N, replacement=True, generator=gen).to(torch.int32)
            signs = torch.tensor(sign_order(self.step_size), dtype=torch.float32, device=x.device)
            table = (choice, signs[None, None, :] + 0.1 * torch.randn((B, 3 * N, 2), generator=gen, dtype=torch.float32,
                                                                      device=x.device))
        return self._query("simbapp", x, target, logp0, adv_target0, active, table[0], table[1])

    def query_sensitivity(self, x, target):
        """The sensitivity map of the shape-invariant query attack for clouds x [B,3,N]: (nrm [B,3,N], order int32 [B,N],
        dir [B,N,3], key [B,N]). The normals come from the coordinates (get_normal_vector), the gradient is the surrogate's
        at the clamped cloud U^T P' - t, taken to the frame and ranked by pc3d_si_rank_f32."""
        normal_vec = self.get_normal_vector(x.transpose(1, 2))
        normal_vec = normal_vec / torch.sqrt(torch.sum(normal_vec ** 2, dim=-1, keepdim=True))
        nrm = normal_vec.transpose(1, 2).contiguous()
        xe = ops.si_frame(x, nrm=nrm)
        lo, hi = x - self.eps, x + self.eps
        inside = (xe >= lo) & (xe <= hi)               # the clamp passes the gradient on where it does not bind
        g = self._wb_grad(torch.min(torch.max(xe, lo), hi), target) * inside
        key, dirs, order, _ = ops.si_rank(g.contiguous(), nrm)
        return nrm, order, dirs, key

    def shape_invariant_query_attack(self, points, target, table=None):
        """Black-box query-based attack on point-cloud sensitivity maps, batched. Returns, as the reference does, the LAST
        CANDIDATE EVALUATED, accepted or not. table: (nrm [B,3,N], order int32 [B,N], dir [B,N,3]) in place of the
        sensitivity map."""
        x, target, logp0, adv_target0 = self._query_prepare(points, target, "ours")
        active = torch.ones_like(target, dtype=torch.bool)      # no early return (:533-534 is commented out)
        with torch.no_grad():
            nrm, order, dirs = table if table is not None else self.query_sensitivity(x, target)[:3]
        eps = torch.tensor(sign_order(self.step_size), dtype=torch.float32)
        return self._query("ours", x, target, logp0, adv_target0, active, order,
                           eps, nrm.float().contiguous(), dirs.float().contiguous())
