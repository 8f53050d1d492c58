"""Point-adding C&W attack (Xiang et al., CVPR'19) — MI355X mirror of attack/Gen3DAdv/IndpAdd_attack.py.

Same constructor / ``attack(data, target)`` signature and return values as the reference (IndpAdd_attack.py:47-49,
84, 289). The victim sees [ori | adv]: the K original points followed by A added points, of which only the A are
optimised; the distance the binary search keeps is the set distance ``dist_func(adv, ori)`` itself (:159-162), and
there is no clip. What changes is where the work happens:

* the victim's input is ONE persistent buffer ``cat_buf [B,3,K+A]`` holding ``ori`` once; the iterate is the view
  ``cat_buf[:, :, K:]`` (no ``torch.cat`` per iteration, every kernel takes strided points);
* with this package's own functors (Chamfer / Hausdorff adv2ori, FarChamfer) an iteration is the victim's fused loss +
  input gradient, the adv -> ori search (pc3d_nn_f32) and ONE update launch (pc3d_add_update_f32: set distance,
  bookkeeping, total gradient, Adam), captured into hipGraphs as the CW mirror's loop; victims without the fused entry
  point go through autograd with the same search + update launch; arbitrary user callables keep the reference's
  protocol (``torch.cat``, ``torch.optim.Adam``);
* no host synchronisation inside a binary step, B > 1 works (the fail counters are sums over the batch).

The binary search, the weight adjustment and the graph capture are the CW mirror's (attack/CW/CW_attack.py), shared by
subclassing.
"""
import numpy as np
import torch
import torch.nn.functional as F
import torch.optim as optim

from ... import graphed as _graphed
from ... import ops
from ..CW.CW_attack import CW as _CW
from ..CW.CW_attack import rand_row  # noqa: F401  (the reference defines the same function, :8-12)
from ..CW.CW_utils import dist_utils as _dist_utils


def critical_scores(model, pc, label):
    """Per-point importance of the reference's selection (:15-39): sum over xyz of the squared gradient of
    F.cross_entropy(model(pc), label) (batch mean) with respect to the input. pc [B,3,K] on the GPU -> [B,K] fp32."""
    x = pc.detach().float().clone().requires_grad_()
    label = label.long().to(pc.device).view(-1)
    with torch.enable_grad():
        loss = F.cross_entropy(_graphed.logits_of(model(x)), label)
        g, = torch.autograd.grad(loss, x)
    return (g ** 2).sum(1)


def get_critical_points(model, pc, label, num):
    """attack/Gen3DAdv/IndpAdd_attack.py:15-39: the `num` points of pc [B,3,K] with the largest critical_scores, in
    descending order of score -> [B,3,num]. Ties (many scores are exactly 0: PointNet's max-pool routes gradient to a few
    hundred points) go to the lower point index; torch.topk leaves their order unspecified (ops.topk_desc, DESIGN A-15)."""
    if not pc.is_cuda:
        pc = pc.cuda()
    model.eval()
    score = critical_scores(model, pc, label)
    idx = ops.topk_desc(score.float().contiguous(), int(num)).long()
    return torch.gather(pc.detach().float(), 2, idx[:, None, :].expand(-1, 3, -1)).clone()


class CWAdd(_CW):
    """Class for CW attack."""
    ragged = False      # the added points' loop knows no per-cloud lengths: attack(..., lengths) raises ValueError

    def __init__(self, model, trans_model, adv_func, dist_func, attack_lr=1e-2, init_weight=5e3, max_weight=4e4,
                 binary_step=10, num_iter=500, num_add=512, attack_method='untarget', device=None, verbose=False,
                 fused=True, graph=True, sample_seeds=None, global_batch=None, deterministic=None):
        """Arguments as attack/Gen3DAdv/IndpAdd_attack.py:47-49; the extra keywords are the CW mirror's (device, verbose,
        fused, graph, sample_seeds, global_batch, deterministic). `init_points` (attribute, default None): a [B,3,A]
        start cloud used instead of the critical-point selection — the tests start from a stored selection with it."""
        super().__init__(model, trans_model, adv_func, None, dist_func, attack_lr=attack_lr, init_weight=init_weight,
                         max_weight=max_weight, binary_step=binary_step, num_iter=num_iter, attack_method=attack_method,
                         device=device, verbose=verbose, fused=fused, graph=graph, sample_seeds=sample_seeds,
                         global_batch=global_batch, deterministic=deterministic)
        self.num_add = num_add
        self.init_points = None

    # -- start points --------------------------------------------------------------------------------------------
    def _initial_points(self, ori, label):
        """[B,3,A] fp32 on the device: the critical points of the clean cloud (:107-108)."""
        return get_critical_points(self.model, ori, label, self.num_add)

    # -- which iteration runs --------------------------------------------------------------------------------------
    def _add_kind(self, A):
        """(kind, cd_w, P) of pc3d_add_update_f32 when the distance functor is one of this package's own set distances
        adv -> ori, else None (generic path)."""
        df = self.dist_func
        if type(df) is _dist_utils.ChamferDist and df.method == 'adv2ori':
            return "chamfer", 1.0, 0
        if type(df) is _dist_utils.HausdorffDist and df.method == 'adv2ori':
            return "hausdorff", 1.0, 0
        if (type(df) is _dist_utils.FarChamferDist and type(df.chamfer_dist) is _dist_utils.ChamferDist
                and df.chamfer_dist.method == 'adv2ori' and df.num_add > 0 and A % df.num_add == 0
                and A // df.num_add <= ops.ADD_UPDATE_MAX_CLUSTER):
            return "far_chamfer", float(df.cd_w), A // df.num_add
        return None

    def _path(self, A):
        """'fast' (fused victim + search + update launch), 'direct' (autograd victim + search + update launch) or
        'generic' (the reference's protocol with torch.optim.Adam)."""
        if (not self.fused or self.device.type != "cuda" or A > ops.ADD_UPDATE_MAX_POINTS or self._add_kind(A) is None
                or self._own_adv_kind() is None):
            return "generic"
        return "fast" if hasattr(self.model, "fused_attack_grad") else "direct"

    def _capturable(self):
        return self.graph and getattr(self, "_cur_path", None) == "fast"

    # -- the state machine (CW mirror's hooks) ------------------------------------------------------------------------
    def _begin(self, data, target):
        dev, B = self.device, data.shape[0]
        # the start points first, then the clean prediction (CW._begin): the reference's order (:104-109), so a victim that
        # draws from torch's global generator on every forward (PointNet++) consumes the same draws for the same forwards
        if self.init_points is not None:
            init = torch.as_tensor(self.init_points).float().to(dev).reshape(B, 3, -1).contiguous()
        else:
            ori = data.float().to(dev).detach().transpose(1, 2).contiguous()
            init = self._initial_points(ori, target.long().to(dev).view(-1)).float().contiguous()
        st = super()._begin(data, target)
        K = st["K"]
        A = init.shape[2]
        st["A"], st["init"] = A, init
        st["path"] = self._cur_path = self._path(A)
        st["kind"] = self._add_kind(A) if st["path"] != "generic" else None
        cat = torch.empty((B, 3, K + A), dtype=torch.float32, device=dev)
        cat[:, :, :K].copy_(st["ori"])
        cat[:, :, K:].copy_(init)
        st["cat"] = cat
        st["o_bestattack"] = torch.zeros((B, 3, A), dtype=torch.float32, device=dev)
        st["input_val"] = init.clone()
        return st

    def _begin_binary_step(self, st):
        """Fresh start point (critical points + 1e-7 noise from torch's CPU generator, :134-135), Adam state and
        per-step bests."""
        dev, B, A, K = self.device, st["B"], st["A"], st["K"]
        if st["gens"] is None:
            noise = torch.randn((B, 3, A))
        else:
            noise = torch.stack([torch.randn((3, A), generator=g) for g in st["gens"]])
        start = st["init"] + noise.to(dev) * 1e-7
        weights = torch.from_numpy(st["current_weight"] * st["ratio"]).float()
        if "bestdist" not in st:
            st["bestdist"] = torch.full((B,), 1e10, dtype=torch.float32, device=dev)
            st["bestscore"] = torch.full((B,), -1, dtype=torch.long, device=dev)
            st["weights"] = weights.to(dev)
            # d loss / d (distance of sample b) for `dist_func(adv, ori, weights).mean()`: weights[b] / B
            st["gdist"] = st["weights"] * float(np.float32(1.0) / np.float32(B))
            if st["path"] != "generic":
                st["adv"] = st["cat"][:, :, K:]
                st["exp_avg"] = torch.zeros((B, 3, A), dtype=torch.float32, device=dev)
                st["exp_avg_sq"] = torch.zeros((B, 3, A), dtype=torch.float32, device=dev)
        with torch.no_grad():
            st["bestdist"].fill_(1e10)
            st["bestscore"].fill_(-1)
            st["weights"].copy_(weights)
            torch.mul(st["weights"], float(np.float32(1.0) / np.float32(B)), out=st["gdist"])
            if st["path"] != "generic":
                st["adv"].copy_(start)
                st["exp_avg"].zero_()
                st["exp_avg_sq"].zero_()
        st["step"].zero_()
        if st["path"] == "generic":
            st["adv"] = start.detach().requires_grad_()
            st["opt"] = optim.Adam([st["adv"]], lr=self.attack_lr, weight_decay=0.)

    def _update(self, st, gx):
        """The search + the update launch on the current iterate st["adv"] (a view of st["cat"])."""
        kind, cd_w, P = st["kind"]
        nn_d, nn_idx = ops.nn_raw(st["adv"], st["ori"], True, True)
        ops.add_update(st["adv"], st["ori"], nn_d, nn_idx, st["pred"], st["label"], self.attack_method == 'untarget',
                       st["bestdist"], st["bestscore"], st["o_bestdist"], st["o_bestscore"], st["o_bestattack"],
                       gx[:, :, st["K"]:], st["exp_avg"], st["exp_avg_sq"], st["step"], self.attack_lr, kind, st["gdist"],
                       input_val=st["input_val"], dist_val=st["dist_val"], cd_w=cd_w, P=P)

    def _iterate(self, st, iteration=None, last=False):
        """One pass of the hot-loop body (reference :138-187)."""
        ori, B = st["ori"], st["B"]
        scale = float(np.float32(st["ratio"]) / np.float32(B))
        if st["path"] == "fast":
            # the classifier tail writes pred and advances the step word; then search + update
            with torch.no_grad():
                _, _, gx = self.model.fused_attack_grad(st["cat"], st["target"], *self._own_adv_kind(),
                                                        pred_out=st["pred"], step=st["step"], scale=st["ratio"] / B)
                self._update(st, gx)
            return
        if st["path"] == "direct":
            # a victim without the fused entry point: its input gradient from autograd, the loss kernel in raw mode (+4:
            # the functor's value on the logits as given) writes the prediction and d loss / d logits
            alias = st["cat"].detach().requires_grad_()
            lg = _graphed.logits_of(self.model(alias))
            lg = lg if (lg.dtype == torch.float32 and lg.stride(1) == 1) else lg.float().contiguous()
            kind, kappa = self._own_adv_kind()
            _, _, _, g_logits = ops.cls_loss(lg.detach(), st["target"], ops.LOSS_KINDS[kind] + 4, kappa, scale,
                                             pred_out=st["pred"])
            gx, = torch.autograd.grad([lg], [alias], [g_logits])
            with torch.no_grad():
                ops.i32_add(st["step"], 1)
                self._update(st, gx)
            return
        # generic: arbitrary callables, the reference's protocol (cat, dist_func on [B,A,3] / [B,K,3], Adam)
        adv = st["adv"]
        cat = torch.cat([ori, adv], dim=-1)
        logits = _graphed.logits_of(self.model(cat))
        pred = torch.argmax(logits, dim=-1)
        ori_t = ori.transpose(1, 2).contiguous()
        with torch.no_grad():
            cur = adv.detach()
            dist_val = self.dist_func(cur.transpose(1, 2).contiguous(), ori_t, batch_avg=False).detach().float().view(-1)
            self._bookkeep_torch(st, cur, pred, dist_val)
            st["dist_val"].copy_(dist_val)
        adv_loss = self.adv_func(logits, st["target"]).mean()
        if st["ratio"] != 1.0:
            adv_loss = adv_loss * st["ratio"]
        # the reference hands its weights over as a CPU float64 tensor (:181); the functors move them
        weights = torch.from_numpy(st["current_weight"] * st["ratio"])
        dist_loss = self.dist_func(adv.transpose(1, 2).contiguous(), ori_t, weights=weights).mean()
        loss = adv_loss + dist_loss
        opt = st["opt"]
        opt.zero_grad()
        loss.backward()
        opt.step()

    # -- after the search -----------------------------------------------------------------------------------------
    def _finish(self, st):
        """(o_bestdist [B] float64, o_bestattack [B,3,A] fp32 device, success_num): samples that never succeeded take
        the last iterate (:230-234); success_num counts the samples with a nonzero lower bound (:237)."""
        fail_idx = torch.from_numpy(st["lower_bound"] == 0.).to(self.device)
        o_bestattack = torch.where(fail_idx[:, None, None], st["input_val"], st["o_bestattack"])
        return st["o_bestdist"].double().cpu().numpy(), o_bestattack, (st["lower_bound"] > 0.).sum()

    def _result(self, st, o_bestattack):
        """concat(ori, best) as [B, K+A, 3] float64 (:286-289)."""
        out = torch.cat([st["ori"].double(), o_bestattack.double()], dim=-1)
        return out.transpose(1, 2).cpu().numpy()

    def _attack(self, data, target):
        """Attack on given data to target.
        Args:
            data (torch.FloatTensor): victim data, [B, num_points, 3]
            target (torch.LongTensor): target output, [B]
        Returns (o_bestdist [B] float64, concat(ori, added) [B,K+A,3] float64, success_num) like the reference (:289).
        """
        st = self._begin(data, target)
        target = st["target"]
        self._search(st)
        o_bestdist, o_bestattack, success_num = self._finish(st)
        if self.verbose:
            print('Successfully attack {}/{}'.format(success_num, st["B"]))
        # The checks run the victim, the shuffled cloud and the transfer model on the ADDED POINTS ALONE
        # ([B,3,A], :239-282), not on the concatenation the attack returns — the reference's behaviour, kept.
        with torch.no_grad():
            attack_pred = torch.argmax(_graphed.logits_of(self.model(o_bestattack)), dim=1)
            self.attack_fail += int((~self._success(attack_pred, target)).sum().item())
            best_np = o_bestattack.double().cpu().numpy()
            shuffled = rand_row(best_np.transpose((0, 2, 1)))       # numpy's global RNG, as the reference
            shuffled = torch.from_numpy(shuffled.transpose((0, 2, 1)).copy()).float().to(self.device)
            shuffle_pred = torch.argmax(_graphed.logits_of(self.model(shuffled)), dim=1)
            self.shuffle_fail += int((~self._success(shuffle_pred, target)).sum().item())
            trans_pred = torch.argmax(_graphed.logits_of(self.trans_model(o_bestattack)), dim=1)
            self.trans_fail += int((~self._success(trans_pred, target)).sum().item())
        if self.verbose:
            print('attack result: ', attack_pred.tolist(), 'shuffle result: ', shuffle_pred.tolist(),
                  'transfer result: ', trans_pred.tolist())
        return o_bestdist, self._result(st, o_bestattack), success_num
