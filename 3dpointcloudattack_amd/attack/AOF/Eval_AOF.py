"""Untargeted AOF (attack on frequency) — MI355X mirror of attack/AOF/Eval_AOF.py.

``attack()`` is the reference's module-level function over the module globals ``args, model, trans_model, test_loader,
clip_func, adv_func`` (:118-259); here it also RETURNS ``(all_adv_pc, all_real_lbl, at_num, trans_num, total_num)``, which
the reference leaves as locals. The work on one batch is the class ``AOF``:

``AOF(model, trans_model, adv_func, clip_func, lr=1e-2, low_pass=100, step=2, epochs=200, batch_size=1).attack(data [B,K,3],
label [B]) -> (o_bestdist [B], best_pc [B,K,3], success_num)``; ``trans_num``, ``preds``, ``trans_preds``, ``shuffle_preds``,
``shuffle_trans_preds`` and ``o_bestscore`` are attributes after each call.

As written in the reference, and kept:
  * every binary step REBINDS the cloud to ori + 1e-7 * randn (torch's CPU generator): the distances of that step and the
    final clip refer to the noisy cloud of the LAST step (:142-143,:172,:206);
  * an iteration records FIRST, on the iterate it has just evaluated (:168-185), then optimises; the distance is the
    largest coordinate deviation of the whole cloud (amax |adv - data|), the comparison a strict <, and success needs the
    low-frequency cloud misclassified as well;
  * the loss is 0.5 adv_func(model(lfc + hfc)) + 0.5 adv_func(model(lfc)), Adam on lfc only (:187-190);
  * a cloud that never succeeded is the ZERO cloud clipped towards the data (:205-206; no last-iterate fallback as in
    TAOF) — it can still be misclassified, and then counts as a success;
  * ``total_num += args.batch_size``, the argument, whatever the batch holds (:227).

On MI355X. The bookkeeping is one launch (pc3d_aof_record_f32) and never leaves the device (the reference copies the
cloud to the host in every iteration). With a PointNet victim (plain or feature transform), one of this package's
adversarial functors and this package's ClipPointsLinf the iteration is, from replayed hipGraphs and as one chain:
ONE victim pass over the stacked [2B,3,N] buffer (rows [:B] = lfc + hfc, rows [B:] = lfc; 0.5 mean_B(a) + 0.5 mean_B(b) =
mean_2B(cat), so scale = 0.5 / B gives the reference's gradient), the record launch (it uses the predictions of the forward
the loss needs anyway), pc3d_aof_update_f32 (gradient sum + Adam + lfc + hfc + clip) and pc3d_spectral_reproject_sum_f32
(which writes lfc, hfc and the next iterate lfc + hfc straight into the stacked buffer); the buffers and the captured graphs
stay on the ``AOF`` object, so the batches of a loader share one capture. Anything else runs the same loop through autograd
on this package's ops.

``basis="lowband"`` (default ``"full"``) computes the [B,N,low_pass] basis of the Laplacian's low band on this package's own
kernels instead of the dense decomposition and re-projects on it (see TAOF_attack.py), in both loops.
"""
import time

import numpy as np
import torch
import torch.optim as optim

from ... import graphed as _graphed
from ... import ops
from ..CW.CW_utils import adv_utils as _adv_utils
from ..CW.CW_utils import clip_utils as _clip_utils
from .TAOF_attack import check_basis, get_Laplace_from_pc, get_lowband_from_pc, knn     # noqa: F401  (:46-62, :72-93)

try:
    from tqdm import tqdm
except ImportError:          # the progress bar is all the reference uses it for
    def tqdm(it, *a, **k):
        return it

GRAPH_BLOCK = 8     # iterations per replayed graph; the remainder of `epochs` replays the one-iteration graph


def rand_row(array):
    """:65-69 — one np.random.shuffle of the row order of a [B,K,C] array / tensor (the global numpy generator)."""
    row_total = array.shape[1]
    row_sequence = np.arange(row_total)
    np.random.shuffle(row_sequence)
    if torch.is_tensor(array):
        return array[:, torch.from_numpy(row_sequence).to(array.device), :]
    return array[:, row_sequence, :]


def normalize_points(points):
    """:96-103 — points [K,3]: centred, scaled by the largest norm (which the reference prints)."""
    points = points - torch.mean(points, 0, keepdim=True)
    dist = torch.max(torch.sqrt(torch.sum(points ** 2, dim=1)))
    print(dist)
    return points / dist


def need_clip(pc, ori_pc, budget=0.1):
    """:106-115 — [B] float mask: 1 where any point of the cloud moved by more than the budget."""
    with torch.no_grad():
        diff = pc - ori_pc
        norm = torch.sum(diff ** 2, dim=1) ** 0.5
        bt = torch.sum(budget / (norm + 1e-9) < 1.0, dim=-1)
        return (bt > 0).to(torch.float)


class AOF:
    """The untargeted AOF attack on one batch (Eval_AOF.py:126-238); the defaults are the reference's argparse defaults."""

    def __init__(self, model, trans_model, adv_func, clip_func, lr=1e-2, low_pass=100, step=2, epochs=200, batch_size=1,
                 device=None, verbose=False, fused=True, graph=True, deterministic=None, basis="full"):
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.deterministic = deterministic     # None: ops.DETERMINISTIC; True / False: that mode during attack()
        self.basis = check_basis(basis)     # "full": dense Laplacian + eigh, V and V^T; "lowband": ops.lowband_basis, U
        self.model = model.to(self.device)
        self.model.eval()
        self.trans_model = trans_model.to(self.device)
        self.trans_model.eval()
        self.adv_func = adv_func
        self.clip_func = clip_func
        self.lr = lr
        self.low_pass = low_pass
        self.step = step
        self.epochs = epochs
        self.batch_size = batch_size     # what the module-level attack() adds to total_num per batch (:227)
        self.verbose = verbose
        self.fused = fused
        self.graph = graph
        self._fused_cache = _graphed.LoopCache(1)     # the fused loop (static buffers and graphs, see _fused_loop)
        self.trans_num = 0
        self.preds = self.trans_preds = self.shuffle_preds = self.shuffle_trans_preds = self.o_bestscore = None

    def _fused_kind(self):
        if not self.fused or not hasattr(self.model, "fused_loss_and_grad") or type(self.clip_func) is not _clip_utils.ClipPointsLinf:
            return None
        return _adv_utils.own_adv_kind(self.adv_func)

    def attack(self, data, label):
        if self.deterministic is None:
            return self._attack(data, label)
        with ops.deterministic(self.deterministic):
            return self._attack(data, label)

    def _attack(self, data, label):
        dev = self.device
        B, K = data.shape[:2]
        ori_data = data.float().to(dev).detach().transpose(1, 2).contiguous()
        label = label.long().to(dev).detach().view(-1)
        for net in (self.model, self.trans_model):
            for param in net.parameters():
                param.requires_grad = False
        fk = self._fused_kind()
        data_last, st = (self._attack_generic if fk is None else self._attack_fused)(ori_data, label, fk)

        with torch.no_grad():
            adv_pc = st["o_bestattack"]          # never found: zeros (:137), clipped towards the data like the others
            if self.clip_func is not None:
                adv_pc = self.clip_func(adv_pc, data_last)
            adv_pc = adv_pc.contiguous()
            preds = torch.argmax(_graphed.logits_of(self.model(adv_pc)), dim=-1)
            trans_preds = torch.argmax(_graphed.logits_of(self.trans_model(adv_pc)), dim=-1)
            shuffle_pc = rand_row(adv_pc.transpose(2, 1).float()).transpose(2, 1).contiguous()
            self.shuffle_preds = torch.argmax(_graphed.logits_of(self.model(shuffle_pc)), dim=-1)
            self.shuffle_trans_preds = torch.argmax(_graphed.logits_of(self.trans_model(shuffle_pc)), dim=-1)
        self.preds, self.trans_preds, self.o_bestscore = preds, trans_preds, st["o_bestscore"].clone()
        success_num = int((preds != label).sum().item())
        self.trans_num = int((trans_preds != label).sum().item())
        if self.verbose:
            print("best linf distance:", st["o_bestdist"].tolist())
        return (st["o_bestdist"].double().cpu().numpy(), adv_pc.transpose(1, 2).contiguous().detach().cpu().numpy(), success_num)

    def _noisy(self, ori_data):
        B, _, K = ori_data.shape
        return ori_data.clone().detach() + torch.randn((B, 3, K)).to(ori_data.device) * 1e-7     # :142-143

    # ---- any victim, any callable functors: the reference's loop through autograd (:141-199) ----------------------------
    @staticmethod
    def _bests(B, K, dev):
        return dict(o_bestdist=torch.full((B,), 1e10, dtype=torch.float32, device=dev),
                    o_bestscore=torch.full((B,), -1, dtype=torch.long, device=dev),
                    o_bestattack=torch.zeros((B, 3, K), dtype=torch.float32, device=dev))

    def _attack_generic(self, ori_data, label, fk):
        model = _graphed.wrap(self.model, enable=self.graph)      # hipGraph replay for deterministic victims
        st = self._bests(ori_data.shape[0], ori_data.shape[2], self.device)
        lp = self.low_pass
        data = ori_data
        for binary_step in range(self.step):
            data = self._noisy(ori_data)
            if self.basis == "lowband":
                U = get_lowband_from_pc(data, lp)      # constant for the whole binary step
                reproject = lambda a: ops.band_reproject(a.contiguous(), U)
            else:
                _, V = get_Laplace_from_pc(data)
                V = V.float().contiguous()
                Vt = V.transpose(2, 1).contiguous()      # constant for the whole binary step
                reproject = lambda a, V=V, Vt=Vt: ops.spectral_reproject(a.contiguous(), V, Vt, lp)
            lfc, hfc = reproject(data)      # :145-147
            lfc.requires_grad_()
            opt = optim.Adam([lfc], lr=self.lr, weight_decay=0)
            for i in range(self.epochs):
                adv_pc = lfc + hfc
                logits = _graphed.logits_of(model(adv_pc))
                lfc_logits = _graphed.logits_of(model(lfc))
                with torch.no_grad():      # record values (:168-185)
                    ops.aof_record(adv_pc.detach(), data, torch.argmax(logits, dim=1), torch.argmax(lfc_logits, dim=1), label,
                                   st["o_bestdist"], st["o_bestscore"], st["o_bestattack"])
                loss = 0.5 * self.adv_func(logits, label).mean() + 0.5 * self.adv_func(lfc_logits, label).mean()
                opt.zero_grad()
                loss.backward()
                opt.step()
                with torch.no_grad():      # clip (:193-199)
                    adv_pc = lfc.detach() + hfc
                    if self.clip_func is not None:
                        adv_pc = self.clip_func(adv_pc, data)
                    lfc.data, hfc = reproject(adv_pc)
        return data, st

    # ---- PointNet victim + this package's functor + ClipPointsLinf: no autograd, every buffer updated IN PLACE, the
    # iteration replayed from hipGraphs ------------------------------------------------------------------------------------
    def _fused_loop(self, B, K, fk):
        """The fused iteration as a DeviceLoop: its state (all static buffers: the graphs point at them) in `bufs`, one
        iteration — 3 launches beside the victim's — as the body. _load takes a batch in and rewinds the bests, _new_step
        draws the step's noisy cloud and its basis, _begin_step alone rewinds to the start of the step.
        The last loop is kept on the instance from one attack() call to the next: a capture (two eager warm-up passes,
        GRAPH_BLOCK + 1 captured iterations, two graph instantiations) costs as much as ~150 replayed iterations, and the
        reference's driver calls the attack once per batch of the loader. It is rebuilt when the shape, the loop's
        constants, the kernel flavour or the victim's weights change (the victim re-folds its weight pack on exactly that
        event: model/pointnet.py keys the folded caches on the same addresses and version counters)."""
        dev, model = self.device, self.model
        lp, budget, lr = self.low_pass, float(self.clip_func.budget), self.lr
        key = _graphed.loop_key(model, dev, B, K, fk, float(lr), int(lp), budget, bool(self.graph), self.basis)
        loop = self._fused_cache.get(key)
        if loop is not None:
            return loop
        f32 = dict(dtype=torch.float32, device=dev)
        buf = torch.empty((2 * B, 3, K), **f32)      # rows [:B] = lfc + hfc, rows [B:] = lfc: the victim's stacked input
        adv, lfc = buf[:B], buf[B:]
        hfc, coeff, clipped, data, ori = (torch.empty((B, 3, K), **f32) for _ in range(5))
        m, v = torch.zeros((B, 3, K), **f32), torch.zeros((B, 3, K), **f32)
        U = V = Vt = None
        if self.basis == "lowband":      # [B,N,lp] instead of V and V^T
            ops.lowband_block(K, lp)      # refuse a low_pass past the block before anything is allocated
            U = torch.empty((B, K, lp), **f32)
        else:
            V, Vt = torch.empty((B, K, K), **f32), torch.empty((B, K, K), **f32)
        step = torch.zeros((1,), dtype=torch.int32, device=dev)
        label2 = torch.zeros((2 * B,), dtype=torch.long, device=dev)
        label = label2[:B]
        c = dict(buf=buf, adv=adv, lfc=lfc, hfc=hfc, coeff=coeff, clipped=clipped, data=data, ori=ori, m=m, v=v, U=U, V=V, Vt=Vt,
                 lp=lp, step=step, label2=label2, **self._bests(B, K, dev))

        def iterate():
            with torch.no_grad():
                _, pred2, _, g = model.fused_loss_and_grad(buf, label2, *fk, scale=0.5 / B)
                ops.aof_record(adv, data, pred2[:B], pred2[B:], label, c["o_bestdist"], c["o_bestscore"], c["o_bestattack"],
                               step=step)      # also advances the Adam step word
                ops.aof_update(lfc, g[:B], g[B:], m, v, hfc, data, step, lr, budget, out=clipped)
                _reproject(c, clipped)

        return self._fused_cache.put(key, _graphed.DeviceLoop(key, dev, owners=(model,), counts=(1, GRAPH_BLOCK), warmup=2,
                                                              body=iterate, bufs=c))

    @staticmethod
    def _load(c, ori_data, lab):
        c["ori"].copy_(ori_data)
        c["label2"].copy_(lab.repeat(2))
        _rewind_bests(c)

    def _new_step(self, c):
        data = c["data"]
        data.copy_(self._noisy(c["ori"]))
        if c["U"] is not None:
            c["U"].copy_(get_lowband_from_pc(data, c["lp"]))      # the low band: once per binary step
        else:
            _, Vn = get_Laplace_from_pc(data)      # the eigen-decomposition: once per binary step
            c["V"].copy_(Vn)
            c["Vt"].copy_(Vn.transpose(2, 1))
        _begin_step(c)

    def _attack_fused(self, ori_data, label, fk):
        B, _, K = ori_data.shape
        loop = self._fused_loop(B, K, fk)
        c = loop.bufs

        def rewind():
            _rewind_bests(c)
            _begin_step(c)

        self._load(c, ori_data, label)
        for binary_step in range(self.step):
            self._new_step(c)
            if self.graph and self.epochs > 0:
                loop.capture(rewind)
            loop.run(self.epochs)
        return (c["data"] if self.step > 0 else ori_data), c


def _rewind_bests(c):
    c["o_bestdist"].fill_(1e10), c["o_bestscore"].fill_(-1), c["o_bestattack"].zero_()


def _reproject(c, src):
    """lfc, hfc and the next iterate lfc + hfc of `src`, straight into the stacked buffer."""
    if c["U"] is not None:
        ops.band_reproject(src, c["U"], c["lfc"], c["hfc"], sum=c["adv"])
    else:
        ops.spectral_reproject(src, c["V"], c["Vt"], c["lp"], c["lfc"], c["hfc"], c["coeff"], sum=c["adv"])


def _begin_step(c):
    _reproject(c, c["data"])      # :145-147
    c["m"].zero_(), c["v"].zero_(), c["step"].zero_()


# ---- the reference's module-level driver (:118-259): the globals its __main__ sets --------------------------------------
args = None
model = None
trans_model = None
test_loader = None
clip_func = None
adv_func = None


def attack(**overrides):
    """Eval_AOF.py:118-259 over this module's globals of the same names (keywords override them for this call; further
    keywords — device, fused, graph, deterministic, verbose — go to ``AOF``). Prints what the reference prints; returns
    (all_adv_pc [num_data,K,3], all_real_lbl [num_data], at_num, trans_num, total_num)."""
    g = dict(args=args, model=model, trans_model=trans_model, test_loader=test_loader, clip_func=clip_func, adv_func=adv_func)
    extra = {k: overrides.pop(k) for k in list(overrides) if k not in g}
    g.update(overrides)
    a = g["args"]
    atk = AOF(g["model"], g["trans_model"], g["adv_func"], g["clip_func"], lr=a.lr, low_pass=a.low_pass, step=a.step,
              epochs=a.epochs, batch_size=a.batch_size, **extra)
    iter_num = 0
    at_num, total_num, trans_num = 0.0, 0.0, 0.0
    all_adv_pc = []
    all_real_lbl = []
    st = time.time()
    for data, label in tqdm(g["test_loader"]):
        iter_num += 1
        _, best_pc, success_num = atk.attack(data, label)
        label = label.long().to(atk.device)
        at_num += success_num
        trans_num += atk.trans_num
        total_num += a.batch_size
        print("\n", atk.preds)
        print(atk.trans_preds)
        print(label)
        if iter_num % 1 == 0:
            print(f"attack success rate:{at_num / total_num}, trans success rate: {trans_num / total_num}")
        all_adv_pc.append(best_pc)
        all_real_lbl.append(label.detach().cpu().numpy())
    et = time.time()
    print(f"attack success rate:{at_num / total_num}, trans success rate: {trans_num / total_num}, consuming time:{et - st} seconds")
    all_adv_pc = np.concatenate(all_adv_pc, axis=0)      # [num_data, K, 3]
    all_real_lbl = np.concatenate(all_real_lbl, axis=0)  # [num_data]
    return all_adv_pc, all_real_lbl, at_num, trans_num, total_num
