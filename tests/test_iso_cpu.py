"""CPU: the isometry attack restated in plain torch against the reference's recorded runs (tests/golden/iso.npz, written by
make_golden_iso.py from the real reference), the numpy mirrors bit for bit, the signatures, the drop-in import paths.

``RestatedISO`` is the algorithm of attack/ISO (TSI + CTRI) as DESIGN.md §8.4 describes it: any device, any dtype,
batched with a done-mask, the same ``tsi_batch`` rule as the product's ISOAttack. The GPU tests use it as the same-device
reference for victims and settings the fixture does not hold."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, ROOT

PKG = "3dpointcloudattack_amd.attack.ISO."
ARGS = ("num_steps", "step_size", "LAMBDA", "target", "kappa", "num_init", "d", "a", "b")


def mirrors():
    return (importlib.import_module(PKG + "iso_attack"), importlib.import_module(PKG + "thompson_sample"),
            importlib.import_module(PKG + "isometry_init"))


def case_args(fx, key):
    a = dict(zip(ARGS, fx[f"{key}_args"].tolist()))
    for k in ("num_steps", "LAMBDA", "target", "kappa", "num_init", "d"):
        a[k] = int(a[k])
    return a


def penalty_of(W, v, iters=30):
    """The reference's fp32 power iteration on W^T W - I from the start vector v (host)."""
    v = F.normalize(v, dim=0, eps=1e-12)
    M = torch.mm(W.t(), W) - torch.eye(3)
    p = torch.zeros(())
    for _ in range(iters):
        v = F.normalize(torch.matmul(M, v), dim=0, eps=1e-12)
        p = torch.dot(v, torch.matmul(M, v))
    return float(p.abs())


def penalty_tols(fx, key):
    """Per cloud, how far the stored penalty may move when W moves inside band_W: the reference's fp32 power iteration,
    from the cloud's own LAST start vector, evaluated at every corner W +- band_W (all 512 sign patterns; the penalty is
    smooth and the box tiny, so its extreme over the box sits at a corner), the largest change against the value at the
    stored W — plus 16 u (u = 2^-24) for fp32: W^T W - I cancels against the identity, so every entry of the iterated
    matrix carries an absolute rounding error of a few u whatever W is, and the Rayleigh quotient adds its own.
    The start vectors are re-drawn from the case's torch seed in the reference's order (steps[b] draws per cloud, the
    last one counts); the caller's generator state is put back."""
    state = torch.get_rng_state()
    try:
        torch.manual_seed(int(fx[f"{key}_seed"]))
        W, steps, band = fx[f"{key}_W"], fx[f"{key}_steps"], float(fx[f"{key}_band_W"])
        signs = torch.tensor([[1.0 if (c >> k) & 1 else -1.0 for k in range(9)] for c in range(512)]).view(512, 3, 3)
        tols = []
        for b in range(W.shape[0]):
            v = None
            for _ in range(int(steps[b])):
                v = torch.empty(3).normal_(0, 1)
            if v is None or fx[f"{key}_correct"][b] == 1:
                tols.append(0.0)                         # no CTRI, or a failed one: the penalty is 0 by definition
                continue
            Wb = torch.from_numpy(W[b]).float()
            Wc = torch.cat([Wb[None], Wb[None] + band * signs])                   # [513,3,3] fp32
            M = torch.bmm(Wc.transpose(1, 2), Wc) - torch.eye(3)
            u = F.normalize(v, dim=0, eps=1e-12).expand(513, 3)
            pen = torch.zeros(513)
            for _ in range(30):
                u = F.normalize(torch.bmm(M, u[:, :, None])[:, :, 0], dim=1, eps=1e-12)
                pen = (u * torch.bmm(M, u[:, :, None])[:, :, 0]).sum(1)
            pen = pen.abs().double()
            tols.append(float((pen[1:] - pen[0]).abs().max()) + 16 * 2.0 ** -24)
        return tols
    finally:
        torch.set_rng_state(state)


class RestatedISO:
    """Plain-torch restatement. model: callable returning a tuple whose first entry is the [B,ncls] output."""

    def __init__(self, model, num_steps=50, step_size=5e-4, LAMBDA=1000, target=1, kappa=0, num_init=50, d=4, a=-np.pi,
                 b=np.pi, attack_type='combine', thompson=None, tsi_batch=1):
        _, ts, _ = mirrors()
        self.model, self.num_steps, self.step_size, self.target, self.kappa = model, num_steps, step_size, target, kappa
        self.num_init, self.attack_type, self.tsi_batch = num_init, attack_type, tsi_batch
        self.thompson = thompson if thompson is not None else ts.BernThompson(ts.environment(d=d, a0=a, b0=b))
        self.drawn = []                       # every float64 matrix TSI drew, in order
        self.gaps = []                        # top-1/top-2 gap of every CTRI evaluation of a running cloud

    def _eval(self, x, W, label):
        out = self.model(torch.matmul(W, x))[0]
        rates, indices = F.softmax(out, dim=1).sort(1, descending=True)
        return out, rates, indices, (rates * (indices == label[:, None])).sum(1)

    def _tsi(self, x, label, clouds):
        _, _, iso_init = mirrors()
        th, env = self.thompson, self.thompson.environment
        res = {}
        for g0 in range(0, len(clouds), self.tsi_batch):
            group = clouds[g0:g0 + self.tsi_batch]
            mats, probs, active = {b: [] for b in group}, {b: [] for b in group}, list(group)
            for _ in range(self.num_init):
                if not active:
                    break
                arms = []
                for b in active:
                    arms.append(th.get_action())
                    mats[b].append(iso_init.rotation_xyz(*env.arm_to_interval(arms[-1])))
                    self.drawn.append(mats[b][-1])
                W = torch.as_tensor(np.stack([mats[b][-1] for b in active]), dtype=torch.float32).to(x.device, x.dtype)
                with torch.no_grad():
                    _, _, indices, tp = self._eval(x[active], W, label[active])
                wrong = (indices[:, 0] != label[active]).cpu().tolist()
                for j, b in enumerate(list(active)):
                    reward = int(wrong[j])
                    th._update_params(arms[j], reward)
                    probs[b].append(float(tp[j]))
                    if reward == 1:
                        active.remove(b)
            for b in group:
                res[b] = (mats[b][int(np.argmin(probs[b]))], len(probs[b]))
        return res

    def _ctri(self, x, label, W):
        S = x.shape[0]
        W = W.clone()
        m, v = torch.zeros_like(W), torch.zeros_like(W)
        done = torch.zeros(S, dtype=torch.bool, device=x.device)
        steps = torch.zeros(S, dtype=torch.int64, device=x.device)
        kept_out, kept_pred = None, torch.zeros(S, dtype=torch.int64, device=x.device)
        b1, b2, eps = 0.9, 0.999, 1e-8
        for t in range(1, self.num_steps + 1):
            Wp = W.detach().requires_grad_()
            out = self.model(torch.matmul(Wp, x))[0]
            srt = out.detach().sort(1, descending=True)
            pred = srt[1][:, 0]
            kept_out = out.detach().clone() if kept_out is None else torch.where(done[:, None], kept_out, out.detach())
            kept_pred = torch.where(done, kept_pred, pred)
            steps = torch.where(done, steps, torch.full_like(steps, t))
            self.gaps += (srt[0][:, 0] - srt[0][:, 1])[~done].tolist()
            done = done | (pred != label)
            if self.target != 0:
                loss = torch.clamp(out.gather(1, srt[1][:, :1]) - out.gather(1, srt[1][:, 1:2]), min=-self.kappa).sum()
            else:
                loss = -F.cross_entropy(out, label, reduction='sum')
            (g,) = torch.autograd.grad(loss, Wp)
            m2 = m + (g - m) * (1 - b1)
            v2 = v * b2 + (1 - b2) * g * g
            denom = v2.sqrt() / ((1 - b2 ** t) ** 0.5) + eps
            W2 = torch.addcdiv(W, m2, denom, value=-(self.step_size / (1 - b1 ** t)))
            keep = done[:, None, None]
            W, m, v = torch.where(keep, W, W2), torch.where(keep, m, m2), torch.where(keep, v, v2)
        return W, steps, kept_out, kept_pred

    def attack(self, pc, label):
        x, label = pc.detach(), label.reshape(-1).long()
        B, dev = x.shape[0], x.device
        with torch.no_grad():
            _, rates, indices, true_before = self._eval(x, torch.eye(3, dtype=x.dtype, device=dev).expand(B, 3, 3), label)
        attacked = (indices[:, 0] == label).cpu().numpy()
        clouds = [int(b) for b in np.nonzero(attacked)[0]]
        W64, draws = np.tile(np.eye(3), (B, 1, 1)), np.zeros(B, dtype=np.int64)
        for b, (mat, n) in self._tsi(x, label, clouds).items():
            W64[b], draws[b] = mat, n
        W = torch.as_tensor(W64, dtype=torch.float32).to(dev, x.dtype)
        tsi_W = W.clone()
        with torch.no_grad():
            _, rates, indices, true_after = self._eval(x, W, label)
        pred_after, pred_prob = indices[:, 0].clone(), rates[:, 0].clone()
        correct = (pred_after == label).cpu().numpy() & attacked
        init_success = attacked & ~correct
        steps, penalty = np.zeros(B, dtype=np.int64), np.zeros(B)
        todo = [b for b in clouds if not init_success[b]]
        if todo and self.attack_type == 'combine':
            Wc, st, kept_out, kept_pred = self._ctri(x[todo], label[todo], W[todo])
            r, i = F.softmax(kept_out, dim=1).sort(1, descending=True)
            W[todo] = Wc
            pred_after[todo], pred_prob[todo] = kept_pred, r[:, 0]
            true_after[todo] = (r * (i == label[todo][:, None])).sum(1)
            still = (kept_pred == label[todo]).cpu().numpy()
            correct[todo] = still
            steps[todo] = st.cpu().numpy()
            for j, b in enumerate(todo):                      # host, cloud order: steps[b] draws, the last one counts
                vec = None
                for _ in range(int(steps[b])):
                    vec = torch.empty(3).normal_(0, 1)
                penalty[b] = 0.0 if still[j] else penalty_of(Wc[j].detach().float().cpu(), vec)
        info = dict(attacked=attacked, init_success=init_success, correct=correct.astype(np.int64),
                    true_prob_before=true_before.cpu().numpy(), true_prob_after=true_after.detach().cpu().numpy(),
                    pred_after=pred_after.cpu().numpy(), pred_prob_after=pred_prob.detach().cpu().numpy(), penalty=penalty,
                    steps=steps, tsi_draws=draws, tsi_W=tsi_W.cpu().numpy())
        return torch.matmul(W, x), W, info


def seeded_attack(cls, model, fx, key, **kw):
    """Seed both generators as the fixture's generator did, build the posterior, run `cls` on the case's clouds."""
    _, ts, _ = mirrors()
    a = case_args(fx, key)
    seed = int(fx[f"{key}_seed"])
    np.random.seed(seed)
    torch.manual_seed(seed)
    th = ts.BernThompson(ts.environment(d=a["d"], a0=a["a"], b0=a["b"]))
    atk = cls(model, num_steps=a["num_steps"], step_size=a["step_size"], LAMBDA=a["LAMBDA"], target=a["target"],
              kappa=a["kappa"], num_init=a["num_init"], thompson=th, **kw)
    return atk, a


def check_against_reference(fx, key, W, info, thompson):
    """The comparison both the restatement (CPU) and the product (GPU) must pass; consumes one draw of each generator."""
    g = lambda n: fx[f"{key}_{n}"]          # noqa: E731
    as_np = lambda t: t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)      # noqa: E731
    for n in ("attacked", "init_success", "tsi_draws", "steps", "correct"):
        assert np.array_equal(as_np(info[n]).astype(np.int64), g(n).astype(np.int64)), (key, n, as_np(info[n]), g(n))
    assert np.array_equal(as_np(info["pred_after"]), g("indices2")[:, 0]), key
    assert np.array_equal(thompson.alpha, g("alpha")) and np.array_equal(thompson.beta, g("beta")), key
    band_W, band_gap = float(g("band_W")), float(g("band_gap"))
    W = as_np(W).astype(np.float64)
    dW = np.abs(W - g("W")).max()
    dp = max(np.abs(as_np(info["true_prob_after"]) - g("true_prob_after")).max(),
             np.abs(as_np(info["pred_prob_after"]) - g("rates2")[:, 0]).max(),
             np.abs(as_np(info["true_prob_before"]) - g("true_prob_before")).max())
    print(f"{key}: |dW| {dW:.3e} (band {band_W:.3e})  |dprob| {dp:.3e} (band {band_gap:.3e})")
    assert dW <= band_W, (key, dW, band_W)
    assert dp <= band_gap, (key, dp, band_gap)
    pen = as_np(info["penalty"])
    tols = penalty_tols(fx, key)
    for b in range(len(pen)):
        tol = tols[b]
        print(f"{key}[{b}]: penalty {pen[b]:.6e} ref {g('penalty')[b]:.6e} tol {tol:.2e}")
        assert abs(pen[b] - g("penalty")[b]) <= tol, (key, b, pen[b], g("penalty")[b], tol)
    assert np.random.uniform() == float(g("next_np")), f"{key}: numpy's generator is not where the reference leaves it"
    assert float(torch.rand(1).double()[0]) == float(g("next_torch")), f"{key}: torch's generator is not where the reference leaves it"


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "iso.npz"))


@pytest.fixture(scope="module")
def oracle():
    from helpers import oracle_pointnet
    return oracle_pointnet


def cases(fx=None):
    return [f"{c}_n{N}" for N in (64, 256) for c in "abcde"]


@pytest.mark.parametrize("key", cases())
def test_restated_reproduces_reference(fx, oracle, key):
    model, sha = oracle(int(fx["weights_seed"]))
    assert sha == str(fx["sha256"])
    for p in model.parameters():
        p.requires_grad_(False)
    atk, _ = seeded_attack(RestatedISO, model, fx, key, tsi_batch=1)
    _, W, info = atk.attack(torch.from_numpy(fx[f"{key}_x"]), torch.from_numpy(fx[f"{key}_label"]))
    # the numpy mirrors (isometry_init, thompson_sample) bit for bit: every drawn float64 matrix, the chosen ones as the
    # float32 values the reference hands on, the posterior (in check_against_reference)
    drawn = np.stack(atk.drawn) if atk.drawn else np.zeros((0, 3, 3))
    assert drawn.shape == fx[f"{key}_tsi_all"].shape and np.array_equal(drawn, fx[f"{key}_tsi_all"])
    assert np.array_equal(info["tsi_W"].astype(np.float64), fx[f"{key}_tsi_W"])
    check_against_reference(fx, key, W, info, atk.thompson)
    assert min(atk.gaps, default=1.0) > float(fx[f"{key}_band_gap"])


def test_fixture_lists_every_case(fx):
    assert list(fx["cases"]) == cases()


def test_mirror_draws_from_numpy_seed(fx):
    """isometry_init / thompson_sample alone: the first posterior draw and rotation of a case from its seed."""
    _, ts, iso_init = mirrors()
    key = "c_n64"
    a = case_args(fx, key)
    np.random.seed(int(fx[f"{key}_seed"]))
    th = ts.BernThompson(ts.environment(d=a["d"], a0=a["a"], b0=a["b"]))
    arm = th.get_action()
    lo, hi = th.environment.arm_to_interval(arm)
    assert np.array_equal(iso_init.rotation_xyz(lo, hi), fx[f"{key}_tsi_all"][0])
    for f in (iso_init.rotation_axis_angle, iso_init.rotation, iso_init.reflection, iso_init.ref_rot):
        M = f()
        assert M.shape == (3, 3) and np.allclose(M @ M.T, np.eye(3), atol=1e-12)


def sig_string(f):
    """'(name, name=default, ...)' with array defaults written as lists (numpy's print options must not matter)."""
    import inspect
    out = []
    for p in inspect.signature(f).parameters.values():
        d = p.default
        out.append(p.name if d is inspect.Parameter.empty else f"{p.name}={np.asarray(d).tolist()!r}" if isinstance(d, np.ndarray)
                   else f"{p.name}={d!r}")
    return "(" + ", ".join(out) + ")"


def test_signatures_equal_reference(fx):
    mods = dict(zip(("iso_attack", "thompson_sample", "isometry_init"), mirrors()))
    assert len(fx["signatures"]) >= 22
    for rec in fx["signatures"]:
        m, q, sig = str(rec).split(":", 2)
        f = mods[m]
        for part in q.split("."):
            f = getattr(f, part)
        assert sig_string(f) == sig, (m, q, sig_string(f), sig)


def test_import_has_no_side_effects_and_dropin_resolves():
    code = r'''
import importlib, sys
sys.path.insert(0, %r)
pc3d = importlib.import_module("3dpointcloudattack_amd")
pc3d.install_dropin()
import numpy as np, torch
s_np, s_t = np.random.get_state()[1].copy(), torch.get_rng_state().clone()
from attack.ISO.iso_attack import (ISOnet, ISOAttack, logits_info, spectral_penalty, iso_penalty, thompson_sample_attack,
                                   gradient_attack)
from attack.ISO.thompson_sample import environment, BetaAlgo, BernThompson
from attack.ISO.isometry_init import rotation_xyz, rotation_axis_angle, rotation, reflection, ref_rot
import attack.ISO.iso_attack as m
assert m is importlib.import_module("3dpointcloudattack_amd.attack.ISO.iso_attack")
assert "open3d" not in sys.modules and not hasattr(m, "device")
assert np.array_equal(s_np, np.random.get_state()[1]) and torch.equal(s_t, torch.get_rng_state())
W = torch.tensor([[1., .1, 0.], [0., 1., 0.], [0., 0., 1.1]])
assert float(iso_penalty(W)) > 0 and float(spectral_penalty(W)) > 0
print("iso dropin ok")
'''
    out = subprocess.run([sys.executable, "-c", code % ROOT], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "iso dropin ok" in out.stdout
