"""CPU: the host side of the ragged additional-experiments CW loop — the ragged restatement with full
lengths is the dense restatement; the three new entries in the library, the header and the signature table; every gate of
CW.attack(lengths=...), which fires before any launch; the lengths check; the loop key; and what `lengths=None` leaves
as it was."""
import importlib
import inspect
import os
import re

import numpy as np
import pytest
import torch

import eot_draw_restatement as dr
import eot_ragged_restatement as rr
import eot_restatement as rs

M = importlib.import_module
ops = M("3dpointcloudattack_amd.ops")
_lib = M("3dpointcloudattack_amd._lib")
cwm = M("3dpointcloudattack_amd.attack.additional_exp.CW_attack")
graphed = M("3dpointcloudattack_amd.graphed")
pointnet = M("3dpointcloudattack_amd.model.pointnet")
defense = M("3dpointcloudattack_amd.defense")
adv_u = M("3dpointcloudattack_amd.attack.CW.CW_utils.adv_utils")
dist_u = M("3dpointcloudattack_amd.attack.CW.CW_utils.dist_utils")

ENTRIES = ("pc3d_eot_prepare_ragged_f32", "pc3d_eot_update_ragged_f32", "pc3d_eot_draw_ragged_f32")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, KMAX = 3, 40
LENGTHS = [40, 33, 2]
WHO = r"CW\.attack\(lengths=\.\.\.\)"


# ----------------------------------------------------------------------------------------------------------------------
# the restatement
# ----------------------------------------------------------------------------------------------------------------------
def _case(E, K=KMAX, Bn=B, seed=3):
    g = torch.Generator().manual_seed(seed)
    ori = torch.randn((Bn, 3, K), generator=g, dtype=torch.float64) * 0.4
    adv = ori + torch.randn((Bn, 3, K), generator=g, dtype=torch.float64) * 0.02
    th = torch.randn(E, generator=g, dtype=torch.float64) * 1e-2
    rot = torch.stack([torch.tensor([[np.cos(t), np.sin(t), 0], [-np.sin(t), np.cos(t), 0], [0, 0, 1]]) for t in th.tolist()])
    idx = torch.stack([torch.randperm(2 * K - 1, generator=g)[:K] + 1 for _ in range(E)])
    S = 1 + E
    return dict(adv=adv, ori=ori, rot=rot, idx=idx, inv=rs.inverse_table(idx, K),
                gx=torch.randn((S * Bn, 3, K), generator=g, dtype=torch.float64) * 0.1,
                m=torch.randn((Bn, 3, K), generator=g, dtype=torch.float64) * 0.05,
                v=torch.rand((Bn, 3, K), generator=g, dtype=torch.float64) * 0.01 + 1e-4,
                w=torch.rand((Bn,), generator=g, dtype=torch.float64) * 20 + 5,
                nn_idx=torch.randint(0, K, (Bn, K), generator=g))


@pytest.mark.parametrize("renorm,resample", [(False, False), (True, False), (False, True), (True, True)])
def test_full_lengths_restate_the_dense_formulas(renorm, resample):
    E = 3
    c = _case(E)
    full = [KMAX] * B
    idx = c["idx"] if resample else None
    inv = c["inv"] if resample else None
    # the per-cloud tables of a batch whose clouds share one table
    idx_b = None if idx is None else idx[:, None].expand(E, B, KMAX)
    inv_b = None if inv is None else inv[:, None].expand(E, B, KMAX, 2)
    dense, ragged = rs.prepare(c["adv"], c["ori"], c["rot"], idx, renorm), rr.prepare(c["adv"], c["ori"], full, c["rot"], idx_b, renorm)
    for d, r in zip(dense, ragged):
        assert torch.equal(d, r)
    pred, goal = torch.tensor([1, 2, 3] * (1 + E)), torch.tensor([1, 0, 3])
    st = (torch.full((B,), 1e10, dtype=torch.float64), torch.full((B,), -1), torch.full((B,), 1e10, dtype=torch.float64),
          torch.full((B,), -1), torch.full((B, 3, KMAX), 7.0, dtype=torch.float64))
    for dist_kind in ("chamfer", "l2"):
        args = (c["gx"], c["m"], c["v"], 6, pred, goal, False, *st)
        kw = dict(renorm=renorm, dist_kind=dist_kind, w=c["w"], nn_idx=c["nn_idx"], one_d=True)
        d = rs.update(c["adv"], c["ori"], *args, rot=c["rot"], inv=inv, **kw)
        r = rr.update(c["adv"], c["ori"], full, *args, rot=c["rot"], inv=inv_b, **kw)
        assert d["upd_o"].tolist() == [True, False, True]
        for k in d:
            assert torch.equal(d[k], r[k]), k


def test_ragged_restatement_pads_with_row_zero_and_divides_by_the_length():
    E = 2
    c = _case(E)
    idx = torch.stack([torch.stack([torch.cat([torch.randperm(2 * L - 1)[:L] + 1, torch.zeros(KMAX - L, dtype=torch.long)])
                                    for L in LENGTHS]) for _ in range(E)])
    X, cen, s, arg = rr.prepare(c["adv"], c["ori"], LENGTHS, c["rot"], idx, True)
    X = X.reshape(1 + E, B, 3, KMAX)
    for b, L in enumerate(LENGTHS):
        assert torch.equal(X[:, b, :, L:], X[:, b, :, :1].expand(-1, -1, KMAX - L))
        assert torch.allclose(cen[0, b], c["adv"][b, :, :L].sum(-1) / L, rtol=0, atol=1e-15)
        assert int(arg[0, b]) < L
        # a renormalised cloud: its largest norm is 1
        assert abs(float(X[0, b, :, :L].norm(dim=0).max()) - 1.0) < 1e-12


def test_ragged_draw_statement_is_the_dense_one_at_every_length():
    rot, idx, inv = rr.draw(77, 5, 3, [40, 33, 2, 1, 33], 40)
    assert np.array_equal(rot, dr.rotation(77, 5, 3))
    for b, L in enumerate([40, 33, 2, 1, 33]):
        _, di, dv = dr.draw(77, 5, 3, L)
        assert np.array_equal(idx[b, :L], di) and np.array_equal(inv[b, :L], dv)
        assert (idx[b, L:] == di[0]).all() and (inv[b, L:] == -1).all()
        assert 1 <= idx[b].min() and idx[b, :L].max() <= 2 * L - 1
    assert np.array_equal(idx[1], idx[4]) and np.array_equal(inv[1], inv[4])        # equal lengths, equal tables
    assert idx[3].tolist() == [1] * 40                                              # one point: column 1 of cat((x, x))


# ----------------------------------------------------------------------------------------------------------------------
# the entries
# ----------------------------------------------------------------------------------------------------------------------
def test_the_three_entries_are_exported_declared_and_listed(pc3d):
    lib = pc3d.load()
    header = open(os.path.join(ROOT, "include", "pc3d.h")).read()
    pointer = _lib.SIGNATURES["pc3d_pad_ragged_f32"][4]
    for name in ENTRIES:
        assert hasattr(lib, name), name
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert decl is not None, name
        sig, dsig = _lib.SIGNATURES[name], _lib.SIGNATURES[name.replace("_ragged", "")]
        assert len(sig) == len(decl.group(1).split(",")), name
        # the dense signature with lengths behind the sizes — the draw gains the batch size as well
        extra = 2 if "draw" in name else 1
        assert len(sig) == len(dsig) + extra and pointer in sig
    for f in (ops.eot_prepare, ops.eot_update, ops.eot_draw):
        params = inspect.signature(f).parameters
        assert list(params)[-1] == "lengths" and params["lengths"].default is None


def test_c_entries_refuse_null_lengths_and_mirror_the_dense_checks(pc3d):
    lib = pc3d.load()
    fake = 4096

    def err():
        return lib.pc3d_last_error().decode()
    # B = 0 returns before any pointer is looked at, as the dense entries do
    assert lib.pc3d_eot_prepare_ragged_f32(0, 0, 0, 40, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0) == 0
    # lengths NULL
    assert lib.pc3d_eot_prepare_ragged_f32(fake, fake, 2, 40, 0, 0, 1, 0, 0, 0, 0, 0, fake, fake, fake, 0) == -22
    assert err().startswith("pc3d_eot_prepare_ragged_f32:") and "null pointer" in err()
    assert lib.pc3d_eot_draw_ragged_f32(1, 0, 0, 1, 2, 3, 2, 40, 0, fake, fake, fake, 0) == -22
    assert err().startswith("pc3d_eot_draw_ragged_f32:") and "null pointer" in err()
    upd = [fake] * 5 + [2, 40, 0, 0, 1, 0, 0, 0, 0, 0] + [fake] * 2 + [0] + [fake] * 5 + [0, 0, 0, 1, fake, 0, 2, 1e-2, 0.9, 0.999,
                                                                                    1e-8, 1, 0.4, 0, 1, 0]
    assert lib.pc3d_eot_update_ragged_f32(*upd) == -22
    assert err().startswith("pc3d_eot_update_ragged_f32:") and "null pointer" in err()
    # the dense entries' own checks in the twin's name: the cap is the capacity's
    assert lib.pc3d_eot_prepare_ragged_f32(fake, fake, 2, 8193, fake, 0, 1, 0, 0, 0, 0, 0, fake, fake, fake, 0) == -22
    assert "pc3d_eot_prepare_ragged_f32: bad sizes" in err() and "K=8193" in err()
    assert lib.pc3d_eot_draw_ragged_f32(1, 0, 0, 1, 2, 3, 2, 8193, fake, fake, fake, fake, 0) == -22
    assert "pc3d_eot_draw_ragged_f32: K=8193 out of range" in err()
    assert lib.pc3d_eot_draw_ragged_f32(1, 0, 1, 2, 2, 3, 2, 40, fake, fake, fake, fake, 0) == -22
    assert "leave the table" in err()
    # ... and the dense entries still speak in their own
    assert lib.pc3d_eot_draw_f32(1, 0, 0, 1, 2, 3, 8193, fake, fake, fake, 0) == -22
    assert err().startswith("pc3d_eot_draw_f32: K=8193 out of range")


# ----------------------------------------------------------------------------------------------------------------------
# the gates of CW.attack(lengths=...)
# ----------------------------------------------------------------------------------------------------------------------
class _NoPadPointNet(pointnet.PointNetCls):
    pad_invariant = False


def _attack(victim=None, **over):
    kw = dict(binary_step=1, num_iter=2, whether_target=True, whether_1d=True, whether_3Dtransform=True,
              whether_renormalization=True, whether_resample=True, device="cpu", graph=False, device_loop=True, device_rng=True,
              seed=5)
    kw.update(over)
    victim = pointnet.PointNetCls(k=40).eval() if victim is None else victim
    return cwm.CW(victim, cwm.AdvLossAdapter(adv_u.LogitsAdvLoss(0.), adv_u.UntargetedLogitsAdvLoss(0.)),
                  cwm.PerSampleDist(dist_u.ChamferDist()), **kw)


def _batch():
    g = torch.Generator().manual_seed(0)
    return torch.randn((B, KMAX, 3), generator=g), torch.tensor([1, 2, 3]), torch.tensor([4, 5, 6])


@pytest.fixture
def no_launch(monkeypatch):
    names = []

    def boom(name, *a):
        names.append(name)
        raise AssertionError(f"{name}: a launch before the refusal")
    monkeypatch.setattr(_lib, "call", boom)
    return names


def test_every_gate_raises_before_any_launch(no_launch):
    data, target, origin = _batch()
    sor = defense.SORDefense(k=2, alpha=1.1, npoint=KMAX)
    cases = {
        "device_loop=False": _attack(device_loop=False),
        "no device-loop plan": _attack(),                                         # a CPU victim has no plan
        "_NoPadPointNet does not declare pad_invariant": _attack(_NoPadPointNet(k=40).eval()),
        "FusedDefended does not declare pad_invariant": _attack(defense.FusedDefended(pointnet.PointNetCls(k=40).eval(), sor)),
        "whether_resample needs device_rng=True": _attack(device_rng=False),
    }
    for what, atk in cases.items():
        with pytest.raises(ValueError, match=WHO) as e:
            atk.attack(data, target, origin, lengths=LENGTHS)
        assert what in str(e.value), (what, str(e.value))
    # rotations without resampling do not depend on a length: host draws pass that gate (the next one, the plan, fires)
    with pytest.raises(ValueError, match="no device-loop plan"):
        _attack(device_rng=False, whether_resample=False).attack(data, target, origin, lengths=LENGTHS)
    assert no_launch == []


def test_bad_lengths_raise_before_any_launch(no_launch):
    data, target, origin = _batch()
    atk = _attack()
    for bad in ([40, 33], [40, 33, 2, 2], [40., 33., 2.], np.array([40., 33., 2.]), torch.tensor([40., 33., 2.]),
                [41, 33, 2], [40, 33, 0], torch.tensor([40, 33, -1])):
        with pytest.raises(ValueError, match=WHO + ": lengths must"):
            atk.attack(data, target, origin, lengths=bad)
    with pytest.raises(ValueError, match=r"\[1, Kmax=40\]"):
        atk.attack(data, target, origin, lengths=[40, 33, 0])
    with pytest.raises(ValueError, match=r"data must be \[B, Kmax, 3\]"):
        atk.attack(data.transpose(1, 2), target, origin, lengths=LENGTHS)
    big = torch.zeros((1, ops.EOT_MAX_POINTS + 1, 3))
    with pytest.raises(ValueError, match="exceeds EOT_MAX_POINTS"):
        atk.attack(big, target[:1], origin[:1], lengths=[5])
    # good lengths in every spelling pass the check: the gate behind it (no plan on the CPU) fires
    for good in (LENGTHS, np.array(LENGTHS), torch.tensor(LENGTHS), np.array(LENGTHS, dtype=np.int32)):
        with pytest.raises(ValueError, match="no device-loop plan"):
            atk.attack(data, target, origin, lengths=good)
    assert no_launch == []


# ----------------------------------------------------------------------------------------------------------------------
# the loop key; lengths=None
# ----------------------------------------------------------------------------------------------------------------------
def _plan(atk, **more):
    """A plan as CW._device_loop_plan spells it (it refuses a CPU victim itself)."""
    victim = graphed.unwrap(atk.model)
    E = atk.EOT_VIEWS
    return dict(victim=victim, kind=("logits", 0.0), dist_kind="chamfer", E=E, renorm=True, resample=True, prepare=True,
                one_d=True, untarget=False, box=0.4, scale=1.0 / (E * B), **more)


def test_the_loop_key_carries_the_flag_and_never_the_lengths():
    atk = _attack()
    assert atk._device_loop_plan(B, KMAX) is None and atk._device_loop_plan(B, KMAX, ragged=True) is None
    dense, ragged = _plan(atk), _plan(atk, ragged=True)
    kd, kr = atk._loop_key(dense, B, KMAX), atk._loop_key(ragged, B, KMAX)
    # the dense key is what it was
    assert kd == graphed.loop_key(dense["victim"], atk.device, B, KMAX, float(atk.attack_lr), True, 5, False,
                                  tuple(sorted((n, v) for n, v in dense.items() if n != "victim")))
    assert kr != kd and any(("ragged", True) in part for part in kr if isinstance(part, tuple))
    assert not any(("ragged", True) in part for part in kd if isinstance(part, tuple))
    # two sets of lengths: one key (nothing of the lengths is in a plan, and attack() hands them over as data)
    assert atk._loop_key(_plan(atk, ragged=True), B, KMAX) == kr
    assert "lengths" not in inspect.signature(atk._loop_key).parameters
    assert "lengths" not in inspect.signature(atk._device_loop_state).parameters
    # global_batch is part of what a captured loop bakes in
    assert atk._loop_key(_plan(atk, batch_mean=7), B, KMAX) != kd


def test_lengths_none_is_the_default():
    params = inspect.signature(cwm.CW.attack).parameters
    assert list(params) == ["self", "data", "target", "origin_label", "lengths"] and params["lengths"].default is None
    init = inspect.signature(cwm.CW.__init__).parameters
    assert list(init)[-2:] == ["sample_seeds", "global_batch"]
    assert init["sample_seeds"].default is None and init["global_batch"].default is None
    atk = _attack()
    assert atk.sample_seeds is None and atk.global_batch is None


def test_sample_seeds_draw_every_cloud_from_its_own_generator(monkeypatch):
    """The 1e-7 start noise on the autograd path of a CPU attack: with sample_seeds the iterate of cloud b starts from
    generator b's draw whatever the batch; without, from the one batch-shaped draw of torch's global generator."""
    data, target, origin = _batch()
    for seeds in (None, [11, 12, 13]):
        atk = _attack(device_loop=False, whether_3Dtransform=False, whether_renormalization=False, sample_seeds=seeds)
        ori = data.transpose(1, 2).contiguous()
        calls = []

        def fwd(x, calls=calls):
            calls.append(x.detach().clone())
            if len(calls) == 2:
                raise RuntimeError("stop")
            return torch.zeros((x.shape[0], 40))
        monkeypatch.setattr(atk, "_forward", fwd)
        torch.manual_seed(123)
        with pytest.raises(RuntimeError, match="stop"):
            atk.attack(data, target, origin)
        if seeds is None:
            torch.manual_seed(123)
            want = ori + torch.randn((B, 3, KMAX)) * 1e-7
        else:
            want = ori + torch.stack([torch.randn((3, KMAX), generator=torch.Generator().manual_seed(s)) for s in seeds]) * 1e-7
        assert torch.equal(calls[1], want)
