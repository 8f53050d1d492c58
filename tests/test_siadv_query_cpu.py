"""CPU: SI-Adv's query attacks against tests/golden/siadv_query.npz (the real reference's simba_attack and
shape_invariant_query_attack run on the CPU one cloud at a time, see tests/golden/make_golden_siadv_query.py).

  * the batched restatement (tests/siadv_query_restatement.py), in fp32 and in float64, reproduces the stored accept
    sequence and query_costs exactly, the losses within band_loss and the points within band_P;
  * the mirror's host draw reproduces the stored simba tables from the stored seed, skipping the early-return clouds;
  * PointCloudAttack has the reference's three method names, and refuses CPU tensors by name.
"""
import copy
import importlib
import os
import types

import numpy as np
import pytest
import torch

import siadv_query_restatement as Q
from conftest import GOLDEN

CASES = ("simba", "ours", "ours_top5")


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "siadv_query.npz"))


@pytest.fixture(scope="module")
def models():
    from oracle import ref_torch as ort
    out = []
    for seed in (3, 4):
        m = ort.PointNetCls(k=40)
        m.load_state_dict(ort.seeded_state_dict(m, seed))
        out.append(m.eval())
    return out


def _mirror():
    return importlib.import_module("3dpointcloudattack_amd.attack.SIadv.SIadv_attack")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_fixture(fx, models, case, dtype):
    tgt = copy.deepcopy(models[1]).to(dtype)
    P, target = torch.from_numpy(fx[f"{case}_points"]).to(dtype), torch.from_numpy(fx[f"{case}_target"])
    signs = torch.tensor(Q.sign_order(float(fx["step_size"])), dtype=dtype)
    assert tuple(fx["signs"]) == Q.sign_order(float(fx["step_size"]))      # the set's order here is the generator's
    frame = None
    if case != "simba":
        frame = (torch.from_numpy(fx[f"{case}_nrm"]).to(dtype), torch.from_numpy(fx[f"{case}_dir"]).to(dtype))
    early = torch.from_numpy(fx[f"{case}_early"])
    q = Q.run_query(tgt, P, target, fx[f"{case}_tab"], signs, case == "ours_top5", frame, active=~early)
    assert np.array_equal(q["accepted"].numpy(), fx[f"{case}_accepted"])
    assert np.array_equal(q["query_costs"].numpy(), fx[f"{case}_query_costs"])
    assert np.array_equal(q["adv_target"].numpy(), fx[f"{case}_adv_target"])
    band_loss, band_P = float(fx[f"{case}_band_loss"]), float(fx[f"{case}_band_P"])
    dl = np.nanmax(np.abs(q["losses"].double().numpy() - fx[f"{case}_loss"]))
    dP = float((q["adv_points"].double() - torch.from_numpy(fx[f"{case}_adv_points"]).double()).abs().max())
    print(f"{case} {dtype}: losses off by {dl:.3e} (band_loss {band_loss:.3e}), points by {dP:.3e} (band_P {band_P:.3e})")
    assert dl <= band_loss and dP <= band_P
    if case == "simba":
        assert early.any() and torch.equal(q["adv_points"][early], P[early])
        if dtype == torch.float32:
            assert np.array_equal(q["adv_points"].numpy(), fx["simba_adv_points"])       # the same fp32 additions


def test_fixture_covers_the_three_ways_a_simba_loop_ends(fx):
    acc, early, best = fx["simba_accepted"], fx["simba_early"], fx["simba_best"]
    ends = (acc != -2).sum(1)
    L = acc.shape[1]
    assert L == 192 and early.any() and (ends[early] == 0).all()
    assert any(not early[b] and ends[b] == L and best[b, -1] < 0 for b in range(4))
    assert any(not early[b] and 0 < ends[b] < L and best[b, ends[b] - 1] >= 0 and (acc[b, :ends[b]] != 0).any() for b in range(4))
    for case in CASES:                                                  # no decision inside the band
        prev = np.concatenate([np.full((4, 1), -999.), fx[f"{case}_best"][:, :-1]], 1)
        a = fx[f"{case}_accepted"]
        m0 = np.abs(fx[f"{case}_loss"][:, :, 0] - prev)[a != -2]
        m1 = np.abs(fx[f"{case}_loss"][:, :, 1] - prev)[(a == 1) | (a == -1)]
        assert min(m0.min(), m1.min()) > float(fx[f"{case}_band_loss"])


def test_host_draw_reproduces_the_stored_tables(fx):
    si = _mirror()
    early = fx["simba_early"]
    np.random.seed(int(fx["simba_np_seed"]))
    tab = si.draw_simba_tables(64, ~early)
    assert tab.dtype == np.int32 and np.array_equal(tab, fx["simba_tab"])
    assert (tab[early] == 0).all() and all(sorted(tab[b].tolist()) == list(range(192)) for b in range(4) if not early[b])
    np.random.seed(int(fx["simba_np_seed"]))                            # an early return consumes no draw
    assert not np.array_equal(si.draw_simba_tables(64, np.ones(4, bool)), fx["simba_tab"])
    assert np.array_equal(si.simba_basis(2), np.array([(0, 0), (1, 0), (2, 0), (0, 1), (1, 1), (2, 1)]))
    np.random.seed(int(fx["simba_np_seed"]))
    assert np.array_equal(Q.draw_simba_tables(64, ~early), fx["simba_tab"])
    assert si.sign_order(0.32) == tuple({0.32, -0.32})


def test_method_names_exist_and_refuse_cpu_tensors(fx, models):
    si = _mirror()
    for method, name in (("simba", "simba_attack"), ("simbapp", "simbapp_attack"), ("ours", "shape_invariant_query_attack")):
        assert callable(getattr(si.PointCloudAttack, name, None)), name
        a = types.SimpleNamespace(eps=0.16, step_size=0.32, max_steps=1, num_class=40, top5_attack=False, defense_method=None,
                                  transfer_attack_method=None, query_attack_method=method)
        atk = si.PointCloudAttack(a, wb_classifier=models[0], classifier=models[1])
        with pytest.raises(NotImplementedError, match=f"{method}.*GPU only"):
            getattr(atk, name)(torch.from_numpy(fx["simba_points"]), torch.from_numpy(fx["simba_target"]))


def test_argument_errors_do_not_touch_the_gpu(pc3d):
    lib = pc3d.load()
    assert lib.pc3d_si_rank_f32(None, 0, 0, 0, None, 0, 0, 0, 1, 8193, None, None, None, None, None) == -22
    assert b"limit of 8192" in lib.pc3d_last_error()                    # the keys are sorted in LDS: refused above it
    assert lib.pc3d_si_rank_f32(None, 0, 0, 0, None, 0, 0, 0, 0, 64, None, None, None, None, None) == 0
    step = [None, 40, None, 3] + [None, 0, 0, 0] * 3 + [None, 4, None, None, 0, 0] + [None] * 7 + [None, 0, 0, 0] * 2 \
        + [None, None, 1, 64, 0, None]
    assert lib.pc3d_query_step_f32(*step) == -22 and b"top must be 1 or 5" in lib.pc3d_last_error()
    step[3], step[1] = 5, 300
    assert lib.pc3d_query_step_f32(*step) == -22 and b"k=300" in lib.pc3d_last_error()
    step[1], step[-4] = 40, 0
    assert lib.pc3d_query_step_f32(*step) == 0                          # an empty batch is a no-op
