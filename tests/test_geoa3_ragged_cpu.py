"""CPU: the host side of the ragged GeoA3 device loop — the refusals, which fire before any device call;
what an absent `cfg.lengths` leaves as it was; the C entry's argument checks; and the condition the GPU file's float64 comparison
rests on: at every length of tests/geoa3_ragged_cases.py the float32 and the float64 restatement take the same decisions,
with a margin (the Hausdorff arg-max, the sign of every curvature inner product, the lp_clip branch, the record)."""
import importlib
import inspect

import numpy as np
import pytest
import torch

import geoa3_ragged_cases as gc
import geoa3_step_restatement as rs
from test_oracle_golden import _geo_cfg

M = importlib.import_module
ops = M("3dpointcloudattack_amd.ops")
_lib = M("3dpointcloudattack_amd._lib")
ga = M("3dpointcloudattack_amd.attack.GeoA3.GeoA3_attack")
graphed = M("3dpointcloudattack_amd.graphed")
pointnet = M("3dpointcloudattack_amd.model.pointnet")
cloud_io = M("3dpointcloudattack_amd.dataset.cloud_io")


class _NoPadPointNet(pointnet.PointNetCls):
    pad_invariant = False


def _batch(sizes=(40, 33, 17)):
    rng = np.random.default_rng(0)
    data, lengths = cloud_io.stack_ragged([rng.standard_normal((n, 3)).astype(np.float32) for n in sizes])
    return torch.from_numpy(data), torch.tensor([1, 2, 3][:len(sizes)]), lengths


def _call(victim, pc, label, lengths, **over):
    cfg = _geo_cfg(**{"device_loop": True, "lengths": lengths, **over})
    return ga.geoA3_attack(victim, None, None, None, None, None, pc, label, cfg, 0, 1)


@pytest.fixture
def no_device_call(monkeypatch):
    """Any call into the library, any estimate of normals and any loop state is a failure."""
    def boom(*a, **k):
        raise AssertionError("a device call before the refusal")
    monkeypatch.setattr(_lib, "call", boom)
    monkeypatch.setattr(ga, "_device_loop_state", boom)
    monkeypatch.setattr(ga, "estimate_normal", boom)
    monkeypatch.setattr(ga, "estimate_normal_ragged", boom)


def test_every_refusal_fires_before_any_device_call(no_device_call):
    victim = pointnet.PointNetCls(k=40).eval()
    pc, label, lengths = _batch()
    with pytest.raises(ValueError, match="cfg.device_loop is not set"):
        _call(victim, pc, label, lengths, device_loop=False)
    cfg = _geo_cfg(lengths=lengths)
    assert not hasattr(cfg, "device_loop")
    with pytest.raises(ValueError, match="cfg.device_loop is not set"):
        ga.geoA3_attack(victim, None, None, None, None, None, pc, label, cfg, 0, 1)
    # a wrong count, floats, a length below max(4, curv_loss_knn + 1) = 17 and one beyond Kmax
    for bad in ([40, 33], [40, 33, 17, 17], [40., 33., 17.], [40, 33, 16], [41, 33, 17], [40, 33, 0]):
        with pytest.raises(ValueError, match="lengths must"):
            _call(victim, pc, label, bad)
    with pytest.raises(ValueError, match=r"max\(4, curv_loss_knn \+ 1\)=4"):        # without curvature: the normals' k = 3 search
        _call(victim, pc, label, [40, 33, 3], curv_loss_weight=0)
    with pytest.raises(ValueError, match="must be \\[B, Kmax, 3\\]"):
        _call(victim, pc.transpose(1, 2), label, lengths)
    # Kmax and k outside ops.geoa3_update_fits
    n = ops.GEOA3_LOOP_MAX_POINTS + 1
    with pytest.raises(ValueError, match="GEOA3_LOOP_MAX_POINTS"):
        _call(victim, torch.zeros(1, n, 3), label[:1], [n])
    assert ops.geoa3_update_fits(2048, 20) and not ops.geoa3_update_fits(2048, 21)
    with pytest.raises(ValueError, match="160 KiB"):
        _call(victim, torch.zeros(1, 2048, 3), label[:1], [2048], curv_loss_knn=21)
    # a victim without pad_invariant; a CPU device
    with pytest.raises(ValueError, match="pad_invariant"):
        _call(_NoPadPointNet(k=40).eval(), pc, label, lengths)
    with pytest.raises(ValueError, match="needs a GPU"):
        _call(victim, pc, label, lengths)
    with pytest.raises(ValueError, match="needs a GPU"):
        _call(victim, pc, label, torch.tensor(lengths))


def test_signatures_keep_their_prefix():
    # the lengths are an attribute of cfg, like the mirror's other options: the function keeps the reference's parameter list
    params = list(inspect.signature(ga.geoA3_attack).parameters.values())
    assert [p.name for p in params] == ["net", "pt_model", "ptm_model", "pts_model", "dgcnn_model", "cur_model", "pc", "label",
                                        "cfg", "i", "loader_len", "saved_dir"]
    assert params[-1].default is None
    assert list(inspect.signature(ga._device_loop_plan).parameters) == ["net", "cfg", "b", "n", "targeted"]
    assert list(inspect.signature(ops.geoa3_update).parameters)[-1] == "lengths"
    assert inspect.signature(ops.geoa3_update).parameters["lengths"].default is None


def _plan(victim):
    """A plan as _device_loop_plan spells it for the default configuration (it refuses a CPU victim itself)."""
    return dict(victim=victim, kind=3, kappa=0.0, dis_kind='CD', two=True, curv=True, k=16, gval=float(np.float32(1.0) / np.float32(3)),
                w_dis=1.0, w_hd=0.1, w_curv=1.0, targeted=False, lr=0.01, scheduler=False, cc_linf=0.0, steps=12, graph=True)


def test_no_lengths_leaves_the_plan_and_the_loop_key():
    victim = pointnet.PointNetCls(k=40).eval()
    cpu = torch.device("cpu")
    assert ga._device_loop_plan(victim, _geo_cfg(device_loop=True), 3, 40, False) is None       # as before: no GPU, no plan
    plan = _plan(victim)
    dense = ga._device_loop_state(plan, 3, 40, cpu)
    # the key of the loop without lengths is what it was: the constants of the plan, nothing about lengths
    assert dense.key == graphed.loop_key(victim, cpu, 3, 40, tuple(sorted((nm, v) for nm, v in plan.items() if nm != "victim")))
    assert "lens" not in dense.bufs and "lens_host" not in dense.bufs
    ragged = ga._device_loop_state(dict(plan, ragged=True), 3, 40, cpu)
    assert ragged is not dense and ragged.key != dense.key
    assert set(ragged.key[2]) - set(dense.key[2]) == {("ragged", True)} and ragged.key[:2] == dense.key[:2]
    # ONE int32 device buffer holds the lengths; the key carries the flag, not the lengths: other lengths find the same loop
    assert ragged.bufs["lens"].dtype == torch.int32 and tuple(ragged.bufs["lens"].shape) == (3,)
    ragged.bufs["lens"].copy_(torch.tensor([40, 33, 17], dtype=torch.int32))
    assert ga._device_loop_state(dict(plan, ragged=True), 3, 40, cpu) is ragged
    assert ga._device_loop_state(plan, 3, 40, cpu) is dense
    assert set(ragged.bufs) - set(dense.bufs) == {"lens", "lens_host"}


def test_seeded_start_offsets_are_what_every_cloud_draws_alone():
    cfg = _geo_cfg(sample_seeds=[5, 6, 7])
    lens = np.array([40, 33, 17])
    gens = [torch.Generator().manual_seed(s) for s in cfg.sample_seeds]
    alone = [torch.Generator().manual_seed(s) for s in cfg.sample_seeds]
    for _ in range(2):          # two binary steps: the generators go on
        o = ga._draw_offset(3, 3, 40, torch.device("cpu"), cfg, gens, lens)
        assert tuple(o.shape) == (3, 3, 40)
        for b, L in enumerate(lens):
            one = ga._draw_offset(1, 3, int(L), torch.device("cpu"), cfg, [alone[b]])
            assert torch.equal(o[b, :, :L], one[0]) and not o[b, :, L:].any()
    # without lengths: the batch-shaped draw, as it was
    g1, g2 = torch.Generator().manual_seed(9), torch.Generator().manual_seed(9)
    assert torch.equal(ga._draw_offset(1, 3, 40, torch.device("cpu"), cfg, [g1]),
                       torch.zeros(3, 40).normal_(0., 1e-3, generator=g2)[None])


def _raw_update(lib, name, N, k, lengths, ptr, B=1, max_steps=1, dis_kind=0, w_hd=0.1):
    """The C entry through ctypes with `ptr` in every pointer slot (never dereferenced on the host: the argument checks come
    before any HIP call)."""
    args = [ptr] * 6 + [B, N, k] + [ptr] * 9 + [0, dis_kind, 1.0, 1.0, w_hd, 1.0, ptr, ptr, max_steps, ptr, ptr, ptr, 0] \
        + [ptr] * 6 + [0.9, 0.999, 1e-8, 0.0, None, None, None]
    if name.endswith("ragged_f32"):
        args.append(lengths)
    return getattr(lib, name)(*args, None)


def test_c_entry_refuses_null_lengths_and_bad_sizes(pc3d):
    lib = pc3d.load()
    assert _lib.SIGNATURES["pc3d_geoa3_update_ragged_f32"] == \
        _lib.SIGNATURES["pc3d_geoa3_update_f32"][:-1] + [_lib._P, _lib._P]
    name = "pc3d_geoa3_update_ragged_f32"
    fake = 4096          # a non-null address that nobody reads
    assert _raw_update(lib, name, 64, 16, None, fake) == -22 and b"null lengths" in lib.pc3d_last_error()
    assert _raw_update(lib, name, 64, 16, fake, None) == -22 and b"null pointer" in lib.pc3d_last_error()
    assert _raw_update(lib, name, 64, 16, None, None, B=0) == 0                      # an empty batch is a no-op
    for kw, word in ((dict(N=0, k=0), b"bad sizes"), (dict(N=2049, k=0), b"bad sizes"), (dict(N=64, k=64), b"out of range"),
                     (dict(N=16, k=16), b"neighbours of N=16"), (dict(N=2048, k=21), b"bytes of LDS"),
                     (dict(N=64, k=16, max_steps=0), b"max_steps"), (dict(N=64, k=16, dis_kind=2), b"dis_kind"),
                     (dict(N=64, k=0, dis_kind=1), b"no Hausdorff term")):
        for nm in (name, "pc3d_geoa3_update_f32"):          # the same checks, the same words, each under its own name
            assert _raw_update(lib, nm, lengths=fake, ptr=fake, **kw) == -22, (nm, kw)
            err = lib.pc3d_last_error()
            assert word in err and err.startswith(nm.encode() + b":"), (nm, kw, err)


def test_lds_request_is_unchanged():
    # 38 N + 2 N k + 512 with every term on: the capacity decides, not the lengths
    assert ops.geoa3_update_lds_bytes(2048, 16) == 38 * 2048 + 2 * 2048 * 16 + 512 == 143872          # 140.5 KiB
    # np = 1028: 36 np + the two reverse indices, each rounded up to 16 bytes
    assert ops.geoa3_update_lds_bytes(1025, 16) == 36 * 1028 + 32800 + 2064 + 512 == 72384
    assert ops.geoa3_update_lds_bytes(1025, 16, curv=False) == 16 * 1028 + 2064 + 512 == 19024
    assert ops.geoa3_update_lds_bytes(1025, 0, curv=False, two_sided=False) == 12 * 1028 + 512 == 12848
    assert ops.GEOA3_LOOP_MAX_POINTS == 2048 and ops.geoa3_update_fits(2048, 16) and not ops.geoa3_update_fits(2052, 16)


# ----------------------------------------------------------------------------------------------------------------------
# the decisions of the float64 comparison's inputs
# ----------------------------------------------------------------------------------------------------------------------
DECISION_CASES = [(L, gc.K) for L in gc.LENGTHS] + [(L, gc.SMALL_K) for L in gc.SMALL_LENGTHS]


@pytest.mark.parametrize("clip", [False, True], ids=["default", "clip_scheduler"])
@pytest.mark.parametrize("L,k", DECISION_CASES)
def test_fp32_and_float64_take_the_same_decisions(L, k, clip):
    over = dict(gc.CONFIGS["clip_scheduler" if clip else "default"])
    nb = gc.neighbours_f64(L, k, clip)
    for b in range(3):          # the three record branches
        inp = gc.inputs(L, k, b, clip)
        r64, r32 = rs.step(torch.float64, inp, nb, **dict(over)), rs.step(torch.float32, inp, nb, **dict(over))
        # the Hausdorff arg-max
        top = r64["d_ao"].topk(2, dim=1)[0]
        assert float(((top[:, 0] - top[:, 1]) / top[:, 0]).min()) > 1e-4
        assert torch.equal(r32["hd_arg"], r64["hd_arg"])
        # the record
        for name in rs.INT_OUT + ("pred",):
            assert torch.equal(r32[name], r64[name]), name
        assert r64["best_step"].tolist() == [over["t"] if b % 3 == 0 else -1]
        assert r64["iter_best_score"].tolist() == [int(r64["pred"][0]) if b % 3 != 2 else -1]
        if b:
            continue            # the geometry does not depend on the record state
        # the sign of every curvature inner product
        assert float(r64["inner"].min()) > 1e-6
        assert torch.equal(torch.sign(gc.signed_inner(torch.float32, inp, nb)), torch.sign(gc.signed_inner(torch.float64, inp, nb)))
        # the lp_clip branch, on Adam's result before the clip
        if clip:
            free = dict(over, cc_linf=0.)
            l64 = rs.step(torch.float64, inp, nb, **dict(free))["offset"].norm(dim=1)
            l32 = rs.step(torch.float32, inp, nb, **dict(free))["offset"].norm(dim=1)
            assert float(((l64 - gc.CC_LINF).abs() / gc.CC_LINF).min()) > 1e-5
            assert torch.equal(l32 < gc.CC_LINF, l64 < gc.CC_LINF)
            if L >= 64:
                assert bool((l64 < gc.CC_LINF).any()) and bool((l64 > gc.CC_LINF).any())
