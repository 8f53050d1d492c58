"""CPU: the SOR / SRS defence heads against tests/golden/defense.npz (the REAL reference, tests/golden/make_golden_defense.py).

The plain-torch restatement of the reference's SOR lives here (``RestatedSOR``: expansion-form float64 matrix, topk,
per-sample mask loop, the cyclic padding rule); the GPU tests import it as their same-device baseline.
"""
import importlib
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

# Tie band of the random-shape sweeps (the fixture cases carry their own, measured by the generator): the fp32
# direct-difference form deviates from the float64 value by the rounding of the subtraction (<= 1/2 ulp of the
# difference, doubled by the square), the square, two additions and the mean over k — about 4 ulp = 4 * 2^-24 relative on
# v, less on thr (a mean over K values). The generator measured 1.4e-7 .. 2.0e-7 on the fixture cases, inside that
# figure. 16 x for a different summation order on the device, as for the fixtures.
SWEEP_BAND = 16 * 4 * 2.0 ** -24
SWEEP_CAP = 1e-4              # share of sweep points that may sit inside the band
# (B, K, k, npoint, alpha) of the sweep: K in 64 .. 4096, npoint >= K, k in 1 .. 8, B in {1, 3, 32}; fixed seeds
SWEEP = [(1, 64, 1, 64, 1.1), (3, 100, 3, 128, 1.1), (32, 256, 2, 256, 1.1), (1, 777, 8, 1024, 1.05),
         (3, 1024, 2, 1024, 1.1), (32, 512, 4, 600, 1.0), (1, 4096, 2, 4096, 1.1), (3, 2048, 5, 2048, 1.1),
         (32, 1024, 2, 1024, 1.1), (1, 3000, 1, 4096, 1.2), (3, 333, 7, 1000, 1.1), (1, 4096, 8, 4096, 1.1)]


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "defense.npz"))


def cases(fx):
    for name in fx["cases"]:
        k, alpha, npoint, band = fx[f"{name}_cfg"]
        yield str(name), int(k), float(alpha), int(npoint), float(band)


def outlier_cloud(rng, n):
    """Unit-ball cloud with every 13th point pushed out by N(0, 0.05^2), as the fixture generator makes them."""
    g = rng.standard_normal((n, 3))
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    p = g * rng.random((n, 1)) ** (1.0 / 3.0)
    p = p - p.mean(axis=0, keepdims=True)
    p = (p / np.max(np.linalg.norm(p, axis=1))).astype(np.float32)
    p[::13] += (0.05 * rng.standard_normal(p[::13].shape)).astype(np.float32)
    return p


def sweep_clouds(i):
    B, K, k, npoint, alpha = SWEEP[i]
    rng = np.random.default_rng(5000 + i)
    return np.stack([outlier_cloud(rng, K) for _ in range(B)]).transpose(0, 2, 1).copy()       # [B,3,K]


class RestatedSOR(torch.nn.Module):
    """The reference's algorithm in plain torch on whatever device x lives on. form "expansion64": the [B,K,K] matrix as
    xx - 2 x.x^T + xx^T in float64 (the reference); "direct32": ((p_i - p_j)^2).sum in fp32 (what the device computes).
    After a forward: v, thr, mask, n (tensors), src [B,npoint] and min_margin = min |v - thr| / thr over all calls."""

    def __init__(self, k=2, alpha=1.1, npoint=1024, form="expansion64"):
        super().__init__()
        self.k, self.alpha, self.npoint, self.form = k, alpha, npoint, form
        self.min_margin = None

    def stats(self, x):
        if self.form == "expansion64":
            pc = x.detach().double().transpose(1, 2)                      # [B,K,3]
            inner = -2.0 * torch.matmul(pc, pc.transpose(2, 1))
            xx = torch.sum(pc ** 2, dim=2, keepdim=True)
            dist = xx + inner + xx.transpose(2, 1)
        else:
            pc = x.detach().float()
            dist = sum((pc[:, c, :, None] - pc[:, c, None, :]) ** 2 for c in range(3))
        value = -((-dist).topk(k=self.k + 1, dim=-1)[0][..., 1:])
        v = value.mean(-1)
        thr = v.mean(-1) + self.alpha * v.std(-1)
        return v, thr

    def forward(self, x):
        v, thr = self.stats(x)
        mask = v <= thr[:, None]
        self.v, self.thr, self.mask, self.n = v, thr, mask, mask.sum(1)
        m = ((v - thr[:, None]).abs() / thr[:, None]).min()
        self.min_margin = m if self.min_margin is None else torch.minimum(self.min_margin, m)
        outs, srcs = [], []
        ar = torch.arange(self.npoint, device=x.device)
        for b in range(x.shape[0]):                                       # the reference's per-sample loop
            kept = torch.nonzero(mask[b])[:, 0]
            src = kept[ar % kept.numel()]
            srcs.append(src)
            outs.append(x[b][:, src])
        self.src = torch.stack(srcs)
        return torch.stack(outs)


def test_restatement_reproduces_every_fixture_case(fx):
    """mask, n_b, src, output (bit-equal to the gathered input) and the input gradient of (out * G).sum()."""
    for name, k, alpha, npoint, band in cases(fx):
        x = torch.from_numpy(fx[f"{name}_x"])
        head = RestatedSOR(k, alpha, npoint)
        x64 = x.double().requires_grad_()
        out64 = head(x64)
        assert np.array_equal(head.mask.numpy(), fx[f"{name}_mask"]), name
        assert np.array_equal(head.n.numpy(), fx[f"{name}_n"]), name
        np.testing.assert_allclose(head.v.numpy(), fx[f"{name}_v"], rtol=1e-12, atol=1e-18, err_msg=name)
        np.testing.assert_allclose(head.thr.numpy(), fx[f"{name}_thr"], rtol=1e-12, err_msg=name)
        out = head(x)
        assert np.array_equal(out.numpy(), fx[f"{name}_out"]), name
        (out64 * torch.from_numpy(fx[f"{name}_G"]).double()).sum().backward()
        np.testing.assert_allclose(x64.grad.numpy(), fx[f"{name}_grad"], rtol=1e-6, err_msg=name)
        assert np.all(x64.grad.numpy()[~np.repeat(fx[f"{name}_mask"][:, None, :], 3, 1)] == 0.0), name


def test_padding_is_cyclic_over_the_kept_points(fx):
    """out[b,:,j] = x[b,:,kept_b[j mod n_b]] against the REFERENCE's stored outputs, bit for bit."""
    for name, k, alpha, npoint, band in cases(fx):
        x, out, mask, n = fx[f"{name}_x"], fx[f"{name}_out"], fx[f"{name}_mask"], fx[f"{name}_n"]
        assert out.shape == (x.shape[0], 3, npoint)
        for b in range(x.shape[0]):
            kept = np.nonzero(mask[b])[0]
            assert len(kept) == n[b] >= 1
            assert np.array_equal(out[b], x[b][:, kept[np.arange(npoint) % n[b]]]), (name, b)
    assert int(fx["wrap_cfg"][2]) // int(fx["wrap_n"].max()) >= 4         # the wrap-around case repeats several times


def test_no_fixture_point_inside_the_tie_band(fx):
    for name, k, alpha, npoint, band in cases(fx):
        v, thr = fx[f"{name}_v"], fx[f"{name}_thr"]
        margin = np.min(np.abs(v - thr[:, None]) / thr[:, None])
        assert 0 < band < 1e-5 and margin > band, (name, margin, band)
        # and the fp32 direct form (what the device computes) stays within band / 16 of the reference, mask included
        head = RestatedSOR(k, alpha, npoint, form="direct32")
        head(torch.from_numpy(fx[f"{name}_x"]))
        assert np.max(np.abs(head.thr.double().numpy() - thr) / thr) <= band / 16 * 1.0000001, name
        assert np.max(np.abs(head.v.double().numpy() - v) / np.maximum(v, thr[:, None])) <= band / 16 * 1.0000001, name
        assert np.array_equal(head.mask.numpy(), fx[f"{name}_mask"]), name


def test_sweep_float64_vs_fp32_restatement_within_cap():
    """The sweep the GPU test runs, on the restatement alone: its fp32 direct form against its float64 form; points
    outside the band must agree, at most SWEEP_CAP of all points may sit inside it."""
    total = excused = 0
    for i, (B, K, k, npoint, alpha) in enumerate(SWEEP):
        x = torch.from_numpy(sweep_clouds(i))
        for b in range(B):                                                # per cloud: bounds the [K,K] temporaries
            r64, r32 = RestatedSOR(k, alpha, npoint), RestatedSOR(k, alpha, npoint, form="direct32")
            r64(x[b:b + 1])
            r32(x[b:b + 1])
            inside = ((r64.v - r64.thr[:, None]).abs() <= SWEEP_BAND * r64.thr[:, None])
            assert torch.equal(r64.mask[~inside], r32.mask[~inside]), (i, b)
            total += inside.numel()
            excused += int(inside.sum())
    print(f"sweep: {excused} of {total} points inside the band")
    assert excused <= SWEEP_CAP * total, (excused, total)


def test_dropin_paths_import(pc3d):
    m = importlib.import_module
    d = m("3dpointcloudattack_amd.defense")
    pkg = m("3dpointcloudattack_amd.attack.SIadv.baselines.defense.drop_points")
    assert m("3dpointcloudattack_amd.attack.SIadv.baselines.defense.drop_points.SOR").SORDefense is d.SORDefense
    assert m("3dpointcloudattack_amd.attack.SIadv.baselines.defense.drop_points.SRS").SRSDefense is d.SRSDefense
    assert pkg.SORDefense is d.SORDefense and pkg.SRSDefense is d.SRSDefense
    sor, srs = d.SORDefense(), d.SRSDefense()
    assert (sor.k, sor.alpha, sor.npoint, srs.drop_num, srs.device_rng) == (2, 1.1, 1024, 500, False)
    assert isinstance(d.Defended(torch.nn.Identity(), sor), torch.nn.Module)
    pc3d.install_dropin()
    try:
        assert m("attack.SIadv.baselines.defense.drop_points.SOR").SORDefense is d.SORDefense
    finally:
        pc3d.uninstall_dropin()


def test_srs_host_mode_draws_the_reference_tables(fx):
    d = importlib.import_module("3dpointcloudattack_amd.defense")
    B, _, K = fx["k1024_x"].shape
    for drop in fx["srs_drops"]:
        np.random.seed(int(fx["srs_seed"]))
        idx = d.SRSDefense(drop_num=int(drop)).draw_host(B, K)
        assert np.array_equal(idx, fx[f"srs{int(drop)}_idx"])
        assert idx.shape == (B, K - int(drop))


def test_value_errors_come_from_the_shapes_alone():
    d = importlib.import_module("3dpointcloudattack_amd.defense")
    with pytest.raises(ValueError, match="npoint"):
        d.SORDefense(npoint=1024)(torch.zeros(2, 3, 1025))                # K > npoint (CPU tensor: never reaches a device)
    with pytest.raises(ValueError, match="neighbours"):
        d.SORDefense(k=5, npoint=8)(torch.zeros(1, 3, 5))                 # K < k + 1
    with pytest.raises(ValueError):
        d.SORDefense()(torch.zeros(2, 1024, 3))                           # not channel-first
    with pytest.raises(ValueError):
        d.SRSDefense(drop_num=64).draw_host(1, 64)                        # nothing left
    with pytest.raises(Exception, match="GPU only"):
        d.SORDefense()(torch.zeros(1, 3, 64))                             # no CPU fallback
    with pytest.raises(Exception, match="GPU only"):
        d.SRSDefense(drop_num=3)(torch.zeros(1, 3, 64))
    with pytest.raises(ValueError):
        d.evaluate_defended(torch.nn.Identity(), d.SORDefense(), np.zeros((2, 5, 4), np.float32), np.zeros(2))


def test_entry_points_check_arguments_before_launching(pc3d):
    _lib = importlib.import_module("3dpointcloudattack_amd._lib")
    lib = pc3d.load()
    for n in ("pc3d_sor_select_f32", "pc3d_sor_fused_f32", "pc3d_sor_bwd_f32", "pc3d_srs_select_i32",
              "pc3d_gather_points_f32"):
        assert n in _lib.SIGNATURES
    z = (None, 0, 0, 0)
    sel = lambda B, K, k1, npoint: lib.pc3d_sor_select_f32(None, *z, B, K, k1, 1.1, npoint, None, None, None, None, None, *z, None)  # noqa: E731
    assert sel(1, 1024, 3, 512) == -22 and b"npoint" in lib.pc3d_last_error()
    assert sel(1, 2, 3, 1024) == -22
    assert sel(1, 100000, 3, 100000) == -22 and b"limit" in lib.pc3d_last_error()
    assert sel(1, 1024, 3, 1024) == -22 and b"null" in lib.pc3d_last_error()
    assert sel(0, 1024, 3, 1024) == 0                                     # empty batch: a no-op
    fus = lambda B, K, k1: lib.pc3d_sor_fused_f32(*z, B, K, k1, 1.1, K, None, None, None, None, None, None, *z, None)  # noqa: E731
    assert fus(1, 8192, 3) == -22 and fus(1, 1024, 12) == -22 and fus(0, 1024, 3) == 0
    assert lib.pc3d_sor_bwd_f32(*z, None, None, 1, 0, 8, *z, None) == -22
    assert lib.pc3d_sor_bwd_f32(*z, None, None, 0, 8, 8, *z, None) == 0
    assert lib.pc3d_srs_select_i32(1, None, 0, 1, 1024, 2000, None, None) == -22
    assert lib.pc3d_srs_select_i32(1, None, 0, 1, 8192, 10, None, None) == -22 and b"limit" in lib.pc3d_last_error()
    assert lib.pc3d_srs_select_i32(1, None, 0, 0, 1024, 10, None, None) == 0
    assert lib.pc3d_gather_points_f32(*z, None, 1, 0, 4, *z, None) == -22
    assert lib.pc3d_gather_points_f32(*z, None, 0, 4, 4, *z, None) == 0
