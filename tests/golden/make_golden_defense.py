#!/usr/bin/env python3
"""Generate tests/golden/defense.npz: the REAL reference's SOR / SRS defence heads run on the CPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_defense.py

The two classes are loaded from the reference tree by file path (attack/SIadv/baselines/defense/drop_points/SOR.py and
SRS.py need nothing beyond torch and numpy). Stored per SOR case: the input cloud x [B,3,K], the reference's float64
v [B,K] and thr [B], the mask, n_b, the output [B,3,npoint], a fixed positive random G [B,3,npoint] and the input
gradient of (out * G).sum() from a float64 run of the reference (stored rounded to fp32), and `band`. For SRS: the
np.random.seed used and the drawn index tables (the reference's output is checked here to be the gather through them).

Threshold ties: the reference compares float64 expansion-form values, the device fp32 direct-difference ones. Per case
the generator measures dev = the largest relative deviation of an fp32 direct-form restatement from the reference's
v / thr, sets band = 16 * dev, and REFUSES to write a case whose smallest margin min_i |v - thr| / thr is not above
the band or whose fp32 mask differs from the float64 one — pick another seed then. It also asserts the padding rule
out[b, :, j] = x[b, :, kept_b[j mod n_b]] bit for bit against the reference output. Only data is written.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, REF, unit_cloud  # noqa: E402

SEED = 77
SRS_SEED = 1234
DROP = os.path.join(REF, "attack", "SIadv", "baselines", "defense", "drop_points")


def load(name):
    spec = importlib.util.spec_from_file_location("ref_" + name, os.path.join(DROP, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def outlier_cloud(rng, n):
    """A unit-ball cloud with every 13th point pushed out by N(0, 0.05^2): what a CW attack leaves behind."""
    p = unit_cloud(rng, n)
    p[::13] += (0.05 * rng.standard_normal(p[::13].shape)).astype(np.float32)
    return p


def ref_v_thr(x, k, alpha):
    """v [B,K], thr [B] in float64 as the reference forms them (expansion form; cdist ** 2 is checked against it)."""
    pc = torch.from_numpy(x).double()                      # [B,K,3]
    inner = -2.0 * torch.matmul(pc, pc.transpose(2, 1))
    xx = torch.sum(pc ** 2, dim=2, keepdim=True)
    dist = xx + inner + xx.transpose(2, 1)
    value = -((-dist).topk(k=k + 1, dim=-1)[0][..., 1:])
    v = value.mean(-1)
    thr = v.mean(-1) + alpha * v.std(-1)
    d2 = torch.cdist(pc, pc) ** 2
    v2 = d2.topk(k + 1, dim=-1, largest=False)[0][..., 1:].mean(-1)
    scale = thr[:, None]
    assert ((v - v2).abs() / scale).max() < 1e-12
    return v.numpy(), thr.numpy()


def direct_v_thr_f32(x, k, alpha):
    p = torch.from_numpy(x)                                # fp32
    d = ((p[:, :, None, :] - p[:, None, :, :]) ** 2).sum(-1)
    v = d.topk(k + 1, dim=-1, largest=False)[0][..., 1:].mean(-1)
    thr = v.mean(-1) + np.float32(alpha) * v.std(-1)
    return v.numpy().astype(np.float64), thr.numpy().astype(np.float64)


def sor_case(SOR, rng, x, k, alpha, npoint, name, fx):
    """x [B,K,3] fp32."""
    B, K = x.shape[:2]
    head = SOR.SORDefense(k=k, alpha=alpha, npoint=npoint)
    xt = torch.from_numpy(x).transpose(1, 2).contiguous()                 # [B,3,K]
    out = head(xt).numpy()                                                 # [B,3,npoint]
    v64, thr64 = ref_v_thr(x, k, alpha)
    v32, thr32 = direct_v_thr_f32(x, k, alpha)
    mask = v64 <= thr64[:, None]
    n = mask.sum(1)
    # deviation of the fp32 direct form (v absolute against thr where v can be 0: exact duplicates)
    dev = max(np.max(np.abs(v32 - v64) / thr64[:, None]) if name == "dup" else
              np.max(np.abs(v32 - v64) / np.maximum(v64, 1e-300)), np.max(np.abs(thr32 - thr64) / thr64))
    band = 16.0 * dev
    margin = np.min(np.abs(v64 - thr64[:, None]) / thr64[:, None])
    if not margin > band:
        raise SystemExit(f"{name}: margin {margin:.3e} is inside the band {band:.3e}: pick another seed")
    if not np.array_equal(v32 <= thr32[:, None], mask):
        raise SystemExit(f"{name}: the fp32 mask differs from the float64 mask: pick another seed")
    for b in range(B):
        kept = np.nonzero(mask[b])[0]
        assert n[b] <= npoint
        src = kept[np.arange(npoint) % n[b]]
        assert np.array_equal(out[b].T, x[b][src]), f"{name}: padding rule broken for cloud {b}"
    G = rng.uniform(0.5, 1.5, size=out.shape).astype(np.float32)          # positive: no cancellation in the sums
    x64 = xt.double().requires_grad_()
    (head(x64) * torch.from_numpy(G).double()).sum().backward()
    fx.update({f"{name}_x": xt.numpy(), f"{name}_v": v64, f"{name}_thr": thr64, f"{name}_mask": mask,
               f"{name}_n": n.astype(np.int64), f"{name}_out": out, f"{name}_G": G,
               f"{name}_grad": x64.grad.numpy().astype(np.float32),
               f"{name}_cfg": np.array([k, alpha, npoint, band], dtype=np.float64)})
    print(f"{name}: B={B} K={K} k={k} alpha={alpha} npoint={npoint} n_b={n.tolist()} dev={dev:.2e} band={band:.2e} "
          f"margin={margin:.2e}")


def main():
    SOR, SRS = load("SOR"), load("SRS")
    rng = np.random.default_rng(SEED)
    fx = {}
    names = []
    for name, (K, k, alpha, npoint) in {"k1024": (1024, 2, 1.1, 1024), "k2048": (2048, 2, 1.1, 2048),
                                        "k5": (1024, 5, 1.05, 1024), "wrap": (256, 2, 1.1, 1024)}.items():
        x = np.stack([outlier_cloud(rng, K) for _ in range(4)])
        sor_case(SOR, rng, x, k, alpha, npoint, name, fx)
        names.append(name)
    # exact duplicates: 64 points of the cloud appear twice (a duplicate is a neighbour at distance 0)
    x = outlier_cloud(rng, 1024)
    x[512:576] = x[:64]
    sor_case(SOR, rng, x[None], 2, 1.1, 1024, "dup", fx)
    names.append("dup")
    # a real scan, sub-sampled to 1024 points
    scan = np.loadtxt(os.path.join(OUT, "data", "0-88-63.txt"), dtype=np.float32)[:, :3]
    x = scan[np.sort(rng.choice(len(scan), 1024, replace=False))]
    sor_case(SOR, rng, x[None], 2, 1.1, 1024, "scan", fx)
    names.append("scan")
    fx["cases"] = np.array(names)

    # SRS: the reference under a seeded global numpy stream, and the tables the same calls draw
    xs = fx["k1024_x"]                                                     # [4,3,1024]
    B, _, K = xs.shape
    for drop in (500, 1):
        np.random.seed(SRS_SEED)
        out = SRS.SRSDefense(drop_num=drop)(torch.from_numpy(xs)).numpy()
        np.random.seed(SRS_SEED)
        idx = np.stack([np.random.choice(K, K - drop, replace=False) for _ in range(B)])
        assert np.array_equal(out, np.stack([xs[b][:, idx[b]] for b in range(B)]))
        fx[f"srs{drop}_idx"] = idx.astype(np.int32)
    fx["srs_seed"] = np.array(SRS_SEED)
    fx["srs_drops"] = np.array([500, 1])
    np.savez_compressed(os.path.join(OUT, "defense.npz"), **fx)
    print("wrote defense.npz", os.path.getsize(os.path.join(OUT, "defense.npz")), "bytes")


if __name__ == "__main__":
    main()
