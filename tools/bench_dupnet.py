"""The DUP-Net head (defense.DUPNet: SOR + the PU-Net upsampler, csrc/punet.hip) at B = 32, K = 1024: us per call of PU-Net
and DUP-Net forward and forward + backward with fixed FPS starts, replayed from hipGraphs after a warm period, beside the
plain-torch restatement of the reference's algorithm (tests/test_dupnet_cpu.RestatedPUNet, eager) on the same GPU; every
switch both ways (conv-before-interp, fused expansion tail); each new kernel alone with its bytes / FLOPs and its fraction of
the HBM or fp32-MFMA peak; the share of the sampling chain; and ms per CW iteration (autograd path) on Defended(PointNet,
DUPNet) against the undefended victim. Writes profiles/dupnet_bench.json.
Usage: python tools/bench_dupnet.py [--out FILE] [--iters N]"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_defense import cw_ms, eager_us, graph_us  # noqa: E402
from test_defense_cpu import outlier_cloud  # noqa: E402
from test_dupnet_cpu import WEIGHT_PARTS, RestatedPUNet, load_state, restated_sor  # noqa: E402

M = importlib.import_module
dev = torch.device("cuda:0")
ops = M("3dpointcloudattack_amd.ops")
dfn = M("3dpointcloudattack_amd.defense")
pum = M("3dpointcloudattack_amd.attack.SIadv.baselines.defense.DUP_Net.pu_modules")
pun = M("3dpointcloudattack_amd.attack.SIadv.baselines.defense.DUP_Net.pu_net")
seeded_state_dict = M("3dpointcloudattack_amd.seeding").seeded_state_dict
HBM_TBS, MFMA_F32_TFLOPS = 8.0, 157.3       # MI355X peaks


def fwd_and_bwd(fn, x, G):
    return (lambda: fn(x.detach())), (lambda: torch.autograd.grad((fn(x) * G).sum(), x))


def network(B, K):
    rng = np.random.default_rng(K)
    x_cf = torch.from_numpy(np.stack([outlier_cloud(rng, K) for _ in range(B)])).to(dev).transpose(1, 2).contiguous().requires_grad_()
    x_cl = x_cf.detach().transpose(1, 2).contiguous().requires_grad_()
    G = torch.rand((B, 4 * K, 3), device=dev) + 0.5
    row = dict(B=B, K=K, up_ratio=4, fps_start=0)
    head = dfn.DUPNet(weights=WEIGHT_PARTS, fps_start=0).to(dev)
    net = head.pu_net

    def measure(tag):
        f, fb = fwd_and_bwd(net, x_cl, G)
        row[f"punet_{tag}fwd_us"] = round(graph_us(f, reps=2, rounds=10), 1)
        row[f"punet_{tag}fwd_bwd_us"] = round(graph_us(fb, reps=2, rounds=10), 1)

    measure("")
    for mod, flag, tag in ((pum, "CONV_BEFORE_INTERP", "interp_before_conv_"), (pun, "EXPAND_FUSED", "layerwise_tail_")):
        old = getattr(mod, flag)
        setattr(mod, flag, not old)
        try:
            measure(tag)
        finally:
            setattr(mod, flag, old)
    f, fb = fwd_and_bwd(lambda t: head(t).transpose(1, 2), x_cf, G)
    row["dupnet_fwd_us"] = round(graph_us(f, reps=2, rounds=10), 1)
    row["dupnet_fwd_bwd_us"] = round(graph_us(fb, reps=2, rounds=10), 1)
    f, fb = fwd_and_bwd(net, x_cl, G)
    row["punet_fwd_eager_us"] = round(eager_us(f, reps=10), 1)
    row["punet_fwd_bwd_eager_us"] = round(eager_us(fb, reps=10), 1)

    # the sampling chain alone: 1024 -> 1024 -> 512 -> 256 -> 128, four dependent launches
    st = torch.zeros((B,), dtype=torch.int32, device=dev)

    def chain():
        p = x_cl.detach()
        for s in (K, K // 2, K // 4, K // 8):
            idx = ops.fps(p, s, st)
            p = ops.group_gather(p, None, idx.view(B, s, 1)).view(B, s, 3)
    row["fps_chain_us"] = round(graph_us(chain, reps=2, rounds=10), 1)
    row["fps_chain_share_of_fwd"] = round(row["fps_chain_us"] / row["punet_fwd_us"], 3)

    rest = RestatedPUNet(load_state(), device=dev)
    starts = torch.zeros((4, B), dtype=torch.int32)
    f, fb = fwd_and_bwd(lambda t: rest.forward(t, starts)[0], x_cl, G)
    row["punet_torch_fwd_us"] = round(eager_us(f, reps=2), 1)
    row["punet_torch_fwd_bwd_us"] = round(eager_us(fb, reps=2), 1)
    f, fb = fwd_and_bwd(lambda t: rest.forward(restated_sor(t).transpose(1, 2), starts)[0], x_cf, G)
    row["dupnet_torch_fwd_us"] = round(eager_us(f, reps=2), 1)
    row["dupnet_torch_fwd_bwd_us"] = round(eager_us(fb, reps=2), 1)
    for k in ("punet", "dupnet"):
        row[f"{k}_fwd_speedup_vs_torch"] = round(row[f"{k}_torch_fwd_us"] / row[f"{k}_fwd_us"], 1)
        row[f"{k}_fwd_bwd_speedup_vs_torch"] = round(row[f"{k}_torch_fwd_bwd_us"] / row[f"{k}_fwd_bwd_us"], 1)
    return row


def kernels(B, N):
    """Each new launch alone at PU-Net's shapes."""
    out = []
    u = torch.rand((B, N, 3), device=dev) * 2 - 1
    for Mk in (512, 256, 128):
        k = u[:, :Mk].contiguous() + 0.01
        F = torch.randn((B, Mk, 64), device=dev)
        bias = torch.randn((64,), device=dev)
        d, idx = ops.knn_raw(u, k, 3)
        buf = torch.empty((B, N, 260), device=dev)
        us = graph_us(lambda: ops.three_interp_raw(d, idx, F, buf, 67, 64, bias, True))
        nbytes = B * N * (24 + 64 * 4) + B * Mk * 64 * 4
        out.append(dict(kernel="three_interp_f32", M=Mk, C=64, us=round(us, 1), bytes=nbytes,
                        hbm_fraction=round(nbytes / (us * 1e-6) / (HBM_TBS * 1e12), 3)))
        Fg, ug, kg = F.clone().requires_grad_(), u.clone().requires_grad_(), k.clone().requires_grad_()
        G = torch.rand((B, N, 64), device=dev)

        def fb():
            y = ops.three_interp(ug, kg, Fg, bias=bias, relu=True)
            torch.autograd.grad((y * G).sum(), (ug, kg, Fg))
        out.append(dict(kernel="search + three_interp forward + backward (autograd)", M=Mk, C=64, us=round(graph_us(fb), 1)))
    r = 4
    h = torch.randn((r * B * N, 128), device=dev)
    w3, b3 = torch.randn((64, 128), device=dev) / 8, torch.randn((64,), device=dev)
    w4, b4 = torch.randn((3, 64), device=dev) / 4, torch.randn((3,), device=dev)
    o, mask = ops.pcd_tail_raw(h, w3, b3, w4, b4, B, N, r)
    g = torch.rand_like(o)
    rows = r * B * N
    for name, fn, flop, nbytes in (("pcd_tail_f32", lambda: ops.pcd_tail_raw(h, w3, b3, w4, b4, B, N, r), 2 * rows * (128 * 64 + 64 * 3),
                                    rows * (128 * 4 + 8 + 12)),
                                   ("pcd_tail_bwd_f32", lambda: ops.pcd_tail_bwd_raw(g, mask, w3, w4, B, N, r),
                                    2 * rows * (128 * 64 + 64 * 3), rows * (128 * 4 + 8 + 12))):
        us = graph_us(fn)
        out.append(dict(kernel=name, rows=rows, us=round(us, 1), flop=flop, bytes=nbytes,
                        mfma_fraction=round(flop / (us * 1e-6) / (MFMA_F32_TFLOPS * 1e12), 3),
                        hbm_fraction=round(nbytes / (us * 1e-6) / (HBM_TBS * 1e12), 3)))
    # the same head as two GEMM launches (what the fused launch replaces)
    us = graph_us(lambda: ops.gemm_nt(ops.gemm_nt(h, w3, b3, "relu", unit_rows=N), w4, b4, unit_rows=N))
    out.append(dict(kernel="the head as two pc3d_gemm_nt_f32 launches", rows=rows, us=round(us, 1)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dupnet_bench.json"))
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    B, K = 32, 1024
    res = dict(device=torch.cuda.get_device_name(0), network=network(B, K), kernels=kernels(B, K))

    def victim(seed):
        m = M("3dpointcloudattack_amd.model.pointnet").PointNetCls(k=40)
        m.load_state_dict(seeded_state_dict(m, seed))
        return m.to(dev).eval()

    rng = np.random.default_rng(0)
    pcs = torch.from_numpy(np.stack([outlier_cloud(rng, K) for _ in range(B)]))
    model, trans = victim(0), victim(1)
    with torch.no_grad():
        labels = model(pcs.transpose(1, 2).contiguous().to(dev))[0].argmax(1).cpu()
    cw = dict(B=B, K=K, path="autograd (fused=False)")
    cw["undefended_ms"] = round(cw_ms(model, trans, pcs, labels, a.iters), 4)
    head = dfn.DUPNet(weights=WEIGHT_PARTS, fps_start=0).to(dev)
    cw["defended_dupnet_ms"] = round(cw_ms(dfn.Defended(model, head), trans, pcs, labels, a.iters), 4)
    cw["head_cost_ms"] = round(cw["defended_dupnet_ms"] - cw["undefended_ms"], 4)
    res["cw_pointnet"] = cw
    print(json.dumps(res))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
