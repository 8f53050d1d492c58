"""Stand-alone timing of the fused PointNet tower (K8): forward and backward eagerly (event-timed), and BOTH backward
entries (the balanced kernel behind pc3d_pointmlp3_max_bwd_f32 and the two-list kernel it replaced) inside replayed
hipGraphs, the way the attack loops launch them. One JSON line per shape; --json PATH also writes the list."""
import argparse, importlib, sys, os, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
ops = importlib.import_module("3dpointcloudattack_amd.ops")
dev = torch.device("cuda:0")
def w(C3):
    return tuple(t.to(dev) for t in (torch.randn(64,3), torch.randn(64), torch.randn(128,64)/8, torch.randn(128), torch.randn(C3,128)/11, torch.randn(C3)))
def graph_us(fn, per=20, reps=50):
    """us per call: `per` calls captured into one graph, replayed `reps` times after a warm replay (as bench.py::graph_ms)"""
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        fn()
        side.synchronize()
        with torch.cuda.graph(g, stream=side):
            for _ in range(per): fn()
        for _ in range(5): g.replay()
        side.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(side)
        for _ in range(reps): g.replay()
        e1.record(side)
        e1.synchronize()
    return e0.elapsed_time(e1) / (per * reps) * 1e3
ap = argparse.ArgumentParser()
ap.add_argument("--json", default=None)
args = ap.parse_args()
rows = []
torch.manual_seed(0)
for B, N in ((32, 1024), (32, 2048), (64, 2048), (32, 4096)):
    x = torch.randn(B, 3, N, device=dev); ws = w(1024); ws = ws + (ws[2].t().contiguous(),)
    T = torch.randn(B, 3, 3, device=dev) * 0.5
    for _ in range(3): p, i, mk = ops.pointmlp3_max_fwd_raw(x, ws, False, want_masks=True)
    g = torch.randn_like(p)
    for _ in range(3): ops.pointmlp3_max_bwd_raw(x, ws, i, g, mk)
    torch.cuda.synchronize()
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    it = 20
    e[0].record()
    for _ in range(it): ops.pointmlp3_max_fwd_raw(x, ws, False)
    e[1].record()
    for _ in range(it): ops.pointmlp3_max_bwd_raw(x, ws, i, g, mk)
    e[2].record(); torch.cuda.synchronize()
    f = e[0].elapsed_time(e[1]) / it; bw = e[1].elapsed_time(e[2]) / it
    flop = 2.0 * B * N * (3*64 + 64*128 + 128*1024)
    row = {"B": B, "N": N, "fwd_us": f*1e3, "fwd_TFLOPs": flop / f / 1e9, "bwd_us": bw*1e3}
    out = torch.zeros_like(x)
    hist = torch.bincount((i.long() // 32).flatten() + (N // 32) * torch.arange(B, device=dev).repeat_interleave(1024))
    row["busiest_tile_hits"] = int(hist.max())
    for name, twolist in (("balanced", False), ("twolist", True)):
        # the trunk's launch (T -> dx, per-tile dT) and the STN tower's (accumulating into the same gx)
        row["graph_bwd_trunk_us_" + name] = graph_us(lambda: ops.pointmlp3_max_bwd_raw(x, ws, i, g, mk, T=T, want_gT=True, out=out, twolist=twolist))
        row["graph_bwd_stn_us_" + name] = graph_us(lambda: ops.pointmlp3_max_bwd_raw(x, ws, i, g, mk, out=out, accumulate=True, twolist=twolist))
    rows.append(row)
    print(json.dumps(row))
if args.json:
    with open(args.json, "w") as fh: json.dump(rows, fh, indent=1)
