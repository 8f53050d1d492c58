"""Stand-alone timing of the fused PointNet tower (K8): forward and backward eagerly (event-timed), and the backward's
kernels by name inside replayed hipGraphs, the way the attack loops launch them: the two forms of the balanced kernel
(tile32: a workgroup per 32 points; packed: a workgroup per 128 points, the W2 product over live rows only) timed
ALTERNATELY, the least of ROUNDS rounds with the round-to-round spread; the packed form ended after each phase (B = 32
shapes); and the two-list kernel both replaced. One JSON line per shape; --json PATH also writes the list."""
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
ap.add_argument("--rounds", type=int, default=5)
args = ap.parse_args()
rows = []
torch.manual_seed(0)
PHASES = ("compaction", "sort", "gather", "w2_product", "w1_product")   # stop_after = 1..5
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
    live = torch.zeros(B, N, dtype=torch.bool, device=dev).scatter_(1, i.long(), True)
    row["live_points_per_cloud"] = float(live.sum(1).float().mean())
    row["row_blocks_per_128_points"] = float(((live.view(B, -1, 128).sum(2) + 31) // 32).float().mean())
    # the trunk's launch (T -> dx, per-tile dT) and the STN tower's (accumulating into the same gx)
    launches = {"trunk": dict(T=T, want_gT=True), "stn": dict(accumulate=True)}
    for tower, kw in launches.items():
        row["graph_bwd_%s_us_twolist" % tower] = graph_us(lambda: ops.pointmlp3_max_bwd_raw(x, ws, i, g, mk, out=out, twolist=True, **kw))
        t = {"tile32": [], "packed": []}
        for _ in range(args.rounds):   # alternated: a drift of the clocks meets both forms
            for name in t:
                t[name].append(graph_us(lambda: ops.pointmlp3_max_bwd_raw(x, ws, i, g, mk, out=out, tile32=(name == "tile32"), **kw)))
        for name, v in t.items():
            row["graph_bwd_%s_us_%s" % (tower, name)] = min(v)
            row["graph_bwd_%s_us_%s_spread" % (tower, name)] = max(v) - min(v)
        if B == 32:   # the packed launch ended after each phase (loads nothing later needs are dropped with it)
            for k, ph in enumerate(PHASES, 1):
                row["graph_bwd_%s_us_packed_upto_%s" % (tower, ph)] = min(
                    graph_us(lambda: ops.pointmlp3_max_bwd_raw(x, ws, i, g, mk, out=out, tile32=False, stop_after=k, **kw)) for _ in range(3))
    rows.append(row)
    print(json.dumps(row))
if args.json:
    with open(args.json, "w") as fh: json.dump(rows, fh, indent=1)
