"""Stand-alone timing of the PointNet tower forward with layer 3 screened on bf16 MFMA (the default launch) against
the exact fp32 kernel (exact=True): both inside replayed hipGraphs, alternated, at B = 32 and N = 1024 / 2048 / 4096,
for both towers of bench.py's victim (seeded weights 0) on bench.py's kind of cloud. Also the screened launch cut
short after each phase (prologue + norms, + screen, + selection; the debug instantiation) and the `stats` of the
full launch: candidates rechecked per (tile, channel), channel blocks that fell back to the exact block.
One JSON line per (tower, N); --json PATH also writes the list."""
import argparse, importlib, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
ops = importlib.import_module("3dpointcloudattack_amd.ops")
pn = importlib.import_module("3dpointcloudattack_amd.model.pointnet")
seeding = importlib.import_module("3dpointcloudattack_amd.seeding")
dev = torch.device("cuda:0")


def unit_cloud(rng, n):      # bench.py's
    g = rng.standard_normal((n, 3))
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    p = g * rng.random((n, 1)) ** (1.0 / 3.0)
    p = p - p.mean(axis=0, keepdims=True)
    return (p / np.max(np.linalg.norm(p, axis=1))).astype(np.float32)


def graph_us(fns, per=20, reps=30, rounds=3):
    """us per call of each fn: `per` calls captured into one graph each, the graphs replayed alternately."""
    side = torch.cuda.Stream()
    graphs = []
    with torch.cuda.stream(side):
        for fn in fns:
            fn()
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                for _ in range(per):
                    fn()
            graphs.append(g)
        best = [float("inf")] * len(fns)
        for g in graphs:
            for _ in range(5):
                g.replay()
        for _ in range(rounds):
            for i, g in enumerate(graphs):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(side)
                for _ in range(reps):
                    g.replay()
                e1.record(side)
                e1.synchronize()
                best[i] = min(best[i], e0.elapsed_time(e1) / (per * reps) * 1e3)
    return best


ap = argparse.ArgumentParser()
ap.add_argument("--json", default=None)
ap.add_argument("--sizes", default="1024,2048,4096")
args = ap.parse_args()
model = pn.PointNetCls(k=40, feature_transform=False)
model.load_state_dict(seeding.seeded_state_dict(model, 0))
model = model.to(dev).eval()
pk = pn.fused_pack(model)
B = 32
rows = []
for N in [int(s) for s in args.sizes.split(",")]:
    rng = np.random.default_rng(1234 + 1)
    x = torch.from_numpy(np.stack([unit_cloud(rng, N) for _ in range(B)])).transpose(1, 2).contiguous().to(dev)
    x = x + 0.01 * torch.randn(x.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(N))
    for tower, relu_last in (("tower_s", True), ("tower_c", False)):
        w = pk[tower]
        kw = {}
        if tower == "tower_c":     # the trunk runs behind the STN's transform
            kw["T"] = (torch.eye(3, device=dev)[None] + 0.05 * torch.randn(B, 3, 3, device=dev)).contiguous()
        ex = ops.pointmlp3_max_fwd_raw(x, w, relu_last, want_masks=True, exact=True, **kw)
        sc = ops.pointmlp3_max_fwd_raw(x, w, relu_last, want_masks=True, **kw)
        same = all(torch.equal(a, b) for a, b in zip((ex[0], ex[1]) + ex[2], (sc[0], sc[1]) + sc[2]))
        dbg = {}
        ops.pointmlp3_max_fwd_raw(x, w, relu_last, fold=False, screen_dbg=dbg, **kw)
        st = dbg["stats"].double()
        ntiles = st.shape[1]
        fns = [lambda: ops.pointmlp3_max_fwd_raw(x, w, relu_last, fold=False, exact=True, **kw),
               lambda: ops.pointmlp3_max_fwd_raw(x, w, relu_last, fold=False, **kw)]
        for stop in (1, 2, 3, 0):
            fns.append(lambda stop=stop: ops.pointmlp3_max_fwd_raw(x, w, relu_last, fold=False,
                                                                   screen_dbg={"stop_after": stop}, **kw))
        t = graph_us(fns)
        row = {"tower": tower, "B": B, "N": N, "bit_equal": bool(same), "exact_us": t[0], "screened_us": t[1],
               "dbg_prologue_us": t[2], "dbg_screen_us": t[3], "dbg_select_us": t[4], "dbg_all_us": t[5],
               "candidates_per_tile_channel": float(st[..., 0].sum() / (B * ntiles * w[4].shape[0])),
               "candidates_per_tile_max": float(st[..., 0].max()),
               "fallback_blocks": int(st[..., 1].sum()), "blocks": int(B * ntiles * w[4].shape[0] // 32)}
        rows.append(row)
        print(json.dumps(row), flush=True)
if args.json:
    with open(args.json, "w") as fh:
        json.dump(rows, fh, indent=1)
