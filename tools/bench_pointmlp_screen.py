"""Stand-alone timing of the PointNet tower forward with layer 3 screened on the matrix pipe against the exact fp32 kernel
(exact=True), in the screened forms: `in_launch` makes its bf16 operands and norms from W3 inside every launch,
`prepared` reads them from the image made once per fold (three bf16 products per k-step), `fp16` reads the scaled fp16
image in the same allocation (one product per k-step, sixteen candidate slots per channel) and rechecks by channel,
`fp16_pair` is that form with the recheck by (channel, candidate) pair: its recheck + stores is
fp16_pair_dbg_all_us - fp16_pair_dbg_select_us (the debug instantiation's columns), as for `fp16`. All inside replayed
hipGraphs, alternated, at B = 32 and N = 1024 / 2048 / 4096, for both towers of bench.py's victim (seeded weights 0) on
bench.py's kind of cloud. Also the screened launches cut short after each phase (prologue + norms, + screen,
+ selection; the debug instantiations) and the `stats` of the full launches: candidates rechecked per (tile, channel),
channel blocks that fell back to the exact block. Every time is the least of the rounds; *_spread_us is the largest
minus the least round of that graph. One JSON line per (tower, N); --json PATH also writes the list."""
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


def graph_us(fns, per=20, reps=30, rounds=5):
    """(least, largest) us per call of each fn over the rounds: `per` calls captured into one graph each, the graphs
    replayed alternately."""
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
        best, worst = [float("inf")] * len(fns), [0.0] * len(fns)
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
                us = e0.elapsed_time(e1) / (per * reps) * 1e3
                best[i], worst[i] = min(best[i], us), max(worst[i], us)
    return best, worst


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
        assert len(w) > 7 and isinstance(w[7], list)     # the folded tower carries the image's holder
        ex = ops.pointmlp3_max_fwd_raw(x, w, relu_last, want_masks=True, exact=True, **kw)
        same = {}
        row = {"tower": tower, "B": B, "N": N}
        C3 = w[4].shape[0]
        fns = [lambda: ops.pointmlp3_max_fwd_raw(x, w, relu_last, fold=False, exact=True, **kw)]
        names = ["exact"]
        for form, sel in (("in_launch", dict(in_launch=True)), ("prepared", dict(form="bf16")),
                          ("fp16", dict(form="fp16", recheck="channel")), ("fp16_pair", dict(form="fp16", recheck="pair"))):
            sc = ops.pointmlp3_max_fwd_raw(x, w, relu_last, want_masks=True, **sel, **kw)
            row["bit_equal_" + form] = bool(all(torch.equal(a, b) for a, b in zip((ex[0], ex[1]) + ex[2], (sc[0], sc[1]) + sc[2])))
            dbg = {}
            ops.pointmlp3_max_fwd_raw(x, w, relu_last, fold=False, screen_dbg=dbg, **sel, **kw)
            st = dbg["stats"].double()
            ntiles = st.shape[1]
            row[form + "_candidates_per_tile_channel"] = float(st[..., 0].sum() / (B * ntiles * C3))
            row[form + "_fallback_blocks"] = int(st[..., 1].sum())
            fns.append(lambda sel=sel: ops.pointmlp3_max_fwd_raw(x, w, relu_last, fold=False, **sel, **kw))
            names.append(form)
            for stop, cut in ((1, "prologue"), (2, "screen"), (3, "select"), (0, "all")):
                fns.append(lambda stop=stop, sel=sel: ops.pointmlp3_max_fwd_raw(x, w, relu_last, fold=False,
                                                                                screen_dbg={"stop_after": stop}, **sel, **kw))
                names.append(form + "_dbg_" + cut)
        assert len(w[7]) == 4 and ops._pm_w3_h(w[7][0]) is not None   # the prepared and fp16 rows did run from the images
        row["blocks"] = int(B * ntiles * C3 // 32)
        best, worst = graph_us(fns)
        for name, lo, hi in zip(names, best, worst):
            row[name + "_us"], row[name + "_spread_us"] = lo, hi - lo
        rows.append(row)
        print(json.dumps(row), flush=True)
if args.json:
    with open(args.json, "w") as fh:
        json.dump(rows, fh, indent=1)
