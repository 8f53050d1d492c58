"""Stand-alone timing of the CW step's small launches whose global loads are issued together at entry (the tower's fold
and the classifier tail), each in BOTH forms: the
one the step runs and the earlier one kept behind serial=True. Every call is timed inside replayed hipGraphs, the way
the attack loop launches it, at the step's shapes (PointNet, B = 32, N = 1024; --n 2048 / 4096 for the sweep's folds).
One JSON line per kernel; --json PATH also writes the list.

--tiles times instead the step's eight launches built on the small-batch linear kernel (five plain layers, the layer +
search, the layer + bookkeeping, the pre-layer) in every tile form (ops.LINEAR_TILES), the forms alternated inside each
round, next to the prediction of the fit 2.3 us + 0.0305 us per KB a workgroup pulls (profiles/
r07_small_launch_loads_bench.json). A form is `eligible` for the rule only if it beats 32x16 by more than 2 % and by
more than the larger min-max spread of the two cells."""
import argparse, importlib, sys, os, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
ops = importlib.import_module("3dpointcloudattack_amd.ops")
dev = torch.device("cuda:0")
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
ap.add_argument("--b", type=int, default=32)
ap.add_argument("--n", type=int, default=1024)
ap.add_argument("--rounds", type=int, default=5, help="alternated (serial, entry) pairs per kernel; the median is reported")
ap.add_argument("--tiles", action="store_true", help="time the eight linear launches of the step in every tile form instead")
args = ap.parse_args()
B, N = args.b, args.n
torch.manual_seed(0)
R = lambda *s: torch.randn(*s, device=dev)


def tile_cases():
    """name -> (K, O, fn(tile)) for the eight launches of one CW step on PointNet (model/pointnet.py: cw_step)"""
    ori = torch.rand(B, 3, N, device=dev) - 0.5
    adv = ori + 0.01 * R(B, 3, N)
    lay = lambda K, O: (R(B, K), R(O, K) / K ** 0.5, R(O), R(B, O))     # X, W, bias, gate
    label = torch.randint(0, 40, (B,), device=dev)
    pred = (label + 1) % 40
    f = lambda v: torch.full((B,), v, device=dev)
    book = (pred, label, True, f(1e10), torch.full((B,), -1, device=dev), f(1e10), torch.full((B,), -1, device=dev),
            torch.zeros_like(adv))
    input_val, dist_val = torch.zeros_like(adv), torch.zeros(B, device=dev)
    step, adam = torch.ones(1, dtype=torch.int32, device=dev), torch.zeros(2, device=dev)
    P = (N + ops._lib.load().pc3d_pointmlp3_bwd_tile_points() - 1) // ops._lib.load().pc3d_pointmlp3_bwd_tile_points()
    parts, Wp, a2 = R(B, P, 16), R(9, 256), R(B, 256)
    s1, s2, c1, c2, cb2, cb1, sb2, sb1 = lay(1024, 512), lay(512, 256), lay(1024, 512), lay(512, 256), lay(256, 512), \
        lay(512, 1024), lay(256, 512), lay(512, 1024)
    return {
        "stn fc1 1024->512 + search (linear_nn)": (1024, 512, lambda t: ops.linear_nn(s1[0], s1[1], s1[2], relu=True, q=adv, r=ori,
                                                                                      q_cf=True, r_cf=True, tile=t)),
        "stn fc2 512->256": (512, 256, lambda t: ops.linear(s2[0], s2[1], s2[2], relu=True, tile=t)),
        "cls fc1 1024->512": (1024, 512, lambda t: ops.linear(c1[0], c1[1], c1[2], relu=True, tile=t)),
        "cls fc2 512->256": (512, 256, lambda t: ops.linear(c2[0], c2[1], c2[2], relu=True, tile=t)),
        "cls fc2 bwd 256->512 + bookkeeping (linear_book)": (256, 512, lambda t: ops.linear_book(
            cb2[0], cb2[1], adv, ori, *book, gate=cb2[3], input_val=input_val, dist_val=dist_val, step=step, lr=0.01, adam=adam,
            tile=t)),
        "cls fc1 bwd 512->1024": (512, 1024, lambda t: ops.linear(cb1[0], cb1[1], tile=t)),
        f"stn fc3+fc2 bwd 256->512 (linear_pre, P={P})": (256, 512, lambda t: ops.linear_pre(parts, 9, Wp, a2, sb2[1], gate=sb2[3],
                                                                                            tile=t)),
        "stn fc1 bwd 512->1024": (512, 1024, lambda t: ops.linear(sb1[0], sb1[1], gate=sb1[3], tile=t)),
    }


if args.tiles:
    forms = list(ops.LINEAR_TILES)
    rows = []
    for name, (K, O, fn) in tile_cases().items():
        t = {f: [] for f in forms}
        for _ in range(args.rounds):
            for f in forms:
                t[f].append(graph_us(lambda: fn(f)))
        row = {"launch": name, "B": B, "N": N, "K": K, "O": O, "forms": {},
               "rule": "32x16 (this entry takes no rule: its tile 0)" if "linear_book" in name else ops.linear_tile(B, K, O)}
        base = sorted(t["32x16"])[len(t["32x16"]) // 2]
        base_spread = max(t["32x16"]) - min(t["32x16"])
        for f in forms:
            tr, tc = (int(v) for v in f.split("x"))
            med, spread = sorted(t[f])[len(t[f]) // 2], max(t[f]) - min(t[f])
            kb = 4 * K * (tr + tc) / 1024
            row["forms"][f] = {"us": med, "us_min_max": [min(t[f]), max(t[f])], "layer_workgroups": -(-O // tc) * -(-B // tr),
                               "kb_per_workgroup": kb, "fit_us_plain_layer": 2.3 + 0.0305 * kb,
                               "eligible": f != "32x16" and base - med > max(0.02 * base, spread, base_spread)}
        rows.append(row)
        print(json.dumps(row))
    if args.json:
        with open(args.json, "w") as fh: json.dump(rows, fh, indent=1)
    sys.exit(0)
cases = []
# the fold of a tower forward: ceil(N / tile) tiles of 1024 channels
nt = (N + ops._pm_tile() - 1) // ops._pm_tile()
pv, pi = R(B, nt, 1024), torch.randint(0, N, (B, nt, 1024), device=dev, dtype=torch.int32)
cases.append((f"fold ntiles={nt}", lambda s: ops.pointmlp3_fold_raw(pv, pi, True, serial=s)))
c2, w3, b3, tgt = R(B, 256).clamp(min=0), R(40, 256) / 16, R(40), torch.randint(0, 40, (B,), device=dev)
step = torch.zeros(1, dtype=torch.int32, device=dev)
cases.append(("cls_tail", lambda s: ops.cls_tail(c2, w3, b3, tgt, 0, scale=1.0 / B, step=step, want_logp=False, serial=s)))
rows = []
for name, fn in cases:
    t = {True: [], False: []}
    for _ in range(args.rounds):
        for s in (True, False):
            t[s].append(graph_us(lambda: fn(s)))
    med = {s: sorted(v)[len(v) // 2] for s, v in t.items()}
    row = {"kernel": name, "B": B, "N": N, "serial_us": med[True], "entry_us": med[False],
           "serial_us_min_max": [min(t[True]), max(t[True])], "entry_us_min_max": [min(t[False]), max(t[False])]}
    rows.append(row)
    print(json.dumps(row))
if args.json:
    with open(args.json, "w") as fh: json.dump(rows, fh, indent=1)
