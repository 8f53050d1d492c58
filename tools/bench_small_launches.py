"""Stand-alone timing of the CW step's small launches whose global loads are issued together at entry (the tower's fold
and the classifier tail), each in BOTH forms: the
one the step runs and the earlier one kept behind serial=True. Every call is timed inside replayed hipGraphs, the way
the attack loop launches it, at the step's shapes (PointNet, B = 32, N = 1024; --n 2048 / 4096 for the sweep's folds).
One JSON line per kernel; --json PATH also writes the list."""
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
args = ap.parse_args()
B, N = args.b, args.n
torch.manual_seed(0)
R = lambda *s: torch.randn(*s, device=dev)
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
