"""GPU: every tile variant of the point-wise GEMM (csrc/gemm.hip, gemm_nt_kernel) and its generated-operand / epilogue
forms, straight through the C ABI so that each test picks its variant itself.

The main instrument is INTEGER-EXACT data: integer-valued operands small enough that every product and every partial
sum, in whatever order a variant takes them, is an integer (or a fixed binary fraction of one) below 2^24. fp32
arithmetic is then exact, the result does not depend on the summation order, and the kernel must EQUAL a float64
reference — zero tolerance, so a dropped, doubled or misplaced term of any size fails. The bound is asserted on
sum_k |x||w| + |bias| + |residual| (which dominates every partial sum in any order), not only on the final value.

1. test_exact_every_variant     all variants x K classes x M / N edges around the variant's own tile, all epilogues
2. test_nan_moat                the same data as views into NaN / sentinel-filled buffers: reads and writes stay inside
3. test_one_summation_order     random data: the non-split variants agree bit for bit; every variant repeats itself
4. test_batch_invariance        ops.linear_act / linear_res_act / gemm_nt(unit_rows=): a cloud alone == in a batch
5. test_gather_exact / test_poolbwd_exact / test_groupmax_exact     the generated A operands, the group-max epilogue
6. test_refusals                what the entry points must turn down before any launch
"""
import importlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
_lib = importlib.import_module("3dpointcloudattack_amd._lib")

VARIANTS = [-1, 0, 1, 2, 3, 4, 5, 6, 8, 11, 12]
NONSPLIT = [-1, 0, 1, 2, 3, 4, 5, 6, 8]
TILE = {-1: (128, 128), 0: (128, 128), 1: (128, 128), 5: (128, 128), 6: (128, 128), 8: (128, 128), 2: (128, 64),
        3: (256, 64), 4: (64, 128), 11: (64, 64), 12: (32, 64)}           # (bm, bn)
ACTS = {None: 0, "relu": 1, "leaky": 2}
GATE_SLOPE, SLOPE = 0.5, 0.25      # powers of two: scaling by them is exact
LIMIT = float(2 ** 24)

# K classes. 36 and 132 are added to the issue's list so that "K % 4 == 0 but a partial group of 8" is more than K = 4.
K_CLASSES = {
    "tail4": [1, 3, 5, 31, 63, 127, 131, 255, 259],   # K % 4 != 0: gm_load4's scalar tail, rows off 16-byte alignment
    "group8": [4, 36, 132],                           # whole float4s, a partial MFMA group of 8
    "past": [33, 65, 129],                            # one k past a main-loop pass of 32 / 64 / 128: idle K groups
    "exact": [8, 32, 64, 96, 128, 256, 512],          # whole groups / whole passes
}
K_ALL = sorted(k for ks in K_CLASSES.values() for k in ks)
K_ISSUE = [1, 3, 4, 5, 8, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 131, 255, 256, 259, 512]
WIDE_K = [k for k in K_ALL if k <= 8]                 # the rows that additionally run operands of 11 bits and more
MAX_M, MAX_N, MAX_K = 2 * 256 + 3, 128 + 33, 512
SENTINEL = 0x7FC12345                                 # a NaN with a payload: the untouched part of an output buffer


def _odd(gen, shape, amax):
    """Odd integers in [-amax', amax'] as float32, amax' the largest odd number <= amax."""
    h = (int(amax) + 1) // 2
    return (torch.randint(-h, h, shape, generator=gen) * 2 + 1).float()


def _wide_wmax(K):
    # x up to 4095 (12 bits: a 10-bit-mantissa multiply cannot hold it), halves through the gate:
    # 2 * (4095 * wmax * K + 2000) < 2^24
    return min(2047, (2 ** 23 - 2000) // (4095 * K))


@pytest.fixture(scope="module")
def pools(dev):
    """Integer-valued data, generated once: every case takes a window of these (never written to)."""
    g = torch.Generator().manual_seed(20240607)
    p = {
        "x": _odd(g, (MAX_M + 64, MAX_K + 16), 63), "w": _odd(g, (MAX_N + 64, MAX_K + 16), 63),
        "b": torch.randint(-1000, 1001, (MAX_N + 64,), generator=g).float(),
        "r": torch.randint(-1000, 1001, (MAX_M + 64, MAX_N + 64), generator=g).float(),
        "gate": torch.randint(-2, 3, (MAX_M + 64, MAX_K + 16), generator=g).float(),     # zeros included: gate > 0 is strict
        "xw": _odd(g, (MAX_M + 64, 8 + 16), 4095),
    }
    for K in WIDE_K:
        p["ww", K] = _odd(g, (MAX_N + 64, K), _wide_wmax(K))
    return {k: v.to(dev) for k, v in p.items()}


def _window(pools, i, M, N, K, wide=False):
    """Contiguous copies of the i-th window of the pools: x [M,K], w [N,K], b [N], r [M,N], gate [M,K]."""
    om, on, ok = (7 * i) % 64, (11 * i) % 64, (5 * i) % 16
    x = (pools["xw"] if wide else pools["x"])[om:om + M, ok:ok + K].contiguous()
    w = pools["ww", K][on:on + N].contiguous() if wide else pools["w"][on:on + N, ok:ok + K].contiguous()
    return (x, w, pools["b"][on:on + N].contiguous(), pools["r"][om:om + M, on:on + N].contiguous(),
            pools["gate"][om:om + M, ok:ok + K].contiguous())


def _p(t):
    return 0 if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _launch(variant, x, w, b, gate, r, act, y, gslope=GATE_SLOPE, slope=SLOPE):
    """One launch through the C ABI: the residual entry point when r is given, else the default / the tiled one."""
    M, K = x.shape
    N = w.shape[0]
    if r is not None:
        assert gate is None
        _lib.call("pc3d_gemm_nt_res_f32", x.data_ptr(), x.stride(0), w.data_ptr(), _p(b), r.data_ptr(), r.stride(0), M, N, K,
                  ACTS[act], slope, y.data_ptr(), y.stride(0), variant, _stream())
    elif variant < 0:
        _lib.call("pc3d_gemm_nt_f32", x.data_ptr(), x.stride(0), w.data_ptr(), _p(b), _p(gate),
                  gate.stride(0) if gate is not None else 0, gslope, M, N, K, ACTS[act], slope, y.data_ptr(), y.stride(0),
                  _stream())
    else:
        _lib.call("pc3d_gemm_nt_tiled_f32", x.data_ptr(), x.stride(0), w.data_ptr(), _p(b), _p(gate),
                  gate.stride(0) if gate is not None else 0, gslope, M, N, K, ACTS[act], slope, y.data_ptr(), y.stride(0),
                  variant, _stream())


def _act(y, act, slope):
    if act == "relu":
        return torch.relu(y)
    if act == "leaky":
        return F.leaky_relu(y, slope)
    return y


def _pre(x, w, b, gate=None, gslope=0.0, r=None):
    """float64 pre-activation: gate(x) @ w^T + b + r."""
    xd = x.double()
    if gate is not None:
        xd = torch.where(gate > 0, xd, gslope * xd)
    y = xd @ w.double().t()
    if b is not None:
        y = y + b.double()
    if r is not None:
        y = y + r.double()
    return y


def _ref(x, w, b, act, slope, gate=None, gslope=0.0, r=None):
    return _act(_pre(x, w, b, gate, gslope, r), act, slope)


def _assert_exact_regime(x, w, b, r, unit):
    """Every partial sum of the pre-activation, in any order, is at most sum_k |x||w| + |b| + |r|; in units of
    1 / unit (the gate halves x) that must stay below 2^24 for fp32 to be exact."""
    bound = x.abs().double() @ w.abs().double().t()
    if b is not None:
        bound = bound + b.abs().double()
    if r is not None:
        bound = bound + r.abs().double()
    assert float(bound.max()) * unit < LIMIT, "test data left the integer-exact regime"
    return bound


def _shape_cases(variant):
    """(K class, K, M edge index, N edge index, M, N): every (K class, M edge, N edge) once, the K of a class cycling."""
    bm, bn = TILE[variant]
    Ms = [1, bm - 1, bm, bm + 1, 2 * bm + 3]
    Ns = [1, bn - 1, bn, bn + 1, bn + 33]
    out = []
    for ci, (cls, ks) in enumerate(K_CLASSES.items()):
        for mi, M in enumerate(Ms):
            for ni, N in enumerate(Ns):
                out.append((cls, ks[(mi * 5 + ni + ci + variant) % len(ks)], mi, ni, M, N))
    return out


class _Checks:
    """Collects (label, got, want) of one shape case and compares them with ONE device round trip."""

    def __init__(self):
        self.items, self.failures, self.n = [], [], 0

    def add(self, label, got, want):
        self.items.append((label, got, want, (got.double() != want).any()))     # NaN != x: unwritten output is caught too

    def flush(self):
        if self.items:
            bad = torch.stack([it[3] for it in self.items]).cpu()
            for (label, got, want, _), f in zip(self.items, bad.tolist()):
                if f:
                    d = got.double() != want
                    at = d.nonzero()[0].tolist()
                    self.failures.append(f"{label}: {int(d.sum())} of {d.numel()} differ, first at {at}: got "
                                         f"{float(got[tuple(at)])!r}, want {float(want[tuple(at)])!r}")
            self.n += len(self.items)
            self.items = []

    def finish(self, what):
        self.flush()
        assert not self.failures, f"{len(self.failures)} of {self.n} {what} differ from the float64 reference:\n" + \
            "\n".join(self.failures[:12])


def _run_epilogues(chk, variant, tag, x, w, b, r, gate):
    """bias on / off x gate on / off x the three activations on the plain entry points, bias x activation x
    (R separate, R aliased to Y) on the residual one; all against the float64 reference."""
    _assert_exact_regime(x, w, b, r, 2)
    M, N = x.shape[0], w.shape[0]
    for bias in (None, b):
        for gt in (None, gate):
            pre = _pre(x, w, bias, gt, GATE_SLOPE)
            assert float(pre.abs().max()) < LIMIT
            for act in ACTS:
                y = torch.full((M, N), float("nan"), device=x.device)
                _launch(variant, x, w, bias, gt, None, act, y)
                chk.add(f"{tag} bias={bias is not None} gate={gt is not None} act={act}", y, _act(pre, act, SLOPE))
        pre = _pre(x, w, bias, r=r)
        assert float(pre.abs().max()) < LIMIT
        for act in ACTS:
            for alias in (False, True):
                y = r.clone() if alias else torch.full((M, N), float("nan"), device=x.device)
                _launch(variant, x, w, bias, None, y if alias else r, act, y)
                chk.add(f"{tag} residual bias={bias is not None} act={act} aliased={alias}", y, _act(pre, act, SLOPE))


# ------------------------------------------------------------------------------------------------------
# 1. integer-exact, every variant
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_exact_every_variant(dev, pools, variant):
    """Zero tolerance against float64 for every (K class, M edge, N edge) of this variant's tile, with bias / gate /
    activation / residual (separate and in place) in every case; K <= 8 additionally with 12-bit x and up to 11-bit w
    (full fp32 products: a tf32- or bf16-style multiply cannot pass)."""
    chk, seen, ks_seen, cases = _Checks(), set(), set(), _shape_cases(variant)
    for i, (cls, K, mi, ni, M, N) in enumerate(cases):
        tag = f"variant {variant} M={M} N={N} K={K}"
        _run_epilogues(chk, variant, tag, *_window(pools, i, M, N, K))
        if K in WIDE_K:
            _run_epilogues(chk, variant, tag + " wide", *_window(pools, i, M, N, K, wide=True))
        chk.flush()
        seen.add((cls, mi, ni))
        ks_seen.add(K)
    chk.flush()
    print(f"\nvariant {variant}: {len(cases)} shape cases, {chk.n} launches; (K class, M edge, N edge) covered: "
          f"{len(seen)} of {len(K_CLASSES) * 25}; K values covered: {len(ks_seen)} of {len(K_ALL)}")
    assert len(seen) == len(K_CLASSES) * 25 and ks_seen == set(K_ALL) and set(K_ISSUE) <= ks_seen
    chk.finish("launches")


# ------------------------------------------------------------------------------------------------------
# 2. NaN moat
# ------------------------------------------------------------------------------------------------------
def _moated(data, extra_rows, c0, aligned, fill=float("nan")):
    """(big, view): `data` [M,C] as big[:M, c0:c0+C] of a buffer with `extra_rows` rows below, at least one column to the
    right and a row stride that is (not) a multiple of 4; everything else is `fill` (an int: that bit pattern)."""
    M, C = data.shape
    ld = c0 + C + 1
    while (ld % 4 == 0) != aligned:
        ld += 1
    big = torch.empty((M + extra_rows, ld), device=data.device)
    if isinstance(fill, int):
        big.view(torch.int32).fill_(fill)
    else:
        big.fill_(fill)
    view = big[:M, c0:c0 + C]
    view.copy_(data)
    return big, view


def _untouched(big, M, c0, N):
    """All of a sentinel-filled buffer outside [:M, c0:c0+N] still holds the sentinel, bit for bit."""
    bits = big.view(torch.int32).clone()
    bits[:M, c0:c0 + N] = SENTINEL
    return (bits != SENTINEL).any()


@pytest.mark.parametrize("variant", VARIANTS)
def test_nan_moat(dev, pools, variant):
    """The exact data as views into larger buffers: NaN around X, gate, W, bias and R (rows below, columns left and right,
    row strides with ld % 4 == 0 and != 0, column offsets 0 / 3 / 8), a sentinel around Y. An exact result means no NaN
    entered a sum (zero fill past K, row < M, col < N on every load); an intact sentinel means no store left the view."""
    bm, bn = TILE[variant]
    chk, moat = _Checks(), []
    Ms = [1, bm - 1, bm, bm + 1, 2 * bm + 3]
    Ns = [1, bn - 1, bn, bn + 1, bn + 33]
    i = 0
    for mi, M in enumerate(Ms):
        for ni, N in enumerate(Ns):
            i += 1
            K = K_ALL[(3 * i + variant) % len(K_ALL)]
            x, w, b, r, gate = _window(pools, i, M, N, K)
            _assert_exact_regime(x, w, b, r, 2)
            c0, cy = (0, 3, 8)[i % 3], (8, 0, 3)[(i // 3) % 3]
            al = bool((i // 2) % 2)
            _, xv = _moated(x, bm, c0, al)
            _, gv = _moated(gate, bm, (3, 8, 0)[i % 3], not al)
            wbig = torch.full((N + bn, K), float("nan"), device=dev)
            wbig[:N] = w
            bbig = torch.full((N + bn,), float("nan"), device=dev)
            bbig[:N] = b
            wv, bv = wbig[:N], bbig[:N]
            tag = f"variant {variant} M={M} N={N} K={K} c0={c0} ldx={xv.stride(0)}"
            for bias, gt, res, act in ((bv, gv, None, "leaky"), (None, None, None, None), (bv, None, "sep", "relu"),
                                       (None, None, "alias", None)):
                ybig, yv = _moated(r if res == "alias" else torch.zeros_like(r), bm, cy, not al, fill=SENTINEL)
                if res == "alias":
                    rv = yv
                elif res == "sep":
                    _, rv = _moated(r, bm, c0, al)
                else:
                    rv = None
                if res != "alias":
                    yv.fill_(float("nan"))
                _launch(variant, xv, wv, bias, gt, rv, act, yv)
                want = _ref(x, w, b if bias is not None else None, act, SLOPE, gate if gt is not None else None, GATE_SLOPE,
                            r if res else None)
                chk.add(f"{tag} bias={bias is not None} gate={gt is not None} res={res} act={act}", yv, want)
                moat.append((f"{tag} res={res}", _untouched(ybig, M, cy, N)))
            chk.flush()
    broken = [lab for (lab, _), f in zip(moat, torch.stack([m[1] for m in moat]).cpu().tolist()) if f]
    assert not broken, "stores outside the output view:\n" + "\n".join(broken[:12])
    chk.finish("moated launches")


# ------------------------------------------------------------------------------------------------------
# 3. one summation order
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(5, 40, 3), (200, 64, 3), (600, 128, 131), (257, 130, 259), (600, 64, 64), (129, 129, 33),
                                   (300, 1024, 512), (515, 130, 70)])
def test_one_summation_order(dev, M, N, K):
    """Random data. The non-split variants sum an element's products in ONE order (gemm.hip, above gemm_nt_launch): their
    outputs are identical bit for bit. The K-split variants sum in another order and are held to the float64
    reference at the project's tolerance, as is the default. Every variant repeats itself bit for bit."""
    g = torch.Generator().manual_seed(M + 3 * N + 7 * K)
    x = torch.randn(M, K, generator=g).to(dev)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(dev)
    b = torch.randn(N, generator=g).to(dev)
    out = {}
    for v in VARIANTS:
        ys = []
        for _ in range(2):
            y = torch.full((M, N), float("nan"), device=dev)
            _launch(v, x, w, b, None, None, "leaky", y, slope=0.2)
            ys.append(y)
        assert torch.equal(ys[0].view(torch.int32), ys[1].view(torch.int32)), f"variant {v} does not repeat itself"
        out[v] = ys[0]
    for v in NONSPLIT[1:]:
        same = out[v].view(torch.int32) == out[-1].view(torch.int32)
        assert bool(same.all()), f"variant {v} differs from the default tiling in {int((~same).sum())} of {same.numel()} elements"
    ref = _ref(x, w, b, "leaky", 0.2)
    for v in (-1, 11, 12):
        torch.testing.assert_close(out[v].double(), ref, rtol=2e-5, atol=2e-5)


# ------------------------------------------------------------------------------------------------------
# 4. batch invariance through ops, the variant pinned
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,N,K,variant", [(300, 128, 131, 11), (64, 128, 256, 12), (2048, 128, 128, -1)])
@pytest.mark.parametrize("op", ["linear_act", "linear_res_act", "gemm_nt"])
def test_batch_invariance(ops, dev, op, R, N, K, variant):
    """A cloud's rows computed alone (B = 1), in a pair (B = 2) and in a batch of 5 are the same bits, forward and
    backward — on the default tiling and on both K-split variants, which ops picks from the per-cloud shape only."""
    assert ops.gemm_variant(R, N, K) == variant
    g = torch.Generator().manual_seed(R + N + K)
    x = torch.randn(5, R, K, generator=g).to(dev)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(dev)
    b = torch.randn(N, generator=g).to(dev)
    r = torch.randn(5, R, N, generator=g).to(dev)
    gy = torch.randn(5, R, N, generator=g).to(dev)

    def run(sl):
        xs, rs, gs = x[sl], r[sl], gy[sl]
        if op == "gemm_nt":
            return (ops.gemm_nt(xs.reshape(-1, K), w, b, "leaky", 0.2, unit_rows=R).view(-1, R, N),)
        xa = xs.clone().requires_grad_()
        if op == "linear_act":
            y = ops.linear_act(xa, w, b, "leaky", 0.2)
            y.backward(gs)
            return y.detach(), xa.grad
        ra = rs.clone().requires_grad_()
        y = ops.linear_res_act(xa, w, b, ra, "relu")
        y.backward(gs)
        return y.detach(), xa.grad, ra.grad

    full = run(slice(0, 5))
    ref = _pre(x.reshape(-1, K), w, b, r=r.reshape(-1, N) if op == "linear_res_act" else None)
    ref = torch.relu(ref) if op == "linear_res_act" else F.leaky_relu(ref, 0.2)
    torch.testing.assert_close(full[0].reshape(-1, N).double(), ref, rtol=2e-5, atol=2e-5)
    for sl in (slice(0, 1), slice(2, 3), slice(4, 5), slice(1, 3), slice(3, 5)):
        part = run(sl)
        for name, a, f in zip(("y", "dx", "dr"), part, full):
            assert torch.equal(a.contiguous().view(torch.int32), f[sl].contiguous().view(torch.int32)), \
                f"{op} {name}: clouds {sl.start}:{sl.stop} alone differ from the same clouds in the batch of 5"


# ------------------------------------------------------------------------------------------------------
# 5. generated operands, group-max epilogue
# ------------------------------------------------------------------------------------------------------
def test_gather_exact(dev):
    """Gathered A (GemmArgs::ga_idx): row m = act_in(P[cloud * NA + idx[m]] + Bc[group]) generated on load, an index == NA
    reading as a zero row; Y, the input sign mask (K % 4 == 0) and the output sign mask (N % 32 == 0) exactly."""
    g = torch.Generator().manual_seed(11)
    B, NA, S = 2, 50, 3
    chk, n = _Checks(), 0
    for ns in (16, 32, 128):
        M = B * S * ns
        idx = torch.randint(0, NA, (B, S, ns), generator=g, dtype=torch.int32)
        idx[..., ns // 2:] = idx[..., :1]            # a repeated-index tail (a ball query pads with its first hit)
        idx[0, 0, 1] = NA                            # reads as a zero row
        idx[-1, -1, 2] = NA
        idx = idx.to(dev)
        for K, want_mask in ((8, True), (64, True), (132, True), (6, False), (35, False), (131, False)):
            P = _odd(g, (B * NA, K), 15).to(dev)
            Bc = torch.randint(-15, 16, (B * S, K), generator=g).float().to(dev)
            rows = torch.cat([P.double(), torch.zeros(1, K, dtype=torch.float64, device=dev)])        # row B * NA: the zero row
            src = torch.arange(B, device=dev).view(B, 1, 1) * NA + idx.long()
            src = torch.where(idx == NA, torch.full_like(src, B * NA), src).reshape(M)
            pre_in = rows[src] + Bc.double().repeat_interleave(ns, 0)
            for N in (48, 64, 96, 160):              # N <= 64: 128 x 64 tiles, else 128 x 128
                w = _odd(g, (N, K), 63).to(dev)
                b = torch.randint(-1000, 1001, (N,), generator=g).float().to(dev)
                for slope_in in (0.0, 0.25):
                    act = (None, "relu", "leaky")[n % 3]
                    n += 1
                    A = torch.where(pre_in > 0, pre_in, slope_in * pre_in)
                    assert float((A.abs() @ w.abs().double().t() + b.abs().double()).max()) * 4 < LIMIT
                    pre = A @ w.double().t() + b.double()
                    y = torch.full((M, N), float("nan"), device=dev)
                    mask = torch.full((M, K // 4), 0xFF, dtype=torch.uint8, device=dev) if want_mask else None
                    ym = torch.full((M, N // 32), -1, dtype=torch.int32, device=dev) if N % 32 == 0 else None
                    _lib.call("pc3d_gemm_nt_gather_f32", P.data_ptr(), K, Bc.data_ptr(), idx.data_ptr(), B, NA, S, ns, slope_in,
                              w.data_ptr(), b.data_ptr(), N, K, ACTS[act], SLOPE, y.data_ptr(), N, _p(mask), _p(ym), _stream())
                    tag = f"gather ns={ns} K={K} N={N} slope_in={slope_in} act={act}"
                    chk.add(tag, y, _act(pre, act, SLOPE))
                    if mask is not None:
                        bits = (pre_in > 0).view(M, K // 4, 4).long()
                        chk.add(tag + " input sign mask", mask, (bits << torch.arange(4, device=dev)).sum(-1).double())
                    if ym is not None:
                        bits = (pre > 0).view(M, N // 32, 32).long()
                        chk.add(tag + " output sign mask", ym.long() & 0xFFFFFFFF,
                                (bits << torch.arange(32, device=dev)).sum(-1).double())
            chk.flush()
    chk.finish("gathered-operand results")


def test_poolbwd_exact(dev):
    """Pooled-gradient A (GemmArgs::pb_g): dY[m, c] = (Y > 0 ? 1 : slope) * ((arg[b, c] == n ? g[b, c] : 0) + g[b, K + c] / Npts)
    generated on load, dX = dY @ W^T. The mean gradients are multiples of Npts / 4, so dY is a multiple of 1 / 16."""
    g = torch.Generator().manual_seed(12)
    B, chk = 2, _Checks()
    for Npts in (128, 256):
        M = B * Npts
        n_idx = torch.arange(Npts, device=dev).view(1, Npts, 1)
        for K in (4, 36, 64, 132):
            Y = torch.randint(-3, 4, (M, K), generator=g).float().to(dev)              # zeros included: Y > 0 is strict
            gr = torch.cat([torch.randint(-31, 32, (B, K), generator=g).float(),
                            torch.randint(-31, 32, (B, K), generator=g).float() * (Npts // 4)], 1).to(dev)
            arg = torch.randint(0, Npts, (B, K), generator=g, dtype=torch.int32)
            arg[:, 0::5] = 0                                                           # winners in the first ...
            arg[:, 1::5] = Npts - 1                                                    # ... and in the last row of a cloud
            arg = arg.to(dev)
            sel = torch.where(arg.view(B, 1, K) == n_idx, gr[:, None, :K].double(), 0.0)
            dY = (torch.where(Y.view(B, Npts, K) > 0, 1.0, 0.25) * (sel + gr[:, None, K:].double() / Npts)).reshape(M, K)
            for N in (40, 130):                      # N <= 64: 128 x 64 tiles, else 128 x 128 double-buffered
                w = _odd(g, (N, K), 63).to(dev)
                assert float((dY.abs() @ w.abs().double().t()).max()) * 16 < LIMIT
                dX = torch.full((M, N), float("nan"), device=dev)
                _lib.call("pc3d_gemm_nt_poolbwd_f32", Y.data_ptr(), K, gr.data_ptr(), arg.data_ptr(), B, Npts, 0.25,
                          w.data_ptr(), N, K, dX.data_ptr(), N, _stream())
                chk.add(f"poolbwd Npts={Npts} K={K} N={N}", dX, dY @ w.double().t())
    chk.finish("pooled-gradient results")


def test_groupmax_exact(ops, dev):
    """Group-max epilogue (GemmArgs::gm_ns) through ops.linear_relu_max: relu(max over a group's rows + bias) and the
    winning row, exactly, on data with exact ties inside a group (duplicated rows): the lowest row wins."""
    g = torch.Generator().manual_seed(13)
    chk = _Checks()
    for ns in (32, 64, 128):
        G = {32: 7, 64: 3, 128: 3}[ns]              # a last 128-row tile that is not full of groups
        assert ns == 128 or G % (128 // ns)
        for C2 in (8, 64, 72, 128):                  # C2 <= 64: variant 8, else 5
            x = _odd(g, (G, ns, C2), 63)
            x[:, ns // 2] = x[:, 3]                  # ties between rows of different lanes / registers / 32-row tiles
            x[:, ns - 1] = x[:, 0]
            x0 = x.to(dev)
            for C3 in (32, 96, 160):
                w = _odd(g, (C3, C2), 63).to(dev)
                b = torch.randint(-1000, 1001, (C3,), generator=g).float().to(dev)
                # ... and, so that a tie AT the maximum is certain: channel 0's winning row of every group, copied half a
                # group further (it stays the maximum; the lower of the two rows must be reported)
                x, gi = x0.clone(), torch.arange(G, device=dev)
                win = (x.double() @ w[0].double()).argmax(1)
                x[gi, (win + ns // 2) % ns] = x[gi, win]
                pre = x.double() @ w.double().t()                                       # [G, ns, C3]
                assert float((x.abs().double() @ w.abs().double().t()).max()) + 1000 < LIMIT
                top = pre.max(dim=1).values
                rows = torch.arange(ns, device=dev).view(1, ns, 1).expand_as(pre)
                first = torch.where(pre == top[:, None], rows, ns).min(dim=1).values    # the lowest row among the ties
                assert bool(((pre == top[:, None]).sum(1)[:, 0] > 1).all())
                tag = f"groupmax ns={ns} C2={C2} C3={C3}"
                chk.add(tag, ops.linear_relu_max(x, w, b), torch.relu(top + b.double()))
                out, arg = ops._group_linear_max_fwd(x, w, b)
                chk.add(tag + " values (raw)", out, torch.relu(top + b.double()))
                chk.add(tag + " winning rows", arg, first.double())
        chk.flush()
    chk.finish("group-max results")


# ------------------------------------------------------------------------------------------------------
# 6. refusals
# ------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    """All of these return before any launch."""
    M, N, K = 128, 64, 64
    x, w, r, y = torch.ones(M, K, device=dev), torch.ones(N, K, device=dev), torch.ones(M, N, device=dev), torch.zeros(M, N, device=dev)
    st = _stream()
    for v in (7, 9, 10, 13, -1):
        with pytest.raises(_lib.Pc3dError):
            _lib.call("pc3d_gemm_nt_tiled_f32", x.data_ptr(), K, w.data_ptr(), 0, 0, 0, 0.0, M, N, K, 0, 0.0, y.data_ptr(), N, v, st)
    for ldx, ldy in ((K - 1, N), (K, N - 1)):
        with pytest.raises(_lib.Pc3dError):
            _lib.call("pc3d_gemm_nt_f32", x.data_ptr(), ldx, w.data_ptr(), 0, 0, 0, 0.0, M, N, K, 0, 0.0, y.data_ptr(), ldy, st)
        for v in (5, 11, 12):
            with pytest.raises(_lib.Pc3dError):
                _lib.call("pc3d_gemm_nt_tiled_f32", x.data_ptr(), ldx, w.data_ptr(), 0, 0, 0, 0.0, M, N, K, 0, 0.0, y.data_ptr(),
                          ldy, v, st)
        with pytest.raises(_lib.Pc3dError):
            _lib.call("pc3d_gemm_nt_res_f32", x.data_ptr(), ldx, w.data_ptr(), 0, r.data_ptr(), N, M, N, K, 0, 0.0, y.data_ptr(),
                      ldy, -1, st)
    for v in (-1, 11):
        with pytest.raises(_lib.Pc3dError):
            _lib.call("pc3d_gemm_nt_res_f32", x.data_ptr(), K, w.data_ptr(), 0, 0, N, M, N, K, 0, 0.0, y.data_ptr(), N, v, st)
    gr, arg = torch.ones(1, 2 * K, device=dev), torch.zeros(1, K, dtype=torch.int32, device=dev)
    for Npts, Kp in ((96, K), (129, K), (128, K - 2), (128, K - 1)):
        with pytest.raises(_lib.Pc3dError):
            _lib.call("pc3d_gemm_nt_poolbwd_f32", x.data_ptr(), K, gr.data_ptr(), arg.data_ptr(), 1, Npts, 0.25, w.data_ptr(), N, Kp,
                      y.data_ptr(), N, st)
    assert float(y.abs().max()) == 0.0               # nothing ran
