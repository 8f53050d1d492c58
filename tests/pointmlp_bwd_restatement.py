"""TEST INFRASTRUCTURE: the backward of the fused 3 -> 64 -> 128 -> C3 tower with max-pool (pc3d_pointmlp3_max_bwd_f32 and
every other form of it, csrc/pointmlp.hip and csrc/pointmlp_ft.hip) in plain torch, for any dtype, written from the
statement those kernels make and not from their code. The raw backward takes argidx, g and both ReLU masks as inputs, so
there is no tie and no ReLU at zero to resolve: the float64 evaluation of the same inputs is its exact reference. It is
the checker of tests/test_pointmlp_bwd_ref_cpu.py (which ties it to torch autograd) and of
tests/test_pointmlp_bwd_ref_gpu.py (which holds every entry point to it); the product never imports it.

    g2[b,n,:] = sum over {c: argidx[b,c] == n and g[b,c] != 0} of g[b,c] W3[c,:]      (-0 counts as 0, NaN is a hit)
    g2 = where(mask2, g2, 0);  g1 = where(mask1, g2 @ W2, 0);  g' = g1 @ W1                      [B,N,3]
    gx[b,c,n] = g'[b,n,c]                         (T None)
    gx[b,c,n] = sum_d T[b,c,d] g'[b,n,d]          (T given: x' = x @ T)
    part_gT[b,t,3c+d] = sum over the points n < N of the 32-point tile t of x[b,c,n] g'[b,n,d];  words 9..15 = +0

Masks are selects, not products: a masked-off lane of a NaN row is 0. mask1 is int64 [B,N], bit j = layer-1 channel j
(bit 63 the sign bit); mask2 is int32 [B,N,4], word j bit r = layer-2 channel 32 j + r. W2 is [128,64] or per cloud
[B,128,64] (the trunk of a feature-transform PointNet).

`run(float64, ...)` is the reference. `run(float32, ..., order=o)` for o in ORDERS are stand-ins for a correct kernel:
every sum of the statement (the channel sum of a point, the two products, the tile sum) taken as one ascending chain,
as a chain with fused multiply-adds, in blocks of 32 summed in turn, or as a pairwise tree. They use elementwise torch
operations only, so their bits do not depend on the BLAS at hand. `magnitude` is the same statement in float64 on
absolute values: A_gx and A_gT per element, the scale every rounding error of an fp32 evaluation is proportional to.

The band: band[e] = m 2^-24 A[e] with m = min(16 m_ref, k_e). k_e is the number of rounded operations behind an
element (hits of the point + 128 + 64 + 3 + 8; for part_gT + 32 more and the tile's largest hit count): no correct fp32
evaluation in any order leaves k_e 2^-24 A. m_ref = M_REF is the largest |fp32 restatement - float64| / (2^-24 A) over all
ORDERS and all cases(), measured by tests/test_pointmlp_bwd_ref_cpu.py::test_fp32_orders_stay_inside_the_band, which
prints it and fails if a case exceeds the value written here:

    M_REF = 3.34 for gx, 2.27 for part_gT   (measured 3.333 and 2.262)

Both come from the single-bit masks, where an element is ONE product g W3 W2 W1 (T) and every one of its four to nine
roundings counts in full: one_per_point hits at N = 257, C3 = 1024 for gx, skewed hits at N = 257, C3 = 64 for part_gT.
With random masks a point sums some thirty terms per stage, the roundings average out, and the fp32 restatements stay
below 0.51 2^-24 A. The band is therefore 53.4 2^-24 A for gx and 36.3 2^-24 A for part_gT (k_e is at least 203 and
never the smaller one).

The smallest err / band that a mutation of mutations() reaches, any case, fp32 restatement on the mutated inputs
against the float64 reference of the unmutated ones: 4.07 (one hit's g set to 0 at N = 32, C3 = 1024, every channel on
the last point: one of 1024 terms of one chain; the selection demands more than 4 and takes the first candidate that
has it). tests/test_pointmlp_bwd_ref_cpu.py::test_every_mutation_kind_occurs prints it.
"""
import functools

import torch

ORDERS = ("chain", "fma", "blocks", "pairwise")
M_REF = {"gx": 3.34, "gT": 2.27}
SMALLEST_MARGIN = 4.0           # what mutations() demands of every pick
MARGIN = 16.                    # the project's margin over the reference's own error (cw_step_restatement.bands)
EPS = 2. ** -24
TILE = 32                       # points per part_gT record
NAN_WORD = 0x7FC00ABC           # a quiet NaN with a payload: survives only if nobody writes the word


# ----------------------------------------------------------------------------------------------------------------------
# masks
# ----------------------------------------------------------------------------------------------------------------------
def unpack_masks(mask1, mask2):
    """(int64 [B,N], int32 [B,N,4]) -> (bool [B,N,64], bool [B,N,128])"""
    m1 = ((mask1[..., None] >> torch.arange(64)) & 1).bool()
    m2 = ((mask2.long()[..., None] >> torch.arange(32)) & 1).bool()
    return m1, m2.reshape(*mask2.shape[:-1], 128)


def pack_masks(m1, m2):
    """the inverse of unpack_masks"""
    lo = (m1[..., :63].long() << torch.arange(63)).sum(-1)
    mask1 = torch.where(m1[..., 63], lo + torch.iinfo(torch.int64).min, lo)        # bit 63: the sign, no overflow
    w = (m2.reshape(*m2.shape[:-1], 4, 32).long() << torch.arange(32)).sum(-1)
    mask2 = torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)
    return mask1, mask2


# ----------------------------------------------------------------------------------------------------------------------
# sums in a stated order
# ----------------------------------------------------------------------------------------------------------------------
def _mad(acc, a, b, fma):
    """acc + a b in acc's dtype; fma: one rounding (the product is exact in float64, fp32 operands)"""
    if fma and acc.dtype == torch.float32:
        return (acc.double() + a.double() * b.double()).float()
    return acc + a * b


def _dot(a, W, order):
    """a [B,N,K] . W [B or 1,K,J] -> [B,N,J], the sum over k in `order`"""
    K = a.shape[-1]
    if order is None:
        return a @ W
    if order == "pairwise":
        p = a[..., :, None] * W[:, None]
        while p.shape[2] > 1:
            q = p[:, :, 0:p.shape[2] - p.shape[2] % 2:2] + p[:, :, 1::2]
            p = torch.cat([q, p[:, :, -1:]], 2) if p.shape[2] % 2 else q
        return p[:, :, 0]
    parts = []
    for k0 in range(0, K, 32 if order == "blocks" else K):
        acc = torch.zeros(a.shape[0], a.shape[1], W.shape[-1], dtype=a.dtype)
        for k in range(k0, min(K, k0 + 32 if order == "blocks" else K)):
            acc = _mad(acc, a[..., k, None], W[:, None, k], order == "fma")
        parts.append(acc)
    return functools.reduce(lambda s, t: s + t, parts)


def _chains(terms, group, ngroups, fma_of=None):
    """out[i] = the ascending chain from +0 over the rows of `terms` [L,K] with group == i (group sorted, stable).
    fma_of = (g [L], w [L,K]): the terms are g w, accumulated with one rounding each. Round r adds the r-th entry of
    every group at once: one index_add_ whose indices are distinct, so nothing is left to its summation order."""
    out = torch.zeros(ngroups, terms.shape[1], dtype=terms.dtype)
    if not len(group):
        return out
    L = len(group)
    first = torch.ones(L, dtype=torch.bool)
    first[1:] = group[1:] != group[:-1]
    start = torch.cummax(torch.where(first, torch.arange(L), torch.zeros(L, dtype=torch.long)), 0).values
    rank = torch.arange(L) - start
    by_rank = torch.argsort(rank, stable=True)
    counts = torch.bincount(rank).tolist()
    o = 0
    for n in counts:
        sel = by_rank[o:o + n]
        o += n
        if fma_of is not None and terms.dtype == torch.float32:
            g, w = fma_of
            out[group[sel]] = (out[group[sel]].double() + g[sel, None].double() * w[sel].double()).float()
        else:
            out.index_add_(0, group[sel], terms[sel])
    return out


def _channel_sum(gv, w3, pt, ch, npts, order):
    """[npts,128]: per point, the sum of gv[l] w3[l,:] over its hits l. pt, ch [L]: the hits sorted by (point, channel)"""
    terms = gv[:, None] * w3
    if order is None:                                              # float64: the order is below anything a band sees
        return torch.zeros(npts, terms.shape[1], dtype=terms.dtype).index_add_(0, pt, terms)
    if order == "chain":
        return _chains(terms, pt, npts)
    if order == "fma":
        return _chains(terms, pt, npts, fma_of=(gv, w3))
    if order == "blocks":
        key = pt * 32 + ch // 32                                   # C3 <= 1024: at most 32 blocks of 32 channels
        uniq, inv = torch.unique_consecutive(key, return_inverse=True)
        return _chains(_chains(terms, inv, len(uniq)), uniq // 32, npts)
    assert order == "pairwise"
    group = pt
    while True:
        L = len(group)
        if not L:
            return torch.zeros(npts, terms.shape[1], dtype=terms.dtype)
        first = torch.ones(L, dtype=torch.bool)
        first[1:] = group[1:] != group[:-1]
        start = torch.cummax(torch.where(first, torch.arange(L), torch.zeros(L, dtype=torch.long)), 0).values
        rank = torch.arange(L) - start
        if int(rank.max()) == 0:
            out = torch.zeros(npts, terms.shape[1], dtype=terms.dtype)
            out[group] = terms
            return out
        pair = torch.unique_consecutive(group * 1024 + rank // 2, return_inverse=True)[1]
        nxt = torch.zeros(int(pair.max()) + 1, terms.shape[1], dtype=terms.dtype)
        even = rank % 2 == 0
        nxt[pair[even]] = terms[even]
        nxt.index_add_(0, pair[~even], terms[~even])                # distinct indices: one addition each
        g2 = torch.zeros(len(nxt), dtype=torch.long)
        g2[pair] = group
        terms, group = nxt, g2


def hits(argidx, g):
    """bool [B,C3]: the channels whose gradient the kernels route at all (g != 0; NaN counts, -0 does not)"""
    return g != 0


def hit_counts(argidx, g, N):
    """int64 [B,N]: hits per point"""
    B = g.shape[0]
    out = torch.zeros(B, N, dtype=torch.long)
    out.scatter_add_(1, argidx.long(), hits(argidx, g).long())
    return out


def run(dtype, x, T, W1, W2, W3, argidx, g, mask1, mask2, order=None, absolute=False):
    """(gx [B,3,N], part_gT [B,ceil(N/32),16]; T None: (gx, None)) in `dtype`. order None: whatever torch does (float64:
    the reference); else one of ORDERS. absolute: every operand replaced by its absolute value (magnitude())."""
    B, _, N = x.shape
    C3 = W3.shape[0]
    hit = hits(argidx, g)
    conv = (lambda t: t.to(dtype).abs()) if absolute else (lambda t: t.to(dtype))
    xd, W1d, W3d, gd = conv(x), conv(W1), conv(W3), conv(g)
    W2d = conv(W2 if W2.dim() == 3 else W2[None])
    m1, m2 = unpack_masks(mask1, mask2)
    b, c = torch.nonzero(hit, as_tuple=True)
    pt = b * N + argidx.long()[b, c]
    srt = torch.argsort(pt * 1024 + c)                              # by (point, channel): keys are distinct
    b, c, pt = b[srt], c[srt], pt[srt]
    g2 = _channel_sum(gd[b, c], W3d[c], pt, c, B * N, order).reshape(B, N, 128)
    zero = torch.zeros((), dtype=dtype)
    g2 = torch.where(m2, g2, zero)
    g1 = torch.where(m1, _dot(g2, W2d, order), zero)
    gp = _dot(g1, W1d[None], order)                                 # [B,N,3]
    if T is None:
        return gp.transpose(1, 2).contiguous(), None
    Td = conv(T.reshape(B, 3, 3))
    gx = _dot(gp, Td.transpose(1, 2), order).transpose(1, 2).contiguous()
    nt = (N + TILE - 1) // TILE
    pad = nt * TILE - N
    prod = xd.transpose(1, 2)[:, :, :, None] * gp[:, :, None, :]    # [B,N,3(c),3(d)]
    prod = torch.cat([prod, torch.zeros(B, pad, 3, 3, dtype=dtype)], 1).reshape(B, nt, TILE, 9)
    if order is None:
        s = prod.sum(2)
    else:
        s = _dot(prod.transpose(2, 3).reshape(B, nt * 9, TILE), torch.ones(1, TILE, 1, dtype=dtype),
                 "chain" if order == "fma" else order).reshape(B, nt, 9)
    return gx, torch.cat([s, torch.zeros(B, nt, 7, dtype=dtype)], 2)


def magnitude(x, T, W1, W2, W3, argidx, g, mask1, mask2):
    """(A_gx, A_gT or None): the statement in float64 on |g|, |W3|, |W2|, |W1|, |T|, |x| with the same hits and masks"""
    return run(torch.float64, x, T, W1, W2, W3, argidx, g, mask1, mask2, absolute=True)


def term_counts(x, T, argidx, g):
    """(k_gx [B,1,N], k_gT [B,nt,1]): the rounded operations behind an element"""
    B, _, N = x.shape
    cnt = hit_counts(argidx, g, N)
    k = cnt + 128 + 64 + 3 + 8
    nt = (N + TILE - 1) // TILE
    per_tile = torch.cat([cnt, torch.zeros(B, nt * TILE - N, dtype=torch.long)], 1).reshape(B, nt, TILE).max(2).values
    return k[:, None, :].double(), (per_tile + 128 + 64 + 3 + 8 + 32)[:, :, None].double()


def bands(x, T, W1, W2, W3, argidx, g, mask1, mask2, m_ref=None):
    """(band_gx, band_gT or None), float64, per element: min(16 m_ref, k_e) 2^-24 A[e]"""
    m_ref = M_REF if m_ref is None else m_ref
    A_gx, A_gT = magnitude(x, T, W1, W2, W3, argidx, g, mask1, mask2)
    k_gx, k_gT = term_counts(x, T, argidx, g)
    b_gx = torch.clamp(k_gx, max=MARGIN * m_ref["gx"]) * EPS * A_gx
    b_gT = None if A_gT is None else torch.clamp(k_gT, max=MARGIN * m_ref["gT"]) * EPS * A_gT
    return b_gx, b_gT


ARGS = ("x", "T", "W1", "W2", "W3", "argidx", "g", "mask1", "mask2")


def args_of(case, **over):
    return tuple(over.get(k, case[k]) for k in ARGS)


@functools.lru_cache(maxsize=None)
def reference(i, form="raw"):
    """(gx, part_gT, band_gx, band_gT, A_gx, A_gT) of case i, float64, computed once and never modified. form "raw": the
    case as it is; "plain": without T; "trunk": with T and the per-cloud W2b."""
    case = cases()[i]
    over = {"raw": {}, "plain": dict(T=None), "trunk": dict(T=case["T_any"], W2=case["W2b"])}[form]
    a = args_of(case, **over)
    return run(torch.float64, *a) + bands(*a) + magnitude(*a)


# ----------------------------------------------------------------------------------------------------------------------
# the checker
# ----------------------------------------------------------------------------------------------------------------------
def klass(t):
    """0 finite, 1 NaN, 2 +inf, 3 -inf"""
    return torch.isnan(t).long() + 2 * (t == float("inf")).long() + 3 * (t == float("-inf")).long()


def ratio(got, ref, band, keep=None):
    """largest |got - ref| / band over the kept elements (0 / 0 = 0, anything else over a zero band = inf)"""
    err = (got.double() - ref).abs()
    r = err / torch.where(band > 0, band, torch.ones_like(band))
    r = torch.where((band <= 0) & (err > 0), torch.full_like(r, float("inf")), r)
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    if keep is not None:
        r = r[keep.expand_as(r)]
    return float(r.max()) if r.numel() else 0.


def clean_points(case):
    """(bool [B,1,N], bool [B,nt,1]): the points without a non-finite hit, and the tiles that hold only such points"""
    B, _, N = case["x"].shape
    bad = torch.zeros(B, N, dtype=torch.long)
    bad.scatter_add_(1, case["argidx"].long(), (~torch.isfinite(case["g"])).long())
    bad = bad > 0
    nt = (N + TILE - 1) // TILE
    tile_bad = torch.cat([bad, torch.zeros(B, nt * TILE - N, dtype=torch.bool)], 1).reshape(B, nt, TILE).any(2)
    return ~bad[:, None, :], ~tile_bad[:, :, None]


def check(case, gx, part_gT, ref, what=""):
    """gx [B,3,N] and part_gT (or None) of any evaluation against reference(...) = ref. Raises AssertionError; returns
    (ratio_gx, ratio_gT). Rows with a non-finite hit are held to the reference's class word by word, all others — row
    independence — to the finite band. Pad words 9..15 of part_gT must be +0 bit for bit."""
    r_gx, r_gT, b_gx, b_gT = ref[:4]
    ok_pt, ok_tile = clean_points(case)
    assert gx.shape == r_gx.shape, what + ": gx shape %s" % (tuple(gx.shape),)
    q_gx = ratio(gx, r_gx, b_gx, ok_pt)
    assert q_gx <= 1., "%s: gx leaves its band: err / band = %.3g" % (what, q_gx)
    assert torch.equal(klass(gx), klass(r_gx)), what + ": gx: NaN / inf where the reference has none, or the reverse"
    q_gT = 0.
    if r_gT is not None:
        assert part_gT is not None and part_gT.shape == r_gT.shape, what + ": part_gT shape"
        q_gT = ratio(part_gT, r_gT, b_gT, ok_tile)
        assert q_gT <= 1., "%s: part_gT leaves its band: err / band = %.3g" % (what, q_gT)
        assert torch.equal(klass(part_gT), klass(r_gT)), what + ": part_gT: NaN / inf class differs"
        assert not part_gT[:, :, 9:].contiguous().view(torch.int32).any(), what + ": part_gT words 9..15 are not +0"
    return q_gx, q_gT


# ----------------------------------------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------------------------------------
def _weights(gen, C3):
    def u(*s, k):
        return (torch.rand(*s, generator=gen) * 2 - 1) / k ** 0.5
    return u(64, 3, k=3), u(64, k=3), u(128, 64, k=64), u(128, k=64), u(C3, 128, k=128), u(C3, k=128)


def forward(dtype, x, T, weights, relu_last=False):
    """the tower forward in plain torch: (pooled [B,C3], argidx [B,C3] int32, mask1, mask2 packed, h3 [B,N,C3])"""
    W1, b1, W2, b2, W3, b3 = (w.to(dtype) for w in weights)
    xp = x.to(dtype).transpose(1, 2)
    if T is not None:
        xp = xp @ T.to(dtype)
    z1 = xp @ W1.t() + b1
    h1 = torch.relu(z1)
    z2 = h1 @ (W2.transpose(-1, -2) if W2.dim() == 2 else W2.transpose(1, 2)) + b2
    h2 = torch.relu(z2)
    h3 = h2 @ W3.t() + b3
    pooled, idx = h3.max(1)
    if relu_last:
        pooled = torch.relu(pooled)
    mask1, mask2 = pack_masks(z1 > 0, z2 > 0)
    return pooled, idx.to(torch.int32), mask1, mask2, h3


def _hit_map(kind, gen, B, N, C3, natural, arg):
    """argidx [B,C3] int32 of the distribution `kind`, different in every cloud"""
    c = torch.arange(C3)
    if kind == "natural":
        return natural
    rows = []
    for b in range(B):
        if kind == "one_owner":
            r = torch.full((C3,), (N // 2 + 7 * b) % N)
        elif kind == "one_per_point":
            r = (c + 5 * b) % N
        elif kind == "skewed":                       # half of the channels on one point, the rest thinning out
            r = ((torch.rand(C3, generator=gen) ** 4) * N).long().clamp(max=N - 1)
            r[c % 2 == 0] = (3 + b) % N
        elif kind == "last_sub_tile":
            lo = (N - 1) // TILE * TILE
            r = lo + (c + b) % (N - lo)
        elif kind == "last_point":
            r = torch.full((C3,), N - 1)
        elif kind == "live_in_tile":                 # arg live points inside the 128-point tile [128, 256), the rest on a sink
            perm = 128 + torch.randperm(128, generator=gen)[:arg].sort().values
            r = torch.full((C3,), 2 * 128 + 44 + b)
            r[:min(arg, C3)] = perm[:C3]
        elif kind == "empty_tiles":                  # hits in every third 32-point tile only
            live = [t for t in range((N + TILE - 1) // TILE) if t % 3 == (1 + b) % 3] or [0]
            t = torch.tensor(live)[torch.randint(0, len(live), (C3,), generator=gen)]
            r = (t * TILE + torch.randint(0, TILE, (C3,), generator=gen)).clamp(max=N - 1)
        else:
            raise ValueError(kind)
        rows.append(r)
    return torch.stack(rows).to(torch.int32)


def _masks(kind, gen, B, N, own, argidx):
    if kind == "own":
        return own
    if kind == "random":
        return pack_masks(torch.rand(B, N, 64, generator=gen) < 0.5, torch.rand(B, N, 128, generator=gen) < 0.5)
    if kind == "all_on":
        return pack_masks(torch.ones(B, N, 64, dtype=torch.bool), torch.ones(B, N, 128, dtype=torch.bool))
    if kind == "single_bit":                         # point p: only mask1 bit p mod 64 and mask2 bit p mod 128
        p = torch.arange(N)
        m1 = (torch.arange(64)[None, :] == (p % 64)[:, None])[None].expand(B, N, 64)
        m2 = (torch.arange(128)[None, :] == (p % 128)[:, None])[None].expand(B, N, 128)
        return pack_masks(m1, m2)
    if kind == "off_on_live":                        # random, and all-off on the first live point of every cloud
        m1 = torch.rand(B, N, 64, generator=gen) < 0.5
        m2 = torch.rand(B, N, 128, generator=gen) < 0.5
        for b in range(B):
            m1[b, int(argidx[b, 0])] = False
            if b % 2 == 0:
                m2[b, int(argidx[b, 0])] = False
            elif argidx.shape[1] > 1:
                m2[b, int(argidx[b, -1])] = False
        return pack_masks(m1, m2)
    raise ValueError(kind)


def _case(seed, name, B, N, C3, hit="natural", arg=0, mask="own", g_kind="randn", use_T=True):
    gen = torch.Generator().manual_seed(7919 * seed + 13 * N + C3)
    x = torch.randn(B, 3, N, generator=gen) * 0.5
    T_any = torch.randn(B, 3, 3, generator=gen) * 0.5
    w = _weights(gen, C3)
    Tf = torch.eye(64)[None] + 0.2 * torch.randn(B, 64, 64, generator=gen)
    W2b = (w[2][None] @ Tf.transpose(1, 2)).contiguous()
    T = T_any if use_T else None
    _, natural, m1, m2, _ = forward(torch.float64, x, T, w)
    argidx = _hit_map(hit, gen, B, N, C3, natural, arg)
    assert int(argidx.min()) >= 0 and int(argidx.max()) < N
    mask1, mask2 = _masks(mask, gen, B, N, (m1, m2), argidx)
    g = torch.randn(B, C3, generator=gen)
    poisoned = False
    if g_kind == "small":
        g = g * 1e-3
    elif g_kind == "large":
        g = g * 1e3
    elif g_kind == "dead_point":                     # every hit of the point of channel 0 carries +0 or -0
        for b in range(B):
            on = argidx[b] == argidx[b, 0]
            g[b, on] = torch.where(torch.arange(C3)[on] % 2 == 0, 0., -0.)
    elif g_kind == "nonfinite":                      # the points of channels 0, 1, 2 (mod 11) get NaN, +inf, -inf
        poisoned = True
        for b in range(B):
            for j, v in enumerate((float("nan"), float("inf"), float("-inf"))):
                ch = (j + b) % 3 + 11 * torch.arange(4)          # four channels each, other ones in every cloud
                g[b, ch[ch < C3]] = v
    elif g_kind != "randn":
        raise ValueError(g_kind)
    return dict(name=name, x=x, T=T, T_any=T_any, W1=w[0], W2=w[2], W3=w[4], W2b=W2b, weights=w, argidx=argidx, g=g,
                mask1=mask1, mask2=mask2, poisoned=poisoned, hit=hit, mask=mask, g_kind=g_kind)


@functools.lru_cache(maxsize=None)
def cases():
    """The one case list, shared by the CPU and the GPU tests; every case is seeded and none is ever modified."""
    spec = []
    sizes = [(1, 32), (31, 64), (32, 1024), (33, 32), (127, 1024), (128, 64), (129, 1024), (160, 1024), (257, 64),
             (384, 1024)]
    hit_kinds = ["natural", "one_owner", "one_per_point", "skewed", "last_sub_tile", "last_point", "empty_tiles"]
    mask_kinds = ["own", "random", "single_bit", "off_on_live", "all_on"]
    g_kinds = ["randn", "small", "large"]
    for i, (N, C3) in enumerate(sizes):              # every size with two hit distributions, masks and g cycling
        for j in range(2):
            k = 2 * i + j
            hit = hit_kinds[k % len(hit_kinds)]
            mask = mask_kinds[k % len(mask_kinds)]
            if mask == "own" and hit != "natural":
                mask = "random"
            spec.append(dict(B=2 + k % 2, N=N, C3=C3, hit=hit, mask=mask, g_kind=g_kinds[k % 3], use_T=k % 4 != 3))
    for live in (1, 31, 32, 33, 64, 65, 96, 97, 128):   # the packed form's row blocks
        spec.append(dict(B=2, N=384, C3=1024, hit="live_in_tile", arg=live, mask="random", use_T=live % 2 == 1))
    spec.append(dict(B=2, N=1024, C3=1024, hit="natural", mask="own"))
    spec.append(dict(B=3, N=160, C3=1024, hit="natural", mask="own", use_T=False))
    spec.append(dict(B=3, N=160, C3=1024, hit="one_owner", mask="single_bit"))
    spec.append(dict(B=2, N=257, C3=1024, hit="one_per_point", mask="single_bit", use_T=False))
    spec.append(dict(B=3, N=129, C3=64, hit="skewed", mask="off_on_live"))
    spec.append(dict(B=2, N=160, C3=32, hit="last_sub_tile", mask="all_on"))
    for hit, mask, N in (("skewed", "random", 160), ("one_owner", "random", 129), ("natural", "own", 257),
                         ("last_sub_tile", "off_on_live", 160)):
        spec.append(dict(B=3, N=N, C3=1024, hit=hit, mask=mask, g_kind="dead_point", use_T=hit != "one_owner"))
    for hit, mask, N, C3 in (("skewed", "random", 160, 1024), ("one_per_point", "single_bit", 257, 1024),
                             ("natural", "own", 384, 1024), ("one_per_point", "off_on_live", 129, 64),
                             ("live_in_tile", "random", 384, 1024)):
        spec.append(dict(B=3, N=N, C3=C3, hit=hit, mask=mask, g_kind="nonfinite", arg=65, use_T=hit != "natural"))
    out = []
    for i, s in enumerate(spec):
        name = "%02d-N%d-C%d-%s%s-%s-%s-%s" % (i, s["N"], s["C3"], s["hit"], str(s.get("arg", "")) if s["hit"] == "live_in_tile" else "",
                                               s["mask"], s.get("g_kind", "randn"), "T" if s.get("use_T", True) else "noT")
        out.append(_case(i, name, **s))
    return tuple(out)


# ----------------------------------------------------------------------------------------------------------------------
# mutations
# ----------------------------------------------------------------------------------------------------------------------
def _flip(case, which, b, n, bit):
    m1, m2 = case["mask1"].clone(), case["mask2"].clone()
    if which == "mask1":
        m1[b, n] ^= (torch.iinfo(torch.int64).min if bit == 63 else 1 << bit)
    else:
        w, r = bit // 32, bit % 32
        m2[b, n, w] ^= (torch.iinfo(torch.int32).min if r == 31 else 1 << r)
    return dict(mask1=m1, mask2=m2)


def _candidates(case, kind, gen):
    """every single-entry corruption of `kind`, in a seeded order: dicts of replaced inputs (all of them valid inputs)"""
    B, _, N = case["x"].shape
    C3 = case["g"].shape[1]
    idx, g = case["argidx"], case["g"]
    live = torch.nonzero(hits(idx, g) & torch.isfinite(g))
    if kind == "x_past_last_full_tile":
        live = live[idx.long()[live[:, 0], live[:, 1]] >= N // TILE * TILE]
    live = live[torch.randperm(len(live), generator=gen)][:24].tolist()
    if kind == "g_zeroed":
        for b, c in live:
            h = g.clone()
            h[b, c] = 0.
            yield dict(g=h)
    elif kind in ("hit_to_next_point", "hit_across_tile"):
        for b, c in live:
            n = int(idx[b, c])
            to = n + 1 if kind == "hit_to_next_point" else (n // TILE + 1) * TILE + n % TILE
            if kind == "hit_across_tile" and to >= N:
                to = n - TILE
            if 0 <= to < N:
                j = idx.clone()
                j[b, c] = to
                yield dict(argidx=j)
    elif kind == "mask1_bit":
        for b, c in live:
            for bit in (63, int(torch.randint(0, 63, (1,), generator=gen))):
                yield _flip(case, "mask1", b, int(idx[b, c]), bit)
    elif kind.startswith("mask2_word"):
        w = int(kind[-1])
        for b, c in live:
            for bit in (32 * w + 31, 32 * w + int(torch.randint(0, 31, (1,), generator=gen))):
                yield _flip(case, "mask2", b, int(idx[b, c]), bit)
    elif kind == "T_transposed":
        if case["T"] is not None:
            yield dict(T=case["T"].transpose(1, 2).contiguous())
    elif kind == "x_past_last_full_tile":
        if case["T"] is not None and N % TILE:
            for b, c in live:
                n = int(idx[b, c])
                if n >= N // TILE * TILE:
                    x = case["x"].clone()
                    x[b, :, n] += 1.
                    yield dict(x=x)
    else:
        raise ValueError(kind)


MUTATIONS = ("g_zeroed", "hit_to_next_point", "hit_across_tile", "mask1_bit", "mask2_word0", "mask2_word1", "mask2_word2",
             "mask2_word3", "T_transposed", "x_past_last_full_tile")


def _stands_out(case, ref, over):
    """the largest float64 change / band the corruption makes, on the rows check() holds to a band"""
    gx, gT = run(torch.float64, *args_of(case, **over))
    ok_pt, ok_tile = clean_points(case)
    r = ratio(gx, ref[0], ref[2], ok_pt)
    if gT is not None:
        r = max(r, ratio(gT, ref[1], ref[3], ok_tile))
    return r


@functools.lru_cache(maxsize=None)
def mutations(i):
    """[(kind, replaced inputs, float64 change / band)] of case i: per kind the FIRST candidate, in a seeded order over
    live finite hits, whose exact (float64) effect on some element exceeds SMALLEST_MARGIN = 4 x that element's band —
    the mutated term is then 4 x above the band, and an evaluation that is itself inside the band still stands 3 x
    outside. A kind without such a candidate in a case (no T, N = 1, no ragged tile, a point whose masks are all off)
    is left out there; tests/test_pointmlp_bwd_ref_cpu.py asserts that every kind occurs."""
    case = cases()[i]
    ref = reference(i)
    out = []
    for kind in MUTATIONS:
        gen = torch.Generator().manual_seed(1000 * i + len(kind))
        for tried, over in enumerate(_candidates(case, kind, gen)):
            if tried >= 12:
                break
            r = _stands_out(case, ref, over)
            if r > SMALLEST_MARGIN:
                out.append((kind, over, r))
                break
    return tuple(out)
