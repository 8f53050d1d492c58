"""Seeded inputs and calls for the bit-exact record of the kernels that use the wave / workgroup primitives of
csrc/pc3d_common.h (wave_argmax_first, wave_incl_scan, wave_sum / wave_max / wave_min at widths 64, 32 and 16,
wave_max_lowest_index, block_sum4_pairwise, block_sum_ordered) and are not already pinned by update_bits_cases.py.

tests/golden/make_wave_bits.py (the recorder) and tests/test_wave_bits_gpu.py (the check) both import this module. ENTRIES
maps a name to a function (ops, dev) -> {"<case>/<output>": tensor}, as in update_bits_cases.py, whose bits / stored / _Gen
are used as they are. B = 3 throughout. The cases are chosen so that a wrong primitive changes an output:

  arg-max     class counts 2, 40, 65 and 130 (one lane, a partial wave, two and three columns per lane); per case a row
              whose maximum is tied in the two 32-lane halves (j, j + 32), a row whose runner-up is tied, and a row tied
              between a lane's own two columns (j, j + 64), where the class count allows each
  scans       per-lane counts with zeros, a nonzero lane 0 and a nonzero last lane, N not a multiple of 64, and for the
              16- and 32-lane scans neighbouring groups with different counts
  block sums  values of mixed magnitude across the waves of a workgroup, so (p0 + p1) + (p2 + p3) and the ascending order
              round differently
"""
import importlib

import numpy as np
import torch

from update_bits_cases import B, F32, _Gen, bits, stored  # noqa: F401  (bits and stored: for the recorder and the test)

CLASS_COUNTS = (2, 40, 65, 130)
WAVE_SCALE = np.asarray([1e-2, 1.0, 37.0, 1e3], dtype=F32)      # magnitude of the values wave w of a 256-thread group holds


def _i64(g, vals):
    return g.t(np.asarray(vals, dtype=np.int64))


def _i32(g, vals):
    return g.t(np.asarray(vals, dtype=np.int32))


def _tied_rows(g, R, k):
    """[R,k] values and per row the index the arg-max must return. Row r is of kind r % 3:
    0: the maximum at j and j + 32; 1: the maximum alone at 5, the runner-up at 7 and 39; 2: the maximum at j and j + 64.
    A class count too small for a kind ties the nearest pair it has instead (k = 2: both classes equal)."""
    z = g.randn(R, k)
    top = np.zeros(R, dtype=np.int64)
    for r in range(R):
        hi = float(z[r].max())
        kind = r % 3
        if k < 40:
            z[r, :] = hi
        elif kind == 0:
            z[r, 3] = z[r, 35] = hi + 1.0
            top[r] = 3
        elif kind == 1:
            z[r, 5] = hi + 1.0
            z[r, 7] = z[r, 39] = hi + 0.5
            top[r] = 5
        elif k >= 65:
            z[r, 0] = z[r, 64] = hi + 1.0
        else:
            z[r, 8] = z[r, 9] = hi + 1.0
            top[r] = 8
    return z, top


def _by_wave(n, threads=256):
    """[n] scale of the value thread i % threads handles: WAVE_SCALE of its wave (a 256-thread group's four waves)."""
    return WAVE_SCALE[((np.arange(n) % threads) // 64) % 4]


# ----------------------------------------------------------------------------------------------------------------------
# arg-max
def cls_loss(ops, dev):
    """kind 0..2 on log_softmax(z), 4..6 on z itself (the raw flag); the target of a runner-up-tie row is its maximum, so
    the tied runner-up decides where the gradient goes."""
    out = {}
    for k in CLASS_COUNTS:
        for kind in (0, 1, 2, 4, 5, 6) if k in (40, 65) else (0, 1, 2):
            name = f"k{k}-kind{kind}"
            g = _Gen("cls_loss/" + name, dev)
            z, top = _tied_rows(g, B, k)
            logp, pred, loss, grad = ops.cls_loss(g.t(z), _i64(g, top), kind, kappa=0.5, scale=1.0 / B)
            out.update({f"{name}/logp": logp, f"{name}/pred": pred, f"{name}/loss": loss, f"{name}/g": grad})
    return out


def cls_tail(ops, dev):
    """fc3 with weights that copy c2's first k entries into the logits (a one-hot W3, zero bias): the ties of c2 arrive
    as exact ties of the logits. k <= 64 (the kernel's limit)."""
    out = {}
    K2 = 256
    for k in (2, 40, 64):
        for kind in (0, 1, 2):
            name = f"k{k}-kind{kind}"
            g = _Gen("cls_tail/" + name, dev)
            z, top = _tied_rows(g, B, k)
            c2 = np.maximum(g.randn(B, K2), 0.0).astype(F32)
            c2[:, :k] = z + 8.0                     # positive: post-ReLU activations
            w3 = np.zeros((k, K2), dtype=F32)
            w3[np.arange(k), np.arange(k)] = 1.0
            logp, pred, loss, g_c2 = ops.cls_tail(g.t(c2), g.t(w3), g.t(np.zeros(k, dtype=F32)), _i64(g, top), kind,
                                                  kappa=0.5, scale=1.0 / B)
            out.update({f"{name}/logp": logp, f"{name}/pred": pred, f"{name}/loss": loss, f"{name}/g_c2": g_c2})
    return out


def cta_cotangent(ops, dev):
    out = {}
    G, S, H = B, 2, 8
    for k in CLASS_COUNTS:
        for mode in ops.CTA_MODES:
            name = f"k{k}-{mode}"
            g = _Gen("cta_cotangent/" + name, dev)
            z, top = _tied_rows(g, G * S, k)
            s = dict(mode=mode, targeted=mode == "ori_minus_tar", ori=_i32(g, top[::S]), tar=_i32(g, (top[::S] + 1) % k),
                     w=g.t(np.asarray([0.25, 0.5], dtype=F32)),
                     poll=torch.zeros((G, ops.CTA_POLL_WORDS), dtype=torch.int32, device=dev),
                     hist_ori=torch.zeros((G, H), dtype=torch.float32, device=dev),
                     hist_max=torch.zeros((G, H), dtype=torch.float32, device=dev))
            got = ops.cta_cotangent(g.t(z), s)
            out.update({f"{name}/g": got, f"{name}/poll": s["poll"], f"{name}/hist_ori": s["hist_ori"],
                        f"{name}/hist_max": s["hist_max"]})
    return out


def ig_cotangent(ops, dev):
    out = {}
    S = 2
    for k in CLASS_COUNTS:
        for target in (None, 1):
            name = f"k{k}-target{target}"
            g = _Gen("ig_cotangent/" + name, dev)
            z, _ = _tied_rows(g, S * B, k)
            out[f"{name}/g"] = ops.ig_cotangent(g.t(z), B, S, target)
    return out


def ig_steps(ops, dev):
    """The extreme coordinate sits in the last wave's share of the cloud (N = 333: 999 coordinates on 1024 threads)."""
    out = {}
    N = 333
    for baseline in ("black", "white", "zero"):
        name = f"N{N}-{baseline}"
        g = _Gen("ig_steps/" + name, dev)
        x = g.randn(B, 3, N)
        x[B - 1, 2, N - 2] = -7.0 if baseline == "black" else 7.0
        clouds, base = ops.ig_steps(g.t(x), np.linspace(0.0, 1.0, 3), baseline)
        out.update({f"{name}/clouds": clouds, f"{name}/base": base})
    return out


def query_step(ops, dev):
    """Coordinate mode, one accept / reject decision per cloud from 2B tied rows of log-probabilities."""
    out = {}
    N, L = 20, 7
    for k, top in ((2, 1), (40, 5), (65, 1), (130, 5)):
        name = f"k{k}-top{top}"
        g = _Gen("query_step/" + name, dev)
        lp, tops = _tied_rows(g, 2 * B, k)
        i32 = dict(dtype=torch.int32, device=dev)
        s = dict(top=top, st=g.t(g.randn(B, 3, N)), cand=torch.zeros((2 * B, 3, N), dtype=torch.float32, device=dev),
                 last=torch.zeros((B, 3, N), dtype=torch.float32, device=dev), ori=None, nrm=None, dir=None,
                 tab=g.t(g.idx(3 * N, B, L)), eps=g.t(np.asarray([0.3, -0.3], dtype=F32)), label=_i64(g, tops[::2]),
                 pos=torch.zeros(B, **i32), done=torch.zeros(B, **i32), queries=torch.full((B,), 5, **i32),
                 adv_target=_i32(g, tops[::2]), last_try=torch.zeros(B, **i32),
                 best=g.t(np.asarray([0.0, -999.0, 1e3], dtype=F32)),
                 last_logp=torch.zeros((B, k), dtype=torch.float32, device=dev),
                 acc_trace=torch.full((B, L), -2, **i32),
                 loss_trace=torch.zeros((B, L, 2), dtype=torch.float32, device=dev))
        ops.query_step(s, init=True)
        ops.query_step(s, g.t(lp))
        out.update({f"{name}/{key}": s[key] for key in ("st", "cand", "last", "pos", "done", "queries", "adv_target",
                                                         "last_try", "best", "last_logp", "acc_trace", "loss_trace")})
    return out


def geoa3_record(ops, dev):
    """NaN ranks above every number in this kernel (torch.argmax's rule), unlike wave_argmax_first: row 1 of the nan case
    holds one, behind a larger index's number."""
    out = {}
    N = 21
    for k in (40, 130):
        for nan in (False, True):
            name = f"k{k}-nan{int(nan)}"
            g = _Gen("geoa3_record/" + name, dev)
            z, top = _tied_rows(g, B, k)
            if nan:
                z[1, 38] = np.nan
            st = {"best_loss": g.t(np.asarray([1e10, 0.0, 1e10], dtype=F32)),
                  "best_attack": torch.zeros((B, 3, N), dtype=torch.float32, device=dev),
                  "best_bs": _i64(g, [-1, -1, -1]), "best_step": _i64(g, [-1, -1, -1]),
                  "iter_best_loss": g.t(np.asarray([1e10, 1e10, 0.0], dtype=F32)), "iter_best_score": _i64(g, [-1, -1, -1])}
            label = ops.geoa3_record(g.t(z), _i64(g, (top + 1) % k), False, g.t(g.rand(B)), g.t(g.randn(B, 3, N)), 2, 7,
                                     st["best_loss"], st["best_attack"], st["best_bs"], st["best_step"],
                                     st["iter_best_loss"], st["iter_best_score"])
            out[f"{name}/label"] = label
            out.update({f"{name}/{key}": t for key, t in st.items()})
    return out


# ----------------------------------------------------------------------------------------------------------------------
# workgroup sums
def geoa3_terms(ops, dev):
    """Sums of mixed magnitude by wave; the Hausdorff maximum tied at 266 (wave 0's second pass) and 70 (wave 1): 70."""
    out = {}
    for N, M, curv in ((350, 350, True), (350, 257, False), (65, 65, True)):
        name = f"N{N}-M{M}-curv{int(curv)}"
        g = _Gen("geoa3_terms/" + name, dev)
        d_ao = g.rand(B, N) * _by_wave(N)
        d_oa = g.rand(B, M) * _by_wave(M)
        if N > 266:
            d_ao[:, 266] = d_ao[:, 70] = 2e3
        else:
            d_ao[:, 3] = d_ao[:, 35] = 2e3
        k_adv = g.t(g.rand(B, N) * _by_wave(N)) if curv else None
        k_ori = g.t(g.rand(B, M)) if curv else None
        idx_ao = g.t(g.rng.integers(0, M, (B, N)).astype(np.int64)) if curv else None
        t_ao, t_oa = g.t(d_ao).requires_grad_(), g.t(d_oa).requires_grad_()
        cls = g.t(g.randn(B)).requires_grad_()
        if curv:
            k_adv.requires_grad_()
        terms = ops.geoa3_terms(t_ao, t_oa, k_adv, k_ori, idx_ao, cls, g.t(g.rand(B) + 0.5), 1.0, 0.1, 1.0 if curv else 0.0)
        (terms * g.t(g.randn(5, B))).sum().backward()
        out.update({f"{name}/terms": terms, f"{name}/g_ao": t_ao.grad, f"{name}/g_oa": t_oa.grad, f"{name}/g_cls": cls.grad})
        if curv:
            out[f"{name}/g_k"] = k_adv.grad
    return out


def knn_outlier_loss(ops, dev):
    """The loss is the workgroup sum of the values past mean + alpha * std, so every wave needs some of those, and of
    another magnitude: the points' scale follows the wave that reads them (1 : 1.1 : 1.2 : 1.3) and a tenth of the points
    of every wave lie three times as far out."""
    out = {}
    for N, k, cf in ((300, 5, False), (257, 3, True), (65, 5, False)):
        name = f"N{N}-k{k}-cf{int(cf)}"
        g = _Gen("knn_outlier_loss/" + name, dev)
        scale = np.asarray([1.0, 1.1, 1.2, 1.3], dtype=F32)[(np.arange(N) % 256) // 64] * np.where(np.arange(N) % 10 == 3, 3.0, 1.0)
        pc = g.randn(B, 3, N) * scale.astype(F32)[None, None, :]
        t = g.layout(pc, cf).requires_grad_()
        loss = ops.knn_outlier_loss(t, k=k, alpha=1.05, cf=cf)
        (loss * g.t(g.rand(B) + 0.5)).sum().backward()
        out.update({f"{name}/loss": loss, f"{name}/grad": t.grad})
    return out


def sor_select(ops, dev):
    """The SOR head's float64 mean and variance over the workgroup (block_sum_ordered), fused and two-launch forms. The head
    returns float32 copies and integer decisions: another order of the sixteen float64 partials moves the threshold by a
    few 2^-53 of itself, which these outputs show only if a point sits that close to it. The entry pins the results; it
    cannot see the order (all terms are positive, so no case can magnify it)."""
    defense = importlib.import_module(ops.__name__.rsplit(".", 1)[0] + ".defense")
    out = {}
    for K, k, fused in ((350, 2, False), (350, 2, True), (1100, 4, False), (65, 2, True)):
        name = f"K{K}-k{k}-fused{int(fused)}"
        g = _Gen("sor_select/" + name, dev)
        x = g.randn(B, 3, K) * _by_wave(K, 1024)[None, None, :]
        x[:, :, ::16] *= 4.0                        # points the threshold drops
        res = defense.sor_select(g.t(x), k=k, alpha=1.1, npoint=K, cf=True, fused=fused, want_stats=True)
        out.update({f"{name}/{key}": res[key] for key in ("out", "count", "rank", "src", "v", "thr")})
    return out


# ----------------------------------------------------------------------------------------------------------------------
# scans
def fps(ops, dev):
    """The pruned kernel (N <= 4096) compacts its survivors through block_excl_scan: clustered clouds prune unevenly."""
    out = {}
    for N, S in ((333, 64), (1100, 100), (65, 65)):
        name = f"N{N}-S{S}"
        g = _Gen("fps/" + name, dev)
        centres = g.randn(B, 7, 3) * 3.0
        xyz = centres[:, g.rng.integers(0, 7, N), :] + g.randn(B, N, 3, scale=0.1)
        out[f"{name}/idx"] = ops.fps(g.t(xyz), S, _i32(g, [0, N - 1, 5]))
    return out


def _grouping(g, G, ns, NA):
    """[G,ns] int32 grouping in the ball query's form: cnt listed points, then copies of the first. The counts include 1
    (nothing but padding), ns (no padding) and differ from group to group."""
    cnt = g.rng.integers(1, ns + 1, size=G)
    cnt[0], cnt[G - 1], cnt[1] = ns, ns, 1
    rows = np.stack([g.rng.choice(NA, ns, replace=False) for _ in range(G)])
    return np.where(np.arange(ns)[None, :] < cnt[:, None], rows, rows[:, :1]).astype(np.int32)


def sa_blocks(ops, dev):
    """The unit table: sa_unit_pack_kernel scans tiles per thread. Only the ntiles tiles the launch wrote are kept."""
    out = {}
    for S, ns, unit in ((70, 32, 16), (70, 32, 8), (37, 64, 8), (45, 128, 32)):
        name = f"S{S}-ns{ns}-unit{unit}"
        g = _Gen("sa_blocks/" + name, dev)
        idx = g.t(_grouping(g, B * S, ns, 512).reshape(B, S, ns))
        tb, nt, _ = ops.sa_blocks(idx, unit)
        slots = 8 if unit == 8 else 4
        out.update({f"{name}/ntiles": nt, f"{name}/tb": tb[:int(nt.item()) * slots].clone()})
    return out


def grouped_mlp_max(ops, dev):
    """A set-abstraction chain forward and backward on the sparse, packed path: group_max_bwd_csr_kernel (64-lane scan of
    the row histogram), gs_tiles_kernel (int max, 64-lane scan) and gemm_groupsum_packed_kernel (16-lane scan
    of the active-row words; ns = 64 has two words per group, so neighbouring 16-lane groups hold other groups' counts)."""
    out = {}
    for NA, S, ns, C1, C2, C3 in ((256, 37, 32, 64, 64, 128), (256, 21, 64, 32, 64, 96), (300, 9, 128, 64, 96, 128)):
        name = f"S{S}-ns{ns}-C{C1}-{C2}-{C3}"
        g = _Gen("grouped_mlp_max/" + name, dev)
        idx = g.t(_grouping(g, B * S, ns, NA).reshape(B, S, ns))
        P, Bc = g.t(g.randn(B, NA, C1)).requires_grad_(), g.t(g.randn(B, S, C1)).requires_grad_()
        layers = [(g.t(g.randn(C2, C1, scale=C1 ** -0.5)), g.t(g.randn(C2))),
                  (g.t(g.randn(C3, C2, scale=C2 ** -0.5)), g.t(g.randn(C3)))]
        w = g.randn(B, S, C3)
        w[:, ::3] = 0.0                             # groups without an active row
        res = ops.grouped_mlp_max(P, Bc, idx, layers, rev=ops.group_reverse(idx, NA))
        (res * g.t(w)).sum().backward()
        out.update({f"{name}/out": res, f"{name}/gP": P.grad, f"{name}/gBc": Bc.grad})
    return out


def _tower(g, C3):
    u = lambda *s, k: ((g.rng.random(s) * 2 - 1) / np.sqrt(k)).astype(F32)      # noqa: E731
    return tuple(g.t(a) for a in (u(64, 3, k=3), u(64, k=3), u(128, 64, k=64), u(128, k=64), u(C3, 128, k=128), u(C3, k=128)))


def pointnet_tower(ops, dev):
    """The screened tower forward (its candidate lists are placed by a 64-lane scan; T_head: the 32-lane sum of the input
    transform, with th_K = 256 and another) and the tower backward (64-lane scans of the hit counts, the 32-lane scan of
    the counting sort), plain and through a transform, N not a multiple of the tiles."""
    out = {}
    for N, C3, thK in ((333, 1024, 256), (130, 352, 100), (1, 32, 0)):
        name = f"N{N}-C{C3}-thK{thK}"
        g = _Gen("pointnet_tower/" + name, dev)
        x = g.t(g.randn(B, 3, N, scale=0.5))
        w = _tower(g, C3)
        gp = g.randn(B, C3)
        gp[:, ::5] = 0.0
        if thK:
            head = (g.t(g.randn(B, thK)), g.t(g.randn(9, thK, scale=thK ** -0.5)), g.t(np.eye(3, dtype=F32).reshape(9)))
            pooled, idx, masks, T = ops.pointmlp3_max_fwd_raw(x, w, False, want_masks=True, T_head=head)
            T = T.view(B, 3, 3)
            gx, gT = ops.pointmlp3_max_bwd_raw(x, w, idx, g.t(gp), masks, T=T, want_gT=True)
            out.update({f"{name}/T": T, f"{name}/gT": gT})
        else:
            pooled, idx, masks = ops.pointmlp3_max_fwd_raw(x, w, False, want_masks=True)
            gx = ops.pointmlp3_max_bwd_raw(x, w, idx, g.t(gp), masks)
        pe, ie = ops.pointmlp3_max_fwd_raw(x, w, True, exact=True)
        out.update({f"{name}/pooled": pooled, f"{name}/idx": idx, f"{name}/mask1": masks[0], f"{name}/mask2": masks[1],
                    f"{name}/gx": gx, f"{name}/pooled_exact_relu": pe, f"{name}/idx_exact_relu": ie})
    return out


def pointnet_ft_tower_bwd(ops, dev):
    """The feature-transform victim's blocked tower backward, without a transform and with one (dL/dT partials)."""
    out = {}
    for N, C3 in ((333, 1024), (130, 352)):
        name = f"N{N}-C{C3}"
        g = _Gen("pointnet_ft_tower_bwd/" + name, dev)
        x = g.t(g.randn(B, 3, N, scale=0.5))
        w = _tower(g, C3)
        gp = g.randn(B, C3)
        gp[:, ::5] = 0.0
        pooled, idx, masks = ops.pointmlp3_max_fwd_raw(x, w, False, want_masks=True)
        out[f"{name}/plain/gx"] = ops.pointnet_ft_tower_bwd_raw(x, None, w[0], w[2], w[4], idx, g.t(gp), masks, None, 0)[0]
        T = g.t(np.eye(3, dtype=F32) + g.randn(B, 3, 3, scale=0.2))
        pooled, idx, masks = ops.pointnet_ft_tower_fwd_raw(x, T, *w, False)
        part_gT, nt = ops.pointnet_ft_gT_workspace(B, N, dev, towers=1)
        gx = ops.pointnet_ft_tower_bwd_raw(x, T, w[0], w[2], w[4], idx, g.t(gp), masks, part_gT, 0)[0]
        out.update({f"{name}/T/pooled": pooled, f"{name}/T/idx": idx, f"{name}/T/gx": gx, f"{name}/T/gT": part_gT})
    return out


# ----------------------------------------------------------------------------------------------------------------------
# sums and maxima over groups of lanes
def curve_walk(ops, dev):
    """Softmax, momentum and score reductions over 32 lanes (two curves a wavefront: k = 20, C <= 32) and over 64."""
    out = {}
    for N, C, k, cn, L in ((70, 16, 20, 5, 4), (70, 32, 20, 6, 3), (64, 64, 20, 3, 3), (70, 16, 40, 3, 3)):
        name = f"N{N}-C{C}-k{k}-cn{cn}"
        g = _Gen("curve_walk/" + name, dev)
        feats = g.t(g.randn(B, N, C)).requires_grad_()
        adj = g.t(g.idx(N, B, N, k))
        start = g.t(np.stack([g.rng.choice(N, cn, replace=False) for _ in range(B)]).astype(np.int32))
        ws = (g.t(g.randn(2 * C, scale=C ** -0.5)), g.t(g.randn(1)), g.t(g.randn(2, 2 * C, scale=C ** -0.5)), g.t(g.randn(2)))
        curves = ops.curve_walk(feats, adj, start, *ws, L)
        (curves * g.t(g.randn(B, cn, L, C))).sum().backward()
        out.update({f"{name}/curves": curves, f"{name}/g_feats": feats.grad})
    return out


def three_interp(ops, dev):
    """PU-Net's interpolation backward: three sums over the 16 lanes of a point, 16 points a workgroup (N = 37: a ragged
    last workgroup)."""
    out = {}
    for N, M, C, relu in ((37, 19, 32, False), (65, 40, 64, True)):
        name = f"N{N}-M{M}-C{C}-relu{int(relu)}"
        g = _Gen("three_interp/" + name, dev)
        u, kn = g.t(g.randn(B, N, 3)).requires_grad_(), g.t(g.randn(B, M, 3)).requires_grad_()
        feats = g.t(g.randn(B, M, C)).requires_grad_()
        y = ops.three_interp(u, kn, feats, bias=g.t(g.randn(C)) if relu else None, relu=relu)
        (y * g.t(g.randn(B, N, C))).sum().backward()
        out.update({f"{name}/y": y, f"{name}/g_unknown": u.grad, f"{name}/g_known": kn.grad, f"{name}/g_feats": feats.grad})
    return out


def affine3(ops, dev):
    """The three-column product's backward: L lanes a row (L follows C), three sums over them."""
    out = {}
    for N, C in ((37, 16), (37, 64), (21, 128), (9, 256), (5, 4)):
        name = f"N{N}-C{C}"
        g = _Gen("affine3/" + name, dev)
        x = g.t(g.randn(B, N, 3)).requires_grad_()
        y = ops.affine3(x, g.t(g.randn(C, 3)), g.t(g.randn(C)), -1.0)
        (y * g.t(g.randn(B, N, C))).sum().backward()
        out.update({f"{name}/y": y, f"{name}/gx": x.grad.contiguous()})
    return out


def lpfa_prep(ops, dev):
    """CurveNet's LPFA front: the backward sums three columns over the LP lanes of a point (LP follows C)."""
    out = {}
    for N, C in ((45, 8), (37, 32), (21, 64), (9, 128)):
        name = f"N{N}-C{C}"
        g = _Gen("lpfa_prep/" + name, dev)
        x, pts = g.t(g.randn(B, N, C)).requires_grad_(), g.t(g.randn(B, N, 3)).requires_grad_()
        A, Bc = ops.lpfa_prep(x, pts, g.t(g.randn(C, 3)), g.t(g.randn(C, 3)), g.t(g.randn(C)))
        ((A * g.t(g.randn(B, N, C))).sum() + (Bc * g.t(g.randn(B, N, C))).sum()).backward()
        out.update({f"{name}/A": A, f"{name}/Bc": Bc, f"{name}/gx": x.grad, f"{name}/gpts": pts.grad})
    return out


ENTRIES = {f.__name__: f for f in (cls_loss, cls_tail, cta_cotangent, ig_cotangent, ig_steps, query_step, geoa3_record,
                                   geoa3_terms, knn_outlier_loss, sor_select, fps, sa_blocks, grouped_mlp_max,
                                   pointnet_tower, pointnet_ft_tower_bwd, curve_walk, three_interp, affine3, lpfa_prep)}
