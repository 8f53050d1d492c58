"""Seeded inputs and calls for the bit-exact record of the optimiser-update kernels (tests/golden/update_bits.npz).

tests/golden/make_update_bits.py (the recorder) and tests/test_update_bits_gpu.py (the check) both import this module, so
the two cannot drift apart: ENTRIES maps an entry point of `ops` to a function that builds its cases with numpy, runs
them on the device and returns {"<case>/<output>": tensor}. Every case draws from its own generator, seeded by its name.
B = 3 throughout; the other sizes are the smallest at which each kernel takes every one of its paths.
"""
import hashlib
import itertools
import zlib

import numpy as np
import torch

B = 3
F32 = np.float32
ARRAY_MAX_BYTES = 4096      # outputs up to this size are stored as arrays, larger ones as their sha256


def bits(t):
    """The tensor's storage as integers (so that NaN == NaN and -0 != +0), contiguous, on the CPU."""
    t = t.detach().contiguous().cpu()
    if t.is_floating_point():
        t = t.view({4: torch.int32, 8: torch.int64}[t.element_size()])
    return t


def stored(t):
    """What the fixture keeps of an output: its integer view, or the sha256 of that view's bytes (uint8[32])."""
    a = bits(t).numpy()
    if a.nbytes <= ARRAY_MAX_BYTES:
        return a
    return np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8).copy()


class _Gen:
    def __init__(self, name, dev):
        self.rng = np.random.default_rng(zlib.crc32(name.encode()))
        self.dev = dev

    def t(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def randn(self, *shape, scale=1.0):
        return (self.rng.standard_normal(shape) * scale).astype(F32)

    def rand(self, *shape, scale=1.0):
        return (self.rng.random(shape) * scale).astype(F32)

    def idx(self, hi, *shape):
        return self.rng.integers(0, hi, shape).astype(np.int32)

    def unit(self, *shape):      # [..., 3, K] unit vectors along dim -2
        a = self.rng.standard_normal(shape)
        return (a / np.linalg.norm(a, axis=-2, keepdims=True)).astype(F32)

    def layout(self, a, cf):
        """[B,3,K] array -> the device tensor ops takes for `cf`: [B,3,K] or a contiguous [B,K,3]."""
        t = self.t(a)
        return t if cf else t.transpose(1, 2).contiguous()

    def step(self, device_word):
        """Host step 1, or a device step word holding 1000 (the pow path far from its first values)."""
        return torch.tensor([1000], dtype=torch.int32, device=self.dev) if device_word else 1

    def moments(self, *shape):
        return self.randn(*shape, scale=0.01), self.rand(*shape, scale=1e-3)


def _i64(g, vals):
    return g.t(np.asarray(vals, dtype=np.int64))


def _f32(g, vals):
    return g.t(np.asarray(vals, dtype=F32))


def adam_clip_step(ops, dev):
    out = {}
    for K, mode, g2, cf, word in itertools.product((1, 257), ("none", "linf", "project"), (False, True), (True, False),
                                                   (False, True)):
        name = f"K{K}-{mode}-g2{int(g2)}-cf{int(cf)}-dev{int(word)}"
        g = _Gen("adam_clip_step/" + name, dev)
        ori = g.randn(B, 3, K)
        p = g.layout(ori + g.randn(B, 3, K, scale=0.05), cf)
        grad = g.layout(g.randn(B, 3, K, scale=0.1), cf)
        grad2 = g.layout(g.randn(B, 3, K, scale=0.1), cf) if g2 else None
        m0, v0 = g.moments(B, 3, K)
        m, v = g.layout(m0, cf), g.layout(v0, cf)
        normal = g.layout(g.unit(B, 3, K), cf) if mode == "project" else None
        ops.adam_clip_step(p, grad, m, v, g.step(word), 0.01, ori=None if mode == "none" else g.layout(ori, cf),
                           normal=normal, budget=0.0 if mode == "none" else 0.06, cf=cf, g2=grad2)
        out.update({f"{name}/p": p, f"{name}/m": m, f"{name}/v": v})
    return out


def clip(ops, dev):
    out = {}
    K = 257
    for normals, cf in ((False, True), (True, True), (True, False)):
        name = f"K{K}-n{int(normals)}-cf{int(cf)}"
        g = _Gen("clip/" + name, dev)
        ori, n = g.randn(B, 3, K), g.unit(B, 3, K)
        pc = ori + g.randn(B, 3, K, scale=0.05)
        pc[:, :, 0] = ori[:, :, 0] - 0.01 * n[:, :, 0]      # against the normal: the projection's degenerate branch
        out[f"{name}/out"] = ops.clip(g.layout(pc, cf), g.layout(ori, cf), g.layout(n, cf) if normals else None, budget=0.06,
                                      cf=cf)
    return out


def _cw_inputs(g, K, cf):
    ori = g.randn(B, 3, K)
    adv = ori + g.randn(B, 3, K, scale=0.05)
    m0, v0 = g.moments(B, 3, K)
    return {"ori": g.layout(ori, cf), "adv": g.layout(adv, cf), "g": g.layout(g.randn(B, 3, K, scale=0.1), cf),
            "m": g.layout(m0, cf), "v": g.layout(v0, cf), "w": g.t(g.rand(B) + 0.5), "nn_idx": g.t(g.idx(K, B, K)),
            "l2norm": g.t(np.sqrt(((adv - ori) ** 2).sum((1, 2), dtype=F32)).astype(F32))}


def _book_state(g, untarget, like):
    """Sample 0 succeeds and becomes the best (copy), sample 1 succeeds against bestdist 0 (no change), sample 2 fails.
    Targeted: success is pred == label, and sample 0 sits exactly on it."""
    label = [4, 7, 9]
    pred = [5, 8, 9] if untarget else [4, 7, 3]
    return {"pred": _i64(g, pred), "label": _i64(g, label), "bestdist": _f32(g, [1e10, 0.0, 1e10]),
            "bestscore": _i64(g, [-1, -1, -1]), "o_bestdist": _f32(g, [1e10, 0.0, 1e10]),
            "o_bestscore": _i64(g, [-1, -1, -1]), "o_bestattack": torch.zeros_like(like),
            "input_val": torch.zeros_like(like), "dist_val": torch.zeros(B, dtype=torch.float32, device=g.dev)}


_BOOK_OUT = ("bestdist", "bestscore", "o_bestdist", "o_bestscore", "o_bestattack", "input_val", "dist_val")


def cw_update(ops, dev):
    """K = 333: one point per thread; 2049: three of the 1024-thread form's four-point instantiation."""
    out = {}
    for K, kind, untarget in itertools.product((333, 2049), (0, 1, 2), (True, False)):
        name = f"K{K}-kind{kind}-untarget{int(untarget)}"
        g = _Gen("cw_update/" + name, dev)
        cf = K == 333
        a = _cw_inputs(g, K, cf)
        s = _book_state(g, untarget, a["adv"])
        ops.cw_update(a["adv"], a["ori"], s["pred"], s["label"], untarget, s["bestdist"], s["bestscore"], s["o_bestdist"],
                      s["o_bestscore"], s["o_bestattack"], a["g"], a["m"], a["v"], g.step(not untarget), 0.01, 0.08,
                      input_val=s["input_val"], dist_val=s["dist_val"], dist_kind=kind, w=a["w"] if kind else None,
                      nn_idx=a["nn_idx"] if kind == 2 else None, cf=cf)
        out.update({f"{name}/{k}": a[k] for k in ("adv", "m", "v")})
        out.update({f"{name}/{k}": s[k] for k in _BOOK_OUT})
    return out


def cw_step(ops, dev):
    out = {}
    for K, kind in itertools.product((333, 2049), (0, 1, 2)):
        name = f"K{K}-kind{kind}"
        g = _Gen("cw_step/" + name, dev)
        cf = K == 333
        a = _cw_inputs(g, K, cf)
        ops.cw_step(a["adv"], a["g"], a["m"], a["v"], g.step(K == 2049), 0.01, a["ori"], 0.08, dist_kind=kind,
                    w=a["w"] if kind else None, l2norm=a["l2norm"] if kind == 1 else None,
                    nn_idx=a["nn_idx"] if kind == 2 else None, cf=cf)
        out.update({f"{name}/{k}": a[k] for k in ("adv", "m", "v")})
    return out


def add_update(ops, dev):
    """A = 300 / 700 / 1500: the one-, two- and four-points-per-thread instantiations (thresholds 512 and 1024)."""
    out = {}
    K = 333
    for (A, P), kind in itertools.product(((300, 30), (700, 35), (1500, 60)), ("chamfer", "hausdorff", "far_chamfer")):
        name = f"A{A}-{kind}"
        g = _Gen("add_update/" + name, dev)
        untarget = kind != "hausdorff"
        full = g.randn(B, 3, K + A)
        full[:, :, K + 1] = full[:, :, K]      # a duplicate point, as resampled clusters have
        full = g.t(full)
        grad = g.t(g.randn(B, 3, K + A, scale=0.1))
        adv = full[:, :, K:]
        nn_d = g.rand(B, A)
        nn_d[:, 7] = nn_d[:, A - 9] = 2.0      # a tied maximum: Hausdorff takes the first
        m0, v0 = g.moments(B, 3, A)
        m, v = g.t(m0), g.t(v0)
        s = _book_state(g, untarget, m)
        ops.add_update(adv, full[:, :, :K], g.t(nn_d), g.t(g.idx(K, B, A)), s["pred"], s["label"], untarget, s["bestdist"],
                       s["bestscore"], s["o_bestdist"], s["o_bestscore"], s["o_bestattack"], grad[:, :, K:], m, v,
                       g.step(kind == "chamfer"), 0.01, kind, g.t(g.rand(B) + 0.5), input_val=s["input_val"],
                       dist_val=s["dist_val"], cd_w=0.7, P=P)
        out.update({f"{name}/full": full, f"{name}/m": m, f"{name}/v": v})
        out.update({f"{name}/{k}": s[k] for k in _BOOK_OUT})
    return out


def aof_update(ops, dev):
    out = {}
    N = 333
    for budget, word in itertools.product((0.06, 0.0), (False, True)):
        name = f"N{N}-budget{int(budget > 0)}-dev{int(word)}"
        g = _Gen("aof_update/" + name, dev)
        data = g.randn(B, 3, N)
        hfc = g.randn(B, 3, N, scale=0.3)
        lfc = g.t(data - hfc + g.randn(B, 3, N, scale=0.05))
        m0, v0 = g.moments(B, 3, N)
        m, v = g.t(m0), g.t(v0)
        res = ops.aof_update(lfc, g.t(g.randn(B, 3, N, scale=0.1)), g.t(g.randn(B, 3, N, scale=0.1)), m, v, g.t(hfc),
                             g.t(data), g.step(word), 0.01, budget)
        out.update({f"{name}/lfc": lfc, f"{name}/m": m, f"{name}/v": v, f"{name}/out": res})
    return out


def iso_update(ops, dev):
    """Cloud 0 keeps running (Adam), cloud 1 was done on entry, cloud 2 stops at this evaluation."""
    out = {}
    N, ncls = 65, 40
    for form in ("g", "gW"):
        name = f"N{N}-{form}"
        g = _Gen("iso_update/" + name, dev)
        x = g.t(g.randn(B, 3, N))
        xo = torch.zeros_like(x)
        W = g.t(np.eye(3, dtype=F32) + g.randn(B, 3, 3, scale=0.01))
        m0, v0 = g.moments(B, 3, 3)
        m, v = g.t(m0), g.t(v0)
        done = g.t(np.asarray([0, 1, 0], dtype=np.int32))
        steps = g.t(np.asarray([0 if form == "g" else 999, 5, 41], dtype=np.int32))
        kept_out = torch.zeros(B, ncls, dtype=torch.float32, device=dev)
        kept_pred = _i64(g, [-1, -1, -1])
        grad = g.t(g.randn(B, 3, N, scale=0.1)) if form == "g" else None
        gW = g.t(g.randn(B, 3, 3, scale=0.1)) if form == "gW" else None
        ops.iso_update(x, xo, W, m, v, _i64(g, [4, 7, 8]), _i64(g, [4, 7, 9]), g.t(g.randn(B, ncls)), done, steps, kept_out,
                       kept_pred, 0.01, g=grad, gW=gW)
        out.update({f"{name}/{k}": t for k, t in (("xo", xo), ("W", W), ("m", m), ("v", v), ("done", done), ("steps", steps),
                                                  ("kept_out", kept_out), ("kept_pred", kept_pred))})
    return out


def _knn_lists(g, N, k):
    """Self first, then k random valid neighbours."""
    idx = g.idx(N, B, N, k + 1)
    idx[:, :, 0] = np.arange(N, dtype=np.int32)[None, :]
    return idx


def knn_attack_update(ops, dev):
    out = {}
    k = 5
    for N, clip_mode, knn in itertools.product((257, 1025), ("clip", "project_clip"), (True, False)):
        name = f"N{N}-{clip_mode}-knn{int(knn)}"
        g = _Gen("knn_attack_update/" + name, dev)
        ori = g.randn(B, 3, N)
        adv = g.t(ori + g.randn(B, 3, N, scale=0.05))
        m0, v0 = g.moments(B, 3, N)
        m, v = g.t(m0), g.t(v0)
        # sorted neighbour distances with a heavy tail: about a tenth of the points pass mean + 1.05 std
        d = np.sort(g.rand(B, N, k + 1) * (1.0 + 5.0 * (g.rng.random((B, N, 1)) < 0.1)), axis=2).astype(F32)
        d[:, :, 0] = 0.0
        normal = g.t(g.unit(B, 3, N)) if N == 257 else None      # None: ori doubles as the normal
        ops.knn_attack_update(adv, g.t(ori), g.t(g.randn(B, 3, N, scale=0.1)), m, v, g.step(N == 1025), 0.01, knn_d=g.t(d),
                              knn_idx=g.t(_knn_lists(g, N, k)), nn_idx=g.t(g.idx(N, B, N)), c_chamfer=0.01,
                              c_knn=0.003 if knn else 0.0, alpha=1.05, budget=0.06, clip_mode=clip_mode, normal=normal)
        out.update({f"{name}/adv": adv, f"{name}/m": m, f"{name}/v": v})
    return out


def geoa3_update(ops, dev):
    """Two launches in a row on the same state: the second reads the advanced step words and the decayed lr."""
    out = {}
    steps_max = 4
    for N, k, cc in itertools.product((257, 1025), (0, 4), (0.0, 0.05)):
        name = f"N{N}-k{k}-cc{int(cc > 0)}"
        g = _Gen("geoa3_update/" + name, dev)
        ori = g.randn(B, 3, N)
        off = g.randn(B, 3, N, scale=0.03)
        m0, v0 = g.moments(B, 3, N)
        st = {"x": g.t(ori + off), "offset": g.t(off), "m": g.t(m0), "v": g.t(v0),
              "step": g.t(np.asarray([0, 2, 999], dtype=np.int32)), "lr": g.t(np.full(B, 0.01)),
              "constrain": g.t(g.rand(B)), "loss_rows": torch.zeros(steps_max, B, dtype=torch.float32, device=dev),
              "best_loss": _f32(g, [1e10, 0.0, 1e10]), "best_attack": torch.zeros(B, 3, N, dtype=torch.float32, device=dev),
              "best_bs": _i64(g, [-1, -1, -1]), "best_step": _i64(g, [-1, -1, -1]),
              "iter_best_loss": _f32(g, [1e10, 1e10, 0.0]), "iter_best_score": _i64(g, [-1, -1, -1]),
              "terms_out": torch.zeros(5, B, dtype=torch.float32, device=dev),
              "hd_arg_out": torch.zeros(B, dtype=torch.int32, device=dev),
              "g_out": torch.zeros(B, 3, N, dtype=torch.float32, device=dev)}
        const = dict(nn_ao=g.t(g.idx(N, B, N)), nn_oa=g.t(g.idx(N, B, N)), knn_idx=g.t(_knn_lists(g, N, k)) if k else None,
                     normal_ori=g.t(g.unit(B, 3, N)) if k else None, kappa_ori=g.t(g.rand(B, N)) if k else None)
        args = (g.t(ori), g.t(g.randn(B, 3, N, scale=0.1)))
        words = (g.t(np.asarray([2], dtype=np.int32)), g.t(g.rand(B) + 0.5), g.t(g.randn(B)), _i64(g, [5, 8, 9]),
                 _i64(g, [4, 7, 9]))      # search_step, scale, cls, pred, target: untargeted, cloud 2 fails
        for launch in (1, 2):
            ops.geoa3_update(st["x"], args[0], st["offset"], args[1], st["m"], st["v"], st["step"], words[0], st["lr"],
                             words[1], words[2], words[3], words[4], False, st["constrain"], st["loss_rows"], st["best_loss"],
                             st["best_attack"], st["best_bs"], st["best_step"], st["iter_best_loss"], st["iter_best_score"],
                             dis_kind="CD", gval=1.0, w_dis=1.0, w_hd=0.1, w_curv=1.0 if k else 0.0, scheduler=True,
                             cc_linf=cc, terms_out=st["terms_out"], hd_arg_out=st["hd_arg_out"], g_out=st["g_out"], **const)
            out.update({f"{name}/launch{launch}/{key}": t.clone() for key, t in st.items()})
    return out


ENTRIES = {f.__name__: f for f in (adam_clip_step, clip, cw_update, cw_step, add_update, aof_update, iso_update,
                                   knn_attack_update, geoa3_update)}
