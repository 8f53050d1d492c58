"""TEST INFRASTRUCTURE: a numpy restatement of csrc/pointmlp_screen_h_bound.h (the error bound of the PointNet tower's
fp16 screen) and of the arithmetic it speaks about. The product never imports it. Norms, the exact chain and the
accumulation orders are those of pointmlp_screen_bound_restatement.

  a'  a 2^sa, one exponent per tile (the tile's largest na lands in [2^13, 2^14)); w' = w 2^sw[c], one per channel
  S   sum_k fp16(a'_k) fp16(w'_k), accumulated in fp32 in an order nobody documents
  E   PMH_C (na 2^sa + PMH_NA_FLOOR) (nw 2^sw), every operation in fp32 as in the header
  and the claim is |v 2^(sa + sw) - S| <= E.
"""
import numpy as np

from pointmlp_screen_bound_restatement import f32, norm_up, sumsq

PMH_C = f32(1.0625 * 2.0 ** -10)
PMH_NA_FLOOR = f32(1.0)
PMH_EXP = 13
PMH_CW_MAX = f32(32.0)


def scale_exp(n):
    """The exponent s with n 2^s in [2^13, 2^14), from the bits of a normal positive fp32 n, as the header takes it."""
    bits = np.ascontiguousarray(n, dtype=f32).view(np.uint32)
    return (PMH_EXP + 127 - ((bits >> 23) & 0xFF).astype(np.int64)).reshape(np.shape(n))


def pow2(s):
    return ((np.asarray(s, np.int64) + 127).astype(np.uint32) << 23).view(f32)


def fp16_rne(x, flush=False):
    """fp32 -> fp16 (round to nearest even) -> fp32. flush: fp16 subnormals (|x| < 2^-14) become zero."""
    r = np.asarray(x, f32).astype(np.float16).astype(f32)
    if flush:
        r = np.where(np.abs(r) < f32(2.0 ** -14), f32(0) * r, r)
    return r


def scales(a, w):
    """(na [P], nw [C], 2^sa (one for the tile), 2^sw [C], sa, sw)."""
    na, nw = norm_up(sumsq(a)), norm_up(sumsq(w))
    sa, sw = scale_exp(na.max()), scale_exp(nw)
    return na, nw, pow2(sa), pow2(sw), int(sa), sw


def terms(a, w, flush=False):
    """The screen's 128 operand pairs: the fp16 images of the scaled rows."""
    _, _, two_sa, two_sw, _, _ = scales(a, w)
    return fp16_rne((a * two_sa).astype(f32), flush), fp16_rne((w * two_sw[:, None]).astype(f32), flush)


def bound(a, w):
    """(naE [P], cw [C], E [P,C], sa, sw [C]) as the kernel and the prepare launch form them."""
    na, nw, two_sa, two_sw, sa, sw = scales(a, w)
    naE = (na * two_sa).astype(f32) + PMH_NA_FLOOR
    cw = (PMH_C * (nw * two_sw).astype(f32)).astype(f32)
    return naE, cw, (naE[:, None] * cw[None, :]).astype(f32), sa, sw


def scaled(v, sa, sw):
    """v 2^(sa + sw[c]) in float64 (exact: |sa + sw| <= 116)."""
    return v.astype(np.float64) * np.exp2((sa + sw).astype(np.float64))[None, :]
