"""TEST INFRASTRUCTURE: a numpy restatement of csrc/pointmlp_screen_bound.h (the error bound of the PointNet tower's
bf16 screen) and of the arithmetic it speaks about. The product never imports it.

  v  the exact kernel's value: the fp32 fmaf chain from +0 in that kernel's k order (t ascending; within t the
     components 0..3; within a component k = 8t + c, then 8t + 4 + c)
  S  sum_k (ah_k wh_k + ah_k wl_k + al_k wh_k), xh = bf16(x), xl = bf16(x - xh), accumulated in fp32 in an order nobody
     documents: several orders are offered here
  E  PMS_C * norm_up(sum a^2) * norm_up(sum w^2), every operation in fp32 as in the header
"""
import numpy as np

f32 = np.float32
PMS_NORM_INFLATE = f32(1.0) + f32(2.0 ** -15)
PMS_NORM_FLOOR = f32(2.0 ** -45)
PMS_NORM_MAX = f32(2.0 ** 60)
PMS_C = f32(2.0 ** -13)

K_ORDER = np.array([8 * t + 4 * half + c for t in range(16) for c in range(4) for half in range(2)])


def fma32(a, b, c):
    """fmaf on fp32 arrays: the product of two fp32 is exact in float64; the one float64 rounding of the sum in front of
    the fp32 rounding can differ from a true fma only in a double-rounding tie, 2^-29 relative at worst."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def bf16_rne(x, flush=False):
    """fp32 -> bf16 (round to nearest even) -> fp32. flush: bf16 subnormals (|x| < 2^-126) become zero."""
    u = np.ascontiguousarray(x, dtype=f32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(f32)
    if flush:
        r = np.where(np.abs(r) < f32(2.0 ** -126), f32(0) * r, r)
    return r.reshape(np.shape(x))


def chain(a, w):
    """v [P,C]: the exact kernel's fmaf chain; a [P,128], w [C,128] fp32."""
    v = np.zeros((a.shape[0], w.shape[0]), f32)
    for k in K_ORDER:
        v = fma32(a[:, k][:, None], w[:, k][None, :], v)
    return v


def split(x, flush=False):
    """(xh, xl): the two bf16 terms of fp32 x (x - xh is exact in fp32)."""
    xh = bf16_rne(x, flush)
    return xh, bf16_rne((x.astype(f32) - xh).astype(f32), flush)


def terms(a, w, flush=False):
    """The screen's 3 x 128 operand pairs in the kernel's issue order: per k-step of 16, hi.hi, hi.lo, lo.hi."""
    ah, al = split(a, flush)
    wh, wl = split(w, flush)
    A, W = [], []
    for t in range(a.shape[1] // 16):
        k = slice(16 * t, 16 * t + 16)
        A += [ah[:, k], ah[:, k], al[:, k]]
        W += [wh[:, k], wl[:, k], wh[:, k]]
    return np.concatenate(A, axis=1), np.concatenate(W, axis=1)


def screen_sequential(A, W, order=None):
    """S [P,C] with the exact products (bf16 x bf16 fits fp32) added one by one in fp32."""
    s = np.zeros((A.shape[0], W.shape[0]), f32)
    for k in (range(A.shape[1]) if order is None else order):
        s = fma32(A[:, k][:, None], W[:, k][None, :], s)
    return s


def screen_pairwise(A, W):
    p = (A[:, None, :].astype(np.float64) * W[None, :, :].astype(np.float64)).astype(f32)    # exact
    while p.shape[2] > 1:
        if p.shape[2] % 2:
            p = np.concatenate([p, np.zeros_like(p[:, :, :1])], axis=2)
        p = (p[:, :, 0::2] + p[:, :, 1::2]).astype(f32)
    return p[:, :, 0]


def screen_f64(A, W):
    return (A.astype(np.float64) @ W.astype(np.float64).T).astype(f32)


def sumsq(x):
    s = np.zeros(x.shape[0], f32)
    for k in range(x.shape[1]):
        s = fma32(x[:, k], x[:, k], s)
    return s


def norm_up(ss):
    return (np.sqrt(ss.astype(f32)) * PMS_NORM_INFLATE).astype(f32) + PMS_NORM_FLOOR


def norm_ok(n):
    return n <= PMS_NORM_MAX


def bound(a, w):
    """(na [P], cw [C], E [P,C]) as the kernel forms them."""
    na, cw = norm_up(sumsq(a)), (PMS_C * norm_up(sumsq(w))).astype(f32)
    return na, cw, (na[:, None] * cw[None, :]).astype(f32)


def lo_hi(S, na, cw):
    m = np.broadcast_to(-na[:, None], S.shape).astype(f32)
    c = np.broadcast_to(cw[None, :], S.shape).astype(f32)
    return fma32(m, c, S), fma32(-m, c, S)


def candidates(S, na, cw):
    """[P,C] bool: the points whose upper bound reaches the best lower bound of their channel."""
    lo, hi = lo_hi(S, na, cw)
    return hi >= lo.max(axis=0, keepdims=True)
