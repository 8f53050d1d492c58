// The error bound of the PointNet tower's fp16 screen (pointmlp_screen.hip, the H form), in plain C++ so that the kernel,
// a host program and the numpy restatement (tests/pointmlp_screen_h_bound_restatement.py) state ONE formula. DESIGN §3.1
// derives it. Norms, their range check and pms_lo / pms_hi are those of pointmlp_screen_bound.h.
//
//   v   the exact kernel's value: the fp32 fmaf chain over k of a_k w_k from +0
//   a'  a 2^sa, sa ONE exponent per tile: the tile's largest na lands in [2^13, 2^14)     (PMH_EXP = 13)
//   w'  w 2^sw, sw one exponent per channel: nw 2^sw lands in [2^13, 2^14)
//   xh  fp16(x'), round to nearest even; what the matrix pipe then sees may also be flushed to zero below 2^-14:
//         |x' - xh| <= max(u |x'|, eta),   u = 2^-11, eta = 2^-14    (no overflow: |x'| < 2^14)
//   S   sum_k ah_k wh_k: ONE fp16 MFMA product per k-step into an fp32 accumulator, in an order and with roundings
//       nobody documents. The products ah wh are exact in fp32 (22 significant bits).
//   |v 2^(sa + sw) - S| <= E = PMH_C (na 2^sa + PMH_NA_FLOOR) (nw 2^sw)
//
// With A = ||a'|| <= na 2^sa, W = ||w'|| <= nw 2^sw, sum |a' w'| <= A W and sum |x'| <= sqrt(128) ||x'||:
//   (2u + u^2) A W                                   the two conversions, relative part            2^-10 (1 + 2^-12)
//   gamma_128 A W                                    the exact chain's own roundings               2^-17 (1 + 2^-16)
//   128 * 2^-23 * 1.016 * (1 + u)^2 A W              the MFMAs' internal accumulation: 128 additions, each off by up to
//                                                    a whole ulp of the sum of |terms| (any order)  2^-16 * 1.017
//   = 2^-10 * 1.02395 A W, and the absolute terms
//   eta (1 + u) sqrt(128) (A + W) (1 + 2^-16)        conversions that land below fp16's normal range (or are flushed)
//   128 eta^2 (1 + 2^-16)                            both of a pair do
//   128 * 2^-126 * 2^(sa + sw) <= 2^-2               the chain's underflows, scaled (sa, sw <= 58)
// Because nw 2^sw >= 2^13, the W-proportional absolute term is at most 2^-10 * 0.708 (nw 2^sw), the A-proportional one
// 2^-10 * 2^-13.5 A (nw 2^sw), the two constants 2^-10 * 0.032 (nw 2^sw): an additive 0.74 on A, rounded up to
// PMH_NA_FLOOR = 1 (2^-13 of the tile's largest row: it only shows on rows far below that one), and 1.02404 in front.
// PMH_C = 2^-10 * 1.0625 leaves 3.7 % over that for the roundings of na 2^sa + 1, cw, S - E and S + E (2^-13 of E in
// all: |S| <= 2^10 E).
#pragma once
#include "pointmlp_screen_bound.h"

namespace pc3d {

constexpr float PMH_C = 0x1.1p-10f;
constexpr float PMH_NA_FLOOR = 1.0f;
constexpr int PMH_EXP = 13;
constexpr float PMH_CW_MAX = 0x1p5f;        // a valid channel's cw is below PMH_C * 2^14 < 2^5; +inf marks an invalid one

// n in [2^-45, 2^60] (a norm that passed pms_norm_ok): the exponent s with n 2^s in [2^PMH_EXP, 2^(PMH_EXP + 1)), and 2^s
PMS_HD inline int pmh_scale_exp(float n) { return PMH_EXP + 127 - (int)((__builtin_bit_cast(unsigned, n) >> 23) & 0xffu); }
PMS_HD inline float pmh_pow2(int s) { return __builtin_bit_cast(float, (unsigned)(s + 127) << 23); }   // -126 <= s <= 127
// the point's factor of E in the scaled domain (the products with 2^s are exact)
PMS_HD inline float pmh_na(float na, float two_sa) { return na * two_sa + PMH_NA_FLOOR; }
// the channel's factor of E in the scaled domain
PMS_HD inline float pmh_cw(float nw, float two_sw) { return PMH_C * (nw * two_sw); }
PMS_HD inline bool pmh_cw_ok(float cw) { return cw < PMH_CW_MAX; }     // false for NaN and +inf

}  // namespace pc3d
