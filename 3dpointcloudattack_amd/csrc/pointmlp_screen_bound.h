// The error bound of the PointNet tower's bf16 screen (pointmlp_screen.hip), in plain C++ so that the kernel, a host
// program and the numpy restatement (tests/pointmlp_screen_bound_restatement.py) state ONE formula. DESIGN §3.1 derives it.
//
//   v = the exact kernel's value: the fp32 fmaf chain over k of a_k w_k from +0
//   S = sum_k (ah_k wh_k + ah_k wl_k + al_k wh_k) with xh = bf16(x), xl = bf16(x - xh): three bf16 MFMA products per
//       k-step into one fp32 accumulator, in an order and with roundings nobody documents
//   |v - S| <= E = PMS_C * na * nw,   na = pms_norm_up(sum_k a_k^2),  nw = pms_norm_up(sum_k w_k^2)
//
// valid while na, nw <= PMS_NORM_MAX (no overflow anywhere: chain partial sums stay under 2^121, bf16 images stay
// finite); a tile or channel block outside that range, or with a non-finite norm, is not screened at all.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PMS_HD __host__ __device__
#else
#define PMS_HD
#endif

namespace pc3d {

// sqrt(sum of squares) computed in fp32 is low by at most (K + 2) * 2^-24 relative (K = 128 terms, any order, plus the
// root), and by at most sqrt(K) * 2^-63 absolute for squares that underflow: the factor and the floor cover both. The
// floor also keeps na * nw >= 2^-90, which is what lets the relative constant absorb every absolute term (flushed
// subnormal operands, terms, products and results: at most 2^-118 in all, plus 2^-76 na nw).
constexpr float PMS_NORM_INFLATE = 1.0f + 0x1p-15f;
constexpr float PMS_NORM_FLOOR = 0x1p-45f;
constexpr float PMS_NORM_MAX = 0x1p60f;

// needed, each times sum |a_k w_k| <= ||a|| ||w|| (Cauchy-Schwarz); bf16 keeps 8 significant bits, so rounding to
// nearest is 2^-8 relative, |xl| <= 2^-8 (1 + 2^-8) |x| and |x - xh - xl| <= 2^-16 |x|:
//   3 * 2^-16 (1 + 2^-7)   the dropped al wl and the two residuals                                   4.62e-5
//   2^-17 (1 + 2^-16)      gamma_128, the exact chain's own roundings                                0.76e-5
//   384 * 2^-23 * 1.016    allowed for the MFMAs' internal accumulation: 384 additions, each off by up to a whole
//                          ulp of the sum of |terms| (covers truncation as well as rounding, any order)  4.65e-5
// = 1.003e-4. PMS_C = 2^-13 = 1.2207e-4 leaves 21 % for the roundings of E, S - E and S + E and the absolute terms.
constexpr float PMS_C = 0x1p-13f;

PMS_HD inline float pms_norm_up(float sumsq) { return sqrtf(sumsq) * PMS_NORM_INFLATE + PMS_NORM_FLOOR; }
PMS_HD inline bool pms_norm_ok(float n) { return n <= PMS_NORM_MAX; }   // false for NaN and +inf
PMS_HD inline float pms_cw(float nw) { return PMS_C * nw; }             // the channel's factor of E
PMS_HD inline float pms_E(float na, float cw) { return na * cw; }
// lower / upper bound of v: one rounding each (monotonic, so pms_hi >= pms_lo for the same operands)
PMS_HD inline float pms_lo(float S, float na, float cw) { return __builtin_fmaf(-na, cw, S); }
PMS_HD inline float pms_hi(float S, float na, float cw) { return __builtin_fmaf(na, cw, S); }

}  // namespace pc3d
