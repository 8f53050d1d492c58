// Device code shared by the PointNet tower kernels (pointmlp.hip, pointmlp_ft.hip): tile constants, the point load
// with the 3 x 3 input transform, and layer 1 (3 -> 64, ReLU) into LDS with its decision masks.
#pragma once
#include "pc3d_common.h"

namespace pc3d {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int PM_C1 = 64;
constexpr int PM_C2 = 128;
constexpr int PM_TP = 128;           // forward: points per workgroup
constexpr int PM_LD1 = PM_C1 + 4;    // LDS row strides (floats): +4 keeps ds_read_b128 conflict-free
constexpr int PM_LD2 = PM_C2 + 4;
constexpr int PM_BTP = 32;           // backward: points per workgroup
constexpr int PM_MAXC3 = 1024;       // backward: widest pooled layer held in LDS

// T: the 3 x 3 transform of THIS cloud (or null)
__device__ __forceinline__ void load_point(const PtsView& x, const float* T, int b, int n, int N, float& px,
                                           float& py, float& pz) {
  px = py = pz = 0.f;
  if (n < N) {
    const float* p = x.p + (int64_t)b * x.bs + (int64_t)n * x.ps;
    const float x0 = p[0], x1 = p[x.cs], x2 = p[2 * x.cs];
    if (T) {
      const float* t = T;
      px = __builtin_fmaf(x2, t[6], __builtin_fmaf(x1, t[3], x0 * t[0]));
      py = __builtin_fmaf(x2, t[7], __builtin_fmaf(x1, t[4], x0 * t[1]));
      pz = __builtin_fmaf(x2, t[8], __builtin_fmaf(x1, t[5], x0 * t[2]));
    } else {
      px = x0, py = x1, pz = x2;
    }
  }
}

// h1[p][c] = relu(W1[c,:].x_p + b1[c]) for `npts` points whose coordinates sit in xs[3][npts]; lanes run over c.
// m1 (may be null) receives, for point p, the 64-bit mask of its positive channels: the wave's lanes ARE the 64
// channels, so the mask is one ballot; lane i keeps point i's mask and the wave stores `per` consecutive words.
template <int NPTS, int NTHREADS>
__device__ __forceinline__ void layer1_to_lds(const float* xs, float* h1, const float* W1, const float* b1,
                                              uint64_t* m1 = nullptr, int nvalid = NPTS) {
  const int c = threadIdx.x & (PM_C1 - 1);
  const int grp = threadIdx.x >> 6;
  constexpr int per = NPTS / (NTHREADS / 64);
  static_assert(per <= 64, "one mask word per lane");
  const float w0 = W1[c * 3 + 0], w1 = W1[c * 3 + 1], w2 = W1[c * 3 + 2], bb = b1[c];
  unsigned long long mine = 0ull;
#pragma unroll 4
  for (int i = 0; i < per; ++i) {
    const int p = grp * per + i;
    float v = __builtin_fmaf(w2, xs[2 * NPTS + p], __builtin_fmaf(w1, xs[NPTS + p], __builtin_fmaf(w0, xs[p], bb)));
    h1[p * PM_LD1 + c] = fmaxf(v, 0.f);
    const unsigned long long bal = __builtin_amdgcn_ballot_w64(v > 0.f);
    if (c == i) mine = bal;
  }
  if (m1 != nullptr && c < per && grp * per + c < nvalid) m1[grp * per + c] = mine;
}

constexpr int PM_MAXC3F = 1024;      // forward: widest layer 3 (cross-wave max scratch aliases the h2 tile)
constexpr int PM_FT = 512;           // forward: threads per workgroup (8 waves = 2 per SIMD: one wave's epilogue /
                                     // operand waits overlap the other's MFMAs)

}  // namespace pc3d
