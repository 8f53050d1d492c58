// Shared device bodies of the isometry attack's kernels (iso.hip): the 3x3 product of one point and the weight-gradient
// reduction of one cloud. pc3d_iso_wgrad_f32 and the fused pc3d_iso_update_f32 both run iso_wgrad_block, and the update's
// epilogue and pc3d_iso_apply_f32 both run iso_mat3, so the fused launch produces the same bits as the separate ones.
#pragma once
#include "pc3d_common.h"

namespace pc3d {

constexpr int ISO_T = 256;             // threads per workgroup of every kernel in iso.hip
constexpr int ISO_WAVES = ISO_T / kWave;

// y = W x (transpose = 0) or W^T x (transpose != 0), W row-major [9]. One product and two fused multiply-adds per row.
__device__ __forceinline__ void iso_mat3(const float* __restrict__ w, int transpose, float x0, float x1, float x2, float* y) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float w0 = transpose ? w[a] : w[3 * a], w1 = transpose ? w[3 + a] : w[3 * a + 1],
                w2 = transpose ? w[6 + a] : w[3 * a + 2];
    y[a] = __builtin_fmaf(w2, x2, __builtin_fmaf(w1, x1, w0 * x0));
  }
}

// s_out[3 a + c] = sum_n g[a, n] * x[c, n] over the N points of ONE cloud (g, x: views already moved to that cloud; bs unused).
// The order is fixed by ISO_T alone: thread t adds n = t, t + ISO_T, ... in ascending order, the 64 lanes of a wave fold
// in a xor tree, and the ISO_WAVES wave sums are added in wave order — it depends on neither the batch nor the number of
// matrices per cloud, and no atomics are involved. Every thread of the workgroup must call; s_out is valid for all after.
__device__ __forceinline__ void iso_wgrad_block(const float* __restrict__ g, int64_t g_ps, int64_t g_cs,
                                                const float* __restrict__ x, int64_t x_ps, int64_t x_cs, int N,
                                                float (*s_part)[9], float* s_out) {
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  float acc[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) acc[k] = 0.f;
  for (int n = tid; n < N; n += ISO_T) {
    const float* gp = g + (int64_t)n * g_ps;
    const float* xp = x + (int64_t)n * x_ps;
    const float gv[3] = {gp[0], gp[g_cs], gp[2 * g_cs]};
    const float xv[3] = {xp[0], xp[x_cs], xp[2 * x_cs]};
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[3 * a + c] = __builtin_fmaf(gv[a], xv[c], acc[3 * a + c]);
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) acc[k] = wave_sum(acc[k]);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 9; ++k) s_part[wave][k] = acc[k];
  }
  __syncthreads();
  if (tid < 9) {
    float s = s_part[0][tid];
#pragma unroll
    for (int w = 1; w < ISO_WAVES; ++w) s += s_part[w][tid];
    s_out[tid] = s;
  }
  __syncthreads();
}

}  // namespace pc3d
