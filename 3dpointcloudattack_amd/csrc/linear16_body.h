// The small-batch linear layer as a device function: linear16_kernel (head.hip) and the kernels that carry an
// independent piece of the attack iteration as extra workgroups of the same launch (linear_riders.hip) compile these
// statements. The workgroup's coordinates are arguments, not blockIdx. The tile (rows x outputs per workgroup) is a
// template parameter: 32 x 16, 16 x 16, 16 x 8 or 8 x 8 — every form computes the same bits (see linear16_body).
#pragma once
#include "pc3d_common.h"

namespace pc3d {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int LN_T = 512;  // threads: 8 waves split K
constexpr int LN_W = LN_T / 64;

struct LinArgs {
  const float* X;     // [B, P, K] (P partial slabs summed on load; P = 1 for a plain matrix)
  int ldx;            // row stride of X in floats (>= P*K)
  int P;
  const float* W;     // [O, K] row-major
  const float* bias;  // [O] or null
  const float* gate;  // [B, O] or null: Y = gate > 0 ? Y : gslope * Y  (the (Leaky)ReLU mask of a saved forward activation)
  int ldg;
  float* Y;           // [B, O]
  int ldy;
  int B, K, O;
  int relu;           // 1: Y = Y > 0 ? Y : slope * Y  (slope 0 = ReLU)
  float slope, gslope;
};

// pc3d_linear_f32 takes linear16_body, in one of its tile forms, for these shapes (everything else runs linear_kernel's
// 32 x 32 tiles)
static inline bool linear16_applies(int K, int P, int O) { return (K & 15) == 0 && P == 1 && K / 16 <= 8 * LN_W && O >= 64; }

// The tile forms by their numbers in the C entries (include/pc3d.h: PC3D_LIN_TILE_*); 0 there = the rule's choice
constexpr int kLinTileForms = 4;
static inline bool linear_tile_dims(int tile, int* tr, int* tc) {
  static const int dims[kLinTileForms][2] = {{32, 16}, {16, 16}, {16, 8}, {8, 8}};
  if (tile < 1 || tile > kLinTileForms) return false;
  *tr = dims[tile - 1][0], *tc = dims[tile - 1][1];
  return true;
}

// 32 rows x 16 outputs per workgroup on v_mfma_f32_16x16x4_f32: twice the workgroups (CUs) of the 32 x 32 tiling for
// the same layer, half the MFMA time and half the weight bytes per workgroup — these launches are latency-bound and
// use at most O/32 of the 256 CUs. Operand mapping: lane (r = lane & 15, q = lane >> 4) holds the float4 at
// k = 16c + 4q of row r; MFMA call e consumes element e of every lane's float4, so its four k-slices are
// k = 16c + 4q + e — the same permutation on both operands, i.e. an exact fp32 sum in a permuted k order.
// (bx, by) = (output tile, row tile) of this workgroup; all LN_T threads call it.
__device__ __forceinline__ void linear16_body_32x16(const LinArgs& a, int bx, int by) {
  __shared__ float red[LN_W][32][17];
  const int o0 = bx * 16, b0 = by * 32;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int xb0 = (b0 + r < a.B) ? b0 + r : a.B - 1;
  const int xb1 = (b0 + 16 + r < a.B) ? b0 + 16 + r : a.B - 1;
  const int wo = (o0 + r < a.O) ? o0 + r : a.O - 1;
  const float* x0 = a.X + (int64_t)xb0 * a.ldx + 4 * q;
  const float* x1 = a.X + (int64_t)xb1 * a.ldx + 4 * q;
  const float* wr = a.W + (int64_t)wo * a.K + 4 * q;
  const int nchunk = a.K / 16;          // chunks of 16 k; wave w takes chunks w, w+8, ... (<= 8 per wave)
  float4 xv0[8], xv1[8], wv[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = wave + i * LN_W;
    if (c < nchunk) {
      xv0[i] = *reinterpret_cast<const float4*>(x0 + 16 * c);
      xv1[i] = *reinterpret_cast<const float4*>(x1 + 16 * c);
      wv[i] = *reinterpret_cast<const float4*>(wr + 16 * c);
    }
  }
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = wave + i * LN_W;
    if (c < nchunk) {   // D[row = sample][col = output]; two independent accumulators cover the 40-cycle MFMA latency
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(xv0[i].x, wv[i].x, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(xv1[i].x, wv[i].x, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(xv0[i].y, wv[i].y, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(xv1[i].y, wv[i].y, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(xv0[i].z, wv[i].z, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(xv1[i].z, wv[i].z, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(xv0[i].w, wv[i].w, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(xv1[i].w, wv[i].w, acc1, 0, 0, 0);
    }
  }
  // 16x16x4 result layout: lane holds column r, rows 4*q + e
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    red[wave][4 * q + e][r] = acc0[e];
    red[wave][16 + 4 * q + e][r] = acc1[e];
  }
  __syncthreads();
  {
    const int row = threadIdx.x >> 4, col = threadIdx.x & 15;   // 512 threads = 32 x 16 outputs
    float s = red[0][row][col];
#pragma unroll
    for (int w = 1; w < LN_W; ++w) s += red[w][row][col];
    const int b = b0 + row, o = o0 + col;
    if (b < a.B && o < a.O) {
      if (a.bias) s += a.bias[o];
      if (a.relu) s = s > 0.f ? s : s * a.slope;
      if (a.gate && !(a.gate[(int64_t)b * a.ldg + o] > 0.f)) s *= a.gslope;
      a.Y[(int64_t)b * a.ldy + o] = s;
    }
  }
}

// TR <= 16 rows x TC <= 16 outputs per workgroup: the same operand mapping, k permutation and chunk -> wave assignment
// (c = wave + 8 i) with ONE accumulator per wave, so a layer spreads over 2-8 times the workgroups (CUs) and each pulls
// 4 K (TR + TC) bytes instead of 4 K 48. An output element depends only on its own row of X and its own row of W, and
// the epilogue adds the eight waves' partials in the same ascending order: the bits of the 32 x 16 form. Lanes whose
// row (r >= TR) or output (r >= TC) lies outside the tile issue no load and feed 0.0f; their products land in rows /
// columns of D that are never stored.
template <int TR, int TC>
__device__ __forceinline__ void linear16_body_small(const LinArgs& a, int bx, int by) {
  static_assert((TR == 16 || TR == 8) && (TC == 16 || TC == 8), "tile forms: 16 x 16, 16 x 8, 8 x 8");
  __shared__ float red[LN_W][TR][TC + 1];
  const int o0 = bx * TC, b0 = by * TR;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int xb = (b0 + r < a.B) ? b0 + r : a.B - 1;
  const int wo = (o0 + r < a.O) ? o0 + r : a.O - 1;
  const float* x0 = a.X + (int64_t)xb * a.ldx + 4 * q;
  const float* wr = a.W + (int64_t)wo * a.K + 4 * q;
  const bool xin = r < TR, win = r < TC;
  const int nchunk = a.K / 16;
  float4 xv[8], wv[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = wave + i * LN_W;
    xv[i] = make_float4(0.f, 0.f, 0.f, 0.f), wv[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < nchunk) {
      if (xin) xv[i] = *reinterpret_cast<const float4*>(x0 + 16 * c);
      if (win) wv[i] = *reinterpret_cast<const float4*>(wr + 16 * c);
    }
  }
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = wave + i * LN_W;
    if (c < nchunk) {
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[i].x, wv[i].x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[i].y, wv[i].y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[i].z, wv[i].z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[i].w, wv[i].w, acc, 0, 0, 0);
    }
  }
  // 16x16x4 result layout: lane holds column r, rows 4*q + e
  if (win && 4 * q < TR) {
#pragma unroll
    for (int e = 0; e < 4; ++e) red[wave][4 * q + e][r] = acc[e];
  }
  __syncthreads();
  if (threadIdx.x < TR * TC) {
    const int row = threadIdx.x / TC, col = threadIdx.x % TC;
    float s = red[0][row][col];
#pragma unroll
    for (int w = 1; w < LN_W; ++w) s += red[w][row][col];
    const int b = b0 + row, o = o0 + col;
    if (b < a.B && o < a.O) {
      if (a.bias) s += a.bias[o];
      if (a.relu) s = s > 0.f ? s : s * a.slope;
      if (a.gate && !(a.gate[(int64_t)b * a.ldg + o] > 0.f)) s *= a.gslope;
      a.Y[(int64_t)b * a.ldy + o] = s;
    }
  }
}

template <int TR, int TC>
__device__ __forceinline__ void linear16_body(const LinArgs& a, int bx, int by) {
  if constexpr (TR == 32) {
    static_assert(TC == 16, "tile forms: 32 x 16");
    linear16_body_32x16(a, bx, by);
  } else {
    linear16_body_small<TR, TC>(a, bx, by);
  }
}

// Expands the statement once per tile form with TR / TC as constants and runs the one numbered `tile` (1..kLinTileForms).
#define PC3D_LIN_TILE_SWITCH(tile, ...)                        \
  switch (tile) {                                              \
    case 1: { constexpr int TR = 32, TC = 16; __VA_ARGS__; } break;   \
    case 2: { constexpr int TR = 16, TC = 16; __VA_ARGS__; } break;   \
    case 3: { constexpr int TR = 16, TC = 8; __VA_ARGS__; } break;    \
    case 4: { constexpr int TR = 8, TC = 8; __VA_ARGS__; } break;     \
    default: break;                                            \
  }

// The tile the entries take when the caller passes 0: a pure function of the layer's shape (the table is stated in
// include/pc3d.h next to pc3d_linear_tile and was fixed from profiles/linear_tiles_bench.json).
// Measured (B = 32; K = 256, 512, 1024): above the 2.3 us launch floor a launch lasts 0.0305 us per KB that ONE workgroup
// pulls, 4 K (rows + outputs) bytes, however many workgroups there are — up to one per CU; the 8 x 8 form of 512 -> 1024
// (512 workgroups) is slower than its 16 x 8 form (256). So: the smallest tile that keeps the layer within 256
// workgroups. K < 256 was not measured and keeps 32 x 16, as does a layer that 32 x 16 itself puts past 256 workgroups.
static inline int linear_tile_rule(int B, int K, int O) {
  if (K < 256 || B < 1 || O < 1) return 1;
  for (int tile = kLinTileForms; tile > 1; --tile) {   // 8 x 8, 16 x 8, 16 x 16: ascending bytes per workgroup
    int tr = 32, tc = 16;
    linear_tile_dims(tile, &tr, &tc);
    if ((int64_t)cdiv(O, tc) * cdiv(B, tr) <= 256) return tile;
  }
  return 1;
}

// tile argument of an entry -> form number (0 = the rule), or 0 for a number that names no form
static inline int linear_tile_pick(int tile, int B, int K, int O) {
  if (tile == 0) return linear_tile_rule(B, K, O);
  return (tile >= 1 && tile <= kLinTileForms) ? tile : 0;
}

}  // namespace pc3d
