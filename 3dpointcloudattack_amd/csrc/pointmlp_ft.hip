// K8-FT — the PointNet towers of a victim built with feature_transform=True (model/pointnet.py:51-87, :101-117).
// gfx950, fp32-input MFMA (exact fp32 FMA chains), eval mode with BatchNorm folded.
//
//   x' = T3^T x,  h = relu(W1 x' + b1)                                        [64, N]
//   Tf = I + head(max_n relu-tower_{64->64->128->1024}(h))                    [64, 64]   (STNkd)
//   pooled = max_n (W3 relu(W2 Tf^T h + b2) + b3)
//
// Two forward towers share one kernel template (the layer-3 main loop is pointmlp3_max_fwd_kernel's, see pointmlp.hip):
//   EXTRA = true   STNkd's tower 3 -> 64 -> [64 -> 64] -> 128 -> 1024: h is recomputed from x (192 FMAs per point) and
//                  the extra 64 x 64 layer runs on MFMA in place in LDS, between layers 1 and 2;
//   EXTRA = false  the trunk with a PER-CLOUD layer-2 weight W2_b = W2 Tf_b^T (ft_fold_w2_kernel), which replaces the
//                  per-point 64 x 64 product u = Tf^T h.
// Neither writes a per-point activation: the ReLU decisions leave as bit masks, (max, argmax) per tile.
//
// Backward (winners only, as pointmlp3_max_bwd_twolist_kernel): the tile's hits are gathered in ascending channel
// order, the masked layers are chained on MFMA. The trunk form also emits q[n, j] = (W2^T g_z2)[j, n], from which
// ft_dtf_kernel forms dL/dTf[i, j] = sum_n h[i, n] q[n, j] in ascending n: a fixed order, no float atomics.
#include <stdlib.h>
#include "pc3d_common.h"
#include "pointmlp_body.h"

namespace pc3d {

struct FTFwdArgs {
  PtsView x;
  int N, C3, ntiles;
  const float* T;             // [B,3,3]: x'[n,:] = x[n,:] @ T
  const float *W1, *b1;       // [64,3]
  const float *WA, *bA;       // EXTRA: [64,64]
  const float* W2;            // [128,64], cloud b's at W2 + b * w2_bs
  int64_t w2_bs;
  const float *b2, *W3, *b3;
  float* part_val;            // [B, ntiles, C3]
  int32_t* part_idx;          // [B, ntiles, C3]
  uint64_t* mask1;            // [B,N]    bit c = (h channel c of the point > 0)
  uint64_t* maskA;            // [B,N]    EXTRA: bit c = (output c of the 64 -> 64 layer > 0)
  uint32_t* mask2;            // [B,N,4]  word j bit r = (128-wide layer's output 32j + r > 0)
};

template <bool EXTRA>
__global__ __launch_bounds__(PM_FT) __attribute__((amdgpu_waves_per_eu(2, 2))) void ft_tower_fwd_kernel(FTFwdArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[PM_TP * PM_LD2 + 3 * PM_TP];  // 69,120 B static
  float* h1 = lds;                       // [128][68]   (dead after layer 2)
  float* h2 = lds;                       // [128][132]  (overwrites h1 behind a barrier)
  float* xs = lds + PM_TP * PM_LD2;      // [3][128]
  const int tile = blockIdx.x, b = blockIdx.y;
  const int n0 = tile * PM_TP;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;

  if (threadIdx.x < PM_TP) {
    float px, py, pz;
    load_point(a.x, a.T + (int64_t)b * 9, b, n0 + threadIdx.x, a.N, px, py, pz);
    xs[threadIdx.x] = px;
    xs[PM_TP + threadIdx.x] = py;
    xs[2 * PM_TP + threadIdx.x] = pz;
  }
  __syncthreads();
  layer1_to_lds<PM_TP, PM_FT>(xs, h1, a.W1, a.b1, a.mask1 + (int64_t)b * a.N + n0, a.N - n0);
  __syncthreads();

  if (EXTRA) {
    // ---- the 64 -> 64 layer on MFMA, in place: wave owns channel block (wave & 1) of point tile (wave >> 1)
    const int cb = wave & 1, tl = wave >> 1;
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    const float* wrow = a.WA + (32 * cb + r) * PM_C1 + 4 * h;
    const float* arow = h1 + (tl * 32 + r) * PM_LD1 + 4 * h;
#pragma unroll
    for (int t = 0; t < PM_C1 / 8; ++t) {
      const float4 bw = *reinterpret_cast<const float4*>(wrow + 8 * t);
      const float4 av = *reinterpret_cast<const float4*>(arow + 8 * t);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bw.x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bw.y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bw.z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bw.w, acc, 0, 0, 0);
    }
    __syncthreads();  // every wave is done reading h1
    const float bias = a.bA[32 * cb + r];
    unsigned long long mine = 0ull;   // lane e keeps the ballot of accumulator row e: points pt(e,0) [low word], pt(e,1) [high]
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int pt = tl * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
      const float v = acc[e] + bias;
      h1[pt * PM_LD1 + 32 * cb + r] = fmaxf(v, 0.f);
      const unsigned long long bal = __builtin_amdgcn_ballot_w64(v > 0.f);
      if (lane == e) mine = bal;
    }
    if (lane < 16) {   // the 64-bit mask of a point is two 32-bit words: word cb belongs to this wave
      const int pt0 = n0 + tl * 32 + (lane & 3) + 8 * (lane >> 2);
      uint32_t* mA = reinterpret_cast<uint32_t*>(a.maskA) + ((int64_t)b * a.N) * 2 + cb;
      if (pt0 < a.N) mA[(int64_t)pt0 * 2] = (uint32_t)mine;
      if (pt0 + 4 < a.N) mA[(int64_t)(pt0 + 4) * 2] = (uint32_t)(mine >> 32);
    }
    __syncthreads();
  }

  // ---- layer 2 on MFMA: D[pt][c2] = sum_k h1[pt][k] W2_b[c2][k]; wave owns c2 block (wave&3) and 2 of the 4 point tiles
  {
    const float* W2 = a.W2 + (int64_t)b * a.w2_bs;
    const int c2b = wave & 3, tl0 = (wave >> 2) * 2;
    f32x16 acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
    const float* wrow = W2 + (32 * c2b + r) * PM_C1 + 4 * h;
#pragma unroll
    for (int t = 0; t < PM_C1 / 8; ++t) {
      const float4 bw = *reinterpret_cast<const float4*>(wrow + 8 * t);
      float4 av[2];
#pragma unroll
      for (int tl = 0; tl < 2; ++tl)
        av[tl] = *reinterpret_cast<const float4*>(h1 + ((tl0 + tl) * 32 + r) * PM_LD1 + 8 * t + 4 * h);
#pragma unroll
      for (int tl = 0; tl < 2; ++tl) {
        acc[tl] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[tl].x, bw.x, acc[tl], 0, 0, 0);
        acc[tl] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[tl].y, bw.y, acc[tl], 0, 0, 0);
        acc[tl] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[tl].z, bw.z, acc[tl], 0, 0, 0);
        acc[tl] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[tl].w, bw.w, acc[tl], 0, 0, 0);
      }
    }
    __syncthreads();  // every wave is done reading h1
    const float bias = a.b2[32 * c2b + r];
    unsigned long long mine = 0ull;   // lane 16*tl + e keeps the ballot of (tl, e)
#pragma unroll
    for (int tl = 0; tl < 2; ++tl)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int pt = (tl0 + tl) * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
        const float v = acc[tl][e] + bias;
        h2[pt * PM_LD2 + 32 * c2b + r] = fmaxf(v, 0.f);
        const unsigned long long bal = __builtin_amdgcn_ballot_w64(v > 0.f);
        if (lane == 16 * tl + e) mine = bal;
      }
    if (lane < 32) {
      const int tl = lane >> 4, e = lane & 15;
      const int pt0 = n0 + (tl0 + tl) * 32 + (e & 3) + 8 * (e >> 2);
      uint32_t* m2 = a.mask2 + ((int64_t)b * a.N) * 4 + c2b;
      if (pt0 < a.N) m2[(int64_t)pt0 * 4] = (uint32_t)mine;
      if (pt0 + 4 < a.N) m2[(int64_t)(pt0 + 4) * 4] = (uint32_t)(mine >> 32);
    }
  }
  __syncthreads();

  // ---- layer 3 + max over the tile's points: pointmlp3_max_fwd_kernel's main loop (points on the MFMA rows, channels
  // on the lanes, A operands held in 64 VGPRs, W3 double-buffered in registers across channel blocks, in-register max)
  const int ptile = wave & 3, cgrp = wave >> 2;
  float4 areg[PM_C2 / 8];
#pragma unroll
  for (int t = 0; t < PM_C2 / 8; ++t)
    areg[t] = *reinterpret_cast<const float4*>(h2 + (ptile * 32 + r) * PM_LD2 + 8 * t + 4 * h);
  __syncthreads();  // h2 fully consumed into registers: the LDS region is reused for the cross-wave max below
  float* pv = lds;                                        // [4 point tiles][C3]
  int* pi = reinterpret_cast<int*>(lds + 4 * PM_MAXC3F);  // [4 point tiles][C3]
  const int nblk = a.C3 / 32;
  const int blk_per_grp = (nblk + 1) / 2;
  const int cb_end = (cgrp + 1) * blk_per_grp < nblk ? (cgrp + 1) * blk_per_grp : nblk;
  auto load_row = [&](float4 (&dst)[PM_C2 / 8], int cb) {
    const int cbc = cb < cb_end ? cb : cb_end - 1;
    const float* wrow = a.W3 + (int64_t)(cbc * 32 + r) * PM_C2 + 4 * h;
#pragma unroll
    for (int t = 0; t < PM_C2 / 8; ++t) dst[t] = *reinterpret_cast<const float4*>(wrow + 8 * t);
  };
  auto run_block = [&](const float4 (&cur)[PM_C2 / 8], float4 (&nxt)[PM_C2 / 8], int cb) {
    const int cbn = (cb + 1 < cb_end) ? cb + 1 : cb_end - 1;
    const float* nrow = a.W3 + (int64_t)(cbn * 32 + r) * PM_C2 + 4 * h;
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
    for (int t = 0; t < PM_C2 / 8; ++t) {
      nxt[t] = *reinterpret_cast<const float4*>(nrow + 8 * t);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(areg[t].x, cur[t].x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(areg[t].y, cur[t].y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(areg[t].z, cur[t].z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(areg[t].w, cur[t].w, acc, 0, 0, 0);
      __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);  // 1 VMEM read
      __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);  // 4 MFMA
    }
    const int ch = cb * 32 + r;
    float best = -__builtin_inff();
    int be = 0;
    const int base = n0 + ptile * 32;
    if (base + 32 <= a.N) {             // (uniform)
#pragma unroll
      for (int e = 0; e < 16; ++e)      // ascending point index in e for fixed h: strict > keeps the lowest
        if (acc[e] > best) best = acc[e], be = (e & 3) + 8 * (e >> 2);
    } else {
#pragma unroll
      for (int e = 0; e < 16; ++e)
        if (base + (e & 3) + 8 * (e >> 2) + 4 * h < a.N && acc[e] > best) best = acc[e], be = (e & 3) + 8 * (e >> 2);
    }
    int bi = best == -__builtin_inff() ? base : base + be + 4 * h;
    argmax_xor32(best, bi);
    if (h == 0) {
      pv[ptile * a.C3 + ch] = best;
      pi[ptile * a.C3 + ch] = bi;
    }
  };
  float4 bwA[PM_C2 / 8], bwB[PM_C2 / 8];
  const int cb_begin = cgrp * blk_per_grp;
  if (cb_begin < cb_end) {
    load_row(bwA, cb_begin);
    for (int cb = cb_begin; cb < cb_end; cb += 2) {
      run_block(bwA, bwB, cb);
      if (cb + 1 < cb_end) run_block(bwB, bwA, cb + 1);
    }
  }
  __syncthreads();
  for (int ch = threadIdx.x; ch < a.C3; ch += PM_FT) {
    float best = pv[ch];
    int bi = pi[ch];
#pragma unroll
    for (int t = 1; t < 4; ++t) {  // ascending point tile: strict > keeps the lowest point index on ties
      const float v = pv[t * a.C3 + ch];
      if (v > best) {
        best = v;
        bi = pi[t * a.C3 + ch];
      }
    }
    const int64_t o = ((int64_t)b * a.ntiles + tile) * a.C3 + ch;
    a.part_val[o] = best + a.b3[ch];
    a.part_idx[o] = bi;
  }
}

// W2_b[c][i] = sum_j W2[c][j] Tf_b[i][j]  (= W2 Tf_b^T): workgroup = (32 rows c, cloud b), ascending j.
__global__ __launch_bounds__(256) void ft_fold_w2_kernel(const float* W2, const float* Tf, float* out) {
  __shared__ float tf[PM_C1 * (PM_C1 + 1)];
  __shared__ float ws[32 * PM_C1];
  const int b = blockIdx.y, c0 = blockIdx.x * 32;
  const float* t = Tf + (int64_t)b * PM_C1 * PM_C1;
  for (int i = threadIdx.x; i < PM_C1 * PM_C1; i += 256) tf[(i >> 6) * (PM_C1 + 1) + (i & 63)] = t[i];
  for (int i = threadIdx.x; i < 32 * PM_C1; i += 256) ws[i] = W2[c0 * PM_C1 + i];
  __syncthreads();
  const int i = threadIdx.x & 63, cg = threadIdx.x >> 6;
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  for (int j = 0; j < PM_C1; ++j) {
    const float tv = tf[i * (PM_C1 + 1) + j];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = __builtin_fmaf(ws[(cg * 8 + e) * PM_C1 + j], tv, acc[e]);
  }
  float* o = out + ((int64_t)b * PM_C2 + c0) * PM_C1;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[(cg * 8 + e) * PM_C1 + i] = acc[e];
}

// ---------------------------------------------------------------------------------------------------------
struct FTBwdArgs {
  PtsView x;
  int N, C3;
  const float* T;         // [B,3,3]
  const float* W1;        // [64,3]
  const float* WA;        // EXTRA: [64,64]
  const float* W2;        // [128,64], cloud b's at W2 + b * w2_bs
  int64_t w2_bs;
  const float* W2q;       // trunk: the UNfolded W2 (q = g_z2 . W2) or null
  const float* W3;
  const int32_t* argidx;  // [B,C3]
  const uint64_t* mask1;  // [B,N]
  const uint64_t* maskA;  // [B,N]   EXTRA
  const uint32_t* mask2;  // [B,N,4]
  const float* g;         // [B,C3] upstream gradient on pooled (already masked for a ReLU after the pool)
  PtsViewMut gx;          // gradient wrt the RAW points x
  float* part_gT;         // [B, gT_tiles, 16]: this launch writes rows gT_off + tile
  int gT_tiles, gT_off;
  float* q;               // [B,N,64] or null
  int accumulate;
};

// acc[pt][col] = sum_k A[pt][k] W[k][col] over the NT*8 values of k this wave owns; w holds the lane's B operands
template <int NT>
__device__ __forceinline__ f32x16 ft_chain(const float4 (&w)[NT], const float* arow) {
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const float4 av = *reinterpret_cast<const float4*>(arow + 8 * t);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, w[t].x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, w[t].y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, w[t].z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, w[t].w, acc, 0, 0, 0);
  }
  return acc;
}
// the lane's B operands of ft_chain from a row-major W [K][64]: rows k0 + 8t + {0..3}, column col
template <int NT>
__device__ __forceinline__ void ft_load_cols(float4 (&w)[NT], const float* W, int k0, int col) {
  const float* wcol = W + (int64_t)k0 * PM_C1 + col;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    w[t].x = wcol[(8 * t + 0) * PM_C1];
    w[t].y = wcol[(8 * t + 1) * PM_C1];
    w[t].z = wcol[(8 * t + 2) * PM_C1];
    w[t].w = wcol[(8 * t + 3) * PM_C1];
  }
}

// Workgroup = (batch b, 32 points), 4 waves. Phase A is pointmlp3_max_bwd_twolist_kernel's ordered gather, summed in runs.
// T == null: a tower on the raw points (STN3d's): no transform chain, no dL/dT partials.
constexpr int FT_RUN = 32;           // longest register run of the gather
template <bool EXTRA>
__global__ __launch_bounds__(256) void ft_tower_bwd_kernel(FTBwdArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[PM_BTP * PM_LD2 + PM_BTP * PM_LD1 + 4 * PM_BTP + PM_MAXC3 + (3 * PM_MAXC3) / 2];  // 36.4 KB
  float* g2s = lds;                                   // [32][132]
  float* h1s = g2s + PM_BTP * PM_LD2;                 // [32][68]
  float* xs = h1s + PM_BTP * PM_LD1;                  // [3][32]    scratch of phase D
  int* s_scan = reinterpret_cast<int*>(xs + 3 * PM_BTP);   // [32] wave totals
  float* s_g = xs + 4 * PM_BTP;                       // [C3]
  short* s_n = reinterpret_cast<short*>(s_g + PM_MAXC3);   // [C3] local point index or -1
  short* list0 = s_n + PM_MAXC3;                      // [C3] channels hitting points 0..15, ascending
  short* list1 = list0 + PM_MAXC3;                    // [C3] channels hitting points 16..31
  __shared__ uint32_t s_m2[PM_BTP][4];
  __shared__ uint64_t s_m1[PM_BTP], s_mA[PM_BTP];
  const int tile = blockIdx.x, b = blockIdx.y;
  const int n0 = tile * PM_BTP;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int jb = wave & 1, kh = wave >> 1;
  float* part_gT = a.T ? a.part_gT + ((int64_t)b * a.gT_tiles + a.gT_off + tile) * 16 : nullptr;

  // ---- A1. classify 4 consecutive channels per thread, block-wide ordered compaction (small loads first)
  int ld_n[PM_MAXC3 / 256];
  float ld_g[PM_MAXC3 / 256];
#pragma unroll
  for (int e = 0; e < PM_MAXC3 / 256; ++e) {
    const int c = tid * (PM_MAXC3 / 256) + e;
    ld_n[e] = (c < a.C3) ? a.argidx[(int64_t)b * a.C3 + c] : -1;
    ld_g[e] = (c < a.C3) ? a.g[(int64_t)b * a.C3 + c] : 0.f;
  }
  uint32_t ld_m2 = 0u;
  uint64_t ld_m1 = 0ull, ld_mA = 0ull;
  if (tid < PM_BTP * 4 && n0 + (tid >> 2) < a.N) ld_m2 = a.mask2[((int64_t)b * a.N + n0) * 4 + tid];
  if (tid < PM_BTP && n0 + tid < a.N) {
    ld_m1 = a.mask1[(int64_t)b * a.N + n0 + tid];
    if (EXTRA) ld_mA = a.maskA[(int64_t)b * a.N + n0 + tid];
  }
  // the MFMA B operands depend on nothing: fetched now, their L2 latency hides under phase A
  float4 w2tr[PM_C2 / 16];
  ft_load_cols(w2tr, a.W2 + (int64_t)b * a.w2_bs, 64 * kh + 4 * h, 32 * jb + r);
  int cnt0 = 0, cnt1 = 0;
  int myn[PM_MAXC3 / 256];
#pragma unroll
  for (int e = 0; e < PM_MAXC3 / 256; ++e) {
    const int c = tid * (PM_MAXC3 / 256) + e;
    int n = -1;
    if (c < a.C3) {
      n = ld_n[e] - n0;
      const float gv = ld_g[e];
      if (n < 0 || n >= PM_BTP || gv == 0.f) n = -1;
      s_g[c] = gv;
      s_n[c] = (short)n;
    }
    myn[e] = n;
    cnt0 += (n >= 0 && n < 16) ? 1 : 0;
    cnt1 += (n >= 16) ? 1 : 0;
  }
  if (tid < PM_BTP * 4) s_m2[tid >> 2][tid & 3] = ld_m2;
  if (tid < PM_BTP) s_m1[tid] = ld_m1, s_mA[tid] = ld_mA;
  for (int i = tid; i < PM_BTP * PM_LD2; i += 256) g2s[i] = 0.f;
  int packed = cnt0 | (cnt1 << 16);
  const int incl = wave_incl_scan(packed, lane);
  if (lane == 63) s_scan[wave] = incl;
  __syncthreads();
  int base = 0, total = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const int v = s_scan[w];
    if (w < wave) base += v;
    total += v;
  }
  const int len0 = total & 0xffff, len1 = total >> 16;
  if (len0 + len1 == 0) {  // no critical point in this tile: every gradient it owns is exactly zero
    if (tid < 3 * PM_BTP && !a.accumulate) {
      const int p = tid & (PM_BTP - 1), c = tid >> 5;
      if (n0 + p < a.N) a.gx.p[(int64_t)b * a.gx.bs + (int64_t)(n0 + p) * a.gx.ps + c * a.gx.cs] = 0.f;
    }
    if (part_gT && tid < 16) part_gT[tid] = 0.f;
    if (a.q) {
      for (int i = tid; i < PM_BTP * PM_C1; i += 256)
        if (n0 + (i >> 6) < a.N) a.q[((int64_t)b * a.N + n0) * PM_C1 + i] = 0.f;
    }
    return;
  }
  {
    const int excl = base + incl - packed;
    int o0 = excl & 0xffff, o1 = excl >> 16;
#pragma unroll
    for (int e = 0; e < PM_MAXC3 / 256; ++e) {
      const int n = myn[e];
      const int c = tid * (PM_MAXC3 / 256) + e;
      if (n >= 0 && n < 16) list0[o0++] = (short)c;
      if (n >= 16) list1[o1++] = (short)c;
    }
  }
  __syncthreads();

  // ---- A2. ordered accumulation: thread (k, half) walks its half's list in ascending channel order. A run of entries
  // that hit the same point is summed in a register and added to the point's row once per run, and a run is cut after
  // FT_RUN entries: a point that wins hundreds of channels (all 1024 when the cloud has one point) is then summed in
  // blocks like a GEMM sums it, not as one chain whose rounding error grows with its length (measured on 1024 terms:
  // 6.3e-7 relative L2 as one chain, 1.6e-7 in blocks of 32). The list is shared by the half, so the cuts are uniform.
  {
    const int k = tid & (PM_C2 - 1), ph = tid >> 7;
    const short* list = ph ? list1 : list0;
    const int len = ph ? len1 : len0;
    float racc = 0.f;
    int cur = -1, run = 0;
    auto add = [&](int c, float w) {
      const int n = s_n[c];
      if (n != cur || run == FT_RUN) {
        if (cur >= 0) g2s[cur * PM_LD2 + k] += racc;
        racc = 0.f, cur = n, run = 0;
      }
      racc = __builtin_fmaf(s_g[c], w, racc);
      ++run;
    };
    int i = 0;
    for (; i + 8 <= len; i += 8) {  // 8 independent W3 loads in flight per round trip
      int c[8];
      float w[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        c[e] = list[i + e];
        w[e] = a.W3[(int64_t)c[e] * PM_C2 + k];
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) add(c[e], w[e]);
    }
    for (; i < len; ++i) {
      const int c = list[i];
      add(c, a.W3[(int64_t)c * PM_C2 + k]);
    }
    if (cur >= 0) g2s[cur * PM_LD2 + k] += racc;
    // the 128-wide layer's ReLU: this thread is the only writer of column k for its half's 16 points
#pragma unroll
    for (int p = 0; p < 16; ++p) {
      const int pt = 16 * ph + p;
      if (!((s_m2[pt][k >> 5] >> (k & 31)) & 1u)) g2s[pt * PM_LD2 + k] = 0.f;
    }
  }
  __syncthreads();

  // ---- C. g1[pt][j] = sum_k2 g2[pt][k2] W2_b[k2][j] on MFMA: wave = (j block jb, K half kh); the upper K half hands
  // its partial tile to the lower one through LDS (fixed order). The trunk forms q = g2 . W2 (unfolded) beside it.
  {
    const float* arow = g2s + r * PM_LD2 + 64 * kh + 4 * h;
    f32x16 acc = ft_chain(w2tr, arow), accq;
    const bool with_q = !EXTRA && a.q != nullptr;   // (uniform)
    if (with_q) {
      float4 wq[PM_C2 / 16];
      ft_load_cols(wq, a.W2q, 64 * kh + 4 * h, 32 * jb + r);
      accq = ft_chain(wq, arow);
    }
    __syncthreads();   // g2s is dead once every wave has read its A operands: it doubles as the exchange buffer
    float* cr = g2s + jb * (32 * 33);
    float* crq = g2s + (2 + jb) * (32 * 33);
    if (kh == 1) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int pt = (e & 3) + 8 * (e >> 2) + 4 * h;
        cr[pt * 33 + r] = acc[e];
        if (with_q) crq[pt * 33 + r] = accq[e];
      }
    }
    __syncthreads();
    if (kh == 0) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int pt = (e & 3) + 8 * (e >> 2) + 4 * h;
        const bool on = ((EXTRA ? s_mA[pt] : s_m1[pt]) >> (32 * jb + r)) & 1ull;
        h1s[pt * PM_LD1 + 32 * jb + r] = on ? (acc[e] + cr[pt * 33 + r]) : 0.f;
        if (with_q && n0 + pt < a.N)
          a.q[((int64_t)b * a.N + n0 + pt) * PM_C1 + 32 * jb + r] = accq[e] + crq[pt * 33 + r];
      }
    }
    __syncthreads();
  }
  if (EXTRA) {
    // ---- C'. the 64 -> 64 layer: g1[pt][j] = sum_k gA[pt][k] WA[k][j], K halves of 32, masked by h's ReLU
    float4 wa[PM_C1 / 16];
    ft_load_cols(wa, a.WA, 32 * kh + 4 * h, 32 * jb + r);
    f32x16 acc = ft_chain(wa, h1s + r * PM_LD1 + 32 * kh + 4 * h);
    __syncthreads();   // every wave has read its A operands from h1s
    float* cr = g2s + jb * (32 * 33);
    if (kh == 1) {
#pragma unroll
      for (int e = 0; e < 16; ++e) cr[((e & 3) + 8 * (e >> 2) + 4 * h) * 33 + r] = acc[e];
    }
    __syncthreads();
    if (kh == 0) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int pt = (e & 3) + 8 * (e >> 2) + 4 * h;
        const bool on = (s_m1[pt] >> (32 * jb + r)) & 1ull;
        h1s[pt * PM_LD1 + 32 * jb + r] = on ? (acc[e] + cr[pt * 33 + r]) : 0.f;
      }
    }
    __syncthreads();
  }

  // ---- D. g'[p][c] = sum_j W1[j][c] g1[p][j]  (gradient wrt x' = x @ T)
  float* gp = xs;  // [3][32] scratch
  if (wave < 3 && lane < PM_BTP) {   // wave = coordinate c (uniform), lane = point
    const int p = lane, c = wave;
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int j = 0; j < PM_C1; j += 4) {
      const float4 hv = *reinterpret_cast<const float4*>(h1s + p * PM_LD1 + j);
      s0 = __builtin_fmaf(a.W1[j * 3 + c], hv.x, s0);
      s1 = __builtin_fmaf(a.W1[(j + 1) * 3 + c], hv.y, s1);
      s0 = __builtin_fmaf(a.W1[(j + 2) * 3 + c], hv.z, s0);
      s1 = __builtin_fmaf(a.W1[(j + 3) * 3 + c], hv.w, s1);
    }
    gp[c * PM_BTP + p] = s0 + s1;
  }
  __syncthreads();
  if (wave == 0) {  // lanes 0..31 = the tile's points; lanes 32..63 contribute zeros to the reductions
    const int p = lane & (PM_BTP - 1);
    const bool live = lane < PM_BTP;
    const float g0 = live ? gp[p] : 0.f, g1v = live ? gp[PM_BTP + p] : 0.f, g2v = live ? gp[2 * PM_BTP + p] : 0.f;
    float o0 = g0, o1 = g1v, o2 = g2v;
    if (a.T) {
      // x' = x @ T  =>  dL/dx[c] = sum_c' g'[c'] T[c][c'] ;  dL/dT[c][c'] = sum_p x[p][c] g'[p][c']
      // (the chain starts from +0, so a dead point, g' = +0, gets +0 and not -0 under a row of negative T entries)
      const float* t = a.T + (int64_t)b * 9;
      o0 = __builtin_fmaf(g2v, t[2], __builtin_fmaf(g1v, t[1], __builtin_fmaf(g0, t[0], 0.f)));
      o1 = __builtin_fmaf(g2v, t[5], __builtin_fmaf(g1v, t[4], __builtin_fmaf(g0, t[3], 0.f)));
      o2 = __builtin_fmaf(g2v, t[8], __builtin_fmaf(g1v, t[7], __builtin_fmaf(g0, t[6], 0.f)));
      float xr[3] = {0.f, 0.f, 0.f};
      if (live && n0 + p < a.N) {
        const float* xp = a.x.p + (int64_t)b * a.x.bs + (int64_t)(n0 + p) * a.x.ps;
        xr[0] = xp[0], xr[1] = xp[a.x.cs], xr[2] = xp[2 * a.x.cs];
      }
      const float gv[3] = {g0, g1v, g2v};
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          const float sum = wave_sum(xr[c] * gv[d]);
          if (lane == 0) part_gT[c * 3 + d] = sum;
        }
      if (lane >= 9 && lane < 16) part_gT[lane] = 0.f;
    }
    if (live && n0 + p < a.N) {
      float* o = a.gx.p + (int64_t)b * a.gx.bs + (int64_t)(n0 + p) * a.gx.ps;
      if (a.accumulate) {
        o[0] += o0, o[a.gx.cs] += o1, o[2 * a.gx.cs] += o2;
      } else {
        o[0] = o0, o[a.gx.cs] = o1, o[2 * a.gx.cs] = o2;
      }
    }
  }
}

// dL/dTf[b][i][j] = sum_n h[i,n] q[n,j] with h = relu(W1 x' + b1) recomputed (the forward's FMA chain, so the same
// bits). Workgroup = (16 rows i, cloud b); thread = (column j, 4 rows); n ascends, chunk after chunk: a fixed order.
constexpr int FT_DCH = 128;          // points per chunk: one load round trip and two barriers per 128 points
__global__ __launch_bounds__(256) void ft_dtf_kernel(PtsView x, int N, const float* T, const float* W1, const float* b1,
                                                     const float* q, float* gTf) {
  __shared__ float hs[FT_DCH][16];
  __shared__ float qs[FT_DCH][PM_C1];
  const int b = blockIdx.y, i0 = blockIdx.x * 16;
  const int tid = threadIdx.x;
  const int j = tid & 63, ig = tid >> 6;
  // this thread's share of h: (points tid >> 4 + 16 e, row i0 + (tid & 15))
  const int hi = i0 + (tid & 15);
  const float w0 = W1[hi * 3 + 0], w1 = W1[hi * 3 + 1], w2 = W1[hi * 3 + 2], bb = b1[hi];
  const float* Tb = T + (int64_t)b * 9;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int n0 = 0; n0 < N; n0 += FT_DCH) {
#pragma unroll
    for (int e = 0; e < FT_DCH / 16; ++e) {
      const int p = (tid >> 4) + 16 * e;
      float px, py, pz;
      load_point(x, Tb, b, n0 + p, N, px, py, pz);
      const float v = __builtin_fmaf(w2, pz, __builtin_fmaf(w1, py, __builtin_fmaf(w0, px, bb)));
      hs[p][tid & 15] = (n0 + p < N) ? fmaxf(v, 0.f) : 0.f;
    }
#pragma unroll
    for (int e = 0; e < FT_DCH * PM_C1 / 256; ++e) {
      const int i = tid + 256 * e;
      qs[i >> 6][i & 63] = (n0 + (i >> 6) < N) ? q[((int64_t)b * N + n0) * PM_C1 + i] : 0.f;
    }
    __syncthreads();
#pragma unroll 8
    for (int p = 0; p < FT_DCH; ++p) {
      const float qv = qs[p][j];
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = __builtin_fmaf(hs[p][4 * ig + e], qv, acc[e]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) gTf[((int64_t)b * PM_C1 + i0 + 4 * ig + e) * PM_C1 + j] = acc[e];
}

}  // namespace pc3d

using namespace pc3d;

extern "C" int pc3d_pointnet_ft_tower_fwd_f32(const float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs, int B, int N,
                                              const float* T, const float* W1, const float* b1, const float* WA,
                                              const float* bA, const float* W2, int64_t w2_bs, const float* b2,
                                              const float* W3, const float* b3, int C3, float* part_val,
                                              int32_t* part_idx, uint64_t* mask1, uint64_t* maskA, uint32_t* mask2,
                                              void* stream) {
  const char* who = "pc3d_pointnet_ft_tower_fwd_f32";
  PC3D_REQUIRE(B >= 0 && N >= 1, "%s: bad sizes B=%d N=%d", who, B, N);
  PC3D_REQUIRE(C3 >= 32 && C3 % 32 == 0 && C3 <= PM_MAXC3F, "%s: C3=%d must be a multiple of 32 <= 1024", who, C3);
  PC3D_REQUIRE(B <= 65535, "%s: B=%d exceeds grid.y limit", who, B);
  PC3D_REQUIRE(w2_bs == 0 || w2_bs >= PM_C2 * PM_C1, "%s: w2_bs=%lld overlaps the clouds' weights", who, (long long)w2_bs);
  if (B == 0) return PC3D_OK;
  PC3D_REQUIRE(x && T && W1 && b1 && W2 && b2 && W3 && b3 && part_val && part_idx && mask1 && mask2, "%s: null pointer", who);
  PC3D_REQUIRE((WA == nullptr) == (bA == nullptr) && (WA == nullptr) == (maskA == nullptr),
               "%s: WA, bA and maskA must all be given (the 64 -> 64 layer) or all be NULL", who);
  const int ntiles = cdiv(N, PM_TP);
  FTFwdArgs a{{x, x_bs, x_ps, x_cs}, N, C3, ntiles, T, W1, b1, WA, bA, W2, w2_bs, b2, W3, b3, part_val, part_idx,
              mask1, maskA, mask2};
  if (WA)
    hipLaunchKernelGGL(ft_tower_fwd_kernel<true>, dim3(ntiles, B), dim3(PM_FT), 0, as_stream(stream), a);
  else
    hipLaunchKernelGGL(ft_tower_fwd_kernel<false>, dim3(ntiles, B), dim3(PM_FT), 0, as_stream(stream), a);
  PC3D_LAUNCH_CHECK(who);
  return PC3D_OK;
}

extern "C" int pc3d_pointnet_ft_fold_w2_f32(const float* W2, const float* Tf, int B, float* W2b, void* stream) {
  const char* who = "pc3d_pointnet_ft_fold_w2_f32";
  PC3D_REQUIRE(B >= 0 && B <= 65535, "%s: bad batch B=%d", who, B);
  if (B == 0) return PC3D_OK;
  PC3D_REQUIRE(W2 && Tf && W2b, "%s: null pointer", who);
  hipLaunchKernelGGL(ft_fold_w2_kernel, dim3(PM_C2 / 32, B), dim3(256), 0, as_stream(stream), W2, Tf, W2b);
  PC3D_LAUNCH_CHECK(who);
  return PC3D_OK;
}

extern "C" int pc3d_pointnet_ft_tower_bwd_f32(const float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs, int B, int N,
                                              const float* T, const float* W1, const float* WA, const float* W2,
                                              int64_t w2_bs, const float* W2q, const float* W3, int C3,
                                              const int32_t* argidx, const uint64_t* mask1, const uint64_t* maskA,
                                              const uint32_t* mask2, const float* g_pooled, float* grad_x,
                                              int64_t gx_bs, int64_t gx_ps, int64_t gx_cs, float* part_gT,
                                              int gT_tiles, int gT_off, float* q, int accumulate, void* stream) {
  const char* who = "pc3d_pointnet_ft_tower_bwd_f32";
  PC3D_REQUIRE(B >= 0 && N >= 1, "%s: bad sizes B=%d N=%d", who, B, N);
  PC3D_REQUIRE(C3 >= 32 && C3 % 32 == 0 && C3 <= PM_MAXC3, "%s: C3=%d must be a multiple of 32 <= 1024", who, C3);
  PC3D_REQUIRE(B <= 65535, "%s: B=%d exceeds grid.y limit", who, B);
  PC3D_REQUIRE(w2_bs == 0 || w2_bs >= PM_C2 * PM_C1, "%s: w2_bs=%lld overlaps the clouds' weights", who, (long long)w2_bs);
  const int ntiles = cdiv(N, PM_BTP);
  PC3D_REQUIRE(T == nullptr || (gT_off >= 0 && gT_off + ntiles <= gT_tiles), "%s: part_gT rows [%d, %d) do not fit its %d rows",
               who, gT_off, gT_off + ntiles, gT_tiles);
  if (B == 0) return PC3D_OK;
  PC3D_REQUIRE(x && W1 && W2 && W3 && argidx && mask1 && mask2 && g_pooled && grad_x && (part_gT || !T), "%s: null pointer", who);
  PC3D_REQUIRE((WA == nullptr) == (maskA == nullptr), "%s: WA and maskA must both be given or both be NULL", who);
  PC3D_REQUIRE((W2q == nullptr) == (q == nullptr) && (WA == nullptr || W2q == nullptr),
               "%s: W2q and q go together (the trunk form), and not with WA (the 64 -> 64 form)", who);
  FTBwdArgs a{{x, x_bs, x_ps, x_cs}, N, C3, T, W1, WA, W2, w2_bs, W2q, W3, argidx, mask1, maskA, mask2, g_pooled,
              {grad_x, gx_bs, gx_ps, gx_cs}, part_gT, gT_tiles, gT_off, q, accumulate};
  if (WA)
    hipLaunchKernelGGL(ft_tower_bwd_kernel<true>, dim3(ntiles, B), dim3(256), 0, as_stream(stream), a);
  else
    hipLaunchKernelGGL(ft_tower_bwd_kernel<false>, dim3(ntiles, B), dim3(256), 0, as_stream(stream), a);
  PC3D_LAUNCH_CHECK(who);
  return PC3D_OK;
}

extern "C" int pc3d_pointnet_ft_dtf_f32(const float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs, int B, int N,
                                        const float* T, const float* W1, const float* b1, const float* q, float* g_Tf,
                                        void* stream) {
  const char* who = "pc3d_pointnet_ft_dtf_f32";
  PC3D_REQUIRE(B >= 0 && B <= 65535 && N >= 1, "%s: bad sizes B=%d N=%d", who, B, N);
  if (B == 0) return PC3D_OK;
  PC3D_REQUIRE(x && T && W1 && b1 && q && g_Tf, "%s: null pointer", who);
  hipLaunchKernelGGL(ft_dtf_kernel, dim3(PM_C1 / 16, B), dim3(256), 0, as_stream(stream), PtsView{x, x_bs, x_ps, x_cs}, N,
                     T, W1, b1, q, g_Tf);
  PC3D_LAUNCH_CHECK(who);
  return PC3D_OK;
}
