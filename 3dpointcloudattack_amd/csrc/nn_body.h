// The two-scan nearest-neighbour search as a device function: nn_kernel (nn.hip) and the linear launch that carries the
// search as extra workgroups (linear_riders.hip) compile these statements. The workgroup's (query tile, cloud) and its
// dynamic LDS are arguments, not blockIdx / the extern array.
#pragma once
#include "pc3d_common.h"

namespace pc3d {

struct NNDir {
  PtsView q, r;
  int N, M;
  float* d;
  int32_t* i;
  int64_t* i64 = nullptr;   // the same indices as 64-bit integers (the pytorch3d-style API hands out int64), or null
};
struct NNArgs {
  NNDir dir[2];
};

constexpr int kNNMaxTile = 4096;           // reference points per LDS tile (48 KiB SoA)
constexpr float kFar = 1.0e18f;            // sentinel coordinate: (1e18)^2*3 < FLT_MAX, never the minimum

constexpr int kNNChunk = 8;                // reference points per arg-min bookkeeping step

// the one distance formula of this file (scan and index resolution must agree bit for bit)
__device__ __forceinline__ float nn_dist(float rx, float ry, float rz, float qx, float qy, float qz) {
  const float dx = rx - qx, dy = ry - qy, dz = rz - qz;
  float d = dx * dx;
  d = __builtin_fmaf(dy, dy, d);
  return __builtin_fmaf(dz, dz, d);
}

// WAVES waves share the queries and split the staged reference tile (8 for small, launch-bound problems).
// (bx_, b) = (tile of 64*Q queries, cloud) of this workgroup; lds = its dynamic LDS (nn_lds_bytes); all threads call it.
template <int Q, int WAVES>
__device__ __forceinline__ void nn_body(const NNDir& D, int mt_cap, int bx_, int b, float* lds) {
  constexpr int kNNWaves = WAVES, kNNThreads = WAVES * 64;
  const int N = D.N, M = D.M;
  const int q0 = bx_ * (kWave * Q);
  if (q0 >= N) return;  // grid.x is sized for the larger direction
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x >> 6;

  // tile geometry (uniform): mt = points staged per pass, slice = points scanned per wave, multiple of the chunk
  const int mt = M < mt_cap ? M : mt_cap;
  const int slice = ((mt + kNNWaves * kNNChunk - 1) / (kNNWaves * kNNChunk)) * kNNChunk;
  const int mt_pad = slice * kNNWaves;
  float* sx = lds;
  float* sy = lds + mt_pad;
  float* sz = lds + 2 * mt_pad;

  float qx[Q], qy[Q], qz[Q], best[Q];
  int bidx[Q];
  const float* qb = D.q.p + (int64_t)b * D.q.bs;
#pragma unroll
  for (int k = 0; k < Q; ++k) {
    int qi = q0 + k * kWave + lane;
    if (qi >= N) qi = N - 1;  // clamp: duplicates a valid query, result discarded at the store
    const float* qp = qb + (int64_t)qi * D.q.ps;
    qx[k] = qp[0];
    qy[k] = qp[D.q.cs];
    qz[k] = qp[2 * D.q.cs];
    best[k] = __builtin_inff();
    bidx[k] = 0;
  }

  const float* rb = D.r.p + (int64_t)b * D.r.bs;
  for (int m0 = 0; m0 < M; m0 += mt) {
    __syncthreads();  // previous tile fully consumed
    for (int j = threadIdx.x; j < mt_pad; j += kNNThreads) {
      const int m = m0 + j;
      float x = kFar, y = kFar, z = kFar;
      if (j < mt && m < M) {
        const float* rp = rb + (int64_t)m * D.r.ps;
        x = rp[0];
        y = rp[D.r.cs];
        z = rp[2 * D.r.cs];
      }
      sx[j] = x;
      sy[j] = y;
      sz[j] = z;
    }
    __syncthreads();

    const int s0 = wave * slice;
    for (int j = s0; j < s0 + slice; j += kNNChunk) {
      const float4 rx0 = *reinterpret_cast<const float4*>(sx + j), rx1 = *reinterpret_cast<const float4*>(sx + j + 4);
      const float4 ry0 = *reinterpret_cast<const float4*>(sy + j), ry1 = *reinterpret_cast<const float4*>(sy + j + 4);
      const float4 rz0 = *reinterpret_cast<const float4*>(sz + j), rz1 = *reinterpret_cast<const float4*>(sz + j + 4);
      const float rxa[kNNChunk] = {rx0.x, rx0.y, rx0.z, rx0.w, rx1.x, rx1.y, rx1.z, rx1.w};
      const float rya[kNNChunk] = {ry0.x, ry0.y, ry0.z, ry0.w, ry1.x, ry1.y, ry1.z, ry1.w};
      const float rza[kNNChunk] = {rz0.x, rz0.y, rz0.z, rz0.w, rz1.x, rz1.y, rz1.z, rz1.w};
#pragma unroll
      for (int k = 0; k < Q; ++k) {
        float d[kNNChunk];
#pragma unroll
        for (int e = 0; e < kNNChunk; ++e) d[e] = nn_dist(rxa[e], rya[e], rza[e], qx[k], qy[k], qz[k]);
        // chunk minimum with v_min3 (0.5 op / pair); WHICH of the 8 it was is resolved once, after the scan
        float m = __builtin_fminf(__builtin_fminf(d[0], d[1]), d[2]);
        m = __builtin_fminf(__builtin_fminf(m, d[3]), d[4]);
        m = __builtin_fminf(__builtin_fminf(m, d[5]), d[6]);
        m = __builtin_fminf(m, d[7]);
        if (m < best[k]) {     // strict: the EARLIEST chunk holding the minimum wins
          best[k] = m;
          bidx[k] = m0 + j;
        }
      }
    }
  }

  // merge the four waves' candidates (ascending wave = ascending reference index inside a tile; across
  // tiles compare indices explicitly so the lowest index wins ties)
  // (the merge area sits BEHIND the staged tile: when the whole reference cloud fitted one tile it is still there,
  // and the arg-min below is resolved from LDS instead of eight dependent global loads per query)
  __syncthreads();
  float* cd = lds + 3 * mt_pad;                           // [kNNWaves][64*Q]
  int* ci = reinterpret_cast<int*>(cd + kNNWaves * kWave * Q);
  const bool resident = M <= mt;
#pragma unroll
  for (int k = 0; k < Q; ++k) {
    cd[wave * (kWave * Q) + k * kWave + lane] = best[k];
    ci[wave * (kWave * Q) + k * kWave + lane] = bidx[k];
  }
  __syncthreads();
  for (int t = threadIdx.x; t < kWave * Q; t += kNNThreads) {
    float bd = cd[t];
    int bi = ci[t];
#pragma unroll
    for (int w = 1; w < kNNWaves; ++w) {
      const float d = cd[w * (kWave * Q) + t];
      const int i = ci[w * (kWave * Q) + t];
      if (d < bd || (d == bd && i < bi)) {
        bd = d;
        bi = i;
      }
    }
    const int qi = q0 + t;
    if (qi < N) {
      if (D.d) D.d[(int64_t)b * N + qi] = bd;
      if (D.i || D.i64) {
        // bi is the first index of the winning chunk: the arg-min is the first of its 8 points whose distance,
        // recomputed with the same instructions, equals the minimum (ties -> lowest index, as torch.min)
        const float* qp = qb + (int64_t)qi * D.q.ps;
        const float x = qp[0], y = qp[D.q.cs], z = qp[2 * D.q.cs];
        int arg = bi;
        if (resident) {        // bi is a multiple of 8 inside the staged (padded with far sentinels) tile
#pragma unroll
          for (int e = kNNChunk - 1; e >= 0; --e)
            if (nn_dist(sx[bi + e], sy[bi + e], sz[bi + e], x, y, z) == bd) arg = bi + e;
        } else {
#pragma unroll
          for (int e = kNNChunk - 1; e >= 0; --e) {
            const int m = bi + e;
            if (m < M) {
              const float* rp = rb + (int64_t)m * D.r.ps;
              if (nn_dist(rp[0], rp[D.r.cs], rp[2 * D.r.cs], x, y, z) == bd) arg = m;
            }
          }
        }
        if (D.i) D.i[(int64_t)b * N + qi] = arg;
        if (D.i64) D.i64[(int64_t)b * N + qi] = arg;
      }
    }
  }
}

// LDS of one workgroup: the staged tile (SoA, padded to whole chunks per wave) + the merge area behind it
static inline size_t nn_lds_bytes(int M, int Q, int waves, int* mt_cap_out) {
  const int cap = kNNMaxTile;   // 1024 / 2048 / 4096 measured equal at B=32, N=4096
  const int mt = M < cap ? M : cap;
  const int slice = ((mt + waves * kNNChunk - 1) / (waves * kNNChunk)) * kNNChunk;
  const size_t tile = (size_t)3 * slice * waves * sizeof(float);
  const size_t merge = (size_t)waves * kWave * Q * 8;
  *mt_cap_out = cap;
  return tile + merge;
}

// Queries per lane and waves per workgroup of the two-scan search for a problem size (maxN / maxM over the directions)
static inline void nn_plan(int maxN, int maxM, int B, int ndir, int* Q_out, int* waves_out) {
  // Queries per lane: enough ILP to cover the LDS broadcast reads, but keep >= ~4 waves per SIMD's worth of
  // workgroups on 256 CUs (grid = tiles x B x ndir).
  const long q_total = (long)maxN * B * ndir;
  int Q = 4;
  if (q_total / (kWave * 4) < 1024) Q = 2;
  if (q_total / (kWave * 2) < 1024) Q = 1;
  // Small problems are bound by each workgroup's latency chain (stage the tile, scan it, merge), not by issue rate:
  // eight waves split the staged tile instead of four, halving the scan each wave walks.
  // (sixteen waves per workgroup measured no better: 16.4 against 14.4 us for both directions at B=32, N=1024)
  *Q_out = Q;
  *waves_out = (Q == 1 && maxM >= 512) ? 8 : 4;
}

}  // namespace pc3d
