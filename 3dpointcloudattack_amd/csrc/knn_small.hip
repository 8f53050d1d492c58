// Values-only small-k search: the k1 (2 .. 9) smallest squared distances of every query, ascending, no indices — what
// SOR asks of a search (attack/SIadv/baselines/defense/drop_points/SOR.py: k + 1 = 3 columns, the indices never read).
//
// knn.hip's wave-per-query kernel keeps a sorted list ACROSS the 64 lanes of a wave (built for K up to 64): at k1 = 3 its
// seeding rounds and serial insertions outweigh its scan. Here a lane owns a query (Q queries per lane, as nn_body.h) and
// its k1-entry list lives in k1 registers per query; an insertion is k1 branch-free integer instructions (a median of
// three per entry) that every lane runs for every candidate, so there is no divergence, no ballot and no cross-lane
// traffic in the scan. The reference cloud is staged through LDS as SoA tiles and read by all lanes at the same address (a
// broadcast: no bank conflicts); the WAVES waves of a workgroup share the queries and split the tile, each keeping a
// partial list per query, and the partial lists are merged through LDS (in the tile's own memory) at the end.
//
// Bits. The distance is knn.hip's and sor_fused_kernel's: dx*dx, then two fmaf. Entries are ordered by knn_list.h's integer
// key (the bit pattern of a squared distance, which is >= +0 or NaN; NaN sorts above +inf) and stored, as
// knn_wave_kernel stores them, with NaN as +inf: its seed replaces a NaN by +inf and its scan never inserts a key above
// +inf's. The candidate multiset is knn_wave_kernel's too: the M reference points plus far sentinels (1e18 per
// coordinate) up to the next multiple of 64 — they only ever show where fewer than k1 distances are below 3e36.
// The k1 smallest keys of a multiset do not depend on the order the candidates are visited in or on how they are split:
// any tiling, any split of the reference set across waves and any merge order give the same bits, so the output equals
// pc3d_knn_f32's distances bit for bit BY CONSTRUCTION, with no tie rule to keep (equal keys are equal bits).
#include "pc3d_common.h"
#include "knn_list.h"

namespace pc3d {

constexpr int kKsTile = 2048;        // reference points per LDS tile (24 KiB SoA); the merge area reuses it
constexpr int kKsChunk = 8;          // candidates per LDS read step (two float4 per coordinate)
constexpr float kKsFar = 1.0e18f;    // knn.hip's sentinel coordinate

struct KnnSmallArgs {
  PtsView q, r;
  int N, M;
  float* d;    // [B,N,K1]
};

// candidate c into the ascending list l. Entry i of the new list is the median of (old l[i-1], old l[i], c) — c clamped
// between its two neighbours — and entry 0 the minimum: k1 VALU per candidate (the max-of-min form below is the shape the
// compiler selects v_med3_i32 for), against 2 k1 for a min / max pair per entry.
__device__ __forceinline__ int ks_min(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int ks_max(int a, int b) { return a > b ? a : b; }
__device__ __forceinline__ int ks_med3(int a, int b, int c) { return ks_max(ks_min(a, b), ks_min(ks_max(a, b), c)); }
template <int K1>
__device__ __forceinline__ void ks_insert(int (&l)[K1], int c) {
#pragma unroll
  for (int i = K1 - 1; i > 0; --i) l[i] = ks_med3(l[i - 1], l[i], c);   // descending: l[i-1] is still the old entry
  l[0] = ks_min(l[0], c);
}

// a squared distance (>= +0, or NaN with either sign) -> key in [0, kKnnInfKey]: one unsigned minimum
__device__ __forceinline__ int ks_key(float d) {
  const unsigned u = __builtin_bit_cast(unsigned, d);
  return (int)(u < (unsigned)kKnnInfKey ? u : (unsigned)kKnnInfKey);
}

template <int K1, int Q, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void knn_small_kernel(KnnSmallArgs a) {
  constexpr int kThreads = WAVES * 64;
  static_assert(64 % (WAVES * kKsChunk) == 0, "every wave's share of a 64-candidate step is whole chunks");
  static_assert((size_t)WAVES * K1 * 64 * Q <= (size_t)3 * kKsTile, "the merge area fits the tile's memory");
  __shared__ __attribute__((aligned(16))) float lds[3 * kKsTile];
  const int N = a.N, M = a.M;
  const int b = blockIdx.y;
  const int q0 = blockIdx.x * (64 * Q);
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  float* sx = lds;
  float* sy = lds + kKsTile;
  float* sz = lds + 2 * kKsTile;

  float qx[Q], qy[Q], qz[Q];
  int l[Q][K1];
  const float* qb = a.q.p + (int64_t)b * a.q.bs;
#pragma unroll
  for (int k = 0; k < Q; ++k) {
    int qi = q0 + k * 64 + lane;
    if (qi >= N) qi = N - 1;   // clamp: duplicates a valid query, its result is not stored
    const float* qp = qb + (int64_t)qi * a.q.ps;
    qx[k] = qp[0], qy[k] = qp[a.q.cs], qz[k] = qp[2 * a.q.cs];
#pragma unroll
    for (int i = 0; i < K1; ++i) l[k][i] = kKnnInfKey;
  }

  const float* rb = a.r.p + (int64_t)b * a.r.bs;
  const int Mp = (M + 63) & ~63;   // with knn_wave_kernel's sentinels
  for (int m0 = 0; m0 < Mp; m0 += kKsTile) {
    const int mt = (Mp - m0) < kKsTile ? (Mp - m0) : kKsTile;   // a multiple of 64
    __syncthreads();   // previous tile fully consumed
    for (int j = threadIdx.x; j < mt; j += kThreads) {
      float x = kKsFar, y = kKsFar, z = kKsFar;
      if (m0 + j < M) {
        const float* rp = rb + (int64_t)(m0 + j) * a.r.ps;
        x = rp[0], y = rp[a.r.cs], z = rp[2 * a.r.cs];
      }
      sx[j] = x, sy[j] = y, sz[j] = z;
    }
    __syncthreads();
    const int slice = mt / WAVES;   // a multiple of the chunk
    const int s0 = wave * slice;
    for (int j = s0; j < s0 + slice; j += kKsChunk) {
      const float4 rx0 = *reinterpret_cast<const float4*>(sx + j), rx1 = *reinterpret_cast<const float4*>(sx + j + 4);
      const float4 ry0 = *reinterpret_cast<const float4*>(sy + j), ry1 = *reinterpret_cast<const float4*>(sy + j + 4);
      const float4 rz0 = *reinterpret_cast<const float4*>(sz + j), rz1 = *reinterpret_cast<const float4*>(sz + j + 4);
      const float rxa[kKsChunk] = {rx0.x, rx0.y, rx0.z, rx0.w, rx1.x, rx1.y, rx1.z, rx1.w};
      const float rya[kKsChunk] = {ry0.x, ry0.y, ry0.z, ry0.w, ry1.x, ry1.y, ry1.z, ry1.w};
      const float rza[kKsChunk] = {rz0.x, rz0.y, rz0.z, rz0.w, rz1.x, rz1.y, rz1.z, rz1.w};
#pragma unroll
      for (int k = 0; k < Q; ++k) {
#pragma unroll
        for (int e = 0; e < kKsChunk; ++e) {
          const float dx = rxa[e] - qx[k], dy = rya[e] - qy[k], dz = rza[e] - qz[k];
          float t = dx * dx;
          t = __builtin_fmaf(dy, dy, t);
          t = __builtin_fmaf(dz, dz, t);
          ks_insert<K1>(l[k], ks_key(t));
        }
      }
    }
  }

  // merge the waves' partial lists: [WAVES][K1][64 * Q] keys in the tile's memory
  __syncthreads();
  int* mg = reinterpret_cast<int*>(lds);
#pragma unroll
  for (int k = 0; k < Q; ++k)
#pragma unroll
    for (int i = 0; i < K1; ++i) mg[(wave * K1 + i) * (64 * Q) + k * 64 + lane] = l[k][i];
  __syncthreads();
  for (int t = threadIdx.x; t < 64 * Q; t += kThreads) {
    int m[K1];
#pragma unroll
    for (int i = 0; i < K1; ++i) m[i] = mg[i * (64 * Q) + t];
#pragma unroll
    for (int w = 1; w < WAVES; ++w)
#pragma unroll
      for (int i = 0; i < K1; ++i) ks_insert<K1>(m, mg[(w * K1 + i) * (64 * Q) + t]);
    const int qi = q0 + t;
    if (qi < N) {
      float* dp = a.d + ((int64_t)b * N + qi) * K1;
#pragma unroll
      for (int i = 0; i < K1; ++i) dp[i] = __builtin_bit_cast(float, m[i]);
    }
  }
}

template <int K1>
static void knn_small_launch(const KnnSmallArgs& a, int B, hipStream_t st) {
  // Queries per lane and waves per workgroup as nn_plan (nn_body.h) chooses them: two queries per lane once that still
  // leaves >= 1024 workgroups; otherwise one, and eight waves split the tile when the cloud is large enough to feed them.
  const long q_total = (long)a.N * B;
  if (q_total / 128 >= 1024)
    hipLaunchKernelGGL((knn_small_kernel<K1, 2, 4>), dim3(cdiv(a.N, 128), B), dim3(256), 0, st, a);
  else if (a.M >= 512)
    hipLaunchKernelGGL((knn_small_kernel<K1, 1, 8>), dim3(cdiv(a.N, 64), B), dim3(512), 0, st, a);
  else
    hipLaunchKernelGGL((knn_small_kernel<K1, 1, 4>), dim3(cdiv(a.N, 64), B), dim3(256), 0, st, a);
}

}  // namespace pc3d

using namespace pc3d;

extern "C" int pc3d_knn_small_f32(const float* q, int64_t q_bs, int64_t q_ps, int64_t q_cs,
                                  const float* r, int64_t r_bs, int64_t r_ps, int64_t r_cs,
                                  int B, int N, int M, int k1, float* dists, void* stream) {
  PC3D_REQUIRE(B >= 0 && N >= 0 && M >= 1, "pc3d_knn_small_f32: bad sizes B=%d N=%d M=%d", B, N, M);
  PC3D_REQUIRE(k1 >= 2 && k1 <= 9, "pc3d_knn_small_f32: k1=%d out of range [2,9]", k1);
  PC3D_REQUIRE(k1 <= M, "pc3d_knn_small_f32: k1=%d exceeds the reference set size M=%d", k1, M);
  PC3D_REQUIRE(M <= (1 << 30) && N <= (1 << 30), "pc3d_knn_small_f32: N=%d / M=%d exceed 2^30 points", N, M);
  PC3D_REQUIRE(B <= 65535, "pc3d_knn_small_f32: B=%d exceeds grid.y limit", B);
  if (B == 0 || N == 0) return PC3D_OK;
  PC3D_REQUIRE(q && r && dists, "pc3d_knn_small_f32: null pointer");
  const KnnSmallArgs a{{q, q_bs, q_ps, q_cs}, {r, r_bs, r_ps, r_cs}, N, M, dists};
  hipStream_t st = as_stream(stream);
  switch (k1) {
    case 2: knn_small_launch<2>(a, B, st); break;
    case 3: knn_small_launch<3>(a, B, st); break;
    case 4: knn_small_launch<4>(a, B, st); break;
    case 5: knn_small_launch<5>(a, B, st); break;
    case 6: knn_small_launch<6>(a, B, st); break;
    case 7: knn_small_launch<7>(a, B, st); break;
    case 8: knn_small_launch<8>(a, B, st); break;
    default: knn_small_launch<9>(a, B, st); break;
  }
  PC3D_LAUNCH_CHECK("pc3d_knn_small_f32");
  return PC3D_OK;
}
