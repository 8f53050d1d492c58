// Point-dropping defences put in front of a victim (attack/SIadv/baselines/defense/drop_points/{SOR,SRS}.py of the
// reference): statistical outlier removal and simple random sampling as heads with a FIXED output shape and no host
// round trip, so a defended victim sits inside an attack loop (and a captured hipGraph) like any other.
//
//   sor_select   one workgroup per cloud: v (mean of the k neighbour distances), mean + alpha * unbiased std in fp64 with a
//                fixed summation order, the mask, the ordered compaction (ballot + popcount prefix across the waves: no
//                sort, no atomics), the cyclic padding src[j] = kept[j mod n] and the gather of the kept points
//   sor_fused    the same behind a brute-force search of the cloud held in LDS (K <= 4096): one launch instead of two
//   sor_bwd      gather form of the gradient: one thread per input point sums the output slots that copy it, ascending
//   srs_select   counter-based hash keys per point, the smallest K - drop_num picked by an in-LDS bitonic network
//   gather       out[b,:,j] = x[b,:,idx[b,j]] for an index table (SRS; any layout on both sides)
#include "pc3d_common.h"

namespace pc3d {
namespace {

constexpr int kSorThreads = 1024;                  // 16 waves: one workgroup owns a cloud
constexpr int kSorWaves = kSorThreads / kWave;
constexpr int kSorMaxPoints = 8192;                // kept list in LDS (32 KB)
constexpr int kSorFusedMaxPoints = 4096;           // cloud in LDS (48 KB)
constexpr int kSrsMaxPoints = 4096;                // 64-bit keys of the padded cloud in LDS (32 KB)
constexpr int kSrsIdxBits = 13;

struct SorArgs {
  const float* d;        // [B,K,k1] ascending squared distances, self first
  PtsView x;
  int K, k1, npoint;
  double alpha;
  float *v, *thr;        // [B,K], [B] (either may be null)
  int32_t *count, *rank, *src;
  PtsViewMut out;
};

// Everything after the search, for the cloud of this workgroup. d: the cloud's [K,k1] distances (thread t reads the rows
// t, t + kSorThreads, ... only), kept: K ints of LDS.
__device__ void sor_tail(const SorArgs& a, const float* d, int b, int* kept, double* red, int* wcnt) {
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int K = a.K, k1 = a.k1;
  const double kk = (double)(k1 - 1);
  auto vof = [&](int i) {
    double s = 0.0;
    for (int c = 1; c < k1; ++c) s += (double)d[(int64_t)i * k1 + c];
    return s / kk;
  };
  double part = 0.0;
  for (int i = tid; i < K; i += kSorThreads) part += vof(i);
  const double mean = block_sum_ordered<kSorWaves>(part, red) / (double)K;
  part = 0.0;
  for (int i = tid; i < K; i += kSorThreads) {
    const double e = vof(i) - mean;
    part += e * e;
  }
  const double var = block_sum_ordered<kSorWaves>(part, red) / (double)(K - 1);
  const double thr = mean + a.alpha * sqrt(var);
  if (tid == 0 && a.thr) a.thr[b] = (float)thr;

  int base = 0;
  for (int c0 = 0; c0 < K; c0 += kSorThreads) {
    const int i = c0 + tid;
    double v = 0.0;
    bool keep = false;
    if (i < K) {
      v = vof(i);
      keep = v <= thr;
      if (a.v) a.v[(int64_t)b * K + i] = (float)v;
    }
    const unsigned long long m = __ballot(keep);                   // wave64: one bit per lane
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wcnt[wave] = __popcll(m);
    __syncthreads();
    int off = base, tot = 0;
    for (int w = 0; w < kSorWaves; ++w) {
      const int c = wcnt[w];
      off += w < wave ? c : 0;
      tot += c;
    }
    if (i < K) {
      const int r = keep ? off + before : -1;
      a.rank[(int64_t)b * K + i] = r;
      if (keep) kept[r] = i;
    }
    base += tot;
    __syncthreads();
  }
  const int n = base;
  if (tid == 0) a.count[b] = n;
  const float* xb = a.x.p + (int64_t)b * a.x.bs;
  float* ob = a.out.p + (int64_t)b * a.out.bs;
  for (int j = tid; j < a.npoint; j += kSorThreads) {
    // n == 0 only when every v is NaN (alpha < 0 or non-finite input): nothing to copy
    const int s = n > 0 ? kept[j % n] : -1;
    a.src[(int64_t)b * a.npoint + j] = s;
    const float qn = __builtin_nanf("");
    const float* xp = xb + (int64_t)(s < 0 ? 0 : s) * a.x.ps;
    float* op = ob + (int64_t)j * a.out.ps;
    op[0] = s < 0 ? qn : xp[0];
    op[a.out.cs] = s < 0 ? qn : xp[a.x.cs];
    op[2 * a.out.cs] = s < 0 ? qn : xp[2 * a.x.cs];
  }
}

__global__ __launch_bounds__(kSorThreads) void sor_select_kernel(SorArgs a) {
  extern __shared__ int kept_dyn[];
  __shared__ double red[kSorWaves];
  __shared__ int wcnt[kSorWaves];
  const int b = blockIdx.x;
  sor_tail(a, a.d + (int64_t)b * a.K * a.k1, b, kept_dyn, red, wcnt);
}

// Brute-force self-kNN of the cloud in LDS with the arithmetic of knn.hip's scan (dx*dx, then two fused multiply-adds), so
// the K1 smallest values are the same bits; they go to d (global, read back by the same thread), then the tail.
template <int K1>
__global__ __launch_bounds__(kSorThreads) void sor_fused_kernel(SorArgs a, float* __restrict__ dws) {
  __shared__ float sp[3][kSorFusedMaxPoints];
  __shared__ double red[kSorWaves];
  __shared__ int wcnt[kSorWaves];
  const int b = blockIdx.x, tid = threadIdx.x, K = a.K;
  const float* xb = a.x.p + (int64_t)b * a.x.bs;
  for (int i = tid; i < K; i += kSorThreads) {
    const float* xp = xb + (int64_t)i * a.x.ps;
    sp[0][i] = xp[0];
    sp[1][i] = xp[a.x.cs];
    sp[2][i] = xp[2 * a.x.cs];
  }
  __syncthreads();
  float* d = dws + (int64_t)b * K * K1;
  for (int i = tid; i < K; i += kSorThreads) {
    const float qx = sp[0][i], qy = sp[1][i], qz = sp[2][i];
    float best[K1];
#pragma unroll
    for (int u = 0; u < K1; ++u) best[u] = __builtin_inff();
    for (int j = 0; j < K; ++j) {
      const float dx = sp[0][j] - qx, dy = sp[1][j] - qy, dz = sp[2][j] - qz;
      float t = dx * dx;
      t = __builtin_fmaf(dy, dy, t);
      t = __builtin_fmaf(dz, dz, t);
      if (t < best[K1 - 1]) {
        best[K1 - 1] = t;
#pragma unroll
        for (int u = K1 - 1; u > 0; --u) {
          const float lo = fminf(best[u - 1], best[u]), hi = fmaxf(best[u - 1], best[u]);
          best[u - 1] = lo;
          best[u] = hi;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < K1; ++u) d[(int64_t)i * K1 + u] = best[u];
  }
  __threadfence_block();
  __syncthreads();                                   // the cloud is dead from here: its LDS holds the kept list
  sor_tail(a, d, b, reinterpret_cast<int*>(&sp[0][0]), red, wcnt);
}

struct SorBwdArgs {
  PtsView g;             // [B,npoint]
  const int32_t *count, *rank;
  int K, npoint;
  PtsViewMut grad;       // [B,K]
};

__global__ __launch_bounds__(256) void sor_bwd_kernel(SorBwdArgs a) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.K) return;
  const int r = a.rank[(int64_t)b * a.K + i], n = a.count[b];
  float gx = 0.f, gy = 0.f, gz = 0.f;
  if (r >= 0 && r < n) {
    const float* gb = a.g.p + (int64_t)b * a.g.bs;
    for (int j = r; j < a.npoint; j += n) {
      const float* gp = gb + (int64_t)j * a.g.ps;
      gx += gp[0];
      gy += gp[a.g.cs];
      gz += gp[2 * a.g.cs];
    }
  }
  float* op = a.grad.p + (int64_t)b * a.grad.bs + (int64_t)i * a.grad.ps;
  op[0] = gx;
  op[a.grad.cs] = gy;
  op[2 * a.grad.cs] = gz;
}

// keys[i] = hash(seed, call, b, i) with the point index in the low bits (all keys distinct: a total order, so the network's
// result does not depend on how it is scheduled); pads sort to the end. Ascending bitonic network over P = 2^p >= K keys,
// a barrier after EVERY stage.
__global__ __launch_bounds__(1024) void srs_select_kernel(uint64_t seed, const int32_t* __restrict__ ctr, int ctr_host, int K,
                                                          int M, int P, int32_t* __restrict__ idx) {
  extern __shared__ uint64_t keys[];
  const int b = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
  const uint64_t call = (uint64_t)(uint32_t)(ctr ? ctr[0] : ctr_host);
  const uint64_t s0 = mix64(seed + 0x9E3779B97F4A7C15ull * (call + 1));
  const uint64_t lowmask = (1ull << kSrsIdxBits) - 1ull;
  for (int i = tid; i < P; i += T) {
    const uint64_t h = mix64(s0 ^ (((uint64_t)(uint32_t)b << 32) | (uint32_t)i));
    keys[i] = i < K ? ((h & ~lowmask) | (uint64_t)i) : ~0ull;
  }
  __syncthreads();
  block_bitonic_sort_u64(keys, P, tid, T);
  for (int i = tid; i < M; i += T) idx[(int64_t)b * M + i] = (int32_t)(keys[i] & lowmask);
}

struct GatherArgs {
  PtsView x;
  const int32_t* idx;
  int K, M;
  PtsViewMut out;
};

__global__ __launch_bounds__(256) void gather_points_kernel(GatherArgs a) {
  const int b = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
  if (j >= a.M) return;
  const int s = a.idx[(int64_t)b * a.M + j];
  const bool ok = (unsigned)s < (unsigned)a.K;
  const float* xp = a.x.p + (int64_t)b * a.x.bs + (int64_t)(ok ? s : 0) * a.x.ps;
  float* op = a.out.p + (int64_t)b * a.out.bs + (int64_t)j * a.out.ps;
  const float qn = __builtin_nanf("");
  op[0] = ok ? xp[0] : qn;
  op[a.out.cs] = ok ? xp[a.x.cs] : qn;
  op[2 * a.out.cs] = ok ? xp[2 * a.x.cs] : qn;
}

int sor_check(const char* nm, int B, int K, int k1, double alpha, int npoint, int maxK) {
  PC3D_REQUIRE(B >= 0 && K >= 2 && k1 >= 2 && npoint >= 1, "%s: bad sizes B=%d K=%d k1=%d npoint=%d", nm, B, K, k1, npoint);
  PC3D_REQUIRE(k1 <= K, "%s: k + 1 = %d neighbours asked of a cloud of K=%d points", nm, k1, K);
  PC3D_REQUIRE(K <= npoint, "%s: K=%d exceeds npoint=%d (the kept points may not fit the output)", nm, K, npoint);
  PC3D_REQUIRE(K <= maxK, "%s: K=%d exceeds the limit of %d points", nm, K, maxK);
  PC3D_REQUIRE(alpha == alpha, "%s: alpha is NaN", nm);
  return PC3D_OK;
}

}  // namespace
}  // namespace pc3d

using namespace pc3d;

extern "C" int pc3d_sor_select_f32(const float* dists, const float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs, int B, int K,
                                   int k1, double alpha, int npoint, float* v, float* thr, int32_t* count, int32_t* rank,
                                   int32_t* src, float* out, int64_t o_bs, int64_t o_ps, int64_t o_cs, void* stream) {
  if (int rc = sor_check("pc3d_sor_select_f32", B, K, k1, alpha, npoint, kSorMaxPoints)) return rc;
  if (B == 0) return PC3D_OK;
  PC3D_REQUIRE(dists && x && count && rank && src && out, "pc3d_sor_select_f32: null pointer");
  SorArgs a{dists, {x, x_bs, x_ps, x_cs}, K, k1, npoint, alpha, v, thr, count, rank, src, {out, o_bs, o_ps, o_cs}};
  hipLaunchKernelGGL(sor_select_kernel, dim3(B), dim3(kSorThreads), (size_t)K * sizeof(int), as_stream(stream), a);
  PC3D_LAUNCH_CHECK("pc3d_sor_select_f32");
  return PC3D_OK;
}

extern "C" int pc3d_sor_fused_f32(const float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs, int B, int K, int k1, double alpha,
                                  int npoint, float* dists, float* v, float* thr, int32_t* count, int32_t* rank, int32_t* src,
                                  float* out, int64_t o_bs, int64_t o_ps, int64_t o_cs, void* stream) {
  if (int rc = sor_check("pc3d_sor_fused_f32", B, K, k1, alpha, npoint, kSorFusedMaxPoints)) return rc;
  PC3D_REQUIRE(k1 <= 9, "pc3d_sor_fused_f32: k + 1 = %d out of range [2,9]", k1);
  if (B == 0) return PC3D_OK;
  PC3D_REQUIRE(dists && x && count && rank && src && out, "pc3d_sor_fused_f32: null pointer");
  SorArgs a{dists, {x, x_bs, x_ps, x_cs}, K, k1, npoint, alpha, v, thr, count, rank, src, {out, o_bs, o_ps, o_cs}};
  const hipStream_t st = as_stream(stream);
  switch (k1) {
#define PC3D_SOR_FUSED(n) \
  case n: hipLaunchKernelGGL(sor_fused_kernel<n>, dim3(B), dim3(kSorThreads), 0, st, a, dists); break;
    PC3D_SOR_FUSED(2) PC3D_SOR_FUSED(3) PC3D_SOR_FUSED(4) PC3D_SOR_FUSED(5)
    PC3D_SOR_FUSED(6) PC3D_SOR_FUSED(7) PC3D_SOR_FUSED(8) PC3D_SOR_FUSED(9)
#undef PC3D_SOR_FUSED
  }
  PC3D_LAUNCH_CHECK("pc3d_sor_fused_f32");
  return PC3D_OK;
}

extern "C" int pc3d_sor_bwd_f32(const float* g, int64_t g_bs, int64_t g_ps, int64_t g_cs, const int32_t* count,
                                const int32_t* rank, int B, int K, int npoint, float* grad, int64_t gr_bs, int64_t gr_ps,
                                int64_t gr_cs, void* stream) {
  PC3D_REQUIRE(B >= 0 && K >= 1 && npoint >= 1, "pc3d_sor_bwd_f32: bad sizes B=%d K=%d npoint=%d", B, K, npoint);
  PC3D_REQUIRE(B <= 65535, "pc3d_sor_bwd_f32: B=%d exceeds grid.y limit", B);
  if (B == 0) return PC3D_OK;
  PC3D_REQUIRE(g && count && rank && grad, "pc3d_sor_bwd_f32: null pointer");
  SorBwdArgs a{{g, g_bs, g_ps, g_cs}, count, rank, K, npoint, {grad, gr_bs, gr_ps, gr_cs}};
  hipLaunchKernelGGL(sor_bwd_kernel, dim3(cdiv(K, 256), B), dim3(256), 0, as_stream(stream), a);
  PC3D_LAUNCH_CHECK("pc3d_sor_bwd_f32");
  return PC3D_OK;
}

extern "C" int pc3d_srs_select_i32(int64_t seed, const int32_t* counter, int counter_host, int B, int K, int M, int32_t* idx,
                                   void* stream) {
  PC3D_REQUIRE(B >= 0 && K >= 1 && M >= 1 && M <= K, "pc3d_srs_select_i32: bad sizes B=%d K=%d M=%d (1 <= M <= K)", B, K, M);
  PC3D_REQUIRE(K <= kSrsMaxPoints, "pc3d_srs_select_i32: K=%d exceeds the limit of %d points", K, kSrsMaxPoints);
  if (B == 0) return PC3D_OK;
  PC3D_REQUIRE(idx, "pc3d_srs_select_i32: null pointer");
  int P = 2;
  while (P < K) P <<= 1;
  int T = P / 2;
  T = T < kWave ? kWave : (T > 1024 ? 1024 : T);
  hipLaunchKernelGGL(srs_select_kernel, dim3(B), dim3(T), (size_t)P * sizeof(uint64_t), as_stream(stream), (uint64_t)seed,
                     counter, counter_host, K, M, P, idx);
  PC3D_LAUNCH_CHECK("pc3d_srs_select_i32");
  return PC3D_OK;
}

extern "C" int pc3d_gather_points_f32(const float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs, const int32_t* idx, int B,
                                      int K, int M, float* out, int64_t o_bs, int64_t o_ps, int64_t o_cs, void* stream) {
  PC3D_REQUIRE(B >= 0 && K >= 1 && M >= 1, "pc3d_gather_points_f32: bad sizes B=%d K=%d M=%d", B, K, M);
  PC3D_REQUIRE(B <= 65535, "pc3d_gather_points_f32: B=%d exceeds grid.y limit", B);
  if (B == 0) return PC3D_OK;
  PC3D_REQUIRE(x && idx && out, "pc3d_gather_points_f32: null pointer");
  GatherArgs a{{x, x_bs, x_ps, x_cs}, idx, K, M, {out, o_bs, o_ps, o_cs}};
  hipLaunchKernelGGL(gather_points_kernel, dim3(cdiv(M, 256), B), dim3(256), 0, as_stream(stream), a);
  PC3D_LAUNCH_CHECK("pc3d_gather_points_f32");
  return PC3D_OK;
}
