// The kNN attack's update (attack/KNN/KNN_attack.py:117-136) as ONE launch, one workgroup per sample:
//   * KNNDist's outlier statistics from the sorted self-kNN distances (dist_utils.py:133-151; the arithmetic of
//     knn_outlier_loss_kernel, knn.hip: the same values, the same 256-strided partial sums, the same threshold),
//   * the gradient of the masked kNN term — own side and neighbour side, summed in a fixed order without float atomics,
//   * the Chamfer adv -> ori gradient on the given arg-mins,
//   * Adam on victim + Chamfer + kNN gradient, ProjectInnerPoints (optional) and ClipPointsLinf: adam_element and
//     project_clip of update_body.h, the functions pc3d_adam_clip_step_f32 runs.
// It replaces pc3d_knn_outlier_loss_f32 + pc3d_knn_self_bwd_f32 (+ its ordered-scatter scratch) + pc3d_nn_bwd_f32 +
// pc3d_adam_clip_step_f32 in the captured iteration of CWKNN(device_loop=True).
//
// The neighbour-side sum. Only masked points emit edges (i, j = idx[i, e >= 1]); edge (i, j) adds 2 c (x_j - x_i) to j. Wave 0
// compacts the masked i into an LDS list in ascending order (ballot + popcount); the edges, in (list position, e) order,
// are staged through LDS 2048 at a time as (i << 16 | j); every thread walks the staged entries IN ORDER and adds those
// whose target it owns (j mod 1024 == its thread id: one test per entry however many points the thread owns; the wave
// half of that test is scalar) into the LDS accumulator of that target, which no other thread touches. The order of the additions into a point is therefore the
// edge order — a function of that cloud's own indices alone, not of the batch, the grid or the launch.
//
// LDS per sample: the cloud (12 B / point: the iterate is updated in place, so neighbours are read from this copy), the
// neighbour-side accumulators (12), the mean neighbour distances (4), the masked list (4) + the 8 KiB edge stage:
// 32 N + 8 KiB + 48 B = 136 KiB at N = 4096, the cap (the CU has 160 KiB; 8192 points would need 264).
#include "update_body.h"

namespace pc3d {

constexpr int kKuThreads = 1024;
constexpr int kKuEdges = 2048;                  // staged edges per trip
constexpr int kKuMaxPoints = PC3D_KNN_ATTACK_UPDATE_MAX_POINTS;
static_assert(kKuMaxPoints <= 65536 && (kKuThreads & (kKuThreads - 1)) == 0, "edge entries pack (i << 16 | j); owner test is a mask");

struct KnnUpdArgs {
  PtsViewMut adv;          // the iterate, updated in place
  PtsView ori, normal, g;  // normal.p null: ori doubles as the normal (clip_mode 1)
  PtsViewMut m, v;         // Adam moments, adv's strides
  int N, K1;               // K1 = k + 1 columns of knn_d / knn_idx (self first)
  const float* knn_d;      // [B,N,K1]
  const int32_t* knn_idx;  // [B,N,K1]
  const int32_t* nn_idx;   // [B,N] adv -> ori
  double lr, b1, b2;
  float eps, budget;
  int clip_mode;           // 0: ClipPointsLinf, 1: ProjectInnerPoints then ClipPointsLinf
  float alpha, c_ch, c_knn;
  const int* step_dev;
  int step_host;
};
// Clouds of different sizes in one batch: sample b counts lengths[b] points (int32 [B], read as data, clamped to [1, N]) and
// has constants of its own (what a run of that cloud alone prepares from its own N); c_ch / c_knn above are not read.
struct KnnUpdRaggedArgs : KnnUpdArgs {
  const int32_t* lengths;
  const float* c_ch_b;     // [B]
  const float* c_knn_b;    // [B]
};
template <bool RAGGED> struct KnnUpdArgsOf { using type = KnnUpdArgs; };
template <> struct KnnUpdArgsOf<true> { using type = KnnUpdRaggedArgs; };

static inline size_t knn_upd_lds_bytes(int N) {
  const size_t np = (size_t)((N + 3) & ~3);
  return np * 32 + (size_t)kKuEdges * 4 + 48;
}

// RAGGED: N is the capacity — the stride of knn_d / knn_idx / nn_idx and the size of the LDS arrays — and every loop over
// points, the statistics' divisors and the index clamps run over L = lengths[b] with the dense kernel's thread-to-point
// mapping and summation order: rows < L have the bits of the dense launch at N = L on that cloud alone. Rows >= L are never
// loaded (they may hold NaN), their m / v stay, and adv's take the NEW point 0 (the padding the victim's passes and the
// adv -> ori search rely on). The dense instantiation compiles to the kernel it was before RAGGED existed.
template <bool RAGGED>
__global__ __launch_bounds__(kKuThreads) void knn_attack_update_kernel(typename KnnUpdArgsOf<RAGGED>::type a) {
  extern __shared__ __attribute__((aligned(16))) float ku_lds[];
  const int N = a.N, np = (N + 3) & ~3, K1 = a.K1, k = K1 - 1;
  const int b = blockIdx.x, tid = threadIdx.x;
  int L = N;
  float c_ch = a.c_ch, c_knn = a.c_knn;
  if constexpr (RAGGED) {
    L = min(max(a.lengths[b], 1), N);
    c_ch = a.c_ch_b[b], c_knn = a.c_knn_b[b];
  }
  float* sx = ku_lds;
  float* sy = sx + np;
  float* sz = sy + np;
  float* ax = sz + np;      // neighbour-side accumulators
  float* ay = ax + np;
  float* az = ay + np;
  float* s_val = az + np;
  int* s_list = reinterpret_cast<int*>(s_val + np);
  int* s_edge = s_list + np;
  float* part = reinterpret_cast<float*>(s_edge + kKuEdges);      // [4]
  float* s_adam = part + 4;                                       // {step_size, bc2s}
  int* s_nm = reinterpret_cast<int*>(s_adam + 2);
  [[maybe_unused]] float* s_pad = reinterpret_cast<float*>(s_nm + 1);     // [3] RAGGED: the new point 0 (40 of the 48 tail bytes)
  const bool knn = k >= 1 && c_knn != 0.f;
  const float* db = a.knn_d + (int64_t)b * N * K1;
  const int32_t* ib = a.knn_idx + (int64_t)b * N * K1;

  if (tid == 0) {      // Adam's bias corrections in double (as torch), once per workgroup
    const int t = a.step_dev ? a.step_dev[0] : a.step_host;
    s_adam[0] = adam_step_size(a.lr, a.b1, t);
    s_adam[1] = adam_bc2s(a.b2, t);
  }
  const float inv_k = 1.f / (float)(k > 0 ? k : 1);
  for (int p = tid; p < L; p += kKuThreads) {
    const float* xp = a.adv.p + (int64_t)b * a.adv.bs + (int64_t)p * a.adv.ps;
    sx[p] = xp[0], sy[p] = xp[a.adv.cs], sz[p] = xp[2 * a.adv.cs];
    ax[p] = ay[p] = az[p] = 0.f;
    if (knn) {
      float v = 0.f;
      for (int j = 1; j < K1; ++j) v += db[(int64_t)p * K1 + j];
      s_val[p] = v * inv_k;
    }
  }
  __syncthreads();

  float thr = 0.f;
  const float w = 2.f * c_knn;
  if (knn) {
    // mean and unbiased std of the mean neighbour distances, thr = mean + alpha std (knn_outlier_loss_kernel's order)
    float s = 0.f;
    if (tid < 256)
      for (int i = tid; i < L; i += 256) s += s_val[i];
    const float mean = block_sum4_pairwise(s, part) / (float)L;
    float q = 0.f;
    if (tid < 256)
      for (int i = tid; i < L; i += 256) {
        const float dv = s_val[i] - mean;
        q += dv * dv;
      }
    const float var = block_sum4_pairwise(q, part) / (float)(L > 1 ? L - 1 : 1);
    thr = mean + a.alpha * sqrtf(var);
    // the masked points, ascending, by wave 0
    if (tid < 64) {
      int base = 0;
      for (int i0 = 0; i0 < L; i0 += 64) {
        const int i = i0 + tid;
        const bool out = i < L && s_val[i] > thr;
        const unsigned long long bal = __ballot(out);
        if (out) s_list[base + __popcll(bal & ((1ull << tid) - 1ull))] = i;
        base += __popcll(bal);
      }
      if (tid == 0) s_nm[0] = base;
    }
    __syncthreads();
    const int total = s_nm[0] * k;
    for (int c0 = 0; c0 < total; c0 += kKuEdges) {
      if (c0) __syncthreads();      // the previous trip's entries have been walked
      for (int t = tid; t < kKuEdges; t += kKuThreads) {
        const int f = c0 + t;
        int ent = -1;
        if (f < total) {
          const int sl = f / k, e = f - sl * k + 1, i = s_list[sl];
          const int j = min(max(ib[(int64_t)i * K1 + e], 0), L - 1);
          ent = (i << 16) | j;
        }
        s_edge[t] = ent;
      }
      __syncthreads();
      const int lim = min(kKuEdges, total - c0);
      // One broadcast ds_read_b128 per four entries (entries past lim hold -1). Every lane reads the same four words, so
      // they are taken into scalar registers and the first test — does the target belong to a lane of THIS wave — is
      // scalar work: a wave spends vector instructions on one entry in sixteen.
      const int wave = tid >> 6, lane = tid & 63;
      for (int t = 0; t < lim; t += 4) {
        const int4 e4 = *reinterpret_cast<const int4*>(s_edge + t);
        const int ee[4] = {__builtin_amdgcn_readfirstlane(e4.x), __builtin_amdgcn_readfirstlane(e4.y),
                           __builtin_amdgcn_readfirstlane(e4.z), __builtin_amdgcn_readfirstlane(e4.w)};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (ee[u] < 0 || ((ee[u] >> 6) & (kKuThreads / 64 - 1)) != wave) continue;
          if ((ee[u] & 63) != lane) continue;
          const int i = ee[u] >> 16, j = ee[u] & 0xffff;
          ax[j] += w * (sx[j] - sx[i]);
          ay[j] += w * (sy[j] - sy[i]);
          az[j] += w * (sz[j] - sz[i]);
        }
      }
    }
  }
  __syncthreads();      // (s_adam for the clouds without a kNN term)

  const AdamConsts ad = adam_consts_with(a.b1, a.b2, a.eps, s_adam[0], s_adam[1]);
  const float wc = 2.f * c_ch;
  const PtsView nrm = a.normal.p ? a.normal : a.ori;
  for (int p = tid; p < L; p += kKuThreads) {
    const float x[3] = {sx[p], sy[p], sz[p]};
    const float* op = a.ori.p + (int64_t)b * a.ori.bs + (int64_t)p * a.ori.ps;
    const float o[3] = {op[0], op[a.ori.cs], op[2 * a.ori.cs]};
    float g2[3] = {0.f, 0.f, 0.f};
    if (c_ch != 0.f) {
      const int j = min(max(a.nn_idx[(int64_t)b * N + p], 0), L - 1);
      const float* qp = a.ori.p + (int64_t)b * a.ori.bs + (int64_t)j * a.ori.ps;
      g2[0] = wc * (x[0] - qp[0]);
      g2[1] = wc * (x[1] - qp[a.ori.cs]);
      g2[2] = wc * (x[2] - qp[2 * a.ori.cs]);
    }
    if (knn) {
      float own[3] = {0.f, 0.f, 0.f};
      if (s_val[p] > thr) {
        for (int e = 1; e < K1; ++e) {
          const int j = min(max(ib[(int64_t)p * K1 + e], 0), L - 1);
          own[0] += w * (x[0] - sx[j]);
          own[1] += w * (x[1] - sy[j]);
          own[2] += w * (x[2] - sz[j]);
        }
      }
      g2[0] += own[0] + ax[p];
      g2[1] += own[1] + ay[p];
      g2[2] += own[2] + az[p];
    }
    const float* gp = a.g.p + (int64_t)b * a.g.bs + (int64_t)p * a.g.ps;
    float* mp = a.m.p + (int64_t)b * a.m.bs + (int64_t)p * a.m.ps;
    float* vp = a.v.p + (int64_t)b * a.v.bs + (int64_t)p * a.v.ps;
    float nw[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float g = gp[c * a.g.cs] + g2[c];
      float mm = mp[c * a.m.cs], vv = vp[c * a.v.cs];
      nw[c] = adam_element(ad, x[c], g, mm, vv);
      mp[c * a.m.cs] = mm;
      vp[c * a.v.cs] = vv;
    }
    float dx = nw[0] - o[0], dy = nw[1] - o[1], dz = nw[2] - o[2];
    float nx = 0.f, ny = 0.f, nz = 0.f;
    if (a.clip_mode == 1) {
      const float* n = nrm.p + (int64_t)b * nrm.bs + (int64_t)p * nrm.ps;
      nx = n[0], ny = n[nrm.cs], nz = n[2 * nrm.cs];
    }
    project_clip(dx, dy, dz, a.clip_mode == 1, nx, ny, nz, a.budget);
    float* xp = a.adv.p + (int64_t)b * a.adv.bs + (int64_t)p * a.adv.ps;
    xp[0] = o[0] + dx;
    xp[a.adv.cs] = o[1] + dy;
    xp[2 * a.adv.cs] = o[2] + dz;
    if constexpr (RAGGED) {
      if (p == 0) s_pad[0] = o[0] + dx, s_pad[1] = o[1] + dy, s_pad[2] = o[2] + dz;      // thread 0 owns point 0
    }
  }
  if constexpr (RAGGED) {
    // re-padding: adv's rows from L on take the new point 0, through LDS behind the barrier (no thread re-reads global
    // memory another thread of the workgroup writes)
    __syncthreads();
    const float n0[3] = {s_pad[0], s_pad[1], s_pad[2]};
    for (int p = L + tid; p < N; p += kKuThreads) {
      float* xp = a.adv.p + (int64_t)b * a.adv.bs + (int64_t)p * a.adv.ps;
      xp[0] = n0[0], xp[a.adv.cs] = n0[1], xp[2 * a.adv.cs] = n0[2];
    }
  }
}

}  // namespace pc3d

using namespace pc3d;

extern "C" int pc3d_knn_attack_update_f32(float* adv, int64_t a_bs, int64_t a_ps, int64_t a_cs,
                                          const float* ori, int64_t o_bs, int64_t o_ps, int64_t o_cs,
                                          const float* normal, int64_t n_bs, int64_t n_ps, int64_t n_cs,
                                          const float* g, int64_t g_bs, int64_t g_ps, int64_t g_cs, float* m, float* v,
                                          int B, int N, int k, const float* knn_d, const int32_t* knn_idx,
                                          const int32_t* nn_idx, double lr, double beta1, double beta2, double eps,
                                          float budget, int clip_mode, float alpha, float c_chamfer, float c_knn,
                                          const int32_t* step_dev, int step_host, void* stream) {
  PC3D_REQUIRE(B >= 0 && N >= 1 && N <= kKuMaxPoints, "pc3d_knn_attack_update_f32: bad sizes B=%d N=%d (1 <= N <= %d)", B, N,
               kKuMaxPoints);
  PC3D_REQUIRE(k >= 0 && k <= 63, "pc3d_knn_attack_update_f32: k=%d out of range [0,63]", k);
  PC3D_REQUIRE(step_dev != nullptr || step_host >= 1, "pc3d_knn_attack_update_f32: step_host must be >= 1 without a device counter");
  PC3D_REQUIRE(clip_mode == 0 || clip_mode == 1, "pc3d_knn_attack_update_f32: clip_mode=%d not in {0,1}", clip_mode);
  const bool knn = k >= 1 && c_knn != 0.f;
  PC3D_REQUIRE(!knn || k + 1 <= N, "pc3d_knn_attack_update_f32: k + 1 = %d neighbours of N=%d points", k + 1, N);
  if (B == 0) return PC3D_OK;
  PC3D_REQUIRE(adv && ori && g && m && v, "pc3d_knn_attack_update_f32: null pointer");
  PC3D_REQUIRE(!knn || (knn_d && knn_idx), "pc3d_knn_attack_update_f32: the kNN term needs knn_d and knn_idx");
  PC3D_REQUIRE(c_chamfer == 0.f || nn_idx != nullptr, "pc3d_knn_attack_update_f32: the Chamfer term needs nn_idx");
  KnnUpdArgs a{{adv, a_bs, a_ps, a_cs}, {ori, o_bs, o_ps, o_cs}, {normal, n_bs, n_ps, n_cs}, {g, g_bs, g_ps, g_cs},
               {m, a_bs, a_ps, a_cs}, {v, a_bs, a_ps, a_cs}, N, k + 1, knn_d, knn_idx, nn_idx, lr, beta1, beta2, (float)eps,
               budget, clip_mode, alpha, c_chamfer, c_knn, step_dev, step_host};
  const size_t lds = knn_upd_lds_bytes(N);
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(knn_attack_update_kernel<false>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)knn_upd_lds_bytes(kKuMaxPoints));
    if (e != hipSuccess) {
      set_error("pc3d_knn_attack_update_f32: LDS opt-in failed: %s", hipGetErrorString(e));
      return (int)e;
    }
  }
  hipLaunchKernelGGL(knn_attack_update_kernel<false>, dim3(B), dim3(kKuThreads), lds, as_stream(stream), a);
  PC3D_LAUNCH_CHECK("pc3d_knn_attack_update_f32");
  return PC3D_OK;
}

extern "C" int pc3d_knn_attack_update_ragged_f32(float* adv, int64_t a_bs, int64_t a_ps, int64_t a_cs,
                                                 const float* ori, int64_t o_bs, int64_t o_ps, int64_t o_cs,
                                                 const float* normal, int64_t n_bs, int64_t n_ps, int64_t n_cs,
                                                 const float* g, int64_t g_bs, int64_t g_ps, int64_t g_cs, float* m, float* v,
                                                 int B, int N, int k, const int32_t* lengths, const float* knn_d,
                                                 const int32_t* knn_idx, const int32_t* nn_idx, double lr, double beta1,
                                                 double beta2, double eps, float budget, int clip_mode, float alpha,
                                                 const float* c_chamfer, const float* c_knn, const int32_t* step_dev,
                                                 int step_host, void* stream) {
  const char* nm = "pc3d_knn_attack_update_ragged_f32";
  PC3D_REQUIRE(B >= 0 && N >= 1 && N <= kKuMaxPoints, "%s: bad sizes B=%d N=%d (1 <= N <= %d)", nm, B, N, kKuMaxPoints);
  PC3D_REQUIRE(k >= 0 && k <= 63, "%s: k=%d out of range [0,63]", nm, k);
  PC3D_REQUIRE(step_dev != nullptr || step_host >= 1, "%s: step_host must be >= 1 without a device counter", nm);
  PC3D_REQUIRE(clip_mode == 0 || clip_mode == 1, "%s: clip_mode=%d not in {0,1}", nm, clip_mode);
  PC3D_REQUIRE(k == 0 || k + 1 <= N, "%s: k + 1 = %d neighbours of N=%d points", nm, k + 1, N);
  if (B == 0) return PC3D_OK;
  // the per-cloud constants are device data: whether a cloud has a kNN or a Chamfer term is not known here
  PC3D_REQUIRE(adv && ori && g && m && v && lengths && c_chamfer && c_knn && nn_idx, "%s: null pointer", nm);
  PC3D_REQUIRE(k == 0 || (knn_d && knn_idx), "%s: k >= 1 needs knn_d and knn_idx", nm);
  KnnUpdRaggedArgs a{};
  static_cast<KnnUpdArgs&>(a) = KnnUpdArgs{{adv, a_bs, a_ps, a_cs}, {ori, o_bs, o_ps, o_cs}, {normal, n_bs, n_ps, n_cs},
                                           {g, g_bs, g_ps, g_cs}, {m, a_bs, a_ps, a_cs}, {v, a_bs, a_ps, a_cs}, N, k + 1,
                                           knn_d, knn_idx, nn_idx, lr, beta1, beta2, (float)eps, budget, clip_mode, alpha,
                                           0.f, 0.f, step_dev, step_host};
  a.lengths = lengths, a.c_ch_b = c_chamfer, a.c_knn_b = c_knn;
  const size_t lds = knn_upd_lds_bytes(N);      // from the capacity: the lengths are device data
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(knn_attack_update_kernel<true>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)knn_upd_lds_bytes(kKuMaxPoints));
    if (e != hipSuccess) {
      set_error("%s: LDS opt-in failed: %s", nm, hipGetErrorString(e));
      return (int)e;
    }
  }
  hipLaunchKernelGGL(knn_attack_update_kernel<true>, dim3(B), dim3(kKuThreads), lds, as_stream(stream), a);
  PC3D_LAUNCH_CHECK(nm);
  return PC3D_OK;
}
