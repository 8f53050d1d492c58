// The shape-invariant white-box attack (attack/SIadv/SIadv_attack.py of the reference, shape_invariant_ifgm): I-FGM in
// the tangent frame of every point. Three kernels:
//   pca_normal  per point, the unit eigenvector of the smallest eigenvalue of the covariance of its K listed neighbours
//               (the point itself among them) about their own mean — what the reference asks of open3d's
//               estimate_normals(KDTreeSearchParamKNN(knn=20)) on the host, one cloud at a time, every step;
//   si_frame    the cloud the reference shows the victim, U^T (U (P + t)) - t, with the normals given or computed from
//               neighbour lists by the same device function (and handed on);
//   si_step     everything of one step that comes after the victim, for all clouds, in place: the spin-axis frame U,
//               the move along the frame's first two axes scaled by the cloud's gradient norm, the way back and the
//               clamp (normals given, or again from neighbour lists).
// The clouds are tiny (12 KB at N = 1024) and the step is a chain of dependent launches: one workgroup per cloud, so that
// a point's normal (20 gathers and a double-precision 3 x 3 solve) is computed once and the cloud-wide norm needs no
// second launch and no atomics.
#include "eig3_body.h"

namespace pc3d {

constexpr int SI_T = 1024;             // threads of si_step's workgroup: one point each at N = 1024
constexpr int SI_WAVES = SI_T / kWave;
constexpr int SI_LDS_MAXN = 5120;      // normals staged in LDS up to this N (60 KB); beyond it through nrm_out

// Normal of one point from its K neighbour indices nb (the point itself included). Mean and covariance in double.
//   sign      the method leaves it free and the attack step does not depend on it (both the frame's third row and one
//             of the other two change sign with it, and they enter as U^T (. U)). Rule here: the last non-zero of
//             (x, y, z) is positive — the hemisphere z > 0, its rim closed by y > 0, then x > 0;
//   K < 3, a zero deviator or a zero cross product: (0, 0, 1), open3d's default normal;
//   an index outside [0, N) is never dereferenced: the point's normal is NaN (as pc3d_gather_points_f32 answers one).
__device__ __forceinline__ void pca_normal_point(const float* __restrict__ xb, int64_t ps, int64_t cs,
                                                 const int32_t* __restrict__ nb, int K, int N, float& ox, float& oy, float& oz) {
  bool bad = false;
  double mx = 0.0, my = 0.0, mz = 0.0;
  for (int j = 0; j < K; ++j) {
    int q = nb[j];
    if ((unsigned)q >= (unsigned)N) bad = true, q = 0;
    const float* p = xb + (int64_t)q * ps;
    mx += (double)p[0], my += (double)p[cs], mz += (double)p[2 * cs];
  }
  const double ik = 1.0 / (double)K;
  mx *= ik, my *= ik, mz *= ik;
  double c00 = 0, c01 = 0, c02 = 0, c11 = 0, c12 = 0, c22 = 0;
  for (int j = 0; j < K; ++j) {
    int q = nb[j];
    if ((unsigned)q >= (unsigned)N) q = 0;
    const float* p = xb + (int64_t)q * ps;
    const double dx = (double)p[0] - mx, dy = (double)p[cs] - my, dz = (double)p[2 * cs] - mz;
    c00 += dx * dx, c01 += dx * dy, c02 += dx * dz;
    c11 += dy * dy, c12 += dy * dz, c22 += dz * dz;
  }
  double nx = 0.0, ny = 0.0, nz = 1.0;
  if (K >= 3) eig3_smallest_vec(c00, c01, c02, c11, c12, c22, nx, ny, nz);
  if (nz < 0.0 || (nz == 0.0 && (ny < 0.0 || (ny == 0.0 && nx < 0.0)))) nx = -nx, ny = -ny, nz = -nz;
  const float nan = __builtin_nanf("");
  ox = bad ? nan : (float)nx, oy = bad ? nan : (float)ny, oz = bad ? nan : (float)nz;
}

struct PcaNormalArgs {
  PtsView x;
  const int32_t* idx;   // [B,N,K], self included
  int N, K;
  PtsViewMut out;
};

__global__ __launch_bounds__(256) void pca_normal_kernel(PcaNormalArgs a) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.N) return;
  float nx, ny, nz;
  pca_normal_point(a.x.p + (int64_t)b * a.x.bs, a.x.ps, a.x.cs, a.idx + ((int64_t)b * a.N + i) * a.K, a.K, a.N, nx, ny, nz);
  float* o = a.out.p + (int64_t)b * a.out.bs + (int64_t)i * a.out.ps;
  o[0] = nx, o[a.out.cs] = ny, o[2 * a.out.cs] = nz;
}

// The spin-axis matrix U of one normal, row-major (get_spin_axis_matrix, SIadv_attack.py:217-247), as written there: the
// rows for |z^2 - 1| < 1e-4 are chosen BEFORE anything divides by sqrt(1 - z^2).
__device__ __forceinline__ void si_frame(float x, float y, float z, float* u) {
  if (__builtin_fabsf(z * z - 1.f) < 1e-4f) {
    const float r = 0.70710678118654752f;        // 1 / sqrt(2)
    u[0] = r, u[1] = -r, u[2] = 0.f;
    u[3] = z * r, u[4] = z * r, u[5] = 0.f;
    u[6] = 0.f, u[7] = 0.f, u[8] = z;
  } else {
    const float den = __builtin_sqrtf(1.f - z * z);
    u[0] = y / den, u[1] = -x / den, u[2] = 0.f;
    u[3] = x * z / den, u[4] = y * z / den, u[5] = -den;
    u[6] = x, u[7] = y, u[8] = z;
  }
}

// g' = U g of one point, third component dropped (:310-311; g' = U g is the chain rule through P = U^T P' - t)
__device__ __forceinline__ void si_grad(const float* u, float gx, float gy, float gz, float& hx, float& hy) {
  hx = u[0] * gx + u[1] * gy + u[2] * gz;
  hy = u[3] * gx + u[4] * gy + u[5] * gz;
}

// t = (P . n) n and P' = U (P + t) of one point (get_transformed_point_cloud, :250-263)
__device__ __forceinline__ void si_to_frame(const float* u, float px, float py, float pz, float nx, float ny, float nz,
                                            float* t3, float* r3) {
  const float dotp = px * nx + py * ny + pz * nz;
  t3[0] = dotp * nx, t3[1] = dotp * ny, t3[2] = dotp * nz;
  const float qx = px + t3[0], qy = py + t3[1], qz = pz + t3[2];
  r3[0] = u[0] * qx + u[1] * qy + u[2] * qz;
  r3[1] = u[3] * qx + u[4] * qy + u[5] * qz;
  r3[2] = u[6] * qx + u[7] * qy + u[8] * qz;
}
// coordinate c of P = U^T P' - t (get_original_point_cloud, :266-276)
__device__ __forceinline__ float si_from_frame(const float* u, const float* r3, const float* t3, int c) {
  return (u[c] * r3[0] + u[3 + c] * r3[1] + u[6 + c] * r3[2]) - t3[c];
}

struct SiFrameArgs {
  PtsView x, nrm;        // nrm.p null: normals from idx
  const int32_t* idx;
  int K, N;
  PtsViewMut xe, nout;   // the cloud the victim is shown; the normals used (p may be null)
};

// The cloud the reference hands to the victim (:293-298): not P but U^T (U (P + t)) - t. Away from the rewritten rows of
// U that is P up to rounding; at those rows U is not the frame of n and the point is displaced by up to ~1e-4 |P|.
__global__ __launch_bounds__(256) void si_frame_kernel(SiFrameArgs a) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.N) return;
  const float* xb = a.x.p + (int64_t)b * a.x.bs;
  float nx, ny, nz;
  if (a.nrm.p) {
    const float* np_ = a.nrm.p + (int64_t)b * a.nrm.bs + (int64_t)i * a.nrm.ps;
    nx = np_[0], ny = np_[a.nrm.cs], nz = np_[2 * a.nrm.cs];
  } else {
    pca_normal_point(xb, a.x.ps, a.x.cs, a.idx + ((int64_t)b * a.N + i) * a.K, a.K, a.N, nx, ny, nz);
  }
  const float* xp = xb + (int64_t)i * a.x.ps;
  float u[9], t3[3], r3[3];
  si_frame(nx, ny, nz, u);
  si_to_frame(u, xp[0], xp[a.x.cs], xp[2 * a.x.cs], nx, ny, nz, t3, r3);
  float* ep = a.xe.p + (int64_t)b * a.xe.bs + (int64_t)i * a.xe.ps;
#pragma unroll
  for (int c = 0; c < 3; ++c) ep[c * a.xe.cs] = si_from_frame(u, r3, t3, c);
  if (a.nout.p) {
    float* no = a.nout.p + (int64_t)b * a.nout.bs + (int64_t)i * a.nout.ps;
    no[0] = nx, no[a.nout.cs] = ny, no[2 * a.nout.cs] = nz;
  }
}

struct SiStepArgs {
  PtsViewMut x;          // the iterate, updated in place
  PtsView ori, g, nrm;   // nrm.p null: normals from idx
  const int32_t* idx;    // [B,N,K] or null
  int K;
  PtsViewMut nout;       // the normals used (p may be null)
  int N, lds_stage;
  float cstep, eps;      // step_size * sqrt(3 * 1024); the clamp
};

__global__ __launch_bounds__(SI_T) void si_step_kernel(SiStepArgs a) {
  extern __shared__ float si_lds[];                 // [3][N] normals (idx mode with lds_stage)
  __shared__ float s_part[SI_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  float* xb = a.x.p + (int64_t)b * a.x.bs;
  const float* gb = a.g.p + (int64_t)b * a.g.bs;
  // where pass 2 finds the normals pass 1 used: the caller's, the LDS stage, or nrm_out
  const float* nb;
  int64_t nps, ncs;
  if (a.nrm.p) {
    nb = a.nrm.p + (int64_t)b * a.nrm.bs, nps = a.nrm.ps, ncs = a.nrm.cs;
  } else if (a.lds_stage) {
    nb = si_lds, nps = 1, ncs = a.N;
  } else {
    nb = a.nout.p + (int64_t)b * a.nout.bs, nps = a.nout.ps, ncs = a.nout.cs;
  }
  // pass 1: normals (idx mode; this is the last read of any OTHER point's coordinates) and the cloud's sum of g'^2
  float acc = 0.f;
  for (int n = tid; n < a.N; n += SI_T) {
    float nx, ny, nz;
    if (a.nrm.p) {
      const float* np_ = nb + (int64_t)n * nps;
      nx = np_[0], ny = np_[ncs], nz = np_[2 * ncs];
    } else {
      pca_normal_point(xb, a.x.ps, a.x.cs, a.idx + ((int64_t)b * a.N + n) * a.K, a.K, a.N, nx, ny, nz);
      float* ns = const_cast<float*>(nb) + (int64_t)n * nps;
      ns[0] = nx, ns[ncs] = ny, ns[2 * ncs] = nz;
    }
    const float* gp = gb + (int64_t)n * a.g.ps;
    float u[9], hx, hy;
    si_frame(nx, ny, nz, u);
    si_grad(u, gp[0], gp[a.g.cs], gp[2 * a.g.cs], hx, hy);
    acc += hx * hx + hy * hy;
  }
  // fixed order, set by SI_T alone: a thread's points ascending, the wave's xor tree, the wave sums in wave order
  acc = wave_sum(acc);
  if (lane == 0) s_part[wave] = acc;
  __syncthreads();                                  // also: every read of the old iterate is done before any write below
  float ss = s_part[0];
#pragma unroll
  for (int w = 1; w < SI_WAVES; ++w) ss += s_part[w];
  const float denom = __builtin_sqrtf(ss) + 1e-9f;
  // pass 2: P' = U (P + t), P' -= c g' / (|g'| + 1e-9), P = U^T P' - t, clamp to ori +- eps (:293-320)
  const float* ob = a.ori.p + (int64_t)b * a.ori.bs;
  for (int n = tid; n < a.N; n += SI_T) {
    const float* np_ = nb + (int64_t)n * nps;
    const float nx = np_[0], ny = np_[ncs], nz = np_[2 * ncs];
    float* xp = xb + (int64_t)n * a.x.ps;
    const float* gp = gb + (int64_t)n * a.g.ps;
    const float* op = ob + (int64_t)n * a.ori.ps;
    const float px = xp[0], py = xp[a.x.cs], pz = xp[2 * a.x.cs];
    float u[9], hx, hy;
    si_frame(nx, ny, nz, u);
    si_grad(u, gp[0], gp[a.g.cs], gp[2 * a.g.cs], hx, hy);
    float t3[3], r3[3];
    si_to_frame(u, px, py, pz, nx, ny, nz, t3, r3);
    r3[0] = r3[0] - (a.cstep * hx) / denom;
    r3[1] = r3[1] - (a.cstep * hy) / denom;
    const float o3[3] = {op[0], op[a.ori.cs], op[2 * a.ori.cs]};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float d = si_from_frame(u, r3, t3, c) - o3[c];
      const float dc = d < -a.eps ? -a.eps : (d > a.eps ? a.eps : d);     // NaN stays NaN, as torch.clamp
      xp[c * a.x.cs] = o3[c] + dc;
    }
    if (a.nout.p && nb != a.nout.p + (int64_t)b * a.nout.bs) {
      float* no = a.nout.p + (int64_t)b * a.nout.bs + (int64_t)n * a.nout.ps;
      no[0] = nx, no[a.nout.cs] = ny, no[2 * a.nout.cs] = nz;
    }
  }
}

}  // namespace pc3d

using namespace pc3d;

extern "C" int pc3d_pca_normal_f32(const float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs, const int32_t* idx, int B,
                                   int N, int K, float* out, int64_t o_bs, int64_t o_ps, int64_t o_cs, void* stream) {
  PC3D_REQUIRE(B >= 0 && N >= 1 && K >= 1, "pc3d_pca_normal_f32: bad sizes B=%d N=%d K=%d", B, N, K);
  PC3D_REQUIRE(B <= 65535, "pc3d_pca_normal_f32: B=%d exceeds grid.y limit", B);
  if (B == 0) return PC3D_OK;
  PC3D_REQUIRE(x && idx && out, "pc3d_pca_normal_f32: null pointer");
  PC3D_REQUIRE(x != out, "pc3d_pca_normal_f32: out must not alias x (a point reads its neighbours)");
  PcaNormalArgs a{{x, x_bs, x_ps, x_cs}, idx, N, K, {out, o_bs, o_ps, o_cs}};
  hipLaunchKernelGGL(pca_normal_kernel, dim3(cdiv(N, 256), B), dim3(256), 0, as_stream(stream), a);
  PC3D_LAUNCH_CHECK("pc3d_pca_normal_f32");
  return PC3D_OK;
}

extern "C" int pc3d_si_frame_f32(const float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs,
                                 const float* nrm, int64_t n_bs, int64_t n_ps, int64_t n_cs,
                                 const int32_t* idx, int K, int B, int N,
                                 float* xe, int64_t e_bs, int64_t e_ps, int64_t e_cs,
                                 float* nrm_out, int64_t no_bs, int64_t no_ps, int64_t no_cs, void* stream) {
  PC3D_REQUIRE(B >= 0 && N >= 1, "pc3d_si_frame_f32: bad sizes B=%d N=%d", B, N);
  PC3D_REQUIRE(B <= 65535, "pc3d_si_frame_f32: B=%d exceeds grid.y limit", B);
  PC3D_REQUIRE((nrm != nullptr) != (idx != nullptr), "pc3d_si_frame_f32: give either the normals nrm or the neighbour lists idx");
  PC3D_REQUIRE(idx == nullptr || K >= 1, "pc3d_si_frame_f32: bad K=%d", K);
  if (B == 0) return PC3D_OK;
  PC3D_REQUIRE(x && xe, "pc3d_si_frame_f32: null pointer");
  PC3D_REQUIRE(xe != x && nrm_out != x && (nrm_out == nullptr || (nrm_out != nrm && nrm_out != xe)),
               "pc3d_si_frame_f32: xe and nrm_out must not alias the inputs or each other (a point reads its neighbours)");
  SiFrameArgs a{{x, x_bs, x_ps, x_cs}, {nrm, n_bs, n_ps, n_cs}, idx, K, N, {xe, e_bs, e_ps, e_cs}, {nrm_out, no_bs, no_ps, no_cs}};
  hipLaunchKernelGGL(si_frame_kernel, dim3(cdiv(N, 256), B), dim3(256), 0, as_stream(stream), a);
  PC3D_LAUNCH_CHECK("pc3d_si_frame_f32");
  return PC3D_OK;
}

extern "C" int pc3d_si_step_f32(float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs,
                                const float* ori, int64_t o_bs, int64_t o_ps, int64_t o_cs,
                                const float* g, int64_t g_bs, int64_t g_ps, int64_t g_cs,
                                const float* nrm, int64_t n_bs, int64_t n_ps, int64_t n_cs,
                                const int32_t* idx, int K, int B, int N,
                                float* nrm_out, int64_t no_bs, int64_t no_ps, int64_t no_cs,
                                double step_size, double eps, void* stream) {
  PC3D_REQUIRE(B >= 0 && N >= 1, "pc3d_si_step_f32: bad sizes B=%d N=%d", B, N);
  PC3D_REQUIRE((nrm != nullptr) != (idx != nullptr), "pc3d_si_step_f32: give either the normals nrm or the neighbour lists idx");
  PC3D_REQUIRE(idx == nullptr || K >= 1, "pc3d_si_step_f32: bad K=%d", K);
  PC3D_REQUIRE(eps >= 0.0, "pc3d_si_step_f32: eps must not be negative");
  if (B == 0) return PC3D_OK;
  PC3D_REQUIRE(x && ori && g, "pc3d_si_step_f32: null pointer");
  PC3D_REQUIRE(x != ori && x != g && x != nrm && x != nrm_out, "pc3d_si_step_f32: x (updated in place) must not alias ori, g, nrm or nrm_out");
  PC3D_REQUIRE(nrm_out == nullptr || nrm_out != nrm, "pc3d_si_step_f32: nrm_out must not alias nrm");
  const int lds_stage = (idx != nullptr && N <= SI_LDS_MAXN) ? 1 : 0;
  PC3D_REQUIRE(idx == nullptr || lds_stage || nrm_out != nullptr,
               "pc3d_si_step_f32: N=%d > %d in idx mode needs nrm_out (the normals pass through it)", N, SI_LDS_MAXN);
  SiStepArgs a{{x, x_bs, x_ps, x_cs}, {ori, o_bs, o_ps, o_cs}, {g, g_bs, g_ps, g_cs}, {nrm, n_bs, n_ps, n_cs}, idx, K,
               {nrm_out, no_bs, no_ps, no_cs}, N, lds_stage, (float)(step_size * sqrt(3.0 * 1024.0)), (float)eps};
  const size_t lds = lds_stage ? (size_t)3 * N * sizeof(float) : 0;
  hipLaunchKernelGGL(si_step_kernel, dim3((unsigned)B), dim3(SI_T), lds, as_stream(stream), a);
  PC3D_LAUNCH_CHECK("pc3d_si_step_f32");
  return PC3D_OK;
}
