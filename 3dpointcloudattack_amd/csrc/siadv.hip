// The shape-invariant white-box attack (attack/SIadv/SIadv_attack.py of the reference, shape_invariant_ifgm): I-FGM in
// the tangent frame of every point. Three kernels (the two of the query attacks, query_step and si_rank, follow them below):
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

// Clouds of different sizes in one batch (the three _ragged entries): cloud b counts L = clamp(lengths[b], 1, N) points,
// lengths int32 [B] read as data, and N is the capacity: the row stride of idx and of the LDS stage.
struct PcaNormalRaggedArgs : PcaNormalArgs { const int32_t* lengths; };
template <bool RAGGED> struct PcaNormalArgsOf { using type = PcaNormalArgs; };
template <> struct PcaNormalArgsOf<true> { using type = PcaNormalRaggedArgs; };

__device__ __forceinline__ int si_ragged_len(const int32_t* lengths, int b, int N) { return min(max(lengths[b], 1), N); }

// RAGGED: a row i < L is the dense row of the cloud alone at N = L (a neighbour index is checked against L); a row i >= L
// repeats row 0's arithmetic on row 0's inputs — the same instructions on the same values, the same bits — and stores it
// at i: the padding rows of out are copies of row 0's normal, and no row >= L of x or idx is read. The dense instantiation
// compiles to the kernel it was before RAGGED existed (the parameter is a type of its own).
template <bool RAGGED>
__global__ __launch_bounds__(256) void pca_normal_kernel(typename PcaNormalArgsOf<RAGGED>::type a) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.N) return;
  int L = a.N, r = i;
  if constexpr (RAGGED) L = si_ragged_len(a.lengths, b, a.N), r = i < L ? i : 0;
  float nx, ny, nz;
  pca_normal_point(a.x.p + (int64_t)b * a.x.bs, a.x.ps, a.x.cs, a.idx + ((int64_t)b * a.N + r) * a.K, a.K, L, nx, ny, nz);
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

struct SiFrameRaggedArgs : SiFrameArgs { const int32_t* lengths; };
template <bool RAGGED> struct SiFrameArgsOf { using type = SiFrameArgs; };
template <> struct SiFrameArgsOf<true> { using type = SiFrameRaggedArgs; };

// The cloud the reference hands to the victim (:293-298): not P but U^T (U (P + t)) - t. Away from the rewritten rows of
// U that is P up to rounding; at those rows U is not the frame of n and the point is displaced by up to ~1e-4 |P|.
// RAGGED: as in pca_normal_kernel — a row i >= L computes row 0 again and stores it at i, so that xe's (and nout's) padding rows
// are copies of their row 0 in every bit (what a pad_invariant victim is shown); rows >= L of x, nrm and idx are not read.
template <bool RAGGED>
__global__ __launch_bounds__(256) void si_frame_kernel(typename SiFrameArgsOf<RAGGED>::type a) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.N) return;
  int L = a.N, r = i;
  if constexpr (RAGGED) L = si_ragged_len(a.lengths, b, a.N), r = i < L ? i : 0;
  const float* xb = a.x.p + (int64_t)b * a.x.bs;
  float nx, ny, nz;
  if (a.nrm.p) {
    const float* np_ = a.nrm.p + (int64_t)b * a.nrm.bs + (int64_t)r * a.nrm.ps;
    nx = np_[0], ny = np_[a.nrm.cs], nz = np_[2 * a.nrm.cs];
  } else {
    pca_normal_point(xb, a.x.ps, a.x.cs, a.idx + ((int64_t)b * a.N + r) * a.K, a.K, L, nx, ny, nz);
  }
  const float* xp = xb + (int64_t)r * a.x.ps;
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

struct SiStepRaggedArgs : SiStepArgs { const int32_t* lengths; };
template <bool RAGGED> struct SiStepArgsOf { using type = SiStepArgs; };
template <> struct SiStepArgsOf<true> { using type = SiStepRaggedArgs; };

// RAGGED: both passes run over n < L with the dense thread-to-point mapping and the dense reduction order, so rows < L have
// the bits of the dense launch on the cloud alone at N = L (a.N stays the capacity: the row stride of idx and of the LDS
// stage). Rows >= L of ori, g, nrm and idx are never read; x's take the NEW row 0 and nout's row 0's normal, both handed
// over through LDS behind a barrier (row 0 is rewritten in place by thread 0 in the same pass).
template <bool RAGGED>
__global__ __launch_bounds__(SI_T) void si_step_kernel(typename SiStepArgsOf<RAGGED>::type a) {
  extern __shared__ float si_lds[];                 // [3][N] normals (idx mode with lds_stage)
  __shared__ float s_part[SI_WAVES + (RAGGED ? 6 : 0)];     // RAGGED: behind the wave sums, the new row 0 and its normal
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  int L = a.N;
  if constexpr (RAGGED) L = si_ragged_len(a.lengths, b, a.N);
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
  for (int n = tid; n < L; n += SI_T) {
    float nx, ny, nz;
    if (a.nrm.p) {
      const float* np_ = nb + (int64_t)n * nps;
      nx = np_[0], ny = np_[ncs], nz = np_[2 * ncs];
    } else {
      pca_normal_point(xb, a.x.ps, a.x.cs, a.idx + ((int64_t)b * a.N + n) * a.K, a.K, L, nx, ny, nz);
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
  for (int n = tid; n < L; n += SI_T) {
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
      if constexpr (RAGGED) {
        if (n == 0) s_part[SI_WAVES + c] = o3[c] + dc;                    // thread 0 owns row 0
      }
    }
    if constexpr (RAGGED) {
      if (n == 0) s_part[SI_WAVES + 3] = nx, s_part[SI_WAVES + 4] = ny, s_part[SI_WAVES + 5] = nz;
    }
    if (a.nout.p && nb != a.nout.p + (int64_t)b * a.nout.bs) {
      float* no = a.nout.p + (int64_t)b * a.nout.bs + (int64_t)n * a.nout.ps;
      no[0] = nx, no[a.nout.cs] = ny, no[2 * a.nout.cs] = nz;
    }
  }
  if constexpr (RAGGED) {
    // re-padding: no thread reads back from global memory what another thread of the workgroup writes
    __syncthreads();
    const float* p0 = s_part + SI_WAVES;
    const float x0 = p0[0], y0 = p0[1], z0 = p0[2], n0x = p0[3], n0y = p0[4], n0z = p0[5];
    for (int n = L + tid; n < a.N; n += SI_T) {
      float* xp = xb + (int64_t)n * a.x.ps;
      xp[0] = x0, xp[a.x.cs] = y0, xp[2 * a.x.cs] = z0;
      if (a.nout.p) {
        float* no = a.nout.p + (int64_t)b * a.nout.bs + (int64_t)n * a.nout.ps;
        no[0] = n0x, no[a.nout.cs] = n0y, no[2 * a.nout.cs] = n0z;
      }
    }
  }
}


// ---------------------------------------------------------------------------------------------------------------------
// The query attacks (simba_attack, simbapp_attack, shape_invariant_query_attack, SIadv_attack.py:343-624): one victim
// forward of the 2B candidate clouds per step, then query_step — the accept / reject decision of step i for every cloud
// and the two candidate clouds of step i + 1, one workgroup per cloud. Nothing is reduced across threads except inside a
// wave: EVERY wave computes both losses of its cloud from the 2 k log-probabilities itself (the same shuffles on the same
// values: the same bits), so the decision needs no LDS and the one barrier only separates the entry loads of the state
// words from thread 0's stores to them.
constexpr int QS_KPL = 4;              // log-probabilities per lane: k <= 256

// CWLoss(kappa = -999, tar = True) of one row held lane-strided in v[] (entry j of lane l: class l + 64 j; beyond k:
// -inf), as written in the reference: the target's entry is replaced by -10000, `other` is the largest (top = 1) or the
// fifth largest (top = 5) of the row, the loss max(other - real, -999). pred: the row's arg-max, the lowest index on a tie.
__device__ __forceinline__ void qs_row_loss(const float* v, int k, int lane, int label, int top, float& loss, int& pred) {
  float m[QS_KPL];
  float real = 0.f;
#pragma unroll
  for (int j = 0; j < QS_KPL; ++j) {
    m[j] = v[j];
    if (lane + 64 * j == label) real = v[j], m[j] = -10000.f;
  }
  real = wave_sum(real);               // one lane holds it, the others 0 (x + 0 is x; -0 becomes +0, the same number)
  float ov = 0.f;
  for (int r = 0; r <= top; ++r) {     // round 0: the raw row's arg-max (the prediction); rounds 1 .. top: the masked row
    float bv = -__builtin_inff();
    int bi = 0x7fffffff;
#pragma unroll
    for (int j = 0; j < QS_KPL; ++j) {
      const float c = r == 0 ? v[j] : m[j];
      const int ci = lane + 64 * j;
      if (ci < k && (c > bv || (c == bv && ci < bi))) bv = c, bi = ci;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float c = __shfl_xor(bv, o, 64);
      const int ci = __shfl_xor(bi, o, 64);
      if (c > bv || (c == bv && ci < bi)) bv = c, bi = ci;
    }
    if (r == 0) {
      pred = bi == 0x7fffffff ? 0 : bi;
    } else {
      ov = bv;
#pragma unroll
      for (int j = 0; j < QS_KPL; ++j)
        if (lane + 64 * j == bi) m[j] = -__builtin_inff();
    }
  }
  const float d = ov - real;
  loss = d > -999.f ? d : (d == d ? -999.f : d);      // torch.max(d, kappa): NaN stays NaN
}

struct QueryStepArgs {
  const float* logp;       // [2B,k]: the victim's output for cand, try 0 then try 1 of every cloud (null with init)
  const int64_t* label;
  int k, top;
  PtsViewMut st;           // the accepted state: the cloud (coordinate mode) or P' (frame mode)
  PtsView ori, nrm;        // frame mode (nrm.p != null): the clean cloud (t = (P . n) n is taken from it) and the normals
  const int32_t* tab;      // [B,L]: 3 * point + channel (coordinate mode) or the point (frame mode)
  int L;
  const float* dir;        // [B,N,3] (frame mode)
  const float* eps;        // the amount of try t at entry l of cloud b: eps[b * eps_bs + l * eps_ls + t]
  int64_t eps_bs, eps_ls;
  int32_t *pos, *done, *queries, *adv_target, *last_try;
  float* best;
  float* last_logp;        // [B,k]: the row of the last try evaluated
  PtsViewMut cand, last;   // [2B,.]; [B,.] the last candidate evaluated, written when the cloud latches (p may be null)
  int32_t* acc_trace;      // [B,L] or null: the accepted try of every entry handled (-1: neither)
  float* loss_trace;       // [B,L,2] or null
  int N, init;
};

__global__ __launch_bounds__(1024) void query_step_kernel(QueryStepArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1), T = blockDim.x;
  const bool frame = a.nrm.p != nullptr;
  const int E = frame ? a.N : 3 * a.N;                       // table entries are in [0, E)
  // entry loads, all issued before anything waits: the state words, the label, both rows
  int pos = a.pos[b];
  int done = a.done[b];
  float best = a.best[b];
  const int label = a.init ? 0 : (int)a.label[b];
  float v0[QS_KPL], v1[QS_KPL];
#pragma unroll
  for (int j = 0; j < QS_KPL; ++j) {
    const int c = lane + 64 * j;
    const bool in = !a.init && c < a.k;
    v0[j] = in ? a.logp[(int64_t)(2 * b) * a.k + c] : -__builtin_inff();
    v1[j] = in ? a.logp[(int64_t)(2 * b + 1) * a.k + c] : -__builtin_inff();
  }
  const bool live = !a.init && !done;
  const bool pos_ok = (unsigned)pos < (unsigned)a.L;
  // the entry this step decides and the one after it, with their amounts: one more round trip, together
  int e_cur = -1, e_nxt = -1;
  float ec0 = 0.f, ec1 = 0.f, en0 = 0.f, en1 = 0.f;
  const int pn = a.init ? pos : pos + 1;
  if (live && pos_ok) {
    e_cur = a.tab[(int64_t)b * a.L + pos];
    const float* ep = a.eps + (int64_t)b * a.eps_bs + (int64_t)pos * a.eps_ls;
    ec0 = ep[0], ec1 = ep[1];
  }
  if (!done && (unsigned)pn < (unsigned)a.L) {
    e_nxt = a.tab[(int64_t)b * a.L + pn];
    const float* ep = a.eps + (int64_t)b * a.eps_bs + (int64_t)pn * a.eps_ls;
    en0 = ep[0], en1 = ep[1];
  }
  __syncthreads();                                           // every thread has read the state words: thread 0 may store
  int acc = -1, bad = 0, latched = 0, ltry = 0;
  if (live) {
    if (!pos_ok || (unsigned)e_cur >= (unsigned)E || (unsigned)label >= (unsigned)a.k) {
      bad = 1;
    } else {
      float l0, l1;
      int p0, p1;
      qs_row_loss(v0, a.k, lane, label, a.top, l0, p0);
      qs_row_loss(v1, a.k, lane, label, a.top, l1, p1);
      acc = l0 > best ? 0 : (l1 > best ? 1 : -1);            // strict >; try 1 is only evaluated when try 0 was rejected
      ltry = acc == 0 ? 0 : 1;
      if (acc >= 0) best = acc == 0 ? l0 : l1;
      pos += 1;
      if (tid == 0) {
        a.queries[b] += acc == 0 ? 1 : 2;
        a.last_try[b] = ltry;
        if (acc >= 0) a.best[b] = best, a.adv_target[b] = acc == 0 ? p0 : p1;
        a.pos[b] = pos;
        if (a.acc_trace) a.acc_trace[(int64_t)b * a.L + pos - 1] = acc;
        if (a.loss_trace) {
          float* lt = a.loss_trace + ((int64_t)b * a.L + pos - 1) * 2;
          lt[0] = l0, lt[1] = l1;
        }
      }
      if (tid < kWave) {
#pragma unroll
        for (int j = 0; j < QS_KPL; ++j)
          if (lane + 64 * j < a.k) a.last_logp[(int64_t)b * a.k + lane + 64 * j] = ltry ? v1[j] : v0[j];
      }
      if (!(best < 0.f && pos < a.L)) latched = 1;
    }
  }
  // the next entry is checked before any candidate is built from it
  if (!done && !bad && !latched && (unsigned)e_nxt >= (unsigned)E) bad = 1;
  if (bad) {
    latched = 1;
    if (tid == 0) a.adv_target[b] = -2;
  }
  if (latched && tid == 0) a.done[b] = 1;
  const bool perturb = !done && !latched;
  const int np_ = perturb ? (frame ? e_nxt : e_nxt / 3) : -1, nc_ = perturb && !frame ? e_nxt % 3 : -1;   // next entry
  const int ap_ = acc >= 0 ? (frame ? e_cur : e_cur / 3) : -1, ac_ = acc >= 0 && !frame ? e_cur % 3 : -1;  // accepted entry
  const float ea = acc == 0 ? ec0 : ec1;
  float* sb = a.st.p + (int64_t)b * a.st.bs;
  float* c0 = a.cand.p + (int64_t)(2 * b) * a.cand.bs;
  float* c1 = c0 + a.cand.bs;
  const bool keep_last = a.last.p && live && !bad && latched;
  for (int n = tid; n < a.N; n += T) {
    if (keep_last) {                                         // before this point's candidates are overwritten
      const float* lc = (ltry ? c1 : c0) + (int64_t)n * a.cand.ps;
      float* lo = a.last.p + (int64_t)b * a.last.bs + (int64_t)n * a.last.ps;
#pragma unroll
      for (int c = 0; c < 3; ++c) lo[c * a.last.cs] = lc[c * a.cand.cs];
    }
    float* sp = sb + (int64_t)n * a.st.ps;
    float o0[3], o1[3];
    if (!frame) {
      float s[3];
      if (a.init || !live) {
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] = sp[c * a.st.cs];
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          s[c] = sp[c * a.st.cs];
          if (n == ap_ && c == ac_) s[c] = s[c] + ea, sp[c * a.st.cs] = s[c];      // points = points + pert
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const bool hit = n == np_ && c == nc_;
        o0[c] = hit ? s[c] + en0 : s[c];
        o1[c] = hit ? s[c] + en1 : s[c];
      }
    } else {
      const float* np3 = a.nrm.p + (int64_t)b * a.nrm.bs + (int64_t)n * a.nrm.ps;
      const float* op = a.ori.p + (int64_t)b * a.ori.bs + (int64_t)n * a.ori.ps;
      const float nx = np3[0], ny = np3[a.nrm.cs], nz = np3[2 * a.nrm.cs];
      float u[9], t3[3], r3[3];
      si_frame(nx, ny, nz, u);
      si_to_frame(u, op[0], op[a.ori.cs], op[2 * a.ori.cs], nx, ny, nz, t3, r3);
      if (a.init) {                                          // P' of the clean cloud
#pragma unroll
        for (int c = 0; c < 3; ++c) sp[c * a.st.cs] = r3[c];
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) r3[c] = sp[c * a.st.cs];
        if (n == ap_) {                                      // new_points = new_points + pert, pert = eps * direction
          const float* dp = a.dir + ((int64_t)b * a.N + n) * 3;
#pragma unroll
          for (int c = 0; c < 3; ++c) r3[c] = r3[c] + ea * dp[c], sp[c * a.st.cs] = r3[c];
        }
      }
      float q0[3] = {r3[0], r3[1], r3[2]}, q1[3] = {r3[0], r3[1], r3[2]};
      if (n == np_) {
        const float* dp = a.dir + ((int64_t)b * a.N + n) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) q0[c] = r3[c] + en0 * dp[c], q1[c] = r3[c] + en1 * dp[c];
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) o0[c] = si_from_frame(u, q0, t3, c), o1[c] = si_from_frame(u, q1, t3, c);
    }
    float* w0 = c0 + (int64_t)n * a.cand.ps;
    float* w1 = c1 + (int64_t)n * a.cand.ps;
#pragma unroll
    for (int c = 0; c < 3; ++c) w0[c * a.cand.cs] = o0[c], w1[c * a.cand.cs] = o1[c];
  }
}

// The sensitivity map of shape_invariant_query_attack (:553-563) for one cloud per workgroup: g' = U g with g'_z = 0, the
// ranking sqrt(g'_x^2 + g'_y^2), the directions g' / (ranking + 1e-16), and the points ordered by (ranking descending,
// index ascending) — Python's stable sorted(..., reverse=True) — by an ascending bitonic network over P = 2^p >= N
// 64-bit keys in LDS: the complement of the ranking's bits (a non-negative float orders as its bits do) above the index.
// All keys are distinct, so the result does not depend on how the network is scheduled. Pads sort to the end.
constexpr int kRankMaxPoints = 8192;   // 64 KB of keys

struct SiRankArgs {
  PtsView g, nrm;
  int N, P;
  float *gp, *key, *dir;   // [B,N,3] (may be null), [B,N], [B,N,3]
  int32_t* order;          // [B,N]
};

__global__ __launch_bounds__(1024) void si_rank_kernel(SiRankArgs a) {
  extern __shared__ uint64_t rk_keys[];
  const int b = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
  for (int n = tid; n < a.P; n += T) {
    uint64_t kk = ~0ull;
    if (n < a.N) {
      const float* gq = a.g.p + (int64_t)b * a.g.bs + (int64_t)n * a.g.ps;
      const float* nq = a.nrm.p + (int64_t)b * a.nrm.bs + (int64_t)n * a.nrm.ps;
      const float gx = gq[0], gy = gq[a.g.cs], gz = gq[2 * a.g.cs];           // six independent loads
      const float nx = nq[0], ny = nq[a.nrm.cs], nz = nq[2 * a.nrm.cs];
      float u[9], hx, hy;
      si_frame(nx, ny, nz, u);
      si_grad(u, gx, gy, gz, hx, hy);
      const float r = __builtin_sqrtf(hx * hx + hy * hy);
      const float den = r + 1e-16f;
      const int64_t o = (int64_t)b * a.N + n;
      a.key[o] = r;
      a.dir[o * 3] = hx / den, a.dir[o * 3 + 1] = hy / den, a.dir[o * 3 + 2] = 0.f / den;
      if (a.gp) a.gp[o * 3] = hx, a.gp[o * 3 + 1] = hy, a.gp[o * 3 + 2] = 0.f;
      kk = ((uint64_t)(~__builtin_bit_cast(uint32_t, r)) << 32) | (uint32_t)n;
    }
    rk_keys[n] = kk;
  }
  __syncthreads();
  for (int k = 2; k <= a.P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (a.P >> 1); t += T) {
        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
        const uint64_t x = rk_keys[lo], y = rk_keys[hi];
        const bool up = (lo & k) == 0;
        if ((x > y) == up) rk_keys[lo] = y, rk_keys[hi] = x;
      }
      __syncthreads();
    }
  for (int i = tid; i < a.N; i += T) a.order[(int64_t)b * a.N + i] = (int32_t)(rk_keys[i] & 0xffffffffull);
}

}  // namespace pc3d

using namespace pc3d;

// the checks, the argument block and the launch of a dense entry and its _ragged twin; ragged false: the dense kernel,
// lengths unused
static int pca_normal_launch(const char* nm, const float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs, const int32_t* idx, int B,
                             int N, int K, const int32_t* lengths, bool ragged, float* out, int64_t o_bs, int64_t o_ps,
                             int64_t o_cs, void* stream) {
  PC3D_REQUIRE(B >= 0 && N >= 1 && K >= 1, "%s: bad sizes B=%d N=%d K=%d", nm, B, N, K);
  PC3D_REQUIRE(B <= 65535, "%s: B=%d exceeds grid.y limit", nm, B);
  if (B == 0) return PC3D_OK;
  PC3D_REQUIRE(x && idx && out && (!ragged || lengths), "%s: null pointer", nm);
  PC3D_REQUIRE(x != out, "%s: out must not alias x (a point reads its neighbours)", nm);
  PcaNormalRaggedArgs a{{{x, x_bs, x_ps, x_cs}, idx, N, K, {out, o_bs, o_ps, o_cs}}, lengths};
  if (ragged)
    hipLaunchKernelGGL(pca_normal_kernel<true>, dim3(cdiv(N, 256), B), dim3(256), 0, as_stream(stream), a);
  else
    hipLaunchKernelGGL(pca_normal_kernel<false>, dim3(cdiv(N, 256), B), dim3(256), 0, as_stream(stream),
                       static_cast<const PcaNormalArgs&>(a));
  PC3D_LAUNCH_CHECK(nm);
  return PC3D_OK;
}

extern "C" int pc3d_pca_normal_f32(const float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs, const int32_t* idx, int B,
                                   int N, int K, float* out, int64_t o_bs, int64_t o_ps, int64_t o_cs, void* stream) {
  return pca_normal_launch("pc3d_pca_normal_f32", x, x_bs, x_ps, x_cs, idx, B, N, K, nullptr, false, out, o_bs, o_ps, o_cs,
                           stream);
}

extern "C" int pc3d_pca_normal_ragged_f32(const float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs, const int32_t* idx,
                                          int B, int N, int K, const int32_t* lengths, float* out, int64_t o_bs,
                                          int64_t o_ps, int64_t o_cs, void* stream) {
  return pca_normal_launch("pc3d_pca_normal_ragged_f32", x, x_bs, x_ps, x_cs, idx, B, N, K, lengths, true, out, o_bs, o_ps,
                           o_cs, stream);
}

static int si_frame_launch(const char* nm, const float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs,
                           const float* nrm, int64_t n_bs, int64_t n_ps, int64_t n_cs, const int32_t* idx, int K, int B, int N,
                           const int32_t* lengths, bool ragged, float* xe, int64_t e_bs, int64_t e_ps, int64_t e_cs,
                           float* nrm_out, int64_t no_bs, int64_t no_ps, int64_t no_cs, void* stream) {
  PC3D_REQUIRE(B >= 0 && N >= 1, "%s: bad sizes B=%d N=%d", nm, B, N);
  PC3D_REQUIRE(B <= 65535, "%s: B=%d exceeds grid.y limit", nm, B);
  PC3D_REQUIRE((nrm != nullptr) != (idx != nullptr), "%s: give either the normals nrm or the neighbour lists idx", nm);
  PC3D_REQUIRE(idx == nullptr || K >= 1, "%s: bad K=%d", nm, K);
  if (B == 0) return PC3D_OK;
  PC3D_REQUIRE(x && xe && (!ragged || lengths), "%s: null pointer", nm);
  PC3D_REQUIRE(xe != x && nrm_out != x && (nrm_out == nullptr || (nrm_out != nrm && nrm_out != xe)),
               "%s: xe and nrm_out must not alias the inputs or each other (a point reads its neighbours)", nm);
  SiFrameRaggedArgs a{{{x, x_bs, x_ps, x_cs}, {nrm, n_bs, n_ps, n_cs}, idx, K, N, {xe, e_bs, e_ps, e_cs},
                       {nrm_out, no_bs, no_ps, no_cs}}, lengths};
  if (ragged)
    hipLaunchKernelGGL(si_frame_kernel<true>, dim3(cdiv(N, 256), B), dim3(256), 0, as_stream(stream), a);
  else
    hipLaunchKernelGGL(si_frame_kernel<false>, dim3(cdiv(N, 256), B), dim3(256), 0, as_stream(stream),
                       static_cast<const SiFrameArgs&>(a));
  PC3D_LAUNCH_CHECK(nm);
  return PC3D_OK;
}

extern "C" int pc3d_si_frame_f32(const float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs,
                                 const float* nrm, int64_t n_bs, int64_t n_ps, int64_t n_cs,
                                 const int32_t* idx, int K, int B, int N,
                                 float* xe, int64_t e_bs, int64_t e_ps, int64_t e_cs,
                                 float* nrm_out, int64_t no_bs, int64_t no_ps, int64_t no_cs, void* stream) {
  return si_frame_launch("pc3d_si_frame_f32", x, x_bs, x_ps, x_cs, nrm, n_bs, n_ps, n_cs, idx, K, B, N, nullptr, false, xe,
                         e_bs, e_ps, e_cs, nrm_out, no_bs, no_ps, no_cs, stream);
}

extern "C" int pc3d_si_frame_ragged_f32(const float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs,
                                        const float* nrm, int64_t n_bs, int64_t n_ps, int64_t n_cs,
                                        const int32_t* idx, int K, int B, int N, const int32_t* lengths,
                                        float* xe, int64_t e_bs, int64_t e_ps, int64_t e_cs,
                                        float* nrm_out, int64_t no_bs, int64_t no_ps, int64_t no_cs, void* stream) {
  return si_frame_launch("pc3d_si_frame_ragged_f32", x, x_bs, x_ps, x_cs, nrm, n_bs, n_ps, n_cs, idx, K, B, N, lengths, true,
                         xe, e_bs, e_ps, e_cs, nrm_out, no_bs, no_ps, no_cs, stream);
}

static int si_step_launch(const char* nm, float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs,
                          const float* ori, int64_t o_bs, int64_t o_ps, int64_t o_cs,
                          const float* g, int64_t g_bs, int64_t g_ps, int64_t g_cs,
                          const float* nrm, int64_t n_bs, int64_t n_ps, int64_t n_cs, const int32_t* idx, int K, int B, int N,
                          const int32_t* lengths, bool ragged, float* nrm_out, int64_t no_bs, int64_t no_ps, int64_t no_cs,
                          double step_size, double eps, void* stream) {
  PC3D_REQUIRE(B >= 0 && N >= 1, "%s: bad sizes B=%d N=%d", nm, B, N);
  PC3D_REQUIRE((nrm != nullptr) != (idx != nullptr), "%s: give either the normals nrm or the neighbour lists idx", nm);
  PC3D_REQUIRE(idx == nullptr || K >= 1, "%s: bad K=%d", nm, K);
  PC3D_REQUIRE(eps >= 0.0, "%s: eps must not be negative", nm);
  if (B == 0) return PC3D_OK;
  PC3D_REQUIRE(x && ori && g && (!ragged || lengths), "%s: null pointer", nm);
  PC3D_REQUIRE(x != ori && x != g && x != nrm && x != nrm_out, "%s: x (updated in place) must not alias ori, g, nrm or nrm_out", nm);
  PC3D_REQUIRE(nrm_out == nullptr || nrm_out != nrm, "%s: nrm_out must not alias nrm", nm);
  const int lds_stage = (idx != nullptr && N <= SI_LDS_MAXN) ? 1 : 0;      // from the capacity: the lengths are device data
  PC3D_REQUIRE(idx == nullptr || lds_stage || nrm_out != nullptr,
               "%s: N=%d > %d in idx mode needs nrm_out (the normals pass through it)", nm, N, SI_LDS_MAXN);
  SiStepRaggedArgs a{{{x, x_bs, x_ps, x_cs}, {ori, o_bs, o_ps, o_cs}, {g, g_bs, g_ps, g_cs}, {nrm, n_bs, n_ps, n_cs}, idx, K,
                      {nrm_out, no_bs, no_ps, no_cs}, N, lds_stage, (float)(step_size * sqrt(3.0 * 1024.0)), (float)eps},
                     lengths};
  const size_t lds = lds_stage ? (size_t)3 * N * sizeof(float) : 0;
  if (ragged)
    hipLaunchKernelGGL(si_step_kernel<true>, dim3((unsigned)B), dim3(SI_T), lds, as_stream(stream), a);
  else
    hipLaunchKernelGGL(si_step_kernel<false>, dim3((unsigned)B), dim3(SI_T), lds, as_stream(stream), static_cast<const SiStepArgs&>(a));
  PC3D_LAUNCH_CHECK(nm);
  return PC3D_OK;
}

extern "C" int pc3d_si_step_f32(float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs,
                                const float* ori, int64_t o_bs, int64_t o_ps, int64_t o_cs,
                                const float* g, int64_t g_bs, int64_t g_ps, int64_t g_cs,
                                const float* nrm, int64_t n_bs, int64_t n_ps, int64_t n_cs,
                                const int32_t* idx, int K, int B, int N,
                                float* nrm_out, int64_t no_bs, int64_t no_ps, int64_t no_cs,
                                double step_size, double eps, void* stream) {
  return si_step_launch("pc3d_si_step_f32", x, x_bs, x_ps, x_cs, ori, o_bs, o_ps, o_cs, g, g_bs, g_ps, g_cs, nrm, n_bs, n_ps,
                        n_cs, idx, K, B, N, nullptr, false, nrm_out, no_bs, no_ps, no_cs, step_size, eps, stream);
}

extern "C" int pc3d_si_step_ragged_f32(float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs,
                                       const float* ori, int64_t o_bs, int64_t o_ps, int64_t o_cs,
                                       const float* g, int64_t g_bs, int64_t g_ps, int64_t g_cs,
                                       const float* nrm, int64_t n_bs, int64_t n_ps, int64_t n_cs,
                                       const int32_t* idx, int K, int B, int N, const int32_t* lengths,
                                       float* nrm_out, int64_t no_bs, int64_t no_ps, int64_t no_cs,
                                       double step_size, double eps, void* stream) {
  return si_step_launch("pc3d_si_step_ragged_f32", x, x_bs, x_ps, x_cs, ori, o_bs, o_ps, o_cs, g, g_bs, g_ps, g_cs, nrm, n_bs,
                        n_ps, n_cs, idx, K, B, N, lengths, true, nrm_out, no_bs, no_ps, no_cs, step_size, eps, stream);
}

extern "C" int pc3d_query_step_f32(const float* logp, int k, const int64_t* label, int top,
                                   float* st, int64_t s_bs, int64_t s_ps, int64_t s_cs,
                                   const float* ori, int64_t o_bs, int64_t o_ps, int64_t o_cs,
                                   const float* nrm, int64_t n_bs, int64_t n_ps, int64_t n_cs,
                                   const int32_t* tab, int L, const float* dir, const float* eps, int64_t eps_bs, int64_t eps_ls,
                                   int32_t* pos, float* best, int32_t* done, int32_t* queries, int32_t* adv_target,
                                   int32_t* last_try, float* last_logp,
                                   float* cand, int64_t c_bs, int64_t c_ps, int64_t c_cs,
                                   float* last, int64_t l_bs, int64_t l_ps, int64_t l_cs,
                                   int32_t* acc_trace, float* loss_trace, int B, int N, int init, void* stream) {
  PC3D_REQUIRE(B >= 0 && N >= 1 && L >= 1, "pc3d_query_step_f32: bad sizes B=%d N=%d L=%d", B, N, L);
  PC3D_REQUIRE(N <= 0x7fffffff / 3, "pc3d_query_step_f32: N=%d too large for the 3 N table entries", N);
  PC3D_REQUIRE(top == 1 || top == 5, "pc3d_query_step_f32: top must be 1 or 5, got %d", top);
  PC3D_REQUIRE(init || (k > top && k <= 64 * QS_KPL), "pc3d_query_step_f32: k=%d classes, need top < k <= %d", k, 64 * QS_KPL);
  PC3D_REQUIRE((ori != nullptr) == (nrm != nullptr) && (dir != nullptr) == (nrm != nullptr),
               "pc3d_query_step_f32: the frame mode takes ori, nrm and dir together, the coordinate mode none of them");
  if (B == 0) return PC3D_OK;
  PC3D_REQUIRE(st && tab && eps && pos && best && done && cand, "pc3d_query_step_f32: null pointer");
  PC3D_REQUIRE(init || (logp && label && queries && adv_target && last_try && last_logp), "pc3d_query_step_f32: null pointer");
  PC3D_REQUIRE(cand != st && cand != ori && cand != nrm && cand != last && st != ori && st != nrm && last != st,
               "pc3d_query_step_f32: st, cand and last must not alias each other or the inputs");
  QueryStepArgs a{logp, label, k, top, {st, s_bs, s_ps, s_cs}, {ori, o_bs, o_ps, o_cs}, {nrm, n_bs, n_ps, n_cs}, tab, L, dir,
                  eps, eps_bs, eps_ls, pos, done, queries, adv_target, last_try, best, last_logp,
                  {cand, c_bs, c_ps, c_cs}, {last, l_bs, l_ps, l_cs}, acc_trace, loss_trace, N, init ? 1 : 0};
  const int T = N >= 1024 ? 1024 : cdiv(N, kWave) * kWave;
  hipLaunchKernelGGL(query_step_kernel, dim3((unsigned)B), dim3(T), 0, as_stream(stream), a);
  PC3D_LAUNCH_CHECK("pc3d_query_step_f32");
  return PC3D_OK;
}

extern "C" int pc3d_si_rank_f32(const float* g, int64_t g_bs, int64_t g_ps, int64_t g_cs,
                                const float* nrm, int64_t n_bs, int64_t n_ps, int64_t n_cs, int B, int N,
                                float* gp, float* key, float* dir, int32_t* order, void* stream) {
  PC3D_REQUIRE(B >= 0 && N >= 1, "pc3d_si_rank_f32: bad sizes B=%d N=%d", B, N);
  PC3D_REQUIRE(N <= kRankMaxPoints, "pc3d_si_rank_f32: N=%d exceeds the limit of %d points (the keys are sorted in LDS)", N,
               kRankMaxPoints);
  if (B == 0) return PC3D_OK;
  PC3D_REQUIRE(g && nrm && key && dir && order, "pc3d_si_rank_f32: null pointer");
  int P = 2;
  while (P < N) P <<= 1;
  SiRankArgs a{{g, g_bs, g_ps, g_cs}, {nrm, n_bs, n_ps, n_cs}, N, P, gp, key, dir, order};
  const int T = P / 2 >= 1024 ? 1024 : (P / 2 < kWave ? kWave : P / 2);
  hipLaunchKernelGGL(si_rank_kernel, dim3((unsigned)B), dim3(T), (size_t)P * sizeof(uint64_t), as_stream(stream), a);
  PC3D_LAUNCH_CHECK("pc3d_si_rank_f32");
  return PC3D_OK;
}
