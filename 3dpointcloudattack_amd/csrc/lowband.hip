// K12d — the low band of the AOF graph Laplacian without a dense decomposition.
// Only V[:, :low_pass] enters AOF's low-frequency component and, V being orthonormal, hfc = adv - lfc: what the attack needs
// is the invariant subspace of the lowest `lp` eigenvalues of a sparse symmetric matrix (<= ~60 non-zeros a row), not all N
// eigenpairs of a dense one. Here: the Laplacian in CSR, Chebyshev-filtered block subspace iteration on a block of
// m = min(N, lp + guard) <= 128 columns (sparse matrix x block products), orthonormalisation through the Gram matrix's own
// eigendecomposition, Rayleigh-Ritz, both on an m x m parallel cyclic Jacobi solver that lives in one workgroup's LDS, and
// the re-projection onto the [B,N,lp] basis. A fixed launch sequence: no host synchronisation, no data-dependent launch
// count, no atomics on floats other than an exact maximum; every cloud is computed from its own data alone.
// tests/lowband_restatement.py restates the method on the CPU.
#include <math.h>

#include "pc3d_common.h"

namespace pc3d {

// ---------------------------------------------------------------------------------------------------------
// CSR of L = D - A: row i holds the off-diagonal entries -exp(-d^2) of the symmetrised mask (j in knn(i) or i in knn(j),
// self excluded), columns ascending; the diagonal is kept apart in deg. One wave per row scans the candidates j in
// order, 64 at a time: the position of an entry is a prefix count of the ballot, so the fill has no atomics.
// ---------------------------------------------------------------------------------------------------------
struct CsrArgs {
  PtsView x;
  const int32_t* idx;   // [B,N,K]
  int N, K, cap;
  int32_t* rowptr;      // [B,N+1]
  int32_t* col;         // [B,cap]
  float* val;           // [B,cap]
  float* deg;           // [B,N]
};

__device__ __forceinline__ bool csr_member(const int32_t* idx, int N, int K, int i, int j) {
  if (j >= N || j == i) return false;
  const int32_t* ri = idx + (int64_t)i * K;
  const int32_t* rj = idx + (int64_t)j * K;
  bool m = false;
  for (int t = 0; t < K; ++t) m |= ri[t] == j;
  if (!m)
    for (int t = 0; t < K; ++t) m |= rj[t] == i;
  return m;
}

__global__ __launch_bounds__(256) void csr_count_kernel(CsrArgs a) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= a.N) return;
  const int32_t* idx = a.idx + (int64_t)b * a.N * a.K;
  int cnt = 0;
  for (int j0 = 0; j0 < a.N; j0 += 64) cnt += __popcll(__ballot(csr_member(idx, a.N, a.K, i, j0 + lane)));
  if (lane == 0) a.rowptr[(int64_t)b * (a.N + 1) + i + 1] = cnt;
}

// counts -> row starts, in place: one workgroup per cloud, each thread a contiguous run of rows
__global__ __launch_bounds__(1024) void csr_scan_kernel(int32_t* rowptr, int N) {
  __shared__ int part[1024];
  int32_t* rp = rowptr + (int64_t)blockIdx.x * (N + 1);
  const int t = threadIdx.x, per = (N + 1023) / 1024;
  const int lo = min(N, t * per), hi = min(N, lo + per);
  int s = 0;
  for (int i = lo; i < hi; ++i) s += rp[i + 1];
  part[t] = s;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const int v = t >= o ? part[t - o] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int run = part[t] - s;     // exclusive prefix of this thread's run
  if (t == 0) rp[0] = 0;
  for (int i = lo; i < hi; ++i) {
    run += rp[i + 1];
    rp[i + 1] = run;
  }
}

__global__ __launch_bounds__(256) void csr_fill_kernel(CsrArgs a) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= a.N) return;
  const int32_t* idx = a.idx + (int64_t)b * a.N * a.K;
  const float* xb = a.x.p + (int64_t)b * a.x.bs;
  const float* pi = xb + (int64_t)i * a.x.ps;
  const float xi = pi[0], yi = pi[a.x.cs], zi = pi[2 * a.x.cs];
  int base = a.rowptr[(int64_t)b * (a.N + 1) + i];
  int32_t* col = a.col + (int64_t)b * a.cap;
  float* val = a.val + (int64_t)b * a.cap;
  float acc = 0.f;
  for (int j0 = 0; j0 < a.N; j0 += 64) {
    const int j = j0 + lane;
    const bool m = csr_member(idx, a.N, a.K, i, j);
    const unsigned long long mask = __ballot(m);
    if (m) {
      const float* pj = xb + (int64_t)j * a.x.ps;
      // the arithmetic of lap_edges_kernel: the squares make w(i,j) and w(j,i) the same bits
      const float dx = xi - pj[0], dy = yi - pj[a.x.cs], dz = zi - pj[2 * a.x.cs];
      const float w = -expf(-((dx * dx + dy * dy) + dz * dz));
      const int pos = base + __popcll(mask & ((1ull << lane) - 1ull));
      if (pos < a.cap) {      // a capacity too small shows in rowptr[N] > cap; nothing is written past it
        col[pos] = j;
        val[pos] = w;
      }
      acc += w;
    }
    base += __popcll(mask);
  }
  acc = wave_sum(acc);
  if (lane == 0) a.deg[(int64_t)b * a.N + i] = -acc;
}

// ---------------------------------------------------------------------------------------------------------
// The block iteration's kernels. A block is [B,N,m] fp32, row n contiguous.
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float lb_hash_unit(unsigned row, unsigned col, unsigned salt) {
  unsigned h = (row * 0x9E3779B1u) ^ (col * 0x85EBCA77u) ^ (salt * 0xC2B2AE3Du);
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return (float)(h >> 8) * 1.1920928955078125e-07f - 1.0f;     // [-1, 1)
}

// the start block (no cloud index in the hash: a cloud's basis does not depend on its place in the batch), resid = 0
__global__ __launch_bounds__(256) void lb_init_kernel(float* X, int N, int m, float* resid) {
  const int b = blockIdx.y;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e == 0) resid[b] = 0.f;
  if (e >= N * m) return;
  X[(int64_t)b * N * m + e] = lb_hash_unit((unsigned)(e / m), (unsigned)(e % m), 0u);
}

// ub[b] = 2 max_i deg_i (Gershgorin)
__global__ __launch_bounds__(256) void lb_maxdeg_kernel(const float* deg, int N, float* ub) {
  __shared__ float red[4];
  const int b = blockIdx.x;
  float v = 0.f;
  for (int i = threadIdx.x; i < N; i += 256) v = fmaxf(v, deg[(int64_t)b * N + i]);
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) ub[b] = 2.f * fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// The scaled three-term Chebyshev recurrence of one outer iteration as a table coef[b][k] = (alpha, beta, gamma):
//   Y_k = alpha (L Y_{k-1}) + beta Y_{k-1} + gamma Y_{k-2};   alpha = 0: the step copies.
// It damps [a, ub], grows below the cut a (the largest Ritz value of the previous iteration) and is 1 at the anchor a0
// (the smallest). The degree is cut where the gain over the block, T_k((c - a0) / e), would pass range_max.
__global__ void lb_coef_kernel(const float* theta, const float* ub, int m, int degree, float range_max, float cut_min,
                               float* coef, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const float hi = ub[b];
  const float a0 = fminf(theta[(int64_t)b * m], hi * 0.5f);
  const float a = fminf(fmaxf(theta[(int64_t)b * m + m - 1], a0 + cut_min * hi), hi * (1.f - cut_min));
  const float e = (hi - a) * 0.5f, c = (hi + a) * 0.5f;
  const float x0 = (c - a0) / e;
  int deff = (int)floorf(logf(2.f * range_max) / logf(x0 + sqrtf(x0 * x0 - 1.f)));
  deff = max(1, min(degree, deff));
  float* cf = coef + (int64_t)b * degree * 4;
  float sigma = e / (a0 - c);
  const float tau = 2.f / sigma;
  bool ok = hi > 0.f && e > 0.f && x0 > 1.f;     // an edgeless cloud (L = 0): every step copies
  for (int k = 1; k <= degree; ++k) {
    float al = 0.f, be = 1.f, ga = 0.f;
    if (ok && k == 1) {
      al = sigma / e;
      be = -c * al;
    } else if (ok && k <= deff) {
      const float sn = 1.f / (tau - sigma);
      al = 2.f * sn / e;
      be = -c * al;
      ga = -(sigma * sn);
      sigma = sn;
    }
    cf[4 * (k - 1) + 0] = al;
    cf[4 * (k - 1) + 1] = be;
    cf[4 * (k - 1) + 2] = ga;
    cf[4 * (k - 1) + 3] = 0.f;
  }
}

struct SpmmArgs {
  const int32_t* rowptr;
  const int32_t* col;
  const float* val;
  const float* deg;
  int N, cap, m;
  const float* Y;      // [B,N,m] the operand
  const float* P;      // [B,N,m] the recurrence's second-last block (MODE 1)
  float* out;          // [B,N,m]
  const float* coef;   // [B,degree,4] (MODE 1), already offset to the step
  int coef_stride;
  const float* theta;  // [B,m] (MODE 2)
  int lp;
  float* resid;        // [B] (MODE 2)
};

// One wave per row, the lane holds columns lane and lane + 64: out = L Y (MODE 0), the recurrence step (MODE 1), or
// resid = max |L u_j - theta_j u_j| over the rows and the columns j < lp (MODE 2; an exact maximum, so the atomic's order
// does not show). The row's sum runs in a fixed order: the diagonal, then the entries by ascending column.
template <int MODE>
__global__ __launch_bounds__(256) void lb_spmm_kernel(SpmmArgs a) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= a.N) return;
  const int m = a.m;
  const int64_t xo = (int64_t)b * a.N * m;
  const float* Y = a.Y + xo;
  const int c0 = lane, c1 = lane + 64;
  const bool h0 = c0 < m, h1 = c1 < m;
  float al = 1.f, be = 0.f, ga = 0.f;
  if (MODE == 1) {
    const float* cf = a.coef + (int64_t)b * a.coef_stride;
    al = cf[0], be = cf[1], ga = cf[2];
  }
  const float y0 = h0 ? Y[(int64_t)n * m + c0] : 0.f, y1 = h1 ? Y[(int64_t)n * m + c1] : 0.f;
  float s0 = 0.f, s1 = 0.f;
  if (MODE != 1 || al != 0.f) {
    const float d = a.deg[(int64_t)b * a.N + n];
    s0 = d * y0, s1 = d * y1;
    const int32_t* rp = a.rowptr + (int64_t)b * (a.N + 1);
    const int lo = min(rp[n], a.cap), hi = min(rp[n + 1], a.cap);
    const int32_t* col = a.col + (int64_t)b * a.cap;
    const float* val = a.val + (int64_t)b * a.cap;
    for (int p = lo; p < hi; ++p) {
      const int j = col[p];
      const float w = val[p];
      if ((unsigned)j >= (unsigned)a.N) continue;
      const float* yr = Y + (int64_t)j * m;
      if (h0) s0 = fmaf(w, yr[c0], s0);
      if (h1) s1 = fmaf(w, yr[c1], s1);
    }
  }
  if (MODE == 0) {
    if (h0) a.out[xo + (int64_t)n * m + c0] = s0;
    if (h1) a.out[xo + (int64_t)n * m + c1] = s1;
  } else if (MODE == 1) {
    float r0 = al * s0 + be * y0, r1 = al * s1 + be * y1;
    if (ga != 0.f) {
      const float* P = a.P + xo;
      if (h0) r0 += ga * P[(int64_t)n * m + c0];
      if (h1) r1 += ga * P[(int64_t)n * m + c1];
    }
    if (h0) a.out[xo + (int64_t)n * m + c0] = r0;
    if (h1) a.out[xo + (int64_t)n * m + c1] = r1;
  } else {
    float r = 0.f;
    if (c0 < a.lp) r = fabsf(s0 - a.theta[(int64_t)b * m + c0] * y0);
    if (c1 < a.lp) r = fmaxf(r, fabsf(s1 - a.theta[(int64_t)b * m + c1] * y1));
    r = wave_max(r);
    if (lane == 0 && r == r) atomicMax(reinterpret_cast<unsigned*>(a.resid + b), __builtin_bit_cast(unsigned, r));
  }
}

// C[b] = A[b]^T Bm[b] (m x m, fp64), reduced over the N rows in ascending order by the one workgroup that owns the
// 32 x 32 tile: no partial sums across workgroups, no atomics.
__global__ __launch_bounds__(256) void lb_gram_kernel(const float* A, const float* Bm, int N, int m, double* C) {
  __shared__ float As[32][33], Bs[32][33];
  const int b = blockIdx.y, tiles = (m + 31) / 32;
  const int ti = blockIdx.x / tiles, tj = blockIdx.x % tiles;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const float* Ab = A + (int64_t)b * N * m;
  const float* Bb = Bm + (int64_t)b * N * m;
  double acc[2][2] = {{0., 0.}, {0., 0.}};
  for (int n0 = 0; n0 < N; n0 += 32) {
    for (int e = threadIdx.x; e < 32 * 32; e += 256) {
      const int r = e >> 5, c = e & 31, n = n0 + r;
      const int ca = ti * 32 + c, cb = tj * 32 + c;
      As[r][c] = (n < N && ca < m) ? Ab[(int64_t)n * m + ca] : 0.f;
      Bs[r][c] = (n < N && cb < m) ? Bb[(int64_t)n * m + cb] : 0.f;
    }
    __syncthreads();
#pragma unroll 8
    for (int r = 0; r < 32; ++r) {
      const double a0 = As[r][ty], a1 = As[r][ty + 16], b0 = Bs[r][tx], b1 = Bs[r][tx + 16];
      acc[0][0] = fma(a0, b0, acc[0][0]);
      acc[0][1] = fma(a0, b1, acc[0][1]);
      acc[1][0] = fma(a1, b0, acc[1][0]);
      acc[1][1] = fma(a1, b1, acc[1][1]);
    }
    __syncthreads();
  }
  double* Cb = C + (int64_t)b * m * m;
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const int i = ti * 32 + ty + 16 * u, j = tj * 32 + tx + 16 * v;
      if (i < m && j < m) Cb[(int64_t)i * m + j] = acc[u][v];
    }
}

// out[b] = X[b] T[b]  ([N,m] x [m,m]); a workgroup takes 32 rows, a thread one column of 16 of them
__global__ __launch_bounds__(256) void lb_rotate_kernel(const float* X, const float* T, int N, int m, float* out) {
  __shared__ float Xs[32][129];
  const int b = blockIdx.y, n0 = blockIdx.x * 32;
  const float* Xb = X + (int64_t)b * N * m;
  const float* Tb = T + (int64_t)b * m * m;
  for (int e = threadIdx.x; e < 32 * m; e += 256) {
    const int r = e / m, c = e - r * m;
    Xs[r][c] = n0 + r < N ? Xb[(int64_t)(n0 + r) * m + c] : 0.f;
  }
  __syncthreads();
  const int j = threadIdx.x & 127, rg = (threadIdx.x >> 7) * 16;
  if (j >= m) return;
  float acc[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (int k = 0; k < m; ++k) {
    const float t = Tb[(int64_t)k * m + j];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = fmaf(Xs[rg + r][k], t, acc[r]);
  }
  float* ob = out + (int64_t)b * N * m;
#pragma unroll
  for (int r = 0; r < 16; ++r)
    if (n0 + rg + r < N) ob[(int64_t)(n0 + rg + r) * m + j] = acc[r];
}

// U[b,n,j] = X[b,n,j] for j < lp; theta likewise
__global__ __launch_bounds__(256) void lb_take_kernel(const float* X, const float* th, int N, int m, int lp, float* U, float* theta) {
  const int b = blockIdx.y;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < lp) theta[(int64_t)b * lp + e] = th[(int64_t)b * m + e];
  if (e >= N * lp) return;
  const int n = e / lp, j = e - n * lp;
  U[(int64_t)b * N * lp + e] = X[((int64_t)b * N + n) * m + j];
}

// ---------------------------------------------------------------------------------------------------------
// The m x m symmetric eigensolver: parallel cyclic Jacobi, one workgroup per cloud, the matrix and the accumulated
// rotations both in LDS (2 x m x (m | 1) floats: 129 KiB at m = 128, which is what bounds m). A round of the round-robin
// tournament rotates m / 2 disjoint pairs at once: angles (in fp64, rounded once), columns of A and V, rows of A, then the
// pairs' own three entries in closed form. Every update has the small-correction form x - s (y + tan(phi/2) x), whose
// rounding error follows the size of the change: a matrix that arrives nearly diagonal (every solve after the first outer
// iteration) leaves as accurate as it came. Rotations below the threshold are skipped, a round without any skips its
// three phases, and the sweeps end when one rotates nothing.
//   ORTH: in = G = Y^T Y. A = D^-1/2 G D^-1/2 (unit diagonal: the filtered columns differ by many orders of magnitude),
//         out T = D^-1/2 Q max(S, floor)^-1/2 Q^T — the symmetric (Loewdin) form, which leaves a nearly orthonormal block
//         where it is; info[b] counts the floored directions.
//   RR:   in = H = X^T L X and G = X^T X. With E = G - I (1e-6, the rounding of X's entries) the projected problem is
//         taken to first order in E: A = H - (E H + H E) / 2, out T = (I - E / 2) Q with the columns by ascending
//         eigenvalue, theta = those eigenvalues.
// ---------------------------------------------------------------------------------------------------------
struct JacArgs {
  const double* in;     // [B,m,m]
  const double* gram;   // [B,m,m] (RR)
  int m, max_sweeps;
  float rel, absf, floor;
  float* T;             // [B,m,m]
  float* theta;         // [B,m] (RR)
  int32_t* info;        // [B] (ORTH; may be null)
};

constexpr int kJacThreads = 1024;
constexpr int kJacMaxM = 128;

__device__ __forceinline__ void jac_pair(int mm, int r, int k, int& p, int& q) {
  const int a = k == 0 ? mm - 1 : (r + k) % (mm - 1);
  const int b = (r + mm - 1 - k) % (mm - 1);
  p = min(a, b), q = max(a, b);
}

template <bool RR>
__global__ __launch_bounds__(kJacThreads) void lb_jacobi_kernel(JacArgs a) {
  extern __shared__ __attribute__((aligned(16))) float jac_lds[];
  __shared__ double dinv[kJacMaxM];
  __shared__ float r_s[kJacMaxM / 2], r_h[kJacMaxM / 2], r_t[kJacMaxM / 2], r_pp[kJacMaxM / 2], r_qq[kJacMaxM / 2], w_s[kJacMaxM];
  __shared__ int r_p[kJacMaxM / 2], r_q[kJacMaxM / 2], rank_s[kJacMaxM];
  __shared__ unsigned scale_bits;
  __shared__ int round_act[2], sweep_act, lost_s;
  const int m = a.m, ld = m | 1, tid = threadIdx.x, b = blockIdx.x;
  float* A = jac_lds;
  float* V = jac_lds + m * ld;
  const double* in = a.in + (int64_t)b * m * m;
  const int mm = m + (m & 1), np = mm / 2;

  if (tid == 0) scale_bits = 0u, round_act[0] = round_act[1] = 0, sweep_act = 0, lost_s = 0;
  if (!RR) {
    if (tid < m) {
      const double g = in[(int64_t)tid * m + tid];
      dinv[tid] = g > 0. ? 1. / sqrt(g) : 0.;
    }
    __syncthreads();
    for (int e = tid; e < m * m; e += kJacThreads) {
      const int i = e / m, j = e - i * m;
      A[i * ld + j] = i == j ? (dinv[i] > 0. ? 1.f : 0.f)
                             : (float)(0.5 * (in[(int64_t)i * m + j] + in[(int64_t)j * m + i]) * dinv[i] * dinv[j]);
      V[i * ld + j] = i == j ? 1.f : 0.f;
    }
  } else {
    // A <- H (fp32), V <- E = G - I, then A <- H - (E H + H E) / 2 from those two, V <- I
    const double* gr = a.gram + (int64_t)b * m * m;
    for (int e = tid; e < m * m; e += kJacThreads) {
      const int i = e / m, j = e - i * m;
      A[i * ld + j] = (float)(0.5 * (in[(int64_t)i * m + j] + in[(int64_t)j * m + i]));
      V[i * ld + j] = (float)(0.5 * (gr[(int64_t)i * m + j] + gr[(int64_t)j * m + i]) - (i == j ? 1. : 0.));
    }
    __syncthreads();
    float corr[(kJacMaxM * kJacMaxM) / kJacThreads];
    int u = 0;
    for (int e = tid; e < m * m; e += kJacThreads, ++u) {
      const int i = e / m, j = e - i * m;
      float s = 0.f;
      for (int k = 0; k < m; ++k) s = fmaf(V[i * ld + k], A[k * ld + j], fmaf(A[i * ld + k], V[k * ld + j], s));
      corr[u] = s;
    }
    __syncthreads();
    u = 0;
    for (int e = tid; e < m * m; e += kJacThreads, ++u) {
      const int i = e / m, j = e - i * m;
      // both (i,j) and (j,i) get the mean of the two corrections below; here the entry's own
      A[i * ld + j] = (float)(0.5 * (in[(int64_t)i * m + j] + in[(int64_t)j * m + i]) - 0.5 * (double)corr[u]);
      V[i * ld + j] = i == j ? 1.f : 0.f;
    }
    __syncthreads();
    // exact symmetry (the correction's two sums round differently): the upper triangle rules
    for (int e = tid; e < m * m; e += kJacThreads) {
      const int i = e / m, j = e - i * m;
      if (i > j) A[i * ld + j] = A[j * ld + i];
    }
  }
  __syncthreads();
  if (tid < m) atomicMax(&scale_bits, __builtin_bit_cast(unsigned, fabsf(A[tid * ld + tid])));
  __syncthreads();
  const float absf = a.absf * __builtin_bit_cast(float, scale_bits);

  int rc = 0;      // rounds so far: the round's flag alternates between two words, the idle one is cleared a round ahead
  for (int sweep = 0; sweep < a.max_sweeps; ++sweep) {
    for (int r = 0; r < mm - 1; ++r, ++rc) {
      // ---- the round's angles
      if (tid == 0) round_act[(rc + 1) & 1] = 0;
      if (tid < np) {
        int p, q;
        jac_pair(mm, r, tid, p, q);
        float s = 0.f, h = 0.f, t = 0.f, app = 0.f, aqq = 0.f;
        if (q < m) {
          app = A[p * ld + p], aqq = A[q * ld + q];
          const float apq = A[p * ld + q];
          if (fabsf(apq) > a.rel * sqrtf(fabsf(app * aqq)) + absf) {
            const double tau = ((double)aqq - (double)app) / (2. * (double)apq);
            const double td = copysign(1., tau) / (fabs(tau) + sqrt(1. + tau * tau));
            const double c = 1. / sqrt(1. + td * td), sd = td * c;
            s = (float)sd, h = (float)(sd / (1. + c)), t = (float)td;
            if (s != 0.f) {
              app = app - t * apq, aqq = aqq + t * apq;
              round_act[rc & 1] = 1, sweep_act = 1;
            }
          }
        }
        r_p[tid] = p, r_q[tid] = q, r_s[tid] = s, r_h[tid] = h, r_t[tid] = t, r_pp[tid] = app, r_qq[tid] = aqq;
      }
      __syncthreads();
      if (!round_act[rc & 1]) continue;      // (the same value in every thread: written before the barrier)
      // ---- columns of A and V
      for (int e = tid; e < np * m; e += kJacThreads) {
        const int k = e / m, row = e - k * m;
        const float s = r_s[k];
        if (s == 0.f) continue;
        const float h = r_h[k];
        const int p = r_p[k], q = r_q[k];
        float x = A[row * ld + p], y = A[row * ld + q];
        A[row * ld + p] = x - s * (y + h * x);
        A[row * ld + q] = y + s * (x - h * y);
        x = V[row * ld + p], y = V[row * ld + q];
        V[row * ld + p] = x - s * (y + h * x);
        V[row * ld + q] = y + s * (x - h * y);
      }
      __syncthreads();
      // ---- rows of A
      for (int e = tid; e < np * m; e += kJacThreads) {
        const int k = e / m, cidx = e - k * m;
        const float s = r_s[k];
        if (s == 0.f) continue;
        const float h = r_h[k];
        const int p = r_p[k], q = r_q[k];
        const float x = A[p * ld + cidx], y = A[q * ld + cidx];
        A[p * ld + cidx] = x - s * (y + h * x);
        A[q * ld + cidx] = y + s * (x - h * y);
      }
      __syncthreads();
      // ---- the pairs' own entries in closed form
      if (tid < np && r_s[tid] != 0.f) {
        const int p = r_p[tid], q = r_q[tid];
        A[p * ld + p] = r_pp[tid], A[q * ld + q] = r_qq[tid];
        A[p * ld + q] = 0.f, A[q * ld + p] = 0.f;
      }
      __syncthreads();
    }
    const int again = sweep_act;
    __syncthreads();
    if (tid == 0) sweep_act = 0;
    __syncthreads();
    if (!again) break;
  }
  __syncthreads();

  // ---- eigenvalues, their ascending order (ties by index)
  if (tid < m) w_s[tid] = A[tid * ld + tid];
  __syncthreads();
  if (tid < m) {
    const float w = w_s[tid];
    int rk = 0;
    for (int i = 0; i < m; ++i) rk += (w_s[i] < w || (w_s[i] == w && i < tid)) ? 1 : 0;
    rank_s[tid] = rk;
  }
  __syncthreads();
  float* T = a.T + (int64_t)b * m * m;
  if (RR) {
    if (tid < m) a.theta[(int64_t)b * m + rank_s[tid]] = w_s[tid];
    // A <- E again (the matrix is spent), T = Q - E Q / 2 with the columns in order
    const double* gr = a.gram + (int64_t)b * m * m;
    for (int e = tid; e < m * m; e += kJacThreads) {
      const int i = e / m, j = e - i * m;
      A[i * ld + j] = (float)(0.5 * (gr[(int64_t)i * m + j] + gr[(int64_t)j * m + i]) - (i == j ? 1. : 0.));
    }
    __syncthreads();
    for (int e = tid; e < m * m; e += kJacThreads) {
      const int i = e / m, j = e - i * m;
      float s = 0.f;
      for (int k = 0; k < m; ++k) s = fmaf(A[i * ld + k], V[k * ld + j], s);
      T[(int64_t)i * m + rank_s[j]] = V[i * ld + j] - 0.5f * s;
    }
  } else {
    if (tid < m) {
      const float w = w_s[tid];
      if (!(w >= a.floor)) atomicAdd(&lost_s, 1);
      w_s[tid] = 1.f / sqrtf(fmaxf(w, a.floor));
    }
    __syncthreads();
    for (int e = tid; e < m * m; e += kJacThreads) {
      const int i = e / m, j = e - i * m;
      double s = 0.;
      for (int k = 0; k < m; ++k) s = fma((double)(V[i * ld + k] * w_s[k]), (double)V[j * ld + k], s);
      T[(int64_t)i * m + j] = (float)(s * dinv[i]);
    }
    if (tid == 0 && a.info) a.info[b] += lost_s;
  }
}

static size_t jac_lds_bytes(int m) { return (size_t)2 * m * (m | 1) * sizeof(float); }

// ---------------------------------------------------------------------------------------------------------
// Band re-projection: coeff = adv U ([B,3,lp]), lfc = coeff U^T, hfc = adv - lfc (U orthonormal), sum = lfc + hfc.
// Launch 1 reduces coeff over runs of 64 rows (one workgroup each; a thread owns a column and adds its rows in order),
// launch 2 adds the runs' partial sums in order, meets each row of U with coeff on one wave and reduces over the lanes
// by a fixed tree. U is read twice per call, [B,N,lp] each time, instead of V and V^T [B,N,N].
// ---------------------------------------------------------------------------------------------------------
constexpr int kBrRows = 64;

struct BandArgs {
  const float* adv;   // [B,3,N]
  const float* U;     // [B,N,lp]
  int N, lp, S;
  float* part;        // [B,S,3,lp]
  float* coeff;       // [B,3,lp] or null
  float* lfc;
  float* hfc;
  float* sum;         // may be null
};

__global__ __launch_bounds__(256) void band_coeff_kernel(BandArgs a) {
  __shared__ float adv_s[3][kBrRows];
  __shared__ float half_s[3][128];
  const int b = blockIdx.y, s = blockIdx.x, n0 = s * kBrRows;
  const int rows = min(kBrRows, a.N - n0);
  for (int e = threadIdx.x; e < 3 * kBrRows; e += 256) {
    const int c = e / kBrRows, r = e - c * kBrRows;
    adv_s[c][r] = r < rows ? a.adv[((int64_t)b * 3 + c) * a.N + n0 + r] : 0.f;
  }
  __syncthreads();
  const int jl = threadIdx.x & 127, rg = threadIdx.x >> 7;      // two halves of the run, 32 rows each
  const float* Ub = a.U + ((int64_t)b * a.N + n0) * a.lp;
  for (int j0 = 0; j0 < a.lp; j0 += 128) {
    const int j = j0 + jl;
    float acc[3] = {0.f, 0.f, 0.f};
    if (j < a.lp)
      for (int r = rg * 32; r < min(rows, rg * 32 + 32); ++r) {
        const float u = Ub[(int64_t)r * a.lp + j];
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] = fmaf(adv_s[c][r], u, acc[c]);
      }
    if (rg == 1)
#pragma unroll
      for (int c = 0; c < 3; ++c) half_s[c][jl] = acc[c];
    __syncthreads();
    if (rg == 0 && j < a.lp)
#pragma unroll
      for (int c = 0; c < 3; ++c) a.part[(((int64_t)b * a.S + s) * 3 + c) * a.lp + j] = acc[c] + half_s[c][jl];
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void band_apply_kernel(BandArgs a) {
  extern __shared__ float co_s[];      // [3][lp]
  const int b = blockIdx.y, n0 = blockIdx.x * kBrRows;
  for (int e = threadIdx.x; e < 3 * a.lp; e += 256) {
    float s = 0.f;
    for (int q = 0; q < a.S; ++q) s += a.part[((int64_t)b * a.S + q) * 3 * a.lp + e];
    co_s[e] = s;
    if (blockIdx.x == 0 && a.coeff) a.coeff[(int64_t)b * 3 * a.lp + e] = s;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int r = wave; r < kBrRows; r += 4) {
    const int n = n0 + r;
    if (n >= a.N) break;
    const float* u = a.U + ((int64_t)b * a.N + n) * a.lp;
    float acc[3] = {0.f, 0.f, 0.f};
    for (int j = lane; j < a.lp; j += 64) {
      const float x = u[j];
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[c] = fmaf(co_s[c * a.lp + j], x, acc[c]);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] = wave_sum(acc[c]);
    if (lane < 3) {
      const float l = lane == 0 ? acc[0] : lane == 1 ? acc[1] : acc[2];
      const int64_t o = ((int64_t)b * 3 + lane) * a.N + n;
      const float h = a.adv[o] - l;
      a.lfc[o] = l;
      a.hfc[o] = h;
      if (a.sum) a.sum[o] = l + h;
    }
  }
}

}  // namespace pc3d

using namespace pc3d;

extern "C" int pc3d_graph_laplacian_csr_f32(const float* xyz, int64_t x_bs, int64_t x_ps, int64_t x_cs, const int32_t* idx, int B,
                                            int N, int K, int cap, int32_t* rowptr, int32_t* col, float* val, float* deg,
                                            void* stream) {
  const char* nm = "pc3d_graph_laplacian_csr_f32";
  PC3D_REQUIRE(B >= 0 && N >= 1 && K >= 1 && cap >= 0, "%s: bad sizes B=%d N=%d K=%d cap=%d", nm, B, N, K, cap);
  PC3D_REQUIRE(B <= 65535, "%s: B=%d exceeds grid.y limit", nm, B);
  PC3D_REQUIRE((int64_t)N * K <= (int64_t)1 << 30, "%s: N * K = %lld exceeds the 32-bit row starts", nm, (long long)N * K);
  if (B == 0) return PC3D_OK;
  PC3D_REQUIRE(xyz && idx && rowptr && deg && (cap == 0 || (col && val)), "%s: null pointer", nm);
  hipStream_t st = as_stream(stream);
  CsrArgs a{{xyz, x_bs, x_ps, x_cs}, idx, N, K, cap, rowptr, col, val, deg};
  hipLaunchKernelGGL(csr_count_kernel, dim3(cdiv(N, 4), B), dim3(256), 0, st, a);
  PC3D_LAUNCH_CHECK("pc3d_graph_laplacian_csr_f32/count");
  hipLaunchKernelGGL(csr_scan_kernel, dim3(B), dim3(1024), 0, st, rowptr, N);
  PC3D_LAUNCH_CHECK("pc3d_graph_laplacian_csr_f32/scan");
  hipLaunchKernelGGL(csr_fill_kernel, dim3(cdiv(N, 4), B), dim3(256), 0, st, a);
  PC3D_LAUNCH_CHECK("pc3d_graph_laplacian_csr_f32/fill");
  return PC3D_OK;
}

namespace {
struct LbWs {
  float *x0, *x1, *x2, *T, *theta, *ub, *coef;
  double *G, *H;
  int32_t* info;
  size_t bytes;
};
LbWs lb_carve(void* ws, int B, int N, int m, int degree) {
  LbWs w{};
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = ws ? static_cast<char*>(ws) + off : nullptr;
    off += (bytes + 255) & ~(size_t)255;
    return p;
  };
  const size_t blk = (size_t)B * N * m * sizeof(float), mat = (size_t)B * m * m;
  w.G = reinterpret_cast<double*>(take(mat * sizeof(double)));
  w.H = reinterpret_cast<double*>(take(mat * sizeof(double)));
  w.x0 = reinterpret_cast<float*>(take(blk));
  w.x1 = reinterpret_cast<float*>(take(blk));
  w.x2 = reinterpret_cast<float*>(take(blk));
  w.T = reinterpret_cast<float*>(take(mat * sizeof(float)));
  w.theta = reinterpret_cast<float*>(take((size_t)B * m * sizeof(float)));
  w.ub = reinterpret_cast<float*>(take((size_t)B * sizeof(float)));
  w.coef = reinterpret_cast<float*>(take((size_t)B * (degree > 0 ? degree : 1) * 4 * sizeof(float)));
  w.info = reinterpret_cast<int32_t*>(take((size_t)B * sizeof(int32_t)));
  w.bytes = off;
  return w;
}
}  // namespace

extern "C" int pc3d_lowband_block(int N, int lp, int guard_min, int guard_div) {
  if (N < 1 || lp < 0 || guard_min < 0 || guard_div < 1) return -1;
  const int guard = guard_min > (lp + guard_div - 1) / guard_div ? guard_min : (lp + guard_div - 1) / guard_div;
  return N < lp + guard ? N : lp + guard;
}

extern "C" int64_t pc3d_lowband_ws_bytes(int B, int N, int m, int degree) {
  if (B < 0 || N < 1 || m < 1 || degree < 0) return -1;
  return (int64_t)lb_carve(nullptr, B, N, m, degree).bytes;
}

extern "C" int pc3d_lowband_basis_f32(const int32_t* rowptr, const int32_t* col, const float* val, const float* deg, int B, int N,
                                      int cap, int lp, int m, int degree, int iters, float range_first, float range_growth,
                                      float range_max, float cut_min, float gram_floor, float jacobi_rel, float jacobi_abs,
                                      int jacobi_sweeps, float* U, float* theta, float* resid, int32_t* lost, void* ws,
                                      int64_t ws_bytes, void* stream) {
  const char* nm = "pc3d_lowband_basis_f32";
  PC3D_REQUIRE(B >= 0 && N >= 1 && cap >= 0 && lp >= 0 && lp <= m && m >= 1 && m <= N,
               "%s: bad sizes B=%d N=%d cap=%d lp=%d m=%d", nm, B, N, cap, lp, m);
  PC3D_REQUIRE(m <= kJacMaxM, "%s: block of %d columns exceeds %d (the eigensolver's matrix and rotations live in one "
               "workgroup's LDS); use the full basis", nm, m, kJacMaxM);
  PC3D_REQUIRE(B <= 65535, "%s: B=%d exceeds grid.y limit", nm, B);
  PC3D_REQUIRE(degree >= 1 && iters >= 0 && jacobi_sweeps >= 1 && range_first > 1.f && range_growth >= 1.f && range_max > 1.f
               && cut_min > 0.f && cut_min < 0.25f && gram_floor > 0.f,
               "%s: bad schedule degree=%d iters=%d sweeps=%d", nm, degree, iters, jacobi_sweeps);
  PC3D_REQUIRE((int64_t)N * m <= (int64_t)1 << 30, "%s: N * m too large", nm);
  if (B == 0) return PC3D_OK;
  PC3D_REQUIRE(rowptr && deg && (cap == 0 || (col && val)) && (lp == 0 || (U && theta)) && resid && ws, "%s: null pointer", nm);
  LbWs w = lb_carve(ws, B, N, m, degree);
  PC3D_REQUIRE(ws_bytes >= (int64_t)w.bytes, "%s: workspace of %lld bytes, %lld needed", nm, (long long)ws_bytes, (long long)w.bytes);
  PC3D_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "%s: workspace must be 8-byte aligned", nm);
  hipStream_t st = as_stream(stream);
  const size_t lds = jac_lds_bytes(m);
  {
    hipError_t e1 = hipFuncSetAttribute(reinterpret_cast<const void*>(&lb_jacobi_kernel<true>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)jac_lds_bytes(kJacMaxM));
    hipError_t e2 = hipFuncSetAttribute(reinterpret_cast<const void*>(&lb_jacobi_kernel<false>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)jac_lds_bytes(kJacMaxM));
    if (e1 != hipSuccess || e2 != hipSuccess) {
      set_error("%s: the eigensolver's LDS size was refused: %s", nm, hipGetErrorString(e1 != hipSuccess ? e1 : e2));
      return (int)(e1 != hipSuccess ? e1 : e2);
    }
  }
  const dim3 rows4(cdiv(N, 4), B), blk256(256), gram_grid(cdiv(m, 32) * cdiv(m, 32), B), rot_grid(cdiv(N, 32), B);
  SpmmArgs sp{rowptr, col, val, deg, N, cap, m, nullptr, nullptr, nullptr, nullptr, degree * 4, w.theta, lp, resid};

  hipLaunchKernelGGL(lb_init_kernel, dim3(cdiv(N * m, 256), B), blk256, 0, st, w.x0, N, m, resid);
  PC3D_LAUNCH_CHECK("pc3d_lowband_basis_f32/init");
  hipLaunchKernelGGL(lb_maxdeg_kernel, dim3(B), blk256, 0, st, deg, N, w.ub);
  PC3D_LAUNCH_CHECK("pc3d_lowband_basis_f32/maxdeg");
  if (lost) {
    hipError_t e = zero_async(reinterpret_cast<float*>(lost), (size_t)B, st);     // (an int32 zero is a float zero)
    if (e != hipSuccess) {
      set_error("%s: zero fill failed: %s", nm, hipGetErrorString(e));
      return (int)e;
    }
  }
  float *cur = w.x0, *f1 = w.x1, *f2 = w.x2;
  auto swap = [](float*& p, float*& q) { float* t = p; p = q; q = t; };
  // cur <- cur G^-1/2, twice
  auto orth2 = [&]() -> int {
    for (int pass = 0; pass < 2; ++pass) {
      hipLaunchKernelGGL(lb_gram_kernel, gram_grid, blk256, 0, st, (const float*)cur, (const float*)cur, N, m, w.G);
      PC3D_LAUNCH_CHECK("pc3d_lowband_basis_f32/gram");
      JacArgs j{w.G, nullptr, m, jacobi_sweeps, jacobi_rel, jacobi_abs, gram_floor, w.T, nullptr, lost};
      hipLaunchKernelGGL(lb_jacobi_kernel<false>, dim3(B), dim3(kJacThreads), lds, st, j);
      PC3D_LAUNCH_CHECK("pc3d_lowband_basis_f32/jacobi");
      hipLaunchKernelGGL(lb_rotate_kernel, rot_grid, blk256, 0, st, (const float*)cur, (const float*)w.T, N, m, f1);
      PC3D_LAUNCH_CHECK("pc3d_lowband_basis_f32/rotate");
      swap(cur, f1);
    }
    return PC3D_OK;
  };
  // cur <- the Ritz vectors of cur's span, theta ascending
  auto ritz = [&]() -> int {
    SpmmArgs s0 = sp;
    s0.Y = cur, s0.out = f1;
    hipLaunchKernelGGL(lb_spmm_kernel<0>, rows4, blk256, 0, st, s0);
    PC3D_LAUNCH_CHECK("pc3d_lowband_basis_f32/product");
    hipLaunchKernelGGL(lb_gram_kernel, gram_grid, blk256, 0, st, (const float*)cur, (const float*)f1, N, m, w.H);
    PC3D_LAUNCH_CHECK("pc3d_lowband_basis_f32/gram");
    hipLaunchKernelGGL(lb_gram_kernel, gram_grid, blk256, 0, st, (const float*)cur, (const float*)cur, N, m, w.G);
    PC3D_LAUNCH_CHECK("pc3d_lowband_basis_f32/gram");
    JacArgs j{w.H, w.G, m, jacobi_sweeps, jacobi_rel, jacobi_abs, gram_floor, w.T, w.theta, nullptr};
    hipLaunchKernelGGL(lb_jacobi_kernel<true>, dim3(B), dim3(kJacThreads), lds, st, j);
    PC3D_LAUNCH_CHECK("pc3d_lowband_basis_f32/jacobi");
    hipLaunchKernelGGL(lb_rotate_kernel, rot_grid, blk256, 0, st, (const float*)cur, (const float*)w.T, N, m, f1);
    PC3D_LAUNCH_CHECK("pc3d_lowband_basis_f32/rotate");
    swap(cur, f1);
    return PC3D_OK;
  };
  int rc = orth2();
  if (rc != PC3D_OK) return rc;
  rc = ritz();
  if (rc != PC3D_OK) return rc;
  float range = range_first;
  for (int it = 0; it < iters; ++it) {
    hipLaunchKernelGGL(lb_coef_kernel, dim3(cdiv(B, 64)), dim3(64), 0, st, (const float*)w.theta, (const float*)w.ub, m, degree,
                       range < range_max ? range : range_max, cut_min, w.coef, B);
    PC3D_LAUNCH_CHECK("pc3d_lowband_basis_f32/coef");
    range = range < range_max ? range * range_growth : range_max;
    // (prev, cur) -> next, then the three rotate; step 1 has gamma = 0 and reads no prev
    float *prev = f1, *y = cur, *next = f2;
    for (int k = 1; k <= degree; ++k) {
      SpmmArgs s1 = sp;
      s1.Y = y, s1.P = prev, s1.out = next, s1.coef = w.coef + 4 * (k - 1);
      hipLaunchKernelGGL(lb_spmm_kernel<1>, rows4, blk256, 0, st, s1);
      PC3D_LAUNCH_CHECK("pc3d_lowband_basis_f32/filter");
      float* t = prev;
      prev = y, y = next, next = t;
    }
    cur = y, f1 = prev, f2 = next;
    rc = orth2();
    if (rc != PC3D_OK) return rc;
    rc = ritz();
    if (rc != PC3D_OK) return rc;
  }
  if (lp > 0) {
    hipLaunchKernelGGL(lb_take_kernel, dim3(cdiv(N * lp, 256), B), blk256, 0, st, (const float*)cur, (const float*)w.theta, N, m, lp,
                       U, theta);
    PC3D_LAUNCH_CHECK("pc3d_lowband_basis_f32/take");
    SpmmArgs s2 = sp;
    s2.Y = cur;
    hipLaunchKernelGGL(lb_spmm_kernel<2>, rows4, blk256, 0, st, s2);
    PC3D_LAUNCH_CHECK("pc3d_lowband_basis_f32/resid");
  }
  return PC3D_OK;
}

extern "C" int64_t pc3d_band_reproject_ws_floats(int B, int N, int lp) {
  if (B < 0 || N < 1 || lp < 0) return -1;
  return (int64_t)B * cdiv(N, kBrRows) * 3 * (lp > 0 ? lp : 1);
}

extern "C" int pc3d_band_reproject_f32(const float* adv, const float* U, int B, int N, int lp, float* coeff, float* lfc, float* hfc,
                                       float* sum, float* ws, void* stream) {
  const char* nm = "pc3d_band_reproject_f32";
  PC3D_REQUIRE(B >= 0 && N >= 1 && lp >= 0 && lp <= N, "%s: bad sizes B=%d N=%d low_pass=%d", nm, B, N, lp);
  PC3D_REQUIRE(B <= 65535, "%s: B=%d exceeds grid.y limit", nm, B);
  PC3D_REQUIRE((size_t)3 * lp * sizeof(float) <= 48 * 1024, "%s: low_pass=%d exceeds the coefficient tile", nm, lp);
  if (B == 0) return PC3D_OK;
  PC3D_REQUIRE(adv && lfc && hfc && ws && (lp == 0 || U), "%s: null pointer", nm);
  hipStream_t st = as_stream(stream);
  const int S = cdiv(N, kBrRows);
  BandArgs a{adv, U, N, lp, S, ws, coeff, lfc, hfc, sum};
  if (lp > 0) {
    hipLaunchKernelGGL(band_coeff_kernel, dim3(S, B), dim3(256), 0, st, a);
    PC3D_LAUNCH_CHECK("pc3d_band_reproject_f32/coeff");
  }
  hipLaunchKernelGGL(band_apply_kernel, dim3(S, B), dim3(256), (size_t)3 * lp * sizeof(float), st, a);
  PC3D_LAUNCH_CHECK("pc3d_band_reproject_f32/bands");
  return PC3D_OK;
}
