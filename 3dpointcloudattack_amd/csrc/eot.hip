// The additional-experiments CW (attack/additional_exp/CW_attack.py) as a device-side loop: the two launches around the
// stacked victim pass of one iteration.
//
//   pc3d_eot_prepare_f32  the stacked victim input X [(1+E) B, 3, K], slot-major (row s B + b): slot 0 is the iterate, slot
//                         e >= 1 is R_e ori + (adv - ori) for the e-th small rotation of that iteration (:195-221), each
//                         optionally centred and scaled to the unit sphere (:107-115 / :224-230) and, for e >= 1, resampled
//                         (:236-239: K of the 2K columns of cat((x, x), 2)). One workgroup per (slot, cloud); the cloud is
//                         walked from global memory three times (centroid, largest norm, output), never copied to LDS.
//   pc3d_eot_update_f32   everything after the victim's backward, one workgroup per cloud: the record block (:151-182), the
//                         gradient of the adversarial term through resampling and renormalisation summed over the views in
//                         ascending order, the gradient of the distance term, Adam and the z-only box (:266-275).
//   pc3d_eot_draw_f32     (opt-in) rows of the tables the two read — rotations, resampling indices and their inverse —
//                         drawn on the device from counter-based hash keys, one workgroup per (row, view).
//
// d x_e / d adv = I, so a view's gradient reaches the iterate through the renormalisation alone:
//   y = q / s, q = p - mean p, s = |q_a| (a = arg-max of the norms, LOWEST index on a tie: torch's max(dim) on the CPU):
//   g_q = g_y / s;  g_q[a] += ds q_a / |q_a| with ds = -sum(g_y . q) / s^2;  g_p = g_q - mean g_q.
// The resampling's backward is a gather through the inverse table (at most two columns draw a point: i and i + K), so no
// atomics; two fp32 terms commute. Every sum over the cloud is a per-thread sum over its strided points in ascending
// order, the wave butterfly, then the waves in ascending order (block_sum_ordered): the bits of a cloud depend on neither
// the batch nor the launch.
#include "update_body.h"

namespace pc3d {

constexpr int kEotMaxPoints = PC3D_EOT_MAX_POINTS;
constexpr int kEotMaxViews = PC3D_EOT_MAX_VIEWS;
constexpr int kEpThreads = 256;
constexpr int kEuThreads = 1024;
static_assert((size_t)kEotMaxPoints * 12 + 1024 <= 160 * 1024, "the update's gradient accumulators (12 B a point) fit the CU's LDS");

// row of the per-iteration tables: (step - back) mod T, never negative
__device__ __forceinline__ int eot_table_row(const int* step_dev, int step_host, int back, int T) {
  const int r = ((step_dev ? step_dev[0] : step_host) - back) % T;
  return r < 0 ? r + T : r;
}
__device__ __forceinline__ int eot_wrap(int j, int K) {
  const int r = j % K;
  return r < 0 ? r + K : r;
}

// point i of a slot before the renormalisation: the iterate itself, or R ori_i + (adv_i - ori_i) (bmm's row times column,
// summed left to right)
__device__ __forceinline__ void eot_point(const float* adv, const float* ori, int K, int i, bool view, const float* R, float* p) {
  const float a[3] = {adv[i], adv[K + i], adv[2 * K + i]};
  if (!view) {
    p[0] = a[0], p[1] = a[1], p[2] = a[2];
    return;
  }
  const float o[3] = {ori[i], ori[K + i], ori[2 * K + i]};
#pragma unroll
  for (int c = 0; c < 3; ++c) p[c] = ((R[3 * c] * o[0] + R[3 * c + 1] * o[1]) + R[3 * c + 2] * o[2]) + (a[c] - o[c]);
}

// q = p - c of the same point in double, from the fp32 inputs (the products and sums are exact to double rounding)
__device__ __forceinline__ void eot_q64(const float* adv, const float* ori, int K, int i, bool view, const float* R, const float* c,
                                        double* q) {
  const double a[3] = {adv[i], adv[K + i], adv[2 * K + i]};
  if (!view) {
    q[0] = a[0] - c[0], q[1] = a[1] - c[1], q[2] = a[2] - c[2];
    return;
  }
  const double o[3] = {ori[i], ori[K + i], ori[2 * K + i]};
#pragma unroll
  for (int k = 0; k < 3; ++k)
    q[k] = (((double)R[3 * k] * o[0] + (double)R[3 * k + 1] * o[1]) + (double)R[3 * k + 2] * o[2]) + (a[k] - o[k]) - (double)c[k];
}

struct EotPrepArgs {
  const float *adv, *ori, *rot;      // adv / ori [B,3,K]; rot [T,E,3,3]
  const int32_t* idx;                // [T,E,K] or null: no resampling
  int B, K, E, T, renorm;
  const int* step_dev;
  int step_host;
  float* X;                          // [(1+E) B,3,K]
  float* stats;                      // [(1+E) B,4]: centroid, scale
  int32_t* arg;                      // [(1+E) B]
};
struct EotPrepRaggedArgs : EotPrepArgs {
  const int32_t* lengths;            // [B] points that count per cloud; idx is then [T,E,B,K], a table per cloud
};
template <bool RAGGED> struct EotPrepArgsOf { using type = EotPrepArgs; };
template <> struct EotPrepArgsOf<true> { using type = EotPrepRaggedArgs; };

// LDS of the ragged instantiations alone: a slot's output column 0 (prepare), the iterate's point 0 before [0..2] and after
// [3..5] the update
__device__ __forceinline__ float* eot_pad_slot() {
  __shared__ float s_pad[6];
  return s_pad;
}

// RAGGED: cloud b counts L = lengths[b] points (clamped to [1, K]; K is the capacity and the row stride). Every walk over the
// cloud stops at L with the dense thread-to-point mapping, so the sums, the arg-max and with them every bit of the rows < L
// are those of the dense launch on that cloud alone at K = L; the rows >= L of adv and ori are never read. The output
// columns >= L of every slot are copies of that slot's output column 0. The dense instantiation compiles to the kernel it was
// before RAGGED existed (the parameter is a type of its own, L is K).
template <bool RAGGED>
__global__ __launch_bounds__(kEpThreads) void eot_prepare_kernel(typename EotPrepArgsOf<RAGGED>::type a) {
  __shared__ float red[kEpThreads / 64];
  __shared__ float s_v[kEpThreads / 64];
  __shared__ int s_i[kEpThreads / 64];
  const int row = blockIdx.x, s = row / a.B, b = row - s * a.B, tid = threadIdx.x, K = a.K;
  int L = K;
  if constexpr (RAGGED) L = min(max(a.lengths[b], 1), K);
  const float* adv = a.adv + (int64_t)b * 3 * K;
  const float* ori = a.ori + (int64_t)b * 3 * K;
  const bool view = s >= 1;
  float R[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
  int t = 0;
  if (view) {
    t = eot_table_row(a.step_dev, a.step_host, 0, a.T);
    const float* rp = a.rot + ((int64_t)t * a.E + (s - 1)) * 9;
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = rp[k];
  }
  float c[3] = {0.f, 0.f, 0.f}, scale = 1.f;
  int am = 0;
  if (a.renorm) {
    float sum[3] = {0.f, 0.f, 0.f};
    for (int i = tid; i < L; i += kEpThreads) {
      float p[3];
      eot_point(adv, ori, K, i, view, R, p);
      sum[0] += p[0], sum[1] += p[1], sum[2] += p[2];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = block_sum_ordered<kEpThreads / 64>(sum[k], red) / (float)L;
    float bv = -1.f;
    int bi = 0x7fffffff;
    for (int i = tid; i < L; i += kEpThreads) {      // ascending: the first of equal norms stays
      float p[3];
      eot_point(adv, ori, K, i, view, R, p);
      const float q0 = p[0] - c[0], q1 = p[1] - c[1], q2 = p[2] - c[2];
      const float n = __builtin_sqrtf(q0 * q0 + q1 * q1 + q2 * q2);
      if (n > bv) bv = n, bi = i;
    }
    int wi = bi;
    const float wv = wave_max_lowest_index(bv, wi);
    __syncthreads();
    if ((tid & 63) == 0) s_v[tid >> 6] = wv, s_i[tid >> 6] = wi;
    __syncthreads();
    bv = s_v[0], bi = s_i[0];
#pragma unroll
    for (int w = 1; w < kEpThreads / 64; ++w)
      if (s_v[w] > bv || (s_v[w] == bv && s_i[w] < bi)) bv = s_v[w], bi = s_i[w];
    scale = bv;
    am = (bi >= 0 && bi < L) ? bi : 0;      // (a cloud of NaN has no arg-max)
  }
  if (tid == 0) {
    a.stats[(int64_t)row * 4 + 0] = c[0];
    a.stats[(int64_t)row * 4 + 1] = c[1];
    a.stats[(int64_t)row * 4 + 2] = c[2];
    a.stats[(int64_t)row * 4 + 3] = scale;
    a.arg[row] = am;
  }
  const int32_t* ix = nullptr;
  if (view && a.idx) {
    if constexpr (RAGGED) ix = a.idx + (((int64_t)t * a.E + (s - 1)) * a.B + b) * K;
    else ix = a.idx + ((int64_t)t * a.E + (s - 1)) * K;
  }
  float* X = a.X + (int64_t)row * 3 * K;
  for (int j = tid; j < L; j += kEpThreads) {
    const int i = ix ? eot_wrap(ix[j], L) : j;
    float p[3];
    eot_point(adv, ori, K, i, view, R, p);
    if (a.renorm) {
#pragma unroll
      for (int k = 0; k < 3; ++k) p[k] = (p[k] - c[k]) / scale;
    }
    X[j] = p[0], X[K + j] = p[1], X[2 * K + j] = p[2];
    if constexpr (RAGGED) {
      if (j == 0) {      // thread 0: the slot's output column 0, for the padding columns
        float* s_pad = eot_pad_slot();
        s_pad[0] = p[0], s_pad[1] = p[1], s_pad[2] = p[2];
      }
    }
  }
  if constexpr (RAGGED) {
    __syncthreads();
    const float* s_pad = eot_pad_slot();
    const float p0 = s_pad[0], p1 = s_pad[1], p2 = s_pad[2];
    for (int j = L + tid; j < K; j += kEpThreads) X[j] = p0, X[K + j] = p1, X[2 * K + j] = p2;
  }
}

struct EotUpdArgs {
  float* adv;                        // [B,3,K], updated in place
  const float *ori, *gx;             // gx [(1+E) B,3,K] (E == 0: [B,3,K])
  float *m, *v;
  int B, K, E, T, renorm;
  const float* rot;                  // [T,E,3,3]
  const int32_t* inv;                // [T,E,K,2] or null
  const float* stats;
  const int32_t* arg;
  const int64_t *pred, *goal;
  int untarget;
  float* bestdist;
  int64_t* bestscore;
  float* o_bestdist;
  int64_t* o_bestscore;
  float *o_bestattack, *input_val, *dist_val, *g_out;
  int dist_kind;                     // 1: L2, 2: Chamfer adv -> ori
  const float* w;
  const int32_t* nn_idx;
  int batch_mean;
  double lr, b1, b2;
  float eps;
  int one_d;
  float box;
  const int* step_dev;
  int step_host;
};
struct EotUpdRaggedArgs : EotUpdArgs {
  const int32_t* lengths;            // [B]; inv is then [T,E,B,K,2]
};
template <bool RAGGED> struct EotUpdArgsOf { using type = EotUpdArgs; };
template <> struct EotUpdArgsOf<true> { using type = EotUpdRaggedArgs; };

// upstream gradient of point i of a view before the resampling: the column itself, or the columns that drew it (K: the row
// stride, L <= K: the columns that exist)
__device__ __forceinline__ void eot_gy(const float* g, const int32_t* inv, int K, int L, int i, float* r) {
  if (!inv) {
    r[0] = g[i], r[1] = g[K + i], r[2] = g[2 * K + i];
    return;
  }
  const int j0 = inv[2 * i], j1 = inv[2 * i + 1];
  const bool h0 = j0 >= 0 && j0 < L, h1 = j1 >= 0 && j1 < L;
  r[0] = r[1] = r[2] = 0.f;
  if (h0) r[0] = g[j0], r[1] = g[K + j0], r[2] = g[2 * K + j0];
  if (h1) {
    if (h0)
      r[0] += g[j1], r[1] += g[K + j1], r[2] += g[2 * K + j1];
    else
      r[0] = g[j1], r[1] = g[K + j1], r[2] = g[2 * K + j1];
  }
}

// RAGGED: as in the prepare launch, every walk, divisor and index bound is the cloud's L = lengths[b] (clamped to [1, K]); the
// rows >= L are never read, keep their m / v, and leave as copies of point 0: the iterate's of its NEW point 0, input_val's
// and (on a copy) o_bestattack's of the point 0 they copy, both handed over through LDS. With L = K every output has the
// dense instantiation's bits.
template <bool RAGGED>
__global__ __launch_bounds__(kEuThreads) void eot_update_kernel(typename EotUpdArgsOf<RAGGED>::type a) {
  extern __shared__ __attribute__((aligned(16))) float acc[];      // [3,K]
  __shared__ float red[kEuThreads / 64];
  __shared__ double redd[kEuThreads / 64];
  __shared__ float s_adam[2];
  __shared__ int s_copy;
  const int b = blockIdx.x, tid = threadIdx.x, K = a.K, B = a.B;
  int L = K;
  if constexpr (RAGGED) L = min(max(a.lengths[b], 1), K);
  float* adv = a.adv + (int64_t)b * 3 * K;
  const float* ori = a.ori + (int64_t)b * 3 * K;
  const int32_t* nn = a.nn_idx ? a.nn_idx + (int64_t)b * K : nullptr;
  const float wb = a.w ? a.w[b] : 1.f;

  // ---- record: the distance of the iterate just evaluated, the decisions on slot 0's prediction ----
  float part = 0.f;
#pragma unroll 1
  for (int i = tid; i < L; i += kEuThreads) {
    if (a.dist_kind) {
      int j = i;
      if (a.dist_kind == 2) j = min(max(nn[i], 0), L - 1);
      const float d0 = adv[i] - ori[j], d1 = adv[K + i] - ori[K + j], d2 = adv[2 * K + i] - ori[2 * K + j];
      part += d0 * d0 + d1 * d1 + d2 * d2;
    }
  }
  const float tot = block_sum_ordered<kEuThreads / 64>(part, red);
  const float nrm = __builtin_sqrtf(tot);
  const float dist = a.dist_kind == 2 ? wb * (tot / (float)L) : (a.dist_kind == 1 ? wb * nrm : 0.f);
  if (tid == 0) {
    s_copy = cw_book_decide(a.dist_val, a.bestdist, a.bestscore, a.o_bestdist, a.o_bestscore, a.untarget, b, dist, a.pred[b],
                            a.goal[b], a.bestdist[b], a.o_bestdist[b]);
    const int t = a.step_dev ? a.step_dev[0] : a.step_host;
    s_adam[0] = adam_step_size(a.lr, a.b1, t);
    s_adam[1] = adam_bc2s(a.b2, t);
  }

  // ---- gradient of the adversarial term: the views in ascending order (without EOT: slot 0) ----
  // (the accumulators: LDS, 12 bytes a point, every entry touched by the one thread that owns the point)
#pragma unroll 1
  for (int i = tid; i < L; i += kEuThreads) acc[i] = acc[K + i] = acc[2 * K + i] = 0.f;
  const int t = eot_table_row(a.step_dev, a.step_host, 1, a.T);      // the row the prepare launch read: the step has advanced
  for (int e = a.E ? 1 : 0; e <= a.E; ++e) {
    const int row = e * B + b;
    const float* g = a.gx + (int64_t)row * 3 * K;
    const bool view = e >= 1;
    float R[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    if (view) {
      const float* rp = a.rot + ((int64_t)t * a.E + (e - 1)) * 9;
#pragma unroll
      for (int k = 0; k < 9; ++k) R[k] = rp[k];
    }
    const int32_t* inv = nullptr;
    if (view && a.inv) {
      if constexpr (RAGGED) inv = a.inv + (((int64_t)t * a.E + (e - 1)) * B + b) * K * 2;
      else inv = a.inv + ((int64_t)t * a.E + (e - 1)) * K * 2;
    }
    if (!a.renorm) {
#pragma unroll 1
      for (int i = tid; i < L; i += kEuThreads) {
        float gy[3];
        eot_gy(g, inv, K, L, i, gy);
        acc[i] += gy[0], acc[K + i] += gy[1], acc[2 * K + i] += gy[2];
      }
      continue;
    }
    const float c[3] = {a.stats[(int64_t)row * 4], a.stats[(int64_t)row * 4 + 1], a.stats[(int64_t)row * 4 + 2]};
    const float s = a.stats[(int64_t)row * 4 + 3];
    const int am = min(max(a.arg[row], 0), L - 1);
    // The two sums of the renormalisation's backward in double: sum g_y . q cancels (its terms have both signs) and lands,
    // times q_a / s^3, on ONE point, so its rounding would be that point's whole error; q is formed from the fp32 inputs
    // without the roundings of the forward's p.
    double sg[3] = {0.0, 0.0, 0.0}, sd = 0.0;
#pragma unroll 1
    for (int i = tid; i < L; i += kEuThreads) {
      float gy[3];
      double q[3];
      eot_gy(g, inv, K, L, i, gy);
      eot_q64(adv, ori, K, i, view, R, c, q);
      sg[0] += gy[0], sg[1] += gy[1], sg[2] += gy[2];
      sd += (gy[0] * q[0] + gy[1] * q[1]) + gy[2] * q[2];
    }
    double S[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) S[k] = block_sum_ordered<kEuThreads / 64>(sg[k], redd);
    const double D = block_sum_ordered<kEuThreads / 64>(sd, redd);
    const double ds = -D / ((double)s * (double)s);
    double qa[3];
    float ua[3], mean[3];
    eot_q64(adv, ori, K, am, view, R, c, qa);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double uk = ds * (qa[k] / (double)s);      // |q_a| = s
      ua[k] = (float)uk;
      mean[k] = (float)((S[k] / (double)s + uk) / (double)L);
    }
#pragma unroll 1
    for (int i = tid; i < L; i += kEuThreads) {
      float gy[3];
      eot_gy(g, inv, K, L, i, gy);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        float gq = gy[k] / s;
        if (i == am) gq += ua[k];
        acc[k * K + i] += gq - mean[k];
      }
    }
  }
  __syncthreads();      // s_copy, s_adam

  // ---- distance gradient, Adam, the z-only box; the copies of the iterate as it stood ----
  const AdamConsts ad = adam_consts_with(a.b1, a.b2, a.eps, s_adam[0], s_adam[1]);
  const int copy = s_copy;
  const float cch = 2.f * wb / ((float)a.batch_mean * (float)L), cl2 = wb / (float)a.batch_mean;
  float* mb = a.m + (int64_t)b * 3 * K;
  float* vb = a.v + (int64_t)b * 3 * K;
#pragma unroll 1
  for (int i = tid; i < L; i += kEuThreads) {
    const float x[3] = {adv[i], adv[K + i], adv[2 * K + i]};
    const float o[3] = {ori[i], ori[K + i], ori[2 * K + i]};
    float gd[3] = {0.f, 0.f, 0.f};
    if (a.dist_kind == 2) {
      const int j = min(max(nn[i], 0), L - 1);
      gd[0] = cch * (x[0] - ori[j]), gd[1] = cch * (x[1] - ori[K + j]), gd[2] = cch * (x[2] - ori[2 * K + j]);
    } else if (a.dist_kind == 1) {
#pragma unroll
      for (int k = 0; k < 3; ++k) gd[k] = cl2 * ((x[k] - o[k]) / nrm);      // 0 / 0 at adv == ori, as torch
    }
    float nw[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      float mm = mb[k * K + i], vv = vb[k * K + i];
      const float gk = acc[k * K + i] + gd[k];
      nw[k] = adam_element(ad, x[k], gk, mm, vv);
      if (a.g_out) a.g_out[(int64_t)b * 3 * K + k * K + i] = gk;
      mb[k * K + i] = mm, vb[k * K + i] = vv;
      if (a.input_val) a.input_val[(int64_t)b * 3 * K + k * K + i] = x[k];
      if (copy) a.o_bestattack[(int64_t)b * 3 * K + k * K + i] = x[k];
    }
    if (a.one_d) {
      const float hi = o[2] + a.box, lo = o[2] - a.box;
      nw[0] = o[0], nw[1] = o[1];
      if (nw[2] > hi) nw[2] = hi;      // a NaN stays, as through torch.min / torch.max
      if (nw[2] < lo) nw[2] = lo;
    }
    adv[i] = nw[0], adv[K + i] = nw[1], adv[2 * K + i] = nw[2];
    if constexpr (RAGGED) {
      if (i == 0) {      // thread 0: point 0 before and after the update, for the padding rows
        float* s_pad = eot_pad_slot();
#pragma unroll
        for (int k = 0; k < 3; ++k) s_pad[k] = x[k], s_pad[3 + k] = nw[k];
      }
    }
  }
  if constexpr (RAGGED) {
    __syncthreads();
    const float* s_pad = eot_pad_slot();
    const float o0[3] = {s_pad[0], s_pad[1], s_pad[2]}, n0[3] = {s_pad[3], s_pad[4], s_pad[5]};
#pragma unroll 1
    for (int i = L + tid; i < K; i += kEuThreads) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        if (a.input_val) a.input_val[(int64_t)b * 3 * K + k * K + i] = o0[k];
        if (copy) a.o_bestattack[(int64_t)b * 3 * K + k * K + i] = o0[k];
        adv[k * K + i] = n0[k];
      }
    }
  }
}


// ---- the loop's tables drawn on the device: a pure function of (seed, n, e), include/pc3d.h states it ----
constexpr int kEdIdxBits = 14;      // a column c < 2 K <= 2^14 rides in the low bits of its key
static_assert(2 * kEotMaxPoints <= (1 << kEdIdxBits), "every column of cat((x, x), 2) fits the key's low bits");
static_assert((size_t)2 * kEotMaxPoints * sizeof(uint64_t) <= 160 * 1024, "the keys of the largest cloud fit the CU's LDS");

// One workgroup per (row, view). keys[c] for the columns c = 1 .. 2K - 1, pads (slot 0 and the slots from 2K on) sort to the
// end; ascending bitonic network over P = 2^p >= 2K slots, a barrier after EVERY stage (block_bitonic_sort_u64, srs_select_kernel's). The
// sorted array's upper part, dead after the sort (P - K >= K words of 8 bytes), then holds pos[2K] (column -> position or
// -1), from which the inverse table is gathered: no atomics.
//
// RAGGED (one workgroup per (row, view, cloud), idx [T,E,B,K], inv [T,E,B,K,2]): cloud b's table is the dense one of a cloud
// of L = lengths[b] points (clamped to [1, K]): the keys of the columns 1 .. 2L - 1 — the cloud index is not part of a key —
// sorted over the smallest 2^p >= 2L slots. The keys are distinct and the pads sort last, so the table does not depend on
// the slots or threads of the launch. Entries >= L: idx takes the cloud's idx[0], inv -1. Cloud 0's workgroup writes the
// rotation, which the batch shares. The dense body compiles as before: Kc is K, Pc is P.
template <bool RAGGED>
__device__ __forceinline__ void eot_draw_body(uint64_t seed, uint64_t n0, int row0, int E, int K, int P,
                                              float* __restrict__ rot, int32_t* __restrict__ idx, int32_t* __restrict__ inv,
                                              int B, const int32_t* __restrict__ lengths) {
  extern __shared__ __attribute__((aligned(16))) uint64_t ed_keys[];
  const int e = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
  const uint64_t n = n0 + (uint64_t)blockIdx.y;
  const int64_t cell = (int64_t)(row0 + (int)blockIdx.y) * E + e;
  const uint64_t s = mix64(seed + 0x9E3779B97F4A7C15ull * (16ull * n + (uint64_t)e + 1ull));
  const int b = RAGGED ? (int)blockIdx.z : 0;
  const int Kc = K;      // the capacity: the tables' row stride
  if constexpr (RAGGED) {
    K = min(max(lengths[b], 1), Kc);
    int p2 = 2;
    while (p2 < 2 * K) p2 <<= 1;
    P = p2;              // <= the launch's P, which the LDS holds
  }
  if (tid == 0 && b == 0) {
    const double two53 = 1.0 / 9007199254740992.0;
    const uint64_t u0 = mix64(s ^ (1ull << 32)), u1 = mix64(s ^ (1ull << 33)), u2 = mix64(s ^ (1ull << 34));
    const double rad = sqrt(-2.0 * log((double)((u0 >> 11) + 1ull) * two53));
    const double theta = 1e-2 * rad * cos(6.283185307179586476925286766559 * ((double)(u1 >> 11) * two53));
    const float c = (float)cos(theta), sn = (float)sin(theta);
    const double r = (double)(u2 >> 11) * two53;
    float R[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    if (r < 0.2)
      R[0] = c, R[1] = sn, R[3] = -sn, R[4] = c;
    else if (r < 0.4)
      R[4] = c, R[5] = sn, R[7] = -sn, R[8] = c;
    else if (r < 0.6)
      R[0] = c, R[2] = sn, R[6] = -sn, R[8] = c;
    float* rp = rot + cell * 9;
#pragma unroll
    for (int k = 0; k < 9; ++k) rp[k] = R[k];
  }
  if (!idx) return;
  const uint64_t lowmask = (1ull << kEdIdxBits) - 1ull;
  for (int c = tid; c < P; c += T)
    ed_keys[c] = (c >= 1 && c < 2 * K) ? ((mix64(s ^ (uint64_t)c) & ~lowmask) | (uint64_t)c) : ~0ull;
  __syncthreads();
  block_bitonic_sort_u64(ed_keys, P, tid, T);
  int32_t* pos = reinterpret_cast<int32_t*>(ed_keys + K);      // [2K] int32 = K words, inside keys[K .. 2K) (2K <= P)
  for (int c = tid; c < 2 * K; c += T) pos[c] = -1;
  __syncthreads();
  int32_t* ix = idx + (RAGGED ? cell * B + b : cell) * Kc;
  const int c0 = (int)(ed_keys[0] & lowmask);      // (keys[0 .. K) stay: pos lies behind them)
  for (int j = tid; j < K; j += T) {
    const int c = (int)(ed_keys[j] & lowmask);      // 1 <= c <= 2K - 1: K <= 2K - 1 real keys sort in front of the pads
    ix[j] = c;
    pos[c] = j;
  }
  __syncthreads();
  int32_t* iv = inv + (RAGGED ? cell * B + b : cell) * Kc * 2;
  for (int i = tid; i < K; i += T) {      // point i is drawn by the columns i (none for i = 0: column 0 is never drawn) and i + K
    const int a = i >= 1 ? pos[i] : -1, b2 = pos[i + K];
    const int first = a < 0 ? b2 : (b2 < 0 ? a : min(a, b2));
    const int second = (a < 0 || b2 < 0) ? -1 : max(a, b2);
    iv[2 * i] = first, iv[2 * i + 1] = second;
  }
  if constexpr (RAGGED) {
    for (int j = K + tid; j < Kc; j += T) ix[j] = c0, iv[2 * j] = -1, iv[2 * j + 1] = -1;
  }
}

__global__ __launch_bounds__(1024) void eot_draw_kernel(uint64_t seed, uint64_t n0, int row0, int E, int K, int P,
                                                        float* __restrict__ rot, int32_t* __restrict__ idx,
                                                        int32_t* __restrict__ inv) {
  eot_draw_body<false>(seed, n0, row0, E, K, P, rot, idx, inv, 1, nullptr);
}

__global__ __launch_bounds__(1024) void eot_draw_ragged_kernel(uint64_t seed, uint64_t n0, int row0, int E, int K, int P,
                                                               float* __restrict__ rot, int32_t* __restrict__ idx,
                                                               int32_t* __restrict__ inv, int B,
                                                               const int32_t* __restrict__ lengths) {
  eot_draw_body<true>(seed, n0, row0, E, K, P, rot, idx, inv, B, lengths);
}

}  // namespace pc3d

using namespace pc3d;

// the checks and the launch of both draw entries; ragged false: the dense kernel, B and lengths unused
static int eot_draw_launch(const char* nm, int64_t seed, int64_t n0, int row0, int cnt, int T, int E, int B, int K,
                           const int32_t* lengths, bool ragged, float* rot, int32_t* idx, int32_t* inv, void* stream) {
  PC3D_REQUIRE(K >= 1 && K <= kEotMaxPoints, "%s: K=%d out of range [1,%d]", nm, K, kEotMaxPoints);
  PC3D_REQUIRE(E >= 1 && E <= kEotMaxViews, "%s: E=%d out of range [1,%d]", nm, E, kEotMaxViews);
  PC3D_REQUIRE(n0 >= 0, "%s: the draw index n0=%lld must be >= 0", nm, (long long)n0);
  PC3D_REQUIRE(row0 >= 0 && cnt >= 0 && T >= 0 && cnt <= T && row0 <= T - cnt, "%s: rows [%d, %d + %d) leave the table of T=%d rows",
               nm, row0, row0, cnt, T);
  PC3D_REQUIRE(cnt <= 65535, "%s: cnt=%d exceeds grid.y limit", nm, cnt);
  PC3D_REQUIRE(!ragged || (B >= 0 && B <= 65535), "%s: B=%d exceeds grid.z limit", nm, B);
  PC3D_REQUIRE((idx == nullptr) == (inv == nullptr), "%s: idx and inv are given together or not at all", nm);
  if (cnt == 0 || (ragged && B == 0)) return PC3D_OK;
  PC3D_REQUIRE(rot && (!ragged || lengths), "%s: null pointer", nm);
  int P = 2;
  while (P < 2 * K) P <<= 1;
  int threads = P / 2;
  threads = threads < kWave ? kWave : (threads > 1024 ? 1024 : threads);
  const size_t lds = idx ? (size_t)P * sizeof(uint64_t) : 0;
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute(ragged ? reinterpret_cast<const void*>(eot_draw_ragged_kernel)
                                              : reinterpret_cast<const void*>(eot_draw_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 2 * kEotMaxPoints * (int)sizeof(uint64_t));
    if (e != hipSuccess) {
      set_error("%s: LDS opt-in failed: %s", nm, hipGetErrorString(e));
      return (int)e;
    }
  }
  if (!ragged)
    hipLaunchKernelGGL(eot_draw_kernel, dim3(E, cnt), dim3(threads), lds, as_stream(stream), (uint64_t)seed, (uint64_t)n0, row0, E,
                       K, P, rot, idx, inv);
  else
    hipLaunchKernelGGL(eot_draw_ragged_kernel, dim3(E, cnt, B), dim3(threads), lds, as_stream(stream), (uint64_t)seed,
                       (uint64_t)n0, row0, E, K, P, rot, idx, inv, B, lengths);
  PC3D_LAUNCH_CHECK(nm);
  return PC3D_OK;
}

extern "C" int pc3d_eot_draw_f32(int64_t seed, int64_t n0, int row0, int cnt, int T, int E, int K, float* rot, int32_t* idx,
                                 int32_t* inv, void* stream) {
  return eot_draw_launch("pc3d_eot_draw_f32", seed, n0, row0, cnt, T, E, 1, K, nullptr, false, rot, idx, inv, stream);
}

extern "C" int pc3d_eot_draw_ragged_f32(int64_t seed, int64_t n0, int row0, int cnt, int T, int E, int B, int K,
                                        const int32_t* lengths, float* rot, int32_t* idx, int32_t* inv, void* stream) {
  return eot_draw_launch("pc3d_eot_draw_ragged_f32", seed, n0, row0, cnt, T, E, B, K, lengths, true, rot, idx, inv, stream);
}

// the checks, the argument block and the launch of both prepare entries
static int eot_prepare_launch(const char* nm, const float* adv, const float* ori, int B, int K, const int32_t* lengths,
                              bool ragged, int E, int T, const float* rot, const int32_t* idx, int renorm,
                              const int32_t* step_dev, int step_host, float* X, float* stats, int32_t* arg, void* stream) {
  PC3D_REQUIRE(B >= 0 && K >= 1 && K <= kEotMaxPoints, "%s: bad sizes B=%d K=%d (1 <= K <= %d)", nm, B, K, kEotMaxPoints);
  PC3D_REQUIRE(E >= 0 && E <= kEotMaxViews, "%s: E=%d out of range [0,%d]", nm, E, kEotMaxViews);
  PC3D_REQUIRE(E == 0 || (T >= 1 && rot != nullptr), "%s: E=%d views need a rotation table (T=%d)", nm, E, T);
  PC3D_REQUIRE(E > 0 || idx == nullptr, "%s: resampling without views", nm);
  PC3D_REQUIRE((int64_t)(1 + E) * B <= 0x7fffffff, "%s: (1 + E) B too large", nm);
  if (B == 0) return PC3D_OK;
  PC3D_REQUIRE(adv && ori && X && stats && arg && (!ragged || lengths), "%s: null pointer", nm);
  EotPrepRaggedArgs a{};
  static_cast<EotPrepArgs&>(a) = EotPrepArgs{adv, ori, rot, idx, B, K, E, E ? T : 1, renorm ? 1 : 0, step_dev, step_host, X, stats, arg};
  a.lengths = lengths;
  if (!ragged)
    hipLaunchKernelGGL(eot_prepare_kernel<false>, dim3((1 + E) * B), dim3(kEpThreads), 0, as_stream(stream),
                       static_cast<const EotPrepArgs&>(a));
  else
    hipLaunchKernelGGL(eot_prepare_kernel<true>, dim3((1 + E) * B), dim3(kEpThreads), 0, as_stream(stream), a);
  PC3D_LAUNCH_CHECK(nm);
  return PC3D_OK;
}

extern "C" int pc3d_eot_prepare_f32(const float* adv, const float* ori, int B, int K, int E, int T, const float* rot,
                                    const int32_t* idx, int renorm, const int32_t* step_dev, int step_host, float* X,
                                    float* stats, int32_t* arg, void* stream) {
  return eot_prepare_launch("pc3d_eot_prepare_f32", adv, ori, B, K, nullptr, false, E, T, rot, idx, renorm, step_dev, step_host,
                            X, stats, arg, stream);
}

extern "C" int pc3d_eot_prepare_ragged_f32(const float* adv, const float* ori, int B, int K, const int32_t* lengths, int E,
                                           int T, const float* rot, const int32_t* idx, int renorm, const int32_t* step_dev,
                                           int step_host, float* X, float* stats, int32_t* arg, void* stream) {
  return eot_prepare_launch("pc3d_eot_prepare_ragged_f32", adv, ori, B, K, lengths, true, E, T, rot, idx, renorm, step_dev,
                            step_host, X, stats, arg, stream);
}

// the checks, the argument block and the launch of both update entries
static int eot_update_launch(const char* nm, float* adv, const float* ori, const float* gx, float* m, float* v, int B, int K,
                             const int32_t* lengths, bool ragged, int E, int T, const float* rot, const int32_t* inv, int renorm,
                             const float* stats, const int32_t* arg, const int64_t* pred, const int64_t* goal, int untarget,
                             float* bestdist, int64_t* bestscore, float* o_bestdist, int64_t* o_bestscore, float* o_bestattack,
                             float* input_val, float* dist_val, float* g_out, int dist_kind, const float* w,
                             const int32_t* nn_idx, int batch_mean, double lr, double beta1, double beta2, double eps, int one_d,
                             float box, const int32_t* step_dev, int step_host, void* stream) {
  PC3D_REQUIRE(B >= 0 && K >= 1 && K <= kEotMaxPoints, "%s: bad sizes B=%d K=%d (1 <= K <= %d)", nm, B, K, kEotMaxPoints);
  PC3D_REQUIRE(E >= 0 && E <= kEotMaxViews, "%s: E=%d out of range [0,%d]", nm, E, kEotMaxViews);
  PC3D_REQUIRE(E == 0 || (T >= 1 && rot != nullptr), "%s: E=%d views need a rotation table (T=%d)", nm, E, T);
  PC3D_REQUIRE(E > 0 || inv == nullptr, "%s: resampling without views", nm);
  PC3D_REQUIRE(dist_kind >= 0 && dist_kind <= 2, "%s: dist_kind=%d not in {0,1,2}", nm, dist_kind);
  PC3D_REQUIRE(batch_mean >= 1, "%s: batch_mean=%d must be >= 1", nm, batch_mean);
  PC3D_REQUIRE(step_dev != nullptr || step_host >= 1, "%s: step_host must be >= 1 without a device counter", nm);
  if (B == 0) return PC3D_OK;
  PC3D_REQUIRE(adv && ori && gx && m && v && (!ragged || lengths), "%s: null pointer", nm);
  PC3D_REQUIRE(!renorm || (stats && arg), "%s: the renormalisation's backward needs stats and arg", nm);
  PC3D_REQUIRE(dist_kind != 2 || nn_idx != nullptr, "%s: the Chamfer term needs nn_idx", nm);
  PC3D_REQUIRE(pred && goal && bestdist && bestscore && o_bestdist && o_bestscore && o_bestattack,
               "%s: the record block needs pred, goal and the best-so-far buffers", nm);
  EotUpdRaggedArgs a{};
  static_cast<EotUpdArgs&>(a) =
      EotUpdArgs{adv, ori, gx, m, v, B, K, E, E ? T : 1, renorm ? 1 : 0, rot, inv, stats, arg, pred, goal, untarget ? 1 : 0,
                 bestdist, bestscore, o_bestdist, o_bestscore, o_bestattack, input_val, dist_val, g_out, dist_kind, w, nn_idx,
                 batch_mean, lr, beta1, beta2, (float)eps, one_d ? 1 : 0, box, step_dev, step_host};
  a.lengths = lengths;
  const size_t lds = (size_t)K * 12;
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute(ragged ? reinterpret_cast<const void*>(eot_update_kernel<true>)
                                              : reinterpret_cast<const void*>(eot_update_kernel<false>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, kEotMaxPoints * 12);
    if (e != hipSuccess) {
      set_error("%s: LDS opt-in failed: %s", nm, hipGetErrorString(e));
      return (int)e;
    }
  }
  if (!ragged)
    hipLaunchKernelGGL(eot_update_kernel<false>, dim3(B), dim3(kEuThreads), lds, as_stream(stream),
                       static_cast<const EotUpdArgs&>(a));
  else
    hipLaunchKernelGGL(eot_update_kernel<true>, dim3(B), dim3(kEuThreads), lds, as_stream(stream), a);
  PC3D_LAUNCH_CHECK(nm);
  return PC3D_OK;
}

extern "C" int pc3d_eot_update_f32(float* adv, const float* ori, const float* gx, float* m, float* v, int B, int K, int E, int T,
                                   const float* rot, const int32_t* inv, int renorm, const float* stats, const int32_t* arg,
                                   const int64_t* pred, const int64_t* goal, int untarget, float* bestdist, int64_t* bestscore,
                                   float* o_bestdist, int64_t* o_bestscore, float* o_bestattack, float* input_val,
                                   float* dist_val, float* g_out, int dist_kind, const float* w, const int32_t* nn_idx, int batch_mean,
                                   double lr, double beta1, double beta2, double eps, int one_d, float box,
                                   const int32_t* step_dev, int step_host, void* stream) {
  return eot_update_launch("pc3d_eot_update_f32", adv, ori, gx, m, v, B, K, nullptr, false, E, T, rot, inv, renorm, stats, arg,
                           pred, goal, untarget, bestdist, bestscore, o_bestdist, o_bestscore, o_bestattack, input_val, dist_val,
                           g_out, dist_kind, w, nn_idx, batch_mean, lr, beta1, beta2, eps, one_d, box, step_dev, step_host, stream);
}

extern "C" int pc3d_eot_update_ragged_f32(float* adv, const float* ori, const float* gx, float* m, float* v, int B, int K,
                                          const int32_t* lengths, int E, int T, const float* rot, const int32_t* inv, int renorm,
                                          const float* stats, const int32_t* arg, const int64_t* pred, const int64_t* goal,
                                          int untarget, float* bestdist, int64_t* bestscore, float* o_bestdist,
                                          int64_t* o_bestscore, float* o_bestattack, float* input_val, float* dist_val,
                                          float* g_out, int dist_kind, const float* w, const int32_t* nn_idx, int batch_mean,
                                          double lr, double beta1, double beta2, double eps, int one_d, float box,
                                          const int32_t* step_dev, int step_host, void* stream) {
  return eot_update_launch("pc3d_eot_update_ragged_f32", adv, ori, gx, m, v, B, K, lengths, true, E, T, rot, inv, renorm, stats,
                           arg, pred, goal, untarget, bestdist, bestscore, o_bestdist, o_bestscore, o_bestattack, input_val,
                           dist_val, g_out, dist_kind, w, nn_idx, batch_mean, lr, beta1, beta2, eps, one_d, box, step_dev,
                           step_host, stream);
}
