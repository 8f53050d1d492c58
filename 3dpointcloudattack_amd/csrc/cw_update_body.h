// The CW iteration's per-point update and per-sample bookkeeping as device functions: the stand-alone kernels of
// attack_step.hip, the bookkeeping rider of a linear launch (linear_riders.hip) and the update epilogue of the tower
// backward (pointmlp.hip) compile these statements, so every form of the iteration computes the same bits.
// The Adam element, ClipPointsLinf and the decision itself are update_body.h's.
#pragma once
#include "update_body.h"

namespace pc3d {

struct BookArgs {
  PtsView adv, ori;          // [B,K] points
  int K;
  const int64_t* pred;       // [B]
  const int64_t* label;      // [B]
  int untarget;              // success = pred != label (1) or pred == label (0)
  float* bestdist;           // [B] per-binary-step best
  int64_t* bestscore;        // [B]
  float* o_bestdist;         // [B] overall best
  int64_t* o_bestscore;      // [B]
  PtsViewMut o_bestattack;   // [B,K] points: copy of adv where the overall best improved
  PtsViewMut input_val;      // [B,K] points: always the iterate this pass started from (may be null)
  float* dist_val;           // [B] out: ||adv-ori||_F (feeds the L2 distance gradient)
  int32_t* step;             // Adam step word, incremented once per launch (may be null)
};

// The constants of one update launch that do not depend on the point
struct CwPointConsts {
  int dist_kind;             // 0: none, 1: L2Dist, 2: ChamferDist adv2ori
  int B, K;
  AdamConsts ad;
  float budget;
};

// One point of the CW update: g = g_model + d/dadv [ mean_b w_b * D(adv_b, ori_b) ], then Adam, then ClipPointsLinf.
//   p / o: the point and its original; g: the victim's gradient (the distance term is added in place);
//   q: ori[nn_idx] (kind 2); wb = w[b]; l2n = ||adv_b - ori_b||_F (kind 1); m / v: Adam moments, updated in place;
//   np: the new point.
__device__ __forceinline__ void cw_point_update(const CwPointConsts& c, const float (&p)[3], const float (&o)[3],
                                                float (&g)[3], const float (&q)[3], float wb, float l2n, float (&m)[3],
                                                float (&v)[3], float (&np)[3]) {
  if (c.dist_kind == 1) {
    // torch: d sqrt(s)/ds = 1/(2 sqrt(s)), ds/dp = 2 (p - o)  ->  (p-o)/norm ; weight/B from the batch mean
    const float cc = wb / (float)c.B;
    g[0] += cc * ((p[0] - o[0]) / l2n);
    g[1] += cc * ((p[1] - o[1]) / l2n);
    g[2] += cc * ((p[2] - o[2]) / l2n);
  } else if (c.dist_kind == 2) {
    const float cc = 2.f * (wb / (float)c.B) / (float)c.K;
    g[0] += cc * (p[0] - q[0]);
    g[1] += cc * (p[1] - q[1]);
    g[2] += cc * (p[2] - q[2]);
  }
  float np_[3];
#pragma unroll
  for (int e = 0; e < 3; ++e) np_[e] = adam_element(c.ad, p[e], g[e], m[e], v[e]);
  np[0] = np_[0] - o[0], np[1] = np_[1] - o[1], np[2] = np_[2] - o[2];
  clip_linf(np[0], np[1], np[2], c.budget);
  np[0] = o[0] + np[0];
  np[1] = o[1] + np[1];
  np[2] = o[2] + np[2];
}

// the decision on a BookArgs. The kernels go through this form: with the six words passed at their call sites instead, the
// register-bound cw_update_kernel<2/4/8> allocate worse (83 VGPRs for 77, scratch 36 for 0 and 504 for 280 bytes a lane)
__device__ __forceinline__ int cw_book_decide(const BookArgs& a, int b, float dist, int64_t pr, int64_t lb, float bd, float obd) {
  return cw_book_decide(a.dist_val, a.bestdist, a.bestscore, a.o_bestdist, a.o_bestscore, a.untarget, b, dist, pr, lb, bd, obd);
}

constexpr int kCwBookThreads = 512;

// Bookkeeping of sample b by ONE 512-thread workgroup with the reduction tree of cw_update_kernel<PER> (1024 threads):
// thread t stands for that kernel's threads t and t + 512 — its per-thread sums run over points tid + i * 1024, the 16
// partial sums are the wave_sum of one 64-lane group each, added in ascending order — then the square root, the
// decisions and the copies. adam (may be null): workgroup 0 also writes {step_size, bc2s} for the step word's value.
__device__ __forceinline__ void cw_book_body(const BookArgs& a, int b, double lr, double b1, double b2, const int32_t* step_dev,
                                             float* adam) {
  __shared__ float part[16];
  __shared__ int s_copy;
  const int tid = threadIdx.x;
  const int64_t pr = a.pred[b], lb = a.label[b];
  const float bd = a.bestdist[b], obd = a.o_bestdist[b];
  const int per = (a.K + 1023) >> 10;
  float acc[2] = {0.f, 0.f};
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll 2
    for (int i = 0; i < per; ++i) {
      const int k = tid + h * kCwBookThreads + i * 1024;
      float dx = 0.f, dy = 0.f, dz = 0.f;
      if (k < a.K) {
        const float* p = a.adv.p + (int64_t)b * a.adv.bs + (int64_t)k * a.adv.ps;
        const float* o = a.ori.p + (int64_t)b * a.ori.bs + (int64_t)k * a.ori.ps;
        dx = p[0] - o[0], dy = p[a.adv.cs] - o[a.ori.cs], dz = p[2 * a.adv.cs] - o[2 * a.ori.cs];
      }
      acc[h] += dx * dx + dy * dy + dz * dz;
    }
  }
  acc[0] = wave_sum(acc[0]);
  acc[1] = wave_sum(acc[1]);
  if ((tid & 63) == 0) part[tid >> 6] = acc[0], part[8 + (tid >> 6)] = acc[1];
  __syncthreads();
  if (tid == 0) {
    float tot = 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) tot += part[w];
    const float dist = __builtin_sqrtf(tot);
    s_copy = cw_book_decide(a, b, dist, pr, lb, bd, obd);
    if (adam && b == 0) {
      const int t = step_dev[0];
      adam[0] = adam_step_size(lr, b1, t);
      adam[1] = adam_bc2s(b2, t);
    }
  }
  __syncthreads();
  const bool copy = s_copy != 0;
  if (!copy && a.input_val.p == nullptr) return;
  for (int k = tid; k < a.K; k += kCwBookThreads) {
    const float* p = a.adv.p + (int64_t)b * a.adv.bs + (int64_t)k * a.adv.ps;
    const float x = p[0], y = p[a.adv.cs], z = p[2 * a.adv.cs];
    if (a.input_val.p) {
      float* q = a.input_val.p + (int64_t)b * a.input_val.bs + (int64_t)k * a.input_val.ps;
      q[0] = x, q[a.input_val.cs] = y, q[2 * a.input_val.cs] = z;
    }
    if (copy) {
      float* q = a.o_bestattack.p + (int64_t)b * a.o_bestattack.bs + (int64_t)k * a.o_bestattack.ps;
      q[0] = x, q[a.o_bestattack.cs] = y, q[2 * a.o_bestattack.cs] = z;
    }
  }
}

}  // namespace pc3d
