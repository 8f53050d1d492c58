// The optimiser step of the attack loops as device functions: torch.optim.Adam on one element, the per-point clips and
// the best-attack decision. Every update kernel (elementwise.hip, cw_update_body.h, aof.hip, add_step.hip, knn_attack.hip,
// geoa3_loop.hip, iso.hip) compiles THESE statements, so every form of an iteration computes the same bits; the build
// keeps -ffp-contract=off, so inlining does not change them. tests/test_update_bits_gpu.py holds them to recorded bits.
#pragma once
#include "pc3d_common.h"

namespace pc3d {

// torch.optim.Adam, single-tensor form, weight_decay 0, amsgrad off:
//   m += (g - m)(1-b1);  v = v*b2 + (1-b2) g*g;  denom = sqrt(v)/sqrt(1-b2^t) + eps;  p -= lr/(1-b1^t) * m/denom
// The scalars follow torch's python-double arithmetic (1-beta, 1-beta**t, lr/bc1 in double), rounded to fp32 once.
struct AdamConsts {
  float omb1, omb2, fb2;     // (float)(1 - beta1), (float)(1 - beta2), (float)beta2
  float step_size, bc2s;     // adam_step_size / adam_bc2s
  float eps;
};

// the two bias-correction factors for step t
__device__ __forceinline__ float adam_step_size(double lr, double b1, int t) { return (float)(lr / (1.0 - pow(b1, (double)t))); }
__device__ __forceinline__ float adam_bc2s(double b2, int t) { return (float)sqrt(1.0 - pow(b2, (double)t)); }

// for the kernels that evaluate the two factors once per workgroup and hand them on through LDS
__device__ __forceinline__ AdamConsts adam_consts_with(double b1, double b2, float eps, float step_size, float bc2s) {
  return AdamConsts{(float)(1.0 - b1), (float)(1.0 - b2), (float)b2, step_size, bc2s, eps};
}
__device__ __forceinline__ AdamConsts adam_consts(double lr, double b1, double b2, float eps, int t) {
  return adam_consts_with(b1, b2, eps, adam_step_size(lr, b1, t), adam_bc2s(b2, t));
}

// one element: the moments are updated in place; returns denom
__device__ __forceinline__ float adam_moments(const AdamConsts& c, float g, float& m, float& v) {
  m = m + (g - m) * c.omb1;
  v = v * c.fb2 + c.omb2 * g * g;
  return __builtin_sqrtf(v) / c.bc2s + c.eps;
}
// ... and the new value of the parameter p
__device__ __forceinline__ float adam_element(const AdamConsts& c, float p, float g, float& m, float& v) {
  const float denom = adam_moments(c, g, m, v);
  return p - c.step_size * (m / denom);
}

// ClipPointsLinf (clip_utils.py:43-56) on one point's perturbation: a per-point L2 budget ("Linf" in the reference's
// naming); budget <= 0: no clip
__device__ __forceinline__ void clip_linf(float& dx, float& dy, float& dz, float budget) {
  if (budget > 0.f) {
    const float norm = __builtin_sqrtf(dx * dx + dy * dy + dz * dz);
    const float s = fminf(budget / (norm + 1e-9f), 1.f);
    dx *= s, dy *= s, dz *= s;
  }
}

// ProjectInnerPoints (clip_utils.py:67-108) on one point's perturbation, n the point's normal
__device__ __forceinline__ void project_inner(float& dx, float& dy, float& dz, float nx, float ny, float nz) {
  const float inner = dx * nx + dy * ny + dz * nz;
  if (inner < 0.f) {
    // vng = n x d ; vref = vng x n
    const float gx = ny * dz - nz * dy, gy = nz * dx - nx * dz, gz = nx * dy - ny * dx;
    const float gnorm = __builtin_sqrtf(gx * gx + gy * gy + gz * gz);
    const float rx = gy * nz - gz * ny, ry = gz * nx - gx * nz, rz = gx * ny - gy * nx;
    const float rnorm = __builtin_sqrtf(rx * rx + ry * ry + rz * rz);
    // reference: diff_proj = diff * vref / (|vref| + 1e-9)   (elementwise product, kept as written)
    const float den = rnorm + 1e-9f;
    float px = dx * rx / den, py = dy * ry / den, pz = dz * rz / den;
    if (gnorm < 1e-6f) px = py = pz = 0.f;
    dx = px, dy = py, dz = pz;
  }
}

__device__ __forceinline__ void project_clip(float& dx, float& dy, float& dz, bool has_normal, float nx, float ny,
                                             float nz, float budget) {
  if (has_normal) project_inner(dx, dy, dz, nx, ny, nz);
  clip_linf(dx, dy, dz, budget);
}

// The best-attack decision of the CW-family loops for sample b (one thread): dist is the iterate's distance, pr / lb its
// prediction and label, bd / obd the values of bestdist[b] / o_bestdist[b] (the caller may have loaded them before its
// reduction: nothing writes them in between). Returns 1 when the iterate becomes the overall best.
__device__ __forceinline__ int cw_book_decide(float* dist_val, float* bestdist, int64_t* bestscore, float* o_bestdist,
                                              int64_t* o_bestscore, int untarget, int b, float dist, int64_t pr, int64_t lb,
                                              float bd, float obd) {
  if (dist_val) dist_val[b] = dist;
  const bool succ = untarget ? (pr != lb) : (pr == lb);
  if (succ && dist < bd) {
    bestdist[b] = dist;
    bestscore[b] = pr;
  }
  int copy = 0;
  if (succ && dist < obd) {
    o_bestdist[b] = dist;
    o_bestscore[b] = pr;
    copy = 1;
  }
  return copy;
}

}  // namespace pc3d
