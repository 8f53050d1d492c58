// K12c — the untargeted AOF iteration's own launches (attack/AOF/Eval_AOF.py:162-199), beside the victim pass and the
// spectral re-projection of spectral.hip:
//   * aof_record_kernel: the bookkeeping of :168-185 on the iterate that was just evaluated — dist = max |adv - data| over
//     the whole cloud, the three-way decision, the conditional copy into o_bestattack. One workgroup per cloud.
//   * aof_update_kernel: :187-195 between the backward and the re-projection — g = g1 + g2, torch's Adam on lfc, adv =
//     lfc + hfc, ClipPointsLinf against data. One thread per point; adam_element and clip_linf (update_body.h) are what
//     adam_clip_kernel and clip_kernel call, so the launch gives the bits of pc3d_adam_clip_step_f32 + torch.add + pc3d_clip_f32.
// Every tensor is a contiguous [B,3,N] block given by its own pointer: the loop keeps (lfc + hfc | lfc) and the two
// gradient terms as the halves of [2B,3,N] buffers of the victim's stacked pass.
#include "update_body.h"

namespace pc3d {

struct AofRecordArgs {
  const float* adv;        // [B,3,N]
  const float* data;       // [B,3,N]
  int N;
  const int64_t* pred;     // [B]
  const int64_t* lfc_pred; // [B]
  const int64_t* label;    // [B]
  float* o_bestdist;       // [B]
  int64_t* o_bestscore;    // [B]
  float* o_bestattack;     // [B,3,N]
  float* dist_val;         // [B] or null
  int32_t* step;           // Adam step word, incremented once per launch (may be null)
};

constexpr int kAofRecordThreads = 256;

__global__ __launch_bounds__(kAofRecordThreads) void aof_record_kernel(AofRecordArgs a) {
  __shared__ float s_max[kAofRecordThreads / 64];
  __shared__ int s_nan[kAofRecordThreads / 64];
  __shared__ int s_copy;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n3 = 3 * a.N;
  const float* adv = a.adv + (int64_t)b * n3;
  const float* dat = a.data + (int64_t)b * n3;
  // pass 1: a maximum does not depend on the order. fmaxf drops a NaN operand, torch.amax (and numpy's `nan < x`)
  // does not: a NaN is carried beside the maximum as a flag.
  float mx = 0.f;
  int bad = 0;
  for (int i = tid; i < n3; i += kAofRecordThreads) {
    const float d = fabsf(adv[i] - dat[i]);
    if (d != d) bad = 1;
    else mx = fmaxf(mx, d);
  }
  mx = wave_max(mx);
  bad = __any(bad);
  if ((tid & 63) == 0) s_max[tid >> 6] = mx, s_nan[tid >> 6] = bad;
  __syncthreads();
  if (tid == 0) {
    float dist = s_max[0];
    int nan = s_nan[0];
#pragma unroll
    for (int w = 1; w < kAofRecordThreads / 64; ++w) dist = fmaxf(dist, s_max[w]), nan |= s_nan[w];
    if (nan) dist = __builtin_nanf("");
    if (a.dist_val) a.dist_val[b] = dist;
    const int64_t pr = a.pred[b], lp = a.lfc_pred[b], lb = a.label[b];
    int copy = 0;
    if (pr != lb && dist < a.o_bestdist[b] && lp != lb) {     // NaN < x is false: no update
      a.o_bestdist[b] = dist;
      a.o_bestscore[b] = pr;
      copy = 1;
    }
    s_copy = copy;
    if (a.step && b == 0) a.step[0] += 1;
  }
  __syncthreads();
  if (s_copy == 0) return;
  // pass 2
  float* dst = a.o_bestattack + (int64_t)b * n3;
  for (int i = tid; i < n3; i += kAofRecordThreads) dst[i] = adv[i];
}

struct AofUpdateArgs {
  float* lfc;              // [B,3,N] the optimised band, updated in place
  const float* g1;         // [B,3,N] d loss / d(lfc + hfc)
  const float* g2;         // [B,3,N] d loss / d lfc
  float* m;                // [B,3,N] exp_avg
  float* v;                // [B,3,N] exp_avg_sq
  const float* hfc;        // [B,3,N]
  const float* data;       // [B,3,N] the cloud the clip is taken against
  float* out;              // [B,3,N] clip(lfc_new + hfc, data)
  int N;
  double lr, b1, b2;
  float eps, budget;
  const int32_t* step_dev; // device step number t (>= 1); null -> step_host
  int step_host;
};

__global__ __launch_bounds__(256) void aof_update_kernel(AofUpdateArgs a) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  if (k >= a.N) return;
  const int t = a.step_dev ? a.step_dev[0] : a.step_host;
  const AdamConsts ad = adam_consts(a.lr, a.b1, a.b2, a.eps, t);
  const int64_t base = (int64_t)b * 3 * a.N + k;
  float np_[3], o[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int64_t i = base + (int64_t)c * a.N;
    float g = a.g1[i];
    g += a.g2[i];
    float m = a.m[i], v = a.v[i];
    const float p = adam_element(ad, a.lfc[i], g, m, v);
    a.m[i] = m;
    a.v[i] = v;
    a.lfc[i] = p;
    np_[c] = p + a.hfc[i];
    o[c] = a.data[i];
  }
  float dx = np_[0] - o[0], dy = np_[1] - o[1], dz = np_[2] - o[2];
  clip_linf(dx, dy, dz, a.budget);
  a.out[base] = o[0] + dx;
  a.out[base + a.N] = o[1] + dy;
  a.out[base + 2 * (int64_t)a.N] = o[2] + dz;
}

}  // namespace pc3d

using namespace pc3d;

extern "C" int pc3d_aof_record_f32(const float* adv, const float* data, int B, int N, const int64_t* pred, const int64_t* lfc_pred,
                                   const int64_t* label, float* o_bestdist, int64_t* o_bestscore, float* o_bestattack,
                                   float* dist_val, int32_t* step, void* stream) {
  PC3D_REQUIRE(B >= 0 && N >= 1 && N <= (1 << 28), "pc3d_aof_record_f32: bad sizes B=%d N=%d", B, N);
  if (B == 0) return PC3D_OK;
  PC3D_REQUIRE(adv && data && pred && lfc_pred && label && o_bestdist && o_bestscore && o_bestattack,
               "pc3d_aof_record_f32: null pointer");
  AofRecordArgs a{adv, data, N, pred, lfc_pred, label, o_bestdist, o_bestscore, o_bestattack, dist_val, step};
  hipLaunchKernelGGL(aof_record_kernel, dim3(B), dim3(kAofRecordThreads), 0, as_stream(stream), a);
  PC3D_LAUNCH_CHECK("pc3d_aof_record_f32");
  return PC3D_OK;
}

extern "C" int pc3d_aof_update_f32(float* lfc, const float* g1, const float* g2, float* m, float* v, const float* hfc,
                                   const float* data, float* out, int B, int N, double lr, double beta1, double beta2, double eps,
                                   float budget, const int32_t* step_dev, int step_host, void* stream) {
  PC3D_REQUIRE(B >= 0 && N >= 1 && B <= 65535 && N <= (1 << 28), "pc3d_aof_update_f32: bad sizes B=%d N=%d", B, N);
  PC3D_REQUIRE(step_dev != nullptr || step_host >= 1, "pc3d_aof_update_f32: step_host must be >= 1 without a device counter");
  if (B == 0) return PC3D_OK;
  PC3D_REQUIRE(lfc && g1 && g2 && m && v && hfc && data && out, "pc3d_aof_update_f32: null pointer");
  AofUpdateArgs a{lfc, g1, g2, m, v, hfc, data, out, N, lr, beta1, beta2, (float)eps, budget, step_dev, step_host};
  hipLaunchKernelGGL(aof_update_kernel, dim3(cdiv(N, 256), B), dim3(256), 0, as_stream(stream), a);
  PC3D_LAUNCH_CHECK("pc3d_aof_update_f32");
  return PC3D_OK;
}
