// The isometry attack (attack/ISO/iso_attack.py of the reference): x' = W x with one 3x3 matrix per cloud, optimised by
// Adam through a frozen victim. Three kernels, fp32:
//   iso_apply   out[b R + r] = W[b R + r] x[b] (or W^T: the input-gradient direction), the cloud read once for its R matrices;
//   iso_wgrad   gW[i] = g[i] x[i / R]^T, one workgroup per matrix, fixed summation order (iso_body.h);
//   iso_update  everything of one CTRI step that is not the victim, per cloud and in one launch: the early-stop latch,
//               the record of the evaluation, the weight gradient, Adam on the 9 parameters and the next iterate W x.
// The clouds are tiny (12 KB at N = 1024): what counts is that a step adds one launch and no host round trip.
#include "iso_body.h"
#include "update_body.h"

namespace pc3d {

struct IsoApplyArgs {
  PtsView x;
  const float* W;
  PtsViewMut out;
  int R, N, transpose;
};

__global__ __launch_bounds__(ISO_T) void iso_apply_kernel(IsoApplyArgs a) {
  const int n = blockIdx.x * ISO_T + threadIdx.x, b = blockIdx.y;
  if (n >= a.N) return;
  const float* xp = a.x.p + (int64_t)b * a.x.bs + (int64_t)n * a.x.ps;
  const float x0 = xp[0], x1 = xp[a.x.cs], x2 = xp[2 * a.x.cs];
  for (int r = 0; r < a.R; ++r) {
    const int64_t i = (int64_t)b * a.R + r;
    float y[3];
    iso_mat3(a.W + i * 9, a.transpose, x0, x1, x2, y);
    float* op = a.out.p + i * a.out.bs + (int64_t)n * a.out.ps;
    op[0] = y[0];
    op[a.out.cs] = y[1];
    op[2 * a.out.cs] = y[2];
  }
}

struct IsoWgradArgs {
  PtsView g, x;
  float* gW;
  int R, N;
};

__global__ __launch_bounds__(ISO_T) void iso_wgrad_kernel(IsoWgradArgs a) {
  __shared__ float s_part[ISO_WAVES][9];
  __shared__ float s_gw[9];
  const int64_t i = blockIdx.x;
  iso_wgrad_block(a.g.p + i * a.g.bs, a.g.ps, a.g.cs, a.x.p + (i / a.R) * a.x.bs, a.x.ps, a.x.cs, a.N, s_part, s_gw);
  if (threadIdx.x < 9) a.gW[i * 9 + threadIdx.x] = s_gw[threadIdx.x];
}

struct IsoUpdateArgs {
  PtsView x, g;            // the clean cloud; dL/dx' of this evaluation (p null: gW_in holds the weight gradient)
  const float* gW_in;      // [B,9] or null
  PtsViewMut xo;           // the victim's input buffer: receives W x
  int N, ncls;
  const int64_t *pred, *label;
  const float* row;        // this evaluation's output rows [B, ncls], row stride row_ld
  int64_t row_ld;
  int32_t *done, *steps;
  float* kept_out;
  int64_t* kept_pred;
  float *W, *m, *v;        // [B,9]
  double lr, b1, b2;
  float eps;
};

__global__ __launch_bounds__(ISO_T) void iso_update_kernel(IsoUpdateArgs a) {
  __shared__ float s_part[ISO_WAVES][9];
  __shared__ float s_gw[9];
  __shared__ float s_w[9];
  __shared__ int s_state[3];     // done on entry, done after the latch, the step number t of this evaluation
  const int b = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) {
    const int d0 = a.done[b] != 0;
    s_state[0] = d0;
    s_state[1] = (d0 || a.pred[b] != a.label[b]) ? 1 : 0;
    s_state[2] = a.steps[b] + 1;
  }
  __syncthreads();
  const int d0 = s_state[0], d1 = s_state[1], t = s_state[2];
  if (!d0) {                                        // record: the evaluation a stopping cloud reports is this one
    for (int j = tid; j < a.ncls; j += ISO_T) a.kept_out[(int64_t)b * a.ncls + j] = a.row[(int64_t)b * a.row_ld + j];
    if (tid == 0) {
      a.steps[b] = t;
      a.kept_pred[b] = a.pred[b];
      a.done[b] = d1;
    }
  }
  if (!d1) {                                        // workgroup-uniform: the barriers inside are reached by all threads
    if (a.g.p)
      iso_wgrad_block(a.g.p + (int64_t)b * a.g.bs, a.g.ps, a.g.cs, a.x.p + (int64_t)b * a.x.bs, a.x.ps, a.x.cs, a.N, s_part, s_gw);
    if (tid < 9) {
      const AdamConsts ad = adam_consts(a.lr, a.b1, a.b2, a.eps, t);
      const int64_t k = (int64_t)b * 9 + tid;
      const float g = a.g.p ? s_gw[tid] : a.gW_in[k];
      float m = a.m[k], v = a.v[k];
      const float denom = adam_moments(ad, g, m, v);
      a.m[k] = m;
      a.v[k] = v;
      // this loop's own last line: (-step_size * m) / denom rounds differently from adam_element's step_size * (m / denom)
      const float w = a.W[k] + (-ad.step_size * m) / denom;
      a.W[k] = w;
      s_w[tid] = w;
    }
  } else if (tid < 9) {
    s_w[tid] = a.W[(int64_t)b * 9 + tid];
  }
  __syncthreads();
  const float* xb = a.x.p + (int64_t)b * a.x.bs;
  float* ob = a.xo.p + (int64_t)b * a.xo.bs;
  for (int n = tid; n < a.N; n += ISO_T) {
    const float* xp = xb + (int64_t)n * a.x.ps;
    float y[3];
    iso_mat3(s_w, 0, xp[0], xp[a.x.cs], xp[2 * a.x.cs], y);
    float* op = ob + (int64_t)n * a.xo.ps;
    op[0] = y[0];
    op[a.xo.cs] = y[1];
    op[2 * a.xo.cs] = y[2];
  }
}

}  // namespace pc3d

using namespace pc3d;

extern "C" int pc3d_iso_apply_f32(const float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs, const float* W, int B, int R, int N,
                                  int transpose, float* out, int64_t o_bs, int64_t o_ps, int64_t o_cs, void* stream) {
  PC3D_REQUIRE(B >= 0 && B <= 65535 && R >= 1 && N >= 1, "pc3d_iso_apply_f32: bad sizes B=%d R=%d N=%d (B <= 65535)", B, R, N);
  if (B == 0) return PC3D_OK;
  PC3D_REQUIRE(x && W && out, "pc3d_iso_apply_f32: null pointer");
  PC3D_REQUIRE(x != out, "pc3d_iso_apply_f32: out must not alias x (x is read once for R outputs)");
  IsoApplyArgs a{{x, x_bs, x_ps, x_cs}, W, {out, o_bs, o_ps, o_cs}, R, N, transpose ? 1 : 0};
  hipLaunchKernelGGL(iso_apply_kernel, dim3(cdiv(N, ISO_T), B), dim3(ISO_T), 0, as_stream(stream), a);
  PC3D_LAUNCH_CHECK("pc3d_iso_apply_f32");
  return PC3D_OK;
}

extern "C" int pc3d_iso_wgrad_f32(const float* g, int64_t g_bs, int64_t g_ps, int64_t g_cs,
                                  const float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs, int B, int R, int N, float* gW,
                                  void* stream) {
  PC3D_REQUIRE(B >= 0 && R >= 1 && N >= 1 && (int64_t)B * R <= 0x7fffffffLL, "pc3d_iso_wgrad_f32: bad sizes B=%d R=%d N=%d", B, R, N);
  if (B == 0) return PC3D_OK;
  PC3D_REQUIRE(g && x && gW, "pc3d_iso_wgrad_f32: null pointer");
  IsoWgradArgs a{{g, g_bs, g_ps, g_cs}, {x, x_bs, x_ps, x_cs}, gW, R, N};
  hipLaunchKernelGGL(iso_wgrad_kernel, dim3((unsigned)(B * R)), dim3(ISO_T), 0, as_stream(stream), a);
  PC3D_LAUNCH_CHECK("pc3d_iso_wgrad_f32");
  return PC3D_OK;
}

extern "C" int pc3d_iso_update_f32(const float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs,
                                   const float* g, int64_t g_bs, int64_t g_ps, int64_t g_cs, const float* gW_in,
                                   int B, int N, const int64_t* pred, const int64_t* label, const float* row, int64_t row_ld,
                                   int ncls, int32_t* done, int32_t* steps, float* kept_out, int64_t* kept_pred,
                                   float* W, float* m, float* v, double lr, double beta1, double beta2, double eps,
                                   float* xo, int64_t xo_bs, int64_t xo_ps, int64_t xo_cs, void* stream) {
  PC3D_REQUIRE(B >= 0 && N >= 1 && ncls >= 1 && row_ld >= ncls, "pc3d_iso_update_f32: bad sizes B=%d N=%d ncls=%d row_ld=%lld", B, N,
               ncls, (long long)row_ld);
  PC3D_REQUIRE((g != nullptr) != (gW_in != nullptr), "pc3d_iso_update_f32: give either the point gradient g or the weight gradient gW_in");
  if (B == 0) return PC3D_OK;
  PC3D_REQUIRE(x && pred && label && row && done && steps && kept_out && kept_pred && W && m && v && xo,
               "pc3d_iso_update_f32: null pointer");
  PC3D_REQUIRE(xo != x && xo != g, "pc3d_iso_update_f32: the iterate buffer xo must not alias x or g");
  IsoUpdateArgs a{{x, x_bs, x_ps, x_cs}, {g, g_bs, g_ps, g_cs}, gW_in, {xo, xo_bs, xo_ps, xo_cs}, N, ncls, pred, label, row, row_ld,
                  done, steps, kept_out, kept_pred, W, m, v, lr, beta1, beta2, (float)eps};
  hipLaunchKernelGGL(iso_update_kernel, dim3((unsigned)B), dim3(ISO_T), 0, as_stream(stream), a);
  PC3D_LAUNCH_CHECK("pc3d_iso_update_f32");
  return PC3D_OK;
}
