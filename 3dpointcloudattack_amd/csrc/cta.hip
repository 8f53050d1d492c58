// The critical-point attack (attack/CTA/CTA.py and CTA_sumloss.py of the reference): integrated-gradients saliency of a
// set of clouds, then an optimiser loop that moves only the most salient points until the victim changes its mind.
// Five kernels; the victim's passes run between them (model/pointnet.py: fused_forward, fused_input_grad):
//   ig_steps       the baseline (minimum / maximum of the WHOLE batch tensor, or zero) and all steps x B interpolated
//                  clouds baseline + alpha_s * (x - baseline), one launch;
//   ig_cotangent   the cotangent VanillaGradient.get_mask puts on the log-softmax output, taken back to the logits:
//                  one-hot at the target class or the multi-hot of every row's top-1 class, rows >= set_size zero;
//   ig_reduce      sum over the steps in step order in double, times (x - baseline) / steps: the float64 mask [3,N,B]
//                  and both contribution tables (CTA.py: [3,B], summed over the points; CTA_sumloss.py: [B,N]);
//   cta_cotangent  the loop's loss forms as a cotangent on the logits, plus the records, the stop windows and the
//                  success flag of sample 0 of every set;
//   cta_update     gradient mask through the selection table, Adam (no bias correction, eps inside the root, step 1) or
//                  Momentum on the whole set, the step counters, the success latch; or, in control mode, the host's
//                  control words (advance the level and reset the iterate; latch).
// Per-set state lives in one int32 row poll[g, 0..63], which the host reads back in one copy every 25 steps:
//   0..24 the window of z[0][ori] (float bits)   25..49 the window of z[0][tar]   50 latch (1 success, 2 host)
//   51 cur_step   52 step   53 num_p_per   54 this step's success flag
// No atomics anywhere; every sum has one fixed order.
#include "pc3d_common.h"

namespace pc3d {

constexpr int CTA_KPL = 4;             // logits per lane: k <= 256
constexpr int CTA_POLL = 64;           // int32 words per set
constexpr int CTA_WIN = 25;            // the reference's stop window
constexpr int P_LATCH = 50, P_CUR = 51, P_STEP = 52, P_NPP = 53, P_SUCC = 54;

// arg-max of a row held lane-strided in v[] (entry j of lane l: class l + 64 j), the lowest index on a tie, classes in
// `skip` left out
__device__ __forceinline__ void cta_argmax(const float* v, int k, int lane, int skip, float& bv, int& bi) {
  bv = -__builtin_inff(), bi = 0x7fffffff;
#pragma unroll
  for (int j = 0; j < CTA_KPL; ++j) {
    const int c = lane + 64 * j;
    if (c < k && c != skip && (v[j] > bv || (v[j] == bv && c < bi))) bv = v[j], bi = c;
  }
  wave_argmax_first(bv, bi);
}

__device__ __forceinline__ void cta_load_row(const float* row, int k, int lane, float* v) {
#pragma unroll
  for (int j = 0; j < CTA_KPL; ++j) {
    const int c = lane + 64 * j;
    v[j] = c < k ? row[c] : -__builtin_inff();
  }
}

// softmax of the row as torch's log_softmax forward and backward form it: exp((z - max) - log(sum exp(z - max)))
__device__ __forceinline__ void cta_softmax(const float* v, int k, int lane, float m, float* p) {
  float e = 0.f;
#pragma unroll
  for (int j = 0; j < CTA_KPL; ++j)
    if (lane + 64 * j < k) e += __builtin_expf(v[j] - m);
  const float lse = __builtin_logf(wave_sum(e));
#pragma unroll
  for (int j = 0; j < CTA_KPL; ++j) p[j] = lane + 64 * j < k ? __builtin_expf((v[j] - m) - lse) : 0.f;
}

// ---------------------------------------------------------------------------------------------------------------------
struct IgStepsArgs {
  PtsView x;
  int B, N, S, kind;       // kind 0: minimum ('black'), 1: maximum ('white'), 2: zero
  const double* alpha;     // [S]
  float* out;              // [S*B,3,N]
  float* base;             // [1]
};

__global__ __launch_bounds__(1024) void ig_steps_kernel(IgStepsArgs a) {
  __shared__ float s_part[1024 / kWave];
  const int tid = threadIdx.x, T = blockDim.x, lane = tid & (kWave - 1), wave = tid / kWave;
  float base = 0.f;
  if (a.kind != 2) {
    // minimum / maximum of all B * 3 * N coordinates: exact whatever the order, which here is set by T alone
    const bool mn = a.kind == 0;
    float acc = mn ? __builtin_inff() : -__builtin_inff();
    const int64_t tot = (int64_t)a.B * 3 * a.N;
    for (int64_t i = tid; i < tot; i += T) {
      const int64_t b = i / (3 * a.N), r = i % (3 * a.N);
      const float val = a.x.p[b * a.x.bs + (r / a.N) * a.x.cs + (r % a.N) * a.x.ps];
      acc = mn ? fminf(acc, val) : fmaxf(acc, val);
    }
    acc = mn ? wave_min(acc) : wave_max(acc);
    if (lane == 0) s_part[wave] = acc;
    __syncthreads();
    base = s_part[0];
    for (int w = 1; w < T / kWave; ++w) base = mn ? fminf(base, s_part[w]) : fmaxf(base, s_part[w]);
  }
  const int s = blockIdx.x;
  if (s == 0 && blockIdx.y == 0 && tid == 0) a.base[0] = base;
  const float al = (float)a.alpha[s];      // torch multiplies a float tensor by a double scalar in float
  for (int b = blockIdx.y; b < a.B; b += gridDim.y) {
    float* ob = a.out + ((int64_t)s * a.B + b) * 3 * a.N;
    const float* xb = a.x.p + (int64_t)b * a.x.bs;
    for (int r = tid; r < 3 * a.N; r += T) {
      const float d = xb[(r / a.N) * a.x.cs + (r % a.N) * a.x.ps] - base;
      const float pr = al * d;             // rounded once, then added (the file is built with -ffp-contract=off)
      ob[r] = base + pr;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
struct IgCotArgs {
  const float* z;          // [R,k], row r = step * B + sample
  int R, B, k, set_size, target;   // target < 0: the multi-hot of every row's top-1 class
  float* g;                // [R,k]
};

__global__ __launch_bounds__(256) void ig_cotangent_kernel(IgCotArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  const int r = blockIdx.x * (256 / kWave) + threadIdx.x / kWave;
  if (r >= a.R) return;
  const int j = r % a.B, s0 = r - j;
  float* gr = a.g + (int64_t)r * a.k;
  if (j >= a.set_size) {
#pragma unroll
    for (int q = 0; q < CTA_KPL; ++q)
      if (lane + 64 * q < a.k) gr[lane + 64 * q] = 0.f;
    return;
  }
  float t[CTA_KPL] = {0.f, 0.f, 0.f, 0.f};
  if (a.target >= 0) {
#pragma unroll
    for (int q = 0; q < CTA_KPL; ++q) t[q] = lane + 64 * q == a.target ? 1.f : 0.f;
  } else {
    for (int i = 0; i < a.B; ++i) {      // target[j][logits.topk(1, dim=1)[1]] = 1: every row's class goes into row j
      float w[CTA_KPL], bv;
      int bi;
      cta_load_row(a.z + (int64_t)(s0 + i) * a.k, a.k, lane, w);
      cta_argmax(w, a.k, lane, -1, bv, bi);
#pragma unroll
      for (int q = 0; q < CTA_KPL; ++q)
        if (lane + 64 * q == bi) t[q] = 1.f;
    }
  }
  float tsum = 0.f;
#pragma unroll
  for (int q = 0; q < CTA_KPL; ++q) tsum += t[q];
  tsum = wave_sum(tsum);                 // small whole numbers: exact in any order
  float v[CTA_KPL], p[CTA_KPL], m;
  int mi;
  cta_load_row(a.z + (int64_t)r * a.k, a.k, lane, v);
  cta_argmax(v, a.k, lane, -1, m, mi);
  cta_softmax(v, a.k, lane, m, p);
#pragma unroll
  for (int q = 0; q < CTA_KPL; ++q)
    if (lane + 64 * q < a.k) gr[lane + 64 * q] = t[q] - p[q] * tsum;     // log_softmax backward: grad - exp(out) * sum(grad)
}

// ---------------------------------------------------------------------------------------------------------------------
struct IgReduceArgs {
  const float* g;          // [S*B,3,N]
  PtsView x;
  const float* base;       // [1]
  int S, B, N;
  double *mask, *contri_cn, *contri_bn;    // [3,N,B], [3,B], [B,N]
};

__global__ __launch_bounds__(256) void ig_reduce_kernel(IgReduceArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const float base = a.base[0];
  for (int n = tid; n < a.N; n += 256) {
    double m3[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double acc = 0.0;
      for (int s = 0; s < a.S; ++s) acc += (double)a.g[(((int64_t)s * a.B + b) * 3 + c) * a.N + n];
      const float d = a.x.p[(int64_t)b * a.x.bs + c * a.x.cs + (int64_t)n * a.x.ps] - base;
      m3[c] = acc * (double)d / (double)a.S;
      a.mask[((int64_t)c * a.N + n) * a.B + b] = m3[c];
    }
    a.contri_bn[(int64_t)b * a.N + n] = (m3[0] + m3[1]) + m3[2];
  }
  __syncthreads();                       // the block's own stores to mask are visible to it
  if (tid < 3) {
    double acc = 0.0;
    for (int n = 0; n < a.N; ++n) acc += a.mask[((int64_t)tid * a.N + n) * a.B + b];
    a.contri_cn[tid * a.B + b] = acc;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
struct CtaCotArgs {
  const float* z;          // [G*S,k]
  int G, S, k, mode;       // mode 0: ori - tar, 1: ori - second, 2: ori only, 3: log-softmax neuron
  int targeted, H;
  const int32_t *ori, *tar;        // [G]; tar may be null when nothing reads it
  const float* w;          // [S] per-sample weights (alpha folded in)
  int32_t* poll;           // [G,64]
  float *hist_ori, *hist_max;      // [G,H]
  float* g;                // [G*S,k]
  float* zlast;            // [G*S,k] or null: the logits of the last forward of every set that is not latched
};

__global__ __launch_bounds__(1024) void cta_cotangent_kernel(CtaCotArgs a) {
  const int gset = blockIdx.x, lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave, nw = blockDim.x / kWave;
  int32_t* pl = a.poll + (int64_t)gset * CTA_POLL;
  const int latch = pl[P_LATCH], cs = pl[P_CUR];   // this kernel stores neither word
  const int ori = a.ori[gset], tar = a.tar ? a.tar[gset] : -1;
  for (int j = wave; j < a.S; j += nw) {
    const int64_t r = (int64_t)gset * a.S + j;
    float* gr = a.g + r * a.k;
    float v[CTA_KPL], o[CTA_KPL] = {0.f, 0.f, 0.f, 0.f};
    cta_load_row(a.z + r * a.k, a.k, lane, v);
    float m, m2;
    int mi, mi2;
    cta_argmax(v, a.k, lane, -1, m, mi);
    const float wj = latch ? 0.f : a.w[j];
    if (a.mode == 3) {
      float p[CTA_KPL];
      cta_softmax(v, a.k, lane, m, p);
#pragma unroll
      for (int q = 0; q < CTA_KPL; ++q) o[q] = wj * ((lane + 64 * q == ori ? 1.f : 0.f) - p[q]);
    } else {
      int sub = -1;
      if (a.mode == 0) sub = tar;
      if (a.mode == 1) {                 // torch.topk(z, 2).indices[-1]: the runner-up by (value descending, class ascending)
        cta_argmax(v, a.k, lane, mi, m2, mi2);
        sub = mi2;
      }
#pragma unroll
      for (int q = 0; q < CTA_KPL; ++q) {
        const int c = lane + 64 * q;
        o[q] = (c == ori ? wj : 0.f) - (c == sub ? wj : 0.f);
      }
    }
#pragma unroll
    for (int q = 0; q < CTA_KPL; ++q)
      if (lane + 64 * q < a.k) gr[lane + 64 * q] = o[q];
    if (a.zlast && !latch) {
#pragma unroll
      for (int q = 0; q < CTA_KPL; ++q)
        if (lane + 64 * q < a.k) a.zlast[r * a.k + lane + 64 * q] = v[q];
    }
    if (j == 0 && !latch) {
      // the records of sample 0: z[ori], max of the row with z[ori] NEGATED (not left out), z[tar], the success test
      float zo = 0.f, zt = 0.f, mo = -__builtin_inff();
#pragma unroll
      for (int q = 0; q < CTA_KPL; ++q) {
        const int c = lane + 64 * q;
        if (c < a.k) {
          if (c == ori) zo = v[q];
          if (c == tar) zt = v[q];
          mo = fmaxf(mo, c == ori ? -v[q] : v[q]);
        }
      }
      zo = wave_sum(zo), zt = wave_sum(zt), mo = wave_max(mo);     // one lane holds the value, the others 0
      if (lane == 0) {
        if (cs >= 0 && cs < a.H) a.hist_ori[(int64_t)gset * a.H + cs] = zo, a.hist_max[(int64_t)gset * a.H + cs] = mo;
        const int wpos = (cs >= 0 ? cs : 0) % CTA_WIN;
        pl[wpos] = __builtin_bit_cast(int32_t, zo);
        pl[CTA_WIN + wpos] = __builtin_bit_cast(int32_t, zt);
        pl[P_SUCC] = a.targeted ? (mi == tar ? 1 : 0) : (mi != ori ? 1 : 0);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
struct CtaUpdateArgs {
  float* x;                // [G*S,3,N] the iterate
  const float *g, *proto;  // [G*S,3,N]
  float *v, *s;            // optimiser state; s null for Momentum
  const int32_t* sel;      // [G,P,W] flat slots sample * N + point per level; anything outside [0, S*N) is padding
  int P, W, cap;
  int32_t *poll, *ctrl;    // [G,64]; [G] host-written: 1 advance, 2 latch
  int G, S, N, opt, control;
  float c1, c1m, c2, c2m, xi;
};

__global__ __launch_bounds__(1024) void cta_update_kernel(CtaUpdateArgs a) {
  extern __shared__ unsigned char cta_flag[];      // [S*N]: the slot is unmasked
  const int gset = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
  int32_t* pl = a.poll + (int64_t)gset * CTA_POLL;
  const int latch = pl[P_LATCH], cs = pl[P_CUR], st = pl[P_STEP], npp = pl[P_NPP], succ = pl[P_SUCC];
  const int cw = a.ctrl ? a.ctrl[gset] : 0;
  __syncthreads();                                 // every thread has read the state words: thread 0 may store
  const int64_t E = (int64_t)a.S * 3 * a.N, off = (int64_t)gset * E;
  if (a.control) {
    if (latch || cw == 0) return;
    if (cw == 1) {                                 // next level: the iterate back to the prototype, the optimiser state kept
      for (int64_t i = tid; i < E; i += T) a.x[off + i] = a.proto[off + i];
      if (tid == 0) pl[P_NPP] = npp + 1, pl[P_CUR] = 0;
    } else if (tid == 0) {
      pl[P_LATCH] = 2;
    }
    if (tid == 0) a.ctrl[gset] = 0;
    return;
  }
  if (latch) return;
  const int SN = a.S * a.N;
  int L = npp < a.cap ? npp : a.cap;
  L = L < a.P ? L : a.P;
  for (int i = tid; i < SN; i += T) cta_flag[i] = 0;
  __syncthreads();
  const int32_t* sl = a.sel + (int64_t)gset * a.P * a.W;
  for (int e = tid; e < L * a.W; e += T) {
    const int slot = sl[e];
    if ((unsigned)slot < (unsigned)SN) cta_flag[slot] = 1;       // several threads may store the same 1
  }
  __syncthreads();
  for (int64_t i = tid; i < E; i += T) {
    const int j = (int)(i / (3 * a.N)), n = (int)(i % a.N);
    const float gm = cta_flag[j * a.N + n] ? a.g[off + i] : 0.f;
    const float xo = a.x[off + i];
    if (a.opt == 0) {
      const float vn = a.c1 * a.v[off + i] + a.c1m * gm;
      const float sn = a.c2 * a.s[off + i] + a.c2m * (gm * gm);
      a.v[off + i] = vn, a.s[off + i] = sn;
      a.x[off + i] = xo + (-vn) / __fsqrt_rn(sn + a.xi);
    } else {
      const float vn = a.c1 * a.v[off + i] - gm;
      a.v[off + i] = vn;
      a.x[off + i] = xo + vn;
    }
  }
  if (tid == 0) {
    pl[P_CUR] = cs + 1, pl[P_STEP] = st + 1;
    if (succ) pl[P_LATCH] = 1;                     // success on this step's forward: frozen after this step's update
  }
}

}  // namespace pc3d

using namespace pc3d;

extern "C" int pc3d_ig_steps_f32(const float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs, int B, int N, int kind,
                                 const double* alpha, int S, float* out, float* base, void* stream) {
  PC3D_REQUIRE(B >= 1 && N >= 1 && S >= 1, "pc3d_ig_steps_f32: bad sizes B=%d N=%d S=%d", B, N, S);
  PC3D_REQUIRE(kind >= 0 && kind <= 2, "pc3d_ig_steps_f32: kind must be 0 (min), 1 (max) or 2 (zero), got %d", kind);
  PC3D_REQUIRE((int64_t)S * B <= 0x7fffffff / 3 / (int64_t)N, "pc3d_ig_steps_f32: S*B*3*N too large");
  PC3D_REQUIRE(x && alpha && out && base, "pc3d_ig_steps_f32: null pointer");
  PC3D_REQUIRE(out != x, "pc3d_ig_steps_f32: out must not alias x");
  IgStepsArgs a{{x, x_bs, x_ps, x_cs}, B, N, S, kind, alpha, out, base};
  hipLaunchKernelGGL(ig_steps_kernel, dim3((unsigned)S, (unsigned)(B < 8 ? B : 8)), dim3(1024), 0, as_stream(stream), a);
  PC3D_LAUNCH_CHECK("pc3d_ig_steps_f32");
  return PC3D_OK;
}

extern "C" int pc3d_ig_cotangent_f32(const float* z, int R, int B, int k, int set_size, int target, float* g, void* stream) {
  PC3D_REQUIRE(R >= 1 && B >= 1 && R % B == 0, "pc3d_ig_cotangent_f32: R=%d rows must be whole steps of B=%d", R, B);
  PC3D_REQUIRE(k >= 1 && k <= 64 * CTA_KPL, "pc3d_ig_cotangent_f32: k=%d classes, need 1 <= k <= %d", k, 64 * CTA_KPL);
  PC3D_REQUIRE(set_size >= 0 && target < k, "pc3d_ig_cotangent_f32: bad set_size=%d or target=%d", set_size, target);
  PC3D_REQUIRE(z && g && z != g, "pc3d_ig_cotangent_f32: null or aliased pointer");
  IgCotArgs a{z, R, B, k, set_size, target, g};
  hipLaunchKernelGGL(ig_cotangent_kernel, dim3((unsigned)cdiv(R, 256 / kWave)), dim3(256), 0, as_stream(stream), a);
  PC3D_LAUNCH_CHECK("pc3d_ig_cotangent_f32");
  return PC3D_OK;
}

extern "C" int pc3d_ig_reduce_f64(const float* g, int S, int B, int N, const float* x, int64_t x_bs, int64_t x_ps,
                                  int64_t x_cs, const float* base, double* mask, double* contri_cn, double* contri_bn,
                                  void* stream) {
  PC3D_REQUIRE(B >= 1 && N >= 1 && S >= 1, "pc3d_ig_reduce_f64: bad sizes B=%d N=%d S=%d", B, N, S);
  PC3D_REQUIRE(g && x && base && mask && contri_cn && contri_bn, "pc3d_ig_reduce_f64: null pointer");
  IgReduceArgs a{g, {x, x_bs, x_ps, x_cs}, base, S, B, N, mask, contri_cn, contri_bn};
  hipLaunchKernelGGL(ig_reduce_kernel, dim3((unsigned)B), dim3(256), 0, as_stream(stream), a);
  PC3D_LAUNCH_CHECK("pc3d_ig_reduce_f64");
  return PC3D_OK;
}

extern "C" int pc3d_cta_cotangent_f32(const float* z, int G, int S, int k, int mode, int targeted, const int32_t* ori,
                                      const int32_t* tar, const float* w, int32_t* poll, float* hist_ori, float* hist_max,
                                      int H, float* g, float* zlast, void* stream) {
  PC3D_REQUIRE(G >= 0 && S >= 1 && H >= 1, "pc3d_cta_cotangent_f32: bad sizes G=%d S=%d H=%d", G, S, H);
  PC3D_REQUIRE(k >= 2 && k <= 64 * CTA_KPL, "pc3d_cta_cotangent_f32: k=%d classes, need 2 <= k <= %d", k, 64 * CTA_KPL);
  PC3D_REQUIRE(mode >= 0 && mode <= 3, "pc3d_cta_cotangent_f32: mode must be 0..3, got %d", mode);
  if (G == 0) return PC3D_OK;
  PC3D_REQUIRE(z && ori && w && poll && hist_ori && hist_max && g && z != g && z != zlast && g != zlast,
               "pc3d_cta_cotangent_f32: null or aliased pointer");
  PC3D_REQUIRE(tar || (mode != 0 && !targeted), "pc3d_cta_cotangent_f32: a targeted loss needs tar");
  CtaCotArgs a{z, G, S, k, mode, targeted ? 1 : 0, H, ori, tar, w, poll, hist_ori, hist_max, g, zlast};
  const int T = (S < 16 ? S : 16) * kWave;
  hipLaunchKernelGGL(cta_cotangent_kernel, dim3((unsigned)G), dim3(T), 0, as_stream(stream), a);
  PC3D_LAUNCH_CHECK("pc3d_cta_cotangent_f32");
  return PC3D_OK;
}

extern "C" int pc3d_cta_update_f32(float* x, const float* g, const float* proto, float* v, float* s, const int32_t* sel,
                                   int P, int W, int cap, int32_t* poll, int32_t* ctrl, int G, int S, int N, int opt,
                                   int control, double b1, double b2, double xi, void* stream) {
  PC3D_REQUIRE(G >= 0 && S >= 1 && N >= 1, "pc3d_cta_update_f32: bad sizes G=%d S=%d N=%d", G, S, N);
  PC3D_REQUIRE((int64_t)S * N <= 49152, "pc3d_cta_update_f32: S*N=%lld exceeds the limit of 49152 slots (flags in LDS)",
               (long long)S * N);
  PC3D_REQUIRE(opt == 0 || opt == 1, "pc3d_cta_update_f32: opt must be 0 (Adam) or 1 (Momentum), got %d", opt);
  if (G == 0) return PC3D_OK;
  PC3D_REQUIRE(x && proto && poll && x != proto, "pc3d_cta_update_f32: null or aliased pointer");
  if (control) {
    PC3D_REQUIRE(ctrl, "pc3d_cta_update_f32: the control mode needs ctrl");
  } else {
    PC3D_REQUIRE(P >= 1 && W >= 1 && cap >= 0 && (int64_t)P * W <= 0x7fffffff, "pc3d_cta_update_f32: bad table P=%d W=%d cap=%d", P, W, cap);
    PC3D_REQUIRE(g && v && sel && (opt == 1 || s), "pc3d_cta_update_f32: null pointer");
    PC3D_REQUIRE(x != g && x != v && x != s && v != s && v != g, "pc3d_cta_update_f32: x, g, v and s must not alias");
  }
  // the constants as torch forms them: python doubles 0.9, 1 - 0.9, ... rounded to float when they meet a float tensor
  CtaUpdateArgs a{x, g, proto, v, s, sel, P, W, cap, poll, ctrl, G, S, N, opt, control ? 1 : 0,
                  (float)b1, (float)(1.0 - b1), (float)b2, (float)(1.0 - b2), (float)xi};
  const int64_t work = (int64_t)S * N;
  const int T = work >= 1024 ? 1024 : cdiv((int)work, kWave) * kWave;
  const size_t lds = control ? 0 : (size_t)((S * N + 3) / 4 * 4);
  hipLaunchKernelGGL(cta_update_kernel, dim3((unsigned)G), dim3(T), lds, as_stream(stream), a);
  PC3D_LAUNCH_CHECK("pc3d_cta_update_f32");
  return PC3D_OK;
}
