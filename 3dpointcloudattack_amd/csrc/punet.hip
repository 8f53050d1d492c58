// PU-Net in front of a victim (attack/SIadv/baselines/defense/DUP_Net/ of the reference): the two pieces of the upsampler
// that the classifiers' kernels do not cover.
//
//   three_interp      3-NN inverse-distance interpolation of a feature-propagation level (pu_modules.py:161-168) from the
//                     search's (distance, index) lists: w_j = 1 / (d_j + 1e-8), normalised; output written at a column offset
//                     of a wider row buffer, bias + ReLU in the epilogue (the level's 1x1 convolution runs BEFORE it on the
//                     known rows: the weights sum to one)
//   three_interp_bwd  two launches, no atomics: per unknown point the three products <g, F[idx_j]> (16 lanes per point,
//                     butterfly sum), the weight / distance / coordinate gradients and one record per (point, j); then per
//                     known row a gather through the sorted reverse index of idx, ascending
//   pcd_tail          relu(W3 h + b3) (128 -> 64, fp32 MFMA) and the 64 -> 3 coordinate head in one launch, the output in
//                     the reference's [B, branch * N + n, 3] order; the ReLU's sign as two words per row for the backward
//   pcd_tail_bwd      g3 = sign * (W4^T g) generated on load, times W3 (64 -> 128, fp32 MFMA)
#include "pc3d_common.h"

namespace pc3d {
namespace {

typedef float floatx16 __attribute__((ext_vector_type(16)));

constexpr float kInterpEps = 1e-8f;

__device__ __forceinline__ void interp_weights(const float* __restrict__ d, float* w, float* r, float& s) {
  r[0] = 1.0f / (d[0] + kInterpEps);
  r[1] = 1.0f / (d[1] + kInterpEps);
  r[2] = 1.0f / (d[2] + kInterpEps);
  s = (r[0] + r[1]) + r[2];
  w[0] = r[0] / s, w[1] = r[1] / s, w[2] = r[2] / s;
}

__device__ __forceinline__ int clamp_row(int i, int M) { return (unsigned)i < (unsigned)M ? i : 0; }

struct InterpArgs {
  const float* d;        // [B,N,3]
  const int32_t* idx;    // [B,N,3]
  const float* F;        // [B,M,ldf]
  int64_t ldf;
  int N, M, C;
  float* out;            // [B,N,ldo], already at the column offset
  int64_t ldo;
  const float* bias;     // [C] or null
  int relu, vec_out;
};

// one thread per (point, four channels)
__global__ __launch_bounds__(256) void three_interp_kernel(InterpArgs a) {
  const int b = blockIdx.y, C4 = a.C >> 2;
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int n = t / C4, c = (t - n * C4) * 4;
  if (n >= a.N) return;
  const int64_t row = (int64_t)b * a.N + n;
  float w[3], r[3], s;
  interp_weights(a.d + row * 3, w, r, s);
  const float* Fb = a.F + (int64_t)b * a.M * a.ldf + c;
  const float4 f0 = *reinterpret_cast<const float4*>(Fb + (int64_t)clamp_row(a.idx[row * 3 + 0], a.M) * a.ldf);
  const float4 f1 = *reinterpret_cast<const float4*>(Fb + (int64_t)clamp_row(a.idx[row * 3 + 1], a.M) * a.ldf);
  const float4 f2 = *reinterpret_cast<const float4*>(Fb + (int64_t)clamp_row(a.idx[row * 3 + 2], a.M) * a.ldf);
  float4 v;
  v.x = (w[0] * f0.x + w[1] * f1.x) + w[2] * f2.x;
  v.y = (w[0] * f0.y + w[1] * f1.y) + w[2] * f2.y;
  v.z = (w[0] * f0.z + w[1] * f1.z) + w[2] * f2.z;
  v.w = (w[0] * f0.w + w[1] * f1.w) + w[2] * f2.w;
  if (a.bias) {
    const float4 bb = *reinterpret_cast<const float4*>(a.bias + c);
    v.x += bb.x, v.y += bb.y, v.z += bb.z, v.w += bb.w;
  }
  if (a.relu) v.x = fmaxf(v.x, 0.f), v.y = fmaxf(v.y, 0.f), v.z = fmaxf(v.z, 0.f), v.w = fmaxf(v.w, 0.f);
  float* o = a.out + row * a.ldo + c;
  if (a.vec_out) {
    *reinterpret_cast<float4*>(o) = v;
  } else {              // a column offset that is not a multiple of four (3 + 64 l in the concatenation)
    o[0] = v.x, o[1] = v.y, o[2] = v.z, o[3] = v.w;
  }
}

struct InterpBwdArgs {
  PtsView u, k;          // unknown [B,N], known [B,M]
  const float* d;
  const int32_t* idx;
  const float* F;
  int64_t ldf;
  const float* g;        // [B,N,ldg] upstream gradient at the column offset
  int64_t ldg;
  const float* y;        // [B,N,ldy] the forward's output at the column offset (ReLU mask) or null
  int64_t ldy;
  int N, M, C;
  float* wrec;           // [B,N,3]   the weights
  float* krec;           // [B,N,3,3] the gradient every (point, j) sends to the coordinates of known row idx_j
  float* gu;             // [B,N,3]
};

// the upstream gradient of four channels behind the ReLU (scalar loads: the column offset need not be a multiple of four)
__device__ __forceinline__ float4 masked_g(const float* __restrict__ g, const float* __restrict__ y) {
  float4 v = make_float4(g[0], g[1], g[2], g[3]);
  if (y) {
    v.x = y[0] > 0.f ? v.x : 0.f, v.y = y[1] > 0.f ? v.y : 0.f;
    v.z = y[2] > 0.f ? v.z : 0.f, v.w = y[3] > 0.f ? v.w : 0.f;
  }
  return v;
}

// 16 lanes per unknown point, 16 points per workgroup
__global__ __launch_bounds__(256) void three_interp_bwd_points_kernel(InterpBwdArgs a) {
  const int b = blockIdx.y, l = threadIdx.x & 15;
  const int n0 = blockIdx.x * 16 + (threadIdx.x >> 4);
  const bool valid = n0 < a.N;
  const int n = valid ? n0 : a.N - 1;
  const int64_t row = (int64_t)b * a.N + n;
  int id[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) id[j] = clamp_row(a.idx[row * 3 + j], a.M);
  const float* Fb = a.F + (int64_t)b * a.M * a.ldf;
  const float* gp = a.g + row * a.ldg;
  const float* yp = a.y ? a.y + row * a.ldy : nullptr;
  float acc[3] = {0.f, 0.f, 0.f};
  for (int c = l * 4; c < a.C; c += 64) {
    const float4 gv = masked_g(gp + c, yp ? yp + c : nullptr);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float4 f = *reinterpret_cast<const float4*>(Fb + (int64_t)id[j] * a.ldf + c);
      acc[j] += ((gv.x * f.x + gv.y * f.y) + gv.z * f.z) + gv.w * f.w;
    }
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) acc[j] = wave_sum<16>(acc[j]);      // over the 16 lanes of a point
  if (l != 0 || !valid) return;
  float w[3], r[3], s;
  interp_weights(a.d + row * 3, w, r, s);
  const float mean = (w[0] * acc[0] + w[1] * acc[1]) + w[2] * acc[2];
  const float* up = a.u.p + (int64_t)b * a.u.bs + (int64_t)n * a.u.ps;
  const float ux = up[0], uy = up[a.u.cs], uz = up[2 * a.u.cs];
  float gx = 0.f, gy = 0.f, gz = 0.f;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    // L -> w_j -> r_j (through the normalisation) -> d_j = |u - k_j|^2
    const float dd = -(r[j] * r[j]) * ((acc[j] - mean) / s);
    const float* kp = a.k.p + (int64_t)b * a.k.bs + (int64_t)id[j] * a.k.ps;
    const float tx = 2.f * (ux - kp[0]) * dd, ty = 2.f * (uy - kp[a.k.cs]) * dd, tz = 2.f * (uz - kp[2 * a.k.cs]) * dd;
    gx += tx, gy += ty, gz += tz;
    float* kr = a.krec + (row * 3 + j) * 3;
    kr[0] = -tx, kr[1] = -ty, kr[2] = -tz;
    a.wrec[row * 3 + j] = w[j];
  }
  float* o = a.gu + row * 3;
  o[0] = gx, o[1] = gy, o[2] = gz;
}

struct InterpBwdKnownArgs {
  const float* g;
  int64_t ldg;
  const float* y;
  int64_t ldy;
  const float *wrec, *krec;
  const int32_t *off, *lst;      // [B,M+1], [B,3N]: the entries n * 3 + j that read known row m, ascending
  int N, M, C;
  float* gF;             // [B,M,C]
  float* gk;             // [B,M,3]
};

// one thread per (known row, four channels): sums its reverse-index segment in ascending order
__global__ __launch_bounds__(256) void three_interp_bwd_known_kernel(InterpBwdKnownArgs a) {
  const int b = blockIdx.y, C4 = a.C >> 2;
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int m = t / C4, c = (t - m * C4) * 4;
  if (m >= a.M) return;
  const int E = 3 * a.N;
  int e0 = a.off[(int64_t)b * (a.M + 1) + m], e1 = a.off[(int64_t)b * (a.M + 1) + m + 1];
  e0 = e0 < 0 ? 0 : e0;
  e1 = e1 > E ? E : e1;
  const int32_t* lst = a.lst + (int64_t)b * E;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  float kx = 0.f, ky = 0.f, kz = 0.f;
  for (int q = e0; q < e1; ++q) {
    const int e = lst[q];
    if ((unsigned)e >= (unsigned)E) continue;
    const int64_t rec = (int64_t)b * E + e;
    const int64_t row = (int64_t)b * a.N + e / 3;
    const float w = a.wrec[rec];
    const float4 gv = masked_g(a.g + row * a.ldg + c, a.y ? a.y + row * a.ldy + c : nullptr);
    s.x += w * gv.x, s.y += w * gv.y, s.z += w * gv.z, s.w += w * gv.w;
    if (c == 0) kx += a.krec[rec * 3], ky += a.krec[rec * 3 + 1], kz += a.krec[rec * 3 + 2];
  }
  const int64_t mrow = (int64_t)b * a.M + m;
  *reinterpret_cast<float4*>(a.gF + mrow * a.C + c) = s;
  if (c == 0) a.gk[mrow * 3] = kx, a.gk[mrow * 3 + 1] = ky, a.gk[mrow * 3 + 2] = kz;
}

// ---- the coordinate head -------------------------------------------------------------------------------------------
constexpr int kTailK = 128, kTailMid = 64;         // pcd_layer: 128 -> 64 -> 3
constexpr int kTailBM = 128;                       // rows per workgroup (four waves of 32 rows)
constexpr int kTailBK = 32, kTailLD = 36;          // K step and the padded row of a staged operand tile
constexpr int kTailHLD = kTailMid + 1;

// Row (branch, b, n) of the [R*B*N, .] activations goes to row (b, branch * N + n) of the [B, R*N, 3] output.
__global__ __launch_bounds__(256) void pcd_tail_kernel(const float* __restrict__ H, int64_t ldh, const float* __restrict__ W3,
                                                       const float* __restrict__ b3, const float* __restrict__ W4,
                                                       const float* __restrict__ b4, int B, int N, int R,
                                                       uint32_t* __restrict__ mask, float* __restrict__ out) {
  __shared__ float lds[kTailBM * kTailHLD];          // operand tiles (128 + 64 rows of 36), then the 128 x 64 activations
  float* As = lds;
  float* Bs = lds + kTailBM * kTailLD;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, h = lane >> 5;
  const int64_t M = (int64_t)R * B * N, m0 = (int64_t)blockIdx.x * kTailBM;
  floatx16 acc[2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
  for (int k0 = 0; k0 < kTailK; k0 += kTailBK) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int f = tid + q * 256, row = f >> 3, kq = (f & 7) * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (m0 + row < M) v = *reinterpret_cast<const float4*>(H + (m0 + row) * ldh + k0 + kq);
      *reinterpret_cast<float4*>(As + row * kTailLD + kq) = v;
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int f = tid + q * 256, row = f >> 3, kq = (f & 7) * 4;
      *reinterpret_cast<float4*>(Bs + row * kTailLD + kq) = *reinterpret_cast<const float4*>(W3 + row * kTailK + k0 + kq);
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < kTailBK / 8; ++t) {
      const float4 av = *reinterpret_cast<const float4*>(As + (wv * 32 + r) * kTailLD + 8 * t + 4 * h);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const float4 bv = *reinterpret_cast<const float4*>(Bs + (j * 32 + r) * kTailLD + 8 * t + 4 * h);
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, acc[j], 0, 0, 0);
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, acc[j], 0, 0, 0);
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, acc[j], 0, 0, 0);
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, acc[j], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  // D: the lane holds column r of each 32-column tile, rows (e & 3) + 8 (e >> 2) + 4 h of the wave's 32
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int col = j * 32 + r;
    const float bj = b3[col];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int rl = wv * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
      const float v = acc[j][e] + bj;
      const unsigned long long bal = __builtin_amdgcn_ballot_w64(v > 0.f);   // lanes 0-31: row rl of h = 0, lanes 32-63: of h = 1
      if (r == 0 && m0 + rl < M) mask[(m0 + rl) * 2 + j] = (uint32_t)(h ? (bal >> 32) : bal);
      lds[rl * kTailHLD + col] = v > 0.f ? v : 0.f;
    }
  }
  __syncthreads();
  const int row = tid >> 1, half = tid & 1;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll 8
  for (int c = 0; c < 32; ++c) {
    const int cc = half * 32 + c;
    const float hv = lds[row * kTailHLD + cc];
    s0 += hv * W4[cc], s1 += hv * W4[kTailMid + cc], s2 += hv * W4[2 * kTailMid + cc];
  }
  s0 += __shfl_xor(s0, 1, 64), s1 += __shfl_xor(s1, 1, 64), s2 += __shfl_xor(s2, 1, 64);
  if (half == 0 && m0 + row < M) {
    const int64_t g = m0 + row, bn = (int64_t)B * N;
    const int64_t br = g / bn, rem = g - br * bn, b = rem / N, n = rem - b * N;
    float* o = out + ((b * R + br) * N + n) * 3;
    o[0] = s0 + b4[0], o[1] = s1 + b4[1], o[2] = s2 + b4[2];
  }
}

__global__ __launch_bounds__(256) void pcd_tail_bwd_kernel(const float* __restrict__ G, const uint32_t* __restrict__ mask,
                                                           const float* __restrict__ W4, const float* __restrict__ W3T, int B,
                                                           int N, int R, float* __restrict__ gh, int64_t ldgh) {
  __shared__ float lds[(kTailBM + kTailK) * kTailLD];
  float* As = lds;
  float* Bs = lds + kTailBM * kTailLD;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, h = lane >> 5;
  const int64_t M = (int64_t)R * B * N, m0 = (int64_t)blockIdx.x * kTailBM, bn = (int64_t)B * N;
  // the four rows this thread stages: their upstream gradient and sign words
  float g0[4], g1[4], g2[4];
  uint32_t mw[4][2];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int64_t g = m0 + ((tid + q * 256) >> 3);
    g0[q] = g1[q] = g2[q] = 0.f;
    mw[q][0] = mw[q][1] = 0u;
    if (g < M) {
      const int64_t br = g / bn, rem = g - br * bn, b = rem / N, n = rem - b * N;
      const float* gp = G + ((b * R + br) * N + n) * 3;
      g0[q] = gp[0], g1[q] = gp[1], g2[q] = gp[2];
      mw[q][0] = mask[g * 2], mw[q][1] = mask[g * 2 + 1];
    }
  }
  floatx16 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
#pragma unroll
  for (int k0 = 0; k0 < kTailMid; k0 += kTailBK) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int f = tid + q * 256, row = f >> 3, kq = (f & 7) * 4, c = k0 + kq;
      const uint32_t bits = mw[q][c >> 5] >> (c & 31);
      float4 v;
      v.x = (bits & 1u) ? (g0[q] * W4[c] + g1[q] * W4[kTailMid + c]) + g2[q] * W4[2 * kTailMid + c] : 0.f;
      v.y = (bits & 2u) ? (g0[q] * W4[c + 1] + g1[q] * W4[kTailMid + c + 1]) + g2[q] * W4[2 * kTailMid + c + 1] : 0.f;
      v.z = (bits & 4u) ? (g0[q] * W4[c + 2] + g1[q] * W4[kTailMid + c + 2]) + g2[q] * W4[2 * kTailMid + c + 2] : 0.f;
      v.w = (bits & 8u) ? (g0[q] * W4[c + 3] + g1[q] * W4[kTailMid + c + 3]) + g2[q] * W4[2 * kTailMid + c + 3] : 0.f;
      *reinterpret_cast<float4*>(As + row * kTailLD + kq) = v;
      *reinterpret_cast<float4*>(Bs + row * kTailLD + kq) = *reinterpret_cast<const float4*>(W3T + row * kTailMid + c);
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < kTailBK / 8; ++t) {
      const float4 av = *reinterpret_cast<const float4*>(As + (wv * 32 + r) * kTailLD + 8 * t + 4 * h);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float4 bv = *reinterpret_cast<const float4*>(Bs + (j * 32 + r) * kTailLD + 8 * t + 4 * h);
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, acc[j], 0, 0, 0);
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, acc[j], 0, 0, 0);
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, acc[j], 0, 0, 0);
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, acc[j], 0, 0, 0);
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int64_t g = m0 + wv * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
      if (g < M) gh[g * ldgh + j * 32 + r] = acc[j][e];
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int interp_check(const char* nm, int B, int N, int M, int C) {
  PC3D_REQUIRE(B >= 0 && N >= 1 && M >= 3 && C >= 4, "%s: bad sizes B=%d N=%d M=%d C=%d (M >= 3, C >= 4)", nm, B, N, M, C);
  PC3D_REQUIRE(C % 4 == 0, "%s: C=%d must be a multiple of 4", nm, C);
  PC3D_REQUIRE(B <= 65535, "%s: B=%d exceeds grid.y limit", nm, B);
  PC3D_REQUIRE((int64_t)N * (C / 4) < (int64_t)1 << 31 && (int64_t)M * (C / 4) < (int64_t)1 << 31 && (int64_t)3 * N < (int64_t)1 << 31,
               "%s: N=%d M=%d C=%d too large", nm, N, M, C);
  return PC3D_OK;
}

int tail_check(const char* nm, int B, int N, int R, int C2, int C3) {
  PC3D_REQUIRE(B >= 0 && N >= 1 && R >= 1, "%s: bad sizes B=%d N=%d R=%d", nm, B, N, R);
  PC3D_REQUIRE(C2 == kTailK && C3 == kTailMid, "%s: widths %d -> %d -> 3 asked, the kernel is built for %d -> %d -> 3", nm, C2, C3,
               kTailK, kTailMid);
  PC3D_REQUIRE((int64_t)R * B * N < (int64_t)1 << 31, "%s: R*B*N = %lld rows exceed the launch limit", nm,
               (long long)R * B * N);
  return PC3D_OK;
}

}  // namespace
}  // namespace pc3d

using namespace pc3d;

extern "C" int pc3d_three_interp_f32(const float* dists, const int32_t* idx, const float* feats, int64_t ldf, int B, int N, int M,
                                     int C, const float* bias, int relu, float* out, int64_t ldo, void* stream) {
  if (int rc = interp_check("pc3d_three_interp_f32", B, N, M, C)) return rc;
  PC3D_REQUIRE(ldf >= C && ldf % 4 == 0 && ldo >= C, "pc3d_three_interp_f32: ldf=%lld (>= C, multiple of 4), ldo=%lld (>= C)",
               (long long)ldf, (long long)ldo);
  if (B == 0) return PC3D_OK;
  PC3D_REQUIRE(dists && idx && feats && out, "pc3d_three_interp_f32: null pointer");
  PC3D_REQUIRE(aligned16(feats) && (!bias || aligned16(bias)), "pc3d_three_interp_f32: feats / bias must be 16-byte aligned");
  InterpArgs a{dists, idx, feats, ldf, N, M, C, out, ldo, bias, relu ? 1 : 0, (aligned16(out) && ldo % 4 == 0) ? 1 : 0};
  hipLaunchKernelGGL(three_interp_kernel, dim3(cdiv(N * (C / 4), 256), B), dim3(256), 0, as_stream(stream), a);
  PC3D_LAUNCH_CHECK("pc3d_three_interp_f32");
  return PC3D_OK;
}

extern "C" int pc3d_three_interp_bwd_f32(const float* u, int64_t u_bs, int64_t u_ps, int64_t u_cs, const float* k, int64_t k_bs,
                                         int64_t k_ps, int64_t k_cs, const float* dists, const int32_t* idx, const float* feats,
                                         int64_t ldf, const float* g, int64_t ldg, const float* y, int64_t ldy,
                                         const int32_t* rev_off, const int32_t* rev_lst, int B, int N, int M, int C, float* wrec,
                                         float* krec, float* gu, float* gF, float* gk, void* stream) {
  if (int rc = interp_check("pc3d_three_interp_bwd_f32", B, N, M, C)) return rc;
  PC3D_REQUIRE(ldf >= C && ldf % 4 == 0 && ldg >= C && (!y || ldy >= C), "pc3d_three_interp_bwd_f32: bad leading dimensions");
  if (B == 0) return PC3D_OK;
  PC3D_REQUIRE(u && k && dists && idx && feats && g && rev_off && rev_lst && wrec && krec && gu && gF && gk,
               "pc3d_three_interp_bwd_f32: null pointer");
  PC3D_REQUIRE(aligned16(feats) && aligned16(gF), "pc3d_three_interp_bwd_f32: feats / gF must be 16-byte aligned");
  const hipStream_t st = as_stream(stream);
  InterpBwdArgs a{{u, u_bs, u_ps, u_cs}, {k, k_bs, k_ps, k_cs}, dists, idx, feats, ldf, g, ldg, y, ldy, N, M, C, wrec, krec, gu};
  hipLaunchKernelGGL(three_interp_bwd_points_kernel, dim3(cdiv(N, 16), B), dim3(256), 0, st, a);
  PC3D_LAUNCH_CHECK("pc3d_three_interp_bwd_f32");
  InterpBwdKnownArgs kn{g, ldg, y, ldy, wrec, krec, rev_off, rev_lst, N, M, C, gF, gk};
  hipLaunchKernelGGL(three_interp_bwd_known_kernel, dim3(cdiv(M * (C / 4), 256), B), dim3(256), 0, st, kn);
  PC3D_LAUNCH_CHECK("pc3d_three_interp_bwd_f32");
  return PC3D_OK;
}

extern "C" int pc3d_pcd_tail_f32(const float* h, int64_t ldh, const float* w3, const float* b3, const float* w4, const float* b4,
                                 int B, int N, int R, int C2, int C3, uint32_t* mask, float* out, void* stream) {
  if (int rc = tail_check("pc3d_pcd_tail_f32", B, N, R, C2, C3)) return rc;
  PC3D_REQUIRE(ldh >= C2 && ldh % 4 == 0, "pc3d_pcd_tail_f32: ldh=%lld must be >= %d and a multiple of 4", (long long)ldh, C2);
  if (B == 0) return PC3D_OK;
  PC3D_REQUIRE(h && w3 && b3 && w4 && b4 && mask && out, "pc3d_pcd_tail_f32: null pointer");
  PC3D_REQUIRE(aligned16(h) && aligned16(w3), "pc3d_pcd_tail_f32: h / w3 must be 16-byte aligned");
  const int64_t M = (int64_t)R * B * N;
  hipLaunchKernelGGL(pcd_tail_kernel, dim3((unsigned)((M + kTailBM - 1) / kTailBM)), dim3(256), 0, as_stream(stream), h, ldh, w3, b3,
                     w4, b4, B, N, R, mask, out);
  PC3D_LAUNCH_CHECK("pc3d_pcd_tail_f32");
  return PC3D_OK;
}

extern "C" int pc3d_pcd_tail_bwd_f32(const float* g, const uint32_t* mask, const float* w4, const float* w3t, int B, int N, int R,
                                     int C2, int C3, float* gh, int64_t ldgh, void* stream) {
  if (int rc = tail_check("pc3d_pcd_tail_bwd_f32", B, N, R, C2, C3)) return rc;
  PC3D_REQUIRE(ldgh >= C2, "pc3d_pcd_tail_bwd_f32: ldgh=%lld must be >= %d", (long long)ldgh, C2);
  if (B == 0) return PC3D_OK;
  PC3D_REQUIRE(g && mask && w4 && w3t && gh, "pc3d_pcd_tail_bwd_f32: null pointer");
  PC3D_REQUIRE(aligned16(w3t), "pc3d_pcd_tail_bwd_f32: w3t must be 16-byte aligned");
  const int64_t M = (int64_t)R * B * N;
  hipLaunchKernelGGL(pcd_tail_bwd_kernel, dim3((unsigned)((M + kTailBM - 1) / kTailBM)), dim3(256), 0, as_stream(stream), g, mask, w4,
                     w3t, B, N, R, gh, ldgh);
  PC3D_LAUNCH_CHECK("pc3d_pcd_tail_bwd_f32");
  return PC3D_OK;
}
