// Device code shared by the PointNet tower kernels (pointmlp.hip, pointmlp_ft.hip): tile constants, the point load
// with the 3 x 3 input transform, and layer 1 (3 -> 64, ReLU) into LDS with its decision masks.
#pragma once
#include <type_traits>
#include "pc3d_common.h"

namespace pc3d {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int PM_C1 = 64;
constexpr int PM_C2 = 128;
constexpr int PM_TP = 128;           // forward: points per workgroup
constexpr int PM_LD1 = PM_C1 + 4;    // LDS row strides (floats): +4 keeps ds_read_b128 conflict-free
constexpr int PM_LD2 = PM_C2 + 4;
constexpr int PM_BTP = 32;           // backward: points per workgroup
constexpr int PM_MAXC3 = 1024;       // backward: widest pooled layer held in LDS

// T: the 3 x 3 transform of THIS cloud (or null)
__device__ __forceinline__ void load_point(const PtsView& x, const float* T, int b, int n, int N, float& px,
                                           float& py, float& pz) {
  px = py = pz = 0.f;
  if (n < N) {
    const float* p = x.p + (int64_t)b * x.bs + (int64_t)n * x.ps;
    const float x0 = p[0], x1 = p[x.cs], x2 = p[2 * x.cs];
    if (T) {
      const float* t = T;
      px = __builtin_fmaf(x2, t[6], __builtin_fmaf(x1, t[3], x0 * t[0]));
      py = __builtin_fmaf(x2, t[7], __builtin_fmaf(x1, t[4], x0 * t[1]));
      pz = __builtin_fmaf(x2, t[8], __builtin_fmaf(x1, t[5], x0 * t[2]));
    } else {
      px = x0, py = x1, pz = x2;
    }
  }
}

// h1[p][c] = relu(W1[c,:].x_p + b1[c]) for `npts` points whose coordinates sit in xs[3][npts]; lanes run over c.
// m1 (may be null) receives, for point p, the 64-bit mask of its positive channels: the wave's lanes ARE the 64
// channels, so the mask is one ballot; lane i keeps point i's mask and the wave stores `per` consecutive words.
template <int NPTS, int NTHREADS>
__device__ __forceinline__ void layer1_to_lds(const float* xs, float* h1, const float* W1, const float* b1,
                                              uint64_t* m1 = nullptr, int nvalid = NPTS) {
  const int c = threadIdx.x & (PM_C1 - 1);
  const int grp = threadIdx.x >> 6;
  constexpr int per = NPTS / (NTHREADS / 64);
  static_assert(per <= 64, "one mask word per lane");
  const float w0 = W1[c * 3 + 0], w1 = W1[c * 3 + 1], w2 = W1[c * 3 + 2], bb = b1[c];
  unsigned long long mine = 0ull;
#pragma unroll 4
  for (int i = 0; i < per; ++i) {
    const int p = grp * per + i;
    float v = __builtin_fmaf(w2, xs[2 * NPTS + p], __builtin_fmaf(w1, xs[NPTS + p], __builtin_fmaf(w0, xs[p], bb)));
    h1[p * PM_LD1 + c] = fmaxf(v, 0.f);
    const unsigned long long bal = __builtin_amdgcn_ballot_w64(v > 0.f);
    if (c == i) mine = bal;
  }
  if (m1 != nullptr && c < per && grp * per + c < nvalid) m1[grp * per + c] = mine;
}

constexpr int PM_MAXC3F = 1024;      // forward: widest layer 3 (cross-wave max scratch aliases the h2 tile)
constexpr int PM_FT = 512;           // forward: threads per workgroup (8 waves = 2 per SIMD: one wave's epilogue /
                                     // operand waits overlap the other's MFMAs)


// ---- the tower forward's arguments and prologue, shared by the exact kernel (pointmlp.hip) and the screened one
// (pointmlp_screen.hip): the same statements, so h2 and the two masks are the same bits by construction
struct PMFwdArgs {
  PtsView x;
  int N, C3, ntiles;
  const float* T;  // [B,3,3] or null: x'[n,:] = x[n,:] @ T  (model/pointnet.py:106-109)
  const float *W1, *b1, *W2, *b2, *W3, *b3;
  float* part_val;    // [B, ntiles, C3]
  int32_t* part_idx;  // [B, ntiles, C3]
  uint64_t* mask1;    // [B,N]    bit c  = (layer-1 output c of the point > 0), or null
  uint32_t* mask2;    // [B,N,4]  word j bit r = (layer-2 output 32j+r of the point > 0), or null
  // optional "transform head" (T == null): T[b] = th_W [9,th_K] . th_in[b] + th_b — STN3d's fc3 (+ identity folded
  // into th_b, model/pointnet.py:45-47) evaluated in this kernel's prologue instead of a launch of its own; tile 0 of
  // every cloud also writes it to th_out [B,9] for the backward
  const float *th_in, *th_W, *th_b;
  int th_K;
  float* th_out;
};

// The ragged instantiations' arguments: the dense ones and lengths [B] (device memory, read as data). A launch that
// carries them treats cloud b as L = clamp(lengths[b], 1, N) points: N stays the buffers' row count (every stride and the
// tile count), rows at and beyond L are never read and are handled as rows beyond N are (include/pc3d.h, the contract).
struct PMFwdArgsR : PMFwdArgs {
  const int32_t* lengths;
};
template <bool RAGGED>
using PMFwdArgsT = std::conditional_t<RAGGED, PMFwdArgsR, PMFwdArgs>;

__device__ __forceinline__ int pm_ragged_len(const int32_t* lengths, int b, int N) {
  const int l = lengths[b];
  return l < 1 ? 1 : l > N ? N : l;
}

// zero mask words for the workgroup's rows n0 + [0, 128) that lie in [from, N): thread = (row tid >> 2, mask2 word tid & 3)
__device__ __forceinline__ void pm_fwd_zero_masks(const PMFwdArgs& a, int b, int n0, int from) {
  if (a.mask1 == nullptr) return;
  const int n = n0 + ((int)threadIdx.x >> 2);
  if (threadIdx.x < 4 * PM_TP && n >= from && n < a.N) {
    a.mask2[((int64_t)b * a.N + n) * 4 + (threadIdx.x & 3)] = 0u;
    if ((threadIdx.x & 3) == 0) a.mask1[(int64_t)b * a.N + n] = 0ull;
  }
}

// A workgroup whose whole tile lies at or beyond its cloud's length (tile >= 1: tile 0 always holds point 0). It leaves
// ahead of the prologue's first barrier having written partials that the folds' strict `>` never takes and zero masks.
__device__ __forceinline__ void pm_fwd_skip_tile(const PMFwdArgs& a, int b, int tile) {
  const int64_t o = ((int64_t)b * a.ntiles + tile) * a.C3;
  for (int ch = threadIdx.x; ch < a.C3; ch += PM_FT) {
    a.part_val[o + ch] = -__builtin_inff();
    a.part_idx[o + ch] = 0;
  }
  pm_fwd_zero_masks(a, b, tile * PM_TP, tile * PM_TP);
}

constexpr int PM_FWD_LDS_FLOATS = PM_TP * PM_LD2 + 3 * PM_TP;   // h2 tile [128][132] (h1 aliases it) + xs [3][128]

// Transform head, x . T, layer 1 (VALU) and layer 2 (fp32 MFMA) of the workgroup's 128 points; mask1 / mask2 / th_out
// leave here. On return h2 [128][PM_LD2] sits at lds and every wave has passed the barrier behind its last write.
// nb: the cloud's points, a.N in a dense launch, its length in a ragged one (rows in [nb, a.N) get zero mask words).
template <bool RAGGED = false>
__device__ __forceinline__ void pm_fwd_prologue(const PMFwdArgs& a, float* lds, int nb) {
  float* h1 = lds;                       // [128][68]   (dead after layer 2)
  float* h2 = lds;                       // [128][132]  (overwrites h1 behind a barrier)
  float* xs = lds + PM_TP * PM_LD2;      // [3][128]
  const int tile = blockIdx.x, b = blockIdx.y;
  const int n0 = tile * PM_TP;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;

  const float* Tb = a.T ? a.T + (int64_t)b * 9 : nullptr;
  // raw coordinates first (their load latency overlaps the transform head's), the transform is applied afterwards
  float px = 0.f, py = 0.f, pz = 0.f;
  if (threadIdx.x < PM_TP) load_point(a.x, nullptr, b, n0 + threadIdx.x, nb, px, py, pz);
  if constexpr (RAGGED) pm_fwd_zero_masks(a, b, n0, nb);
  if (a.th_in) {   // 9 outputs x th_K: 32 lanes per output, strided partial sums + a half-wave reduction
    __shared__ float Ts[9];
    if (threadIdx.x < 9 * 32) {
      const int j = threadIdx.x >> 5, l = threadIdx.x & 31;
      const float* in = a.th_in + (int64_t)b * a.th_K;
      const float* w = a.th_W + (int64_t)j * a.th_K;
      float sacc = 0.f;
      if (a.th_K == 256) {      // STN3d: all eight operand pairs in flight at once
        float iv[8], wv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) iv[u] = in[l + 32 * u], wv[u] = w[l + 32 * u];
#pragma unroll
        for (int u = 0; u < 8; ++u) sacc = __builtin_fmaf(iv[u], wv[u], sacc);
      } else {
        for (int k = l; k < a.th_K; k += 32) sacc = __builtin_fmaf(in[k], w[k], sacc);
      }
#pragma unroll      // wave_sum<32>'s statements, kept in place: the headline's forward prologue
      for (int o = 16; o > 0; o >>= 1) sacc += __shfl_xor(sacc, o, 32);
      if (l == 0) {
        const float t = sacc + a.th_b[j];
        Ts[j] = t;
        if (tile == 0) a.th_out[(int64_t)b * 9 + j] = t;
      }
    }
    __syncthreads();
    Tb = Ts;
  }
  if (threadIdx.x < PM_TP) {
    if (Tb) {   // x' = x @ T (model/pointnet.py:106-109)
      const float x0 = px, x1 = py, x2 = pz;
      px = __builtin_fmaf(x2, Tb[6], __builtin_fmaf(x1, Tb[3], x0 * Tb[0]));
      py = __builtin_fmaf(x2, Tb[7], __builtin_fmaf(x1, Tb[4], x0 * Tb[1]));
      pz = __builtin_fmaf(x2, Tb[8], __builtin_fmaf(x1, Tb[5], x0 * Tb[2]));
    }
    xs[threadIdx.x] = px;
    xs[PM_TP + threadIdx.x] = py;
    xs[2 * PM_TP + threadIdx.x] = pz;
  }
  __syncthreads();
  layer1_to_lds<PM_TP, PM_FT>(xs, h1, a.W1, a.b1, a.mask1 ? a.mask1 + (int64_t)b * a.N + n0 : nullptr, nb - n0);
  __syncthreads();

  // ---- layer 2 on MFMA: D[pt][c2] = sum_k h1[pt][k] W2[c2][k]; wave owns c2 block (wave&3) and 2 of the 4 point tiles
  {
    const int c2b = wave & 3, tl0 = (wave >> 2) * 2;
    f32x16 acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
    const float* wrow = a.W2 + (32 * c2b + r) * PM_C1 + 4 * h;
#pragma unroll
    for (int t = 0; t < PM_C1 / 8; ++t) {
      const float4 bw = *reinterpret_cast<const float4*>(wrow + 8 * t);
      float4 av[2];
#pragma unroll
      for (int tl = 0; tl < 2; ++tl)
        av[tl] = *reinterpret_cast<const float4*>(h1 + ((tl0 + tl) * 32 + r) * PM_LD1 + 8 * t + 4 * h);
#pragma unroll
      for (int tl = 0; tl < 2; ++tl) {
        acc[tl] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[tl].x, bw.x, acc[tl], 0, 0, 0);
        acc[tl] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[tl].y, bw.y, acc[tl], 0, 0, 0);
        acc[tl] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[tl].z, bw.z, acc[tl], 0, 0, 0);
        acc[tl] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[tl].w, bw.w, acc[tl], 0, 0, 0);
      }
    }
    __syncthreads();  // every wave is done reading h1
    const float bias = a.b2[32 * c2b + r];
    unsigned long long mine = 0ull;   // lane 16*tl + e keeps the ballot of (tl, e): points pt(e,0) [low word], pt(e,1) [high]
#pragma unroll
    for (int tl = 0; tl < 2; ++tl)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int pt = (tl0 + tl) * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
        const float v = acc[tl][e] + bias;
        h2[pt * PM_LD2 + 32 * c2b + r] = fmaxf(v, 0.f);
        const unsigned long long bal = __builtin_amdgcn_ballot_w64(v > 0.f);
        if (lane == 16 * tl + e) mine = bal;
      }
    if (a.mask2 != nullptr && lane < 32) {   // the backward's layer-2 ReLU mask: exactly the decisions taken here
      const int tl = lane >> 4, e = lane & 15;
      const int pt0 = n0 + (tl0 + tl) * 32 + (e & 3) + 8 * (e >> 2);
      uint32_t* m2 = a.mask2 + ((int64_t)b * a.N) * 4 + c2b;
      if (pt0 < nb) m2[(int64_t)pt0 * 4] = (uint32_t)mine;
      if (pt0 + 4 < nb) m2[(int64_t)(pt0 + 4) * 4] = (uint32_t)(mine >> 32);
    }
  }
  __syncthreads();
}


// pointmlp_screen.hip: the same launch with layer 3 screened on the matrix pipe and rechecked exactly (the same bits).
// The prepared image of W3 (pm_w3_prepare_launch wrote it from THIS W3) that PC3D_PM_FWD_SCREEN_PREP reads; the
// in-launch form, PC3D_PM_FWD_SCREEN, makes the operands from the fp32 rows inside the launch.
struct PMScreenPrep {
  const __attribute__((ext_vector_type(8))) __bf16* w3_bf;   // [C3/32][8][2][64] x 8 bf16
  const float* w3_nw;                                        // [C3]
  const float4* w3_q;                                        // [32][C3]
};
// The fp16 image of the same W3 (pm_w3_prepare_h_launch) that the H forms read: layer 3 screened with ONE scaled fp16
// product per k-step (pointmlp_screen_h_bound.h), the same recheck, the same bits in every output; they need neither the
// bf16 image nor its w3_bf. dbg_S / dbg_E of these forms are written in the unscaled domain.
struct PMScreenPrepH {
  const __attribute__((ext_vector_type(8))) _Float16* w3_h;  // [C3/32][8][64] x 8 fp16: W3[32 cb + r][16 t + 8 h + 0..7] 2^sw
  const float* w3_cw;                                        // [C3] the channel's factor of E, scaled; +inf: not screened
  const float* w3_nw;                                        // [C3] (read by the dump instantiation only)
  const float4* w3_q;                                        // [32][C3]
};
// Launches `form`, one of PC3D_PM_FWD_SCREEN .. PC3D_PM_FWD_SCREEN_H_PAIR (include/pc3d.h; stats / dbg_S / dbg_E /
// stop_after as there). A form whose instantiation cannot be launched yet (first use on a device while the stream is
// capturing) steps aside for the next of H_PAIR -> H -> PREP -> SCREEN. Returns 0 when launched, 1 when none could be
// (the caller launches the exact kernel), < 0 on an error. prep / hprep: read by PREP and the H forms / by the H forms.
int pm_fwd_screen_launch(const PMFwdArgs& a, int B, void* stream, int32_t* stats, float* dbg_S, float* dbg_E,
                         int stop_after, int form, const PMScreenPrep& prep, const PMScreenPrepH& hprep);
// The ragged instantiation of the production form, PC3D_PM_FWD_SCREEN_H_PAIR. Returns 0 when launched, 1 when it cannot
// be yet (its first use on the device falls into a capture: the caller launches the ragged exact kernel), < 0 on an error.
int pm_fwd_screen_ragged_launch(const PMFwdArgsR& a, int B, void* stream, const PMScreenPrepH& hprep);
// pm_fwd_pair_ready: 1 once the production H_PAIR instantiation can be launched on the current device.
int pm_fwd_pair_ready();
// w3_bf (C3 * 512 B), w3_nw (C3 floats), w3_q (C3 * 128 floats) from the folded fp32 W3 [C3,128]
int pm_w3_prepare_launch(const float* W3, int C3, void* w3_bf, float* w3_nw, float* w3_q, void* stream);
// w3_h (C3 * 256 B) and w3_cw (C3 floats) from W3 and the w3_nw that pm_w3_prepare_launch wrote for it
int pm_w3_prepare_h_launch(const float* W3, int C3, const float* w3_nw, void* w3_h, float* w3_cw, void* stream);

}  // namespace pc3d
