// K8 — PointNet per-point MLP 3 -> C1(64) -> C2(128) -> C3 (1x1 conv + folded eval-BN + ReLU) fused with the
// max-pool over points, forward and backward-to-input.  gfx950, fp32-input MFMA (exact fp32 FMA chains).
//
// Replaces: model/pointnet.py:34-37 (STN3d tower) and :110-123 (PointNetfeat trunk): three Conv1d+BN(+ReLU) and
// torch.max over N, which materialise [B,64,N], [B,128,N] and [B,1024,N] activations (134 MB at B=32,N=1024).
//
// Forward: workgroup = (batch b, tile of 128 points), 8 waves. Layers 1-2 are computed once per tile into LDS
// (h2 tile [128 pts][128 ch], 66 KiB) and their ReLU decisions leave as per-point bit masks; layer 3 runs on v_mfma_f32_32x32x2_f32 with POINTS on the MFMA row index
// and CHANNELS on the column (lane) index, so the max over a tile's points is an in-register reduction
// (16 accumulator values per lane and channel block) + one cross-half shuffle; W3 rows stream from L2 as float4 per lane with a
// permuted-k order shared by both operands. Only (max, argmax) per (b, tile, channel) leaves the CU; a tiny second
// kernel folds the tiles. The [B,C3,N] activation is never written.
//
// Backward: max-pool routes each channel's gradient to ONE point, so dgrad of layer 3 is sparse:
// workgroup = (b, tile of 32 points) gathers the channels whose argmax falls in its tile in ascending channel order
// (deterministic, no atomics), applies the ReLU decisions of layers 1-2 that the FORWARD launch recorded as per-point
// bit masks (24 B per point — nothing is recomputed) and chains W2^T on MFMA and W1^T on the VALU.
#include <stdlib.h>
#include "pc3d_common.h"
#include "cw_update_body.h"
#include "pointmlp_body.h"

namespace pc3d {

// RAGGED: the cloud ends at its length instead of at N (pointmlp_body.h, PMFwdArgsR); a tile beyond it is skipped.
template <bool RAGGED>
__global__ __launch_bounds__(PM_FT) __attribute__((amdgpu_waves_per_eu(2, 2))) void pointmlp3_max_fwd_kernel(PMFwdArgsT<RAGGED> a) {
  __shared__ __attribute__((aligned(16))) float lds[PM_FWD_LDS_FLOATS];  // 69,120 B static
  const int tile = blockIdx.x, b = blockIdx.y;
  const int n0 = tile * PM_TP;
  int nb = a.N;              // the cloud's points
  if constexpr (RAGGED) {
    nb = pm_ragged_len(a.lengths, b, a.N);
    if (n0 >= nb) return pm_fwd_skip_tile(a, b, tile);   // (uniform) ahead of the first barrier
  }
  pm_fwd_prologue<RAGGED>(a, lds, nb);   // layers 1-2, masks, transform head: h2 [128][132] at lds, behind a barrier
  float* h2 = lds;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;

  // ---- layer 3 + max over the tile's points.
  // Wave w owns point tile (w & 3) = 32 points and half of the channel blocks ((w >> 2) selects blocks
  // [16*(w>>2), +16) of 32 channels when C3 = 1024). Its A operands (h2 of its 32 points, all 128 k) are read from LDS
  // ONCE into 64 VGPRs; only W3 streams (float4 per lane per 8 k, L2-resident, 4 waves share each row block).
  // One 16-register accumulator per channel block: a single dependent MFMA chain issues back-to-back on gfx950
  // (32x32x2 f32: issue interval = dependent latency = 64 cycles), and the SIMD's second wave fills every gap.
  const int ptile = wave & 3, cgrp = wave >> 2;
  float4 areg[PM_C2 / 8];
#pragma unroll
  for (int t = 0; t < PM_C2 / 8; ++t)
    areg[t] = *reinterpret_cast<const float4*>(h2 + (ptile * 32 + r) * PM_LD2 + 8 * t + 4 * h);
  __syncthreads();  // h2 fully consumed into registers: the LDS region is reused for the cross-wave max below
  float* pv = lds;                                        // [4 point tiles][C3]
  int* pi = reinterpret_cast<int*>(lds + 4 * PM_MAXC3F);  // [4 point tiles][C3]
  const int nblk = a.C3 / 32;
  const int blk_per_grp = (nblk + 1) / 2;
  const int cb_end = (cgrp + 1) * blk_per_grp < nblk ? (cgrp + 1) * blk_per_grp : nblk;
  // W3 rows are double-buffered in registers ACROSS channel blocks: while block cb runs its 64 MFMAs, the 16 float4
  // of block cb+1 are fetched (one load per 4 MFMAs, pinned with sched_group_barrier so hipcc cannot sink them to
  // just-in-time), i.e. every load has a full block (~4k cycles) to land.
  auto load_row = [&](float4 (&dst)[PM_C2 / 8], int cb) {
    const int cbc = cb < cb_end ? cb : cb_end - 1;  // past the end: harmless re-load of the last block
    const float* wrow = a.W3 + (int64_t)(cbc * 32 + r) * PM_C2 + 4 * h;
#pragma unroll
    for (int t = 0; t < PM_C2 / 8; ++t) dst[t] = *reinterpret_cast<const float4*>(wrow + 8 * t);
  };
  auto run_block = [&](const float4 (&cur)[PM_C2 / 8], float4 (&nxt)[PM_C2 / 8], int cb) {
    const int cbn = (cb + 1 < cb_end) ? cb + 1 : cb_end - 1;
    const float* nrow = a.W3 + (int64_t)(cbn * 32 + r) * PM_C2 + 4 * h;
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
    for (int t = 0; t < PM_C2 / 8; ++t) {
      nxt[t] = *reinterpret_cast<const float4*>(nrow + 8 * t);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(areg[t].x, cur[t].x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(areg[t].y, cur[t].y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(areg[t].z, cur[t].z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(areg[t].w, cur[t].w, acc, 0, 0, 0);
      __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);  // 1 VMEM read
      __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);  // 4 MFMA
    }
    const int ch = cb * 32 + r;
    float best = -__builtin_inff();
    // the winning accumulator row as an inline constant per select; the point index is formed once after the loop (and the
    // bounds test only runs in a ragged last tile): the epilogue's VALU instructions do not overlap the other wave's MFMAs
    int be = 0;
    const int base = n0 + ptile * 32;
    if (base + 32 <= nb) {              // (uniform)
#pragma unroll
      for (int e = 0; e < 16; ++e)      // ascending point index in e for fixed h: strict > keeps the lowest
        if (acc[e] > best) best = acc[e], be = (e & 3) + 8 * (e >> 2);
    } else {
#pragma unroll
      for (int e = 0; e < 16; ++e)
        if (base + (e & 3) + 8 * (e >> 2) + 4 * h < nb && acc[e] > best) best = acc[e], be = (e & 3) + 8 * (e >> 2);
    }
    int bi = best == -__builtin_inff() ? base : base + be + 4 * h;
    argmax_xor32(best, bi);
    if (h == 0) {
      pv[ptile * a.C3 + ch] = best;
      pi[ptile * a.C3 + ch] = bi;
    }
  };
  float4 bwA[PM_C2 / 8], bwB[PM_C2 / 8];
  const int cb_begin = cgrp * blk_per_grp;
  if (cb_begin < cb_end) {
    load_row(bwA, cb_begin);
    for (int cb = cb_begin; cb < cb_end; cb += 2) {
      run_block(bwA, bwB, cb);
      if (cb + 1 < cb_end) run_block(bwB, bwA, cb + 1);
    }
  }
  __syncthreads();
  for (int ch = threadIdx.x; ch < a.C3; ch += PM_FT) {
    float best = pv[ch];
    int bi = pi[ch];
#pragma unroll
    for (int t = 1; t < 4; ++t) {  // ascending point tile: strict > keeps the lowest point index on ties
      const float v = pv[t * a.C3 + ch];
      if (v > best) {
        best = v;
        bi = pi[t * a.C3 + ch];
      }
    }
    const int64_t o = ((int64_t)b * a.ntiles + tile) * a.C3 + ch;
    a.part_val[o] = best + a.b3[ch];
    a.part_idx[o] = bi;
  }
}

// fold tiles: pooled[b,c] = max_t part[b,t,c] (first tile wins ties => lowest point index), optional ReLU.
// The values AND the indices of PM_FOLD_U tiles are loaded together, unconditionally (tiles past ntiles are predicated
// off), and the winner is selected in registers in ascending tile order with the same strict `>`: one load round trip
// per PM_FOLD_U tiles, where loading a value, comparing and then fetching the winner's index is one (or two) per tile.
// SERIAL keeps that earlier form (pc3d_pointmlp3_fold_f32 with serial = 1: parity test and tools/bench_small_launches.py).
constexpr int PM_FOLD_U = 8;
template <bool SERIAL>
__global__ __launch_bounds__(256) void pointmlp3_fold_kernel(const float* part_val, const int32_t* part_idx,
                                                             int ntiles, int C3, int relu_last, float* pooled,
                                                             int32_t* argidx) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  if (c >= C3) return;
  const int64_t base = (int64_t)b * ntiles * C3 + c;
  float best;
  int bi;
  if (SERIAL) {
    best = part_val[base];
    bi = part_idx[base];
    for (int t = 1; t < ntiles; ++t) {
      const float v = part_val[base + (int64_t)t * C3];
      if (v > best) {
        best = v;
        bi = part_idx[base + (int64_t)t * C3];
      }
    }
  } else {
    best = 0.f, bi = 0;
    for (int t0 = 0; t0 < ntiles; t0 += PM_FOLD_U) {
      float v[PM_FOLD_U];
      int ix[PM_FOLD_U];
#pragma unroll
      for (int u = 0; u < PM_FOLD_U; ++u) {
        if (t0 + u < ntiles) {
          v[u] = part_val[base + (int64_t)(t0 + u) * C3];
          ix[u] = part_idx[base + (int64_t)(t0 + u) * C3];
        }
      }
#pragma unroll
      for (int u = 0; u < PM_FOLD_U; ++u) {
        if (t0 + u < ntiles) {
          const bool take = (t0 + u == 0) || (v[u] > best);   // tile 0 starts the running best, whatever it holds
          best = take ? v[u] : best;
          bi = take ? ix[u] : bi;
        }
      }
    }
  }
  if (relu_last) best = fmaxf(best, 0.f);
  pooled[(int64_t)b * C3 + c] = best;
  argidx[(int64_t)b * C3 + c] = bi;
}

// ---------------------------------------------------------------------------------------------------------
struct PMBwdArgs {
  PtsView x;
  int N, C3;
  const float* T;
  const float *W1, *b1, *W2, *b2, *W3, *W2T;  // W2T = W2 transposed, [64][128] row-major
  const int32_t* argidx;  // [B,C3]
  const uint64_t* mask1;  // [B,N]   layer-1 ReLU decisions of the forward launch (bit c)
  const uint32_t* mask2;  // [B,N,4] layer-2 ReLU decisions (word j, bit r = channel 32j+r)
  const float* g;         // [B,C3] upstream gradient on pooled (already masked for relu_last by the caller)
  PtsViewMut gx;          // T == null: gradient wrt the tower input; T given: gradient wrt the RAW points x
  float* part_gT;         // [B, ntiles, 16] per-tile partial of d/dT (9 used) or null
  int accumulate;         // gx += instead of gx =
};

// The two-list form of the backward (kept for parity tests and tools/bench_pointmlp.py; pc3d_pointmlp3_max_bwd_f32
// launches pointmlp3_max_bwd_kernel below, which computes the same bits).
// Workgroup = (batch b, 32 points), 4 waves; <= 36 KiB LDS so four workgroups share a CU (the kernel is a chain of
// dependent latencies, residency is what hides them).
//  A. channels whose arg-max lies in the tile are compacted IN CHANNEL ORDER (block prefix sum) into two lists
//     (points 0-15 / 16-31) and their rows g[c]*W3[c,:] are accumulated into g2s[pt][128] — ordered => deterministic;
//     each thread then clears the entries of its own column whose layer-2 ReLU was off in the FORWARD launch (the
//     forward kernel hands over its decisions as bit masks: nothing is recomputed, and no decision can differ);
//  C. g1 = (g2 masked) . W2 on MFMA with K = 128 split over wave pairs, masked by the forward's layer-1 bits;
//  D. g' = g1 . W1 on the VALU, then the x' = x @ T chain (dL/dx, per-tile partial of dL/dT).
__global__ __launch_bounds__(256) void pointmlp3_max_bwd_twolist_kernel(PMBwdArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[PM_BTP * PM_LD2 + PM_BTP * PM_LD1 + 4 * PM_BTP + PM_MAXC3 + (3 * PM_MAXC3) / 2];  // 36.4 KB
  float* g2s = lds;                                   // [32][132]
  float* h1s = g2s + PM_BTP * PM_LD2;                 // [32][68]   g1
  float* xs = h1s + PM_BTP * PM_LD1;                  // [3][32]    scratch of phase D
  int* s_scan = reinterpret_cast<int*>(xs + 3 * PM_BTP);   // [32] wave totals
  float* s_g = xs + 4 * PM_BTP;                       // [C3]
  short* s_n = reinterpret_cast<short*>(s_g + PM_MAXC3);   // [C3] local point index or -1
  short* list0 = s_n + PM_MAXC3;                      // [C3] channels hitting points 0..15, ascending
  short* list1 = list0 + PM_MAXC3;                    // [C3] channels hitting points 16..31
  __shared__ uint32_t s_m2[PM_BTP][4];
  __shared__ uint64_t s_m1[PM_BTP];
  const int tile = blockIdx.x, b = blockIdx.y;
  const int n0 = tile * PM_BTP;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;

  // ---- A1. classify 4 consecutive channels per thread, block-wide ordered compaction.
  // Issue the (tiny) arg-max / gradient / mask loads FIRST: vector-memory results return in issue order, so anything
  // issued behind the 32 KiB weight prefetch below would wait for all of it.
  int ld_n[PM_MAXC3 / 256];
  float ld_g[PM_MAXC3 / 256];
#pragma unroll
  for (int e = 0; e < PM_MAXC3 / 256; ++e) {
    const int c = tid * (PM_MAXC3 / 256) + e;
    ld_n[e] = (c < a.C3) ? a.argidx[(int64_t)b * a.C3 + c] : -1;
    ld_g[e] = (c < a.C3) ? a.g[(int64_t)b * a.C3 + c] : 0.f;
  }
  uint32_t ld_m2 = 0u;
  uint64_t ld_m1 = 0ull;
  if (tid < PM_BTP * 4 && n0 + (tid >> 2) < a.N) ld_m2 = a.mask2[((int64_t)b * a.N + n0) * 4 + tid];
  if (tid < PM_BTP && n0 + tid < a.N) ld_m1 = a.mask1[(int64_t)b * a.N + n0 + tid];
  // MFMA B operand of phase C depends on nothing: fetch it now so its L2 latency hides under phase A
  float4 w2tr[PM_C2 / 16];
  {
    // phase C: wave = (j block wave&1, K half wave>>1): k in [64*(wave>>1), +64)
    const float* wtrow = a.W2T + (32 * (wave & 1) + r) * PM_C2 + 64 * (wave >> 1) + 4 * h;
#pragma unroll
    for (int t = 0; t < PM_C2 / 16; ++t) w2tr[t] = *reinterpret_cast<const float4*>(wtrow + 8 * t);
  }
  int cnt0 = 0, cnt1 = 0;
  int myn[PM_MAXC3 / 256];
#pragma unroll
  for (int e = 0; e < PM_MAXC3 / 256; ++e) {
    const int c = tid * (PM_MAXC3 / 256) + e;
    int n = -1;
    if (c < a.C3) {
      n = ld_n[e] - n0;
      const float gv = ld_g[e];
      if (n < 0 || n >= PM_BTP || gv == 0.f) n = -1;
      s_g[c] = gv;
      s_n[c] = (short)n;
    }
    myn[e] = n;
    cnt0 += (n >= 0 && n < 16) ? 1 : 0;
    cnt1 += (n >= 16) ? 1 : 0;
  }
  if (tid < PM_BTP * 4) s_m2[tid >> 2][tid & 3] = ld_m2;
  if (tid < PM_BTP) s_m1[tid] = ld_m1;
  for (int i = tid; i < PM_BTP * PM_LD2; i += 256) g2s[i] = 0.f;
  int packed = cnt0 | (cnt1 << 16);
  int incl = packed;      // wave_incl_scan's statements, kept in place in this file: the headline's backward
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(incl, o, 64);
    if (lane >= o) incl += v;
  }
  if (lane == 63) s_scan[wave] = incl;
  __syncthreads();
  int base = 0, total = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const int v = s_scan[w];
    if (w < wave) base += v;
    total += v;
  }
  const int len0 = total & 0xffff, len1 = total >> 16;
  if (len0 + len1 == 0) {  // no critical point in this tile: gradient is exactly zero
    if (tid < 3 * PM_BTP && !a.accumulate) {
      const int p = tid & (PM_BTP - 1), c = tid >> 5;
      if (n0 + p < a.N) a.gx.p[(int64_t)b * a.gx.bs + (int64_t)(n0 + p) * a.gx.ps + c * a.gx.cs] = 0.f;
    }
    if (a.part_gT && tid < 16) a.part_gT[((int64_t)b * gridDim.x + tile) * 16 + tid] = 0.f;
    return;
  }
  {
    const int excl = base + incl - packed;
    int o0 = excl & 0xffff, o1 = excl >> 16;
#pragma unroll
    for (int e = 0; e < PM_MAXC3 / 256; ++e) {
      const int n = myn[e];
      const int c = tid * (PM_MAXC3 / 256) + e;
      if (n >= 0 && n < 16) list0[o0++] = (short)c;
      if (n >= 16) list1[o1++] = (short)c;
    }
  }
  __syncthreads();

  // ---- A2. ordered accumulation: thread (k, half) walks its half's list; loads are independent -> pipelined
  {
    const int k = tid & (PM_C2 - 1), ph = tid >> 7;
    const short* list = ph ? list1 : list0;
    const int len = ph ? len1 : len0;
    int i = 0;
    for (; i + 8 <= len; i += 8) {  // 8 independent W3 loads in flight per round trip
      int c[8];
      float w[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        c[e] = list[i + e];
        w[e] = a.W3[(int64_t)c[e] * PM_C2 + k];
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float* dst = g2s + (int)s_n[c[e]] * PM_LD2 + k;
        *dst = __builtin_fmaf(s_g[c[e]], w[e], *dst);
      }
    }
    for (; i + 2 <= len; i += 2) {
      const int c0 = list[i], c1 = list[i + 1];
      const float w0 = a.W3[(int64_t)c0 * PM_C2 + k], w1 = a.W3[(int64_t)c1 * PM_C2 + k];
      float* d0 = g2s + (int)s_n[c0] * PM_LD2 + k;
      *d0 = __builtin_fmaf(s_g[c0], w0, *d0);
      float* d1 = g2s + (int)s_n[c1] * PM_LD2 + k;
      *d1 = __builtin_fmaf(s_g[c1], w1, *d1);
    }
    for (; i < len; ++i) {
      const int c = list[i];
      float* dst = g2s + (int)s_n[c] * PM_LD2 + k;
      *dst = __builtin_fmaf(s_g[c], a.W3[(int64_t)c * PM_C2 + k], *dst);
    }
    // layer-2 ReLU of the forward pass: this thread is the only writer of column k for its half's 16 points, so it
    // applies the mask to them without a barrier (bit k&31 of word k>>5 of the point's mask2)
#pragma unroll
    for (int p = 0; p < 16; ++p) {
      const int pt = 16 * ph + p;
      if (!((s_m2[pt][k >> 5] >> (k & 31)) & 1u)) g2s[pt * PM_LD2 + k] = 0.f;
    }
  }
  __syncthreads();

  // ---- C. g1[pt][j] = sum_k2 g2[pt][k2] W2[k2][j] on MFMA: wave = (j block wave&1, K half wave>>1)
  {
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    const int jb = wave & 1, kh = wave >> 1;
#pragma unroll
    for (int t = 0; t < PM_C2 / 16; ++t) {
      const float4 bw = w2tr[t];
      const float4 av = *reinterpret_cast<const float4*>(g2s + r * PM_LD2 + 64 * kh + 8 * t + 4 * h);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bw.x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bw.y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bw.z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bw.w, acc, 0, 0, 0);
    }
    // the upper K half hands its partial tile to the lower one through LDS (fixed order: deterministic); g2s is dead
    // once every wave has read its A operands, so it doubles as the exchange buffer (one [32][33] tile per j block)
    __syncthreads();
    float* cr = g2s + jb * (32 * 33);
    if (kh == 1) {
#pragma unroll
      for (int e = 0; e < 16; ++e) cr[((e & 3) + 8 * (e >> 2) + 4 * h) * 33 + r] = acc[e];
    }
    __syncthreads();
    if (kh == 0) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int pt = (e & 3) + 8 * (e >> 2) + 4 * h;
        const bool on = (s_m1[pt] >> (32 * jb + r)) & 1ull;          // layer-1 ReLU of the forward pass
        h1s[pt * PM_LD1 + 32 * jb + r] = on ? (acc[e] + cr[pt * 33 + r]) : 0.f;
      }
    }
  }
  __syncthreads();

  // ---- D. g'[p][c] = sum_j W1[j][c] g1[p][j]  (gradient wrt the tower input x' = x @ T)
  float* gp = xs;  // [3][32] scratch
  if (wave < 3 && lane < PM_BTP) {   // wave = coordinate c (uniform -> W1 comes through scalar loads), lane = point
    const int p = lane, c = wave;
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int j = 0; j < PM_C1; j += 4) {
      const float4 hv = *reinterpret_cast<const float4*>(h1s + p * PM_LD1 + j);
      s0 = __builtin_fmaf(a.W1[j * 3 + c], hv.x, s0);
      s1 = __builtin_fmaf(a.W1[(j + 1) * 3 + c], hv.y, s1);
      s0 = __builtin_fmaf(a.W1[(j + 2) * 3 + c], hv.z, s0);
      s1 = __builtin_fmaf(a.W1[(j + 3) * 3 + c], hv.w, s1);
    }
    gp[c * PM_BTP + p] = s0 + s1;
  }
  __syncthreads();
  if (wave == 0) {  // lanes 0..31 = the tile's points; lanes 32..63 contribute zeros to the reductions
    const int p = lane & (PM_BTP - 1);
    const bool live = lane < PM_BTP;
    const float g0 = live ? gp[p] : 0.f, g1v = live ? gp[PM_BTP + p] : 0.f, g2v = live ? gp[2 * PM_BTP + p] : 0.f;
    float o0 = g0, o1 = g1v, o2 = g2v;
    if (a.T) {
      // x' = x @ T  =>  dL/dx[c] = sum_c' g'[c'] T[c][c'] ;  dL/dT[c][c'] = sum_p x[p][c] g'[p][c']
      // (the chain starts from +0, so a dead point, g' = +0, gets +0 and not -0 under a row of negative T entries)
      const float* t = a.T + (int64_t)b * 9;
      o0 = __builtin_fmaf(g2v, t[2], __builtin_fmaf(g1v, t[1], __builtin_fmaf(g0, t[0], 0.f)));
      o1 = __builtin_fmaf(g2v, t[5], __builtin_fmaf(g1v, t[4], __builtin_fmaf(g0, t[3], 0.f)));
      o2 = __builtin_fmaf(g2v, t[8], __builtin_fmaf(g1v, t[7], __builtin_fmaf(g0, t[6], 0.f)));
      if (a.part_gT) {
        float xr[3] = {0.f, 0.f, 0.f};
        if (live && n0 + p < a.N) {
          const float* xp = a.x.p + (int64_t)b * a.x.bs + (int64_t)(n0 + p) * a.x.ps;
          xr[0] = xp[0], xr[1] = xp[a.x.cs], xr[2] = xp[2 * a.x.cs];
        }
        const float gv[3] = {g0, g1v, g2v};
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
          for (int d = 0; d < 3; ++d) {
            const float sum = wave_sum(xr[c] * gv[d]);
            if (lane == 0) a.part_gT[((int64_t)b * gridDim.x + tile) * 16 + c * 3 + d] = sum;
          }
        if (lane >= 9 && lane < 16) a.part_gT[((int64_t)b * gridDim.x + tile) * 16 + lane] = 0.f;
      }
    }
    if (live && n0 + p < a.N) {
      float* q = a.gx.p + (int64_t)b * a.gx.bs + (int64_t)(n0 + p) * a.gx.ps;
      if (a.accumulate) {
        q[0] += o0, q[a.gx.cs] += o1, q[2 * a.gx.cs] += o2;
      } else {
        q[0] = o0, q[a.gx.cs] = o1, q[2 * a.gx.cs] = o2;
      }
    }
  }
}


// The balanced form. Same grid, tile, LDS budget and arithmetic as the two-list kernel above; what differs is how the
// layer-3 gather (phase A) is scheduled:
//  A1. the tile's hits are compacted in channel order into ONE list of (local point, channel) pairs, then a stable
//      counting sort over the 32 points orders them by point and, within a point, by ascending channel;
//  A2. the four waves share out WHOLE points: point p goes to wave floor(4 * start[p] / L) (start = its offset in the
//      sorted list, L = hits in the tile), so a wave gets at most ceil(L / 4) hits plus the rest of its last point.
//      A lane holds a float2 of k (a W3 row is one 512-B request of the wave) and a point's row is the register chain
//      acc = fma(g[c], W3[c,k], acc) from +0 in ascending channel order — the chain the two-list kernel forms through
//      LDS read-modify-writes, so every bit of g2 is the same whichever wave runs it — written once with the layer-2
//      mask applied. The walk is wave-uniform: one LDS read fetches up to 64 list entries (and one their gradients),
//      v_readlane hands them out as scalars, so point changes are scalar branches and 32 independent row loads are in
//      flight per wave with nothing but the FMAs behind them.
// Everything that depends on nothing (T[b], the tile's raw x, the old gx of an accumulating launch, W1) is fetched at
// entry, in front of the W2 operand prefetch, and parked in LDS. That prefetch reads W2 itself ([128][64]: 32 lanes =
// 32 consecutive j of one k2 row, two 128-B lines per instruction) instead of W2T, where every lane of a float4 load
// sits in a row of its own (64 lines per instruction; measured 2.5 us of the launch's first 5.8).
constexpr int PM_BSEG = 8;           // list segments (of 32 lanes = 32 bins each) of the counting sort
constexpr int PM_BFLY = 32;          // W3 rows in flight per wave

// phase C of the backward kernels: g1 = (g2 masked) . W2 on MFMA, K split over wave pairs, layer-1 mask applied.
// One call = one block of 32 rows of g2s / h1s / s_m1 and four waves (wave = 0..3). live: false for a group of waves
// that has no row block left (the packed form); it then only keeps the barriers.
__device__ __forceinline__ void pm_bwd_phase_c(const float4 (&w2tr)[PM_C2 / 16], float* g2s, float* h1s,
                                               const uint64_t* s_m1, int wave, int r, int h, bool live = true) {
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  const int jb = wave & 1, kh = wave >> 1;
  if (live) {
#pragma unroll
    for (int t = 0; t < PM_C2 / 16; ++t) {
      const float4 bw = w2tr[t];
      const float4 av = *reinterpret_cast<const float4*>(g2s + r * PM_LD2 + 64 * kh + 8 * t + 4 * h);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bw.x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bw.y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bw.z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bw.w, acc, 0, 0, 0);
    }
  }
  __syncthreads();   // g2s is dead once every wave has read its A operands: it doubles as the exchange buffer
  float* cr = g2s + jb * (32 * 33);
  if (live && kh == 1) {
#pragma unroll
    for (int e = 0; e < 16; ++e) cr[((e & 3) + 8 * (e >> 2) + 4 * h) * 33 + r] = acc[e];
  }
  __syncthreads();
  if (live && kh == 0) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int pt = (e & 3) + 8 * (e >> 2) + 4 * h;
      const bool on = (s_m1[pt] >> (32 * jb + r)) & 1ull;          // layer-1 ReLU of the forward pass
      h1s[pt * PM_LD1 + 32 * jb + r] = on ? (acc[e] + cr[pt * 33 + r]) : 0.f;
    }
  }
}

// a finished point's row: layer-2 ReLU of the forward pass, one store (lane = k 2*lane, 2*lane + 1).
// key = an entry >> 10: the point itself or, in the packed form, (row slot << 7 | point)
template <bool PACKED>
__device__ __forceinline__ void pm_bwd_put_row(const uint32_t (*s_m2)[4], float* g2s, int key, int lane, float2 acc) {
  const int pt = PACKED ? (key & 127) : key, row = PACKED ? (key >> 7) : key;
  const uint32_t m = s_m2[pt][lane >> 4] >> ((2 * lane) & 31);
  float2 o;
  o.x = (m & 1u) ? acc.x : 0.f, o.y = (m & 2u) ? acc.y : 0.f;
  *reinterpret_cast<float2*>(g2s + row * PM_LD2 + 2 * lane) = o;
}

// NB entries of the wave's current chunk, from entry u on: lane s of my_e / my_g holds entry s (point << 10 | channel)
// and its gradient; nb = entries in the chunk. TAIL: the batch may reach past nb (entries at or past nb repeat the
// last one and are not accumulated). Everything but the row loads and the FMAs is scalar.
template <int NB, bool TAIL, bool PACKED = false>
__device__ __forceinline__ void pm_bwd_rows(const float* W3, int my_e, int my_g, const uint32_t (*s_m2)[4], float* g2s,
                                            int u, int nb, int lane, float2& acc, int& cur) {
  int e[NB];
  float2 w[NB];
#pragma unroll
  for (int t = 0; t < NB; ++t) {
    const int s = (!TAIL || u + t < nb) ? u + t : nb - 1;
    e[t] = __builtin_amdgcn_readlane(my_e, s);
    w[t] = *reinterpret_cast<const float2*>(W3 + (size_t)(uint32_t)((e[t] & (PM_MAXC3 - 1)) * PM_C2 + 2 * lane));
  }
#pragma unroll
  for (int t = 0; t < NB; ++t) {
    if (!TAIL || u + t < nb) {
      const float gv = __builtin_bit_cast(float, __builtin_amdgcn_readlane(my_g, u + t));
      const int n = e[t] >> 10;
      if (__builtin_expect(n != cur, 0)) {
        if (cur >= 0) pm_bwd_put_row<PACKED>(s_m2, g2s, cur, lane, acc);
        acc = make_float2(0.f, 0.f);
        cur = n;
      }
      acc.x = __builtin_fmaf(gv, w[t].x, acc.x);
      acc.y = __builtin_fmaf(gv, w[t].y, acc.y);
    }
  }
}

// The CW update as the epilogue of the LAST backward launch of an iteration (the STN tower's, in accumulate form): the
// three values lane p of wave 0 holds at the end — the gradient already in gx plus this tower's — are the whole input
// gradient of point p, so Adam + clip + the distance gradient (cw_point_update) run right there instead of in a launch
// of their own. A workgroup reads and writes only its own 32 points: updating adv in place is safe.
struct PMUpdArgs {
  PtsViewMut adv;            // the iterate (the tower's x), updated in place; m / v share its layout
  float *m, *v;
  PtsView ori;
  const int32_t* nn_idx;     // [B,N] (kind 2)
  const float* w;            // [B] (kind 1, 2)
  const float* dist_val;     // [B] ||adv - ori||_F (kind 1)
  const float* adam;         // [2] {step_size, bc2s}
  int B;
  int dist_kind;
  float omb1, omb2, fb2, eps, budget;
};
constexpr int PM_UPD_LD = 3 * PM_BTP;   // parked operands: [p, ori, m, v, ori[nn]][coordinate][point] + 4 per-sample words

// the lane of point n = n0 + p (p = its index among the workgroup's TPTS points) with its whole input gradient
// (g0, g1, g2); s_u = the operands parked at entry, [5][3][TPTS] + 4 per-sample words
template <int TPTS = PM_BTP>
__device__ __forceinline__ void pm_bwd_update_point(const PMUpdArgs& u, const float* s_u, int N, int b, int n, int p,
                                                    float g0, float g1, float g2) {
  constexpr int LD = 3 * TPTS;
  const float* s_uc = s_u + 5 * LD;
  const CwPointConsts c{u.dist_kind, u.B, N, AdamConsts{u.omb1, u.omb2, u.fb2, s_uc[2], s_uc[3], u.eps}, u.budget};
  float pin[3], oin[3], m[3], v[3], q[3], np_[3], g[3] = {g0, g1, g2};
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    pin[e] = s_u[0 * LD + e * TPTS + p];
    oin[e] = s_u[1 * LD + e * TPTS + p];
    m[e] = s_u[2 * LD + e * TPTS + p];
    v[e] = s_u[3 * LD + e * TPTS + p];
    q[e] = s_u[4 * LD + e * TPTS + p];
  }
  cw_point_update(c, pin, oin, g, q, s_uc[0], s_uc[1], m, v, np_);
  const int64_t off = (int64_t)b * u.adv.bs + (int64_t)n * u.adv.ps;
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    u.m[off + e * u.adv.cs] = m[e];
    u.v[off + e * u.adv.cs] = v[e];
    u.adv.p[off + e * u.adv.cs] = np_[e];
  }
}

// UPD: the accumulate form whose epilogue applies the CW update instead of storing gx (pointmlp3_max_bwd_update_kernel)
template <bool UPD>
__device__ __forceinline__ void pm_bwd_body(const PMBwdArgs& a, const PMUpdArgs& u) {
  __shared__ __attribute__((aligned(16))) float lds[PM_BTP * PM_LD2 + PM_BTP * PM_LD1 + 4 * PM_BTP + PM_MAXC3 + PM_MAXC3];  // 34.3 KB
  float* g2s = lds;                                   // [32][132]
  float* h1s = g2s + PM_BTP * PM_LD2;                 // [32][68]   g1 (phase C on); before that the sort's counters
  float* xs = h1s + PM_BTP * PM_LD1;                  // [3][32]    scratch of phase D
  int* s_scan = reinterpret_cast<int*>(xs + 3 * PM_BTP);   // [32] wave totals
  float* s_g = xs + 4 * PM_BTP;                       // [C3]
  unsigned short* s_hit = reinterpret_cast<unsigned short*>(s_g + PM_MAXC3);   // [C3] (point << 10 | channel), channel order
  unsigned short* s_sorted = s_hit + PM_MAXC3;        // [C3] the same, ordered by (point, channel)
  int* s_cnt = reinterpret_cast<int*>(h1s);           // [8][32] hits of point p in list segment q
  int* s_start = s_cnt + PM_BSEG * PM_BTP;            // [33]    offset of point p in the sorted list
  __shared__ uint32_t s_m2[PM_BTP][4];
  __shared__ uint64_t s_m1[PM_BTP];
  __shared__ float s_W1[PM_C1 * 3];
  __shared__ float s_x[3 * PM_BTP], s_gxo[3 * PM_BTP], s_T[12];
  __shared__ float s_u[UPD ? 5 * PM_UPD_LD + 4 : 1];
  static_assert(PM_MAXC3 <= 1024 && PM_BTP <= 32, "a hit is packed as point << 10 | channel in 16 bits");
  const int tile = blockIdx.x, b = blockIdx.y;
  const int n0 = tile * PM_BTP;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;

  // ---- entry: every load that depends on nothing, smallest first (vector-memory results return in issue order, so
  // anything issued behind the 32 KiB weight prefetch below would wait for all of it)
  float ld_u[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  if (UPD) {   // the update's operands first: ori[nn_idx] is the one dependent load of the launch
    if (tid < 3 * PM_BTP) {
      const int p = tid & (PM_BTP - 1), c = tid >> 5;
      if (n0 + p < a.N) {
        const int64_t off = (int64_t)b * u.adv.bs + (int64_t)(n0 + p) * u.adv.ps + c * u.adv.cs;
        const float* ob = u.ori.p + (int64_t)b * u.ori.bs + c * u.ori.cs;
        const int j = (u.dist_kind == 2) ? u.nn_idx[(int64_t)b * a.N + n0 + p] : 0;
        ld_u[0] = u.adv.p[off];
        ld_u[1] = ob[(int64_t)(n0 + p) * u.ori.ps];
        ld_u[2] = u.m[off];
        ld_u[3] = u.v[off];
        if (u.dist_kind == 2) ld_u[4] = ob[(int64_t)j * u.ori.ps];
      }
    } else if (tid < 3 * PM_BTP + 4) {
      const int e = tid - 3 * PM_BTP;
      if (e == 0) ld_u[0] = u.w ? u.w[b] : 0.f;
      else if (e == 1) ld_u[0] = u.dist_val ? u.dist_val[b] : 0.f;
      else ld_u[0] = u.adam[e - 2];
    }
  }
  int ld_n[PM_MAXC3 / 256];
  float ld_g[PM_MAXC3 / 256];
#pragma unroll
  for (int e = 0; e < PM_MAXC3 / 256; ++e) {
    const int c = tid * (PM_MAXC3 / 256) + e;
    ld_n[e] = (c < a.C3) ? a.argidx[(int64_t)b * a.C3 + c] : -1;
    ld_g[e] = (c < a.C3) ? a.g[(int64_t)b * a.C3 + c] : 0.f;
  }
  uint32_t ld_m2 = 0u;
  uint64_t ld_m1 = 0ull;
  if (tid < PM_BTP * 4 && n0 + (tid >> 2) < a.N) ld_m2 = a.mask2[((int64_t)b * a.N + n0) * 4 + tid];
  if (tid < PM_BTP && n0 + tid < a.N) ld_m1 = a.mask1[(int64_t)b * a.N + n0 + tid];
  const bool want_gT = a.T != nullptr && a.part_gT != nullptr;
  float ld_w1 = 0.f, ld_px = 0.f, ld_t = 0.f;
  if (tid < PM_C1 * 3) ld_w1 = a.W1[tid];
  if (tid < 3 * PM_BTP) {   // (coordinate tid >> 5, point tid & 31): the tile's raw x and the gradient already in gx
    const int p = tid & (PM_BTP - 1), c = tid >> 5;
    if (n0 + p < a.N) {
      if (want_gT) ld_px = a.x.p[(int64_t)b * a.x.bs + (int64_t)(n0 + p) * a.x.ps + c * a.x.cs];
      if (a.accumulate) ld_t = a.gx.p[(int64_t)b * a.gx.bs + (int64_t)(n0 + p) * a.gx.ps + c * a.gx.cs];
    }
  } else if (tid >= 128 && tid < 137 && a.T) {
    ld_t = a.T[(int64_t)b * 9 + tid - 128];
  }
  // MFMA B operand of phase C depends on nothing either: its L2 latency hides under phase A
  float4 w2tr[PM_C2 / 16];
  {
    // phase C: wave = (j block wave&1, K half wave>>1): k2 in [64*(wave>>1), +64); lane (r, h) holds, for step t,
    // W2[64*(wave>>1) + 8t + 4h + {0..3}][32*(wave&1) + r]  (= the float4 of W2T the two-list kernel loads)
    const float* wcol = a.W2 + (64 * (wave >> 1) + 4 * h) * PM_C1 + 32 * (wave & 1) + r;
#pragma unroll
    for (int t = 0; t < PM_C2 / 16; ++t) {
      w2tr[t].x = wcol[(8 * t + 0) * PM_C1];
      w2tr[t].y = wcol[(8 * t + 1) * PM_C1];
      w2tr[t].z = wcol[(8 * t + 2) * PM_C1];
      w2tr[t].w = wcol[(8 * t + 3) * PM_C1];
    }
  }

  // ---- A1. classify 4 consecutive channels per thread; block-wide ordered compaction of the hits
  int cnt = 0;
  int myn[PM_MAXC3 / 256];
#pragma unroll
  for (int e = 0; e < PM_MAXC3 / 256; ++e) {
    const int c = tid * (PM_MAXC3 / 256) + e;
    int n = -1;
    if (c < a.C3) {
      n = ld_n[e] - n0;
      const float gv = ld_g[e];
      if (n < 0 || n >= PM_BTP || gv == 0.f) n = -1;
      s_g[c] = gv;
    }
    myn[e] = n;
    cnt += (n >= 0) ? 1 : 0;
  }
  if (tid < PM_BTP * 4) s_m2[tid >> 2][tid & 3] = ld_m2;
  if (tid < PM_BTP) s_m1[tid] = ld_m1;
  if (tid < PM_C1 * 3) s_W1[tid] = ld_w1;
  if (tid < 3 * PM_BTP) {
    s_x[tid] = ld_px;
    s_gxo[tid] = ld_t;
  } else if (tid >= 128 && tid < 137) {
    s_T[tid - 128] = ld_t;
  }
  if (UPD) {
    if (tid < 3 * PM_BTP) {
#pragma unroll
      for (int e = 0; e < 5; ++e) s_u[e * PM_UPD_LD + tid] = ld_u[e];
    } else if (tid < 3 * PM_BTP + 4) {
      s_u[5 * PM_UPD_LD + tid - 3 * PM_BTP] = ld_u[0];
    }
  }
  for (int i = tid; i < PM_BTP * PM_LD2; i += 256) g2s[i] = 0.f;   // a point without a hit keeps a zero row
  int incl = cnt;      // wave_incl_scan's statements, kept in place
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(incl, o, 64);
    if (lane >= o) incl += v;
  }
  if (lane == 63) s_scan[wave] = incl;
  __syncthreads();
  int base = 0, L = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const int v = s_scan[w];
    if (w < wave) base += v;
    L += v;
  }
  if (L == 0) {  // no critical point in this tile: gradient is exactly zero
    if (UPD && wave == 0 && lane < PM_BTP && n0 + lane < a.N)   // the gradient already in gx is the whole gradient
      pm_bwd_update_point(u, s_u, a.N, b, n0 + lane, lane, s_gxo[lane], s_gxo[PM_BTP + lane], s_gxo[2 * PM_BTP + lane]);
    if (tid < 3 * PM_BTP && !a.accumulate) {
      const int p = tid & (PM_BTP - 1), c = tid >> 5;
      if (n0 + p < a.N) a.gx.p[(int64_t)b * a.gx.bs + (int64_t)(n0 + p) * a.gx.ps + c * a.gx.cs] = 0.f;
    }
    if (a.part_gT && tid < 16) a.part_gT[((int64_t)b * gridDim.x + tile) * 16 + tid] = 0.f;
    return;
  }
  {
    int o = base + incl - cnt;
#pragma unroll
    for (int e = 0; e < PM_MAXC3 / 256; ++e) {
      const int n = myn[e];
      if (n >= 0) s_hit[o++] = (unsigned short)((n << 10) | (tid * (PM_MAXC3 / 256) + e));
    }
  }
  __syncthreads();

  // ---- stable counting sort by point: the list is cut into 8 segments (multiples of 4 entries, read 4 at a time);
  // group q of 32 lanes owns segment q, its lane p counts, then places, the hits of point p
  const int grp = tid >> 5, gl = tid & 31;
  const int seg = 4 * ((L + 4 * PM_BSEG - 1) / (4 * PM_BSEG));
  const int s0 = grp * seg < L ? grp * seg : L;
  const int s1 = s0 + seg < L ? s0 + seg : L;
  {
    int k = 0;
    for (int j = s0; j < s1; j += 4) {
      const uint2 v = *reinterpret_cast<const uint2*>(s_hit + j);
      const int e[4] = {(int)(v.x & 0xffffu), (int)(v.x >> 16), (int)(v.y & 0xffffu), (int)(v.y >> 16)};
#pragma unroll
      for (int t = 0; t < 4; ++t) k += (j + t < s1 && (e[t] >> 10) == gl) ? 1 : 0;
    }
    s_cnt[grp * PM_BTP + gl] = k;
  }
  __syncthreads();
  int p_tot = 0, p_start;   // of point gl: its hits in the tile, its offset in the sorted list
  {
    int before = 0;         // hits of point gl in the segments in front of this group's
#pragma unroll
    for (int q = 0; q < PM_BSEG; ++q) {
      const int v = s_cnt[q * PM_BTP + gl];
      if (q < grp) before += v;
      p_tot += v;
    }
    int inc = p_tot;      // wave_incl_scan<32>'s statements, kept in place
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) {
      const int v = __shfl_up(inc, o, 32);
      if (gl >= o) inc += v;
    }
    p_start = inc - p_tot;
    if (grp == 0) {
      s_start[gl] = p_start;
      if (gl == 31) s_start[32] = inc;
    }
    int o = p_start + before;
    for (int j = s0; j < s1; j += 4) {
      const uint2 v = *reinterpret_cast<const uint2*>(s_hit + j);
      const int e[4] = {(int)(v.x & 0xffffu), (int)(v.x >> 16), (int)(v.y & 0xffffu), (int)(v.y >> 16)};
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (j + t < s1 && (e[t] >> 10) == gl) s_sorted[o++] = (unsigned short)e[t];
    }
  }
  __syncthreads();

  // ---- A2. point p belongs to wave floor(4 * start[p] / L); a wave's points are consecutive in the sorted list
  {
    int owner = 0;
#pragma unroll
    for (int q = 1; q < 4; ++q) owner += (p_start * 4 >= q * L) ? 1 : 0;
    // (both halves of a wave hold the same per-point values: the low word is the mask of this wave's points)
    const uint32_t mine = (uint32_t)__builtin_amdgcn_ballot_w64(p_tot > 0 && owner == wave);
    if (mine != 0u) {
      int i = __builtin_amdgcn_readfirstlane(s_start[__builtin_ctz(mine)]);
      const int end = __builtin_amdgcn_readfirstlane(s_start[32 - __builtin_clz(mine)]);
      float2 acc = make_float2(0.f, 0.f);
      int cur = -1;
      while (i < end) {   // chunks of up to 64 entries: lane s fetches entry i + s and its gradient
        const int nb = end - i < 64 ? end - i : 64;
        const int my_e = s_sorted[i + (lane < nb ? lane : nb - 1)];
        const int my_g = __builtin_bit_cast(int, s_g[my_e & (PM_MAXC3 - 1)]);
        int u = 0;
        for (; u + PM_BFLY <= nb; u += PM_BFLY) pm_bwd_rows<PM_BFLY, false>(a.W3, my_e, my_g, s_m2, g2s, u, nb, lane, acc, cur);
        if (u + 16 <= nb) {
          pm_bwd_rows<16, false>(a.W3, my_e, my_g, s_m2, g2s, u, nb, lane, acc, cur);
          u += 16;
        }
        if (u + 8 <= nb) {
          pm_bwd_rows<8, false>(a.W3, my_e, my_g, s_m2, g2s, u, nb, lane, acc, cur);
          u += 8;
        }
        for (; u < nb; u += 4) pm_bwd_rows<4, true>(a.W3, my_e, my_g, s_m2, g2s, u, nb, lane, acc, cur);
        i += nb;
      }
      pm_bwd_put_row<false>(s_m2, g2s, cur, lane, acc);
    }
  }
  __syncthreads();   // also: the sort's counters in h1s are dead

  // ---- C. g1[pt][j] = sum_k2 g2[pt][k2] W2[k2][j] on MFMA: wave = (j block wave&1, K half wave>>1)
  pm_bwd_phase_c(w2tr, g2s, h1s, s_m1, wave, r, h);
  __syncthreads();

  // ---- D. g'[p][c] = sum_j W1[j][c] g1[p][j]  (gradient wrt the tower input x' = x @ T)
  float* gp = xs;  // [3][32] scratch
  if (wave < 3 && lane < PM_BTP) {   // wave = coordinate c, lane = point
    const int p = lane, c = wave;
    float sa = 0.f, sb = 0.f;
#pragma unroll
    for (int j = 0; j < PM_C1; j += 4) {
      const float4 hv = *reinterpret_cast<const float4*>(h1s + p * PM_LD1 + j);
      sa = __builtin_fmaf(s_W1[j * 3 + c], hv.x, sa);
      sb = __builtin_fmaf(s_W1[(j + 1) * 3 + c], hv.y, sb);
      sa = __builtin_fmaf(s_W1[(j + 2) * 3 + c], hv.z, sa);
      sb = __builtin_fmaf(s_W1[(j + 3) * 3 + c], hv.w, sb);
    }
    gp[c * PM_BTP + p] = sa + sb;
  }
  __syncthreads();
  if (wave == 0) {  // lanes 0..31 = the tile's points; lanes 32..63 contribute zeros to the reductions
    const int p = lane & (PM_BTP - 1);
    const bool live = lane < PM_BTP;
    const float g0 = live ? gp[p] : 0.f, g1v = live ? gp[PM_BTP + p] : 0.f, g2v = live ? gp[2 * PM_BTP + p] : 0.f;
    float o0 = g0, o1 = g1v, o2 = g2v;
    if (a.T) {
      // x' = x @ T  =>  dL/dx[c] = sum_c' g'[c'] T[c][c'] ;  dL/dT[c][c'] = sum_p x[p][c] g'[p][c']
      // (the chain starts from +0, so a dead point, g' = +0, gets +0 and not -0 under a row of negative T entries)
      const float* t = s_T;
      o0 = __builtin_fmaf(g2v, t[2], __builtin_fmaf(g1v, t[1], __builtin_fmaf(g0, t[0], 0.f)));
      o1 = __builtin_fmaf(g2v, t[5], __builtin_fmaf(g1v, t[4], __builtin_fmaf(g0, t[3], 0.f)));
      o2 = __builtin_fmaf(g2v, t[8], __builtin_fmaf(g1v, t[7], __builtin_fmaf(g0, t[6], 0.f)));
      if (a.part_gT) {
        float xr[3] = {0.f, 0.f, 0.f};
        if (live) xr[0] = s_x[p], xr[1] = s_x[PM_BTP + p], xr[2] = s_x[2 * PM_BTP + p];   // zeros past N
        const float gv[3] = {g0, g1v, g2v};
        // nine wave_sum butterflies (the same additions, in the same order, each), stepped together so that their
        // cross-lane round trips overlap; lane j keeps sum j and lanes 0..15 store the tile's 16 words at once
        float sum[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) sum[j] = xr[j / 3] * gv[j % 3];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          float other[9];
#pragma unroll
          for (int j = 0; j < 9; ++j) other[j] = __shfl_xor(sum[j], o, 64);
#pragma unroll
          for (int j = 0; j < 9; ++j) sum[j] += other[j];
        }
        float mine = 0.f;
#pragma unroll
        for (int j = 0; j < 9; ++j) mine = (lane == j) ? sum[j] : mine;
        if (lane < 16) a.part_gT[((int64_t)b * gridDim.x + tile) * 16 + lane] = mine;
      }
    }
    if (UPD) {
      if (live && n0 + p < a.N)
        pm_bwd_update_point(u, s_u, a.N, b, n0 + p, p, s_gxo[p] + o0, s_gxo[PM_BTP + p] + o1, s_gxo[2 * PM_BTP + p] + o2);
    } else if (live && n0 + p < a.N) {
      float* q = a.gx.p + (int64_t)b * a.gx.bs + (int64_t)(n0 + p) * a.gx.ps;
      if (a.accumulate) {
        q[0] = s_gxo[p] + o0, q[a.gx.cs] = s_gxo[PM_BTP + p] + o1, q[2 * a.gx.cs] = s_gxo[2 * PM_BTP + p] + o2;
      } else {
        q[0] = o0, q[a.gx.cs] = o1, q[2 * a.gx.cs] = o2;
      }
    }
  }
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void pointmlp3_max_bwd_kernel(PMBwdArgs a) {
  pm_bwd_body<false>(a, PMUpdArgs{});
}
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void pointmlp3_max_bwd_update_kernel(PMBwdArgs a,
                                                                                                                   PMUpdArgs u) {
  pm_bwd_body<true>(a, u);
}

// The packed form. A workgroup owns PM_PTP = 128 consecutive points of one cloud (8 waves; one workgroup per CU at
// B = 32, N = 1024), so argidx / g are classified and the W2 operand is fetched once per 128 points instead of once per
// 32, and phase C multiplies LIVE rows only: a point with at least one hit gets a row slot — its rank among the
// tile's live points in ascending point order — and g2s / h1s hold slots, not points. MFMA rows are independent, so a
// live row's g1 has the bits it has in pm_bwd_body; a dead point's g' is +0 there (a zero g2 row gives +0
// accumulators, and the W1 chains start from +0) and is set to +0 here. The hits (g == 0 dropped), a point's chain,
// the masks and phase D are pm_bwd_body's; the eight waves share out whole points by position in the sorted list, as its
// four do. Only the sort is another one: the stable counting sort, carried over with 4 segments x 128 bins, was the
// longest phase (6.3 of 19.7 us: a thread walks a quarter of a list four times as long), so the list ordered by
// (point, channel) is read off a [128][1024]-bit map instead (2.3 us) — same list, entry = (slot << 17 | point << 10 |
// channel). From g' on the statements are pm_bwd_body's per 32-point sub-tile (wave s = sub-tile s, each point on the
// lane it has there), a sub-tile without a hit takes that kernel's early exit (its stores are exact +0; the chain
// through T starts from +0, fma(g'[0], T[c][0], +0), so that a dead point next to a live one gets +0 as well, whatever
// the signs in T), and part_gT keeps one 16-word record per 32 points.
// STOP: 0, or the phase after which the launch ends (tools/bench_pointmlp.py's phase table; production is STOP = 0).
constexpr int PM_PTP = 128;                  // points per workgroup
constexpr int PM_PNT = 512;                  // threads per workgroup
constexpr int PM_PTQ = PM_PNT / PM_PTP;      // threads per point of the sort (each a quarter of the point's bitmap row)
constexpr int PM_PSUB = PM_PTP / PM_BTP;     // 32-point sub-tiles

// end of a truncated launch (timing only, outputs are not written): a store behind a test of what the phases left in
// LDS keeps them from being dropped as dead code
__device__ __forceinline__ void pm_bwdp_stop(const PMBwdArgs& a, const float* lds_word) {
  if (threadIdx.x == 0 && __builtin_bit_cast(uint32_t, *lds_word) == 0x7fc12345u) a.gx.p[(int64_t)blockIdx.y * a.gx.bs] = 0.f;
}

// RAGGED (UPD = false, STOP = 0 only): lengths [B] is given and cloud b ends at nb = clamp(lengths[b], 1, N): x, mask1 and
// mask2 are read below nb only, a hit at or beyond nb is dropped, gx rows in [nb, N) are written 0 (accumulate: left
// alone) and their sub-tile records are zero. A workgroup at or beyond nb writes those zeros and scans nothing.
template <bool UPD, int STOP, bool RAGGED = false>
__device__ __forceinline__ void pm_bwdp_body(const PMBwdArgs& a, const PMUpdArgs& u, const int32_t* lengths = nullptr) {
  static_assert(!RAGGED || (!UPD && STOP == 0), "the ragged twin is the production packed form only");
  constexpr int TP = PM_PTP, NT = PM_PNT, NW = PM_PNT / 64, CPT = PM_MAXC3 / PM_PNT;
  __shared__ __attribute__((aligned(16))) float g2s[TP * PM_LD2];   // [slot][132]  67.6 KB: every point may be live
  __shared__ __attribute__((aligned(16))) float h1s[TP * PM_LD1];   // [slot][68]   g1; before that the sort's counters
  __shared__ float s_g[PM_MAXC3];
  __shared__ uint32_t s_sorted[PM_MAXC3];      // (slot << 17 | point << 10 | channel), by (point, channel)
  __shared__ uint32_t s_m2[TP][4];
  __shared__ uint64_t s_m1[TP], s_m1r[TP];     // layer-1 masks by point, and by row slot
  __shared__ unsigned char s_pt[TP];           // point of a row slot
  __shared__ float s_W1[PM_C1 * 3];
  __shared__ float s_x[3 * TP], s_gxo[3 * TP], s_gp[3 * TP], s_T[12];
  __shared__ int s_scan[NW], s_live[NW], s_wbeg[NW], s_wend[NW];
  __shared__ float s_u[UPD ? 5 * 3 * TP + 4 : 1];
  uint32_t* s_bits = reinterpret_cast<uint32_t*>(h1s);            // [128][32] bit c of row p: channel c hits point p
  int* s_start = reinterpret_cast<int*>(s_bits + TP * (PM_MAXC3 / 32));   // [129] offset of point p in the sorted list
  static_assert(PM_MAXC3 <= 1024 && PM_PTP <= 128, "a sorted entry is slot << 17 | point << 10 | channel, a key slot << 7 | point");
  static_assert(CPT * PM_PNT == PM_MAXC3 && 3 * PM_PTP + 9 <= PM_PNT, "thread shares of the entry loads");
  static_assert(PM_PTQ == 4 && PM_MAXC3 / 32 == 8 * PM_PTQ, "four threads per bitmap row, eight words (two uint4) each");
  static_assert(TP * (PM_MAXC3 / 32) + TP + 1 <= TP * PM_LD1, "bitmap and offsets alias h1s");
  const int tile = blockIdx.x, b = blockIdx.y;
  const int n0 = tile * TP;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int pp = tid & (TP - 1), pc = tid >> 7;   // tid < 3 * TP: (point, coordinate) of the per-point operands
  int nb = a.N;              // the cloud's points
  if constexpr (RAGGED) {
    nb = pm_ragged_len(lengths, b, a.N);
    if (n0 >= nb) {          // (uniform) ahead of the first barrier
      if (tid < 3 * TP && !a.accumulate && n0 + pp < a.N)
        a.gx.p[(int64_t)b * a.gx.bs + (int64_t)(n0 + pp) * a.gx.ps + pc * a.gx.cs] = 0.f;
      if (a.part_gT && wave < PM_PSUB && n0 + PM_BTP * wave < a.N && lane < 16)
        a.part_gT[((int64_t)b * ((a.N + PM_BTP - 1) / PM_BTP) + tile * PM_PSUB + wave) * 16 + lane] = 0.f;
      return;
    }
  }

  // ---- entry: every load that depends on nothing, smallest first (as pm_bwd_body)
  float ld_u[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  if (UPD) {
    if (tid < 3 * TP) {
      if (n0 + pp < a.N) {
        const int64_t off = (int64_t)b * u.adv.bs + (int64_t)(n0 + pp) * u.adv.ps + pc * u.adv.cs;
        const float* ob = u.ori.p + (int64_t)b * u.ori.bs + pc * u.ori.cs;
        const int j = (u.dist_kind == 2) ? u.nn_idx[(int64_t)b * a.N + n0 + pp] : 0;
        ld_u[0] = u.adv.p[off];
        ld_u[1] = ob[(int64_t)(n0 + pp) * u.ori.ps];
        ld_u[2] = u.m[off];
        ld_u[3] = u.v[off];
        if (u.dist_kind == 2) ld_u[4] = ob[(int64_t)j * u.ori.ps];
      }
    } else if (tid < 3 * TP + 4) {
      const int e = tid - 3 * TP;
      if (e == 0) ld_u[0] = u.w ? u.w[b] : 0.f;
      else if (e == 1) ld_u[0] = u.dist_val ? u.dist_val[b] : 0.f;
      else ld_u[0] = u.adam[e - 2];
    }
  }
  int ld_n[CPT];
  float ld_g[CPT];
#pragma unroll
  for (int e = 0; e < CPT; ++e) {
    const int c = tid * CPT + e;
    ld_n[e] = (c < a.C3) ? a.argidx[(int64_t)b * a.C3 + c] : -1;
    ld_g[e] = (c < a.C3) ? a.g[(int64_t)b * a.C3 + c] : 0.f;
  }
  uint32_t ld_m2 = 0u;
  uint64_t ld_m1 = 0ull;
  if (n0 + (tid >> 2) < nb) ld_m2 = a.mask2[((int64_t)b * a.N + n0) * 4 + tid];
  if (tid < TP && n0 + tid < nb) ld_m1 = a.mask1[(int64_t)b * a.N + n0 + tid];
  const bool want_gT = a.T != nullptr && a.part_gT != nullptr;
  float ld_w1 = 0.f, ld_px = 0.f, ld_t = 0.f;
  if (tid < PM_C1 * 3) ld_w1 = a.W1[tid];
  if (tid < 3 * TP) {
    if (n0 + pp < nb) {
      if (want_gT) ld_px = a.x.p[(int64_t)b * a.x.bs + (int64_t)(n0 + pp) * a.x.ps + pc * a.x.cs];
      if (a.accumulate) ld_t = a.gx.p[(int64_t)b * a.gx.bs + (int64_t)(n0 + pp) * a.gx.ps + pc * a.gx.cs];
    }
  } else if (tid < 3 * TP + 9 && a.T) {
    ld_t = a.T[(int64_t)b * 9 + tid - 3 * TP];
  }
  // MFMA B operand of phase C, once per 128 points: waves w and w + 4 hold the same (j block w&1, K half (w&3)>>1)
  const int cw = wave & 3;
  float4 w2tr[PM_C2 / 16];
  {
    const float* wcol = a.W2 + (64 * (cw >> 1) + 4 * h) * PM_C1 + 32 * (cw & 1) + r;
#pragma unroll
    for (int t = 0; t < PM_C2 / 16; ++t) {
      w2tr[t].x = wcol[(8 * t + 0) * PM_C1];
      w2tr[t].y = wcol[(8 * t + 1) * PM_C1];
      w2tr[t].z = wcol[(8 * t + 2) * PM_C1];
      w2tr[t].w = wcol[(8 * t + 3) * PM_C1];
    }
  }

  // ---- A1. classify 2 consecutive channels per thread. The sort by (point, channel) goes through a bitmap: a hit
  // sets bit `channel` of row `point` (an atomic OR: the result does not depend on the order), and reading the rows in
  // order gives every point's channels ascending. Thread t owns words 8t..8t+7: quarter t & 3 of the row of point t >> 2.
  reinterpret_cast<uint4*>(s_bits)[2 * tid] = make_uint4(0u, 0u, 0u, 0u);
  reinterpret_cast<uint4*>(s_bits)[2 * tid + 1] = make_uint4(0u, 0u, 0u, 0u);
  int myn[CPT];
#pragma unroll
  for (int e = 0; e < CPT; ++e) {
    const int c = tid * CPT + e;
    int n = -1;
    if (c < a.C3) {
      n = ld_n[e] - n0;
      const float gv = ld_g[e];
      if (n < 0 || n >= TP || gv == 0.f) n = -1;
      if constexpr (RAGGED) n = n0 + n < nb ? n : -1;
      s_g[c] = gv;
    }
    myn[e] = n;
  }
  s_m2[tid >> 2][tid & 3] = ld_m2;
  if (tid < TP) s_m1[tid] = ld_m1;
  if (tid < PM_C1 * 3) s_W1[tid] = ld_w1;
  if (tid < 3 * TP) {
    s_x[tid] = ld_px;
    s_gxo[tid] = ld_t;
    s_gp[tid] = 0.f;   // g' of a point without a hit
  } else if (tid < 3 * TP + 9) {
    s_T[tid - 3 * TP] = ld_t;
  }
  if (tid < NW) s_wbeg[tid] = PM_MAXC3, s_wend[tid] = 0;
  if (UPD) {
    if (tid < 3 * TP) {
#pragma unroll
      for (int e = 0; e < 5; ++e) s_u[e * 3 * TP + tid] = ld_u[e];
    } else if (tid < 3 * TP + 4) {
      s_u[5 * 3 * TP + tid - 3 * TP] = ld_u[0];
    }
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < CPT; ++e) {
    const int c = tid * CPT + e;
    if (myn[e] >= 0) atomicOr(&s_bits[myn[e] * (PM_MAXC3 / 32) + (c >> 5)], 1u << (c & 31));
  }
  __syncthreads();
  uint32_t wd[8];   // this thread's eight words
  {
    const uint4 wa = reinterpret_cast<const uint4*>(s_bits)[2 * tid], wb = reinterpret_cast<const uint4*>(s_bits)[2 * tid + 1];
    wd[0] = wa.x, wd[1] = wa.y, wd[2] = wa.z, wd[3] = wa.w, wd[4] = wb.x, wd[5] = wb.y, wd[6] = wb.z, wd[7] = wb.w;
  }
  int cnt = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) cnt += __builtin_popcount(wd[k]);
  int incl = cnt;   // the sorted list in thread order: an inclusive scan of the counts gives every thread its offset
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(incl, o, 64);
    if (lane >= o) incl += v;
  }
  int p_tot = cnt;  // hits of the point, in all four of its lanes
  p_tot += __shfl_xor(p_tot, 1, 64);
  p_tot += __shfl_xor(p_tot, 2, 64);
  // live points of this wave (one bit per point, at its first lane); a point's row slot = live points in front of it
  const uint64_t lv = __builtin_amdgcn_ballot_w64(p_tot > 0 && (lane & 3) == 0);
  if (lane == 63) s_scan[wave] = incl, s_live[wave] = __builtin_popcountll(lv);
  __syncthreads();
  int base = 0, L = 0, slot = __builtin_popcountll(lv & ((1ull << (lane & ~3)) - 1ull)), nlive = 0;
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    const int v = s_scan[w], q = s_live[w];
    if (w < wave) base += v, slot += q;
    L += v;
    nlive += q;
  }
  int subL = 0;   // waves 0..3: hits in sub-tile `wave`
  if (L > 0) {
    if (STOP == 1) return pm_bwdp_stop(a, reinterpret_cast<const float*>(s_scan));
    {
      const int pt = tid >> 2;
      int o = base + incl - cnt;
      const int p_start = __shfl(o, lane & ~3, 64);
      if ((lane & 3) == 0) {
        s_start[pt] = p_start;
        if (tid == 0) s_start[TP] = L;
        if (p_tot > 0) {
          s_pt[slot] = (unsigned char)pt;
          s_m1r[slot] = s_m1[pt];
          // A2: point p belongs to wave floor(8 * start[p] / L); a wave's points are consecutive in the sorted list
          int owner = 0;
#pragma unroll
          for (int q = 1; q < NW; ++q) owner += (p_start * NW >= q * L) ? 1 : 0;
          atomicMin(&s_wbeg[owner], p_start);
          atomicMax(&s_wend[owner], p_start + p_tot);
        }
      }
      const uint32_t key = ((uint32_t)slot << 17) | ((uint32_t)pt << 10) | (uint32_t)(256 * (tid & 3));
#pragma unroll
      for (int k = 0; k < 8; ++k)
        for (uint32_t wv = wd[k]; wv != 0u; wv &= wv - 1u) s_sorted[o++] = key | (uint32_t)(32 * k + __builtin_ctz(wv));
    }
    __syncthreads();
    if (wave < PM_PSUB) subL = s_start[PM_BTP * (wave + 1)] - s_start[PM_BTP * wave];
    if (STOP == 2) return pm_bwdp_stop(a, reinterpret_cast<const float*>(s_sorted));
    const int nblk = (nlive + 31) >> 5;
    for (int i = nlive * PM_LD2 + tid; i < nblk * 32 * PM_LD2; i += NT) g2s[i] = 0.f;   // the last block's spare rows

    // ---- the gather: pm_bwd_body's walk over this wave's points
    {
      int i = __builtin_amdgcn_readfirstlane(s_wbeg[wave]);
      const int end = __builtin_amdgcn_readfirstlane(s_wend[wave]);
      if (i < end) {
        float2 acc = make_float2(0.f, 0.f);
        int cur = -1;
        while (i < end) {
          const int nb = end - i < 64 ? end - i : 64;
          const int my_e = (int)s_sorted[i + (lane < nb ? lane : nb - 1)];
          const int my_g = __builtin_bit_cast(int, s_g[my_e & (PM_MAXC3 - 1)]);
          int q = 0;
          for (; q + PM_BFLY <= nb; q += PM_BFLY) pm_bwd_rows<PM_BFLY, false, true>(a.W3, my_e, my_g, s_m2, g2s, q, nb, lane, acc, cur);
          if (q + 16 <= nb) {
            pm_bwd_rows<16, false, true>(a.W3, my_e, my_g, s_m2, g2s, q, nb, lane, acc, cur);
            q += 16;
          }
          if (q + 8 <= nb) {
            pm_bwd_rows<8, false, true>(a.W3, my_e, my_g, s_m2, g2s, q, nb, lane, acc, cur);
            q += 8;
          }
          for (; q < nb; q += 4) pm_bwd_rows<4, true, true>(a.W3, my_e, my_g, s_m2, g2s, q, nb, lane, acc, cur);
          i += nb;
        }
        pm_bwd_put_row<true>(s_m2, g2s, cur, lane, acc);
      }
    }
    __syncthreads();   // also: the sort's counters in h1s are dead
    if (STOP == 3) return pm_bwdp_stop(a, g2s);

    // ---- C. ceil(live / 32) row blocks, two at a time: waves 0..3 take block 2i, waves 4..7 block 2i + 1
    for (int i = 0; 2 * i < nblk; ++i) {
      const int rb = 2 * i + (wave >> 2);
      pm_bwd_phase_c(w2tr, g2s + rb * 32 * PM_LD2, h1s + rb * 32 * PM_LD1, s_m1r + rb * 32, cw, r, h, rb < nblk);
      __syncthreads();
    }
    if (STOP == 4) return pm_bwdp_stop(a, h1s);

    // ---- D. g' of the live rows, placed at the point's position (thread = (coordinate, row slot))
    if (tid < 3 * TP && pp < nlive) {
      const int c = pc;
      float sa = 0.f, sb = 0.f;
#pragma unroll
      for (int j = 0; j < PM_C1; j += 4) {
        const float4 hv = *reinterpret_cast<const float4*>(h1s + pp * PM_LD1 + j);
        sa = __builtin_fmaf(s_W1[j * 3 + c], hv.x, sa);
        sb = __builtin_fmaf(s_W1[(j + 1) * 3 + c], hv.y, sb);
        sa = __builtin_fmaf(s_W1[(j + 2) * 3 + c], hv.z, sa);
        sb = __builtin_fmaf(s_W1[(j + 3) * 3 + c], hv.w, sb);
      }
      s_gp[c * TP + s_pt[pp]] = sa + sb;
    }
    __syncthreads();
    if (STOP == 5) return pm_bwdp_stop(a, s_gp);
  }

  // ---- the chain through T, the dT partial and the stores, per 32-point sub-tile as pm_bwd_body has them
  const int ns = n0 + PM_BTP * wave;   // first point of this wave's sub-tile
  if (wave >= PM_PSUB || ns >= a.N) return;
  const int64_t rec = ((int64_t)b * ((a.N + PM_BTP - 1) / PM_BTP) + tile * PM_PSUB + wave) * 16;
  const int p = lane & (PM_BTP - 1);
  const int q = PM_BTP * wave + p;     // the point's index in the workgroup's tile
  const bool live = lane < PM_BTP;
  if (subL == 0) {   // no critical point in this sub-tile: gradient is exactly zero
    if (UPD && live && ns + p < a.N)
      pm_bwd_update_point<TP>(u, s_u, a.N, b, ns + p, q, s_gxo[q], s_gxo[TP + q], s_gxo[2 * TP + q]);
    if (!a.accumulate && live && ns + p < a.N) {
      float* o = a.gx.p + (int64_t)b * a.gx.bs + (int64_t)(ns + p) * a.gx.ps;
      o[0] = 0.f, o[a.gx.cs] = 0.f, o[2 * a.gx.cs] = 0.f;
    }
    if (a.part_gT && lane < 16) a.part_gT[rec + lane] = 0.f;
    return;
  }
  const float g0 = live ? s_gp[q] : 0.f, g1v = live ? s_gp[TP + q] : 0.f, g2v = live ? s_gp[2 * TP + q] : 0.f;
  float o0 = g0, o1 = g1v, o2 = g2v;
  if (a.T) {
    const float* t = s_T;
    o0 = __builtin_fmaf(g2v, t[2], __builtin_fmaf(g1v, t[1], __builtin_fmaf(g0, t[0], 0.f)));
    o1 = __builtin_fmaf(g2v, t[5], __builtin_fmaf(g1v, t[4], __builtin_fmaf(g0, t[3], 0.f)));
    o2 = __builtin_fmaf(g2v, t[8], __builtin_fmaf(g1v, t[7], __builtin_fmaf(g0, t[6], 0.f)));
    if (a.part_gT) {
      float xr[3] = {0.f, 0.f, 0.f};
      if (live) xr[0] = s_x[q], xr[1] = s_x[TP + q], xr[2] = s_x[2 * TP + q];   // zeros past N
      const float gv[3] = {g0, g1v, g2v};
      float sum[9];
#pragma unroll
      for (int j = 0; j < 9; ++j) sum[j] = xr[j / 3] * gv[j % 3];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        float other[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) other[j] = __shfl_xor(sum[j], o, 64);
#pragma unroll
        for (int j = 0; j < 9; ++j) sum[j] += other[j];
      }
      float mine = 0.f;
#pragma unroll
      for (int j = 0; j < 9; ++j) mine = (lane == j) ? sum[j] : mine;
      if (lane < 16) a.part_gT[rec + lane] = mine;
    }
  }
  if (UPD) {
    if (live && ns + p < a.N)
      pm_bwd_update_point<TP>(u, s_u, a.N, b, ns + p, q, s_gxo[q] + o0, s_gxo[TP + q] + o1, s_gxo[2 * TP + q] + o2);
  } else if (live && ns + p < a.N) {
    float* o = a.gx.p + (int64_t)b * a.gx.bs + (int64_t)(ns + p) * a.gx.ps;
    if (a.accumulate) {
      if constexpr (RAGGED) {
        if (ns + p >= nb) return;   // an accumulating launch leaves the rows beyond the length alone
      }
      o[0] = s_gxo[q] + o0, o[a.gx.cs] = s_gxo[TP + q] + o1, o[2 * a.gx.cs] = s_gxo[2 * TP + q] + o2;
    } else {
      o[0] = o0, o[a.gx.cs] = o1, o[2 * a.gx.cs] = o2;
    }
  }
}

__global__ __launch_bounds__(PM_PNT) __attribute__((amdgpu_waves_per_eu(2, 2))) void pointmlp3_max_bwd_packed_kernel(PMBwdArgs a) {
  pm_bwdp_body<false, 0>(a, PMUpdArgs{});
}
__global__ __launch_bounds__(PM_PNT) __attribute__((amdgpu_waves_per_eu(2, 2))) void pointmlp3_max_bwd_update_packed_kernel(
    PMBwdArgs a, PMUpdArgs u) {
  pm_bwdp_body<true, 0>(a, u);
}
struct PMBwdArgsR : PMBwdArgs {
  const int32_t* lengths;   // [B] (device memory, read as data)
};
__global__ __launch_bounds__(PM_PNT) __attribute__((amdgpu_waves_per_eu(2, 2))) void pointmlp3_max_bwd_packed_ragged_kernel(PMBwdArgsR a) {
  pm_bwdp_body<false, 0, true>(a, PMUpdArgs{}, a.lengths);
}
template <int STOP>
__global__ __launch_bounds__(PM_PNT) __attribute__((amdgpu_waves_per_eu(2, 2))) void pointmlp3_max_bwd_packed_dbg_kernel(PMBwdArgs a) {
  pm_bwdp_body<false, STOP>(a, PMUpdArgs{});
}

}  // namespace pc3d

using namespace pc3d;

extern "C" int pc3d_pointmlp3_tile_points(void) { return PM_TP; }
extern "C" int pc3d_pointmlp3_bwd_tile_points(void) { return PM_BTP; }

// The tower forward in every form (include/pc3d.h states the argument rules; they are checked here, before any HIP call).
// Layer 3 is screened on the matrix pipe and rechecked exactly (pointmlp_screen.hip: the same bits) at every shape this
// entry accepts; the exact kernel on request, and when no screened instantiation can be launched yet.
extern "C" int pc3d_pointmlp3_max_fwd_f32(const float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs, int B, int N,
                                          const float* T, const float* th_in, const float* th_W, const float* th_b,
                                          int th_K, float* T_out, const float* W1, const float* b1, const float* W2,
                                          const float* b2, const float* W3, const float* b3, int C1, int C2, int C3,
                                          int relu_last, float* part_val, int32_t* part_idx, float* pooled,
                                          int32_t* argidx, uint64_t* mask1, uint32_t* mask2, int form, const void* w3_bf,
                                          const float* w3_nw, const float* w3_q, const void* w3_h, const float* w3_cw,
                                          int32_t* stats, float* dbg_S, float* dbg_E, int stop_after, void* stream) {
  PC3D_REQUIRE(form >= PC3D_PM_FWD_EXACT && form <= PC3D_PM_FWD_SCREEN_H_PAIR, "pc3d_pointmlp3_max_fwd_f32: unknown form %d", form);
  PC3D_REQUIRE(th_in == nullptr || (T == nullptr && th_W && th_b && T_out && th_K >= 1),
               "pc3d_pointmlp3_max_fwd_f32: T or a complete transform head (input, weights [9,K], bias [9], T_out), not both");
  PC3D_REQUIRE(stats != nullptr || (dbg_S == nullptr && dbg_E == nullptr && stop_after == 0),
               "pc3d_pointmlp3_max_fwd_f32: dbg_S, dbg_E and stop_after belong to the debug launch, which stats [B, ntiles, 2] selects");
  PC3D_REQUIRE((dbg_S == nullptr) == (dbg_E == nullptr), "pc3d_pointmlp3_max_fwd_f32: dbg_S and dbg_E go together");
  PC3D_REQUIRE(stop_after >= 0 && stop_after <= 3, "pc3d_pointmlp3_max_fwd_f32: stop_after = %d", stop_after);
  PC3D_REQUIRE(form != PC3D_PM_FWD_EXACT || stats == nullptr, "pc3d_pointmlp3_max_fwd_f32: stats belongs to a screened form");
  PC3D_REQUIRE(form < PC3D_PM_FWD_SCREEN_PREP || (w3_bf && w3_nw && w3_q),
               "pc3d_pointmlp3_max_fwd_f32: the prepared image needs w3_bf, w3_nw and w3_q");
  PC3D_REQUIRE(form < PC3D_PM_FWD_SCREEN_H || (w3_h && w3_cw), "pc3d_pointmlp3_max_fwd_f32: both prepared images are needed");
  PC3D_REQUIRE(B >= 0 && N >= 1, "pc3d_pointmlp3_max_fwd_f32: bad sizes B=%d N=%d", B, N);
  PC3D_REQUIRE(C1 == PM_C1 && C2 == PM_C2 && C3 >= 32 && C3 % 32 == 0 && C3 <= PM_MAXC3F,
               "pc3d_pointmlp3_max_fwd_f32: unsupported widths %d/%d/%d (need 64/128/multiple of 32 <= 1024)", C1, C2, C3);
  PC3D_REQUIRE(B <= 65535, "pc3d_pointmlp3_max_fwd_f32: B=%d exceeds grid.y limit", B);
  if (B == 0) return PC3D_OK;
  PC3D_REQUIRE(x && W1 && b1 && W2 && b2 && W3 && b3 && part_val && part_idx,
               "pc3d_pointmlp3_max_fwd_f32: null pointer");
  PC3D_REQUIRE((pooled == nullptr) == (argidx == nullptr),
               "pc3d_pointmlp3_max_fwd_f32: pooled and argidx must both be given or both be NULL");
  PC3D_REQUIRE((mask1 == nullptr) == (mask2 == nullptr),
               "pc3d_pointmlp3_max_fwd_f32: mask1 and mask2 must both be given or both be NULL");
  const int ntiles = cdiv(N, PM_TP);
  PMFwdArgs a{{x, x_bs, x_ps, x_cs}, N, C3, ntiles, T, W1, b1, W2, b2, W3, b3, part_val, part_idx, mask1, mask2,
              th_in, th_W, th_b, th_K, T_out};
  hipStream_t st = as_stream(stream);
  int rc = 1;
  if (form != PC3D_PM_FWD_EXACT) {
    const PMScreenPrep q{reinterpret_cast<decltype(PMScreenPrep::w3_bf)>(w3_bf), w3_nw, reinterpret_cast<const float4*>(w3_q)};
    const PMScreenPrepH qh{reinterpret_cast<decltype(PMScreenPrepH::w3_h)>(w3_h), w3_cw, w3_nw, reinterpret_cast<const float4*>(w3_q)};
    rc = pm_fwd_screen_launch(a, B, stream, stats, dbg_S, dbg_E, stop_after, form, q, qh);
    if (rc < 0) return rc;
  }
  if (rc != 0) hipLaunchKernelGGL(pointmlp3_max_fwd_kernel<false>, dim3(ntiles, B), dim3(PM_FT), 0, st, a);
  PC3D_LAUNCH_CHECK("pc3d_pointmlp3_max_fwd_f32");
  if (pooled) {  // NULL: leave the per-tile partials unfolded (a fused consumer, or kernel-only timing)
    hipLaunchKernelGGL(pointmlp3_fold_kernel<false>, dim3(cdiv(C3, 256), B), dim3(256), 0, st, part_val, part_idx, ntiles,
                       C3, relu_last, pooled, argidx);
    PC3D_LAUNCH_CHECK("pc3d_pointmlp3_max_fwd_f32/fold");
  }
  return PC3D_OK;
}

// The forward with per-cloud lengths (include/pc3d.h: the contract and the argument rules). The exact kernel or the
// production screened one, each in its ragged instantiation; the fold launch is the dense entry's.
extern "C" int pc3d_pointmlp3_max_fwd_ragged_f32(const float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs, int B, int N,
                                                 const float* T, const float* th_in, const float* th_W, const float* th_b,
                                                 int th_K, float* T_out, const float* W1, const float* b1, const float* W2,
                                                 const float* b2, const float* W3, const float* b3, int C1, int C2, int C3,
                                                 int relu_last, float* part_val, int32_t* part_idx, float* pooled,
                                                 int32_t* argidx, uint64_t* mask1, uint32_t* mask2, int form,
                                                 const void* w3_bf, const float* w3_nw, const float* w3_q, const void* w3_h,
                                                 const float* w3_cw, int32_t* stats, float* dbg_S, float* dbg_E,
                                                 int stop_after, const int32_t* lengths, void* stream) {
  PC3D_REQUIRE(lengths != nullptr, "pc3d_pointmlp3_max_fwd_ragged_f32: lengths [B] is required");
  PC3D_REQUIRE(form == PC3D_PM_FWD_EXACT || form == PC3D_PM_FWD_SCREEN_H_PAIR,
               "pc3d_pointmlp3_max_fwd_ragged_f32: form %d has no ragged twin (PC3D_PM_FWD_EXACT or PC3D_PM_FWD_SCREEN_H_PAIR)", form);
  PC3D_REQUIRE(form != PC3D_PM_FWD_SCREEN_H_PAIR || (w3_bf && w3_nw && w3_q && w3_h && w3_cw),
               "pc3d_pointmlp3_max_fwd_ragged_f32: both prepared images are needed");
  PC3D_REQUIRE(stats == nullptr && dbg_S == nullptr && dbg_E == nullptr && stop_after == 0,
               "pc3d_pointmlp3_max_fwd_ragged_f32: stats, dbg_S, dbg_E and stop_after belong to the dense entry's debug launch");
  PC3D_REQUIRE(th_in == nullptr || (T == nullptr && th_W && th_b && T_out && th_K >= 1),
               "pc3d_pointmlp3_max_fwd_ragged_f32: T or a complete transform head (input, weights [9,K], bias [9], T_out), not both");
  PC3D_REQUIRE(B >= 0 && N >= 1, "pc3d_pointmlp3_max_fwd_ragged_f32: bad sizes B=%d N=%d", B, N);
  PC3D_REQUIRE(C1 == PM_C1 && C2 == PM_C2 && C3 >= 32 && C3 % 32 == 0 && C3 <= PM_MAXC3F,
               "pc3d_pointmlp3_max_fwd_ragged_f32: unsupported widths %d/%d/%d (need 64/128/multiple of 32 <= 1024)", C1, C2, C3);
  PC3D_REQUIRE(B <= 65535, "pc3d_pointmlp3_max_fwd_ragged_f32: B=%d exceeds grid.y limit", B);
  if (B == 0) return PC3D_OK;
  PC3D_REQUIRE(x && W1 && b1 && W2 && b2 && W3 && b3 && part_val && part_idx,
               "pc3d_pointmlp3_max_fwd_ragged_f32: null pointer");
  PC3D_REQUIRE((pooled == nullptr) == (argidx == nullptr),
               "pc3d_pointmlp3_max_fwd_ragged_f32: pooled and argidx must both be given or both be NULL");
  PC3D_REQUIRE((mask1 == nullptr) == (mask2 == nullptr),
               "pc3d_pointmlp3_max_fwd_ragged_f32: mask1 and mask2 must both be given or both be NULL");
  const int ntiles = cdiv(N, PM_TP);
  const PMFwdArgsR a{{{x, x_bs, x_ps, x_cs}, N, C3, ntiles, T, W1, b1, W2, b2, W3, b3, part_val, part_idx, mask1, mask2,
                      th_in, th_W, th_b, th_K, T_out}, lengths};
  hipStream_t st = as_stream(stream);
  int rc = 1;
  if (form != PC3D_PM_FWD_EXACT) {
    const PMScreenPrepH qh{reinterpret_cast<decltype(PMScreenPrepH::w3_h)>(w3_h), w3_cw, w3_nw, reinterpret_cast<const float4*>(w3_q)};
    rc = pm_fwd_screen_ragged_launch(a, B, stream, qh);
    if (rc < 0) return rc;
  }
  if (rc != 0) hipLaunchKernelGGL(pointmlp3_max_fwd_kernel<true>, dim3(ntiles, B), dim3(PM_FT), 0, st, a);
  PC3D_LAUNCH_CHECK("pc3d_pointmlp3_max_fwd_ragged_f32");
  if (pooled) {
    hipLaunchKernelGGL(pointmlp3_fold_kernel<false>, dim3(cdiv(C3, 256), B), dim3(256), 0, st, part_val, part_idx, ntiles,
                       C3, relu_last, pooled, argidx);
    PC3D_LAUNCH_CHECK("pc3d_pointmlp3_max_fwd_ragged_f32/fold");
  }
  return PC3D_OK;
}

extern "C" int pc3d_pointmlp3_fold_f32(const float* part_val, const int32_t* part_idx, int B, int ntiles, int C3,
                                       int relu_last, float* pooled, int32_t* argidx, int serial, void* stream) {
  PC3D_REQUIRE(B >= 0 && B <= 65535 && ntiles >= 1 && C3 >= 1, "pc3d_pointmlp3_fold_f32: bad sizes B=%d ntiles=%d C3=%d", B,
               ntiles, C3);
  if (B == 0) return PC3D_OK;
  PC3D_REQUIRE(part_val && part_idx && pooled && argidx, "pc3d_pointmlp3_fold_f32: null pointer");
  const dim3 grid(cdiv(C3, 256), B);
  if (serial)
    hipLaunchKernelGGL(pointmlp3_fold_kernel<true>, grid, dim3(256), 0, as_stream(stream), part_val, part_idx, ntiles, C3,
                       relu_last, pooled, argidx);
  else
    hipLaunchKernelGGL(pointmlp3_fold_kernel<false>, grid, dim3(256), 0, as_stream(stream), part_val, part_idx, ntiles, C3,
                       relu_last, pooled, argidx);
  PC3D_LAUNCH_CHECK("pc3d_pointmlp3_fold_f32");
  return PC3D_OK;
}

// ---- the prepared images of W3 that the SCREEN_PREP and SCREEN_H forms read (pointmlp_screen.hip)
extern "C" int pc3d_pointmlp3_w3_prepare_f32(const float* W3, int C3, void* w3_bf, float* w3_nw, float* w3_q, void* stream) {
  PC3D_REQUIRE(C3 >= 32 && C3 % 32 == 0 && C3 <= PM_MAXC3F, "pc3d_pointmlp3_w3_prepare_f32: C3 = %d (need a multiple of 32 <= 1024)", C3);
  PC3D_REQUIRE(W3 && w3_bf && w3_nw && w3_q, "pc3d_pointmlp3_w3_prepare_f32: null pointer");
  pm_w3_prepare_launch(W3, C3, w3_bf, w3_nw, w3_q, stream);
  PC3D_LAUNCH_CHECK("pc3d_pointmlp3_w3_prepare_f32");
  return PC3D_OK;
}

extern "C" int pc3d_pointmlp3_w3_prepare_h_f32(const float* W3, int C3, const float* w3_nw, void* w3_h, float* w3_cw,
                                               void* stream) {
  PC3D_REQUIRE(C3 >= 32 && C3 % 32 == 0 && C3 <= PM_MAXC3F, "pc3d_pointmlp3_w3_prepare_h_f32: C3 = %d (need a multiple of 32 <= 1024)", C3);
  PC3D_REQUIRE(W3 && w3_nw && w3_h && w3_cw, "pc3d_pointmlp3_w3_prepare_h_f32: null pointer");
  pm_w3_prepare_h_launch(W3, C3, w3_nw, w3_h, w3_cw, stream);
  PC3D_LAUNCH_CHECK("pc3d_pointmlp3_w3_prepare_h_f32");
  return PC3D_OK;
}

// 1 once the production pair instantiation can be launched on the current device (its dynamic-LDS attribute is set at
// its first use outside a capture); 0 before: a launch that asks for the pair recheck then runs the channel one
extern "C" int pc3d_pointmlp3_pair_recheck_ready(void) { return pm_fwd_pair_ready(); }

// which kernel PC3D_PM_BWD_DEFAULT launches in the two backward entries; every form stays reachable by its own value
constexpr int PM_BWD_DEFAULT_FORM = PC3D_PM_BWD_PACKED;

extern "C" int pc3d_pointmlp3_max_bwd_f32(const float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs, int B, int N,
                                          const float* T, const float* W1, const float* b1, const float* W2,
                                          const float* b2, const float* W3, const float* W2T, int C1, int C2,
                                          int C3, const int32_t* argidx, const uint64_t* mask1,
                                          const uint32_t* mask2, const float* g_pooled, float* grad_x,
                                          int64_t gx_bs, int64_t gx_ps, int64_t gx_cs, float* part_gT,
                                          int accumulate, int form, int stop_after, void* stream) {
  PC3D_REQUIRE(form >= PC3D_PM_BWD_DEFAULT && form <= PC3D_PM_BWD_TWOLIST, "pc3d_pointmlp3_max_bwd_f32: unknown form %d", form);
  PC3D_REQUIRE(stop_after >= 0 && stop_after <= 5 && (stop_after == 0 || form == PC3D_PM_BWD_PACKED),
               "pc3d_pointmlp3_max_bwd_f32: stop_after = %d (1..5, with the packed form only)", stop_after);
  PC3D_REQUIRE(B >= 0 && N >= 1, "pc3d_pointmlp3_max_bwd_f32: bad sizes B=%d N=%d", B, N);
  PC3D_REQUIRE(C1 == PM_C1 && C2 == PM_C2 && C3 >= 32 && C3 % 32 == 0 && C3 <= PM_MAXC3,
               "pc3d_pointmlp3_max_bwd_f32: unsupported widths %d/%d/%d", C1, C2, C3);
  PC3D_REQUIRE(B <= 65535, "pc3d_pointmlp3_max_bwd_f32: B=%d exceeds grid.y limit", B);
  if (B == 0) return PC3D_OK;
  PC3D_REQUIRE(x && W1 && b1 && W2 && b2 && W3 && W2T && argidx && mask1 && mask2 && g_pooled && grad_x,
               "pc3d_pointmlp3_max_bwd_f32: null pointer");
  PMBwdArgs a{{x, x_bs, x_ps, x_cs}, N, C3, T, W1, b1, W2, b2, W3, W2T, argidx, mask1, mask2, g_pooled, {grad_x, gx_bs, gx_ps, gx_cs},
              part_gT, accumulate};
  const dim3 g32(cdiv(N, PM_BTP), B), gp(cdiv(N, PM_PTP), B);
  hipStream_t st = as_stream(stream);
  switch (form == PC3D_PM_BWD_DEFAULT ? PM_BWD_DEFAULT_FORM : form) {
    case PC3D_PM_BWD_TWOLIST: hipLaunchKernelGGL(pointmlp3_max_bwd_twolist_kernel, g32, dim3(256), 0, st, a); break;
    case PC3D_PM_BWD_TILE32: hipLaunchKernelGGL(pointmlp3_max_bwd_kernel, g32, dim3(256), 0, st, a); break;
    default:
      switch (stop_after) {   // the packed form, whole or ended after phase stop_after
        case 0: hipLaunchKernelGGL(pointmlp3_max_bwd_packed_kernel, gp, dim3(PM_PNT), 0, st, a); break;
        case 1: hipLaunchKernelGGL(pointmlp3_max_bwd_packed_dbg_kernel<1>, gp, dim3(PM_PNT), 0, st, a); break;
        case 2: hipLaunchKernelGGL(pointmlp3_max_bwd_packed_dbg_kernel<2>, gp, dim3(PM_PNT), 0, st, a); break;
        case 3: hipLaunchKernelGGL(pointmlp3_max_bwd_packed_dbg_kernel<3>, gp, dim3(PM_PNT), 0, st, a); break;
        case 4: hipLaunchKernelGGL(pointmlp3_max_bwd_packed_dbg_kernel<4>, gp, dim3(PM_PNT), 0, st, a); break;
        default: hipLaunchKernelGGL(pointmlp3_max_bwd_packed_dbg_kernel<5>, gp, dim3(PM_PNT), 0, st, a); break;
      }
  }
  PC3D_LAUNCH_CHECK("pc3d_pointmlp3_max_bwd_f32");
  return PC3D_OK;
}

// The backward with per-cloud lengths: the packed form's ragged instantiation (include/pc3d.h).
extern "C" int pc3d_pointmlp3_max_bwd_ragged_f32(const float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs, int B, int N,
                                                 const float* T, const float* W1, const float* b1, const float* W2,
                                                 const float* b2, const float* W3, const float* W2T, int C1, int C2,
                                                 int C3, const int32_t* argidx, const uint64_t* mask1,
                                                 const uint32_t* mask2, const float* g_pooled, float* grad_x,
                                                 int64_t gx_bs, int64_t gx_ps, int64_t gx_cs, float* part_gT,
                                                 int accumulate, int form, int stop_after, const int32_t* lengths,
                                                 void* stream) {
  PC3D_REQUIRE(lengths != nullptr, "pc3d_pointmlp3_max_bwd_ragged_f32: lengths [B] is required");
  PC3D_REQUIRE(form == PC3D_PM_BWD_DEFAULT || form == PC3D_PM_BWD_PACKED,
               "pc3d_pointmlp3_max_bwd_ragged_f32: form %d has no ragged twin (PC3D_PM_BWD_DEFAULT or PC3D_PM_BWD_PACKED)", form);
  PC3D_REQUIRE(stop_after == 0, "pc3d_pointmlp3_max_bwd_ragged_f32: stop_after = %d belongs to the dense entry", stop_after);
  static_assert(PM_BWD_DEFAULT_FORM == PC3D_PM_BWD_PACKED, "the ragged twin is the default form's");
  PC3D_REQUIRE(B >= 0 && N >= 1, "pc3d_pointmlp3_max_bwd_ragged_f32: bad sizes B=%d N=%d", B, N);
  PC3D_REQUIRE(C1 == PM_C1 && C2 == PM_C2 && C3 >= 32 && C3 % 32 == 0 && C3 <= PM_MAXC3,
               "pc3d_pointmlp3_max_bwd_ragged_f32: unsupported widths %d/%d/%d", C1, C2, C3);
  PC3D_REQUIRE(B <= 65535, "pc3d_pointmlp3_max_bwd_ragged_f32: B=%d exceeds grid.y limit", B);
  if (B == 0) return PC3D_OK;
  PC3D_REQUIRE(x && W1 && b1 && W2 && b2 && W3 && W2T && argidx && mask1 && mask2 && g_pooled && grad_x,
               "pc3d_pointmlp3_max_bwd_ragged_f32: null pointer");
  const PMBwdArgsR a{{{x, x_bs, x_ps, x_cs}, N, C3, T, W1, b1, W2, b2, W3, W2T, argidx, mask1, mask2, g_pooled,
                      {grad_x, gx_bs, gx_ps, gx_cs}, part_gT, accumulate}, lengths};
  hipLaunchKernelGGL(pointmlp3_max_bwd_packed_ragged_kernel, dim3(cdiv(N, PM_PTP), B), dim3(PM_PNT), 0, as_stream(stream), a);
  PC3D_LAUNCH_CHECK("pc3d_pointmlp3_max_bwd_ragged_f32");
  return PC3D_OK;
}

extern "C" int pc3d_pointmlp3_max_bwd_update_f32(float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs, int B, int N,
                                                 const float* W1, const float* b1, const float* W2, const float* b2,
                                                 const float* W3, const float* W2T, int C1, int C2, int C3,
                                                 const int32_t* argidx, const uint64_t* mask1, const uint32_t* mask2,
                                                 const float* g_pooled, const float* grad_x, int64_t gx_bs,
                                                 int64_t gx_ps, int64_t gx_cs, const float* ori, int64_t o_bs,
                                                 int64_t o_ps, int64_t o_cs, float* m, float* v, double beta1,
                                                 double beta2, double eps, float budget, const float* adam,
                                                 int dist_kind, const float* w, const float* dist_val,
                                                 const int32_t* nn_idx, int form, void* stream) {
  PC3D_REQUIRE(form >= PC3D_PM_BWD_DEFAULT && form <= PC3D_PM_BWD_TILE32,
               "pc3d_pointmlp3_max_bwd_update_f32: unknown form %d (the default, the packed or the tile32 one)", form);
  PC3D_REQUIRE(B >= 0 && N >= 1, "pc3d_pointmlp3_max_bwd_update_f32: bad sizes B=%d N=%d", B, N);
  PC3D_REQUIRE(C1 == PM_C1 && C2 == PM_C2 && C3 >= 32 && C3 % 32 == 0 && C3 <= PM_MAXC3,
               "pc3d_pointmlp3_max_bwd_update_f32: unsupported widths %d/%d/%d", C1, C2, C3);
  PC3D_REQUIRE(B <= 65535, "pc3d_pointmlp3_max_bwd_update_f32: B=%d exceeds grid.y limit", B);
  PC3D_REQUIRE(dist_kind >= 0 && dist_kind <= 2, "pc3d_pointmlp3_max_bwd_update_f32: dist_kind=%d not in {0,1,2}", dist_kind);
  if (B == 0) return PC3D_OK;
  PC3D_REQUIRE(x && W1 && b1 && W2 && b2 && W3 && W2T && argidx && mask1 && mask2 && g_pooled && grad_x && ori && m && v && adam,
               "pc3d_pointmlp3_max_bwd_update_f32: null pointer");
  PC3D_REQUIRE(dist_kind == 0 || w != nullptr, "pc3d_pointmlp3_max_bwd_update_f32: distance term needs the weights w");
  PC3D_REQUIRE(dist_kind != 1 || dist_val != nullptr, "pc3d_pointmlp3_max_bwd_update_f32: L2 term needs dist_val");
  PC3D_REQUIRE(dist_kind != 2 || nn_idx != nullptr, "pc3d_pointmlp3_max_bwd_update_f32: Chamfer term needs nn_idx");
  // gx is only read here (the sum goes into the update, not back to memory)
  PMBwdArgs a{{x, x_bs, x_ps, x_cs}, N, C3, nullptr, W1, b1, W2, b2, W3, W2T, argidx, mask1, mask2, g_pooled,
              {const_cast<float*>(grad_x), gx_bs, gx_ps, gx_cs}, nullptr, 1};
  PMUpdArgs u{{x, x_bs, x_ps, x_cs}, m, v, {ori, o_bs, o_ps, o_cs}, nn_idx, w, dist_val, adam, B, dist_kind,
              (float)(1.0 - beta1), (float)(1.0 - beta2), (float)beta2, (float)eps, budget};
  if ((form == PC3D_PM_BWD_DEFAULT ? PM_BWD_DEFAULT_FORM : form) == PC3D_PM_BWD_PACKED)
    hipLaunchKernelGGL(pointmlp3_max_bwd_update_packed_kernel, dim3(cdiv(N, PM_PTP), B), dim3(PM_PNT), 0, as_stream(stream), a, u);
  else
    hipLaunchKernelGGL(pointmlp3_max_bwd_update_kernel, dim3(cdiv(N, PM_BTP), B), dim3(256), 0, as_stream(stream), a, u);
  PC3D_LAUNCH_CHECK("pc3d_pointmlp3_max_bwd_update_f32");
  return PC3D_OK;
}
