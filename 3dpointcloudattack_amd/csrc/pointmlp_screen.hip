// K8s — the PointNet tower forward (pointmlp.hip) with layer 3 SCREENED on bf16 MFMA and the survivors rechecked
// exactly. Same grid, tile, arguments and outputs as pointmlp3_max_fwd_kernel, and the same bits in every output.
//
// Layer 3 (128 -> C3) feeds a max over points: of a tile's 128 values per channel only the winner leaves the kernel.
//  screen  S[p][c] = sum_k (ah aw + ah wl + al wh) on v_mfma_f32_32x32x16_bf16 (16x the fp32 MFMA rate), where
//          xh = bf16(x), xl = bf16(x - xh): both operands split in two bf16 terms, the lo x lo product dropped. Three
//          MFMAs per k-step instead of one buy a bound 65x tighter than the single product's 2^-7: 1.0x candidates per
//          (tile, channel) instead of 4.3 (measured), and the recheck, not the screen, is what costs. A wave
//          owns WHOLE channel blocks (block = 32 channels; blocks wave, wave + 8, ...) and all 128 points: its A
//          operands come from two bf16 images of h2 in LDS (hi, lo), W3 rows are read in fp32 once
//          per workgroup and converted in registers, so the cross-point max never leaves the wave.
//  bound   |v - S| <= E = PMS_C na[p] nw[c]  (pointmlp_screen_bound.h; Cauchy-Schwarz form: one norm per point, made
//          once per tile, one per channel, made from the fp32 row the lane holds anyway).
//  select  L = max_p (S - E) over the tile's valid points; candidates are the points with S + E >= L. They contain
//          the exact arg-max and every exact tie with it.
//  recheck one lane per candidate runs the exact kernel's fmaf chain (h2 from LDS, the fp32 W3 row from L2) and
//          enters (value, lowest point) into the channel's 64-bit key with an LDS max: order-free, so deterministic.
//  fallback (wave-uniform) the exact fp32 MFMA block on the same h2: a tile with a non-finite or huge h2, a channel
//          block with a non-finite or huge W3 row, a block with more than PMS_CAP candidates.
//
// PREP: the same launch fed from a PREPARED image of W3 (pms_w3_prepare_kernel, made once per fold: W3 is a frozen victim
// weight). Same S, E, candidates and outputs in every bit; what differs is where the operands come from and how the
// recheck is laid out:
//  w3_bf [C3/32][8][2][64] x 16 B  the screen's B operands as the MFMA reads them: for channel block cb, k-step t, lane
//          (r, h) = r + 32 h, the 8 hi terms ([..][0][lane]) and the 8 lo terms ([..][1][lane]) of
//          W3[32 cb + r][16 t + 8 h + 0..7]; one wave load of 16 B per lane reads 1 KB contiguous. The screen loop streams
//          them through a ring of four k-steps that runs on across the block boundary: no fp32 row buffer, no split.
//  w3_nw [C3]  pms_norm_up of the row's sum of squares, accumulated in the in-launch order (so cw and E keep their bits).
//  w3_q  [32][C3] float4  w3_q[t][c] = W3[c][4t .. 4t+3]: the recheck goes BY CHANNEL (lane <-> channel, its fp32 row in
//          registers from two contiguous 512-B runs per load), over the channel's candidates in s_pts[c][PMS_PCAP]; the
//          winner's key stays in registers: no list, no scan, no LDS atomics, no decode pass. A block in which a channel
//          has more than PMS_PCAP candidates runs the exact block.
//
// H (further down): PREP with ONE fp16 product per k-step in place of the three bf16 ones, operands scaled by powers of
// two into fp16's range; a bound eight times wider, sixteen slots per channel, the same recheck and the same bits.
// H with PAIR: the recheck goes by (channel, candidate) pair instead, one lane each, over a per-wave list in LDS, and a
// channel's pairs meet in its 64-bit LDS key as in the in-launch form; the same bits.
#include "pc3d_common.h"
#include "pointmlp_body.h"
#include "pointmlp_screen_bound.h"
#include "pointmlp_screen_h_bound.h"

namespace pc3d {

using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;

constexpr int PMS_CAP = 128;                               // candidates per (tile, channel block) before it falls back
constexpr int PMS_SLOTS = PM_MAXC3F / 32 / (PM_FT / 64);   // channel blocks per wave (4)
constexpr int PMS_WLIST = PMS_SLOTS * PMS_CAP;             // list entries per wave
constexpr int PMS_LDA = PM_C2 + 8;                         // bf16 row stride: +16 B keeps ds_read_b128 conflict-free
// dynamic LDS: h2 + xs (69,120 B) | na [128] f32 | key [1024] u64 | lists [8][512] u16 | bf16 h2 hi, lo [2][128][136]
// = 155,648 B
constexpr size_t PMS_LDS_BYTES = (size_t)PM_FWD_LDS_FLOATS * 4 + PM_TP * 4 + (size_t)PM_MAXC3F * 8 +
                                 (PM_FT / 64) * PMS_WLIST * 2 + 2 * (size_t)PM_TP * PMS_LDA * 2;
static_assert(PMS_LDS_BYTES + 1024 <= 160 * 1024, "one workgroup's LDS on gfx950");
static_assert((PM_FWD_LDS_FLOATS * 4 + PM_TP * 4) % 8 == 0, "the keys are 8-byte aligned");
static_assert(PM_TP == 128 && PMS_SLOTS <= 4, "a list entry is slot << 12 | channel-in-block << 7 | point");

constexpr int PMS_PCAP = 8;                                // PREP: candidates per (tile, channel) before the block falls back
// PREP's dynamic LDS: h2 + xs | na [128] f32 | pts [1024][PMS_PCAP] u8 | bf16 h2 hi, lo = 147,968 B
constexpr size_t PMS_A16_OFF = (size_t)PM_FWD_LDS_FLOATS * 4 + PM_TP * 4 + (size_t)PM_MAXC3F * 8 + (PM_FT / 64) * PMS_WLIST * 2;
constexpr size_t PMS_A16_OFF_PREP = (size_t)PM_FWD_LDS_FLOATS * 4 + PM_TP * 4 + (size_t)PM_MAXC3F * PMS_PCAP;
constexpr size_t PMS_LDS_BYTES_PREP = PMS_A16_OFF_PREP + 2 * (size_t)PM_TP * PMS_LDA * 2;
static_assert(PMS_LDS_BYTES_PREP <= PMS_LDS_BYTES && PMS_A16_OFF_PREP % 16 == 0 && PMS_A16_OFF % 16 == 0, "PREP's LDS map");
static_assert(PMS_PCAP >= 4 && PMS_PCAP <= 15, "a channel's candidate count is kept in 4 bits");

struct PMScreenDbg {
  int32_t* stats;    // [B, ntiles, 2]: candidates rechecked, channel blocks that fell back (added to)
  float* dbg_S;      // [B, N, C3] or null (screened blocks only)
  float* dbg_E;
  int stop_after;    // timing only (outputs are then garbage): 1 prologue + norms, 2 + screen, 3 + select, 0 everything
};

// eight fp32 values as two bf16 terms each: xh = bf16(x), xl = bf16(x - xh) (the difference is exact in fp32)
__device__ __forceinline__ void pms_split8(const float4& lo, const float4& hi, bf16x8& oh, bf16x8& ol) {
  const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    oh[i] = (__bf16)v[i];
    ol[i] = (__bf16)(v[i] - (float)oh[i]);
  }
}

// accumulator register e of point sub-tile pt, lane half h  ->  point of the tile
__device__ __forceinline__ constexpr int pms_point(int pt, int e, int h) { return pt * 32 + (e & 3) + 8 * (e >> 2) + 4 * h; }

// L = max over the lane's points of S - E; then, given the channel's L, the 64 candidate flags (bit 16 * (pt & 1) + e of
// word pt >> 1). s_na holds +inf for the points past the end of a ragged last tile: their S - E is -inf, so they never
// raise L, and the caller clears their flags.
__device__ __forceinline__ float pms_lower(const f32x16 (&acc)[4], const float* s_na, float cw, int h) {
  float L = -__builtin_inff();
#pragma unroll
  for (int pt = 0; pt < 4; ++pt)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 na = *reinterpret_cast<const float4*>(s_na + pt * 32 + 8 * q + 4 * h);
      L = fmaxf(L, pms_lo(acc[pt][4 * q + 0], na.x, cw));
      L = fmaxf(L, pms_lo(acc[pt][4 * q + 1], na.y, cw));
      L = fmaxf(L, pms_lo(acc[pt][4 * q + 2], na.z, cw));
      L = fmaxf(L, pms_lo(acc[pt][4 * q + 3], na.w, cw));
    }
  return L;
}
__device__ __forceinline__ void pms_flags(const f32x16 (&acc)[4], const float* s_na, float cw, int h, float L,
                                          unsigned (&flags)[2]) {
#pragma unroll
  for (int wd = 0; wd < 2; ++wd) {
    unsigned f = 0u;                      // shifted in from the top bit down: no 32 mask constants held in registers
#pragma unroll
    for (int pq = 7; pq >= 0; --pq) {
      const int pt = 2 * wd + (pq >> 2), q = pq & 3;
      const float4 na = *reinterpret_cast<const float4*>(s_na + pt * 32 + 8 * q + 4 * h);
      f = (f << 1) | (pms_hi(acc[pt][4 * q + 3], na.w, cw) >= L ? 1u : 0u);
      f = (f << 1) | (pms_hi(acc[pt][4 * q + 2], na.z, cw) >= L ? 1u : 0u);
      f = (f << 1) | (pms_hi(acc[pt][4 * q + 1], na.y, cw) >= L ? 1u : 0u);
      f = (f << 1) | (pms_hi(acc[pt][4 * q + 0], na.x, cw) >= L ? 1u : 0u);
    }
    flags[wd] = f;
  }
}

// The exact kernel's layer 3 + max for ONE channel block and all four point sub-tiles, by one wave, A operands from the
// fp32 h2 in LDS: the same MFMA chain per (point, channel), the same selects in the same order, so the same bits.
__device__ __forceinline__ void pms_exact_block(const float* h2, const float* W3, const float* b3, int cb, int n0, int N,
                                             float* out_val, int32_t* out_idx) {
  const int lane = threadIdx.x & 63;
  const int r = lane & 31, h = lane >> 5;
  float4 bw[PM_C2 / 8];
  const float* wrow = W3 + (int64_t)(cb * 32 + r) * PM_C2 + 4 * h;
#pragma unroll
  for (int t = 0; t < PM_C2 / 8; ++t) bw[t] = *reinterpret_cast<const float4*>(wrow + 8 * t);
  float tbest = 0.f;
  int tbi = 0;
#pragma unroll 1
  for (int pt = 0; pt < 4; ++pt) {
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
    for (int t = 0; t < PM_C2 / 8; ++t) {
      const float4 av = *reinterpret_cast<const float4*>(h2 + (pt * 32 + r) * PM_LD2 + 8 * t + 4 * h);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bw[t].x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bw[t].y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bw[t].z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bw[t].w, acc, 0, 0, 0);
    }
    float best = -__builtin_inff();
    int be = 0;
    const int base = n0 + pt * 32;
#pragma unroll
    for (int e = 0; e < 16; ++e)      // ascending point index in e for fixed h: strict > keeps the lowest
      if (base + (e & 3) + 8 * (e >> 2) + 4 * h < N && acc[e] > best) best = acc[e], be = (e & 3) + 8 * (e >> 2);
    int bi = best == -__builtin_inff() ? base : base + be + 4 * h;
    argmax_xor32(best, bi);
    if (pt == 0 || best > tbest) tbest = best, tbi = bi;   // ascending sub-tile, strict >: the exact kernel's cross-wave max
  }
  if (h == 0) {
    out_val[cb * 32 + r] = tbest + b3[cb * 32 + r];
    out_idx[cb * 32 + r] = tbi;
  }
}

// The prepared image of W3 (see the head of the file): one wave per channel block. Lane (r, h) holds what the in-launch
// screen's lane holds and forms the norm in the same order, so w3_nw is that launch's nw in every bit.
__global__ __launch_bounds__(64) void pms_w3_prepare_kernel(const float* __restrict__ W3, bf16x8* __restrict__ w3_bf,
                                                            float* __restrict__ w3_nw, float4* __restrict__ w3_q, int C3) {
  const int cb = blockIdx.x, lane = threadIdx.x;
  const int r = lane & 31, h = lane >> 5;
  float4 w[PM_C2 / 8];
  const float* wrow = W3 + (int64_t)(cb * 32 + r) * PM_C2 + 8 * h;
  float ss = 0.f;
#pragma unroll
  for (int t = 0; t < PM_C2 / 16; ++t) {
    w[2 * t] = *reinterpret_cast<const float4*>(wrow + 16 * t);
    w[2 * t + 1] = *reinterpret_cast<const float4*>(wrow + 16 * t + 4);
  }
#pragma unroll
  for (int t = 0; t < PM_C2 / 8; ++t) {
    ss = __builtin_fmaf(w[t].x, w[t].x, ss), ss = __builtin_fmaf(w[t].y, w[t].y, ss);
    ss = __builtin_fmaf(w[t].z, w[t].z, ss), ss = __builtin_fmaf(w[t].w, w[t].w, ss);
  }
  ss = sum_xor32(ss);
  if (h == 0) w3_nw[cb * 32 + r] = pms_norm_up(ss);
#pragma unroll
  for (int t = 0; t < PM_C2 / 16; ++t) {
    bf16x8 bh, bl;
    pms_split8(w[2 * t], w[2 * t + 1], bh, bl);
    w3_bf[((cb * (PM_C2 / 16) + t) * 2 + 0) * 64 + lane] = bh;
    w3_bf[((cb * (PM_C2 / 16) + t) * 2 + 1) * 64 + lane] = bl;
  }
  for (int i = lane; i < 32 * (PM_C2 / 4); i += 64) {
    const int c = cb * 32 + (i & 31), t = i >> 5;
    w3_q[(int64_t)t * C3 + c] = *reinterpret_cast<const float4*>(W3 + (int64_t)c * PM_C2 + 4 * t);
  }
}

// DBG: stats and the truncated forms for phase timing; DUMP: dbg_S / dbg_E as well (tests of tiny shapes: it spills).
// The production kernel is <false, false> and carries none of it.
// PREP: the operands come from the prepared image w3 (the head of the file), which is not read otherwise.
template <bool DBG, bool DUMP, bool PREP>
__global__ __launch_bounds__(PM_FT) __attribute__((amdgpu_waves_per_eu(2, 2))) void pointmlp3_max_fwd_screen_kernel(
    PMFwdArgs a, PMScreenDbg d, PMScreenPrep w3) {
  extern __shared__ __attribute__((aligned(16))) float pms_lds[];
  float* h2 = pms_lds;                                                              // [128][132] fp32, kept to the end
  float* s_na = pms_lds + PM_FWD_LDS_FLOATS;                                        // [128] upper bounds of ||h2[p]||
  unsigned long long* s_key = reinterpret_cast<unsigned long long*>(s_na + PM_TP);  // [C3] (value, lowest point) keys
  unsigned short* s_list = reinterpret_cast<unsigned short*>(s_key + PM_MAXC3F);    // [8 waves][PMS_WLIST]
  __bf16* s_a16 = reinterpret_cast<__bf16*>(reinterpret_cast<char*>(pms_lds) +
                                            (PREP ? PMS_A16_OFF_PREP : PMS_A16_OFF));   // [128][PMS_LDA] bf16 image of h2: hi
  __bf16* s_a16l = s_a16 + PM_TP * PMS_LDA;                                         // and lo terms
  pm_fwd_prologue(a, pms_lds, a.N);
  const int tile = blockIdx.x, b = blockIdx.y;
  const int n0 = tile * PM_TP;
  const int nvalid = a.N - n0;            // >= 1
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int64_t obase = ((int64_t)b * a.ntiles + tile) * a.C3;

  // ---- one norm per point (4 threads per point, 32 k each, fixed order), h2's bf16 image and the keys' start value
  bool bad;
  {
    const int p = threadIdx.x >> 2, q = threadIdx.x & 3;
    const float* row = h2 + p * PM_LD2 + 32 * q;
    float ss = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const float4 v = *reinterpret_cast<const float4*>(row + 8 * t), u = *reinterpret_cast<const float4*>(row + 8 * t + 4);
      ss = __builtin_fmaf(v.x, v.x, ss), ss = __builtin_fmaf(v.y, v.y, ss);
      ss = __builtin_fmaf(v.z, v.z, ss), ss = __builtin_fmaf(v.w, v.w, ss);
      ss = __builtin_fmaf(u.x, u.x, ss), ss = __builtin_fmaf(u.y, u.y, ss);
      ss = __builtin_fmaf(u.z, u.z, ss), ss = __builtin_fmaf(u.w, u.w, ss);
      bf16x8 vh, vl;
      pms_split8(v, u, vh, vl);
      *reinterpret_cast<bf16x8*>(s_a16 + p * PMS_LDA + 32 * q + 8 * t) = vh;
      *reinterpret_cast<bf16x8*>(s_a16l + p * PMS_LDA + 32 * q + 8 * t) = vl;
    }
    ss += __shfl_xor(ss, 1, 64);
    ss += __shfl_xor(ss, 2, 64);
    const float na = pms_norm_up(ss);
    bad = !pms_norm_ok(na);               // NaN, inf or huge h2 anywhere in the tile: no screen for this tile
    if (q == 0) s_na[p] = p < nvalid ? na : __builtin_inff();   // past the end of a ragged tile: see pms_lower
    if (!PREP)
      for (int c = threadIdx.x; c < a.C3; c += PM_FT) s_key[c] = 0ull;
  }
  const bool tile_bad = __syncthreads_or(bad ? 1 : 0) != 0;
  if (DBG && d.stop_after == 1) return;

  unsigned vmask[2] = {0u, 0u};           // the lane's 64 points that exist (all of them but in a ragged last tile)
#pragma unroll
  for (int pt = 0; pt < 4; ++pt)
#pragma unroll
    for (int e = 0; e < 16; ++e) vmask[pt >> 1] |= (pms_point(pt, e, h) < nvalid) ? (1u << (16 * (pt & 1) + e)) : 0u;
  const int nblk = a.C3 / 32;
  if constexpr (PREP) {
    unsigned char* s_pts = reinterpret_cast<unsigned char*>(s_na + PM_TP);   // [C3][PMS_PCAP] a channel's candidate points
    const int nslots = wave < nblk ? (nblk - wave + PM_FT / 64 - 1) / (PM_FT / 64) : 0;   // <= PMS_SLOTS
    unsigned screened = 0u, cnts = 0u;    // bit slot: screened; bits 4 slot .. + 3: candidates of the lane's channel r
    int ncand = 0, nfall = 0;
    float sink = 0.f;
    // the B operands' ring: four k-steps ahead in the wave's stream of blocks, across the block boundary
    const bf16x8* wb = w3.w3_bf + lane;
    bf16x8 qh[4], ql[4];
    float nw_next = 0.f;
    if (nslots > 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        qh[i] = wb[((wave * (PM_C2 / 16) + i) * 2 + 0) * 64];
        ql[i] = wb[((wave * (PM_C2 / 16) + i) * 2 + 1) * 64];
      }
      nw_next = w3.w3_nw[wave * 32 + r];
    }
#pragma unroll 1
    for (int slot = 0; slot < nslots; ++slot) {
      const int cb = wave + (PM_FT / 64) * slot;
      const int nxt = slot + 1 < nslots ? cb + PM_FT / 64 : cb;   // past the wave's last block: a valid address, unused
      const float nw = nw_next;
      nw_next = w3.w3_nw[nxt * 32 + r];
      const float cw = pms_cw(nw);
      // (uniform) a non-finite or huge h2 in the tile, or such a W3 row in the block (its prepared norm fails too)
      bool fall = tile_bad || __builtin_amdgcn_ballot_w64(!pms_norm_ok(nw)) != 0ull;
      if (!fall) {
        f32x16 acc[4];
#pragma unroll
        for (int pt = 0; pt < 4; ++pt)
#pragma unroll
          for (int e = 0; e < 16; ++e) acc[pt][e] = 0.f;
#pragma unroll
        for (int t = 0; t < PM_C2 / 16; ++t) {
          const bf16x8 bh = qh[t & 3], bl = ql[t & 3];
          {
            const int cs = t < 4 ? cb : nxt, ts = (t + 4) & 7;
            qh[t & 3] = wb[((cs * (PM_C2 / 16) + ts) * 2 + 0) * 64];
            ql[t & 3] = wb[((cs * (PM_C2 / 16) + ts) * 2 + 1) * 64];
          }
#pragma unroll
          for (int pt = 0; pt < 4; ++pt) {   // A: lane (r, h) holds the terms of h2[32 pt + r][16 t + 8 h + 0..7]
            const bf16x8 ah = *reinterpret_cast<const bf16x8*>(s_a16 + (pt * 32 + r) * PMS_LDA + 16 * t + 8 * h);
            const bf16x8 al = *reinterpret_cast<const bf16x8*>(s_a16l + (pt * 32 + r) * PMS_LDA + 16 * t + 8 * h);
            acc[pt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[pt], 0, 0, 0);
            acc[pt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc[pt], 0, 0, 0);
            acc[pt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc[pt], 0, 0, 0);
          }
        }
        // the order of the 16 loads, 64 LDS reads and 96 MFMAs above, pinned (hipcc otherwise sinks the loads to just in
        // time): a k-step's two loads lead it and land four k-steps later; the A operands are read two (pt) groups ahead
        __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);        // 4 DS read
#pragma unroll
        for (int g = 0; g < 4 * (PM_C2 / 16); ++g) {
          if (g % 4 == 0) __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);   // 2 VMEM read
          __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);      // 3 MFMA
          if (g + 2 < 4 * (PM_C2 / 16)) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
        }
        if (DBG && d.stop_after == 2) {
#pragma unroll
          for (int pt = 0; pt < 4; ++pt)
#pragma unroll
            for (int e = 0; e < 16; ++e) sink += acc[pt][e];
          continue;
        }
        if (DUMP && d.dbg_S != nullptr) {
          int c3v = a.C3;
          unsigned vm[2] = {vmask[0], vmask[1]};
          asm volatile("" : "+v"(c3v), "+v"(vm[0]), "+v"(vm[1]));   // opaque: nothing of the 64 stores is hoisted out of the block loop
          const int64_t o0 = ((int64_t)b * a.N + n0) * a.C3 + cb * 32 + r;
#pragma unroll
          for (int pt = 0; pt < 4; ++pt)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
              const int p = pms_point(pt, e, h);
              if ((vm[pt >> 1] >> (16 * (pt & 1) + e)) & 1u) {
                d.dbg_S[o0 + (int64_t)p * c3v] = acc[pt][e];
                d.dbg_E[o0 + (int64_t)p * c3v] = pms_E(s_na[p], cw);
              }
            }
        }
        unsigned flags[2];
        float L = pms_lower(acc, s_na, cw, h);
        L = fmaxf(L, __shfl_xor(L, 32, 64));
        pms_flags(acc, s_na, cw, h, L, flags);
        flags[0] &= vmask[0], flags[1] &= vmask[1];
        const int cnt = __builtin_popcount(flags[0]) + __builtin_popcount(flags[1]);
        const int other = __shfl_xor(cnt, 32, 64);   // the channel's other half of the points
        if (__builtin_amdgcn_ballot_w64(cnt + other > PMS_PCAP) != 0ull) {
          fall = true;                    // (uniform) a channel with more candidates than its slots: the exact block instead
        } else {
          unsigned char* mine = s_pts + (cb * 32 + r) * PMS_PCAP + (h ? other : 0);   // h = 1 writes behind h = 0's
#pragma unroll
          for (int wd = 0; wd < 2; ++wd) {
            unsigned f = flags[wd];
            while (f) {
              const int bit = __builtin_ctz(f);
              f &= f - 1;
              *mine++ = (unsigned char)pms_point(2 * wd + (bit >> 4), bit & 15, h);
            }
          }
          cnts |= (unsigned)(cnt + other) << (4 * slot);
          screened |= 1u << slot;
          if (DBG) ncand += h ? 0 : cnt + other;
        }
      } else {                            // not screened: the ring moves on to the next block's first k-steps
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          qh[i] = wb[((nxt * (PM_C2 / 16) + i) * 2 + 0) * 64];
          ql[i] = wb[((nxt * (PM_C2 / 16) + i) * 2 + 1) * 64];
        }
      }
      if (fall) {
        pms_exact_block(h2, a.W3, a.b3, cb, n0, a.N, a.part_val + obase, a.part_idx + obase);
        ++nfall;
      }
    }
    if (DBG && d.stop_after == 2) {
      if (sink == 12345.678f) a.part_val[obase] = sink;   // keeps the products alive
      return;
    }
    if (DBG && d.stats != nullptr) {
#pragma unroll      // wave_sum's statements, kept in place like the scan below
      for (int o = 32; o > 0; o >>= 1) ncand += __shfl_xor(ncand, o, 64);
      if (lane == 0) {
        int32_t* st = d.stats + ((int64_t)b * a.ntiles + tile) * 2;
        if (ncand) atomicAdd(st, ncand);
        if (nfall) atomicAdd(st + 1, nfall);
      }
    }
    if (DBG && d.stop_after == 3) {
      if (cnts == 0xffffffffu) a.part_val[obase] = 0.f;
      return;
    }

    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // the channels' candidate points, written by other lanes
    // ---- recheck by channel: lanes 0..31 the channels of slot 2j, lanes 32..63 those of slot 2j + 1; the lane holds its
    // channel's fp32 row and runs the exact kernel's chain (t ascending; x, y, z, w; k = 8t + c, then 8t + 4 + c) for each
    // of the channel's candidates; the largest key (see the in-launch form) is the exact kernel's winner
#pragma unroll 1
    for (int j = 0; 2 * j < nslots; ++j) {
      const int sl = 2 * j + h;
      const bool live = sl < nslots && ((screened >> sl) & 1u);
      const int n = live ? (int)((cnts >> (4 * sl)) & 15u) : 0;
      if (__builtin_amdgcn_ballot_w64(n > 0) == 0ull) continue;   // (uniform)
      const int c = (wave + (PM_FT / 64) * (live ? sl : 0)) * 32 + r;   // an idle lane: a valid row, unused
      float4 wv[PM_C2 / 4];               // the whole row in flight at once: one round trip per trip
#pragma unroll
      for (int t = 0; t < PM_C2 / 4; ++t) wv[t] = w3.w3_q[(int64_t)t * a.C3 + c];
      unsigned long long key = 0ull;
#pragma unroll 1
      for (int i = 0; i < PMS_PCAP; ++i) {
        if (__builtin_amdgcn_ballot_w64(i < n) == 0ull) break;    // (uniform)
        const int p = i < n ? s_pts[c * PMS_PCAP + i] : 0;
        const float4* ar = reinterpret_cast<const float4*>(h2 + p * PM_LD2);
        float v = 0.f;
#pragma unroll
        for (int t = 0; t < PM_C2 / 8; ++t) {
          const float4 a0 = ar[2 * t], a1 = ar[2 * t + 1];
          const float4 w0 = wv[2 * t], w1 = wv[2 * t + 1];
          v = __builtin_fmaf(a0.x, w0.x, v), v = __builtin_fmaf(a1.x, w1.x, v);
          v = __builtin_fmaf(a0.y, w0.y, v), v = __builtin_fmaf(a1.y, w1.y, v);
          v = __builtin_fmaf(a0.z, w0.z, v), v = __builtin_fmaf(a1.z, w1.z, v);
          v = __builtin_fmaf(a0.w, w0.w, v), v = __builtin_fmaf(a1.w, w1.w, v);
        }
        const unsigned vb = __builtin_bit_cast(unsigned, v);
        const unsigned zb = (v == 0.f) ? 0u : vb;
        const unsigned ord = (zb & 0x80000000u) ? ~zb : (zb | 0x80000000u);
        const unsigned low = ((unsigned)(127 - p) << 1) | ((vb == 0x80000000u) ? 1u : 0u);
        const unsigned long long k = ((unsigned long long)ord << 32) | low;
        if (i < n && k > key) key = k;
      }
      if (live) {
        const unsigned ord = (unsigned)(key >> 32), low = (unsigned)key;
        unsigned vb = (ord & 0x80000000u) ? (ord & 0x7fffffffu) : ~ord;
        if (low & 1u) vb = 0x80000000u;
        a.part_val[obase + c] = __builtin_bit_cast(float, vb) + a.b3[c];
        a.part_idx[obase + c] = n0 + 127 - (int)((low >> 1) & 127u);
      }
    }
    return;
  }
  unsigned short* my_list = s_list + wave * PMS_WLIST;
  int wave_cnt = 0, nfall = 0;
  unsigned screened = 0u;                 // bit slot: that block of the wave went through the screen
  float sink = 0.f;
#pragma unroll 1
  for (int slot = 0; slot < PMS_SLOTS; ++slot) {
    const int cb = wave + (PM_FT / 64) * slot;
    if (cb >= nblk) break;                // (uniform)
    bool fall = tile_bad;
    float4 w[PM_C2 / 8];
    float cw = 0.f;
    if (!fall) {                          // the block's fp32 rows: lane (r, h) holds W3[32 cb + r][16 t + 8 h + 0..7]
      const float* wrow = a.W3 + (int64_t)(cb * 32 + r) * PM_C2 + 8 * h;
      float ss = 0.f;
#pragma unroll
      for (int t = 0; t < PM_C2 / 16; ++t) {
        w[2 * t] = *reinterpret_cast<const float4*>(wrow + 16 * t);
        w[2 * t + 1] = *reinterpret_cast<const float4*>(wrow + 16 * t + 4);
      }
#pragma unroll
      for (int t = 0; t < PM_C2 / 8; ++t) {
        ss = __builtin_fmaf(w[t].x, w[t].x, ss), ss = __builtin_fmaf(w[t].y, w[t].y, ss);
        ss = __builtin_fmaf(w[t].z, w[t].z, ss), ss = __builtin_fmaf(w[t].w, w[t].w, ss);
      }
      ss = sum_xor32(ss);
      const float nw = pms_norm_up(ss);
      cw = pms_cw(nw);
      fall = __builtin_amdgcn_ballot_w64(!pms_norm_ok(nw)) != 0ull;   // a non-finite or huge W3 row in the block
    }
    if (!fall) {
      f32x16 acc[4];
#pragma unroll
      for (int pt = 0; pt < 4; ++pt)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[pt][e] = 0.f;
#pragma unroll
      for (int t = 0; t < PM_C2 / 16; ++t) {
        bf16x8 bh, bl;
        pms_split8(w[2 * t], w[2 * t + 1], bh, bl);
#pragma unroll
        for (int pt = 0; pt < 4; ++pt) {   // A: lane (r, h) holds the terms of h2[32 pt + r][16 t + 8 h + 0..7]
          const bf16x8 ah = *reinterpret_cast<const bf16x8*>(s_a16 + (pt * 32 + r) * PMS_LDA + 16 * t + 8 * h);
          const bf16x8 al = *reinterpret_cast<const bf16x8*>(s_a16l + (pt * 32 + r) * PMS_LDA + 16 * t + 8 * h);
          acc[pt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[pt], 0, 0, 0);
          acc[pt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc[pt], 0, 0, 0);
          acc[pt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc[pt], 0, 0, 0);
        }
      }
      if (DBG && d.stop_after == 2) {
#pragma unroll
        for (int pt = 0; pt < 4; ++pt)
#pragma unroll
          for (int e = 0; e < 16; ++e) sink += acc[pt][e];
        continue;
      }
      if (DUMP && d.dbg_S != nullptr) {
        int c3v = a.C3;
        unsigned vm[2] = {vmask[0], vmask[1]};
        asm volatile("" : "+v"(c3v), "+v"(vm[0]), "+v"(vm[1]));   // opaque: nothing of the 64 stores is hoisted out of the block loop
        const int64_t o0 = ((int64_t)b * a.N + n0) * a.C3 + cb * 32 + r;
#pragma unroll
        for (int pt = 0; pt < 4; ++pt)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int p = pms_point(pt, e, h);
            if ((vm[pt >> 1] >> (16 * (pt & 1) + e)) & 1u) {
              d.dbg_S[o0 + (int64_t)p * c3v] = acc[pt][e];
              d.dbg_E[o0 + (int64_t)p * c3v] = pms_E(s_na[p], cw);
            }
          }
      }
      unsigned flags[2];
      float L = pms_lower(acc, s_na, cw, h);
      L = fmaxf(L, __shfl_xor(L, 32, 64));
      pms_flags(acc, s_na, cw, h, L, flags);
      flags[0] &= vmask[0], flags[1] &= vmask[1];
      const int cnt = __builtin_popcount(flags[0]) + __builtin_popcount(flags[1]);
      int incl = cnt;      // wave_incl_scan's statements, kept in place: the headline's forward
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
      }
      const int total = __builtin_amdgcn_readlane(incl, 63);
      if (total > PMS_CAP) {
        fall = true;                      // (uniform) more candidates than the list holds: the exact block instead
      } else {
        int off = wave_cnt + incl - cnt;  // wave_cnt + total <= PMS_WLIST: every slot adds at most PMS_CAP
#pragma unroll
        for (int wd = 0; wd < 2; ++wd) {
          unsigned f = flags[wd];
          while (f) {
            const int bit = __builtin_ctz(f);
            f &= f - 1;
            const int p = pms_point(2 * wd + (bit >> 4), bit & 15, h);
            my_list[off++] = (unsigned short)((slot << 12) | (r << 7) | p);
          }
        }
        wave_cnt += total;
        screened |= 1u << slot;
      }
    }
    if (fall) {
      pms_exact_block(h2, a.W3, a.b3, cb, n0, a.N, a.part_val + obase, a.part_idx + obase);
      ++nfall;
    }
  }
  if (DBG && d.stop_after == 2) {
    if (sink == 12345.678f) a.part_val[obase] = sink;   // keeps the products alive
    return;
  }
  if (DBG && d.stats != nullptr && lane == 0) {
    int32_t* st = d.stats + ((int64_t)b * a.ntiles + tile) * 2;
    if (wave_cnt) atomicAdd(st, wave_cnt);
    if (nfall) atomicAdd(st + 1, nfall);
  }
  if (DBG && d.stop_after == 3) {
    if (wave_cnt == 123456789) a.part_val[obase] = 0.f;
    return;
  }

  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // the wave's list entries, written by other lanes
  // ---- recheck: one lane per candidate, the exact kernel's chain (t ascending; x, y, z, w; k = 8t + c, then 8t + 4 + c)
  for (int i = lane; i < wave_cnt; i += 64) {
    const int e = my_list[i];
    const int p = e & 127, c = (wave + (PM_FT / 64) * (e >> 12)) * 32 + ((e >> 7) & 31);
    const float4* wr = reinterpret_cast<const float4*>(a.W3 + (int64_t)c * PM_C2);
    const float4* ar = reinterpret_cast<const float4*>(h2 + p * PM_LD2);
    float4 wv[PM_C2 / 4];                 // the whole row in flight at once: one round trip per pass
#pragma unroll
    for (int t = 0; t < PM_C2 / 4; ++t) wv[t] = wr[t];
    float v = 0.f;
#pragma unroll
    for (int t = 0; t < PM_C2 / 8; ++t) {
      const float4 a0 = ar[2 * t], a1 = ar[2 * t + 1];
      const float4 w0 = wv[2 * t], w1 = wv[2 * t + 1];
      v = __builtin_fmaf(a0.x, w0.x, v), v = __builtin_fmaf(a1.x, w1.x, v);
      v = __builtin_fmaf(a0.y, w0.y, v), v = __builtin_fmaf(a1.y, w1.y, v);
      v = __builtin_fmaf(a0.z, w0.z, v), v = __builtin_fmaf(a1.z, w1.z, v);
      v = __builtin_fmaf(a0.w, w0.w, v), v = __builtin_fmaf(a1.w, w1.w, v);
    }
    // key: the value as an ordered integer (both zeros as one value), then the LOWEST point, then whether it was -0:
    // the largest key is the exact kernel's winner (v is finite here: the norms' range check rules out overflow)
    const unsigned vb = __builtin_bit_cast(unsigned, v);
    const unsigned zb = (v == 0.f) ? 0u : vb;
    const unsigned ord = (zb & 0x80000000u) ? ~zb : (zb | 0x80000000u);
    const unsigned low = ((unsigned)(127 - p) << 1) | ((vb == 0x80000000u) ? 1u : 0u);
    atomicMax(&s_key[c], ((unsigned long long)ord << 32) | low);
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // only this wave touches its channels' keys
  for (int i = lane; i < 32 * PMS_SLOTS; i += 64) {
    const int slot = i >> 5;
    if (!((screened >> slot) & 1u)) continue;
    const int c = (wave + (PM_FT / 64) * slot) * 32 + (i & 31);
    const unsigned long long key = s_key[c];
    const unsigned ord = (unsigned)(key >> 32), low = (unsigned)key;
    unsigned vb = (ord & 0x80000000u) ? (ord & 0x7fffffffu) : ~ord;
    if (low & 1u) vb = 0x80000000u;
    a.part_val[obase + c] = __builtin_bit_cast(float, vb) + a.b3[c];
    a.part_idx[obase + c] = n0 + 127 - (int)((low >> 1) & 127u);
  }
}

// ---- H: the prepared form with ONE fp16 product per k-step (pointmlp_screen_h_bound.h). Same prologue, grid, tile,
// select, recheck chain, key order and exact block as PREP; what differs:
//  operands  a' = h2 2^sa, one exponent per TILE (the tile's largest na lands in [2^13, 2^14): one LDS max in the norms
//            phase), as one fp16 image in LDS; w' = W3 2^sw[c] from the prepared image w3_h (pms_w3_prepare_h_kernel).
//            Powers of two: the scaling is exact, and within a channel it moves S, E and v alike, so L, the flags and the
//            candidates are formed in the scaled domain and nothing is scaled back.
//  bound     E = s_na[p] cw, s_na[p] = na 2^sa + 1, cw = w3_cw[c] = PMH_C nw 2^sw (+inf: the channel's norm failed
//            pms_norm_ok; its block runs the exact block, like a tile with a norm that failed).
//  slots     PMH_PCAP = 16 candidates per (tile, channel): the bound is 8x the three-product one, and the LDS of the
//            second image is free.
using f16x8 = __attribute__((ext_vector_type(8))) _Float16;

constexpr int PMH_PCAP = 16;
// H's dynamic LDS: h2 + xs | na [128] f32 | the tile's largest na (16 B) | pts [1024][PMH_PCAP] u8 | fp16 h2 = 120,848 B
constexpr size_t PMH_AMAX_OFF = (size_t)PM_FWD_LDS_FLOATS * 4 + PM_TP * 4;
constexpr size_t PMH_PTS_OFF = PMH_AMAX_OFF + 16;
constexpr size_t PMH_A16_OFF = PMH_PTS_OFF + (size_t)PM_MAXC3F * PMH_PCAP;
constexpr size_t PMH_LDS_BYTES = PMH_A16_OFF + (size_t)PM_TP * PMS_LDA * 2;
static_assert(PMH_LDS_BYTES + 1024 <= 160 * 1024 && PMH_A16_OFF % 16 == 0 && PMH_PTS_OFF % 16 == 0, "H's LDS map");
static_assert(PMH_PCAP >= 4 && PMH_PCAP <= 31 && 5 * PMS_SLOTS <= 32, "a channel's candidate count is kept in 5 bits per slot");
static_assert(PM_TP <= 256, "a candidate point is one byte");
// the PAIR recheck's LDS behind H's map: keys [8 waves][128 channels] u64 | lists [8 waves][2048] u16 = 161,808 B in all
constexpr int PMP_WCH = 32 * PMS_SLOTS;                    // channels per wave
constexpr int PMP_WLIST = PMP_WCH * PMH_PCAP;              // (channel, candidate) pairs per wave at most
constexpr size_t PMP_KEY_OFF = PMH_LDS_BYTES;
constexpr size_t PMP_LIST_OFF = PMP_KEY_OFF + (size_t)(PM_FT / 64) * PMP_WCH * 8;
constexpr size_t PMP_LDS_BYTES = PMP_LIST_OFF + (size_t)(PM_FT / 64) * PMP_WLIST * 2;
static_assert(PMP_LDS_BYTES + 1024 <= 160 * 1024 && PMP_KEY_OFF % 8 == 0 && PMP_LIST_OFF % 2 == 0, "the pair recheck's LDS map");
static_assert(PMP_WCH <= 128 && PMS_SLOTS % 2 == 0 && PMH_PCAP == 16, "a list entry is channel-in-wave << 8 | point; a channel's slots are one 16-B read");

__global__ __launch_bounds__(64) void pms_w3_prepare_h_kernel(const float* __restrict__ W3, const float* __restrict__ w3_nw,
                                                              f16x8* __restrict__ w3_h, float* __restrict__ w3_cw) {
  const int cb = blockIdx.x, lane = threadIdx.x;
  const int r = lane & 31, h = lane >> 5;
  const float nw = w3_nw[cb * 32 + r];
  const bool ok = pms_norm_ok(nw);
  const float two_sw = ok ? pmh_pow2(pmh_scale_exp(nw)) : 0.f;    // not screened: zeros, never multiplied
  const float* wrow = W3 + (int64_t)(cb * 32 + r) * PM_C2 + 8 * h;
#pragma unroll
  for (int t = 0; t < PM_C2 / 16; ++t) {
    const float4 lo = *reinterpret_cast<const float4*>(wrow + 16 * t), hi = *reinterpret_cast<const float4*>(wrow + 16 * t + 4);
    const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    f16x8 o;
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = ok ? (_Float16)(v[i] * two_sw) : (_Float16)0.f;   // round to nearest even
    w3_h[(cb * (PM_C2 / 16) + t) * 64 + lane] = o;
  }
  if (h == 0) w3_cw[cb * 32 + r] = ok ? pmh_cw(nw, two_sw) : __builtin_inff();
}

// PAIR: the recheck goes by (channel, candidate) PAIR, one lane each, instead of by channel (further down).
// RAGGED (the production instantiation <false, false, true> only): the cloud ends at its length instead of at N
// (pointmlp_body.h, PMFwdArgsR); a tile beyond it is skipped.
template <bool DBG, bool DUMP, bool PAIR, bool RAGGED = false>
__global__ __launch_bounds__(PM_FT) __attribute__((amdgpu_waves_per_eu(2, 2))) void pointmlp3_max_fwd_screen_h_kernel(
    PMFwdArgsT<RAGGED> a, PMScreenDbg d, PMScreenPrepH w3) {
  static_assert(!RAGGED || (!DBG && !DUMP && PAIR), "the ragged twin is the production form only");
  extern __shared__ __attribute__((aligned(16))) float pms_lds[];
  float* h2 = pms_lds;                                                              // [128][132] fp32, kept to the end
  float* s_na = pms_lds + PM_FWD_LDS_FLOATS;                                        // [128] na 2^sa + 1 (+inf: no such point)
  unsigned* s_amax = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(pms_lds) + PMH_AMAX_OFF);
  unsigned char* s_pts = reinterpret_cast<unsigned char*>(pms_lds) + PMH_PTS_OFF;   // [C3][PMH_PCAP] a channel's candidates
  _Float16* s_a16 = reinterpret_cast<_Float16*>(reinterpret_cast<char*>(pms_lds) + PMH_A16_OFF);   // [128][PMS_LDA]
  const int tile = blockIdx.x, b = blockIdx.y;
  const int n0 = tile * PM_TP;
  int nb = a.N;                           // the cloud's points
  if constexpr (RAGGED) {
    nb = pm_ragged_len(a.lengths, b, a.N);
    if (n0 >= nb) return pm_fwd_skip_tile(a, b, tile);   // (uniform) ahead of the first barrier
  }
  const int nvalid = nb - n0;             // >= 1
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int64_t obase = ((int64_t)b * a.ntiles + tile) * a.C3;
  const int nblk = a.C3 / 32;
  const int nslots = wave < nblk ? (nblk - wave + PM_FT / 64 - 1) / (PM_FT / 64) : 0;   // <= PMS_SLOTS
  // the wave's first block of B operands and its first cw: they depend on nothing the prologue computes
  const f16x8* wb = w3.w3_h + lane;
  f16x8 q[PM_C2 / 16];
  float cw_next = 0.f;
  if (nslots > 0) {
#pragma unroll
    for (int t = 0; t < PM_C2 / 16; ++t) q[t] = wb[(wave * (PM_C2 / 16) + t) * 64];
    cw_next = w3.w3_cw[wave * 32 + r];
  }
  if (threadIdx.x == 0) *s_amax = 0u;     // outside what the prologue touches; its barriers publish it
  pm_fwd_prologue<RAGGED>(a, pms_lds, nb);

  // ---- one norm per point (4 threads per point, 32 k each, fixed order: PREP's na in every bit), the tile's largest,
  // then h2's fp16 image with the tile's scale
  bool bad;
  float na;
  float4 hv[8];
  const int p = threadIdx.x >> 2, pq = threadIdx.x & 3;
  {
    const float* row = h2 + p * PM_LD2 + 32 * pq;
    float ss = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const float4 v = *reinterpret_cast<const float4*>(row + 8 * t), u = *reinterpret_cast<const float4*>(row + 8 * t + 4);
      ss = __builtin_fmaf(v.x, v.x, ss), ss = __builtin_fmaf(v.y, v.y, ss);
      ss = __builtin_fmaf(v.z, v.z, ss), ss = __builtin_fmaf(v.w, v.w, ss);
      ss = __builtin_fmaf(u.x, u.x, ss), ss = __builtin_fmaf(u.y, u.y, ss);
      ss = __builtin_fmaf(u.z, u.z, ss), ss = __builtin_fmaf(u.w, u.w, ss);
      hv[2 * t] = v, hv[2 * t + 1] = u;
    }
    ss += __shfl_xor(ss, 1, 64);
    ss += __shfl_xor(ss, 2, 64);
    na = pms_norm_up(ss);
    bad = !pms_norm_ok(na);               // NaN, inf or huge h2 anywhere in the tile: no screen for this tile
    // all 128 rows count, the ones past the end of a ragged tile too: no image entry can leave fp16's range
    const float wmax = wave_max(na);      // positive floats order as their bits do
    if (lane == 0) atomicMax(s_amax, __builtin_bit_cast(unsigned, wmax));
  }
  const bool tile_bad = __syncthreads_or(bad ? 1 : 0) != 0;
  float two_sa = 1.f;
  if (!tile_bad) {                        // (uniform)
    const float amax = __builtin_bit_cast(float, *s_amax);          // in [2^-45, 2^60]
    two_sa = pmh_pow2(pmh_scale_exp(amax));
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const float4 v = hv[2 * t], u = hv[2 * t + 1];
      const float x[8] = {v.x, v.y, v.z, v.w, u.x, u.y, u.z, u.w};
      f16x8 o;
#pragma unroll
      for (int i = 0; i < 8; ++i) o[i] = (_Float16)(x[i] * two_sa);   // round to nearest even (not cvt_pkrtz)
      *reinterpret_cast<f16x8*>(s_a16 + p * PMS_LDA + 32 * pq + 8 * t) = o;
    }
    if (pq == 0) s_na[p] = p < nvalid ? pmh_na(na, two_sa) : __builtin_inff();   // past the end: see pms_lower
  }
  __syncthreads();
  if (DBG && d.stop_after == 1) return;

  unsigned vmask[2] = {0u, 0u};           // the lane's 64 points that exist (all of them but in a ragged last tile)
#pragma unroll
  for (int pt = 0; pt < 4; ++pt)
#pragma unroll
    for (int e = 0; e < 16; ++e) vmask[pt >> 1] |= (pms_point(pt, e, h) < nvalid) ? (1u << (16 * (pt & 1) + e)) : 0u;
  unsigned screened = 0u, cnts = 0u;      // bit slot: screened; bits 5 slot .. + 4: candidates of the lane's channel r
  int ncand = 0, nfall = 0;
  float sink = 0.f;
#pragma unroll 1
  for (int slot = 0; slot < nslots; ++slot) {
    const int cb = wave + (PM_FT / 64) * slot;
    const int nxt = slot + 1 < nslots ? cb + PM_FT / 64 : cb;   // past the wave's last block: a valid address, unused
    const float cw = cw_next;             // the next one is loaded behind the products: the select hides its round trip
    // (uniform) a non-finite or huge h2 in the tile, or such a W3 row in the block (its prepared cw says so)
    bool fall = tile_bad || __builtin_amdgcn_ballot_w64(!pmh_cw_ok(cw)) != 0ull;
    if (!fall) {
      f32x16 acc[4];
#pragma unroll
      for (int pt = 0; pt < 4; ++pt)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[pt][e] = 0.f;
#pragma unroll
      for (int t = 0; t < PM_C2 / 16; ++t) {
        const f16x8 bq = q[t];
        q[t] = wb[(nxt * (PM_C2 / 16) + t) * 64];   // the ring: the same k-step of the wave's next block
#pragma unroll
        for (int pt = 0; pt < 4; ++pt) {   // A: lane (r, h) holds h2'[32 pt + r][16 t + 8 h + 0..7]
          const f16x8 ah = *reinterpret_cast<const f16x8*>(s_a16 + (pt * 32 + r) * PMS_LDA + 16 * t + 8 * h);
          acc[pt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bq, acc[pt], 0, 0, 0);
        }
      }
      // the order of the 8 loads, 32 LDS reads and 32 MFMAs above, pinned as in PREP: a k-step's load leads it and lands
      // a whole block later; the A operands are read two (pt) groups ahead
      __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);        // 2 DS read
#pragma unroll
      for (int g = 0; g < 4 * (PM_C2 / 16); ++g) {
        if (g % 4 == 0) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);   // 1 VMEM read
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);      // 1 MFMA
        if (g + 2 < 4 * (PM_C2 / 16)) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      }
      __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);        // the next block's cw
      cw_next = w3.w3_cw[nxt * 32 + r];
      if (DBG && d.stop_after == 2) {
#pragma unroll
        for (int pt = 0; pt < 4; ++pt)
#pragma unroll
          for (int e = 0; e < 16; ++e) sink += acc[pt][e];
        continue;
      }
      if (DUMP && d.dbg_S != nullptr) {   // unscaled: S 2^-(sa + sw), E 2^-(sa + sw) (exact but for underflow)
        int c3v = a.C3;
        unsigned vm[2] = {vmask[0], vmask[1]};
        asm volatile("" : "+v"(c3v), "+v"(vm[0]), "+v"(vm[1]));   // opaque: nothing of the 64 stores is hoisted out of the block loop
        const int64_t o0 = ((int64_t)b * a.N + n0) * a.C3 + cb * 32 + r;
        const float back_a = 1.f / two_sa, back_w = 1.f / pmh_pow2(pmh_scale_exp(w3.w3_nw[cb * 32 + r]));
#pragma unroll
        for (int pt = 0; pt < 4; ++pt)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int pp = pms_point(pt, e, h);
            if ((vm[pt >> 1] >> (16 * (pt & 1) + e)) & 1u) {
              d.dbg_S[o0 + (int64_t)pp * c3v] = acc[pt][e] * back_a * back_w;
              d.dbg_E[o0 + (int64_t)pp * c3v] = pms_E(s_na[pp], cw) * back_a * back_w;
            }
          }
      }
      unsigned flags[2];
      float L = pms_lower(acc, s_na, cw, h);
      L = fmaxf(L, __shfl_xor(L, 32, 64));
      pms_flags(acc, s_na, cw, h, L, flags);
      flags[0] &= vmask[0], flags[1] &= vmask[1];
      const int cnt = __builtin_popcount(flags[0]) + __builtin_popcount(flags[1]);
      const int other = __shfl_xor(cnt, 32, 64);   // the channel's other half of the points
      if (__builtin_amdgcn_ballot_w64(cnt + other > PMH_PCAP) != 0ull) {
        fall = true;                      // (uniform) a channel with more candidates than its slots: the exact block instead
      } else {
        unsigned char* mine = s_pts + (cb * 32 + r) * PMH_PCAP + (h ? other : 0);   // h = 1 writes behind h = 0's
#pragma unroll
        for (int wd = 0; wd < 2; ++wd) {
          unsigned f = flags[wd];
          while (f) {
            const int bit = __builtin_ctz(f);
            f &= f - 1;
            *mine++ = (unsigned char)pms_point(2 * wd + (bit >> 4), bit & 15, h);
          }
        }
        cnts |= (unsigned)(cnt + other) << (5 * slot);
        screened |= 1u << slot;
        if (DBG) ncand += h ? 0 : cnt + other;
      }
    } else {                              // not screened: the ring moves on to the next block
#pragma unroll
      for (int t = 0; t < PM_C2 / 16; ++t) q[t] = wb[(nxt * (PM_C2 / 16) + t) * 64];
      cw_next = w3.w3_cw[nxt * 32 + r];
    }
    if (fall) {
      pms_exact_block(h2, a.W3, a.b3, cb, n0, nb, a.part_val + obase, a.part_idx + obase);
      ++nfall;
    }
  }
  if (DBG && d.stop_after == 2) {
    if (sink == 12345.678f) a.part_val[obase] = sink;   // keeps the products alive
    return;
  }
  if (DBG && d.stats != nullptr) {
    ncand = wave_sum(ncand);
    if (lane == 0) {
      int32_t* st = d.stats + ((int64_t)b * a.ntiles + tile) * 2;
      if (ncand) atomicAdd(st, ncand);
      if (nfall) atomicAdd(st + 1, nfall);
    }
  }
  if (DBG && d.stop_after == 3) {
    if (cnts == 0xffffffffu) a.part_val[obase] = 0.f;
    return;
  }

  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // the channels' candidate points, written by other lanes
  if constexpr (PAIR) {
    // ---- recheck by pair: one lane per (channel, candidate) of the wave's screened blocks, so a trip's 64 chains are
    // 64 chains somebody needs (by channel, a trip lasts as long as its fullest channel and most lanes idle behind their
    // first chain). Only this wave touches its list and its keys: no barrier.
    unsigned long long* my_key = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(pms_lds) + PMP_KEY_OFF) + wave * PMP_WCH;
    unsigned short* my_list = reinterpret_cast<unsigned short*>(reinterpret_cast<char*>(pms_lds) + PMP_LIST_OFF) + wave * PMP_WLIST;
    // the schedule: channels slot-major then r, which is lane order within a pass (lane = 32 (slot & 1) + r); an
    // exclusive scan of the counts gives a channel its first pair, and the channel's lane writes its pairs
    int total = 0;                        // (uniform) <= PMP_WLIST
#pragma unroll 1
    for (int j = 0; 2 * j < nslots; ++j) {
      const int sl = 2 * j + h;
      const bool live = sl < nslots && ((screened >> sl) & 1u);   // a fallen or missing slot counts 0
      const int n = live ? (int)((cnts >> (5 * sl)) & 31u) : 0;
      int pass_total;
      const int excl = wave_excl_scan_bits<5>(n, pass_total);   // n <= PMH_PCAP = 16
      my_key[64 * j + lane] = 0ull;       // channel-in-wave 32 sl + r
      const int c = (wave + (PM_FT / 64) * (live ? sl : 0)) * 32 + r;   // an idle lane: a valid row, unused
      const uint4 pv = *reinterpret_cast<const uint4*>(s_pts + c * PMH_PCAP);   // the channel's sixteen slots
      unsigned short* dst = my_list + total + excl;
      const unsigned tag = (unsigned)(64 * j + lane) << 8;
#pragma unroll 1
      for (int i = 0; __builtin_amdgcn_ballot_w64(i < n) != 0ull; ++i) {   // (uniform) up to the fullest channel
        const unsigned pw = i < 4 ? pv.x : i < 8 ? pv.y : i < 12 ? pv.z : pv.w;
        if (i < n) dst[i] = (unsigned short)(tag | ((pw >> (8 * (i & 3))) & 255u));
      }
      total += pass_total;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // the list and the zeroed keys
    if (total > 0) {                      // (uniform)
      // lane l of trip k takes pair 64 k + l; the lanes past the end of the last trip sit it out (their pair is the
      // last one's, a valid row, and nothing of it is loaded, read or entered)
      int e = my_list[min(lane, total - 1)];
      int c3s = a.C3;
      asm volatile("" : "+s"(c3s));       // opaque: the rows' 64-bit stride is formed here, not held from the kernel's head
#pragma unroll 1
      for (int k0 = 0; k0 < total; k0 += 64) {
        const bool act = k0 + lane < total;
        const int ci = e >> 8, pc = e & 255;
        e = my_list[min(k0 + 64 + lane, total - 1)];   // the next trip's pair, asked for ahead of this trip's chain
        if (!act) continue;
        const int c = (wave + (PM_FT / 64) * (ci >> 5)) * 32 + (ci & 31);
        float4 wv[PM_C2 / 4];             // ascending channels: a load covers a few contiguous runs of w3_q[t]
#pragma unroll
        for (int t = 0; t < PM_C2 / 4; ++t) wv[t] = w3.w3_q[(int64_t)t * c3s + c];
        const float4* ar = reinterpret_cast<const float4*>(h2 + pc * PM_LD2);
        __builtin_amdgcn_sched_barrier(0);
        float v = 0.f;
#pragma unroll
        for (int t = 0; t < PM_C2 / 8; ++t) {   // the chain of the channel form, literally
          const float4 a0 = ar[2 * t], a1 = ar[2 * t + 1];
          const float4 w0 = wv[2 * t], w1 = wv[2 * t + 1];
          v = __builtin_fmaf(a0.x, w0.x, v), v = __builtin_fmaf(a1.x, w1.x, v);
          v = __builtin_fmaf(a0.y, w0.y, v), v = __builtin_fmaf(a1.y, w1.y, v);
          v = __builtin_fmaf(a0.z, w0.z, v), v = __builtin_fmaf(a1.z, w1.z, v);
          v = __builtin_fmaf(a0.w, w0.w, v), v = __builtin_fmaf(a1.w, w1.w, v);
        }
        // the h2 row's reads pinned four k-groups ahead of the chain, as in the channel form
        __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);        // 8 DS read
#pragma unroll
        for (int g = 0; g < PM_C2 / 8; ++g) {
          __builtin_amdgcn_sched_group_barrier(0x002, 8, 0);      // 8 VALU: the group's fmaf
          if (g + 4 < PM_C2 / 8) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
        }
        const unsigned vb = __builtin_bit_cast(unsigned, v);
        const unsigned zb = (v == 0.f) ? 0u : vb;
        const unsigned ord = (zb & 0x80000000u) ? ~zb : (zb | 0x80000000u);
        const unsigned low = ((unsigned)(127 - pc) << 1) | ((vb == 0x80000000u) ? 1u : 0u);
        // a channel's pairs are neighbours but may straddle a trip: an LDS max on the channel's key, order-free
        atomicMax(&my_key[ci], ((unsigned long long)ord << 32) | low);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // the keys, entered by other lanes
#pragma unroll
    for (int j = 0; j < PMS_SLOTS / 2; ++j) {
      const int sl = 2 * j + h;
      if (!(sl < nslots && ((screened >> sl) & 1u))) continue;   // a fallen block's channels were stored by the exact block
      const int c = (wave + (PM_FT / 64) * sl) * 32 + r;
      const unsigned long long key = my_key[64 * j + lane];
      const unsigned ord = (unsigned)(key >> 32), low = (unsigned)key;
      unsigned vb = (ord & 0x80000000u) ? (ord & 0x7fffffffu) : ~ord;
      if (low & 1u) vb = 0x80000000u;
      a.part_val[obase + c] = __builtin_bit_cast(float, vb) + a.b3[c];
      a.part_idx[obase + c] = n0 + 127 - (int)((low >> 1) & 127u);
    }
    return;
  }
  // ---- recheck by channel, as in PREP: the exact kernel's chain from the UNSCALED fp32 h2 and fp32 row
#pragma unroll 1
  for (int j = 0; 2 * j < nslots; ++j) {
    const int sl = 2 * j + h;
    const bool live = sl < nslots && ((screened >> sl) & 1u);
    const int n = live ? (int)((cnts >> (5 * sl)) & 31u) : 0;
    if (__builtin_amdgcn_ballot_w64(n > 0) == 0ull) continue;   // (uniform)
    const int c = (wave + (PM_FT / 64) * (live ? sl : 0)) * 32 + r;   // an idle lane: a valid row, unused
    float4 wv[PM_C2 / 4];               // the whole row in flight at once: one round trip per trip
#pragma unroll
    for (int t = 0; t < PM_C2 / 4; ++t) wv[t] = w3.w3_q[(int64_t)t * a.C3 + c];
    unsigned long long key = 0ull;
#pragma unroll 1
    for (int i = 0; i < PMH_PCAP; ++i) {
      if (__builtin_amdgcn_ballot_w64(i < n) == 0ull) break;    // (uniform)
      const int pc = i < n ? s_pts[c * PMH_PCAP + i] : 0;
      const float4* ar = reinterpret_cast<const float4*>(h2 + pc * PM_LD2);
      __builtin_amdgcn_sched_barrier(0);
      float v = 0.f;
#pragma unroll
      for (int t = 0; t < PM_C2 / 8; ++t) {
        const float4 a0 = ar[2 * t], a1 = ar[2 * t + 1];
        const float4 w0 = wv[2 * t], w1 = wv[2 * t + 1];
        v = __builtin_fmaf(a0.x, w0.x, v), v = __builtin_fmaf(a1.x, w1.x, v);
        v = __builtin_fmaf(a0.y, w0.y, v), v = __builtin_fmaf(a1.y, w1.y, v);
        v = __builtin_fmaf(a0.z, w0.z, v), v = __builtin_fmaf(a1.z, w1.z, v);
        v = __builtin_fmaf(a0.w, w0.w, v), v = __builtin_fmaf(a1.w, w1.w, v);
      }
      // hipcc reads the h2 row two float4 ahead of the chain and then waits out an LDS round trip (64 lanes, 64 rows)
      // per k-group of 8: pinned four groups ahead instead (32 VGPRs), the chain's order untouched
      __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);        // 8 DS read
#pragma unroll
      for (int g = 0; g < PM_C2 / 8; ++g) {
        __builtin_amdgcn_sched_group_barrier(0x002, 8, 0);      // 8 VALU: the group's fmaf
        if (g + 4 < PM_C2 / 8) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
      }
      const unsigned vb = __builtin_bit_cast(unsigned, v);
      const unsigned zb = (v == 0.f) ? 0u : vb;
      const unsigned ord = (zb & 0x80000000u) ? ~zb : (zb | 0x80000000u);
      const unsigned low = ((unsigned)(127 - pc) << 1) | ((vb == 0x80000000u) ? 1u : 0u);
      const unsigned long long k = ((unsigned long long)ord << 32) | low;
      if (i < n && k > key) key = k;
    }
    if (live) {
      const unsigned ord = (unsigned)(key >> 32), low = (unsigned)key;
      unsigned vb = (ord & 0x80000000u) ? (ord & 0x7fffffffu) : ~ord;
      if (low & 1u) vb = 0x80000000u;
      a.part_val[obase + c] = __builtin_bit_cast(float, vb) + a.b3[c];
      a.part_idx[obase + c] = n0 + 127 - (int)((low >> 1) & 127u);
    }
  }
}

// A screened instantiation needs its dynamic-LDS attribute, which is set at its first use on a device and never while
// the stream is capturing. pms_usable: per instantiation, per device, the attribute is set.
template <auto KERNEL>
static bool pms_usable[64] = {};

// 0: launched. 1: not launched — the instantiation cannot be yet (the caller takes the next form). < 0: an error.
template <auto KERNEL, size_t LDS, class Q, class A = PMFwdArgs>
static int pms_launch_t(const A& a, int B, hipStream_t st, const PMScreenDbg& d, const Q& q) {
  int dev = 0;
  PC3D_REQUIRE(hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64, "pointmlp3 screen: no current device");
  if (!pms_usable<KERNEL>[dev]) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) {
      (void)hipGetLastError();
      return 1;
    }
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS);
    PC3D_REQUIRE(e == hipSuccess, "pointmlp3 screen: hipFuncSetAttribute(MaxDynamicSharedMemorySize): %s", hipGetErrorString(e));
    pms_usable<KERNEL>[dev] = true;
  }
  hipLaunchKernelGGL(KERNEL, dim3(a.ntiles, B), dim3(PM_FT), LDS, st, a, d, q);
  return 0;
}

// the production, the statistics or the dump instantiation of a form, as d asks
template <bool PAIR>
static int pms_launch_h(const PMFwdArgs& a, int B, hipStream_t st, const PMScreenDbg& d, const PMScreenPrepH& q) {
  constexpr size_t lds = PAIR ? PMP_LDS_BYTES : PMH_LDS_BYTES;
  if (d.dbg_S || d.dbg_E) return pms_launch_t<pointmlp3_max_fwd_screen_h_kernel<true, true, PAIR>, lds>(a, B, st, d, q);
  if (d.stats || d.stop_after) return pms_launch_t<pointmlp3_max_fwd_screen_h_kernel<true, false, PAIR>, lds>(a, B, st, d, q);
  return pms_launch_t<pointmlp3_max_fwd_screen_h_kernel<false, false, PAIR>, lds>(a, B, st, d, q);
}

// the production instantiation of pms_launch_h<PAIR> has its attribute on the current device (a template, so that it
// names the kernel after pms_launch_h has: the kernels keep their order in the code object)
template <bool PAIR>
static bool pms_h_usable() {
  int dev = 0;
  return hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64 &&
         pms_usable<pointmlp3_max_fwd_screen_h_kernel<false, false, PAIR>>[dev];
}

template <bool PREP>
static int pms_launch_form(const PMFwdArgs& a, int B, hipStream_t st, const PMScreenDbg& d, const PMScreenPrep& q) {
  constexpr size_t lds = PREP ? PMS_LDS_BYTES_PREP : PMS_LDS_BYTES;
  if (d.dbg_S || d.dbg_E) return pms_launch_t<pointmlp3_max_fwd_screen_kernel<true, true, PREP>, lds>(a, B, st, d, q);
  if (d.stats || d.stop_after) return pms_launch_t<pointmlp3_max_fwd_screen_kernel<true, false, PREP>, lds>(a, B, st, d, q);
  return pms_launch_t<pointmlp3_max_fwd_screen_kernel<false, false, PREP>, lds>(a, B, st, d, q);
}

int pm_fwd_screen_launch(const PMFwdArgs& a, int B, void* stream, int32_t* stats, float* dbg_S, float* dbg_E,
                         int stop_after, int form, const PMScreenPrep& prep, const PMScreenPrepH& hprep) {
  const PMScreenDbg d{stats, dbg_S, dbg_E, stop_after};
  hipStream_t st = as_stream(stream);
  // every case falls through to the next form when its own instantiation could not be launched (its first use on the
  // device falls into a capture): the pair recheck to the channel one, the fp16 screen to the prepared bf16 one, that
  // one to the in-launch form, which reads no image
  switch (form) {
    case PC3D_PM_FWD_SCREEN_H_PAIR:
      if (pms_launch_h<true>(a, B, st, d, hprep) == 0) return 0;
      [[fallthrough]];
    case PC3D_PM_FWD_SCREEN_H:
      if (pms_launch_h<false>(a, B, st, d, hprep) == 0) return 0;
      [[fallthrough]];
    case PC3D_PM_FWD_SCREEN_PREP:
      if (pms_launch_form<true>(a, B, st, d, prep) == 0) return 0;
      [[fallthrough]];
    default:
      return pms_launch_form<false>(a, B, st, d, PMScreenPrep{nullptr, nullptr, nullptr});
  }
}

// (named behind every dense instantiation: the kernels keep their order in the code object)
int pm_fwd_screen_ragged_launch(const PMFwdArgsR& a, int B, void* stream, const PMScreenPrepH& hprep) {
  return pms_launch_t<pointmlp3_max_fwd_screen_h_kernel<false, false, true, true>, PMP_LDS_BYTES>(
      a, B, as_stream(stream), PMScreenDbg{nullptr, nullptr, nullptr, 0}, hprep);
}

int pm_fwd_pair_ready() { return pms_h_usable<true>() ? 1 : 0; }

int pm_w3_prepare_launch(const float* W3, int C3, void* w3_bf, float* w3_nw, float* w3_q, void* stream) {
  hipLaunchKernelGGL(pms_w3_prepare_kernel, dim3(C3 / 32), dim3(64), 0, as_stream(stream), W3,
                     reinterpret_cast<bf16x8*>(w3_bf), w3_nw, reinterpret_cast<float4*>(w3_q), C3);
  return 0;
}

int pm_w3_prepare_h_launch(const float* W3, int C3, const float* w3_nw, void* w3_h, float* w3_cw, void* stream) {
  hipLaunchKernelGGL(pms_w3_prepare_h_kernel, dim3(C3 / 32), dim3(64), 0, as_stream(stream), W3, w3_nw,
                     reinterpret_cast<f16x8*>(w3_h), w3_cw);
  return 0;
}

}  // namespace pc3d
