// GeoA3's iteration after the victim's passes and the searches (attack/GeoA3/GeoA3_attack.py:139-181, :321-351 with
// loss_utils.py:36-105 and lp_clip, :92-102) as ONE launch, one workgroup of 1024 threads per cloud:
//   1. record  — the success test on the prediction the loss launch wrote, the constraint value of the PREVIOUS iteration,
//                the six best_* / iter_best_* words and the copy of the iterate (pc3d_geoa3_record_f32's formulation);
//   2. terms   — dis (Chamfer, two- or single-sided, or the L2 sum), hd (max of the adv -> ori squared distances, first
//                index on ties), curv (mean of (kappa_adv - kappa_ori[nn])^2, kappa_fwd_kernel's arithmetic), constrain and
//                loss_n = cls + scale * constrain, written to row `step` of the loss buffer;
//   3. gradient of gval * scale * constrain w.r.t. the iterate, added to the victim's (already scaled) gradient;
//   4. Adam on the offset (adam_element of update_body.h, what pc3d_adam_clip_step_f32 runs), the scheduler's lr *= 0.9990, lp_clip, x = ori + offset.
// It stands for pc3d_geoa3_record_f32 + pc3d_kappa_gather_f32 + pc3d_geoa3_terms_f32 + pc3d_geoa3_terms_bwd_f32 +
// pc3d_kappa_bwd_f32 + two pc3d_nn_bwd_f32 + pc3d_adam_clip_step_f32 in the captured iteration of
// geoA3_attack(cfg.device_loop = True). Distances are direct-form squared distances recomputed from the points on the given
// arg-mins: the searches hand over indices only.
//
// The sums into a point. Two kinds of gradient arrive at a point from OTHER points: the curvature term of every point i
// that lists it as a neighbour (edge (i, e) -> idx[i, e], k edges per point), and the ori -> adv Chamfer term of every ori
// point whose arg-min it is. For each kind the workgroup builds a reverse index in LDS — a counting sort by target: in-degrees
// by integer LDS atomics, an exclusive scan, the sources dropped into their target's bucket (integer atomics again: the
// bucket's CONTENT is fixed, its order is not), and then the owner of a target sorts its bucket ascending by source. Every
// point gathers its incoming edges in that order, after its own-side sum in neighbour order: the order of the additions is a
// function of that cloud's own indices alone, not of the batch, the grid or the launch. No float atomics anywhere.
// A source that names the same target twice contributes two equal values, so their mutual order is immaterial.
//
// State words are PER CLOUD (step [B] int32, lr [B] double): each workgroup reads and advances its own, so no workgroup can
// see another's update, and a cloud's bits do not depend on its batch.
//
// LDS per cloud of N points (np = N rounded up to 4), k = curvature neighbours:
//   always             the iterate                                   12 np
//   curvature          normals of the nearest ori points 12 np, kappa difference 4 np, bucket ends 4 np,
//                      the reverse index 2 N k (uint16 sources)
//   two-sided Chamfer  bucket ends 4 np, the reverse index 2 np
//   scratch            512 B
// = 38 N + 2 N k + 512 B: 140.5 KiB at N = 2048, k = 16 — the cap. The CU has 160 KiB; N = 4096 at k = 16 would need 280 KiB
// (the reverse index alone 128), and a reverse index in global memory would put back the round trips this launch removes.
// Whatever N and k, a launch whose 38 N + 2 N k + 512 bytes exceed 160 KiB is refused (at N = 2048: k > 20).
#include "update_body.h"

namespace pc3d {

constexpr int kGuThreads = 1024;
constexpr int kGuWaves = kGuThreads / 64;
constexpr int kGuMaxPoints = PC3D_GEOA3_UPDATE_MAX_POINTS;
constexpr size_t kGuLdsLimit = 160 * 1024;
constexpr int kGuScratch = 512;
static_assert(kGuMaxPoints <= 65536, "reverse-index entries are uint16");

struct GeoUpdArgs {
  float* x;                  // [B,3,N] the iterate, rewritten as ori + offset
  const float* ori;          // [B,3,N]
  float* offset;             // [B,3,N] Adam's variable
  const float* g;            // [B,3,N] the victim's gradient, already scaled
  float *m, *v;              // [B,3,N]
  int N, K1;                 // K1 = k + 1 columns of knn_idx (self first); 1: no curvature term
  const int32_t* nn_ao;      // [B,N] adv -> ori arg-mins, or null (L2 without curvature)
  const int32_t* nn_oa;      // [B,N] ori -> adv arg-mins, or null (single-sided)
  const int32_t* knn_idx;    // [B,N,K1] or null
  const float* normal_ori;   // [B,3,N] (curvature)
  const float* kappa_ori;    // [B,N]   (curvature)
  const float* cls;          // [B]
  const float* scale;        // [B]
  const int64_t* pred;       // [B]
  const int64_t* target;     // [B]
  int targeted, dis_kind;    // dis_kind 0: Chamfer, 1: L2 sum
  float gval, w_dis, w_hd, w_curv;
  float* constrain;          // [B] in: the previous iteration's value, out: this one's
  float* loss_rows;          // [max_steps,B]
  int max_steps, B;
  int32_t* step;             // [B]
  const int32_t* search_step;   // [1]
  double* lr;                // [B]
  int scheduler;
  float* best_loss;          // [B]
  float* best_attack;        // [B,3,N]
  int64_t *best_bs, *best_step;
  float* iter_best_loss;
  int64_t* iter_best_score;
  double b1, b2;
  float eps, cc_linf;
  float* terms_out;          // [5,B] dis, hd, curv, constrain, loss_n — or null
  int32_t* hd_arg_out;       // [B] or null
  float* g_out;              // [B,3,N] the total gradient, or null
};
// Clouds of different sizes in one batch: cloud b counts lengths[b] points (int32 [B], read as data, clamped to [1, N]).
struct GeoUpdRaggedArgs : GeoUpdArgs {
  const int32_t* lengths;
};
template <bool RAGGED> struct GeoUpdArgsOf { using type = GeoUpdArgs; };
template <> struct GeoUpdArgsOf<true> { using type = GeoUpdRaggedArgs; };

static inline size_t geo_upd_lds_bytes(int N, int k, bool curv, bool two) {
  const size_t np = (size_t)((N + 3) & ~3);
  size_t s = np * 12 + kGuScratch;
  if (curv) s += np * 20 + (((size_t)N * k * 2 + 15) & ~(size_t)15);
  if (two) s += np * 4 + ((np * 2 + 15) & ~(size_t)15);
  return s;
}

// the sum of one value per thread in a fixed order: the wave's shuffle tree, then the 16 wave partials ascending
__device__ __forceinline__ float gu_block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = 0.f;
#pragma unroll
  for (int w = 0; w < kGuWaves; ++w) s += red[w];
  return s;
}

// counts [N] -> exclusive offsets, in place; thread t owns the `per` consecutive entries from t * per
__device__ __forceinline__ void gu_exclusive_scan(int* cnt, int N, int* red) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int per = (N + kGuThreads - 1) / kGuThreads, lo = tid * per, hi = min(lo + per, N);
  int s = 0;
  for (int i = lo; i < hi; ++i) s += cnt[i];
  int inc = s;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(inc, o, 64);
    if (lane >= o) inc += up;
  }
  __syncthreads();
  if (lane == 63) red[wave] = inc;
  __syncthreads();
  int base = inc - s;
  for (int w = 0; w < wave; ++w) base += red[w];
  for (int i = lo; i < hi; ++i) {
    const int c = cnt[i];
    cnt[i] = base;
    base += c;
  }
  __syncthreads();
}

__device__ __forceinline__ void gu_sort_bucket(uint16_t* rev, int s, int e) {
  for (int a = s + 1; a < e; ++a) {
    const uint16_t key = rev[a];
    int c = a - 1;
    while (c >= s && rev[c] > key) {
      rev[c + 1] = rev[c];
      --c;
    }
    rev[c + 1] = key;
  }
}

// RAGGED: N is the capacity — the row stride of every [B,3,N], [B,N] and [B,N,K1] buffer and the size of the LDS arrays —
// and every loop over points, the means' divisors, the index clamps, the bucket bounds and the scans run over L =
// clamp(lengths[b], 1, N) with the dense kernel's thread-to-point mapping and summation order: rows < L have the bits of the
// dense launch at N = L on that cloud alone. Rows >= L of no input are loaded (they may hold NaN or any integer); those of
// m, v, offset and g_out stay; x's take the NEW point 0 — the padding the victim's passes and the next searches rely on: an
// exact copy of row 0 loses every tie to index 0 — and the record copies the iterate's row 0 into best_attack's. The dense
// instantiation compiles to the kernel it was before RAGGED existed (the parameter is a type of its own).
template <bool RAGGED>
__global__ __launch_bounds__(kGuThreads) void geoa3_update_kernel(typename GeoUpdArgsOf<RAGGED>::type a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gu_lds[];
  const int N = a.N, np = (N + 3) & ~3, K1 = a.K1, k = K1 - 1;
  const int b = blockIdx.x, tid = threadIdx.x;
  int L = N;
  if constexpr (RAGGED) L = min(max(a.lengths[b], 1), N);
  const bool curv = a.knn_idx != nullptr && k >= 1 && a.w_curv != 0.f;
  const bool two = a.dis_kind == 0 && a.nn_oa != nullptr;
  const bool chamfer = a.dis_kind == 0;
  // carve (every offset a multiple of 16)
  float* scr = reinterpret_cast<float*>(gu_lds);                 // scratch: 128 words
  float* red = scr;                                              // [16]
  float* redv = scr + 16;                                        // [16]
  int* redi = reinterpret_cast<int*>(scr + 32);                  // [16]
  float* s_c = scr + 48;                                         // broadcast constants
  int* s_i = reinterpret_cast<int*>(scr + 64);                   // broadcast integers
  [[maybe_unused]] float* s_pad = scr + 80;                      // [3] RAGGED: the new point 0
  float* sx = scr + kGuScratch / 4;
  float* sy = sx + np;
  float* sz = sy + np;
  unsigned char* nxt = reinterpret_cast<unsigned char*>(sz + np);
  float *nx = nullptr, *ny = nullptr, *nz = nullptr, *kd = nullptr;
  int *off = nullptr, *off2 = nullptr;
  uint16_t *rev = nullptr, *rev2 = nullptr;
  if (curv) {
    nx = reinterpret_cast<float*>(nxt), ny = nx + np, nz = ny + np, kd = nz + np;
    off = reinterpret_cast<int*>(kd + np);
    rev = reinterpret_cast<uint16_t*>(off + np);
    nxt = reinterpret_cast<unsigned char*>(rev) + (((size_t)N * k * 2 + 15) & ~(size_t)15);
  }
  if (two) {
    off2 = reinterpret_cast<int*>(nxt);
    rev2 = reinterpret_cast<uint16_t*>(off2 + np);
  }
  const int64_t base3 = (int64_t)b * 3 * N, base1 = (int64_t)b * N;
  const float* xg = a.x + base3;
  const float* og = a.ori + base3;
  const int32_t* ib = curv ? a.knn_idx + base1 * K1 : nullptr;

  // ---- 1. record, the state words, Adam's bias corrections (thread 0); the cloud into LDS (everyone) ----
  if (tid == 0) {
    const int t0 = a.step[b];
    const double lrv = a.lr[b];
    const int t = t0 + 1;
    s_c[0] = adam_step_size(lrv, a.b1, t);
    s_c[1] = adam_bc2s(a.b2, t);
    a.step[b] = t;
    if (a.scheduler) a.lr[b] = lrv * 0.9990;
    const int64_t lab = a.pred[b];
    const bool ok = a.targeted ? (lab == a.target[b]) : (lab != a.target[b]);
    const float met = a.constrain[b];
    const bool upd = ok && met < a.best_loss[b];
    if (upd) a.best_loss[b] = met, a.best_bs[b] = (int64_t)a.search_step[0], a.best_step[b] = (int64_t)t0;
    if (ok && met < a.iter_best_loss[b]) a.iter_best_loss[b] = met, a.iter_best_score[b] = lab;
    s_i[0] = upd ? 1 : 0;
    s_i[1] = t0;
  }
  for (int p = tid; p < L; p += kGuThreads) {
    sx[p] = xg[p], sy[p] = xg[N + p], sz[p] = xg[2 * N + p];
    if (curv) {
      const int q = min(max(a.nn_ao[base1 + p], 0), L - 1);
      const float* nb = a.normal_ori + base3;
      nx[p] = nb[q], ny[p] = nb[N + q], nz[p] = nb[2 * N + q];
      off[p] = 0;
    }
    if (two) off2[p] = 0;
  }
  if constexpr (RAGGED) {      // the iterate's padding rows are copies of its row 0: written so, not read
    const float x0 = xg[0], y0 = xg[N], z0 = xg[2 * N];
    for (int p = L + tid; p < N; p += kGuThreads) sx[p] = x0, sy[p] = y0, sz[p] = z0;
  }
  __syncthreads();
  if (s_i[0]) {
    float* dst = a.best_attack + base3;
    for (int p = tid; p < N; p += kGuThreads) dst[p] = sx[p], dst[N + p] = sy[p], dst[2 * N + p] = sz[p];
  }

  // ---- 2. terms ----
  float s_ao = 0.f, s_oa = 0.f, s_cv = 0.f, mx = -__builtin_inff();
  int mi = 0x7fffffff;
  for (int p = tid; p < L; p += kGuThreads) {
    const float px = sx[p], py = sy[p], pz = sz[p];
    if (a.nn_ao != nullptr || !chamfer) {
      const int q = chamfer ? min(max(a.nn_ao[base1 + p], 0), L - 1) : p;
      const float dx = px - og[q], dy = py - og[N + q], dz = pz - og[2 * N + q];
      const float d = dx * dx + dy * dy + dz * dz;
      s_ao += d;
      if (chamfer && d > mx) mx = d, mi = p;      // ascending p within a thread: strict > keeps the first maximum
    }
    if (two) {
      const int i = min(max(a.nn_oa[base1 + p], 0), L - 1);
      const float dx = og[p] - sx[i], dy = og[N + p] - sy[i], dz = og[2 * N + p] - sz[i];
      s_oa += dx * dx + dy * dy + dz * dz;
      atomicAdd(off2 + i, 1);
    }
    if (curv) {
      const float ux = nx[p], uy = ny[p], uz = nz[p];
      const int32_t* nb = ib + (int64_t)p * K1;
      float s = 0.f;
      for (int e = 1; e < K1; ++e) {
        const int j = min(max(nb[e], 0), L - 1);
        const float dx = sx[j] - px, dy = sy[j] - py, dz = sz[j] - pz;
        const float len = fmaxf(sqrtf(dx * dx + dy * dy + dz * dz), 1e-12f);
        s += fabsf((dx / len) * ux + (dy / len) * uy + (dz / len) * uz);
        atomicAdd(off + j, 1);
      }
      const int q = min(max(a.nn_ao[base1 + p], 0), L - 1);
      const float t = s / (float)k - a.kappa_ori[base1 + q];
      kd[p] = t;
      s_cv += t * t;
    }
  }
  s_ao = gu_block_sum(s_ao, red);
  s_oa = gu_block_sum(s_oa, red);
  s_cv = gu_block_sum(s_cv, red);
  {      // arg-max over the workgroup: (value, lowest index)
    const float wv = wave_max(mx);
    int cand = (mx == wv) ? mi : 0x7fffffff;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cand = min(cand, __shfl_xor(cand, o, 64));
    __syncthreads();
    if ((tid & 63) == 0) redv[tid >> 6] = wv, redi[tid >> 6] = cand;
    __syncthreads();
  }
  if (tid == 0) {
    mx = redv[0], mi = redi[0];
    for (int w = 1; w < kGuWaves; ++w)
      if (redv[w] > mx || (redv[w] == mx && redi[w] < mi)) mx = redv[w], mi = redi[w];
    const bool has_hd = chamfer && mi != 0x7fffffff;
    const float dis = chamfer ? s_ao / (float)L + (two ? s_oa / (float)L : 0.f) : s_ao;
    const float hd = has_hd ? mx : 0.f;
    const float cv = curv ? s_cv / (float)L : 0.f;
    const float con = (a.w_dis * dis + a.w_hd * hd) + a.w_curv * cv;
    const float sc = a.scale[b];
    const float ln = a.cls[b] + sc * con;
    const int t0 = s_i[1];
    a.constrain[b] = con;
    if (t0 >= 0 && t0 < a.max_steps) a.loss_rows[(int64_t)t0 * a.B + b] = ln;
    if (a.terms_out) {
      float* o = a.terms_out;
      o[b] = dis, o[a.B + b] = hd, o[2 * a.B + b] = cv, o[3 * a.B + b] = con, o[4 * a.B + b] = ln;
    }
    if (a.hd_arg_out) a.hd_arg_out[b] = has_hd ? mi : 0;
    // d (gval * loss_n) / d term, in pc3d_geoa3_terms_bwd_f32's order
    const float g_con = a.gval * sc;
    s_c[2] = a.w_dis * g_con;      // g_dis
    s_c[3] = a.w_hd * g_con;       // g_hd
    s_c[4] = a.w_curv * g_con;     // g_cv
    s_i[2] = has_hd ? mi : -1;
  }
  __syncthreads();

  // ---- 3a. the reverse indices ----
  if (curv) {
    gu_exclusive_scan(off, L, redi);
    const int total = L * k;
    for (int p = tid; p < L; p += kGuThreads) {
      const int32_t* nb = ib + (int64_t)p * K1;
      for (int e = 1; e < K1; ++e) {
        const int j = min(max(nb[e], 0), L - 1);
        const int pos = atomicAdd(off + j, 1);      // afterwards off[j] is the END of bucket j
        if (pos < total) rev[pos] = (uint16_t)p;
      }
    }
  }
  if (two) {
    gu_exclusive_scan(off2, L, redi);
    for (int p = tid; p < L; p += kGuThreads) {
      const int i = min(max(a.nn_oa[base1 + p], 0), L - 1);
      const int pos = atomicAdd(off2 + i, 1);
      if (pos < L) rev2[pos] = (uint16_t)p;
    }
  }
  __syncthreads();

  // ---- 3b / 4. gradient, Adam, lp_clip, the next iterate ----
  const AdamConsts ad = adam_consts_with(a.b1, a.b2, a.eps, s_c[0], s_c[1]);
  const float g_dis = s_c[2], g_hd = s_c[3], g_cv = s_c[4];
  const int hd_arg = s_i[2];
  const float inv_k = 1.f / (float)(k > 0 ? k : 1);
  for (int p = tid; p < L; p += kGuThreads) {
    const float px = sx[p], py = sy[p], pz = sz[p];
    float gx = 0.f, gy = 0.f, gz = 0.f;
    if (chamfer) {
      if (a.nn_ao != nullptr) {
        const int q = min(max(a.nn_ao[base1 + p], 0), L - 1);
        const float w = g_dis / (float)L + (p == hd_arg ? g_hd : 0.f);
        gx = 2.f * (px - og[q]) * w, gy = 2.f * (py - og[N + q]) * w, gz = 2.f * (pz - og[2 * N + q]) * w;
      }
      if (two) {
        const int s = p ? off2[p - 1] : 0, e = min(off2[p], L);
        gu_sort_bucket(rev2, s, e);
        const float w = g_dis / (float)L;
        for (int t = s; t < e; ++t) {
          const int j = rev2[t];
          gx += 2.f * (px - og[j]) * w, gy += 2.f * (py - og[N + j]) * w, gz += 2.f * (pz - og[2 * N + j]) * w;
        }
      }
    } else {
      gx = 2.f * (px - og[p]) * g_dis, gy = 2.f * (py - og[N + p]) * g_dis, gz = 2.f * (pz - og[2 * N + p]) * g_dis;
    }
    if (curv) {
      // own side: kappa_bwd_kernel's edge arithmetic, -sum to the point itself
      {
        const float ux = nx[p], uy = ny[p], uz = nz[p];
        const float gk = (g_cv * 2.f * kd[p] / (float)L) * inv_k;
        const int32_t* nb = ib + (int64_t)p * K1;
        float ox = 0.f, oy = 0.f, oz = 0.f;
        for (int e = 1; e < K1; ++e) {
          const int j = min(max(nb[e], 0), L - 1);
          const float dx = sx[j] - px, dy = sy[j] - py, dz = sz[j] - pz;
          const float nrm = sqrtf(dx * dx + dy * dy + dz * dz);
          const bool clamped = !(nrm > 1e-12f);
          const float len = clamped ? 1e-12f : nrm;
          const float vx = dx / len, vy = dy / len, vz = dz / len;
          const float dot = vx * ux + vy * uy + vz * uz;
          const float sg = dot > 0.f ? gk : (dot < 0.f ? -gk : 0.f);
          const float c = clamped ? 0.f : dot;      // the -v <v,n> term comes from d|d|/dd, which the clamp cuts
          ox += sg * (ux - vx * c) / len, oy += sg * (uy - vy * c) / len, oz += sg * (uz - vz * c) / len;
        }
        gx -= ox, gy -= oy, gz -= oz;
      }
      // neighbour side: the points that list p, ascending
      const int s = p ? off[p - 1] : 0, e = min(off[p], L * k);
      gu_sort_bucket(rev, s, e);
      for (int t = s; t < e; ++t) {
        const int i = rev[t];
        const float ux = nx[i], uy = ny[i], uz = nz[i];
        const float gk = (g_cv * 2.f * kd[i] / (float)L) * inv_k;
        const float dx = px - sx[i], dy = py - sy[i], dz = pz - sz[i];
        const float nrm = sqrtf(dx * dx + dy * dy + dz * dz);
        const bool clamped = !(nrm > 1e-12f);
        const float len = clamped ? 1e-12f : nrm;
        const float vx = dx / len, vy = dy / len, vz = dz / len;
        const float dot = vx * ux + vy * uy + vz * uz;
        const float sg = dot > 0.f ? gk : (dot < 0.f ? -gk : 0.f);
        const float c = clamped ? 0.f : dot;
        gx += sg * (ux - vx * c) / len, gy += sg * (uy - vy * c) / len, gz += sg * (uz - vz * c) / len;
      }
    }
    const float gt[3] = {a.g[base3 + p] + gx, a.g[base3 + N + p] + gy, a.g[base3 + 2 * N + p] + gz};
    float nw[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int64_t at = base3 + (int64_t)c * N + p;
      if (a.g_out) a.g_out[at] = gt[c];
      float mm = a.m[at], vv = a.v[at];
      nw[c] = adam_element(ad, a.offset[at], gt[c], mm, vv);
      a.m[at] = mm;
      a.v[at] = vv;
    }
    if (a.cc_linf != 0.f) {      // lp_clip (:92-102)
      const float len = __builtin_sqrtf((nw[0] * nw[0] + nw[1] * nw[1]) + nw[2] * nw[2]);
      if (!(len < a.cc_linf)) {
        const bool big = len > 1e-6f;
#pragma unroll
        for (int c = 0; c < 3; ++c) nw[c] = big ? nw[c] / len * a.cc_linf : 0.f;
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int64_t at = base3 + (int64_t)c * N + p;
      a.offset[at] = nw[c];
      const float xn = og[(int64_t)c * N + p] + nw[c];
      a.x[at] = xn;
      if constexpr (RAGGED) {
        if (p == 0) s_pad[c] = xn;      // thread 0 owns point 0
      }
    }
  }
  if constexpr (RAGGED) {
    // re-padding: x's rows from L on take the new point 0, through LDS behind the barrier (no thread re-reads global memory
    // another thread of the workgroup writes)
    __syncthreads();
    const float n0[3] = {s_pad[0], s_pad[1], s_pad[2]};
    float* xo = a.x + base3;
    for (int p = L + tid; p < N; p += kGuThreads) xo[p] = n0[0], xo[N + p] = n0[1], xo[2 * N + p] = n0[2];
  }
}

}  // namespace pc3d

using namespace pc3d;

// the checks, the argument block and the launch of both entries; lengths null: the dense kernel
static int geo_upd_launch(const char* nm, float* x, const float* ori, float* offset, const float* g, float* m, float* v, int B,
                          int N, int k, const int32_t* nn_ao, const int32_t* nn_oa, const int32_t* knn_idx,
                          const float* normal_ori, const float* kappa_ori, const float* cls, const float* scale,
                          const int64_t* pred, const int64_t* target, int targeted, int dis_kind, float gval, float w_dis,
                          float w_hd, float w_curv, float* constrain, float* loss_rows, int max_steps, int32_t* step,
                          const int32_t* search_step, double* lr, int scheduler, float* best_loss, float* best_attack,
                          int64_t* best_bs, int64_t* best_step, float* iter_best_loss, int64_t* iter_best_score, double beta1,
                          double beta2, double eps, float cc_linf, float* terms_out, int32_t* hd_arg_out, float* g_out,
                          const int32_t* lengths, bool ragged, void* stream) {
  PC3D_REQUIRE(B >= 0 && N >= 1 && N <= kGuMaxPoints, "%s: bad sizes B=%d N=%d (1 <= N <= %d)", nm, B, N, kGuMaxPoints);
  PC3D_REQUIRE(k >= 0 && k <= 63, "%s: k=%d out of range [0,63]", nm, k);
  PC3D_REQUIRE(dis_kind == 0 || dis_kind == 1, "%s: dis_kind=%d not in {0,1}", nm, dis_kind);
  PC3D_REQUIRE(max_steps >= 1, "%s: max_steps=%d", nm, max_steps);
  const bool curv = knn_idx != nullptr && k >= 1 && w_curv != 0.f;
  const bool two = dis_kind == 0 && nn_oa != nullptr;
  PC3D_REQUIRE(!curv || k + 1 <= N, "%s: k + 1 = %d neighbours of N=%d points", nm, k + 1, N);
  PC3D_REQUIRE(dis_kind == 0 || w_hd == 0.f, "%s: the L2 kind has no Hausdorff term", nm);
  const size_t lds = geo_upd_lds_bytes(N, k, curv, two);      // from the capacity: the lengths are device data
  PC3D_REQUIRE(lds <= kGuLdsLimit, "%s: N=%d, k=%d need %zu bytes of LDS (limit %zu)", nm, N, k, lds, kGuLdsLimit);
  if (B == 0) return PC3D_OK;
  PC3D_REQUIRE(!ragged || lengths != nullptr, "%s: null lengths", nm);
  PC3D_REQUIRE(x && ori && offset && g && m && v && cls && scale && pred && target && constrain && loss_rows && step &&
                   search_step && lr && best_loss && best_attack && best_bs && best_step && iter_best_loss && iter_best_score,
               "%s: null pointer", nm);
  PC3D_REQUIRE(dis_kind == 1 || nn_ao != nullptr, "%s: the Chamfer kind needs nn_ao", nm);
  PC3D_REQUIRE(!curv || (nn_ao && normal_ori && kappa_ori), "%s: the curvature term needs nn_ao, normal_ori and kappa_ori", nm);
  GeoUpdRaggedArgs a{};
  a.x = x, a.ori = ori, a.offset = offset, a.g = g, a.m = m, a.v = v, a.N = N, a.K1 = k + 1;
  a.nn_ao = nn_ao, a.nn_oa = nn_oa, a.knn_idx = knn_idx, a.normal_ori = normal_ori, a.kappa_ori = kappa_ori;
  a.cls = cls, a.scale = scale, a.pred = pred, a.target = target, a.targeted = targeted, a.dis_kind = dis_kind;
  a.gval = gval, a.w_dis = w_dis, a.w_hd = w_hd, a.w_curv = w_curv, a.constrain = constrain, a.loss_rows = loss_rows;
  a.max_steps = max_steps, a.B = B, a.step = step, a.search_step = search_step, a.lr = lr, a.scheduler = scheduler;
  a.best_loss = best_loss, a.best_attack = best_attack, a.best_bs = best_bs, a.best_step = best_step;
  a.iter_best_loss = iter_best_loss, a.iter_best_score = iter_best_score, a.b1 = beta1, a.b2 = beta2, a.eps = (float)eps;
  a.cc_linf = cc_linf, a.terms_out = terms_out, a.hd_arg_out = hd_arg_out, a.g_out = g_out, a.lengths = lengths;
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(ragged ? reinterpret_cast<const void*>(geoa3_update_kernel<true>)
                                              : reinterpret_cast<const void*>(geoa3_update_kernel<false>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)kGuLdsLimit);
    if (e != hipSuccess) {
      set_error("%s: LDS opt-in failed: %s", nm, hipGetErrorString(e));
      return (int)e;
    }
  }
  if (ragged)
    hipLaunchKernelGGL(geoa3_update_kernel<true>, dim3(B), dim3(kGuThreads), lds, as_stream(stream), a);
  else
    hipLaunchKernelGGL(geoa3_update_kernel<false>, dim3(B), dim3(kGuThreads), lds, as_stream(stream),
                       static_cast<const GeoUpdArgs&>(a));
  PC3D_LAUNCH_CHECK(nm);
  return PC3D_OK;
}

extern "C" int pc3d_geoa3_update_f32(float* x, const float* ori, float* offset, const float* g, float* m, float* v, int B,
                                     int N, int k, const int32_t* nn_ao, const int32_t* nn_oa, const int32_t* knn_idx,
                                     const float* normal_ori, const float* kappa_ori, const float* cls, const float* scale,
                                     const int64_t* pred, const int64_t* target, int targeted, int dis_kind, float gval,
                                     float w_dis, float w_hd, float w_curv, float* constrain, float* loss_rows,
                                     int max_steps, int32_t* step, const int32_t* search_step, double* lr, int scheduler,
                                     float* best_loss, float* best_attack, int64_t* best_bs, int64_t* best_step,
                                     float* iter_best_loss, int64_t* iter_best_score, double beta1, double beta2,
                                     double eps, float cc_linf, float* terms_out, int32_t* hd_arg_out, float* g_out,
                                     void* stream) {
  return geo_upd_launch("pc3d_geoa3_update_f32", x, ori, offset, g, m, v, B, N, k, nn_ao, nn_oa, knn_idx, normal_ori, kappa_ori,
                        cls, scale, pred, target, targeted, dis_kind, gval, w_dis, w_hd, w_curv, constrain, loss_rows, max_steps,
                        step, search_step, lr, scheduler, best_loss, best_attack, best_bs, best_step, iter_best_loss,
                        iter_best_score, beta1, beta2, eps, cc_linf, terms_out, hd_arg_out, g_out, nullptr, false, stream);
}

extern "C" int pc3d_geoa3_update_ragged_f32(float* x, const float* ori, float* offset, const float* g, float* m, float* v,
                                            int B, int N, int k, const int32_t* nn_ao, const int32_t* nn_oa,
                                            const int32_t* knn_idx, const float* normal_ori, const float* kappa_ori,
                                            const float* cls, const float* scale, const int64_t* pred, const int64_t* target,
                                            int targeted, int dis_kind, float gval, float w_dis, float w_hd, float w_curv,
                                            float* constrain, float* loss_rows, int max_steps, int32_t* step,
                                            const int32_t* search_step, double* lr, int scheduler, float* best_loss,
                                            float* best_attack, int64_t* best_bs, int64_t* best_step, float* iter_best_loss,
                                            int64_t* iter_best_score, double beta1, double beta2, double eps, float cc_linf,
                                            float* terms_out, int32_t* hd_arg_out, float* g_out, const int32_t* lengths,
                                            void* stream) {
  return geo_upd_launch("pc3d_geoa3_update_ragged_f32", x, ori, offset, g, m, v, B, N, k, nn_ao, nn_oa, knn_idx, normal_ori,
                        kappa_ori, cls, scale, pred, target, targeted, dis_kind, gval, w_dis, w_hd, w_curv, constrain, loss_rows,
                        max_steps, step, search_step, lr, scheduler, best_loss, best_attack, best_bs, best_step, iter_best_loss,
                        iter_best_score, beta1, beta2, eps, cc_linf, terms_out, hd_arg_out, g_out, lengths, true, stream);
}
