// The per-iteration update of the point-adding attacks (attack/Gen3DAdv: CWAdd, CWAddClusters) as ONE launch.
//
// The victim sees [ori | adv] (K + A points); only the A added points are optimised, and the distance the binary search
// keeps is a SET distance from the added points to the original cloud (attack/Gen3DAdv/IndpAdd_attack.py:159-162), not
// the L2 norm pc3d_cw_update_f32 keeps. Given the adv -> ori nearest-neighbour search of the current iterate (values
// d_i and arg-mins, pc3d_nn_f32) and the victim's input gradient on the A columns, one workgroup per sample:
//   1. reduces the set distance: Chamfer adv2ori = mean_i d_i, Hausdorff adv2ori = max_i d_i, or FarChamfer =
//      sum over clusters of the farthest intra-cluster pair ||a_y - a_x + 1e-7|| + cd_w * Chamfer (dist_utils.py);
//   2. updates the best-attack state on that distance (untargeted / targeted success as pc3d_cw_update_f32);
//   3. assembles the total gradient: the victim's + w_b * d(distance)/d(adv), where w_b is d loss / d distance_b
//      (the binary-search weight over the batch size);
//   4. applies Adam (no clip: the adding attacks take no clip functor) through the strided view of adv.
// Tie rules (they matter: resampled clusters contain duplicate points): Hausdorff routes its gradient to the FIRST
// maximal i; the farthest pair is the first maximum of torch's reduction order, inner max over x (first x), then over
// y (first y). Every reduction runs in a fixed order, so a run is bit-reproducible.
#include "update_body.h"

namespace pc3d {

constexpr int kAddThreads = 512;
constexpr int kAddWaves = kAddThreads / kWave;
constexpr int kAddMaxPoints = 2048;   // 4 points per thread in registers; the LDS copy for the pair term: 2 x 24 KiB
constexpr int kAddMaxCluster = 64;    // one wavefront per cluster

struct AddArgs {
  PtsViewMut adv;            // [B, A] points, a view into the victim's input (updated in place)
  PtsView ori;               // [B, K] points
  PtsView g;                 // [B, A] points: the victim's input gradient on the added columns
  int B, A, K;
  const float* nn_d;         // [B, A] squared distance of every added point to its nearest original point
  const int32_t* nn_idx;     // [B, A] index of that point
  const int64_t* pred;       // [B]
  const int64_t* label;      // [B]
  int untarget;
  float* bestdist;           // [B]
  int64_t* bestscore;        // [B]
  float* o_bestdist;         // [B]
  int64_t* o_bestscore;      // [B]
  float* o_bestattack;       // [B, 3, A] contiguous
  float* input_val;          // [B, 3, A] contiguous (may be null): the iterate this pass started from
  float* dist_val;           // [B] out (may be null): the set distance of that iterate
  float* m;                  // [B, 3, A] contiguous Adam state
  float* v;
  double lr, b1, b2;
  float eps;
  const int32_t* step_dev;
  int step_host;
  int kind;                  // 1 Chamfer, 2 Hausdorff, 3 FarChamfer
  const float* w;            // [B] d loss / d distance_b
  float cd_w;                // FarChamfer's Chamfer weight
  int P;                     // FarChamfer's points per cluster (A % P == 0, P <= 64)
};

// FAR: the FarChamfer instantiation; only it reserves the LDS copy of the points (the others keep ~100 B of LDS, so
// their residency is not capped by the pair term's 56 KiB)
template <int PER, bool FAR>
__global__ __launch_bounds__(kAddThreads) void add_update_kernel(AddArgs a) {
  constexpr int kL = FAR ? kAddMaxPoints : 1;
  __shared__ float s_px[kL], s_py[kL], s_pz[kL];
  __shared__ float s_fx[kL], s_fy[kL], s_fz[kL];
  __shared__ float s_cl[kL];   // farthest-pair value of every cluster
  __shared__ float s_part[kAddWaves];
  __shared__ int s_pidx[kAddWaves];
  __shared__ int s_copy, s_hidx;
  __shared__ float s_step_size, s_bc2s;
  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int A = a.A;
  constexpr bool far = FAR;
  const int64_t cb = (int64_t)b * 3 * A;   // the contiguous [B,3,A] buffers
  float px[PER], py[PER], pz[PER], qx[PER], qy[PER], qz[PER], gx[PER], gy[PER], gz[PER], dd[PER];
  float m_[PER][3], v_[PER][3];
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int k = tid + i * kAddThreads;
    if (k < A) {
      const float* p = a.adv.p + (int64_t)b * a.adv.bs + (int64_t)k * a.adv.ps;
      const float* gp = a.g.p + (int64_t)b * a.g.bs + (int64_t)k * a.g.ps;
      const int j = a.nn_idx[(int64_t)b * A + k];
      const float* q = a.ori.p + (int64_t)b * a.ori.bs + (int64_t)j * a.ori.ps;
      px[i] = p[0], py[i] = p[a.adv.cs], pz[i] = p[2 * a.adv.cs];
      gx[i] = gp[0], gy[i] = gp[a.g.cs], gz[i] = gp[2 * a.g.cs];
      qx[i] = q[0], qy[i] = q[a.ori.cs], qz[i] = q[2 * a.ori.cs];
      dd[i] = a.nn_d[(int64_t)b * A + k];
#pragma unroll
      for (int c = 0; c < 3; ++c) m_[i][c] = a.m[cb + (int64_t)c * A + k], v_[i][c] = a.v[cb + (int64_t)c * A + k];
      if (far) {
        s_px[k] = px[i], s_py[k] = py[i], s_pz[k] = pz[i];
        s_fx[k] = s_fy[k] = s_fz[k] = 0.f;
      }
    } else {
      px[i] = py[i] = pz[i] = qx[i] = qy[i] = qz[i] = gx[i] = gy[i] = gz[i] = 0.f;
      dd[i] = 0.f;
#pragma unroll
      for (int c = 0; c < 3; ++c) m_[i][c] = v_[i][c] = 0.f;
    }
  }
  // 1. the nearest-neighbour part of the distance: a sum (Chamfer, FarChamfer) or the first maximum (Hausdorff)
  if (a.kind == 2) {
    float best = -1.f;
    int bi = 0x7fffffff, unused = 0;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int k = tid + i * kAddThreads;
      if (k < A && dd[i] > best) best = dd[i], bi = k;   // k grows with i: strict > keeps the first
    }
    wave_argmax_first(best, bi, unused);
    if (lane == 0) s_part[wv] = best, s_pidx[wv] = bi;
  } else {
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < PER; ++i) acc += dd[i];
    acc = wave_sum(acc);
    if (lane == 0) s_part[wv] = acc;
  }
  __syncthreads();
  // 2. the farthest pair of every cluster, one wavefront per cluster: lane y scans x in order (first maximum over x),
  //    then the wavefront takes the first maximum over y. Its gradient +-u goes to (y*, x*); clusters are disjoint, so
  //    no two wavefronts touch the same point, and y* == x* cancels exactly as in autograd (u + (-u) = 0).
  if (far) {
    const int P = a.P, ncl = A / P;
    const float wb = a.w[b];
    for (int c = wv; c < ncl; c += kAddWaves) {
      const int base = c * P;
      float best = -1.f;
      int by = 0x7fffffff, bx = 0;
      if (lane < P) {
        const float ay = s_px[base + lane], by_ = s_py[base + lane], bz = s_pz[base + lane];
        by = lane;
        for (int x = 0; x < P; ++x) {
          const float dx = ay - s_px[base + x] + 1e-7f, dy = by_ - s_py[base + x] + 1e-7f, dz = bz - s_pz[base + x] + 1e-7f;
          const float n = __builtin_sqrtf(dx * dx + dy * dy + dz * dz);
          if (n > best) best = n, bx = x;
        }
      }
      wave_argmax_first(best, by, bx);
      if (lane == 0) {
        const int y = base + by, x = base + bx;
        s_cl[c] = best;
        const float dx = s_px[y] - s_px[x] + 1e-7f, dy = s_py[y] - s_py[x] + 1e-7f, dz = s_pz[y] - s_pz[x] + 1e-7f;
        const float gn = wb / best;   // d ||delta|| / d delta = delta / ||delta||, times the upstream weight
        const float ux = dx * gn, uy = dy * gn, uz = dz * gn;
        s_fx[y] += ux, s_fy[y] += uy, s_fz[y] += uz;
        s_fx[x] -= ux, s_fy[x] -= uy, s_fz[x] -= uz;
      }
    }
  }
  __syncthreads();
  // 3. the distance, the bookkeeping and the Adam bias corrections, once per sample
  if (tid == 0) {
    float dist;
    if (a.kind == 2) {
      float best = s_part[0];
      int bi = s_pidx[0];
      for (int w = 1; w < kAddWaves; ++w)
        if (s_part[w] > best || (s_part[w] == best && s_pidx[w] < bi)) best = s_part[w], bi = s_pidx[w];
      dist = best;
      s_hidx = bi;
    } else {
      float tot = 0.f;
      for (int w = 0; w < kAddWaves; ++w) tot += s_part[w];
      dist = tot / (float)A;
      if (far) {
        float fs = 0.f;
        for (int c = 0; c < A / a.P; ++c) fs += s_cl[c];
        dist = fs + dist * a.cd_w;
      }
    }
    s_copy = cw_book_decide(a.dist_val, a.bestdist, a.bestscore, a.o_bestdist, a.o_bestscore, a.untarget, b, dist,
                            a.pred[b], a.label[b], a.bestdist[b], a.o_bestdist[b]);
    const int t = a.step_dev ? a.step_dev[0] : a.step_host;
    s_step_size = adam_step_size(a.lr, a.b1, t);
    s_bc2s = adam_bc2s(a.b2, t);
  }
  __syncthreads();
  // 4. total gradient + Adam (adam_element, what pc3d_adam_clip_step_f32 runs; no clip), written back through adv's strides
  const bool copy = s_copy != 0;
  const float wb = a.w[b];
  // d distance / d a_i of the nearest-neighbour term: 2 (a_i - o_nn(i)) times cc (Chamfer: 1/A of the mean)
  const float cc = (a.kind == 2) ? 2.f * wb : 2.f * (wb * (far ? a.cd_w : 1.f)) / (float)A;
  const int hidx = (a.kind == 2) ? s_hidx : -1;
  const AdamConsts ad = adam_consts_with(a.b1, a.b2, a.eps, s_step_size, s_bc2s);
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int k = tid + i * kAddThreads;
    if (k >= A) continue;
    const float pin[3] = {px[i], py[i], pz[i]};
    if (a.input_val) {
#pragma unroll
      for (int c = 0; c < 3; ++c) a.input_val[cb + (int64_t)c * A + k] = pin[c];
    }
    if (copy) {
#pragma unroll
      for (int c = 0; c < 3; ++c) a.o_bestattack[cb + (int64_t)c * A + k] = pin[c];
    }
    float gd[3] = {0.f, 0.f, 0.f};
    if (a.kind != 2 || k == hidx) {
      gd[0] = cc * (px[i] - qx[i]);
      gd[1] = cc * (py[i] - qy[i]);
      gd[2] = cc * (pz[i] - qz[i]);
    }
    if (far) gd[0] += s_fx[k], gd[1] += s_fy[k], gd[2] += s_fz[k];
    const float g[3] = {gx[i] + gd[0], gy[i] + gd[1], gz[i] + gd[2]};
    float* pp = a.adv.p + (int64_t)b * a.adv.bs + (int64_t)k * a.adv.ps;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      pp[c * a.adv.cs] = adam_element(ad, pin[c], g[c], m_[i][c], v_[i][c]);
      a.m[cb + (int64_t)c * A + k] = m_[i][c];
      a.v[cb + (int64_t)c * A + k] = v_[i][c];
    }
  }
}

template <bool FAR>
static void launch_add(const AddArgs& a, int B, int A, hipStream_t st) {
  if (A <= kAddThreads) hipLaunchKernelGGL((add_update_kernel<1, FAR>), dim3(B), dim3(kAddThreads), 0, st, a);
  else if (A <= 2 * kAddThreads) hipLaunchKernelGGL((add_update_kernel<2, FAR>), dim3(B), dim3(kAddThreads), 0, st, a);
  else hipLaunchKernelGGL((add_update_kernel<4, FAR>), dim3(B), dim3(kAddThreads), 0, st, a);
}

}  // namespace pc3d

using namespace pc3d;

extern "C" int pc3d_add_update_f32(float* adv, int64_t a_bs, int64_t a_ps, int64_t a_cs,
                                   const float* ori, int64_t o_bs, int64_t o_ps, int64_t o_cs, int B, int A, int K,
                                   const float* nn_d, const int32_t* nn_idx, const int64_t* pred, const int64_t* label,
                                   int untarget, float* bestdist, int64_t* bestscore, float* o_bestdist,
                                   int64_t* o_bestscore, float* o_bestattack, float* input_val, float* dist_val,
                                   const float* g, int64_t g_bs, int64_t g_ps, int64_t g_cs, float* m, float* v,
                                   double lr, double beta1, double beta2, double eps, const int32_t* step_dev,
                                   int step_host, int kind, const float* w, float cd_w, int P, void* stream) {
  PC3D_REQUIRE(B >= 0 && A >= 1 && A <= kAddMaxPoints && K >= 1,
               "pc3d_add_update_f32: bad sizes B=%d A=%d K=%d (1 <= A <= %d)", B, A, K, kAddMaxPoints);
  PC3D_REQUIRE(kind >= 1 && kind <= 3, "pc3d_add_update_f32: kind=%d not in {1,2,3}", kind);
  PC3D_REQUIRE(kind != 3 || (P >= 1 && P <= kAddMaxCluster && A % P == 0),
               "pc3d_add_update_f32: clusters of P=%d points must tile A=%d (1 <= P <= %d)", P, A, kAddMaxCluster);
  PC3D_REQUIRE(step_dev != nullptr || step_host >= 1, "pc3d_add_update_f32: step_host must be >= 1 without a device counter");
  if (B == 0) return PC3D_OK;
  PC3D_REQUIRE(adv && ori && nn_d && nn_idx && pred && label && bestdist && bestscore && o_bestdist && o_bestscore &&
               o_bestattack && g && m && v && w, "pc3d_add_update_f32: null pointer");
  AddArgs a{};
  a.adv = PtsViewMut{adv, a_bs, a_ps, a_cs};
  a.ori = PtsView{ori, o_bs, o_ps, o_cs};
  a.g = PtsView{g, g_bs, g_ps, g_cs};
  a.B = B, a.A = A, a.K = K;
  a.nn_d = nn_d, a.nn_idx = nn_idx, a.pred = pred, a.label = label, a.untarget = untarget;
  a.bestdist = bestdist, a.bestscore = bestscore, a.o_bestdist = o_bestdist, a.o_bestscore = o_bestscore;
  a.o_bestattack = o_bestattack, a.input_val = input_val, a.dist_val = dist_val, a.m = m, a.v = v;
  a.lr = lr, a.b1 = beta1, a.b2 = beta2, a.eps = (float)eps, a.step_dev = step_dev, a.step_host = step_host;
  a.kind = kind, a.w = w, a.cd_w = cd_w, a.P = (kind == 3) ? P : 1;
  if (kind == 3) launch_add<true>(a, B, A, as_stream(stream));
  else launch_add<false>(a, B, A, as_stream(stream));
  PC3D_LAUNCH_CHECK("pc3d_add_update_f32");
  return PC3D_OK;
}
