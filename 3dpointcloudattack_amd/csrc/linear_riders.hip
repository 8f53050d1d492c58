// Riders: pieces of the CW iteration that do not sit on the victim's dependency chain, carried as EXTRA WORKGROUPS of a
// small-batch linear launch that exists anyway (a head layer keeps 16-64 of the 256 CUs busy, and a launch of its own
// inside a replayed graph costs ~4.5 us before it does anything). No cross-workgroup hand-off, no second stream, no
// graph branch: the first workgroups run linear16_body (dispatched first: the chain waits for them), the rest run the
// rider, and the two never touch the same memory.
//   pc3d_linear_nn_f32   linear + the adv -> ori nearest-neighbour search (nn_body<1, 8>)
//   pc3d_linear_book_f32 linear + the per-sample bookkeeping of the CW update (cw_book_body) and the Adam factors
// Built WITHOUT nn.o's -fno-honor-nans: the linear epilogue's `s > 0.f` / `!(gate > 0.f)` keep their NaN semantics.
#include "pc3d_common.h"
#include "cw_update_body.h"
#include "linear16_body.h"
#include "nn_body.h"

namespace pc3d {

template <int TR, int TC>
__global__ __launch_bounds__(LN_T) void linear16_nn_kernel(LinArgs a, int lin_gx, int lin_wgs, NNDir D, int mt_cap,
                                                           int nn_gx, int nn_total) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int wg = blockIdx.x;
  if (wg < lin_wgs) {
    const int by = wg / lin_gx;
    linear16_body<TR, TC>(a, wg - by * lin_gx, by);
    return;
  }
  // a cloud's search workgroups on one XCD (ids are dealt round-robin to the XCDs: a constant offset keeps the bands)
  const int t = xcd_band_id(wg - lin_wgs, nn_total);
  if (t < 0) return;
  const int b = t / nn_gx;
  nn_body<1, 8>(D, mt_cap, t - b * nn_gx, b, lds);
}

// Reference points up to which the search rides: the staged tile (12 B per point) + the merge area + the layer's 17 KB
// (the 32 x 16 form's `red`; 8.5 / 4.5 / 2.25 KB for 16 x 16 / 16 x 8 / 8 x 8, so the smaller tiles only add room)
// stay under 64 KB per workgroup, so two workgroups share a CU as the stand-alone layer's do. Larger clouds (one tile up
// to kNNMaxTile = 4096 points) keep the search's own launch.
constexpr int kRiderMaxRef = 2048;

struct BookRiderArgs {
  BookArgs bk;
  double lr, b1, b2;
  const int32_t* step_dev;
  float* adam;     // [2] out: {step_size, bc2s} of the step word's value, or null
};

template <int TR, int TC>
__global__ __launch_bounds__(LN_T) void linear16_book_kernel(LinArgs a, int lin_gx, int lin_wgs, BookRiderArgs r) {
  static_assert(kCwBookThreads == LN_T, "the bookkeeping rider is written for the linear launch's workgroup size");
  const int wg = blockIdx.x;
  if (wg < lin_wgs) {
    const int by = wg / lin_gx;
    linear16_body<TR, TC>(a, wg - by * lin_gx, by);
    return;
  }
  cw_book_body(r.bk, wg - lin_wgs, r.lr, r.b1, r.b2, r.step_dev, r.adam);
}

// the bookkeeping alone (the host layer does not take the 32 x 16 tiling)
__global__ __launch_bounds__(LN_T) void cw_book_kernel(BookRiderArgs r) {
  cw_book_body(r.bk, blockIdx.x, r.lr, r.b1, r.b2, r.step_dev, r.adam);
}

}  // namespace pc3d

using namespace pc3d;

extern "C" int pc3d_linear_nn_f32(const float* X, int ldx, int P, int B, int K, const float* W, const float* bias, int O,
                                  int relu, float slope, const float* gate, int ldg, float gate_slope, float* Y, int ldy,
                                  const float* q, int64_t q_bs, int64_t q_ps, int64_t q_cs,
                                  const float* r, int64_t r_bs, int64_t r_ps, int64_t r_cs,
                                  int NB, int N, int M, float* min_d2, int32_t* idx, int ride, int tile, void* stream) {
  // the search's own checks (as pc3d_nn_f32); the linear's are made by pc3d_linear_f32 below or repeated here
  PC3D_REQUIRE(NB >= 0 && N >= 0 && M >= 1, "pc3d_linear_nn_f32: bad sizes NB=%d N=%d M=%d (M must be >= 1)", NB, N, M);
  PC3D_REQUIRE(tile >= 0 && tile <= kLinTileForms, "pc3d_linear_nn_f32: tile=%d names no form (0 = the rule, 1..%d)", tile,
               kLinTileForms);
  int Q = 0, waves = 0;
  if (NB > 0 && N > 0) nn_plan(N, M, NB, 1, &Q, &waves);
  const bool fits = ride && B > 0 && NB > 0 && N > 0 && K >= 1 && O >= 1 && P >= 1 && linear16_applies(K, P, O) &&
                    waves == 8 && M <= kRiderMaxRef;
  if (!fits) {   // outside the rider's range: the two existing launches
    const int rc = pc3d_linear_f32(X, ldx, P, B, K, W, bias, O, relu, slope, gate, ldg, gate_slope, Y, ldy, tile, stream);
    if (rc != PC3D_OK) return rc;
    return pc3d_nn_f32(q, q_bs, q_ps, q_cs, r, r_bs, r_ps, r_cs, NB, N, M, min_d2, idx, stream);
  }
  PC3D_REQUIRE(ldx >= P * K && ldy >= O, "pc3d_linear_nn_f32: leading dimensions too small (ldx=%d ldy=%d)", ldx, ldy);
  PC3D_REQUIRE(ldx % 4 == 0, "pc3d_linear_nn_f32: ldx=%d must be a multiple of 4 for 16-byte loads", ldx);
  PC3D_REQUIRE(X && W && Y && q && r, "pc3d_linear_nn_f32: null pointer");
  PC3D_REQUIRE(gate == nullptr || ldg >= O, "pc3d_linear_nn_f32: ldg=%d too small", ldg);
  PC3D_REQUIRE(NB <= 65535, "pc3d_linear_nn_f32: NB=%d exceeds the search's batch limit 65535", NB);
  LinArgs a{X, ldx, P, W, bias, gate, ldg, Y, ldy, B, K, O, relu, slope, gate_slope};
  const NNDir D{{q, q_bs, q_ps, q_cs}, {r, r_bs, r_ps, r_cs}, N, M, min_d2, idx};
  int mt_cap;
  const size_t lds = nn_lds_bytes(M, 1, 8, &mt_cap);
  const int form = linear_tile_pick(tile, B, K, O);
  int tr = 32, tc = 16;
  linear_tile_dims(form, &tr, &tc);
  const int lin_gx = cdiv(O, tc), lin_wgs = lin_gx * cdiv(B, tr);   // the layer's workgroups stay first in dispatch order
  const int nn_gx = cdiv(N, kWave), nn_total = nn_gx * NB;
  PC3D_LIN_TILE_SWITCH(form, hipLaunchKernelGGL((linear16_nn_kernel<TR, TC>), dim3(lin_wgs + xcd_grid(nn_total)), dim3(LN_T),
                                                lds, as_stream(stream), a, lin_gx, lin_wgs, D, mt_cap, nn_gx, nn_total));
  PC3D_LAUNCH_CHECK("pc3d_linear_nn_f32");
  return PC3D_OK;
}

extern "C" int pc3d_linear_book_f32(const float* X, int ldx, int P, int B, int K, const float* W, const float* bias, int O,
                                    int relu, float slope, const float* gate, int ldg, float gate_slope, float* Y, int ldy,
                                    const float* adv, int64_t a_bs, int64_t a_ps, int64_t a_cs,
                                    const float* ori, int64_t o_bs, int64_t o_ps, int64_t o_cs, int NB, int NK,
                                    const int64_t* pred, const int64_t* label, int untarget,
                                    float* bestdist, int64_t* bestscore, float* o_bestdist, int64_t* o_bestscore,
                                    float* o_bestattack, float* input_val, float* dist_val,
                                    double lr, double beta1, double beta2, const int32_t* step_dev, float* adam,
                                    int ride, int tile, void* stream) {
  PC3D_REQUIRE(NB >= 0 && NK >= 1 && NK <= 8192, "pc3d_linear_book_f32: bad sizes NB=%d NK=%d (NK <= 8192)", NB, NK);
  PC3D_REQUIRE(adam == nullptr || step_dev != nullptr, "pc3d_linear_book_f32: the Adam factors need the device step word");
  PC3D_REQUIRE(tile >= 0 && tile <= kLinTileForms, "pc3d_linear_book_f32: tile=%d names no form (0 = the rule, 1..%d)", tile,
               kLinTileForms);
  PC3D_REQUIRE(NB == 0 || (adv && ori && pred && label && bestdist && bestscore && o_bestdist && o_bestscore && o_bestattack),
               "pc3d_linear_book_f32: null pointer");
  // o_bestattack / input_val share adv's layout (as pc3d_cw_update_f32)
  BookRiderArgs r{BookArgs{{adv, a_bs, a_ps, a_cs}, {ori, o_bs, o_ps, o_cs}, NK, pred, label, untarget, bestdist, bestscore,
                           o_bestdist, o_bestscore, {o_bestattack, a_bs, a_ps, a_cs}, {input_val, a_bs, a_ps, a_cs},
                           dist_val, nullptr},
                  lr, beta1, beta2, step_dev, adam};
  const bool fits = ride && B > 0 && NB > 0 && K >= 1 && O >= 1 && P >= 1 && linear16_applies(K, P, O);
  if (!fits) {
    const int rc = pc3d_linear_f32(X, ldx, P, B, K, W, bias, O, relu, slope, gate, ldg, gate_slope, Y, ldy, tile, stream);
    if (rc != PC3D_OK || NB == 0) return rc;
    hipLaunchKernelGGL(cw_book_kernel, dim3(NB), dim3(LN_T), 0, as_stream(stream), r);
    PC3D_LAUNCH_CHECK("pc3d_linear_book_f32/book");
    return PC3D_OK;
  }
  PC3D_REQUIRE(ldx >= P * K && ldy >= O, "pc3d_linear_book_f32: leading dimensions too small (ldx=%d ldy=%d)", ldx, ldy);
  PC3D_REQUIRE(ldx % 4 == 0, "pc3d_linear_book_f32: ldx=%d must be a multiple of 4 for 16-byte loads", ldx);
  PC3D_REQUIRE(X && W && Y, "pc3d_linear_book_f32: null pointer");
  PC3D_REQUIRE(gate == nullptr || ldg >= O, "pc3d_linear_book_f32: ldg=%d too small", ldg);
  LinArgs a{X, ldx, P, W, bias, gate, ldg, Y, ldy, B, K, O, relu, slope, gate_slope};
  // tile 0 is 32 x 16 here, not the rule: this launch lasts as long as its bookkeeping workgroups, which start behind the
  // layer's — at the step's shape (B = 32, 256 -> 512) no smaller tile measured faster and 8 x 8 (256 workgroups in front
  // of the bookkeeping) measured 19 % slower (profiles/linear_tiles_bench.json)
  const int form = tile == 0 ? 1 : tile;
  int tr = 32, tc = 16;
  linear_tile_dims(form, &tr, &tc);
  const int lin_gx = cdiv(O, tc), lin_wgs = lin_gx * cdiv(B, tr);
  PC3D_LIN_TILE_SWITCH(form, hipLaunchKernelGGL((linear16_book_kernel<TR, TC>), dim3(lin_wgs + NB), dim3(LN_T), 0,
                                                as_stream(stream), a, lin_gx, lin_wgs, r));
  PC3D_LAUNCH_CHECK("pc3d_linear_book_f32");
  return PC3D_OK;
}
