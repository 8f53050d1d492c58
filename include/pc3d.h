/*
 * pc3d.h — C-ABI of libpc3d_hip.so, the MI355X (gfx950) point-set kernel library behind the
 * attack-iteration hot path of LI-Yiquan/3DPointCloudAttack.
 *
 * Conventions (all entry points):
 *   - every pointer is a CALLER-OWNED DEVICE buffer (e.g. torch.Tensor.data_ptr()); the library allocates
 *     nothing and keeps no mutable global state besides a thread-local error string;
 *   - work is enqueued on `stream` (a hipStream_t passed as void*; NULL = the null stream) and the call
 *     returns before completion; nothing inside synchronises, so every entry point is hipGraph-capturable;
 *   - return value 0 = ok; >0 = hipError_t of the failing runtime call; <0 = argument error
 *     (PC3D_EINVAL). No C++ exception crosses the boundary. pc3d_last_error() gives the text.
 *   - point sets are fp32 and addressed by ELEMENT strides (batch, point, channel) so both reference
 *     layouts are zero-copy: [B,N,3] is (3N,3,1); [B,3,N] is (3N,1,N).
 *   - indices are int32 on the wire (N < 2^31); the Python mirror widens to int64 where the reference
 *     returns LongTensors.
 *
 * The reference has one FFI precedent whose style this follows: `extern "C" void render_ball(...)` loaded
 * with ctypes and fed raw caller-owned buffers (reference utils/render_balls_so.cpp:12-14,
 * utils/show3d_balls.py:22,80-84). Each function below names the reference code it replaces.
 */
#ifndef PC3D_H
#define PC3D_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PC3D_OK 0
#define PC3D_EINVAL (-22)

/* Library version (major*10000 + minor*100 + patch). */
int pc3d_version(void);
/* Thread-local text of the last non-zero return on this thread ("" if none). */
const char* pc3d_last_error(void);

/* ---------------------------------------------------------------------------------------------------------
 * K1  nearest neighbour of every query point in a reference set (squared L2, direct-difference form).
 *   min_d2[b,i] = min_j |q[b,i,:]-r[b,j,:]|^2 ; idx[b,i] = lowest j attaining it.
 * Replaces the [B,N,M] materialisations + min() of
 *   attack/CW/CW_utils/distance.py:15-32,40-50,58-70 (batch_pairwise_dist + ChamferDistance/HausdorffDistance),
 *   utils/dis_utils_torch.py:8-28 (cdist + min), utils/dis_utils_numpy.py:13-38 (scipy distance_matrix + min),
 *   attack/GeoA3/knn_utils.py:10-20 with K=1 (attack/GeoA3/loss_utils.py:36-58).
 * q: B x N points, r: B x M points, strides in elements. min_d2: [B,N] f32, idx: [B,N] i32 (either may be NULL).
 * ------------------------------------------------------------------------------------------------------- */
int pc3d_nn_f32(const float* q, int64_t q_bs, int64_t q_ps, int64_t q_cs,
                const float* r, int64_t r_bs, int64_t r_ps, int64_t r_cs,
                int B, int N, int M, float* min_d2, int32_t* idx, void* stream);
/* pc3d_nn_f32 that also writes the indices as int64 (idx64 [B,N], may be NULL; idx may be NULL too): the pytorch3d-style
 * knn_points of attack/GeoA3/knn_utils.py:22-55 returns int64 indices — written here instead of by a conversion launch. */
int pc3d_nn_i64_f32(const float* q, int64_t q_bs, int64_t q_ps, int64_t q_cs,
                    const float* r, int64_t r_bs, int64_t r_ps, int64_t r_cs,
                    int B, int N, int M, float* min_d2, int32_t* idx, int64_t* idx64, void* stream);


/* Both directions in ONE launch (grid.z = 2): a->b into (dA,iA) [B,N]; b->a into (dB,iB) [B,M]. */
int pc3d_nn_bidir_f32(const float* a, int64_t a_bs, int64_t a_ps, int64_t a_cs,
                      const float* b, int64_t b_bs, int64_t b_ps, int64_t b_cs,
                      int B, int N, int M,
                      float* dA, int32_t* iA, float* dB, int32_t* iB, void* stream);

/* Both directions from ONE evaluation of every distance (the two-scan form above computes each d(a_i,b_j) twice):
 * a workgroup keeps 64*Q points of `a` in registers, scans a range of `b` from LDS, takes the row minima as before
 * and reduces the column minima across the lanes with a halving butterfly (v_permlane32/16_swap + DPP); what one
 * workgroup cannot finish (column minima per tile of `a`; row minima when `b` is split to fill the chip) goes through
 * the caller's workspace and is folded by a second, small launch. Same results as pc3d_nn_bidir_f32, bit for bit
 * (distances; indices = lowest index attaining the minimum). Replaces the same reference code as pc3d_nn_f32 for the
 * callers that need both directions: distance.py:40-50,58-70 (ChamferDistance/HausdorffDistance return both),
 * utils/dis_utils_numpy.py:23-38, utils/dis_utils_torch.py:14-28, attack/GeoA3/loss_utils.py:36-46.
 * ws: device scratch of at least pc3d_nn_bidir_shared_ws_bytes(B,N,M) bytes, 16-byte aligned, owned by the caller,
 * free to reuse once the stream has passed this call. dA/iA/dB/iB: any may be NULL. */
int64_t pc3d_nn_bidir_shared_ws_bytes(int B, int N, int M);
int pc3d_nn_bidir_shared_f32(const float* a, int64_t a_bs, int64_t a_ps, int64_t a_cs,
                             const float* b, int64_t b_bs, int64_t b_ps, int64_t b_cs,
                             int B, int N, int M,
                             float* dA, int32_t* iA, float* dB, int32_t* iB,
                             void* ws, int64_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * K8b  point-wise dense layer on fp32 MFMA:  Y[M,N] = act( gate(X)[M,K] . W[N,K]^T + bias[N] ).
 * Replaces the library GEMM + activation passes of the shared MLPs of PointNet++ set abstraction
 * (model/pointnet2_utils.py:190-197,243-257), DGCNN's EdgeConv products and conv5 (model/dgcnn.py:297-320) and
 * CurveNet's 1x1 convolutions (model/curvenet_util.py:189-193,321-331), with eval BatchNorm folded into W / bias.
 * Backward to the input (frozen weights, no weight gradient): the same entry point on W^T with X = dY and
 * gate = the layer's output Y:  dX = (dY * act'(Y)) . W   (gate_slope = 0 for ReLU, = slope for LeakyReLU).
 * X: [M,K] row stride ldx; W: [N,K] row-major; bias [N] or NULL; gate [M,K] row stride ldg or NULL (X is then read
 * as gate > 0 ? X : gate_slope * X); act: 0 none, 1 ReLU, 2 LeakyReLU(slope); Y: [M,N] row stride ldy. Exact fp32
 * (v_mfma_f32_32x32x2_f32). Any M, N, K >= 1.
 * ------------------------------------------------------------------------------------------------------- */
int pc3d_gemm_nt_f32(const float* X, int64_t ldx, const float* W, const float* bias, const float* gate, int64_t ldg,
                     float gate_slope, int M, int N, int K, int act, float slope, float* Y, int64_t ldy, void* stream);
/* The same product with an EXPLICIT tiling. pc3d_gemm_nt_f32 picks its tile shape from (N, K) alone and sums every
 * output element's products in ascending k — its result for a row never depends on how many rows share the launch.
 * variant: 0 / 1 128x128 tiles, 4 waves (double / single buffered); 2 128x64 (N <= 64); 3 256x64; 4 64x128; 5 / 6
 * 128x128, 8 waves (single / double buffered); 8 as 5 with four workgroups per CU; 11: 64x64 tiles with the K steps
 * split over two groups of waves, 12: 32x64 tiles with four K groups — for launches with few tiles and a long K
 * (CurveNet's deep levels); the K split sums an element's products in a different (fixed) order, so a caller chooses
 * it from per-cloud shapes, not from the batch (ops.gemm_variant). Anything else: PC3D_EINVAL. */
int pc3d_gemm_nt_tiled_f32(const float* X, int64_t ldx, const float* W, const float* bias, const float* gate,
                           int64_t ldg, float gate_slope, int M, int N, int K, int act, float slope, float* Y,
                           int64_t ldy, int variant, void* stream);
/* The same layer with a residual branch summed in before the activation:  Y = act(X . W^T + bias + R)  — the tail
 * of a CurveNet CIC block, relu(conv2(..) + shortcut) (model/curvenet_util.py:372-376). R: [M,N] row stride ldr.
 * Its backward: G = pc3d_gate_f32(dY, Y) once, then dR = G and dX = pc3d_gemm_nt_f32(G, W^T). */
int pc3d_gemm_nt_res_f32(const float* X, int64_t ldx, const float* W, const float* bias, const float* R, int64_t ldr,
                         int M, int N, int K, int act, float slope, float* Y, int64_t ldy, int variant, void* stream);
/* (variant: < 0 = the default tiling, else as pc3d_gemm_nt_tiled_f32) */
/* out[i] = y[i] > 0 ? g[i] : slope * g[i] over n contiguous floats (16-byte aligned buffers): the derivative of a
 * (Leaky)ReLU taken from its OUTPUT's sign, for layers whose pre-activation had more than one producer. */
int pc3d_gate_f32(const float* g, const float* y, int64_t n, float slope, float* out, void* stream);

/* Point normals from the k-NN covariance (attack/GeoA3/utility.py:43-92 estimate_normal): eigenvector of the smallest
 * eigenvalue of the 3 x 3 covariance of the k neighbours (closed form, double arithmetic), sign fixed against the
 * summed centred neighbours (:73-75). Replaces a batched 3 x 3 symeig (rocsolver: 5 ms per call at B=32, N=1024).
 * x: [B,N] points (element strides); idx: [B,N,K1] int32 neighbour lists with the point itself first (K1 = k + 1,
 * as pc3d_knn_f32 returns them for a self-query); out: [B,N] normals (element strides). */
int pc3d_estimate_normal_f32(const float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs, const int32_t* idx,
                             int B, int N, int K1, float* out, int64_t o_bs, int64_t o_ps, int64_t o_cs, void* stream);
/* GeoA3's curvature proxy (attack/GeoA3/loss_utils.py:60-90): kappa[b,i] = mean over the k = K1 - 1 neighbours j
 * (idx[b,i,1:], the first entry is the point itself) of |<(p_j - p_i) / max(|p_j - p_i|, 1e-12), n_i>|, and its
 * backward to the points (gx [B,N,3] contiguous, overwritten; float atomics). x, nrm: [B,N] points / normals with
 * element strides; idx [B,N,K1] int32. One launch each way instead of ~30. */
int pc3d_kappa_f32(const float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs, const float* nrm, int64_t n_bs, int64_t n_ps,
                   int64_t n_cs, const int32_t* idx, int B, int N, int K1, float* out, void* stream);
/* pc3d_kappa_f32 with the normals taken THROUGH an index: point i uses normal nidx[b,i] of the M source normals (nrm
 * [B,M] with element strides; the reference gathers the nearest original point's normal first, loss_utils.py:72-82) and
 * the normals used are written to nout [B,3,N] (contiguous, channels first) — what pc3d_kappa_bwd_f32 then takes. */
int pc3d_kappa_gather_f32(const float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs, const float* nrm, int64_t n_bs,
                          int64_t n_ps, int64_t n_cs, int M, const int64_t* nidx, const int32_t* idx, int B, int N, int K1,
                          float* out, float* nout, void* stream);
int pc3d_kappa_bwd_f32(const float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs, const float* nrm, int64_t n_bs,
                       int64_t n_ps, int64_t n_cs, const int32_t* idx, const float* gout, int B, int N, int K1, float* gx,
                       int deterministic, void* stream);
/* (deterministic = 1: every wavefront accumulates into its own LDS slab and the slabs are combined in a fixed order —
 * bit-identical gradients run to run and for a cloud alone or inside a batch; 0: slabs shared by the wavefronts / global
 * float atomics, order-dependent in the last bits. (3 + 4) N floats of LDS, N <= 8192.) */

/* GeoA3's per-sample loss assembly as one launch each way (attack/GeoA3/GeoA3_attack.py:139-181 on top of
 * loss_utils.py:36-58,92-105): from the adv->ori nearest-neighbour squared distances d_ao [B,N] (and indices idx_ao
 * [B,N] int64), the ori->adv distances d_oa [B,M] (NULL = pseudo-Chamfer), the curvature proxies k_adv [B,N] / k_ori
 * [B,M] (both NULL = no curvature term), the classification loss cls [B] and the trade-off constants scale [B]:
 *   out[0,b] dis  = mean d_ao (+ mean d_oa)     out[1,b] hd = max d_ao     out[2,b] curv = mean (k_adv - k_ori[idx_ao])^2
 *   out[3,b] constrain = w_dis dis + w_hd hd + w_curv curv                 out[4,b] loss_n = cls + scale constrain
 * out [5,B]; hd_arg [B] int32 = first arg-max of d_ao (where torch.max routes the gradient). The backward takes the
 * upstream gradients of all five outputs (g_out [5,B]) and overwrites g_d_ao [B,N], g_d_oa [B,M] (may be NULL),
 * g_k_adv [B,N] (may be NULL) and g_cls [B]. */
int pc3d_geoa3_terms_f32(const float* d_ao, const float* d_oa, const float* k_adv, const float* k_ori,
                         const int64_t* idx_ao, const float* cls, const float* scale, int B, int N, int M, float w_dis,
                         float w_hd, float w_curv, float* out, int32_t* hd_arg, void* stream);
int pc3d_geoa3_terms_bwd_f32(const float* g_out, const float* k_adv, const float* k_ori, const int64_t* idx_ao,
                             const float* scale, const int32_t* hd_arg, int B, int N, int M, float w_dis, float w_hd,
                             float w_curv, float* g_d_ao, float* g_d_oa, float* g_k_adv, float* g_cls, void* stream);

/* Best-attack bookkeeping of one GeoA3 iteration in one launch (attack/GeoA3/GeoA3_attack.py:307-330): label_out[b] =
 * first arg-max of logits[b,:] (NaN counts as the maximum, like torch.argmax); success = (label == target[b]) when
 * targeted, (label != target[b]) otherwise; where success and metric[b] < best_loss[b]: best_loss, best_bs = search_step,
 * best_step = step and best_attack[b,:] = iterate[b,:] (n3 floats per sample, contiguous); where success and metric[b] <
 * iter_best_loss[b]: iter_best_loss and iter_best_score = label. All state is updated in place. */
int pc3d_geoa3_record_f32(const float* logits, int ld, int B, int ncls, const int64_t* target, int targeted,
                          const float* metric, const float* iterate, int n3, int64_t search_step, int64_t step,
                          float* best_loss, float* best_attack, int64_t* best_bs, int64_t* best_step,
                          float* iter_best_loss, int64_t* iter_best_score, int64_t* label_out, void* stream);

/* First layer of a set-abstraction MLP without the grouped input tensor (model/pointnet2_utils.py:118-135,190-197): the
 * layer is linear in [x_j - c_s ; f_j], so  W1 [x_j - c_s ; f_j] + b1 = P[idx[s,j]] + Bc[s]  with P = [x | f] W1^T per
 * POINT (B*NA rows, pc3d_gemm_nt_f32) and Bc[s] = b1 - (Wx x)[centroid s].
 *   pc3d_group_act_f32     : H[b,s,j,:] = act(P[b,idx[b,s,j],:] + Bc[b,s,:])   act = LeakyReLU(slope), slope 0 = ReLU
 *   pc3d_group_act_bwd_f32 : gP[b,idx] += g', gBc[b,s] = sum_j g'  with g' = act'(H) gH (gP is zero-filled here; float
 *                            atomics, ball-query padding merged on chip).
 * P [B,NA,C], Bc [B,S,C], idx [B,S,K] int32 (outside [0,NA): zero row / no gradient), H, gH [B,S,K,C]; C % 4 == 0,
 * C <= 512 for the backward. */
int pc3d_group_act_f32(const float* P, const float* Bc, const int32_t* idx, int B, int NA, int S, int K, int C,
                       float slope, float* H, void* stream);
int pc3d_group_act_bwd_f32(const float* gH, const float* H, const int32_t* idx, int B, int NA, int S, int K, int C,
                           float slope, float* gP, float* gBc, int deterministic, void* stream);
/* (deterministic = 1: gP through the ordered LDS scatter described at pc3d_scatter_rows_det_f32 instead of float atomics) */
/* Layers 1 + 2 of a set-abstraction MLP in one launch, without the [B,S,ns,C1] layer-1 output:
 *   Y[(b,s,j), :] = act(W act_in(P[b, idx[b,s,j], :] + Bc[b,s,:]) + bias)
 * = pc3d_group_act_f32 followed by pc3d_gemm_nt_f32, with the rows of the GEMM's X operand generated on load (P [B*NA, K]
 * with row stride ldp, Bc [B*S, K], idx [B,S,ns] int32, outside [0,NA): zero row of P). act_in = LeakyReLU(slope_in),
 * 0 = ReLU; act / slope as pc3d_gemm_nt_f32. Y [B*S*ns, N] with row stride ldy. mask (may be NULL; needs K % 4 == 0):
 * [B*S*ns, K/4] bytes, bit c % 4 of byte c / 4 = "element c of the generated row had a positive pre-activation" — the
 * only thing the backward of act_in needs from the tensor that is no longer stored:
 *   pc3d_group_act_bwd_mask_f32 = pc3d_group_act_bwd_f32 reading that mask instead of H. */
int pc3d_gemm_nt_gather_f32(const float* P, int64_t ldp, const float* Bc, const int32_t* idx, int B, int NA, int S, int ns,
                            float slope_in, const float* W, const float* bias, int N, int K, int act, float slope, float* Y,
                            int64_t ldy, uint8_t* mask, uint32_t* ymask, void* stream);
/* pc3d_group_max_linear_bwd_f32 with the channels split over `ksplit` (1 or 4) thread groups of a workgroup, the partial
 * sums added in chunk order: for launches with few groups (a group-all layer: ONE group per cloud, C3 = 1024 channels to
 * walk serially). A row's summation order depends on ksplit, so the caller chooses it from the per-cloud shape, never
 * from the batch. C3 % 32 == 0. */
int pc3d_group_max_linear_bwd_ks_f32(const float* gout, const float* out, const int64_t* arg, const float* W, int G, int ns,
                                     int C2, int C3, const float* xin, float* gx, int ksplit, void* stream);
/* ymask (may be NULL; needs N % 32 == 0): [B*S*ns, N/32] words, bit n % 32 of word n / 32 of a row = "Y[row, n] > 0 before
 * the activation" — the sign of layer 2's output for ITS backward, so that Y itself need not be kept after the next
 * layer has consumed it:  pc3d_group_max_linear_bwd_mask_f32 = pc3d_group_max_linear_bwd_f32 with that mask for xin. */
int pc3d_group_max_linear_bwd_mask_f32(const float* gout, const float* out, const int64_t* arg, const float* W, int G, int ns,
                                       int C2, int C3, const uint32_t* xmask, float* gx, void* stream);
int pc3d_group_act_bwd_mask_f32(const float* gH, const uint8_t* mask, const int32_t* idx, int B, int NA, int S, int K, int C,
                                float slope, float* gP, float* gBc, int deterministic, void* stream);

/* The WHOLE set-abstraction MLP after its per-point first layer + the max over the group in ONE launch
 * (model/pointnet2_utils.py:173-199): out[g,c] = relu(max_j (W3 relu(W2 relu(P[b, idx[g,j], :] + Bc[g,:]) + b2))[c] + b3[c]),
 * arg[g,c] = the winning member j (lowest on ties) — pc3d_gemm_nt_gather_f32 followed by the group-max form of the last
 * layer, without the [B*S*ns, C2] layer-2 output in memory (268 MB per level at SSG's sizes). Results are bit-identical
 * to that two-launch form (same operand order, same fp32 MFMA sequence). P [B*NA, C1] row stride ldp, Bc [B*S, C1],
 * idx [B,S,ns] int32 (outside [0,NA): zero row of P), W2 [C2,C1], W3 [C3,C2]; ns in {32, 64, 128}; C1 in {32, 64, 128},
 * C2 a multiple of 32 up to 128, C3 a multiple of 32. mask1 [B*S*ns, C1/4] bytes and mask2 [B*S*ns, C2/32] words receive the sign bits
 * of the generated layer-1 rows / of the layer-2 pre-activations (as pc3d_gemm_nt_gather_f32 writes them): all the
 * backward (pc3d_group_max_linear_bwd_mask_f32, pc3d_gemm_nt_f32 on W2^T, pc3d_group_act_bwd_*) needs. */
int pc3d_sa_chain_f32(const float* P, int64_t ldp, const float* Bc, const int32_t* idx, int B, int NA, int S, int ns,
                      const float* W2, const float* b2, int C1, int C2, const float* W3, const float* b3, int C3,
                      uint8_t* mask1, uint32_t* mask2, float* out, int64_t* arg, void* stream);
/* The same launch over a TABLE of row units: the 16- / 32-row units of the grouped rows that hold nothing but the ball
 * query's padding (copies of a group's first point, model/pointnet2_utils.py:84-104 — they can neither change nor win the
 * group max) are left out and the others packed four to a tile, whole groups per tile: fewer tiles instead of wasted
 * products (SSG: 13.5 of 32 and 22 of 64 rows per group are listed points). Same out / arg; mask1 / mask2 are written for
 * the kept units only (the backward never reads the others: their rows carry exact zeros).
 *   pc3d_sa_chain_table_unit: rows per unit the launch expects for a shape — 16 (the resident-weight kernel, 64-row tiles),
 *   8 (the streaming kernel, groups of <= 64 rows: an 8-row quarter of a 32 x 32 MFMA accumulator tile is a register group
 *   of its own, so the max is taken per 8 rows), 32 (the streaming kernel, groups of 128 rows), 0 (no table).
 *   pc3d_sa_blocks_i32: builds the table from idx [B,S,ns] — flags [B*S] bytes (scratch: bit u = unit u of the group is
 *   kept), tb int32 unit ids in original row space (-1 = empty slot): unit 8 -> [B*S*8] (64-row tiles of eight slots, at
 *   most eight units per group), unit 16 -> [B*S*4] (64-row tiles of four slots), unit 32 -> [ceil(B*S*ns/128)*4]
 *   (128-row tiles of four slots; at most four units per group for 16 / 32); ntiles [1] — two small launches (idx is known
 *   as soon as the ball query has run). Whole groups per tile; tiles past ntiles are undefined for units 8 / 16. B*S <= 64 K
 *   groups (48 K for unit 32): beyond that the entry point fails and the caller launches pc3d_sa_chain_f32 over every row.
 *   pc3d_sa_chain_tb_f32: tb / ntiles NULL = pc3d_sa_chain_f32; `unit` must be what pc3d_sa_chain_table_unit says. */
int pc3d_sa_chain_table_unit(int S, int ns, int C1, int C2, int C3);
int pc3d_sa_blocks_i32(const int32_t* idx, int B, int S, int ns, int unit, uint8_t* flags, int32_t* tb, int32_t* ntiles,
                       void* stream);
int pc3d_sa_chain_tb_f32(const float* P, int64_t ldp, const float* Bc, const int32_t* idx, int B, int NA, int S, int ns,
                         const float* W2, const float* b2, int C1, int C2, const float* W3, const float* b3, int C3,
                         uint8_t* mask1, uint32_t* mask2, float* out, int64_t* arg, const int32_t* tb, const int32_t* ntiles,
                         int unit, void* stream);

/* The backward of a set-abstraction chain (pc3d_sa_chain_f32) from the max down to the points, on the ACTIVE rows only.
 * A row of a group that wins no channel of the max carries no gradient — 58-65 % of the rows at the single-scale
 * classifier's levels (the ball query pads a group with copies of its first point, and a copy never wins): the three
 * launches below neither write, read nor multiply those rows (model/pointnet2_utils.py:190-198 differentiated).
 *   pc3d_group_max_linear_bwd_sparse_f32 = pc3d_group_max_linear_bwd_mask_f32 that also writes amask [G, ceil(ns/32)] words
 *       (bit j of group g = "row j won at least one channel") and stores ONLY those rows of gx [G*ns, C2]; the other
 *       rows of gx stay undefined.
 *   pc3d_gemm_nt_groupsum_f32: Y = X . Wt^T (pc3d_gemm_nt_f32 without bias / activation) AND the groups pass of
 *       pc3d_group_act_bwd_rev_f32 on Y in one launch — X = gx above [B*S*ns, K] (row stride ldx), Wt [C1, K] = W2
 *       transposed, Y [B*S*ns, C1] = the gradient of the generated layer-1 rows (NOT masked by mask1; written: the active
 *       rows, and zeros for inactive rows that are not padding copies j > 0 with idx[g,j] == idx[g,0] — those copies are
 *       not in the reverse lists of pc3d_group_reverse_i32, the points pass reaches them through `tail` only), gBc [B*S, C1] = per group the sum of mask1 * Y over its rows, tail [B*S, C1] the same sum over the rows
 *       j > 0 that repeat the group's first index (idx [B,S,ns]); mask1 [B*S*ns, C1/4] bytes from the forward. amask NULL =
 *       every row is active. A tile's active rows are compacted before the product (half the MFMA blocks at those
 *       levels). Bit-identical to the separate launches on full tensors: the skipped terms are exact zeros, the others
 *       are summed in the same order. ns in {32, 64, 128}; C1 in {32, 64, 128}; K a multiple of 32.
 *   pc3d_group_act_bwd_points_f32: the points pass of pc3d_group_act_bwd_rev_f32 alone (gP [B,NA,C] from gH, its sign
 *       bytes, the groups pass's tail and the reverse index off / lst); amask (may be NULL) [B*S, ceil(K/32)]: rows of gH
 *       whose bit is clear are skipped. */
int pc3d_group_max_linear_bwd_sparse_f32(const float* gout, const float* out, const int64_t* arg, const float* W, int G, int ns,
                                         int C2, int C3, const uint32_t* xmask, float* gx, uint32_t* amask, void* stream);
int pc3d_gemm_nt_groupsum_f32(const float* X, int64_t ldx, const float* Wt, const uint8_t* mask1, const int32_t* idx,
                              const uint32_t* amask, int B, int S, int ns, int C1, int K, float* Y, float* gBc, float* tail,
                              void* stream);
/* pc3d_gemm_nt_groupsum_f32 with amask over PACKED tiles: a tile is a run of whole groups whose active rows fill 128 rows
 * (a first one-workgroup launch assigns groups to tiles from amask's bit counts), instead of 128 consecutive rows of
 * which a third are active. Same results bit for bit. scratch: B*S + 4 + ceil(B*S / 4) int32 (overwritten). ns in {32, 64};
 * amask must not be NULL. */
int pc3d_gemm_nt_groupsum_packed_f32(const float* X, int64_t ldx, const float* Wt, const uint8_t* mask1, const int32_t* idx,
                                     const uint32_t* amask, int B, int S, int ns, int C1, int K, float* Y, float* gBc,
                                     float* tail, int32_t* scratch, void* stream);
int pc3d_group_act_bwd_points_f32(const float* gH, const uint8_t* mask, const float* tail, const int32_t* off,
                                  const int32_t* lst, const uint32_t* amask, int B, int NA, int S, int K, int C, float slope,
                                  float* gP, void* stream);

/* The coordinate part of a set-abstraction layer's first 1x1 convolution (model/pointnet2_utils.py:118-135,190-197: the
 * Conv2d over [xyz_j - centre_s ; feat_j] is linear, so it splits into a per-POINT part P = Wx x + Wf f and a per-CENTRE
 * part Bc = b1 - Wx c; the Wf part is a GEMM with the coordinate part as its residual operand). Three-column products:
 *   pc3d_affine3_f32      out[b,n,c] = bias[c] + sign * (W[c,0] x + W[c,1] y + W[c,2] z);  x a [B,N,3] view with element
 *                         strides (x_bs, x_ps, x_cs) — a channels-first [B,3,N] tensor is read in place; W [C,3], bias [C]
 *                         or NULL, C % 4 == 0, out [B*N, C] with row stride ldo.
 *   pc3d_affine3_bwd_f32  out[b,n,:] = add[b,n,:] + sign * sum_c g[b,n,c] W[c,:];  g [B*N, C] row stride ldg, add (may be
 *                         NULL) and out [B,N,3] views with their own strides (the gradient of a channels-first tensor is
 *                         written in that layout). Fixed summation order.
 *   pc3d_scatter_points_det_f32  out[b, idx[b,s], :] += val[b,s,:] in ascending s: the gradient of the centres
 *                         new_xyz = xyz[fps_idx] (:113, index_points) folded into the gradient of xyz; idx [B,S] int32,
 *                         val [B,S,3] contiguous, out as above. One wavefront owns a cloud's column: no float atomics on
 *                         memory, repeated centres are summed in order. */
int pc3d_affine3_f32(const float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs, int B, int N, const float* W,
                     const float* bias, float sign, int C, float* out, int64_t ldo, void* stream);
int pc3d_affine3_bwd_f32(const float* g, int64_t ldg, int B, int N, int C, const float* W, float sign,
                         const float* add, int64_t a_bs, int64_t a_ps, int64_t a_cs,
                         float* out, int64_t o_bs, int64_t o_ps, int64_t o_cs, void* stream);
int pc3d_scatter_points_det_f32(const int32_t* idx, const float* val, int B, int S, int N, float* out, int64_t o_bs,
                                int64_t o_ps, int64_t o_cs, void* stream);
/* out[g,c] = max_r Y[g,r,c], arg[g,c] = the first row holding it (a NaN wins, as torch.max): the group max of a
 * set-abstraction layer whose last layer is too wide for the fused form (model/pointnet2_utils.py:198). Y [G,ns,C]. */
int pc3d_rows_max_f32(const float* Y, int64_t G, int ns, int C, float* out, int64_t* arg, void* stream);

/* The same backward WITHOUT float atomics, as a gather over a reverse index of the grouping.
 * pc3d_group_reverse_i32: per cloud, the list of grouped rows that reference each point (a counting sort on the device:
 *   two passes of integer atomics + a scan). idx [B,S,K] int32 as above; cnt [B,NA] int32 scratch; off [B,NA+1] int32
 *   (list of point p = lst[b][off[b,p] .. off[b,p+1])); lst [B, L] int32 with L = pc3d_group_reverse_list_len(S, K) =
 *   S*K + S. Entry codes: s*K + j = row (s,j) of the cloud; S*K + s = "the sum of the rows of group s that repeat its
 *   first index" (the ball query's padding), listed under that first index. Entries outside [0,NA) are in no list.
 *   Every list is sorted ascending after the fill (the atomics hand out slots in arrival order), so the gather below
 *   sums in ONE order: deterministic gradients. It depends on idx only: build it once per forward, beside the MLPs.
 * pc3d_group_act_bwd_rev_f32: gBc and the per-group padded-tail sums in one pass over the groups (tail [B,S,C] scratch),
 *   then gP[b,p,:] = sum over the list of p — every row of gP written once, no zero fill. The sign of the activation
 *   comes from H [B,S,K,C] or, when H is NULL, from the bit mask of pc3d_gemm_nt_gather_f32. C % 4 == 0, C <= 512. */
int64_t pc3d_group_reverse_list_len(int S, int K);
int pc3d_group_reverse_i32(const int32_t* idx, int B, int NA, int S, int K, int32_t* cnt, int32_t* off, int32_t* lst,
                           void* stream);
int pc3d_group_act_bwd_rev_f32(const float* gH, const float* H, const uint8_t* mask, const int32_t* idx, const int32_t* off,
                               const int32_t* lst, int B, int NA, int S, int K, int C, float slope, float* gP, float* gBc,
                               float* tail, void* stream);

/* Backward of  [max_n | mean_n] LeakyReLU(Y[b,n,:], slope)  followed straight by the backward of the layer that produced Y
 * (model/dgcnn.py:317-320 after conv5, model/curvenet.py:64-67 after conv0), in ONE GEMM: dX = dY W with the rows of dY
 * generated on load from the pre-activation Y [B*Npts, K] (row stride ldy_in), the upstream gradient g [B, 2K] (max part,
 * then mean part) and the arg-max rows arg [B, K] of pc3d_act_pool_f32 — pc3d_act_pool_bwd_f32 + pc3d_gemm_nt_f32 without
 * the [B*Npts, K] gradient tensor. W [N, K] row-major (the producing layer's weight TRANSPOSED, as for any backward on
 * pc3d_gemm_nt_f32); dX [B*Npts, N] with row stride ldx_out. K % 4 == 0. */
int pc3d_gemm_nt_poolbwd_f32(const float* Y, int64_t ldy_in, const float* g, const int32_t* arg, int B, int Npts,
                             float slope_pool, const float* W, int N, int K, float* dX, int64_t ldx_out, void* stream);

/* Row reductions of a [B,N] f32 matrix into out[B].
 *   op:  0 = mean, 1 = max, 2 = sum        pre: 0 = identity, 1 = sqrt(max(x,0)) applied per element first
 * mean/max of squared distances = ChamferDistance/HausdorffDistance (distance.py:44-49,64-69);
 * pre=1 gives the Euclidean variants of dis_utils_{numpy,torch}.py. Deterministic (fixed tree order). */
int pc3d_rowreduce_f32(const float* x, int B, int N, int op, int pre, float* out, void* stream);

/* Backward through the gathered NN pairs of pc3d_nn_bidir_f32 (autograd of distance.py:40-50,58-70 and of
 * every loss built on per-point NN distances).  With upstream per-point weights wA on dA and wB on dB
 * (element strides (w_bs, w_ps) — a stride of 0 broadcasts, so "mean over points" needs no expanded tensor —
 * and scalar multipliers sA, sB):
 *   grad_a[i] = 2 sA wA[i] (a_i - b_iA[i]) + sum_{j: iB[j]==i} 2 sB wB[j] (a_i - b_j)
 *   grad_b[j] = 2 sB wB[j] (b_j - a_iB[j]) + sum_{i: iA[i]==j} 2 sA wA[i] (b_j - a_i)
 * wA/wB may be NULL (that direction contributes nothing). grad_a/grad_b are OVERWRITTEN; either may be NULL.
 * deterministic != 0: ordered accumulation (bitwise reproducible) instead of float atomics. */
int pc3d_nn_bwd_f32(const float* a, int64_t a_bs, int64_t a_ps, int64_t a_cs,
                    const float* b, int64_t b_bs, int64_t b_ps, int64_t b_cs,
                    int B, int N, int M,
                    const int32_t* iA, const float* wA, int64_t wA_bs, int64_t wA_ps, float sA,
                    const int32_t* iB, const float* wB, int64_t wB_bs, int64_t wB_ps, float sB,
                    float* grad_a, int64_t ga_bs, int64_t ga_ps, int64_t ga_cs,
                    float* grad_b, int64_t gb_bs, int64_t gb_ps, int64_t gb_cs,
                    int deterministic, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * K8  PointNet per-point MLP 3 -> 64 -> 128 -> C3 (1x1 conv, eval-mode BatchNorm folded into W/b by the caller,
 * ReLU after layers 1-2 and optionally after the pool) fused with max-pool over the N points.
 * Replaces model/pointnet.py:34-37 (STN3d tower, relu_last=1) and :110-123 (PointNetfeat trunk, relu_last=0),
 * i.e. three Conv1d+BN(+ReLU) and torch.max(x, 2) with their [B,C,N] activations.
 * One entry per launch; which kernel form runs is the argument `form`. Every form of a launch writes the same bits
 * into every output. The rules below are checked before any HIP call; breaking one is PC3D_EINVAL.
 *
 * pc3d_pointmlp3_max_fwd_f32
 *   x      B x N points (element strides)
 *   T      optional [B,3,3] row-major input transform, x'[n,:] = x[n,:] @ T[b] (the torch.bmm of
 *          model/pointnet.py:106-109), NULL = identity
 *   th_in, th_W, th_b, th_K, T_out   the transform head. th_in != NULL: T[b] = th_W [9,th_K] . th_in[b] + th_b — the
 *          last layer of STN3d (model/pointnet.py:45-47: fc3, with the flattened identity added into th_b) — is computed
 *          in the launch's prologue instead of a launch of its own between the two towers, and T_out [B,9] receives it
 *          (the backward launch reads it as its T). T must then be NULL, and th_W, th_b, T_out and th_K >= 1 are
 *          required. th_in == NULL: the other four are not read.
 *   W1 [64,3] b1[64]  W2 [128,64] b2[128]  W3 [C3,128] b3[C3]   row-major, BN already folded; C3 % 32 == 0, <= 1024
 *   part_val/part_idx  caller workspace [B, ceil(N / pc3d_pointmlp3_tile_points()), C3] f32 / i32
 *   pooled [B,C3] f32 (after the optional ReLU), argidx [B,C3] i32 = lowest point index attaining the max;
 *          pass both NULL to keep only the per-tile partials (no fold launch)
 *   mask1 [B,N] u64, mask2 [B,N,4] u32 (both or neither)  the ReLU decisions of layers 1 and 2 per point (bit c of
 *          mask1 = channel c of layer 1 is positive; word j bit r of mask2 = channel 32j+r of layer 2 is positive),
 *          which the backward launch consumes instead of recomputing the two layers
 *   form   fp32 throughout: layers 2 and 3 are exact fp32 FMA chains (v_mfma_f32_32x32x2_f32) in
 *          PC3D_PM_FWD_EXACT. The other forms SCREEN layer 3: a cheap product S of h2 and W3 on the matrix pipe with a
 *          rigorous bound E, and only the points whose S + E reaches the tile's best S - E are recomputed as the exact
 *          fp32 fmaf chain; tiles / channel blocks with non-finite or huge operands, or with more candidates than their
 *          list holds, run the exact fp32 MFMA block.
 *            PC3D_PM_FWD_SCREEN         both operands split in two bf16 terms inside the launch (three products on
 *                                       v_mfma_f32_32x32x16_bf16; bound: csrc/pointmlp_screen_bound.h)
 *            PC3D_PM_FWD_SCREEN_PREP    the same screen with its operands and the recheck's rows read from the
 *                                       prepared image w3_bf / w3_nw / w3_q; the recheck goes by channel
 *            PC3D_PM_FWD_SCREEN_H       ONE scaled fp16 product per k-step from the fp16 image w3_h / w3_cw (sixteen
 *                                       candidate slots per channel instead of eight; csrc/pointmlp_screen_h_bound.h)
 *            PC3D_PM_FWD_SCREEN_H_PAIR  SCREEN_H with the recheck laid out by (channel, candidate) PAIR, one lane each
 *          A screened instantiation's first use on a device must fall outside a stream capture; while it has not, the
 *          launch runs the next of H_PAIR -> H -> PREP -> SCREEN -> the exact kernel.
 *          pc3d_pointmlp3_pair_recheck_ready: 1 once the production H_PAIR instantiation can be launched on the current
 *          device, 0 before.
 *   w3_bf, w3_nw, w3_q / w3_h, w3_cw   the prepared images of the SAME W3 (the caller answers for that), see
 *          pc3d_pointmlp3_w3_prepare_f32 / _h_f32. SCREEN_PREP needs the first three, the H forms all five (the bf16
 *          image serves while an H instantiation cannot be launched yet); EXACT and SCREEN read none.
 *   stats  != NULL selects the debug instantiation of a screened form (tests and tools/bench_pointmlp_screen.py; an
 *          error with EXACT). [B, ntiles, 2] i32, ADDED to (zero it first): candidates rechecked, channel blocks that
 *          ran the exact block.
 *   dbg_S, dbg_E   [B, N, C3] f32, both or neither, only with stats (tiny shapes): the screen's value and bound of every
 *          (point, channel) of a screened block; the H forms write them in the unscaled domain.
 *   stop_after   0..3, nonzero only with stats: 1 / 2 / 3 return after the prologue and norms / the screen / the
 *          selection (timing only: the outputs are then undefined); 0: all.
 * ------------------------------------------------------------------------------------------------------- */
enum { PC3D_PM_FWD_EXACT = 0, PC3D_PM_FWD_SCREEN = 1, PC3D_PM_FWD_SCREEN_PREP = 2, PC3D_PM_FWD_SCREEN_H = 3,
       PC3D_PM_FWD_SCREEN_H_PAIR = 4 };
int pc3d_pointmlp3_tile_points(void);
int pc3d_pointmlp3_bwd_tile_points(void);
int pc3d_pointmlp3_pair_recheck_ready(void);
int pc3d_pointmlp3_max_fwd_f32(const float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs, int B, int N,
                               const float* T, const float* th_in, const float* th_W, const float* th_b, int th_K,
                               float* T_out, const float* W1, const float* b1, const float* W2, const float* b2,
                               const float* W3, const float* b3, int C1, int C2, int C3, int relu_last,
                               float* part_val, int32_t* part_idx, float* pooled, int32_t* argidx, uint64_t* mask1,
                               uint32_t* mask2, int form, const void* w3_bf, const float* w3_nw, const float* w3_q,
                               const void* w3_h, const float* w3_cw, int32_t* stats, float* dbg_S, float* dbg_E,
                               int stop_after, void* stream);
/* The fold launch of the entry above on its own: pooled[b,c] = max_t part_val[b,t,c] (the first tile wins ties),
 * argidx the winner's part_idx, optional ReLU; part_* are [B,ntiles,C3]. serial = 1 runs the earlier kernel, which
 * loads one tile's value, compares, and then fetches the winner's index: the same bits. Parity tests and
 * tools/bench_small_launches.py only; nothing on a hot path calls it. */
int pc3d_pointmlp3_fold_f32(const float* part_val, const int32_t* part_idx, int B, int ntiles, int C3, int relu_last,
                            float* pooled, int32_t* argidx, int serial, void* stream);
/* The prepared image of the folded W3 [C3,128] (a frozen victim weight: made once per fold, csrc/pointmlp_screen.hip):
 * w3_bf [C3/32][8][2][64][8] bf16 (block, k-step, hi / lo, lane r + 32 h, the 8 terms of W3[32 cb + r][16 t + 8 h + 0..7]),
 * w3_nw [C3] f32 (the screen's upper bound of the row norm), w3_q [32][C3][4] f32 (w3_q[t][c] = W3[c][4t..4t+3]). */
int pc3d_pointmlp3_w3_prepare_f32(const float* W3, int C3, void* w3_bf, float* w3_nw, float* w3_q, void* stream);
/* The fp16 image of the same W3, made from it and from the w3_nw that pc3d_pointmlp3_w3_prepare_f32 wrote:
 * w3_h [C3/32][8][64][8] fp16 (block, k-step, lane r + 32 h, the 8 values of W3[32 cb + r][16 t + 8 h + 0..7] * 2^sw[c],
 * rounded to nearest even; sw[c] puts w3_nw[c] * 2^sw[c] into [2^13, 2^14)), w3_cw [C3] f32 (the channel's factor of the
 * screen's bound in that scaled domain, csrc/pointmlp_screen_h_bound.h; +inf for a channel whose norm is out of range). */
int pc3d_pointmlp3_w3_prepare_h_f32(const float* W3, int C3, const float* w3_nw, void* w3_h, float* w3_cw, void* stream);

/* Backward-to-input of the above (weights are frozen during an attack: no weight gradients, SURVEY A-14).
 * g_pooled [B,C3] is the upstream gradient on `pooled`; with relu_last the caller zeroes it where pooled <= 0.
 * T == NULL: grad_x receives the gradient w.r.t. the tower input. T given: the kernel chains through x' = x @ T:
 * grad_x receives the gradient w.r.t. the RAW points x, and part_gT (if non-NULL, workspace
 * [B, ceil(N / pc3d_pointmlp3_bwd_tile_points()), 16], 9 used) the per-tile partial sums of dL/dT (row-major 3x3), one
 * record per 32 points in every form; their sum over tiles is the gradient that flows on into the STN head.
 * accumulate != 0: grad_x += (used to add the STN tower's contribution on top of the trunk's).
 * W2T is W2 transposed ([64,128] row-major); required, but only the two-list form reads it: the balanced kernel fetches
 * its MFMA operand from W2 itself (coalesced in that operand's lane order).
 * mask1 / mask2 are the forward launch's outputs of those names (required).
 * The max-pool routes each channel to one point, so the layer-3 dgrad is a sparse ordered gather: the tile's hits are
 * sorted by point and each point's row is one fma chain in ascending channel order, whole points shared out over the
 * workgroup's waves: deterministic, and independent of which wave runs a point.
 * form: the same computation, bit for bit (tests/test_pointmlp_bwd_packed_gpu.py); everything but PC3D_PM_BWD_DEFAULT
 * is for the parity tests and tools/bench_pointmlp.py.
 *   PC3D_PM_BWD_DEFAULT   the one of the next two that the library prefers (the packed form)
 *   PC3D_PM_BWD_PACKED    the balanced kernel, a workgroup per 128 points: argidx / g / W2 fetched once for them and the
 *                         W2 product over the rows of points that have a hit only
 *   PC3D_PM_BWD_TILE32    the balanced kernel, a workgroup per 32 points, every row of a tile through the W2 product
 *   PC3D_PM_BWD_TWOLIST   the earlier two-list kernel (hits split at points 0-15 / 16-31, rows accumulated through LDS)
 * stop_after: 0, or with PC3D_PM_BWD_PACKED only 1..5: end the launch after classification and count / sorted list /
 * gather / W2 product / W1 product (timing only: outputs are not written). */
enum { PC3D_PM_BWD_DEFAULT = 0, PC3D_PM_BWD_PACKED = 1, PC3D_PM_BWD_TILE32 = 2, PC3D_PM_BWD_TWOLIST = 3 };
int pc3d_pointmlp3_max_bwd_f32(const float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs, int B, int N,
                               const float* T, const float* W1, const float* b1, const float* W2,
                               const float* b2, const float* W3, const float* W2T, int C1, int C2, int C3,
                               const int32_t* argidx, const uint64_t* mask1, const uint32_t* mask2,
                               const float* g_pooled,
                               float* grad_x, int64_t gx_bs, int64_t gx_ps, int64_t gx_cs,
                               float* part_gT, int accumulate, int form, int stop_after, void* stream);

/* The two launches above with per-cloud lengths: lengths [B] i32 in device memory, read as data by the kernels (a
 * captured launch serves any lengths written into that buffer later). Cloud b has L = clamp(lengths[b], 1, N) points;
 * N stays the buffers' row count: it is used for every stride, for the tile count and for the workspaces' shapes, and
 * every other argument is the dense entry's.
 * The contract: a launch given lengths reads no row n >= L of x, and on the rows below L (and in pooled, argidx, T_out,
 * part_gT's sum) it writes the bits the dense launch writes for that cloud, whether the dense launch is given the L rows
 * alone or the N rows padded with copies of point 0.
 * Forward: rows in [L, N) of mask1 / mask2 are written as zero words. A 128-point tile that lies wholly at or beyond L
 * is skipped: its workgroup leaves ahead of its first barrier and writes only part_val = -inf, part_idx = 0 for its C3
 * entries (the folds' strict `>` never takes them; tile 0 is never skipped and keeps the T_out store) and those zero mask
 * words. form is PC3D_PM_FWD_EXACT or PC3D_PM_FWD_SCREEN_H_PAIR (the production form; all five image pointers are then
 * needed), the other forms have no ragged twin; stats, dbg_S and dbg_E must be NULL and stop_after 0. While the ragged
 * H_PAIR instantiation's first use on a device falls into a stream capture, the launch runs the ragged exact kernel.
 * Backward: form is PC3D_PM_BWD_DEFAULT or PC3D_PM_BWD_PACKED (the packed kernel's ragged twin), stop_after 0. x,
 * mask1 and mask2 are read below L only and a route (argidx) at or beyond L is dropped; grad_x rows in [L, N) are written
 * 0 (accumulate != 0: left untouched) and part_gT's records of the 32-point sub-tiles at and beyond L are zero. A
 * workgroup whose 128 points lie at or beyond L writes those zeros and scans nothing.
 * lengths == NULL, another form, a debug argument: PC3D_EINVAL before any HIP call. B == 0 is a no-op. */
int pc3d_pointmlp3_max_fwd_ragged_f32(const float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs, int B, int N,
                                      const float* T, const float* th_in, const float* th_W, const float* th_b, int th_K,
                                      float* T_out, const float* W1, const float* b1, const float* W2, const float* b2,
                                      const float* W3, const float* b3, int C1, int C2, int C3, int relu_last,
                                      float* part_val, int32_t* part_idx, float* pooled, int32_t* argidx, uint64_t* mask1,
                                      uint32_t* mask2, int form, const void* w3_bf, const float* w3_nw, const float* w3_q,
                                      const void* w3_h, const float* w3_cw, int32_t* stats, float* dbg_S, float* dbg_E,
                                      int stop_after, const int32_t* lengths, void* stream);
int pc3d_pointmlp3_max_bwd_ragged_f32(const float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs, int B, int N,
                                      const float* T, const float* W1, const float* b1, const float* W2,
                                      const float* b2, const float* W3, const float* W2T, int C1, int C2, int C3,
                                      const int32_t* argidx, const uint64_t* mask1, const uint32_t* mask2,
                                      const float* g_pooled,
                                      float* grad_x, int64_t gx_bs, int64_t gx_ps, int64_t gx_cs,
                                      float* part_gT, int accumulate, int form, int stop_after, const int32_t* lengths,
                                      void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * PointNet with the feature transform (model/pointnet.py:51-87 STNkd, :101-117), eval mode, BatchNorm folded:
 *   x' = x @ T,  h = relu(W1 x' + b1),  Tf = I + head(max_n tower_{64->64->128->1024}(h)),
 *   pooled = max_n (W3 relu(W2 Tf^T h + b2) + b3).
 * The towers are the pc3d_pointmlp3_* design (one launch, no per-point activation leaves the CU, ReLU decisions as
 * per-point bit masks, (max, argmax) per tile of pc3d_pointmlp3_tile_points() points in part_val / part_idx
 * [B, ntiles, C3], folded by pc3d_pointmlp3_fold_f32) with two extensions; T [B,3,3] is required.
 *
 * pc3d_pointnet_ft_tower_fwd_f32:
 *   WA, bA, maskA given: STNkd's tower 3 -> 64 -> [64 -> 64] -> 128 -> C3. h is recomputed from x (W1, b1 are the
 *     TRUNK's layer 1); WA [64,64] / bA is the extra layer, whose decisions go to maskA [B,N] (bit c = channel c).
 *   WA, bA, maskA NULL: the trunk 3 -> 64 -> 128 -> C3.
 *   W2 [128,64] is read at W2 + b * w2_bs floats for cloud b (w2_bs = 0: one weight for all clouds). The trunk takes
 *   the folded W2_b = W2 Tf_b^T of pc3d_pointnet_ft_fold_w2_f32 (w2_bs = 8192), which replaces the per-point
 *   64 x 64 product Tf^T h. mask1 [B,N] / mask2 [B,N,4] as pc3d_pointmlp3_max_fwd_f32. */
int pc3d_pointnet_ft_tower_fwd_f32(const float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs, int B, int N,
                                   const float* T, const float* W1, const float* b1, const float* WA, const float* bA,
                                   const float* W2, int64_t w2_bs, const float* b2, const float* W3, const float* b3,
                                   int C3, float* part_val, int32_t* part_idx, uint64_t* mask1, uint64_t* maskA,
                                   uint32_t* mask2, void* stream);
/* W2b[b][c][i] = sum_j W2[c][j] Tf[b][i][j] (W2 [128,64], Tf [B,64,64], W2b [B,128,64]); ascending j. */
int pc3d_pointnet_ft_fold_w2_f32(const float* W2, const float* Tf, int B, float* W2b, void* stream);
/* Backward-to-input of pc3d_pointnet_ft_tower_fwd_f32 (winners only: the ordered gather of
 * pc3d_pointmlp3_max_bwd_f32's PC3D_PM_BWD_TWOLIST form, then the masked layers on MFMA). grad_x receives (accumulate != 0: is added) the
 * gradient w.r.t. the RAW points; rows [gT_off, gT_off + ceil(N / pc3d_pointmlp3_bwd_tile_points())) of part_gT
 * [B, gT_tiles, 16] the per-tile partials of dL/dT, so that both towers' partials sit in ONE workspace the STN head's
 * backward sums. WA / maskA given: the 64 -> 64 form (W2q, q NULL). W2q / q given: the trunk; W2 is the folded
 * per-cloud weight, W2q the UNfolded W2, and q [B,N,64] receives q[b,n,:] = g_z2[b,n,:] . W2 (zero rows for points
 * that won no channel) for pc3d_pointnet_ft_dtf_f32. Neither: a plain 3 -> 64 -> 128 -> C3 tower. T == NULL (part_gT
 * is then not written): a tower on the raw points, i.e. what pc3d_pointmlp3_max_bwd_f32 computes for STN3d's tower.
 * Unlike that entry, the gather sums a run of channels that hit the same point in a register and cuts runs at 32
 * entries, so a point that wins hundreds of channels is summed in blocks, not as one chain: all three towers of a
 * feature-transform victim go through this entry. */
int pc3d_pointnet_ft_tower_bwd_f32(const float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs, int B, int N,
                                   const float* T, const float* W1, const float* WA, const float* W2, int64_t w2_bs,
                                   const float* W2q, const float* W3, int C3, const int32_t* argidx,
                                   const uint64_t* mask1, const uint64_t* maskA, const uint32_t* mask2,
                                   const float* g_pooled, float* grad_x, int64_t gx_bs, int64_t gx_ps, int64_t gx_cs,
                                   float* part_gT, int gT_tiles, int gT_off, float* q, int accumulate, void* stream);
/* g_Tf[b][i][j] = sum_n h[b][i][n] q[b][n][j] with h = relu(W1 (x @ T) + b1) recomputed by the forward's FMA chain;
 * one thread owns an (i, j) and walks n in ascending order: no atomics, the same bits every run. */
int pc3d_pointnet_ft_dtf_f32(const float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs, int B, int N, const float* T,
                             const float* W1, const float* b1, const float* q, float* g_Tf, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Classifier heads. Y[b,o] = epi(sum_k X[b,k] W[o,k] + bias[o]) for small row counts (the B samples of a batch),
 * fp32 MFMA. X may be given as P partial slabs per row ([B,P,K], summed on load; P=1 = plain matrix; ldx = row
 * stride in floats). epi: optional (Leaky)ReLU (relu = 1: Y = Y > 0 ? Y : slope * Y; slope 0 = ReLU), then optional
 * gate (Y = gate[b,o] > 0 ? Y : gate_slope * Y — the activation mask of a saved forward output, which makes the same
 * kernel the backward of Linear + (Leaky)ReLU when W is passed transposed: dX_prev = gate_prev(dY . W)).
 * Replaces F.linear / BatchNorm1d(eval, folded) / ReLU of model/pointnet.py:38-47,144-147 (LeakyReLU(0.2): the DGCNN
 * head, model/dgcnn.py:322-326) and their autograd.
 *
 * Shapes with K % 16 == 0, K <= 1024, P == 1 and O >= 64 run a kernel whose eight waves split K in chunks of 16
 * (chunk c belongs to wave c % 8) and whose tile — rows x outputs per workgroup — is one of four forms:
 *   PC3D_LIN_TILE_32X16   two row tiles of 16 per workgroup, grid (O/16, ceil(B/32))
 *   PC3D_LIN_TILE_16X16   one row tile,                      grid (O/16, ceil(B/16))
 *   PC3D_LIN_TILE_16X8    eight outputs,                     grid (O/8,  ceil(B/16))
 *   PC3D_LIN_TILE_8X8     eight rows, eight outputs,         grid (O/8,  ceil(B/8))
 * A workgroup pulls 4 K (rows + outputs) bytes, and above the launch floor a launch lasts as long as one workgroup's
 * pull: the smaller tiles spread the same layer over more CUs. Every form computes the SAME BITS (an output depends on
 * its own row of X and of W only; the k order, the chunk -> wave assignment and the order in which the waves' partial
 * sums are added do not depend on the tile; tests/test_linear_tiles_gpu.py). tile = PC3D_LIN_TILE_RULE (0) takes
 * pc3d_linear_tile(B, K, O); a form by name is for the parity tests and the bench tool. Other shapes run 32 x 32 tiles
 * and ignore `tile`.
 *
 * pc3d_linear_tile: the rule, a pure function of the layer's shape (no timing, environment or process state). Its
 * table, fixed from profiles/linear_tiles_bench.json and the headline pairs, with
 * wgs(form) = ceil(O / outputs) * ceil(B / rows):
 *   K < 256 (not measured)                      ->  PC3D_LIN_TILE_32X16
 *   otherwise the first of 8X8, 16X8, 16X16 with wgs(form) <= 256 (one workgroup per CU), else 32X16
 * At B = 32: 1024 -> 512, 512 -> 256 and 256 -> 512 take 8X8 (256, 128, 256 workgroups), 512 -> 1024 takes 16X8 (256).
 * pc3d_linear_book_f32 alone does not take the rule for tile 0 (see there).
 * ------------------------------------------------------------------------------------------------------- */
enum { PC3D_LIN_TILE_RULE = 0, PC3D_LIN_TILE_32X16 = 1, PC3D_LIN_TILE_16X16 = 2, PC3D_LIN_TILE_16X8 = 3,
       PC3D_LIN_TILE_8X8 = 4 };
int pc3d_linear_tile(int B, int K, int O);
int pc3d_linear_f32(const float* X, int ldx, int P, int B, int K, const float* W, const float* bias, int O,
                    int relu, float slope, const float* gate, int ldg, float gate_slope, float* Y, int ldy, int tile,
                    void* stream);
/* The same layer with its X operand produced on the fly by a tiny pre-layer (the backward of STN3d's fc3, 9 -> 256,
 * folded into the launch of fc2's backward, model/pointnet.py:44-45 and their autograd):
 *   X[b,k] = gate_pre[b,k] > 0 ? sum_{j<J} (sum_p parts[b,p,j]) Wp[j,k] : 0 ;   Y[b,o] = gate(sum_k X[b,k] W[o,k])
 * parts [B,P,Jp] (J <= Jp columns used, J <= 16), Wp [J,K] row-major, gate_pre [B,K] (row stride ldgp), K % 16 == 0.
 * tile: as pc3d_linear_f32's (the summed slab S and the on-the-fly X follow the row tile; the same bits in every form). */
int pc3d_linear_pre_f32(const float* parts, int P, int Jp, int J, const float* Wp, const float* gate_pre, int ldgp, int B,
                        int K, const float* W, int O, const float* gate, int ldg, float* Y, int ldy, int tile,
                        void* stream);

/* log_softmax (model/pointnet.py:148) + argmax + adversarial loss on the log-probabilities and its gradient w.r.t.
 * the LOGITS, one launch. kind 0 = UntargetedLogitsAdvLoss, 1 = LogitsAdvLoss, 2 = CrossEntropyAdvLoss, 3 = minus kind 2
 * (GeoA3's untargeted classification loss, attack/GeoA3/GeoA3_attack.py:125-127)
 * (attack/CW/CW_utils/adv_utils.py:64-80, 17-33, 42-51); per-sample loss[b] (before the batch mean), pred[b],
 * logp [B,ncls], g_logits [B,ncls] = scale * dloss_b/dlogits (scale = 1/B reproduces .mean()). Outputs may be NULL.
 * kind + 4: the loss is taken on `logits` AS GIVEN (no log-softmax) — what the reference's functors compute on whatever the
 * victim returns, log-probabilities (PointNet, PointNet++, DGCNN) or raw logits (CurveNet); kind 6 is then nll_loss. */
int pc3d_cls_loss_f32(const float* logits, int ld, int B, int ncls, const int64_t* target, int kind, float kappa,
                      float scale, float* logp, int64_t* pred, float* loss, float* g_logits, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * K9  clip / projection of the perturbation pc - ori, one launch (attack/CW/CW_utils/clip_utils.py).
 *   mode 0: per-point L2 norm <= budget  — ClipPointsLinf (:43-56; the reference's "Linf" is a per-point L2 clip,
 *           SURVEY A-10); with `normal` != NULL the inner-point tangent projection ProjectInnerPoints (:67-108)
 *           runs first = ProjectInnerClipLinf (:124-136). budget <= 0 skips the clip (projection only).
 *   mode 1: global L2 norm of the whole perturbation <= budget — ClipPointsL2 (:16-29). `normal` ignored.
 * All tensors B x K points with element strides; out may alias pc.
 * ------------------------------------------------------------------------------------------------------- */
int pc3d_clip_f32(const float* pc, int64_t pc_bs, int64_t pc_ps, int64_t pc_cs,
                  const float* ori, int64_t o_bs, int64_t o_ps, int64_t o_cs,
                  const float* normal, int64_t n_bs, int64_t n_ps, int64_t n_cs,
                  int B, int K, int mode, float budget,
                  float* out, int64_t out_bs, int64_t out_ps, int64_t out_cs, void* stream);

/* K10 (+K9)  one torch.optim.Adam step (weight_decay 0, amsgrad off) on the adversarial points, optionally fused
 * with the mode-0 clip/projection against `ori` (ori NULL = plain Adam). Replaces opt.step() + clip_func of
 * attack/CW/CW_attack.py:169-174 and attack/KNN/KNN_attack.py:129-136.
 * m, v (exp_avg, exp_avg_sq) share p's strides and are updated in place. The step number t (>= 1) comes from the
 * device word *step_dev when non-NULL (hipGraph replay), else from step_host. g2 (may be NULL): a second gradient,
 * summed with g on load — the victim's and the distance term's branches of loss.backward() (attack/KNN/KNN_attack.py:
 * 125-129), which autograd would add in a launch of its own. */
int pc3d_adam_clip_step_f32(float* p, int64_t p_bs, int64_t p_ps, int64_t p_cs,
                            const float* g, int64_t g_bs, int64_t g_ps, int64_t g_cs,
                            const float* g2, int64_t g2_bs, int64_t g2_ps, int64_t g2_cs,
                            float* m, float* v,
                            const float* ori, int64_t o_bs, int64_t o_ps, int64_t o_cs,
                            const float* normal, int64_t n_bs, int64_t n_ps, int64_t n_cs,
                            int B, int K, double lr, double beta1, double beta2, double eps, float budget,
                            const int32_t* step_dev, int step_host, void* stream);

/* *ctr += delta on the stream (advances the Adam step word between graph replays). */
int pc3d_i32_add(int32_t* ctr, int delta, void* stream);

/* Dense pairwise distances out[b,i,j] (contiguous [B,N,M] f32): mode 0 = |x_i-y_j|^2, mode 1 = Euclidean.
 * For callers that really consume the matrix: _Distance.batch_pairwise_dist (distance.py:15-32),
 * dis_utils_torch.pairwise_distances (:8-11), dis_utils_numpy.pairwise_distances (:13-20),
 * pointnet2_utils.square_distance (model/pointnet2_utils.py:19-38). Direct-difference form. */
int pc3d_pairwise_f32(const float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs,
                      const float* y, int64_t y_bs, int64_t y_ps, int64_t y_cs,
                      int B, int N, int M, int mode, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * K2/K4  K nearest reference points (xyz, squared L2, direct-difference form) of every query, ascending;
 * ties put the lower reference index first. 1 <= K <= min(64, M). dists/idx: [B,N,K] f32 / i32 (either may be NULL).
 * Replaces the [B,N,M] matrix + topk of attack/CW/CW_utils/dist_utils.py:133-144 (KNNDist),
 * attack/GeoA3/knn_utils.py:10-55 (knn_points), attack/AOF/TAOF_attack.py:13-28, model/dgcnn.py:194-200 on xyz,
 * model/curvenet_util.py:10-17. Self-kNN (q == r) returns the point itself first (distance 0), like the reference.
 * ------------------------------------------------------------------------------------------------------- */
int pc3d_knn_f32(const float* q, int64_t q_bs, int64_t q_ps, int64_t q_cs,
                 const float* r, int64_t r_bs, int64_t r_ps, int64_t r_cs,
                 int B, int N, int M, int K, float* dists, int32_t* idx, void* stream);
/* The neighbour graph of ONE cloud set (self-kNN, K = k + 1 columns, self first) with the two views of it that
 * CurveNet's blocks use (model/curvenet_util.py:10-17 `knn`, :232 `idx[:, :, :k]`, walk.py `idx[:, :, 1:]`) written by the
 * same launch instead of two slicing copies per resolution: idx [B,N,K]; idx_noself [B,N,K-1] (may be NULL) = columns
 * 1 .. K-1; idx_first [B,N,k2] (may be NULL, k2 <= K) = columns 0 .. k2-1. Same search and tie rule as pc3d_knn_f32. */
int pc3d_knn_graph_i32(const float* pts, int64_t p_bs, int64_t p_ps, int64_t p_cs, int B, int N, int K, int32_t* idx,
                       int32_t* idx_noself, int32_t* idx_first, int k2, void* stream);
/* The same two searches with a HINT: hint [B,N,K] int32 (may be NULL, may be `idx` itself — a wavefront reads the rows of
 * its queries before it writes them) holds K reference indices per query from an earlier search of nearly the same clouds:
 * the previous iteration of an attack loop (the reference re-runs its matrix + topk from scratch every iteration,
 * model/curvenet_util.py:10-17, attack/CW/CW_utils/dist_utils.py:133-144). Their largest distance bounds the K-th
 * distance, so only candidates at or below it are ever inserted (K + a few instead of K ln(M / K) per query). The RESULT
 * does not depend on the hint — distances, indices and tie order are those of pc3d_knn_f32; a hint row that is out of
 * range, repeats an index or has a non-finite bound makes its wavefront run the unhinted scan. */
int pc3d_knn_hint_f32(const float* q, int64_t q_bs, int64_t q_ps, int64_t q_cs,
                      const float* r, int64_t r_bs, int64_t r_ps, int64_t r_cs,
                      int B, int N, int M, int K, float* dists, int32_t* idx, const int32_t* hint, void* stream);
int pc3d_knn_graph_hint_i32(const float* pts, int64_t p_bs, int64_t p_ps, int64_t p_cs, int B, int N, int K, int32_t* idx,
                            int32_t* idx_noself, int32_t* idx_first, int k2, const int32_t* hint, void* stream);
/* pc3d_knn_hint_f32 on a batch of clouds of different sizes. len_q / len_r: int32 [B] on the device (they may be the same
 * pointer), read by the kernel as data, so one captured launch serves any lengths. N and M stay the capacities: the row
 * strides of dists / idx / hint ([B,N,K]) and the grid. Cloud b, with n = clamp(len_q[b], 0, N), m = clamp(len_r[b], 0, M):
 * the queries i < n search the candidates 0 .. m-1 only; rows i >= n of dists / idx are neither read nor written. The
 * tiling starts at candidate 0 and the tile does not depend on m, ties keep the lowest index: row i of cloud b equals, in
 * every bit (distances and indices), pc3d_knn_f32 on that cloud alone at N = n, M = m. A hint entry >= m makes its
 * wavefront run the unhinted scan; the result never depends on the hint.
 * PRECONDITION m >= K for every cloud with n > 0: the lengths are device data, so the caller checks it (on a cloud that
 * breaks it the rows hold unspecified values). Whatever the two buffers hold, nothing outside the buffers is read or
 * written (the clamps). K <= M is checked against the capacity. */
int pc3d_knn_ragged_f32(const float* q, int64_t q_bs, int64_t q_ps, int64_t q_cs,
                        const float* r, int64_t r_bs, int64_t r_ps, int64_t r_cs,
                        int B, int N, int M, int K, float* dists, int32_t* idx, const int32_t* hint,
                        const int32_t* len_q, const int32_t* len_r, void* stream);
/* Values only, small k: dists [B,N,k1] = the k1 smallest squared distances of every query, ascending, 2 <= k1 <= 9,
 * k1 <= M; no indices. Bit for bit the dists of pc3d_knn_f32 (same distance arithmetic, same key order, NaN stored as
 * +inf, the same far sentinels up to the next multiple of 64 candidates): the k1 smallest keys of a multiset do not
 * depend on the order of the scan. One query per lane with its list in registers (csrc/knn_small.hip); what the SOR
 * defence needs of a search (k1 = 3, attack/SIadv/baselines/defense/drop_points/SOR.py:34-43). */
int pc3d_knn_small_f32(const float* q, int64_t q_bs, int64_t q_ps, int64_t q_cs,
                       const float* r, int64_t r_bs, int64_t r_ps, int64_t r_cs,
                       int B, int N, int M, int k1, float* dists, void* stream);


/* Backward of the K distances with upstream w [B,N,K]: grad_q dense, grad_r scattered (float atomics; when
 * deterministic != 0 in a fixed order: with det_ws = B*N*K*3 floats of scratch the edges' contributions are recorded
 * and summed by the ordered LDS scatter of pc3d_scatter_rows_det_f32, with det_ws NULL every reference point scans
 * the whole index list). Both are OVERWRITTEN; either may be NULL. When q and r are the same cloud (self-kNN) the
 * caller adds the two results. */
int pc3d_knn_bwd_f32(const float* q, int64_t q_bs, int64_t q_ps, int64_t q_cs,
                     const float* r, int64_t r_bs, int64_t r_ps, int64_t r_cs,
                     int B, int N, int M, int K, const int32_t* idx, const float* w,
                     float* grad_q, int64_t gq_bs, int64_t gq_ps, int64_t gq_cs,
                     float* grad_r, int64_t gr_bs, int64_t gr_ps, int64_t gr_cs,
                     int deterministic, float* det_ws, void* stream);
/* Self-kNN form of that backward (q and r are the SAME cloud x, the kNN attack's regulariser): grad [B,N,3 strides] =
 * the dense term + the scattered term in one buffer; w_scale [B] (may be NULL) multiplies every w[b,...] — an upstream
 * per-sample gradient folded into the launch. deterministic / det_ws as above. */
int pc3d_knn_self_bwd_f32(const float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs, int B, int N, int K,
                          const int32_t* idx, const float* w, const float* w_scale, float* grad, int64_t g_bs, int64_t g_ps,
                          int64_t g_cs, int deterministic, float* det_ws, void* stream);
/* The kNN-distance outlier penalty of the kNN attack (attack/CW/CW_utils/dist_utils.py:112-160 KNNDist.forward) from the
 * K1 = k + 1 sorted self-kNN distances d [B,N,K1] (entry 0 = the point itself): value_i = mean_{j>=1} d[i,j]; thr =
 * mean_i value + alpha * std_i value (unbiased); loss[b] = mean_i value_i [value_i > thr]; and the weights its backward
 * hands to pc3d_knn_self_bwd_f32: w[b,i,j] = [value_i > thr] / (N k) for j >= 1, 0 for j = 0 (the mask is a constant of
 * the graph, :146-151). One workgroup per sample, fixed-order reductions. */
int pc3d_knn_outlier_loss_f32(const float* d, int B, int N, int K1, float alpha, float* loss, float* w, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * K11  per-iteration bookkeeping of the CW-family loops on the device (attack/CW/CW_attack.py:129-153): per-sample
 * dist = ||adv-ori||_F, success = (pred != label) [untarget] or (pred == label); where success && dist < bestdist
 * update (bestdist, bestscore); where success && dist < o_bestdist update (o_bestdist, o_bestscore) and copy adv[b]
 * into o_bestattack[b]. input_val (may be NULL) always receives adv (the iterate this pass started from, :133).
 * dist_val[B] (may be NULL) receives dist; *step (may be NULL) is incremented by one (the Adam step word).
 * Replaces the D2H copy of the whole cloud + Python per-sample loop of every iteration.
 * ------------------------------------------------------------------------------------------------------- */
int pc3d_cw_bookkeep_f32(const float* adv, int64_t a_bs, int64_t a_ps, int64_t a_cs,
                         const float* ori, int64_t o_bs, int64_t o_ps, int64_t o_cs, int B, int K,
                         const int64_t* pred, const int64_t* label, int untarget,
                         float* bestdist, int64_t* bestscore, float* o_bestdist, int64_t* o_bestscore,
                         float* o_bestattack, int64_t ba_bs, int64_t ba_ps, int64_t ba_cs,
                         float* input_val, int64_t iv_bs, int64_t iv_ps, int64_t iv_cs,
                         float* dist_val, int32_t* step, void* stream);

/* CW update in one launch: g = g_model + d/dadv[ mean_b w[b] * D(adv_b, ori_b) ]; Adam (as pc3d_adam_clip_step_f32);
 * per-point clip to `budget` (ClipPointsLinf; <= 0: none). dist_kind 0: none; 1: L2Dist (needs l2norm[B] =
 * ||adv-ori||_F, e.g. dist_val of the bookkeeping launch); 2: ChamferDist('adv2ori') (needs nn_idx [B,K] from
 * pc3d_nn_f32). Replaces loss.backward() of the distance term + opt.step() + clip_func (CW_attack.py:161-174). */
int pc3d_cw_step_f32(float* p, int64_t p_bs, int64_t p_ps, int64_t p_cs,
                     const float* g, int64_t g_bs, int64_t g_ps, int64_t g_cs, float* m, float* v,
                     const float* ori, int64_t o_bs, int64_t o_ps, int64_t o_cs, int B, int K,
                     double lr, double beta1, double beta2, double eps, float budget,
                     const int32_t* step_dev, int step_host, int dist_kind, const float* w,
                     const float* l2norm, const int32_t* nn_idx, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * K5  farthest-point sampling (model/pointnet2_utils.py:60-81; model/curvenet_util.py:69-90 with start 0).
 * One workgroup per cloud performs all S dependent arg-max steps on chip. start[B] = first sampled index per
 * cloud (the reference draws it with torch.randint every forward, SURVEY A-4; NULL = 0). out [B,S] i32.
 * Same fp32 arithmetic as the reference (((dx*dx+dy*dy)+dz*dz), running min initialised to 1e10, lowest index on
 * ties) so the index sequence is reproduced bit for bit. N <= 8192.
 * ------------------------------------------------------------------------------------------------------- */
int pc3d_fps_f32(const float* xyz, int64_t x_bs, int64_t x_ps, int64_t x_cs, int B, int N, int S,
                 const int32_t* start, int32_t* out, void* stream);
/* The same sampling with the workgroup size named (64, 128, 256, 512 or 1024 threads per cloud, N <= 32 * threads; results
 * are identical; pc3d_fps_f32 takes 64 up to N = 512, else 256): for tests and measurements. */
int pc3d_fps_threads_f32(int threads, const float* xyz, int64_t x_bs, int64_t x_ps, int64_t x_cs, int B, int N, int S,
                         const int32_t* start, int32_t* out, void* stream);
/* The same sampling on ONE wavefront per cloud with exact pruning (csrc/fps_pruned.hip): the cloud is split into rows of 64
 * spatially close points (a k-d partition built inside the launch), and a step updates only the rows whose bounding box is
 * closer to the new centre than the row's largest running distance. Same arithmetic per point, ties to the lowest index:
 * the index sequence equals pc3d_fps_threads_f32's bit for bit. N <= 4096. Measured no faster than the full-update kernel
 * (DESIGN.md §3.9), so pc3d_fps_f32 does not choose it; kept for the evidence and as the base of further work. */
int pc3d_fps_pruned_f32(const float* xyz, int64_t x_bs, int64_t x_ps, int64_t x_cs, int B, int N, int S,
                        const int32_t* start, int32_t* out, void* stream);


/* K6  ball query (model/pointnet2_utils.py:84-104): out[b,s,:] = the first `nsample` point indices in ascending
 * order with |xyz_i - centers_s|^2 <= radius^2, padded with the first hit (N if there is none). out [B,S,nsample] i32.
 * Direct-difference distances (the reference's -2ab+a^2+b^2 differs by fp32 rounding at the ball's surface). */
int pc3d_ball_query_f32(const float* xyz, int64_t x_bs, int64_t x_ps, int64_t x_cs,
                        const float* centers, int64_t c_bs, int64_t c_ps, int64_t c_cs,
                        int B, int N, int S, float radius, int nsample, int32_t* out, void* stream);
/* The same query on a named kernel (pc3d_ball_query_f32 chooses by problem size; results are identical): kernel 1 = a
 * wavefront per centre, 2 = a centre per lane with the cloud split over the workgroup's four wavefronts (N <= 65535,
 * nsample <= 96). For tests and measurements. */
int pc3d_ball_query_kernel_f32(int kernel, const float* xyz, int64_t x_bs, int64_t x_ps, int64_t x_cs,
                               const float* centers, int64_t c_bs, int64_t c_ps, int64_t c_cs,
                               int B, int N, int S, float radius, int nsample, int32_t* out, void* stream);

/* K7  group gather, channels-last (model/pointnet2_utils.py:41-57,121-131): out[b,s,j,:] =
 * [xyz[b,idx[b,s,j]] - centers[b,s] (3, xyz may be NULL), feat[b,idx[b,s,j],:] (D, feat [B,N,D] contiguous or NULL)].
 * centers NULL = no subtraction (plain index_points). out [B,S,ns,3+D] contiguous. */
int pc3d_group_gather_f32(const float* xyz, int64_t x_bs, int64_t x_ps, int64_t x_cs, const float* feat, int D,
                          const int32_t* idx, const float* centers, int64_t c_bs, int64_t c_ps, int64_t c_cs,
                          int B, int N, int S, int ns, float* out, void* stream);

/* Backward of K7: grad_xyz [B,N,3] / grad_feat [B,N,D] (contiguous, OVERWRITTEN, either may be NULL) receive the
 * scatter-add of g_out [B,S,ns,(3)+D]; center_idx [B,S] (index of each centre in xyz, or NULL) receives minus the
 * sum over its group. det_ws NULL: float atomics (order-dependent in the last bits); det_ws = B*S*3 floats of scratch:
 * the ordered LDS scatter of pc3d_scatter_rows_det_f32 (deterministic). */
int pc3d_group_gather_bwd_f32(const float* g_out, const int32_t* idx, const int32_t* center_idx, int B, int N, int S,
                              int ns, int D, int has_xyz, float* grad_xyz, float* grad_feat, float* det_ws, void* stream);

/* Backward to x of out[g,c] = max_r relu(x[g,r,:] . W[c,:] + b[c]) — the last 1x1 conv + ReLU + max over the group of
 * a set-abstraction layer (model/pointnet2_utils.py:190-197, :243-257). gout/out [G,C3], arg [G,C3] int64 = winning row
 * inside the group (torch.max indices), W [C3,C2]; gx [G,ns,C2] overwritten. Sparse row accumulation in ascending
 * channel order (deterministic) instead of autograd's dense product on a one-nonzero-per-channel tensor. ns <= 128.
 * xin (may be NULL): x itself when x is the ReLU output of the previous layer — gx is zeroed where xin <= 0, which folds
 * that layer's ReLU backward into this launch. */
/* Forward of that operator without the [G*ns, C3] activation: out[g,c] = max_r relu(x[g,r,:] . W[c,:] + b[c]),
 * arg[g,c] = the winning row (int64, lowest on ties; unspecified where out == 0). x [G,ns,C2], ns <= 128,
 * C2 % 8 == 0 and <= 128, C3 % 32 == 0. fp32 MFMA. */
int pc3d_group_linear_max_f32(const float* x, const float* W, const float* b, int G, int ns, int C2, int C3,
                              float* out, int64_t* arg, void* stream);
/* The same with the kernel named (identical results): 0 = the library chooses, 1 = a workgroup per group, 2 = the
 * tiled GEMM main loop with a group-max epilogue (ns in {32, 64, 128} only, else PC3D_EINVAL). */
int pc3d_group_linear_max_kernel_f32(int kernel, const float* x, const float* W, const float* b, int G, int ns, int C2,
                                     int C3, float* out, int64_t* arg, void* stream);
int pc3d_group_max_linear_bwd_f32(const float* gout, const float* out, const int64_t* arg, const float* W,
                                  int G, int ns, int C2, int C3, const float* xin, float* gx, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * K3  DGCNN dynamic graph (model/dgcnn.py:194-227,299-313).
 * pc3d_knn_feat_f32: idx[b,i,:] = the K nearest points of i in C-dimensional feature space (self included, nearest
 * first, lowest index on ties) for channels-last features x [B,N,C]; C % 8 == 0, C <= 128, K <= 64, any N. The
 * distances |xi-xj|^2 = |xi|^2 + |xj|^2 - 2 xi.xj of 32 queries x 128 references at a time are formed by fp32 MFMA in
 * LDS and scanned against K-lists held across the lanes; nothing of size N*N reaches HBM (the reference writes
 * [B,N,N] and calls topk).
 * pc3d_gather_max_f32: out[b,i,c] = max (sign[c] < 0: min; sign NULL: max) over j in idx[b,i,:] of P[b,j,c], with
 * the winning j in arg (may be NULL) — the neighbour reduction of an EdgeConv expressed as W[xj-xi; xi] = P_j + Q_i.
 * pc3d_gather_max_bwd_f32: gP[b,arg,c] += g (gP overwritten; deterministic = 0: global float atomics, 1: one wavefront
 * per (cloud, channel slice) accumulates in LDS in source order — see pc3d_scatter_rows_det_f32).
 * ------------------------------------------------------------------------------------------------------- */
int pc3d_knn_feat_f32(const float* x, int B, int N, int C, int K, int32_t* idx, void* stream);
int pc3d_gather_max_f32(const float* P, const int32_t* idx, const float* sign, int B, int N, int C, int K,
                        float* out, int32_t* arg, void* stream);
int pc3d_gather_max_bwd_f32(const float* g, const int32_t* arg, int B, int N, int C, float* gP, int deterministic,
                            void* stream);
/* The same reduction for S query rows over N source points (idx, out, arg, g: [B,S,..]; P, gP: [B,N,C]; indices are
 * clamped to [0,N-1]): CurveNet's MaskedMaxPool, max over the ball-query neighbours of every FPS centroid
 * (model/curvenet_util.py:469-484). */
int pc3d_gather_max_rows_f32(const float* P, const int32_t* idx, int B, int N, int S, int C, int K, float* out,
                             int32_t* arg, void* stream);
int pc3d_gather_max_rows_bwd_f32(const float* g, const int32_t* arg, int B, int N, int S, int C, float* gP,
                                 int deterministic, void* stream);

/* -------------------------------------------------------------------------------------------------------
 * Deterministic scatter-add (new; the reference's autograd of index_points / get_graph_feature / knn_gather —
 * model/pointnet2_utils.py:41-57, model/dgcnn.py:203-227, attack/GeoA3/knn_utils.py:58-86 — is deterministic on its CPU
 * path, a scatter with global float atomics is not):
 *   out[b, tgt[b,r], c] = sum over the records r = 0 .. R-1, in that order, of m(val[b,r,c])
 * with m = identity, or the derivative of a LeakyReLU taken from the sign of act[b,r,c]. ONE wavefront owns the LDS tile
 * of all N destination rows x a slice of channels and walks the records in order (ds_add_f32 of one wave execute in
 * issue order), so the result is a pure function of the inputs: the same run to run, under hipGraph replay, and for a
 * cloud alone or inside a batch. tgt [B,R] int32 (outside [0,N): skipped, or clamped when clamp = 1); val [B,R,ldv],
 * act [B,R,lda] or NULL; out [B,N,ldo] overwritten (accumulate = 1: added to). N <= 40960 (a CU's LDS).
 * The deterministic modes of the backward entry points above run on this kernel.
 * ------------------------------------------------------------------------------------------------------- */
/* Sorted reverse index of a gather (CSR): for idx [B,E] int32 with values in [0,NA) (clamp = 1: clamped into it; 0:
 * others are in no list), lst[b, off[b,t] .. off[b,t+1]) = the entries e with idx[b,e] == t in ASCENDING e. cnt [B,NA]
 * int32 scratch, off [B,NA+1], lst [B,E]. pc3d_rev_gather_sum_f32: out[b,t,:] = sum over that segment, front to back, of
 * m(val[b,e,:]) (m as for pc3d_scatter_rows_det_f32) — the same sums as the scatter below, every destination row in
 * parallel; what the deterministic backward of the wide many-edge gathers (LPFA) runs on. */
int pc3d_rev_index_i32(const int32_t* idx, int B, int E, int NA, int clamp, int32_t* cnt, int32_t* off, int32_t* lst,
                       void* stream);
int pc3d_rev_gather_sum_f32(const float* val, int64_t ldv, const float* act, int64_t lda, float slope, const int32_t* off,
                            const int32_t* lst, int B, int E, int NA, int C, float* out, int64_t ldo, void* stream);
int pc3d_scatter_rows_det_f32(const int32_t* tgt, const float* val, int64_t ldv, const float* act, int64_t lda, float slope,
                              int B, int R, int N, int C, float* out, int64_t ldo, int accumulate, int clamp, void* stream);
/* One EdgeConv layer's epilogue (model/dgcnn.py:299-313): PQ [B,N,2C] = [P | Q] from ONE GEMM against [U;V];
 * out[b,i,c] = leaky_slope(max_j P[b,idx[b,i,j],c] + Q[b,i,c]), arg = the winning j. C % 4 == 0.
 * Backward: gPQ [B,N,2C] overwritten: dQ = g * leaky'(out), dP scattered to arg (float atomics). */
int pc3d_edge_max_f32(const float* PQ, const int32_t* idx, int B, int N, int C, int K, float slope,
                      float* out, int32_t* arg, void* stream);
/* The same launch also writing out into a column slice of a wider buffer (out2 + (b N + i) ld2, 16-byte aligned, ld2 % 4 == 0):
 * DGCNN concatenates its four EdgeConv outputs for conv5 (model/dgcnn.py:315 `torch.cat`) — written here, the copy goes. */
int pc3d_edge_max_cat_f32(const float* PQ, const int32_t* idx, int B, int N, int C, int K, float slope,
                          float* out, int32_t* arg, float* out2, int64_t ld2, void* stream);
/* Global pooling head (model/dgcnn.py:317-320, model/curvenet.py:64-67): z = leaky_slope(Y) (slope 0: ReLU),
 * out[b, 0:C] = max_i z[b,i,:], out[b, C:2C] = mean_i z[b,i,:], arg [B,C] = lowest arg-max row; one pass over
 * Y [B,N,C]. Backward: gY overwritten in one pass from gout [B,2C]. C % 4 == 0. Deterministic. */
int pc3d_act_pool_f32(const float* Y, int B, int N, int C, float slope, float* out, int32_t* arg, void* stream);
int pc3d_act_pool_bwd_f32(const float* Y, const float* gout, const int32_t* arg, int B, int N, int C, float slope,
                          float* gY, void* stream);
/* g [B,N,C] with row stride ldg >= C floats: the slice of a wider gradient (the backward of DGCNN's torch.cat over the four
 * EdgeConv outputs hands over [B,N,512] column slices) is read in place. */
int pc3d_edge_max_bwd_f32(const float* g, int64_t ldg, const float* out, const int32_t* arg, int B, int N, int C,
                          float slope, float* gPQ, int deterministic, void* stream);
/* The deterministic form with the channel-slice width of its owner-wave kernel named (slice & 255: 1, 2, 4, 8, 16; 0 = the
 * library chooses; identical results for every width — a wavefront per (cloud, slice) sums the points in order). Two more bits
 * for measurements: 256 = fp32 instead of fp64 LDS tiles, 512 = workgroups in launch order instead of XCD bands. */
/* The deterministic form for an EdgeConv output with TWO consumers (DGCNN: conv5 through the concatenation, and the next
 * layer): the upstream gradient is g + g2 (one fp32 add per element, on load), g2 [B,N,ldg2 >= C] — the sum autograd would
 * form in a launch of its own (model/dgcnn.py:299-315 under autograd). */
int pc3d_edge_max_bwd_sum_f32(const float* g, int64_t ldg, const float* g2, int64_t ldg2, const float* out,
                              const int32_t* arg, int B, int N, int C, float slope, float* gPQ, void* stream);
int pc3d_edge_max_bwd_slice_f32(const float* g, int64_t ldg, const float* out, const int32_t* arg, int B, int N, int C,
                                float slope, float* gPQ, int slice, void* stream);

/* K16  guided curve walk of CurveNet (model/walk.py:74-153 `Walk.forward`), one launch per step and direction: one or
 * two curves per wavefront, lane j scores neighbour j. feats [B,N,C] (C in {8,16,32,64}), adj [B,N,k] (k <= 64, self
 * excluded), start [B,cn]. agent_w [2C] / agent_b [1]: the 1x1 agent conv + eval BatchNorm folded, neighbour part
 * first (walk.py:128-131); mom_w [2,2C] / mom_b [2]: the momentum conv folded, current-feature columns first
 * (walk.py:104-115). Per step: descriptor blend by the 2-way softmax momentum, neighbour scores damped by
 * clamp(1 + cos(last move, candidate move), 0, 1) (walk.py:55-72), hard arg-max pick (lowest slot on ties) with the
 * softmax as its straight-through gradient. Outputs: curves [B,cn,L,C] (the reference's [B,C,cn,L] transposed) and,
 * for the backward, nodes / pick [B,cn,L], pre [B,cn,L,C], mom [B,cn,L,2].
 * Backward: gfeats [B,N,C] and coef [B,N] are ACCUMULATED into (zero them first); the full gradient is
 * gfeats + coef (x) agent_w[0:C] (the rank-1 score term is left to the caller as one dense pass). Float atomics.
 * deterministic = 1: the steps record their contributions in ws and the entry point sums them in record order with
 * the ordered LDS scatter (pc3d_scatter_rows_det_f32); gfeats and coef are then OVERWRITTEN, and gfeats already
 * INCLUDES the rank-1 term coef (x) agent_w[0:C] (added by the scatter on its way out: no dense pass for the caller).
 * ws: pc3d_curve_walk_bwd_ws_floats(B, cn, C, L, k, deterministic) floats of scratch (the gradients that travel from
 * step to step; in deterministic mode also the records). */
int pc3d_curve_walk_fwd_f32(const float* feats, const int32_t* adj, const int32_t* start, const float* agent_w,
                            const float* agent_b, const float* mom_w, const float* mom_b, int B, int N, int C, int k,
                            int cn, int L, float* curves, int32_t* nodes, int32_t* pick, float* pre, float* mom,
                            void* stream);
int pc3d_curve_walk_bwd_f32(const float* gcurves, const float* feats, const int32_t* adj, const float* agent_w,
                            const float* agent_b, const float* mom_w, const float* mom_b, int B, int N, int C, int k,
                            int cn, int L, const float* curves, const int32_t* nodes, const int32_t* pick,
                            const float* pre, const float* mom, float* gfeats, float* coef, float* ws, int deterministic,
                            void* stream);
int64_t pc3d_curve_walk_bwd_ws_floats(int B, int cn, int C, int L, int k, int deterministic);

/* K17  the two bandwidth-bound halves of CurveNet's local point-feature aggregation (model/curvenet_util.py:199-236,
 * `LPFA.group_feature` / `LPFA.forward`) around its 1x1-conv GEMM; channels-last, C % 4 == 0:
 *   edge_act: E[b,i,j,:] = leaky_slope(A[b,idx[b,i,j],:] + Bc[b,i,:])   A, Bc [B,N,C], idx [B,N,K] -> E [B,N,K,C]
 *             backward: gBc [B,N,C] overwritten, gA [B,N,C] ACCUMULATED (zero it first; float atomics)
 *   act_mean: out[b,i,:] = mean_j leaky_slope(Z[b,i,j,:])                Z [B,N,K,C] -> out [B,N,C]
 *             backward: gZ overwritten (deterministic). */
int pc3d_edge_act_f32(const float* A, const float* Bc, const int32_t* idx, int B, int N, int K, int C, float slope,
                      float* E, void* stream);
int pc3d_edge_act_bwd_f32(const float* gE, const float* E, const int32_t* idx, int B, int N, int K, int C, float slope,
                          float* gA, float* gBc, int deterministic, const int32_t* rev_off, const int32_t* rev_lst,
                          void* stream);
/* (deterministic = 0: gA must be zero-filled by the caller, float atomics; 1: gA overwritten — by a gather through the
 * sorted reverse index of idx when rev_off / rev_lst (pc3d_rev_index_i32 with E = N*K, NA = N, clamp = 1) are given,
 * else by the ordered LDS scatter) */
int pc3d_act_mean_f32(const float* Z, int B, int N, int K, int C, float slope, float* out, void* stream);
int pc3d_act_mean_bwd_f32(const float* Z, const float* gout, int B, int N, int K, int C, float slope, float* gZ,
                          void* stream);
/* The whole LPFA block for ONE 1x1-conv layer of equal width (model/curvenet_util.py:204-236 with mlp_num = 1, what every
 * CIC block of the classifier uses) in one launch each way, without any [B,N,K,C] tensor:
 *   out[b,i,:] = mean_j LeakyReLU_s2( W . LeakyReLU_s1(A[b,idx[b,i,j],:] + Bc[b,i,:]) + bias )
 * A, Bc, out, gout, gA, gBc [B,N,C]; idx [B,N,K] int32 (clamped); W [C,C] (out, in), Wt its transpose; C in
 * {16,32,64,128}, K <= 30. Backward: gA, gBc overwritten — gA through float atomics when edge_scratch is NULL, else
 * deterministically: the per-edge gradients go to edge_scratch [B,N,K,C] and every gA row sums its edges in ascending edge
 * order — a gather through the sorted reverse index of idx (rev_off / rev_lst from pc3d_rev_index_i32, E = N*K, NA = N,
 * clamp = 1) when given, else the ordered LDS scatter. */
int pc3d_lpfa_fused_f32(const float* A, const float* Bc, const int32_t* idx, const float* W, const float* bias, int B,
                        int N, int K, int C, float slope1, float slope2, float* out, void* stream);
int pc3d_lpfa_fused_bwd_f32(const float* gout, const float* A, const float* Bc, const int32_t* idx, const float* W,
                            const float* Wt, const float* bias, int B, int N, int K, int C, float slope1, float slope2,
                            float* gA, float* gBc, float* edge_scratch, const int32_t* rev_off, const int32_t* rev_lst,
                            void* stream);

/* K18  per-cloud half of CurveNet's curve aggregation (model/curvenet_util.py:379-437 `CurveAggregation.forward`):
 * curves [B,cn,cl,C] (channels-last) -> attention keys Kp [B,C,R] and values Vp [B,R,C], R = cn + cl, such that the
 * block's output is leaky(x + softmax_rows(x^T Kp[:, :cn]) Vp[:cn] + softmax_rows(x^T Kp[:, cn:]) Vp[cn:]).
 * w_att [C] (line_conv_att), Wa / Wb / Wc [mid,C] (conva / convb / convc), Wn / Wl [mid,mid] (convn / convl),
 * Wd [C,2 mid] + bd [C] (convd with its eval BatchNorm folded; bd is added to the first cn value rows).
 * LDS-resident, weights included: pc3d_curve_agg_lds_bytes(cn, cl, C, mid, backward) bytes, which must not exceed the
 * CU's 160 KB (error otherwise; the classifier's blocks need 58 / 97 KB). Backward: gcurves [B,cn,cl,C] overwritten
 * from gKp / gVp; deterministic. */
int64_t pc3d_curve_agg_lds_bytes(int cn, int cl, int C, int mid, int backward);
int pc3d_curve_agg_kv_f32(const float* curves, const float* w_att, const float* Wa, const float* Wb, const float* Wn,
                          const float* Wl, const float* Wc, const float* Wd, const float* bd, int B, int cn, int cl,
                          int C, int mid, float* Kp, float* Vp, void* stream);
int pc3d_curve_agg_kv_bwd_f32(const float* gKp, const float* gVp, const float* curves, const float* w_att,
                              const float* Wa, const float* Wb, const float* Wn, const float* Wl, const float* Wc,
                              const float* Wd, const float* bd, int B, int cn, int cl, int C, int mid, float* gcurves,
                              void* stream);

/* K19  channels-last glue of a CurveNet CIC block (csrc/curvenet_cl.hip); all tensors fp32, C % 4 == 0.
 *   att_scale (model/curvenet_util.py:452-455, CurveGrouping): att[p] = sigmoid(x[p,:] . w), xs[p,:] = x[p,:] att[p]
 *     for M rows; backward to x of a gradient on xs (att itself only feeds the top-k selection).
 *   topk_desc (:457): indices of the K largest scores of every cloud, descending, ties to the lower index (the
 *     reference asks torch.topk for sorted=False, whose order is device dependent — DESIGN.md A-15). N <= 8192.
 *   curve_attn (:425-437, CurveAggregation's per-point half): with the keys Kp [B,C,R] / values Vp [B,R,C] of
 *     pc3d_curve_agg_kv_f32 (R = cn + cl),  out = LeakyReLU_slope(x + softmax(x Kp[:, :cn]) Vp[:cn] + softmax(x Kp[:, cn:])
 *     Vp[cn:]).  C in {8,16,32,64}, R <= 128. Backward: gx [B,N,C], gKp, gVp (overwritten); ws = device scratch of
 *     pc3d_curve_attn_bwd_ws_floats(..) floats.
 *   lpfa_prep (:204-236, LPFA): A = x + p G1^T, Bc = p G2^T + t - x for M rows (x [M,C], p [M,3], G1, G2 [C,3], t [C]),
 *     the two per-point terms of leaky((x_j - x_i) + xyz2feature([p_i; p_j; p_j - p_i])) = leaky(A_j + Bc_i); backward
 *     gx = gA - gBc, gp = gA G1 + gBc G2. */
int pc3d_att_scale_f32(const float* x, const float* w, int64_t M, int C, float* xs, float* att, void* stream);
int pc3d_att_scale_bwd_f32(const float* g, const float* x, const float* att, const float* w, int64_t M, int C, float* gx,
                           void* stream);
int pc3d_topk_desc_f32(const float* score, int B, int N, int K, int32_t* idx, void* stream);
int pc3d_curve_attn_f32(const float* x, const float* Kp, const float* Vp, int B, int N, int C, int cn, int cl,
                        float slope, float* out, void* stream);
int64_t pc3d_curve_attn_bwd_ws_floats(int B, int N, int C, int cn, int cl);
int pc3d_curve_attn_bwd_f32(const float* gout, const float* out, const float* x, const float* Kp, const float* Vp, int B,
                            int N, int C, int cn, int cl, float slope, float* gx, float* gKp, float* gVp, float* ws,
                            void* stream);
int pc3d_lpfa_prep_f32(const float* x, const float* pts, const float* G1, const float* G2, const float* t, int64_t M,
                       int C, float* A, float* Bc, void* stream);
int pc3d_lpfa_prep_bwd_f32(const float* gA, const float* gBc, const float* G1, const float* G2, int64_t M, int C,
                           float* gx, float* gpts, void* stream);

/* K12  dense graph Laplacian L = D - A of the symmetrised kNN graph with Gaussian weights A_ij = exp(-|pi-pj|^2)
 * (attack/AOF/TAOF_attack.py:31-52, attack/AOF/Eval_AOF.py:72-93). idx [B,N,K] from pc3d_knn_f32 (self included, as
 * in the reference's topk); L [B,N,N] f32 is overwritten. Only the N*K graph edges are evaluated. */
int pc3d_graph_laplacian_f32(const float* xyz, int64_t x_bs, int64_t x_ps, int64_t x_cs,
                             const int32_t* idx, int B, int N, int K, float* L, void* stream);

/* K12b  AOF's per-iteration spectral re-projection (attack/AOF/TAOF_attack.py:114-126 at the start of a binary step,
 * :164-170 after every optimiser step): coeff = adv . V, lfc = coeff[..., :lp] . V[..., :lp]^T, hfc = coeff[..., lp:] .
 * V[..., lp:]^T — three torch.bmm with a 3-row left operand in the reference. Here two HBM-bound launches that read V^T
 * and V once each: adv, coeff (scratch), lfc, hfc [B,3,N] contiguous; V [B,N,N] (column j = eigenvector j, as
 * torch.symeig / torch.linalg.eigh return it) and Vt = V^T [B,N,N], both contiguous. Sums in a fixed order. */
int pc3d_spectral_reproject_f32(const float* adv, const float* V, const float* Vt, int B, int N, int lp, float* coeff,
                                float* lfc, float* hfc, void* stream);
/* The same two launches with a fourth output sum = lfc + hfc [B,3,N]: one fp32 add by the thread of the second launch
 * that already holds both values (the bits of torch.add(lfc, hfc)), so the next iteration's adv_pc = lfc + hfc
 * (attack/AOF/Eval_AOF.py:163) costs no launch. lfc, hfc keep the bits of pc3d_spectral_reproject_f32. Every output is
 * its own pointer: lfc and sum may be the two halves of one [2B,3,N] buffer (the victim's stacked pass). */
int pc3d_spectral_reproject_sum_f32(const float* adv, const float* V, const float* Vt, int B, int N, int lp, float* coeff,
                                    float* lfc, float* hfc, float* sum, void* stream);
/* The building block: out[b,c,r] = sum_k vec[b,c,k] * mat[b,r,k] for the 3 rows of vec [B,3,K] against every row of
 * mat [B,R,K]; with out_hi != NULL the columns k < split go to out_lo and the others to out_hi (both [B,3,R]). */
int pc3d_rowdot3_f32(const float* mat, const float* vec, int B, int R, int K, int split, float* out_lo, float* out_hi,
                     void* stream);

/* K12d  the low band of the Laplacian without a dense decomposition (csrc/lowband.hip).
 *
 * pc3d_graph_laplacian_csr_f32: the Laplacian of pc3d_graph_laplacian_f32 as per-cloud CSR. rowptr [B,N+1]; col, val
 * [B,cap] hold the off-diagonal entries -exp(-|pi-pj|^2) (the same arithmetic, the same symmetrised mask, self excluded),
 * columns ascending within a row; deg [B,N] is the diagonal, summed in a fixed order. A pure function of its inputs (no
 * atomics). cap is the caller's capacity per cloud: nothing is written past it, and rowptr[b,N] > cap tells the caller
 * that cloud b did not fit (2 N K always fits; there is no bound on a row's in-degree below N - 1). */
int pc3d_graph_laplacian_csr_f32(const float* xyz, int64_t x_bs, int64_t x_ps, int64_t x_cs, const int32_t* idx, int B, int N,
                                 int K, int cap, int32_t* rowptr, int32_t* col, float* val, float* deg, void* stream);
/* The block size m = min(N, lp + max(guard_min, ceil(lp / guard_div))) of the iteration below (-1: bad arguments), and the
 * bytes of its workspace. */
int pc3d_lowband_block(int N, int lp, int guard_min, int guard_div);
int64_t pc3d_lowband_ws_bytes(int B, int N, int m, int degree);
/* U [B,N,lp] (orthonormal columns spanning the eigenspace of the lowest lp eigenvalues), theta [B,lp] (the Ritz values,
 * ascending) and resid [B] = max_i |L u_i - theta_i u_i|_inf of the CSR Laplacian above, by Chebyshev-filtered block
 * subspace iteration on m <= 128 columns: `iters` outer iterations of a filter of degree <= `degree` (cut where its gain
 * over the block would pass min(range_max, range_first range_growth^it)), two symmetric orthonormalisations through the
 * Gram matrix's eigendecomposition (eigenvalues floored at gram_floor; lost [B], may be NULL, counts the floored ones) and
 * a Rayleigh-Ritz step, the m x m problems on a parallel cyclic Jacobi solver (rotations below jacobi_rel sqrt|a_pp a_qq|
 * + jacobi_abs max|a_ii| skipped, at most jacobi_sweeps sweeps). Filter bounds on the device: upper 2 max deg, lower cut
 * the largest Ritz value of the previous iteration, anchor the smallest, kept cut_min of the upper bound apart. The start
 * block is a hash of (row, column). A fixed launch sequence without host synchronisation; each cloud is a function of its
 * own rows alone. ws: pc3d_lowband_ws_bytes bytes, 8-byte aligned. */
int pc3d_lowband_basis_f32(const int32_t* rowptr, const int32_t* col, const float* val, const float* deg, int B, int N, int cap,
                           int lp, int m, int degree, int iters, float range_first, float range_growth, float range_max,
                           float cut_min, float gram_floor, float jacobi_rel, float jacobi_abs, int jacobi_sweeps, float* U,
                           float* theta, float* resid, int32_t* lost, void* ws, int64_t ws_bytes, void* stream);
/* AOF's re-projection on the band basis: coeff = adv U [B,3,lp] (may be NULL), lfc = coeff U^T, hfc = adv - lfc, and with
 * sum != NULL sum = lfc + hfc as that fp32 sum (the next iterate of the untargeted loop); adv, lfc, hfc, sum [B,3,N]
 * contiguous, each output its own pointer (they may be slices of larger buffers), U [B,N,lp]. Two launches that read U
 * once each, sums in a fixed order. ws: pc3d_band_reproject_ws_floats floats. */
int64_t pc3d_band_reproject_ws_floats(int B, int N, int lp);
int pc3d_band_reproject_f32(const float* adv, const float* U, int B, int N, int lp, float* coeff, float* lfc, float* hfc,
                            float* sum, float* ws, void* stream);

/* K12c  bookkeeping of the untargeted AOF loop on the device (attack/AOF/Eval_AOF.py:168-185), one workgroup per
 * cloud: dist = max |adv - data| over the whole [3,N] cloud (an exact maximum: the bits of torch.amax); where
 * pred != label && dist < o_bestdist && lfc_pred != label (strict <) update (o_bestdist, o_bestscore) and copy adv[b]
 * into o_bestattack[b]. A NaN anywhere in the cloud makes dist NaN and, as numpy's `nan < x` is False, leaves the bests
 * alone. adv, data, o_bestattack [B,3,N] contiguous; pred, lfc_pred, label int64 [B], each its own pointer (the two
 * predictions may be the halves of one [2B] tensor); dist_val [B] (may be NULL) receives dist; *step (may be NULL) is
 * incremented by one (the Adam step word that pc3d_aof_update_f32 reads next). */
int pc3d_aof_record_f32(const float* adv, const float* data, int B, int N, const int64_t* pred, const int64_t* lfc_pred,
                        const int64_t* label, float* o_bestdist, int64_t* o_bestscore, float* o_bestattack,
                        float* dist_val, int32_t* step, void* stream);
/* K12c  the untargeted AOF loop between the backward and the re-projection (attack/AOF/Eval_AOF.py:187-195), one thread
 * per point: g = g1 + g2 (the two terms of the loss, already scaled); torch.optim.Adam on lfc with m, v in place and the
 * step number t (>= 1) from *step_dev when non-NULL, else step_host, in the arithmetic of pc3d_adam_clip_step_f32;
 * out = ClipPointsLinf(lfc + hfc, data): per-point L2 norm, budget / (norm + 1e-9) capped at 1, budget <= 0: none. The
 * bits of pc3d_adam_clip_step_f32 (g2 given, no clip) + torch.add + pc3d_clip_f32 (mode 0). All tensors [B,3,N]
 * contiguous, each its own pointer; out must not alias an input. */
int pc3d_aof_update_f32(float* lfc, const float* g1, const float* g2, float* m, float* v, const float* hfc,
                        const float* data, float* out, int B, int N, double lr, double beta1, double beta2, double eps,
                        float budget, const int32_t* step_dev, int step_host, void* stream);

/* Classifier tail in one launch: logits = c2 W3^T + b3 (fc3), log_softmax / pred / adversarial loss as
 * pc3d_cls_loss_f32, and g_c2 = (g_logits W3) * (c2 > 0) (fc3 backward + ReLU mask of fc2's activation). K2 <= 256,
 * ncls <= 64. *step (may be NULL) is incremented by one. */
int pc3d_cls_tail_f32(const float* c2, int B, int K2, const float* W3, const float* b3, int ncls,
                      const int64_t* target, int kind, float kappa, float scale, float* logp,
                      int64_t* pred, float* loss, float* g_c2, int32_t* step, void* stream);
/* The same by the earlier kernel, which stages W3 and c2 one load -> wait -> LDS write at a time: the same bits. Parity
 * tests and tools/bench_small_launches.py only. */
int pc3d_cls_tail_serial_f32(const float* c2, int B, int K2, const float* W3, const float* b3, int ncls,
                             const int64_t* target, int kind, float kappa, float scale, float* logp,
                             int64_t* pred, float* loss, float* g_c2, int32_t* step, void* stream);

/* pc3d_cw_bookkeep_f32 + pc3d_cw_step_f32 as ONE launch (one workgroup per sample): bookkeeping on the current
 * iterate, then total gradient + Adam + clip on that sample's points. o_bestattack / input_val / m / v share adv's
 * strides; input_val / dist_val may be NULL. The step number is READ from *step_dev (or step_host). */
int pc3d_cw_update_f32(float* adv, int64_t a_bs, int64_t a_ps, int64_t a_cs,
                       const float* ori, int64_t o_bs, int64_t o_ps, int64_t o_cs, int B, int K,
                       const int64_t* pred, const int64_t* label, int untarget,
                       float* bestdist, int64_t* bestscore, float* o_bestdist, int64_t* o_bestscore,
                       float* o_bestattack, float* input_val, float* dist_val,
                       const float* g, int64_t g_bs, int64_t g_ps, int64_t g_cs, float* m, float* v,
                       double lr, double beta1, double beta2, double eps, float budget,
                       const int32_t* step_dev, int step_host, int dist_kind, const float* w,
                       const int32_t* nn_idx, void* stream);
/* pc3d_cw_update_f32 on a batch of clouds of different sizes: sample b counts lengths[b] points (int32 [B] on the
 * device, read as data and clamped to [1, K]); its rows from lengths[b] on are padding, copies of its point 0. The norm,
 * the Chamfer factor 2 w_b / (B lengths[b]), Adam and the clip run over the counted rows with the dense kernel's thread
 * mapping and reduction order, so a sample has the bits of the dense launch on that cloud alone (K = lengths[b]); with
 * all lengths = K every output equals pc3d_cw_update_f32's. Padding rows are never read (they may hold NaN): their m / v
 * stay, adv takes the NEW point 0, input_val / o_bestattack the old one where the dense kernel copies. K <= 8192. */
int pc3d_cw_update_ragged_f32(float* adv, int64_t a_bs, int64_t a_ps, int64_t a_cs,
                              const float* ori, int64_t o_bs, int64_t o_ps, int64_t o_cs, int B, int K,
                              const int32_t* lengths, const int64_t* pred, const int64_t* label, int untarget,
                              float* bestdist, int64_t* bestscore, float* o_bestdist, int64_t* o_bestscore,
                              float* o_bestattack, float* input_val, float* dist_val,
                              const float* g, int64_t g_bs, int64_t g_ps, int64_t g_cs, float* m, float* v,
                              double lr, double beta1, double beta2, double eps, float budget,
                              const int32_t* step_dev, int step_host, int dist_kind, const float* w,
                              const int32_t* nn_idx, void* stream);
/* x[b, :, k] = x[b, :, 0] for every k >= lengths[b] (int32 [B] on the device, clamped to [1, K]), in place, one launch:
 * the padding the ragged update keeps. Rows at and beyond the length are only written; B <= 65535. */
int pc3d_pad_ragged_f32(float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs, const int32_t* lengths, int B, int K,
                        void* stream);

/* The kNN attack's update (attack/KNN/KNN_attack.py:117-136) as ONE launch, one workgroup per sample: the gradient of
 * ChamferkNNDist('adv2ori') from the two search results, Adam and the clip, on the iterate adv (updated IN PLACE; m / v
 * share its strides). It stands for pc3d_knn_outlier_loss_f32 + pc3d_knn_self_bwd_f32 + the Chamfer backward +
 * pc3d_adam_clip_step_f32.
 *   knn_d / knn_idx [B,N,k+1]: the sorted self-kNN of adv, the point itself first (pc3d_knn_hint_f32 with adv as both sets);
 *   nn_idx [B,N]: arg-min over ori of every adv point (pc3d_nn_f32). Indices outside [0,N) are clamped.
 * Per sample: value_i = mean_{j>=1} knn_d[i,j]; thr = mean_i value + alpha * std_i value (unbiased), the arithmetic and
 * summation order of pc3d_knn_outlier_loss_f32; mask_i = value_i > thr, a constant of the graph (dist_utils.py:145-151).
 *   g_knn[i] = mask_i sum_{e>=1} 2 c_knn (x_i - x_idx[i,e])  +  sum_{(i',e): mask_i', idx[i',e] = i} 2 c_knn (x_i - x_i')
 * where the second sum runs over i' ascending, then e ascending (no float atomics: the bits depend on neither the batch
 * nor the launch); g_chamfer[i] = 2 c_chamfer (x_i - ori[nn_idx[i]]); Adam (torch's, weight_decay 0, bias corrections
 * from *step_dev or step_host >= 1, as pc3d_adam_clip_step_f32) on g + (g_chamfer + g_knn); then clip_mode 0:
 * ClipPointsLinf(budget) (budget <= 0: none), clip_mode 1: ProjectInnerPoints with `normal` first (clip_utils.py:74-107;
 * normal NULL: ori doubles as the normal, SURVEY A-11).
 * c_chamfer / c_knn: d loss / d (mean_i |x_i - ori_nn(i)|^2) / N and d loss / d (KNNDist term) / (N k) of the sample, fp32
 * constants prepared by the host (functor weights, the reference's `* K`, the batch mean, the shard ratio).
 * c_knn == 0 or k == 0: no kNN term (plain ChamferDist; knn_d / knn_idx may be NULL); c_chamfer == 0: nn_idx may be NULL.
 * N <= PC3D_KNN_ATTACK_UPDATE_MAX_POINTS: a sample's cloud, accumulators, values and masked list live in LDS, 32 bytes a
 * point + 8 KiB of staged edges (136 KiB of the CU's 160 at the cap); 0 <= k <= 63, k + 1 <= N. */
#define PC3D_KNN_ATTACK_UPDATE_MAX_POINTS 4096
int pc3d_knn_attack_update_f32(float* adv, int64_t a_bs, int64_t a_ps, int64_t a_cs,
                               const float* ori, int64_t o_bs, int64_t o_ps, int64_t o_cs,
                               const float* normal, int64_t n_bs, int64_t n_ps, int64_t n_cs,
                               const float* g, int64_t g_bs, int64_t g_ps, int64_t g_cs, float* m, float* v,
                               int B, int N, int k, const float* knn_d, const int32_t* knn_idx,
                               const int32_t* nn_idx, double lr, double beta1, double beta2, double eps,
                               float budget, int clip_mode, float alpha, float c_chamfer, float c_knn,
                               const int32_t* step_dev, int step_host, void* stream);
/* pc3d_knn_attack_update_f32 on a batch of clouds of different sizes: sample b counts L = lengths[b] points (int32 [B] on
 * the device, read as data, clamped to [1, N]) and has its own constants c_chamfer[b] / c_knn[b] (float32 [B] on the
 * device: what a run of that cloud alone prepares from its own point count); its kNN term exists when k >= 1 and
 * c_knn[b] != 0. N is the capacity: the stride of knn_d / knn_idx ([B,N,k+1]) and nn_idx ([B,N]) and the size of the LDS
 * arrays (N <= PC3D_KNN_ATTACK_UPDATE_MAX_POINTS). Every loop over points, the outlier statistics' / L and / (L - 1) and
 * the index clamps [0, L-1] run over L with the dense kernel's thread-to-point mapping and summation order: rows < L of
 * adv / m / v have the bits of the dense launch at N = L on that cloud alone, and with all lengths = N and equal constants
 * every output equals pc3d_knn_attack_update_f32's. Rows >= L of adv, g, knn_d, knn_idx, nn_idx and normal are never read
 * (they may hold NaN), their m / v are not written, and adv's take the NEW point 0: the padding the victim's passes and
 * the adv -> ori search of the loop rely on. knn_d / knn_idx: from pc3d_knn_ragged_f32 on the same lengths.
 * PRECONDITION L >= k + 1 where the kNN term exists (the caller's to check; indices are clamped either way). nn_idx must
 * not be NULL. */
int pc3d_knn_attack_update_ragged_f32(float* adv, int64_t a_bs, int64_t a_ps, int64_t a_cs,
                                      const float* ori, int64_t o_bs, int64_t o_ps, int64_t o_cs,
                                      const float* normal, int64_t n_bs, int64_t n_ps, int64_t n_cs,
                                      const float* g, int64_t g_bs, int64_t g_ps, int64_t g_cs, float* m, float* v,
                                      int B, int N, int k, const int32_t* lengths, const float* knn_d,
                                      const int32_t* knn_idx, const int32_t* nn_idx, double lr, double beta1,
                                      double beta2, double eps, float budget, int clip_mode, float alpha,
                                      const float* c_chamfer, const float* c_knn, const int32_t* step_dev,
                                      int step_host, void* stream);

/* The additional-experiments CW (attack/additional_exp/CW_attack.py) around ONE stacked victim pass per iteration. Every
 * point tensor is a contiguous [B,3,K]; K <= PC3D_EOT_MAX_POINTS, 0 <= E <= PC3D_EOT_MAX_VIEWS views.
 * pc3d_eot_prepare_f32 writes the victim input X [(1+E) B,3,K], slot-major (row s B + b), one workgroup per (slot, cloud):
 *   slot 0 = adv[b]; slot e >= 1 = rot[t,e-1] ori[b] + (adv[b] - ori[b]) with rot [T,E,3,3] row-major (bmm's product, summed
 *   left to right) at table row t = step mod T (*step_dev, or step_host), the rotation shared by the batch;
 *   renorm != 0: every slot is centred on its mean and divided by its largest point norm (both reductions in a fixed order;
 *   the LOWEST index wins a tie); stats [(1+E) B,4] = centroid, scale and arg [(1+E) B] = the arg-max are written either way
 *   (0, 0, 0, 1 and 0 without renorm);
 *   idx [T,E,K] int32 (NULL: none): column j of slot e >= 1 is column idx[t,e-1,j] mod K of that slot's cloud (K of the 2K
 *   columns of cat((x, x), 2)); slot 0 is never resampled.
 * pc3d_eot_update_f32 does the rest of the iteration, one workgroup per cloud, without float atomics (a cloud's bits depend
 * on neither the batch nor the launch); the step number t' >= 1 (*step_dev, or step_host) is the one Adam uses and the
 * tables are read at row (t' - 1) mod T, the row the prepare launch read before the victim's tail advanced the word:
 *   record   dist = w[b] d(adv, ori): dist_kind 2 Chamfer adv -> ori, the mean over i of |adv_i - ori[nn_idx[i]]|^2 (direct
 *            form; nn_idx [B,K] from pc3d_nn_f32, clamped), 1 L2 (Frobenius norm), 0 none; the decisions of the CW loops
 *            (strict <, a NaN distance updates nothing) on pred[b] (slot 0's prediction) and goal[b] into bestdist /
 *            bestscore / o_bestdist / o_bestscore [B]; o_bestattack[b] = adv[b] when it becomes the overall best;
 *            input_val = adv and dist_val[b] = dist (either may be NULL); g_out [B,3,K] (may be NULL) receives the total
 *            gradient Adam consumes;
 *   gradient of the adversarial term: for e = 1 .. E ascending, gx[e B + b] (the stacked pass's input gradient; with E > 0
 *            slot 0's rows are ignored, with E == 0 they are the gradient) gathered through inv [T,E,K,2] int32 (NULL: no
 *            resampling): the at most two columns that drew point i, or -1; then with renorm != 0 through the
 *            renormalisation on the stored stats / arg: g_q = g_y / s, ds = -sum(g_y . q) / s^2 added to the arg-max point
 *            along q / |q|, g_p = g_q - mean g_q (fixed summation order); the views are summed into the iterate's gradient;
 *   gradient of the distance term: Chamfer 2 w[b] / (batch_mean K) (adv_i - ori[nn_idx[i]]); L2 w[b] / batch_mean
 *            (adv - ori) / |adv - ori|_F (no guard at zero, as torch); batch_mean: the size of the batch of the loss mean;
 *   Adam     torch's (pc3d_adam_clip_step_f32's arithmetic) on the sum; one_d != 0: x and y are copied from ori and z is
 *            clamped to ori_z +- box. adv, m, v are updated in place.
 * The update keeps the cloud's gradient accumulators in LDS, 12 bytes a point (96 KiB at the cap); the sums of the
 * renormalisation's backward are accumulated in double. */
#define PC3D_EOT_MAX_POINTS 8192
#define PC3D_EOT_MAX_VIEWS 16
int pc3d_eot_prepare_f32(const float* adv, const float* ori, int B, int K, int E, int T, const float* rot,
                         const int32_t* idx, int renorm, const int32_t* step_dev, int step_host, float* X,
                         float* stats, int32_t* arg, void* stream);
int pc3d_eot_update_f32(float* adv, const float* ori, const float* gx, float* m, float* v, int B, int K, int E, int T,
                        const float* rot, const int32_t* inv, int renorm, const float* stats, const int32_t* arg,
                        const int64_t* pred, const int64_t* goal, int untarget, float* bestdist, int64_t* bestscore,
                        float* o_bestdist, int64_t* o_bestscore, float* o_bestattack, float* input_val,
                        float* dist_val, float* g_out, int dist_kind, const float* w, const int32_t* nn_idx,
                        int batch_mean,
                        double lr, double beta1, double beta2, double eps, int one_d, float box,
                        const int32_t* step_dev, int step_host, void* stream);

/* The loop's per-iteration tables drawn on the device instead of by the host generators (opt-in; NOT draw-for-draw
 * comparable with the reference's torch.randn / random.random / random.sample streams). Fills the rows row0 .. row0 + cnt - 1
 * of rot [T,E,3,3], idx [T,E,K] and inv [T,E,K,2] (idx and inv NULL together: rot only) for the draw indices
 * n = n0 + row - row0; no other row is touched. 0 <= row0, row0 + cnt <= T, 1 <= E <= PC3D_EOT_MAX_VIEWS,
 * 1 <= K <= PC3D_EOT_MAX_POINTS, n0 >= 0; cnt == 0 is a no-op. One workgroup per (row, view), no atomics.
 * The draw of (seed, n, e), e = 0 .. E - 1, is a pure function; all integer arithmetic is mod 2^64:
 *   mix64(z): z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB; z ^ (z >> 31)
 *             (the splitmix64 finaliser);  G = 0x9E3779B97F4A7C15;
 *   s   = mix64((uint64)seed + G * (16 * n + e + 1));
 *   u_j = mix64(s ^ (1 << (32 + j))) for j = 0, 1, 2 (the column keys below hash s ^ c with c < 2^14: no shared input);
 *   rotation, in double:  theta = 1e-2 * sqrt(-2 ln(((u_0 >> 11) + 1) * 2^-53)) * cos(2 pi ((u_1 >> 11) * 2^-53));
 *             c = cos(theta), s_ = sin(theta), each rounded to float32;  r = (u_2 >> 11) * 2^-53, compared in double:
 *             r < 0.2: [[c,s_,0],[-s_,c,0],[0,0,1]];  r < 0.4: [[1,0,0],[0,c,s_],[0,-s_,c]];
 *             r < 0.6: [[c,0,s_],[0,1,0],[-s_,0,c]];  else the identity (the 0 and 1 entries are exact) — the matrices
 *             of the reference's draw (:195-218): theta ~ 1e-2 N(0,1), the cases with probability 0.2 / 0.2 / 0.2 / 0.4;
 *   resampling: for every column c = 1 .. 2K - 1, key(c) = (mix64(s ^ c) & ~0x3FFF) | c — distinct, so their order is
 *             total; idx[j] = the c of the j-th smallest key, j < K: K columns of range(1, 2K) without replacement in
 *             random order (random.sample(range(1, 2K), K)'s distribution), ONE draw per (n, e) shared by the batch;
 *             inv[i] = the at most two positions j, ascending, with idx[j] mod K == i, else -1.
 * The keys are sorted in LDS, 8 bytes a slot over 2^p >= 2K slots (128 KiB at the cap). */
int pc3d_eot_draw_f32(int64_t seed, int64_t n0, int row0, int cnt, int T, int E, int K, float* rot, int32_t* idx,
                      int32_t* inv, void* stream);

/* The three launches for clouds of different sizes in one batch: the dense kernel bodies instantiated a second time, with
 * lengths [B] int32 (device data, must not be NULL; each value is clamped to [1, K]) behind the sizes. K is the capacity: the
 * row stride of every tensor, the bound of the cap and of the LDS checks. Cloud b counts L = lengths[b] points; every walk,
 * divisor (the centroid, both means, the Chamfer term) and index bound (nn_idx, arg, idx, inv) is L, in the dense launch's
 * thread-to-point mapping and summation order, so the rows < L of every output carry the bits of the dense entry run on
 * that cloud alone at K = L, and with every length = K the dense launch's bits. No row >= L of adv, ori, gx, m, v is read.
 *   pc3d_eot_prepare_ragged_f32: idx is [T,E,B,K], a table per cloud, column j < L of slot e >= 1 is column
 *     idx[t,e-1,b,j] mod L; the columns j >= L of EVERY slot of X are written as copies of that slot's output column 0, so a
 *     victim that does not know the lengths sees a valid padded cloud.
 *   pc3d_eot_update_ragged_f32: inv is [T,E,B,K,2]; rows >= L of m, v (and g_out) are left alone; rows >= L of adv take the
 *     NEW row 0, rows >= L of input_val and (where the overall best is copied) of o_bestattack the row 0 they copy: all
 *     three leave the launch as padded clouds.
 *   pc3d_eot_draw_ragged_f32: rot stays [T,E,3,3], shared by the batch; idx [T,E,B,K] and inv [T,E,B,K,2]; one workgroup per
 *     (row, view, cloud). Cloud b's table is pc3d_eot_draw_f32's of (seed, n, e) at K = L, entry for entry: the keys of the
 *     columns 1 .. 2L - 1 — the cloud index is not part of a key, so two clouds of one length share their draws, as the
 *     whole batch does in the dense loop — and since the keys are distinct and the pads sort last, the table is a pure
 *     function of (seed, n, e, L) whatever sort size or thread count the launch takes from the capacity K. The entries
 *     j >= L are CHOSEN as idx = the cloud's idx[.., 0] (a valid column, should a reader ignore the length) and inv = -1
 *     (no column draws a row that does not exist); no kernel reads them. */
int pc3d_eot_prepare_ragged_f32(const float* adv, const float* ori, int B, int K, const int32_t* lengths, int E, int T,
                                const float* rot, const int32_t* idx, int renorm, const int32_t* step_dev, int step_host,
                                float* X, float* stats, int32_t* arg, void* stream);
int pc3d_eot_update_ragged_f32(float* adv, const float* ori, const float* gx, float* m, float* v, int B, int K,
                               const int32_t* lengths, int E, int T, const float* rot, const int32_t* inv, int renorm,
                               const float* stats, const int32_t* arg, const int64_t* pred, const int64_t* goal, int untarget,
                               float* bestdist, int64_t* bestscore, float* o_bestdist, int64_t* o_bestscore,
                               float* o_bestattack, float* input_val, float* dist_val, float* g_out, int dist_kind,
                               const float* w, const int32_t* nn_idx, int batch_mean, double lr, double beta1, double beta2,
                               double eps, int one_d, float box, const int32_t* step_dev, int step_host, void* stream);
int pc3d_eot_draw_ragged_f32(int64_t seed, int64_t n0, int row0, int cnt, int T, int E, int B, int K, const int32_t* lengths,
                             float* rot, int32_t* idx, int32_t* inv, void* stream);

/* GeoA3's iteration after the victim's passes and the searches (attack/GeoA3/GeoA3_attack.py:139-181, :321-351, lp_clip
 * :92-102) as ONE launch, one workgroup per cloud; every point tensor is a contiguous [B,3,N]. In this order:
 *   record   pc3d_geoa3_record_f32's decisions on pred[b] (the loss launch's prediction), target[b], constrain[b] as it
 *            ARRIVES (the previous iteration's value; the caller puts 1e10 there before step 0) and the iterate x as it
 *            stands; the step and search step written to best_step / best_bs are step[b] and *search_step;
 *   terms    on the arg-mins nn_ao [B,N] (adv -> ori), nn_oa [B,N] (ori -> adv; NULL: single-sided Chamfer) and the self-kNN
 *            lists knn_idx [B,N,k+1] (self first; NULL, k == 0 or w_curv == 0: no curvature term), squared distances
 *            recomputed in the direct form: dis = mean_i d_ao (+ mean_j d_oa), or with dis_kind 1 the L2 sum over the
 *            points (nn_ao then only serves the curvature term and may be NULL without one; w_hd must be 0);
 *            hd = max_i d_ao, first index on ties; curv = mean_i (kappa_i - kappa_ori[nn_ao[i]])^2 with pc3d_kappa_f32's
 *            arithmetic on the normals normal_ori[:, nn_ao[i]]; constrain = (w_dis dis + w_hd hd) + w_curv curv goes back
 *            into constrain[b], loss_n = cls[b] + scale[b] constrain into loss_rows[step[b], b] (skipped past max_steps);
 *   gradient of gval scale[b] constrain w.r.t. x, added to g (the victim's gradient, already scaled); every sum into a
 *            point runs in a fixed order (own side in list order, then the incoming terms ascending by source): the bits
 *            depend on neither the batch nor the launch; no float atomics;
 *   update   Adam (pc3d_adam_clip_step_f32's arithmetic, bias corrections from step[b] + 1, lr[b]) on offset; step[b] += 1;
 *            scheduler != 0: lr[b] *= 0.9990; cc_linf != 0: lp_clip; x = ori + offset.
 * terms_out [5,B] (dis, hd, curv, constrain, loss_n), hd_arg_out [B] and g_out [B,3,N] (the total gradient) may be NULL.
 * Indices outside [0,N) are clamped. N <= PC3D_GEOA3_UPDATE_MAX_POINTS and 38 N + 2 N k + 512 bytes of LDS <= 160 KiB:
 * the cloud, the gathered normals and a reverse index of the N k curvature edges live in LDS (140.5 KiB at N = 2048,
 * k = 16). */
#define PC3D_GEOA3_UPDATE_MAX_POINTS 2048
int pc3d_geoa3_update_f32(float* x, const float* ori, float* offset, const float* g, float* m, float* v, int B, int N,
                          int k, const int32_t* nn_ao, const int32_t* nn_oa, const int32_t* knn_idx,
                          const float* normal_ori, const float* kappa_ori, const float* cls, const float* scale,
                          const int64_t* pred, const int64_t* target, int targeted, int dis_kind, float gval, float w_dis,
                          float w_hd, float w_curv, float* constrain, float* loss_rows, int max_steps, int32_t* step,
                          const int32_t* search_step, double* lr, int scheduler, float* best_loss, float* best_attack,
                          int64_t* best_bs, int64_t* best_step, float* iter_best_loss, int64_t* iter_best_score,
                          double beta1, double beta2, double eps, float cc_linf, float* terms_out, int32_t* hd_arg_out,
                          float* g_out, void* stream);

/* pc3d_geoa3_update_f32 on a batch of clouds of different sizes: cloud b counts L = lengths[b] points (int32 [B] on the
 * device, read as data, clamped to [1, N]; must not be NULL). N stays the capacity — the row stride of every [B,3,N], [B,N]
 * and [B,N,k+1] buffer and the size the LDS request and every check above are computed from. Every loop over points, every
 * mean's divisor, the Hausdorff maximum, both reverse indices and every index clamp range over L with the dense launch's
 * thread-to-point mapping and summation order: rows < L of every output, the cloud's words and its loss_rows column have
 * the bits of pc3d_geoa3_update_f32 at N = L on that cloud alone. Rows >= L of x, g, m, v, offset, nn_ao, nn_oa, knn_idx,
 * normal_ori, kappa_ori and ori are never loaded (they may hold NaN or any integer); those of m, v, offset and g_out are
 * not written; x's take the NEW row 0 (the padding the victim's passes and the next searches rely on: an exact copy of
 * row 0 loses every tie to index 0), and a record copies the iterate with its rows >= L set to its row 0 into best_attack.
 * Precondition: k + 1 <= lengths[b] with a curvature term (the searches that fill knn_idx need as many points); whatever
 * the buffers hold, the clamps keep every access inside them. */
int pc3d_geoa3_update_ragged_f32(float* x, const float* ori, float* offset, const float* g, float* m, float* v, int B, int N,
                                 int k, const int32_t* nn_ao, const int32_t* nn_oa, const int32_t* knn_idx,
                                 const float* normal_ori, const float* kappa_ori, const float* cls, const float* scale,
                                 const int64_t* pred, const int64_t* target, int targeted, int dis_kind, float gval,
                                 float w_dis, float w_hd, float w_curv, float* constrain, float* loss_rows, int max_steps,
                                 int32_t* step, const int32_t* search_step, double* lr, int scheduler, float* best_loss,
                                 float* best_attack, int64_t* best_bs, int64_t* best_step, float* iter_best_loss,
                                 int64_t* iter_best_score, double beta1, double beta2, double eps, float cc_linf,
                                 float* terms_out, int32_t* hd_arg_out, float* g_out, const int32_t* lengths, void* stream);

/* The point-adding attacks' iteration (attack/Gen3DAdv CWAdd / CWAddClusters) as ONE launch, one workgroup per sample:
 * the set distance adv -> ori from the search output (nn_d / nn_idx [B,A], pc3d_nn_f32), bookkeeping on it, total
 * gradient (g, the victim's gradient on the A added columns, + w[b] * d distance / d adv) and Adam without clip, written
 * back through adv's strides. kind: 1 Chamfer adv2ori (mean), 2 Hausdorff adv2ori (max), 3 FarChamfer (farthest
 * intra-cluster pair over A/P clusters of P points + cd_w * Chamfer). o_bestattack / input_val / m / v are contiguous
 * [B,3,A]; input_val / dist_val may be NULL. 1 <= A <= 2048, 1 <= P <= 64 with A % P == 0. The step number is READ
 * from *step_dev (or step_host). */
int pc3d_add_update_f32(float* adv, int64_t a_bs, int64_t a_ps, int64_t a_cs,
                        const float* ori, int64_t o_bs, int64_t o_ps, int64_t o_cs, int B, int A, int K,
                        const float* nn_d, const int32_t* nn_idx, const int64_t* pred, const int64_t* label,
                        int untarget, float* bestdist, int64_t* bestscore, float* o_bestdist, int64_t* o_bestscore,
                        float* o_bestattack, float* input_val, float* dist_val,
                        const float* g, int64_t g_bs, int64_t g_ps, int64_t g_cs, float* m, float* v,
                        double lr, double beta1, double beta2, double eps, const int32_t* step_dev, int step_host,
                        int kind, const float* w, float cd_w, int P, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Point-dropping defences in front of a victim (attack/SIadv/baselines/defense/drop_points/SOR.py, SRS.py).
 * ------------------------------------------------------------------------------------------------------- */
/* Statistical outlier removal (SOR.py:24-76) after the search, ONE launch, one workgroup per cloud. dists [B,K,k1]: the
 * k1 = k + 1 ascending squared distances of the self-kNN search (pc3d_knn_f32 on q == r: column 0 is the point itself).
 * v[b,i] = mean of columns 1 .. k; thr[b] = mean_i v + alpha * std_i v (unbiased), both in fp64 with a fixed summation
 * order; the points with v <= thr are kept in ascending index order, count[b] = n_b of them; rank [B,K] = position among
 * the kept or -1; src [B,npoint] = kept_b[j mod n_b] (the reference's repeat-then-top-up padding); out [B,npoint]
 * (element strides) = the points of x at src. v [B,K] / thr [B] (fp32 copies) may be NULL. 2 <= k1 <= K <= npoint,
 * K <= 8192. A cloud whose v are all NaN keeps nothing: count 0, src -1, out NaN. */
int pc3d_sor_select_f32(const float* dists, const float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs, int B, int K, int k1,
                        double alpha, int npoint, float* v, float* thr, int32_t* count, int32_t* rank, int32_t* src,
                        float* out, int64_t o_bs, int64_t o_ps, int64_t o_cs, void* stream);
/* Search and selection in one launch: the cloud in LDS, every point scans it with the search's arithmetic (the same
 * distance bits as pc3d_knn_f32). dists [B,K,k1] is written (and must be given). k1 <= 9, K <= 4096. One workgroup per
 * cloud: B of the chip's 256 compute units work, where the two-launch form's search fills all of them. */
int pc3d_sor_fused_f32(const float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs, int B, int K, int k1, double alpha, int npoint,
                       float* dists, float* v, float* thr, int32_t* count, int32_t* rank, int32_t* src,
                       float* out, int64_t o_bs, int64_t o_ps, int64_t o_cs, void* stream);
/* Backward of the copies: grad[b,i,:] = sum over j = rank[b,i], rank + n_b, ... < npoint of g[b,j,:] in ascending j, zero
 * for dropped points. One thread per input point, no atomics: the same bits in every run and for every batch size. */
int pc3d_sor_bwd_f32(const float* g, int64_t g_bs, int64_t g_ps, int64_t g_cs, const int32_t* count, const int32_t* rank,
                     int B, int K, int npoint, float* grad, int64_t gr_bs, int64_t gr_ps, int64_t gr_cs, void* stream);
/* Simple random sampling drawn on the device (SRS.py:23-32 draws on the host with numpy): idx [B,M] = M distinct indices
 * of [0,K) per cloud, uniformly chosen and in random order — every point gets the key hash(seed, call, b, i), the M
 * smallest keys win (bitonic network in LDS), indices are emitted in key order. `call` is read from *counter (a device
 * word the caller advances with pc3d_i32_add, so replays of a captured graph draw new subsets) or, with counter NULL,
 * is counter_host. 1 <= M <= K <= 4096. */
int pc3d_srs_select_i32(int64_t seed, const int32_t* counter, int counter_host, int B, int K, int M, int32_t* idx,
                        void* stream);
/* out[b,j,:] = x[b,idx[b,j],:] for an index table idx [B,M] int32 (element strides on both sides); an index outside
 * [0,K) reads nothing and writes NaN. */
int pc3d_gather_points_f32(const float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs, const int32_t* idx, int B, int K, int M,
                           float* out, int64_t o_bs, int64_t o_ps, int64_t o_cs, void* stream);

/* -------------------------------------------------------------------------------------------------------
 * PU-Net, the upsampler of the DUP-Net defence (attack/SIadv/baselines/defense/DUP_Net/).
 * ------------------------------------------------------------------------------------------------------- */
/* 3-NN inverse-distance interpolation of a feature-propagation level (pu_modules.py:161-168) from the search's lists:
 * dists / idx [B,N,3] (pc3d_knn_f32 of the N unknown points among the M known ones), feats [B,M,ldf] channels-last.
 * out[b,n,c] = act(sum_j w_j feats[b,idx_j,c] + bias[c]), w_j = r_j / (r_0 + r_1 + r_2), r_j = 1 / (d_j + 1e-8); out is
 * [B,N,ldo] and points at the first of the C columns written (a column offset of a wider row buffer; any alignment).
 * bias [C] may be NULL; relu != 0 applies max(., 0). C % 4 == 0, ldf % 4 == 0, M >= 3. */
int pc3d_three_interp_f32(const float* dists, const int32_t* idx, const float* feats, int64_t ldf, int B, int N, int M, int C,
                          const float* bias, int relu, float* out, int64_t ldo, void* stream);
/* Backward to the known features AND to both coordinate sets (the reference differentiates through the distances):
 * g [B,N,ldg] upstream gradient (at the column offset), y [B,N,ldy] the forward's output there (its sign is the ReLU mask)
 * or NULL; u [B,N] / k [B,M] the unknown / known points (element strides). gu [B,N,3], gF [B,M,C], gk [B,M,3] are
 * contiguous and fully written. rev_off [B,M+1] / rev_lst [B,3N]: the sorted reverse index of idx (pc3d_rev_index_i32):
 * the scatter to the known rows is a gather through it in ascending order — no atomics, the same bits in every run and
 * for every batch size. wrec [B,N,3] and krec [B,N,3,3] are scratch. */
int pc3d_three_interp_bwd_f32(const float* u, int64_t u_bs, int64_t u_ps, int64_t u_cs, const float* k, int64_t k_bs,
                              int64_t k_ps, int64_t k_cs, const float* dists, const int32_t* idx, const float* feats, int64_t ldf,
                              const float* g, int64_t ldg, const float* y, int64_t ldy, const int32_t* rev_off,
                              const int32_t* rev_lst, int B, int N, int M, int C, float* wrec, float* krec, float* gu, float* gF,
                              float* gk, void* stream);
/* The coordinate head (pu_net.py:83-86,131) in one launch: out = W4 relu(W3 h + b3) + b4 with widths C2 = 128 -> C3 = 64
 * -> 3 on the fp32 MFMA. h [R*B*N, ldh] holds the R expansion branches one after the other (row (r*B + b)*N + n); out is
 * [B, R*N, 3] with branch r at rows r*N .. (the reference concatenates the branches along the point axis). mask
 * [R*B*N, 2] receives the sign bits of the 64 hidden channels of every row for the backward. */
int pc3d_pcd_tail_f32(const float* h, int64_t ldh, const float* w3, const float* b3, const float* w4, const float* b4, int B,
                      int N, int R, int C2, int C3, uint32_t* mask, float* out, void* stream);
/* gh [R*B*N, ldgh] = (mask * (g W4)) W3 for the upstream gradient g [B, R*N, 3]; w3t [128,64] is W3 transposed. */
int pc3d_pcd_tail_bwd_f32(const float* g, const uint32_t* mask, const float* w4, const float* w3t, int B, int N, int R, int C2,
                          int C3, float* gh, int64_t ldgh, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * The CW iteration (attack/CW/CW_attack.py:111-174) with its independent pieces carried by launches that exist anyway:
 * 15 launches per iteration instead of 17, still one chain. Every entry computes the bits of the launches it replaces.
 *
 * pc3d_linear_nn_f32: pc3d_linear_f32 (first 15 arguments) + pc3d_nn_f32 (q, r, NB clouds, N queries, M reference
 * points, min_d2 / idx) as ONE launch: the search's workgroups ride behind the layer's. ride = 0, or a shape outside
 * the rider's range (the layer not on the tiled kernel of pc3d_linear_f32, the search not on its 512-thread form or
 * M > 2048), runs the two existing launches instead: callers always make one call. tile: the layer's tile as
 * pc3d_linear_f32's; the layer's workgroups, however many the tile makes them, come first in dispatch order.
 * ------------------------------------------------------------------------------------------------------- */
int pc3d_linear_nn_f32(const float* X, int ldx, int P, int B, int K, const float* W, const float* bias, int O,
                       int relu, float slope, const float* gate, int ldg, float gate_slope, float* Y, int ldy,
                       const float* q, int64_t q_bs, int64_t q_ps, int64_t q_cs,
                       const float* r, int64_t r_bs, int64_t r_ps, int64_t r_cs,
                       int NB, int N, int M, float* min_d2, int32_t* idx, int ride, int tile, void* stream);
/* pc3d_linear_f32 + the bookkeeping half of pc3d_cw_update_f32 (||adv-ori|| into dist_val, best-distance decisions,
 * the input_val / o_bestattack copies; same reduction tree, same bits) for NB samples of NK <= 8192 points, as NB extra
 * workgroups of the layer's launch. adam [2] (may be NULL) receives Adam's {lr / (1 - beta1^t), sqrt(1 - beta2^t)} for
 * the value t of the device step word step_dev. ride = 0 or a layer outside the tiled kernel: two launches (the layer
 * then as pc3d_linear_f32 with the same tile). tile: a form by name as pc3d_linear_f32's; 0 is PC3D_LIN_TILE_32X16 in
 * the one launch — it lasts as long as the bookkeeping workgroups behind the layer's, and no smaller tile measured
 * faster there. */
int pc3d_linear_book_f32(const float* X, int ldx, int P, int B, int K, const float* W, const float* bias, int O,
                         int relu, float slope, const float* gate, int ldg, float gate_slope, float* Y, int ldy,
                         const float* adv, int64_t a_bs, int64_t a_ps, int64_t a_cs,
                         const float* ori, int64_t o_bs, int64_t o_ps, int64_t o_cs, int NB, int NK,
                         const int64_t* pred, const int64_t* label, int untarget,
                         float* bestdist, int64_t* bestscore, float* o_bestdist, int64_t* o_bestscore,
                         float* o_bestattack, float* input_val, float* dist_val,
                         double lr, double beta1, double beta2, const int32_t* step_dev, float* adam,
                         int ride, int tile, void* stream);
/* pc3d_pointmlp3_max_bwd_f32 in accumulate form (T = NULL, no dL/dT) whose epilogue applies the update half of
 * pc3d_cw_update_f32 to the tower's input x (= the iterate adv, updated IN PLACE together with m / v, which share its
 * strides) instead of storing grad_x + this tower's gradient: distance gradient (dist_kind 0 / 1 / 2 as
 * pc3d_cw_step_f32; dist_val = ||adv-ori|| per sample for kind 1, nn_idx for kind 2), Adam with the factors adam [2] of
 * pc3d_linear_book_f32, ClipPointsLinf (budget > 0). grad_x is only read.
 * form: PC3D_PM_BWD_DEFAULT, or PC3D_PM_BWD_PACKED / PC3D_PM_BWD_TILE32 by name (the same bits; parity test and bench
 * tool only); the two-list kernel has no update epilogue: PC3D_PM_BWD_TWOLIST is PC3D_EINVAL here. */
int pc3d_pointmlp3_max_bwd_update_f32(float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs, int B, int N,
                                      const float* W1, const float* b1, const float* W2, const float* b2,
                                      const float* W3, const float* W2T, int C1, int C2, int C3,
                                      const int32_t* argidx, const uint64_t* mask1, const uint32_t* mask2,
                                      const float* g_pooled, const float* grad_x, int64_t gx_bs, int64_t gx_ps,
                                      int64_t gx_cs, const float* ori, int64_t o_bs, int64_t o_ps, int64_t o_cs,
                                      float* m, float* v, double beta1, double beta2, double eps, float budget,
                                      const float* adam, int dist_kind, const float* w, const float* dist_val,
                                      const int32_t* nn_idx, int form, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * The isometry attack (attack/ISO/iso_attack.py): x' = W x with one 3x3 matrix per cloud, in front of a frozen victim.
 * W is row-major [., 9]; point tensors are B clouds (or B * R for the per-matrix ones) of N points with element strides.
 * ------------------------------------------------------------------------------------------------------- */
/* out[b R + r, :, n] = W[b R + r] x[b, :, n] for R >= 1 matrices per cloud (ISOnet's nn.Linear(3, 3, bias=False),
 * iso_attack.py:96-100); transpose != 0 applies W^T instead, the input-gradient direction of the same op. x [B clouds] is
 * read once for its R matrices; out [B * R clouds] must not alias it. B <= 65535. */
int pc3d_iso_apply_f32(const float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs, const float* W, int B, int R, int N,
                       int transpose, float* out, int64_t o_bs, int64_t o_ps, int64_t o_cs, void* stream);
/* gW[i, a, c] = sum_n g[i, a, n] * x[i / R, c, n] for the B * R matrices (g: B * R clouds, x: B clouds, gW [B * R, 9]).
 * One workgroup per matrix and one summation order that depends on neither B nor R; no float atomics. */
int pc3d_iso_wgrad_f32(const float* g, int64_t g_bs, int64_t g_ps, int64_t g_cs,
                       const float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs, int B, int R, int N, float* gW,
                       void* stream);
/* Everything of one CTRI step (gradient_attack, iso_attack.py:127-153) that is not the victim, per cloud, one launch:
 *   latch   a cloud that is not done and has pred[b] != label[b] becomes done (the reference's `break`);
 *   record  while the cloud was not done ON ENTRY: steps[b] += 1, kept_out[b] = row[b] (this evaluation's [ncls] output
 *           row, row stride row_ld), kept_pred[b] = pred[b];
 *   update  a cloud that is still not done takes one torch.optim.Adam step (weight_decay 0, amsgrad off) on W[b] with
 *           the gradient gW[b] = g[b] x[b]^T — pc3d_iso_wgrad_f32's reduction, the same bits — or with gW_in[b] when
 *           g is NULL (exactly one of g, gW_in is given). m, v [B,9]. The step number t of the Adam step is the
 *           cloud's own device word: the value steps[b] has just taken, so a replayed launch needs no host counter;
 *   next    xo[b] = W[b] x[b] for every cloud (a done cloud rewrites the same values). xo aliases neither x nor g.
 * done, steps: int32 [B], zero before the first step. A done cloud's W, m, v, steps and kept_* never change again. */
int pc3d_iso_update_f32(const float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs,
                        const float* g, int64_t g_bs, int64_t g_ps, int64_t g_cs, const float* gW_in,
                        int B, int N, const int64_t* pred, const int64_t* label, const float* row, int64_t row_ld,
                        int ncls, int32_t* done, int32_t* steps, float* kept_out, int64_t* kept_pred,
                        float* W, float* m, float* v, double lr, double beta1, double beta2, double eps,
                        float* xo, int64_t xo_bs, int64_t xo_ps, int64_t xo_cs, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * The shape-invariant white-box attack (attack/SIadv/SIadv_attack.py, shape_invariant_ifgm): I-FGM in every point's
 * tangent frame, with the normals re-estimated on the device every step (csrc/siadv.hip).
 * ------------------------------------------------------------------------------------------------------- */
/* out[b, i] = the unit eigenvector of the smallest eigenvalue of the covariance of the K points idx[b, i, :] of cloud b
 * about their own mean (the point itself is among them: idx comes from a self-kNN search, self first). This is what
 * the reference asks of open3d's estimate_normals(KDTreeSearchParamKNN(knn=K)). Mean, covariance and the closed-form
 * 3 x 3 solve (shared with pc3d_estimate_normal_f32) in double.
 *   sign         free in the method; here the last non-zero of (x, y, z) is positive. No sign fix against the
 *                neighbours as in pc3d_estimate_normal_f32: the attack step does not depend on the sign.
 *   degenerate   K < 3, a zero covariance deviator or a zero cross product give (0, 0, 1).
 *   bad index    an entry outside [0, N) is never dereferenced; that point's normal is NaN.
 * out must not alias x. B <= 65535. */
int pc3d_pca_normal_f32(const float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs, const int32_t* idx, int B, int N,
                        int K, float* out, int64_t o_bs, int64_t o_ps, int64_t o_cs, void* stream);
/* xe = U^T (U (x + t)) - t per point, with U = get_spin_axis_matrix(n) and t = (x . n) n: the cloud the reference hands to
 * the victim in every step (SIadv_attack.py:293-298). It is x up to rounding except at the rows of U that are rewritten
 * for |n_z^2 - 1| < 1e-4, where U is not the frame of n and the point moves by up to ~1e-4 |x|; the gradient of
 * pc3d_si_step_f32 is the victim's at xe. Normals given (nrm) or from idx as pc3d_pca_normal_f32 computes them (exactly one
 * of the two); nrm_out (may be NULL) receives them. xe and nrm_out alias nothing else. B <= 65535. */
int pc3d_si_frame_f32(const float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs,
                      const float* nrm, int64_t n_bs, int64_t n_ps, int64_t n_cs,
                      const int32_t* idx, int K, int B, int N,
                      float* xe, int64_t e_bs, int64_t e_ps, int64_t e_cs,
                      float* nrm_out, int64_t no_bs, int64_t no_ps, int64_t no_cs, void* stream);
/* One I-FGM step of shape_invariant_ifgm (SIadv_attack.py:293-320) for B clouds of N points, IN PLACE on x, one launch,
 * one workgroup per cloud. g = dL/dxe of the victim at pc3d_si_frame_f32's xe. The normals are either given (nrm, idx NULL) or computed in
 * the prologue from the neighbour lists idx [B,N,K] exactly as pc3d_pca_normal_f32 computes them (nrm NULL). Per point,
 * the reference's arithmetic as written:
 *   U        get_spin_axis_matrix(n), the rows for |n_z^2 - 1| < 1e-4 chosen before anything divides by sqrt(1 - n_z^2);
 *   t        (P . n) n;         P' = U (P + t);         g' = U g with g'_z = 0;
 *   P'      -= step_size * sqrt(3 * 1024) * g' / (sqrt(sum over the cloud of g'^2) + 1e-9);
 *   P        = U^T P' - t, then P - ori clamped to [-eps, eps] per coordinate (NaN stays NaN).
 * The cloud's sum runs in one fixed order that depends on neither B nor N's split over a grid; no float atomics.
 * nrm_out (may be NULL) receives the normals used; in idx mode with N > 5120 it is required (the normals pass through
 * it instead of LDS). x must not alias any other argument. A NaN normal (bad index) makes its whole cloud NaN. */
int pc3d_si_step_f32(float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs,
                     const float* ori, int64_t o_bs, int64_t o_ps, int64_t o_cs,
                     const float* g, int64_t g_bs, int64_t g_ps, int64_t g_cs,
                     const float* nrm, int64_t n_bs, int64_t n_ps, int64_t n_cs,
                     const int32_t* idx, int K, int B, int N,
                     float* nrm_out, int64_t no_bs, int64_t no_ps, int64_t no_cs,
                     double step_size, double eps, void* stream);
/* The three entries above on a batch of clouds of different sizes: cloud b counts L = clamp(lengths[b], 1, N) points
 * (lengths int32 [B] on the device, read by the kernel as data, never NULL) and N is the capacity, the row stride of every
 * buffer. The kernels are the second instantiations of the dense bodies; the argument checks, the aliasing rules and the
 * limits are the dense entries' (the LDS stage of pc3d_si_step_ragged_f32 is decided by N, not by L, and its step keeps
 * sqrt(3 * 1024) whatever L is). The contract of all three: rows < L have the bits of the dense entry on that cloud alone
 * at N = L, and the rows >= L of every output are copies of the output's row 0.
 *   pc3d_pca_normal_ragged_f32   a neighbour index is checked against L (an entry >= L is never dereferenced: NaN for
 *                                that point). Rows >= L of x and idx are never read.
 *   pc3d_si_frame_ragged_f32     rows >= L of xe and of nrm_out (when given) repeat row 0's arithmetic, so they equal row 0
 *                                in every bit: what a victim whose pooling ignores copies of a point must be shown. Rows
 *                                >= L of x, nrm and idx are never read.
 *   pc3d_si_step_ragged_f32      the cloud's sum of g'^2 runs over n < L in the dense order; rows >= L of x receive the NEW
 *                                row 0 and rows >= L of nrm_out row 0's normal, in the same launch (handed over through
 *                                LDS: row 0 is rewritten in place). Rows >= L of ori, g, nrm and idx are never read. */
int pc3d_pca_normal_ragged_f32(const float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs, const int32_t* idx, int B, int N,
                               int K, const int32_t* lengths, float* out, int64_t o_bs, int64_t o_ps, int64_t o_cs,
                               void* stream);
int pc3d_si_frame_ragged_f32(const float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs,
                             const float* nrm, int64_t n_bs, int64_t n_ps, int64_t n_cs,
                             const int32_t* idx, int K, int B, int N, const int32_t* lengths,
                             float* xe, int64_t e_bs, int64_t e_ps, int64_t e_cs,
                             float* nrm_out, int64_t no_bs, int64_t no_ps, int64_t no_cs, void* stream);
int pc3d_si_step_ragged_f32(float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs,
                            const float* ori, int64_t o_bs, int64_t o_ps, int64_t o_cs,
                            const float* g, int64_t g_bs, int64_t g_ps, int64_t g_cs,
                            const float* nrm, int64_t n_bs, int64_t n_ps, int64_t n_cs,
                            const int32_t* idx, int K, int B, int N, const int32_t* lengths,
                            float* nrm_out, int64_t no_bs, int64_t no_ps, int64_t no_cs,
                            double step_size, double eps, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * SI-Adv's query attacks (simba_attack, simbapp_attack, shape_invariant_query_attack, SIadv_attack.py:343-624) as one
 * batched loop: per step one victim forward of the 2B candidate clouds and one launch of pc3d_query_step_f32.
 * ------------------------------------------------------------------------------------------------------- */
/* Decides entry pos[b] of every cloud's table from logp [2B,k] (the victim's log-probabilities for cand: rows 2b and
 * 2b + 1 are the two tries of cloud b) and writes the two candidate clouds of the next entry into cand [2B,.]. One
 * workgroup per cloud, fixed order, no atomics. Per cloud that is not done:
 *   loss_t  = max(other - real, -999) with real = logp[label] and other the largest (top = 1) or fifth largest (top = 5)
 *             entry of the row after the label's entry is replaced by -10000 (CWLoss, kappa = -999, tar = True);
 *   try 0 is accepted when loss_0 > best (strict), otherwise try 1 when loss_1 > best; queries += 1 or 2;
 *   accepted: the one-entry change goes into the state st, best = the loss, adv_target = the row's arg-max (lowest index
 *             on a tie); last_try / last_logp = the last try evaluated and its row;
 *   pos += 1; done = !(best < 0 && pos < L).
 * Coordinate mode (ori, nrm, dir NULL): st is the cloud, table entry e in [0, 3N) stands for coordinate e % 3 of point
 * e / 3, candidate t = st with eps_t added there. Frame mode: st is P' = U (ori + t), entry e in [0, N) is a point,
 * candidate t = U^T (P' + eps_t * dir[b, e] at that point) - t for the WHOLE cloud, U and t = (ori . n) n from nrm as
 * pc3d_si_step_f32 forms them. eps_t of entry l of cloud b is eps[b * eps_bs + l * eps_ls + t] (strides 0: two constants).
 * A cloud that is done changes nothing and gets unperturbed candidates. init != 0: nothing is decided (logp may be NULL);
 * the candidates of entry pos[b] are written, and in frame mode st = P' of ori first. last (may be NULL) receives, when
 * the cloud latches, the last candidate cloud evaluated. acc_trace [B,L] / loss_trace [B,L,2] (may be NULL) receive the
 * accepted try (-1: neither) and both losses of every entry decided. A table entry, a position or a label out of range
 * is never used as an index: the cloud is latched done with adv_target = -2. k <= 256. */
int pc3d_query_step_f32(const float* logp, int k, const int64_t* label, int top,
                        float* st, int64_t s_bs, int64_t s_ps, int64_t s_cs,
                        const float* ori, int64_t o_bs, int64_t o_ps, int64_t o_cs,
                        const float* nrm, int64_t n_bs, int64_t n_ps, int64_t n_cs,
                        const int32_t* tab, int L, const float* dir, const float* eps, int64_t eps_bs, int64_t eps_ls,
                        int32_t* pos, float* best, int32_t* done, int32_t* queries, int32_t* adv_target,
                        int32_t* last_try, float* last_logp,
                        float* cand, int64_t c_bs, int64_t c_ps, int64_t c_cs,
                        float* last, int64_t l_bs, int64_t l_ps, int64_t l_cs,
                        int32_t* acc_trace, float* loss_trace, int B, int N, int init, void* stream);
/* The sensitivity map of shape_invariant_query_attack (:553-563), one launch: per point g' = U g (g = the surrogate's
 * gradient at the cloud pc3d_si_frame_f32 shows it, U from nrm) with g'_z = 0 -> gp [B,N,3] (may be NULL), the ranking
 * key = sqrt(g'_x^2 + g'_y^2) [B,N], dir = g' / (key + 1e-16) [B,N,3] (a zero gradient gives zeros), and order [B,N]: the
 * points by (key descending, index ascending), which is Python's stable sorted(..., reverse=True). In-LDS bitonic
 * network over the next power of two; N <= 8192. */
int pc3d_si_rank_f32(const float* g, int64_t g_bs, int64_t g_ps, int64_t g_cs,
                     const float* nrm, int64_t n_bs, int64_t n_ps, int64_t n_cs, int B, int N,
                     float* gp, float* key, float* dir, int32_t* order, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * The critical-point attack (attack/CTA/CTA.py, CTA_sumloss.py): integrated-gradients saliency of a set of clouds and
 * the optimiser loop on its most salient points (csrc/cta.hip). No atomics; every sum has one order.
 * ------------------------------------------------------------------------------------------------------- */
/* IntegratedGradients.get_mask's step clouds, one launch: base = the minimum (kind 0, 'black') or maximum (kind 1,
 * 'white') over ALL B*3*N coordinates of x, or 0 (kind 2); out[s*B + b] = base + (float)alpha[s] * (x[b] - base), the
 * product rounded to float once and then added, as torch evaluates baseline + alpha * image_diff for a double scalar
 * alpha. alpha: S doubles in device memory (np.linspace(0, 1, S)). out [S*B,3,N] contiguous; base [1] receives base. */
int pc3d_ig_steps_f32(const float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs, int B, int N, int kind,
                      const double* alpha, int S, float* out, float* base, void* stream);
/* The cotangent of VanillaGradient.get_mask taken back from the log-softmax output to the logits z [R,k] (row r = step *
 * B + sample, R a multiple of B): g = t - softmax(z) * sum(t) with t one-hot at `target` (target >= 0) or, target < 0,
 * the multi-hot of the top-1 classes (lowest class on a tie) of ALL B rows of the step; rows of samples >= set_size are
 * zero. k <= 256. */
int pc3d_ig_cotangent_f32(const float* z, int R, int B, int k, int set_size, int target, float* g, void* stream);
/* mask[c,n,b] = (sum over s = 0..S-1, in that order, of (double)g[s*B + b, c, n]) * (double)(x[b,c,n] - base) / S, the
 * float64 [3,N,B] array IntegratedGradients.get_mask returns (g [S*B,3,N] contiguous: the victim's input gradients of
 * pc3d_ig_steps_f32's clouds; base: its base word). Also both contribution tables: contri_cn [3,B] = the mask summed over
 * the points in ascending order (CTA.py), contri_bn [B,N] = (m[0] + m[1]) + m[2] per point (CTA_sumloss.py). */
int pc3d_ig_reduce_f64(const float* g, int S, int B, int N, const float* x, int64_t x_bs, int64_t x_ps, int64_t x_cs,
                       const float* base, double* mask, double* contri_cn, double* contri_bn, void* stream);
/* The loop's loss as a cotangent on the logits z [G*S,k] of G sets of S clouds: row (g, j) gets w[j] times
 *   mode 0: e[ori] - e[tar]     mode 1: e[ori] - e[second], second = torch.topk(z, 2).indices[-1] (value descending,
 *   class ascending)            mode 2: e[ori]     mode 3: e[ori] - softmax(z)   (the gradient of log_softmax(z)[ori]).
 * In the same launch, for sample 0 of every set that is not latched, at position cur_step of the set: hist_ori = z[ori],
 * hist_max = the row's maximum with z[ori] NEGATED ([G,H] each; nothing is stored beyond H), the 25-entry windows of
 * z[ori] and z[tar] in poll, and the success flag (targeted: arg-max == tar, else arg-max != ori; lowest class on a
 * tie). poll [G,64] int32: 0..24 / 25..49 the windows (float bits), 50 latch, 51 cur_step, 52 step, 53 num_p_per,
 * 54 success flag. A latched set gets a zero cotangent. zlast [G*S,k] (may be NULL) receives the
 * rows of every set that is not latched: the logits of its last forward. k <= 256. */
int pc3d_cta_cotangent_f32(const float* z, int G, int S, int k, int mode, int targeted, const int32_t* ori,
                           const int32_t* tar, const float* w, int32_t* poll, float* hist_ori, float* hist_max, int H,
                           float* g, float* zlast, void* stream);
/* One optimiser step of every live set, in place on x [G*S,3,N] (contiguous, as g, proto, v, s): the gradient is kept at
 * the slots (sample * N + point) listed in levels 0 .. min(num_p_per, cap, P) - 1 of the set's table sel [G,P,W] and
 * zeroed elsewhere (entries outside [0, S*N) are padding), then for ALL coordinates of the set
 *   opt 0:  v = b1 v + (1 - b1) g;  s = b2 s + (1 - b2) g^2;  x += -v / sqrt(s + xi)   (no bias correction, step 1)
 *   opt 1:  v = b1 v - g;           x += v
 * cur_step += 1, step += 1, and latch = 1 when the step's success flag is set. control != 0: no step; a set with
 * ctrl[g] == 1 gets x = proto, num_p_per += 1, cur_step = 0 (the optimiser state stays), with ctrl[g] == 2 latch = 2;
 * ctrl[g] is cleared. Latched sets are untouched in both modes. S*N <= 49152. */
int pc3d_cta_update_f32(float* x, const float* g, const float* proto, float* v, float* s, const int32_t* sel, int P,
                        int W, int cap, int32_t* poll, int32_t* ctrl, int G, int S, int N, int opt, int control,
                        double b1, double b2, double xi, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PC3D_H */
