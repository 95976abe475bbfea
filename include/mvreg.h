/*
 * mvreg — MI355X-native pairwise registration hot path of LMPCR
 * (zgojcic/3D_multiview_reg).  C ABI of libmvreg_hip.so.
 *
 * Conventions (every entry point):
 *   - returns 0 (MVR_OK) or a negative error code; never throws across the ABI;
 *   - all pointers are DEVICE pointers allocated by the caller (no hidden
 *     allocation); workspaces are sized by the paired *_workspace_bytes() query;
 *   - calls are stream-ordered on `stream` (a hipStream_t; 0 = legacy default),
 *     re-entrant, and thread-safe across distinct streams/devices;
 *   - strides are in ELEMENTS;
 *   - empty work: when the count that sizes an array is 0 (no rows, pairs, points or fragments), the entry point
 *     returns MVR_OK after validating its scalar arguments and never reads the pointers of the empty arrays, which
 *     may be NULL (a zero-element torch tensor's data_ptr() is 0).  Outputs whose size does not depend on that
 *     count (per-fragment counts, offsets, hash tables that are cleared) are still written, so their pointers stay
 *     required.
 *
 * Process-wide settings: exactly two entry points, mvr_set_math (operand arithmetic) and mvr_debug_force (tests:
 * fallback paths), write process-global values of the library, read by the host side of each later call when it
 * builds its launches.  They are not per stream, per thread or per call.  Set them once, before any thread issues
 * work: two threads selecting different settings race, and a change never affects launches already enqueued.  The
 * defaults are the fp32-equivalent paths the parity tests pin; the Python mirror sets the arithmetic only through
 * lib._native.set_math, before the first forward.
 *
 * Each entry point names the reference interface it replaces
 * (paths relative to the reference repo).
 */
#ifndef MVREG_H
#define MVREG_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* mvr_stream_t; /* == hipStream_t */

#define MVR_OK 0
#define MVR_EINVAL -1
#define MVR_ELAUNCH -2

/* ------------------------------------------------------------------------
 * Weighted Procrustes / Kabsch.
 * Replaces lib/utils.py:164-237 kabsch_transformation_estimation (+ residuals
 * lib/utils.py:240-256), and — when guard_pos != NULL — the batch-coupled
 * zero-weight guard of lib/filtering/oanet.py:177-178 (if any pair q has
 * guard_pos[q]==0, every pair's weights get +1/N; w and w_copy are rewritten).
 * guard_group > 0 evaluates the guard per group of that many consecutive pairs (the reference
 * evaluation batch of 32 when a batch is split across ranks); 0 = the whole batch.
 *   x1(p,n,:) = x1[p*x_pstride + n*x_nstride + 0..2], x2 likewise.
 *   w may be NULL (all ones).  R [P,3,3] row-major, t [P,3], res [P, res_pstride],
 *   status[P]: 0 ok, 1 non-finite covariance (reference's SVD-exception branch:
 *   R=I, t=0).  res/res_copy/w_copy/status may be NULL.
 * ---------------------------------------------------------------------- */
int mvr_procrustes(const float* x1, const float* x2, int64_t x_pstride, int64_t x_nstride, float* w,
                   int64_t w_pstride, const int32_t* guard_pos, float* w_copy, int64_t wc_pstride, int P, int N,
                   int normalize, float eps, float* R, float* t, float* res, int64_t res_pstride, float* res_copy,
                   int64_t rc_pstride, int32_t* status, int guard_group, mvr_stream_t stream);
/* fp64 variant (fp64 inputs compute in fp64 in the reference, utils.py:164).  In both variants the covariance is
 * accumulated in fp64 about the pair's first point (x1[p,0], x2[p,0]), not about the origin, so clouds far from
 * the origin keep their digits: for 257 points of spread 1 at distance 1e4, R of mvr_procrustes_f64 was measured
 * within 6.1e-16 of a two-pass long-double Kabsch on an MI355X (4.7e-9 with the moments about the origin); t
 * follows R as mu2 - R mu1.  mvr_procrustes: R within 3e-8 of the same reference on the fp32-rounded inputs at
 * distance 1e3, the rounding of R itself.  The first point serves as origin whatever its weight, so it must be
 * representative of the cloud: a zero-weight first point far from the others (padding, an outlier at 1e6) costs
 * the digits that its distance from the cloud has. */
int mvr_procrustes_f64(const double* x1, const double* x2, int64_t x_pstride, int64_t x_nstride, double* w,
                       int64_t w_pstride, const int32_t* guard_pos, double* w_copy, int64_t wc_pstride, int P, int N,
                       int normalize, double eps, double* R, double* t, double* res, int64_t res_pstride,
                       double* res_copy, int64_t rc_pstride, int32_t* status, int guard_group,
                       mvr_stream_t stream);

/* ------------------------------------------------------------------------
 * RANSAC over given correspondences, batched over pairs.
 * Replaces lib/utils.py:671-709 run_ransac (Open3D 0.9
 * registration_ransac_based_on_correspondence, point-to-point estimation without
 * scaling, ransac_n = 4, max distance 0.05, RANSACConvergenceCriteria(50000, 2500):
 * 2500 iterations) as called at scripts/benchmark_pairwise_registration.py:100,212.
 *   x1(p,i,:) = x1[p*x_pstride + 3i + 0..2] (fp64), x2 likewise; n[p] correspondences of pair p.
 *   Outputs: T [P,4,4] row-major (x2 ~ T x1; identity when no hypothesis has an inlier or
 *   n[p] < ransac_n), fitness [P], rmse [P], best_iter [P] (-1: none).
 *   Draw j of iteration i for pair p: splitmix64(seed + ((p<<40)|(i<<8)|j) * 0x9E3779B97F4A7C15) % n[p]
 *   (Open3D draws std::rand() % n from a clock seed).  hyp_out [P,iters,12] (R row-major, t) may be
 *   NULL; workspace >= mvr_ransac_workspace_bytes(P, iters).
 * ---------------------------------------------------------------------- */
size_t mvr_ransac_workspace_bytes(int P, int iters);
int mvr_ransac(const double* x1, const double* x2, int64_t x_pstride, const int32_t* n, int P, int ransac_n,
               int iters, double max_dist, uint64_t seed, double* T, double* fitness, double* rmse,
               int32_t* best_iter, double* hyp_out, void* workspace, size_t workspace_bytes, mvr_stream_t stream);

/* ------------------------------------------------------------------------
 * RANSAC with correspondence checkers and a validation cap, batched over pairs (csrc/ransac.hip;
 * DESIGN.md 4.26).  What Open3D's global-registration examples configure (3-point samples,
 * CorrespondenceCheckerBasedOnEdgeLength(0.9) + ...BasedOnDistance, ...BasedOnNormal, 100000 iterations): a cheap
 * test per sample decides whether its hypothesis is scored at all.  It replaces nothing in the reference (whose
 * Open3D 0.9 call passes no checkers: mvr_ransac above, which stays as it is).
 *   x1, x2, x_pstride, n, P, ransac_n (3..8), iters, max_dist, seed and the draws: as mvr_ransac.
 *   Iteration `it` of pair p PASSES when, in this order,
 *     1. edge_sim > 0: no correspondence is drawn twice;
 *     2. edge_sim > 0: every pair j < k of its draws has ls2 >= sim2 * lt2 and lt2 >= sim2 * ls2, with
 *        ls2 = (d0*d0 + d1*d1) + d2*d2 of the two source points, lt2 of the two target points and
 *        sim2 = edge_sim * edge_sim (rounded fp64 operations, no fma, no square root);
 *     3. the Umeyama fit of its draws, as mvr_ransac computes it;
 *     4. check_dist > 0: every drawn correspondence has |R s + t - d|^2 < check_dist^2 (the evaluation's own
 *        operation order);
 *     5. nrm1 and nrm2 both given: every drawn correspondence has (R n1) . n2 >= normal_cos, each sum left to right.
 *   edge_sim in [0, 1) (0: checks 1-2 off), check_dist >= 0 (0: off), normal_cos in [-1, 1]; nrm1 / nrm2 fp64 in
 *   the layout of x1 / x2 (unit normals of the source / target points), either NULL: check 5 off.
 *   The first max_validation passing iterations, in ascending iteration order, are the validated hypotheses: each
 *   is scored over all n[p] correspondences as in mvr_ransac, and the result is the best by (inliers descending,
 *   rmse ascending, iteration ascending).  With every checker off and max_validation >= iters, T, fitness, rmse
 *   and best_iter equal mvr_ransac's bit for bit.  Nothing depends on scheduling: two runs give the same bytes.
 *   There is no confidence-based early exit (Open3D >= 0.12 stops once the best fitness makes further draws
 *   unlikely to improve): when to stop would depend on each pair's running best, which a batched launch of all
 *   iterations does not have.
 *   Outputs: T [P,4,4], fitness [P], rmse [P] (identity, 0, 0 when n[p] < ransac_n, nothing passes, or no validated
 *   hypothesis has an inlier), best_iter [P] (the iteration id; -1: none), n_pass [P] (iterations that pass),
 *   n_valid [P] = min(n_pass, max_validation).  Optional (NULL: not exported): pass_bits [P][ceil(iters/64)] uint64
 *   (bit it % 64 of word it / 64), valid_iter [P][max_validation] int32 (the validated iterations, -1 beyond
 *   n_valid[p]), hyp_out [P][max_validation][12] (R row-major, t of the validated hypotheses; rows beyond
 *   n_valid[p] are not written).
 *   workspace (8-byte aligned) >= mvr_ransac_checked_workspace_bytes(P, iters, max_validation): per pair the pass
 *   bits and, per validated hypothesis, the iteration id, a count, an error sum and 12 doubles.
 *   MVR_EINVAL: P < 0 or >= 2^23, ransac_n outside 3..8, iters outside (0, 2^30), max_validation < 1, max_dist not
 *   positive and finite, a non-finite or out-of-range edge_sim / check_dist / normal_cos, P * ceil(iters/256)
 *   >= 2^31, a short workspace and, with P > 0, a NULL x1, x2, n, T, fitness, rmse, best_iter, n_pass, n_valid or
 *   workspace.
 * ---------------------------------------------------------------------- */
size_t mvr_ransac_checked_workspace_bytes(int P, int iters, int max_validation);
int mvr_ransac_checked(const double* x1, const double* x2, int64_t x_pstride, const int32_t* n, int P, int ransac_n,
                       int iters, double max_dist, uint64_t seed, int max_validation, double edge_sim,
                       double check_dist, const double* nrm1, const double* nrm2, double normal_cos, double* T,
                       double* fitness, double* rmse, int32_t* best_iter, int32_t* n_pass, int32_t* n_valid,
                       uint64_t* pass_bits, int32_t* valid_iter, double* hyp_out, void* workspace,
                       size_t workspace_bytes, mvr_stream_t stream);

/* ------------------------------------------------------------------------
 * Fast Global Registration over given correspondences, batched over pairs (csrc/fgr.hip).
 * Zhou, Park, Koltun, ECCV 2016: what Open3D offers as registration_fgr_based_on_feature_matching, restated from the
 * maths (Open3D bit parity is not a goal).  It replaces nothing in the reference.  No hypotheses are sampled: a
 * Geman-McClure cost over the correspondences is minimised by Gauss-Newton steps while its scale shrinks.
 *   x1, x2, x_pstride, n, P and the draws: as mvr_ransac (x2 ~ T x1, n[p] valid rows of pair p);
 *   n_max = x_pstride / 3 bounds every n[p].  All geometry is fp64.  Pair p, in four steps:
 *   A. Tuple filter (tuple_factor > 0).  Test it = 0 .. tuple_factor * n[p] - 1 draws three rows, draw j being
 *      splitmix64(seed + ((p<<40)|(it<<8)|j) * 0x9E3779B97F4A7C15) % n[p].  It passes when the rows are distinct and
 *      every pair of them has ls2 >= s2 * lt2 and lt2 >= s2 * ls2 (check 2 of mvr_ransac_checked with
 *      s2 = tuple_scale * tuple_scale: rounded fp64 operations, no fma, so the set of passing tests is exact).  The
 *      first max_tuples passing tests in ascending `it` give the used rows: three per tuple in draw order, repeats
 *      across tuples kept.  n_tuples[p] of them, n_used[p] = 3 n_tuples[p].  tuple_factor == 0: the used rows are all
 *      n[p] rows, n_tuples[p] = 0, n_used[p] = n[p].
 *   B. Normalisation over all n[p] rows: mu1, mu2 the means of x1, x2, scale the largest |x1_i - mu1|, |x2_i - mu2|,
 *      p = (x1 - mu1) / scale, q = (x2 - mu2) / scale, delta = max_dist / scale.
 *   C. From R = I, t = 0, mu = 1, for k = 0 .. iters - 1: if k % 4 == 0 and mu > delta^2, mu <- mu / division_factor
 *      (not clamped); over the used rows p' = R p + t, e = p' - q, w = (mu / (|e|^2 + mu))^2; H = sum w J^T J,
 *      g = sum w J^T e with J = [-[p']x | I]; xi = -H^-1 g by Cholesky, a pivot not above 1e-12 of the largest
 *      diagonal entry ends the loop with status bit 8 and T kept; T <- D T, D = [Rz(xi2) Ry(xi1) Rx(xi0) | xi[3:6]].
 *   D. T [P,4,4] row-major = [R | scale t + mu2 - R mu1]; fitness [P], rmse [P] over all n[p] rows at max_dist as
 *      mvr_ransac scores a hypothesis (d2 < max_dist^2, inliers / n[p], sqrt(sum d2 / inliers), 0 without inliers).
 *      iters == 0 gives the loop's start in the clouds' units, R = I and t = mu2 - mu1 (the centroids aligned, not the
 *      4 x 4 identity), scored the same way; status 0.
 *   trace (NULL: not exported) [P,iters,2]: row k holds the mu of iteration k and the mean of w |e|^2 over the used
 *   rows at the T the iteration started from; the rows after the iteration that ended the loop early hold -1.
 *   status [P], the bits of lib/icp.py: 1 few (n[p] < 3, fewer than 3 used rows, scale 0), 4 invalid (a coordinate
 *   among the n[p] rows is not finite, or n[p] outside [0, n_max]), 8 degenerate (step C).  A pair with bit 1 or 4
 *   gets T = identity, fitness = rmse = 0, n_used = n_tuples = 0 and a trace of -1.
 *   One workgroup per pair, one launch, no atomics, every sum in a fixed order: two runs give the same bytes.
 *   workspace (8-byte aligned) >= mvr_fgr_workspace_bytes(P, n_max, max_tuples): max(n_max, 3 max_tuples) rows of 6
 *   doubles per pair.
 *   MVR_EINVAL: P < 0 or >= 2^23, iters < 0, max_dist not positive and finite, division_factor not finite or <= 1,
 *   tuple_factor < 0, tuple_scale outside (0, 1] with tuple_factor > 0, max_tuples < 1, x_pstride < 0,
 *   tuple_factor * n_max >= 2^31, a short workspace and, with P > 0, a NULL x1, x2, n, T, fitness, rmse, n_used,
 *   n_tuples, status or workspace.
 * ---------------------------------------------------------------------- */
size_t mvr_fgr_workspace_bytes(int P, int n_max, int max_tuples);
int mvr_fgr(const double* x1, const double* x2, int64_t x_pstride, const int32_t* n, int P, double max_dist,
            int iters, double division_factor, int tuple_factor, int max_tuples, double tuple_scale, uint64_t seed,
            double* T, double* fitness, double* rmse, int32_t* n_used, int32_t* n_tuples, int32_t* status,
            double* trace, void* workspace, size_t workspace_bytes, mvr_stream_t stream);

/* ------------------------------------------------------------------------
 * Multiview pose synchronisation, batched over scenes (csrc/sync.hip).
 * The closed-form weighted solve of the paper's sections 3.2-3.3 with optional IRLS; the reference never released
 * this stage (its README.md:116), so it replaces nothing: it turns the pairwise estimates of a scene into one pose
 * per fragment.
 *   Edge e of scene s is row s*e_sstride + e of R_pair [.,9] (row-major), t_pair [.,3], ij [.,2], w [.] (NULL: all
 *   ones): x_j ~ R x_i + t with source i = ij[.,0], target j = ij[.,1] (lib.utils.pair_index order), w >= 0; any
 *   i != j in either order, repeated edges allowed.  n_edges [S], n_frags [S] are device arrays
 *   (<= max_edges, <= max_frags).  Fragment f of scene s is row s*f_sstride + f of R [.,9], t [.,3], member [.].
 *   Poses: X = R_f x_f + t_f in the frame of fragment `anchor` (R = I, t = 0 there).  member[f] = 1 for the
 *   fragments connected to the anchor over edges with w > 0; the others come out as R = I, t = 0, member = 0 and
 *   their edges with weight 0.  irls_iters re-weighting passes w <- w0 / (1 + (e/c_rot)^2) / (1 + (d/c_trans)^2)
 *   with e = |R_k - R_j^T R_i|_F and d = |t_i - t_j - R_j t_k|_2; w_out, res_rot, res_trans [., same rows as w]
 *   are the last pass's weights and residuals.  member, w_out, res_rot, res_trans may be NULL.
 *   status [S], bits: 1 some fragment is not a member; 2 the eigen-solve of some pass stopped at its iteration
 *   cap; 4 an edge was ignored (index out of range, i == j, a non-finite value or a negative weight; it comes out
 *   with weight and residuals 0), or the scene is invalid (anchor >= n_frags[s], a count negative or above its
 *   maximum): the whole scene comes out as identity, member = 0.
 *   fp64 throughout; one workgroup per scene, every pass inside the one launch.  max_frags <= MVR_SYNC_MAX_FRAGS;
 *   workspace (8-byte aligned) >= mvr_sync_workspace_bytes(S, max_frags, max_edges).  MVR_EINVAL for negative
 *   S / max_frags / max_edges / irls_iters, max_frags above the maximum, anchor outside [0, max_frags) (when
 *   max_frags > 0), c_rot or c_trans <= 0 with irls_iters > 0, a short workspace, and with S > 0 a NULL n_edges,
 *   n_frags, status, R or t (max_frags > 0) or R_pair, t_pair or ij (max_edges > 0).
 * ---------------------------------------------------------------------- */
#define MVR_SYNC_MAX_FRAGS 128
size_t mvr_sync_workspace_bytes(int S, int max_frags, int max_edges);
int mvr_sync_poses(const double* R_pair, const double* t_pair, const int32_t* ij, const double* w, int64_t e_sstride,
                   const int32_t* n_edges, const int32_t* n_frags, int S, int max_frags, int max_edges, int anchor,
                   int irls_iters, double c_rot, double c_trans, double* R, double* t, int64_t f_sstride,
                   int32_t* member, double* w_out, double* res_rot, double* res_trans, int32_t* status,
                   void* workspace, size_t workspace_bytes, mvr_stream_t stream);

/* ------------------------------------------------------------------------
 * Process-wide selections (the only two; every other choice a launch makes is a function of its arguments).
 * mvr_set_math: the operand arithmetic of every kernel that has a choice.  0 (default) f32eq: every fp32 product on
 *   the three-term bf16 split (h + m + l, 6 MFMAs: fp32-equivalent operands).  1 split16: the two-term fp16 split
 *   (h + l, 3 MFMAs per product, 22-bit operands) in the generic GEMM, the point convs, diff_pool / the 4-wave
 *   diff_unpool, the sparse convs with > 64 output channels and the feature-NN distances, wherever the launch has a
 *   range flag: weight rows range-scaled, activations range-checked, and a guarded split-bf16 re-run of any launch
 *   whose operands left the fp16 window; split-bf16 directly where the output overwrites an input.  Returns the
 *   previous mode.
 * mvr_debug_force (tests): force one of the fallback paths the library keeps for shapes its fast kernels do not
 *   cover — 0 the feature NN's online softmax only, 1 point convs and OAFilter conv2 on the generic GEMM, 2 diff_pool
 *   / diff_unpool unfused (embedding GEMM + softmax + pooling GEMM), 3 the block's conv1 stored instead of folded
 *   into the first PointCN, 4 diff_pool without key splits, 5 the 8-wave diff_unpool at <= 512 clusters, 6 the
 *   OANet block's point activations row-major instead of chunk-major (bit-identical).  value 0 restores the
 *   default.  Returns the previous value (MVR_EINVAL for an unknown path).
 * ---------------------------------------------------------------------- */
int mvr_set_math(int mode);
int mvr_debug_force(int what, int value);

/* ------------------------------------------------------------------------
 * One fused MFMA batched GEMM of the OANet schedule (exposed for tests):
 *   C[b](m,n) = sum_k pro_A(A(m,k)) pro_B(B(k,n)) + bias + R[b](m,n)
 * pro: 0 none, 1 relu(A*sc[k]+sh[k]), 2 relu(B*sc[k]+sh[k]) (sc/sh at [b*sPb + k]),
 *      3 B(k,n) * f[b*sPb + (k/128)*pld + n] (per-tile softmax factor).
 * bias_mode: 0 none, 1 per m, 2 per n.  stats_mode: 0 none, 1 row sum/sumsq,
 * 2 row softmax (C <- exp(v - tile row max), partials (tile max, sum)), 3 the same per column,
 * 4 column sum/sumsq (float2 partials, see csrc/gemm.hpp).
 * Layout: 16-byte aligned pointers, all strides multiples of 4 floats, rows padded to
 * round_up(K|N, 4) floats holding finite values (MVR_EINVAL otherwise).
 * math: must be 1, the three-term bf16 split (x = h+m+l, products hh+hm+mh+mm+hl+lh on
 * v_mfma_f32_32x32x16_bf16, fp32 accumulation: fp32-level accuracy); other values return MVR_EINVAL (the exact
 * fp32-MFMA variant of round 2 was removed: 2.7x slower at the same accuracy class).
 * Replaces the nn.Conv2d(k=1) / torch.matmul calls of lib/filtering/oanet.py.
 * ---------------------------------------------------------------------- */
int mvr_gemm_f32(int M, int N, int K, int batch, const float* A, int64_t sAb, int64_t lda, const float* B,
                 int64_t sBb, int64_t ldb, int b_kcontig, float* C, int64_t sCb, int64_t ldc, const float* R,
                 int64_t sRb, const float* bias, int bias_mode, const float* psc, const float* psh, int64_t sPb,
                 int64_t pld, int pro, float* stats, int64_t st_ld, int st_off, int stats_mode, int math,
                 int32_t* range_flag, mvr_stream_t stream);
/* OAFilter conv2 (oanet.py:72-81: the 1x1 conv over the clusters on the transpose, W2 [K][K] shared by every pair):
 * C[b](m, n) = sum_k relu(A[b](m, k) psc[b*sPb + k] + psh[b*sPb + k]) W(n, k) + bias[n] + R[b](m, n), M = 128, row
 * statistics per 128-column tile as mvr_gemm_f32's stats_mode 1 (st_off 0), on the split-once kernel (gemm.hip
 * oaf_conv2_kernel: W split into an image once per launch, each A element folded and split once per workgroup,
 * 128 x 256 tiles).  img: >= mvr_oaf_conv2_image_bytes(N, K) bytes of 16-byte aligned device scratch, written by the
 * call.  Layout as mvr_gemm_f32; K % 4 == 0 and 32 < K <= 512.  MVR_EINVAL when the shape is not the kernel's
 * (mvr_oan_block_forward then runs the generic GEMM). */
int mvr_oaf_conv2_f32(int M, int N, int K, int batch, const float* A, int64_t sAb, int64_t lda, const float* W,
                      int64_t ldw, float* C, int64_t sCb, int64_t ldc, const float* R, int64_t sRb, const float* bias,
                      const float* psc, const float* psh, int64_t sPb, float* stats, int64_t st_ld, void* img,
                      int64_t img_bytes, mvr_stream_t stream);
size_t mvr_oaf_conv2_image_bytes(int N, int K);

/* ------------------------------------------------------------------------
 * OANet block (lib/filtering/oanet.py:132-185 OANBlock.forward) — parameters
 * are the reference module's tensors (conv weights [Cout][Cin] row-major =
 * the Conv2d weight with its 1x1 tail dropped).
 * ---------------------------------------------------------------------- */
typedef struct { const float* weight; const float* bias; } mvr_conv_p;
typedef struct { const float* gamma; const float* beta; const float* mean; const float* var; } mvr_bn_p;
typedef struct { mvr_bn_p bn1; mvr_conv_p conv3; mvr_bn_p bn5; mvr_conv_p conv7; mvr_conv_p shortcut; } mvr_pointcn_p;
typedef struct {
  mvr_bn_p bn1; mvr_conv_p conv1; /* conv1: IN(1e-3) BN ReLU Conv          (oanet.py:64-69) */
  mvr_bn_p bn2; mvr_conv_p conv2; /* conv2: BN(points) ReLU Conv(points)  (oanet.py:72-76) */
  mvr_bn_p bn3; mvr_conv_p conv3; /* conv3: IN(1e-3) BN ReLU Conv          (oanet.py:77-83) */
} mvr_oafilter_p;

#define MVR_OAN_MAX_HALF 8
typedef struct {
  int in_channels;  /* 6 (reg_init) or 8 (reg_iter) */
  int channels;     /* net_channel (128) */
  int clusters;     /* clusters (500) */
  int half_layers;  /* (net_depth / (iter_num+1)) / 2  (3) */
  mvr_conv_p conv1;
  mvr_pointcn_p l1_1[MVR_OAN_MAX_HALF];
  mvr_bn_p down_bn; mvr_conv_p down_conv;
  mvr_oafilter_p l2[MVR_OAN_MAX_HALF];
  mvr_bn_p up_bn; mvr_conv_p up_conv;
  mvr_pointcn_p l1_2[MVR_OAN_MAX_HALF]; /* l1_2[0] has a shortcut conv (2C -> C) */
  mvr_conv_p output;
} mvr_oan_block_p;

size_t mvr_oan_block_workspace_bytes(int channels, int clusters, int in_channels, int P, int N);

/* input(p,c,n) = input[p*in_pstride + c*ld + n]  (Cin = blk->in_channels); ld >= round_up(N, 4),
 * a multiple of 4, input 16-byte aligned, padding columns [N, ld) finite (zero).
 * xs(p,n,0..5) = xs[p*xs_pstride + n*xs_nstride + 0..5]  (x1 | x2 for Kabsch)
 * Outputs: logits/scores [P,N] (contiguous), R [P,3,3], t [P,3], res [P,N];
 * latent(p,c,n) = latent[p*C*ld + c*ld + n] (may be NULL); res_row/score_row: optional copies written at
 * row pointers with pair stride row_pstride (the next block's input rows 6,7).
 * guard_pos: int32 [P]: per-pair counts of positive weights (zeroed here).  status: int32 [P] (may be NULL).
 * guard_group: scope of the zero-row guard (see mvr_procrustes): 0 the whole batch, > 0 groups of that many
 * pairs; < 0 the block stops after its output head — scores hold relu(tanh(logits)) unguarded, guard_pos the
 * counts, and R, t, res, res_row, score_row are left to the caller's mvr_procrustes (a guard evaluated over
 * pairs on other devices: lib/distributed.py scene mode).
 * bn_train: 0 BatchNorm with running statistics (module.eval()); 1 batch statistics over all P pairs
 * (module.train(): the reference's forward batch); G > 1 batch statistics per group of G consecutive pairs (the
 * last group may be smaller) — G forwards of the reference's loader batches in one call (pair it with
 * guard_group = G). */
/* Diagnostics: how many split-bf16 re-runs of split-fp16 attention launches ran on the current device since
   the last reset (synchronises the device); -1 on error. */
int mvr_attn_reruns(int reset);
/* Debugging: while buf is non-NULL, every mvr_oan_block_forward launch sequence adds a position-weighted
 * 64-bit hash of each stage's activation to the next of cap device slots (zeroed by the caller);
 * NULL disables.  Not for concurrent use from two streams. */
int mvr_debug_stage_hash(unsigned long long* buf, int cap);
/* Debugging: copy the statistics partials hashed as stage `stage` into dst (bytes); NULL disables. */
int mvr_debug_stage_dump(int stage, void* dst, size_t bytes);
/* Diagnostics: the point-activation layout the latest mvr_oan_block_forward chose — 1 chunk-major (every 32-point
 * chunk of a pair one contiguous block), 0 row-major, -1 no forward yet (bench.py records it in its config). */
int mvr_oan_last_layout(void);
int mvr_oan_block_forward(const mvr_oan_block_p* blk, const float* input, int64_t in_pstride, int64_t ld,
                          const float* xs, int64_t xs_pstride, int64_t xs_nstride, int P, int N, int bn_train,
                          float* logits,
                          float* scores, float* R, float* t, float* res, float* latent, float* res_row,
                          float* score_row, int64_t row_pstride, int32_t* guard_pos, int32_t* status, int guard_group,
                          void* workspace,
                          size_t workspace_bytes, mvr_stream_t stream);

/* Fused diff_pool (lib/filtering/oanet.py:96-110), channels == 128, clusters <= 1024:
 *   x_down(p,c,j) = sum_n x(p,c,n) softmax_n(e(p,j,n)),  e = W . relu(x * sc + sh) + b
 * x(p,c,n) = x[p*x_pstride + c*x_ld + n] (x_ld >= round_up(N,4), multiple of 4, 16-byte aligned);
 * sc/sh(p,c) = sc[p*s_pstride + c] (the embedding conv's InstanceNorm+BatchNorm folded to an affine);
 * weight [clusters][128] (16-byte aligned), bias [clusters] (may be NULL);
 * out(p,c,j) = out[p*out_pstride + c*out_ld + j], out_ld >= round_up(clusters,4), columns [clusters,
 * round_up(clusters,4)) written 0.  stats (may be NULL): float pairs (sum, squared deviations from the
 * tile mean) of row c over the 128-column tile t at stats[2*((p*ceil(clusters/128) + t)*st_ld + st_off + c)].
 * The [clusters x N] embedding never leaves the chip (flash-style online softmax). */
int mvr_oan_diff_pool(const float* x, int64_t x_pstride, int64_t x_ld, const float* sc, const float* sh,
                      int64_t s_pstride, const float* weight, const float* bias, int P, int channels, int N,
                      int clusters, float* out, int64_t out_pstride, int64_t out_ld, float* stats, int64_t st_ld,
                      int st_off, mvr_stream_t stream);
/* The same with a workspace (mvr_oan_diff_pool_workspace_bytes(P, 128, clusters) bytes, 16-byte aligned):
 * when one workgroup per (pair, 256-cluster block) leaves the last dispatch round partly idle, the
 * points of each block are split over 2 or 4 workgroups whose partial (output, running max, sum) the
 * last one to finish merges.  Same results up to fp32 summation order. */
size_t mvr_oan_diff_pool_workspace_bytes(int P, int channels, int clusters);
int mvr_oan_diff_pool_ws(const float* x, int64_t x_pstride, int64_t x_ld, const float* sc, const float* sh,
                         int64_t s_pstride, const float* weight, const float* bias, int P, int channels, int N,
                         int clusters, float* out, int64_t out_pstride, int64_t out_ld, float* stats, int64_t st_ld,
                         int st_off, void* workspace, size_t workspace_bytes, mvr_stream_t stream);

/* Fused diff_unpool (lib/filtering/oanet.py:113-129), channels == 128, clusters <= 1024:
 *   out(p,c,n) = sum_j x_down(p,c,j) softmax_j(e(p,j,n)),  e = W . relu(x_up * sc + sh) + b
 * x_up as x above; x_down(p,c,j) = x_down[p*xd_pstride + c*xd_ld + j]; out like x (columns [N,
 * round_up(N,4)) written 0); stats per 128-column tile of N as above (ceil(N/128) tiles per pair).
 * workspace: mvr_oan_diff_unpool_workspace_bytes(P, 128, clusters) bytes, 16-byte aligned (the
 * split-bf16 images of W and x_down). */
size_t mvr_oan_diff_unpool_workspace_bytes(int P, int channels, int clusters);
int mvr_oan_diff_unpool(const float* x_up, int64_t x_pstride, int64_t x_ld, const float* sc, const float* sh,
                        int64_t s_pstride, const float* weight, const float* bias, const float* x_down,
                        int64_t xd_pstride, int64_t xd_ld, int P, int channels, int N, int clusters, float* out,
                        int64_t out_pstride, int64_t out_ld, float* stats, int64_t st_ld, int st_off,
                        void* workspace, size_t workspace_bytes, mvr_stream_t stream);

/* Correspondences [P][N][C] (strided) -> channel-major network input out[p*out_pstride + c*out_ld + n]
 * (the transpose of lib/filtering/oanet.py:234). */
int mvr_xs_to_channels(const float* xs, int64_t xs_pstride, int64_t xs_nstride, int C, int P, int N, float* out,
                       int64_t out_pstride, int64_t out_ld, mvr_stream_t stream);

/* ------------------------------------------------------------------------
 * Overlap gate (lib/utils.py:713-786 compute_overlap_ratio; benchmark:219-220).
 * Open3D VoxelDownSample restated: per fragment b (xyz float32 [n,3], frag_off [B+1] device int64),
 * voxel index floor((p - (min_b - v/2)) / v) in fp64, centroid = fp64 sum of the voxel's points in input
 * order / count.  out_xyz fp64 [n,3] capacity (voxels of a fragment contiguous, fragments in order),
 * out_off [B+1] (device).  B <= 4096.
 * Coordinate limit: a voxel index is kept in 16 bits per axis, so every fragment must satisfy
 * floor((max - min) / v + 0.5) <= 65535 along each axis, i.e. an extent below about 65535.5 v (1,638 m at
 * v = 0.025, 65.5 m at v = 0.001).  The index is relative to the fragment's own minimum, so where a fragment lies
 * does not matter.  A fragment beyond the limit is detected on the device without a synchronisation: the call still
 * returns MVR_OK and out_off[B] holds -1 instead of the voxel total; out_off[0..B-1] and out_xyz are then not
 * meaningful (nothing is written out of bounds).  lib.overlap.FragmentOverlap raises ValueError on it.
 * ---------------------------------------------------------------------- */
size_t mvr_voxel_centroids_workspace_bytes(int64_t n);
int mvr_voxel_centroids(const float* xyz, const int64_t* frag_off, int B, int64_t n, double voxel, void* workspace,
                        size_t workspace_bytes, double* out_xyz, int64_t* out_off, mvr_stream_t stream);
/* mvr_voxel_centroids with colours: colors float32 [n,3] in the row order of xyz, out_colors fp64 [n,3] capacity in
 * the row order of out_xyz: the fp64 mean of the voxel's colours, summed in input order (what Open3D's
 * voxel_down_sample does with colours).  The same passes: out_xyz and out_off are bit-identical to
 * mvr_voxel_centroids', and the workspace is mvr_voxel_centroids_workspace_bytes(n).  With n > 0 colors and
 * out_colors must not be NULL. */
int mvr_voxel_centroids_colored(const float* xyz, const int64_t* frag_off, int B, int64_t n, double voxel,
                                void* workspace, size_t workspace_bytes, const float* colors, double* out_xyz,
                                int64_t* out_off, double* out_colors, mvr_stream_t stream);
/* Radius index over fp64 points [M,3] in fragments off [B+1] (device): points sorted by (fragment, cell of
 * size r) + a hash of the occupied cells.  `index` holds mvr_radius_index_bytes(M) bytes and stays valid
 * for mvr_radius_overlap_count, mvr_icp_refine, mvr_estimate_normals, mvr_icp_refine_plane,
 * mvr_icp_refine_generalized, mvr_compute_fpfh, mvr_knn_self, mvr_radius_count, mvr_iss_saliency, mvr_radius_nms,
 * mvr_color_gradient, mvr_icp_refine_colored and mvr_cluster_dbscan calls on the same points.
 * B < 32768.
 * Cell keys: the cell coordinate floor(x / r) + 2^15 is kept modulo 2^16 per axis, so coordinates are NOT limited:
 * cells 65536 r apart along an axis (3,276.8 m at r = 0.05) share a key.  That aliasing is harmless: the aliased
 * cells of a fragment form one run of the sorted order under one hash entry, a query walks the whole run, and
 * every candidate still passes the fp64 distance test, so a far point is never matched and a near one never
 * missed; the cost is the longer run.  The fragment index is kept above the 48 coordinate bits and never aliases. */
size_t mvr_radius_index_bytes(int64_t M);
int mvr_radius_index_build(const double* xyz, const int64_t* off, int B, int64_t M, double r, void* index,
                           size_t bytes, mvr_stream_t stream);
/* counts[2p + d] = number of points q of fragment pairs[2p + d] whose image T[p][d] q (3x4 row-major fp64,
 * T [P][2][12]) lies at Euclidean distance < r from some point of fragment pairs[2p + 1 - d].
 * With trans the reference's argument: T[p][0] = inv(trans) (pc_i side), T[p][1] = trans (pc_j side).
 * max_points >= the largest fragment. */
int mvr_radius_overlap_count(const void* index, size_t bytes, const double* xyz, const int64_t* off, int B,
                             int64_t M, const int64_t* pairs, const double* T, int P, int64_t max_points, double r,
                             int32_t* counts, mvr_stream_t stream);

/* ------------------------------------------------------------------------
 * Point-to-point ICP refinement, batched over pairs, on a radius index (csrc/icp.hip).
 * The reference stops at the coarse estimate, so this replaces nothing of it: it is the fine registration that
 * Open3D's registration_icp (TransformationEstimationPointToPoint) does after the global estimate, restated from
 * the maths; Open3D parity is unpinned.
 *   index, xyz [M,3], off [B+1], r_index: the arguments of the mvr_radius_index_build call that made `index`.
 *   Pair p: source fragment pairs[2p], target fragment pairs[2p + 1], start T0[12p..] (3x4 row-major) with
 *   x_target ~ R x_source + t (the estimators' convention; the inverse of mvr_radius_overlap_count's trans).
 *   eval(T): every source point x maps to q = R x + t; its correspondence is the target point nearest to q (the
 *   lowest row on equal distances), valid iff sqrt(ex*ex + ey*ey + ez*ez) < max_dist (strict, the expression of the
 *   overlap gate).  n_corr = the valid ones, fitness = n_corr / n_source (0 for an empty source),
 *   rmse = sqrt(sum d^2 / n_corr) (0 without correspondences).
 *   Loop: state = eval(T0); up to max_iters times: stop with status bit 1 when n_corr < 3; T = the unweighted
 *   Kabsch solution over the valid pairs on the original source points (det-corrected; no composition of
 *   increments); new = eval(T); stop when |new.fitness - fitness| < tol_fitness and |new.rmse - rmse| < tol_rmse
 *   (absolute differences; the new state is kept).  max_iters solves without that, and a tolerance > 0: status
 *   bit 2 (also with max_iters == 0, a pure evaluation of T0: its cap of 0 solves is reached).  Both tolerances 0:
 *   exactly max_iters solves, bit 2 never set.
 *   Outputs per pair: T [P,12], fitness / rmse / n_corr of the returned T, iters = the solves done, status (bits:
 *   1 fewer than 3 correspondences at an evaluation the loop looked at; 2 the cap; 4 an invalid pair: a fragment
 *   index outside [0, B), offsets outside [0, M] or a non-finite T0 — then T = T0 copied bit for bit,
 *   fitness = rmse = 0, iters = n_corr = 0).  trace [P, max_iters + 1, 2]: (fitness, rmse) of every evaluation, -1
 *   in the rows after the last one.  n_corr, iters and trace may be NULL.
 *   fp64 throughout; one workgroup per pair, every iteration inside the one launch, no workspace; a pair's outputs
 *   are a function of the pair alone (bit-identical whatever the batch around it).
 *   MVR_EINVAL, scalars first: negative P, M or max_iters; B <= 0 or B >= 32768; M >= 2^31; max_dist or
 *   r_index <= 0; max_dist > r_index (the 27 cells around a query must cover its search ball); a negative
 *   tolerance.  P == 0 then returns MVR_OK.  With P > 0: a NULL pairs, T0, T, fitness, rmse or status; with M > 0 a
 *   NULL index, xyz or off, or index_bytes < mvr_radius_index_bytes(M).
 * ---------------------------------------------------------------------- */
int mvr_icp_refine(const void* index, size_t index_bytes, const double* xyz, const int64_t* off, int B, int64_t M,
                   double r_index, const int64_t* pairs, const double* T0, int P, double max_dist, int max_iters,
                   double tol_fitness, double tol_rmse, double* T, double* fitness, double* rmse, int32_t* n_corr,
                   int32_t* iters, int32_t* status, double* trace, mvr_stream_t stream);

/* ------------------------------------------------------------------------
 * Per-point normals on a radius index (csrc/normals.hip): Open3D's
 * estimate_normals(KDTreeSearchParamRadius(radius)) restated from the maths; Open3D parity is unpinned.
 *   index, xyz [M,3], off [B+1], r_index: the arguments of the mvr_radius_index_build call that made `index`.
 *   The neighbours of point i are the points of its own fragment with sqrt(ex*ex + ey*ey + ez*ez) < radius (strict,
 *   the expression of the overlap gate), e = x_j - x_i; the point itself is one of them.  n_nbr[i] = their number
 *   (n_nbr may be NULL).  Fewer than 3: the normal is (0, 0, 1).  Otherwise C = mean(e e^T) - mean(e) mean(e)^T over
 *   the neighbours and the normal is the unit eigenvector of C's smallest eigenvalue (cyclic symmetric Jacobi; on
 *   exactly equal eigenvalues the later axis of the decomposition).  A zero row and column of C keep their axis
 *   exactly: a fragment in the plane z = 0 gets exactly (0, 0, +-1).
 *   Sign: with viewpoints [B,3] (one per fragment, device) the normal of a point p of fragment b is flipped so that
 *   n . (v_b - p) >= 0.  With viewpoints == NULL the sign is whatever the eigen-solve leaves: unspecified, and it
 *   may differ between builds; mvr_icp_refine_plane does not depend on it.
 *   normals [M,3] and n_nbr [M] in the row order of xyz; every row is written.  fp64 throughout; one thread per point,
 *   no atomics, no workspace; a point's outputs are a function of its fragment alone.
 *   MVR_EINVAL, scalars first: negative M or M >= 2^31; B <= 0 or B >= 32768; radius or r_index <= 0;
 *   radius > r_index (the 27 cells around a point must cover its ball).  M == 0 then returns MVR_OK.  With M > 0: a
 *   NULL index, xyz, off or normals, or index_bytes < mvr_radius_index_bytes(M).
 * ---------------------------------------------------------------------- */
int mvr_estimate_normals(const void* index, size_t index_bytes, const double* xyz, const int64_t* off, int B,
                         int64_t M, double r_index, double radius, const double* viewpoints, double* normals,
                         int32_t* n_nbr, mvr_stream_t stream);

/* ------------------------------------------------------------------------
 * Point-to-plane ICP refinement, batched over pairs (csrc/icp_plane.hip): the loop of Open3D's
 * registration_icp with TransformationEstimationPointToPlane, restated from the maths; Open3D parity is unpinned.
 * The arguments are those of mvr_icp_refine plus normals [M,3] (the row order of xyz; unit length is the caller's
 * business, mvr_estimate_normals gives it; their sign does not matter: a and b below change sign together).
 *   eval(T), fitness, rmse, n_corr: exactly mvr_icp_refine's (Euclidean distances), so the two methods' figures
 *   compare.
 *   Loop: state = eval(T0); up to max_iters times: stop with status bit 1 when n_corr < 6.  Over the valid pairs
 *   q = T x, y its match, n the normal of y, c = the target fragment's first point (a per-pair origin: the cross
 *   products then have the size of the fragment, not of its distance from the world origin):
 *   a = [(q - c) x n, n], b = (q - y) . n; solve (sum a a^T) xi = -sum a b by Cholesky.  A pivot that fails
 *   pivot > 1e-12 max_i H_ii (a NaN fails it too) stops the loop with status bit 8, T kept, iters not counted.
 *   Otherwise D = [R_inc | xi[3:6] + c - R_inc c], R_inc = Rz(xi[2]) Ry(xi[1]) Rx(xi[0]), and T <- D T: increments
 *   compose and T is not re-orthonormalised.  new = eval(T); the stopping rule, bit 2, bit 4, the trace, the NULL
 *   outputs and the invalid-pair behaviour are mvr_icp_refine's.
 *   Status bits: 1 fewer than 6 correspondences; 2 the cap; 4 an invalid pair; 8 a degenerate system.
 *   One workgroup per pair, every iteration inside the one launch, no atomics, no workspace; a pair's outputs are a
 *   function of the pair alone.
 *   MVR_EINVAL: the rules of mvr_icp_refine; with P > 0 and M > 0 also a NULL normals.
 * ---------------------------------------------------------------------- */
int mvr_icp_refine_plane(const void* index, size_t index_bytes, const double* xyz, const double* normals,
                         const int64_t* off, int B, int64_t M, double r_index, const int64_t* pairs, const double* T0,
                         int P, double max_dist, int max_iters, double tol_fitness, double tol_rmse, double* T,
                         double* fitness, double* rmse, int32_t* n_corr, int32_t* iters, int32_t* status,
                         double* trace, mvr_stream_t stream);

/* ------------------------------------------------------------------------
 * Generalized (plane-to-plane) ICP refinement, batched over pairs (csrc/icp_gicp.hip): the loop of
 * Segal et al.'s GICP, Open3D's registration_generalized_icp, restated from the maths; Open3D parity is unpinned.
 * The arguments are those of mvr_icp_refine_plane plus epsilon.  normals [M,3] (the row order of xyz) covers every
 * fragment: a pair uses the normals of its source and of its target.  They are taken as given and NOT renormalised:
 * they must be unit (mvr_estimate_normals output is unit to 1e-14).  Their sign does not matter: only n n^T enters.
 *   A point with unit normal n has covariance C = I - (1 - epsilon) n n^T: 1 in the surface, epsilon along the
 *   normal (what Open3D's GICP assigns, from given normals or from the neighbourhood covariance).
 *   eval(T), fitness, rmse, n_corr: exactly mvr_icp_refine's (Euclidean distances), so the three methods' figures
 *   compare.
 *   Loop: state = eval(T0); up to max_iters times: stop with status bit 1 when n_corr < 6.  Over the valid pairs
 *   q = T x, y its match, R the rotation part of T, n the normal of y, m = R n_s with n_s the normal of x, c = the
 *   target fragment's first point (the per-pair origin of mvr_icp_refine_plane):
 *     M = 2 I - (1 - epsilon)(n n^T + m m^T)   (= C_y + R C_x R^T for unit normals and orthonormal R)
 *     A = M^-1, symmetric 3 x 3, inverted in closed form (cofactors over the determinant); eigenvalues of M in
 *     [2 epsilon, 2]
 *     G = [ -[q - c]x | I ]  (3 x 6: rotation first, translation last, as in mvr_icp_refine_plane),  d = q - y
 *     H = sum G^T A G,  g = sum G^T A d;  solve H xi = -g by Cholesky.
 *   A pivot that fails pivot > 1e-12 max_i H_ii (a NaN fails it too) stops the loop with status bit 8, T kept, iters
 *   not counted; normals that make M singular or non-finite end there.  Otherwise D = [R_inc | xi[3:6] + c - R_inc c],
 *   R_inc = Rz(xi[2]) Ry(xi[1]) Rx(xi[0]), and T <- D T: increments compose and T is not re-orthonormalised.
 *   new = eval(T); the stopping rule, bit 2, bit 4, the trace, the NULL outputs and the invalid-pair behaviour are
 *   mvr_icp_refine's.  epsilon == 1: M = 2 I, the normals drop out, and the loop is Gauss-Newton point-to-point.
 *   Status bits: 1 fewer than 6 correspondences; 2 the cap; 4 an invalid pair; 8 a degenerate system.
 *   fp64 throughout; one workgroup per pair, every iteration inside the one launch, no atomics, no workspace; a
 *   pair's outputs are a function of the pair alone.
 *   MVR_EINVAL: the rules of mvr_icp_refine_plane; also epsilon outside (0, 1] (a NaN included), checked with the
 *   scalars before P == 0 returns MVR_OK.
 * ---------------------------------------------------------------------- */
int mvr_icp_refine_generalized(const void* index, size_t index_bytes, const double* xyz, const double* normals,
                               const int64_t* off, int B, int64_t M, double r_index, const int64_t* pairs,
                               const double* T0, int P, double max_dist, double epsilon, int max_iters,
                               double tol_fitness, double tol_rmse, double* T, double* fitness, double* rmse,
                               int32_t* n_corr, int32_t* iters, int32_t* status, double* trace, mvr_stream_t stream);

/* ------------------------------------------------------------------------
 * Robust kernels on the three ICP variants, batched over pairs (csrc/icp_robust.hip): what Open3D's
 * RobustKernel does to registration_icp and registration_generalized_icp, restated from the maths; Open3D parity is
 * unpinned.  The arguments are those of mvr_icp_refine_generalized plus method, kernel, kernel_k and w_sum.
 *   method: MVR_ICP_POINT_TO_POINT (mvr_icp_refine), MVR_ICP_POINT_TO_PLANE (mvr_icp_refine_plane),
 *   MVR_ICP_GENERALIZED (mvr_icp_refine_generalized).  normals may be NULL for point-to-point; epsilon is looked at
 *   for generalized only.
 *   kernel, with r the residual of a valid correspondence and k = kernel_k > 0 the kernel's scale:
 *     MVR_KERNEL_L2      w = 1
 *     MVR_KERNEL_HUBER   w = k / max(|r|, k)
 *     MVR_KERNEL_CAUCHY  w = 1 / (1 + (r / k)^2)
 *     MVR_KERNEL_GM      w = k / (k + r^2)^2
 *     MVR_KERNEL_TUKEY   w = (1 - (r / k)^2)^2 for |r| <= k, else 0
 *   All are continuous in r, Tukey's at |r| == k too.  L1 is not built: its weight 1 / |r| is unbounded at r = 0.
 *   kernel_k is not looked at for L2.
 *   Point-to-point: r = |q - y| (the distance of the search).  The solve is the weighted Kabsch solution on the
 *   original source points: with W = sum w the means sum w x / W and sum w y / W, the covariance
 *   sum w x y^T - W m_x m_y^T, and mvr_icp_refine's per-pair origins, SVD and det correction.  If W > 0 fails (a NaN
 *   fails it too) the loop ends with status bit 8, T kept, iters not counted: bit 8 exists for this method through
 *   this entry only.
 *   Point-to-plane: r = b = (q - y) . n;  H = sum w a a^T, g = sum w a b, with a, b, c and the Cholesky pivot rule of
 *   mvr_icp_refine_plane.  All-zero weights fail the first pivot: bit 8.
 *   Generalized: r = sqrt(d^T A d), d = q - y and A = M^-1 of mvr_icp_refine_generalized (a negative rounding of
 *   d^T A d counts as 0);  H = sum w G^T A G, g = sum w G^T A d.
 *   The weights of a solve are evaluated at the T the solve starts from: one step of iteratively reweighted least
 *   squares per ICP iteration, as Open3D does.  eval(T), fitness, rmse, n_corr, the stopping rule, the trace, the
 *   status bits 1, 2 and 4 and the least correspondence counts (3 / 6 / 6, on the unweighted count) are exactly those
 *   of the method's own entry: weights enter the solve only, so the figures compare across kernels.
 *   MVR_KERNEL_L2 returns, for each method, T, fitness, rmse, n_corr, iters, status and trace bit-identical to the
 *   method's own entry (a weight of exactly 1.0 in the same products).
 *   w_sum [P] (may be NULL): sum w over the valid correspondences of the returned T's evaluation; with L2 that equals
 *   n_corr; 0 for an invalid pair.
 *   fp64 throughout; one workgroup per pair, every iteration inside the one launch, no atomics, no workspace, the
 *   reduction in a fixed order; a pair's outputs are a function of the pair alone.
 *   MVR_EINVAL, scalars first: the rules of the method's own entry (epsilon for generalized only); a method or a
 *   kernel outside its range; for a kernel other than L2 a kernel_k that is not > 0 (a NaN included).  P == 0 then
 *   returns MVR_OK.  With P > 0 and M > 0 a NULL normals for the two methods that use them.
 * ---------------------------------------------------------------------- */
#define MVR_ICP_POINT_TO_POINT 0
#define MVR_ICP_POINT_TO_PLANE 1
#define MVR_ICP_GENERALIZED 2
#define MVR_KERNEL_L2 0
#define MVR_KERNEL_HUBER 1
#define MVR_KERNEL_CAUCHY 2
#define MVR_KERNEL_GM 3
#define MVR_KERNEL_TUKEY 4
int mvr_icp_refine_robust(const void* index, size_t index_bytes, const double* xyz, const double* normals,
                          const int64_t* off, int B, int64_t M, double r_index, const int64_t* pairs, const double* T0,
                          int P, int method, double max_dist, double epsilon, int kernel, double kernel_k,
                          int max_iters, double tol_fitness, double tol_rmse, double* T, double* fitness, double* rmse,
                          int32_t* n_corr, int32_t* iters, int32_t* status, double* trace, double* w_sum,
                          mvr_stream_t stream);

/* ------------------------------------------------------------------------
 * Per-point intensity and its tangent-plane gradient on a radius index (csrc/color_grad.hip): what
 * Open3D's registration_colored_icp prepares on its target (InitializePointCloudForColoredICP), restated from the
 * maths; Open3D parity is unpinned.
 *   index, xyz [M,3], off [B+1], r_index: the arguments of the mvr_radius_index_build call that made `index`.
 *   normals [M,3] (taken as given, not renormalised; their sign does not matter), colors fp64 [M,3] in the row order
 *   of xyz.
 *   intensity[i] = I_i = (c0 + c1 + c2) / 3.0, evaluated in that order.
 *   The neighbours of point i are the points of its own fragment with sqrt(ex*ex + ey*ey + ez*ez) < radius (strict),
 *   e = x_j - x_i; the point itself is one of them.  n_nbr[i] = their number (n_nbr may be NULL).  Fewer than 4: the
 *   gradient is 0.  Otherwise, with n the normal of i and u = e - (e . n) n over the neighbours in the index's walk
 *   order:  A = sum u u^T + (n_nbr - 1)^2 n n^T,  h = sum u (I_j - I_i);  grad[i] = d with A d = h by 3 x 3 Cholesky
 *   (the normal equations of Open3D's rows u_j . d = I_j - I_i and (n_nbr - 1) n . d = 0).  A pivot that fails
 *   pivot > 1e-12 max_i A_ii (a NaN fails it too) gives gradient 0, and so does a solution that is not finite (a NaN
 *   or infinite colour in the ball): the gradient is always finite.
 *   intensity [M], grad [M,3] and n_nbr [M] in the row order of xyz; every row is written.  fp64 throughout; one
 *   thread per point, no atomics, no LDS, no workspace; a point's outputs are a function of its fragment alone.
 *   MVR_EINVAL, scalars first: the rules of mvr_estimate_normals.  M == 0 then returns MVR_OK.  With M > 0: a NULL
 *   index, xyz, normals, colors, off, intensity or grad, or index_bytes < mvr_radius_index_bytes(M).
 * ---------------------------------------------------------------------- */
int mvr_color_gradient(const void* index, size_t index_bytes, const double* xyz, const double* normals,
                       const double* colors, const int64_t* off, int B, int64_t M, double r_index, double radius,
                       double* intensity, double* grad, int32_t* n_nbr, mvr_stream_t stream);

/* ------------------------------------------------------------------------
 * Coloured ICP refinement, batched over pairs (csrc/icp_colored.hip): the loop of Park, Zhou and
 * Koltun's coloured ICP (2017), Open3D's registration_colored_icp, restated from the maths; Open3D parity is
 * unpinned.  The arguments are those of mvr_icp_refine_plane plus intensity [M], grad [M,3] (mvr_color_gradient's
 * outputs, the row order of xyz), lambda_geometric, and mvr_icp_refine_robust's kernel, kernel_k and w_sum.
 *   eval(T), fitness, rmse, n_corr: exactly mvr_icp_refine's (Euclidean distances), so the methods' figures compare.
 *   Loop: state = eval(T0); up to max_iters times: stop with status bit 1 when n_corr < 6.  Over the valid pairs, for
 *   source row i moved to q = T x_i and matched with target row t: y its point, n its normal, d its gradient,
 *   c = the target fragment's first point (the per-pair origin of mvr_icp_refine_plane), lambda = lambda_geometric:
 *     e = q - y;  g = e . n;  r_I = I[i] - (I[t] + d . (e - g n));  dM = -(d - (d . n) n)
 *     J_G = [(q - c) x n, n],  J_I = [(q - c) x dM, dM]
 *     w_G = w(sqrt(lambda) g),  w_I = w(sqrt(1 - lambda) r_I)     (the kernel sees the scaled residuals, as Open3D's)
 *     H = sum lambda w_G J_G J_G^T + (1 - lambda) w_I J_I J_I^T
 *     b = sum lambda w_G J_G g + (1 - lambda) w_I J_I r_I;  solve H xi = -b by Cholesky.
 *   The pivot rule with status bit 8, the increment about c, T <- D T, the stopping rule, bits 2 and 4, the trace, the
 *   NULL outputs and the invalid-pair behaviour are mvr_icp_refine_plane's.  lambda == 1 is the point-to-plane solve.
 *   kernel, kernel_k: mvr_icp_refine_robust's weights w(r); MVR_KERNEL_L2 is the plain loop (no weight is computed).
 *   w_sum [P] (may be NULL): sum (lambda w_G + (1 - lambda) w_I) over the valid correspondences of the returned T's
 *   evaluation; with L2 that is n_corr exactly; 0 for an invalid pair.
 *   fp64 throughout; one workgroup per pair, every iteration inside the one launch, no atomics, no workspace, the
 *   reduction in a fixed order; a pair's outputs are a function of the pair alone.
 *   MVR_EINVAL, scalars first: lambda_geometric outside [0, 1] (a NaN included); a kernel outside its range; for a
 *   kernel other than L2 a kernel_k that is not > 0; the rules of mvr_icp_refine.  P == 0 then returns MVR_OK.  With
 *   P > 0 and M > 0 also a NULL normals, intensity or grad.
 * ---------------------------------------------------------------------- */
int mvr_icp_refine_colored(const void* index, size_t index_bytes, const double* xyz, const double* normals,
                           const double* intensity, const double* grad, const int64_t* off, int B, int64_t M,
                           double r_index, const int64_t* pairs, const double* T0, int P, double max_dist,
                           double lambda_geometric, int kernel, double kernel_k, int max_iters, double tol_fitness,
                           double tol_rmse, double* T, double* fitness, double* rmse, int32_t* n_corr, int32_t* iters,
                           int32_t* status, double* trace, double* w_sum, mvr_stream_t stream);

/* ------------------------------------------------------------------------
 * Per-pair 6 x 6 information matrices on a radius index (csrc/info.hip): what Open3D's
 * get_information_matrix_from_point_clouds gives a pose-graph edge, restated from the maths.
 * The arguments are those of mvr_icp_refine without the loop settings; T [P,12] (3x4 row-major) is evaluated as it
 * is.  The correspondences of pair p are exactly those of eval(T) of mvr_icp_refine: the target point y nearest to
 * q = R x + t, valid iff sqrt(ex*ex + ey*ey + ez*ez) < max_dist (strict), the lowest row on equal distances.
 *   info [P,36] row-major = sum over the valid correspondences of G_y^T G_y with G_y = [ I3 | -[y]x ] (3 x 6), y the
 *   target point: the parameter order is (translation v, rotation omega), the order lib.utils
 *   computeTransformationErr assumes, so info[0] == n_corr exactly, and xi^T info xi is the summed squared
 *   displacement of the matched target-side points under the small motion q -> q + v + omega x q about the target
 *   frame's origin.  Open3D uses the same G with the blocks in (omega, v) order (lib.icp.information_matrix offers
 *   that permutation).  Open3D is absent here, so Open3D parity is unpinned; Redwood's published .info files are
 *   not pinned either: whether they were built with omega or with the quaternion's vector part (a factor of 2 on the
 *   rotation block) cannot be checked here.
 *   n_corr [P] (may be NULL), rmse [P] = sqrt(sum d^2 / n_corr) (0 without correspondences), status [P]: 0, or 4 for
 *   an invalid pair by the rules of mvr_icp_refine's bit 4 — then info all zero, n_corr = 0, rmse = 0.
 *   fp64 throughout; one workgroup per pair, no atomics, no workspace, the reduction in a fixed order: a pair's
 *   outputs are a function of the pair alone (bit-identical whatever the batch around it).
 *   MVR_EINVAL, scalars first: negative P or M; B <= 0 or B >= 32768; M >= 2^31; max_dist or r_index <= 0;
 *   max_dist > r_index.  P == 0 then returns MVR_OK.  With P > 0: a NULL pairs, T, info, rmse or status; with M > 0
 *   a NULL index, xyz or off, or index_bytes < mvr_radius_index_bytes(M).
 * ---------------------------------------------------------------------- */
int mvr_pair_information(const void* index, size_t index_bytes, const double* xyz, const int64_t* off, int B,
                         int64_t M, double r_index, const int64_t* pairs, const double* T, int P, double max_dist,
                         double* info, int32_t* n_corr, double* rmse, int32_t* status, mvr_stream_t stream);

/* ------------------------------------------------------------------------
 * FPFH descriptors on a radius index (csrc/fpfh.hip): the Fast Point Feature Histogram of Rusu et
 * al., what Open3D's compute_fpfh_feature(KDTreeSearchParamRadius(radius)) and PCL's FPFHEstimation give, restated
 * from the maths; Open3D / PCL parity is unpinned.  tests/fpfh_oracle.py is the numpy restatement.
 *   index, xyz [M,3], off [B+1], r_index: the arguments of the mvr_radius_index_build call that made `index`;
 *   normals [M,3] fp64 in the row order of xyz, taken as given (not renormalised).  Their SIGN MATTERS here, unlike
 *   for the ICPs: orient them consistently, e.g. with the viewpoints of mvr_estimate_normals.
 *   Neighbours of point i: the points j != i (by row, so a coincident point is one) of its own fragment with
 *   sqrt(ex*ex + ey*ey + ez*ez) < radius (strict, the expression of mvr_estimate_normals), e = x_j - x_i; k_i their
 *   number.
 *   Pair feature of (i, j): d = |e|, a1 = n_i . e / d, a2 = n_j . e / d.  If |a1| < |a2| the roles swap:
 *   (n_a, n_b, e, f2) = (n_j, n_i, -e, -a2), otherwise (n_i, n_j, e, a1).  v = (e x n_a) / |e x n_a|, w = n_a x v,
 *   f0 = atan2(w . n_b, n_a . n_b), f1 = v . n_b.  A neighbour with d == 0 or |e x n_a| == 0 adds nothing to the
 *   histogram but still counts in k_i.
 *   Bins, eleven per feature, each index clamped to [0, 10]: floor(11 (f0 + pi) / (2 pi)) in bins 0..10,
 *   floor(11 (f1 + 1) / 2) in bins 11..21, floor(11 (f2 + 1) / 2) in bins 22..32.
 *   SPFH: spfh_i[c] = 100 count_i[c] / k_i from integer counts (independent of the order of the neighbours); zeros
 *   when k_i == 0.
 *   FPFH: acc[c] = sum over the neighbours with d > 0 of spfh_j[c] / d^2 (d^2 = ex*ex + ey*ey + ez*ez); each of the
 *   three groups of 11 of acc with a positive sum is scaled to sum to 100; fpfh_i = acc + spfh_i.  Geometry and
 *   accumulation are fp64; the outputs are rounded to fp32 once.
 *   fpfh [M,33] and spfh_out [M,33] (may be NULL) in the row order of xyz; every row is written.  Two launches (SPFH,
 *   then FPFH) with the fp64 SPFH rows in `workspace` (>= mvr_compute_fpfh_workspace_bytes(M)); one thread per
 *   point, no atomics; a point's outputs are a function of its fragment alone.
 *   MVR_EINVAL, scalars first: the rules of mvr_estimate_normals (radius > r_index among them).  M == 0 then returns
 *   MVR_OK.  With M > 0: a NULL index, xyz, off, normals, fpfh or workspace, index_bytes <
 *   mvr_radius_index_bytes(M), or workspace_bytes < mvr_compute_fpfh_workspace_bytes(M).
 * ---------------------------------------------------------------------- */
size_t mvr_compute_fpfh_workspace_bytes(int64_t M);
int mvr_compute_fpfh(const void* index, size_t index_bytes, const double* xyz, const double* normals,
                     const int64_t* off, int B, int64_t M, double r_index, double radius, float* fpfh,
                     float* spfh_out, void* workspace, size_t workspace_bytes, mvr_stream_t stream);

/* ------------------------------------------------------------------------
 * Exact k nearest neighbours of every point within its own fragment, on a radius index (csrc/knn_self.hip;
 * DESIGN.md 4.21a): Open3D's KDTreeFlann.search_knn_vector_3d on the cloud the tree was built on, restated from the
 * maths; Open3D parity is unpinned.  tests/knn_oracle.py is the numpy restatement.
 *   index, xyz [M,3], off [B+1], r_index: the arguments of the mvr_radius_index_build call that made `index`.
 *   Candidates of point i: every point j of its own fragment, i itself included.
 *   d2(i, j) = (ex*ex + ey*ey) + ez*ez, e = x_j - x_i, in fp64 with every product and sum rounded on its own (no
 *   FMA), so a host restatement reproduces dist2 bit for bit.
 *   Row i of idx [M,k] / dist2 [M,k] holds the min(k, n_b) smallest candidates ordered by (d2, row) lexicographically:
 *   on equal distances the lower row first, so with exact duplicates a point need not be its own first neighbour.
 *   idx are rows of xyz (global, not fragment-local).  The remaining entries are idx = -1, dist2 = +inf.  Every one
 *   of the M k entries is written and nothing beyond them; rows are in the row order of xyz.  (A candidate whose d2
 *   is NaN is never returned.)
 *   The search is exact for any input and any r_index: r_index only decides the cost.  One thread per point walks the
 *   cells around it ring by ring (2 rings); a point whose k-th neighbour is not certain by then is resolved by a
 *   second launch that scans its fragment's rows, n_b distance evaluations.  A point's outputs are a function of its
 *   fragment alone: bit-identical whatever other fragments are in the batch (apart from the row offset in idx) and
 *   from run to run.  No host synchronisation.  After the call the first int32 of `workspace`
 *   (>= mvr_knn_self_workspace_bytes(M)) holds the number of points the second launch resolved (a diagnostic).
 *   MVR_EINVAL, scalars first: negative M or M >= 2^31; B <= 0 or B >= 32768; r_index <= 0; k < 1 or k > 64.
 *   M == 0 then returns MVR_OK.  With M > 0: a NULL index, xyz, off, idx, dist2 or workspace,
 *   index_bytes < mvr_radius_index_bytes(M), or workspace_bytes < mvr_knn_self_workspace_bytes(M).
 * ---------------------------------------------------------------------- */
size_t mvr_knn_self_workspace_bytes(int64_t M);
int mvr_knn_self(const void* index, size_t index_bytes, const double* xyz, const int64_t* off, int B, int64_t M,
                 double r_index, int k, int32_t* idx, double* dist2, void* workspace, size_t workspace_bytes,
                 mvr_stream_t stream);

/* ------------------------------------------------------------------------
 * Outlier statistics of a fragment's own points (csrc/outlier.hip): what Open3D's
 * remove_statistical_outlier(nb_neighbors, std_ratio) and remove_radius_outlier(nb_points, radius) decide on, each
 * fragment its own cloud as when Open3D is called per fragment, restated from the maths; Open3D parity is unpinned.
 * mvr_statistical_outlier: dist2 [M,k] is the output of mvr_knn_self with k = nb_neighbors (the point itself counts
 *   among them, as in Open3D).  mean_i = (sum over the found entries, in ascending slot order, of sqrt(dist2[i,s]))
 *   / min(k, n_b); per fragment b: mu_b = mean of mean_i, sd_b = sqrt(sum (mean_i - mu_b)^2 / (n_b - 1)),
 *   thr_b = mu_b + std_ratio sd_b, keep_i = mean_i < thr_b (strict).  A fragment with n_b < 2 keeps all its points
 *   and has thr_b = +inf (Open3D divides by zero there).  Outputs keep [M] (0 / 1), mean_dist [M], thr [B].
 *   One workgroup per fragment, sums in a fixed order through a fixed tree: bit-identical from run to run, and a
 *   fragment's outputs do not depend on the batch around it.
 *   MVR_EINVAL, scalars first: negative M or M >= 2^31; B <= 0 or B >= 32768; k < 1 or k > 64; std_ratio <= 0.
 *   M == 0 then returns MVR_OK with nothing written (thr neither).  With M > 0: a NULL dist2, off, keep, mean_dist
 *   or thr.
 * mvr_radius_count: count[i] = the number of points of i's fragment with sqrt(ex*ex + ey*ey + ez*ez) < radius,
 *   e = x_j - x_i: the expression, the strictness and the inclusion of the point itself of mvr_estimate_normals'
 *   n_nbr (one walk, csrc/rindex.hpp).  Open3D keeps a point when count > nb_points.
 *   MVR_EINVAL, scalars first: the rules of mvr_estimate_normals (radius > r_index among them).  M == 0 then returns
 *   MVR_OK.  With M > 0: a NULL index, xyz, off or count, or index_bytes < mvr_radius_index_bytes(M).
 * ---------------------------------------------------------------------- */
int mvr_statistical_outlier(const double* dist2, const int64_t* off, int B, int64_t M, int k, double std_ratio,
                            uint8_t* keep, double* mean_dist, double* thr, mvr_stream_t stream);
int mvr_radius_count(const void* index, size_t index_bytes, const double* xyz, const int64_t* off, int B, int64_t M,
                     double r_index, double radius, int32_t* count, mvr_stream_t stream);

/* ------------------------------------------------------------------------
 * DBSCAN clustering of every fragment's own points, on a radius index (csrc/dbscan.hip): what
 * Open3D's cluster_dbscan(eps, min_points) returns when it is called per fragment, restated from the definition;
 * Open3D parity is unpinned.  tests/dbscan_oracle.py restates Open3D's sequential loop in numpy.
 *   index, xyz [M,3], off [B+1], r_index: the arguments of the mvr_radius_index_build call that made `index`.
 *   Neighbourhood: N(i) = the rows t of i's fragment with sqrt(ex*ex + ey*ey + ez*ez) < eps, e = x_t - x_i: the
 *   expression, the strictness and the inclusion of i itself (and of its duplicates) of mvr_radius_count (one walk,
 *   csrc/rindex.hpp), so the relation is symmetric bit for bit.  Open3D and sklearn take d <= eps: the results differ
 *   only where a distance equals eps exactly.
 *   Core: row i is core iff |N(i)| >= min_points.
 *   Clusters: the connected components of the graph on the core rows with an edge i - t iff t is in N(i).  A
 *   fragment's clusters are numbered 0 .. n_b - 1 by ascending smallest core row.
 *   Border: a row that is not core with at least one core row in N(i) takes the lowest-numbered cluster among its
 *   core neighbours' clusters.  Noise: every other row that is not core, label -1.
 *   That is what the sequential loop (Open3D's, sklearn's) returns: it grows the clusters one after another in
 *   seed order, a cluster is first reached at its smallest core row, and a border point keeps the first cluster
 *   that reaches it, the lowest-numbered one.
 *   Outputs: labels [M] (the cluster's number within its fragment, or -1); n_clusters [B] (0 for an empty
 *   fragment); sizes [M] or NULL: sizes[off[b] + c] = the points labelled c in fragment b, 0 for c >= n_clusters[b],
 *   all M entries written; core [M] or NULL: 1 / 0.  Nothing is written behind these extents.
 *   The outputs are a pure function of the fragment's points and their row order: bit-identical whatever other
 *   fragments are in the batch, whatever the launch geometry, and from run to run (the components are united by
 *   lock-free hooking of the larger root under the smaller, whose result, the smallest core row as the root, does not
 *   depend on the interleaving; no thread waits for another).  No host synchronisation.
 *   MVR_EINVAL, scalars first: negative M or M >= 2^31; B <= 0 or B >= 32768; r_index <= 0; eps outside
 *   (0, r_index] (a NaN is outside); min_points < 1.  M == 0 then returns MVR_OK with nothing written.  With M > 0: a
 *   NULL index, xyz, off, labels, n_clusters or workspace, index_bytes < mvr_radius_index_bytes(M), or
 *   workspace_bytes < mvr_dbscan_workspace_bytes(M).
 * ---------------------------------------------------------------------- */
size_t mvr_dbscan_workspace_bytes(int64_t M);
int mvr_cluster_dbscan(const void* index, size_t index_bytes, const double* xyz, const int64_t* off, int B, int64_t M,
                       double r_index, double eps, int min_points, int32_t* labels, int32_t* n_clusters,
                       int32_t* sizes, uint8_t* core, void* workspace, size_t workspace_bytes, mvr_stream_t stream);

/* ------------------------------------------------------------------------
 * ISS keypoints (Intrinsic Shape Signatures, Zhong 2009) of every fragment's own points, on a radius index
 * (csrc/iss.hip): Open3D's compute_iss_keypoints restated from the maths, each fragment its own cloud;
 * Open3D parity is unpinned.  tests/iss_oracle.py is the numpy restatement.  Two launches, each one thread per point,
 * fp64, no atomics, no workspace; a point's outputs are a function of its fragment alone and repeat bit for bit.
 *   index, xyz [M,3], off [B+1], r_index: the arguments of the mvr_radius_index_build call that made `index`.
 * mvr_iss_saliency: the neighbours of point i are the points of its fragment with
 *   sqrt(ex*ex + ey*ey + ez*ez) < salient_radius, e = x_j - x_i (strict, i itself among them: the set and the count
 *   n_nbr of mvr_estimate_normals).  C = their covariance about their own mean, divided by n, accumulated in
 *   coordinates relative to x_i; l1 >= l2 >= l3 its eigenvalues (cyclic Jacobi).  saliency[i] = l3 when
 *   n >= min_neighbors, l3 > min_ratio l1, l2 < gamma_21 l1 and l3 < gamma_32 l2; exactly -1.0 otherwise.  The
 *   products are Open3D's quotients l2 / l1 < gamma_21, l3 / l2 < gamma_32 without the divisions.  min_ratio is an
 *   addition: on a planar neighbourhood l3 is zero up to rounding, which would otherwise decide; 0 gives
 *   Open3D's rule.  n_nbr [M] may be NULL.  Every saliency[i] and n_nbr[i] is written.
 *   MVR_EINVAL, scalars first: negative M or M >= 2^31; B <= 0 or B >= 32768; r_index <= 0; salient_radius outside
 *   (0, r_index]; a gamma outside (0, 1]; min_ratio outside [0, 1); min_neighbors < 1 (NaN is outside every range).
 *   M == 0 then returns MVR_OK.  With M > 0: a NULL index, xyz, off or saliency, or
 *   index_bytes < mvr_radius_index_bytes(M).
 * mvr_radius_nms: non-maximum suppression of any score [M] over the ball of `radius` (the same membership rule).
 *   keep[i] = 1 when score[i] > 0, the ball of i holds at least min_neighbors points (i among them), and no point
 *   j != i of the ball has score[j] > score[i], or score[j] == score[i] with j < i; 0 otherwise.  Every keep[i] is
 *   written.  A NaN score is never kept and never suppresses (every comparison with it is false).
 *   The tie rule differs from Open3D on purpose: Open3D keeps both points of a tie, so duplicated points (which share
 *   their neighbours and hence their saliency) give duplicated keypoints; here only the lower row survives.
 *   MVR_EINVAL, scalars first: as above with `radius`; M == 0 then returns MVR_OK.  With M > 0: a NULL index, xyz,
 *   off, score or keep, or index_bytes < mvr_radius_index_bytes(M).
 * ---------------------------------------------------------------------- */
int mvr_iss_saliency(const void* index, size_t index_bytes, const double* xyz, const int64_t* off, int B, int64_t M,
                     double r_index, double salient_radius, double gamma_21, double gamma_32, double min_ratio,
                     int min_neighbors, double* saliency, int32_t* n_nbr, mvr_stream_t stream);
int mvr_radius_nms(const void* index, size_t index_bytes, const double* xyz, const int64_t* off, int B, int64_t M,
                   double r_index, double radius, int min_neighbors, const double* score, uint8_t* keep,
                   mvr_stream_t stream);

/* ------------------------------------------------------------------------
 * Nearest neighbour in feature space between ragged fragments (csrc/feat_match.hip), for any channel
 * count 1 <= C <= 64 (mvr_feat_knn2 is the MFMA kernel for C == 32 and equal-sized sampled sets).
 *   F [M,C] fp32 with row stride C, fragments off [B+1] (device); pairs [P,2] (device): (query fragment, target
 *   fragment); qoff [P+1] (device): the prefix sums of the query fragments' sizes, computed by the caller on the host,
 *   who passes n_queries == qoff[P] and max_q == the largest query fragment of a pair (they size the launch).
 *   For query row i of pair p: idx[qoff[p] + i] = the row within the target fragment that minimises
 *   sum_c (a_c - b_c)^2, accumulated in fp32 over c ascending; ties go to the smallest row; dist2 (may be NULL) that
 *   sum.  An empty target fragment gives -1 (dist2 +inf); so does a pair with a fragment index outside [0, B), and a
 *   query row beyond the query fragment's size where qoff disagrees with off.  Plain fp32 vector arithmetic, no
 *   MFMA, no atomics, no workspace: a query's outputs are a function of its pair alone.
 *   MVR_EINVAL, scalars first: C outside 1..64; negative P, M, n_queries or max_q; B <= 0 or B >= 32768;
 *   M >= 2^31; max_q > 65535 * 256.  P == 0 or n_queries == 0 then returns MVR_OK.  Otherwise a NULL F, off, pairs,
 *   qoff or idx, or max_q == 0.
 * ---------------------------------------------------------------------- */
int mvr_feat_match(const float* F, int C, const int64_t* off, int B, int64_t M, const int64_t* pairs,
                   const int64_t* qoff, int P, int64_t n_queries, int64_t max_q, int32_t* idx, float* dist2,
                   mvr_stream_t stream);

/* ------------------------------------------------------------------------
 * Pose-graph refinement over SE(3), batched over scenes (csrc/posegraph.hip): the Levenberg-
 * Marquardt stage of Open3D's global_optimization / Choi et al. 2015, restated from the maths (Open3D parity is
 * unpinned; this entry has no line process or robust kernel, mvr_posegraph_optimize_lp below has the line process).
 * tests/posegraph_oracle.py is the normative text.
 *   Scenes, edges, fragments, strides and conventions are mvr_sync_poses': edge e = (i, j) with x_j ~ T_e x_i,
 *   T_e = (R_pair, t_pair); pose M_f: X = R_f x_f + t_f.  info [., 36]: the edge's 6 x 6 matrix in (v, omega) order
 *   (mvr_pair_information's), rows as R_pair; (info + info^T) / 2 is what is used.  R0 [., 9], t0 [., 3]: the initial
 *   poses, rows as R / t.  The anchor's pose is held at its input value.
 *   Residual: D_e = M_j^-1 M_i T_e^-1, xi_e = (v, omega) with v the translation of D_e and omega the rotation vector
 *   of its rotation: a = vee(D - D^T) / 2, theta = atan2(|a|, (tr D - 1) / 2), omega = a theta / |a| (|a| <= 1e-8:
 *   a (1 + theta^2 / 6); inaccurate near theta = pi, where no edge of a sane start lies).
 *   Cost c = sum_e w_e xi_e^T info_e xi_e.  Update delta_f = (dv, dw), applied on the left: R_f <- Exp(dw) R_f,
 *   t_f <- Exp(dw) t_f + dv.  First-order Jacobian: d xi_e / d delta_i = A_e, d xi_e / d delta_j = -A_e,
 *   A_e = Ad(M_j^-1) = [[R_j^T, -R_j^T [t_j]x], [0, R_j^T]].  H = sum w J^T info J, g = sum w J^T info xi; the rows
 *   and columns of the anchor and of the non-members are replaced by identity.
 *   Members: the fragments reachable from the anchor over edges with w > 0; an edge with a non-member end gets
 *   weight 0; non-members come out with their input pose and member 0.
 *   Loop: lambda = lambda0.  A trial solves (H + lambda diag H) delta = -g by Cholesky, forms the candidate poses and
 *   their cost c'; c' < c accepts (lambda /= 10), otherwise the poses stay (lambda *= 10).  A pivot that is not
 *   positive is a rejected trial without a candidate.  Every trial counts in iters.  Converged: after an accepted
 *   trial with c - c' <= tol_cost c, after any trial that had a candidate with max|delta| <= tol_step (applied if it
 *   was accepted), or when c == 0 (also at the start).  Both tolerances 0: max_iters trials unless c reaches 0 or
 *   delta is exactly 0.
 *   Outputs: R, t, member (may be NULL), cost [S,2] (initial, final), iters [S], status [S], trace [S, max_iters + 1]
 *   (may be NULL): the cost held at the start and after every trial (unchanged by a rejected one), -1 after the last.
 *   Status bits: 1 some fragment is not a member; 2 max_iters trials without convergence while a tolerance is
 *   positive; 4 an edge was ignored (index out of range, i == j, a non-finite T, info or w, a negative w, or
 *   max|info - info^T| > 1e-9 |info|_F), or the scene is invalid (anchor >= n_frags[s], a count negative or above its
 *   maximum, n_frags 0 with edges, a non-finite initial pose): the poses are copied through, member 0, cost 0,
 *   iters 0, bit 1 as well when it has fragments; 8 the last trial's factorisation failed.
 *   fp64 throughout; one workgroup per scene, every trial inside the one launch, no floating-point or global
 *   atomics (two flag words in LDS are set by an idempotent atomicOr): a scene's outputs are a function of the
 *   scene alone.  max_frags <= MVR_SYNC_MAX_FRAGS; workspace (8-byte aligned) >=
 *   mvr_posegraph_workspace_bytes(S, max_frags, max_edges).
 *   MVR_EINVAL: negative S / max_frags / max_edges / max_iters; max_frags above the maximum; anchor outside
 *   [0, max_frags) (when max_frags > 0); lambda0 negative or non-finite; a negative tolerance.  S == 0 or
 *   max_frags == 0 then returns MVR_OK.  Otherwise a NULL n_edges, n_frags, R0, t0, R, t, cost, iters or status; with
 *   max_edges > 0 a NULL R_pair, t_pair, ij or info; a short or misaligned workspace; with S > 1 a stride below its
 *   maximum count.
 * ---------------------------------------------------------------------- */
size_t mvr_posegraph_workspace_bytes(int S, int max_frags, int max_edges);
int mvr_posegraph_optimize(const double* R_pair, const double* t_pair, const int32_t* ij, const double* w,
                           const double* info, int64_t e_sstride, const int32_t* n_edges, const int32_t* n_frags,
                           int S, int max_frags, int max_edges, int anchor, const double* R0, const double* t0,
                           int max_iters, double lambda0, double tol_cost, double tol_step, double* R, double* t,
                           int64_t f_sstride, int32_t* member, double* cost, int32_t* iters, int32_t* status,
                           double* trace, void* workspace, size_t workspace_bytes, mvr_stream_t stream);

/* ------------------------------------------------------------------------
 * Pose-graph refinement with a line process on the uncertain edges (csrc/posegraph.hip): the robust
 * stage of Open3D's global_optimization / Choi et al. 2015, restated from the maths (Open3D parity is unpinned).
 * tests/posegraph_lp_oracle.py is the normative text.  Everything not said here (conventions, residual xi_e,
 * (info + info^T) / 2, members, ignored edges, the update, the Levenberg-Marquardt trial, stopping rules, status bits
 * 1 / 2 / 4 / 8, the trace, determinism, the NULL and stride rules) is mvr_posegraph_optimize's.
 *   uncertain [., 1] int32 (rows as R_pair; may be NULL: every edge is uncertain): non-zero marks a loop-closure
 *   edge.  An edge "counts" when its weight is positive after the validity and membership rules.
 *   r_e = w_e xi_e^T info_e xi_e.  mu = mu_scale * mean of info_e[0] over the counted uncertain edges (info[0] is the
 *   correspondence count in the (v, omega) order; Open3D's info(3, 3) in its (omega, v) order).  mu_scale =
 *   preference_loop_closure * max_correspondence_distance^2 in Open3D's terms; the caller forms the product.
 *   l_e = s_e^2, s_e = mu / (mu + r_e), for a counted uncertain edge; 1 for a counted certain edge.
 *   Cost c = (sum_certain r_e + sum_uncertain l_e r_e) + mu sum_uncertain (s_e - 1)^2, each sum in the fixed order;
 *   at the closed-form l this is the Geman-McClure cost sum_certain r_e + sum_uncertain mu r_e / (mu + r_e).
 *   Start: l in closed form at the initial poses, c from it.  A trial builds H and g with the weights w_e l_e, l held,
 *   and evaluates the candidate's cost c' with the same held l (and the held third sum); c' < c accepts.  After an
 *   accepted trial l is recomputed in closed form at the new poses (from the r_e the candidate's cost pass formed),
 *   which gives c'' <= c'; the held cost becomes c'', lambda /= 10, and the tol_cost test is c - c'' <= tol_cost c.
 *   After a rejected trial lambda *= 10 and l stays.  Every cost in the trace is thus a Geman-McClure cost, and the
 *   trace does not rise.
 *   Status bit 16: a counted uncertain edge exists but mu is not positive and finite (e.g. all-zero information on
 *   the uncertain edges); the scene then runs with every edge certain, l = 1.
 *   Without a counted uncertain edge (uncertain all zero) R, t, member, cost, iters, status and trace equal
 *   mvr_posegraph_optimize's byte for byte: the second and third sums are 0.0 and every weight is w_e * 1.0.
 *   Outputs beyond mvr_posegraph_optimize's: line [., 1] fp64 (rows as R_pair): the final l_e, 1 for a counted
 *   certain edge, 0 for an edge that does not count and for every edge of an invalid scene; mu [S] (may be NULL): mu
 *   as computed, 0 when no uncertain edge counts.
 *   workspace (8-byte aligned) >= mvr_posegraph_lp_workspace_bytes(S, max_frags, max_edges): mvr_posegraph_optimize's
 *   plus l and r, two doubles per edge.
 *   MVR_EINVAL: as mvr_posegraph_optimize; a mu_scale that is not finite and positive (checked first); a NULL line
 *   with max_edges > 0 (where mvr_posegraph_optimize's pointers are required).
 * ---------------------------------------------------------------------- */
size_t mvr_posegraph_lp_workspace_bytes(int S, int max_frags, int max_edges);
int mvr_posegraph_optimize_lp(const double* R_pair, const double* t_pair, const int32_t* ij, const double* w,
                              const double* info, const int32_t* uncertain, int64_t e_sstride, const int32_t* n_edges,
                              const int32_t* n_frags, int S, int max_frags, int max_edges, int anchor, const double* R0,
                              const double* t0, int max_iters, double lambda0, double tol_cost, double tol_step,
                              double mu_scale, double* R, double* t, int64_t f_sstride, int32_t* member, double* cost,
                              int32_t* iters, int32_t* status, double* trace, double* line, double* mu,
                              void* workspace, size_t workspace_bytes, mvr_stream_t stream);

/* ------------------------------------------------------------------------
 * Scene fusion (csrc/fuse.hip): the registered fragments mapped by their poses into one frame and
 * merged per voxel.  What Open3D users write as `pcd_combined += pcd.transform(pose)` followed by
 * voxel_down_sample(voxel): VoxelDownSample of the concatenated, transformed cloud, restated; Open3D parity unpinned.
 * tests/fuse_oracle.py is the numpy restatement.
 *   xyz [M,3], normals [M,3] (may be NULL), off [B+1] (device): the fp64 arrays of a lib.overlap.FragmentOverlap, in
 *   its row order and with its fragment offsets.  poses [B,12]: 3x4 row-major [R | t], fragment -> scene (the poses
 *   of mvr_sync_poses / mvr_posegraph_optimize).  member [B] (may be NULL: every fragment): 0 leaves a fragment out.
 *   Transform: every point of a member fragment b maps to q_d = R[d][0]*x + R[d][1]*y + R[d][2]*z + t_d in fp64;
 *   normals map by R only.
 *   Grid: lo_d = (min over all mapped member points of q_d) - voxel/2; voxel index floor((q_d - lo_d) / voxel), the
 *   expression of mvr_voxel_centroids.  Key: 21 bits per axis, (ix << 42) | (iy << 21) | iz.
 *   Range: the fp64 quotient is tested before the cast.  An index outside [0, 2^21) (a scene wider than about
 *   2,097,151.5 voxels along an axis: 52 km at voxel = 0.025) or a non-finite q makes the call return MVR_OK with
 *   *out_count = -1; the rows are then not meaningful, and nothing is written out of bounds (the convention of
 *   mvr_voxel_centroids' out_off[B]).  lib.multiview.fuse_scene raises ValueError on it.
 *   Output: one row per occupied voxel in ascending key order, *out_count = V (device scalar; no synchronisation).
 *   out_xyz [M,3] capacity: the fp64 sum of the voxel's mapped points in input order (ascending fragment, then
 *   ascending row: the stable sort keeps it) / their count.  out_n_points [M]: that count.  out_n_frags [M]: the
 *   number of distinct fragments among them (in that order: the fragment changes along the run, plus 1).
 *   out_normals [M,3] (required iff normals): the sum of the rotated normals in the same order / its Euclidean norm;
 *   an exactly zero sum gives (0, 0, 1), the convention of mvr_estimate_normals.  Normals are taken as given (not
 *   renormalised) and their ORIENTATION MATTERS: opposite normals of one surface cancel, so orient them, e.g. with
 *   the viewpoints of mvr_estimate_normals.
 *   Determinism: no floating-point atomics; a minimum is exact in any order and every sum is one thread's left fold,
 *   so the result is a function of the inputs alone, bit-identical from run to run.
 *   Launches: transform + partial minima, origin, keys, the radix sort (64 key bits: 1 clear, 1 histogram,
 *   8 passes), sorted keys, head flags, scan (3), run starts, count, one thread per occupied voxel over its run.
 *   M < 2^31; B is bounded by int only (the fragment is not in the key).
 *   MVR_EINVAL, scalars first: negative M; M >= 2^31; B <= 0; voxel not > 0; a NULL out_count.  M == 0 then returns
 *   MVR_OK with *out_count = 0 (the point arrays and the workspace may be NULL); member fragments without a point
 *   give 0 as well.  With M > 0: a NULL xyz, off, poses, workspace, out_xyz, out_n_points or out_n_frags,
 *   workspace_bytes < mvr_fuse_scene_workspace_bytes(M), or exactly one of normals / out_normals given.
 * ---------------------------------------------------------------------- */
size_t mvr_fuse_scene_workspace_bytes(int64_t M);
int mvr_fuse_scene(const double* xyz, const double* normals, const int64_t* off, int B, int64_t M,
                   const double* poses, const uint8_t* member, double voxel, void* workspace, size_t workspace_bytes,
                   double* out_xyz, double* out_normals, int32_t* out_n_points, int32_t* out_n_frags,
                   int64_t* out_count, mvr_stream_t stream);

/* Farthest point sampling per fragment (Sampler 'fps', lib/layers.py:134-141 — pointnet2
 * furthest_point_sample semantics of oracle/fps.py: seed = first point, running min of squared
 * distances, first maximum on ties).  xyz [sum n][3] with fragment row offsets (device `offsets`
 * and the same values on the host, B+1 entries); idx_out [B][m] int64 global rows.  n >= m for
 * every fragment (MVR_EINVAL otherwise: FPS draws m distinct points).  Limit: n <= 81,920 points per fragment
 * (512 threads x 160 running distances in registers, the largest instance); a larger fragment is MVR_EINVAL.
 * The kernel is chosen by the largest fragment of the batch and smaller fragments ride in it. */
int mvr_fps(const float* xyz, const int64_t* offsets, const int64_t* offsets_host, int B, int m, int64_t* idx_out,
            mvr_stream_t stream);

/* Coordinate-space nearest neighbour, knn_point(k=1, pos1, pos2) (lib/utils.py:274-299): for batch row b and
 * query i of pos2 ([B][M] rows of 3 floats at pos2 + b*p2_bstride + i*p2_rstride), the nearest of the N rows of
 * pos1 under the reference's fp32 squared distance ((dx^2 + dy^2) + dz^2, no contraction); first index on equal
 * distances.  dist_out [B][M] (may be NULL), idx_out [B][M] int64 (may be NULL, not both).  Row strides >= 3. */
int mvr_knn1(const float* pos1, int64_t p1_bstride, int64_t p1_rstride, const float* pos2, int64_t p2_bstride,
             int64_t p2_rstride, int B, int N, int M, float* dist_out, int64_t* idx_out, mvr_stream_t stream);

/* Mutual nearest-neighbour flag of the soft matches, extract_mutuals (lib/utils.py:822-848): j = knn1 of x1m[b,i]
 * among x2[b, 0..N), flag_out[b*N + i] = |x1[b,i] - x2m[b,j]|^2 < thr2 ? 1 : 0 (thr2 = threshold^2 rounded to
 * fp32, as the reference's float32 comparison does).  idx_out [B][N] (may be NULL) receives j. */
int mvr_mutuals(const float* x1, int64_t x1_bstride, int64_t x1_rstride, const float* x2, int64_t x2_bstride,
                int64_t x2_rstride, const float* x1m, int64_t x1m_bstride, int64_t x1m_rstride, const float* x2m,
                int64_t x2m_bstride, int64_t x2m_rstride, int B, int N, float thr2, float* flag_out, int64_t* idx_out,
                mvr_stream_t stream);

/* ------------------------------------------------------------------------
 * Feature-space (soft) nearest neighbour for a batch of fragment pairs.
 * Replaces lib/layers.py:44-88 Soft_NN.forward (+ pairwise_distance
 * lib/utils.py:968-992, the pair gather lib/utils.py:850-885 and the xs
 * assembly lib/utils.py:915).  For pair p = (s, t) = pairs[2p], pairs[2p+1]:
 *   queries Fq[s*fq_fstride + n*32 + c], targets Ft[t*ft_fstride + m*32 + c],
 *   target coords Xt[t*xt_fstride + m*3 + k]  (n < Nq, m < Mt, C must be 32);
 * mode 0: x_corr = softmax_m((2 fq.ft - |ft|^2) * inv_tau2) . Xt   ('soft')
 * mode 1: x_corr = Xt[argmax_m(fq.ft*2 - |ft|^2)]                   ('soft'+st, 'hard')
 * out(p,n,:) = [Xq(s,n,0..2) (if Xq != NULL) | x_corr(0..2)] at
 * out[p*out_pstride + n*out_nstride]; idx_out [P][Nq] argmax (mode 1, may be NULL).
 * ---------------------------------------------------------------------- */
int mvr_feat_nn(const float* Fq, int64_t fq_fstride, const float* Ft, int64_t ft_fstride, const float* Xq,
                int64_t xq_fstride, const float* Xt, int64_t xt_fstride, const int64_t* pairs, int P, int Nq, int Mt,
                int C, float inv_tau2, int mode, float* out, int64_t out_pstride, int64_t out_nstride,
                int32_t* idx_out, mvr_stream_t stream);
/* mvr_feat_nn with a workspace (mvr_feat_nn_workspace_bytes(n_frag, Mt), 16-byte aligned): the soft fast path then
 * splits the target fragments' features once per call into an image of its LDS stages (Ft holds n_frag fragments of
 * Mt targets; every pair's target index < n_frag) and stages them by LDS-DMA.  Results identical to mvr_feat_nn. */
size_t mvr_feat_nn_workspace_bytes(int n_frag, int Mt);
int mvr_feat_nn_ws(const float* Fq, int64_t fq_fstride, const float* Ft, int64_t ft_fstride, const float* Xq,
                   int64_t xq_fstride, const float* Xt, int64_t xt_fstride, const int64_t* pairs, int P, int Nq,
                   int Mt, int C, float inv_tau2, int mode, float* out, int64_t out_pstride, int64_t out_nstride,
                   int32_t* idx_out, int n_frag, void* workspace, size_t workspace_bytes, mvr_stream_t stream);

/* soft_gumbel correspondences (lib/layers.py:72-78: F.gumbel_softmax(-dist, tau, hard) . y_c): mvr_feat_nn's pairs
 * and layouts, x_corr = softmax((2 fq.ft - |ft|^2 + g) * inv_tau) . Xt (hard = 0) or Xt[argmax of the same noisy
 * logits] (hard = 1: the straight-through forward value; idx_out receives the index), with g = -ln(-ln u) per (query,
 * target) and u a counter-based hash of (seed, pairs[2p], pairs[2p+1], query, target) — reproducible across batch
 * shapes (oracle/soft_nn.py restates it); not torch's Philox stream. */
int mvr_feat_nn_gumbel(const float* Fq, int64_t fq_fstride, const float* Ft, int64_t ft_fstride, const float* Xq,
                       int64_t xq_fstride, const float* Xt, int64_t xt_fstride, const int64_t* pairs, int P, int Nq,
                       int Mt, int C, float inv_tau, int hard, uint64_t seed, float* out, int64_t out_pstride,
                       int64_t out_nstride, int32_t* idx_out, mvr_stream_t stream);

/* Two nearest neighbours in feature space (scripts/extract_data.py:178-184, sklearn NearestNeighbors
 * kneighbors(n_neighbors=2), Euclidean): for pair p and query j of fragment pairs[2p] (Fq rows, fragment stride
 * fq_fstride), idx2_out[(p*Nq + j)*2 + k] = k-th nearest row of fragment pairs[2p+1] (Ft, Mt >= 2 rows),
 * smallest distance first, first index on ties (split-bf16 MFMA distances; fp32-level near-ties may order
 * differently from fp64).  dist2_out (may be NULL): the fp64 distances of those two rows.  C == 32. */
int mvr_feat_knn2(const float* Fq, int64_t fq_fstride, const float* Ft, int64_t ft_fstride, const int64_t* pairs,
                  int P, int Nq, int Mt, int C, int32_t* idx2_out, double* dist2_out, mvr_stream_t stream);

/* Row gather dst[i][:] = src[idx[i]][:] (C floats per row): the Sampler's
 * index_select (lib/layers.py:151-152) with host-drawn (np.random) indices. */
int mvr_gather_rows(const float* src, int C, const int64_t* idx, int n, float* dst, mvr_stream_t stream);

/* ------------------------------------------------------------------------
 * Sparse-voxel primitives of the FCGF descriptor (MinkowskiEngine 0.4 calls in
 * lib/descriptor/fcgf.py, scripts/pairwise_demo.py:79-93, scripts/utils.py:102-120).
 * coords are int32 [M][4] = (batch, x, y, z); hash tables are opaque device
 * buffers of mvr_hash_table_bytes(M) bytes.
 * ---------------------------------------------------------------------- */
size_t mvr_hash_table_bytes(int64_t M);
size_t mvr_voxelize_workspace_bytes(int64_t n);
/* ME.utils.sparse_quantize(floor(xyz/voxel), return_index=True) per fragment, batched:
 * fragment b owns points [frag_off[b], frag_off[b+1]).  floor((double)x / voxel) in float64 with a correctly
 * rounded division — the reference's numpy arithmetic on Open3D's float64 points (scripts/utils.py:108-109).  Writes the unique voxels in
 * first-occurrence order: coords_out [n][4] (first count rows valid), sel_out [n]
 * (source point index), counts_out int64 [1+B] = {total, per-fragment}. */
int mvr_voxelize(const float* xyz, const int64_t* frag_off, int B, int64_t n, double voxel, void* workspace,
                 size_t workspace_bytes, int32_t* coords_out, int64_t* sel_out, int64_t* counts_out,
                 mvr_stream_t stream);
/* mvr_voxelize over float64 points (the caller's float64 array floored as it is: scripts/utils.py:108-109 applies
 * np.floor to Open3D's float64 points; no float32 rounding first).  Same workspace size, outputs and order. */
int mvr_voxelize_f64(const double* xyz, const int64_t* frag_off, int B, int64_t n, double voxel, void* workspace,
                     size_t workspace_bytes, int32_t* coords_out, int64_t* sel_out, int64_t* counts_out,
                     mvr_stream_t stream);
/* mvr_voxelize for a hinted voxel count (distinct_hint: the expected voxels of the whole batch).  Each fragment's
 * keys are split into hash buckets sized so that the mean fragment's share of the hint fills half of a workgroup's
 * LDS table; a bucket with more voxels than its table takes, or a coordinate outside the keys' 17-bit range, sets
 * counts_out[B + 1] (counts_out has B + 2 entries): the caller then re-runs mvr_voxelize.  Otherwise the same
 * outputs as mvr_voxelize. */
size_t mvr_voxelize_hint_workspace_bytes(int64_t n, int64_t distinct_hint);
int mvr_voxelize_hint(const float* xyz, const int64_t* frag_off, int B, int64_t n, double voxel,
                      int64_t distinct_hint, void* ws, size_t ws_bytes, int32_t* coords_out, int64_t* sel_out,
                      int64_t* counts_out, mvr_stream_t stream);
size_t mvr_coords_downsample_workspace_bytes(int64_t M);
/* strided coordinate set floor(c/s)*s (first-occurrence order); counts_out as above */
int mvr_coords_downsample(const int32_t* coords, int64_t M, int B, int stride_out, void* workspace,
                          size_t workspace_bytes, int32_t* coords_out, int64_t* counts_out, mvr_stream_t stream);
int mvr_hash_build(const int32_t* coords, int64_t M, void* table, size_t table_bytes, mvr_stream_t stream);
/* the same for a coordinate set on the lattice of `stride` (a power of two: every coordinate a multiple of it, the
 * tensor stride of an FCGF level): the 2x2x2 cells of that lattice share one 8-slot bucket of the table, so a kernel
 * map's stencil probes read a few runs instead of scattered slots (MinkowskiEngine's CoordinateManager keeps one map
 * per tensor stride likewise, fcgf.py:118-227).  Same lookups and results as mvr_hash_build. */
int mvr_hash_build_lattice(const int32_t* coords, int64_t M, int stride, void* table, size_t table_bytes,
                           mvr_stream_t stream);
/* kernel map as a neighbour table nbr[o][k] (k = (dx+r) + ks(dy+r) + ks^2(dz+r)):
 * row of out_coords[o] + sign*off_k*step in the input table (sign -1 if transposed), or -1 */
int mvr_kernel_map(const int32_t* out_coords, int64_t Mout, const void* in_table, size_t in_table_bytes, int ksize,
                   int step, int transposed, int32_t* nbr, mvr_stream_t stream);
/* mvr_kernel_map visiting the output rows in row_order (int32 [Mout], a permutation; NULL: row order) — the same
 * table; a spatial order (mvr_kernel_map_orders with nbr NULL) makes the workgroups that run together probe
 * neighbouring cells of the input table */
int mvr_kernel_map_x(const int32_t* out_coords, int64_t Mout, const void* in_table, size_t in_table_bytes, int ksize,
                     int step, int transposed, int32_t* nbr, const int32_t* row_order, mvr_stream_t stream);
/* 3^3 map of a set onto itself (out set == the table's set in row order: FCGF's stride-1 convs), equal to
 * mvr_kernel_map(coords, M, table, ..., 3, step, 0, nbr): half the offsets are probed, each hit also writes its mirror
 * entry (neighbour 26 - k of i is o when neighbour k of o is i), the centre is the row itself. */
int mvr_kernel_map_sym(const int32_t* coords, int64_t M, const void* table, size_t table_bytes, int step, int32_t* nbr,
                       mvr_stream_t stream);
/* dst [Md][K] = the transpose of src [Ms][K]: dst[i][k] = o where src[o][k] = i, else -1.  The transposed stride-2
 * conv's map between two sets (mvr_kernel_map(..., transposed = 1)) is the transpose of the strided conv's map between
 * them (FCGF's up maps from its down maps). */
int mvr_kernel_map_transpose(const int32_t* src, int64_t Ms, int K, int32_t* dst, int64_t Md, mvr_stream_t stream);
/* Row order of a kernel map: output rows sorted by their active-offset mask (K <= 27), so that a
 * tile of consecutive rows shares its active offsets; with out_coords (int32 [Mout][4], the map's output
 * coordinates, multiples of step) rows of one mask are further ordered by fragment and Morton code of
 * coordinates / step (spatially compact tiles: L2 reuse of the gathered rows).  Stable: ties keep row order.
 * A hand-written onesweep LSD radix sort (csrc/radix.hip: a control-block clear, one histogram launch, one launch
 * per 8-bit digit).  Workspace: mvr_kernel_map_order_bytes(Mout). */
size_t mvr_kernel_map_order_bytes(int64_t Mout);
int mvr_kernel_map_order(const int32_t* nbr, const int32_t* out_coords, int step, int64_t Mout, int K, int32_t* perm,
                         void* workspace, size_t workspace_bytes, mvr_stream_t stream);
/* The row orders of n_maps (<= 16) kernel maps in ONE sort (the map index in the top key bits): host arrays
 * nbr[j] (int32 [Mo[j]][K]), out_coords[j] (or out_coords NULL: masks only) with steps[j]; perm_out int32
 * [sum Mo]: map j's order (local row indices, exactly mvr_kernel_map_order's) at offset Mo[0] + ... + Mo[j-1].
 * Workspace: mvr_kernel_map_orders_bytes(sum Mo).  (FCGF: all ten 3^3 maps of a scene, lib/sparse.py
 * CoordinateManager.prepare_orders.)  nbr NULL with K = 0: coordinate sets only (out_coords required) — each
 * set's rows in (fragment, Morton code of coordinates / step) order, stable (the kernel maps' visiting order). */
size_t mvr_kernel_map_orders_bytes(int64_t total);
int mvr_kernel_map_orders(int n_maps, const int32_t* const* nbr, const int32_t* const* out_coords, const int* steps,
                          const int64_t* Mo, int K, int32_t* perm_out, void* workspace, size_t workspace_bytes,
                          mvr_stream_t stream);
/* The same stable radix sort on its own: values int32 [n] (NULL: 0..n-1) in ascending order of the key bits
 * [0, bits) of keys uint64 [n] -> vals_out.  Workspace: mvr_radix_sort_pairs_bytes(n). */
size_t mvr_radix_sort_pairs_bytes(int64_t n);
int mvr_radix_sort_pairs(const uint64_t* keys, const int32_t* vals, int64_t n, int bits, int32_t* vals_out,
                         void* workspace, size_t workspace_bytes, mvr_stream_t stream);
/* MinkowskiConvolution forward, gather-GEMM over the neighbour table (nbr NULL & K==1:
 * identity map, i.e. a 1x1x1 conv); W [K][Cin][Cout]; epilogue (+bias[Cout]) ->
 * BatchNorm eval (bn.gamma NULL: none) -> (+res[o*ldres+c]) -> ReLU if relu.
 * perm (optional): order in which output rows are tiled (mvr_kernel_map_order); results are
 * written to their own rows either way.
 * wimg (required, 16-byte aligned): the weights pre-split by mvr_spconv_wimage -> split-bf16 MFMA path
 * (fp32-level accuracy, ~2.7x the exact-fp32 MFMA rate).  Cin a multiple of 32 (every FCGF conv), Cout and ldin
 * multiples of 4, in and W 16-byte aligned; MVR_EINVAL otherwise.
 * range_flag (optional, device int32 owned by the stream's call sequence): enables the split-fp16 pass when
 * mvr_set_math(1) (the flag is cleared by the call, set by a split-fp16 pass whose operands left the fp16
 * window, and read by its guarded split-bf16 re-run); NULL -> split-bf16 only.  out is either disjoint from res
 * or equal to it (in place). */
int mvr_spconv(const float* in, int64_t ldin, int Cin, const int32_t* nbr, const int32_t* perm, int K, int64_t Mout,
               const float* W, int Cout, const float* bias, mvr_bn_p bn, float bn_eps, const float* res,
               int64_t ldres, int relu, float* out, int64_t ldout, const void* wimg, int32_t* range_flag,
               mvr_stream_t stream);
/* mvr_spconv with split-bf16 planes beside the fp32 buffers (FCGF: every conv's output feeds the next conv's
 * gathers).  in_planes (optional, 16-byte aligned, ldin % 8 == 0): the input's (h, m, l) bf16 planes, row r plane p
 * at in_planes + (3 r + p) ldin — the split the kernel would otherwise repeat for each of a row's ~14 gathers; the
 * split-bf16 pass gathers them instead of `in` (bit-identical results; a split-fp16 pass still reads `in`).
 * out_planes (optional): also write the output's planes, row r plane p at out_planes + (3 r + p) ldout. */
int mvr_spconv_x(const float* in, int64_t ldin, int Cin, const int32_t* nbr, const int32_t* perm, int K, int64_t Mout,
                 const float* W, int Cout, const float* bias, mvr_bn_p bn, float bn_eps, const float* res,
                 int64_t ldres, int relu, float* out, int64_t ldout, const void* wimg, int32_t* range_flag,
                 const uint16_t* in_planes, uint16_t* out_planes, mvr_stream_t stream);
/* Weight image of mvr_spconv's split paths: W [K][Cin][Cout] fp32 -> three bf16 planes in
 * [K][ceil(Cin/32)][plane][round_up(Cout,128)][40] rows (80-byte rows, zero padded), then the same rows as two
 * fp16 planes of W[.][.][c] s_c (s_c: a power of two bringing output channel c's weights to <= 2^14), then
 * s_c and 1 / (s_c 2^6) per channel. */
size_t mvr_spconv_wimage_bytes(int K, int Cin, int Cout);
int mvr_spconv_wimage(const float* W, int K, int Cin, int Cout, void* img, size_t bytes, mvr_stream_t stream);
/* Brick map of a coordinate set (4x4x4 bricks: hash of brick coordinates -> 64 row slots), the
 * neighbourhood structure of the large-stencil conv below.  Workspace:
 * mvr_brick_map_bytes(M).  _stride: a set at tensor stride `stride` (a power of two, coordinates multiples of it):
 * cells are coordinates / stride; mvr_brick_map_build = stride 1. */
size_t mvr_brick_map_bytes(int64_t M);
int mvr_brick_map_build(const int32_t* coords, int64_t M, void* workspace, size_t workspace_bytes,
                        mvr_stream_t stream);
int mvr_brick_map_build_stride(const int32_t* coords, int64_t M, int stride, void* workspace, size_t workspace_bytes,
                               mvr_stream_t stream);
/* single-input-channel conv with a large stencil (FCGF conv1, 7^3) over the input set's brick map
 * (in_bricks built from the Min input coordinates; input cell = coordinate / step).
 * out_coords NULL: the output set is the input set itself (Mout == Min, step 1, ksize 7; output row o =
 * input row o) — computed brick by brick as dense 7^3 windows on split-bf16 MFMA. */
int mvr_spconv_c1(const int32_t* out_coords, int64_t Mout, const void* in_bricks, int64_t Min, size_t in_bricks_bytes,
                  const float* feat, int ksize, int step, const float* W, int Cout, mvr_bn_p bn, float bn_eps,
                  int relu, float* out, int64_t ldout, mvr_stream_t stream);
/* mvr_spconv_c1 (brick path, out_coords NULL) also writing the output's split-bf16 planes (mvr_spconv_x's layout) */
int mvr_spconv_c1_x(const int32_t* out_coords, int64_t Mout, const void* in_bricks, int64_t Min,
                    size_t in_bricks_bytes, const float* feat, int ksize, int step, const float* W, int Cout,
                    mvr_bn_p bn, float bn_eps, int relu, float* out, int64_t ldout, uint16_t* out_planes,
                    mvr_stream_t stream);
/* x[o][:C] /= ||x[o][:C]||  (fcgf.py:274-278) */
int mvr_l2norm_rows(float* x, int64_t M, int C, int64_t ld, mvr_stream_t stream);

/* Sampler 'rand' (lib/layers.py:145-148) on the host: for each fragment b in order,
 * np.random.choice(arange(start_b, start_b + counts[b]), tgt, replace=False) drawn from numpy's
 * legacy MT19937 RandomState (key uint32[624] and *pos as np.random.get_state() gives them; advanced
 * in place for np.random.set_state()).  out int64 [B][tgt]; ws int64 scratch of max(counts).
 * Requires tgt <= counts[b].  Host-only (no device work, no stream). */
int mvr_sample_rand_mt19937(uint32_t* key, int32_t* pos, const int64_t* counts, int B, int tgt, int64_t* out,
                            int64_t* ws);

/* Opt-in per-kernel-class device timing (hipEvents on the launching stream).
 * mvr_prof_set(1) resets and enables; mvr_prof_get(kind, ...) synchronises the
 * recorded events and returns totals since then (kinds: csrc/prof.hpp ProfKind). */
int mvr_prof_set(int on);
/* kinds that get event records while enabled: bit k = kind k (default: all) */
int mvr_prof_mask(unsigned mask);
int mvr_prof_get(int kind, double* ms, long long* launches, double* flops, double* bytes);
/* launch order since mvr_prof_set(1): kind and algorithmic bytes per profiled launch (<= cap);
 * returns the count (joins rocprofv3 PMC dispatch rows to kernel classes) */
int mvr_prof_seq(int* kinds, double* bytes, int cap);
/* the library's source identity (sha256 prefix of its sources + variant flags) as a NUL-terminated string: MVR_OK,
 * or the buffer size needed when cap is too small (bench.py uses the PMC counters only of this same build) */
int mvr_source_hash(char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif
