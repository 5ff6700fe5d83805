/*
 * sgm_hip_icp.h -- rigid registration of two point clouds on the device: the rigid motion T that lays a source cloud on a target
 * cloud by iterated closest points, the share of the source that finds a partner (fitness) and how far those pairs are apart
 * (inlier rmse), so that two clouds -- a rig that moved between pairs, a second pair of the same scene, a cloud read from a file --
 * can be merged, the rig's motion read off, or a model compared with a scan.  Every other cloud call works on one cloud; this one
 * joins two.  Included by sgm_hip.h: a caller includes that header and gets this one with it.
 *
 * It is a file of its own for the reason sgm_hip_confidence.h gives: the entry points sgm_hip.h and the headers before this one
 * declare are held, symbol for symbol, against lists fixed earlier; these are bound beside them (_lib.py: ICP_EXPORTS).
 *
 * In user code the place of these calls is usually taken by Open3D's registration_icp and evaluate_registration.  This is
 * NOT Open3D's function: it is the definition below, our own.  The differences: the correspondence tie rule (equal binary32
 * distances go to the lowest target index); the range rule (step 3 of sgm_hip_radius.h for the target, and for every transformed
 * source point); point-to-point is solved by the same Gauss-Newton step as point-to-plane, not by Umeyama's closed form; the update
 * is a quaternion (1, a/2, b/2, c/2) divided by its squared norm, not a product of Euler angle rotations; and every sum is taken in
 * one fixed pairwise tree, so the same bits come out on every run.
 *
 * Definition.
 *
 * Inputs: source xyz_s float32 [ns][3] and target xyz_t float32 [nt][3], each with disp float32 [n] or null; normals_t float32
 * [nt][3] or null; r = max_correspondence_distance, binary32; origin o[3], float32, finite; T0 double [16], row-major; estimation, 0
 * for point-to-point and 1 for point-to-plane; max_iteration, 0 .. 1000; relative_fitness and relative_rmse, doubles >= 0.
 * ns, nt <= 2^24 - 1, as in sgm_hip_radius.h; a larger one is SGM_ERR_UNSUPPORTED.  Refused with SGM_ERR_INVALID_ARG and every
 * output untouched: a T0 with an entry that is not finite or a last row other than (0, 0, 0, 1); estimation = 1 with null
 * normals; an r that step 2 of sgm_hip_radius.h refuses.
 *
 *   1. Target grid.  Steps 1 to 3 of sgm_hip_radius.h on the target with radius r and origin o: validity, the host constants r2, v,
 *      inv, and the range rule.  Target points that are not valid or out of range are nobody's partner.  Source validity is step 1
 *      of that header; m_s is the number of valid source points.
 *   2. Transform.  M is the 12 entries of the first three rows of the current T, each rounded to binary32.  For a valid source point
 *      (x, y, z):  p'_x = fmaf(M02, z, fmaf(M01, y, fmaf(M00, x, M03))) and likewise p'_y from row 1 and p'_z from row 2: three
 *      fused multiply-adds in binary32 per coordinate, starting from the translation, as in step 5 of sgm_hip_plane.h.  A valid
 *      source point whose p' has a coordinate that is not finite, or is out of range (step 3 of sgm_hip_radius.h applied to p'),
 *      is UNPLACED: it has no correspondence, and it is counted.
 *   3. Correspondence.  Among the in-range target points j, d2(p', q_j) is step 4 of sgm_hip_radius.h with dx = q_x - p'_x,
 *      dy = q_y - p'_y, dz = q_z - p'_z:  d2 = (dx * dx + dy * dy) + dz * dz in binary32, nothing fused.  The correspondence of
 *      source point i is the j with the smallest d2 among those with d2 <= r2 (inclusive); ties in the binary32 d2 go to the lowest
 *      target index.  corr[i] = j, or -1 if there is none (also for the points that are not valid or unplaced).  The statement is
 *      over all in-range target points.  The lemma of sgm_hip_radius.h is about any two in-range points p, q with d2 <= r2 -- its
 *      proof uses nothing but that both satisfy the range rule, not that both are records of the grid -- so it holds for a placed
 *      p' and a target point, and the 27 cells around the cell of p' suffice.
 *   4. Terms, per source point, in binary64 from the binary32 values, every operation rounded on its own, nothing fused.  With
 *      p = p' and q the partner:  d_x = p_x - q_x, d_y = p_y - q_y, d_z = p_z - q_z.  The 28 terms s_0 .. s_27 are the upper
 *      triangle of a symmetric 6 x 6 matrix in row order (s_0 .. s_5 row 0, s_6 .. s_10 row 1 from the diagonal, s_11 .. s_14,
 *      s_15 .. s_17, s_18, s_19, s_20), the right-hand side s_21 .. s_26, and s_27 = d2 of step 3 converted to binary64.
 *      Point-to-plane (estimation 1).  The partner's normal n is USABLE iff its three components are finite and
 *      (n_x * n_x + n_y * n_y) + n_z * n_z, in binary32, lies in [0.25, 4] -- which excludes the (0, 0, 0) sgm_covariance_normals
 *      returns for a point without a normal.  With a usable normal:  e = (n_x * d_x + n_y * d_y) + n_z * d_z;  the row
 *      a = (p_y * n_z - p_z * n_y,  p_z * n_x - p_x * n_z,  p_x * n_y - p_y * n_x,  n_x,  n_y,  n_z), each of the first three two
 *      products and a difference;  the matrix entry (j, k) is a_j * a_k, one product;  s_{21 + j} = -(a_j * e).  A correspondence
 *      with an unusable normal counts for fitness and rmse (s_27 = d2) but contributes +0.0 to s_0 .. s_26, and it is counted.
 *      Point-to-point (estimation 0).  The three rows [-[p]x | I] with the residual d give
 *        s_0 = p_y * p_y + p_z * p_z   s_1 = -(p_x * p_y)   s_2 = -(p_x * p_z)   s_3 = 0    s_4 = -p_z   s_5 = p_y
 *        s_6 = p_x * p_x + p_z * p_z   s_7 = -(p_y * p_z)   s_8 = p_z   s_9 = 0   s_10 = -p_x
 *        s_11 = p_x * p_x + p_y * p_y   s_12 = -p_y   s_13 = p_x   s_14 = 0
 *        s_15 = 1   s_16 = 0   s_17 = 0   s_18 = 1   s_19 = 0   s_20 = 1
 *        s_21 = -(p_y * d_z - p_z * d_y)   s_22 = -(p_z * d_x - p_x * d_z)   s_23 = -(p_x * d_y - p_y * d_x)
 *        s_24 = -d_x   s_25 = -d_y   s_26 = -d_z
 *      (every 0 above is +0.0).  A source point without a correspondence contributes +0.0 to all 28.
 *   5. Tree sum.  Each of the 28 sums over i = 0 .. ns - 1 is taken in the canonical pairwise tree: the ns terms in source order are
 *      padded with +0.0 to the next power of two, then s[k] = s[2k] + s[2k + 1] is repeated until one value is left.  No atomics;
 *      the result does not depend on how the device is launched.  n_corr, the number of correspondences, is an integer count.
 *   6. Solve (host, binary64, fixed order; sgm_icp_solve).  A x = b with A the symmetric matrix of s_0 .. s_20 and b = s_21 .. s_26
 *      by LDL^T without pivoting.  For j = 0 .. 5:  v_k = L_jk * D_k for k = 0 .. j - 1;  D_j = A_jj - L_j0 * v_0 - ... (the products
 *      subtracted one after the other in ascending k);  then for i = j + 1 .. 5:  L_ij = (A_ij - L_i0 * v_0 - ...) / D_j, likewise.
 *      A pivot D_j that is not finite or not > 0 is the status DEGENERATE, and T stays as it was.  Then y_i = b_i - L_i0 * y_0 - ...
 *      (ascending k < i) for i = 0 .. 5;  z_i = y_i / D_i;  x_i = z_i - L_{i+1,i} * x_{i+1} - ... (ascending k > i) for i = 5 .. 0.
 *      A solution with an entry that is not finite is DEGENERATE as well.
 *   7. Update.  (alpha, beta, gamma, t_x, t_y, t_z) = x.  The quaternion is (1, qx, qy, qz) = (1, alpha * 0.5, beta * 0.5,
 *      gamma * 0.5);  nn = ((1 + qx * qx) + qy * qy) + qz * qz;  its rotation matrix with the division by the squared norm written
 *      out, + - * / only, no sin, cos or sqrt:
 *        R00 = (((1 + qx * qx) - qy * qy) - qz * qz) / nn   R01 = (2 * (qx * qy - qz)) / nn   R02 = (2 * (qx * qz + qy)) / nn
 *        R10 = (2 * (qx * qy + qz)) / nn   R11 = (((1 - qx * qx) + qy * qy) - qz * qz) / nn   R12 = (2 * (qy * qz - qx)) / nn
 *        R20 = (2 * (qx * qz - qy)) / nn   R21 = (2 * (qy * qz + qx)) / nn   R22 = (((1 - qx * qx) - qy * qy) + qz * qz) / nn
 *      dT = [R | t] and T <- dT * T as a plain triple loop: for i, j in 0 .. 2 / 0 .. 3 the entry is
 *      ((dT_i0 * T_0j + dT_i1 * T_1j) + dT_i2 * T_2j) + dT_i3 * T_3j, from the left.  The last row is kept exactly (0, 0, 0, 1).
 *   8. Loop and stop.  Steps 2 to 5 under T0 are evaluation 0:  fitness = n_corr / m_s in binary64 (0 for m_s = 0),
 *      rmse = sqrt(s_27 / n_corr) (0 for n_corr = 0);  history row 0 is (fitness, rmse).  Then, repeatedly: if n_corr < 6, stop with
 *      status TOO FEW;  if max_iteration iterations are done, stop with status MAX ITERATION;  steps 6 and 7 -- degenerate: stop
 *      with that status --;  evaluate again and record the next history row;  stop as CONVERGED when |fitness - previous fitness| <
 *      relative_fitness and |rmse - previous rmse| < relative_rmse.  max_iteration = 0 is the evaluation alone and equals
 *      sgm_evaluate_registration.  The reported T, fitness, rmse, corr and d2 all belong to the last evaluation.
 *   9. Outputs.  out_T double [16];  out_fitness, out_rmse;  out_corr int32 [ns];  out_d2 float32 [ns], the d2 of step 3 and the
 *      quiet NaN 0x7FC00000 where there is no correspondence;  out_history double [max_iteration + 1][2], the rows past the last
 *      evaluation left as they were;  out_stats uint64 [8]: m_s, target points in range, valid target points out of range,
 *      iterations done, final n_corr, final unplaced count, final unusable-normal count, status (0 converged, 1 max_iteration,
 *      2 too few, 3 degenerate).  Any output may be null.  nt = 0 is a target with nothing in range.  ns = 0 succeeds without
 *      touching the device: T = T0, fitness 0, rmse 0, history row 0 = (0, 0), status 2, the other stats 0.
 *
 * Every result is a function of integer counts, fixed-order binary32 and binary64 arithmetic and the tree: the same bits come out on
 * every run.  tests/icp_ref.py restates the definition in numpy, the correspondence over all pairs and over 27 cells, the solve and
 * the update in plain Python floats; the device results equal it bit for bit, and sgm_icp_solve equals it bit for bit without a GPU.
 * Only + - * and conversions run on the device in binary64; every division and the square root run on the host.
 *
 * Cost.  An evaluation walks the 27 cells around every placed source point with no early stop: its work is the number of
 * candidates in those cells.  Thin both clouds first (sgm_voxel_downsample) and register at a few voxel sizes.  Not offered:
 * point-to-plane with source normals, colour terms, a robust kernel, a global initialisation, a multi-scale schedule, a batch form
 * and an asynchronous form.
 */
#ifndef SGM_HIP_ICP_H
#define SGM_HIP_ICP_H

#include "sgm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host pointers, blocking.  out_corr and out_d2 have ns entries, out_history max_iteration + 1 rows of 2.  Any output may be null.
 * SGM_ERR_INVALID_ARG, with every output untouched and an sgm_last_error that names the entry, for a null e / xyz_s (with ns > 0) /
 * xyz_t (with nt > 0) / origin / T0, ns < 0 or nt < 0, what the definition refuses, an estimation that is neither 0 nor 1, a
 * max_iteration outside 0 .. 1000, a threshold that is negative or NaN; SGM_ERR_UNSUPPORTED for ns or nt > 2^24 - 1.
 * The engine reuses the radius search's buffers for the target's grid and keeps 8 bytes per source point (corr, d2), 224 bytes per
 * 256 source points (the blocks' partial sums) and, for the host entries, the staged target; sgm_trim gives them back.  With
 * SGM_OPT_PROFILE = 1 the stage record (sgm_get_stage_times) is afterwards the target grid's and the LAST evaluation's: icp_count,
 * icp_clear, icp_insert, icp_starts, icp_sort, icp_correspond, icp_terms, icp_reduce. */
int sgm_register_icp(sgm_engine *e, const float *xyz_s, const float *disp_s, int64_t ns, const float *xyz_t, const float *disp_t,
                     const float *normals_t, int64_t nt, float max_correspondence_distance, const float origin[3], const double T0[16],
                     int estimation, int max_iteration, double relative_fitness, double relative_rmse, double out_T[16],
                     double *out_fitness, double *out_rmse, int32_t *out_corr, float *out_d2, double *out_history, uint64_t out_stats[8]);

/* The same with DEVICE pointers for the point data and the per-point outputs d_out_corr and d_out_d2, on the engine's stream; origin,
 * T0 and the small results are host pointers.  Blocks once for the number of target points in range, which sizes the table, as every
 * consumer of that grid does, and once per evaluation for the 28 sums and the count: the 232-byte record goes to page-locked
 * memory in one copy, which also carries the 16 bytes of the evaluation's other counts that lie behind the record.  Outputs must
 * not overlap inputs or each other. */
int sgm_register_icp_device(sgm_engine *e, const void *d_xyz_s, const void *d_disp_s, int64_t ns, const void *d_xyz_t, const void *d_disp_t,
                            const void *d_normals_t, int64_t nt, float max_correspondence_distance, const float origin[3],
                            const double T0[16], int estimation, int max_iteration, double relative_fitness, double relative_rmse,
                            double out_T[16], double *out_fitness, double *out_rmse, void *d_out_corr, void *d_out_d2,
                            double *out_history, uint64_t out_stats[8]);

/* Steps 1 to 5 and the two figures of step 8 alone under a caller's transform T: sgm_register_icp with max_iteration = 0 and
 * point-to-point terms, whose out_T would be T.  out_stats as above (status 1, or 2 with fewer than 6 correspondences). */
int sgm_evaluate_registration(sgm_engine *e, const float *xyz_s, const float *disp_s, int64_t ns, const float *xyz_t, const float *disp_t,
                              int64_t nt, float max_correspondence_distance, const float origin[3], const double T[16],
                              double *out_fitness, double *out_rmse, int32_t *out_corr, float *out_d2, uint64_t out_stats[8]);

/* The same with DEVICE pointers for the point data and d_out_corr, d_out_d2.  Blocks twice: for the grid's size and for the sums. */
int sgm_evaluate_registration_device(sgm_engine *e, const void *d_xyz_s, const void *d_disp_s, int64_t ns, const void *d_xyz_t,
                                     const void *d_disp_t, int64_t nt, float max_correspondence_distance, const float origin[3],
                                     const double T[16], double *out_fitness, double *out_rmse, void *d_out_corr, void *d_out_d2,
                                     uint64_t out_stats[8]);

/* Step 2 on a point list, so that a registered cloud can be merged with its target: out_xyz [n][3] = the points under T (every row,
 * valid or not: a NaN stays a NaN), and, with normals, out_normals [n][3] by the rotation part only, n'_x = fmaf(M02, n_z,
 * fmaf(M01, n_y, M00 * n_x)) and likewise.  normals and out_normals are both null or both given; out_xyz may be null.  T is checked
 * like T0.  The host entry blocks; outputs may be the inputs (in place). */
int sgm_transform_points(sgm_engine *e, const float *xyz, const float *normals, int64_t n, const double T[16], float *out_xyz,
                         float *out_normals);

/* The same with DEVICE pointers, on the engine's stream; does not block.  In place is allowed; otherwise nothing may overlap. */
int sgm_transform_points_device(sgm_engine *e, const void *d_xyz, const void *d_normals, int64_t n, const double T[16], void *d_out_xyz,
                                void *d_out_normals);

/* Steps 6 and 7 on the host alone: no engine, no GPU.  sums: the 28 of step 5; estimation: 0 or 1 (both forms share the solve);
 * T_out = dT * T_in and *status = 0, or T_out = T_in and *status = 3 (degenerate).  T_in and T_out may be the same array.
 * SGM_ERR_INVALID_ARG for a null pointer or another estimation. */
int sgm_icp_solve(const double sums[28], int estimation, double T_in[16], double T_out[16], int *status);

#ifdef __cplusplus
}
#endif
#endif
