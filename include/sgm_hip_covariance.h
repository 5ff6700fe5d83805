/*
 * sgm_hip_covariance.h -- covariance (PCA) normals for a point LIST on the device: per point the unit normal of the plane fitted
 * to its neighbours within a fixed radius -- the eigenvector of the smallest eigenvalue of their covariance matrix --, the surface
 * variation and the number of neighbours.  sgm_normals_grid and sgm_mesh_grid_normals (sgm_hip_normals.h) need the pixel grid and
 * its quads; this needs points only, so the centroids of sgm_voxel_downsample, a list cleaned by sgm_radius_outlier or
 * sgm_statistical_outlier, a cloud read back from a file or two pairs' clouds concatenated can have normals.  It runs on the grid
 * of cells of sgm_hip_radius.h.  Included by sgm_hip.h: a caller includes that header and gets this one with it.
 *
 * It is a file of its own for the reason sgm_hip_confidence.h gives: the entry points sgm_hip.h and the headers before this one
 * declare are held, symbol for symbol, against lists fixed earlier; these are bound beside them (_lib.py: COVARIANCE_EXPORTS).
 *
 * In user code the place of this call is usually taken by Open3D's estimate_normals(KDTreeSearchParamRadius(radius)) followed by
 * orient_normals_towards_camera_location.  This is NOT Open3D's function: it is the definition below, our own.  Ours never counts
 * the query point as a neighbour (it enters the moments as their tenth term), has the range rule of sgm_hip_radius.h, forms the
 * moments in integers from offsets quantised to radius / 32768, solves the 3 x 3 problem by six fixed Jacobi sweeps, and gives a
 * point with fewer than min_neighbors neighbours no normal at all.
 *
 * Definition.
 *
 * Inputs: xyz float32 [n][3]; disp float32 [n] or null; radius r, float32; min_neighbors k, 2 <= k <= 2^24 - 1; origin o[3],
 * float32, finite; viewpoint w[3], float32, finite; orient, 0 or 1.  n <= 2^24 - 1 points, as in sgm_hip_radius.h.
 *
 *   1 - 4. Validity, host constants, range and distance are steps 1 to 4 of sgm_hip_radius.h, word for word: r2 = r * r;
 *      v = r * 1.03125f;  inv = 1.0f / v, with the same refusals; cells of edge v anchored at o with indices in -2^16 .. 2^16 - 1;
 *      dx = x_j - x_i, dy, dz likewise and d2 = (dx * dx + dy * dy) + dz * dz in binary32, nothing fused.  One more host constant:
 *      qscale = 32768.0f / r, one binary32 division; an r whose qscale is not finite is refused.
 *   5. Neighbours.  For an in-range point i, N_i is the set of the in-range points j != i with d2 <= r2 (the test is inclusive,
 *      duplicates of point i count), and c_i = |N_i|.  Nothing stops the search early.  Point i HAS A NORMAL iff c_i >= k.
 *   6. Moments, in integers.  Per neighbour j and axis a: q_a = (int32)rintf(d_a * qscale) with d_a the binary32 difference of
 *      step 4 (dx, dy, dz); the product is one binary32 operation, the rounding is to nearest, ties to even.
 *      |q_a| <= 2^15 + 1: by (b) of the lemma of sgm_hip_radius.h a neighbour has |d_a| <= r (1 + 2^-21); qscale <= (2^15 / r)
 *      (1 + 2^-24) and the product rounds once, so |d_a * qscale| <= 2^15 (1 + 2^-21)(1 + 2^-24)^2 < 2^15 + 0.02, whose nearest
 *      integer is at most 2^15 + 1 (in fact 2^15).
 *      In signed 64-bit integers, over j in N_i:  S_a = sum q_a (three sums);  S_ab = sum q_a q_b for a <= b (six sums, in the
 *      order 00, 01, 02, 11, 12, 22).  |S_a| < 2^24 * 2^16 = 2^40 and |S_ab| < 2^24 * 2^31 = 2^55.  The point itself is one more
 *      term with offset 0, which changes no sum: m = c_i + 1 is the number of terms.
 *      Integer sums do not depend on the order of their terms.  That is the point of quantising: the rank of a record inside its
 *      cell comes from an atomic and differs from run to run, so a floating-point sum over the neighbours would not be reproducible.
 *   7. Covariance (times m), in binary64, every operation rounded on its own:
 *      C_ab = (double)S_ab - ((double)S_a * (double)S_b) / (double)m   for the six a <= b.
 *      The conversions from int64 round to nearest even (every value below 2^53 converts exactly).  s = max(C_00, C_11, C_22).
 *      If not s > 0 the point is DEGENERATE -- every neighbour sits on the point --: its normal is (0, 0, 0), its curvature -1,
 *      and it is counted.  Otherwise all six entries are divided by s: A = C / s, symmetric, a_ab for a <= b.
 *   8. Eigenvectors by cyclic Jacobi: V = I, then exactly 6 sweeps over (p, q) = (0,1), (0,2), (1,2), in this order.  A rotation
 *      with a_pq == 0 is skipped.  Otherwise, every product, sum, difference, quotient and square root a separate correctly
 *      rounded binary64 operation:
 *        theta = (a_qq - a_pp) / (2 * a_pq)
 *        t = sgn / (|theta| + sqrt(theta * theta + 1)),  sgn = +1 for theta >= 0 and -1 otherwise (an overflowing theta * theta
 *            gives t = +-0, which is right)
 *        c = 1 / sqrt(t * t + 1);   sn = t * c;   h = t * a_pq
 *        a_pp = a_pp - h;   a_qq = a_qq + h;   a_pq = 0
 *        for the third index r:  a_rp' = c * a_rp - sn * a_rq;   a_rq' = sn * a_rp + c * a_rq   (both from the old values)
 *        for each row i of V:    v_ip' = c * v_ip - sn * v_iq;   v_iq' = sn * v_ip + c * v_iq
 *   9. The normal.  i* = the index of the smallest diagonal entry a_ii, the lowest index among equals.  nv = column i* of V.
 *      len = sqrt((nv0 * nv0 + nv1 * nv1) + nv2 * nv2);  nv_a = nv_a / len.  With orient: w_a = (double)p_a - (double)viewpoint_a;
 *      if (nv0 * w0 + nv1 * w1) + nv2 * w2 > 0 the normal is negated, so that it points towards the viewpoint.  Without orient
 *      the sign is what the rotations left: deterministic, and without meaning.  Then each component is rounded to binary32.
 *  10. The curvature (surface variation).  l_a = max(a_aa, 0);  den = (l_0 + l_1) + l_2;  kappa = l_i* / den, and 0 if den is 0;
 *      rounded to binary32.  It lies in 0 .. 1/3: 0 on a plane, 1/3 where the neighbours spread alike in all directions.
 *  11. Outputs, all at the source index, nothing compacted.  out_normals float32 [n][3]: (0, 0, 0) where a point has no normal;
 *      out_curvature float32 [n]: -1 where a point has no normal; out_counts uint32 [n]: the full c_i, and 0 for the points in no
 *      cell; out_stats uint64 [4]: points in range, valid points out of range, points with a normal (degenerate ones not among
 *      them), degenerate points.
 *
 * The definition is grid-free like that of sgm_hip_radius.h, whose lemma makes the 27 cells around a point hold all of N_i.  Every
 * float result is a function of nine integer sums and a count: the same bits come out on every run.  tests/covariance_ref.py
 * restates the definition in numpy, over all pairs and over 27 cells; the device results equal it bit for bit.
 *
 * Accuracy.  The offsets are quantised to r / 32768: a neighbour moves by at most r / 65536 per axis before the plane is fitted,
 * which tilts the normal of a patch of extent r by an angle of the order of 2^-16 and less where many neighbours average it out
 * (tests/test_covariance_reference.py measures it against an unquantised binary64 PCA of the same neighbours).  The Jacobi sweeps
 * leave off-diagonals of exactly 0 on every neighbourhood tried; against LAPACK the eigenvalues agree to a few ulp.
 *
 * Cost.  The work of a call is the number of candidates in the 27 cells around each point, and nothing cuts it short.  A radius
 * that puts the whole cloud into a few cells is quadratic in n.  The radius should hold ten to a few tens of neighbours: for the
 * centroids of a voxel grid about twice the voxel size.  A fixed metric radius gives the far range of a stereo cloud, whose point
 * spacing grows with depth, fewer neighbours and so fewer normals; a radius scaled by depth, a k-nearest search, a batch form and
 * an asynchronous form are not offered.
 */
#ifndef SGM_HIP_COVARIANCE_H
#define SGM_HIP_COVARIANCE_H

#include "sgm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host pointers, blocking.  out_normals has n rows of 3, out_curvature and out_counts n entries, out_stats 4.  Any of the four may
 * be null.  SGM_ERR_INVALID_ARG, with the outputs untouched, for a null e / xyz, n < 0, a radius refused by step 2 of
 * sgm_hip_radius.h or with a qscale that is not finite, min_neighbors outside 2 .. 2^24 - 1, a null or non-finite origin or
 * viewpoint, an orient that is neither 0 nor 1; SGM_ERR_UNSUPPORTED for n > 2^24 - 1.  n = 0 succeeds with out_stats all zero.
 * SGM_ERR_HIP if a point found no slot in the table (a defect, never a hang: every probe is bounded by the table's capacity, and
 * nothing waits for anything).
 * The engine reuses the table, records and staging of sgm_radius_outlier and adds 12 + 4 bytes per point for the staged normals
 * and curvatures (and, with the solve as a kernel of its own, 80 bytes per point in range); sgm_trim gives them back.  With
 * SGM_OPT_PROFILE = 1 the stage record (sgm_get_stage_times) is the call's afterwards: cov_count, cov_clear, cov_insert,
 * cov_starts, cov_sort, cov_query (one launch, two where some point is in no cell and gets its zeros and -1 from a pass of its
 * own) and, where the solve is a kernel of its own (a debug switch), cov_solve. */
int sgm_covariance_normals(sgm_engine *e, const float *xyz, const float *disp, int64_t n, float radius, int min_neighbors,
                           const float origin[3], const float viewpoint[3], int orient,
                           float *out_normals, float *out_curvature, uint32_t *out_counts, uint64_t *out_stats);

/* The same with DEVICE pointers for the point data and the three per-point outputs, on the engine's stream; origin, viewpoint and
 * out_stats are host pointers.  Blocks once for the number of points in range, which sizes the table, and again at the end only if
 * out_stats is given: without it the outputs are complete when the stream has run (sgm_synchronize).  Outputs must not overlap
 * inputs or each other. */
int sgm_covariance_normals_device(sgm_engine *e, const void *d_xyz, const void *d_disp_f32, int64_t n, float radius, int min_neighbors,
                                  const float origin[3], const float viewpoint[3], int orient,
                                  void *d_out_normals, void *d_out_curvature, void *d_out_counts, uint64_t *out_stats);

#ifdef __cplusplus
}
#endif
#endif
