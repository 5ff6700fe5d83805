/*
 * sgm_hip_plane.h -- plane segmentation of a point cloud on the device: the dominant plane of the cloud (floor, table, wall) as a
 * model (a, b, c, d) with unit normal, per point whether it lies within a distance threshold of that plane and its signed distance
 * to it, and the cloud split into the points on the plane and the valid points off it, from the XYZ image of sgm_reproject /
 * sgm_pipeline (or any point list).  sgm_cluster_dbscan on a stereo cloud of a real scene returns one huge cluster, because the floor
 * connects everything that stands on it; with the plane's points removed it returns the objects.  The signed distance is the height
 * above ground that a fixed rig wants per frame: sgm_plane_inliers applies a model fitted once to every later cloud.
 * Included by sgm_hip.h: a caller includes that header and gets this one with it.
 *
 * It is a file of its own for the reason sgm_hip_confidence.h gives: the entry points sgm_hip.h and the headers before this one
 * declare are held, symbol for symbol, against lists fixed earlier; these are bound beside them (_lib.py: PLANE_EXPORTS).
 *
 * In user code the place of this call is usually taken by Open3D's segment_plane(distance_threshold, ransac_n, num_iterations).
 * This is NOT Open3D's function: it is the definition below, our own.  Ours is seeded and counter-based, so it gives the same bits
 * on every run; it scores every hypothesis on every valid point (no early stop, no subsampling); it breaks ties to the lowest
 * hypothesis index; it refits from integer moments with a range rule; it classifies with the refitted model; and it orients the
 * normal towards the origin.
 *
 * Definition.
 *
 * Inputs: xyz float32 [n][3]; disp float32 [n] or null; colors_rgb uint8 [n][3] or null; distance_threshold t, binary32;
 * num_iterations K, 1 <= K <= 65536; seed, uint32; refine, 0 or 1; select, 0 or 1.  n <= 2^24 - 1 points, as in sgm_hip_radius.h;
 * a larger n is SGM_ERR_UNSUPPORTED.
 *
 *   1. Validity is step 1 of sgm_hip_radius.h: point i is valid iff X, Y and Z are all finite and disp[i] > 0 (disp null: all
 *      three finite).  v_0 < v_1 < ... < v_{m-1} are the source indices of the m valid points.
 *   2. Host constants.  qscale = 32.0f / t, one binary32 division.  Refused: a t that is not finite, is <= 0 or is not a normal
 *      number, and a t whose qscale is not finite.
 *   3. Samples.  For hypothesis k = 0 .. K - 1 and j = 0, 1, 2 the counter is c = 3k + j and, all in uint32 arithmetic mod 2^32,
 *        x = seed ^ (c * 0x9E3779B9)
 *        x ^= x >> 16;  x *= 0x7FEB352D;  x ^= x >> 15;  x *= 0x846CA68B;  x ^= x >> 16
 *      The sample rank is ((uint64)x * m) >> 32 and the sample point p_j = xyz[v_rank].  Nothing forces the three ranks to differ.
 *      With m < 3 no hypothesis is formed at all (step 6).
 *   4. Hypothesis plane, in binary64 from the binary32 coordinates, every operation rounded on its own:  e1 = p_1 - p_0,
 *      e2 = p_2 - p_0;  n = e1 x e2, each component two products and a difference (n0 = e1_y * e2_z - e1_z * e2_y,
 *      n1 = e1_z * e2_x - e1_x * e2_z, n2 = e1_x * e2_y - e1_y * e2_x);  len2 = (n0 * n0 + n1 * n1) + n2 * n2.  The hypothesis is
 *      DEGENERATE iff len2 is not finite or not > 0: its count is 0, it can never be the best, and it is counted.  Otherwise
 *      len = sqrt(len2);  n_a = n_a / len;  d = -((n0 * p_00 + n1 * p_01) + n2 * p_02) with p_00, p_01, p_02 the coordinates of
 *      p_0.  Oriented and rounded by step 9 this is the plane (a, b, c, d) of hypothesis k in binary32.
 *   5. Signed distance and the inlier test -- the hot path.  s = fmaf(c, z, fmaf(b, y, fmaf(a, x, d))): three fused multiply-adds
 *      in binary32 in this order, starting from d.  A valid point is an inlier of a plane iff |s| <= t; the test is inclusive (and
 *      fails for a NaN).  cnt_k is the number of valid inliers of hypothesis k, an integer.  The library is built with
 *      floating-point contraction off; the fused operations are written as such or come from the matrix cores, whose binary32
 *      result is this same chain followed by fma(0, 0, s), which can only turn -0 into +0.
 *   6. Best.  k* is the lowest k with the largest cnt_k.  If m < 3 or cnt_k* < 3, NO PLANE is found: the model is (0, 0, 0, 0),
 *      every inlier byte is 0, every distance is the quiet NaN 0x7FC00000, n_inliers = 0, and the call succeeds.
 *   7. Refit (refine = 1 only), from integer moments as in sgm_hip_covariance.h.  The anchor is p_0 of hypothesis k*.  Per inlier
 *      of hypothesis k* and axis a:  d_a = p_a - anchor_a in binary32;  u_a = d_a * qscale in binary32;  the inlier is IN REFIT
 *      RANGE iff |u_a| <= 524288.0f on all three axes;  q_a = (int32)rintf(u_a), to nearest, ties to even.  Over the m_r inliers
 *      in refit range, in signed 64-bit integers:  S_a = sum q_a (three sums) and S_ab = sum q_a q_b for a <= b (six, in the order
 *      00, 01, 02, 11, 12, 22).  |q_a| <= 2^19 and m_r < 2^24, so |S_a| < 2^43 and |S_ab| <= 2^24 * 2^38 = 2^62: nothing
 *      overflows.  If m_r >= 3, steps 7 to 9 of sgm_hip_covariance.h apply word for word with m = m_r terms (there is no extra
 *      term for "the point itself"): the covariance C_ab = (double)S_ab - ((double)S_a * (double)S_b) / (double)m_r, the division
 *      by the largest diagonal entry, six Jacobi sweeps, the column of the smallest diagonal entry and its normalisation, without
 *      that header's orientation.  If that problem is not degenerate, the refitted plane has that unit normal nv and passes through
 *      the centroid g_a = (double)anchor_a + ((double)S_a / (double)m_r) / (double)qscale:  d = -((nv0 * g0 + nv1 * g1) + nv2 * g2),
 *      all in binary64; oriented and rounded by step 9 it is the final model, and refined = 1.  Otherwise -- m_r < 3, the
 *      degenerate case, refine = 0 -- the model stays hypothesis k*'s.
 *      Inliers outside the refit range stay inliers; they only do not vote.  A stereo cloud has valid points at enormous Z.  A
 *      quantum tied to the cloud's extent would let one of them ruin the fit: everything near the camera would quantise to a few
 *      steps.  A quantum of t / 32 with +-16384 t of range around a point of the plane cannot be ruined that way: the fit is
 *      resolved to a thirty-second of the tolerance it is asked for, over 32768 tolerances of extent.
 *   8. Classification with the final model.  out_inlier[i] = 1 iff point i is valid and |s_i| <= t (step 5 with the final model),
 *      otherwise 0;  out_distance[i] = s_i for the valid points and 0x7FC00000 for the others;  n_inliers is their number.  The
 *      compacted outputs out_points, out_colors and out_index (the source index of each row) hold, in source order, the inliers
 *      (select = 0) or the valid points that are not inliers (select = 1; with no plane found: every valid point); *n_selected is
 *      the number of rows, and rows past it are left as they were.
 *   9. Orientation and rounding of any plane (a, b, c, d) held in binary64.  All four are negated if d < 0; if d == 0, all four
 *      are negated if the first non-zero of a, b, c is negative.  This puts the origin, where the camera is, on the non-negative
 *      side: s >= 0 there, and a floor below the camera has its normal pointing up at it.  Then each is rounded to binary32 and
 *      0.0f is added to each in binary32, so no negative zero comes out.
 *
 * Outputs besides those of step 8: out_model float32 [4]; out_stats uint64 [8]: valid points m, degenerate hypotheses, k*,
 * cnt_k*, m_r, inliers of k* out of refit range, refined (0 / 1), found (0 / 1).  With m < 3 all but the first are 0; with
 * refine = 0 or no plane found, m_r, the out-of-range count and refined are 0.
 *
 * Every float result is a function of integer counts, integer sums and fixed-order arithmetic: the counts and sums do not depend on
 * the order in which the device's atomics arrive, and the same bits come out on every run.  tests/plane_ref.py restates the
 * definition in numpy, with fmaf emulated exactly; the device results equal it bit for bit under both forms of step 5.
 *
 * Cost.  Step 5 is m x K evaluations whatever the cloud looks like: nothing stops early and nothing is subsampled.  Open3D's
 * probability-based early stop, ransac_n > 3, a batch form, other shapes (cylinders, spheres) and an asynchronous form are not
 * offered.
 */
#ifndef SGM_HIP_PLANE_H
#define SGM_HIP_PLANE_H

#include "sgm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host pointers, blocking.  out_inlier and out_distance have n entries; out_points, out_colors and out_index are sized by the
 * caller for the worst case, n rows, and rows past *n_selected are left as they were.  Any of out_inlier / out_distance /
 * out_points / out_colors / out_index / out_model / out_stats / n_selected may be null.  colors_rgb without out_colors is accepted
 * and ignored.  SGM_ERR_INVALID_ARG, with every output untouched and an sgm_last_error that names the entry, for a null e / xyz /
 * n_inliers, n < 0, a distance_threshold refused by step 2, num_iterations outside 1 .. 65536, a refine or select that is neither
 * 0 nor 1, out_colors without colors_rgb; SGM_ERR_UNSUPPORTED for n > 2^24 - 1.  n = 0 succeeds as "no plane".
 * The engine keeps 16 bytes per point for the list of valid points, 20 bytes per hypothesis and one byte per point; sgm_trim gives
 * them back.  With SGM_OPT_PROFILE = 1 the stage record (sgm_get_stage_times) is the call's afterwards: plane_valid, plane_sample,
 * plane_count, plane_best, plane_moments and plane_solve (refine = 1 only), plane_classify, plane_compact. */
int sgm_segment_plane(sgm_engine *e, const float *xyz, const float *disp, const uint8_t *colors_rgb, int64_t n,
                      float distance_threshold, int num_iterations, uint32_t seed, int refine, int select,
                      uint8_t *out_inlier, float *out_distance, float *out_points, uint8_t *out_colors, uint32_t *out_index,
                      float out_model[4], uint64_t out_stats[8], int64_t *n_inliers, int64_t *n_selected);

/* The same with DEVICE pointers for the point data and the per-point and compacted outputs, on the engine's stream; out_model,
 * out_stats, n_inliers and n_selected are host pointers.  Blocks once, at the end, until those host words are known: the kernels
 * read the number of valid points from device memory.  Outputs must not overlap inputs or each other. */
int sgm_segment_plane_device(sgm_engine *e, const void *d_xyz, const void *d_disp_f32, const void *d_colors_rgb, int64_t n,
                             float distance_threshold, int num_iterations, uint32_t seed, int refine, int select,
                             void *d_out_inlier, void *d_out_distance, void *d_out_points, void *d_out_colors, void *d_out_index,
                             float out_model[4], uint64_t out_stats[8], int64_t *n_inliers, int64_t *n_selected);

/* Step 8 alone on a caller's model (a, b, c, d) and threshold: a fixed rig fits its floor once and applies it to every frame.  The
 * outputs are those of step 8.  Refused like the above, and also: a null model, a model whose four values are not all finite or
 * whose (a * a + b * b) + c * c, in binary32, is not within 2^-10 of 1.  The stage record: plane_classify, plane_compact. */
int sgm_plane_inliers(sgm_engine *e, const float *xyz, const float *disp, const uint8_t *colors_rgb, int64_t n,
                      const float model[4], float distance_threshold, int select,
                      uint8_t *out_inlier, float *out_distance, float *out_points, uint8_t *out_colors, uint32_t *out_index,
                      int64_t *n_inliers, int64_t *n_selected);

/* The same with DEVICE pointers for the point data and the outputs; model, n_inliers and n_selected are host pointers.  Blocks
 * once, at the end. */
int sgm_plane_inliers_device(sgm_engine *e, const void *d_xyz, const void *d_disp_f32, const void *d_colors_rgb, int64_t n,
                             const float model[4], float distance_threshold, int select,
                             void *d_out_inlier, void *d_out_distance, void *d_out_points, void *d_out_colors, void *d_out_index,
                             int64_t *n_inliers, int64_t *n_selected);

#ifdef __cplusplus
}
#endif
#endif
