/*
 * sgm_hip_radius.h -- radius outlier removal for a point cloud on the device: how many other points lie within a fixed radius of
 * each point, and the points that have at least nb_points such neighbours, from the XYZ image of sgm_reproject / sgm_pipeline (or
 * any point list).  It removes the clumps of mismatches that are consistent in disparity but float in space, which the filters
 * in the image do not see; unlike sgm_voxel_downsample with min_points it is not tied to a grid and keeps the samples themselves.
 * Included by sgm_hip.h: a caller includes that header and gets this one with it.
 *
 * It is a file of its own for the reason sgm_hip_confidence.h gives: the entry points sgm_hip.h and the headers before this one
 * declare are held, symbol for symbol, against lists fixed earlier; these are bound beside them (_lib.py: RADIUS_EXPORTS).
 *
 * In user code the place of this call is usually taken by Open3D's remove_radius_outlier(nb_points, radius).  This is NOT Open3D's
 * function: it is the definition below, our own.  Ours does not count the point itself (Open3D's search finds the query point and
 * counts it), it has a range rule (step 3), and its count output saturates at max_count.
 *
 * Definition.
 *
 * Inputs: xyz float32 [n][3]; disp float32 [n] or null; colors_rgb uint8 [n][3] or null; radius r, float32; nb_points >= 1;
 * max_count >= nb_points; origin o[3], float32, finite.  n <= 2^24 - 1 = 16 777 215 points (a 4096 x 2160 frame has 8 847 360); a
 * larger n is SGM_ERR_UNSUPPORTED.
 *
 *   1. Validity, as in sgm_hip_voxel.h.  Point i is valid iff X, Y and Z are all finite and disp[i] > 0 (disp null: all three
 *      finite).
 *   2. Host constants, formed once in binary32, every operation rounded on its own, nothing fused:
 *      r2 = r * r;  v = r * 1.03125f;  inv = 1.0f / v.  Refused: an r that is not finite or is <= 0, an r2 that is not a finite
 *      normal number (r2 < 2^-126 or infinite), an inv that is not finite.
 *   3. Range.  Per axis a: t = (p_a - o_a) * inv, two binary32 operations; g = floorf(t).  A valid point is in range iff
 *      -2^16 <= g < 2^16 on all three axes.  Valid points out of range are dropped and counted (n_out_of_range): they are nobody's
 *      neighbour, their count is 0 and their keep is 0, like those of the points that are not valid.
 *   4. Distance.  For two in-range points i and j: dx = x_j - x_i, dy = y_j - y_i, dz = z_j - z_i and
 *      d2 = (dx * dx + dy * dy) + dz * dz, every operation rounded to binary32 in this order, nothing fused (the library is built
 *      with floating-point contraction off).  d2 is symmetric in i and j: dx only changes its sign.
 *   5. Count.  c_i = the number of in-range points j != i with d2 <= r2: the test is inclusive, and duplicates of point i (other
 *      indices, the same coordinates) count.  count_i = min(c_i, max_count);  keep_i = c_i >= nb_points.  (max_count >= nb_points,
 *      so keep_i can be read off count_i: keep_i = count_i >= nb_points.)
 *   6. Outputs.  out_keep uint8 [n], 0 or 1 -- usable as the `confidence` of valid_points, triangulate_points and
 *      estimate_normals with min_confidence = 1; out_counts uint32 [n]; and the kept points compacted in source order: out_points
 *      float32 [][3], out_colors uint8 [][3], out_index uint32 [] (the source index of each kept point); rows past *n_kept are
 *      left as they were.
 *
 * The definition is grid-free: step 5 is a statement over all pairs.  The grid of step 3 fixes the range rule only; the device
 * uses it to find the pairs, which is sound by the
 *
 * Lemma.  Two in-range points p, q with d2 <= r2 have |g_a(p) - g_a(q)| <= 1 on every axis a.
 * Proof.  Write u = 2^-24.  (a) t_a is computed from the real number (p_a - o_a) / v by three roundings -- the difference, inv and
 * the product -- each of relative error at most u, and an in-range point has |t_a| <= 2^16, so t_a is off that real number by at
 * most (3u + O(u^2)) * 2^16 < 0.0118.  (b) r2 is normal, so r2 >= 2^-126 and r2 <= r^2 (1 + u).  Each of the three squares and
 * two sums of d2 is a rounding of relative error at most u unless a square underflows, where it is off by at most 2^-150
 * absolutely, which is at most 2^-24 r2; the differences dx, dy, dz are roundings of relative error at most u as well (two for
 * each square).  So the true squared distance is at most r2 (1 + 5u) + 3u r2 <= r^2 (1 + 10u), and the true |p_a - q_a| is at
 * most r (1 + 2^-21).  (c) v = r * 1.03125 (1 + e), |e| <= u.  So
 * |(p_a - o_a) / v - (q_a - o_a) / v| <= (1 + 2^-21) / (1.03125 (1 - u)) < 0.9698, and by (a)
 * |t_a(p) - t_a(q)| < 0.9698 + 2 * 0.0118 = 0.9934 < 1.  Two numbers less than 1 apart have floors at most 1 apart.
 * tests/test_radius_reference.py checks the claim on random clouds and on points placed within an ulp of cell faces.
 *
 * Every result is an integer count or a predicate on one: the output does not depend on the order in which the device's atomics
 * arrive, and the same bits come out on every run.  tests/radius_ref.py restates the definition in numpy, over all pairs and over
 * 27 cells; the device results equal it bit for bit.
 *
 * Cost.  The work of a call is the number of candidates in the 27 cells around each point, cut short per point once its count
 * has reached max_count.  A radius that puts the whole cloud into a few cells, with a large max_count, is quadratic in n; nothing
 * bounds that except max_count.  A fixed metric radius also thins the far range of a stereo cloud, whose point spacing grows with
 * depth; a radius scaled by depth is not offered.  Statistical outlier removal, which asks for the mean distance to the k nearest
 * neighbours instead of a count and takes its threshold from the cloud, is sgm_hip_statistical.h; it runs on this grid.
 */
#ifndef SGM_HIP_RADIUS_H
#define SGM_HIP_RADIUS_H

#include "sgm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host pointers, blocking.  out_keep and out_counts have n entries; out_points, out_colors and out_index are sized by the caller
 * for the worst case, n rows, and rows past *n_kept are left as they were.  Any of out_keep / out_counts / out_points /
 * out_colors / out_index / n_out_of_range may be null.  colors_rgb without out_colors is accepted and ignored.
 * SGM_ERR_INVALID_ARG, with the outputs untouched, for a null e / xyz / n_kept, n < 0, a radius refused by step 2, a non-finite
 * or null origin, nb_points < 1, max_count < nb_points, out_colors without colors_rgb; SGM_ERR_UNSUPPORTED for n > 2^24 - 1.
 * n = 0 succeeds with 0 kept points.  SGM_ERR_HIP if a point found no slot in the table (the probe is bounded by the table's
 * capacity and the table has at least as many slots as points arrive: this is a defect, never a hang).
 * The engine keeps a table of 16 bytes per slot -- the smallest power of two of at least twice the points in range --, 16 bytes
 * per point in range for the sorted records and 8 bytes per point; sgm_trim gives them back.  With SGM_OPT_PROFILE = 1 the stage
 * record (sgm_get_stage_times) is the call's afterwards: radius_count, radius_clear, radius_insert, radius_starts, radius_sort,
 * radius_query, radius_compact. */
int sgm_radius_outlier(sgm_engine *e, const float *xyz, const float *disp, const uint8_t *colors_rgb, int64_t n,
                       float radius, const float origin[3], int nb_points, int max_count,
                       uint8_t *out_keep, uint32_t *out_counts, float *out_points, uint8_t *out_colors, uint32_t *out_index,
                       int64_t *n_kept, int64_t *n_out_of_range);

/* The same with DEVICE pointers for the point data, on the engine's stream; origin, n_kept and n_out_of_range are host
 * pointers.  Blocks twice: once for the number of points in range, which sizes the table, and at the end until the two counts
 * are known.  Outputs must not overlap inputs or each other. */
int sgm_radius_outlier_device(sgm_engine *e, const void *d_xyz, const void *d_disp_f32, const void *d_colors_rgb, int64_t n,
                              float radius, const float origin[3], int nb_points, int max_count,
                              void *d_out_keep, void *d_out_counts, void *d_out_points, void *d_out_colors, void *d_out_index,
                              int64_t *n_kept, int64_t *n_out_of_range);

#ifdef __cplusplus
}
#endif
#endif
