/*
 * sgm_hip_statistical.h -- statistical outlier removal for a point cloud on the device: per point the mean distance to its
 * nb_neighbors nearest other points within max_radius, and the points whose mean is not above the cloud's own mean of these means
 * plus std_ratio standard deviations.  Where sgm_radius_outlier (sgm_hip_radius.h) asks "does this point have nb neighbours within
 * r?" with one absolute threshold, this asks "is this point's neighbourhood as tight as the cloud's typical neighbourhood?" with
 * a threshold the cloud sets itself: it removes the loose fringe around depth edges and the sparse haze that passes a count test.
 * Included by sgm_hip.h: a caller includes that header and gets this one with it.
 *
 * It is a file of its own for the reason sgm_hip_confidence.h gives: the entry points sgm_hip.h and the headers before this one
 * declare are held, symbol for symbol, against lists fixed earlier; these are bound beside them (_lib.py: STATISTICAL_EXPORTS).
 *
 * In user code the place of this call is usually taken by Open3D's remove_statistical_outlier(nb_neighbors, std_ratio).  This is
 * NOT Open3D's function: it is the definition below, our own.  Open3D searches the k nearest points without bound and counts the
 * query point among them; ours searches within max_radius only, never counts the point itself, calls a point with fewer than k
 * neighbours there an outlier outright, has the range rule of sgm_hip_radius.h, and forms the statistic in integers.
 *
 * Definition.
 *
 * Inputs: xyz float32 [n][3]; disp float32 [n] or null; colors_rgb uint8 [n][3] or null; nb_neighbors k, 1 <= k <= 64; std_ratio,
 * float32, finite and >= 0; max_radius r, float32; origin o[3], float32, finite.  n <= 2^24 - 1 points, as in sgm_hip_radius.h.
 *
 *   1 - 4. Validity, host constants, range and distance are steps 1 to 4 of sgm_hip_radius.h with r = max_radius, word for word:
 *      r2 = r * r;  v = r * 1.03125f;  inv = 1.0f / v, with the same refusals; cells of edge v anchored at o with indices in
 *      -2^16 .. 2^16 - 1; d2 = (dx * dx + dy * dy) + dz * dz in binary32, nothing fused.  One more host constant:
 *      qscale = 524288.0f / r, one binary32 division; an r whose qscale is not finite is refused.
 *   5. Neighbours.  For an in-range point i, N_i is the multiset of d2(i, j) over the in-range points j != i with d2 <= r2 (the
 *      test is inclusive, duplicates of point i count), and c_i = |N_i|.  Point i is DENSE iff c_i >= k.  The in-range points that
 *      are not dense are SPARSE: their k-th neighbour lies beyond max_radius, which makes them outliers by definition.  They are
 *      not kept, take no part in the statistic and are counted (n_sparse).
 *   6. The mean distance of a dense point.  e_1 <= ... <= e_k are the k smallest elements of N_i, as values (which of two equal
 *      values is taken does not show).  s_m = sqrtf(e_m), the correctly rounded square root;  acc = s_1, then acc = acc + s_m for
 *      m = 2 .. k in this ascending order, every addition rounded to binary32;  mean_i = acc / (float)k, the correctly rounded
 *      division.
 *   7. The statistic, in integers.  q_i = (uint32)(mean_i * qscale): one binary32 product, then truncation.  q_i < 2^19 + 4:
 *      with u = 2^-24, e_m <= r2 <= r^2 (1 + u) gives s_m <= r (1 + 2 u); the k - 1 additions and the division lose at most a
 *      factor (1 + u)^k <= (1 + u)^64, so mean_i <= r (1 + 67 u); qscale <= (2^19 / r)(1 + u) and the product rounds once more:
 *      mean_i * qscale <= 2^19 (1 + 70 u) < 2^19 + 3.  Over the dense points: m = their number, A = sum of q_i, B = sum of q_i^2,
 *      in unsigned 64-bit integers (B < 2^24 * 2^39 = 2^63).  Integer sums do not depend on the order in which they are formed.
 *   8. The threshold, on the host in binary64, every operation rounded on its own:  mu = (double)A / (double)m;
 *      var = m >= 2 ? ((double)B - (double)A * mu) / (double)(m - 1) : 0, and a negative var becomes 0;
 *      thr = mu + (double)std_ratio * sqrt(var);  T = (uint32)floor(thr), and a thr of 2^32 - 1 or more gives T = 2^32 - 2 (no q
 *      comes near it: every dense point is kept).  With m = 0 nothing is kept and T = 0.
 *   9. Keep.  keep_i = dense_i and q_i <= T: the test is inclusive, as the radius test is.
 *  10. Outputs.  out_keep uint8 [n], 0 or 1 -- usable as the `confidence` of valid_points, triangulate_points and
 *      estimate_normals with min_confidence = 1, as the radius mask is; out_mean float32 [n]: mean_i for the dense points and
 *      -1.0f for every other point; the kept points compacted in source order: out_points float32 [][3], out_colors uint8 [][3],
 *      out_index uint32 [] (the source index of each kept point), rows past *n_kept left as they were; out_stats uint64 [8]:
 *      points in range, valid points out of range, dense, sparse, A, B, T, 0.
 *
 * The definition is grid-free like that of sgm_hip_radius.h, whose lemma makes the 27 cells around a point hold all of N_i.  Every
 * float result is a function of one point's neighbour multiset, formed in a fixed order, and everything that crosses points is an
 * integer sum: the same bits come out on every run.  tests/statistical_ref.py restates the definition in numpy, over all pairs
 * and over 27 cells; the device results equal it bit for bit.
 *
 * Cost.  The work of a call is the number of candidates in the 27 cells around each point, and nothing cuts it short: where
 * sgm_radius_outlier stops a point's search at max_count, the k nearest are known only when every candidate has been seen.  A
 * max_radius that puts the whole cloud into a few cells is quadratic in n.  max_radius should hold a few times k neighbours at
 * the density that is to count as ordinary: much less and most points are sparse, much more and the time goes into candidates
 * that cannot be among the k nearest.  A fixed metric max_radius thins the far range of a stereo cloud like the radius of
 * sgm_radius_outlier does; a radius scaled by depth and an unbounded k-nearest search are not offered.
 */
#ifndef SGM_HIP_STATISTICAL_H
#define SGM_HIP_STATISTICAL_H

#include "sgm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host pointers, blocking.  out_keep and out_mean have n entries; out_points, out_colors and out_index are sized by the caller
 * for the worst case, n rows, and rows past *n_kept are left as they were; out_stats has 8 entries.  Any of out_keep / out_mean /
 * out_points / out_colors / out_index / out_stats may be null.  colors_rgb without out_colors is accepted and ignored.
 * SGM_ERR_INVALID_ARG, with the outputs untouched, for a null e / xyz / n_kept, n < 0, nb_neighbors outside 1 .. 64, a std_ratio
 * that is negative or not finite, a max_radius refused by step 2 of sgm_hip_radius.h or with a qscale that is not finite, a
 * non-finite or null origin, out_colors without colors_rgb; SGM_ERR_UNSUPPORTED for n > 2^24 - 1.  n = 0 succeeds with 0 kept
 * points and out_stats all zero.  SGM_ERR_HIP if a point found no slot in the table (a defect, never a hang: every probe is
 * bounded by the table's capacity, and nothing waits for anything).
 * The engine reuses the table, records and staging of sgm_radius_outlier and adds 4 bytes per point for the staged means;
 * sgm_trim gives them back.  With SGM_OPT_PROFILE = 1 the stage record (sgm_get_stage_times) is the call's afterwards:
 * stat_count, stat_clear, stat_insert, stat_starts, stat_sort, stat_query, stat_reduce, stat_keep, stat_compact. */
int sgm_statistical_outlier(sgm_engine *e, const float *xyz, const float *disp, const uint8_t *colors_rgb, int64_t n,
                            int nb_neighbors, float std_ratio, float max_radius, const float origin[3],
                            uint8_t *out_keep, float *out_mean, float *out_points, uint8_t *out_colors, uint32_t *out_index,
                            int64_t *n_kept, uint64_t *out_stats);

/* The same with DEVICE pointers for the point data, on the engine's stream; origin, n_kept and out_stats are host pointers.
 * Blocks three times: for the number of points in range, which sizes the table; for the sums m, A and B, from which the host
 * forms T; and at the end until the number of kept points is known.  Outputs must not overlap inputs or each other. */
int sgm_statistical_outlier_device(sgm_engine *e, const void *d_xyz, const void *d_disp_f32, const void *d_colors_rgb, int64_t n,
                                   int nb_neighbors, float std_ratio, float max_radius, const float origin[3],
                                   void *d_out_keep, void *d_out_mean, void *d_out_points, void *d_out_colors, void *d_out_index,
                                   int64_t *n_kept, uint64_t *out_stats);

#ifdef __cplusplus
}
#endif
#endif
