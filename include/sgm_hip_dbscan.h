/*
 * sgm_hip_dbscan.h -- density clustering of a point cloud on the device: the cloud split into the objects it holds.  Per point the
 * number of the cluster it belongs to (or -1: noise), whether it is a core point, and per cluster its size, from the XYZ image of
 * sgm_reproject / sgm_pipeline or any point list (the centroids of sgm_voxel_downsample, a list cleaned by sgm_radius_outlier or
 * sgm_statistical_outlier).  The outlier removals give a verdict per point; this says which points hang together.  It runs on the
 * grid of cells of sgm_hip_radius.h.  Included by sgm_hip.h: a caller includes that header and gets this one with it.
 *
 * It is a file of its own for the reason sgm_hip_confidence.h gives: the entry points sgm_hip.h and the headers before this one
 * declare are held, symbol for symbol, against lists fixed earlier; these are bound beside them (_lib.py: DBSCAN_EXPORTS).
 *
 * In user code the place of this call is usually taken by Open3D's cluster_dbscan(eps, min_points), often followed by "keep the
 * largest cluster".  This is NOT Open3D's cluster_dbscan (nor scikit-learn's DBSCAN): it is the definition below, our own.  Ours
 * does not count the point itself among its neighbours (Open3D and scikit-learn do: their min_points / min_samples is ours plus
 * one), it has the range rule of sgm_hip_radius.h, it gives a border point to its NEAREST core point instead of to whichever
 * cluster reaches it first, and it numbers the clusters by their smallest core index instead of by the order of a traversal.
 *
 * Definition.
 *
 * Inputs: xyz float32 [n][3]; disp float32 [n] or null; eps r, float32; min_points k, 1 <= k <= 2^24 - 1; origin o[3], float32,
 * finite.  n <= 2^24 - 1 points, as in sgm_hip_radius.h; a larger n is SGM_ERR_UNSUPPORTED.
 *
 *   1. Validity, as in sgm_hip_voxel.h.  Point i is valid iff X, Y and Z are all finite and disp[i] > 0 (disp null: all three
 *      finite).
 *   2. Host constants, formed once in binary32, every operation rounded on its own, nothing fused:
 *      r2 = r * r;  v = r * 1.03125f;  inv = 1.0f / v.  Refused: an r that is not finite or is <= 0, an r2 that is not a finite
 *      normal number (r2 < 2^-126 or infinite), an inv that is not finite.
 *   3. Range.  Per axis a: t = (p_a - o_a) * inv, two binary32 operations; g = floorf(t).  A valid point is in range iff
 *      -2^16 <= g < 2^16 on all three axes.  Valid points out of range are dropped and counted: they are nobody's neighbour and
 *      they are noise, like the points that are not valid.
 *   4. Distance.  For two in-range points i and j: dx = x_j - x_i, dy = y_j - y_i, dz = z_j - z_i and
 *      d2 = (dx * dx + dy * dy) + dz * dz, every operation rounded to binary32 in this order, nothing fused (the library is built
 *      with floating-point contraction off).  d2 is symmetric in i and j: dx only changes its sign.
 *   5. Core points.  c_i = the number of in-range points j != i with d2 <= r2: the test is inclusive, duplicates of point i (other
 *      indices, the same coordinates) count, and the point itself does not.  Point i is CORE iff c_i >= k.  The core mask is
 *      therefore, byte for byte, the keep mask of sgm_radius_outlier with nb_points = k.  (Open3D and scikit-learn count the point
 *      itself: their min_points is ours plus one.)
 *   6. Clusters.  Two core points i and j are linked iff d2 <= r2.  A cluster is a connected component of the core points under
 *      that relation.
 *   7. Border points.  An in-range point that is not core and has at least one core point within r2 is a BORDER point and belongs
 *      to the cluster of its nearest core point: the one of the smallest d2, compared as the binary32 value; among core points of
 *      the same d2 the one of the smallest source index.  A border point never links two clusters.  (Classic DBSCAN hands a border
 *      point to whichever cluster reaches it first, which depends on the order of the traversal; this rule is what makes the
 *      result independent of every order.)
 *   8. Noise.  Every other point has the label -1: the in-range points that are neither core nor border, the valid points out of
 *      range and the points that are not valid.
 *   9. Numbering.  A cluster's representative is the smallest source index among its core points.  The clusters are numbered
 *      0, 1, ... in ascending order of their representatives.
 *  10. Outputs.  out_labels int32 [n]: the cluster's number or -1; out_core uint8 [n], 0 or 1; out_sizes uint32 []: per cluster
 *      the number of its core and border points -- the caller sizes it for the worst case, n rows, and rows past *n_clusters are
 *      left as they were; out_stats uint64 [6]: points in range, valid points out of range, core points, border points, in-range
 *      noise points, clusters; *n_clusters int64.
 *
 * The definition is grid-free like that of sgm_hip_radius.h: steps 5 to 7 are statements over all pairs, and that header's lemma
 * makes the 27 cells around a point hold every point within r2 of it, so the device finds every link there.  Every output is an
 * integer that is a function of the set of links, not of the order in which the device finds them: the same bits come out on
 * every run.  tests/dbscan_ref.py restates the definition in numpy, over all pairs and over 27 cells; the device results equal it
 * bit for bit.  Under a permutation of the points the partition and the core mask stay and only the numbering changes.
 *
 * Cost.  The work of a call is the number of candidates in the 27 cells around each point, once cut short at k neighbours (the
 * core pass) and once in full (the link pass): a core point has to meet every core neighbour, so nothing stops it early.  An eps
 * that puts the whole cloud into a few cells is quadratic in n.  A fixed metric eps also splits the far range of a stereo cloud,
 * whose point spacing grows with depth, into many small clusters and noise; an eps scaled by depth is not offered, nor are HDBSCAN,
 * OPTICS, a batch form or an asynchronous form.  The usual chain is sgm_voxel_downsample first, which evens the density out, then
 * this call on the centroids with eps about twice the voxel size.
 */
#ifndef SGM_HIP_DBSCAN_H
#define SGM_HIP_DBSCAN_H

#include "sgm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host pointers, blocking.  out_labels and out_core have n entries, out_sizes is sized by the caller for n rows, out_stats has 6.
 * Any of the four may be null; n_clusters is required.  SGM_ERR_INVALID_ARG, with the outputs untouched, for a null e / xyz /
 * n_clusters, n < 0, an eps refused by step 2, min_points outside 1 .. 2^24 - 1, a null or non-finite origin; SGM_ERR_UNSUPPORTED
 * for n > 2^24 - 1.  n = 0 succeeds with 0 clusters and out_stats all zero.  SGM_ERR_HIP if a point found no slot in the table (a
 * defect, never a hang: every probe is bounded by the table's capacity, every loop of the union-find ends because a link strictly
 * fell, and nothing waits for anything).
 * The engine reuses the table, records and staging of sgm_radius_outlier and adds 4 + 4 + 4 bytes per point -- the parent link,
 * the nearest core point and the root's rank -- and 4 + 4 for the host entry's staged labels and sizes; sgm_trim gives them back.
 * With SGM_OPT_PROFILE = 1 the stage record (sgm_get_stage_times) is the call's afterwards: dbscan_count, dbscan_clear,
 * dbscan_insert, dbscan_starts, dbscan_sort, dbscan_core (the count cut short at min_points, then the core bit marked in the
 * sorted records and the links set to identity: two launches), dbscan_link, dbscan_number (the roots counted, scanned and ranked:
 * three launches), dbscan_label. */
int sgm_cluster_dbscan(sgm_engine *e, const float *xyz, const float *disp, int64_t n, float eps, int min_points,
                       const float origin[3], int32_t *out_labels, uint8_t *out_core, uint32_t *out_sizes, uint64_t *out_stats,
                       int64_t *n_clusters);

/* The same with DEVICE pointers for the point data and the three per-point / per-cluster outputs, on the engine's stream; origin,
 * out_stats and n_clusters are host pointers.  Blocks twice: once for the number of points in range, which sizes the table, and
 * at the end until the counts are known.  Outputs must not overlap inputs or each other. */
int sgm_cluster_dbscan_device(sgm_engine *e, const void *d_xyz, const void *d_disp_f32, int64_t n, float eps, int min_points,
                              const float origin[3], void *d_out_labels, void *d_out_core, void *d_out_sizes, uint64_t *out_stats,
                              int64_t *n_clusters);

#ifdef __cplusplus
}
#endif
#endif
