/*
 * sgm_hip_voxel.h -- voxel-grid downsampling of a point cloud on the device: one centroid, one mean colour and one count per
 * occupied voxel of a regular grid, from the XYZ image of sgm_reproject / sgm_pipeline (or any point list).  It thins the cloud
 * that sgm_compact_points would hand out at full density, and with min_points > 1 it drops the voxels that hold a lone mismatch.
 * Included by sgm_hip.h: a caller includes that header and gets this one with it.
 *
 * It is a file of its own for the reason sgm_hip_confidence.h gives: the entry points sgm_hip.h and the headers before this one
 * declare are held, symbol for symbol, against lists fixed earlier; these are bound beside them (_lib.py: VOXEL_EXPORTS).
 *
 * In user code the place of this call is usually taken by Open3D's voxel_down_sample.  This is NOT Open3D's function: it is the
 * definition below, our own, with every sum taken in integers so that the result does not depend on the order in which the
 * device's atomics arrive.  Neither Open3D's values nor its output order are reproduced.
 *
 * Definition.
 *
 * Inputs: xyz float32 [n][3]; disp float32 [n] or null; colors_rgb uint8 [n][3] or null; voxel_size v, float32, finite, > 0, with a
 * finite 1.0f / v; origin o[3], float32, finite; min_points >= 1.  n <= 2^24 - 1 = 16 777 215 points (a 4096 x 2160 frame has
 * 8 847 360); a larger n is SGM_ERR_UNSUPPORTED.
 *
 *   1. Validity.  Point i is valid iff X, Y and Z are all finite and disp[i] > 0 (disp null: all three finite).  (The compaction
 *      looks at X alone; here every coordinate is floored.)
 *   2. Voxel index and fraction.  inv = 1.0f / v, formed once on the host in binary32.  Per axis a: t = (p_a - o_a) * inv, every
 *      operation rounded to binary32, nothing fused; g = floorf(t).  A valid point is in range iff -2^20 <= g < 2^20 on all three
 *      axes; valid points out of range are dropped and counted (n_out_of_range).  f = t - g in binary32, and
 *      u = min((uint32)(f * 65536.0f), 65535).  (The min is needed: for a tiny negative t such as -1e-10, g = -1 and t - g rounds
 *      to exactly 1.0f.)
 *   3. Key.  key = (g_x + 2^20) << 42 | (g_y + 2^20) << 21 | (g_z + 2^20), 63 bits.
 *   4. Per voxel, as mathematical integers: the count c of its points, S_a = sum of u_a per axis, C_k = sum of colour k per
 *      channel, first = the smallest source index among its points.  With n <= 2^24 - 1: c < 2^24, S_a < 2^40, C_k < 2^32, which
 *      is how the device holds them (c and S_x share one 64-bit word, 24 + 40 bits; S_y, S_z 64-bit words; C_r, C_g halves of one
 *      64-bit word; C_b and first 32-bit words).  No field can carry into its neighbour.
 *   5. Kept voxels are those with c >= min_points, in ascending order of first: a voxel sits where its first point sits in the
 *      source order (row-major for an XYZ image).
 *   6. Per kept voxel: M_a = (2 S_a + c) / (2 c) in integer division (the mean fraction in 1/65536 of a voxel, rounded half up);
 *      m_a = (float)M_a * (1 / 65536), exact; centroid_a = ((float)g_a + m_a) * v + o_a, three binary32 operations in this order,
 *      nothing fused.  Colour k = (2 C_k + c) / (2 c) as uint8.  Count c as uint32.
 * tests/voxel_ref.py restates this in numpy; the device results equal it bit for bit.
 *
 * Accuracy: against the exact mean of a voxel's members the centroid is off by less than v * 2^-15 (the quantisation of u and
 * the rounding of M) plus a few binary32 roundings of the coordinate's own magnitude (tests/test_voxel_reference.py derives and
 * checks the bound).
 */
#ifndef SGM_HIP_VOXEL_H
#define SGM_HIP_VOXEL_H

#include "sgm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host pointers, blocking.  Outputs are sized by the caller for the worst case, n rows: out_points float32 [n][3], out_colors
 * uint8 [n][3], out_counts uint32 [n]; rows past *n_voxels are left as they were.  Any of out_colors / out_counts /
 * n_out_of_range may be null.  colors_rgb without out_colors is accepted and ignored.
 * SGM_ERR_INVALID_ARG, with the outputs untouched, for a null e / xyz / out_points / n_voxels, n < 0, a voxel_size that is not
 * finite or <= 0 or whose 1.0f / v is not finite, a non-finite origin, min_points < 1, out_colors without colors_rgb;
 * SGM_ERR_UNSUPPORTED for n > 2^24 - 1.  n = 0 succeeds with 0 voxels.  SGM_ERR_HIP if a point found no slot in the table (the
 * probe is bounded by the table's capacity and the table is larger than the points that arrive: this is a defect, never a hang).
 * The engine keeps a table of 48 bytes per slot -- the smallest power of two of at least twice the points in range -- and one
 * 32-bit word per point; sgm_trim gives both back.  With SGM_OPT_PROFILE = 1 the stage record (sgm_get_stage_times) is the
 * call's afterwards: voxel_count, voxel_clear, voxel_insert, voxel_heads. */
int sgm_voxel_downsample(sgm_engine *e, const float *xyz, const float *disp, const uint8_t *colors_rgb, int64_t n,
                         float voxel_size, const float origin[3], int min_points,
                         float *out_points, uint8_t *out_colors, uint32_t *out_counts,
                         int64_t *n_voxels, int64_t *n_out_of_range);

/* The same with DEVICE pointers for the point data, on the engine's stream; origin, n_voxels and n_out_of_range are host
 * pointers.  Blocks twice: once for the number of points in range, which sizes the table, and at the end until the two counts
 * are known.  Outputs must not overlap inputs or each other. */
int sgm_voxel_downsample_device(sgm_engine *e, const void *d_xyz, const void *d_disp_f32, const void *d_colors_rgb, int64_t n,
                                float voxel_size, const float origin[3], int min_points,
                                void *d_out_points, void *d_out_colors, void *d_out_counts,
                                int64_t *n_voxels, int64_t *n_out_of_range);

#ifdef __cplusplus
}
#endif
#endif
