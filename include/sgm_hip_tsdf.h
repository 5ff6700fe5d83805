/*
 * sgm_hip_tsdf.h -- many frames fused into one model: a truncated signed distance volume on the device.  A dense volume of voxels
 * takes organised XYZ images with their camera poses -- one per call -- and keeps, per voxel, the integer sum of the quantised signed
 * distances to the surface each frame saw, the number of frames that saw it and, optionally, the sum of their colours; the zero
 * crossings of the averaged distance are then extracted as one point list.  Every other cloud call works on one cloud, and
 * sgm_register_icp joins two; this one joins N, and averages where concatenating the transformed clouds only piles noisy surfaces
 * on each other.  Included by sgm_hip.h: a caller includes that header and gets this one with it.
 *
 * It is a file of its own for the reason sgm_hip_confidence.h gives: the entry points sgm_hip.h and the headers before this one
 * declare are held, symbol for symbol, against lists fixed earlier; these are bound beside them (_lib.py: TSDF_EXPORTS).
 *
 * In user code the place of these calls is usually taken by Open3D's UniformTSDFVolume / ScalableTSDFVolume (integrate,
 * extract_point_cloud).  This is NOT Open3D's integration: it is the definition below, our own.  The differences: the depth of a
 * pixel is the Z of the XYZ image, not a depth image; the distance is along the camera's Z axis and is quantised to an integer of
 * 1 / 32767 of the truncation distance; the per-voxel state is an integer sum and an integer count, not a running float average, so
 * that the order of the frames does not matter; the weight of a frame is 1 and stops at 65535; the extraction interpolates from the
 * two averaged distances of an edge in binary32 and takes the colour of the nearer end, and it walks the voxels in index order.
 *
 * Definition.
 *
 * Volume.  Dimensions nx, ny, nz, each 1 .. 4096, with V = nx * ny * nz <= 2^30; voxel_size vs and sdf_trunc tau, binary32, finite,
 * positive; origin o[3], finite.  Voxel (i, j, k) has the linear index v = (k * ny + j) * nx + i, x fastest.  The planes belong to the
 * caller: sum int32 [V], weight int32 [V] and optionally rgb_sum uint32 [3][V], planar.  All zero is the empty volume; resetting the
 * volume is the caller zeroing these planes.
 *
 * Frame.  xyz float32 [H][W][3]; disp float32 [H][W] or null; colors uint8 [H][W][3] or null -- colours are given iff rgb_sum is;
 * cam = (fx, fy, cx, cy), binary32; front, +1 or -1, the sign of Z in front of the camera (the Q of the notebook gives NEGATIVE Z,
 * so this is an argument, not an assumption); extrinsic double [16], world -> camera, row-major, checked like T0 of sgm_hip_icp.h
 * (every entry finite, last row (0, 0, 0, 1)), its first three rows rounded to binary32 as M; max_depth, binary32, > 0 or +inf.
 * H, W >= 1 and H * W <= 2^27.
 *
 * Integration, per voxel, all in binary32, nothing contracted:
 *   1. Centre.  c_a = fmaf((float)i_a + 0.5f, vs, o_a) for a = x, y, z.
 *   2. Camera frame.  p = M c by the three-fma chain of step 2 of sgm_hip_icp.h:  p_x = fmaf(M02, c_z, fmaf(M01, c_y,
 *      fmaf(M00, c_x, M03))) and likewise p_y, p_z.
 *   3. In front.  Required: front * p_z > 0.  Otherwise the voxel is OUTSIDE.
 *   4. Pixel.  iz = 1.0f / p_z;  u = fmaf(fx, p_x * iz, cx) + 0.5f;  w = fmaf(fy, p_y * iz, cy) + 0.5f.  Required, as float
 *      comparisons before any conversion, so that NaN and inf fail:  0 <= u < (float)W and 0 <= w < (float)H.  Otherwise the voxel
 *      is OUTSIDE.  px = (int)floorf(u), py = (int)floorf(w).
 *   5. Depth.  With (X, Y, Z) and disp of pixel (py, px): the pixel is USABLE iff X, Y, Z are all finite and disp > 0 (step 1 of
 *      sgm_hip_radius.h; a null disp passes), front * Z > 0 and front * Z <= max_depth.  Otherwise the voxel has NO DEPTH.
 *   6. Distance.  s = front * (Z - p_z).  s < -tau: the voxel is OCCLUDED, no update.  t = fminf(s, tau);
 *      q = (int)rintf(t * kappa), ties to even, with kappa = 32767.0f / tau formed once on the host.
 *   7. Update.  A voxel with weight == 65535 is SATURATED and left alone.  Otherwise sum += q, weight += 1 and, with colours,
 *      rgb_sum[c][v] += colour[c] for c = 0, 1, 2.
 * The sums are integers (|sum| <= 65535 * 32767 < 2^31, rgb_sum <= 65535 * 255): below saturation, integrating a set of frames in
 * any order gives the same bytes.  Saturation is where that ends: the 65536th frame a voxel sees is dropped, and which one that is
 * depends on the order.
 *
 * Statistics.  out_stats uint64 [8]: voxels updated; of them those with s < tau (not clamped); no depth; occluded; saturated;
 * outside; usable pixels of the frame; 0.  The first six add up to V.
 *
 * Extraction of the zero crossings, with min_weight >= 1.  For voxel v in ascending order and axis a = x, y, z in that order, the
 * neighbour v' is one step along +a and must be inside the volume.  The edge is a CROSSING iff weight(v) >= min_weight,
 * weight(v') >= min_weight and (sum(v) < 0) != (sum(v') < 0).  f0 = (float)sum(v) / (float)weight(v), f1 likewise of v';
 * theta = f0 / (f0 - f1), binary32 (the signs differ, so the divisor is not zero; f0 = 0 against a negative neighbour gives 0).  The
 * point is c(v) of step 1 with coordinate a replaced by fmaf(theta, vs, c_a).  The colour is that of v if theta <= 0.5f, else
 * that of v'; each channel is (2 * rgb_sum + weight) / (2 * weight) in integers -- the mean, rounded half up.  The output is in
 * that order: out_points float32 [][3], out_colors uint8 [][3].  The caller gives a capacity in rows; the call writes
 * min(total, capacity) rows and returns the int64 total; with null outputs (or capacity 0) it only counts.  Rows past the count
 * are left as they were.
 *
 * Every result is a function of integer sums and fixed binary32 arithmetic per voxel: the same bits come out on every run.
 * tests/tsdf_ref.py restates the definition in numpy, each part twice; the device results equal it bit for bit.
 *
 * Not offered: a hashed or sparse volume (the planes are dense: 8 bytes per voxel, 20 with colours); truncation scaled with depth;
 * weights other than 1; normals from the gradient -- sgm_covariance_normals (estimate_normals_radius) on the extracted list serves
 * for now; a marching-cubes mesh; ray casting; a batch of frames per call.
 */
#ifndef SGM_HIP_TSDF_H
#define SGM_HIP_TSDF_H

#include "sgm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One frame into the volume.  Host pointers, blocking: the planes go up, are updated and come down.  dims = (nx, ny, nz);
 * rgb_sum and colors are both null or both given; disp and out_stats may be null.
 * SGM_ERR_INVALID_ARG, with nothing touched and an sgm_last_error that names the entry, for a null e / dims / origin / sum /
 * weight / xyz / cam / extrinsic, colours without rgb_sum or rgb_sum without colours, a front other than +1 or -1, a cam entry,
 * voxel_size, sdf_trunc or origin that is not finite, a voxel_size or sdf_trunc <= 0, a kappa = 32767.0f / sdf_trunc that is not
 * finite, an extrinsic with an entry that is not finite or a last row other than (0, 0, 0, 1), a max_depth that is not > 0, H or
 * W < 1;  SGM_ERR_UNSUPPORTED for a dimension outside 1 .. 4096, V > 2^30 or H * W > 2^27.
 * With SGM_OPT_PROFILE = 1 the stage record (sgm_get_stage_times) is afterwards the call's: tsdf_integrate. */
int sgm_tsdf_integrate(sgm_engine *e, const int32_t dims[3], float voxel_size, float sdf_trunc, const float origin[3], int32_t *sum,
                       int32_t *weight, uint32_t *rgb_sum, const float *xyz, const float *disp, const uint8_t *colors_rgb, int H, int W,
                       const float cam[4], int front, const double extrinsic[16], float max_depth, uint64_t out_stats[8]);

/* The same with DEVICE pointers for the planes and the frame, on the engine's stream; dims, origin, cam, extrinsic and out_stats
 * are host pointers.  Blocks only if out_stats is asked for.  The planes must not overlap each other or the frame. */
int sgm_tsdf_integrate_device(sgm_engine *e, const int32_t dims[3], float voxel_size, float sdf_trunc, const float origin[3], void *d_sum,
                              void *d_weight, void *d_rgb_sum, const void *d_xyz, const void *d_disp, const void *d_colors_rgb, int H, int W,
                              const float cam[4], int front, const double extrinsic[16], float max_depth, uint64_t out_stats[8]);

/* The zero crossings of the volume.  Host pointers, blocking.  out_points has capacity rows of 3 floats, out_colors (null, or
 * with rgb_sum only) capacity rows of 3 bytes; both null or capacity 0: the call only counts.  *out_total is the number of
 * crossings, whatever the capacity.  Never touches the planes.  Refuses like sgm_tsdf_integrate, and min_weight < 1, a null
 * out_total, a negative capacity, out_colors without rgb_sum or without out_points.
 * Stage record: tsdf_count, tsdf_scan and, unless the call only counts, tsdf_emit. */
int sgm_tsdf_extract_points(sgm_engine *e, const int32_t dims[3], float voxel_size, const float origin[3], const int32_t *sum,
                            const int32_t *weight, const uint32_t *rgb_sum, int min_weight, int64_t capacity, float *out_points,
                            uint8_t *out_colors, int64_t *out_total);

/* The same with DEVICE pointers for the planes and the two outputs, on the engine's stream.  Blocks once, for the total.  The
 * engine keeps 12 bytes per 1024 voxels (the blocks' counts and their 64-bit offsets); sgm_trim gives them back. */
int sgm_tsdf_extract_points_device(sgm_engine *e, const int32_t dims[3], float voxel_size, const float origin[3], const void *d_sum,
                                   const void *d_weight, const void *d_rgb_sum, int min_weight, int64_t capacity, void *d_out_points,
                                   void *d_out_colors, int64_t *out_total);

#ifdef __cplusplus
}
#endif
#endif
