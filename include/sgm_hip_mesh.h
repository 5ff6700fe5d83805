/*
 * sgm_hip_mesh.h -- a triangle mesh from the organised cloud on the device: two triangles per pixel quad of the XYZ image of
 * sgm_reproject / sgm_pipeline wherever the disparity is continuous, as a vertex list, optional vertex colours and an indexed face
 * list.  It is the surface over the points sgm_compact_points hands out as a list, and the last step of compute -> filter ->
 * reproject -> cloud.  Included by sgm_hip.h: a caller includes that header and gets this one with it.
 *
 * It is a file of its own for the reason sgm_hip_confidence.h gives: the entry points sgm_hip.h and the headers before this one
 * declare are held, symbol for symbol, against lists fixed earlier; these are bound beside them (_lib.py: MESH_EXPORTS).
 *
 * In user code the place of this call is usually taken by a meshing function of a library such as Open3D.  This is NOT Open3D's
 * meshing nor any other library's: it is the definition below, our own, a pure function of the inputs with the output order fixed
 * by the source order, so that the result is the same bits on every run.  There are no atomics and no tolerance.
 *
 * Definition.
 *
 * Inputs: xyz float32 [H][W][3]; disp float32 [H][W], required (the float disparity of sgm_disp_to_float / sgm_pipeline_device, in
 * pixels); colors_rgb uint8 [H][W][3] or null; max_diff float32, finite, >= 0.  H, W >= 1 and H * W <= 2^26 = 67 108 864 pixels (a
 * 4096 x 2160 frame has 8 847 360); a larger frame is SGM_ERR_UNSUPPORTED.  H < 2 or W < 2 succeeds with 0 vertices and 0 faces.
 *
 *   1. Validity.  Pixel p is valid iff X, Y and Z are all finite and disp[p] > 0.  (The voxel grid's predicate, not the
 *      compaction's, which looks at X alone.)
 *   2. Connection.  Two pixels p, q are connected iff both are valid and fabsf(disp[p] - disp[q]) <= max_diff: one binary32
 *      subtraction, one absolute value, one comparison.  An infinite or NaN difference is not connected.
 *   3. Candidate triangles.  For the quad at (y, x), 0 <= y < H - 1, 0 <= x < W - 1, with the corners a = (y, x), b = (y, x + 1),
 *      c = (y + 1, x), d = (y + 1, x + 1):
 *          on diagonal a-d:  T0 = (a, c, d),  T1 = (a, d, b);      on diagonal b-c:  T2 = (a, c, b),  T3 = (b, c, d).
 *      The quad takes diagonal a-d iff a and d are both valid and either b and c are not both valid or
 *      |disp a - disp d| <= |disp b - disp c| (the differences formed as in step 2; a tie goes to a-d); otherwise it takes b-c.
 *      A triangle of the chosen diagonal is emitted iff all three of its edges are connected; the other diagonal's triangles are
 *      never emitted.  With exactly three valid corners this leaves the one triangle of those three.  The vertex order is the one
 *      listed: for a frame where X grows with x, Y with y and Z away from the camera all four have their normal (q - p) x (r - p)
 *      towards the camera.
 *   4. Vertices.  A pixel is a vertex iff at least one emitted triangle names it.  Vertices come out in row-major order of their
 *      pixels as float32 [V][3], copied bit for bit from xyz; with colors_rgb, colours as uint8 [V][3].  Valid pixels that no
 *      triangle uses are not output.
 *   5. Faces.  int32 [F][3], indices into that vertex list, ordered by quad, row-major; within a quad the first triangle (T0 or
 *      T2) comes before the second (T1 or T3).
 * tests/mesh_ref.py restates this in numpy; the device results equal it bit for bit.
 */
#ifndef SGM_HIP_MESH_H
#define SGM_HIP_MESH_H

#include "sgm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host pointers, blocking.  Outputs are sized by the caller for the worst case: out_vertices float32 [H * W][3], out_colors uint8
 * [H * W][3], out_faces int32 [2 (H - 1)(W - 1)][3]; rows past *n_vertices / *n_faces are left as they were.  Outputs must not
 * overlap inputs or each other.  colors_rgb without out_colors is accepted and ignored.
 * SGM_ERR_INVALID_ARG, with the outputs and the counts untouched, for a null e / xyz / disp / out_vertices / out_faces /
 * n_vertices / n_faces, H < 1 or W < 1, a max_diff that is not finite or < 0, out_colors without colors_rgb;
 * SGM_ERR_UNSUPPORTED for H * W > 2^26.
 * The engine keeps one byte and one 32-bit word per pixel and two 32-bit words per 256 pixels (the host entry also a staging copy of
 * the faces); sgm_trim gives the per-pixel ones back.  With SGM_OPT_PROFILE = 1 the stage record (sgm_get_stage_times) is the
 * call's afterwards: mesh_quads, mesh_used, mesh_scan, mesh_vertices, mesh_faces. */
int sgm_mesh_grid(sgm_engine *e, const float *xyz, const float *disp, const uint8_t *colors_rgb, int H, int W, float max_diff,
                  float *out_vertices, uint8_t *out_colors, int32_t *out_faces, int64_t *n_vertices, int64_t *n_faces);

/* The same with DEVICE pointers for the image data, on the engine's stream; n_vertices and n_faces are host pointers.  Blocks
 * once, at the end, until the two counts are known. */
int sgm_mesh_grid_device(sgm_engine *e, const void *d_xyz, const void *d_disp_f32, const void *d_colors_rgb, int H, int W,
                         float max_diff, void *d_out_vertices, void *d_out_colors, void *d_out_faces,
                         int64_t *n_vertices, int64_t *n_faces);

#ifdef __cplusplus
}
#endif
#endif
