/*
 * sgm_hip_normals.h -- one normal per vertex of the grid mesh of sgm_hip_mesh.h, and the same as a normal image over the organised
 * cloud: the area-weighted sum of the normals of the emitted triangles around a pixel, normalised, and on request turned towards
 * the camera.  It is what a viewer, a lighting pass or a surface reconstruction needs beside the vertices and the faces.  Included
 * by sgm_hip.h: a caller includes that header and gets this one with it.
 *
 * It is a file of its own for the reason sgm_hip_confidence.h gives: the entry points sgm_hip.h and the headers before this one
 * declare are held, symbol for symbol, against lists fixed earlier; these are bound beside them (_lib.py: NORMALS_EXPORTS).
 *
 * In user code the place of these calls is usually taken by Open3D's estimate_normals (on a cloud) or compute_vertex_normals (on a
 * mesh).  This is NOT Open3D's estimate_normals nor its compute_vertex_normals nor any other library's: it is the definition below,
 * our own, a pure function of the inputs with every operation and its order written out, so that the result is the same bits on
 * every run.  There are no atomics and no tolerance.
 *
 * Definition.
 *
 * Inputs: those of sgm_mesh_grid -- xyz float32 [H][W][3]; disp float32 [H][W], required; max_diff float32, finite, >= 0; H, W >= 1
 * and H * W <= 2^26 -- and orient, 0 or 1.  Steps 1 - 3 of sgm_hip_mesh.h decide which triangles are emitted, steps 4 and 5 which
 * pixels are vertices and how they are numbered.  The steps below continue from there.  Every operation is a binary32 operation
 * rounded to nearest, done one at a time in the order written, nothing fused; the divisions and the square root are the correctly
 * rounded ones.
 *
 *   6. Face normal.  For an emitted triangle (p, q, r) in its listed vertex order: e1 = q - p and e2 = r - p, three subtractions
 *      each; n = (e1.y e2.z - e1.z e2.y,  e1.z e2.x - e1.x e2.z,  e1.x e2.y - e1.y e2.x), each component two rounded products and
 *      one subtraction.  It is not normalised: its length weights it by the triangle's area.
 *   7. Sum.  The normal sum s of a pixel starts at (+0, +0, +0) and adds, component by component, the face normals of the emitted
 *      triangles that name the pixel, in face order: first those of the quad above left (the pixel is its corner d), then of the
 *      quad above (c), then of the quad to the left (b), then of its own quad (a); within a quad the first triangle before the
 *      second.  That is at most eight additions per component (six triangles of one diagonal choice, eight when the diagonals
 *      alternate).
 *   8. Normalise.  m = max(|s.x|, |s.y|, |s.z|).  If the pixel is no vertex, or m is zero, infinite or NaN (a NaN component makes
 *      m NaN), the normal is (+0, +0, +0).  Otherwise u = s / m (three divisions), l = sqrtf((u.x u.x + u.y u.y) + u.z u.z), and
 *      the normal is u / l (three divisions).  Dividing by m first keeps l within [1, sqrt 3] for clouds of any unit.
 *   9. Orientation.  With orient = 1: t = (n.x P.x + n.y P.y) + n.z P.z with P the pixel's own point and n the normal of step 8;
 *      if t > 0 all three components change sign (a +0 component becomes -0), so that the normal points into the half space of
 *      the camera at the origin.  The FACES KEEP THEIR WINDING: a vertex normal turned here may point against the winding of the
 *      faces around it.  With orient = 0 the normal is as the winding gives it (for a frame where X grows with x, Y with y and Z
 *      away from the camera: towards the camera).
 * What subnormal intermediates give is whatever IEEE arithmetic gives and is not pinned by a test.
 * tests/normals_ref.py restates this in numpy, twice; the device results equal it bit for bit.
 */
#ifndef SGM_HIP_NORMALS_H
#define SGM_HIP_NORMALS_H

#include "sgm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The normal IMAGE: out_normals float32 [H][W][3], every pixel written, (+0, +0, +0) where the pixel is no vertex.  Host pointers,
 * blocking.  H < 2 or W < 2 (no quad) gives an all-zero image.  The output must not overlap the inputs.
 * SGM_ERR_INVALID_ARG, with the output untouched, for a null e / xyz / disp / out_normals, H < 1 or W < 1, a max_diff that is not
 * finite or < 0, an orient other than 0 and 1; SGM_ERR_UNSUPPORTED for H * W > 2^26.
 * The engine keeps what sgm_mesh_grid keeps and, for the host entries, a staging copy of the normals; sgm_trim gives them back.
 * With SGM_OPT_PROFILE = 1 the stage record is the call's afterwards: mesh_quads, normals_grid. */
int sgm_normals_grid(sgm_engine *e, const float *xyz, const float *disp, int H, int W, float max_diff, int orient, float *out_normals);

/* The same with DEVICE pointers, in the order of the engine's stream: it returns without waiting for the image. */
int sgm_normals_grid_device(sgm_engine *e, const void *d_xyz, const void *d_disp_f32, int H, int W, float max_diff, int orient,
                            void *d_out_normals);

/* The mesh of sgm_mesh_grid, bit for bit, and beside it out_normals float32 [V][3]: one row per vertex, in vertex order -- the rows
 * of the normal image at the vertices' pixels.  Host pointers, blocking.  Arguments, sizes and refusals are those of sgm_mesh_grid;
 * out_normals is required and sized like out_vertices, float32 [H * W][3], and an orient other than 0 and 1 is
 * SGM_ERR_INVALID_ARG.  The stage record: that of sgm_mesh_grid, then mesh_normals. */
int sgm_mesh_grid_normals(sgm_engine *e, const float *xyz, const float *disp, const uint8_t *colors_rgb, int H, int W, float max_diff,
                          int orient, float *out_vertices, uint8_t *out_colors, int32_t *out_faces, float *out_normals,
                          int64_t *n_vertices, int64_t *n_faces);

/* The same with DEVICE pointers for the image data, on the engine's stream; n_vertices and n_faces are host pointers.  Blocks
 * once, at the end, until the two counts are known. */
int sgm_mesh_grid_normals_device(sgm_engine *e, const void *d_xyz, const void *d_disp_f32, const void *d_colors_rgb, int H, int W,
                                 float max_diff, int orient, void *d_out_vertices, void *d_out_colors, void *d_out_faces,
                                 void *d_out_normals, int64_t *n_vertices, int64_t *n_faces);

#ifdef __cplusplus
}
#endif
#endif
