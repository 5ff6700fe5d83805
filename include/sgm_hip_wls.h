/*
 * sgm_hip_wls.h -- the edge-aware disparity post-filter: a confidence-weighted, image-guided fast global smoother (FGS: Min et
 * al., "Fast Global Image Smoothing Based on Weighted Least Squares", 2014) over a disparity map.  It fills the holes the
 * uniqueness test, the LR check and the speckle filter cut from confident neighbours, removes outliers and keeps depth edges
 * where the guide image has edges.  Included by sgm_hip.h: a caller includes that header and gets this one with it.
 *
 * It is a file of its own for the reason sgm_hip_confidence.h gives: the entry points sgm_hip.h itself declares are held,
 * symbol for symbol, against lists fixed earlier; these are bound beside them (_lib.py: WLS_EXPORTS).
 *
 * In cv2 user code the place of this filter is taken by cv2.ximgproc.createDisparityWLSFilter.  This is NOT that filter bit
 * for bit: it is the definition below, our own.  cv2's filter computes an LR-consistency confidence with a depth-discontinuity
 * radius when it is given both maps; what this library offers in that place is the confidence of sgm_hip_lrc.h (a definition of
 * our own as well), fed into this filter as `conf`.  What remains unbuilt: cv2's ROI handling, and bit parity with cv2.
 *
 * Definition.  Inputs: disp int16 [H][W] (disparity * 16); `invalid`, the value that marks invalid pixels (the engine's maps
 * use (minDisparity - 1) * 16); guide uint8 [H][W] or interleaved [H][W][3] (cn = 1 or 3), tight; conf uint8 [H][W] in
 * 0 .. 100, or null; lambda, 0 <= lambda <= 1e7; lut, 256 floats, the edge weights.  Outputs: out int16 [H][W] (may be the
 * buffer of disp) and, optionally, out_f32 float [H][W].
 *
 * All arithmetic is IEEE binary32; every operation below is rounded on its own, in the order written: no fused multiply-add,
 * no approximate reciprocal, subnormals kept.
 *   1. Start.  c = 0 where disp == invalid, elsewhere float(conf), or 100 when conf is null.  u = float(disp) * c where valid,
 *      else 0.  v = c.
 *   2. Weights.  Neighbours i, i + 1 of a line get w_i = lut[|g_i - g_{i+1}|]; for cn = 3 the index is the largest of the three
 *      channels' absolute differences.
 *   3. Iterations.  T = 3; lambda_t = float(1.5 * lambda * 4^(T-t) / (4^T - 1)), computed in double on the host, t = 1, 2, 3.
 *      Each iteration is a pass over all rows (u and v both), then a pass over all columns.
 *   4. One line of length n (Thomas algorithm), k_i = lambda_t * w_i for i = 0 .. n - 2:
 *        a_i = -k_{i-1} with a_0 = 0;  c_i = -k_i with c_{n-1} = 0;  b_i = (1 - a_i) - c_i.
 *        Forward:  r = 1 / b_0; c'_0 = c_0 * r; x'_0 = x_0 * r;  for i >= 1: m = b_i - a_i * c'_{i-1}; r = 1 / m;
 *                  c'_i = c_i * r; x'_i = (x_i - a_i * x'_{i-1}) * r.
 *        Backward: x_{n-1} = x'_{n-1}; x_i = x'_i - c'_i * x_{i+1}.
 *      c' is shared by u and v; n = 1 is the identity.
 *   5. Finish.  A pixel is valid iff v >= 1.0f (at least one percent of full confidence reached it).  Valid: q = u / v,
 *      out = clamp(rint(q), -32768, 32767) with round-half-even, out_f32 = q * 0.0625f.  Invalid: out = invalid, out_f32 = 0.
 * tests/wls_ref.py restates this in numpy; the device results equal it bit for bit.
 */
#ifndef SGM_HIP_WLS_H
#define SGM_HIP_WLS_H

#include "sgm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The default edge weights: lut[k] = float(exp(-k / sigma)), the exp in double, k = 0 .. 255.  Host only, needs no GPU and no
 * engine.  SGM_ERR_INVALID_ARG for a null lut and for a sigma that is <= 0 or not finite. */
int sgm_wls_weights(double sigma, float lut[256]);

/* Host pointers, blocking (the call shape of sgm_median3x3).  conf and out_f32 may be null; out may be disp.
 * SGM_ERR_INVALID_ARG for a null e / disp / guide / lut / out, non-positive H or W, cn not 1 or 3, lambda outside [0, 1e7] or
 * not finite, invalid outside int16: nothing is enqueued then and the engine stays usable.  The engine keeps three float
 * planes [H][W] for the filter (12 * H * W bytes, regrown for a larger shape; sgm_trim gives them back).  With
 * SGM_OPT_PROFILE = 1 the stage record (sgm_get_stage_times) is the filter's afterwards: wls_init, wls_rows, wls_cols,
 * wls_final, the three iterations added up. */
int sgm_wls_filter(sgm_engine *e, const int16_t *disp, const uint8_t *guide, int cn, const uint8_t *conf, int H, int W,
                   int invalid, double lambda, const float lut[256], int16_t *out, float *out_f32);

/* The same with DEVICE pointers for disp, guide, conf, out and out_f32, in the order of the engine's stream; lut stays a host
 * pointer and is read before the call returns.  Same refusals; the status of the enqueued work comes through
 * sgm_synchronize. */
int sgm_wls_filter_device(sgm_engine *e, const void *d_disp_i16, const void *d_guide_u8, int cn, const void *d_conf_u8, int H,
                          int W, int invalid, double lambda, const float lut[256], void *d_out_i16, void *d_out_f32);

#ifdef __cplusplus
}
#endif
#endif
