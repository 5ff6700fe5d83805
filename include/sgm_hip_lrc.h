/*
 * sgm_hip_lrc.h -- the left-right consistency confidence: a uint8 map in 0 .. 100 from a left-view and a right-view disparity
 * map, made of the agreement of the two maps and of their roughness around a pixel.  It is what the edge-aware filter of
 * sgm_hip_wls.h is fed with when both maps exist (the uniqueness margin of sgm_hip_confidence.h knows nothing about occlusions).
 * Included by sgm_hip.h: a caller includes that header and gets this one with it.
 *
 * It is a file of its own for the reason sgm_hip_confidence.h gives: the entry points sgm_hip.h and the headers before this one
 * declare are held, symbol for symbol, against lists fixed earlier; these are bound beside them (_lib.py: LRC_EXPORTS).
 *
 * In cv2 user code the place of this map is taken by the confidence cv2.ximgproc's DisparityWLSFilter computes when it is given
 * both maps (LRCthresh, depthDiscontinuityRadius, getConfidenceMap).  This is NOT cv2's computeConfidenceMap bit for bit: it is
 * the definition below, our own, in integers.  cv2's ROI handling is not built, and nothing of cv2's filter is restated here.
 *
 * Definition.
 *
 * Inputs: dl, dr int16 [H][W], disparity * 16.  dr is in this project's right-view convention (sgm_hip_right.h): a valid right
 * pixel (y, x) with disparity d matches left pixel (y, x + d).  `invalid` marks invalid pixels in both maps.  base: uint8 [H][W]
 * in 0 .. 100, or null: the left-view match confidence.  thresh T, 0 .. 32767, in sixteenths (24 is cv2's LRCthresh).  radius r,
 * 0 .. 16.  var_max V, 1 .. 2^30, in sixteenths squared (2304: a standard deviation of three pixels inside the window counts as
 * a depth edge).
 * Outputs: conf_left, conf_right uint8 [H][W] in 0 .. 100.  Either may be null, not both.
 *
 * Everything is integer arithmetic; quantities marked 64 are int64, and no intermediate leaves int64 inside the argument ranges
 * above (tests/lrc_ref.py asserts it, the maps alternating -32768 / 32767 at r = 16 with V = 1 and V = 2^30 included).
 *
 *   1. Smoothness factor of a map M at pixel p.  F_M(p) = 0 if M[p] == invalid.  Otherwise consider the pixels q inside the
 *      image with |qy - py| <= r, |qx - px| <= r and M[q] != invalid.  Let n = their count, s1 = sum M[q], s2 = sum M[q]^2 (64),
 *      num = n * s2 - s1^2 (64, >= 0).  Then F_M(p) = 100 - min(100, (100 * num) / (n^2 * V)), with C integer division.
 *      With r = 0, F is 100 on every valid pixel.
 *   2. Left confidence at (y, x).  Let d = dl[y][x] and xr = x - floor((d + 8) / 16).  The confidence is 0 if d is invalid, if xr
 *      is outside [0, W), if dr[y][xr] is invalid, or if |d - dr[y][xr]| > T.  Otherwise it is min(F_dl(y, x), F_dr(y, xr)), and
 *      also min with base[y][x] when base is given.
 *   3. Right confidence at (y, x).  Let d = dr[y][x] and xl = x + floor((d + 8) / 16).  The confidence is 0 by the same four
 *      conditions, tested against dl[y][xl].  Otherwise it is min(F_dr(y, x), F_dl(y, xl)), and also min with base[y][xl] when
 *      base is given.
 * tests/lrc_ref.py restates this in numpy; the device results equal it bit for bit.
 *
 * Outputs must not overlap inputs: the right confidence reads dl, base and the left map's factor at another column than it
 * writes.  The two outputs must not overlap each other.
 */
#ifndef SGM_HIP_LRC_H
#define SGM_HIP_LRC_H

#include "sgm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host pointers, blocking (the call shape of sgm_wls_filter).  base may be null; one of conf_left / conf_right may be null.
 * SGM_ERR_INVALID_ARG for a null e / disp_left / disp_right, both outputs null, non-positive H or W, thresh outside 0 .. 32767,
 * radius outside 0 .. 16, var_max outside 1 .. 2^30, invalid outside int16, an output pointer equal to an input pointer or to
 * the other output: nothing is enqueued then and the engine stays usable.  The engine keeps the two factor planes, uint8 [H][W]
 * each (2 * H * W bytes, regrown for a larger shape; sgm_trim gives them back).  With SGM_OPT_PROFILE = 1 the stage record
 * (sgm_get_stage_times) is the call's afterwards: lrc_factor, lrc_match. */
int sgm_lrc_confidence(sgm_engine *e, const int16_t *disp_left, const int16_t *disp_right, const uint8_t *base, int H, int W,
                       int invalid, int thresh, int radius, int var_max, uint8_t *conf_left, uint8_t *conf_right);

/* The same with DEVICE pointers, in the order of the engine's stream.  Same refusals; the status of the enqueued work comes
 * through sgm_synchronize. */
int sgm_lrc_confidence_device(sgm_engine *e, const void *d_left_i16, const void *d_right_i16, const void *d_base_u8, int H, int W,
                              int invalid, int thresh, int radius, int var_max, void *d_conf_left_u8, void *d_conf_right_u8);

/* N pairs of maps of one shape, device pointers, in the order of the engine's stream.  d_lefts, d_rights: host arrays of N device
 * pointers; d_bases, d_conf_lefts, d_conf_rights: such arrays, or NULL for "no base" / "no left map" / "no right map" for every
 * pair (not both outputs).  invalid, thresh, radius, var_max are shared by the N pairs.  The pointer arrays are read before the
 * call returns.  Pair i's results equal sgm_lrc_confidence_device on pair i alone, bit for bit.  The batch runs in chunks of C
 * pairs, chunk after chunk on the engine's stream, every launch over all pairs of a chunk: C is chosen as the batch filter
 * chooses it (sgm_hip_wls_batch.h: the smallest of N, 64, SGM_OPT_GROUP_MAX when non-zero, and what free device memory allows);
 * the factor planes grow to [C][2][H][W] and are allocated before anything is enqueued.  The stage record adds up all chunks.
 * SGM_ERR_INVALID_ARG for what sgm_lrc_confidence_device refuses, for N <= 0, a null entry in any array that was given, and an
 * output pointer of any pair equal to an input pointer of any pair or to another output: nothing is enqueued then and the
 * engine stays usable.  N = 1 is valid and equals the single call. */
int sgm_lrc_confidence_batch_device(sgm_engine *e, int N, const void *const *d_lefts, const void *const *d_rights,
                                    const void *const *d_bases, int H, int W, int invalid, int thresh, int radius, int var_max,
                                    void *const *d_conf_lefts, void *const *d_conf_rights);

#ifdef __cplusplus
}
#endif
#endif
