/*
 * sgm_hip_wls_batch.h -- the batch form of the edge-aware disparity post-filter of sgm_hip_wls.h: N maps of one shape per call.
 * Included by sgm_hip.h: a caller includes that header and gets this one with it.
 *
 * A file of its own for the reason sgm_hip_confidence.h gives: the entry points sgm_hip.h and sgm_hip_wls.h declare are held,
 * symbol for symbol, against lists fixed earlier; these are bound beside them (_lib.py: WLS_BATCH_EXPORTS).
 *
 * Why it exists.  One lane walks one line of a map from end to end and back (sgm_hip_wls.h, step 4), so a single 4K map gives
 * the GPU 34 + 60 waves and the time of a pass follows the line length.  A batch multiplies the lanes and leaves the chain as
 * long as it was: the arithmetic of a line, its order and the results are those of the single call.
 *
 * The definition is that of sgm_hip_wls.h, applied to every map on its own.  cn, invalid, lambda and lut are shared by the N
 * maps.  The batch is filtered in chunks of C maps, chunk after chunk on the engine's stream: C is the smallest of N, 64,
 * SGM_OPT_GROUP_MAX when that option is non-zero, and what free device memory allows beside the reserve the batch entries of
 * sgm_hip.h keep (4 GiB or 5 %).  The engine's three float planes grow to [C][H][W] (12 * C * H * W bytes; sgm_trim gives them
 * back).  Everything the call allocates is allocated before anything is enqueued: an allocation that fails returns its error
 * with nothing in flight.  With SGM_OPT_PROFILE = 1 the stage record (sgm_get_stage_times) is the call's afterwards: wls_init,
 * wls_rows, wls_cols, wls_final, all chunks and iterations added up.
 */
#ifndef SGM_HIP_WLS_BATCH_H
#define SGM_HIP_WLS_BATCH_H

#include "sgm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* N maps of one shape, device pointers, in the order of the engine's stream.  d_disp_i16, d_guide_u8, d_out_i16: host arrays of
 * N device pointers; d_conf_u8 and d_out_f32: such arrays, or NULL for "no confidence map" / "no float map" for every map.
 * cn, invalid, lambda, lut are shared by the N maps.  The pointer arrays and lut are read before the call returns.
 * d_out_i16[i] may be d_disp_i16[i]; guides may be shared between maps; the outputs of different maps must not overlap.
 * Map i's results equal sgm_wls_filter_device on map i alone, bit for bit (the definition of sgm_hip_wls.h).
 * SGM_ERR_INVALID_ARG for what sgm_wls_filter_device refuses, for N <= 0, a null required array and a null entry in any array
 * that was given: nothing is enqueued then and the engine stays usable.  N = 1 is valid and equals the single call. */
int sgm_wls_filter_batch_device(sgm_engine *e, int N, const void *const *d_disp_i16, const void *const *d_guide_u8, int cn,
                                const void *const *d_conf_u8, int H, int W, int invalid, double lambda, const float lut[256],
                                void *const *d_out_i16, void *const *d_out_f32);
/* Host pointers, blocking: disp [N][H][W], guide [N][H][W](*cn), conf [N][H][W] or NULL, out [N][H][W] (may be disp),
 * out_f32 [N][H][W] or NULL, all tight.  Staged chunk by chunk through buffers the engine owns. */
int sgm_wls_filter_batch(sgm_engine *e, int N, const int16_t *disp, const uint8_t *guide, int cn, const uint8_t *conf, int H, int W,
                         int invalid, double lambda, const float lut[256], int16_t *out, float *out_f32);

#ifdef __cplusplus
}
#endif
#endif
