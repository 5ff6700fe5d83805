/*
 * sgm_hip_right.h -- the device binding of the right-view disparity map (SGM_OPT_RIGHT_VIEW, SGM_TAP_RIGHT_RAW,
 * SGM_TAP_RIGHT: sgm_hip.h).  Included by sgm_hip.h: a caller includes that header and gets this one with it.
 *
 * A file of its own for the reason sgm_hip_confidence.h is one: the entry points sgm_hip.h itself declares are held, symbol
 * for symbol, against the binding's export list and the load list of the plain-C smoke program (tests/c/abi_smoke.c); an
 * entry point added after those lists were fixed is declared here and bound beside them (_lib.py: RIGHT_EXPORTS).
 */
#ifndef SGM_HIP_RIGHT_H
#define SGM_HIP_RIGHT_H

#include "sgm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* SGM_OPT_RIGHT_VIEW = 1 only: N device pointers to tight int16 [H][W] maps for the NEXT image call on e --
 * sgm_compute_device or sgm_pipeline_device (N = 1), or sgm_pipeline_batch_device (N = its N; pair after pair and chained
 * groups alike).  Pair i's final right-view map (SGM_TAP_RIGHT) is written to d_right_i16[i] in stream order instead of the
 * engine's own buffer.  The binding is consumed by that call, whether it succeeds or fails; N = 0 clears it.
 * SGM_ERR_INVALID_ARG if the option is off or a pointer is null; an N that differs from the image call's pair count is
 * reported by the image call.  The host entries (sgm_compute, sgm_compute_batch) drop a binding unused: after sgm_compute
 * the map is read through the taps. */
int sgm_bind_right_device(sgm_engine *e, int N, void *const *d_right_i16);

#ifdef __cplusplus
}
#endif
#endif
