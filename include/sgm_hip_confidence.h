/*
 * sgm_hip_confidence.h -- the device binding of the per-pixel match confidence (SGM_OPT_CONFIDENCE, SGM_TAP_CONF_RAW,
 * SGM_TAP_CONF: sgm_hip.h).  Included by sgm_hip.h: a caller includes that header and gets this one with it.
 *
 * It is a file of its own because the list of entry points that sgm_hip.h itself declares is held, symbol for symbol,
 * against the binding's export list and against the load list of the plain-C smoke program (tests/c/abi_smoke.c); an entry
 * point added after those lists were fixed is declared here and bound beside them (_lib.py: CONFIDENCE_EXPORTS).
 */
#ifndef SGM_HIP_CONFIDENCE_H
#define SGM_HIP_CONFIDENCE_H

#include "sgm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* SGM_OPT_CONFIDENCE = 1 only: N device pointers to tight uint8 [H][W] maps for the NEXT image call on e --
 * sgm_compute_device or sgm_pipeline_device (N = 1), or sgm_pipeline_batch_device (N = its N).  Pair i's final confidence
 * map (SGM_TAP_CONF) is written to d_conf_u8[i] in stream order instead of the engine's own buffer.  The binding is
 * consumed by that call, whether it succeeds or fails; N = 0 clears it.  SGM_ERR_INVALID_ARG if the option is off or a
 * pointer is null; an N that differs from the image call's pair count is reported by the image call.  The host entries
 * (sgm_compute, sgm_compute_batch) drop a binding unused: after sgm_compute the map is read through the taps. */
int sgm_bind_confidence_device(sgm_engine *e, int N, void *const *d_conf_u8);

#ifdef __cplusplus
}
#endif
#endif
