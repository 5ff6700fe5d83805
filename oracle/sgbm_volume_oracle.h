/*
 * sgbm_volume_oracle.h -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * A second C restatement of SURVEY.md Appendix A, in the plain volume form of tests/bruteforce_sgbm.py,
 * tests/bruteforce_hh4.py and tests/bruteforce_color.py: per-channel pre-filter and Birchfield-Tomasi pixel cost summed
 * over 1 or 3 interleaved channels, box sums by direct summation over the clamped window, the recurrence of A.5 run ONCE
 * PER DIRECTION over the whole C volume, S = saturating sum of the directions, selection (A.6), then the frozen
 * oracle's own oracle_median3x3_i16 / oracle_filter_speckles_i16.
 *
 * sgbm_oracle.c is frozen and refuses everything but modes 0 and 1 on one channel; the numpy restatements reach frames
 * of a few thousand pixels.  This file makes MODE_HH4 (mode 3) and colour pairs reachable at full size.  It is pinned by
 * tests/test_volume_oracle.py: bit for bit against the frozen oracle for modes 0 / 1 on one channel, bit for bit against
 * the numpy restatements for mode 3 and three channels.  The numpy files stay the authority for what HH4 and colour mean.
 *
 * Parameters and taps are the frozen oracle's structs (sgbm_oracle.h); the headroom record has the same definition
 * (the running-sum intermediate of A.9 included).  Outside the int16 regime (headroom_ok = 0) the values are those of
 * 16-bit wrap-around in the cost stage and are not claimed equal to anything.
 */
#ifndef SGBM_VOLUME_ORACLE_H
#define SGBM_VOLUME_ORACLE_H

#include "sgbm_oracle.h"

#ifdef __cplusplus
extern "C" {
#endif

/* u8 H x W x channels (interleaved, row stride in bytes) x 2 -> int16 H x W (disp * 16).  mode 0, 1 or 3; channels 1 or 3.
 * returns 0, or < 0 for arguments it does not take */
int volume_oracle_compute(const oracle_sgbm_params *p, const uint8_t *left, const uint8_t *right, int H, int W,
                          int channels, int64_t stride, int16_t *disp, oracle_sgbm_taps *taps);

#ifdef __cplusplus
}
#endif
#endif
