// kernels_lrc.h -- the left-right consistency confidence (include/sgm_hip_lrc.h: sgm_lrc_confidence): a uint8 map in 0 .. 100
// from a left-view and a right-view disparity map.  Integer arithmetic throughout; the header's definition is the contract.
//
//   k_lrc_factor   the smoothness factor F of BOTH maps of every pair of a chunk in one launch: blockIdx.z = 2 * pair + side.
//                  A workgroup owns a tile of LRC_TW x LRC_TH pixels.  It brings the tile with its r-wide halo into LDS (pixels
//                  outside the image enter as `invalid`, which is how the definition treats them), forms the ROW sums
//                  (n, s1, s2) of every tile row, halo rows included, then the COLUMN sums of those and the factor.  The window
//                  sums are separable, so a pixel costs 2 * (2r + 1) LDS reads instead of (2r + 1)^2.
//   k_lrc_match    the two gathers and the min: one lane per pixel, left and right confidence of a pair in one pass.
// The maps' own pointers travel as by-value tables (MapPtrs of sgm_device.h), as in the edge-aware filter; the factor planes of a
// chunk are one buffer of the engine, uint8 [pairs][2][H][W], addressed with 64-bit offsets.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sgm_device.h"

namespace sgm {

constexpr int LRC_TW = 64, LRC_TH = 16;   // the tile of k_lrc_factor
constexpr int LRC_THREADS = 256;
constexpr int LRC_RMAX = 16;

// LDS of k_lrc_factor at radius r, in this order: s2 int64 [rows][TW], s1 int32 [rows][TW], raw int16 [rows][cols],
// n uint8 [rows][TW] with rows = TH + 2r, cols = TW + 2r.  48 KiB at r = 16.
inline size_t lrc_lds_bytes(int r)
{
    const size_t rows = LRC_TH + 2 * r, cols = LRC_TW + 2 * r;
    return rows * LRC_TW * (8 + 4 + 1) + rows * cols * 2;
}

// 100 - min(100, (100 * num) / (n^2 * V)) with num = n * s2 - s1^2, all int64.  The quotient is only wanted up to 100, so it is
// found as the largest k in 0 .. 100 with k * den <= 100 * num: seven multiply-compares, the same integer as the division for
// every input (den > 0), and no 64-bit divide.  Largest operands: 100 * num and 100 * den, both under 2^57 (sgm_hip_lrc.h).
__host__ __device__ inline int lrc_factor(int n, int64_t s1, int64_t s2, int64_t vmax)
{
    const int64_t a = 100 * ((int64_t)n * s2 - s1 * s1), den = (int64_t)n * n * vmax;
    int lo = 0, hi = 100;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((int64_t)mid * den <= a) lo = mid;
        else hi = mid - 1;
    }
    return 100 - lo;
}

__global__ __launch_bounds__(LRC_THREADS) void k_lrc_factor(MapPtrs lefts, MapPtrs rights, int invalid, int r, int64_t vmax, int H,
                                                            int W, uint8_t *__restrict__ fac)
{
    extern __shared__ __align__(8) unsigned char lrc_lds[];
    const int rows = LRC_TH + 2 * r, cols = LRC_TW + 2 * r, win = 2 * r + 1;
    int64_t *const s2 = (int64_t *)lrc_lds;
    int32_t *const s1 = (int32_t *)(s2 + rows * LRC_TW);
    int16_t *const raw = (int16_t *)(s1 + rows * LRC_TW);
    uint8_t *const cnt = (uint8_t *)(raw + rows * cols);
    const int z = blockIdx.z, tid = threadIdx.x;
    const int16_t *__restrict__ M = (const int16_t *)((z & 1) ? rights.p[z >> 1] : lefts.p[z >> 1]);
    const int x0 = blockIdx.x * LRC_TW, y0 = blockIdx.y * LRC_TH;
    // the tile and its halo; what lies outside the image counts as invalid
    for (int i = tid; i < rows * cols; i += LRC_THREADS) {
        const int ry = i / cols, rx = i - ry * cols, y = y0 - r + ry, x = x0 - r + rx;
        raw[i] = (y >= 0 && y < H && x >= 0 && x < W) ? M[(int64_t)y * W + x] : (int16_t)invalid;
    }
    __syncthreads();
    // row sums: entry (ry, tx) covers raw[ry][tx .. tx + 2r]
    for (int i = tid; i < rows * LRC_TW; i += LRC_THREADS) {
        const int16_t *p = raw + (i / LRC_TW) * cols + (i % LRC_TW);
        int n = 0, a = 0;
        int64_t b = 0;
        for (int k = 0; k < win; k++) {
            const int v = p[k];
            if (v != invalid) {
                n++;
                a += v;
                b += v * v;      // (at most 2^30)
            }
        }
        cnt[i] = (uint8_t)n;
        s1[i] = a;
        s2[i] = b;
    }
    __syncthreads();
    // column sums of the row sums, and the factor
    const int tx = tid % LRC_TW, x = x0 + tx;
    for (int ty = tid / LRC_TW; ty < LRC_TH; ty += LRC_THREADS / LRC_TW) {
        const int y = y0 + ty;
        if (x >= W || y >= H) continue;
        int f = 0;
        if (raw[(ty + r) * cols + tx + r] != invalid) {
            int n = 0;
            int64_t a = 0, b = 0;
            for (int k = 0; k < win; k++) {
                const int j = (ty + k) * LRC_TW + tx;
                n += cnt[j];
                a += s1[j];
                b += s2[j];
            }
            f = lrc_factor(n, a, b, vmax);
        }
        fac[((int64_t)z * H + y) * W + x] = (uint8_t)f;
    }
}

// one of the two confidences at column x of a row: d the map's own value there, xo the matching column in the other map's row
// `other`; f_own / f_other the factor rows; base_at: the column base is read at (the LEFT pixel of the match)
__device__ inline int lrc_one(int d, int xo, int x, const int16_t *__restrict__ other, const uint8_t *__restrict__ f_own,
                              const uint8_t *__restrict__ f_other, const uint8_t *__restrict__ base, int base_at, int invalid,
                              int thresh, int W)
{
    if (d == invalid || xo < 0 || xo >= W) return 0;
    const int e = other[xo];
    if (e == invalid || abs(d - e) > thresh) return 0;
    int c = min((int)f_own[x], (int)f_other[xo]);
    if (base) c = min(c, (int)base[base_at]);
    return c;
}

__global__ __launch_bounds__(256) void k_lrc_match(MapPtrs lefts, MapPtrs rights, MapPtrs bases, int invalid, int thresh, int H, int W,
                                                   const uint8_t *__restrict__ fac, MapPtrs conf_lefts, MapPtrs conf_rights)
{
    const int x = blockIdx.x * 256 + threadIdx.x, m = blockIdx.z;
    if (x >= W) return;
    const int64_t row = (int64_t)blockIdx.y * W, plane = (int64_t)H * W;
    const int16_t *__restrict__ dl = (const int16_t *)lefts.p[m] + row, *__restrict__ dr = (const int16_t *)rights.p[m] + row;
    const uint8_t *__restrict__ base = bases.p[m] ? (const uint8_t *)bases.p[m] + row : nullptr;
    const uint8_t *__restrict__ fl = fac + 2 * m * plane + row, *__restrict__ fr = fl + plane;
    uint8_t *const cl = (uint8_t *)conf_lefts.p[m], *const cr = (uint8_t *)conf_rights.p[m];
    if (cl) {
        const int d = dl[x], xr = x - ((d + 8) >> 4);      // (arithmetic shift: floor)
        cl[row + x] = (uint8_t)lrc_one(d, xr, x, dr, fl, fr, base, x, invalid, thresh, W);
    }
    if (cr) {
        const int d = dr[x], xl = x + ((d + 8) >> 4);
        cr[row + x] = (uint8_t)lrc_one(d, xl, x, dl, fr, fl, base, xl, invalid, thresh, W);
    }
}

}  // namespace sgm
