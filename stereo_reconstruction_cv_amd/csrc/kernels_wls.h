// kernels_wls.h -- the edge-aware disparity filter (include/sgm_hip_wls.h: sgm_wls_filter): a confidence-weighted,
// image-guided fast global smoother (Min et al., "Fast Global Image Smoothing Based on Weighted Least Squares", 2014).
//
// Three float planes u (disparity * confidence), v (confidence) and c' (the Thomas algorithm's modified upper diagonal)
// are smoothed line by line: all rows, then all columns, three times with a falling lambda; the result is u / v.  The
// arithmetic of a line is the contract of the header -- IEEE binary32, every operation rounded on its own, in the order
// written there -- so nothing here is reassociated, fused (the library is built with -ffp-contract=off) or split: one lane
// walks one line from end to end and back.  What the kernels arrange is only where a lane's operands come from:
//   k_wls_rows   one lane per ROW.  Wave 0 of a workgroup owns 64 rows and walks them in tiles of TC columns; a tile of u, v
//                and of the edge weights is brought into LDS with row-major (coalesced) accesses, rows padded to TC + 1 floats
//                so that the 64 lanes of a column step hit 64 banks, and goes back the same way.  The other RW - 1 waves do
//                nothing but help with that traffic, so that a tile's loads are in flight together.
//   k_wls_cols   one lane per COLUMN: the lanes of a wave touch 64 adjacent floats of a row at every step.  Rows are
//                fetched UNR at a time before the dependent chain consumes them.
// The edge weights are looked up on the fly, lut[|g_i - g_{i+1}|] (3 channels: the largest of the three differences), from
// the 256-entry table that travels as a kernel argument and sits in LDS.
//
// Every kernel runs over a chunk of up to BATCH_MAPS_MAX maps of one shape: blockIdx.y is the map, and a single map
// (sgm_wls_filter) is a chunk of one.  The planes u, v, c' of map m are the m-th [H][W] slice of the engine's three buffers
// (64-bit offsets: 64 planes of a 4K map pass 2^31 bytes); the maps' own pointers -- map, guide, confidence, outputs -- travel as by-value tables
// in the kernel arguments (MapPtrs, sgm_device.h), each kernel with the tables it reads, so nothing is copied to the device
// for them and nothing of them outlives the launch.  A map's tail workgroup is cut to its own rows / columns, so it touches
// no neighbour's plane.
// How many workgroups share a CU depends on the chunk, so the shape of the row kernel is a template argument -- RW waves per
// workgroup, tiles of TC columns (LDS: 3 * 64 * (TC + 1) floats + the table) -- and so are the rows in flight of the column
// kernel; sgm_engine.hip says which are used and DESIGN.md 4.15 / 4.16 what each gave.  Every shape gives the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sgm_device.h"

namespace sgm {

constexpr int WLS_T = 64;       // rows per workgroup of k_wls_rows; columns (= lanes, one wave) of k_wls_cols

struct WlsLut { float w[256]; };

__device__ inline void wls_lut_to_lds(const WlsLut &lut, float *sl)
{
    for (int i = threadIdx.x; i < 256; i += blockDim.x) sl[i] = lut.w[i];
    __syncthreads();
}

// table index of the neighbours at pixel indices i and j of a tight CN-channel guide
template <int CN>
__device__ inline int wls_gdiff(const uint8_t *__restrict__ g, int64_t i, int64_t j)
{
    int d = abs((int)g[i * CN] - (int)g[j * CN]);
    if (CN == 3) {
        d = max(d, abs((int)g[i * 3 + 1] - (int)g[j * 3 + 1]));
        d = max(d, abs((int)g[i * 3 + 2] - (int)g[j * 3 + 2]));
    }
    return d;
}

// The forward step of one line element: kp = k_{i-1} (unused when first), k = k_i (unused when last); cp / up / vp come in as
// the primed values of element i - 1 and leave as those of element i; u, v: x_i of the two right-hand sides.
__device__ inline void wls_forward(bool first, bool last, float kp, float k, float u, float v, float &cp, float &up, float &vp)
{
    const float a = first ? 0.f : -kp, c = last ? 0.f : -k;
    const float b = (1.f - a) - c;
    if (first) {
        const float r = 1.f / b;
        cp = c * r;
        up = u * r;
        vp = v * r;
    } else {
        const float m = b - a * cp;
        const float r = 1.f / m;
        cp = c * r;
        up = (u - a * up) * r;
        vp = (v - a * vp) * r;
    }
}

// u = disp * c, v = c with c = 0 where disp is invalid, else the confidence (100 without a map)
__global__ __launch_bounds__(256) void k_wls_init(MapPtrs disps, MapPtrs confs, int invalid, int64_t n, float *__restrict__ u,
                                                  float *__restrict__ v)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int16_t *__restrict__ disp = (const int16_t *)disps.p[blockIdx.y];
    const uint8_t *__restrict__ conf = (const uint8_t *)confs.p[blockIdx.y];
    const int64_t o = (int64_t)blockIdx.y * n + i;
    const int d = disp[i];
    const bool ok = d != invalid;
    const float c = ok ? (conf ? (float)conf[i] : 100.f) : 0.f;
    u[o] = ok ? (float)d * c : 0.f;
    v[o] = c;
}

template <int CN, int RW, int TC>
__global__ __launch_bounds__(RW * WLS_T) void k_wls_rows(float *__restrict__ u, float *__restrict__ v, float *__restrict__ cpl,
                                                         MapPtrs guides, WlsLut lut, float lam, int H, int W)
{
    constexpr int LD = TC + 1;                  // floats per LDS tile row: odd, so the 64 lanes of a column step hit 64 banks
    constexpr int RS = RW * WLS_T / TC;         // tile rows the workgroup's threads cover at once
    static_assert(RW * WLS_T % TC == 0 && WLS_T % RS == 0, "the threads cover whole tile rows, and the tile in whole sweeps");
    __shared__ float su[WLS_T * LD], sv[WLS_T * LD], sc[WLS_T * LD], sl[256];
    wls_lut_to_lds(lut, sl);
    const int64_t plane = (int64_t)blockIdx.y * H * W;
    u += plane;
    v += plane;
    cpl += plane;
    const uint8_t *__restrict__ guide = (const uint8_t *)guides.p[blockIdx.y];
    const int tc = threadIdx.x % TC, tr = threadIdx.x / TC, y0 = blockIdx.x * WLS_T;
    const int rows = min(WLS_T, H - y0), ntile = (W + TC - 1) / TC;
    const bool walker = (int)threadIdx.x < rows;                                       // (rows <= 64: lanes of wave 0)
    const int wl = threadIdx.x & (WLS_T - 1);
    float *const mu = su + wl * LD, *const mv = sv + wl * LD, *const mc = sc + wl * LD;   // the walker's row
    float kp = 0.f, cp = 0.f, up = 0.f, vp = 0.f;
    for (int t = 0; t < ntile; t++) {
        const int x0 = t * TC, x = x0 + tc, nc = min(TC, W - x0);
        if (x < W) {
#pragma unroll
            for (int j = 0; j < WLS_T / RS; j++) {
                const int r = tr + RS * j;
                if (r < rows) {
                    const int64_t i = (int64_t)(y0 + r) * W + x;
                    su[r * LD + tc] = u[i];
                    sv[r * LD + tc] = v[i];
                    sc[r * LD + tc] = x < W - 1 ? sl[wls_gdiff<CN>(guide, i, i + 1)] : 0.f;   // the weight w_x
                }
            }
        }
        __syncthreads();
        if (walker) {
            for (int c = 0; c < nc; c++) {
                const float k = lam * mc[c];
                wls_forward(x0 + c == 0, x0 + c == W - 1, kp, k, mu[c], mv[c], cp, up, vp);
                mc[c] = cp;
                mu[c] = up;
                mv[c] = vp;
                kp = k;
            }
        }
        __syncthreads();
        if (x < W) {
#pragma unroll
            for (int j = 0; j < WLS_T / RS; j++) {
                const int r = tr + RS * j;
                if (r < rows) {
                    const int64_t i = (int64_t)(y0 + r) * W + x;
                    u[i] = su[r * LD + tc];
                    v[i] = sv[r * LD + tc];
                    cpl[i] = sc[r * LD + tc];
                }
            }
        }
        __syncthreads();
    }
    // back substitution, the tiles in reverse: up / vp now carry x_{i+1}
    for (int t = ntile - 1; t >= 0; t--) {
        const int x0 = t * TC, x = x0 + tc, nc = min(TC, W - x0);
        if (x < W) {
#pragma unroll
            for (int j = 0; j < WLS_T / RS; j++) {
                const int r = tr + RS * j;
                if (r < rows) {
                    const int64_t i = (int64_t)(y0 + r) * W + x;
                    su[r * LD + tc] = u[i];
                    sv[r * LD + tc] = v[i];
                    sc[r * LD + tc] = cpl[i];
                }
            }
        }
        __syncthreads();
        if (walker) {
            for (int c = nc - 1; c >= 0; c--) {
                if (x0 + c == W - 1) {
                    up = mu[c];
                    vp = mv[c];
                } else {
                    const float cc = mc[c];
                    up = mu[c] - cc * up;
                    vp = mv[c] - cc * vp;
                }
                mu[c] = up;
                mv[c] = vp;
            }
        }
        __syncthreads();
        if (x < W) {
#pragma unroll
            for (int j = 0; j < WLS_T / RS; j++) {
                const int r = tr + RS * j;
                if (r < rows) {
                    const int64_t i = (int64_t)(y0 + r) * W + x;
                    u[i] = su[r * LD + tc];
                    v[i] = sv[r * LD + tc];
                }
            }
        }
        __syncthreads();
    }
}

template <int CN, int UNR>
__global__ __launch_bounds__(WLS_T) void k_wls_cols(float *__restrict__ u, float *__restrict__ v, float *__restrict__ cpl,
                                                    MapPtrs guides, WlsLut lut, float lam, int H, int W)
{
    __shared__ float sl[256];
    wls_lut_to_lds(lut, sl);
    const int x = blockIdx.x * WLS_T + threadIdx.x;
    if (x >= W) return;
    const int64_t plane = (int64_t)blockIdx.y * H * W;
    u += plane;
    v += plane;
    cpl += plane;
    const uint8_t *__restrict__ guide = (const uint8_t *)guides.p[blockIdx.y];
    float kp = 0.f, cp = 0.f, up = 0.f, vp = 0.f;
    for (int y0 = 0; y0 < H; y0 += UNR) {
        float uu[UNR], vv[UNR], ww[UNR];
#pragma unroll
        for (int j = 0; j < UNR; j++) {
            const int y = y0 + j;
            if (y < H) {
                const int64_t i = (int64_t)y * W + x;
                uu[j] = u[i];
                vv[j] = v[i];
                ww[j] = y < H - 1 ? sl[wls_gdiff<CN>(guide, i, i + W)] : 0.f;
            }
        }
#pragma unroll
        for (int j = 0; j < UNR; j++) {
            const int y = y0 + j;
            if (y < H) {
                const int64_t i = (int64_t)y * W + x;
                const float k = lam * ww[j];
                wls_forward(y == 0, y == H - 1, kp, k, uu[j], vv[j], cp, up, vp);
                cpl[i] = cp;
                u[i] = up;
                v[i] = vp;
                kp = k;
            }
        }
    }
    for (int y0 = (H - 1) / UNR * UNR; y0 >= 0; y0 -= UNR) {
        float uu[UNR], vv[UNR], cc[UNR];
#pragma unroll
        for (int j = UNR - 1; j >= 0; j--) {
            const int y = y0 + j;
            if (y < H) {
                const int64_t i = (int64_t)y * W + x;
                uu[j] = u[i];
                vv[j] = v[i];
                cc[j] = cpl[i];
            }
        }
#pragma unroll
        for (int j = UNR - 1; j >= 0; j--) {
            const int y = y0 + j;
            if (y < H) {
                const int64_t i = (int64_t)y * W + x;
                if (y == H - 1) {
                    up = uu[j];
                    vp = vv[j];
                } else {
                    up = uu[j] - cc[j] * up;
                    vp = vv[j] - cc[j] * vp;
                }
                u[i] = up;
                v[i] = vp;
            }
        }
    }
}

// valid iff v >= 1 (one percent of full confidence reached the pixel): out = rint(u / v), out_f32 = (u / v) / 16
__global__ __launch_bounds__(256) void k_wls_final(const float *__restrict__ u, const float *__restrict__ v, int invalid, int64_t n,
                                                   MapPtrs outs, MapPtrs outfs)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int16_t *__restrict__ out = (int16_t *)outs.p[blockIdx.y];
    float *__restrict__ out_f32 = (float *)outfs.p[blockIdx.y];
    const int64_t o = (int64_t)blockIdx.y * n + i;
    const float vi = v[o];
    const bool ok = vi >= 1.f;
    const float q = ok ? u[o] / vi : 0.f;
    out[i] = ok ? (int16_t)fminf(fmaxf(rintf(q), -32768.f), 32767.f) : (int16_t)invalid;
    if (out_f32) out_f32[i] = ok ? q * 0.0625f : 0.f;
}

}  // namespace sgm
