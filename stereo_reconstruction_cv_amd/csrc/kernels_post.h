// kernels_post.h -- everything after the aggregated cost: right-view map + sub-pixel + LR check,
// 3x3 median, speckle filter (parallel connected components), float scaling/masking,
// reprojection to XYZ and the validity mask.
//
// Replaces, in order: the tail of upstream computeDisparitySGBM, medianBlur(disp, disp, 3) and
// filterSpeckles inside stereo.compute (/root/reference/main.ipynb:668),
// the numpy lines main.ipynb:668-670, cv2.reprojectImageTo3D (main.ipynb:697; SURVEY.md
// Appendix B) and the mask of main.ipynb:726-730.  CPU restatement: oracle/sgbm_oracle.c.
#pragma once
#include "kernels_cost.h"
#include "kernels_path.h"
#include <float.h>

namespace sgm {

// ------------------------------------------------------------------------------------------
// One workgroup per image row.  The right-view disparity map of upstream ("disp2", filled in
// descending x, a candidate replaces the holder only with a strictly smaller cost) is the
// argmin over candidates of (cost, then larger x): an LDS atomicMin on (cost << 16 | 0xffff-x).
__global__ __launch_bounds__(256) void k_select(Geom g, const uint2 *__restrict__ wta,
                                                int16_t *__restrict__ disp)
{
    extern __shared__ uint32_t keys[];  // W entries
    const int y = blockIdx.x, W = g.W, maxX1 = g.minX1 + g.W1;
    const int INV = g.invalid_scaled;
    for (int x = threadIdx.x; x < W; x += blockDim.x) keys[x] = 0xffffffffu;
    __syncthreads();
    for (int x = g.minX1 + threadIdx.x; x < maxX1; x += blockDim.x) {
        const uint32_t k = wta[(int64_t)y * W + x].x;
        if (k != 0xffffffffu) {
            const int best = (int)(k & 0xffffu);
            const int x2 = x - best - g.minD;
            atomicMin(&keys[x2], (k & 0xffff0000u) | (uint32_t)(0xffff - x));
        }
    }
    __syncthreads();
    for (int x = threadIdx.x; x < W; x += blockDim.x) {
        int d1 = INV;
        if (x >= g.minX1 && x < maxX1) {
            const uint2 kv = wta[(int64_t)y * W + x];
            if (kv.x != 0xffffffffu) {
                const int best = (int)(kv.x & 0xffffu), s0 = (int)(kv.x >> 16);
                int dsc = best * 16;
                if (best > 0 && best < g.D - 1) {
                    const int sm = (int)(kv.y & 0xffffu), sp = (int)(kv.y >> 16);
                    const int denom2 = max(sm + sp - 2 * s0, 1);
                    dsc += ((sm - sp) * 16 + denom2) / (denom2 * 2);  // C division, toward zero
                }
                d1 = dsc + g.minD * 16;
            }
        }
        if (d1 != INV) {
            const int lo = d1 >> 4, hi = (d1 + 15) >> 4;
            const int xa = x - lo, xb = x - hi;
            bool kill = false;
            if (xa >= 0 && xa < W && xb >= 0 && xb < W) {
                const uint32_t ka = keys[xa], kb = keys[xb];
                const int da = ka == 0xffffffffu ? INV : (0xffff - (int)(ka & 0xffffu)) - xa;
                const int db = kb == 0xffffffffu ? INV : (0xffff - (int)(kb & 0xffffu)) - xb;
                kill = da >= g.minD && abs(da - lo) > g.d12 && db >= g.minD && abs(db - hi) > g.d12;
            }
            if (kill) d1 = INV;
        }
        disp[(int64_t)y * W + x] = (int16_t)d1;
    }
}

// ------------------------------------------------------------------------------------------
// Winner-take-all over the finished S volume, one LANE per pixel ("transposed" WTA).
//
// Inside the path kernels a pixel's D disparities are spread over the 64 lanes, so the argmin and
// the uniqueness test are wave reductions: ~110 instructions per pixel of a latency-bound kernel.
// Read back from HBM the same S vector can be scanned by a single lane with no cross-lane work:
// a block stages 64 consecutive pixels (64 * D * 2 bytes, one coalesced sweep) into LDS with a
// padded row stride, then every lane walks its own pixel twice --
//   pass 1: key = min over d of (S[d] << 16 | d)              -> minS and the FIRST best d
//   pass 2: far = min of S[d] over |d - best| > 1 (packed)    -> uniqueness (A.6 step 2)
// ~20 wave instructions per pixel, no dependent chain between pixels; the kernel is bound by
// reading V once.  Same record format as wta_pixels (kernels_path.h); same arithmetic as the
// selection loop of oracle/sgbm_oracle.c.
constexpr int wta_t_stride(int D) { return D * 2 + 8; }  // bytes per staged pixel row (8-byte aligned, breaks the bank stride)

// S = sat(S + S2), element-wise: only when the aggregated volume is kept for inspection (SGM_OPT_KEEP_AGGR)
// after a frame whose fifth path went into a volume of its own.
__global__ __launch_bounds__(256) void k_add_sat(int16_t *__restrict__ S, const int16_t *__restrict__ S2, int64_t n8)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    uint4 a = reinterpret_cast<uint4 *>(S)[i];
    const uint4 b = reinterpret_cast<const uint4 *>(S2)[i];
    a.x = pk_adds_s(a.x, b.x);
    a.y = pk_adds_s(a.y, b.y);
    a.z = pk_adds_s(a.z, b.z);
    a.w = pk_adds_s(a.w, b.w);
    reinterpret_cast<uint4 *>(S)[i] = a;
}

// LG = log2(chunks per row) when D is a power of two (16..512): compile-time trip counts, the next
// block's loads prefetched into registers during the current block's scan.  LG = -1: any D
// (multiple of 16), plain staging.
// NV: the costs are the saturating sum of NV volumes.  2: S + S2 (MODE_SGBM with D <= 128: the fifth path runs
// beside the sweep into a volume of its own); 3: S + S2 + S3 (D <= 64: both in-row paths run beside the per-row
// pre-pass and the element-wise vertical kernel, each into a volume of its own); 5: the five directions of MODE_SGBM each
// in a volume of its own (D <= 64: k_lines3_g + the two in-row paths); 4: the four axis-aligned directions of MODE_HH4
// (D <= 64: k_axis_paths4_g).  Every path cost is >= 0 and the
// sum saturates, so the order of the additions does not matter -- kernels_path.h.
template <bool POSW, int LG, int NV = 1>
__global__ __launch_bounds__(64) void k_wta_t(Geom g, const int16_t *__restrict__ S, uint2 *__restrict__ wta, int64_t npix,
                                              const int16_t *__restrict__ S2 = nullptr, const int16_t *__restrict__ S3 = nullptr,
                                              const int16_t *__restrict__ S4 = nullptr, const int16_t *__restrict__ S5 = nullptr)
{
    constexpr bool CONF = false;
    [[maybe_unused]] uint8_t *const conf = nullptr;
#include "kernels_wta_body.h"
}

// CONF (SGM_OPT_CONFIDENCE): the lane also stores the pixel's uniqueness margin as a byte --
//   conf_raw = 100 if far == 0, else (far - minS) * 100 / far      (C division; 0 .. 100)
// with far the smallest S outside best-1 .. best+1, the quantity the positive-weight form already has.  For integer
// u in 0 .. 100 upstream's test keeps a pixel iff far * (100 - u) >= minS * 100 iff conf_raw >= u, so the byte is the
// largest uniquenessRatio under which the pixel survives.  It does not depend on uniquenessRatio; the CONF form takes the
// engine's ratio at run time (far for a positive weight, the per-d products otherwise), one instantiation for both.
// conf is the uint8 [H][W] map conf_raw (columns outside minX1 .. minX1 + W1 are not written: the engine clears the map first).
// The body is the text of k_wta_t's (kernels_wta_body.h), so that k_wta_t itself compiles to what it was without the option.
template <int LG, int NV = 1>
__global__ __launch_bounds__(64) void k_wta_conf_t(Geom g, const int16_t *__restrict__ S, uint2 *__restrict__ wta, int64_t npix,
                                                   const int16_t *__restrict__ S2, const int16_t *__restrict__ S3,
                                                   const int16_t *__restrict__ S4, const int16_t *__restrict__ S5,
                                                   uint8_t *__restrict__ conf)
{
    constexpr bool CONF = true, POSW = false;
#include "kernels_wta_body.h"
}

// ------------------------------------------------------------------------------------------
// The deciding half of the split winner-take-all (kernels_path.h: wta_reduce_pixels did the lane reductions inside the chained
// second sweep).  One thread per matched pixel: raw = {minS << 16 | nq << 6 | ln, w0, w1, pv >> 16 | nx << 16}, the words of the
// first lane that holds a minimum and the facing halves of its neighbours' (layout: kernels_path.h).  wta_select_words finds
// the best d and its clamped neighbours among them and takes the uniqueness decision.  Writes k_wta_t's record.
__global__ __launch_bounds__(256) void k_wta_select(Geom g, const uint4 *__restrict__ raw, uint2 *__restrict__ wta, UniqRecip q)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= g.W1) return;
    const int64_t i = (int64_t)y * g.W + g.minX1 + x;
    const uint4 r = raw[i];
    uint2 o;
    wta_select_words(g.D / 128, q, r.x, r.y, r.z, r.w, o.x, o.y);
    wta[i] = o;
}

// conf = conf_raw where the final disparity (after LR check, median and speckle filter) is valid, 0 where it is the
// invalid value; VEC: four pixels per thread (4-byte aligned maps, 8-byte aligned disparities), the tail pixel by pixel
template <bool VEC>
__global__ __launch_bounds__(256) void k_conf_final(const uint8_t *__restrict__ conf_raw, const int16_t *__restrict__ disp,
                                                    int invalid, uint8_t *__restrict__ out, int64_t n)
{
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * (VEC ? 4 : 1);
    if (VEC && i + 4 <= n) {
        const uint32_t c = *reinterpret_cast<const uint32_t *>(conf_raw + i);
        const uint2 d = *reinterpret_cast<const uint2 *>(disp + i);
        const int d0 = (int16_t)(d.x & 0xffffu), d1 = (int16_t)(d.x >> 16), d2 = (int16_t)(d.y & 0xffffu), d3 = (int16_t)(d.y >> 16);
        const uint32_t m = (d0 != invalid ? 0xffu : 0u) | (d1 != invalid ? 0xff00u : 0u) | (d2 != invalid ? 0xff0000u : 0u) |
                           (d3 != invalid ? 0xff000000u : 0u);
        *reinterpret_cast<uint32_t *>(out + i) = c & m;
        return;
    }
    for (int64_t j = i; j < n && j < i + (VEC ? 4 : 1); j++) out[j] = (int)disp[j] != invalid ? conf_raw[j] : (uint8_t)0;
}

__device__ __forceinline__ void cswap(int &a, int &b)
{
    const int lo = min(a, b), hi = max(a, b);
    a = lo;
    b = hi;
}

// dst2 (nullable): a second copy of the result -- the engine's output buffer, on which the speckle
// filter then works in place, while dst stays readable as the "after median" tap
__global__ __launch_bounds__(256) void k_median3(const int16_t *__restrict__ src,
                                                 int16_t *__restrict__ dst, int16_t *__restrict__ dst2, int H, int W)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const int16_t *r0 = src + (int64_t)max(y - 1, 0) * W;
    const int16_t *r1 = src + (int64_t)y * W;
    const int16_t *r2 = src + (int64_t)min(y + 1, H - 1) * W;
    const int xl = max(x - 1, 0), xr = min(x + 1, W - 1);
    int p0 = r0[xl], p1 = r0[x], p2 = r0[xr], p3 = r1[xl], p4 = r1[x], p5 = r1[xr], p6 = r2[xl], p7 = r2[x], p8 = r2[xr];
    // 19-exchange median-of-9 network
    cswap(p1, p2); cswap(p4, p5); cswap(p7, p8); cswap(p0, p1); cswap(p3, p4); cswap(p6, p7);
    cswap(p1, p2); cswap(p4, p5); cswap(p7, p8); cswap(p0, p3); cswap(p5, p8); cswap(p4, p7);
    cswap(p3, p6); cswap(p1, p4); cswap(p2, p5); cswap(p4, p7); cswap(p4, p2); cswap(p6, p4);
    cswap(p4, p2);
    dst[(int64_t)y * W + x] = (int16_t)p4;
    if (dst2) dst2[(int64_t)y * W + x] = (int16_t)p4;
}

// ------------------------------------------------------------------------------------------
// Speckle filter (A.8) as connected components over horizontal RUNS: a run is a maximal stretch
// of one row whose neighbouring pixels are linked (both != newVal, |a-b| <= maxDiff).  Every
// pixel of a run points at the run's first pixel; first pixels form a lock-free union-find
// forest (links only ever decrease, atomicMin) joined where runs of adjacent rows touch.  The
// component partition, hence the output, does not depend on the traversal order upstream uses.
//
//   label[i] : -1 invalid | i's run start (non-start pixels, immutable) | parent link (starts)
//   rlen[s]  : length of the run starting at s          csz[r] : pixels of the component rooted at r
__device__ __forceinline__ int uf_load(const int *L, int a)
{
    // agent scope: a CU's L1 is never refreshed by other CUs' atomics
    return __hip_atomic_load(L + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int uf_find(int *L, int a)
{
    int p = uf_load(L, a);
    while (p != a) {
        const int gp = uf_load(L, p);
        if (gp != p) atomicMin(&L[a], gp);  // path halving; any ancestor is a valid parent
        a = p;
        p = gp;
    }
    return a;
}
__device__ __forceinline__ void uf_union(int *L, int a, int b)
{
    bool done;
    do {
        a = uf_find(L, a);
        b = uf_find(L, b);
        if (a < b) {
            const int old = atomicMin(&L[b], a);
            done = (old == b);
            b = old;
        } else if (b < a) {
            const int old = atomicMin(&L[a], b);
            done = (old == a);
            a = old;
        } else {
            done = true;
        }
    } while (!done);
}

__device__ __forceinline__ bool linked(int a, int b, int newVal, int maxDiff)
{
    return a != newVal && b != newVal && abs(a - b) <= maxDiff;
}

// one wave per row: run starts by an inclusive prefix-max of "x where a run begins"
__global__ __launch_bounds__(64) void k_ccl_rows(const int16_t *__restrict__ img, int *__restrict__ label,
                                                 int *__restrict__ rlen, int *__restrict__ csz, int W,
                                                 int newVal, int maxDiff)
{
    const int y = blockIdx.x, lane = threadIdx.x;
    const int16_t *row = img + (int64_t)y * W;
    const int64_t base = (int64_t)y * W;
    int carry = -1;  // start of the run the previous chunk ended in
    for (int x0 = 0; x0 < W; x0 += 64) {
        const int x = x0 + lane;
        const bool in = x < W;
        const int v = in ? row[x] : newVal;
        const int vl = (in && x > 0) ? row[x - 1] : newVal;
        const int vr = (in && x < W - 1) ? row[x + 1] : newVal;
        const bool valid = v != newVal;
        const bool starts = valid && !linked(v, vl, newVal, maxDiff);
        int s = starts ? x : -1;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(s, o);
            if (lane >= o) s = max(s, t);
        }
        s = max(s, carry);
        if (in) {
            label[base + x] = valid ? (int)(base + s) : -1;
            csz[base + x] = 0;
            if (valid && !linked(v, vr, newVal, maxDiff)) rlen[base + s] = x - s + 1;  // run ends here
        }
        carry = __shfl(s, 63);
    }
}

// join runs of adjacent rows; one union per maximal stretch of vertical links between two runs
__global__ __launch_bounds__(256) void k_ccl_merge(const int16_t *__restrict__ img, int *label, int H, int W,
                                                   int newVal, int maxDiff)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= W || y == 0) return;
    const int64_t i = (int64_t)y * W + x;
    const int v = img[i], u = img[i - W];
    if (!linked(v, u, newVal, maxDiff)) return;
    bool need = x == 0;
    if (!need) {
        const int vl = img[i - 1], ul = img[i - W - 1];
        // the stretch starts here if the left column is not linked the same way
        need = !linked(v, vl, newVal, maxDiff) || !linked(u, ul, newVal, maxDiff) || !linked(vl, ul, newVal, maxDiff);
    }
    if (!need) return;
    const bool vs = x == 0 || !linked(v, img[i - 1], newVal, maxDiff);
    const bool us = x == 0 || !linked(u, img[i - W - 1], newVal, maxDiff);
    const int a = vs ? (int)i : label[i];          // run starts (non-start labels are immutable)
    const int b = us ? (int)(i - W) : label[i - W];
    uf_union(label, a, b);
}

// per run: add its length to its component's root and point the run start at the root
__global__ __launch_bounds__(256) void k_ccl_count(const int16_t *__restrict__ img, int *label,
                                                   const int *__restrict__ rlen, int *__restrict__ csz, int H, int W,
                                                   int newVal, int maxDiff)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const int64_t i = (int64_t)y * W + x;
    const int v = img[i];
    if (v == newVal) return;
    if (x > 0 && linked(v, img[i - 1], newVal, maxDiff)) return;  // not a run start
    const int r = uf_find(label, (int)i);
    atomicAdd(&csz[r], rlen[i]);
    if (r != (int)i) atomicMin(&label[i], r);  // run start -> root directly (all unions are done): k_ccl_apply needs one hop
}

__global__ __launch_bounds__(256) void k_ccl_apply(int16_t *__restrict__ img, int *label,
                                                   const int *__restrict__ csz, int H, int W, int newVal,
                                                   int maxDiff, int maxSpeckleSize)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const int64_t i = (int64_t)y * W + x;
    const int l = label[i];
    if (l < 0) return;
    const int r = label[l];  // l is i itself or i's run start, which k_ccl_count pointed at the root
    if (csz[r] <= maxSpeckleSize) img[i] = (int16_t)newVal;
}

// ------------------------------------------------------------------------------------------
// main.ipynb:668-670 : f = i16 / 16 ; f * float(f > 0)   (invalid -> -0.0, zero -> +0.0)
__global__ __launch_bounds__(256) void k_disp_to_float(const int16_t *__restrict__ d, float *__restrict__ out,
                                                       int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float f = (float)d[i] / 16.0f;
    out[i] = f * (f > 0.0f ? 1.0f : 0.0f);
}

// order-preserving float <-> uint key for atomicMin
__device__ __forceinline__ uint32_t fkey(float f)
{
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float fkey_inv(uint32_t k)
{
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__global__ __launch_bounds__(256) void k_min_f32(const float *__restrict__ d, int64_t n, uint32_t *minkey)
{
    uint32_t k = 0xffffffffu;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        k = min(k, fkey(d[i]));
    k = wave_min_u32(k);
    if ((threadIdx.x & 63) == 0) atomicMin(minkey, k);
}

struct QMat {
    double q[16];
};

// Appendix B: homogeneous point in double, sums in index order from 0, one rounding to float,
// divide as multiply by the reciprocal, one more rounding.  The library is built with
// -ffp-contract=off so that no fused multiply-add changes the double arithmetic.
__device__ __forceinline__ void reproject_px(float fd, int x, int y, int64_t i, const QMat &Q, const uint32_t *minkey,
                                             float *__restrict__ xyz)
{
    const double d = (double)fd;
    const double v[4] = {(double)x, (double)y, d, 1.0};
    double h[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 4; k++) s += Q.q[r * 4 + k] * v[k];
        h[r] = s;
    }
    const double ia = 1.0 / h[3];
    float o[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const float f = (float)h[r];
        o[r] = (float)((double)f * ia);
    }
    if (minkey) {
        const double mn = (double)fkey_inv(*minkey);
        if (fabs(d - mn) <= (double)FLT_EPSILON) o[2] = 10000.f;
    }
    xyz[i * 3 + 0] = o[0];
    xyz[i * 3 + 1] = o[1];
    xyz[i * 3 + 2] = o[2];
}

__global__ __launch_bounds__(256) void k_reproject(const float *__restrict__ disp, int H, int W, QMat Q,
                                                   const uint32_t *minkey, float *__restrict__ xyz)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const int64_t i = (int64_t)y * W + x;
    reproject_px(disp[i], x, y, i, Q, minkey, xyz);
}

// The driver cell in one launch (main.ipynb:668-670 then :697): int16 disparity -> float disparity
// (stored if dispf is non-null) -> XYZ.  Same arithmetic as k_disp_to_float followed by k_reproject.
__global__ __launch_bounds__(256) void k_float_xyz(const int16_t *__restrict__ d16, int H, int W, QMat Q,
                                                   float *__restrict__ dispf, float *__restrict__ xyz)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const int64_t i = (int64_t)y * W + x;
    const float f0 = (float)d16[i] / 16.0f;
    const float f = f0 * (f0 > 0.0f ? 1.0f : 0.0f);
    if (dispf) dispf[i] = f;
    reproject_px(f, x, y, i, Q, nullptr, xyz);
}

// main.ipynb:726-730
__global__ __launch_bounds__(256) void k_valid_mask(const float *__restrict__ xyz, const float *__restrict__ disp,
                                                    int64_t n, uint8_t *__restrict__ mask)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float X = xyz[i * 3];
    mask[i] = (uint8_t)(!isnan(X) && !isinf(X) && disp[i] > 0.0f);
}

// ------------------------------------------------------------------------------------------
// Valid-point compaction + colour gather (/root/reference/main.ipynb:726-737):
//   mask = ~isnan(X) & ~isinf(X) & (disp > 0);  valid_points = points_3D[mask];  valid_colors = colors[mask]
// numpy boolean indexing keeps row-major order, so the compaction is an ordered one:
// per-256-pixel block counts -> exclusive scan -> ordered scatter (ballot + popcount inside a wave).
__device__ __forceinline__ bool point_valid(const float *xyz, const float *disp, int64_t i)
{
    const float X = xyz[i * 3];
    return !isnan(X) && !isinf(X) && disp[i] > 0.0f;
}

__global__ __launch_bounds__(256) void k_compact_count(const float *__restrict__ xyz, const float *__restrict__ disp,
                                                       int64_t n, uint32_t *__restrict__ counts)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool v = i < n && point_valid(xyz, disp, i);
    const unsigned long long b = __builtin_amdgcn_ballot_w64(v);
    __shared__ uint32_t wsum[4];
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = (uint32_t)__builtin_popcountll(b);
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// exclusive scan of `m` block counts by one workgroup (m is a few 10^4 at most); total -> counts[m]
__global__ __launch_bounds__(1024) void k_compact_scan(uint32_t *counts, int m)
{
    __shared__ uint32_t part[1024];
    const int t = threadIdx.x;
    const int per = (m + 1023) / 1024;
    const int lo = min(t * per, m), hi = min(lo + per, m);
    uint32_t s = 0;
    for (int i = lo; i < hi; i++) s += counts[i];
    part[t] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {  // inclusive Hillis-Steele scan of the partials
        const uint32_t v = t >= o ? part[t - o] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint32_t run = t ? part[t - 1] : 0u;
    for (int i = lo; i < hi; i++) {
        const uint32_t c = counts[i];
        counts[i] = run;
        run += c;
    }
    if (t == 1023) counts[m] = part[1023];
}

__global__ __launch_bounds__(256) void k_compact_scatter(const float *__restrict__ xyz, const float *__restrict__ disp,
                                                         const uint8_t *__restrict__ colors, int64_t n,
                                                         const uint32_t *__restrict__ offsets,
                                                         float *__restrict__ out_xyz, uint8_t *__restrict__ out_rgb)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool v = i < n && point_valid(xyz, disp, i);
    const unsigned long long b = __builtin_amdgcn_ballot_w64(v);
    __shared__ uint32_t wsum[4];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) wsum[w] = (uint32_t)__builtin_popcountll(b);
    __syncthreads();
    uint32_t base = offsets[blockIdx.x];
    for (int k = 0; k < w; k++) base += wsum[k];
    if (v) {
        const uint32_t o = base + (uint32_t)__builtin_popcountll(b & ((1ull << lane) - 1ull));
        out_xyz[(int64_t)o * 3 + 0] = xyz[i * 3 + 0];
        out_xyz[(int64_t)o * 3 + 1] = xyz[i * 3 + 1];
        out_xyz[(int64_t)o * 3 + 2] = xyz[i * 3 + 2];
        if (colors) {
            out_rgb[(int64_t)o * 3 + 0] = colors[i * 3 + 0];
            out_rgb[(int64_t)o * 3 + 1] = colors[i * 3 + 1];
            out_rgb[(int64_t)o * 3 + 2] = colors[i * 3 + 2];
        }
    }
}

// the total of a compaction (counts[m] after k_compact_scan) as the int64 the caller's device memory holds
__global__ void k_compact_total(const uint32_t *__restrict__ total, int64_t *__restrict__ out) { *out = (int64_t)*total; }

}  // namespace sgm
