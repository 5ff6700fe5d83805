// kernels_right.h -- the right-view disparity map (SGM_OPT_RIGHT_VIEW) from the aggregated volume the left view leaves in
// device memory: a winner-take-all over the DIAGONALS of S, then sub-pixel step and right-to-left check per row.
//
// Right pixel xr1 (a matched column of the right map, xr = minX1 - minD + xr1) has, at candidate k, the cost
//   SR(k) = S[y][xr1 + k][k],   k in [0, n),   n = min(D, W1 - xr1)
// -- the cost left pixel xr1 + k paid for disparity k.  Consecutive k of one right pixel lie (D + 1) * 2 bytes apart, so a
// lane cannot walk its own pixel through global memory the way k_wta_t's lanes walk theirs through a staged row.
// No counterpart upstream: OpenCV's disp2 (k_select, kernels_post.h) is the integer argmin over the left WINNERS only.
// CPU restatement: tests/right_view_ref.py.
#pragma once
#include "kernels_post.h"

namespace sgm {

constexpr int RV_T = 256;    // right pixels per workgroup = threads (four waves)
constexpr int RV_CH = 32;    // disparities staged per step: 64-byte segments of T + CH - 1 left columns
constexpr int RV_STRIDE = RV_CH * 2 + 4;   // bytes per staged column: 17 dwords, odd -- the diagonal read is conflict-free
constexpr int RV_COLS = RV_T + RV_CH - 1;  // left columns a step needs: lane t reads column t + j at disparity j
constexpr int RV_Q = RV_CH / 8;            // 16-byte pieces per staged column

struct RightVols {
    const int16_t *S[5];   // the volumes whose saturating sum is the aggregated cost (Plan::nvol), S[0] always
    int nv;
};

// median of three for a <= b: one v_med3_u32 (the form the backend matches)
__device__ __forceinline__ uint32_t rv_med3(uint32_t a, uint32_t b, uint32_t x) { return min(max(a, b), max(min(a, b), x)); }

// saturating int16 sum of the volumes at one element, in the order k_wta_t adds them
__device__ __forceinline__ int rv_cost_at(const RightVols &v, int64_t i)
{
    int s = v.S[0][i];
    for (int q = 1; q < v.nv; q++) s = max(min(s + (int)v.S[q][i], 32767), -32768);
    return s;
}

// One workgroup: RV_T consecutive right pixels of one row, lane = right pixel.  k is walked in steps of RV_CH: a step
// stages the RV_CH disparities [k0, k0 + RV_CH) of the left columns x0 + k0 .. x0 + k0 + RV_COLS - 1 (those inside the
// row: a diagonal never reaches the next row) into LDS, 64 contiguous bytes per column -- read amplification
// (T + CH - 1) / T = 1.12 -- and every lane takes its RV_CH candidates from the staged diagonal.  The running state is the
// FOUR smallest (cost << 16 | k) keys, sorted: the first is (minS, first best k); the smallest cost outside best - 1 ..
// best + 1 is the first of the other three whose k lies outside (at most two can lie inside), which decides upstream's
// ratio test for a positive weight 100 - u in the same pass.  A non-positive weight (uniquenessRatio >= 100) needs the
// per-candidate products: a second walk over the same steps, taken by that case alone.
// Record: rrec[y * W1 + xr1] = {key or 0xffffffff if rejected, SR(best - 1) | SR(best + 1) << 16} -- k_wta_t's format;
// the neighbours are two gathered loads per volume (only for 0 < best < n - 1, the only case k_right_check uses them in).
__global__ __launch_bounds__(RV_T) void k_right_wta(Geom g, RightVols vols, uint2 *__restrict__ rrec)
{
    __shared__ __attribute__((aligned(16))) uint8_t cols[RV_COLS * RV_STRIDE + 12];
    const int t = threadIdx.x, y = blockIdx.y, x0 = blockIdx.x * RV_T, D = g.D, W1 = g.W1;
    const int xr1 = x0 + t;
    const int n = min(D, W1 - xr1);                 // <= 0 in the lanes past the row's end
    const int nmax = min(D, W1 - x0);               // lane 0's: the longest diagonal of the tile
    const int64_t row0 = (int64_t)y * W1;

    auto stage = [&](int k0) {
        // pieces of 16 bytes: column c = q / RV_Q of the step, piece q % RV_Q of its RV_CH disparities
        const int nq = min(RV_Q, (D - k0) >> 3);    // D is a multiple of 16: the last step may hold 16 disparities
        const int ncol = min(RV_COLS, W1 - (x0 + k0));
        for (int q = t; q < ncol * RV_Q; q += RV_T) {
            const int c = q / RV_Q, w = q % RV_Q;
            if (w < nq) {
                const int64_t at = (row0 + x0 + k0 + c) * D + k0 + w * 8;
                uint4 r = *reinterpret_cast<const uint4 *>(vols.S[0] + at);
                for (int v = 1; v < vols.nv; v++) {
                    const uint4 b = *reinterpret_cast<const uint4 *>(vols.S[v] + at);
                    r.x = pk_adds_s(r.x, b.x);
                    r.y = pk_adds_s(r.y, b.y);
                    r.z = pk_adds_s(r.z, b.z);
                    r.w = pk_adds_s(r.w, b.w);
                }
                uint32_t *dst = reinterpret_cast<uint32_t *>(cols + c * RV_STRIDE + w * 16);
                dst[0] = r.x;
                dst[1] = r.y;
                dst[2] = r.z;
                dst[3] = r.w;
            }
        }
    };
    // lane t's candidate j of the step: column t + j, disparity j
    const uint16_t *mine = reinterpret_cast<const uint16_t *>(cols + t * RV_STRIDE);
    constexpr int JS = RV_STRIDE / 2 + 1;           // uint16 elements from candidate j to j + 1

    uint32_t a0 = 0xffffffffu, a1 = 0xffffffffu, a2 = 0xffffffffu, a3 = 0xffffffffu;   // sorted: a0 <= a1 <= a2 <= a3
    auto insert = [&](uint32_t key) {
        const uint32_t b3 = rv_med3(a2, a3, key), b2 = rv_med3(a1, a2, key), b1 = rv_med3(a0, a1, key);
        a0 = min(a0, key);
        a1 = b1;
        a2 = b2;
        a3 = b3;
    };
    for (int k0 = 0; k0 < nmax; k0 += RV_CH) {
        __syncthreads();                            // the previous step's reads are done
        stage(k0);
        __syncthreads();
        const int rem = n - k0;                     // candidates of this lane from k0 on
        if (__all(rem >= RV_CH)) {                  // (per wave) the whole step is inside every lane's diagonal
#pragma unroll
            for (int j = 0; j < RV_CH; j++) insert(((uint32_t)mine[j * JS] << 16) | (uint32_t)(k0 + j));
        } else {
#pragma unroll
            for (int j = 0; j < RV_CH; j++) {
                const uint32_t key = ((uint32_t)mine[j * JS] << 16) | (uint32_t)(k0 + j);
                insert(j < rem ? key : 0xffffffffu);
            }
        }
    }
    const int minS = (int)(a0 >> 16), best = (int)(a0 & 0xffffu);
    const int wgt = 100 - g.uniq, thr = minS * 100;
    bool reject = false;
    if (wgt > 0) {
        // the first of a1 .. a3 outside best - 1 .. best + 1 (0xffffffff: fewer candidates than that -- no competitor)
        auto outside = [&](uint32_t k) { return k != 0xffffffffu && abs((int)(k & 0xffffu) - best) > 1; };
        const uint32_t far = outside(a1) ? a1 : (outside(a2) ? a2 : (outside(a3) ? a3 : 0xffffffffu));
        reject = far != 0xffffffffu && (int)(far >> 16) * wgt < thr;
    } else {
        for (int k0 = 0; k0 < nmax; k0 += RV_CH) {
            __syncthreads();
            stage(k0);
            __syncthreads();
            const int rem = n - k0;
#pragma unroll 8
            for (int j = 0; j < RV_CH; j++)
                reject |= j < rem && abs(k0 + j - best) > 1 && (int)mine[j * JS] * wgt < thr;
        }
    }
    if (n <= 0) return;
    reject = reject || minS == SGM_MAX_COST;
    uint32_t nb = 0;
    if (!reject && best > 0 && best < n - 1) {
        const int64_t at = (row0 + xr1 + best) * D + best;   // S[y][xr1 + best][best]; its diagonal neighbours are D + 1 away
        nb = (uint32_t)(rv_cost_at(vols, at - D - 1) & 0xffff) | ((uint32_t)(rv_cost_at(vols, at + D + 1) & 0xffff) << 16);
    }
    rrec[row0 + xr1] = make_uint2(reject ? 0xffffffffu : a0, nb);
}

// One workgroup per row: sub-pixel value and right-to-left check, the mirror of k_select's.  dL(x), the left winner's
// integer disparity, comes from the left view's WTA record (before the left LR check): best + minD, or minD - 1 where the
// winner-take-all rejected the pixel or x is no matched left column.  Writes right_raw [H][W], INV outside the matched
// columns of the right map.
__global__ __launch_bounds__(256) void k_right_check(Geom g, const uint2 *__restrict__ wta, const uint2 *__restrict__ rrec,
                                                     int16_t *__restrict__ out)
{
    extern __shared__ int16_t dl[];   // W entries
    const int y = blockIdx.x, W = g.W, W1 = g.W1, maxX1 = g.minX1 + W1, x0 = g.minX1 - g.minD;
    const int INV = g.invalid_scaled;
    for (int x = threadIdx.x; x < W; x += blockDim.x) {
        int d = g.minD - 1;
        if (x >= g.minX1 && x < maxX1) {
            const uint32_t k = wta[(int64_t)y * W + x].x;
            if (k != 0xffffffffu) d = (int)(k & 0xffffu) + g.minD;
        }
        dl[x] = (int16_t)d;
    }
    __syncthreads();
    for (int xr = threadIdx.x; xr < W; xr += blockDim.x) {
        int d1 = INV;
        const int xr1 = xr - x0;
        if (xr1 >= 0 && xr1 < W1) {
            const uint2 kv = rrec[(int64_t)y * W1 + xr1];
            if (kv.x != 0xffffffffu) {
                const int best = (int)(kv.x & 0xffffu), s0 = (int)(kv.x >> 16), n = min(g.D, W1 - xr1);
                int dsc = best * 16;
                if (best > 0 && best < n - 1) {
                    const int sm = (int)(kv.y & 0xffffu), sp = (int)(kv.y >> 16);
                    const int denom2 = max(sm + sp - 2 * s0, 1);
                    dsc += ((sm - sp) * 16 + denom2) / (denom2 * 2);  // C division, toward zero
                }
                d1 = dsc + g.minD * 16;
            }
        }
        if (d1 != INV) {
            const int lo = d1 >> 4, hi = (d1 + 15) >> 4;
            const int xa = xr + lo, xb = xr + hi;
            if (xa >= 0 && xa < W && xb >= 0 && xb < W) {
                const int da = dl[xa], db = dl[xb];
                if (da >= g.minD && abs(da - lo) > g.d12 && db >= g.minD && abs(db - hi) > g.d12) d1 = INV;
            }
        }
        out[(int64_t)y * W + xr] = (int16_t)d1;
    }
}

}  // namespace sgm
