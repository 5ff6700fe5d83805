// kernels_census.h -- the census matching cost (SGM_OPT_COST = SGM_COST_CENSUS; include/sgm_hip.h has the definition).
//
//   k_census         : u8 image -> one 64-bit descriptor per pixel: bit k is 1 iff the k-th of the 62 neighbours
//                      (dy in -3..3, dx in -4..4, centre left out, coordinates clamped to the image) is darker than the pixel.
//                      Left image: [H][W]; right image: [H][W] stored MIRRORED in x, as the right planes of k_features are, so
//                      that ascending disparity is ascending address.
//   k_pix_census     : pix(y, xi, k) = popcount(cL(y, xi + minX1) ^ cR(y, xi + minX1 - minD - k)) as bytes [H][W1][D], where
//                      k_pix puts its bytes: the box stages behind it are BT's k_box_u8, or k_hsum_u8 + BT's k_vsum*.
//                      One wave per (row, chunk of CENSUS_XL columns); lanes span the disparities, 2 * NP per lane.
//   k_pix_census_px  : the same for D <= 32, one THREAD per pixel (as k_pix_px: lanes spanning D = 16 would idle 7 of 8).
//   k_hsum_u8        : the bytes -> int16 horizontal box sums [H][W1][D], the input of k_vsum_ring / k_vsum, for the
//                      configurations k_box_u8 does not cover; one thread per 8 adjacent disparities of a pixel.
#pragma once
#include "kernels_cost.h"

namespace sgm {

constexpr int CENSUS_XL = 128;  // columns per chunk of k_pix_census (the engine's COST_XL)

// blockIdx.z = 0: left image -> desc_l; 1: right image -> desc_r (one launch for the pair).  A block takes 256 columns of one
// row and stages the 7 rows x (256 + 8) bytes it compares in LDS; rows and columns are clamped while staging, so images
// shorter than the window (H < 7, W < 9) and a last, partial block need nothing special.
__global__ __launch_bounds__(256) void k_census(const uint8_t *__restrict__ imgL, const uint8_t *__restrict__ imgR, int64_t stride,
                                                int H, int W, uint64_t *__restrict__ desc_l, uint64_t *__restrict__ desc_r)
{
    constexpr int RY = 3, RX = 4, TW = 256 + 2 * RX;
    __shared__ uint8_t tile[2 * RY + 1][TW];
    const int t = threadIdx.x, x0 = blockIdx.x * 256, y = blockIdx.y;
    const bool is_right = blockIdx.z != 0;
    const uint8_t *img = is_right ? imgR : imgL;
    for (int k = t; k < (2 * RY + 1) * TW; k += 256) {
        const int r = k / TW, c = k - r * TW;
        const int yy = min(max(y + r - RY, 0), H - 1), xx = min(max(x0 + c - RX, 0), W - 1);
        tile[r][c] = img[(int64_t)yy * stride + xx];
    }
    __syncthreads();
    const int x = x0 + t;
    if (x >= W) return;
    const uint32_t ctr = tile[RY][t + RX];
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int dy = 0; dy <= 2 * RY; dy++)
#pragma unroll
        for (int dx = 0; dx <= 2 * RX; dx++) {
            const int idx = dy * (2 * RX + 1) + dx, mid = RY * (2 * RX + 1) + RX;
            if (idx == mid) continue;
            const int k = idx < mid ? idx : idx - 1;  // 0 .. 61
            const uint32_t bit = tile[dy][t + dx] < ctr ? 1u : 0u;
            if (k < 32) lo |= bit << k;
            else hi |= bit << (k - 32);
        }
    const uint64_t d = ((uint64_t)hi << 32) | lo;
    if (!is_right) desc_l[(int64_t)y * W + x] = d;
    else desc_r[(int64_t)y * W + (W - 1 - x)] = d;
}

// One wave per (row, chunk of CENSUS_XL columns).  Lane l owns the disparity indices K * l .. K * l + K - 1 (K = 2 * NP) and
// keeps their K right descriptors in registers.  From one column to the next every disparity's right pixel moves one to the
// left: the lane drops its highest descriptor, and the one it gains is the one its lower neighbour lane drops (a DPP wave
// shift of both halves); lane 0 gains the next descriptor of the row, the same for the whole wave (staged in LDS with the
// chunk's left descriptors and read at a wave-uniform address: a broadcast, no bank conflict).  The K registers are a
// ring: the column loop is unrolled by K, so the slot that is replaced and the slot of every output byte are static.
// Per (x, d): two v_xor, two v_bcnt (the second accumulates on the first), and the byte pack.
template <int NP>
__global__ __launch_bounds__(64) void k_pix_census(Geom g, const uint64_t *__restrict__ desc_l, const uint64_t *__restrict__ desc_r,
                                                   uint8_t *__restrict__ pix, int nchunks)
{
    constexpr int K = 2 * NP, XL = CENSUS_XL;
    __shared__ uint64_t sl[XL], sr[XL];  // column j0 + k: its left descriptor; the right descriptor of its disparity index 0
    const int lane = threadIdx.x;
    const int unit = blockIdx.x;
    const int y = __builtin_amdgcn_readfirstlane(unit / nchunks), ck = unit - y * nchunks;  // (uniform: see uniform_rsrc)
    const int W1 = g.W1, W = g.W;
    const int j0 = ck * XL, j1 = min(j0 + XL, W1) - 1, n = j1 - j0 + 1;
    const bool active = K * lane < g.D;
    const uint64_t *lrow = desc_l + (int64_t)y * W + (j0 + g.minX1);
    const uint64_t *rrow = desc_r + (int64_t)y * W;
    // mirrored position of (column j, disparity index e): (W-1-(j+minX1)) + minD + e; base0: column j0, index 0
    const int base0 = W - 1 - (j0 + g.minX1) + g.minD;
    for (int k = lane; k < n; k += 64) {
        const int pos = base0 - k;
        sl[k] = lrow[k];
        sr[k] = pos >= 0 && pos < W ? rrow[pos] : (uint64_t)0;
    }
    // the ring at column j0: slot i holds disparity index K * lane + i (lanes past D: whatever is in range, never stored)
    uint32_t rlo[K], rhi[K];
#pragma unroll
    for (int i = 0; i < K; i++) {
        const int pos = base0 + K * lane + i;
        const uint64_t v = pos >= 0 && pos < W ? rrow[pos] : (uint64_t)0;
        rlo[i] = (uint32_t)v;
        rhi[i] = (uint32_t)(v >> 32);
    }
    __syncthreads();  // single wave; orders the LDS staging before the reads below
    // this row of the output; lanes past D store nowhere (offset beyond the descriptor)
    const int row_bytes = W1 * g.D;
    const __amdgpu_buffer_rsrc_t orow = uniform_rsrc(pix, (int64_t)y * row_bytes, row_bytes);
    const int voff = active ? K * lane : row_bytes;
    // the K bytes of column j; ph: slot s holds disparity index K * lane + ((s + ph) & (K - 1))
    auto emit = [&](int j, int ph) __attribute__((always_inline)) {
        const uint64_t l = sl[j - j0];
        const uint32_t llo = (uint32_t)l, lhi = (uint32_t)(l >> 32);
        uint32_t q[(K + 3) / 4];
#pragma unroll
        for (int w = 0; w < (K + 3) / 4; w++) q[w] = 0;
#pragma unroll
        for (int o = 0; o < K; o++) {
            const int s = (o - ph) & (K - 1);
            const uint32_t c = (uint32_t)__builtin_popcount(rlo[s] ^ llo) + (uint32_t)__builtin_popcount(rhi[s] ^ lhi);
            q[o / 4] |= c << (8 * (o & 3));
        }
        const int so = j * g.D;
        if constexpr (NP == 1) {
            __builtin_amdgcn_raw_buffer_store_b16((unsigned short)q[0], orow, voff, so, 0);
        } else if constexpr (NP == 2) {
            __builtin_amdgcn_raw_buffer_store_b32(q[0], orow, voff, so, 0);
        } else {
#pragma unroll
            for (int w = 0; w < K / 4; w += 2) {  // 64-bit MUBUF stores only, kept apart (sgm_device.h: buf_store says why)
                v2u32 o2;
                o2.x = q[w];
                o2.y = q[w + 1];
                __builtin_amdgcn_raw_buffer_store_b64(o2, orow, voff + 4 * w, so, 0);
                if (w + 2 < K / 4) asm volatile("" ::: "memory");
            }
        }
    };
    // column j, the t-th after an aligned one (t = 1 .. K): slot K - t is the one that held the highest index
    auto step = [&](int j, int t) __attribute__((always_inline)) {
        const uint64_t nr = sr[j - j0];
        const int s = (K - t) & (K - 1);
        rlo[s] = from_lower_lane(rlo[s], (uint32_t)nr);
        rhi[s] = from_lower_lane(rhi[s], (uint32_t)(nr >> 32));
        emit(j, t & (K - 1));
    };
    emit(j0, 0);
    int j = j0 + 1;
    for (; j + K - 1 <= j1; j += K) {
#pragma unroll
        for (int u = 0; u < K; u++) step(j + u, u + 1);
    }
#pragma unroll
    for (int u = 0; u < K; u++)
        if (j + u <= j1) step(j + u, u + 1);
}

// D <= 32: one thread per pixel, the right descriptors of a 256-pixel block (256 + D - 1 of them) staged in LDS; adjacent
// threads read adjacent descriptors (8-byte stride: no bank conflict).
__global__ __launch_bounds__(256) void k_pix_census_px(Geom g, const uint64_t *__restrict__ desc_l, const uint64_t *__restrict__ desc_r,
                                                       uint8_t *__restrict__ pix)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];  // uint64 [255 + D]
    uint64_t *seg = reinterpret_cast<uint64_t *>(smem);
    const int t = threadIdx.x, y = blockIdx.y, b0 = blockIdx.x * 256;
    const int W = g.W, W1 = g.W1, D = g.D;
    // the block's smallest mirrored position belongs to xi = b0 + 255, index 0
    const int pmin = W - 1 - (b0 + 255 + g.minX1) + g.minD;
    const uint64_t *rrow = desc_r + (int64_t)y * W;
    for (int s = t; s < 255 + D; s += 256) {
        const int pos = pmin + s;
        seg[s] = pos >= 0 && pos < W ? rrow[pos] : (uint64_t)0;
    }
    __syncthreads();
    const int xi = b0 + t;
    if (xi >= W1) return;
    const uint64_t l = desc_l[(int64_t)y * W + xi + g.minX1];
    const uint64_t *sp = seg + (255 - t);
    uint32_t *out = reinterpret_cast<uint32_t *>(pix + ((int64_t)y * W1 + xi) * D);
    for (int e0 = 0; e0 < D; e0 += 4) {
        uint32_t packed = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) packed |= (uint32_t)__builtin_popcountll(l ^ sp[e0 + q]) << (8 * q);
        out[e0 / 4] = packed;
    }
}

// hs(y, xi, .) = sum over t in -SW2..SW2 of pix(y, clamp(xi + t, 0, W1 - 1), .)  (A.4), any D (a multiple of 16) and any
// radius.  Adjacent threads take adjacent 8-byte groups of a pixel's disparities and then the next pixel's, so loads and
// stores are contiguous across a wave; the 2 * SW2 + 1 reads of a byte come from the cache.
__global__ __launch_bounds__(256) void k_hsum_u8(Geom g, const uint8_t *__restrict__ pix, int16_t *__restrict__ hsum)
{
    const int W1 = g.W1, D = g.D, R = g.SW2, D8 = D >> 3;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;  // 8-disparity group of the row
    if (i >= (int64_t)W1 * D8) return;
    const int xi = (int)(i / D8), e0 = ((int)(i - (int64_t)xi * D8)) * 8;
    const uint8_t *row = pix + (int64_t)blockIdx.y * W1 * D + e0;
    uint32_t acc[4] = {0, 0, 0, 0};
    for (int t = -R; t <= R; t++) {
        const int xc = min(max(xi + t, 0), W1 - 1);
        const uint2 v = *reinterpret_cast<const uint2 *>(row + (int64_t)xc * D);
        acc[0] = pk_add(acc[0], __builtin_amdgcn_perm(0u, v.x, 0x0c010c00u));
        acc[1] = pk_add(acc[1], __builtin_amdgcn_perm(0u, v.x, 0x0c030c02u));
        acc[2] = pk_add(acc[2], __builtin_amdgcn_perm(0u, v.y, 0x0c010c00u));
        acc[3] = pk_add(acc[3], __builtin_amdgcn_perm(0u, v.y, 0x0c030c02u));
    }
    *reinterpret_cast<uint4 *>(hsum + ((int64_t)blockIdx.y * W1 + xi) * D + e0) = make_uint4(acc[0], acc[1], acc[2], acc[3]);
}

}  // namespace sgm
