// kernels_color.h -- matching cost of 8-bit 3-channel pairs (SGM_OPT_CHANNELS = 3).
//
// Upstream's calcPixelCostBT with cn = 3 (restated): every channel of the interleaved row gets the A.2
// prefilter from its own neighbours (same channel at x-1 / x+1 of rows y-1, y, y+1) and a raw plane, the border columns
// hold ftzero in all six planes, and the pixel cost is the sum over the six planes -- exactly the sum of the three
// single-channel pixel costs of the channel images (at most 3 * (2 * ftzero + 63) = 567 at preFilterCap 63, and
// 3 * (255 + 63) = 954 once the byte-valued prefilter wraps).  Nothing
// downstream of the pixel cost changes, so the colour path ends in the int16 pipeline's vertical box sum (k_vsum_ring /
// k_vsum), which also writes the headroom record.  C is written once: the three channels are summed in registers.
//
//   k_features_c3 : u8 [H][stride] interleaved rows (3 bytes per pixel) -> per channel (value, lo, hi) of the gradient
//                   and raw planes, the arithmetic of k_features.  Left: [H][W][3] packed 8-byte records; right: 18
//                   byte planes (channel c: planes 6c .. 6c+5, in k_features' order) MIRRORED in x.
//   k_hsum_c3     : k_hsum with the three channels' Birchfield-Tomasi terms added before they enter the LDS ring.
#pragma once
#include "kernels_cost.h"

namespace sgm {

constexpr int C3_PLANES = 18;  // right-image byte planes of a colour pair: 3 channels x (gradient, raw) x (value, lo, hi)

// blockIdx.z = 0: left image -> left_rec; 1: right image -> right_planes (one launch for the pair)
__global__ __launch_bounds__(256) void k_features_c3(const uint8_t *__restrict__ imgL, const uint8_t *__restrict__ imgR,
                                                     int64_t stride, int H, int W, int ftzero,
                                                     uint2 *__restrict__ left_rec_,
                                                     uint8_t *__restrict__ right_planes_)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= W) return;
    const bool is_right = blockIdx.z != 0;
    const uint8_t *img = is_right ? imgR : imgL;
    const uint8_t *row = img + (int64_t)y * stride;
    const uint8_t *up = y > 0 ? row - stride : row;
    const uint8_t *dn = y < H - 1 ? row + stride : row;
    const int64_t psz = (int64_t)H * W;
    const int64_t o = (int64_t)y * W + (W - 1 - x);  // mirrored position in a right plane
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        int pf[3], rw[3];  // values at x-1, x, x+1 of this channel (only read where they exist)
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int xx = x + k - 1;
            if (xx <= 0 || xx >= W - 1) {  // border columns hold ftzero in all six planes (A.2, A.10), as a byte
                pf[k] = ftzero & 0xff;
                rw[k] = ftzero & 0xff;
            } else {
                const int a = 3 * (xx + 1) + ch, b = 3 * (xx - 1) + ch;
                int g = 2 * ((int)row[a] - (int)row[b]) + ((int)up[a] - (int)up[b]) + ((int)dn[a] - (int)dn[b]);
                pf[k] = (min(max(g, -ftzero), ftzero) + ftzero) & 0xff;  // a byte, as in k_features
                rw[k] = row[3 * xx + ch];
            }
        }
        uint32_t out[2];
#pragma unroll
        for (int c = 0; c < 2; c++) {
            const int *v = c == 0 ? pf : rw;
            const int a = v[1];
            const int l = x > 0 ? (a + v[0]) / 2 : a;
            const int r = x < W - 1 ? (a + v[2]) / 2 : a;
            const int lo = min(a, min(l, r)), hi = max(a, max(l, r));
            out[c] = (uint32_t)a | ((uint32_t)lo << 8) | ((uint32_t)hi << 16);
        }
        if (!is_right) {
            left_rec_[((int64_t)y * W + x) * 3 + ch] = make_uint2(out[0], out[1]);
        } else {
#pragma unroll
            for (int c = 0; c < 2; c++) {
                right_planes_[(ch * 6 + c * 3 + 0) * psz + o] = (uint8_t)(out[c] & 0xff);
                right_planes_[(ch * 6 + c * 3 + 1) * psz + o] = (uint8_t)((out[c] >> 8) & 0xff);
                right_planes_[(ch * 6 + c * 3 + 2) * psz + o] = (uint8_t)((out[c] >> 16) & 0xff);
            }
        }
    }
}

// LDS layout of one k_hsum_c3 workgroup (one wave): [ring RS*64*NP dwords][3 left records per column][18 planes]
static inline HsumLds hsum_c3_lds_layout(int NP, int RS, int XL, int SW2)
{
    HsumLds l;
    l.ring_bytes = RS * 64 * NP * 4;
    const int nj = XL + 2 * SW2 + 2;
    l.lrec_bytes = ((nj * 3 * 8) + 15) & ~15;
    l.seg_len = (nj + 128 * NP + 15) & ~15;
    l.total_bytes = l.ring_bytes + l.lrec_bytes + C3_PLANES * l.seg_len;
    return l;
}

// pix of one column for this lane's NP packed disparity pairs: the sum of the three channels' single-channel costs
template <int NP>
__device__ __forceinline__ void pix_c3(const uint2 *rec3, const uint32_t (&w)[C3_PLANES][NP], uint32_t (&pix)[NP])
{
#pragma unroll
    for (int i = 0; i < NP; i++) pix[i] = 0;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        const uint2 rec = rec3[ch];
        const uint32_t U = splat_byte<0>(rec.x), U0 = splat_byte<1>(rec.x), U1 = splat_byte<2>(rec.x);
        const uint32_t R = splat_byte<0>(rec.y), R0 = splat_byte<1>(rec.y), R1 = splat_byte<2>(rec.y);
#pragma unroll
        for (int i = 0; i < NP; i++) {
            const uint32_t a = bt_pair(U, U0, U1, w[6 * ch + 0][i], w[6 * ch + 1][i], w[6 * ch + 2][i]);
            const uint32_t b = bt_pair(R, R0, R1, w[6 * ch + 3][i], w[6 * ch + 4][i], w[6 * ch + 5][i]);
            pix[i] = pk_add(pix[i], pk_add(a, pk_shr_u(b, 2)));
        }
    }
}

// k_hsum for colour pairs: one wave per (row, chunk of XL output columns), lanes span the disparities, sliding windows of
// the 18 right-image planes in registers, a ring of the last RS summed pixel-cost columns in LDS, the running horizontal
// sum stored as int16 (the input of k_vsum_ring / k_vsum).  RS_T > 0: the unrolled interior fast path of k_hsum.
template <int NP, int RS_T>
__global__ __launch_bounds__(64) void k_hsum_c3(Geom g, const uint2 *__restrict__ lrec, const uint8_t *__restrict__ rplanes,
                                                int16_t *__restrict__ hsum, int XL, int nchunks, int RS, int ring_bytes,
                                                int lrec_bytes, int seg_len)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint32_t *ring = reinterpret_cast<uint32_t *>(smem);
    uint2 *lds_lrec = reinterpret_cast<uint2 *>(smem + ring_bytes);  // [column - j0][channel]
    uint8_t *seg = smem + ring_bytes + lrec_bytes;

    const int lane = threadIdx.x;
    const int unit = blockIdx.x;
    const int y = __builtin_amdgcn_readfirstlane(unit / nchunks), ck = unit - y * nchunks;  // (uniform: see uniform_rsrc)
    const int W1 = g.W1, SW2 = g.SW2, W = g.W;
    const int xs = ck * XL, xe = min(xs + XL, W1);
    const int j0 = max(xs - SW2 - 1, 0), j1 = min(xe - 1 + SW2, W1 - 1);
    const int nj = j1 - j0 + 1;
    const bool active = 2 * NP * lane < g.D;

    // ---- stage this row's features for the chunk (the three records of a column are adjacent in lrec) ----
    {
        const uint2 *src = lrec + ((int64_t)y * W + (j0 + g.minX1)) * 3;
        for (int k = lane; k < 3 * nj; k += 64) lds_lrec[k] = src[k];
    }
    {
        // mirrored position of (column j, disparity index e): (W-1-(j+minX1)) + minD + e
        const int base_j1 = W - 1 - (j1 + g.minX1) + g.minD;
        const int len = (j1 - j0) + 128 * NP;
        const int64_t psz = (int64_t)g.H * W;
        for (int s = lane; s < len; s += 64) {
            const int pos = base_j1 + s;
            const bool ok = pos >= 0 && pos < W;
#pragma unroll
            for (int c = 0; c < C3_PLANES; c++)
                seg[c * seg_len + s] = ok ? rplanes[c * psz + (int64_t)y * W + pos] : (uint8_t)0;
        }
    }
    __syncthreads();  // single wave; orders the LDS staging before the reads below

    // ---- sliding windows of the 18 right-image planes ----
    uint32_t w[C3_PLANES][NP];
    {
        const int off = (j1 - j0) + 2 * NP * lane;
#pragma unroll
        for (int c = 0; c < C3_PLANES; c++)
#pragma unroll
            for (int i = 0; i < NP; i++)
                w[c][i] = (uint32_t)seg[c * seg_len + off + 2 * i] | ((uint32_t)seg[c * seg_len + off + 2 * i + 1] << 16);
    }

    uint32_t hs[NP];
#pragma unroll
    for (int i = 0; i < NP; i++) hs[i] = 0;
    int next_x = xs;
    // this row of the output as a buffer resource; lanes past D get an out-of-range offset, so their stores are dropped
    // by the bounds check instead of by a branch
    const int row_bytes = W1 * g.D * 2;
    const __amdgpu_buffer_rsrc_t orow = uniform_rsrc(hsum, (int64_t)y * g.rowsz * 2, row_bytes);
    const int voff = active ? 4 * NP * lane : row_bytes;
    const int pxb = g.D * 2;

    // the generic step: column j with every clamp and the first-output special case
    auto column = [&](int j) {
        if (j > j0) {
            const int off = (j1 - j) + 2 * NP * lane;
#pragma unroll
            for (int c = 0; c < C3_PLANES; c++) {
                const uint32_t nw = seg[c * seg_len + off];
#pragma unroll
                for (int i = NP - 1; i >= 1; i--) w[c][i] = __builtin_amdgcn_alignbit(w[c][i], w[c][i - 1], 16);
                w[c][0] = (w[c][0] << 16) | nw;
            }
        }
        uint32_t pix[NP];
        pix_c3<NP>(lds_lrec + 3 * (j - j0), w, pix);
        uint32_t *slot = ring + ((j & (RS - 1)) * 64 + lane) * NP;
#pragma unroll
        for (int i = 0; i < NP; i++) slot[i] = pix[i];
        // every output column whose right-most (clamped) tap is now available
        while (next_x < xe && min(next_x + SW2, W1 - 1) <= j) {
            const int x = next_x;
            if (x == xs) {
#pragma unroll
                for (int i = 0; i < NP; i++) hs[i] = 0;
                for (int t = -SW2; t <= SW2; t++) {
                    const int jc = min(max(x + t, 0), W1 - 1);
                    const uint32_t *p = ring + ((jc & (RS - 1)) * 64 + lane) * NP;
#pragma unroll
                    for (int i = 0; i < NP; i++) hs[i] = pk_add(hs[i], p[i]);
                }
            } else {
                const uint32_t *pa = ring + ((min(x + SW2, W1 - 1) & (RS - 1)) * 64 + lane) * NP;
                const uint32_t *pb = ring + ((max(x - SW2 - 1, 0) & (RS - 1)) * 64 + lane) * NP;
#pragma unroll
                for (int i = 0; i < NP; i++) hs[i] = pk_sub(pk_add(hs[i], pa[i]), pb[i]);
            }
            Pack<NP> o;
#pragma unroll
            for (int i = 0; i < NP; i++) o.r[i] = hs[i];
            buf_store<NP>(o, orow, voff, x * pxb);
            next_x++;
        }
    };

    int j = j0;
    if (RS_T > 0) {
        const int bs = 2 * SW2 + 1;
        // fast columns (as in k_hsum): exactly one output x = j - SW2, not the chunk's first, no clamped tap
        int ja = max(xs + 1 + SW2, j0 + bs);
        ja = (ja + RS_T - 1) & ~(RS_T - 1);
        const int jb = min(xe - 1 + SW2, W1 - 2);  // last fast column
        if (ja + RS_T - 1 <= jb) {
            for (; j < ja; j++) column(j);
            const uint32_t *ring_lane = ring + lane * NP;
            uint32_t *ring_lane_w = ring + lane * NP;
            // per-lane tap address of plane 0 for the block's LAST column (plane c is seg_len * c further on)
            int tap = 2 * NP * lane + (j1 - j) - (RS_T - 1);
            // the record address is the same in every lane; hidden from the compiler so that the records stay in VGPRs
            int recp = 3 * (j - j0);
            asm volatile("" : "+v"(recp));
            int so = (j - SW2) * pxb;
            for (; j + RS_T - 1 <= jb; j += RS_T) {
#pragma unroll
                for (int u = 0; u < RS_T; u++) {  // column j + u, ring slot u
#pragma unroll
                    for (int c = 0; c < C3_PLANES; c++) {
                        const uint32_t nw = seg[c * seg_len + tap + (RS_T - 1 - u)];
#pragma unroll
                        for (int i = NP - 1; i >= 1; i--) w[c][i] = __builtin_amdgcn_alignbit(w[c][i], w[c][i - 1], 16);
                        w[c][0] = (w[c][0] << 16) | nw;
                    }
                    uint32_t pix[NP];
                    pix_c3<NP>(lds_lrec + recp + 3 * u, w, pix);
                    const uint32_t *old = ring_lane + ((u - bs) & (RS_T - 1)) * 64 * NP;  // column j + u - bs
                    Pack<NP> o;
#pragma unroll
                    for (int i = 0; i < NP; i++) {
                        hs[i] = pk_sub(pk_add(hs[i], pix[i]), old[i]);
                        ring_lane_w[u * 64 * NP + i] = pix[i];
                        o.r[i] = hs[i];
                    }
                    buf_store<NP>(o, orow, voff, so);
                    so += pxb;
                }
                tap -= RS_T;
                recp += 3 * RS_T;
            }
            next_x = j - SW2;
        }
    }
    for (; j <= j1; j++) column(j);
}

}  // namespace sgm
