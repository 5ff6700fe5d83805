// kernels_icp.h -- rigid registration of two point clouds (include/sgm_hip_icp.h: sgm_register_icp, sgm_evaluate_registration,
// sgm_transform_points): per source point the nearest target point within r under the current transform, the 28 sums of the
// Gauss-Newton system over those pairs, and the transform applied to a list.  The header's definition is the contract.  The target's
// grid of cells is radius_build_grid's, unchanged; the 6 x 6 solve and the update run on the host (sgm_icp_solve).
//
//   k_icp_correspond  THE HOT KERNEL.  One lane per source point in SOURCE order: validity, the three fused multiply-adds per
//                     coordinate of step 2, the range rule, then rad_walk over the TARGET's table with a visitor that keeps
//                     (d2, index) in two registers -- no early stop, the tie compare on the index word.  The first caller of rad_walk
//                     whose query point is not a record of the grid: nothing is "self", and the lane's own cell may be empty (the
//                     probe then ends at the first EMPTY slot like any other).  Writes corr and d2; counts the valid and the unplaced.
//   k_icp_terms       one lane per source point: the pair's 28 binary64 terms (step 4) in registers, the canonical pairwise tree
//                     inside the wave by shuffles (lane 2k takes lane 2k + 1, then 4k takes 4k + 2, ...), across the four waves in
//                     LDS, one record of 28 doubles per 256-aligned block.  Integer counts by ballots and one atomic per wave.
//   k_icp_reduce      ONE workgroup continues the same tree over the blocks' records, 1024 at a time, then over the chunks: the
//                     tree's shape is a function of ns alone, never of a grid size.  Leaves the 232-byte result record.
//   k_icp_transform   step 2 on a point list; normals by the rotation part only.
// The tree pads with +0.0 up to the next power of two N of ns; positions past N, which exist only because a block has 256 lanes
// and a chunk 1024 records, hold -0.0, the one value x + (-0.0) = x is exact for, every x and both zeros included.
// Only + - * and conversions run here in binary64; every division and the square root are the host's.  No atomics on floats.
// The build has -ffp-contract=off: every fused operation below is written as fmaf.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_radius.h"

namespace sgm {

constexpr int ICP_SUMS = 28;                       // 21 of the upper triangle, 6 of the right-hand side, the sum of d2
constexpr int ICP_MAX_ITERATION = 1000;
constexpr int ICP_REDUCE_CHUNK = 1024;             // k_icp_reduce: records per step = its block size
constexpr uint32_t ICP_QNAN = 0x7FC00000u;

struct IcpResult {   // what the host reads per evaluation: 232 bytes
    double sums[ICP_SUMS];
    uint32_t n_corr, pad;
};
static_assert(sizeof(IcpResult) == 232, "the per-evaluation readback is one 232-byte copy");

struct IcpCtl {      // the counts of one evaluation, zeroed before it
    uint32_t m_s, unplaced, n_corr, unusable;
};

struct IcpM {        // the 12 entries of T rounded to binary32, row-major
    float m[12];
};

// step 2: three fused multiply-adds per coordinate, starting from the translation
__device__ __forceinline__ void icp_apply(const IcpM &M, float x, float y, float z, float &px, float &py, float &pz)
{
    px = __builtin_fmaf(M.m[2], z, __builtin_fmaf(M.m[1], y, __builtin_fmaf(M.m[0], x, M.m[3])));
    py = __builtin_fmaf(M.m[6], z, __builtin_fmaf(M.m[5], y, __builtin_fmaf(M.m[4], x, M.m[7])));
    pz = __builtin_fmaf(M.m[10], z, __builtin_fmaf(M.m[9], y, __builtin_fmaf(M.m[8], x, M.m[11])));
}

__global__ __launch_bounds__(256) void k_icp_correspond(const float *__restrict__ xyz_s, const float *__restrict__ disp_s, int64_t ns, IcpM M,
                                                        const float4 *__restrict__ sorted, const RadSlot *__restrict__ tab, uint32_t mask,
                                                        RadGrid G, int32_t *__restrict__ corr, float *__restrict__ d2out,
                                                        IcpCtl *__restrict__ ctl)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool valid = false, unplaced = false;
    if (i < ns) {
        const float x = xyz_s[i * 3], y = xyz_s[i * 3 + 1], z = xyz_s[i * 3 + 2];
        valid = isfinite(x) && isfinite(y) && isfinite(z) && (!disp_s || disp_s[i] > 0.0f);
        float best = __builtin_inff();
        uint32_t bi = VOX_NONE;
        if (valid) {
            float px, py, pz;
            icp_apply(M, x, y, z, px, py, pz);
            uint32_t g;
            unplaced = !(isfinite(px) && isfinite(py) && isfinite(pz) && radius_axis(px, G.ox, G.inv, g) && radius_axis(py, G.oy, G.inv, g) &&
                         radius_axis(pz, G.oz, G.inv, g));
            if (!unplaced && tab)   // (tab null: no target point is in range, nobody has a correspondence)
                rad_walk(sorted, tab, mask, G, px, py, pz, [] { return true; }, [&](bool inside, uint32_t w, float, float, float, float d2) {
                    if (inside && (d2 < best || (d2 == best && w < bi))) best = d2, bi = w;
                });
        }
        corr[i] = bi == VOX_NONE ? -1 : (int32_t)bi;
        d2out[i] = bi == VOX_NONE ? __uint_as_float(ICP_QNAN) : best;
    }
    const uint32_t nv = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(valid));
    const uint32_t nu = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(unplaced));
    if ((threadIdx.x & 63) == 0) {
        if (nv) atomicAdd(&ctl->m_s, nv);
        if (nu) atomicAdd(&ctl->unplaced, nu);
    }
}

// the canonical tree inside a wave: afterwards lane 0 holds ((l0 + l1) + (l2 + l3)) + ...
__device__ __forceinline__ double icp_wave_tree(double v)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v = v + __shfl_down(v, o);
    return v;
}

// the same tree over c[0], c[stride], ... (cnt of them, a power of two) in place, by one thread
__device__ __forceinline__ double icp_serial_tree(double *c, int cnt, int stride)
{
    for (int s = 1; s < cnt; s <<= 1)
        for (int k = 0; k < cnt; k += 2 * s) c[k * stride] = c[k * stride] + c[(k + s) * stride];
    return c[0];
}

__global__ __launch_bounds__(256) void k_icp_terms(const float *__restrict__ xyz_s, int64_t ns, int64_t npad, IcpM M,
                                                   const float *__restrict__ xyz_t, const float *__restrict__ nrm_t, int estimation,
                                                   const int32_t *__restrict__ corr, const float *__restrict__ d2in,
                                                   double *__restrict__ partial, IcpCtl *__restrict__ ctl)
{
    __shared__ double red[4 * ICP_SUMS];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int32_t c = i < ns ? corr[i] : -1;
    const double fill = i < npad ? 0.0 : -0.0;   // past the tree's padded length: the neutral element
    double s[ICP_SUMS];
#pragma unroll
    for (int j = 0; j < ICP_SUMS; j++) s[j] = fill;
    bool unusable = false;
    if (c >= 0) {
        float fx, fy, fz;
        icp_apply(M, xyz_s[i * 3], xyz_s[i * 3 + 1], xyz_s[i * 3 + 2], fx, fy, fz);
        const double px = (double)fx, py = (double)fy, pz = (double)fz;
        const double dx = px - (double)xyz_t[(int64_t)c * 3], dy = py - (double)xyz_t[(int64_t)c * 3 + 1],
                     dz = pz - (double)xyz_t[(int64_t)c * 3 + 2];
        s[27] = (double)d2in[i];
        if (estimation == 1) {
            const float n0 = nrm_t[(int64_t)c * 3], n1 = nrm_t[(int64_t)c * 3 + 1], n2 = nrm_t[(int64_t)c * 3 + 2];
            const float len2 = (n0 * n0 + n1 * n1) + n2 * n2;
            unusable = !(isfinite(n0) && isfinite(n1) && isfinite(n2) && len2 >= 0.25f && len2 <= 4.0f);
            if (!unusable) {
                const double nx = (double)n0, ny = (double)n1, nz = (double)n2;
                const double e = (nx * dx + ny * dy) + nz * dz;
                const double a[6] = {py * nz - pz * ny, pz * nx - px * nz, px * ny - py * nx, nx, ny, nz};
#pragma unroll
                for (int r = 0; r < 6; r++)
#pragma unroll
                    for (int q = r; q < 6; q++) s[r * 6 - r * (r - 1) / 2 + (q - r)] = a[r] * a[q];   // (row r begins at 0, 6, 11, 15, 18, 20)
#pragma unroll
                for (int r = 0; r < 6; r++) s[21 + r] = -(a[r] * e);
            }
        } else {
            // J = [-[p']x | I]: the upper triangle of J^T J in row order, then -J^T d
            s[0] = py * py + pz * pz, s[1] = -(px * py), s[2] = -(px * pz), s[3] = 0.0, s[4] = -pz, s[5] = py;
            s[6] = px * px + pz * pz, s[7] = -(py * pz), s[8] = pz, s[9] = 0.0, s[10] = -px;
            s[11] = px * px + py * py, s[12] = -py, s[13] = px, s[14] = 0.0;
            s[15] = 1.0, s[16] = 0.0, s[17] = 0.0, s[18] = 1.0, s[19] = 0.0, s[20] = 1.0;
            s[21] = -(py * dz - pz * dy), s[22] = -(pz * dx - px * dz), s[23] = -(px * dy - py * dx);
            s[24] = -dx, s[25] = -dy, s[26] = -dz;
        }
    }
#pragma unroll
    for (int j = 0; j < ICP_SUMS; j++) {
        const double v = icp_wave_tree(s[j]);
        if (lane == 0) red[w * ICP_SUMS + j] = v;
    }
    const uint32_t nc = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(c >= 0));
    const uint32_t nu = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(unusable));
    if (lane == 0) {
        if (nc) atomicAdd(&ctl->n_corr, nc);
        if (nu) atomicAdd(&ctl->unusable, nu);
    }
    __syncthreads();
    if (threadIdx.x < ICP_SUMS) {
        const int j = threadIdx.x;
        // planar: sum j of every block side by side, so that k_icp_reduce's lanes read consecutive doubles
        partial[(int64_t)j * gridDim.x + blockIdx.x] = (red[j] + red[ICP_SUMS + j]) + (red[2 * ICP_SUMS + j] + red[3 * ICP_SUMS + j]);
    }
}

// nparts records (planar: partial[j][nparts], as k_icp_terms leaves them with a grid of nparts blocks), padded to npow (a power of
// two) with +0.0; one workgroup of ICP_REDUCE_CHUNK lanes, at most 64 chunks
__global__ __launch_bounds__(ICP_REDUCE_CHUNK) void k_icp_reduce(const double *__restrict__ partial, uint32_t nparts, uint32_t npow,
                                                                 const IcpCtl *__restrict__ ctl, IcpResult *__restrict__ res)
{
    __shared__ double wred[16 * ICP_SUMS];
    __shared__ double chunk[64 * ICP_SUMS];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t nchunks = (npow + ICP_REDUCE_CHUNK - 1) / ICP_REDUCE_CHUNK;   // (1, or npow / 1024: a power of two <= 64)
    for (uint32_t ch = 0; ch < nchunks; ch++) {
        const uint32_t idx = ch * ICP_REDUCE_CHUNK + threadIdx.x;
#pragma unroll
        for (int j = 0; j < ICP_SUMS; j++) {
            const double v = icp_wave_tree(idx < nparts ? partial[(size_t)j * nparts + idx] : (idx < npow ? 0.0 : -0.0));
            if (lane == 0) wred[w * ICP_SUMS + j] = v;
        }
        __syncthreads();
        if (threadIdx.x < ICP_SUMS) chunk[ch * ICP_SUMS + threadIdx.x] = icp_serial_tree(wred + threadIdx.x, 16, ICP_SUMS);
        __syncthreads();
    }
    if (threadIdx.x < ICP_SUMS) res->sums[threadIdx.x] = icp_serial_tree(chunk + threadIdx.x, (int)nchunks, ICP_SUMS);
    if (threadIdx.x == 0) res->n_corr = ctl->n_corr, res->pad = 0u;
}

// sgm_transform_points: the points by step 2; the normals by the rotation part, the first term a plain product.  In place is
// sound: a lane reads its own three values before it writes them.
__global__ __launch_bounds__(256) void k_icp_transform(const float *xyz, const float *nrm, int64_t n, IcpM M, float *out_xyz, float *out_nrm)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (out_xyz) {
        float px, py, pz;
        icp_apply(M, xyz[i * 3], xyz[i * 3 + 1], xyz[i * 3 + 2], px, py, pz);
        out_xyz[i * 3] = px, out_xyz[i * 3 + 1] = py, out_xyz[i * 3 + 2] = pz;
    }
    if (out_nrm) {
        const float x = nrm[i * 3], y = nrm[i * 3 + 1], z = nrm[i * 3 + 2];
        const float qx = __builtin_fmaf(M.m[2], z, __builtin_fmaf(M.m[1], y, M.m[0] * x));
        const float qy = __builtin_fmaf(M.m[6], z, __builtin_fmaf(M.m[5], y, M.m[4] * x));
        const float qz = __builtin_fmaf(M.m[10], z, __builtin_fmaf(M.m[9], y, M.m[8] * x));
        out_nrm[i * 3] = qx, out_nrm[i * 3 + 1] = qy, out_nrm[i * 3 + 2] = qz;
    }
}

}  // namespace sgm
