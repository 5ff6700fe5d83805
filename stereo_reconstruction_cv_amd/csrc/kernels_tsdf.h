// kernels_tsdf.h -- the truncated signed distance volume (include/sgm_hip_tsdf.h: sgm_tsdf_integrate, sgm_tsdf_extract_points):
// one frame into the caller's planes, and the zero crossings of the planes as an ordered point list.  The header's definition is
// the contract.
//
//   k_tsdf_integrate  THE HOT KERNEL.  One lane per voxel, x along the wave: a wave is 64 consecutive voxels of one (j, k) row, a
//                     workgroup four consecutive rows of one 64-voxel column of rows, so every plane access of a wave is one
//                     contiguous 256 bytes.  Steps 1 to 7 in registers; the frame is read by a gather (12 + 4 bytes of the one
//                     pixel the voxel projects to, + 3 of its colour), which the caches serve: neighbouring voxels hit
//                     neighbouring pixels.  Only a voxel that reaches step 7 reads its weight, only one that is updated reads and
//                     writes its sum (and colour sums): outside, no-depth and occluded voxels cost no plane traffic.  One lane owns
//                     each voxel, so no atomic touches the volume.  Plane offsets are 64-bit.  No LDS, no scratch.  The six counts are
//                     an instantiation of their own (STATS): six ballots per wave, the workgroup's sums in 24 bytes of LDS, ONE
//                     atomic instruction per workgroup (lane c < 6 adds count c) into one of 256 copies of the record, a 64-byte
//                     line each, which the host adds up (why not one atomic per wave into one record: DESIGN.md 4.28).
//   k_tsdf_usable     the seventh count (usable pixels of the frame), only when the counts are asked for: a ballot and one atomic
//                     per wave.  Part of the tsdf_integrate stage.
//   k_tsdf_count      per 1024 consecutive voxels the number of crossings (0 .. 3 per voxel): four rounds of 256 lanes, dword
//                     accesses, a voxel below min_weight reads nothing but its weight.
//   k_tsdf_scan       ONE workgroup: the exclusive scan of the blocks' counts into 64-bit offsets, the total behind them.  The
//                     shape of k_compact_scan (kernels_post.h), which itself keeps 32-bit totals in place; this one reads uint32
//                     counts and writes uint64 offsets, so V = 2^30 with three crossings per voxel is inside its range.
//   k_tsdf_emit       recomputes the crossings of its 1024 voxels and writes them at the scanned offsets: the position inside the
//                     block from ballots and popcounts (x, y, z of a voxel adjacent), across rounds and waves through 16 words of
//                     LDS.  A block without crossings, or wholly past the capacity, returns after one load.
// The build has -ffp-contract=off: every fused operation below is written as fmaf.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sgm {

constexpr int TSDF_MAX_DIM = 4096;
constexpr int64_t TSDF_MAX_VOXELS = (int64_t)1 << 30;
constexpr int64_t TSDF_MAX_PIXELS = (int64_t)1 << 27;
constexpr int TSDF_MAX_WEIGHT = 65535;
constexpr int TSDF_STAT_SLOTS = 256;              // copies of the eight counts of an integration, a 64-byte line each; the host adds them up
constexpr int TSDF_BLOCK_VOXELS = 1024;            // k_tsdf_count / k_tsdf_emit: voxels per workgroup, four rounds of 256

struct TsdfVol {     // the volume: dimensions, voxel size, origin
    int nx, ny, nz;
    float vs, ox, oy, oz;
};

struct TsdfFrame {   // the frame: M (the extrinsic's first three rows in binary32), the camera, the signs and the limits
    float m[12];
    float fx, fy, cx, cy, front, max_depth, tau, kappa;
    int H, W;
};

// step 1: the centre of voxel index i along one axis
__device__ __forceinline__ float tsdf_centre(int i, float vs, float o) { return __builtin_fmaf((float)i + 0.5f, vs, o); }

// step 5: X, Y, Z finite, disp > 0 (a null disp passes), in front and within max_depth
__device__ __forceinline__ bool tsdf_pixel_usable(const float *__restrict__ xyz, const float *__restrict__ disp, int64_t pix, float front,
                                                  float max_depth, float &Z)
{
    const float X = xyz[pix * 3], Y = xyz[pix * 3 + 1];
    Z = xyz[pix * 3 + 2];
    if (!(isfinite(X) && isfinite(Y) && isfinite(Z))) return false;
    if (disp && !(disp[pix] > 0.0f)) return false;
    const float d = front * Z;
    return d > 0.0f && d <= max_depth;
}

// classes of a voxel in one frame: the order of out_stats[1 ..], with "updated" = the first two
enum { TSDF_UPD = 0, TSDF_UPD_CLAMPED = 1, TSDF_NO_DEPTH = 2, TSDF_OCCLUDED = 3, TSDF_SATURATED = 4, TSDF_OUTSIDE = 5, TSDF_NONE = 6 };

// STATS: the six counts are wanted.  An instantiation of its own, so that the plain kernel carries neither the ballots nor any LDS.
template <bool STATS>
__global__ __launch_bounds__(256) void k_tsdf_integrate(TsdfVol vol, TsdfFrame fr, uint32_t xchunks, uint32_t rows, int64_t V,
                                                        int32_t *__restrict__ sum, int32_t *__restrict__ weight, uint32_t *__restrict__ rgb,
                                                        const float *__restrict__ xyz, const float *__restrict__ disp,
                                                        const uint8_t *__restrict__ colors, unsigned long long *__restrict__ stats)
{
    const uint32_t xc = blockIdx.x % xchunks, rg = blockIdx.x / xchunks;
    const int lane = threadIdx.x & 63;
    const uint32_t row = rg * 4u + (threadIdx.x >> 6);
    const int i = (int)(xc * 64u) + lane;
    int cls = TSDF_NONE;
    if (row < rows && i < vol.nx) {
        const int j = (int)(row % (uint32_t)vol.ny), k = (int)(row / (uint32_t)vol.ny);
        const int64_t v = (int64_t)row * vol.nx + i;
        const float cx = tsdf_centre(i, vol.vs, vol.ox), cy = tsdf_centre(j, vol.vs, vol.oy), cz = tsdf_centre(k, vol.vs, vol.oz);
        const float px = __builtin_fmaf(fr.m[2], cz, __builtin_fmaf(fr.m[1], cy, __builtin_fmaf(fr.m[0], cx, fr.m[3])));
        const float py = __builtin_fmaf(fr.m[6], cz, __builtin_fmaf(fr.m[5], cy, __builtin_fmaf(fr.m[4], cx, fr.m[7])));
        const float pz = __builtin_fmaf(fr.m[10], cz, __builtin_fmaf(fr.m[9], cy, __builtin_fmaf(fr.m[8], cx, fr.m[11])));
        cls = TSDF_OUTSIDE;
        if (fr.front * pz > 0.0f) {
            const float iz = 1.0f / pz;
            const float u = __builtin_fmaf(fr.fx, px * iz, fr.cx) + 0.5f;
            const float w = __builtin_fmaf(fr.fy, py * iz, fr.cy) + 0.5f;
            if (u >= 0.0f && u < (float)fr.W && w >= 0.0f && w < (float)fr.H) {   // float comparisons first: NaN and inf fail
                const int qx = (int)__builtin_floorf(u), qy = (int)__builtin_floorf(w);
                const int64_t pix = (int64_t)qy * fr.W + qx;
                float Z;
                cls = TSDF_NO_DEPTH;
                if (tsdf_pixel_usable(xyz, disp, pix, fr.front, fr.max_depth, Z)) {
                    const float s = fr.front * (Z - pz);
                    cls = TSDF_OCCLUDED;
                    if (!(s < -fr.tau)) {
                        const float t = __builtin_fminf(s, fr.tau);
                        const int q = (int)__builtin_rintf(t * fr.kappa);
                        const int32_t wt = weight[v];
                        cls = TSDF_SATURATED;
                        if (wt != TSDF_MAX_WEIGHT) {
                            sum[v] += q;
                            weight[v] = wt + 1;
                            if (rgb) {
                                rgb[v] += colors[pix * 3];
                                rgb[V + v] += colors[pix * 3 + 1];
                                rgb[2 * V + v] += colors[pix * 3 + 2];
                            }
                            cls = s < fr.tau ? TSDF_UPD : TSDF_UPD_CLAMPED;
                        }
                    }
                }
            }
        }
    }
    if constexpr (STATS) {   // six ballots per wave, the workgroup's sums in LDS, then ONE atomic instruction per workgroup: lane c adds count c
        __shared__ uint32_t wg[6];
        if (threadIdx.x < 6) wg[threadIdx.x] = 0u;
        __syncthreads();
        const uint32_t n0 = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(cls == TSDF_UPD));
        const uint32_t n1 = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(cls == TSDF_UPD_CLAMPED));
        const uint32_t n2 = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(cls == TSDF_NO_DEPTH));
        const uint32_t n3 = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(cls == TSDF_OCCLUDED));
        const uint32_t n4 = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(cls == TSDF_SATURATED));
        const uint32_t n5 = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(cls == TSDF_OUTSIDE));
        const uint32_t c = lane == 0 ? n0 + n1 : lane == 1 ? n0 : lane == 2 ? n2 : lane == 3 ? n3 : lane == 4 ? n4 : n5;
        if (lane < 6 && c) atomicAdd(&wg[lane], c);
        __syncthreads();
        // the record is kept TSDF_STAT_SLOTS times, one 64-byte line each: workgroups that run together add to different lines
        if (threadIdx.x < 6 && wg[threadIdx.x])
            atomicAdd(&stats[(size_t)(blockIdx.x % TSDF_STAT_SLOTS) * 8 + threadIdx.x], (unsigned long long)wg[threadIdx.x]);
    }
}

__global__ __launch_bounds__(256) void k_tsdf_usable(const float *__restrict__ xyz, const float *__restrict__ disp, int64_t npix, float front,
                                                     float max_depth, unsigned long long *__restrict__ stats)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    float Z;
    const bool ok = p < npix && tsdf_pixel_usable(xyz, disp, p, front, max_depth, Z);
    const unsigned long long b = __builtin_amdgcn_ballot_w64(ok);
    if ((threadIdx.x & 63) == 0 && b)
        atomicAdd(&stats[(size_t)(blockIdx.x % TSDF_STAT_SLOTS) * 8 + 6], (unsigned long long)__builtin_popcountll(b));
}

// The crossings of voxel v: bit a set iff the edge to the neighbour along +a is one.  i, j, k: the voxel's indices.
__device__ __forceinline__ uint32_t tsdf_crossings(const TsdfVol &vol, const int32_t *__restrict__ sum, const int32_t *__restrict__ weight,
                                                   int64_t v, int min_weight, int &i, int &j, int &k)
{
    if (weight[v] < min_weight) return 0u;
    const uint32_t rowi = (uint32_t)v / (uint32_t)vol.nx;      // (v < V <= 2^30: the index itself fits 32 bits, the byte offsets do not)
    i = (int)((uint32_t)v - rowi * (uint32_t)vol.nx), j = (int)(rowi % (uint32_t)vol.ny), k = (int)(rowi / (uint32_t)vol.ny);
    const bool neg = sum[v] < 0;
    const int64_t sx = 1, sy = vol.nx, sz = (int64_t)vol.nx * vol.ny;
    uint32_t m = 0u;
    if (i + 1 < vol.nx && weight[v + sx] >= min_weight && (sum[v + sx] < 0) != neg) m |= 1u;
    if (j + 1 < vol.ny && weight[v + sy] >= min_weight && (sum[v + sy] < 0) != neg) m |= 2u;
    if (k + 1 < vol.nz && weight[v + sz] >= min_weight && (sum[v + sz] < 0) != neg) m |= 4u;
    return m;
}

__global__ __launch_bounds__(256) void k_tsdf_count(TsdfVol vol, int64_t V, const int32_t *__restrict__ sum, const int32_t *__restrict__ weight,
                                                    int min_weight, uint32_t *__restrict__ counts)
{
    const int64_t base = (int64_t)blockIdx.x * TSDF_BLOCK_VOXELS;
    uint32_t n = 0u;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int64_t v = base + r * 256 + threadIdx.x;
        int i, j, k;
        if (v < V) n += (uint32_t)__builtin_popcount(tsdf_crossings(vol, sum, weight, v, min_weight, i, j, k));
    }
    for (int o = 32; o; o >>= 1) n += __shfl_down(n, o);
    __shared__ uint32_t wsum[4];
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// exclusive scan of m block counts (uint32) into 64-bit offsets by one workgroup; the total -> off[m]
__global__ __launch_bounds__(1024) void k_tsdf_scan(const uint32_t *__restrict__ counts, int m, unsigned long long *__restrict__ off)
{
    __shared__ unsigned long long part[1024];
    const int t = threadIdx.x;
    const int per = (m + 1023) / 1024;
    const int lo = min(t * per, m), hi = min(lo + per, m);
    unsigned long long s = 0;
    for (int i = lo; i < hi; i++) s += counts[i];
    part[t] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {  // inclusive Hillis-Steele scan of the partials
        const unsigned long long v = t >= o ? part[t - o] : 0ull;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    unsigned long long run = t ? part[t - 1] : 0ull;
    for (int i = lo; i < hi; i++) {
        off[i] = run;
        run += counts[i];
    }
    if (t == 1023) off[m] = part[1023];
}

// the averaged distance of a voxel and the rounded mean of one colour channel
__device__ __forceinline__ float tsdf_mean(int32_t s, int32_t w) { return (float)s / (float)w; }

__global__ __launch_bounds__(256) void k_tsdf_emit(TsdfVol vol, int64_t V, const int32_t *__restrict__ sum, const int32_t *__restrict__ weight,
                                                   const uint32_t *__restrict__ rgb, int min_weight,
                                                   const unsigned long long *__restrict__ off, int64_t capacity, float *__restrict__ out_p,
                                                   uint8_t *__restrict__ out_c)
{
    const unsigned long long first = off[blockIdx.x];
    if (off[blockIdx.x + 1] == first || first >= (unsigned long long)capacity) return;   // (uniform) nothing to write here
    const int64_t base = (int64_t)blockIdx.x * TSDF_BLOCK_VOXELS;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    __shared__ uint32_t wsum[16];
    uint32_t mk[4], pre[4];
    int vi[4], vj[4], vk[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int64_t v = base + r * 256 + threadIdx.x;
        vi[r] = vj[r] = vk[r] = 0;
        mk[r] = v < V ? tsdf_crossings(vol, sum, weight, v, min_weight, vi[r], vj[r], vk[r]) : 0u;
        const unsigned long long bx = __builtin_amdgcn_ballot_w64(mk[r] & 1u), by = __builtin_amdgcn_ballot_w64(mk[r] & 2u),
                                 bz = __builtin_amdgcn_ballot_w64(mk[r] & 4u);
        pre[r] = (uint32_t)(__builtin_popcountll(bx & below) + __builtin_popcountll(by & below) + __builtin_popcountll(bz & below));
        if (lane == 0) wsum[r * 4 + wv] = (uint32_t)(__builtin_popcountll(bx) + __builtin_popcountll(by) + __builtin_popcountll(bz));
    }
    __syncthreads();
    const int64_t step[3] = {1, vol.nx, (int64_t)vol.nx * vol.ny};
#pragma unroll
    for (int r = 0; r < 4; r++) {
        if (!mk[r]) continue;
        unsigned long long o = first + pre[r];
        for (int q = 0; q < r * 4 + wv; q++) o += wsum[q];
        const int64_t v = base + r * 256 + threadIdx.x;
        const int32_t w0 = weight[v];
        const float f0 = tsdf_mean(sum[v], w0);
        const float c[3] = {tsdf_centre(vi[r], vol.vs, vol.ox), tsdf_centre(vj[r], vol.vs, vol.oy), tsdf_centre(vk[r], vol.vs, vol.oz)};
#pragma unroll
        for (int a = 0; a < 3; a++) {
            if (!(mk[r] >> a & 1u)) continue;
            if (o < (unsigned long long)capacity) {
                const int64_t v1 = v + step[a];
                const int32_t w1 = weight[v1];
                const float f1 = tsdf_mean(sum[v1], w1);
                const float theta = f0 / (f0 - f1);
                float *p = out_p + o * 3;
                p[0] = a == 0 ? __builtin_fmaf(theta, vol.vs, c[0]) : c[0];
                p[1] = a == 1 ? __builtin_fmaf(theta, vol.vs, c[1]) : c[1];
                p[2] = a == 2 ? __builtin_fmaf(theta, vol.vs, c[2]) : c[2];
                if (out_c) {
                    const int64_t vc = theta <= 0.5f ? v : v1;
                    const int64_t wc = theta <= 0.5f ? w0 : w1;
#pragma unroll
                    for (int ch = 0; ch < 3; ch++)
                        out_c[o * 3 + ch] = (uint8_t)((2 * (int64_t)rgb[ch * V + vc] + wc) / (2 * wc));
                }
            }
            o++;
        }
    }
}

}  // namespace sgm
