// kernels_plane.h -- plane segmentation of a point cloud (include/sgm_hip_plane.h: sgm_segment_plane, sgm_plane_inliers): K seeded
// hypotheses from three valid points each, every hypothesis scored on every valid point, the best one refitted from integer
// moments, the cloud classified with the final model.  The header's definition is the contract; nothing here uses the grid of
// cells, and nothing is scattered: the hot kernel is points x hypotheses of dense binary32 arithmetic.
//
//   k_plane_valid_count / k_plane_valid_scatter   the ordered compaction of kernels_post.h (count -> k_compact_scan -> scatter)
//                     with the predicate of step 1; the valid points go to a float4 list (x, y, z, 0) in source order, so rank r
//                     of step 3 is entry r, and their number m to the call's control block.  Everything after reads m from there:
//                     the host sizes every grid from n and never waits for m.
//   k_plane_sample    one lane per hypothesis: the three ranks, the plane in binary64 (step 4), oriented and rounded (step 9).  A
//                     degenerate hypothesis is stored as four NaNs -- no point passes its test, its count stays 0 -- and counted.
//   k_plane_count_valu / k_plane_count_mfma   THE HOT KERNELS, two forms of step 5 with the same bits.  blockIdx.y is a tile of 64
//                     hypotheses, blockIdx.x strides over chunks of PLANE_CHUNK valid points, a wave takes a quarter of a chunk.
//                     valu: a lane owns a hypothesis; the chunk is staged in LDS, one array per coordinate (past the end: NaN,
//                     which fails the ordered <=), and every lane reads the same address per step, a broadcast; per pair three
//                     fused multiply-adds (the compiler pairs two points into v_pk_fma_f32, which the planar staging feeds
//                     without moves), one compare with |.|, one add-with-carry.  mfma: v_mfma_f32_16x16x4_f32 on 16 points x 16 hypotheses, A = the points' rows
//                     (x, y, z, 0) straight from the list (64 consecutive floats per step and wave), B = the planes' columns
//                     (a, b, c, 0), C = d per column: the k-ordered chain fma(0, 0, fma(c, z, fma(b, y, fma(a, x, d)))), whose
//                     last term can only turn -0 into +0.  Four independent accumulators per wave (the four sixteens of the
//                     tile); a lane's four results belong to one column, so it counts them itself and the four lanes of a column
//                     add up at the end.  Both: the block's four waves add in LDS, one integer atomic per hypothesis and block.
//   k_plane_best      one workgroup: the lowest k with the largest count (step 6), found or not, the anchor and the model of k*.
//   k_plane_moments   step 7's sums over the inliers of k*: per-lane int64 accumulators, wave shuffles, 64-bit LDS atomics, then
//                     eleven 64-bit global atomics per block (nine sums, m_r, the inliers out of refit range).  Integers: order-free.
//   k_plane_solve     one lane: cov_normal (kernels_covariance.h, the device function behind k_cov_solve), the centroid, step 9.
//   k_plane_classify  step 8, streaming: inlier byte, distance, the byte the compaction selects by, the number of inliers.  The
//                     selected points then go through k_radius_keep_count, k_compact_scan and k_radius_scatter.
// The build has -ffp-contract=off: every fused operation below is written as fmaf or comes from the matrix core.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_covariance.h"
#include "kernels_post.h"

namespace sgm {

constexpr int PLANE_MAX_K = 65536;
constexpr int PLANE_TILE = 64;      // hypotheses per blockIdx.y
constexpr int PLANE_CHUNK = 1024;   // valid points per step of a block: 256 per wave
constexpr int PLANE_COUNT_BLOCKS = 4096;
constexpr int PLANE_MOMENT_BLOCKS = 1024;
constexpr uint32_t PLANE_QNAN = 0x7FC00000u;
constexpr bool PLANE_DEFAULT_MFMA = false;   // which form of step 5 runs without SGM_DBG_PLANE_OTHER_COUNT (DESIGN.md 4.25 has the table)

struct PlaneCtl {   // the control block of one call, zeroed before it
    uint32_t m, degenerate, kbest, cbest, found, refined, n_inliers, pad;
    float model[4], anchor[4];
    long long S[9];
    unsigned long long m_r, n_oor;
};

typedef float plane_f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bool plane_valid(const float *__restrict__ xyz, const float *__restrict__ disp, int64_t i)
{
    const float X = xyz[i * 3], Y = xyz[i * 3 + 1], Z = xyz[i * 3 + 2];
    return isfinite(X) && isfinite(Y) && isfinite(Z) && (!disp || disp[i] > 0.0f);
}

// step 3: the rank of counter c among m valid points
__device__ __forceinline__ uint32_t plane_rank(uint32_t seed, uint32_t c, uint32_t m)
{
    uint32_t x = seed ^ (c * 0x9E3779B9u);
    x ^= x >> 16, x *= 0x7FEB352Du, x ^= x >> 15, x *= 0x846CA68Bu, x ^= x >> 16;
    return (uint32_t)(((unsigned long long)x * m) >> 32);
}

// step 9: a plane held in binary64, oriented and rounded
__device__ __forceinline__ float4 plane_round(double a, double b, double c, double d)
{
    const double first = a != 0.0 ? a : (b != 0.0 ? b : c);
    if (d < 0.0 || (d == 0.0 && first < 0.0)) a = -a, b = -b, c = -c, d = -d;
    return make_float4((float)a + 0.0f, (float)b + 0.0f, (float)c + 0.0f, (float)d + 0.0f);
}

// step 5: the signed distance, three fused multiply-adds from d
__device__ __forceinline__ float plane_dist(const float4 h, float x, float y, float z)
{
    return __builtin_fmaf(h.z, z, __builtin_fmaf(h.y, y, __builtin_fmaf(h.x, x, h.w)));
}

__global__ __launch_bounds__(256) void k_plane_valid_count(const float *__restrict__ xyz, const float *__restrict__ disp, int64_t n,
                                                           uint32_t *__restrict__ counts)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool v = i < n && plane_valid(xyz, disp, i);
    const unsigned long long b = __builtin_amdgcn_ballot_w64(v);
    __shared__ uint32_t wsum[4];
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = (uint32_t)__builtin_popcountll(b);
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

__global__ __launch_bounds__(256) void k_plane_valid_scatter(const float *__restrict__ xyz, const float *__restrict__ disp, int64_t n,
                                                             const uint32_t *__restrict__ offsets, int mblocks,
                                                             float4 *__restrict__ vpts, PlaneCtl *__restrict__ ctl)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool v = i < n && plane_valid(xyz, disp, i);
    const unsigned long long b = __builtin_amdgcn_ballot_w64(v);
    __shared__ uint32_t wsum[4];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) wsum[w] = (uint32_t)__builtin_popcountll(b);
    __syncthreads();
    uint32_t base = offsets[blockIdx.x];
    for (int k = 0; k < w; k++) base += wsum[k];
    if (v) {
        const uint32_t o = base + (uint32_t)__builtin_popcountll(b & ((1ull << lane) - 1ull));   // o <= i < n
        vpts[o] = make_float4(xyz[i * 3], xyz[i * 3 + 1], xyz[i * 3 + 2], 0.0f);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) ctl->m = offsets[mblocks];
}

__global__ __launch_bounds__(256) void k_plane_sample(const float4 *__restrict__ vpts, uint32_t K, uint32_t seed,
                                                      float4 *__restrict__ hyp, PlaneCtl *__restrict__ ctl)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    const uint32_t m = ctl->m;
    const float nan = __uint_as_float(PLANE_QNAN);
    float4 h = make_float4(nan, nan, nan, nan);
    bool degenerate = false;
    if (k < K && m >= 3u) {
        const float4 p0 = vpts[plane_rank(seed, 3u * k, m)], p1 = vpts[plane_rank(seed, 3u * k + 1u, m)],
                     p2 = vpts[plane_rank(seed, 3u * k + 2u, m)];   // (ranks < m)
        const double ax = (double)p1.x - (double)p0.x, ay = (double)p1.y - (double)p0.y, az = (double)p1.z - (double)p0.z;
        const double bx = (double)p2.x - (double)p0.x, by = (double)p2.y - (double)p0.y, bz = (double)p2.z - (double)p0.z;
        double n0 = ay * bz - az * by, n1 = az * bx - ax * bz, n2 = ax * by - ay * bx;
        const double len2 = (n0 * n0 + n1 * n1) + n2 * n2;
        degenerate = !(isfinite(len2) && len2 > 0.0);
        if (!degenerate) {
            const double len = sqrt(len2);
            n0 = n0 / len, n1 = n1 / len, n2 = n2 / len;
            const double d = -((n0 * (double)p0.x + n1 * (double)p0.y) + n2 * (double)p0.z);
            h = plane_round(n0, n1, n2, d);
        }
    }
    if (k < K) hyp[k] = h;
    const uint32_t nd = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(degenerate));
    if ((threadIdx.x & 63) == 0 && nd) atomicAdd(&ctl->degenerate, nd);
}

// the four waves' counts of one hypothesis tile added in LDS; one atomic per hypothesis and block
__device__ __forceinline__ void plane_count_flush(uint32_t (*red)[PLANE_TILE], int w, int slot, bool owner, uint32_t c, uint32_t K,
                                                  uint32_t *__restrict__ cnt)
{
    if (owner) red[w][slot] = c;
    __syncthreads();
    if (threadIdx.x < PLANE_TILE) {
        const uint32_t k = blockIdx.y * PLANE_TILE + threadIdx.x;
        const uint32_t t = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
        if (k < K && t) atomicAdd(&cnt[k], t);
    }
}

__global__ __launch_bounds__(256) void k_plane_count_valu(const float4 *__restrict__ vpts, const PlaneCtl *__restrict__ ctl,
                                                          const float4 *__restrict__ hyp, uint32_t K, float t,
                                                          uint32_t *__restrict__ cnt)
{
    __shared__ float sx[PLANE_CHUNK], sy[PLANE_CHUNK], sz[PLANE_CHUNK];   // (planar: two points' x are a v_pk_fma_f32 operand as read)
    __shared__ uint32_t red[4][PLANE_TILE];
    const uint32_t m = ctl->m;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t k = blockIdx.y * PLANE_TILE + lane;
    const float4 h = hyp[min(k, K - 1u)];   // (a lane past K scores the last hypothesis and adds nothing)
    const float nan = __uint_as_float(PLANE_QNAN);
    const uint32_t chunks = (m + PLANE_CHUNK - 1u) / PLANE_CHUNK;
    uint32_t c = 0;
    for (uint32_t ch = blockIdx.x; ch < chunks; ch += gridDim.x) {   // (m is the same for the whole block)
        __syncthreads();
        for (int j = threadIdx.x; j < PLANE_CHUNK; j += 256) {
            const uint32_t i = ch * PLANE_CHUNK + j;
            const float4 p = i < m ? vpts[i] : make_float4(nan, nan, nan, 0.0f);
            sx[j] = p.x, sy[j] = p.y, sz[j] = p.z;
        }
        __syncthreads();
        const int q = w * (PLANE_CHUNK / 4);
#pragma unroll 8
        for (int j = 0; j < PLANE_CHUNK / 4; j++) c += fabsf(plane_dist(h, sx[q + j], sy[q + j], sz[q + j])) <= t ? 1u : 0u;
    }
    plane_count_flush(red, w, lane, true, c, K, cnt);
}

// (two workgroups per compute unit asked for: at most 256 registers a lane, so the accumulators are VGPRs the compares can read)
__global__ __launch_bounds__(256, 2) void k_plane_count_mfma(const float4 *__restrict__ vpts, const PlaneCtl *__restrict__ ctl,
                                                          const float4 *__restrict__ hyp, uint32_t K, float t,
                                                          uint32_t *__restrict__ cnt)
{
    __shared__ uint32_t red[4][PLANE_TILE];
    const uint32_t m = ctl->m;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int col = lane & 15, kq = lane >> 4;   // the lane's column of B and C / D, and its k of A and B
    const float *__restrict__ vf = (const float *)vpts, *__restrict__ hf = (const float *)hyp;
    const float nan = __uint_as_float(PLANE_QNAN);
    float b[4];
    plane_f32x4 dv[4];
    uint32_t c[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int s = 0; s < 4; s++) {
        const uint32_t k = min(blockIdx.y * PLANE_TILE + s * 16 + col, K - 1u);
        b[s] = kq < 3 ? hf[4 * (size_t)k + kq] : 0.0f;
        const float d = hf[4 * (size_t)k + 3];
        dv[s] = plane_f32x4{d, d, d, d};
    }
    const float past = kq < 3 ? nan : 0.0f;   // the row of a point past the end: (NaN, NaN, NaN, 0)
    const uint32_t chunks = (m + PLANE_CHUNK - 1u) / PLANE_CHUNK;
    for (uint32_t ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
        const uint32_t base = ch * PLANE_CHUNK + w * (PLANE_CHUNK / 4);
        if (base >= m) continue;   // (the same for the whole wave)
#pragma unroll 4
        for (int st = 0; st < PLANE_CHUNK / 64; st++) {
            const uint32_t i = base + st * 16 + col;
            const float a = i < m ? vf[4 * (size_t)i + kq] : past;
#pragma unroll
            for (int s = 0; s < 4; s++) {
                const plane_f32x4 r = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[s], dv[s], 0, 0, 0);
                c[s] += fabsf(r[0]) <= t ? 1u : 0u;
                c[s] += fabsf(r[1]) <= t ? 1u : 0u;
                c[s] += fabsf(r[2]) <= t ? 1u : 0u;
                c[s] += fabsf(r[3]) <= t ? 1u : 0u;
            }
        }
    }
    // the four lanes of a column hold the counts of four rows each
#pragma unroll
    for (int s = 0; s < 4; s++) {
        c[s] += __shfl_xor(c[s], 16);
        c[s] += __shfl_xor(c[s], 32);
    }
    // lane 16 s' + col publishes sixteen s'
    const uint32_t mine = kq == 0 ? c[0] : (kq == 1 ? c[1] : (kq == 2 ? c[2] : c[3]));
    plane_count_flush(red, w, lane, true, mine, K, cnt);
}

__global__ __launch_bounds__(1024) void k_plane_best(const uint32_t *__restrict__ cnt, uint32_t K, uint32_t seed,
                                                     const float4 *__restrict__ hyp, const float4 *__restrict__ vpts,
                                                     PlaneCtl *__restrict__ ctl)
{
    __shared__ uint32_t bc[1024], bk[1024];
    const int t = threadIdx.x;
    uint32_t c = 0, kk = 0xFFFFFFFFu;
    for (uint32_t k = t; k < K; k += 1024u) {
        const uint32_t v = cnt[k];
        if (kk == 0xFFFFFFFFu || v > c) c = v, kk = k;   // (ascending k: the first of the largest)
    }
    bc[t] = c, bk[t] = kk;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if (t < o) {
            const uint32_t c2 = bc[t + o], k2 = bk[t + o];
            if (c2 > bc[t] || (c2 == bc[t] && k2 < bk[t])) bc[t] = c2, bk[t] = k2;
        }
        __syncthreads();
    }
    if (t == 0) {
        const uint32_t m = ctl->m, kb = bk[0], cb = bc[0];   // (K >= 1: kb < K)
        ctl->kbest = kb, ctl->cbest = cb;
        if (m >= 3u && cb >= 3u) {
            const float4 h = hyp[kb], a = vpts[plane_rank(seed, 3u * kb, m)];
            ctl->found = 1u;
            ctl->model[0] = h.x, ctl->model[1] = h.y, ctl->model[2] = h.z, ctl->model[3] = h.w;
            ctl->anchor[0] = a.x, ctl->anchor[1] = a.y, ctl->anchor[2] = a.z, ctl->anchor[3] = 0.0f;
        }
    }
}

__device__ __forceinline__ long long plane_wave_sum(long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}

__global__ __launch_bounds__(256) void k_plane_moments(const float4 *__restrict__ vpts, PlaneCtl *__restrict__ ctl, float t, float qscale)
{
    __shared__ unsigned long long acc[11];
    if (!ctl->found) return;   // (the same for every lane of the grid)
    if (threadIdx.x < 11) acc[threadIdx.x] = 0ull;
    __syncthreads();
    const uint32_t m = ctl->m;
    const float4 h = make_float4(ctl->model[0], ctl->model[1], ctl->model[2], ctl->model[3]);
    const float ax = ctl->anchor[0], ay = ctl->anchor[1], az = ctl->anchor[2];
    long long s[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < m; i += gridDim.x * 256u) {
        const float4 p = vpts[i];
        if (!(fabsf(plane_dist(h, p.x, p.y, p.z)) <= t)) continue;
        const float ux = (p.x - ax) * qscale, uy = (p.y - ay) * qscale, uz = (p.z - az) * qscale;
        if (!(fabsf(ux) <= 524288.0f && fabsf(uy) <= 524288.0f && fabsf(uz) <= 524288.0f)) {
            s[10] += 1;
            continue;
        }
        const long long qx = (int)rintf(ux), qy = (int)rintf(uy), qz = (int)rintf(uz);
        s[0] += qx, s[1] += qy, s[2] += qz;
        s[3] += qx * qx, s[4] += qx * qy, s[5] += qx * qz, s[6] += qy * qy, s[7] += qy * qz, s[8] += qz * qz;
        s[9] += 1;
    }
#pragma unroll
    for (int j = 0; j < 11; j++) {
        const long long v = plane_wave_sum(s[j]);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&acc[j], (unsigned long long)v);
    }
    __syncthreads();
    if (threadIdx.x < 11 && acc[threadIdx.x]) {
        unsigned long long *dst = threadIdx.x < 9 ? (unsigned long long *)&ctl->S[threadIdx.x] : (threadIdx.x == 9 ? &ctl->m_r : &ctl->n_oor);
        atomicAdd(dst, acc[threadIdx.x]);
    }
}

__global__ __launch_bounds__(64) void k_plane_solve(PlaneCtl *__restrict__ ctl, float qscale)
{
    if (threadIdx.x != 0 || !ctl->found || ctl->m_r < 3ull) return;
    const double mr = (double)ctl->m_r;
    double n0, n1, n2, l0, l1, l2, lmin;
    if (!cov_normal(ctl->S[0], ctl->S[1], ctl->S[2], ctl->S[3], ctl->S[4], ctl->S[5], ctl->S[6], ctl->S[7], ctl->S[8], mr, n0, n1, n2, l0,
                    l1, l2, lmin))
        return;
    const double qs = (double)qscale;
    const double g0 = (double)ctl->anchor[0] + ((double)ctl->S[0] / mr) / qs, g1 = (double)ctl->anchor[1] + ((double)ctl->S[1] / mr) / qs,
                 g2 = (double)ctl->anchor[2] + ((double)ctl->S[2] / mr) / qs;
    const double d = -((n0 * g0 + n1 * g1) + n2 * g2);
    const float4 h = plane_round(n0, n1, n2, d);
    ctl->model[0] = h.x, ctl->model[1] = h.y, ctl->model[2] = h.z, ctl->model[3] = h.w;
    ctl->refined = 1u;
}

// step 8.  src: the call's control block, whose model and `found` hold (sgm_segment_plane), or null for the caller's model
__global__ __launch_bounds__(256) void k_plane_classify(const float *__restrict__ xyz, const float *__restrict__ disp, int64_t n,
                                                        float4 model, const PlaneCtl *__restrict__ src, float t, int select,
                                                        uint8_t *__restrict__ out_inlier, float *__restrict__ out_distance,
                                                        uint8_t *__restrict__ keep, uint32_t *__restrict__ n_inliers)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool found = true;
    float4 h = model;
    if (src) {
        found = src->found != 0u;
        h = make_float4(src->model[0], src->model[1], src->model[2], src->model[3]);
    }
    bool inl = false;
    if (i < n) {
        const bool valid = plane_valid(xyz, disp, i);
        float s = __uint_as_float(PLANE_QNAN);
        if (valid && found) {
            s = plane_dist(h, xyz[i * 3], xyz[i * 3 + 1], xyz[i * 3 + 2]);
            inl = fabsf(s) <= t;
        }
        if (out_inlier) out_inlier[i] = inl ? 1 : 0;
        if (out_distance) out_distance[i] = s;
        keep[i] = (select ? valid && !inl : inl) ? 1 : 0;
    }
    const uint32_t ni = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(inl));
    __shared__ uint32_t wsum[4];
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = ni;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t tot = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        if (tot) atomicAdd(n_inliers, tot);
    }
}

}  // namespace sgm
