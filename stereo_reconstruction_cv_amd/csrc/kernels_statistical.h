// kernels_statistical.h -- statistical outlier removal (include/sgm_hip_statistical.h: sgm_statistical_outlier): per point the
// mean distance to its k nearest other points within max_radius, the integer statistic of these means over the cloud, and the
// points at or under the threshold the host forms from it.  The grid of cells is that of kernels_radius.h, built by the same
// kernels (count, clear, insert, starts, sort); the header's definition is the contract.
//
//   k_stat_query<CAP> THE HOT KERNEL.  One lane per point in the order of the sorted records, over its 27 cells by rad_walk
//                     (kernels_radius.h) -- nothing ends a point's search early --, and the visitor keeps the k smallest d2 the
//                     lane has seen.  Non-negative binary32 values order as their bit patterns, so the list is one of unsigned words, ascending, in CAP registers
//                     (CAP = 8, 16, 32, 64: the smallest that holds k): the first CAP - k words are 0 for good and pass every
//                     candidate on, the last k start at STAT_FAR, and a candidate goes in by CAP fully unrolled compare-exchanges
//                     (min stays, max moves on; the largest falls off the end).  Every index is a constant: the list never
//                     leaves the registers (a list indexed at run time would live in scratch memory).  A candidate that is not
//                     below the list's last word -- the k-th smallest so far -- skips the insertion, and a wave none of whose
//                     lanes inserts branches over it.  Then steps 6 and 7: the square roots summed in ascending order, the mean,
//                     q.  Writes mean_i (or -1) to the source index and q_i (or STAT_SPARSE) over the point's rank word, which
//                     nobody needs after k_radius_sort.
//   k_stat_reduce     m, A and B over the dense points: a ballot for m, shuffles for the two 64-bit sums, per wave; the block's
//                     four waves meet in LDS and the block adds to each word once, with an ordinary 64-bit global atomicAdd at
//                     device scope.  Grid-stride over at most RAD_COUNT_BLOCKS blocks.
//   k_stat_keep       keep_i = in range and q_i <= T (STAT_SPARSE is above every T); the points that are in no cell get their
//                     mean of -1 here.  The kept points then go through k_radius_keep_count, k_compact_scan and k_radius_scatter.
// Nothing waits for anything, and every probe is bounded by the table's capacity (rad_find).  Built with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_radius.h"

namespace sgm {

constexpr int STAT_MAX_K = 64;
constexpr uint32_t STAT_FAR = 0xFFFFFFFFu;      // above the bits of every d2 <= r2 (r2 is finite)
constexpr uint32_t STAT_SPARSE = 0xFFFFFFFFu;   // in the q word: in range, fewer than k neighbours (q < 2^19 + 4, T <= 2^32 - 2)
enum { STAT_SUM_M = 0, STAT_SUM_A = 1, STAT_SUM_B = 2, STAT_SUM_WORDS = 4 };

template <int CAP>
__global__ __launch_bounds__(256) void k_stat_query(const float4 *__restrict__ sorted, uint32_t n_in, RadGrid G,
                                                    const RadSlot *__restrict__ tab, uint32_t mask, uint32_t k, float qscale,
                                                    uint32_t *__restrict__ pt_words, float *__restrict__ mean_out)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_in) return;
    const float4 me = sorted[t];
    const float x = me.x, y = me.y, z = me.z;
    const uint32_t self = __float_as_uint(me.w);
    uint32_t e[CAP];
#pragma unroll
    for (int m = 0; m < CAP; m++) e[m] = (uint32_t)m + k < (uint32_t)CAP ? 0u : STAT_FAR;
    uint32_t c = 0;
    rad_walk(sorted, tab, mask, G, x, y, z, [] { return true; }, [&](bool inside, uint32_t w, float, float, float, float d2) {
        const bool near = inside && w != self;
        c += near ? 1u : 0u;
        uint32_t v = near ? __float_as_uint(d2) : STAT_FAR;
        if (v < e[CAP - 1]) {
#pragma unroll
            for (int m = 0; m < CAP; m++) {
                const uint32_t lo = min(e[m], v);
                v = max(e[m], v);
                e[m] = lo;
            }
        }
    });
    float mean = -1.0f;
    uint32_t qi = STAT_SPARSE;
    if (c >= k) {
        float acc = 0.0f;   // (0 + s_1 is s_1)
#pragma unroll
        for (int m = 0; m < CAP; m++) {
            const float s = sqrtf(__uint_as_float(e[m]));
            acc = (uint32_t)m + k < (uint32_t)CAP ? acc : acc + s;
        }
        mean = acc / (float)k;
        qi = (uint32_t)(mean * qscale);
    }
    pt_words[2 * (size_t)self + 1] = qi;
    if (mean_out) mean_out[self] = mean;
}

__global__ __launch_bounds__(256) void k_stat_reduce(const uint2 *__restrict__ pt, int64_t n, unsigned long long *__restrict__ sums)
{
    const int64_t nblk = (n + 255) / 256;
    unsigned long long a = 0, b = 0;
    uint32_t m = 0;   // (meaningful in lane 0 of each wave)
    for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const int64_t i = blk * 256 + threadIdx.x;
        const uint2 sr = i < n ? pt[i] : make_uint2(VOX_NONE, 0u);
        const bool dense = sr.x != VOX_NONE && sr.y != STAT_SPARSE;
        m += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(dense));
        const unsigned long long q = dense ? sr.y : 0u;
        a += q;
        b += q * q;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        a += __shfl_down(a, d);
        b += __shfl_down(b, d);
    }
    __shared__ unsigned long long wsum[4][3];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
        wsum[w][STAT_SUM_M] = m;
        wsum[w][STAT_SUM_A] = a;
        wsum[w][STAT_SUM_B] = b;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const unsigned long long s = wsum[0][threadIdx.x] + wsum[1][threadIdx.x] + wsum[2][threadIdx.x] + wsum[3][threadIdx.x];
        if (s) atomicAdd(&sums[threadIdx.x], s);
    }
}

__global__ __launch_bounds__(256) void k_stat_keep(const uint2 *__restrict__ pt, int64_t n, uint32_t T, uint8_t *__restrict__ keep,
                                                   float *__restrict__ mean_out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint2 sr = pt[i];
    const bool in = sr.x != VOX_NONE;
    keep[i] = in && sr.y <= T ? 1 : 0;
    if (mean_out && !in) mean_out[i] = -1.0f;
}

}  // namespace sgm
