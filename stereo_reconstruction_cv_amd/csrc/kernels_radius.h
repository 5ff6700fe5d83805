// kernels_radius.h -- radius outlier removal (include/sgm_hip_radius.h: sgm_radius_outlier): per point the number of other points
// within r, through a uniform grid of cells of edge r * 1.03125 held in a hash table.  The header's lemma is what makes 27 cells
// enough; its definition is the contract.  Every result is an integer count, so the order in which the atomics arrive shows
// neither in the counts nor in what is kept (it does show in the order of the cells and of the points inside a cell, which
// nothing reads out).
//
//   k_radius_count    how many points are valid and in range, and how many valid but out of range: the first sizes the table
//   k_radius_clear    every slot: key EMPTY, count 0, start 0.  The table never depends on what it held.
//   k_radius_insert   one lane per point: find or claim the cell's slot (the shape of vox_find_or_claim on 16-byte slots: atomicCAS
//                     on the 64-bit key, linear probing, at most `capacity` probes, no waiting), then atomicAdd 1 on the slot's
//                     count, whose old value is the point's rank in its cell.  Slot and rank go to a per-point pair of words.
//   k_radius_starts   one lane per four slots: the block's occupied slots take a contiguous stretch of the sorted array with one
//                     atomicAdd of their total on a cursor; the order of the cells is that of the arrivals and is free.
//   k_radius_sort     one lane per point: its record (x, y, z, source index: 16 bytes) goes to start + rank; points that are in
//                     no cell get count 0 and keep 0 here.
//   k_radius_query    THE HOT KERNEL.  One lane per point in sorted order (SORTED = true, the default: the lanes of a wave are
//                     neighbours in one or two cells and share most of their 27 cells, so the slot loads and the run loads of a wave
//                     are mostly one address) or in source order (false: behind SGM_DBG_RADIUS_SOURCE_ORDER).  The walk over the
//                     27 cells is rad_walk below, which every search on this grid shares; the count lives in a register and the
//                     lane stops once it has reached max_count, which is what bounds the work in a dense cloud.
//   k_radius_keep_count / k_radius_scatter   the ordered compaction of kernels_post.h (count -> k_compact_scan -> scatter) with
//                     the predicate keep[i]; the scatter also writes the source index.
// All atomics are the ordinary vector global atomics atomicAdd / atomicCAS / atomicOr compile to, at device scope; no lane waits
// for another.  The library is compiled with -ffp-contract=off (Makefile): step 4 of the definition must not fuse.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_voxel.h"   // vox_hash, VOX_EMPTY, VOX_NONE

namespace sgm {

constexpr int RAD_GBIAS = 1 << 16;                 // cell indices -2^16 .. 2^16 - 1, biased into 17 bits
constexpr int64_t RAD_MAX_POINTS = (1ll << 24) - 1;
constexpr int RAD_COUNT_BLOCKS = 1024;             // k_radius_count: grid-stride, two global atomics per block
constexpr int RAD_STARTS_PER_BLOCK = 1024;         // k_radius_starts: four slots per lane
constexpr int RAD_RUN_LOADS = 4;                   // k_radius_query: records of a run loaded per step

// One slot: 16 bytes.  A key has 51 bits, so none equals VOX_EMPTY.
struct __align__(16) RadSlot {
    unsigned long long key;
    uint32_t count;   // points of the cell (n <= 2^24 - 1)
    uint32_t start;   // where the cell's run begins in the sorted records
};
static_assert(sizeof(RadSlot) == 16, "k_radius_clear and the query's probe move a slot as one 16-byte word");

struct RadGrid {
    float inv, r2, ox, oy, oz;
};

// control words of one call: [0] points in range, [1] valid points out of range, [2] a point found no slot, [3] the cursor of
// k_radius_starts
enum { RAD_CTL_IN = 0, RAD_CTL_OUT = 1, RAD_CTL_ERR = 2, RAD_CTL_CURSOR = 3, RAD_CTL_WORDS = 4 };

// step 3 for one axis: false if the index leaves the range
__device__ __forceinline__ bool radius_axis(float p, float o, float inv, uint32_t &gb)
{
    const float g = floorf((p - o) * inv);
    if (!(g >= -65536.0f && g < 65536.0f)) return false;
    gb = (uint32_t)((int)g + RAD_GBIAS);
    return true;
}

__device__ __forceinline__ unsigned long long radius_key(uint32_t gx, uint32_t gy, uint32_t gz)
{
    return (unsigned long long)gx << 34 | (unsigned long long)gy << 17 | gz;
}

// 0: not valid, 1: valid and in range (g is set), 2: valid, out of range
__device__ __forceinline__ int radius_classify(const float *__restrict__ xyz, const float *__restrict__ disp, int64_t i, const RadGrid &G,
                                               uint32_t g[3])
{
    const float X = xyz[i * 3], Y = xyz[i * 3 + 1], Z = xyz[i * 3 + 2];
    if (!(isfinite(X) && isfinite(Y) && isfinite(Z))) return 0;
    if (disp && !(disp[i] > 0.0f)) return 0;
    if (!radius_axis(X, G.ox, G.inv, g[0]) || !radius_axis(Y, G.oy, G.inv, g[1]) || !radius_axis(Z, G.oz, G.inv, g[2])) return 2;
    return 1;
}

__global__ __launch_bounds__(256) void k_radius_count(const float *__restrict__ xyz, const float *__restrict__ disp, int64_t n, RadGrid G,
                                                      uint32_t *__restrict__ ctl)
{
    __shared__ uint32_t tot[2];
    if (threadIdx.x < 2) tot[threadIdx.x] = 0;
    __syncthreads();
    const int64_t m = (n + 255) / 256;
    uint32_t nin = 0, nout = 0;   // (meaningful in lane 0 of each wave)
    for (int64_t b = blockIdx.x; b < m; b += gridDim.x) {
        const int64_t i = b * 256 + threadIdx.x;
        uint32_t g[3];
        const int cls = i < n ? radius_classify(xyz, disp, i, G, g) : 0;
        nin += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(cls == 1));
        nout += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(cls == 2));
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&tot[0], nin);
        atomicAdd(&tot[1], nout);
    }
    __syncthreads();
    if (threadIdx.x < 2 && tot[threadIdx.x]) atomicAdd(&ctl[threadIdx.x], tot[threadIdx.x]);
}

__global__ __launch_bounds__(256) void k_radius_clear(RadSlot *__restrict__ tab, uint32_t cap)
{
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s < cap) *(uint4 *)(tab + s) = make_uint4(~0u, ~0u, 0u, 0u);
}

// vox_find_or_claim on this table's slots: every slot is looked at once at most (mask + 1 probes), and no probe waits for
// anything -- a slot is EMPTY, ours, or somebody else's for good.  VOX_NONE if the table is full of other keys.
__device__ __forceinline__ uint32_t rad_find_or_claim(RadSlot *tab, uint32_t mask, unsigned long long key)
{
    uint32_t s = vox_hash(key) & mask;
    for (uint32_t probe = 0; probe <= mask; probe++, s = (s + 1) & mask) {
        unsigned long long *const kp = &tab[s].key;
        unsigned long long cur = __hip_atomic_load(kp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == VOX_EMPTY) {
            cur = atomicCAS(kp, VOX_EMPTY, key);
            if (cur == VOX_EMPTY) return s;
        }
        if (cur == key) return s;
    }
    return VOX_NONE;
}

// the read-only form for the query, on a table nobody writes any more: the slot that holds `key`, or VOX_NONE -- at the first
// EMPTY slot, or after mask + 1 probes in a table without one
__device__ __forceinline__ uint32_t rad_find(const RadSlot *__restrict__ tab, uint32_t mask, unsigned long long key, uint32_t &count,
                                             uint32_t &start)
{
    uint32_t s = vox_hash(key) & mask;
    for (uint32_t probe = 0; probe <= mask; probe++, s = (s + 1) & mask) {
        const uint4 w = *(const uint4 *)(tab + s);
        const unsigned long long cur = (unsigned long long)w.y << 32 | w.x;
        if (cur == key) {
            count = w.z;
            start = w.w;
            return s;
        }
        if (cur == VOX_EMPTY) break;
    }
    return VOX_NONE;
}

// THE WALK of every search on this grid (k_radius_query, k_stat_query, k_cov_query, k_dbscan_link), and the one place where its
// shape is decided.  The own cell of (x, y, z) by the arithmetic that put the point there (an in-range point: the
// three calls succeed), then the 27 cells around it, one after the other: a read-only probe, then the cell's run, RAD_RUN_LOADS
// records at a time -- the loads of one step do not depend on each other, so a lane waits for memory once per step and not once
// per record; the indices past the run's end are clamped to its last record and come with inside = false.  (Nine first probes in
// flight per plane of cells were measured and lost.)  go() is asked before every cell and before every step, so a search that
// stops early passes that by less than RAD_RUN_LOADS candidates.  visit(inside, w, dx, dy, dz, d2) gets every candidate in the
// order of the cells and of the runs: inside = a record of the run within r2 (the point itself among them: leaving it out is the
// visitor's), w its index word.  The walk never returns from the kernel: a lane whose go() is false from the start walks nothing
// and is still there afterwards (k_cov_query ends wave-wide).
template <class Go, class Visit>
__device__ __forceinline__ void rad_walk(const float4 *__restrict__ sorted, const RadSlot *__restrict__ tab, uint32_t mask, const RadGrid &G,
                                         float x, float y, float z, Go go, Visit visit)
{
    uint32_t gx = 0, gy = 0, gz = 0;
    radius_axis(x, G.ox, G.inv, gx);
    radius_axis(y, G.oy, G.inv, gy);
    radius_axis(z, G.oz, G.inv, gz);
    for (int k = 0; k < 27 && go(); k++) {
        const uint32_t nx = gx + (uint32_t)(k / 9) - 1u, ny = gy + (uint32_t)(k / 3 % 3) - 1u, nz = gz + (uint32_t)(k % 3) - 1u;
        if (nx >= 2u * RAD_GBIAS || ny >= 2u * RAD_GBIAS || nz >= 2u * RAD_GBIAS) continue;   // (0 - 1 wraps to a large number)
        uint32_t cnt = 0, start = 0;
        if (rad_find(tab, mask, radius_key(nx, ny, nz), cnt, start) == VOX_NONE || !cnt) continue;
        const uint32_t end = start + cnt;
        for (uint32_t j = start; j < end && go(); j += RAD_RUN_LOADS) {
            float4 q[RAD_RUN_LOADS];
#pragma unroll
            for (int u = 0; u < RAD_RUN_LOADS; u++) q[u] = sorted[min(j + (uint32_t)u, end - 1u)];
#pragma unroll
            for (int u = 0; u < RAD_RUN_LOADS; u++) {
                const float dx = q[u].x - x, dy = q[u].y - y, dz = q[u].z - z;
                const float d2 = (dx * dx + dy * dy) + dz * dz;
                visit(j + (uint32_t)u < end && d2 <= G.r2, __float_as_uint(q[u].w), dx, dy, dz, d2);
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_radius_insert(const float *__restrict__ xyz, const float *__restrict__ disp, int64_t n, RadGrid G,
                                                       RadSlot *tab, uint32_t mask, uint2 *__restrict__ slot_rank, uint32_t *ctl)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t g[3];
    uint2 sr = make_uint2(VOX_NONE, 0u);
    if (radius_classify(xyz, disp, i, G, g) == 1) {
        const uint32_t s = rad_find_or_claim(tab, mask, radius_key(g[0], g[1], g[2]));
        if (s == VOX_NONE) atomicOr(&ctl[RAD_CTL_ERR], 1u);
        else sr = make_uint2(s, atomicAdd(&tab[s].count, 1u));
    }
    slot_rank[i] = sr;
}

__global__ __launch_bounds__(256) void k_radius_starts(RadSlot *__restrict__ tab, uint32_t cap, uint32_t *ctl)
{
    const uint32_t s0 = (blockIdx.x * 256u + threadIdx.x) * 4u;
    uint32_t c[4], sum = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        c[k] = s0 + k < cap ? tab[s0 + k].count : 0u;
        sum += c[k];
    }
    // exclusive scan of `sum` over the block: inside the wave by shuffles, across the four waves through LDS
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t inc = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(inc, d);
        if (lane >= d) inc += t;
    }
    __shared__ uint32_t wsum[4], base;
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        base = total ? atomicAdd(&ctl[RAD_CTL_CURSOR], total) : 0u;
    }
    __syncthreads();
    uint32_t run = base + inc - sum;
    for (int k = 0; k < w; k++) run += wsum[k];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (c[k]) tab[s0 + k].start = run;
        run += c[k];
    }
}

__global__ __launch_bounds__(256) void k_radius_sort(const float *__restrict__ xyz, int64_t n, const RadSlot *__restrict__ tab,
                                                     const uint2 *__restrict__ slot_rank, float4 *__restrict__ sorted,
                                                     uint8_t *__restrict__ keep, uint32_t *__restrict__ counts)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint2 sr = slot_rank[i];
    if (sr.x == VOX_NONE) {
        keep[i] = 0;
        if (counts) counts[i] = 0u;
        return;
    }
    sorted[tab[sr.x].start + sr.y] = make_float4(xyz[i * 3], xyz[i * 3 + 1], xyz[i * 3 + 2], __uint_as_float((uint32_t)i));
}

template <bool SORTED>
__global__ __launch_bounds__(256) void k_radius_query(const float4 *__restrict__ sorted, uint32_t n_in, const float *__restrict__ xyz,
                                                      const uint2 *__restrict__ slot_rank, int64_t n, RadGrid G,
                                                      const RadSlot *__restrict__ tab, uint32_t mask, uint32_t nb_points,
                                                      uint32_t max_count, uint8_t *__restrict__ keep, uint32_t *__restrict__ counts)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    float x, y, z;
    uint32_t self;
    if (SORTED) {
        if (t >= n_in) return;
        const float4 me = sorted[t];
        x = me.x, y = me.y, z = me.z;
        self = __float_as_uint(me.w);
    } else {
        if (t >= n || slot_rank[t].x == VOX_NONE) return;
        x = xyz[t * 3], y = xyz[t * 3 + 1], z = xyz[t * 3 + 2];
        self = (uint32_t)t;
    }
    // c can pass max_count by less than RAD_RUN_LOADS, which the min below takes back
    uint32_t c = 0;
    rad_walk(sorted, tab, mask, G, x, y, z, [&] { return c < max_count; },
             [&](bool inside, uint32_t w, float, float, float, float) { c += (inside && w != self) ? 1u : 0u; });
    keep[self] = c >= nb_points ? 1 : 0;
    if (counts) counts[self] = min(c, max_count);
}

__global__ __launch_bounds__(256) void k_radius_keep_count(const uint8_t *__restrict__ keep, int64_t n, uint32_t *__restrict__ counts)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool v = i < n && keep[i];
    const unsigned long long b = __builtin_amdgcn_ballot_w64(v);
    __shared__ uint32_t wsum[4];
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = (uint32_t)__builtin_popcountll(b);
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

__global__ __launch_bounds__(256) void k_radius_scatter(const uint8_t *__restrict__ keep, const float *__restrict__ xyz,
                                                        const uint8_t *__restrict__ colors, int64_t n, const uint32_t *__restrict__ offsets,
                                                        float *__restrict__ out_xyz, uint8_t *__restrict__ out_rgb,
                                                        uint32_t *__restrict__ out_index)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool v = i < n && keep[i];
    const unsigned long long b = __builtin_amdgcn_ballot_w64(v);
    __shared__ uint32_t wsum[4];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) wsum[w] = (uint32_t)__builtin_popcountll(b);
    __syncthreads();
    uint32_t base = offsets[blockIdx.x];
    for (int k = 0; k < w; k++) base += wsum[k];
    if (v) {
        const int64_t o = base + (uint32_t)__builtin_popcountll(b & ((1ull << lane) - 1ull));
        if (out_xyz) {
            out_xyz[o * 3 + 0] = xyz[i * 3 + 0];
            out_xyz[o * 3 + 1] = xyz[i * 3 + 1];
            out_xyz[o * 3 + 2] = xyz[i * 3 + 2];
        }
        if (out_rgb) {
            out_rgb[o * 3 + 0] = colors[i * 3 + 0];
            out_rgb[o * 3 + 1] = colors[i * 3 + 1];
            out_rgb[o * 3 + 2] = colors[i * 3 + 2];
        }
        if (out_index) out_index[o] = (uint32_t)i;
    }
}

}  // namespace sgm
