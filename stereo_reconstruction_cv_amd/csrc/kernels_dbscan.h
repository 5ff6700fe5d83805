// kernels_dbscan.h -- density clustering (include/sgm_hip_dbscan.h: sgm_cluster_dbscan) on the grid of cells of kernels_radius.h:
// the table, the ranks, the starts and the records sorted by cell are radius_build_grid's, and the core predicate is
// k_radius_query<true> with nb_points = max_count = min_points, both unchanged.  The header's definition is the contract.  What is
// new here:
//
//   k_dbscan_mark     one lane per sorted record: the link of its point set to identity, its nearest core point to none, and
//                     (MARK = true, the default) the core bit of its point copied into bit 31 of the record's index word, so that
//                     the link kernel reads it with the run.  A kernel of its own: no lane of it reads another lane's word.
//                     MARK = false (SGM_DBG_DBSCAN_GATHER_CORE) leaves the records alone; the link kernel then gathers
//                     core[source index] per candidate.
//   k_dbscan_link     THE HOT KERNEL.  One lane per point in sorted order over its 27 cells by rad_walk (kernels_radius.h), and
//                     nothing stops it early.  The visitor: a core lane unites itself (uf_union of kernels_post.h,
//                     on links indexed by source index) with every core candidate within r2 whose source index is smaller than its
//                     own -- every linked pair is met twice and handled once --, after a look at the two current links, which
//                     are equal for most pairs once a neighbourhood has grown together.  A lane that is not core keeps the
//                     minimum of (d2 bits << 32 | source index) over its core candidates in a register pair and stores the
//                     index, or none.
//   k_dbscan_roots    one lane per point in source order: the roots -- core points whose link is themselves -- counted per block;
//   k_compact_scan    (kernels_post.h, unchanged) the blocks' offsets and the number of clusters;
//   k_dbscan_rank     each root's rank among the roots in source order, which is the cluster's number: after the unions the root
//                     of a component is its smallest index (a union links the larger root to the smaller one), the header's
//                     representative.  The same lanes zero the rows of the sizes that will be written.
//   k_dbscan_label    one lane per point: rank[find(core ? i : nearest core)] or -1; the sizes by one integer atomicAdd per
//                     distinct label of a wave; the three statistics by ballots and one atomicAdd per block.
//
// The links only ever decrease (atomicMin), every loop of uf_find / uf_union ends because a value strictly fell, and no lane waits
// for another: no spin on a flag, no cooperative launch, no grid barrier.  All atomics are the ordinary vector global atomics at
// agent scope.  The partition is a function of the set of linked pairs, and rank, label, size and statistics are integers derived
// from it: the order in which the atomics arrive shows nowhere.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_post.h"     // uf_load, uf_find, uf_union
#include "kernels_radius.h"

namespace sgm {

constexpr uint32_t DB_CORE_BIT = 0x80000000u;   // bit 31 of a sorted record's index word (an index has 24 bits)
constexpr uint32_t DB_INDEX_MASK = 0x00FFFFFFu;
constexpr uint32_t DB_NONE = 0xFFFFFFFFu;       // no core point within r2

// control words of one call, beside those of the radius search: core, border and in-range noise points
enum { DB_CTL_CORE = 0, DB_CTL_BORDER = 1, DB_CTL_NOISE = 2, DB_CTL_WORDS = 4 };

template <bool MARK>
__global__ __launch_bounds__(256) void k_dbscan_mark(float4 *__restrict__ sorted, uint32_t n_in, const uint8_t *__restrict__ core,
                                                     int *__restrict__ parent, uint32_t *__restrict__ nearest)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n_in) return;
    uint32_t *const word = (uint32_t *)(sorted + t) + 3;
    const uint32_t self = *word & DB_INDEX_MASK;
    parent[self] = (int)self;
    nearest[self] = DB_NONE;
    if (MARK && core[self]) *word = self | DB_CORE_BIT;
}

template <bool GATHER>
__global__ __launch_bounds__(256) void k_dbscan_link(const float4 *__restrict__ sorted, uint32_t n_in, RadGrid G,
                                                     const RadSlot *__restrict__ tab, uint32_t mask, const uint8_t *__restrict__ core,
                                                     int *parent, uint32_t *__restrict__ nearest)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n_in) return;
    const float4 me = sorted[t];
    const float x = me.x, y = me.y, z = me.z;
    const uint32_t mw = __float_as_uint(me.w), self = mw & DB_INDEX_MASK;
    const bool me_core = GATHER ? core[self] != 0 : (mw & DB_CORE_BIT) != 0;
    unsigned long long best = ~0ull;
    rad_walk(sorted, tab, mask, G, x, y, z, [] { return true; }, [&](bool inside, uint32_t w, float, float, float, float d2) {
        const uint32_t other = w & DB_INDEX_MASK;
        if (!(inside && (GATHER ? core[other] != 0 : (w & DB_CORE_BIT) != 0))) return;
        if (me_core) {
            // each linked pair once, from its larger index; equal links: the two are in one tree already
            if (other < self && uf_load(parent, (int)self) != uf_load(parent, (int)other)) uf_union(parent, (int)self, (int)other);
        } else {
            const unsigned long long key = (unsigned long long)__float_as_uint(d2) << 32 | other;   // d2 >= 0: its bits order as its value
            best = key < best ? key : best;
        }
    });
    if (!me_core && best != ~0ull) nearest[self] = (uint32_t)best;
}

// a root: a core point that is its own link once every union has been made
__device__ __forceinline__ bool dbscan_is_root(const uint8_t *__restrict__ core, const int *__restrict__ parent, int64_t i, int64_t n)
{
    return i < n && core[i] && parent[i] == (int)i;
}

__global__ __launch_bounds__(256) void k_dbscan_roots(const uint8_t *__restrict__ core, const int *__restrict__ parent, int64_t n,
                                                      uint32_t *__restrict__ counts)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const unsigned long long b = __builtin_amdgcn_ballot_w64(dbscan_is_root(core, parent, i, n));
    __shared__ uint32_t wsum[4];
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = (uint32_t)__builtin_popcountll(b);
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// offsets: the blocks' exclusive offsets, offsets[m] the number of clusters
__global__ __launch_bounds__(256) void k_dbscan_rank(const uint8_t *__restrict__ core, const int *__restrict__ parent, int64_t n,
                                                     const uint32_t *__restrict__ offsets, int m, uint32_t *__restrict__ rank,
                                                     uint32_t *__restrict__ sizes)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool v = dbscan_is_root(core, parent, i, n);
    const unsigned long long b = __builtin_amdgcn_ballot_w64(v);
    __shared__ uint32_t wsum[4];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) wsum[w] = (uint32_t)__builtin_popcountll(b);
    __syncthreads();
    uint32_t base = offsets[blockIdx.x];
    for (int k = 0; k < w; k++) base += wsum[k];
    if (v) rank[i] = base + (uint32_t)__builtin_popcountll(b & ((1ull << lane) - 1ull));
    if (sizes && i < (int64_t)offsets[m]) sizes[i] = 0u;   // (clusters <= points: the lanes suffice; the rows past the clusters stay)
}

__global__ __launch_bounds__(256) void k_dbscan_label(const uint2 *__restrict__ slot_rank, const uint8_t *__restrict__ core, int *parent,
                                                      const uint32_t *__restrict__ nearest, const uint32_t *__restrict__ rank, int64_t n,
                                                      int *__restrict__ labels, uint32_t *sizes, uint32_t *ctl)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int label = -1;
    bool is_core = false, in_range = false;
    if (i < n && slot_rank[i].x != VOX_NONE) {
        in_range = true;
        is_core = core[i] != 0;
        const uint32_t from = is_core ? (uint32_t)i : nearest[i];
        if (from != DB_NONE) label = (int)rank[uf_find(parent, (int)from)];
    }
    if (i < n && labels) labels[i] = label;
    if (sizes) {   // one add per distinct label of the wave: neighbours in source order mostly share theirs
        unsigned long long todo = __builtin_amdgcn_ballot_w64(label >= 0);
        while (todo) {
            const int lead = __builtin_amdgcn_readlane(label, (int)__builtin_ctzll(todo));
            const unsigned long long mine = __builtin_amdgcn_ballot_w64(label == lead);
            if ((threadIdx.x & 63) == (unsigned)__builtin_ctzll(mine)) atomicAdd(&sizes[lead], (uint32_t)__builtin_popcountll(mine));
            todo &= ~mine;
        }
    }
    const unsigned long long bc = __builtin_amdgcn_ballot_w64(is_core), bb = __builtin_amdgcn_ballot_w64(in_range && !is_core && label >= 0),
                             bn = __builtin_amdgcn_ballot_w64(in_range && label < 0);
    __shared__ uint32_t tot[3];
    if (threadIdx.x < 3) tot[threadIdx.x] = 0;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&tot[0], (uint32_t)__builtin_popcountll(bc));
        atomicAdd(&tot[1], (uint32_t)__builtin_popcountll(bb));
        atomicAdd(&tot[2], (uint32_t)__builtin_popcountll(bn));
    }
    __syncthreads();
    if (threadIdx.x < 3 && tot[threadIdx.x]) atomicAdd(&ctl[threadIdx.x], tot[threadIdx.x]);
}

}  // namespace sgm
