// kernels_voxel.h -- voxel-grid downsampling of a point cloud (include/sgm_hip_voxel.h: sgm_voxel_downsample): one centroid, one
// mean colour and one count per occupied voxel.  Everything that is summed is an integer, so the order in which the atomics arrive
// does not show in the result; the header's definition is the contract.
//
//   k_voxel_count       how many points are valid and in range, and how many valid but out of range: the first sizes the table
//   k_voxel_clear       every slot of the table: key EMPTY, sums 0, first = 0xffffffff.  The table never depends on what it held.
//   k_voxel_insert      one lane per point: find or claim the voxel's slot (atomicCAS on the 64-bit key, linear probing, at most
//                       `capacity` probes, no waiting on another lane), then add into the slot's sums and atomicMin its `first`;
//                       the point's slot goes to a per-point word.  <PRE = true>: lanes of a wave that are neighbours and share
//                       a key (the usual case in an organised cloud) are summed in registers by a segmented scan first, and the
//                       last lane of each run issues the atomics for the run.
//   k_voxel_head_count  } the ordered compaction of kernels_post.h (count -> k_compact_scan -> scatter) with the predicate "this
//   k_voxel_scatter     } point is its voxel's first and the voxel holds min_points"; the scatter computes the output row
//                         (step 6 of the definition) from the slot.
// All atomics are the ordinary vector global atomics atomicAdd / atomicCAS / atomicMin / atomicOr compile to, at device scope.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sgm {

constexpr unsigned long long VOX_EMPTY = ~0ull;    // no key has bit 63 set
constexpr uint32_t VOX_NONE = 0xffffffffu;         // per-point word: the point is in no voxel
constexpr int VOX_GBIAS = 1 << 20;
constexpr int64_t VOX_MAX_POINTS = (1ll << 24) - 1;
constexpr unsigned long long VOX_S_MASK = (1ull << 40) - 1;
constexpr int VOX_COUNT_BLOCKS = 1024;             // k_voxel_count: grid-stride, two global atomics per block
constexpr bool VOX_PRE_DEFAULT = true;             // k_voxel_insert<PRE> the library runs (DESIGN.md 4.18 has both times); SGM_DBG_VOXEL_OTHER_REDUCTION runs the other

// One slot: 48 bytes.  Field widths for n <= VOX_MAX_POINTS: c < 2^24, S_a <= 65535 c < 2^40, C_k <= 255 c < 2^32.
struct __align__(16) VoxSlot {
    unsigned long long key;
    unsigned long long sx_c;   // S_x | c << 40
    unsigned long long sy, sz;
    unsigned long long rg;     // C_r | C_g << 32
    uint32_t b;                // C_b
    uint32_t first;
};
static_assert(sizeof(VoxSlot) == 48, "k_voxel_clear writes a slot as three 16-byte words");

struct VoxGrid {
    float inv, v, ox, oy, oz;
};

// control words of one call: [0] points in range, [1] valid points out of range, [2] a point found no slot
enum { VOX_CTL_IN = 0, VOX_CTL_OUT = 1, VOX_CTL_ERR = 2, VOX_CTL_WORDS = 4 };

// steps 1 .. 3 for one axis: false if the index leaves the range
__device__ __forceinline__ bool voxel_axis(float p, float o, float inv, uint32_t &gb, uint32_t &u)
{
    const float t = (p - o) * inv;
    const float g = floorf(t);
    if (!(g >= -1048576.0f && g < 1048576.0f)) return false;
    const float f = t - g;
    u = min((uint32_t)(f * 65536.0f), 65535u);
    gb = (uint32_t)((int)g + VOX_GBIAS);
    return true;
}

// 0: not valid, 1: valid and in range (key and u are set), 2: valid, out of range
__device__ __forceinline__ int voxel_classify(const float *__restrict__ xyz, const float *__restrict__ disp, int64_t i, const VoxGrid &G,
                                              unsigned long long &key, uint32_t u[3])
{
    const float X = xyz[i * 3], Y = xyz[i * 3 + 1], Z = xyz[i * 3 + 2];
    if (!(isfinite(X) && isfinite(Y) && isfinite(Z))) return 0;
    if (disp && !(disp[i] > 0.0f)) return 0;
    uint32_t gx, gy, gz;
    if (!voxel_axis(X, G.ox, G.inv, gx, u[0]) || !voxel_axis(Y, G.oy, G.inv, gy, u[1]) || !voxel_axis(Z, G.oz, G.inv, gz, u[2])) return 2;
    key = (unsigned long long)gx << 42 | (unsigned long long)gy << 21 | gz;
    return 1;
}

__global__ __launch_bounds__(256) void k_voxel_count(const float *__restrict__ xyz, const float *__restrict__ disp, int64_t n, VoxGrid G,
                                                     uint32_t *__restrict__ ctl)
{
    __shared__ uint32_t tot[2];
    if (threadIdx.x < 2) tot[threadIdx.x] = 0;
    __syncthreads();
    const int64_t m = (n + 255) / 256;
    uint32_t nin = 0, nout = 0;   // (meaningful in lane 0 of each wave)
    for (int64_t b = blockIdx.x; b < m; b += gridDim.x) {
        const int64_t i = b * 256 + threadIdx.x;
        unsigned long long key;
        uint32_t u[3];
        const int cls = i < n ? voxel_classify(xyz, disp, i, G, key, u) : 0;
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

__global__ __launch_bounds__(256) void k_voxel_clear(VoxSlot *__restrict__ tab, uint32_t cap)
{
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s >= cap) return;
    uint4 *const w = (uint4 *)(tab + s);
    w[0] = make_uint4(~0u, ~0u, 0u, 0u);   // key, sx_c
    w[1] = make_uint4(0u, 0u, 0u, 0u);     // sy, sz
    w[2] = make_uint4(0u, 0u, 0u, ~0u);    // rg, b, first
}

__device__ __forceinline__ uint32_t vox_hash(unsigned long long k)
{
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return (uint32_t)k;
}

// The slot that holds `key`, claimed if nobody had: every slot is looked at once at most (mask + 1 probes), and no probe waits
// for anything -- a slot is EMPTY, ours, or somebody else's for good.  VOX_NONE if the table is full of other keys.
__device__ __forceinline__ uint32_t vox_find_or_claim(VoxSlot *tab, uint32_t mask, unsigned long long key)
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

template <bool PRE>
__global__ __launch_bounds__(256) void k_voxel_insert(const float *__restrict__ xyz, const float *__restrict__ disp,
                                                      const uint8_t *__restrict__ colors, int64_t n, VoxGrid G, VoxSlot *tab, uint32_t mask,
                                                      uint32_t *__restrict__ slot_of, uint32_t *ctl)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long key = VOX_EMPTY;
    uint32_t u[3] = {0, 0, 0};
    const bool in = i < n && voxel_classify(xyz, disp, i, G, key, u) == 1;
    if (!in) key = VOX_EMPTY;
    uint32_t cr = 0, cg = 0, cb = 0;
    if (in && colors) {
        cr = colors[i * 3];
        cg = colors[i * 3 + 1];
        cb = colors[i * 3 + 2];
    }
    // what this lane adds, in the fields of one wave's partial sums: c <= 64 above S_x <= 64 * 65535 < 2^22; C_r, C_g < 2^14 each
    uint32_t a0 = in ? (1u << 22 | u[0]) : 0u, a1 = u[1], a2 = u[2], a3 = cr | cg << 16, a4 = cb;
    uint32_t first = (uint32_t)i;
    bool issue = in;
    int tail = 0;
    if (PRE) {
        // runs of neighbouring lanes with one key; lanes that are in no voxel carry EMPTY and form runs that issue nothing
        const int lane = threadIdx.x & 63;
        const unsigned long long prev = __shfl_up(key, 1);
        const unsigned long long starts = __builtin_amdgcn_ballot_w64(lane == 0 || prev != key);
        const int head = 63 - __builtin_clzll(starts & (~0ull >> (63 - lane)));
        const unsigned long long above = lane == 63 ? 0ull : starts >> (lane + 1);
        tail = above ? lane + __builtin_ctzll(above) : 63;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {   // segmented inclusive scan: the last lane of a run ends with the run's sums
            const uint32_t t0 = __shfl_up(a0, d), t1 = __shfl_up(a1, d), t2 = __shfl_up(a2, d), t3 = __shfl_up(a3, d), t4 = __shfl_up(a4, d);
            if (lane - d >= head) {
                a0 += t0;
                a1 += t1;
                a2 += t2;
                a3 += t3;
                a4 += t4;
            }
        }
        first = (uint32_t)(i - (lane - head));
        issue = in && lane == tail;
    }
    uint32_t s = VOX_NONE;
    if (issue) {
        s = vox_find_or_claim(tab, mask, key);
        if (s == VOX_NONE) {
            atomicOr(&ctl[VOX_CTL_ERR], 1u);
        } else {
            VoxSlot *const t = tab + s;
            atomicAdd(&t->sx_c, (unsigned long long)(a0 & 0x3fffffu) | (unsigned long long)(a0 >> 22) << 40);
            atomicAdd(&t->sy, (unsigned long long)a1);
            atomicAdd(&t->sz, (unsigned long long)a2);
            if (colors) {
                atomicAdd(&t->rg, (unsigned long long)(a3 & 0xffffu) | (unsigned long long)(a3 >> 16) << 32);
                atomicAdd(&t->b, a4);
            }
            atomicMin(&t->first, first);
        }
    }
    if (PRE) s = __shfl(s, tail);   // (a run of EMPTY lanes gets its tail's VOX_NONE)
    if (i < n) slot_of[i] = s;
}

// point i is the head of a kept voxel: in a voxel, that voxel's first point, and the voxel holds min_points
__device__ __forceinline__ bool vox_is_head(const uint32_t *__restrict__ slot_of, const VoxSlot *__restrict__ tab, int64_t i, int64_t n,
                                            uint32_t min_points, uint32_t &s)
{
    if (i >= n) return false;
    s = slot_of[i];
    if (s == VOX_NONE) return false;
    return tab[s].first == (uint32_t)i && (uint32_t)(tab[s].sx_c >> 40) >= min_points;
}

__global__ __launch_bounds__(256) void k_voxel_head_count(const uint32_t *__restrict__ slot_of, const VoxSlot *__restrict__ tab, int64_t n,
                                                          uint32_t min_points, uint32_t *__restrict__ counts)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t s;
    const bool v = vox_is_head(slot_of, tab, i, n, min_points, s);
    const unsigned long long b = __builtin_amdgcn_ballot_w64(v);
    __shared__ uint32_t wsum[4];
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = (uint32_t)__builtin_popcountll(b);
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// step 6 for one axis: the sum S over c points in the voxel with biased index gb
__device__ __forceinline__ float vox_centroid(unsigned long long S, unsigned long long c, uint32_t gb, float v, float o)
{
    const uint32_t M = (uint32_t)((2 * S + c) / (2 * c));
    const float m = (float)M * (1.0f / 65536.0f);
    return ((float)((int)gb - VOX_GBIAS) + m) * v + o;
}

__global__ __launch_bounds__(256) void k_voxel_scatter(const uint32_t *__restrict__ slot_of, const VoxSlot *__restrict__ tab, int64_t n,
                                                       uint32_t min_points, const uint32_t *__restrict__ offsets, VoxGrid G,
                                                       float *__restrict__ out_xyz, uint8_t *__restrict__ out_rgb,
                                                       uint32_t *__restrict__ out_cnt)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t s = VOX_NONE;
    const bool v = vox_is_head(slot_of, tab, i, n, min_points, s);
    const unsigned long long b = __builtin_amdgcn_ballot_w64(v);
    __shared__ uint32_t wsum[4];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) wsum[w] = (uint32_t)__builtin_popcountll(b);
    __syncthreads();
    uint32_t base = offsets[blockIdx.x];
    for (int k = 0; k < w; k++) base += wsum[k];
    if (v) {
        const int64_t o = base + (uint32_t)__builtin_popcountll(b & ((1ull << lane) - 1ull));
        const VoxSlot t = tab[s];
        const unsigned long long c = t.sx_c >> 40;
        out_xyz[o * 3 + 0] = vox_centroid(t.sx_c & VOX_S_MASK, c, (uint32_t)(t.key >> 42) & 0x1fffffu, G.v, G.ox);
        out_xyz[o * 3 + 1] = vox_centroid(t.sy, c, (uint32_t)(t.key >> 21) & 0x1fffffu, G.v, G.oy);
        out_xyz[o * 3 + 2] = vox_centroid(t.sz, c, (uint32_t)t.key & 0x1fffffu, G.v, G.oz);
        if (out_rgb) {
            out_rgb[o * 3 + 0] = (uint8_t)((2 * (t.rg & 0xffffffffull) + c) / (2 * c));
            out_rgb[o * 3 + 1] = (uint8_t)((2 * (t.rg >> 32) + c) / (2 * c));
            out_rgb[o * 3 + 2] = (uint8_t)((2 * (unsigned long long)t.b + c) / (2 * c));
        }
        if (out_cnt) out_cnt[o] = (uint32_t)c;
    }
}

}  // namespace sgm
