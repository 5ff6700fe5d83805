// kernels_mesh.h -- a triangle mesh from the organised cloud (include/sgm_hip_mesh.h: sgm_mesh_grid): two triangles per pixel quad
// wherever the disparity is continuous, as vertices in row-major pixel order and faces in row-major quad order.  The header's
// definition is the contract.  Everything is a pure function of the inputs: no atomics, and the order comes from the ordered
// compaction of kernels_post.h done twice -- per-block counts, k_compact_scan (unchanged), scatter by ballot + popcount -- once
// over the pixels that are vertices and once over the quads' triangles.
//
// The pixels are walked in row-major order in blocks of MESH_BLOCK = 1024; pixel i stands for itself and for the quad whose corner
// a it is, so quad order and pixel order are the same walk.  (1024, not the compaction's 256: k_compact_scan is one workgroup
// whose time goes with the number of counts, and at 256 the two scans were 29 % of a 4K call -- DESIGN.md 4.19.)
//
//   k_mesh_quads     per quad one code byte (the chosen diagonal, which of its two triangles are emitted, which corners they name;
//                    0 for the pixels of the last row and column, which head no quad) and the block's number of triangles.
//                    256 lanes, four neighbouring pixels each: a lane reads its four pixels and the four below them -- <WIDE>: as
//                    16-byte loads, three for the 12 floats of xyz and one for the disparities, which needs 16-byte aligned
//                    images and W % 4 == 0; otherwise float by float -- and the fifth pair from the next lane by a shuffle (lane
//                    63 reads it).  Every pixel is read twice, the second time from the cache.
//   k_mesh_used      the block's number of vertices: a pixel is one iff one of the (up to) four quads it is a corner of names it,
//                    four code bytes.  One lane per pixel, as in the two below.
//   k_mesh_vertices  the ordered scatter of the vertices (xyz and colour rows copied as they are) and the pixel -> vertex number
//                    map, written on used pixels only and read on used pixels only.
//   k_mesh_faces     the ordered scatter of the triangles: a lane emits 0, 1 or 2, so its place in the wave is the popcount of
//                    two ballots below it; the three corners' numbers come from the map.
// Offsets into the images and the outputs are 64-bit; H * W <= 2^26, so a pixel's number, x and y fit 32 bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sgm {

constexpr int64_t MESH_MAX_PIXELS = 1ll << 26;
constexpr int MESH_BLOCK = 1024;   // pixels per block, in all four kernels
// the code byte of a quad
enum {
    MESH_BC = 1,        // the quad takes diagonal b-c (else a-d)
    MESH_FIRST = 2,     // T0 (a-d) or T2 (b-c) is emitted
    MESH_SECOND = 4,    // T1 (a-d) or T3 (b-c) is emitted
    MESH_A = 16, MESH_B = 32, MESH_C = 64, MESH_D = 128   // an emitted triangle names this corner
};

// step 1 as one float: the pixel's disparity where the pixel is valid, NaN where it is not (a valid disparity is > 0, never NaN).
// Step 2 then needs no validity: fabsf(p - q) <= max_diff is false as soon as either side is NaN.
__device__ __forceinline__ float mesh_vdisp(float X, float Y, float Z, float d)
{
    return (isfinite(X) && isfinite(Y) && isfinite(Z) && d > 0.0f) ? d : __builtin_nanf("");
}

__device__ __forceinline__ float mesh_vdisp_at(const float *__restrict__ xyz, const float *__restrict__ disp, int64_t i, int64_t n)
{
    return i < n ? mesh_vdisp(xyz[i * 3], xyz[i * 3 + 1], xyz[i * 3 + 2], disp[i]) : __builtin_nanf("");
}

// the same for the four pixels i0 .. i0 + 3 (i0 a multiple of 4); pixels past the frame give NaN
template <bool WIDE>
__device__ __forceinline__ void mesh_vdisp4(const float *__restrict__ xyz, const float *__restrict__ disp, int64_t i0, int64_t n, float *v)
{
    if (WIDE && i0 + 3 < n) {   // 48 and 16 bytes from a 16-byte boundary
        const float4 *p = (const float4 *)(xyz + i0 * 3);
        const float4 p0 = p[0], p1 = p[1], p2 = p[2], d = *(const float4 *)(disp + i0);
        v[0] = mesh_vdisp(p0.x, p0.y, p0.z, d.x);
        v[1] = mesh_vdisp(p0.w, p1.x, p1.y, d.y);
        v[2] = mesh_vdisp(p1.z, p1.w, p2.x, d.z);
        v[3] = mesh_vdisp(p2.y, p2.z, p2.w, d.w);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = mesh_vdisp_at(xyz, disp, i0 + k, n);
    }
}

// steps 2 and 3 for one quad from its corners' mesh_vdisp
__device__ __forceinline__ uint32_t mesh_quad_code(float a, float b, float c, float d, float md)
{
    const bool va = !isnan(a), vb = !isnan(b), vc = !isnan(c), vd = !isnan(d);
    const float ad = fabsf(a - d), bc = fabsf(b - c);
    const bool cab = fabsf(a - b) <= md, cac = fabsf(a - c) <= md, cad = ad <= md;
    const bool cbc = bc <= md, cbd = fabsf(b - d) <= md, ccd = fabsf(c - d) <= md;
    if (va && vd && (!(vb && vc) || ad <= bc)) {
        const bool t0 = cac && ccd && cad, t1 = cad && cbd && cab;   // (a, c, d)  (a, d, b)
        return (t0 ? MESH_FIRST | MESH_A | MESH_C | MESH_D : 0) | (t1 ? MESH_SECOND | MESH_A | MESH_D | MESH_B : 0);
    }
    const bool t2 = cac && cbc && cab, t3 = cbc && ccd && cbd;       // (a, c, b)  (b, c, d)
    return MESH_BC | (t2 ? MESH_FIRST | MESH_A | MESH_C | MESH_B : 0) | (t3 ? MESH_SECOND | MESH_B | MESH_C | MESH_D : 0);
}

// the sum of the waves' numbers goes to counts[block]
__device__ __forceinline__ void mesh_block_count(uint32_t wave_total, uint32_t *__restrict__ counts)
{
    __shared__ uint32_t wsum[MESH_BLOCK / 64];
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = wave_total;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (int k = 0; k < (int)(blockDim.x >> 6); k++) s += wsum[k];
        counts[blockIdx.x] = s;
    }
}

template <bool WIDE>
__global__ __launch_bounds__(MESH_BLOCK / 4) void k_mesh_quads(const float *__restrict__ xyz, const float *__restrict__ disp, int H, int W,
                                                               float md, uint8_t *__restrict__ code, uint32_t *__restrict__ fcnt)
{
    const int64_t n = (int64_t)H * W;
    const int64_t i0 = ((int64_t)blockIdx.x * (MESH_BLOCK / 4) + threadIdx.x) * 4;
    float a[5], c[5];
    mesh_vdisp4<WIDE>(xyz, disp, i0, n, a);
    mesh_vdisp4<WIDE>(xyz, disp, i0 + W, n, c);
    a[4] = __shfl_down(a[0], 1);
    c[4] = __shfl_down(c[0], 1);
    if ((threadIdx.x & 63) == 63) {
        a[4] = mesh_vdisp_at(xyz, disp, i0 + 4, n);
        c[4] = mesh_vdisp_at(xyz, disp, i0 + 4 + W, n);
    }
    uint32_t x = 0, y = 0, q4 = 0, faces = 0;
    if (i0 < n) {
        x = (uint32_t)i0 % (uint32_t)W;
        y = (uint32_t)i0 / (uint32_t)W;
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        uint32_t q = 0;
        if (i0 + k < n && x + 1 < (uint32_t)W && y + 1 < (uint32_t)H) q = mesh_quad_code(a[k], a[k + 1], c[k], c[k + 1], md);
        q4 |= q << (8 * k);
        faces += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64((q & MESH_FIRST) != 0)) +
                 (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64((q & MESH_SECOND) != 0));
        if (++x == (uint32_t)W) {
            x = 0;
            y++;
        }
    }
    if (i0 + 3 < n) {
        *(uint32_t *)(code + i0) = q4;   // (the engine's own buffer: 16-byte aligned)
    } else {
        for (int k = 0; k < 4; k++)
            if (i0 + k < n) code[i0 + k] = (uint8_t)(q4 >> (8 * k));
    }
    mesh_block_count(faces, fcnt);
}

// step 4: pixel i is a vertex iff a quad it is a corner of names it -- as a of its own quad, b of the one to the left, c of the one
// above, d of the one above left.  (Pixels of the last row and column carry code 0.)
__device__ __forceinline__ bool mesh_is_vertex(const uint8_t *__restrict__ code, int64_t i, int64_t n, int W)
{
    if (i >= n) return false;
    const uint32_t x = (uint32_t)i % (uint32_t)W;
    uint32_t u = code[i] & MESH_A;
    if (x > 0) u |= code[i - 1] & MESH_B;
    if (i >= W) {
        u |= code[i - W] & MESH_C;
        if (x > 0) u |= code[i - W - 1] & MESH_D;
    }
    return u != 0;
}

__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_used(const uint8_t *__restrict__ code, int H, int W, uint32_t *__restrict__ vcnt)
{
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    const bool v = mesh_is_vertex(code, i, (int64_t)H * W, W);
    mesh_block_count((uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(v)), vcnt);
}

// what the waves of the block in front of this one hold, on top of the block's offset
__device__ __forceinline__ uint32_t mesh_wave_base(uint32_t wave_total, const uint32_t *__restrict__ offsets)
{
    __shared__ uint32_t wsum[MESH_BLOCK / 64];
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) wsum[w] = wave_total;
    __syncthreads();
    uint32_t base = offsets[blockIdx.x];
    for (int k = 0; k < w; k++) base += wsum[k];
    return base;
}

__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_vertices(const float *__restrict__ xyz, const uint8_t *__restrict__ colors,
                                                              const uint8_t *__restrict__ code, int H, int W,
                                                              const uint32_t *__restrict__ offsets, float *__restrict__ out_xyz,
                                                              uint8_t *__restrict__ out_rgb, uint32_t *__restrict__ number)
{
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    const bool v = mesh_is_vertex(code, i, (int64_t)H * W, W);
    const unsigned long long b = __builtin_amdgcn_ballot_w64(v);
    const uint32_t base = mesh_wave_base((uint32_t)__builtin_popcountll(b), offsets);
    if (v) {
        const uint32_t o = base + (uint32_t)__builtin_popcountll(b & ((1ull << (threadIdx.x & 63)) - 1ull));
        number[i] = o;
        out_xyz[(int64_t)o * 3 + 0] = xyz[i * 3 + 0];
        out_xyz[(int64_t)o * 3 + 1] = xyz[i * 3 + 1];
        out_xyz[(int64_t)o * 3 + 2] = xyz[i * 3 + 2];
        if (colors) {
            out_rgb[(int64_t)o * 3 + 0] = colors[i * 3 + 0];
            out_rgb[(int64_t)o * 3 + 1] = colors[i * 3 + 1];
            out_rgb[(int64_t)o * 3 + 2] = colors[i * 3 + 2];
        }
    }
}

__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_faces(const uint8_t *__restrict__ code, const uint32_t *__restrict__ number, int H, int W,
                                                           const uint32_t *__restrict__ offsets, int32_t *__restrict__ out_faces)
{
    const int64_t n = (int64_t)H * W;
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    const uint32_t q = i < n ? code[i] : 0u;
    const unsigned long long b1 = __builtin_amdgcn_ballot_w64((q & MESH_FIRST) != 0), b2 = __builtin_amdgcn_ballot_w64((q & MESH_SECOND) != 0);
    const uint32_t base = mesh_wave_base((uint32_t)(__builtin_popcountll(b1) + __builtin_popcountll(b2)), offsets);
    if (q & (MESH_FIRST | MESH_SECOND)) {   // (a quad: i + W + 1 < n)
        const unsigned long long below = (1ull << (threadIdx.x & 63)) - 1ull;
        int64_t o = (int64_t)base + __builtin_popcountll(b1 & below) + __builtin_popcountll(b2 & below);
        // a corner that no emitted triangle names has no number (its word of the map is whatever it was) and is not read
        const int32_t a = q & MESH_A ? (int32_t)number[i] : 0, b = q & MESH_B ? (int32_t)number[i + 1] : 0;
        const int32_t c = q & MESH_C ? (int32_t)number[i + W] : 0, d = q & MESH_D ? (int32_t)number[i + W + 1] : 0;
        const bool bc = q & MESH_BC;
        if (q & MESH_FIRST) {        // T0 = (a, c, d)   T2 = (a, c, b)
            out_faces[o * 3 + 0] = a;
            out_faces[o * 3 + 1] = c;
            out_faces[o * 3 + 2] = bc ? b : d;
            o++;
        }
        if (q & MESH_SECOND) {       // T1 = (a, d, b)   T3 = (b, c, d)
            out_faces[o * 3 + 0] = bc ? b : a;
            out_faces[o * 3 + 1] = bc ? c : d;
            out_faces[o * 3 + 2] = bc ? d : b;
        }
    }
}

}  // namespace sgm
