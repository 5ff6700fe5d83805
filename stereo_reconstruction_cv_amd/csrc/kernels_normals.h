// kernels_normals.h -- one normal per vertex of the grid mesh (include/sgm_hip_normals.h: sgm_normals_grid, sgm_mesh_grid_normals):
// the sum of the face normals of the emitted triangles around a pixel, normalised and on request turned towards the camera.  The
// header's definition is the contract.  Like kernels_mesh.h, whose code bytes it reads, it is a pure function of the inputs: one
// streaming pass, one lane per pixel in the row-major walk of MESH_BLOCK pixels per block, no atomics.
//
//   k_normals<LIST>  a lane reads the (up to) four code bytes around its pixel -- the quads it is corner d, c, b and a of -- as
//                    mesh_is_vertex does, and is done if none of them names it.  Otherwise it reads the nine points of its 3 x 3
//                    neighbourhood, the neighbours from the cache (a point is read by up to nine lanes, eight of them in the
//                    same or a neighbouring wave; k_mesh_quads' second read is the precedent), forms the face normals in face
//                    order and adds them up.  <false>: the dense store of the image, zero on non-vertices.  <true>: the ordered
//                    scatter of the list, to the row k_mesh_vertices numbered the pixel with (4 bytes read per vertex beside
//                    the 24 of its point and its normal; redoing the ballot + popcount numbering would cost a block barrier).
//                    The kernel is bound by its instruction count, not by its traffic.
// A point or a code byte outside the frame is never addressed: the row above row 0, the column left of column 0, the row below
// the last and the column right of the last are excluded by x and y, not by the codes.  Offsets are 64-bit.
#pragma once
#include "kernels_mesh.h"

namespace sgm {

struct NrmVec { float x, y, z; };

__device__ __forceinline__ NrmVec nrm_point(const float *__restrict__ xyz, int64_t i)
{
    return NrmVec{xyz[i * 3], xyz[i * 3 + 1], xyz[i * 3 + 2]};
}

// steps 6 and 7 for one triangle (p, q, r): its face normal added to s.  Products and differences are separate roundings (the build
// has -ffp-contract=off).
__device__ __forceinline__ void nrm_add_face(NrmVec &s, const NrmVec &p, const NrmVec &q, const NrmVec &r)
{
    const float e1x = q.x - p.x, e1y = q.y - p.y, e1z = q.z - p.z;
    const float e2x = r.x - p.x, e2y = r.y - p.y, e2z = r.z - p.z;
    s.x += e1y * e2z - e1z * e2y;
    s.y += e1z * e2x - e1x * e2z;
    s.z += e1x * e2y - e1y * e2x;
}

// the triangles of the quad (a, b, c, d) with code q that name the corner `me` (MESH_A .. MESH_D), first before second:
//   a-d:  T0 = (a, c, d) names all but b,  T1 = (a, d, b) all but c;      b-c:  T2 = (a, c, b) all but d,  T3 = (b, c, d) all but a
__device__ __forceinline__ void nrm_add_quad(NrmVec &s, uint32_t q, uint32_t me, const NrmVec &a, const NrmVec &b, const NrmVec &c,
                                             const NrmVec &d)
{
    const bool bc = q & MESH_BC;
    if ((q & MESH_FIRST) && me != (bc ? MESH_D : MESH_B)) nrm_add_face(s, a, c, bc ? b : d);
    if ((q & MESH_SECOND) && me != (bc ? MESH_A : MESH_C)) nrm_add_face(s, bc ? b : a, bc ? c : d, bc ? d : b);
}

template <bool LIST>
__global__ __launch_bounds__(MESH_BLOCK) void k_normals(const float *__restrict__ xyz, const uint8_t *__restrict__ code,
                                                        const uint32_t *__restrict__ number, int H, int W, int orient,
                                                        float *__restrict__ out)
{
    const int64_t n = (int64_t)H * W;
    const int64_t i = (int64_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t x = (uint32_t)i % (uint32_t)W, y = (uint32_t)i / (uint32_t)W;
    const bool left = x > 0, up = y > 0;
    // the four quads around the pixel; the last row and column carry code 0, so a quad named here lies inside the frame
    const uint32_t qd = left && up ? code[i - W - 1] : 0u, qc = up ? code[i - W] : 0u, qb = left ? code[i - 1] : 0u, qa = code[i];
    NrmVec r{0.0f, 0.0f, 0.0f};
    if ((qd & MESH_D) | (qc & MESH_C) | (qb & MESH_B) | (qa & MESH_A)) {   // step 4: a vertex
        const bool right = x + 1 < (uint32_t)W, down = y + 1 < (uint32_t)H;
        const NrmVec z{0.0f, 0.0f, 0.0f};
        const NrmVec p11 = nrm_point(xyz, i);
        const NrmVec p00 = qd ? nrm_point(xyz, i - W - 1) : z, p01 = up ? nrm_point(xyz, i - W) : z;
        const NrmVec p02 = up && right ? nrm_point(xyz, i - W + 1) : z, p10 = left ? nrm_point(xyz, i - 1) : z;
        const NrmVec p12 = right ? nrm_point(xyz, i + 1) : z, p20 = left && down ? nrm_point(xyz, i + W - 1) : z;
        const NrmVec p21 = down ? nrm_point(xyz, i + W) : z, p22 = right && down ? nrm_point(xyz, i + W + 1) : z;
        NrmVec s{0.0f, 0.0f, 0.0f};
        nrm_add_quad(s, qd, MESH_D, p00, p01, p10, p11);
        nrm_add_quad(s, qc, MESH_C, p01, p02, p11, p12);
        nrm_add_quad(s, qb, MESH_B, p10, p11, p20, p21);
        nrm_add_quad(s, qa, MESH_A, p11, p12, p21, p22);
        // step 8 (fmaxf drops a NaN, so the three components are asked themselves)
        const float m = fmaxf(fmaxf(fabsf(s.x), fabsf(s.y)), fabsf(s.z));
        if (isfinite(s.x) && isfinite(s.y) && isfinite(s.z) && m > 0.0f) {
            const float ux = s.x / m, uy = s.y / m, uz = s.z / m;
            const float l = sqrtf((ux * ux + uy * uy) + uz * uz);
            r = NrmVec{ux / l, uy / l, uz / l};
            // step 9
            if (orient && (r.x * p11.x + r.y * p11.y) + r.z * p11.z > 0.0f) r = NrmVec{-r.x, -r.y, -r.z};
        }
        if (LIST) {
            const int64_t o = (int64_t)number[i] * 3;
            out[o] = r.x;
            out[o + 1] = r.y;
            out[o + 2] = r.z;
        }
    }
    if (!LIST) {
        out[i * 3] = r.x;
        out[i * 3 + 1] = r.y;
        out[i * 3 + 2] = r.z;
    }
}

}  // namespace sgm
