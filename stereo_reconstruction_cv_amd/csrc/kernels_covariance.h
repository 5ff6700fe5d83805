// kernels_covariance.h -- covariance normals of a point list (include/sgm_hip_covariance.h: sgm_covariance_normals): per point
// the integer moments of its neighbours within r, and from them in binary64 the covariance, its eigenvectors by six Jacobi
// sweeps, the normal and the surface variation.  The grid of cells is that of kernels_radius.h, built by the same kernels (count,
// clear, insert, starts, sort); the header's definition is the contract.
//
//   k_cov_query<SEPARATE, SELECT>  THE HOT KERNEL.  One lane per point in the order of the sorted records, over its 27 cells by
//                     rad_walk (kernels_radius.h) -- nothing ends a point's search early.  The visitor: per neighbour the three
//                     offsets quantised by one product and one v_rndne each, and nine signed 64-bit sums in registers (eighteen
//                     VGPRs, every index a constant): three 64-bit adds and six 32 x 32 + 64 multiply-adds (v_mad_i64_i32).
//                     SELECT = false: the accumulation is left out for a candidate that is no neighbour, so a wave none of whose
//                     lanes has a neighbour in the candidate branches over it; true: the offsets of a candidate that is no
//                     neighbour are made 0 and the accumulation runs for all.  SEPARATE = false: steps 7 to 10 at the end of the same lane (cov_solve), the
//                     outputs to the source index, the two counts of out_stats by a ballot per wave and one atomicAdd per block
//                     and word; true: the nine sums and the count go to ten staged 64-bit words per point and k_cov_solve does
//                     the rest.
//   k_cov_solve       SEPARATE only: one lane per sorted record, steps 7 to 10 from the staged words; outputs and counts as above.
//   k_cov_fill        the points that are in no cell: normal (0, 0, 0), curvature -1 (their count of 0 is k_radius_sort's).
// cov_solve is plain binary64 C++: the build has -ffp-contract=off, and the compiler's expansions of the binary64 division and
// square root are the correctly rounded ones.  The Jacobi sweeps run in a loop that is not unrolled over three inlined rotations
// on named scalars, so nothing is indexed at run time and nothing goes to scratch memory.
// Nothing waits for anything, and every probe is bounded by the table's capacity (rad_find).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_radius.h"

namespace sgm {

constexpr int COV_MIN_K = 2;
constexpr int COV_WORDS = 10;   // the staged words of a point: S_0 S_1 S_2 S_00 S_01 S_02 S_11 S_12 S_22 c
enum { COV_CTL_NORMAL = 0, COV_CTL_DEGENERATE = 1, COV_CTL_WORDS = 4 };

struct CovView {
    float qscale, wx, wy, wz;   // the host constant of step 4, the viewpoint
    uint32_t k, orient;
};

// one Jacobi rotation of step 8 on the pair (p, q) with third index r: every operation on its own
__device__ __forceinline__ void cov_rotate(double &app, double &aqq, double &apq, double &arp, double &arq, double &v0p, double &v0q,
                                           double &v1p, double &v1q, double &v2p, double &v2q)
{
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double root = sqrt(theta * theta + 1.0);
    const double den = fabs(theta) + root;
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / den;
    const double c = 1.0 / sqrt(t * t + 1.0);
    const double sn = t * c;
    const double h = t * apq;
    app = app - h;
    aqq = aqq + h;
    apq = 0.0;
    const double rp = c * arp - sn * arq, rq = sn * arp + c * arq;
    arp = rp, arq = rq;
    const double p0 = c * v0p - sn * v0q, q0 = sn * v0p + c * v0q;
    v0p = p0, v0q = q0;
    const double p1 = c * v1p - sn * v1q, q1 = sn * v1p + c * v1q;
    v1p = p1, v1q = q1;
    const double p2 = c * v2p - sn * v2q, q2 = sn * v2p + c * v2q;
    v2p = p2, v2q = q2;
}

// one of three binary64 values by masks of which exactly one is all ones
__device__ __forceinline__ double cov_pick(double a, double b, double c, long long ma, long long mb, long long mc)
{
    return __longlong_as_double((__double_as_longlong(a) & ma) | (__double_as_longlong(b) & mb) | (__double_as_longlong(c) & mc));
}

// steps 7 to 9 up to the normalisation, for m terms: the unit normal in binary64 (n0, n1, n2), the diagonal after the sweeps
// (l0, l1, l2) and its smallest entry.  false: degenerate.  (kernels_plane.h refits a plane with this.)
__device__ __forceinline__ bool cov_normal(long long s0, long long s1, long long s2, long long s00, long long s01, long long s02,
                                           long long s11, long long s12, long long s22, double m, double &n0, double &n1, double &n2,
                                           double &l0, double &l1, double &l2, double &lmin)
{
    const double d0 = (double)s0, d1 = (double)s1, d2 = (double)s2;
    double a00 = (double)s00 - (d0 * d0) / m, a01 = (double)s01 - (d0 * d1) / m, a02 = (double)s02 - (d0 * d2) / m;
    double a11 = (double)s11 - (d1 * d1) / m, a12 = (double)s12 - (d1 * d2) / m, a22 = (double)s22 - (d2 * d2) / m;
    const double s = fmax(fmax(a00, a11), a22);
    if (!(s > 0.0)) return false;
    a00 = a00 / s, a01 = a01 / s, a02 = a02 / s, a11 = a11 / s, a12 = a12 / s, a22 = a22 / s;
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
#pragma unroll 1
    for (int sweep = 0; sweep < 6; sweep++) {
        cov_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);   // (0, 1), r = 2
        cov_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);   // (0, 2), r = 1
        cov_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);   // (1, 2), r = 0
    }
    // column i* of V, i* the first smallest diagonal entry.  The column is picked by masks on the bit patterns: written as selects
    // the compiler turns the choice into a load from a nine-word table in scratch memory.
    const bool pick1 = a11 < a00, pick2 = a22 < (pick1 ? a11 : a00);
    lmin = pick2 ? a22 : (pick1 ? a11 : a00);
    const long long m2 = pick2 ? -1ll : 0ll, m1 = pick1 && !pick2 ? -1ll : 0ll, m0 = ~(m1 | m2);
    n0 = cov_pick(v00, v01, v02, m0, m1, m2), n1 = cov_pick(v10, v11, v12, m0, m1, m2), n2 = cov_pick(v20, v21, v22, m0, m1, m2);
    const double len = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
    n0 = n0 / len, n1 = n1 / len, n2 = n2 / len;
    l0 = fmax(a00, 0.0), l1 = fmax(a11, 0.0), l2 = fmax(a22, 0.0);
    return true;
}

// steps 7 to 10 for a point with c >= k neighbours.  false: degenerate (the caller writes zeros and -1)
__device__ __forceinline__ bool cov_solve(long long s0, long long s1, long long s2, long long s00, long long s01, long long s02,
                                          long long s11, long long s12, long long s22, uint32_t c, float x, float y, float z,
                                          const CovView &V, float nrm[3], float &kappa)
{
    double n0, n1, n2, l0, l1, l2, lmin;
    if (!cov_normal(s0, s1, s2, s00, s01, s02, s11, s12, s22, (double)(c + 1u), n0, n1, n2, l0, l1, l2, lmin)) return false;
    if (V.orient) {
        const double w0 = (double)x - (double)V.wx, w1 = (double)y - (double)V.wy, w2 = (double)z - (double)V.wz;
        if ((n0 * w0 + n1 * w1) + n2 * w2 > 0.0) n0 = -n0, n1 = -n1, n2 = -n2;
    }
    nrm[0] = (float)n0, nrm[1] = (float)n1, nrm[2] = (float)n2;
    const double lsum = (l0 + l1) + l2;
    kappa = lsum == 0.0 ? 0.0f : (float)(fmax(lmin, 0.0) / lsum);
    return true;
}

// the outputs of one point at its source index (steps 9 to 11) and the block's two counts: every lane of the block comes here
__device__ __forceinline__ void cov_finish(bool live, long long s0, long long s1, long long s2, long long s00, long long s01,
                                           long long s02, long long s11, long long s12, long long s22, uint32_t c, float x, float y,
                                           float z, uint32_t self, const CovView &V, float *__restrict__ normals,
                                           float *__restrict__ curvature, uint32_t *__restrict__ counts, uint32_t *__restrict__ ctl)
{
    float nrm[3] = {0.0f, 0.0f, 0.0f}, kappa = -1.0f;
    const bool enough = live && c >= V.k;
    const bool solved = enough && cov_solve(s0, s1, s2, s00, s01, s02, s11, s12, s22, c, x, y, z, V, nrm, kappa);
    if (live) {
        if (normals) {
            normals[3 * (size_t)self] = nrm[0];
            normals[3 * (size_t)self + 1] = nrm[1];
            normals[3 * (size_t)self + 2] = nrm[2];
        }
        if (curvature) curvature[self] = kappa;
        if (counts) counts[self] = c;
    }
    const uint32_t nn = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(solved));
    const uint32_t nd = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(enough && !solved));
    __shared__ uint32_t wsum[4][2];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
        wsum[w][COV_CTL_NORMAL] = nn;
        wsum[w][COV_CTL_DEGENERATE] = nd;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const uint32_t t = wsum[0][threadIdx.x] + wsum[1][threadIdx.x] + wsum[2][threadIdx.x] + wsum[3][threadIdx.x];
        if (t) atomicAdd(&ctl[threadIdx.x], t);
    }
}

template <bool SEPARATE, bool SELECT>
__global__ __launch_bounds__(256) void k_cov_query(const float4 *__restrict__ sorted, uint32_t n_in, RadGrid G,
                                                   const RadSlot *__restrict__ tab, uint32_t mask, CovView V,
                                                   long long *__restrict__ staged, float *__restrict__ normals,
                                                   float *__restrict__ curvature, uint32_t *__restrict__ counts,
                                                   uint32_t *__restrict__ ctl)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = t < n_in;
    const float4 me = sorted[live ? t : (int64_t)n_in - 1];   // (n_in >= 1; a lane past the end does nothing with it)
    const float x = me.x, y = me.y, z = me.z;
    const uint32_t self = __float_as_uint(me.w);
    long long s0 = 0, s1 = 0, s2 = 0, s00 = 0, s01 = 0, s02 = 0, s11 = 0, s12 = 0, s22 = 0;
    uint32_t c = 0;
    // (a lane past the end walks nothing and stays: cov_finish is wave-wide)
    rad_walk(sorted, tab, mask, G, x, y, z, [&] { return live; }, [&](bool inside, uint32_t w, float dx, float dy, float dz, float) {
        // (& and not &&: w is read whether or not the candidate is inside, so its record stays one 16-byte load.  With && the
        // compiler loads the index word of a step's first record under the distance test, a dependent load with a full wait in
        // the loop: 2 to 8 % of cov_query, measured)
        const bool near = inside & (w != self);
        c += near ? 1u : 0u;
        // SELECT: a candidate that is no neighbour adds zeros (its products may be anything: they are not converted)
        if (!SELECT && !near) return;
        const auto quant = [&](float d) { return (int)rintf(near ? d * V.qscale : 0.0f); };
        const int qx = quant(dx), qy = quant(dy), qz = quant(dz);
        s0 += qx, s1 += qy, s2 += qz;
        s00 += (long long)qx * qx, s01 += (long long)qx * qy, s02 += (long long)qx * qz;
        s11 += (long long)qy * qy, s12 += (long long)qy * qz, s22 += (long long)qz * qz;
    });
    if (SEPARATE) {
        if (!live) return;
        long long *w = staged + (size_t)t * COV_WORDS;
        w[0] = s0, w[1] = s1, w[2] = s2, w[3] = s00, w[4] = s01, w[5] = s02, w[6] = s11, w[7] = s12, w[8] = s22, w[9] = (long long)c;
    } else {
        cov_finish(live, s0, s1, s2, s00, s01, s02, s11, s12, s22, c, x, y, z, self, V, normals, curvature, counts, ctl);
    }
}

__global__ __launch_bounds__(256) void k_cov_solve(const float4 *__restrict__ sorted, uint32_t n_in, CovView V,
                                                   const long long *__restrict__ staged, float *__restrict__ normals,
                                                   float *__restrict__ curvature, uint32_t *__restrict__ counts,
                                                   uint32_t *__restrict__ ctl)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = t < n_in;
    const int64_t r = live ? t : (int64_t)n_in - 1;
    const float4 me = sorted[r];
    const long long *w = staged + (size_t)r * COV_WORDS;
    cov_finish(live, w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], w[8], (uint32_t)w[9], me.x, me.y, me.z, __float_as_uint(me.w), V,
               normals, curvature, counts, ctl);
}

__global__ __launch_bounds__(256) void k_cov_fill(const uint2 *__restrict__ pt, int64_t n, float *__restrict__ normals,
                                                  float *__restrict__ curvature)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || pt[i].x != VOX_NONE) return;
    if (normals) normals[3 * i] = 0.0f, normals[3 * i + 1] = 0.0f, normals[3 * i + 2] = 0.0f;
    if (curvature) curvature[i] = -1.0f;
}

}  // namespace sgm
