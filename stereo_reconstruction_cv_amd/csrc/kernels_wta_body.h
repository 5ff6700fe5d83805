// kernels_wta_body.h -- the body of k_wta_t and k_wta_conf_t (kernels_post.h), included once in each: NOT a header of its
// own.  Expects in scope: the kernel's parameters (g, S, wta, npix, S2 .. S5), POSW, LG, NV, and
//   constexpr bool CONF; uint8_t *conf     -- CONF: also store the confidence byte (conf_raw) of every pixel to conf
// Kept as shared text rather than a shared device function: k_wta_t must compile to the same instructions with and without
// the confidence form beside it (through an inlined function its __restrict__ kernel arguments reach the optimiser as scoped
// metadata, and every instantiation came out scheduled differently).
    constexpr bool TWO = NV >= 2, THREE = NV >= 3, FOUR = NV >= 4, FIVE = NV >= 5;
    static_assert(NV >= 1 && NV <= 5, "volumes: 1 .. 5");
    extern __shared__ __attribute__((aligned(16))) uint8_t rows[];
    const int lane = threadIdx.x, D = LG >= 0 ? (8 << LG) : g.D, W1 = g.W1;
    const int stride = wta_t_stride(D);
    const int cpr = D * 2 / 16;  // 16-byte chunks per pixel row; a lane moves cpr chunks per block
    const int64_t nblocks = (npix + 63) / 64;
    constexpr int PF = LG < 0 ? 8 : (LG >= 5 ? 32 : (1 << LG));  // chunks per lane held in registers
    uint4 v[PF], v2[TWO ? PF : 1], v3[THREE ? PF : 1], v4[FOUR ? PF : 1], v5[FIVE ? PF : 1];
    // chunk c = lane + 64 k of the block's contiguous 64 * D * 2 bytes: loads with a clamped index
    // (no branch between them), committed to the padded LDS rows afterwards
    auto issue = [&](int64_t blk, int k0) {
        const int64_t left = npix - blk * 64;  // (integer compare: min<int64_t>() goes through v_min_f64)
        const int total = (left < 64 ? (int)left : 64) * cpr;
        const uint4 *src = reinterpret_cast<const uint4 *>(S + blk * 64 * D);
#pragma unroll
        for (int u = 0; u < PF; u++) v[u] = src[min(lane + 64 * (k0 + u), total - 1)];
        if constexpr (TWO) {
            const uint4 *src2 = reinterpret_cast<const uint4 *>(S2 + blk * 64 * D);
#pragma unroll
            for (int u = 0; u < PF; u++) v2[u] = src2[min(lane + 64 * (k0 + u), total - 1)];
        }
        if constexpr (THREE) {
            const uint4 *src3 = reinterpret_cast<const uint4 *>(S3 + blk * 64 * D);
#pragma unroll
            for (int u = 0; u < PF; u++) v3[u] = src3[min(lane + 64 * (k0 + u), total - 1)];
        }
        if constexpr (FOUR && !FIVE) {
            const uint4 *src4 = reinterpret_cast<const uint4 *>(S4 + blk * 64 * D);
#pragma unroll
            for (int u = 0; u < PF; u++) v4[u] = src4[min(lane + 64 * (k0 + u), total - 1)];
        }
        if constexpr (FIVE) {
            const uint4 *src4 = reinterpret_cast<const uint4 *>(S4 + blk * 64 * D);
            const uint4 *src5 = reinterpret_cast<const uint4 *>(S5 + blk * 64 * D);
#pragma unroll
            for (int u = 0; u < PF; u++) v4[u] = src4[min(lane + 64 * (k0 + u), total - 1)];
#pragma unroll
            for (int u = 0; u < PF; u++) v5[u] = src5[min(lane + 64 * (k0 + u), total - 1)];
        }
    };
    auto summed = [&](int u) {  // chunk u of the cost rows: S, or sat(S + S2)
        uint4 r = v[u];
        if constexpr (TWO) {
            r.x = pk_adds_s(r.x, v2[u].x);
            r.y = pk_adds_s(r.y, v2[u].y);
            r.z = pk_adds_s(r.z, v2[u].z);
            r.w = pk_adds_s(r.w, v2[u].w);
        }
        if constexpr (THREE) {
            r.x = pk_adds_s(r.x, v3[u].x);
            r.y = pk_adds_s(r.y, v3[u].y);
            r.z = pk_adds_s(r.z, v3[u].z);
            r.w = pk_adds_s(r.w, v3[u].w);
        }
        if constexpr (FOUR && !FIVE) {
            r.x = pk_adds_s(r.x, v4[u].x);
            r.y = pk_adds_s(r.y, v4[u].y);
            r.z = pk_adds_s(r.z, v4[u].z);
            r.w = pk_adds_s(r.w, v4[u].w);
        }
        if constexpr (FIVE) {
            r.x = pk_adds_s(pk_adds_s(r.x, v4[u].x), v5[u].x);
            r.y = pk_adds_s(pk_adds_s(r.y, v4[u].y), v5[u].y);
            r.z = pk_adds_s(pk_adds_s(r.z, v4[u].z), v5[u].z);
            r.w = pk_adds_s(pk_adds_s(r.w, v4[u].w), v5[u].w);
        }
        return r;
    };
    auto commit = [&](int64_t blk, int k0) {
        const int64_t left = npix - blk * 64;
        const int total = (left < 64 ? (int)left : 64) * cpr;
#pragma unroll
        for (int u = 0; u < PF; u++) {
            const int c = lane + 64 * (k0 + u);
            if (c < total) {
                const int px = LG >= 0 ? c >> LG : c / cpr, w = c - px * cpr;
                uint2 *dst = reinterpret_cast<uint2 *>(rows + px * stride + w * 16);
                const uint4 q = summed(u);
                dst[0] = make_uint2(q.x, q.y);
                dst[1] = make_uint2(q.z, q.w);
            }
        }
    };
    int64_t blk = blockIdx.x;
    if (LG >= 0 && blk < nblocks) issue(blk, 0);
    for (; blk < nblocks; blk += gridDim.x) {
    const int64_t p0 = blk * 64;
    const int np = npix - p0 < 64 ? (int)(npix - p0) : 64;
    __syncthreads();  // (one wave per block: orders the LDS traffic of consecutive blocks)
    if (LG >= 0) {
        commit(blk, 0);
        if (LG == 6) {  // D = 512: the second half of the rows, not prefetched
            issue(blk, PF);
            commit(blk, PF);
        }
    } else {
        for (int k0 = 0; k0 < cpr; k0 += PF) {  // cpr need not be a multiple of PF: clamped loads, guarded commits
            issue(blk, k0);
            const int total = np * cpr;
#pragma unroll
            for (int u = 0; u < PF; u++) {
                const int c = lane + 64 * (k0 + u);
                if (k0 + u < cpr && c < total) {
                    const int px = c / cpr, w = c - px * cpr;
                    uint2 *dst = reinterpret_cast<uint2 *>(rows + px * stride + w * 16);
                    const uint4 q = summed(u);
                    dst[0] = make_uint2(q.x, q.y);
                    dst[1] = make_uint2(q.z, q.w);
                }
            }
        }
    }
    __syncthreads();
    if (LG >= 0 && blk + gridDim.x < nblocks) issue(blk + gridDim.x, 0);  // next block's loads fly during this scan
    if (lane < np) {
    const uint8_t *row = rows + lane * stride;
    // pass 1
    uint32_t key = 0xffffffffu;
#pragma unroll 64  // fully unrolled for D <= 256: constant offsets and disparity indices, many LDS reads in flight
    for (int d0 = 0; d0 < D; d0 += 4) {
        const uint2 v = *reinterpret_cast<const uint2 *>(row + d0 * 2);
        const uint32_t k0 = (v.x << 16) | (uint32_t)d0, k1 = (v.x & 0xffff0000u) | (uint32_t)(d0 + 1);
        const uint32_t k2 = (v.y << 16) | (uint32_t)(d0 + 2), k3 = (v.y & 0xffff0000u) | (uint32_t)(d0 + 3);
        key = min(min(key, min(k0, k1)), min(k2, k3));
    }
    const int minS = (int)(key >> 16), best = (int)(key & 0xffffu);
    const int wgt = 100 - g.uniq, thr = minS * 100;
    bool reject;
    // S[best -+ 1] for the sub-pixel step (clamped: k_select uses them only for 0 < best < D-1)
    const int dm = max(best - 1, 0), dp = min(best + 1, D - 1);
    uint16_t *rw = reinterpret_cast<uint16_t *>(rows + lane * stride);
    const uint32_t nb = (uint32_t)rw[dm] | ((uint32_t)rw[dp] << 16);
    if constexpr (CONF) {
        // the per-d test first (non-positive weight only: it needs the row as it is), then the far minimum for the byte
        const bool posw = wgt > 0;
        reject = false;
        if (!posw) {
            for (int d = 0; d < D; d++) {
                const int sv = *reinterpret_cast<const uint16_t *>(row + d * 2);
                reject |= (sv * wgt < thr) && (abs(best - d) > 1);
            }
        }
        rw[dm] = (uint16_t)SGM_MAX_COST;
        rw[best] = (uint16_t)SGM_MAX_COST;
        rw[dp] = (uint16_t)SGM_MAX_COST;
        uint32_t far2 = SGM_SENT;
#pragma unroll 64
        for (int d0 = 0; d0 < D; d0 += 4) {
            const uint2 v = *reinterpret_cast<const uint2 *>(row + d0 * 2);
            far2 = pk_min_s(far2, pk_min_s(v.x, v.y));
        }
        const uint32_t far = min(far2 & 0xffffu, far2 >> 16);  // D >= 16: some d lies outside best-1 .. best+1
        if (posw) reject = (int)far * wgt < thr;
        const uint32_t c = far == 0 ? 100u : (far - (uint32_t)minS) * 100u / far;  // below 2^22: plain unsigned division
        const int64_t pc = p0 + lane;
        const int yc = (int)(pc / W1), xc = (int)(pc - (int64_t)yc * W1);
        conf[(int64_t)yc * g.W + g.minX1 + xc] = (uint8_t)c;
    } else if (POSW) {
        // wgt > 0: one comparison against the smallest S outside best-1..best+1.  The row in LDS is
        // this lane's alone and not needed again: overwrite those three entries with MAX_COST and
        // take a plain packed minimum of the row.
        rw[dm] = (uint16_t)SGM_MAX_COST;
        rw[best] = (uint16_t)SGM_MAX_COST;
        rw[dp] = (uint16_t)SGM_MAX_COST;
        uint32_t far = SGM_SENT;
#pragma unroll 64
        for (int d0 = 0; d0 < D; d0 += 4) {
            const uint2 v = *reinterpret_cast<const uint2 *>(row + d0 * 2);
            far = pk_min_s(far, pk_min_s(v.x, v.y));
        }
        reject = (int)min(far & 0xffffu, far >> 16) * wgt < thr;
    } else {
        reject = false;
        for (int d = 0; d < D; d++) {
            const int sv = *reinterpret_cast<const uint16_t *>(row + d * 2);
            reject |= (sv * wgt < thr) && (abs(best - d) > 1);
        }
    }
    reject = reject || (minS == SGM_MAX_COST);
    const int64_t p = p0 + lane;
    const int y = (int)(p / W1), x = (int)(p - (int64_t)y * W1);
    wta[(int64_t)y * g.W + g.minX1 + x] = make_uint2(reject ? 0xffffffffu : key, nb);
    }  // lane < np
    }  // blocks of this workgroup
