/*
 * sgbm_volume_oracle.c -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.  See sgbm_volume_oracle.h.
 *
 * The volume form of SURVEY.md Appendix A, stage by stage as tests/bruteforce_sgbm.py states it (bruteforce_hh4.py for
 * the direction set of mode 3, bruteforce_color.py for three channels), in C so that it reaches full-size frames:
 *
 *   1. per image row: pre-filter and half-pixel interval of every channel (A.2), Birchfield-Tomasi cost summed over the
 *      channels (A.3, A.10), horizontal window sum by direct summation over clamped columns          -> volume HS
 *   2. vertical window sum by direct summation over clamped rows (A.4)                                  -> volume C
 *   3. for every direction of the mode's set, the recurrence of A.5 over the whole of C; S = the saturating sum
 *   4. per row: winner-take-all, uniqueness, right view, sub-pixel fit, left-right check (A.6)
 *   5. the frozen oracle's median and speckle filter (A.7, A.8)
 *
 * Nothing is shared with sgbm_oracle.c but the two post filters and the structs: that file walks the frame once per pass
 * with all directions of the pass interleaved and running window sums; this one holds whole volumes.
 *
 * S: every L_r(p, d) = C(p, d) + (min(...) - min_d L_r(q, .)) >= C(p, d) >= 0 inside the int16 regime, so clipping the
 * running sum at 32767 after every direction equals clipping the total once: S is kept as int16.  HS lives in the S
 * buffer, which is dead until stage 3.
 */
#include "sgbm_volume_oracle.h"

#include <stdlib.h>
#include <string.h>

#define MAX_COST 32767

static inline int vmin(int a, int b) { return a < b ? a : b; }
static inline int vmax(int a, int b) { return a > b ? a : b; }
static inline int vclamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

typedef struct {
    int H, W, cn;
    int minD, D, minX1, W1;
    int r;
    int P1, P2, uniq, d12, ftzero, invalid;
    int mode;
} vgeom_t;

/* A.1 */
static void vnormalise(const oracle_sgbm_params *p, int H, int W, int cn, vgeom_t *g)
{
    const int dim = p->blockSize > 0 ? p->blockSize : 5;
    g->H = H;
    g->W = W;
    g->cn = cn;
    g->minD = p->minDisparity;
    g->D = p->numDisparities;
    g->minX1 = vmax(g->minD + g->D, 0);
    g->W1 = W + vmin(g->minD, 0) - g->minX1;
    g->r = dim / 2;
    g->P1 = p->P1 > 0 ? p->P1 : 2;
    g->P2 = vmax(p->P2 > 0 ? p->P2 : 5, g->P1 + 1);
    g->uniq = p->uniquenessRatio >= 0 ? p->uniquenessRatio : 10;
    g->d12 = p->disp12MaxDiff > 0 ? p->disp12MaxDiff : 1;
    g->ftzero = vmax(p->preFilterCap, 15) | 1;
    g->invalid = (g->minD - 1) * 16;
    g->mode = p->mode;
}

/* ---- stage 1 ------------------------------------------------------------------------------------------------------ */
/* one image row, one channel: f[0..2] = value, low, high of the pre-filtered gradient, f[3..5] of the intensity; both
 * hold ftzero (as a byte) in the first and the last column (A.2) */
static void channel_row(const uint8_t *img, int64_t stride, int cn, int c, int y, int H, int W, int ftzero, uint8_t *const f[6])
{
    const uint8_t *mid = img + (int64_t)y * stride + c;
    const uint8_t *up = img + (int64_t)vmax(y - 1, 0) * stride + c;
    const uint8_t *dn = img + (int64_t)vmin(y + 1, H - 1) * stride + c;
    for (int x = 0; x < W; x++) {
        if (x == 0 || x == W - 1) {
            f[0][x] = f[3][x] = (uint8_t)ftzero;
            continue;
        }
        const int a = (x - 1) * cn, b = (x + 1) * cn;
        const int grad = 2 * (mid[b] - mid[a]) + (up[b] - up[a]) + (dn[b] - dn[a]);
        f[0][x] = (uint8_t)(vclamp(grad, -ftzero, ftzero) + ftzero);
        f[3][x] = mid[x * cn];
    }
    for (int k = 0; k < 6; k += 3) {
        const uint8_t *v = f[k];
        for (int x = 0; x < W; x++) {
            const int l = x > 0 ? (v[x] + v[x - 1]) / 2 : v[x];
            const int r = x < W - 1 ? (v[x] + v[x + 1]) / 2 : v[x];
            f[k + 1][x] = (uint8_t)vmin(v[x], vmin(l, r));
            f[k + 2][x] = (uint8_t)vmax(v[x], vmax(l, r));
        }
    }
}

/* pix[(x - minX1) * D + k] += the pixel cost of one channel at disparity minD + k (A.3): gradient in full, intensity / 4 */
static void add_pixel_cost(const vgeom_t *g, uint8_t *const fl[6], uint8_t *const fr[6], int16_t *pix)
{
    for (int xi = 0; xi < g->W1; xi++) {
        const int x = xi + g->minX1;
        int16_t *out = pix + (int64_t)xi * g->D;
        for (int k = 0; k < 6; k += 3) {
            const int u = fl[k][x], u0 = fl[k + 1][x], u1 = fl[k + 2][x];
            const uint8_t *v = fr[k], *v0 = fr[k + 1], *v1 = fr[k + 2];
            const int sh = k == 0 ? 0 : 2;
            for (int d = 0; d < g->D; d++) {
                const int xr = x - g->minD - d;
                const int c0 = vmax(0, vmax(u - v1[xr], v0[xr] - u));
                const int c1 = vmax(0, vmax(v[xr] - u1, u0 - v[xr]));
                out[d] = (int16_t)(out[d] + (vmin(c0, c1) >> sh));
            }
        }
    }
}

static void stage_hsum(const vgeom_t *g, const uint8_t *left, const uint8_t *right, int64_t stride, int16_t *HS)
{
    const int W = g->W, W1 = g->W1, D = g->D;
    const int64_t rowsz = (int64_t)W1 * D;
    uint8_t *fbuf = (uint8_t *)malloc((size_t)W * 12);
    uint8_t *fl[6], *fr[6];
    for (int k = 0; k < 6; k++) {
        fl[k] = fbuf + (size_t)W * k;
        fr[k] = fbuf + (size_t)W * (6 + k);
    }
    int16_t *pix = (int16_t *)malloc((size_t)rowsz * sizeof(int16_t));
    int32_t *sum = (int32_t *)malloc((size_t)D * sizeof(int32_t));
    for (int y = 0; y < g->H; y++) {
        memset(pix, 0, (size_t)rowsz * sizeof(int16_t));
        for (int c = 0; c < g->cn; c++) {
            channel_row(left, stride, g->cn, c, y, g->H, W, g->ftzero, fl);
            channel_row(right, stride, g->cn, c, y, g->H, W, g->ftzero, fr);
            add_pixel_cost(g, fl, fr, pix);
        }
        int16_t *hs = HS + (int64_t)y * rowsz;
        for (int xi = 0; xi < W1; xi++) {
            for (int d = 0; d < D; d++) sum[d] = 0;
            for (int i = -g->r; i <= g->r; i++) {
                const int16_t *src = pix + (int64_t)vclamp(xi + i, 0, W1 - 1) * D;
                for (int d = 0; d < D; d++) sum[d] += src[d];
            }
            for (int d = 0; d < D; d++) hs[(int64_t)xi * D + d] = (int16_t)sum[d];
        }
    }
    free(sum);
    free(pix);
    free(fbuf);
}

/* ---- stage 2 ------------------------------------------------------------------------------------------------------ */
/* C and the first word of the headroom record: max C + P2, and the intermediate C(y - 1) + HS(min(y + r, H - 1)) that
 * upstream's vertical running sum holds in an int16 lane before it subtracts the row that leaves the window (A.9) */
static int stage_vsum(const vgeom_t *g, const int16_t *HS, int16_t *C)
{
    const int H = g->H;
    const int64_t rowsz = (int64_t)g->W1 * g->D;
    int32_t *sum = (int32_t *)malloc((size_t)rowsz * sizeof(int32_t));
    int mx = 0;
    for (int y = 0; y < H; y++) {
        memset(sum, 0, (size_t)rowsz * sizeof(int32_t));
        for (int j = -g->r; j <= g->r; j++) {
            const int16_t *src = HS + (int64_t)vclamp(y + j, 0, H - 1) * rowsz;
            for (int64_t i = 0; i < rowsz; i++) sum[i] += src[i];
        }
        int16_t *c = C + (int64_t)y * rowsz;
        for (int64_t i = 0; i < rowsz; i++) {
            c[i] = (int16_t)sum[i];
            mx = vmax(mx, c[i]);
        }
        if (y > 0) {
            const int16_t *prev = c - rowsz, *in = HS + (int64_t)vmin(y + g->r, H - 1) * rowsz;
            for (int64_t i = 0; i < rowsz; i++) mx = vmax(mx, prev[i] + in[i]);
        }
    }
    free(sum);
    return mx + g->P2;
}

/* ---- stage 3 ------------------------------------------------------------------------------------------------------ */
/* L(p, d) = C(p, d) + min(Lq[d], Lq[d - 1] + P1, Lq[d + 1] + P1, mq + P2) - mq, added to S with the sum clipped at
 * MAX_COST; returns min_d L(p, d).  Lq points at d = 0 of the predecessor's vector, whose slots d = -1 and d = D hold
 * MAX_COST. */
static inline int path_pixel(const int16_t *restrict Cp, const int16_t *restrict Lq, int mq, int P1, int P2, int D,
                             int16_t *restrict Lo, int16_t *restrict Sp, int first)
{
    const int far = mq + P2;
    int mn = MAX_COST;
    for (int d = 0; d < D; d++) {
        const int t = vmin(vmin((int)Lq[d], far), vmin((int)Lq[d - 1], (int)Lq[d + 1]) + P1);
        const int L = Cp[d] + t - mq;
        Lo[d] = (int16_t)L;
        Sp[d] = (int16_t)vmin(first ? L : Sp[d] + L, MAX_COST);
        mn = vmin(mn, L);
    }
    return mn;
}

/* rows of W1 + 2 vectors of D + 2 entries: vector x + 1 belongs to column x; the vectors 0 and W1 + 1, and every vector of
 * a cleared row, are the state outside the frame: L = 0, min = 0 */
static void clear_state(int16_t *L, int16_t *M, int W1, int D)
{
    for (int x = 0; x < W1 + 2; x++) {
        int16_t *v = L + (int64_t)x * (D + 2);
        v[0] = MAX_COST;
        for (int d = 1; d <= D; d++) v[d] = 0;
        v[D + 1] = MAX_COST;
        M[x] = 0;
    }
}

/* one direction (the predecessor of p is p - (rx, ry)) over the whole volume; returns max over pixels of min_d L */
static int stage_direction(const vgeom_t *g, int rx, int ry, const int16_t *C, int16_t *S, int first)
{
    const int H = g->H, W1 = g->W1, D = g->D;
    const int64_t rowsz = (int64_t)W1 * D;
    int16_t *Lb[2], *Mb[2];
    for (int k = 0; k < 2; k++) {
        Lb[k] = (int16_t *)malloc((size_t)(W1 + 2) * (D + 2) * sizeof(int16_t));
        Mb[k] = (int16_t *)malloc((size_t)(W1 + 2) * sizeof(int16_t));
        clear_state(Lb[k], Mb[k], W1, D);
    }
    int id = 0, mmax = 0;
    for (int n = 0; n < H; n++) {
        const int y = ry >= 0 ? n : H - 1 - n;
        int16_t *Lc = Lb[id], *Mc = Mb[id];
        /* ry = 0: the predecessor is in this row (every row starts from the state outside the frame, which the vectors
         * 0 and W1 + 1 hold); otherwise in the row walked before this one */
        const int16_t *Lp = ry == 0 ? Lc : Lb[1 - id], *Mp = ry == 0 ? Mc : Mb[1 - id];
        for (int m = 0; m < W1; m++) {
            const int x = rx >= 0 ? m : W1 - 1 - m;
            const int64_t q = x - rx + 1;
            const int mn = path_pixel(C + (int64_t)y * rowsz + (int64_t)x * D, Lp + q * (D + 2) + 1, Mp[q], g->P1, g->P2, D,
                                      Lc + (int64_t)(x + 1) * (D + 2) + 1, S + (int64_t)y * rowsz + (int64_t)x * D, first);
            Mc[x + 1] = (int16_t)mn;
            mmax = vmax(mmax, mn);
        }
        if (ry != 0) id = 1 - id;
    }
    for (int k = 0; k < 2; k++) {
        free(Lb[k]);
        free(Mb[k]);
    }
    return mmax;
}

/* ---- stage 4 ------------------------------------------------------------------------------------------------------ */
static void stage_select(const vgeom_t *g, const int16_t *S, int16_t *disp)
{
    const int W = g->W, W1 = g->W1, D = g->D, minD = g->minD;
    int *d2 = (int *)malloc((size_t)W * sizeof(int)), *d2c = (int *)malloc((size_t)W * sizeof(int));
    for (int y = 0; y < g->H; y++) {
        int16_t *out = disp + (int64_t)y * W;
        for (int x = 0; x < W; x++) {
            out[x] = (int16_t)g->invalid;
            d2[x] = g->invalid;
            d2c[x] = MAX_COST;
        }
        for (int xi = W1 - 1; xi >= 0; xi--) {
            const int16_t *s = S + ((int64_t)y * W1 + xi) * D;
            int best = 0;
            for (int d = 1; d < D; d++)
                if (s[d] < s[best]) best = d; /* the first minimum */
            const int ms = s[best];
            if (ms >= MAX_COST) continue; /* no S below MAX_COST: invalid, and the right view is left alone */
            int unique = 1;
            for (int d = 0; d < D && unique; d++)
                if (s[d] * (100 - g->uniq) < ms * 100 && abs(best - d) > 1) unique = 0;
            if (!unique) continue;
            const int x2 = xi + g->minX1 - best - minD;
            if (d2c[x2] > ms) {
                d2c[x2] = ms;
                d2[x2] = best + minD;
            }
            int dsc = best * 16;
            if (0 < best && best < D - 1) {
                const int den = vmax(s[best - 1] + s[best + 1] - 2 * s[best], 1);
                dsc += ((s[best - 1] - s[best + 1]) * 16 + den) / (den * 2); /* C division: towards zero */
            }
            out[xi + g->minX1] = (int16_t)(dsc + minD * 16);
        }
        for (int x = g->minX1; x < g->minX1 + W1; x++) {
            const int d1 = out[x];
            if (d1 == g->invalid) continue;
            const int lo = d1 >> 4, hi = (d1 + 15) >> 4;
            const int xa = x - lo, xb = x - hi;
            if (0 <= xa && xa < W && d2[xa] >= minD && abs(d2[xa] - lo) > g->d12 && 0 <= xb && xb < W && d2[xb] >= minD &&
                abs(d2[xb] - hi) > g->d12)
                out[x] = (int16_t)g->invalid;
        }
    }
    free(d2);
    free(d2c);
}

static const int DIRS5[5][2] = {{1, 0}, {1, 1}, {0, 1}, {-1, 1}, {-1, 0}};
static const int DIRS8[8][2] = {{1, 0}, {1, 1}, {0, 1}, {-1, 1}, {-1, 0}, {1, -1}, {0, -1}, {-1, -1}};
static const int DIRS4[4][2] = {{1, 0}, {-1, 0}, {0, 1}, {0, -1}};

int volume_oracle_compute(const oracle_sgbm_params *p, const uint8_t *left, const uint8_t *right, int H, int W,
                          int channels, int64_t stride, int16_t *disp, oracle_sgbm_taps *taps)
{
    if (!p || !left || !right || !disp || H <= 0 || W < 2 || p->numDisparities <= 0) return -1;
    if (p->mode != 0 && p->mode != 1 && p->mode != 3) return -2;
    if (channels != 1 && channels != 3) return -3;
    if (stride < (int64_t)W * channels) return -4;
    vgeom_t g;
    vnormalise(p, H, W, channels, &g);
    const int64_t n = (int64_t)H * W;
    int max_cp2 = 0, max_delta = 0;
    if (g.W1 <= 0) {
        for (int64_t i = 0; i < n; i++) disp[i] = (int16_t)g.invalid;
    } else {
        const size_t vol = (size_t)g.W1 * g.D * H * sizeof(int16_t);
        int16_t *C = taps && taps->C ? taps->C : (int16_t *)malloc(vol);
        int16_t *S = taps && taps->S ? taps->S : (int16_t *)malloc(vol);
        if (!C || !S) return -5;
        stage_hsum(&g, left, right, stride, S);
        max_cp2 = stage_vsum(&g, S, C);
        const int(*dirs)[2] = g.mode == 0 ? DIRS5 : (g.mode == 1 ? DIRS8 : DIRS4);
        const int ndirs = g.mode == 0 ? 5 : (g.mode == 1 ? 8 : 4);
        int mmax = 0;
        for (int k = 0; k < ndirs; k++) mmax = vmax(mmax, stage_direction(&g, dirs[k][0], dirs[k][1], C, S, k == 0));
        max_delta = g.P2 + mmax;
        stage_select(&g, S, disp);
        if (!(taps && taps->C)) free(C);
        if (!(taps && taps->S)) free(S);
    }
    if (taps) {
        taps->max_cost_plus_p2 = max_cp2;
        taps->max_delta = max_delta;
        taps->headroom_ok = max_cp2 <= MAX_COST && max_delta <= MAX_COST;
    }
    if (taps && taps->disp_raw) memcpy(taps->disp_raw, disp, (size_t)n * sizeof(int16_t));
    int16_t *tmp = (int16_t *)malloc((size_t)n * sizeof(int16_t));
    memcpy(tmp, disp, (size_t)n * sizeof(int16_t));
    oracle_median3x3_i16(tmp, disp, H, W);
    free(tmp);
    if (taps && taps->disp_median) memcpy(taps->disp_median, disp, (size_t)n * sizeof(int16_t));
    if (p->speckleRange >= 0 && p->speckleWindowSize > 0)
        oracle_filter_speckles_i16(disp, H, W, (p->minDisparity - 1) * 16, p->speckleWindowSize, 16 * p->speckleRange);
    return 0;
}
