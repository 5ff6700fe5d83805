/* sgm_debug.h -- A/B switches of the engine (SGM_OPT_DEBUG, a bit mask).  NOT part of the drop-in boundary
 * (include/sgm_hip.h): measurement scaffolding for tools/ and tests/ only.  Results stay bit-exact for every bit
 * except SGM_DBG_SKIP_BOUNDARY_LOADS, which sgm_set_option refuses unless SGM_ALLOW_WRONG_RESULTS=1 is in the
 * environment.  Bits that selected kernels round 2 measured and rejected (4096: four-direction row kernel and
 * three-role grouped pre-pass for small D; 8192: that schedule for D <= 32 only; 16384: short prefetch blocks in
 * the upward pre-pass) went away with those kernels in round 3. */
#ifndef SGM_DEBUG_H
#define SGM_DEBUG_H

#define SGM_OPT_DEBUG 4 /* sgm_set_option(e, SGM_OPT_DEBUG, mask) */

/* Poison switch: sgm_set_option(e, SGM_OPT_POISON, b) with b in 0..255 fills, in stream order, every device buffer that
 * e and the engines behind it (peer, peer2, group) own with the byte b -- all but the sticky give-up flag chain_err, which
 * is state by contract -- and ARMS the switch: from then on every buffer that any engine of the process allocates or
 * regrows is filled with b as well.  Any other value (-1) disarms it and fills nothing.  For tests that must not depend
 * on what a call finds in the engine's buffers (tests/test_gpu_history.py); while it is not armed the engine enqueues
 * nothing for it, and no kernel knows about it. */
#define SGM_OPT_POISON 9

enum {
    SGM_DBG_WTA_IN_LAST_PATH = 2,        /* winner-take-all fused into the last path kernel everywhere (pre-pass schedule) */
    SGM_DBG_NO_LANE_GROUPS = 4,          /* D <= 64 through the wave-per-pixel kernels */
    SGM_DBG_NARROW_VSUM = 8,             /* k_vsum_ring with 4 int16 per thread */
    SGM_DBG_PREPASS_3_LAUNCHES = 16,     /* boundary pre-pass as three launches of the single-direction kernel */
    SGM_DBG_NO_PREPASS_OVERLAP = 32,     /* MODE_HH: upward pre-pass on the main stream */
    SGM_DBG_SKIP_BOUNDARY_LOADS = 64,    /* the sweep's loader wave skips its HBM loads: timing only, results WRONG */
    SGM_DBG_FORK_PREPASS_EARLY = 128,    /* fork the upward pre-pass right after the cost stage */
    SGM_DBG_INT16_COST = 256,            /* int16 cost pipeline (k_hsum + k_vsum_ring) instead of the byte one */
    SGM_DBG_PREPASS_ONE_CHUNK = 512,     /* pre-pass in one chunk with the plain line-per-block layout */
    SGM_DBG_WTA_SEPARATE = 2048,         /* winner-take-all always as its own pass */
    SGM_DBG_SMALL_D_RECORD = 8192,       /* D <= 64, MODE_SGBM: per-row record + element-wise vertical kernel (k_prepass3_g + k_vert3_g) instead of k_lines3_g's volumes */
    SGM_DBG_IN_ROW_ON_MAIN_STREAM = 4096, /* D <= 64, MODE_SGBM: the left-to-right in-row path after the vertical kernel (S +=) instead of beside it */
    SGM_DBG_FIFTH_PATH_AFTER_SWEEP = 65536, /* MODE_SGBM, D <= 128: the fifth path after the sweep (S +=) instead of beside it */
    /* sgm_wls_filter* and sgm_wls_filter_batch* (a single map is a batch of one): the other shapes of the line kernels that
     * DESIGN.md 4.15 / 4.16 measured (tools/wls_batch_times.py); two small fields, not flags.  0 in a field leaves the choice
     * to the library (index 0 for a chunk of several maps; rows 3, columns 1 for a chunk of one), any other value selects that
     * shape for every chunk; the results are the same bits for every value (tests/test_gpu_wls.py runs them all). */
    SGM_DBG_WLS_BATCH_ROWS_SHIFT = 17,     /* 3 bits: k_wls_rows<CN, RW, TC>, the index into wls_rows_shapes (sgm_engine.hip) */
    SGM_DBG_WLS_BATCH_COLS_SHIFT = 20,     /* 2 bits: k_wls_cols<CN, UNR>, the index into wls_cols_shapes */
    /* sgm_voxel_downsample* (tools/voxel_times.py); the results are the same bits under both */
    SGM_DBG_VOXEL_TIGHT_TABLE = 1 << 22,   /* capacity = the smallest power of two >= the points in range (not twice them): the load can reach 1.0 */
    SGM_DBG_VOXEL_OTHER_REDUCTION = 1 << 23, /* k_voxel_insert without the wave pre-reduction where it is the default (kernels_voxel.h: VOX_PRE_DEFAULT), with it where not */
    /* sgm_radius_outlier* (tools/radius_times.py); the results are the same bits under both */
    SGM_DBG_RADIUS_TIGHT_TABLE = 1 << 24,   /* capacity = the smallest power of two >= the points in range (not twice them): the load can reach 1.0 */
    SGM_DBG_RADIUS_SOURCE_ORDER = 1 << 25,  /* k_radius_query over the points in source order instead of sorted by cell */
    /* sgm_statistical_outlier* (tools/statistical_times.py); SGM_DBG_RADIUS_TIGHT_TABLE acts on its table too; the same bits under all */
    SGM_DBG_STAT_WIDE_LIST = 1 << 26,       /* k_stat_query<64> whatever nb_neighbors is: the cost of the list's capacity apart from that of k */
    /* sgm_covariance_normals* (tools/covariance_times.py); SGM_DBG_RADIUS_TIGHT_TABLE acts on its table too; the same bits under all */
    SGM_DBG_COV_SEPARATE_SOLVE = 1 << 27,   /* steps 7 to 10 in a kernel of their own (k_cov_solve) over ten staged words per point instead of at the end of k_cov_query's lane */
    SGM_DBG_COV_SELECT_ACCUM = 1 << 28,     /* k_cov_query adds zeros for a candidate that is no neighbour instead of branching over the accumulation */
    /* sgm_cluster_dbscan* (tools/dbscan_times.py); SGM_DBG_RADIUS_TIGHT_TABLE acts on its table and SGM_DBG_RADIUS_SOURCE_ORDER on nothing of it; the same bits under all */
    SGM_DBG_DBSCAN_GATHER_CORE = 1 << 29,   /* k_dbscan_link gathers core[source index] per candidate instead of reading the core bit k_dbscan_mark put into the sorted record */
    /* sgm_segment_plane* (tools/plane_times.py); the same bits under both */
    SGM_DBG_PLANE_OTHER_COUNT = 1 << 30     /* step 5 by the form that is not the default (kernels_plane.h: PLANE_DEFAULT_MFMA): k_plane_count_mfma where k_plane_count_valu is, and the other way round */
};

/* Plan readout: what normalise + make_plan decide for one compute of a frame of H x W pixels on an engine with these
 * options, without an engine and without a GPU (like sgm_geometry).  For tests that must prove which schedule a case
 * takes instead of assuming it; the fields are those of Geom and Plan in sgm_engine.hip.  chain_window: workgroups of one
 * automatic chained sweep launch over `frames` frames (0 where the plan is not chained). */
typedef struct {
    int W1, minX1, NP, partial;  /* partial: the PARTIAL instantiation (with_np; with_gw where the small-D kernels run) */
    int byte_cost, pix_px, GWc, RBb, vsum_ring;
    int rows4, GWs, chain, R, nbands;
    int fused_prepass, prepass_g, pre_nch, pre_rows, overlap;
    int fused_wta, nvol, path_w_main, speckle;
    int chain_window;
} sgm_debug_plan_t;

#ifdef __cplusplus
extern "C"
#endif
int sgm_debug_plan(const sgm_params *p, int H, int W, int channels, int schedule, int sweep_rows, int prepass_rows,
                   int debug, int frames, sgm_debug_plan_t *out);
/* ... and with the options that change a plan but came after that signature was fixed: SGM_OPT_CONFIDENCE, SGM_OPT_RIGHT_VIEW */
#ifdef __cplusplus
extern "C"
#endif
int sgm_debug_plan_opts(const sgm_params *p, int H, int W, int channels, int schedule, int sweep_rows, int prepass_rows,
                        int debug, int frames, int confidence, int right_view, sgm_debug_plan_t *out);
/* ... and SGM_OPT_COST: cost = SGM_COST_BT gives what sgm_debug_plan_opts gives; with SGM_COST_CENSUS byte_cost says which box
 * route the census bytes take (k_box_u8, or k_hsum_u8 + k_vsum*), and 3 channels return the compute's error code */
#ifdef __cplusplus
extern "C"
#endif
int sgm_debug_plan_cost(const sgm_params *p, int H, int W, int channels, int schedule, int sweep_rows, int prepass_rows,
                        int debug, int frames, int confidence, int right_view, int cost, sgm_debug_plan_t *out);

/* Split winner-take-all (kernels_path.h: wta_reduce_pixels, kernels_post.h: k_wta_select), for tests; none needs a GPU.
 * sgm_debug_uniq_threshold: T1 = ceil(100 minS / (100 - uniquenessRatio)) as the kernels compute it from the integer
 *   reciprocal (before they clamp it to 0x8000); -1 outside minS 0 .. 32767, uniquenessRatio 0 .. 99.
 * sgm_debug_wta_split: 1 if one compute of an H x W frame with these options takes the split form (Plan::wta_split), else 0
 *   (negative: an error code).
 * sgm_debug_wta_raw_bytes: bytes of raw-record buffers that e and the engines of its chained group hold.
 * sgm_debug_wta_select_n: the deciding half on the host -- the function k_wta_select runs per pixel (kernels_path.h:
 *   wta_select_words), over n raw records of four words each; writes the two words of k_wta_t's record per pixel.  An error
 *   code for D outside {128, 256} or uniquenessRatio outside 0 .. 99. */
#ifdef __cplusplus
extern "C" {
#endif
int sgm_debug_uniq_threshold(int minS, int uniquenessRatio);
int sgm_debug_wta_split(const sgm_params *p, int H, int W, int schedule, int sweep_rows, int debug, int confidence, int right_view,
                        int keep_aggr);
long long sgm_debug_wta_raw_bytes(const sgm_engine *e);
int sgm_debug_wta_select_n(int D, int uniquenessRatio, const uint32_t *raw /* n x 4 */, int n, uint32_t *wta /* n x 2 */);
#ifdef __cplusplus
}
#endif

#endif
