// sgm_engine.hip -- host side of the C ABI declared in include/sgm_hip.h.
//
// Owns the device buffers and the stage schedule of one stereo matcher on one GPU / stream.
// Mirrors the reference's call shape (cv2.StereoSGBM_create -> .compute -> reprojectImageTo3D,
// /root/reference/main.ipynb:655-670, 697); see the header for the per-entry-point mapping.
#include "../../include/sgm_hip.h"
#include "sgm_debug.h"

#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "kernels_cost.h"
#include "kernels_census.h"
#include "kernels_path.h"
#include "kernels_post.h"
#include "kernels_rectify.h"
#include "kernels_sweep.h"
#include "kernels_group.h"
#include "kernels_right.h"
#include "kernels_wls.h"
#include "kernels_lrc.h"
#include "kernels_voxel.h"
#include "kernels_radius.h"
#include "kernels_statistical.h"
#include "kernels_covariance.h"
#include "kernels_dbscan.h"
#include "kernels_plane.h"
#include "kernels_icp.h"
#include "kernels_tsdf.h"
#include "kernels_mesh.h"
#include "kernels_normals.h"

using namespace sgm;

// ---- error plumbing ----------------------------------------------------------------------
static thread_local char g_err[512] = "";

static int set_err(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess)                                                                      \
            return set_err(SGM_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),     \
                           __FILE__, __LINE__);                                                    \
    } while (0)

// ---- engine --------------------------------------------------------------------------------
// Guarded allocation mode (environment SGM_DEBUG_ALLOC=1, read once per process; tests/test_gpu_guard.py runs parity
// cases under it in a child process).  Every device buffer of an engine is then placed through the HIP virtual-memory
// calls so that
//   * it ENDS exactly at the end of its mapping (sizes that are no multiple of 16 bytes: up to 15 bytes earlier) and the
//     pages behind -- and in front of -- the mapping are reserved but never mapped: a read or write past the buffer is a
//     GPU memory access fault at once instead of a silent touch of a neighbouring allocation.  Scalar loads (k_pix's
//     left-pixel records) and flat / global accesses carry no bounds check, unlike the buffer-descriptor accesses;
//   * the low half of every address inside the buffer has bit 31 SET: a 64-bit pointer put together from two 32-bit
//     halves with a signed low half (the int that __builtin_amdgcn_readfirstlane returns) turns into 0xffffffff'xxxxxxxx
//     there -- the cause of round 3's memory access fault, DESIGN.md 4.6 -- while hipMalloc hands out such addresses
//     only now and then.
// Buffers above 1 GiB keep plain hipMalloc (the tests that use the mode run small frames).
static int debug_alloc_mode()
{
    static const int m = [] {
        const char *s = getenv("SGM_DEBUG_ALLOC");
        return s ? atoi(s) : 0;
    }();
    return m;
}

// Poison switch (csrc/sgm_debug.h: SGM_OPT_POISON; test scaffolding).  -1: not armed.  0..255: armed -- every buffer that
// DevBuf::ensure allocates or regrows is filled with this byte before anything can use it, so that growth does not bring
// hipMalloc's friendly contents back between two poisoned calls.  One word per process, like SGM_DEBUG_ALLOC: ensure() has
// no engine to ask, and the internal engines of the batch entries are created in the middle of a call.
static int g_poison_byte = -1;

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    // guarded mode only: the address range reserved, the part of it that is mapped, the physical allocation
    void *va = nullptr, *map = nullptr;
    size_t va_bytes = 0, map_bytes = 0;
    hipMemGenericAllocationHandle_t handle{};
    bool guarded = false;

    int ensure_guarded(size_t bytes)
    {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return set_err(SGM_ERR_HIP, "hipGetDevice failed");
        hipMemAllocationProp prop{};
        prop.type = hipMemAllocationTypePinned;
        prop.location.type = hipMemLocationTypeDevice;
        prop.location.id = dev;
        size_t gran = 0;
        if (hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityMinimum) != hipSuccess || gran == 0)
            return set_err(SGM_ERR_HIP, "SGM_DEBUG_ALLOC: hipMemGetAllocationGranularity failed");
        const size_t G4 = (size_t)1 << 32;
        const size_t mb = (bytes + gran - 1) / gran * gran;   // mapped bytes: whole granules
        // room for a 4 GiB boundary with the mapping right below it and one unmapped granule on either side
        const size_t vb = mb + G4 + 2 * gran;
        void *r = nullptr;
        if (hipMemAddressReserve(&r, vb, gran, nullptr, 0) != hipSuccess)
            return set_err(SGM_ERR_NOMEM, "SGM_DEBUG_ALLOC: hipMemAddressReserve(%zu) failed", vb);
        const uintptr_t r0 = (uintptr_t)r;
        const uintptr_t m1 = (r0 + gran + mb + G4 - 1) / G4 * G4;   // first 4 GiB boundary with room for guard + mapping below it
        const uintptr_t m0 = m1 - mb;                               // low halves of [m0, m1): [2^32 - mb, 2^32), bit 31 set (mb <= 2 GiB)
        hipMemGenericAllocationHandle_t h{};
        if (m0 < r0 + gran || m1 + gran > r0 + vb || hipMemCreate(&h, mb, &prop, 0) != hipSuccess) {
            (void)hipMemAddressFree(r, vb);
            return set_err(SGM_ERR_NOMEM, "SGM_DEBUG_ALLOC: hipMemCreate(%zu) failed", mb);
        }
        hipMemAccessDesc acc{};
        acc.location = prop.location;
        acc.flags = hipMemAccessFlagsProtReadWrite;
        if (hipMemMap((void *)m0, mb, 0, h, 0) != hipSuccess || hipMemSetAccess((void *)m0, mb, &acc, 1) != hipSuccess) {
            (void)hipMemRelease(h);
            (void)hipMemAddressFree(r, vb);
            return set_err(SGM_ERR_HIP, "SGM_DEBUG_ALLOC: hipMemMap / hipMemSetAccess failed");
        }
        va = r;
        va_bytes = vb;
        map = (void *)m0;
        map_bytes = mb;
        handle = h;
        guarded = true;
        p = (void *)((m1 - bytes) & ~(uintptr_t)15);   // the buffer ends where the mapping ends (16-byte aligned start)
        cap = bytes;
        return SGM_OK;
    }
    int ensure(size_t bytes)
    {
        if (bytes <= cap) return SGM_OK;
        if (p) {
            if (release() != hipSuccess) return SGM_ERR_HIP;
        }
        if (debug_alloc_mode() && bytes <= ((size_t)1 << 30)) {
            int rc = ensure_guarded(bytes);
            return rc ? rc : poison_new();
        }
        hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) {
            p = nullptr;
            set_err(SGM_ERR_NOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
            return SGM_ERR_NOMEM;
        }
        cap = bytes;
        return poison_new();
    }
    // armed poison switch only: [p, p + cap) filled and the fill complete before ensure() returns (the engine's streams are
    // non-blocking, so nothing orders them behind the null stream but the host)
    int poison_new()
    {
        if (g_poison_byte < 0) return SGM_OK;
        if (hipMemsetAsync(p, g_poison_byte, cap, nullptr) != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess)
            return set_err(SGM_ERR_HIP, "SGM_OPT_POISON: filling a new buffer of %zu bytes failed", cap);
        return SGM_OK;
    }
    hipError_t release()
    {
        hipError_t e = hipSuccess;
        if (guarded) {
            e = hipMemUnmap(map, map_bytes);
            (void)hipMemRelease(handle);
            (void)hipMemAddressFree(va, va_bytes);
            guarded = false;
            va = map = nullptr;
        } else if (p) {
            e = hipFree(p);
        }
        p = nullptr;
        cap = 0;
        return e;
    }
};

// page-locked host memory (staging of sgm_compute_batch): copies to / from it are truly asynchronous
struct HostBuf {
    void *p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes)
    {
        if (bytes <= cap) return SGM_OK;
        release();
        hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
        if (e != hipSuccess) {
            p = nullptr;
            set_err(SGM_ERR_NOMEM, "hipHostMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
            return SGM_ERR_NOMEM;
        }
        cap = bytes;
        return SGM_OK;
    }
    void release()
    {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
};

// The schedule of one compute (make_plan decides it; run_compute, ensure_plan_buffers and the batch entries follow it)
struct Plan {
    // cost stage
    bool byte_cost;        // per-pixel cost as bytes + k_box_u8 (else the int16 pipeline k_hsum + k_vsum*)
    bool pix_px;           // int16 pipeline: k_pix_px + k_hsum_px (D <= 32) in place of k_hsum
    int GWc, RBb;          // k_box_u8: lane-group width, rows per band
    bool vsum_ring, vsum_wide;  // int16 pipeline: k_vsum_ring (else the generic k_vsum), with 8 int16 per thread (else 4)
    int cn;                // channels of the images (SGM_OPT_CHANNELS), the CN of k_features / k_hsum: 3 always takes the int16 pipeline
    bool census;           // SGM_OPT_COST = SGM_COST_CENSUS: k_census + k_pix_census* in front of the box stages (byte_cost: k_box_u8,
                           // else k_hsum_u8 + k_vsum*); private: not part of sgm_debug_plan_t
    // path stage
    bool v1;               // schedule 0: one kernel per direction
    int GWs;               // lane-group width of the small-D kernels (64: none)
    bool rows4;            // small-D schedule (D <= 64 outside throughput mode, D <= 32 always)
    bool chain;            // chained sweeps (schedule 2)
    int npass, R, nbands;
    bool axis;             // MODE_HH4: the path set is the four axis-aligned directions -- two passes of the axis-only kernels
    int nroles;            // roles per pixel of the band record: 3, or 1 (axis)
    bool prepass_g;        // pre-pass: lane-grouped lines (k_prepass3_g), or three roles per wave (k_prepass3) in pre_nch
    bool fused_prepass;    // chunks of pre_rows rows (pre_plain: the plain layout), or the single-direction kernel
    bool pre_plain;
    int pre_nch, pre_rows;
    bool overlap, fork_early;  // MODE_HH: upward pre-pass on the auxiliary stream; forked right after the cost stage
    // winner-take-all
    bool fused_wta;        // inside the last path kernel (else k_wta_t)
    bool wta_split;        // (never with fused_wta) the chained second sweep leaves raw records instead of S (SWEEP_REDUCE), the
                           // wta stage is k_wta_select; private: not part of sgm_debug_plan_t
    int nvol;              // volumes k_wta_t adds up: 1 (S), 2 (+ the fifth path's), 3 (+ the other in-row path's), 5 (k_paths5_g),
                           // 4 (k_axis_paths4_g: MODE_HH4 in the small-D schedule)
    bool path_w_main, path_w_lines;  // MODE_SGBM's fifth path on the main stream behind the sweeps; as the general line kernel
    bool speckle;          // the speckle filter runs
};

// Every device buffer an engine owns, ONCE: BUF(name) a member of the engine, ARR(name, dims) a two-dimensional array member,
// MAP(name) a member of SideMap, which the engine holds twice (conf.name, right.name).  The list expands to the member
// declarations and to the walk over all of them (each_devbuf) behind release_buffers, poison_buffers and plan_bytes_held: a
// buffer added here is released, poisoned and counted; tests/test_history_walks.py refuses a DevBuf declared anywhere else.
#define SGM_ENGINE_DEVBUFS(BUF, ARR, MAP) \
    BUF(in_left) BUF(in_right)                   /* staging for host-pointer calls */ \
    BUF(lrec) BUF(rplanes)                       /* features (census: the 64-bit descriptors of the left / the mirrored right image) */ \
    BUF(hsum) BUF(cost) BUF(aggr)                /* int16 [H][W1][D] volumes */ \
    BUF(aggr2) BUF(aggr3)                        /* MODE_SGBM: the fifth path's own volume (D <= 128; added to S by the winner-take-all), the other in-row path's (D <= 64) */ \
    BUF(aggr4) BUF(aggr5)                        /* MODE_SGBM, D <= 64: the volumes of the vertical and the second diagonal direction (k_paths5_g) */ \
    BUF(wta)                                     /* uint2 [H][W] */ \
    BUF(wta_raw)                                 /* Plan::wta_split only: uint4 [H][W] raw records of the chained second sweep */ \
    BUF(bndL) BUF(bndL2)                         /* band-boundary state of the sweep pre-pass (down / up) */ \
    BUF(pstate) BUF(pstate2)                     /* line state between the row chunks of the pre-pass (ping-pong, down / up) */ \
    BUF(disp_raw) BUF(disp_med) BUF(disp_out)    /* int16 [H][W] */ \
    MAP(raw) MAP(fin)                            /* [H][W], option on only.  conf: uint8, the margin of the winner-take-all; masked by the final map.  right: int16 */ \
    BUF(rrec)                                    /* SGM_OPT_RIGHT_VIEW only: uint2 [H][W1] record of the diagonal winner-take-all */ \
    BUF(label) BUF(csize) BUF(rlen)              /* int32 [H][W] each */ \
    BUF(f32) BUF(xyz) BUF(mask) BUF(minkey)      /* host-pointer post stages */ \
    BUF(rmap1) BUF(rmap2) BUF(rsrc) BUF(rdst)    /* host-pointer rectification stages */ \
    BUF(ccount) BUF(cpts) BUF(crgb) BUF(crgb_in) /* point compaction */ \
    BUF(wls_u) BUF(wls_v) BUF(wls_c)             /* sgm_wls_filter: float [H][W] planes u, v, c' (kernels_wls.h); sgm_trim releases these three by name */ \
    BUF(lrc_f)                                   /* sgm_lrc_confidence: uint8 [pairs of a chunk][2][H][W], the smoothness factors (kernels_lrc.h); sgm_trim releases it by name */ \
    BUF(vox_tab) BUF(vox_slot) BUF(vox_ctl) BUF(vox_cnt) /* sgm_voxel_downsample: the hash table (VoxSlot [capacity]), each point's slot (uint32 [n]), the call's control words, the host entry's staged counts (kernels_voxel.h); sgm_trim releases the first two by name */ \
    BUF(rad_tab) BUF(rad_sorted) BUF(rad_pt) BUF(rad_ctl) BUF(rad_keep) BUF(rad_cnt) BUF(rad_idx) /* sgm_radius_outlier: the hash table of cells (RadSlot [capacity]), the records sorted by cell (float4 [points in range]), each point's slot and rank (uint2 [n]), the call's control words, the keep bytes where the caller asks for none and the host entry's staged ones (uint8 [n]), its staged counts and indices (uint32 [n] each; kernels_radius.h); sgm_trim releases all but the control words by name */ \
    BUF(stat_mean) BUF(stat_sums)                /* sgm_statistical_outlier, beside the radius search's buffers it reuses: the host entry's staged means (float32 [n]) and the call's 64-bit sums m, A, B (kernels_statistical.h); sgm_trim releases the first by name */ \
    BUF(cov_nrm) BUF(cov_curv) BUF(cov_mom) BUF(cov_ctl) /* sgm_covariance_normals, beside the radius search's buffers it reuses: the host entry's staged normals (float32 [n][3]) and curvatures (float32 [n]), the staged moments where the solve is a kernel of its own (int64 [points in range][10]) and the call's two counts (kernels_covariance.h); sgm_trim releases the first three by name */ \
    BUF(db_parent) BUF(db_near) BUF(db_rank) BUF(db_ctl) BUF(db_lab) BUF(db_sizes) /* sgm_cluster_dbscan, beside the radius search's buffers it reuses: per point the union-find link (int32 [n]), the nearest core point (uint32 [n]) and the root's rank (uint32 [n]), the call's three counts, and the host entry's staged labels (int32 [n]) and sizes (uint32 [n]; kernels_dbscan.h); sgm_trim releases all but the counts by name */ \
    BUF(pl_pts) BUF(pl_hyp) BUF(pl_cnt) BUF(pl_ctl) BUF(pl_inl) BUF(pl_dist) /* sgm_segment_plane, sgm_plane_inliers: the valid points in source order (float4 [n]), the hypotheses (float4 [K]) and their counts (uint32 [K]), the call's control block, and the host entries' staged inlier bytes (uint8 [n]) and distances (float32 [n]; kernels_plane.h); the byte the compaction selects by is rad_keep, the staged rows are cpts, crgb and rad_idx; sgm_trim releases all but the control block by name */ \
    BUF(icp_corr) BUF(icp_d2) BUF(icp_part) BUF(icp_ctl) BUF(icp_txyz) BUF(icp_tdisp) BUF(icp_tnrm) /* sgm_register_icp, sgm_evaluate_registration, sgm_transform_points, beside the radius search's buffers they reuse for the target's grid: per source point the correspondence (int32 [ns]) and its squared distance (float32 [ns]), the blocks' partial sums (double [blocks of 256][28]), the result record and the counts of one evaluation, and the host entries' staged target points, disparities and normals (kernels_icp.h); the staged source is xyz and f32; sgm_trim releases all but the record by name */ \
    BUF(tsdf_sum) BUF(tsdf_w) BUF(tsdf_rgb) BUF(tsdf_cnt) BUF(tsdf_off) BUF(tsdf_ctl) /* sgm_tsdf_integrate, sgm_tsdf_extract_points: the host entries' staged planes (int32 [V], int32 [V], uint32 [3][V]), the extraction's counts per 1024 voxels (uint32 [blocks]) and their scanned offsets (uint64 [blocks + 1]), and the 256 copies of the eight counts of one integration (kernels_tsdf.h); the staged frame is xyz, f32 and crgb_in, the staged rows are cpts and crgb; sgm_trim releases all but the counts by name */ \
    BUF(mesh_code) BUF(mesh_num) BUF(mesh_fcnt) BUF(mesh_vcnt) BUF(mesh_faces) /* sgm_mesh_grid: a code byte per quad (uint8 [H][W]), the pixel -> vertex number map (uint32 [H][W]), the blocks' numbers of faces and of vertices (uint32 [blocks + 1] each), the host entry's staged faces (kernels_mesh.h); sgm_trim releases the first two and the last by name */ \
    BUF(mesh_nrm)                                /* sgm_normals_grid, sgm_mesh_grid_normals: the host entries' staged normals (float32 [H][W][3]; kernels_normals.h); sgm_trim releases it by name */ \
    BUF(headroom)                                /* uint32[2]: max C_true (incl. upstream's running-sum intermediate), max min_d L_r */ \
    BUF(chain_ctl) BUF(chain_err)                /* chained sweeps: ticket + progress words (zeroed before every launch); sticky give-up flag */ \
    ARR(io, [2][5])                              /* sgm_compute_batch, throughput mode: the transfer slots (sgm_engine says what they hold) */
#define SGM_DEVBUF_DECL(name) DevBuf name;
#define SGM_DEVBUF_DECL_ARR(name, dims) DevBuf name dims;
#define SGM_DEVBUF_NONE(...)
#define SGM_DEVBUF_VISIT(name) f(e->name);   // (these three: each_devbuf, its e and f)
#define SGM_DEVBUF_VISIT_ARR(name, dims) for (auto &row : e->name) for (auto &b : row) f(b);
#define SGM_DEVBUF_VISIT_MAP(name) f(e->conf.name); f(e->right.name);

// The optional per-pair map.  SGM_OPT_CONFIDENCE and SGM_OPT_RIGHT_VIEW are one mechanism: an option, two maps [H][W] (raw, and
// final behind the left map's epilogue), a tap on each, and a bind entry that sends the final maps of the next image call to
// the caller's memory.  The constants that differ come first; the kernels are stage_confidence / stage_right_view.
struct SideMap {
    const int bpp;                                                // bytes per pixel of either map
    const char *const opt_name, *const bind_name, *const noun;    // as the error texts spell them
    const int tap_raw, tap_fin;
    const char *const tap_fin_name;
    int on = 0;                // the option
    int last = 0;              // what the last compute on this engine left: 0 no maps, 1 raw + fin, 2 fin went to a bound pointer
    std::vector<void *> bind;  // the bind entry: where the next image call writes its pairs' final maps
    SGM_ENGINE_DEVBUFS(SGM_DEVBUF_NONE, SGM_DEVBUF_NONE, SGM_DEVBUF_DECL)
};

// The device pointers of one pair, as one value.  Null: no float map / no XYZ image; conf and rmap -- the engine's own buffer
// (SideMap::fin); disp_i16 -- in pipeline_one only -- the engine's disp_out.
struct PairIO { const void *left, *right; void *disp_i16, *disp_f32, *xyz_f32; uint8_t *conf; int16_t *rmap; };

struct sgm_engine {
    sgm_params params;
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipStream_t aux = nullptr;            // second stream: MODE_HH overlaps the upward pre-pass with the downward sweep
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipStream_t aux2 = nullptr;           // third stream (D <= 64, MODE_SGBM: the left-to-right in-row path beside everything else)
    hipEvent_t ev_join2 = nullptr;
    int keep_aggr = 0;
    bool no_wta_split = false;            // internal engines: the caller's engine keeps S (inherit_options), so the group's sweep stores it
    int profile = 0;
    int schedule = 1;    // 0: one kernel per direction (v1); 1: fused 4-direction sweeps; 2: chained sweeps, no pre-pass (throughput mode)
    int chain_wgs = 0;   // schedule 2: workgroups (= bands in flight) per sweep launch; 0 = automatic
    Plan plan{};         // what PH_PRE of the last compute decided (run_group checks it against the group's)
    int sweep_rows = 0;  // rows per band of the sweep (0 = automatic)
    int debug = 0;       // timing experiments (SweepArgs::dbg)
    int prepass_rows = 0;  // rows per chunk of the boundary pre-pass (0 = automatic, about 135, a multiple of 8)
    int cn = 1;          // SGM_OPT_CHANNELS: 1 or 3 interleaved 8-bit channels per image pixel
    int cost_fn = SGM_COST_BT;  // SGM_OPT_COST: the matching cost of every compute on the engine
    // SGM_OPT_CONFIDENCE: every compute also produces the uniqueness margin; SGM_OPT_RIGHT_VIEW: the right-view map
    SideMap conf{1, "SGM_OPT_CONFIDENCE", "sgm_bind_confidence_device", "confidence", SGM_TAP_CONF_RAW, SGM_TAP_CONF, "SGM_TAP_CONF"};
    SideMap right{2, "SGM_OPT_RIGHT_VIEW", "sgm_bind_right_device", "right-view", SGM_TAP_RIGHT_RAW, SGM_TAP_RIGHT, "SGM_TAP_RIGHT"};
    // sgm_compute_batch: up to three pairs in flight = this engine + two peers (own stream and device
    // buffers), each with page-locked staging buffers for the images and the disparity map
    sgm_engine *peer = nullptr, *peer2 = nullptr;
    std::vector<sgm_engine *> group;      // sgm_pipeline_batch_device: the other engines of a chained group (own streams and buffers)
    int last_group = 0;                   // engines of `group` the last batch call used (sgm_get_headroom looks at all of them)
    int last_peers = 0;                   // peers the last sgm_compute_batch in latency mode used (likewise)
    bool in_batch = false;                // a batch entry is running: the computes it starts on this engine keep last_group
    bool hr_accumulate = false;           // batch calls: the headroom record of this engine is NOT reset by the next compute (it then covers every pair the engine ran in the call)
    int group_max = 0;                    // SGM_OPT_GROUP_MAX: pairs per chained launch (0 = as many as fit in memory, up to CHAIN_MAX_FRAMES)
    // sgm_compute_batch, throughput mode: two groups in flight (the transfers of group g + 1 / g - 1 beside the kernels of
    // group g).  Each engine of a group keeps the device images of ITS pair twice -- slot g & 1: left, right, int16 map,
    // float map, XYZ -- with an event behind the upload and one behind the pair's last kernel; the engine the caller
    // holds owns the two copy streams.
    // (the slots themselves, DevBuf io[2][5], are declared by the list below)
    HostBuf pin_io[2][3];                 // page-locked staging of the slot's images (left, right) and of its int16 map
    // events of a slot: images uploaded / images consumed by the cost stage / last kernel of the pair done / map downloaded
    hipEvent_t ev_io_in[2] = {nullptr, nullptr}, ev_io_used[2] = {nullptr, nullptr}, ev_io_out[2] = {nullptr, nullptr},
               ev_io_dl[2] = {nullptr, nullptr};
    hipStream_t copy_in = nullptr, copy_out = nullptr;
    hipEvent_t ev_group = nullptr;
    HostBuf pin_left, pin_right, pin_disp;
    HostBuf pin_icp;                      // sgm_register_icp: the 232-byte result record and the three counts of one evaluation
    hipEvent_t ev_done = nullptr;

    // shape of the last compute
    int H = 0, W = 0;
    Geom g{};

    // device buffers: the list above, each entry once
    SGM_ENGINE_DEVBUFS(SGM_DEVBUF_DECL, SGM_DEVBUF_DECL_ARR, SGM_DEVBUF_NONE)

    // profiling
    std::vector<hipEvent_t> events;
    std::vector<const char *> stage_names;
    std::vector<int> stage_launches;
    std::vector<uint64_t> stage_range;   // roctx range ids of the open stages
    int nstages = 0;
    int nevents = 0;                      // events of the pool used by this compute
    std::vector<int> stage_ev;            // [2 i], [2 i + 1]: begin / end event of stage i (indices into `events`)
    int last_end_ev = -1;                 // end event of the stage that was closed last, and its stream
    hipStream_t last_end_stream = nullptr;
};

// f(DevBuf &) for every device buffer of e (an engine, or a const one), in the order of the list
template <class E, class F>
static void each_devbuf(E *e, F f)
{
    SGM_ENGINE_DEVBUFS(SGM_DEVBUF_VISIT, SGM_DEVBUF_VISIT_ARR, SGM_DEVBUF_VISIT_MAP)
}

static int normalise(const sgm_params *p, int H, int W, Geom *g)
{
    if (p->numDisparities <= 0) return set_err(SGM_ERR_INVALID_ARG, "numDisparities must be > 0");
    if (p->mode != 0 && p->mode != 1 && p->mode != 3)
        return set_err(SGM_ERR_UNSUPPORTED, "mode %d: MODE_SGBM (0), MODE_HH (1) and MODE_HH4 (3) are built; MODE_SGBM_3WAY (2) is not", p->mode);
    if (p->numDisparities % 16 != 0)
        return set_err(SGM_ERR_UNSUPPORTED, "numDisparities=%d must be divisible by 16 (OpenCV's documented contract)", p->numDisparities);
    if (p->numDisparities > 1024) return set_err(SGM_ERR_UNSUPPORTED, "numDisparities=%d > 1024", p->numDisparities);
    const int dim = p->blockSize > 0 ? p->blockSize : 5;
    if (dim > 31) return set_err(SGM_ERR_UNSUPPORTED, "blockSize=%d > 31", dim);
    g->H = H;
    g->W = W;
    g->minD = p->minDisparity;
    g->D = p->numDisparities;
    const int maxD = g->minD + g->D;
    g->minX1 = std::max(maxD, 0);
    const int maxX1 = W + std::min(g->minD, 0);
    g->W1 = maxX1 - g->minX1;
    g->SW2 = g->SH2 = dim / 2;
    g->P1 = p->P1 > 0 ? p->P1 : 2;
    g->P2 = std::max(p->P2 > 0 ? p->P2 : 5, g->P1 + 1);
    g->uniq = p->uniquenessRatio >= 0 ? p->uniquenessRatio : 10;
    g->d12 = p->disp12MaxDiff > 0 ? p->disp12MaxDiff : 1;
    g->ftzero = std::max(p->preFilterCap, 15) | 1;
    g->invalid_scaled = (g->minD - 1) * 16;
    g->mode = p->mode;
    g->NP = g->D <= 128 ? 1 : (g->D <= 256 ? 2 : (g->D <= 512 ? 4 : 8));
    g->rowsz = (int64_t)std::max(g->W1, 0) * g->D;
    g->hr = nullptr;
    return SGM_OK;
}

// ---- stage bookkeeping -----------------------------------------------------------------------
// roctx ranges around every stage while SGM_OPT_PROFILE is on (named ranges in rocprofv3
// --marker-trace timelines; they bracket the host-side enqueue of the stage).  The tracing library
// is looked up at run time: no link-time dependency, silently absent when it is not installed.
struct Roctx {
    uint64_t (*start)(const char *) = nullptr;
    void (*stop)(uint64_t) = nullptr;
    Roctx()
    {
        for (const char *lib : {"librocprofiler-sdk-roctx.so", "libroctx64.so"}) {
            if (void *h = dlopen(lib, RTLD_NOW | RTLD_LOCAL)) {
                start = (uint64_t(*)(const char *))dlsym(h, "roctxRangeStartA");
                stop = (void (*)(uint64_t))dlsym(h, "roctxRangeStop");
                if (start && stop) return;
                start = nullptr;
                stop = nullptr;
            }
        }
    }
};
static Roctx &roctx()
{
    static Roctx r;
    return r;
}

// Stage brackets (SGM_OPT_PROFILE).  An event record is a marker packet that the next kernel of the stream
// waits for; two of them between every pair of stages cost a 720p frame 13 % (10-18 us per stage boundary
// on the rocprof timeline).  So a stage that begins right where the previous stage of the same stream
// ended -- nothing enqueued in between -- takes that stage's end event as its begin: one record per boundary.
static int new_stage_event(sgm_engine *e, hipStream_t on, int *idx)
{
    if ((size_t)e->nevents == e->events.size()) {
        hipEvent_t ev;
        HIP_TRY(hipEventCreate(&ev));
        e->events.push_back(ev);
    }
    *idx = e->nevents++;
    HIP_TRY(hipEventRecord(e->events[*idx], on));
    return SGM_OK;
}
static int stage_begin(sgm_engine *e, const char *name, hipStream_t on = nullptr)
{
    if (!e->profile) return SGM_OK;
    hipStream_t st = on ? on : e->stream;
    const size_t i = (size_t)e->nstages;
    e->stage_range.resize(i + 1);
    if (roctx().start) e->stage_range[i] = roctx().start(name);
    e->stage_names.resize(i + 1);
    e->stage_launches.resize(i + 1);
    e->stage_ev.resize(2 * (i + 1));
    e->stage_names[i] = name;
    e->stage_launches[i] = 0;
    if (e->last_end_ev >= 0 && e->last_end_stream == st) {
        e->stage_ev[2 * i] = e->last_end_ev;
    } else {
        int rc = new_stage_event(e, st, &e->stage_ev[2 * i]);
        if (rc) return rc;
    }
    return SGM_OK;
}
static int stage_end(sgm_engine *e, int launches, hipStream_t on = nullptr)
{
    if (!e->profile) return SGM_OK;
    hipStream_t st = on ? on : e->stream;
    const size_t i = (size_t)e->nstages;
    e->stage_launches[i] = launches;
    int rc = new_stage_event(e, st, &e->stage_ev[2 * i + 1]);
    if (rc) return rc;
    e->last_end_ev = e->stage_ev[2 * i + 1];
    e->last_end_stream = st;
    if (roctx().stop) roctx().stop(e->stage_range[i]);
    e->nstages++;
    return SGM_OK;
}
// something other than a stage was enqueued (a wait for another stream, a memset ...): the next stage needs a begin event of its own
static void stage_break(sgm_engine *e) { e->last_end_ev = -1; }
// a call takes the stage record over: stage_times reports this call's stages from here on
static void stage_reset(sgm_engine *e)
{
    e->nstages = 0;
    e->nevents = 0;
    e->last_end_ev = -1;
}

#define KCHECK() HIP_TRY(hipGetLastError())

// ---- template ladders --------------------------------------------------------------------------
// f(NP, PARTIAL) as std::integral_constant for the geometry: NP 128-disparity pieces per lane, PARTIAL = the last piece is not full
// NP = 1, 2, 4 only.  D > 512 (NP = 8) never comes here: its plan (make_plan: wide_d) runs two kernel templates -- k_path
// and k_hsum (gray and colour) -- and those go through with_np_wide; a fourth rung HERE would instantiate every sweep,
// pre-pass and lane-group kernel for a packing their registers and LDS do not hold.
static bool np_partial(const Geom &g) { return g.D != 128 * g.NP; }
template <class F>
static auto with_np(const Geom &g, F &&f)
{
    using std::integral_constant;
    const bool partial = np_partial(g);
    if (g.NP == 1) return partial ? f(integral_constant<int, 1>(), std::true_type()) : f(integral_constant<int, 1>(), std::false_type());
    if (g.NP == 2) return partial ? f(integral_constant<int, 2>(), std::true_type()) : f(integral_constant<int, 2>(), std::false_type());
    return partial ? f(integral_constant<int, 4>(), std::true_type()) : f(integral_constant<int, 4>(), std::false_type());
}
// with_np plus the NP = 8 rung, for the kernels that have that instantiation
template <class F>
static auto with_np_wide(const Geom &g, F &&f)
{
    using std::integral_constant;
    if (g.NP == 8) return np_partial(g) ? f(integral_constant<int, 8>(), std::true_type()) : f(integral_constant<int, 8>(), std::false_type());
    return with_np(g, f);
}
// f(GW, PARTIAL) for a lane-group width of the small-D kernels (8, 16, 32); PARTIAL = the group is not full (D = 48 in
// groups of 32; D = 16, 32, 64 fill theirs)
template <class F>
static auto with_gw(int GW, int D, F &&f)
{
    using std::integral_constant;
    if (GW == 8) return f(integral_constant<int, 8>(), std::false_type());
    if (GW == 16) return f(integral_constant<int, 16>(), std::false_type());
    return D < 64 ? f(integral_constant<int, 32>(), std::true_type()) : f(integral_constant<int, 32>(), std::false_type());
}
// f(R) for a window radius 1 .. 5 (the instantiations of the box kernels); nothing for any other radius
template <class F>
static void with_radius(int r, F &&f)
{
    using std::integral_constant;
    switch (r) {
    case 1: f(integral_constant<int, 1>()); break;
    case 2: f(integral_constant<int, 2>()); break;
    case 3: f(integral_constant<int, 3>()); break;
    case 4: f(integral_constant<int, 4>()); break;
    case 5: f(integral_constant<int, 5>()); break;
    default: break;
    }
}

// ---- path launch dispatch ---------------------------------------------------------------------
template <int NP, bool PARTIAL>
static void launch_path_np(const Geom &g, int rx, int ry, int mode, const int16_t *C, int16_t *S, int keepS,
                           uint2 *wta, Boundary bd, hipStream_t st)
{
    const int nlines = ry == 0 ? g.H : g.W1;
    dim3 grid(nlines, mode == PATH_BOUNDARY ? 3 : 1), block(64);
    const bool posw = g.uniq < 100;  // positive uniqueness weight: the WTA variant without products
    if (mode == PATH_FIRST)
        hipLaunchKernelGGL((k_path<NP, PARTIAL, PATH_FIRST, true>), grid, block, 0, st, g, rx, ry, C, S, keepS, wta, bd);
    else if (mode == PATH_ACCUM)
        hipLaunchKernelGGL((k_path<NP, PARTIAL, PATH_ACCUM, true>), grid, block, 0, st, g, rx, ry, C, S, keepS, wta, bd);
    else if (mode == PATH_LAST && posw)
        hipLaunchKernelGGL((k_path<NP, PARTIAL, PATH_LAST, true>), grid, block, 0, st, g, rx, ry, C, S, keepS, wta, bd);
    else if (mode == PATH_LAST)
        hipLaunchKernelGGL((k_path<NP, PARTIAL, PATH_LAST, false>), grid, block, 0, st, g, rx, ry, C, S, keepS, wta, bd);
    else if constexpr (NP < 8)  // (the boundary role belongs to the fused sweeps' pre-pass: D <= 512)
        hipLaunchKernelGGL((k_path<NP, PARTIAL, PATH_BOUNDARY, true>), grid, block, 0, st, g, rx, ry, C, S, keepS, wta, bd);
}

static void launch_path(const Geom &g, int rx, int ry, int mode, const int16_t *C, int16_t *S, int keepS,
                        uint2 *wta, hipStream_t st, Boundary bd = Boundary{nullptr, 1, 0})
{
    with_np_wide(g, [&](auto np, auto part) { launch_path_np<np, part>(g, rx, ry, mode, C, S, keepS, wta, bd, st); });
}

// ---- sweep launch dispatch --------------------------------------------------------------------
// ---- small D: lane-grouped kernels (kernels_group.h) ----
static int group_width(const Geom &g, int H)
{
    if (g.D > 64 || (int64_t)H * g.rowsz * 2 >= (int64_t)0x7fff0000) return 64;
    return g.D <= 16 ? 8 : (g.D <= 32 ? 16 : 32);
}
template <int GW, int NP, bool PARTIAL>
static void launch_rows_g(const Geom &g, int H, int rx, int mode, const int16_t *C, int16_t *S, int keepS, uint2 *wta, hipStream_t st)
{
    constexpr int G = 64 / GW;
    dim3 grid((H + G - 1) / G), block(64);
    if (mode == PATH_FIRST)
        hipLaunchKernelGGL((k_rows_g<GW, NP, PARTIAL, PATH_FIRST, true>), grid, block, 0, st, g, rx, C, S, keepS, wta);
    else if (mode == PATH_ACCUM)
        hipLaunchKernelGGL((k_rows_g<GW, NP, PARTIAL, PATH_ACCUM, true>), grid, block, 0, st, g, rx, C, S, keepS, wta);
    else if (g.uniq < 100)
        hipLaunchKernelGGL((k_rows_g<GW, NP, PARTIAL, PATH_LAST, true>), grid, block, 0, st, g, rx, C, S, keepS, wta);
    else
        hipLaunchKernelGGL((k_rows_g<GW, NP, PARTIAL, PATH_LAST, false>), grid, block, 0, st, g, rx, C, S, keepS, wta);
}
// the in-row path of a pass (rows are independent): GW < 64 packs 64/GW rows into a wave
static void launch_rows_grouped(const Geom &g, int H, int GW, int rx, int mode, const int16_t *C, int16_t *S, int keepS, uint2 *wta, hipStream_t st)
{
    auto go = [&](auto gw, auto np, auto part) { launch_rows_g<gw, np, part>(g, H, rx, mode, C, S, keepS, wta, st); };
    if (GW < 64) with_gw(GW, g.D, [&](auto gw, auto part) { go(gw, std::integral_constant<int, 1>(), part); });
    else with_np(g, [&](auto np, auto part) { go(std::integral_constant<int, 64>(), np, part); });
}

template <int NP, bool PARTIAL, int MODE, bool POSW>
static int launch_sweep_one(const Geom &g, const SweepArgs &a, int nbands, hipStream_t st)
{
    const size_t lds = sweep_lds_bytes(NP, a.R);
    HIP_TRY(hipFuncSetAttribute((const void *)k_sweep<NP, PARTIAL, MODE, POSW>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((k_sweep<NP, PARTIAL, MODE, POSW>), dim3(nbands), dim3((a.R + 1) * 64), lds, st, g, a);
    return SGM_OK;
}
template <int NP, bool PARTIAL>
static int launch_sweep_np(const Geom &g, const SweepArgs &a, int mode, int nbands, hipStream_t st)
{
    if (mode == SWEEP_FIRST) return launch_sweep_one<NP, PARTIAL, SWEEP_FIRST, true>(g, a, nbands, st);
    if (mode == SWEEP_ACCUM) return launch_sweep_one<NP, PARTIAL, SWEEP_ACCUM, true>(g, a, nbands, st);
    if (g.uniq < 100) return launch_sweep_one<NP, PARTIAL, SWEEP_LAST, true>(g, a, nbands, st);
    return launch_sweep_one<NP, PARTIAL, SWEEP_LAST, false>(g, a, nbands, st);
}
// axis-only sweeps (MODE_HH4; kernels_sweep.h: k_axis_sweep, k_axis_chain): one role in the rings and in the record
template <int NP, bool PARTIAL, int MODE>
static int launch_axis_sweep_one(const Geom &g, const SweepArgs &a, int nbands, hipStream_t st)
{
    const size_t lds = sweep_lds_bytes(NP, a.R, 1);
    HIP_TRY(hipFuncSetAttribute((const void *)k_axis_sweep<NP, PARTIAL, MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((k_axis_sweep<NP, PARTIAL, MODE>), dim3(nbands), dim3((a.R + 1) * 64), lds, st, g, a);
    return SGM_OK;
}
template <int NP, bool PARTIAL, int MODE>
static int launch_axis_chain_one(const Geom &g, const SweepArgs &a, const ChainFrames &fr, int wgs, hipStream_t st)
{
    const size_t lds = sweep_lds_bytes(NP, a.R, 1) + 16;  // + the ticket word
    HIP_TRY(hipFuncSetAttribute((const void *)k_axis_chain<NP, PARTIAL, MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((k_axis_chain<NP, PARTIAL, MODE>), dim3(wgs), dim3((a.R + 2) * 64), lds, st, g, a, fr);
    return SGM_OK;
}
// the sweep kernels take the direction of the walk from the pass (kernels_sweep.h: XD): the first pass runs top-down and left
// to right, every other pass the other way round
static int check_sweep_direction(const SweepArgs &a, int mode)
{
    if ((mode == SWEEP_FIRST) != (a.xdir > 0) || a.xdir != a.ydir)
        return set_err(SGM_ERR_INVALID_ARG, "internal: sweep mode %d with direction (%d, %d)", mode, a.xdir, a.ydir);
    return SGM_OK;
}
static int launch_sweep(const Geom &g, const SweepArgs &a, int mode, int nbands, hipStream_t st, bool axis = false)
{
    if (int rc = check_sweep_direction(a, mode)) return rc;
    if (axis) {
        if (mode == SWEEP_LAST) return set_err(SGM_ERR_INVALID_ARG, "internal: the axis-only sweeps have no fused winner-take-all");
        return with_np(g, [&](auto np, auto part) {
            return mode == SWEEP_FIRST ? launch_axis_sweep_one<np, part, SWEEP_FIRST>(g, a, nbands, st)
                                       : launch_axis_sweep_one<np, part, SWEEP_ACCUM>(g, a, nbands, st);
        });
    }
    return with_np(g, [&](auto np, auto part) { return launch_sweep_np<np, part>(g, a, mode, nbands, st); });
}

// chained sweep (kernels_sweep.h: k_sweep_chain): `wgs` persistent workgroups of R compute waves + loader + publisher
template <int NP, bool PARTIAL, int MODE>
static int launch_chain_one(const Geom &g, const SweepArgs &a, const ChainFrames &fr, int wgs, hipStream_t st)
{
    const size_t lds = sweep_lds_bytes(NP, a.R) + 16;  // + the ticket word
    HIP_TRY(hipFuncSetAttribute((const void *)k_sweep_chain<NP, PARTIAL, MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((k_sweep_chain<NP, PARTIAL, MODE>), dim3(wgs), dim3((a.R + 2) * 64), lds, st, g, a, fr);
    return SGM_OK;
}
template <int NP, bool PARTIAL>
static int launch_chain_np(const Geom &g, const SweepArgs &a, const ChainFrames &fr, int mode, int wgs, hipStream_t st)
{
    if (mode == SWEEP_FIRST) return launch_chain_one<NP, PARTIAL, SWEEP_FIRST>(g, a, fr, wgs, st);
    // (SWEEP_REDUCE: full waves of NP = 1, 2 -- make_plan sets Plan::wta_split for nothing else)
    if constexpr (!PARTIAL && NP <= 2)
        if (mode == SWEEP_REDUCE) return launch_chain_one<NP, PARTIAL, SWEEP_REDUCE>(g, a, fr, wgs, st);
    if (mode == SWEEP_REDUCE) return set_err(SGM_ERR_INVALID_ARG, "internal: no SWEEP_REDUCE form of this chained sweep");
    return launch_chain_one<NP, PARTIAL, SWEEP_ACCUM>(g, a, fr, wgs, st);
}
static int launch_chain(const Geom &g, const SweepArgs &a, const ChainFrames &fr, int mode, int wgs, hipStream_t st, bool axis = false)
{
    if (int rc = check_sweep_direction(a, mode)) return rc;
    if (axis && mode == SWEEP_REDUCE) return set_err(SGM_ERR_INVALID_ARG, "internal: the axis-only sweeps have no SWEEP_REDUCE form");
    if (axis)
        return with_np(g, [&](auto np, auto part) {
            return mode == SWEEP_FIRST ? launch_axis_chain_one<np, part, SWEEP_FIRST>(g, a, fr, wgs, st)
                                       : launch_axis_chain_one<np, part, SWEEP_ACCUM>(g, a, fr, wgs, st);
        });
    return with_np(g, [&](auto np, auto part) { return launch_chain_np<np, part>(g, a, fr, mode, wgs, st); });
}
// workgroups of a chained launch over nf frames: a band trails the band above by about 2 (R - 1) + 17 lockstep steps and
// lasts T steps, so a frame keeps about T / lag workgroups busy; more would only wait (and hold CUs)
static int chain_window(const Geom &g, int R, int nbands, int nf, int override_wgs)
{
    const int pps = sweep_pps(g.NP);
    const int T = (g.W1 + pps - 1) / pps + 2 * (R - 1), lag = 2 * (R - 1) + 17;
    const int per_frame = override_wgs > 0 ? override_wgs : std::max(4, (T + lag - 1) / lag);
    return (int)std::min<int64_t>({(int64_t)per_frame * nf, (int64_t)nbands * nf, 256});
}

// rows per band: about 240 bands (one workgroup per CU, most of the 256 CUs busy), bounded by
// SWEEP_MAX_ROWS (register budget of the workgroup) and the 160 KiB of LDS.  MODE_HH: about 200 bands --
// a band's step time is set by its busiest SIMD (3 waves with 9 rows + loader as with 11 + loader), so
// taller bands cost the sweep nothing, write and read 18 % less boundary state and leave more CUs to the
// upward pre-pass that runs beside the downward sweep (4K: 11.05 -> 10.9 ms; MODE_SGBM: no gain).
// Chained schedule: bands are not tied to the number of CUs (a window of workgroups slides over them), so the tallest
// band the workgroup can hold: 12 rows = three compute waves on every SIMD, and the least hand-off traffic (3 / R volumes).
static int sweep_rows_for(const Geom &g, int override_rows, int npass, bool chained = false)
{
    int maxR = chained ? CHAIN_MAX_ROWS : SWEEP_MAX_ROWS;
    while (maxR > 1 && sweep_lds_bytes(g.NP, maxR) + 16 > 160 * 1024) maxR--;
    if (chained && override_rows <= 0) return std::max(1, std::min(maxR, g.H));
    const int bands = npass == 2 ? 200 : 240;
    int R = override_rows > 0 ? override_rows : (g.H + bands - 1) / bands;
    if (override_rows <= 0) R = std::max(R, 4);
    return std::max(1, std::min(R, maxR));
}

// columns per workgroup of k_box_u8: 4 waves x (64 / GW groups) x 4 columns
static int box_columns(int GW) { return 16 * (64 / GW); }

// ---- the schedule of one compute, decided from the geometry and the engine's options alone ----------------
// (run_compute follows it; the batch entries read it BEFORE anything is allocated or enqueued: whether a configuration
// runs chained, and what a pair costs in device memory).  Every A/B switch of sgm_debug.h that picks a schedule is read
// here; the sweep kernels see the mask itself (SweepArgs::dbg).
static Plan make_plan(const sgm_engine *e, const Geom &g, int H)
{
    const int dbg = e->debug;
    Plan p;
    // Byte pipeline (default): k_pix writes the per-pixel cost as uint8, k_box_u8 does the whole box
    // filter from it.  Needs a window radius 1..5 (instantiations), a cost that fits a byte, and a
    // pix volume below the 2 GiB a buffer descriptor spans here.  D <= 64: k_box_u8 in lane groups (several columns'
    // disparities side by side in a wave); the per-pixel cost comes from k_pix_px (D <= 32, one thread per pixel) or
    // k_pix (D = 48, 64: half its lanes idle, still less than the int16 pipeline's 3 V more traffic).
    // debug 256: the int16 pipeline always; debug 4 (no lane groups): the int16 pipeline for D <= 64.
    // Colour pairs (cn = 3) take the int16 pipeline: their per-pixel cost (up to 3 * (min(2 * ftzero, 255) + 63)) does not
    // fit a byte.  A gray pixel cost is at most min(2 * ftzero, 255) + 63 (the prefilter values are bytes, k_features), so
    // 2 * ftzero + 63 <= 255 below is the exact bound for ftzero <= 96 and keeps every larger ftzero off the byte volumes.
    // Census (SGM_OPT_COST; gray pairs only, census_refused): the per-pixel cost is a Hamming distance of 62 bits, a byte
    // whatever preFilterCap says -- the ftzero bound falls away, the others stay.
    p.cn = e->cn;
    p.census = e->cost_fn == SGM_COST_CENSUS;
    p.byte_cost = p.cn == 1 && !(dbg & SGM_DBG_INT16_COST) && (g.D > 64 || !(dbg & SGM_DBG_NO_LANE_GROUPS)) && g.SW2 >= 1 && g.SW2 <= 5 &&
                  g.SH2 == g.SW2 && (p.census || 2 * g.ftzero + 63 <= 255) && (int64_t)H * g.rowsz < (int64_t)0x7ff00000;
    // int16 pipeline, D <= 32: one thread per pixel (lanes spanning D would mostly idle; at D = 64 the wave-per-
    // chunk kernel is still ahead); the byte volume borrows the S buffer, unused before the paths
    // (census: not read -- its int16 pipeline is always the byte costs + k_hsum_u8, at every D)
    p.pix_px = p.cn == 1 && g.D <= 32 && !(dbg & SGM_DBG_NO_LANE_GROUPS) && 2 * g.ftzero + 63 <= 255;
    p.GWc = g.D > 64 ? 64 : (g.D <= 16 ? 8 : (g.D <= 32 ? 16 : 32));  // lane-group width of k_box_u8
    // rows per band of k_box_u8 (a band re-reads 2 * SH2 rows above it; multiples of 16: the register rings): 96, less
    // on frames too small to fill the chip with bands that tall
    const int cpw = box_columns(p.GWc);
    p.RBb = 96;
    for (int cand : {48, 32, 16})
        if ((int64_t)((g.W1 + cpw - 1) / cpw) * ((H + p.RBb - 1) / p.RBb) * 4 < 1024) p.RBb = cand;
    p.vsum_ring = g.SH2 >= 1 && g.SH2 <= 5;         // ring variant: each hsum row is read once
    p.vsum_wide = !(dbg & SGM_DBG_NARROW_VSUM);    // 8 int16 per thread (debug 8: 4, for A/B timing)

    p.v1 = e->schedule == 0;
    // D <= 32: rows without hand-off: band height 1, the pre-pass stores every row's
    // state; needs the 3-volume state buffer below the 4 GiB a 32-bit buffer offset reaches.
    // (At D = 64 the fused sweep is still ahead: 720p 0.35 against 0.39 ms, and 3 V of state.)
    p.GWs = (dbg & SGM_DBG_NO_LANE_GROUPS) ? 64 : group_width(g, H);
    // Throughput mode (schedule 2) takes D = 48 .. 64 through the chained sweeps all the same (half the lanes idle, but
    // 7 V of traffic per pair instead of the 22 V of the per-row state: batches of small frames are bound by HBM --
    // 64 pairs 720p D=64: 0.38 against 0.55 ms per pair); D <= 32 keeps the small-D kernels in every mode.
    p.rows4 = p.GWs <= 32 && e->sweep_rows <= 0 && !(e->schedule == 2 && p.GWs == 32) &&
              (int64_t)H * g.rowsz * 2 * 3 < (int64_t)0xfff00000;
    // the path set: MODE_SGBM one pass of 5 directions, MODE_HH two passes of 4, MODE_HH4 two passes of the 2 axis-aligned ones
    p.axis = g.mode == 3;
    p.nroles = p.axis ? 1 : 3;
    p.npass = g.mode == 0 ? 1 : 2;
    // Chained schedule (SGM_OPT_SCHEDULE 2, kernels_sweep.h: k_sweep_chain): no pre-pass; the bands of a sweep hand the
    // state of their last row to each other.  Only where the fused sweep runs (the small-D schedule keeps its own
    // kernels), where there is more than one band, and not with debug 2 (winner-take-all inside the second sweep).
    p.chain = e->schedule == 2 && !p.rows4 && !((dbg & SGM_DBG_WTA_IN_LAST_PATH) && g.mode == 1) && g.W1 > 0;
    p.R = p.rows4 ? 1 : sweep_rows_for(g, e->sweep_rows, p.npass, p.chain);
    if (p.chain && (H + p.R - 1) / p.R <= 1) {
        p.chain = false;
        p.R = sweep_rows_for(g, e->sweep_rows, p.npass, false);
    }
    p.nbands = (H + p.R - 1) / p.R;
    // small-D schedule: lane-grouped pre-pass lines, state stored after every row (debug 16: the single-direction kernel)
    p.prepass_g = p.rows4 && !(dbg & SGM_DBG_PREPASS_3_LAUNCHES);
    // Narrow frames (fewer than ~1.5 lines per SIMD) are bound by the latency of one wave's
    // instruction stream: there the single-direction kernel with one wave per (line, role) -- three
    // times the waves, a third of the work each -- is faster (720p D=64: 0.26 against 0.34 ms); its
    // three readers of C are served by L2 / the Infinity Cache at these sizes.
    const bool narrow = g.W1 <= 1536 && e->prepass_rows == 0;  // (an explicit chunk height selects k_prepass3: tests)
    // the three roles fused in one wave (k_prepass3); debug bit 16 selects the 3-launch variant.
    // Row chunks of about 135 rows, one launch each, base columns grouped per XCD: two of the
    // three reads of a C pixel hit L2 (kernels_path.h).  debug 512: one chunk, plain layout (A/B).
    // (MODE_HH4 has one pre-pass kernel, k_axis_prepass: a column scan without chunks)
    p.fused_prepass = !p.axis && !p.rows4 && !(dbg & SGM_DBG_PREPASS_3_LAUNCHES) && !narrow && (int64_t)g.rowsz * H < (1ll << 31);
    p.pre_plain = (dbg & SGM_DBG_PREPASS_ONE_CHUNK) != 0;
    p.pre_nch = p.pre_plain ? 1 : (e->prepass_rows > 0 ? (H + e->prepass_rows - 1) / e->prepass_rows : std::max(1, (H + 67) / 135));
    // multiples of 8 rows (two prefetch blocks): a chunk then ends in straight-line code
    // (debug 512 is ONE chunk whatever SGM_OPT_PREPASS_ROWS says: with the chunk height taken from the option the rows
    // below the first chunk were never walked and the bands under them started from stale boundary state)
    p.pre_rows = e->prepass_rows > 0 && !p.pre_plain ? e->prepass_rows : ((H + p.pre_nch - 1) / p.pre_nch + 7) / 8 * 8;
    // MODE_HH: the upward pre-pass only reads C, so it runs on the auxiliary stream while the
    // main stream does the downward pre-pass and sweep (memory-bound beside issue-bound work)
    p.overlap = p.npass == 2 && p.nbands > 1 && !(dbg & SGM_DBG_NO_PREPASS_OVERLAP) && !p.chain;
    // debug bit 64+128: fork right after the cost stage (both pre-passes side by side) instead
    // of after the downward pre-pass (upward pre-pass beside the downward sweep)
    p.fork_early = (dbg & SGM_DBG_FORK_PREPASS_EARLY) != 0;

    // Winner-take-all: a separate pass over S (k_wta_t, one lane per pixel) after the second sweep
    // of MODE_HH and after the in-row path of MODE_SGBM for D <= 128; fused into the in-row path
    // kernel for MODE_SGBM with D > 128 (there the separate form costs a third volume of traffic:
    // 4K D=256 2.49 ms fused against 2.56 + 0.73; D=128: 2.01 against 1.42 + 0.43, 1080p 0.79 against
    // 0.44 + 0.10).  debug 2 forces the fused form everywhere, debug 2048 the separate one (A/B, cross-check).
    // (The v1 schedule always fuses it into its last path kernel.)
    // MODE_HH4: always the separate pass (the axis-only sweeps have no SWEEP_LAST form).
    // SGM_OPT_CONFIDENCE: always the separate pass -- the confidence byte comes from k_wta_conf_t alone, so
    // the routes that fuse by default (v1, MODE_SGBM with D > 128, D > 512) store S once more and read it back: 2 V more.
    // SGM_OPT_RIGHT_VIEW: likewise -- the diagonal winner-take-all (k_right_wta) reads S from device memory.
    const bool conf = e->conf.on != 0 || e->right.on != 0;
    p.fused_wta = !conf && (p.v1 || (!p.axis && !(dbg & SGM_DBG_WTA_SEPARATE) && (((dbg & SGM_DBG_WTA_IN_LAST_PATH) && !p.rows4) ||
                                                                                  (g.mode == 0 && ((dbg & SGM_DBG_NO_LANE_GROUPS) || g.D > 128)))));
    // MODE_SGBM with the separate winner-take-all (D <= 128): the fifth path (in-row, right to left) needs
    // nothing but C, so it runs on the auxiliary stream from here on, as a FIRST pass into a volume of its
    // own (2 V of traffic instead of the 3 V of "S +="), beside the pre-pass and the sweep -- which at these
    // D are bound by instruction issue, not by HBM; k_wta_t adds the two volumes while it stages them.
    // debug 65536: the fifth path after the sweep, accumulating into S (A/B).
    // Split winner-take-all (kernels_path.h: wta_reduce_pixels): the chained second sweep of MODE_HH does the lane reductions on
    // the S it holds and stores a raw record per pixel instead of S; the wta stage is then k_wta_select.  2 V less traffic
    // per pair.  Full waves of D = 128 / 256 with a positive uniqueness weight, and only where nothing else wants S: not with
    // SGM_OPT_KEEP_AGGR, the confidence map or the right view.  debug 2048 takes the separate pass here too (A/B, cross-check).
    p.wta_split = p.chain && g.mode == 1 && !p.axis && !p.fused_wta && !np_partial(g) && g.NP <= 2 && g.uniq < 100 &&
                  !e->keep_aggr && !e->no_wta_split && !conf && !(dbg & SGM_DBG_WTA_SEPARATE);
    const bool two_vol = g.mode == 0 && !p.fused_wta && !p.v1 && g.D <= 128 && !(dbg & SGM_DBG_NO_LANE_GROUPS) &&
                         !(dbg & SGM_DBG_FIFTH_PATH_AFTER_SWEEP);
    // D <= 64 (small-D schedule): the OTHER in-row path (left to right) needs nothing but C either.  It used to follow
    // the element-wise vertical kernel as "S +=" on the main stream -- a chain of W1 dependent steps on the
    // critical path of a latency-bound frame; now it runs as a FIRST pass into a third volume on a stream of its
    // own, beside the per-row pre-pass and k_vert3_g, and the winner-take-all adds three volumes.
    const bool three_vol = two_vol && p.rows4 && !(dbg & SGM_DBG_IN_ROW_ON_MAIN_STREAM);
    // ... and so do the three directions that come from the row above: the walk along their lines (the "pre-pass" of
    // the small-D schedule) forms L_r(p, .) on its way, so each role writes it to a volume of its own and the
    // winner-take-all adds five volumes: no per-row record (3 V written, 3 V read), no element-wise kernel behind
    // the walk -- and all five directions are ONE launch (k_paths5_g: why, see there).  debug 8192: the record form
    // with the in-row paths on streams of their own (A/B; MODE_HH keeps it).
    const bool five_vol = three_vol && !(dbg & SGM_DBG_SMALL_D_RECORD);
    p.nvol = five_vol ? 5 : three_vol ? 3 : two_vol ? 2 : 1;
    // MODE_HH4 in the small-D schedule: all four directions in one launch, a volume each (k_axis_paths4_g), no record
    if (p.axis && p.rows4 && !p.v1) {
        p.nvol = 4;
        p.overlap = false;
    }
    // otherwise MODE_SGBM's fifth path follows the sweep on the main stream (S +=, or with the winner-take-all);
    // debug 4 (no lane groups): as the general line kernel (A/B)
    p.path_w_main = !p.v1 && g.mode == 0 && p.nvol == 1;
    p.path_w_lines = (dbg & SGM_DBG_NO_LANE_GROUPS) != 0;
    p.speckle = e->params.speckleRange >= 0 && e->params.speckleWindowSize > 0;  // upstream's condition for filterSpeckles
    // D > 512 (16 disparities per lane, NP = 8): the int16 cost pipeline and one k_path launch per
    // direction with the winner-take-all in the last, whatever the schedule option, the band / chunk / window options
    // and the schedule bits of SGM_OPT_DEBUG say -- no other kernel has an NP = 8 instantiation.  The batch entries
    // then run such pairs one after the other (batch_plan: joint needs a chained plan).
    if (g.NP == 8) {
        p.v1 = true;
        p.byte_cost = p.pix_px = p.rows4 = p.chain = p.prepass_g = p.fused_prepass = false;
        p.overlap = p.fork_early = p.path_w_main = false;
        p.GWs = 64;
        p.fused_wta = !conf;
        p.wta_split = false;
        p.nvol = 1;
    }
    return p;
}

// ---- the matcher on device buffers ---------------------------------------------------------
static int ensure_speckle_buffers(sgm_engine *e, size_t npx)
{
    int rc;
    if ((rc = e->label.ensure(npx * 4)) || (rc = e->csize.ensure(npx * 4))) return rc;
    return e->rlen.ensure(npx * 4);
}
// control words of a chained launch over nf frames: ticket + one progress word per band (zeroed before every launch)
static size_t chain_ctl_bytes(int nf, int nbands) { return ((size_t)(1 + (size_t)nf * nbands) * 4 + 15) & ~(size_t)15; }

// Every device buffer one compute of this shape needs under plan p, allocated BEFORE anything is enqueued (a pair of a
// chained group that does not fit then costs nothing but a smaller group).  Records the shape in e->g.
// device bytes the engine holds.  Only ever compared with itself across one ensure_plan_buffers call (prepare_group: that
// call allocated something iff this grew), and the call touches none of the buffers it does not size: summing EVERY buffer
// gives the comparison the same outcome as summing those alone.
static size_t plan_bytes_held(const sgm_engine *e)
{
    size_t n = 0;
    each_devbuf(e, [&](const DevBuf &b) { n += b.cap; });
    return n;
}
static int ensure_plan_buffers(sgm_engine *e, const Plan &p, int H, int W)
{
    Geom g;
    int rc = normalise(&e->params, H, W, &g);
    if (rc) return rc;
    e->g = g;
    e->H = H;
    e->W = W;
    const size_t npx = (size_t)H * W;
    const size_t vol = (size_t)std::max<int64_t>(g.rowsz, 0) * H * sizeof(int16_t);
    // 64 bytes of slack behind the last record: k_pix reads the records with scalar loads -- no bounds check, and the
    // compiler may merge or widen them (the widest scalar load is 64 bytes).  Every load STARTS at a record of the
    // frame, so none can leave the allocation.  (Not in the guarded mode: there the buffer ends where its mapping
    // ends, and the parity cases of tests/test_gpu_guard.py show that no load goes past the last record at all.)
    // (colour pairs: three records per pixel and 18 planes, k_features<3>)
    // (census: one 8-byte descriptor per pixel and image -- the left ones fit lrec as it is, the right ones take 8 bytes
    // per pixel of rplanes instead of 6; k_pix_census* read both with plain global loads, each behind an explicit test
    // that its position lies inside the row: no scalar loads, no slack needed)
    if ((rc = e->lrec.ensure(npx * 8 * p.cn + (debug_alloc_mode() ? 0 : 64)))) return rc;
    if ((rc = e->rplanes.ensure(p.census ? npx * 8 : npx * 6 * p.cn))) return rc;
    if (vol) {
        // The byte pipeline keeps its per-pixel costs (V / 2) in the S buffer: they are dead when the block cost C is
        // complete, and no kernel writes S before that (the sweeps, the in-row paths and k_paths5_g all read C; in a batch
        // every pair's cost stage is complete before the joint sweep launch starts).  Only the int16 pipeline needs a
        // volume of its own for the horizontal sums.  4K D=256: 13 -> 9 GB per engine (round 3 allocated V for them always).
        if (!p.byte_cost && (rc = e->hsum.ensure(vol))) return rc;
        if ((rc = e->cost.ensure(vol))) return rc;
        if ((rc = e->aggr.ensure(vol))) return rc;
        DevBuf *more[] = {&e->aggr2, &e->aggr3, &e->aggr4, &e->aggr5};  // the volumes k_wta_t adds to S (Plan::nvol)
        for (int k = 1; k < p.nvol; k++)
            if ((rc = more[k - 1]->ensure(vol))) return rc;
    }
    if ((rc = e->wta.ensure(npx * 8))) return rc;
    if (p.wta_split && (rc = e->wta_raw.ensure(npx * 16))) return rc;
    if ((rc = e->disp_raw.ensure(npx * 2))) return rc;
    if ((rc = e->disp_med.ensure(npx * 2))) return rc;
    for (SideMap *m : {&e->conf, &e->right})
        if (m->on && ((rc = m->raw.ensure(npx * m->bpp)) || (rc = m->fin.ensure(npx * m->bpp)))) return rc;
    if (e->right.on && g.W1 > 0 && (rc = e->rrec.ensure((size_t)H * g.W1 * 8))) return rc;
    if ((rc = e->headroom.ensure(8))) return rc;
    e->g.hr = (uint32_t *)e->headroom.p;
    if (g.W1 > 0 && !p.v1 && p.nbands > 1 && p.nvol < 4) {
        const size_t bnd_bytes = (size_t)p.nbands * g.W1 * p.nroles * g.D * 2;
        if ((rc = e->bndL.ensure(bnd_bytes))) return rc;
        if (!p.chain) {
            if (p.npass == 2 && (rc = e->bndL2.ensure(bnd_bytes))) return rc;
            if (!p.axis) {  // (k_axis_prepass carries no state between launches)
                const size_t st_bytes = (size_t)2 * 3 * g.W1 * g.D * 2;  // ping-pong line state between pre-pass chunks
                if ((rc = e->pstate.ensure(st_bytes))) return rc;
                if (p.npass == 2 && (rc = e->pstate2.ensure(st_bytes))) return rc;
            }
        }
    }
    if (p.speckle && (rc = ensure_speckle_buffers(e, npx))) return rc;
    if (p.chain) {
        if ((rc = e->chain_ctl.ensure(chain_ctl_bytes(1, p.nbands)))) return rc;
        if (!e->chain_err.p) {  // the sticky give-up flag (check_chain) starts out clear
            if ((rc = e->chain_err.ensure(16))) return rc;
            HIP_TRY(hipMemsetAsync(e->chain_err.p, 0, 16, e->stream));
        }
    }
    return SGM_OK;
}

static int run_speckles(sgm_engine *e, int16_t *d_img, int H, int W, int newVal, int maxSpeckleSize, int maxDiff)
{
    const size_t npx = (size_t)H * W;
    int rc;
    if ((rc = ensure_speckle_buffers(e, npx))) return rc;
    int *label = (int *)e->label.p, *csz = (int *)e->csize.p, *rlen = (int *)e->rlen.p;
    hipStream_t st = e->stream;
    dim3 g2((W + 255) / 256, H);
    hipLaunchKernelGGL(k_ccl_rows, dim3(H), dim3(64), 0, st, (const int16_t *)d_img, label, rlen, csz, W, newVal, maxDiff);
    hipLaunchKernelGGL(k_ccl_merge, g2, dim3(256), 0, st, (const int16_t *)d_img, label, H, W, newVal, maxDiff);
    hipLaunchKernelGGL(k_ccl_count, g2, dim3(256), 0, st, (const int16_t *)d_img, label, (const int *)rlen, csz, H, W, newVal, maxDiff);
    hipLaunchKernelGGL(k_ccl_apply, g2, dim3(256), 0, st, d_img, label, (const int *)csz, H, W, newVal, maxDiff, maxSpeckleSize);
    KCHECK();
    return SGM_OK;
}

__global__ void k_fill_i16(int16_t *p, int64_t n, int16_t v)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

// ---- cost stage launches ---------------------------------------------------------------------
constexpr int COST_XL = 128;  // columns per chunk of k_pix / k_hsum
static int cost_chunks(const Geom &g) { return (g.W1 + COST_XL - 1) / COST_XL; }

// per-pixel cost of the whole frame as bytes (px: the S buffer, ensure_plan_buffers)
static void launch_pix(const Geom &g, const uint2 *lrec, const uint8_t *rpl, uint8_t *px, hipStream_t st)
{
    if (g.D <= 32) {  // one thread per pixel
        hipLaunchKernelGGL(k_pix_px, dim3((g.W1 + 255) / 256, g.H), dim3(256), (size_t)6 * (256 + g.D), st, g, lrec, rpl, px);
        return;
    }
    // LDS: the six planes' segments widened to 16 bits, two copies each (kernels_cost.h: 6.2 / 9.2 / 15.2 KiB at NP = 1 / 2 / 4)
    static_assert(COST_XL <= PIX_XL, "k_pix sizes its LDS copies for chunks of at most PIX_XL columns");
    const int nchunks = cost_chunks(g);
    dim3 grid((unsigned)((int64_t)g.H * nchunks)), block(64);
    if (g.NP == 1) hipLaunchKernelGGL(k_pix<1>, grid, block, (size_t)pix_lds_bytes<1>(), st, g, lrec, rpl, px, COST_XL, nchunks, 0);
    else if (g.NP == 2) hipLaunchKernelGGL(k_pix<2>, grid, block, (size_t)pix_lds_bytes<2>(), st, g, lrec, rpl, px, COST_XL, nchunks, 0);
    else hipLaunchKernelGGL(k_pix<4>, grid, block, (size_t)pix_lds_bytes<4>(), st, g, lrec, rpl, px, COST_XL, nchunks, 0);
}

// census: Hamming distances of the descriptors as bytes, where launch_pix puts its bytes.  D <= 32: one thread per pixel
// (debug 4, "no lane groups": the wave form with idle lanes, for A/B timing -- tools/census_stages.py)
static_assert(CENSUS_XL == COST_XL, "k_pix_census chunks are the cost stage's");
static void launch_pix_census(const Geom &g, int dbg, const uint64_t *dl, const uint64_t *dr, uint8_t *px, hipStream_t st)
{
    if (g.D <= 32 && !(dbg & SGM_DBG_NO_LANE_GROUPS)) {
        hipLaunchKernelGGL(k_pix_census_px, dim3((g.W1 + 255) / 256, g.H), dim3(256), (size_t)8 * (256 + g.D), st, g, dl, dr, px);
        return;
    }
    const int nchunks = cost_chunks(g);
    dim3 grid((unsigned)((int64_t)g.H * nchunks)), block(64);
    if (g.NP == 1) hipLaunchKernelGGL(k_pix_census<1>, grid, block, 0, st, g, dl, dr, px, nchunks);
    else if (g.NP == 2) hipLaunchKernelGGL(k_pix_census<2>, grid, block, 0, st, g, dl, dr, px, nchunks);
    else if (g.NP == 4) hipLaunchKernelGGL(k_pix_census<4>, grid, block, 0, st, g, dl, dr, px, nchunks);
    else hipLaunchKernelGGL(k_pix_census<8>, grid, block, 0, st, g, dl, dr, px, nchunks);
}

// box filter of the byte costs -> block cost C (k_box_u8), bands of p.RBb rows
static void launch_box(const Geom &g, const Plan &p, const uint8_t *px, int16_t *C, hipStream_t st)
{
    const int cpw = box_columns(p.GWc), RBb = p.RBb;
    dim3 grid((g.W1 + cpw - 1) / cpw, (g.H + RBb - 1) / RBb), block(256);
    with_radius(g.SW2, [&](auto r) {
        constexpr int R = decltype(r)::value;
        if (p.GWc == 8) hipLaunchKernelGGL((k_box_u8<R, 1, 8>), grid, block, 0, st, g, px, C, RBb);
        else if (p.GWc == 16) hipLaunchKernelGGL((k_box_u8<R, 1, 16>), grid, block, 0, st, g, px, C, RBb);
        else if (p.GWc == 32) hipLaunchKernelGGL((k_box_u8<R, 1, 32>), grid, block, 0, st, g, px, C, RBb);
        else if (g.NP == 1) hipLaunchKernelGGL((k_box_u8<R, 1>), grid, block, 0, st, g, px, C, RBb);
        else if (g.NP == 2) hipLaunchKernelGGL((k_box_u8<R, 2>), grid, block, 0, st, g, px, C, RBb);
        else hipLaunchKernelGGL((k_box_u8<R, 4>), grid, block, 0, st, g, px, C, RBb);
    });
}

// int16 pipeline: pixel cost (summed over the cn channels) + horizontal box sum, all rows (k_hsum); RS_T = RS
// instantiations carry the unrolled interior fast path (block sizes up to 15)
template <int NP, int RS_T, int CN>
static int launch_hsum_t(const Geom &g, const uint2 *lrec, const uint8_t *rpl, int16_t *HS, int RS, hipStream_t st)
{
    const int nchunks = cost_chunks(g);
    // (largest: NP = 8, blockSize 31 -> RS = 32: a 64 KiB ring + 1.3 KiB of records + 7 KiB of planes, of 160 KiB; colour
    // pairs 3.8 KiB of records + 20.8 KiB of planes)
    const HsumLds l = hsum_lds_layout(g.NP, RS, COST_XL, g.SW2, CN);
    if (l.total_bytes > 160 * 1024)
        return set_err(SGM_ERR_UNSUPPORTED, "k_hsum%s needs %d bytes of LDS", CN == 3 ? "_c3" : "", l.total_bytes);
    if (l.total_bytes > 48 * 1024)
        HIP_TRY(hipFuncSetAttribute((const void *)k_hsum<NP, RS_T, CN>, hipFuncAttributeMaxDynamicSharedMemorySize, l.total_bytes));
    hipLaunchKernelGGL((k_hsum<NP, RS_T, CN>), dim3((unsigned)((int64_t)g.H * nchunks)), dim3(64), l.total_bytes, st, g, lrec,
                       rpl, HS, COST_XL, nchunks, RS, l.ring_bytes, l.lrec_bytes, l.seg_len);
    return SGM_OK;
}
static int launch_hsum(const Geom &g, int cn, const uint2 *lrec, const uint8_t *rpl, int16_t *HS, hipStream_t st)
{
    int RS = 1;  // ring of the last blockSize+1 cost vectors, rounded to a power of two
    while (RS < 2 * g.SW2 + 2) RS <<= 1;
    auto go = [&](auto c) {
        constexpr int CN = decltype(c)::value;
        return with_np_wide(g, [&](auto np, auto) {
            if (RS == 4) return launch_hsum_t<np, 4, CN>(g, lrec, rpl, HS, RS, st);
            if (RS == 8) return launch_hsum_t<np, 8, CN>(g, lrec, rpl, HS, RS, st);
            if (RS == 16) return launch_hsum_t<np, 16, CN>(g, lrec, rpl, HS, RS, st);
            return launch_hsum_t<np, 0, CN>(g, lrec, rpl, HS, RS, st);
        });
    };
    return cn == 3 ? go(std::integral_constant<int, 3>()) : go(std::integral_constant<int, 1>());
}

// int16 pipeline: vertical box sum -> block cost C (k_vsum_ring in bands of 96 rows; the generic k_vsum for radii above 5)
static void launch_vsum(const Geom &g, const Plan &p, const int16_t *hs, int16_t *C, hipStream_t st)
{
    const int H = g.H;
    if (!p.vsum_ring) {
        dim3 block(256), grid((unsigned)((g.rowsz / 8 + 255) / 256), (H + 63) / 64);
        hipLaunchKernelGGL(k_vsum, grid, block, 0, st, hs, C, H, g.rowsz, g.SH2, 64, g.hr);
        return;
    }
    const int RB = 96;  // rows per band of the vertical sum; multiple of every ring size used below
    dim3 block(256), grid((unsigned)((g.rowsz / (p.vsum_wide ? 8 : 4) + 255) / 256), (H + RB - 1) / RB);
    with_radius(g.SH2, [&](auto r) {
        constexpr int SH2 = decltype(r)::value;
        if (p.vsum_wide) hipLaunchKernelGGL((k_vsum_ring<SH2, 4>), grid, block, 0, st, hs, C, H, g.rowsz, RB, g.hr);
        else hipLaunchKernelGGL((k_vsum_ring<SH2, 2>), grid, block, 0, st, hs, C, H, g.rowsz, RB, g.hr);
    });
}

// ---- path stage launches ---------------------------------------------------------------------
// one row chunk [s0, s1) (in sweep order) of the fused three-role pre-pass; chunk index c picks the
// ping-pong halves of the line-state buffer (kernels_path.h)
static void launch_prepass3(const sgm_engine *e, const Plan &p, int xdir, int ydir, int16_t *bl, hipStream_t on, int c, int s0, int s1)
{
    const Geom &g = e->g;
    const int cpx = p.pre_plain ? 0 : (g.W1 + 7) / 8;
    // (Padding the grid so that every SIMD holds the same number of waves, and halving the
    // prefetch depth, were both measured: no change -- DESIGN.md 4.4.)
    const int wpb = SGM_PREPASS_WPB;
    dim3 grid(p.pre_plain ? (g.W1 + wpb - 1) / wpb : 8 * ((cpx + wpb - 1) / wpb)), block(64 * wpb);
    const size_t half = (size_t)3 * g.W1 * g.D;  // int16 elements of one state buffer
    int16_t *sbuf = (int16_t *)(ydir > 0 ? e->pstate.p : e->pstate2.p);
    const int16_t *sin = sbuf ? sbuf + (size_t)(c & 1) * half : nullptr;
    int16_t *sout = sbuf ? sbuf + (size_t)((c + 1) & 1) * half : nullptr;
    const int16_t *C = (const int16_t *)e->cost.p;
    // (prefetch blocks of 2 rows for the pass that runs beside the sweep -- 70 registers instead of 106 -- were
    // measured in round 2: within noise; that instantiation is gone)
    with_np(g, [&](auto np, auto part) {
        hipLaunchKernelGGL((k_prepass3<np, part>), grid, block, 0, on, g, xdir, ydir, C, bl, p.R, s0, s1, sin, sout, cpx);
    });
}
// the boundary pre-pass of one pass into bl, on stream `on`; returns the launch count.  Roles of the pre-pass:
// 0 = predecessor one step earlier in the sweep's x order (x - xdir), 1 = same column, 2 = one step later
static int launch_prepass(const sgm_engine *e, const Plan &p, int xdir, int ydir, int16_t *bl, hipStream_t on)
{
    const Geom &g = e->g;
    const int16_t *C = (const int16_t *)e->cost.p;
    if (p.axis) {  // the vertical path alone: one wave per column, record [band][x][1][D]
        with_np(g, [&](auto np, auto part) {
            hipLaunchKernelGGL((k_axis_prepass<np, part>), dim3(g.W1), dim3(64), 0, on, g, ydir, C, bl, p.R, p.nbands);
        });
        return 1;
    }
    if (p.prepass_g) {
        // one role per wave (grid.y = 3): these frames have too few lines to fill the SIMDs with
        // three-role waves (4K D=16: 478)
        const int G = 64 / p.GWs;
        dim3 grid((g.W1 + G - 1) / G, 3), block(64);
        with_gw(p.GWs, g.D, [&](auto gw, auto part) {
            hipLaunchKernelGGL((k_prepass3_g<gw, part>), grid, block, 0, on, g, xdir, ydir, C, bl);
        });
        return 1;
    }
    if (p.fused_prepass) {
        int n = 0;
        for (int c = 0; c < p.pre_nch; c++) {
            const int s0 = c * p.pre_rows, s1 = std::min(g.H, s0 + p.pre_rows);
            if (s0 >= s1) break;
            launch_prepass3(e, p, xdir, ydir, bl, on, c, s0, s1);
            n++;
        }
        return n;
    }
    // one launch of the single-direction kernel, grid.y = role
    launch_path(g, xdir, ydir, PATH_BOUNDARY, C, (int16_t *)e->aggr.p, 0, (uint2 *)e->wta.p, on, Boundary{bl, p.R, 0});
    return 1;
}

// D <= 64, band height 1: the three directions from the previous row are element-wise given the
// pre-pass state of every row (k_vert3_g, one streaming pass over all pixels)
static void launch_vert3(const Geom &g, int GW, bool first, int dir, const int16_t *C, int16_t *S, const int16_t *bq, int rmaj,
                         hipStream_t st)
{
    dim3 grid((g.W1 + 255) / 256, g.H), block(256);
    with_gw(GW, g.D, [&](auto gw, auto part) {
        if (first) hipLaunchKernelGGL((k_vert3_g<gw, PATH_FIRST, part>), grid, block, 0, st, g, dir, dir, C, S, bq, rmaj);
        else hipLaunchKernelGGL((k_vert3_g<gw, PATH_ACCUM, part>), grid, block, 0, st, g, dir, dir, C, S, bq, rmaj);
    });
}

// D <= 64, MODE_SGBM: all five directions in one launch, one volume each (k_paths5_g; the one pass runs top-down)
static void launch_paths5(const Geom &g, int GW, const int16_t *C, int16_t *const Sv[5], hipStream_t st)
{
    const int G = 64 / GW, nr = (g.H + G - 1) / G, nl = (g.W1 + G - 1) / G;
    // (Measured beside it: rows and lines as two launches one after the other, in either order -- 4K D=16 0.60 /
    // 0.59 ms against 0.57 ms, 720p D=64 0.21 / 0.22 against 0.19; occupancy capped at one or two waves per SIMD
    // through an LDS allocation -- 0.66 against 0.65 ms, 0.23 / 0.27 against 0.20.  Neither the order nor the
    // number of waves per SIMD matters: the stage moves 6 ... 10 V in 32-byte pieces per row and is bound by
    // the memory side)
    dim3 grid(2 * nr + 3 * nl), block(64);
    with_gw(GW, g.D, [&](auto gw, auto part) {
        hipLaunchKernelGGL((k_paths5_g<gw, part>), grid, block, 0, st, g, 1, 1, C, Sv[0], Sv[3], Sv[4], Sv[1], Sv[2], nr);
    });
}

// D <= 64, MODE_HH4: the four axis-aligned directions in one launch, one volume each (k_axis_paths4_g)
static void launch_axis_paths4(const Geom &g, int GW, const int16_t *C, int16_t *const Sv[5], hipStream_t st)
{
    const int G = 64 / GW, nr = (g.H + G - 1) / G, nl = (g.W1 + G - 1) / G;
    dim3 grid(2 * nr + 2 * nl), block(64);
    with_gw(GW, g.D, [&](auto gw, auto part) {
        hipLaunchKernelGGL((k_axis_paths4_g<gw, part>), grid, block, 0, st, g, C, Sv[0], Sv[1], Sv[2], Sv[3], nr);
    });
}

// ---- winner-take-all launch ------------------------------------------------------------------
// k_wta_t over S plus NV - 1 more volumes.  LG = log2(D / 8) for the powers of two that have an instantiation (NV = 1:
// D = 16 .. 512; 2: up to 128; 3, 4, 5: up to 64), -1 (any D) otherwise
// CONF: k_wta_conf_t, which also writes the confidence byte to `conf` (one instantiation for either sign of the weight)
template <bool POSW, int LG, int NV, bool CONF>
static int launch_wta_t(const Geom &g, int16_t *const Sv[5], uint2 *wta, uint8_t *conf, int64_t npix, hipStream_t st)
{
    const size_t lds = (size_t)64 * wta_t_stride(g.D);
    // persistent blocks: LDS (64 padded rows) allows four waves per CU; each loops over its share
    dim3 grid((unsigned)std::min<int64_t>((npix + 63) / 64, 4 * 256)), block(64);
    if constexpr (CONF) {
        if (lds > 160 * 1024) return set_err(SGM_ERR_UNSUPPORTED, "k_wta_conf_t needs %zu bytes of LDS", lds);
        if (lds > 48 * 1024)
            HIP_TRY(hipFuncSetAttribute((const void *)k_wta_conf_t<LG, NV>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((k_wta_conf_t<LG, NV>), grid, block, lds, st, g, (const int16_t *)Sv[0], wta, npix, (const int16_t *)Sv[1],
                           (const int16_t *)Sv[2], (const int16_t *)Sv[3], (const int16_t *)Sv[4], conf);
    } else {
        if (lds > 48 * 1024)
            HIP_TRY(hipFuncSetAttribute((const void *)k_wta_t<POSW, LG, NV>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((k_wta_t<POSW, LG, NV>), grid, block, lds, st, g, (const int16_t *)Sv[0], wta, npix,
                           (const int16_t *)Sv[1], (const int16_t *)Sv[2], (const int16_t *)Sv[3], (const int16_t *)Sv[4]);
    }
    return SGM_OK;
}
template <bool POSW, int NV, bool CONF, int LG = 1>
static int launch_wta_lg(int lg, const Geom &g, int16_t *const Sv[5], uint2 *wta, uint8_t *conf, int64_t npix, hipStream_t st)
{
    if constexpr (LG > (NV == 1 ? 6 : NV == 2 ? 4 : 3)) return launch_wta_t<POSW, -1, NV, CONF>(g, Sv, wta, conf, npix, st);
    else if (lg == LG) return launch_wta_t<POSW, LG, NV, CONF>(g, Sv, wta, conf, npix, st);
    else return launch_wta_lg<POSW, NV, CONF, LG + 1>(lg, g, Sv, wta, conf, npix, st);
}
// conf: null, or the raw map of a confidence compute (already cleared)
static int launch_wta(const Geom &g, int nvol, int16_t *const Sv[5], uint2 *wta, uint8_t *conf, hipStream_t st)
{
    const int64_t npix = (int64_t)g.H * g.W1;
    int lg = -1;  // log2(D / 8) when D is a power of two
    for (int q = 1; q <= 6; q++)
        if (g.D == (8 << q)) lg = q;
    auto go = [&](auto posw, auto cf) {
        constexpr bool POSW = decltype(posw)::value, CONF = decltype(cf)::value;
        if (nvol == 5) return launch_wta_lg<POSW, 5, CONF>(lg, g, Sv, wta, conf, npix, st);
        if (nvol == 4) return launch_wta_lg<POSW, 4, CONF>(lg, g, Sv, wta, conf, npix, st);
        if (nvol == 3) return launch_wta_lg<POSW, 3, CONF>(lg, g, Sv, wta, conf, npix, st);
        if (nvol == 2) return launch_wta_lg<POSW, 2, CONF>(lg, g, Sv, wta, conf, npix, st);
        return launch_wta_lg<POSW, 1, CONF>(lg, g, Sv, wta, conf, npix, st);
    };
    if (conf) return go(std::false_type(), std::true_type());
    return g.uniq < 100 ? go(std::true_type(), std::false_type()) : go(std::false_type(), std::false_type());
}

// ---- the stages of one compute -----------------------------------------------------------------
// Phases of one compute.  A single pair runs them all; the batch entry with chained sweeps
// (sgm_pipeline_batch_device) runs PH_PRE of every pair, then ONE sweep launch per pass for all pairs, then PH_POST
// of every pair.
enum { PH_PRE = 1 /* features, block cost, MODE_SGBM's fifth path beside the sweep */, PH_MID = 2 /* pre-pass + sweeps */,
       PH_POST = 4 /* the rest */, PH_ALL = 7 };

// one stage on stream `on`: `enqueue` returns its launch count, or an SGM_ERR_* code (< 0)
template <class F>
static int run_stage(sgm_engine *e, const char *name, hipStream_t on, F &&enqueue)
{
    int rc = stage_begin(e, name, on);
    if (rc) return rc;
    const int n = enqueue();
    if (n < 0) return n;
    KCHECK();
    return stage_end(e, n, on);
}
// ... on the engine's own stream
template <class F>
static int run_stage(sgm_engine *e, const char *name, F &&enqueue)
{
    return run_stage(e, name, e->stream, enqueue);
}

// the auxiliary streams and their events, created on first use
static int ensure_aux(sgm_engine *e, bool second)
{
    if (!e->aux) {
        HIP_TRY(hipStreamCreateWithFlags(&e->aux, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming));
    }
    if (second && !e->aux2) {
        HIP_TRY(hipStreamCreateWithFlags(&e->aux2, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&e->ev_join2, hipEventDisableTiming));
    }
    return SGM_OK;
}

static int stage_features(sgm_engine *e, const Plan &p, const uint8_t *d_left, const uint8_t *d_right, int64_t stride)
{
    const Geom &g = e->g;
    if (p.census)
        return run_stage(e, "census", e->stream, [&] {
            hipLaunchKernelGGL(k_census, dim3((g.W + 255) / 256, g.H, 2), dim3(256), 0, e->stream, d_left, d_right, stride, g.H, g.W,
                               (uint64_t *)e->lrec.p, (uint64_t *)e->rplanes.p);
            return 1;
        });
    return run_stage(e, p.cn == 3 ? "features_c3" : "features", e->stream, [&] {
        hipLaunchKernelGGL(p.cn == 3 ? k_features<3> : k_features<1>, dim3((g.W + 255) / 256, g.H, 2), dim3(256), 0, e->stream,
                           d_left, d_right, stride, g.H, g.W, g.ftzero, (uint2 *)e->lrec.p, (uint8_t *)e->rplanes.p);
        return 1;
    });
}

// per-pixel cost and box sums -> block cost C
// (Running the cost stage and the downward pre-pass as a pipeline over row chunks on separate
// streams was built and measured in round 2: the overlapped kernels only slow each other down --
// cost_box 1.17 -> 2.75 ms, prepass_dn 2.05 -> 3.19 ms, frame 11.97 against 11.90 ms -- this phase
// of the frame is bound by HBM bandwidth, not by the order of its launches.  DESIGN.md 4.4.)
static int stage_cost(sgm_engine *e, const Plan &p)
{
    const Geom &g = e->g;
    hipStream_t st = e->stream;
    const uint2 *lrec = (const uint2 *)e->lrec.p;
    const uint8_t *rpl = (const uint8_t *)e->rplanes.p;
    uint8_t *px = (uint8_t *)e->aggr.p;  // (the byte costs live in the S buffer until C is complete: ensure_plan_buffers)
    int16_t *C = (int16_t *)e->cost.p, *HS = (int16_t *)e->hsum.p;
    int rc;
    if (p.census) {
        // the bytes of k_pix_census*, then the box stages on the bytes: k_box_u8, or k_hsum_u8 + k_vsum* (blockSize 1 and
        // above 11, D > 512, byte volumes from 2 GiB, debug 256); either commits the headroom word.  (k_hsum_px, which the
        // BT pipeline runs for D <= 32, is one thread per PIXEL: at 4K D = 256 its 16-byte reads 256 bytes apart took
        // 12.7 ms for this stage; k_hsum_u8's threads span the disparities.)
        rc = run_stage(e, "cost_pix_census", st, [&] {
            launch_pix_census(g, e->debug, (const uint64_t *)e->lrec.p, (const uint64_t *)e->rplanes.p, px, st);
            return 1;
        });
        if (rc) return rc;
        if (p.byte_cost) return run_stage(e, "cost_box", st, [&] { launch_box(g, p, px, C, st); return 1; });
        rc = run_stage(e, "cost_hsum", st, [&] {
            hipLaunchKernelGGL(k_hsum_u8, dim3((unsigned)(((int64_t)g.W1 * (g.D / 8) + 255) / 256), g.H), dim3(256), 0, st, g,
                               (const uint8_t *)px, HS);
            return 1;
        });
        if (rc) return rc;
        return run_stage(e, "cost_vsum", st, [&] { launch_vsum(g, p, HS, C, st); return 1; });
    }
    if (p.byte_cost) {
        if ((rc = run_stage(e, "cost_pix", st, [&] { launch_pix(g, lrec, rpl, px, st); return 1; }))) return rc;
        return run_stage(e, "cost_box", st, [&] { launch_box(g, p, px, C, st); return 1; });
    }
    rc = run_stage(e, p.cn == 3 ? "cost_hsum_c3" : "cost_hsum", st, [&] {
        if (!p.pix_px) {
            const int r = launch_hsum(g, p.cn, lrec, rpl, HS, st);
            return r ? r : 1;
        }
        launch_pix(g, lrec, rpl, px, st);
        hipLaunchKernelGGL(k_hsum_px, dim3((g.W1 + 255) / 256, g.H), dim3(256), 0, st, g, (const uint8_t *)px, HS);
        return 1;
    });
    if (rc) return rc;
    return run_stage(e, "cost_vsum", st, [&] { launch_vsum(g, p, HS, C, st); return 1; });
}

// MODE_SGBM, Plan::nvol 2 and 3: the in-row paths on the auxiliary streams, from here on, each into a volume of its own
static int fork_in_row(sgm_engine *e, const Plan &p)
{
    if (p.nvol != 2 && p.nvol != 3) return SGM_OK;
    const Geom &g = e->g;
    const int16_t *C = (const int16_t *)e->cost.p;
    uint2 *wta = (uint2 *)e->wta.p;
    int rc;
    if ((rc = ensure_aux(e, p.nvol == 3))) return rc;
    HIP_TRY(hipEventRecord(e->ev_fork, e->stream));
    HIP_TRY(hipStreamWaitEvent(e->aux, e->ev_fork, 0));
    rc = run_stage(e, "path_W", e->aux, [&] {
        launch_rows_grouped(g, g.H, p.GWs, -1, PATH_FIRST, C, (int16_t *)e->aggr2.p, 1, wta, e->aux);
        return 1;
    });
    if (rc) return rc;
    HIP_TRY(hipEventRecord(e->ev_join, e->aux));
    if (p.nvol == 3) {
        HIP_TRY(hipStreamWaitEvent(e->aux2, e->ev_fork, 0));
        rc = run_stage(e, "path_E", e->aux2, [&] {
            launch_rows_grouped(g, g.H, p.GWs, +1, PATH_FIRST, C, (int16_t *)e->aggr3.p, 1, wta, e->aux2);
            return 1;
        });
        if (rc) return rc;
        HIP_TRY(hipEventRecord(e->ev_join2, e->aux2));
    }
    return SGM_OK;
}

// v1 schedule: one kernel per direction, vertical-ish first, horizontal last (WTA)
static int paths_v1(sgm_engine *e, const Plan &p)
{
    struct Dir { int rx, ry; const char *name; };
    static const Dir dirs[8] = {{0, 1, "path_S"}, {1, 1, "path_SE"}, {-1, 1, "path_SW"}, {0, -1, "path_N"},
                                {1, -1, "path_NE"}, {-1, -1, "path_NW"}, {1, 0, "path_E"}, {-1, 0, "path_W_wta"}};
    const Geom &g = e->g;
    for (int k = 0; k < 8; k++) {
        if (g.mode == 0 && k >= 3 && k < 6) continue;  // (the upward directions: MODE_HH only)
        if (g.mode == 3 && dirs[k].rx != 0 && dirs[k].ry != 0) continue;  // (MODE_HH4: no diagonals)
        // (SGM_OPT_CONFIDENCE: the last direction only accumulates; k_wta_conf_t follows)
        const int mode = k == 0 ? PATH_FIRST : (k == 7 && p.fused_wta ? PATH_LAST : PATH_ACCUM);
        int rc = run_stage(e, k == 7 && !p.fused_wta ? "path_W" : dirs[k].name, e->stream, [&] {
            launch_path(g, dirs[k].rx, dirs[k].ry, mode, (const int16_t *)e->cost.p, (int16_t *)e->aggr.p, k == 7 ? e->keep_aggr : 0,
                        (uint2 *)e->wta.p, e->stream);
            return 1;
        });
        if (rc) return rc;
    }
    return SGM_OK;
}

// MODE_HH: the upward pre-pass on the auxiliary stream, from "now" on the main stream
static int fork_prepass_up(sgm_engine *e, const Plan &p)
{
    int rc;
    if ((rc = ensure_aux(e, false))) return rc;
    HIP_TRY(hipEventRecord(e->ev_fork, e->stream));
    HIP_TRY(hipStreamWaitEvent(e->aux, e->ev_fork, 0));
    if ((rc = run_stage(e, "prepass_up", e->aux, [&] { return launch_prepass(e, p, -1, -1, (int16_t *)e->bndL2.p, e->aux); })))
        return rc;
    HIP_TRY(hipEventRecord(e->ev_join, e->aux));
    return SGM_OK;
}

// fused schedules: per pass a read-only boundary pre-pass (3 line scans) + one sweep; chained sweeps; the small-D kernels
static int paths_fused(sgm_engine *e, const Plan &p)
{
    const Geom &g = e->g;
    hipStream_t st = e->stream;
    const int16_t *C = (const int16_t *)e->cost.p;
    int16_t *S = (int16_t *)e->aggr.p;
    uint2 *wta = (uint2 *)e->wta.p;
    int rc;
    if (p.nvol == 4)
        return run_stage(e, "paths4", st, [&] {
            int16_t *const Sv[5] = {S, (int16_t *)e->aggr2.p, (int16_t *)e->aggr3.p, (int16_t *)e->aggr4.p, nullptr};
            launch_axis_paths4(g, p.GWs, C, Sv, st);
            return 1;
        });
    if (p.overlap && p.fork_early && (rc = fork_prepass_up(e, p))) return rc;
    for (int pass = 0; pass < p.npass; pass++) {
        const int ydir = pass == 0 ? 1 : -1, xdir = ydir;
        int16_t *bl = (int16_t *)(pass == 0 ? e->bndL.p : e->bndL2.p);
        if (p.nbands > 1 && !(p.overlap && pass == 1) && !p.chain && p.nvol != 5) {
            rc = run_stage(e, pass == 0 ? "prepass_dn" : "prepass_up", st, [&] { return launch_prepass(e, p, xdir, ydir, bl, st); });
            if (rc) return rc;
        }
        if (p.overlap && pass == 0 && !p.fork_early && (rc = fork_prepass_up(e, p))) return rc;
        if (p.overlap && pass == 1) {
            HIP_TRY(hipStreamWaitEvent(st, e->ev_join, 0));
            stage_break(e);  // (the wait is not part of the next stage)
        }
        // winner-take-all: fused into the last path kernel (debug 2), or -- default -- a
        // separate pass over S with one lane per pixel (k_wta_t)
        const bool last = pass == p.npass - 1 && g.mode == 1 && p.fused_wta && !p.rows4;
        SweepArgs a{ydir, xdir, p.R, C, S, (const int16_t *)bl, wta, e->keep_aggr, e->debug, nullptr, nullptr, nullptr, p.nbands};
        ChainFrames fr;
        if (p.chain) {
            // one record serves both passes (they follow each other on the stream)
            fr.nf = 1;
            fr.C[0] = C;
            fr.S[0] = S;
            fr.bnd[0] = (int16_t *)e->bndL.p;
            fr.hr[0] = g.hr;
            fr.raw[0] = (uint4 *)e->wta_raw.p;
            a.ctl = (uint32_t *)e->chain_ctl.p;
            a.err = (uint32_t *)e->chain_err.p;
            HIP_TRY(hipMemsetAsync(e->chain_ctl.p, 0, chain_ctl_bytes(1, p.nbands), st));
            stage_break(e);
        }
        const char *name = p.nvol == 5 ? "paths5" : p.chain ? (pass == 0 ? "chain_dn" : "chain_up")
                                                             : (pass == 0 ? "sweep_dn" : (p.fused_wta ? "sweep_up_wta" : "sweep_up"));
        rc = run_stage(e, name, st, [&]() -> int {
            if (p.nvol == 5) {
                int16_t *const Sv[5] = {S, (int16_t *)e->aggr2.p, (int16_t *)e->aggr3.p, (int16_t *)e->aggr4.p, (int16_t *)e->aggr5.p};
                launch_paths5(g, p.GWs, C, Sv, st);
            } else if (p.rows4) {
                // per-row state written by the grouped pre-pass: role-major; by the single-direction kernel (debug 16): band layout
                launch_vert3(g, p.GWs, pass == 0, xdir, C, S, bl, p.prepass_g ? 1 : 0, st);
                // only the in-row direction is a recurrence (k_rows_g, S +=) -- unless it runs on a stream of its own
                if (p.nvol < 3) launch_rows_grouped(g, g.H, p.GWs, xdir, PATH_ACCUM, C, S, 1, wta, st);
            } else if (p.chain) {
                const int cm = pass == 0 ? SWEEP_FIRST : (p.wta_split ? SWEEP_REDUCE : SWEEP_ACCUM);
                if (int r = launch_chain(g, a, fr, cm, chain_window(g, p.R, p.nbands, 1, e->chain_wgs), st, p.axis)) return r;
            } else if (int r = launch_sweep(g, a, pass == 0 ? SWEEP_FIRST : (last ? SWEEP_LAST : SWEEP_ACCUM), p.nbands, st, p.axis)) {
                return r;
            }
            return 1;
        });
        if (rc) return rc;
    }
    return SGM_OK;
}

// MODE_SGBM's fifth path joins S: the main stream waits for the volumes of the auxiliary streams, or the path runs here
static int stage_join(sgm_engine *e, const Plan &p)
{
    if (p.nvol == 2 || p.nvol == 3) {
        HIP_TRY(hipStreamWaitEvent(e->stream, e->ev_join, 0));
        if (p.nvol == 3) HIP_TRY(hipStreamWaitEvent(e->stream, e->ev_join2, 0));
        stage_break(e);
        return SGM_OK;
    }
    if (!p.path_w_main) return SGM_OK;
    const Geom &g = e->g;
    return run_stage(e, p.fused_wta ? "path_W_wta" : "path_W", e->stream, [&] {
        const int pm = p.fused_wta ? PATH_LAST : PATH_ACCUM;
        const int16_t *C = (const int16_t *)e->cost.p;
        int16_t *S = (int16_t *)e->aggr.p;
        if (p.path_w_lines) launch_path(g, -1, 0, pm, C, S, e->keep_aggr, (uint2 *)e->wta.p, e->stream);
        else launch_rows_grouped(g, g.H, p.GWs, -1, pm, C, S, e->keep_aggr, (uint2 *)e->wta.p, e->stream);
        return 1;
    });
}

static int stage_wta(sgm_engine *e, const Plan &p)
{
    if (p.fused_wta) return SGM_OK;
    const Geom &g = e->g;
    if (p.wta_split)  // the sweep left raw records: one thread per pixel decides (the stage keeps its name and its one launch)
        return run_stage(e, "wta", e->stream, [&] {
            hipLaunchKernelGGL(k_wta_select, dim3((g.W1 + 255) / 256, g.H), dim3(256), 0, e->stream, g, (const uint4 *)e->wta_raw.p,
                               (uint2 *)e->wta.p, uniq_recip(g.uniq));
            return 1;
        });
    uint8_t *conf = e->conf.on ? (uint8_t *)e->conf.raw.p : nullptr;
    return run_stage(e, conf ? "wta_conf" : "wta", e->stream, [&] {
        int16_t *const Sv[5] = {(int16_t *)e->aggr.p, p.nvol >= 2 ? (int16_t *)e->aggr2.p : nullptr,
                                p.nvol >= 3 ? (int16_t *)e->aggr3.p : nullptr, p.nvol >= 4 ? (int16_t *)e->aggr4.p : nullptr,
                                p.nvol >= 5 ? (int16_t *)e->aggr5.p : nullptr};
        if (int rc = launch_wta(g, p.nvol, Sv, (uint2 *)e->wta.p, conf, e->stream)) return rc;
        if (e->keep_aggr) {  // the volume a caller inspects is the whole sum
            const int64_t n8 = (int64_t)g.rowsz * g.H / 8;  // rowsz = W1 * D is a multiple of 16
            for (int k = 1; k < 5; k++)
                if (Sv[k]) hipLaunchKernelGGL(k_add_sat, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, e->stream, Sv[0], (const int16_t *)Sv[k], n8);
        }
        return 1;
    });
}

// right view, sub-pixel, LR check
static int stage_select(sgm_engine *e)
{
    const Geom &g = e->g;
    return run_stage(e, "select_lr", e->stream, [&]() -> int {
        const size_t lds = (size_t)g.W * 4;
        if (lds > 48 * 1024) HIP_TRY(hipFuncSetAttribute((const void *)k_select, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k_select, dim3(g.H), dim3(256), lds, e->stream, g, (const uint2 *)e->wta.p, (int16_t *)e->disp_raw.p);
        return 1;
    });
}

// 3x3 median, then the speckle filter on the output
static int stage_median_speckle(sgm_engine *e, const Plan &p, int16_t *d_disp)
{
    const int H = e->g.H, W = e->g.W;
    int rc = run_stage(e, "median3", e->stream, [&] {
        // the result goes to the median tap AND to the output buffer (the speckle filter works in place there)
        hipLaunchKernelGGL(k_median3, dim3((W + 255) / 256, H), dim3(256), 0, e->stream, (const int16_t *)e->disp_raw.p,
                           (int16_t *)e->disp_med.p, d_disp, H, W);
        return 1;
    });
    if (rc || !p.speckle) return rc;
    const sgm_params &q = e->params;
    return run_stage(e, "speckle", e->stream, [&] {
        const int r = run_speckles(e, d_disp, H, W, (q.minDisparity - 1) * 16, q.speckleWindowSize, 16 * q.speckleRange);
        return r ? r : 4;
    });
}

// SGM_OPT_CONFIDENCE: conf.fin = conf.raw masked by the final map, behind the speckle filter on the pair's stream; into the
// engine's buffer, or to the pointer bound for this pair (sgm_bind_confidence_device)
static int stage_confidence(sgm_engine *e, const int16_t *d_disp, uint8_t *d_conf)
{
    const int64_t n = (int64_t)e->g.H * e->g.W;
    uint8_t *out = d_conf ? d_conf : (uint8_t *)e->conf.fin.p;
    e->conf.last = d_conf ? 2 : 1;
    return run_stage(e, "conf", e->stream, [&] {
        const uint8_t *raw = (const uint8_t *)e->conf.raw.p;
        const bool vec = (((uintptr_t)raw | (uintptr_t)out) & 3) == 0 && ((uintptr_t)d_disp & 7) == 0;
        if (vec)
            hipLaunchKernelGGL(k_conf_final<true>, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, e->stream, raw, d_disp,
                               e->g.invalid_scaled, out, n);
        else
            hipLaunchKernelGGL(k_conf_final<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e->stream, raw, d_disp,
                               e->g.invalid_scaled, out, n);
        return 1;
    });
}

// SGM_OPT_RIGHT_VIEW: the right-view map behind the left map's epilogue on the pair's stream (kernels_right.h) -- diagonal
// winner-take-all over the volumes the left one read, sub-pixel step + right-to-left check against the left WTA record,
// then the left map's own median and speckle stages (the speckle scratch is free again: same stream).  The final map goes
// into the engine's buffer, or to the pointer bound for this pair (sgm_bind_right_device).
static int stage_right_view(sgm_engine *e, const Plan &p, int16_t *d_rmap)
{
    const Geom &g = e->g;
    const int H = g.H, W = g.W;
    int16_t *raw = (int16_t *)e->right.raw.p, *out = d_rmap ? d_rmap : (int16_t *)e->right.fin.p;
    e->right.last = d_rmap ? 2 : 1;
    int rc;
    if (g.W1 <= 0) {  // no matched column: no volume, nothing to scan
        const int64_t npx = (int64_t)H * W;
        rc = run_stage(e, "right_fill_invalid", e->stream, [&] {
            hipLaunchKernelGGL(k_fill_i16, dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, e->stream, raw, npx, (int16_t)g.invalid_scaled);
            return 1;
        });
        if (rc) return rc;
    } else {
        rc = run_stage(e, "right_wta", e->stream, [&] {
            RightVols v{};
            // (SGM_OPT_KEEP_AGGR: stage_wta has folded the other volumes into S already)
            v.nv = e->keep_aggr ? 1 : p.nvol;
            const DevBuf *vol[5] = {&e->aggr, &e->aggr2, &e->aggr3, &e->aggr4, &e->aggr5};
            for (int k = 0; k < v.nv; k++) v.S[k] = (const int16_t *)vol[k]->p;
            hipLaunchKernelGGL(k_right_wta, dim3((g.W1 + RV_T - 1) / RV_T, H), dim3(RV_T), 0, e->stream, g, v, (uint2 *)e->rrec.p);
            return 1;
        });
        if (rc) return rc;
        rc = run_stage(e, "right_check", e->stream, [&]() -> int {
            const size_t lds = (size_t)W * 2;
            if (lds > 48 * 1024) HIP_TRY(hipFuncSetAttribute((const void *)k_right_check, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(k_right_check, dim3(H), dim3(256), lds, e->stream, g, (const uint2 *)e->wta.p, (const uint2 *)e->rrec.p, raw);
            return 1;
        });
        if (rc) return rc;
    }
    rc = run_stage(e, "right_median3", e->stream, [&] {
        hipLaunchKernelGGL(k_median3, dim3((W + 255) / 256, H), dim3(256), 0, e->stream, (const int16_t *)raw, out, (int16_t *)nullptr, H, W);
        return 1;
    });
    if (rc || !p.speckle) return rc;
    const sgm_params &q = e->params;
    return run_stage(e, "right_speckle", e->stream, [&] {
        const int r = run_speckles(e, out, H, W, (q.minDisparity - 1) * 16, q.speckleWindowSize, 16 * q.speckleRange);
        return r ? r : 4;
    });
}

// io.conf: SGM_OPT_CONFIDENCE only -- where this pair's final confidence map goes (null: the engine's own buffer)
// io.rmap: SGM_OPT_RIGHT_VIEW only -- likewise for this pair's final right-view map
// SGM_OPT_COST: the census cost is built for gray pairs (include/sgm_hip.h); asked at compute time, before anything is
// allocated or enqueued, so the engine stays usable
static int census_refused(const sgm_engine *e)
{
    if (e && e->cost_fn == SGM_COST_CENSUS && e->cn == 3)
        return set_err(SGM_ERR_UNSUPPORTED, "SGM_OPT_COST = SGM_COST_CENSUS with SGM_OPT_CHANNELS = 3: the census cost takes single-channel images");
    return SGM_OK;
}

static int run_compute(sgm_engine *e, const PairIO &io, int H, int W, int64_t stride, int phases = PH_ALL)
{
    const uint8_t *d_left = (const uint8_t *)io.left, *d_right = (const uint8_t *)io.right;
    int16_t *d_disp = (int16_t *)io.disp_i16;
    if (!e || !d_left || !d_right || !d_disp) return set_err(SGM_ERR_INVALID_ARG, "null pointer");
    if (census_refused(e)) return SGM_ERR_UNSUPPORTED;
    if (H <= 0 || W < 2 || stride < (int64_t)W * e->cn)
        return set_err(SGM_ERR_INVALID_ARG, "bad shape H=%d W=%d stride=%lld (channels %d)", H, W, (long long)stride, e->cn);
    if (W > 32767 || H > 32767) return set_err(SGM_ERR_UNSUPPORTED, "image larger than 32767 in a dimension");
    HIP_TRY(hipSetDevice(e->device));
    Geom g0;
    int rc = normalise(&e->params, H, W, &g0);
    if (rc) return rc;
    const Plan p = make_plan(e, g0, H);
    if (phases != PH_ALL && !p.chain) return set_err(SGM_ERR_INVALID_ARG, "phased compute needs the chained schedule");
    if ((rc = ensure_plan_buffers(e, p, H, W))) return rc;
    const bool do_pre = (phases & PH_PRE) != 0, do_mid = (phases & PH_MID) != 0, do_post = (phases & PH_POST) != 0;
    if (do_pre) {
        stage_reset(e);
        e->plan = p;
        e->conf.last = e->right.last = 0;
    } else {
        stage_break(e);
    }
    if (do_pre && !e->hr_accumulate) {
        HIP_TRY(hipMemsetAsync(e->headroom.p, 0, 8, e->stream));  // headroom record of this compute (sgm_get_headroom)
        // a compute of its own forgets the internal engines of an earlier batch call: their records belong to that call
        if (!e->in_batch) e->last_group = e->last_peers = 0;
    }

    if (e->g.W1 <= 0) {
        // no column can be matched: the whole map is invalid (upstream early-out), then median
        // and speckle act on a constant image
        const int64_t npx = (int64_t)H * W;
        if (e->conf.on) {
            HIP_TRY(hipMemsetAsync(e->conf.raw.p, 0, (size_t)npx, e->stream));
            stage_break(e);
        }
        rc = run_stage(e, "fill_invalid", e->stream, [&] {
            hipLaunchKernelGGL(k_fill_i16, dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, e->stream, (int16_t *)e->disp_raw.p, npx,
                               (int16_t)e->g.invalid_scaled);
            return 1;
        });
        if (rc) return rc;
    } else {
        if (do_pre && ((rc = stage_features(e, p, d_left, d_right, stride)) || (rc = stage_cost(e, p)) || (rc = fork_in_row(e, p))))
            return rc;
        if (do_mid && (rc = p.v1 ? paths_v1(e, p) : paths_fused(e, p))) return rc;
        if (!do_post) return SGM_OK;
        if ((rc = stage_join(e, p))) return rc;
        if (e->conf.on) {  // columns no disparity can be matched at keep 0: k_wta_conf_t writes minX1 .. minX1 + W1 only
            HIP_TRY(hipMemsetAsync(e->conf.raw.p, 0, (size_t)H * W, e->stream));
            stage_break(e);
        }
        if ((rc = stage_wta(e, p)) || (rc = stage_select(e))) return rc;
    }
    if ((rc = stage_median_speckle(e, p, d_disp))) return rc;
    if (e->conf.on && (rc = stage_confidence(e, d_disp, io.conf))) return rc;
    return e->right.on ? stage_right_view(e, p, io.rmap) : SGM_OK;
}

static int run_to_float(sgm_engine *e, const int16_t *d_disp, int64_t n, float *d_out)
{
    hipLaunchKernelGGL(k_disp_to_float, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e->stream, d_disp, d_out, n);
    KCHECK();
    return SGM_OK;
}

static int run_reproject(sgm_engine *e, const float *d_disp, int H, int W, const double Q[16], int handle_missing,
                         float *d_xyz)
{
    if (!Q) return set_err(SGM_ERR_INVALID_ARG, "Q is null");
    QMat q;
    memcpy(q.q, Q, sizeof(q.q));
    uint32_t *mk = nullptr;
    if (handle_missing) {
        int rc = e->minkey.ensure(4);
        if (rc) return rc;
        mk = (uint32_t *)e->minkey.p;
        HIP_TRY(hipMemsetAsync(mk, 0xff, 4, e->stream));
        const int64_t n = (int64_t)H * W;
        const unsigned nb = (unsigned)std::min<int64_t>((n + 255) / 256, 2048);
        hipLaunchKernelGGL(k_min_f32, dim3(nb), dim3(256), 0, e->stream, d_disp, n, mk);
    }
    dim3 grid((W + 255) / 256, H), block(256);
    hipLaunchKernelGGL(k_reproject, grid, block, 0, e->stream, d_disp, H, W, q, (const uint32_t *)mk, d_xyz);
    KCHECK();
    return SGM_OK;
}

// float scaling + reprojection of one pair on its engine's stream (shared by the single-pair and the batch entry)
static int run_float_xyz(sgm_engine *e, const int16_t *di, int H, int W, const double Q[16], void *d_disp_f32, void *d_xyz_f32)
{
    const int64_t n = (int64_t)H * W;
    if (!d_disp_f32 && !d_xyz_f32) return SGM_OK;
    if (d_xyz_f32) {
        if (!Q) return set_err(SGM_ERR_INVALID_ARG, "Q is null");
        QMat q;
        memcpy(q.q, Q, sizeof(q.q));
        return run_stage(e, "float_xyz", [&] {
            hipLaunchKernelGGL(k_float_xyz, dim3((W + 255) / 256, H), dim3(256), 0, e->stream, di, H, W, q,
                               (float *)d_disp_f32, (float *)d_xyz_f32);
            return 1;
        });
    }
    return run_stage(e, "to_float", [&] {
        const int rc = run_to_float(e, di, n, (float *)d_disp_f32);
        return rc ? rc : 1;
    });
}

// ---- exported C ABI -------------------------------------------------------------------------------
extern "C" {

int sgm_abi_version(void) { return SGM_ABI_VERSION; }

const char *sgm_last_error(void) { return g_err; }

int sgm_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int sgm_geometry(const sgm_params *params, int W, int *minX1, int *W1)
{
    if (!params) return set_err(SGM_ERR_INVALID_ARG, "params is null");
    Geom g;
    int rc = normalise(params, 1, W, &g);
    if (rc) return rc;
    if (minX1) *minX1 = g.minX1;
    if (W1) *W1 = g.W1;
    return SGM_OK;
}

// csrc/sgm_debug.h: the plan of one compute, read out on the host.  The options go through sgm_set_option into an engine
// that is never handed out (it owns no stream and no buffer), then the very calls run_compute makes.
static int debug_plan_on(const sgm_params *params, int H, int W, int channels, int schedule, int sweep_rows, int prepass_rows,
                         int debug, int frames, int confidence, int right_view, int cost, sgm_debug_plan_t *out)
{
    if (!params || !out) return set_err(SGM_ERR_INVALID_ARG, "params/out is null");
    if (H <= 0 || W < 2 || W > 32767 || H > 32767) return set_err(SGM_ERR_INVALID_ARG, "bad shape H=%d W=%d", H, W);
    sgm_engine e;
    e.params = *params;
    int rc;
    if ((rc = sgm_set_option(&e, SGM_OPT_CHANNELS, channels)) || (rc = sgm_set_option(&e, SGM_OPT_SCHEDULE, schedule)) ||
        (rc = sgm_set_option(&e, SGM_OPT_SWEEP_ROWS, sweep_rows)) || (rc = sgm_set_option(&e, SGM_OPT_PREPASS_ROWS, prepass_rows)) ||
        (rc = sgm_set_option(&e, SGM_OPT_DEBUG, debug)) || (rc = sgm_set_option(&e, SGM_OPT_CONFIDENCE, confidence)) ||
        (rc = sgm_set_option(&e, SGM_OPT_RIGHT_VIEW, right_view)) || (rc = sgm_set_option(&e, SGM_OPT_COST, cost)) ||
        (rc = census_refused(&e)))
        return rc;
    Geom g;
    if ((rc = normalise(&e.params, H, W, &g))) return rc;
    const Plan p = make_plan(&e, g, H);
    const bool small_d = p.rows4 && p.GWs < 64;
    out->W1 = g.W1;
    out->minX1 = g.minX1;
    out->NP = g.NP;
    out->partial = small_d ? with_gw(p.GWs, g.D, [](auto, auto part) { return (int)decltype(part)::value; })
                           : (int)np_partial(g);
    out->byte_cost = p.byte_cost;
    out->pix_px = p.pix_px;
    out->GWc = p.GWc;
    out->RBb = p.RBb;
    out->vsum_ring = p.vsum_ring;
    out->rows4 = p.rows4;
    out->GWs = p.GWs;
    out->chain = p.chain;
    out->R = p.R;
    out->nbands = p.nbands;
    out->fused_prepass = p.fused_prepass;
    out->prepass_g = p.prepass_g;
    out->pre_nch = p.pre_nch;
    out->pre_rows = p.pre_rows;
    out->overlap = p.overlap;
    out->fused_wta = p.fused_wta;
    out->nvol = p.nvol;
    out->path_w_main = p.path_w_main;
    out->speckle = p.speckle;
    out->chain_window = p.chain && g.W1 > 0 ? chain_window(g, p.R, p.nbands, std::max(frames, 1), 0) : 0;
    return SGM_OK;
}

int sgm_debug_plan(const sgm_params *params, int H, int W, int channels, int schedule, int sweep_rows, int prepass_rows,
                   int debug, int frames, sgm_debug_plan_t *out)
{
    return debug_plan_on(params, H, W, channels, schedule, sweep_rows, prepass_rows, debug, frames, 0, 0, SGM_COST_BT, out);
}

// the same readout with the options that change the plan but came after sgm_debug_plan's signature was fixed
int sgm_debug_plan_opts(const sgm_params *params, int H, int W, int channels, int schedule, int sweep_rows, int prepass_rows,
                        int debug, int frames, int confidence, int right_view, sgm_debug_plan_t *out)
{
    return debug_plan_on(params, H, W, channels, schedule, sweep_rows, prepass_rows, debug, frames, confidence, right_view, SGM_COST_BT, out);
}

// ... and with SGM_OPT_COST (0 gives what sgm_debug_plan_opts gives; census with 3 channels: the error code of the compute)
int sgm_debug_plan_cost(const sgm_params *params, int H, int W, int channels, int schedule, int sweep_rows, int prepass_rows,
                        int debug, int frames, int confidence, int right_view, int cost, sgm_debug_plan_t *out)
{
    return debug_plan_on(params, H, W, channels, schedule, sweep_rows, prepass_rows, debug, frames, confidence, right_view, cost, out);
}

// csrc/sgm_debug.h: the split winner-take-all -- its threshold as the kernels compute it, whether a plan takes it, and what an
// engine holds for it
int sgm_debug_uniq_threshold(int minS, int uniquenessRatio)
{
    if (minS < 0 || minS > SGM_MAX_COST || uniquenessRatio < 0 || uniquenessRatio > 99) return -1;
    return (int)uniq_t1((uint32_t)minS, uniq_recip(uniquenessRatio));
}
int sgm_debug_wta_split(const sgm_params *params, int H, int W, int schedule, int sweep_rows, int debug, int confidence, int right_view,
                        int keep_aggr)
{
    if (!params) return set_err(SGM_ERR_INVALID_ARG, "params is null");
    if (H <= 0 || W < 2 || W > 32767 || H > 32767) return set_err(SGM_ERR_INVALID_ARG, "bad shape H=%d W=%d", H, W);
    sgm_engine e;
    e.params = *params;
    int rc;
    if ((rc = sgm_set_option(&e, SGM_OPT_SCHEDULE, schedule)) || (rc = sgm_set_option(&e, SGM_OPT_SWEEP_ROWS, sweep_rows)) ||
        (rc = sgm_set_option(&e, SGM_OPT_DEBUG, debug)) || (rc = sgm_set_option(&e, SGM_OPT_CONFIDENCE, confidence)) ||
        (rc = sgm_set_option(&e, SGM_OPT_RIGHT_VIEW, right_view)) || (rc = sgm_set_option(&e, SGM_OPT_KEEP_AGGR, keep_aggr)))
        return rc;
    Geom g;
    if ((rc = normalise(&e.params, H, W, &g))) return rc;
    return make_plan(&e, g, H).wta_split ? 1 : 0;
}
int sgm_debug_wta_select_n(int D, int uniquenessRatio, const uint32_t *raw, int n, uint32_t *wta)
{
    if (D != 128 && D != 256) return set_err(SGM_ERR_INVALID_ARG, "split winner-take-all: D = 128 or 256, not %d", D);
    if (uniquenessRatio < 0 || uniquenessRatio > 99) return set_err(SGM_ERR_INVALID_ARG, "uniquenessRatio %d outside 0..99", uniquenessRatio);
    if (n < 0 || (n > 0 && (!raw || !wta))) return set_err(SGM_ERR_INVALID_ARG, "raw/wta is null or n < 0");
    const UniqRecip q = uniq_recip(uniquenessRatio);
    for (int i = 0; i < n; i++) wta_select_words(D / 128, q, raw[4 * i], raw[4 * i + 1], raw[4 * i + 2], raw[4 * i + 3], wta[2 * i], wta[2 * i + 1]);
    return SGM_OK;
}
long long sgm_debug_wta_raw_bytes(const sgm_engine *e)
{
    if (!e) return -1;
    long long n = (long long)e->wta_raw.cap;
    for (const sgm_engine *q : e->group) n += (long long)q->wta_raw.cap;
    return n;
}

int sgm_create(const sgm_params *params, int device_id, void *stream, sgm_engine **out)
{
    if (!params || !out) return set_err(SGM_ERR_INVALID_ARG, "params/out is null");
    *out = nullptr;
    Geom g;
    int rc = normalise(params, 1, 64, &g);  // parameter validation only
    if (rc) return rc;
    int n = 0;
    hipError_t he = hipGetDeviceCount(&n);
    if (he != hipSuccess || n <= 0)
        return set_err(SGM_ERR_NO_DEVICE, "no HIP device available (%s); this library has no CPU fallback",
                       he == hipSuccess ? "device count 0" : hipGetErrorString(he));
    if (device_id < 0 || device_id >= n) return set_err(SGM_ERR_NO_DEVICE, "device_id %d out of range [0,%d)", device_id, n);
    HIP_TRY(hipSetDevice(device_id));
    sgm_engine *e = new (std::nothrow) sgm_engine();
    if (!e) return set_err(SGM_ERR_NOMEM, "out of host memory");
    e->params = *params;
    e->device = device_id;
    if (stream) {
        e->stream = (hipStream_t)stream;
    } else {
        hipError_t se = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking);
        if (se != hipSuccess) {
            delete e;
            return set_err(SGM_ERR_HIP, "hipStreamCreate failed: %s", hipGetErrorString(se));
        }
        e->own_stream = true;
    }
    *out = e;
    return SGM_OK;
}

// every device buffer of an engine (the engine stays usable: buffers come back on the next call that needs them)
static void release_buffers(sgm_engine *e)
{
    each_devbuf(e, [](DevBuf &b) { (void)b.release(); });
    e->g.hr = nullptr;
}

// SGM_OPT_POISON (csrc/sgm_debug.h): every byte of every device buffer the engine owns -- [p, p + cap) of each DevBuf
// member, which is also the whole buffer under SGM_DEBUG_ALLOC=1 -- set to `byte`, in the order of the engine's stream, and
// the same for the engines behind it (peer, peer2, group), each on its own stream.  Every stream is waited for at the end:
// the batch entries order the engines of a group with events of their own, not with the caller's stream.
// chain_err is the one member that is state by contract (the sticky give-up flag that check_chain reports and clears); it is
// LEFT ALONE, neither filled nor re-cleared.  (Every buffer: the walk over SGM_ENGINE_DEVBUFS, tests/test_history_walks.py.)
static int poison_buffers(sgm_engine *e, int byte)
{
    HIP_TRY(hipSetDevice(e->device));
    hipError_t he = hipSuccess;
    each_devbuf(e, [&](DevBuf &b) {
        if (&b != &e->chain_err && b.p && b.cap && he == hipSuccess) he = hipMemsetAsync(b.p, byte, b.cap, e->stream);
    });
    if (he != hipSuccess) return set_err(SGM_ERR_HIP, "SGM_OPT_POISON: hipMemsetAsync failed: %s", hipGetErrorString(he));
    int rc;
    if (e->peer && (rc = poison_buffers(e->peer, byte))) return rc;
    if (e->peer2 && (rc = poison_buffers(e->peer2, byte))) return rc;
    for (sgm_engine *q : e->group)
        if ((rc = poison_buffers(q, byte))) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    return SGM_OK;
}

void sgm_destroy(sgm_engine *e)
{
    if (!e) return;
    (void)hipSetDevice(e->device);
    (void)hipStreamSynchronize(e->stream);
    if (e->copy_in) {
        (void)hipStreamSynchronize(e->copy_in);
        (void)hipStreamDestroy(e->copy_in);
    }
    if (e->copy_out) {
        (void)hipStreamSynchronize(e->copy_out);
        (void)hipStreamDestroy(e->copy_out);
    }
    release_buffers(e);
    for (hipEvent_t ev : e->events) (void)hipEventDestroy(ev);
    for (auto *evs : {e->ev_io_in, e->ev_io_used, e->ev_io_out, e->ev_io_dl})
        for (int k = 0; k < 2; k++)
            if (evs[k]) (void)hipEventDestroy(evs[k]);
    for (auto &slot : e->pin_io)
        for (HostBuf &b : slot) b.release();
    if (e->aux2) {
        (void)hipStreamSynchronize(e->aux2);
        (void)hipEventDestroy(e->ev_join2);
        (void)hipStreamDestroy(e->aux2);
    }
    if (e->aux) {
        (void)hipStreamSynchronize(e->aux);
        (void)hipEventDestroy(e->ev_fork);
        (void)hipEventDestroy(e->ev_join);
        (void)hipStreamDestroy(e->aux);
    }
    if (e->own_stream) (void)hipStreamDestroy(e->stream);
    e->pin_left.release();
    e->pin_right.release();
    e->pin_disp.release();
    e->pin_icp.release();
    if (e->ev_done) (void)hipEventDestroy(e->ev_done);
    if (e->peer) sgm_destroy(e->peer);
    if (e->peer2) sgm_destroy(e->peer2);
    for (sgm_engine *q : e->group) sgm_destroy(q);
    if (e->ev_group) (void)hipEventDestroy(e->ev_group);
    delete e;
}

int sgm_set_option(sgm_engine *e, int option, int value)
{
    if (!e) return set_err(SGM_ERR_INVALID_ARG, "engine is null");
    if (option == SGM_OPT_KEEP_AGGR) e->keep_aggr = value ? 1 : 0;
    else if (option == SGM_OPT_PROFILE) e->profile = value ? 1 : 0;
    else if (option == SGM_OPT_SCHEDULE) e->schedule = std::max(0, std::min(value, 2));
    else if (option == SGM_OPT_CHAIN_WGS) e->chain_wgs = std::max(0, value);
    else if (option == SGM_OPT_SWEEP_ROWS) e->sweep_rows = std::max(0, value);
    else if (option == SGM_OPT_DEBUG) {
        // csrc/sgm_debug.h; bit 64 (the sweep's loader skips its loads: timing only, results WRONG) must be asked for twice
        if ((value & SGM_DBG_SKIP_BOUNDARY_LOADS) && !(getenv("SGM_ALLOW_WRONG_RESULTS") && atoi(getenv("SGM_ALLOW_WRONG_RESULTS")) == 1))
            return set_err(SGM_ERR_INVALID_ARG, "debug bit 64 makes results wrong (timing experiments only): set SGM_ALLOW_WRONG_RESULTS=1 to use it");
        e->debug = value;
    }
    else if (option == SGM_OPT_PREPASS_ROWS) e->prepass_rows = std::max(0, value);
    else if (option == SGM_OPT_GROUP_MAX) e->group_max = std::max(0, std::min(value, CHAIN_MAX_FRAMES));
    else if (option == SGM_OPT_CHANNELS) {
        if (value != 1 && value != 3)
            return set_err(SGM_ERR_INVALID_ARG, "SGM_OPT_CHANNELS %d: only 1 and 3 interleaved 8-bit channels are supported", value);
        e->cn = value;
    }
    else if (option == SGM_OPT_COST) {
        if (value != SGM_COST_BT && value != SGM_COST_CENSUS)
            return set_err(SGM_ERR_INVALID_ARG, "SGM_OPT_COST %d: SGM_COST_BT (0) or SGM_COST_CENSUS (1)", value);
        e->cost_fn = value;
    }
    else if (option == SGM_OPT_CONFIDENCE || option == SGM_OPT_RIGHT_VIEW) {
        SideMap &m = option == SGM_OPT_CONFIDENCE ? e->conf : e->right;
        if (value != 0 && value != 1) return set_err(SGM_ERR_INVALID_ARG, "%s %d: 0 (off) or 1 (on)", m.opt_name, value);
        m.on = value;
        if (!value) m.bind.clear();
    }
    else if (option == SGM_OPT_POISON) {
        // csrc/sgm_debug.h: 0..255 fills every buffer now and arms DevBuf::ensure; anything else disarms
        g_poison_byte = value >= 0 && value <= 255 ? value : -1;
        if (g_poison_byte >= 0) return poison_buffers(e, g_poison_byte);
    }
    else return set_err(SGM_ERR_INVALID_ARG, "unknown option %d", option);
    return SGM_OK;
}

// Chained sweeps bound every wait for another workgroup (kernels_sweep.h: ChainWait); a wait that gave up leaves a
// flag beside the control words and wrong results in whatever was computed since the last check.  The flag is looked at
// wherever the host synchronises with the engine's stream anyway, and by sgm_check for callers that order the engine's
// stream with events of their own (dist.IngestPipeline, bench.py); once reported it is cleared, so that the engine is
// usable again (the next launch zeroes its control words as every launch does).
static int check_chain(sgm_engine *e)
{
    if (!e->chain_err.p) return SGM_OK;
    uint32_t f = 0;
    HIP_TRY(hipMemcpy(&f, e->chain_err.p, 4, hipMemcpyDeviceToHost));
    if (f) {
        HIP_TRY(hipMemset(e->chain_err.p, 0, 4));
        return set_err(SGM_ERR_HIP, "chained sweep: a workgroup gave up waiting for the band above it (results since the last check are invalid)");
    }
    return SGM_OK;
}

int sgm_synchronize(sgm_engine *e)
{
    if (!e) return set_err(SGM_ERR_INVALID_ARG, "engine is null");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return check_chain(e);
}

int sgm_check(sgm_engine *e)
{
    if (!e) return set_err(SGM_ERR_INVALID_ARG, "engine is null");
    HIP_TRY(hipSetDevice(e->device));
    return check_chain(e);
}

// gives back what the engine can build again: the internal engines of sgm_pipeline_batch_device / sgm_compute_batch (a
// group of 4K D=256 pairs holds about 9 GB per pair) and the page-locked staging buffers
int sgm_trim(sgm_engine *e)
{
    if (!e) return set_err(SGM_ERR_INVALID_ARG, "engine is null");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (sgm_engine *q : e->group) sgm_destroy(q);
    e->group.clear();
    e->last_group = 0;
    if (e->peer) sgm_destroy(e->peer);
    if (e->peer2) sgm_destroy(e->peer2);
    e->peer = e->peer2 = nullptr;
    e->last_peers = 0;
    e->pin_left.release();
    e->pin_right.release();
    e->pin_disp.release();
    e->pin_icp.release();
    for (auto &slot : e->pin_io)
        for (HostBuf &b : slot) b.release();
    for (DevBuf *b : {&e->wls_u, &e->wls_v, &e->wls_c, &e->lrc_f, &e->vox_tab, &e->vox_slot, &e->mesh_code, &e->mesh_num, &e->mesh_faces, &e->mesh_nrm,
                      &e->rad_tab, &e->rad_sorted, &e->rad_pt, &e->rad_keep, &e->rad_cnt, &e->rad_idx, &e->stat_mean, &e->cov_nrm, &e->cov_curv, &e->cov_mom,
                      &e->db_parent, &e->db_near, &e->db_rank, &e->db_lab, &e->db_sizes, &e->pl_pts, &e->pl_hyp, &e->pl_cnt, &e->pl_inl, &e->pl_dist,
                      &e->icp_corr, &e->icp_d2, &e->icp_part, &e->icp_txyz, &e->icp_tdisp, &e->icp_tnrm,
                      &e->tsdf_sum, &e->tsdf_w, &e->tsdf_rgb, &e->tsdf_cnt, &e->tsdf_off})
        (void)b->release();   // the filter's planes, the LR confidence's factors, the voxel table, the mesh's maps, the staged normals, the radius search's table, records and staging, the staged means of the statistical one and the staged normals, curvatures and moments of the covariance normals, the links, ranks and staging of the clustering and the valid list, hypotheses, counts and staging of the plane segmentation and the correspondences, partial sums and staged target of the registration come back on the next call
    return check_chain(e);
}

// The binding of a bind entry belongs to the next image call, whatever becomes of that call: taken off the engine here.
// *out: the n pointers (empty: none bound).
static int take_binding(SideMap &m, int n, std::vector<void *> *out)
{
    out->clear();
    out->swap(m.bind);
    if (!out->empty() && (int)out->size() != n)
        return set_err(SGM_ERR_INVALID_ARG, "%s bound %d maps, this call has %d pair(s)", m.bind_name, (int)out->size(), n);
    return SGM_OK;
}
// an image call takes BOTH bindings before it looks at either result
static int take_bindings(sgm_engine *e, int n, std::vector<void *> *conf, std::vector<void *> *right)
{
    const int brc = take_binding(e->conf, n, conf), rrc = take_binding(e->right, n, right);
    return brc ? brc : rrc;
}
// the host entries: a binding is for the device entries (the host entries' maps are read through the taps)
static void clear_bindings(sgm_engine *e) { e->conf.bind.clear(), e->right.bind.clear(); }
// pair i's pointer of a binding taken (null: none bound)
static void *bound_at(const std::vector<void *> &b, int i) { return b.empty() ? nullptr : b[i]; }

static int bind(SideMap &m, int N, void *const *ptrs)
{
    m.bind.clear();
    if (N == 0) return SGM_OK;
    if (N < 0 || !ptrs) return set_err(SGM_ERR_INVALID_ARG, "bad argument");
    if (!m.on) return set_err(SGM_ERR_INVALID_ARG, "%s needs %s=1", m.bind_name, m.opt_name);
    for (int i = 0; i < N; i++)
        if (!ptrs[i]) return set_err(SGM_ERR_INVALID_ARG, "null %s pointer for pair %d", m.noun, i);
    m.bind.assign(ptrs, ptrs + N);
    return SGM_OK;
}

int sgm_bind_right_device(sgm_engine *e, int N, void *const *d_right_i16)
{
    return e ? bind(e->right, N, d_right_i16) : set_err(SGM_ERR_INVALID_ARG, "engine is null");
}

int sgm_bind_confidence_device(sgm_engine *e, int N, void *const *d_conf_u8)
{
    return e ? bind(e->conf, N, d_conf_u8) : set_err(SGM_ERR_INVALID_ARG, "engine is null");
}

int sgm_compute_device(sgm_engine *e, const void *d_left, const void *d_right, int H, int W, int64_t stride_bytes,
                       void *d_disp_i16)
{
    if (!e) return set_err(SGM_ERR_INVALID_ARG, "null pointer");
    std::vector<void *> bound, rbound;
    if (int rc = take_bindings(e, 1, &bound, &rbound)) return rc;
    const PairIO io{d_left, d_right, d_disp_i16, nullptr, nullptr, (uint8_t *)bound_at(bound, 0), (int16_t *)bound_at(rbound, 0)};
    return run_compute(e, io, H, W, stride_bytes);
}

int sgm_disp_to_float_device(sgm_engine *e, const void *d_disp_i16, int64_t n, void *d_out_f32)
{
    if (!e || !d_disp_i16 || !d_out_f32 || n <= 0) return set_err(SGM_ERR_INVALID_ARG, "bad argument");
    HIP_TRY(hipSetDevice(e->device));
    return run_to_float(e, (const int16_t *)d_disp_i16, n, (float *)d_out_f32);
}

int sgm_reproject_device(sgm_engine *e, const void *d_disp_f32, int H, int W, const double Q[16], int handle_missing,
                         void *d_xyz_f32)
{
    if (!e || !d_disp_f32 || !d_xyz_f32 || H <= 0 || W <= 0) return set_err(SGM_ERR_INVALID_ARG, "bad argument");
    HIP_TRY(hipSetDevice(e->device));
    return run_reproject(e, (const float *)d_disp_f32, H, W, Q, handle_missing, (float *)d_xyz_f32);
}

int sgm_valid_mask_device(sgm_engine *e, const void *d_xyz, const void *d_disp_f32, int64_t n, void *d_mask_u8)
{
    if (!e || !d_xyz || !d_disp_f32 || !d_mask_u8 || n <= 0) return set_err(SGM_ERR_INVALID_ARG, "bad argument");
    HIP_TRY(hipSetDevice(e->device));
    hipLaunchKernelGGL(k_valid_mask, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e->stream, (const float *)d_xyz,
                       (const float *)d_disp_f32, n, (uint8_t *)d_mask_u8);
    KCHECK();
    return SGM_OK;
}

// ---- rectification in front of the path (gui.py:160-164) ----------------------------------------

// (P[:, :3] * R)^-1 in double, the closed form cv::invert uses for 3x3 (lapack.cpp)
static bool rectify_inverse(const double K[9], const double *R, const double *P, int pcols, double ir[9])
{
    double A[9], Rm[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, M[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) A[r * 3 + c] = P ? P[r * pcols + c] : K[r * 3 + c];
    if (R) memcpy(Rm, R, sizeof(Rm));
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            double s = 0;
            for (int q = 0; q < 3; q++) s += A[r * 3 + q] * Rm[q * 3 + c];
            M[r * 3 + c] = s;
        }
    const double m00 = M[0], m01 = M[1], m02 = M[2], m10 = M[3], m11 = M[4], m12 = M[5], m20 = M[6], m21 = M[7], m22 = M[8];
    double d = m00 * (m11 * m22 - m12 * m21) - m01 * (m10 * m22 - m12 * m20) + m02 * (m10 * m21 - m11 * m20);
    if (d == 0.) return false;
    d = 1. / d;
    ir[0] = (m11 * m22 - m12 * m21) * d;
    ir[1] = (m02 * m21 - m01 * m22) * d;
    ir[2] = (m01 * m12 - m02 * m11) * d;
    ir[3] = (m12 * m20 - m10 * m22) * d;
    ir[4] = (m00 * m22 - m02 * m20) * d;
    ir[5] = (m02 * m10 - m00 * m12) * d;
    ir[6] = (m10 * m21 - m11 * m20) * d;
    ir[7] = (m01 * m20 - m00 * m21) * d;
    ir[8] = (m00 * m11 - m01 * m10) * d;
    return true;
}

int sgm_init_undistort_rectify_map_device(sgm_engine *e, const double K[9], const double *dist, int ndist,
                                          const double *R, const double *P, int pcols, int W, int H,
                                          void *d_map1_f32, void *d_map2_f32)
{
    if (!e || !K || !d_map1_f32 || !d_map2_f32 || W <= 0 || H <= 0) return set_err(SGM_ERR_INVALID_ARG, "bad argument");
    if (P && pcols != 3 && pcols != 4) return set_err(SGM_ERR_INVALID_ARG, "newCameraMatrix must be 3x3 or 3x4");
    RectifyArgs a;
    memset(&a, 0, sizeof(a));
    if (dist) {
        if (ndist == 14) return set_err(SGM_ERR_UNSUPPORTED, "tilted-sensor distortion terms are not supported");
        if (ndist != 4 && ndist != 5 && ndist != 8 && ndist != 12)
            return set_err(SGM_ERR_INVALID_ARG, "distCoeffs must hold 4, 5, 8 or 12 values");
        for (int i = 0; i < ndist; i++) a.k[i] = dist[i];
    }
    if (!rectify_inverse(K, R, P, pcols, a.ir)) return set_err(SGM_ERR_INVALID_ARG, "newCameraMatrix * R is singular");
    a.fx = K[0];
    a.fy = K[4];
    a.u0 = K[2];
    a.v0 = K[5];
    HIP_TRY(hipSetDevice(e->device));
    hipLaunchKernelGGL(k_rectify_map, dim3((H + 63) / 64), dim3(64), 0, e->stream, a, W, H, (float *)d_map1_f32, (float *)d_map2_f32);
    KCHECK();
    return SGM_OK;
}

int sgm_init_undistort_rectify_map(sgm_engine *e, const double K[9], const double *dist, int ndist, const double *R,
                                   const double *P, int pcols, int W, int H, float *map1_out, float *map2_out)
{
    if (!e || !map1_out || !map2_out || W <= 0 || H <= 0) return set_err(SGM_ERR_INVALID_ARG, "bad argument");
    const size_t bytes = (size_t)W * H * 4;
    int rc;
    HIP_TRY(hipSetDevice(e->device));
    if ((rc = e->rmap1.ensure(bytes)) || (rc = e->rmap2.ensure(bytes))) return rc;
    if ((rc = sgm_init_undistort_rectify_map_device(e, K, dist, ndist, R, P, pcols, W, H, e->rmap1.p, e->rmap2.p))) return rc;
    HIP_TRY(hipMemcpyAsync(map1_out, e->rmap1.p, bytes, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(map2_out, e->rmap2.p, bytes, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return SGM_OK;
}

int sgm_remap_linear_u8_device(sgm_engine *e, const void *d_src, int sH, int sW, int64_t sstride, int cn,
                               const void *d_map1_f32, const void *d_map2_f32, int dH, int dW, void *d_dst,
                               int64_t dstride)
{
    if (!e || !d_src || !d_map1_f32 || !d_map2_f32 || !d_dst || sH <= 0 || sW <= 0 || dH <= 0 || dW <= 0)
        return set_err(SGM_ERR_INVALID_ARG, "bad argument");
    if (cn < 1 || cn > 4) return set_err(SGM_ERR_UNSUPPORTED, "remap supports 1..4 interleaved 8-bit channels, got %d", cn);
    if (sstride < (int64_t)sW * cn || dstride < (int64_t)dW * cn) return set_err(SGM_ERR_INVALID_ARG, "stride smaller than a row");
    if (sH > 32767 || sW > 32767) return set_err(SGM_ERR_UNSUPPORTED, "source larger than 32767 pixels (upstream's int16 coordinates)");
    HIP_TRY(hipSetDevice(e->device));
    dim3 grid((dW + 255) / 256, dH), block(256);
    const uint8_t *s = (const uint8_t *)d_src;
    const float *m1 = (const float *)d_map1_f32, *m2 = (const float *)d_map2_f32;
    uint8_t *d = (uint8_t *)d_dst;
    switch (cn) {
    case 1: hipLaunchKernelGGL(k_remap_linear<1>, grid, block, 0, e->stream, s, sH, sW, sstride, m1, m2, dH, dW, d, dstride); break;
    case 2: hipLaunchKernelGGL(k_remap_linear<2>, grid, block, 0, e->stream, s, sH, sW, sstride, m1, m2, dH, dW, d, dstride); break;
    case 3: hipLaunchKernelGGL(k_remap_linear<3>, grid, block, 0, e->stream, s, sH, sW, sstride, m1, m2, dH, dW, d, dstride); break;
    default: hipLaunchKernelGGL(k_remap_linear<4>, grid, block, 0, e->stream, s, sH, sW, sstride, m1, m2, dH, dW, d, dstride); break;
    }
    KCHECK();
    return SGM_OK;
}

int sgm_remap_linear_u8(sgm_engine *e, const uint8_t *src, int sH, int sW, int64_t sstride, int cn, const float *map1,
                        const float *map2, int dH, int dW, uint8_t *dst)
{
    if (!e || !src || !map1 || !map2 || !dst || sH <= 0 || sW <= 0 || dH <= 0 || dW <= 0)
        return set_err(SGM_ERR_INVALID_ARG, "bad argument");
    if (cn < 1 || cn > 4) return set_err(SGM_ERR_UNSUPPORTED, "remap supports 1..4 interleaved 8-bit channels, got %d", cn);
    if (sstride < (int64_t)sW * cn) return set_err(SGM_ERR_INVALID_ARG, "stride smaller than a row");
    HIP_TRY(hipSetDevice(e->device));
    const size_t sbytes = (size_t)sH * sW * cn, mbytes = (size_t)dH * dW * 4, dbytes = (size_t)dH * dW * cn;
    int rc;
    if ((rc = e->rsrc.ensure(sbytes)) || (rc = e->rmap1.ensure(mbytes)) || (rc = e->rmap2.ensure(mbytes)) || (rc = e->rdst.ensure(dbytes)))
        return rc;
    HIP_TRY(hipMemcpy2DAsync(e->rsrc.p, (size_t)sW * cn, src, (size_t)sstride, (size_t)sW * cn, sH, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->rmap1.p, map1, mbytes, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->rmap2.p, map2, mbytes, hipMemcpyHostToDevice, e->stream));
    if ((rc = sgm_remap_linear_u8_device(e, e->rsrc.p, sH, sW, (int64_t)sW * cn, cn, e->rmap1.p, e->rmap2.p, dH, dW, e->rdst.p, (int64_t)dW * cn)))
        return rc;
    HIP_TRY(hipMemcpyAsync(dst, e->rdst.p, dbytes, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return SGM_OK;
}

// one pair through cell c13 on e
static int pipeline_one(sgm_engine *e, const PairIO &io, int H, int W, int64_t stride_bytes, const double Q[16])
{
    PairIO p = io;
    if (!p.disp_i16) {
        if (int rc = e->disp_out.ensure((size_t)H * W * 2)) return rc;
        p.disp_i16 = e->disp_out.p;
    }
    if (int rc = run_compute(e, p, H, W, stride_bytes)) return rc;
    // float scaling + reprojection in one launch (the float map is stored only if asked for)
    return run_float_xyz(e, (const int16_t *)p.disp_i16, H, W, Q, p.disp_f32, p.xyz_f32);
}

int sgm_pipeline_device(sgm_engine *e, const void *d_left, const void *d_right, int H, int W, int64_t stride_bytes,
                        const double Q[16], void *d_disp_i16, void *d_disp_f32, void *d_xyz_f32)
{
    if (!e) return set_err(SGM_ERR_INVALID_ARG, "engine is null");
    std::vector<void *> bound, rbound;
    if (int rc = take_bindings(e, 1, &bound, &rbound)) return rc;
    const PairIO io{d_left, d_right, d_disp_i16, d_disp_f32, d_xyz_f32, (uint8_t *)bound_at(bound, 0), (int16_t *)bound_at(rbound, 0)};
    return pipeline_one(e, io, H, W, stride_bytes, Q);
}

// ---- N pairs, throughput mode --------------------------------------------------------------------------------
// With the chained schedule (SGM_OPT_SCHEDULE 2 on `e`) and a configuration the fused sweeps cover, the pairs go through
// the frame in lockstep of its phases: cost stage of every pair (each on the stream of one of up to CHAIN_MAX_FRAMES
// internal engines), then ONE chained sweep launch per pass over all pairs of the group on `e`'s stream, then the
// winner-take-all and the epilogue of every pair.  One frame's chain of bands keeps only about 50 workgroups busy; a
// group of 6 or more fills the GPU, and no boundary pre-pass runs at all.

// an internal engine (a peer or a member of a chained group) plans as `e` does: every option that steers make_plan, and
// none of the per-call ones
static void inherit_options(sgm_engine *q, const sgm_engine *e)
{
    q->schedule = e->schedule;
    q->sweep_rows = e->sweep_rows;
    q->debug = e->debug;
    q->chain_wgs = e->chain_wgs;
    q->prepass_rows = e->prepass_rows;
    q->cn = e->cn;
    q->cost_fn = e->cost_fn;
    q->conf.on = e->conf.on;
    q->right.on = e->right.on;
    // e keeps S: its plan keeps the store of S, and the group runs ONE sweep kernel.  (Read before keep_aggr is cleared: the
    // host batch path calls this with q == e, and e's own plan follows its own keep_aggr.)
    q->no_wta_split = q != e && e->keep_aggr != 0;
    q->keep_aggr = 0;
    q->profile = 0;
}

// The engines of a chained group for up to `want` pairs: e itself + internal engines, created, configured like e and
// sized for the shape.  Fewer than `want` when device memory runs out (or would drop below a reserve of 4 GiB / 5 %:
// the caller and the runtime need room too) -- a batch then simply takes more groups.  *n_out >= 1.
static int prepare_group(sgm_engine *e, int want, int H, int W, const Plan &pl, int *n_out, size_t extra_per_pair = 0)
{
    int rc;
    *n_out = 0;
    if (e->group_max > 0) want = std::min(want, e->group_max);
    want = std::max(1, std::min(want, CHAIN_MAX_FRAMES));
    if ((rc = ensure_plan_buffers(e, pl, H, W))) return rc;
    *n_out = 1;
    if (want > 1 && !e->ev_group) HIP_TRY(hipEventCreateWithFlags(&e->ev_group, hipEventDisableTiming));
    bool retried = false;
    for (int k = 1; k < want; k++) {
        const bool is_new = (int)e->group.size() < k;
        if (is_new) {
            sgm_engine *q = nullptr;
            if ((rc = sgm_create(&e->params, e->device, nullptr, &q))) return rc;
            e->group.push_back(q);
        }
        sgm_engine *q = e->group[k - 1];
        inherit_options(q, e);
        if (!q->ev_done) HIP_TRY(hipEventCreateWithFlags(&q->ev_done, hipEventDisableTiming));
        // (nothing allocated -- the engine's buffers already hold this plan -- needs no reserve check; a shape it ran before
        //  may still need more: colour pairs (SGM_OPT_CHANNELS = 3) take larger feature buffers and the int16 hsum volume)
        const size_t held = plan_bytes_held(q);
        rc = ensure_plan_buffers(q, pl, H, W);
        const bool sized = plan_bytes_held(q) == held;
        size_t fr = 0, tot = 0;
        // (the reserve: 4 GiB or 5 % -- every stream, event pool and first launch of a kernel costs the runtime device memory
        //  too, and "out of memory" from a kernel launch cannot be recovered from -- plus what the caller of this function
        //  is about to allocate per pair: the host entry's transfer slots)
        if (!rc && !sized && hipMemGetInfo(&fr, &tot) == hipSuccess &&
            fr < std::max<size_t>((size_t)4 << 30, tot / 20) + extra_per_pair * (size_t)(k + 1))
            rc = SGM_ERR_NOMEM;
        if (rc == SGM_ERR_NOMEM) {
            release_buffers(q);   // (a half-sized engine would only hold memory the smaller group could use)
            q->H = q->W = 0;
            // engines behind this one may still hold the buffers of an earlier, larger batch or another shape: give those
            // back once and try this engine again before settling for a smaller group
            bool freed = false;
            for (size_t j = (size_t)k; j < e->group.size(); j++)
                if (e->group[j]->cost.p || e->group[j]->aggr.p) {
                    release_buffers(e->group[j]);
                    e->group[j]->H = e->group[j]->W = 0;
                    freed = true;
                }
            if (freed && !retried) {
                retried = true;
                k--;
                continue;
            }
            break;
        }
        if (rc) return rc;
        *n_out = k + 1;
    }
    return SGM_OK;
}

// every stream a batch call may have work on is drained before an error is returned, and the engines get their
// per-call flags back
struct BatchGuard {
    sgm_engine *e;
    bool ok = false;
    ~BatchGuard()
    {
        e->hr_accumulate = false;
        e->in_batch = false;
        for (sgm_engine *q : e->group) q->hr_accumulate = false;
        if (ok) return;
        (void)hipStreamSynchronize(e->stream);
        for (sgm_engine *q : e->group) (void)hipStreamSynchronize(q->stream);
        if (e->copy_in) (void)hipStreamSynchronize(e->copy_in);
        if (e->copy_out) (void)hipStreamSynchronize(e->copy_out);
    }
};

// One group (n >= 2 pairs on eng[0 .. n-1], eng[0] = e) through cost stages, joint sweeps, epilogues.  The host entry
// passes three event arrays (all null for resident pairs): in_ready[k] -- pair k's cost stage waits for it (its images have
// arrived); in_used[k] -- recorded when pair k's images have been read for the last time (k_features); out_done[k] -- recorded
// behind pair k's last kernel.  io[k]: the pointers of pair k.
static int run_group(sgm_engine *e, sgm_engine *const *eng, int n, const Plan &pl, const PairIO *io, int H, int W, int64_t stride_bytes,
                     const double Q[16], const hipEvent_t *in_ready, const hipEvent_t *in_used, const hipEvent_t *out_done)
{
    int rc;
    // cost stage of every pair on the stream of its own engine, from where `e`'s stream stands now (the caller's
    // inputs may have been produced on it).  Side by side rather than one after the other: the per-pixel cost
    // kernel is bound by the vector units, the box filter by HBM -- pairs in different kernels overlap (12 pairs
    // 4K D=256: 7.2 against 7.4 ms per pair with the cost stages in one stream).
    HIP_TRY(hipEventRecord(e->ev_group, e->stream));
    for (int k = 1; k < n; k++) HIP_TRY(hipStreamWaitEvent(eng[k]->stream, e->ev_group, 0));
    for (int k = 0; k < n; k++) {
        if (in_ready && in_ready[k]) HIP_TRY(hipStreamWaitEvent(eng[k]->stream, in_ready[k], 0));
        if ((rc = run_compute(eng[k], io[k], H, W, stride_bytes, PH_PRE))) return rc;
        const Plan &q = eng[k]->plan;
        if (!q.chain || q.R != pl.R || q.nbands != pl.nbands || q.axis != pl.axis || q.wta_split != pl.wta_split)
            return set_err(SGM_ERR_HIP, "internal: a pair of a chained group did not plan the group's chained sweep");
        if (in_used && in_used[k]) HIP_TRY(hipEventRecord(in_used[k], eng[k]->stream));   // (behind the whole cost stage: the images are read by its first kernel only)
    }
    // ---- the sweeps of all n pairs: one launch per pass on e's stream, behind every pair's cost stage
    const Geom &g = e->g;
    const int R = pl.R, nbands = pl.nbands, npass = pl.npass;
    const size_t ctl_bytes = chain_ctl_bytes(n, nbands);
    if ((rc = e->chain_ctl.ensure(ctl_bytes))) return rc;
    for (int k = 1; k < n; k++) {
        HIP_TRY(hipEventRecord(eng[k]->ev_done, eng[k]->stream));
        HIP_TRY(hipStreamWaitEvent(e->stream, eng[k]->ev_done, 0));
    }
    stage_break(e);
    ChainFrames fr;
    fr.nf = n;
    for (int k = 0; k < n; k++) {
        fr.C[k] = (const int16_t *)eng[k]->cost.p;
        fr.S[k] = (int16_t *)eng[k]->aggr.p;
        fr.bnd[k] = (int16_t *)eng[k]->bndL.p;
        fr.hr[k] = eng[k]->g.hr;
        fr.raw[k] = (uint4 *)eng[k]->wta_raw.p;
    }
    for (int pass = 0; pass < npass; pass++) {
        const int ydir = pass == 0 ? 1 : -1;
        SweepArgs a{ydir, ydir, R, nullptr, nullptr, nullptr, nullptr, 0, e->debug, (uint32_t *)e->chain_ctl.p, nullptr,
                    (uint32_t *)e->chain_err.p, nbands};
        HIP_TRY(hipMemsetAsync(e->chain_ctl.p, 0, ctl_bytes, e->stream));
        stage_break(e);
        const int cm = pass == 0 ? SWEEP_FIRST : (pl.wta_split ? SWEEP_REDUCE : SWEEP_ACCUM);
        rc = run_stage(e, pass == 0 ? "chain_dn" : "chain_up", [&] {
            const int err = launch_chain(g, a, fr, cm, chain_window(g, R, nbands, n, e->chain_wgs), e->stream, pl.axis);
            return err ? err : 1;
        });
        if (rc) return rc;
    }
    HIP_TRY(hipEventRecord(e->ev_group, e->stream));
    // ---- the rest of every pair on its own stream (memory-bound kernels of different pairs side by side)
    for (int k = 0; k < n; k++) {
        if (k > 0) HIP_TRY(hipStreamWaitEvent(eng[k]->stream, e->ev_group, 0));
        // Host entry: the epilogues three at a time, not all at once -- they are bound by HBM either way, and pair k's map
        // can travel to the host while the epilogues of the pairs behind it still run (all n at once end together: the
        // whole group's download would follow the last kernel).
        if (out_done && k >= 3 && out_done[k - 3]) HIP_TRY(hipStreamWaitEvent(eng[k]->stream, out_done[k - 3], 0));
        if ((rc = run_compute(eng[k], io[k], H, W, stride_bytes, PH_POST))) return rc;
        if ((rc = run_float_xyz(eng[k], (const int16_t *)io[k].disp_i16, H, W, Q, io[k].disp_f32, io[k].xyz_f32))) return rc;
        if (out_done && out_done[k]) HIP_TRY(hipEventRecord(out_done[k], eng[k]->stream));
    }
    // e's stream ends behind everything the group did
    for (int k = 1; k < n; k++) {
        HIP_TRY(hipEventRecord(eng[k]->ev_done, eng[k]->stream));
        HIP_TRY(hipStreamWaitEvent(e->stream, eng[k]->ev_done, 0));
    }
    stage_break(e);
    return SGM_OK;
}

// can this call run chained, and with which plan ?  (decided from the geometry alone: nothing is created or enqueued)
static int batch_plan(sgm_engine *e, int N, int H, int W, Plan *pl, bool *joint)
{
    if (H <= 0 || W < 2) return set_err(SGM_ERR_INVALID_ARG, "bad shape H=%d W=%d", H, W);
    if (W > 32767 || H > 32767) return set_err(SGM_ERR_UNSUPPORTED, "image larger than 32767 in a dimension");
    if (census_refused(e)) return SGM_ERR_UNSUPPORTED;
    Geom g;
    int rc = normalise(&e->params, H, W, &g);
    if (rc) return rc;
    *pl = make_plan(e, g, H);
    *joint = e->schedule == 2 && N > 1 && pl->chain && e->group_max != 1;
    return SGM_OK;
}

// N pairs in groups of at most `cap`: groups of equal size, and the engines that run a group's pairs (e + its internal ones)
static std::vector<sgm_engine *> group_engines(sgm_engine *e, int N, int cap, int *ngroups)
{
    *ngroups = (N + cap - 1) / cap;
    std::vector<sgm_engine *> eng((N + *ngroups - 1) / *ngroups);
    for (size_t k = 0; k < eng.size(); k++) eng[k] = k == 0 ? e : e->group[k - 1];
    return eng;
}

// N pairs resident in device memory.  Chained groups when the configuration allows (groups as large as device memory
// holds, up to CHAIN_MAX_FRAMES or SGM_OPT_GROUP_MAX; a batch larger than a group is cut into groups of equal size);
// otherwise pair after pair on `e` (the schedule `e` is set to).  Results equal N calls of sgm_pipeline_device.
// Asynchronous like sgm_pipeline_device: returns when everything is enqueued; sgm_synchronize(e) waits for all of it.
// On an error every stream of the group is drained before the call returns.
int sgm_pipeline_batch_device(sgm_engine *e, int N, const void *const *d_left, const void *const *d_right, int H, int W,
                              int64_t stride_bytes, const double Q[16], void *const *d_disp_i16, void *const *d_disp_f32,
                              void *const *d_xyz_f32)
{
    if (!e) return set_err(SGM_ERR_INVALID_ARG, "bad argument");
    std::vector<void *> bound, rbound;
    const int brc = take_bindings(e, N, &bound, &rbound);   // (consumed before anything else can fail)
    if (N <= 0 || !d_left || !d_right || !d_disp_i16) return set_err(SGM_ERR_INVALID_ARG, "bad argument");
    if (brc) return brc;
    for (int i = 0; i < N; i++)
        if (!d_left[i] || !d_right[i] || !d_disp_i16[i]) return set_err(SGM_ERR_INVALID_ARG, "null pointer for pair %d", i);
    if (stride_bytes < (int64_t)W * e->cn)
        return set_err(SGM_ERR_INVALID_ARG, "bad shape H=%d W=%d stride=%lld (channels %d)", H, W, (long long)stride_bytes, e->cn);
    if (d_xyz_f32 && !Q) return set_err(SGM_ERR_INVALID_ARG, "Q is null");
    std::vector<PairIO> io(N);
    for (int i = 0; i < N; i++)
        io[i] = PairIO{d_left[i], d_right[i], d_disp_i16[i], d_disp_f32 ? d_disp_f32[i] : nullptr, d_xyz_f32 ? d_xyz_f32[i] : nullptr,
                       (uint8_t *)bound_at(bound, i), (int16_t *)bound_at(rbound, i)};
    HIP_TRY(hipSetDevice(e->device));
    int rc;
    Plan pl;
    bool joint = false;
    if ((rc = batch_plan(e, N, H, W, &pl, &joint))) return rc;
    BatchGuard guard{e};
    e->in_batch = true;
    e->last_peers = 0;
    e->last_group = 0;
    int cap = 1;
    if (joint && (rc = prepare_group(e, N, H, W, pl, &cap))) return rc;
    if (!joint || cap < 2) {
        for (int i = 0; i < N; i++) {
            e->hr_accumulate = i > 0;     // (the headroom record of the call covers every pair)
            if ((rc = pipeline_one(e, io[i], H, W, stride_bytes, Q))) return rc;
        }
        guard.ok = true;
        return SGM_OK;
    }
    int ngroups;
    const std::vector<sgm_engine *> eng = group_engines(e, N, cap, &ngroups);
    const int per = (int)eng.size();
    e->last_group = std::min(per, N) - 1;
    for (int i0 = 0; i0 < N; i0 += per) {
        const int n = std::min(N - i0, per);
        for (int k = 0; k < n; k++) eng[k]->hr_accumulate = i0 > 0;
        if (n == 1) {
            if ((rc = pipeline_one(e, io[i0], H, W, stride_bytes, Q))) return rc;
            continue;
        }
        if ((rc = run_group(e, eng.data(), n, pl, io.data() + i0, H, W, stride_bytes, Q, nullptr, nullptr, nullptr))) return rc;
    }
    guard.ok = true;
    return SGM_OK;
}

int sgm_compute(sgm_engine *e, const uint8_t *left, const uint8_t *right, int H, int W, int64_t stride_bytes,
                int16_t *disp_out)
{
    if (!e || !left || !right || !disp_out) return set_err(SGM_ERR_INVALID_ARG, "null pointer");
    clear_bindings(e);
    const int64_t rowb = (int64_t)W * e->cn;  // bytes of one image row (SGM_OPT_CHANNELS)
    if (H <= 0 || W < 2 || stride_bytes < rowb)
        return set_err(SGM_ERR_INVALID_ARG, "bad shape H=%d W=%d stride=%lld (channels %d)", H, W, (long long)stride_bytes, e->cn);
    if (census_refused(e)) return SGM_ERR_UNSUPPORTED;
    HIP_TRY(hipSetDevice(e->device));
    const size_t npx = (size_t)H * W, ib = (size_t)H * rowb;
    int rc;
    if ((rc = e->in_left.ensure(ib)) || (rc = e->in_right.ensure(ib)) || (rc = e->disp_out.ensure(npx * 2))) return rc;
    HIP_TRY(hipMemcpy2DAsync(e->in_left.p, rowb, left, (size_t)stride_bytes, rowb, H, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpy2DAsync(e->in_right.p, rowb, right, (size_t)stride_bytes, rowb, H, hipMemcpyHostToDevice, e->stream));
    const PairIO io{e->in_left.p, e->in_right.p, e->disp_out.p, nullptr, nullptr, nullptr, nullptr};
    if ((rc = run_compute(e, io, H, W, rowb))) return rc;
    HIP_TRY(hipMemcpyAsync(disp_out, e->disp_out.p, npx * 2, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return check_chain(e);
}

// memcpy between pageable and page-locked host memory with a few threads (large blocks only: one thread moves about
// 10 GB/s, a 4K frame is 8 - 17 MB)
static void host_copy(void *dst, const void *src, size_t bytes)
{
    const int nt = bytes >= ((size_t)4 << 20) ? 4 : 1;
    if (nt == 1) {
        std::memcpy(dst, src, bytes);
        return;
    }
    const size_t part = (bytes / nt + 4095) & ~(size_t)4095;
    std::thread th[3];
    for (int t = 1; t < nt; t++) {
        const size_t o = std::min(bytes, part * t), n = std::min(bytes - o, part);
        th[t - 1] = std::thread([=] { std::memcpy((char *)dst + o, (const char *)src + o, n); });
    }
    std::memcpy(dst, src, std::min(bytes, part));
    for (int t = 1; t < nt; t++) th[t - 1].join();
}

// N independent pairs from / to host memory.  Up to three pairs are in flight: pair i runs on engine
// i % 3 (the engine itself and two peers with their own streams and device buffers, created on first
// use).  Images and disparity maps are staged through page-locked buffers of the engine they run on, so
// every transfer is asynchronous: while the host copies the results of pair i - 3 out of, and pair i
// into, the staging buffers of one engine, the other two keep the GPU busy with two frames (a second
// frame fills the issue slots and the HBM time one frame leaves idle).  The XYZ image
// (99.5 MB per 4K pair) goes straight to the caller's buffer: staging it would cost the host more than
// the pageable copy does.
int sgm_compute_batch(sgm_engine *e, int N, const uint8_t *lefts, const uint8_t *rights, int H, int W,
                      int16_t *disps_out, float *xyz_out, const double *Q16)
{
    if (!e || !lefts || !rights || !disps_out || N <= 0) return set_err(SGM_ERR_INVALID_ARG, "bad argument");
    clear_bindings(e);   // (no per-pair confidence or right-view map from this entry: sgm_hip.h)
    if (xyz_out && !Q16) return set_err(SGM_ERR_INVALID_ARG, "xyz_out requested without Q");
    if (H <= 0 || W < 2) return set_err(SGM_ERR_INVALID_ARG, "bad shape");
    HIP_TRY(hipSetDevice(e->device));
    const size_t npx = (size_t)H * W, ib = npx * e->cn;  // pixels, bytes of one image ([H][W][cn], tight rows)
    const int64_t rowb = (int64_t)W * e->cn;
    int rc;
    Plan pl;
    bool joint = false;
    if ((rc = batch_plan(e, N, H, W, &pl, &joint))) return rc;
    if (joint) {
        // Throughput mode: chained groups as large as device memory holds, TWO groups in flight -- while the kernels of
        // group g run, the images of group g + 1 are uploaded and the maps of group g - 1 downloaded on two copy streams
        // of their own.  Every pair has its device images twice (slot g & 1) on the engine that runs it, with page-locked
        // staging beside them (copies from / to pageable memory would block the host until the GPU gets round to them --
        // and a chained sweep launch holds every CU for its whole length), and four events:
        //   in:   images uploaded   -- the pair's cost stage waits for this one only: the first kernels start when the first
        //                              pair has arrived, not the whole group
        //   used: images consumed   -- the upload of group g + 2 into the same slot waits for it
        //   out:  last kernel done  -- the pair's download waits for this one only (the epilogues of a group run three at a
        //                              time, so maps leave while the pairs behind them are still being finished)
        //   dl:   map in the staging buffer -- the host copies it to the caller's array; passed before the slot is reused
        // The host copies caller -> staging -> caller with a few threads (one thread moves about 10 GB/s; 17 4K maps are 282 MB).
        // The XYZ images (99.5 MB each) go straight to the caller's memory: staging them would pin gigabytes.
        BatchGuard guard{e};
        e->in_batch = true;
        e->last_peers = 0;   // (set again below if the call ends up spreading its pairs over the peers)
        int cap = 1;
        const size_t slot_bytes = 2 * (2 * ib + npx * 2 + (xyz_out ? npx * 16 : 0));
        if ((rc = prepare_group(e, N, H, W, pl, &cap, slot_bytes))) return rc;
        if (cap >= 2) {
            if (!e->copy_in) HIP_TRY(hipStreamCreateWithFlags(&e->copy_in, hipStreamNonBlocking));
            if (!e->copy_out) HIP_TRY(hipStreamCreateWithFlags(&e->copy_out, hipStreamNonBlocking));
            int ngroups;
            const std::vector<sgm_engine *> eng = group_engines(e, N, cap, &ngroups);
            const int per = (int)eng.size();
            e->last_group = per - 1;
            for (sgm_engine *q : eng) {
                for (int sl = 0; sl < (ngroups > 1 ? 2 : 1); sl++) {
                    if ((rc = q->io[sl][0].ensure(ib)) || (rc = q->io[sl][1].ensure(ib)) || (rc = q->io[sl][2].ensure(npx * 2))) return rc;
                    if ((rc = q->pin_io[sl][0].ensure(ib)) || (rc = q->pin_io[sl][1].ensure(ib)) || (rc = q->pin_io[sl][2].ensure(npx * 2))) return rc;
                    if (xyz_out && ((rc = q->io[sl][3].ensure(npx * 4)) || (rc = q->io[sl][4].ensure(npx * 12)))) return rc;
                    for (hipEvent_t *ev : {&q->ev_io_in[sl], &q->ev_io_used[sl], &q->ev_io_out[sl], &q->ev_io_dl[sl]})
                        if (!*ev) HIP_TRY(hipEventCreateWithFlags(ev, hipEventDisableTiming));
                }
            }
            std::vector<PairIO> io(per);
            std::vector<hipEvent_t> evi(per), evu(per), evo(per);
            auto upload = [&](int gi) -> int {     // images of group gi -> slot gi & 1, pair by pair
                const int sl = gi & 1, i0 = gi * per, n = std::min(N - i0, per);
                for (int k = 0; k < n; k++) {
                    sgm_engine *q = eng[k];
                    const size_t i = (size_t)(i0 + k);
                    if (gi >= 2) {
                        HIP_TRY(hipEventSynchronize(q->ev_io_in[sl]));                 // the staging buffers: their last upload has left them (long ago)
                        HIP_TRY(hipStreamWaitEvent(e->copy_in, q->ev_io_used[sl], 0));  // the device images: group gi - 2 has read them
                    }
                    host_copy(q->pin_io[sl][0].p, lefts + i * ib, ib);
                    host_copy(q->pin_io[sl][1].p, rights + i * ib, ib);
                    HIP_TRY(hipMemcpyAsync(q->io[sl][0].p, q->pin_io[sl][0].p, ib, hipMemcpyHostToDevice, e->copy_in));
                    HIP_TRY(hipMemcpyAsync(q->io[sl][1].p, q->pin_io[sl][1].p, ib, hipMemcpyHostToDevice, e->copy_in));
                    HIP_TRY(hipEventRecord(q->ev_io_in[sl], e->copy_in));
                }
                return SGM_OK;
            };
            auto compute = [&](int gi) -> int {    // kernels of group gi, and -- behind each pair's last one -- its download
                const int sl = gi & 1, i0 = gi * per, n = std::min(N - i0, per);
                for (int k = 0; k < n; k++) {
                    sgm_engine *q = eng[k];
                    q->hr_accumulate = gi > 0;
                    io[k] = PairIO{q->io[sl][0].p, q->io[sl][1].p, q->io[sl][2].p, xyz_out ? q->io[sl][3].p : nullptr,
                                   xyz_out ? q->io[sl][4].p : nullptr, nullptr, nullptr};
                    evi[k] = q->ev_io_in[sl];
                    evu[k] = q->ev_io_used[sl];
                    evo[k] = q->ev_io_out[sl];
                }
                if (n == 1) {   // (a last group of one pair: the plain entry on e, behind its upload)
                    HIP_TRY(hipStreamWaitEvent(e->stream, evi[0], 0));
                    int r2 = pipeline_one(e, io[0], H, W, rowb, Q16);
                    if (r2) return r2;
                    HIP_TRY(hipEventRecord(evu[0], e->stream));
                    HIP_TRY(hipEventRecord(evo[0], e->stream));
                } else {
                    int r2 = run_group(e, eng.data(), n, pl, io.data(), H, W, rowb, Q16, evi.data(), evu.data(), evo.data());
                    if (r2) return r2;
                }
                for (int k = 0; k < n; k++) {
                    sgm_engine *q = eng[k];
                    HIP_TRY(hipStreamWaitEvent(e->copy_out, q->ev_io_out[sl], 0));
                    HIP_TRY(hipMemcpyAsync(q->pin_io[sl][2].p, q->io[sl][2].p, npx * 2, hipMemcpyDeviceToHost, e->copy_out));
                    HIP_TRY(hipEventRecord(q->ev_io_dl[sl], e->copy_out));
                }
                return SGM_OK;
            };
            auto finish = [&](int gi) -> int {     // maps (and XYZ) of group gi into the caller's arrays
                const int sl = gi & 1, i0 = gi * per, n = std::min(N - i0, per);
                for (int k = 0; k < n; k++) {
                    sgm_engine *q = eng[k];
                    const size_t i = (size_t)(i0 + k);
                    HIP_TRY(hipEventSynchronize(q->ev_io_dl[sl]));
                    host_copy(disps_out + i * npx, q->pin_io[sl][2].p, npx * 2);
                    if (xyz_out) HIP_TRY(hipMemcpy(xyz_out + i * npx * 3, q->io[sl][4].p, npx * 12, hipMemcpyDeviceToHost));
                }
                return SGM_OK;
            };
            if ((rc = upload(0))) return rc;
            for (int gi = 0; gi < ngroups; gi++) {
                if ((rc = compute(gi))) return rc;
                if (gi + 1 < ngroups && (rc = upload(gi + 1))) return rc;     // beside the kernels of group gi
                if (gi > 0 && (rc = finish(gi - 1))) return rc;                // (its slot's maps are rewritten by group gi + 1, enqueued after this)
            }
            if ((rc = finish(ngroups - 1))) return rc;
            HIP_TRY(hipStreamSynchronize(e->stream));
            guard.ok = true;
            return check_chain(e);
        }
        // (not even two pairs fit beside each other: pair after pair below)
    }
    const int neng = std::min(N, 3);
    if (neng > 1 && !e->peer && (rc = sgm_create(&e->params, e->device, nullptr, &e->peer))) return rc;
    if (neng > 2 && !e->peer2 && (rc = sgm_create(&e->params, e->device, nullptr, &e->peer2))) return rc;
    sgm_engine *eng[3] = {e, e->peer, e->peer2};
    const int saved_keep = e->keep_aggr, saved_profile = e->profile;
    // every exit drains the streams of all engines (copies into / out of the page-locked staging buffers and kernels may
    // still be in flight when an error is returned) and gives the caller's engine its own options back
    struct Drain {
        sgm_engine **eng;
        int n, keep, prof;
        ~Drain()
        {
            for (int k = 0; k < n; k++)
                if (eng[k]) {
                    (void)hipStreamSynchronize(eng[k]->stream);
                    eng[k]->hr_accumulate = false;
                }
            eng[0]->keep_aggr = keep;
            eng[0]->profile = prof;
        }
    } drain{eng, neng, saved_keep, saved_profile};
    for (int k = 0; k < neng; k++) {
        sgm_engine *q = eng[k];
        inherit_options(q, e);
        if ((rc = q->in_left.ensure(ib)) || (rc = q->in_right.ensure(ib)) || (rc = q->disp_out.ensure(npx * 2))) return rc;
        if ((rc = q->pin_left.ensure(ib)) || (rc = q->pin_right.ensure(ib)) || (rc = q->pin_disp.ensure(npx * 2))) return rc;
        if (xyz_out && ((rc = q->f32.ensure(npx * 4)) || (rc = q->xyz.ensure(npx * 12)))) return rc;
        if (!q->ev_done) HIP_TRY(hipEventCreateWithFlags(&q->ev_done, hipEventDisableTiming));
    }
    // results of pair i leave its engine right before the engine is reused for pair i + neng
    auto finish = [&](int i) -> int {
        sgm_engine *q = eng[i % neng];
        HIP_TRY(hipEventSynchronize(q->ev_done));
        std::memcpy(disps_out + (size_t)i * npx, q->pin_disp.p, npx * 2);
        if (xyz_out) HIP_TRY(hipMemcpy(xyz_out + (size_t)i * npx * 3, q->xyz.p, npx * 12, hipMemcpyDeviceToHost));
        return SGM_OK;
    };
    for (int i = 0; i < N; i++) {
        sgm_engine *q = eng[i % neng];
        if (i >= neng && (rc = finish(i - neng))) return rc;
        std::memcpy(q->pin_left.p, lefts + (size_t)i * ib, ib);
        std::memcpy(q->pin_right.p, rights + (size_t)i * ib, ib);
        HIP_TRY(hipMemcpyAsync(q->in_left.p, q->pin_left.p, ib, hipMemcpyHostToDevice, q->stream));
        HIP_TRY(hipMemcpyAsync(q->in_right.p, q->pin_right.p, ib, hipMemcpyHostToDevice, q->stream));
        q->hr_accumulate = i >= neng;   // (the headroom record of the call covers every pair: each engine keeps its pairs' maximum)
        const PairIO io{q->in_left.p, q->in_right.p, q->disp_out.p, xyz_out ? q->f32.p : nullptr, xyz_out ? q->xyz.p : nullptr,
                        nullptr, nullptr};
        if ((rc = pipeline_one(q, io, H, W, rowb, Q16))) return rc;
        HIP_TRY(hipMemcpyAsync(q->pin_disp.p, q->disp_out.p, npx * 2, hipMemcpyDeviceToHost, q->stream));
        HIP_TRY(hipEventRecord(q->ev_done, q->stream));
    }
    for (int i = std::max(0, N - neng); i < N; i++)
        if ((rc = finish(i))) return rc;
    e->last_peers = neng - 1;   // (sgm_get_headroom: the pairs of this call ran on the peers as well)
    return SGM_OK;
}

int sgm_disp_to_float(sgm_engine *e, const int16_t *disp, int64_t n, float *out)
{
    if (!e || !disp || !out || n <= 0) return set_err(SGM_ERR_INVALID_ARG, "bad argument");
    HIP_TRY(hipSetDevice(e->device));
    int rc;
    if ((rc = e->disp_out.ensure((size_t)n * 2)) || (rc = e->f32.ensure((size_t)n * 4))) return rc;
    HIP_TRY(hipMemcpyAsync(e->disp_out.p, disp, (size_t)n * 2, hipMemcpyHostToDevice, e->stream));
    if ((rc = run_to_float(e, (const int16_t *)e->disp_out.p, n, (float *)e->f32.p))) return rc;
    HIP_TRY(hipMemcpyAsync(out, e->f32.p, (size_t)n * 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return SGM_OK;
}

int sgm_reproject(sgm_engine *e, const float *disp, int H, int W, const double Q[16], int handle_missing, float *xyz_out)
{
    if (!e || !disp || !xyz_out || !Q || H <= 0 || W <= 0) return set_err(SGM_ERR_INVALID_ARG, "bad argument");
    HIP_TRY(hipSetDevice(e->device));
    const size_t npx = (size_t)H * W;
    int rc;
    if ((rc = e->f32.ensure(npx * 4)) || (rc = e->xyz.ensure(npx * 12))) return rc;
    HIP_TRY(hipMemcpyAsync(e->f32.p, disp, npx * 4, hipMemcpyHostToDevice, e->stream));
    if ((rc = run_reproject(e, (const float *)e->f32.p, H, W, Q, handle_missing, (float *)e->xyz.p))) return rc;
    HIP_TRY(hipMemcpyAsync(xyz_out, e->xyz.p, npx * 12, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return SGM_OK;
}

int sgm_valid_mask(sgm_engine *e, const float *xyz, const float *disp, int64_t n, uint8_t *mask)
{
    if (!e || !xyz || !disp || !mask || n <= 0) return set_err(SGM_ERR_INVALID_ARG, "bad argument");
    HIP_TRY(hipSetDevice(e->device));
    int rc;
    if ((rc = e->f32.ensure((size_t)n * 4)) || (rc = e->xyz.ensure((size_t)n * 12)) || (rc = e->mask.ensure((size_t)n))) return rc;
    HIP_TRY(hipMemcpyAsync(e->f32.p, disp, (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->xyz.p, xyz, (size_t)n * 12, hipMemcpyHostToDevice, e->stream));
    if ((rc = sgm_valid_mask_device(e, e->xyz.p, e->f32.p, n, e->mask.p))) return rc;
    HIP_TRY(hipMemcpyAsync(mask, e->mask.p, (size_t)n, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return SGM_OK;
}

// the three launches of an ordered compaction on the engine's stream; the total stays in e->ccount[m]
static int enqueue_compaction(sgm_engine *e, const void *d_xyz, const void *d_disp_f32, const void *d_colors_rgb, int64_t n,
                              void *d_out_points, void *d_out_colors, int *m_out)
{
    if (!e || !d_xyz || !d_disp_f32 || !d_out_points || n <= 0) return set_err(SGM_ERR_INVALID_ARG, "bad argument");
    if (d_out_colors && !d_colors_rgb) return set_err(SGM_ERR_INVALID_ARG, "out_colors requested without colors");
    if (n >= (1ll << 32)) return set_err(SGM_ERR_UNSUPPORTED, "more than 2^32 points");
    HIP_TRY(hipSetDevice(e->device));
    const int m = (int)((n + 255) / 256);
    int rc;
    if ((rc = e->ccount.ensure((size_t)(m + 1) * 4))) return rc;
    uint32_t *cnt = (uint32_t *)e->ccount.p;
    hipStream_t st = e->stream;
    hipLaunchKernelGGL(k_compact_count, dim3(m), dim3(256), 0, st, (const float *)d_xyz, (const float *)d_disp_f32, n, cnt);
    hipLaunchKernelGGL(k_compact_scan, dim3(1), dim3(1024), 0, st, cnt, m);
    hipLaunchKernelGGL(k_compact_scatter, dim3(m), dim3(256), 0, st, (const float *)d_xyz, (const float *)d_disp_f32,
                       (const uint8_t *)(d_out_colors ? d_colors_rgb : nullptr), n, (const uint32_t *)cnt,
                       (float *)d_out_points, (uint8_t *)d_out_colors);
    KCHECK();
    *m_out = m;
    return SGM_OK;
}

int sgm_compact_points_device(sgm_engine *e, const void *d_xyz, const void *d_disp_f32, const void *d_colors_rgb,
                              int64_t n, void *d_out_points, void *d_out_colors, int64_t *n_valid)
{
    if (!n_valid) return set_err(SGM_ERR_INVALID_ARG, "bad argument");
    int m = 0;
    int rc = enqueue_compaction(e, d_xyz, d_disp_f32, d_colors_rgb, n, d_out_points, d_out_colors, &m);
    if (rc) return rc;
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, (uint32_t *)e->ccount.p + m, 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    *n_valid = (int64_t)total;
    return SGM_OK;
}

// the same without a host round trip: the count goes to device memory (stream order), nothing is synchronised
int sgm_compact_points_device_async(sgm_engine *e, const void *d_xyz, const void *d_disp_f32, const void *d_colors_rgb,
                                    int64_t n, void *d_out_points, void *d_out_colors, void *d_n_valid_i64)
{
    if (!d_n_valid_i64) return set_err(SGM_ERR_INVALID_ARG, "bad argument");
    int m = 0;
    int rc = enqueue_compaction(e, d_xyz, d_disp_f32, d_colors_rgb, n, d_out_points, d_out_colors, &m);
    if (rc) return rc;
    hipLaunchKernelGGL(k_compact_total, dim3(1), dim3(1), 0, e->stream, (const uint32_t *)e->ccount.p + m, (int64_t *)d_n_valid_i64);
    KCHECK();
    return SGM_OK;
}

// One input of an add-on's host entry: `bytes` from `host` go up to the engine's `dev`.  A null host or no bytes: not staged.
struct HostIn {
    const void *host;
    DevBuf *dev;
    size_t bytes;
    void *d() const { return host && bytes ? dev->p : nullptr; }   // what the device entry gets (after the buffers have been made)
};
// One output: `host` (null: not asked for) gets rows of `row` bytes from the engine's `dev`, which is made to hold cap of them
// (cap < 0: the call's n) -- as many as *rows says once the device entry has run, or all of them with rows null
struct HostOut {
    void *host;
    DevBuf *dev;
    size_t row;
    const int64_t *rows;
    int64_t cap = -1;
    void *d() const { return host ? dev->p : nullptr; }
};

// What the host entries of the add-ons share: every buffer made, the inputs up, run() -- the device entry on in.d() and out.d() --,
// then the outputs down and one synchronise.  n: the rows an output holds unless it says otherwise.
extern "C++" {   // (templates: this part of the file has C linkage)
template <class Run>
static int host_call(sgm_engine *e, int64_t n, std::initializer_list<HostIn> ins, std::initializer_list<HostOut> outs, Run run)
{
    HIP_TRY(hipSetDevice(e->device));
    int rc;
    for (const HostIn &i : ins)
        if (i.host && i.bytes && (rc = i.dev->ensure(i.bytes))) return rc;
    for (const HostOut &o : outs)
        if (o.host && (rc = o.dev->ensure((size_t)(o.cap < 0 ? n : o.cap) * o.row))) return rc;
    for (const HostIn &i : ins)
        if (i.host && i.bytes) HIP_TRY(hipMemcpyAsync(i.dev->p, i.host, i.bytes, hipMemcpyHostToDevice, e->stream));
    if ((rc = run())) {
        (void)hipStreamSynchronize(e->stream);   // (the caller's memory is the source of nothing when the call returns)
        return rc;
    }
    for (const HostOut &o : outs) {
        const int64_t rows = o.rows ? *o.rows : (o.cap < 0 ? n : o.cap);
        if (o.host && rows > 0) HIP_TRY(hipMemcpyAsync(o.host, o.dev->p, (size_t)rows * o.row, hipMemcpyDeviceToHost, e->stream));
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    return SGM_OK;
}
// the point-list form: the cloud up (xyz to e->xyz; disp, colors: to e->f32, e->crgb_in, or null), run(d_disp, d_colors)
template <class Run>
static int cloud_host_call(sgm_engine *e, const float *xyz, const float *disp, const uint8_t *colors, int64_t n,
                           std::initializer_list<HostOut> outs, Run run)
{
    const HostIn pts{xyz, &e->xyz, (size_t)n * 12}, dsp{disp, &e->f32, (size_t)n * 4}, rgb{colors, &e->crgb_in, (size_t)n * 3};
    return host_call(e, n, {pts, dsp, rgb}, outs, [&] { return run(dsp.d(), rgb.d()); });
}
}  // extern "C++"

// the statistics of a call into the caller's table (null: not asked for)
static void put_stats(uint64_t *out, std::initializer_list<uint64_t> s)
{
    if (out) std::copy(s.begin(), s.end(), out);
}

int sgm_compact_points(sgm_engine *e, const float *xyz, const float *disp, const uint8_t *colors_rgb, int64_t n,
                       float *out_points, uint8_t *out_colors, int64_t *n_valid)
{
    if (!e || !xyz || !disp || !out_points || !n_valid || n <= 0) return set_err(SGM_ERR_INVALID_ARG, "bad argument");
    if (out_colors && !colors_rgb) return set_err(SGM_ERR_INVALID_ARG, "out_colors requested without colors");
    const HostOut pts{out_points, &e->cpts, 12, n_valid}, rgb{out_colors, &e->crgb, 3, n_valid};
    return cloud_host_call(e, xyz, disp, out_colors ? colors_rgb : nullptr, n, {pts, rgb}, [&](void *d_disp, void *d_colors) {
        return sgm_compact_points_device(e, e->xyz.p, d_disp, d_colors, n, pts.d(), rgb.d(), n_valid);
    });
}

int sgm_median3x3(sgm_engine *e, const int16_t *src, int H, int W, int16_t *dst)
{
    if (!e || !src || !dst || H <= 0 || W <= 0) return set_err(SGM_ERR_INVALID_ARG, "bad argument");
    HIP_TRY(hipSetDevice(e->device));
    const size_t npx = (size_t)H * W;
    int rc;
    if ((rc = e->disp_raw.ensure(npx * 2)) || (rc = e->disp_med.ensure(npx * 2))) return rc;
    HIP_TRY(hipMemcpyAsync(e->disp_raw.p, src, npx * 2, hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(k_median3, dim3((W + 255) / 256, H), dim3(256), 0, e->stream, (const int16_t *)e->disp_raw.p,
                       (int16_t *)e->disp_med.p, (int16_t *)nullptr, H, W);
    KCHECK();
    HIP_TRY(hipMemcpyAsync(dst, e->disp_med.p, npx * 2, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return SGM_OK;
}

// ---- what the batched add-on entries share (the edge-aware filter and the left-right confidence) ------------------------------
// Maps (the confidence: pairs) per chunk, and the buffers of the call sized for it.  C = min(N, BATCH_MAPS_MAX, SGM_OPT_GROUP_MAX
// if set), cut to what free device memory allows beside the reserve of prepare_group (4 GiB or 5 %) when a buffer has to grow;
// at least 1.  All allocations of the call happen here, before anything is enqueued.
struct BatchNeed { DevBuf *b; size_t per_map; };
static int batch_reserve(sgm_engine *e, int N, std::initializer_list<BatchNeed> needs, int *C_out)
{
    int C = std::min(N, BATCH_MAPS_MAX);
    if (e->group_max > 0) C = std::min(C, e->group_max);
    size_t per_map = 0, freed = 0;   // of the buffers that grow: bytes per map, and what they give back first (DevBuf::ensure)
    for (const BatchNeed &n : needs)
        if (n.b->cap < n.per_map * (size_t)C) {
            per_map += n.per_map;
            freed += n.b->cap;
        }
    size_t fr = 0, tot = 0;
    if (per_map && hipMemGetInfo(&fr, &tot) == hipSuccess) {
        const size_t reserve = std::max<size_t>((size_t)4 << 30, tot / 20), have = fr + freed;
        const size_t room = have > reserve ? have - reserve : 0;
        C = (int)std::max<size_t>(1, std::min<size_t>((size_t)C, room / per_map));
    }
    for (const BatchNeed &n : needs)
        if (int rc = n.b->ensure(n.per_map * (size_t)C)) return rc;
    *C_out = C;
    return SGM_OK;
}

// the by-value table of a chunk's n device pointers from the caller's array (null: the chunk has no such map, every entry null)
static MapPtrs map_ptrs(const void *const *a, int n)
{
    MapPtrs t{};
    for (int i = 0; a && i < n; i++) t.p[i] = (void *)a[i];
    return t;
}

// ---- the edge-aware disparity filter (include/sgm_hip_wls.h, sgm_hip_wls_batch.h; kernels_wls.h) ------------------------------
// One map is a batch of one: the single entries and the batch entries run the same four kernels.
int sgm_wls_weights(double sigma, float lut[256])
{
    if (!lut || !std::isfinite(sigma) || sigma <= 0.0) return set_err(SGM_ERR_INVALID_ARG, "sgm_wls_weights: null table or sigma %g not a positive finite number", sigma);
    for (int k = 0; k < 256; k++) lut[k] = (float)exp(-(double)k / sigma);
    return SGM_OK;
}

static int wls_check_args(const sgm_engine *e, const void *disp, const void *guide, int cn, int H, int W, int invalid, double lambda,
                          const float *lut, const void *out)
{
    if (!e || !disp || !guide || !lut || !out) return set_err(SGM_ERR_INVALID_ARG, "sgm_wls_filter: null pointer");
    if (H <= 0 || W <= 0) return set_err(SGM_ERR_INVALID_ARG, "sgm_wls_filter: bad shape H=%d W=%d", H, W);
    if (cn != 1 && cn != 3) return set_err(SGM_ERR_INVALID_ARG, "sgm_wls_filter: guide with %d channels (1 or 3)", cn);
    if (!std::isfinite(lambda) || lambda < 0.0 || lambda > 1e7) return set_err(SGM_ERR_INVALID_ARG, "sgm_wls_filter: lambda %g outside [0, 1e7]", lambda);
    if (invalid < -32768 || invalid > 32767) return set_err(SGM_ERR_INVALID_ARG, "sgm_wls_filter: invalid value %d outside int16", invalid);
    return SGM_OK;
}

// The shapes of the line kernels.  Entry 0 is the one the library uses for a chunk of several maps, entries 3 (rows) and 1
// (columns) for a chunk of one (run_wls_batch); the others are what DESIGN.md 4.15 / 4.16 measured against them and stay
// reachable through SGM_OPT_DEBUG (sgm_debug.h) for tools/wls_batch_times.py.  Every shape gives the same bits.
struct WlsRowsShape { int rw, tc; };   // k_wls_rows<CN, RW, TC>: waves per workgroup, columns per tile
static const WlsRowsShape wls_rows_shapes[] = {{4, 32}, {2, 64}, {1, 64}, {4, 64}, {2, 32}};
static const int wls_cols_shapes[] = {8, 16, 32, 4};   // k_wls_cols<CN, UNR>: rows in flight per lane

extern "C++" {   // (templates: this part of the file has C linkage)
template <int CN>
static void launch_wls_rows(int shape, dim3 grid, hipStream_t st, float *u, float *v, float *c, const MapPtrs &g, const WlsLut &t,
                            float lam, int H, int W)
{
    switch (shape) {
    case 1: hipLaunchKernelGGL((k_wls_rows<CN, 2, 64>), grid, dim3(2 * WLS_T), 0, st, u, v, c, g, t, lam, H, W); break;
    case 2: hipLaunchKernelGGL((k_wls_rows<CN, 1, 64>), grid, dim3(1 * WLS_T), 0, st, u, v, c, g, t, lam, H, W); break;
    case 3: hipLaunchKernelGGL((k_wls_rows<CN, 4, 64>), grid, dim3(4 * WLS_T), 0, st, u, v, c, g, t, lam, H, W); break;
    case 4: hipLaunchKernelGGL((k_wls_rows<CN, 2, 32>), grid, dim3(2 * WLS_T), 0, st, u, v, c, g, t, lam, H, W); break;
    default: hipLaunchKernelGGL((k_wls_rows<CN, 4, 32>), grid, dim3(4 * WLS_T), 0, st, u, v, c, g, t, lam, H, W); break;
    }
}
template <int CN>
static void launch_wls_cols(int shape, dim3 grid, hipStream_t st, float *u, float *v, float *c, const MapPtrs &g, const WlsLut &t,
                            float lam, int H, int W)
{
    switch (shape) {
    case 1: hipLaunchKernelGGL((k_wls_cols<CN, 16>), grid, dim3(WLS_T), 0, st, u, v, c, g, t, lam, H, W); break;
    case 2: hipLaunchKernelGGL((k_wls_cols<CN, 32>), grid, dim3(WLS_T), 0, st, u, v, c, g, t, lam, H, W); break;
    case 3: hipLaunchKernelGGL((k_wls_cols<CN, 4>), grid, dim3(WLS_T), 0, st, u, v, c, g, t, lam, H, W); break;
    default: hipLaunchKernelGGL((k_wls_cols<CN, 8>), grid, dim3(WLS_T), 0, st, u, v, c, g, t, lam, H, W); break;
    }
}
}  // extern "C++"

static int wls_batch_check_args(const sgm_engine *e, int N, const void *const *disp, const void *const *guide, int cn,
                                const void *const *conf, int H, int W, int invalid, double lambda, const float *lut,
                                const void *const *out, const void *const *outf, bool arrays)
{
    if (N <= 0) return set_err(SGM_ERR_INVALID_ARG, "sgm_wls_filter_batch: N=%d maps", N);
    if (int rc = wls_check_args(e, disp, guide, cn, H, W, invalid, lambda, lut, out)) return rc;
    if (!arrays) return SGM_OK;
    for (int i = 0; i < N; i++)
        if (!disp[i] || !guide[i] || !out[i] || (conf && !conf[i]) || (outf && !outf[i]))
            return set_err(SGM_ERR_INVALID_ARG, "sgm_wls_filter_batch: null pointer for map %d", i);
    return SGM_OK;
}

// One chunk of n <= BATCH_MAPS_MAX maps: init, three times (rows, columns), final, every launch over all n maps.  conf / outf: null
// for none.  The planes hold n maps (batch_reserve).
static int run_wls_batch(sgm_engine *e, int n, const void *const *d_disp, const void *const *d_guide, int cn, const void *const *d_conf,
                         int H, int W, int invalid, double lambda, const float *lut, void *const *d_out, void *const *d_outf)
{
    const int64_t npx = (int64_t)H * W;
    float *u = (float *)e->wls_u.p, *v = (float *)e->wls_v.p, *c = (float *)e->wls_c.p;
    WlsLut t;
    memcpy(t.w, lut, sizeof(t.w));
    const MapPtrs disps = map_ptrs(d_disp, n), guides = map_ptrs(d_guide, n), confs = map_ptrs(d_conf, n), outs = map_ptrs(d_out, n),
                  outfs = map_ptrs(d_outf, n);
    const unsigned rsh = ((unsigned)e->debug >> SGM_DBG_WLS_BATCH_ROWS_SHIFT) & 7, csh = ((unsigned)e->debug >> SGM_DBG_WLS_BATCH_COLS_SHIFT) & 3;
    // a chunk of one map has the CUs to itself, one workgroup each at most: there 64-column tiles and 16 rows in flight are the
    // faster shapes (entries 3 and 1).  A non-zero debug field overrides that.
    const int rshape = !rsh ? (n == 1 ? 3 : 0) : rsh < sizeof(wls_rows_shapes) / sizeof(wls_rows_shapes[0]) ? (int)rsh : 0;
    const int cshape = !csh ? (n == 1 ? 1 : 0) : csh < sizeof(wls_cols_shapes) / sizeof(wls_cols_shapes[0]) ? (int)csh : 0;
    const dim3 px((unsigned)((npx + 255) / 256), n);
    int rc;
    stage_break(e);   // (the host entry's copies lie between the chunks)
    rc = run_stage(e, "wls_init", [&] {
        hipLaunchKernelGGL(k_wls_init, px, dim3(256), 0, e->stream, disps, confs, invalid, npx, u, v);
        return 1;
    });
    if (rc) return rc;
    const int T = 3;
    for (int it = 1; it <= T; it++) {
        const float lam = (float)(1.5 * lambda * (double)(1 << (2 * (T - it))) / (double)((1 << (2 * T)) - 1));
        if (W > 1) {   // (a line of one element is the identity)
            const dim3 grid((H + WLS_T - 1) / WLS_T, n);
            rc = run_stage(e, "wls_rows", [&] {
                if (cn == 3) launch_wls_rows<3>(rshape, grid, e->stream, u, v, c, guides, t, lam, H, W);
                else launch_wls_rows<1>(rshape, grid, e->stream, u, v, c, guides, t, lam, H, W);
                return 1;
            });
            if (rc) return rc;
        }
        if (H > 1) {
            const dim3 grid((W + WLS_T - 1) / WLS_T, n);
            rc = run_stage(e, "wls_cols", [&] {
                if (cn == 3) launch_wls_cols<3>(cshape, grid, e->stream, u, v, c, guides, t, lam, H, W);
                else launch_wls_cols<1>(cshape, grid, e->stream, u, v, c, guides, t, lam, H, W);
                return 1;
            });
            if (rc) return rc;
        }
    }
    return run_stage(e, "wls_final", [&] {
        hipLaunchKernelGGL(k_wls_final, px, dim3(256), 0, e->stream, (const float *)u, (const float *)v, invalid, npx, outs, outfs);
        return 1;
    });
}

int sgm_wls_filter_batch_device(sgm_engine *e, int N, const void *const *d_disp_i16, const void *const *d_guide_u8, int cn,
                                const void *const *d_conf_u8, int H, int W, int invalid, double lambda, const float lut[256],
                                void *const *d_out_i16, void *const *d_out_f32)
{
    if (int rc = wls_batch_check_args(e, N, d_disp_i16, d_guide_u8, cn, d_conf_u8, H, W, invalid, lambda, lut, d_out_i16, d_out_f32, true))
        return rc;
    HIP_TRY(hipSetDevice(e->device));
    const size_t pb = (size_t)H * W * 4;
    int rc, C = 1;
    if ((rc = batch_reserve(e, N, {{&e->wls_u, pb}, {&e->wls_v, pb}, {&e->wls_c, pb}}, &C))) return rc;
    if (e->profile) stage_reset(e);   // the stage record is the call's from here on
    for (int i0 = 0; i0 < N; i0 += C)
        if ((rc = run_wls_batch(e, std::min(C, N - i0), d_disp_i16 + i0, d_guide_u8 + i0, cn, d_conf_u8 ? d_conf_u8 + i0 : nullptr, H, W,
                                invalid, lambda, lut, d_out_i16 + i0, d_out_f32 ? d_out_f32 + i0 : nullptr)))
            return rc;
    return SGM_OK;
}

int sgm_wls_filter_batch(sgm_engine *e, int N, const int16_t *disp, const uint8_t *guide, int cn, const uint8_t *conf, int H, int W,
                         int invalid, double lambda, const float lut[256], int16_t *out, float *out_f32)
{
    if (int rc = wls_batch_check_args(e, N, (const void *const *)disp, (const void *const *)guide, cn, nullptr, H, W, invalid, lambda, lut,
                                      (const void *const *)out, nullptr, false))
        return rc;
    HIP_TRY(hipSetDevice(e->device));
    const size_t npx = (size_t)H * W, pb = npx * 4;
    // staging, [C] of each: the maps in disp_out (filtered in place), the guides in in_left, the confidence maps in in_right, the
    // float maps in f32
    int rc, C = 1;
    if ((rc = batch_reserve(e, N, {{&e->wls_u, pb}, {&e->wls_v, pb}, {&e->wls_c, pb}, {&e->disp_out, npx * 2}, {&e->in_left, npx * cn},
                                   {&e->in_right, conf ? npx : 0}, {&e->f32, out_f32 ? pb : 0}}, &C)))
        return rc;
    if (e->profile) stage_reset(e);   // the stage record is the call's from here on
    std::vector<void *> pd(C), pg(C), pc(C), pf(C);
    for (int k = 0; k < C; k++) {
        pd[k] = (char *)e->disp_out.p + (size_t)k * npx * 2;
        pg[k] = (char *)e->in_left.p + (size_t)k * npx * cn;
        pc[k] = conf ? (char *)e->in_right.p + (size_t)k * npx : nullptr;
        pf[k] = out_f32 ? (char *)e->f32.p + (size_t)k * pb : nullptr;
    }
    for (int i0 = 0; i0 < N; i0 += C) {
        const size_t n = (size_t)std::min(C, N - i0), o = (size_t)i0 * npx;
        HIP_TRY(hipMemcpyAsync(e->disp_out.p, disp + o, n * npx * 2, hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipMemcpyAsync(e->in_left.p, guide + o * cn, n * npx * cn, hipMemcpyHostToDevice, e->stream));
        if (conf) HIP_TRY(hipMemcpyAsync(e->in_right.p, conf + o, n * npx, hipMemcpyHostToDevice, e->stream));
        if ((rc = run_wls_batch(e, (int)n, pd.data(), pg.data(), cn, conf ? pc.data() : nullptr, H, W, invalid, lambda, lut, pd.data(),
                                out_f32 ? pf.data() : nullptr))) {
            (void)hipStreamSynchronize(e->stream);   // (the caller's memory is the target of nothing when the call returns)
            return rc;
        }
        HIP_TRY(hipMemcpyAsync(out + o, e->disp_out.p, n * npx * 2, hipMemcpyDeviceToHost, e->stream));
        if (out_f32) HIP_TRY(hipMemcpyAsync(out_f32 + o, e->f32.p, n * pb, hipMemcpyDeviceToHost, e->stream));
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    return SGM_OK;
}

// the single entries: their own refusals (sgm_wls_filter: ...), then a batch of one
int sgm_wls_filter_device(sgm_engine *e, const void *d_disp_i16, const void *d_guide_u8, int cn, const void *d_conf_u8, int H, int W,
                          int invalid, double lambda, const float lut[256], void *d_out_i16, void *d_out_f32)
{
    if (int rc = wls_check_args(e, d_disp_i16, d_guide_u8, cn, H, W, invalid, lambda, lut, d_out_i16)) return rc;
    return sgm_wls_filter_batch_device(e, 1, &d_disp_i16, &d_guide_u8, cn, d_conf_u8 ? &d_conf_u8 : nullptr, H, W, invalid, lambda, lut,
                                       &d_out_i16, d_out_f32 ? &d_out_f32 : nullptr);
}

int sgm_wls_filter(sgm_engine *e, const int16_t *disp, const uint8_t *guide, int cn, const uint8_t *conf, int H, int W, int invalid,
                   double lambda, const float lut[256], int16_t *out, float *out_f32)
{
    if (int rc = wls_check_args(e, disp, guide, cn, H, W, invalid, lambda, lut, out)) return rc;
    return sgm_wls_filter_batch(e, 1, disp, guide, cn, conf, H, W, invalid, lambda, lut, out, out_f32);
}

// ---- the left-right consistency confidence (include/sgm_hip_lrc.h, kernels_lrc.h) ---------------------------------------------
// One pair is a batch of one: the single entries and the batch entry run the same two kernels.
static int lrc_check_args(const sgm_engine *e, const void *left, const void *right, int H, int W, int invalid, int thresh, int radius,
                          int var_max, const void *cl, const void *cr)
{
    if (!e || !left || !right) return set_err(SGM_ERR_INVALID_ARG, "sgm_lrc_confidence: null pointer");
    if (!cl && !cr) return set_err(SGM_ERR_INVALID_ARG, "sgm_lrc_confidence: both outputs are null");
    if (H <= 0 || W <= 0) return set_err(SGM_ERR_INVALID_ARG, "sgm_lrc_confidence: bad shape H=%d W=%d", H, W);
    if (invalid < -32768 || invalid > 32767) return set_err(SGM_ERR_INVALID_ARG, "sgm_lrc_confidence: invalid value %d outside int16", invalid);
    if (thresh < 0 || thresh > 32767) return set_err(SGM_ERR_INVALID_ARG, "sgm_lrc_confidence: thresh %d outside 0 .. 32767", thresh);
    if (radius < 0 || radius > LRC_RMAX) return set_err(SGM_ERR_INVALID_ARG, "sgm_lrc_confidence: radius %d outside 0 .. %d", radius, LRC_RMAX);
    if (var_max < 1 || var_max > (1 << 30)) return set_err(SGM_ERR_INVALID_ARG, "sgm_lrc_confidence: var_max %d outside 1 .. 2^30", var_max);
    return SGM_OK;
}

// no output of any pair is an input of any pair, or another output
static int lrc_check_overlap(int N, const void *const *left, const void *const *right, const void *const *base, const void *const *cl,
                             const void *const *cr)
{
    std::vector<const void *> in, out;
    for (int i = 0; i < N; i++) {
        in.push_back(left[i]);
        in.push_back(right[i]);
        if (base) in.push_back(base[i]);
        if (cl) out.push_back(cl[i]);
        if (cr) out.push_back(cr[i]);
    }
    std::sort(in.begin(), in.end());
    std::sort(out.begin(), out.end());
    for (size_t k = 0; k < out.size(); k++)
        if (std::binary_search(in.begin(), in.end(), out[k]) || (k && out[k] == out[k - 1]))
            return set_err(SGM_ERR_INVALID_ARG, "sgm_lrc_confidence: an output is also an input or another output (outputs must not overlap anything)");
    return SGM_OK;
}

// One chunk of n <= BATCH_MAPS_MAX pairs, arguments checked, lrc_f holding n pairs of planes: factor, match.
static int run_lrc_batch(sgm_engine *e, int n, const void *const *d_left, const void *const *d_right, const void *const *d_base, int H,
                         int W, int invalid, int thresh, int radius, int var_max, void *const *d_cl, void *const *d_cr)
{
    const MapPtrs lefts = map_ptrs(d_left, n), rights = map_ptrs(d_right, n), bases = map_ptrs(d_base, n), cls = map_ptrs(d_cl, n),
                  crs = map_ptrs(d_cr, n);
    uint8_t *fac = (uint8_t *)e->lrc_f.p;
    int rc;
    stage_break(e);
    rc = run_stage(e, "lrc_factor", [&] {
        hipLaunchKernelGGL(k_lrc_factor, dim3((W + LRC_TW - 1) / LRC_TW, (H + LRC_TH - 1) / LRC_TH, 2 * n), dim3(LRC_THREADS),
                           lrc_lds_bytes(radius), e->stream, lefts, rights, invalid, radius, (int64_t)var_max, H, W, fac);
        return 1;
    });
    if (rc) return rc;
    return run_stage(e, "lrc_match", [&] {
        hipLaunchKernelGGL(k_lrc_match, dim3((W + 255) / 256, H, n), dim3(256), 0, e->stream, lefts, rights, bases, invalid, thresh, H, W,
                           (const uint8_t *)fac, cls, crs);
        return 1;
    });
}

int sgm_lrc_confidence_batch_device(sgm_engine *e, int N, const void *const *d_lefts, const void *const *d_rights,
                                    const void *const *d_bases, int H, int W, int invalid, int thresh, int radius, int var_max,
                                    void *const *d_conf_lefts, void *const *d_conf_rights)
{
    if (N <= 0) return set_err(SGM_ERR_INVALID_ARG, "sgm_lrc_confidence_batch: N=%d pairs", N);
    if (int rc = lrc_check_args(e, d_lefts, d_rights, H, W, invalid, thresh, radius, var_max, d_conf_lefts, d_conf_rights)) return rc;
    for (int i = 0; i < N; i++)
        if (!d_lefts[i] || !d_rights[i] || (d_bases && !d_bases[i]) || (d_conf_lefts && !d_conf_lefts[i]) ||
            (d_conf_rights && !d_conf_rights[i]))
            return set_err(SGM_ERR_INVALID_ARG, "sgm_lrc_confidence_batch: null pointer for pair %d", i);
    if (int rc = lrc_check_overlap(N, d_lefts, d_rights, d_bases, d_conf_lefts, d_conf_rights)) return rc;
    HIP_TRY(hipSetDevice(e->device));
    int rc, C = 1;
    if ((rc = batch_reserve(e, N, {{&e->lrc_f, (size_t)H * W * 2}}, &C))) return rc;
    if (e->profile) stage_reset(e);   // the stage record is the call's from here on
    for (int i0 = 0; i0 < N; i0 += C)
        if ((rc = run_lrc_batch(e, std::min(C, N - i0), d_lefts + i0, d_rights + i0, d_bases ? d_bases + i0 : nullptr, H, W, invalid,
                                thresh, radius, var_max, d_conf_lefts ? d_conf_lefts + i0 : nullptr,
                                d_conf_rights ? d_conf_rights + i0 : nullptr)))
            return rc;
    return SGM_OK;
}

int sgm_lrc_confidence_device(sgm_engine *e, const void *d_left_i16, const void *d_right_i16, const void *d_base_u8, int H, int W,
                              int invalid, int thresh, int radius, int var_max, void *d_conf_left_u8, void *d_conf_right_u8)
{
    if (int rc = lrc_check_args(e, d_left_i16, d_right_i16, H, W, invalid, thresh, radius, var_max, d_conf_left_u8, d_conf_right_u8))
        return rc;
    return sgm_lrc_confidence_batch_device(e, 1, &d_left_i16, &d_right_i16, d_base_u8 ? &d_base_u8 : nullptr, H, W, invalid, thresh,
                                           radius, var_max, d_conf_left_u8 ? &d_conf_left_u8 : nullptr,
                                           d_conf_right_u8 ? &d_conf_right_u8 : nullptr);
}

int sgm_lrc_confidence(sgm_engine *e, const int16_t *disp_left, const int16_t *disp_right, const uint8_t *base, int H, int W,
                       int invalid, int thresh, int radius, int var_max, uint8_t *conf_left, uint8_t *conf_right)
{
    if (int rc = lrc_check_args(e, disp_left, disp_right, H, W, invalid, thresh, radius, var_max, conf_left, conf_right)) return rc;
    {
        const void *l = disp_left, *r = disp_right, *b = base, *cl = conf_left, *cr = conf_right;
        if (int rc = lrc_check_overlap(1, &l, &r, base ? &b : nullptr, conf_left ? &cl : nullptr, conf_right ? &cr : nullptr)) return rc;
    }
    HIP_TRY(hipSetDevice(e->device));
    const size_t npx = (size_t)H * W;
    int rc;
    // staging: the left map in disp_out, the right map in disp_raw, base in in_left, the two results in in_right and mask
    if ((rc = e->disp_out.ensure(npx * 2)) || (rc = e->disp_raw.ensure(npx * 2)) || (base && (rc = e->in_left.ensure(npx))) ||
        (conf_left && (rc = e->in_right.ensure(npx))) || (conf_right && (rc = e->mask.ensure(npx))))
        return rc;
    HIP_TRY(hipMemcpyAsync(e->disp_out.p, disp_left, npx * 2, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->disp_raw.p, disp_right, npx * 2, hipMemcpyHostToDevice, e->stream));
    if (base) HIP_TRY(hipMemcpyAsync(e->in_left.p, base, npx, hipMemcpyHostToDevice, e->stream));
    if ((rc = sgm_lrc_confidence_device(e, e->disp_out.p, e->disp_raw.p, base ? e->in_left.p : nullptr, H, W, invalid, thresh, radius,
                                        var_max, conf_left ? e->in_right.p : nullptr, conf_right ? e->mask.p : nullptr))) {
        (void)hipStreamSynchronize(e->stream);   // (the caller's memory is the source of nothing when the call returns)
        return rc;
    }
    if (conf_left) HIP_TRY(hipMemcpyAsync(conf_left, e->in_right.p, npx, hipMemcpyDeviceToHost, e->stream));
    if (conf_right) HIP_TRY(hipMemcpyAsync(conf_right, e->mask.p, npx, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return SGM_OK;
}

// ---- voxel-grid downsampling (include/sgm_hip_voxel.h, kernels_voxel.h) ------------------------------------------------------
static int voxel_check_args(const sgm_engine *e, const void *xyz, const void *colors, int64_t n, float v, const float *origin,
                            int min_points, const void *out_points, const void *out_colors, const int64_t *n_voxels)
{
    if (!e || !xyz || !out_points || !n_voxels) return set_err(SGM_ERR_INVALID_ARG, "sgm_voxel_downsample: null pointer");
    if (n < 0) return set_err(SGM_ERR_INVALID_ARG, "sgm_voxel_downsample: n=%lld points", (long long)n);
    if (!std::isfinite(v) || !(v > 0.0f) || !std::isfinite(1.0f / v))
        return set_err(SGM_ERR_INVALID_ARG, "sgm_voxel_downsample: voxel_size %g is not finite and positive with a finite reciprocal", (double)v);
    if (!origin || !std::isfinite(origin[0]) || !std::isfinite(origin[1]) || !std::isfinite(origin[2]))
        return set_err(SGM_ERR_INVALID_ARG, "sgm_voxel_downsample: the origin is null or not finite");
    if (min_points < 1) return set_err(SGM_ERR_INVALID_ARG, "sgm_voxel_downsample: min_points %d < 1", min_points);
    if (out_colors && !colors) return set_err(SGM_ERR_INVALID_ARG, "sgm_voxel_downsample: out_colors requested without colors");
    if (n > VOX_MAX_POINTS)
        return set_err(SGM_ERR_UNSUPPORTED, "sgm_voxel_downsample: %lld points, more than 2^24 - 1 (the widths of a voxel's sums)", (long long)n);
    return SGM_OK;
}

// the result of a call that found no point in range, for the two calls that report a count and the points out of range
static void cloud_nothing(int64_t *n_result, int64_t *n_out_of_range, int64_t n_out)
{
    *n_result = 0;
    if (n_out_of_range) *n_out_of_range = n_out;
}

int sgm_voxel_downsample_device(sgm_engine *e, const void *d_xyz, const void *d_disp_f32, const void *d_colors_rgb, int64_t n,
                                float voxel_size, const float origin[3], int min_points, void *d_out_points, void *d_out_colors,
                                void *d_out_counts, int64_t *n_voxels, int64_t *n_out_of_range)
{
    if (int rc = voxel_check_args(e, d_xyz, d_colors_rgb, n, voxel_size, origin, min_points, d_out_points, d_out_colors, n_voxels)) return rc;
    if (n == 0) return cloud_nothing(n_voxels, n_out_of_range, 0), SGM_OK;
    HIP_TRY(hipSetDevice(e->device));
    const int m = (int)((n + 255) / 256);
    int rc;
    if ((rc = e->vox_ctl.ensure(VOX_CTL_WORDS * 4)) || (rc = e->vox_slot.ensure((size_t)n * 4)) || (rc = e->ccount.ensure((size_t)(m + 1) * 4)))
        return rc;
    if (e->profile) stage_reset(e);   // the stage record is the call's from here on
    const VoxGrid G{1.0f / voxel_size, voxel_size, origin[0], origin[1], origin[2]};
    const float *xyz = (const float *)d_xyz, *disp = (const float *)d_disp_f32;
    const uint8_t *colors = (const uint8_t *)(d_out_colors ? d_colors_rgb : nullptr);
    uint32_t *ctl = (uint32_t *)e->vox_ctl.p, *slot_of = (uint32_t *)e->vox_slot.p, *cnt = (uint32_t *)e->ccount.p;
    hipStream_t st = e->stream;
    // 1. how many points arrive: the table is sized from them, and a cloud with none is done here
    HIP_TRY(hipMemsetAsync(ctl, 0, VOX_CTL_WORDS * 4, st));
    stage_break(e);
    rc = run_stage(e, "voxel_count", [&] {
        hipLaunchKernelGGL(k_voxel_count, dim3(std::min(m, VOX_COUNT_BLOCKS)), dim3(256), 0, st, xyz, disp, n, G, ctl);
        return 1;
    });
    if (rc) return rc;
    uint32_t h_ctl[VOX_CTL_WORDS] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(h_ctl, ctl, sizeof(h_ctl), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    stage_break(e);
    const uint32_t n_in = h_ctl[VOX_CTL_IN];
    if (n_in == 0) return cloud_nothing(n_voxels, n_out_of_range, (int64_t)h_ctl[VOX_CTL_OUT]), SGM_OK;
    if (n_out_of_range) *n_out_of_range = (int64_t)h_ctl[VOX_CTL_OUT];
    // 2. the table: the smallest power of two of at least twice the points in range (debug: of at least the points themselves)
    const uint64_t want = (e->debug & SGM_DBG_VOXEL_TIGHT_TABLE) ? (uint64_t)n_in : 2 * (uint64_t)n_in;
    uint32_t cap = 1;
    while (cap < want) cap <<= 1;   // (n_in < 2^24: at most 2^25)
    if ((rc = e->vox_tab.ensure((size_t)cap * sizeof(VoxSlot)))) return rc;
    VoxSlot *tab = (VoxSlot *)e->vox_tab.p;
    if ((rc = run_stage(e, "voxel_clear", [&] { hipLaunchKernelGGL(k_voxel_clear, dim3((cap + 255) / 256), dim3(256), 0, st, tab, cap); return 1; })))
        return rc;
    // 3. insert and accumulate
    rc = run_stage(e, "voxel_insert", [&] {
        const bool pre = VOX_PRE_DEFAULT != !!(e->debug & SGM_DBG_VOXEL_OTHER_REDUCTION);
        if (pre) hipLaunchKernelGGL(k_voxel_insert<true>, dim3(m), dim3(256), 0, st, xyz, disp, colors, n, G, tab, cap - 1, slot_of, ctl);
        else hipLaunchKernelGGL(k_voxel_insert<false>, dim3(m), dim3(256), 0, st, xyz, disp, colors, n, G, tab, cap - 1, slot_of, ctl);
        return 1;
    });
    if (rc) return rc;
    // 4. the heads of the kept voxels through the ordered compaction; the scatter computes the rows
    rc = run_stage(e, "voxel_heads", [&] {
        hipLaunchKernelGGL(k_voxel_head_count, dim3(m), dim3(256), 0, st, (const uint32_t *)slot_of, (const VoxSlot *)tab, n, (uint32_t)min_points, cnt);
        hipLaunchKernelGGL(k_compact_scan, dim3(1), dim3(1024), 0, st, cnt, m);
        hipLaunchKernelGGL(k_voxel_scatter, dim3(m), dim3(256), 0, st, (const uint32_t *)slot_of, (const VoxSlot *)tab, n, (uint32_t)min_points,
                           (const uint32_t *)cnt, G, (float *)d_out_points, (uint8_t *)d_out_colors, (uint32_t *)d_out_counts);
        return 3;
    });
    if (rc) return rc;
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(h_ctl, ctl, sizeof(h_ctl), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&total, cnt + m, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (h_ctl[VOX_CTL_ERR])
        return set_err(SGM_ERR_HIP, "sgm_voxel_downsample: a point found no slot in a table of %u slots for %u points", cap, n_in);
    *n_voxels = (int64_t)total;
    return SGM_OK;
}

int sgm_voxel_downsample(sgm_engine *e, const float *xyz, const float *disp, const uint8_t *colors_rgb, int64_t n, float voxel_size,
                         const float origin[3], int min_points, float *out_points, uint8_t *out_colors, uint32_t *out_counts,
                         int64_t *n_voxels, int64_t *n_out_of_range)
{
    if (int rc = voxel_check_args(e, xyz, colors_rgb, n, voxel_size, origin, min_points, out_points, out_colors, n_voxels)) return rc;
    if (n == 0) return cloud_nothing(n_voxels, n_out_of_range, 0), SGM_OK;
    int64_t nv = 0, noor = 0;
    const HostOut pts{out_points, &e->cpts, 12, &nv}, rgb{out_colors, &e->crgb, 3, &nv}, cnt{out_counts, &e->vox_cnt, 4, &nv};
    if (int rc = cloud_host_call(e, xyz, disp, out_colors ? colors_rgb : nullptr, n, {pts, rgb, cnt}, [&](void *d_disp, void *d_colors) {
            return sgm_voxel_downsample_device(e, e->xyz.p, d_disp, d_colors, n, voxel_size, origin, min_points, pts.d(), rgb.d(), cnt.d(), &nv,
                                               &noor);
        }))
        return rc;
    *n_voxels = nv;
    if (n_out_of_range) *n_out_of_range = noor;
    return SGM_OK;
}

// ---- radius outlier removal (include/sgm_hip_radius.h, kernels_radius.h) -------------------------------------------------------
// What the four calls on the grid of cells check alike, in the order they check it: null pointers, n, the radius under the entry's
// word for it (scale: a further quotient scale / r that must stay finite, or 0), the origin, the number of points.  own(after)
// makes the entry's own checks that stand behind the check on n (after = 0), the radius (1) and the origin (2).
extern "C++" {   // (a template: this part of the file has C linkage)
template <class Own>
static int cloud_check_args(const char *who, bool null, int64_t n, const char *rname, float r, float scale, const float *origin, Own own)
{
    int rc;
    if (null) return set_err(SGM_ERR_INVALID_ARG, "%s: null pointer", who);
    if (n < 0) return set_err(SGM_ERR_INVALID_ARG, "%s: n=%lld points", who, (long long)n);
    if ((rc = own(0))) return rc;
    const float r2 = r * r, v = r * 1.03125f;
    if (!std::isfinite(r) || !(r > 0.0f) || !std::isnormal(r2) || !std::isfinite(1.0f / v) || !std::isfinite(scale / r))
        return set_err(SGM_ERR_INVALID_ARG, "%s: %s %g is not finite and positive with a finite normal square", who, rname, (double)r);
    if ((rc = own(1))) return rc;
    if (!origin || !std::isfinite(origin[0]) || !std::isfinite(origin[1]) || !std::isfinite(origin[2]))
        return set_err(SGM_ERR_INVALID_ARG, "%s: the origin is null or not finite", who);
    if ((rc = own(2))) return rc;
    if (n > RAD_MAX_POINTS)
        return set_err(SGM_ERR_UNSUPPORTED, "%s: %lld points, more than 2^24 - 1 (a source index shares a record with its point)", who, (long long)n);
    return SGM_OK;
}
}  // extern "C++"

static int radius_check_args(const sgm_engine *e, const void *xyz, const void *colors, int64_t n, float r, const float *origin,
                             int nb_points, int max_count, const void *out_colors, const int64_t *n_kept)
{
    return cloud_check_args("sgm_radius_outlier", !e || !xyz || !n_kept, n, "radius", r, 0.0f, origin, [&](int after) -> int {
        if (after != 2) return SGM_OK;
        if (nb_points < 1) return set_err(SGM_ERR_INVALID_ARG, "sgm_radius_outlier: nb_points %d < 1", nb_points);
        if (max_count < nb_points) return set_err(SGM_ERR_INVALID_ARG, "sgm_radius_outlier: max_count %d < nb_points %d", max_count, nb_points);
        if (out_colors && !colors) return set_err(SGM_ERR_INVALID_ARG, "sgm_radius_outlier: out_colors requested without colors");
        return SGM_OK;
    });
}

// The grid of cells of one call, as radius_build_grid leaves it
struct CloudGrid {
    RadGrid G;
    uint32_t n_in, n_out, cap, mask;   // points in range, valid points out of range, the table's slots (0 with no point in range)
    const RadSlot *tab;                // rad_tab
    float4 *sorted;                    // rad_sorted: n_in records
    uint2 *slot_rank;                  // rad_pt: n pairs
    int m;                             // blocks of 256 over the n points
};

static int cloud_no_slot(const char *who, const CloudGrid &g)
{
    return set_err(SGM_ERR_HIP, "%s: a point found no slot in a table of %u slots for %u points", who, g.cap, g.n_in);
}

// The grid of cells every search runs on, steps 1 to 5 of the device entries: the control words, the count of the points that
// arrive (read back: n_in, n_out; with none the call is done and nothing else is built), then the table (cap slots in rad_tab),
// each point's slot and rank (rad_pt), the cells' starts and the records sorted by cell (rad_sorted).  keep and counts are what
// k_radius_sort zeroes for the points in no cell (counts may be null).  names: the five stage names of the caller's record.
static int radius_build_grid(sgm_engine *e, const float *xyz, const float *disp, int64_t n, float r, const float origin[3], uint8_t *keep,
                             uint32_t *counts, const char *const names[5], CloudGrid *g)
{
    const int m = (int)((n + 255) / 256);
    int rc;
    uint32_t *ctl = (uint32_t *)e->rad_ctl.p;
    uint2 *slot_rank = (uint2 *)e->rad_pt.p;
    hipStream_t st = e->stream;
    const RadGrid G{1.0f / (r * 1.03125f), r * r, origin[0], origin[1], origin[2]};
    *g = CloudGrid{G, 0, 0, 0, 0, nullptr, nullptr, slot_rank, m};
    // 1. how many points arrive: the table and the sorted records are sized from them, and a cloud with none is done here
    HIP_TRY(hipMemsetAsync(ctl, 0, RAD_CTL_WORDS * 4, st));
    stage_break(e);
    rc = run_stage(e, names[0], [&] {
        hipLaunchKernelGGL(k_radius_count, dim3(std::min(m, RAD_COUNT_BLOCKS)), dim3(256), 0, st, xyz, disp, n, G, ctl);
        return 1;
    });
    if (rc) return rc;
    uint32_t h_ctl[RAD_CTL_WORDS] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(h_ctl, ctl, sizeof(h_ctl), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    stage_break(e);
    const uint32_t n_in = g->n_in = h_ctl[RAD_CTL_IN];
    g->n_out = h_ctl[RAD_CTL_OUT];
    if (n_in == 0) return SGM_OK;
    // 2. the table: the smallest power of two of at least twice the points in range (debug: of at least the points themselves)
    const uint64_t want = (e->debug & SGM_DBG_RADIUS_TIGHT_TABLE) ? (uint64_t)n_in : 2 * (uint64_t)n_in;
    uint32_t cap = 1;
    while (cap < want) cap <<= 1;   // (n_in < 2^24: at most 2^25)
    g->cap = cap, g->mask = cap - 1;
    if ((rc = e->rad_tab.ensure((size_t)cap * sizeof(RadSlot))) || (rc = e->rad_sorted.ensure((size_t)n_in * 16))) return rc;
    RadSlot *tab = (RadSlot *)e->rad_tab.p;
    float4 *sorted = g->sorted = (float4 *)e->rad_sorted.p;
    g->tab = tab;
    if ((rc = run_stage(e, names[1], [&] { hipLaunchKernelGGL(k_radius_clear, dim3((cap + 255) / 256), dim3(256), 0, st, tab, cap); return 1; })))
        return rc;
    // 3. insert: each point's cell and its rank there
    rc = run_stage(e, names[2], [&] {
        hipLaunchKernelGGL(k_radius_insert, dim3(m), dim3(256), 0, st, xyz, disp, n, G, tab, cap - 1, slot_rank, ctl);
        return 1;
    });
    if (rc) return rc;
    // 4. where each cell's run begins
    rc = run_stage(e, names[3], [&] {
        hipLaunchKernelGGL(k_radius_starts, dim3((cap + RAD_STARTS_PER_BLOCK - 1) / RAD_STARTS_PER_BLOCK), dim3(256), 0, st, tab, cap, ctl);
        return 1;
    });
    if (rc) return rc;
    // 5. the records sorted by cell; the points in no cell get their zeros
    return run_stage(e, names[4], [&] {
        hipLaunchKernelGGL(k_radius_sort, dim3(m), dim3(256), 0, st, xyz, n, (const RadSlot *)tab, (const uint2 *)slot_rank, sorted, keep, counts);
        return 1;
    });
}

// step 7 of both: the kept points through the ordered compaction; *total comes back with the call's control words (blocks), and
// a set RAD_CTL_ERR is the error of `who` (cloud_no_slot)
// The ordered compaction of the points with a set keep byte: the blocks' counts, their scan (the total behind them in ccount) and,
// when an output of rows is asked for, the scatter.  Returns the launches, for the caller's stage.
static int launch_keep_compaction(sgm_engine *e, int m, const uint8_t *keep, const float *xyz, const uint8_t *colors, int64_t n,
                                  void *d_out_points, void *d_out_colors, void *d_out_index)
{
    uint32_t *cnt = (uint32_t *)e->ccount.p;
    hipLaunchKernelGGL(k_radius_keep_count, dim3(m), dim3(256), 0, e->stream, keep, n, cnt);
    hipLaunchKernelGGL(k_compact_scan, dim3(1), dim3(1024), 0, e->stream, cnt, m);
    if (!d_out_points && !d_out_colors && !d_out_index) return 2;
    hipLaunchKernelGGL(k_radius_scatter, dim3(m), dim3(256), 0, e->stream, keep, xyz, colors, n, (const uint32_t *)cnt, (float *)d_out_points,
                       (uint8_t *)d_out_colors, (uint32_t *)d_out_index);
    return 3;
}

static int radius_compact_kept(sgm_engine *e, const char *who, const char *stage, const CloudGrid &g, const uint8_t *keep, const float *xyz,
                               const uint8_t *colors, int64_t n, void *d_out_points, void *d_out_colors, void *d_out_index, uint32_t *total)
{
    const int m = g.m;
    int rc;
    uint32_t h_ctl[RAD_CTL_WORDS] = {0, 0, 0, 0};
    uint32_t *cnt = (uint32_t *)e->ccount.p;
    hipStream_t st = e->stream;
    if ((rc = run_stage(e, stage, [&] { return launch_keep_compaction(e, m, keep, xyz, colors, n, d_out_points, d_out_colors, d_out_index); })))
        return rc;
    HIP_TRY(hipMemcpyAsync(h_ctl, e->rad_ctl.p, RAD_CTL_WORDS * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(total, cnt + m, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return h_ctl[RAD_CTL_ERR] ? cloud_no_slot(who, g) : SGM_OK;
}

int sgm_radius_outlier_device(sgm_engine *e, const void *d_xyz, const void *d_disp_f32, const void *d_colors_rgb, int64_t n, float radius,
                              const float origin[3], int nb_points, int max_count, void *d_out_keep, void *d_out_counts,
                              void *d_out_points, void *d_out_colors, void *d_out_index, int64_t *n_kept, int64_t *n_out_of_range)
{
    if (int rc = radius_check_args(e, d_xyz, d_colors_rgb, n, radius, origin, nb_points, max_count, d_out_colors, n_kept)) return rc;
    if (n == 0) return cloud_nothing(n_kept, n_out_of_range, 0), SGM_OK;
    HIP_TRY(hipSetDevice(e->device));
    const int m = (int)((n + 255) / 256);
    int rc;
    if ((rc = e->rad_ctl.ensure(RAD_CTL_WORDS * 4)) || (rc = e->rad_pt.ensure((size_t)n * 8)) || (rc = e->ccount.ensure((size_t)(m + 1) * 4)) ||
        (!d_out_keep && (rc = e->rad_keep.ensure((size_t)n))))
        return rc;
    if (e->profile) stage_reset(e);   // the stage record is the call's from here on
    const float *xyz = (const float *)d_xyz, *disp = (const float *)d_disp_f32;
    const uint8_t *colors = (const uint8_t *)(d_out_colors ? d_colors_rgb : nullptr);
    uint32_t *counts = (uint32_t *)d_out_counts;
    uint8_t *keep = (uint8_t *)(d_out_keep ? d_out_keep : e->rad_keep.p);
    hipStream_t st = e->stream;
    static const char *const names[5] = {"radius_count", "radius_clear", "radius_insert", "radius_starts", "radius_sort"};
    CloudGrid g;
    if ((rc = radius_build_grid(e, xyz, disp, n, radius, origin, keep, counts, names, &g))) return rc;
    if (g.n_in == 0) {   // nobody has a neighbour
        if (d_out_keep) HIP_TRY(hipMemsetAsync(d_out_keep, 0, (size_t)n, st));
        if (counts) HIP_TRY(hipMemsetAsync(counts, 0, (size_t)n * 4, st));
        HIP_TRY(hipStreamSynchronize(st));
        return cloud_nothing(n_kept, n_out_of_range, (int64_t)g.n_out), SGM_OK;
    }
    // 6. the counts
    rc = run_stage(e, "radius_query", [&] {
        if (e->debug & SGM_DBG_RADIUS_SOURCE_ORDER)
            hipLaunchKernelGGL(k_radius_query<false>, dim3(m), dim3(256), 0, st, (const float4 *)g.sorted, g.n_in, xyz, (const uint2 *)g.slot_rank,
                               n, g.G, g.tab, g.mask, (uint32_t)nb_points, (uint32_t)max_count, keep, counts);
        else
            hipLaunchKernelGGL(k_radius_query<true>, dim3((g.n_in + 255) / 256), dim3(256), 0, st, (const float4 *)g.sorted, g.n_in, xyz,
                               (const uint2 *)g.slot_rank, n, g.G, g.tab, g.mask, (uint32_t)nb_points, (uint32_t)max_count, keep, counts);
        return 1;
    });
    if (rc) return rc;
    // 7. the kept points through the ordered compaction
    uint32_t total = 0;
    if ((rc = radius_compact_kept(e, "sgm_radius_outlier", "radius_compact", g, keep, xyz, colors, n, d_out_points, d_out_colors, d_out_index,
                                  &total)))
        return rc;
    *n_kept = (int64_t)total;
    if (n_out_of_range) *n_out_of_range = (int64_t)g.n_out;
    return SGM_OK;
}

int sgm_radius_outlier(sgm_engine *e, const float *xyz, const float *disp, const uint8_t *colors_rgb, int64_t n, float radius,
                       const float origin[3], int nb_points, int max_count, uint8_t *out_keep, uint32_t *out_counts, float *out_points,
                       uint8_t *out_colors, uint32_t *out_index, int64_t *n_kept, int64_t *n_out_of_range)
{
    if (int rc = radius_check_args(e, xyz, colors_rgb, n, radius, origin, nb_points, max_count, out_colors, n_kept)) return rc;
    if (n == 0) return cloud_nothing(n_kept, n_out_of_range, 0), SGM_OK;
    int64_t nk = 0, noor = 0;
    const HostOut keep{out_keep, &e->rad_keep, 1, nullptr}, cnt{out_counts, &e->rad_cnt, 4, nullptr}, pts{out_points, &e->cpts, 12, &nk},
        rgb{out_colors, &e->crgb, 3, &nk}, idx{out_index, &e->rad_idx, 4, &nk};
    if (int rc = cloud_host_call(e, xyz, disp, out_colors ? colors_rgb : nullptr, n, {keep, cnt, pts, rgb, idx}, [&](void *d_disp, void *d_colors) {
            return sgm_radius_outlier_device(e, e->xyz.p, d_disp, d_colors, n, radius, origin, nb_points, max_count, keep.d(), cnt.d(), pts.d(),
                                             rgb.d(), idx.d(), &nk, &noor);
        }))
        return rc;
    *n_kept = nk;
    if (n_out_of_range) *n_out_of_range = noor;
    return SGM_OK;
}

// ---- statistical outlier removal (include/sgm_hip_statistical.h, kernels_statistical.h) ------------------------------------------
static int stat_check_args(const sgm_engine *e, const void *xyz, const void *colors, int64_t n, int k, float ratio, float r, const float *origin,
                           const void *out_colors, const int64_t *n_kept)
{
    return cloud_check_args("sgm_statistical_outlier", !e || !xyz || !n_kept, n, "max_radius", r, 524288.0f, origin, [&](int after) -> int {
        if (after == 0 && (k < 1 || k > STAT_MAX_K))
            return set_err(SGM_ERR_INVALID_ARG, "sgm_statistical_outlier: nb_neighbors %d outside 1 .. %d", k, STAT_MAX_K);
        if (after == 0 && (!std::isfinite(ratio) || !(ratio >= 0.0f)))
            return set_err(SGM_ERR_INVALID_ARG, "sgm_statistical_outlier: std_ratio %g is not finite and >= 0", (double)ratio);
        if (after == 2 && out_colors && !colors) return set_err(SGM_ERR_INVALID_ARG, "sgm_statistical_outlier: out_colors requested without colors");
        return SGM_OK;
    });
}

// step 8 of the definition: T from m, A, B in binary64, every operation on its own (the build has -ffp-contract=off)
static uint32_t stat_threshold(uint64_t m, uint64_t A, uint64_t B, float ratio)
{
    if (m == 0) return 0;
    const double mu = (double)A / (double)m;
    double var = 0.0;
    if (m >= 2) {
        const double prod = (double)A * mu;
        const double diff = (double)B - prod;
        var = diff / (double)(m - 1);
    }
    if (var < 0.0) var = 0.0;
    const double dev = (double)ratio * std::sqrt(var);
    const double thr = std::floor(mu + dev);
    return thr >= 4294967295.0 ? 4294967294u : (uint32_t)thr;
}

static void stat_nothing(int64_t *n_kept, uint64_t *out_stats, uint64_t n_out)
{
    *n_kept = 0;
    put_stats(out_stats, {0, n_out, 0, 0, 0, 0, 0, 0});
}

int sgm_statistical_outlier_device(sgm_engine *e, const void *d_xyz, const void *d_disp_f32, const void *d_colors_rgb, int64_t n,
                                   int nb_neighbors, float std_ratio, float max_radius, const float origin[3], void *d_out_keep,
                                   void *d_out_mean, void *d_out_points, void *d_out_colors, void *d_out_index, int64_t *n_kept,
                                   uint64_t *out_stats)
{
    if (int rc = stat_check_args(e, d_xyz, d_colors_rgb, n, nb_neighbors, std_ratio, max_radius, origin, d_out_colors, n_kept)) return rc;
    if (n == 0) return stat_nothing(n_kept, out_stats, 0), SGM_OK;
    HIP_TRY(hipSetDevice(e->device));
    const int m = (int)((n + 255) / 256);
    int rc;
    if ((rc = e->rad_ctl.ensure(RAD_CTL_WORDS * 4)) || (rc = e->stat_sums.ensure(STAT_SUM_WORDS * 8)) || (rc = e->rad_pt.ensure((size_t)n * 8)) ||
        (rc = e->ccount.ensure((size_t)(m + 1) * 4)) || (!d_out_keep && (rc = e->rad_keep.ensure((size_t)n))))
        return rc;
    if (e->profile) stage_reset(e);   // the stage record is the call's from here on
    const float qscale = 524288.0f / max_radius;
    const float *xyz = (const float *)d_xyz, *disp = (const float *)d_disp_f32;
    const uint8_t *colors = (const uint8_t *)(d_out_colors ? d_colors_rgb : nullptr);
    float *mean = (float *)d_out_mean;
    unsigned long long *sums = (unsigned long long *)e->stat_sums.p;
    uint8_t *keep = (uint8_t *)(d_out_keep ? d_out_keep : e->rad_keep.p);
    hipStream_t st = e->stream;
    static const char *const names[5] = {"stat_count", "stat_clear", "stat_insert", "stat_starts", "stat_sort"};
    CloudGrid g;
    if ((rc = radius_build_grid(e, xyz, disp, n, max_radius, origin, keep, nullptr, names, &g))) return rc;
    const uint32_t n_in = g.n_in, n_out = g.n_out;
    uint2 *pt = g.slot_rank;
    if (n_in == 0) {   // nobody has a neighbour
        if (d_out_keep) HIP_TRY(hipMemsetAsync(d_out_keep, 0, (size_t)n, st));
        if (mean) HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)mean, (int)0xBF800000u, (size_t)n, st));   // -1.0f
        HIP_TRY(hipStreamSynchronize(st));
        return stat_nothing(n_kept, out_stats, n_out), SGM_OK;
    }
    // 6. per point the k nearest, their mean distance and q: the list of a lane has the smallest capacity that holds k
    HIP_TRY(hipMemsetAsync(sums, 0, STAT_SUM_WORDS * 8, st));
    stage_break(e);
    rc = run_stage(e, "stat_query", [&] {
        const dim3 qgrid((n_in + 255) / 256);
        const uint32_t k = (uint32_t)nb_neighbors;
#define SGM_STAT_QUERY(CAP) \
    hipLaunchKernelGGL(k_stat_query<CAP>, qgrid, dim3(256), 0, st, (const float4 *)g.sorted, n_in, g.G, g.tab, g.mask, k, qscale, (uint32_t *)pt, mean)
        if (e->debug & SGM_DBG_STAT_WIDE_LIST) SGM_STAT_QUERY(64);
        else if (k <= 8) SGM_STAT_QUERY(8);
        else if (k <= 16) SGM_STAT_QUERY(16);
        else if (k <= 32) SGM_STAT_QUERY(32);
        else SGM_STAT_QUERY(64);
#undef SGM_STAT_QUERY
        return 1;
    });
    if (rc) return rc;
    // 7. m, A, B over the dense points; the host forms T from them
    rc = run_stage(e, "stat_reduce", [&] {
        hipLaunchKernelGGL(k_stat_reduce, dim3(std::min(m, RAD_COUNT_BLOCKS)), dim3(256), 0, st, (const uint2 *)pt, n, sums);
        return 1;
    });
    if (rc) return rc;
    unsigned long long h_sums[STAT_SUM_WORDS] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(h_sums, sums, sizeof(h_sums), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    stage_break(e);
    const uint32_t T = stat_threshold(h_sums[STAT_SUM_M], h_sums[STAT_SUM_A], h_sums[STAT_SUM_B], std_ratio);
    // 8. keep, then the kept points through the ordered compaction
    if ((rc = run_stage(e, "stat_keep", [&] { hipLaunchKernelGGL(k_stat_keep, dim3(m), dim3(256), 0, st, (const uint2 *)pt, n, T, keep, mean); return 1; })))
        return rc;
    uint32_t total = 0;
    if ((rc = radius_compact_kept(e, "sgm_statistical_outlier", "stat_compact", g, keep, xyz, colors, n, d_out_points, d_out_colors, d_out_index,
                                  &total)))
        return rc;
    *n_kept = (int64_t)total;
    put_stats(out_stats, {n_in, n_out, h_sums[STAT_SUM_M], n_in - h_sums[STAT_SUM_M], h_sums[STAT_SUM_A], h_sums[STAT_SUM_B], T, 0});
    return SGM_OK;
}

int sgm_statistical_outlier(sgm_engine *e, const float *xyz, const float *disp, const uint8_t *colors_rgb, int64_t n, int nb_neighbors,
                            float std_ratio, float max_radius, const float origin[3], uint8_t *out_keep, float *out_mean, float *out_points,
                            uint8_t *out_colors, uint32_t *out_index, int64_t *n_kept, uint64_t *out_stats)
{
    if (int rc = stat_check_args(e, xyz, colors_rgb, n, nb_neighbors, std_ratio, max_radius, origin, out_colors, n_kept)) return rc;
    if (n == 0) return stat_nothing(n_kept, out_stats, 0), SGM_OK;
    int64_t nk = 0;
    uint64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const HostOut keep{out_keep, &e->rad_keep, 1, nullptr}, mean{out_mean, &e->stat_mean, 4, nullptr}, pts{out_points, &e->cpts, 12, &nk},
        rgb{out_colors, &e->crgb, 3, &nk}, idx{out_index, &e->rad_idx, 4, &nk};
    if (int rc = cloud_host_call(e, xyz, disp, out_colors ? colors_rgb : nullptr, n, {keep, mean, pts, rgb, idx}, [&](void *d_disp, void *d_colors) {
            return sgm_statistical_outlier_device(e, e->xyz.p, d_disp, d_colors, n, nb_neighbors, std_ratio, max_radius, origin, keep.d(), mean.d(),
                                                  pts.d(), rgb.d(), idx.d(), &nk, stats);
        }))
        return rc;
    *n_kept = nk;
    if (out_stats) std::copy(stats, stats + 8, out_stats);
    return SGM_OK;
}

// ---- covariance normals of a point list (include/sgm_hip_covariance.h, kernels_covariance.h) --------------------------------------
static int cov_check_args(const sgm_engine *e, const void *xyz, int64_t n, float r, int k, const float *origin, const float *viewpoint,
                          int orient)
{
    return cloud_check_args("sgm_covariance_normals", !e || !xyz, n, "radius", r, 32768.0f, origin, [&](int after) -> int {
        if (after == 1 && (k < COV_MIN_K || (int64_t)k > RAD_MAX_POINTS))
            return set_err(SGM_ERR_INVALID_ARG, "sgm_covariance_normals: min_neighbors %d outside %d .. 2^24 - 1", k, COV_MIN_K);
        if (after == 2 && (!viewpoint || !std::isfinite(viewpoint[0]) || !std::isfinite(viewpoint[1]) || !std::isfinite(viewpoint[2])))
            return set_err(SGM_ERR_INVALID_ARG, "sgm_covariance_normals: the viewpoint is null or not finite");
        if (after == 2 && orient != 0 && orient != 1)
            return set_err(SGM_ERR_INVALID_ARG, "sgm_covariance_normals: orient %d is neither 0 nor 1", orient);
        return SGM_OK;
    });
}

static void cov_nothing(uint64_t *out_stats, uint64_t n_out) { put_stats(out_stats, {0, n_out, 0, 0}); }

int sgm_covariance_normals_device(sgm_engine *e, const void *d_xyz, const void *d_disp_f32, int64_t n, float radius, int min_neighbors,
                                  const float origin[3], const float viewpoint[3], int orient, void *d_out_normals,
                                  void *d_out_curvature, void *d_out_counts, uint64_t *out_stats)
{
    if (int rc = cov_check_args(e, d_xyz, n, radius, min_neighbors, origin, viewpoint, orient)) return rc;
    if (n == 0) return cov_nothing(out_stats, 0), SGM_OK;
    HIP_TRY(hipSetDevice(e->device));
    const int m = (int)((n + 255) / 256);
    int rc;
    if ((rc = e->rad_ctl.ensure(RAD_CTL_WORDS * 4)) || (rc = e->cov_ctl.ensure(COV_CTL_WORDS * 4)) || (rc = e->rad_pt.ensure((size_t)n * 8)) ||
        (rc = e->rad_keep.ensure((size_t)n)))
        return rc;
    if (e->profile) stage_reset(e);   // the stage record is the call's from here on
    const CovView V{32768.0f / radius, viewpoint[0], viewpoint[1], viewpoint[2], (uint32_t)min_neighbors, (uint32_t)orient};
    const float *xyz = (const float *)d_xyz, *disp = (const float *)d_disp_f32;
    float *normals = (float *)d_out_normals, *curv = (float *)d_out_curvature;
    uint32_t *counts = (uint32_t *)d_out_counts;
    uint32_t *ctl = (uint32_t *)e->cov_ctl.p;
    hipStream_t st = e->stream;
    static const char *const names[5] = {"cov_count", "cov_clear", "cov_insert", "cov_starts", "cov_sort"};
    CloudGrid g;
    // (the keep bytes k_radius_sort zeroes for the points in no cell are nobody's here: they go to the engine's own)
    if ((rc = radius_build_grid(e, xyz, disp, n, radius, origin, (uint8_t *)e->rad_keep.p, counts, names, &g))) return rc;
    const uint32_t n_in = g.n_in, n_out = g.n_out;
    if (n_in == 0) {   // nobody has a neighbour
        if (normals) HIP_TRY(hipMemsetAsync(normals, 0, (size_t)n * 12, st));
        if (curv) HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)curv, (int)0xBF800000u, (size_t)n, st));   // -1.0f
        if (counts) HIP_TRY(hipMemsetAsync(counts, 0, (size_t)n * 4, st));
        if (out_stats) HIP_TRY(hipStreamSynchronize(st));
        return cov_nothing(out_stats, n_out), SGM_OK;
    }
    const bool separate = (e->debug & SGM_DBG_COV_SEPARATE_SOLVE) != 0, select = (e->debug & SGM_DBG_COV_SELECT_ACCUM) != 0;
    if (separate && (rc = e->cov_mom.ensure((size_t)n_in * COV_WORDS * 8))) return rc;
    const float4 *sorted = g.sorted;
    long long *staged = (long long *)(separate ? e->cov_mom.p : nullptr);
    // 6. per point the moments of its neighbours and (fused) the normal; the points in no cell get their zeros and -1 first
    HIP_TRY(hipMemsetAsync(ctl, 0, COV_CTL_WORDS * 4, st));
    stage_break(e);
    const dim3 qgrid((n_in + 255) / 256);
    rc = run_stage(e, "cov_query", [&] {
        const bool fill = n_in < (uint64_t)n && (normals || curv);
        if (fill) hipLaunchKernelGGL(k_cov_fill, dim3(m), dim3(256), 0, st, (const uint2 *)g.slot_rank, n, normals, curv);
#define SGM_COV_QUERY(SEP, SEL) \
    hipLaunchKernelGGL((k_cov_query<SEP, SEL>), qgrid, dim3(256), 0, st, sorted, n_in, g.G, g.tab, g.mask, V, staged, normals, curv, counts, ctl)
        if (separate && select) SGM_COV_QUERY(true, true);
        else if (separate) SGM_COV_QUERY(true, false);
        else if (select) SGM_COV_QUERY(false, true);
        else SGM_COV_QUERY(false, false);
#undef SGM_COV_QUERY
        return fill ? 2 : 1;
    });
    if (rc) return rc;
    if (separate) {   // 7. the solve as a kernel of its own
        rc = run_stage(e, "cov_solve", [&] {
            hipLaunchKernelGGL(k_cov_solve, qgrid, dim3(256), 0, st, sorted, n_in, V, (const long long *)staged, normals, curv, counts, ctl);
            return 1;
        });
        if (rc) return rc;
    }
    if (!out_stats) return SGM_OK;
    uint32_t h_ctl[RAD_CTL_WORDS] = {0, 0, 0, 0}, h_cov[COV_CTL_WORDS] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(h_ctl, e->rad_ctl.p, sizeof(h_ctl), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h_cov, ctl, sizeof(h_cov), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (h_ctl[RAD_CTL_ERR]) return cloud_no_slot("sgm_covariance_normals", g);
    put_stats(out_stats, {n_in, n_out, h_cov[COV_CTL_NORMAL], h_cov[COV_CTL_DEGENERATE]});
    return SGM_OK;
}

int sgm_covariance_normals(sgm_engine *e, const float *xyz, const float *disp, int64_t n, float radius, int min_neighbors,
                           const float origin[3], const float viewpoint[3], int orient, float *out_normals, float *out_curvature,
                           uint32_t *out_counts, uint64_t *out_stats)
{
    if (int rc = cov_check_args(e, xyz, n, radius, min_neighbors, origin, viewpoint, orient)) return rc;
    if (n == 0) return cov_nothing(out_stats, 0), SGM_OK;
    uint64_t stats[4] = {0, 0, 0, 0};   // (always asked for: the host entry reports a full table whatever the caller wants)
    const HostOut nrm{out_normals, &e->cov_nrm, 12, nullptr}, curv{out_curvature, &e->cov_curv, 4, nullptr}, cnt{out_counts, &e->rad_cnt, 4, nullptr};
    if (int rc = cloud_host_call(e, xyz, disp, nullptr, n, {nrm, curv, cnt}, [&](void *d_disp, void *) {
            return sgm_covariance_normals_device(e, e->xyz.p, d_disp, n, radius, min_neighbors, origin, viewpoint, orient, nrm.d(), curv.d(), cnt.d(),
                                                 stats);
        }))
        return rc;
    if (out_stats) std::copy(stats, stats + 4, out_stats);
    return SGM_OK;
}

// ---- density clustering of the point cloud (include/sgm_hip_dbscan.h, kernels_dbscan.h) -------------------------------------------
static int dbscan_check_args(const sgm_engine *e, const void *xyz, int64_t n, float r, int k, const float *origin, const int64_t *n_clusters)
{
    return cloud_check_args("sgm_cluster_dbscan", !e || !xyz || !n_clusters, n, "eps", r, 0.0f, origin, [&](int after) -> int {
        if (after == 1 && (k < 1 || (int64_t)k > RAD_MAX_POINTS))
            return set_err(SGM_ERR_INVALID_ARG, "sgm_cluster_dbscan: min_points %d outside 1 .. 2^24 - 1", k);
        return SGM_OK;
    });
}

static void dbscan_nothing(int64_t *n_clusters, uint64_t *out_stats, uint64_t n_out)
{
    *n_clusters = 0;
    put_stats(out_stats, {0, n_out, 0, 0, 0, 0});
}

int sgm_cluster_dbscan_device(sgm_engine *e, const void *d_xyz, const void *d_disp_f32, int64_t n, float eps, int min_points,
                              const float origin[3], void *d_out_labels, void *d_out_core, void *d_out_sizes, uint64_t *out_stats,
                              int64_t *n_clusters)
{
    if (int rc = dbscan_check_args(e, d_xyz, n, eps, min_points, origin, n_clusters)) return rc;
    if (n == 0) return dbscan_nothing(n_clusters, out_stats, 0), SGM_OK;
    HIP_TRY(hipSetDevice(e->device));
    const int m = (int)((n + 255) / 256);
    int rc;
    if ((rc = e->rad_ctl.ensure(RAD_CTL_WORDS * 4)) || (rc = e->db_ctl.ensure(DB_CTL_WORDS * 4)) || (rc = e->rad_pt.ensure((size_t)n * 8)) ||
        (rc = e->ccount.ensure((size_t)(m + 1) * 4)) || (!d_out_core && (rc = e->rad_keep.ensure((size_t)n))) ||
        (rc = e->db_parent.ensure((size_t)n * 4)) || (rc = e->db_near.ensure((size_t)n * 4)) || (rc = e->db_rank.ensure((size_t)n * 4)))
        return rc;
    if (e->profile) stage_reset(e);   // the stage record is the call's from here on
    const float *xyz = (const float *)d_xyz, *disp = (const float *)d_disp_f32;
    uint8_t *core = (uint8_t *)(d_out_core ? d_out_core : e->rad_keep.p);
    int *labels = (int *)d_out_labels;
    uint32_t *sizes = (uint32_t *)d_out_sizes;
    hipStream_t st = e->stream;
    static const char *const names[5] = {"dbscan_count", "dbscan_clear", "dbscan_insert", "dbscan_starts", "dbscan_sort"};
    CloudGrid g;
    if ((rc = radius_build_grid(e, xyz, disp, n, eps, origin, core, nullptr, names, &g))) return rc;
    const uint32_t n_in = g.n_in, n_out = g.n_out;
    if (n_in == 0) {   // nobody has a neighbour: everything is noise
        if (labels) HIP_TRY(hipMemsetAsync(labels, 0xFF, (size_t)n * 4, st));   // -1
        if (d_out_core) HIP_TRY(hipMemsetAsync(d_out_core, 0, (size_t)n, st));
        HIP_TRY(hipStreamSynchronize(st));
        return dbscan_nothing(n_clusters, out_stats, n_out), SGM_OK;
    }
    float4 *sorted = g.sorted;
    const uint2 *slot_rank = g.slot_rank;
    int *parent = (int *)e->db_parent.p;
    uint32_t *nearest = (uint32_t *)e->db_near.p, *rank = (uint32_t *)e->db_rank.p, *ctl = (uint32_t *)e->db_ctl.p, *cnt = (uint32_t *)e->ccount.p;
    const bool gather = (e->debug & SGM_DBG_DBSCAN_GATHER_CORE) != 0;
    const dim3 qgrid((n_in + 255) / 256);
    // 5. the core points: the radius filter's count, cut short at min_points; then the core bit beside the sorted records and the
    // links set to identity
    HIP_TRY(hipMemsetAsync(ctl, 0, DB_CTL_WORDS * 4, st));
    stage_break(e);
    rc = run_stage(e, "dbscan_core", [&] {
        hipLaunchKernelGGL(k_radius_query<true>, qgrid, dim3(256), 0, st, (const float4 *)sorted, n_in, xyz, slot_rank, n, g.G, g.tab, g.mask,
                           (uint32_t)min_points, (uint32_t)min_points, core, (uint32_t *)nullptr);
        if (gather) hipLaunchKernelGGL(k_dbscan_mark<false>, qgrid, dim3(256), 0, st, sorted, n_in, (const uint8_t *)core, parent, nearest);
        else hipLaunchKernelGGL(k_dbscan_mark<true>, qgrid, dim3(256), 0, st, sorted, n_in, (const uint8_t *)core, parent, nearest);
        return 2;
    });
    if (rc) return rc;
    // 6, 7. the links between core points and each other point's nearest core point
    rc = run_stage(e, "dbscan_link", [&] {
        if (gather) hipLaunchKernelGGL(k_dbscan_link<true>, qgrid, dim3(256), 0, st, (const float4 *)sorted, n_in, g.G, g.tab, g.mask, (const uint8_t *)core, parent, nearest);
        else hipLaunchKernelGGL(k_dbscan_link<false>, qgrid, dim3(256), 0, st, (const float4 *)sorted, n_in, g.G, g.tab, g.mask, (const uint8_t *)core, parent, nearest);
        return 1;
    });
    if (rc) return rc;
    // 9. the roots in source order are the clusters in the order of their numbers
    rc = run_stage(e, "dbscan_number", [&] {
        hipLaunchKernelGGL(k_dbscan_roots, dim3(m), dim3(256), 0, st, (const uint8_t *)core, (const int *)parent, n, cnt);
        hipLaunchKernelGGL(k_compact_scan, dim3(1), dim3(1024), 0, st, cnt, m);
        hipLaunchKernelGGL(k_dbscan_rank, dim3(m), dim3(256), 0, st, (const uint8_t *)core, (const int *)parent, n, (const uint32_t *)cnt, m, rank, sizes);
        return 3;
    });
    if (rc) return rc;
    // 8, 10. labels, sizes, statistics
    rc = run_stage(e, "dbscan_label", [&] {
        hipLaunchKernelGGL(k_dbscan_label, dim3(m), dim3(256), 0, st, slot_rank, (const uint8_t *)core, parent, (const uint32_t *)nearest,
                           (const uint32_t *)rank, n, labels, sizes, ctl);
        return 1;
    });
    if (rc) return rc;
    uint32_t h_ctl[RAD_CTL_WORDS] = {0, 0, 0, 0}, h_db[DB_CTL_WORDS] = {0, 0, 0, 0}, total = 0;
    HIP_TRY(hipMemcpyAsync(h_ctl, e->rad_ctl.p, sizeof(h_ctl), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h_db, ctl, sizeof(h_db), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&total, cnt + m, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (h_ctl[RAD_CTL_ERR]) return cloud_no_slot("sgm_cluster_dbscan", g);
    *n_clusters = (int64_t)total;
    put_stats(out_stats, {n_in, n_out, h_db[DB_CTL_CORE], h_db[DB_CTL_BORDER], h_db[DB_CTL_NOISE], total});
    return SGM_OK;
}

int sgm_cluster_dbscan(sgm_engine *e, const float *xyz, const float *disp, int64_t n, float eps, int min_points, const float origin[3],
                       int32_t *out_labels, uint8_t *out_core, uint32_t *out_sizes, uint64_t *out_stats, int64_t *n_clusters)
{
    if (int rc = dbscan_check_args(e, xyz, n, eps, min_points, origin, n_clusters)) return rc;
    if (n == 0) return dbscan_nothing(n_clusters, out_stats, 0), SGM_OK;
    int64_t nc = 0;
    uint64_t stats[6] = {0, 0, 0, 0, 0, 0};
    const HostOut lab{out_labels, &e->db_lab, 4, nullptr}, core{out_core, &e->rad_keep, 1, nullptr}, sizes{out_sizes, &e->db_sizes, 4, &nc};
    if (int rc = cloud_host_call(e, xyz, disp, nullptr, n, {lab, core, sizes}, [&](void *d_disp, void *) {
            return sgm_cluster_dbscan_device(e, e->xyz.p, d_disp, n, eps, min_points, origin, lab.d(), core.d(), sizes.d(), stats, &nc);
        }))
        return rc;
    *n_clusters = nc;
    if (out_stats) std::copy(stats, stats + 6, out_stats);
    return SGM_OK;
}

// ---- plane segmentation of the point cloud (include/sgm_hip_plane.h, kernels_plane.h) ---------------------------------------------
// What both pairs of entries refuse, under the entry's name.  fit: the entry has num_iterations and refine; otherwise a model.
static int plane_check_args(const char *who, const sgm_engine *e, const void *xyz, const void *colors, const void *out_colors, int64_t n,
                            float t, bool fit, int K, int refine, int select, const float *model, const int64_t *n_inliers)
{
    if (!e || !xyz || !n_inliers) return set_err(SGM_ERR_INVALID_ARG, "%s: null pointer", who);
    if (n < 0) return set_err(SGM_ERR_INVALID_ARG, "%s: n=%lld points", who, (long long)n);
    if (!std::isfinite(t) || !(t > 0.0f) || !std::isnormal(t) || !std::isfinite(32.0f / t))
        return set_err(SGM_ERR_INVALID_ARG, "%s: distance_threshold %g is not finite, positive and normal with a finite 32 / t", who, (double)t);
    if (fit) {
        if (K < 1 || K > PLANE_MAX_K) return set_err(SGM_ERR_INVALID_ARG, "%s: num_iterations %d outside 1 .. 65536", who, K);
        if (refine != 0 && refine != 1) return set_err(SGM_ERR_INVALID_ARG, "%s: refine %d is neither 0 nor 1", who, refine);
    } else {
        if (!model) return set_err(SGM_ERR_INVALID_ARG, "%s: null pointer", who);
        const float len2 = (model[0] * model[0] + model[1] * model[1]) + model[2] * model[2];
        if (!std::isfinite(model[0]) || !std::isfinite(model[1]) || !std::isfinite(model[2]) || !std::isfinite(model[3]) ||
            !(std::fabs(len2 - 1.0f) <= 0.0009765625f))
            return set_err(SGM_ERR_INVALID_ARG, "%s: the model is not four finite numbers with a unit normal (squared length %g)", who, (double)len2);
    }
    if (select != 0 && select != 1) return set_err(SGM_ERR_INVALID_ARG, "%s: select %d is neither 0 nor 1", who, select);
    if (out_colors && !colors) return set_err(SGM_ERR_INVALID_ARG, "%s: out_colors requested without colors", who);
    if (n > RAD_MAX_POINTS) return set_err(SGM_ERR_UNSUPPORTED, "%s: %lld points, more than 2^24 - 1", who, (long long)n);
    return SGM_OK;
}

// Both device entries.  K >= 1: the whole definition; K < 0: step 8 alone with the caller's model.  Blocks once, at the end.
static int plane_run(sgm_engine *e, const float *xyz, const float *disp, const uint8_t *colors, int64_t n, float t, int K, uint32_t seed,
                     int refine, int select, const float *model, void *d_out_inlier, void *d_out_distance, void *d_out_points,
                     void *d_out_colors, void *d_out_index, float *out_model, uint64_t *out_stats, int64_t *n_inliers, int64_t *n_selected)
{
    HIP_TRY(hipSetDevice(e->device));
    const int m = (int)((n + 255) / 256);
    const bool fit = K >= 1;
    int rc;
    if ((rc = e->pl_ctl.ensure(sizeof(PlaneCtl))) || (rc = e->ccount.ensure((size_t)(m + 1) * 4)) || (rc = e->rad_keep.ensure((size_t)n)) ||
        (fit && ((rc = e->pl_pts.ensure((size_t)n * 16)) || (rc = e->pl_hyp.ensure((size_t)K * 16)) || (rc = e->pl_cnt.ensure((size_t)K * 4)))))
        return rc;
    if (e->profile) stage_reset(e);   // the stage record is the call's from here on
    hipStream_t st = e->stream;
    PlaneCtl *ctl = (PlaneCtl *)e->pl_ctl.p;
    uint32_t *cnt = (uint32_t *)e->ccount.p;
    uint8_t *keep = (uint8_t *)e->rad_keep.p;
    HIP_TRY(hipMemsetAsync(ctl, 0, sizeof(PlaneCtl), st));
    stage_break(e);
    if (fit) {
        float4 *vpts = (float4 *)e->pl_pts.p, *hyp = (float4 *)e->pl_hyp.p;
        uint32_t *hcnt = (uint32_t *)e->pl_cnt.p;
        const float qscale = 32.0f / t;
        HIP_TRY(hipMemsetAsync(hcnt, 0, (size_t)K * 4, st));
        // 1. the valid points in source order, and their number m in the control block
        rc = run_stage(e, "plane_valid", [&] {
            hipLaunchKernelGGL(k_plane_valid_count, dim3(m), dim3(256), 0, st, xyz, disp, n, cnt);
            hipLaunchKernelGGL(k_compact_scan, dim3(1), dim3(1024), 0, st, cnt, m);
            hipLaunchKernelGGL(k_plane_valid_scatter, dim3(m), dim3(256), 0, st, xyz, disp, n, (const uint32_t *)cnt, m, vpts, ctl);
            return 3;
        });
        if (rc) return rc;
        // 3, 4. the hypotheses
        rc = run_stage(e, "plane_sample", [&] {
            hipLaunchKernelGGL(k_plane_sample, dim3((K + 255) / 256), dim3(256), 0, st, (const float4 *)vpts, (uint32_t)K, seed, hyp, ctl);
            return 1;
        });
        if (rc) return rc;
        // 5. every hypothesis on every valid point: a tile of 64 hypotheses per blockIdx.y, the chunks of points strided over blockIdx.x
        const int tiles = (K + PLANE_TILE - 1) / PLANE_TILE;
        const int chunks = (int)((n + PLANE_CHUNK - 1) / PLANE_CHUNK);
        const dim3 cgrid(std::max(1, std::min(chunks, PLANE_COUNT_BLOCKS / tiles)), tiles);
        const bool mfma = ((e->debug & SGM_DBG_PLANE_OTHER_COUNT) != 0) != PLANE_DEFAULT_MFMA;
        rc = run_stage(e, "plane_count", [&] {
            if (mfma)
                hipLaunchKernelGGL(k_plane_count_mfma, cgrid, dim3(256), 0, st, (const float4 *)vpts, (const PlaneCtl *)ctl, (const float4 *)hyp,
                                   (uint32_t)K, t, hcnt);
            else
                hipLaunchKernelGGL(k_plane_count_valu, cgrid, dim3(256), 0, st, (const float4 *)vpts, (const PlaneCtl *)ctl, (const float4 *)hyp,
                                   (uint32_t)K, t, hcnt);
            return 1;
        });
        if (rc) return rc;
        // 6. the best
        rc = run_stage(e, "plane_best", [&] {
            hipLaunchKernelGGL(k_plane_best, dim3(1), dim3(1024), 0, st, (const uint32_t *)hcnt, (uint32_t)K, seed, (const float4 *)hyp,
                               (const float4 *)vpts, ctl);
            return 1;
        });
        if (rc) return rc;
        // 7. the refit
        if (refine) {
            rc = run_stage(e, "plane_moments", [&] {
                hipLaunchKernelGGL(k_plane_moments, dim3(std::min(m, PLANE_MOMENT_BLOCKS)), dim3(256), 0, st, (const float4 *)vpts, ctl, t, qscale);
                return 1;
            });
            if (rc) return rc;
            if ((rc = run_stage(e, "plane_solve", [&] { hipLaunchKernelGGL(k_plane_solve, dim3(1), dim3(64), 0, st, ctl, qscale); return 1; }))) return rc;
        }
    }
    // 8. the classification and the selected points through the ordered compaction
    const float4 given = fit ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : make_float4(model[0], model[1], model[2], model[3]);
    rc = run_stage(e, "plane_classify", [&] {
        hipLaunchKernelGGL(k_plane_classify, dim3(m), dim3(256), 0, st, xyz, disp, n, given, (const PlaneCtl *)(fit ? ctl : nullptr), t, select,
                           (uint8_t *)d_out_inlier, (float *)d_out_distance, keep, &ctl->n_inliers);
        return 1;
    });
    if (rc) return rc;
    if ((rc = run_stage(e, "plane_compact", [&] { return launch_keep_compaction(e, m, keep, xyz, colors, n, d_out_points, d_out_colors, d_out_index); })))
        return rc;
    PlaneCtl h;
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&total, cnt + m, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *n_inliers = (int64_t)h.n_inliers;
    if (n_selected) *n_selected = (int64_t)total;
    if (out_model) std::copy(h.model, h.model + 4, out_model);
    put_stats(out_stats, {h.m, h.degenerate, h.kbest, h.cbest, h.m_r, h.n_oor, h.refined, h.found});
    return SGM_OK;
}

static void plane_nothing(float *out_model, uint64_t *out_stats, int64_t *n_inliers, int64_t *n_selected)
{
    *n_inliers = 0;
    if (n_selected) *n_selected = 0;
    if (out_model) std::fill(out_model, out_model + 4, 0.0f);
    put_stats(out_stats, {0, 0, 0, 0, 0, 0, 0, 0});
}

int sgm_segment_plane_device(sgm_engine *e, const void *d_xyz, const void *d_disp_f32, const void *d_colors_rgb, int64_t n,
                             float distance_threshold, int num_iterations, uint32_t seed, int refine, int select, void *d_out_inlier,
                             void *d_out_distance, void *d_out_points, void *d_out_colors, void *d_out_index, float out_model[4],
                             uint64_t out_stats[8], int64_t *n_inliers, int64_t *n_selected)
{
    if (int rc = plane_check_args("sgm_segment_plane", e, d_xyz, d_colors_rgb, d_out_colors, n, distance_threshold, true, num_iterations,
                                  refine, select, nullptr, n_inliers))
        return rc;
    if (n == 0) return plane_nothing(out_model, out_stats, n_inliers, n_selected), SGM_OK;
    return plane_run(e, (const float *)d_xyz, (const float *)d_disp_f32, (const uint8_t *)(d_out_colors ? d_colors_rgb : nullptr), n,
                     distance_threshold, num_iterations, seed, refine, select, nullptr, d_out_inlier, d_out_distance, d_out_points, d_out_colors,
                     d_out_index, out_model, out_stats, n_inliers, n_selected);
}

int sgm_plane_inliers_device(sgm_engine *e, const void *d_xyz, const void *d_disp_f32, const void *d_colors_rgb, int64_t n,
                             const float model[4], float distance_threshold, int select, void *d_out_inlier, void *d_out_distance,
                             void *d_out_points, void *d_out_colors, void *d_out_index, int64_t *n_inliers, int64_t *n_selected)
{
    if (int rc = plane_check_args("sgm_plane_inliers", e, d_xyz, d_colors_rgb, d_out_colors, n, distance_threshold, false, 0, 0, select, model,
                                  n_inliers))
        return rc;
    if (n == 0) return plane_nothing(nullptr, nullptr, n_inliers, n_selected), SGM_OK;
    return plane_run(e, (const float *)d_xyz, (const float *)d_disp_f32, (const uint8_t *)(d_out_colors ? d_colors_rgb : nullptr), n,
                     distance_threshold, -1, 0u, 0, select, model, d_out_inlier, d_out_distance, d_out_points, d_out_colors, d_out_index, nullptr,
                     nullptr, n_inliers, n_selected);
}

// the host entries of both: the staging, the device entry `run`, the results
extern "C++" {   // (a template: this part of the file has C linkage)
template <class Run>
static int plane_host_call(sgm_engine *e, const float *xyz, const float *disp, const uint8_t *colors_rgb, int64_t n, uint8_t *out_inlier,
                           float *out_distance, float *out_points, uint8_t *out_colors, uint32_t *out_index, int64_t *n_inliers,
                           int64_t *n_selected, Run run)
{
    int64_t ni = 0, ns = 0;
    const HostOut inl{out_inlier, &e->pl_inl, 1, nullptr}, dist{out_distance, &e->pl_dist, 4, nullptr}, pts{out_points, &e->cpts, 12, &ns},
        rgb{out_colors, &e->crgb, 3, &ns}, idx{out_index, &e->rad_idx, 4, &ns};
    if (int rc = cloud_host_call(e, xyz, disp, out_colors ? colors_rgb : nullptr, n, {inl, dist, pts, rgb, idx}, [&](void *d_disp, void *d_colors) {
            return run(d_disp, d_colors, inl.d(), dist.d(), pts.d(), rgb.d(), idx.d(), &ni, &ns);
        }))
        return rc;
    *n_inliers = ni;
    if (n_selected) *n_selected = ns;
    return SGM_OK;
}
}  // extern "C++"

int sgm_segment_plane(sgm_engine *e, const float *xyz, const float *disp, const uint8_t *colors_rgb, int64_t n, float distance_threshold,
                      int num_iterations, uint32_t seed, int refine, int select, uint8_t *out_inlier, float *out_distance, float *out_points,
                      uint8_t *out_colors, uint32_t *out_index, float out_model[4], uint64_t out_stats[8], int64_t *n_inliers,
                      int64_t *n_selected)
{
    if (int rc = plane_check_args("sgm_segment_plane", e, xyz, colors_rgb, out_colors, n, distance_threshold, true, num_iterations, refine,
                                  select, nullptr, n_inliers))
        return rc;
    if (n == 0) return plane_nothing(out_model, out_stats, n_inliers, n_selected), SGM_OK;
    float model[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    uint64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (int rc = plane_host_call(e, xyz, disp, colors_rgb, n, out_inlier, out_distance, out_points, out_colors, out_index, n_inliers, n_selected,
                                 [&](void *d_disp, void *d_colors, void *d_inl, void *d_dist, void *d_pts, void *d_rgb, void *d_idx, int64_t *ni,
                                     int64_t *ns) {
                                     return sgm_segment_plane_device(e, e->xyz.p, d_disp, d_colors, n, distance_threshold, num_iterations, seed,
                                                                     refine, select, d_inl, d_dist, d_pts, d_rgb, d_idx, model, stats, ni, ns);
                                 }))
        return rc;
    if (out_model) std::copy(model, model + 4, out_model);
    if (out_stats) std::copy(stats, stats + 8, out_stats);
    return SGM_OK;
}

int sgm_plane_inliers(sgm_engine *e, const float *xyz, const float *disp, const uint8_t *colors_rgb, int64_t n, const float model[4],
                      float distance_threshold, int select, uint8_t *out_inlier, float *out_distance, float *out_points, uint8_t *out_colors,
                      uint32_t *out_index, int64_t *n_inliers, int64_t *n_selected)
{
    if (int rc = plane_check_args("sgm_plane_inliers", e, xyz, colors_rgb, out_colors, n, distance_threshold, false, 0, 0, select, model, n_inliers))
        return rc;
    if (n == 0) return plane_nothing(nullptr, nullptr, n_inliers, n_selected), SGM_OK;
    return plane_host_call(e, xyz, disp, colors_rgb, n, out_inlier, out_distance, out_points, out_colors, out_index, n_inliers, n_selected,
                           [&](void *d_disp, void *d_colors, void *d_inl, void *d_dist, void *d_pts, void *d_rgb, void *d_idx, int64_t *ni,
                               int64_t *ns) {
                               return sgm_plane_inliers_device(e, e->xyz.p, d_disp, d_colors, n, model, distance_threshold, select, d_inl, d_dist,
                                                               d_pts, d_rgb, d_idx, ni, ns);
                           });
}

// ---- rigid registration of two point clouds (include/sgm_hip_icp.h, kernels_icp.h) ------------------------------------------------
// step 6 of the definition: LDL^T without pivoting, host, binary64, fixed order (the build has -ffp-contract=off).  false: degenerate.
static bool icp_solve6(const double s[ICP_SUMS], double x[6])
{
    double A[6][6], L[6][6], D[6], v[6], y[6];
    for (int r = 0, k = 0; r < 6; r++)
        for (int q = r; q < 6; q++, k++) A[r][q] = A[q][r] = s[k];
    for (int j = 0; j < 6; j++) {
        for (int k = 0; k < j; k++) v[k] = L[j][k] * D[k];
        double dj = A[j][j];
        for (int k = 0; k < j; k++) dj = dj - L[j][k] * v[k];
        if (!(std::isfinite(dj) && dj > 0.0)) return false;
        D[j] = dj;
        for (int i = j + 1; i < 6; i++) {
            double t = A[i][j];
            for (int k = 0; k < j; k++) t = t - L[i][k] * v[k];
            L[i][j] = t / dj;
        }
    }
    for (int i = 0; i < 6; i++) {
        y[i] = s[21 + i];
        for (int k = 0; k < i; k++) y[i] = y[i] - L[i][k] * y[k];
    }
    for (int i = 0; i < 6; i++) y[i] = y[i] / D[i];
    for (int i = 5; i >= 0; i--) {
        x[i] = y[i];
        for (int k = i + 1; k < 6; k++) x[i] = x[i] - L[k][i] * x[k];
    }
    for (int i = 0; i < 6; i++)
        if (!std::isfinite(x[i])) return false;
    return true;
}

// step 7: the quaternion (1, x0 / 2, x1 / 2, x2 / 2) as a rotation with the division by its squared norm written out, then dT * T
static void icp_update(const double x[6], const double Tin[16], double Tout[16])
{
    const double qx = x[0] * 0.5, qy = x[1] * 0.5, qz = x[2] * 0.5;
    const double xx = qx * qx, yy = qy * qy, zz = qz * qz;
    const double nn = ((1.0 + xx) + yy) + zz;
    const double dT[3][4] = {{(((1.0 + xx) - yy) - zz) / nn, (2.0 * (qx * qy - qz)) / nn, (2.0 * (qx * qz + qy)) / nn, x[3]},
                             {(2.0 * (qx * qy + qz)) / nn, (((1.0 - xx) + yy) - zz) / nn, (2.0 * (qy * qz - qx)) / nn, x[4]},
                             {(2.0 * (qx * qz - qy)) / nn, (2.0 * (qy * qz + qx)) / nn, (((1.0 - xx) - yy) + zz) / nn, x[5]}};
    double out[16];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 4; j++)
            out[4 * i + j] = ((dT[i][0] * Tin[j] + dT[i][1] * Tin[4 + j]) + dT[i][2] * Tin[8 + j]) + dT[i][3] * Tin[12 + j];
    out[12] = out[13] = out[14] = 0.0, out[15] = 1.0;
    std::copy(out, out + 16, Tout);
}

int sgm_icp_solve(const double sums[28], int estimation, double T_in[16], double T_out[16], int *status)
{
    if (!sums || !T_in || !T_out || !status) return set_err(SGM_ERR_INVALID_ARG, "sgm_icp_solve: null pointer");
    if (estimation != 0 && estimation != 1) return set_err(SGM_ERR_INVALID_ARG, "sgm_icp_solve: estimation %d is neither 0 nor 1", estimation);
    double x[6];
    if (!icp_solve6(sums, x)) {
        if (T_out != T_in) std::copy(T_in, T_in + 16, T_out);
        *status = 3;
        return SGM_OK;
    }
    icp_update(x, T_in, T_out);
    *status = 0;
    return SGM_OK;
}

static int icp_check_T(const char *who, const double *T)
{
    for (int k = 0; k < 16; k++)
        if (!std::isfinite(T[k])) return set_err(SGM_ERR_INVALID_ARG, "%s: the transformation has an entry that is not finite", who);
    if (T[12] != 0.0 || T[13] != 0.0 || T[14] != 0.0 || T[15] != 1.0)
        return set_err(SGM_ERR_INVALID_ARG, "%s: the last row of the transformation is not (0, 0, 0, 1)", who);
    return SGM_OK;
}

// What the registration entries refuse, under the entry's name, before anything touches the device
static int icp_check_args(const char *who, const sgm_engine *e, const void *xyz_s, int64_t ns, const void *xyz_t, int64_t nt, float r,
                          const float *origin, const double *T, int estimation, const void *normals_t, int max_iteration, double rel_fitness,
                          double rel_rmse)
{
    if (!e || !T || (ns > 0 && !xyz_s) || (nt > 0 && !xyz_t)) return set_err(SGM_ERR_INVALID_ARG, "%s: null pointer", who);
    if (ns < 0 || nt < 0) return set_err(SGM_ERR_INVALID_ARG, "%s: ns=%lld, nt=%lld points", who, (long long)ns, (long long)nt);
    const float r2 = r * r, v = r * 1.03125f;
    if (!std::isfinite(r) || !(r > 0.0f) || !std::isnormal(r2) || !std::isfinite(1.0f / v))
        return set_err(SGM_ERR_INVALID_ARG, "%s: max_correspondence_distance %g is not finite and positive with a finite normal square", who, (double)r);
    if (!origin || !std::isfinite(origin[0]) || !std::isfinite(origin[1]) || !std::isfinite(origin[2]))
        return set_err(SGM_ERR_INVALID_ARG, "%s: the origin is null or not finite", who);
    if (int rc = icp_check_T(who, T)) return rc;
    if (estimation != 0 && estimation != 1) return set_err(SGM_ERR_INVALID_ARG, "%s: estimation %d is neither 0 nor 1", who, estimation);
    if (estimation == 1 && !normals_t) return set_err(SGM_ERR_INVALID_ARG, "%s: point-to-plane needs the target's normals", who);
    if (max_iteration < 0 || max_iteration > ICP_MAX_ITERATION)
        return set_err(SGM_ERR_INVALID_ARG, "%s: max_iteration %d outside 0 .. %d", who, max_iteration, ICP_MAX_ITERATION);
    if (!(rel_fitness >= 0.0) || !(rel_rmse >= 0.0))
        return set_err(SGM_ERR_INVALID_ARG, "%s: relative_fitness %g or relative_rmse %g is negative or not a number", who, rel_fitness, rel_rmse);
    if (ns > RAD_MAX_POINTS || nt > RAD_MAX_POINTS)
        return set_err(SGM_ERR_UNSUPPORTED, "%s: %lld and %lld points, more than 2^24 - 1", who, (long long)ns, (long long)nt);
    return SGM_OK;
}

// All four registration entries behind their checks.  Blocks once for the target grid's size and once per evaluation.
static int icp_run(sgm_engine *e, const char *who, const float *xyz_s, const float *disp_s, int64_t ns, const float *xyz_t, const float *disp_t,
                   const float *nrm_t, int64_t nt, float r, const float origin[3], const double T0[16], int estimation, int max_iteration,
                   double rel_fitness, double rel_rmse, double *out_T, double *out_fitness, double *out_rmse, void *d_out_corr, void *d_out_d2,
                   double *out_history, uint64_t *out_stats)
{
    double T[16];
    std::copy(T0, T0 + 16, T);
    std::vector<double> hist;
    uint64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 2};
    double fitness = 0.0, rmse = 0.0;
    if (ns == 0) {
        hist = {0.0, 0.0};
    } else {
        HIP_TRY(hipSetDevice(e->device));
        const int mblocks = (int)((ns + 255) / 256);
        int64_t npad = 1;
        while (npad < ns) npad <<= 1;
        uint32_t npow = 1;
        while (npow < (uint32_t)mblocks) npow <<= 1;
        const size_t pin_bytes = sizeof(IcpResult) + sizeof(IcpCtl) + RAD_CTL_WORDS * 4;
        int rc;
        if ((rc = e->rad_ctl.ensure(RAD_CTL_WORDS * 4)) || (rc = e->icp_ctl.ensure(sizeof(IcpResult) + sizeof(IcpCtl))) ||
            (rc = e->icp_part.ensure((size_t)mblocks * ICP_SUMS * 8)) || (rc = e->pin_icp.ensure(pin_bytes)) ||
            (nt > 0 && ((rc = e->rad_pt.ensure((size_t)nt * 8)) || (rc = e->rad_keep.ensure((size_t)nt)))) ||
            (!d_out_corr && (rc = e->icp_corr.ensure((size_t)ns * 4))) || (!d_out_d2 && (rc = e->icp_d2.ensure((size_t)ns * 4))))
            return rc;
        if (e->profile) stage_reset(e);   // the stage record is the call's from here on
        hipStream_t st = e->stream;
        IcpResult *d_res = (IcpResult *)e->icp_ctl.p;
        IcpCtl *d_ctl = (IcpCtl *)((char *)e->icp_ctl.p + sizeof(IcpResult));
        const IcpResult *h_res = (const IcpResult *)e->pin_icp.p;
        const IcpCtl *h_ctl = (const IcpCtl *)((const char *)e->pin_icp.p + sizeof(IcpResult));
        const uint32_t *h_rad = (const uint32_t *)((const char *)e->pin_icp.p + sizeof(IcpResult) + sizeof(IcpCtl));
        int32_t *corr = (int32_t *)(d_out_corr ? d_out_corr : e->icp_corr.p);
        float *d2 = (float *)(d_out_d2 ? d_out_d2 : e->icp_d2.p);
        double *part = (double *)e->icp_part.p;
        // 1. the target's grid: radius_build_grid, unchanged, under stage names of this call
        static const char *const names[5] = {"icp_count", "icp_clear", "icp_insert", "icp_starts", "icp_sort"};
        CloudGrid g{RadGrid{1.0f / (r * 1.03125f), r * r, origin[0], origin[1], origin[2]}, 0, 0, 0, 0, nullptr, nullptr, nullptr, 0};
        if (nt > 0) {
            if ((rc = radius_build_grid(e, xyz_t, disp_t, nt, r, origin, (uint8_t *)e->rad_keep.p, nullptr, names, &g))) return rc;
        } else {
            HIP_TRY(hipMemsetAsync(e->rad_ctl.p, 0, RAD_CTL_WORDS * 4, st));
        }
        const int grid_stages = e->nstages, grid_events = e->nevents;
        // 2 to 5. one evaluation under T: the counts zeroed, the three kernels, the record and the counts read back, one wait
        auto evaluate = [&]() -> int {
            IcpM M;
            for (int k = 0; k < 12; k++) M.m[k] = (float)T[k];
            if (e->profile) e->nstages = grid_stages, e->nevents = grid_events;   // the record keeps the grid's stages and the last evaluation's
            HIP_TRY(hipMemsetAsync(d_ctl, 0, sizeof(IcpCtl), st));
            stage_break(e);
            int rc2;
            rc2 = run_stage(e, "icp_correspond", [&] {
                hipLaunchKernelGGL(k_icp_correspond, dim3(mblocks), dim3(256), 0, st, xyz_s, disp_s, ns, M, (const float4 *)g.sorted, g.tab, g.mask,
                                   g.G, corr, d2, d_ctl);
                return 1;
            });
            if (rc2) return rc2;
            rc2 = run_stage(e, "icp_terms", [&] {
                hipLaunchKernelGGL(k_icp_terms, dim3(mblocks), dim3(256), 0, st, xyz_s, ns, npad, M, xyz_t, nrm_t, estimation, (const int32_t *)corr,
                                   (const float *)d2, part, d_ctl);
                return 1;
            });
            if (rc2) return rc2;
            rc2 = run_stage(e, "icp_reduce", [&] {
                hipLaunchKernelGGL(k_icp_reduce, dim3(1), dim3(ICP_REDUCE_CHUNK), 0, st, (const double *)part, (uint32_t)mblocks, npow,
                                   (const IcpCtl *)d_ctl, d_res);
                return 1;
            });
            if (rc2) return rc2;
            // ONE copy: the 232-byte record and, adjacent to it in icp_ctl, the evaluation's 16 bytes of counts
            HIP_TRY(hipMemcpyAsync(e->pin_icp.p, d_res, sizeof(IcpResult) + sizeof(IcpCtl), hipMemcpyDeviceToHost, st));
            if (hist.empty())   // the grid's control words once, in the first wait: only k_radius_insert sets RAD_CTL_ERR, no walk does
                HIP_TRY(hipMemcpyAsync((char *)e->pin_icp.p + sizeof(IcpResult) + sizeof(IcpCtl), e->rad_ctl.p, RAD_CTL_WORDS * 4,
                                       hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (hist.empty() && h_rad[RAD_CTL_ERR]) return cloud_no_slot(who, g);
            const uint32_t nc = h_res->n_corr, ms = h_ctl->m_s;
            fitness = ms ? (double)nc / (double)ms : 0.0;
            rmse = nc ? std::sqrt(h_res->sums[27] / (double)nc) : 0.0;
            hist.push_back(fitness), hist.push_back(rmse);
            return SGM_OK;
        };
        if ((rc = evaluate())) return rc;
        int iterations = 0, status;
        for (;;) {
            if (h_res->n_corr < 6u) { status = 2; break; }
            if (iterations == max_iteration) { status = 1; break; }
            double x[6];
            if (!icp_solve6(h_res->sums, x)) { status = 3; break; }
            icp_update(x, T, T);
            const double f0 = fitness, r0 = rmse;
            if ((rc = evaluate())) return rc;
            iterations++;
            if (std::fabs(fitness - f0) < rel_fitness && std::fabs(rmse - r0) < rel_rmse) { status = 0; break; }
        }
        put_stats(stats, {h_ctl->m_s, g.n_in, g.n_out, (uint64_t)iterations, h_res->n_corr, h_ctl->unplaced, h_ctl->unusable, (uint64_t)status});
    }
    if (out_T) std::copy(T, T + 16, out_T);
    if (out_fitness) *out_fitness = fitness;
    if (out_rmse) *out_rmse = rmse;
    if (out_history) std::copy(hist.begin(), hist.end(), out_history);
    if (out_stats) std::copy(stats, stats + 8, out_stats);
    return SGM_OK;
}

int sgm_register_icp_device(sgm_engine *e, const void *d_xyz_s, const void *d_disp_s, int64_t ns, const void *d_xyz_t, const void *d_disp_t,
                            const void *d_normals_t, int64_t nt, float max_correspondence_distance, const float origin[3],
                            const double T0[16], int estimation, int max_iteration, double relative_fitness, double relative_rmse,
                            double out_T[16], double *out_fitness, double *out_rmse, void *d_out_corr, void *d_out_d2,
                            double *out_history, uint64_t out_stats[8])
{
    const char *who = "sgm_register_icp";
    if (int rc = icp_check_args(who, e, d_xyz_s, ns, d_xyz_t, nt, max_correspondence_distance, origin, T0, estimation, d_normals_t, max_iteration,
                                relative_fitness, relative_rmse))
        return rc;
    return icp_run(e, who, (const float *)d_xyz_s, (const float *)d_disp_s, ns, (const float *)d_xyz_t, (const float *)d_disp_t,
                   (const float *)d_normals_t, nt, max_correspondence_distance, origin, T0, estimation, max_iteration, relative_fitness,
                   relative_rmse, out_T, out_fitness, out_rmse, d_out_corr, d_out_d2, out_history, out_stats);
}

int sgm_evaluate_registration_device(sgm_engine *e, const void *d_xyz_s, const void *d_disp_s, int64_t ns, const void *d_xyz_t,
                                     const void *d_disp_t, int64_t nt, float max_correspondence_distance, const float origin[3],
                                     const double T[16], double *out_fitness, double *out_rmse, void *d_out_corr, void *d_out_d2,
                                     uint64_t out_stats[8])
{
    const char *who = "sgm_evaluate_registration";
    if (int rc = icp_check_args(who, e, d_xyz_s, ns, d_xyz_t, nt, max_correspondence_distance, origin, T, 0, nullptr, 0, 0.0, 0.0)) return rc;
    return icp_run(e, who, (const float *)d_xyz_s, (const float *)d_disp_s, ns, (const float *)d_xyz_t, (const float *)d_disp_t, nullptr, nt,
                   max_correspondence_distance, origin, T, 0, 0, 0.0, 0.0, nullptr, out_fitness, out_rmse, d_out_corr, d_out_d2, nullptr, out_stats);
}

// The host entries of both: the two clouds up (the source to xyz and f32, the target to icp_txyz, icp_tdisp, icp_tnrm), icp_run on
// them, corr and d2 down.  An empty cloud is not staged (no target: no pair ever reads a normal); with no source nothing runs.
static int icp_run_host(sgm_engine *e, const char *who, const float *xyz_s, const float *disp_s, int64_t ns, const float *xyz_t,
                        const float *disp_t, const float *normals_t, int64_t nt, float r, const float origin[3], const double T0[16],
                        int estimation, int max_iteration, double rel_fitness, double rel_rmse, double *out_T, double *out_fitness,
                        double *out_rmse, int32_t *out_corr, float *out_d2, double *out_history, uint64_t *out_stats)
{
    if (ns == 0)
        return icp_run(e, who, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nt, r, origin, T0, estimation, max_iteration, rel_fitness,
                       rel_rmse, out_T, out_fitness, out_rmse, nullptr, nullptr, out_history, out_stats);
    const HostIn s{xyz_s, &e->xyz, (size_t)ns * 12}, ds{disp_s, &e->f32, (size_t)ns * 4}, t{xyz_t, &e->icp_txyz, (size_t)nt * 12},
        dt{disp_t, &e->icp_tdisp, (size_t)nt * 4}, nrm{normals_t, &e->icp_tnrm, (size_t)nt * 12};
    const HostOut corr{out_corr, &e->icp_corr, 4, nullptr}, d2{out_d2, &e->icp_d2, 4, nullptr};
    return host_call(e, ns, {s, ds, t, dt, nrm}, {corr, d2}, [&] {
        return icp_run(e, who, (const float *)s.d(), (const float *)ds.d(), ns, (const float *)t.d(), (const float *)dt.d(),
                       (const float *)nrm.d(), nt, r, origin, T0, estimation, max_iteration, rel_fitness, rel_rmse, out_T, out_fitness, out_rmse,
                       corr.d(), d2.d(), out_history, out_stats);
    });
}

int sgm_register_icp(sgm_engine *e, const float *xyz_s, const float *disp_s, int64_t ns, const float *xyz_t, const float *disp_t,
                     const float *normals_t, int64_t nt, float max_correspondence_distance, const float origin[3], const double T0[16],
                     int estimation, int max_iteration, double relative_fitness, double relative_rmse, double out_T[16],
                     double *out_fitness, double *out_rmse, int32_t *out_corr, float *out_d2, double *out_history, uint64_t out_stats[8])
{
    const char *who = "sgm_register_icp";
    if (int rc = icp_check_args(who, e, xyz_s, ns, xyz_t, nt, max_correspondence_distance, origin, T0, estimation, normals_t, max_iteration,
                                relative_fitness, relative_rmse))
        return rc;
    return icp_run_host(e, who, xyz_s, disp_s, ns, xyz_t, disp_t, normals_t, nt, max_correspondence_distance, origin, T0, estimation,
                        max_iteration, relative_fitness, relative_rmse, out_T, out_fitness, out_rmse, out_corr, out_d2, out_history, out_stats);
}

int sgm_evaluate_registration(sgm_engine *e, const float *xyz_s, const float *disp_s, int64_t ns, const float *xyz_t, const float *disp_t,
                              int64_t nt, float max_correspondence_distance, const float origin[3], const double T[16],
                              double *out_fitness, double *out_rmse, int32_t *out_corr, float *out_d2, uint64_t out_stats[8])
{
    const char *who = "sgm_evaluate_registration";
    if (int rc = icp_check_args(who, e, xyz_s, ns, xyz_t, nt, max_correspondence_distance, origin, T, 0, nullptr, 0, 0.0, 0.0)) return rc;
    return icp_run_host(e, who, xyz_s, disp_s, ns, xyz_t, disp_t, nullptr, nt, max_correspondence_distance, origin, T, 0, 0, 0.0, 0.0, nullptr,
                        out_fitness, out_rmse, out_corr, out_d2, nullptr, out_stats);
}

static int icp_transform_check(const sgm_engine *e, const void *xyz, const void *normals, int64_t n, const double *T, const void *out_xyz,
                               const void *out_normals)
{
    const char *who = "sgm_transform_points";
    if (!e || !T || (n > 0 && !xyz)) return set_err(SGM_ERR_INVALID_ARG, "%s: null pointer", who);
    if (n < 0) return set_err(SGM_ERR_INVALID_ARG, "%s: n=%lld points", who, (long long)n);
    if ((normals == nullptr) != (out_normals == nullptr))
        return set_err(SGM_ERR_INVALID_ARG, "%s: normals and out_normals are not both null or both given", who);
    if (!out_xyz && !out_normals) return set_err(SGM_ERR_INVALID_ARG, "%s: no output", who);
    if (int rc = icp_check_T(who, T)) return rc;
    if (n > RAD_MAX_POINTS) return set_err(SGM_ERR_UNSUPPORTED, "%s: %lld points, more than 2^24 - 1", who, (long long)n);
    return SGM_OK;
}

int sgm_transform_points_device(sgm_engine *e, const void *d_xyz, const void *d_normals, int64_t n, const double T[16], void *d_out_xyz,
                                void *d_out_normals)
{
    if (int rc = icp_transform_check(e, d_xyz, d_normals, n, T, d_out_xyz, d_out_normals)) return rc;
    if (n == 0) return SGM_OK;
    HIP_TRY(hipSetDevice(e->device));
    IcpM M;
    for (int k = 0; k < 12; k++) M.m[k] = (float)T[k];
    hipLaunchKernelGGL(k_icp_transform, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e->stream, (const float *)d_xyz, (const float *)d_normals,
                       n, M, (float *)d_out_xyz, (float *)d_out_normals);
    KCHECK();
    return SGM_OK;
}

int sgm_transform_points(sgm_engine *e, const float *xyz, const float *normals, int64_t n, const double T[16], float *out_xyz,
                         float *out_normals)
{
    if (int rc = icp_transform_check(e, xyz, normals, n, T, out_xyz, out_normals)) return rc;
    if (n == 0) return SGM_OK;
    // in place: an output comes down from the buffer its input went up to
    const HostIn pts{xyz, &e->xyz, (size_t)n * 12}, nrm{normals, &e->icp_tnrm, (size_t)n * 12};
    const HostOut opts{out_xyz, &e->xyz, 12, nullptr}, onrm{out_normals, &e->icp_tnrm, 12, nullptr};
    return host_call(e, n, {pts, nrm}, {opts, onrm}, [&] { return sgm_transform_points_device(e, pts.d(), nrm.d(), n, T, opts.d(), onrm.d()); });
}

// ---- the truncated signed distance volume (include/sgm_hip_tsdf.h, kernels_tsdf.h) -------------------------------------------------
// What every entry of the header refuses about the volume, under the entry's name, before anything touches the device.  *V: nx ny nz.
static int tsdf_check_volume(const char *who, const sgm_engine *e, const int32_t *dims, float vs, const float *origin, const void *sum,
                             const void *weight, TsdfVol *vol, int64_t *V)
{
    if (!e || !dims || !origin || !sum || !weight) return set_err(SGM_ERR_INVALID_ARG, "%s: null pointer", who);
    if (!std::isfinite(vs) || !(vs > 0.0f)) return set_err(SGM_ERR_INVALID_ARG, "%s: voxel_size %g is not finite and positive", who, (double)vs);
    if (!std::isfinite(origin[0]) || !std::isfinite(origin[1]) || !std::isfinite(origin[2]))
        return set_err(SGM_ERR_INVALID_ARG, "%s: the origin is not finite", who);
    for (int a = 0; a < 3; a++)
        if (dims[a] < 1 || dims[a] > TSDF_MAX_DIM)
            return set_err(SGM_ERR_UNSUPPORTED, "%s: dimension %d outside 1 .. %d", who, (int)dims[a], TSDF_MAX_DIM);
    *V = (int64_t)dims[0] * dims[1] * dims[2];
    if (*V > TSDF_MAX_VOXELS) return set_err(SGM_ERR_UNSUPPORTED, "%s: %lld voxels, more than 2^30", who, (long long)*V);
    *vol = TsdfVol{dims[0], dims[1], dims[2], vs, origin[0], origin[1], origin[2]};
    return SGM_OK;
}

// ... and about the frame of an integration
static int tsdf_check_frame(const char *who, float tau, const void *rgb_sum, const void *xyz, const void *colors, int H, int W, const float *cam,
                            int front, const double *extrinsic, float max_depth, TsdfFrame *fr)
{
    if (!xyz || !cam || !extrinsic) return set_err(SGM_ERR_INVALID_ARG, "%s: null pointer", who);
    if ((rgb_sum == nullptr) != (colors == nullptr))
        return set_err(SGM_ERR_INVALID_ARG, "%s: rgb_sum and colors are not both null or both given", who);
    if (front != 1 && front != -1) return set_err(SGM_ERR_INVALID_ARG, "%s: front %d is neither +1 nor -1", who, front);
    for (int k = 0; k < 4; k++)
        if (!std::isfinite(cam[k])) return set_err(SGM_ERR_INVALID_ARG, "%s: the camera (fx, fy, cx, cy) has an entry that is not finite", who);
    const float kappa = 32767.0f / tau;
    if (!std::isfinite(tau) || !(tau > 0.0f) || !std::isfinite(kappa))
        return set_err(SGM_ERR_INVALID_ARG, "%s: sdf_trunc %g is not finite and positive with a finite 32767 / sdf_trunc", who, (double)tau);
    if (int rc = icp_check_T(who, extrinsic)) return rc;
    if (!(max_depth > 0.0f)) return set_err(SGM_ERR_INVALID_ARG, "%s: max_depth %g is not > 0", who, (double)max_depth);
    if (H < 1 || W < 1) return set_err(SGM_ERR_INVALID_ARG, "%s: a frame of %d x %d", who, H, W);
    if ((int64_t)H * W > TSDF_MAX_PIXELS) return set_err(SGM_ERR_UNSUPPORTED, "%s: %d x %d pixels, more than 2^27", who, H, W);
    for (int k = 0; k < 12; k++) fr->m[k] = (float)extrinsic[k];
    fr->fx = cam[0], fr->fy = cam[1], fr->cx = cam[2], fr->cy = cam[3];
    fr->front = (float)front, fr->max_depth = max_depth, fr->tau = tau, fr->kappa = kappa;
    fr->H = H, fr->W = W;
    return SGM_OK;
}

// the integration behind its checks: the stage, and the counts if they are asked for (the only wait)
static int tsdf_integrate_run(sgm_engine *e, const TsdfVol &vol, int64_t V, const TsdfFrame &fr, void *d_sum, void *d_weight, void *d_rgb,
                              const void *d_xyz, const void *d_disp, const void *d_colors, uint64_t *out_stats)
{
    HIP_TRY(hipSetDevice(e->device));
    int rc;
    constexpr size_t ctl_bytes = (size_t)TSDF_STAT_SLOTS * 64;
    if (out_stats && (rc = e->tsdf_ctl.ensure(ctl_bytes))) return rc;
    if (e->profile) stage_reset(e);   // the stage record is the call's from here on
    hipStream_t st = e->stream;
    unsigned long long *d_stats = out_stats ? (unsigned long long *)e->tsdf_ctl.p : nullptr;
    if (d_stats) HIP_TRY(hipMemsetAsync(d_stats, 0, ctl_bytes, st));
    const uint32_t xchunks = (uint32_t)((vol.nx + 63) / 64), rows = (uint32_t)vol.ny * (uint32_t)vol.nz;
    const uint32_t blocks = xchunks * ((rows + 3u) / 4u);
    const int64_t npix = (int64_t)fr.H * fr.W;
    rc = run_stage(e, "tsdf_integrate", [&] {
        if (!d_stats) {
            hipLaunchKernelGGL(k_tsdf_integrate<false>, dim3(blocks), dim3(256), 0, st, vol, fr, xchunks, rows, V, (int32_t *)d_sum,
                               (int32_t *)d_weight, (uint32_t *)d_rgb, (const float *)d_xyz, (const float *)d_disp, (const uint8_t *)d_colors,
                               d_stats);
            return 1;
        }
        hipLaunchKernelGGL(k_tsdf_integrate<true>, dim3(blocks), dim3(256), 0, st, vol, fr, xchunks, rows, V, (int32_t *)d_sum, (int32_t *)d_weight,
                           (uint32_t *)d_rgb, (const float *)d_xyz, (const float *)d_disp, (const uint8_t *)d_colors, d_stats);
        hipLaunchKernelGGL(k_tsdf_usable, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, (const float *)d_xyz, (const float *)d_disp,
                           npix, fr.front, fr.max_depth, d_stats);
        return 2;
    });
    if (rc) return rc;
    if (out_stats) {
        std::vector<uint64_t> h((size_t)TSDF_STAT_SLOTS * 8);      // the 256 copies of the record, added up here
        HIP_TRY(hipMemcpyAsync(h.data(), d_stats, ctl_bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        std::fill(out_stats, out_stats + 8, (uint64_t)0);
        for (size_t k = 0; k < h.size(); k++) out_stats[k & 7] += h[k];
    }
    return SGM_OK;
}

int sgm_tsdf_integrate_device(sgm_engine *e, const int32_t dims[3], float voxel_size, float sdf_trunc, const float origin[3], void *d_sum,
                              void *d_weight, void *d_rgb_sum, const void *d_xyz, const void *d_disp, const void *d_colors_rgb, int H, int W,
                              const float cam[4], int front, const double extrinsic[16], float max_depth, uint64_t out_stats[8])
{
    const char *who = "sgm_tsdf_integrate_device";
    TsdfVol vol;
    TsdfFrame fr;
    int64_t V = 0;
    if (int rc = tsdf_check_volume(who, e, dims, voxel_size, origin, d_sum, d_weight, &vol, &V)) return rc;
    if (int rc = tsdf_check_frame(who, sdf_trunc, d_rgb_sum, d_xyz, d_colors_rgb, H, W, cam, front, extrinsic, max_depth, &fr)) return rc;
    return tsdf_integrate_run(e, vol, V, fr, d_sum, d_weight, d_rgb_sum, d_xyz, d_disp, d_colors_rgb, out_stats);
}

int sgm_tsdf_integrate(sgm_engine *e, const int32_t dims[3], float voxel_size, float sdf_trunc, const float origin[3], int32_t *sum,
                       int32_t *weight, uint32_t *rgb_sum, const float *xyz, const float *disp, const uint8_t *colors_rgb, int H, int W,
                       const float cam[4], int front, const double extrinsic[16], float max_depth, uint64_t out_stats[8])
{
    const char *who = "sgm_tsdf_integrate";
    TsdfVol vol;
    TsdfFrame fr;
    int64_t V = 0;
    if (int rc = tsdf_check_volume(who, e, dims, voxel_size, origin, sum, weight, &vol, &V)) return rc;
    if (int rc = tsdf_check_frame(who, sdf_trunc, rgb_sum, xyz, colors_rgb, H, W, cam, front, extrinsic, max_depth, &fr)) return rc;
    const size_t npix = (size_t)H * W;
    // in place: a plane comes down from the buffer it went up to
    const HostIn s{sum, &e->tsdf_sum, (size_t)V * 4}, w{weight, &e->tsdf_w, (size_t)V * 4}, c{rgb_sum, &e->tsdf_rgb, (size_t)V * 12},
        pts{xyz, &e->xyz, npix * 12}, dsp{disp, &e->f32, npix * 4}, rgb{colors_rgb, &e->crgb_in, npix * 3};
    const HostOut os{sum, &e->tsdf_sum, 4, nullptr}, ow{weight, &e->tsdf_w, 4, nullptr}, oc{rgb_sum, &e->tsdf_rgb, 12, nullptr};
    uint64_t stats[8];
    if (int rc = host_call(e, V, {s, w, c, pts, dsp, rgb}, {os, ow, oc}, [&] {
            return tsdf_integrate_run(e, vol, V, fr, s.d(), w.d(), c.d(), pts.d(), dsp.d(), rgb.d(), out_stats ? stats : nullptr);
        }))
        return rc;
    if (out_stats) std::copy(stats, stats + 8, out_stats);
    return SGM_OK;
}

// What the extraction refuses beside the volume
static int tsdf_check_extract(const char *who, const void *rgb_sum, int min_weight, int64_t capacity, const void *out_points, const void *out_colors,
                              const int64_t *out_total)
{
    if (!out_total) return set_err(SGM_ERR_INVALID_ARG, "%s: null pointer", who);
    if (min_weight < 1) return set_err(SGM_ERR_INVALID_ARG, "%s: min_weight %d is not >= 1", who, min_weight);
    if (capacity < 0) return set_err(SGM_ERR_INVALID_ARG, "%s: a capacity of %lld rows", who, (long long)capacity);
    if (out_colors && !rgb_sum) return set_err(SGM_ERR_INVALID_ARG, "%s: out_colors requested without rgb_sum", who);
    if (out_colors && !out_points) return set_err(SGM_ERR_INVALID_ARG, "%s: out_colors requested without out_points", who);
    return SGM_OK;
}

// the extraction behind its checks: count, scan, emit (unless the call only counts), then ONE wait for the total
static int tsdf_extract_run(sgm_engine *e, const TsdfVol &vol, int64_t V, const void *d_sum, const void *d_weight, const void *d_rgb,
                            int min_weight, int64_t capacity, void *d_out_points, void *d_out_colors, int64_t *out_total)
{
    HIP_TRY(hipSetDevice(e->device));
    const int m = (int)((V + TSDF_BLOCK_VOXELS - 1) / TSDF_BLOCK_VOXELS);
    int rc;
    if ((rc = e->tsdf_cnt.ensure((size_t)m * 4)) || (rc = e->tsdf_off.ensure((size_t)(m + 1) * 8))) return rc;
    if (e->profile) stage_reset(e);   // the stage record is the call's from here on
    hipStream_t st = e->stream;
    uint32_t *cnt = (uint32_t *)e->tsdf_cnt.p;
    unsigned long long *off = (unsigned long long *)e->tsdf_off.p;
    rc = run_stage(e, "tsdf_count", [&] {
        hipLaunchKernelGGL(k_tsdf_count, dim3(m), dim3(256), 0, st, vol, V, (const int32_t *)d_sum, (const int32_t *)d_weight, min_weight, cnt);
        return 1;
    });
    if (rc) return rc;
    rc = run_stage(e, "tsdf_scan", [&] {
        hipLaunchKernelGGL(k_tsdf_scan, dim3(1), dim3(1024), 0, st, (const uint32_t *)cnt, m, off);
        return 1;
    });
    if (rc) return rc;
    if (d_out_points && capacity > 0) {
        rc = run_stage(e, "tsdf_emit", [&] {
            hipLaunchKernelGGL(k_tsdf_emit, dim3(m), dim3(256), 0, st, vol, V, (const int32_t *)d_sum, (const int32_t *)d_weight,
                               (const uint32_t *)d_rgb, min_weight, (const unsigned long long *)off, capacity, (float *)d_out_points,
                               (uint8_t *)d_out_colors);
            return 1;
        });
        if (rc) return rc;
    }
    unsigned long long total = 0;
    HIP_TRY(hipMemcpyAsync(&total, off + m, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *out_total = (int64_t)total;
    return SGM_OK;
}

int sgm_tsdf_extract_points_device(sgm_engine *e, const int32_t dims[3], float voxel_size, const float origin[3], const void *d_sum,
                                   const void *d_weight, const void *d_rgb_sum, int min_weight, int64_t capacity, void *d_out_points,
                                   void *d_out_colors, int64_t *out_total)
{
    const char *who = "sgm_tsdf_extract_points_device";
    TsdfVol vol;
    int64_t V = 0;
    if (int rc = tsdf_check_volume(who, e, dims, voxel_size, origin, d_sum, d_weight, &vol, &V)) return rc;
    if (int rc = tsdf_check_extract(who, d_rgb_sum, min_weight, capacity, d_out_points, d_out_colors, out_total)) return rc;
    return tsdf_extract_run(e, vol, V, d_sum, d_weight, d_rgb_sum, min_weight, capacity, d_out_points, d_out_colors, out_total);
}

int sgm_tsdf_extract_points(sgm_engine *e, const int32_t dims[3], float voxel_size, const float origin[3], const int32_t *sum,
                            const int32_t *weight, const uint32_t *rgb_sum, int min_weight, int64_t capacity, float *out_points,
                            uint8_t *out_colors, int64_t *out_total)
{
    const char *who = "sgm_tsdf_extract_points";
    TsdfVol vol;
    int64_t V = 0;
    if (int rc = tsdf_check_volume(who, e, dims, voxel_size, origin, sum, weight, &vol, &V)) return rc;
    if (int rc = tsdf_check_extract(who, rgb_sum, min_weight, capacity, out_points, out_colors, out_total)) return rc;
    // the colour sums go up only if colours are asked for; the rows that come down are the written ones
    const HostIn s{sum, &e->tsdf_sum, (size_t)V * 4}, w{weight, &e->tsdf_w, (size_t)V * 4}, c{out_colors ? rgb_sum : nullptr, &e->tsdf_rgb, (size_t)V * 12};
    int64_t total = 0, rows = 0;
    const HostOut pts{capacity > 0 ? out_points : nullptr, &e->cpts, 12, &rows, capacity},
        rgb{capacity > 0 ? out_colors : nullptr, &e->crgb, 3, &rows, capacity};
    if (int rc = host_call(e, V, {s, w, c}, {pts, rgb}, [&] {
            const int rc2 = tsdf_extract_run(e, vol, V, s.d(), w.d(), c.d(), min_weight, capacity, pts.d(), rgb.d(), &total);
            rows = std::min(total, capacity);
            return rc2;
        }))
        return rc;
    *out_total = total;
    return SGM_OK;
}

// ---- triangle mesh from the organised cloud (include/sgm_hip_mesh.h, kernels_mesh.h) and its normals (include/sgm_hip_normals.h,
// kernels_normals.h) -----------------------------------------------------------------------------------------------------------------
// What every entry of the two headers refuses, under the entry's name.  null: one of its required pointers is.
static int mesh_check_args(const char *who, bool null, int H, int W, float max_diff, int orient, bool out_colors_without_colors)
{
    if (null) return set_err(SGM_ERR_INVALID_ARG, "%s: null pointer", who);
    if (H < 1 || W < 1) return set_err(SGM_ERR_INVALID_ARG, "%s: a frame of %d x %d pixels", who, H, W);
    if (!std::isfinite(max_diff) || !(max_diff >= 0.0f))
        return set_err(SGM_ERR_INVALID_ARG, "%s: max_diff %g is not finite and >= 0", who, (double)max_diff);
    if (orient != 0 && orient != 1) return set_err(SGM_ERR_INVALID_ARG, "%s: orient %d is not 0 or 1", who, orient);
    if (out_colors_without_colors) return set_err(SGM_ERR_INVALID_ARG, "%s: out_colors requested without colors", who);
    if ((int64_t)H * W > MESH_MAX_PIXELS) return set_err(SGM_ERR_UNSUPPORTED, "%s: %d x %d pixels, more than 2^26", who, H, W);
    return SGM_OK;
}

// steps 1 - 3: every quad's code and the blocks' numbers of triangles, into the engine's mesh_code and mesh_fcnt (m blocks)
static int mesh_stage_quads(sgm_engine *e, const float *xyz, const float *disp, int H, int W, float max_diff, int m)
{
    uint8_t *code = (uint8_t *)e->mesh_code.p;
    uint32_t *fcnt = (uint32_t *)e->mesh_fcnt.p;
    hipStream_t st = e->stream;
    return run_stage(e, "mesh_quads", [&] {
        // (16-byte loads where every group of four pixels, and the four below it, starts on a 16-byte boundary)
        const bool wide = W % 4 == 0 && (uintptr_t)xyz % 16 == 0 && (uintptr_t)disp % 16 == 0;
        if (wide) hipLaunchKernelGGL(k_mesh_quads<true>, dim3(m), dim3(MESH_BLOCK / 4), 0, st, xyz, disp, H, W, max_diff, code, fcnt);
        else hipLaunchKernelGGL(k_mesh_quads<false>, dim3(m), dim3(MESH_BLOCK / 4), 0, st, xyz, disp, H, W, max_diff, code, fcnt);
        return 1;
    });
}

// The mesh on the engine's stream from device pointers, for sgm_mesh_grid_device and sgm_mesh_grid_normals_device: with
// d_out_normals also one normal per vertex.  Arguments checked; blocks once, at the end, for the two counts.
static int mesh_run(sgm_engine *e, const void *d_xyz, const void *d_disp_f32, const void *d_colors_rgb, int H, int W, float max_diff,
                    int orient, void *d_out_vertices, void *d_out_colors, void *d_out_faces, void *d_out_normals, int64_t *n_vertices,
                    int64_t *n_faces)
{
    if (H < 2 || W < 2) {   // no quad
        *n_vertices = 0;
        *n_faces = 0;
        return SGM_OK;
    }
    HIP_TRY(hipSetDevice(e->device));
    const int64_t n = (int64_t)H * W;
    const int m = (int)((n + MESH_BLOCK - 1) / MESH_BLOCK);   // (n <= 2^26: at most 2^16 blocks)
    int rc;
    if ((rc = e->mesh_code.ensure((size_t)n)) || (rc = e->mesh_num.ensure((size_t)n * 4)) || (rc = e->mesh_fcnt.ensure((size_t)(m + 1) * 4)) ||
        (rc = e->mesh_vcnt.ensure((size_t)(m + 1) * 4)))
        return rc;
    if (e->profile) stage_reset(e);   // the stage record is the call's from here on
    const float *xyz = (const float *)d_xyz, *disp = (const float *)d_disp_f32;
    const uint8_t *colors = (const uint8_t *)(d_out_colors ? d_colors_rgb : nullptr);
    uint8_t *code = (uint8_t *)e->mesh_code.p;
    uint32_t *number = (uint32_t *)e->mesh_num.p, *fcnt = (uint32_t *)e->mesh_fcnt.p, *vcnt = (uint32_t *)e->mesh_vcnt.p;
    hipStream_t st = e->stream;
    // 1. every quad's code and the blocks' numbers of triangles; 2. from the codes, the blocks' numbers of vertices
    if ((rc = mesh_stage_quads(e, xyz, disp, H, W, max_diff, m))) return rc;
    if ((rc = run_stage(e, "mesh_used", [&] { hipLaunchKernelGGL(k_mesh_used, dim3(m), dim3(MESH_BLOCK), 0, st, (const uint8_t *)code, H, W, vcnt); return 1; })))
        return rc;
    // 3. both lists of counts become offsets, the totals behind them
    rc = run_stage(e, "mesh_scan", [&] {
        hipLaunchKernelGGL(k_compact_scan, dim3(1), dim3(1024), 0, st, vcnt, m);
        hipLaunchKernelGGL(k_compact_scan, dim3(1), dim3(1024), 0, st, fcnt, m);
        return 2;
    });
    if (rc) return rc;
    // 4. the vertices and each used pixel's number; 5. the faces, in those numbers
    rc = run_stage(e, "mesh_vertices", [&] {
        hipLaunchKernelGGL(k_mesh_vertices, dim3(m), dim3(MESH_BLOCK), 0, st, xyz, colors, (const uint8_t *)code, H, W, (const uint32_t *)vcnt,
                           (float *)d_out_vertices, (uint8_t *)d_out_colors, number);
        return 1;
    });
    if (rc) return rc;
    rc = run_stage(e, "mesh_faces", [&] {
        hipLaunchKernelGGL(k_mesh_faces, dim3(m), dim3(MESH_BLOCK), 0, st, (const uint8_t *)code, (const uint32_t *)number, H, W,
                           (const uint32_t *)fcnt, (int32_t *)d_out_faces);
        return 1;
    });
    if (rc) return rc;
    // 6 - 9. the vertices' normals, to the rows step 4 numbered the pixels with
    if (d_out_normals) {
        rc = run_stage(e, "mesh_normals", [&] {
            hipLaunchKernelGGL(k_normals<true>, dim3(m), dim3(MESH_BLOCK), 0, st, xyz, (const uint8_t *)code, (const uint32_t *)number, H, W, orient,
                               (float *)d_out_normals);
            return 1;
        });
        if (rc) return rc;
    }
    uint32_t nv = 0, nf = 0;
    HIP_TRY(hipMemcpyAsync(&nv, vcnt + m, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&nf, fcnt + m, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *n_vertices = (int64_t)nv;
    *n_faces = (int64_t)nf;
    return SGM_OK;
}

// The same from host pointers through the engine's staging buffers, for sgm_mesh_grid and sgm_mesh_grid_normals
static int mesh_host_call(sgm_engine *e, const float *xyz, const float *disp, const uint8_t *colors_rgb, int H, int W, float max_diff,
                          int orient, float *out_vertices, uint8_t *out_colors, int32_t *out_faces, float *out_normals, int64_t *n_vertices,
                          int64_t *n_faces)
{
    int64_t nv = 0, nf = 0;
    if (H >= 2 && W >= 2) {   // (otherwise no quad)
        const size_t n = (size_t)H * W;
        const HostIn pts{xyz, &e->xyz, n * 12}, dsp{disp, &e->f32, n * 4}, rgb{out_colors ? colors_rgb : nullptr, &e->crgb_in, n * 3};
        const HostOut vtx{out_vertices, &e->cpts, 12, &nv}, vrgb{out_colors, &e->crgb, 3, &nv}, nrm{out_normals, &e->mesh_nrm, 12, &nv},
            faces{out_faces, &e->mesh_faces, 12, &nf, 2 * (int64_t)(H - 1) * (W - 1)};
        if (int rc = host_call(e, (int64_t)n, {pts, dsp, rgb}, {vtx, vrgb, nrm, faces}, [&] {
                return mesh_run(e, pts.d(), dsp.d(), rgb.d(), H, W, max_diff, orient, vtx.d(), vrgb.d(), faces.d(), nrm.d(), &nv, &nf);
            }))
            return rc;
    }
    *n_vertices = nv;
    *n_faces = nf;
    return SGM_OK;
}

int sgm_mesh_grid_device(sgm_engine *e, const void *d_xyz, const void *d_disp_f32, const void *d_colors_rgb, int H, int W, float max_diff,
                         void *d_out_vertices, void *d_out_colors, void *d_out_faces, int64_t *n_vertices, int64_t *n_faces)
{
    if (int rc = mesh_check_args("sgm_mesh_grid", !e || !d_xyz || !d_disp_f32 || !d_out_vertices || !d_out_faces || !n_vertices || !n_faces, H, W,
                                 max_diff, 0, d_out_colors && !d_colors_rgb))
        return rc;
    return mesh_run(e, d_xyz, d_disp_f32, d_colors_rgb, H, W, max_diff, 0, d_out_vertices, d_out_colors, d_out_faces, nullptr, n_vertices, n_faces);
}

int sgm_mesh_grid(sgm_engine *e, const float *xyz, const float *disp, const uint8_t *colors_rgb, int H, int W, float max_diff,
                  float *out_vertices, uint8_t *out_colors, int32_t *out_faces, int64_t *n_vertices, int64_t *n_faces)
{
    if (int rc = mesh_check_args("sgm_mesh_grid", !e || !xyz || !disp || !out_vertices || !out_faces || !n_vertices || !n_faces, H, W, max_diff, 0,
                                 out_colors && !colors_rgb))
        return rc;
    return mesh_host_call(e, xyz, disp, colors_rgb, H, W, max_diff, 0, out_vertices, out_colors, out_faces, nullptr, n_vertices, n_faces);
}

int sgm_mesh_grid_normals_device(sgm_engine *e, const void *d_xyz, const void *d_disp_f32, const void *d_colors_rgb, int H, int W,
                                 float max_diff, int orient, void *d_out_vertices, void *d_out_colors, void *d_out_faces,
                                 void *d_out_normals, int64_t *n_vertices, int64_t *n_faces)
{
    if (int rc = mesh_check_args("sgm_mesh_grid_normals",
                                 !e || !d_xyz || !d_disp_f32 || !d_out_vertices || !d_out_faces || !d_out_normals || !n_vertices || !n_faces, H, W,
                                 max_diff, orient, d_out_colors && !d_colors_rgb))
        return rc;
    return mesh_run(e, d_xyz, d_disp_f32, d_colors_rgb, H, W, max_diff, orient, d_out_vertices, d_out_colors, d_out_faces, d_out_normals,
                    n_vertices, n_faces);
}

int sgm_mesh_grid_normals(sgm_engine *e, const float *xyz, const float *disp, const uint8_t *colors_rgb, int H, int W, float max_diff,
                          int orient, float *out_vertices, uint8_t *out_colors, int32_t *out_faces, float *out_normals,
                          int64_t *n_vertices, int64_t *n_faces)
{
    if (int rc = mesh_check_args("sgm_mesh_grid_normals", !e || !xyz || !disp || !out_vertices || !out_faces || !out_normals || !n_vertices || !n_faces,
                                 H, W, max_diff, orient, out_colors && !colors_rgb))
        return rc;
    return mesh_host_call(e, xyz, disp, colors_rgb, H, W, max_diff, orient, out_vertices, out_colors, out_faces, out_normals, n_vertices, n_faces);
}

// The normal image: the quads' codes, then one pass over the pixels.  Nothing is counted, so nothing waits.
int sgm_normals_grid_device(sgm_engine *e, const void *d_xyz, const void *d_disp_f32, int H, int W, float max_diff, int orient,
                            void *d_out_normals)
{
    if (int rc = mesh_check_args("sgm_normals_grid", !e || !d_xyz || !d_disp_f32 || !d_out_normals, H, W, max_diff, orient, false)) return rc;
    HIP_TRY(hipSetDevice(e->device));
    const int64_t n = (int64_t)H * W;
    if (e->profile) stage_reset(e);   // the stage record is the call's from here on
    if (H < 2 || W < 2) {             // no quad, no vertex, no stage
        HIP_TRY(hipMemsetAsync(d_out_normals, 0, (size_t)n * 12, e->stream));
        return SGM_OK;
    }
    const int m = (int)((n + MESH_BLOCK - 1) / MESH_BLOCK);
    int rc;
    if ((rc = e->mesh_code.ensure((size_t)n)) || (rc = e->mesh_fcnt.ensure((size_t)(m + 1) * 4))) return rc;
    if ((rc = mesh_stage_quads(e, (const float *)d_xyz, (const float *)d_disp_f32, H, W, max_diff, m))) return rc;
    return run_stage(e, "normals_grid", [&] {
        hipLaunchKernelGGL(k_normals<false>, dim3(m), dim3(MESH_BLOCK), 0, e->stream, (const float *)d_xyz, (const uint8_t *)e->mesh_code.p,
                           (const uint32_t *)nullptr, H, W, orient, (float *)d_out_normals);
        return 1;
    });
}

int sgm_normals_grid(sgm_engine *e, const float *xyz, const float *disp, int H, int W, float max_diff, int orient, float *out_normals)
{
    if (int rc = mesh_check_args("sgm_normals_grid", !e || !xyz || !disp || !out_normals, H, W, max_diff, orient, false)) return rc;
    const size_t n = (size_t)H * W;
    if (H < 2 || W < 2) {
        memset(out_normals, 0, n * 12);
        return SGM_OK;
    }
    const HostIn pts{xyz, &e->xyz, n * 12}, dsp{disp, &e->f32, n * 4};
    const HostOut nrm{out_normals, &e->mesh_nrm, 12, nullptr};
    return host_call(e, (int64_t)n, {pts, dsp}, {nrm}, [&] { return sgm_normals_grid_device(e, pts.d(), dsp.d(), H, W, max_diff, orient, nrm.d()); });
}

int sgm_filter_speckles(sgm_engine *e, int16_t *img, int H, int W, int newVal, int maxSpeckleSize, int maxDiff)
{
    if (!e || !img || H <= 0 || W <= 0) return set_err(SGM_ERR_INVALID_ARG, "bad argument");
    HIP_TRY(hipSetDevice(e->device));
    const size_t npx = (size_t)H * W;
    int rc;
    if ((rc = e->disp_out.ensure(npx * 2))) return rc;
    HIP_TRY(hipMemcpyAsync(e->disp_out.p, img, npx * 2, hipMemcpyHostToDevice, e->stream));
    if ((rc = run_speckles(e, (int16_t *)e->disp_out.p, H, W, newVal, maxSpeckleSize, maxDiff))) return rc;
    HIP_TRY(hipMemcpyAsync(img, e->disp_out.p, npx * 2, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return SGM_OK;
}

int sgm_get_tap(sgm_engine *e, int tap, void *host_dst, int64_t bytes)
{
    if (!e || !host_dst) return set_err(SGM_ERR_INVALID_ARG, "bad argument");
    if (e->H <= 0) return set_err(SGM_ERR_INVALID_ARG, "no compute has run yet");
    HIP_TRY(hipSetDevice(e->device));
    const int64_t npx = (int64_t)e->H * e->W;
    const int64_t vol = std::max<int64_t>(e->g.rowsz, 0) * e->H * 2;
    const void *src = nullptr;
    int64_t need = 0;
    switch (tap) {
    case SGM_TAP_COST: src = e->cost.p; need = vol; break;
    case SGM_TAP_AGGR:
        if (!e->keep_aggr) return set_err(SGM_ERR_INVALID_ARG, "SGM_TAP_AGGR needs SGM_OPT_KEEP_AGGR=1 before compute");
        src = e->aggr.p; need = vol; break;
    case SGM_TAP_DISP_RAW: src = e->disp_raw.p; need = npx * 2; break;
    case SGM_TAP_DISP_MEDIAN: src = e->disp_med.p; need = npx * 2; break;
    case SGM_TAP_CONF_RAW:
    case SGM_TAP_CONF:
    case SGM_TAP_RIGHT_RAW:
    case SGM_TAP_RIGHT: {
        const SideMap &m = tap == SGM_TAP_CONF_RAW || tap == SGM_TAP_CONF ? e->conf : e->right;
        if (!m.last) return set_err(SGM_ERR_INVALID_ARG, "tap %d needs %s=1 before compute", tap, m.opt_name);
        if (tap == m.tap_fin && m.last == 2)
            return set_err(SGM_ERR_INVALID_ARG, "%s: the last compute wrote its map to the pointer bound with %s", m.tap_fin_name, m.bind_name);
        src = tap == m.tap_raw ? m.raw.p : m.fin.p; need = npx * m.bpp; break;
    }
    default: return set_err(SGM_ERR_INVALID_ARG, "unknown tap %d", tap);
    }
    if (bytes != need) return set_err(SGM_ERR_INVALID_ARG, "tap %d holds %lld bytes, caller passed %lld", tap, (long long)need, (long long)bytes);
    if (need == 0) return SGM_OK;
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(host_dst, src, (size_t)need, hipMemcpyDeviceToHost));
    return check_chain(e);
}

int sgm_get_headroom(sgm_engine *e, int *max_cost_plus_p2, int *max_delta, int *ok)
{
    if (!e) return set_err(SGM_ERR_INVALID_ARG, "engine is null");
    if (e->H <= 0 || !e->headroom.p) return set_err(SGM_ERR_INVALID_ARG, "no compute has run yet");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    // the last call's record: after a batch call, the maximum over every pair of the batch (each pair of a chained group
    // keeps its record on the internal engine that ran it; e's stream ends behind all of them)
    uint32_t h[2] = {0, 0};
    HIP_TRY(hipMemcpy(h, e->headroom.p, 8, hipMemcpyDeviceToHost));
    std::vector<sgm_engine *> behind;
    for (int k = 0; k < e->last_group && k < (int)e->group.size(); k++) behind.push_back(e->group[k]);
    if (e->last_peers >= 1 && e->peer) behind.push_back(e->peer);      // (sgm_compute_batch in latency mode: the call has
    if (e->last_peers >= 2 && e->peer2) behind.push_back(e->peer2);    //  drained their streams before it returned)
    for (sgm_engine *o : behind) {
        uint32_t q[2] = {0, 0};
        if (!o->headroom.p) continue;
        HIP_TRY(hipMemcpy(q, o->headroom.p, 8, hipMemcpyDeviceToHost));
        h[0] = std::max(h[0], q[0]);
        h[1] = std::max(h[1], q[1]);
    }
    // an int16 lane upstream holds C_true + P2 and min_d L_r + P2: both must fit
    const int64_t a = e->g.W1 > 0 ? (int64_t)h[0] + e->g.P2 : 0, b = e->g.W1 > 0 ? (int64_t)h[1] + e->g.P2 : 0;
    if (max_cost_plus_p2) *max_cost_plus_p2 = (int)std::min<int64_t>(a, INT32_MAX);
    if (max_delta) *max_delta = (int)std::min<int64_t>(b, INT32_MAX);
    if (ok) *ok = (a <= SGM_MAX_COST && b <= SGM_MAX_COST) ? 1 : 0;
    return SGM_OK;
}

int sgm_get_stage_times(sgm_engine *e, sgm_stage_times *out)
{
    if (!e || !out) return set_err(SGM_ERR_INVALID_ARG, "bad argument");
    if (!e->profile) return set_err(SGM_ERR_INVALID_ARG, "SGM_OPT_PROFILE is off");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    // one entry per stage NAME: a stage may consist of several bracketed launches (row chunks of the
    // pipelined first pass, on streams of their own) -- their HIP-event times and launch counts add up
    out->n = 0;
    for (int i = 0; i < e->nstages; i++) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, e->events[e->stage_ev[i * 2]], e->events[e->stage_ev[i * 2 + 1]]));
        int k = 0;
        while (k < out->n && strcmp(out->name[k], e->stage_names[i]) != 0) k++;
        if (k == out->n) {
            if (out->n >= SGM_MAX_STAGES - 1) continue;
            out->name[k] = e->stage_names[i];
            out->ms[k] = 0.f;
            out->launches[k] = 0;
            out->n++;
        }
        out->ms[k] += ms;
        out->launches[k] += e->stage_launches[i];
    }
    // stages overlap (auxiliary / chunk streams): also report first-begin -> last-end of the main stream
    if (e->nstages > 0) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, e->events[e->stage_ev[0]], e->events[e->stage_ev[(e->nstages - 1) * 2 + 1]]));
        out->name[out->n] = "_wall";
        out->ms[out->n] = ms;
        out->launches[out->n] = 0;
        out->n++;
    }
    return SGM_OK;
}

// SURVEY.md 8(d):  B_alg = 2HW (L,R in) + V (1 + 3 Np) + 2HW (disp out) + 8HW (median, speckle r+w)
//                          [+ 16 HW reproject], V = 2 H W1 D bytes, Np = 5 (mode 0), 8 (mode 1) or 4 (mode 3).
int64_t sgm_algorithmic_bytes(const sgm_params *params, int H, int W, int with_reproject)
{
    Geom g;
    if (!params || normalise(params, H, W, &g)) return -1;
    const int64_t HW = (int64_t)H * W;
    const int64_t V = 2 * (int64_t)H * std::max(g.W1, 0) * g.D;
    const int Np = g.mode == 1 ? 8 : (g.mode == 3 ? 4 : 5);
    int64_t b = 2 * HW + V * (1 + 3 * Np) + 2 * HW + 8 * HW;
    if (with_reproject) b += 16 * HW;
    return b;
}

}  // extern "C"
