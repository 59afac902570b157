// fs_capi.hip — the C ABI of include/fitslam_frontier.h: context, staging of grid / landmarks / lookup
// table into HBM, host-side precomputation (fan directions, yaw rotations, crowding factors, dense
// table) and the launch sequences.  No CPU compute fallback exists: every scoring entry point
// launches the HIP kernels of fs_raymarch.hip / fs_fim.hip / fs_rank.hip or fails.
#include "fs_internal.h"
#include "fs_keepout.h"
#include "fs_median_sort.h"
#include "fs_navfn_wave.h"
#include "fs_roadmap_astar.h"
#include "fs_thetastar.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <map>
#include <string>
#include <thread>
#include <unordered_map>
#include <unordered_set>
#include <utility>
#include <vector>

hipError_t fs_launch_rank(int32_t n, const fs_record *d_records, const uint8_t *d_black,
                          const double *d_len, const double *d_head, double alpha, double beta,
                          double max_vx, double max_wz, double max_gt, double *d_cost, double *d_au,
                          double *d_du, int32_t *d_order, int32_t *d_err, void **scratch, size_t *scratch_bytes,
                          hipStream_t s);

// Counts every (re)allocation of device / page-locked memory the library makes, in any context: a captured launch graph holds
// raw pointers, and is only replayed while this number is what it was at capture time.
std::atomic<uint64_t> fs_alloc_generation{0};     // (atomic: fs_multi stages its members from one host thread each)

namespace {

// Development build FS_POISON (`FS_POISON=1 python fit-slam_amd/_build.py`, a library of its own like every FS_DEV build): a
// buffer that grows is RETIRED, not freed — nothing allocated later can land on its address — and both the retired and the new
// memory are filled with 0xCD.  A launch that still holds a pointer taken before the growth then writes where nobody reads, and
// whoever reads the new buffer finds the pattern instead of a result: the stale-pointer defect of round 5 (fs_score_candidates_dev,
// DESIGN.md 0) fails every time under this build instead of only when the allocator happens to hand out a different address;
// so does anything that relies on fresh device memory being zero.  Leaks by design; test processes only.
#ifdef FS_POISON
static void poison_device(void *p, size_t bytes)
{
    (void)hipDeviceSynchronize();
    (void)hipMemset(p, 0xCD, bytes);
    (void)hipDeviceSynchronize();
}
#endif

// Bytes the DevBuf / PinnedBuf objects of every context hold at this moment (fs_get_counter 1036): `ensure` adds what it allocated,
// `release`, the destructor and a move take off what they free.  Process-wide like fs_alloc_generation, so a test can ask for
// "a destroyed context gave everything back" exactly, on a device whose memory other processes use too.  Not in it: memory an
// FS_POISON build has retired (it is no buffer's any more), rank_scratch and sort_scratch (raw pointers grown in fs_rank.hip /
// fs_sort.hip).
std::atomic<int64_t> buf_bytes_held{0};

// A buffer owns its memory: destruction frees it, a move hands it over, a copy does not exist.
template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    hipError_t ensure(size_t n)
    {
        if (n <= cap) return hipSuccess;
        buf_bytes_held -= (int64_t)(cap * sizeof(T));
#ifdef FS_POISON
        if (p) poison_device(p, cap * sizeof(T));                 // retired
#else
        if (p) (void)hipFree(p);
#endif
        p = nullptr; cap = 0;
        size_t want = std::max<size_t>(n, 64);
        ++fs_alloc_generation;
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&p), want * sizeof(T));
        if (e == hipSuccess) { cap = want; buf_bytes_held += (int64_t)(want * sizeof(T)); }
#ifdef FS_POISON
        if (e == hipSuccess) poison_device(p, want * sizeof(T));
#endif
        return e;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        buf_bytes_held -= (int64_t)(cap * sizeof(T));
        p = nullptr; cap = 0;
    }
};

// page-locked staging memory of a context: copies from / to it are true DMA transfers that overlap with the host, copies
// from pageable user memory are staged by the runtime in small synchronous pieces (measured on C3's 20 k candidates: 1.29 ms per
// fs_score_candidates call with pageable copies of the three input columns and the records)
// The buffer is also MAPPED into the device's address space (`dev`, nullptr if the runtime refuses): a small call lets its
// kernels read the candidate columns from it and write the results into it directly — a transfer of a few hundred bytes costs
// 4-5 us as an operation of its own on the stream (measured: five result columns against two, 46 against 33 us per one-pose
// call), a handful of PCIe reads and posted writes inside kernels that run anyway cost nothing that shows.
struct PinnedBuf {
    char *p = nullptr, *dev = nullptr;
    size_t cap = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
    PinnedBuf(PinnedBuf &&o) noexcept : p(o.p), dev(o.dev), cap(o.cap) { o.p = nullptr; o.dev = nullptr; o.cap = 0; }
    PinnedBuf &operator=(PinnedBuf &&o) noexcept
    {
        if (this != &o) { release(); p = o.p; dev = o.dev; cap = o.cap; o.p = nullptr; o.dev = nullptr; o.cap = 0; }
        return *this;
    }
    ~PinnedBuf() { release(); }
    hipError_t ensure(size_t bytes)
    {
        if (bytes <= cap) return hipSuccess;
        buf_bytes_held -= (int64_t)cap;
#ifdef FS_POISON
        if (p) { (void)hipDeviceSynchronize(); std::memset(p, 0xCD, cap); }      // retired (see DevBuf)
#else
        if (p) (void)hipHostFree(p);
#endif
        p = nullptr; dev = nullptr; cap = 0;
        const size_t want = std::max<size_t>(bytes, 4096);
        ++fs_alloc_generation;
        hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&p), want, hipHostMallocMapped);
#ifdef FS_POISON
        if (e == hipSuccess) std::memset(p, 0xCD, want);
#endif
        if (e != hipSuccess) {
            // a runtime / device that refuses MAPPED page-locked memory still gets plain page-locked staging: dev stays nullptr and
            // every entry point takes its transfer path (the sticky error of the refused call is cleared first)
            (void)hipGetLastError();
            p = nullptr;
            e = hipHostMalloc(reinterpret_cast<void **>(&p), want, hipHostMallocDefault);
            if (e != hipSuccess) { p = nullptr; return e; }
            cap = want;
            buf_bytes_held += (int64_t)want;
            return hipSuccess;
        }
        cap = want;
        buf_bytes_held += (int64_t)want;
        void *d = nullptr;
        if (hipHostGetDevicePointer(&d, p, 0) == hipSuccess) dev = static_cast<char *>(d);
        else (void)hipGetLastError();
        return hipSuccess;
    }
    void release()
    {
        if (p) (void)hipHostFree(p);
        buf_bytes_held -= (int64_t)cap;
        p = nullptr; dev = nullptr; cap = 0;
    }
};
#define FS_ZERO_COPY_MAX_N 1024   // candidates / poses up to which a host-buffer call reads and writes the mapped staging buffers in place

struct TimedLaunch {
    int kind;
    hipEvent_t start, stop;
};

// One captured launch sequence of a small host-buffer call: valid while the context's epoch (every staging /
// parameter call bumps it) and the allocation generation are what they were when it was captured.
struct GraphEntry {
    hipGraphExec_t exec = nullptr;
    uint64_t stamp = 0;          // epoch + allocation generation the graph was captured under
    uint64_t warm_stamp = 0;     // ... a plain call has run under (it made every allocation the sequence needs)
    bool broken = false;         // capture failed once: this sequence stays on plain launches
};

// One keep-out zone as the layer stores it (zone_specs_, keepout_layer.hpp): the request, never its cells — those follow from
// the staged map's geometry.  n_cells: distinct cells it marks on the map staged now.
struct KoZone {
    int32_t kind;                // FS_KO_FOV: size = height [m];  FS_KO_DISC: size = radius [m], yaw = 0
    double wx, wy, yaw, size;
    int64_t n_cells;
};
// the geometry a zone's cells depend on
struct KoGeom {
    int32_t nx, ny;
    double ox, oy, res;
    bool operator==(const KoGeom &o) const { return nx == o.nx && ny == o.ny && ox == o.ox && oy == o.oy && res == o.res; }
};

// One cost table of the inflation layer on the device: what it was computed from, its reach in cells, cost_by_d2 [R * R + 1]
struct InflTable {
    double inflation_radius, inscribed_radius, cost_scaling_factor, res;
    int32_t R;
    DevBuf<uint8_t> d_cost;
};
#define FS_INFL_TABLES 8

}  // namespace

struct fs_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string err;

    // ray parameters
    bool have_ray = false;
    fs_ray_params rp{};
    int32_t n_yaw = 0, n_elev = 0, window = 0;
    DevBuf<double> d_dir;
    DevBuf<float> d_yawR;
    double max_gt = 0.0, min_gt = 0.0;

    // grid
    bool have_grid = false;
    DevBuf<uint8_t> d_cells;                        // dense row-major image (FsGridDev)
    DevBuf<uint32_t> d_cls;                         // 2-bit class image, cut lazily for cls_ranges (long rays only)
    bool have_cls = false;
    DevBuf<uint32_t> d_cls_table, d_cls_pool;       // "ray.layout" 3: brick table + pool of distinct bricks (the sparse form of d_cls)
    bool have_sparse = false;
    int64_t sparse_bricks = 0, sparse_pool_bricks = 0;    // counters 1000 / 1001
    int32_t cls_ranges[4] = {0, 0, 0, 0};
    int32_t nx = 0, ny = 0, nz = 0;
    double origin[3] = {0, 0, 0};
    double res = 0.0;

    // keep-out zones (fs_keepout.hip): the stored requests; the union of their cells on the staged 2-D map, valid for ko_geom;
    // the scratch image ONE zone is rasterised into (all zero between calls); ray table and per-zone cell counts
    std::vector<KoZone> ko_zones;
    bool ko_mask_valid = false;
    KoGeom ko_geom{0, 0, 0.0, 0.0, 0.0};
    DevBuf<uint8_t> d_ko_mask, d_ko_scratch;
    DevBuf<int32_t> d_ko_rays;
    DevBuf<unsigned long long> d_ko_counts;

    // the inflation layer (fs_inflate.hip): the cost tables of the parameter sets seen (the host fills one with
    // its libm and uploads it once; the reference runs three sets, a handful is kept), the row distances of the call, its counters
    std::vector<InflTable> infl_tables;
    size_t infl_next = 0;                           // the slot a new set takes once all are used
    DevBuf<uint16_t> d_infl_g;
    DevBuf<unsigned long long> d_infl_counts;

    // the information layer (fs_infolayer.hip): anchor | flag [nb + 1] | rank [nb + 1] | list; the heading pairs
    // (il_quat: their host copy, alive until the call's last wait); the pose records of a batch; the worker's values
    // [scored][K]; info [nb] | per_yaw [K][nb]; rocPRIM's scratch; n_changed
    int64_t opt_il_batch = 65536;                   // "infolayer.batch": poses per scoring launch
    DevBuf<int32_t> d_il_idx;
    DevBuf<double> d_il_quat;
    std::vector<double> il_quat;
    DevBuf<float> d_il_rt, d_il_val, d_il_out;
    DevBuf<char> d_il_temp;
    DevBuf<unsigned long long> d_il_count;

    // the sensor sweep (fs_sense.hip): the ground-truth world, of the staged grid's shape; the mark image of seen
    // cells (all zero between calls — sense_mark_clean says it is known to be); the direction table of the last non-NULL `sensor`
    // (sense_dir: its host copy, what a new one is compared with); the call's inputs and results (d_sense_out: box [6] | status [n]
    // | seen_unknown [n]; d_sense_counts [4]: the merge's seen / revealed cells, the census)
    bool have_world = false;
    DevBuf<uint8_t> d_world, d_sense_mark, d_sense_mapped;
    bool sense_mark_clean = false;
    std::vector<double> sense_dir;
    DevBuf<double> d_sense_dir, d_sense_origin;
    DevBuf<int32_t> d_sense_first, d_sense_rays, d_sense_out;
    DevBuf<unsigned long long> d_sense_counts;
    // the drive (fs_drive.hip): stations and goals; one int32 block of inputs, presets and results (see fs_drive)
    DevBuf<double> d_drive_xyz;
    DevBuf<int32_t> d_drive_i32;

    // the landmark sensor (fs_sense_landmarks.hip): the ground-truth cloud as raw xyz [wl_m][3], in a k-d leaf order
    // of its own (SoA padded to wl_chunks chunks, spheres, d_wl_perm: the world index per slot) and with one sighting counter and
    // one `discovered` flag per landmark; wl_discovered: how many flags are set; wl_staged: the staged cloud IS the discovered set
    // (cleared by every other route that stages a cloud).  d_wl_out: totals [3] (new, discovered, discovered and usable) |
    // n_in_view [n]; d_wl_blocks: per block of 256 landmarks the counts [2] and, behind them, their exclusive sums.
    bool have_wl = false, wl_staged = false;
    int32_t wl_m = 0, wl_chunks = 0, wl_discovered = 0;
    DevBuf<float> d_wl_raw, d_wl_lx, d_wl_ly, d_wl_lz, d_wl_spheres, d_wl_Rt;
    DevBuf<int32_t> d_wl_perm, d_wl_inv, d_wl_out, d_wl_blocks;
    DevBuf<uint32_t> d_wl_views;
    DevBuf<uint8_t> d_wl_flag;
    // the gated drive (fs_drive_slam.hip): d_ds_out = fallbacks [1] | in_view [T] | voxels [T] | information [T]
    // (float bits), what comes back; the slabs' partial sums; counters 1047 .. 1049: host waits of the last call, voxels per pose
    // the LDS tier takes at most, workgroups that took the fallback tier
    DevBuf<int32_t> d_ds_out;
    DevBuf<double> d_ds_partial;
    int64_t ds_waits = 0, ds_capacity = (int64_t)FS_GATE_SLABS * FS_GATE_SLOTS, ds_fallbacks = 0;

    // landmarks
    bool have_lm = false;
    int32_t m = 0, n_chunks = 0;
    DevBuf<float> d_lx, d_ly, d_lz, d_spheres;
    bool opt_cull = true;
    bool opt_learn = true;         // "fim.learn": the pass prediction uses the voxel ratio finished calls have shown (0: the fixed cap only — results then do not depend on the calls a context has served before)
    bool opt_special = true;       // "fim.specialise": the INFO_ONLY / YAW_ONLY workers where they apply (0: always the general worker)
    bool yaw_exact = false;        // every rotation of d_yawR is about Z with exact zeros / one (what YAW_ONLY relies on)
    int opt_bits1 = 14;            // development knobs (fs_set_option "fim.bits1", "fim.skip32")
    int opt_skip32 = 13;
    // "fim.headroom": what the pass prediction multiplies the learnt voxel ratio by, in 32nds.  The ratio is the LARGEST any big
    // pose showed and a pass is sized for a table 3/4 full, so 28/32 still leaves the worst pose seen at 86 % load; round 3's
    // 5/4 sent 7 312 of C3's 20 000 poses into a second pass at the reference's visibility request where 2 943 hold more voxels
    // than one pass takes (tools/ref_visibility_probe.py, profiles/r04/ref_visibility_pass_margin.jsonl: 1.87 -> 1.69 ms)
    int opt_headroom = 28;
    DevBuf<unsigned long long> d_counters;
    // fs_set_occlusion: landmarks count only in line of sight on the staged grid.  Off: no call comes near the code.
    fs_occlusion_params occ{0, 254, 254, 0.3};

    // lookup table
    bool have_table = false;
    std::vector<float> records;           // as in the .dat, [n][4]
    std::vector<float> dense;             // host copy of the dense table
    int32_t jx0 = 0, jy0 = 0, jz0 = 0, tx = 0, ty = 0, tz = 0;
    DevBuf<float> d_table, d_factor;
    bool have_factor = false;
    bool table_full = false;
    float fac[5] = {0, 0, 0, 0, 0};

    // fim parameters
    fs_fim_params fp{14.0, 1.0};

    // key-frames (computeInformationForPose)
    bool have_kf = false;
    int32_t n_kf = 0;
    int64_t n_kf_points = 0;
    std::vector<double> kf_pose;          // host copy [n_kf][7]: the check points depend on the call's parameters
    DevBuf<double> d_kf_check, d_kf_tri;
    DevBuf<int32_t> d_kf_off, d_kf_flagged, d_kf_cells, d_kf_points;
    DevBuf<float> d_kpx, d_kpy, d_kpz;
    DevBuf<uint32_t> d_kf_gtable;
    DevBuf<unsigned long long> d_kf_counters;

    // hash tables
    DevBuf<uint32_t> d_gtable;
    int ghash_bits = 0;
    static constexpr int kPool = 64;      // tier 3 (rare: no candidate of C3 or C5 reaches it): 64 x 1024 threads — an empty launch of 256 cost 7.5 us per call

    // per-candidate scratch
    DevBuf<double> d_goal, d_yaw, d_len, d_head, d_cost, d_au, d_du, d_sums;
    DevBuf<int32_t> d_fsize, d_arrival, d_argmax, d_status, d_nvis, d_nvox, d_raycounts, d_order, d_err;
    DevBuf<uint8_t> d_black, d_achin, d_ach;
    DevBuf<float> d_info, d_trace, d_logdet, d_fim21, d_Rt;
    DevBuf<uint32_t> d_overflow, d_tested, d_split_flags;
    int opt_split = 3;             // "fim.split": log2 of the workgroups ONE info-only pose is spread over when a call has few poses (0: off)
    DevBuf<int32_t> d_flagged;
    size_t tested_zeroed = 0;
    DevBuf<fs_record> d_records;
    void *rank_scratch = nullptr;
    size_t rank_scratch_bytes = 0;
    void *sort_scratch = nullptr;
    size_t sort_scratch_bytes = 0;
    DevBuf<int32_t> d_perm;
    PinnedBuf h_in, h_out;         // staging of the per-call candidate columns / of the records
    DevBuf<char> d_in;             // the candidate columns of the host-buffer entry points, packed as in h_in
    const double *in_goal = nullptr; const int32_t *in_fsize = nullptr; const uint8_t *in_black = nullptr, *in_achin = nullptr;
    // fs_score_arrival_begin -> _end: where the columns waiting in h_out go (caller's arrays) once the stream has drained
    struct PendingCol { void *host; size_t off, bytes; };
    std::vector<PendingCol> arrival_pending;
    std::vector<PendingCol> fim_pending;           // fs_score_fim_begin -> _end, likewise
    // ... and the finish of a split info-only call that fs_score_fim_end runs on the HOST (host_finish, fs_score_fim_begin): the
    // partial sums of every (pose, w) item land in mapped page-locked memory behind a flag word; the kernel arguments are kept for
    // the rare call that needs the HBM tier and the finish kernel after all
    PinnedBuf h_fin;
    bool fin_active = false;
    FsFimArgs fin_args{};
    size_t fin_off_info = 0, fin_off_nvox = 0;
    bool fin_want_nvox = false;
    bool opt_host_finish = true;   // "fim.hostfinish"
    // the gather role of fs_multi_get_frontier_costs' member 0 (its own block still goes through h_in / d_in): the planner's
    // path columns and the blacklist of the WHOLE list; the gathered records live in d_out, ahead of the ranking's columns
    PinnedBuf h_gin;
    DevBuf<char> d_gin;
    // scratch of the per-tick entry points (fs_trace_segments, fs_frontier_cells, fs_information_frontier_pair,
    // fs_upload_grid_bricks): owned by the context and grown on demand, never allocated and freed per call
    DevBuf<double> d_seg_start, d_seg_end, d_tri;
    DevBuf<uint8_t> d_seg_ok, d_seg_hit, d_mask, d_brick_cells, d_win;
    PinnedBuf h_win;               // fs_update_grid_region: the packed window
    DevBuf<int32_t> d_seg_traced, d_seg_unknown, d_seg_all, d_brick_xyz, d_bad;
    DevBuf<unsigned long long> d_count;
    // fs_frontier_clusters
    DevBuf<int32_t> d_fc_parent_t, d_fc_parent_f, d_fc_aux, d_fc_state, d_fc_labels;
    DevBuf<uint32_t> d_fc_queue;
    DevBuf<uint8_t> d_fc_visited;
    DevBuf<fs_frontier_cluster> d_fc_clusters;
    DevBuf<long long> d_fc_sums;
    // fs_search_frontiers (fs_search.hip)
    DevBuf<int32_t> d_fs_bcount, d_fs_cidx, d_fs_root, d_fs_best_idx, d_fs_csize, d_fs_owner, d_fs_key, d_fs_pos, d_fs_q, d_fs_state, d_fs_seeds;
    DevBuf<int32_t> d_fs_emit_comp, d_fs_emit_seed, d_fs_emit_base, d_fs_rec_base, d_fs_fsize;
    DevBuf<unsigned long long> d_fs_best_d2;
    DevBuf<fs_msort_elem> d_fs_sort;
    DevBuf<fs_frontier_record> d_fs_rec;
    DevBuf<double> d_fs_every, d_fs_goal, d_fs_black_xy;
    DevBuf<uint8_t> d_fs_black;
    int64_t fs_levels = 0, fs_guarded = 0;      // counters 1014 / 1015 of the last search
    int32_t fs_seed_order = FS_SEEDS_NEAREST;   // fs_set_frontier_seed_order: the seeds of a search without caller seeds
    bool fs_outer = false;                      // the search in flight walks the outer search (Reference seeds)
    int64_t fs_outer_levels = 0, fs_outer_popped = 0;   // counters 1019 / 1020 of the last Reference search
    // "cloud.order": where the landmark cloud is put into its k-d leaf order — 0 on the host, 2 on the device (fs_cloud.hip), 1 (default)
    // on the device from FS_CLOUD_DEVICE_FROM landmarks on: fs_upload_landmarks 1.2 ms at C3's 100 k landmarks, 4.4 ms at 500 k on the
    // device (the host form: 4.4 / 20.2 ms with its top levels on threads of their own, 13.3 / 78.9 ms on one thread —
    // tools/landmark_staging_probe.py); a level costs the device ~ 0.03 ms of launches whatever its size, so a 2 k cloud is faster
    // on the host (0.06 against 0.18 ms).  Scratch of the device path below.
    int opt_cloud_order = 1;
    DevBuf<float> d_cloud_raw;
    DevBuf<int32_t> d_cloud_perm, d_cloud_bounds;
    DevBuf<uint64_t> d_cloud_keys;
    DevBuf<uint32_t> d_cloud_bbox;
    DevBuf<char> d_cloud_temp;
    // fs_landmarks_in_view (fs_view.hip).  Kept with the staged cloud by both ordering routes and refreshed by every
    // upload: d_view_perm [n_chunks * 64] = the landmark's position in the uploaded array per staged slot (-1: a sentinel),
    // d_view_inv [m] = the slot per position (-1: unusable).  The rest is the call's scratch.
    DevBuf<int32_t> d_view_perm, d_view_inv, d_view_counts;
    DevBuf<float> d_view_Rt;
    DevBuf<uint32_t> d_view_mask;
    DevBuf<int64_t> d_view_off;
    DevBuf<fs_view_landmark> d_view_out;
    int32_t opt_view_round = 0;    // "view.round_poses": poses per round; 0 = as many as FS_VIEW_MASK_BYTES of mask words hold
    bool opt_sort = true;
    bool opt_sort_reverse = false; // development: blocks in reverse Morton order (order-sensitivity measurements)
    bool opt_costmap = true;       // the spatial sort puts the blocks that were expensive in the previous call first ("sort.costmap")
    const uint32_t *sort_keys = nullptr;   // this call's sort keys / the cost map inside sort_scratch (nullptr: list not sorted)
    uint32_t *sort_costmap = nullptr;
    int opt_layout = 0;            // "ray.layout": 0 by ray length, 1 row-major byte walk, 2 class-image walk, 3 sparse class image (experiment)

    // launch graphs of the small host-buffer calls ("graph" option; off while kernel timing is on)
    bool opt_zero_copy = true;     // "zerocopy": small host-buffer calls read / write the mapped page-locked buffers in place
    bool opt_graph = false;        // measured 5-7 us SLOWER per call than plain launches on ROCm 7.2 (profiles/r04/small_call_graphs.json): off by default
    uint64_t epoch = 1;
    std::map<uint64_t, GraphEntry> graphs;
    DevBuf<char> d_out;            // packed results of fs_get_frontier_costs (records | cost | utilities | order | error flag)

    // batched grid planner (fs_navfn.hip): the potential field is kept per (grid generation, robot cell, allow_unknown); every
    // staging call that writes the grid bumps grid_gen
    uint64_t grid_gen = 1;
    bool nav_valid = false;
    uint64_t nav_gen = 0;
    int32_t nav_rx = -1, nav_ry = -1, nav_allow = -1, nav_buf = 0;
    int64_t nav_builds = 0, nav_rounds = 0, nav_launches = 0;
    DevBuf<uint8_t> d_nav_cost;
    DevBuf<float> d_nav_pot;          // [2][ny][nx]: the round buffers
    DevBuf<uint32_t> d_nav_flags;     // [2][tiles]
    DevBuf<int32_t> d_nav_any;        // one word per round of a batch
    DevBuf<float> d_nav_path;         // [n][2][4 * max(nx, ny)] path points
    DevBuf<char> d_nav_in, d_nav_out; // goal cells | headings;  path length | length in m | heading | achievable
    PinnedBuf h_nav_in, h_nav_out;
    // the REFERENCE grid search (fs_set_grid_search): one calcNavFnAstar wave per distinct goal cell (fs_navfn_wave.h), in batches
    // of slots; nothing is kept across calls
    int32_t nav_search = FS_GRID_SEARCH_CONVERGED;
    int32_t nw_opt_slots = 0;                 // "navfn.wave_slots": 0 = as many as "navfn.wave_bytes" holds
    int64_t nw_opt_bytes = (int64_t)1 << 30;  // "navfn.wave_bytes"
    int32_t nw_opt_cap = 10000;               // "navfn.wave_cap": entries of each priority buffer (tests; the reference's 10 000)
    int64_t nw_batches = 0;                   // slot batches of the last call (counter 1038)
    DevBuf<float> d_nw_pot;           // [slots][ny][nx]
    DevBuf<uint8_t> d_nw_pend;        // [slots][ny][nx]
    DevBuf<int32_t> d_nw_buf;         // [slots][3][cap]
    DevBuf<int32_t> d_nw_idx;         // stats [4] | wave cell [n] | frontier wave [n] | first [n] | wave limit [n] (NwIdxLayout)
    PinnedBuf h_nw_idx;               // stats | wave cell | frontier wave, as the host form sends them

    // Fisher information along the planned paths (fs_pathinfo.hip)
    bool opt_pi_dedup = true;         // "pathinfo.dedup": one pose record per distinct (from cell, to cell) (0: one per way point)
    int64_t pi_waypoints = 0, pi_distinct = 0;      // way points of the last call, pose records it scored
    DevBuf<int32_t> d_pi_off;         // count [n + 1] | offset [n + 1]
    DevBuf<uint64_t> d_pi_key;        // [2][bound]
    DevBuf<int32_t> d_pi_idx;         // [5][bound]: way point in / out of the sort, head, rank, slot
    DevBuf<float> d_pi_rt;            // [bound][12]
    DevBuf<double> d_pi_pose;         // [bound][7] (dump)
    DevBuf<float> d_pi_val;           // [bound] (dump)
    DevBuf<char> d_pi_temp, d_pi_out; // rocPRIM's scratch;  hdr [2] | info_mean | info_min | first_unsafe | n_waypoints
    PinnedBuf h_pi_out;

    // frontier roadmap (fs_roadmap.hip).  The host keeps FrontierRoadMap's two containers — the spatial hash (cell ->
    // node ids in insertion order) and roadmap_ (a key flag and an adjacency list in append order per node) — and the device a copy
    // of them as CSR.  Every mutation bumps rm_gen; the device copy, its transpose and the shortest-path tree (kept per root node)
    // are valid for the generation they were made for.
    double rm_cell = 1.0, rm_radius = 6.1, rm_min_frontier = 0.25, rm_min_robot = 0.25;
    std::vector<double> rm_xy;
    std::map<std::pair<int, int>, std::vector<int32_t>> rm_hash;
    std::vector<uint8_t> rm_key;
    std::vector<std::vector<int32_t>> rm_adj;
    uint64_t rm_gen = 1, rm_dev_gen = 0, rm_t_gen = 0, rm_tree_gen = 0;
    int32_t rm_tree_root = -1, rm_tree_buf = 0;
    int64_t rm_tree_builds = 0, rm_tree_rounds = 0, rm_traced = 0;
    DevBuf<double> d_rm_xy, d_rm_d;
    DevBuf<uint8_t> d_rm_key;
    DevBuf<uint64_t> d_rm_cell_key;
    DevBuf<int32_t> d_rm_row, d_rm_col, d_rm_trow, d_rm_tcol, d_rm_tmp, d_rm_cell_start, d_rm_cell_nodes, d_rm_cand_off, d_rm_cand;
    DevBuf<int32_t> d_rm_hops, d_rm_pred, d_rm_word;
    DevBuf<char> d_rm_in, d_rm_out;   // goals | headings | modes;  path length | length in m | heading | achievable
    PinnedBuf h_rm_in, h_rm_out;
    // the REFERENCE roadmap search (fs_set_roadmap_search): per-goal A* queries (fs_roadmap_astar.h).  The plan's goal node of every
    // frontier, the goal-node marks and their scan (query indices), the query list, results and stats; the global route's pool;
    // h_as_io holds the stats read back and the next-goal search's query list.  as_args / as_plan: the last call's launches, which
    // rm_astar_settle repeats on a grown pool.
    int32_t rm_search = FS_ROADMAP_SEARCH_TREE;
    int32_t astar_lds_entries = 2048;         // "roadmap.astar_lds_entries": records of a query in LDS (0: the global route only)
    int32_t astar_cap = 16384;                // records of a query on the global route (grows when one outgrows it)
    int64_t as_queries = 0, as_max_pops = 0, as_global = 0;
    DevBuf<int32_t> d_as_gnode, d_as_mark, d_as_qidx, d_as_src, d_as_dst, d_as_status, d_as_stats;
    DevBuf<double> d_as_len;
    DevBuf<char> d_as_pool;
    PinnedBuf h_as_io;
    FsRmAstarArgs as_args{};
    FsRmPlanArgs as_plan{};
    // roadmap routes (fs_roadmap_routes).  rt_chains: the plan in flight is that call's, so the A* queries also emit
    // their node chains into d_rt_pool (rt_pool_cap slots in use; "routes.pool_nodes" sets it, a call that overflows it grows it to
    // what it needed and runs the queries again).  rt_plan / rt_max_q: the plan's arguments and query bound, for the launches that
    // follow it.
    bool opt_rt_dedup = true;                 // "routes.dedup": one pose record per distinct (from node, to node) (0: one per leg)
    bool rt_chains = false;
    int64_t rt_pool_cap = 1 << 16;
    int64_t rt_routes = 0, rt_walks = 0, rt_poses = 0, rt_retries = 0;     // counters 1026-1029
    FsRmPlanArgs rt_plan{};
    int32_t rt_max_q = 0;
    DevBuf<int32_t> d_rt_chain_len, d_rt_pool, d_rt_idx, d_rt_of, d_rt_node, d_rt_refined;
    DevBuf<int64_t> d_rt_chain_base, d_rt_off;
    DevBuf<unsigned long long> d_rt_cursor;   // [2]: the chain pool's cursor, the refinement's walks
    DevBuf<uint8_t> d_rt_complete;
    PinnedBuf h_rt, h_rt_list;
    // next goal (fs_roadmap_next_goal): a batch of trees with buffers of its own (the single tree above stays
    // cached), the pair matrix, the tour search's winners
    int32_t tour_one_wg = RM_TREE_ONE_WG;     // "roadmap.tour_one_wg": above this many nodes the batch runs a round per launch
    int64_t tour_tree_builds = 0, tour_tree_rounds = 0, tour_evaluated = 0;
    DevBuf<double> d_tour_d;
    DevBuf<int32_t> d_tour_hops, d_tour_pred, d_tour_word;
    DevBuf<char> d_tour_work;                 // matrix | result | block winners
    PinnedBuf h_tour_out;                     // matrix | result | rounds of each tree
    // key-frame anchors of the roadmap (fs_roadmap_kf.hip).  kf_order is keyframe_mapping_'s shadow: its keys are
    // inserted in the sequence the reference inserts them, so iterating it is iterating keyframe_mapping_.  Records live on the
    // device: (handle, p_c float3, ordinal in its key frame's vector), appended in time order.
    std::vector<double> kf_queue;                       // no_kf_parent_queue_: pending node positions [k][2], FIFO
    std::unordered_map<int32_t, int32_t> kf_handle;     // id -> handle (every id a message has named)
    std::vector<int32_t> kf_handle_id;                  // handle -> id
    std::vector<int64_t> kf_handle_count;               // handle -> records (the length of keyframe_mapping_[id])
    std::unordered_map<int32_t, int32_t> kf_order;      // id -> handle, in keyframe_mapping_'s insertion sequence
    std::vector<int32_t> kf_slot;                       // handle -> slot of the latest message (-1: not in it)
    int64_t kf_records = 0;
    int32_t kf_one_wg = FS_KF_DEDUP_ONE_WG;             // "roadmap.dedup_one_wg": above this many points a round per launch
    int64_t kf_rounds = 0, kf_points = 0;               // counters 1017 / 1018 (1016: kf_records)
    DevBuf<float> d_kf_rt, d_kf_rec_p, d_kf_pts, d_kf_out;
    DevBuf<double> d_kf_queue;
    DevBuf<int32_t> d_kf_rec_h, d_kf_rec_ord, d_kf_tab, d_kf_work, d_kf_cand, d_kf_word;
    DevBuf<uint64_t> d_kf_cell_key, d_kf_hkey;
    DevBuf<uint8_t> d_kf_state;
    PinnedBuf h_kf;
    // the per-tick update (fs_roadmap_update.hip): the extended node list and key flags, the points, the work arrays
    // of FsRmUpdate, the result (header | kept positions | key flags | pairs) as the host reads it
    int64_t ru_walks = 0, ru_owners = 0, ru_rounds = 0;     // the last update's walks, owners and keep rounds (counters 1033-1035)
    DevBuf<double> d_ru_xy, d_ru_pts;
    DevBuf<uint8_t> d_ru_key, d_ru_rejected;
    DevBuf<uint64_t> d_ru_conf;
    DevBuf<int32_t> d_ru_work, d_ru_rank_of, d_ru_cand;
    PinnedBuf h_ru;

    // any-angle leg refinement (fs_refine.hip): a slab of rf_max_fields fp64 fields; slot s holds the field of
    // rf_key[s] for grid generation rf_gen[s] (0: empty).  Every staging call that writes the grid bumps grid_gen, which drops them.
    struct RfKey {
        int32_t src = -1, allow = 0, corners = 0;
        double w_euc = 0.0, w_trav = 0.0;
        bool operator==(const RfKey &o) const { return src == o.src && allow == o.allow && corners == o.corners && w_euc == o.w_euc && w_trav == o.w_trav; }
    };
    int32_t rf_max_fields = 16;               // "refine.max_fields": fields relaxed together / kept
    std::vector<RfKey> rf_key;
    std::vector<uint64_t> rf_gen;
    size_t rf_slab_cells = 0;                 // nx * ny the slab was laid out for
    int64_t rf_builds = 0, rf_rounds = 0, rf_walks = 0;
    int64_t rf_chain_cap = 0;
    int32_t rf_vert_cap = 0, rf_pose_cap = 0;
    DevBuf<double> d_rf_g;
    DevBuf<uint32_t> d_rf_flags;              // [2][fields][tiles]
    DevBuf<int32_t> d_rf_any, d_rf_in, d_rf_scratch;   // rounds x fields words | legs' inputs | chain, parents, vertex cells
    DevBuf<char> d_rf_out, d_rf_pts;          // per-leg columns | vertex and pose slots (when the page-locked buffer is not mapped)
    PinnedBuf h_rf_in, h_rf_out, h_rf_pts;
    // the REFERENCE refine search (fs_set_refine_search): the reference's Theta* search per distinct (start cell, goal cell)
    // (fs_thetastar.h), in batches of slots; nothing is kept across calls but the hypot table of the grid's shape
    int32_t rf_search = FS_REFINE_SEARCH_FIELD;
    int32_t rs_opt_slots = 0;                 // "refine.search_slots": 0 = as many as "refine.search_bytes" holds
    int64_t rs_opt_bytes = (int64_t)1 << 30;  // "refine.search_bytes"
    int64_t rs_searches = 0, rs_batches = 0, rs_pops = 0, rs_walks = 0, rs_max_heap = 0;   // counters 1042-1046, of the last call
    int32_t rs_vtx_cap = 256;
    int32_t rs_hyp_nx = 0, rs_hyp_ny = 0;     // the shape d_rs_hyp was filled for
    DevBuf<double> d_rs_hyp;          // [nx][ny] std::hypot of cell differences, by this host's libm
    DevBuf<char> d_rs_slab;           // [slots][slot bytes]
    DevBuf<char> d_rs_io;             // search cells | per-search columns | vertex cells (RsLayout)
    PinnedBuf h_rs_io;

    // task allocation (fs_allocate.hip).  d_al_work: the working copy | MinPos' matrix | MinPos' P; d_al_out: the
    // packed result (AllocOut); d_al_stats: status and counters 1030-1032 of the last solve (read when fs_get_counter asks).
    // The fleet call keeps its trees, plans and matrix in buffers of its own: the single-robot tree cache and d_rm_out stay as
    // fs_roadmap_plan left them.
    DevBuf<char> d_al_in, d_al_work, d_al_out;
    DevBuf<int32_t> d_al_stats;
    PinnedBuf h_al_in, h_al_out;
    DevBuf<double> d_fl_d;
    DevBuf<int32_t> d_fl_hops, d_fl_pred, d_fl_word;
    DevBuf<char> d_fl_in, d_fl_plan, d_fl_out;   // the staged inputs;  path length | heading, [R][n] each;  the packed results
    PinnedBuf h_fl_in, h_fl_out;

    // timing
    bool timing = false;
    std::vector<TimedLaunch> launches;
    std::vector<hipEvent_t> event_pool;
};

namespace {

int fail(fs_ctx *c, int code, const char *fmt, ...)
{
    if (c) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        c->err = buf;
    }
    return code;
}

#define FS_HIP(c, call)                                                                          \
    do {                                                                                         \
        hipError_t e__ = (call);                                                                 \
        if (e__ != hipSuccess) return fail((c), FS_E_HIP, "%s: %s", #call, hipGetErrorString(e__)); \
    } while (0)

// ---------------------------------------------------------------- launch graphs for the small host-buffer calls
// The reference scores tens of frontiers per behaviour-tree tick and ONE pose per isPoseSafe: such a call is a dozen launches of
// nearly empty kernels, and what it costs is launch latency.  `enqueue` puts the call's whole device-side sequence — one
// transfer in, the kernels, one transfer out; fixed sizes, fixed pointers, no allocation, no synchronisation — on the context's
// stream.  The first call in a given state runs it plainly (and makes every allocation it needs), the second captures it into a
// hipGraph, every later one replays the graph with ONE launch.  Any staging or parameter call (epoch) and any reallocation
// (fs_alloc_generation) sends the sequence through that cycle again; a capture that fails leaves it on plain launches.
// MEASURED (profiles/r04/small_call_graphs.json, alternating runs in one session): the replay costs 5-7 us MORE per call than the
// six plain launches it replaces (REF2D, one frontier: 61.0 -> 66.7 us; 50 frontiers: 86.5 -> 92.5 us) — hipGraphLaunch is the
// expensive launch on this runtime.  The "graph" option is therefore OFF by default; the path stays, tested, for runtimes
// where that changes.
#define FS_GRAPH_MAX_N 1024      // candidates per graphed call: buckets of 2^k up to here (below the spatial sort's threshold)

template <typename F>
int run_maybe_graphed(fs_ctx *c, uint64_t key, F enqueue)
{
    if (!c->opt_graph || c->timing) return enqueue();
    if (c->graphs.size() > 256) {                              // (a caller that varies the parameters baked into a key without end)
        for (auto &g : c->graphs) if (g.second.exec) (void)hipGraphExecDestroy(g.second.exec);
        c->graphs.clear();
    }
    GraphEntry &g = c->graphs[key];
    const uint64_t stamp = (c->epoch << 32) ^ fs_alloc_generation;
    if (g.broken) return enqueue();
    if (g.exec && g.stamp == stamp) {
        if (hipGraphLaunch(g.exec, c->stream) == hipSuccess) return FS_OK;
        g.broken = true;
        return enqueue();
    }
    if (g.exec) { (void)hipGraphExecDestroy(g.exec); g.exec = nullptr; }
    if (g.warm_stamp != stamp) {
        const int rc = enqueue();                              // plain: allocations, lazily cut images, attribute calls happen here
        g.warm_stamp = (c->epoch << 32) ^ fs_alloc_generation;
        return rc;
    }
    hipGraph_t graph = nullptr;
    if (hipStreamBeginCapture(c->stream, hipStreamCaptureModeRelaxed) != hipSuccess) { g.broken = true; return enqueue(); }
    const int rc = enqueue();
    const hipError_t e_end = hipStreamEndCapture(c->stream, &graph);
    const bool same_state = ((c->epoch << 32) ^ fs_alloc_generation) == stamp;
    if (rc != FS_OK || e_end != hipSuccess || !graph || !same_state ||
        hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0) != hipSuccess) {
        if (graph) (void)hipGraphDestroy(graph);
        g.exec = nullptr; g.broken = true;
        (void)hipGetLastError();
        return rc != FS_OK ? rc : enqueue();                   // nothing has run yet: the capture only recorded
    }
    (void)hipGraphDestroy(graph);
    g.stamp = stamp;
    if (hipGraphLaunch(g.exec, c->stream) != hipSuccess) { g.broken = true; return enqueue(); }
    return FS_OK;
}

int graph_bucket(int32_t n)
{
    int b = 1;
    while (b < n) b <<= 1;
    return b;
}

double std_min(double a, double b) { return (b < a) ? b : a; }
double std_max(double a, double b) { return (a < b) ? b : a; }

hipEvent_t get_event(fs_ctx *c)
{
    if (!c->event_pool.empty()) {
        hipEvent_t e = c->event_pool.back();
        c->event_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

struct ScopedTimer {
    fs_ctx *c;
    TimedLaunch t{};
    bool on;
    hipStream_t s;
    ScopedTimer(fs_ctx *ctx, int kind, hipStream_t stream = nullptr) : c(ctx), on(ctx->timing), s(stream ? stream : ctx->stream)
    {
        if (!on) return;
        t.kind = kind;
        t.start = get_event(c);
        t.stop = get_event(c);
        (void)hipEventRecord(t.start, s);
    }
    ~ScopedTimer()
    {
        if (!on) return;
        (void)hipEventRecord(t.stop, s);
        c->launches.push_back(t);
    }
};

// ---------------------------------------------------------------- planner host helpers
// The planners' relaxations (the NavFn field, the roadmap and tour trees, the anchor de-duplication, the refine fields) are
// deterministic Jacobi rounds: a round after a quiet round is quiet too.  Rounds are therefore launched in batches without a host
// synchronisation in between, and a batch that overshoots the last round costs launches, never a different result.
#define PLAN_BATCH_FIRST 8
#define PLAN_BATCH 16
#define PLAN_MAX_ROUNDS (1 << 22)

// Polls `cols` relaxations that run in lockstep: `launch(r0, count)` enqueues rounds r0 .. r0 + count - 1, round k of the batch
// writing its "something changed" words at words + k * cols (cleared here before every batch; words holds
// max(first, batch) * cols).  A column's last round is the first quiet one; the call ends once every column has one.  After a
// batch that leaves a column unsettled, "rounds launched >= limit" fails as "<what> did not settle in <shown> rounds".
// rounds[f]: the rounds of column f, the quiet one included.
template <class Launch>
int poll_rounds(fs_ctx *c, int32_t *words, int first, int batch, int cols, int64_t limit, const char *what, int64_t shown,
                Launch launch, int64_t *rounds)
{
    std::vector<int32_t> any((size_t)std::max(first, batch) * cols);
    std::fill(rounds, rounds + cols, -1);
    int64_t r = 0;
    for (int count = first;; count = batch) {
        FS_HIP(c, hipMemsetAsync(words, 0, sizeof(int32_t) * count * cols, c->stream));
        const int rc = launch(r, count);
        if (rc) return rc;
        r += count;
        FS_HIP(c, hipMemcpyAsync(any.data(), words, sizeof(int32_t) * count * cols, hipMemcpyDeviceToHost, c->stream));
        FS_HIP(c, hipStreamSynchronize(c->stream));
        bool done = true;
        for (int f = 0; f < cols; ++f) {
            if (rounds[f] >= 0) continue;
            int k = 0;
            while (k < count && any[(size_t)k * cols + f]) ++k;
            if (k < count) rounds[f] = r - count + k + 1;           // the first quiet round of the batch
            else done = false;
        }
        if (done) break;
        if (r >= limit) return fail(c, FS_E_HIP, "%s did not settle in %lld rounds", what, (long long)shown);
    }
    return FS_OK;
}

// Costmap2D::worldToMap on the staged grid
bool grid_world_to_map(const fs_ctx *c, double wx, double wy, int32_t &mx, int32_t &my)
{
    if (wx < c->origin[0] || wy < c->origin[1]) return false;
    const double qx = (wx - c->origin[0]) / c->res, qy = (wy - c->origin[1]) / c->res;
    if (!(qx < 4294967296.0) || !(qy < 4294967296.0)) return false;
    const unsigned ux = static_cast<unsigned>(qx), uy = static_cast<unsigned>(qy);
    if (ux >= (unsigned)c->nx || uy >= (unsigned)c->ny) return false;
    mx = (int32_t)ux; my = (int32_t)uy;
    return true;
}

// The device bound and a grid staged: what every call on the staged map needs first
int grid_check(fs_ctx *c)
{
    FS_HIP(c, hipSetDevice(c->device));
    if (!c->have_grid) return fail(c, FS_E_STATE, "fs_upload_grid has not been called");
    return FS_OK;
}

// ... and that grid 2-D: what every planner stage needs (`what` names the stage in the error)
int grid2d_check(fs_ctx *c, const char *what)
{
    if (const int rc = grid_check(c)) return rc;
    if (c->nz != 1) return fail(c, FS_E_INVALID, "%s is defined on a 2-D costmap (nz == 1)", what);
    return FS_OK;
}

// fs_frontier_clusters' kernels (fs_launch_frontier_clusters), shared with the frontier search: every buffer they use, then the
// launch from the robot's cell.  `labels`: the label image is written too; max_clusters: room for cluster records (0: none).
int fc_ensure(fs_ctx *c, bool labels, int32_t max_clusters)
{
    const size_t cells = (size_t)c->nx * c->ny;
    FS_HIP(c, c->d_fc_parent_t.ensure(cells)); FS_HIP(c, c->d_fc_parent_f.ensure(cells)); FS_HIP(c, c->d_fc_aux.ensure(cells));
    FS_HIP(c, c->d_fc_queue.ensure(cells)); FS_HIP(c, c->d_fc_visited.ensure(cells)); FS_HIP(c, c->d_fc_state.ensure(8));
    if (labels) FS_HIP(c, c->d_fc_labels.ensure(cells));
    FS_HIP(c, c->d_fc_clusters.ensure((size_t)std::max(max_clusters, 1))); FS_HIP(c, c->d_fc_sums.ensure(2 * (size_t)std::max(max_clusters, 1)));
    return FS_OK;
}

int fc_launch(fs_ctx *c, const double robot_xy[2], int32_t robot_cell, double max_frontier_distance, int32_t max_frontier_cluster_size,
              int32_t lethal_threshold, bool labels, int32_t max_clusters)
{
    const double reach = max_frontier_distance + (max_frontier_cluster_size * c->res * 1.414);      // DEP/src/FrontierSearch.cpp:67
    ScopedTimer t(c, 5);
    FS_HIP(c, fs_launch_frontier_clusters(c->d_cells.p, c->nx, c->ny, c->origin[0], c->origin[1], c->res, robot_xy[0], robot_xy[1],
                                          robot_cell, reach, lethal_threshold, c->d_fc_parent_t.p, c->d_fc_parent_f.p, c->d_fc_aux.p,
                                          c->d_fc_queue.p, c->d_fc_visited.p, c->d_fc_state.p, labels ? c->d_fc_labels.p : nullptr,
                                          max_clusters, c->d_fc_clusters.p, c->d_fc_sums.p, c->stream));
    return FS_OK;
}

// Output block of a planner's path columns (d_nav_out, d_rm_out and their host copies): path length | length in m | heading |
// achievable.
struct PlanOutLayout {
    size_t len, len_m, head, ach, total;
    explicit PlanOutLayout(size_t n) : len(0), len_m(8 * n), head(16 * n), ach(24 * n), total(24 * n + ((n + 15) & ~(size_t)15)) {}
};

// ... from their host copy (the stream has drained) into the caller's four arrays
void plan_columns_to_caller(const PinnedBuf &h_out, size_t n, double *path_length, double *path_length_m, double *path_heading, uint8_t *achievable)
{
    const PlanOutLayout O(n);
    std::memcpy(path_length, h_out.p + O.len, 8 * n);
    std::memcpy(path_length_m, h_out.p + O.len_m, 8 * n);
    std::memcpy(path_heading, h_out.p + O.head, 8 * n);
    std::memcpy(achievable, h_out.p + O.ach, n);
}

// Output block of fs_plan_paths_information in d_pi_out / h_pi_out: total, records | info_mean | info_min | first_unsafe
struct PathInfoOutLayout {
    size_t hdr, mean, min, unsafe, total;
    explicit PathInfoOutLayout(size_t n) : hdr(0), mean(16), min(16 + 8 * n), unsafe(16 + 12 * n), total(16 + 16 * n) {}
};
#define PI_BOUND_DIRECT (1 << 19)     // way points the call makes room for before it knows how many there are

// ---------------------------------------------------------------- lookup-table math (host, float32)
// FIP/src/fisher_information/FisherInformationHelpers.cpp:71-96,114-123 with Q = I.
float information_of_point_local(const float p[3])
{
    const float n = std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
    const float inv_n = 1 / n, inv_n3 = 1 / (n * n * n);
    float dfdp[3][3], right[3][6], jac[3][6];
    for (int r = 0; r < 3; ++r)
        for (int col = 0; col < 3; ++col) dfdp[r][col] = inv_n * (r == col ? 1.0f : 0.0f) - (inv_n3 * p[r]) * p[col];
    const float skew[3][3] = {{0, -p[2], p[1]}, {p[2], 0, -p[0]}, {-p[1], p[0], 0}};
    for (int r = 0; r < 3; ++r)
        for (int col = 0; col < 3; ++col) {
            right[r][col] = (float)(-1.0) * (r == col ? 1.0f : 0.0f);
            right[r][col + 3] = skew[r][col];
        }
    for (int r = 0; r < 3; ++r)
        for (int col = 0; col < 6; ++col) {
            float acc = 0.0f;
            for (int k = 0; k < 3; ++k) acc += dfdp[r][k] * right[k][col];
            jac[r][col] = acc;
        }
    float trace = 0.0f;
    for (int col = 0; col < 6; ++col) {
        float acc = 0.0f;
        for (int k = 0; k < 3; ++k) acc += jac[k][col] * jac[k][col];
        trace += acc;
    }
    return trace;
}

const float kStepMin = 0.09f, kStepMax = 0.3f, kSubSampleUntil = -1.0f;   // FisherInfoManager.hpp:25-30

// FisherInfoManager.hpp:108-123
void voxel_coordinate(float x, float y, float z, float key[3], long lattice[3])
{
    double step;
    if (std::fabs(x) < kSubSampleUntil && std::fabs(y) < kSubSampleUntil && std::fabs(z) < kSubSampleUntil) step = kStepMin;
    else step = kStepMax;
    const double r[3] = {std::round(x * (1 / step)), std::round(y * (1 / step)), std::round(z * (1 / step))};
    for (int i = 0; i < 3; ++i) {
        key[i] = (float)(r[i] * step);
        if (lattice) lattice[i] = (long)r[i];
    }
}

struct KeyBits {
    uint32_t b[3];
    bool operator==(const KeyBits &o) const { return b[0] == o.b[0] && b[1] == o.b[1] && b[2] == o.b[2]; }
};
struct KeyBitsHash {
    size_t operator()(const KeyBits &k) const
    {
        size_t h = 0;
        for (uint32_t v : k.b) h ^= std::hash<uint32_t>{}(v) + 0x9e3779b9 + (h << 6) + (h >> 2);
        return h;
    }
};
KeyBits key_bits(const float k[3])
{
    KeyBits out;
    for (int i = 0; i < 3; ++i) {
        float f = (k[i] == 0.0f) ? 0.0f : k[i];     // -0 == +0 under float equality
        std::memcpy(&out.b[i], &f, 4);
    }
    return out;
}

// FisherInfoManager.cpp:117-229 — produces the file's record sequence.
void generate_records(float minX, float maxX, float minY, float maxY, float minZ, float maxZ, std::vector<float> &rec)
{
    rec.clear();
    float max_fi = -std::numeric_limits<float>::max();
    minX = std::floor(minX * (1 / kStepMax)) * kStepMax;
    minY = std::floor(minY * (1 / kStepMax)) * kStepMax;
    minZ = std::floor(minZ * (1 / kStepMax)) * kStepMax;
    maxX = std::ceil(maxX * (1 / kStepMax)) * kStepMax;
    maxY = std::ceil(maxY * (1 / kStepMax)) * kStepMax;
    maxZ = std::ceil(maxZ * (1 / kStepMax)) * kStepMax;
    std::unordered_set<KeyBits, KeyBitsHash> existing;
    float inc = kStepMin;
    for (float cx = minX; cx <= maxX; cx += inc) {
        if (cx > kSubSampleUntil + kStepMax) inc = kStepMax;
        for (float cy = minY; cy <= maxY; cy += inc) {
            for (float cz = minZ; cz <= maxZ; cz += inc) {
                float key[3];
                voxel_coordinate(cx, cy, cz, key, nullptr);
                if (!existing.insert(key_bits(key)).second) continue;
                const float value = information_of_point_local(key);
                if (std::isnan(value)) continue;
                max_fi = std::max(max_fi, value);
                rec.insert(rec.end(), {key[0], key[1], key[2], value});
            }
        }
    }
    rec.insert(rec.end(), {0.0f, 0.0f, 0.0f, max_fi});
}

// The FIM worker's pass prediction learns the cloud's voxels-per-landmark ratio from finished calls (counters[12], fs_fim.hip);
// what it learnt holds for one cloud, one table and one visibility volume.
static void reset_voxel_ratio(fs_ctx *c)
{
    if (!c->d_counters.p) return;
    (void)hipSetDevice(c->device);                         // (callers on the table path have not bound the device yet)
    (void)hipMemsetAsync(c->d_counters.p + 12, 0, 2 * sizeof(unsigned long long), c->stream);   // both ratios (FsFimArgs::ratio_slot)
}

// Dense re-indexing of the record list by the integer voxel lattice (what loadLookupTable's
// unordered_map resolves to: later duplicates overwrite, FisherInfoManager.cpp:245-251).
int build_dense(fs_ctx *c)
{
    reset_voxel_ratio(c);
    const int64_t n = (int64_t)c->records.size() / 4;
    if (n <= 0) return fail(c, FS_E_INVALID, "lookup table has no records");
    const double step = (double)kStepMax, inv = 1 / step;
    long lo[3] = {LONG_MAX, LONG_MAX, LONG_MAX}, hi[3] = {LONG_MIN, LONG_MIN, LONG_MIN};
    std::vector<long> lat((size_t)n * 3);
    for (int64_t i = 0; i < n; ++i) {
        const float *r = &c->records[4 * i];
        for (int a = 0; a < 3; ++a) {
            const long j = std::lround((double)r[a] * inv);
            const float back = (float)((double)j * step);
            if (!(back == r[a])) return fail(c, FS_E_INVALID, "lookup record %lld is off the 0.3 m voxel lattice", (long long)i);
            lat[3 * i + a] = j;
            lo[a] = std::min(lo[a], j);
            hi[a] = std::max(hi[a], j);
        }
    }
    const int64_t dx = hi[0] - lo[0] + 1, dy = hi[1] - lo[1] + 1, dz = hi[2] - lo[2] + 1;
    if (dx * dy * dz > (int64_t)FS_MAX_TABLE_CELLS) return fail(c, FS_E_INVALID, "lookup table lattice too large (%lld cells)", (long long)(dx * dy * dz));
    c->jx0 = (int32_t)lo[0]; c->jy0 = (int32_t)lo[1]; c->jz0 = (int32_t)lo[2];
    c->tx = (int32_t)dx; c->ty = (int32_t)dy; c->tz = (int32_t)dz;
    c->dense.assign((size_t)(dx * dy * dz), std::numeric_limits<float>::quiet_NaN());
    for (int64_t i = 0; i < n; ++i) {
        const size_t idx = ((size_t)(lat[3 * i] - lo[0]) * dy + (size_t)(lat[3 * i + 1] - lo[1])) * dz + (size_t)(lat[3 * i + 2] - lo[2]);
        c->dense[idx] = c->records[4 * i + 3];
    }
    c->table_full = true;
    for (float v : c->dense) if (!std::isfinite(v)) { c->table_full = false; break; }   // (NaN = absent; an infinite value also takes the guarded kernel)
    FS_HIP(c, c->d_table.ensure(c->dense.size()));
    FS_HIP(c, hipMemcpyAsync(c->d_table.p, c->dense.data(), c->dense.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (!c->have_factor) {
        // getFactorFromNum(num, 0.8f) — FisherInfoManager.hpp:102-106 (pow/exp in double, float return)
        std::vector<float> fac(FS_FACTOR_N, 0.0f);
        const float s = 0.8f;
        for (int k = 1; k < FS_FACTOR_N; ++k) fac[k] = (float)std::exp(1 - std::pow((double)k, (double)s));
        for (int k = 1; k <= 4; ++k) c->fac[k] = fac[k];
        FS_HIP(c, c->d_factor.ensure(fac.size()));
        FS_HIP(c, hipMemcpyAsync(c->d_factor.p, fac.data(), fac.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
        FS_HIP(c, hipStreamSynchronize(c->stream));
        c->have_factor = true;
    }
    FS_HIP(c, hipStreamSynchronize(c->stream));
    c->have_table = true;
    ++c->epoch;
    return FS_OK;
}

// getTransformFromPose (FisherInformationHelpers.cpp:16-26): float translation, Eigen::Quaternionf -> rotation.
void pose_to_rt(const double pose7[7], float Rt[12])
{
    const float x = (float)pose7[3], y = (float)pose7[4], z = (float)pose7[5], w = (float)pose7[6];
    const float tx = 2.0f * x, ty = 2.0f * y, tz = 2.0f * z;
    const float twx = tx * w, twy = ty * w, twz = tz * w;
    const float txx = tx * x, txy = ty * x, txz = tz * x;
    const float tyy = ty * y, tyz = tz * y, tzz = tz * z;
    Rt[0] = 1.0f - (tyy + tzz); Rt[1] = txy - twz;          Rt[2] = txz + twy;
    Rt[3] = txy + twz;          Rt[4] = 1.0f - (txx + tzz); Rt[5] = tyz - twx;
    Rt[6] = txz - twy;          Rt[7] = tyz + twx;          Rt[8] = 1.0f - (txx + tyy);
    Rt[9] = (float)pose7[0]; Rt[10] = (float)pose7[1]; Rt[11] = (float)pose7[2];
}

// The poses of a visibility call: pose7[n] into Rt[n][12].  False when a quaternion is off unit norm: chunk culling reasons in
// world space and needs R orthonormal, so such a call (the reference would feed the quaternion to Eigen unnormalised) takes
// the brute-force scan.
bool poses_to_rt(const double *pose7, int32_t n, float *Rt)
{
    bool unit = true;
    for (int32_t i = 0; i < n; ++i) {
        const double *q = pose7 + 7 * (size_t)i + 3;
        const double nq = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
        if (!(std::fabs(nq - 1.0) <= 1.0e-4)) unit = false;
        pose_to_rt(pose7 + 7 * (size_t)i, Rt + 12 * (size_t)i);
    }
    return unit;
}

// Cells at the far end of a line-of-sight walk that are not tested, M = 1 + (unsigned)(margin / resolution); a walk has fewer than
// 2^31 visits, so a larger quotient tests nothing either way
uint32_t occlusion_margin(const fs_ctx *c, double end_margin_m)
{
    const double q = end_margin_m / c->res;
    return 1u + (q < 2147483647.0 ? (uint32_t)q : 2147483647u);
}

// Landmark chunks per wave of a visibility scan over `items` poses: a single pose is the reference's real call, so fewer chunks
// per wave until the launch fills the chip's wave slots
int32_t chunks_per_wave(int64_t items, int32_t n_chunks)
{
    int32_t group = 64;
    while (group > 4 && items * ((n_chunks + group - 1) / group) < 2048) group >>= 1;
    return group;
}

// Which image of the grid the arrival fan walks.  The class walk spends ~1.3x the instructions per step and touches 4-8x fewer
// cache lines (L2 -> L1 fill 4.4 GB -> 0.5 GB per C3 launch).  Measured (profiles/r03/ray_class_walk.json): on 3-D grids it wins
// at every ray length (C3: 0.190 against 0.229 ms at 40 cells, 0.63 against 1.12 ms at 160); on a 2-D costmap a short fan lives
// in L1 either way and the byte walk's cheaper set-up wins (REF2D: 0.059 against 0.073 ms) until the rays get long.
// "ray.layout" forces one.
#ifndef FS_CLASS_WALK_FROM
#define FS_CLASS_WALK_FROM 96.0
#endif
bool use_class_walk(const fs_ctx *c, double max_length_cells)
{
    // (the walk forms brick addresses with 24-bit multiplies: the largest brick stride, 512 * bricks_x * bricks_y, must fit)
    const uint64_t stride = 512ull * (uint64_t)((c->nx + 7) >> 3) * (uint64_t)((c->ny + 7) >> 3);
    // (... and it forms the cell address A in 32 bits: a grid thin in x / y and deep in z can pass the 2^31-cell limit and still
    // pad to 2^32 class cells or more — 4 x 4 x 2^26 does; such a grid keeps the byte walk)
    const uint64_t padded_cells = stride * (uint64_t)((c->nz + 7) >> 3);
    if (c->opt_layout == 1 || stride >= (1ull << 24) || padded_cells >= (1ull << 32)) return false;
    if (c->opt_layout >= 2) return true;
    return c->nz > 1 || max_length_cells >= FS_CLASS_WALK_FROM;
}

FsGridDev grid_dev(const fs_ctx *c)
{
    const uint32_t bx = (uint32_t)(c->nx + 7) >> 3, by = (uint32_t)(c->ny + 7) >> 3, bz = (uint32_t)(c->nz + 7) >> 3;
    return FsGridDev{c->d_cells.p, c->nx, c->ny, c->nz, c->origin[0], c->origin[1], c->origin[2], c->res, c->d_counters.p + 29,
                     c->have_cls ? c->d_cls.p : nullptr, {512u - 8u, 512u * bx - 64u, 512u * bx * by - 512u}, 512u * bx * by * bz, nullptr};
}

// the ground-truth world, which is of the staged grid's shape and has no class image
FsGridDev world_dev(const fs_ctx *c)
{
    FsGridDev w = grid_dev(c);
    w.cells = c->d_world.p;
    w.cls = nullptr;
    return w;
}

// every upload path ends here: images derived from the grid are cut again on next use
int retile_grid(fs_ctx *c, int32_t, int32_t, int32_t)
{
    c->have_cls = false;
    c->have_sparse = false;
    return FS_OK;
}

// The sparse form of the class image: the dense one (already cut on the device) is read back, every brick whose 512 cells are
// of ONE class points at the shared uniform brick of that class (pool slots 0..3), every other brick gets a slot of its own.
// A staging-time pass on the host — this is the experiment's set-up, not a path anybody waits for per tick.
int build_sparse_class_image(fs_ctx *c)
{
    const uint64_t bricks = (uint64_t)((c->nx + 7) >> 3) * (uint64_t)((c->ny + 7) >> 3) * (uint64_t)((c->nz + 7) >> 3);
    std::vector<uint32_t> dense(bricks * 32), table(bricks), pool;
    FS_HIP(c, hipMemcpyAsync(dense.data(), c->d_cls.p, dense.size() * 4, hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipStreamSynchronize(c->stream));
    static const uint32_t uniform[4] = {0x00000000u, 0x55555555u, 0xAAAAAAAAu, 0xFFFFFFFFu};
    pool.reserve(4 * 32 + (size_t)(bricks / 2) * 32);
    for (int k = 0; k < 4; ++k) pool.insert(pool.end(), 32, uniform[k]);
    for (uint64_t b = 0; b < bricks; ++b) {
        const uint32_t *w = &dense[b * 32];
        bool same = true;
        for (int i = 1; i < 32 && same; ++i) same = w[i] == w[0];
        int k = -1;
        if (same) for (int u = 0; u < 4; ++u) if (w[0] == uniform[u]) k = u;
        if (k >= 0) { table[b] = (uint32_t)k; continue; }
        table[b] = (uint32_t)(pool.size() / 32);
        pool.insert(pool.end(), w, w + 32);
    }
    if (pool.size() / 32 >= (1ull << 23)) return fail(c, FS_E_INVALID, "sparse class image: more than 2^23 distinct bricks");   // (slot << 9 must stay in 32 bits)
    FS_HIP(c, c->d_cls_table.ensure(table.size())); FS_HIP(c, c->d_cls_pool.ensure(pool.size()));
    FS_HIP(c, hipMemcpyAsync(c->d_cls_table.p, table.data(), table.size() * 4, hipMemcpyHostToDevice, c->stream));
    FS_HIP(c, hipMemcpyAsync(c->d_cls_pool.p, pool.data(), pool.size() * 4, hipMemcpyHostToDevice, c->stream));
    FS_HIP(c, hipStreamSynchronize(c->stream));
    c->sparse_bricks = (int64_t)bricks; c->sparse_pool_bricks = (int64_t)(pool.size() / 32);
    c->have_sparse = true;
    ++c->epoch;
    return FS_OK;
}

int check_scoring_state(fs_ctx *c, bool need_rays, bool need_fim)
{
    if (need_rays && !c->have_ray) return fail(c, FS_E_STATE, "fs_set_ray_params has not been called");
    if (need_rays && !c->have_grid) return fail(c, FS_E_STATE, "fs_upload_grid has not been called");
    if (need_fim && !c->have_lm) return fail(c, FS_E_STATE, "fs_upload_landmarks has not been called");
    if (need_fim && !c->have_table) return fail(c, FS_E_STATE, "no lookup table: call fs_lookup_generate / fs_lookup_load");
    return FS_OK;
}

// The end point clamp of CostCalculator.cpp:47-48 folded into one interval per axis, b = lo_x, hi_x, lo_y, hi_y, lo_z, hi_z:
// max(poly_min, origin), min(poly_max, origin + sizeInMeters), getSizeInMeters = (size - 1 + 0.5) * resolution
void ray_clamp_bounds(const fs_ctx *c, const fs_ray_params &p, double b[6])
{
    const double smx = (c->nx - 1 + 0.5) * c->res, smy = (c->ny - 1 + 0.5) * c->res, smz = (c->nz - 1 + 0.5) * c->res;
    b[0] = std_max(p.polygon[0], c->origin[0]);
    b[1] = std_min(p.polygon[2], c->origin[0] + smx);
    b[2] = std_max(p.polygon[1], c->origin[1]);
    b[3] = std_min(p.polygon[3], c->origin[1] + smy);
    b[4] = c->origin[2];
    b[5] = c->origin[2] + smz;
}

int fill_ray_args(fs_ctx *c, FsRayArgs &a, bool class_ok = true)
{
    const fs_ray_params &p = c->rp;
    a.grid = grid_dev(c);
    a.dir = c->d_dir.p;
    a.n_yaw = c->n_yaw; a.n_elev = c->n_elev; a.window = c->window;
    a.max_length = (unsigned int)(p.max_camera_depth / c->res);             // CostCalculator.cpp:28
    // Long fans walk the class image, cut for exactly this visitor (the ray parameters' ranges; a launch with another visitor
    // — fs_max_arrival — passes class_ok = false and walks the byte image).  It is cut on first use and again when the map or
    // the ranges change: one streaming pass over the grid.
    a.layout = 0;
    if (class_ok && use_class_walk(c, (double)a.max_length)) {
        const int32_t want[4] = {p.obst_min, p.obst_max, p.trace_min, p.trace_max};
        if (!c->have_cls || std::memcmp(want, c->cls_ranges, sizeof want) != 0) {
            if (c->d_cls.ensure(fs_class_image_words(c->nx, c->ny, c->nz)) != hipSuccess ||
                fs_launch_classify(c->d_cells.p, c->d_cls.p, c->nx, c->ny, c->nz, want[0], want[1], want[2], want[3], c->stream) != hipSuccess)
                return fail(c, FS_E_HIP, "could not stage the class image of the grid");
            std::memcpy(c->cls_ranges, want, sizeof want);
            c->have_cls = true;
            c->have_sparse = false;
            ++c->epoch;
        }
        a.grid = grid_dev(c);
        a.layout = 1;
        if (c->opt_layout == 3) {
            if (!c->have_sparse) { const int rc = build_sparse_class_image(c); if (rc) return rc; }
            a.grid.cls = c->d_cls_pool.p;
            a.grid.cls_table = c->d_cls_table.p;
            a.layout = 2;
        }
    }
    a.obst_min = p.obst_min; a.obst_max = p.obst_max; a.trace_min = p.trace_min; a.trace_max = p.trace_max;
    a.clamp = 1;
    double b[6];
    ray_clamp_bounds(c, p, b);
    a.lo_x = b[0]; a.hi_x = b[1]; a.lo_y = b[2]; a.hi_y = b[3]; a.lo_z = b[4]; a.hi_z = b[5];
    a.footprint_radius = std::ceil(p.robot_radius / c->res);               // CostCalculator.cpp:77
    a.delta_theta = p.delta_theta;
    a.half_fov = p.camera_fov / 2;
    a.min_gt = c->min_gt;
    return FS_OK;
}

// What fs_set_ray_params admits, and the fan it stands for: n_yaw accumulated thetas, the FOV window k, the direction table
// dir[(e * n_yaw + i) * 3] (FsRayArgs::dir) and the thetas themselves.  Shared with fs_sense's `sensor`.
int ray_fan_build(fs_ctx *c, const fs_ray_params *p, std::vector<double> &dir, int &n_yaw, int &k)
{
    if (!(p->delta_theta > 0.0) || !(p->max_camera_depth > 0.0) || !(p->camera_fov > 0.0))
        return fail(c, FS_E_INVALID, "max_camera_depth, delta_theta and camera_fov must be positive");
    if (p->n_elev < 1 || p->n_elev > FS_MAX_ELEV) return fail(c, FS_E_INVALID, "n_elev must be in [1,%d]", FS_MAX_ELEV);
    if (!std::isfinite(p->delta_theta) || !std::isfinite(p->max_camera_depth) || !std::isfinite(p->camera_fov) || !std::isfinite(p->robot_radius) ||
        !(p->robot_radius >= 0.0))
        return fail(c, FS_E_INVALID, "max_camera_depth, delta_theta, camera_fov and robot_radius must be finite (robot_radius >= 0)");
    for (int e = 0; e < p->n_elev; ++e)
        if (!std::isfinite(p->elev[e])) return fail(c, FS_E_INVALID, "elevation angles must be finite");
    for (int j = 0; j < 4; ++j)
        if (p->polygon[j] != p->polygon[j]) return fail(c, FS_E_INVALID, "polygon bounds must not be NaN");      // (+-DBL_MAX / +-inf = no clamp)
    // DEP/src/CostCalculator.cpp:36 — accumulated theta, `theta <= 2*pi`
    std::vector<double> theta;
    if (p->n_rays > 0) {
        double t = 0;
        for (int i = 0; i < p->n_rays; ++i) { theta.push_back(t); t += p->delta_theta; }
    } else {
        for (double t = 0; t <= (2 * M_PI); t += p->delta_theta) {
            theta.push_back(t);
            if (theta.size() > 4096) break;
        }
    }
    n_yaw = (int)theta.size();
    k = static_cast<int>(p->camera_fov / p->delta_theta);                    // :87
    if (n_yaw > 4096) return fail(c, FS_E_INVALID, "more than 4096 yaw rays");
    if (k < 1 || n_yaw < k)
        return fail(c, FS_E_INVALID, "fewer yaw rays (%d) than the FOV window (%d): the reference would build a negative-size vector (CostCalculator.cpp:90)", n_yaw, k);
    dir.assign((size_t)n_yaw * p->n_elev * 3, 0.0);
    for (int e = 0; e < p->n_elev; ++e) {
        const double d_h = p->max_camera_depth * std::cos(p->elev[e]);
        const double d_z = p->max_camera_depth * std::sin(p->elev[e]);
        for (int i = 0; i < n_yaw; ++i) {
            double *d = &dir[((size_t)e * n_yaw + i) * 3];
            d[0] = d_h * std::cos(theta[i]);                                 // :42
            d[1] = d_h * std::sin(theta[i]);                                 // :43
            d[2] = d_z;
        }
    }
    return FS_OK;
}

// A visibility volume as the kernels take it (FsFimArgs' fields of the same names): the range and the culling reach, the cone of
// the exact predicate and the slightly wider one of the chunk culling.  Shared by fs_set_fim_params' volume and a landmark sensor's.
void fim_volume(double max_dist, double max_angle, float &maxd2, float &max_dist_f, float &cos2, int32_t &cone_mode, float &cos_a, float &sin_a)
{
    maxd2 = (float)(max_dist * max_dist);
    max_dist_f = (float)max_dist * 1.0001f + 1.0e-3f;              // culling reach, rounded outwards
    if (max_angle >= M_PI) {
        cone_mode = 0; cos2 = 0.0f; cos_a = -1.0f; sin_a = 0.0f;
    } else {
        const float cs = (float)std::cos(max_angle);
        cos2 = cs * cs;
        cone_mode = (cs >= 0.0f) ? 1 : 2;
        // chunk culling uses a slightly wider cone (alpha + 1e-3 rad) than the exact per-landmark predicate
        cos_a = (float)std::cos(max_angle + 1.0e-3);
        sin_a = (float)std::sin(max_angle + 1.0e-3);
        if (max_angle + 1.0e-3 >= M_PI / 2) cone_mode = (cone_mode == 1) ? 3 : 2;   // 3: exact predicate of mode 1, no cone culling
    }
}

int fill_fim_args(fs_ctx *c, FsFimArgs &a)
{
    a.lx = c->d_lx.p; a.ly = c->d_ly.p; a.lz = c->d_lz.p;
    a.spheres = c->d_spheres.p;
    a.n_chunks = c->n_chunks;
    a.cull = c->opt_cull ? 1 : 0;
    a.table = c->d_table.p;
    a.jx0 = c->jx0; a.jy0 = c->jy0; a.jz0 = c->jz0;
    a.tx = c->tx; a.ty = c->ty; a.tz = c->tz;
    a.inv_step = 1 / (double)kStepMax;
    a.inv_step_f = (float)a.inv_step;
    a.factor = c->d_factor.p;
    a.fac1 = c->fac[1]; a.fac2 = c->fac[2]; a.fac3 = c->fac[3]; a.fac4 = c->fac[4];
    a.table_full = c->table_full ? 1 : 0;
    fim_volume(c->fp.max_dist, c->fp.max_angle, a.maxd2, a.max_dist_f, a.cos2, a.cone_mode, a.cos_a, a.sin_a);
    a.far_lattice = !((double)a.max_dist_f * a.inv_step < 1000.0) ? 1 : 0;   // (NaN / inf / huge ranges: exact path for every landmark)
    {   // fl32(p * fl32(1/step)) is within |r| * 2^-23 of the double product the reference rounds (one rounding of the factor, one of
        // the product); twice that at the largest |r| a scored landmark can have, plus an absolute cushion, is the band around a
        // half-integer inside which the kernel re-evaluates in fp64 (0.4995 covered |r| < 2^10 wholesale: 40 times the lanes at 14 m)
        const double r_max = std::max(1.0, (double)a.max_dist_f * a.inv_step);
        const double band = 2.0 * r_max * 1.1920929e-7 + 1.0e-6;
        a.key_thr = a.far_lattice ? 0.0f : (float)(0.5 - band);
    }
    // LDS tier: 2^14 slots (64 KiB, two 512-thread workgroups per CU) or fewer for small clouds; crowded poses are
    // scored in passes; the HBM tier behind it takes what still overflows
    int bits = 10;
    while (bits < c->opt_bits1 && (1 << bits) < 2 * c->m) ++bits;
    // the table's box in the camera frame: lattice index j holds |p / step - j| <= 0.5, so a landmark outside
    // [(j0 - 0.5) step, (j0 + t - 0.5) step] on any axis misses the table whatever the others are; 1 mm outwards covers the
    // rounding of the kernel's fp32 products (|p| <= max_dist).  Used by the INFO_ONLY worker only.
    {
        const double step = (double)kStepMax;
        const int32_t j0[3] = {c->jx0, c->jy0, c->jz0}, tn[3] = {c->tx, c->ty, c->tz};
        for (int k = 0; k < 3; ++k) {
            a.box_lo[k] = std::nextafter((float)(((double)j0[k] - 0.5) * step - 1.0e-3), -INFINITY);
            a.box_hi[k] = std::nextafter((float)(((double)(j0[k] + tn[k]) - 0.5) * step + 1.0e-3), INFINITY);
        }
    }
    a.info_only = 0; a.yaw_only = 0;
    a.learn = c->opt_learn ? 1 : 0;
    a.hash_bits = bits;
    a.skip32 = c->opt_skip32;
    a.headroom = c->opt_headroom;
    a.gtable = c->d_gtable.p;
    a.ghash_bits = c->ghash_bits;
    a.counters = c->d_counters.p;
    return FS_OK;
}

int ensure_candidate_scratch(fs_ctx *c, size_t n, bool want_fim21)
{
    FS_HIP(c, c->d_arrival.ensure(n)); FS_HIP(c, c->d_argmax.ensure(n)); FS_HIP(c, c->d_status.ensure(n));
    FS_HIP(c, c->d_yaw.ensure(n)); FS_HIP(c, c->d_ach.ensure(n));
    FS_HIP(c, c->d_info.ensure(n)); FS_HIP(c, c->d_trace.ensure(n)); FS_HIP(c, c->d_logdet.ensure(n));
    FS_HIP(c, c->d_nvis.ensure(n)); FS_HIP(c, c->d_nvox.ensure(n)); FS_HIP(c, c->d_overflow.ensure(n));
    FS_HIP(c, c->d_sums.ensure(n * 18));
    FS_HIP(c, c->d_flagged.ensure(n * 2));
    if (c->d_tested.cap < n) {
        FS_HIP(c, c->d_tested.ensure(n));
        FS_HIP(c, hipMemsetAsync(c->d_tested.p, 0, c->d_tested.cap * sizeof(uint32_t), c->stream));
    }
    if (want_fim21) FS_HIP(c, c->d_fim21.ensure(n * 21));
    return FS_OK;
}

// ---------------------------------------------------------------- keep-out zones

// addNewMarkedAreaFOV / addNewMarkedArea for one stored zone on a map of geometry g: its rays appended to `rays` (none when the
// apex is off the map — the reference's early return, keepout_layer.cpp:205-206 — or the size in cells cannot be converted)
void ko_zone_rays(const KoZone &z, const KoGeom &g, std::vector<fs_ko_ray> &rays)
{
    int32_t ax = 0, ay = 0;
    uint32_t size_cells = 0;
    if (!fs_ko_world_to_map(z.wx, z.wy, g.ox, g.oy, g.res, g.nx, g.ny, &ax, &ay)) return;
    if (!fs_ko_size_in_cells(z.size, g.res, &size_cells)) return;
    const size_t at = rays.size();
    rays.resize(at + FS_KO_MAX_RAYS);
    const int n = z.kind == FS_KO_FOV ? fs_ko_fov_rays(ax, ay, size_cells, z.yaw, g.nx, g.ny, &rays[at])
                                      : fs_ko_disc_rays(ax, ay, size_cells, g.nx, g.ny, &rays[at]);
    rays.resize(at + (size_t)n);
}

// Zones [first, end) rasterised on the 2-D grid of geometry g whose cells are in d_cells: each is marked into the scratch image
// and folded — painted into the grid, counted, added to the union mask — on its bounding box; one wait for the counts at the
// end.  A zone is folded on its own because its n_cells are ITS distinct cells, and zones overlap (the robot marks where it
// keeps getting stuck).  box: the cells [x0, x1] x [y0, y1] written (x1 < x0: none).
int ko_rasterise(fs_ctx *c, size_t first, const KoGeom &g, int32_t box[4])
{
    const size_t n = c->ko_zones.size() - first;
    std::vector<fs_ko_ray> rays;
    std::vector<size_t> start(n + 1, 0);
    for (size_t k = 0; k < n; ++k) {
        ko_zone_rays(c->ko_zones[first + k], g, rays);
        start[k + 1] = rays.size();
    }
    box[0] = g.nx; box[1] = g.ny; box[2] = -1; box[3] = -1;
    for (size_t k = 0; k < n; ++k) c->ko_zones[first + k].n_cells = 0;
    if (rays.empty()) return FS_OK;
    FS_HIP(c, c->d_ko_rays.ensure(rays.size() * 4));
    FS_HIP(c, c->d_ko_counts.ensure(FS_KEEPOUT_MAX_ZONES));
    FS_HIP(c, hipMemcpyAsync(c->d_ko_rays.p, rays.data(), rays.size() * sizeof(fs_ko_ray), hipMemcpyHostToDevice, c->stream));
    FS_HIP(c, hipMemsetAsync(c->d_ko_counts.p, 0, n * sizeof(unsigned long long), c->stream));
    for (size_t k = 0; k < n; ++k) {
        if (start[k + 1] == start[k]) continue;
        int32_t x0 = g.nx, y0 = g.ny, x1 = -1, y1 = -1;
        for (size_t r = start[k]; r < start[k + 1]; ++r) {
            x0 = std::min(x0, std::min(rays[r].ax, rays[r].ex)); x1 = std::max(x1, std::max(rays[r].ax, rays[r].ex));
            y0 = std::min(y0, std::min(rays[r].ay, rays[r].ey)); y1 = std::max(y1, std::max(rays[r].ay, rays[r].ey));
        }
        FS_HIP(c, fs_launch_keepout_mark(c->d_ko_rays.p + 4 * start[k], (int64_t)(start[k + 1] - start[k]), c->d_ko_scratch.p, g.nx, g.ny, c->stream));
        FS_HIP(c, fs_launch_keepout_fold(c->d_ko_scratch.p, c->d_ko_mask.p, c->d_cells.p, g.nx, g.ny, x0, y0, x1 - x0 + 1, y1 - y0 + 1,
                                         c->d_ko_counts.p + k, c->stream));
        box[0] = std::min(box[0], x0); box[1] = std::min(box[1], y0); box[2] = std::max(box[2], x1); box[3] = std::max(box[3], y1);
    }
    std::vector<unsigned long long> counts(n, 0);
    FS_HIP(c, hipMemcpyAsync(counts.data(), c->d_ko_counts.p, n * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipStreamSynchronize(c->stream));              // (the ray table and the counts are this call's)
    for (size_t k = 0; k < n; ++k) c->ko_zones[first + k].n_cells = (int64_t)counts[k];
    return FS_OK;
}

// matchSize (keepout_layer.cpp:184-199): the cache is dropped and every stored zone rasterised again for geometry g.  The
// reference's loop there calls addNewMarkedAreaFOV, which pushes onto zone_specs_ WHILE the loop iterates it — undefined
// behaviour, and duplicate zones where it survives.  Not restated: one stored request stays one zone.
int ko_rebuild(fs_ctx *c, const KoGeom &g, int32_t box[4])
{
    const size_t cells = (size_t)g.nx * (size_t)g.ny;
    c->ko_mask_valid = false;
    FS_HIP(c, c->d_ko_mask.ensure(cells)); FS_HIP(c, c->d_ko_scratch.ensure(cells));
    FS_HIP(c, hipMemsetAsync(c->d_ko_mask.p, 0, cells, c->stream));
    FS_HIP(c, hipMemsetAsync(c->d_ko_scratch.p, 0, cells, c->stream));
    const int rc = ko_rasterise(c, 0, g, box);
    if (rc) return rc;
    c->ko_geom = g;
    c->ko_mask_valid = true;
    return FS_OK;
}

// The layer's cycle after a snapshot (fs_upload_grid, fs_upload_grid_bricks): the new cells are on the device, every zone is
// painted into them — from the union mask when the geometry is the one it was cut for, else after matchSize.  A 3-D grid is
// staged unmarked (the layer is a 2-D costmap's): the zones are kept and mark nothing.  Callers skip this with no zone stored.
int ko_after_snapshot(fs_ctx *c, int32_t nx, int32_t ny, int32_t nz, const double origin_xyz[3], double resolution)
{
    if (nz != 1) {
        c->ko_mask_valid = false;
        for (KoZone &z : c->ko_zones) z.n_cells = 0;
        return FS_OK;
    }
    const KoGeom g{nx, ny, origin_xyz[0], origin_xyz[1], resolution};
    int32_t box[4];
    if (!c->ko_mask_valid || !(c->ko_geom == g)) return ko_rebuild(c, g, box);
    FS_HIP(c, fs_launch_keepout_apply(c->d_ko_mask.p, c->d_cells.p, nx, ny, 0, 0, nx, ny, nullptr, c->stream));
    return FS_OK;
}

// The two steps of every route that writes cells of the staged map (last paragraph), enqueued after the write.  First the
// keep-out layer, which runs last in the cycle: the stored zones are painted again over the window that changed.
int ko_repaint_window(fs_ctx *c, int32_t x0, int32_t y0, int32_t sx, int32_t sy)
{
    if (!c->ko_zones.empty() && c->ko_mask_valid)
        FS_HIP(c, fs_launch_keepout_apply(c->d_ko_mask.p, c->d_cells.p, c->nx, c->ny, x0, y0, sx, sy, nullptr, c->stream));
    return FS_OK;
}

// Then the images cut from the cells: the class image is cut again for the bricks the box touches (none for an empty box; a
// whole-map re-cut is a streaming pass over the grid — 1 GiB on C5 — for a box of a few thousand cells), the sparse image is dropped.
int cells_changed_in_box(fs_ctx *c, int32_t x0, int32_t y0, int32_t z0, int32_t sx, int32_t sy, int32_t sz)
{
    if (c->have_cls && sx > 0 && sy > 0 && sz > 0) {
        const int b0[3] = {x0 >> 3, y0 >> 3, z0 >> 3};
        const int nb[3] = {((x0 + sx - 1) >> 3) - b0[0] + 1, ((y0 + sy - 1) >> 3) - b0[1] + 1, ((z0 + sz - 1) >> 3) - b0[2] + 1};
        FS_HIP(c, fs_launch_classify_region(c->d_cells.p, c->d_cls.p, c->nx, c->ny, c->nz, c->cls_ranges[0], c->cls_ranges[1], c->cls_ranges[2],
                                            c->cls_ranges[3], b0, nb, c->stream));
    }
    c->have_sparse = false;
    return FS_OK;
}

// The window of fs_update_grid_region and fs_read_grid_region on the staged grid: refused, empty (nothing to move), or whole with
// the strides' defaults filled in
int window_check(fs_ctx *c, int32_t x0, int32_t y0, int32_t z0, int32_t sx, int32_t sy, int32_t sz, const uint8_t *cells,
                 int64_t &row_stride, int64_t &slice_stride, bool &empty)
{
    empty = true;
    if (sx < 0 || sy < 0 || sz < 0) return fail(c, FS_E_INVALID, "negative window size");
    if (x0 < 0 || y0 < 0 || z0 < 0 || (int64_t)x0 + sx > c->nx || (int64_t)y0 + sy > c->ny || (int64_t)z0 + sz > c->nz)
        return fail(c, FS_E_INVALID, "window [%d,%lld) x [%d,%lld) x [%d,%lld) leaves the %d x %d x %d grid", x0, (long long)x0 + sx, y0, (long long)y0 + sy,
                    z0, (long long)z0 + sz, c->nx, c->ny, c->nz);
    if (sx == 0 || sy == 0 || sz == 0) return FS_OK;
    if (!cells) return FS_E_INVALID;
    if (row_stride == 0) row_stride = sx;
    if (slice_stride == 0) slice_stride = row_stride * (int64_t)sy;
    if (row_stride < sx || slice_stride < row_stride * (int64_t)(sy - 1) + sx) return fail(c, FS_E_INVALID, "window strides smaller than the window");
    empty = false;
    return FS_OK;
}

// fs_sense's and fs_drive's prologue in three steps; a caller's own checks stand between them.  What a sweep needs staged:
int sweep_state_check(fs_ctx *c, const fs_ray_params *sensor)
{
    if (const int rc = grid_check(c)) return rc;
    if (!c->have_world) return fail(c, FS_E_STATE, "fs_upload_world has not been called");
    if (!sensor && !c->have_ray) return fail(c, FS_E_STATE, "fs_set_ray_params has not been called and no sensor is given");
    return FS_OK;
}

// The sweep's fan: `sensor`'s (validated and built by the same host code as fs_set_ray_params'; the table goes to the device only
// when it is not the one already there) or, sensor == NULL, the context's.  Every one of the n_first first_ray lies inside it,
// and the outputs are those of a sweep that reveals nothing.
int sweep_fan_setup(fs_ctx *c, const fs_ray_params *sensor, const int32_t *first_ray, size_t n_first, FsSenseArgs &a, int64_t *n_seen,
                    int64_t *n_revealed, int32_t window[6])
{
    if (sensor) {
        std::vector<double> dir;
        int n_yaw = 0, k = 0;
        const int rc = ray_fan_build(c, sensor, dir, n_yaw, k);
        if (rc) return rc;
        if (dir != c->sense_dir) {
            c->sense_dir.clear();
            FS_HIP(c, c->d_sense_dir.ensure(dir.size()));
            FS_HIP(c, hipMemcpyAsync(c->d_sense_dir.p, dir.data(), dir.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
            FS_HIP(c, hipStreamSynchronize(c->stream));
            c->sense_dir.swap(dir);
        }
        a.dir = c->d_sense_dir.p;
        a.n_yaw = n_yaw; a.n_elev = sensor->n_elev; a.window = k;
    } else {
        a.dir = c->d_dir.p;
        a.n_yaw = c->n_yaw; a.n_elev = c->n_elev; a.window = c->window;
    }
    if (first_ray)
        for (size_t i = 0; i < n_first; ++i)
            if (first_ray[i] < -1 || first_ray[i] > a.n_yaw - a.window)
                return fail(c, FS_E_INVALID, "first_ray[%zu] = %d is outside [-1, %d]", i, first_ray[i], a.n_yaw - a.window);
    if (n_seen) *n_seen = 0;
    if (n_revealed) *n_revealed = 0;
    if (window) std::fill(window, window + 6, 0);
    return FS_OK;
}

// For a sweep that has poses: the world, the staged grid, the walk's cap, the visitor's ranges and the clamp bounds of its ray
// parameters, then the mark image
int sweep_world_setup(fs_ctx *c, const fs_ray_params *sensor, FsSenseArgs &a)
{
    const fs_ray_params &p = sensor ? *sensor : c->rp;
    a.world = world_dev(c);
    a.staged = c->d_cells.p;
    a.max_length = (unsigned int)(p.max_camera_depth / c->res);             // CostCalculator.cpp:28
    a.obst_min = p.obst_min; a.obst_max = p.obst_max; a.trace_min = p.trace_min; a.trace_max = p.trace_max;
    double b[6];
    ray_clamp_bounds(c, p, b);
    a.lo_x = b[0]; a.hi_x = b[1]; a.lo_y = b[2]; a.hi_y = b[3]; a.lo_z = b[4]; a.hi_z = b[5];
    // the mark image: allocated and zeroed once per grid shape, all zero again after every merge
    const size_t total = (size_t)c->nx * (size_t)c->ny * (size_t)c->nz;
    const bool grown = c->d_sense_mark.cap < total;
    FS_HIP(c, c->d_sense_mark.ensure(total));
    if (grown || !c->sense_mark_clean) FS_HIP(c, hipMemsetAsync(c->d_sense_mark.p, 0, c->d_sense_mark.cap, c->stream));
    c->sense_mark_clean = false;
    return FS_OK;
}

// the ground-truth world and the mark image of its shape leave the context (the stream has drained)
void drop_world(fs_ctx *c)
{
    c->d_world.release();
    c->d_sense_mark.release();
    c->have_world = false;
    c->sense_mark_clean = false;
}

// A snapshot's geometry (fs_upload_grid, fs_upload_grid_bricks), checked in two parts: the brick route's own check stands between
int snapshot_geometry_check(fs_ctx *c, int32_t nx, int32_t ny, int32_t nz, const double origin_xyz[3], double resolution)
{
    if (nx <= 0 || ny <= 0 || nz <= 0 || !(resolution > 0.0) || !std::isfinite(resolution)) return fail(c, FS_E_INVALID, "bad grid shape or resolution");
    // (worldToMap with a NaN origin is a float-to-integer conversion of NaN: undefined in the reference, refused here)
    if (!std::isfinite(origin_xyz[0]) || !std::isfinite(origin_xyz[1]) || !std::isfinite(origin_xyz[2])) return fail(c, FS_E_INVALID, "grid origin must be finite");
    return FS_OK;
}

int snapshot_size_check(fs_ctx *c, int32_t nx, int32_t ny, int32_t nz, uint64_t &total)
{
    total = (uint64_t)nx * (uint64_t)ny * (uint64_t)nz;
    // (cell offsets are 32-bit unsigned in the walks, one z step is a signed 32-bit stride; everything else indexes in 64 bits)
    if (total >= (1ull << 32) || (uint64_t)nx * (uint64_t)ny >= (1ull << 31)) return fail(c, FS_E_INVALID, "dense grids are limited to 2^32 cells (and 2^31 per z slice)");
    return FS_OK;
}

// ... and its tail, the new cells on their way into d_cells: the keep-out layer's cycle, the derived images, the wait, then the
// context describes the new map
int snapshot_done(fs_ctx *c, int32_t nx, int32_t ny, int32_t nz, const double origin_xyz[3], double resolution)
{
    if (!c->ko_zones.empty())
        if (const int rc = ko_after_snapshot(c, nx, ny, nz, origin_xyz, resolution)) return rc;
    if (const int rc = retile_grid(c, nx, ny, nz)) return rc;
    FS_HIP(c, hipStreamSynchronize(c->stream));
    if (c->have_world && (nx != c->nx || ny != c->ny || nz != c->nz)) drop_world(c);   // (the world is of the staged grid's shape)
    c->nx = nx; c->ny = ny; c->nz = nz;
    c->origin[0] = origin_xyz[0]; c->origin[1] = origin_xyz[1]; c->origin[2] = origin_xyz[2];
    c->res = resolution;
    c->have_grid = true;
    c->max_gt = 0.0; c->min_gt = 0.0;
    ++c->epoch;
    return FS_OK;
}

}  // namespace

// ================================================================== C ABI

extern "C" {

int fs_abi_version(void) { return FS_ABI_VERSION; }

int fs_ctx_create(int device_id, void *stream, fs_ctx **out)
{
    if (!out) return FS_E_INVALID;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device_id < 0 || device_id >= count) return FS_E_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) != hipSuccess) return FS_E_NO_DEVICE;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return FS_E_NO_DEVICE;   // kernels are built for gfx950 only
    if (hipSetDevice(device_id) != hipSuccess) return FS_E_NO_DEVICE;
    fs_ctx *c = new fs_ctx();
    c->device = device_id;
    if (stream) {
        c->stream = reinterpret_cast<hipStream_t>(stream);
    } else {
        if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
            delete c;
            return FS_E_HIP;
        }
        c->own_stream = true;
    }
    // device-side counters (fs_get_counter; 29 / 30: range checks of FS_BOUNDS builds)
    if (c->d_counters.ensure(FS_N_COUNTERS) != hipSuccess ||
        hipMemsetAsync(c->d_counters.p, 0, FS_N_COUNTERS * sizeof(unsigned long long), c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) {
        fs_ctx_destroy(c);
        return FS_E_HIP;
    }
    *out = c;
    return FS_OK;
}

void fs_ctx_destroy(fs_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    for (auto &t : c->launches) { (void)hipEventDestroy(t.start); (void)hipEventDestroy(t.stop); }
    for (auto e : c->event_pool) (void)hipEventDestroy(e);
    for (auto &g : c->graphs) if (g.second.exec) (void)hipGraphExecDestroy(g.second.exec);
    // (grown inside fs_rank.hip / fs_sort.hip: raw pointers, not buffers)
    if (c->rank_scratch) (void)hipFree(c->rank_scratch);
    if (c->sort_scratch) (void)hipFree(c->sort_scratch);
    // every DevBuf / PinnedBuf member frees itself with the context; a stream of the context's own goes after them
    const hipStream_t stream = c->stream;
    const bool own_stream = c->own_stream;
    delete c;
    if (own_stream) (void)hipStreamDestroy(stream);
}

const char *fs_last_error(const fs_ctx *c) { return c ? c->err.c_str() : "null context"; }

int fs_synchronize(fs_ctx *c)
{
    if (!c) return FS_E_INVALID;
    FS_HIP(c, hipSetDevice(c->device));
    FS_HIP(c, hipStreamSynchronize(c->stream));
    return FS_OK;
}

int fs_enable_kernel_timing(fs_ctx *c, int enable)
{
    if (!c) return FS_E_INVALID;
    c->timing = enable != 0;
    return FS_OK;
}

int fs_kernel_time(fs_ctx *c, int kind, double *total_ms, int64_t *launches)
{
    if (!c) return FS_E_INVALID;
    FS_HIP(c, hipSetDevice(c->device));
    FS_HIP(c, hipStreamSynchronize(c->stream));
    double tot = 0.0;
    int64_t cnt = 0;
    std::vector<TimedLaunch> keep;
    for (auto &t : c->launches) {
        if (t.kind == kind) {
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, t.start, t.stop) == hipSuccess) { tot += ms; ++cnt; }
            c->event_pool.push_back(t.start);
            c->event_pool.push_back(t.stop);
        } else {
            keep.push_back(t);
        }
    }
    c->launches.swap(keep);
    if (total_ms) *total_ms = tot;
    if (launches) *launches = cnt;
    return FS_OK;
}

// ------------------------------------------------------------------ arrival information

int fs_set_ray_params(fs_ctx *c, const fs_ray_params *p)
{
    if (!c || !p) return FS_E_INVALID;
    FS_HIP(c, hipSetDevice(c->device));
    std::vector<double> dir;
    int n_yaw = 0, k = 0;
    {
        const int rc = ray_fan_build(c, p, dir, n_yaw, k);
        if (rc) return rc;
    }
    // rotation of the pose (goal, best yaw) for every possible argmax: orientationAroundZAxis(yaw)
    // (setRPY(0,0,yaw)) -> Quaternionf -> rotation matrix, as isPoseSafe(Point,Point) + getTransformFromPose
    const int n_win = n_yaw - k + 1;
    std::vector<float> yawR((size_t)n_win * 9);
    for (int i = 0; i < n_win; ++i) {
        const double yaw = (i * p->delta_theta) + (p->camera_fov / 2);       // :119
        const double half = yaw * 0.5;
        const double pose7[7] = {0, 0, 0, 0.0, 0.0, std::sin(half), std::cos(half)};
        float Rt[12];
        pose_to_rt(pose7, Rt);
        std::copy(Rt, Rt + 9, &yawR[(size_t)i * 9]);
    }
    bool yaw_exact = true;
    for (int i = 0; i < n_win; ++i) {
        const float *R = &yawR[(size_t)i * 9];
        yaw_exact = yaw_exact && R[2] == 0.0f && R[5] == 0.0f && R[6] == 0.0f && R[7] == 0.0f && R[8] == 1.0f;
    }
    FS_HIP(c, c->d_dir.ensure(dir.size()));
    FS_HIP(c, c->d_yawR.ensure(yawR.size()));
    FS_HIP(c, hipMemcpyAsync(c->d_dir.p, dir.data(), dir.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    FS_HIP(c, hipMemcpyAsync(c->d_yawR.p, yawR.data(), yawR.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    FS_HIP(c, hipStreamSynchronize(c->stream));
    c->rp = *p;
    c->n_yaw = n_yaw; c->n_elev = p->n_elev; c->window = k;
    c->yaw_exact = yaw_exact;
    c->have_ray = true;
    ++c->epoch;
    c->max_gt = 0.0; c->min_gt = 0.0;
    return FS_OK;
}

int fs_ray_fan_shape(const fs_ctx *c, int32_t *n_yaw, int32_t *n_elev, int32_t *window)
{
    if (!c || !c->have_ray) return FS_E_STATE;
    if (n_yaw) *n_yaw = c->n_yaw;
    if (n_elev) *n_elev = c->n_elev;
    if (window) *window = c->window;
    return FS_OK;
}

int fs_upload_grid(fs_ctx *c, const uint8_t *cells, int32_t nx, int32_t ny, int32_t nz,
                   const double origin_xyz[3], double resolution)
{
    if (!c || !cells || !origin_xyz) return FS_E_INVALID;
    FS_HIP(c, hipSetDevice(c->device));
    if (const int rc = snapshot_geometry_check(c, nx, ny, nz, origin_xyz, resolution)) return rc;
    uint64_t total = 0;
    if (const int rc = snapshot_size_check(c, nx, ny, nz, total)) return rc;
    ++c->grid_gen;
    FS_HIP(c, c->d_cells.ensure((size_t)total));
    FS_HIP(c, hipMemcpyAsync(c->d_cells.p, cells, (size_t)total, hipMemcpyHostToDevice, c->stream));
    return snapshot_done(c, nx, ny, nz, origin_xyz, resolution);
}

// Layer::updateCosts' window of the master grid (include/fitslam_frontier.h): packed on the host into page-locked memory, one
// transfer, one scatter into the row-major image, then what follows every write of cells (ko_repaint_window, cells_changed_in_box).
int fs_update_grid_region(fs_ctx *c, int32_t x0, int32_t y0, int32_t z0, int32_t sx, int32_t sy, int32_t sz,
                          const uint8_t *cells, int64_t row_stride, int64_t slice_stride)
{
    if (!c) return FS_E_INVALID;
    if (const int rc = grid_check(c)) return rc;
    bool empty = true;
    if (const int rc = window_check(c, x0, y0, z0, sx, sy, sz, cells, row_stride, slice_stride, empty)) return rc;
    if (empty) return FS_OK;
    const size_t total = (size_t)sx * (size_t)sy * (size_t)sz;
    ++c->grid_gen;
    FS_HIP(c, c->h_win.ensure(total));
    FS_HIP(c, c->d_win.ensure(total));
    for (int32_t z = 0; z < sz; ++z)
        for (int32_t y = 0; y < sy; ++y)
            std::memcpy(c->h_win.p + ((size_t)z * sy + y) * sx, cells + (size_t)z * (size_t)slice_stride + (size_t)y * (size_t)row_stride, (size_t)sx);
    FS_HIP(c, hipMemcpyAsync(c->d_win.p, c->h_win.p, total, hipMemcpyHostToDevice, c->stream));
    FS_HIP(c, fs_launch_window_scatter(c->d_win.p, c->d_cells.p, c->nx, c->ny, x0, y0, z0, sx, sy, sz, c->stream));
    if (const int rc = ko_repaint_window(c, x0, y0, sx, sy)) return rc;       // (inside the window is all that changed)
    if (const int rc = cells_changed_in_box(c, x0, y0, z0, sx, sy, sz)) return rc;
    FS_HIP(c, hipStreamSynchronize(c->stream));                  // (the page-locked window is the next call's again)
    if (c->h_win.cap > ((size_t)64 << 20)) { c->h_win.release(); c->d_win.release(); }   // (a window of map size: not worth keeping)
    ++c->epoch;
    return FS_OK;
}

int fs_upload_grid_bricks(fs_ctx *c, int32_t nx, int32_t ny, int32_t nz, const double origin_xyz[3], double resolution,
                          uint8_t default_value, int64_t n_bricks, const int32_t *brick_xyz, const uint8_t *brick_cells)
{
    if (!c || !origin_xyz || n_bricks < 0 || (n_bricks > 0 && (!brick_xyz || !brick_cells))) return FS_E_INVALID;
    FS_HIP(c, hipSetDevice(c->device));
    if (const int rc = snapshot_geometry_check(c, nx, ny, nz, origin_xyz, resolution)) return rc;
    if ((nx & 7) || (ny & 7) || (nz & 7)) return fail(c, FS_E_INVALID, "brick upload needs dimensions that are multiples of 8");
    uint64_t total = 0;
    if (const int rc = snapshot_size_check(c, nx, ny, nz, total)) return rc;
    ++c->grid_gen;
    FS_HIP(c, c->d_cells.ensure((size_t)total));
    FS_HIP(c, hipMemsetAsync(c->d_cells.p, default_value, (size_t)total, c->stream));
    if (n_bricks > 0) {
        DevBuf<int32_t> &d_xyz = c->d_brick_xyz, &d_bad = c->d_bad;
        DevBuf<uint8_t> &d_bc = c->d_brick_cells;
        FS_HIP(c, d_xyz.ensure((size_t)n_bricks * 3)); FS_HIP(c, d_bc.ensure((size_t)n_bricks * 512)); FS_HIP(c, d_bad.ensure(1));
        FS_HIP(c, hipMemsetAsync(d_bad.p, 0, 4, c->stream));
        FS_HIP(c, hipMemcpyAsync(d_xyz.p, brick_xyz, sizeof(int32_t) * 3 * (size_t)n_bricks, hipMemcpyHostToDevice, c->stream));
        FS_HIP(c, hipMemcpyAsync(d_bc.p, brick_cells, (size_t)n_bricks * 512, hipMemcpyHostToDevice, c->stream));
        FS_HIP(c, fs_launch_brick_scatter(n_bricks, d_xyz.p, d_bc.p, c->d_cells.p, nx, ny, nz, d_bad.p, c->stream));
        int32_t bad = 0;
        FS_HIP(c, hipMemcpyAsync(&bad, d_bad.p, 4, hipMemcpyDeviceToHost, c->stream));
        FS_HIP(c, hipStreamSynchronize(c->stream));
        if (d_bc.cap > ((size_t)64 << 20)) { d_bc.release(); d_xyz.release(); }   // a whole-map brick list (C5: 385 MB) is not worth keeping
        if (bad) { c->have_grid = false; return fail(c, FS_E_INVALID, "a brick lies outside the grid"); }
    }
    return snapshot_done(c, nx, ny, nz, origin_xyz, resolution);
}

int fs_frontier_cells(fs_ctx *c, int32_t lethal_threshold, uint8_t *mask, int64_t *count)
{
    if (!c || !count) return FS_E_INVALID;
    if (const int rc = grid_check(c)) return rc;
    const size_t total = (size_t)c->nx * c->ny * c->nz;
    DevBuf<uint8_t> &d_mask = c->d_mask;
    DevBuf<unsigned long long> &d_count = c->d_count;
    if (mask) FS_HIP(c, d_mask.ensure(total));
    FS_HIP(c, d_count.ensure(1));
    FS_HIP(c, hipMemsetAsync(d_count.p, 0, sizeof(unsigned long long), c->stream));
    {
        ScopedTimer t(c, 5);
        FS_HIP(c, fs_launch_frontier_cells(c->d_cells.p, c->nx, c->ny, c->nz, lethal_threshold, mask ? d_mask.p : nullptr, d_count.p, c->stream));
    }
    unsigned long long n = 0;
    FS_HIP(c, hipMemcpyAsync(&n, d_count.p, sizeof n, hipMemcpyDeviceToHost, c->stream));
    if (mask) FS_HIP(c, hipMemcpyAsync(mask, d_mask.p, total, hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipStreamSynchronize(c->stream));
    *count = (int64_t)n;
    if (d_mask.cap > ((size_t)64 << 20)) d_mask.release();       // a whole-map mask (128 MB at 512^3, 1 GiB at 1024^3) is not worth keeping between ticks
    return FS_OK;
}

// ------------------------------------------------------------------ sensor sweep on a ground-truth world

int fs_upload_world(fs_ctx *c, const uint8_t *cells, int32_t nx, int32_t ny, int32_t nz)
{
    if (!c) return FS_E_INVALID;
    if (const int rc = grid_check(c)) return rc;
    if (!cells) {
        FS_HIP(c, hipStreamSynchronize(c->stream));
        drop_world(c);
        return FS_OK;
    }
    if (nx != c->nx || ny != c->ny || nz != c->nz)
        return fail(c, FS_E_INVALID, "the world is %d x %d x %d, the staged grid %d x %d x %d", nx, ny, nz, c->nx, c->ny, c->nz);
    const size_t total = (size_t)nx * (size_t)ny * (size_t)nz;
    c->have_world = false;
    FS_HIP(c, c->d_world.ensure(total));
    FS_HIP(c, hipMemcpyAsync(c->d_world.p, cells, total, hipMemcpyHostToDevice, c->stream));
    FS_HIP(c, hipStreamSynchronize(c->stream));
    c->have_world = true;
    return FS_OK;
}

int fs_sense(fs_ctx *c, int32_t n, const double *origin_xyz, const int32_t *first_ray, const fs_ray_params *sensor, int32_t *ray_unknown,
             int32_t *seen_unknown, int32_t *status, int64_t *n_seen, int64_t *n_revealed, int32_t window[6])
{
    if (!c || n < 0 || (n > 0 && (!origin_xyz || !seen_unknown || !status))) return FS_E_INVALID;
    if (const int rc = sweep_state_check(c, sensor)) return rc;
    FsSenseArgs a{};
    if (const int rc = sweep_fan_setup(c, sensor, first_ray, (size_t)n, a, n_seen, n_revealed, window)) return rc;
    if (n == 0) return FS_OK;

    if (const int rc = sweep_world_setup(c, sensor, a)) return rc;
    const size_t n_rays = (size_t)a.n_yaw * (size_t)a.n_elev;
    const size_t un = (size_t)n;
    FS_HIP(c, c->d_sense_origin.ensure(3 * un)); FS_HIP(c, c->d_sense_out.ensure(6 + 2 * un)); FS_HIP(c, c->d_sense_counts.ensure(4));
    if (first_ray) FS_HIP(c, c->d_sense_first.ensure(un));
    if (ray_unknown) FS_HIP(c, c->d_sense_rays.ensure(un * n_rays));
    const int32_t box0[6] = {c->nx, c->ny, c->nz, -1, -1, -1};
    FS_HIP(c, hipMemcpyAsync(c->d_sense_origin.p, origin_xyz, 3 * un * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (first_ray) FS_HIP(c, hipMemcpyAsync(c->d_sense_first.p, first_ray, un * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    FS_HIP(c, hipMemcpyAsync(c->d_sense_out.p, box0, sizeof box0, hipMemcpyHostToDevice, c->stream));
    a.n = n;
    a.origin = c->d_sense_origin.p;
    a.first_ray = first_ray ? c->d_sense_first.p : nullptr;
    a.mark = c->d_sense_mark.p;
    a.ray_unknown = ray_unknown ? c->d_sense_rays.p : nullptr;
    a.box = c->d_sense_out.p;
    a.status = c->d_sense_out.p + 6;
    a.seen_unknown = c->d_sense_out.p + 6 + un;
    FS_HIP(c, fs_launch_sense(a, c->stream));
    std::vector<int32_t> out(6 + 2 * un);
    FS_HIP(c, hipMemcpyAsync(out.data(), c->d_sense_out.p, out.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (ray_unknown) FS_HIP(c, hipMemcpyAsync(ray_unknown, c->d_sense_rays.p, un * n_rays * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipStreamSynchronize(c->stream));                  // (the one wait between the two kernels: status, box, counts per pose)
    std::copy(out.begin() + 6, out.begin() + 6 + n, status);
    std::copy(out.begin() + 6 + n, out.end(), seen_unknown);
    if (out[3] < out[0]) {                                       // no pose on the map: nothing was marked, nothing changes
        c->sense_mark_clean = true;
        return FS_OK;
    }
    const int32_t x0 = out[0], y0 = out[1], z0 = out[2], sx = out[3] - out[0] + 1, sy = out[4] - out[1] + 1, sz = out[5] - out[2] + 1;
    if (x0 < 0 || y0 < 0 || z0 < 0 || sy < 1 || sz < 1 || out[3] >= c->nx || out[4] >= c->ny || out[5] >= c->nz)
        return fail(c, FS_E_HIP, "fs_sense: the seen cells' box [%d,%d] x [%d,%d] x [%d,%d] leaves the grid", out[0], out[3], out[1], out[4], out[2], out[5]);
    ++c->grid_gen;
    FS_HIP(c, hipMemsetAsync(c->d_sense_counts.p, 0, 2 * sizeof(unsigned long long), c->stream));
    FS_HIP(c, fs_launch_sense_merge(c->d_world.p, c->d_cells.p, c->d_sense_mark.p, c->nx, c->ny, x0, y0, z0, sx, sy, sz, c->d_sense_counts.p, c->stream));
    if (const int rc = ko_repaint_window(c, x0, y0, sx, sy)) return rc;
    if (const int rc = cells_changed_in_box(c, x0, y0, z0, sx, sy, sz)) return rc;
    unsigned long long counts[2] = {0ull, 0ull};
    FS_HIP(c, hipMemcpyAsync(counts, c->d_sense_counts.p, sizeof counts, hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipStreamSynchronize(c->stream));                  // (the counts are the merge's)
    c->sense_mark_clean = true;
    ++c->epoch;
    if (n_seen) *n_seen = (int64_t)counts[0];
    if (n_revealed) *n_revealed = (int64_t)counts[1];
    if (window) { window[0] = x0; window[1] = y0; window[2] = z0; window[3] = sx; window[4] = sy; window[5] = sz; }
    return FS_OK;
}

int fs_goals_mapped(fs_ctx *c, int32_t n, const double *goal_xyz, uint8_t *mapped)
{
    if (!c || n < 0 || (n > 0 && (!goal_xyz || !mapped))) return FS_E_INVALID;
    const int rc = grid2d_check(c, "fs_goals_mapped");
    if (rc) return rc;
    if (n == 0) return FS_OK;
    const size_t un = (size_t)n;
    FS_HIP(c, c->d_sense_origin.ensure(3 * un)); FS_HIP(c, c->d_sense_mapped.ensure(un));
    FS_HIP(c, hipMemcpyAsync(c->d_sense_origin.p, goal_xyz, 3 * un * sizeof(double), hipMemcpyHostToDevice, c->stream));
    FS_HIP(c, fs_launch_goals_mapped(c->d_cells.p, c->nx, c->ny, c->origin[0], c->origin[1], c->res, n, c->d_sense_origin.p, c->d_sense_mapped.p, c->stream));
    FS_HIP(c, hipMemcpyAsync(mapped, c->d_sense_mapped.p, un, hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipStreamSynchronize(c->stream));
    return FS_OK;
}

// The drive: every step's launches go onto the stream back to back, the stop decisions stay on the device, and
// the one wait at the end reads every output.  d_drive_i32, T = all stations: n_stations [R] | first station [R] | state [R][2] |
// union box [4] | station_status [T] | seen_unknown [T] | station boxes [T][4] | first_ray [T]; the part from `state` up to the
// boxes is what comes back.
//
// fs_drive_slam is the same drive with stations of `stride` 7 doubles (a pose each; fs_drive: 3) and a DriveSlam:
// its own refusals after fs_drive's and before anything is written, its launches after every step's merge — the gate launch in
// place of the goal launch — and its results behind the same wait.  The slam_* pieces stand with the landmark sensor's host code.
}  // extern "C"

struct DriveSlam {
    const fs_landmark_sensor *lm_sensor;      // the caller's, or nullptr
    float *information;                       // the caller's outputs, each may be nullptr
    int32_t *voxels, *in_view, *n_new, *n_discovered;
    fs_landmark_sensor s;                     // resolved by slam_check
    fs_drive_slam_params p;                   // the caller's, or the defaults
    FsDriveSlamArgs a;                        // filled by slam_begin
    std::vector<float> Rt;                    // the stations' pose records, the host's until the drive's wait
    size_t T;
};
static int slam_check(fs_ctx *c, DriveSlam &g);
static int slam_begin(fs_ctx *c, DriveSlam &g, const double *pose7, size_t T, const FsDriveArgs &d);
static int slam_step(fs_ctx *c, DriveSlam &g, int32_t k);
static int slam_copy_back(fs_ctx *c, DriveSlam &g, std::vector<int32_t> &back);
static int slam_end(fs_ctx *c, DriveSlam &g, const std::vector<int32_t> &back, const int32_t *station_status);

static int drive_run(fs_ctx *c, int32_t n_robots, const double *station_xyz, int stride, const int32_t *n_stations, const int32_t *first_ray,
                     const double *goal_xyz, const fs_ray_params *sensor, const fs_drive_params *params, int32_t *status, int32_t *reached,
                     int32_t *station_status, int32_t *seen_unknown, int64_t *n_seen, int64_t *n_revealed, int32_t window[6], DriveSlam *slam)
{
    if (!c || n_robots < 0 || (n_robots > 0 && (!station_xyz || !n_stations || !goal_xyz || !status || !reached || !station_status || !seen_unknown)))
        return FS_E_INVALID;
    if (const int rc = sweep_state_check(c, sensor)) return rc;
    if (c->nz != 1) return fail(c, FS_E_INVALID, "fs_drive is defined on a 2-D costmap (nz == 1)");
    if (n_robots > FS_DRIVE_MAX_ROBOTS) return fail(c, FS_E_INVALID, "%d robots, at most %d", n_robots, FS_DRIVE_MAX_ROBOTS);
    const size_t R = (size_t)n_robots;
    size_t T = 0;
    int32_t K = 0;
    for (size_t r = 0; r < R; ++r) {
        if (n_stations[r] < 1) return fail(c, FS_E_INVALID, "n_stations[%zu] = %d: every robot needs a station", r, n_stations[r]);
        if (n_stations[r] > FS_DRIVE_MAX_STATIONS) return fail(c, FS_E_INVALID, "n_stations[%zu] = %d, at most %d", r, n_stations[r], FS_DRIVE_MAX_STATIONS);
        T += (size_t)n_stations[r];
        K = std::max(K, n_stations[r]);
    }
    const fs_drive_params dp = params ? *params : fs_drive_params{253, 254, 1};
    FsDriveArgs a{};
    const double *dir_was = c->sense_dir.data();
    if (const int rc = sweep_fan_setup(c, sensor, first_ray, T, a.sense, nullptr, nullptr, nullptr)) return rc;
    if (slam) {
        if (const int rc = slam_check(c, *slam)) return rc;
        c->ds_waits = c->sense_dir.data() != dir_was ? 1 : 0;    // (a sensor whose direction table was not the one on the device)
    }
    if (n_seen) *n_seen = 0;
    if (n_revealed) *n_revealed = 0;
    if (window) std::fill(window, window + 6, 0);
    if (R == 0) {
        if (slam && slam->n_new) *slam->n_new = 0;
        if (slam && slam->n_discovered) *slam->n_discovered = c->wl_discovered;
        return FS_OK;
    }

    if (const int rc = sweep_world_setup(c, sensor, a.sense)) return rc;
    // what a station can touch: its cell +- the fan's reach (an end point lies within depth of the pose, so its cell within
    // max_length + 2 of the pose's), clipped; empty for a station off the map.  It sizes the merge launch and says where the
    // keep-out zones are painted again — over more cells than the sweep saw, which repeats what is already painted there.
    const int32_t reach = (int32_t)std::min<unsigned int>(a.sense.max_length, (unsigned int)(c->nx + c->ny)) + 3;
    struct Win { int32_t x0, y0, x1, y1; };
    std::vector<int32_t> off(R);
    std::vector<Win> cons(T);
    {
        size_t t = 0;
        for (size_t r = 0; r < R; ++r) {
            off[r] = (int32_t)t;
            for (int32_t k = 0; k < n_stations[r]; ++k, ++t) {
                int32_t mx = 0, my = 0;
                if (grid_world_to_map(c, station_xyz[(size_t)stride * t], station_xyz[(size_t)stride * t + 1], mx, my))
                    cons[t] = Win{std::max(mx - reach, 0), std::max(my - reach, 0), std::min(mx + reach, c->nx - 1), std::min(my + reach, c->ny - 1)};
                else
                    cons[t] = Win{c->nx, c->ny, -1, -1};
            }
        }
    }
    const size_t o_n = 0, o_off = R, o_state = 2 * R, o_union = 4 * R, o_status = 4 * R + 4, o_seen = o_status + T, o_box = o_seen + T,
                 o_first = o_box + 4 * T, n_i32 = o_first + (first_ray ? T : 0), n_back = o_box - o_state;
    std::vector<int32_t> h(n_i32);
    for (size_t r = 0; r < R; ++r) {
        h[o_n + r] = n_stations[r]; h[o_off + r] = off[r];
        h[o_state + 2 * r] = FS_DRIVE_DRIVING; h[o_state + 2 * r + 1] = 0;
    }
    h[o_union] = c->nx; h[o_union + 1] = c->ny; h[o_union + 2] = -1; h[o_union + 3] = -1;
    for (size_t t = 0; t < T; ++t) {
        h[o_status + t] = -1; h[o_seen + t] = 0;
        h[o_box + 4 * t] = c->nx; h[o_box + 4 * t + 1] = c->ny; h[o_box + 4 * t + 2] = -1; h[o_box + 4 * t + 3] = -1;
    }
    if (first_ray) std::copy(first_ray, first_ray + T, h.begin() + (std::ptrdiff_t)o_first);
    std::vector<double> xyz(3 * (T + R));
    for (size_t t = 0; t < T; ++t) std::copy(station_xyz + (size_t)stride * t, station_xyz + (size_t)stride * t + 3, xyz.begin() + (std::ptrdiff_t)(3 * t));
    std::copy(goal_xyz, goal_xyz + 3 * R, xyz.begin() + (std::ptrdiff_t)(3 * T));
    FS_HIP(c, c->d_drive_xyz.ensure(xyz.size())); FS_HIP(c, c->d_drive_i32.ensure(n_i32)); FS_HIP(c, c->d_sense_counts.ensure(4));
    FS_HIP(c, hipMemcpyAsync(c->d_drive_xyz.p, xyz.data(), xyz.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    FS_HIP(c, hipMemcpyAsync(c->d_drive_i32.p, h.data(), n_i32 * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    FS_HIP(c, hipMemsetAsync(c->d_sense_counts.p, 0, 2 * sizeof(unsigned long long), c->stream));
    int32_t *const d = c->d_drive_i32.p;
    a.sense.n = (int32_t)T;
    a.sense.origin = c->d_drive_xyz.p;
    a.sense.first_ray = first_ray ? d + o_first : nullptr;
    a.sense.mark = c->d_sense_mark.p;
    a.sense.ray_unknown = nullptr;
    a.sense.box = nullptr;
    a.sense.status = d + o_status;
    a.sense.seen_unknown = d + o_seen;
    a.staged = grid_dev(c);
    a.staged.cls = nullptr;
    a.n_robots = n_robots;
    a.n_stations = d + o_n; a.station_off = d + o_off;
    a.goal = c->d_drive_xyz.p + 3 * T;
    a.block_min = dp.block_min; a.block_max = dp.block_max;
    a.move_max_length = (double)c->nx + (double)c->ny;
    a.state = d + o_state; a.station_box = d + o_box; a.union_box = d + o_union;
    a.counts = c->d_sense_counts.p;
    if (slam)
        if (const int rc = slam_begin(c, *slam, station_xyz, T, a)) return rc;

    ++c->grid_gen;
    Win all{c->nx, c->ny, -1, -1};
    for (int32_t k = 0; k < K; ++k) {
        Win w{c->nx, c->ny, -1, -1};
        unsigned long long most = 0;
        for (size_t r = 0; r < R; ++r) {
            if (k >= n_stations[r]) continue;
            const Win &s = cons[(size_t)off[r] + (size_t)k];
            if (s.x1 < s.x0) continue;
            w = Win{std::min(w.x0, s.x0), std::min(w.y0, s.y0), std::max(w.x1, s.x1), std::max(w.y1, s.y1)};
            most = std::max(most, (unsigned long long)(s.x1 - s.x0 + 1) * (unsigned long long)(s.y1 - s.y0 + 1));
        }
        a.step = k;
        FS_HIP(c, fs_launch_drive_step(a, c->stream));
        if (w.x1 >= w.x0) {
            FS_HIP(c, fs_launch_drive_merge(a, (unsigned)((most + 255ull) / 256ull), c->stream));
            if (const int rc = ko_repaint_window(c, w.x0, w.y0, w.x1 - w.x0 + 1, w.y1 - w.y0 + 1)) return rc;
            all = Win{std::min(all.x0, w.x0), std::min(all.y0, w.y0), std::max(all.x1, w.x1), std::max(all.y1, w.y1)};
        }
        if (slam) { if (const int rc = slam_step(c, *slam, k)) return rc; }
        else if (dp.stop_when_mapped) FS_HIP(c, fs_launch_drive_goal(a, c->stream));
    }
    // once, for everything the drive can have touched (an empty box where every station was off the map)
    if (const int rc = cells_changed_in_box(c, all.x0, all.y0, 0, all.x1 - all.x0 + 1, all.y1 - all.y0 + 1, 1)) return rc;
    std::vector<int32_t> back(n_back);
    unsigned long long counts[2] = {0ull, 0ull};
    FS_HIP(c, hipMemcpyAsync(back.data(), d + o_state, n_back * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipMemcpyAsync(counts, c->d_sense_counts.p, sizeof counts, hipMemcpyDeviceToHost, c->stream));
    std::vector<int32_t> slam_back;
    if (slam)
        if (const int rc = slam_copy_back(c, *slam, slam_back)) return rc;
    FS_HIP(c, hipStreamSynchronize(c->stream));                  // (the one wait of the call)
    c->sense_mark_clean = true;
    ++c->epoch;
    for (size_t r = 0; r < R; ++r) {
        const int32_t st = back[2 * r];
        status[r] = st == FS_DRIVE_DRIVING ? FS_DRIVE_ARRIVED : st;           // still driving after the last step: out of stations
        reached[r] = back[2 * r + 1];
    }
    const int32_t *ub = back.data() + (o_union - o_state);
    std::copy(back.begin() + (std::ptrdiff_t)(o_status - o_state), back.begin() + (std::ptrdiff_t)(o_seen - o_state), station_status);
    std::copy(back.begin() + (std::ptrdiff_t)(o_seen - o_state), back.end(), seen_unknown);
    if (n_seen) *n_seen = (int64_t)counts[0];
    if (n_revealed) *n_revealed = (int64_t)counts[1];
    if (window && ub[2] >= ub[0]) { window[0] = ub[0]; window[1] = ub[1]; window[2] = 0; window[3] = ub[2] - ub[0] + 1; window[4] = ub[3] - ub[1] + 1; window[5] = 1; }
    return slam ? slam_end(c, *slam, slam_back, station_status) : FS_OK;
}

extern "C" {

int fs_drive(fs_ctx *c, int32_t n_robots, const double *station_xyz, const int32_t *n_stations, const int32_t *first_ray, const double *goal_xyz,
             const fs_ray_params *sensor, const fs_drive_params *params, int32_t *status, int32_t *reached, int32_t *station_status,
             int32_t *seen_unknown, int64_t *n_seen, int64_t *n_revealed, int32_t window[6])
{
    return drive_run(c, n_robots, station_xyz, 3, n_stations, first_ray, goal_xyz, sensor, params, status, reached, station_status, seen_unknown,
                     n_seen, n_revealed, window, nullptr);
}

int fs_grid_census(fs_ctx *c, int64_t counts[4])
{
    if (!c || !counts) return FS_E_INVALID;
    if (const int rc = grid_check(c)) return rc;
    unsigned long long v[4] = {0ull, 0ull, 0ull, 0ull};
    FS_HIP(c, c->d_sense_counts.ensure(4));
    FS_HIP(c, hipMemsetAsync(c->d_sense_counts.p, 0, sizeof v, c->stream));
    FS_HIP(c, fs_launch_grid_census(c->d_cells.p, (size_t)c->nx * (size_t)c->ny * (size_t)c->nz, c->d_sense_counts.p, c->stream));
    FS_HIP(c, hipMemcpyAsync(v, c->d_sense_counts.p, sizeof v, hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipStreamSynchronize(c->stream));
    for (int k = 0; k < 4; ++k) counts[k] = (int64_t)v[k];
    return FS_OK;
}

int fs_frontier_clusters(fs_ctx *c, const double robot_xy[2], int32_t lethal_threshold, double max_frontier_distance,
                         int32_t max_frontier_cluster_size, int32_t *labels, int32_t max_clusters,
                         fs_frontier_cluster *clusters, int32_t *n_clusters, int64_t *n_cells)
{
    if (!c || !robot_xy || !n_clusters || max_clusters < 0 || (max_clusters > 0 && !clusters)) return FS_E_INVALID;
    int rc = grid2d_check(c, "the frontier search");
    if (rc) return rc;
    *n_clusters = 0;
    if (n_cells) *n_cells = 0;
    const size_t cells = (size_t)c->nx * c->ny;
    // :26-33 — worldToMap of the robot position; off the map: no frontiers
    int32_t mx = 0, my = 0;
    if (!grid_world_to_map(c, robot_xy[0], robot_xy[1], mx, my)) {
        if (labels) std::fill(labels, labels + cells, -1);
        return FS_OK;
    }
    rc = fc_ensure(c, labels != nullptr, max_clusters);
    if (rc) return rc;
    rc = fc_launch(c, robot_xy, (int32_t)((unsigned int)my * (unsigned int)c->nx + (unsigned int)mx), max_frontier_distance,
                   max_frontier_cluster_size, lethal_threshold, labels != nullptr, max_clusters);
    if (rc) return rc;
    // results through the page-locked buffer: the counters, the first clusters (as many as a map of this size usually has) and
    // the labels are requested together and waited for once; only a map with more clusters costs a second round trip
    const size_t first = (size_t)std::min<int32_t>(max_clusters, 4096);
    const size_t o_state = 0, o_cl = 64, o_labels = (o_cl + first * sizeof(fs_frontier_cluster) + 63) & ~(size_t)63;
    FS_HIP(c, c->h_out.ensure(o_labels + (labels ? sizeof(int32_t) * cells : 0)));
    FS_HIP(c, hipMemcpyAsync(c->h_out.p + o_state, c->d_fc_state.p, 8 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (first) FS_HIP(c, hipMemcpyAsync(c->h_out.p + o_cl, c->d_fc_clusters.p, first * sizeof(fs_frontier_cluster), hipMemcpyDeviceToHost, c->stream));
    if (labels) FS_HIP(c, hipMemcpyAsync(c->h_out.p + o_labels, c->d_fc_labels.p, sizeof(int32_t) * cells, hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipStreamSynchronize(c->stream));
    int32_t state[8];
    std::memcpy(state, c->h_out.p + o_state, sizeof state);
    if (labels) std::memcpy(labels, c->h_out.p + o_labels, sizeof(int32_t) * cells);
    const int32_t stored = std::min(state[5], max_clusters);
    if (stored > 0) {
        std::memcpy(clusters, c->h_out.p + o_cl, sizeof(fs_frontier_cluster) * std::min<size_t>((size_t)stored, first));
        if ((size_t)stored > first) {
            FS_HIP(c, hipMemcpyAsync(clusters + first, c->d_fc_clusters.p + first, sizeof(fs_frontier_cluster) * ((size_t)stored - first), hipMemcpyDeviceToHost, c->stream));
            FS_HIP(c, hipStreamSynchronize(c->stream));
        }
        // slots were handed out in arrival order: present the clusters by ascending label
        std::sort(clusters, clusters + stored, [](const fs_frontier_cluster &u, const fs_frontier_cluster &v) { return u.label < v.label; });
    }
    *n_clusters = state[5];
    if (n_cells) *n_cells = state[6];
    if (c->d_fc_labels.cap * sizeof(int32_t) > ((size_t)64 << 20)) c->d_fc_labels.release();   // (same rule as the stencil mask and the brick list)
    return FS_OK;
}

}  // extern "C"

namespace {

// fs_search_frontiers up to its results: fs_frontier_clusters' kernels (no cluster records, no labels), then fs_search.hip's stage.
// Not synchronised.  *on_map = false: the robot is off the map and nothing was enqueued.  want_cols: the scoring calls' goal
// [records][3] and size [records] columns are written too (d_fs_goal, d_fs_fsize); *args_out: the stage's arguments.
int search_enqueue(fs_ctx *c, const double robot_xy[2], int32_t lethal_threshold, double max_frontier_distance, int32_t min_size,
                   int32_t max_size, int32_t n_seeds, const int32_t *seeds, bool want_every, bool *on_map_out,
                   bool want_cols = false, FsSearchArgs *args_out = nullptr)
{
    *on_map_out = false;
    if (!robot_xy) return fail(c, FS_E_INVALID, "null robot position");
    if (min_size < 0 || max_size < 1) return fail(c, FS_E_INVALID, "min_frontier_cluster_size >= 0 and max_frontier_cluster_size >= 1");
    if (seeds && n_seeds < 0) return fail(c, FS_E_INVALID, "n_seeds < 0");
    int rc = grid2d_check(c, "the frontier search");
    if (rc) return rc;
    const size_t cells = (size_t)c->nx * c->ny;
    if (seeds) {
        if ((size_t)n_seeds > cells) return fail(c, FS_E_INVALID, "more seeds than cells");
        for (int32_t k = 0; k < n_seeds; ++k)
            if (seeds[k] < 0 || (size_t)seeds[k] >= cells) return fail(c, FS_E_INVALID, "seed %d: cell %d is off the map", k, seeds[k]);
    }
    // :26-33 — worldToMap of the robot position (as fs_frontier_clusters)
    int32_t mx = 0, my = 0;
    c->fs_outer = !seeds && c->fs_seed_order == FS_SEEDS_REFERENCE;
    if (c->fs_outer) c->fs_outer_levels = c->fs_outer_popped = 0;
    if (!grid_world_to_map(c, robot_xy[0], robot_xy[1], mx, my)) return FS_OK;
    const int32_t robot_cell = (int32_t)((unsigned int)my * (unsigned int)c->nx + (unsigned int)mx);
    const size_t nb = (cells + 1023) / 1024, ne = std::max(cells, (size_t)(seeds ? n_seeds : 0)) + 1;
    rc = fc_ensure(c, false, 0);
    if (rc) return rc;
    FS_HIP(c, c->d_fs_bcount.ensure(nb + 1)); FS_HIP(c, c->d_fs_cidx.ensure(cells)); FS_HIP(c, c->d_fs_root.ensure(cells));
    FS_HIP(c, c->d_fs_best_idx.ensure(cells)); FS_HIP(c, c->d_fs_csize.ensure(cells)); FS_HIP(c, c->d_fs_owner.ensure(cells));
    FS_HIP(c, c->d_fs_key.ensure(cells)); FS_HIP(c, c->d_fs_pos.ensure(cells)); FS_HIP(c, c->d_fs_q.ensure(cells));
    FS_HIP(c, c->d_fs_state.ensure(16)); FS_HIP(c, c->d_fs_best_d2.ensure(cells));
    FS_HIP(c, c->d_fs_emit_comp.ensure(ne)); FS_HIP(c, c->d_fs_emit_seed.ensure(ne)); FS_HIP(c, c->d_fs_emit_base.ensure(ne));
    FS_HIP(c, c->d_fs_rec_base.ensure(ne)); FS_HIP(c, c->d_fs_sort.ensure(cells)); FS_HIP(c, c->d_fs_rec.ensure(cells));
    if (want_every) FS_HIP(c, c->d_fs_every.ensure(2 * cells));
    if (want_cols) { FS_HIP(c, c->d_fs_goal.ensure(3 * cells)); FS_HIP(c, c->d_fs_fsize.ensure(cells)); }
    if (seeds && n_seeds > 0) {
        FS_HIP(c, c->d_fs_seeds.ensure((size_t)n_seeds));
        FS_HIP(c, hipMemcpyAsync(c->d_fs_seeds.p, seeds, sizeof(int32_t) * (size_t)n_seeds, hipMemcpyHostToDevice, c->stream));
    }
    FS_HIP(c, hipMemsetAsync(c->d_fs_state.p, 0, 16 * sizeof(int32_t), c->stream));
    rc = fc_launch(c, robot_xy, robot_cell, max_frontier_distance, max_size, lethal_threshold, false, 0);
    if (rc) return rc;
    FsSearchArgs a{};
    a.parent_f = c->d_fc_parent_f.p; a.aux = c->d_fc_aux.p;
    a.nx = c->nx; a.ny = c->ny; a.ox = c->origin[0]; a.oy = c->origin[1]; a.res = c->res;
    a.robot_cell = robot_cell;
    // a component has at most nx * ny cells, so every max_size >= nx * ny cuts exactly as nx * ny does (and max + 1 cannot wrap)
    a.min_size = min_size; a.max_size = (int32_t)std::min<int64_t>(max_size, (int64_t)cells);
    a.n_seeds = seeds ? n_seeds : -1; a.seeds = c->d_fs_seeds.p;
    a.outer = c->fs_outer ? 1 : 0; a.parent_t = c->d_fc_parent_t.p; a.fc_state = c->d_fc_state.p;
    a.bcount = c->d_fs_bcount.p; a.cidx = c->d_fs_cidx.p; a.comp_root = c->d_fs_root.p; a.best_idx = c->d_fs_best_idx.p;
    a.csize = c->d_fs_csize.p; a.owner = c->d_fs_owner.p; a.best_d2 = c->d_fs_best_d2.p;
    a.emit_comp = c->d_fs_emit_comp.p; a.emit_seed = c->d_fs_emit_seed.p; a.emit_base = c->d_fs_emit_base.p; a.rec_base = c->d_fs_rec_base.p;
    a.key = c->d_fs_key.p; a.pos = c->d_fs_pos.p; a.q = c->d_fs_q.p; a.sortbuf = c->d_fs_sort.p; a.rec = c->d_fs_rec.p;
    a.goal_xyz = want_cols ? c->d_fs_goal.p : nullptr; a.fsize = want_cols ? c->d_fs_fsize.p : nullptr;
    a.every = want_every ? c->d_fs_every.p : nullptr;
    a.state = c->d_fs_state.p;
    {
        ScopedTimer t(c, 9);
        FS_HIP(c, fs_launch_frontier_search(a, c->stream));
    }
    if (args_out) *args_out = a;
    *on_map_out = true;
    return FS_OK;
}

// the search's results: the counts and the first records in one round trip; more records than the first round holds, and the
// every list, in a second.  *n_records / *n_cells are what was found.
int search_results(fs_ctx *c, int32_t max_records, fs_frontier_record *records, int32_t *n_records, int64_t max_every, double *every_xy,
                   int64_t *n_cells)
{
    const size_t first = (size_t)std::min<int32_t>(max_records, 1024);
    const size_t o_rec = 64;
    FS_HIP(c, c->h_out.ensure(o_rec + first * sizeof(fs_frontier_record)));
    FS_HIP(c, hipMemcpyAsync(c->h_out.p, c->d_fs_state.p, 16 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (first) FS_HIP(c, hipMemcpyAsync(c->h_out.p + o_rec, c->d_fs_rec.p, first * sizeof(fs_frontier_record), hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipStreamSynchronize(c->stream));
    int32_t state[16];
    std::memcpy(state, c->h_out.p, sizeof state);
    c->fs_levels = state[FSS_LEVELS];
    c->fs_guarded = state[FSS_GUARDED];
    if (c->fs_outer) { c->fs_outer_levels = state[FSS_OUTER_LEVELS]; c->fs_outer_popped = state[FSS_OUTER_POPPED]; }
    if (state[FSS_ERROR] == 2) return fail(c, FS_E_HIP, "internal error: the outer search did not meet every component the clustering found");
    if (state[FSS_ERROR]) return fail(c, FS_E_INVALID, "a seed is not a frontier cell the search found, or two seeds share a component");
    const int32_t n = state[FSS_RECORDS], stored = std::min(n, max_records);
    if (stored > 0) {
        std::memcpy(records, c->h_out.p + o_rec, sizeof(fs_frontier_record) * std::min<size_t>((size_t)stored, first));
        if ((size_t)stored > first)
            FS_HIP(c, hipMemcpyAsync(records + first, c->d_fs_rec.p + first, sizeof(fs_frontier_record) * ((size_t)stored - first), hipMemcpyDeviceToHost, c->stream));
    }
    const int64_t every = std::min<int64_t>(state[FSS_CELLS], max_every);
    if (every_xy && every > 0) FS_HIP(c, hipMemcpyAsync(every_xy, c->d_fs_every.p, 2 * sizeof(double) * (size_t)every, hipMemcpyDeviceToHost, c->stream));
    if ((size_t)stored > first || (every_xy && every > 0)) FS_HIP(c, hipStreamSynchronize(c->stream));
    *n_records = n;
    if (n_cells) *n_cells = state[FSS_CELLS];
    return FS_OK;
}

// The list of fs_get_frontier_costs_searched / _searched_roadmap: the search writes the goal and size columns where the planner and
// the scorer read them, the blacklist is matched there too (d_fs_black), and the found records come up — the count (which sizes
// every launch that follows) with the first round, a list longer than that round holds at the price of a second.  *on_map = false:
// the robot is off the map, nothing ran and *n stays as it is.  More than max_records: *n is set and the call refuses.
int searched_list(fs_ctx *c, const double robot_pose7[7], int32_t lethal_threshold, double max_frontier_distance, int32_t min_size,
                  int32_t max_size, int32_t n_blacklist, const double *blacklist_xy, int32_t max_records, bool *on_map, int32_t *n,
                  std::vector<fs_frontier_record> &found)
{
    FsSearchArgs sa{};
    int rc = search_enqueue(c, robot_pose7, lethal_threshold, max_frontier_distance, min_size, max_size, 0, nullptr, false, on_map, true, &sa);
    if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
    if (!*on_map) return FS_OK;
    const size_t cells = (size_t)c->nx * c->ny;
    FS_HIP(c, c->d_fs_black.ensure(cells));
    if (n_blacklist > 0) {
        FS_HIP(c, c->d_fs_black_xy.ensure(2 * (size_t)n_blacklist));
        FS_HIP(c, hipMemcpyAsync(c->d_fs_black_xy.p, blacklist_xy, 16 * (size_t)n_blacklist, hipMemcpyHostToDevice, c->stream));
    }
    FS_HIP(c, fs_launch_search_blacklist(sa, c->d_fs_black_xy.p, n_blacklist, c->d_fs_black.p, c->stream));
    std::vector<fs_frontier_record> first((size_t)std::min<int32_t>(max_records, 1024));
    found.swap(first);
    int32_t count = 0;
    rc = search_results(c, (int32_t)found.size(), found.data(), &count, 0, nullptr, nullptr);
    if (rc) return rc;
    *n = count;
    if (count > max_records) return fail(c, FS_E_INVALID, "%d frontiers found, room for %d: no partial ranking", count, max_records);
    if ((size_t)count > found.size()) {
        const size_t have = found.size();
        found.resize((size_t)count);
        FS_HIP(c, hipMemcpyAsync(found.data() + have, c->d_fs_rec.p + have, sizeof(fs_frontier_record) * ((size_t)count - have), hipMemcpyDeviceToHost, c->stream));
        FS_HIP(c, hipStreamSynchronize(c->stream));
    }
    return FS_OK;
}

}  // namespace

extern "C" {

int fs_search_frontiers(fs_ctx *c, const double robot_xy[2], int32_t lethal_threshold, double max_frontier_distance,
                        int32_t min_frontier_cluster_size, int32_t max_frontier_cluster_size, int32_t n_seeds, const int32_t *seeds,
                        int32_t max_records, fs_frontier_record *records, int32_t *n_records,
                        int64_t max_every, double *every_xy, int64_t *n_cells)
{
    if (!c) return FS_E_INVALID;
    if (!n_records || max_records < 0 || (max_records > 0 && !records) || max_every < 0) return fail(c, FS_E_INVALID, "null pointer or negative capacity");
    *n_records = 0;
    if (n_cells) *n_cells = 0;
    bool on_map = false;
    const int rc = search_enqueue(c, robot_xy, lethal_threshold, max_frontier_distance, min_frontier_cluster_size, max_frontier_cluster_size,
                                  n_seeds, seeds, every_xy != nullptr && max_every > 0, &on_map);
    if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
    if (!on_map) return FS_OK;
    return search_results(c, max_records, records, n_records, max_every, every_xy, n_cells);
}

int fs_set_frontier_seed_order(fs_ctx *c, int32_t order)
{
    if (!c) return FS_E_INVALID;
    if (order != FS_SEEDS_NEAREST && order != FS_SEEDS_REFERENCE) return fail(c, FS_E_INVALID, "unknown frontier seed order %d", order);
    c->fs_seed_order = order;
    return FS_OK;
}

int fs_set_arrival_limits(fs_ctx *c, double max_gt, double min_gt)
{
    if (!c) return FS_E_INVALID;
    c->max_gt = max_gt; c->min_gt = min_gt;
    ++c->epoch;
    return FS_OK;
}

int fs_max_arrival(fs_ctx *c, double *max_value, double *max_gt, double *min_gt)
{
    if (!c) return FS_E_INVALID;
    FS_HIP(c, hipSetDevice(c->device));
    int rc = check_scoring_state(c, true, false);
    if (rc) return rc;
    FsRayArgs a{};
    if (const int rc_args = fill_ray_args(c, a, false)) return rc_args;     // (another visitor than the one a class image is cut for)
    // DEP/src/CostCalculator.cpp:140 visitor (260,260,0,255); :142-148 no clamping; start (0,0)
    a.obst_min = 260; a.obst_max = 260; a.trace_min = 0; a.trace_max = 255;
    a.clamp = 0;
    a.min_gt = 0.0;
    a.footprint_radius = 0.0;
    const double zcal = (c->nz > 1) ? c->origin[2] + 0.5 * c->nz * c->res : c->origin[2];
    const double goal[3] = {0.0, 0.0, zcal};
    FS_HIP(c, c->d_goal.ensure(3));
    rc = ensure_candidate_scratch(c, 1, false);
    if (rc) return rc;
    FS_HIP(c, hipMemcpyAsync(c->d_goal.p, goal, sizeof goal, hipMemcpyHostToDevice, c->stream));
    a.n = 1; a.goal = c->d_goal.p;
    a.arrival = c->d_arrival.p; a.argmax = c->d_argmax.p; a.status = c->d_status.p;
    a.yaw = c->d_yaw.p; a.achievable = c->d_ach.p;
    {
        ScopedTimer t(c, 0);
        FS_HIP(c, fs_launch_raymarch(a, c->stream));
    }
    int32_t arrival = 0, status = 0;
    FS_HIP(c, hipMemcpyAsync(&arrival, c->d_arrival.p, 4, hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipMemcpyAsync(&status, c->d_status.p, 4, hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipStreamSynchronize(c->stream));
    if (status != FS_STATUS_OK) {
        // :145-148 — returns 0 and leaves the limits unset
        if (max_value) *max_value = 0.0;
        if (max_gt) *max_gt = c->max_gt;
        if (min_gt) *min_gt = c->min_gt;
        return FS_OK;
    }
    c->max_gt = arrival * c->rp.factor_max;           // :186
    c->min_gt = c->rp.factor_min * c->max_gt;         // :188
    ++c->epoch;
    if (max_value) *max_value = (double)arrival;
    if (max_gt) *max_gt = c->max_gt;
    if (min_gt) *min_gt = c->min_gt;
    return FS_OK;
}

// Spatial processing order for the ray-march kernel (outputs stay in list order).  Small lists are not worth a sort.
static int maybe_sort(fs_ctx *c, FsRayArgs &a)
{
    a.perm = nullptr;
    c->sort_keys = nullptr; c->sort_costmap = nullptr;
    if (!c->opt_sort || a.n < 2048) return FS_OK;
    FS_HIP(c, c->d_perm.ensure(a.n));
    ScopedTimer t(c, 4);
    FS_HIP(c, fs_launch_sort_candidates(a.n, a.goal, a.grid, c->d_perm.p, &c->sort_scratch, &c->sort_scratch_bytes,
                                        c->d_counters.p + 10, &c->sort_keys, &c->sort_costmap, c->opt_costmap ? 1 : 0, c->opt_sort_reverse ? 1 : 0, c->stream));
    a.perm = c->d_perm.p;
    return FS_OK;
}

static int upload_candidates(fs_ctx *c, int32_t n, const double *goal_xyz, const int32_t *fsize,
                             const uint8_t *black, const uint8_t *achin)
{
    // the columns are packed into the context's page-locked buffer (every host-buffer entry point synchronises before it
    // returns, so the previous call's transfer out of that buffer is over) and travel as ONE transfer into a device buffer of
    // the same layout: goal | frontier size | blacklist | achievable
    const size_t nn = (size_t)n, pad = (nn + 15) & ~(size_t)15;
    const size_t o_goal = 0, o_fsize = o_goal + 24 * nn, o_black = ((o_fsize + 4 * nn) + 15) & ~(size_t)15, o_achin = o_black + pad;
    const size_t total = o_achin + pad;
    FS_HIP(c, c->h_in.ensure(total));
    FS_HIP(c, c->d_in.ensure(total));
    std::memcpy(c->h_in.p + o_goal, goal_xyz, 24 * nn);
    if (fsize) std::memcpy(c->h_in.p + o_fsize, fsize, 4 * nn);
    if (black) std::memcpy(c->h_in.p + o_black, black, nn);
    if (achin) std::memcpy(c->h_in.p + o_achin, achin, nn);
    const size_t used = achin ? total : (black ? o_black + pad : (fsize ? o_fsize + 4 * nn : 24 * nn));
    // a short list is read by the kernels where it lies (mapped page-locked memory): no transfer of its own
    const bool in_place = c->opt_zero_copy && n <= FS_ZERO_COPY_MAX_N && c->h_in.dev;
    const char *base = in_place ? c->h_in.dev : c->d_in.p;
    if (!in_place) FS_HIP(c, hipMemcpyAsync(c->d_in.p, c->h_in.p, used, hipMemcpyHostToDevice, c->stream));
    c->in_goal = reinterpret_cast<const double *>(base + o_goal);
    c->in_fsize = fsize ? reinterpret_cast<const int32_t *>(base + o_fsize) : nullptr;
    c->in_black = black ? reinterpret_cast<const uint8_t *>(base + o_black) : nullptr;
    c->in_achin = achin ? reinterpret_cast<const uint8_t *>(base + o_achin) : nullptr;
    return FS_OK;
}

// fs_score_arrival in two halves (see fs_score_candidates_begin / _end): everything up to the copies into the caller's
// buffers is issued here ...
int fs_score_arrival_begin(fs_ctx *c, int32_t n, const double *goal_xyz, const int32_t *frontier_size,
                           const uint8_t *blacklisted, const uint8_t *achievable_in,
                           int32_t *ray_counts, int32_t *arrival, int32_t *argmax, double *yaw,
                           uint8_t *achievable, int32_t *status)
{
    if (!c) return FS_E_INVALID;
    FS_HIP(c, hipSetDevice(c->device));
    int rc = check_scoring_state(c, true, false);
    if (rc) return rc;
    if (n < 0 || (n > 0 && (!goal_xyz || !arrival || !argmax || !yaw || !achievable || !status)))
        return fail(c, FS_E_INVALID, "null output or input pointer");
    if (n == 0) return FS_OK;
    rc = upload_candidates(c, n, goal_xyz, frontier_size, blacklisted, achievable_in);
    if (rc) return rc;
    rc = ensure_candidate_scratch(c, n, false);
    if (rc) return rc;
    const size_t per = (size_t)c->n_yaw * c->n_elev;
    if (ray_counts) FS_HIP(c, c->d_raycounts.ensure((size_t)n * per));
    FsRayArgs a{};
    if (const int rc_args = fill_ray_args(c, a)) return rc_args;
    a.n = n; a.goal = c->in_goal;
    a.frontier_size = c->in_fsize;
    a.blacklisted = c->in_black;
    a.achievable_in = c->in_achin;
    a.ray_counts = ray_counts ? c->d_raycounts.p : nullptr;
    a.arrival = c->d_arrival.p; a.argmax = c->d_argmax.p; a.status = c->d_status.p;
    a.yaw = c->d_yaw.p; a.achievable = c->d_ach.p;
    // a short list: the kernel writes its five result columns straight into the mapped page-locked buffer (five transfers less;
    // the per-ray counts, if asked for, are the one column large enough to keep its transfer)
    {
        const size_t nn0 = (size_t)n;
        const size_t o_arr = 0, o_arg = o_arr + ((4 * nn0 + 15) & ~(size_t)15), o_st = o_arg + ((4 * nn0 + 15) & ~(size_t)15);
        const size_t o_yaw = o_st + ((4 * nn0 + 15) & ~(size_t)15), o_ach = o_yaw + ((8 * nn0 + 15) & ~(size_t)15), o_rc = o_ach + ((nn0 + 15) & ~(size_t)15);
        FS_HIP(c, c->h_out.ensure(o_rc + (ray_counts ? 4 * nn0 * per : 0)));
        if (c->opt_zero_copy && n <= FS_ZERO_COPY_MAX_N && c->h_out.dev) {
            char *hd = c->h_out.dev;
            a.arrival = reinterpret_cast<int32_t *>(hd + o_arr); a.argmax = reinterpret_cast<int32_t *>(hd + o_arg);
            a.status = reinterpret_cast<int32_t *>(hd + o_st); a.yaw = reinterpret_cast<double *>(hd + o_yaw);
            a.achievable = reinterpret_cast<uint8_t *>(hd + o_ach);
            rc = maybe_sort(c, a);
            if (rc) return rc;
            {
                ScopedTimer t(c, 0);
                FS_HIP(c, fs_launch_raymarch(a, c->stream));
            }
            c->arrival_pending.clear();
            if (ray_counts) {
                FS_HIP(c, hipMemcpyAsync(c->h_out.p + o_rc, c->d_raycounts.p, 4 * nn0 * per, hipMemcpyDeviceToHost, c->stream));
                c->arrival_pending.push_back({ray_counts, o_rc, 4 * nn0 * per});
            }
            c->arrival_pending.push_back({arrival, o_arr, 4 * nn0}); c->arrival_pending.push_back({argmax, o_arg, 4 * nn0});
            c->arrival_pending.push_back({status, o_st, 4 * nn0}); c->arrival_pending.push_back({yaw, o_yaw, 8 * nn0});
            c->arrival_pending.push_back({achievable, o_ach, nn0});
            return FS_OK;
        }
    }
    rc = maybe_sort(c, a);
    if (rc) return rc;
    {
        ScopedTimer t(c, 0);
        FS_HIP(c, fs_launch_raymarch(a, c->stream));
    }
    // The columns come back through the context's page-locked buffer: a copy into the caller's pageable arrays (std::vector in
    // the ROS adapter, numpy in the binding) would make every one of these calls host-synchronous — `begin` would return only
    // when this device is done, and fs_multi_score_arrival would run its devices one after the other.
    struct Col { void *host; const void *dev; size_t bytes; };
    const size_t nn = (size_t)n;
    const Col cols[6] = {{ray_counts, c->d_raycounts.p, 4 * nn * per}, {arrival, c->d_arrival.p, 4 * nn}, {argmax, c->d_argmax.p, 4 * nn},
                         {status, c->d_status.p, 4 * nn}, {yaw, c->d_yaw.p, 8 * nn}, {achievable, c->d_ach.p, nn}};
    size_t total = 0;
    for (const Col &col : cols) if (col.host) total += (col.bytes + 15) & ~(size_t)15;
    FS_HIP(c, c->h_out.ensure(total));
    c->arrival_pending.clear();
    size_t off = 0;
    for (const Col &col : cols) {
        if (!col.host) continue;
        FS_HIP(c, hipMemcpyAsync(c->h_out.p + off, col.dev, col.bytes, hipMemcpyDeviceToHost, c->stream));
        c->arrival_pending.push_back({col.host, off, col.bytes});
        off += (col.bytes + 15) & ~(size_t)15;
    }
    return FS_OK;
}

// ... and waited for here: one synchronisation, then the columns go to the caller's arrays
int fs_score_arrival_end(fs_ctx *c)
{
    if (!c) return FS_E_INVALID;
    FS_HIP(c, hipSetDevice(c->device));
    const hipError_t e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { c->arrival_pending.clear(); return fail(c, FS_E_HIP, "hipStreamSynchronize: %s", hipGetErrorString(e)); }
    for (const fs_ctx::PendingCol &col : c->arrival_pending) std::memcpy(col.host, c->h_out.p + col.off, col.bytes);
    c->arrival_pending.clear();
    return FS_OK;
}

int fs_score_arrival(fs_ctx *c, int32_t n, const double *goal_xyz, const int32_t *frontier_size,
                     const uint8_t *blacklisted, const uint8_t *achievable_in,
                     int32_t *ray_counts, int32_t *arrival, int32_t *argmax, double *yaw,
                     uint8_t *achievable, int32_t *status)
{
    const int rc = fs_score_arrival_begin(c, n, goal_xyz, frontier_size, blacklisted, achievable_in, ray_counts, arrival, argmax, yaw, achievable, status);
    if (rc || n == 0) return rc;
    return fs_score_arrival_end(c);
}

int fs_trace_segments(fs_ctx *c, int32_t n, const double *start_xyz, const double *end_xyz, double max_length_cells,
                      int32_t obst_min, int32_t obst_max, int32_t trace_min, int32_t trace_max,
                      uint8_t *ok, int32_t *traced, uint8_t *hit, int32_t *unknown, int32_t *all)
{
    if (!c) return FS_E_INVALID;
    if (const int rc = grid_check(c)) return rc;
    if (n < 0 || (n > 0 && (!start_xyz || !end_xyz || !ok || !traced || !hit || !unknown || !all))) return fail(c, FS_E_INVALID, "null pointer");
    if (n == 0) return FS_OK;
    DevBuf<double> &d_s = c->d_seg_start, &d_e = c->d_seg_end;
    DevBuf<uint8_t> &d_ok = c->d_seg_ok, &d_hit = c->d_seg_hit;
    DevBuf<int32_t> &d_tr = c->d_seg_traced, &d_un = c->d_seg_unknown, &d_all = c->d_seg_all;
    FS_HIP(c, d_s.ensure((size_t)n * 3)); FS_HIP(c, d_e.ensure((size_t)n * 3));
    FS_HIP(c, d_ok.ensure(n)); FS_HIP(c, d_hit.ensure(n)); FS_HIP(c, d_tr.ensure(n)); FS_HIP(c, d_un.ensure(n)); FS_HIP(c, d_all.ensure(n));
    FS_HIP(c, hipMemcpyAsync(d_s.p, start_xyz, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    FS_HIP(c, hipMemcpyAsync(d_e.p, end_xyz, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    FsSegArgs a{};
    a.grid = grid_dev(c);
    a.n = n; a.start = d_s.p; a.end = d_e.p; a.max_length = max_length_cells;
    a.obst_min = obst_min; a.obst_max = obst_max; a.trace_min = trace_min; a.trace_max = trace_max;
    a.ok = d_ok.p; a.hit = d_hit.p; a.traced = d_tr.p; a.unknown = d_un.p; a.all = d_all.p;
    FS_HIP(c, fs_launch_segments(a, c->stream));
    FS_HIP(c, hipMemcpyAsync(ok, d_ok.p, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipMemcpyAsync(hit, d_hit.p, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipMemcpyAsync(traced, d_tr.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipMemcpyAsync(unknown, d_un.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipMemcpyAsync(all, d_all.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipStreamSynchronize(c->stream));
    return FS_OK;
}

// ------------------------------------------------------------------ Fisher information

}  // extern "C"

// Host half of fs_upload_landmarks: the cloud in k-d leaf order as SoA + one bounding sphere per chunk.  A function of the
// input alone — fs_multi runs it once and hands the result to every device.
void fs_stage_landmarks(const float *xyz, int32_t m, FsStagedCloud &out)
{
    // Chunks of 64 consecutive landmarks are the unit of visibility culling, so the cloud is put into the leaf order
    // of a k-d tree with exactly 64 landmarks per leaf: split the longest axis of the bounding box at the multiple of
    // 64 nearest the median, left part first; a remainder always goes right and ends up as the last, short chunk.
    // Against chunks cut from the Morton order (which straddle the curve's jumps) the bounding spheres shrink from
    // 1.78 m to 1.27 m on the C3 cloud and 20 % fewer landmarks survive the culling.  Non-finite points go last.
    std::vector<int32_t> order((size_t)m);
    int32_t n_finite = 0;
    {
        int32_t tail = m;
        for (int32_t i = 0; i < m; ++i) {
            const float *p = xyz + 3 * (size_t)i;
            // (usable: finite and within 1e17 m of the origin — see below; fabsf of a NaN compares false)
            if (std::fabs(p[0]) <= 1.0e17f && std::fabs(p[1]) <= 1.0e17f && std::fabs(p[2]) <= 1.0e17f) order[n_finite++] = i;
            else order[--tail] = i;
        }
        std::reverse(order.begin() + n_finite, order.end());      // keep the non-finite ones in input order
    }
    {
        // [lo, hi) ranges of `order`: split, then the left part, then the right one.  A range is worked on without looking at any
        // other, so the two halves of the top levels go to threads of their own (up to eight leaves of the recursion at once: this
        // ordering is what a new cloud costs per SLAM map update — fs_upload_landmarks 13.2 -> 4.3 ms at C3, 79.9 -> 20.6 ms at C5's
        // 500 k landmarks, tools/landmark_staging_probe.py — and the result is the same
        // permutation whoever computes it).
        const unsigned hw = std::thread::hardware_concurrency();
        int par_depth = hw >= 8 ? 3 : hw >= 4 ? 2 : hw >= 2 ? 1 : 0;
        if (const char *e = std::getenv("FS_KD_THREADS")) {       // measurement aid: 1 = everything on the calling thread
            const int t = std::atoi(e);
            par_depth = t >= 8 ? 3 : t >= 4 ? 2 : t >= 2 ? 1 : 0;
        }
        std::function<void(int32_t, int32_t, int)> build = [&](int32_t lo_i, int32_t hi_i, int depth) {
            for (;;) {
                const int32_t n = hi_i - lo_i;
                if (n <= FS_CHUNK) return;
                float blo[3] = {INFINITY, INFINITY, INFINITY}, bhi[3] = {-INFINITY, -INFINITY, -INFINITY};
                for (int32_t i = lo_i; i < hi_i; ++i) {
                    const float *p = xyz + 3 * (size_t)order[i];
                    for (int a = 0; a < 3; ++a) { blo[a] = std::min(blo[a], p[a]); bhi[a] = std::max(bhi[a], p[a]); }
                }
                int ax = 0;
                if (bhi[1] - blo[1] > bhi[ax] - blo[ax]) ax = 1;
                if (bhi[2] - blo[2] > bhi[ax] - blo[ax]) ax = 2;
                int32_t k = (n / 2) / FS_CHUNK * FS_CHUNK;
                if (k == 0) k = FS_CHUNK;
                std::nth_element(order.begin() + lo_i, order.begin() + lo_i + k, order.begin() + hi_i, [&](int32_t u, int32_t v) {
                    const float pu = xyz[3 * (size_t)u + ax], pv = xyz[3 * (size_t)v + ax];
                    return pu < pv || (pu == pv && u < v);        // ties by index: the order is a function of the input
                });
                if (depth < par_depth && n >= 16384) {
                    std::thread left;
                    try {
                        left = std::thread(build, lo_i, lo_i + k, depth + 1);
                    } catch (...) {                               // no thread to be had: the left part runs here
                        build(lo_i, lo_i + k, depth + 1);
                    }
                    build(lo_i + k, hi_i, depth + 1);
                    if (left.joinable()) left.join();
                    return;
                }
                build(lo_i, lo_i + k, depth + 1);
                lo_i += k;                                        // (the right part: this loop's next turn)
                ++depth;
            }
        };
        build(0, n_finite, 0);
    }
    const int32_t n_chunks = std::max<int32_t>(1, (m + FS_CHUNK - 1) / FS_CHUNK);
    const size_t mp = (size_t)n_chunks * FS_CHUNK;
    // SoA + far-away sentinels in the padding: (1e18)^2 is finite in fp32 and beyond any max_dist^2
    std::vector<float> &x = out.x, &y = out.y, &z = out.z, &sph = out.sph;
    x.assign(mp, 1.0e18f); y.assign(mp, 1.0e18f); z.assign(mp, 1.0e18f); sph.assign((size_t)n_chunks * 4, 0.0f);
    // A point with a NaN or an infinite coordinate lies outside every visibility volume (n^2 <= max_dist^2 is false for it), and the
    // kernels must never see it: their cone predicate is ONE v_min3_f32, which DROPS a NaN operand — a landmark at x = +inf seen from
    // a pose whose rotation has exact zeros (px = +inf, py = 0 * inf = NaN, n^2 = NaN) would pass as visible (found in round 5 by
    // tests/test_gpu_hardening.py::test_non_finite_and_far_away_landmarks_are_never_visible).  Such points keep their slots (the
    // cloud's size and order are the caller's) but are staged as the far-away sentinel of the padding.  The same for a FINITE
    // coordinate beyond 1e17 m: rotated into a camera frame it can overflow fp32 to +-inf, and an invisible landmark's terms are
    // removed by a factor q = 0, which inf * 0 = NaN defeats (NaN in the 6x6 sums of every pose with a general rotation).  Nothing
    // that far out is within any range fs_set_fim_params accepts (max_dist < 1e9 m).
    out.perm.assign(mp, -1);                                      // (sentinels: the padding and the unusable points' slots)
    for (int32_t i = 0; i < n_finite; ++i) {
        const float *p = xyz + 3 * (size_t)order[i];
        x[i] = p[0]; y[i] = p[1]; z[i] = p[2];
        out.perm[i] = order[i];
    }
    for (int32_t ch = 0; ch < n_chunks; ++ch) {
        double blo[3] = {1e300, 1e300, 1e300}, bhi[3] = {-1e300, -1e300, -1e300};
        int cnt = 0;
        for (int k = 0; k < FS_CHUNK; ++k) {
            const size_t i = (size_t)ch * FS_CHUNK + k;
            if (i >= (size_t)n_finite) continue;                  // (padding and the non-finite points: sentinels, in no sphere)
            const double p[3] = {x[i], y[i], z[i]};
            for (int a = 0; a < 3; ++a) { blo[a] = std::min(blo[a], p[a]); bhi[a] = std::max(bhi[a], p[a]); }
            ++cnt;
        }
        float *s4 = &sph[4 * (size_t)ch];
        if (cnt == 0) { s4[0] = s4[1] = s4[2] = 0.0f; s4[3] = -1.0e30f; continue; }   // never accepted, holds nothing visible
        const float ctr[3] = {(float)(0.5 * (blo[0] + bhi[0])), (float)(0.5 * (blo[1] + bhi[1])), (float)(0.5 * (blo[2] + bhi[2]))};
        double r2 = 0.0;
        for (int k = 0; k < FS_CHUNK; ++k) {
            const size_t i = (size_t)ch * FS_CHUNK + k;
            if (i >= (size_t)n_finite) continue;                  // (padding and the non-finite points: sentinels, in no sphere)
            const double dx = (double)x[i] - ctr[0], dy = (double)y[i] - ctr[1], dz = (double)z[i] - ctr[2];
            r2 = std::max(r2, dx * dx + dy * dy + dz * dz);
        }
        s4[0] = ctr[0]; s4[1] = ctr[1]; s4[2] = ctr[2];
        s4[3] = (float)(std::sqrt(r2) * 1.01 + 2.0e-3);          // safety margin: culling must never drop a visible landmark
    }
    out.m = m; out.n_chunks = n_chunks;
}

static int staged_cloud_done(fs_ctx *c, int32_t m, int32_t n_chunks);

// Device half: four copies and the HBM-tier tables.
int fs_upload_staged_landmarks(fs_ctx *c, const FsStagedCloud &st)
{
    if (!c) return FS_E_INVALID;
    FS_HIP(c, hipSetDevice(c->device));
    const int32_t m = st.m, n_chunks = st.n_chunks;
    const size_t mp = (size_t)n_chunks * FS_CHUNK;
    const std::vector<float> &x = st.x, &y = st.y, &z = st.z, &sph = st.sph;
    if (st.perm.size() != mp) return fail(c, FS_E_INVALID, "staged cloud without its permutation");
    FS_HIP(c, c->d_lx.ensure(mp)); FS_HIP(c, c->d_ly.ensure(mp)); FS_HIP(c, c->d_lz.ensure(mp));
    FS_HIP(c, c->d_spheres.ensure(sph.size()));
    FS_HIP(c, hipMemcpyAsync(c->d_lx.p, x.data(), sizeof(float) * mp, hipMemcpyHostToDevice, c->stream));
    FS_HIP(c, hipMemcpyAsync(c->d_ly.p, y.data(), sizeof(float) * mp, hipMemcpyHostToDevice, c->stream));
    FS_HIP(c, hipMemcpyAsync(c->d_lz.p, z.data(), sizeof(float) * mp, hipMemcpyHostToDevice, c->stream));
    FS_HIP(c, hipMemcpyAsync(c->d_spheres.p, sph.data(), sizeof(float) * sph.size(), hipMemcpyHostToDevice, c->stream));
    FS_HIP(c, c->d_view_perm.ensure(mp)); FS_HIP(c, c->d_view_inv.ensure((size_t)std::max(m, 1)));
    FS_HIP(c, hipMemcpyAsync(c->d_view_perm.p, st.perm.data(), sizeof(int32_t) * mp, hipMemcpyHostToDevice, c->stream));
    FS_HIP(c, fs_view_keep_perm(nullptr, 0, (int32_t)mp, m, c->d_view_perm.p, c->d_view_inv.p, c->stream));
    FS_HIP(c, hipStreamSynchronize(c->stream));
    return staged_cloud_done(c, m, n_chunks);
}

#define FS_CLOUD_DEVICE_FROM 4096
#define FS_VIEW_MASK_BYTES ((size_t)64 << 20)   // fs_landmarks_in_view: the mask words of one round of poses (12.5 KB per pose at 100 k landmarks)
#define FS_VIEW_MAX_ROUND 65536                 // ... and the poses of a round at most, whatever the cloud's size
bool fs_ctx_cloud_on_device(const fs_ctx *c, int32_t m) { return c && (c->opt_cloud_order == 2 || (c->opt_cloud_order == 1 && m >= FS_CLOUD_DEVICE_FROM)); }

// every route that stages a cloud ends here: sizes, the learnt voxel ratio, the HBM tier's hash tables (one per pool workgroup, 2x the
// landmark count).  The cloud is then NOT the landmark sensor's discovered set unless fs_sense_landmarks says so afterwards.
static int staged_cloud_done(fs_ctx *c, int32_t m, int32_t n_chunks)
{
    c->m = m; c->n_chunks = n_chunks;
    reset_voxel_ratio(c);
    int gb = 12;
    while ((1ll << gb) < 2ll * std::max(m, 1)) ++gb;
    c->ghash_bits = gb;
    FS_HIP(c, c->d_gtable.ensure((size_t)fs_ctx::kPool << gb));
    c->have_lm = true;
    c->wl_staged = false;
    ++c->epoch;
    return FS_OK;
}

// where an ordered cloud goes: the staged cloud's arrays (fs_upload_landmarks, fs_sense_landmarks) or the world cloud's
struct CloudDest {
    DevBuf<float> &lx, &ly, &lz, &spheres;
    DevBuf<int32_t> &perm, &inv;
};

// The device ordering (fs_cloud.hip) of a cloud whose raw xyz [m][3] is on the device — or on its way there on the context's stream:
// `start` is called with the first permutation buffer once the scratch is allocated and enqueues whatever fills d_raw and the
// n_usable usable landmarks' positions in ascending order.  The level layout is a function of n_usable alone, so that number is all
// the host has to know.  Ends with the stream drained: what `start` reads on the host may go afterwards.
static int order_cloud_on_device(fs_ctx *c, const float *d_raw, int32_t m, int32_t n_usable, const std::function<int(int32_t *)> &start,
                                 const CloudDest &d, int32_t &n_chunks_out)
{
    const int32_t n_chunks = std::max<int32_t>(1, (m + FS_CHUNK - 1) / FS_CHUNK);
    const size_t mp = (size_t)n_chunks * FS_CHUNK;
    std::vector<int32_t> bounds, level_off, level_nodes, level_largest;
    fs_cloud_levels(n_usable, bounds, level_off, level_nodes, level_largest);
    const size_t temp_bytes = fs_cloud_sort_temp_bytes(n_usable, c->stream);
    FS_HIP(c, d.lx.ensure(mp)); FS_HIP(c, d.ly.ensure(mp)); FS_HIP(c, d.lz.ensure(mp));
    FS_HIP(c, d.spheres.ensure((size_t)n_chunks * 4));
    FS_HIP(c, c->d_cloud_perm.ensure(2 * (size_t)std::max(n_usable, 1)));
    FS_HIP(c, c->d_cloud_keys.ensure(2 * (size_t)std::max(n_usable, 1)));
    FS_HIP(c, c->d_cloud_bounds.ensure(std::max<size_t>(bounds.size(), 1)));
    FS_HIP(c, c->d_cloud_temp.ensure(std::max<size_t>(temp_bytes, 256)));
    FS_HIP(c, c->d_cloud_bbox.ensure(fs_cloud_top_bbox_words()));
    int32_t *perm_a = c->d_cloud_perm.p, *perm_b = perm_a + std::max(n_usable, 1);
    if (const int rc = start(perm_a)) return rc;
    if (!bounds.empty()) FS_HIP(c, hipMemcpyAsync(c->d_cloud_bounds.p, bounds.data(), sizeof(int32_t) * bounds.size(), hipMemcpyHostToDevice, c->stream));
    int32_t *perm = perm_a;
    FS_HIP(c, fs_cloud_order_device(d_raw, n_usable, c->d_cloud_bounds.p, level_off, level_nodes, level_largest, perm_a, perm_b, c->d_cloud_keys.p,
                                    c->d_cloud_keys.p + std::max(n_usable, 1), c->d_cloud_temp.p, temp_bytes, c->d_cloud_bbox.p, c->stream, &perm));
    FS_HIP(c, fs_cloud_finish(d_raw, perm, n_usable, n_chunks, d.lx.p, d.ly.p, d.lz.p, d.spheres.p, c->stream));
    // the order is kept (the scratch above may be released): fs_landmarks_in_view names landmarks by their place in the array
    FS_HIP(c, d.perm.ensure(mp)); FS_HIP(c, d.inv.ensure((size_t)std::max(m, 1)));
    FS_HIP(c, fs_view_keep_perm(perm, n_usable, (int32_t)mp, m, d.perm.p, d.inv.p, c->stream));
    FS_HIP(c, hipStreamSynchronize(c->stream));                  // (the caller's cloud and the vectors above are read until here)
    if (c->d_cloud_raw.cap > ((size_t)16 << 20)) { c->d_cloud_raw.release(); c->d_cloud_perm.release(); c->d_cloud_keys.release(); c->d_cloud_temp.release(); }
    n_chunks_out = n_chunks;
    return FS_OK;
}

// the usable landmarks of a host cloud (as fs_stage_landmarks: finite and within 1e17 m; fabsf of a NaN compares false): how many,
// and — only when some are not (rare) — which, in input order
static int32_t usable_landmarks(const float *xyz, int32_t m, std::vector<int32_t> &usable)
{
    auto ok = [&](int32_t i) {
        const float *p = xyz + 3 * (size_t)i;
        return std::fabs(p[0]) <= 1.0e17f && std::fabs(p[1]) <= 1.0e17f && std::fabs(p[2]) <= 1.0e17f;
    };
    int32_t n_usable = 0;
    for (int32_t i = 0; i < m; ++i) n_usable += ok(i) ? 1 : 0;
    usable.clear();
    if (n_usable != m) {
        usable.reserve((size_t)n_usable);
        for (int32_t i = 0; i < m; ++i) if (ok(i)) usable.push_back(i);
    }
    return n_usable;
}

// a host cloud goes up as it is into d_raw and is put into k-d leaf order there: the host only finds out how many landmarks are
// usable and which, if any, are not
static int order_host_cloud_on_device(fs_ctx *c, const float *xyz, int32_t m, float *d_raw, const CloudDest &d, int32_t &n_chunks)
{
    std::vector<int32_t> usable;
    const int32_t n_usable = usable_landmarks(xyz, m, usable);
    return order_cloud_on_device(c, d_raw, m, n_usable, [&](int32_t *perm_a) -> int {
        if (m > 0) FS_HIP(c, hipMemcpyAsync(d_raw, xyz, sizeof(float) * 3 * (size_t)m, hipMemcpyHostToDevice, c->stream));
        if (n_usable == m) FS_HIP(c, fs_cloud_iota(perm_a, n_usable, c->stream));
        else if (n_usable > 0) FS_HIP(c, hipMemcpyAsync(perm_a, usable.data(), sizeof(int32_t) * (size_t)n_usable, hipMemcpyHostToDevice, c->stream));
        return FS_OK;
    }, d, n_chunks);
}

// "cloud.order" 1 / 2: fs_upload_landmarks on the device route
static int upload_landmarks_device_order(fs_ctx *c, const float *xyz, int32_t m)
{
    FS_HIP(c, hipSetDevice(c->device));
    c->have_lm = false;                                          // (until the new cloud is whole: an error on the way leaves no cloud, not half of one)
    FS_HIP(c, c->d_cloud_raw.ensure(3 * (size_t)std::max(m, 1)));
    int32_t n_chunks = 0;
    const CloudDest staged{c->d_lx, c->d_ly, c->d_lz, c->d_spheres, c->d_view_perm, c->d_view_inv};
    if (const int rc = order_host_cloud_on_device(c, xyz, m, c->d_cloud_raw.p, staged, n_chunks)) return rc;
    return staged_cloud_done(c, m, n_chunks);
}

extern "C" {

int fs_upload_landmarks(fs_ctx *c, const float *xyz, int32_t m)
{
    if (!c || (m > 0 && !xyz) || m < 0) return FS_E_INVALID;
    // chunk masks live in LDS (one bit per chunk) next to the 64-KiB tier-1 table
    if (m > 2000000) return fail(c, FS_E_INVALID, "at most 2,000,000 landmarks per context");
    if (fs_ctx_cloud_on_device(c, m)) return upload_landmarks_device_order(c, xyz, m);
    FsStagedCloud st;
    fs_stage_landmarks(xyz, m, st);
    return fs_upload_staged_landmarks(c, st);
}

int fs_set_option(fs_ctx *c, const char *key, double value)
{
    if (!c || !key) return FS_E_INVALID;
    ++c->epoch;                                            // (whatever the knob is, captured launch sequences are taken again)
    if (std::strcmp(key, "graph") == 0) { c->opt_graph = value != 0.0; return FS_OK; }
    if (std::strcmp(key, "zerocopy") == 0) { c->opt_zero_copy = value != 0.0; return FS_OK; }
    if (std::strcmp(key, "fim.cull") == 0) { c->opt_cull = value != 0.0; return FS_OK; }
    if (std::strcmp(key, "fim.specialise") == 0) { c->opt_special = value != 0.0; return FS_OK; }
    if (std::strcmp(key, "fim.learn") == 0) { c->opt_learn = value != 0.0; return FS_OK; }
    if (std::strcmp(key, "cloud.order") == 0 && value >= 0 && value <= 2) { c->opt_cloud_order = (int)value; return FS_OK; }
    if (std::strcmp(key, "ray.sort") == 0) { c->opt_sort = value != 0.0; return FS_OK; }
    if (std::strcmp(key, "sort.costmap") == 0) { c->opt_costmap = value != 0.0; return FS_OK; }
    if (std::strcmp(key, "sort.reverse") == 0) { c->opt_sort_reverse = value != 0.0; return FS_OK; }
    if (std::strcmp(key, "fim.hostfinish") == 0) { c->opt_host_finish = value != 0; ++c->epoch; return FS_OK; }
    if (std::strcmp(key, "fim.split") == 0 && value >= 0 && value <= 5) { c->opt_split = (int)value; ++c->epoch; return FS_OK; }
    if (std::strcmp(key, "ray.layout") == 0 && value >= 0 && value <= 3) { c->opt_layout = (int)value; return FS_OK; }
    if (std::strcmp(key, "fim.bits1") == 0 && value >= 10 && value <= 14) { c->opt_bits1 = (int)value; return FS_OK; }
    if (std::strcmp(key, "fim.skip32") == 0 && value >= 1 && value <= 32) { c->opt_skip32 = (int)value; return FS_OK; }
    if (std::strcmp(key, "fim.headroom") == 0 && value >= 8 && value <= 64) { c->opt_headroom = (int)value; return FS_OK; }
    if (std::strcmp(key, "roadmap.tour_one_wg") == 0 && value >= 0 && value <= RM_TREE_ONE_WG) { c->tour_one_wg = (int32_t)value; return FS_OK; }
    if (std::strcmp(key, "roadmap.astar_lds_entries") == 0 && value >= 0 && value <= 2048) { c->astar_lds_entries = (int32_t)value; return FS_OK; }
    if (std::strcmp(key, "roadmap.dedup_one_wg") == 0 && value >= 0 && value <= FS_KF_DEDUP_ONE_WG) { c->kf_one_wg = (int32_t)value; return FS_OK; }
    if (std::strcmp(key, "navfn.wave_slots") == 0 && value >= 0 && value <= 65535) { c->nw_opt_slots = (int32_t)value; return FS_OK; }
    if (std::strcmp(key, "navfn.wave_bytes") == 0 && value >= 1 && value <= 1099511627776.0) { c->nw_opt_bytes = (int64_t)value; return FS_OK; }
    if (std::strcmp(key, "navfn.wave_cap") == 0 && value >= 16 && value <= 10000) { c->nw_opt_cap = (int32_t)value; return FS_OK; }
    if (std::strcmp(key, "refine.search_slots") == 0 && value >= 0 && value <= 65535) { c->rs_opt_slots = (int32_t)value; return FS_OK; }
    if (std::strcmp(key, "refine.search_bytes") == 0 && value >= 1 && value <= 1099511627776.0) { c->rs_opt_bytes = (int64_t)value; return FS_OK; }
    if (std::strcmp(key, "view.round_poses") == 0 && value >= 0 && value <= FS_VIEW_MAX_ROUND) { c->opt_view_round = (int32_t)value; return FS_OK; }
    if (std::strcmp(key, "pathinfo.dedup") == 0) { c->opt_pi_dedup = value != 0.0; return FS_OK; }
    if (std::strcmp(key, "infolayer.batch") == 0 && value >= 1 && value <= (double)(1 << 24)) { c->opt_il_batch = (int64_t)value; return FS_OK; }
    if (std::strcmp(key, "routes.dedup") == 0) { c->opt_rt_dedup = value != 0.0; return FS_OK; }
    if (std::strcmp(key, "routes.pool_nodes") == 0 && value >= 1 && value <= (double)(1 << 30)) { c->rt_pool_cap = (int64_t)value; return FS_OK; }
    if (std::strcmp(key, "refine.max_fields") == 0 && value >= 1 && value <= RF_MAX_FIELDS) {
        if ((int32_t)value != c->rf_max_fields) { c->rf_max_fields = (int32_t)value; c->rf_key.clear(); c->rf_gen.clear(); }
        return FS_OK;
    }
    return fail(c, FS_E_INVALID, "unknown option %s", key);
}

int fs_get_counter(fs_ctx *c, int which, int64_t *value, int reset)
{
    // host-side figures: the field behind each id and whether `reset` clears it
    static const struct {
        int id;
        int64_t fs_ctx::*v;
        bool reset;
    } host[] = {
        // the sparse class image ("ray.layout" 3): bricks of the grid, bricks its pool holds
        {1000, &fs_ctx::sparse_bricks, false}, {1001, &fs_ctx::sparse_pool_bricks, false},
        // the grid planner (fs_plan_paths): potential fields built, rounds of the last one, round launches in all
        {1002, &fs_ctx::nav_builds, true}, {1003, &fs_ctx::nav_rounds, false}, {1004, &fs_ctx::nav_launches, true},
        // the roadmap planner (fs_roadmap_plan): shortest-path trees built, rounds of the last one; segments the roadmap calls have
        // walked (fs_roadmap_rebuild, fs_roadmap_connect)
        {1005, &fs_ctx::rm_tree_builds, true}, {1006, &fs_ctx::rm_tree_rounds, false}, {1007, &fs_ctx::rm_traced, true},
        // the next-goal search (fs_roadmap_next_goal): trees built, rounds of the last call's batch (its slowest tree), tours evaluated
        {1008, &fs_ctx::tour_tree_builds, true}, {1009, &fs_ctx::tour_tree_rounds, false}, {1010, &fs_ctx::tour_evaluated, true},
        // the leg refinement (fs_refine_paths / fs_refine_field): fields built, rounds of the last field built, line-of-sight walks
        {1011, &fs_ctx::rf_builds, true}, {1012, &fs_ctx::rf_rounds, false}, {1013, &fs_ctx::rf_walks, true},
        // the frontier search (fs_search_frontiers): breadth-first levels of the last search's deepest component, its pieces whose
        // median sort the guard stopped
        {1014, &fs_ctx::fs_levels, false}, {1015, &fs_ctx::fs_guarded, false},
        // the key-frame anchors (fs_roadmap_set_keyframes / fs_roadmap_optimize): anchor records stored (the store is
        // keyframe_mapping_), de-duplication rounds of the last optimise, points it de-duplicated
        {1016, &fs_ctx::kf_records, false}, {1017, &fs_ctx::kf_rounds, false}, {1018, &fs_ctx::kf_points, false},
        // the outer search of the last Reference-seeded frontier search: levels walked, cells popped
        {1019, &fs_ctx::fs_outer_levels, false}, {1020, &fs_ctx::fs_outer_popped, false},
        // the REFERENCE roadmap search: A* queries run, pops of the last call's largest query, queries that took the global route
        {1021, &fs_ctx::as_queries, true}, {1022, &fs_ctx::as_max_pops, false}, {1023, &fs_ctx::as_global, true},
        // the path information (fs_plan_paths_information): way points of the last call, distinct poses it scored
        {1024, &fs_ctx::pi_waypoints, false}, {1025, &fs_ctx::pi_distinct, false},
        // the roadmap routes (fs_roadmap_routes): distinct routes of the last call, isConnectable walks of its refinement, distinct
        // leg poses it scored; calls that ran the A* again on a grown chain pool
        {1026, &fs_ctx::rt_routes, false}, {1027, &fs_ctx::rt_walks, false}, {1028, &fs_ctx::rt_poses, false}, {1029, &fs_ctx::rt_retries, true},
        // the per-tick update (fs_roadmap_update): walks, owners (distinct closest nodes) and keep-rule rounds of the last call
        {1033, &fs_ctx::ru_walks, false}, {1034, &fs_ctx::ru_owners, false}, {1035, &fs_ctx::ru_rounds, false},
        // the REFERENCE grid search: slot batches of the last call
        {1038, &fs_ctx::nw_batches, false},
        // the REFERENCE refine search, of the last call under it: searches, slot batches, nodes popped, line-of-sight walks, largest heap
        {1042, &fs_ctx::rs_searches, false}, {1043, &fs_ctx::rs_batches, false}, {1044, &fs_ctx::rs_pops, false},
        {1045, &fs_ctx::rs_walks, false}, {1046, &fs_ctx::rs_max_heap, false},
        // the gated drive (fs_drive_slam): host waits of the last call, occupied voxels per pose its LDS tier takes at most, workgroups
        // that took the fallback tier
        {1047, &fs_ctx::ds_waits, false}, {1048, &fs_ctx::ds_capacity, false}, {1049, &fs_ctx::ds_fallbacks, true},
    };
    // ... its waves, the waves that ended on the cycle budget, the waves that dropped a push at the cap and the chunks run again, of
    // the last call: they stay on the device until asked for
    if (c && value && (which == 1037 || (which >= 1039 && which <= 1041))) {
        FS_HIP(c, hipSetDevice(c->device));
        *value = 0;
        if (!c->d_nw_idx.p) return FS_OK;
        int32_t v = 0;
        FS_HIP(c, hipMemcpyAsync(&v, c->d_nw_idx.p + (which == 1037 ? 0 : which - 1038), sizeof v, hipMemcpyDeviceToHost, c->stream));
        FS_HIP(c, hipStreamSynchronize(c->stream));
        *value = v;
        return FS_OK;
    }
    // the task allocator (fs_allocate_tasks, fs_allocate_tasks_dev, fs_fleet_allocate_roadmap): augmentations, step-5 runs and
    // step-3 primes of the last solve.  The solve leaves them on the device (the device form is not waited for): read here
    if (c && value && which >= 1030 && which <= 1032) {
        FS_HIP(c, hipSetDevice(c->device));
        *value = 0;
        if (!c->d_al_stats.p) return FS_OK;
        int32_t v = 0;
        FS_HIP(c, hipMemcpyAsync(&v, c->d_al_stats.p + 1 + (which - 1030), sizeof v, hipMemcpyDeviceToHost, c->stream));
        FS_HIP(c, hipStreamSynchronize(c->stream));
        *value = v;
        return FS_OK;
    }
    // bytes the DevBuf / PinnedBuf objects hold (buf_bytes_held): of the whole process, not of this context alone
    if (c && value && which == 1036) { *value = buf_bytes_held.load(); return FS_OK; }
    for (const auto &h : host)
        if (c && value && which == h.id) {
            *value = c->*h.v;
            if (reset && h.reset) c->*h.v = 0;
            return FS_OK;
        }
    if (!c || !value || which < 0 || which >= FS_N_COUNTERS) return FS_E_INVALID;
    FS_HIP(c, hipSetDevice(c->device));
    *value = 0;
    if (!c->d_counters.p) return FS_OK;
    unsigned long long v = 0;
    FS_HIP(c, hipMemcpyAsync(&v, c->d_counters.p + which, sizeof v, hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipStreamSynchronize(c->stream));
    *value = (int64_t)v;
    if (reset) {
        FS_HIP(c, hipMemsetAsync(c->d_counters.p + which, 0, sizeof v, c->stream));
        FS_HIP(c, hipStreamSynchronize(c->stream));
    }
    return FS_OK;
}

int fs_lookup_generate(fs_ctx *c, const float bounds[6])
{
    if (!c) return FS_E_INVALID;
    FS_HIP(c, hipSetDevice(c->device));
    // DEP/src/fisher_information/GenerateLookupMain.cpp:9 — double literals narrowed to the float parameters
    const float def[6] = {(float)0.0, (float)21.0, (float)(-8.5 * 1.732), (float)(8.5 * 1.732), (float)(-8.5 * 1.732), (float)(8.5 * 1.732)};
    const float *b = bounds ? bounds : def;
    generate_records(b[0], b[1], b[2], b[3], b[4], b[5], c->records);
    return build_dense(c);
}

int fs_lookup_set_records(fs_ctx *c, const float *records, int64_t n)
{
    if (!c || !records || n <= 0) return FS_E_INVALID;
    FS_HIP(c, hipSetDevice(c->device));
    c->records.assign(records, records + 4 * n);
    return build_dense(c);
}

int fs_lookup_load(fs_ctx *c, const char *path)
{
    if (!c || !path) return FS_E_INVALID;
    FS_HIP(c, hipSetDevice(c->device));
    FILE *f = std::fopen(path, "rb");
    if (!f) return fail(c, FS_E_IO, "Cannot load lookup table. Does it exist in the path? (%s)", path);
    std::vector<float> rec;
    float r[4];
    while (std::fread(r, sizeof(float), 4, f) == 4) rec.insert(rec.end(), r, r + 4);   // FisherInfoManager.cpp:247-248
    std::fclose(f);
    if (rec.empty()) return fail(c, FS_E_IO, "lookup table file %s holds no complete record", path);
    c->records.swap(rec);
    return build_dense(c);
}

int fs_lookup_save(fs_ctx *c, const char *path)
{
    if (!c || !path) return FS_E_INVALID;
    if (!c->have_table) return fail(c, FS_E_STATE, "no lookup table to save");
    FILE *f = std::fopen(path, "wb");
    if (!f) return fail(c, FS_E_IO, "Error opening file for writing (%s)", path);
    const size_t n = c->records.size();
    const size_t w = std::fwrite(c->records.data(), sizeof(float), n, f);
    std::fclose(f);
    return w == n ? FS_OK : fail(c, FS_E_IO, "short write to %s", path);
}

int fs_lookup_num_records(const fs_ctx *c, int64_t *n)
{
    if (!c || !n) return FS_E_INVALID;
    *n = (int64_t)c->records.size() / 4;
    return FS_OK;
}

int fs_lookup_get_records(const fs_ctx *c, float *records)
{
    if (!c || !records) return FS_E_INVALID;
    std::memcpy(records, c->records.data(), c->records.size() * sizeof(float));
    return FS_OK;
}

int fs_lookup_query(const fs_ctx *c, const float p[3], float *value)
{
    if (!c || !p || !value) return FS_E_INVALID;
    if (!c->have_table) return FS_E_STATE;
    float key[3];
    long j[3];
    voxel_coordinate(p[0], p[1], p[2], key, j);
    const long jx = j[0] - c->jx0, jy = j[1] - c->jy0, jz = j[2] - c->jz0;
    if (jx < 0 || jx >= c->tx || jy < 0 || jy >= c->ty || jz < 0 || jz >= c->tz) *value = std::numeric_limits<float>::quiet_NaN();
    else *value = c->dense[((size_t)jx * c->ty + jy) * c->tz + jz];
    return FS_OK;
}

int fs_set_fim_params(fs_ctx *c, const fs_fim_params *p)
{
    if (!c || !p) return FS_E_INVALID;
    if (!(p->max_dist > 0.0) || !(p->max_angle > 0.0)) return fail(c, FS_E_INVALID, "max_dist and max_angle must be positive");
    // (the padding of the landmark arrays and every unusable landmark sit at 1e18 m: max_dist^2 must stay far below (1e18)^2 in fp32)
    if (!(p->max_dist < 1.0e9)) return fail(c, FS_E_INVALID, "max_dist must be below 1e9 m");
    if (p->max_dist != c->fp.max_dist || p->max_angle != c->fp.max_angle) reset_voxel_ratio(c);
    c->fp = *p;
    ++c->epoch;
    return FS_OK;
}

// The scoring route with fs_set_occlusion enabled, in place of run_fim_tier1 + run_fim_rest: no LDS tier, no pose
// splitting (a.split_shift stays 0), no finish on the host — every pose goes through the HBM-tier worker with the line-of-sight
// test in its visibility, then the finish kernel as usual.  The grid is the staged one AT THIS CALL: nothing is kept per landmark.
static int occlusion_args(fs_ctx *c, FsFimArgs &a)
{
    if (!c->have_grid) return fail(c, FS_E_STATE, "occlusion is enabled (fs_set_occlusion) and fs_upload_grid has not been called");
    a.occ_grid = grid_dev(c);
    a.occ_min = c->occ.occ_min; a.occ_max = c->occ.occ_max;
    a.occ_margin = occlusion_margin(c, c->occ.end_margin_m);
    a.split_shift = 0; a.split_flags = nullptr; a.host_flag = nullptr;
    return FS_OK;
}

static int run_fim_occluded(fs_ctx *c, FsFimArgs &a)
{
    a.cand_perm = nullptr; a.cand_lo = 0; a.cand_count = a.n;
    {
        ScopedTimer t(c, 2);
        FS_HIP(c, fs_launch_fim_occluded(a, fs_ctx::kPool, c->stream));
    }
    FS_HIP(c, fs_launch_fim_finish(a, c->stream));
    return FS_OK;
}

int fs_set_occlusion(fs_ctx *c, const fs_occlusion_params *p)
{
    if (!c) return FS_E_INVALID;
    const fs_occlusion_params def{0, 254, 254, 0.3};
    if (!p) p = &def;
    if (p->occ_min < 0 || p->occ_max > 255 || p->occ_min > p->occ_max) return fail(c, FS_E_INVALID, "occ_min / occ_max must be costs 0..255 with occ_min <= occ_max");
    if (!(p->end_margin_m >= 0.0) || !(p->end_margin_m < 1.0e6)) return fail(c, FS_E_INVALID, "end_margin_m must be finite, >= 0 and below 1e6 m");
    c->occ = *p;
    c->occ.enabled = p->enabled ? 1 : 0;
    ++c->epoch;                                            // (captured launch sequences are taken again)
    return FS_OK;
}

int fs_get_occlusion(const fs_ctx *c, fs_occlusion_params *p)
{
    if (!c || !p) return FS_E_INVALID;
    *p = c->occ;
    return FS_OK;
}

int fs_line_of_sight(fs_ctx *c, int32_t n, const double *from_xyz, const double *to_xyz, uint8_t *ok, uint8_t *blocked, int32_t *tested_cells)
{
    if (!c) return FS_E_INVALID;
    if (const int rc = grid_check(c)) return rc;
    if (n < 0 || (n > 0 && (!from_xyz || !to_xyz || !ok || !blocked))) return fail(c, FS_E_INVALID, "null pointer");
    if (n == 0) return FS_OK;
    // (the segment tracer's buffers: the same shapes, never in use at the same time)
    DevBuf<double> &d_s = c->d_seg_start, &d_e = c->d_seg_end;
    DevBuf<uint8_t> &d_ok = c->d_seg_ok, &d_hit = c->d_seg_hit;
    DevBuf<int32_t> &d_all = c->d_seg_all;
    FS_HIP(c, d_s.ensure((size_t)n * 3)); FS_HIP(c, d_e.ensure((size_t)n * 3));
    FS_HIP(c, d_ok.ensure(n)); FS_HIP(c, d_hit.ensure(n)); FS_HIP(c, d_all.ensure(n));
    FS_HIP(c, hipMemcpyAsync(d_s.p, from_xyz, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    FS_HIP(c, hipMemcpyAsync(d_e.p, to_xyz, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    FsFimArgs fa{};
    if (const int rc = occlusion_args(c, fa)) return rc;
    FsLosArgs a{};
    a.grid = fa.occ_grid;
    a.n = n; a.from = d_s.p; a.to = d_e.p;
    a.occ_min = fa.occ_min; a.occ_max = fa.occ_max; a.margin = fa.occ_margin;
    a.ok = d_ok.p; a.blocked = d_hit.p; a.tested = d_all.p;
    FS_HIP(c, fs_launch_los(a, c->stream));
    FS_HIP(c, hipMemcpyAsync(ok, d_ok.p, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipMemcpyAsync(blocked, d_hit.p, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    if (tested_cells) FS_HIP(c, hipMemcpyAsync(tested_cells, d_all.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipStreamSynchronize(c->stream));
    return FS_OK;
}

// A call with few poses leaves most of the chip idle — ONE pose is one of 512 workgroup slots, and the reference's real call is one
// pose per tick (FisherInfoBTPlugin.cpp:24-57): spread each pose over W = 2^shift workgroups by voxel slab (fs_fim.hip, SPLIT), as
// long as all n * W items are resident at once and the cloud is big enough to be worth W workgroups' fixed cost (cull, table
// clear, reduction): at least 128 chunks (8 k landmarks) per workgroup — C1's 2 k landmarks measured 3 us SLOWER split eight ways.
// Same multiset of (voxel value, rank) terms; the partial sums are added in the finish kernel.  Sets a.split_shift / a.split_flags
// and grows the per-item scratch; a.cone_mode / a.table_full / a.info_only must be filled in.
static int maybe_split(fs_ctx *c, FsFimArgs &a, size_t n, bool want_fim21)
{
    a.split_shift = 0; a.split_flags = nullptr;
    if (c->opt_split <= 0 || !fs_fim_can_split(a)) return FS_OK;
    int shift = c->opt_split;
    while (shift > 0 && ((n << shift) > 256 || (c->n_chunks >> shift) < 128)) --shift;
    // (W = 1 — a cloud too small to be worth several workgroups — still goes through the split workers when the call asks for
    // info_ref alone and has few poses: they are what lets fs_score_fim_end do the finish on the host, one launch instead of three)
    if (shift == 0 && !(a.info_only && c->opt_host_finish && n <= 256)) return FS_OK;
    if (c->d_split_flags.cap < n) {
        FS_HIP(c, c->d_split_flags.ensure(n));
        FS_HIP(c, hipMemsetAsync(c->d_split_flags.p, 0, c->d_split_flags.cap * sizeof(uint32_t), c->stream));
    }
    const int rc = ensure_candidate_scratch(c, n << shift, want_fim21);
    if (rc) return rc;
    a.split_shift = shift; a.split_flags = c->d_split_flags.p;
    // The W contiguous slabs of the lattice along the camera's x axis (fs_fim.hip, slab_of): cut so that every slab holds the same
    // share of the visibility volume's cross-section over the stretch where the table and the range overlap (in front of the
    // camera only when there is a cone) — plane j at x = j * step shows a disc of radius^2 = min(max_dist^2 - x^2, (x tan(angle))^2).
    // Uniform landmark density assumed; what lies outside the stretch goes to the open-ended first / last slab.
    {
        const int W = 1 << shift;
        const double step = 1.0 / a.inv_step, R = c->fp.max_dist;
        const int reach = (int)std::ceil(R * a.inv_step) + 1;
        const bool cone = a.cone_mode == 1;
        int lo = std::max(c->jx0, cone ? 0 : -reach), hi = std::min(c->jx0 + c->tx - 1, reach);
        if (hi < lo) hi = lo;
        const double tan2 = cone ? std::pow(std::tan(std::min(c->fp.max_angle, 1.55)), 2) : 0.0;
        std::vector<double> cum((size_t)(hi - lo + 2), 0.0);
        for (int j = lo; j <= hi; ++j) {
            const double x = j * step;
            double r2 = std::max(R * R - x * x, 0.0);
            if (cone) r2 = std::min(r2, x * x * tan2);
            cum[(size_t)(j - lo + 1)] = cum[(size_t)(j - lo)] + r2 + 1e-9;      // (+ eps: strictly increasing, so every slab gets planes while there are any)
        }
        a.split_bound[0] = -(1 << 29);
        a.split_bound[W] = 1 << 29;
        int j = lo;
        for (int w = 1; w < W; ++w) {
            const double want = cum.back() * (double)w / (double)W;
            while (j < hi && cum[(size_t)(j - lo + 1)] < want) ++j;
            a.split_bound[w] = std::max(j, a.split_bound[w - 1] > -(1 << 28) ? a.split_bound[w - 1] : lo);
        }
    }
    return FS_OK;
}

static void bind_fim_outputs(fs_ctx *c, FsFimArgs &a)
{
    a.info_ref = c->d_info.p; a.trace = c->d_trace.p; a.logdet = c->d_logdet.p;
    a.n_visible = c->d_nvis.p; a.n_voxels = c->d_nvox.p; a.overflow = c->d_overflow.p;
    a.sums = c->d_sums.p;
    a.tested = c->d_tested.p;
    a.flagged = c->d_flagged.p;
    if (a.fim21) a.fim21 = c->d_fim21.p;       // (maybe_split may have grown — moved — the column since the caller asked for it)
}

// tier 1 on candidates [lo, lo + count) of the processing order
static int run_fim_tier1(fs_ctx *c, FsFimArgs &a, const int32_t *perm, int32_t lo, int32_t count)
{
    a.cand_perm = perm; a.cand_lo = lo; a.cand_count = count;
    ScopedTimer t(c, 1);
    FS_HIP(c, fs_launch_fim(a, c->stream));
    return FS_OK;
}

static int run_fim_rest(fs_ctx *c, FsFimArgs &a)
{
    {
        // the HBM tier exits at once unless the LDS tier flagged a candidate (device-side work list)
        ScopedTimer t(c, 2);
        FS_HIP(c, fs_launch_fim_overflow(a, fs_ctx::kPool, c->stream));
    }
    // (a launch of its own on purpose: running the finish inside the HBM-tier launch — its last workgroup, found with a sign-off
    // counter — measured 6-8 us SLOWER per small call than the launch it saves: profiles/EXPERIMENTS.md, round 5)
    FS_HIP(c, fs_launch_fim_finish(a, c->stream));
    return FS_OK;
}

// fs_score_fim in two halves (as fs_score_candidates_begin / _end): `begin` stages the poses, launches the kernels and requests
// the columns into the context's page-locked buffer, all asynchronous on the context's stream; `end` waits for that stream and
// copies the columns into the caller's arrays.  fs_multi_score_fim starts every member before it waits for the first.
int fs_score_fim_begin(fs_ctx *c, int32_t n, const double *pose7, float *info_ref, float *fim21,
                       float *trace, float *logdet, int32_t *n_visible, int32_t *n_voxels)
{
    if (!c) return FS_E_INVALID;
    c->fim_pending.clear();
    FS_HIP(c, hipSetDevice(c->device));
    int rc = check_scoring_state(c, false, true);
    if (rc) return rc;
    if (n < 0 || (n > 0 && (!pose7 || !info_ref))) return fail(c, FS_E_INVALID, "null pose or output pointer");
    if (n == 0) return FS_OK;
    // One pose per call is the reference's operating point (FisherInfoBTPlugin.cpp:24-57), so the call's fixed cost matters: the
    // pose records go through the context's page-locked buffer (one true DMA instead of a staged pageable copy) and every
    // requested output column comes back through the other one — asynchronous copies, ONE synchronisation.
    const size_t nn = (size_t)n;
    FS_HIP(c, c->h_in.ensure(nn * 12 * sizeof(float)));
    float *Rt = reinterpret_cast<float *>(c->h_in.p);
    const bool unit = poses_to_rt(pose7, n, Rt);
    FS_HIP(c, c->d_Rt.ensure(nn * 12));
    rc = ensure_candidate_scratch(c, n, fim21 != nullptr);
    if (rc) return rc;
    FsFimArgs a{};
    if (const int rc_args = fill_fim_args(c, a)) return rc_args;
    a.n = n; a.Rt = c->d_Rt.p;
    if (!unit) a.cull = 0;
    a.fim21 = fim21 ? c->d_fim21.p : nullptr;
    // isPoseSafe reads the scalar alone (FIP/src/fisher_information/FisherInfoManager.cpp:83-100): a call that asks for nothing
    // but info_ref (and, at no cost, n_voxels) takes the worker without the 6x6 sums and with the exact table-box cull
    a.info_only = (c->opt_special && !fim21 && !trace && !logdet && !n_visible) ? 1 : 0;
    // (the box cull leaves only chunks that can hold voxels of the table, so a pose shows more distinct voxels per landmark
    // scanned than the 13/32 the general worker caps its pass prediction at — C3, cone off: up to 0.5; an extra pass costs a
    // re-test of the landmarks, an overflow the HBM tier)
    if (a.info_only && a.skip32 < 20) a.skip32 = 20;
    const bool occluded = c->occ.enabled != 0;
    rc = occluded ? occlusion_args(c, a) : maybe_split(c, a, nn, fim21 != nullptr);
    if (rc) return rc;
    struct Col { void *host; const void *dev; size_t bytes; };
    const Col cols[6] = {{info_ref, c->d_info.p, 4 * nn}, {fim21, c->d_fim21.p, 84 * nn}, {trace, c->d_trace.p, 4 * nn},
                         {logdet, c->d_logdet.p, 4 * nn}, {n_visible, c->d_nvis.p, 4 * nn}, {n_voxels, c->d_nvox.p, 4 * nn}};
    size_t total = 0;
    uint64_t col_mask = 0;
    for (int k = 0; k < 6; ++k) if (cols[k].host) { total += (cols[k].bytes + 15) & ~(size_t)15; col_mask |= 1ull << k; }
    FS_HIP(c, c->h_out.ensure(total));
    // up to FS_ZERO_COPY_MAX_N poses the worker reads the pose records from, and the finish kernel writes the requested columns
    // into, the mapped page-locked buffers: the call is three launches and one synchronisation, no transfers
    const bool in_place = c->opt_zero_copy && n <= FS_ZERO_COPY_MAX_N && c->h_in.dev && c->h_out.dev;
    // ONE launch for the isPoseSafe call.  A split info-only call needs the finish kernel only to add W partial sums per pose, and the
    // HBM-tier launch only if an item ran out of table: both are launches of ~4.6 us of GPU timeline each.  Here the items write
    // their partial sums into mapped page-locked memory, fs_score_fim_end adds them on the host (the same double additions in the
    // same order as the finish kernel: same bits) — and only if an item raised the flag next to them does it launch the HBM tier
    // and the finish kernel after all and wait a second time.  (What the finish kernel also does per call — folding the test
    // counts into the running totals, zeroing per-call counters — is deferred to the next call that runs it: statistics only; the
    // work cursor is untouched by a call whose items all fit the grid, which split calls do by construction.)
    const bool host_finish = c->opt_host_finish && a.info_only && a.split_flags && in_place && !c->timing && !c->opt_graph;
    c->fin_active = false;
    if (host_finish) {
        FS_HIP(c, c->h_fin.ensure(16 + sizeof(double) * 18 * (nn << a.split_shift)));
        if (!c->h_fin.dev) return fail(c, FS_E_HIP, "mapped page-locked memory unavailable");
        std::memset(c->h_fin.p, 0, 16);
    }
    auto enqueue = [&]() -> int {
        if (in_place) a.Rt = reinterpret_cast<const float *>(c->h_in.dev);
        else FS_HIP(c, hipMemcpyAsync(c->d_Rt.p, c->h_in.p, nn * 12 * sizeof(float), hipMemcpyHostToDevice, c->stream));
        bind_fim_outputs(c, a);
        if (in_place) {
            void **slot[6] = {reinterpret_cast<void **>(&a.info_ref), reinterpret_cast<void **>(&a.fim21), reinterpret_cast<void **>(&a.trace),
                              reinterpret_cast<void **>(&a.logdet), reinterpret_cast<void **>(&a.n_visible), reinterpret_cast<void **>(&a.n_voxels)};
            size_t o = 0;
            for (int k = 0; k < 6; ++k) {
                if (!cols[k].host) continue;
                *slot[k] = c->h_out.dev + o;
                o += (cols[k].bytes + 15) & ~(size_t)15;
            }
        }
        if (host_finish) {
            a.sums = reinterpret_cast<double *>(c->h_fin.dev + 16);
            a.host_flag = reinterpret_cast<uint32_t *>(c->h_fin.dev);
        }
        int r;
        if (occluded) r = run_fim_occluded(c, a);
        else {
            r = run_fim_tier1(c, a, nullptr, 0, a.n << a.split_shift);      // (split: n * W work items)
            if (r) return r;
            if (host_finish) { c->fin_args = a; c->fin_active = true; return FS_OK; }
            r = run_fim_rest(c, a);
        }
        if (r) return r;
        if (in_place) return FS_OK;
        size_t o = 0;
        for (const Col &col : cols) {
            if (!col.host) continue;
            FS_HIP(c, hipMemcpyAsync(c->h_out.p + o, col.dev, col.bytes, hipMemcpyDeviceToHost, c->stream));
            o += (col.bytes + 15) & ~(size_t)15;
        }
        return FS_OK;
    };
    // ONE pose is isPoseSafe's call: its launch sequence is captured (per number of poses up to 4, requested columns, cull mode)
    if (n <= 4) rc = run_maybe_graphed(c, (2ull << 40) | ((uint64_t)a.split_shift << 32) | ((uint64_t)n << 8) | (col_mask << 1) | (uint64_t)(a.cull ? 1 : 0) | (in_place ? 128u : 0u), enqueue);
    else rc = enqueue();
    if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
    size_t off = 0;
    for (int k = 0; k < 6; ++k) {
        const Col &col = cols[k];
        if (!col.host) continue;
        if (k == 0) c->fin_off_info = off;
        if (k == 5) c->fin_off_nvox = off;
        c->fim_pending.push_back({col.host, off, col.bytes});
        off += (col.bytes + 15) & ~(size_t)15;
    }
    c->fin_want_nvox = n_voxels != nullptr;
    return FS_OK;
}

int fs_score_fim_end(fs_ctx *c)
{
    if (!c) return FS_E_INVALID;
    if (c->fim_pending.empty()) return FS_OK;
    FS_HIP(c, hipSetDevice(c->device));
    const hipError_t e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { c->fim_pending.clear(); c->fin_active = false; return fail(c, FS_E_HIP, "hipStreamSynchronize: %s", hipGetErrorString(e)); }
    if (c->fin_active) {
        c->fin_active = false;
        const FsFimArgs &a = c->fin_args;
        uint32_t flag = 0;
        std::memcpy(&flag, c->h_fin.p, 4);
        if (flag == 0) {
            // the finish kernel's info-only branch (fs_fim.hip), on the host: W partial sums per pose, added in item order
            const double *S = reinterpret_cast<const double *>(c->h_fin.p + 16);
            float *info = reinterpret_cast<float *>(c->h_out.p + c->fin_off_info);
            int32_t *nvox = c->fin_want_nvox ? reinterpret_cast<int32_t *>(c->h_out.p + c->fin_off_nvox) : nullptr;
            const int W = 1 << a.split_shift;
            for (int32_t p = 0; p < a.n; ++p) {
                const double *S0 = S + ((size_t)p << a.split_shift) * 18;
                double s_info = S0[0], s_nvox = S0[17];
                for (int w = 1; w < W; ++w) { s_info += S0[(size_t)w * 18]; s_nvox += S0[(size_t)w * 18 + 17]; }
                info[p] = (float)s_info;
                if (nvox) nvox[p] = (int)(s_nvox + 0.5);
            }
        } else {
            // an item ran out of table: the HBM tier redoes the flagged poses, the finish kernel sorts out which result stands
            const int rc = run_fim_rest(c, c->fin_args);
            const hipError_t e2 = hipStreamSynchronize(c->stream);
            if (rc || e2 != hipSuccess) { c->fim_pending.clear(); return rc ? rc : fail(c, FS_E_HIP, "hipStreamSynchronize: %s", hipGetErrorString(e2)); }
        }
    }
    for (const fs_ctx::PendingCol &col : c->fim_pending) std::memcpy(col.host, c->h_out.p + col.off, col.bytes);
    c->fim_pending.clear();
    return FS_OK;
}

int fs_score_fim(fs_ctx *c, int32_t n, const double *pose7, float *info_ref, float *fim21,
                 float *trace, float *logdet, int32_t *n_visible, int32_t *n_voxels)
{
    const int rc = fs_score_fim_begin(c, n, pose7, info_ref, fim21, trace, logdet, n_visible, n_voxels);
    if (rc) return rc;
    return fs_score_fim_end(c);
}

// The landmarks in view of each pose.  Two passes at most, one synchronisation each.  Pass 1 marks, counts and
// scans round by round (a round's masks are the scratch of the next) and brings `offsets` back — the caller's count-only form
// ends there, and so does a call with nothing to store.  Pass 2 emits: a call of ONE round (every call within FS_VIEW_MASK_BYTES)
// still holds its masks; a call of several marks each round again, only the rounds that have entries below max_total.
int fs_landmarks_in_view(fs_ctx *c, int32_t n, const double *pose7, int64_t max_total, int64_t *offsets, fs_view_landmark *out)
{
    if (!c) return FS_E_INVALID;
    if (n < 0 || max_total < 0 || (n > 0 && (!pose7 || !offsets)) || (max_total > 0 && !out)) return fail(c, FS_E_INVALID, "null pointer or negative size");
    FS_HIP(c, hipSetDevice(c->device));
    int rc = check_scoring_state(c, false, true);
    if (rc) return rc;
    FsFimArgs fa{};
    if (const int rc_args = fill_fim_args(c, fa)) return rc_args;
    const bool occluded = c->occ.enabled != 0;
    if (occluded) { rc = occlusion_args(c, fa); if (rc) return rc; }
    if (n == 0) { if (offsets) offsets[0] = 0; return FS_OK; }
    const size_t nn = (size_t)n;
    std::vector<float> Rt(nn * 12);
    if (!poses_to_rt(pose7, n, Rt.data())) fa.cull = 0;
    const int32_t words = std::max(1, (c->m + 31) / 32);
    int64_t per_round = c->opt_view_round > 0 ? c->opt_view_round
                                              : std::max<int64_t>(1, std::min<int64_t>(FS_VIEW_MAX_ROUND, (int64_t)(FS_VIEW_MASK_BYTES / (sizeof(uint32_t) * (size_t)words))));
    per_round = std::min<int64_t>(per_round, n);
    const int64_t rounds = ((int64_t)n + per_round - 1) / per_round;
    FS_HIP(c, c->d_view_Rt.ensure(nn * 12)); FS_HIP(c, c->d_view_off.ensure(nn + 1));
    FS_HIP(c, c->d_view_mask.ensure((size_t)per_round * (size_t)words)); FS_HIP(c, c->d_view_counts.ensure((size_t)per_round));
    FsViewArgs a{};
    a.lx = c->d_lx.p; a.ly = c->d_ly.p; a.lz = c->d_lz.p; a.spheres = c->d_spheres.p;
    a.n_chunks = c->n_chunks; a.m = c->m;
    a.perm = c->d_view_perm.p; a.inv = c->d_view_inv.p;
    a.Rt = c->d_view_Rt.p;
    a.words = words; a.mask = c->d_view_mask.p; a.counts = c->d_view_counts.p;
    a.group = chunks_per_wave(per_round, c->n_chunks);
    a.cull = fa.cull; a.max_dist_f = fa.max_dist_f;
    a.maxd2 = fa.maxd2; a.cos2 = fa.cos2; a.cone_mode = fa.cone_mode;
    a.table = fa.table; a.jx0 = fa.jx0; a.jy0 = fa.jy0; a.jz0 = fa.jz0; a.tx = fa.tx; a.ty = fa.ty; a.tz = fa.tz; a.inv_step = fa.inv_step;
    a.occluded = occluded ? 1 : 0;
    if (occluded) { a.occ_min = fa.occ_min; a.occ_max = fa.occ_max; a.occ_margin = fa.occ_margin; a.occ_grid = fa.occ_grid; }
    a.offsets = c->d_view_off.p; a.max_total = 0; a.out = nullptr;
    auto mark_round = [&](int64_t r) -> int {
        a.pose_lo = (int32_t)(r * per_round);
        a.n_round = (int32_t)std::min<int64_t>(per_round, (int64_t)n - r * per_round);
        FS_HIP(c, hipMemsetAsync(c->d_view_mask.p, 0, sizeof(uint32_t) * (size_t)a.n_round * (size_t)words, c->stream));
        FS_HIP(c, fs_launch_view_mark(a, c->stream));
        return FS_OK;
    };
    FS_HIP(c, hipMemcpyAsync(c->d_view_Rt.p, Rt.data(), sizeof(float) * 12 * nn, hipMemcpyHostToDevice, c->stream));
    FS_HIP(c, hipMemsetAsync(c->d_view_off.p, 0, sizeof(int64_t), c->stream));
    for (int64_t r = 0; r < rounds; ++r) {
        rc = mark_round(r);
        if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
        FS_HIP(c, fs_launch_view_count(a, c->stream));
    }
    FS_HIP(c, hipMemcpyAsync(offsets, c->d_view_off.p, sizeof(int64_t) * (nn + 1), hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipStreamSynchronize(c->stream));
    const int64_t stored = std::min<int64_t>(offsets[n], max_total);
    if (!out || stored <= 0) return FS_OK;
    FS_HIP(c, c->d_view_out.ensure((size_t)stored));
    a.max_total = stored; a.out = c->d_view_out.p;
    for (int64_t r = 0; r < rounds; ++r) {
        if (offsets[r * per_round] >= stored) break;              // (ascending: nothing of this round or a later one is stored)
        if (rounds > 1) { rc = mark_round(r); if (rc) { (void)hipStreamSynchronize(c->stream); return rc; } }
        else { a.pose_lo = 0; a.n_round = n; }
        FS_HIP(c, fs_launch_view_emit(a, c->stream));
    }
    FS_HIP(c, hipMemcpyAsync(out, c->d_view_out.p, sizeof(fs_view_landmark) * (size_t)stored, hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipStreamSynchronize(c->stream));
    if (c->d_view_out.cap * sizeof(fs_view_landmark) > ((size_t)64 << 20)) c->d_view_out.release();   // (a large list is not kept between calls)
    return FS_OK;
}

// ------------------------------------------------------------------ landmark sensor on a ground-truth cloud

}  // extern "C"

// flags from counters, the per-block counts and their offsets: enqueued; d_wl_out [0..2] then holds new / discovered / usable
static int wl_enqueue_flags(fs_ctx *c, uint32_t min_views)
{
    const size_t n_blocks = ((size_t)std::max(c->wl_m, 1) + 255) / 256;
    FS_HIP(c, c->d_wl_blocks.ensure(4 * n_blocks));
    FS_HIP(c, hipMemsetAsync(c->d_wl_out.p, 0, 3 * sizeof(int32_t), c->stream));
    FS_HIP(c, fs_launch_landmark_flags(c->d_wl_raw.p, c->d_wl_views.p, c->d_wl_flag.p, c->wl_m, min_views, c->d_wl_blocks.p,
                                       c->d_wl_blocks.p + 2 * n_blocks, c->d_wl_out.p, c->stream));
    return FS_OK;
}

// The staged cloud becomes the discovered set (n_disc landmarks, n_usable of them usable — the counts wl_enqueue_flags left): the
// compaction in ascending world index, then the body fs_upload_landmarks' device route runs.
static int wl_restage(fs_ctx *c, int32_t n_disc, int32_t n_usable)
{
    const size_t n_blocks = ((size_t)std::max(c->wl_m, 1) + 255) / 256;
    c->have_lm = false;                                          // (until the new cloud is whole)
    FS_HIP(c, c->d_cloud_raw.ensure(3 * (size_t)std::max(n_disc, 1)));
    int32_t n_chunks = 0;
    const CloudDest staged{c->d_lx, c->d_ly, c->d_lz, c->d_spheres, c->d_view_perm, c->d_view_inv};
    const int rc = order_cloud_on_device(c, c->d_cloud_raw.p, n_disc, n_usable, [&](int32_t *perm_a) -> int {
        FS_HIP(c, fs_launch_landmark_scatter(c->d_wl_raw.p, c->d_wl_flag.p, c->wl_m, c->d_wl_blocks.p + 2 * n_blocks, n_disc, n_usable,
                                             c->d_cloud_raw.p, perm_a, c->stream));
        return FS_OK;
    }, staged, n_chunks);
    if (rc) return rc;
    if (const int rc2 = staged_cloud_done(c, n_disc, n_chunks)) return rc2;
    c->wl_discovered = n_disc;
    c->wl_staged = true;
    return FS_OK;
}

// a landmark sensor as fs_sense_landmarks and fs_drive_slam take it: the caller's, or the context's defaults; refused with nothing written
static int lm_sensor_resolve(fs_ctx *c, const fs_landmark_sensor *sensor, fs_landmark_sensor &s)
{
    if (sensor) s = *sensor;
    else s = fs_landmark_sensor{c->fp.max_dist, c->fp.max_angle, c->have_world ? 1 : 0, 1, c->occ.occ_min, c->occ.occ_max, c->occ.end_margin_m};
    if (!(s.max_dist > 0.0) || !(s.max_angle > 0.0)) return fail(c, FS_E_INVALID, "sensor: max_dist and max_angle must be positive");
    if (!(s.max_dist < 1.0e9)) return fail(c, FS_E_INVALID, "sensor: max_dist must be below 1e9 m");
    if (s.line_of_sight != 0 && s.line_of_sight != 1) return fail(c, FS_E_INVALID, "sensor: line_of_sight must be 0 or 1");
    if (s.min_views < 1) return fail(c, FS_E_INVALID, "sensor: min_views must be at least 1");
    if (s.occ_min < 0 || s.occ_max > 255 || s.occ_min > s.occ_max) return fail(c, FS_E_INVALID, "sensor: occ_min / occ_max must be costs 0..255 with occ_min <= occ_max");
    if (!(s.end_margin_m >= 0.0) || !(s.end_margin_m < 1.0e6)) return fail(c, FS_E_INVALID, "sensor: end_margin_m must be finite, >= 0 and below 1e6 m");
    return FS_OK;
}

// the world cloud, the sensor's volume and its line of sight through the WORLD grid, as the sweep kernels read them
static void lm_sweep_args(fs_ctx *c, const fs_landmark_sensor &s, bool unit, int64_t poses, FsLandmarkSenseArgs &a)
{
    float cos_a, sin_a;
    fim_volume(s.max_dist, s.max_angle, a.maxd2, a.max_dist_f, a.cos2, a.cone_mode, cos_a, sin_a);
    a.cull = (unit && c->opt_cull) ? 1 : 0;
    a.lx = c->d_wl_lx.p; a.ly = c->d_wl_ly.p; a.lz = c->d_wl_lz.p; a.spheres = c->d_wl_spheres.p; a.perm = c->d_wl_perm.p;
    a.n_chunks = c->wl_chunks; a.m_world = c->wl_m;
    a.group = chunks_per_wave(poses, c->wl_chunks);
    a.los = s.line_of_sight;
    if (a.los) {
        a.world = world_dev(c);
        a.occ_min = s.occ_min; a.occ_max = s.occ_max;
        a.occ_margin = occlusion_margin(c, s.end_margin_m);
    }
    a.views = c->d_wl_views.p;
}

// ---- the gated drive's share of drive_run (fs_drive_slam)

// its refusals, after fs_drive's and before anything is written
static int slam_check(fs_ctx *c, DriveSlam &g)
{
    if (!c->have_wl) return fail(c, FS_E_STATE, "fs_upload_world_landmarks has not been called");
    if (!c->have_table) return fail(c, FS_E_STATE, "no lookup table: call fs_lookup_generate / fs_lookup_load");
    if (const int rc = lm_sensor_resolve(c, g.lm_sensor, g.s)) return rc;
    if (g.p.gate != 0 && g.p.gate != 1) return fail(c, FS_E_INVALID, "gate must be 0 or 1");
    if (g.p.gate_first_station < 0) return fail(c, FS_E_INVALID, "gate_first_station must not be negative");
    if (!std::isfinite(g.p.information_threshold)) return fail(c, FS_E_INVALID, "information_threshold must be finite");
    return FS_OK;
}

// the pose records of all stations (made once: every pose is known before the call), the sweep's and the gate's arguments, the
// outputs' presets.  d: the drive's arguments, complete.
static int slam_begin(fs_ctx *c, DriveSlam &g, const double *pose7, size_t T, const FsDriveArgs &d)
{
    const size_t R = (size_t)d.n_robots;
    g.T = T;
    g.Rt.resize(T * 12);
    const bool unit = poses_to_rt(pose7, (int32_t)T, g.Rt.data());
    FsDriveSlamArgs &a = g.a;
    a = FsDriveSlamArgs{};
    lm_sweep_args(c, g.s, unit, (int64_t)R, a.sweep);
    FsFimArgs fa{};
    if (const int rc = fill_fim_args(c, fa)) return rc;
    const size_t n_blocks = ((size_t)std::max(c->wl_m, 1) + 255) / 256;
    FS_HIP(c, c->d_wl_Rt.ensure(T * 12)); FS_HIP(c, c->d_wl_out.ensure(4)); FS_HIP(c, c->d_wl_blocks.ensure(4 * n_blocks));
    FS_HIP(c, c->d_ds_out.ensure(1 + 3 * T)); FS_HIP(c, c->d_ds_partial.ensure(R * FS_GATE_SLABS * 2));
    FS_HIP(c, hipMemcpyAsync(c->d_wl_Rt.p, g.Rt.data(), sizeof(float) * 12 * T, hipMemcpyHostToDevice, c->stream));
    FS_HIP(c, hipMemsetAsync(c->d_ds_out.p, 0, sizeof(int32_t) * (1 + 3 * T), c->stream));
    FS_HIP(c, hipMemsetAsync(c->d_wl_out.p, 0, sizeof(int32_t), c->stream));             // newly discovered: summed over the steps
    int32_t *const o = c->d_ds_out.p;
    a.sweep.Rt = c->d_wl_Rt.p; a.sweep.n = (int32_t)T; a.sweep.n_in_view = o + 1;
    a.n_robots = d.n_robots; a.n_stations = d.n_stations; a.station_off = d.station_off; a.state = d.state; a.goal = d.goal;
    a.staged = d.staged;
    a.stop_when_mapped = g.p.stop_when_mapped;
    a.flag = c->d_wl_flag.p;
    a.cull = (unit && fa.cull) ? 1 : 0;
    a.max_dist_f = fa.max_dist_f; a.maxd2 = fa.maxd2; a.cos2 = fa.cos2; a.cone_mode = fa.cone_mode;
    a.table = fa.table; a.jx0 = fa.jx0; a.jy0 = fa.jy0; a.jz0 = fa.jz0; a.tx = fa.tx; a.ty = fa.ty; a.tz = fa.tz; a.inv_step = fa.inv_step;
    a.table_full = fa.table_full; a.factor = fa.factor;
    a.occluded = c->occ.enabled != 0 ? 1 : 0;
    a.occ_min = c->occ.occ_min; a.occ_max = c->occ.occ_max; a.occ_margin = occlusion_margin(c, c->occ.end_margin_m);
    a.partial = c->d_ds_partial.p;
    a.voxels = o + 1 + T; a.information = reinterpret_cast<float *>(o + 1 + 2 * T); a.fallbacks = o;
    a.threshold = g.p.information_threshold; a.gate = g.p.gate; a.gate_first = g.p.gate_first_station;
    return FS_OK;
}

// steps 3b, 3c, 4 and 5 of step k, behind the step's merge
static int slam_step(fs_ctx *c, DriveSlam &g, int32_t k)
{
    const size_t n_blocks = ((size_t)std::max(c->wl_m, 1) + 255) / 256;
    g.a.step = k;
    FS_HIP(c, fs_launch_drive_slam_sweep(g.a, c->stream));
    FS_HIP(c, hipMemsetAsync(c->d_wl_out.p + 1, 0, 2 * sizeof(int32_t), c->stream));     // discovered, usable: the step's totals
    FS_HIP(c, fs_launch_landmark_flags(c->d_wl_raw.p, c->d_wl_views.p, c->d_wl_flag.p, c->wl_m, (uint32_t)g.s.min_views, c->d_wl_blocks.p,
                                       c->d_wl_blocks.p + 2 * n_blocks, c->d_wl_out.p, c->stream));
    FS_HIP(c, fs_launch_drive_slam_info(g.a, c->stream));
    FS_HIP(c, fs_launch_drive_slam_gate(g.a, c->stream));
    return FS_OK;
}

// back = totals [3] | d_ds_out, on their way
static int slam_copy_back(fs_ctx *c, DriveSlam &g, std::vector<int32_t> &back)
{
    back.assign(4 + 3 * g.T, 0);
    FS_HIP(c, hipMemcpyAsync(back.data(), c->d_wl_out.p, 3 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipMemcpyAsync(back.data() + 3, c->d_ds_out.p, (1 + 3 * g.T) * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    return FS_OK;
}

// after the drive's wait: the staged cloud becomes the discovered set once, by fs_sense_landmarks' rule; then the outputs
static int slam_end(fs_ctx *c, DriveSlam &g, const std::vector<int32_t> &back, const int32_t *station_status)
{
    const size_t T = g.T;
    ++c->ds_waits;                                               // (the drive's own)
    c->ds_fallbacks += back[3];
    if (back[1] < 0 || back[1] > c->wl_m || back[2] < 0 || back[2] > back[1])
        return fail(c, FS_E_HIP, "fs_drive_slam: %d discovered, %d usable of %d world landmarks", back[1], back[2], c->wl_m);
    c->wl_discovered = back[1];
    if (back[0] > 0 || !c->wl_staged) {
        if (const int rc = wl_restage(c, back[1], back[2])) return rc;
        ++c->ds_waits;                                           // (order_cloud_on_device's)
    }
    const int32_t *in_view = back.data() + 4, *voxels = in_view + T, *info = voxels + T;
    for (size_t t = 0; t < T; ++t) {
        if (g.in_view) g.in_view[t] = station_status[t] == -1 ? -1 : in_view[t];
        if (g.voxels) g.voxels[t] = voxels[t];
        if (g.information) std::memcpy(g.information + t, info + t, sizeof(float));
    }
    if (g.n_new) *g.n_new = back[0];
    if (g.n_discovered) *g.n_discovered = back[1];
    return FS_OK;
}

static void drop_world_landmarks(fs_ctx *c)
{
    c->have_wl = false; c->wl_staged = false;
    c->wl_m = c->wl_chunks = c->wl_discovered = 0;
    c->d_wl_raw.release(); c->d_wl_lx.release(); c->d_wl_ly.release(); c->d_wl_lz.release(); c->d_wl_spheres.release();
    c->d_wl_perm.release(); c->d_wl_inv.release(); c->d_wl_views.release(); c->d_wl_flag.release(); c->d_wl_blocks.release();
}

extern "C" {

int fs_upload_world_landmarks(fs_ctx *c, const float *xyz, int32_t m_world, const uint8_t *known)
{
    if (!c || m_world < 0 || (m_world > 0 && !xyz)) return FS_E_INVALID;
    if (m_world > 2000000) return fail(c, FS_E_INVALID, "at most 2,000,000 landmarks per world cloud");
    FS_HIP(c, hipSetDevice(c->device));
    if (!xyz) {                                                  // (m_world == 0) released; the staged cloud stays as it is
        FS_HIP(c, hipStreamSynchronize(c->stream));
        drop_world_landmarks(c);
        return FS_OK;
    }
    const size_t mw = (size_t)std::max(m_world, 1);
    c->have_wl = false; c->wl_staged = false;                    // (until the new world cloud is whole)
    FS_HIP(c, c->d_wl_raw.ensure(3 * mw)); FS_HIP(c, c->d_wl_views.ensure(mw)); FS_HIP(c, c->d_wl_flag.ensure(mw));
    FS_HIP(c, c->d_wl_out.ensure(4));
    std::vector<uint8_t> flag((size_t)m_world, 0);
    if (known) for (int32_t i = 0; i < m_world; ++i) flag[(size_t)i] = known[i] ? 1 : 0;
    FS_HIP(c, hipMemsetAsync(c->d_wl_views.p, 0, sizeof(uint32_t) * mw, c->stream));
    if (m_world > 0) FS_HIP(c, hipMemcpyAsync(c->d_wl_flag.p, flag.data(), (size_t)m_world, hipMemcpyHostToDevice, c->stream));
    const CloudDest world{c->d_wl_lx, c->d_wl_ly, c->d_wl_lz, c->d_wl_spheres, c->d_wl_perm, c->d_wl_inv};
    int32_t n_chunks = 0;
    if (const int rc = order_host_cloud_on_device(c, xyz, m_world, c->d_wl_raw.p, world, n_chunks)) return rc;
    c->wl_m = m_world; c->wl_chunks = n_chunks; c->wl_discovered = 0;
    c->have_wl = true;
    // the staged cloud becomes the known set: no counter reaches UINT32_MAX, so the flags are counted and nothing is new
    if (const int rc = wl_enqueue_flags(c, 0xFFFFFFFFu)) return rc;
    int32_t totals[3] = {0, 0, 0};
    FS_HIP(c, hipMemcpyAsync(totals, c->d_wl_out.p, sizeof totals, hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipStreamSynchronize(c->stream));
    return wl_restage(c, totals[1], totals[2]);
}

int fs_sense_landmarks(fs_ctx *c, int32_t n, const double *pose7, const fs_landmark_sensor *sensor, int32_t *n_in_view, int32_t *n_new,
                       int32_t *n_discovered)
{
    if (!c || n < 0 || (n > 0 && !pose7)) return FS_E_INVALID;
    fs_landmark_sensor s;
    if (const int rc = lm_sensor_resolve(c, sensor, s)) return rc;
    FS_HIP(c, hipSetDevice(c->device));
    if (!c->have_wl) return fail(c, FS_E_STATE, "fs_upload_world_landmarks has not been called");
    if (s.line_of_sight && (!c->have_grid || !c->have_world)) return fail(c, FS_E_STATE, "line_of_sight needs a world grid (fs_upload_world)");
    if (n == 0) {                                                // nothing changes; the counts are the world cloud's as it stands
        if (n_new) *n_new = 0;
        if (n_discovered) *n_discovered = c->wl_discovered;
        return FS_OK;
    }

    const size_t nn = (size_t)n;
    FsLandmarkSenseArgs a{};
    std::vector<float> Rt(nn * 12);
    lm_sweep_args(c, s, poses_to_rt(pose7, n, Rt.data()), n, a);
    a.n = n;
    FS_HIP(c, c->d_wl_Rt.ensure(nn * 12)); FS_HIP(c, c->d_wl_out.ensure(3 + nn));
    a.Rt = c->d_wl_Rt.p; a.n_in_view = c->d_wl_out.p + 3;
    FS_HIP(c, hipMemcpyAsync(c->d_wl_Rt.p, Rt.data(), sizeof(float) * 12 * nn, hipMemcpyHostToDevice, c->stream));
    FS_HIP(c, hipMemsetAsync(c->d_wl_out.p + 3, 0, sizeof(int32_t) * nn, c->stream));
    FS_HIP(c, fs_launch_sense_landmarks(a, c->stream));
    if (const int rc = wl_enqueue_flags(c, (uint32_t)s.min_views)) { (void)hipStreamSynchronize(c->stream); return rc; }
    std::vector<int32_t> out(3 + nn);
    FS_HIP(c, hipMemcpyAsync(out.data(), c->d_wl_out.p, out.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipStreamSynchronize(c->stream));                  // (the one wait: the level layout depends on the discovered count)
    if (out[1] < 0 || out[1] > c->wl_m || out[2] < 0 || out[2] > out[1])
        return fail(c, FS_E_HIP, "fs_sense_landmarks: %d discovered, %d usable of %d world landmarks", out[1], out[2], c->wl_m);
    c->wl_discovered = out[1];
    if (out[0] > 0 || !c->wl_staged)
        if (const int rc = wl_restage(c, out[1], out[2])) return rc;
    if (n_in_view) std::copy(out.begin() + 3, out.end(), n_in_view);
    if (n_new) *n_new = out[0];
    if (n_discovered) *n_discovered = out[1];
    return FS_OK;
}

int fs_world_landmarks_get(fs_ctx *c, int32_t *m_world, int32_t *n_discovered, int32_t *world_index, int32_t *views)
{
    if (!c) return FS_E_INVALID;
    FS_HIP(c, hipSetDevice(c->device));
    if (!c->have_wl) return fail(c, FS_E_STATE, "fs_upload_world_landmarks has not been called");
    const size_t mw = (size_t)c->wl_m;
    std::vector<uint8_t> flag;
    if (world_index && mw > 0) {
        flag.resize(mw);
        FS_HIP(c, hipMemcpyAsync(flag.data(), c->d_wl_flag.p, mw, hipMemcpyDeviceToHost, c->stream));
    }
    if (views && mw > 0) FS_HIP(c, hipMemcpyAsync(views, c->d_wl_views.p, sizeof(uint32_t) * mw, hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipStreamSynchronize(c->stream));
    if (world_index) {
        int32_t r = 0;
        for (size_t i = 0; i < flag.size() && r < c->wl_discovered; ++i) if (flag[i]) world_index[r++] = (int32_t)i;
    }
    if (m_world) *m_world = c->wl_m;
    if (n_discovered) *n_discovered = c->wl_discovered;
    return FS_OK;
}

int fs_staged_cloud_get(fs_ctx *c, int32_t *m, int32_t *n_chunks, float *soa, float *spheres, int32_t *perm)
{
    if (!c) return FS_E_INVALID;
    FS_HIP(c, hipSetDevice(c->device));
    if (!c->have_lm) return fail(c, FS_E_STATE, "fs_upload_landmarks has not been called");
    const size_t mp = (size_t)c->n_chunks * FS_CHUNK;
    if (soa) {
        FS_HIP(c, hipMemcpyAsync(soa, c->d_lx.p, sizeof(float) * mp, hipMemcpyDeviceToHost, c->stream));
        FS_HIP(c, hipMemcpyAsync(soa + mp, c->d_ly.p, sizeof(float) * mp, hipMemcpyDeviceToHost, c->stream));
        FS_HIP(c, hipMemcpyAsync(soa + 2 * mp, c->d_lz.p, sizeof(float) * mp, hipMemcpyDeviceToHost, c->stream));
    }
    if (spheres) FS_HIP(c, hipMemcpyAsync(spheres, c->d_spheres.p, sizeof(float) * 4 * (size_t)c->n_chunks, hipMemcpyDeviceToHost, c->stream));
    if (perm) FS_HIP(c, hipMemcpyAsync(perm, c->d_view_perm.p, sizeof(int32_t) * mp, hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipStreamSynchronize(c->stream));
    if (m) *m = c->m;
    if (n_chunks) *n_chunks = c->n_chunks;
    return FS_OK;
}

int fs_drive_slam(fs_ctx *c, int32_t n_robots, const double *station_pose7, const int32_t *n_stations, const int32_t *first_ray, const double *goal_xyz,
                  const fs_ray_params *sensor, const fs_landmark_sensor *lm_sensor, const fs_drive_slam_params *params, int32_t *status,
                  int32_t *reached, int32_t *station_status, int32_t *seen_unknown, float *station_information, int32_t *station_voxels,
                  int32_t *station_in_view, int64_t *n_seen, int64_t *n_revealed, int32_t window[6], int32_t *n_new, int32_t *n_discovered)
{
    DriveSlam g{};
    g.lm_sensor = lm_sensor;
    g.p = params ? *params : fs_drive_slam_params{253, 254, 1, 1, 550.0, 1};
    g.information = station_information; g.voxels = station_voxels; g.in_view = station_in_view;
    g.n_new = n_new; g.n_discovered = n_discovered;
    const fs_drive_params dp{g.p.block_min, g.p.block_max, g.p.stop_when_mapped};
    return drive_run(c, n_robots, station_pose7, 7, n_stations, first_ray, goal_xyz, sensor, &dp, status, reached, station_status, seen_unknown,
                     n_seen, n_revealed, window, &g);
}

int fs_information_frontier_pair(fs_ctx *c, int32_t n, const double *est_pose7, const double *triangle_xy, float *information)
{
    if (!c) return FS_E_INVALID;
    FS_HIP(c, hipSetDevice(c->device));
    if (!c->have_lm) return fail(c, FS_E_STATE, "fs_upload_landmarks has not been called");
    if (n < 0 || (n > 0 && (!est_pose7 || !triangle_xy || !information))) return fail(c, FS_E_INVALID, "null pointer");
    if (n == 0) return FS_OK;
    std::vector<float> Rt((size_t)n * 12);
    for (int32_t i = 0; i < n; ++i) pose_to_rt(est_pose7 + 7 * (size_t)i, &Rt[12 * (size_t)i]);
    DevBuf<double> &d_tri = c->d_tri;
    FS_HIP(c, c->d_Rt.ensure(Rt.size())); FS_HIP(c, d_tri.ensure((size_t)n * 6)); FS_HIP(c, c->d_info.ensure(n));
    FS_HIP(c, hipMemcpyAsync(c->d_Rt.p, Rt.data(), Rt.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    FS_HIP(c, hipMemcpyAsync(d_tri.p, triangle_xy, sizeof(double) * 6 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    // the landmark arrays are padded with far-away sentinels: those never fall inside a triangle
    FS_HIP(c, fs_launch_frontier_pair(n, c->d_lx.p, c->d_ly.p, c->d_lz.p, c->n_chunks * FS_CHUNK, c->d_Rt.p, d_tri.p, c->d_info.p, c->stream));
    FS_HIP(c, hipMemcpyAsync(information, c->d_info.p, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipStreamSynchronize(c->stream));
    return FS_OK;
}

// ------------------------------------------------------------------ key-frame pose information (row a24)

namespace {

// quatToEuler(...)[2] (util.hpp:77-88): tf2::Matrix3x3(tf2::Quaternion).getRPY, yaw component.  tf2 is third party;
// setRotation / getEulerYPR as published for Humble (gimbal-lock branch returns yaw 0).
double yaw_of_quaternion(const double q[4])
{
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double s = 2.0 / (x * x + y * y + z * z + w * w);
    const double ys = y * s, zs = z * s;
    const double m00 = 1.0 - (y * ys + z * zs), m10 = x * ys + w * zs, m20 = x * zs - w * ys;
    if (std::fabs(m20) >= 1.0) return 0.0;
    const double cp = std::cos(-std::asin(m20));
    return std::atan2(m10 / cp, m00 / cp);
}

// getVerticesOfFrustum2D (util.hpp:101-119)
void frustum_triangle(const double pose7[7], double depth, double hfov, double t[6])
{
    const double yaw = yaw_of_quaternion(pose7 + 3);
    t[0] = pose7[0]; t[1] = pose7[1];
    t[2] = pose7[0] + depth * std::cos(yaw - hfov / 2); t[3] = pose7[1] + depth * std::sin(yaw - hfov / 2);
    t[4] = pose7[0] + depth * std::cos(yaw + hfov / 2); t[5] = pose7[1] + depth * std::sin(yaw + hfov / 2);
}

}  // namespace

int fs_upload_keyframes(fs_ctx *c, int32_t n_kf, const double *kf_pose7, const int32_t *kf_offsets, const float *points_xyz)
{
    if (!c || n_kf < 0 || (n_kf > 0 && (!kf_pose7 || !kf_offsets))) return FS_E_INVALID;
    FS_HIP(c, hipSetDevice(c->device));
    const int64_t total = n_kf > 0 ? kf_offsets[n_kf] : 0;
    if (n_kf > 0 && kf_offsets[0] != 0) return fail(c, FS_E_INVALID, "kf_offsets[0] must be 0");
    for (int32_t k = 0; k < n_kf; ++k)
        if (kf_offsets[k + 1] < kf_offsets[k]) return fail(c, FS_E_INVALID, "kf_offsets must be non-decreasing");
    if (total > 0 && !points_xyz) return fail(c, FS_E_INVALID, "null pointer");
    std::vector<float> px((size_t)total), py((size_t)total), pz((size_t)total);
    for (int64_t i = 0; i < total; ++i) { px[i] = points_xyz[3 * i]; py[i] = points_xyz[3 * i + 1]; pz[i] = points_xyz[3 * i + 2]; }
    FS_HIP(c, c->d_kf_off.ensure((size_t)n_kf + 1));
    FS_HIP(c, c->d_kpx.ensure((size_t)total)); FS_HIP(c, c->d_kpy.ensure((size_t)total)); FS_HIP(c, c->d_kpz.ensure((size_t)total));
    const int32_t zero = 0;
    FS_HIP(c, hipMemcpyAsync(c->d_kf_off.p, n_kf > 0 ? kf_offsets : &zero, sizeof(int32_t) * ((size_t)n_kf + 1), hipMemcpyHostToDevice, c->stream));
    if (total > 0) {
        FS_HIP(c, hipMemcpyAsync(c->d_kpx.p, px.data(), sizeof(float) * (size_t)total, hipMemcpyHostToDevice, c->stream));
        FS_HIP(c, hipMemcpyAsync(c->d_kpy.p, py.data(), sizeof(float) * (size_t)total, hipMemcpyHostToDevice, c->stream));
        FS_HIP(c, hipMemcpyAsync(c->d_kpz.p, pz.data(), sizeof(float) * (size_t)total, hipMemcpyHostToDevice, c->stream));
    }
    FS_HIP(c, hipStreamSynchronize(c->stream));
    c->kf_pose.assign(kf_pose7, kf_pose7 + 7 * (size_t)n_kf);
    c->n_kf = n_kf; c->n_kf_points = total; c->have_kf = true;
    return FS_OK;
}

int fs_information_for_pose(fs_ctx *c, int32_t n, const double *pose7, const fs_keyframe_params *prm,
                            float *information, int32_t *n_cells, int32_t *n_points)
{
    if (!c) return FS_E_INVALID;
    FS_HIP(c, hipSetDevice(c->device));
    if (!c->have_kf) return fail(c, FS_E_STATE, "fs_upload_keyframes has not been called");
    if (!c->have_grid) return fail(c, FS_E_STATE, "fs_upload_grid has not been called");
    if (n < 0 || !prm || (n > 0 && (!pose7 || !information))) return fail(c, FS_E_INVALID, "null pointer");
    if (!(prm->q_diag > 0.0f)) return fail(c, FS_E_INVALID, "q_diag must be positive");
    if (n == 0) return FS_OK;
    // host side: triangles (libm in double, like the reference) and poses
    std::vector<double> tri((size_t)n * 12);
    std::vector<float> Rt((size_t)n * 12);
    for (int32_t i = 0; i < n; ++i) {
        frustum_triangle(pose7 + 7 * (size_t)i, prm->max_depth, prm->hfov, &tri[12 * (size_t)i]);                          // :851
        frustum_triangle(pose7 + 7 * (size_t)i, prm->max_depth + prm->max_depth_error, prm->hfov, &tri[12 * (size_t)i + 6]);   // :174
        pose_to_rt(pose7 + 7 * (size_t)i, &Rt[12 * (size_t)i]);
    }
    // getVerticesToCheck (util.hpp:134-156) of every key-frame at depth + error
    std::vector<double> chk((size_t)c->n_kf * 12);
    for (int32_t k = 0; k < c->n_kf; ++k) {
        double *o = &chk[12 * (size_t)k];
        frustum_triangle(&c->kf_pose[7 * (size_t)k], prm->max_depth + prm->max_depth_error, prm->hfov, o);
        o[6] = (o[0] + o[2]) / 2;  o[7] = (o[1] + o[3]) / 2;
        o[8] = (o[2] + o[4]) / 2;  o[9] = (o[3] + o[5]) / 2;
        o[10] = (o[4] + o[0]) / 2; o[11] = (o[5] + o[1]) / 2;
    }
    // HBM tables of the fallback pass: every point could open its own cell
    int gbits = 10;
    const uint64_t worst = std::min<uint64_t>((uint64_t)c->n_kf_points, (uint64_t)c->nx * (uint64_t)c->ny);
    while (gbits < 30 && ((uint64_t)1 << gbits) < 2 * worst) ++gbits;
    int pool = 64;
    while (pool > 1 && ((size_t)pool * 3 << gbits) * sizeof(uint32_t) > ((size_t)1 << 30)) pool >>= 1;
    FS_HIP(c, c->d_kf_gtable.ensure((size_t)pool * 3 << gbits));
    FS_HIP(c, c->d_kf_tri.ensure(tri.size())); FS_HIP(c, c->d_Rt.ensure(Rt.size())); FS_HIP(c, c->d_kf_check.ensure(chk.size()));
    FS_HIP(c, c->d_info.ensure(n)); FS_HIP(c, c->d_kf_cells.ensure(n)); FS_HIP(c, c->d_kf_points.ensure(n));
    FS_HIP(c, c->d_kf_flagged.ensure(n)); FS_HIP(c, c->d_kf_counters.ensure(1));
    FS_HIP(c, hipMemcpyAsync(c->d_kf_tri.p, tri.data(), tri.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    FS_HIP(c, hipMemcpyAsync(c->d_Rt.p, Rt.data(), Rt.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (!chk.empty()) FS_HIP(c, hipMemcpyAsync(c->d_kf_check.p, chk.data(), chk.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    FS_HIP(c, hipMemsetAsync(c->d_kf_counters.p, 0, sizeof(unsigned long long), c->stream));
    FsKfArgs a{};
    a.n = n; a.tri = c->d_kf_tri.p; a.Rt = c->d_Rt.p;
    a.n_kf = c->n_kf; a.kf_check = c->d_kf_check.p; a.kf_offsets = c->d_kf_off.p;
    a.px = c->d_kpx.p; a.py = c->d_kpy.p; a.pz = c->d_kpz.p;
    a.radius = prm->radius;
    const float q = prm->q_diag;
    a.qinv = (q * q) * (1 / (q * (q * q)));                   // Eigen's 3x3 cofactor inverse of q*I (util.hpp:722)
    a.nx = c->nx; a.ny = c->ny; a.ox = c->origin[0]; a.oy = c->origin[1]; a.res = c->res;
    a.info = c->d_info.p; a.n_cells = c->d_kf_cells.p; a.n_points = c->d_kf_points.p;
    a.flagged = c->d_kf_flagged.p; a.counters = c->d_kf_counters.p;
    a.gtable = c->d_kf_gtable.p; a.gbits = gbits;
    FS_HIP(c, fs_launch_kf_info(a, pool, c->stream));
    FS_HIP(c, hipMemcpyAsync(information, c->d_info.p, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    if (n_cells) FS_HIP(c, hipMemcpyAsync(n_cells, c->d_kf_cells.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    if (n_points) FS_HIP(c, hipMemcpyAsync(n_points, c->d_kf_points.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipStreamSynchronize(c->stream));
    return FS_OK;
}

// ------------------------------------------------------------------ fused scoring

int fs_score_candidates_dev(fs_ctx *c, int32_t n, const double *d_goal_xyz, const int32_t *d_frontier_size,
                            const uint8_t *d_blacklisted, const uint8_t *d_achievable_in, fs_record *d_records)
{
    if (!c) return FS_E_INVALID;
    FS_HIP(c, hipSetDevice(c->device));
    int rc = check_scoring_state(c, true, true);
    if (rc) return rc;
    if (n < 0 || (n > 0 && (!d_goal_xyz || !d_records))) return fail(c, FS_E_INVALID, "null device pointer");
    if (n == 0) return FS_OK;
    rc = ensure_candidate_scratch(c, n, false);
    if (rc) return rc;
    // What decides the size of the per-item scratch comes FIRST: a short list spreads each pose over several workgroups
    // (maybe_split), which may grow — and so move — every per-candidate column; no pointer into them is taken before that.
    FsFimArgs fa{};
    fill_fim_args(c, fa);
    fa.n = n;
    fa.fim21 = nullptr;
    fa.yaw_only = (c->opt_special && c->yaw_exact) ? 1 : 0;   // the ray-march kernel copies the pose's rotation out of d_yawR
    const bool occluded = c->occ.enabled != 0;
    rc = occluded ? occlusion_args(c, fa) : maybe_split(c, fa, (size_t)n, false);   // a handful of frontiers: each pose over several workgroups
    if (rc) return rc;
    FsRayArgs ra{};
    if (const int rc_args = fill_ray_args(c, ra)) return rc_args;
    ra.n = n; ra.goal = d_goal_xyz;
    ra.frontier_size = d_frontier_size; ra.blacklisted = d_blacklisted; ra.achievable_in = d_achievable_in;
    ra.ray_counts = nullptr;
    ra.arrival = c->d_arrival.p; ra.argmax = c->d_argmax.p; ra.status = c->d_status.p;
    ra.yaw = c->d_yaw.p; ra.achievable = c->d_ach.p;
    FS_HIP(c, c->d_Rt.ensure((size_t)n * 12));
    ra.yawR = c->d_yawR.p; ra.pose12 = c->d_Rt.p;
    rc = maybe_sort(c, ra);
    if (rc) return rc;
    fa.Rt = c->d_Rt.p;
    fa.status = c->d_status.p;
    if (ra.perm && c->opt_costmap) { fa.costmap = c->sort_costmap; fa.cand_key = c->sort_keys; }   // heavy blocks first next time
    bind_fim_outputs(c, fa);
    {
        ScopedTimer t(c, 0);
        FS_HIP(c, fs_launch_raymarch(ra, c->stream));
    }
    // the finish kernel assembles the records (one launch less than a separate pack)
    if (occluded) {
        fa.records = d_records;
        fa.rec_arrival = c->d_arrival.p; fa.rec_argmax = c->d_argmax.p; fa.rec_yaw = c->d_yaw.p; fa.rec_achievable = c->d_ach.p;
        return run_fim_occluded(c, fa);
    }
    // the FIM kernel visits the candidates in the same spatial order: neighbouring poses walk the same landmark chunks
    rc = run_fim_tier1(c, fa, ra.perm, 0, n << fa.split_shift);
    if (rc) return rc;
    fa.records = d_records;
    fa.rec_arrival = c->d_arrival.p; fa.rec_argmax = c->d_argmax.p; fa.rec_yaw = c->d_yaw.p; fa.rec_achievable = c->d_ach.p;
    rc = run_fim_rest(c, fa);
    if (rc) return rc;
    return FS_OK;
}

// fs_score_candidates in two halves, so that one host thread can keep several devices busy (fs_multi.hip): `begin` stages
// the candidate columns, launches the kernels and requests the records into the context's page-locked buffer — everything
// asynchronous on the context's stream; `end` waits for that stream and hands the records over.
int fs_score_candidates_begin(fs_ctx *c, int32_t n, const double *goal_xyz, const int32_t *frontier_size,
                              const uint8_t *blacklisted, const uint8_t *achievable_in)
{
    if (!c) return FS_E_INVALID;
    FS_HIP(c, hipSetDevice(c->device));
    if (n < 0 || (n > 0 && !goal_xyz)) return fail(c, FS_E_INVALID, "null pointer");
    if (n == 0) return FS_OK;
    int rc = check_scoring_state(c, true, true);
    if (rc) return rc;
    rc = upload_candidates(c, n, goal_xyz, frontier_size, blacklisted, achievable_in);
    if (rc) return rc;
    FS_HIP(c, c->d_records.ensure(n));
    FS_HIP(c, c->h_out.ensure(sizeof(fs_record) * (size_t)n));
    // a short list: the finish kernel writes the records straight into the mapped page-locked buffer
    const bool in_place = c->opt_zero_copy && n <= FS_ZERO_COPY_MAX_N && c->h_out.dev;
    rc = fs_score_candidates_dev(c, n, c->in_goal, c->in_fsize, c->in_black, c->in_achin,
                                 in_place ? reinterpret_cast<fs_record *>(c->h_out.dev) : c->d_records.p);
    if (rc) return rc;
    if (!in_place) FS_HIP(c, hipMemcpyAsync(c->h_out.p, c->d_records.p, sizeof(fs_record) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    return FS_OK;
}

int fs_score_candidates_end(fs_ctx *c, int32_t n, fs_record *records)
{
    if (!c) return FS_E_INVALID;
    if (n < 0 || (n > 0 && !records)) return fail(c, FS_E_INVALID, "null pointer");
    if (n == 0) return FS_OK;
    FS_HIP(c, hipSetDevice(c->device));
    FS_HIP(c, hipStreamSynchronize(c->stream));
    std::memcpy(records, c->h_out.p, sizeof(fs_record) * (size_t)n);
    return FS_OK;
}

}  // extern "C"

namespace {

// arrival information only, device columns in, arrival-only records out (the Fisher columns of a record stay zero)
int arrival_records_dev(fs_ctx *c, int32_t n, const double *d_goal, const int32_t *d_fsize, const uint8_t *d_black, const uint8_t *d_achin,
                        fs_record *d_records)
{
    int rc = check_scoring_state(c, true, false);
    if (rc) return rc;
    rc = ensure_candidate_scratch(c, n, false);
    if (rc) return rc;
    FsRayArgs a{};
    if (const int rc_args = fill_ray_args(c, a)) return rc_args;
    a.n = n; a.goal = d_goal; a.frontier_size = d_fsize; a.blacklisted = d_black; a.achievable_in = d_achin;
    a.arrival = c->d_arrival.p; a.argmax = c->d_argmax.p; a.status = c->d_status.p; a.yaw = c->d_yaw.p; a.achievable = c->d_ach.p;
    a.records = d_records;
    rc = maybe_sort(c, a);
    if (rc) return rc;
    ScopedTimer t(c, 0);
    FS_HIP(c, fs_launch_raymarch(a, c->stream));
    return FS_OK;
}

// The whole of a host-buffer scoring call — candidate columns (and, for ranking, the planner's path columns) in, records (and
// costs, utilities, order) out — as ONE transfer in, the kernels, ONE transfer out and one synchronisation; up to FS_GRAPH_MAX_N
// candidates the device-side sequence is a captured launch graph per power-of-two bucket (run_maybe_graphed): the list is
// padded to the bucket with blacklisted dummies, which no kernel spends work on and which a stable ascending sort leaves behind
// every real candidate.
// `planned`: the achievability and path columns already lie in device memory (fs_get_frontier_costs_planned: the planner wrote
// them on this stream) — they are read there, never staged through the host, and the call is not graphed.
struct PlannedCols {
    const uint8_t *achievable;
    const double *path_length, *path_heading;
};
// `dev`: the goal, size and blacklist columns lie in device memory as well (fs_get_frontier_costs_searched: the search wrote them);
// goal_xyz / frontier_size / blacklisted are then ignored and nothing is staged through the host.  Only with `planned`.
struct DevCols {
    const double *goal_xyz;
    const int32_t *frontier_size;
    const uint8_t *blacklisted;
};

int frontier_costs_core(fs_ctx *c, int32_t n, const double *goal_xyz, const int32_t *frontier_size, const uint8_t *blacklisted,
                        const uint8_t *achievable_in, const double *path_length, const double *path_heading,
                        double alpha, double beta, double max_vx, double max_wz, bool with_fim,
                        fs_record *records, double *weighted_cost, double *arrival_utility, double *distance_utility, int32_t *order,
                        const PlannedCols *planned = nullptr, const DevCols *dev = nullptr)
{
    if (dev && !planned) return fail(c, FS_E_INVALID, "device-resident candidate columns need the planner's columns");
    FS_HIP(c, hipSetDevice(c->device));
    int rc = check_scoring_state(c, true, with_fim);
    if (rc) return rc;
    const bool rank = path_length != nullptr || planned != nullptr;
    const bool graphed = c->opt_graph && !c->timing && n <= FS_GRAPH_MAX_N && !planned;
    const int32_t cap = graphed ? graph_bucket(n) : n;
    const size_t nn = (size_t)n, cc = (size_t)cap, pad = (cc + 15) & ~(size_t)15;
    // input block: goal | path length | path heading | frontier size | blacklist | achievable
    const size_t i_goal = 0, i_len = i_goal + 24 * cc, i_head = i_len + (rank ? 8 * cc : 0), i_fsize = i_head + (rank ? 8 * cc : 0);
    const size_t i_black = (i_fsize + 4 * cc + 15) & ~(size_t)15, i_achin = i_black + pad, total_in = i_achin + pad;
    // output block: records | cost | arrival utility | distance utility | order | range-error flag
    const size_t o_rec = 0, o_cost = o_rec + sizeof(fs_record) * cc, o_au = o_cost + (rank ? 8 * cc : 0), o_du = o_au + (rank ? 8 * cc : 0);
    const size_t o_order = o_du + (rank ? 8 * cc : 0), o_err = (o_order + (rank ? 4 * cc : 0) + 15) & ~(size_t)15, total_out = o_err + 16;
    FS_HIP(c, c->h_in.ensure(total_in)); FS_HIP(c, c->d_in.ensure(total_in));
    FS_HIP(c, c->h_out.ensure(total_out)); FS_HIP(c, c->d_out.ensure(total_out));
    char *h = c->h_in.p;
    if (!dev) {                                                 // (with dev the columns never visit the host)
        std::memcpy(h + i_goal, goal_xyz, 24 * nn);
        if (rank && !planned) { std::memcpy(h + i_len, path_length, 8 * nn); std::memcpy(h + i_head, path_heading, 8 * nn); }
        if (frontier_size) std::memcpy(h + i_fsize, frontier_size, 4 * nn); else std::memset(h + i_fsize, 0, 4 * nn);
        if (blacklisted) std::memcpy(h + i_black, blacklisted, nn); else std::memset(h + i_black, 0, nn);
        if (achievable_in) std::memcpy(h + i_achin, achievable_in, nn); else std::memset(h + i_achin, 1, nn);
    }
    if (cap > n) {                                              // the dummies: blacklisted, at the origin, nothing else
        std::memset(h + i_goal + 24 * nn, 0, 24 * (cc - nn));
        if (rank) { std::memset(h + i_len + 8 * nn, 0, 8 * (cc - nn)); std::memset(h + i_head + 8 * nn, 0, 8 * (cc - nn)); }
        std::memset(h + i_fsize + 4 * nn, 0, 4 * (cc - nn));
        std::memset(h + i_black + nn, 1, cc - nn);
        std::memset(h + i_achin + nn, 1, cc - nn);
    }
    // a short list is read and its results are written where they lie, in the mapped page-locked buffers: no transfers at all
    const bool in_place = c->opt_zero_copy && cap <= FS_ZERO_COPY_MAX_N && c->h_in.dev && c->h_out.dev;
    char *din = in_place ? c->h_in.dev : c->d_in.p, *dout = in_place ? c->h_out.dev : c->d_out.p;
    auto enqueue = [&]() -> int {
        if (!in_place && !dev) FS_HIP(c, hipMemcpyAsync(din, c->h_in.p, total_in, hipMemcpyHostToDevice, c->stream));
        const double *d_goal = reinterpret_cast<const double *>(din + i_goal);
        const int32_t *d_fsize = reinterpret_cast<const int32_t *>(din + i_fsize);
        const uint8_t *d_black = reinterpret_cast<const uint8_t *>(din + i_black), *d_achin = reinterpret_cast<const uint8_t *>(din + i_achin);
        const double *d_len = reinterpret_cast<const double *>(din + i_len), *d_head = reinterpret_cast<const double *>(din + i_head);
        if (planned) { d_achin = planned->achievable; d_len = planned->path_length; d_head = planned->path_heading; }
        if (dev) { d_goal = dev->goal_xyz; d_fsize = dev->frontier_size; d_black = dev->blacklisted; }
        fs_record *d_rec = reinterpret_cast<fs_record *>(dout + o_rec);
        int r = with_fim ? fs_score_candidates_dev(c, cap, d_goal, d_fsize, d_black, d_achin, d_rec)
                         : arrival_records_dev(c, cap, d_goal, d_fsize, d_black, d_achin, d_rec);
        if (r) return r;
        if (rank) {
            r = fs_rank_candidates_dev(c, cap, d_rec, d_black, d_len, d_head,
                                       alpha, beta, max_vx, max_wz, reinterpret_cast<double *>(dout + o_cost), reinterpret_cast<double *>(dout + o_au),
                                       reinterpret_cast<double *>(dout + o_du), reinterpret_cast<int32_t *>(dout + o_order), reinterpret_cast<int32_t *>(dout + o_err));
            if (r) return r;
        }
        if (!in_place) FS_HIP(c, hipMemcpyAsync(c->h_out.p, dout, rank ? total_out : sizeof(fs_record) * cc, hipMemcpyDeviceToHost, c->stream));
        return FS_OK;
    };
    if (graphed) {
        // what a captured sequence has baked in besides the pointers: the bucket, which kernels run, the ranking's parameters
        uint64_t key = ((uint64_t)cap << 8) | (with_fim ? 1u : 0u) | (rank ? 2u : 0u) | (in_place ? 4u : 0u) | (1ull << 40);
        if (rank) {
            const double prm[4] = {alpha, beta, max_vx, max_wz};
            uint64_t hsh = 1469598103934665603ull;
            for (size_t k = 0; k < sizeof prm; ++k) hsh = (hsh ^ reinterpret_cast<const unsigned char *>(prm)[k]) * 1099511628211ull;
            key ^= hsh << 41;
        }
        rc = run_maybe_graphed(c, key, enqueue);
    } else {
        rc = enqueue();
    }
    const hipError_t e_sync = hipStreamSynchronize(c->stream);      // (also after a failure: what was queued out of h_in has landed)
    if (rc) return rc;
    if (e_sync != hipSuccess) return fail(c, FS_E_HIP, "hipStreamSynchronize: %s", hipGetErrorString(e_sync));
    const char *ho = c->h_out.p;
    std::memcpy(records, ho + o_rec, sizeof(fs_record) * nn);
    if (rank) {
        std::memcpy(weighted_cost, ho + o_cost, 8 * nn);
        if (arrival_utility) std::memcpy(arrival_utility, ho + o_au, 8 * nn);
        if (distance_utility) std::memcpy(distance_utility, ho + o_du, 8 * nn);
        if (order) std::memcpy(order, ho + o_order, 4 * nn);       // (stable sort: the dummies come after every real candidate)
        int32_t err = 0;
        std::memcpy(&err, ho + o_err, 4);
        if (err) return fail(c, FS_E_RANGE, "utility outside [0,1] (the reference throws: FrontierCostsManager.cpp:148-149,173-174)");
    }
    return FS_OK;
}

}  // namespace

// ------------------------------------------------------------------ pieces of fs_multi_get_frontier_costs (fs_multi.hip)
// One process, several GPUs, ONE call: every member scores its block of the frontier list on its own device and stream, the
// blocks' records are moved device to device into ONE list on member 0's device (fs_multi.hip: peer copies over xGMI, each on
// the member's stream behind its kernels, an event per member that member 0's stream waits for), fs_rank_candidates_dev runs
// there on the whole list, and what the caller asked for comes back in ONE transfer.  Nothing below synchronises except _end.

hipStream_t fs_ctx_stream(fs_ctx *c) { return c->stream; }
int fs_ctx_device(const fs_ctx *c) { return c->device; }

namespace {
struct GatherLayout {
    size_t i_len, i_head, i_black, total_in;
    size_t o_rec, o_cost, o_au, o_du, o_order, o_err, total_out;
    explicit GatherLayout(size_t n)
    {
        i_len = 0; i_head = 8 * n; i_black = 16 * n; total_in = i_black + ((n + 15) & ~(size_t)15);
        o_rec = 0; o_cost = sizeof(fs_record) * n; o_au = o_cost + 8 * n; o_du = o_au + 8 * n; o_order = o_du + 8 * n;
        o_err = (o_order + 4 * n + 15) & ~(size_t)15; total_out = o_err + 16;
    }
};
}  // namespace

// member 0, first: the whole list's path columns and blacklist go to its device (one transfer, on its stream); *d_list is where
// the n records of the gathered list will live
int fs_gather_begin(fs_ctx *c, int32_t n, const uint8_t *blacklisted, const double *path_length, const double *path_heading, fs_record **d_list)
{
    if (!c || n <= 0 || !path_length || !path_heading || !d_list) return FS_E_INVALID;
    FS_HIP(c, hipSetDevice(c->device));
    const size_t nn = (size_t)n;
    const GatherLayout L(nn);
    FS_HIP(c, c->h_gin.ensure(L.total_in)); FS_HIP(c, c->d_gin.ensure(L.total_in));
    FS_HIP(c, c->h_out.ensure(L.total_out)); FS_HIP(c, c->d_out.ensure(L.total_out));
    std::memcpy(c->h_gin.p + L.i_len, path_length, 8 * nn);
    std::memcpy(c->h_gin.p + L.i_head, path_heading, 8 * nn);
    if (blacklisted) std::memcpy(c->h_gin.p + L.i_black, blacklisted, nn); else std::memset(c->h_gin.p + L.i_black, 0, nn);
    FS_HIP(c, hipMemcpyAsync(c->d_gin.p, c->h_gin.p, L.total_in, hipMemcpyHostToDevice, c->stream));
    *d_list = reinterpret_cast<fs_record *>(c->d_out.p + L.o_rec);
    return FS_OK;
}

// any member: stage the block's candidate columns and score them — into d_dst when the member may write the gathered list
// itself (member 0; a member on member 0's device), else into its own record buffer; *d_block says where the records are
int fs_block_score_begin(fs_ctx *c, int32_t n, const double *goal_xyz, const int32_t *frontier_size, const uint8_t *blacklisted,
                         const uint8_t *achievable_in, bool with_fim, fs_record *d_dst, fs_record **d_block)
{
    if (!c || n <= 0 || !goal_xyz || !d_block) return FS_E_INVALID;
    FS_HIP(c, hipSetDevice(c->device));
    int rc = check_scoring_state(c, true, with_fim);
    if (rc) return rc;
    rc = upload_candidates(c, n, goal_xyz, frontier_size, blacklisted, achievable_in);
    if (rc) return rc;
    if (!d_dst) { FS_HIP(c, c->d_records.ensure(n)); d_dst = c->d_records.p; }
    rc = with_fim ? fs_score_candidates_dev(c, n, c->in_goal, c->in_fsize, c->in_black, c->in_achin, d_dst)
                  : arrival_records_dev(c, n, c->in_goal, c->in_fsize, c->in_black, c->in_achin, d_dst);
    if (rc) return rc;
    *d_block = d_dst;
    return FS_OK;
}

// the fallback without peer access: a block's records to the member's page-locked buffer (member 0's stream copies them on from there)
int fs_block_records_to_host(fs_ctx *c, int32_t n, const fs_record *d_block, const fs_record **h_block)
{
    if (!c || n <= 0 || !d_block || !h_block) return FS_E_INVALID;
    FS_HIP(c, hipSetDevice(c->device));
    FS_HIP(c, c->h_out.ensure(sizeof(fs_record) * (size_t)n));
    FS_HIP(c, hipMemcpyAsync(c->h_out.p, d_block, sizeof(fs_record) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    *h_block = reinterpret_cast<const fs_record *>(c->h_out.p);
    return FS_OK;
}

// member 0, once its stream waits for every block: U1 costs and order over the whole list, then the ONE transfer out
int fs_gather_rank(fs_ctx *c, int32_t n, double alpha, double beta, double max_vx, double max_wz)
{
    if (!c || n <= 0) return FS_E_INVALID;
    FS_HIP(c, hipSetDevice(c->device));
    const GatherLayout L((size_t)n);
    char *in = c->d_gin.p, *out = c->d_out.p;
    const int rc = fs_rank_candidates_dev(c, n, reinterpret_cast<const fs_record *>(out + L.o_rec), reinterpret_cast<const uint8_t *>(in + L.i_black),
                                          reinterpret_cast<const double *>(in + L.i_len), reinterpret_cast<const double *>(in + L.i_head),
                                          alpha, beta, max_vx, max_wz, reinterpret_cast<double *>(out + L.o_cost), reinterpret_cast<double *>(out + L.o_au),
                                          reinterpret_cast<double *>(out + L.o_du), reinterpret_cast<int32_t *>(out + L.o_order), reinterpret_cast<int32_t *>(out + L.o_err));
    if (rc) return rc;
    FS_HIP(c, hipMemcpyAsync(c->h_out.p, out, L.total_out, hipMemcpyDeviceToHost, c->stream));
    return FS_OK;
}

int fs_gather_end(fs_ctx *c, int32_t n, fs_record *records, double *weighted_cost, double *arrival_utility, double *distance_utility, int32_t *order)
{
    if (!c || n <= 0) return FS_E_INVALID;
    FS_HIP(c, hipSetDevice(c->device));
    FS_HIP(c, hipStreamSynchronize(c->stream));
    const size_t nn = (size_t)n;
    const GatherLayout L(nn);
    const char *ho = c->h_out.p;
    if (records) std::memcpy(records, ho + L.o_rec, sizeof(fs_record) * nn);
    if (weighted_cost) std::memcpy(weighted_cost, ho + L.o_cost, 8 * nn);
    if (arrival_utility) std::memcpy(arrival_utility, ho + L.o_au, 8 * nn);
    if (distance_utility) std::memcpy(distance_utility, ho + L.o_du, 8 * nn);
    if (order) std::memcpy(order, ho + L.o_order, 4 * nn);
    int32_t err = 0;
    std::memcpy(&err, ho + L.o_err, 4);
    if (err) return fail(c, FS_E_RANGE, "utility outside [0,1] (the reference throws: FrontierCostsManager.cpp:148-149,173-174)");
    return FS_OK;
}

extern "C" {

int fs_score_candidates(fs_ctx *c, int32_t n, const double *goal_xyz, const int32_t *frontier_size,
                        const uint8_t *blacklisted, const uint8_t *achievable_in, fs_record *records)
{
    if (!c) return FS_E_INVALID;
    if (n < 0 || (n > 0 && (!goal_xyz || !records))) return fail(c, FS_E_INVALID, "null pointer");
    if (n == 0) return FS_OK;
    // up to FS_GRAPH_MAX_N candidates — the reference's operating point — the call is one captured launch graph
    if (c->opt_graph && !c->timing && n <= FS_GRAPH_MAX_N)
        return frontier_costs_core(c, n, goal_xyz, frontier_size, blacklisted, achievable_in, nullptr, nullptr, 0, 0, 0, 0, true,
                                   records, nullptr, nullptr, nullptr, nullptr);
    const int rc = fs_score_candidates_begin(c, n, goal_xyz, frontier_size, blacklisted, achievable_in);
    if (rc) return rc;
    return fs_score_candidates_end(c, n, records);
}

int fs_get_frontier_costs(fs_ctx *c, int32_t n, const double *goal_xyz, const int32_t *frontier_size, const uint8_t *blacklisted,
                          const uint8_t *achievable_in, const double *path_length, const double *path_heading,
                          double alpha, double beta, double max_vx, double max_wz, int with_fisher_information,
                          fs_record *records, double *weighted_cost, double *arrival_utility, double *distance_utility, int32_t *order)
{
    if (!c) return FS_E_INVALID;
    if (n < 0 || (n > 0 && (!goal_xyz || !path_length || !path_heading || !records || !weighted_cost))) return fail(c, FS_E_INVALID, "null pointer");
    if (n == 0) return FS_OK;
    return frontier_costs_core(c, n, goal_xyz, frontier_size, blacklisted, achievable_in, path_length, path_heading, alpha, beta, max_vx, max_wz,
                               with_fisher_information != 0, records, weighted_cost, arrival_utility, distance_utility, order);
}

// ------------------------------------------------------------------ utility + ranking

int fs_rank_candidates_dev(fs_ctx *c, int32_t n, const fs_record *d_records, const uint8_t *d_blacklisted,
                           const double *d_path_length, const double *d_path_heading,
                           double alpha, double beta, double max_vx, double max_wz,
                           double *d_weighted_cost, double *d_arrival_utility, double *d_distance_utility,
                           int32_t *d_order, int32_t *d_range_error)
{
    if (!c) return FS_E_INVALID;
    FS_HIP(c, hipSetDevice(c->device));
    if (n < 0 || (n > 0 && (!d_records || !d_path_length || !d_path_heading || !d_weighted_cost))) return fail(c, FS_E_INVALID, "null device pointer");
    if (n == 0) return FS_OK;
    // columns the caller does not want still have to be written somewhere: the context's own scratch
    if (!d_arrival_utility) { FS_HIP(c, c->d_au.ensure(n)); d_arrival_utility = c->d_au.p; }
    if (!d_distance_utility) { FS_HIP(c, c->d_du.ensure(n)); d_distance_utility = c->d_du.p; }
    if (!d_order) { FS_HIP(c, c->d_order.ensure(n)); d_order = c->d_order.p; }
    if (!d_range_error) { FS_HIP(c, c->d_err.ensure(1)); d_range_error = c->d_err.p; }
    ScopedTimer t(c, 3);
    FS_HIP(c, fs_launch_rank(n, d_records, d_blacklisted, d_path_length, d_path_heading, alpha, beta, max_vx, max_wz, c->max_gt,
                             d_weighted_cost, d_arrival_utility, d_distance_utility, d_order, d_range_error,
                             &c->rank_scratch, &c->rank_scratch_bytes, c->stream));
    return FS_OK;
}

// The host-buffer form: one packed transfer in through the context's page-locked buffer, fs_rank_candidates_dev on the
// context's own device columns, the requested columns back through the other page-locked buffer, ONE synchronisation.
int fs_rank_candidates(fs_ctx *c, int32_t n, const fs_record *records, const uint8_t *blacklisted,
                       const double *path_length, const double *path_heading,
                       double alpha, double beta, double max_vx, double max_wz,
                       double *weighted_cost, double *arrival_utility, double *distance_utility,
                       int32_t *order)
{
    if (!c) return FS_E_INVALID;
    FS_HIP(c, hipSetDevice(c->device));
    if (n < 0 || (n > 0 && (!records || !path_length || !path_heading || !weighted_cost))) return fail(c, FS_E_INVALID, "null pointer");
    if (n == 0) return FS_OK;
    const size_t nn = (size_t)n, pad = (nn + 15) & ~(size_t)15;
    const size_t o_rec = 0, o_len = o_rec + sizeof(fs_record) * nn, o_head = o_len + 8 * nn, o_black = o_head + 8 * nn;
    const size_t total_in = o_black + pad;
    FS_HIP(c, c->h_in.ensure(total_in));
    FS_HIP(c, c->d_in.ensure(total_in));
    std::memcpy(c->h_in.p + o_rec, records, sizeof(fs_record) * nn);
    std::memcpy(c->h_in.p + o_len, path_length, 8 * nn);
    std::memcpy(c->h_in.p + o_head, path_heading, 8 * nn);
    if (blacklisted) std::memcpy(c->h_in.p + o_black, blacklisted, nn);
    FS_HIP(c, hipMemcpyAsync(c->d_in.p, c->h_in.p, blacklisted ? total_in : o_black, hipMemcpyHostToDevice, c->stream));
    FS_HIP(c, c->d_cost.ensure(n)); FS_HIP(c, c->d_au.ensure(n)); FS_HIP(c, c->d_du.ensure(n));
    FS_HIP(c, c->d_order.ensure(n)); FS_HIP(c, c->d_err.ensure(1));
    const int rc = fs_rank_candidates_dev(c, n, reinterpret_cast<const fs_record *>(c->d_in.p + o_rec),
                                          blacklisted ? reinterpret_cast<const uint8_t *>(c->d_in.p + o_black) : nullptr,
                                          reinterpret_cast<const double *>(c->d_in.p + o_len), reinterpret_cast<const double *>(c->d_in.p + o_head),
                                          alpha, beta, max_vx, max_wz, c->d_cost.p, c->d_au.p, c->d_du.p, c->d_order.p, c->d_err.p);
    if (rc) return rc;
    struct Col { void *host; const void *dev; size_t bytes; };
    const Col cols[5] = {{weighted_cost, c->d_cost.p, 8 * nn}, {arrival_utility, c->d_au.p, 8 * nn}, {distance_utility, c->d_du.p, 8 * nn},
                         {order, c->d_order.p, 4 * nn}, {nullptr, c->d_err.p, 4}};
    size_t total = 16;
    for (const Col &col : cols) if (col.host) total += (col.bytes + 15) & ~(size_t)15;
    FS_HIP(c, c->h_out.ensure(total));
    FS_HIP(c, hipMemcpyAsync(c->h_out.p, c->d_err.p, 4, hipMemcpyDeviceToHost, c->stream));
    size_t off = 16;
    for (const Col &col : cols) {
        if (!col.host) continue;
        FS_HIP(c, hipMemcpyAsync(c->h_out.p + off, col.dev, col.bytes, hipMemcpyDeviceToHost, c->stream));
        off += (col.bytes + 15) & ~(size_t)15;
    }
    FS_HIP(c, hipStreamSynchronize(c->stream));
    off = 16;
    for (const Col &col : cols) {
        if (!col.host) continue;
        std::memcpy(col.host, c->h_out.p + off, col.bytes);
        off += (col.bytes + 15) & ~(size_t)15;
    }
    int32_t err = 0;
    std::memcpy(&err, c->h_out.p, 4);
    if (err) return fail(c, FS_E_RANGE, "utility outside [0,1] (the reference throws: FrontierCostsManager.cpp:148-149,173-174)");
    return FS_OK;
}

// ------------------------------------------------------------------ self test

int fs_selftest_fp64(fs_ctx *c, int32_t max_abs, int64_t *mismatches)
{
    if (!c || !mismatches || max_abs < 1 || max_abs > 2048) return FS_E_INVALID;
    FS_HIP(c, hipSetDevice(c->device));
    const int side = max_abs + 1;
    const size_t total = (size_t)side * side;
    DevBuf<double> ds, dd;
    FS_HIP(c, ds.ensure(total)); FS_HIP(c, dd.ensure(total));
    FS_HIP(c, fs_launch_selftest(max_abs, ds.p, dd.p, c->stream));
    std::vector<double> hs(total), hd(total);
    FS_HIP(c, hipMemcpyAsync(hs.data(), ds.p, total * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipMemcpyAsync(hd.data(), dd.p, total * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipStreamSynchronize(c->stream));
    ds.release(); dd.release();
    int64_t bad = 0;
    for (int dx = 0; dx < side; ++dx)
        for (int dy = 0; dy < side; ++dy) {
            const size_t t = (size_t)dx * side + dy;
            // The reference calls std::hypot (Helpers.cpp:49); glibc's hypot is within 1 ulp but not
            // always correctly rounded, so the device (and this check) use the correctly rounded sqrt of
            // the exact integer dx^2+dy^2.  A 1-ulp change of dist cannot flip (unsigned)(scale*abs_da):
            // tests/test_oracle_raycast.py::test_hypot_vs_sqrt_never_changes_step_count proves it exhaustively.
            const double dist = std::sqrt((double)((long long)dx * dx + (long long)dy * dy));
            const double q = (dist == 0.0) ? 1.0 : 40.0 / dist;
            if (std::memcmp(&dist, &hs[t], 8) != 0) ++bad;
            if (std::memcmp(&q, &hd[t], 8) != 0) ++bad;
        }
    *mismatches = bad;
    return FS_OK;
}

}  // extern "C"

// ================================================================== batched grid planner (fs_navfn.hip)
// FrontierCostCalculator::setPlanForFrontier ("A*PlannerDistance", DEP/src/CostCalculator.cpp:193-393) for a whole frontier list:
// every frontier plans back to the same robot cell (setStart(map_goal); setGoal(map_start), :269-271), so ONE potential field
// from the robot serves the list and only the descents are per frontier.

namespace {

// CostCalculator.cpp:209-217: quatToEuler's yaw of the robot and the bearing of the goal, both in [0, 2 pi), the smaller way round
double nav_heading(const double pose7[7], double gx, double gy)
{
    const double qx = pose7[3], qy = pose7[4], qz = pose7[5], qw = pose7[6];
    double robot_yaw = std::atan2(2.0 * (qw * qz + qx * qy), 1.0 - 2.0 * (qy * qy + qz * qz));
    if (robot_yaw < 0) robot_yaw = robot_yaw + (M_PI * 2);
    double goal_yaw = std::atan2(gy - pose7[1], gx - pose7[0]);
    if (goal_yaw < 0) goal_yaw = goal_yaw + (M_PI * 2);
    double h = std::abs(robot_yaw - goal_yaw);
    if (h > M_PI) h = (2 * M_PI) - h;
    return h;
}

int navfn_wave_check(fs_ctx *c);

int nav_check(fs_ctx *c, const double robot_pose7[7])
{
    if (!robot_pose7) return fail(c, FS_E_INVALID, "null robot pose");
    const int rc = grid2d_check(c, "the grid planner");
    if (rc || c->nav_search != FS_GRID_SEARCH_REFERENCE) return rc;
    return navfn_wave_check(c);
}

// The field for (robot cell, allow_unknown) on the staged grid: the cached one, or built now (synchronises the stream).
int navfn_field(fs_ctx *c, int32_t rx, int32_t ry, int32_t allow, const float **field)
{
    const int nx = c->nx, ny = c->ny;
    const size_t ns = (size_t)nx * (size_t)ny;
    allow = allow ? 1 : 0;
    if (!(c->nav_valid && c->nav_gen == c->grid_gen && c->nav_rx == rx && c->nav_ry == ry && c->nav_allow == allow)) {
        c->nav_valid = false;
        const size_t tiles = (size_t)((nx + NAVFN_TILE - 1) / NAVFN_TILE) * (size_t)((ny + NAVFN_TILE - 1) / NAVFN_TILE);
        FS_HIP(c, c->d_nav_cost.ensure(ns));
        FS_HIP(c, c->d_nav_pot.ensure(2 * ns));
        FS_HIP(c, c->d_nav_flags.ensure(2 * tiles));
        FS_HIP(c, c->d_nav_any.ensure(PLAN_BATCH));
        float *buf[2] = {c->d_nav_pot.p, c->d_nav_pot.p + ns};
        uint32_t *flags[2] = {c->d_nav_flags.p, c->d_nav_flags.p + tiles};
        {
            ScopedTimer t(c, 6);
            FS_HIP(c, fs_launch_navfn_costs(c->d_cells.p, nx, ny, allow, c->d_nav_cost.p, c->stream));
            FS_HIP(c, fs_launch_navfn_init(buf[0], buf[1], nx, ny, rx, ry, flags[0], c->stream));
        }
        int64_t rounds = 0, launched = 0;
        const auto launch = [&](int64_t r0, int count) -> int {
            {
                ScopedTimer t(c, 7);
                for (int64_t k = 0, r = r0; k < count; ++k, ++r)
                    FS_HIP(c, fs_launch_navfn_round(buf[r & 1], buf[(r + 1) & 1], c->d_nav_cost.p, flags[r & 1], flags[(r + 1) & 1], nx, ny,
                                                    c->d_nav_any.p + k, c->stream));
            }
            c->nav_launches += count;
            launched = r0 + count;
            return FS_OK;
        };
        const int rc = poll_rounds(c, c->d_nav_any.p, PLAN_BATCH_FIRST, PLAN_BATCH, 1, PLAN_MAX_ROUNDS, "potential field", PLAN_MAX_ROUNDS,
                                   launch, &rounds);
        if (rc) return rc;
        c->nav_buf = (int32_t)(launched & 1);        // (after a quiet round both buffers hold the field)
        c->nav_valid = true;
        c->nav_gen = c->grid_gen; c->nav_rx = rx; c->nav_ry = ry; c->nav_allow = allow;
        c->nav_rounds = rounds;
        ++c->nav_builds;
    }
    *field = c->d_nav_pot.p + (size_t)c->nav_buf * ns;
    return FS_OK;
}

// Staging block of the path kernel in h_nav_in / d_nav_in: goal cells | headings.
struct NavInLayout {
    size_t cell, head, total;
    explicit NavInLayout(size_t n) : cell(0), head((4 * n + 7) & ~(size_t)7), total(head + 8 * n) {}
};

int32_t navfn_max_cycles(const fs_ctx *c) { return 4 * std::max(c->nx, c->ny); }      // CostCalculator.cpp:284

// every buffer a plan of nn goals uses is sized before a pointer into any of them is taken
int navfn_ensure(fs_ctx *c, size_t nn)
{
    const NavInLayout I(nn);
    FS_HIP(c, c->h_nav_in.ensure(I.total)); FS_HIP(c, c->d_nav_in.ensure(I.total));
    FS_HIP(c, c->d_nav_out.ensure(PlanOutLayout(nn).total));
    FS_HIP(c, c->d_nav_path.ensure(nn * 2 * (size_t)navfn_max_cycles(c)));
    return FS_OK;
}

// The path kernel's arguments on `field` for the goal cells and headings in d_nav_in: the four columns land in d_nav_out.
FsNavfnPathArgs navfn_path_args(fs_ctx *c, const float *field, int32_t n, int32_t rx, int32_t ry)
{
    const NavInLayout I((size_t)n);
    const PlanOutLayout O((size_t)n);
    FsNavfnPathArgs a{};
    a.pot = field; a.nx = c->nx; a.ny = c->ny; a.n = n;
    a.goal_cell = reinterpret_cast<const int32_t *>(c->d_nav_in.p + I.cell);
    a.heading_in = reinterpret_cast<const double *>(c->d_nav_in.p + I.head);
    a.robot_x = rx; a.robot_y = ry; a.max_cycles = navfn_max_cycles(c);
    a.scratch = c->d_nav_path.p;
    a.ox = c->origin[0]; a.oy = c->origin[1]; a.res = c->res;
    a.path_length = reinterpret_cast<double *>(c->d_nav_out.p + O.len);
    a.path_length_m = reinterpret_cast<double *>(c->d_nav_out.p + O.len_m);
    a.path_heading = reinterpret_cast<double *>(c->d_nav_out.p + O.head);
    a.achievable = reinterpret_cast<uint8_t *>(c->d_nav_out.p + O.ach);
    return a;
}

// The path kernel on the one converged `field`.
int navfn_paths(fs_ctx *c, const float *field, int32_t n, int32_t rx, int32_t ry)
{
    const FsNavfnPathArgs a = navfn_path_args(c, field, n, rx, ry);
    ScopedTimer t(c, 8);
    FS_HIP(c, fs_launch_navfn_paths(a, c->stream));
    return FS_OK;
}

// ---- the REFERENCE search (fs_set_grid_search): per distinct goal cell the calcNavFnAstar wave from the robot cell that stops at it
// (fs_navfn_wave.h), one wavefront per wave, then calcPath on that wave's field.  The converged field and its cache are not touched.
struct NwIdxLayout {
    size_t stats, cell, wave, first, limit, total;       // in int32 words of d_nw_idx
    explicit NwIdxLayout(size_t n) : stats(0), cell(4), wave(4 + n), first(4 + 2 * n), limit(4 + 3 * n), total(4 + 4 * n) {}
};

int navfn_wave_check(fs_ctx *c)
{
    if (c->nx > FS_NW_MAX_SIDE || c->ny > FS_NW_MAX_SIDE)
        return fail(c, FS_E_INVALID, "the REFERENCE grid search takes maps of at most %d cells a side (this one: %d x %d)", FS_NW_MAX_SIDE, c->nx, c->ny);
    return FS_OK;
}

// The slots for up to max_waves waves of a list of nn frontiers, the cost array, and the kernels' arguments.
int navfn_wave_prepare(fs_ctx *c, int32_t rx, int32_t ry, int32_t allow, size_t nn, int64_t max_waves, FsNavfnWaveArgs &w)
{
    const size_t ns = (size_t)c->nx * (size_t)c->ny, cap = (size_t)c->nw_opt_cap;
    const int64_t per_slot = (int64_t)(5 * ns + 12 * cap);
    int64_t slots = c->nw_opt_slots > 0 ? c->nw_opt_slots : std::max<int64_t>(1, c->nw_opt_bytes / per_slot);
    slots = std::min<int64_t>(std::min<int64_t>(slots, 65535), std::max<int64_t>(1, max_waves));
    const NwIdxLayout L(nn);
    FS_HIP(c, c->d_nav_cost.ensure(ns));
    FS_HIP(c, c->d_nw_pot.ensure((size_t)slots * ns));
    FS_HIP(c, c->d_nw_pend.ensure((size_t)slots * ns));
    FS_HIP(c, c->d_nw_buf.ensure((size_t)slots * 3 * cap));
    FS_HIP(c, c->d_nw_idx.ensure(L.total));
    FS_HIP(c, fs_launch_navfn_costs(c->d_cells.p, c->nx, c->ny, allow ? 1 : 0, c->d_nav_cost.p, c->stream));
    w = FsNavfnWaveArgs{};
    w.cost = c->d_nav_cost.p; w.nx = c->nx; w.ny = c->ny; w.rx = rx; w.ry = ry;
    w.cap = (int32_t)cap; w.slots = (int32_t)slots;
    w.pot = c->d_nw_pot.p; w.pending = c->d_nw_pend.p; w.buf = c->d_nw_buf.p;
    w.wave_cell = c->d_nw_idx.p + L.cell; w.frontier_wave = c->d_nw_idx.p + L.wave;
    w.stats = c->d_nw_idx.p + L.stats; w.wave_limit = c->d_nw_idx.p + L.limit;
    return FS_OK;
}

// Batch by batch, with no synchronisation in between: the fill, the waves, the descents of that batch's frontiers before the slots
// are used again.  `waves` bounds the call's waves (the host form: their number); the descents of batch 0 also write the columns
// of the frontiers without a wave, so they run even where there is none.
int navfn_wave_batches(fs_ctx *c, const FsNavfnWaveArgs &w, int64_t waves, int32_t n, int32_t rx, int32_t ry)
{
    const FsNavfnPathArgs a = navfn_path_args(c, w.pot, n, rx, ry);
    const int64_t batches = (waves + w.slots - 1) / w.slots;
    c->nw_batches = batches;
    for (int64_t b = 0; b < std::max<int64_t>(batches, 1); ++b) {
        const int64_t base = b * w.slots;
        if (b < batches) {
            ScopedTimer t(c, 7);
            FS_HIP(c, fs_launch_navfn_wave_batch(w, (int32_t)base, (int32_t)std::min<int64_t>(w.slots, waves - base), c->stream));
        }
        ScopedTimer t(c, 8);
        FS_HIP(c, fs_launch_navfn_paths_wave(a, w, (int32_t)base, c->stream));
    }
    return FS_OK;
}

// navfn_plan_enqueue's tail under REFERENCE: cell [n] are the goal cells on the host (-1: not planned), d_nav_in is on its way.
int navfn_wave_plan_host(fs_ctx *c, int32_t rx, int32_t ry, int32_t allow, int32_t n, const int32_t *cell)
{
    const size_t nn = (size_t)n;
    std::vector<int32_t> distinct;
    for (size_t i = 0; i < nn; ++i)
        if (cell[i] >= 0) distinct.push_back(cell[i]);
    std::sort(distinct.begin(), distinct.end());
    distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
    FsNavfnWaveArgs w;
    const int rc = navfn_wave_prepare(c, rx, ry, allow, nn, (int64_t)distinct.size(), w);
    if (rc) return rc;
    const NwIdxLayout L(nn);
    FS_HIP(c, c->h_nw_idx.ensure(4 * L.first));
    int32_t *h = reinterpret_cast<int32_t *>(c->h_nw_idx.p);
    h[0] = (int32_t)distinct.size(); h[1] = h[2] = h[3] = 0;
    for (size_t k = 0; k < nn; ++k) h[L.cell + k] = k < distinct.size() ? distinct[k] : -1;
    for (size_t i = 0; i < nn; ++i)
        h[L.wave + i] = cell[i] < 0 ? -1 : (int32_t)(std::lower_bound(distinct.begin(), distinct.end(), cell[i]) - distinct.begin());
    FS_HIP(c, hipMemcpyAsync(c->d_nw_idx.p, h, 4 * L.first, hipMemcpyHostToDevice, c->stream));
    return navfn_wave_batches(c, w, (int64_t)distinct.size(), n, rx, ry);
}

// navfn_plan_enqueue_dev's tail under REFERENCE: the goal cells are in d_nav_in (-1: not planned) and the distinct ones are listed
// on the device, so the host cuts batches for n waves and the kernels of a batch beyond the last wave return at once.
int navfn_wave_plan_dev(fs_ctx *c, int32_t rx, int32_t ry, bool robot_on, int32_t allow, int32_t n)
{
    const size_t nn = (size_t)n;
    FsNavfnWaveArgs w;
    const int rc = navfn_wave_prepare(c, rx, ry, allow, nn, n, w);
    if (rc) return rc;
    const NwIdxLayout L(nn);
    const NavInLayout I(nn);
    FS_HIP(c, hipMemsetAsync(c->d_nw_idx.p, 0, 16, c->stream));
    FS_HIP(c, fs_launch_navfn_wave_cells(reinterpret_cast<const int32_t *>(c->d_nav_in.p + I.cell), n, c->d_nw_idx.p + L.first, c->d_nw_idx.p + L.cell,
                                         c->d_nw_idx.p + L.wave, c->d_nw_idx.p + L.stats, c->stream));
    return navfn_wave_batches(c, w, robot_on ? n : 0, n, rx, ry);
}

// Goal cells and headings staged, the field (cached or built), the path kernel: the four columns land in d_nav_out on the
// context's stream.  Not synchronised.
int navfn_plan_enqueue(fs_ctx *c, const double robot7[7], int32_t allow, int32_t n, const double *goal_xyz, const uint8_t *achievable_in)
{
    const size_t nn = (size_t)n;
    const NavInLayout I(nn);
    int rc = navfn_ensure(c, nn);
    if (rc) return rc;
    int32_t rx = 0, ry = 0;
    const bool robot_on = grid_world_to_map(c, robot7[0], robot7[1], rx, ry);
    int32_t *cell = reinterpret_cast<int32_t *>(c->h_nav_in.p + I.cell);
    double *head = reinterpret_cast<double *>(c->h_nav_in.p + I.head);
    bool need_field = false;
    for (size_t i = 0; i < nn; ++i) {
        int32_t gx = 0, gy = 0;
        const bool planned = (!achievable_in || achievable_in[i]) && robot_on && grid_world_to_map(c, goal_xyz[3 * i], goal_xyz[3 * i + 1], gx, gy);
        cell[i] = planned ? gy * c->nx + gx : -1;
        head[i] = planned ? nav_heading(robot7, goal_xyz[3 * i], goal_xyz[3 * i + 1]) : 0.0;
        need_field |= planned;
    }
    if (c->nav_search == FS_GRID_SEARCH_REFERENCE) {
        FS_HIP(c, hipMemcpyAsync(c->d_nav_in.p, c->h_nav_in.p, I.total, hipMemcpyHostToDevice, c->stream));
        return navfn_wave_plan_host(c, rx, ry, allow, n, cell);
    }
    const float *field = nullptr;
    if (need_field) { rc = navfn_field(c, rx, ry, allow, &field); if (rc) return rc; }
    FS_HIP(c, hipMemcpyAsync(c->d_nav_in.p, c->h_nav_in.p, I.total, hipMemcpyHostToDevice, c->stream));
    return navfn_paths(c, field, n, rx, ry);
}

// navfn_plan_enqueue for goal points that lie in device memory (fs_get_frontier_costs_searched: the search wrote them): the goal
// cells are computed on the device; only the headings come from the host, where setPlanForFrontier's heading is defined with the
// host's libm (h_heading [n], used where a plan succeeds).  Every goal is planned (no achievable_in).  Not synchronised.
int navfn_plan_enqueue_dev(fs_ctx *c, const double robot7[7], int32_t allow, int32_t n, const double *d_goal_xyz, const double *h_heading)
{
    const size_t nn = (size_t)n;
    const NavInLayout I(nn);
    int rc = navfn_ensure(c, nn);
    if (rc) return rc;
    int32_t rx = 0, ry = 0;
    const bool robot_on = grid_world_to_map(c, robot7[0], robot7[1], rx, ry);
    const bool reference = c->nav_search == FS_GRID_SEARCH_REFERENCE;
    const float *field = nullptr;
    if (!reference && robot_on && n > 0) { rc = navfn_field(c, rx, ry, allow, &field); if (rc) return rc; }
    std::memcpy(c->h_nav_in.p + I.head, h_heading, 8 * nn);
    FS_HIP(c, hipMemcpyAsync(c->d_nav_in.p + I.head, c->h_nav_in.p + I.head, 8 * nn, hipMemcpyHostToDevice, c->stream));
    FS_HIP(c, fs_launch_goal_cells(d_goal_xyz, n, c->nx, c->ny, c->origin[0], c->origin[1], c->res, robot_on ? 1 : 0,
                                   reinterpret_cast<int32_t *>(c->d_nav_in.p + I.cell), c->stream));
    if (reference) return navfn_wave_plan_dev(c, rx, ry, robot_on, allow, n);
    return navfn_paths(c, field, n, rx, ry);
}

// A planner's four columns for the caller: `enqueue()` plans n goals into d_out, the columns come up through h_out (synchronises
// the stream).
template <class Enqueue>
int plan_to_host(fs_ctx *c, const DevBuf<char> &d_out, PinnedBuf &h_out, int32_t n, Enqueue enqueue, double *path_length,
                 double *path_length_m, double *path_heading, uint8_t *achievable)
{
    const int rc = enqueue();
    if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
    const size_t nn = (size_t)n;
    const PlanOutLayout O(nn);
    FS_HIP(c, h_out.ensure(O.total));
    FS_HIP(c, hipMemcpyAsync(h_out.p, d_out.p, O.total, hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipStreamSynchronize(c->stream));
    plan_columns_to_caller(h_out, nn, path_length, path_length_m, path_heading, achievable);
    return FS_OK;
}

// Ranking on a planner's device columns: `enqueue()` plans n goals into d_out, `rank(cols)` scores and ranks on the columns where
// the planner wrote them (scoring reads its achievability, ranking its path columns); path_length_m, if asked for, comes up
// through h_out, which is sized before the plan is enqueued.
template <class Enqueue, class Rank>
int rank_on_plan(fs_ctx *c, const DevBuf<char> &d_out, PinnedBuf &h_out, int32_t n, Enqueue enqueue, Rank rank, double *path_length_m)
{
    const size_t nn = (size_t)n;
    const PlanOutLayout O(nn);
    FS_HIP(c, h_out.ensure(O.total));
    int rc = enqueue();
    if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
    if (path_length_m) FS_HIP(c, hipMemcpyAsync(h_out.p + O.len_m, d_out.p + O.len_m, 8 * nn, hipMemcpyDeviceToHost, c->stream));
    const PlannedCols cols{reinterpret_cast<const uint8_t *>(d_out.p + O.ach), reinterpret_cast<const double *>(d_out.p + O.len),
                           reinterpret_cast<const double *>(d_out.p + O.head)};
    rc = rank(cols);
    if (rc) {
        // (frontier_costs_core can fail before its own synchronisation: the copy into h_out above must have landed before a later
        // call may grow that buffer)
        (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    if (path_length_m) std::memcpy(path_length_m, h_out.p + O.len_m, 8 * nn);
    return FS_OK;
}

// The pose records of fs_plan_paths_information / fs_roadmap_routes (fs_pathinfo.hip: keys, sort, heads, records) for up to `bound`
// way points or legs (`what` in the error text): the d_pi_* buffers are sized, `a` is pointed at them, the kernels are launched and
// the header (total, distinct) is on its way to `hdr`.  Not synchronised; `stop` is the caller's return after a failed launch.
template <class Stop>
int pathinfo_prepare(fs_ctx *c, FsPathInfoArgs &a, int64_t bound, bool dump, const char *what, int64_t *hdr, Stop stop)
{
    const size_t room = (size_t)bound;
    if (a.dedup) { FS_HIP(c, c->d_pi_key.ensure(2 * room)); }
    FS_HIP(c, c->d_pi_idx.ensure(5 * room));
    FS_HIP(c, c->d_pi_rt.ensure(12 * room));
    if (dump) { FS_HIP(c, c->d_pi_pose.ensure(7 * room)); FS_HIP(c, c->d_pi_val.ensure(room)); }
    a.bound = bound;
    a.key_in = c->d_pi_key.p; a.key_out = c->d_pi_key.p + room;
    a.wp_in = c->d_pi_idx.p; a.wp_out = a.wp_in + room; a.head = a.wp_out + room; a.rank = a.head + room; a.slot = a.rank + room;
    a.rt = c->d_pi_rt.p;
    a.pose7 = dump ? c->d_pi_pose.p : nullptr;
    a.wp_info = dump ? c->d_pi_val.p : nullptr;
    if (fs_launch_pathinfo_prepare(a, c->stream) != hipSuccess) return stop(fail(c, FS_E_HIP, "%s: launch failed", what));
    FS_HIP(c, hipMemcpyAsync(hdr, a.hdr, 16, hipMemcpyDeviceToHost, c->stream));
    return FS_OK;
}

// fs_score_fim's launch sequence on n > 0 pose records that lie on the device (rt [n][12]); *info is the worker's info_ref column.
// `split`: a call of few poses may spread each over several workgroups (maybe_split), which changes the order of a pose's
// partial sums with n — a caller whose values must not depend on how its poses are batched passes false.  What decides the size of
// the per-item scratch comes before any pointer into it.  A refused scratch returns as it is; every later failure goes through
// the caller's `stop`.
template <class Stop>
int score_records(fs_ctx *c, const float *rt, int64_t n, bool split, Stop stop, const float **info)
{
    int rc = ensure_candidate_scratch(c, (size_t)n, false);
    if (rc) return rc;
    FsFimArgs fa{};
    if (const int rc_args = fill_fim_args(c, fa)) return rc_args;
    fa.n = (int32_t)n;
    fa.info_only = c->opt_special ? 1 : 0;
    if (fa.info_only && fa.skip32 < 20) fa.skip32 = 20;        // (as fs_score_fim_begin)
    const bool occluded = c->occ.enabled != 0;
    if (occluded) rc = occlusion_args(c, fa);
    else if (split) rc = maybe_split(c, fa, (size_t)n, false);
    if (rc) return stop(rc);
    fa.Rt = rt;
    bind_fim_outputs(c, fa);
    if (occluded) rc = run_fim_occluded(c, fa);
    else {
        rc = run_fim_tier1(c, fa, nullptr, 0, fa.n << fa.split_shift);
        if (rc) return stop(rc);
        rc = run_fim_rest(c, fa);
    }
    if (rc) return stop(rc);
    *info = fa.info_ref;
    return FS_OK;
}

// ... and the information of the pose records of pathinfo_prepare (distinct > 0, known after the caller's synchronisation); a.info
// is where the finish kernel finds it.
template <class Stop>
int pathinfo_score(fs_ctx *c, FsPathInfoArgs &a, int64_t distinct, Stop stop)
{
    return score_records(c, c->d_pi_rt.p, distinct, true, stop, &a.info);
}

}  // namespace

extern "C" {

int fs_navfn_potential(fs_ctx *c, const double robot_pose7[7], int32_t allow_unknown, float *potential)
{
    if (!c) return FS_E_INVALID;
    if (!potential) return fail(c, FS_E_INVALID, "null pointer");
    int rc = nav_check(c, robot_pose7);
    if (rc) return rc;
    int32_t rx = 0, ry = 0;
    if (!grid_world_to_map(c, robot_pose7[0], robot_pose7[1], rx, ry)) return fail(c, FS_E_INVALID, "the robot is off the costmap: no potential field");
    const float *field = nullptr;
    rc = navfn_field(c, rx, ry, allow_unknown, &field);
    if (rc) return rc;
    FS_HIP(c, hipMemcpyAsync(potential, field, sizeof(float) * (size_t)c->nx * (size_t)c->ny, hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipStreamSynchronize(c->stream));
    return FS_OK;
}

int fs_set_grid_search(fs_ctx *c, int32_t search)
{
    if (!c) return FS_E_INVALID;
    if (search != FS_GRID_SEARCH_CONVERGED && search != FS_GRID_SEARCH_REFERENCE) return fail(c, FS_E_INVALID, "unknown grid search %d", search);
    c->nav_search = search;
    return FS_OK;
}

int fs_navfn_wave_potential(fs_ctx *c, const double robot_pose7[7], int32_t allow_unknown, const double goal_xyz[3], float *potential, int32_t *limit)
{
    if (!c) return FS_E_INVALID;
    if (!potential || !goal_xyz || !robot_pose7) return fail(c, FS_E_INVALID, "null pointer");
    int rc = grid2d_check(c, "the grid planner");
    if (rc) return rc;
    rc = navfn_wave_check(c);
    if (rc) return rc;
    int32_t rx = 0, ry = 0, gx = 0, gy = 0;
    if (!grid_world_to_map(c, robot_pose7[0], robot_pose7[1], rx, ry)) return fail(c, FS_E_INVALID, "the robot is off the costmap: no wave");
    if (!grid_world_to_map(c, goal_xyz[0], goal_xyz[1], gx, gy)) return fail(c, FS_E_INVALID, "the goal is off the costmap: no wave");
    FsNavfnWaveArgs w;
    rc = navfn_wave_prepare(c, rx, ry, allow_unknown, 1, 1, w);
    if (rc) return rc;
    const NwIdxLayout L(1);
    FS_HIP(c, c->h_nw_idx.ensure(4 * L.total));
    int32_t *h = reinterpret_cast<int32_t *>(c->h_nw_idx.p);
    h[0] = 1; h[1] = h[2] = h[3] = 0;
    h[L.cell] = gy * c->nx + gx; h[L.wave] = 0;
    const auto stop = [&](int code) { (void)hipStreamSynchronize(c->stream); return code; };
    FS_HIP(c, hipMemcpyAsync(c->d_nw_idx.p, h, 4 * L.first, hipMemcpyHostToDevice, c->stream));
    c->nw_batches = 1;
    if (fs_launch_navfn_wave_batch(w, 0, 1, c->stream) != hipSuccess) return stop(fail(c, FS_E_HIP, "the wave: launch failed"));
    FS_HIP(c, hipMemcpyAsync(potential, w.pot, sizeof(float) * (size_t)c->nx * (size_t)c->ny, hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipMemcpyAsync(h + L.limit, w.wave_limit, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipStreamSynchronize(c->stream));
    if (limit) *limit = h[L.limit];
    return FS_OK;
}

int fs_plan_paths(fs_ctx *c, const double robot_pose7[7], int32_t allow_unknown, int32_t n, const double *goal_xyz,
                  const uint8_t *achievable_in, double *path_length, double *path_length_m, double *path_heading, uint8_t *achievable)
{
    if (!c) return FS_E_INVALID;
    if (n < 0 || (n > 0 && (!goal_xyz || !path_length || !path_length_m || !path_heading || !achievable))) return fail(c, FS_E_INVALID, "null pointer");
    int rc = nav_check(c, robot_pose7);
    if (rc) return rc;
    if (n == 0) return FS_OK;
    return plan_to_host(c, c->d_nav_out, c->h_nav_out, n,
                        [&] { return navfn_plan_enqueue(c, robot_pose7, allow_unknown, n, goal_xyz, achievable_in); },
                        path_length, path_length_m, path_heading, achievable);
}

int fs_plan_paths_information(fs_ctx *c, const double robot_pose7[7], int32_t allow_unknown, int32_t n, const double *goal_xyz,
                              const uint8_t *achievable_in, const fs_path_info_params *params, double *path_length,
                              double *path_length_m, double *path_heading, uint8_t *achievable, int32_t *n_waypoints, double *info_mean,
                              float *info_min, int32_t *first_unsafe, int64_t max_waypoints, int64_t *n_total, int32_t *waypoint_offset,
                              double *waypoint_pose7, float *waypoint_info)
{
    if (!c) return FS_E_INVALID;
    if (n < 0 || (n > 0 && (!goal_xyz || !path_length || !path_length_m || !path_heading || !achievable || !n_waypoints || !info_mean ||
                            !info_min || !first_unsafe)))
        return fail(c, FS_E_INVALID, "null pointer");
    const int dump_ptrs = (n_total ? 1 : 0) + (waypoint_offset ? 1 : 0) + (waypoint_pose7 ? 1 : 0) + (waypoint_info ? 1 : 0);
    if (dump_ptrs != 0 && dump_ptrs != 4) return fail(c, FS_E_INVALID, "the way-point dump takes all four pointers or none");
    const bool dump = dump_ptrs == 4;
    if (dump && max_waypoints < 0) return fail(c, FS_E_INVALID, "negative max_waypoints");
    const fs_path_info_params def = {1.5, 10, 550.0};        // CostCalculator.cpp:328, :332; FisherInfoBTPlugin.cpp:20
    const fs_path_info_params prm = params ? *params : def;
    if (!(prm.sample_distance_m >= 0.0)) return fail(c, FS_E_INVALID, "sample_distance_m must not be negative");
    if (prm.lookahead_points < 0) return fail(c, FS_E_INVALID, "lookahead_points must not be negative");
    if (!std::isfinite(prm.fi_threshold)) return fail(c, FS_E_INVALID, "fi_threshold must be finite");
    int rc = nav_check(c, robot_pose7);
    if (rc) return rc;
    rc = check_scoring_state(c, false, true);
    if (rc) return rc;
    c->pi_waypoints = 0; c->pi_distinct = 0;
    if (dump) { *n_total = 0; waypoint_offset[0] = 0; }
    if (n == 0) return FS_OK;
    const size_t nn = (size_t)n;
    // s = (int)(sample_distance / resolution) (:328); a quotient beyond the int range samples nothing, as no path is that long
    const double cut = prm.sample_distance_m / c->res;
    const int64_t step = (cut < 2147483647.0 ? (int64_t)(int)cut : (int64_t)2147483647) + 1;
    const int64_t per_path = (int64_t)navfn_max_cycles(c) / step;       // a path has at most max_cycles points
    if ((int64_t)n * per_path > (int64_t)INT32_MAX) return fail(c, FS_E_INVALID, "%d paths of up to %lld way points: beyond 2^31", n, (long long)per_path);
    int64_t bound = (int64_t)n * per_path;
    const PlanOutLayout O(nn);
    const PathInfoOutLayout P(nn);
    // every buffer whose size is known before the plan is sized before a pointer into any of them is taken
    FS_HIP(c, c->h_nav_out.ensure(O.total));
    FS_HIP(c, c->d_pi_off.ensure(2 * (nn + 1)));
    FS_HIP(c, c->d_pi_out.ensure(P.total)); FS_HIP(c, c->h_pi_out.ensure(P.total));
    // (an error after the first launch waits for the stream: the next call may grow what the launches still use)
    const auto stop = [&](int code) { (void)hipStreamSynchronize(c->stream); return code; };
    rc = navfn_plan_enqueue(c, robot_pose7, allow_unknown, n, goal_xyz, achievable_in);
    if (rc) return stop(rc);
    FS_HIP(c, hipMemcpyAsync(c->h_nav_out.p, c->d_nav_out.p, O.total, hipMemcpyDeviceToHost, c->stream));
    FsPathInfoArgs a{};
    a.n = n; a.nx = c->nx; a.ny = c->ny; a.max_cycles = navfn_max_cycles(c);
    a.step = step; a.lookahead = prm.lookahead_points;
    a.ox = c->origin[0]; a.oy = c->origin[1]; a.res = c->res;
    a.path = c->d_nav_path.p;
    a.path_length = reinterpret_cast<const double *>(c->d_nav_out.p + O.len);
    a.achievable = reinterpret_cast<const uint8_t *>(c->d_nav_out.p + O.ach);
    a.dedup = c->opt_pi_dedup ? 1 : 0;
    a.fi_threshold = prm.fi_threshold;
    int64_t *hdr = reinterpret_cast<int64_t *>(c->h_pi_out.p + P.hdr);
    const auto bind = [&]() {      // (after the last growth of d_pi_temp)
        a.count = c->d_pi_off.p; a.offset = c->d_pi_off.p + nn + 1;
        a.hdr = reinterpret_cast<int64_t *>(c->d_pi_out.p + P.hdr);
        a.info_mean = reinterpret_cast<double *>(c->d_pi_out.p + P.mean);
        a.info_min = reinterpret_cast<float *>(c->d_pi_out.p + P.min);
        a.first_unsafe = reinterpret_cast<int32_t *>(c->d_pi_out.p + P.unsafe);
        a.temp = c->d_pi_temp.p; a.temp_bytes = c->d_pi_temp.cap;
    };
    const auto ensure_temp = [&](int64_t room) -> int {
        const size_t bytes = fs_pathinfo_temp_bytes(a, room, c->stream);
        if (bytes == 0) return fail(c, FS_E_HIP, "rocPRIM refused the size query");
        FS_HIP(c, c->d_pi_temp.ensure(bytes));
        return FS_OK;
    };
    const bool direct = bound <= PI_BOUND_DIRECT;
    rc = ensure_temp(direct ? bound : 0);
    if (rc) return stop(rc);
    bind();
    if (fs_launch_pathinfo_offsets(a, c->stream) != hipSuccess) return stop(fail(c, FS_E_HIP, "way-point offsets: launch failed"));
    if (!direct) {
        // a list whose paths could hold more way points than the call makes room for unseen (a sample distance of a few cells on a
        // large map): the total is read first, at the price of one more synchronisation
        FS_HIP(c, hipMemcpyAsync(hdr, a.offset + n, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        FS_HIP(c, hipStreamSynchronize(c->stream));
        int32_t total32 = 0;
        std::memcpy(&total32, hdr, sizeof total32);
        bound = total32;
        rc = ensure_temp(bound);
        if (rc) return stop(rc);
        bind();
    }
    if (bound > 0 && (rc = pathinfo_prepare(c, a, bound, dump, "way points", hdr, stop))) return rc;
    // THE mid-call synchronisation: the worker's item count (and the room its per-item scratch needs) must be on the host
    FS_HIP(c, hipStreamSynchronize(c->stream));
    const int64_t total = bound > 0 ? hdr[0] : 0, distinct = bound > 0 ? hdr[1] : 0;
    c->pi_waypoints = total; c->pi_distinct = distinct;
    if (dump) *n_total = total;
    if (dump && total > max_waypoints) return fail(c, FS_E_RANGE, "%lld way points, room for %lld", (long long)total, (long long)max_waypoints);
    if (distinct > 0 && (rc = pathinfo_score(c, a, distinct, stop))) return rc;
    if (fs_launch_pathinfo_finish(a, c->stream) != hipSuccess) return stop(fail(c, FS_E_HIP, "path information columns: launch failed"));
    FS_HIP(c, hipMemcpyAsync(c->h_pi_out.p + P.mean, c->d_pi_out.p + P.mean, P.total - P.mean, hipMemcpyDeviceToHost, c->stream));
    if (dump) {
        FS_HIP(c, hipMemcpyAsync(waypoint_offset, a.offset, sizeof(int32_t) * (nn + 1), hipMemcpyDeviceToHost, c->stream));
        if (total > 0) {
            FS_HIP(c, hipMemcpyAsync(waypoint_pose7, a.pose7, sizeof(double) * 7 * (size_t)total, hipMemcpyDeviceToHost, c->stream));
            FS_HIP(c, hipMemcpyAsync(waypoint_info, a.wp_info, sizeof(float) * (size_t)total, hipMemcpyDeviceToHost, c->stream));
        }
    }
    FS_HIP(c, hipMemcpyAsync(n_waypoints, a.count, sizeof(int32_t) * nn, hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipStreamSynchronize(c->stream));
    plan_columns_to_caller(c->h_nav_out, nn, path_length, path_length_m, path_heading, achievable);
    std::memcpy(info_mean, c->h_pi_out.p + P.mean, 8 * nn);
    std::memcpy(info_min, c->h_pi_out.p + P.min, 4 * nn);
    std::memcpy(first_unsafe, c->h_pi_out.p + P.unsafe, 4 * nn);
    return FS_OK;
}

int fs_get_frontier_costs_planned(fs_ctx *c, const double robot_pose7[7], int32_t allow_unknown, int32_t n, const double *goal_xyz,
                                  const int32_t *frontier_size, const uint8_t *blacklisted, double alpha, double beta, double max_vx, double max_wz,
                                  int with_fisher_information, fs_record *records, double *weighted_cost, double *arrival_utility,
                                  double *distance_utility, int32_t *order, double *path_length_m)
{
    if (!c) return FS_E_INVALID;
    if (n < 0 || (n > 0 && (!goal_xyz || !records || !weighted_cost))) return fail(c, FS_E_INVALID, "null pointer");
    int rc = nav_check(c, robot_pose7);
    if (rc) return rc;
    if (n == 0) return FS_OK;
    rc = check_scoring_state(c, true, with_fisher_information != 0);
    if (rc) return rc;
    return rank_on_plan(
        c, c->d_nav_out, c->h_nav_out, n, [&] { return navfn_plan_enqueue(c, robot_pose7, allow_unknown, n, goal_xyz, nullptr); },
        [&](const PlannedCols &cols) {
            return frontier_costs_core(c, n, goal_xyz, frontier_size, blacklisted, nullptr, nullptr, nullptr, alpha, beta, max_vx, max_wz,
                                       with_fisher_information != 0, records, weighted_cost, arrival_utility, distance_utility, order, &cols);
        },
        path_length_m);
}

int fs_get_frontier_costs_searched(fs_ctx *c, const double robot_pose7[7], int32_t lethal_threshold, double max_frontier_distance,
                                   int32_t min_frontier_cluster_size, int32_t max_frontier_cluster_size, int32_t allow_unknown,
                                   int32_t n_blacklist, const double *blacklist_xy, double alpha, double beta, double max_vx, double max_wz,
                                   int with_fisher_information, int32_t max_records, fs_frontier_record *frontiers, int32_t *n_frontiers,
                                   fs_record *records, double *weighted_cost, double *arrival_utility, double *distance_utility,
                                   int32_t *order, double *path_length_m)
{
    if (!c) return FS_E_INVALID;
    if (!robot_pose7 || !n_frontiers || max_records < 0 || (max_records > 0 && (!frontiers || !records || !weighted_cost)) ||
        n_blacklist < 0 || (n_blacklist > 0 && !blacklist_xy))
        return fail(c, FS_E_INVALID, "null pointer or negative count");
    *n_frontiers = 0;
    int rc = nav_check(c, robot_pose7);
    if (rc) return rc;
    rc = check_scoring_state(c, true, with_fisher_information != 0);
    if (rc) return rc;
    bool on_map = false;
    std::vector<fs_frontier_record> found;
    rc = searched_list(c, robot_pose7, lethal_threshold, max_frontier_distance, min_frontier_cluster_size, max_frontier_cluster_size,
                       n_blacklist, blacklist_xy, max_records, &on_map, n_frontiers, found);
    if (rc) return rc;
    const int32_t n = *n_frontiers;
    if (n == 0) return FS_OK;                   // (a robot off the map among them)
    // setPlanForFrontier's heading is the host's libm by the planner's definition: computed from the records the
    // caller receives, the only column that goes up
    std::vector<double> heading((size_t)n);
    for (int32_t k = 0; k < n; ++k) heading[k] = nav_heading(robot_pose7, found[k].goal_x, found[k].goal_y);
    rc = rank_on_plan(
        c, c->d_nav_out, c->h_nav_out, n, [&] { return navfn_plan_enqueue_dev(c, robot_pose7, allow_unknown, n, c->d_fs_goal.p, heading.data()); },
        [&](const PlannedCols &cols) {
            const DevCols dev{c->d_fs_goal.p, c->d_fs_fsize.p, c->d_fs_black.p};
            return frontier_costs_core(c, n, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, alpha, beta, max_vx, max_wz,
                                       with_fisher_information != 0, records, weighted_cost, arrival_utility, distance_utility, order, &cols, &dev);
        },
        path_length_m);
    if (rc) return rc;
    std::memcpy(frontiers, found.data(), sizeof(fs_frontier_record) * (size_t)n);
    return FS_OK;
}

}  // extern "C"

// ================================================================== frontier roadmap (fs_roadmap.hip)
// FrontierRoadMap's node and edge bookkeeping (populateNodes, constructNewEdges) stays on the host, where its order-dependent
// insertions are cheap; every isConnectable of a call is walked on the device in one batch, the whole-graph rebuild and the
// planner run there.

namespace {

#define RM_MAX_PER_CELL 20          // populateNodes throws once a cell holds more (FrontierRoadmap.cpp:244-248)

int32_t rm_nodes(const fs_ctx *c) { return (int32_t)(c->rm_xy.size() / 2); }

// getNodesWithinRadius(node p, radius_to_decide_edges) in the reference's order (p itself included: callers skip it)
void rm_within_radius(const fs_ctx *c, int32_t p, std::vector<int32_t> &out)
{
    out.clear();
    const double px = c->rm_xy[2 * (size_t)p], py = c->rm_xy[2 * (size_t)p + 1];
    const int cx = fs_rm_cell(px, c->rm_cell), cy = fs_rm_cell(py, c->rm_cell);
    const int cr = (int)std::ceil(c->rm_radius / c->rm_cell);
    for (int dx = -cr; dx <= cr; ++dx)
        for (int dy = -cr; dy <= cr; ++dy) {
            const auto it = c->rm_hash.find({cx + dx, cy + dy});
            if (it == c->rm_hash.end()) continue;
            for (const int32_t q : it->second) {
                const double ex = px - c->rm_xy[2 * (size_t)q], ey = py - c->rm_xy[2 * (size_t)q + 1];
                if (std::sqrt(ex * ex + ey * ey) < c->rm_radius) out.push_back(q);
            }
        }
}

// isConnectable (FrontierRoadmap.cpp:716-737): visitor (253, 254, 0, 255), max_length = (unsigned)(max_connection_length / res)
// handed on as a double, max_connection_length = 1.5 * radius (:20); rejected above radius / res * 0.3 unknown cells
FsSegArgs rm_seg_args(fs_ctx *c, int32_t n)
{
    FsSegArgs a{};
    a.grid = grid_dev(c);
    a.n = n; a.start = c->d_seg_start.p; a.end = c->d_seg_end.p;
    a.max_length = (double)(unsigned)(c->rm_radius * 1.5 / c->res);
    a.obst_min = 253; a.obst_max = 254; a.trace_min = 0; a.trace_max = 255;
    a.ok = c->d_seg_ok.p; a.hit = c->d_seg_hit.p; a.traced = c->d_seg_traced.p; a.unknown = c->d_seg_unknown.p; a.all = c->d_seg_all.p;
    return a;
}
double rm_unknown_limit(const fs_ctx *c) { return c->rm_radius / c->res * 0.3; }

int rm_seg_ensure(fs_ctx *c, size_t n)
{
    FS_HIP(c, c->d_seg_start.ensure(3 * n)); FS_HIP(c, c->d_seg_end.ensure(3 * n));
    FS_HIP(c, c->d_seg_ok.ensure(n)); FS_HIP(c, c->d_seg_hit.ensure(n));
    FS_HIP(c, c->d_seg_traced.ensure(n)); FS_HIP(c, c->d_seg_unknown.ensure(n)); FS_HIP(c, c->d_seg_all.ensure(n));
    return FS_OK;
}

// node positions and the spatial hash (occupied cells in ascending key order) on the device; synchronised by the caller before
// the host vectors go out of scope
int rm_upload_nodes(fs_ctx *c, FsRoadmapDev &g, std::vector<uint64_t> &keys, std::vector<int32_t> &start, std::vector<int32_t> &nodes)
{
    const int32_t n = rm_nodes(c);
    std::vector<std::pair<uint64_t, const std::vector<int32_t> *>> cells;
    for (const auto &kv : c->rm_hash)
        if (!kv.second.empty()) cells.push_back({((uint64_t)(uint32_t)kv.first.first << 32) | (uint32_t)kv.first.second, &kv.second});
    std::sort(cells.begin(), cells.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
    keys.clear(); start.assign(1, 0); nodes.clear();
    for (const auto &e : cells) {
        keys.push_back(e.first);
        nodes.insert(nodes.end(), e.second->begin(), e.second->end());
        start.push_back((int32_t)nodes.size());
    }
    FS_HIP(c, c->d_rm_xy.ensure(2 * (size_t)n)); FS_HIP(c, c->d_rm_cell_key.ensure(keys.size()));
    FS_HIP(c, c->d_rm_cell_start.ensure(start.size())); FS_HIP(c, c->d_rm_cell_nodes.ensure(nodes.size()));
    FS_HIP(c, hipMemcpyAsync(c->d_rm_xy.p, c->rm_xy.data(), sizeof(double) * 2 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    FS_HIP(c, hipMemcpyAsync(c->d_rm_cell_key.p, keys.data(), sizeof(uint64_t) * keys.size(), hipMemcpyHostToDevice, c->stream));
    FS_HIP(c, hipMemcpyAsync(c->d_rm_cell_start.p, start.data(), sizeof(int32_t) * start.size(), hipMemcpyHostToDevice, c->stream));
    FS_HIP(c, hipMemcpyAsync(c->d_rm_cell_nodes.p, nodes.data(), sizeof(int32_t) * nodes.size(), hipMemcpyHostToDevice, c->stream));
    g = FsRoadmapDev{n, c->d_rm_xy.p, c->rm_cell, c->rm_radius, (int32_t)keys.size(), c->d_rm_cell_key.p, c->d_rm_cell_start.p,
                     c->d_rm_cell_nodes.p};
    return FS_OK;
}

// the device's nodes, key flags and CSR for the current generation (uploaded from the host lists after a host-side mutation) ...
int rm_device_csr(fs_ctx *c)
{
    const int32_t n = rm_nodes(c);
    if (c->rm_dev_gen != c->rm_gen) {
        std::vector<int32_t> row(1, 0), col;
        for (const auto &l : c->rm_adj) { col.insert(col.end(), l.begin(), l.end()); row.push_back((int32_t)col.size()); }
        FS_HIP(c, c->d_rm_xy.ensure(2 * (size_t)n)); FS_HIP(c, c->d_rm_key.ensure(n));
        FS_HIP(c, c->d_rm_row.ensure(row.size())); FS_HIP(c, c->d_rm_col.ensure(col.size()));
        FS_HIP(c, hipMemcpyAsync(c->d_rm_xy.p, c->rm_xy.data(), sizeof(double) * 2 * (size_t)n, hipMemcpyHostToDevice, c->stream));
        FS_HIP(c, hipMemcpyAsync(c->d_rm_key.p, c->rm_key.data(), (size_t)n, hipMemcpyHostToDevice, c->stream));
        FS_HIP(c, hipMemcpyAsync(c->d_rm_row.p, row.data(), sizeof(int32_t) * row.size(), hipMemcpyHostToDevice, c->stream));
        FS_HIP(c, hipMemcpyAsync(c->d_rm_col.p, col.data(), sizeof(int32_t) * col.size(), hipMemcpyHostToDevice, c->stream));
        FS_HIP(c, hipStreamSynchronize(c->stream));
        c->rm_dev_gen = c->rm_gen;
    }
    return FS_OK;
}

// ... then its transpose
int rm_device_graph(fs_ctx *c)
{
    const int32_t n = rm_nodes(c);
    const int rc = rm_device_csr(c);
    if (rc) return rc;
    if (c->rm_t_gen != c->rm_gen) {
        size_t e = 0;
        for (const auto &l : c->rm_adj) e += l.size();
        FS_HIP(c, c->d_rm_tmp.ensure(2 * (size_t)n + 1)); FS_HIP(c, c->d_rm_trow.ensure((size_t)n + 1)); FS_HIP(c, c->d_rm_tcol.ensure(e));
        int32_t *indeg = c->d_rm_tmp.p, *cursor = c->d_rm_tmp.p + n;
        FS_HIP(c, hipMemsetAsync(c->d_rm_tmp.p, 0, sizeof(int32_t) * 2 * (size_t)n, c->stream));
        FS_HIP(c, fs_launch_rm_transpose(n, c->d_rm_row.p, c->d_rm_col.p, indeg, nullptr, nullptr, nullptr, c->stream, 0));
        FS_HIP(c, fs_launch_rm_scan(indeg, n, c->d_rm_trow.p, c->stream));
        FS_HIP(c, fs_launch_rm_transpose(n, c->d_rm_row.p, c->d_rm_col.p, nullptr, c->d_rm_trow.p, cursor, c->d_rm_tcol.p, c->stream, 1));
        c->rm_t_gen = c->rm_gen;
    }
    return FS_OK;
}

// The shortest-path tree from `root` for the current generation: the cached one, or built now (synchronises the stream).
int rm_tree(fs_ctx *c, int32_t root, const double **d, const int32_t **pred)
{
    const int32_t n = rm_nodes(c);
    const size_t nn = (size_t)n;
    if (!(c->rm_tree_gen == c->rm_gen && c->rm_tree_root == root)) {
        c->rm_tree_gen = 0;
        int rc = rm_device_graph(c);
        if (rc) return rc;
        FS_HIP(c, c->d_rm_d.ensure(2 * nn)); FS_HIP(c, c->d_rm_hops.ensure(2 * nn)); FS_HIP(c, c->d_rm_pred.ensure(2 * nn));
        FS_HIP(c, c->d_rm_word.ensure(PLAN_BATCH));
        FsRmTree t{n, root, c->d_rm_xy.p, c->d_rm_trow.p, c->d_rm_tcol.p, {c->d_rm_d.p, c->d_rm_d.p + nn}, {c->d_rm_hops.p, c->d_rm_hops.p + nn},
                   {c->d_rm_pred.p, c->d_rm_pred.p + nn}};
        FS_HIP(c, fs_launch_rm_tree_init(t, c->stream));
        // d settles within n - 1 rounds (a minimum over walks is reached on a simple path), hops / predecessor within n more
        const int64_t max_rounds = 2 * (int64_t)n + 2;
        int64_t rounds = 0;
        if (n <= RM_TREE_ONE_WG) {
            FS_HIP(c, fs_launch_rm_tree_block(t, (int32_t)max_rounds, c->d_rm_word.p, c->stream));
            int32_t r = 0;
            FS_HIP(c, hipMemcpyAsync(&r, c->d_rm_word.p, sizeof r, hipMemcpyDeviceToHost, c->stream));
            FS_HIP(c, hipStreamSynchronize(c->stream));
            if (r < 0) return fail(c, FS_E_HIP, "the roadmap tree did not settle in %lld rounds", (long long)max_rounds);
            rounds = r;
        } else {
            const auto launch = [&](int64_t r0, int count) -> int {
                for (int k = 0; k < count; ++k) FS_HIP(c, fs_launch_rm_tree_round(t, (int32_t)((r0 + k) & 1), c->d_rm_word.p + k, c->stream));
                return FS_OK;
            };
            rc = poll_rounds(c, c->d_rm_word.p, PLAN_BATCH, PLAN_BATCH, 1, max_rounds, "the roadmap tree", max_rounds, launch, &rounds);
            if (rc) return rc;
        }
        c->rm_tree_buf = (int32_t)(rounds & 1);        // (after the quiet round both buffers hold the tree)
        c->rm_tree_gen = c->rm_gen; c->rm_tree_root = root;
        c->rm_tree_rounds = rounds;
        ++c->rm_tree_builds;
    }
    *d = c->d_rm_d.p + (size_t)c->rm_tree_buf * nn;
    *pred = c->d_rm_pred.p + (size_t)c->rm_tree_buf * nn;
    return FS_OK;
}

// ---- the REFERENCE search (fs_set_roadmap_search): one A* per distinct (start, goal) pair, one wave per query

// records of a query in LDS for a roadmap of n nodes: the option, capped by what fits beside the per-node state (0: global route only)
int32_t rm_astar_lds_cap(const fs_ctx *c, int32_t n)
{
    const int64_t fit = ((int64_t)RM_ASTAR_LDS_BYTES - 5 * (int64_t)n - 16) / 28;
    const int64_t cap = std::min<int64_t>(c->astar_lds_entries, fit);
    return cap >= 16 ? (int32_t)cap : 0;
}

// The query launches on `a` (n_nodes, the graph, the query list, nq and the LDS cap filled in by the caller): the global route's
// pool sized, the stats cleared, the LDS route then the global route, the stats copied to h_as_io.  Nothing synchronises.
int rm_astar_enqueue(fs_ctx *c, FsRmAstarArgs &a, int32_t max_q)
{
    const size_t slot = fs_rm_astar_bytes(c->astar_cap, a.n_nodes);
    FS_HIP(c, c->d_as_pool.ensure(slot * RM_ASTAR_SLOTS)); FS_HIP(c, c->d_as_stats.ensure(8)); FS_HIP(c, c->h_as_io.ensure(64));
    a.pool = c->d_as_pool.p; a.slot_bytes = slot; a.slots = RM_ASTAR_SLOTS; a.cap = c->astar_cap;
    a.stats = c->d_as_stats.p;
    FS_HIP(c, hipMemsetAsync(c->d_as_stats.p, 0, 8 * sizeof(int32_t), c->stream));
    FS_HIP(c, fs_launch_rm_astar(a, max_q, c->stream));
    FS_HIP(c, hipMemcpyAsync(c->h_as_io.p, c->d_as_stats.p, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    c->as_args = a;
    return FS_OK;
}

// After the caller's synchronisation: the counters from the stats; queries that outgrew the global route's pool run again on a
// pool four times larger, each round followed by `redo()` (the launches that read the query results) and a synchronisation.
// *redone: whether that happened.
template <class Redo>
int rm_astar_settle(fs_ctx *c, Redo redo, bool *redone)
{
    int32_t st[4];
    std::memcpy(st, c->h_as_io.p, sizeof st);
    c->as_queries += st[0]; c->as_global += st[2];
    int64_t pops = st[1];
    *redone = false;
    while (st[3] > 0) {
        if (c->astar_cap > (1 << 28) / 4) return fail(c, FS_E_HIP, "an A* query outgrew %d records", c->astar_cap);
        c->astar_cap *= 4;
        FsRmAstarArgs &a = c->as_args;
        const size_t slot = fs_rm_astar_bytes(c->astar_cap, a.n_nodes);
        FS_HIP(c, c->d_as_pool.ensure(slot * RM_ASTAR_SLOTS));
        a.pool = c->d_as_pool.p; a.slot_bytes = slot; a.cap = c->astar_cap;
        FS_HIP(c, hipMemsetAsync(c->d_as_stats.p, 0, 8 * sizeof(int32_t), c->stream));
        FS_HIP(c, fs_launch_rm_astar_global(a, c->stream));
        const int rc = redo();
        if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
        FS_HIP(c, hipMemcpyAsync(c->h_as_io.p, c->d_as_stats.p, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        FS_HIP(c, hipStreamSynchronize(c->stream));
        std::memcpy(st, c->h_as_io.p, sizeof st);
        pops = std::max<int64_t>(pops, st[1]);
        *redone = true;
    }
    c->as_max_pops = pops;
    return FS_OK;
}

// roadmap_plan_enqueue's REFERENCE form: the goal nodes marked and scanned into distinct queries from the start node, the queries,
// then the columns from their results.  The tree and its cache are not touched.
int roadmap_astar_enqueue(fs_ctx *c, FsRmPlanArgs &a)
{
    const int32_t nodes = a.n_nodes;
    FsRmAstarArgs q{};
    q.n_nodes = nodes; q.root = a.root;
    const size_t nn = (size_t)nodes;
    FS_HIP(c, c->d_as_gnode.ensure((size_t)a.n)); FS_HIP(c, c->d_as_mark.ensure(nn)); FS_HIP(c, c->d_as_qidx.ensure(nn + 1));
    const int32_t max_q = a.root >= 0 ? std::min(a.n, nodes) : 0;
    FS_HIP(c, c->d_as_dst.ensure((size_t)std::max(max_q, 1))); FS_HIP(c, c->d_as_status.ensure((size_t)std::max(max_q, 1)));
    FS_HIP(c, c->d_as_len.ensure((size_t)std::max(max_q, 1)));
    if (max_q > 0) {
        const int rc = rm_device_graph(c);
        if (rc) return rc;
        a.xy = c->d_rm_xy.p; a.key = c->d_rm_key.p;
        FS_HIP(c, hipMemsetAsync(c->d_as_mark.p, 0, sizeof(int32_t) * nn, c->stream));
    }
    FS_HIP(c, fs_launch_rm_astar_goals(a, c->d_as_gnode.p, c->d_as_mark.p, c->stream));
    if (max_q > 0) {
        FS_HIP(c, fs_launch_rm_scan(c->d_as_mark.p, nodes, c->d_as_qidx.p, c->stream));
        FS_HIP(c, fs_launch_rm_astar_list(nodes, c->d_as_mark.p, c->d_as_qidx.p, c->d_as_dst.p, c->stream));
        q.xy = c->d_rm_xy.p; q.row = c->d_rm_row.p; q.col = c->d_rm_col.p;
    } else {
        FS_HIP(c, hipMemsetAsync(c->d_as_qidx.p, 0, sizeof(int32_t) * (nn + 1), c->stream));
    }
    q.nq = c->d_as_qidx.p + nodes; q.dst = c->d_as_dst.p; q.status = c->d_as_status.p; q.len = c->d_as_len.p;
    q.lds_cap = rm_astar_lds_cap(c, nodes);
    if (c->rt_chains) {
        const size_t mq = (size_t)std::max(max_q, 1);
        FS_HIP(c, c->d_rt_chain_len.ensure(mq)); FS_HIP(c, c->d_rt_chain_base.ensure(mq));
        FS_HIP(c, c->d_rt_pool.ensure((size_t)c->rt_pool_cap)); FS_HIP(c, c->d_rt_cursor.ensure(2));
        FS_HIP(c, hipMemsetAsync(c->d_rt_cursor.p, 0, sizeof(unsigned long long), c->stream));
        q.chain_len = c->d_rt_chain_len.p; q.chain_base = c->d_rt_chain_base.p; q.chain_pool = c->d_rt_pool.p;
        q.chain_cap = c->rt_pool_cap; q.chain_cursor = c->d_rt_cursor.p;
        c->rt_max_q = max_q;
    }
    int rc = rm_astar_enqueue(c, q, max_q);
    if (rc) return rc;
    c->as_plan = a;
    FS_HIP(c, fs_launch_rm_astar_cols(a, c->d_as_gnode.p, c->d_as_qidx.p, c->d_as_status.p, c->d_as_len.p, c->stream));
    return FS_OK;
}

// the columns again from the settled query results (rm_astar_settle's redo for the plan)
int roadmap_astar_cols(fs_ctx *c)
{
    FS_HIP(c, fs_launch_rm_astar_cols(c->as_plan, c->d_as_gnode.p, c->d_as_qidx.p, c->d_as_status.p, c->d_as_len.p, c->stream));
    return FS_OK;
}

// The per-goal staging of a roadmap plan for one robot pose: the xy copy of the goals, getPlan's mode (0 not planned, 1 the robot
// stands on the goal, 2 searched) and setPlanForFrontier's heading.  Returns whether any goal is searched (the plan needs a tree).
bool rm_stage_goals(const double robot7[7], size_t n, const double *goal_xyz, const uint8_t *achievable_in, double *goal, uint8_t *mode,
                    double *head)
{
    bool need_tree = false;
    for (size_t i = 0; i < n; ++i) {
        const double gx = goal_xyz[3 * i], gy = goal_xyz[3 * i + 1];
        goal[2 * i] = gx; goal[2 * i + 1] = gy;
        // getPlan's early return (FrontierRoadmap.cpp:548-554) comes before any search
        mode[i] = (achievable_in && !achievable_in[i]) ? 0 : (robot7[0] == gx && robot7[1] == gy) ? 1 : 2;
        head[i] = mode[i] ? nav_heading(robot7, gx, gy) : 0.0;
        need_tree |= mode[i] == 2;
    }
    return need_tree;
}

// Start node, tree (cached or built), goals staged, the plan kernel: the four columns land in d_rm_out on the context's stream.
// REFERENCE search: the A* queries instead of the tree (their stats in h_as_io: rm_astar_settle after the synchronisation).
int roadmap_plan_enqueue(fs_ctx *c, const double robot7[7], int32_t n, const double *goal_xyz, const uint8_t *achievable_in)
{
    const size_t nn = (size_t)n;
    const size_t i_goal = 0, i_head = 16 * nn, i_mode = 24 * nn, total_in = 24 * nn + nn;
    const PlanOutLayout O(nn);
    FS_HIP(c, c->h_rm_in.ensure(total_in)); FS_HIP(c, c->d_rm_in.ensure(total_in));
    FS_HIP(c, c->d_rm_out.ensure(O.total));
    double *goal = reinterpret_cast<double *>(c->h_rm_in.p + i_goal), *head = reinterpret_cast<double *>(c->h_rm_in.p + i_head);
    uint8_t *mode = reinterpret_cast<uint8_t *>(c->h_rm_in.p + i_mode);
    const bool need_tree = rm_stage_goals(robot7, nn, goal_xyz, achievable_in, goal, mode, head);
    const int32_t nodes = rm_nodes(c);
    const int32_t root = fs_rm_closest(c->rm_xy.data(), c->rm_key.data(), nodes, c->rm_cell, robot7[0], robot7[1]);
    const bool reference = c->rm_search == FS_ROADMAP_SEARCH_REFERENCE;
    const double *d = nullptr;
    const int32_t *pred = nullptr;
    if (!reference && need_tree && root >= 0) { const int rc = rm_tree(c, root, &d, &pred); if (rc) return rc; }
    FS_HIP(c, hipMemcpyAsync(c->d_rm_in.p, c->h_rm_in.p, total_in, hipMemcpyHostToDevice, c->stream));
    FsRmPlanArgs a{};
    a.n_nodes = nodes; a.xy = c->d_rm_xy.p; a.key = c->d_rm_key.p; a.cell = c->rm_cell;
    a.d = d; a.pred = pred; a.root = root;
    a.n = n;
    a.goal = reinterpret_cast<const double *>(c->d_rm_in.p + i_goal);
    a.heading_in = reinterpret_cast<const double *>(c->d_rm_in.p + i_head);
    a.mode = reinterpret_cast<const uint8_t *>(c->d_rm_in.p + i_mode);
    a.path_length = reinterpret_cast<double *>(c->d_rm_out.p + O.len);
    a.path_length_m = reinterpret_cast<double *>(c->d_rm_out.p + O.len_m);
    a.path_heading = reinterpret_cast<double *>(c->d_rm_out.p + O.head);
    a.achievable = reinterpret_cast<uint8_t *>(c->d_rm_out.p + O.ach);
    if (reference) {
        if (!need_tree) a.root = -1;                    // (no goal is searched)
        c->rt_plan = a;
        return roadmap_astar_enqueue(c, a);
    }
    c->rt_plan = a;
    FS_HIP(c, fs_launch_rm_plan(a, c->stream));
    return FS_OK;
}

bool rm_finite_xy(const double *xy, int32_t n, int stride)
{
    for (int32_t i = 0; i < n; ++i)
        if (!std::isfinite(xy[(size_t)stride * i]) || !std::isfinite(xy[(size_t)stride * i + 1])) return false;
    return true;
}

// the record store grows without losing what it holds (DevBuf::ensure does not keep contents)
template <class T>
int kf_grow(fs_ctx *c, DevBuf<T> &b, size_t used, size_t need)
{
    if (need <= b.cap) return FS_OK;
    DevBuf<T> nb;
    FS_HIP(c, nb.ensure(std::max(need, 2 * b.cap)));
    if (used) FS_HIP(c, hipMemcpyAsync(nb.p, b.p, sizeof(T) * used, hipMemcpyDeviceToDevice, c->stream));
    FS_HIP(c, hipStreamSynchronize(c->stream));
    b = std::move(nb);
    return FS_OK;
}

// base[h] of every handle in keyframe_mapping_'s iteration order: the prefix of the record counts of the handles before it (only
// the key frames of the latest message when `present_only`, the others -1).  Returns the total.
int64_t kf_bases(const fs_ctx *c, bool present_only, std::vector<int32_t> &base)
{
    base.assign(c->kf_handle_id.size(), -1);
    int64_t m = 0;
    for (const auto &kv : c->kf_order) {
        const int32_t h = kv.second;
        if (present_only && c->kf_slot[(size_t)h] < 0) continue;
        base[(size_t)h] = (int32_t)m;
        m += c->kf_handle_count[(size_t)h];
    }
    return m;
}

// the de-duplication rounds (fs_roadmap_kf.hip): one workgroup's loop up to kf_one_wg points, a round per launch above it, polled in
// batches of PLAN_BATCH.  Returns the rounds run (the last one quiet) through *rounds.
int kf_dedup_rounds(fs_ctx *c, const FsKfDedup &d, int64_t *rounds)
{
    const int64_t max_rounds = (int64_t)d.m + 1;
    if (d.m <= c->kf_one_wg) {
        FS_HIP(c, fs_launch_kf_dedup_block(d, (int32_t)max_rounds, c->stream));
        *rounds = -2;                   // read from hdr[2] with the results
        return FS_OK;
    }
    FS_HIP(c, c->d_kf_word.ensure(PLAN_BATCH));
    const auto launch = [&](int64_t r0, int count) -> int {
        for (int k = 0; k < count; ++k) FS_HIP(c, fs_launch_kf_dedup_round(d, (int)((r0 + k) & 1), c->d_kf_word.p + k, c->stream));
        return FS_OK;
    };
    // (fails once more than m + 1 rounds have run)
    return poll_rounds(c, c->d_kf_word.p, PLAN_BATCH, PLAN_BATCH, 1, max_rounds + 1, "the de-duplication", max_rounds, launch, rounds);
}

// UpdateRoadmapBT: the list at d_pts (device memory, point i at d_pts[stride * i]) and the robot pose, decided on
// the device by fs_roadmap_update.hip and applied to the host mirror.  Two synchronisations: the sizes (header, candidate total),
// then the result.  The caller has checked the grid and the input.
struct RmUpdateOut {
    int32_t kept = 0, robot = 0;
    int64_t edges = 0;
};

int rm_update_core(fs_ctx *c, int32_t n, const double *d_pts, int32_t stride, const double robot_xy[2], bool add_robot, RmUpdateOut *out)
{
    const int32_t n_old = rm_nodes(c);
    if (n > FS_RU_MAX_POINTS) return fail(c, FS_E_INVALID, "more than %d points in one roadmap update", FS_RU_MAX_POINTS);
    if (n_old == 0 && n == 0 && !add_robot) return FS_OK;
    if ((int64_t)n_old + n + 1 > (int64_t)INT32_MAX / 4) return fail(c, FS_E_RANGE, "too many roadmap nodes");
    int rc = n_old > 0 ? rm_device_csr(c) : FS_OK;     // the nodes, key flags and lists of this generation (kept from the last plan)
    if (rc) return rc;
    const size_t nn = (size_t)n, m = nn + 1, cap = (size_t)n_old + m;
    const int32_t words = (n + 63) / 64;
    FS_HIP(c, c->d_ru_xy.ensure(2 * cap)); FS_HIP(c, c->d_ru_key.ensure(cap)); FS_HIP(c, c->d_ru_rank_of.ensure(cap));
    FS_HIP(c, c->d_ru_rejected.ensure(nn)); FS_HIP(c, c->d_ru_conf.ensure(nn * (size_t)words));
    // ints: occupants [n] | closest [m] | owner [m] | cand_count [m] | cand_off [m + 1] | hdr
    const size_t o_closest = nn, o_owner = o_closest + m, o_count = o_owner + m, o_off = o_count + m, o_hdr = o_off + m + 1;
    FS_HIP(c, c->d_ru_work.ensure(o_hdr + FS_RU_H_WORDS));
    int32_t *w = c->d_ru_work.p;
    if (n_old > 0) {
        FS_HIP(c, hipMemcpyAsync(c->d_ru_xy.p, c->d_rm_xy.p, sizeof(double) * 2 * (size_t)n_old, hipMemcpyDeviceToDevice, c->stream));
        FS_HIP(c, hipMemcpyAsync(c->d_ru_key.p, c->d_rm_key.p, (size_t)n_old, hipMemcpyDeviceToDevice, c->stream));
    }
    FS_HIP(c, hipMemsetAsync(c->d_ru_rank_of.p, 0x7f, sizeof(int32_t) * cap, c->stream));
    FsRmUpdate u{};
    u.n = n; u.pts = d_pts; u.stride = stride; u.rx = robot_xy[0]; u.ry = robot_xy[1]; u.add_robot = add_robot ? 1 : 0;
    u.n_old = n_old; u.xy = c->d_ru_xy.p; u.key = c->d_ru_key.p; u.row = c->d_rm_row.p; u.col = c->d_rm_col.p;
    u.cell = c->rm_cell; u.radius = c->rm_radius; u.min_frontier = c->rm_min_frontier; u.min_robot = c->rm_min_robot; u.oz = c->origin[2];
    u.words = words; u.conf = c->d_ru_conf.p; u.rejected = c->d_ru_rejected.p; u.occupants = w; u.hdr = w + o_hdr;
    u.closest = w + o_closest; u.rank_of = c->d_ru_rank_of.p; u.owner = w + o_owner; u.cand_count = w + o_count; u.cand_off = w + o_off;
    FS_HIP(c, fs_launch_ru_nodes(u, c->stream));
    FS_HIP(c, fs_launch_ru_owners(u, c->stream));
    // the sizes: the candidate total (cand_off's last entry) and the header behind it
    const size_t head_ints = 1 + FS_RU_H_WORDS;
    FS_HIP(c, c->h_ru.ensure(sizeof(int32_t) * head_ints));
    FS_HIP(c, hipMemcpyAsync(c->h_ru.p, w + o_off + m, sizeof(int32_t) * head_ints, hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipStreamSynchronize(c->stream));
    int32_t head[1 + FS_RU_H_WORDS];
    std::memcpy(head, c->h_ru.p, sizeof head);
    const int32_t total = head[0], *hdr = head + 1;
    const int32_t kept = hdr[FS_RU_H_KEPT], robot = hdr[FS_RU_H_ROBOT], tripped = hdr[FS_RU_H_TRIPPED], nodes = hdr[FS_RU_H_NODES];
    if (hdr[FS_RU_H_ROUNDS] < 0) return fail(c, FS_E_HIP, "roadmap update: the keep rule did not settle in %d rounds", (int)n + 1);
    if (kept < 0 || kept > n || robot < 0 || robot > 1 || nodes != n_old + kept + robot || total < 0 || (tripped && total != 0))
        return fail(c, FS_E_HIP, "roadmap update: inconsistent header (%d kept of %d, %d candidates)", (int)kept, (int)n, (int)total);
    const size_t added = (size_t)(kept + robot), tt = (size_t)total;
    // the result: kept positions | pairs | inserted count | key flags
    const size_t r_xy = 0, r_pairs = r_xy + 16 * added, r_ins = r_pairs + 8 * tt, r_key = r_ins + 8, r_total = r_key + (size_t)nodes;
    FS_HIP(c, c->h_ru.ensure(r_total));
    if (!tripped && total > 0) {
        rc = rm_seg_ensure(c, tt);
        if (rc) return rc;
        // ints: tmp_q | tmp_order | cand | cand_rank | flag [total] | flag_off [total + 1] | pairs [total][2]
        FS_HIP(c, c->d_ru_cand.ensure(8 * tt + 1));
        int32_t *k = c->d_ru_cand.p;
        u.tmp_q = k; u.tmp_order = k + tt; u.cand = k + 2 * tt; u.cand_rank = k + 3 * tt; u.flag = k + 4 * tt; u.flag_off = k + 5 * tt;
        u.pairs = k + 6 * tt + 1;
        u.seg_start = c->d_seg_start.p; u.seg_end = c->d_seg_end.p;
        u.seg_ok = c->d_seg_ok.p; u.seg_hit = c->d_seg_hit.p; u.seg_unknown = c->d_seg_unknown.p; u.unknown_limit = rm_unknown_limit(c);
        FS_HIP(c, fs_launch_ru_candidates(u, total, c->stream));
        FS_HIP(c, fs_launch_segments(rm_seg_args(c, total), c->stream));
        FS_HIP(c, fs_launch_ru_insert(u, total, c->stream));
        FS_HIP(c, hipMemcpyAsync(c->h_ru.p + r_pairs, u.pairs, 8 * tt, hipMemcpyDeviceToHost, c->stream));
    }
    FS_HIP(c, hipMemcpyAsync(c->h_ru.p + r_ins, u.hdr + FS_RU_H_INSERTED, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (added) FS_HIP(c, hipMemcpyAsync(c->h_ru.p + r_xy, u.xy + 2 * (size_t)n_old, 16 * added, hipMemcpyDeviceToHost, c->stream));
    if (!tripped && nodes > 0) FS_HIP(c, hipMemcpyAsync(c->h_ru.p + r_key, u.key, (size_t)nodes, hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipStreamSynchronize(c->stream));
    int32_t inserted = 0;
    std::memcpy(&inserted, c->h_ru.p + r_ins, sizeof inserted);
    const int32_t *pairs = reinterpret_cast<const int32_t *>(c->h_ru.p + r_pairs);
    if (inserted < 0 || inserted > total) return fail(c, FS_E_HIP, "roadmap update: %d pairs of %d candidates", (int)inserted, (int)total);
    for (int32_t e = 0; e < 2 * inserted; ++e)
        if (pairs[e] < 0 || pairs[e] >= nodes) return fail(c, FS_E_HIP, "roadmap update: a pair names node %d of %d", (int)pairs[e], (int)nodes);
    // the mirror: the kept nodes as populateNodes appends them, the key flags, the pairs as constructNewEdges pushes them
    ++c->rm_gen;
    const double *axy = reinterpret_cast<const double *>(c->h_ru.p + r_xy);
    int cx = 0, cy = 0;
    for (size_t k = 0; k < added; ++k) {
        const double x = axy[2 * k], y = axy[2 * k + 1];
        cx = fs_rm_cell(x, c->rm_cell); cy = fs_rm_cell(y, c->rm_cell);
        c->rm_hash[{cx, cy}].push_back(rm_nodes(c));
        c->rm_xy.push_back(x); c->rm_xy.push_back(y);
        c->rm_key.push_back(0);
        c->rm_adj.emplace_back();
        c->kf_queue.push_back(x); c->kf_queue.push_back(y);
    }
    out->kept = kept; out->robot = robot;
    c->ru_walks = total; c->ru_owners = hdr[FS_RU_H_OWNERS]; c->ru_rounds = hdr[FS_RU_H_ROUNDS];
    if (tripped)
        return fail(c, FS_E_RANGE, "hash cell (%d, %d) holds more than %d nodes (the reference throws; the node stays added, the rest of the "
                    "update is not run)", cx, cy, RM_MAX_PER_CELL);
    if (nodes > 0) std::memcpy(c->rm_key.data(), c->h_ru.p + r_key, (size_t)nodes);
    for (int32_t e = 0; e < inserted; ++e) {
        const int32_t p = pairs[2 * e], q = pairs[2 * e + 1];
        c->rm_adj[(size_t)p].push_back(q); c->rm_adj[(size_t)q].push_back(p);
    }
    out->edges = inserted;
    c->rm_traced += total;
    return FS_OK;
}

}  // namespace

extern "C" {

int fs_set_roadmap_params(fs_ctx *c, double grid_cell_size, double radius_to_decide_edges, double min_distance_between_two_frontier_nodes,
                          double min_distance_between_robot_pose_and_node)
{
    if (!c) return FS_E_INVALID;
    if (!(grid_cell_size > 0 && std::isfinite(grid_cell_size)) || !(radius_to_decide_edges > 0 && std::isfinite(radius_to_decide_edges)) ||
        !(min_distance_between_two_frontier_nodes >= 0 && std::isfinite(min_distance_between_two_frontier_nodes)) ||
        !(min_distance_between_robot_pose_and_node >= 0 && std::isfinite(min_distance_between_robot_pose_and_node)))
        return fail(c, FS_E_INVALID, "roadmap parameters: cell and radius > 0, distances >= 0, all finite");
    c->rm_cell = grid_cell_size; c->rm_radius = radius_to_decide_edges;
    c->rm_min_frontier = min_distance_between_two_frontier_nodes; c->rm_min_robot = min_distance_between_robot_pose_and_node;
    // the hash is cut by the cell size: a new parameter set starts an empty roadmap, as a new FrontierRoadMap does
    c->rm_xy.clear(); c->rm_hash.clear(); c->rm_key.clear(); c->rm_adj.clear();
    ++c->rm_gen;
    // ... and no pending node, key frame or anchor.  Fresh maps, not clear(): a cleared unordered_map keeps its buckets, and the
    // bucket count decides the iteration order of what is inserted next.
    c->kf_queue.clear();
    std::unordered_map<int32_t, int32_t>().swap(c->kf_handle);
    std::unordered_map<int32_t, int32_t>().swap(c->kf_order);
    c->kf_handle_id.clear(); c->kf_handle_count.clear(); c->kf_slot.clear();
    c->kf_records = 0;
    return FS_OK;
}

int fs_roadmap_add_nodes(fs_ctx *c, int32_t n, const double *xy, int32_t is_robot_pose)
{
    if (!c) return FS_E_INVALID;
    if (n < 0 || (n > 0 && !xy)) return fail(c, FS_E_INVALID, "null pointer");
    if (!rm_finite_xy(xy, n, 2)) return fail(c, FS_E_INVALID, "non-finite node position");
    if (n == 0) return FS_OK;
    ++c->rm_gen;
    const double min_d = is_robot_pose ? c->rm_min_robot : c->rm_min_frontier;
    for (int32_t i = 0; i < n; ++i) {
        const double x = xy[2 * (size_t)i], y = xy[2 * (size_t)i + 1];
        const int cx = fs_rm_cell(x, c->rm_cell), cy = fs_rm_cell(y, c->rm_cell);
        bool fresh = true;
        for (int dx = -1; dx <= 1 && fresh; ++dx)
            for (int dy = -1; dy <= 1 && fresh; ++dy) {
                const auto it = c->rm_hash.find({cx + dx, cy + dy});
                if (it == c->rm_hash.end()) continue;
                for (const int32_t q : it->second) {
                    const double ex = x - c->rm_xy[2 * (size_t)q], ey = y - c->rm_xy[2 * (size_t)q + 1];
                    if (std::sqrt(ex * ex + ey * ey) < min_d) { fresh = false; break; }
                }
            }
        if (!fresh) continue;
        std::vector<int32_t> &cell = c->rm_hash[{cx, cy}];
        cell.push_back(rm_nodes(c));
        c->rm_xy.push_back(x); c->rm_xy.push_back(y);
        c->rm_key.push_back(0);
        c->rm_adj.emplace_back();
        c->kf_queue.push_back(x); c->kf_queue.push_back(y);     // populateNodes(addNewToQueue = true) queues before its throw
        if (cell.size() > RM_MAX_PER_CELL)
            return fail(c, FS_E_RANGE, "hash cell (%d, %d) holds more than %d nodes (the reference throws; the node stays added, the rest of the list is not)",
                        cx, cy, RM_MAX_PER_CELL);
    }
    return FS_OK;
}

int fs_roadmap_rebuild(fs_ctx *c)
{
    if (!c) return FS_E_INVALID;
    int rc = grid2d_check(c, "the roadmap");
    if (rc) return rc;
    const int32_t n = rm_nodes(c);
    ++c->rm_gen;
    std::fill(c->rm_key.begin(), c->rm_key.end(), (uint8_t)1);     // roadmap_.clear(), then roadmap_[point] = {} for every node
    for (auto &l : c->rm_adj) l.clear();
    if (n == 0) return FS_OK;
    const size_t nn = (size_t)n;
    FsRoadmapDev g{};
    std::vector<uint64_t> keys;
    std::vector<int32_t> cstart, cnodes;
    rc = rm_upload_nodes(c, g, keys, cstart, cnodes);
    if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
    FS_HIP(c, c->d_rm_tmp.ensure(nn + 1)); FS_HIP(c, c->d_rm_cand_off.ensure(nn + 1)); FS_HIP(c, c->d_rm_row.ensure(nn + 1));
    FS_HIP(c, c->d_rm_key.ensure(nn));
    FS_HIP(c, hipMemcpyAsync(c->d_rm_key.p, c->rm_key.data(), nn, hipMemcpyHostToDevice, c->stream));
    // candidates: count, scan, fill
    FS_HIP(c, fs_launch_rm_candidates(g, nullptr, c->d_rm_tmp.p, c->origin[2], nullptr, nullptr, nullptr, c->stream));
    FS_HIP(c, fs_launch_rm_scan(c->d_rm_tmp.p, n, c->d_rm_cand_off.p, c->stream));
    int32_t total = 0;
    FS_HIP(c, hipMemcpyAsync(&total, c->d_rm_cand_off.p + n, sizeof total, hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipStreamSynchronize(c->stream));
    rc = rm_seg_ensure(c, (size_t)total);
    if (rc) return rc;
    FS_HIP(c, c->d_rm_cand.ensure((size_t)total));
    FS_HIP(c, fs_launch_rm_candidates(g, c->d_rm_cand_off.p, nullptr, c->origin[2], c->d_seg_start.p, c->d_seg_end.p, c->d_rm_cand.p, c->stream));
    // every isConnectable of the rebuild: one batch of segment walks
    FS_HIP(c, fs_launch_segments(rm_seg_args(c, total), c->stream));
    // accepted edges: count, scan, compact in order
    const double limit = rm_unknown_limit(c);
    FS_HIP(c, fs_launch_rm_edges(n, c->d_rm_cand_off.p, c->d_rm_cand.p, c->d_seg_ok.p, c->d_seg_hit.p, c->d_seg_unknown.p, limit, nullptr,
                                 c->d_rm_tmp.p, nullptr, c->stream));
    FS_HIP(c, fs_launch_rm_scan(c->d_rm_tmp.p, n, c->d_rm_row.p, c->stream));
    std::vector<int32_t> row(nn + 1);
    FS_HIP(c, hipMemcpyAsync(row.data(), c->d_rm_row.p, sizeof(int32_t) * (nn + 1), hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipStreamSynchronize(c->stream));
    const int32_t e = row[nn];
    FS_HIP(c, c->d_rm_col.ensure((size_t)e));
    FS_HIP(c, fs_launch_rm_edges(n, c->d_rm_cand_off.p, c->d_rm_cand.p, c->d_seg_ok.p, c->d_seg_hit.p, c->d_seg_unknown.p, limit, c->d_rm_row.p,
                                 nullptr, c->d_rm_col.p, c->stream));
    std::vector<int32_t> col((size_t)e);
    FS_HIP(c, hipMemcpyAsync(col.data(), c->d_rm_col.p, sizeof(int32_t) * (size_t)e, hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipStreamSynchronize(c->stream));
    for (int32_t p = 0; p < n; ++p) c->rm_adj[(size_t)p].assign(col.begin() + row[(size_t)p], col.begin() + row[(size_t)p + 1]);
    c->rm_dev_gen = c->rm_gen;
    c->rm_traced += total;
    return FS_OK;
}

int fs_roadmap_connect(fs_ctx *c, int32_t n, const double *xy)
{
    if (!c) return FS_E_INVALID;
    if (n < 0 || (n > 0 && !xy)) return fail(c, FS_E_INVALID, "null pointer");
    if (!rm_finite_xy(xy, n, 2)) return fail(c, FS_E_INVALID, "non-finite point");
    int rc = grid2d_check(c, "the roadmap");
    if (rc) return rc;
    const int32_t nodes = rm_nodes(c);
    if (n == 0 || nodes == 0) return FS_OK;      // (an empty hash: the reference's closest-node search would not return)
    // every point's closest hash node and its neighbours within the radius; the walks neighbour -> closest node in one batch
    std::vector<int32_t> closest((size_t)n), nb_off(1, 0), nb, tmp;
    for (int32_t i = 0; i < n; ++i) {
        closest[(size_t)i] = fs_rm_closest(c->rm_xy.data(), nullptr, nodes, c->rm_cell, xy[2 * (size_t)i], xy[2 * (size_t)i + 1]);
        rm_within_radius(c, closest[(size_t)i], tmp);
        for (const int32_t q : tmp) if (q != closest[(size_t)i]) nb.push_back(q);
        nb_off.push_back((int32_t)nb.size());
    }
    const size_t total = nb.size();
    std::vector<uint8_t> ok(total), hit(total);
    std::vector<int32_t> unknown(total);
    if (total) {
        std::vector<double> s(3 * total), e(3 * total);
        for (int32_t i = 0; i < n; ++i)
            for (int32_t k = nb_off[(size_t)i]; k < nb_off[(size_t)i + 1]; ++k) {
                const int32_t q = nb[(size_t)k], p = closest[(size_t)i];
                s[3 * (size_t)k] = c->rm_xy[2 * (size_t)q]; s[3 * (size_t)k + 1] = c->rm_xy[2 * (size_t)q + 1]; s[3 * (size_t)k + 2] = c->origin[2];
                e[3 * (size_t)k] = c->rm_xy[2 * (size_t)p]; e[3 * (size_t)k + 1] = c->rm_xy[2 * (size_t)p + 1]; e[3 * (size_t)k + 2] = c->origin[2];
            }
        rc = rm_seg_ensure(c, total);
        if (rc) return rc;
        FS_HIP(c, hipMemcpyAsync(c->d_seg_start.p, s.data(), sizeof(double) * 3 * total, hipMemcpyHostToDevice, c->stream));
        FS_HIP(c, hipMemcpyAsync(c->d_seg_end.p, e.data(), sizeof(double) * 3 * total, hipMemcpyHostToDevice, c->stream));
        FS_HIP(c, fs_launch_segments(rm_seg_args(c, (int32_t)total), c->stream));
        FS_HIP(c, hipMemcpyAsync(ok.data(), c->d_seg_ok.p, total, hipMemcpyDeviceToHost, c->stream));
        FS_HIP(c, hipMemcpyAsync(hit.data(), c->d_seg_hit.p, total, hipMemcpyDeviceToHost, c->stream));
        FS_HIP(c, hipMemcpyAsync(unknown.data(), c->d_seg_unknown.p, sizeof(int32_t) * total, hipMemcpyDeviceToHost, c->stream));
        FS_HIP(c, hipStreamSynchronize(c->stream));
        c->rm_traced += (int64_t)total;
    }
    // constructNewEdges' insertions, in order (FrontierRoadmap.cpp:279-334)
    ++c->rm_gen;
    const double limit = rm_unknown_limit(c);
    for (int32_t i = 0; i < n; ++i) {
        const int32_t p = closest[(size_t)i];
        c->rm_key[(size_t)p] = 1;
        for (int32_t k = nb_off[(size_t)i]; k < nb_off[(size_t)i + 1]; ++k) {
            const int32_t q = nb[(size_t)k];
            c->rm_key[(size_t)q] = 1;
            std::vector<int32_t> &a = c->rm_adj[(size_t)p], &b = c->rm_adj[(size_t)q];
            if (std::find(a.begin(), a.end(), q) != a.end() || std::find(b.begin(), b.end(), p) != b.end()) continue;
            if (ok[(size_t)k] && !hit[(size_t)k] && !((double)unknown[(size_t)k] > limit)) { a.push_back(q); b.push_back(p); }
        }
    }
    return FS_OK;
}

int fs_roadmap_update(fs_ctx *c, int32_t n, const double *xy, const double robot_xy[2], int32_t add_robot_pose, int32_t *n_nodes_added,
                      int32_t *robot_added, int64_t *n_edges_added)
{
    if (!c) return FS_E_INVALID;
    if (n_nodes_added) *n_nodes_added = 0;
    if (robot_added) *robot_added = 0;
    if (n_edges_added) *n_edges_added = 0;
    if (n < 0 || (n > 0 && !xy) || !robot_xy) return fail(c, FS_E_INVALID, "null pointer");
    if (!rm_finite_xy(xy, n, 2) || !rm_finite_xy(robot_xy, 1, 2)) return fail(c, FS_E_INVALID, "non-finite point");
    int rc = grid2d_check(c, "the roadmap");
    if (rc) return rc;
    FS_HIP(c, c->d_ru_pts.ensure(2 * (size_t)n));
    if (n > 0) FS_HIP(c, hipMemcpyAsync(c->d_ru_pts.p, xy, sizeof(double) * 2 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    RmUpdateOut out;
    rc = rm_update_core(c, n, c->d_ru_pts.p, 2, robot_xy, add_robot_pose != 0, &out);
    if (n_nodes_added) *n_nodes_added = out.kept;
    if (robot_added) *robot_added = out.robot;
    if (n_edges_added) *n_edges_added = out.edges;
    return rc;
}

int fs_roadmap_set_keyframes(fs_ctx *c, int32_t n, const int32_t *kf_id, const double *pose7, int32_t *n_anchored, int32_t *n_orphaned)
{
    if (!c) return FS_E_INVALID;
    if (n < 0 || (n > 0 && (!kf_id || !pose7))) return fail(c, FS_E_INVALID, "null pointer");
    FS_HIP(c, hipSetDevice(c->device));
    // the message's table: one slot per distinct id holding its last pose (latest_keyframe_poses_), every occurrence's id in the
    // cell of its own position (spatial_kf_map_) — checked whole before anything changes
    std::unordered_map<int32_t, int32_t> slot_of;
    std::vector<int32_t> slot_id, occ_slot((size_t)n);
    std::vector<float> rt;
    for (int32_t i = 0; i < n; ++i) {
        const double *q = pose7 + 7 * (size_t)i;
        for (int k = 0; k < 7; ++k)
            if (!std::isfinite(q[k])) return fail(c, FS_E_INVALID, "key frame %d: non-finite pose", (int)i);
        float T[FS_KF_RT];
        const float det = fs_kf_pose_table(q, T);
        bool finite = std::isfinite(det) && det != 0.0f;
        for (int k = 0; k < FS_KF_RT; ++k) finite = finite && std::isfinite(T[k]);
        if (!finite) return fail(c, FS_E_INVALID, "key frame %d: the float rotation has no inverse", (int)i);
        const auto it = slot_of.emplace(kf_id[i], (int32_t)slot_id.size());
        if (it.second) { slot_id.push_back(kf_id[i]); rt.resize(rt.size() + FS_KF_RT); }
        occ_slot[(size_t)i] = it.first->second;
        std::copy(T, T + FS_KF_RT, rt.begin() + (size_t)FS_KF_RT * it.first->second);
    }
    const int32_t slots = (int32_t)slot_id.size();
    std::vector<int32_t> ints((size_t)slots);                  // handle [slots] | cell_start [cells + 1] | cell_slots [n]
    for (int32_t s = 0; s < slots; ++s) {
        const auto it = c->kf_handle.emplace(slot_id[(size_t)s], (int32_t)c->kf_handle_id.size());
        if (it.second) { c->kf_handle_id.push_back(slot_id[(size_t)s]); c->kf_handle_count.push_back(0); }
        ints[(size_t)s] = it.first->second;
    }
    c->kf_slot.assign(c->kf_handle_id.size(), -1);
    for (int32_t s = 0; s < slots; ++s) c->kf_slot[(size_t)ints[(size_t)s]] = s;
    std::map<uint64_t, std::vector<int32_t>> cells;
    for (int32_t i = 0; i < n; ++i) {
        const int cx = fs_rm_cell(pose7[7 * (size_t)i], c->rm_cell), cy = fs_rm_cell(pose7[7 * (size_t)i + 1], c->rm_cell);
        cells[((uint64_t)(uint32_t)cx << 32) | (uint32_t)cy].push_back(occ_slot[(size_t)i]);
    }
    std::vector<uint64_t> keys;
    const size_t o_start = ints.size();
    ints.push_back(0);
    for (const auto &kv : cells) { keys.push_back(kv.first); ints.push_back(ints.back() + (int32_t)kv.second.size()); }
    const size_t o_slots = ints.size();
    for (const auto &kv : cells) ints.insert(ints.end(), kv.second.begin(), kv.second.end());
    FS_HIP(c, c->d_kf_rt.ensure(rt.size())); FS_HIP(c, c->d_kf_tab.ensure(ints.size())); FS_HIP(c, c->d_kf_cell_key.ensure(keys.size()));
    if (!rt.empty()) FS_HIP(c, hipMemcpyAsync(c->d_kf_rt.p, rt.data(), sizeof(float) * rt.size(), hipMemcpyHostToDevice, c->stream));
    FS_HIP(c, hipMemcpyAsync(c->d_kf_tab.p, ints.data(), sizeof(int32_t) * ints.size(), hipMemcpyHostToDevice, c->stream));
    if (!keys.empty()) FS_HIP(c, hipMemcpyAsync(c->d_kf_cell_key.p, keys.data(), sizeof(uint64_t) * keys.size(), hipMemcpyHostToDevice, c->stream));
    // the queue, drained: parents counted, scanned, the records appended in (queue order, list order)
    const int32_t k = (int32_t)(c->kf_queue.size() / 2);
    int32_t anchored = 0, orphaned = 0;
    if (k > 0) {
        const size_t nk = (size_t)k;
        FS_HIP(c, c->d_kf_queue.ensure(2 * nk)); FS_HIP(c, c->d_kf_work.ensure(2 * nk + 1));
        FS_HIP(c, hipMemcpyAsync(c->d_kf_queue.p, c->kf_queue.data(), sizeof(double) * 2 * nk, hipMemcpyHostToDevice, c->stream));
        const FsKfTable t{c->rm_cell, c->d_kf_rt.p, c->d_kf_tab.p, (int32_t)keys.size(), c->d_kf_cell_key.p, c->d_kf_tab.p + o_start,
                          c->d_kf_tab.p + o_slots};
        int32_t *count = c->d_kf_work.p, *off = c->d_kf_work.p + nk;
        FS_HIP(c, fs_launch_kf_anchor(t, k, c->d_kf_queue.p, nullptr, count, nullptr, nullptr, c->stream));
        FS_HIP(c, fs_launch_rm_scan(count, k, off, c->stream));
        FS_HIP(c, c->h_kf.ensure(sizeof(int32_t) * (nk + 1)));
        int32_t *h = reinterpret_cast<int32_t *>(c->h_kf.p);
        FS_HIP(c, hipMemcpyAsync(h, count, sizeof(int32_t) * nk, hipMemcpyDeviceToHost, c->stream));
        FS_HIP(c, hipMemcpyAsync(h + nk, off + nk, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        FS_HIP(c, hipStreamSynchronize(c->stream));
        for (size_t i = 0; i < nk; ++i) orphaned += h[i] == 0 ? 1 : 0;
        anchored = k - orphaned;
        const int64_t total = h[nk], used = c->kf_records;
        if (used + total > (int64_t)INT32_MAX) return fail(c, FS_E_RANGE, "more than 2^31 - 1 anchor records");
        int rc = kf_grow(c, c->d_kf_rec_h, (size_t)used, (size_t)(used + total));
        if (!rc) rc = kf_grow(c, c->d_kf_rec_ord, (size_t)used, (size_t)(used + total));
        if (!rc) rc = kf_grow(c, c->d_kf_rec_p, 3 * (size_t)used, 3 * (size_t)(used + total));
        if (rc) return rc;
        if (total > 0) {
            FS_HIP(c, fs_launch_kf_anchor(t, k, c->d_kf_queue.p, off, nullptr, c->d_kf_rec_h.p + used, c->d_kf_rec_p.p + 3 * used, c->stream));
            // keyframe_mapping_[id].push_back in record order: the shadow map's insertions and each record's ordinal in its vector
            FS_HIP(c, c->h_kf.ensure(sizeof(int32_t) * 2 * (size_t)total));
            h = reinterpret_cast<int32_t *>(c->h_kf.p);
            FS_HIP(c, hipMemcpyAsync(h, c->d_kf_rec_h.p + used, sizeof(int32_t) * (size_t)total, hipMemcpyDeviceToHost, c->stream));
            FS_HIP(c, hipStreamSynchronize(c->stream));
            int32_t *ord = h + total;
            for (int64_t r = 0; r < total; ++r) {
                const int32_t hd = h[r];
                const int32_t id = c->kf_handle_id[(size_t)hd];
                if (c->kf_order.count(id) == 0) c->kf_order[id] = hd;
                ord[r] = (int32_t)c->kf_handle_count[(size_t)hd]++;
            }
            FS_HIP(c, hipMemcpyAsync(c->d_kf_rec_ord.p + used, ord, sizeof(int32_t) * (size_t)total, hipMemcpyHostToDevice, c->stream));
            FS_HIP(c, hipStreamSynchronize(c->stream));
            c->kf_records += total;
        }
        c->kf_queue.clear();
    }
    if (n_anchored) *n_anchored = anchored;
    if (n_orphaned) *n_orphaned = orphaned;
    return FS_OK;
}

int fs_roadmap_optimize(fs_ctx *c)
{
    if (!c) return FS_E_INVALID;
    int rc = grid2d_check(c, "the roadmap");
    if (rc) return rc;
    // optimizeSHM's sequence: the records of the latest message's key frames in keyframe_mapping_'s order, re-placed
    std::vector<int32_t> tab;
    const int64_t m64 = kf_bases(c, true, tab);
    if (m64 > (int64_t)INT32_MAX / 2) return fail(c, FS_E_RANGE, "too many anchor points");
    const int32_t m = (int32_t)m64;
    const size_t H = tab.size(), mm = (size_t)m;
    tab.insert(tab.end(), c->kf_slot.begin(), c->kf_slot.end());        // base [H] | slot [H]
    std::vector<float> out;
    int32_t kept = 0, cut = INT32_MAX;
    int64_t rounds = 0;
    if (m > 0) {
        uint32_t cap = 64;
        while (cap < 2 * (uint32_t)m) cap <<= 1;
        FS_HIP(c, c->d_kf_tab.ensure(2 * H)); FS_HIP(c, c->d_kf_pts.ensure(2 * mm)); FS_HIP(c, c->d_kf_out.ensure(4 + 2 * mm));
        FS_HIP(c, c->d_kf_hkey.ensure(cap)); FS_HIP(c, c->d_kf_state.ensure(2 * mm));
        // ints: hcount [cap] | hcursor [cap] | hstart [cap + 1] | hpts [m] | pslot [m] | count [m] | cand_off [m + 1] | keep_off [m + 1]
        const size_t o_cursor = cap, o_start = 2 * (size_t)cap, o_pts = o_start + cap + 1, o_slot = o_pts + mm, o_count = o_slot + mm,
                     o_cand = o_count + mm, o_keep = o_cand + mm + 1, n_ints = o_keep + mm + 1;
        FS_HIP(c, c->d_kf_work.ensure(n_ints));
        int32_t *w = c->d_kf_work.p;
        FS_HIP(c, hipMemcpyAsync(c->d_kf_tab.p, tab.data(), sizeof(int32_t) * tab.size(), hipMemcpyHostToDevice, c->stream));
        FS_HIP(c, fs_launch_kf_place((int32_t)c->kf_records, c->d_kf_rec_h.p, c->d_kf_rec_ord.p, c->d_kf_rec_p.p, c->d_kf_tab.p + H, c->d_kf_tab.p,
                                     c->d_kf_rt.p, c->d_kf_pts.p, c->stream));
        FS_HIP(c, hipMemsetAsync(c->d_kf_state.p, 0, 2 * mm, c->stream));
        FsKfDedup d{};
        d.m = m; d.xy = c->d_kf_pts.p; d.cell = c->rm_cell; d.min_d = c->rm_min_frontier; d.mask = cap - 1;
        d.hkey = c->d_kf_hkey.p; d.hcount = w; d.hcursor = w + o_cursor; d.hstart = w + o_start; d.hpts = w + o_pts; d.pslot = w + o_slot;
        d.cand_off = w + o_cand; d.state[0] = c->d_kf_state.p; d.state[1] = c->d_kf_state.p + mm;
        d.hdr = reinterpret_cast<int32_t *>(c->d_kf_out.p);
        FS_HIP(c, fs_launch_kf_dedup_cells(d, c->stream));
        FS_HIP(c, fs_launch_kf_dedup_conflicts(d, nullptr, w + o_count, nullptr, c->stream));
        FS_HIP(c, fs_launch_rm_scan(w + o_count, m, w + o_cand, c->stream));
        int32_t total = 0;
        FS_HIP(c, hipMemcpyAsync(&total, w + o_cand + mm, sizeof total, hipMemcpyDeviceToHost, c->stream));
        FS_HIP(c, hipStreamSynchronize(c->stream));
        FS_HIP(c, c->d_kf_cand.ensure((size_t)total));
        d.cand = c->d_kf_cand.p;
        FS_HIP(c, fs_launch_kf_dedup_conflicts(d, w + o_cand, nullptr, c->d_kf_cand.p, c->stream));
        rc = kf_dedup_rounds(c, d, &rounds);
        if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
        FS_HIP(c, fs_launch_kf_dedup_finish(d, 0, w + o_count, w + o_keep, c->d_kf_out.p + 4, c->stream));
        FS_HIP(c, c->h_kf.ensure(sizeof(float) * (4 + 2 * mm)));
        FS_HIP(c, hipMemcpyAsync(c->h_kf.p, c->d_kf_out.p, sizeof(float) * (4 + 2 * mm), hipMemcpyDeviceToHost, c->stream));
        FS_HIP(c, hipStreamSynchronize(c->stream));
        const int32_t *hdr = reinterpret_cast<const int32_t *>(c->h_kf.p);
        kept = hdr[0]; cut = hdr[1];
        if (rounds == -2) rounds = hdr[2];
        if (rounds < 0) return fail(c, FS_E_HIP, "the de-duplication did not settle in %lld rounds", (long long)m + 1);
        if (kept < 0 || kept > m) return fail(c, FS_E_HIP, "de-duplication: %d points kept of %d", (int)kept, (int)m);
        const float *xy = reinterpret_cast<const float *>(c->h_kf.p) + 4;
        out.assign(xy, xy + 2 * (size_t)kept);
    }
    c->kf_rounds = rounds; c->kf_points = m;
    // the hash populateNodes leaves: the kept points in sequence order, no key and no edge until the rebuild
    ++c->rm_gen;
    c->rm_xy.assign(out.begin(), out.end());
    c->rm_hash.clear();
    for (int32_t i = 0; i < kept; ++i)
        c->rm_hash[{fs_rm_cell(c->rm_xy[2 * (size_t)i], c->rm_cell), fs_rm_cell(c->rm_xy[2 * (size_t)i + 1], c->rm_cell)}].push_back(i);
    c->rm_key.assign((size_t)kept, 0);
    c->rm_adj.assign((size_t)kept, {});
    if (cut != INT32_MAX)
        return fail(c, FS_E_RANGE, "optimise: a hash cell holds more than %d nodes (the reference throws out of optimizeSHM; %d nodes kept, "
                    "no key node, no edge)", FS_KF_MAX_PER_CELL, (int)kept);
    return fs_roadmap_rebuild(c);
}

int fs_roadmap_get_anchors(fs_ctx *c, int32_t *n_pending, int64_t *n_records, int32_t *kf_id, float *point_c)
{
    if (!c) return FS_E_INVALID;
    if (n_pending) *n_pending = (int32_t)(c->kf_queue.size() / 2);
    if (n_records) *n_records = c->kf_records;
    if ((!kf_id && !point_c) || c->kf_records == 0) return FS_OK;
    FS_HIP(c, hipSetDevice(c->device));
    const size_t R = (size_t)c->kf_records;
    std::vector<int32_t> h(2 * R);
    std::vector<float> p(3 * R);
    FS_HIP(c, hipMemcpyAsync(h.data(), c->d_kf_rec_h.p, sizeof(int32_t) * R, hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipMemcpyAsync(h.data() + R, c->d_kf_rec_ord.p, sizeof(int32_t) * R, hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipMemcpyAsync(p.data(), c->d_kf_rec_p.p, sizeof(float) * 3 * R, hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipStreamSynchronize(c->stream));
    std::vector<int32_t> base;
    kf_bases(c, false, base);
    for (size_t r = 0; r < R; ++r) {
        const size_t o = (size_t)base[(size_t)h[r]] + (size_t)h[R + r];
        if (kf_id) kf_id[o] = c->kf_handle_id[(size_t)h[r]];
        if (point_c) std::copy(&p[3 * r], &p[3 * r] + 3, point_c + 3 * o);
    }
    return FS_OK;
}

int fs_roadmap_get_graph(fs_ctx *c, int32_t *n_nodes, int64_t *n_edges, double *xy, uint8_t *key, int32_t *row_ptr, int32_t *col)
{
    if (!c) return FS_E_INVALID;
    const int32_t n = rm_nodes(c);
    int64_t e = 0;
    for (const auto &l : c->rm_adj) e += (int64_t)l.size();
    if (n_nodes) *n_nodes = n;
    if (n_edges) *n_edges = e;
    if (xy) std::memcpy(xy, c->rm_xy.data(), sizeof(double) * 2 * (size_t)n);
    if (key) std::memcpy(key, c->rm_key.data(), (size_t)n);
    if (row_ptr || col) {
        int64_t k = 0;
        for (int32_t p = 0; p < n; ++p) {
            if (row_ptr) row_ptr[p] = (int32_t)k;
            for (const int32_t q : c->rm_adj[(size_t)p]) { if (col) col[k] = q; ++k; }
        }
        if (row_ptr) row_ptr[n] = (int32_t)k;
    }
    return FS_OK;
}

int fs_set_roadmap_search(fs_ctx *c, int32_t search)
{
    if (!c) return FS_E_INVALID;
    if (search != FS_ROADMAP_SEARCH_TREE && search != FS_ROADMAP_SEARCH_REFERENCE) return fail(c, FS_E_INVALID, "unknown roadmap search %d", search);
    c->rm_search = search;
    return FS_OK;
}

int fs_roadmap_plan(fs_ctx *c, const double robot_pose7[7], int32_t n, const double *goal_xyz, const uint8_t *achievable_in,
                    double *path_length, double *path_length_m, double *path_heading, uint8_t *achievable)
{
    if (!c) return FS_E_INVALID;
    if (!robot_pose7 || n < 0 || (n > 0 && (!goal_xyz || !path_length || !path_length_m || !path_heading || !achievable)))
        return fail(c, FS_E_INVALID, "null pointer");
    FS_HIP(c, hipSetDevice(c->device));
    if (n == 0) return FS_OK;
    int rc = plan_to_host(c, c->d_rm_out, c->h_rm_out, n, [&] { return roadmap_plan_enqueue(c, robot_pose7, n, goal_xyz, achievable_in); },
                          path_length, path_length_m, path_heading, achievable);
    if (rc || c->rm_search != FS_ROADMAP_SEARCH_REFERENCE) return rc;
    bool redone = false;
    rc = rm_astar_settle(c, [&] { return roadmap_astar_cols(c); }, &redone);
    if (rc || !redone) return rc;
    return plan_to_host(c, c->d_rm_out, c->h_rm_out, n, [] { return FS_OK; }, path_length, path_length_m, path_heading, achievable);
}

int fs_get_frontier_costs_roadmap(fs_ctx *c, const double robot_pose7[7], int32_t n, const double *goal_xyz, const int32_t *frontier_size,
                                  const uint8_t *blacklisted, double alpha, double beta, double max_vx, double max_wz, int with_fisher_information,
                                  fs_record *records, double *weighted_cost, double *arrival_utility, double *distance_utility, int32_t *order,
                                  double *path_length_m)
{
    if (!c) return FS_E_INVALID;
    if (!robot_pose7 || n < 0 || (n > 0 && (!goal_xyz || !records || !weighted_cost))) return fail(c, FS_E_INVALID, "null pointer");
    FS_HIP(c, hipSetDevice(c->device));
    if (n == 0) return FS_OK;
    int rc = check_scoring_state(c, true, with_fisher_information != 0);
    if (rc) return rc;
    const auto rank = [&](const PlannedCols &cols) {
        return frontier_costs_core(c, n, goal_xyz, frontier_size, blacklisted, nullptr, nullptr, nullptr, alpha, beta, max_vx, max_wz,
                                   with_fisher_information != 0, records, weighted_cost, arrival_utility, distance_utility, order, &cols);
    };
    rc = rank_on_plan(c, c->d_rm_out, c->h_rm_out, n, [&] { return roadmap_plan_enqueue(c, robot_pose7, n, goal_xyz, nullptr); }, rank,
                      path_length_m);
    if (rc || c->rm_search != FS_ROADMAP_SEARCH_REFERENCE) return rc;
    // (the ranking synchronised; a query that outgrew the global route's pool leaves columns to be written again, and ranked again)
    bool redone = false;
    rc = rm_astar_settle(c, [&] { return roadmap_astar_cols(c); }, &redone);
    if (rc || !redone) return rc;
    return rank_on_plan(c, c->d_rm_out, c->h_rm_out, n, [] { return FS_OK; }, rank, path_length_m);
}


// search -> roadmap update -> roadmap plan -> arrival (+ Fisher) -> U1 -> order: the update reads the goal column the
// search left on the device, the plan takes its goals from the records the caller receives, the scorer the device columns
int fs_get_frontier_costs_searched_roadmap(fs_ctx *c, const double robot_pose7[7], int32_t lethal_threshold, double max_frontier_distance,
                                           int32_t min_frontier_cluster_size, int32_t max_frontier_cluster_size, int32_t add_robot_pose,
                                           int32_t n_blacklist, const double *blacklist_xy, double alpha, double beta, double max_vx,
                                           double max_wz, int with_fisher_information, int32_t max_records, fs_frontier_record *frontiers,
                                           int32_t *n_frontiers, fs_record *records, double *weighted_cost, double *arrival_utility,
                                           double *distance_utility, int32_t *order, double *path_length_m)
{
    if (!c) return FS_E_INVALID;
    if (!robot_pose7 || !n_frontiers || max_records < 0 || (max_records > 0 && (!frontiers || !records || !weighted_cost)) ||
        n_blacklist < 0 || (n_blacklist > 0 && !blacklist_xy))
        return fail(c, FS_E_INVALID, "null pointer or negative count");
    *n_frontiers = 0;
    if (!rm_finite_xy(robot_pose7, 1, 2)) return fail(c, FS_E_INVALID, "non-finite robot position");
    int rc = grid2d_check(c, "the roadmap");
    if (rc) return rc;
    rc = check_scoring_state(c, true, with_fisher_information != 0);
    if (rc) return rc;
    bool on_map = false;
    std::vector<fs_frontier_record> found;
    rc = searched_list(c, robot_pose7, lethal_threshold, max_frontier_distance, min_frontier_cluster_size, max_frontier_cluster_size,
                       n_blacklist, blacklist_xy, max_records, &on_map, n_frontiers, found);
    if (rc) return rc;
    const int32_t n = *n_frontiers;
    if (n > 0) std::memcpy(frontiers, found.data(), sizeof(fs_frontier_record) * (size_t)n);
    // UpdateRoadmapBT on the searched list (a robot off the map found nothing: the update of an empty list)
    RmUpdateOut upd;
    rc = rm_update_core(c, n, c->d_fs_goal.p, 3, robot_pose7, add_robot_pose != 0, &upd);
    if (rc || n == 0) return rc;
    std::vector<double> goal(3 * (size_t)n);
    for (int32_t k = 0; k < n; ++k) { goal[3 * (size_t)k] = found[(size_t)k].goal_x; goal[3 * (size_t)k + 1] = found[(size_t)k].goal_y; goal[3 * (size_t)k + 2] = 0.0; }
    const auto rank = [&](const PlannedCols &cols) {
        const DevCols dev{c->d_fs_goal.p, c->d_fs_fsize.p, c->d_fs_black.p};
        return frontier_costs_core(c, n, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, alpha, beta, max_vx, max_wz,
                                   with_fisher_information != 0, records, weighted_cost, arrival_utility, distance_utility, order, &cols, &dev);
    };
    rc = rank_on_plan(c, c->d_rm_out, c->h_rm_out, n, [&] { return roadmap_plan_enqueue(c, robot_pose7, n, goal.data(), nullptr); }, rank,
                      path_length_m);
    if (rc || c->rm_search != FS_ROADMAP_SEARCH_REFERENCE) return rc;
    bool redone = false;
    rc = rm_astar_settle(c, [&] { return roadmap_astar_cols(c); }, &redone);
    if (rc || !redone) return rc;
    return rank_on_plan(c, c->d_rm_out, c->h_rm_out, n, [] { return FS_OK; }, rank, path_length_m);
}


// The routes of the plan.  Launch order: the plan (under the REFERENCE search its queries also emit their chains) ->
// route lengths, numbering, route_of -> [sizes on the host: offsets, the FS_E_RANGE checks] -> the lists -> refinePath -> the legs'
// keys, sort, heads, records (fs_pathinfo.hip) -> [distinct poses on the host] -> the info-only scorer -> the per-route columns.
int fs_roadmap_routes(fs_ctx *c, const double robot_pose7[7], int32_t n, const double *goal_xyz, const uint8_t *achievable_in,
                      const fs_route_params *params, double *path_length, double *path_length_m, double *path_heading,
                      uint8_t *achievable, int32_t *route_of, int32_t max_routes, int32_t *n_routes, int32_t *goal_node,
                      uint8_t *complete, int32_t *n_legs, double *info_mean, float *info_min, int32_t *first_unsafe, int64_t max_nodes,
                      int64_t *n_nodes_total, int64_t *node_offset, int32_t *node, int64_t *n_refined_total, int64_t *refined_offset,
                      int32_t *refined_node, double *leg_pose7, float *leg_info)
{
    if (!c) return FS_E_INVALID;
    if (!robot_pose7 || n < 0 || (n > 0 && (!goal_xyz || !path_length || !path_length_m || !path_heading || !achievable || !route_of || !n_routes)))
        return fail(c, FS_E_INVALID, "null pointer");
    if (max_routes < 0 || max_nodes < 0) return fail(c, FS_E_INVALID, "negative max_routes / max_nodes");
    if (max_routes > 0 && (!goal_node || !complete || !n_legs)) return fail(c, FS_E_INVALID, "null pointer");
    const fs_route_params def = {1, 1, 550.0};               // FisherInfoBTPlugin.cpp:20
    const fs_route_params prm = params ? *params : def;
    if (!std::isfinite(prm.fi_threshold)) return fail(c, FS_E_INVALID, "fi_threshold must be finite");
    const bool refine = prm.refine != 0, with_info = prm.with_information != 0;
    const int raw_ptrs = (n_nodes_total ? 1 : 0) + (node_offset ? 1 : 0) + (node ? 1 : 0);
    const int ref_ptrs = (n_refined_total ? 1 : 0) + (refined_offset ? 1 : 0) + (refined_node ? 1 : 0);
    const int leg_ptrs = (leg_pose7 ? 1 : 0) + (leg_info ? 1 : 0);
    if ((raw_ptrs != 0 && raw_ptrs != 3) || (ref_ptrs != 0 && ref_ptrs != 3) || (leg_ptrs != 0 && leg_ptrs != 2))
        return fail(c, FS_E_INVALID, "a dump takes all the pointers of its group or none");
    const bool dump_raw = raw_ptrs == 3, dump_ref = ref_ptrs == 3, dump_leg = leg_ptrs == 2;
    if (dump_ref && !refine) return fail(c, FS_E_INVALID, "the refined dump needs params->refine");
    if (!with_info && (dump_leg || info_mean || info_min || first_unsafe))
        return fail(c, FS_E_INVALID, "information outputs need params->with_information");
    if (with_info && max_routes > 0 && (!info_mean || !info_min || !first_unsafe)) return fail(c, FS_E_INVALID, "null pointer");
    FS_HIP(c, hipSetDevice(c->device));
    int rc = FS_OK;
    if (refine && (rc = grid2d_check(c, "refinePath"))) return rc;
    if (with_info && (rc = check_scoring_state(c, false, true))) return rc;
    c->rt_routes = 0; c->rt_walks = 0; c->rt_poses = 0;
    if (n == 0) {
        if (n_routes) *n_routes = 0;
        if (dump_raw) { *n_nodes_total = 0; node_offset[0] = 0; }
        if (dump_ref) { *n_refined_total = 0; refined_offset[0] = 0; }
        return FS_OK;
    }
    const size_t nn = (size_t)n, nodes = (size_t)rm_nodes(c);
    const bool reference = c->rm_search == FS_ROADMAP_SEARCH_REFERENCE;
    const PlanOutLayout O(nn);
    // page-locked block: n_routes | cursor, walks | route_len | goal_node | route_of | refined_len | complete | node_off
    const size_t h_cnt = 0, h_u64 = 8, h_len = 24, h_goal = h_len + 4 * nodes, h_of = h_goal + 4 * nodes, h_rlen = h_of + 4 * nn,
                 h_comp = h_rlen + 4 * nodes, h_off = (h_comp + nodes + 7) & ~(size_t)7, h_total = h_off + 8 * (nodes + 1);
    FS_HIP(c, c->h_rt.ensure(h_total)); FS_HIP(c, c->h_rm_out.ensure(O.total));
    // device words: len | has | ridx [nodes + 1] | goal_node | route_len | route_q | refined_len
    FS_HIP(c, c->d_rt_idx.ensure(7 * nodes + 1)); FS_HIP(c, c->d_rt_of.ensure(nn)); FS_HIP(c, c->d_rt_off.ensure(nodes + 1));
    FS_HIP(c, c->d_rt_complete.ensure(std::max<size_t>(nodes, 1))); FS_HIP(c, c->d_rt_cursor.ensure(2));
    FS_HIP(c, c->d_as_gnode.ensure(nn)); FS_HIP(c, c->d_as_mark.ensure(std::max<size_t>(nodes, 1))); FS_HIP(c, c->d_as_qidx.ensure(nodes + 1));
    // (an error after the first launch waits for the stream: the next call may grow what the launches still use)
    const auto stop = [&](int code) { (void)hipStreamSynchronize(c->stream); return code; };
    c->rt_chains = reference;
    rc = roadmap_plan_enqueue(c, robot_pose7, n, goal_xyz, achievable_in);
    c->rt_chains = false;
    if (rc) return stop(rc);
    FsRmRouteArgs ra{};
    ra.n_nodes = (int32_t)nodes;
    ra.mark = c->d_as_mark.p;
    ra.len = c->d_rt_idx.p; ra.has = ra.len + nodes; int32_t *ridx = ra.has + nodes; ra.ridx = ridx;
    ra.goal_node = ridx + nodes + 1; ra.route_len = ra.goal_node + nodes; ra.route_q = ra.route_len + nodes;
    int32_t *d_rlen = ra.route_q + nodes;
    ra.n = n; ra.gnode = c->d_as_gnode.p; ra.route_of = c->d_rt_of.p;
    if (reference) {
        ra.qidx = c->d_as_qidx.p; ra.status = c->d_as_status.p; ra.chain_len = c->d_rt_chain_len.p; ra.chain_base = c->d_rt_chain_base.p;
        // (a plan without a start node or a searched goal makes no query and leaves the marks as they were)
        if (c->rt_plan.root < 0 && nodes > 0) FS_HIP(c, hipMemsetAsync(c->d_as_mark.p, 0, sizeof(int32_t) * nodes, c->stream));
    } else {
        // the plan's goal nodes and their marks, as the REFERENCE plan makes them
        if (nodes > 0) FS_HIP(c, hipMemsetAsync(c->d_as_mark.p, 0, sizeof(int32_t) * nodes, c->stream));
        FS_HIP(c, fs_launch_rm_astar_goals(c->rt_plan, c->d_as_gnode.p, c->d_as_mark.p, c->stream));
        ra.d = c->rt_plan.d; ra.pred = c->rt_plan.pred;
        ra.hops = c->rt_plan.d ? c->d_rm_hops.p + (size_t)c->rm_tree_buf * nodes : nullptr;
    }
    // stage 1, and everything the host sizes the rest by
    const auto stage1 = [&]() -> int {
        ra.chain_pool = c->d_rt_pool.p;
        FS_HIP(c, fs_launch_rm_route_lengths(ra, c->stream));
        if (nodes > 0) FS_HIP(c, fs_launch_rm_scan(ra.has, (int32_t)nodes, ridx, c->stream));
        else FS_HIP(c, hipMemsetAsync(ridx, 0, sizeof(int32_t), c->stream));
        FS_HIP(c, fs_launch_rm_route_index(ra, c->stream));
        FS_HIP(c, hipMemcpyAsync(c->h_rt.p + h_cnt, ridx + nodes, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        if (reference) FS_HIP(c, hipMemcpyAsync(c->h_rt.p + h_u64, c->d_rt_cursor.p, 8, hipMemcpyDeviceToHost, c->stream));
        if (nodes > 0) {
            FS_HIP(c, hipMemcpyAsync(c->h_rt.p + h_len, ra.route_len, 4 * nodes, hipMemcpyDeviceToHost, c->stream));
            FS_HIP(c, hipMemcpyAsync(c->h_rt.p + h_goal, ra.goal_node, 4 * nodes, hipMemcpyDeviceToHost, c->stream));
        }
        FS_HIP(c, hipMemcpyAsync(c->h_rt.p + h_of, ra.route_of, 4 * nn, hipMemcpyDeviceToHost, c->stream));
        FS_HIP(c, hipMemcpyAsync(c->h_rm_out.p, c->d_rm_out.p, O.total, hipMemcpyDeviceToHost, c->stream));
        FS_HIP(c, hipStreamSynchronize(c->stream));
        return FS_OK;
    };
    if ((rc = stage1())) return stop(rc);
    if (reference) {
        // a query that outgrew the A*'s record pool ran again (its chain with it); a call whose chains outgrew the chain pool runs
        // every query again on a pool of the size the cursor asks for — the chains then sit where this run's atomics put them, and
        // the gather below orders them, so the lists do not depend on the schedule
        bool redone = false;
        rc = rm_astar_settle(c, [&] { return roadmap_astar_cols(c); }, &redone);
        if (rc) return rc;
        unsigned long long cursor = 0;
        if (redone) {
            FS_HIP(c, hipMemcpyAsync(c->h_rt.p + h_u64, c->d_rt_cursor.p, 8, hipMemcpyDeviceToHost, c->stream));
            FS_HIP(c, hipStreamSynchronize(c->stream));
        }
        std::memcpy(&cursor, c->h_rt.p + h_u64, 8);
        if ((int64_t)cursor > c->rt_pool_cap) {
            if (cursor > (1ull << 30)) return fail(c, FS_E_RANGE, "%llu route nodes: beyond the chain pool's limit", cursor);
            ++c->rt_retries;
            c->rt_pool_cap = (int64_t)cursor;
            FS_HIP(c, c->d_rt_pool.ensure((size_t)cursor));
            FsRmAstarArgs &q = c->as_args;
            q.chain_pool = c->d_rt_pool.p; q.chain_cap = c->rt_pool_cap;
            FS_HIP(c, hipMemsetAsync(c->d_rt_cursor.p, 0, 8, c->stream));
            FS_HIP(c, hipMemsetAsync(c->d_as_stats.p, 0, 8 * sizeof(int32_t), c->stream));
            FS_HIP(c, fs_launch_rm_astar(q, c->rt_max_q, c->stream));
            redone = true;
        }
        if (redone && (rc = stage1())) return stop(rc);
    }
    int32_t routes = 0;
    std::memcpy(&routes, c->h_rt.p + h_cnt, sizeof routes);
    const int32_t *h_route_len = reinterpret_cast<const int32_t *>(c->h_rt.p + h_len);
    int64_t *h_node_off = reinterpret_cast<int64_t *>(c->h_rt.p + h_off);
    h_node_off[0] = 0;
    for (int32_t r = 0; r < routes; ++r) h_node_off[r + 1] = h_node_off[r] + h_route_len[r];
    const int64_t total = h_node_off[routes];
    c->rt_routes = routes;
    *n_routes = routes;
    if (dump_raw) *n_nodes_total = total;
    if (dump_ref) *n_refined_total = total;                  // (its upper bound: what FS_E_RANGE reports before any list is made)
    if (routes > max_routes) return fail(c, FS_E_RANGE, "%d routes, room for %d", routes, max_routes);
    if ((dump_raw || dump_ref || dump_leg) && total > max_nodes)
        return fail(c, FS_E_RANGE, "%lld route nodes, room for %lld", (long long)total, (long long)max_nodes);
    const int64_t leg_bound = total - routes;                // (every route holds at least one node)
    if (leg_bound > (int64_t)INT32_MAX) return fail(c, FS_E_INVALID, "%lld route legs: beyond 2^31", (long long)leg_bound);
    const size_t nr = (size_t)routes, nt = (size_t)total;
    // stage 2: the lists, then refinePath
    FS_HIP(c, c->d_rt_node.ensure(std::max<size_t>(nt, 1)));
    if (refine) { FS_HIP(c, c->d_rt_refined.ensure(std::max<size_t>(nt, 1))); FS_HIP(c, c->h_rt_list.ensure(4 * std::max<size_t>(nt, 1))); }
    FS_HIP(c, hipMemcpyAsync(c->d_rt_off.p, h_node_off, 8 * (nr + 1), hipMemcpyHostToDevice, c->stream));
    ra.n_routes = routes; ra.node_off = c->d_rt_off.p; ra.node = c->d_rt_node.p; ra.chain_pool = c->d_rt_pool.p;
    FS_HIP(c, fs_launch_rm_route_emit(ra, c->stream));
    FS_HIP(c, hipMemsetAsync(c->d_rt_cursor.p + 1, 0, 8, c->stream));
    if (refine) {
        FsRouteRefineArgs fa{};
        fa.grid = grid_dev(c);
        fa.max_length = (double)(unsigned)(c->rm_radius * 1.5 / c->res);
        fa.unknown_limit = rm_unknown_limit(c);
        fa.xy = c->d_rm_xy.p;
        fa.n_routes = routes; fa.node_off = c->d_rt_off.p; fa.node = c->d_rt_node.p;
        fa.refined = c->d_rt_refined.p; fa.refined_len = d_rlen; fa.complete = c->d_rt_complete.p;
        fa.walks = c->d_rt_cursor.p + 1;
        FS_HIP(c, fs_launch_route_refine(fa, c->stream));
        if (nr > 0) {
            FS_HIP(c, hipMemcpyAsync(c->h_rt.p + h_rlen, d_rlen, 4 * nr, hipMemcpyDeviceToHost, c->stream));
            FS_HIP(c, hipMemcpyAsync(c->h_rt.p + h_comp, c->d_rt_complete.p, nr, hipMemcpyDeviceToHost, c->stream));
        }
        if (dump_ref && nt > 0) FS_HIP(c, hipMemcpyAsync(c->h_rt_list.p, c->d_rt_refined.p, 4 * nt, hipMemcpyDeviceToHost, c->stream));
        FS_HIP(c, hipMemcpyAsync(c->h_rt.p + h_u64 + 8, c->d_rt_cursor.p + 1, 8, hipMemcpyDeviceToHost, c->stream));
    }
    if (dump_raw && nt > 0) FS_HIP(c, hipMemcpyAsync(node, c->d_rt_node.p, 4 * nt, hipMemcpyDeviceToHost, c->stream));
    const int32_t *d_list_len = refine ? d_rlen : ra.route_len;
    const PathInfoOutLayout P(nr);
    FsPathInfoArgs a{};
    int64_t legs = 0, distinct = 0;
    if (with_info) {
        // the legs through fs_plan_paths_information's route: a "frontier" is a route, a "way point" a leg
        FS_HIP(c, c->d_pi_off.ensure(2 * (nr + 1)));
        FS_HIP(c, c->d_pi_out.ensure(P.total)); FS_HIP(c, c->h_pi_out.ensure(P.total));
        a.n = routes;
        a.node_xy = c->d_rm_xy.p; a.n_nodes = (int32_t)nodes;
        a.list = refine ? c->d_rt_refined.p : c->d_rt_node.p; a.list_off = c->d_rt_off.p; a.list_len = d_list_len;
        a.dedup = c->opt_rt_dedup ? 1 : 0;
        a.fi_threshold = prm.fi_threshold;
        const size_t bytes = fs_pathinfo_temp_bytes(a, leg_bound, c->stream);
        if (bytes == 0) return stop(fail(c, FS_E_HIP, "rocPRIM refused the size query"));
        FS_HIP(c, c->d_pi_temp.ensure(bytes));
        a.count = c->d_pi_off.p; a.offset = c->d_pi_off.p + nr + 1;
        a.hdr = reinterpret_cast<int64_t *>(c->d_pi_out.p + P.hdr);
        a.info_mean = reinterpret_cast<double *>(c->d_pi_out.p + P.mean);
        a.info_min = reinterpret_cast<float *>(c->d_pi_out.p + P.min);
        a.first_unsafe = reinterpret_cast<int32_t *>(c->d_pi_out.p + P.unsafe);
        a.temp = c->d_pi_temp.p; a.temp_bytes = c->d_pi_temp.cap;
        if (fs_launch_pathinfo_offsets(a, c->stream) != hipSuccess) return stop(fail(c, FS_E_HIP, "leg offsets: launch failed"));
        int64_t *hdr = reinterpret_cast<int64_t *>(c->h_pi_out.p + P.hdr);
        if (leg_bound > 0 && (rc = pathinfo_prepare(c, a, leg_bound, dump_leg, "route legs", hdr, stop))) return rc;
        // the scoring launch is sized by the number of distinct poses
        FS_HIP(c, hipStreamSynchronize(c->stream));
        legs = leg_bound > 0 ? hdr[0] : 0; distinct = leg_bound > 0 ? hdr[1] : 0;
        c->rt_poses = distinct;
        if (distinct > 0 && (rc = pathinfo_score(c, a, distinct, stop))) return rc;
        if (fs_launch_pathinfo_finish(a, c->stream) != hipSuccess) return stop(fail(c, FS_E_HIP, "route information columns: launch failed"));
        FS_HIP(c, hipMemcpyAsync(c->h_pi_out.p + P.mean, c->d_pi_out.p + P.mean, P.total - P.mean, hipMemcpyDeviceToHost, c->stream));
        if (dump_leg && legs > 0) {
            FS_HIP(c, hipMemcpyAsync(leg_pose7, a.pose7, sizeof(double) * 7 * (size_t)legs, hipMemcpyDeviceToHost, c->stream));
            FS_HIP(c, hipMemcpyAsync(leg_info, a.wp_info, sizeof(float) * (size_t)legs, hipMemcpyDeviceToHost, c->stream));
        }
    }
    FS_HIP(c, hipStreamSynchronize(c->stream));
    // everything is on the host: the caller's arrays
    plan_columns_to_caller(c->h_rm_out, nn, path_length, path_length_m, path_heading, achievable);
    std::memcpy(route_of, c->h_rt.p + h_of, 4 * nn);
    const int32_t *h_list_len = refine ? reinterpret_cast<const int32_t *>(c->h_rt.p + h_rlen) : h_route_len;
    if (nr > 0) {
        std::memcpy(goal_node, c->h_rt.p + h_goal, 4 * nr);
        if (refine) std::memcpy(complete, c->h_rt.p + h_comp, nr);
        else std::memset(complete, 1, nr);
        for (size_t r = 0; r < nr; ++r) n_legs[r] = h_list_len[r] - 1;
        if (with_info) {
            std::memcpy(info_mean, c->h_pi_out.p + P.mean, 8 * nr);
            std::memcpy(info_min, c->h_pi_out.p + P.min, 4 * nr);
            std::memcpy(first_unsafe, c->h_pi_out.p + P.unsafe, 4 * nr);
        }
    }
    if (refine) {
        unsigned long long walks = 0;
        std::memcpy(&walks, c->h_rt.p + h_u64 + 8, 8);
        c->rt_walks = (int64_t)walks;
    }
    if (dump_raw) std::memcpy(node_offset, h_node_off, 8 * (nr + 1));
    if (dump_ref) {
        const int32_t *src = reinterpret_cast<const int32_t *>(c->h_rt_list.p);
        int64_t k = 0;
        for (size_t r = 0; r < nr; ++r) {
            refined_offset[r] = k;
            std::memcpy(refined_node + k, src + h_node_off[r], 4 * (size_t)h_list_len[r]);
            k += h_list_len[r];
        }
        refined_offset[nr] = k;
        *n_refined_total = k;
    }
    return FS_OK;
}

}  // extern "C"

// ================================================================== next goal (FullPathOptimizer::getNextGoal)
// The selection is sequential and small and stays on the host; the pair matrix (one tree per source, all in one launch) and the
// exhaustive tour search run on the device.

namespace {

#define FS_SAFE 0
#define FS_UNSAFE 1
#define FS_UNDETERMINED 2
#define TOUR_SEL_LOCAL 1
#define TOUR_SEL_GLOBAL 2
#define TOUR_SEL_CLOSEST 4

// work buffer on the device: matrix | result (length, robot leg, rank, count) | block winners (length, leg, rank, count columns)
constexpr size_t kTourOffRes = 2048, kTourOffBlk = 2048 + 64, kTourMaxBlk = 1024;
constexpr size_t kTourWork = kTourOffBlk + 4 * 8 * kTourMaxBlk;
// pinned host block: matrix | result | rounds of each tree
constexpr size_t kTourOffRounds = kTourOffRes + 64, kTourOut = kTourOffRounds + 4 * RM_TOUR_MAX_TREES;

// getFilteredFrontiersN (FullPathOptimizer.cpp:157-227) with all its quirks; ties in path length go to the lower input index (the
// reference's std::sort is not stable).  cg = closest_global_frontier, -1 while unset.
void tour_select(int32_t n, const double *plm, const std::vector<uint8_t> &eligible, int32_t n_local, double radius,
                 std::vector<int32_t> &loc, std::vector<int32_t> &glob, int32_t &cg)
{
    std::vector<int32_t> all;
    for (int32_t i = 0; i < n; ++i) if (eligible[(size_t)i]) all.push_back(i);
    std::stable_sort(all.begin(), all.end(), [plm](int32_t a, int32_t b) { return plm[a] < plm[b]; });
    loc.clear(); glob.clear(); cg = -1;
    if (all.empty()) return;
    bool global_assigned = false, need_to_pop = false;
    int64_t counter = 1;
    for (const int32_t f : all) {
        const double L = plm[f];
        if (L <= radius && counter <= n_local) { loc.push_back(f); cg = f; need_to_pop = true; }
        else if (L <= radius && counter > n_local) { cg = f; need_to_pop = false; }
        else if (L > radius) {
            if (!global_assigned) { cg = f; global_assigned = true; }
            need_to_pop = false;
            glob.push_back(f);
        }
        ++counter;
    }
    if (need_to_pop) loc.pop_back();
    if (glob.empty() && loc.empty()) glob.push_back(cg);
}

// isRobotPoseSafe (FullPathOptimizer.cpp:342-352) through the one-pose info-only scorer: safe when info_ref > threshold
int tour_pose_safe(fs_ctx *c, const double *pose7, double threshold, int32_t *status)
{
    float info = 0.0f;
    int32_t nvox = 0;
    const int rc = fs_score_fim(c, 1, pose7, &info, nullptr, nullptr, nullptr, nullptr, &nvox);
    if (rc) return rc;
    *status = (double)info > threshold ? FS_SAFE : FS_UNSAFE;
    return FS_OK;
}

// rank -> the lexicographic permutation of 0..k-1 of that rank (factorial number system)
void tour_unrank(int64_t rank, int k, int32_t *perm)
{
    int64_t f = 1;
    for (int t = 2; t < k; ++t) f *= t;
    std::vector<int32_t> left;
    for (int t = 0; t < k; ++t) left.push_back(t);
    for (int t = 0; t < k; ++t) {
        const int64_t d = rank / f;
        rank -= d * f;
        if (t < k - 1) f /= (k - 1 - t);
        perm[t] = left[(size_t)d];
        left.erase(left.begin() + d);
    }
}

// K shortest-path trees of the device roadmap (rm_device_graph has run), one per root, in batches of RM_TOUR_MAX_TREES and in the
// caller's buffers: d / hops / pred [K][2][nodes] (the single-tree cache of rm_tree is neither read nor replaced), `word` of
// max(PLAN_BATCH, K) words.  Up to tour_one_wg nodes a batch is one workgroup's loop per tree, not waited for: word[b] will hold the
// rounds of tree b (negative: not settled) and the caller reads them with its results.  Above, a round per launch, polled (`what`
// names the trees in poll_rounds' error); *rounds is then what the slowest batch took.  After its quiet round both buffers of a
// tree hold it: buffer 0 is read.
int rm_trees_enqueue(fs_ctx *c, const DevBuf<double> &d, const DevBuf<int32_t> &hops, const DevBuf<int32_t> &pred, const DevBuf<int32_t> &word,
                     const int32_t *roots, int32_t K, const char *what, bool *polled, int64_t *rounds)
{
    const int32_t n = rm_nodes(c);
    const int64_t max_rounds = 2 * (int64_t)n + 2;        // as rm_tree
    *polled = n > c->tour_one_wg;
    *rounds = 0;
    for (int32_t k0 = 0; k0 < K; k0 += RM_TOUR_MAX_TREES) {
        FsRmTreeBatch B{};
        const size_t o = 2 * (size_t)n * (size_t)k0;
        B.t = FsRmTree{n, -1, c->d_rm_xy.p, c->d_rm_trow.p, c->d_rm_tcol.p, {d.p + o, nullptr}, {hops.p + o, nullptr}, {pred.p + o, nullptr}};
        B.k = std::min<int32_t>(RM_TOUR_MAX_TREES, K - k0);
        for (int32_t b = 0; b < B.k; ++b) B.root[b] = roots[k0 + b];
        FS_HIP(c, fs_launch_rm_batch_init(B, c->stream));
        if (!*polled) {
            FS_HIP(c, fs_launch_rm_batch_block(B, (int32_t)max_rounds, word.p + k0, c->stream));
            continue;
        }
        const auto launch = [&](int64_t r0, int count) -> int {
            for (int k = 0; k < count; ++k) FS_HIP(c, fs_launch_rm_batch_round(B, (int32_t)((r0 + k) & 1), word.p + k, c->stream));
            return FS_OK;
        };
        int64_t batch_rounds = 0;
        const int rc = poll_rounds(c, word.p, PLAN_BATCH, PLAN_BATCH, 1, max_rounds, what, max_rounds, launch, &batch_rounds);
        if (rc) return rc;
        *rounds = std::max(*rounds, batch_rounds);
    }
    return FS_OK;
}

// The trees of the batch (one per distinct source root), then the pair kernel and the tour search, all on the stream; the
// one-workgroup route leaves everything to the caller's single synchronisation, the round-per-launch route polls its rounds.
// Result, matrix and (one-workgroup route) the trees' rounds are copied to h_tour_out.
int tour_enqueue(fs_ctx *c, const FsRmPairArgs &pa_in, int32_t K, const int32_t *roots, int32_t k, bool *polled, int64_t *rounds_out)
{
    const int32_t n = rm_nodes(c);
    const size_t nn = (size_t)n;
    FsRmPairArgs pa = pa_in;
    FS_HIP(c, c->d_tour_work.ensure(kTourWork)); FS_HIP(c, c->h_tour_out.ensure(kTourOut));
    FS_HIP(c, c->d_tour_word.ensure(std::max(PLAN_BATCH, RM_TOUR_MAX_TREES)));
    *polled = false;
    *rounds_out = 0;
    if (K > 0) {
        int rc = rm_device_graph(c);
        if (rc) return rc;
        FS_HIP(c, c->d_tour_d.ensure(2 * nn * K)); FS_HIP(c, c->d_tour_hops.ensure(2 * nn * K)); FS_HIP(c, c->d_tour_pred.ensure(2 * nn * K));
        rc = rm_trees_enqueue(c, c->d_tour_d, c->d_tour_hops, c->d_tour_pred, c->d_tour_word, roots, K, "the tour trees", polled, rounds_out);
        if (rc) return rc;
        if (!*polled)
            FS_HIP(c, hipMemcpyAsync(c->h_tour_out.p + kTourOffRounds, c->d_tour_word.p, sizeof(int32_t) * (size_t)K, hipMemcpyDeviceToHost,
                                     c->stream));
        pa.d = c->d_tour_d.p; pa.pred = c->d_tour_pred.p;
    }
    pa.n_nodes = n; pa.xy = c->d_rm_xy.p;
    pa.M = reinterpret_cast<double *>(c->d_tour_work.p);
    FS_HIP(c, fs_launch_rm_pairs(pa, c->stream));
    int64_t total = 1;
    for (int t = 2; t <= k; ++t) total *= t;
    FsRmTourArgs ta{};
    ta.k = k; ta.M = pa.M; ta.total = total;
    const int32_t blocks = fs_rm_tour_blocks(total, &ta.chunk);
    char *blk = c->d_tour_work.p + kTourOffBlk;
    ta.blen = reinterpret_cast<double *>(blk); ta.bleg = ta.blen + kTourMaxBlk;
    ta.brank = reinterpret_cast<int64_t *>(ta.bleg + kTourMaxBlk); ta.bcnt = ta.brank + kTourMaxBlk;
    FS_HIP(c, fs_launch_rm_tour(ta, blocks, reinterpret_cast<double *>(c->d_tour_work.p + kTourOffRes), c->stream));
    FS_HIP(c, hipMemcpyAsync(c->h_tour_out.p, c->d_tour_work.p, kTourOffRes + 32, hipMemcpyDeviceToHost, c->stream));
    c->tour_evaluated += total;
    return FS_OK;
}

// The REFERENCE search's pair lengths: pair (i, j), i < j, is the A* from start[i] to start[j] (distinct pairs run once; equal
// points and points without a key node run none).  The queries are enqueued and pa points the pair kernel at their results.
int tour_astar_enqueue(fs_ctx *c, FsRmPairArgs &pa)
{
    const int32_t m = pa.m, nodes = rm_nodes(c);
    std::vector<int32_t> qs, qd;
    for (int32_t l = 0; l < m * m; ++l) pa.query[l] = -1;
    for (int32_t i = 0; i < m; ++i)
        for (int32_t j = i + 1; j < m; ++j) {
            if ((pa.pxy[2 * i] == pa.pxy[2 * j] && pa.pxy[2 * i + 1] == pa.pxy[2 * j + 1]) || pa.start[i] < 0 || pa.start[j] < 0) continue;
            size_t q = 0;
            while (q < qs.size() && !(qs[q] == pa.start[i] && qd[q] == pa.start[j])) ++q;
            if (q == qs.size()) { qs.push_back(pa.start[i]); qd.push_back(pa.start[j]); }
            pa.query[i * m + j] = (int32_t)q;
        }
    const int32_t nq = (int32_t)qs.size();
    // the query list staged behind the stats in h_as_io: nq | src [nq] | dst [nq]
    FS_HIP(c, c->h_as_io.ensure(64 + 4 * (1 + 2 * (size_t)nq)));
    FS_HIP(c, c->d_as_src.ensure(1 + 2 * (size_t)nq));
    FS_HIP(c, c->d_as_status.ensure((size_t)std::max(nq, 1))); FS_HIP(c, c->d_as_len.ensure((size_t)std::max(nq, 1)));
    int32_t *h = reinterpret_cast<int32_t *>(c->h_as_io.p + 64);
    h[0] = nq;
    std::copy(qs.begin(), qs.end(), h + 1);
    std::copy(qd.begin(), qd.end(), h + 1 + nq);
    FS_HIP(c, hipMemcpyAsync(c->d_as_src.p, h, 4 * (1 + 2 * (size_t)nq), hipMemcpyHostToDevice, c->stream));
    FsRmAstarArgs q{};
    q.n_nodes = nodes;
    if (nq > 0) {
        const int rc = rm_device_graph(c);
        if (rc) return rc;
        q.xy = c->d_rm_xy.p; q.row = c->d_rm_row.p; q.col = c->d_rm_col.p;
    }
    q.nq = c->d_as_src.p; q.src = c->d_as_src.p + 1; q.dst = c->d_as_src.p + 1 + nq;
    q.status = c->d_as_status.p; q.len = c->d_as_len.p;
    q.lds_cap = rm_astar_lds_cap(c, nodes);
    const int rc = rm_astar_enqueue(c, q, nq);
    if (rc) return rc;
    pa.q_status = c->d_as_status.p; pa.q_len = c->d_as_len.p;
    return FS_OK;
}

}  // namespace

extern "C" {

int fs_roadmap_next_goal(fs_ctx *c, const double robot_pose7[7], int32_t n, const double *goal_xyz, const double *path_length_m,
                         const uint8_t *achievable, const uint8_t *blacklisted, int32_t n_blacklist_circles, const double *blacklist_xy,
                         int32_t n_local, double local_radius, const double *fi_pose7, double fi_threshold, int32_t *next_index,
                         int32_t *status, int32_t *tour, int32_t *tour_size, double *tour_length, int64_t *n_tied, uint8_t *selection,
                         double *pair_length_m)
{
    if (!c) return FS_E_INVALID;
    if (!robot_pose7 || n < 0 || (n > 0 && (!goal_xyz || !path_length_m || !achievable)) || n_blacklist_circles < 0 ||
        (n_blacklist_circles > 0 && !blacklist_xy) || !next_index || !status || !tour || !tour_size || !tour_length || !n_tied)
        return fail(c, FS_E_INVALID, "null pointer");
    if (n_local < 1 || n_local > RM_TOUR_MAX_LOCAL) return fail(c, FS_E_INVALID, "n_local must be 1..%d", RM_TOUR_MAX_LOCAL);
    if (!(local_radius >= 0 && std::isfinite(local_radius))) return fail(c, FS_E_INVALID, "local_radius must be finite and >= 0");
    if (!std::isfinite(robot_pose7[0]) || !std::isfinite(robot_pose7[1])) return fail(c, FS_E_INVALID, "non-finite robot pose");
    FS_HIP(c, hipSetDevice(c->device));
    if (rm_nodes(c) == 0) return fail(c, FS_E_STATE, "no roadmap: fs_roadmap_add_nodes has not given it a node");
    // eligibility: achievable, not blacklisted, outside every blacklist circle (isInBlacklistedRegion: distance < 1.7)
    std::vector<uint8_t> eligible((size_t)n);
    for (int32_t i = 0; i < n; ++i) {
        bool ok = achievable[i] && !(blacklisted && blacklisted[i]);
        for (int32_t b = 0; ok && b < n_blacklist_circles; ++b) {
            const double ex = goal_xyz[3 * (size_t)i] - blacklist_xy[2 * (size_t)b], ey = goal_xyz[3 * (size_t)i + 1] - blacklist_xy[2 * (size_t)b + 1];
            if (std::sqrt(ex * ex + ey * ey) < 1.7) ok = false;
        }
        if (ok && (std::isnan(path_length_m[i]) || !std::isfinite(goal_xyz[3 * (size_t)i]) || !std::isfinite(goal_xyz[3 * (size_t)i + 1])))
            return fail(c, FS_E_INVALID, "eligible frontier %d has a NaN path length or a non-finite goal", (int)i);
        eligible[(size_t)i] = ok;
    }
    std::vector<int32_t> loc, glob;
    int32_t cg = -1;
    tour_select(n, path_length_m, eligible, n_local, local_radius, loc, glob, cg);
    if (selection) {
        for (int32_t i = 0; i < n; ++i) selection[i] = 0;
        for (const int32_t f : loc) selection[f] = TOUR_SEL_LOCAL;
        for (const int32_t f : glob) selection[f] = TOUR_SEL_GLOBAL;
        if (cg >= 0) selection[cg] |= TOUR_SEL_CLOSEST;
    }
    *next_index = -1; *status = FS_UNDETERMINED; *tour_size = 0; *tour_length = 0.0; *n_tied = 0;
    const int32_t k = (int32_t)loc.size();
    if (k == 0) {
        if (glob.empty()) return FS_OK;                                 // the zero frontier
        *next_index = cg; tour[0] = cg; *tour_size = 1; *status = FS_SAFE;
        return fi_pose7 ? tour_pose_safe(c, fi_pose7, fi_threshold, status) : FS_OK;
    }
    // the nodes [robot, locals in selection order, closest global], their closest key nodes, one tree per distinct source root
    const int32_t m = k + 2, nodes = rm_nodes(c);
    FsRmPairArgs pa{};
    pa.m = m; pa.charge = local_radius * 100000.0;
    for (int32_t i = 0; i < m; ++i) {
        const double *g = i == 0 ? robot_pose7 : goal_xyz + 3 * (size_t)(i <= k ? loc[(size_t)i - 1] : cg);
        pa.pxy[2 * i] = g[0]; pa.pxy[2 * i + 1] = g[1];
        pa.start[i] = fs_rm_closest(c->rm_xy.data(), c->rm_key.data(), nodes, c->rm_cell, g[0], g[1]);
    }
    int32_t roots[RM_TOUR_MAX_TREES], K = 0;
    const bool reference = c->rm_search == FS_ROADMAP_SEARCH_REFERENCE;
    for (int32_t i = 0; i < m - 1 && !reference; ++i) {
        pa.tree[i] = 0;
        if (pa.start[i] < 0) continue;
        int32_t b = 0;
        while (b < K && roots[b] != pa.start[i]) ++b;
        if (b == K) roots[K++] = pa.start[i];
        pa.tree[i] = b;
    }
    bool polled = false;
    int64_t rounds = 0;
    int rc = reference ? tour_astar_enqueue(c, pa) : FS_OK;
    if (!rc) rc = tour_enqueue(c, pa, K, roots, k, &polled, &rounds);
    if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
    FS_HIP(c, hipStreamSynchronize(c->stream));
    if (reference) {
        bool redone = false;
        rc = rm_astar_settle(c, [&] { return tour_enqueue(c, pa, 0, roots, k, &polled, &rounds); }, &redone);
        if (rc) return rc;
    }
    if (!polled) {
        for (int32_t b = 0; b < K; ++b) {
            int32_t r = 0;
            std::memcpy(&r, c->h_tour_out.p + kTourOffRounds + 4 * (size_t)b, sizeof r);
            if (r < 0) return fail(c, FS_E_HIP, "a tour tree did not settle in %lld rounds", (long long)(2 * (int64_t)nodes + 2));
            rounds = std::max<int64_t>(rounds, r);
        }
    }
    c->tour_tree_builds += K;
    c->tour_tree_rounds = rounds;
    if (pair_length_m) std::memcpy(pair_length_m, c->h_tour_out.p, sizeof(double) * (size_t)m * (size_t)m);
    double res[2];
    int64_t ri[2];
    std::memcpy(res, c->h_tour_out.p + kTourOffRes, sizeof res);
    std::memcpy(ri, c->h_tour_out.p + kTourOffRes + 16, sizeof ri);
    *tour_length = res[0];
    *n_tied = ri[1];
    if (!(res[0] < pa.charge)) return FS_OK;                            // getBestFullPath false: the zero frontier
    int32_t perm[RM_TOUR_MAX_LOCAL];
    tour_unrank(ri[0], k, perm);
    for (int32_t t = 0; t < k; ++t) tour[t] = loc[(size_t)perm[t]];
    tour[k] = cg;
    *tour_size = k + 1;
    *next_index = tour[0];
    *status = FS_SAFE;
    return fi_pose7 ? tour_pose_safe(c, fi_pose7, fi_threshold, status) : FS_OK;
}

}  // extern "C"

// ================================================================== any-angle leg refinement (fs_refine.hip)
// computePathBetweenPointsThetaStar (DEP/src/Helpers.cpp:540-588) for a batch of legs: one converged cost field per distinct start
// cell — relaxed together, kept per context —, then one wave per leg for the descent, Theta*'s parent rule and the interpolation.

namespace {

int rf_check(fs_ctx *c, double w_euc, double w_trav, int32_t corners)
{
    const int rc = grid2d_check(c, "the leg refinement");
    if (rc) return rc;
    if (corners != 4 && corners != 8) return fail(c, FS_E_INVALID, "corners must be 4 or 8");
    // (w_euc > 0 makes the field's fixed point unique; the bounds keep DBL_MAX an absorbing "not reached")
    if (!(w_euc > 0.0 && w_euc <= 1e6) || !(w_trav >= 0.0 && w_trav <= 1e6)) return fail(c, FS_E_INVALID, "weights outside 0 < w_euc <= 1e6, 0 <= w_traversal <= 1e6");
    return FS_OK;
}

void rf_moves(double w_euc, double e[8])
{
    static const int m[8][2] = {{0, 1}, {0, -1}, {1, 0}, {-1, 0}, {1, -1}, {-1, 1}, {1, 1}, {-1, -1}};
    for (int i = 0; i < 8; ++i) e[i] = w_euc * std::sqrt((double)(m[i][0] * m[i][0] + m[i][1] * m[i][1]));
}

// The fields of `srcs` (at most rf_max_fields distinct start cells) in the slab: cached ones found, the others built now in one
// batch (polls the stream).  slot[i] = the slab block of srcs[i].
int rf_fields(fs_ctx *c, const fs_ctx::RfKey &base, const std::vector<int32_t> &srcs, std::vector<int32_t> &slot)
{
    const int M = c->rf_max_fields;
    const size_t ns = (size_t)c->nx * (size_t)c->ny;
    const double *before = c->d_rf_g.p;
    FS_HIP(c, c->d_rf_g.ensure((size_t)M * ns));
    if (c->rf_slab_cells != ns || (int)c->rf_key.size() != M || c->d_rf_g.p != before) {
        c->rf_key.assign(M, fs_ctx::RfKey{});
        c->rf_gen.assign(M, 0);
        c->rf_slab_cells = ns;
    }
    slot.assign(srcs.size(), -1);
    std::vector<char> used(M, 0);
    for (size_t i = 0; i < srcs.size(); ++i) {
        fs_ctx::RfKey k = base;
        k.src = srcs[i];
        for (int s = 0; s < M; ++s)
            if (!used[s] && c->rf_gen[s] == c->grid_gen && c->rf_key[s] == k) { slot[i] = s; used[s] = 1; break; }
    }
    FsRefineFieldArgs a{};
    a.n = 0;
    for (size_t i = 0; i < srcs.size(); ++i) {
        if (slot[i] >= 0) continue;
        int pick = -1;
        for (int s = 0; s < M && pick < 0; ++s) if (!used[s] && c->rf_gen[s] != c->grid_gen) pick = s;   // empty or stale first
        for (int s = 0; s < M && pick < 0; ++s) if (!used[s]) pick = s;
        if (pick < 0) return fail(c, FS_E_INVALID, "more fields than refine.max_fields in one group");
        used[pick] = 1;
        slot[i] = pick;
        a.f[a.n++] = FsRefineFieldDesc{pick, srcs[i]};
    }
    if (a.n == 0) return FS_OK;
    const int nx = c->nx, ny = c->ny;
    a.cells = c->d_cells.p; a.g = c->d_rf_g.p;
    a.nx = nx; a.ny = ny; a.tx = (nx + RF_TILE - 1) / RF_TILE; a.ty = (ny + RF_TILE - 1) / RF_TILE;
    a.allow = base.allow; a.corners = base.corners; a.w_trav = base.w_trav;
    rf_moves(base.w_euc, a.e);
    const size_t tiles = (size_t)a.tx * (size_t)a.ty;
    FS_HIP(c, c->d_rf_flags.ensure(2 * (size_t)a.n * tiles));
    FS_HIP(c, c->d_rf_any.ensure((size_t)PLAN_BATCH * a.n));
    uint32_t *flags[2] = {c->d_rf_flags.p, c->d_rf_flags.p + (size_t)a.n * tiles};
    for (int i = 0; i < a.n; ++i) c->rf_gen[a.f[i].slot] = 0;      // (until the build has finished)
    FS_HIP(c, fs_launch_refine_init(a, flags[0], c->stream));
    const auto launch = [&](int64_t r0, int count) -> int {
        for (int64_t k = 0, r = r0; k < count; ++k, ++r)
            FS_HIP(c, fs_launch_refine_round(a, flags[r & 1], flags[(r + 1) & 1], c->d_rf_any.p + (size_t)k * a.n, c->stream));
        return FS_OK;
    };
    std::vector<int64_t> rounds((size_t)a.n);
    const int rc = poll_rounds(c, c->d_rf_any.p, PLAN_BATCH_FIRST, PLAN_BATCH, a.n, PLAN_MAX_ROUNDS, "cost field", PLAN_MAX_ROUNDS, launch,
                               rounds.data());
    if (rc) return rc;
    for (int i = 0; i < a.n; ++i) {
        fs_ctx::RfKey k = base;
        k.src = a.f[i].src;
        c->rf_key[a.f[i].slot] = k;
        c->rf_gen[a.f[i].slot] = c->grid_gen;
    }
    c->rf_builds += a.n;
    c->rf_rounds = rounds[(size_t)a.n - 1];
    return FS_OK;
}

// Per-leg output columns in d_rf_out / h_rf_out: status | n_vertices | n_poses (int32) | cost (f64) | chain length | LOS walks (i64).
struct RfOutLayout {
    size_t st, nv, np, cost, chain, walks, total;
    explicit RfOutLayout(size_t n) : st(0), nv(4 * n), np(8 * n), cost((12 * n + 7) & ~(size_t)7), chain(cost + 8 * n), walks(chain + 8 * n),
                                     total(walks + 8 * n) {}
};

// ---- the REFERENCE search (fs_set_refine_search): ThetaStar::generatePath itself per distinct (start cell, goal cell), one wavefront
// per search in batches of slots, one synchronisation, then backtrace's list through linearInterpolation on the host (std::hypot of
// world differences: fs_thetastar.h).  The fields, their cache and counters 1011-1013 are not touched.
struct RsLayout {
    size_t in, st, nv, mh, cost, pops, walks, vtx, total;      // byte offsets in d_rs_io / h_rs_io
    RsLayout(size_t n, size_t vcap) : in(0), st(8 * n), nv(12 * n), mh(16 * n), cost((20 * n + 7) & ~(size_t)7), pops(cost + 8 * n),
                                      walks(pops + 8 * n), vtx(walks + 8 * n), total(vtx + 4 * n * vcap) {}
};

int rs_check(fs_ctx *c)
{
    if (c->nx > FS_THETA_MAX_SIDE || c->ny > FS_THETA_MAX_SIDE)
        return fail(c, FS_E_INVALID, "the REFERENCE refine search takes maps of at most %d cells a side (this one: %d x %d)", FS_THETA_MAX_SIDE, c->nx, c->ny);
    return FS_OK;
}

int rs_refine_paths(fs_ctx *c, int32_t n, const double *start_xy, const double *goal_xy, int32_t allow, double w_euc, double w_trav,
                    int32_t corners, int32_t *status, double *cost, int32_t *n_vertices, double *vertex_xy, int32_t *n_poses, double *pose_xy)
{
    int rc = rs_check(c);
    if (rc) return rc;
    const size_t nn = (size_t)n;
    const int nx = c->nx, ny = c->ny;
    const size_t ns = (size_t)nx * (size_t)ny;
    // refusals before any search (worldToMap of start, then goal); the distinct (start cell, goal cell) in order of first appearance
    std::vector<int32_t> pre(nn, 0), of(nn, -1), cellsv;
    std::map<std::pair<int32_t, int32_t>, int32_t> seen;
    for (size_t i = 0; i < nn; ++i) {
        int32_t sx = 0, sy = 0, gx = 0, gy = 0;
        if (!grid_world_to_map(c, start_xy[2 * i], start_xy[2 * i + 1], sx, sy)) { pre[i] = FS_REFINE_START_OFF_MAP; continue; }
        if (!grid_world_to_map(c, goal_xy[2 * i], goal_xy[2 * i + 1], gx, gy)) { pre[i] = FS_REFINE_GOAL_OFF_MAP; continue; }
        const std::pair<int32_t, int32_t> key(sy * nx + sx, gy * nx + gx);
        auto it = seen.find(key);
        if (it == seen.end()) { it = seen.emplace(key, (int32_t)(cellsv.size() / 2)).first; cellsv.push_back(key.first); cellsv.push_back(key.second); }
        of[i] = it->second;
    }
    const size_t S = cellsv.size() / 2;
    c->rs_searches = (int64_t)S; c->rs_batches = 0; c->rs_pops = 0; c->rs_walks = 0; c->rs_max_heap = 0;
    if (S > 0) {
        // the table of this grid shape, by the libm this process runs on
        if (c->rs_hyp_nx != nx || c->rs_hyp_ny != ny || !c->d_rs_hyp.p) {
            std::vector<double> hyp(ns);
            fs_theta_fill_table(hyp.data(), nx, ny);
            c->rs_hyp_nx = c->rs_hyp_ny = 0;
            FS_HIP(c, c->d_rs_hyp.ensure(ns));
            FS_HIP(c, hipMemcpyAsync(c->d_rs_hyp.p, hyp.data(), 8 * ns, hipMemcpyHostToDevice, c->stream));
            FS_HIP(c, hipStreamSynchronize(c->stream));       // (hyp is pageable and leaves scope)
            c->rs_hyp_nx = nx; c->rs_hyp_ny = ny;
        }
        const int64_t per_slot = fs_refine_search_slot_bytes((int64_t)ns);
        int64_t slots = c->rs_opt_slots > 0 ? c->rs_opt_slots : std::max<int64_t>(1, c->rs_opt_bytes / per_slot);
        slots = std::min<int64_t>(std::min<int64_t>(slots, 65535), (int64_t)S);
        FS_HIP(c, c->d_rs_slab.ensure((size_t)slots * (size_t)per_slot));
        for (int attempt = 0;; ++attempt) {
            const size_t vcap = (size_t)c->rs_vtx_cap;
            const RsLayout L(S, vcap);
            FS_HIP(c, c->d_rs_io.ensure(L.total)); FS_HIP(c, c->h_rs_io.ensure(L.total));
            std::memcpy(c->h_rs_io.p + L.in, cellsv.data(), 8 * S);
            FS_HIP(c, hipMemcpyAsync(c->d_rs_io.p + L.in, c->h_rs_io.p + L.in, 8 * S, hipMemcpyHostToDevice, c->stream));
            FsRefineSearchArgs a{};
            a.cells = c->d_cells.p; a.nx = nx; a.ny = ny; a.allow = allow ? 1 : 0; a.corners = corners; a.w_euc = w_euc; a.w_trav = w_trav;
            a.hyp = c->d_rs_hyp.p; a.slab = c->d_rs_slab.p; a.slot_bytes = per_slot;
            char *o = c->d_rs_io.p;
            a.search_in = reinterpret_cast<const int32_t *>(o + L.in);
            a.vtx_cap = (int32_t)vcap; a.vtx = reinterpret_cast<int32_t *>(o + L.vtx);
            a.status = reinterpret_cast<int32_t *>(o + L.st); a.n_vertices = reinterpret_cast<int32_t *>(o + L.nv);
            a.max_heap = reinterpret_cast<int32_t *>(o + L.mh); a.cost = reinterpret_cast<double *>(o + L.cost);
            a.pops = reinterpret_cast<int64_t *>(o + L.pops); a.walks = reinterpret_cast<int64_t *>(o + L.walks);
            c->rs_batches = ((int64_t)S + slots - 1) / slots;
            for (int64_t base = 0; base < (int64_t)S; base += slots)
                FS_HIP(c, fs_launch_refine_search_batch(a, (int32_t)base, (int32_t)std::min<int64_t>(slots, (int64_t)S - base), c->stream));
            FS_HIP(c, hipMemcpyAsync(c->h_rs_io.p + L.st, c->d_rs_io.p + L.st, L.total - L.st, hipMemcpyDeviceToHost, c->stream));
            FS_HIP(c, hipStreamSynchronize(c->stream));
            const int32_t *nv = reinterpret_cast<const int32_t *>(c->h_rs_io.p + L.nv);
            int32_t most = 0;
            for (size_t k = 0; k < S; ++k) most = std::max(most, nv[k]);
            if (most <= (int32_t)vcap) break;
            if (attempt >= 1) return fail(c, FS_E_HIP, "vertex scratch did not settle");
            c->rs_vtx_cap = most;                             // (a parent chain longer than the scratch: grown, the searches run again)
        }
    }
    const RsLayout L(S, (size_t)c->rs_vtx_cap);
    const char *h = c->h_rs_io.p;
    for (size_t k = 0; k < S; ++k) {
        c->rs_pops += reinterpret_cast<const int64_t *>(h + L.pops)[k];
        c->rs_walks += reinterpret_cast<const int64_t *>(h + L.walks)[k];
        c->rs_max_heap = std::max<int64_t>(c->rs_max_heap, reinterpret_cast<const int32_t *>(h + L.mh)[k]);
    }
    // per distinct search: the vertices' world points and the published poses, once
    std::vector<std::vector<double>> vx(S), vy(S), px(S), py(S);
    std::vector<char> done(S, 0);
    size_t vo = 0, po = 0;
    for (size_t i = 0; i < nn; ++i) {
        if (pre[i]) { status[i] = pre[i]; cost[i] = std::numeric_limits<double>::max(); n_vertices[i] = 0; n_poses[i] = 0; continue; }
        const size_t k = (size_t)of[i];
        status[i] = reinterpret_cast<const int32_t *>(h + L.st)[k];
        cost[i] = reinterpret_cast<const double *>(h + L.cost)[k];
        if (status[i] == FS_REFINE_OK && !done[k]) {
            const int32_t nv = reinterpret_cast<const int32_t *>(h + L.nv)[k];
            const int32_t *v = reinterpret_cast<const int32_t *>(h + L.vtx) + k * (size_t)c->rs_vtx_cap;
            vx[k].resize((size_t)nv); vy[k].resize((size_t)nv);
            for (int32_t j = 0; j < nv; ++j) {
                vx[k][(size_t)j] = fs_theta_map_to_world(c->origin[0], c->res, v[j] % nx);
                vy[k][(size_t)j] = fs_theta_map_to_world(c->origin[1], c->res, v[j] / nx);
            }
            fs_theta_interpolate(vx[k].data(), vy[k].data(), (size_t)nv, c->res, px[k], py[k]);
            done[k] = 1;
        }
        n_vertices[i] = (int32_t)vx[k].size();
        n_poses[i] = (int32_t)px[k].size();
        if (status[i] != FS_REFINE_OK) { n_vertices[i] = 0; n_poses[i] = 0; }
        for (int32_t j = 0; vertex_xy && j < n_vertices[i]; ++j) { vertex_xy[2 * (vo + j)] = vx[k][(size_t)j]; vertex_xy[2 * (vo + j) + 1] = vy[k][(size_t)j]; }
        for (int32_t j = 0; pose_xy && j < n_poses[i]; ++j) { pose_xy[2 * (po + j)] = px[k][(size_t)j]; pose_xy[2 * (po + j) + 1] = py[k][(size_t)j]; }
        vo += (size_t)n_vertices[i];
        po += (size_t)n_poses[i];
    }
    return FS_OK;
}

}  // namespace

extern "C" {

int fs_set_refine_search(fs_ctx *c, int32_t search)
{
    if (!c) return FS_E_INVALID;
    if (search != FS_REFINE_SEARCH_FIELD && search != FS_REFINE_SEARCH_REFERENCE) return fail(c, FS_E_INVALID, "unknown refine search %d", search);
    c->rf_search = search;
    return FS_OK;
}

int fs_refine_field(fs_ctx *c, const double start_xy[2], int32_t allow_unknown, double w_euc, double w_traversal, int32_t corners, double *g)
{
    if (!c) return FS_E_INVALID;
    if (!start_xy || !g) return fail(c, FS_E_INVALID, "null pointer");
    int rc = rf_check(c, w_euc, w_traversal, corners);
    if (rc) return rc;
    int32_t sx = 0, sy = 0;
    if (!grid_world_to_map(c, start_xy[0], start_xy[1], sx, sy)) return fail(c, FS_E_INVALID, "the start is off the costmap: no field");
    fs_ctx::RfKey base;
    base.allow = allow_unknown ? 1 : 0; base.corners = corners; base.w_euc = w_euc; base.w_trav = w_traversal;
    std::vector<int32_t> slot;
    rc = rf_fields(c, base, std::vector<int32_t>{sy * c->nx + sx}, slot);
    if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
    const size_t ns = (size_t)c->nx * (size_t)c->ny;
    FS_HIP(c, hipMemcpyAsync(g, c->d_rf_g.p + (size_t)slot[0] * ns, sizeof(double) * ns, hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipStreamSynchronize(c->stream));
    return FS_OK;
}

int fs_refine_paths(fs_ctx *c, int32_t n, const double *start_xy, const double *goal_xy, int32_t allow_unknown, double w_euc,
                    double w_traversal, int32_t corners, int32_t *status, double *cost, int32_t *n_vertices, double *vertex_xy,
                    int32_t *n_poses, double *pose_xy)
{
    if (!c) return FS_E_INVALID;
    if (n < 0 || (n > 0 && (!start_xy || !goal_xy || !status || !cost || !n_vertices || !n_poses))) return fail(c, FS_E_INVALID, "null pointer");
    int rc = rf_check(c, w_euc, w_traversal, corners);
    if (rc) return rc;
    if (n == 0) return FS_OK;
    if (c->rf_search == FS_REFINE_SEARCH_REFERENCE)
        return rs_refine_paths(c, n, start_xy, goal_xy, allow_unknown, w_euc, w_traversal, corners, status, cost, n_vertices, vertex_xy, n_poses, pose_xy);
    const size_t nn = (size_t)n;
    const int nx = c->nx, ny = c->ny, M = c->rf_max_fields;
    fs_ctx::RfKey base;
    base.allow = allow_unknown ? 1 : 0; base.corners = corners; base.w_euc = w_euc; base.w_trav = w_traversal;
    // refusals before any field (worldToMap of start, then goal), the distinct start cells in order of first appearance
    std::vector<int32_t> pre(nn, 0), scell(nn, -1), gcell(nn, -1), fld(nn, -1), srcs;
    std::map<int32_t, int32_t> seen;
    for (size_t i = 0; i < nn; ++i) {
        int32_t sx = 0, sy = 0, gx = 0, gy = 0;
        if (!grid_world_to_map(c, start_xy[2 * i], start_xy[2 * i + 1], sx, sy)) { pre[i] = FS_REFINE_START_OFF_MAP; continue; }
        if (!grid_world_to_map(c, goal_xy[2 * i], goal_xy[2 * i + 1], gx, gy)) { pre[i] = FS_REFINE_GOAL_OFF_MAP; continue; }
        scell[i] = sy * nx + sx; gcell[i] = gy * nx + gx;
        auto it = seen.find(scell[i]);
        if (it == seen.end()) { it = seen.emplace(scell[i], (int32_t)srcs.size()).first; srcs.push_back(scell[i]); }
        fld[i] = it->second;
    }
    const int n_groups = (int)((srcs.size() + M - 1) / M);
    const RfOutLayout O(nn);
    if (c->rf_chain_cap == 0) {
        c->rf_chain_cap = std::max<int64_t>(4096, 4 * ((int64_t)nx + ny));
        c->rf_vert_cap = 256;
        c->rf_pose_cap = std::max<int32_t>(1024, 2 * (nx + ny));
    }
    int64_t walks = 0;
    for (int attempt = 0; n_groups > 0; ++attempt) {
        const int64_t ccap = c->rf_chain_cap;
        const int32_t vcap = c->rf_vert_cap, pcap = c->rf_pose_cap;
        const size_t pts_bytes = 16 * nn * ((size_t)vcap + (size_t)pcap);
        // every buffer this attempt uses is sized before a pointer into any of them is taken
        FS_HIP(c, c->h_rf_in.ensure(16 * nn)); FS_HIP(c, c->d_rf_in.ensure(4 * nn));
        FS_HIP(c, c->d_rf_scratch.ensure(3 * nn * (size_t)ccap));
        FS_HIP(c, c->d_rf_out.ensure(O.total)); FS_HIP(c, c->h_rf_out.ensure(O.total));
        FS_HIP(c, c->h_rf_pts.ensure(pts_bytes));
        const bool mapped = c->h_rf_pts.dev != nullptr;
        if (!mapped) FS_HIP(c, c->d_rf_pts.ensure(pts_bytes));
        double *pts = reinterpret_cast<double *>(mapped ? c->h_rf_pts.dev : c->d_rf_pts.p);
        int32_t *in = reinterpret_cast<int32_t *>(c->h_rf_in.p);
        FsRefineLegArgs a{};
        a.cells = c->d_cells.p; a.nx = nx; a.ny = ny;
        a.ox = c->origin[0]; a.oy = c->origin[1]; a.res = c->res;
        a.allow = base.allow; a.corners = corners; a.w_euc = w_euc; a.w_trav = w_traversal;
        rf_moves(w_euc, a.e);
        a.chain = c->d_rf_scratch.p; a.par = a.chain + nn * (size_t)ccap; a.vtx = a.par + nn * (size_t)ccap; a.chain_cap = ccap;
        a.vert = pts; a.vert_cap = vcap; a.pose = pts + 2 * nn * (size_t)vcap; a.pose_cap = pcap;
        char *o = c->d_rf_out.p;
        a.status = reinterpret_cast<int32_t *>(o + O.st); a.n_vertices = reinterpret_cast<int32_t *>(o + O.nv);
        a.n_poses = reinterpret_cast<int32_t *>(o + O.np); a.cost = reinterpret_cast<double *>(o + O.cost);
        a.chain_len = reinterpret_cast<int64_t *>(o + O.chain); a.walks = reinterpret_cast<int64_t *>(o + O.walks);
        size_t nk = 0;
        for (int grp = 0; grp < n_groups; ++grp) {
            const size_t f0 = (size_t)grp * M, f1 = std::min(srcs.size(), f0 + M);
            std::vector<int32_t> slot;
            rc = rf_fields(c, base, std::vector<int32_t>(srcs.begin() + f0, srcs.begin() + f1), slot);
            if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
            a.g = c->d_rf_g.p;                                // (the slab exists only after rf_fields: the first call allocates it)
            const size_t k0 = nk;
            for (size_t i = 0; i < nn; ++i) {
                if (pre[i] || (size_t)fld[i] < f0 || (size_t)fld[i] >= f1) continue;
                in[4 * nk] = scell[i]; in[4 * nk + 1] = gcell[i]; in[4 * nk + 2] = slot[fld[i] - f0]; in[4 * nk + 3] = (int32_t)i;
                ++nk;
            }
            FS_HIP(c, hipMemcpyAsync(c->d_rf_in.p + 4 * k0, in + 4 * k0, 16 * (nk - k0), hipMemcpyHostToDevice, c->stream));
            a.leg_in = c->d_rf_in.p + 4 * k0;
            FS_HIP(c, fs_launch_refine_legs(a, (int32_t)(nk - k0), c->stream));
        }
        FS_HIP(c, hipMemcpyAsync(c->h_rf_out.p, c->d_rf_out.p, O.total, hipMemcpyDeviceToHost, c->stream));
        if (!mapped) FS_HIP(c, hipMemcpyAsync(c->h_rf_pts.p, c->d_rf_pts.p, pts_bytes, hipMemcpyDeviceToHost, c->stream));
        FS_HIP(c, hipStreamSynchronize(c->stream));
        const char *h = c->h_rf_out.p;
        const int32_t *st = reinterpret_cast<const int32_t *>(h + O.st), *nv = reinterpret_cast<const int32_t *>(h + O.nv),
                      *np = reinterpret_cast<const int32_t *>(h + O.np);
        const int64_t *cl = reinterpret_cast<const int64_t *>(h + O.chain), *wk = reinterpret_cast<const int64_t *>(h + O.walks);
        bool again = false;
        walks = 0;
        for (size_t i = 0; i < nn; ++i) {
            if (pre[i]) continue;
            if (st[i] == FS_REFINE_BROKEN) return fail(c, FS_E_HIP, "leg %zu: the descent left the cost field", i);
            if (st[i] == FS_REFINE_OVERFLOW) {
                again = true;
                c->rf_chain_cap = std::max<int64_t>(c->rf_chain_cap, cl[i]);
                c->rf_vert_cap = std::max(c->rf_vert_cap, nv[i]);
                c->rf_pose_cap = std::max(c->rf_pose_cap, np[i]);
            }
            walks += wk[i];
        }
        if (!again) break;
        if (attempt >= 3) return fail(c, FS_E_HIP, "leg scratch did not settle");
    }
    c->rf_walks += walks;
    const char *h = c->h_rf_out.p;
    const double *pts = reinterpret_cast<const double *>(c->h_rf_pts.p);
    const size_t vcap = (size_t)c->rf_vert_cap, pcap = (size_t)c->rf_pose_cap;
    size_t vo = 0, po = 0;
    for (size_t i = 0; i < nn; ++i) {
        if (pre[i]) { status[i] = pre[i]; cost[i] = std::numeric_limits<double>::max(); n_vertices[i] = 0; n_poses[i] = 0; continue; }
        status[i] = reinterpret_cast<const int32_t *>(h + O.st)[i];
        cost[i] = reinterpret_cast<const double *>(h + O.cost)[i];
        n_vertices[i] = reinterpret_cast<const int32_t *>(h + O.nv)[i];
        n_poses[i] = reinterpret_cast<const int32_t *>(h + O.np)[i];
        if (vertex_xy && n_vertices[i]) std::memcpy(vertex_xy + 2 * vo, pts + 2 * i * vcap, 16 * (size_t)n_vertices[i]);
        if (pose_xy && n_poses[i]) std::memcpy(pose_xy + 2 * po, pts + 2 * nn * vcap + 2 * i * pcap, 16 * (size_t)n_poses[i]);
        vo += (size_t)n_vertices[i];
        po += (size_t)n_poses[i];
    }
    return FS_OK;
}

}  // extern "C"

// ================================================================== multi-robot task allocation (fs_allocate.hip)
// TaskAllocator (DEPX/frontier_multirobot_allocator/taskAllocator.cpp:7-66): every robot's cost and distance rows, then MinPos and /
// or Munkres, in one launch of one workgroup; and the fleet call, which builds those rows on the device — arrival information scored
// once for the list, one shortest-path tree per distinct start node, one plan launch over R x n, U1 per robot — and solves on them
// where they lie.

namespace {

// the packed result of a solve at the head of d_al_out / d_fl_out
struct AllocHeader {
    double total;
    double assigned[FS_ALLOC_MAX_ROBOTS];
    int32_t assignment[FS_ALLOC_MAX_ROBOTS];
    int32_t status, err, pad[2];
};
constexpr size_t kAllocHeader = 1024;
static_assert(sizeof(AllocHeader) <= kAllocHeader, "the header block holds the header");

int alloc_check(fs_ctx *c, int32_t R, int32_t n, int32_t method)
{
    if (R < 1 || R > FS_ALLOC_MAX_ROBOTS) return fail(c, FS_E_INVALID, "n_robots must be 1..%d", FS_ALLOC_MAX_ROBOTS);
    if (n < 1 || n > FS_ALLOC_MAX_TASKS) return fail(c, FS_E_INVALID, "n_tasks must be 1..%d", FS_ALLOC_MAX_TASKS);
    if (method != FS_ALLOC_HUNGARIAN && method != FS_ALLOC_MINPOS) return fail(c, FS_E_INVALID, "unknown allocation method %d", method);
    return FS_OK;
}

// The solve on device matrices, on the stream, not waited for.  d_modified may be nullptr (MINPOS then keeps its matrix in the
// context's scratch); d_assigned may be nullptr.  The counters of the solve stay in d_al_stats until fs_get_counter asks.
int alloc_enqueue(fs_ctx *c, int32_t R, int32_t n, const double *d_cost, const double *d_distance, int32_t method, int32_t *d_assignment,
                  double *d_total, double *d_assigned, int32_t *d_rank, double *d_modified, int32_t *d_status)
{
    const size_t rn = (size_t)R * (size_t)n;
    const bool minpos = method == FS_ALLOC_MINPOS;
    FS_HIP(c, c->d_al_work.ensure(8 * rn * ((minpos && !d_modified) ? 2 : 1)));
    if (!c->d_al_stats.p) {
        FS_HIP(c, c->d_al_stats.ensure(4));
        FS_HIP(c, hipMemsetAsync(c->d_al_stats.p, 0, 4 * sizeof(int32_t), c->stream));
    }
    FsAllocArgs a{};
    a.n_robots = R; a.n_tasks = n; a.method = method;
    a.cost = d_cost; a.distance = minpos ? d_distance : nullptr;
    a.rank = minpos ? d_rank : nullptr;
    a.work = reinterpret_cast<double *>(c->d_al_work.p);
    a.modified = !minpos ? nullptr : d_modified ? d_modified : a.work + rn;
    a.assignment = d_assignment; a.total_cost = d_total; a.assigned_cost = d_assigned;
    a.status = d_status; a.stats = c->d_al_stats.p + 1;
    FS_HIP(c, fs_launch_allocate(a, c->stream));
    return FS_OK;
}

int alloc_status(fs_ctx *c, int32_t status, int32_t R, int32_t n)
{
    if (status == FS_E_INVALID) return fail(c, FS_E_INVALID, "a cost or distance entry is NaN, infinite or negative");
    if (status == FS_E_RANGE)
        return fail(c, FS_E_RANGE, "step 5 ran more than (%d + 1) * (%d + 1) times", (int)R, (int)std::min(R, n));
    if (status != FS_OK) return fail(c, FS_E_HIP, "the allocator returned status %d", (int)status);
    return FS_OK;
}

}  // namespace

extern "C" {

int fs_allocate_tasks_dev(fs_ctx *c, int32_t n_robots, int32_t n_tasks, const double *d_cost, const double *d_distance, int32_t method,
                          int32_t *d_assignment, double *d_total_cost, int32_t *d_rank, double *d_modified_cost, int32_t *d_status)
{
    if (!c) return FS_E_INVALID;
    const int rc = alloc_check(c, n_robots, n_tasks, method);
    if (rc) return rc;
    if (!d_cost || !d_assignment || !d_total_cost || !d_status) return fail(c, FS_E_INVALID, "null device pointer");
    if (method == FS_ALLOC_MINPOS && !d_distance) return fail(c, FS_E_INVALID, "FS_ALLOC_MINPOS needs the distance matrix");
    FS_HIP(c, hipSetDevice(c->device));
    return alloc_enqueue(c, n_robots, n_tasks, d_cost, d_distance, method, d_assignment, d_total_cost, nullptr, d_rank, d_modified_cost, d_status);
}

int fs_allocate_tasks(fs_ctx *c, int32_t n_robots, int32_t n_tasks, const double *cost, const double *distance, int32_t method,
                      int32_t *assignment, double *total_cost, int32_t *rank, double *modified_cost)
{
    if (!c) return FS_E_INVALID;
    int rc = alloc_check(c, n_robots, n_tasks, method);
    if (rc) return rc;
    if (!cost || !assignment || !total_cost) return fail(c, FS_E_INVALID, "null pointer");
    const bool minpos = method == FS_ALLOC_MINPOS;
    if (minpos && !distance) return fail(c, FS_E_INVALID, "FS_ALLOC_MINPOS needs the distance matrix");
    FS_HIP(c, hipSetDevice(c->device));
    const size_t R = (size_t)n_robots, rn = R * (size_t)n_tasks;
    // in: cost | distance;  out: header | MinPos' matrix | MinPos' P
    const size_t total_in = 8 * rn * (minpos ? 2 : 1), o_mod = kAllocHeader, o_rank = o_mod + 8 * rn, total_out = o_rank + 4 * rn;
    const bool want_matrices = minpos && (rank || modified_cost);
    FS_HIP(c, c->h_al_in.ensure(total_in)); FS_HIP(c, c->d_al_in.ensure(total_in));
    FS_HIP(c, c->h_al_out.ensure(total_out)); FS_HIP(c, c->d_al_out.ensure(total_out));
    std::memcpy(c->h_al_in.p, cost, 8 * rn);
    if (minpos) std::memcpy(c->h_al_in.p + 8 * rn, distance, 8 * rn);
    FS_HIP(c, hipMemcpyAsync(c->d_al_in.p, c->h_al_in.p, total_in, hipMemcpyHostToDevice, c->stream));
    AllocHeader *dh = reinterpret_cast<AllocHeader *>(c->d_al_out.p);
    rc = alloc_enqueue(c, n_robots, n_tasks, reinterpret_cast<const double *>(c->d_al_in.p), reinterpret_cast<const double *>(c->d_al_in.p + 8 * rn),
                       method, dh->assignment, &dh->total, nullptr, reinterpret_cast<int32_t *>(c->d_al_out.p + o_rank),
                       reinterpret_cast<double *>(c->d_al_out.p + o_mod), &dh->status);
    if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
    FS_HIP(c, hipMemcpyAsync(c->h_al_out.p, c->d_al_out.p, want_matrices ? total_out : kAllocHeader, hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipStreamSynchronize(c->stream));
    const AllocHeader *h = reinterpret_cast<const AllocHeader *>(c->h_al_out.p);
    rc = alloc_status(c, h->status, n_robots, n_tasks);
    if (rc) return rc;
    std::memcpy(assignment, h->assignment, 4 * R);
    *total_cost = h->total;
    if (minpos && rank) std::memcpy(rank, c->h_al_out.p + o_rank, 4 * rn);
    if (minpos && modified_cost) std::memcpy(modified_cost, c->h_al_out.p + o_mod, 8 * rn);
    return FS_OK;
}

int fs_fleet_allocate_roadmap(fs_ctx *c, int32_t n_robots, const double *robot_pose7, int32_t n, const double *goal_xyz,
                              const int32_t *frontier_size, const uint8_t *blacklisted, double alpha, double beta, double max_vx, double max_wz,
                              int32_t method, int32_t *assignment, double *total_cost, double *assigned_cost, fs_record *records,
                              double *weighted_cost, double *path_length_m, uint8_t *achievable)
{
    if (!c) return FS_E_INVALID;
    int rc = alloc_check(c, n_robots, n, method);
    if (rc) return rc;
    if (!robot_pose7 || !goal_xyz || !assignment || !total_cost || !assigned_cost) return fail(c, FS_E_INVALID, "null pointer");
    FS_HIP(c, hipSetDevice(c->device));
    rc = check_scoring_state(c, true, false);
    if (rc) return rc;
    const int32_t R = n_robots, nodes = rm_nodes(c);
    const size_t nn = (size_t)n, rn = (size_t)R * nn, pad_n = (nn + 15) & ~(size_t)15, pad_rn = (rn + 15) & ~(size_t)15, nnodes = (size_t)nodes;
    const bool reference = c->rm_search == FS_ROADMAP_SEARCH_REFERENCE;
    // in: goal xy | headings [R][n] | plan descriptors [R] | goal xyz | frontier size | blacklist | modes [R][n]
    const size_t i_goal2 = 0, i_head = i_goal2 + 16 * nn, i_desc = i_head + 8 * rn, i_goal3 = (i_desc + sizeof(FsRmPlanArgs) * (size_t)R + 15) & ~(size_t)15;
    const size_t i_fsize = i_goal3 + 24 * nn, i_black = (i_fsize + 4 * nn + 15) & ~(size_t)15, i_mode = i_black + pad_n, total_in = i_mode + pad_rn;
    // out: header | records | cost [R][n] | length in m [R][n] | achievable [R][n];  scratch: path length | heading, [R][n] each
    const size_t o_rec = kAllocHeader, o_cost = o_rec + sizeof(fs_record) * nn, o_lenm = o_cost + 8 * rn, o_ach = o_lenm + 8 * rn, total_out = o_ach + pad_rn;
    FS_HIP(c, c->h_fl_in.ensure(total_in)); FS_HIP(c, c->d_fl_in.ensure(total_in));
    FS_HIP(c, c->h_fl_out.ensure(total_out)); FS_HIP(c, c->d_fl_out.ensure(total_out)); FS_HIP(c, c->d_fl_plan.ensure(16 * rn));
    char *h = c->h_fl_in.p;
    double *goal2 = reinterpret_cast<double *>(h + i_goal2), *head = reinterpret_cast<double *>(h + i_head);
    uint8_t *mode = reinterpret_cast<uint8_t *>(h + i_mode);
    std::memcpy(h + i_goal3, goal_xyz, 24 * nn);
    if (frontier_size) std::memcpy(h + i_fsize, frontier_size, 4 * nn); else std::memset(h + i_fsize, 0, 4 * nn);
    if (blacklisted) std::memcpy(h + i_black, blacklisted, nn); else std::memset(h + i_black, 0, nn);
    // every robot's start node, modes and headings as roadmap_plan_enqueue takes them (the xy copy of the goals is the same for
    // every robot); a tree per distinct start node that a robot with a goal to search stands at
    std::vector<int32_t> root((size_t)R), tree((size_t)R, -1), roots;
    for (int32_t r = 0; r < R; ++r) {
        const double *pose = robot_pose7 + 7 * (size_t)r;
        const bool need_tree = rm_stage_goals(pose, nn, goal_xyz, nullptr, goal2, mode + (size_t)r * nn, head + (size_t)r * nn);
        root[(size_t)r] = fs_rm_closest(c->rm_xy.data(), c->rm_key.data(), nodes, c->rm_cell, pose[0], pose[1]);
        if (reference || !need_tree || root[(size_t)r] < 0) continue;
        size_t b = 0;
        while (b < roots.size() && roots[b] != root[(size_t)r]) ++b;
        if (b == roots.size()) roots.push_back(root[(size_t)r]);
        tree[(size_t)r] = (int32_t)b;
    }
    const int32_t K = (int32_t)roots.size();
    char *din = c->d_fl_in.p, *dout = c->d_fl_out.p;
    double *d_len = reinterpret_cast<double *>(c->d_fl_plan.p), *d_head = d_len + rn;
    double *d_cost = reinterpret_cast<double *>(dout + o_cost), *d_lenm = reinterpret_cast<double *>(dout + o_lenm);
    uint8_t *d_ach = reinterpret_cast<uint8_t *>(dout + o_ach);
    if (K > 0) {
        rc = rm_device_graph(c);
        if (rc) return rc;
        FS_HIP(c, c->d_fl_d.ensure(2 * nnodes * K)); FS_HIP(c, c->d_fl_hops.ensure(2 * nnodes * K)); FS_HIP(c, c->d_fl_pred.ensure(2 * nnodes * K));
        FS_HIP(c, c->d_fl_word.ensure((size_t)std::max<int32_t>(PLAN_BATCH, FS_ALLOC_MAX_ROBOTS)));
    }
    FsRmPlanArgs *desc = reinterpret_cast<FsRmPlanArgs *>(h + i_desc);
    for (int32_t r = 0; r < R; ++r) {
        FsRmPlanArgs a{};
        const size_t o = (size_t)r * nn;
        a.n_nodes = nodes; a.xy = c->d_rm_xy.p; a.key = c->d_rm_key.p; a.cell = c->rm_cell; a.root = root[(size_t)r];
        if (tree[(size_t)r] >= 0) {       // (after its quiet round both buffers of a tree hold it: buffer 0 is read)
            a.d = c->d_fl_d.p + 2 * nnodes * (size_t)tree[(size_t)r];
            a.pred = c->d_fl_pred.p + 2 * nnodes * (size_t)tree[(size_t)r];
        }
        a.n = n;
        a.goal = reinterpret_cast<const double *>(din + i_goal2);
        a.heading_in = reinterpret_cast<const double *>(din + i_head) + o;
        a.mode = reinterpret_cast<const uint8_t *>(din + i_mode) + o;
        a.path_length = d_len + o; a.path_length_m = d_lenm + o; a.path_heading = d_head + o; a.achievable = d_ach + o;
        desc[r] = a;
    }
    FS_HIP(c, hipMemcpyAsync(din, h, total_in, hipMemcpyHostToDevice, c->stream));
    // ---- the plans
    bool block_route = false;
    if (reference) {
        // the A* queries robot by robot through the single-robot path (its buffers are one robot's), each settled before the next;
        // the four columns move into the robot's rows on the device
        const PlanOutLayout O(nn);
        for (int32_t r = 0; r < R; ++r) {
            const size_t o = (size_t)r * nn;
            rc = roadmap_plan_enqueue(c, robot_pose7 + 7 * (size_t)r, n, goal_xyz, nullptr);
            if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
            FS_HIP(c, hipStreamSynchronize(c->stream));
            bool redone = false;
            rc = rm_astar_settle(c, [&] { return roadmap_astar_cols(c); }, &redone);
            if (rc) return rc;
            const char *src = c->d_rm_out.p;
            FS_HIP(c, hipMemcpyAsync(d_len + o, src + O.len, 8 * nn, hipMemcpyDeviceToDevice, c->stream));
            FS_HIP(c, hipMemcpyAsync(d_lenm + o, src + O.len_m, 8 * nn, hipMemcpyDeviceToDevice, c->stream));
            FS_HIP(c, hipMemcpyAsync(d_head + o, src + O.head, 8 * nn, hipMemcpyDeviceToDevice, c->stream));
            FS_HIP(c, hipMemcpyAsync(d_ach + o, src + O.ach, nn, hipMemcpyDeviceToDevice, c->stream));
        }
    } else {
        // the trees, with the fleet's own buffers (the single-robot tree cache is neither read nor replaced)
        bool polled = false;
        int64_t rounds = 0;
        rc = rm_trees_enqueue(c, c->d_fl_d, c->d_fl_hops, c->d_fl_pred, c->d_fl_word, roots.data(), K, "the fleet's trees", &polled, &rounds);
        if (rc) return rc;
        block_route = !polled;
        FS_HIP(c, fs_launch_rm_fleet_plan(reinterpret_cast<const FsRmPlanArgs *>(din + i_desc), R, n, c->stream));
    }
    // ---- arrival information, once for the list (achievable_in = all), then every robot's U1 row and the solve where the rows lie
    AllocHeader *dh = reinterpret_cast<AllocHeader *>(dout);
    const uint8_t *d_black = reinterpret_cast<const uint8_t *>(din + i_black);
    fs_record *d_rec = reinterpret_cast<fs_record *>(dout + o_rec);
    rc = arrival_records_dev(c, n, reinterpret_cast<const double *>(din + i_goal3), reinterpret_cast<const int32_t *>(din + i_fsize), d_black,
                             nullptr, d_rec);
    if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
    FS_HIP(c, hipMemsetAsync(&dh->err, 0, sizeof(int32_t), c->stream));
    FS_HIP(c, fs_launch_fleet_costs(R, n, d_rec, d_black, d_ach, d_len, d_head, alpha, beta, max_vx, max_wz, c->max_gt, d_cost, &dh->err, c->stream));
    rc = alloc_enqueue(c, R, n, d_cost, d_lenm, method, dh->assignment, &dh->total, dh->assigned, nullptr, nullptr, &dh->status);
    if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
    // one transfer out: the header, the records behind it if asked for, the matrices behind those if asked for
    const size_t bytes_out = (weighted_cost || path_length_m || achievable) ? total_out : records ? o_cost : kAllocHeader;
    FS_HIP(c, hipMemcpyAsync(c->h_fl_out.p, dout, bytes_out, hipMemcpyDeviceToHost, c->stream));
    int32_t rounds_h[FS_ALLOC_MAX_ROBOTS];
    if (block_route && K > 0) FS_HIP(c, hipMemcpyAsync(rounds_h, c->d_fl_word.p, sizeof(int32_t) * (size_t)K, hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipStreamSynchronize(c->stream));
    if (block_route)
        for (int32_t b = 0; b < K; ++b)
            if (rounds_h[b] < 0) return fail(c, FS_E_HIP, "a tree of the fleet did not settle in %lld rounds", (long long)(2 * (int64_t)nodes + 2));
    const char *ho = c->h_fl_out.p;
    const AllocHeader *hh = reinterpret_cast<const AllocHeader *>(ho);
    if (hh->err) return fail(c, FS_E_RANGE, "utility outside [0,1] (the reference throws: FrontierCostsManager.cpp:148-149,173-174)");
    rc = alloc_status(c, hh->status, R, n);
    if (rc) return rc;
    std::memcpy(assignment, hh->assignment, 4 * (size_t)R);
    std::memcpy(assigned_cost, hh->assigned, 8 * (size_t)R);
    *total_cost = hh->total;
    if (records) std::memcpy(records, ho + o_rec, sizeof(fs_record) * nn);
    if (weighted_cost) std::memcpy(weighted_cost, ho + o_cost, 8 * rn);
    if (path_length_m) std::memcpy(path_length_m, ho + o_lenm, 8 * rn);
    if (achievable) std::memcpy(achievable, ho + o_ach, rn);
    return FS_OK;
}

}  // extern "C"

// ------------------------------------------------------------------ keep-out zones (fs_keepout.hip)

namespace {

// A new zone: stored; on a staged 2-D grid rasterised, painted and counted on its bounding box, and the class image re-cut
// for the bricks of that box.  Cached arrival limits stay (as for fs_update_grid_region: the fan does not depend on the cells).
int ko_add(fs_ctx *c, int32_t kind, double wx, double wy, double yaw, double size_m, int32_t *zone_id, int64_t *n_cells)
{
    if (!c) return FS_E_INVALID;
    FS_HIP(c, hipSetDevice(c->device));
    if (!std::isfinite(wx) || !std::isfinite(wy) || !std::isfinite(yaw) || !std::isfinite(size_m) || !(size_m >= 0.0))
        return fail(c, FS_E_INVALID, "a keep-out zone needs a finite position and yaw and a finite size >= 0");
    if (c->have_grid && c->nz != 1) return fail(c, FS_E_INVALID, "keep-out zones are defined on a 2-D costmap (nz == 1)");
    uint32_t size_cells = 0;
    if (c->have_grid && !fs_ko_size_in_cells(size_m, c->res, &size_cells))
        return fail(c, FS_E_INVALID, "the zone's size is 2^31 cells or more (the reference's conversion to unsigned int is undefined)");
    if (c->ko_zones.size() >= (size_t)FS_KEEPOUT_MAX_ZONES) return fail(c, FS_E_INVALID, "at most %d keep-out zones per context", FS_KEEPOUT_MAX_ZONES);
    c->ko_zones.push_back(KoZone{kind, wx, wy, yaw, size_m, 0});
    const size_t id = c->ko_zones.size() - 1;
    if (c->have_grid) {
        const KoGeom g{c->nx, c->ny, c->origin[0], c->origin[1], c->res};
        int32_t box[4];
        const int rc = c->ko_mask_valid ? ko_rasterise(c, id, g, box) : ko_rebuild(c, g, box);
        if (rc) { c->ko_zones.pop_back(); c->ko_mask_valid = false; return rc; }
        if (box[2] >= box[0]) {
            if (const int rc2 = cells_changed_in_box(c, box[0], box[1], 0, box[2] - box[0] + 1, box[3] - box[1] + 1, 1)) return rc2;
            ++c->grid_gen;
            ++c->epoch;
        }
    }
    if (zone_id) *zone_id = (int32_t)id;
    if (n_cells) *n_cells = c->ko_zones[id].n_cells;
    return FS_OK;
}

}  // namespace

extern "C" {

int fs_keepout_add_fov(fs_ctx *c, double wx, double wy, double yaw, double height_m, int32_t *zone_id, int64_t *n_cells)
{
    return ko_add(c, FS_KO_FOV, wx, wy, yaw, height_m, zone_id, n_cells);
}

int fs_keepout_add_disc(fs_ctx *c, double wx, double wy, double radius_m, int32_t *zone_id, int64_t *n_cells)
{
    return ko_add(c, FS_KO_DISC, wx, wy, 0.0, radius_m, zone_id, n_cells);
}

int fs_keepout_clear(fs_ctx *c)
{
    if (!c) return FS_E_INVALID;
    c->ko_zones.clear();
    c->ko_mask_valid = false;
    return FS_OK;
}

int fs_keepout_get(fs_ctx *c, int32_t *n_zones, double *spec, int64_t *n_cells, uint8_t *mask)
{
    if (!c || !n_zones) return FS_E_INVALID;
    FS_HIP(c, hipSetDevice(c->device));
    *n_zones = (int32_t)c->ko_zones.size();
    for (size_t k = 0; k < c->ko_zones.size(); ++k) {
        const KoZone &z = c->ko_zones[k];
        if (spec) { spec[5 * k] = (double)z.kind; spec[5 * k + 1] = z.wx; spec[5 * k + 2] = z.wy; spec[5 * k + 3] = z.yaw; spec[5 * k + 4] = z.size; }
        if (n_cells) n_cells[k] = z.n_cells;
    }
    if (mask) {
        if (!c->have_grid) return fail(c, FS_E_STATE, "fs_upload_grid has not been called");
        const size_t cells = (size_t)c->nx * (size_t)c->ny;
        if (c->ko_mask_valid) {
            FS_HIP(c, hipMemcpyAsync(mask, c->d_ko_mask.p, cells, hipMemcpyDeviceToHost, c->stream));
            FS_HIP(c, hipStreamSynchronize(c->stream));
        } else {
            std::memset(mask, 0, cells);
        }
    }
    return FS_OK;
}

// MarkLethalFOV::tick (FisherInfoBTPlugin.cpp:148-182) with blacklistFrontier (:93-103); `float` as there
int fs_mark_lethal_fov(fs_ctx *c, const double robot_pose7[7], double blacklist_pose7[7], int32_t *zone_id, int64_t *n_cells)
{
    if (!c || !robot_pose7) return FS_E_INVALID;
    for (int i = 0; i < 7; ++i)
        if (!std::isfinite(robot_pose7[i])) return fail(c, FS_E_INVALID, "the robot pose must be finite");
    const double robotYaw = yaw_of_quaternion(robot_pose7 + 3);                                  // :158
    if (!std::isfinite(robotYaw)) return fail(c, FS_E_INVALID, "the robot pose has no yaw (zero quaternion)");
    const float blacklist_x = (float)(robot_pose7[0] + (2.5 * std::cos(robotYaw)));               // :159-160
    const float blacklist_y = (float)(robot_pose7[1] + (2.5 * std::sin(robotYaw)));
    const float blacklist_x_fov = (float)(robot_pose7[0] + (0.8 * std::cos(robotYaw)));           // :162-163
    const float blacklist_y_fov = (float)(robot_pose7[1] + (0.8 * std::sin(robotYaw)));
    // addNewMarkedAreaFOV(req->lethal_point.x, req->lethal_point.y, req->yaw, 3.5)  (keepout_layer.cpp:174)
    const int rc = ko_add(c, FS_KO_FOV, (double)blacklist_x_fov, (double)blacklist_y_fov, robotYaw, 3.5, zone_id, n_cells);
    if (rc) return rc;
    if (blacklist_pose7) {
        blacklist_pose7[0] = (double)blacklist_x + (1.7 * std::cos(robotYaw));                   // :96-98; the goal point's z is 0
        blacklist_pose7[1] = (double)blacklist_y + (1.7 * std::sin(robotYaw));
        blacklist_pose7[2] = 0.0;
        // eulerToQuat(0, 0, robotYaw + M_PI): tf2's setRPY with roll = pitch = 0, then normalize() (GeometryUtils.hpp:49-61)
        const double half = (robotYaw + M_PI) * 0.5, z = std::sin(half), w = std::cos(half);
        const double inv = 1.0 / std::sqrt(z * z + w * w);
        blacklist_pose7[3] = 0.0; blacklist_pose7[4] = 0.0; blacklist_pose7[5] = z * inv; blacklist_pose7[6] = w * inv;
    }
    return FS_OK;
}

// fs_update_grid_region's mirror: the window is gathered into a packed buffer on the device, copied to page-locked memory in
// one transfer and laid out with the caller's strides
int fs_read_grid_region(fs_ctx *c, int32_t x0, int32_t y0, int32_t z0, int32_t sx, int32_t sy, int32_t sz,
                        uint8_t *cells, int64_t row_stride, int64_t slice_stride)
{
    if (!c) return FS_E_INVALID;
    if (const int rc = grid_check(c)) return rc;
    bool empty = true;
    if (const int rc = window_check(c, x0, y0, z0, sx, sy, sz, cells, row_stride, slice_stride, empty)) return rc;
    if (empty) return FS_OK;
    const size_t total = (size_t)sx * (size_t)sy * (size_t)sz;
    FS_HIP(c, c->h_win.ensure(total));
    FS_HIP(c, c->d_win.ensure(total));
    FS_HIP(c, fs_launch_window_gather(c->d_cells.p, c->d_win.p, c->nx, c->ny, x0, y0, z0, sx, sy, sz, c->stream));
    FS_HIP(c, hipMemcpyAsync(c->h_win.p, c->d_win.p, total, hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipStreamSynchronize(c->stream));
    for (int32_t z = 0; z < sz; ++z)
        for (int32_t y = 0; y < sy; ++y)
            std::memcpy(cells + (size_t)z * (size_t)slice_stride + (size_t)y * (size_t)row_stride, c->h_win.p + ((size_t)z * sy + y) * sx, (size_t)sx);
    if (c->h_win.cap > ((size_t)64 << 20)) { c->h_win.release(); c->d_win.release(); }   // (a window of map size: not worth keeping)
    return FS_OK;
}

}  // extern "C"

// ------------------------------------------------------------------ inflation layer (fs_inflate.hip)

namespace {

// What both entry points refuse about the parameters and the staged grid, in fs_inflate's order; R = the seeds' reach in cells
int infl_check(fs_ctx *c, const fs_inflation_params *p, int32_t &R)
{
    if (const int rc = grid_check(c)) return rc;
    if (c->nz != 1) return fail(c, FS_E_INVALID, "the inflation layer is defined on a 2-D costmap (nz == 1)");
    if (!std::isfinite(p->inflation_radius) || !std::isfinite(p->inscribed_radius) || !std::isfinite(p->cost_scaling_factor) ||
        !(p->inflation_radius >= 0.0) || !(p->inscribed_radius >= 0.0) || !(p->cost_scaling_factor >= 0.0))
        return fail(c, FS_E_INVALID, "the inflation layer needs finite radii and a finite scaling factor, all >= 0");
    R = fs_inflation_cell_radius(p->inflation_radius, c->res);
    if (R < 0) return fail(c, FS_E_INVALID, "an inflation radius of more than %d cells", FS_INFLATE_MAX_CELLS);
    return FS_OK;
}

// The cost table of (p, the staged resolution) on the device: one of those kept, or filled on the host and uploaded into a free
// slot — the oldest one's once all are used
int infl_table(fs_ctx *c, const fs_inflation_params *p, int32_t R, const uint8_t *&d_cost)
{
    for (const InflTable &t : c->infl_tables)
        if (t.inflation_radius == p->inflation_radius && t.inscribed_radius == p->inscribed_radius &&
            t.cost_scaling_factor == p->cost_scaling_factor && t.res == c->res) { d_cost = t.d_cost.p; return FS_OK; }
    size_t slot = c->infl_tables.size();
    if (slot < (size_t)FS_INFL_TABLES) c->infl_tables.emplace_back();
    else slot = c->infl_next++ % FS_INFL_TABLES;
    InflTable &t = c->infl_tables[slot];
    t.res = 0.0;                                                  // (no key matches it until it is whole)
    const size_t n = (size_t)R * (size_t)R + 1;
    std::vector<uint8_t> cost(n);
    fs_inflation_cost_table(*p, c->res, R, cost.data());
    FS_HIP(c, t.d_cost.ensure(n));
    FS_HIP(c, hipMemcpyAsync(t.d_cost.p, cost.data(), n, hipMemcpyHostToDevice, c->stream));
    FS_HIP(c, hipStreamSynchronize(c->stream));                  // (the host copy is this function's)
    t.inflation_radius = p->inflation_radius; t.inscribed_radius = p->inscribed_radius; t.cost_scaling_factor = p->cost_scaling_factor;
    t.R = R; t.res = c->res;
    d_cost = t.d_cost.p;
    return FS_OK;
}

}  // namespace

extern "C" {

int fs_inflation_costs(const fs_ctx *ctx, const fs_inflation_params *p, int32_t *cell_radius, uint8_t *cost_by_d2)
{
    fs_ctx *c = const_cast<fs_ctx *>(ctx);                        // (the error text is the context's)
    if (!c || !p || !cell_radius) return FS_E_INVALID;
    int32_t R = 0;
    if (const int rc = infl_check(c, p, R)) return rc;
    *cell_radius = R;
    if (cost_by_d2) fs_inflation_cost_table(*p, c->res, R, cost_by_d2);
    return FS_OK;
}

// The rows pass, the columns pass and what follows every write of cells (cells_changed_in_box; the keep-out zones need no
// repaint: max(253, cost) is 253) on the stream back to back, one wait at the end for the two counters
int fs_inflate(fs_ctx *c, const fs_inflation_params *p, int32_t x0, int32_t y0, int32_t sx, int32_t sy, int64_t *n_seeds, int64_t *n_changed)
{
    if (!c || !p) return FS_E_INVALID;
    int32_t R = 0;
    if (const int rc = infl_check(c, p, R)) return rc;
    if (sx < 0 || sy < 0) return fail(c, FS_E_INVALID, "negative window size");
    if (x0 < 0 || y0 < 0 || (int64_t)x0 + sx > c->nx || (int64_t)y0 + sy > c->ny)
        return fail(c, FS_E_INVALID, "window [%d,%lld) x [%d,%lld) leaves the %d x %d grid", x0, (long long)x0 + sx, y0, (long long)y0 + sy, c->nx, c->ny);
    if (n_seeds) *n_seeds = 0;
    if (n_changed) *n_changed = 0;
    if (sx == 0 || sy == 0 || R == 0) return FS_OK;
    const uint8_t *d_cost = nullptr;
    if (const int rc = infl_table(c, p, R, d_cost)) return rc;
    const FsInflateBox b = fs_inflate_box(c->nx, c->ny, x0, y0, sx, sy, R);
    FS_HIP(c, c->d_infl_g.ensure((size_t)b.gh * (size_t)sx));
    FS_HIP(c, c->d_infl_counts.ensure(2));
    ++c->grid_gen;
    FS_HIP(c, hipMemsetAsync(c->d_infl_counts.p, 0, 2 * sizeof(unsigned long long), c->stream));
    FS_HIP(c, fs_launch_inflate_rows(c->d_cells.p, c->nx, c->ny, x0, y0, sx, sy, R, c->d_infl_g.p, c->d_infl_counts.p, c->stream));
    FS_HIP(c, fs_launch_inflate_cols(c->d_infl_g.p, d_cost, c->d_cells.p, c->nx, c->ny, x0, y0, sx, sy, R, p->inflate_unknown != 0,
                                     c->d_infl_counts.p + 1, c->stream));
    if (const int rc = cells_changed_in_box(c, x0, y0, 0, sx, sy, 1)) return rc;
    unsigned long long counts[2] = {0ull, 0ull};
    FS_HIP(c, hipMemcpyAsync(counts, c->d_infl_counts.p, sizeof counts, hipMemcpyDeviceToHost, c->stream));
    FS_HIP(c, hipStreamSynchronize(c->stream));                  // (the counts are the two passes')
    if (c->d_infl_g.cap * sizeof(uint16_t) > ((size_t)64 << 20)) c->d_infl_g.release();   // (row distances of a map-sized window: not worth keeping)
    ++c->epoch;
    if (n_seeds) *n_seeds = (int64_t)counts[0];
    if (n_changed) *n_changed = (int64_t)counts[1];
    return FS_OK;
}

}  // extern "C"

// ------------------------------------------------------------------ information layer (fs_infolayer.hip)

extern "C" {

// Anchors, compaction, THE mid-call synchronisation for n_scored (it sizes the scoring launches), then per batch of poses the
// records, fs_score_fim's launch sequence and the values' copy, then reduce / cost / store and what follows every write of cells
// (cells_changed_in_box; keep-out cells are not writable, so no repaint), one wait at the end: two synchronisations.
int fs_information_layer(fs_ctx *c, const fs_info_layer_params *p, int32_t x0, int32_t y0, int32_t sx, int32_t sy, float *info,
                         int32_t *anchor_cell, float *info_per_yaw, double *quat_zw, int64_t *n_scored, int64_t *n_changed)
{
    if (!c || !p) return FS_E_INVALID;
    int rc = grid2d_check(c, "the information layer");
    if (rc) return rc;
    if (p->stride_cells < 1 || p->stride_cells > FS_INFO_LAYER_MAX_STRIDE) return fail(c, FS_E_INVALID, "stride_cells must be 1 .. %d", FS_INFO_LAYER_MAX_STRIDE);
    if (p->n_yaw < 1 || p->n_yaw > FS_INFO_LAYER_MAX_YAW) return fail(c, FS_E_INVALID, "n_yaw must be 1 .. %d", FS_INFO_LAYER_MAX_YAW);
    if (!std::isfinite(p->yaw0) || !std::isfinite(p->pose_z)) return fail(c, FS_E_INVALID, "yaw0 and pose_z must be finite");
    if (p->reduce != FS_INFO_REDUCE_MIN && p->reduce != FS_INFO_REDUCE_MEAN && p->reduce != FS_INFO_REDUCE_MAX) return fail(c, FS_E_INVALID, "unknown reduction %d", p->reduce);
    if (!std::isfinite(p->info_lo) || !std::isfinite(p->info_hi) || !(p->info_hi > p->info_lo) || !std::isfinite(p->info_hi - p->info_lo))
        return fail(c, FS_E_INVALID, "info_lo and info_hi must be finite with info_hi > info_lo");
    if (p->max_cost < 1 || p->max_cost > 252) return fail(c, FS_E_INVALID, "max_cost must be 1 .. 252");
    if (sx < 0 || sy < 0) return fail(c, FS_E_INVALID, "negative window size");
    if (x0 < 0 || y0 < 0 || (int64_t)x0 + sx > c->nx || (int64_t)y0 + sy > c->ny)
        return fail(c, FS_E_INVALID, "window [%d,%lld) x [%d,%lld) leaves the %d x %d grid", x0, (long long)x0 + sx, y0, (long long)y0 + sy, c->nx, c->ny);
    rc = check_scoring_state(c, false, true);
    if (rc) return rc;
    if (n_scored) *n_scored = 0;
    if (n_changed) *n_changed = 0;
    const int K = p->n_yaw;
    c->il_quat.resize(2 * (size_t)K);
    for (int k = 0; k < K; ++k) {
        const double psi = p->yaw0 + (double)k * (2.0 * M_PI / (double)K);
        c->il_quat[2 * k] = std::sin(psi / 2.0); c->il_quat[2 * k + 1] = std::cos(psi / 2.0);
    }
    if (quat_zw) std::memcpy(quat_zw, c->il_quat.data(), sizeof(double) * 2 * (size_t)K);
    if (sx == 0 || sy == 0) return FS_OK;
    const int s = p->stride_cells;
    const int32_t nbx = (sx + s - 1) / s, nby = (sy + s - 1) / s;
    const size_t nb = (size_t)nbx * (size_t)nby;
    const bool want_yaw = info_per_yaw != nullptr;
    const size_t temp_bytes = fs_infolayer_temp_bytes((int64_t)nb, c->stream);
    if (temp_bytes == 0) return fail(c, FS_E_HIP, "rocPRIM refused the size query");
    FS_HIP(c, c->d_il_temp.ensure(temp_bytes));
    FS_HIP(c, c->d_il_idx.ensure(4 * nb + 2));
    FS_HIP(c, c->d_il_quat.ensure(2 * (size_t)FS_INFO_LAYER_MAX_YAW));
    FS_HIP(c, c->d_il_out.ensure(nb * (want_yaw ? (size_t)K + 1 : 1)));
    FS_HIP(c, c->d_il_count.ensure(1));
    FsInfoLayerArgs a{};
    a.cells = c->d_cells.p; a.nx = c->nx; a.ny = c->ny;
    a.ox = c->origin[0]; a.oy = c->origin[1]; a.res = c->res;
    a.x0 = x0; a.y0 = y0; a.sx = sx; a.sy = sy; a.s = s; a.nbx = nbx; a.nby = nby;
    a.K = K; a.reduce = p->reduce; a.max_cost = p->max_cost; a.write = p->write != 0;
    a.pose_z = p->pose_z; a.info_lo = p->info_lo; a.info_hi = p->info_hi;
    a.quat_zw = c->d_il_quat.p;
    a.anchor = c->d_il_idx.p; a.flag = a.anchor + nb; a.rank = a.flag + nb + 1; a.list = a.rank + nb + 1;
    a.info = c->d_il_out.p; a.per_yaw = want_yaw ? c->d_il_out.p + nb : nullptr;
    a.n_changed = c->d_il_count.p;
    a.temp = c->d_il_temp.p; a.temp_bytes = c->d_il_temp.cap;
    // (an error after the first launch waits for the stream: the next call may grow what the launches still use)
    const auto stop = [&](int code) { (void)hipStreamSynchronize(c->stream); return code; };
#define IL_HIP(call)                                                                                                  \
    do {                                                                                                              \
        const hipError_t e__ = (call);                                                                                \
        if (e__ != hipSuccess) return stop(fail(c, FS_E_HIP, "%s: %s", #call, hipGetErrorString(e__)));               \
    } while (0)
    IL_HIP(hipMemcpyAsync(c->d_il_quat.p, c->il_quat.data(), sizeof(double) * 2 * (size_t)K, hipMemcpyHostToDevice, c->stream));
    if (fs_launch_infolayer_anchors(a, c->stream) != hipSuccess) return stop(fail(c, FS_E_HIP, "information layer anchors: launch failed"));
    int32_t scored32 = 0;
    IL_HIP(hipMemcpyAsync(&scored32, a.rank + nb, sizeof scored32, hipMemcpyDeviceToHost, c->stream));
    IL_HIP(hipStreamSynchronize(c->stream));                  // THE mid-call synchronisation: n_scored sizes the scoring launches
    const int64_t total = (int64_t)scored32 * K;
    if (total > 0) {
        const int64_t batch = std::min<int64_t>(c->opt_il_batch, total);
        IL_HIP(c->d_il_val.ensure((size_t)total));
        IL_HIP(c->d_il_rt.ensure(12 * (size_t)batch));
        a.val = c->d_il_val.p;
        for (int64_t p0 = 0; p0 < total; p0 += batch) {
            const int64_t n = std::min(batch, total - p0);
            if (fs_launch_infolayer_records(a, p0, n, c->d_il_rt.p, c->stream) != hipSuccess) return stop(fail(c, FS_E_HIP, "information layer records: launch failed"));
            const float *values = nullptr;
            rc = score_records(c, c->d_il_rt.p, n, false, stop, &values);
            if (rc) return stop(rc);
            IL_HIP(hipMemcpyAsync(a.val + p0, values, sizeof(float) * (size_t)n, hipMemcpyDeviceToDevice, c->stream));
        }
    }
    const bool writes = a.write && total > 0;
    if (writes) ++c->grid_gen;
    IL_HIP(hipMemsetAsync(c->d_il_count.p, 0, sizeof(unsigned long long), c->stream));
    if (fs_launch_infolayer_store(a, c->stream) != hipSuccess) return stop(fail(c, FS_E_HIP, "information layer store: launch failed"));
    if (writes && (rc = cells_changed_in_box(c, x0, y0, 0, sx, sy, 1))) return stop(rc);
    unsigned long long changed = 0ull;
    IL_HIP(hipMemcpyAsync(&changed, c->d_il_count.p, sizeof changed, hipMemcpyDeviceToHost, c->stream));
    if (info) IL_HIP(hipMemcpyAsync(info, a.info, sizeof(float) * nb, hipMemcpyDeviceToHost, c->stream));
    if (anchor_cell) IL_HIP(hipMemcpyAsync(anchor_cell, a.anchor, sizeof(int32_t) * nb, hipMemcpyDeviceToHost, c->stream));
    if (want_yaw) IL_HIP(hipMemcpyAsync(info_per_yaw, a.per_yaw, sizeof(float) * nb * (size_t)K, hipMemcpyDeviceToHost, c->stream));
    IL_HIP(hipStreamSynchronize(c->stream));
#undef IL_HIP
    // (the values of a map-sized lattice at stride 1: not worth keeping)
    if (c->d_il_val.cap * sizeof(float) > ((size_t)64 << 20)) c->d_il_val.release();
    if (c->d_il_out.cap * sizeof(float) > ((size_t)64 << 20)) c->d_il_out.release();
    if (writes) ++c->epoch;
    if (n_scored) *n_scored = scored32;
    if (n_changed) *n_changed = (int64_t)changed;
    return FS_OK;
}

}  // extern "C"
