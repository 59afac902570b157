/*
 * fitslam_frontier.h — C ABI of the MI355X-native frontier-scoring path.
 *
 * This is the drop-in boundary for ONE hot path of suchetanrs/FIT-SLAM: per-candidate arrival
 * information (ray fan through the occupancy grid, unknown-cell counts, FOV window max, best yaw)
 * and landmark Fisher information (voxel-lookup scalar with crowding discount + 6x6 FIM).
 * Plain pointers and sizes only; no C++ / torch / ROS types.  Every entry point cites the reference
 * interface it replaces.  Abbreviations (under the FIT-SLAM tree):
 *   DEP/ = dev_ws/src/DEPRECATED/frontier_exploration/frontier_exploration/
 *   FIP/ = dev_ws/src/fit-slam2/fisher_information_plugins/
 *
 * Conventions
 *   - every function returns FS_OK (0) or a negative FS_E_* code and never throws; the message of
 *     the last failure on a context is available from fs_last_error().
 *   - a context is single-caller (externally synchronised), owns one HIP stream (or borrows the
 *     one passed at creation) and owns device copies of grid, landmarks and lookup table.
 *     DIFFERENT contexts may be used from different host threads at the same time.
 *     Host buffers stay caller-owned; nothing is allocated across the ABI.
 *   - grid layout [nz][ny][nx] uint8, index = (z*ny + y)*nx + x; nz == 1 is the reference's
 *     nav2_costmap_2d::Costmap2D (cost constants: 255 unknown, 254 lethal, 253 inscribed, 0 free).
 *   - there is NO CPU fallback: if the HIP runtime or a gfx950 device is missing, fs_ctx_create
 *     fails with FS_E_NO_DEVICE.
 */
#ifndef FITSLAM_FRONTIER_H_
#define FITSLAM_FRONTIER_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FS_ABI_VERSION 1

/* return codes */
#define FS_OK            0
#define FS_E_INVALID    -1   /* bad argument / parameters (e.g. fewer rays than the FOV window) */
#define FS_E_NO_DEVICE  -2   /* HIP runtime or device unavailable — no CPU fallback exists */
#define FS_E_HIP        -3   /* a HIP call failed */
#define FS_E_STATE      -4   /* call order: grid / landmarks / table / params not set yet */
#define FS_E_IO         -5   /* lookup-table file could not be read or written */
#define FS_E_RANGE      -6   /* utility outside [0,1] (the reference throws, FrontierCostsManager.cpp:148-149,173-174) */

/* per-candidate status (records.flags bits 8..15, status[] of fs_score_arrival) */
#define FS_STATUS_OK          0
#define FS_STATUS_OFF_MAP     1   /* a worldToMap failed: arrival 0, yaw 0 (DEP/src/CostCalculator.cpp:50-55) */
#define FS_STATUS_BLACKLISTED 2   /* DEP/src/FrontierCostsManager.cpp:77-86 */

#define FS_MAX_ELEV 16

typedef struct fs_ctx fs_ctx;

/* Replaces FrontierCostCalculator's constructor parameters (DEP/src/CostCalculator.cpp:5-21:
 * costCalculator/max_camera_depth, delta_theta, camera_fov, Costmap2DROS::getRobotRadius()),
 * the RayTracedCells ranges of DEP/src/CostCalculator.cpp:40, the limits factors of :186-188
 * (a parameter in fit-slam2: fit_slam2/params/active_slam_exploration_params.yaml:17) and
 * CostAssigner's polygon bbox (DEP/src/CostAssigner.cpp:148-165). */
typedef struct {
    double max_camera_depth;     /* 2.0  */
    double delta_theta;          /* 0.10 */
    double camera_fov;           /* 1.04 */
    double robot_radius;         /* 0.60 */
    int32_t n_rays;              /* 0: the reference loop `theta <= 2*pi` (63 rays at 0.10); >0: exactly n yaw rays */
    int32_t n_elev;              /* elevation rings of the 3-D extension; 1 with elev[0] == 0 is the reference */
    double elev[FS_MAX_ELEV];    /* radians */
    int32_t obst_min, obst_max;  /* 240, 254 */
    int32_t trace_min, trace_max;/* 255, 255 */
    double factor_max;           /* 1.2  */
    double factor_min;           /* 0.70 */
    double polygon[4];           /* minx, miny, maxx, maxy */
} fs_ray_params;

/* Replaces the GetLandmarksInView request fields (FIP/src/fisher_information/FisherInfoManager.cpp:60-65)
 * by an explicit visibility predicate (DESIGN.md "Visibility"). */
typedef struct {
    double max_dist;             /* 14.0; must be positive and below 1e9 m */
    double max_angle;            /* 1.0 rad from the camera +x axis; >= pi disables the cone */
} fs_fim_params;

/* Fixed-size per-candidate result record (the unit of the multi-GPU all-gather). 32 bytes. */
typedef struct {
    int32_t arrival;             /* Frontier::setArrivalInformation (DEP/src/CostCalculator.cpp:112) */
    int32_t argmax;              /* maxIndex of the FOV window (:98-107) */
    float   yaw;                 /* goal orientation, maxIndex*delta_theta + fov/2 (:119) */
    float   info_ref;            /* isPoseSafe's `information` (FIP/src/.../FisherInfoManager.cpp:100) */
    float   trace;               /* trace of the unit-weight 6x6 FIM over the visible landmarks */
    float   logdet;              /* log det of that FIM (D-optimality); -inf if singular */
    int32_t n_visible;           /* landmarks passing the visibility predicate */
    uint32_t flags;              /* bit0 achievable; bits 8..15 status; bits 16..31 min(n_voxels, 65535) */
} fs_record;

#define FS_FLAG_ACHIEVABLE 1u
#define FS_RECORD_STATUS(flags)   (((flags) >> 8) & 0xffu)
#define FS_RECORD_NVOXELS(flags)  (((flags) >> 16) & 0xffffu)

/* ---------------------------------------------------------------- context */

/* device_id: HIP device ordinal.  stream: a hipStream_t to borrow (e.g. the caller's current
 * stream) or NULL to create one owned by the context. */
int  fs_ctx_create(int device_id, void *stream, fs_ctx **out);
void fs_ctx_destroy(fs_ctx *ctx);
const char *fs_last_error(const fs_ctx *ctx);
int  fs_abi_version(void);
int  fs_synchronize(fs_ctx *ctx);

/* (per-kernel timing, device counters, tuning knobs and the fp64 self test — development and measurement aids that have no
 * counterpart in the reference — are declared in fitslam_frontier_dev.h) */

/* ---------------------------------------------------------------- arrival information (ray-cast) */

/* Replaces FrontierCostCalculator::FrontierCostCalculator (DEP/src/CostCalculator.cpp:5-21). */
int fs_set_ray_params(fs_ctx *ctx, const fs_ray_params *p);
/* number of yaw rays / FOV window the parameters produce (DEP/src/CostCalculator.cpp:36,87) */
int fs_ray_fan_shape(const fs_ctx *ctx, int32_t *n_yaw, int32_t *n_elev, int32_t *window);

/* Replaces the raw `nav2_costmap_2d::Costmap2D *exploration_costmap_` the scorer holds
 * (DEP/src/CostCalculator.cpp:10).  Copies the grid to HBM — the snapshot point; call it under the
 * costmap mutex.  Invalidates cached arrival limits. */
int fs_upload_grid(fs_ctx *ctx, const uint8_t *cells, int32_t nx, int32_t ny, int32_t nz,
                   const double origin_xyz[3], double resolution);

/* Same snapshot from a SPARSE map: n_bricks bricks of 8x8x8 cells (brick_xyz [n][3] in brick units, brick_cells
 * [n][512] with index (z*8 + y)*8 + x), everything else default_value (255 = unknown).  This is the wire format of
 * a hashed voxel map (BASELINE.json configs[4], 1024^3); in HBM the grid stays dense (1 GiB of 288 GB) so that the
 * ray walk needs no hash probe per cell.  Dimensions must be multiples of 8. */
int fs_upload_grid_bricks(fs_ctx *ctx, int32_t nx, int32_t ny, int32_t nz, const double origin_xyz[3], double resolution,
                          uint8_t default_value, int64_t n_bricks, const int32_t *brick_xyz, const uint8_t *brick_cells);

/* A WINDOW of the staged map rewritten in place — what a costmap update cycle does to the master grid: every layer's
 * `updateCosts(master_grid, min_i, min_j, max_i, max_j)` writes inside the cycle's bounds through `getCharMap()` (the costmap
 * is a rolling / bounded-update one, fit_slam2/params/active_slam_nav2_params.yaml:124) — with ONE exception among the
 * reference's own layers: LethalMarker::updateCosts ignores min_i..max_j and writes every cell of every keep-out zone on every
 * cycle (DEP/src/nav2_plugins/lethal_marker.cpp:305-325, fit_slam2_nav2_plugins/plugins/keepout_layer.cpp:279-300).  A zone
 * outside the window is therefore on the host's master grid and not in the window: forward the zone itself (fs_keepout_add_fov
 * below), and this call paints the stored zones again inside the window it wrote.  The window is cells
 * [x0, x0+sx) x [y0, y0+sy) x [z0, z0+sz) of the grid fs_upload_grid staged (same shape, origin and resolution: a map that
 * moved or was resized is a new snapshot).  `cells` points at the window's first cell, x fastest; row_stride / slice_stride are
 * the byte distances between its rows / z slices — pass `getCharMap() + y0 * size_x + x0` with row_stride = size_x to send a
 * window of the live costmap without packing it; 0 = tightly packed (sx, sx * sy).  Images derived from the grid are updated
 * for the bricks the window touches only; cached arrival limits stay (setMaxArrivalInformation's fan does not depend on the
 * cells, DEP/src/CostCalculator.cpp:123-191).  Scoring afterwards equals scoring after fs_upload_grid of the whole rewritten
 * map, bit for bit.  An empty window is a no-op; one that leaves the grid is refused (FS_E_INVALID), nothing written. */
int fs_update_grid_region(fs_ctx *ctx, int32_t x0, int32_t y0, int32_t z0, int32_t sx, int32_t sy, int32_t sz,
                          const uint8_t *cells, int64_t row_stride, int64_t slice_stride);

/* The window [x0, x0+sx) x [y0, y0+sy) x [z0, z0+sz) of the staged grid copied back to the host: the mirror of
 * fs_update_grid_region (same window rules and strides; 2-D and 3-D grids).  What `getCharMap()` shows of the master grid after
 * a cycle; nothing on the device changes. */
int fs_read_grid_region(fs_ctx *ctx, int32_t x0, int32_t y0, int32_t z0, int32_t sx, int32_t sy, int32_t sz,
                        uint8_t *cells, int64_t row_stride, int64_t slice_stride);

/* ---------------------------------------------------------------- keep-out zones (costmap layer LethalMarker)
 *
 * Replaces the costmap layer fit_slam2_nav2_plugins::LethalMarker (fit_slam2_nav2_plugins/plugins/keepout_layer.cpp) on the
 * staged 2-D grid (nz == 1).  The context stores every zone as its REQUEST (zone_specs_) and rasterises it exactly as the layer
 * does: a fan of lines from the apex cell to 20 sampled base cells (getPointsInIsoscelesTriangle :74-126) or to 360 cells of a
 * circle (getPointsInSemiCircle, DEP/src/nav2_plugins/lethal_marker.cpp:51-72), each walked with rayTraceGeneric (:13-41) —
 * NOT a filled shape: the cells between the rays stay as they are.  Every cell of every zone holds cost 253 (markCells
 * :212-218) after each staging call, as after each cycle of the layer (updateCosts :279-300): fs_upload_grid and
 * fs_upload_grid_bricks paint all zones into the new snapshot, fs_update_grid_region paints them again inside its window.  A
 * snapshot with another shape, origin or resolution re-rasterises the stored requests first (matchSize :184-199).
 * Deviations, both deliberate: (1) matchSize's loop pushes onto zone_specs_ while iterating it (undefined behaviour, duplicate
 * zones where it survives) — here one request stays one zone; (2) the reference's master grid is re-derived every cycle, the
 * staged grid is not: fs_keepout_clear forgets the zones but CANNOT restore the cells they painted — stage the map again.
 * With no zone stored, every staging call does exactly what it does without this layer.
 *   - a zone added before any grid is staged is stored and painted by the first snapshot
 *   - a zone whose apex is off the map is stored with *n_cells = 0 (worldToMap fails: the early return :205-206) and gets its
 *     cells when a later snapshot contains the apex
 *   - non-finite arguments, a negative size, or a size of 2^31 cells or more (the reference's conversion to `unsigned int` is
 *     undefined) are refused with FS_E_INVALID, nothing stored; so is a new zone while a 3-D grid (nz > 1) is staged
 *   - a 3-D snapshot with zones stored is staged unmarked: the zones are kept and report n_cells = 0
 *   - at most FS_KEEPOUT_MAX_ZONES zones per context; one more is refused with FS_E_INVALID
 * zone_id (index in the order of the requests) and n_cells (DISTINCT cells the zone marks on the staged map) may be NULL. */
#define FS_KEEPOUT_MAX_ZONES 1024
/* Replaces LethalMarker::addNewMarkedAreaFOV(center_wx, center_wy, angleYaw, height) (keepout_layer.cpp:201-210), the body of
 * the `mark_lethal_zone` service (:171-176, which passes height 3.5). */
int fs_keepout_add_fov(fs_ctx *ctx, double wx, double wy, double yaw, double height_m, int32_t *zone_id, int64_t *n_cells);
/* Replaces LethalMarker::addNewMarkedArea(center_wx, center_wy, radius) of the older layer
 * (DEP/src/nav2_plugins/lethal_marker.cpp:218-226; its service :193-198). */
int fs_keepout_add_disc(fs_ctx *ctx, double wx, double wy, double radius_m, int32_t *zone_id, int64_t *n_cells);
/* Forgets every zone (the reference has no counterpart short of re-creating the layer).  Cells already painted stay 253. */
int fs_keepout_clear(fs_ctx *ctx);
/* The layer's state: *n_zones; spec [n][5] = kind (0 FOV, 1 disc), wx, wy, yaw, size [m] (zone_specs_); n_cells [n]; mask
 * [ny][nx] = 1 where any zone marks the staged map (the union of latest_cells_to_mark_index_; all 0 on a 3-D grid).  spec,
 * n_cells and mask may be NULL; arrays of FS_KEEPOUT_MAX_ZONES entries always suffice. */
int fs_keepout_get(fs_ctx *ctx, int32_t *n_zones, double *spec, int64_t *n_cells, uint8_t *mask);
/* Replaces MarkLethalFOV::tick (fisher_information_plugins/src/fisher_information/FisherInfoBTPlugin.cpp:148-182) without the
 * service round trip: yaw of robot_pose7 (x, y, z, qx, qy, qz, qw); a FOV zone of height 3.5 m with its apex 0.8 m ahead of the
 * robot, the apex rounded to `float` as there (:162-163); blacklist_pose7 (may be NULL) = the pose blacklistFrontier (:93-103)
 * appends to `posearray_blacklisted_region`: the point 2.5 m ahead (rounded to float, :159-160) moved 1.7 m further along the
 * yaw, z = 0, orientation yaw + pi about Z.  Publishing it is the caller's job. */
int fs_mark_lethal_fov(fs_ctx *ctx, const double robot_pose7[7], double blacklist_pose7[7], int32_t *zone_id, int64_t *n_cells);

/* ---------------------------------------------------------------- inflation layer (nav2_costmap_2d::InflationLayer)
 *
 * The costmap layer every planner of the reference reads through: its global costmap stacks static_layer, inflation_layer
 * (inflation_radius 5.0, cost_scaling_factor 0.6), lethal_marker_global_costmap and lethal_inflation_layer (radius 0.3) at
 * resolution 0.05 with robot_radius 0.05 (fit_slam2/params/active_slam_nav2_params.yaml:153-170).  nav2's InflationLayer is
 * third-party and not under the reference tree, so the behaviour is stated here, after ROS 2 Humble's
 * InflationLayer::computeCost and the write rule of InflationLayer::updateCosts.  fs_inflate inflates the staged 2-D grid
 * (nz == 1) IN PLACE inside the window [x0, x0+sx) x [y0, y0+sy):
 *   R     = (int)max(0.0, ceil(inflation_radius / resolution))                       (Costmap2D::cellDistance)
 *   seeds = the cells equal to 254 (LETHAL_OBSTACLE) of the window grown by R on every side and clipped to the map; unknown
 *           cells (255) are never seeds (inflate_around_unknown is not built)
 *   d2    = for a cell of the window, the smallest dx^2 + dy^2 to a seed, in integers; no seed with d2 <= R^2: untouched
 *   cost  = 254 for d2 == 0; else with d = sqrt((double)d2) * resolution: 253 where d <= inscribed_radius, else
 *           (unsigned char)(252 * exp(-1.0 * cost_scaling_factor * (d - inscribed_radius)))       (computeCost, in double)
 *   write = old == 255 and (inflate_unknown ? cost > 0 : cost >= 253): the cost; every other cell: max(old, cost)
 * The costs are a table indexed by d2 that the HOST fills with its own libm (fs_inflation_costs returns it) and uploads once per
 * distinct (parameters, resolution); the device works in integers only.
 * ONE deliberate deviation: Humble propagates with a distance-ordered brushfire over 4-neighbours that carries each cell's
 * source seed, so a cell whose nearest seed cannot reach it through a 4-connected chain of cells that adopted that same seed
 * gets the distance to another seed.  Here every cell gets its EXACT nearest seed — independent of order, the same for a window
 * as for the whole map, and never a cost below the brushfire's (DESIGN.md 4.26 has the measured count of cells that differ).
 *   - idempotent: costs are <= 253 and never become seeds
 *   - it cannot LOWER a cost: a wall that vanished keeps its band until its cells are rewritten — stage the raw map again
 *     (the limit of fs_keepout_clear); keep-out cells stay 253 by the write rule; two calls with different radii compose by max,
 *     as the reference's two inflation layers do
 *   - cells outside the window are never written (Humble restricts its writes to the cycle's bounds in the same way)
 *   - refused with FS_E_INVALID, nothing written: non-finite or negative radii or scaling factor, R > FS_INFLATE_MAX_CELLS, a
 *     window that leaves the grid, a 3-D grid staged; no grid staged: FS_E_STATE
 *   - an empty window or R == 0 is a no-op that reports zeros
 * n_seeds (seeds in the grown, clipped window) and n_changed (window cells whose byte changed) may be NULL.  Images derived from
 * the grid follow as after fs_update_grid_region, cached arrival limits stay: scoring, planning and searching afterwards equal
 * the same calls after fs_upload_grid of the inflated map, bit for bit. */
#define FS_INFLATE_MAX_CELLS 512
typedef struct fs_inflation_params {
    double inflation_radius, inscribed_radius, cost_scaling_factor;   /* [m], [m], [1/m] */
    int32_t inflate_unknown, reserved;
} fs_inflation_params;
int fs_inflate(fs_ctx *ctx, const fs_inflation_params *p, int32_t x0, int32_t y0, int32_t sx, int32_t sy,
               int64_t *n_seeds, int64_t *n_changed);
/* *cell_radius = R and cost_by_d2 [R * R + 1] (may be NULL: ask for R first) = the cost table fs_inflate would use on the grid
 * staged now; the refusals of fs_inflate that concern the parameters and the grid. */
int fs_inflation_costs(const fs_ctx *ctx, const fs_inflation_params *p, int32_t *cell_radius, uint8_t *cost_by_d2);

/* ---------------------------------------------------------------- information layer (this project's own extension)
 *
 * Traversability costs that know where SLAM keeps tracking: the Fisher information of a lattice of poses, as costs of the
 * staged 2-D grid, BEFORE the plan.  The reference has no such layer — its answer to a path that drops below isPoseSafe's
 * threshold is to blacklist the goal and paint a keep-out zone afterwards (MarkLethalFOV) — so the rule is stated here and is
 * normative.  On the staged 2-D grid (nz == 1), inside the window [x0, x0+sx) x [y0, y0+sy):
 *   1 blocks  with s = stride_cells, block (i, j) covers the cells x in [x0 + i*s, min(x0 + (i+1)*s, x0 + sx)), y likewise; the
 *             field has nbx = ceil(sx / s) by nby = ceil(sy / s) blocks; the centre cell is cx = min(x0 + i*s + s/2, x0 + sx - 1)
 *             in integers, cy likewise
 *   2 anchor  a cell is WRITABLE when its cost is <= 252 (known, neither inscribed nor lethal); the anchor of a block is its
 *             writable cell with the smallest dx^2 + dy^2 to the centre cell, ties to the smaller y, then the smaller x; a block
 *             without a writable cell is not scored: its info is NaN, its anchor -1, nothing in it is written
 *   3 poses   for every scored block and every k < K = n_yaw: position = the anchor's cell centre, origin + (cell + 0.5) * res in
 *             double, at height pose_z; orientation (0, 0, sin(psi_k / 2), cos(psi_k / 2)), psi_k = yaw0 + k * (2 pi / K)
 *             evaluated on the HOST in double with its libm (quat_zw returns the K pairs; the device calls no trigonometric
 *             function); the pose record is made as fs_score_fim makes it of that pose7
 *   4 value   fs_score_fim's info_ref at that pose under the context's cloud, table and fs_set_fim_params, through the info-only
 *             worker; with fs_set_occlusion enabled through the occluded worker, as fs_plan_paths_information chooses — its launch
 *             sequence WITHOUT the pose split (a pose is never spread over several workgroups: the split's slab count follows the
 *             number of poses in a launch, and a value must not depend on the batch it fell into)
 *   5 reduce  per block over k in order: FS_INFO_REDUCE_MIN / _MAX the float minimum / maximum; _MEAN the fp64 sum in k order,
 *             divided by K, rounded once to float
 *   6 cost    t = (info_hi - (double)v) / (info_hi - info_lo); if !(t > 0) t = 0; if t > 1 t = 1;
 *             cost = (unsigned char)(max_cost * t) — one multiply in double, then truncation; correctly rounded fp64 operations,
 *             no fused multiply-add: the same expression on the host from the returned float gives the same byte
 *   7 store   (write != 0) every writable cell of a scored block becomes max(old, cost); nothing else is written — not unknown
 *             cells, not cells at 253 and above, not cells outside the window, not cells of unscored blocks
 * Like fs_inflate the layer cannot LOWER a cost: stage the raw map again to remove it.  Applied after fs_inflate it composes by
 * max, as nav2's updateWithMax layers do.  After a write the images derived from the grid follow as after fs_update_grid_region;
 * cached arrival limits stay.
 * Outputs, each may be NULL: info [nby][nbx] (NaN: unscored), anchor_cell [nby][nbx] (y * nx + x, or -1), info_per_yaw
 * [K][nby][nbx] (NaN: unscored), quat_zw [K][2] (the uploaded sin, cos pairs), n_scored (scored blocks), n_changed (cells whose
 * byte changed).
 *   - FS_E_INVALID, nothing written: a parameter outside the ranges below or not finite, info_hi <= info_lo, a window that
 *     leaves the grid or has a negative size, a 3-D grid staged; FS_E_STATE: no grid staged; then what fs_score_fim refuses
 *     (no cloud, no table), with its codes
 *   - an empty window, or one without a writable cell, reports zeros (info NaN, anchors -1) and launches no scorer
 *   - poses are scored in batches of fs_set_option("infolayer.batch", n) (default 65536) so the per-pose scratch stays bounded;
 *     no pose's launch sequence depends on the batch size (poses are never split over workgroups here); what remains is the FIM
 *     worker's own call-to-call variation in the last bits of its float sums, here as in two fs_score_fim calls
 *   - TWO synchronisations: one to learn n_scored (it sizes the scoring launches), one at the end */
#define FS_INFO_LAYER_MAX_STRIDE 32
#define FS_INFO_LAYER_MAX_YAW 64
#define FS_INFO_REDUCE_MIN 0
#define FS_INFO_REDUCE_MEAN 1
#define FS_INFO_REDUCE_MAX 2
typedef struct fs_info_layer_params {
    int32_t stride_cells;       /* 1 .. FS_INFO_LAYER_MAX_STRIDE */
    int32_t n_yaw;              /* K, 1 .. FS_INFO_LAYER_MAX_YAW */
    double  yaw0;               /* heading k is yaw0 + k * (2*pi / K), evaluated on the host in double */
    double  pose_z;             /* camera height of every pose */
    int32_t reduce;             /* FS_INFO_REDUCE_MIN | _MEAN | _MAX over the K headings */
    double  info_lo, info_hi;   /* finite, info_hi > info_lo */
    int32_t max_cost;           /* 1 .. 252 */
    int32_t write;              /* 0: compute and return the field only, the grid is not touched */
} fs_info_layer_params;
int fs_information_layer(fs_ctx *ctx, const fs_info_layer_params *p, int32_t x0, int32_t y0, int32_t sx, int32_t sy,
                         float *info, int32_t *anchor_cell, float *info_per_yaw, double *quat_zw, int64_t *n_scored, int64_t *n_changed);

/* Frontier-cell predicate of FrontierSearch::isNewFrontierCell (DEP/src/FrontierSearch.cpp:218-249; isFree / isLethal /
 * isUnknown: DEP/include/.../FrontierSearch.hpp:129-142; frontierSearch/lethal_threshold 160) evaluated for every cell
 * of the staged grid, slice by slice: unknown cell, no lethal in-plane 4-neighbour, at least one free one.
 * mask [nz][ny][nx] (1 = frontier cell) may be NULL; *count = number of frontier cells.  The BFS clustering of the
 * reference (searchFrom / buildNewFrontier) consumes this mask on the host. */
int fs_frontier_cells(fs_ctx *ctx, int32_t lethal_threshold, uint8_t *mask, int64_t *count);

/* Frontier detection + clustering (second half).  Replaces, for a 2-D costmap (nz == 1),
 * std::vector<FrontierPtr> FrontierSearch::searchFrom(geometry_msgs::msg::Point position) (DEP/include/.../FrontierSearch.hpp:62,
 * DEP/src/FrontierSearch.cpp:21-96) with buildNewFrontier (:98-216), nearestFreeCell (DEP/src/Helpers.cpp:285-329) and
 * isNewFrontierCell (:218-249): the frontier cells the search collects — the 8-connected components of the frontier-cell
 * set that touch the region the outer search expands from the robot (cost < 254, within max_frontier_distance +
 * max_frontier_cluster_size * resolution * 1.414) — as clusters.
 *   labels   [ny][nx] or NULL: -1, or the cluster's label = the smallest cell index (y * nx + x) of its component
 *   clusters [max_clusters], ascending label; *n_clusters = clusters found (may exceed max_clusters: the first ones by label are
 *            stored); *n_cells = frontier cells found = every_frontier_list.size() of the reference
 * The reference then cuts a component into pieces of max_frontier_cluster_size + 1 cells in the order of its queue and takes
 * an angular median as each piece's goal point (:146-205): order-dependent steps that stay with the caller; a component of
 * `size` cells yields size / (max + 1) full pieces and, if size % (max + 1) > min_frontier_cluster_size, one more.
 * A robot position off the map gives no cluster (:28-33). */
typedef struct {
    int32_t label;               /* smallest cell index of the component */
    int32_t size;                /* cells in the component */
    double  centroid_x, centroid_y;   /* mean of the cell centres (mapToWorld), world frame */
    int32_t min_x, min_y, max_x, max_y;   /* bounding box in cells */
} fs_frontier_cluster;
int fs_frontier_clusters(fs_ctx *ctx, const double robot_xy[2], int32_t lethal_threshold, double max_frontier_distance,
                         int32_t max_frontier_cluster_size, int32_t *labels, int32_t max_clusters,
                         fs_frontier_cluster *clusters, int32_t *n_clusters, int64_t *n_cells);

/* The whole of FrontierSearch::searchFrom on the device: fs_frontier_clusters' components, then what
 * buildNewFrontier (:98-216) does with each — a breadth-first walk from a seed cell in nhood8 order, pieces of
 * max_frontier_cluster_size + 1 cells in the order of that queue, the remainder if it exceeds min_frontier_cluster_size, per piece
 * the angular-median goal point (getCentroidOfCells, SortByMedianFunctor, libstdc++'s std::sort, the middle element) — and
 * searchFrom's size filter.  The label image never leaves the device.
 *   seeds     NULL (n_seeds ignored): the context's seed order (fs_set_frontier_seed_order).  FS_SEEDS_NEAREST (the default):
 *             per component (ascending label) its cell nearest the robot's cell, squared cell distance, ties to the smaller index.
 *             FS_SEEDS_REFERENCE: searchFrom's own outer search (:44-94) on the device, so the records equal the reference's list,
 *             order, seeds and goal points included.  Otherwise n_seeds cells (y * nx + x), each starting one buildNewFrontier,
 *             records in list order, whatever the seed order: the reference's own order when the seeds are the cells its outer
 *             search met first.  A seed that is not a frontier cell the search found, or a second seed in one component:
 *             FS_E_INVALID, nothing written.
 *   records   [max_records]; *n_records = records found (may exceed max_records: the first ones are stored)
 *   every_xy  [max_every][2] or NULL: every_frontier_list, the world coordinates of every collected cell in emission order (cells of
 *             dropped pieces included); *n_cells = its length (may exceed max_every)
 * min_frontier_cluster_size >= 0 and max_frontier_cluster_size >= 1 (any value up to INT32_MAX: one at or above nx * ny cuts no
 * component).  A robot position off the map gives no records.  The call
 * synchronises once when every_xy is NULL and at most 1024 records are stored; the goal's UID (generateUID) is the caller's. */
typedef struct {
    double  goal_x, goal_y;      /* the goal point (mapToWorld of the median cell) */
    int32_t size;                /* Frontier::getSize(): cells of the piece */
    int32_t label;               /* the component's label (as fs_frontier_clusters) */
    int32_t goal_cell;           /* y * nx + x of the goal point */
    int32_t seed_cell;           /* the seed of the buildNewFrontier call that made the piece */
} fs_frontier_record;
int fs_search_frontiers(fs_ctx *ctx, const double robot_xy[2], int32_t lethal_threshold, double max_frontier_distance,
                        int32_t min_frontier_cluster_size, int32_t max_frontier_cluster_size, int32_t n_seeds, const int32_t *seeds,
                        int32_t max_records, fs_frontier_record *records, int32_t *n_records,
                        int64_t max_every, double *every_xy, int64_t *n_cells);

/* The seeds of fs_search_frontiers without caller seeds and of fs_get_frontier_costs_searched, per context.  FS_SEEDS_NEAREST (a
 * fresh context's): each component from its cell nearest the robot's cell, components in label order.  FS_SEEDS_REFERENCE: the
 * reference's outer breadth-first search from the robot (DEP/src/FrontierSearch.cpp:44-94) decides each component's seed and the
 * order of the list, walked level by level on the device.  Any other value: FS_E_INVALID, the setting unchanged. */
#define FS_SEEDS_NEAREST   0
#define FS_SEEDS_REFERENCE 1
int fs_set_frontier_seed_order(fs_ctx *ctx, int32_t order);

/* Replaces double FrontierCostCalculator::setMaxArrivalInformation() (DEP/include/.../CostCalculator.hpp:58,
 * DEP/src/CostCalculator.cpp:123-191): geometric maximum of the FOV window on an obstacle-free fan from
 * world (0,0).  max_value = the window maximum (0 if (0,0) is off-map: limits stay unset, as the
 * reference); caches max_gt = factor_max*max_value, min_gt = factor_min*max_gt in the context. */
int fs_max_arrival(fs_ctx *ctx, double *max_value, double *max_gt, double *min_gt);
/* override the cached limits (e.g. restored from a running node) */
int fs_set_arrival_limits(fs_ctx *ctx, double max_gt, double min_gt);

/* Replaces void FrontierCostCalculator::setArrivalInformationForFrontier(FrontierPtr&, std::vector<double>&)
 * (DEP/include/.../CostCalculator.hpp:56, DEP/src/CostCalculator.cpp:23-121) applied to the whole
 * frontier list of FrontierCostsManager::assignCosts (DEP/src/FrontierCostsManager.cpp:74-119),
 * including its blacklist branch (:77-86).  Order-preserving.
 *   goal_xyz      [n][3] Frontier::getGoalPoint() (z: origin_z for 2-D grids)
 *   frontier_size [n]    Frontier::getSize() or NULL (0)
 *   blacklisted   [n]    or NULL (none)
 *   achievable_in [n]    Frontier::isAchievable() before the call, or NULL (true)
 *   ray_counts    [n][n_elev][n_yaw] information_along_ray, or NULL
 *   arrival, argmax [n]; yaw [n] (theta_s_star); achievable [n]; status [n] */
int fs_score_arrival(fs_ctx *ctx, int32_t n, const double *goal_xyz, const int32_t *frontier_size,
                     const uint8_t *blacklisted, const uint8_t *achievable_in,
                     int32_t *ray_counts, int32_t *arrival, int32_t *argmax, double *yaw,
                     uint8_t *achievable, int32_t *status);

/* Replaces bool getTracedCells(double sx, double sy, double wx, double wy, RayTracedCells&, double max_length,
 * Costmap2D*) (DEP/include/.../Helpers.hpp:125-126, DEP/src/Helpers.cpp:32-96) with a RayTracedCells visitor
 * (Helpers.hpp:20-111) for a batch of arbitrary segments — the form FrontierRoadMap::isConnectable
 * (DEP/src/planners/FrontierRoadmap.cpp:716-737, visitor (253,254,0,255)) and the recovery controller
 * (fit_slam2_recovery/src/recovery_controller.cpp:78-88, visitor (256,256,0,255)) use.
 *   start_xyz, end_xyz [n][3]; max_length_cells as the reference passes it (a double, in cells)
 *   ok [n]      the bool return (false: a worldToMap failed)        traced [n]  getCells().size()
 *   hit [n]     hasHitObstacle()     unknown [n] getNumUnknown()     all [n]     getCellsSize() */
int fs_trace_segments(fs_ctx *ctx, int32_t n, const double *start_xyz, const double *end_xyz, double max_length_cells,
                      int32_t obst_min, int32_t obst_max, int32_t trace_min, int32_t trace_max,
                      uint8_t *ok, int32_t *traced, uint8_t *hit, int32_t *unknown, int32_t *all);

/* ---------------------------------------------------------------- Fisher information */

/* Replaces the per-query service response `map_points` (FIP/src/.../FisherInfoManager.cpp:60-88)
 * by the whole landmark cloud staged once: xyz [m][3] float32, world frame.  A point with a NaN / infinite coordinate, or one
 * beyond 1e17 m, is visible from nowhere; it keeps its place in the count m and contributes to no pose. */
int fs_upload_landmarks(fs_ctx *ctx, const float *xyz, int32_t m);

/* Replaces generateLookupTable(minX,maxX,minY,maxY,minZ,maxZ) (FIP/include/.../FisherInfoManager.hpp:94,
 * FIP/src/.../FisherInfoManager.cpp:117-229).  bounds == NULL uses gen_fi_lookup's arguments
 * (DEP/src/fisher_information/GenerateLookupMain.cpp:9). */
int fs_lookup_generate(fs_ctx *ctx, const float bounds[6]);
/* Replaces loadLookupTable() (FisherInfoManager.hpp:96, FisherInfoManager.cpp:231-262): raw
 * {float key[3]; float value} records, host-endian, no header.  Missing file -> FS_E_IO (the reference throws). */
int fs_lookup_load(fs_ctx *ctx, const char *path);
int fs_lookup_save(fs_ctx *ctx, const char *path);        /* byte-compatible with the reference's .dat */
int fs_lookup_set_records(fs_ctx *ctx, const float *records /* [n][4] */, int64_t n);
int fs_lookup_num_records(const fs_ctx *ctx, int64_t *n);
int fs_lookup_get_records(const fs_ctx *ctx, float *records /* [n][4] */);
/* getInformationFromLookup(Eigen::Vector3f&, ...) (FisherInfoManager.cpp:264-285): plain table value, NaN on miss */
int fs_lookup_query(const fs_ctx *ctx, const float p_camera[3], float *value);

int fs_set_fim_params(fs_ctx *ctx, const fs_fim_params *p);

/* Replaces bool FisherInformationManager::isPoseSafe(geometry_msgs::msg::Pose&, bool, float& information)
 * (FIP/include/.../FisherInfoManager.hpp:125, FIP/src/.../FisherInfoManager.cpp:39-115) for a batch of
 * poses; `safe = info_ref[i] > threshold` stays with the caller (threshold 550, FisherInfoBTPlugin.cpp:20).
 *   pose7     [n][7] position xyz + orientation quaternion xyzw (geometry_msgs::Pose order)
 *   info_ref  [n]    the reference scalar: sum of table value x crowding factor over visible landmarks
 *   fim21     [n][21] upper triangle (row-major) of the unit-weight 6x6 FIM, or NULL
 *   trace, logdet [n] or NULL;  n_visible, n_voxels [n] or NULL
 * A call that passes NULL for fim21, trace, logdet and n_visible — i.e. asks for what isPoseSafe itself reads (:83-100), plus
 * n_voxels if wanted — is served by a worker that neither accumulates the 6x6 sums nor looks at landmarks outside the lookup
 * table's box (a table miss contributes nothing, :90-94): same info_ref (to the last bits) and the same n_voxels, less work.
 * The visibility volume is fs_set_fim_params'; the reference's own request is max_dist 14, max_angle 4.0 (cone off, :63-64). */
int fs_score_fim(fs_ctx *ctx, int32_t n, const double *pose7, float *info_ref, float *fim21,
                 float *trace, float *logdet, int32_t *n_visible, int32_t *n_voxels);

/* Landmarks count only in LINE OF SIGHT on the staged grid (SURVEY.md App. A.3's optional occlusion test; an extension, OFF by
 * default — the reference counts a landmark behind a wall).  The rule, for a camera position s and a landmark w: the line is
 * BLOCKED when getTracedCells(s, w) on the staged grid is ok (fs_trace_segments' walk, uncapped: scale 1, cell visits
 * v = 0 .. end) and some visit with v + M <= end, M = 1 + (unsigned)(end_margin_m / resolution), has a cost in
 * [occ_min, occ_max].  The start cell is tested; the last M visits, at the landmark's end, are not (a landmark sits ON a
 * surface).  If either end is off the map nothing is tested and the line is not blocked.  On a 2-D grid (nz == 1) the walk is
 * planar: both z coordinates are replaced by origin_z; on a 3-D grid it is the 3-D walk between the two points.
 * With `enabled`, a landmark is visible from a pose if it passes fs_set_fim_params' predicate AND the line from the pose's
 * float32 translation (getTransformFromPose's t) to the landmark's float32 position, both widened to double, is not blocked;
 * voxel counts, crowding ranks, F, trace, log det, n_visible, n_voxels and the records follow from that visible set exactly as
 * without it.  Applies to fs_score_fim, the Fisher columns of fs_score_candidates / fs_get_frontier_costs*, the way points of
 * fs_plan_paths_information and the legs of fs_roadmap_routes.  The grid is read at call time: map updates and keep-out
 * repaints take effect at once, nothing is cached per landmark.  Scoring with `enabled` and no grid staged: FS_E_STATE.
 * occ_min / occ_max outside 0..255 or out of order, end_margin_m negative, not finite or >= 1e6: FS_E_INVALID, settings unchanged. */
typedef struct fs_occlusion_params {
    int32_t enabled;           /* 0 */
    int32_t occ_min, occ_max;  /* 254, 254: LETHAL only — the keep-out layer's 253 zones are virtual and hide nothing */
    double  end_margin_m;      /* 0.3 = the FI voxel step */
} fs_occlusion_params;
int fs_set_occlusion(fs_ctx *ctx, const fs_occlusion_params *p);   /* NULL: the defaults above */
int fs_get_occlusion(const fs_ctx *ctx, fs_occlusion_params *p);
/* The rule above (range and margin of fs_set_occlusion; `enabled` is not consulted) for n caller-given pairs.
 *   from_xyz, to_xyz [n][3]
 *   ok [n]            both ends on the map       blocked [n]  the line is blocked
 *   tested_cells [n]  visits the rule covers: end + 1 - M, 0 when the line is shorter than M or not ok; or NULL */
int fs_line_of_sight(fs_ctx *ctx, int32_t n, const double *from_xyz, const double *to_xyz,
                     uint8_t *ok, uint8_t *blocked, int32_t *tested_cells);

/* Which landmarks each pose sees.  Stands in for the GetLandmarksInView round trip of isPoseSafe
 * (FIP/src/fisher_information/FisherInfoManager.cpp:52-88): the reference sends the pose to the SLAM process and gets `map_points`
 * back in the pose's frame; here the cloud is the one fs_upload_landmarks staged and the answer is a list per pose.
 * Pose i's landmarks are exactly the set fs_score_fim counts in n_visible[i] under the context's settings at call time:
 * fs_set_fim_params' predicate and, with fs_set_occlusion enabled, the line of sight on the staged grid.  A landmark that misses
 * the lookup table's box is listed (table_value NaN) — it counts in n_visible; a non-finite or far-away landmark keeps its
 * place in 0 .. m-1 and is never listed.
 *   pose7    [n][7]      as fs_score_fim; turned into R, t the same way (getTransformFromPose)
 *   offsets  [n + 1]     CSR row pointer over the TRUE counts: offsets[0] = 0, offsets[i + 1] - offsets[i] = pose i's count,
 *                        whatever max_total is
 *   out      [max_total] entry k of pose i is stored at out[offsets[i] + k] iff that position is < max_total; nothing at or
 *                        beyond max_total is written.  Within a pose the entries are in ascending `index`.
 * out == NULL with max_total == 0 is the count-only form.  offsets[n] > max_total is not an error: the caller reads it and calls
 * again.  The entries of a pose in list order, fed to the reference's loop (:85-97 — voxel key, pointCount, factor, NaN
 * skipped), reproduce info_ref and n_voxels; they are also the points of the `fim_pointcloud` publisher (:15,101-107).
 * The output is a function of the inputs alone: not of the staged order of the cloud ("cloud.order"), not of call history.
 * NULL ctx, n < 0, max_total < 0, offsets == NULL (or pose7 == NULL) with n > 0, out == NULL with max_total > 0: FS_E_INVALID,
 * nothing written.  No cloud, no lookup table, or occlusion enabled and no grid: FS_E_STATE.  n == 0: FS_OK, offsets[0] = 0.
 * Synchronises once (count-only, or nothing to store) or twice.  No fs_multi_* form: call it on fs_multi_ctx(m, 0). */
typedef struct fs_view_landmark {
    int32_t index;        /* position of the landmark in the array fs_upload_landmarks was given (0 .. m-1) */
    float   p_camera[3];  /* the landmark in the pose's frame: what map_points[].position carries (:85-88) */
    float   table_value;  /* getInformationFromLookup(Eigen::Vector3f&) at p_camera: plain table value, NaN on a miss */
} fs_view_landmark;       /* 20 bytes */
int fs_landmarks_in_view(fs_ctx *ctx, int32_t n, const double *pose7, int64_t max_total, int64_t *offsets /* [n + 1] */,
                         fs_view_landmark *out /* [max_total] or NULL */);

/* Replaces float computeInformationFrontierPair(std::vector<Point>& lndmrk_w, Pose& kf_pose_w, Pose& est_pose_w,
 * std::vector<Point2D>& FOVFrontierPair) (FIP/src/.../FisherInformationHelpers.cpp:125-143; isInside / onLeft:
 * FIP/include/.../FisherInformationHelpers.hpp:20-43) for a batch of (estimation pose, CCW triangle) pairs over the
 * staged landmark cloud: sum of the local-Jacobian trace (computeInformationOfPointLocal, :106-112) of the landmarks
 * whose (x, y) lies strictly inside the triangle.  triangle_xy [n][3][2].  (kf_pose_w only feeds an unused local in
 * the reference; the function itself is not called at run time there.) */
int fs_information_frontier_pair(fs_ctx *ctx, int32_t n, const double *est_pose7, const double *triangle_xy, float *information);

/* Key-frame pose information.  Replaces, for a batch of poses,
 *   std::pair<float, std::vector<Eigen::Vector3f>> frontier_exploration_information_affine::computeInformationForPose(
 *       Pose& pose, std::vector<Pose>& neighbouring_poses, std::vector<int> neighbouring_ids, slam_msgs::msg::MapData&,
 *       double max_depth, double hfov, double max_depth_error, Eigen::Matrix3f Q, bool pcl_return, Logger, Costmap2D*, bool)
 * (DEP/include/frontier_exploration/deprecated/util.hpp:840-916; dead code in the reference — its call site is the commented
 * block DEP/src/CostCalculator.cpp:326-365) together with getNodesInRadius (util.hpp:616-632), frustumOverlap (:172-185),
 * getVerticesOfFrustum2D (:101-119), isPointInsideTriangle (:49-66) and the affine computeInformationOfPoint (:687-759).
 * fs_upload_keyframes stages slam_msgs MapData: key-frame poses (graph.poses) and their world points (nodes[].word_pts)
 * as a CSR list.  The costmap geometry (x/y origin, resolution, size) is the one of fs_upload_grid. */
typedef struct fs_keyframe_params {
    double max_depth;          /* 2.0   (CostCalculator.cpp:358) */
    double hfov;               /* 1.089 */
    double max_depth_error;    /* 0.5 */
    float  q_diag;             /* Q = q_diag * I, 0.01f (CostCalculator.cpp:356) */
    double radius;             /* getNodesInRadius radius, 4.5; < 0: every key-frame is a neighbour */
} fs_keyframe_params;
int fs_upload_keyframes(fs_ctx *ctx, int32_t n_keyframes, const double *kf_pose7 /* [n][7] xyz + quat xyzw */,
                        const int32_t *kf_offsets /* [n + 1] */, const float *points_xyz /* [kf_offsets[n]][3] */);
/* information [n]: the pose information (.first of the pair); n_cells [n]: information_map.size(); n_points [n]: points that
 * were added (inside the FOV triangle and on the map); the last two may be NULL.  The point list of pcl_return is not produced. */
int fs_information_for_pose(fs_ctx *ctx, int32_t n, const double *pose7, const fs_keyframe_params *params,
                            float *information, int32_t *n_cells, int32_t *n_points);

/* ---------------------------------------------------------------- fused scoring */

/* Replaces the scoring half of bool CostAssigner::getFrontierCosts(req, res)
 * (DEP/include/.../CostAssigner.hpp:70, DEP/src/CostAssigner.cpp:73-119): arrival information for every
 * candidate, then Fisher information at the pose (goal, best yaw) built like
 * isPoseSafe(Point, Point, bool) builds one (FIP/src/.../FisherInfoManager.cpp:31-37,
 * DEP/include/.../util/GeometryUtils.hpp:112-124).  Candidates whose status != OK get zero FI.
 * records [n] host memory, same order as the input list. */
int fs_score_candidates(fs_ctx *ctx, int32_t n, const double *goal_xyz, const int32_t *frontier_size,
                        const uint8_t *blacklisted, const uint8_t *achievable_in, fs_record *records);

/* Same, with every buffer already resident in HBM (device pointers; frontier_size / blacklisted /
 * achievable_in may be NULL).  Asynchronous on the context's stream: call fs_synchronize or
 * synchronise the borrowed stream before reading d_records.  This is the form the multi-GPU
 * shard runner uses: d_records is the send buffer of the RCCL all-gather. */
int fs_score_candidates_dev(fs_ctx *ctx, int32_t n, const double *d_goal_xyz, const int32_t *d_frontier_size,
                            const uint8_t *d_blacklisted, const uint8_t *d_achievable_in, fs_record *d_records);

/* ---------------------------------------------------------------- one process, several GPUs */

/* The reference scores in-process, from its one behaviour-tree thread (DEP/src/main.cpp:9-24,
 * DEP/src/ExplorationBT.cpp:376-410: ProcessFrontierCostsBT::onStart -> CostAssigner::getFrontierCosts).  fs_multi keeps that
 * shape on a multi-GPU node: ONE object, ONE calling thread, no launcher and no second process.  It owns one fs_ctx per
 * entry of device_ids (an ordinal may repeat: two contexts on one GPU, each with its stream), every staging call is
 * applied to all of them (the grid, the cloud and the table are replicated: 128 MiB + 1.2 MB + 2.8 MB at 512^3), and
 * fs_multi_score_candidates cuts the frontier list into contiguous blocks of ceil(n / G) candidates (fs_multi_shard_bounds
 * — the same rule the multi-process bench uses), starts block g on device g without waiting, then collects the 32-byte
 * records of all blocks into the caller's buffer in list order.  fs_multi_get_frontier_costs is the one-call form: blocks
 * gathered device to device over xGMI onto member 0's GPU, ranked there, one transfer out (below). */
typedef struct fs_multi fs_multi;
int  fs_multi_create(const int *device_ids, int n_devices, fs_multi **out);
void fs_multi_destroy(fs_multi *m);
int  fs_multi_num_devices(const fs_multi *m);
fs_ctx *fs_multi_ctx(fs_multi *m, int i);                  /* member context i (options, counters, ranking); owned by m */
const char *fs_multi_last_error(const fs_multi *m);
/* block [*lo, *hi) of shard `shard` of `n_shards` over a list of n: lo = min(n, shard * ceil(n / n_shards)), hi = min(n, lo + ceil(n / n_shards)) */
int  fs_multi_shard_bounds(int32_t n, int n_shards, int shard, int32_t *lo, int32_t *hi);
/* each of these applies the fs_* call of the same name to every member (first failure is returned).  The two uploads reach
   all devices at the same time (one short-lived host thread per member; the cloud is k-d ordered once for all of them);
   the caller sees one blocking call. */
int  fs_multi_set_option(fs_multi *m, const char *key, double value);
int  fs_multi_set_ray_params(fs_multi *m, const fs_ray_params *p);
int  fs_multi_upload_grid(fs_multi *m, const uint8_t *cells, int32_t nx, int32_t ny, int32_t nz, const double origin_xyz[3], double resolution);
int  fs_multi_update_grid_region(fs_multi *m, int32_t x0, int32_t y0, int32_t z0, int32_t sx, int32_t sy, int32_t sz,
                                 const uint8_t *cells, int64_t row_stride, int64_t slice_stride);   /* the window on every device */
/* the keep-out layer of every member (fs_keepout_add_fov / _add_disc / _clear, fs_mark_lethal_fov: the same request and the
   same map on each, so the same cells; LethalMarker::addNewMarkedAreaFOV keepout_layer.cpp:201-210, addNewMarkedArea
   lethal_marker.cpp:218-226, MarkLethalFOV::tick FisherInfoBTPlugin.cpp:148-182).  The outputs are member 0's. */
int  fs_multi_keepout_add_fov(fs_multi *m, double wx, double wy, double yaw, double height_m, int32_t *zone_id, int64_t *n_cells);
int  fs_multi_keepout_add_disc(fs_multi *m, double wx, double wy, double radius_m, int32_t *zone_id, int64_t *n_cells);
int  fs_multi_keepout_clear(fs_multi *m);
int  fs_multi_mark_lethal_fov(fs_multi *m, const double robot_pose7[7], double blacklist_pose7[7], int32_t *zone_id, int64_t *n_cells);
/* fs_inflate on every member (the same map on each, so the same cells); the counts are member 0's */
int  fs_multi_inflate(fs_multi *m, const fs_inflation_params *p, int32_t x0, int32_t y0, int32_t sx, int32_t sy,
                      int64_t *n_seeds, int64_t *n_changed);
/* fs_information_layer on every member (the same map, cloud and table on each, so the same cells); the outputs are member 0's */
int  fs_multi_information_layer(fs_multi *m, const fs_info_layer_params *p, int32_t x0, int32_t y0, int32_t sx, int32_t sy,
                                float *info, int32_t *anchor_cell, float *info_per_yaw, double *quat_zw, int64_t *n_scored,
                                int64_t *n_changed);
int  fs_multi_upload_landmarks(fs_multi *m, const float *xyz, int32_t n_landmarks);
int  fs_multi_lookup_generate(fs_multi *m, const float bounds[6]);
int  fs_multi_lookup_load(fs_multi *m, const char *path);
int  fs_multi_set_fim_params(fs_multi *m, const fs_fim_params *p);
int  fs_multi_set_occlusion(fs_multi *m, const fs_occlusion_params *p);
/* setMaxArrivalInformation once (member 0), the limits handed to every member */
int  fs_multi_max_arrival(fs_multi *m, double *max_value, double *max_gt, double *min_gt);
/* fs_score_arrival over all members (same arguments; every output array in list order) */
int  fs_multi_score_arrival(fs_multi *m, int32_t n, const double *goal_xyz, const int32_t *frontier_size,
                            const uint8_t *blacklisted, const uint8_t *achievable_in,
                            int32_t *ray_counts, int32_t *arrival, int32_t *argmax, double *yaw,
                            uint8_t *achievable, int32_t *status);
/* fs_score_candidates over all members: host buffers in, records [n] out, list order; returns when every block is in */
int  fs_multi_score_candidates(fs_multi *m, int32_t n, const double *goal_xyz, const int32_t *frontier_size,
                               const uint8_t *blacklisted, const uint8_t *achievable_in, fs_record *records);
/* fs_score_fim over all members (FisherInformationManager::isPoseSafe's batch, FIP/src/fisher_information/FisherInfoManager.cpp:39-115):
   poses cut into the same contiguous blocks, every member started before the first is waited for, every column in list order */
int  fs_multi_score_fim(fs_multi *m, int32_t n, const double *pose7, float *info_ref, float *fim21,
                        float *trace, float *logdet, int32_t *n_visible, int32_t *n_voxels);
/* fs_get_frontier_costs — the whole of CostAssigner::getFrontierCosts (DEP/src/CostAssigner.cpp:73-119; the in-process call of
 * DEP/src/ExplorationBT.cpp:376-410) — over all members, with the records NEVER visiting the host between scoring and ranking:
 * member g scores block g on its device; its 32-byte records are moved device to device into ONE list on member 0's GPU
 * (hipMemcpyPeerAsync over xGMI on the member's stream behind its kernels, one event per member that member 0's stream waits
 * for; a member that shares member 0's GPU writes the list itself); fs_rank_candidates_dev ranks the gathered list there; ONE
 * transfer brings records, costs, utilities and order back.  Same arguments, same results (integers, costs and order bit for
 * bit) as fs_get_frontier_costs on one context.  A gather onto the ranking device, not an all-gather: in one process only
 * that device needs the list.  Where the runtime refuses peer access between a member and member 0 the blocks bounce through
 * page-locked host memory instead; the call still succeeds and fs_multi_last_error says so (fs_multi_gather_mode: 2). */
int  fs_multi_get_frontier_costs(fs_multi *m, int32_t n, const double *goal_xyz, const int32_t *frontier_size, const uint8_t *blacklisted,
                                 const uint8_t *achievable_in, const double *path_length, const double *path_heading,
                                 double alpha, double beta, double max_vx, double max_wz, int with_fisher_information,
                                 fs_record *records, double *weighted_cost, double *arrival_utility, double *distance_utility, int32_t *order);
/* how fs_multi_get_frontier_costs moves the blocks: 1 device to device (peer access granted, or every member on one GPU),
   2 through page-locked host memory (peer access refused), 3 / forced values: fs_multi_set_option("multi.gather", 0 auto | 1 | 2 | 3
   = device copies even between members of one GPU | 4 = those copies through hipMemcpyPeerAsync), for tests of the paths a one-GPU
   box cannot take by itself.  < 0: error */
int  fs_multi_gather_mode(fs_multi *m);

/* ---------------------------------------------------------------- utility + ranking */

/* Replaces the U1 block of FrontierCostsManager::assignCosts (DEP/src/FrontierCostsManager.cpp:118,126-205)
 * and the four parallel vectors of GetFrontierCostsResponse (DEP/include/.../CostAssigner.hpp:51-59),
 * on the GPU.  records [n] host (from fs_score_candidates or gathered from all shards);
 * path_length / path_heading [n] from the planner (out of scope; inputs here).
 * Outputs: weighted_cost, arrival_utility, distance_utility [n]; order [n] = candidate indices by
 * ascending cost (stable).  Returns FS_E_RANGE where the reference would throw. */
int fs_rank_candidates(fs_ctx *ctx, int32_t n, const fs_record *records, const uint8_t *blacklisted,
                       const double *path_length, const double *path_heading,
                       double alpha, double beta, double max_vx, double max_wz,
                       double *weighted_cost, double *arrival_utility, double *distance_utility,
                       int32_t *order);

/* The whole of bool CostAssigner::getFrontierCosts(req, res) (DEP/include/.../CostAssigner.hpp:43-59,70; DEP/src/CostAssigner.cpp:73-119)
 * — FrontierCostsManager::assignCosts' arrival information for every frontier (DEP/src/FrontierCostsManager.cpp:74-119) followed by
 * its U1 block (:126-205) — as ONE call: frontier list and the planner's path columns in, scored and ranked candidates out; one
 * transfer each way and one synchronisation, the records never visit the host between scoring and ranking.  Up to 1024
 * frontiers (the reference handles tens per tick) the kernels read the inputs from, and write the results into, the context's
 * mapped page-locked buffers in place — plain launches, no transfers of their own.  (Replaying the sequence as a captured launch
 * graph exists behind fs_set_option("graph", 1) of fitslam_frontier_dev.h and is OFF by default: it measured 5-7 us slower per
 * call than the plain launches on this runtime; only with it on is the list padded to power-of-two buckets.)
 *   path_length, path_heading [n]  what the planner set on each frontier (Frontier::setPathLength / setPathHeading; inputs here).
 *                                  The reference plans a frontier only once its arrival information has left it achievable
 *                                  (FrontierCostsManager.cpp:88-91); here the columns come first — those of a frontier that turns
 *                                  out unachievable (or is blacklisted) are never read: same costs, the plan was spare work
 *   with_fisher_information        0: arrival information only — what the reference's assignCosts uses; the Fisher columns of the
 *                                  records stay zero.  1: also the Fisher information at the pose (goal, best yaw), as fs_score_candidates
 *   records [n]; weighted_cost [n]; arrival_utility, distance_utility, order [n] or NULL.  FS_E_RANGE where the reference throws. */
int fs_get_frontier_costs(fs_ctx *ctx, int32_t n, const double *goal_xyz, const int32_t *frontier_size, const uint8_t *blacklisted,
                          const uint8_t *achievable_in, const double *path_length, const double *path_heading,
                          double alpha, double beta, double max_vx, double max_wz, int with_fisher_information,
                          fs_record *records, double *weighted_cost, double *arrival_utility, double *distance_utility, int32_t *order);

/* Same, behind the scoring call on the device: every pointer is device memory (d_records = the records fs_score_candidates_dev
 * wrote, or the receive buffer of the all-gather), launched on the context's stream and NOT waited for — score and rank run
 * back to back without the records ever visiting the host ("fused after scoring").  d_arrival_utility,
 * d_distance_utility, d_order may be NULL (not wanted).  d_range_error (one int32, or NULL): non-zero after the kernels have run
 * where the reference would throw (FS_E_RANGE of the host form) — read it together with the results. */
int fs_rank_candidates_dev(fs_ctx *ctx, int32_t n, const fs_record *d_records, const uint8_t *d_blacklisted,
                           const double *d_path_length, const double *d_path_heading,
                           double alpha, double beta, double max_vx, double max_wz,
                           double *d_weighted_cost, double *d_arrival_utility, double *d_distance_utility,
                           int32_t *d_order, int32_t *d_range_error);

/* ---------------------------------------------------------------- grid planner (the path columns) */

/* FrontierCostCalculator::setPlanForFrontier ("A*PlannerDistance", DEP/src/CostCalculator.cpp:193-393) for n frontiers at once:
 * one NavFn potential from the robot cell over the staged 2-D grid, then NavFn::calcPath from every goal.  robot_pose7 = xyz + quat xyzw.
 * achievable_in [n] or NULL (= all).  Outputs [n]: path_length (points), path_length_m, path_heading, achievable.
 * The field is the fixed point of NavFn's cell update under the tiled schedule of DESIGN.md 4.9 (the reference's A* stops its wave
 * at the goal and drops pushes beyond 10 000 per buffer: per frontier, a partial field); it is kept per context for (grid,
 * robot cell, allow_unknown) — fs_upload_grid, fs_upload_grid_bricks and fs_update_grid_region drop it.  A frontier that is not
 * planned (achievable_in 0, robot or goal off the map, goal cell unreached, calcPath failed): achievable 0 and DBL_MAX in the
 * three columns.  nz > 1: FS_E_INVALID.
 * Under FS_GRID_SEARCH_REFERENCE (fs_set_grid_search) every frontier is planned on the reference's own partial field instead: per
 * distinct goal cell, the calcNavFnAstar wave from the robot cell that stops at that cell.  achievable is 1 when the robot and the
 * goal are on the map, the wave reached the goal cell (potarr[goal] < POT_HIGH) and calcPath > 0 on that wave's field; the three
 * path columns are defined exactly as above, on that path.  The converged field and its cache are neither used nor touched.  A map
 * with a side above 4096 cells: FS_E_INVALID (the bound below which the wave's heuristic has been checked against libm's hypot). */
int fs_plan_paths(fs_ctx *ctx, const double robot_pose7[7], int32_t allow_unknown, int32_t n, const double *goal_xyz,
                  const uint8_t *achievable_in, double *path_length, double *path_length_m, double *path_heading, uint8_t *achievable);
/* the potential field fs_plan_paths descends, [ny][nx] float (NavFn::getPotArray): for tests and visualisation.  Robot off the
 * map: FS_E_INVALID */
int fs_navfn_potential(fs_ctx *ctx, const double robot_pose7[7], int32_t allow_unknown, float *potential);
/* How fs_plan_paths, fs_plan_paths_information, fs_get_frontier_costs_planned and fs_get_frontier_costs_searched plan on the grid, per
 * context.  FS_GRID_SEARCH_CONVERGED (a fresh context's): ONE converged field per (grid, robot cell, allow_unknown), descended from
 * every frontier.  FS_GRID_SEARCH_REFERENCE: the reference's per-frontier A* wave (NavFn::calcNavFnAstar: three priority buffers of
 * 10 000 cells, the curT / priInc thresholds, the stop at the frontier cell, max(nx * ny / 20, nx + ny) cycles) once per distinct
 * goal cell, one wavefront per wave on the device, and calcPath on that wave's field — the reference's columns bit for bit
 * (DESIGN.md 4.9 records where the converged field differs).  Any other value: FS_E_INVALID, the setting unchanged.
 * fs_set_option: "navfn.wave_slots" (0: as many waves side by side as "navfn.wave_bytes", default 1 GiB, holds; a positive value is
 * the slot count itself) — results are identical for every slot count —, "navfn.wave_cap" (16..10 000, default 10 000: the
 * capacity of each priority buffer; for tests, only the default is the reference's). */
#define FS_GRID_SEARCH_CONVERGED 0
#define FS_GRID_SEARCH_REFERENCE 1
int fs_set_grid_search(fs_ctx *ctx, int32_t search);
/* The field of ONE wave of the REFERENCE grid search, [ny][nx] float: NavFn::getPotArray after calcNavFnAstar from the robot cell
 * with the wave stopped at the goal's cell.  For tests and visualisation; works whatever the context's grid search is.  limit (may
 * be NULL): bit 0 the cycle budget ran out, bit 1 a push was dropped at the buffer cap.  Robot or goal off the map, nz > 1, a side
 * above 4096 cells: FS_E_INVALID. */
int fs_navfn_wave_potential(fs_ctx *ctx, const double robot_pose7[7], int32_t allow_unknown, const double goal_xyz[3], float *potential,
                            int32_t *limit);
/* fs_get_frontier_costs with the path columns planned on the device: plan -> arrival (+ Fisher) -> U1 -> order, one call; the
 * planner's achievability feeds achievable_in; path_length_m [n] or NULL.  Same results, bit for bit, as fs_plan_paths followed by
 * fs_get_frontier_costs on its columns; the path columns never visit the host in between. */
int fs_get_frontier_costs_planned(fs_ctx *ctx, const double robot_pose7[7], int32_t allow_unknown, int32_t n, const double *goal_xyz,
                  const int32_t *frontier_size, const uint8_t *blacklisted, double alpha, double beta, double max_vx, double max_wz,
                  int with_fisher_information, fs_record *records, double *weighted_cost, double *arrival_utility,
                  double *distance_utility, int32_t *order, double *path_length_m);
/* Fisher information along every planned path: will SLAM keep tracking on the way to the frontier?  The sampling
 * is setPlanForFrontier's (DEP/src/CostCalculator.cpp:302-366, 382-390: a way point once more than (int)(sample_distance /
 * resolution) path points have gone by, turned towards the point `lookahead` further on by getRelativePoseGivenTwoPoints, the
 * sum of the positive values over the number of way points); the value of a way point is isPoseSafe's scalar
 * (FIP/src/fisher_information/FisherInfoManager.cpp:31-37, over a path in DEP/src/FullPathOptimizer.cpp:308-340): fs_score_fim's
 * info_ref at that pose under the context's landmarks, table and fs_set_fim_params. */
typedef struct fs_path_info_params {
    double  sample_distance_m;  /* 1.5  (CostCalculator.cpp:328) */
    int32_t lookahead_points;   /* 10   (:332) */
    double  fi_threshold;       /* 550.0 (FisherInfoBTPlugin.cpp:20); a way point is unsafe unless info > threshold */
} fs_path_info_params;
/* The plan is fs_plan_paths' own (same field cache, same four columns, bit for bit).  params NULL: the defaults above.
 * Path f of len points (point 0 at the frontier, len - 1 at the robot) has len / (s + 1) way points, s = (int)(sample_distance_m /
 * resolution); way point k, counted from the robot, stands on the cell centre of point j = len - (k + 1)(s + 1), z = 0, and looks
 * at the cell centre of point max(j - lookahead_points, 0) (the same cell: yaw 0).
 * Per frontier [n]: n_waypoints; info_mean = (the fp64 sum of the values > 0, in way-point order) / n_waypoints, 0 without way
 * points; info_min (+inf without); first_unsafe = the first k with !(info > fi_threshold), -1 if none.  A frontier that is not
 * planned: 0, 0, +inf, -1.
 * The dump — n_total, waypoint_offset [n + 1], waypoint_pose7 [max_waypoints][7], waypoint_info [max_waypoints]: all four or all
 * NULL — lists every way point in list order; a pose of the dump handed to fs_score_fim makes the same pose record.  More way
 * points than max_waypoints: FS_E_RANGE with *n_total set and nothing else written.
 * FS_E_INVALID: sample_distance_m NaN or negative, lookahead_points negative, fi_threshold not finite; otherwise refuses what
 * fs_plan_paths and fs_score_fim refuse, with their codes.  Synchronises twice (the number of distinct poses sizes the scoring
 * launch), plus the round polling of a field that is not cached. */
int fs_plan_paths_information(fs_ctx *ctx, const double robot_pose7[7], int32_t allow_unknown, int32_t n, const double *goal_xyz,
                  const uint8_t *achievable_in, const fs_path_info_params *params, double *path_length, double *path_length_m,
                  double *path_heading, uint8_t *achievable, int32_t *n_waypoints, double *info_mean, float *info_min,
                  int32_t *first_unsafe, int64_t max_waypoints, int64_t *n_total, int32_t *waypoint_offset, double *waypoint_pose7,
                  float *waypoint_info);
/* searchFrom -> plan -> score -> rank in one call: fs_search_frontiers with the context's seed order (fs_set_frontier_seed_order)
 * and no caller seeds from the pose's xy, then
 * fs_get_frontier_costs_planned on its records (goal_xyz = (goal_x, goal_y, 0), frontier_size = size, blacklisted = the goal point
 * equals one of blacklist_xy [n_blacklist][2] bit for bit: FrontierGoalPointEquality, the key of frontier_blacklist_).  Every
 * column after frontiers [max_records] has *n_frontiers entries.  More records than max_records: FS_E_INVALID with *n_frontiers
 * set and nothing else written (a ranking over part of the list would be wrong).  The goal, size and blacklist columns stay in
 * device memory between the search and the scoring (only the planner's host-libm heading goes up).  Same results, bit for bit,
 * as the two calls, except the Fisher float sums (info_ref, trace, logdet), which are not run-to-run bit-stable in the scorer
 * itself; the ranking's columns read only its integers. */
int fs_get_frontier_costs_searched(fs_ctx *ctx, const double robot_pose7[7], int32_t lethal_threshold, double max_frontier_distance,
                  int32_t min_frontier_cluster_size, int32_t max_frontier_cluster_size, int32_t allow_unknown,
                  int32_t n_blacklist, const double *blacklist_xy, double alpha, double beta, double max_vx, double max_wz,
                  int with_fisher_information, int32_t max_records, fs_frontier_record *frontiers, int32_t *n_frontiers,
                  fs_record *records, double *weighted_cost, double *arrival_utility, double *distance_utility, int32_t *order,
                  double *path_length_m);

/* ---------------------------------------------------------------- frontier roadmap (the reference's default planner) */

/* FrontierRoadMap's parameters (DEP/params/exploration.yaml:23-27; defaults 1.0, 6.1, 0.25, 0.25); max_connection_length is
 * 1.5 * radius (DEP/src/planners/FrontierRoadmap.cpp:20).  A new parameter set starts an empty roadmap. */
int fs_set_roadmap_params(fs_ctx *ctx, double grid_cell_size, double radius_to_decide_edges, double min_distance_between_two_frontier_nodes,
                          double min_distance_between_robot_pose_and_node);
/* How fs_roadmap_plan, fs_get_frontier_costs_roadmap and the pair lengths of fs_roadmap_next_goal search the roadmap, per context
 * (fs_set_roadmap_params leaves it).  FS_ROADMAP_SEARCH_TREE (a fresh context's): ONE shortest-path tree per (roadmap, start node)
 * under squared segment lengths.  FS_ROADMAP_SEARCH_REFERENCE: the reference's per-goal A* (FrontierRoadmapAStar::getPlan,
 * astar.cpp:42-93) for every distinct (start, goal) node pair — std::priority_queue's heap order, the squared heuristic, the closed
 * set tested on successors only — so the lengths are the reference's (DESIGN.md 4.10 records where the tree differs).  Any other
 * value: FS_E_INVALID, the setting unchanged. */
#define FS_ROADMAP_SEARCH_TREE      0
#define FS_ROADMAP_SEARCH_REFERENCE 1
int fs_set_roadmap_search(fs_ctx *ctx, int32_t search);
/* FrontierRoadMap::populateNodes(populateClosest = true) (FrontierRoadmap.cpp:185-252) — addNodes (is_robot_pose 0) or
 * addRobotPoseAsNode (1): a point closer than the minimum distance to a node of the 3 x 3 hash cells around it is dropped.  xy [n][2].
 * A cell that comes to hold more than 20 nodes: FS_E_RANGE, that node added, the rest of the list not (the reference throws). */
int fs_roadmap_add_nodes(fs_ctx *ctx, int32_t n, const double *xy, int32_t is_robot_pose);
/* FrontierRoadMap::reConstructGraph(entireGraph = true, optimizeRoadmap = false) (FrontierRoadmap.cpp:347-408) on the device: every
 * node becomes a key of the roadmap, its list the nodes within the radius that pass isConnectable (:716-737) on the staged 2-D grid,
 * in getNodesWithinRadius's order.  nz > 1: FS_E_INVALID. */
int fs_roadmap_rebuild(fs_ctx *ctx);
/* FrontierRoadMap::constructNewEdges (FrontierRoadmap.cpp:279-334; with the robot pose in xy also constructNewEdgeRobotPose): each
 * point's closest hash node linked both ways to the nodes within the radius it can connect to.  Every isConnectable of the call is
 * walked on the device in one batch, the insertions follow on the host in the reference's order.  xy [n][2].  No node: a no-op. */
int fs_roadmap_connect(fs_ctx *ctx, int32_t n, const double *xy);
/* UpdateRoadmapBT (ExplorationBT.cpp:247-257) in one call, decided on the device: addNodes(xy),
 * addRobotPoseAsNode(robot_xy) if add_robot_pose, constructNewEdges(xy), constructNewEdgeRobotPose(robot_xy).  The roadmap afterwards
 * equals, bit for bit (node list, key flags, adjacency in append order, pending key-frame queue), fs_roadmap_add_nodes(xy, 0);
 * fs_roadmap_add_nodes(robot_xy, 1); fs_roadmap_connect(xy ++ robot_xy).  Outputs (each may be NULL): points of xy added as nodes,
 * whether the robot pose was, undirected edges inserted.  Counters 1033-1035 (fs_get_counter): the call's isConnectable walks, its
 * owners (distinct closest nodes, the only ones that build candidate lists) and the rounds of its keep rule.
 * Non-finite input, a null pointer, nz > 1, more than 16384 points: FS_E_INVALID with NOTHING changed — every check comes before
 * the first addition (the three-call sequence adds its nodes before fs_roadmap_connect refuses a 3-D grid).  A cell that comes to
 * hold more than 20 nodes: FS_E_RANGE with the roadmap as the three calls leave it when they stop at the failing one — the nodes
 * up to and including that one added, the robot pose not added if the list tripped, no edge built.  n == 0 without the robot pose
 * on an empty roadmap: a no-op.  The roadmap generation is bumped once.  Two synchronisations (sizes, result). */
int fs_roadmap_update(fs_ctx *ctx, int32_t n, const double *xy /* [n][2] */, const double robot_xy[2], int32_t add_robot_pose,
                      int32_t *n_nodes_added, int32_t *robot_added, int64_t *n_edges_added);
/* The roadmap, for tests and visualisation: node positions xy [n][2] in insertion order, key [n] (1: a key of roadmap_, what
 * getClosestNodeInRoadMap considers), the adjacency as CSR row_ptr [n + 1], col [n_edges] in append order.  Any pointer may be NULL
 * (call first with NULL arrays for the sizes). */
int fs_roadmap_get_graph(fs_ctx *ctx, int32_t *n_nodes, int64_t *n_edges, double *xy, uint8_t *key, int32_t *row_ptr, int32_t *col);
/* FrontierCostCalculator::setPlanForFrontierRoadmap ("RoadmapPlannerDistance", DEP/src/CostCalculator.cpp:395-438) for n frontiers:
 * the start is the key node closest to the robot, each goal's end node the key node closest to it (getClosestNodeInRoadMap,
 * FrontierRoadmap.cpp:506-543).  The route, by the context's roadmap search (fs_set_roadmap_search): FS_ROADMAP_SEARCH_TREE, the
 * shortest-path tree from the start under squared segment lengths — ONE tree per (roadmap, start node), kept until the roadmap
 * changes — where the reference runs an A* per frontier (astar.cpp:42-93; DESIGN.md 4.10 records where the two differ);
 * FS_ROADMAP_SEARCH_REFERENCE, that A* once per distinct goal node, one wave per query on the device, bit for bit the reference's
 * lengths (the tree and its cache are not touched).  Outputs [n]: path_length = path_length_m (metres, summed from the goal end),
 * path_heading, achievable.  achievable_in 0, no key node or goal node not reached: achievable 0 and DBL_MAX in the three columns; a
 * goal at the robot's exact position: length 0.  One synchronisation (the tree's round polling above one workgroup's size, or a
 * query that outgrows the A*'s global pool, adds more). */
int fs_roadmap_plan(fs_ctx *ctx, const double robot_pose7[7], int32_t n, const double *goal_xyz, const uint8_t *achievable_in,
                    double *path_length, double *path_length_m, double *path_heading, uint8_t *achievable);
/* fs_get_frontier_costs with the path columns planned on the roadmap in the same call: plan -> arrival (+ Fisher) -> U1 -> order.
 * Same results, bit for bit, as fs_roadmap_plan followed by fs_get_frontier_costs on its columns, under either roadmap search
 * (fs_set_roadmap_search); the path columns never visit the host. */
int fs_get_frontier_costs_roadmap(fs_ctx *ctx, const double robot_pose7[7], int32_t n, const double *goal_xyz, const int32_t *frontier_size,
                  const uint8_t *blacklisted, double alpha, double beta, double max_vx, double max_wz, int with_fisher_information,
                  fs_record *records, double *weighted_cost, double *arrival_utility, double *distance_utility, int32_t *order,
                  double *path_length_m);
/* The default planner's tick in one call: search -> roadmap update -> roadmap plan -> arrival (+ Fisher) -> U1 -> order.
 * fs_get_frontier_costs_searched's arguments without allow_unknown and with add_robot_pose (fs_roadmap_update's): the search with the
 * context's seed order (fs_set_frontier_seed_order), fs_roadmap_update on its goal points and the pose's xy — read from the goal column
 * the search left on the device — then fs_get_frontier_costs_roadmap on the records under the context's roadmap search
 * (fs_set_roadmap_search).  Same results, bit for bit, as fs_search_frontiers, fs_roadmap_update and fs_get_frontier_costs_roadmap in
 * turn (the Fisher float sums excepted, as in fs_get_frontier_costs_searched).  More records than max_records: FS_E_INVALID with
 * *n_frontiers set, the roadmap untouched.  FS_E_RANGE from the update: returned with *n_frontiers and the frontier records written,
 * the roadmap as fs_roadmap_update leaves it, nothing ranked.  A robot off the map finds nothing; the update of an empty list runs. */
int fs_get_frontier_costs_searched_roadmap(fs_ctx *ctx, const double robot_pose7[7], int32_t lethal_threshold, double max_frontier_distance,
                  int32_t min_frontier_cluster_size, int32_t max_frontier_cluster_size, int32_t add_robot_pose,
                  int32_t n_blacklist, const double *blacklist_xy, double alpha, double beta, double max_vx, double max_wz,
                  int with_fisher_information, int32_t max_records, fs_frontier_record *frontiers, int32_t *n_frontiers,
                  fs_record *records, double *weighted_cost, double *arrival_utility, double *distance_utility, int32_t *order,
                  double *path_length_m);
/* The routes behind fs_roadmap_plan's numbers: RoadmapPlanResult::path of getPlan (FrontierRoadmap.cpp:550-635,
 * astar.cpp:57-69 — what the reference publishes as frontier_roadmap_nav2_plan), its line-of-sight shortcut
 * FrontierRoadMap::refinePath (:657-714) on the staged grid, and FullPathOptimizer::isPathSafe's question (FullPathOptimizer.cpp:
 * 308-340) — does SLAM keep tracking on the way? — as the Fisher information of every leg. */
typedef struct fs_route_params {
    int32_t refine;            /* 1: the legs that are scored are refinePath's list; 0: getPlan's */
    int32_t with_information;  /* 0: routes only (no landmarks / table needed; the information columns and the leg dump must be NULL) */
    double  fi_threshold;      /* 550.0 (FisherInfoBTPlugin.cpp:20): a leg is unsafe unless info > threshold */
} fs_route_params;             /* NULL: {1, 1, 550.0} */
/* path_length .. achievable [n] are fs_roadmap_plan's own, bit for bit, under the context's roadmap search; the tree cache and the
 * counters 1005-1006 / 1021-1023 move as that call moves them.
 * Routes.  One route per DISTINCT goal node that a planned frontier's plan reached, in ascending node index (indices are
 * fs_roadmap_get_graph's): goal_node, complete, n_legs, info_mean, info_min, first_unsafe [max_routes], *n_routes of them;
 * route_of [n] = the frontier's route, -1 where achievable is 0 or the goal is the robot's exact position (length 0: the
 * reference returns an empty path).  FS_ROADMAP_SEARCH_TREE: root, ..., v — the predecessors from the goal's closest key node v back
 * to the root, reversed, hops[v] + 1 nodes.  FS_ROADMAP_SEARCH_REFERENCE: the A*'s path — the record chain from allNodes[goal] along
 * parent, reversed, start first (stale records included).  Either way the route's segment lengths summed from the goal end are
 * path_length_m, bit for bit.
 * refinePath on route P[0..m-1]: R = [P[0]], kk = 0; while kk < m - 1: next = kk + 1; while next < m and isConnectable(P[kk],
 * P[next]): ++next; if next - 1 == kk: stop (complete = 0, R is truncated); append P[next - 1], kk = next - 1.  The scan stops at
 * the first refusal, isConnectable walks FROM P[kk] (the direction matters) and is fs_roadmap_rebuild's predicate on the grid
 * staged NOW.  complete = 1 and R = [P[0]] for m = 1.  params->refine needs a 2-D grid (else fs_roadmap_rebuild's refusal);
 * without it no grid is read, complete is 1 and the refined dump must be NULL.
 * Legs.  The scored list L is R (refine) or P; leg k is (L[k], L[k + 1]), n_legs = len(L) - 1.  Its pose is
 * getRelativePoseGivenTwoPoints: (x, y, 0) of L[k], yaw atan2 towards L[k + 1], quaternion (0, 0, sin(yaw / 2), cos(yaw / 2)); its
 * value fs_score_fim's info_ref at that pose under the context's landmarks, table and fs_set_fim_params.  Equal (from, to) pairs
 * are scored once ("routes.dedup", default 1).  info_mean, info_min, first_unsafe as fs_plan_paths_information defines them over
 * the legs in order (0, +inf, -1 without legs).  The reference's literal isPathSafe tests pathToFollow[0] -> [1] on every
 * iteration: that is leg 0's value here (first_unsafe == 0 is its verdict); its trailing robot-pose overlap gate is not part of
 * this call.
 * Dumps, each group all or none: {n_nodes_total, node_offset [max_routes + 1], node [max_nodes]} the raw lists as CSR;
 * {n_refined_total, refined_offset [max_routes + 1], refined_node [max_nodes]} the refined ones; {leg_pose7 [max_nodes][7],
 * leg_info [max_nodes]} the legs route by route (route r's first leg is at offset_L[r] - r).  n_routes may be NULL only when
 * n == 0.  More routes than max_routes, or (with a dump) more raw nodes than max_nodes: FS_E_RANGE with *n_routes and the given
 * totals set and nothing else written.
 * FS_E_INVALID: a dump group half given, a dump that the params switch off, fi_threshold not finite, max_routes / max_nodes
 * negative; otherwise refuses what fs_roadmap_plan refuses and, with_information, what fs_score_fim refuses, with their codes.
 * Counters (fs_get_counter): 1026 distinct routes of the last call, 1027 isConnectable walks of its refinement, 1028 distinct leg
 * poses it scored, 1029 times a call ran the A* again because the chain pool was too small (fs_set_option "routes.pool_nodes":
 * its size to begin with, 65536 nodes; it grows to what a call needed).  Synchronises three times (the
 * routes' sizes, the number of distinct poses, the results); twice without information. */
int fs_roadmap_routes(fs_ctx *ctx, const double robot_pose7[7], int32_t n, const double *goal_xyz, const uint8_t *achievable_in,
                  const fs_route_params *params, double *path_length, double *path_length_m, double *path_heading,
                  uint8_t *achievable, int32_t *route_of, int32_t max_routes, int32_t *n_routes, int32_t *goal_node,
                  uint8_t *complete, int32_t *n_legs, double *info_mean, float *info_min, int32_t *first_unsafe, int64_t max_nodes,
                  int64_t *n_nodes_total, int64_t *node_offset, int32_t *node, int64_t *n_refined_total, int64_t *refined_offset,
                  int32_t *refined_node, double *leg_pose7, float *leg_info);

/* Key-frame anchors (FrontierRoadMap's loop-closure correction).  Every node fs_roadmap_add_nodes accepts — the one
 * that trips its FS_E_RANGE included — is queued as pending (no_kf_parent_queue_); fs_set_roadmap_params clears the queue, the key
 * frames and the anchors, as a new FrontierRoadMap starts empty.
 * fs_roadmap_set_keyframes: mapDataCallback (DEP/src/planners/FrontierRoadmap.cpp:42-130) for one map message of n key frames, kf_id [n]
 * and pose7 [n][7] = x y z qx qy qz qw.  The message replaces the key-frame table (an id named twice keeps its last pose) and the
 * key-frame cell hash (getGridCell with the roadmap's grid_cell_size: each cell lists its ids in message order, duplicates kept).
 * Then every pending node is taken in FIFO order: the parents are every id of its own cell; else the first occupied cell of the
 * square of radius (int)(grid_cell_size * m), m = 1, 2, ..., scanned dx outer / dy inner, given up once the radius passes 7 (not
 * necessarily the nearest cell).  For each parent, T_kf^-1 * (float x, float y, 0) is appended to the anchors of that id, in float32:
 * T_kf = Translation3f * Quaternionf with the quaternion NOT normalised and the general 3 x 3 inverse, not the transpose.  A node
 * without parents is dropped.  The queue ends empty; anchors are never removed.  n_anchored / n_orphaned (may be NULL): pending
 * nodes that got parents / were dropped.  An empty message (n = 0) drops every pending node.  A non-finite pose, or one whose float
 * rotation has determinant 0: FS_E_INVALID and nothing changes.
 * fs_roadmap_optimize: reConstructGraph(entireGraph = true, optimizeRoadmap = true) (:347-408) — optimizeSHM (:132-155), then the
 * rebuild of fs_roadmap_rebuild.  Every anchor of an id the latest message holds becomes the point (T_kf * p_c).xy (float), in the
 * order of the reference's std::unordered_map<int, std::vector<Eigen::Vector3f>> keyframe_mapping_ under libstdc++ (its iteration
 * order, then append order); anchors of other ids are skipped and kept.  populateNodes(populateClosest = true) on an empty hash turns
 * the points into the new node list (a point closer than min_distance_between_two_frontier_nodes to an earlier kept point of the 3 x 3
 * cells around it is dropped; a node anchored to two key frames may become two nodes).  A cell that comes to hold more than 20 nodes:
 * FS_E_RANGE, the node list as the reference's hash is left when it throws (up to and including that node) with no key node and no edge.
 * nz > 1: FS_E_INVALID; no grid staged: FS_E_STATE.
 * fs_roadmap_get_anchors: the pending nodes and the anchors in the order fs_roadmap_optimize consumes them (every id, present or
 * not), kf_id [n_records], point_c [n_records][3]; call with NULL arrays for the sizes. */
int fs_roadmap_set_keyframes(fs_ctx *ctx, int32_t n, const int32_t *kf_id, const double *pose7, int32_t *n_anchored, int32_t *n_orphaned);
int fs_roadmap_optimize(fs_ctx *ctx);
int fs_roadmap_get_anchors(fs_ctx *ctx, int32_t *n_pending, int64_t *n_records, int32_t *kf_id, float *point_c);

/* ---------------------------------------------------------------- next goal (FullPathOptimizer::getNextGoal) */
/* FullPathOptimizer::getNextGoal (DEP/src/FullPathOptimizer.cpp:548-661) on the roadmap the context holds.
 * Inputs: the frontier list as fs_roadmap_plan left it — goal_xyz [n][3], path_length_m [n], achievable [n], blacklisted [n] (may be
 * NULL) — and blacklist_xy [n_blacklist_circles][2], the circle centres isInBlacklistedRegion tests (distance < 1.7 m).
 * getFilteredFrontiersN (:157-227) splits the eligible frontiers into at most n_local (1..12; the reference's 5) locals of path length
 * <= local_radius (the reference's 12.0) and globals, with every quirk of the reference; ties in path length go to the lower index.
 * The pair lengths over the nodes [robot, locals in selection order, closest global] are getPlan(i, true, j, true) for i < j — by
 * the context's roadmap search (fs_set_roadmap_search): one shortest-path tree per source, all in one launch, or the reference's A*
 * from closest(i) to closest(j) per distinct pair —, 0 for equal points, local_radius * 100000 where there is no path; the tour search tries every
 * order of the locals (robot -> locals -> closest global) and keeps the shortest, ties to the shortest robot leg, then the first
 * order in lexicographic order of the selection positions.  fi_pose7 NULL: use_fi false; otherwise isRobotPoseSafe on it through the
 * info-only scorer (unsafe unless info_ref > fi_threshold) on the reference's two branches.
 * Outputs: next_index (-1: the reference's zero frontier), status (0 SAFE, 1 UNSAFE, 2 UNDETERMINED), tour [<= n_local + 1] and
 * tour_size (the locals in visiting order, then the closest global; without locals only the closest global; 0 with the zero
 * frontier), tour_length (the winning length; 0 when no tour was searched), n_tied (tours of that length; 0 when none was searched).
 * selection [n] (may be NULL): 1 local, 2 global, 0 in neither list (not eligible, or a local the reference drops), | 4 on the
 * closest global.  pair_length_m (may be NULL): room for (n_local + 2)^2; with k >= 1 locals the (k + 2)^2 symmetric matrix is
 * written row-major (row 0: the robot's lengths, calculateLengthRobotToGoal).  No roadmap node: FS_E_STATE; n_local outside 1..12:
 * FS_E_INVALID.  One synchronisation (plus the scorer's own when the FI check runs, and the round polling of roadmaps too large
 * for one workgroup per tree). */
int fs_roadmap_next_goal(fs_ctx *ctx, const double robot_pose7[7], int32_t n, const double *goal_xyz, const double *path_length_m,
                         const uint8_t *achievable, const uint8_t *blacklisted, int32_t n_blacklist_circles, const double *blacklist_xy,
                         int32_t n_local, double local_radius, const double *fi_pose7, double fi_threshold, int32_t *next_index,
                         int32_t *status, int32_t *tour, int32_t *tour_size, double *tour_length, int64_t *n_tied, uint8_t *selection,
                         double *pair_length_m);

/* ---------------------------------------------------------------- leg refinement (computePathBetweenPointsThetaStar) */
/* The path the robot drives: computePathBetweenPointsThetaStar (DEP/src/Helpers.cpp:540-588; FullPathOptimizer::refineAndPublishPath
 * and getNextGoal's per-leg plans) for n legs on the staged 2-D grid.  start_xy, goal_xy [n][2] world.  Parameters as the reference's
 * ThetaStar: allow_unknown, w_euc (> 0; the reference's 1), w_traversal (>= 0; 2), corners (4 or 8: a prefix of moves[]; 8).
 * Restated as data-parallel work: one converged fp64 cost field per distinct start cell — kept per context for
 * (grid, start cell, allow_unknown, weights, corners) until fs_upload_grid, fs_upload_grid_bricks or fs_update_grid_region —, the
 * descent from the goal in moves[] order, Theta*'s resetParent rule along the descent with line-of-sight sums taken as exact integers.
 * Outputs [n]: status (0 path, 1 start off the map, 2 goal off the map, 3 start unsafe, 4 goal unsafe, 5 no path), cost (the goal's
 * g; DBL_MAX without a path), n_vertices, n_poses (0 without a path).  vertex_xy [sum n_vertices][2]: the any-angle vertices of each
 * leg, start first, goal last, at cell centres; pose_xy [sum n_poses][2]: ThetaStar::backtrace + linearInterpolation at the costmap
 * resolution, the published poses; legs back to back in input order.  Either may be NULL: call first with both NULL for the counts.
 * A bad leg does not fail the call; nz > 1: FS_E_INVALID.  One synchronisation, plus the round polling of fields not cached. */
int fs_refine_paths(fs_ctx *ctx, int32_t n, const double *start_xy, const double *goal_xy, int32_t allow_unknown, double w_euc,
                    double w_traversal, int32_t corners, int32_t *status, double *cost, int32_t *n_vertices, double *vertex_xy,
                    int32_t *n_poses, double *pose_xy);
/* How fs_refine_paths plans a leg, per context.  FS_REFINE_SEARCH_FIELD (a fresh context's): the restatement above.
 * FS_REFINE_SEARCH_REFERENCE: the reference's own search, ThetaStar::generatePath as it runs — a binary heap of
 * nodes whose f is rewritten in place and never re-sifted, popped in libstdc++'s exact order; resetParent with the fp64 left fold of
 * the line-of-sight terms; the strict f test of setNeighbors; and the loop that never examines the entry it popped last, so a leg
 * whose search ends that way (every one-cell corridor) has status 5 here where the FIELD search finds a path.  One wavefront per
 * distinct (start cell, goal cell) of the call.  fs_refine_paths keeps its signature: status as above; cost = the goal record's g;
 * vertex_xy = the parent chain at cell centres, start first, the goal once; pose_xy = backtrace + linearInterpolation as the
 * reference publishes them, interpolated by the host library with std::hypot.  status, vertices and poses equal the reference's
 * compiled planner bit for bit, cost equals the CPU restatement (tests/thetastar_ref).  Every hypot of the search is read from a
 * table the host library fills with its own libm per grid shape (8 B per cell).  One deviation: a line-of-sight cell off the map is
 * unsafe (the reference reads outside its array for a straight walk along row or column 0).  Nothing is cached across calls; the
 * fields of the FIELD search and fs_refine_field are untouched.  A side above 4096 cells: FS_E_INVALID.  One synchronisation (one
 * more in the first call on a grid shape, for the table).  Any other value: FS_E_INVALID, the setting unchanged.
 * fs_set_option: "refine.search_slots" (0: as many searches side by side as "refine.search_bytes", default 1 GiB, holds, at about
 * 45 B per cell each; a positive value is the slot count itself) — results are identical for every slot count. */
#define FS_REFINE_SEARCH_FIELD 0
#define FS_REFINE_SEARCH_REFERENCE 1
int fs_set_refine_search(fs_ctx *ctx, int32_t search);
/* the cost field fs_refine_paths descends from start_xy, [ny][nx] double (DBL_MAX where not reached; everywhere for an unsafe start):
 * for tests and visualisation; the same whatever fs_set_refine_search says.  Start off the map: FS_E_INVALID */
int fs_refine_field(fs_ctx *ctx, const double start_xy[2], int32_t allow_unknown, double w_euc, double w_traversal, int32_t corners,
                    double *g);

/* ---------------------------------------------------------------- multi-robot task allocation (TaskAllocator) */
/* The reference's shared TaskAllocator (DEPX/frontier_multirobot_allocator: taskAllocator.cpp:7-66, minPos/minPos.cpp:20-44,88-98,
 * hungarian/Hungarian.cpp:25-395), which ProcessFrontierCostsBT feeds with every robot's cost and distance rows
 * (DEP/src/ExplorationBT.cpp:418) and GetAllocatedGoalBT solves (:842-859).  cost and distance are [n_robots][n_tasks] row-major,
 * robot-major as addRobotTasks pushes the rows.
 * FS_ALLOC_HUNGARIAN: HungarianAlgorithm::Solve on cost.  FS_ALLOC_MINPOS: P[i][j] = robots k != i with distance[k][j] <
 * distance[i][j] (strict), the modified matrix = cost where P == 0 and DBL_MAX elsewhere, Solve on the modified matrix.
 * Semantics are the reference's bit for bit: Buehren's Munkres with its scan orders — rows (n_robots <= n_tasks) or columns reduced
 * by their minimum, greedy stars in ascending order, step 3's passes over the columns in ascending order (first uncovered zero row of
 * each uncovered column; a column uncovered to the right is still visited in the same pass), step 4's path on the stars as they were,
 * step 5's h = smallest uncovered entry, added to every covered row and THEN subtracted from every uncovered column — and its zero
 * test fabs(x) < DBL_EPSILON everywhere.  assignment [n_robots]: the robot's task, -1 = none (more robots than tasks).  total_cost:
 * the assigned entries of the matrix that was solved (the modified one under MINPOS) summed in ascending robot order; +inf when two
 * of them are DBL_MAX, as in the reference.  rank, modified_cost [n_robots][n_tasks] (may be NULL; written under MINPOS only):
 * P and the modified matrix.
 * One workgroup runs the whole solve in one launch; one transfer each way and one synchronisation.
 * Limits and deliberate deviations from the reference, each FS_E_INVALID with nothing written:
 *   - n_robots outside 1..FS_ALLOC_MAX_ROBOTS, n_tasks outside 1..FS_ALLOC_MAX_TASKS (the reference has no limit; an empty matrix
 *     is undefined behaviour there);
 *   - an entry of cost (or, under MINPOS, of distance) that is NaN or +-inf (the reference would compute inf - inf); DBL_MAX is
 *     allowed — it is what U1 gives a dead frontier and what MinPos writes;
 *   - a negative entry (the reference prints a warning and goes on);
 *   - FS_ALLOC_MINPOS without distance (the reference's allocator always holds both matrices).
 * FS_E_RANGE: step 5 ran more than (n_robots + 1) * (min(n_robots, n_tasks) + 1) times — in exact arithmetic every run leads to a
 * row cover or an augmentation, which bounds the count by that product; the reference would loop on.  Nothing written.
 * Counters 1030-1032 (fs_get_counter): augmentations, step-5 runs, step-3 primes of the last solve. */
#define FS_ALLOC_HUNGARIAN 0   /* TaskAllocator::solveAllocationHungarian */
#define FS_ALLOC_MINPOS    1   /* TaskAllocator::solveAllocationMinPos    */
#define FS_ALLOC_MAX_ROBOTS 64
#define FS_ALLOC_MAX_TASKS  4096
int fs_allocate_tasks(fs_ctx *ctx, int32_t n_robots, int32_t n_tasks, const double *cost, const double *distance, int32_t method,
                      int32_t *assignment, double *total_cost, int32_t *rank, double *modified_cost);
/* The same with device pointers, enqueued on the context's stream and not waited for.  d_status [1]: FS_OK, FS_E_INVALID (an entry
 * refused) or FS_E_RANGE as above, with nothing else written unless FS_OK — read it together with the results.  The argument
 * checks (sizes, method, null pointers, MINPOS without d_distance) are made on the host and returned. */
int fs_allocate_tasks_dev(fs_ctx *ctx, int32_t n_robots, int32_t n_tasks, const double *d_cost, const double *d_distance, int32_t method,
                          int32_t *d_assignment, double *d_total_cost, int32_t *d_rank, double *d_modified_cost, int32_t *d_status);
/* One exploration tick of a fleet on one shared map: the cost and distance rows of n_robots robots at robot_pose7 [n_robots][7]
 * for the n frontiers, and the allocation on them, in one call.  Row r of weighted_cost, path_length_m and achievable
 * [n_robots][n] (each may be NULL) is, bit for bit, what fs_get_frontier_costs_roadmap(ctx, robot_pose7[r], ...,
 * with_fisher_information = 0, ...) gives that robot — weighted_cost, path_length_m and its records' achievable flag — under the
 * context's roadmap search (fs_set_roadmap_search), TREE or REFERENCE; assignment [n_robots] and total_cost are fs_allocate_tasks
 * on those rows with distance = path_length_m (the response's frontier_distances from getPathLengthInM, DEP/src/CostAssigner.cpp:96).
 * assigned_cost [n_robots]: weighted_cost[r][assignment[r]] — DBL_MAX = a dead frontier was assigned, NaN for -1.  records [n] (may
 * be NULL): the arrival records of the list, scored ONCE with achievable_in = all (a robot's own call also clears the achievable flag
 * where its plan fails — achievable[r] is that flag; nothing else differs).
 * On the device: arrival information once for the list; one shortest-path tree per DISTINCT start node (robots that share a
 * closest key node share a tree) in batched launches of up to 13 trees, in buffers of the call's own — the single-robot tree cache
 * is neither read nor replaced; one plan launch over n_robots x n; per robot the normalisation over ITS live set (not blacklisted,
 * record achievable, its plan achievable) and the U1 cost; MinPos and the solve on the matrix where it lies.  One transfer in, one
 * out, one synchronisation; the matrices visit the host only when asked for.  Under FS_ROADMAP_SEARCH_REFERENCE the A* queries are
 * enqueued and settled robot by robot (one synchronisation per robot).  A robot without a start node gets a DBL_MAX row, which the
 * solve takes as the reference would.  n_robots > n is allowed: some robots get -1.
 * FS_E_INVALID: fs_allocate_tasks' limits on n_robots and n (n = 0 included) and method.  FS_E_RANGE: U1 out of bounds for any
 * robot, as in fs_get_frontier_costs, or the solve's step-5 cap.  Otherwise refuses what fs_get_frontier_costs_roadmap refuses. */
int fs_fleet_allocate_roadmap(fs_ctx *ctx, int32_t n_robots, const double *robot_pose7, int32_t n, const double *goal_xyz,
                  const int32_t *frontier_size, const uint8_t *blacklisted, double alpha, double beta, double max_vx, double max_wz,
                  int32_t method, int32_t *assignment, double *total_cost, double *assigned_cost, fs_record *records,
                  double *weighted_cost, double *path_length_m, uint8_t *achievable);

/* ---------------------------------------------------------------- sensor sweep on a ground-truth world (closed loop)
 *
 * THIS PROJECT'S OWN EXTENSION.  The reference's map comes from its depth camera and the traversability mapper, both outside the
 * vendored tree; it closes the exploration loop only in simulation and measures it with comparision_scripts/
 * explored_map_counter.cpp (known cells per second).  Here the arrival fan (DEP/src/CostCalculator.cpp:23-121) — the reference's
 * PREDICTION of what a camera at a goal would reveal — is walked through a ground-truth WORLD grid instead, and what it sees is
 * copied into the staged map on the device: a map update that never crosses the bus, and the first check of `arrival` against
 * what is actually seen. */

/* The ground truth: same costs, shape, origin and resolution as the staged grid; dense in HBM next to it (the 2^32-cell limit
 * applies).  No grid staged: FS_E_STATE.  A shape other than the staged grid's: FS_E_INVALID, nothing changed.  cells == NULL
 * releases it.  A later fs_upload_grid / fs_upload_grid_bricks with ANOTHER shape drops it, the same shape keeps it;
 * fs_update_grid_region never touches it. */
int fs_upload_world(fs_ctx *ctx, const uint8_t *cells, int32_t nx, int32_t ny, int32_t nz);

/* One sweep from each of n poses.  The fan is exactly the arrival fan of `sensor` (validated as fs_set_ray_params validates; its
 * direction table is cached in the context until a different one arrives) or, sensor == NULL, of the context's ray parameters:
 * accumulated theta, end point sx + depth cos(e) cos(theta) clamped as fs_score_arrival clamps it, max_length =
 * (unsigned)(depth / resolution), getTracedCells' walk with its end + 1 visits.  Fields used: max_camera_depth, delta_theta,
 * camera_fov, n_rays, n_elev, elev, obst_*, trace_*, polygon.
 *   rays of pose p   first_ray[p] == -1, or first_ray == NULL: all n_yaw rays (a lidar); otherwise the window =
 *                    (int)(camera_fov / delta_theta) rays starting there — what `argmax` of the scoring calls names.  A value
 *                    outside [-1, n_yaw - window]: FS_E_INVALID, nothing written.
 *   per used ray     visits go in order through the WORLD.  Every visited cell is seen; the first visited cell whose world cost
 *                    lies in [obst_min, obst_max] is seen too (the camera sees the wall's face) and ends the ray.
 *                    ray_unknown [n][n_elev][n_yaw] (may be NULL) = the visits BEFORE that blocking visit whose STAGED cost
 *                    before the call lies in [trace_min, trace_max]; unused rays get 0.  seen_unknown [p] = the sum over the
 *                    pose's used rays: the figure to hold against `arrival`.
 *   off the map      a pose whose own worldToMap fails, or any of whose USED rays' end points fails, sees nothing at all, as the
 *                    arrival fan aborts (CostCalculator.cpp:50-55): status FS_STATUS_OFF_MAP, counts 0.  Every other pose:
 *                    FS_STATUS_OK.
 * After all poses: staged[cell] = world[cell] for every cell seen by any pose, no other cell changes; *n_seen = distinct seen
 * cells; *n_revealed = those that were 255 before and whose world cost is not 255; window = x0 y0 z0 sx sy sz, the bounding box
 * of the seen cells (sizes 0 when nothing was seen).  n_seen, n_revealed, window, ray_unknown may be NULL.  The context then does
 * what fs_update_grid_region does for that window: stored keep-out zones are painted again inside it, derived images are re-cut
 * for the bricks it touches, cached arrival limits stay.  Every figure is an integer that does not depend on the order the
 * device works in.  n == 0, or nothing seen: a no-op that returns FS_OK.  No world staged: FS_E_STATE.  2-D and 3-D grids. */
int fs_sense(fs_ctx *ctx, int32_t n, const double *origin_xyz /* [n][3] */, const int32_t *first_ray /* [n] or NULL */,
             const fs_ray_params *sensor /* NULL: the context's ray parameters */,
             int32_t *ray_unknown /* [n][n_elev][n_yaw] or NULL */, int32_t *seen_unknown /* [n] */, int32_t *status /* [n] */,
             int64_t *n_seen, int64_t *n_revealed, int32_t window[6] /* x0 y0 z0 sx sy sz, may be NULL */);

/* Replaces CheckIfGoalMapped -> surroundingCellsMapped (DEP/src/Helpers.cpp:98-133) for a batch of goals on the staged 2-D grid
 * (nz == 1).  mapped [i], in this order: goal off the map -> 0; its cell is 254 -> 1; three or more of its nhood8 cells are
 * 254 -> 1; otherwise 0 if any cell of nhood20 (nhood4 plus the nhood8 of each of those, clipped at the map's edges as
 * Helpers.cpp:186-275 clips them; the cell itself is among them) is 255, else 1. */
int fs_goals_mapped(fs_ctx *ctx, int32_t n, const double *goal_xyz /* [n][3] */, uint8_t *mapped /* [n] */);

/* The explored-cell counter's figure (comparision_scripts/explored_map_counter.cpp) on the staged grid: counts = cells known
 * (!= 255; OccupancyGrid -1 corresponds to 255), unknown (== 255), lethal (== 254), free (== 0). */
int fs_grid_census(fs_ctx *ctx, int64_t counts[4] /* known (!= 255), unknown (== 255), lethal (== 254), free (== 0) */);

/* ---------------------------------------------------------------- driving through the world (closed loop)
 *
 * THIS PROJECT'S OWN EXTENSION, built on fs_sense.  In the reference the robot is driven by its controller server, its map grows
 * from the depth camera while it drives, and CheckIfGoalMapped ends a goal in mid-drive; none of that is in the vendored tree.
 * Here n_robots robots drive their lists of STATIONS (poses cut from a planned path) through the world, sensing at every station
 * and stopping on their own, with every decision taken on the device: one call, one wait, however many stations.
 *
 * Robot r has n_stations[r] >= 1 stations, station_xyz holds the robots' lists back to back, first_ray (may be NULL) one entry
 * per station with fs_sense's meaning and validation.  Steps k = 0 .. max n_stations - 1; all robots still driving move in
 * lockstep, and every step's moves see the staged map as step k - 1 of ALL robots left it:
 *   1 move (k >= 1)  a robot without a station k stops, FS_DRIVE_ARRIVED.  Otherwise the segment station k - 1 -> station k is
 *                    walked as fs_trace_segments walks it, uncapped (max_length_cells = nx + ny), and in this order: a
 *                    worldToMap failure stops the robot FS_DRIVE_OFF_MAP; any visited STAGED cost in [block_min, block_max]
 *                    (stored keep-out zones are painted there) FS_DRIVE_BLOCKED; otherwise any visited WORLD cost in that range
 *                    FS_DRIVE_COLLIDED — it drove into something it had not seen; otherwise reached[r] = k.  A stopped robot
 *                    stays at station reached[r] and does nothing more.
 *   2 sense          the robots still driving sweep from their station k exactly as ONE fs_sense call over those poses would
 *                    (counts against the staged map before this step's merge): station_status = FS_STATUS_OK / FS_STATUS_OFF_MAP,
 *                    seen_unknown as fs_sense's.  A station that sees nothing does not stop the robot.
 *   3 merge          as fs_sense: staged = world on the cells seen in this step, stored keep-out zones painted again.
 *   4 goal           with stop_when_mapped, a robot whose goal fs_goals_mapped now calls mapped stops, FS_DRIVE_MAPPED.
 * A robot still driving after the last step has run out of stations: FS_DRIVE_ARRIVED.
 * status, reached [n_robots]; station_status, seen_unknown one entry per station: -1 and 0 for a station never reached (station
 * 0 always is).  *n_seen = the sum over the steps of the step's distinct seen cells, *n_revealed likewise — both equal the sums of
 * the equivalent fs_sense calls; window = the bounding box of everything seen (sizes 0: nothing).  These three may be NULL.
 * Every figure is an integer sum, minimum or maximum and depends neither on the order of the robots nor on the device's.
 * At the end the context does once what fs_update_grid_region does, for a window that holds everything the drive touched.
 * Decided before anything is written: no grid, no world, no ray parameters (and no sensor): FS_E_STATE; nz > 1, a first_ray
 * outside [-1, n_yaw - window], n_stations[r] < 1 or > FS_DRIVE_MAX_STATIONS, n_robots > FS_DRIVE_MAX_ROBOTS: FS_E_INVALID.
 * n_robots == 0: a no-op.  params == NULL: block 253..254 (isConnectable's visitor), stop_when_mapped 1.  Landmarks are not
 * sensed on the way: run fs_sense_landmarks on the reached stations afterwards, or drive with fs_drive_slam (below). */
#define FS_DRIVE_ARRIVED  0   /* out of stations */
#define FS_DRIVE_BLOCKED  1   /* the staged map shows something in the block range on the next segment */
#define FS_DRIVE_COLLIDED 2   /* only the world does */
#define FS_DRIVE_OFF_MAP  3   /* an end of the next segment is off the map */
#define FS_DRIVE_MAPPED   4   /* the goal is mapped (stop_when_mapped) */
#define FS_DRIVE_MAX_STATIONS 2048
#define FS_DRIVE_MAX_ROBOTS   4096

typedef struct fs_drive_params {
    int32_t block_min, block_max;  /* the costs that stop a move */
    int32_t stop_when_mapped;
} fs_drive_params;

int fs_drive(fs_ctx *ctx, int32_t n_robots, const double *station_xyz /* [sum n_stations][3] */, const int32_t *n_stations /* [n_robots] */,
             const int32_t *first_ray /* [sum n_stations] or NULL */, const double *goal_xyz /* [n_robots][3] */,
             const fs_ray_params *sensor /* NULL: the context's ray parameters */, const fs_drive_params *params /* NULL: the defaults */,
             int32_t *status /* [n_robots] */, int32_t *reached /* [n_robots] */, int32_t *station_status /* [sum n_stations] */,
             int32_t *seen_unknown /* [sum n_stations] */, int64_t *n_seen, int64_t *n_revealed,
             int32_t window[6] /* x0 y0 z0 sx sy sz, may be NULL */);

/* ---------------------------------------------------------------- landmark sensor on a ground-truth cloud (closed loop)
 *
 * THIS PROJECT'S OWN EXTENSION, the other half of fs_sense.  In the reference the map points behind every Fisher-information
 * figure come from the ORB-SLAM3 wrapper (GetLandmarksInView, FIP/src/fisher_information/FisherInfoManager.cpp:52-88), which is
 * outside the vendored tree.  Here a ground-truth WORLD cloud lives in HBM beside the world grid, the poses the robot visits see
 * parts of it, and the staged cloud — what fs_score_fim, fs_score_candidates and fs_landmarks_in_view read — is the part seen
 * so far, put into its order on the device, never crossing the bus. */

/* The world cloud: up to 2 000 000 points (fs_upload_landmarks' limit; more: FS_E_INVALID), kept on the device as raw xyz, in a
 * k-d leaf order of its own with one bounding sphere per 64-landmark chunk, and with one uint32 sighting counter (0) and one
 * `discovered` flag per landmark.  known [i] != 0 marks landmark i discovered from the start; NULL: none.  After the call the
 * staged cloud is exactly the known set, possibly empty, staged as described under fs_sense_landmarks.  A non-finite world
 * landmark, or one beyond 1e17 m (fs_upload_landmarks' usability test), keeps its index and is never seen.  xyz == NULL with
 * m_world == 0 releases the world cloud and leaves the staged cloud alone; xyz != NULL with m_world == 0 stages an empty world.
 * Needs neither a grid nor a lookup table.  NULL context, m_world < 0, xyz == NULL with m_world > 0: FS_E_INVALID. */
int fs_upload_world_landmarks(fs_ctx *ctx, const float *xyz /* [m_world][3] */, int32_t m_world,
                              const uint8_t *known /* [m_world] or NULL */);

typedef struct fs_landmark_sensor {
    double  max_dist, max_angle;   /* validated as fs_set_fim_params validates them */
    int32_t line_of_sight;         /* 0: predicate only; 1: also the line of sight through the WORLD grid */
    int32_t min_views;             /* >= 1: sightings (all calls together) before a landmark counts as discovered */
    int32_t occ_min, occ_max;      /* as fs_occlusion_params */
    double  end_margin_m;
} fs_landmark_sensor;

/* One sweep of the world cloud from each of n poses.  Pose p SEES world landmark i when
 *   - the visibility predicate of fs_set_fim_params accepts it under the sensor's volume: the same getTransformFromPose
 *     conversion of pose7, the same fp32 transform and comparison as fs_score_fim and fs_landmarks_in_view, and
 *   - with line_of_sight == 1, the line from the pose's float32 translation to the landmark's float32 position, both widened to
 *     double, is not blocked on the WORLD grid (fs_upload_world) under the rule of fs_set_occlusion, word for word: the uncapped
 *     walk, the start cell tested, the last 1 + (unsigned)(end_margin_m / resolution) cells at the landmark's end left out, an
 *     end off the map tests nothing, planar on nz == 1.
 * Every sighting adds 1 to the landmark's counter (modulo 2^32); identical poses count separately.  A landmark becomes
 * discovered when its counter reaches min_views and stays discovered for good.  n_in_view [p] (may be NULL) = landmarks pose p
 * sees, discovered before or not; *n_new (may be NULL) = landmarks that became discovered in this call; *n_discovered (may be
 * NULL) = the total afterwards.  Every figure is an integer sum that does not depend on the order the device works in; there is
 * no "who discovered it".
 *   sensor == NULL   fs_set_fim_params' volume, min_views 1, range and margin of fs_set_occlusion (its `enabled` is not
 *                    consulted), line_of_sight 1 if a world grid is staged, else 0.
 *   restaging        After the sweep the staged cloud is rebuilt — on the device — if anything became discovered or if the staged
 *                    cloud is not currently the discovered set (fs_upload_landmarks was called in between: that call leaves the
 *                    world cloud, counters and flags alone).  The discovered landmarks' raw xyz are compacted in ascending world
 *                    index and staged as fs_upload_landmarks stages that array under "cloud.order" 2, whatever the option says
 *                    and however small the set; an empty set is staged as fs_upload_landmarks(ctx, NULL, 0) stages it.  The
 *                    only host traffic is the poses in, the counts out and one read-back of the discovered count.  Afterwards
 *                    "upload index" in fs_landmarks_in_view means rank in the discovered set; fs_world_landmarks_get maps rank
 *                    to world index.
 * FS_E_INVALID, nothing changed or written: NULL context, n < 0, pose7 == NULL with n > 0, an invalid sensor (volume, min_views
 * < 1, line_of_sight other than 0 / 1, cost range or margin as fs_set_occlusion refuses them).  FS_E_STATE, nothing changed or
 * written: no world cloud staged; line_of_sight == 1 with no world grid staged (also after fs_upload_grid of another shape has
 * dropped it).  n == 0 returns FS_OK and changes nothing (*n_new = 0, *n_discovered = the total as it stands). */
int fs_sense_landmarks(fs_ctx *ctx, int32_t n, const double *pose7 /* [n][7] */,
                       const fs_landmark_sensor *sensor /* NULL: see above */,
                       int32_t *n_in_view /* [n] or NULL */, int32_t *n_new /* or NULL */, int32_t *n_discovered /* or NULL */);

/* The state of the world cloud: its size, the number of discovered landmarks, their world indices in ascending order (entry r is
 * the landmark fs_landmarks_in_view calls r while the staged cloud is the discovered set) and every landmark's sighting counter.
 * Each pointer may be NULL.  No world cloud staged: FS_E_STATE. */
int fs_world_landmarks_get(fs_ctx *ctx, int32_t *m_world, int32_t *n_discovered,
                           int32_t *world_index /* [n_discovered] ascending, or NULL */,
                           int32_t *views /* [m_world] or NULL */);

/* The staged landmark cloud as the kernels read it: m landmarks in n_chunks chunks of 64; soa [3][n_chunks * 64] = x, y, z in k-d
 * leaf order with the far-away sentinels in the padding; spheres [n_chunks][4]; perm [n_chunks * 64] = the landmark's position in the
 * staged array per slot, -1 for a sentinel.  Every pointer may be NULL (call once for the sizes).  A read-back like
 * fs_read_grid_region: what two routes that claim to stage the same cloud (fs_upload_landmarks with the device ordering,
 * fs_sense_landmarks) are held to, byte for byte — the Fisher float sums are not bit-stable from call to call even on one cloud.  No cloud staged: FS_E_STATE. */
int fs_staged_cloud_get(fs_ctx *ctx, int32_t *m, int32_t *n_chunks, float *soa, float *spheres, int32_t *perm);

/* ---------------------------------------------------------------- a drive gated on Fisher information (closed loop)
 *
 * THIS PROJECT'S OWN EXTENSION, fs_drive with the behaviour FIT-SLAM is named for: in the reference the robot evaluates isPoseSafe
 * at its current pose on every behaviour-tree iteration while it is under way (EvaluateFisherInformation), and an unsafe pose ends
 * the goal.  fs_drive_slam is fs_drive — same stations, moves, sweeps, merges, goal test, outputs and refusals — whose stations
 * are POSES: station_pose7 [sum n_stations][7] = xyz + quaternion xyzw; the xyz part is fs_drive's station_xyz, the full pose
 * (through getTransformFromPose, as fs_sense_landmarks and fs_score_fim convert it) is what the landmark sensor and the gate use.
 * After fs_drive's steps 1 move, 2 sense and 3 merge of step k, for the robots that sensed in this step:
 *   3b landmark sweep  exactly as ONE fs_sense_landmarks call with lm_sensor over those robots' station-k poses: +1 per sighting,
 *                      station_in_view = that call's n_in_view, a landmark whose counter reaches min_views is discovered for
 *                      good, line_of_sight walks the WORLD grid.  All robots' sightings of the step land before anybody is scored.
 *   3c information     station_information / station_voxels = what fs_score_fim returns as info_ref / n_voxels for the pose on a
 *                      context whose staged cloud is the set discovered after 3b, whose staged grid is this context's after step
 *                      3's merge and whose fs_set_fim_params, lookup table and fs_set_occlusion are this context's (with
 *                      occlusion enabled: the line-of-sight rule on the STAGED grid).  The integer is equal; the float agrees to
 *                      rounding (fs_score_fim's own sums are not bit-stable from call to call).
 *   4  goal            as fs_drive: FS_DRIVE_MAPPED.
 *   5  gate            with gate != 0 and k >= gate_first_station, a robot still driving whose information is not
 *                      > information_threshold (isPoseSafe's `total > threshold`, on the float reported) stops at station k,
 *                      FS_DRIVE_UNSAFE.  MAPPED wins over UNSAFE in the same step.  Stations before gate_first_station are swept
 *                      and reported but never stop the robot (the reference spins in place to initialise before it judges).
 * After the last step the staged cloud becomes the discovered set ONCE, by fs_sense_landmarks' restaging rule (something was
 * discovered, or the staged cloud is not currently that set); the steps themselves read the world cloud and its flags and never
 * restage.  *n_new / *n_discovered are fs_sense_landmarks' figures for the whole call.  The host waits once for the drive and
 * once more when it restages, however many stations and robots.
 * station_information, station_voxels, station_in_view: one entry per station, 0, 0 and -1 for a station never reached; each may
 * be NULL, and so may n_new and n_discovered.  Marking the zone lethal after an UNSAFE stop (fs_mark_lethal_fov) is the caller's step.
 * params == NULL: fs_drive's defaults, threshold 550.0 (the value the reference's plugin constructor forces), gate 1,
 * gate_first_station 1.  lm_sensor == NULL: fs_sense_landmarks' defaults.
 * Refused before anything is written, counters included, in this order: fs_drive's refusals; no world cloud: FS_E_STATE; no lookup
 * table: FS_E_STATE; an invalid lm_sensor (as fs_sense_landmarks refuses it), gate other than 0 / 1, gate_first_station < 0 or a
 * non-finite threshold: FS_E_INVALID.  n_robots == 0: a no-op, *n_new = 0, *n_discovered = the total as it stands. */
#define FS_DRIVE_UNSAFE   5   /* the pose's information is not above the threshold (fs_drive_slam) */

typedef struct fs_drive_slam_params {
    int32_t block_min, block_max;  /* fs_drive_params' fields */
    int32_t stop_when_mapped;
    int32_t gate;                  /* 0: sweep and report, never stop for information; 1: stop */
    double  information_threshold;
    int32_t gate_first_station;    /* stations with a smaller index never stop the robot */
} fs_drive_slam_params;

int fs_drive_slam(fs_ctx *ctx, int32_t n_robots, const double *station_pose7 /* [sum n_stations][7] */, const int32_t *n_stations /* [n_robots] */,
                  const int32_t *first_ray /* [sum n_stations] or NULL */, const double *goal_xyz /* [n_robots][3] */,
                  const fs_ray_params *sensor /* NULL: the context's ray parameters */, const fs_landmark_sensor *lm_sensor /* NULL: see above */,
                  const fs_drive_slam_params *params /* NULL: the defaults */,
                  int32_t *status /* [n_robots] */, int32_t *reached /* [n_robots] */, int32_t *station_status /* [sum n_stations] */,
                  int32_t *seen_unknown /* [sum n_stations] */, float *station_information /* [sum n_stations] or NULL */,
                  int32_t *station_voxels /* [sum n_stations] or NULL */, int32_t *station_in_view /* [sum n_stations] or NULL */,
                  int64_t *n_seen, int64_t *n_revealed, int32_t window[6] /* x0 y0 z0 sx sy sz, may be NULL */,
                  int32_t *n_new /* or NULL */, int32_t *n_discovered /* or NULL */);

#ifdef __cplusplus
}
#endif
#endif
