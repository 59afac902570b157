// fs_internal.h — structures shared by the HIP kernels and the C-ABI host layer (not installed).
#ifndef FS_INTERNAL_H_
#define FS_INTERNAL_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <vector>

#include "../../include/fitslam_frontier.h"
#include "../../include/fitslam_frontier_dev.h"

// Instrumentation paths (cycle stamps, schedule recorder, range checks) exist in FS_DEV builds only — the
// builds fit-slam_amd/_build.py makes under a library name of their own when one of its FS_* knobs is set.
#ifndef FS_DEV
#undef FS_FIM_STAMPS
#undef FS_FIM_STAMPS_PER_WAVE
#undef FS_FIM_SCHEDULE
#undef FS_FIM_BOUNDS
#undef FS_RAY_BOUNDS
#endif

// ---- ray-march kernel arguments ---------------------------------------------------------------
// The occupancy grid lives in HBM as the dense row-major image [nz][ny][nx] the uploads write — what short rays, the
// footprint disc, the segment tracer and the frontier-cell stencil read — and, for long rays, as the CLASS image: what the
// arrival visitor needs of a cell is two bits — in the trace range? in the obstacle range? (Helpers.hpp:64-71) — so the grid is
// classified once per (map, visitor ranges) and packed 16 cells to a dword in bricks of 8 x 8 x 8 cells = 128 B = one cache
// line: cell (x, y, z) is 2-bit field A & 15 of dword A >> 4,
//     A = x + (x >> 3) * cls_m[0] + (y << 3) + (y >> 3) * cls_m[1] + (z << 6) + (z >> 3) * cls_m[2]
// (brick-linear order [z >> 3][y >> 3][x >> 3], cell order [z & 7][y & 7][x & 7]; 512^3 -> 32 MiB).
struct FsGridDev {
    const uint8_t *cells;      // [nz][ny][nx]
    int32_t nx, ny, nz;
    double ox, oy, oz;         // origin
    double res;
    unsigned long long *dbg;   // range-checked builds (FS_BOUNDS=1): where a walk that left the grid is recorded
    const uint32_t *cls;       // class image, or nullptr while it has not been cut
    uint32_t cls_m[3];         // 512 - 8, 512 * bricks_x - 64, 512 * bricks_x * bricks_y - 512  (brick stride of the axis minus 8 << l)
    uint32_t cls_cells;        // cells the image holds (padded to whole bricks)
    // SPARSE form of the class image ("ray.layout" 3; BASELINE.json configs[4] "sparse-hashed voxel grid"): `cls` is then a POOL of
    // 128-B bricks and cls_table[brick-linear index] the slot of the brick's content in it — slots 0..3 are the four uniform
    // bricks (every cell of one class: all-unknown, all-free, ...), shared by every brick of that content.  nullptr: dense.
    const uint32_t *cls_table;
};

// dwords of the class image of an nx x ny x nz grid, and the kernel that fills it (bit 0: cost in [trace_min, trace_max], bit 1: in [obst_min, obst_max])
size_t fs_class_image_words(int nx, int ny, int nz);
hipError_t fs_launch_classify(const uint8_t *d_cells, uint32_t *d_cls, int nx, int ny, int nz, int obst_min, int obst_max,
                              int trace_min, int trace_max, hipStream_t s);
// ... only the n_bricks[3] bricks from brick brick0[3] on (what a rewritten window of the map touches), and the kernel that puts
// a packed window [sz][sy][sx] into the row-major image at (x0, y0, z0): fs_update_grid_region
hipError_t fs_launch_classify_region(const uint8_t *d_cells, uint32_t *d_cls, int nx, int ny, int nz, int obst_min, int obst_max,
                                     int trace_min, int trace_max, const int brick0[3], const int n_bricks[3], hipStream_t s);
hipError_t fs_launch_window_scatter(const uint8_t *d_window, uint8_t *d_grid, int nx, int ny, int x0, int y0, int z0,
                                    int sx, int sy, int sz, hipStream_t s);
// ... and its mirror: the window at (x0, y0, z0) of the row-major image, packed [sz][sy][sx] (fs_read_grid_region)
hipError_t fs_launch_window_gather(const uint8_t *d_grid, uint8_t *d_window, int nx, int ny, int x0, int y0, int z0,
                                   int sx, int sy, int sz, hipStream_t s);

// keep-out zones (fs_keepout.hip).  mark: one lane per ray {ax, ay, ex, ey} of d_rays [n_rays][4], each walks
// its line (fs_keepout.h) and stores 1 into d_image [ny][nx]; a ray with an end off the map is skipped.  apply: over the
// rectangle [x0, x0+sx) x [y0, y0+sy) of a 2-D grid, cells[i] = src[i] ? 253 : cells[i]; d_count (may be NULL) += cells of src
// in the rectangle.  fold = the same for ONE zone rasterised into the scratch image d_src: its cells also enter the union
// mask d_mask and leave d_src, which is all zero again afterwards.
hipError_t fs_launch_keepout_mark(const int32_t *d_rays, int64_t n_rays, uint8_t *d_image, int nx, int ny, hipStream_t s);
hipError_t fs_launch_keepout_apply(const uint8_t *d_mask, uint8_t *d_cells, int nx, int ny, int x0, int y0, int sx, int sy,
                                   unsigned long long *d_count, hipStream_t s);
hipError_t fs_launch_keepout_fold(uint8_t *d_src, uint8_t *d_mask, uint8_t *d_cells, int nx, int ny, int x0, int y0, int sx, int sy,
                                  unsigned long long *d_count, hipStream_t s);

// the inflation layer (fs_inflate.hip) on the window [x0, x0+sx) x [y0, y0+sy) of a 2-D grid, R = the seeds' reach in
// cells (1 .. FS_INFLATE_MAX_CELLS).  The box: that window grown by R on every side and clipped to the map — where seeds are looked
// for and counted.  cell_radius: Costmap2D::cellDistance, -1 beyond the limit.  cost_table: InflationLayer::computeCost for every
// d2 = dx^2 + dy^2 in 0 .. R^2, on the host (libm's exp and sqrt).  rows: d_g [gh][sx] = distance along the row to the nearest
// seed (cell == 254) within R, 0xFFFF for none; *d_n_seeds += seeds in the box.  cols: every window cell whose nearest seed has
// d2 <= R^2 takes d_cost_by_d2[d2] under the layer's write rule; *d_n_changed += cells whose byte changed.
struct FsInflateBox {
    int32_t gx0, gy0, gw, gh;
};
inline FsInflateBox fs_inflate_box(int nx, int ny, int x0, int y0, int sx, int sy, int R)
{
    const int gx0 = x0 - R > 0 ? x0 - R : 0, gy0 = y0 - R > 0 ? y0 - R : 0;
    const long long gx1 = (long long)x0 + sx + R < nx ? (long long)x0 + sx + R : nx, gy1 = (long long)y0 + sy + R < ny ? (long long)y0 + sy + R : ny;
    return FsInflateBox{gx0, gy0, (int32_t)(gx1 - gx0), (int32_t)(gy1 - gy0)};
}
int fs_inflation_cell_radius(double inflation_radius, double res);
void fs_inflation_cost_table(const fs_inflation_params &p, double res, int R, uint8_t *cost_by_d2);
hipError_t fs_launch_inflate_rows(const uint8_t *d_cells, int nx, int ny, int x0, int y0, int sx, int sy, int R, uint16_t *d_g,
                                  unsigned long long *d_n_seeds, hipStream_t s);
hipError_t fs_launch_inflate_cols(const uint16_t *d_g, const uint8_t *d_cost_by_d2, uint8_t *d_cells, int nx, int ny, int x0, int y0,
                                  int sx, int sy, int R, int inflate_unknown, unsigned long long *d_n_changed, hipStream_t s);

struct FsRayArgs {
    FsGridDev grid;
    // fan geometry, precomputed on the host in double with libm (ray directions are
    // candidate-independent; device cos/sin could differ from libm in the last ulp and flip a
    // truncation at a cell boundary):  dir[(e*n_yaw + i)*3 + {0,1,2}] = D*cos(phi_e)*cos(theta_i), ... , D*sin(phi_e)
    const double *dir;
    int32_t n_yaw, n_elev, window;
    uint32_t max_length;       // (unsigned)(max_camera_depth / resolution), CostCalculator.cpp:28
    int32_t obst_min, obst_max, trace_min, trace_max;
    int32_t clamp;             // CostCalculator.cpp:47-48 (1) or setMaxArrivalInformation (0)
    int32_t layout;            // 0: row-major byte image (WalkLinear), 1: class image (WalkClass), 2: sparse class image (WalkSparse)
    double lo_x, hi_x, lo_y, hi_y, lo_z, hi_z;   // folded clamp bounds: max(poly_min, origin), min(poly_max, origin + sizeInMeters)
    double footprint_radius;   // ceil(robot_radius / resolution)
    double delta_theta, half_fov;
    double min_gt;             // min_arrival_info_gt_
    // candidates
    int32_t n;
    const double *goal;        // [n][3]
    const int32_t *frontier_size;   // or nullptr
    const uint8_t *blacklisted;     // or nullptr
    const uint8_t *achievable_in;   // or nullptr
    const int32_t *perm;            // spatial processing order (candidate ids) or nullptr; outputs stay in list order
    // outputs (device)
    int32_t *ray_counts;       // [n][n_elev][n_yaw] or nullptr
    int32_t *arrival, *argmax, *status;
    double *yaw;
    uint8_t *achievable;
    const float *yawR;         // [n_windows][9] rotation per argmax index (for pose12)
    float *pose12;             // [n][12] R (row-major) + t of the pose (goal, best yaw), or nullptr
    fs_record *records;        // [n] arrival-only records (Fisher columns zero), or nullptr: what fs_get_frontier_costs ranks when no FI is asked for
};

// ---- generic segment tracing (getTracedCells + a RayTracedCells visitor per segment)
struct FsSegArgs {
    FsGridDev grid;
    int32_t n;
    const double *start, *end;      // [n][3]
    double max_length;              // cells (the reference passes it as double)
    int32_t obst_min, obst_max, trace_min, trace_max;
    uint8_t *ok, *hit;
    int32_t *traced, *unknown, *all;
};
hipError_t fs_launch_segments(const FsSegArgs &a, hipStream_t s);
// ---- line of sight (fs_line_of_sight; the same rule inside the occluded FIM worker: fs_walk.h)
struct FsLosArgs {
    FsGridDev grid;
    int32_t n;
    const double *from, *to;        // [n][3]
    int32_t occ_min, occ_max;       // costs that block
    uint32_t margin;                // M = 1 + (unsigned)(end_margin_m / resolution): visits at the far end that are not tested
    uint8_t *ok, *blocked;
    int32_t *tested;                // or nullptr
};
hipError_t fs_launch_los(const FsLosArgs &a, hipStream_t s);
hipError_t fs_launch_brick_scatter(int64_t n_bricks, const int32_t *d_coords, const uint8_t *d_cells, uint8_t *d_grid,
                                   int nx, int ny, int nz, int *d_bad, hipStream_t s);
hipError_t fs_launch_frontier_pair(int n, const float *lx, const float *ly, const float *lz, int m, const float *d_Rt,
                                   const double *d_tri, float *d_out, hipStream_t s);
hipError_t fs_launch_frontier_cells(const uint8_t *d_grid, int nx, int ny, int nz, int lethal_threshold, uint8_t *d_mask,
                                    unsigned long long *d_count, hipStream_t s);

hipError_t fs_launch_frontier_clusters(const uint8_t *d_map, int nx, int ny, double ox, double oy, double res, double px, double py,
                                       int32_t start_pos, double reach, int32_t lethal_threshold, int32_t *d_parent_t, int32_t *d_parent_f,
                                       int32_t *d_aux, uint32_t *d_queue, uint8_t *d_visited, int32_t *d_state, int32_t *d_labels,
                                       int32_t max_clusters, fs_frontier_cluster *d_clusters, long long *d_sums, hipStream_t s);

// ---- frontier search tail (fs_search.hip): pieces and goal points of the components fs_launch_frontier_clusters
// found (launched with max_clusters = 0, so that aux[root] == -2 marks a found component).  Every scratch array holds nx * ny
// entries (emit_* / rec_base: max(nx * ny, n_seeds) + 1); state [16] zeroed before the launch.
struct fs_msort_elem;                     // fs_median_sort.h
// FSS_ERROR: 1 a refused caller seed, 2 a found component the outer search never met (internal)
enum { FSS_COMPONENTS = 0, FSS_EMITTED = 1, FSS_CELLS = 2, FSS_RECORDS = 3, FSS_ERROR = 4, FSS_LEVELS = 5, FSS_GUARDED = 6,
       FSS_OUTER_LEVELS = 7, FSS_OUTER_POPPED = 8 };
struct FsSearchArgs {
    const int32_t *parent_f, *aux;
    int32_t nx, ny;
    double ox, oy, res;
    int32_t robot_cell;
    int32_t min_size, max_size;
    int32_t n_seeds;                      // < 0: Nearest seeds, or Reference seeds when `outer`
    const int32_t *seeds;                 // [n_seeds] (device)
    int32_t outer;                        // 1: Reference seeds, from the outer search's walk (n_seeds < 0)
    const int32_t *parent_t, *fc_state;   // the clusters kernels' expandable-cell roots and state (state[0]: the start cell)
    int32_t *bcount, *cidx, *comp_root, *best_idx, *csize, *owner;
    unsigned long long *best_d2;
    int32_t *emit_comp, *emit_seed, *emit_base, *rec_base;
    int32_t *key, *pos, *q;
    fs_msort_elem *sortbuf;
    fs_frontier_record *rec;              // [nx * ny]
    double *goal_xyz;                     // [nx * ny][3] or NULL: the goal column of the scoring calls
    int32_t *fsize;                       // [nx * ny] or NULL: the frontier-size column
    double *every;                        // [nx * ny][2] or NULL
    int32_t *state;
};
hipError_t fs_launch_frontier_search(const FsSearchArgs &a, hipStream_t s);
// after the search, on the same stream: blacklisted [records] = the goal point equals one of black_xy [n_black][2] bit for bit
hipError_t fs_launch_search_blacklist(const FsSearchArgs &a, const double *d_black_xy, int32_t n_black, uint8_t *d_blacklisted, hipStream_t s);
// the grid planner's goal cells (y * nx + x, -1 off the map) of device-resident goal points [n][3]
hipError_t fs_launch_goal_cells(const double *d_goal_xyz, int32_t n, int32_t nx, int32_t ny, double ox, double oy, double res, int32_t robot_on,
                                int32_t *d_cell, hipStream_t s);

// ---- batched grid planner (fs_navfn.hip): one NavFn potential field per (grid, robot cell, allow_unknown) by a
// tiled Jacobi schedule, then NavFn::calcPath from every frontier.  The tile size is part of the field's definition.
#define NAVFN_TILE 32
struct FsNavfnPathArgs {
    const float *pot;          // [ny][nx] converged field
    int32_t nx, ny;
    int32_t n;
    const int32_t *goal_cell;  // [n] y * nx + x of the frontier cell, -1: not planned (achievable_in 0, off the map, robot off the map)
    const double *heading_in;  // [n] setPlanForFrontier's heading (host, libm), used where the plan succeeds
    int32_t robot_x, robot_y;
    int32_t max_cycles;        // 4 * max(nx, ny)
    float *scratch;            // [n][2][max_cycles] path points x then y
    double ox, oy, res;
    double *path_length, *path_length_m, *path_heading;   // path_length_m may be nullptr
    uint8_t *achievable;
};
hipError_t fs_launch_navfn_costs(const uint8_t *d_cells, int nx, int ny, int allow_unknown, uint8_t *d_cost, hipStream_t s);
hipError_t fs_launch_navfn_init(float *d_a, float *d_b, int nx, int ny, int rx, int ry, uint32_t *d_flags_prev, hipStream_t s);
hipError_t fs_launch_navfn_round(const float *d_a, float *d_b, const uint8_t *d_cost, const uint32_t *d_prev, uint32_t *d_cur, int nx, int ny,
                                 int32_t *d_any, hipStream_t s);
hipError_t fs_launch_navfn_paths(const FsNavfnPathArgs &a, hipStream_t s);
// the REFERENCE grid search (fs_set_grid_search; fs_navfn_wave.h): one calcNavFnAstar wave per distinct goal cell, one wavefront per
// wave, in batches of `slots` waves; the descents of a batch read their wave's slot
struct FsNavfnWaveArgs {
    const uint8_t *cost;       // [ny][nx] the planner's costs
    int32_t nx, ny, rx, ry;
    int32_t cap;               // entries of each priority buffer
    int32_t slots;
    float *pot;                // [slots][ny][nx]
    uint8_t *pending;          // [slots][ny][nx]
    int32_t *buf;              // [slots][3][cap]
    const int32_t *wave_cell;      // [waves] the goal cell of every wave
    const int32_t *frontier_wave;  // [n] the wave of every frontier, -1: none
    int32_t *stats;            // [4] waves of the call; waves that ended on the cycle budget, that dropped a push, chunks run again
    int32_t *wave_limit;       // [waves] FS_NW_LIMIT_* of every wave
};
// the distinct goal cells of d_cell [n] (-1: not planned) on the device: d_wave_cell, d_frontier_wave, d_stats[0]; d_first [n] scratch
hipError_t fs_launch_navfn_wave_cells(const int32_t *d_cell, int32_t n, int32_t *d_first, int32_t *d_wave_cell, int32_t *d_frontier_wave,
                                      int32_t *d_stats, hipStream_t s);
// waves base .. base + count - 1 (count <= slots) on slots 0 .. count - 1: the fill, then the waves
hipError_t fs_launch_navfn_wave_batch(const FsNavfnWaveArgs &w, int32_t base, int32_t count, hipStream_t s);
hipError_t fs_launch_navfn_paths_wave(const FsNavfnPathArgs &a, const FsNavfnWaveArgs &w, int32_t base, hipStream_t s);

// ---- any-angle leg refinement (fs_refine.hip): one converged fp64 cost field per start cell (all fields of a
// call relaxed in the same launches, blockIdx.y = field), then one wave per leg: descent, Theta*'s parent rule, interpolation.
#define RF_TILE 32
#define RF_MAX_FIELDS 32           // the most fields one build relaxes together ("refine.max_fields" is 1..RF_MAX_FIELDS)
// per-leg status of fs_refine_paths (include/fitslam_frontier.h); OVERFLOW / BROKEN never leave the library
enum : int32_t {
    FS_REFINE_OK = 0, FS_REFINE_START_OFF_MAP = 1, FS_REFINE_GOAL_OFF_MAP = 2, FS_REFINE_START_UNSAFE = 3, FS_REFINE_GOAL_UNSAFE = 4,
    FS_REFINE_NO_PATH = 5, FS_REFINE_OVERFLOW = 100, FS_REFINE_BROKEN = 101
};
struct FsRefineFieldDesc {
    int32_t slot;              // which [ny][nx] block of the field slab
    int32_t src;               // y * nx + x of the start cell
};
struct FsRefineFieldArgs {
    const uint8_t *cells;      // the staged 2-D grid
    double *g;                 // the field slab [slots][ny][nx]
    int32_t nx, ny, tx, ty;
    int32_t allow, corners;
    double w_trav;
    double e[8];               // w_euc * sqrt(dx^2 + dy^2) of moves[]
    int32_t n;                 // fields in this build (gridDim.y)
    FsRefineFieldDesc f[RF_MAX_FIELDS];
};
struct FsRefineLegArgs {
    const uint8_t *cells;
    const double *g;           // the field slab
    int32_t nx, ny;
    double ox, oy, res;
    int32_t allow, corners;
    double w_euc, w_trav;
    double e[8];
    const int32_t *leg_in;     // [blocks][4]: start cell, goal cell, field slot, output index
    int32_t *chain, *par, *vtx;   // [legs][chain_cap] scratch: the descent (goal first), the chain's parents, the vertex cells
    int64_t chain_cap;
    double *vert;              // [legs][vert_cap][2] vertex world points
    int32_t vert_cap;
    double *pose;              // [legs][pose_cap][2] interpolated poses
    int32_t pose_cap;
    int32_t *status, *n_vertices, *n_poses;   // [legs]
    double *cost;
    int64_t *chain_len, *walks;
};
hipError_t fs_launch_refine_init(const FsRefineFieldArgs &a, uint32_t *d_flags_prev, hipStream_t s);
hipError_t fs_launch_refine_round(const FsRefineFieldArgs &a, const uint32_t *d_prev, uint32_t *d_cur, int32_t *d_any, hipStream_t s);
hipError_t fs_launch_refine_legs(const FsRefineLegArgs &a, int32_t n_blocks, hipStream_t s);
// the REFERENCE refine search (fs_set_refine_search; fs_thetastar.h): the reference's Theta* search once per distinct (start cell,
// goal cell), one wavefront per search, in batches of `slots` searches; a slot holds one search's cell map, heap and records
struct FsRefineSearchArgs {
    const uint8_t *cells;
    int32_t nx, ny;
    int32_t allow, corners;
    double w_euc, w_trav;
    const double *hyp;         // [nx][ny] the host libm's hypot of cell differences
    char *slab;                // [slots][slot_bytes]
    int64_t slot_bytes;
    const int32_t *search_in;  // [searches][2]: start cell, goal cell
    int32_t vtx_cap;
    int32_t *vtx;              // [searches][vtx_cap] the vertex cells, start first
    int32_t *status, *n_vertices, *max_heap;   // [searches]
    double *cost;              // [searches] the goal record's g
    int64_t *pops, *walks;     // [searches]
};
// bytes of one slot for ns cells, every array 8-byte aligned (the kernel cuts a slot the same way)
__host__ __device__ inline int64_t fs_rs_up8(int64_t v) { return (v + 7) & ~(int64_t)7; }
__host__ __device__ inline int64_t fs_refine_search_slot_bytes(int64_t ns)
{
    return fs_rs_up8(4 * ns) + fs_rs_up8(4 * (ns + 1)) + fs_rs_up8(4 * ns) + 3 * 8 * ns + fs_rs_up8(4 * ns) + fs_rs_up8(ns);
}
// searches base .. base + count - 1 (count <= slots) on slots 0 .. count - 1: the cell maps cleared, then the searches
hipError_t fs_launch_refine_search_batch(const FsRefineSearchArgs &a, int32_t base, int32_t count, hipStream_t s);

// ---- frontier roadmap (fs_roadmap.hip): FrontierRoadMap's spatial hash and roadmap_ on the device
// FrontierRoadMap::getGridCell: floor(x / grid_cell_size), truncated to int
__host__ __device__ inline int fs_rm_cell(double v, double cell) { return (int)floor(v / cell); }

// getClosestNodeInRoadMap (key != nullptr: nodes that are keys of roadmap_ only) / getClosestNodeInHashmap (key == nullptr) of the
// query (qx, qy), DEP/src/planners/FrontierRoadmap.cpp:464-543, as a scan over the node list: the reference grows a square of
// (int)(cell * m) hash cells, m = 1, 2, ..., until one holds a candidate, and keeps the first strict minimum of the distance in
// its scan order (dx outer, dy inner, insertion order).  That square is the first (int)(cell * m) >= the Chebyshev cell distance
// of the nearest candidate, so two passes over the nodes give the same node: the radius, then the minimum distance with ties to the
// smallest (dx, dy, index).  -1: no candidate (the reference searches forever).
__host__ __device__ inline int32_t fs_rm_closest(const double *xy, const uint8_t *key, int32_t n, double cell, double qx, double qy)
{
    const int64_t cx = fs_rm_cell(qx, cell), cy = fs_rm_cell(qy, cell);
    int64_t cmin = INT64_MAX;
    for (int32_t k = 0; k < n; ++k) {
        if (key && !key[k]) continue;
        const int64_t ax = fs_rm_cell(xy[2 * k], cell) - cx, ay = fs_rm_cell(xy[2 * k + 1], cell) - cy;
        const int64_t c = (ax < 0 ? -ax : ax) > (ay < 0 ? -ay : ay) ? (ax < 0 ? -ax : ax) : (ay < 0 ? -ay : ay);
        if (c < cmin) cmin = c;
    }
    if (cmin == INT64_MAX) return -1;
    int64_t m = (int64_t)floor((double)cmin / cell);
    if (m < 1) m = 1;
    while (m > 1 && (int64_t)(cell * (double)(m - 1)) >= cmin) --m;
    while ((int64_t)(cell * (double)m) < cmin) ++m;
    const int64_t R = (int64_t)(cell * (double)m);
    int32_t best = -1;
    double bd = 0.0;
    int64_t bdx = 0, bdy = 0;
    for (int32_t k = 0; k < n; ++k) {
        if (key && !key[k]) continue;
        const int64_t ax = fs_rm_cell(xy[2 * k], cell) - cx, ay = fs_rm_cell(xy[2 * k + 1], cell) - cy;
        if (ax < -R || ax > R || ay < -R || ay > R) continue;
        const double ex = qx - xy[2 * k], ey = qy - xy[2 * k + 1];
        const double d = sqrt(ex * ex + ey * ey);                   // distanceBetweenFrontiers (pow(e, 2) == e * e)
        if (best < 0 || d < bd || (d == bd && (ax < bdx || (ax == bdx && ay < bdy)))) {
            best = k; bd = d; bdx = ax; bdy = ay;
        }
    }
    return best;
}

struct FsRoadmapDev {
    int32_t n;                 // nodes, insertion order
    const double *xy;          // [n][2]
    double cell, radius;       // grid_cell_size, radius_to_decide_edges
    int32_t n_cells;           // occupied hash cells
    const uint64_t *cell_key;  // [n_cells] ascending: (uint32)cx << 32 | (uint32)cy
    const int32_t *cell_start; // [n_cells + 1] into cell_nodes
    const int32_t *cell_nodes; // node ids cell by cell, insertion order inside a cell
};
// reConstructGraph(entireGraph = true): candidates of every node in getNodesWithinRadius order (count, then fill the segments
// candidate -> node after an exclusive scan of the counts), the segment walk (fs_launch_segments), then the accepted edges
// compacted in order (count, scan, fill)
hipError_t fs_launch_rm_candidates(const FsRoadmapDev &g, const int32_t *d_off, int32_t *d_count, double oz, double *d_start,
                                   double *d_end, int32_t *d_cand, hipStream_t s);
hipError_t fs_launch_rm_edges(int32_t n, const int32_t *d_cand_off, const int32_t *d_cand, const uint8_t *d_ok, const uint8_t *d_hit,
                              const int32_t *d_unknown, double unknown_limit, const int32_t *d_row, int32_t *d_count, int32_t *d_col,
                              hipStream_t s);
// exclusive scan of n counts by one workgroup: out[0..n], out[n] = the total
hipError_t fs_launch_rm_scan(const int32_t *d_in, int32_t n, int32_t *d_out, hipStream_t s);
// the transposed CSR (in-edges), the shortest-path tree from node `root` and the path columns
hipError_t fs_launch_rm_transpose(int32_t n, const int32_t *d_row, const int32_t *d_col, int32_t *d_indeg, int32_t *d_trow,
                                  int32_t *d_cursor, int32_t *d_tcol, hipStream_t s, int phase);
struct FsRmTree {
    int32_t n, root;
    const double *xy;
    const int32_t *trow, *tcol;      // in-edges of every node
    double *d[2];                    // the two round buffers of the key (distance, hops, predecessor)
    int32_t *hops[2], *pred[2];
};
#define RM_TREE_ONE_WG 16384         // up to this many nodes the whole relaxation is one workgroup's loop
hipError_t fs_launch_rm_tree_init(const FsRmTree &t, hipStream_t s);
hipError_t fs_launch_rm_tree_block(const FsRmTree &t, int32_t max_rounds, int32_t *d_rounds, hipStream_t s);
hipError_t fs_launch_rm_tree_round(const FsRmTree &t, int32_t src, int32_t *d_any, hipStream_t s);
struct FsRmPlanArgs {
    int32_t n_nodes;
    const double *xy;
    const uint8_t *key;
    double cell;
    const double *d;                 // converged tree (nullptr: no start node)
    const int32_t *pred;
    int32_t root;
    int32_t n;
    const double *goal;              // [n][2]
    const uint8_t *mode;             // [n] 0 not planned, 1 goal == robot xy, 2 plan
    const double *heading_in;        // [n]
    double *path_length, *path_length_m, *path_heading;
    uint8_t *achievable;
};
hipError_t fs_launch_rm_plan(const FsRmPlanArgs &a, hipStream_t s);
// R plans in one launch (fs_fleet_allocate_roadmap): d_robots [n_robots] in device memory, each with n frontiers
hipError_t fs_launch_rm_fleet_plan(const FsRmPlanArgs *d_robots, int32_t n_robots, int32_t n, hipStream_t s);

// ---- the REFERENCE roadmap search: FrontierRoadmapAStar::getPlan per distinct (start, goal) pair, one wave per
// query (fs_roadmap_astar.h).  A query's heap, records and per-node state sit in LDS while they fit (lds_cap records); a query that
// outgrows them, or every query when lds_cap is 0, runs again on the global route: `slots` waves, each with a slot of the pool
// holding `cap` records.  A query that outgrows that too keeps status FS_ASTAR_OVERFLOW and is counted in stats[3]; the host grows
// the pool and launches the global route again.
struct FsRmAstarArgs {
    int32_t n_nodes;
    const double *xy;
    const int32_t *row, *col;       // the roadmap's adjacency lists (CSR, the reference's order)
    const int32_t *nq;              // [1] queries (a device word)
    const int32_t *src;             // [q] start node, or nullptr: `root` for every query
    int32_t root;
    const int32_t *dst;             // [q] goal node
    int32_t *status;                // [q] FS_ASTAR_FOUND / NO_PATH / OVERFLOW
    double *len;                    // [q] path length (FOUND)
    int32_t *stats;                 // [0] queries, [1] pops of the largest query, [2] queries sent to the global route, [3] queries
                                    //     that outgrew the global route's capacity
    int32_t lds_cap;                // records in LDS (0: every query takes the global route)
    char *pool;                     // global route: slot b at pool + b * slot_bytes
    size_t slot_bytes;
    int32_t slots, cap;
    // the node chain of a FOUND query (fs_roadmap_routes), or chain_len == nullptr: not emitted.  The query takes
    // chain_len[q] slots of chain_pool from chain_base[q] = the cursor before its atomic bump, goal node first; a chain that would
    // end beyond chain_cap is not written (the cursor still counts it: the host grows the pool to the cursor and runs again).
    int32_t *chain_len;             // [q]
    int64_t *chain_base;            // [q]
    int32_t *chain_pool;
    int64_t chain_cap;
    unsigned long long *chain_cursor;   // [1]
};
#define RM_ASTAR_LDS_BYTES 65536
#define RM_ASTAR_SLOTS 32
// bytes of one query's storage: heap (f, record), records (g, node, parent), best record and closed flag of every node
inline size_t fs_rm_astar_bytes(int32_t cap, int32_t n) { return ((size_t)28 * (size_t)cap + (size_t)5 * (size_t)n + 15) & ~(size_t)15; }
// the LDS route over queries 0 .. nq - 1 (grid: max_q workgroups, an upper bound of nq), then the global route
hipError_t fs_launch_rm_astar(const FsRmAstarArgs &a, int32_t max_q, hipStream_t s);
hipError_t fs_launch_rm_astar_global(const FsRmAstarArgs &a, hipStream_t s);
// the plan's queries: every frontier's goal node (mode 2, a start node) marked, the marks scanned into query indices, the query
// list; then the path columns from the query results
hipError_t fs_launch_rm_astar_goals(const FsRmPlanArgs &p, int32_t *d_gnode, int32_t *d_mark, hipStream_t s);
hipError_t fs_launch_rm_astar_list(int32_t n_nodes, const int32_t *d_mark, const int32_t *d_qidx, int32_t *d_dst, hipStream_t s);
hipError_t fs_launch_rm_astar_cols(const FsRmPlanArgs &p, const int32_t *d_gnode, const int32_t *d_qidx, const int32_t *d_status,
                                   const double *d_len, hipStream_t s);

// ---- roadmap routes (fs_roadmap_routes): the node list of every distinct goal node the plan reached, its
// refinePath shortcut (FrontierRoadmap.cpp:657-714) and, through fs_pathinfo.hip, the Fisher information of its legs.
// Stage 1 (before the host knows any size): a node's route length — hops + 1 under the tree, the A* chain's length under the
// REFERENCE search, 0 where no planned frontier ends or the goal was not reached — the nodes with a route numbered in ascending
// order (fs_launch_rm_scan of `has`), the routes' goal nodes and lengths, every frontier's route.
struct FsRmRouteArgs {
    int32_t n_nodes;
    const int32_t *mark;            // [n_nodes] fs_launch_rm_astar_goals' marks: a planned frontier ends at this node
    // TREE: the converged tree (d == nullptr: no route at all)
    const double *d;
    const int32_t *hops, *pred;
    // REFERENCE (status != nullptr): the queries' results and chains
    const int32_t *qidx, *status, *chain_len;
    const int64_t *chain_base;
    const int32_t *chain_pool;
    int32_t *len, *has;             // [n_nodes] the node's route length; 1 where it is positive
    const int32_t *ridx;            // [n_nodes + 1] exclusive scan of `has`
    int32_t *goal_node, *route_len, *route_q;   // [routes] (route_q: the route's query, REFERENCE)
    int32_t n;                      // frontiers
    const int32_t *gnode;           // [n] fs_launch_rm_astar_goals' goal nodes
    int32_t *route_of;              // [n]
    // stage 2 (the host has scanned route_len into node_off): the lists, start node first
    int32_t n_routes;
    const int64_t *node_off;        // [n_routes + 1]
    int32_t *node;
};
hipError_t fs_launch_rm_route_lengths(const FsRmRouteArgs &a, hipStream_t s);      // len, has
hipError_t fs_launch_rm_route_index(const FsRmRouteArgs &a, hipStream_t s);        // goal_node, route_len, route_q, route_of
hipError_t fs_launch_rm_route_emit(const FsRmRouteArgs &a, hipStream_t s);         // node
// refinePath on every route (fs_raymarch.hip, beside the segment walker): one wave per route, lane l walks P[kk] -> P[kk + 1 + l]
// by isConnectable on the staged grid, a ballot finds the first failure.  refined lists sit at the raw lists' offsets.
struct FsRouteRefineArgs {
    FsGridDev grid;
    double max_length;              // isConnectable's (unsigned)(1.5 * radius / resolution)
    double unknown_limit;           // 0.3 * radius / resolution
    const double *xy;               // [n_nodes][2]
    int32_t n_routes;
    const int64_t *node_off;
    const int32_t *node;
    int32_t *refined;               // route r's list from node_off[r] on
    int32_t *refined_len;           // [n_routes]
    uint8_t *complete;              // [n_routes] 0: the shortcut stopped at a node that cannot see its successor
    unsigned long long *walks;      // [1] segment walks (added to)
};
hipError_t fs_launch_route_refine(const FsRouteRefineArgs &a, hipStream_t s);

// ---- next goal (FullPathOptimizer::getNextGoal): the pair matrix over [robot, locals, closest global] and the
// exhaustive tour search over the locals' orders
#define RM_TOUR_MAX_LOCAL 12                          // 12! < 2^31
#define RM_TOUR_MAX_NODES (RM_TOUR_MAX_LOCAL + 2)
#define RM_TOUR_MAX_TREES (RM_TOUR_MAX_LOCAL + 1)     // a tree per distinct source root: the robot and the locals
// K trees in one set of buffers: tree b's two round buffers at + 2 * n * b of t.d[0] / t.hops[0] / t.pred[0] (t.root and the
// second buffer pointers are ignored); every tree is relax()'s, so each equals the single tree from its root
struct FsRmTreeBatch {
    FsRmTree t;
    int32_t k;
    int32_t root[RM_TOUR_MAX_TREES];
};
hipError_t fs_launch_rm_batch_init(const FsRmTreeBatch &b, hipStream_t s);
// one workgroup per tree (n <= the one-workgroup limit): rounds[b] as rm_tree_block's rounds[0]
hipError_t fs_launch_rm_batch_block(const FsRmTreeBatch &b, int32_t max_rounds, int32_t *d_rounds, hipStream_t s);
// one round of every tree per launch, blockIdx.y = tree: any[0] = 1 when a key of any tree changed
hipError_t fs_launch_rm_batch_round(const FsRmTreeBatch &b, int32_t src, int32_t *d_any, hipStream_t s);
struct FsRmPairArgs {
    int32_t m;                              // nodes of the matrix
    int32_t n_nodes;                        // roadmap nodes
    const double *xy;                       // [n_nodes][2]
    const double *d;                        // tree b's converged distances at d + 2 * n_nodes * b
    const int32_t *pred;                    // ... and predecessors
    double charge;                          // an unreachable pair's length
    double pxy[2 * RM_TOUR_MAX_NODES];      // the nodes' goal points
    int32_t start[RM_TOUR_MAX_NODES];       // closest key node of each point (-1: none)
    int32_t tree[RM_TOUR_MAX_NODES];        // the tree rooted at start[i] (sources 0..m-2)
    double *M;                              // [m][m], symmetric, 0 on the diagonal
    // REFERENCE search (q_status != nullptr): pair (i, j), i < j, is A* query query[i * m + j] (-1: no start node)
    const int32_t *q_status;
    const double *q_len;
    int32_t query[RM_TOUR_MAX_NODES * RM_TOUR_MAX_NODES];
};
hipError_t fs_launch_rm_pairs(const FsRmPairArgs &a, hipStream_t s);
// the tour search: lane chunks of lexicographic ranks, one (length, robot leg, rank, count) per block, then one workgroup over the
// blocks; out = {length, robot leg} doubles then {rank, count} int64 at out + 2
struct FsRmTourArgs {
    int32_t k;                              // locals; the matrix is (k + 2)^2
    const double *M;
    int64_t total;                          // k!
    int64_t chunk;                          // ranks per lane
    double *blen, *bleg;                    // [blocks]
    int64_t *brank, *bcnt;
};
int32_t fs_rm_tour_blocks(int64_t total, int64_t *chunk);
hipError_t fs_launch_rm_tour(const FsRmTourArgs &a, int32_t blocks, double *d_out, hipStream_t s);

// ---- the per-tick roadmap update (fs_roadmap_update.hip): UpdateRoadmapBT's addNodes, addRobotPoseAsNode,
// constructNewEdges and constructNewEdgeRobotPose decided on the device by the rules of fs_roadmap_update.h
#define FS_RU_MAX_POINTS 16384      // points of one update (the conflict rows are n x n bits)
enum : int32_t {                    // the header the host reads
    FS_RU_H_KEPT = 0,               // points of the list added as nodes
    FS_RU_H_TRIPPED,                // 0, 1: the list overfilled a cell, 2: the robot pose did
    FS_RU_H_ROBOT,                  // the robot pose was added
    FS_RU_H_NODES,                  // nodes after the additions
    FS_RU_H_OWNERS,                 // distinct closest nodes
    FS_RU_H_ROUNDS,                 // Jacobi rounds of the keep rule (-1: did not settle)
    FS_RU_H_INSERTED,               // (p, q) pairs inserted
    FS_RU_H_WORDS
};
struct FsRmUpdate {
    int32_t n;                      // points of the list
    const double *pts;              // device, point i at pts[stride * i], pts[stride * i + 1]
    int32_t stride;
    double rx, ry;                  // the robot pose
    int32_t add_robot;
    int32_t n_old;                  // nodes before the call
    double *xy;                     // [n_old + n + 1][2]: the nodes, the kept points appended
    uint8_t *key;                   // [n_old + n + 1]
    const int32_t *row, *col;       // the adjacency lists before the call (CSR over n_old nodes)
    double cell, radius, min_frontier, min_robot, oz;
    int32_t words;                  // 64-bit words of a conflict row: (n + 63) / 64
    uint64_t *conf;                 // [n][words]
    uint8_t *rejected;              // [n] an existing node rejects the point
    int32_t *occupants;             // [n] existing nodes in the point's cell
    int32_t *hdr;                   // [FS_RU_H_WORDS]
    int32_t *closest;               // [n + 1] closest hash node of every point, then of the robot pose
    int32_t *rank_of;               // [n_old + n + 1] first query of a node, then its owner rank (>= n + 1: not an owner)
    int32_t *owner;                 // [n + 1] rank -> node
    int32_t *cand_count, *cand_off; // [n + 1], [n + 2] candidates per owner rank
    int32_t *tmp_q, *tmp_order;     // [total] candidates in index order with their scan cell
    int32_t *cand, *cand_rank;      // [total] candidates in getNodesWithinRadius order, their owner's rank
    double *seg_start, *seg_end;    // [total][3] the walks candidate -> owner
    const uint8_t *seg_ok, *seg_hit;
    const int32_t *seg_unknown;
    double unknown_limit;
    int32_t *flag, *flag_off;       // [total], [total + 1] inserted candidates and their scan
    int32_t *pairs;                 // [total][2] the inserted (p, q) in order
};
hipError_t fs_launch_ru_nodes(const FsRmUpdate &u, hipStream_t s);                     // keep rule, cell cap, robot pose -> xy, hdr
hipError_t fs_launch_ru_owners(const FsRmUpdate &u, hipStream_t s);                    // closest, owners, candidate counts and offsets
hipError_t fs_launch_ru_candidates(const FsRmUpdate &u, int32_t total, hipStream_t s); // the ordered lists and their segments
hipError_t fs_launch_ru_insert(const FsRmUpdate &u, int32_t total, hipStream_t s);     // flags, scan, pairs

// ---- key-frame anchors of the roadmap (fs_roadmap_kf.hip): mapDataCallback's anchoring, optimizeSHM's re-placement
// and de-duplication
#define FS_KF_RT 24                   // a key-frame slot: R [9] row-major, t [3], R^-1 [9], -R^-1 t [3] (float)
#define FS_KF_MAX_PER_CELL 20         // populateNodes throws once a cell holds more (FrontierRoadmap.cpp:244-248)
#define FS_KF_DEDUP_ONE_WG 16384      // up to this many points the de-duplication rounds are one workgroup's loop
float fs_kf_pose_table(const double pose7[7], float T[FS_KF_RT]);
struct FsKfTable {                    // one map message
    double cell;                      // grid_cell_size (getGridCell)
    const float *rt;                  // [slots][FS_KF_RT]: one slot per distinct id (its last pose in the message)
    const int32_t *handle;            // [slots] the id's handle in the record store
    int32_t n_cells;                  // occupied key-frame cells
    const uint64_t *cell_key;         // [n_cells] ascending: (uint32)cx << 32 | (uint32)cy
    const int32_t *cell_start;        // [n_cells + 1]
    const int32_t *cell_slots;        // slots cell by cell, in message order (duplicates kept)
};
// pending nodes xy [n][2] (queue order): parents counted (d_off == nullptr) or the records (handle, p_c) written from d_off[i] on
hipError_t fs_launch_kf_anchor(const FsKfTable &t, int32_t n, const double *d_xy, const int32_t *d_off, int32_t *d_count, int32_t *d_rec_h,
                               float *d_rec_p, hipStream_t s);
// record i -> out_xy[h_base[h] + rec_ord[i]] = (T_kf * p_c).xy, T_kf the slot h_slot[h] of d_rt; h_base[h] < 0: skipped
hipError_t fs_launch_kf_place(int32_t n_rec, const int32_t *d_rec_h, const int32_t *d_rec_ord, const float *d_rec_p, const int32_t *d_h_slot,
                              const int32_t *d_h_base, const float *d_rt, float *d_out_xy, hipStream_t s);
struct FsKfDedup {
    int32_t m;                        // points, sequence order
    const float *xy;                  // [m][2]
    double cell, min_d;
    uint32_t mask;                    // hash capacity - 1 (capacity a power of two >= 2m)
    uint64_t *hkey;                   // [capacity] cell key of each hash slot
    int32_t *hcount, *hcursor;        // [capacity]
    int32_t *hstart;                  // [capacity + 1]
    int32_t *hpts;                    // [m] points slot by slot
    int32_t *pslot;                   // [m] each point's hash slot
    const int32_t *cand_off, *cand;   // conflicts: [m + 1], [total]
    uint8_t *state[2];                // round buffers: 0 undecided, 1 accepted, 2 rejected
    int32_t *hdr;                     // [4]: kept points, cut (the point that is a cell's 21st node; INT32_MAX none), rounds, 0
};
hipError_t fs_launch_kf_dedup_cells(const FsKfDedup &d, hipStream_t s);
hipError_t fs_launch_kf_dedup_conflicts(const FsKfDedup &d, const int32_t *d_off, int32_t *d_count, int32_t *d_out, hipStream_t s);
hipError_t fs_launch_kf_dedup_block(const FsKfDedup &d, int32_t max_rounds, hipStream_t s);
hipError_t fs_launch_kf_dedup_round(const FsKfDedup &d, int32_t src, int32_t *d_any, hipStream_t s);
// the cut, then the kept points compacted in order into d_out_xy (hdr[0] = how many); reads the verdicts from buffer src
hipError_t fs_launch_kf_dedup_finish(const FsKfDedup &d, int32_t src, int32_t *d_keep, int32_t *d_keep_off, float *d_out_xy, hipStream_t s);

// ---- key-frame pose information (computeInformationForPose)
struct FsKfArgs {
    int32_t n;                 // poses
    const double *tri;         // [n][12]: FOV triangle at max_depth, then at max_depth + max_depth_error (x0,y0,x1,y1,x2,y2)
    const float *Rt;           // [n][12]
    int32_t n_kf;
    const double *kf_check;    // [n_kf][12]: the key-frame frustum's three vertices and three edge midpoints (depth + error)
    const int32_t *kf_offsets; // [n_kf + 1] into the point arrays
    const float *px, *py, *pz; // key-frame world points, SoA
    double radius;             // < 0: no radius filter
    float qinv;                // Q^-1 diagonal
    int32_t nx, ny;
    double ox, oy, res;
    float *info;
    int32_t *n_cells, *n_points;
    int32_t *flagged;          // [n] poses redone with the HBM table
    unsigned long long *counters;   // [1]
    uint32_t *gtable;          // [pool][3][1 << gbits]
    int32_t gbits;
};
hipError_t fs_launch_kf_info(const FsKfArgs &a, int pool, hipStream_t s);

// ---- Fisher information along the planned paths (fs_pathinfo.hip): setPlanForFrontier's way points, one pose record
// per distinct (from cell, to cell), the per-frontier columns; and along the legs of roadmap routes
struct FsPathInfoArgs {
    int32_t n;                        // frontiers
    int32_t nx, ny, max_cycles;       // the grid; the stride of a path's x / y arrays in `path`
    int64_t step;                     // s + 1, s = (int)(sample_distance / resolution): a way point every `step` path points
    int32_t lookahead;                // the pose looks at the point this many further on (towards the frontier)
    double ox, oy, res;
    const float *path;                // navfn_paths_kernel's scratch [n][2][max_cycles]
    const double *path_length;        // [n] the planner's columns
    const uint8_t *achievable;        // [n]
    int32_t dedup;                    // 1: one record per distinct key; 0: one per way point
    int64_t bound;                    // room for way points in every array below, and the size of the launches
    int32_t *count, *offset;          // [n + 1]; offset[n] = total
    uint64_t *key_in, *key_out;       // [bound] (dedup)
    int32_t *wp_in, *wp_out, *head, *rank;   // [bound] (dedup): way point of a key, head of a run of equal keys, heads up to here
    int32_t *slot;                    // [bound] way point -> record
    float *rt;                        // [bound][12] the pose records the FIM worker reads
    double *pose7;                    // [bound][7] or nullptr: the dump
    int64_t *hdr;                     // [2]: total, records
    void *temp;                       // rocPRIM's scratch
    size_t temp_bytes;
    // finish
    const float *info;                // [records] the worker's info_ref column
    float *wp_info;                   // [bound] or nullptr: the dump
    double fi_threshold;
    double *info_mean;                // [n]
    float *info_min;                  // [n]
    int32_t *first_unsafe;            // [n]
    // Route legs instead of grid-path way points (fs_roadmap_routes; node_xy != nullptr): "frontier" f is the node
    // list list[list_off[f] .. + list_len[f]), its way point k the leg (list[k], list[k + 1]) — pose at the first node looking at
    // the second, key = first * n_nodes + second.  path, path_length, achievable, step, lookahead and the grid fields are unused.
    const double *node_xy;            // [n_nodes][2]
    int32_t n_nodes;
    const int32_t *list;
    const int64_t *list_off;          // [n]
    const int32_t *list_len;          // [n]
};
size_t fs_pathinfo_temp_bytes(const FsPathInfoArgs &a, int64_t bound, hipStream_t s);    // rocPRIM's scratch for n, nx, ny and that room; 0: it refused
hipError_t fs_launch_pathinfo_offsets(const FsPathInfoArgs &a, hipStream_t s);            // count, offset
hipError_t fs_launch_pathinfo_prepare(const FsPathInfoArgs &a, hipStream_t s);            // keys ... records, hdr
hipError_t fs_launch_pathinfo_finish(const FsPathInfoArgs &a, hipStream_t s);             // the per-frontier columns

// ---- the information layer (fs_infolayer.hip): Fisher information of a pose lattice on the staged 2-D grid as costs.
// Blocks of s x s cells tile the window [x0, x0+sx) x [y0, y0+sy) (nbx x nby of them, row-major); pose p = scored block (p / K) in
// block order, heading p % K.
struct FsInfoLayerArgs {
    uint8_t *cells;                   // the staged grid [ny][nx]
    int32_t nx, ny;
    double ox, oy, res;
    int32_t x0, y0, sx, sy, s, nbx, nby;
    int32_t K, reduce, max_cost, write;
    double pose_z, info_lo, info_hi;
    const double *quat_zw;            // [K][2] sin, cos of half the heading: the host's libm
    int32_t *anchor;                  // [nb] anchor cell y * nx + x, or -1
    int32_t *flag, *rank;             // [nb + 1] scored?; scored blocks before this one (rank[nb] = n_scored)
    int32_t *list;                    // [n_scored] the scored blocks in block order
    float *val;                       // [n_scored][K] the worker's info_ref per pose
    float *info;                      // [nb] the reduced value, NaN where unscored
    float *per_yaw;                   // [K][nb] or nullptr
    unsigned long long *n_changed;    // [1]
    void *temp;                       // rocPRIM's scratch
    size_t temp_bytes;
};
size_t fs_infolayer_temp_bytes(int64_t nb, hipStream_t s);                                 // rocPRIM's scratch for nb blocks; 0: it refused
hipError_t fs_launch_infolayer_anchors(const FsInfoLayerArgs &a, hipStream_t s);           // anchor, flag, rank, list
hipError_t fs_launch_infolayer_records(const FsInfoLayerArgs &a, int64_t p0, int64_t n, float *rt, hipStream_t s);   // rt [n][12] of poses [p0, p0 + n)
hipError_t fs_launch_infolayer_store(const FsInfoLayerArgs &a, hipStream_t s);             // info, per_yaw, the cells, n_changed

// ---- landmark staging (fs_capi.hip), split so that fs_multi orders a cloud once for all its devices
struct FsStagedCloud {
    int32_t m = 0, n_chunks = 0;
    std::vector<float> x, y, z;     // SoA in k-d leaf order, padded to whole chunks with far-away sentinels
    std::vector<float> sph;         // [n_chunks][4] bounding spheres (cx, cy, cz, r + safety margin)
    std::vector<int32_t> perm;      // per staged slot: the landmark's position in the uploaded array, -1 for a sentinel (fs_landmarks_in_view)
};
void fs_stage_landmarks(const float *xyz, int32_t m, FsStagedCloud &out);
int fs_upload_staged_landmarks(fs_ctx *c, const FsStagedCloud &st);
// ... and the same ordering computed on the device ("cloud.order", fs_cloud.hip): every level's node boundaries (a function of the
// number of usable landmarks alone), the level loop (keys kernel + one stable radix sort per level), the SoA gather and the spheres
bool fs_ctx_cloud_on_device(const fs_ctx *c, int32_t m);
void fs_cloud_levels(int32_t n_usable, std::vector<int32_t> &bounds, std::vector<int32_t> &level_off, std::vector<int32_t> &level_nodes,
                     std::vector<int32_t> &level_largest);
size_t fs_cloud_sort_temp_bytes(int32_t n, hipStream_t s);
hipError_t fs_cloud_iota(int32_t *d_perm, int32_t n, hipStream_t s);
hipError_t fs_cloud_order_device(const float *d_raw, int32_t n_usable, const int32_t *d_bounds, const std::vector<int32_t> &level_off,
                                 const std::vector<int32_t> &level_nodes, const std::vector<int32_t> &level_largest, int32_t *d_perm_a, int32_t *d_perm_b, uint64_t *d_keys_a,
                                 uint64_t *d_keys_b, void *d_temp, size_t temp_bytes, uint32_t *d_top_bbox, hipStream_t s, int32_t **perm_out);
size_t fs_cloud_top_bbox_words();   // scratch of the top levels' bounding boxes (d_top_bbox; nullptr: one workgroup per node at every level)
hipError_t fs_cloud_finish(const float *d_raw, const int32_t *d_perm, int32_t n_usable, int32_t n_chunks, float *d_lx, float *d_ly, float *d_lz,
                           float *d_spheres, hipStream_t s);

// ---- landmarks in view of each pose (fs_landmarks_in_view; fs_view.hip)
// The cloud's permutation, kept by both ordering routes: keep[slot] = the landmark's position in the uploaded array (-1 for a
// sentinel: padding, unusable landmarks), inv[position] = its slot (-1: unusable).  d_src: the first n_usable slots' positions as
// the device route left them, or nullptr when `keep` has been uploaded whole (the host route).
hipError_t fs_view_keep_perm(const int32_t *d_src, int32_t n_usable, int32_t padded, int32_t m, int32_t *d_keep, int32_t *d_inv, hipStream_t s);
struct FsViewArgs {
    const float *lx, *ly, *lz, *spheres;   // the staged cloud, as FsFimArgs
    int32_t n_chunks, m;
    const int32_t *perm, *inv;             // fs_view_keep_perm's keep [n_chunks * 64] and inv [m]
    const float *Rt;                       // [n][12] pose records of the whole call
    int32_t pose_lo, n_round;              // this round's poses: pose_lo .. pose_lo + n_round - 1
    int32_t words;                         // mask words per pose: ceil(m / 32)
    uint32_t *mask;                        // [n_round][words], bit i of a pose: landmark i is in view
    int32_t *counts;                       // [n_round]
    int32_t group;                         // chunks per wave of the mark kernel (a power of two, 4 .. 64)
    int32_t cull;                          // 0: every chunk is tested
    float max_dist_f;                      // culling reach (FsFimArgs::max_dist_f)
    float maxd2, cos2;                     // the predicate (FsFimArgs' fields)
    int32_t cone_mode;
    const float *table;                    // dense lookup table (FsFimArgs' fields)
    int32_t jx0, jy0, jz0, tx, ty, tz;
    double inv_step;
    int32_t occluded, occ_min, occ_max;    // fs_set_occlusion (FsFimArgs' fields); occ_grid is read only when occluded
    uint32_t occ_margin;
    FsGridDev occ_grid;
    int64_t *offsets;                      // [n + 1] CSR row pointer over the true counts
    int64_t max_total;                     // entries `out` holds
    fs_view_landmark *out;
};
hipError_t fs_launch_view_mark(const FsViewArgs &a, hipStream_t s);      // mask of the round's poses (zeroed by the caller)
hipError_t fs_launch_view_count(const FsViewArgs &a, hipStream_t s);     // counts, then offsets[pose_lo + 1 ..] from offsets[pose_lo]
hipError_t fs_launch_view_emit(const FsViewArgs &a, hipStream_t s);      // the entries below max_total

// ---- sensor sweep on a ground-truth world (fs_sense; fs_sense.hip)
// sense: one wavefront per pose walks the pose's used rays through `world` (an FsGridDev whose cells are the world's), stores 1
// into mark [nz][ny][nx] at every seen cell, counts the staged-unknown visits per ray and folds the seen cells' bounding box into
// box [6] = min x, y, z, max x, y, z (preset to nx, ny, nz, -1, -1, -1).  merge: over the window, staged = world where the mark is
// set, counts [2] += seen cells, revealed cells (255 before, not 255 in the world); the marks are cleared.
struct FsSenseArgs {
    FsGridDev world;
    const uint8_t *staged;     // the staged grid, same shape
    const double *dir;         // the fan's direction table, as FsRayArgs::dir
    int32_t n_yaw, n_elev, window;
    uint32_t max_length;
    int32_t obst_min, obst_max, trace_min, trace_max;
    double lo_x, hi_x, lo_y, hi_y, lo_z, hi_z;   // the folded clamp bounds, as FsRayArgs'
    int32_t n;
    const double *origin;      // [n][3]
    const int32_t *first_ray;  // [n] or nullptr: -1 = all n_yaw rays, else the window from there (checked on the host)
    uint8_t *mark;
    int32_t *ray_unknown;      // [n][n_elev][n_yaw] or nullptr
    int32_t *seen_unknown, *status;   // [n]
    int32_t *box;              // [6]
};
hipError_t fs_launch_sense(const FsSenseArgs &a, hipStream_t s);
hipError_t fs_launch_sense_merge(const uint8_t *d_world, uint8_t *d_staged, uint8_t *d_mark, int nx, int ny, int x0, int y0, int z0,
                                 int sx, int sy, int sz, unsigned long long *d_counts, hipStream_t s);
// surroundingCellsMapped (Helpers.cpp:98-133) of d_goal [n][3] on the 2-D grid, one lane per goal
hipError_t fs_launch_goals_mapped(const uint8_t *d_cells, int nx, int ny, double ox, double oy, double res, int32_t n, const double *d_goal,
                                  uint8_t *d_mapped, hipStream_t s);
// d_counts [4] += cells != 255, == 255, == 254, == 0
hipError_t fs_launch_grid_census(const uint8_t *d_cells, size_t total, unsigned long long *d_counts, hipStream_t s);

// ---- driving station lists through the world (fs_drive; fs_drive.hip)
// One step k of all robots is three or four launches on one stream, none of which waits for anything but its predecessor:
//   step   — one wavefront per robot still FS_DRIVE_DRIVING: out of stations -> ARRIVED; k >= 1: the move station k - 1 -> k on the
//            staged map and the world (OFF_MAP / BLOCKED / COLLIDED, else reached = k); then the sweep from station k as
//            fs_sense_kernel does it, the seen cells' box into station_box [station][4] = min x, y, max x, y (preset nx, ny, -1, -1)
//            and into union_box [4]
//   merge  — blockIdx.y = robot, over that robot's box of this step: as fs_sense_merge_kernel; a cell in several robots' boxes
//            belongs to the lowest robot whose box holds it
//   (fs_launch_keepout_apply over the step's window, by the caller, when zones are stored)
//   goal   — one lane per robot still driving: surroundingCellsMapped of its goal -> MAPPED
#define FS_DRIVE_DRIVING (-1)      // state[2 r] while robot r drives; the FS_DRIVE_* codes of the header once it has stopped
struct FsDriveArgs {
    FsSenseArgs sense;             // the fan and the world as fs_sense fills them; origin = station_xyz [total][3], first_ray [total] or
                                   // nullptr, status / seen_unknown [total] (preset -1 / 0); n, ray_unknown and box are not used
    FsGridDev staged;              // the staged grid, for the move
    int32_t n_robots, step;
    const int32_t *n_stations;     // [R]
    const int32_t *station_off;    // [R] first station of each robot
    const double *goal;            // [R][3]
    int32_t block_min, block_max;
    double move_max_length;        // nx + ny: never cuts a segment
    int32_t *state;                // [R][2] status, reached (preset FS_DRIVE_DRIVING, 0)
    int32_t *station_box;          // [total][4]
    int32_t *union_box;            // [4] preset nx, ny, -1, -1
    unsigned long long *counts;    // [2] += seen, revealed
};
hipError_t fs_launch_drive_step(const FsDriveArgs &a, hipStream_t s);
// merge_blocks: blocks per robot (the caller sizes them by the largest window a robot can touch in this step)
hipError_t fs_launch_drive_merge(const FsDriveArgs &a, unsigned merge_blocks, hipStream_t s);
hipError_t fs_launch_drive_goal(const FsDriveArgs &a, hipStream_t s);

// ---- landmark sensor on a ground-truth cloud (fs_sense_landmarks; fs_sense_landmarks.hip)
// sweep: one wavefront per (pose, group of chunks) of the WORLD cloud; a landmark a pose sees gets views[world index] += 1, the
// pose n_in_view[pose] += 1 (both zero-based sums: the caller clears n_in_view, views carry on from earlier calls).
struct FsLandmarkSenseArgs {
    const float *lx, *ly, *lz, *spheres;   // the world cloud in its own k-d leaf order, as FsFimArgs' staged one
    const int32_t *perm;                   // [n_chunks * 64]: the world index per slot, -1 for a sentinel
    int32_t n_chunks, m_world;
    const float *Rt;                       // [n][12]
    int32_t n;
    int32_t group;                         // chunks per wave (a power of two, 4 .. 64)
    int32_t cull;                          // 0: every chunk is tested
    float max_dist_f;                      // culling reach (FsFimArgs::max_dist_f)
    float maxd2, cos2;                     // the predicate (FsFimArgs' fields)
    int32_t cone_mode;
    int32_t los, occ_min, occ_max;         // line of sight through `world` (read only when los)
    uint32_t occ_margin;
    FsGridDev world;                       // the WORLD grid
    uint32_t *views;                       // [m_world]
    int32_t *n_in_view;                    // [n]
};
hipError_t fs_launch_sense_landmarks(const FsLandmarkSenseArgs &a, hipStream_t s);
// flags: views >= min_views sets flag for good; d_totals [3] += newly discovered, discovered, discovered and usable;
// d_block_counts / d_block_off [2 * ceil(m_world / 256)]: the last two per block of 256 landmarks and their exclusive sums.
hipError_t fs_launch_landmark_flags(const float *d_raw, const uint32_t *d_views, uint8_t *d_flag, int32_t m_world, uint32_t min_views,
                                    int32_t *d_block_counts, int32_t *d_block_off, int32_t *d_totals, hipStream_t s);
// scatter: the discovered landmarks' raw xyz in ascending world index -> d_raw_out [n_disc][3]; the ranks of the usable ones,
// ascending -> d_usable_out [n_usable] (what fs_cloud_order_device starts from)
hipError_t fs_launch_landmark_scatter(const float *d_raw, const uint8_t *d_flag, int32_t m_world, const int32_t *d_block_off, int32_t n_disc,
                                      int32_t n_usable, float *d_raw_out, int32_t *d_usable_out, hipStream_t s);

// ---- a drive gated on Fisher information (fs_drive_slam; fs_drive_slam.hip)
// After fs_drive's step and merge launches of step k, for the robots that swept in it (still FS_DRIVE_DRIVING, with a station k):
//   sweep — one wavefront per (robot, group of chunks): landmark_sweep_group from the robot's station-k pose record; the station's
//           in_view += landmarks seen.  (fs_launch_landmark_flags follows, by the caller.)
//   info  — FS_GATE_SLABS workgroups per robot: isPoseSafe's scalar of the station's pose straight from the WORLD cloud, counting
//           only landmarks flagged discovered; workgroup w owns the voxels whose table x index is w modulo FS_GATE_SLABS, counts
//           them in an LDS hash table of FS_GATE_SLOTS slots and, when that runs full, again in passes over ranges of its voxels'
//           indices (fallbacks [0] += 1); partial [robot][slab][2] = information, occupied voxels.
//   gate  — one lane per robot, in place of fs_drive's goal launch: the partial sums in slab order -> information / voxels of the
//           station; then MAPPED (stop_when_mapped), else UNSAFE when gated and not information > threshold.
#define FS_GATE_SLABS 8
#define FS_GATE_SLOTS 2048
struct FsDriveSlamArgs {
    FsLandmarkSenseArgs sweep;     // the world cloud and the sensor's volume as fs_sense_landmarks fills them; Rt = [total][12] pose
                                   // records of all stations, n_in_view [total] (zero-based sums); n is not used
    int32_t n_robots, step;
    const int32_t *n_stations;     // [R]
    const int32_t *station_off;    // [R]
    int32_t *state;                // [R][2], FsDriveArgs::state
    const double *goal;            // [R][3]
    FsGridDev staged;              // the staged grid: the goal test and, with occlusion, the gate's line of sight
    int32_t stop_when_mapped;
    // the gate's view: fs_set_fim_params' volume, the lookup table and fs_set_occlusion of the context (FsFimArgs' fields)
    const uint8_t *flag;           // [m_world] discovered
    int32_t cull;
    float max_dist_f, maxd2, cos2;
    int32_t cone_mode;
    const float *table;
    int32_t jx0, jy0, jz0, tx, ty, tz;
    double inv_step;
    int32_t table_full;
    const float *factor;           // [FS_FACTOR_N]
    int32_t occluded, occ_min, occ_max;
    uint32_t occ_margin;
    double *partial;               // [R][FS_GATE_SLABS][2]
    float *information;            // [total]
    int32_t *voxels;               // [total]
    int32_t *fallbacks;            // [1]
    double threshold;
    int32_t gate, gate_first;
};
hipError_t fs_launch_drive_slam_sweep(const FsDriveSlamArgs &a, hipStream_t s);
hipError_t fs_launch_drive_slam_info(const FsDriveSlamArgs &a, hipStream_t s);
hipError_t fs_launch_drive_slam_gate(const FsDriveSlamArgs &a, hipStream_t s);

// ---- FIM kernel arguments ---------------------------------------------------------------------
struct FsFimArgs {
    // landmarks: SoA in k-d leaf order, n_chunks chunks of 64 (the tail padded with far-away sentinels),
    // one bounding sphere (cx, cy, cz, r + safety margin) per chunk
    const float *lx, *ly, *lz;
    const float *spheres;      // [n_chunks][4]
    int32_t n_chunks;
    int32_t n_groups;          // passes of (waves x 64) chunks per workgroup; set by the launcher per kernel configuration
    int32_t cull;              // 0: every chunk is tested (brute force)
    // dense lookup table indexed by the integer voxel lattice
    const float *table;        // [tx][ty][tz], NaN = absent
    int32_t jx0, jy0, jz0;     // lattice index of table[0][0][0]
    int32_t tx, ty, tz;
    double inv_step;           // 1 / (double)0.3f  (FisherInfoManager.hpp:119)
    float inv_step_f;          // (float)inv_step, fast path of the voxel index
    int32_t far_lattice;       // 1: max_dist / step may reach 2^10 lattice cells — the fp32 fast path of the voxel index is not proven there
    float key_thr;             // fast path accepted while |r - rint(r)| < key_thr = 0.5 - 2 * (error bound of the fp32 product at the largest |r|)
    const float *factor;       // crowding factor by rank, [FS_FACTOR_N]; rank >= FS_FACTOR_N -> 0
    float fac1, fac2, fac3, fac4;   // factor[1..4]
    int32_t table_full;        // 1: only finite values inside the table box (true for every generated table)
    // visibility
    float maxd2;               // (float)(max_dist^2)
    float cos2;                // c*c, c = (float)cos(max_angle)
    int32_t cone_mode;         // 0 disabled, 1 c >= 0 (cone also culled per chunk), 2 c < 0, 3 c >= 0 but too wide to cull
    float max_dist_f, cos_a, sin_a;   // chunk culling (cone culled only in mode 1)
    // specialised workers (fs_fim.hip): info_only — the call reads info_ref / n_voxels only (fs_score_fim with NULL for the other
    // columns: what isPoseSafe needs); yaw_only — every pose record is a rotation about Z (checked on the host)
    int32_t info_only, yaw_only;
    int32_t learn;                    // 1: predict scoring passes with the voxel ratio learnt from finished calls (counters[ratio_slot]); 0: skip32 only
    // which learnt ratio this call predicts with and feeds: 12 — distinct voxels per landmark of the chunks in RANGE AND CONE (what the
    // cone workers hash from); 13 — per landmark of the chunks that can also meet the table's BOX (what the INFO_ONLY and the cone-off
    // workers hash from).  Two bases, two ratios: a pose shows up to twice as many voxels per landmark of the second kind.
    // Set by the launchers (fs_fim.hip), not by the caller.
    int32_t ratio_slot;
    // One pose over W = 2^split_shift workgroups (INFO_ONLY LDS worker; fs_fim.hip, SPLIT): cand_count = n * W work items, sums
    // [n * W][18], split_flags [n] (zero between calls: bit 0 a pose's item has handed the pose to the HBM tier, bit 1 the HBM
    // tier's result stands in the pose's first slot).  0: off.
    int32_t split_shift;
    uint32_t *split_flags;
    // slab w of a split pose = lattice x indices [split_bound[w], split_bound[w + 1]) (contiguous slabs; the first and the last one
    // are open-ended): cut by the host so that every slab holds the same share of the visibility volume's cross-section inside
    // the table (FS_SPLIT_MAX_W slabs at most)
    int32_t split_bound[33];
    // a split info-only call whose finish runs on the HOST (fs_capi.hip, host_finish): `sums` then points into mapped page-locked
    // memory, and an item that hands its pose to the HBM tier also raises this word there (plain store; nullptr: not such a call)
    uint32_t *host_flag;
    float box_lo[3], box_hi[3];       // the lookup table's box in the camera frame: half a voxel beyond the outermost lattice points, plus 1 mm
    // poses: Rt[n][12] (R row-major 9 + t 3), written by the host (explicit poses) or by the ray-march kernel
    int32_t n;
    const float *Rt;
    const int32_t *status;     // [n] or nullptr: status != 0 -> zero FI
    // tier 1 may be launched on a slice of the (spatially ordered) candidate list: workgroup b scores candidate
    // cand_perm[cand_lo + b] (cand_perm == nullptr: cand_lo + b), b < cand_count
    const int32_t *cand_perm;
    int32_t cand_lo, cand_count;
    // cost map of the spatial sort (fs_sort.hip), or nullptr: the landmark tests a candidate took are stored under its
    // block, costmap[cand_key[c] & (FS_COST_BINS - 1)], for the order of the next call
    uint32_t *costmap;
    const uint32_t *cand_key;
    // outputs (device)
    float *info_ref, *trace, *logdet, *fim21;   // fim21 may be nullptr
    int32_t *n_visible, *n_voxels;
    double *sums;              // [n][18] reduced per-candidate sums (info, 15 FIM block sums, n_visible, n_voxels)
    uint32_t *overflow;        // [n] tier that must re-score the candidate (0 = done)
    int32_t *flagged;          // [n] work list: candidates the LDS tier hands to the HBM tier
    uint32_t *tested;          // [n] landmark tests spent on the candidate (all tiers); zeroed by the finish kernel
    // fused scoring: the finish kernel also assembles the 32-byte records (nullptr: separate outputs only)
    fs_record *records;
    const int32_t *rec_arrival, *rec_argmax;
    const double *rec_yaw;
    const uint8_t *rec_achievable;
    unsigned long long *counters;   // [16]: 0 landmarks tested; per call 1 multi-pass candidates, 2 handed to the HBM tier, 3 unresolved; 4..6 their running totals; 8 / 9 work-list cursors of the LDS / HBM tier;
                                    // 10 / 11 landmark tests / candidates since the last spatial sort (its cost-map mean); 12 / 13 learnt voxel ratios (ratio_slot)
    // hash tables
    int32_t hash_bits;         // LDS tier (512-thread workgroups)
    int32_t skip32;            // pass-count prediction: distinct voxels <= skip32/32 of the landmarks scanned
    int32_t headroom;          // ... and, once a ratio has been learnt, headroom/32 of it (40 = 5/4) + 1/32 when that is smaller
    uint32_t *gtable;          // tier 3: HBM tables [pool][1 << ghash_bits]
    int32_t ghash_bits;
    // occlusion (fs_set_occlusion; read by the occluded worker alone, at the end so that no other field moves): a
    // landmark that passes the predicate is visible only if the line from the pose's translation to it is not blocked on `occ_grid`
    int32_t occ_min, occ_max;
    uint32_t occ_margin;       // M of the rule
    FsGridDev occ_grid;
};

#define FS_COST_BINS   8192     // blocks of the sort's cost map (13 Morton bits)
#define FS_CHUNK       64       // landmarks per chunk (one wave)
#define FS_FACTOR_N    352      // (float)exp(1 - k^0.8) is exactly 0.0f from k = 337 on
// device-side counters of a context (fs_get_counter).  FS_FIM_SCHEDULE development builds append two words per candidate
// (< FS_SCHEDULE_MAX): the 100 MHz tick at which a workgroup of the persistent FIM grid started it, and
// duration | workgroup << 32 | passes << 56 (tools/fim_schedule.py).
#define FS_SCHEDULE_MAX 32768
#if defined(FS_FIM_STAMPS_PER_WAVE)
#define FS_N_COUNTERS 80
#elif defined(FS_FIM_SCHEDULE)
#define FS_N_COUNTERS (32 + 2 * FS_SCHEDULE_MAX)
#else
#define FS_N_COUNTERS 32
#endif
#define FS_SLOT_CNT_BITS 11     // slot = (key+1) << 11 | count
#define FS_SLOT_CNT_MASK ((1u << FS_SLOT_CNT_BITS) - 1u)
#define FS_SLOT_CNT_SAT  1024u  // counts beyond this contribute exactly 0.0f anyway
#define FS_MAX_TABLE_CELLS ((1u << (32 - FS_SLOT_CNT_BITS)) - 2u)


extern std::atomic<uint64_t> fs_alloc_generation;   // bumped by every device / page-locked (re)allocation of the library (fs_capi.hip): launch graphs hold raw pointers

// launchers (defined in the .hip files)
hipError_t fs_launch_raymarch(const FsRayArgs &a, hipStream_t s);
hipError_t fs_launch_sort_candidates(int32_t n, const double *d_goal, const FsGridDev &grid, int32_t *d_perm,
                                    void **scratch, size_t *scratch_bytes, unsigned long long *d_cost_acc,
                                    const uint32_t **d_keys, uint32_t **d_costmap, int use_costmap, int reverse, hipStream_t s);
hipError_t fs_launch_fim(const FsFimArgs &a, hipStream_t s);
bool fs_fim_can_split(const FsFimArgs &a);     // may split_shift be set for this call? (needs info_only, cone_mode, table_full filled in)
hipError_t fs_launch_fim_overflow(const FsFimArgs &a, int pool, hipStream_t s);
// the occluded route (fs_set_occlusion enabled): every pose filed into the HBM tier's work list, then the HBM-tier worker with
// the line-of-sight test in its visibility; fs_launch_fim_finish follows as usual
hipError_t fs_launch_fim_occluded(const FsFimArgs &a, int pool, hipStream_t s);
hipError_t fs_launch_fim_finish(const FsFimArgs &a, hipStream_t s);
hipError_t fs_launch_selftest(int32_t max_abs, double *d_sqrt, double *d_div, hipStream_t s);

// fs_score_candidates split for the multi-device scorer (fs_capi.hip): launch everything / wait and copy out
extern "C" int fs_score_candidates_begin(fs_ctx *c, int32_t n, const double *goal_xyz, const int32_t *frontier_size,
                                         const uint8_t *blacklisted, const uint8_t *achievable_in);
extern "C" int fs_score_candidates_end(fs_ctx *c, int32_t n, fs_record *records);
extern "C" int fs_score_arrival_begin(fs_ctx *c, int32_t n, const double *goal_xyz, const int32_t *frontier_size,
                                      const uint8_t *blacklisted, const uint8_t *achievable_in, int32_t *ray_counts, int32_t *arrival,
                                      int32_t *argmax, double *yaw, uint8_t *achievable, int32_t *status);
extern "C" int fs_score_arrival_end(fs_ctx *c);
extern "C" int fs_score_fim_begin(fs_ctx *c, int32_t n, const double *pose7, float *info_ref, float *fim21, float *trace, float *logdet,
                                  int32_t *n_visible, int32_t *n_voxels);
extern "C" int fs_score_fim_end(fs_ctx *c);

// ---- multi-robot task allocation (fs_allocate.hip): MinPos and Munkres in one launch of one workgroup
struct FsAllocArgs {
    int32_t n_robots, n_tasks, method;
    const double *cost;               // [R][n] row-major
    const double *distance;           // [R][n] (MINPOS)
    int32_t *rank;                    // [R][n] MinPos' P, or nullptr
    double *modified;                 // [R][n] MinPos' matrix (MINPOS: never nullptr — the solve reads it)
    double *work;                     // [R][n] the working copy
    int32_t *assignment;              // [R]
    double *total_cost;               // [1]
    double *assigned_cost;            // [R] cost[r][assignment[r]] (NaN for -1), or nullptr
    int32_t *status;                  // [1] FS_OK / FS_E_INVALID (an entry refused: nothing else written) / FS_E_RANGE (step 5's cap)
    int32_t *stats;                   // [3] augmentations, step-5 runs, step-3 primes
};
hipError_t fs_launch_allocate(const FsAllocArgs &a, hipStream_t s);
// the fleet's R x n cost matrix (fs_rank.hip, beside u1_cost): row r from robot r's plan columns at + r * n, one workgroup per
// robot — normalisation over that robot's live set, then the U1 cost.  d_ach [R][n]: the plan's achievability in, AND the
// record's achievable flag out (what the robot's own record carries).  err: |= 1 where a utility leaves [0, 1]
hipError_t fs_launch_fleet_costs(int32_t n_robots, int32_t n, const fs_record *d_records, const uint8_t *d_black, uint8_t *d_ach,
                                 const double *d_len, const double *d_head, double alpha, double beta, double max_vx, double max_wz,
                                 double max_gt, double *d_cost, int32_t *d_err, hipStream_t s);

// pieces of fs_multi_get_frontier_costs (defined in fs_capi.hip, sequenced by fs_multi.hip)
hipStream_t fs_ctx_stream(fs_ctx *c);
int fs_ctx_device(const fs_ctx *c);
int fs_gather_begin(fs_ctx *c, int32_t n, const uint8_t *blacklisted, const double *path_length, const double *path_heading, fs_record **d_list);
int fs_block_score_begin(fs_ctx *c, int32_t n, const double *goal_xyz, const int32_t *frontier_size, const uint8_t *blacklisted,
                         const uint8_t *achievable_in, bool with_fim, fs_record *d_dst, fs_record **d_block);
int fs_block_records_to_host(fs_ctx *c, int32_t n, const fs_record *d_block, const fs_record **h_block);
int fs_gather_rank(fs_ctx *c, int32_t n, double alpha, double beta, double max_vx, double max_wz);
int fs_gather_end(fs_ctx *c, int32_t n, fs_record *records, double *weighted_cost, double *arrival_utility, double *distance_utility, int32_t *order);

#endif
