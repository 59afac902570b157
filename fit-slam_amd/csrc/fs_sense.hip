// fs_sense.hip — the sensor sweep on a ground-truth world (fs_sense), surroundingCellsMapped for a batch (fs_goals_mapped) and the
// explored-cell census (fs_grid_census).  DESIGN.md 4.22.
//
// The sweep is this project's own extension: the reference's map comes from its depth camera and the traversability mapper, which
// are outside the vendored tree.  What it walks is the reference's: the arrival fan of setArrivalInformationForFrontier
// (DEP/src/CostCalculator.cpp:23-121) — direction table, end point clamp, both worldToMap truncations and getTracedCells' visit
// count evaluated as fs_raymarch.hip evaluates them (fs_walk.h) — through a second dense image of the grid's shape, the WORLD.
//   sense  — one wavefront per pose, rays on lanes (r = lane, lane + 64, ...).  A first pass over the pose's USED rays finds out
//            whether any end point is off the map (then the pose sees nothing, as the arrival fan aborts, :50-55).  The second
//            pass walks them: every visit up to and including the first whose world cost is an obstacle is SEEN — a plain byte
//            store of 1 into the mark image (many lanes store the same value: no race, no owner) — and the visits before it whose
//            staged cost is in the trace range are counted.  Seen cells of a ray lie between its start cell and its last seen cell
//            (a Bresenham walk is monotone on every axis), so the pose's bounding box is a wave reduction over those two cells per
//            ray and goes out with one atomicMin / atomicMax per wave and axis.
//   merge  — over the bounding window, x fastest: where the mark is set, staged = world, the cell is counted (seen; revealed when
//            it was 255 and the world is not) and the mark is cleared, so the image is all zero between calls.  Wave sums, then
//            one atomic per block and counter.
// Every figure is an integer sum, minimum or maximum: nothing depends on the order the device works in.
// The fan walk of one pose, the goal predicate and the block sums live in fs_sense_dev.h: fs_drive.hip runs them too.
#include "fs_internal.h"
#include "fs_walk.h"
#include "fs_sense_dev.h"       // the fan walk, the goal predicate and the block sums, shared with fs_drive.hip

#define FS_SENSE_WAVES 4        // poses per workgroup

namespace {

__global__ __launch_bounds__(FS_SENSE_WAVES * 64)
void fs_sense_kernel(const FsSenseArgs a)
{
    const int lane = threadIdx.x & 63;
    const int p = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * FS_SENSE_WAVES + (threadIdx.x >> 6)));
    if (p >= a.n) return;
    const int n_rays = a.n_yaw * a.n_elev;
    const double sx = a.origin[3 * (size_t)p], sy = a.origin[3 * (size_t)p + 1], sz = a.origin[3 * (size_t)p + 2];
    const int first = a.first_ray ? a.first_ray[p] : -1;
    int32_t *ray_out = a.ray_unknown ? a.ray_unknown + (size_t)p * (size_t)n_rays : nullptr;
    const SenseFan f = sense_fan(a, lane, sx, sy, sz, first, ray_out);
    if (lane != 0) return;
    if (!f.ok) { a.seen_unknown[p] = 0; a.status[p] = FS_STATUS_OFF_MAP; return; }
    a.seen_unknown[p] = f.total;
    a.status[p] = FS_STATUS_OK;
    atomicMin(a.box + 0, (int)f.bx0); atomicMin(a.box + 1, (int)f.by0); atomicMin(a.box + 2, (int)f.bz0);
    atomicMax(a.box + 3, (int)f.bx1); atomicMax(a.box + 4, (int)f.by1); atomicMax(a.box + 5, (int)f.bz1);
}

__global__ __launch_bounds__(256)
void fs_sense_merge_kernel(const uint8_t *__restrict__ world, uint8_t *__restrict__ staged, uint8_t *__restrict__ mark, int nx, int ny,
                           int x0, int y0, int z0, int sx, int sy, int sz, unsigned long long *d_counts)
{
    const unsigned long long cells = (unsigned long long)sx * (unsigned long long)sy * (unsigned long long)sz;
    const unsigned long long stride = (unsigned long long)gridDim.x * 256ull;
    unsigned long long v[2] = {0ull, 0ull};
    for (unsigned long long t = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; t < cells; t += stride) {
        const unsigned long long row = t / (unsigned)sx;
        const int x = (int)(t - row * (unsigned)sx), z = (int)(row / (unsigned)sy), y = (int)(row - (unsigned long long)z * (unsigned)sy);
        const size_t at = ((size_t)(z0 + z) * (size_t)ny + (size_t)(y0 + y)) * (size_t)nx + (size_t)(x0 + x);
        if (mark[at]) {
            const uint8_t w = world[at], s = staged[at];
            staged[at] = w;
            mark[at] = (uint8_t)0;
            v[0] += 1ull;
            v[1] += (s == 255 && w != 255) ? 1ull : 0ull;
        }
    }
    block_add<2>(v, d_counts);
}

// surroundingCellsMapped for a batch, one lane per goal (goal_mapped, fs_sense_dev.h)
__global__ void fs_goals_mapped_kernel(const uint8_t *__restrict__ cells, int nx, int ny, double ox, double oy, double res, int32_t n,
                                       const double *__restrict__ goal, uint8_t *__restrict__ mapped)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    mapped[g] = goal_mapped(cells, nx, ny, ox, oy, res, goal[3 * (size_t)g], goal[3 * (size_t)g + 1]) ? 1 : 0;
}

__device__ __forceinline__ void census_byte(uint32_t c, unsigned long long (&v)[4])
{
    v[0] += c != 255u; v[1] += c == 255u; v[2] += c == 254u; v[3] += c == 0u;
}

__global__ __launch_bounds__(256)
void fs_grid_census_kernel(const uint8_t *__restrict__ cells, size_t total, unsigned long long *d_counts)
{
    const size_t words = total / 16, stride = (size_t)gridDim.x * 256;
    const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long v[4] = {0ull, 0ull, 0ull, 0ull};
    for (size_t w = tid; w < words; w += stride) {                            // (the image starts on an allocation boundary)
        const uint4 q = reinterpret_cast<const uint4 *>(cells)[w];
        const uint32_t d[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int b = 0; b < 4; ++b) census_byte((d[k] >> (8 * b)) & 255u, v);
    }
    for (size_t i = words * 16 + tid; i < total; i += stride) census_byte(cells[i], v);
    block_add<4>(v, d_counts);
}

}  // namespace

hipError_t fs_launch_sense(const FsSenseArgs &a, hipStream_t s)
{
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(fs_sense_kernel, dim3((unsigned)((a.n + FS_SENSE_WAVES - 1) / FS_SENSE_WAVES)), dim3(FS_SENSE_WAVES * 64), 0, s, a);
    return hipGetLastError();
}

hipError_t fs_launch_sense_merge(const uint8_t *d_world, uint8_t *d_staged, uint8_t *d_mark, int nx, int ny, int x0, int y0, int z0,
                                 int sx, int sy, int sz, unsigned long long *d_counts, hipStream_t s)
{
    const unsigned long long cells = (unsigned long long)sx * (unsigned long long)sy * (unsigned long long)sz;
    if (cells == 0) return hipSuccess;
    const unsigned long long blocks = (cells + 255) / 256;
    hipLaunchKernelGGL(fs_sense_merge_kernel, dim3((unsigned)(blocks < 65536ull ? blocks : 65536ull)), dim3(256), 0, s, d_world, d_staged, d_mark,
                       nx, ny, x0, y0, z0, sx, sy, sz, d_counts);
    return hipGetLastError();
}

hipError_t fs_launch_goals_mapped(const uint8_t *d_cells, int nx, int ny, double ox, double oy, double res, int32_t n, const double *d_goal,
                                  uint8_t *d_mapped, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(fs_goals_mapped_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d_cells, nx, ny, ox, oy, res, n, d_goal, d_mapped);
    return hipGetLastError();
}

hipError_t fs_launch_grid_census(const uint8_t *d_cells, size_t total, unsigned long long *d_counts, hipStream_t s)
{
    if (total == 0) return hipSuccess;
    const size_t blocks = (total / 16 + 255) / 256 + 1;
    hipLaunchKernelGGL(fs_grid_census_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s, d_cells, total, d_counts);
    return hipGetLastError();
}
