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
#include "fs_internal.h"
#include "fs_walk.h"

#define FS_SENSE_WAVES 4        // poses per workgroup

namespace {

__device__ __forceinline__ double std_min(double a, double b) { return (b < a) ? b : a; }   // std::min(a,b)
__device__ __forceinline__ double std_max(double a, double b) { return (a < b) ? b : a; }   // std::max(a,b)

// ray r = e * n_yaw + i of the pose's fan: its clamped end point (CostCalculator.cpp:42-48, as fs_raymarch_kernel forms it)
__device__ __forceinline__ void sense_end_point(const FsSenseArgs &a, int r, double sx, double sy, double sz, double &wx, double &wy, double &wz)
{
    wx = sx + a.dir[3 * r];
    wy = sy + a.dir[3 * r + 1];
    wz = sz + a.dir[3 * r + 2];
    wx = std_max(a.lo_x, std_min(a.hi_x, wx));
    wy = std_max(a.lo_y, std_min(a.hi_y, wy));
    wz = std_max(a.lo_z, std_min(a.hi_z, wz));
}

__global__ __launch_bounds__(FS_SENSE_WAVES * 64)
void fs_sense_kernel(const FsSenseArgs a)
{
    const int lane = threadIdx.x & 63;
    const int p = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * FS_SENSE_WAVES + (threadIdx.x >> 6)));
    if (p >= a.n) return;
    const int n_rays = a.n_yaw * a.n_elev;
    const double sx = a.origin[3 * (size_t)p], sy = a.origin[3 * (size_t)p + 1], sz = a.origin[3 * (size_t)p + 2];
    const int first = a.first_ray ? a.first_ray[p] : -1;
    const int i_lo = first < 0 ? 0 : first, i_hi = first < 0 ? a.n_yaw : first + a.window;     // used yaws [i_lo, i_hi)
    int32_t *ray_out = a.ray_unknown ? a.ray_unknown + (size_t)p * (size_t)n_rays : nullptr;

    uint32_t x0 = 0, y0 = 0, z0 = 0;
    const bool start_ok = world_to_map(a.world, sx, sy, sz, x0, y0, z0);
    bool fail = !start_ok;
    if (start_ok) {
        for (int r = lane; r < n_rays; r += 64) {
            const int i = r % a.n_yaw;
            if (i < i_lo || i >= i_hi) continue;
            double wx, wy, wz;
            sense_end_point(a, r, sx, sy, sz, wx, wy, wz);
            uint32_t x1, y1, z1;
            if (!world_to_map(a.world, wx, wy, wz, x1, y1, z1)) fail = true;
        }
    }
    if (__any(fail)) {                           // :50-55 — the first failing ray aborts the fan: nothing is seen
        if (ray_out)
            for (int r = lane; r < n_rays; r += 64) ray_out[r] = 0;
        if (lane == 0) { a.seen_unknown[p] = 0; a.status[p] = FS_STATUS_OFF_MAP; }
        return;
    }

    // the visitor's inclusive ranges intersected with a byte's, one unsigned compare each (an empty range matches nothing)
    const int omin = a.obst_min > 0 ? a.obst_min : 0, omax = a.obst_max < 255 ? a.obst_max : 255;
    const int tmin = a.trace_min > 0 ? a.trace_min : 0, tmax = a.trace_max < 255 ? a.trace_max : 255;
    const bool o_any = omax >= omin, t_any = tmax >= tmin;
    const uint32_t orange = o_any ? (uint32_t)(omax - omin) : 0u, trange = t_any ? (uint32_t)(tmax - tmin) : 0u;
    const uint32_t nx = (uint32_t)a.world.nx, ny = (uint32_t)a.world.ny;

    int total = 0;
    uint32_t bx0 = x0, by0 = y0, bz0 = z0, bx1 = x0, by1 = y0, bz1 = z0;      // every used ray sees at least the start cell
    for (int r = lane; r < n_rays; r += 64) {
        const int i = r % a.n_yaw;
        int count = 0;
        if (i >= i_lo && i < i_hi) {
            double wx, wy, wz;
            sense_end_point(a, r, sx, sy, sz, wx, wy, wz);
            uint32_t x1, y1, z1;
            (void)world_to_map(a.world, wx, wy, wz, x1, y1, z1);               // (succeeded in the first pass)
            WalkLinear w;
            walk_init(w, a.world, x0, y0, z0, x1, y1, z1, (double)a.max_length);
            uint32_t last = w.offset;
            for (uint32_t v = 0; v <= w.end; ++v) {
                const int cw = walk_cell(a.world, w);
#ifdef FS_RAY_BOUNDS
                if (cw == 256) break;                                          // the walk left the grid (recorded): no store there
#endif
                const int cs = (int)a.staged[w.offset];
                a.mark[w.offset] = (uint8_t)1;
                last = w.offset;
                if (o_any && (uint32_t)(cw - omin) <= orange) break;           // the wall's face is seen; it ends the ray
                count += (t_any && (uint32_t)(cs - tmin) <= trange) ? 1 : 0;
                walk_step(w);
            }
            const uint32_t row = last / nx;
            const uint32_t lx = last - row * nx, lz = row / ny, ly = row - lz * ny;
            bx0 = min(bx0, lx); bx1 = max(bx1, lx);
            by0 = min(by0, ly); by1 = max(by1, ly);
            bz0 = min(bz0, lz); bz1 = max(bz1, lz);
        }
        if (ray_out) ray_out[r] = count;
        total += count;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        total += __shfl_xor(total, d);
        bx0 = min(bx0, (uint32_t)__shfl_xor((int)bx0, d)); bx1 = max(bx1, (uint32_t)__shfl_xor((int)bx1, d));
        by0 = min(by0, (uint32_t)__shfl_xor((int)by0, d)); by1 = max(by1, (uint32_t)__shfl_xor((int)by1, d));
        bz0 = min(bz0, (uint32_t)__shfl_xor((int)bz0, d)); bz1 = max(bz1, (uint32_t)__shfl_xor((int)bz1, d));
    }
    if (lane == 0) {
        a.seen_unknown[p] = total;
        a.status[p] = FS_STATUS_OK;
        atomicMin(a.box + 0, (int)bx0); atomicMin(a.box + 1, (int)by0); atomicMin(a.box + 2, (int)bz0);
        atomicMax(a.box + 3, (int)bx1); atomicMax(a.box + 4, (int)by1); atomicMax(a.box + 5, (int)bz1);
    }
}

// sum over the wave's lanes, in every lane
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// the block's sums of up to four per-thread counters into d_counts: wave sums, then one atomic per counter
template <int K>
__device__ __forceinline__ void block_add(const unsigned long long (&v)[K], unsigned long long *d_counts)
{
    __shared__ unsigned long long s_part[4][K];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const unsigned long long s = wave_sum(v[k]);
        if (lane == 0) s_part[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < K) {
        const unsigned long long s = s_part[0][threadIdx.x] + s_part[1][threadIdx.x] + s_part[2][threadIdx.x] + s_part[3][threadIdx.x];
        if (s) atomicAdd(d_counts + threadIdx.x, s);
    }
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

// surroundingCellsMapped (DEP/src/Helpers.cpp:98-133) with nhood4 / nhood8 / nhood20 (:185-275) as loops over the offsets the
// reference pushes, each behind the reference's own edge test
__global__ void fs_goals_mapped_kernel(const uint8_t *__restrict__ cells, int nx, int ny, double ox, double oy, double res, int32_t n,
                                       const double *__restrict__ goal, uint8_t *__restrict__ mapped)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    const FsGridDev grid{cells, nx, ny, 1, ox, oy, 0.0, res, nullptr, nullptr, {0u, 0u, 0u}, 0u, nullptr};
    uint32_t mx, my, mz;
    if (!world_to_map(grid, goal[3 * (size_t)g], goal[3 * (size_t)g + 1], 0.0, mx, my, mz)) { mapped[g] = 0; return; }   // :101-104
    const int cx = (int)mx, cy = (int)my;
    auto in = [&](int x, int y) { return x >= 0 && x < nx && y >= 0 && y < ny; };
    auto cost = [&](int x, int y) { return (int)cells[(size_t)y * (size_t)nx + (size_t)x]; };
    if (cost(cx, cy) == 254) { mapped[g] = 1; return; }                       // :106-107
    int lethal = 0;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx)
            if ((dx || dy) && in(cx + dx, cy + dy) && cost(cx + dx, cy + dy) == 254) ++lethal;   // :111-118 over nhood8
    if (lethal >= 3) { mapped[g] = 1; return; }
    bool unknown = false;                                                     // :121-130 over nhood20
    const int n4[4][2] = {{-1, 0}, {1, 0}, {0, -1}, {0, 1}};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int qx = cx + n4[k][0], qy = cy + n4[k][1];
        if (!in(qx, qy)) continue;
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx)                                  // the neighbour itself (nhood4) and its nhood8
                if (in(qx + dx, qy + dy) && cost(qx + dx, qy + dy) == 255) unknown = true;
    }
    mapped[g] = unknown ? 0 : 1;
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
