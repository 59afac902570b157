// fs_sense_dev.h — device code the sensor sweep (fs_sense.hip) shares with the drive (fs_drive.hip, DESIGN.md
// 4.24): one pose's fan walked through the world by one wavefront, surroundingCellsMapped for one goal, and the block sums of
// the merge kernels.  Device code only; included after fs_internal.h and fs_walk.h.
#ifndef FS_SENSE_DEV_H_
#define FS_SENSE_DEV_H_

#include "fs_internal.h"
#include "fs_walk.h"

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

// What one wavefront's sweep of one pose gives, the same in every lane: ok = the pose sees something (else the fan aborted and
// nothing was marked); total = the staged-unknown visits of its used rays; the seen cells' bounding box.
struct SenseFan {
    bool ok;
    int total;
    uint32_t bx0, by0, bz0, bx1, by1, bz1;
};

// One pose's fan from (sx, sy, sz), rays on lanes (r = lane, lane + 64, ...), `first` as FsSenseArgs::first_ray's entries.  A
// first pass over the pose's USED rays finds out whether any end point is off the map (then the pose sees nothing, as the
// arrival fan aborts, :50-55).  The second pass walks them: every visit up to and including the first whose world cost is an
// obstacle is SEEN — a plain byte store of 1 into the mark image (many lanes store the same value: no race, no owner) — and the
// visits before it whose staged cost is in the trace range are counted (per ray into ray_out [n_elev][n_yaw] when given; an
// aborted fan zeroes it).  Seen cells of a ray lie between its start cell and its last seen cell (a Bresenham walk is monotone
// on every axis), so the pose's bounding box is a wave reduction over those two cells per ray.
__device__ __forceinline__ SenseFan sense_fan(const FsSenseArgs &a, int lane, double sx, double sy, double sz, int first, int32_t *ray_out)
{
    const int n_rays = a.n_yaw * a.n_elev;
    const int i_lo = first < 0 ? 0 : first, i_hi = first < 0 ? a.n_yaw : first + a.window;     // used yaws [i_lo, i_hi)

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
        return SenseFan{false, 0, 0u, 0u, 0u, 0u, 0u, 0u};
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
    return SenseFan{true, total, bx0, by0, bz0, bx1, by1, bz1};
}

// sum over the wave's lanes, in every lane
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// the block's sums of up to four per-thread counters into d_counts: wave sums, then one atomic per counter (blocks of 256)
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

// surroundingCellsMapped (DEP/src/Helpers.cpp:98-133) for one goal on a 2-D image, with nhood4 / nhood8 / nhood20 (:185-275) as
// loops over the offsets the reference pushes, each behind the reference's own edge test
__device__ __forceinline__ bool goal_mapped(const uint8_t *__restrict__ cells, int nx, int ny, double ox, double oy, double res, double gx, double gy)
{
    const FsGridDev grid{cells, nx, ny, 1, ox, oy, 0.0, res, nullptr, nullptr, {0u, 0u, 0u}, 0u, nullptr};
    uint32_t mx, my, mz;
    if (!world_to_map(grid, gx, gy, 0.0, mx, my, mz)) return false;           // :101-104
    const int cx = (int)mx, cy = (int)my;
    auto in = [&](int x, int y) { return x >= 0 && x < nx && y >= 0 && y < ny; };
    auto cost = [&](int x, int y) { return (int)cells[(size_t)y * (size_t)nx + (size_t)x]; };
    if (cost(cx, cy) == 254) return true;                                     // :106-107
    int lethal = 0;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx)
            if ((dx || dy) && in(cx + dx, cy + dy) && cost(cx + dx, cy + dy) == 254) ++lethal;   // :111-118 over nhood8
    if (lethal >= 3) return true;
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
    return !unknown;
}

}  // namespace

#endif
