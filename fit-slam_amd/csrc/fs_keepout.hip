// fs_keepout.hip — keep-out zones on the staged 2-D grid: what the reference's costmap layer LethalMarker does to
// the master grid (fit_slam2_nav2_plugins/plugins/keepout_layer.cpp:279-300: markCells writes 253 into every cached cell of
// every zone, every cycle, whatever the cycle's bounds).
//
// (1) Mark.  The end cells of a zone's rays are computed on the host (fp64 + libm, fs_keepout.h); the device walks integers
//     only: one lane per ray, each stores 1 into a byte image for every cell of its line.  Lanes that meet on a cell store
//     the same value.
// (2) Apply / fold.  cells[i] = src[i] ? 253 : cells[i] over a rectangle, four cells per lane where the rectangle allows
//     (rows of the image start at any byte: the groups are aligned in the image's linear index, the ends of a row go byte by
//     byte).  `fold` is the step of ONE new zone: src is the scratch image that zone was marked into — its cells are counted
//     (the zone's distinct cells, n_cells), enter the union mask and leave the scratch image.
#include "fs_internal.h"
#include "fs_keepout.h"

namespace {

__global__ __launch_bounds__(256)
void fs_keepout_mark_kernel(const fs_ko_ray *__restrict__ rays, long long n_rays, uint8_t *__restrict__ image, int nx, int ny)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rays) return;
    const fs_ko_ray r = rays[i];
    // (the walk stays inside the box its two ends span: both on the map = every store on the map)
    if (r.ax < 0 || r.ax >= nx || r.ex < 0 || r.ex >= nx || r.ay < 0 || r.ay >= ny || r.ey < 0 || r.ey >= ny) return;
    fs_ko_walk(r, [&](int32_t x, int32_t y) { image[(size_t)y * (size_t)nx + (size_t)x] = 1; });
}

// One lane per aligned group of four cells of one row of the rectangle; groups_per_row covers a row from the group its first
// cell falls into to the group of its last one.
template <bool FOLD>
__global__ __launch_bounds__(256)
void fs_keepout_apply_kernel(uint8_t *src, uint8_t *mask, uint8_t *__restrict__ cells, int nx, int x0, int y0, int sx, int sy,
                             int groups_per_row, unsigned long long *count)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    int found = 0;
    if (t < (long long)groups_per_row * sy) {
        const int g = (int)(t % groups_per_row), y = y0 + (int)(t / groups_per_row);
        const size_t lo = (size_t)y * (size_t)nx + (size_t)x0, hi = lo + (size_t)sx;          // the row's cells [lo, hi)
        const size_t base = (lo & ~(size_t)3) + 4 * (size_t)g;
        if (base >= lo && base + 4 <= hi) {
            const uint32_t m = *reinterpret_cast<const uint32_t *>(src + base);                // bytes 0 / 1
            if (m) {
                const uint32_t sel = m * 0xFFu;                                                // 0x00 / 0xFF per byte
                uint32_t *cw = reinterpret_cast<uint32_t *>(cells + base);
                *cw = (*cw & ~sel) | (0x01010101u * FS_KO_COST & sel);
                if (FOLD) {
                    uint32_t *mw = reinterpret_cast<uint32_t *>(mask + base);
                    *mw |= m;
                    *reinterpret_cast<uint32_t *>(src + base) = 0u;
                }
                found = __popc(m);
            }
        } else {
            const size_t end = base + 4 < hi ? base + 4 : hi;
            for (size_t i = base > lo ? base : lo; i < end; ++i) {
                if (!src[i]) continue;
                cells[i] = FS_KO_COST;
                if (FOLD) { mask[i] = 1; src[i] = 0; }
                ++found;
            }
        }
    }
    if (count) {                                                                               // (uniform over the launch)
        for (int d = 32; d >= 1; d >>= 1) found += __shfl_xor(found, d);
        if ((threadIdx.x & 63) == 0 && found) atomicAdd(count, (unsigned long long)found);
    }
}

template <bool FOLD>
hipError_t launch_apply(uint8_t *src, uint8_t *mask, uint8_t *cells, int nx, int ny, int x0, int y0, int sx, int sy,
                        unsigned long long *count, hipStream_t s)
{
    if (sx <= 0 || sy <= 0) return hipSuccess;
    if (x0 < 0 || y0 < 0 || (long long)x0 + sx > nx || (long long)y0 + sy > ny) return hipErrorInvalidValue;
    const int groups_per_row = (sx + 3) / 4 + 1;
    const long long total = (long long)groups_per_row * sy;
    hipLaunchKernelGGL(fs_keepout_apply_kernel<FOLD>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s,
                       src, mask, cells, nx, x0, y0, sx, sy, groups_per_row, count);
    return hipGetLastError();
}

}  // namespace

hipError_t fs_launch_keepout_mark(const int32_t *d_rays, int64_t n_rays, uint8_t *d_image, int nx, int ny, hipStream_t s)
{
    if (n_rays <= 0) return hipSuccess;
    hipLaunchKernelGGL(fs_keepout_mark_kernel, dim3((unsigned)((n_rays + 255) / 256)), dim3(256), 0, s,
                       reinterpret_cast<const fs_ko_ray *>(d_rays), (long long)n_rays, d_image, nx, ny);
    return hipGetLastError();
}

hipError_t fs_launch_keepout_apply(const uint8_t *d_mask, uint8_t *d_cells, int nx, int ny, int x0, int y0, int sx, int sy,
                                   unsigned long long *d_count, hipStream_t s)
{
    return launch_apply<false>(const_cast<uint8_t *>(d_mask), nullptr, d_cells, nx, ny, x0, y0, sx, sy, d_count, s);
}

hipError_t fs_launch_keepout_fold(uint8_t *d_src, uint8_t *d_mask, uint8_t *d_cells, int nx, int ny, int x0, int y0, int sx, int sy,
                                  unsigned long long *d_count, hipStream_t s)
{
    return launch_apply<true>(d_src, d_mask, d_cells, nx, ny, x0, y0, sx, sy, d_count, s);
}
