// fs_inflate.hip — the inflation layer on the staged 2-D grid: nav2 Humble's InflationLayer::computeCost and the
// write rule of InflationLayer::updateCosts, with the EXACT distance to the nearest lethal cell in place of the layer's ordered
// brushfire.  The transform is separable and everything on the device is an integer:
//
// (1) Rows.  One wavefront per 64 cells of one row of the window grown by R and clipped to the map.  A ballot per 64 cells gives
//     a bit image of the seeds (cells == 254): the wave's own word and up to ceil(R / 64) words on either side.  Each lane finds
//     its nearest set bit to the left and to the right with count-leading / count-trailing zeros and stores
//     g = min |dx| <= R as uint16, FS_INFL_NONE where the row has no seed within R.  Only the columns of the write window are
//     stored; the waves over the grown margin count their seeds (n_seeds) and stop.
// (2) Columns.  One workgroup per 64 columns x 16 rows of the write window, one lane per column and four rows: the rows
//     [tile - R, tile + R] of g pass through LDS in chunks of 64 rows (R reaches 512: the halo never has to fit at once), each
//     row read once per lane updates four running minima of dy^2 + g^2.  A row of g that is "none" for the whole wavefront is
//     skipped; no |dy| <= R test is needed — dy^2 alone is beyond R^2 then, and a cell whose minimum is beyond R^2 is untouched.
//     Then the cost from the host's table (the device never calls exp), the write rule, and one wave-reduced atomic for n_changed.
//
// The rows pass reads the cells and writes g; the columns pass reads g and writes the cells: in place without a second image.
#include "fs_internal.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr unsigned FS_INFL_NONE = 0xFFFFu;               // g: no seed within R in this row
constexpr unsigned FS_INFL_FAR = 0x40000000u;            // its square in the column pass: beyond every R^2, and + dy^2 cannot wrap
constexpr int FS_INFL_SIDE_WORDS = (FS_INFLATE_MAX_CELLS + 63) / 64;
constexpr int FS_INFL_TILE_ROWS = 16, FS_INFL_ROWS_PER_LANE = 4, FS_INFL_CHUNK_ROWS = 64;

__global__ __launch_bounds__(256)
void fs_inflate_rows_kernel(const uint8_t *__restrict__ cells, int nx, FsInflateBox b, int x0, int sx, int R, int side_words,
                            int blocks_per_row, uint16_t *__restrict__ g, unsigned long long *n_seeds)
{
    __shared__ unsigned long long words[4][2 * FS_INFL_SIDE_WORDS + 1];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = b.gy0 + (int)(blockIdx.x / (unsigned)blocks_per_row);
    const int span = (int)(blockIdx.x % (unsigned)blocks_per_row) * 4 + wave;
    const int xs = b.gx0 + span * 64, gx1 = b.gx0 + b.gw;              // the wave's cells [xs, xs + 64) of the grown window [gx0, gx1)
    const bool stores = xs < x0 + sx && xs + 64 > x0;                  // (wave-uniform) some of them are columns of the write window
    const uint8_t *line = cells + (size_t)row * (size_t)nx;
    if (xs < gx1) {
        for (int j = stores ? -side_words : 0; j <= (stores ? side_words : 0); ++j) {
            const int x = xs + 64 * j + lane;
            const bool seed = x >= b.gx0 && x < gx1 && line[x] == 254;
            const unsigned long long w = __ballot(seed);
            if (lane == 0) {
                words[wave][j + side_words] = w;
                if (j == 0 && w) atomicAdd(n_seeds, (unsigned long long)__popcll(w));
            }
        }
    }
    __syncthreads();
    const int x = xs + lane;
    if (!stores || x < x0 || x >= x0 + sx) return;
    const unsigned long long *w = words[wave] + side_words;           // w[j]: cells [xs + 64 j, xs + 64 j + 64)
    unsigned left = FS_INFL_NONE, right = FS_INFL_NONE;
    unsigned long long m = w[0] & (~0ull >> (63 - lane));              // bits 0 .. lane
    if (m) left = (unsigned)(lane - (63 - __builtin_clzll(m)));
    else
        for (int j = 1; j <= side_words; ++j)
            if (w[-j]) { left = (unsigned)(lane + 64 * (j - 1) + 1 + __builtin_clzll(w[-j])); break; }
    m = w[0] & (~0ull << lane);                                        // bits lane .. 63
    if (m) right = (unsigned)(__builtin_ctzll(m) - lane);
    else
        for (int j = 1; j <= side_words; ++j)
            if (w[j]) { right = (unsigned)(64 * j + __builtin_ctzll(w[j]) - lane); break; }
    const unsigned d = left < right ? left : right;
    g[(size_t)(row - b.gy0) * (size_t)sx + (size_t)(x - x0)] = (uint16_t)(d <= (unsigned)R ? d : FS_INFL_NONE);
}

__global__ __launch_bounds__(256)
void fs_inflate_cols_kernel(const uint16_t *__restrict__ g, const uint8_t *__restrict__ cost_by_d2, uint8_t *__restrict__ cells, int nx,
                            FsInflateBox b, int x0, int y0, int sx, int sy, int R, int inflate_unknown, int col_tiles,
                            unsigned long long *n_changed)
{
    __shared__ uint16_t tile[FS_INFL_CHUNK_ROWS][64];
    const int wave = threadIdx.x >> 6, col = threadIdx.x & 63;
    const int cx = (int)(blockIdx.x % (unsigned)col_tiles) * 64 + col;                // column of the window
    const bool col_ok = cx < sx;
    const int ty0 = y0 + (int)(blockIdx.x / (unsigned)col_tiles) * FS_INFL_TILE_ROWS;  // the tile's rows [ty0, ty1) of the map
    const int ty1 = ty0 + FS_INFL_TILE_ROWS < y0 + sy ? ty0 + FS_INFL_TILE_ROWS : y0 + sy;
    const int yb = ty0 + wave * FS_INFL_ROWS_PER_LANE;                                 // this lane's rows yb .. yb + 3
    const int s0 = ty0 - R > b.gy0 ? ty0 - R : b.gy0;                                  // rows of g that can reach the tile: [s0, s1)
    const int s1 = ty1 + R < b.gy0 + b.gh ? ty1 + R : b.gy0 + b.gh;
    unsigned best[FS_INFL_ROWS_PER_LANE];
#pragma unroll
    for (int k = 0; k < FS_INFL_ROWS_PER_LANE; ++k) best[k] = FS_INFL_FAR;
    for (int c0 = s0; c0 < s1; c0 += FS_INFL_CHUNK_ROWS) {                             // (uniform over the workgroup)
        const int n = s1 - c0 < FS_INFL_CHUNK_ROWS ? s1 - c0 : FS_INFL_CHUNK_ROWS;
        __syncthreads();
        for (int r = wave; r < n; r += 4)
            tile[r][col] = col_ok ? g[(size_t)(c0 + r - b.gy0) * (size_t)sx + (size_t)cx] : (uint16_t)FS_INFL_NONE;
        __syncthreads();
        for (int r = 0; r < n; ++r) {
            const unsigned gv = tile[r][col];
            if (!__ballot(gv != FS_INFL_NONE)) continue;
            const unsigned gg = gv == FS_INFL_NONE ? FS_INFL_FAR : gv * gv;
            const int dy = c0 + r - yb;
#pragma unroll
            for (int k = 0; k < FS_INFL_ROWS_PER_LANE; ++k) {
                const unsigned d2 = gg + (unsigned)((dy - k) * (dy - k));
                best[k] = d2 < best[k] ? d2 : best[k];
            }
        }
    }
    int changed = 0;
#pragma unroll
    for (int k = 0; k < FS_INFL_ROWS_PER_LANE; ++k) {
        const int y = yb + k;
        if (!col_ok || y >= ty1 || best[k] > (unsigned)(R * R)) continue;
        const unsigned c = cost_by_d2[best[k]];
        uint8_t *cell = cells + (size_t)y * (size_t)nx + (size_t)(x0 + cx);
        const unsigned o = *cell;
        // InflationLayer::updateCosts: NO_INFORMATION takes the cost where it is positive (inflate_unknown) or inscribed and above,
        // every other cell the larger of the two
        const unsigned v = (o == 255u && (inflate_unknown ? c > 0u : c >= 253u)) ? c : (o > c ? o : c);
        if (v != o) { *cell = (uint8_t)v; ++changed; }
    }
    for (int d = 32; d >= 1; d >>= 1) changed += __shfl_xor(changed, d);
    if (col == 0 && changed) atomicAdd(n_changed, (unsigned long long)changed);
}

bool window_ok(int nx, int ny, int x0, int y0, int sx, int sy, int R)
{
    return nx > 0 && ny > 0 && sx > 0 && sy > 0 && x0 >= 0 && y0 >= 0 && (long long)x0 + sx <= nx && (long long)y0 + sy <= ny &&
           R >= 1 && R <= FS_INFLATE_MAX_CELLS;
}

}  // namespace

int fs_inflation_cell_radius(double inflation_radius, double res)
{
    // Costmap2D::cellDistance: (unsigned int)max(0.0, ceil(world_dist / resolution)) — compared as a double first, a radius
    // beyond the limit is never converted
    const double cells = std::max(0.0, std::ceil(inflation_radius / res));
    return cells <= (double)FS_INFLATE_MAX_CELLS ? (int)cells : -1;
}

void fs_inflation_cost_table(const fs_inflation_params &p, double res, int R, uint8_t *cost_by_d2)
{
    // InflationLayer::computeCost (nav2_costmap_2d/inflation_layer.hpp, Humble) for distance sqrt(d2) cells; LETHAL_OBSTACLE 254,
    // INSCRIBED_INFLATED_OBSTACLE 253
    for (int d2 = 0; d2 <= R * R; ++d2) {
        uint8_t cost = 254;
        if (d2 > 0) {
            const double euclidean_distance = std::sqrt((double)d2) * res;
            if (euclidean_distance <= p.inscribed_radius) cost = 253;
            else cost = (unsigned char)((253 - 1) * std::exp(-1.0 * p.cost_scaling_factor * (euclidean_distance - p.inscribed_radius)));
        }
        cost_by_d2[d2] = cost;
    }
}

hipError_t fs_launch_inflate_rows(const uint8_t *d_cells, int nx, int ny, int x0, int y0, int sx, int sy, int R, uint16_t *d_g,
                                  unsigned long long *d_n_seeds, hipStream_t s)
{
    if (!window_ok(nx, ny, x0, y0, sx, sy, R)) return hipErrorInvalidValue;
    const FsInflateBox b = fs_inflate_box(nx, ny, x0, y0, sx, sy, R);
    const int blocks_per_row = (b.gw + 255) / 256;
    const long long blocks = (long long)blocks_per_row * b.gh;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fs_inflate_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, s, d_cells, nx, b, x0, sx, R, (R + 63) / 64,
                       blocks_per_row, d_g, d_n_seeds);
    return hipGetLastError();
}

hipError_t fs_launch_inflate_cols(const uint16_t *d_g, const uint8_t *d_cost_by_d2, uint8_t *d_cells, int nx, int ny, int x0, int y0,
                                  int sx, int sy, int R, int inflate_unknown, unsigned long long *d_n_changed, hipStream_t s)
{
    if (!window_ok(nx, ny, x0, y0, sx, sy, R)) return hipErrorInvalidValue;
    const FsInflateBox b = fs_inflate_box(nx, ny, x0, y0, sx, sy, R);
    const int col_tiles = (sx + 63) / 64;
    const long long blocks = (long long)col_tiles * ((sy + FS_INFL_TILE_ROWS - 1) / FS_INFL_TILE_ROWS);
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fs_inflate_cols_kernel, dim3((unsigned)blocks), dim3(256), 0, s, d_g, d_cost_by_d2, d_cells, nx, b, x0, y0, sx, sy,
                       R, inflate_unknown ? 1 : 0, col_tiles, d_n_changed);
    return hipGetLastError();
}
