// fs_navfn.hip — the batched grid planner of fs_plan_paths / fs_navfn_potential: NavFn's potential field from
// the robot cell, computed ONCE per (grid, robot cell, allow_unknown) by a deterministic tiled schedule, and NavFn::calcPath
// from every frontier on it, one lane per frontier.
//
// Reference: DEP/src/planners/planner.cpp — setCostmap (:258-290), setupNavFn's border ring (:385-425), updateCell /
// updateCellAstar's value (:471-700), calcPath (:915-1147), gradCell (:1150-1218); the columns: DEP/src/CostCalculator.cpp:193-393.
//
// The field.  Start: POT_HIGH everywhere, 0 at the robot cell.  Update of a cell n with cost < COST_OBS: P[n] = min(P[n], T_n(P)),
// T_n the planar-wave value of its four neighbours.  T_n is not monotone (it jumps at dc == hf), so the fixed point depends on the
// order of the updates: the ORDER IS PART OF THE DEFINITION, and it is this one —
//   * the map is cut into NAVFN_TILE x NAVFN_TILE tiles; rounds read snapshot A and write B (two buffers, swapped per round);
//   * a tile is ACTIVE in a round when, in the round before, a cell changed on the edge a 4-neighbour tile shares with it (round 0:
//     the robot's tile alone).  An active tile loads its interior plus a 1-cell halo from A (outside the map: POT_HIGH), runs
//     synchronous (Jacobi) sweeps over its interior until a sweep changes nothing, writes its interior to B and reports which of
//     its four edges changed against A;
//   * an inactive tile that changed in the round before copies its interior from A to B (both buffers then agree on it again);
//   * the field is done after a round in which no tile changed.  Both buffers then hold it.
// Nothing depends on which workgroup runs when: a round reads only A and the flags of the round before.  No atomics.
// tests/navfn_ref/navfn_ref.cpp performs exactly these steps on the CPU; the tests hold this file to it bit for bit.
#include "fs_internal.h"

#include <float.h>

#define NAVFN_THREADS 256
#define NAVFN_W (NAVFN_TILE + 2)
#define NAVFN_PER_THREAD (NAVFN_TILE * NAVFN_TILE / NAVFN_THREADS)
static_assert(NAVFN_TILE * NAVFN_TILE % NAVFN_THREADS == 0, "every thread owns the same number of cells of a tile");

namespace {

constexpr float kPotHigh = 1.0e10f;     // POT_HIGH
constexpr int kObs = 254, kNeutral = 50;
constexpr float kPathStep = 0.5f;

enum : uint32_t { kChanged = 1u, kEdgeX0 = 2u, kEdgeX1 = 4u, kEdgeY0 = 8u, kEdgeY1 = 16u, kForce = 32u };

// setCostmap(cmap, isROS = true, allow_unknown) and the border ring of setupNavFn
__global__ void navfn_costs_kernel(const uint8_t *__restrict__ cells, int nx, int ny, int allow_unknown, uint8_t *__restrict__ cost)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= (int64_t)nx * ny) return;
    const int x = (int)(k % nx), y = (int)(k / nx);
    const int v = cells[k];
    int c = kObs;
    if (v < 253) {
        c = (int)(50 + 0.8 * v);             // COST_NEUTRAL + COST_FACTOR * v (double), truncated
        if (c >= kObs) c = kObs - 1;
    } else if (v == 255 && allow_unknown) {
        c = kObs - 1;
    }
    if (x == 0 || y == 0 || x == nx - 1 || y == ny - 1) c = kObs;
    cost[k] = (uint8_t)c;
}

// both buffers POT_HIGH with 0 at the robot cell; the flags of "round -1": the robot's tile forced
__global__ void navfn_init_kernel(float *__restrict__ a, float *__restrict__ b, int64_t ns, int64_t robot, uint32_t *__restrict__ flags_prev,
                                  int64_t tiles, int64_t robot_tile)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < ns) {
        const float v = (k == robot) ? 0.0f : kPotHigh;
        a[k] = v;
        b[k] = v;
    }
    if (k < tiles) flags_prev[k] = (k == robot_tile) ? kForce : 0u;
}

// updateCell's value from the four neighbours (double literals of the quadratic evaluated in double)
__device__ __forceinline__ float cell_update(float l, float r, float u, float d, float hf)
{
    float tc = (l < r) ? l : r;
    float ta = (u < d) ? u : d;
    float dc = tc - ta;
    if (dc < 0) { dc = -dc; ta = tc; }
    if (dc >= hf) return ta + hf;
    const float q = dc / hf;
    const float v = (float)(-0.2301 * (double)q * (double)q + 0.5307 * (double)q + 0.7040);
    return ta + hf * v;
}

// One round: workgroup t = one tile.  any[0] is raised (plain store of 1) when a tile changed.
__global__ __launch_bounds__(NAVFN_THREADS) void navfn_round_kernel(const float *__restrict__ A, float *__restrict__ B, const uint8_t *__restrict__ cost,
                                                                     const uint32_t *__restrict__ prev, uint32_t *__restrict__ cur, int nx, int ny,
                                                                     int tx, int ty, int32_t *__restrict__ any)
{
    __shared__ float s[2][NAVFN_W * NAVFN_W];
    const int t = blockIdx.x, i = t % tx, j = t / tx, tid = threadIdx.x;
    const uint32_t self = prev[t];
    const bool active = (self & kForce) || (i > 0 && (prev[t - 1] & kEdgeX1)) || (i + 1 < tx && (prev[t + 1] & kEdgeX0)) ||
                        (j > 0 && (prev[t - tx] & kEdgeY1)) || (j + 1 < ty && (prev[t + tx] & kEdgeY0));
    const int x0 = i * NAVFN_TILE, y0 = j * NAVFN_TILE, x1 = min(x0 + NAVFN_TILE, nx), y1 = min(y0 + NAVFN_TILE, ny);
    if (!active) {
        if (tid == 0) cur[t] = 0u;
        if (self & kChanged)
            for (int k = tid; k < NAVFN_TILE * NAVFN_TILE; k += NAVFN_THREADS) {
                const int x = x0 + (k % NAVFN_TILE), y = y0 + (k / NAVFN_TILE);
                if (x < x1 && y < y1) B[(int64_t)y * nx + x] = A[(int64_t)y * nx + x];
            }
        return;
    }
    for (int k = tid; k < NAVFN_W * NAVFN_W; k += NAVFN_THREADS) {
        const int x = x0 - 1 + (k % NAVFN_W), y = y0 - 1 + (k / NAVFN_W);
        const float v = (x >= 0 && y >= 0 && x < nx && y < ny) ? A[(int64_t)y * nx + x] : kPotHigh;
        s[0][k] = v;
        s[1][k] = v;
    }
    // the cells this thread owns: their LDS slot, cost (>= COST_OBS or off the map: never updated) and value in A
    int slot[NAVFN_PER_THREAD];
    float hf[NAVFN_PER_THREAD], orig[NAVFN_PER_THREAD];
    bool upd[NAVFN_PER_THREAD];
#pragma unroll
    for (int q = 0; q < NAVFN_PER_THREAD; ++q) {
        const int k = tid + q * NAVFN_THREADS, lx = k % NAVFN_TILE, ly = k / NAVFN_TILE, x = x0 + lx, y = y0 + ly;
        slot[q] = (ly + 1) * NAVFN_W + lx + 1;
        const bool in = x < x1 && y < y1;
        const int c = in ? cost[(int64_t)y * nx + x] : kObs;
        upd[q] = c < kObs;
        hf[q] = (float)c;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NAVFN_PER_THREAD; ++q) orig[q] = s[0][slot[q]];
    int src = 0;
    for (;;) {
        const float *S = s[src];
        float *D = s[src ^ 1];
        int ch = 0;
#pragma unroll
        for (int q = 0; q < NAVFN_PER_THREAD; ++q) {
            const int l = slot[q];
            float p = S[l];
            if (upd[q]) {
                const float pot = cell_update(S[l - 1], S[l + 1], S[l - NAVFN_W], S[l + NAVFN_W], hf[q]);
                if (pot < p) { p = pot; ch = 1; }
            }
            D[l] = p;
        }
        src ^= 1;
        if (!__syncthreads_or(ch)) break;
    }
    uint32_t bits = 0;
#pragma unroll
    for (int q = 0; q < NAVFN_PER_THREAD; ++q) {
        const int k = tid + q * NAVFN_THREADS, lx = k % NAVFN_TILE, ly = k / NAVFN_TILE, x = x0 + lx, y = y0 + ly;
        if (x >= x1 || y >= y1) continue;
        const float p = s[src][slot[q]];
        B[(int64_t)y * nx + x] = p;
        if (p != orig[q]) {
            bits |= kChanged;
            if (x == x0) bits |= kEdgeX0;
            if (x == x1 - 1) bits |= kEdgeX1;
            if (y == y0) bits |= kEdgeY0;
            if (y == y1 - 1) bits |= kEdgeY1;
        }
    }
    uint32_t all = 0;
    if (__syncthreads_or(bits & kChanged)) all |= kChanged;
    if (__syncthreads_or(bits & kEdgeX0)) all |= kEdgeX0;
    if (__syncthreads_or(bits & kEdgeX1)) all |= kEdgeX1;
    if (__syncthreads_or(bits & kEdgeY0)) all |= kEdgeY0;
    if (__syncthreads_or(bits & kEdgeY1)) all |= kEdgeY1;
    if (tid == 0) {
        cur[t] = all;
        if (all) any[0] = 1;
    }
}

// ---------------------------------------------------------------- calcPath, one lane per frontier
__device__ __forceinline__ float hyp(float x, float y) { return (float)sqrt((double)x * x + (double)y * y); }

// `int minp = potarr[...]` as x86-64 converts: POT_HIGH (out of the int range) becomes INT_MIN
__device__ __forceinline__ int to_int_x86(float f) { return (f >= 2147483648.0f || f < -2147483648.0f || f != f) ? INT_MIN : (int)f; }

struct Field {
    const float *P;
    int nx;
    int64_t ns;
    __device__ float pot(int64_t i) const { return (i >= 0 && i < ns) ? P[i] : kPotHigh; }   // outside the array: POT_HIGH
    // gradCell: the normalised gradient of cell n ((0, 0) on the first / last row and where the norm is 0)
    __device__ void grad(int64_t n, float &gx, float &gy) const
    {
        gx = 0.0f; gy = 0.0f;
        if (n < nx || n > ns - nx) return;
        const float cv = pot(n);
        float dx = 0.0f, dy = 0.0f;
        if (cv >= kPotHigh) {
            if (pot(n - 1) < kPotHigh) dx = -(float)kObs;
            else if (pot(n + 1) < kPotHigh) dx = (float)kObs;
            if (pot(n - nx) < kPotHigh) dy = -(float)kObs;
            else if (pot(n + nx) < kPotHigh) dy = (float)kObs;
        } else {
            if (pot(n - 1) < kPotHigh) dx += pot(n - 1) - cv;
            if (pot(n + 1) < kPotHigh) dx += cv - pot(n + 1);
            if (pot(n - nx) < kPotHigh) dy += pot(n - nx) - cv;
            if (pot(n + nx) < kPotHigh) dy += cv - pot(n + nx);
        }
        float norm = hyp(dx, dy);
        if (norm > 0) {
            norm = (float)(1.0 / (double)norm);
            gx = norm * dx;
            gy = norm * dy;
        }
    }
};

__global__ void navfn_paths_kernel(FsNavfnPathArgs a)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= a.n) return;
    const double dmax = DBL_MAX;
    double len_pts = dmax, len_m = dmax, head = dmax;
    uint8_t ok = 0;
    const int32_t goal = a.goal_cell[f];
    const Field F{a.pot, a.nx, (int64_t)a.nx * a.ny};
    if (goal >= 0 && F.pot(goal) < kPotHigh) {
        float *px = a.scratch + (int64_t)f * 2 * a.max_cycles, *py = px + a.max_cycles;
        const int nx = a.nx;
        const int64_t ns = F.ns;
        int64_t stc = goal;
        float dx = 0.0f, dy = 0.0f;
        int npath = 0, len = 0;
        for (int it = 0; it < a.max_cycles; ++it) {
            const int64_t near_raw = stc + (int64_t)(int)round((double)dx) + (int64_t)(int)((double)nx * round((double)dy));
            const int64_t nearest = max((int64_t)0, min(ns - 1, near_raw));
            if (F.pot(nearest) < (float)kNeutral) {
                px[npath] = (float)a.robot_x; py[npath] = (float)a.robot_y;
                len = ++npath;
                break;
            }
            if (stc < nx || stc > ns - nx) break;
            px[npath] = (float)(int)(stc % nx) + dx;
            py[npath] = (float)(int)(stc / nx) + dy;
            ++npath;
            const bool osc = npath > 2 && px[npath - 1] == px[npath - 3] && py[npath - 1] == py[npath - 3];
            const int64_t up = stc - nx, dn = stc + nx;
            if (F.pot(stc) >= kPotHigh || F.pot(stc + 1) >= kPotHigh || F.pot(stc - 1) >= kPotHigh || F.pot(dn) >= kPotHigh ||
                F.pot(dn + 1) >= kPotHigh || F.pot(dn - 1) >= kPotHigh || F.pot(up) >= kPotHigh || F.pot(up + 1) >= kPotHigh ||
                F.pot(up - 1) >= kPotHigh || osc) {
                // follow the grid to the lowest of the eight neighbours (compared against an int, as the reference's minp)
                int64_t minc = stc;
                int minp = to_int_x86(F.pot(stc));
                const int64_t cand[8] = {up - 1, up, up + 1, stc - 1, stc + 1, dn - 1, dn, dn + 1};
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (F.pot(cand[k]) < (float)minp) { minp = to_int_x86(F.pot(cand[k])); minc = cand[k]; }
                stc = minc;
                dx = 0.0f; dy = 0.0f;
                if (F.pot(stc) >= kPotHigh) break;
            } else {
                float g0x, g0y, g1x, g1y, g2x, g2y, g3x, g3y;
                F.grad(stc, g0x, g0y); F.grad(stc + 1, g1x, g1y); F.grad(dn, g2x, g2y); F.grad(dn + 1, g3x, g3y);
                const float x1 = (float)((1.0 - (double)dx) * (double)g0x + (double)(dx * g1x));
                const float x2 = (float)((1.0 - (double)dx) * (double)g2x + (double)(dx * g3x));
                const float x = (float)((1.0 - (double)dy) * (double)x1 + (double)(dy * x2));
                const float y1 = (float)((1.0 - (double)dx) * (double)g0y + (double)(dx * g1y));
                const float y2 = (float)((1.0 - (double)dx) * (double)g2y + (double)(dx * g3y));
                const float y = (float)((1.0 - (double)dy) * (double)y1 + (double)(dy * y2));
                if (x == 0.0f && y == 0.0f) break;
                const float ss = kPathStep / hyp(x, y);
                dx += x * ss;
                dy += y * ss;
                if (dx > 1.0f) { ++stc; dx = (float)((double)dx - 1.0); }
                if (dx < -1.0f) { --stc; dx = (float)((double)dx + 1.0); }
                if (dy > 1.0f) { stc += nx; dy = (float)((double)dy - 1.0); }
                if (dy < -1.0f) { stc -= nx; dy = (float)((double)dy + 1.0); }
            }
        }
        if (len > 0) {
            // CostCalculator.cpp:303-315: mapToWorld(unsigned, unsigned) of every point, segments (i, i+1) for i = len-2 .. 1
            double s = 0.0, prev_x = 0.0, prev_y = 0.0;
            for (int k = len - 1; k >= 0; --k) {
                const double wx = a.ox + ((double)(uint32_t)(int64_t)px[k] + 0.5) * a.res;
                const double wy = a.oy + ((double)(uint32_t)(int64_t)py[k] + 0.5) * a.res;
                if (k != 0 && k != len - 1) {
                    const double ex = wx - prev_x, ey = wy - prev_y;
                    s += sqrt(ex * ex + ey * ey);
                }
                prev_x = wx; prev_y = wy;
            }
            ok = 1;
            len_pts = (double)len;
            len_m = s;
            head = a.heading_in[f];
        }
    }
    a.path_length[f] = len_pts;
    if (a.path_length_m) a.path_length_m[f] = len_m;
    a.path_heading[f] = head;
    a.achievable[f] = ok;
}

}  // namespace

hipError_t fs_launch_navfn_costs(const uint8_t *d_cells, int nx, int ny, int allow_unknown, uint8_t *d_cost, hipStream_t s)
{
    const int64_t ns = (int64_t)nx * ny;
    hipLaunchKernelGGL(navfn_costs_kernel, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, s, d_cells, nx, ny, allow_unknown, d_cost);
    return hipGetLastError();
}

hipError_t fs_launch_navfn_init(float *d_a, float *d_b, int nx, int ny, int rx, int ry, uint32_t *d_flags_prev, hipStream_t s)
{
    const int64_t ns = (int64_t)nx * ny, tx = (nx + NAVFN_TILE - 1) / NAVFN_TILE, ty = (ny + NAVFN_TILE - 1) / NAVFN_TILE;
    const int64_t tiles = tx * ty, m = ns > tiles ? ns : tiles;
    hipLaunchKernelGGL(navfn_init_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, d_a, d_b, ns, (int64_t)ry * nx + rx, d_flags_prev, tiles,
                       (int64_t)(ry / NAVFN_TILE) * tx + rx / NAVFN_TILE);
    return hipGetLastError();
}

hipError_t fs_launch_navfn_round(const float *d_a, float *d_b, const uint8_t *d_cost, const uint32_t *d_prev, uint32_t *d_cur, int nx, int ny,
                                 int32_t *d_any, hipStream_t s)
{
    const int tx = (nx + NAVFN_TILE - 1) / NAVFN_TILE, ty = (ny + NAVFN_TILE - 1) / NAVFN_TILE;
    hipLaunchKernelGGL(navfn_round_kernel, dim3((unsigned)(tx * ty)), dim3(NAVFN_THREADS), 0, s, d_a, d_b, d_cost, d_prev, d_cur, nx, ny, tx, ty, d_any);
    return hipGetLastError();
}

hipError_t fs_launch_navfn_paths(const FsNavfnPathArgs &a, hipStream_t s)
{
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(navfn_paths_kernel, dim3((unsigned)((a.n + 63) / 64)), dim3(64), 0, s, a);
    return hipGetLastError();
}
