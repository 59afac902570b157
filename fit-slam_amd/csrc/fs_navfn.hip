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
//
// The REFERENCE search (fs_set_grid_search) does not use that field: per distinct goal cell it runs the reference's own partial wave
// (NavFn::calcNavFnAstar, defined once in fs_navfn_wave.h), one wavefront per wave, and descends on that wave's field — the
// kernels at the end of this file.
#include "fs_internal.h"
#include "fs_navfn_wave.h"

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
                const float pot = fs_nw_cell_update(S[l - 1], S[l + 1], S[l - NAVFN_W], S[l + NAVFN_W], hf[q]);
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

// calcPath from frontier f down `field` and the four columns (the points go to the frontier's scratch)
__device__ __forceinline__ void navfn_descend(const FsNavfnPathArgs &a, int f, const float *__restrict__ field)
{
    const double dmax = DBL_MAX;
    double len_pts = dmax, len_m = dmax, head = dmax;
    uint8_t ok = 0;
    const int32_t goal = a.goal_cell[f];
    const Field F{field, a.nx, (int64_t)a.nx * a.ny};
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

__global__ void navfn_paths_kernel(FsNavfnPathArgs a)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= a.n) return;
    navfn_descend(a, f, a.pot);
}

// ---------------------------------------------------------------- the REFERENCE search: one wave per distinct goal cell
// (fs_navfn_wave.h holds the wave's definition; this is its walk in chunks of 64 entries, one per lane)

// The distinct goal cells of a list whose cells lie in device memory.  first[f]: the lowest frontier with f's cell (-1: not planned).
__global__ void navfn_wave_first_kernel(const int32_t *__restrict__ cell, int32_t n, int32_t *__restrict__ first)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n) return;
    const int32_t c = cell[f];
    int32_t g = -1;
    if (c >= 0)
        for (g = 0; g < f; ++g)
            if (cell[g] == c) break;
    first[f] = g;
}

// ... their waves in order of first appearance: frontier_wave[f], wave_cell[wave]; thread n counts them into stats[0]
__global__ void navfn_wave_rank_kernel(const int32_t *__restrict__ cell, const int32_t *__restrict__ first, int32_t n,
                                       int32_t *__restrict__ wave_cell, int32_t *__restrict__ frontier_wave, int32_t *__restrict__ stats)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f > n) return;
    const int32_t upto = (f == n) ? n : first[f];
    int32_t r = 0;
    for (int32_t g = 0; g < upto; ++g) r += (first[g] == g) ? 1 : 0;
    if (f == n) { stats[0] = r; return; }
    frontier_wave[f] = (upto < 0) ? -1 : r;
    if (upto == f) wave_cell[r] = cell[f];
}

// the slots of a batch: POT_HIGH, nothing pending (blockIdx.y = slot; slots beyond the list's last wave are left alone)
__global__ void navfn_wave_fill_kernel(FsNavfnWaveArgs a, int32_t base)
{
    const int slot = blockIdx.y;
    if (base + slot >= a.stats[0]) return;
    const int64_t ns = (int64_t)a.nx * a.ny, k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= ns) return;
    a.pot[slot * ns + k] = kPotHigh;
    a.pending[slot * ns + k] = 0;
}

__device__ __forceinline__ int32_t uni(int32_t v) { return __builtin_amdgcn_readfirstlane(v); }

// One workgroup of ONE wavefront per slot; wave `base + slot` of the call.  The wave's control state (fill counts, curT, limit, the
// three buffer pointers) is held by every lane and computed from wave-uniform values only; lane k of a chunk owns entry k.
// Lanes hand values to each other through global memory (potential, pending, buffers), and the compiler orders memory per lane
// only: every phase that reads what another lane wrote in the phase before is separated from it by __syncthreads().  For a
// workgroup of one wavefront that is a workgroup-scope release/acquire fence plus a barrier the wave passes at once; the lanes share
// one CU's write-through L1, so workgroup scope is enough.  No atomic decides anything (the three statistics at the end are counted
// with atomics and read by nobody on the device).  Every loop is bounded before it starts: cycles, cur_n, the bits of `todo`.
__global__ __launch_bounds__(FS_NW_WIDTH) void navfn_wave_kernel(FsNavfnWaveArgs a, int32_t base)
{
    const int slot = blockIdx.x, lane = threadIdx.x;
    const int32_t wid = base + slot;
    if (wid >= a.stats[0]) return;
    const int32_t nx = a.nx;
    const int64_t ns = (int64_t)nx * a.ny;
    const fs_nw_map m{a.cost, nx, a.ny};
    const int32_t goal = a.wave_cell[wid];
    fs_nw_wave w{};
    w.pot = a.pot + slot * ns;
    w.pending = a.pending + slot * ns;
    w.cur = a.buf + (int64_t)slot * 3 * a.cap; w.next = w.cur + a.cap; w.over = w.next + a.cap;
    w.cap = a.cap;
    w.sx = goal % nx; w.sy = goal / nx;
    w.hash = nullptr;
    int32_t cycles = 0;
    if (lane == 0) cycles = fs_nw_begin(m, w, a.rx, a.ry);
    cycles = uni(cycles);
    w.cur_n = uni(w.cur_n); w.next_n = 0; w.over_n = 0;
    w.limit = uni(w.limit);
    w.curT = __int_as_float(uni(__float_as_int(w.curT)));
    __syncthreads();
    int32_t cycle = 0, replays = 0;
    for (; cycle < cycles; ++cycle) {
        if (w.cur_n == 0 && w.next_n == 0) break;
        for (int32_t i = lane; i < w.cur_n; i += FS_NW_WIDTH) w.pending[w.cur[i]] = 0;
        __syncthreads();
        for (int32_t at = 0; at < w.cur_n;) {
            const int32_t cnt = min(FS_NW_WIDTH, w.cur_n - at);
            // evaluate: every lane its entry, from memory
            fs_nw_eval e;
            e.cell = 0; e.p = 0.0f; e.bits = 0u;
            e.pos[0] = e.pos[1] = e.pos[2] = e.pos[3] = 0;
            if (lane < cnt) e = fs_nw_evaluate(m, w, w.cur[at + lane]);
            // commit, in entry order, in wave-uniform code: entry j's bits and cell are broadcast, the appends and the cap are
            // decided on the uniform fill counts, the later lanes react in registers
            uint64_t todo = __ballot((e.bits & (FS_NW_STORE | FS_NW_CANDS)) != 0u);
            uint64_t dep = 0;
            while (todo) {
                const int j = uni((int32_t)__builtin_ctzll(todo));
                if (dep && (int)__builtin_ctzll(dep) <= j) break;
                todo &= todo - 1;
                const int32_t cell_j = __builtin_amdgcn_readlane(e.cell, j);
                uint32_t bits_j = (uint32_t)__builtin_amdgcn_readlane((int32_t)e.bits, j);
                int32_t pos[4] = {0, 0, 0, 0};
                bits_j = fs_nw_commit_entry(w.next_n, w.over_n, w.limit, w.cap, bits_j, pos);
                const bool mine = lane == j;
                const uint32_t met = fs_nw_react(e.bits, e.cell, nx, cell_j, bits_j);
                e.bits = mine ? bits_j : ((lane > j && lane < cnt) ? met : e.bits);
                e.pos[0] = mine ? pos[0] : e.pos[0]; e.pos[1] = mine ? pos[1] : e.pos[1];
                e.pos[2] = mine ? pos[2] : e.pos[2]; e.pos[3] = mine ? pos[3] : e.pos[3];
                dep = __ballot((e.bits & FS_NW_DEP) != 0u);
            }
            // the prefix up to the first entry whose evaluation an earlier store made stale is final; the next chunk starts there
            // (lane 0 is never stale: a chunk advances by at least one entry)
            const int32_t done = dep ? min(cnt, (int32_t)__builtin_ctzll(dep)) : cnt;
            if (lane < done) fs_nw_commit_write(w, nx, e);
            if (done < cnt) ++replays;
            at += done;
            __syncthreads();
        }
        fs_nw_end_cycle(w);
        if (w.pot[goal] < kPotHigh) break;
    }
    if (cycle >= cycles) w.limit |= FS_NW_LIMIT_CYCLES;
    if (lane == 0) {
        a.wave_limit[wid] = w.limit;
        if (w.limit & FS_NW_LIMIT_CYCLES) atomicAdd(&a.stats[1], 1);
        if (w.limit & FS_NW_LIMIT_CAP) atomicAdd(&a.stats[2], 1);
        if (replays) atomicAdd(&a.stats[3], replays);
    }
}

// the descents of a batch: every frontier whose wave ran in it, on its wave's slot; the frontiers without a wave with batch 0
__global__ void navfn_paths_wave_kernel(FsNavfnPathArgs a, FsNavfnWaveArgs wv, int32_t base)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= a.n) return;
    const int32_t wid = wv.frontier_wave[f];
    if (wid < 0 ? base != 0 : (wid < base || wid >= base + wv.slots)) return;
    navfn_descend(a, f, wid < 0 ? wv.pot : wv.pot + (int64_t)(wid - base) * a.nx * a.ny);
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

hipError_t fs_launch_navfn_wave_cells(const int32_t *d_cell, int32_t n, int32_t *d_first, int32_t *d_wave_cell, int32_t *d_frontier_wave,
                                      int32_t *d_stats, hipStream_t s)
{
    if (n > 0) hipLaunchKernelGGL(navfn_wave_first_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, d_cell, n, d_first);
    hipLaunchKernelGGL(navfn_wave_rank_kernel, dim3((unsigned)((n + 64) / 64)), dim3(64), 0, s, d_cell, d_first, n, d_wave_cell, d_frontier_wave, d_stats);
    return hipGetLastError();
}

hipError_t fs_launch_navfn_wave_batch(const FsNavfnWaveArgs &w, int32_t base, int32_t count, hipStream_t s)
{
    if (count <= 0) return hipSuccess;
    const int64_t ns = (int64_t)w.nx * w.ny;
    hipLaunchKernelGGL(navfn_wave_fill_kernel, dim3((unsigned)((ns + 255) / 256), (unsigned)count), dim3(256), 0, s, w, base);
    hipLaunchKernelGGL(navfn_wave_kernel, dim3((unsigned)count), dim3(FS_NW_WIDTH), 0, s, w, base);
    return hipGetLastError();
}

hipError_t fs_launch_navfn_paths_wave(const FsNavfnPathArgs &a, const FsNavfnWaveArgs &w, int32_t base, hipStream_t s)
{
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(navfn_paths_wave_kernel, dim3((unsigned)((a.n + 63) / 64)), dim3(64), 0, s, a, w, base);
    return hipGetLastError();
}
