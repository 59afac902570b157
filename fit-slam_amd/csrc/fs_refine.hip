// fs_refine.hip — the any-angle leg refinement of fs_refine_paths / fs_refine_field: the path the robot drives to
// its next goal (FullPathOptimizer::refineAndPublishPath and getNextGoal's per-leg plans, computePathBetweenPointsThetaStar), restated
// as data-parallel work — a converged fp64 cost field per start cell, one descent per leg, Theta*'s parent rule along the descent.
//
// Reference: DEP/src/Helpers.cpp:540-588 (the planner's set-up and refusals), DEP/include/.../planners/theta_star.hpp (getCost,
// isSafe in both forms, getTraversalCost, getEuclideanCost, moves[]), DEP/src/planners/theta_star.cpp (resetParent, losCheck,
// backtrace, linearInterpolation).
//
// The field.  g(start) = trav(start); every other safe cell v: g(v) = min over the first `corners` moves of ((g(u) + euc(u, v)) +
// trav(v)), u = v + move.  Every step costs at least w_euc > 0, so the fixed point is unique and does NOT depend on the schedule:
// the map is cut into RF_TILE x RF_TILE tiles, a round runs every tile whose neighbourhood (edges, and corners with 8 moves) changed
// in the round before (round 0: the start's tile), a tile relaxes its interior in LDS Gauss-Seidel sweeps until a sweep changes
// nothing and writes back the cells that changed.  One buffer per field: only a cell's tile writes it, values only decrease, a
// halo read while its owner writes is an upper bound either way.  The field is done after a round in which no tile changed.  No
// atomics.  blockIdx.y = field: every field a call needs is relaxed in the same launches.
//
// The legs, one wave each: the descent from the goal (lanes = moves, the first move in moves[] order whose cell satisfies the
// field's equation with equality), the chain c0 = start ... cP = goal with resetParent's rule (a line of sight to the parent's
// parent, walked by all 64 lanes: Bresenham's position at step k is closed-form and the sum is an exact int64), the vertices, and
// backtrace + linearInterpolation.  tests/thetastar_ref/thetastar_ref.cpp restates all of it; the tests hold this file to it bit
// for bit.
//
// The REFERENCE search (fs_set_refine_search): the reference's Theta* search itself, stated once in fs_thetastar.h.  One wavefront per
// search; a slot of global memory holds its cell map, heap and records.  The search is serial: every lane runs the header's steps
// with the same values (wave-uniform code, ordinary stores), and the wave's width is spent inside a step — resetParent's walk puts
// iteration k on lane k mod 64, gathers the terms in LDS and adds them in walk order (an ordered fold, not a tree); setNeighbors
// evaluates the moves on lanes 0..corners-1 and commits them one by one in moves[] order.  No hypot is computed here: the host's
// table is read (fs_thetastar.h).
#include "fs_internal.h"
#include "fs_thetastar.h"

#include <float.h>

#define RF_THREADS 256
#define RF_W (RF_TILE + 2)
#define RF_PER_THREAD (RF_TILE * RF_TILE / RF_THREADS)
static_assert(RF_TILE * RF_TILE % RF_THREADS == 0, "every thread owns the same number of cells of a tile");

namespace {

constexpr double kInf = DBL_MAX;
__constant__ int kMx[8] = {0, 0, 1, -1, 1, -1, 1, -1};
__constant__ int kMy[8] = {1, -1, 0, 0, -1, 1, 1, -1};

enum : uint32_t {
    kChanged = 1u, kEdgeX0 = 2u, kEdgeX1 = 4u, kEdgeY0 = 8u, kEdgeY1 = 16u,
    kC00 = 32u, kC10 = 64u, kC01 = 128u, kC11 = 256u,          // corner cells: (x side, y side), 0 = low, 1 = high
    kForce = 512u
};

__device__ __forceinline__ bool rf_safe(int v, int allow) { return (v == 255 && allow) || v < 254; }
// getTraversalCost: w * c * c / 254 / 254, c = getCost = 26 + 0.9 * raw
__device__ __forceinline__ double rf_trav(int v, double w) { const double c = 26 + 0.9 * (double)v; return w * c * c / 254 / 254; }

__global__ void rf_init_kernel(FsRefineFieldArgs a, uint32_t *__restrict__ flags_prev)
{
    const int f = blockIdx.y;
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t ns = (int64_t)a.nx * a.ny;
    const int32_t src = a.f[f].src;
    double *G = a.g + (int64_t)a.f[f].slot * ns;
    if (k < ns) {
        double v = kInf;
        if (k == src) {
            const int c = a.cells[k];
            if (rf_safe(c, a.allow)) v = rf_trav(c, a.w_trav);
        }
        G[k] = v;
    }
    const int64_t tiles = (int64_t)a.tx * a.ty;
    if (k < tiles) {
        const int sx = src % a.nx, sy = src / a.nx;
        flags_prev[(int64_t)f * tiles + k] = (k == (int64_t)(sy / RF_TILE) * a.tx + sx / RF_TILE) ? kForce : 0u;
    }
}

// One round: blockIdx.x = tile, blockIdx.y = field.  any[f] is raised (plain store of 1) when a tile of field f changed.
__global__ __launch_bounds__(RF_THREADS) void rf_round_kernel(FsRefineFieldArgs a, const uint32_t *__restrict__ prev_all,
                                                              uint32_t *__restrict__ cur_all, int32_t *__restrict__ any)
{
    __shared__ double s[RF_W * RF_W];
    const int f = blockIdx.y, t = blockIdx.x, tx = a.tx, ty = a.ty, nx = a.nx, ny = a.ny, tid = threadIdx.x;
    const int64_t tiles = (int64_t)tx * ty, ns = (int64_t)nx * ny;
    const uint32_t *prev = prev_all + (int64_t)f * tiles;
    uint32_t *cur = cur_all + (int64_t)f * tiles;
    double *G = a.g + (int64_t)a.f[f].slot * ns;
    const int32_t src = a.f[f].src;
    const int i = t % tx, j = t / tx;
    const bool diag = a.corners == 8;
    bool active = (prev[t] & kForce) || (i > 0 && (prev[t - 1] & kEdgeX1)) || (i + 1 < tx && (prev[t + 1] & kEdgeX0)) ||
                  (j > 0 && (prev[t - tx] & kEdgeY1)) || (j + 1 < ty && (prev[t + tx] & kEdgeY0));
    if (diag && !active)
        active = (i > 0 && j > 0 && (prev[t - tx - 1] & kC11)) || (i + 1 < tx && j > 0 && (prev[t - tx + 1] & kC01)) ||
                 (i > 0 && j + 1 < ty && (prev[t + tx - 1] & kC10)) || (i + 1 < tx && j + 1 < ty && (prev[t + tx + 1] & kC00));
    if (!active) {
        if (tid == 0) cur[t] = 0u;
        return;
    }
    const int x0 = i * RF_TILE, y0 = j * RF_TILE, x1 = min(x0 + RF_TILE, nx), y1 = min(y0 + RF_TILE, ny);
    for (int k = tid; k < RF_W * RF_W; k += RF_THREADS) {
        const int x = x0 - 1 + (k % RF_W), y = y0 - 1 + (k / RF_W);
        s[k] = (x >= 0 && y >= 0 && x < nx && y < ny) ? G[(int64_t)y * nx + x] : kInf;
    }
    int off[8];
    double e[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) { off[m] = kMy[m] * RF_W + kMx[m]; e[m] = a.e[m]; }
    int slot[RF_PER_THREAD];
    double tr[RF_PER_THREAD], orig[RF_PER_THREAD];
    bool upd[RF_PER_THREAD];
#pragma unroll
    for (int q = 0; q < RF_PER_THREAD; ++q) {
        const int k = tid + q * RF_THREADS, lx = k % RF_TILE, ly = k / RF_TILE, x = x0 + lx, y = y0 + ly;
        slot[q] = (ly + 1) * RF_W + lx + 1;
        const bool in = x < x1 && y < y1;
        const int64_t cell = (int64_t)y * nx + x;
        const int c = in ? a.cells[cell] : 254;
        upd[q] = in && cell != src && rf_safe(c, a.allow);
        tr[q] = rf_trav(c, a.w_trav);
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < RF_PER_THREAD; ++q) orig[q] = s[slot[q]];
    for (;;) {
        int ch = 0;
#pragma unroll
        for (int q = 0; q < RF_PER_THREAD; ++q) {
            if (!upd[q]) continue;
            const int l = slot[q];
            double m = s[l];
            for (int mv = 0; mv < a.corners; ++mv) {
                const double cand = (s[l + off[mv]] + e[mv]) + tr[q];
                if (cand < m) m = cand;
            }
            if (m < s[l]) { s[l] = m; ch = 1; }
        }
        if (!__syncthreads_or(ch)) break;
    }
    uint32_t bits = 0;
#pragma unroll
    for (int q = 0; q < RF_PER_THREAD; ++q) {
        const int k = tid + q * RF_THREADS, x = x0 + k % RF_TILE, y = y0 + k / RF_TILE;
        if (x >= x1 || y >= y1) continue;
        const double v = s[slot[q]];
        if (v != orig[q]) {
            G[(int64_t)y * nx + x] = v;
            bits |= kChanged;
            const bool lx = x == x0, hx = x == x1 - 1, ly = y == y0, hy = y == y1 - 1;
            if (lx) bits |= kEdgeX0;
            if (hx) bits |= kEdgeX1;
            if (ly) bits |= kEdgeY0;
            if (hy) bits |= kEdgeY1;
            if (lx && ly) bits |= kC00;
            if (hx && ly) bits |= kC10;
            if (lx && hy) bits |= kC01;
            if (hx && hy) bits |= kC11;
        }
    }
    uint32_t all = 0;
    for (uint32_t b = kChanged; b <= kC11; b <<= 1)
        if (__syncthreads_or(bits & b)) all |= b;
    if (tid == 0) {
        cur[t] = all;
        if (all) any[f] = 1;
    }
}

// ---------------------------------------------------------------- the legs, one wave each

// One cell of a line-of-sight walk (the three-argument isSafe): false if unsafe or off the map, else (2600 + 90 raw)^2 (unknown
// with allow_unknown: 25300^2)
__device__ __forceinline__ bool rf_los_cell(const FsRefineLegArgs &a, int x, int y, int64_t &term)
{
    if (x < 0 || y < 0 || x >= a.nx || y >= a.ny) return false;
    const int v = a.cells[(int64_t)y * a.nx + x];
    if (v == 255 && a.allow) { term = (int64_t)25300 * 25300; return true; }
    if (v >= 254) return false;
    const int64_t q = 2600 + 90 * (int64_t)v;
    term = q * q;
    return true;
}

__device__ __forceinline__ int64_t wave_sum(int64_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// losCheck from (x0, y0) to (x1, y1), iteration k of the Bresenham loop on lane k mod 64: before iteration k the major coordinate
// has moved k steps, the minor one floor(k m / n), and the error term is k m mod n.  Returns (wave-uniform) the line of sight and
// the exact integer sum.
__device__ bool rf_los(const FsRefineLegArgs &a, int x0, int y0, int x1, int y1, int64_t &sum)
{
    const int dx = abs(x1 - x0), dy = abs(y1 - y0);
    const int sx = x1 > x0 ? 1 : -1, sy = y1 > y0 ? 1 : -1;
    const int ux = (sx - 1) / 2, uy = (sy - 1) / 2;
    const bool xmaj = dx >= dy;
    const int n = xmaj ? dx : dy, m = xmaj ? dy : dx;
    int64_t acc = 0, t = 0;
    bool bad = false;
    for (int k = threadIdx.x; k < n && !bad; k += 64) {
        const int64_t km = (int64_t)k * m, steps = km / n;
        int64_t f = km - steps * n + m;
        if (xmaj) {
            const int cx = x0 + k * sx;
            int cy = y0 + (int)steps * sy;
            if (f >= dx) { if (rf_los_cell(a, cx + ux, cy + uy, t)) acc += t; else bad = true; cy += sy; f -= dx; }
            if (!bad && f != 0) { if (rf_los_cell(a, cx + ux, cy + uy, t)) acc += t; else bad = true; }
            if (!bad && dy == 0) {
                if (rf_los_cell(a, cx + ux, cy, t)) acc += t;
                else if (rf_los_cell(a, cx + ux, cy - 1, t)) acc += t;
                else bad = true;
            }
        } else {
            const int cy = y0 + k * sy;
            int cx = x0 + (int)steps * sx;
            if (f >= dy) { if (rf_los_cell(a, cx + ux, cy + uy, t)) acc += t; else bad = true; cx += sx; f -= dy; }
            if (!bad && f != 0) { if (rf_los_cell(a, cx + ux, cy + uy, t)) acc += t; else bad = true; }
            if (!bad && dx == 0) {
                if (rf_los_cell(a, cx, cy + uy, t)) acc += t;
                else if (rf_los_cell(a, cx - 1, cy + uy, t)) acc += t;
                else bad = true;
            }
        }
    }
    const bool blocked = __any(bad);
    sum = wave_sum(acc);
    return !blocked;
}

__device__ __forceinline__ double rf_euc(double w, int ax, int ay, int bx, int by)
{
    const int64_t dx = ax - bx, dy = ay - by;
    return w * sqrt((double)(dx * dx + dy * dy));
}

__global__ __launch_bounds__(64) void rf_legs_kernel(FsRefineLegArgs a)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    const int32_t *in = a.leg_in + 4 * (int64_t)b;
    const int32_t out = in[3];
    const int32_t src = in[0], goal = in[1];
    const int nx = a.nx;
    const int64_t ns = (int64_t)nx * a.ny;
    const double *G = a.g + (int64_t)in[2] * ns;
    int32_t *chain = a.chain + (int64_t)out * a.chain_cap;
    int32_t *par = a.par + (int64_t)out * a.chain_cap;
    int32_t *vtx = a.vtx + (int64_t)out * a.chain_cap;
    int status = FS_REFINE_NO_PATH;
    double cost = kInf;
    int64_t L = 0, walks = 0;
    int32_t nv = 0, np = 0;
    const int cs = a.cells[src], cg = a.cells[goal];
    if (!rf_safe(cs, a.allow)) status = FS_REFINE_START_UNSAFE;
    else if (!rf_safe(cg, a.allow)) status = FS_REFINE_GOAL_UNSAFE;
    else if (G[goal] < kInf) {
        // the descent, goal first: chain[0] = goal ... chain[P] = start
        int64_t v = goal;
        L = 1;
        if (lane == 0) chain[0] = (int32_t)v;
        bool broken = false;
        while (v != src) {
            const int x = (int)(v % nx), y = (int)(v / nx);
            const double gv = G[v], tv = rf_trav(a.cells[v], a.w_trav);
            bool eq = false;
            if (lane < a.corners) {
                const int ux = x + kMx[lane], uy = y + kMy[lane];
                if (ux >= 0 && uy >= 0 && ux < nx && uy < a.ny) {
                    const double gu = G[(int64_t)uy * nx + ux];
                    eq = gu < kInf && (gu + a.e[lane]) + tv == gv;
                }
            }
            const unsigned long long mask = __ballot(eq);
            if (!mask || L > ns) { broken = true; break; }
            const int mv = __ffsll((long long)mask) - 1;
            v = (int64_t)(y + kMy[mv]) * nx + (x + kMx[mv]);
            if (lane == 0 && L < a.chain_cap) chain[L] = (int32_t)v;
            ++L;
        }
        if (broken) status = FS_REFINE_BROKEN;
        else if (L > a.chain_cap) status = FS_REFINE_OVERFLOW;
        else {
            __syncthreads();
            const int64_t P = L - 1;
            // the chain: G(c0) = trav(start), parent(c0) = c0; resetParent against the parent's parent at every step
            double Gprev = rf_trav(cs, a.w_trav), Gpp = Gprev;
            int64_t pprev = 0;
            if (lane == 0) par[0] = 0;
            for (int64_t i = 1; i <= P; ++i) {
                const int32_t c = chain[P - i], cp = chain[P - i + 1], an = chain[P - pprev];
                const int cx = c % nx, cy = c / nx, px = cp % nx, py = cp / nx, ax = an % nx, ay = an / nx;
                double Gi = (Gprev + rf_euc(a.w_euc, px, py, cx, cy)) + rf_trav(a.cells[c], a.w_trav);
                int64_t p = i - 1;
                double Gp = Gprev;
                int64_t sum = 0;
                ++walks;
                if (rf_los(a, cx, cy, ax, ay, sum)) {
                    const double los = a.w_trav * (double)sum / 645160000.0;
                    const double g2 = (Gpp + rf_euc(a.w_euc, cx, cy, ax, ay)) + los;
                    if (g2 < Gi) { Gi = g2; p = pprev; Gp = Gpp; }
                }
                if (lane == 0) par[i] = (int32_t)p;
                Gprev = Gi; pprev = p; Gpp = Gp;
            }
            cost = Gprev;
            __syncthreads();
            // the vertices: the parent chain from the goal, written start first
            for (int64_t i = P; i != 0; i = par[i]) ++nv;
            ++nv;
            if (lane == 0) {
                int32_t k = nv - 1;
                for (int64_t i = P; i != 0; i = par[i]) vtx[k--] = chain[P - i];
                vtx[0] = chain[P];
            }
            __syncthreads();
            // backtrace (the goal twice) + linearInterpolation at the costmap resolution
            double *vo = a.vert + 2 * (int64_t)out * a.vert_cap;
            double *po = a.pose + 2 * (int64_t)out * a.pose_cap;
            for (int32_t k = lane; k < nv && k < a.vert_cap; k += 64) {
                const int32_t c = vtx[k];
                vo[2 * k] = a.ox + ((double)(uint32_t)(c % nx) + 0.5) * a.res;
                vo[2 * k + 1] = a.oy + ((double)(uint32_t)(c / nx) + 0.5) * a.res;
            }
            int64_t off = 0;
            for (int32_t j = 0; j < nv; ++j) {
                const int32_t c1 = vtx[j], c2 = vtx[j + 1 < nv ? j + 1 : nv - 1];
                const double x1 = a.ox + ((double)(uint32_t)(c1 % nx) + 0.5) * a.res, y1 = a.oy + ((double)(uint32_t)(c1 / nx) + 0.5) * a.res;
                const double x2 = a.ox + ((double)(uint32_t)(c2 % nx) + 0.5) * a.res, y2 = a.oy + ((double)(uint32_t)(c2 / nx) + 0.5) * a.res;
                const double ex = x2 - x1, ey = y2 - y1;
                const double dist = sqrt(ex * ex + ey * ey);
                const int loops = (int)(dist / a.res);
                const double sa = ey / dist, ca = ex / dist;
                const int cnt = loops > 1 ? loops : 1;
                for (int k = lane; k < cnt; k += 64) {
                    const int64_t o = off + k;
                    if (o >= a.pose_cap) break;
                    po[2 * o] = k == 0 ? x1 : x1 + k * a.res * ca;
                    po[2 * o + 1] = k == 0 ? y1 : y1 + k * a.res * sa;
                }
                off += cnt;
            }
            np = (int32_t)(off < INT32_MAX ? off : INT32_MAX);
            status = (nv > a.vert_cap || np > a.pose_cap) ? FS_REFINE_OVERFLOW : FS_REFINE_OK;
        }
    }
    if (lane == 0) {
        a.status[out] = status;
        a.cost[out] = status == FS_REFINE_OK || status == FS_REFINE_OVERFLOW ? cost : kInf;
        a.n_vertices[out] = nv;
        a.n_poses[out] = np;
        a.chain_len[out] = L;
        a.walks[out] = walks;
    }
}

// ---------------------------------------------------------------- the REFERENCE search, one wave each

__device__ __forceinline__ fs_theta_mem rs_slot(const FsRefineSearchArgs &a, int32_t slot)
{
    const int64_t ns = (int64_t)a.nx * a.ny;
    char *p = a.slab + (int64_t)slot * a.slot_bytes;
    fs_theta_mem m;
    m.at = reinterpret_cast<int32_t *>(p); p += fs_rs_up8(4 * ns);
    m.heap = reinterpret_cast<int32_t *>(p); p += fs_rs_up8(4 * (ns + 1));
    m.cell = reinterpret_cast<int32_t *>(p); p += fs_rs_up8(4 * ns);
    m.g = reinterpret_cast<double *>(p); p += 8 * ns;
    m.h = reinterpret_cast<double *>(p); p += 8 * ns;
    m.f = reinterpret_cast<double *>(p); p += 8 * ns;
    m.parent = reinterpret_cast<int32_t *>(p); p += fs_rs_up8(4 * ns);
    m.queued = reinterpret_cast<uint8_t *>(p);
    return m;
}

// blockIdx.y = slot: no cell has a record
__global__ void rs_fill_kernel(FsRefineSearchArgs a)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, ns = (int64_t)a.nx * a.ny;
    if (k < ns) rs_slot(a, (int32_t)blockIdx.y).at[k] = -1;
}

__global__ __launch_bounds__(64) void rs_search_kernel(FsRefineSearchArgs a, int32_t base)
{
    __shared__ double s_term[128];
    __shared__ int s_cnt[64];
    const int lane = threadIdx.x;
    const int64_t k = (int64_t)base + blockIdx.x;
    const fs_theta_mem m = rs_slot(a, (int32_t)blockIdx.x);
    const fs_theta_map M{a.cells, a.nx, a.ny, a.allow, a.corners, a.w_euc, a.w_trav, a.w_euc < 1.0 ? a.w_euc : 1.0, a.hyp};
    const int32_t src = a.search_in[2 * k], goal = a.search_in[2 * k + 1];
    int status = FS_REFINE_NO_PATH;
    double cost = kInf;
    int32_t nv = 0;
    fs_theta_state S{};
    if (!fs_theta_safe(a.cells[src], a.allow)) status = FS_REFINE_START_UNSAFE;
    else if (!fs_theta_safe(a.cells[goal], a.allow)) status = FS_REFINE_GOAL_UNSAFE;
    else {
        fs_theta_begin(M, m, S, src % a.nx, src / a.nx, goal % a.nx, goal / a.nx);
        bool found = false;
        while (S.hsize > 0) {
            if (fs_theta_is_goal(M, m, S)) { found = true; break; }
            int x0, y0, x1, y1;
            const int32_t gp = fs_theta_reset_cells(M, m, S, x0, y0, x1, y1);
            // losCheck: 64 iterations at a time, each lane's terms and verdict, then the terms added in walk order
            const int n = fs_theta_walk_len(x0, y0, x1, y1);
            bool ok = true;
            double los = 0;
            for (int k0 = 0; k0 < n; k0 += 64) {
                double t[2] = {0.0, 0.0};
                const int cnt = k0 + lane < n ? fs_theta_walk_iter(M, x0, y0, x1, y1, k0 + lane, t) : 0;
                if (__any(cnt < 0)) { ok = false; break; }
                s_term[2 * lane] = t[0]; s_term[2 * lane + 1] = t[1]; s_cnt[lane] = cnt;
                __syncthreads();
                const int act = n - k0 < 64 ? n - k0 : 64;
                for (int l = 0; l < act; ++l) {
                    const int c = s_cnt[l];
                    if (c > 0) los += s_term[2 * l];
                    if (c > 1) los += s_term[2 * l + 1];
                }
                __syncthreads();
            }
            fs_theta_reset_parent(M, m, S, gp, ok, los, x0, y0, x1, y1);
            // setNeighbors: evaluated across lanes, committed in moves[] order
            const double g = m.g[S.cur];
            int32_t cell = 0;
            double gc = 0, hc = 0, fc = 0;
            const bool valid = lane < a.corners && fs_theta_neighbor(M, S, x0, y0, g, lane, cell, gc, hc, fc);
            const unsigned long long mask = __ballot(valid);
            for (int i = 0; i < a.corners; ++i) {
                if (!((mask >> i) & 1ull)) continue;
                fs_theta_commit(m, S, __shfl(cell, i, 64), __shfl(gc, i, 64), __shfl(hc, i, 64), __shfl(fc, i, 64));
            }
            fs_theta_next(m, S);
        }
        if (found) {
            status = FS_REFINE_OK;
            cost = m.g[S.cur];
            nv = fs_theta_backtrace(m, S.cur, a.vtx + k * a.vtx_cap, a.vtx_cap);
        }
    }
    if (lane == 0) {
        a.status[k] = status;
        a.cost[k] = cost;
        a.n_vertices[k] = nv;
        a.max_heap[k] = S.max_heap;
        a.pops[k] = S.pops;
        a.walks[k] = S.walks;
    }
}

}  // namespace

hipError_t fs_launch_refine_init(const FsRefineFieldArgs &a, uint32_t *d_flags_prev, hipStream_t s)
{
    const int64_t ns = (int64_t)a.nx * a.ny, tiles = (int64_t)a.tx * a.ty, m = ns > tiles ? ns : tiles;
    hipLaunchKernelGGL(rf_init_kernel, dim3((unsigned)((m + 255) / 256), (unsigned)a.n), dim3(256), 0, s, a, d_flags_prev);
    return hipGetLastError();
}

hipError_t fs_launch_refine_round(const FsRefineFieldArgs &a, const uint32_t *d_prev, uint32_t *d_cur, int32_t *d_any, hipStream_t s)
{
    hipLaunchKernelGGL(rf_round_kernel, dim3((unsigned)(a.tx * a.ty), (unsigned)a.n), dim3(RF_THREADS), 0, s, a, d_prev, d_cur, d_any);
    return hipGetLastError();
}

hipError_t fs_launch_refine_legs(const FsRefineLegArgs &a, int32_t n_blocks, hipStream_t s)
{
    if (n_blocks <= 0) return hipSuccess;
    hipLaunchKernelGGL(rf_legs_kernel, dim3((unsigned)n_blocks), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t fs_launch_refine_search_batch(const FsRefineSearchArgs &a, int32_t base, int32_t count, hipStream_t s)
{
    if (count <= 0) return hipSuccess;
    const int64_t ns = (int64_t)a.nx * a.ny;
    hipLaunchKernelGGL(rs_fill_kernel, dim3((unsigned)((ns + 255) / 256), (unsigned)count), dim3(256), 0, s, a);
    hipLaunchKernelGGL(rs_search_kernel, dim3((unsigned)count), dim3(64), 0, s, a, base);
    return hipGetLastError();
}
