// fs_thetastar.h — the reference's Theta* search (ThetaStar::generatePath, DEP/src/planners/theta_star.cpp) as it runs, for the
// REFERENCE refine search (fs_set_refine_search).  The device (fs_refine.hip) and a CPU driver
// (tests/thetastar_search_ref/) compile this same source, as they do fs_navfn_wave.h and fs_roadmap_astar.h.
//
// Node store.  One record per touched cell: cell (x, y), g, h, f, parent record, queued.  at[cell] is node_position_: the cell's
// record, -1 while it has none.  A fresh record has f = g = h = DBL_MAX.
//
// Open list.  std::priority_queue<tree_node *, vector, comp> with comp(a, b) = a->f > b->f, held here as a binary heap of RECORD IDS
// whose comparisons read f THROUGH the id at the moment they are made: the reference rewrites f, g and the parent of a queued node
// in place and never re-sifts, so the array is usually not a valid heap and which entry surfaces is decided by the exact comparison
// sequence of libstdc++'s __push_heap and __adjust_heap, restated here step for step (fs_roadmap_astar.h does the same for a heap
// that holds its keys; this one must not).
//
// The loop, as the reference writes it: the start record is pushed AND taken as the first current node, so it is expanded before it
// is ever popped and can sit in the heap twice (heap entries <= cells + 1); while the heap is non-empty: isGoal(current),
// resetParent(current), setNeighbors(current), current = top, pop.  The entry popped last is therefore never examined: no path.
//   resetParent   queued = false; losCheck from the node to its parent's parent; when it holds and (g(grandparent) + w_euc *
//                 hypot) + los < g, the node takes the grandparent, that g, and f = g + h.
//   losCheck      the Bresenham walk below; every cell it visits passes the three-argument isSafe — c = 26 + 0.9 raw below 254, or
//                 an unknown cell with allow_unknown, which counts as c = 253 — and adds w c c / 254 / 254 to an fp64 sum, in walk
//                 order (a left fold: the device gathers a walk's terms across lanes and adds them in this order).  The dy == 0 and
//                 dx == 0 clauses try a second cell only when the first is refused.  A cell off the map is unsafe here (the
//                 reference reads outside its array for a straight walk along row or column 0).
//   setNeighbors  the first `corners` of moves[] in order; a neighbour on the map that passes the two-argument isSafe (raw < 254, or
//                 unknown with allow_unknown) gets g' = (g + w_euc * hypot(step)) + trav(neighbour) (an unknown neighbour costs
//                 c = 255.5), h' = w_h * hypot(to the goal), f' = g' + h'; its record is created if it has none; when f > f'
//                 (strictly) it takes g', h', f' and the current node as parent, and if it is not queued its x, y are written and
//                 it is pushed.
//
// hypot.  The reference calls std::hypot, which is not the correctly rounded sqrt(x^2 + y^2) (glibc 2.35 differs on 52 418 integer
// pairs below 4096, first at (27, 17)), and a device hypot cannot be held to the host's libm.  Every hypot of the search takes two
// integer cell differences bounded by the grid, so the search reads them from a table hyp[|dx| * ny + |dy|] = std::hypot(dx, dy)
// that the host fills with the libm it runs on (fs_theta_fill_table; hypot is even and symmetric, C Annex F).  linearInterpolation's
// hypot takes world differences: fs_theta_interpolate is host code.  All of it is compiled with -ffp-contract=off.
#pragma once

#include <float.h>
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FS_THETA_HD __host__ __device__
#else
#define FS_THETA_HD
#endif

enum { FS_THETA_FOUND = 0, FS_THETA_NO_PATH = 5 };
#define FS_THETA_MAX_SIDE 4096

// the costmap, the planner's parameters and the hypot table
struct fs_theta_map {
    const uint8_t *cells;      // [ny][nx] raw costmap bytes
    int32_t nx, ny;
    int32_t allow, corners;
    double w_euc, w_trav, w_h; // w_h = min(w_euc, 1): the heuristic's weight
    const double *hyp;         // [nx][ny]: hyp[|dx| * ny + |dy|] = std::hypot(dx, dy)
};

// One search's storage (ns = nx * ny): 41 B per cell and the heap's one entry more.
struct fs_theta_mem {
    int32_t *at;               // [ns] cell -> record, -1: none (cleared before every search)
    int32_t *heap;             // [ns + 1] record ids
    int32_t *cell;             // [ns] records: y * nx + x, written when the record is pushed
    double *g, *h, *f;         // [ns]
    int32_t *parent;           // [ns] record id
    uint8_t *queued;           // [ns]
};

struct fs_theta_state {
    int32_t nrec, hsize, cur;
    int32_t gx, gy;
    int64_t pops, walks;
    int32_t max_heap;
};

FS_THETA_HD inline int fs_theta_move_x(int i) { return i == 2 || i == 4 || i == 6 ? 1 : (i == 3 || i == 5 || i == 7 ? -1 : 0); }
FS_THETA_HD inline int fs_theta_move_y(int i) { return i == 0 || i == 5 || i == 6 ? 1 : (i == 1 || i == 4 || i == 7 ? -1 : 0); }

FS_THETA_HD inline double fs_theta_hypot(const fs_theta_map &M, int dx, int dy)
{
    return M.hyp[(int64_t)(dx < 0 ? -dx : dx) * M.ny + (dy < 0 ? -dy : dy)];
}
// the two-argument isSafe
FS_THETA_HD inline bool fs_theta_safe(int v, int allow) { return (v == 255 && allow) || v < 254; }
// getTraversalCost: w * c * c / 254 / 254, c = getCost = 26 + 0.9 * raw
FS_THETA_HD inline double fs_theta_trav(int v, double w) { const double c = 26 + 0.9 * (double)v; return w * c * c / 254 / 254; }
// the three-argument isSafe on one cell of a walk: false if refused (or off the map), else its term
FS_THETA_HD inline bool fs_theta_walk_cell(const fs_theta_map &M, int x, int y, double &term)
{
    if (x < 0 || y < 0 || x >= M.nx || y >= M.ny) return false;
    const int v = M.cells[(int64_t)y * M.nx + x];
    double c = 26 + 0.9 * (double)v;
    if (!((v == 255 && M.allow) || c < 254)) return false;
    if (v == 255) c = 254 - 1;
    term = M.w_trav * c * c / 254 / 254;
    return true;
}

// Iteration k of losCheck's loop from (x0, y0) to (x1, y1) (max(|dx|, |dy|) iterations): before it the major coordinate has moved k
// steps, the minor one floor(k m / n), and the error term is k m mod n.  Returns how many terms it adds, t[0] then t[1] (a straight
// walk adds one per iteration, any other at most two), or -1 when it refuses a cell: no line of sight.
FS_THETA_HD inline int fs_theta_walk_iter(const fs_theta_map &M, int x0, int y0, int x1, int y1, int k, double t[2])
{
    const int dx = x1 > x0 ? x1 - x0 : x0 - x1, dy = y1 > y0 ? y1 - y0 : y0 - y1;
    const int sx = x1 > x0 ? 1 : -1, sy = y1 > y0 ? 1 : -1;
    const int ux = (sx - 1) / 2, uy = (sy - 1) / 2;
    const bool xmaj = dx >= dy;
    const int n = xmaj ? dx : dy, m = xmaj ? dy : dx;
    const int64_t km = (int64_t)k * m, steps = km / n;
    int64_t f = km - steps * n + m;
    int cnt = 0;
    if (xmaj) {
        const int cx = x0 + k * sx;
        int cy = y0 + (int)steps * sy;
        if (f >= dx) { if (!fs_theta_walk_cell(M, cx + ux, cy + uy, t[cnt])) return -1; ++cnt; cy += sy; f -= dx; }
        if (f != 0) { if (!fs_theta_walk_cell(M, cx + ux, cy + uy, t[cnt])) return -1; ++cnt; }
        if (dy == 0) { if (!fs_theta_walk_cell(M, cx + ux, cy, t[cnt]) && !fs_theta_walk_cell(M, cx + ux, cy - 1, t[cnt])) return -1; ++cnt; }
    } else {
        const int cy = y0 + k * sy;
        int cx = x0 + (int)steps * sx;
        if (f >= dy) { if (!fs_theta_walk_cell(M, cx + ux, cy + uy, t[cnt])) return -1; ++cnt; cx += sx; f -= dy; }
        if (f != 0) { if (!fs_theta_walk_cell(M, cx + ux, cy + uy, t[cnt])) return -1; ++cnt; }
        if (dx == 0) { if (!fs_theta_walk_cell(M, cx, cy + uy, t[cnt]) && !fs_theta_walk_cell(M, cx - 1, cy + uy, t[cnt])) return -1; ++cnt; }
    }
    return cnt;
}
FS_THETA_HD inline int fs_theta_walk_len(int x0, int y0, int x1, int y1)
{
    const int dx = x1 > x0 ? x1 - x0 : x0 - x1, dy = y1 > y0 ? y1 - y0 : y0 - y1;
    return dx >= dy ? dx : dy;
}

// losCheck, one iteration after the other (the host form): the fp64 left fold of the terms in walk order
FS_THETA_HD inline bool fs_theta_los(const fs_theta_map &M, int x0, int y0, int x1, int y1, double &sum)
{
    sum = 0;
    const int n = fs_theta_walk_len(x0, y0, x1, y1);
    double t[2];
    for (int k = 0; k < n; ++k) {
        const int cnt = fs_theta_walk_iter(M, x0, y0, x1, y1, k, t);
        if (cnt < 0) return false;
        if (cnt > 0) sum += t[0];
        if (cnt > 1) sum += t[1];
    }
    return true;
}

// ---- the open list: comp(a, b) = f[a] > f[b], read through the ids at every comparison

// std::__push_heap(first, hole, top = 0, value) with comp(parent, value)
FS_THETA_HD inline void fs_theta_sift_up(int32_t *heap, const double *f, int32_t hole, int32_t r)
{
    int32_t parent = (hole - 1) / 2;
    while (hole > 0 && f[heap[parent]] > f[r]) {
        heap[hole] = heap[parent];
        hole = parent;
        parent = (hole - 1) / 2;
    }
    heap[hole] = r;
}

// priority_queue::push: push_back, then std::push_heap
FS_THETA_HD inline void fs_theta_push(int32_t *heap, const double *f, int32_t &size, int32_t r)
{
    fs_theta_sift_up(heap, f, size, r);
    ++size;
}

// top() and pop(): std::pop_heap (the last entry sifted from the root by __adjust_heap over size - 1 entries, then __push_heap), then
// pop_back.  Returns the top's record.
FS_THETA_HD inline int32_t fs_theta_pop(int32_t *heap, const double *f, int32_t &size)
{
    const int32_t top = heap[0];
    if (size > 1) {
        const int32_t len = size - 1, v = heap[len];
        int32_t hole = 0, child = 0;
        while (child < (len - 1) / 2) {
            child = 2 * (child + 1);
            if (f[heap[child]] > f[heap[child - 1]]) child--;
            heap[hole] = heap[child];
            hole = child;
        }
        if ((len & 1) == 0 && child == (len - 2) / 2) {
            child = 2 * (child + 1);
            heap[hole] = heap[child - 1];
            hole = child - 1;
        }
        fs_theta_sift_up(heap, f, hole, v);
    }
    --size;
    return top;
}

// ---- the search's steps

// a record for `cell` (at[cell] must be -1): f = g = h = DBL_MAX, not queued
FS_THETA_HD inline int32_t fs_theta_new_record(const fs_theta_mem &m, fs_theta_state &S, int32_t cell)
{
    const int32_t r = S.nrec++;
    m.g[r] = DBL_MAX; m.h[r] = DBL_MAX; m.f[r] = DBL_MAX;
    m.parent[r] = -1; m.queued[r] = 0; m.cell[r] = cell;
    m.at[cell] = r;
    return r;
}

// the start record: pushed, and the first current node
FS_THETA_HD inline void fs_theta_begin(const fs_theta_map &M, const fs_theta_mem &m, fs_theta_state &S, int sx, int sy, int gx, int gy)
{
    S.nrec = 0; S.hsize = 0; S.gx = gx; S.gy = gy; S.pops = 0; S.walks = 0;
    const int32_t cell = sy * M.nx + sx;
    const int32_t s = fs_theta_new_record(m, S, cell);
    m.g[s] = fs_theta_trav(M.cells[cell], M.w_trav);
    m.h[s] = M.w_h * fs_theta_hypot(M, sx - gx, sy - gy);
    m.parent[s] = s;
    m.queued[s] = 1;
    m.f[s] = m.g[s] + m.h[s];
    fs_theta_push(m.heap, m.f, S.hsize, s);
    S.max_heap = S.hsize;
    S.cur = s;
}

FS_THETA_HD inline bool fs_theta_is_goal(const fs_theta_map &M, const fs_theta_mem &m, const fs_theta_state &S)
{
    return m.cell[S.cur] == S.gy * M.nx + S.gx;
}

// resetParent's walk runs from the current node to its grandparent: the two cells (returns the grandparent's record)
FS_THETA_HD inline int32_t fs_theta_reset_cells(const fs_theta_map &M, const fs_theta_mem &m, const fs_theta_state &S, int &x0, int &y0, int &x1, int &y1)
{
    const int32_t gp = m.parent[m.parent[S.cur]];
    const int32_t c = m.cell[S.cur], a = m.cell[gp];
    x0 = c % M.nx; y0 = c / M.nx; x1 = a % M.nx; y1 = a / M.nx;
    return gp;
}

// resetParent once the walk's verdict and sum are known
FS_THETA_HD inline void fs_theta_reset_parent(const fs_theta_map &M, const fs_theta_mem &m, fs_theta_state &S, int32_t gp, bool los_ok, double los,
                                              int x0, int y0, int x1, int y1)
{
    const int32_t cur = S.cur;
    m.queued[cur] = 0;
    ++S.walks;
    if (!los_ok) return;
    const double gc = (m.g[gp] + M.w_euc * fs_theta_hypot(M, x0 - x1, y0 - y1)) + los;
    if (gc < m.g[cur]) { m.parent[cur] = gp; m.g[cur] = gc; m.f[cur] = gc + m.h[cur]; }
}

// neighbour i of the cell (x, y) whose record holds g: false when it is off the map or unsafe, else its cell and g', h', f'
FS_THETA_HD inline bool fs_theta_neighbor(const fs_theta_map &M, const fs_theta_state &S, int x, int y, double g, int i, int32_t &cell, double &gc,
                                          double &hc, double &fc)
{
    const int mx = x + fs_theta_move_x(i), my = y + fs_theta_move_y(i);
    if (mx < 0 || my < 0 || mx >= M.nx || my >= M.ny) return false;
    cell = my * M.nx + mx;
    const int v = M.cells[cell];
    if (!fs_theta_safe(v, M.allow)) return false;
    gc = (g + M.w_euc * fs_theta_hypot(M, x - mx, y - my)) + fs_theta_trav(v, M.w_trav);
    hc = M.w_h * fs_theta_hypot(M, mx - S.gx, my - S.gy);
    fc = gc + hc;
    return true;
}

// setNeighbors' body for one evaluated neighbour
FS_THETA_HD inline void fs_theta_commit(const fs_theta_mem &m, fs_theta_state &S, int32_t cell, double gc, double hc, double fc)
{
    int32_t r = m.at[cell];
    if (r < 0) r = fs_theta_new_record(m, S, cell);
    if (m.f[r] > fc) {
        m.g[r] = gc; m.h[r] = hc; m.f[r] = fc; m.parent[r] = S.cur;
        if (!m.queued[r]) {
            m.cell[r] = cell;
            m.queued[r] = 1;
            fs_theta_push(m.heap, m.f, S.hsize, r);
            if (S.hsize > S.max_heap) S.max_heap = S.hsize;
        }
    }
}

// current = top, pop
FS_THETA_HD inline void fs_theta_next(const fs_theta_mem &m, fs_theta_state &S)
{
    S.cur = fs_theta_pop(m.heap, m.f, S.hsize);
    ++S.pops;
}

// backtrace: the parent chain from record r, written start first into out (up to cap cells); returns the chain's length
FS_THETA_HD inline int32_t fs_theta_backtrace(const fs_theta_mem &m, int32_t r, int32_t *out, int32_t cap)
{
    int32_t n = 1;
    for (int32_t p = r; m.parent[p] != p; p = m.parent[p]) ++n;
    int32_t k = n - 1;
    for (int32_t p = r;; p = m.parent[p], --k) {
        if (k < cap) out[k] = m.cell[p];
        if (m.parent[p] == p) break;
    }
    return n;
}

// The whole search, one step after the other (the host form; the device splits a walk's iterations and a node's neighbours over a
// wave and commits them in this order).  at[] = -1 on entry; start and goal on the map and safe.  FS_THETA_FOUND with S.cur the
// goal's record, or FS_THETA_NO_PATH.
FS_THETA_HD inline int fs_theta_run(const fs_theta_map &M, const fs_theta_mem &m, fs_theta_state &S, int sx, int sy, int gx, int gy)
{
    fs_theta_begin(M, m, S, sx, sy, gx, gy);
    while (S.hsize > 0) {
        if (fs_theta_is_goal(M, m, S)) return FS_THETA_FOUND;
        int x0, y0, x1, y1;
        const int32_t gp = fs_theta_reset_cells(M, m, S, x0, y0, x1, y1);
        double los = 0;
        const bool ok = fs_theta_los(M, x0, y0, x1, y1, los);
        fs_theta_reset_parent(M, m, S, gp, ok, los, x0, y0, x1, y1);
        const double g = m.g[S.cur];
        for (int i = 0; i < M.corners; ++i) {
            int32_t cell;
            double gc, hc, fc;
            if (fs_theta_neighbor(M, S, x0, y0, g, i, cell, gc, hc, fc)) fs_theta_commit(m, S, cell, gc, hc, fc);
        }
        fs_theta_next(m, S);
    }
    return FS_THETA_NO_PATH;
}

// ---------------------------------------------------------------- host only: the table and the published poses
#include <cmath>
#include <vector>

// hyp[dx * ny + dy] = std::hypot(dx, dy) of the libm this process runs on, 0 <= dx < nx, 0 <= dy < ny
inline void fs_theta_fill_table(double *hyp, int32_t nx, int32_t ny)
{
    for (int32_t dx = 0; dx < nx; ++dx)
        for (int32_t dy = 0; dy < ny; ++dy) hyp[(size_t)dx * ny + dy] = std::hypot((double)dx, (double)dy);
}

// costmap mapToWorld
inline double fs_theta_map_to_world(double o, double res, int32_t m) { return o + ((unsigned)m + 0.5) * res; }

// ThetaStar::backtrace's list (the vertices, the goal twice) through linearInterpolation at distance `res`: every segment's first
// point and the points k * res along it, k < (int)(length / res); appended to px, py
inline void fs_theta_interpolate(const double *vx, const double *vy, size_t nv, double res, std::vector<double> &px, std::vector<double> &py)
{
    for (size_t j = 0; j < nv; ++j) {
        const size_t j2 = j + 1 < nv ? j + 1 : nv - 1;
        const double x1 = vx[j], y1 = vy[j], x2 = vx[j2], y2 = vy[j2];
        px.push_back(x1); py.push_back(y1);
        const double ex = x2 - x1, ey = y2 - y1;
        const double dist = std::hypot(ex, ey);
        const int loops = (int)(dist / res);
        const double sa = ey / dist, ca = ex / dist;
        for (int k = 1; k < loops; ++k) {
            px.push_back(x1 + k * res * ca);
            py.push_back(y1 + k * res * sa);
        }
    }
}
