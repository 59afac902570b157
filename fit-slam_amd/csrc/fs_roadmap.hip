// fs_roadmap.hip — the frontier roadmap's device work: edge construction of reConstructGraph(entireGraph = true)
// as one batch of segment walks, and the roadmap planner of setPlanForFrontierRoadmap as ONE shortest-path tree per tick plus a
// lane per frontier.
//
// Reference: DEP/src/planners/FrontierRoadmap.cpp — reConstructGraph (:347-408), getNodesWithinRadius (:410-436),
// getClosestNodeInRoadMap (:506-543), getPlan (:545-631), isConnectable (:716-737); DEP/src/planners/astar.cpp:42-93;
// DEP/src/CostCalculator.cpp:395-438.
//
// Edges.  Node p's candidates are the nodes q != p of the hash cells within ceil(radius / cell) of p's cell, dx outer, dy inner,
// insertion order inside a cell, with distance(p, q) < radius; each is walked q -> p (isConnectable(closestNode, point)) by the
// segment kernel behind fs_trace_segments, and p's list is its accepted candidates in that order.  Lists are independent, so the
// CSR is a pure function of the node list and the grid.
//
// Tree.  key(v) = (d, hops, predecessor), lexicographic; key(root) = (0, 0, -1); otherwise the minimum over in-edges u -> v with
// d(u) finite of (d(u) + w(u, v), hops(u) + 1, u), w the squared segment length (sqDistanceBetweenFrontiers).  Rounds are Jacobi
// steps (read buffer A, write buffer B) from (inf, INT32_MAX, -1) until a round changes nothing.  Floating-point addition is
// monotone, so d converges to the minimum over paths of the left-to-right sums whatever the schedule, and hops / predecessor to the
// shortest tight in-edge chain / its least index (DESIGN.md 4.10 states when that is unique); no atomic decides a predecessor.
#include "fs_internal.h"

#include <float.h>

namespace {

constexpr int kScanThreads = 1024;

__device__ __forceinline__ int32_t find_cell(const FsRoadmapDev &g, int cx, int cy)
{
    const uint64_t k = ((uint64_t)(uint32_t)cx << 32) | (uint32_t)cy;
    int32_t lo = 0, hi = g.n_cells;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (g.cell_key[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    return (lo < g.n_cells && g.cell_key[lo] == k) ? lo : -1;
}

// getNodesWithinRadius(p, radius) without p itself: counted (d_off == nullptr) or written from d_off[p] on
__global__ void rm_candidates_kernel(const FsRoadmapDev g, const int32_t *__restrict__ off, int32_t *__restrict__ count, double oz,
                                     double *__restrict__ start, double *__restrict__ end, int32_t *__restrict__ cand)
{
    const int32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= g.n) return;
    const double px = g.xy[2 * p], py = g.xy[2 * p + 1];
    const int cx = fs_rm_cell(px, g.cell), cy = fs_rm_cell(py, g.cell);
    const int cr = (int)ceil(g.radius / g.cell);
    int32_t k = off ? off[p] : 0;
    for (int dx = -cr; dx <= cr; ++dx)
        for (int dy = -cr; dy <= cr; ++dy) {
            const int32_t c = find_cell(g, cx + dx, cy + dy);
            if (c < 0) continue;
            for (int32_t j = g.cell_start[c]; j < g.cell_start[c + 1]; ++j) {
                const int32_t q = g.cell_nodes[j];
                const double qx = g.xy[2 * q], qy = g.xy[2 * q + 1];
                const double ex = px - qx, ey = py - qy;
                if (!(sqrt(ex * ex + ey * ey) < g.radius) || q == p) continue;
                if (off) {
                    start[3 * k] = qx; start[3 * k + 1] = qy; start[3 * k + 2] = oz;
                    end[3 * k] = px; end[3 * k + 1] = py; end[3 * k + 2] = oz;
                    cand[k] = q;
                }
                ++k;
            }
        }
    if (!off) count[p] = k;
}

// isConnectable's verdict on the walk of candidate i
__device__ __forceinline__ bool accepted(const uint8_t *ok, const uint8_t *hit, const int32_t *unknown, double limit, int32_t i)
{
    return ok[i] && !hit[i] && !((double)unknown[i] > limit);
}

// One wave per node, lanes over its candidates 64 at a time: the accepted ones counted (d_row == nullptr) or compacted in order
__global__ __launch_bounds__(256) void rm_edges_kernel(int32_t n, const int32_t *__restrict__ cand_off, const int32_t *__restrict__ cand,
                                                       const uint8_t *__restrict__ ok, const uint8_t *__restrict__ hit,
                                                       const int32_t *__restrict__ unknown, double limit, const int32_t *__restrict__ row,
                                                       int32_t *__restrict__ count, int32_t *__restrict__ col)
{
    const int32_t p = (int32_t)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const int lane = threadIdx.x & 63;
    if (p >= n) return;
    const int32_t b = cand_off[p], e = cand_off[p + 1];
    int32_t k = row ? row[p] : 0;
    for (int32_t i0 = b; i0 < e; i0 += 64) {
        const int32_t i = i0 + lane;
        const bool acc = i < e && accepted(ok, hit, unknown, limit, i);
        const uint64_t m = __ballot(acc);
        if (row && acc) col[k + __popcll(m & ((1ull << lane) - 1ull))] = cand[i];
        k += __popcll(m);
    }
    if (!row && lane == 0) count[p] = k;
}

// exclusive scan by one workgroup: every thread sums a contiguous chunk, the chunk sums are scanned in LDS
__global__ __launch_bounds__(kScanThreads) void rm_scan_kernel(const int32_t *__restrict__ in, int32_t n, int32_t *__restrict__ out)
{
    __shared__ int32_t s[kScanThreads];
    const int t = threadIdx.x;
    const int32_t chunk = (n + kScanThreads - 1) / kScanThreads;
    const int32_t b = min(n, t * chunk), e = min(n, b + chunk);
    int32_t sum = 0;
    for (int32_t i = b; i < e; ++i) sum += in[i];
    s[t] = sum;
    __syncthreads();
    for (int d = 1; d < kScanThreads; d <<= 1) {
        const int32_t v = t >= d ? s[t - d] : 0;
        __syncthreads();
        s[t] += v;
        __syncthreads();
    }
    int32_t run = s[t] - sum;
    for (int32_t i = b; i < e; ++i) {
        const int32_t v = in[i];
        out[i] = run;
        run += v;
    }
    if (t == kScanThreads - 1) out[n] = s[t];
}

// transposed CSR: phase 0 in-degrees, phase 1 (after the scan of them into trow) every edge u -> v stored under v.  Slots inside
// a list are taken with an atomic cursor, so their order varies from build to build; the tree's reduction over a list is a
// minimum under a total order and does not depend on it.
__global__ void rm_transpose_kernel(int32_t n, const int32_t *__restrict__ row, const int32_t *__restrict__ col, int32_t *__restrict__ indeg,
                                    const int32_t *__restrict__ trow, int32_t *__restrict__ cursor, int32_t *__restrict__ tcol, int phase)
{
    const int32_t u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= n) return;
    for (int32_t j = row[u]; j < row[u + 1]; ++j) {
        const int32_t v = col[j];
        if (phase == 0) atomicAdd(&indeg[v], 1);
        else tcol[trow[v] + atomicAdd(&cursor[v], 1)] = u;
    }
}

__global__ void rm_tree_init_kernel(FsRmTree t)
{
    const int32_t root = t.root;
    const int32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= t.n) return;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        t.d[b][v] = v == root ? 0.0 : INFINITY;
        t.hops[b][v] = v == root ? 0 : INT32_MAX;
        t.pred[b][v] = -1;
    }
}

// One Jacobi step for node v: buffer `src` -> buffer src ^ 1, the key recomputed from the in-neighbours' keys alone (v's own old
// key takes no part, so that a fixed point is the system's solution, not a remnant of an earlier round).  Returns whether it changed.
__device__ __forceinline__ bool relax(const FsRmTree &t, int src, int32_t v)
{
    const double *D = t.d[src];
    const int32_t *H = t.hops[src], *P = t.pred[src];
    const bool is_root = v == t.root;
    double bd = is_root ? 0.0 : INFINITY;
    int32_t bh = is_root ? 0 : INT32_MAX, bp = -1;
    const double vx = t.xy[2 * v], vy = t.xy[2 * v + 1];
    for (int32_t j = t.trow[v]; !is_root && j < t.trow[v + 1]; ++j) {
        const int32_t u = t.tcol[j];
        const double du = D[u];
        if (!(du < INFINITY)) continue;
        const double ex = t.xy[2 * u] - vx, ey = t.xy[2 * u + 1] - vy;
        const double cd = du + (ex * ex + ey * ey);
        const int32_t ch = H[u] + 1;
        if (cd < bd || (cd == bd && (ch < bh || (ch == bh && u < bp)))) { bd = cd; bh = ch; bp = u; }
    }
    const bool changed = bd != D[v] || bh != H[v] || bp != P[v];
    t.d[src ^ 1][v] = bd; t.hops[src ^ 1][v] = bh; t.pred[src ^ 1][v] = bp;
    return changed;
}

// The whole relaxation in one workgroup (n <= RM_TREE_ONE_WG): rounds separated by the workgroup barrier.  rounds[0] = rounds run
// (the last one quiet), or -1 if max_rounds passed without a quiet round.  The converged tree is in buffer rounds[0] & 1.
__global__ __launch_bounds__(1024) void rm_tree_block_kernel(FsRmTree t, int32_t max_rounds, int32_t *__restrict__ rounds)
{
    int src = 0;
    for (int32_t r = 1; r <= max_rounds; ++r) {
        int ch = 0;
        for (int32_t v = threadIdx.x; v < t.n; v += blockDim.x) ch |= relax(t, src, v) ? 1 : 0;
        src ^= 1;
        if (!__syncthreads_or(ch)) {
            if (threadIdx.x == 0) rounds[0] = r;
            return;
        }
    }
    if (threadIdx.x == 0) rounds[0] = -1;
}

// ... or one round per launch (larger graphs): any[0] = 1 (plain store) when a key changed
__global__ __launch_bounds__(256) void rm_tree_round_kernel(FsRmTree t, int32_t src, int32_t *__restrict__ any)
{
    const int32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    const int ch = (v < t.n && relax(t, src, v)) ? 1 : 0;
    if (__syncthreads_or(ch) && threadIdx.x == 0) any[0] = 1;
}

// setPlanForFrontierRoadmap, one lane per frontier: the goal's closest key node, then the tree's predecessors back to the root,
// the segment lengths summed from the goal end as astar.cpp:57-63 does
__global__ void rm_plan_kernel(const FsRmPlanArgs a)
{
    const int32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= a.n) return;
    const double dmax = DBL_MAX;
    double len = dmax, head = dmax;
    uint8_t ok = 0;
    if (a.mode[f] == 1) {
        len = 0.0; head = a.heading_in[f]; ok = 1;
    } else if (a.mode[f] == 2 && a.d) {
        int32_t v = fs_rm_closest(a.xy, a.key, a.n_nodes, a.cell, a.goal[2 * f], a.goal[2 * f + 1]);
        if (v >= 0 && a.d[v] < INFINITY) {
            double s = 0.0;
            for (int32_t k = 0; v != a.root && k < a.n_nodes; ++k) {
                const int32_t u = a.pred[v];
                const double ex = a.xy[2 * v] - a.xy[2 * u], ey = a.xy[2 * v + 1] - a.xy[2 * u + 1];
                s += sqrt(ex * ex + ey * ey);
                v = u;
            }
            len = s; head = a.heading_in[f]; ok = 1;
        }
    }
    a.path_length[f] = len;
    a.path_length_m[f] = len;
    a.path_heading[f] = head;
    a.achievable[f] = ok;
}

}  // namespace

hipError_t fs_launch_rm_candidates(const FsRoadmapDev &g, const int32_t *d_off, int32_t *d_count, double oz, double *d_start,
                                   double *d_end, int32_t *d_cand, hipStream_t s)
{
    if (g.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(rm_candidates_kernel, dim3((unsigned)((g.n + 63) / 64)), dim3(64), 0, s, g, d_off, d_count, oz, d_start, d_end, d_cand);
    return hipGetLastError();
}

hipError_t fs_launch_rm_edges(int32_t n, const int32_t *d_cand_off, const int32_t *d_cand, const uint8_t *d_ok, const uint8_t *d_hit,
                              const int32_t *d_unknown, double unknown_limit, const int32_t *d_row, int32_t *d_count, int32_t *d_col,
                              hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(rm_edges_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, n, d_cand_off, d_cand, d_ok, d_hit, d_unknown,
                       unknown_limit, d_row, d_count, d_col);
    return hipGetLastError();
}

hipError_t fs_launch_rm_scan(const int32_t *d_in, int32_t n, int32_t *d_out, hipStream_t s)
{
    hipLaunchKernelGGL(rm_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, d_in, n, d_out);
    return hipGetLastError();
}

hipError_t fs_launch_rm_transpose(int32_t n, const int32_t *d_row, const int32_t *d_col, int32_t *d_indeg, int32_t *d_trow,
                                  int32_t *d_cursor, int32_t *d_tcol, hipStream_t s, int phase)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(rm_transpose_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, d_row, d_col, d_indeg, d_trow, d_cursor,
                       d_tcol, phase);
    return hipGetLastError();
}

hipError_t fs_launch_rm_tree_init(const FsRmTree &t, hipStream_t s)
{
    if (t.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(rm_tree_init_kernel, dim3((unsigned)((t.n + 255) / 256)), dim3(256), 0, s, t);
    return hipGetLastError();
}

hipError_t fs_launch_rm_tree_block(const FsRmTree &t, int32_t max_rounds, int32_t *d_rounds, hipStream_t s)
{
    hipLaunchKernelGGL(rm_tree_block_kernel, dim3(1), dim3(1024), 0, s, t, max_rounds, d_rounds);
    return hipGetLastError();
}

hipError_t fs_launch_rm_tree_round(const FsRmTree &t, int32_t src, int32_t *d_any, hipStream_t s)
{
    if (t.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(rm_tree_round_kernel, dim3((unsigned)((t.n + 255) / 256)), dim3(256), 0, s, t, src, d_any);
    return hipGetLastError();
}

hipError_t fs_launch_rm_plan(const FsRmPlanArgs &a, hipStream_t s)
{
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(rm_plan_kernel, dim3((unsigned)((a.n + 63) / 64)), dim3(64), 0, s, a);
    return hipGetLastError();
}
