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
#include "fs_roadmap_astar.h"

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
__device__ __forceinline__ void tree_block(const FsRmTree &t, int32_t max_rounds, int32_t *__restrict__ rounds)
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

__global__ __launch_bounds__(1024) void rm_tree_block_kernel(FsRmTree t, int32_t max_rounds, int32_t *__restrict__ rounds)
{
    tree_block(t, max_rounds, rounds);
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
__device__ __forceinline__ void plan_frontier(const FsRmPlanArgs &a, int32_t f)
{
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

__global__ void rm_plan_kernel(const FsRmPlanArgs a)
{
    const int32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f < a.n) plan_frontier(a, f);
}

// the fleet's plan (fs_fleet_allocate_roadmap): blockIdx.y is the robot, robots[r] its own plan — its tree, root,
// modes, headings and its row of the four columns; the goals are shared
__global__ void rm_fleet_plan_kernel(const FsRmPlanArgs *__restrict__ robots)
{
    const FsRmPlanArgs a = robots[blockIdx.y];
    const int32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f < a.n) plan_frontier(a, f);
}


// ---- next goal

// tree b of a batch: the graph of B.t, its own root and round buffers
__device__ __forceinline__ FsRmTree batch_tree(const FsRmTreeBatch &B, int b)
{
    FsRmTree t = B.t;
    const size_t o = 2 * (size_t)t.n * (size_t)b;
    t.root = B.root[b];
    t.d[0] = B.t.d[0] + o; t.d[1] = t.d[0] + t.n;
    t.hops[0] = B.t.hops[0] + o; t.hops[1] = t.hops[0] + t.n;
    t.pred[0] = B.t.pred[0] + o; t.pred[1] = t.pred[0] + t.n;
    return t;
}

__global__ void rm_batch_init_kernel(FsRmTreeBatch B)
{
    const FsRmTree t = batch_tree(B, blockIdx.y);
    const int32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= t.n) return;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        t.d[b][v] = v == t.root ? 0.0 : INFINITY;
        t.hops[b][v] = v == t.root ? 0 : INT32_MAX;
        t.pred[b][v] = -1;
    }
}

// every tree of the batch in a workgroup of its own, the loop of rm_tree_block_kernel.  The tree's descriptor sits in LDS: relax()
// picks its buffers by the round's parity, and a descriptor in registers would be indexed through scratch.
__global__ __launch_bounds__(1024) void rm_batch_block_kernel(FsRmTreeBatch B, int32_t max_rounds, int32_t *__restrict__ rounds)
{
    __shared__ FsRmTree t;
    if (threadIdx.x == 0) t = batch_tree(B, blockIdx.x);
    __syncthreads();
    tree_block(t, max_rounds, rounds + blockIdx.x);
}

__global__ __launch_bounds__(256) void rm_batch_round_kernel(FsRmTreeBatch B, int32_t src, int32_t *__restrict__ any)
{
    __shared__ FsRmTree t;
    if (threadIdx.x == 0) t = batch_tree(B, blockIdx.y);
    __syncthreads();
    const int32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    const int ch = (v < t.n && relax(t, src, v)) ? 1 : 0;
    if (__syncthreads_or(ch) && threadIdx.x == 0) any[0] = 1;
}

// getPlan(point i, true, point j, true) for every pair i < j, one lane each: the tree from i's closest key node, the segment
// lengths summed from j's end back along the predecessors as rm_plan_kernel does.  The lower index is the direction (DESIGN.md
// 4.11); M[j][i] = M[i][j].
__global__ __launch_bounds__(256) void rm_pairs_kernel(const FsRmPairArgs a)
{
    const int32_t l = threadIdx.x, m = a.m;
    if (l >= m * m) return;
    const int32_t i = l / m, j = l % m;
    if (i == j) { a.M[l] = 0.0; return; }
    if (i > j) return;
    double len = a.charge;
    if (a.pxy[2 * i] == a.pxy[2 * j] && a.pxy[2 * i + 1] == a.pxy[2 * j + 1]) {
        len = 0.0;
    } else if (a.q_status) {
        const int32_t q = a.query[l];
        if (q >= 0 && a.q_status[q] == FS_ASTAR_FOUND) len = a.q_len[q];
    } else {
        const int32_t root = a.start[i];
        int32_t v = a.start[j];
        if (root >= 0 && v >= 0) {
            const size_t o = 2 * (size_t)a.n_nodes * (size_t)a.tree[i];
            const double *d = a.d + o;
            const int32_t *pred = a.pred + o;
            if (d[v] < INFINITY) {
                double s = 0.0;
                for (int32_t k = 0; v != root && k < a.n_nodes; ++k) {
                    const int32_t u = pred[v];
                    const double ex = a.xy[2 * v] - a.xy[2 * u], ey = a.xy[2 * v + 1] - a.xy[2 * u + 1];
                    s += sqrt(ex * ex + ey * ey);
                    v = u;
                }
                len = s;
            }
        }
    }
    a.M[i * m + j] = len;
    a.M[j * m + i] = len;
}

constexpr int kTourThreads = 256;
constexpr int kTourMinChunk = 64;       // ranks per lane at least (the unranking is paid once per lane)
constexpr int kTourMaxBlocks = 1024;

// a lane's or a block's best tour: the lexicographic minimum of (length, robot leg, rank), and how many tours have that length
struct TourBest {
    double len, leg;
    int64_t rank, cnt;
};

__device__ __forceinline__ void tour_merge(TourBest &a, const TourBest &b)
{
    if (b.len < a.len) {
        a = b;
    } else if (b.len == a.len) {
        a.cnt += b.cnt;
        if (b.leg < a.leg || (b.leg == a.leg && b.rank < a.rank)) { a.leg = b.leg; a.rank = b.rank; }
    }
}

// the workgroup's minimum in thread 0: across the wave by shuffles, then across the waves in LDS
__device__ TourBest tour_block_reduce(TourBest x)
{
    __shared__ TourBest part[kTourThreads / 64];
    for (int o = 32; o > 0; o >>= 1) {
        TourBest y;
        y.len = __shfl_xor(x.len, o); y.leg = __shfl_xor(x.leg, o);
        y.rank = __shfl_xor(x.rank, o); y.cnt = __shfl_xor(x.cnt, o);
        tour_merge(x, y);
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = x;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w) tour_merge(x, part[w]);
    return x;
}

// The exhaustive tour search.  Lane g takes the ranks [g * chunk, (g + 1) * chunk) of the lexicographic order of the locals'
// positions 0..k-1: it unranks the first (factorial number system), then steps with next_permutation.  Tour length = the legs
// robot -> p0 -> ... -> p(k-1) -> global added left to right in fp64 from 0.0, the reference's order; the prefix sums of the legs are
// kept, so a step re-adds only the legs from the first changed position on, and every length is bit-equal to a full recomputation.
// The permutation and the prefix sums live in LDS, [position][lane].
__global__ __launch_bounds__(kTourThreads) void rm_tour_kernel(const FsRmTourArgs a)
{
    __shared__ double Ms[RM_TOUR_MAX_NODES * RM_TOUR_MAX_NODES];
    __shared__ double P[RM_TOUR_MAX_LOCAL + 1][kTourThreads];
    __shared__ uint8_t perm[RM_TOUR_MAX_LOCAL][kTourThreads];
    const int k = a.k, m = k + 2, L = threadIdx.x;
    for (int i = L; i < m * m; i += blockDim.x) Ms[i] = a.M[i];
    __syncthreads();
    TourBest best{INFINITY, INFINITY, INT64_MAX, 0};
    const int64_t r0 = ((int64_t)blockIdx.x * blockDim.x + L) * a.chunk;
    const int64_t r1 = r0 + a.chunk < a.total ? r0 + a.chunk : a.total;
    if (r0 < a.total) {
        // unrank r0: digit t (base k - t) picks the digit-th unused position
        int64_t f = 1;
        for (int t = 2; t < k; ++t) f *= t;                      // (k - 1)!
        uint32_t used = 0;
        int64_t r = r0;
        for (int t = 0; t < k; ++t) {
            const int64_t dgt = r / f;
            r -= dgt * f;
            if (t < k - 1) f /= (k - 1 - t);
            int c = -1;
            for (int64_t s = 0; s <= dgt;) { ++c; if (!(used >> c & 1u)) ++s; }
            used |= 1u << c;
            perm[t][L] = (uint8_t)c;
        }
        int first = 0;                                          // legs from position `first` on are (re)added
        for (int64_t rank = r0;; ++rank) {
            int prev = first == 0 ? 0 : perm[first - 1][L] + 1;
            double acc = first == 0 ? 0.0 : P[first][L];
            for (int t = first; t < k; ++t) {
                const int cur = perm[t][L] + 1;
                acc += Ms[prev * m + cur];
                P[t + 1][L] = acc;
                prev = cur;
            }
            acc += Ms[prev * m + (k + 1)];
            tour_merge(best, TourBest{acc, Ms[perm[0][L] + 1], rank, 1});
            if (rank + 1 >= r1) break;
            // next_permutation: i = the last ascent, j = the last element above p[i]; swap, reverse the suffix
            int i = k - 2;
            while (perm[i][L] >= perm[i + 1][L]) --i;           // an ascent exists: rank + 1 < k!
            int j = k - 1;
            while (perm[j][L] <= perm[i][L]) --j;
            uint8_t x = perm[i][L]; perm[i][L] = perm[j][L]; perm[j][L] = x;
            for (int lo = i + 1, hi = k - 1; lo < hi; ++lo, --hi) { x = perm[lo][L]; perm[lo][L] = perm[hi][L]; perm[hi][L] = x; }
            first = i;
        }
    }
    best = tour_block_reduce(best);
    if (L == 0) { a.blen[blockIdx.x] = best.len; a.bleg[blockIdx.x] = best.leg; a.brank[blockIdx.x] = best.rank; a.bcnt[blockIdx.x] = best.cnt; }
}

// one workgroup over the blocks' winners (the same total order, so the result does not depend on the blocks' order)
__global__ __launch_bounds__(kTourThreads) void rm_tour_reduce_kernel(const FsRmTourArgs a, int32_t blocks, double *__restrict__ out)
{
    TourBest best{INFINITY, INFINITY, INT64_MAX, 0};
    for (int32_t b = threadIdx.x; b < blocks; b += blockDim.x) tour_merge(best, TourBest{a.blen[b], a.bleg[b], a.brank[b], a.bcnt[b]});
    best = tour_block_reduce(best);
    if (threadIdx.x == 0) {
        out[0] = best.len; out[1] = best.leg;
        int64_t *o = reinterpret_cast<int64_t *>(out + 2);
        o[0] = best.rank; o[1] = best.cnt;
    }
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

hipError_t fs_launch_rm_fleet_plan(const FsRmPlanArgs *d_robots, int32_t n_robots, int32_t n, hipStream_t s)
{
    if (n <= 0 || n_robots <= 0) return hipSuccess;
    hipLaunchKernelGGL(rm_fleet_plan_kernel, dim3((unsigned)((n + 63) / 64), (unsigned)n_robots), dim3(64), 0, s, d_robots);
    return hipGetLastError();
}

hipError_t fs_launch_rm_batch_init(const FsRmTreeBatch &b, hipStream_t s)
{
    if (b.t.n <= 0 || b.k <= 0) return hipSuccess;
    hipLaunchKernelGGL(rm_batch_init_kernel, dim3((unsigned)((b.t.n + 255) / 256), (unsigned)b.k), dim3(256), 0, s, b);
    return hipGetLastError();
}

hipError_t fs_launch_rm_batch_block(const FsRmTreeBatch &b, int32_t max_rounds, int32_t *d_rounds, hipStream_t s)
{
    if (b.k <= 0) return hipSuccess;
    hipLaunchKernelGGL(rm_batch_block_kernel, dim3((unsigned)b.k), dim3(1024), 0, s, b, max_rounds, d_rounds);
    return hipGetLastError();
}

hipError_t fs_launch_rm_batch_round(const FsRmTreeBatch &b, int32_t src, int32_t *d_any, hipStream_t s)
{
    if (b.t.n <= 0 || b.k <= 0) return hipSuccess;
    hipLaunchKernelGGL(rm_batch_round_kernel, dim3((unsigned)((b.t.n + 255) / 256), (unsigned)b.k), dim3(256), 0, s, b, src, d_any);
    return hipGetLastError();
}

hipError_t fs_launch_rm_pairs(const FsRmPairArgs &a, hipStream_t s)
{
    if (a.m < 2 || a.m > RM_TOUR_MAX_NODES) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rm_pairs_kernel, dim3(1), dim3(256), 0, s, a);
    return hipGetLastError();
}

// blocks of the tour search for k! tours and the ranks per lane
int32_t fs_rm_tour_blocks(int64_t total, int64_t *chunk)
{
    int64_t blocks = (total + (int64_t)kTourThreads * kTourMinChunk - 1) / ((int64_t)kTourThreads * kTourMinChunk);
    blocks = blocks < 1 ? 1 : blocks > kTourMaxBlocks ? kTourMaxBlocks : blocks;
    const int64_t lanes = blocks * kTourThreads;
    *chunk = (total + lanes - 1) / lanes;
    return (int32_t)blocks;
}

hipError_t fs_launch_rm_tour(const FsRmTourArgs &a, int32_t blocks, double *d_out, hipStream_t s)
{
    if (a.k < 1 || a.k > RM_TOUR_MAX_LOCAL || blocks < 1 || blocks > kTourMaxBlocks) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rm_tour_kernel, dim3((unsigned)blocks), dim3(kTourThreads), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rm_tour_reduce_kernel, dim3(1), dim3(kTourThreads), 0, s, a, blocks, d_out);
    return hipGetLastError();
}


// ---- the REFERENCE search: FrontierRoadmapAStar::getPlan per distinct (start, goal) pair, one wave per query

namespace {

constexpr int kAstarThreads = 64;

// one query's storage laid out from `base` (fs_rm_astar_bytes(cap, n) bytes, 16-byte aligned): doubles first
__device__ __forceinline__ fs_astar_mem astar_carve(char *base, int32_t cap, int32_t n)
{
    fs_astar_mem m;
    m.heap_f = reinterpret_cast<double *>(base);
    m.rec_g = m.heap_f + cap;
    m.heap_rec = reinterpret_cast<int32_t *>(m.rec_g + cap);
    m.rec_node = m.heap_rec + cap;
    m.rec_parent = m.rec_node + cap;
    m.best = m.rec_parent + cap;
    m.closed = reinterpret_cast<uint8_t *>(m.best + n);
    m.cap = cap;
    return m;
}

// fs_astar_run by one wave: lane 0 owns the heap and the records; the lanes evaluate a popped node's successors 64 at a time (g, h,
// f and the closed / best-g test), and the accepted ones are committed one at a time in adjacency order, each re-tested at commit
// (an earlier commit of the same chunk can only lower a best g, so a successor rejected at evaluation stays rejected).  The
// workgroup is this one wave: its barriers order lane 0's stores before the other lanes' loads, in LDS and in global memory alike.
__device__ __forceinline__ int astar_wave(const fs_astar_graph &G, const fs_astar_mem &m, int32_t start, int32_t goal, double *len,
                                          int32_t *pops, int32_t *goal_rec)
{
    const int lane = threadIdx.x;
    for (int32_t v = lane; v < G.n; v += kAstarThreads) { m.best[v] = -1; m.closed[v] = 0; }
    __syncthreads();
    int32_t nrec = 0, hsize = 0;                                    // (lane 0's)
    if (lane == 0) fs_astar_begin(m, start, nrec, hsize);
    __syncthreads();
    const double gx = G.xy[2 * goal], gy = G.xy[2 * goal + 1];
    int32_t np = 0;
    double L = 0.0;
    int result = FS_ASTAR_NO_PATH;
    for (;;) {
        int32_t r = -1;
        if (lane == 0 && hsize > 0) r = fs_astar_pop(m.heap_f, m.heap_rec, hsize);
        r = __shfl(r, 0);
        if (r < 0) break;
        ++np;
        const int32_t cur = m.rec_node[r];
        if (G.xy[2 * cur] == gx && G.xy[2 * cur + 1] == gy) {
            if (lane == 0) L = fs_astar_length(m, G.xy, m.best[cur]);
            *goal_rec = m.best[cur];
            result = FS_ASTAR_FOUND;
            break;
        }
        const double cg = m.rec_g[r];
        if (lane == 0) m.closed[cur] = 1;
        __syncthreads();
        const int32_t b = G.row[cur], e = G.row[cur + 1];
        bool ovf = false;
        for (int32_t j0 = b; j0 < e && !ovf; j0 += kAstarThreads) {
            const int32_t j = j0 + lane;
            int32_t nb = 0;
            double g = 0.0, f = 0.0;
            bool cand = false;
            if (j < e) {
                nb = G.col[j];
                g = cg + fs_astar_sq(G.xy, cur, nb);
                const double h = fs_astar_sq(G.xy, nb, goal);
                f = g + h;
                cand = fs_astar_accepts(m, nb, g);
            }
            uint64_t mask = __ballot(cand);
            while (mask) {
                const int t = __builtin_ctzll(mask);
                mask &= mask - 1;
                const int32_t nb_t = __shfl(nb, t);
                const double g_t = __shfl(g, t), f_t = __shfl(f, t);
                int full = 0;
                if (lane == 0 && fs_astar_accepts(m, nb_t, g_t) && !fs_astar_commit(m, cur, nb_t, g_t, f_t, nrec, hsize)) full = 1;
                if (__shfl(full, 0)) { ovf = true; break; }
            }
            __syncthreads();
        }
        if (ovf) { result = FS_ASTAR_OVERFLOW; break; }
    }
    *len = L;
    *pops = np;
    return result;
}

__device__ __forceinline__ int32_t astar_src(const FsRmAstarArgs &a, int32_t q) { return a.src ? a.src[q] : a.root; }

// the FOUND query's path (astar.cpp:57-69) while its records are still there: the chain from record r up the parents, goal node
// first, into the query's slots of the chain pool (lane 0).  The cursor is bumped by every chain, written or not.
__device__ __forceinline__ void astar_chain(const FsRmAstarArgs &a, const fs_astar_mem &m, int32_t q, int32_t r)
{
    int32_t L = 0;
    for (int32_t p = r; p >= 0; p = m.rec_parent[p]) ++L;
    const int64_t base = (int64_t)atomicAdd(a.chain_cursor, (unsigned long long)L);
    a.chain_len[q] = L;
    a.chain_base[q] = base;
    if (base + L > a.chain_cap) return;
    int64_t k = base;
    for (int32_t p = r; p >= 0; p = m.rec_parent[p]) a.chain_pool[k++] = m.rec_node[p];
}

// the LDS route, one workgroup (one wave) per query
__global__ __launch_bounds__(kAstarThreads) void rm_astar_lds_kernel(const FsRmAstarArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int32_t q = blockIdx.x, nq = a.nq[0];
    if (q == 0 && threadIdx.x == 0) a.stats[0] = nq;
    if (q >= nq) return;
    int st = FS_ASTAR_OVERFLOW;
    double len = 0.0;
    int32_t pops = 0, rec = -1;
    if (a.lds_cap > 0) {
        const fs_astar_graph G{a.n_nodes, a.xy, a.row, a.col};
        const fs_astar_mem m = astar_carve(smem, a.lds_cap, a.n_nodes);
        st = astar_wave(G, m, astar_src(a, q), a.dst[q], &len, &pops, &rec);
        if (a.chain_len && st == FS_ASTAR_FOUND && threadIdx.x == 0) astar_chain(a, m, q, rec);
    }
    if (threadIdx.x == 0) {
        a.status[q] = st;
        if (st == FS_ASTAR_OVERFLOW) {
            atomicAdd(&a.stats[2], 1);
        } else {
            a.len[q] = len;
            atomicMax(&a.stats[1], pops);
        }
    }
}

// the global route: `slots` workgroups take the queries left with FS_ASTAR_OVERFLOW in turn, each in its slot of the pool
__global__ __launch_bounds__(kAstarThreads) void rm_astar_global_kernel(const FsRmAstarArgs a)
{
    const int32_t nq = a.nq[0];
    const fs_astar_graph G{a.n_nodes, a.xy, a.row, a.col};
    const fs_astar_mem m = astar_carve(a.pool + (size_t)blockIdx.x * a.slot_bytes, a.cap, a.n_nodes);
    for (int32_t q = blockIdx.x; q < nq; q += gridDim.x) {
        if (a.status[q] != FS_ASTAR_OVERFLOW) continue;
        double len = 0.0;
        int32_t pops = 0, rec = -1;
        const int st = astar_wave(G, m, astar_src(a, q), a.dst[q], &len, &pops, &rec);
        if (threadIdx.x == 0) {
            if (a.chain_len && st == FS_ASTAR_FOUND) astar_chain(a, m, q, rec);
            if (st == FS_ASTAR_OVERFLOW) {
                atomicAdd(&a.stats[3], 1);
            } else {
                a.status[q] = st;
                a.len[q] = len;
                atomicMax(&a.stats[1], pops);
            }
        }
        __syncthreads();                // (the slot is reused by the next query)
    }
}

// every planned frontier's goal node (getClosestNodeInRoadMap of the goal), marked as a query
__global__ void rm_astar_goals_kernel(const FsRmPlanArgs a, int32_t *__restrict__ gnode, int32_t *__restrict__ mark)
{
    const int32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= a.n) return;
    int32_t v = -1;
    if (a.mode[f] == 2 && a.root >= 0) v = fs_rm_closest(a.xy, a.key, a.n_nodes, a.cell, a.goal[2 * f], a.goal[2 * f + 1]);
    gnode[f] = v;
    if (v >= 0) mark[v] = 1;
}

__global__ void rm_astar_list_kernel(int32_t n, const int32_t *__restrict__ mark, const int32_t *__restrict__ qidx, int32_t *__restrict__ dst)
{
    const int32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v < n && mark[v]) dst[qidx[v]] = v;
}

// rm_plan_kernel's columns from the goal node's query
__global__ void rm_astar_cols_kernel(const FsRmPlanArgs a, const int32_t *__restrict__ gnode, const int32_t *__restrict__ qidx,
                                     const int32_t *__restrict__ status, const double *__restrict__ qlen)
{
    const int32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= a.n) return;
    const double dmax = DBL_MAX;
    double len = dmax, head = dmax;
    uint8_t ok = 0;
    if (a.mode[f] == 1) {
        len = 0.0; head = a.heading_in[f]; ok = 1;
    } else if (a.mode[f] == 2 && gnode[f] >= 0) {
        const int32_t q = qidx[gnode[f]];
        if (status[q] == FS_ASTAR_FOUND) { len = qlen[q]; head = a.heading_in[f]; ok = 1; }
    }
    a.path_length[f] = len;
    a.path_length_m[f] = len;
    a.path_heading[f] = head;
    a.achievable[f] = ok;
}


// ---- routes

// a node's route: hops + 1 nodes under the tree, the chain of its query under the REFERENCE search; 0 where no planned frontier
// ends or the goal was not reached
__global__ void rm_route_lengths_kernel(const FsRmRouteArgs a)
{
    const int32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= a.n_nodes) return;
    int32_t len = 0;
    if (a.mark[v]) {
        if (a.status) {
            const int32_t q = a.qidx[v];
            if (a.status[q] == FS_ASTAR_FOUND) len = a.chain_len[q];
        } else if (a.d && a.d[v] < INFINITY) {
            len = a.hops[v] + 1;
        }
    }
    a.len[v] = len;
    a.has[v] = len > 0 ? 1 : 0;
}

// lanes over the nodes, then over the frontiers: route ridx[v] ends at node v; a frontier's route is its goal node's
__global__ void rm_route_index_kernel(const FsRmRouteArgs a)
{
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.n_nodes && a.has[i]) {
        const int32_t r = a.ridx[i];
        a.goal_node[r] = i;
        a.route_len[r] = a.len[i];
        a.route_q[r] = a.status ? a.qidx[i] : -1;
    }
    if (i < a.n) {
        const int32_t v = a.gnode[i];
        a.route_of[i] = (v >= 0 && a.has[v]) ? a.ridx[v] : -1;
    }
}

// one wave per route, start node first: the tree's predecessors from the goal node back (lane 0: the chain is sequential), or
// the query's chain out of the pool, reversed (every lane)
__global__ __launch_bounds__(256) void rm_route_emit_kernel(const FsRmRouteArgs a)
{
    const int32_t r = (int32_t)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= a.n_routes) return;
    const int64_t base = a.node_off[r];
    const int32_t m = (int32_t)(a.node_off[r + 1] - base);
    if (a.status) {
        const int64_t src = a.chain_base[a.route_q[r]];
        for (int32_t k = lane; k < m; k += 64) a.node[base + k] = a.chain_pool[src + (m - 1 - k)];
    } else if (lane == 0) {
        int32_t v = a.goal_node[r];
        for (int32_t k = m - 1; k >= 0; --k) { a.node[base + k] = v; v = a.pred[v]; }
    }
}

}  // namespace

hipError_t fs_launch_rm_route_lengths(const FsRmRouteArgs &a, hipStream_t s)
{
    if (a.n_nodes <= 0) return hipSuccess;
    hipLaunchKernelGGL(rm_route_lengths_kernel, dim3((unsigned)((a.n_nodes + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t fs_launch_rm_route_index(const FsRmRouteArgs &a, hipStream_t s)
{
    const int32_t lanes = a.n_nodes > a.n ? a.n_nodes : a.n;
    if (lanes <= 0) return hipSuccess;
    hipLaunchKernelGGL(rm_route_index_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t fs_launch_rm_route_emit(const FsRmRouteArgs &a, hipStream_t s)
{
    if (a.n_routes <= 0) return hipSuccess;
    hipLaunchKernelGGL(rm_route_emit_kernel, dim3((unsigned)((a.n_routes + 3) / 4)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t fs_launch_rm_astar(const FsRmAstarArgs &a, int32_t max_q, hipStream_t s)
{
    if (max_q > 0) {
        const size_t lds = a.lds_cap > 0 ? fs_rm_astar_bytes(a.lds_cap, a.n_nodes) : 0;
        if (lds > RM_ASTAR_LDS_BYTES) return hipErrorInvalidValue;
        hipLaunchKernelGGL(rm_astar_lds_kernel, dim3((unsigned)max_q), dim3(kAstarThreads), lds, s, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return fs_launch_rm_astar_global(a, s);
}

hipError_t fs_launch_rm_astar_global(const FsRmAstarArgs &a, hipStream_t s)
{
    if (a.slots < 1 || a.cap < 1 || !a.pool) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rm_astar_global_kernel, dim3((unsigned)a.slots), dim3(kAstarThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t fs_launch_rm_astar_goals(const FsRmPlanArgs &p, int32_t *d_gnode, int32_t *d_mark, hipStream_t s)
{
    if (p.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(rm_astar_goals_kernel, dim3((unsigned)((p.n + 63) / 64)), dim3(64), 0, s, p, d_gnode, d_mark);
    return hipGetLastError();
}

hipError_t fs_launch_rm_astar_list(int32_t n_nodes, const int32_t *d_mark, const int32_t *d_qidx, int32_t *d_dst, hipStream_t s)
{
    if (n_nodes <= 0) return hipSuccess;
    hipLaunchKernelGGL(rm_astar_list_kernel, dim3((unsigned)((n_nodes + 255) / 256)), dim3(256), 0, s, n_nodes, d_mark, d_qidx, d_dst);
    return hipGetLastError();
}

hipError_t fs_launch_rm_astar_cols(const FsRmPlanArgs &p, const int32_t *d_gnode, const int32_t *d_qidx, const int32_t *d_status,
                                   const double *d_len, hipStream_t s)
{
    if (p.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(rm_astar_cols_kernel, dim3((unsigned)((p.n + 63) / 64)), dim3(64), 0, s, p, d_gnode, d_qidx, d_status, d_len);
    return hipGetLastError();
}
