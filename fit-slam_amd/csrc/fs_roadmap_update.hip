// fs_roadmap_update.hip — UpdateRoadmapBT on the device: addNodes(frontier_list), addRobotPoseAsNode,
// constructNewEdges(frontier_list) and constructNewEdgeRobotPose decided by the order-free rules of fs_roadmap_update.h.
//
// Reference: DEP/src/ExplorationBT.cpp:247-257; DEP/src/planners/FrontierRoadmap.cpp — populateNodes (:185-252),
// constructNewEdges (:279-334), getNodesWithinRadius (:410-436), getClosestNodeInHashmap (:464-504), isConnectable (:716-737).
//
// The hash is not built: a node's hash cell is a function of its position, so every hash question ("the nodes of the 3 x 3 cells",
// "the cells within the radius, dx outer, dy inner") is a filter and an order over the node list.  A wave scans the list 64 nodes
// at a time; at 430 points and 20 000 nodes that is 8.6 M distance tests per stage, far below what building, sorting and probing
// a hash per call would cost in launches.
//
//   screen      a wave per point: rejected by an existing node?  existing nodes in its cell;  its conflict row (earlier points)
//   keep        one workgroup: the Jacobi rounds seeded with the screened rejections, the cell cap, the kept points appended to the
//               node list in order, then the robot pose against the old and the new nodes
//   closest     a wave per point and one for the robot pose: getClosestNodeInHashmap after the additions (two passes, cross-lane
//               minima under fs_rm_closest's tie rule);  the first query of every closest node by atomicMin
//   owners      one workgroup: the first occurrences numbered in order (owner ranks), their key flags
//   candidates  a wave per owner: counted, scanned, listed in index order with the scan cell, then placed in getNodesWithinRadius
//               order (a stable rank by scan cell) with the segment candidate -> owner
//   [fs_launch_segments walks them]
//   insert      a lane per candidate: the insert rule, then a scan and the (p, q) pairs in global order
#include "fs_internal.h"
#include "fs_roadmap_update.h"

#include <limits.h>

namespace {

constexpr int kWave = 64;
constexpr int kBlock = 256;
constexpr int kOne = 1024;                                  // the one-workgroup stages
constexpr int kMaxWords = (FS_RU_MAX_POINTS + 64) / 64 + 1; // bit words over n + 1 queries

__device__ __forceinline__ uint64_t below(int lane) { return (1ull << lane) - 1ull; }

__device__ __forceinline__ void point_of(const FsRmUpdate &u, int32_t i, double &x, double &y)
{
    if (i < u.n) { x = u.pts[(size_t)u.stride * i]; y = u.pts[(size_t)u.stride * i + 1]; }
    else { x = u.rx; y = u.ry; }
}

__global__ __launch_bounds__(kBlock) void ru_screen_kernel(const FsRmUpdate u)
{
    const int32_t i = (int32_t)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= u.n) return;
    double x, y;
    point_of(u, i, x, y);
    int rej = 0;
    int32_t occ = 0;
    for (int32_t k = lane; k < u.n_old; k += kWave) {
        const double qx = u.xy[2 * (size_t)k], qy = u.xy[2 * (size_t)k + 1];
        rej |= fs_ru_conflict(x, y, qx, qy, u.cell, u.min_frontier) ? 1 : 0;
        occ += fs_ru_same_cell(x, y, qx, qy, u.cell) ? 1 : 0;
    }
    rej = __any(rej);
    for (int d = 32; d > 0; d >>= 1) occ += __shfl_xor(occ, d);
    if (lane == 0) { u.rejected[i] = rej ? 1 : 0; u.occupants[i] = occ; }
    for (int32_t w = 0; w < u.words; ++w) {
        const int32_t j = w * kWave + lane;
        bool c = false;
        if (j < i) {
            double qx, qy;
            point_of(u, j, qx, qy);
            c = fs_ru_conflict(x, y, qx, qy, u.cell, u.min_frontier);
        }
        const uint64_t m = __ballot(c);
        if (lane == 0) u.conf[(size_t)i * u.words + w] = m;
    }
}

__global__ __launch_bounds__(kOne) void ru_keep_kernel(const FsRmUpdate u)
{
    __shared__ unsigned long long K[2][kMaxWords], R[2][kMaxWords];
    __shared__ int32_t cut, cell_count;
    const int t = threadIdx.x;
    const int32_t n = u.n, words = u.words;
    for (int32_t w = t; w < words; w += kOne) {
        unsigned long long r = 0;
        for (int b = 0; b < 64; ++b) {
            const int32_t i = w * 64 + b;
            if (i < n && u.rejected[i]) r |= 1ull << b;
        }
        K[0][w] = 0; R[0][w] = r;
    }
    if (t == 0) { cut = INT_MAX; cell_count = 0; }
    __syncthreads();
    int src = 0;
    int32_t rounds = -1;
    for (int32_t r = 1; r <= n + 1; ++r) {
        const int dst = src ^ 1;
        for (int32_t w = t; w < words; w += kOne) { K[dst][w] = K[src][w]; R[dst][w] = R[src][w]; }
        __syncthreads();
        int ch = 0;
        for (int32_t i = t; i < n; i += kOne) {
            const int32_t w = i >> 6;
            const unsigned long long bit = 1ull << (i & 63);
            if ((K[src][w] | R[src][w]) & bit) continue;
            const int v = fs_ru_keep_step(u.conf + (size_t)i * words, reinterpret_cast<const uint64_t *>(K[src]),
                                          reinterpret_cast<const uint64_t *>(R[src]), w + 1);
            if (v == FS_RU_KEPT) { atomicOr(&K[dst][w], bit); ch = 1; }
            else if (v == FS_RU_REJECTED) { atomicOr(&R[dst][w], bit); ch = 1; }
        }
        src = dst;
        if (!__syncthreads_or(ch)) { rounds = r; break; }
    }
    // the cell cap: the first kept point that finds its cell full ends the list (and stays)
    const unsigned long long *A = K[src];
    for (int32_t i = t; i < n; i += kOne) {
        if (!((A[i >> 6] >> (i & 63)) & 1ull)) continue;
        double x, y;
        point_of(u, i, x, y);
        int32_t before = u.occupants[i];
        for (int32_t j = 0; j < i; ++j) {
            if (!((A[j >> 6] >> (j & 63)) & 1ull)) continue;
            double qx, qy;
            point_of(u, j, qx, qy);
            before += fs_ru_same_cell(x, y, qx, qy, u.cell) ? 1 : 0;
        }
        if (fs_ru_trips(before)) atomicMin(&cut, i);
    }
    __syncthreads();
    unsigned long long *F = K[src ^ 1];                      // the kept points up to the cut
    for (int32_t w = t; w < words; w += kOne) {
        unsigned long long m = A[w];
        const int64_t last = (int64_t)cut - (int64_t)w * 64;  // bits 0 .. last stay
        if (last < 0) m = 0;
        else if (last < 63) m &= (2ull << last) - 1ull;
        F[w] = m;
    }
    __syncthreads();
    int32_t kept = 0;
    for (int32_t w = 0; w < words; ++w) kept += __popcll(F[w]);
    for (int32_t i = t; i < n; i += kOne) {
        const int32_t w = i >> 6;
        if (!((F[w] >> (i & 63)) & 1ull)) continue;
        int32_t rank = __popcll(F[w] & below(i & 63));
        for (int32_t v = 0; v < w; ++v) rank += __popcll(F[v]);
        const size_t o = (size_t)u.n_old + (size_t)rank;
        double x, y;
        point_of(u, i, x, y);
        u.xy[2 * o] = x; u.xy[2 * o + 1] = y;
        u.key[o] = 0;
    }
    __syncthreads();
    int32_t tripped = cut != INT_MAX ? 1 : 0, robot = 0;
    const int32_t nodes = u.n_old + kept;
    if (u.add_robot && !tripped) {
        int rej = 0;
        int32_t occ = 0;
        for (int32_t k = t; k < nodes; k += kOne) {
            const double qx = u.xy[2 * (size_t)k], qy = u.xy[2 * (size_t)k + 1];
            rej |= fs_ru_conflict(u.rx, u.ry, qx, qy, u.cell, u.min_robot) ? 1 : 0;
            occ += fs_ru_same_cell(u.rx, u.ry, qx, qy, u.cell) ? 1 : 0;
        }
        if (occ) atomicAdd(&cell_count, occ);
        rej = __syncthreads_or(rej);
        if (!rej) {
            robot = 1;
            if (fs_ru_trips(cell_count)) tripped = 2;
            if (t == 0) { u.xy[2 * (size_t)nodes] = u.rx; u.xy[2 * (size_t)nodes + 1] = u.ry; u.key[nodes] = 0; }
        }
    }
    if (t == 0) {
        u.hdr[FS_RU_H_KEPT] = kept; u.hdr[FS_RU_H_TRIPPED] = tripped; u.hdr[FS_RU_H_ROBOT] = robot;
        u.hdr[FS_RU_H_NODES] = nodes + robot; u.hdr[FS_RU_H_OWNERS] = 0; u.hdr[FS_RU_H_ROUNDS] = rounds; u.hdr[FS_RU_H_INSERTED] = 0;
    }
}

__device__ __forceinline__ int64_t iabs64(int64_t v) { return v < 0 ? -v : v; }

// getClosestNodeInHashmap of query i (fs_rm_closest with key == nullptr, the lanes over the nodes)
__global__ __launch_bounds__(kBlock) void ru_closest_kernel(const FsRmUpdate u)
{
    const int32_t i = (int32_t)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const int lane = threadIdx.x & 63;
    const int32_t nodes = u.hdr[FS_RU_H_NODES];
    if (i > u.n || u.hdr[FS_RU_H_TRIPPED] || nodes <= 0) return;
    double qx, qy;
    point_of(u, i, qx, qy);
    const int64_t cx = fs_rm_cell(qx, u.cell), cy = fs_rm_cell(qy, u.cell);
    long long cmin = INT64_MAX;
    for (int32_t k = lane; k < nodes; k += kWave) {
        const int64_t ax = iabs64(fs_rm_cell(u.xy[2 * (size_t)k], u.cell) - cx), ay = iabs64(fs_rm_cell(u.xy[2 * (size_t)k + 1], u.cell) - cy);
        const long long c = ax > ay ? ax : ay;
        cmin = c < cmin ? c : cmin;
    }
    for (int d = 32; d > 0; d >>= 1) { const long long o = __shfl_xor(cmin, d); cmin = o < cmin ? o : cmin; }
    const int64_t R = fs_ru_search_radius(cmin, u.cell);
    int32_t bk = -1;
    double bd = 0.0;
    long long bx = 0, by = 0;
    for (int32_t k = lane; k < nodes; k += kWave) {
        const double nx = u.xy[2 * (size_t)k], ny = u.xy[2 * (size_t)k + 1];
        const int64_t ax = fs_rm_cell(nx, u.cell) - cx, ay = fs_rm_cell(ny, u.cell) - cy;
        if (ax < -R || ax > R || ay < -R || ay > R) continue;
        const double ex = qx - nx, ey = qy - ny;
        const double dd = sqrt(ex * ex + ey * ey);
        if (fs_ru_closer(dd, ax, ay, k, bd, bx, by, bk)) { bk = k; bd = dd; bx = ax; by = ay; }
    }
    for (int d = 32; d > 0; d >>= 1) {
        const int32_t ok = __shfl_xor(bk, d);
        const double od = __shfl_xor(bd, d);
        const long long ox = __shfl_xor(bx, d), oy = __shfl_xor(by, d);
        if (fs_ru_closer(od, ox, oy, ok, bd, bx, by, bk)) { bk = ok; bd = od; bx = ox; by = oy; }
    }
    if (lane == 0) {
        u.closest[i] = bk;
        if (bk >= 0) atomicMin(&u.rank_of[bk], i);
    }
}

// the owners: the first query of every closest node, numbered in query order
__global__ __launch_bounds__(kOne) void ru_owner_kernel(const FsRmUpdate u)
{
    __shared__ unsigned long long F[kMaxWords];
    const int t = threadIdx.x;
    if (u.hdr[FS_RU_H_TRIPPED] || u.hdr[FS_RU_H_NODES] <= 0) return;      // (hdr owners stays 0)
    const int32_t m = u.n + 1, words = (m + 63) / 64;
    for (int32_t w = t; w < words; w += kOne) F[w] = 0;
    __syncthreads();
    for (int32_t i = t; i < m; i += kOne) {
        const int32_t p = u.closest[i];
        if (p >= 0 && u.rank_of[p] == i) atomicOr(&F[i >> 6], 1ull << (i & 63));
    }
    __syncthreads();
    for (int32_t i = t; i < m; i += kOne) {
        const int32_t w = i >> 6;
        if (!((F[w] >> (i & 63)) & 1ull)) continue;
        int32_t rank = __popcll(F[w] & below(i & 63));
        for (int32_t v = 0; v < w; ++v) rank += __popcll(F[v]);
        const int32_t p = u.closest[i];
        u.owner[rank] = p;
        u.rank_of[p] = rank;
        u.key[p] = 1;
    }
    if (t == 0) {
        int32_t owners = 0;
        for (int32_t w = 0; w < words; ++w) owners += __popcll(F[w]);
        u.hdr[FS_RU_H_OWNERS] = owners;
    }
}

// getNodesWithinRadius(owner of rank r) without the owner: counted (fill == 0) or listed in index order with the scan cell
__global__ __launch_bounds__(kBlock) void ru_cand_kernel(const FsRmUpdate u, int fill)
{
    const int32_t r = (int32_t)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const int lane = threadIdx.x & 63;
    if (r > u.n) return;
    if (r >= u.hdr[FS_RU_H_OWNERS]) {
        if (!fill && lane == 0) u.cand_count[r] = 0;
        return;
    }
    const int32_t nodes = u.hdr[FS_RU_H_NODES], p = u.owner[r];
    const double px = u.xy[2 * (size_t)p], py = u.xy[2 * (size_t)p + 1];
    int32_t k = fill ? u.cand_off[r] : 0;
    for (int32_t q0 = 0; q0 < nodes; q0 += kWave) {
        const int32_t q = q0 + lane;
        int32_t order = 0;
        const bool in = q < nodes && q != p && fs_ru_within(px, py, u.xy[2 * (size_t)q], u.xy[2 * (size_t)q + 1], u.cell, u.radius, &order);
        const uint64_t m = __ballot(in);
        if (fill && in) {
            const int32_t o = k + __popcll(m & below(lane));
            u.tmp_q[o] = q; u.tmp_order[o] = order;
        }
        k += __popcll(m);
    }
    if (!fill && lane == 0) u.cand_count[r] = k;
}

// candidate e of the index-ordered list to its place in getNodesWithinRadius order: cells in scan order, index order inside a cell
__global__ __launch_bounds__(kBlock) void ru_place_kernel(const FsRmUpdate u, int32_t total)
{
    const int32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    int32_t lo = 0, hi = u.n + 1;                            // the last rank whose offset is <= e
    while (hi - lo > 1) {
        const int32_t mid = (lo + hi) >> 1;
        if (u.cand_off[mid] <= e) lo = mid;
        else hi = mid;
    }
    const int32_t r = lo, b = u.cand_off[r], en = u.cand_off[r + 1];
    const int32_t mine = u.tmp_order[e];
    int32_t rank = 0;
    for (int32_t f = b; f < en; ++f) {
        const int32_t o = u.tmp_order[f];
        rank += (o < mine || (o == mine && f < e)) ? 1 : 0;
    }
    const int32_t pos = b + rank, q = u.tmp_q[e], p = u.owner[r];
    u.cand[pos] = q; u.cand_rank[pos] = r;
    u.key[q] = 1;
    double *s = u.seg_start + 3 * (size_t)pos, *d = u.seg_end + 3 * (size_t)pos;
    s[0] = u.xy[2 * (size_t)q]; s[1] = u.xy[2 * (size_t)q + 1]; s[2] = u.oz;
    d[0] = u.xy[2 * (size_t)p]; d[1] = u.xy[2 * (size_t)p + 1]; d[2] = u.oz;
}

__device__ __forceinline__ bool walk_ok(const FsRmUpdate &u, int32_t e)
{
    return fs_ru_connectable(u.seg_ok[e], u.seg_hit[e], u.seg_unknown[e], u.unknown_limit);
}

__device__ __forceinline__ bool listed(const FsRmUpdate &u, int32_t a, int32_t b)
{
    if (a >= u.n_old) return false;
    for (int32_t j = u.row[a]; j < u.row[a + 1]; ++j)
        if (u.col[j] == b) return true;
    return false;
}

__global__ __launch_bounds__(kBlock) void ru_flag_kernel(const FsRmUpdate u, int32_t total)
{
    const int32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int32_t r = u.cand_rank[e], p = u.owner[r], q = u.cand[e];
    const bool linked = listed(u, p, q) || listed(u, q, p);
    int32_t rq = u.rank_of[q];
    if (rq > u.n) rq = -1;
    bool conn_pq = false;
    if (rq >= 0 && rq < r)
        for (int32_t f = u.cand_off[rq]; f < u.cand_off[rq + 1]; ++f)
            if (u.cand[f] == p) { conn_pq = walk_ok(u, f); break; }
    u.flag[e] = fs_ru_inserted(linked, walk_ok(u, e), r, rq, conn_pq) ? 1 : 0;
}

__global__ __launch_bounds__(kBlock) void ru_pairs_kernel(const FsRmUpdate u, int32_t total)
{
    const int32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e == 0) u.hdr[FS_RU_H_INSERTED] = u.flag_off[total];
    if (e >= total || !u.flag[e]) return;
    const size_t o = (size_t)u.flag_off[e];
    u.pairs[2 * o] = u.owner[u.cand_rank[e]];
    u.pairs[2 * o + 1] = u.cand[e];
}

inline dim3 lanes_for(int64_t n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); }
inline dim3 waves_for(int64_t n) { return lanes_for(n * kWave); }

}  // namespace

hipError_t fs_launch_ru_nodes(const FsRmUpdate &u, hipStream_t s)
{
    if (u.n > 0) hipLaunchKernelGGL(ru_screen_kernel, waves_for(u.n), dim3(kBlock), 0, s, u);
    hipLaunchKernelGGL(ru_keep_kernel, dim3(1), dim3(kOne), 0, s, u);
    return hipGetLastError();
}

hipError_t fs_launch_ru_owners(const FsRmUpdate &u, hipStream_t s)
{
    const int64_t m = (int64_t)u.n + 1;
    hipLaunchKernelGGL(ru_closest_kernel, waves_for(m), dim3(kBlock), 0, s, u);
    hipLaunchKernelGGL(ru_owner_kernel, dim3(1), dim3(kOne), 0, s, u);
    hipLaunchKernelGGL(ru_cand_kernel, waves_for(m), dim3(kBlock), 0, s, u, 0);
    return fs_launch_rm_scan(u.cand_count, (int32_t)m, u.cand_off, s);
}

hipError_t fs_launch_ru_candidates(const FsRmUpdate &u, int32_t total, hipStream_t s)
{
    if (total <= 0) return hipSuccess;
    hipLaunchKernelGGL(ru_cand_kernel, waves_for((int64_t)u.n + 1), dim3(kBlock), 0, s, u, 1);
    hipLaunchKernelGGL(ru_place_kernel, lanes_for(total), dim3(kBlock), 0, s, u, total);
    return hipGetLastError();
}

hipError_t fs_launch_ru_insert(const FsRmUpdate &u, int32_t total, hipStream_t s)
{
    if (total <= 0) return hipSuccess;
    hipLaunchKernelGGL(ru_flag_kernel, lanes_for(total), dim3(kBlock), 0, s, u, total);
    const hipError_t e = fs_launch_rm_scan(u.flag, total, u.flag_off, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ru_pairs_kernel, lanes_for(total), dim3(kBlock), 0, s, u, total);
    return hipGetLastError();
}
