// fs_pathinfo.hip — the way points of every planned path and their per-frontier Fisher-information columns
// (fs_plan_paths_information).
//
// The reference scored a planned path in two places.  FrontierCostCalculator::setPlanForFrontier (DEP/src/CostCalculator.cpp:302-366,
// 382-390) walks the path from the robot end, cuts a way point once more than (int)(1.5 / resolution) points have gone by (:328),
// turns it towards the point 10 further on (:332, getRelativePoseGivenTwoPoints), adds that pose's information where it is
// positive (:359-363) and stores information_for_path / number_of_wayp (:382-390).  That block is commented out ("moved to FRM");
// its successor is isPoseSafe(point_from, point_to) (FIP/src/fisher_information/FisherInfoManager.cpp:31-37) over consecutive
// path points (FullPathOptimizer::isPathSafe, DEP/src/FullPathOptimizer.cpp:308-340): the lookup scalar info_ref against the
// threshold of FisherInfoBTPlugin.cpp:20.  Here: the sampling of the first, the scalar of the second.
//
// Kernels, in stream order (the FIM worker of fs_fim.hip runs between `prepare` and `finish`, on the records `prepare` wrote):
//   count      one lane per frontier: way points = len / (s + 1)                 -> exclusive scan (rocPRIM) -> offsets, total
//   waypoints  one lane per way point: the two path points -> key = from cell * cells + to cell, the pose7 of the dump
//   (sort by key, rocPRIM)  heads  (inclusive scan, rocPRIM)
//   records    one lane per sorted way point: its pose's slot; the head of a run of equal keys writes the pose record
//   finish     one lane per frontier: the way points' values in order -> mean, minimum, first unsafe way point; the value dump
// Launches are sized by `bound`, the room the host made (it does not know the total yet); lanes beyond the total only pad the sort.
//
// The same route scores the legs of roadmap routes (fs_roadmap_routes; FsPathInfoArgs::node_xy set): a "frontier" is
// a node list, its way point k the leg (node k, node k + 1) — isPathSafe's isPoseSafe(point_from, point_to) over consecutive route
// nodes — and the key a node pair instead of a cell pair.  Only `count`, `waypoints` and the pose of a key differ.
#include "fs_internal.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <cmath>

namespace {

constexpr uint64_t kPadKey = ~0ull;       // sorts behind every real key (real keys are below cells^2 < 2^62)

__global__ void pathinfo_count_kernel(FsPathInfoArgs a)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f > a.n) return;
    int32_t cnt = 0;
    if (f < a.n && a.node_xy) cnt = a.list_len[f] > 0 ? a.list_len[f] - 1 : 0;
    else if (f < a.n && a.achievable[f]) cnt = (int32_t)((int64_t)a.path_length[f] / a.step);
    a.count[f] = cnt;                     // (count[n] = 0: the scan's last output is the total)
}

// the cell the reference's mapToWorld(unsigned, unsigned) reads out of a path point: truncation, as path_length_m's
__device__ __forceinline__ uint32_t point_cell(float v) { return (uint32_t)(int64_t)v; }

// getRelativePoseGivenTwoPoints: position = from, yaw = atan2(to - from), orientationAroundZAxis
__device__ void pose_of_points(double from_x, double from_y, double to_x, double to_y, double pose7[7])
{
    const double yaw = atan2(to_y - from_y, to_x - from_x);
    const double half = yaw * 0.5;
    pose7[0] = from_x; pose7[1] = from_y; pose7[2] = 0.0;
    pose7[3] = 0.0; pose7[4] = 0.0; pose7[5] = sin(half); pose7[6] = cos(half);
}

// ... on the centres of two cells
__device__ void pose_of_cells(const FsPathInfoArgs &a, uint32_t fx, uint32_t fy, uint32_t tx, uint32_t ty, double pose7[7])
{
    const double from_x = a.ox + ((double)fx + 0.5) * a.res, from_y = a.oy + ((double)fy + 0.5) * a.res;
    const double to_x = a.ox + ((double)tx + 0.5) * a.res, to_y = a.oy + ((double)ty + 0.5) * a.res;
    pose_of_points(from_x, from_y, to_x, to_y, pose7);
}

// ... on two roadmap nodes
__device__ void pose_of_nodes(const FsPathInfoArgs &a, int32_t from, int32_t to, double pose7[7])
{
    pose_of_points(a.node_xy[2 * from], a.node_xy[2 * from + 1], a.node_xy[2 * to], a.node_xy[2 * to + 1], pose7);
}

// the pose a key stands for: (from cell, to cell) of the grid, or (from node, to node) of the roadmap
__device__ void pose_of_key(const FsPathInfoArgs &a, uint64_t key, double pose7[7])
{
    if (a.node_xy) {
        pose_of_nodes(a, (int32_t)(key / (uint64_t)a.n_nodes), (int32_t)(key % (uint64_t)a.n_nodes), pose7);
        return;
    }
    const uint64_t cells = (uint64_t)a.nx * (uint64_t)a.ny;
    const uint64_t from = key / cells, to = key % cells;
    pose_of_cells(a, (uint32_t)(from % a.nx), (uint32_t)(from / a.nx), (uint32_t)(to % a.nx), (uint32_t)(to / a.nx), pose7);
}

// pose_to_rt of fs_capi.hip (getTransformFromPose): float translation, Eigen::Quaternionf -> rotation
__device__ void pose_record(const double pose7[7], float *Rt)
{
    const float x = (float)pose7[3], y = (float)pose7[4], z = (float)pose7[5], w = (float)pose7[6];
    const float tx = 2.0f * x, ty = 2.0f * y, tz = 2.0f * z;
    const float twx = tx * w, twy = ty * w, twz = tz * w;
    const float txx = tx * x, txy = ty * x, txz = tz * x;
    const float tyy = ty * y, tyz = tz * y, tzz = tz * z;
    Rt[0] = 1.0f - (tyy + tzz); Rt[1] = txy - twz;          Rt[2] = txz + twy;
    Rt[3] = txy + twz;          Rt[4] = 1.0f - (txx + tzz); Rt[5] = tyz - twx;
    Rt[6] = txz - twy;          Rt[7] = tyz + twx;          Rt[8] = 1.0f - (txx + tyy);
    Rt[9] = (float)pose7[0]; Rt[10] = (float)pose7[1]; Rt[11] = (float)pose7[2];
}

__global__ void pathinfo_waypoints_kernel(FsPathInfoArgs a)
{
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= a.bound) return;
    const int64_t total = a.offset[a.n];
    if (w == 0 && !a.dedup) { a.hdr[0] = total; a.hdr[1] = total; }
    if (w >= total) {
        if (a.dedup) { a.key_in[w] = kPadKey; a.wp_in[w] = (int32_t)w; }
        return;
    }
    // the frontier whose way points hold w: the last f with offset[f] <= w (frontiers without way points share their successor's offset)
    int lo = 0, hi = a.n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.offset[mid] <= w) lo = mid; else hi = mid;
    }
    const int f = lo;
    const int64_t k = w - a.offset[f];
    uint64_t key;
    if (a.node_xy) {
        const int32_t *L = a.list + a.list_off[f];
        key = (uint64_t)L[k] * (uint64_t)a.n_nodes + (uint64_t)L[k + 1];
    } else {
        const int64_t len = (int64_t)a.path_length[f];
        const int64_t j = len - (k + 1) * a.step;                      // in [0, len - step]: k < len / step
        const int64_t jt = j > a.lookahead ? j - a.lookahead : 0;
        const float *px = a.path + (int64_t)f * 2 * a.max_cycles, *py = px + a.max_cycles;
        const uint32_t fx = point_cell(px[j]), fy = point_cell(py[j]), tx = point_cell(px[jt]), ty = point_cell(py[jt]);
        const uint64_t cells = (uint64_t)a.nx * (uint64_t)a.ny;
        key = ((uint64_t)fy * a.nx + fx) * cells + ((uint64_t)ty * a.nx + tx);
    }
    double pose7[7];
    if (a.pose7 || !a.dedup) pose_of_key(a, key, pose7);
    if (a.pose7)
        for (int q = 0; q < 7; ++q) a.pose7[w * 7 + q] = pose7[q];
    if (a.dedup) {
        a.key_in[w] = key;
        a.wp_in[w] = (int32_t)w;
    } else {
        a.slot[w] = (int32_t)w;
        pose_record(pose7, a.rt + w * 12);
    }
}

__global__ void pathinfo_heads_kernel(FsPathInfoArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.bound) return;
    const uint64_t key = a.key_out[i];
    a.head[i] = (key != kPadKey && (i == 0 || a.key_out[i - 1] != key)) ? 1 : 0;
}

__global__ void pathinfo_records_kernel(FsPathInfoArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.bound) return;
    if (i == a.bound - 1) { a.hdr[0] = a.offset[a.n]; a.hdr[1] = a.rank[i]; }
    const uint64_t key = a.key_out[i];
    if (key == kPadKey) return;
    const int32_t id = a.rank[i] - 1;
    a.slot[a.wp_out[i]] = id;
    if (!a.head[i]) return;
    double pose7[7];
    pose_of_key(a, key, pose7);
    pose_record(pose7, a.rt + (int64_t)id * 12);
}

// CostCalculator.cpp:359-363, 382-390 on the way points of frontier f in robot -> frontier order: one lane, one fixed order, no
// atomics — the columns are a function of the values alone
__global__ void pathinfo_finish_kernel(FsPathInfoArgs a)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= a.n) return;
    const int32_t lo = a.offset[f], hi = a.offset[f + 1];
    double sum = 0.0;
    float mn = INFINITY;
    int32_t unsafe = -1;
    for (int32_t w = lo; w < hi; ++w) {
        const float v = a.info[a.slot[w]];
        if (a.wp_info) a.wp_info[w] = v;
        if (v > 0) sum += (double)v;
        mn = fminf(mn, v);
        if (unsafe < 0 && !((double)v > a.fi_threshold)) unsafe = w - lo;
    }
    a.info_mean[f] = hi > lo ? sum / (double)(hi - lo) : 0.0;
    a.info_min[f] = mn;
    a.first_unsafe[f] = unsafe;
}

int key_bits(const FsPathInfoArgs &a)
{
    const uint64_t cells = a.node_xy ? (uint64_t)a.n_nodes : (uint64_t)a.nx * (uint64_t)a.ny;
    const uint64_t top = cells * cells - 1;     // (the pad key has every bit set: it must stay behind whatever the sort looks at)
    int bits = 1;
    while (bits < 64 && (top >> bits) != 0) ++bits;
    return bits < 64 ? bits + 1 : 64;
}

}  // namespace

size_t fs_pathinfo_temp_bytes(const FsPathInfoArgs &a, int64_t bound, hipStream_t s)
{
    size_t scan_n = 0, sort = 0, scan_w = 0;
    if (rocprim::exclusive_scan(nullptr, scan_n, (int32_t *)nullptr, (int32_t *)nullptr, 0, (size_t)a.n + 1, rocprim::plus<int32_t>(), s) != hipSuccess) return 0;
    if (bound > 0) {
        if (rocprim::radix_sort_pairs(nullptr, sort, (uint64_t *)nullptr, (uint64_t *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr, (size_t)bound, 0,
                                      key_bits(a), s) != hipSuccess)
            return 0;
        if (rocprim::inclusive_scan(nullptr, scan_w, (int32_t *)nullptr, (int32_t *)nullptr, (size_t)bound, rocprim::plus<int32_t>(), s) != hipSuccess) return 0;
    }
    return std::max(std::max(scan_n, sort), scan_w) + 256;
}

hipError_t fs_launch_pathinfo_offsets(const FsPathInfoArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(pathinfo_count_kernel, dim3((unsigned)((a.n + 1 + 255) / 256)), dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    size_t bytes = a.temp_bytes;
    return rocprim::exclusive_scan(a.temp, bytes, a.count, a.offset, 0, (size_t)a.n + 1, rocprim::plus<int32_t>(), s);
}

hipError_t fs_launch_pathinfo_prepare(const FsPathInfoArgs &a, hipStream_t s)
{
    if (a.bound <= 0) return hipSuccess;
    const dim3 grid((unsigned)((a.bound + 255) / 256)), block(256);
    hipLaunchKernelGGL(pathinfo_waypoints_kernel, grid, block, 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !a.dedup) return e;
    size_t bytes = a.temp_bytes;
    e = rocprim::radix_sort_pairs(a.temp, bytes, a.key_in, a.key_out, a.wp_in, a.wp_out, (size_t)a.bound, 0, key_bits(a), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pathinfo_heads_kernel, grid, block, 0, s, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    bytes = a.temp_bytes;
    e = rocprim::inclusive_scan(a.temp, bytes, a.head, a.rank, (size_t)a.bound, rocprim::plus<int32_t>(), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pathinfo_records_kernel, grid, block, 0, s, a);
    return hipGetLastError();
}

hipError_t fs_launch_pathinfo_finish(const FsPathInfoArgs &a, hipStream_t s)
{
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(pathinfo_finish_kernel, dim3((unsigned)((a.n + 63) / 64)), dim3(64), 0, s, a);
    return hipGetLastError();
}
