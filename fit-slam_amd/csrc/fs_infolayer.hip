// fs_infolayer.hip — the information layer on the staged 2-D grid (fs_information_layer): the Fisher information of a
// lattice of poses, reduced over K headings, written into the costmap as traversability costs.  This project's own extension: the
// reference has no such layer (its answer to a path that loses tracking is a keep-out zone after the fact).  The rule is in
// include/fitslam_frontier.h; the values come from the FIM worker of fs_fim.hip, which runs between `records` and `store`.
//
// Kernels, in stream order:
//   anchor   L = 2^ceil(log2(min(s*s, 64))) lanes per block of s x s cells, 64 / L blocks per wavefront: each lane scans its share of
//            the block's cells, key = d2 << 10 | ly << 5 | lx for a writable cell (d2 to the centre cell, ly / lx inside the block:
//            ties to the smaller y, then x), a cross-lane minimum over the L lanes -> anchor, flag
//   (exclusive scan of flag, rocPRIM -> rank; rank[nb] = scored blocks)
//   scatter  one lane per block: list[rank] = block — the scored blocks in block order
//   records  one lane per (scored block, heading) of a batch: the pose record, pose_record's arithmetic of fs_pathinfo.hip
//   store    one workgroup per tile of blocks (64 / s x 16 / s of them, at least 1 per axis): a lane per block reduces its K values,
//            writes info / per_yaw and leaves the cost byte in LDS; then the tile's cells take max(old, cost) where writable, one
//            wave-reduced atomic per wavefront for n_changed
// No trigonometry on the device: the K heading pairs are the host's.
#include "fs_internal.h"

#include <rocprim/device/device_scan.hpp>

#include <cmath>

namespace {

constexpr uint32_t kNoKey = ~0u;
constexpr int kTileCellsX = 64, kTileCellsY = 16;            // the store kernel's tile in cells, for s that divide into it
constexpr int kTileBlocksMax = kTileCellsX * kTileCellsY;    // s == 1

__global__ __launch_bounds__(256)
void infolayer_anchor_kernel(FsInfoLayerArgs a, int lanes_log2)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int L = 1 << lanes_log2;
    const int64_t b = t >> lanes_log2, nb = (int64_t)a.nbx * a.nby;
    const int sub = (int)(t & (L - 1));
    const bool live = b < nb;
    uint32_t key = kNoKey;
    int bx0 = 0, by0 = 0;
    if (live) {
        const int i = (int)(b % a.nbx), j = (int)(b / a.nbx);
        bx0 = a.x0 + i * a.s; by0 = a.y0 + j * a.s;
        const int x1 = a.x0 + a.sx, y1 = a.y0 + a.sy;
        const int w = bx0 + a.s < x1 ? a.s : x1 - bx0, h = by0 + a.s < y1 ? a.s : y1 - by0;
        const int cx = bx0 + a.s / 2 < x1 - 1 ? bx0 + a.s / 2 : x1 - 1, cy = by0 + a.s / 2 < y1 - 1 ? by0 + a.s / 2 : y1 - 1;
        for (int q = sub; q < w * h; q += L) {
            const int ly = q / w, lx = q - ly * w;
            const int x = bx0 + lx, y = by0 + ly;
            if (a.cells[(size_t)y * (size_t)a.nx + (size_t)x] > 252) continue;
            const uint32_t d2 = (uint32_t)((x - cx) * (x - cx) + (y - cy) * (y - cy));
            const uint32_t k = d2 << 10 | (uint32_t)ly << 5 | (uint32_t)lx;
            key = k < key ? k : key;
        }
    }
    for (int d = L >> 1; d >= 1; d >>= 1) {                   // (uniform: every lane of the wavefront takes part)
        const uint32_t o = (uint32_t)__shfl_xor((int)key, d);
        key = o < key ? o : key;
    }
    if (live && sub == 0) {
        a.anchor[b] = key == kNoKey ? -1 : (by0 + (int)(key >> 5 & 31u)) * a.nx + bx0 + (int)(key & 31u);
        a.flag[b] = key == kNoKey ? 0 : 1;
    }
    if (t == 0) a.flag[nb] = 0;                               // (the scan's last output is the total)
}

__global__ void infolayer_scatter_kernel(FsInfoLayerArgs a)
{
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= (int64_t)a.nbx * a.nby) return;
    if (a.flag[b]) a.list[a.rank[b]] = (int32_t)b;
}

// pose_record of fs_pathinfo.hip (pose_to_rt of fs_capi.hip) for the pose (x, y, z, 0, 0, qz, qw): the same float products in the
// same order, so the record equals the one fs_score_fim makes of the dumped pose
__device__ __forceinline__ void lattice_pose_record(double px, double py, double pz, double qz, double qw, float *Rt)
{
    const float x = 0.0f, y = 0.0f, z = (float)qz, w = (float)qw;
    const float tx = 2.0f * x, ty = 2.0f * y, tz = 2.0f * z;
    const float twx = tx * w, twy = ty * w, twz = tz * w;
    const float txx = tx * x, txy = ty * x, txz = tz * x;
    const float tyy = ty * y, tyz = tz * y, tzz = tz * z;
    Rt[0] = 1.0f - (tyy + tzz); Rt[1] = txy - twz;          Rt[2] = txz + twy;
    Rt[3] = txy + twz;          Rt[4] = 1.0f - (txx + tzz); Rt[5] = tyz - twx;
    Rt[6] = txz - twy;          Rt[7] = tyz + twx;          Rt[8] = 1.0f - (txx + tyy);
    Rt[9] = (float)px; Rt[10] = (float)py; Rt[11] = (float)pz;
}

__global__ void infolayer_records_kernel(FsInfoLayerArgs a, int64_t p0, int64_t n, float *rt)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const int64_t p = p0 + q;
    const int32_t cell = a.anchor[a.list[p / a.K]];
    const int k = (int)(p % a.K);
    const int x = cell % a.nx, y = cell / a.nx;
    lattice_pose_record(a.ox + ((double)x + 0.5) * a.res, a.oy + ((double)y + 0.5) * a.res, a.pose_z, a.quat_zw[2 * k], a.quat_zw[2 * k + 1],
                        rt + q * 12);
}

// the cost of a reduced value (the header's step 6): correctly rounded fp64 operations, no contraction (the build's -ffp-contract=off)
__device__ __forceinline__ uint8_t info_cost(float v, double lo, double hi, int max_cost)
{
    double t = (hi - (double)v) / (hi - lo);
    if (!(t > 0.0)) t = 0.0;
    if (t > 1.0) t = 1.0;
    return (uint8_t)((double)max_cost * t);
}

__global__ __launch_bounds__(256)
void infolayer_store_kernel(FsInfoLayerArgs a, int tbx, int tby, int tiles_x)
{
    __shared__ uint8_t cost[kTileBlocksMax];
    const int ti = (int)(blockIdx.x % (unsigned)tiles_x), tj = (int)(blockIdx.x / (unsigned)tiles_x);
    const int64_t nb = (int64_t)a.nbx * a.nby;
    for (int q = threadIdx.x; q < tbx * tby; q += 256) {
        const int i = ti * tbx + q % tbx, j = tj * tby + q / tbx;
        uint8_t c = 0;                                        // (an unscored block, or none: max(old, 0) writes nothing)
        if (i < a.nbx && j < a.nby) {
            const int64_t b = (int64_t)j * a.nbx + i;
            float v = NAN;
            if (a.flag[b]) {
                const float *val = a.val + (int64_t)a.rank[b] * a.K;
                if (a.reduce == FS_INFO_REDUCE_MEAN) {
                    double sum = 0.0;
                    for (int k = 0; k < a.K; ++k) sum += (double)val[k];
                    v = (float)(sum / (double)a.K);
                } else {
                    v = val[0];
                    for (int k = 1; k < a.K; ++k) v = a.reduce == FS_INFO_REDUCE_MIN ? fminf(v, val[k]) : fmaxf(v, val[k]);
                }
                c = info_cost(v, a.info_lo, a.info_hi, a.max_cost);
                if (a.per_yaw)
                    for (int k = 0; k < a.K; ++k) a.per_yaw[(int64_t)k * nb + b] = val[k];
            } else if (a.per_yaw)
                for (int k = 0; k < a.K; ++k) a.per_yaw[(int64_t)k * nb + b] = NAN;
            a.info[b] = v;
        }
        cost[q] = c;
    }
    if (!a.write) return;                                     // (uniform)
    __syncthreads();
    const int tx0 = a.x0 + ti * tbx * a.s, ty0 = a.y0 + tj * tby * a.s;
    const int x1 = a.x0 + a.sx, y1 = a.y0 + a.sy;
    const int tw = tx0 + tbx * a.s < x1 ? tbx * a.s : x1 - tx0, th = ty0 + tby * a.s < y1 ? tby * a.s : y1 - ty0;
    int changed = 0;
    for (int q = threadIdx.x; q < tw * th; q += 256) {
        const int ly = q / tw, lx = q - ly * tw;
        const unsigned c = cost[(ly / a.s) * tbx + lx / a.s];
        if (c == 0u) continue;
        uint8_t *cell = a.cells + (size_t)(ty0 + ly) * (size_t)a.nx + (size_t)(tx0 + lx);
        const unsigned o = *cell;
        if (o <= 252u && c > o) { *cell = (uint8_t)c; ++changed; }
    }
    for (int d = 32; d >= 1; d >>= 1) changed += __shfl_xor(changed, d);
    if ((threadIdx.x & 63) == 0 && changed) atomicAdd(a.n_changed, (unsigned long long)changed);
}

bool args_ok(const FsInfoLayerArgs &a)
{
    return a.nx > 0 && a.ny > 0 && a.sx > 0 && a.sy > 0 && a.x0 >= 0 && a.y0 >= 0 && (long long)a.x0 + a.sx <= a.nx &&
           (long long)a.y0 + a.sy <= a.ny && a.s >= 1 && a.s <= FS_INFO_LAYER_MAX_STRIDE && a.nbx == (a.sx + a.s - 1) / a.s &&
           a.nby == (a.sy + a.s - 1) / a.s && a.K >= 1 && a.K <= FS_INFO_LAYER_MAX_YAW;
}

}  // namespace

size_t fs_infolayer_temp_bytes(int64_t nb, hipStream_t s)
{
    size_t bytes = 0;
    if (rocprim::exclusive_scan(nullptr, bytes, (int32_t *)nullptr, (int32_t *)nullptr, 0, (size_t)nb + 1, rocprim::plus<int32_t>(), s) != hipSuccess) return 0;
    return bytes + 256;
}

hipError_t fs_launch_infolayer_anchors(const FsInfoLayerArgs &a, hipStream_t s)
{
    if (!args_ok(a)) return hipErrorInvalidValue;
    int lanes_log2 = 0;
    while (lanes_log2 < 6 && (1 << lanes_log2) < a.s * a.s) ++lanes_log2;
    const int64_t nb = (int64_t)a.nbx * a.nby;
    const int64_t blocks = ((nb << lanes_log2) + 255) / 256;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(infolayer_anchor_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a, lanes_log2);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    size_t bytes = a.temp_bytes;
    e = rocprim::exclusive_scan(a.temp, bytes, a.flag, a.rank, 0, (size_t)nb + 1, rocprim::plus<int32_t>(), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(infolayer_scatter_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t fs_launch_infolayer_records(const FsInfoLayerArgs &a, int64_t p0, int64_t n, float *rt, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    if (!args_ok(a) || p0 < 0 || (n + 255) / 256 > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(infolayer_records_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a, p0, n, rt);
    return hipGetLastError();
}

hipError_t fs_launch_infolayer_store(const FsInfoLayerArgs &a, hipStream_t s)
{
    if (!args_ok(a) || a.max_cost < 1 || a.max_cost > 252) return hipErrorInvalidValue;
    const int tbx = kTileCellsX / a.s > 0 ? kTileCellsX / a.s : 1, tby = kTileCellsY / a.s > 0 ? kTileCellsY / a.s : 1;
    const int tiles_x = (a.nbx + tbx - 1) / tbx;
    const long long blocks = (long long)tiles_x * ((a.nby + tby - 1) / tby);
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(infolayer_store_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a, tbx, tby, tiles_x);
    return hipGetLastError();
}
