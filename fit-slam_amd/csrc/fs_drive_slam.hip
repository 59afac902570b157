// fs_drive_slam.hip — a drive that asks at every station whether SLAM would still be tracking (fs_drive_slam).
//
// Stands in for EvaluateFisherInformation, the behaviour-tree node that calls isPoseSafe at the robot's current pose while it is
// under way (FIP/src/fisher_information/FisherInfoManager.cpp:52-100): an unsafe pose ends the goal.  The drive is
// fs_drive's (fs_drive.hip); after its step and merge launches of step k the host enqueues, still without waiting,
//   sweep — one wavefront per (robot, group of chunks) of the WORLD cloud: a robot that did not sweep in this step returns at
//           once, the others run the landmark sensor's own body (fs_sense_landmarks_dev.h) from their station-k pose.
//   (fs_launch_landmark_flags: counters >= min_views -> discovered, for all robots' sightings of the step)
//   info  — FS_GATE_SLABS workgroups per robot.  The pose is scored straight from the world cloud: chunk spheres against the
//           range sphere, the exact fp32 transform and predicate of fs_view.h under fs_set_fim_params' volume, the discovered
//           flag through perm, the voxel's cell in the lookup table (fs_view_table_cell), with occlusion the line of sight on
//           the STAGED grid.  Slab w owns the voxels whose table x index is w modulo FS_GATE_SLABS — whole voxels, alternating
//           slabs — and counts the landmarks per voxel in an LDS hash table (tier 1).  A slab with more voxels than the table
//           takes counts again (tier 2) in passes over ranges of 2 * FS_GATE_SLOTS consecutive slab-local voxel indices,
//           directly indexed: no pass can run full.  Either way the slab's share is the sum over its occupied voxels of
//           table value * (factor[1] + .. + factor[count]) in fp64, reduced over the workgroup.
//   gate  — one lane per robot, in place of fs_drive's goal launch: the slabs' shares in slab order, the station's outputs, then
//           MAPPED before UNSAFE.
// Every launch ends on its own.  Voxel counts are integers, the order of the fp64 additions inside a slab follows the table's
// slots: the information agrees with fs_score_fim's to rounding, not to the bit (neither does fs_score_fim with itself).
#include "fs_internal.h"
#include "fs_walk.h"
#include "fs_view.h"
#include "fs_sense_dev.h"             // goal_mapped
#include "fs_sense_landmarks_dev.h"   // landmark_sweep_group, chunk_in_reach

#define FS_GATE_THREADS 256
#define FS_GATE_MAX_PROBE 128          // tier 1 gives up (-> tier 2) after this many slots
#define FS_GATE_EMPTY 0xFFFFFFFFu

namespace {

// did robot r sweep in step a.step?  (asked after the step kernel and before the gate: a robot that stopped in the move is no
// longer DRIVING, one without a station k has ARRIVED)
__device__ __forceinline__ bool swept(const FsDriveSlamArgs &a, int r)
{
    return a.state[2 * r] == FS_DRIVE_DRIVING && a.step < a.n_stations[r];
}

__global__ __launch_bounds__(256)
void fs_drive_slam_sweep_kernel(const FsDriveSlamArgs a)
{
    const int lane = threadIdx.x & 63;
    const int groups = (a.sweep.n_chunks + a.sweep.group - 1) / a.sweep.group;
    const long long item = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    if (item >= (long long)a.n_robots * groups) return;
    const int r = (int)(item / groups), grp = (int)(item % groups);
    if (!swept(a, r)) return;
    const size_t at = (size_t)a.station_off[r] + (size_t)a.step;
    const int seen = landmark_sweep_group(a.sweep, a.sweep.Rt + 12 * at, grp, lane);
    if (lane == 0 && seen != 0) atomicAdd(a.sweep.n_in_view + at, seen);
}

// factor[1] + .. + factor[count]: the discount series of one voxel (FisherInfoManager.hpp:102-106; exactly 0 from rank 337 on)
__device__ __forceinline__ double voxel_series(const float *__restrict__ factor, uint32_t count)
{
    const uint32_t n = count < (uint32_t)(FS_FACTOR_N - 1) ? count : (uint32_t)(FS_FACTOR_N - 1);
    double s = 0.0;
    for (uint32_t j = 1; j <= n; ++j) s += (double)factor[j];
    return s;
}

// table value of the slab-local voxel index v of slab `slab`: v = ((ix >> 3) * ty + iy) * tz + iz
__device__ __forceinline__ float slab_table_value(const FsDriveSlamArgs &a, int slab, uint32_t v)
{
    const uint32_t plane = (uint32_t)a.ty * (uint32_t)a.tz;
    const uint32_t q = v / plane;
    return a.table[(size_t)(q * FS_GATE_SLABS + (uint32_t)slab) * plane + (v - q * plane)];
}

// One pass of the workgroup over the world cloud for the pose Rt: every discovered landmark in view whose voxel belongs to `slab`
// is counted — DIRECT false: under its slab-local index in the hash table keys / counts [FS_GATE_SLOTS] (*over = 1 when a lane
// finds no slot); DIRECT true: in counts [index - lo] when that lies below 2 * FS_GATE_SLOTS.  The cheap tests come first, the
// line-of-sight walk last.
template <bool DIRECT>
__device__ __forceinline__ void gate_scan(const FsDriveSlamArgs &a, const float (&Rt)[12], int slab, uint32_t lo, uint32_t *keys, uint32_t *counts,
                                          int *over)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const FsViewVis vis_p{a.maxd2, a.cos2, a.cone_mode};
    const int n_chunks = a.sweep.n_chunks;
    for (int base = wave * 64; base < n_chunks; base += (FS_GATE_THREADS / 64) * 64) {           // (uniform per wave)
        const int j = base + lane;
        bool accept = false;
        if (j < n_chunks)
            accept = !a.cull || chunk_in_reach(*reinterpret_cast<const float4 *>(a.sweep.spheres + 4 * (size_t)j), Rt[9], Rt[10], Rt[11], a.max_dist_f);
        unsigned long long todo = __ballot(accept);
        while (todo != 0ull) {
            const int b = __builtin_ctzll(todo);
            todo &= todo - 1ull;
            const int slot = (base + b) * FS_CHUNK + lane;           // < n_chunks * 64: the arrays are padded to whole chunks
            const float wx = a.sweep.lx[slot], wy = a.sweep.ly[slot], wz = a.sweep.lz[slot];
            float px, py, pz;
            bool vis = fs_view_transform_visible(Rt, vis_p, wx, wy, wz, px, py, pz);
            const int32_t i = a.sweep.perm[slot];
            vis = vis && (uint32_t)i < (uint32_t)a.sweep.m_world && a.flag[(uint32_t)i < (uint32_t)a.sweep.m_world ? i : 0] != 0;
            int ix = 0, iy = 0, iz = 0;
            vis = vis && fs_view_table_cell(a, px, py, pz, ix, iy, iz);
            vis = vis && (ix & (FS_GATE_SLABS - 1)) == slab;
            const uint32_t v = ((uint32_t)(ix >> 3) * (uint32_t)a.ty + (uint32_t)iy) * (uint32_t)a.tz + (uint32_t)iz;
            if (!a.table_full && vis) {                              // a NaN hole of the table is no voxel (missed voxels are skipped)
                const float t = slab_table_value(a, slab, v);
                vis = t == t;
            }
            if (DIRECT) vis = vis && v >= lo && v - lo < 2u * FS_GATE_SLOTS;
            if (a.occluded && vis)
                vis = !line_of_sight(a.staged, (double)Rt[9], (double)Rt[10], (double)Rt[11], (double)wx, (double)wy, (double)wz,
                                     a.occ_min, a.occ_max, a.occ_margin).blocked;
            if (!vis) continue;
            if (DIRECT) {
                atomicAdd(counts + (v - lo), 1u);
            } else {
                uint32_t h = (v * 0x9E3779B1u) >> 21;                // 11 bits: FS_GATE_SLOTS slots
                bool done = false;
                for (int probe = 0; probe < FS_GATE_MAX_PROBE && !done; ++probe) {
                    const uint32_t prev = atomicCAS(keys + h, FS_GATE_EMPTY, v);
                    if (prev == FS_GATE_EMPTY || prev == v) { atomicAdd(counts + h, 1u); done = true; }
                    else h = (h + 1u) & (FS_GATE_SLOTS - 1u);
                }
                if (!done) *over = 1;
            }
        }
    }
}
static_assert(FS_GATE_SLOTS == 2048 && FS_GATE_SLABS == 8, "the hash shift and the slab arithmetic assume 2^11 slots and 2^3 slabs");

__global__ __launch_bounds__(FS_GATE_THREADS)
void fs_drive_slam_info_kernel(const FsDriveSlamArgs a)
{
    __shared__ uint32_t s_tab[2 * FS_GATE_SLOTS];                    // tier 1: keys | counts; tier 2: counts of one range
    __shared__ int s_over;
    __shared__ double s_red[FS_GATE_THREADS / 64][2];
    const int slab = (int)blockIdx.x, r = (int)blockIdx.y, tid = (int)threadIdx.x;
    if (!swept(a, r)) return;                                        // (uniform over the workgroup)
    const size_t at = (size_t)a.station_off[r] + (size_t)a.step;
    float Rt[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) Rt[k] = a.sweep.Rt[12 * at + k];
    uint32_t *keys = s_tab, *counts = s_tab + FS_GATE_SLOTS;
    for (int s = tid; s < FS_GATE_SLOTS; s += FS_GATE_THREADS) { keys[s] = FS_GATE_EMPTY; counts[s] = 0u; }
    if (tid == 0) s_over = 0;
    __syncthreads();
    gate_scan<false>(a, Rt, slab, 0u, keys, counts, &s_over);
    __syncthreads();
    double info = 0.0, nvox = 0.0;
    if (!s_over) {                                                   // (uniform)
        for (int s = tid; s < FS_GATE_SLOTS; s += FS_GATE_THREADS) {
            const uint32_t v = keys[s];
            if (v == FS_GATE_EMPTY) continue;
            info += (double)slab_table_value(a, slab, v) * voxel_series(a.factor, counts[s]);
            nvox += 1.0;
        }
    } else {
        // tier 2: the slab's voxels in ranges of 2 * FS_GATE_SLOTS consecutive indices, each range a pass over the cloud
        if (tid == 0) atomicAdd(a.fallbacks, 1);
        const uint32_t slab_cells = (uint32_t)((a.tx + FS_GATE_SLABS - 1) / FS_GATE_SLABS) * (uint32_t)a.ty * (uint32_t)a.tz;
        for (uint32_t lo = 0; lo < slab_cells; lo += 2u * FS_GATE_SLOTS) {
            __syncthreads();                                         // (the sums of the pass before have been read)
            for (int s = tid; s < 2 * FS_GATE_SLOTS; s += FS_GATE_THREADS) s_tab[s] = 0u;
            __syncthreads();
            gate_scan<true>(a, Rt, slab, lo, nullptr, s_tab, nullptr);
            __syncthreads();
            for (int s = tid; s < 2 * FS_GATE_SLOTS; s += FS_GATE_THREADS) {
                const uint32_t c = s_tab[s];
                if (c == 0u) continue;
                info += (double)slab_table_value(a, slab, lo + (uint32_t)s) * voxel_series(a.factor, c);
                nvox += 1.0;
            }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { info += __shfl_xor(info, d); nvox += __shfl_xor(nvox, d); }
    if ((tid & 63) == 0) { s_red[tid >> 6][0] = info; s_red[tid >> 6][1] = nvox; }
    __syncthreads();
    if (tid == 0) {
        double *out = a.partial + ((size_t)r * FS_GATE_SLABS + (size_t)slab) * 2;
        double i_sum = 0.0, v_sum = 0.0;
#pragma unroll
        for (int w = 0; w < FS_GATE_THREADS / 64; ++w) { i_sum += s_red[w][0]; v_sum += s_red[w][1]; }
        out[0] = i_sum; out[1] = v_sum;
    }
}

__global__ void fs_drive_slam_gate_kernel(const FsDriveSlamArgs a)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.n_robots || !swept(a, r)) return;
    const size_t at = (size_t)a.station_off[r] + (size_t)a.step;
    const double *p = a.partial + (size_t)r * FS_GATE_SLABS * 2;
    double info = 0.0, nvox = 0.0;
    for (int w = 0; w < FS_GATE_SLABS; ++w) { info += p[2 * w]; nvox += p[2 * w + 1]; }
    const float info_f = (float)info;
    a.information[at] = info_f;
    a.voxels[at] = (int)(nvox + 0.5);
    // 4 goal, as fs_drive_goal_kernel; then 5 gate: isPoseSafe's `total > threshold` on the float the call reports
    if (a.stop_when_mapped &&
        goal_mapped(a.staged.cells, a.staged.nx, a.staged.ny, a.staged.ox, a.staged.oy, a.staged.res, a.goal[3 * (size_t)r], a.goal[3 * (size_t)r + 1]))
        a.state[2 * r] = FS_DRIVE_MAPPED;
    else if (a.gate && a.step >= a.gate_first && !((double)info_f > a.threshold))
        a.state[2 * r] = FS_DRIVE_UNSAFE;
}

}  // namespace

hipError_t fs_launch_drive_slam_sweep(const FsDriveSlamArgs &a, hipStream_t s)
{
    const long long groups = (a.sweep.n_chunks + a.sweep.group - 1) / a.sweep.group;
    const long long items = (long long)a.n_robots * groups;
    if (items <= 0) return hipSuccess;
    if ((items + 3) / 4 > 0x7FFFFFFFll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fs_drive_slam_sweep_kernel, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t fs_launch_drive_slam_info(const FsDriveSlamArgs &a, hipStream_t s)
{
    if (a.n_robots <= 0) return hipSuccess;
    if (a.n_robots > 65535) return hipErrorInvalidValue;                       // (gridDim.y; fs_drive's own cap is far below)
    hipLaunchKernelGGL(fs_drive_slam_info_kernel, dim3(FS_GATE_SLABS, (unsigned)a.n_robots), dim3(FS_GATE_THREADS), 0, s, a);
    return hipGetLastError();
}

hipError_t fs_launch_drive_slam_gate(const FsDriveSlamArgs &a, hipStream_t s)
{
    if (a.n_robots <= 0) return hipSuccess;
    hipLaunchKernelGGL(fs_drive_slam_gate_kernel, dim3((unsigned)((a.n_robots + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}
