// fs_sense_landmarks.hip — the landmark sensor on a ground-truth cloud (fs_upload_world_landmarks, fs_sense_landmarks; DESIGN.md
// 4.23).  This project's own extension, like fs_sense.hip: in the reference the map points come from the ORB-SLAM3 wrapper, which
// is outside the vendored tree.  A WORLD cloud lives in HBM in a k-d leaf order of its own (fs_cloud.hip) beside one sighting
// counter and one `discovered` flag per landmark; the staged cloud is the discovered part, put in order again on the device.
//   sweep   — one wave per (pose, group of chunks), as fs_view_mark_kernel (landmark_sweep_group, fs_sense_landmarks_dev.h): the
//             world cloud's spheres against the range sphere
//             (conservative), then the exact transform and predicate (fs_view.h) on the 64 landmarks of every accepted chunk and —
//             with line_of_sight — the walk of fs_walk.h through the WORLD grid for the lanes the predicate accepts.  A seeing
//             lane adds 1 to its landmark's counter; the wave adds popcount(ballot) to the pose's n_in_view once.  Integer sums
//             only: nothing depends on the order the device works in, and nobody is "the" discoverer.
//   flags   — one lane per world landmark: counter >= min_views sets the flag for good; per block the discovered landmarks and
//             the usable ones among them (plain stores), and one atomic per block and total: new, discovered, usable.
//   scan    — one workgroup turns the per-block pairs into exclusive offsets.
//   scatter — one lane per world landmark again: a block prefix ranks every discovered landmark; its raw xyz goes to
//             raw_out[rank] (ascending world index) and, when usable, its rank to usable_out — what the cloud ordering starts from.
#include "fs_internal.h"
#include "fs_sense_landmarks_dev.h"   // one wave's share of a sweep, shared with fs_drive_slam.hip

namespace {

__global__ __launch_bounds__(256)
void fs_sense_landmarks_kernel(const FsLandmarkSenseArgs a)
{
    const int lane = threadIdx.x & 63;
    const int groups = (a.n_chunks + a.group - 1) / a.group;
    const long long item = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    if (item >= (long long)a.n * groups) return;
    const int pose = (int)(item / groups), grp = (int)(item % groups);
    const int seen = landmark_sweep_group(a, a.Rt + 12 * (size_t)pose, grp, lane);
    if (lane == 0 && seen != 0) atomicAdd(a.n_in_view + pose, seen);
}

// as fs_stage_landmarks: finite and within 1e17 m (fabsf of a NaN compares false)
__device__ __forceinline__ bool landmark_usable(const float *p)
{
    return fabsf(p[0]) <= 1.0e17f && fabsf(p[1]) <= 1.0e17f && fabsf(p[2]) <= 1.0e17f;
}

// inclusive sum over the wave's lanes
__device__ __forceinline__ int wave_inclusive_sum(int v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    return v;
}

__global__ __launch_bounds__(256)
void fs_landmark_flags_kernel(const float *__restrict__ raw, const uint32_t *__restrict__ views, uint8_t *__restrict__ flag, int32_t m_world,
                              uint32_t min_views, int32_t *__restrict__ block_counts, int32_t *__restrict__ totals)
{
    __shared__ int s_wave[4][3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = blockIdx.x * 256 + tid;
    bool disc = false, fresh = false, usable = false;
    if (i < m_world) {
        disc = flag[i] != 0;
        if (!disc && views[i] >= min_views) { flag[i] = 1; disc = fresh = true; }
        usable = disc && landmark_usable(raw + 3 * (size_t)i);
    }
    const int n_fresh = __popcll(__ballot(fresh)), n_disc = __popcll(__ballot(disc)), n_usable = __popcll(__ballot(usable));
    if (lane == 0) { s_wave[wave][0] = n_fresh; s_wave[wave][1] = n_disc; s_wave[wave][2] = n_usable; }
    __syncthreads();
    if (tid < 3) {
        const int v = s_wave[0][tid] + s_wave[1][tid] + s_wave[2][tid] + s_wave[3][tid];
        if (tid > 0) block_counts[2 * blockIdx.x + (tid - 1)] = v;
        if (v != 0) atomicAdd(totals + tid, v);
    }
}

// block_off[b] = sum of block_counts[< b], for the two interleaved columns: one workgroup, tiles of 1024 blocks with a carry
__global__ __launch_bounds__(1024)
void fs_landmark_scan_kernel(const int32_t *__restrict__ block_counts, int32_t n_blocks, int32_t *__restrict__ block_off)
{
    __shared__ int s_wave[16][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int carry0 = 0, carry1 = 0;
    for (int b0 = 0; b0 < n_blocks; b0 += 1024) {
        const int b = b0 + tid;
        const int c0 = b < n_blocks ? block_counts[2 * b] : 0, c1 = b < n_blocks ? block_counts[2 * b + 1] : 0;
        const int i0 = wave_inclusive_sum(c0, lane), i1 = wave_inclusive_sum(c1, lane);
        if (lane == 63) { s_wave[wave][0] = i0; s_wave[wave][1] = i1; }
        __syncthreads();
        int before0 = 0, before1 = 0, total0 = 0, total1 = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            before0 += k < wave ? s_wave[k][0] : 0; total0 += s_wave[k][0];
            before1 += k < wave ? s_wave[k][1] : 0; total1 += s_wave[k][1];
        }
        if (b < n_blocks) { block_off[2 * b] = carry0 + before0 + i0 - c0; block_off[2 * b + 1] = carry1 + before1 + i1 - c1; }
        carry0 += total0; carry1 += total1;
        __syncthreads();                                             // s_wave is written again by the next tile
    }
}

__global__ __launch_bounds__(256)
void fs_landmark_scatter_kernel(const float *__restrict__ raw, const uint8_t *__restrict__ flag, int32_t m_world,
                                const int32_t *__restrict__ block_off, int32_t n_disc, int32_t n_usable, float *__restrict__ raw_out,
                                int32_t *__restrict__ usable_out)
{
    __shared__ int s_wave[4][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = blockIdx.x * 256 + tid;
    float x = 0.0f, y = 0.0f, z = 0.0f;
    bool disc = false, usable = false;
    if (i < m_world && flag[i] != 0) {
        const float *p = raw + 3 * (size_t)i;
        x = p[0]; y = p[1]; z = p[2];
        disc = true;
        usable = landmark_usable(p);
    }
    const int d = disc ? 1 : 0, u = usable ? 1 : 0;
    const int id = wave_inclusive_sum(d, lane), iu = wave_inclusive_sum(u, lane);
    if (lane == 63) { s_wave[wave][0] = id; s_wave[wave][1] = iu; }
    __syncthreads();
    int rank = block_off[2 * blockIdx.x] + id - d, urank = block_off[2 * blockIdx.x + 1] + iu - u;
#pragma unroll
    for (int k = 0; k < 4; ++k) { rank += k < wave ? s_wave[k][0] : 0; urank += k < wave ? s_wave[k][1] : 0; }
    // (the counts the host sized the arrays by are the ones these ranks come from; the comparisons cost nothing and keep a
    // disagreement — flags changed between the two kernels — inside the arrays)
    if (disc && (uint32_t)rank < (uint32_t)n_disc) {
        float *q = raw_out + 3 * (size_t)rank;
        q[0] = x; q[1] = y; q[2] = z;
        if (usable && (uint32_t)urank < (uint32_t)n_usable) usable_out[urank] = rank;
    }
}

}  // namespace

hipError_t fs_launch_sense_landmarks(const FsLandmarkSenseArgs &a, hipStream_t s)
{
    const long long groups = (a.n_chunks + a.group - 1) / a.group;
    const long long items = (long long)a.n * groups;
    if (items <= 0) return hipSuccess;
    if ((items + 3) / 4 > 0x7FFFFFFFll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fs_sense_landmarks_kernel, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t fs_launch_landmark_flags(const float *d_raw, const uint32_t *d_views, uint8_t *d_flag, int32_t m_world, uint32_t min_views,
                                    int32_t *d_block_counts, int32_t *d_block_off, int32_t *d_totals, hipStream_t s)
{
    if (m_world <= 0) return hipSuccess;
    const int32_t n_blocks = (m_world + 255) / 256;
    hipLaunchKernelGGL(fs_landmark_flags_kernel, dim3(n_blocks), dim3(256), 0, s, d_raw, d_views, d_flag, m_world, min_views, d_block_counts, d_totals);
    hipLaunchKernelGGL(fs_landmark_scan_kernel, dim3(1), dim3(1024), 0, s, d_block_counts, n_blocks, d_block_off);
    return hipGetLastError();
}

hipError_t fs_launch_landmark_scatter(const float *d_raw, const uint8_t *d_flag, int32_t m_world, const int32_t *d_block_off, int32_t n_disc,
                                      int32_t n_usable, float *d_raw_out, int32_t *d_usable_out, hipStream_t s)
{
    if (m_world <= 0 || n_disc <= 0) return hipSuccess;
    hipLaunchKernelGGL(fs_landmark_scatter_kernel, dim3((m_world + 255) / 256), dim3(256), 0, s, d_raw, d_flag, m_world, d_block_off, n_disc, n_usable,
                       d_raw_out, d_usable_out);
    return hipGetLastError();
}
