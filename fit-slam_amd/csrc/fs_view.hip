// fs_view.hip — which landmarks does each pose see?  (fs_landmarks_in_view)
//
// Stands in for the GetLandmarksInView round trip of isPoseSafe (FIP/src/fisher_information/FisherInfoManager.cpp:52-88): the
// reference asks the SLAM process for the map points a pose sees and gets them back in the pose's frame.  Here the cloud is the
// one fs_upload_landmarks staged, the rule is fs_set_fim_params' predicate (fs_view.h) — with fs_set_occlusion enabled also the
// line of sight of fs_walk.h — and the answer is a CSR list per pose in ascending upload index.
//   mark   — one wave per (pose, group of chunks): the staged spheres against the range sphere (conservative), then the exact
//            transform and predicate on the 64 landmarks of every accepted chunk; a visible lane ORs bit perm[slot] into the
//            pose's mask of ceil(m / 32) words.  OR is associative and commutative: no pose needs a single owner, and the mask —
//            hence everything below — does not depend on the staged order.
//   count  — one workgroup per pose adds the popcounts of its words; one workgroup scans the round's counts into `offsets`,
//            carrying on from the round before.
//   emit   — one workgroup per pose walks its words; a block prefix of the popcounts ranks every set bit; the entry goes to
//            out[offsets[pose] + rank] when that is below max_total.  index = the bit's position, xyz by the inverse permutation,
//            p_camera by the same fixed-order transform, table_value from the dense lattice (what fs_lookup_query mirrors).
#include "fs_internal.h"
#include "fs_walk.h"
#include "fs_view.h"

namespace {

__global__ void fs_view_keep_perm_kernel(const int32_t *__restrict__ src, int32_t n_usable, int32_t padded, int32_t m,
                                         int32_t *__restrict__ keep, int32_t *__restrict__ inv)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= padded) return;
    int32_t i;
    if (src) {
        i = p < n_usable ? src[p] : -1;
        keep[p] = i;
    } else {
        i = keep[p];
    }
    if ((uint32_t)i < (uint32_t)m) inv[i] = p;
}

__global__ __launch_bounds__(256)
void fs_view_mark_kernel(const FsViewArgs a)
{
    const int lane = threadIdx.x & 63;
    const int groups = (a.n_chunks + a.group - 1) / a.group;
    const long long item = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    if (item >= (long long)a.n_round * groups) return;
    const int pr = (int)(item / groups), grp = (int)(item % groups);
    float Rt[12];
    {
        const float *src = a.Rt + 12 * (size_t)(a.pose_lo + pr);
#pragma unroll
        for (int k = 0; k < 12; ++k) Rt[k] = src[k];
    }
    // ---- cull: lane l < group holds chunk grp * group + l.  The conservative range test of the FIM worker's cull (fs_fim.hip,
    // cull_one): reach * reach - d2 >= 0 with the sphere's safety margin in reach; an empty chunk's radius is -1e30
    bool accept = false;
    {
        const int j = grp * a.group + lane;
        if (lane < a.group && j < a.n_chunks) {
            if (!a.cull) accept = true;
            else {
                const float4 s = *reinterpret_cast<const float4 *>(a.spheres + 4 * (size_t)j);
                const float dx = s.x - Rt[9], dy = s.y - Rt[10], dz = s.z - Rt[11];
                const float d2 = dx * dx + dy * dy + dz * dz;
                const float reach = a.max_dist_f + s.w;
                accept = fminf(reach, reach * reach - d2) >= 0.0f;
            }
        }
    }
    unsigned long long todo = __ballot(accept);
    const FsViewVis vis_p{a.maxd2, a.cos2, a.cone_mode};
    uint32_t *mask = a.mask + (size_t)pr * (size_t)a.words;
    while (todo != 0ull) {
        const int b = __builtin_ctzll(todo);
        todo &= todo - 1ull;
        const int slot = (grp * a.group + b) * FS_CHUNK + lane;      // < n_chunks * 64: the arrays are padded to whole chunks
        const float wx = a.lx[slot], wy = a.ly[slot], wz = a.lz[slot];
        float px, py, pz;
        bool vis = fs_view_transform_visible(Rt, vis_p, wx, wy, wz, px, py, pz);
        if (a.occluded && vis)
            vis = !line_of_sight(a.occ_grid, (double)Rt[9], (double)Rt[10], (double)Rt[11], (double)wx, (double)wy, (double)wz,
                                 a.occ_min, a.occ_max, a.occ_margin).blocked;
        if (vis) {
            const int32_t i = a.perm[slot];
            if ((uint32_t)i < (uint32_t)a.m) atomicOr(mask + (i >> 5), 1u << (i & 31));     // (a sentinel never passes; -1 is no bit)
        }
    }
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
void fs_view_count_kernel(const FsViewArgs a)
{
    __shared__ int s_wave[4];
    const int pr = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t *mask = a.mask + (size_t)pr * (size_t)a.words;
    int c = 0;
    for (int w = tid; w < a.words; w += 256) c += __popc(mask[w]);
    c = wave_inclusive_sum(c, lane);
    if (lane == 63) s_wave[wave] = c;
    __syncthreads();
    if (tid == 0) a.counts[pr] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}

// offsets[pose_lo + 1 + i] = offsets[pose_lo] + counts[0] + .. + counts[i]: one workgroup, tiles of 1024 counts with a carry
__global__ __launch_bounds__(1024)
void fs_view_scan_kernel(const FsViewArgs a)
{
    __shared__ long long s_wave[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long carry = a.offsets[a.pose_lo];
    for (int i0 = 0; i0 < a.n_round; i0 += 1024) {
        const int i = i0 + tid;
        long long v = i < a.n_round ? (long long)a.counts[i] : 0ll;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const long long t = __shfl_up(v, d);
            if (lane >= d) v += t;
        }
        if (lane == 63) s_wave[wave] = v;
        __syncthreads();
        long long before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) { before += k < wave ? s_wave[k] : 0ll; total += s_wave[k]; }
        if (i < a.n_round) a.offsets[(size_t)a.pose_lo + 1 + (size_t)i] = carry + before + v;
        carry += total;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256)
void fs_view_emit_kernel(const FsViewArgs a)
{
    __shared__ int s_wave[4];
    const int pr = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pose = a.pose_lo + pr;
    const long long base = a.offsets[pose];
    if (base >= a.max_total) return;                              // nothing of this pose is stored (uniform)
    const uint32_t *mask = a.mask + (size_t)pr * (size_t)a.words;
    float Rt[12];
    {
        const float *src = a.Rt + 12 * (size_t)pose;
#pragma unroll
        for (int k = 0; k < 12; ++k) Rt[k] = src[k];
    }
    const FsViewVis vis_p{a.maxd2, a.cos2, a.cone_mode};
    const float nan = __uint_as_float(0x7FC00000u);
    long long run = base;                                         // where the tile's first entry goes
    for (int w0 = 0; w0 < a.words; w0 += 256) {
        const int w = w0 + tid;
        uint32_t bits = w < a.words ? mask[w] : 0u;
        const int c = __popc(bits);
        const int incl = wave_inclusive_sum(c, lane);
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { before += k < wave ? s_wave[k] : 0; total += s_wave[k]; }
        long long pos = run + before + (incl - c);
        while (bits != 0u && pos < a.max_total) {
            const int i = w * 32 + (__ffs((int)bits) - 1);
            bits &= bits - 1u;
            const int32_t slot = a.inv[i];                        // (i < m: only landmarks set bits)
            fs_view_landmark e;
            e.index = i;
            e.p_camera[0] = e.p_camera[1] = e.p_camera[2] = nan;
            e.table_value = nan;
            if ((uint32_t)slot < (uint32_t)(a.n_chunks * FS_CHUNK)) {
                float px, py, pz;
                (void)fs_view_transform_visible(Rt, vis_p, a.lx[slot], a.ly[slot], a.lz[slot], px, py, pz);
                e.p_camera[0] = px; e.p_camera[1] = py; e.p_camera[2] = pz;
                int ix, iy, iz;
                if (fs_view_table_cell(a, px, py, pz, ix, iy, iz))
                    e.table_value = a.table[((size_t)ix * (size_t)a.ty + (size_t)iy) * (size_t)a.tz + (size_t)iz];
            }
            a.out[pos] = e;
            ++pos;
        }
        run += total;
        __syncthreads();                                          // s_wave is written again by the next tile
        if (run >= a.max_total) break;                            // (uniform: everything further on lies beyond the capacity)
    }
}

}  // namespace

hipError_t fs_view_keep_perm(const int32_t *d_src, int32_t n_usable, int32_t padded, int32_t m, int32_t *d_keep, int32_t *d_inv, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(d_inv, 0xFF, sizeof(int32_t) * (size_t)(m > 0 ? m : 1), s);      // -1: unusable
    if (e != hipSuccess) return e;
    if (padded <= 0) return hipSuccess;
    hipLaunchKernelGGL(fs_view_keep_perm_kernel, dim3((padded + 255) / 256), dim3(256), 0, s, d_src, n_usable, padded, m, d_keep, d_inv);
    return hipGetLastError();
}

hipError_t fs_launch_view_mark(const FsViewArgs &a, hipStream_t s)
{
    const long long groups = (a.n_chunks + a.group - 1) / a.group;
    const long long items = (long long)a.n_round * groups;
    if (items <= 0) return hipSuccess;
    if ((items + 3) / 4 > 0x7FFFFFFFll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fs_view_mark_kernel, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t fs_launch_view_count(const FsViewArgs &a, hipStream_t s)
{
    if (a.n_round <= 0) return hipSuccess;
    hipLaunchKernelGGL(fs_view_count_kernel, dim3(a.n_round), dim3(256), 0, s, a);
    hipLaunchKernelGGL(fs_view_scan_kernel, dim3(1), dim3(1024), 0, s, a);
    return hipGetLastError();
}

hipError_t fs_launch_view_emit(const FsViewArgs &a, hipStream_t s)
{
    if (a.n_round <= 0) return hipSuccess;
    hipLaunchKernelGGL(fs_view_emit_kernel, dim3(a.n_round), dim3(256), 0, s, a);
    return hipGetLastError();
}
