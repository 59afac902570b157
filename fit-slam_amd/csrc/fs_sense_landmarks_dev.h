// fs_sense_landmarks_dev.h — device code the landmark sensor (fs_sense_landmarks.hip) shares with the drive that
// senses landmarks on the way (fs_drive_slam.hip): one wave's share of a sweep of the WORLD cloud.  Device code
// only; included after fs_internal.h.
#ifndef FS_SENSE_LANDMARKS_DEV_H_
#define FS_SENSE_LANDMARKS_DEV_H_

#include "fs_internal.h"
#include "fs_walk.h"
#include "fs_view.h"

namespace {

// the conservative range test of a chunk sphere s = (centre, radius + safety margin) against the pose at (tx, ty, tz) with culling
// reach max_dist_f (fs_view_mark_kernel's test; an empty chunk's radius is -1e30)
__device__ __forceinline__ bool chunk_in_reach(const float4 s, float tx, float ty, float tz, float max_dist_f)
{
    const float dx = s.x - tx, dy = s.y - ty, dz = s.z - tz;
    const float d2 = dx * dx + dy * dy + dz * dz;
    const float reach = max_dist_f + s.w;
    return fminf(reach, reach * reach - d2) >= 0.0f;
}

// Chunk group grp (a.group chunks) of the world cloud from the pose record Rt_src [12], by one whole wave: the spheres against the
// range sphere, then the exact transform and predicate (fs_view.h) on the 64 landmarks of every accepted chunk and — with a.los —
// the walk of fs_walk.h through the WORLD grid for the lanes the predicate accepts.  A seeing lane adds 1 to its landmark's
// counter.  Returns the landmarks seen (wave-uniform).
__device__ __forceinline__ int landmark_sweep_group(const FsLandmarkSenseArgs &a, const float *Rt_src, int grp, int lane)
{
    float Rt[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) Rt[k] = Rt_src[k];
    // ---- cull: lane l < group holds chunk grp * group + l
    bool accept = false;
    {
        const int j = grp * a.group + lane;
        if (lane < a.group && j < a.n_chunks)
            accept = !a.cull || chunk_in_reach(*reinterpret_cast<const float4 *>(a.spheres + 4 * (size_t)j), Rt[9], Rt[10], Rt[11], a.max_dist_f);
    }
    unsigned long long todo = __ballot(accept);
    const FsViewVis vis_p{a.maxd2, a.cos2, a.cone_mode};
    int seen = 0;                                                    // (wave-uniform)
    while (todo != 0ull) {
        const int b = __builtin_ctzll(todo);
        todo &= todo - 1ull;
        const int slot = (grp * a.group + b) * FS_CHUNK + lane;      // < n_chunks * 64: the arrays are padded to whole chunks
        const float wx = a.lx[slot], wy = a.ly[slot], wz = a.lz[slot];
        float px, py, pz;
        bool vis = fs_view_transform_visible(Rt, vis_p, wx, wy, wz, px, py, pz);
        const int32_t i = a.perm[slot];
        vis = vis && (uint32_t)i < (uint32_t)a.m_world;              // (a sentinel never passes the predicate; -1 names no landmark)
        if (a.los && vis)
            vis = !line_of_sight(a.world, (double)Rt[9], (double)Rt[10], (double)Rt[11], (double)wx, (double)wy, (double)wz,
                                 a.occ_min, a.occ_max, a.occ_margin).blocked;
        if (vis) atomicAdd(a.views + i, 1u);
        seen += __popcll(__ballot(vis));
    }
    return seen;
}

}  // namespace

#endif  // FS_SENSE_LANDMARKS_DEV_H_
