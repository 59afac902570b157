// fs_view.h — the landmark transform and the visibility predicate as ONE device function, for the kernels that list the landmarks in
// view of a pose (fs_view.hip).  The Fisher-information worker (fs_fim.hip, fim_worker) holds a copy of its own —
// its code objects are what the benchmark times — and tests/test_gpu_landmarks_in_view.py holds the two together: the lists must
// count what fs_score_fim counts.  Device code only; included after fs_internal.h.
#ifndef FS_VIEW_H_
#define FS_VIEW_H_

namespace {

// what the predicate needs of fs_set_fim_params (FsFimArgs' fields of the same names, filled by fill_fim_args)
struct FsViewVis {
    float maxd2;               // (float)(max_dist^2)
    float cos2;                // c * c, c = (float)cos(max_angle)
    int32_t cone_mode;         // 0 disabled, 1 / 3 c >= 0, 2 c < 0
};

// p = R^T (w - t) in fp32 with the operation order fixed by DESIGN.md "FIM accumulate" (the general three-row form), then
// n2 <= maxd2 and the cone in its FS_CONE_ANY form.  Rt = R row-major (9) + t (3).
__device__ __forceinline__ bool fs_view_transform_visible(const float *Rt, const FsViewVis &v, float wx, float wy, float wz,
                                                          float &px, float &py, float &pz)
{
    const float dx = wx - Rt[9], dy = wy - Rt[10], dz = wz - Rt[11];
    px = __fmaf_rn(Rt[0], dx, __fmaf_rn(Rt[3], dy, Rt[6] * dz));
    py = __fmaf_rn(Rt[1], dx, __fmaf_rn(Rt[4], dy, Rt[7] * dz));
    pz = __fmaf_rn(Rt[2], dx, __fmaf_rn(Rt[5], dy, Rt[8] * dz));
    const float n2 = __fmaf_rn(px, px, __fmaf_rn(py, py, pz * pz));
    const float px2 = px * px;
    bool vis = (n2 <= v.maxd2);
    if (v.cone_mode == 1 || v.cone_mode == 3) vis = vis && (px >= 0.0f) && (px2 >= v.cos2 * n2);
    else if (v.cone_mode == 2) vis = vis && ((px >= 0.0f) || (px2 <= v.cos2 * n2));
    return vis;
}

// The dense table's cell of a camera-frame point: round(x * (1 / step)) of getVoxelCoordinate (FisherInfoManager.hpp:119-121) in
// fp64, as fs_lookup_query's host form — what the FIM worker's fp32 fast path (fs_fim.hip, voxel_key) is proven equal to; compared
// as doubles, so no index leaves the range of an integer before it is known to be in the table.  A: any argument struct with
// FsFimArgs' jx0 .. tz and inv_step.  False: the voxel lies outside the table's box.
template <typename A>
__device__ __forceinline__ bool fs_view_table_cell(const A &a, float px, float py, float pz, int &ix, int &iy, int &iz)
{
    const double rx = round((double)px * a.inv_step) - (double)a.jx0;
    const double ry = round((double)py * a.inv_step) - (double)a.jy0;
    const double rz = round((double)pz * a.inv_step) - (double)a.jz0;
    if (!(rx >= 0.0 && rx < (double)a.tx && ry >= 0.0 && ry < (double)a.ty && rz >= 0.0 && rz < (double)a.tz)) return false;
    ix = (int)rx; iy = (int)ry; iz = (int)rz;
    return true;
}

}  // namespace

#endif  // FS_VIEW_H_
