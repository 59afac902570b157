// fs_roadmap_kf.hip — the roadmap's key-frame anchors: FrontierRoadMap::mapDataCallback's anchoring of the pending
// nodes and optimizeSHM's re-placement and de-duplication, on the device.
//
// Reference: DEP/src/planners/FrontierRoadmap.cpp — mapDataCallback (:42-130), optimizeSHM (:132-155), populateNodes (:185-252),
// reConstructGraph (:347-408); DEP/src/Helpers.cpp:342-352 (getTransformFromPose).
//
// Anchoring.  One lane per pending node (queue order): its own key-frame cell, else the reference's square search — radius
// (int)(grid_cell_size * m), m = 1, 2, ..., given up past 7, dx outer / dy inner, the FIRST occupied cell in that order.  Every
// id of the cell is a parent; each parent appends T_kf^-1 * (float x, float y, 0) to the record store, in (queue order, list order)
// after a count and an exclusive scan.
//
// Re-placement.  One lane per record: T_kf * p_c with the latest message's pose, written at base[handle] + ordinal, where base is
// the prefix of record counts in keyframe_mapping_'s iteration order (the host's shadow map) and ordinal the record's position in
// its key frame's vector — a stable bucket order by rank, which is the reference's sequence.
//
// De-duplication.  populateNodes(populateClosest = true) on an empty hash accepts point i iff no EARLIER ACCEPTED point of the 3 x 3
// cells around it is closer than min_d.  With C(i) = the earlier points of those cells closer than min_d (the conflicts), the
// greedy verdicts are the unique solution of  acc(i) = no j in C(i) is accepted  (induction over i), and Jacobi rounds on it —
// accept once every conflict is rejected, reject once one is accepted, otherwise wait — make only final decisions and settle at
// least the earliest undecided point per round (all its conflicts lie before it), so at most m rounds.  The 20-per-cell throw then
// keeps the accepted points up to and including the first one that is the 21st of its cell.
//
// Floats: the whole library builds with -ffp-contract=off.  R from the quaternion in pose_to_rt's order (not normalised), R^-1 as
// Eigen's general 3 x 3 inverse (cofactors, det = cofactors . column 0, one reciprocal, products by it), every product a plain
// k = 0, 1, 2 sum — the order tests/roadmap_kf_ref/roadmap_kf_ref.cpp restates.
#include "fs_internal.h"

#include <limits.h>

namespace {

constexpr uint64_t kEmpty = 0x8000000080000000ull;      // the cell (INT_MIN, INT_MIN): never a real cell of a finite point

__device__ __forceinline__ uint64_t cell_key(int cx, int cy) { return ((uint64_t)(uint32_t)cx << 32) | (uint32_t)cy; }

__device__ __forceinline__ int32_t kf_find_cell(const FsKfTable &t, uint64_t k)
{
    int32_t lo = 0, hi = t.n_cells;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (t.cell_key[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    return (lo < t.n_cells && t.cell_key[lo] == k) ? lo : -1;
}

// mapDataCallback's parent cell of a node at (x, y): its own cell, else the first occupied cell of the growing square; -1 none
__device__ int32_t kf_parent_cell(const FsKfTable &t, double x, double y)
{
    const int cx = fs_rm_cell(x, t.cell), cy = fs_rm_cell(y, t.cell);
    const int32_t own = kf_find_cell(t, cell_key(cx, cy));
    if (own >= 0) return own;
    int last = -1;
    for (int m = 1;; ++m) {
        const int r = (int)(t.cell * m);
        if (r > 7) return -1;
        if (r == last) continue;             // the same square again: the same (empty) scan
        last = r;
        for (int dx = -r; dx <= r; ++dx)
            for (int dy = -r; dy <= r; ++dy) {
                const int32_t c = kf_find_cell(t, cell_key(cx + dx, cy + dy));
                if (c >= 0) return c;
            }
    }
}

// count (off == nullptr) or write the records of every pending node
__global__ void kf_anchor_kernel(const FsKfTable t, int32_t n, const double *__restrict__ xy, const int32_t *__restrict__ off,
                                 int32_t *__restrict__ count, int32_t *__restrict__ rec_h, float *__restrict__ rec_p)
{
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double x = xy[2 * i], y = xy[2 * i + 1];
    const int32_t c = kf_parent_cell(t, x, y);
    if (!off) { count[i] = c < 0 ? 0 : t.cell_start[c + 1] - t.cell_start[c]; return; }
    if (c < 0) return;
    const float p[3] = {(float)x, (float)y, 0.0f};
    int32_t k = off[i];
    for (int32_t j = t.cell_start[c]; j < t.cell_start[c + 1]; ++j, ++k) {
        const int32_t s = t.cell_slots[j];
        const float *T = t.rt + (size_t)FS_KF_RT * s;
        const float *Ri = T + 12, *ti = T + 21;
#pragma unroll
        for (int a = 0; a < 3; ++a) rec_p[3 * (size_t)k + a] = (Ri[3 * a] * p[0] + Ri[3 * a + 1] * p[1] + Ri[3 * a + 2] * p[2]) + ti[a];
        rec_h[k] = t.handle[s];
    }
}

// optimizeSHM's points: T_kf * p_c of every record whose key frame the latest message holds, at base[h] + ordinal
__global__ void kf_place_kernel(int32_t n_rec, const int32_t *__restrict__ rec_h, const int32_t *__restrict__ rec_ord,
                                const float *__restrict__ rec_p, const int32_t *__restrict__ h_slot, const int32_t *__restrict__ h_base,
                                const float *__restrict__ rt, float *__restrict__ out_xy)
{
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rec) return;
    const int32_t h = rec_h[i], base = h_base[h];
    if (base < 0) return;
    const float *T = rt + (size_t)FS_KF_RT * h_slot[h];
    const float p0 = rec_p[3 * (size_t)i], p1 = rec_p[3 * (size_t)i + 1], p2 = rec_p[3 * (size_t)i + 2];
    const size_t o = (size_t)base + (size_t)rec_ord[i];
    out_xy[2 * o] = (T[0] * p0 + T[1] * p1 + T[2] * p2) + T[9];
    out_xy[2 * o + 1] = (T[3] * p0 + T[4] * p1 + T[5] * p2) + T[10];
}

__device__ __forceinline__ uint32_t hash_slot0(uint64_t k, uint32_t mask)
{
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33;
    return (uint32_t)k & mask;
}

__device__ __forceinline__ int32_t dd_lookup(const FsKfDedup &d, uint64_t k)
{
    for (uint32_t s = hash_slot0(k, d.mask), probe = 0; probe <= d.mask; s = (s + 1) & d.mask, ++probe) {
        const uint64_t v = d.hkey[s];
        if (v == k) return (int32_t)s;
        if (v == kEmpty) return -1;
    }
    return -1;
}

__global__ void dd_clear_kernel(FsKfDedup d)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s > d.mask) return;
    d.hkey[s] = kEmpty; d.hcount[s] = 0; d.hcursor[s] = 0;
    if (s == 0) { d.hdr[0] = 0; d.hdr[1] = INT32_MAX; d.hdr[2] = 0; d.hdr[3] = 0; }
}

// every point's cell into the hash (linear probing, the capacity is >= 2m), the cell's point count
__global__ void dd_insert_kernel(FsKfDedup d)
{
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.m) return;
    const uint64_t k = cell_key(fs_rm_cell((double)d.xy[2 * i], d.cell), fs_rm_cell((double)d.xy[2 * i + 1], d.cell));
    uint32_t s = hash_slot0(k, d.mask);
    for (uint32_t probe = 0; probe <= d.mask; ++probe, s = (s + 1) & d.mask) {
        const uint64_t prev = atomicCAS((unsigned long long *)&d.hkey[s], (unsigned long long)kEmpty, (unsigned long long)k);
        if (prev == kEmpty || prev == k) break;
    }
    d.pslot[i] = (int32_t)s;
    atomicAdd(&d.hcount[s], 1);
}

__global__ void dd_fill_kernel(FsKfDedup d)
{
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.m) return;
    const int32_t s = d.pslot[i];
    d.hpts[d.hstart[s] + atomicAdd(&d.hcursor[s], 1)] = i;
}

// the conflicts of point i: earlier points of the 3 x 3 cells closer than min_d (populateNodes' test, in double), counted
// (off == nullptr) or listed from off[i] on (in the cells' fill order: the verdicts depend on the set only)
__global__ void dd_conflicts_kernel(FsKfDedup d, const int32_t *__restrict__ off, int32_t *__restrict__ count, int32_t *__restrict__ out)
{
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.m) return;
    const double x = d.xy[2 * i], y = d.xy[2 * i + 1];
    const int cx = fs_rm_cell(x, d.cell), cy = fs_rm_cell(y, d.cell);
    int32_t k = off ? off[i] : 0;
    for (int dx = -1; dx <= 1; ++dx)
        for (int dy = -1; dy <= 1; ++dy) {
            const int32_t s = dd_lookup(d, cell_key(cx + dx, cy + dy));
            if (s < 0) continue;
            for (int32_t e = d.hstart[s]; e < d.hstart[s + 1]; ++e) {
                const int32_t j = d.hpts[e];
                if (j >= i) continue;
                const double ex = x - (double)d.xy[2 * j], ey = y - (double)d.xy[2 * j + 1];
                if (!(sqrt(ex * ex + ey * ey) < d.min_d)) continue;
                if (off) out[k] = j;
                ++k;
            }
        }
    if (!off) count[i] = k;
}

// one Jacobi step for point i: buffer src -> src ^ 1 (0 undecided, 1 accepted, 2 rejected); returns whether i was decided now
__device__ __forceinline__ bool dd_relax(const FsKfDedup &d, int src, int32_t i)
{
    const uint8_t *S = src ? d.state[1] : d.state[0];
    uint8_t *D = src ? d.state[0] : d.state[1];
    uint8_t v = S[i];
    bool changed = false;
    if (v == 0) {
        bool all_rejected = true, any_accepted = false;
        for (int32_t e = d.cand_off[i]; e < d.cand_off[i + 1]; ++e) {
            const uint8_t w = S[d.cand[e]];
            any_accepted |= w == 1;
            all_rejected &= w == 2;
        }
        v = any_accepted ? 2 : all_rejected ? 1 : 0;
        changed = v != 0;
    }
    D[i] = v;
    return changed;
}

// every round in one workgroup: hdr[2] = rounds run (the last one quiet), -1 when max_rounds passed.  A quiet round decides nothing,
// so every point was decided before it and both buffers hold the verdicts.
__global__ __launch_bounds__(1024) void dd_block_kernel(FsKfDedup d, int32_t max_rounds)
{
    int src = 0;
    for (int32_t r = 1; r <= max_rounds; ++r) {
        int ch = 0;
        for (int32_t i = threadIdx.x; i < d.m; i += blockDim.x) ch |= dd_relax(d, src, i) ? 1 : 0;
        src ^= 1;
        if (!__syncthreads_or(ch)) {
            if (threadIdx.x == 0) d.hdr[2] = r;
            return;
        }
    }
    if (threadIdx.x == 0) d.hdr[2] = -1;
}

__global__ __launch_bounds__(256) void dd_round_kernel(FsKfDedup d, int32_t src, int32_t *__restrict__ any)
{
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const int ch = (i < d.m && dd_relax(d, src, i)) ? 1 : 0;
    if (__syncthreads_or(ch) && threadIdx.x == 0) any[0] = 1;
}

// the 20-per-cell throw: an accepted point that is the 21st accepted point of its cell in sequence order sets the cut
__global__ void dd_cut_kernel(FsKfDedup d, int32_t src)
{
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint8_t *S = src ? d.state[1] : d.state[0];
    if (i >= d.m || S[i] != 1) return;
    const int32_t s = d.pslot[i];
    int32_t before = 0;
    for (int32_t e = d.hstart[s]; e < d.hstart[s + 1]; ++e) {
        const int32_t j = d.hpts[e];
        before += (j < i && S[j] == 1) ? 1 : 0;
    }
    if (before == FS_KF_MAX_PER_CELL) atomicMin(&d.hdr[1], i);
}

__global__ void dd_keep_kernel(FsKfDedup d, int32_t src, int32_t *__restrict__ keep)
{
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.m) return;
    const uint8_t *S = src ? d.state[1] : d.state[0];
    keep[i] = (S[i] == 1 && i <= d.hdr[1]) ? 1 : 0;
}

// the kept points in sequence order; hdr[0] = how many
__global__ void dd_compact_kernel(FsKfDedup d, int32_t src, const int32_t *__restrict__ keep_off, float *__restrict__ out_xy)
{
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) d.hdr[0] = keep_off[d.m];
    const uint8_t *S = src ? d.state[1] : d.state[0];
    if (i >= d.m || !(S[i] == 1 && i <= d.hdr[1])) return;
    const int32_t o = keep_off[i];
    out_xy[2 * o] = d.xy[2 * i];
    out_xy[2 * o + 1] = d.xy[2 * i + 1];
}

inline dim3 grid_for(int64_t n, int threads) { return dim3((unsigned)((n + threads - 1) / threads)); }

}  // namespace

// getTransformFromPose(pose) as the slot of a key-frame table: R (row-major), t, R^-1 (Eigen's general inverse), -R^-1 t.
// Returns the float determinant of R (0: no inverse).
float fs_kf_pose_table(const double pose7[7], float T[FS_KF_RT])
{
    const float x = (float)pose7[3], y = (float)pose7[4], z = (float)pose7[5], w = (float)pose7[6];
    const float tx = 2.0f * x, ty = 2.0f * y, tz = 2.0f * z;
    const float twx = tx * w, twy = ty * w, twz = tz * w;
    const float txx = tx * x, txy = ty * x, txz = tz * x;
    const float tyy = ty * y, tyz = tz * y, tzz = tz * z;
    float *R = T, *t = T + 9, *Ri = T + 12, *ti = T + 21;
    R[0] = 1.0f - (tyy + tzz); R[1] = txy - twz;          R[2] = txz + twy;
    R[3] = txy + twz;          R[4] = 1.0f - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy;          R[7] = tyz + twx;          R[8] = 1.0f - (txx + tyy);
    t[0] = (float)pose7[0]; t[1] = (float)pose7[1]; t[2] = (float)pose7[2];
    // cofactor(i, j) = m(i1, j1) m(i2, j2) - m(i1, j2) m(i2, j1), i1 = (i + 1) % 3, i2 = (i + 2) % 3 (same for j)
    float cof[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
            cof[i][j] = R[3 * i1 + j1] * R[3 * i2 + j2] - R[3 * i1 + j2] * R[3 * i2 + j1];
        }
    const float det = cof[0][0] * R[0] + cof[1][0] * R[3] + cof[2][0] * R[6];
    const float invdet = 1.0f / det;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Ri[3 * i + j] = cof[j][i] * invdet;
    for (int i = 0; i < 3; ++i) ti[i] = -((Ri[3 * i] * t[0] + Ri[3 * i + 1] * t[1]) + Ri[3 * i + 2] * t[2]);
    return det;
}

hipError_t fs_launch_kf_anchor(const FsKfTable &t, int32_t n, const double *d_xy, const int32_t *d_off, int32_t *d_count, int32_t *d_rec_h,
                               float *d_rec_p, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(kf_anchor_kernel, grid_for(n, 256), dim3(256), 0, s, t, n, d_xy, d_off, d_count, d_rec_h, d_rec_p);
    return hipGetLastError();
}

hipError_t fs_launch_kf_place(int32_t n_rec, const int32_t *d_rec_h, const int32_t *d_rec_ord, const float *d_rec_p, const int32_t *d_h_slot,
                              const int32_t *d_h_base, const float *d_rt, float *d_out_xy, hipStream_t s)
{
    if (n_rec <= 0) return hipSuccess;
    hipLaunchKernelGGL(kf_place_kernel, grid_for(n_rec, 256), dim3(256), 0, s, n_rec, d_rec_h, d_rec_ord, d_rec_p, d_h_slot, d_h_base, d_rt,
                       d_out_xy);
    return hipGetLastError();
}

hipError_t fs_launch_kf_dedup_cells(const FsKfDedup &d, hipStream_t s)
{
    hipLaunchKernelGGL(dd_clear_kernel, grid_for((int64_t)d.mask + 1, 256), dim3(256), 0, s, d);
    if (d.m <= 0) return hipGetLastError();
    hipLaunchKernelGGL(dd_insert_kernel, grid_for(d.m, 256), dim3(256), 0, s, d);
    hipError_t e = fs_launch_rm_scan(d.hcount, (int32_t)(d.mask + 1), d.hstart, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(dd_fill_kernel, grid_for(d.m, 256), dim3(256), 0, s, d);
    return hipGetLastError();
}

hipError_t fs_launch_kf_dedup_conflicts(const FsKfDedup &d, const int32_t *d_off, int32_t *d_count, int32_t *d_out, hipStream_t s)
{
    if (d.m <= 0) return hipSuccess;
    hipLaunchKernelGGL(dd_conflicts_kernel, grid_for(d.m, 256), dim3(256), 0, s, d, d_off, d_count, d_out);
    return hipGetLastError();
}

hipError_t fs_launch_kf_dedup_block(const FsKfDedup &d, int32_t max_rounds, hipStream_t s)
{
    hipLaunchKernelGGL(dd_block_kernel, dim3(1), dim3(1024), 0, s, d, max_rounds);
    return hipGetLastError();
}

hipError_t fs_launch_kf_dedup_round(const FsKfDedup &d, int32_t src, int32_t *d_any, hipStream_t s)
{
    if (d.m <= 0) return hipSuccess;
    hipLaunchKernelGGL(dd_round_kernel, grid_for(d.m, 256), dim3(256), 0, s, d, src, d_any);
    return hipGetLastError();
}

hipError_t fs_launch_kf_dedup_finish(const FsKfDedup &d, int32_t src, int32_t *d_keep, int32_t *d_keep_off, float *d_out_xy, hipStream_t s)
{
    if (d.m > 0) {
        hipLaunchKernelGGL(dd_cut_kernel, grid_for(d.m, 256), dim3(256), 0, s, d, src);
        hipLaunchKernelGGL(dd_keep_kernel, grid_for(d.m, 256), dim3(256), 0, s, d, src, d_keep);
    }
    hipError_t e = fs_launch_rm_scan(d_keep, d.m, d_keep_off, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(dd_compact_kernel, grid_for(d.m > 0 ? d.m : 1, 256), dim3(256), 0, s, d, src, d_keep_off, d_out_xy);
    return hipGetLastError();
}
