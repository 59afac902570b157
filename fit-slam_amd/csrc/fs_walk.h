// fs_walk.h — the cell walk of getTracedCells / bresenham2D (DEP/src/Helpers.cpp:7-96) on the dense byte image, shared by the
// ray-march translation unit (fs_raymarch.hip: arrival fans, fs_trace_segments, refinePath, fs_line_of_sight) and the
// Fisher-information one (fs_fim.hip: the occluded worker).  Device code only; included after fs_internal.h.
#ifndef FS_WALK_H_
#define FS_WALK_H_

#include "fs_internal.h"

namespace {

// (unsigned)((w - origin) / resolution), the quotient of Costmap2D::worldToMap, without the fp64 division in the common
// case.  Only the truncated quotient matters: t = a * (1 / res) lies within 4 ulp (< 1.5e-6 below 2^32) of the correctly
// rounded a / res, so both truncate to the same cell unless t sits within 1e-5 of an integer — then, and for quotients
// next to 2^32 or NaN, the division itself is evaluated (a few lanes in a million).  `q` is what the caller compares and
// truncates: identical decisions to the division in every case.
__device__ __forceinline__ double cell_quotient(double a, double res, double inv_res)
{
    const double t = a * inv_res;
    const double fr = __builtin_amdgcn_fract(t);                       // t - floor(t), in [0, 1)
    if (t < 4294967295.0 && fabs(fr - 0.5) < 0.5 - 1.0e-5) return t;
    return a / res;
}

// nav2_costmap_2d::Costmap2D::worldToMap with a z axis. Quotients >= 2^32 are off-map.
__device__ __forceinline__ bool world_to_map(const FsGridDev &g, double wx, double wy, double wz,
                                             uint32_t &mx, uint32_t &my, uint32_t &mz)
{
    if (wx < g.ox || wy < g.oy || wz < g.oz) return false;
    const double inv_res = 1.0 / g.res;                                // uniform: hoisted out of the ray loops
    const double qx = cell_quotient(wx - g.ox, g.res, inv_res);
    const double qy = cell_quotient(wy - g.oy, g.res, inv_res);
    const double qz = cell_quotient(wz - g.oz, g.res, inv_res);
    if (!(qx < 4294967296.0) || !(qy < 4294967296.0) || !(qz < 4294967296.0)) return false;
    mx = (uint32_t)qx;
    my = (uint32_t)qy;
    mz = (uint32_t)qz;
    return mx < (uint32_t)g.nx && my < (uint32_t)g.ny && mz < (uint32_t)g.nz;
}

__device__ __forceinline__ int sign_ref(int x) { return x > 0 ? 1 : -1; }   // Helpers.hpp:113-116

// WalkLinear — the reference's own formulation on the dense row-major image: a linear offset, constant strides per
// axis, bresenham2D's body (DEP/src/Helpers.cpp:21-27) with a second minor axis.  Cheapest in instructions; rows only give
// x-major rays any cache-line reuse.  The winner for short rays (up to ~96 cells).
struct WalkLinear {
    uint32_t offset;
    uint32_t abs_da, abs_db, abs_dc;
    int err_b, err_c;
    int off_a, off_b, off_c;
    uint32_t end;            // min(max_length_steps, abs_da): loop visits, one more after the loop
};

// one minor axis of a walk: e += |d_minor|; if (e >= |d_major|) { v += sign; e -= |d_major|; } in five instructions —
// the subtraction's borrow IS the comparison (v_sub_co_u32), the smaller of e and e - |d_major| (unsigned wrap) is the new
// error term.  (The compiler spends a sixth on a separate compare.)
__device__ __forceinline__ void minor_step(uint32_t &v, int &e, uint32_t ad, uint32_t da, int sg)
{
    uint32_t t;
    asm("v_add_u32 %[e], %[e], %[ad]\n\t"
        "v_sub_co_u32 %[t], vcc, %[e], %[da]\n\t"
        "v_min_u32 %[e], %[e], %[t]\n\t"
        "v_cndmask_b32 %[t], %[sg], 0, vcc\n\t"
        "v_add_u32 %[v], %[v], %[t]"
        : [e] "+v"(e), [v] "+v"(v), [t] "=&v"(t)
        : [ad] "v"(ad), [da] "v"(da), [sg] "v"(sg)
        : "vcc");
}

__device__ __forceinline__ void walk_step(WalkLinear &w)
{
    w.offset += (uint32_t)w.off_a;
    minor_step(w.offset, w.err_b, w.abs_db, w.abs_da, w.off_b);
    minor_step(w.offset, w.err_c, w.abs_dc, w.abs_da, w.off_c);
}

// The cell under the walk.  Both end points are on the map (worldToMap succeeded) and a Bresenham walk between two
// cells never leaves their bounding box — each axis takes at most |d_axis| steps towards the end point — so every
// visit, including the speculative ones (they stay within `visits`), is inside the grid.
__device__ __forceinline__ int walk_cell(const FsGridDev &g, const WalkLinear &w)
{
#ifdef FS_RAY_BOUNDS   // development: verify the claim above on every visit instead of relying on it
    if (w.offset >= (uint32_t)g.nx * (uint32_t)g.ny * (uint32_t)g.nz) { atomicMax(g.dbg, 1ull); return 256; }
#endif
    return (int)g.cells[w.offset];
}

// getTracedCells from the two map cells on (Helpers.cpp:46-94): `(unsigned)(scale * abs_da)` visits with
// scale = min(1, max_length / hypot(d)).  Evaluated as the reference does (fp64 square root, division, product) only
// where it could matter:
//   * |d|^2 <= max_length^2 in integers (max_length a whole number): hypot(d) <= max_length, the quotient is >= 1 and the
//     scale exactly 1;
//   * otherwise s = |d_major| max_length / |d| in fp32 (v_rsq_f32; relative error < 1e-6) truncates like the fp64 chain
//     (relative error 3e-16) unless it lies within 4e-6 s + 1e-6 of an integer — there the fp64 chain decides.
__device__ __forceinline__ uint32_t walk_visits(int dx, int dy, int dz, uint32_t abs_da, double max_length)
{
    const long long d2 = (long long)dx * dx + (long long)dy * dy + (long long)dz * dz;
    // (a whole number of cells below 2^26 — the arrival fan's case; fs_trace_segments may pass any double — squares exactly)
    const bool whole = max_length < 67108864.0 && max_length == floor(max_length);
    if (whole && d2 < (1ll << 52) && (double)d2 <= max_length * max_length) return abs_da;
    if (d2 < (1ll << 24) && max_length < 16777216.0) {
        const float s = ((float)abs_da * (float)max_length) * __builtin_amdgcn_rsqf((float)d2);
        const float fr = s - floorf(s);
        const float guard = 4.0e-6f * s + 1.0e-6f;
        if (fr > guard && fr < 1.0f - guard) {
            const uint32_t max_steps = (uint32_t)s;
            return max_steps < abs_da ? max_steps : abs_da;
        }
    }
    const double dist = sqrt((double)d2);          // == std::hypot(dx,dy) when dz == 0 (both correctly rounded)
    const double q = max_length / dist;
    const double scale = (dist == 0.0) ? 1.0 : ((q < 1.0) ? q : 1.0);       // std::min(1.0, max_length / dist)
    const uint32_t max_steps = (uint32_t)(scale * (double)abs_da);
    return max_steps < abs_da ? max_steps : abs_da;
}

__device__ __forceinline__ void walk_init(WalkLinear &w, const FsGridDev &g, uint32_t x0, uint32_t y0, uint32_t z0,
                                          uint32_t x1, uint32_t y1, uint32_t z1, double max_length)
{
    const int dx = (int)(x1 - x0), dy = (int)(y1 - y0), dz = (int)(z1 - z0);
    const uint32_t nx = (uint32_t)g.nx, ny = (uint32_t)g.ny;
    w.offset = (z0 * ny + y0) * nx + x0;
    const uint32_t adx = (uint32_t)abs(dx), ady = (uint32_t)abs(dy), adz = (uint32_t)abs(dz);
    const int odx = sign_ref(dx), ody = sign_ref(dy) * (int)nx, odz = sign_ref(dz) * (int)(nx * ny);
    if (adx >= ady && adx >= adz) {
        w.abs_da = adx; w.abs_db = ady; w.abs_dc = adz; w.off_a = odx; w.off_b = ody; w.off_c = odz;
    } else if (ady >= adz) {
        w.abs_da = ady; w.abs_db = adx; w.abs_dc = adz; w.off_a = ody; w.off_b = odx; w.off_c = odz;
    } else {
        w.abs_da = adz; w.abs_db = adx; w.abs_dc = ady; w.off_a = odz; w.off_b = odx; w.off_c = ody;
    }
    w.err_b = w.err_c = (int)(w.abs_da / 2);
    w.end = walk_visits(dx, dy, dz, w.abs_da, max_length);
}

// The line-of-sight rule of fs_set_occlusion (include/fitslam_frontier.h) for one pair: the UNCAPPED walk from
// s to w (scale 1: visits v = 0 .. end, end = |d_major|) is blocked when a visit with v + margin <= end — the start cell
// included, the last `margin` cells at w's end left out — holds a cost in [occ_min, occ_max].  An end off the map: not ok,
// nothing tested, not blocked.  On a 2-D grid both z coordinates are the grid's origin_z.  `tested`: the visits the rule covers,
// end + 1 - margin (0 when the line is shorter than the margin), whether or not an earlier one already blocked.
// The loop runs at most end <= max(nx, ny, nz) - 1 times and stops at the first blocking cell; every visit lies in the
// bounding box of the two cells (see walk_cell).
struct LosResult {
    bool ok, blocked;
    int tested;
};

__device__ __forceinline__ LosResult line_of_sight(const FsGridDev &g, double sx, double sy, double sz, double wx, double wy, double wz,
                                                   int occ_min, int occ_max, uint32_t margin)
{
    if (g.nz == 1) { sz = g.oz; wz = g.oz; }
    uint32_t x0, y0, z0, x1, y1, z1;
    if (!world_to_map(g, wx, wy, wz, x1, y1, z1) || !world_to_map(g, sx, sy, sz, x0, y0, z0)) return LosResult{false, false, 0};
    WalkLinear w;
    walk_init(w, g, x0, y0, z0, x1, y1, z1, 0.0);
    w.end = w.abs_da;                                                  // scale = 1 (the capped count above is dead code here)
    if (w.end < margin) return LosResult{true, false, 0};
    const uint32_t n = w.end - margin + 1u;
    const uint32_t range = (uint32_t)(occ_max - occ_min);              // occ_min <= occ_max (validated by fs_set_occlusion)
    bool blocked = false;
    for (uint32_t v = 0; v < n; ++v) {
        if ((uint32_t)(walk_cell(g, w) - occ_min) <= range) { blocked = true; break; }
        walk_step(w);
    }
    return LosResult{true, blocked, (int)n};
}

}  // namespace

#endif
