// fs_keepout.h — the cell set of a keep-out zone, as the reference's costmap layer LethalMarker rasterises it:
// a FAN OF LINES from the zone's apex cell to sampled end cells, not a filled shape (the gaps between the rays are part of the
// behaviour).  Shared by the host code (fs_capi.hip: the end cells, fp64 with libm as in the reference), the kernel
// (fs_keepout.hip: the integer walk) and the CPU restatement test (tests/keepout_ref/), like fs_roadmap_update.h.
//
// FOV zone.   addNewMarkedAreaFOV -> getPointsInIsoscelesTriangle (fit_slam2_nav2_plugins/plugins/keepout_layer.cpp:201-210,
//             74-126): 20 rays from the apex to samples t = i / 19 along the base of an isosceles triangle of apex angle
//             45 * M_PI / 180, every sample truncated toward zero and clamped into the map (cellEnforceBoundaries, :5-11).
// Disc zone.  addNewMarkedArea -> getPointsInSemiCircle (DEP/src/nav2_plugins/lethal_marker.cpp:218-226, 51-72): 360 rays to
//             the circle of radius_in_cells around the centre, robot_yaw = 0, same truncation and clamp.
// Walk.       rayTraceGeneric (keepout_layer.cpp:13-41): both end points visited, diagonal steps allowed (NOT Helpers.cpp's
//             bresenham2D).  Apex and end cell lie on the map, so every cell of the walk does.
#ifndef FS_KEEPOUT_H
#define FS_KEEPOUT_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define FS_KO_HD __host__ __device__ inline
#else
#define FS_KO_HD inline
#endif

#define FS_KO_FOV 0
#define FS_KO_DISC 1
#define FS_KO_FOV_RAYS 20                 // keepout_layer.cpp:208
#define FS_KO_DISC_RAYS 360               // lethal_marker.cpp:224
#define FS_KO_MAX_RAYS 360
#define FS_KO_COST 253                    // markCells (keepout_layer.cpp:216)

typedef struct { int32_t ax, ay, ex, ey; } fs_ko_ray;      // apex cell -> end cell

// Costmap2D::worldToMap (nav2_costmap_2d/src/costmap_2d.cpp): false below the origin or at / beyond the size.  The quotient is
// compared before it is converted (the reference converts first, which is undefined for a quotient of 2^32 or more).
inline bool fs_ko_world_to_map(double wx, double wy, double ox, double oy, double res, int32_t nx, int32_t ny, int32_t *mx, int32_t *my)
{
    if (wx < ox || wy < oy) return false;
    const double qx = (wx - ox) / res, qy = (wy - oy) / res;
    if (!(qx < 4294967296.0) || !(qy < 4294967296.0)) return false;
    const unsigned ux = (unsigned)qx, uy = (unsigned)qy;
    if (ux >= (unsigned)nx || uy >= (unsigned)ny) return false;
    *mx = (int32_t)ux; *my = (int32_t)uy;
    return true;
}

// `height / resolution` (keepout_layer.cpp:207) or `radius / resolution` (lethal_marker.cpp:223) passed as `unsigned int`:
// truncated.  False where the reference's conversion is undefined or the walk's 32-bit cells would not hold it (negative, not
// finite, 2^31 or more).
inline bool fs_ko_size_in_cells(double size_m, double res, uint32_t *cells)
{
    const double q = size_m / res;
    if (!(q >= 0.0) || !(q < 2147483648.0)) return false;
    *cells = (uint32_t)q;
    return true;
}

// cellEnforceBoundaries (keepout_layer.cpp:5-11) after static_cast<int64_t> (:108-110)
inline void fs_ko_end_cell(double sx, double sy, int32_t nx, int32_t ny, int32_t *ex, int32_t *ey)
{
    int64_t x = (int64_t)sx, y = (int64_t)sy;
    x = (x < 0) ? 0 : x;
    x = (x > (int64_t)nx - 1) ? (int64_t)nx - 1 : x;
    y = (y < 0) ? 0 : y;
    y = (y > (int64_t)ny - 1) ? (int64_t)ny - 1 : y;
    *ex = (int32_t)x; *ey = (int32_t)y;
}

// getPointsInIsoscelesTriangle (keepout_layer.cpp:74-126): the 20 rays of a FOV zone with apex cell (ax, ay)
inline int fs_ko_fov_rays(int32_t ax, int32_t ay, uint32_t height_cells, double direction, int32_t nx, int32_t ny, fs_ko_ray *out)
{
    const unsigned apex_x = (unsigned)ax, apex_y = (unsigned)ay, triangle_height = height_cells, numPoints = FS_KO_FOV_RAYS;
    const double apex_angle = 45 * M_PI / 180;                                                  // :208
    const double base_center_x = apex_x + triangle_height * cos(direction);                     // :86
    const double base_center_y = apex_y + triangle_height * sin(direction);
    const double half_base = triangle_height * tan(apex_angle / 2.0);                           // :90
    const double left_endpoint_x = base_center_x + half_base * cos(direction + M_PI_2);         // :94-97
    const double left_endpoint_y = base_center_y + half_base * sin(direction + M_PI_2);
    const double right_endpoint_x = base_center_x + half_base * cos(direction - M_PI_2);
    const double right_endpoint_y = base_center_y + half_base * sin(direction - M_PI_2);
    for (unsigned i = 0; i < numPoints; ++i) {
        const double t = (double)i / (numPoints - 1);                                           // :103
        const double sample_x = left_endpoint_x + t * (right_endpoint_x - left_endpoint_x);
        const double sample_y = left_endpoint_y + t * (right_endpoint_y - left_endpoint_y);
        out[i].ax = ax; out[i].ay = ay;
        fs_ko_end_cell(sample_x, sample_y, nx, ny, &out[i].ex, &out[i].ey);
    }
    return FS_KO_FOV_RAYS;
}

// getPointsInSemiCircle (lethal_marker.cpp:51-72) with numPoints = 360 and robot_yaw = 0 (:224): the 360 rays of a disc zone
inline int fs_ko_disc_rays(int32_t cx, int32_t cy, uint32_t radius_cells, int32_t nx, int32_t ny, fs_ko_ray *out)
{
    const unsigned center_x = (unsigned)cx, center_y = (unsigned)cy, radius_in_cells = radius_cells, numPoints = FS_KO_DISC_RAYS;
    const double robot_yaw = 0;
    for (unsigned i = 0; i < numPoints; ++i) {
        const double angle = 2.0 * M_PI * i / numPoints;                                        // :57
        const double x = center_x + radius_in_cells * cos(robot_yaw - M_PI_2 + angle);
        const double y = center_y + radius_in_cells * sin(robot_yaw - M_PI_2 + angle);
        out[i].ax = cx; out[i].ay = cy;
        fs_ko_end_cell(x, y, nx, ny, &out[i].ex, &out[i].ey);
    }
    return FS_KO_DISC_RAYS;
}

// rayTraceGeneric (keepout_layer.cpp:13-41): visit(x, y) for every cell of the line, both ends included.  (Its index test :23
// always holds here: both ends are map cells, and the walk never leaves their bounding box.)
template <typename Visit>
FS_KO_HD void fs_ko_walk(fs_ko_ray r, Visit visit)
{
    int64_t x0 = r.ax, y0 = r.ay;
    const int64_t x1 = r.ex, y1 = r.ey;
    const int64_t dx = x1 > x0 ? x1 - x0 : x0 - x1, dy = y1 > y0 ? y1 - y0 : y0 - y1;
    const int64_t sx = (x0 < x1) ? 1 : -1, sy = (y0 < y1) ? 1 : -1;
    int64_t err = dx - dy;
    while (true) {
        visit((int32_t)x0, (int32_t)y0);
        if (x0 == x1 && y0 == y1) break;
        const int64_t e2 = 2 * err;
        if (e2 > -dy) { err -= dy; x0 += sx; }
        if (e2 < dx) { err += dx; y0 += sy; }
    }
}

#endif
