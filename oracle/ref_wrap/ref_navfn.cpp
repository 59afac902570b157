// extern "C" entry points into the reference's grid planner (NavFn) as compiled from its own source (oracle/ref_build.py).
// The source file itself is included, not only its header: NavFn::updateCell is declared inline there, so a separate object
// would not export it.
#include <cstdint>
#include <cstring>

#include "nav2_costmap_2d/costmap_2d_ros.hpp"
#include "planners/planner.cpp"
#include "quiet.hpp"

using frontier_exploration::NavFn;

namespace {

int max_cycles(int nx, int ny) { return 4 * (nx >= ny ? nx : ny); }

void copy_path(NavFn &nav, int len, float *px, float *py)
{
    if (len <= 0) return;
    if (px) memcpy(px, nav.getPathX(), (size_t)len * sizeof(float));
    if (py) memcpy(py, nav.getPathY(), (size_t)len * sizeof(float));
}

}  // namespace

extern "C" {

// What the reference's per-frontier planning does with one goal (its cost calculator's call sequence): worldToMap of the robot
// and the goal, setNavArr, setCostmap(isROS), setStart(goal cell), setGoal(robot cell), calcNavFnAstar, calcPath(4 max(nx, ny)).
// Returns 0 and *len > 0 with a path; 1 robot off the map, 2 goal off the map, 3 the wave did not reach the goal, 4 calcPath gave
// no path.  px / py [4 max(nx, ny)], potarr [ny][nx] and costarr [ny][nx] may be NULL; the last two are written from status 3 on.
int ref_navfn_plan(const uint8_t *cells, int nx, int ny, double ox, double oy, double res, int allow_unknown, const double *robot_xy,
                   const double *goal_xy, int *len, float *px, float *py, float *potarr, uint8_t *costarr)
{
    ref_wrap::Quiet quiet;
    *len = 0;
    const nav2_costmap_2d::Costmap2D map(cells, (unsigned)nx, (unsigned)ny, res, ox, oy);
    NavFn nav(nx, ny);
    nav.setNavArr(nx, ny);
    nav.setCostmap(cells, true, allow_unknown != 0);
    unsigned int mx = 0, my = 0;
    if (!map.worldToMap(robot_xy[0], robot_xy[1], mx, my)) return 1;
    int map_start[2] = {(int)mx, (int)my};
    if (!map.worldToMap(goal_xy[0], goal_xy[1], mx, my)) return 2;
    int map_goal[2] = {(int)mx, (int)my};
    nav.setStart(map_goal);
    nav.setGoal(map_start);
    const bool reached = nav.calcNavFnAstar();
    if (potarr) memcpy(potarr, nav.potarr, (size_t)nx * ny * sizeof(float));
    if (costarr) memcpy(costarr, nav.costarr, (size_t)nx * ny);
    if (!reached) return 3;
    const int n = nav.calcPath(max_cycles(nx, ny));
    if (n == 0) return 4;
    *len = nav.getPathLen();
    copy_path(nav, *len, px, py);
    return 0;
}

// calcPath on a caller's field: setNavArr, setCostmap, setStart(goal cell), setGoal(robot cell), setupNavFn(true), field ->
// potarr, calcPath(4 max(nx, ny)).  A goal cell the field did not reach has no plan, as after propNavFnAstar's own return.
// Returns the path's length (0: none); px / py [4 max(nx, ny)] or NULL.
int ref_navfn_path_on_field(const uint8_t *cells, int nx, int ny, int allow_unknown, int rx, int ry, int gx, int gy, const float *field,
                            float *px, float *py)
{
    ref_wrap::Quiet quiet;
    NavFn nav(nx, ny);
    nav.setNavArr(nx, ny);
    nav.setCostmap(cells, true, allow_unknown != 0);
    int map_start[2] = {rx, ry}, map_goal[2] = {gx, gy};
    nav.setStart(map_goal);
    nav.setGoal(map_start);
    nav.setupNavFn(true);
    memcpy(nav.potarr, field, (size_t)nx * ny * sizeof(float));
    if (!(nav.potarr[(size_t)gy * nx + gx] < POT_HIGH)) return 0;
    const int n = nav.calcPath(max_cycles(nx, ny));
    if (n == 0) return 0;
    copy_path(nav, nav.getPathLen(), px, py);
    return nav.getPathLen();
}

// How many cells with costarr < COST_OBS the reference's own updateCell would lower on a caller's field (each one put back
// afterwards, the priority buffers emptied): 0 on a fixed point of the planar-wave update.  costarr [ny][nx] or NULL.
int64_t ref_navfn_fixed_point(const uint8_t *cells, int nx, int ny, int allow_unknown, int rx, int ry, const float *field, uint8_t *costarr)
{
    ref_wrap::Quiet quiet;
    NavFn nav(nx, ny);
    nav.setNavArr(nx, ny);
    nav.setCostmap(cells, true, allow_unknown != 0);
    int map_start[2] = {rx, ry};
    nav.setGoal(map_start);
    nav.setupNavFn(true);            // the obstacle ring on the border: every cell below COST_OBS has its four neighbours
    memcpy(nav.potarr, field, (size_t)nx * ny * sizeof(float));
    if (costarr) memcpy(costarr, nav.costarr, (size_t)nx * ny);
    int64_t lowered = 0;
    for (int n = 0; n < nx * ny; ++n) {
        if (nav.costarr[n] >= COST_OBS) continue;
        const float before = nav.potarr[n];
        nav.updateCell(n);
        if (nav.potarr[n] < before) ++lowered;
        nav.potarr[n] = before;
        nav.curPe = nav.nextPe = nav.overPe = 0;
        nav.pending[n - 1] = nav.pending[n + 1] = nav.pending[n - nx] = nav.pending[n + nx] = false;
    }
    return lowered;
}

}  // extern "C"
