// extern "C" entry point into the reference's Theta* planner as compiled from its own source (oracle/ref_build.py), driven the
// way the reference's path helper drives it for one leg: worldToMap of both ends, weights 1.0 / 2.0 / 1.0, 8 corners,
// setStartAndGoal, isUnsafeToPlan, generatePath, linearInterpolation at the map's resolution.
#include <cstdint>
#include <vector>

#include "frontier_exploration/planners/theta_star.hpp"
#include "quiet.hpp"

extern "C" {

// status: 0 a path, 1 start off the map, 2 goal off the map, 3 an end on an unsafe cell, 5 no path.  raw [raw_cap][2] is
// generatePath's vertex list, poses [pose_cap][2] the interpolated path; *n_raw / *n_poses are the full counts (call again with
// more room if one exceeds its cap).
int ref_theta_leg(const uint8_t *cells, int nx, int ny, double ox, double oy, double res, const double *start_xy, const double *goal_xy,
                  int allow_unknown, int *n_raw, double *raw, int raw_cap, int *n_poses, double *poses, int pose_cap)
{
    ref_wrap::Quiet quiet;
    *n_raw = 0; *n_poses = 0;
    nav2_costmap_2d::Costmap2D map(cells, (unsigned)nx, (unsigned)ny, res, ox, oy);
    geometry_msgs::msg::Point start, goal;
    start.x = start_xy[0]; start.y = start_xy[1];
    goal.x = goal_xy[0]; goal.y = goal_xy[1];
    unsigned int mx = 0, my = 0;
    if (!map.worldToMap(start.x, start.y, mx, my)) return 1;
    if (!map.worldToMap(goal.x, goal.y, mx, my)) return 2;
    frontier_exploration::ThetaStar planner;
    planner.costmap_ = &map;
    planner.how_many_corners_ = 8;
    planner.allow_unknown_ = allow_unknown != 0;
    planner.w_euc_cost_ = 1.0;
    planner.w_traversal_cost_ = 2.0;
    planner.w_heuristic_cost_ = planner.w_euc_cost_ < 1.0 ? planner.w_euc_cost_ : 1.0;
    planner.setStartAndGoal(start, goal);
    if (planner.isUnsafeToPlan()) return 3;
    std::vector<coordsW> vertices;
    if (!planner.generatePath(vertices)) return 5;
    nav_msgs::msg::Path path;
    planner.linearInterpolation(vertices, map.getResolution(), path);
    *n_raw = (int)vertices.size();
    *n_poses = (int)path.poses.size();
    for (int k = 0; k < *n_raw && k < raw_cap; ++k) { raw[2 * k] = vertices[k].x; raw[2 * k + 1] = vertices[k].y; }
    for (int k = 0; k < *n_poses && k < pose_cap; ++k) {
        poses[2 * k] = path.poses[k].pose.position.x;
        poses[2 * k + 1] = path.poses[k].pose.position.y;
    }
    return 0;
}

}  // extern "C"
