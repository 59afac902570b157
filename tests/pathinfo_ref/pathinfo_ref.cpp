// pathinfo_ref.cpp — CPU restatement of the way points of fs_plan_paths_information.  Test infrastructure: built
// by its tests with `g++ -O2 -ffp-contract=off -shared -fPIC` and loaded through ctypes.
//
// The plan is the converged leg of navfn_ref.cpp, unchanged (one field, Descent::path per goal).  The sampling restates
// FrontierCostCalculator::setPlanForFrontier's loop (DEP/src/CostCalculator.cpp:302-366) literally: the running path_cut_count,
// the test `path_cut_count > (int)(sample_distance / resolution)` after the increment, the reset to 0, the look-ahead point
// std::max(i - lookahead, 0), mapToWorld(unsigned, unsigned) of both points, getRelativePoseGivenTwoPoints' atan2.  The closed
// form the GPU uses (len / (s + 1) way points, the k-th at len - (k + 1)(s + 1)) is NOT used here: the tests compare the two.
#include "../navfn_ref/navfn_ref.cpp"

namespace {

// Costmap2D::mapToWorld(unsigned mx, unsigned my) on a float path point (the truncation length_m uses)
void map_to_world(float mx, float my, double ox, double oy, double res, double &wx, double &wy)
{
    wx = ox + ((double)(uint32_t)(int64_t)mx + 0.5) * res;
    wy = oy + ((double)(uint32_t)(int64_t)my + 0.5) * res;
}

}  // namespace

extern "C" {

// Way points of n goals.  count [n], offset [n + 1], path_length [n] (DBL_MAX: not planned); xyyaw [room][3] and wp_index [room] (the
// path point i the loop stood on), or both NULL (counts only).
// Returns the total, or -2 when it exceeds room.  A robot off the map is not an error: nothing is planned.
int64_t pr_waypoints(const uint8_t *cells, int nx, int ny, double ox, double oy, double res, const double robot7[7], int allow_unknown, int n,
                     const double *goal_xyz, const uint8_t *achievable_in, double sample_distance, int lookahead, int64_t room,
                     int32_t *count, int32_t *offset, double *xyyaw, int32_t *wp_index, double *path_length)
{
    Map m;
    build_costs(cells, nx, ny, allow_unknown, m);
    int rx = 0, ry = 0;
    const bool robot_on = world_to_map(robot7[0], robot7[1], ox, oy, res, nx, ny, rx, ry);
    std::vector<float> field;
    if (robot_on) { Stats st; converged_field(m, rx, ry, field, st); }
    const int max_cycles = 4 * std::max(nx, ny);
    std::vector<float> px((size_t)max_cycles), py((size_t)max_cycles);
    int64_t total = 0;
    for (int f = 0; f < n; ++f) {
        count[f] = 0;
        offset[f] = (int32_t)total;
        path_length[f] = std::numeric_limits<double>::max();
        if (achievable_in && !achievable_in[f]) continue;
        int gx = 0, gy = 0;
        if (!robot_on || !world_to_map(goal_xyz[3 * f], goal_xyz[3 * f + 1], ox, oy, res, nx, ny, gx, gy)) continue;
        if (!(field[(size_t)gy * nx + gx] < kPotHigh)) continue;
        Descent d{field.data(), nx, nx * ny};
        const float *x = px.data(), *y = py.data();
        const int len = d.path(gx, gy, rx, ry, max_cycles, px.data(), py.data());
        if (len <= 0) continue;
        path_length[f] = (double)len;
        int path_cut_count = 0;
        int number_of_wayp = 0;
        for (int i = len - 1; i >= 0; --i) {
            double world_x, world_y;
            map_to_world(x[i], y[i], ox, oy, res, world_x, world_y);
            path_cut_count++;
            if (path_cut_count > static_cast<int>(sample_distance / res)) {
                number_of_wayp++;
                double world_x2, world_y2;
                map_to_world(x[std::max(i - lookahead, 0)], y[std::max(i - lookahead, 0)], ox, oy, res, world_x2, world_y2);
                const double dx = world_x2 - world_x, dy = world_y2 - world_y;
                const double theta = atan2(dy, dx);
                if (xyyaw) {
                    if (total >= room) return -2;
                    xyyaw[3 * total] = world_x; xyyaw[3 * total + 1] = world_y; xyyaw[3 * total + 2] = theta;
                    wp_index[total] = i;
                }
                ++total;
                path_cut_count = 0;
            }
        }
        count[f] = number_of_wayp;
    }
    offset[n] = (int32_t)total;
    return total;
}

}  // extern "C"
