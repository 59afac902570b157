// planner_driver.cpp — runs CostAssignerGPU (fit-slam_amd/host/ros2/src/CostAssignerGPU.cpp, compiled unchanged) with the planner
// "NavFnGPU" against the test doubles of ros2_fakes.hpp on the GPU box; tests/test_ros2_adapter_navfn.py builds it, feeds it the
// workload file of tests/test_ros2_adapter_run.py (same layout) and compares what it writes with the CPU restatement of the grid
// planner (tests/navfn_ref/) fed through the oracle's ranking.
//
//   planner_driver workload.bin result.bin allow_unknown(0|1)
//
// result.bin (float64): for each of the two routes (three-step, fused) n x 9 columns
//   [arrival information, goal orientation, achievable, weighted cost, arrival utility, distance utility, path length (m),
//    response.frontier_costs, path length (points)]; then the number of failed checks.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

#include "fitslam_frontier_ros2/CostAssignerGPU.hpp"

template <typename T>
static void rd(FILE *f, T *p, size_t n)
{
    if (fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); }
}

static int failures = 0;
#define EXPECT(cond, what) do { if (!(cond)) { printf("CHECK FAILED: %s\n", what); ++failures; } else printf("check ok: %s\n", what); } while (0)

int main(int argc, char **argv)
{
    if (argc < 4) { fprintf(stderr, "usage: %s workload.bin result.bin allow_unknown\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t nx, ny, n, m;
    double res, ox, oy, start[3], poly[4];
    rd(f, &nx, 1); rd(f, &ny, 1); rd(f, &res, 1); rd(f, &ox, 1); rd(f, &oy, 1);
    std::vector<unsigned char> cells((size_t)nx * ny);
    rd(f, cells.data(), cells.size());
    rd(f, &n, 1);
    std::vector<double> goals(2 * (size_t)n);
    std::vector<int32_t> fsize(n);
    std::vector<uint8_t> black(n);
    rd(f, goals.data(), goals.size()); rd(f, fsize.data(), n); rd(f, black.data(), n);
    rd(f, &m, 1);
    std::vector<float> lm(3 * (size_t)m);
    rd(f, lm.data(), lm.size());
    rd(f, start, 3); rd(f, poly, 4);
    fclose(f);

    auto &prm = fakes::globals().parameters;                      // DEP/params/exploration.yaml
    prm["costCalculator/max_camera_depth"] = 2.0; prm["costCalculator/delta_theta"] = 0.10; prm["costCalculator/camera_fov"] = 1.04;
    prm["frontierCostsManager/alpha"] = 0.25; prm["frontierCostsManager/beta"] = 1.0;
    prm["frontierCostsManager/planner_allow_unknown"] = std::atoi(argv[3]) ? 1.0 : 0.0;
    prm["frontierCostsManager/vx_max"] = 0.5; prm["frontierCostsManager/wz_max"] = 0.5;
    auto costmap_ros = std::make_shared<nav2_costmap_2d::Costmap2DROS>();
    {
        fakes::CostmapRosState &r = fakes::state_of<fakes::CostmapRosState>(costmap_ros.get());
        r.robot_radius = 0.60;
        fakes::CostmapState &c = fakes::state_of<fakes::CostmapState>(&r.costmap);
        c.cells = cells; c.nx = (unsigned)nx; c.ny = (unsigned)ny; c.ox = ox; c.oy = oy; c.res = res;
    }
    std::shared_ptr<nav2_util::LifecycleNode> node = costmap_ros;
    node->declare_parameter("fitslam_frontier.gpu_devices", std::vector<int64_t>{0, 0});    // two contexts of the one GPU: the multi-device forms run

    geometry_msgs::msg::PoseStamped start_pose;
    start_pose.pose.position = {start[0], start[1], 0.0};
    start_pose.pose.orientation = nav2_util::geometry_utils::orientationAroundZAxis(start[2]);

    std::vector<double> out;
    for (int fused = 0; fused < 2; ++fused) {
        fitslam_frontier_ros2::CostAssignerGPU assigner(costmap_ros);
        assigner.setPlannerMethod("NavFnGPU");
        assigner.setFused(fused != 0);
        geometry_msgs::msg::PolygonStamped boundary;
        for (const auto &xy : {std::pair<double, double>{poly[0], poly[1]}, {poly[0], poly[3]}, {poly[2], poly[3]}, {poly[2], poly[1]}}) {
            geometry_msgs::msg::Point32 p; p.x = (float)xy.first; p.y = (float)xy.second; p.z = 0.0f;
            boundary.polygon.points.push_back(p);
        }
        assigner.updateBoundaryPolygon(boundary);
        auto req = std::make_shared<frontier_exploration::GetFrontierCostsRequest>();
        auto resp = std::make_shared<frontier_exploration::GetFrontierCostsResponse>();
        req->start_pose = start_pose;
        for (int32_t i = 0; i < n; ++i) req->frontier_list.push_back(fakes::make_frontier(goals[2 * i], goals[2 * i + 1], fsize[i]));
        for (int32_t i = 0; i < n; ++i) if (black[i]) req->prohibited_frontiers.push_back(req->frontier_list[i]);
        const int plans0 = fakes::globals().planner_calls, norm0 = fakes::globals().normalisation_calls;
        const bool ok = assigner.getFrontierCosts(req, resp);
        EXPECT(ok && resp->success, fused ? "getFrontierCosts with NavFnGPU (fused route)" : "getFrontierCosts with NavFnGPU (three-step route)");
        EXPECT(fakes::globals().planner_calls == plans0, "the reference's per-frontier planner was not called");
        EXPECT(fakes::globals().normalisation_calls > norm0, "the normalisation factors were recomputed");
        EXPECT(resp->frontier_list.size() == (size_t)n && resp->frontier_list == req->frontier_list, "response carries the request's pointers in order");
        for (int32_t i = 0; i < n; ++i) {
            const fakes::FrontierState &s = fakes::frontier(req->frontier_list[i].get());
            const auto au = s.costs.find("arrival_gain_utility"), du = s.costs.find("distance_utility");
            out.insert(out.end(), {s.arrival, s.goal_orientation, s.achievable ? 1.0 : 0.0, s.weighted_cost,
                                   au == s.costs.end() ? -1000.0 : au->second, du == s.costs.end() ? -1000.0 : du->second, s.path_length_m,
                                   resp->frontier_costs[i], s.path_length});
            if (resp->frontier_distances[i] != s.path_length_m) { printf("CHECK FAILED: response distance of frontier %d\n", i); ++failures; }
        }
    }
    out.push_back((double)failures);
    FILE *o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    fwrite(out.data(), sizeof(double), out.size(), o);
    fclose(o);
    printf("failures: %d\n", failures);
    return failures ? 1 : 0;
}
