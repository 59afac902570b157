// CostAssignerGPU.cpp — see the header.  Every reference line this file replaces is cited next to the code.
#include "fitslam_frontier_ros2/CostAssignerGPU.hpp"

#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <utility>

#include <slam_msgs/srv/get_map.hpp>

#include "frontier_exploration/util/logger.hpp"

namespace fitslam_frontier_ros2
{
using frontier_exploration::GetFrontierCostsRequest;
using frontier_exploration::GetFrontierCostsResponse;

CostAssignerGPU::CostAssignerGPU(std::shared_ptr<nav2_costmap_2d::Costmap2DROS> explore_costmap_ros, std::vector<int> device_ids)
{
    layered_costmap_ = explore_costmap_ros->getLayeredCostmap();                 // CostAssigner.cpp:11
    costmap_ = explore_costmap_ros->getCostmap();                                // FrontierCostsManager.cpp:19
    // CostCalculator.cpp:7-9,19
    max_camera_depth_ = parameterInstance.getValue<double>("costCalculator/max_camera_depth");
    delta_theta_ = parameterInstance.getValue<double>("costCalculator/delta_theta");
    camera_fov_ = parameterInstance.getValue<double>("costCalculator/camera_fov");
    robot_radius_ = explore_costmap_ros->getRobotRadius();
    // FrontierCostsManager.cpp:10-16
    alpha_ = parameterInstance.getValue<double>("frontierCostsManager/alpha");
    beta_ = parameterInstance.getValue<double>("frontierCostsManager/beta");
    planner_allow_unknown_ = parameterInstance.getValue<bool>("frontierCostsManager/planner_allow_unknown");
    max_vx_ = parameterInstance.getValue<double>("frontierCostsManager/vx_max");
    max_wx_ = parameterInstance.getValue<double>("frontierCostsManager/wz_max");

    // the reference's calculator is kept for its planners only (roadmap A* / NavFn / Euclidean: out of the GPU path)
    planner_ = std::make_shared<frontier_exploration::FrontierCostCalculator>(explore_costmap_ros);

    // One scorer object in this process, whatever the number of GPUs: the node's parameter `fitslam_frontier.gpu_devices`
    // (an integer array, default [0]) lists the HIP ordinals; the frontier list of a tick is cut into one contiguous block
    // per entry and the blocks run side by side (fs_multi_*, include/fitslam_frontier.h).
    if (device_ids.empty()) {
        auto node = explore_costmap_ros->shared_from_this();
        std::vector<int64_t> ids{0};
        if (!node->has_parameter("fitslam_frontier.gpu_devices")) node->declare_parameter("fitslam_frontier.gpu_devices", ids);
        node->get_parameter("fitslam_frontier.gpu_devices", ids);
        for (const int64_t d : ids) device_ids.push_back(static_cast<int>(d));
    }
    if (fs_multi_create(device_ids.data(), static_cast<int>(device_ids.size()), &scorer_) != FS_OK)
        throw std::runtime_error("fitslam_frontier: no MI355X (gfx950) under one of fitslam_frontier.gpu_devices; there is no CPU fallback");
    pushRayParams();
    LOG_INFO("CostAssignerGPU: scoring on " << fs_multi_num_devices(scorer_) << " HIP device(s)");
}

CostAssignerGPU::~CostAssignerGPU()
{
    fs_multi_destroy(scorer_);
}

void CostAssignerGPU::check(int rc, const char *what) const
{
    if (rc != FS_OK) throw std::runtime_error(std::string(what) + ": " + fs_multi_last_error(scorer_));
}

void CostAssignerGPU::restoreArrivalLimits()
{
    // setMaxArrivalInformation's cache (CostCalculator.cpp:125,185-188) survives new parameters and new snapshots
    if (!arrival_info_limits_set_) return;
    for (int g = 0; g < fs_multi_num_devices(scorer_); ++g)
        fs_set_arrival_limits(fs_multi_ctx(scorer_, g), max_arrival_info_gt_, min_arrival_info_gt_);
}

void CostAssignerGPU::pushRayParams()
{
    fs_ray_params p;
    std::memset(&p, 0, sizeof p);
    p.max_camera_depth = max_camera_depth_;
    p.delta_theta = delta_theta_;
    p.camera_fov = camera_fov_;
    p.robot_radius = robot_radius_;
    p.n_rays = 0;                       // the reference loop `theta <= 2 * M_PI` (CostCalculator.cpp:36)
    p.n_elev = 1;
    p.elev[0] = 0.0;                    // 2-D costmap: one ring
    p.obst_min = 240; p.obst_max = 254; p.trace_min = 255; p.trace_max = 255;   // CostCalculator.cpp:40
    p.factor_max = 1.2; p.factor_min = 0.70;                                     // CostCalculator.cpp:186-188
    if (polygon_xy_min_max_.size() >= 4) {
        for (int i = 0; i < 4; ++i) p.polygon[i] = polygon_xy_min_max_[i];
    } else {
        p.polygon[0] = p.polygon[1] = -std::numeric_limits<double>::max();
        p.polygon[2] = p.polygon[3] = std::numeric_limits<double>::max();
    }
    check(fs_multi_set_ray_params(scorer_, &p), "fs_multi_set_ray_params");
    restoreArrivalLimits();
}

void CostAssignerGPU::snapshotCostmap()
{
    // The reference reads the live costmap while the costmap thread may be writing it; here the upload
    // is the snapshot point and is taken under the costmap's own mutex.
    std::unique_lock<nav2_costmap_2d::Costmap2D::mutex_t> lock(*(costmap_->getMutex()));
    const double origin[3] = {costmap_->getOriginX(), costmap_->getOriginY(), 0.0};
    check(fs_multi_upload_grid(scorer_, costmap_->getCharMap(), static_cast<int32_t>(costmap_->getSizeInCellsX()),
                               static_cast<int32_t>(costmap_->getSizeInCellsY()), 1, origin, costmap_->getResolution()),
          "fs_multi_upload_grid");
    restoreArrivalLimits();
}

void CostAssignerGPU::setFrontierBlacklist(std::vector<FrontierPtr> &blacklist)
{
    std::lock_guard<std::mutex> lock(blacklist_mutex_);                          // FrontierCostsManager.cpp:217
    for (auto frontier : blacklist) frontier_blacklist_[frontier] = true;
}

bool CostAssignerGPU::updateBoundaryPolygon(geometry_msgs::msg::PolygonStamped &explore_boundary)
{
    // What CostAssigner.cpp:121-167 leaves behind is the bounding box [min x, min y, max x, max y] of the exploration
    // polygon, taken over its float32 vertices (geometry_msgs/Point32).  An empty polygon means "the whole map": the
    // reference then uses the corners (origin) and (getSizeInMeters) — a size, not origin + size, for the far corner: a
    // quirk that decides where rays are clamped (CostCalculator.cpp:47-48), so it is kept.  The vertices accumulate across
    // calls like the reference's member polygon does.
    for (const auto &vertex : explore_boundary.polygon.points) polygon_.points.push_back(vertex);
    if (polygon_.points.empty()) {
        const nav2_costmap_2d::Costmap2D *map = layered_costmap_->getCostmap();
        const float x_lo = static_cast<float>(map->getOriginX()), y_lo = static_cast<float>(map->getOriginY());
        const float x_hi = static_cast<float>(map->getSizeInMetersX()), y_hi = static_cast<float>(map->getSizeInMetersY());
        for (const auto &xy : {std::pair<float, float>{x_lo, y_lo}, {x_lo, y_hi}, {x_hi, y_hi}, {x_hi, y_lo}}) {
            geometry_msgs::msg::Point32 corner;
            corner.x = xy.first; corner.y = xy.second;
            polygon_.points.push_back(corner);
        }
    }
    const double inf = std::numeric_limits<double>::infinity();
    double box[4] = {inf, inf, -inf, -inf};
    for (const auto &vertex : polygon_.points) {
        box[0] = std::min(box[0], static_cast<double>(vertex.x)); box[1] = std::min(box[1], static_cast<double>(vertex.y));
        box[2] = std::max(box[2], static_cast<double>(vertex.x)); box[3] = std::max(box[3], static_cast<double>(vertex.y));
    }
    polygon_xy_min_max_.insert(polygon_xy_min_max_.end(), box, box + 4);         // (appended, as the reference does: the first four count)
    pushRayParams();                                                             // the clamp box of CostCalculator.cpp:47-48
    return true;
}

bool CostAssignerGPU::prepareTick(std::vector<FrontierPtr> &frontier_list)
{
    planner_->reset();                                                           // FrontierCostsManager.cpp:51
    snapshotCostmap();
    if (!arrival_info_limits_set_) {                                             // :52, CostCalculator.cpp:123-191 (cached)
        double max_value = 0, max_gt = 0, min_gt = 0;
        check(fs_multi_max_arrival(scorer_, &max_value, &max_gt, &min_gt), "fs_multi_max_arrival");
        if (max_value != 0.0) {
            arrival_info_limits_set_ = true;
            max_arrival_info_gt_ = max_gt;
            min_arrival_info_gt_ = min_gt;
        }
    }
    if (frontier_list.size() == 0) {                                             // :55-59
        LOG_ERROR("No frontiers found from frontier search.");
        return false;
    }
    if (polygon_xy_min_max_.size() <= 0) {                                       // :61-65
        LOG_ERROR("FrontierPtr cannot be selected, no polygon.");
        return false;
    }
    for (size_t i = 0; i < frontier_list.size(); ++i)                            // :25-45,69-72
        for (size_t j = i + 1; j < frontier_list.size(); ++j)
            if (frontier_list[i] == frontier_list[j]) throw std::runtime_error("Duplicate frontiers found.");
    return true;
}

void CostAssignerGPU::plan(geometry_msgs::msg::Pose start_pose_w, FrontierPtr &frontier)
{
    auto map_data = std::make_shared<slam_msgs::srv::GetMap::Response>();        // CostAssigner.cpp:37 (left empty there too)
    if (planner_method_ == "A*PlannerDistance")
        planner_->setPlanForFrontier(start_pose_w, frontier, map_data, false, planner_allow_unknown_);
    else if (planner_method_ == "RoadmapPlannerDistance")
        planner_->setPlanForFrontierRoadmap(start_pose_w, frontier, map_data, false, planner_allow_unknown_);
    else
        planner_->setPlanForFrontierEuclidean(start_pose_w, frontier, map_data, false, planner_allow_unknown_);
}

// "NavFnGPU": FrontierCostCalculator::setPlanForFrontier ("A*PlannerDistance", CostCalculator.cpp:193-393) for the whole list in
// ONE call — fs_plan_paths on the first device (the grid is already staged there by snapshotCostmap): one NavFn potential from the
// robot cell, every frontier's descent batched.  plan_in[i] = 0: not planned (the reference returns at once for
// an unachievable frontier, :196-204: DBL_MAX columns, achievable false).  Every frontier with apply[i] gets the columns the
// reference's planner would have set; the headings come back in `heading` (the ranking's column).
void CostAssignerGPU::planAllOnDevice(const geometry_msgs::msg::Pose &start_pose_w, std::vector<FrontierPtr> &frontier_list,
                                      const std::vector<double> &goal, const std::vector<uint8_t> &plan_in, const std::vector<uint8_t> &apply,
                                      std::vector<double> &heading)
{
    const int32_t n = static_cast<int32_t>(frontier_list.size());
    const double pose7[7] = {start_pose_w.position.x, start_pose_w.position.y, start_pose_w.position.z, start_pose_w.orientation.x,
                             start_pose_w.orientation.y, start_pose_w.orientation.z, start_pose_w.orientation.w};
    std::vector<double> plen(n), plen_m(n);
    std::vector<uint8_t> ach(n);
    heading.assign(n, 0.0);
    fs_ctx *ctx = fs_multi_ctx(scorer_, 0);
    const int rc = fs_plan_paths(ctx, pose7, planner_allow_unknown_ ? 1 : 0, n, goal.data(), plan_in.data(), plen.data(), plen_m.data(),
                                 heading.data(), ach.data());
    if (rc != FS_OK) throw std::runtime_error(std::string("fs_plan_paths: ") + fs_last_error(ctx));
    for (int32_t i = 0; i < n; ++i) {
        if (!apply[i]) continue;
        auto &f = frontier_list[i];
        f->setAchievability(ach[i] != 0);                                        // :196-204, :257-300
        f->setPathLength(plen[i]);                                               // :330
        f->setPathLengthInM(plen_m[i]);                                          // :331
        if (!ach[i]) f->setFisherInformation(0);
    }
}

// assignCosts through ONE device call (fs_multi_get_frontier_costs).  The planner runs FIRST, on every frontier that is not
// blacklisted and as if achievable; what it decides (a frontier it cannot reach: achievable = false) enters the call as
// achievable_in, which the arrival step can only clear further — the final flag is the AND of the same conditions in either
// order, and the path columns of a frontier that ends up unachievable are never read.  (The same construction as
// FrontierCostsManager::assignCostsFused of the C++ mirror, fit-slam_amd/host/frontier_scoring.hpp, which tests/test_host_mirror.py
// compares bit for bit with the three-step route.)
bool CostAssignerGPU::assignCostsFused(std::vector<FrontierPtr> &frontier_list, geometry_msgs::msg::Pose start_pose_w)
{
    const double dmax = std::numeric_limits<double>::max();
    if (!prepareTick(frontier_list)) return false;
    const int32_t n = static_cast<int32_t>(frontier_list.size());
    std::vector<double> goal(3 * static_cast<size_t>(n)), plen(n, 0.0), phead(n, 0.0), cost(n), au(n), du(n);
    std::vector<int32_t> fsize(n);
    std::vector<uint8_t> black(n, 0), ach_in(n, 1);
    {
        std::lock_guard<std::mutex> lock(blacklist_mutex_);
        for (int32_t i = 0; i < n; ++i) black[i] = frontier_blacklist_.count(frontier_list[i]) > 0 ? 1 : 0;   // :77
    }
    const bool on_device = planner_method_ == "NavFnGPU";
    std::vector<uint8_t> live(n);
    for (int32_t i = 0; i < n; ++i) {
        auto &f = frontier_list[i];
        const geometry_msgs::msg::Point &g = f->getGoalPoint();
        goal[3 * i] = g.x; goal[3 * i + 1] = g.y; goal[3 * i + 2] = 0.0;
        fsize[i] = f->getSize();
        live[i] = black[i] ? 0 : 1;
        if (black[i] || on_device) continue;
        plan(start_pose_w, f);                                                   // (the reference's planners return at once for a frontier that is already unachievable)
        ach_in[i] = f->isAchievable() ? 1 : 0;
        if (ach_in[i]) { plen[i] = f->getPathLength(); phead[i] = f->getPathHeading(); }
    }
    if (on_device) {                                                             // every live frontier planned in one call
        std::vector<double> heading;
        planAllOnDevice(start_pose_w, frontier_list, goal, live, live, heading);
        for (int32_t i = 0; i < n; ++i) {
            if (black[i]) continue;
            ach_in[i] = frontier_list[i]->isAchievable() ? 1 : 0;
            if (ach_in[i]) { plen[i] = frontier_list[i]->getPathLength(); phead[i] = heading[i]; }
        }
    }
    std::vector<fs_record> rec(n);
    const int rc = fs_multi_get_frontier_costs(scorer_, n, goal.data(), fsize.data(), black.data(), ach_in.data(), plen.data(), phead.data(),
                                               alpha_, beta_, max_vx_, max_wx_, /*with_fisher_information=*/0,
                                               rec.data(), cost.data(), au.data(), du.data(), nullptr);
    if (rc == FS_E_RANGE) throw std::runtime_error("Cost out of bounds");        // :148-149,173-174
    check(rc, "fs_multi_get_frontier_costs");
    for (int32_t i = 0; i < n; ++i) {
        auto &f = frontier_list[i];
        if (black[i]) {                                                          // :77-86
            f->setArrivalInformation(0.0); f->setGoalOrientation(0.0); f->setFisherInformation(0.0);
            f->setPathLength(dmax); f->setPathLengthInM(dmax); f->setWeightedCost(dmax);
            continue;
        }
        f->setArrivalInformation(static_cast<double>(rec[i].arrival));           // CostCalculator.cpp:52 / :112
        // goal_yaw = maxIndex * delta_theta + fov / 2 in double (:119); 0 where the goal is off the map (:52-54)
        f->setGoalOrientation(FS_RECORD_STATUS(rec[i].flags) == FS_STATUS_OK ? static_cast<double>(rec[i].argmax) * delta_theta_ + camera_fov_ / 2 : 0.0);
        const bool achievable = (rec[i].flags & FS_FLAG_ACHIEVABLE) != 0;
        f->setAchievability(achievable);                                         // :78-82, :114-118
        if (!achievable) { f->setPathLength(dmax); f->setPathLengthInM(dmax); f->setFisherInformation(0.0); }   // what the skipped plan leaves behind
        planner_->recomputeNormalizationFactors(f);                              // :118
        f->setWeightedCost(cost[i]);                                             // :130 / :198
        f->setCost("arrival_gain_utility", au[i]);                               // :131 / :199
        f->setCost("distance_utility", du[i]);                                   // :132 / :200
    }
    return true;
}

bool CostAssignerGPU::assignCosts(std::vector<FrontierPtr> &frontier_list, geometry_msgs::msg::Pose start_pose_w)
{
    const double dmax = std::numeric_limits<double>::max();
    if (!prepareTick(frontier_list)) return false;

    // ---- arrival information for the whole list: ONE launch instead of the loop of :74-119
    const int32_t n = static_cast<int32_t>(frontier_list.size());
    std::vector<double> goal(3 * static_cast<size_t>(n)), yaw(n);
    std::vector<int32_t> fsize(n), arrival(n), argmax(n), status(n);
    std::vector<uint8_t> black(n, 0), ach_in(n), ach(n);
    {
        std::lock_guard<std::mutex> lock(blacklist_mutex_);
        for (int32_t i = 0; i < n; ++i) {
            const auto &f = frontier_list[i];
            const geometry_msgs::msg::Point &g = f->getGoalPoint();
            goal[3 * i] = g.x; goal[3 * i + 1] = g.y; goal[3 * i + 2] = 0.0;
            fsize[i] = f->getSize();
            ach_in[i] = f->isAchievable() ? 1 : 0;
            black[i] = frontier_blacklist_.count(f) > 0 ? 1 : 0;                 // :77
        }
    }
    check(fs_multi_score_arrival(scorer_, n, goal.data(), fsize.data(), black.data(), ach_in.data(), nullptr, arrival.data(),
                                 argmax.data(), yaw.data(), ach.data(), status.data()), "fs_multi_score_arrival");

    const bool on_device = planner_method_ == "NavFnGPU";
    std::vector<double> heading;
    if (on_device) {                                                             // the plans of :98-109, one call for the list
        std::vector<uint8_t> plan_in(n), apply(n);
        for (int32_t i = 0; i < n; ++i) { apply[i] = black[i] ? 0 : 1; plan_in[i] = (!black[i] && ach[i]) ? 1 : 0; }
        planAllOnDevice(start_pose_w, frontier_list, goal, plan_in, apply, heading);
    }
    for (int32_t i = 0; i < n; ++i) {
        auto &frontier = frontier_list[i];
        if (black[i]) {                                                          // :77-86
            frontier->setArrivalInformation(0.0);
            frontier->setGoalOrientation(0.0);
            frontier->setFisherInformation(0.0);
            frontier->setPathLength(dmax);
            frontier->setPathLengthInM(dmax);
            frontier->setWeightedCost(dmax);
            continue;
        }
        frontier->setArrivalInformation(static_cast<double>(arrival[i]));        // CostCalculator.cpp:52 / :112
        frontier->setGoalOrientation(yaw[i]);                                    // :53 / :119
        if (!on_device) {                                                        // ("NavFnGPU" planned above: achievability is the planner's)
            frontier->setAchievability(ach[i] != 0);                             // :78-82, :114-118
            // planning stays with the reference (:98-109); it skips frontiers that are not achievable
            plan(start_pose_w, frontier);
        }
        planner_->recomputeNormalizationFactors(frontier);                       // :118
    }

    // ---- U1 utility + weighted cost (:126-205): ONE launch
    std::vector<fs_record> rec(n);
    std::vector<double> plen(n), phead(n), cost(n), au(n), du(n);
    for (int32_t i = 0; i < n; ++i) {
        auto &f = frontier_list[i];
        std::memset(&rec[i], 0, sizeof(fs_record));
        rec[i].arrival = black[i] ? 0 : arrival[i];
        rec[i].flags = (!black[i] && f->isAchievable()) ? FS_FLAG_ACHIEVABLE : 0u;
        plen[i] = f->getPathLength();
        phead[i] = (black[i] || !f->isAchievable()) ? 0.0 : (on_device ? heading[i] : f->getPathHeading());
    }
    fs_ctx *rank_ctx = fs_multi_ctx(scorer_, 0);                                  // the gathered list is ranked on the first device
    const int rc = fs_rank_candidates(rank_ctx, n, rec.data(), black.data(), plen.data(), phead.data(), alpha_, beta_, max_vx_, max_wx_,
                                      cost.data(), au.data(), du.data(), nullptr);
    if (rc == FS_E_RANGE) throw std::runtime_error("Cost out of bounds");        // :148-149,173-174
    if (rc != FS_OK) throw std::runtime_error(std::string("fs_rank_candidates: ") + fs_last_error(rank_ctx));
    for (int32_t i = 0; i < n; ++i) {
        if (black[i]) continue;                                                  // its weighted cost is already max (:84)
        frontier_list[i]->setWeightedCost(cost[i]);                              // :130 / :198
        frontier_list[i]->setCost("arrival_gain_utility", au[i]);                // :131 / :199
        frontier_list[i]->setCost("distance_utility", du[i]);                    // :132 / :200
    }
    return true;
}

bool CostAssignerGPU::getFrontierCosts(std::shared_ptr<GetFrontierCostsRequest> requestData,
                                       std::shared_ptr<GetFrontierCostsResponse> resultData)
{
    // The contract of CostAssigner.cpp:73-119: the prohibited frontiers join the blacklist first; the request's frontiers are
    // scored IN PLACE; the response carries the very same pointers in the very same order plus three parallel columns read
    // back from them (weighted cost, path length in metres, arrival information); a failed scoring (empty list, no polygon)
    // only clears `success`.
    setFrontierBlacklist(requestData->prohibited_frontiers);
    resultData->success = fused_ ? assignCostsFused(requestData->frontier_list, requestData->start_pose.pose)
                                 : assignCosts(requestData->frontier_list, requestData->start_pose.pose);
    if (!resultData->success) return false;
    const std::vector<FrontierPtr> &scored = requestData->frontier_list;
    resultData->frontier_list.assign(scored.begin(), scored.end());
    resultData->frontier_costs.resize(scored.size());
    resultData->frontier_distances.resize(scored.size());
    resultData->frontier_arrival_information.resize(scored.size());
    for (size_t i = 0; i < scored.size(); ++i) {
        resultData->frontier_costs[i] = scored[i]->getWeightedCost();
        resultData->frontier_distances[i] = scored[i]->getPathLengthInM();
        resultData->frontier_arrival_information[i] = scored[i]->getArrivalInformation();
    }
    if (resultData->frontier_list != requestData->frontier_list) throw std::runtime_error("Lists are not SAME!");   // :105-108
    return true;
}

}  // namespace fitslam_frontier_ros2
