// roadmap_kf_ref.cpp — a sequential CPU restatement of FrontierRoadMap's key-frame anchoring, written the way
// DEP/src/planners/FrontierRoadmap.cpp writes it: mapDataCallback (:42-130) with its std::queue and key-frame cell hash,
// optimizeSHM (:132-155) walking keyframe_mapping_ as a std::unordered_map<int, std::vector<float3>>, and populateNodes (:185-252) as
// its plain loop over a cell hash.  The edges of the rebuilt roadmap are tests/roadmap_ref's business: the tests feed it the node
// list this file leaves.
//
// Floats: built with -ffp-contract=off.  getTransformFromPose (DEP/src/Helpers.cpp:342-352): R from the (not normalised) quaternion in
// Eigen's toRotationMatrix order; Affine3f::inverse() as Eigen's general 3 x 3 inverse (cofactors, det = cofactors . column 0, one
// reciprocal, each entry cofactor * 1/det) with translation -R^-1 t; every matrix-vector product a plain k = 0, 1, 2 sum.
#include <cmath>
#include <cstdint>
#include <map>
#include <queue>
#include <unordered_map>
#include <utility>
#include <vector>

namespace {

struct F3 { float v[3]; };

struct Affine {                 // Translation3f * Quaternionf
    float R[3][3], t[3];
};

Affine transform_from_pose(const double *p)
{
    const float x = (float)p[3], y = (float)p[4], z = (float)p[5], w = (float)p[6];
    const float tx = 2.0f * x, ty = 2.0f * y, tz = 2.0f * z;
    const float twx = tx * w, twy = ty * w, twz = tz * w;
    const float txx = tx * x, txy = ty * x, txz = tz * x;
    const float tyy = ty * y, tyz = tz * y, tzz = tz * z;
    Affine a;
    a.R[0][0] = 1.0f - (tyy + tzz); a.R[0][1] = txy - twz;          a.R[0][2] = txz + twy;
    a.R[1][0] = txy + twz;          a.R[1][1] = 1.0f - (txx + tzz); a.R[1][2] = tyz - twx;
    a.R[2][0] = txz - twy;          a.R[2][1] = tyz + twx;          a.R[2][2] = 1.0f - (txx + tyy);
    a.t[0] = (float)p[0]; a.t[1] = (float)p[1]; a.t[2] = (float)p[2];
    return a;
}

float cofactor(const float m[3][3], int i, int j)
{
    const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
    return m[i1][j1] * m[i2][j2] - m[i1][j2] * m[i2][j1];
}

Affine inverse(const Affine &a, float *det_out)
{
    Affine r;
    const float det = cofactor(a.R, 0, 0) * a.R[0][0] + cofactor(a.R, 1, 0) * a.R[1][0] + cofactor(a.R, 2, 0) * a.R[2][0];
    const float invdet = 1.0f / det;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) r.R[i][j] = cofactor(a.R, j, i) * invdet;
    for (int i = 0; i < 3; ++i) r.t[i] = -((r.R[i][0] * a.t[0] + r.R[i][1] * a.t[1]) + r.R[i][2] * a.t[2]);
    if (det_out) *det_out = det;
    return r;
}

F3 apply(const Affine &a, const F3 &p)
{
    F3 o;
    for (int i = 0; i < 3; ++i) o.v[i] = (a.R[i][0] * p.v[0] + a.R[i][1] * p.v[1] + a.R[i][2] * p.v[2]) + a.t[i];
    return o;
}

struct PairHash {
    size_t operator()(const std::pair<int, int> &c) const { return std::hash<long long>()(((long long)c.first << 32) ^ (unsigned)c.second); }
};

struct Node { double x, y; };

struct Roadmap {
    double cell, min_frontier, min_robot;
    // the node hash populateNodes fills: cell -> nodes; the node list in insertion order
    std::map<std::pair<int, int>, std::vector<int>> hash;
    std::vector<Node> nodes;
    std::queue<Node> no_kf_parent_queue;
    std::unordered_map<int, std::vector<double>> latest_keyframe_poses;     // id -> pose7
    std::unordered_map<std::pair<int, int>, std::vector<int>, PairHash> spatial_kf_map;
    std::unordered_map<int, std::vector<F3>> keyframe_mapping;

    std::pair<int, int> grid_cell(double x, double y) const
    {
        return {(int)std::floor(x / cell), (int)std::floor(y / cell)};
    }

    // populateNodes(populateClosest = true): 0, or -6 where the reference throws (the node that trips it stays, the rest not)
    int populate(const std::vector<Node> &pts, double min_d, bool add_new_to_queue)
    {
        for (const Node &p : pts) {
            const auto c = grid_cell(p.x, p.y);
            bool is_new = true;
            for (int dx = -1; dx <= 1 && is_new; ++dx)
                for (int dy = -1; dy <= 1 && is_new; ++dy) {
                    const auto it = hash.find({c.first + dx, c.second + dy});
                    if (it == hash.end()) continue;
                    for (int q : it->second) {
                        const double ex = p.x - nodes[q].x, ey = p.y - nodes[q].y;
                        if (std::sqrt(ex * ex + ey * ey) < min_d) { is_new = false; break; }
                    }
                }
            if (!is_new) continue;
            hash[c].push_back((int)nodes.size());
            nodes.push_back(p);
            if (add_new_to_queue) no_kf_parent_queue.push(p);
            if (hash[c].size() > 20) return -6;
        }
        return 0;
    }
};

}  // namespace

extern "C" {

void *kr_create(double cell, double min_frontier, double min_robot)
{
    Roadmap *r = new Roadmap;
    r->cell = cell; r->min_frontier = min_frontier; r->min_robot = min_robot;
    return r;
}

void kr_destroy(void *h) { delete static_cast<Roadmap *>(h); }

// addNodes / addRobotPoseAsNode
int kr_add_nodes(void *h, int n, const double *xy, int is_robot_pose)
{
    Roadmap &r = *static_cast<Roadmap *>(h);
    std::vector<Node> pts((size_t)n);
    for (int i = 0; i < n; ++i) pts[(size_t)i] = {xy[2 * i], xy[2 * i + 1]};
    return r.populate(pts, is_robot_pose ? r.min_robot : r.min_frontier, true);
}

// mapDataCallback; -1 (nothing changed) on a pose whose float rotation has no inverse
int kr_set_keyframes(void *h, int n, const int *ids, const double *pose7, int *n_anchored, int *n_orphaned)
{
    Roadmap &r = *static_cast<Roadmap *>(h);
    for (int i = 0; i < n; ++i) {
        float det;
        inverse(transform_from_pose(pose7 + 7 * i), &det);
        if (!(std::isfinite(det) && det != 0.0f)) return -1;
    }
    r.latest_keyframe_poses.clear();
    r.spatial_kf_map.clear();
    for (int i = 0; i < n; ++i) {
        r.latest_keyframe_poses[ids[i]] = std::vector<double>(pose7 + 7 * i, pose7 + 7 * i + 7);
        r.spatial_kf_map[r.grid_cell(pose7[7 * i], pose7[7 * i + 1])].push_back(ids[i]);
    }
    int anchored = 0, orphaned = 0;
    while (!r.no_kf_parent_queue.empty()) {
        const Node f = r.no_kf_parent_queue.front();
        r.no_kf_parent_queue.pop();
        const F3 pw{{(float)f.x, (float)f.y, 0.0f}};
        const auto cell = r.grid_cell(f.x, f.y);
        std::vector<int> parents;
        if (r.spatial_kf_map.count(cell) == 0) {
            bool found = false;
            int mult = 1;
            while (!found) {
                int radius = r.cell * mult;
                if (radius > 7) break;
                for (int dx = -radius; dx <= radius; ++dx) {
                    for (int dy = -radius; dy <= radius; ++dy) {
                        const std::pair<int, int> nb{cell.first + dx, cell.second + dy};
                        if (r.spatial_kf_map.count(nb) > 0) { parents = r.spatial_kf_map[nb]; found = true; break; }
                    }
                    if (found) break;
                }
                ++mult;
            }
        } else {
            parents = r.spatial_kf_map[cell];
        }
        (parents.empty() ? orphaned : anchored) += 1;
        for (int id : parents) {
            if (r.latest_keyframe_poses.count(id) == 0) continue;
            const Affine T = transform_from_pose(r.latest_keyframe_poses[id].data());
            r.keyframe_mapping[id].push_back(apply(inverse(T, nullptr), pw));
        }
    }
    if (n_anchored) *n_anchored = anchored;
    if (n_orphaned) *n_orphaned = orphaned;
    return 0;
}

// optimizeSHM: the new node list (0), or -6 where populateNodes throws
int kr_optimize(void *h)
{
    Roadmap &r = *static_cast<Roadmap *>(h);
    r.hash.clear();
    r.nodes.clear();
    std::vector<Node> pts;
    for (auto &kv : r.keyframe_mapping) {
        if (r.latest_keyframe_poses.count(kv.first) == 0) continue;
        const Affine T = transform_from_pose(r.latest_keyframe_poses[kv.first].data());
        for (const F3 &pc : kv.second) {
            const F3 w = apply(T, pc);
            pts.push_back({(double)w.v[0], (double)w.v[1]});
        }
    }
    return r.populate(pts, r.min_frontier, false);
}

int kr_nodes(void *h, double *xy)
{
    const Roadmap &r = *static_cast<Roadmap *>(h);
    if (xy)
        for (size_t i = 0; i < r.nodes.size(); ++i) { xy[2 * i] = r.nodes[i].x; xy[2 * i + 1] = r.nodes[i].y; }
    return (int)r.nodes.size();
}

// keyframe_mapping_ in iteration order: returns the record count; ids / points may be null
long long kr_anchors(void *h, int *n_pending, int *ids, float *pts)
{
    const Roadmap &r = *static_cast<Roadmap *>(h);
    if (n_pending) *n_pending = (int)r.no_kf_parent_queue.size();
    long long k = 0;
    for (const auto &kv : r.keyframe_mapping)
        for (const F3 &p : kv.second) {
            if (ids) ids[k] = kv.first;
            if (pts) for (int a = 0; a < 3; ++a) pts[3 * k + a] = p.v[a];
            ++k;
        }
    return k;
}

}  // extern "C"
