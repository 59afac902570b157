// roadmap_ref.cpp — CPU restatement of the frontier roadmap (fs_roadmap_*).  Test infrastructure: built by its
// tests with `g++ -O2 -ffp-contract=off -shared -fPIC` against the oracle's libfso_oracle.so and loaded through ctypes.
//
// Legs, each written from the reference's behaviour (DEP/ = the reference's frontier_exploration package):
//   populate         FrontierRoadMap::populateNodes(populateClosest = true)       DEP/src/planners/FrontierRoadmap.cpp:185-252
//   rebuild          reConstructGraph(entireGraph = true, optimizeRoadmap = false) :347-408, with getNodesWithinRadius :410-436
//   connect          constructNewEdges                                              :279-334
//   closest          getClosestNodeInHashmap / getClosestNodeInRoadMap, the growing square of hash cells as written (:464-543),
//                    bounded by the hash's extent (the reference does not return from an empty search)
//   tree             the shortest-path tree of DESIGN.md 4.10: Jacobi rounds over in-edges, key (d, hops, predecessor)
//   reference_astar  FrontierRoadmapAStar::getPlan (DEP/src/planners/astar.cpp:42-93) per goal: std::priority_queue ordered by
//                    f = g + h (h the SQUARED straight-line distance), the closed set, the strict g-comparison on re-discovery, the
//                    path length summed from the goal end.  Nodes are keyed by index (the reference keys them by an int-truncated
//                    UID of the position; distinct positions are assumed to keep distinct keys).
// isConnectable (:716-737) is the oracle's single-ray trace (fso_trace_ray) with the visitor (253, 254, 0, 255).
// pow(e, 2) of the reference is written e * e (the same correctly rounded square).
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <cfloat>
#include <map>
#include <memory>
#include <queue>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../oracle/fso_oracle.h"

namespace {

struct Roadmap {
    double cell, radius, min_frontier, min_robot;
    std::vector<double> xy;
    std::map<std::pair<int, int>, std::vector<int>> hash;
    std::vector<uint8_t> key;
    std::vector<std::vector<int>> adj;
    int n() const { return (int)(xy.size() / 2); }
};

int grid_cell(double v, double cell) { return (int)floor(v / cell); }
double dist(double ax, double ay, double bx, double by) { return sqrt((ax - bx) * (ax - bx) + (ay - by) * (ay - by)); }
double sq_dist(const Roadmap &r, int a, int b)
{
    const double ex = r.xy[2 * a] - r.xy[2 * b], ey = r.xy[2 * a + 1] - r.xy[2 * b + 1];
    return ex * ex + ey * ey;
}

std::vector<int> within_radius(const Roadmap &r, int p)
{
    std::vector<int> out;
    const double px = r.xy[2 * p], py = r.xy[2 * p + 1];
    const int cx = grid_cell(px, r.cell), cy = grid_cell(py, r.cell);
    const int cr = (int)ceil(r.radius / r.cell);
    for (int dx = -cr; dx <= cr; ++dx)
        for (int dy = -cr; dy <= cr; ++dy) {
            auto it = r.hash.find({cx + dx, cy + dy});
            if (it == r.hash.end()) continue;
            for (int q : it->second)
                if (dist(px, py, r.xy[2 * q], r.xy[2 * q + 1]) < r.radius) out.push_back(q);
        }
    return out;
}

bool connectable(const Roadmap &r, const fso_grid &g, int f1, int f2)
{
    const double max_connection_length = r.radius * 1.5;
    const unsigned max_length = (unsigned)(max_connection_length / g.resolution);
    int32_t traced = 0, hit = 0, unknown = 0, all = 0, nvis = 0;
    if (!fso_trace_ray(&g, r.xy[2 * f1], r.xy[2 * f1 + 1], g.origin_z, r.xy[2 * f2], r.xy[2 * f2 + 1], g.origin_z, (double)max_length, 253, 254, 0,
                       255, 1, &traced, &hit, &unknown, &all, nullptr, &nvis))
        return false;
    if (hit) return false;
    if (unknown > r.radius / g.resolution * 0.3) return false;
    return true;
}

// the growing square of getClosestNode*, bounded by the largest Chebyshev distance from the query's cell to an occupied cell
int closest(const Roadmap &r, double qx, double qy, bool key_only)
{
    const int cx = grid_cell(qx, r.cell), cy = grid_cell(qy, r.cell);
    long long extent = -1;
    for (const auto &kv : r.hash)
        if (!kv.second.empty())
            extent = std::max(extent, std::max(std::llabs((long long)kv.first.first - cx), std::llabs((long long)kv.first.second - cy)));
    if (extent < 0) return -1;
    double min_distance = DBL_MAX;
    int best = -1;
    for (int mult = 1;; ++mult) {
        const int search = (int)(r.cell * mult);
        for (int dx = -search; dx <= search; ++dx)
            for (int dy = -search; dy <= search; ++dy) {
                auto it = r.hash.find({cx + dx, cy + dy});
                if (it == r.hash.end()) continue;
                for (int q : it->second) {
                    if (key_only && !r.key[q]) continue;
                    const double d = dist(qx, qy, r.xy[2 * q], r.xy[2 * q + 1]);
                    if (d < min_distance) { min_distance = d; best = q; }
                }
            }
        if (best >= 0 || search >= extent) return best;
    }
}

// Jacobi rounds over in-edges until a round changes nothing; returns the number of rounds
int tree(const Roadmap &r, int root, std::vector<double> &d, std::vector<int> &hops, std::vector<int> &pred)
{
    const int n = r.n();
    std::vector<std::vector<int>> in((size_t)n);
    for (int u = 0; u < n; ++u)
        for (int v : r.adj[u]) in[v].push_back(u);
    d.assign(n, INFINITY); hops.assign(n, INT32_MAX); pred.assign(n, -1);
    d[root] = 0.0; hops[root] = 0;
    for (int round = 1;; ++round) {
        std::vector<double> d2(n);
        std::vector<int> h2(n), p2(n);
        bool changed = false;
        for (int v = 0; v < n; ++v) {
            double bd = v == root ? 0.0 : INFINITY;
            int bh = v == root ? 0 : INT32_MAX, bp = -1;
            if (v != root)
                for (int u : in[v]) {
                    if (!(d[u] < INFINITY)) continue;
                    const double cd = d[u] + sq_dist(r, u, v);
                    const int ch = hops[u] + 1;
                    if (cd < bd || (cd == bd && (ch < bh || (ch == bh && u < bp)))) { bd = cd; bh = ch; bp = u; }
                }
            d2[v] = bd; h2[v] = bh; p2[v] = bp;
            changed |= bd != d[v] || bh != hops[v] || bp != pred[v];
        }
        d.swap(d2); hops.swap(h2); pred.swap(p2);
        if (!changed) return round;
        if (round > 2 * n + 2) return -1;
    }
}

struct Node {
    int id;
    double g, h, f;
    std::shared_ptr<Node> parent;
};
struct FCompare {
    bool operator()(const std::shared_ptr<Node> &a, const std::shared_ptr<Node> &b) const { return a->f > b->f; }
};

// returns -1: no path, else the length
double reference_astar(const Roadmap &r, int start, int goal)
{
    auto h = [&](int a, int b) { return sq_dist(r, a, b); };
    std::priority_queue<std::shared_ptr<Node>, std::vector<std::shared_ptr<Node>>, FCompare> open;
    std::unordered_set<int> closed;
    std::unordered_map<int, std::shared_ptr<Node>> all;
    auto s = std::make_shared<Node>(Node{start, 0.0, 0.0, 0.0, nullptr});
    open.push(s);
    all[start] = s;
    const double gx = r.xy[2 * goal], gy = r.xy[2 * goal + 1];
    while (!open.empty()) {
        auto cur = open.top();
        open.pop();
        if (r.xy[2 * cur->id] == gx && r.xy[2 * cur->id + 1] == gy) {
            std::vector<std::shared_ptr<Node>> path;
            double total = 0;
            for (auto node = all[cur->id]; node; node = node->parent) {
                path.push_back(node);
                if (path.size() > 1) total += sqrt(h(path[path.size() - 2]->id, node->id));
            }
            return total;
        }
        closed.insert(cur->id);
        for (int nb : r.adj[cur->id]) {
            const double g = cur->g + h(cur->id, nb), hh = h(nb, goal);
            auto succ = std::make_shared<Node>(Node{nb, g, hh, g + hh, nullptr});
            if (closed.count(nb)) continue;
            if (!all.count(nb) || all[nb]->g > succ->g) {
                succ->parent = all[cur->id];
                all[nb] = succ;
                open.push(succ);
            }
        }
    }
    return -1.0;
}

double heading(const double pose7[7], double gx, double gy)
{
    const double qx = pose7[3], qy = pose7[4], qz = pose7[5], qw = pose7[6];
    double robot_yaw = atan2(2.0 * (qw * qz + qx * qy), 1.0 - 2.0 * (qy * qy + qz * qz));
    if (robot_yaw < 0) robot_yaw = robot_yaw + (M_PI * 2);
    double goal_yaw = atan2(gy - pose7[1], gx - pose7[0]);
    if (goal_yaw < 0) goal_yaw = goal_yaw + (M_PI * 2);
    double hd = fabs(robot_yaw - goal_yaw);
    if (hd > M_PI) hd = (2 * M_PI) - hd;
    return hd;
}

fso_grid make_grid(const uint8_t *cells, int nx, int ny, double ox, double oy, double oz, double res)
{
    fso_grid g;
    g.nx = nx; g.ny = ny; g.nz = 1;
    g.origin_x = ox; g.origin_y = oy; g.origin_z = oz;
    g.resolution = res;
    g.cells = cells;
    return g;
}

}  // namespace

extern "C" {

void *rr_create(double cell, double radius, double min_frontier, double min_robot)
{
    return new Roadmap{cell, radius, min_frontier, min_robot, {}, {}, {}, {}};
}

void rr_destroy(void *h) { delete static_cast<Roadmap *>(h); }

// 0, or -6 (FS_E_RANGE) where the reference throws: the node that overfilled its cell stays, the rest of the list is not added
int rr_populate(void *h, int n, const double *xy, int is_robot_pose)
{
    Roadmap &r = *static_cast<Roadmap *>(h);
    const double min_d = is_robot_pose ? r.min_robot : r.min_frontier;
    for (int i = 0; i < n; ++i) {
        const double x = xy[2 * i], y = xy[2 * i + 1];
        const std::pair<int, int> c{grid_cell(x, r.cell), grid_cell(y, r.cell)};
        bool is_new = true;
        for (int dx = -1; dx <= 1 && is_new; ++dx)
            for (int dy = -1; dy <= 1 && is_new; ++dy) {
                auto it = r.hash.find({c.first + dx, c.second + dy});
                if (it == r.hash.end()) continue;
                for (int q : it->second)
                    if (dist(x, y, r.xy[2 * q], r.xy[2 * q + 1]) < min_d) { is_new = false; break; }
            }
        if (!is_new) continue;
        r.hash[c].push_back(r.n());
        r.xy.push_back(x); r.xy.push_back(y);
        r.key.push_back(0);
        r.adj.emplace_back();
        if (r.hash[c].size() > 20) return -6;
    }
    return 0;
}

int rr_rebuild(void *h, const uint8_t *cells, int nx, int ny, double ox, double oy, double oz, double res)
{
    Roadmap &r = *static_cast<Roadmap *>(h);
    const fso_grid g = make_grid(cells, nx, ny, ox, oy, oz, res);
    for (int p = 0; p < r.n(); ++p) {
        r.key[p] = 1;
        r.adj[p].clear();
        for (int q : within_radius(r, p)) {
            if (q == p) continue;
            if (connectable(r, g, q, p) && std::find(r.adj[p].begin(), r.adj[p].end(), q) == r.adj[p].end()) r.adj[p].push_back(q);
        }
    }
    return 0;
}

int rr_connect(void *h, const uint8_t *cells, int nx, int ny, double ox, double oy, double oz, double res, int n, const double *xy)
{
    Roadmap &r = *static_cast<Roadmap *>(h);
    const fso_grid g = make_grid(cells, nx, ny, ox, oy, oz, res);
    for (int i = 0; i < n && r.n() > 0; ++i) {
        const int p = closest(r, xy[2 * i], xy[2 * i + 1], false);
        r.key[p] = 1;
        for (int q : within_radius(r, p)) {
            if (q == p) continue;
            r.key[q] = 1;
            auto &a = r.adj[p], &b = r.adj[q];
            if (std::find(a.begin(), a.end(), q) != a.end() || std::find(b.begin(), b.end(), p) != b.end()) continue;
            if (connectable(r, g, q, p)) { a.push_back(q); b.push_back(p); }
        }
    }
    return 0;
}

void rr_graph(void *h, int *n_nodes, long long *n_edges, double *xy, uint8_t *key, int *row, int *col)
{
    const Roadmap &r = *static_cast<Roadmap *>(h);
    long long e = 0;
    for (const auto &l : r.adj) e += (long long)l.size();
    *n_nodes = r.n();
    *n_edges = e;
    if (xy) memcpy(xy, r.xy.data(), sizeof(double) * r.xy.size());
    if (key) memcpy(key, r.key.data(), r.key.size());
    if (row) {
        long long k = 0;
        for (int p = 0; p < r.n(); ++p) {
            row[p] = (int)k;
            for (int q : r.adj[p]) col[k++] = q;
        }
        row[r.n()] = (int)k;
    }
}

int rr_closest(void *h, double qx, double qy, int key_only) { return closest(*static_cast<Roadmap *>(h), qx, qy, key_only != 0); }

int rr_tree(void *h, int root, double *d, int *hops, int *pred)
{
    const Roadmap &r = *static_cast<Roadmap *>(h);
    std::vector<double> dd;
    std::vector<int> hh, pp;
    const int rounds = tree(r, root, dd, hh, pp);
    std::copy(dd.begin(), dd.end(), d); std::copy(hh.begin(), hh.end(), hops); std::copy(pp.begin(), pp.end(), pred);
    return rounds;
}

// setPlanForFrontierRoadmap for every goal by one leg: 0 the tree, 1 the per-goal A*
int rr_plan(void *h, const double robot7[7], int n, const double *goal_xyz, const uint8_t *achievable_in, int leg, double *path_length,
            double *path_length_m, double *path_heading, uint8_t *achievable)
{
    const Roadmap &r = *static_cast<Roadmap *>(h);
    const int root = closest(r, robot7[0], robot7[1], true);
    std::vector<double> d;
    std::vector<int> hops, pred;
    if (leg == 0 && root >= 0 && tree(r, root, d, hops, pred) < 0) return -1;
    for (int i = 0; i < n; ++i) {
        const double gx = goal_xyz[3 * i], gy = goal_xyz[3 * i + 1];
        double len = DBL_MAX, head = DBL_MAX;
        uint8_t ok = 0;
        if (!achievable_in || achievable_in[i]) {
            if (robot7[0] == gx && robot7[1] == gy) {
                len = 0.0; ok = 1;
            } else if (root >= 0) {
                const int goal = closest(r, gx, gy, true);
                if (leg == 0 && goal >= 0 && d[goal] < INFINITY) {
                    double s = 0.0;
                    for (int v = goal; v != root; v = pred[v]) s += sqrt(sq_dist(r, v, pred[v]));
                    len = s; ok = 1;
                } else if (leg == 1 && goal >= 0) {
                    const double s = reference_astar(r, root, goal);
                    if (s >= 0) { len = s; ok = 1; }
                }
            }
            if (ok) head = heading(robot7, gx, gy);
        }
        path_length[i] = len; path_length_m[i] = len; path_heading[i] = head; achievable[i] = ok;
    }
    return 0;
}

}  // extern "C"
