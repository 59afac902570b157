// roadmap_route_ref.cpp — CPU restatement of the roadmap routes (fs_roadmap_routes) on top of the roadmap
// restatement, which it includes unchanged.  Test infrastructure: built by its tests with `g++ -O2 -ffp-contract=off -shared -fPIC`
// against the oracle's libfso_oracle.so and loaded through ctypes.
//
// Legs, each written from the reference's behaviour (DEP/ = the reference's frontier_exploration package):
//   tree route   root, ..., v: the predecessors of the shortest-path tree from the goal node back, reversed
//   astar route  FrontierRoadmapAStar::getPlan's path (DEP/src/planners/astar.cpp:42-93): std::priority_queue ordered by f, shared_ptr
//                parents, the chain from allNodes[goal] along `parent` pushed goal first and reversed (:57-69)
//   refine       FrontierRoadMap::refinePath (DEP/src/planners/FrontierRoadmap.cpp:657-714) over `connectable` (isConnectable, :716-737)
//   leg poses    getRelativePoseGivenTwoPoints: position of the first node, yaw = atan2 towards the second, orientationAroundZAxis
//                (host libm)
//   routes       setPlanForFrontierRoadmap's goal node of every frontier, one route per distinct goal node that was reached, in
//                ascending node index
#include "../roadmap_ref/roadmap_ref.cpp"

namespace {

// root .. goal along pred, or empty when the goal was not reached
std::vector<int> tree_route(const std::vector<double> &d, const std::vector<int> &pred, int root, int goal)
{
    std::vector<int> out;
    if (!(d[goal] < INFINITY)) return out;
    for (int v = goal; v != root; v = pred[v]) out.push_back(v);
    out.push_back(root);
    std::reverse(out.begin(), out.end());
    return out;
}

// reference_astar of roadmap_ref.cpp, returning the path instead of its length (empty: no path)
std::vector<int> astar_route(const Roadmap &r, int start, int goal)
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
            std::vector<int> path;
            for (auto node = all[cur->id]; node; node = node->parent) path.push_back(node->id);
            std::reverse(path.begin(), path.end());
            return path;
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
    return {};
}

// the path's length as astar.cpp:57-63 sums it: from the goal end
double route_length(const Roadmap &r, const std::vector<int> &p)
{
    double total = 0;
    for (size_t k = p.size(); k-- > 1;) total += sqrt(sq_dist(r, p[k], p[k - 1]));
    return total;
}

std::vector<int> refine(const Roadmap &r, const fso_grid &g, const int *P, int m, int *complete, long long *walks)
{
    std::vector<int> R;
    *complete = 1;
    if (m <= 0) return R;
    R.push_back(P[0]);
    int kk = 0;
    while (kk < m - 1) {
        int next = kk + 1;
        while (next < m) {
            ++*walks;
            if (!connectable(r, g, P[kk], P[next])) break;
            ++next;
        }
        if (next - 1 == kk) { *complete = 0; break; }
        R.push_back(P[next - 1]);
        kk = next - 1;
    }
    return R;
}

}  // namespace

extern "C" {

// Every frontier's route under one leg (0 the tree, 1 the per-goal A*).  route_of [n]; the routes in ascending goal node: goal_node
// [n_routes], node_off [n_routes + 1], node [total], length_m [n_routes] (summed from the goal end).  Returns 0, or -6 when max_routes /
// max_nodes are too small (*n_routes and *total are set either way).
int rrt_routes(void *h, const double robot7[7], int n, const double *goal_xyz, const uint8_t *achievable_in, int leg, int *route_of,
               int max_routes, int *n_routes, int *goal_node, long long max_nodes, long long *total, long long *node_off, int *node,
               double *length_m)
{
    const Roadmap &r = *static_cast<Roadmap *>(h);
    const int root = closest(r, robot7[0], robot7[1], true);
    std::vector<double> d;
    std::vector<int> hops, pred;
    std::vector<int> goal((size_t)n, -1);
    bool any = false;
    for (int i = 0; i < n; ++i) {
        const double gx = goal_xyz[3 * i], gy = goal_xyz[3 * i + 1];
        if (achievable_in && !achievable_in[i]) continue;
        if (robot7[0] == gx && robot7[1] == gy) continue;
        if (root < 0) continue;
        goal[i] = closest(r, gx, gy, true);
        any |= goal[i] >= 0;
    }
    if (leg == 0 && any && tree(r, root, d, hops, pred) < 0) return -1;
    std::map<int, std::vector<int>> routes;                 // goal node -> its list (ascending goal node)
    for (int i = 0; i < n; ++i) {
        if (goal[i] < 0 || routes.count(goal[i])) continue;
        routes[goal[i]] = leg == 0 ? tree_route(d, pred, root, goal[i]) : astar_route(r, root, goal[i]);
    }
    std::map<int, int> index;
    long long k = 0;
    int nr = 0;
    for (const auto &kv : routes)
        if (!kv.second.empty()) { index[kv.first] = nr++; k += (long long)kv.second.size(); }
    *n_routes = nr;
    *total = k;
    if (nr > max_routes || k > max_nodes) return -6;
    for (int i = 0; i < n; ++i) route_of[i] = (goal[i] >= 0 && index.count(goal[i])) ? index[goal[i]] : -1;
    k = 0;
    for (const auto &kv : routes) {
        if (kv.second.empty()) continue;
        const int q = index[kv.first];
        goal_node[q] = kv.first;
        node_off[q] = k;
        length_m[q] = route_length(r, kv.second);
        for (int v : kv.second) node[k++] = v;
    }
    node_off[nr] = k;
    return 0;
}

// refinePath on every list of a CSR, on the given grid: refined_off [n_routes + 1], refined [<= total], complete [n_routes];
// *walks: isConnectable calls.  Returns the refined total.
long long rrt_refine(void *h, const uint8_t *cells, int nx, int ny, double ox, double oy, double oz, double res, int n_routes,
                     const long long *node_off, const int *node, long long *refined_off, int *refined, uint8_t *complete, long long *walks)
{
    const Roadmap &r = *static_cast<Roadmap *>(h);
    const fso_grid g = make_grid(cells, nx, ny, ox, oy, oz, res);
    long long k = 0;
    *walks = 0;
    for (int q = 0; q < n_routes; ++q) {
        int ok = 1;
        const std::vector<int> R = refine(r, g, node + node_off[q], (int)(node_off[q + 1] - node_off[q]), &ok, walks);
        refined_off[q] = k;
        complete[q] = (uint8_t)ok;
        for (int v : R) refined[k++] = v;
    }
    refined_off[n_routes] = k;
    return k;
}

// the legs of every list of a CSR, route by route: pose7 [total - n_routes][7]; returns the number of legs
long long rrt_leg_poses(void *h, int n_routes, const long long *off, const int *list, double *pose7)
{
    const Roadmap &r = *static_cast<Roadmap *>(h);
    long long k = 0;
    for (int q = 0; q < n_routes; ++q)
        for (long long i = off[q]; i + 1 < off[q + 1]; ++i) {
            const int from = list[i], to = list[i + 1];
            const double yaw = atan2(r.xy[2 * to + 1] - r.xy[2 * from + 1], r.xy[2 * to] - r.xy[2 * from]);
            double *p = pose7 + 7 * k++;
            p[0] = r.xy[2 * from]; p[1] = r.xy[2 * from + 1]; p[2] = 0.0;
            p[3] = 0.0; p[4] = 0.0; p[5] = sin(yaw * 0.5); p[6] = cos(yaw * 0.5);
        }
    return k;
}

}  // extern "C"
