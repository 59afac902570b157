// thetastar_search_ref.cpp — the host driver of fit-slam_amd/csrc/fs_thetastar.h (the REFERENCE refine search).
// Test infrastructure: built by its tests with `g++ -O2 -ffp-contract=off -shared -fPIC` and loaded through ctypes.
//
//   ts_leg         one leg in world coordinates through the header's search, table and interpolation (what fs_refine_paths returns
//                  under FS_REFINE_SEARCH_REFERENCE)
//   ts_heap_trace  a sequence of pushes, pops and in-place changes of queued entries' f through the header's heap and through
//                  std::priority_queue over pointers with the same comparator: the two pop orders
//   ts_table_check the header's table against std::hypot over signed arguments, both argument orders
#include "fs_thetastar.h"

#include <cstring>
#include <queue>
#include <vector>

namespace {

bool world_to_map(double ox, double oy, double res, int nx, int ny, double wx, double wy, int &mx, int &my)
{
    if (wx < ox || wy < oy) return false;
    const double qx = (wx - ox) / res, qy = (wy - oy) / res;
    if (!(qx < 4294967296.0) || !(qy < 4294967296.0)) return false;
    const unsigned ux = (unsigned)qx, uy = (unsigned)qy;
    if (ux >= (unsigned)nx || uy >= (unsigned)ny) return false;
    mx = (int)ux; my = (int)uy;
    return true;
}

struct Entry {
    double f;
    int32_t id;
};
struct ByF {
    bool operator()(const Entry *a, const Entry *b) const { return a->f > b->f; }
};

}  // namespace

extern "C" {

// status 0 path, 1 / 2 start / goal off the map, 3 / 4 start / goal unsafe, 5 no path.  vxy [vcap][2]: the vertices once each, start
// first; pxy [pcap][2]: the published poses.  stats: [0] nodes popped, [1] line-of-sight walks, [2] the largest heap, [3] records.
int ts_leg(const uint8_t *cells, int nx, int ny, double ox, double oy, double res, const double *start_xy, const double *goal_xy,
           int allow_unknown, double w_euc, double w_trav, int corners, int *status, double *cost, int *n_vertices, double *vxy, int vcap,
           int *n_poses, double *pxy, int pcap, int64_t *stats)
{
    *cost = DBL_MAX; *n_vertices = 0; *n_poses = 0;
    stats[0] = stats[1] = stats[2] = stats[3] = 0;
    int sx = 0, sy = 0, gx = 0, gy = 0;
    if (!world_to_map(ox, oy, res, nx, ny, start_xy[0], start_xy[1], sx, sy)) { *status = 1; return 0; }
    if (!world_to_map(ox, oy, res, nx, ny, goal_xy[0], goal_xy[1], gx, gy)) { *status = 2; return 0; }
    if (!fs_theta_safe(cells[(size_t)sy * nx + sx], allow_unknown)) { *status = 3; return 0; }
    if (!fs_theta_safe(cells[(size_t)gy * nx + gx], allow_unknown)) { *status = 4; return 0; }
    const size_t ns = (size_t)nx * ny;
    std::vector<double> hyp(ns);
    fs_theta_fill_table(hyp.data(), nx, ny);
    const fs_theta_map M{cells, nx, ny, allow_unknown ? 1 : 0, corners, w_euc, w_trav, w_euc < 1.0 ? w_euc : 1.0, hyp.data()};
    std::vector<int32_t> at(ns, -1), heap(ns + 1), cell(ns), parent(ns);
    std::vector<double> g(ns), h(ns), f(ns);
    std::vector<uint8_t> queued(ns);
    const fs_theta_mem m{at.data(), heap.data(), cell.data(), g.data(), h.data(), f.data(), parent.data(), queued.data()};
    fs_theta_state S;
    *status = fs_theta_run(M, m, S, sx, sy, gx, gy);
    stats[0] = S.pops; stats[1] = S.walks; stats[2] = S.max_heap; stats[3] = S.nrec;
    if (*status != FS_THETA_FOUND) return 0;
    *cost = g[S.cur];
    std::vector<int32_t> v(ns);
    const int32_t nv = fs_theta_backtrace(m, S.cur, v.data(), (int32_t)ns);
    std::vector<double> wx(nv), wy(nv), px, py;
    for (int32_t k = 0; k < nv; ++k) { wx[k] = fs_theta_map_to_world(ox, res, v[k] % nx); wy[k] = fs_theta_map_to_world(oy, res, v[k] / nx); }
    fs_theta_interpolate(wx.data(), wy.data(), (size_t)nv, res, px, py);
    *n_vertices = nv;
    *n_poses = (int)px.size();
    for (int k = 0; k < nv && k < vcap; ++k) { vxy[2 * k] = wx[k]; vxy[2 * k + 1] = wy[k]; }
    for (int k = 0; k < *n_poses && k < pcap; ++k) { pxy[2 * k] = px[k]; pxy[2 * k + 1] = py[k]; }
    return 0;
}

// ops [n]: 0 push a new entry with f = val, 1 pop, 2 set the f of the (arg mod queued)-th queued entry, in push order, to val.  A pop
// or a change on an empty queue is skipped.  The popped ids of the header's heap land in got, std::priority_queue's in want; returns
// the number of pops.
int ts_heap_trace(int n, const int32_t *ops, const int32_t *arg, const double *val, int32_t *got, int32_t *want)
{
    std::vector<Entry> e((size_t)n);
    std::vector<double> f((size_t)n);
    std::vector<int32_t> heap((size_t)n + 1), queued;
    std::priority_queue<Entry *, std::vector<Entry *>, ByF> q;
    int32_t size = 0, ids = 0, pops = 0;
    for (int i = 0; i < n; ++i) {
        if (ops[i] == 0) {
            const int32_t id = ids++;
            e[id] = Entry{val[i], id}; f[id] = val[i];
            q.push(&e[id]);
            fs_theta_push(heap.data(), f.data(), size, id);
            queued.push_back(id);
        } else if (queued.empty()) {
            continue;
        } else if (ops[i] == 1) {
            const int32_t w = q.top()->id;
            q.pop();
            const int32_t g = fs_theta_pop(heap.data(), f.data(), size);
            want[pops] = w; got[pops] = g;
            ++pops;
            // the reference never has two entries of one node but the start's; the queues may already disagree, so drop each one's own
            for (size_t k = 0; k < queued.size(); ++k)
                if (queued[k] == w) { queued.erase(queued.begin() + (long)k); break; }
            if (g != w) return -pops;
        } else {
            const int32_t id = queued[(size_t)arg[i] % queued.size()];
            e[id].f = val[i]; f[id] = val[i];
        }
    }
    return pops;
}

// the table of an nx x ny map against std::hypot(dx, dy) and std::hypot(dy, dx), -nx < dx < nx, -ny < dy < ny: the mismatches
int64_t ts_table_check(int nx, int ny)
{
    std::vector<double> hyp((size_t)nx * ny);
    fs_theta_fill_table(hyp.data(), nx, ny);
    const fs_theta_map M{nullptr, nx, ny, 1, 8, 1.0, 2.0, 1.0, hyp.data()};
    int64_t bad = 0;
    for (int dx = -(nx - 1); dx < nx; ++dx)
        for (int dy = -(ny - 1); dy < ny; ++dy) {
            const double t = fs_theta_hypot(M, dx, dy), a = std::hypot((double)dx, (double)dy), b = std::hypot((double)dy, (double)dx);
            bad += std::memcmp(&t, &a, 8) != 0;
            bad += std::memcmp(&t, &b, 8) != 0;
        }
    return bad;
}

}  // extern "C"
