// roadmap_update_ref.cpp — fs_roadmap_update's order-free rules (fit-slam_amd/csrc/fs_roadmap_update.h) applied
// on the CPU.  Test infrastructure: built by its tests with `g++ -O2 -ffp-contract=off -shared -fPIC` against the oracle's
// libfso_oracle.so and loaded through ctypes.
//
// Nothing here walks the lists in the reference's order: the keep rule runs as Jacobi rounds over conflict rows, the owners and
// the insertions are decided per item from the header's predicates, exactly as the device stages do.  isConnectable's verdicts
// come from the oracle's single-ray trace.  tests/roadmap_ref/roadmap_ref.cpp, run sequentially, is what the result must equal.
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../fit-slam_amd/csrc/fs_roadmap_update.h"
#include "../../oracle/fso_oracle.h"

namespace {

struct Params {
    double cell, radius, min_frontier, min_robot;
};

bool walk(const Params &P, const fso_grid &g, const double *xy, int from, int to)
{
    const unsigned max_length = (unsigned)(P.radius * 1.5 / g.resolution);
    int32_t traced = 0, hit = 0, unknown = 0, all = 0, nvis = 0;
    const int ok = fso_trace_ray(&g, xy[2 * from], xy[2 * from + 1], g.origin_z, xy[2 * to], xy[2 * to + 1], g.origin_z, (double)max_length, 253,
                                 254, 0, 255, 1, &traced, &hit, &unknown, &all, nullptr, &nvis);
    return fs_ru_connectable(ok ? 1 : 0, hit ? 1 : 0, unknown, P.radius / g.resolution * 0.3);
}

// getClosestNodeInHashmap as the two passes of fs_rm_closest, under the header's order
int closest_node(const std::vector<double> &xy, double cell, double qx, double qy)
{
    const int n = (int)(xy.size() / 2);
    const int64_t cx = fs_ru_cell(qx, cell), cy = fs_ru_cell(qy, cell);
    int64_t cmin = INT64_MAX;
    for (int k = 0; k < n; ++k) {
        const int64_t ax = std::llabs((long long)(fs_ru_cell(xy[2 * k], cell) - cx)), ay = std::llabs((long long)(fs_ru_cell(xy[2 * k + 1], cell) - cy));
        cmin = std::min(cmin, std::max(ax, ay));
    }
    if (cmin == INT64_MAX) return -1;
    const int64_t R = fs_ru_search_radius(cmin, cell);
    int bk = -1;
    double bd = 0.0;
    int64_t bx = 0, by = 0;
    for (int k = n - 1; k >= 0; --k) {                   // (any order: the header's order is total)
        const int64_t ax = fs_ru_cell(xy[2 * k], cell) - cx, ay = fs_ru_cell(xy[2 * k + 1], cell) - cy;
        if (ax < -R || ax > R || ay < -R || ay > R) continue;
        const double ex = qx - xy[2 * k], ey = qy - xy[2 * k + 1];
        const double d = sqrt(ex * ex + ey * ey);
        if (fs_ru_closer(d, ax, ay, k, bd, bx, by, bk)) { bk = k; bd = d; bx = ax; by = ay; }
    }
    return bk;
}

}  // namespace

extern "C" {

// The update of a roadmap given as arrays.  Outputs: xy_out [n_old + n + 1][2] and key_out [n_old + n + 1] (the first *n_nodes
// entries), pairs [pairs_cap][2] (the first *n_pairs), stats [4] = walks, owners, keep rounds, unordered pairs with both ends owners,
// not linked before, whose two directions gave opposite verdicts.  Returns 0, -6 (the cell cap: nodes added up to the tripping one, no edge), or -100
// when pairs_cap is too small.
int ruref_update(double cell, double radius, double min_frontier, double min_robot, const uint8_t *cells, int nx, int ny, double ox,
                 double oy, double oz, double res, int n_old, const double *xy_old, const uint8_t *key_old, const int32_t *row,
                 const int32_t *col, int n, const double *pts, const double *robot, int add_robot, int32_t *n_nodes, double *xy_out,
                 uint8_t *key_out, int32_t *n_added, int32_t *robot_added, int32_t *n_pairs, int32_t *pairs, int32_t pairs_cap,
                 int64_t *stats)
{
    const Params P{cell, radius, min_frontier, min_robot};
    fso_grid g;
    g.nx = nx; g.ny = ny; g.nz = 1;
    g.origin_x = ox; g.origin_y = oy; g.origin_z = oz;
    g.resolution = res;
    g.cells = cells;
    std::vector<double> xy(xy_old, xy_old + 2 * (size_t)n_old);
    std::vector<uint8_t> key(key_old, key_old + n_old);
    *n_added = 0; *robot_added = 0; *n_pairs = 0;
    stats[0] = stats[1] = stats[2] = stats[3] = 0;
    auto finish = [&](int rc) {
        *n_nodes = (int32_t)key.size();
        std::copy(xy.begin(), xy.end(), xy_out);
        std::copy(key.begin(), key.end(), key_out);
        return rc;
    };
    if (n_old == 0 && n == 0 && !add_robot) return finish(0);

    // ---- keep: screened against the existing nodes, then the rounds over the conflict rows
    const int words = (n + 63) / 64;
    std::vector<uint64_t> conf((size_t)n * words, 0), kept(words, 0), rejected(words, 0);
    std::vector<int> occupants(n, 0);
    for (int i = 0; i < n; ++i) {
        const double x = pts[2 * i], y = pts[2 * i + 1];
        bool rej = false;
        for (int k = 0; k < n_old; ++k) {
            rej = rej || fs_ru_conflict(x, y, xy[2 * k], xy[2 * k + 1], cell, min_frontier);
            occupants[i] += fs_ru_same_cell(x, y, xy[2 * k], xy[2 * k + 1], cell) ? 1 : 0;
        }
        if (rej) rejected[i >> 6] |= 1ull << (i & 63);
        for (int j = 0; j < i; ++j)
            if (fs_ru_conflict(x, y, pts[2 * j], pts[2 * j + 1], cell, min_frontier)) conf[(size_t)i * words + (j >> 6)] |= 1ull << (j & 63);
    }
    int rounds = -1;
    for (int r = 1; r <= n + 1; ++r) {
        std::vector<uint64_t> k2 = kept, r2 = rejected;
        bool changed = false;
        for (int i = n - 1; i >= 0; --i) {                 // (Jacobi: the order inside a round does not matter)
            const uint64_t bit = 1ull << (i & 63);
            if ((kept[i >> 6] | rejected[i >> 6]) & bit) continue;
            const int v = fs_ru_keep_step(&conf[(size_t)i * words], kept.data(), rejected.data(), (i >> 6) + 1);
            if (v == FS_RU_KEPT) { k2[i >> 6] |= bit; changed = true; }
            else if (v == FS_RU_REJECTED) { r2[i >> 6] |= bit; changed = true; }
        }
        kept.swap(k2); rejected.swap(r2);
        if (!changed) { rounds = r; break; }
    }
    if (rounds < 0) return finish(-101);
    stats[2] = rounds;
    auto is_kept = [&](int i) { return (kept[i >> 6] >> (i & 63)) & 1ull; };
    int cut = INT_MAX;
    for (int i = n - 1; i >= 0; --i) {
        if (!is_kept(i)) continue;
        int before = occupants[i];
        for (int j = 0; j < i; ++j)
            if (is_kept(j) && fs_ru_same_cell(pts[2 * i], pts[2 * i + 1], pts[2 * j], pts[2 * j + 1], cell)) ++before;
        if (fs_ru_trips(before)) cut = std::min(cut, i);
    }
    for (int i = 0; i < n; ++i)
        if (is_kept(i) && i <= cut) { xy.push_back(pts[2 * i]); xy.push_back(pts[2 * i + 1]); key.push_back(0); ++*n_added; }
    if (cut != INT_MAX) return finish(-6);
    if (add_robot) {
        bool rej = false;
        int before = 0;
        for (size_t k = 0; k < key.size(); ++k) {
            rej = rej || fs_ru_conflict(robot[0], robot[1], xy[2 * k], xy[2 * k + 1], cell, min_robot);
            before += fs_ru_same_cell(robot[0], robot[1], xy[2 * k], xy[2 * k + 1], cell) ? 1 : 0;
        }
        if (!rej) {
            xy.push_back(robot[0]); xy.push_back(robot[1]); key.push_back(0);
            *robot_added = 1;
            if (fs_ru_trips(before)) return finish(-6);
        }
    }
    const int nodes = (int)key.size();
    if (nodes == 0) return finish(0);

    // ---- owners
    const int m = n + 1;
    std::vector<int32_t> closest(m);
    for (int i = 0; i < m; ++i) closest[i] = i < n ? closest_node(xy, cell, pts[2 * i], pts[2 * i + 1]) : closest_node(xy, cell, robot[0], robot[1]);
    std::vector<int32_t> owner, rank_of(nodes, -1);
    for (int i = 0; i < m; ++i)
        if (fs_ru_is_owner(closest.data(), i)) { rank_of[closest[i]] = (int32_t)owner.size(); owner.push_back(closest[i]); }
    stats[1] = (int64_t)owner.size();

    // ---- candidates in getNodesWithinRadius order, their walks
    struct Cand { int32_t q, order; bool conn; };
    std::vector<std::vector<Cand>> lists(owner.size());
    for (size_t r = 0; r < owner.size(); ++r) {
        const int p = owner[r];
        key[p] = 1;
        for (int q = 0; q < nodes; ++q) {
            int32_t order = 0;
            if (q == p || !fs_ru_within(xy[2 * p], xy[2 * p + 1], xy[2 * q], xy[2 * q + 1], cell, radius, &order)) continue;
            lists[r].push_back({q, order, false});
        }
        std::stable_sort(lists[r].begin(), lists[r].end(), [](const Cand &a, const Cand &b) { return a.order < b.order; });
        for (Cand &c : lists[r]) {
            key[c.q] = 1;
            c.conn = walk(P, g, xy.data(), c.q, p);
            ++stats[0];
        }
    }

    // ---- insertions: every candidate decided on its own
    auto listed = [&](int a, int b) {
        if (a >= n_old) return false;
        for (int j = row[a]; j < row[a + 1]; ++j)
            if (col[j] == b) return true;
        return false;
    };
    for (size_t r = 0; r < owner.size(); ++r) {
        const int p = owner[r];
        for (const Cand &c : lists[r]) {
            const int rq = rank_of[c.q];
            bool conn_pq = false;
            if (rq >= 0) {
                for (const Cand &d : lists[(size_t)rq])
                    if (d.q == p) conn_pq = d.conn;
                if (rq < (int)r && conn_pq != c.conn && !(listed(p, c.q) || listed(c.q, p))) ++stats[3];
            }
            if (!fs_ru_inserted(listed(p, c.q) || listed(c.q, p), c.conn, (int32_t)r, rq, rq >= 0 && rq < (int)r && conn_pq)) continue;
            if (*n_pairs >= pairs_cap) return finish(-100);
            pairs[2 * *n_pairs] = p; pairs[2 * *n_pairs + 1] = c.q;
            ++*n_pairs;
        }
    }
    return finish(0);
}

}  // extern "C"
