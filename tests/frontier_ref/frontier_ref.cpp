// frontier_ref.cpp — CPU restatement of the order-dependent tail of FrontierSearch::buildNewFrontier (DEP/src/FrontierSearch.cpp:98-216)
// that fs_search_frontiers runs on the device, and the checks of fit-slam_amd/csrc/fs_median_sort.h.
//
// TEST INFRASTRUCTURE, never linked into the product.  Built by tests/frontier_ref.py with g++ -O2 -ffp-contract=off.
//
//   fr_search     the components come in as labels (label = smallest cell index of the component, -1: not a found frontier cell;
//                 fs_frontier_clusters' labels, or the oracle's).  Seeds: the caller's list, or per component (ascending label)
//                 the cell nearest the robot's cell (squared cell distance, ties to the smaller index).  Per seed the breadth-first
//                 walk in nhood8 order, pieces of max + 1 cells in queue order, the remainder if it exceeds min, the centroid of
//                 getCentroidOfCells, and the goal point from a REAL std::sort with SortByMedianFunctor — not the header's restatement.
//   fr_sort_*     the header's restatement against std::sort, element for element.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <queue>
#include <utility>
#include <vector>

#include "fs_median_sort.h"

namespace {

struct Grid {
    int nx, ny;
    double ox, oy, res;
    std::pair<double, double> world(int idx) const
    {
        const unsigned int mx = (unsigned int)(idx % nx), my = (unsigned int)(idx / nx);
        return {ox + (mx + 0.5) * res, oy + (my + 0.5) * res};     // Costmap2D::mapToWorld
    }
    int nhood8(int idx, int out[8]) const
    {
        const int sx = nx;
        const bool l = idx % sx > 0, r = idx % sx < sx - 1, u = idx >= sx, d = idx < sx * (ny - 1);
        int k = 0;
        if (l) out[k++] = idx - 1;
        if (r) out[k++] = idx + 1;
        if (u) out[k++] = idx - sx;
        if (d) out[k++] = idx + sx;
        if (l && u) out[k++] = idx - 1 - sx;
        if (l && d) out[k++] = idx - 1 + sx;
        if (r && u) out[k++] = idx + 1 - sx;
        if (r && d) out[k++] = idx + 1 + sx;
        return k;
    }
};

// FrontierSearch.hpp:84-127
std::pair<double, double> centroid_of_cells(const std::vector<std::pair<double, double>> &cells, double res, double offset)
{
    double sumX = 0, sumY = 0;
    for (const auto &p : cells) { sumX += p.first; sumY += p.second; }
    double cx = sumX / cells.size(), cy = sumY / cells.size();
    bool off = false;
    double varX = 0, varY = 0;
    for (const auto &p : cells) {
        if (std::sqrt(std::pow(p.first - cx, 2) + std::pow(p.second - cy, 2)) < res * 3) off = true;
        varX += std::abs(p.first - cx);
        varY += std::abs(p.second - cy);
    }
    if (varX > varY && off) cy -= offset;
    if (varX < varY && off) cx -= offset;
    return {cx, cy};
}

// FrontierSearch.hpp:156-181
struct SortByMedianFunctor {
    std::pair<double, double> centroid;
    bool operator()(const std::pair<double, double> &a, const std::pair<double, double> &b) const
    {
        auto angle_a = atan2(a.second - centroid.second, a.first - centroid.first);
        if (angle_a < 0) angle_a = angle_a + (2 * M_PI);
        auto angle_b = atan2(b.second - centroid.second, b.first - centroid.first);
        if (angle_b < 0) angle_b = angle_b + (2 * M_PI);
        if (0 <= angle_a && angle_a <= M_PI / 2 && 3 * M_PI / 2 <= angle_b && angle_b <= 2 * M_PI) return false;
        if (0 <= angle_b && angle_b <= M_PI / 2 && 3 * M_PI / 2 <= angle_a && angle_a <= 2 * M_PI) return true;
        return angle_a < angle_b;
    }
};

}  // namespace

extern "C" {

// Returns the number of records (only the first max_out are stored), or -1 for an invalid seed.  cell_piece [ny*nx]: the sequence
// number of the piece (emitted or dropped) a cell was collected into, numbered as the oracle numbers them; every_cells: the cells in
// emission order (every_frontier_list).  *guarded: pieces whose std::sort the header's guard would have stopped (their goal point
// comes from the header's restatement here, as on the device).
int32_t fr_search(const int32_t *labels, int32_t nx, int32_t ny, double ox, double oy, double res, int32_t robot_cell,
                  int32_t min_size, int32_t max_size, int32_t n_seeds, const int32_t *seeds, int32_t max_out, double *goal_xy,
                  int32_t *size, int32_t *label, int32_t *goal_cell, int32_t *seed_cell, int32_t *cell_piece, int32_t *every_cells,
                  int64_t *n_every, int32_t *guarded)
{
    const Grid g{nx, ny, ox, oy, res};
    const int n = nx * ny;
    std::vector<int> seed_list;
    if (seeds) {
        std::vector<char> taken(n, 0);
        for (int k = 0; k < n_seeds; ++k) {
            const int s = seeds[k];
            if (s < 0 || s >= n || labels[s] < 0 || taken[labels[s]]) return -1;
            taken[labels[s]] = 1;
            seed_list.push_back(s);
        }
    } else {
        const int rx = robot_cell % nx, ry = robot_cell / nx;
        std::vector<std::pair<long long, int>> best(n, {-1, -1});
        for (int i = 0; i < n; ++i) {
            const int l = labels[i];
            if (l < 0) continue;
            const long long dx = i % nx - rx, dy = i / nx - ry, d2 = dx * dx + dy * dy;
            if (best[l].second < 0 || d2 < best[l].first) best[l] = {d2, i};
        }
        for (int l = 0; l < n; ++l)
            if (best[l].second >= 0) seed_list.push_back(best[l].second);
    }
    for (int i = 0; i < n; ++i) cell_piece[i] = -1;
    std::vector<char> claimed(n, 0);
    int32_t n_out = 0, piece_seq = 0;
    int64_t every = 0;
    *guarded = 0;
    auto finish = [&](std::vector<std::pair<double, double>> &cells, std::vector<int> &ids, int count, int lab, int seed) {
        const auto c = centroid_of_cells(cells, res, res * 1.414 * 2);
        std::vector<fs_msort_elem> e(cells.size());
        for (size_t k = 0; k < cells.size(); ++k) e[k] = {fs_msort_angle(cells[k].second - c.second, cells[k].first - c.first), ids[k]};
        const int32_t gd = fs_msort_sort(e.data(), (int64_t)e.size());
        int goal;
        if (gd == 0) {                                        // the reference's own call
            std::vector<std::pair<std::pair<double, double>, int>> v(cells.size());
            for (size_t k = 0; k < cells.size(); ++k) v[k] = {cells[k], ids[k]};
            SortByMedianFunctor f{c};
            std::sort(v.begin(), v.end(), [&](const auto &a, const auto &b) { return f(a.first, b.first); });
            goal = v[v.size() / 2].second;
        } else {
            ++*guarded;
            goal = e[e.size() / 2].cell;
        }
        if (count > min_size) {                               // searchFrom's filter (:81)
            if (n_out < max_out) {
                const auto w = g.world(goal);
                goal_xy[2 * n_out] = w.first; goal_xy[2 * n_out + 1] = w.second;
                size[n_out] = count; label[n_out] = lab; goal_cell[n_out] = goal; seed_cell[n_out] = seed;
            }
            ++n_out;
        }
        cells.clear();
        ids.clear();
    };
    for (const int seed : seed_list) {
        const int lab = labels[seed];
        int count = 1;
        std::vector<std::pair<double, double>> cells{g.world(seed)};
        std::vector<int> ids{seed};
        claimed[seed] = 1;
        cell_piece[seed] = piece_seq;
        every_cells[every++] = seed;
        std::queue<int> q;
        q.push(seed);
        int nb[8];
        while (!q.empty()) {
            const int idx = q.front();
            q.pop();
            const int k = g.nhood8(idx, nb);
            for (int j = 0; j < k; ++j) {
                const int m = nb[j];
                if (labels[m] != lab || claimed[m]) continue;
                claimed[m] = 1;
                cells.push_back(g.world(m));
                ids.push_back(m);
                cell_piece[m] = piece_seq;
                every_cells[every++] = m;
                ++count;
                q.push(m);
                if (count > max_size) {
                    finish(cells, ids, count, lab, seed);
                    ++piece_seq;
                    count = 0;
                }
            }
        }
        if (count > min_size) finish(cells, ids, count, lab, seed);
        ++piece_seq;
    }
    *n_every = every;
    return n_out;
}

// the header's restatement against std::sort over (value, id) pairs compared by value: plain < (mode 0) or SortByMedianFunctor's
// angle rule (mode 1).  Returns 1 when equal element for element, 0 when not, -1 when the restatement's guard fired (std::sort
// would have left the array: not run).
int32_t fr_sort_check(const double *values, int32_t n, int32_t mode, int32_t *restated_ids)
{
    struct E { double v; int32_t id; };
    std::vector<E> a(n), b(n);
    for (int k = 0; k < n; ++k) a[k] = b[k] = {values[k], k};
    int32_t guarded;
    if (mode == 0) {
        auto lt = [](const E &u, const E &v) { return u.v < v.v; };
        fs_msort<E, decltype(lt)> s{a.data(), (int64_t)n, lt, 0};
        s.sort();
        guarded = s.guarded;
        if (!guarded) std::sort(b.begin(), b.end(), lt);
    } else {
        auto lt = [](const E &u, const E &v) { return fs_msort_less(u.v, v.v); };
        fs_msort<E, decltype(lt)> s{a.data(), (int64_t)n, lt, 0};
        s.sort();
        guarded = s.guarded;
        if (!guarded) std::sort(b.begin(), b.end(), lt);
    }
    for (int k = 0; k < n; ++k) restated_ids[k] = a[k].id;
    if (guarded) return -1;
    for (int k = 0; k < n; ++k)
        if (a[k].id != b[k].id) return 0;
    return 1;
}

}  // extern "C"
