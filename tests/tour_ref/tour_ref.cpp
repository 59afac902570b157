// CPU restatement of FullPathOptimizer::getNextGoal's selection and tour search, the checker of
// fs_roadmap_next_goal.  Reference: DEP/src/FullPathOptimizer.cpp — getFilteredFrontiersN (:157-227), calculatePathLength
// (:371-420), getBestFullPath (:422-538), getNextGoal (:548-661); FullPathOptimizer.hpp:12-20, 118-130.
//
// Written from the reference's text, not from the device code: the tour search is the reference's loop itself (every order of the
// locals by std::next_permutation from the selection order, the minimum-length tours collected in enumeration order, then the
// first strict minimum of the robot leg), and a Held-Karp dynamic programme gives the optimum length on its own.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

extern "C" {

// isAchievable() && !isBlacklisted() && !isInBlacklistedRegion(): distance to a circle centre < 1.7 (BLACKLISTING_CIRCLE_RADIUS)
void tr_eligible(int n, const double *goal_xyz, const uint8_t *achievable, const uint8_t *blacklisted, int n_circles,
                 const double *circle_xy, uint8_t *out)
{
    for (int i = 0; i < n; ++i) {
        bool ok = achievable[i] && !(blacklisted && blacklisted[i]);
        for (int b = 0; ok && b < n_circles; ++b)
            if (std::sqrt(std::pow(goal_xyz[3 * i] - circle_xy[2 * b], 2) + std::pow(goal_xyz[3 * i + 1] - circle_xy[2 * b + 1], 2)) < 1.7)
                ok = false;
        out[i] = ok;
    }
}

// getFilteredFrontiersN over the eligible frontiers, sorted by path length (stable: ties to the lower index).  Returns the closest
// global (-1: unset); loc / glob receive the lists.
int tr_select(int n, const double *plm, const uint8_t *eligible, int n_local, double radius, int *loc, int *n_loc, int *glob, int *n_glob)
{
    std::vector<int> all;
    for (int i = 0; i < n; ++i) if (eligible[i]) all.push_back(i);
    std::stable_sort(all.begin(), all.end(), [plm](int a, int b) { return plm[a] < plm[b]; });
    std::vector<int> L, G;
    int closest = -1;
    if (!all.empty()) {
        bool global_assigned = false, need_to_pop = false;
        size_t counter = 1;
        for (int f : all) {
            if (plm[f] <= radius && counter <= (size_t)n_local) {
                L.push_back(f); closest = f; need_to_pop = true;
            } else if (plm[f] <= radius && counter > (size_t)n_local) {
                closest = f; need_to_pop = false;
            } else if (plm[f] > radius) {
                if (!global_assigned) { closest = f; global_assigned = true; }
                need_to_pop = false;
                G.push_back(f);
            }
            counter++;
        }
        if (need_to_pop) L.pop_back();
        if (G.empty() && L.empty()) G.push_back(closest);
    }
    std::copy(L.begin(), L.end(), loc); *n_loc = (int)L.size();
    std::copy(G.begin(), G.end(), glob); *n_glob = (int)G.size();
    return closest;
}

// getBestFullPath over the matrix M [(k+2)^2] of the nodes [robot, locals 1..k, global k+1]: every permutation of the locals from
// the identity, calculatePathLength summed left to right from 0.0, bestPaths in enumeration order, then the first strict minimum of
// calculateLengthRobotToGoal (M[0][first local]).  perm [k]: the winner's positions; returns the number of tours tried.
long long tr_tour(int k, const double *M, double *min_length, long long *n_best, int *perm)
{
    const int m = k + 2;
    std::vector<int> p(k);
    for (int i = 0; i < k; ++i) p[i] = i;
    double minLength = std::numeric_limits<double>::max();
    std::vector<std::vector<int>> bestPaths;
    long long tried = 0;
    do {
        std::vector<int> path(1, 0);
        for (int i = 0; i < k; ++i) path.push_back(p[i] + 1);
        path.push_back(k + 1);
        double total = 0.0;
        for (size_t i = 0; i + 1 < path.size(); ++i) total += M[path[i] * m + path[i + 1]];
        if (total < minLength) { minLength = total; bestPaths.clear(); bestPaths.push_back(p); }
        else if (total == minLength) bestPaths.push_back(p);
        ++tried;
    } while (std::next_permutation(p.begin(), p.end()));
    *min_length = minLength;
    *n_best = (long long)bestPaths.size();
    double leg = std::numeric_limits<double>::max();
    for (const auto &b : bestPaths) {
        const double d = 0.0 + M[0 * m + b[0] + 1];
        if (d < leg) { leg = d; std::copy(b.begin(), b.end(), perm); }
    }
    return tried;
}

// Held-Karp: the minimum over orders of the locals of robot -> locals -> global, by subsets (an independent check of the optimum)
double tr_held_karp(int k, const double *M)
{
    const int m = k + 2;
    const double inf = std::numeric_limits<double>::infinity();
    std::vector<double> D((size_t)1 << k, inf);
    std::vector<std::vector<double>> best((size_t)1 << k, std::vector<double>(k, inf));
    for (int j = 0; j < k; ++j) best[(size_t)1 << j][j] = M[0 * m + j + 1];
    for (size_t S = 1; S < ((size_t)1 << k); ++S)
        for (int j = 0; j < k; ++j) {
            if (!(S >> j & 1) || best[S][j] == inf) continue;
            for (int q = 0; q < k; ++q) {
                if (S >> q & 1) continue;
                const size_t T = S | ((size_t)1 << q);
                best[T][q] = std::min(best[T][q], best[S][j] + M[(j + 1) * m + q + 1]);
            }
        }
    double opt = inf;
    const size_t all = ((size_t)1 << k) - 1;
    for (int j = 0; j < k; ++j) opt = std::min(opt, best[all][j] + M[(j + 1) * m + k + 1]);
    return opt;
}

}  // extern "C"
