// extern "C" entry points into the reference's task allocator as compiled from its own sources (oracle/ref_build.py):
// HungarianAlgorithm::Solve and MinPosAlgo::getAssignmentMinPos on row-major matrices.
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <vector>

#include "frontier_multirobot_allocator/hungarian/Hungarian.h"
#include "frontier_multirobot_allocator/minPos/minPos.hpp"
#include "quiet.hpp"

namespace {

std::vector<std::vector<double>> rows(int R, int n, const double *m)
{
    std::vector<std::vector<double>> out((size_t)R);
    for (int r = 0; r < R; ++r) out[r].assign(m + (size_t)r * n, m + (size_t)(r + 1) * n);
    return out;
}

void store(const std::vector<int> &a, int R, int32_t *assignment)
{
    for (int r = 0; r < R; ++r) assignment[r] = r < (int)a.size() ? a[r] : -1;
}

}  // namespace

extern "C" {

// cost [R][n]; assignment [R] (the column of each row, -1: none); returns Solve's total
double ref_hungarian(int R, int n, const double *cost, int32_t *assignment)
{
    ref_wrap::Quiet quiet;
    std::vector<std::vector<double>> c = rows(R, n, cost);
    std::vector<int> a;
    HungarianAlgorithm solver;
    const double total = solver.Solve(c, a);
    store(a, R, assignment);
    return total;
}

// cost, distance [R][n]; assignment [R]; returns getAssignmentMinPos' total (summed over the modified matrix)
double ref_minpos(int R, int n, const double *cost, const double *distance, int32_t *assignment)
{
    ref_wrap::Quiet quiet;
    std::vector<std::vector<double>> c = rows(R, n, cost), d = rows(R, n, distance);
    std::vector<int> a;
    MinPosAlgo algo(d, c);
    const double total = algo.getAssignmentMinPos(a);
    store(a, R, assignment);
    return total;
}

}  // extern "C"
