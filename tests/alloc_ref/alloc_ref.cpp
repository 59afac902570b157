// alloc_ref.cpp — CPU restatement of the reference's multi-robot task allocator: MinPosAlgo's rank matrix and
// modified cost matrix (minPos.cpp:20-44) and HungarianAlgorithm::Solve (Hungarian.cpp:25-395), written as one loop over the
// steps on a row-major matrix, with one starred column per row, one starred row per column and one primed column per row where
// the reference keeps three R x n boolean matrices and recurses from step to step.  Compiled by tests/alloc_ref.py with
// g++ -O2 -ffp-contract=off; the GPU kernel (fit-slam_amd/csrc/fs_allocate.hip) is compared with it bit for bit.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <vector>

namespace {

inline bool is_zero(double x) { return std::fabs(x) < DBL_EPSILON; }

}  // namespace

extern "C" {

// P[i][j] = robots k != i strictly closer to frontier j than robot i; modified = cost where P == 0, DBL_MAX elsewhere
void ar_minpos(int R, int n, const double *cost, const double *distance, int32_t *P, double *modified)
{
    for (int i = 0; i < R; ++i)
        for (int j = 0; j < n; ++j) {
            int count = 0;
            for (int k = 0; k < R; ++k)
                if (k != i && distance[(size_t)k * n + j] < distance[(size_t)i * n + j]) ++count;
            P[(size_t)i * n + j] = count;
            modified[(size_t)i * n + j] = count == 0 ? cost[(size_t)i * n + j] : DBL_MAX;
        }
}

// Munkres on cost [R][n] row-major.  assignment [R] (-1: none), *total summed over `cost` in ascending row order.
// stats [3]: augmentations, step-5 runs, step-3 primes.  Returns 0, or 1 when step 5 ran more than (R + 1) * (min(R, n) + 1) times.
int ar_solve(int R, int n, const double *cost, int32_t *assignment, double *total, int64_t *stats)
{
    const size_t N = (size_t)n;
    std::vector<double> D(cost, cost + (size_t)R * N);
    std::vector<int32_t> star_of_row(R, -1), star_of_col(n, -1), prime_of_row(R, -1);
    std::vector<uint8_t> row_covered(R, 0), col_covered(n, 0);
    int64_t augmentations = 0, step5 = 0, primes = 0;
    const int64_t cap = (int64_t)(R + 1) * ((R < n ? R : n) + 1);
    int min_dim;
    if (R <= n) {
        min_dim = R;
        for (int r = 0; r < R; ++r) {
            double m = D[r * N];
            for (int c = 1; c < n; ++c)
                if (D[r * N + c] < m) m = D[r * N + c];
            for (int c = 0; c < n; ++c) D[r * N + c] -= m;
        }
        for (int r = 0; r < R; ++r)
            for (int c = 0; c < n; ++c)
                if (is_zero(D[r * N + c]) && !col_covered[c]) {
                    star_of_row[r] = c; star_of_col[c] = r; col_covered[c] = 1;
                    break;
                }
    } else {
        min_dim = n;
        for (int c = 0; c < n; ++c) {
            double m = D[c];
            for (int r = 1; r < R; ++r)
                if (D[r * N + c] < m) m = D[r * N + c];
            for (int r = 0; r < R; ++r) D[r * N + c] -= m;
        }
        for (int c = 0; c < n; ++c)
            for (int r = 0; r < R; ++r)
                if (is_zero(D[r * N + c]) && star_of_row[r] < 0) {      // (the row marks of this phase are exactly the starred rows)
                    star_of_row[r] = c; star_of_col[c] = r; col_covered[c] = 1;
                    break;
                }
    }
    int rc = 0;
    for (;;) {
        // step 2b
        int covered = 0;
        for (int c = 0; c < n; ++c) covered += col_covered[c];
        if (covered == min_dim) break;
        // steps 3 and 5 until a primed zero sits in a row without a star
        int path_row = -1, path_col = -1;
        while (path_row < 0) {
            bool primed = false;
            for (int c = 0; c < n && path_row < 0; ++c) {
                if (col_covered[c]) continue;
                for (int r = 0; r < R; ++r) {
                    if (row_covered[r] || !is_zero(D[r * N + c])) continue;
                    prime_of_row[r] = c;
                    ++primes;
                    if (star_of_row[r] < 0) { path_row = r; path_col = c; }
                    else { row_covered[r] = 1; col_covered[star_of_row[r]] = 0; primed = true; }
                    break;
                }
            }
            if (path_row >= 0 || primed) continue;
            // step 5
            if (++step5 > cap) { rc = 1; break; }
            double h = DBL_MAX;
            for (int r = 0; r < R; ++r)
                if (!row_covered[r])
                    for (int c = 0; c < n; ++c)
                        if (!col_covered[c] && D[r * N + c] < h) h = D[r * N + c];
            for (int r = 0; r < R; ++r)
                if (row_covered[r])
                    for (int c = 0; c < n; ++c) D[r * N + c] += h;
            for (int c = 0; c < n; ++c)
                if (!col_covered[c])
                    for (int r = 0; r < R; ++r) D[r * N + c] -= h;
        }
        if (rc) break;
        // step 4: the alternating path from the primed zero, on the stars as they were
        ++augmentations;
        for (int r = path_row, c = path_col;;) {
            const int displaced = star_of_col[c];
            star_of_col[c] = r; star_of_row[r] = c;
            if (displaced < 0) break;
            r = displaced; c = prime_of_row[r];
        }
        for (int r = 0; r < R; ++r) { prime_of_row[r] = -1; row_covered[r] = 0; }
        // step 2a
        for (int c = 0; c < n; ++c)
            if (star_of_col[c] >= 0) col_covered[c] = 1;
    }
    double sum = 0;
    for (int r = 0; r < R; ++r) {
        assignment[r] = rc ? -1 : star_of_row[r];
        if (!rc && star_of_row[r] >= 0) sum += cost[r * N + star_of_row[r]];
    }
    *total = sum;
    if (stats) { stats[0] = augmentations; stats[1] = step5; stats[2] = primes; }
    return rc;
}

}  // extern "C"
