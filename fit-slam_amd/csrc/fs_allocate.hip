// fs_allocate.hip — the multi-robot task allocator on the GPU: TaskAllocator::solveAllocationHungarian /
// solveAllocationMinPos (DEPX/frontier_multirobot_allocator/taskAllocator.cpp:7-66), that is MinPosAlgo's rank matrix and modified
// cost matrix (minPos/minPos.cpp:20-44,88-98) and HungarianAlgorithm::Solve (hungarian/Hungarian.cpp:25-395), bit for bit.
//
// ONE workgroup runs the whole state machine in one launch: the checks, MinPos, the reduction and the greedy stars, then steps
// 2b / 3 / 4 / 2a / 5 until min(R, n) columns are covered.  There is at most one star per row and per column and at most one prime
// per row, so the reference's three R x n boolean matrices are star_of_row[R], star_of_col[n], prime_of_row[R] in LDS beside the
// column covers; the row covers are one 64-bit word.  The working copy D stays in global memory, row-major: lanes span
// consecutive columns.  Every "first in scan order" of the reference is a workgroup-wide minimum over a key that grows in that
// order; step 3's is col * R + row with a lower bound on the column, taken chunk by chunk of blockDim.x columns, so a pass stops
// reading at the first chunk that holds a zero.  The only reduction over values is a minimum (exact in any order; values that are
// not < DBL_MAX count as DBL_MAX, which is what the reference's strict `<` scan from DBL_MAX makes of them), everything else is
// elementwise in the reference's operation order: identical bits.
#include "fs_internal.h"

#include <cfloat>
#include <climits>

namespace {

#define AL_NONE INT_MAX

struct AlShared {
    int32_t star_of_col[FS_ALLOC_MAX_TASKS];
    uint8_t col_covered[FS_ALLOC_MAX_TASKS];
    int32_t star_of_row[FS_ALLOC_MAX_ROBOTS], prime_of_row[FS_ALLOC_MAX_ROBOTS];
    unsigned long long row_covered;          // bit r: row r is covered
    double red_d[16];
    int32_t red_i[16];
};

__device__ __forceinline__ bool al_zero(double x) { return fabs(x) < DBL_EPSILON; }

// workgroup-wide minimum / sum of an int, minimum of a double: every thread gets the result (two barriers each)
__device__ __forceinline__ int32_t al_block_min(AlShared &s, int32_t x)
{
    for (int d = 32; d >= 1; d >>= 1) { const int32_t o = __shfl_xor(x, d); x = (o < x) ? o : x; }
    if ((threadIdx.x & 63) == 0) s.red_i[threadIdx.x >> 6] = x;
    __syncthreads();
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) x = (s.red_i[w] < x) ? s.red_i[w] : x;
    __syncthreads();
    return x;
}
__device__ __forceinline__ int32_t al_block_sum(AlShared &s, int32_t x)
{
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d);
    if ((threadIdx.x & 63) == 0) s.red_i[threadIdx.x >> 6] = x;
    __syncthreads();
    x = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) x += s.red_i[w];
    __syncthreads();
    return x;
}
__device__ __forceinline__ double al_block_min(AlShared &s, double x)
{
    for (int d = 32; d >= 1; d >>= 1) { const double o = __shfl_xor(x, d); x = (o < x) ? o : x; }
    if ((threadIdx.x & 63) == 0) s.red_d[threadIdx.x >> 6] = x;
    __syncthreads();
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) x = (s.red_d[w] < x) ? s.red_d[w] : x;
    __syncthreads();
    return x;
}

__device__ __forceinline__ bool al_entry_ok(double v) { return v >= 0.0 && v <= DBL_MAX; }      // (false for NaN, negative, +inf)

__global__ __launch_bounds__(1024)
void fs_allocate_kernel(FsAllocArgs a)
{
    __shared__ AlShared s;
    const int R = a.n_robots, n = a.n_tasks, T = blockDim.x, tid = threadIdx.x;
    const size_t N = (size_t)n;
    const int64_t total_elems = (int64_t)R * n;

    // ---- the refusals: nothing is written but the status
    int bad = 0;
    for (int64_t i = tid; i < total_elems; i += T) {
        if (!al_entry_ok(a.cost[i])) bad = 1;
        if (a.method == FS_ALLOC_MINPOS && !al_entry_ok(a.distance[i])) bad = 1;
    }
    if (al_block_sum(s, bad) > 0) {
        if (tid == 0) *a.status = FS_E_INVALID;
        return;
    }

    // ---- MinPos: P and the modified matrix M (the solve's input); HUNGARIAN solves on the cost matrix itself
    const double *M = a.cost;
    if (a.method == FS_ALLOC_MINPOS) {
        for (int j = tid; j < n; j += T)
            for (int i = 0; i < R; ++i) {
                const double di = a.distance[i * N + j];
                int count = 0;
                for (int k = 0; k < R; ++k) count += (k != i && a.distance[k * N + j] < di) ? 1 : 0;
                if (a.rank) a.rank[i * N + j] = count;
                a.modified[i * N + j] = count == 0 ? a.cost[i * N + j] : DBL_MAX;
            }
        M = a.modified;
        __syncthreads();
    }

    // ---- the working copy, reduced, and the greedy stars (Hungarian.cpp:92-168)
    double *D = a.work;
    for (int c = tid; c < n; c += T) { s.star_of_col[c] = -1; s.col_covered[c] = 0; }
    if (tid < FS_ALLOC_MAX_ROBOTS) { s.star_of_row[tid] = -1; s.prime_of_row[tid] = -1; }
    if (tid == 0) s.row_covered = 0ull;
    const int wave = tid >> 6, lane = tid & 63, waves = T >> 6;
    int min_dim;
    if (R <= n) {
        min_dim = R;
        for (int r = wave; r < R; r += waves) {                  // a wave per row
            double m = DBL_MAX;
            for (int c = lane; c < n; c += 64) { const double v = M[r * N + c]; m = (v < m) ? v : m; }
            for (int d = 32; d >= 1; d >>= 1) { const double o = __shfl_xor(m, d); m = (o < m) ? o : m; }
            for (int c = lane; c < n; c += 64) D[r * N + c] = M[r * N + c] - m;
        }
        __syncthreads();
        for (int r = 0; r < R; ++r) {
            int32_t cand = AL_NONE;
            for (int c = tid; c < n; c += T)
                if (!s.col_covered[c] && al_zero(D[r * N + c])) { cand = c; break; }
            const int32_t c = al_block_min(s, cand);
            if (c != AL_NONE && tid == 0) { s.star_of_row[r] = c; s.star_of_col[c] = r; s.col_covered[c] = 1; }
            __syncthreads();
        }
    } else {
        min_dim = n;                                             // (n < R <= 64: a lane per column, then a lane per row)
        for (int c = tid; c < n; c += T) {
            double m = DBL_MAX;
            for (int r = 0; r < R; ++r) { const double v = M[r * N + c]; m = (v < m) ? v : m; }
            for (int r = 0; r < R; ++r) D[r * N + c] = M[r * N + c] - m;
        }
        __syncthreads();
        if (wave == 0) {
            unsigned long long starred = 0ull;                   // the rows marked so far (uniform across the wave)
            for (int c = 0; c < n; ++c) {
                const bool z = lane < R && !((starred >> lane) & 1ull) && al_zero(D[lane * N + c]);
                const unsigned long long m = __ballot(z);
                if (m) {
                    const int r = __ffsll((long long)m) - 1;
                    starred |= 1ull << r;
                    if (lane == 0) { s.star_of_row[r] = c; s.star_of_col[c] = r; s.col_covered[c] = 1; }
                }
            }
        }
        __syncthreads();
    }

    int32_t augmentations = 0, step5 = 0, primes = 0, rc = FS_OK;
    const int64_t cap = (int64_t)(R + 1) * (min_dim + 1);
    for (;;) {
        // ---- step 2b
        int covered = 0;
        for (int c = tid; c < n; c += T) covered += s.col_covered[c];
        if (al_block_sum(s, covered) == min_dim) break;
        // ---- steps 3 and 5 until a primed zero sits in a row without a star
        int path_row = -1, path_col = -1;
        while (path_row < 0) {
            // one pass of step 3 over the columns in ascending order
            bool primed = false;
            double vmin = DBL_MAX;            // this thread's minimum over the uncovered entries it read (step 5's h if the pass finds nothing)
            int lb = 0;
            while (lb < n) {
                const unsigned long long rows = s.row_covered;
                int32_t cand = AL_NONE;
                const int c = lb + tid;
                if (c < n && !s.col_covered[c])
                    for (int r = 0; r < R; ++r) {
                        if ((rows >> r) & 1ull) continue;
                        const double v = D[r * N + c];
                        vmin = (v < vmin) ? v : vmin;
                        if (al_zero(v)) { cand = c * R + r; break; }
                    }
                const int32_t key = al_block_min(s, cand);
                if (key == AL_NONE) { lb += T; continue; }
                const int c0 = key / R, r0 = key - c0 * R;
                ++primes;
                const int32_t sc = s.star_of_row[r0];          // (stars do not move during a pass)
                if (tid == 0) s.prime_of_row[r0] = c0;
                if (sc < 0) { path_row = r0; path_col = c0; break; }
                if (tid == 0) { s.row_covered |= 1ull << r0; s.col_covered[sc] = 0; }
                __syncthreads();
                primed = true;
                lb = c0 + 1;
            }
            if (path_row >= 0 || primed) continue;
            // ---- step 5 (the pass above read every uncovered entry under the covers that still hold)
            if (++step5 > cap) { rc = FS_E_RANGE; break; }
            const double h = al_block_min(s, vmin);
            const unsigned long long rows = s.row_covered;
            for (int r = 0; r < R; ++r) {
                const bool add = (rows >> r) & 1ull;
                for (int c = tid; c < n; c += T) {
                    const bool sub = !s.col_covered[c];
                    if (!add && !sub) continue;
                    double x = D[r * N + c];
                    if (add) x += h;                             // (x + h) - h where both apply: two roundings, in this order
                    if (sub) x -= h;
                    D[r * N + c] = x;
                }
            }
            __syncthreads();
        }
        if (rc) break;
        // ---- step 4: the alternating path from the primed zero on the stars as they were; primes cleared, rows uncovered
        ++augmentations;
        __syncthreads();
        if (tid == 0) {
            int r = path_row, c = path_col;
            for (int guard = 0; guard <= R; ++guard) {
                const int displaced = s.star_of_col[c];
                s.star_of_col[c] = r; s.star_of_row[r] = c;
                if (displaced < 0) break;
                r = displaced; c = s.prime_of_row[r];
                if (c < 0) break;                                // (cannot happen: a star in an uncovered column has a primed row)
            }
            s.row_covered = 0ull;
        }
        __syncthreads();
        if (tid < FS_ALLOC_MAX_ROBOTS) s.prime_of_row[tid] = -1;
        __syncthreads();
        // ---- step 2a: covers are only added
        for (int c = tid; c < n; c += T)
            if (s.star_of_col[c] >= 0) s.col_covered[c] = 1;
        __syncthreads();
    }

    // ---- the result: the sum is sequential in ascending row order, so one lane does it
    if (tid == 0) {
        a.stats[0] = augmentations; a.stats[1] = step5; a.stats[2] = primes;
        *a.status = rc;
        if (rc == FS_OK) {
            double sum = 0;
            for (int r = 0; r < R; ++r) {
                const int32_t c = s.star_of_row[r];
                a.assignment[r] = c;
                if (c >= 0) sum += M[r * N + c];
                if (a.assigned_cost) a.assigned_cost[r] = c >= 0 ? a.cost[r * N + c] : __longlong_as_double(0x7ff8000000000000ll);
            }
            *a.total_cost = sum;
        }
    }
}

}  // namespace

hipError_t fs_launch_allocate(const FsAllocArgs &a, hipStream_t s)
{
    // lanes span columns: as many threads as columns, in whole waves, up to one full workgroup
    int threads = ((a.n_tasks + 63) / 64) * 64;
    threads = threads < 64 ? 64 : threads > 1024 ? 1024 : threads;
    hipLaunchKernelGGL(fs_allocate_kernel, dim3(1), dim3(threads), 0, s, a);
    return hipGetLastError();
}
