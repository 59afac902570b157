// roadmap_astar_ref.cpp — host driver of fit-slam_amd/csrc/fs_roadmap_astar.h, the per-goal A* that the device's REFERENCE roadmap
// search runs.  Test infrastructure: built by tests/test_roadmap_astar_restatement.py with
// `g++ -O2 -ffp-contract=off -shared -fPIC` and loaded through ctypes.
#include <stdint.h>

#include <queue>
#include <vector>

#include "../../fit-slam_amd/csrc/fs_roadmap_astar.h"

namespace {

struct Entry {
    double f;
    int32_t id;
};
struct FCompare {
    bool operator()(const Entry &a, const Entry &b) const { return a.f > b.f; }
};

}  // namespace

extern "C" {

// A sequence of heap operations: op[i] >= 0 pushes (f[op[i]], id i), op[i] < 0 pops.  popped[k] = the id of the k-th pop, by the
// header's heap (std_queue == 0) or by std::priority_queue with the reference's comparator (std_queue == 1).  Returns the pops.
int ra_heap_sequence(int n, const int32_t *op, const double *f, int std_queue, int32_t *popped)
{
    int k = 0;
    if (std_queue) {
        std::priority_queue<Entry, std::vector<Entry>, FCompare> q;
        for (int i = 0; i < n; ++i) {
            if (op[i] >= 0) q.push(Entry{f[op[i]], i});
            else if (!q.empty()) { popped[k++] = q.top().id; q.pop(); }
        }
        return k;
    }
    std::vector<double> hf((size_t)n + 1);
    std::vector<int32_t> hr((size_t)n + 1);
    int32_t size = 0;
    for (int i = 0; i < n; ++i) {
        if (op[i] >= 0) fs_astar_push(hf.data(), hr.data(), size, f[op[i]], i);
        else if (size > 0) popped[k++] = fs_astar_pop(hf.data(), hr.data(), size);
    }
    return k;
}

// fs_astar_run from node `start` to node `goal` on a CSR roadmap with room for `cap` records.  Returns FS_ASTAR_FOUND (0, *len
// set), FS_ASTAR_NO_PATH (1) or FS_ASTAR_OVERFLOW (2); *pops the records popped.
int ra_astar(int n, const double *xy, const int32_t *row, const int32_t *col, int start, int goal, int cap, double *len, int32_t *pops)
{
    std::vector<double> hf((size_t)cap), rg((size_t)cap);
    std::vector<int32_t> hr((size_t)cap), rn((size_t)cap), rp((size_t)cap), best((size_t)n, -1);
    std::vector<uint8_t> closed((size_t)n, 0);
    const fs_astar_mem m{hf.data(), hr.data(), rn.data(), rg.data(), rp.data(), best.data(), closed.data(), cap};
    const fs_astar_graph g{n, xy, row, col};
    return fs_astar_run(g, m, start, goal, len, pops);
}

}  // extern "C"
