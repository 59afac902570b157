// fs_roadmap_astar.h — the roadmap planner's per-goal A* (FrontierRoadmapAStar::getPlan, DEP/src/planners/astar.cpp:42-93) as the
// reference runs it, for the REFERENCE roadmap search.  The device (fs_roadmap.hip) and a host test compile this
// same source, as they do fs_median_sort.h.
//
// The open list is std::priority_queue<node, vector, FCompare> with FCompare(a, b) = a->f > b->f: push = push_back + std::push_heap,
// pop = std::pop_heap + pop_back.  Ties in f are frequent on lattice-like roadmaps and their order decides which equal-f record is
// expanded first, so libstdc++'s __push_heap and __adjust_heap are restated step for step; an entry is (f, record id) and the
// comparator reads f alone.
//
// A record is what one make_shared<Node> of the reference holds: (node, g, parent record).  best[v] is all[v], the latest record of
// node v (-1: none); closed[v] is the closed set.  The search, as the reference writes it:
//   - f = g + h, h(v) = the SQUARED distance from v to the goal node (ex * ex + ey * ey), g grows by the squared segment length;
//   - the goal test compares positions, and the path runs from all[popped node] up the parent records;
//   - the closed set is tested for successors only: a stale pop is expanded again, with the popped record's own g;
//   - a successor is accepted when it has no record or its record's g is strictly larger; its parent is all[popped node];
//   - the length is the sum of sqrt(squared segment) from the goal end.
// Nodes are keyed by index (the reference keys them by an int-truncated UID of the position).
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FS_ASTAR_HD __host__ __device__
#else
#define FS_ASTAR_HD
#endif

enum { FS_ASTAR_FOUND = 0, FS_ASTAR_NO_PATH = 1, FS_ASTAR_OVERFLOW = 2 };

// A search's storage: the heap, the records and the per-node state.  `cap` bounds the records, and so the heap (every heap entry
// is a distinct record).  The device points these at LDS or at global memory.
struct fs_astar_mem {
    double *heap_f;
    int32_t *heap_rec;
    int32_t *rec_node;
    double *rec_g;
    int32_t *rec_parent;
    int32_t *best;          // [n]
    uint8_t *closed;        // [n]
    int32_t cap;
};

// the roadmap: positions and the adjacency lists (CSR, the reference's list order)
struct fs_astar_graph {
    int32_t n;
    const double *xy;
    const int32_t *row, *col;
};

// sqDistanceBetweenFrontiers(a, b): pow(e, 2) written e * e
FS_ASTAR_HD inline double fs_astar_sq(const double *xy, int32_t a, int32_t b)
{
    const double ex = xy[2 * a] - xy[2 * b], ey = xy[2 * a + 1] - xy[2 * b + 1];
    return ex * ex + ey * ey;
}

// std::__push_heap(first, hole, top = 0, value) with comp(parent, value) = parent.f > value.f
FS_ASTAR_HD inline void fs_astar_sift_up(double *hf, int32_t *hr, int32_t hole, double f, int32_t r)
{
    int32_t parent = (hole - 1) / 2;
    while (hole > 0 && hf[parent] > f) {
        hf[hole] = hf[parent]; hr[hole] = hr[parent];
        hole = parent;
        parent = (hole - 1) / 2;
    }
    hf[hole] = f; hr[hole] = r;
}

// priority_queue::push: push_back, then std::push_heap
FS_ASTAR_HD inline void fs_astar_push(double *hf, int32_t *hr, int32_t &size, double f, int32_t r)
{
    fs_astar_sift_up(hf, hr, size, f, r);
    ++size;
}

// priority_queue::pop after top(): std::pop_heap (the last entry sifted from the root by __adjust_heap over size - 1 entries), then
// pop_back.  Returns the top's record.
FS_ASTAR_HD inline int32_t fs_astar_pop(double *hf, int32_t *hr, int32_t &size)
{
    const int32_t top = hr[0];
    if (size > 1) {
        const int32_t len = size - 1;
        const double vf = hf[len];
        const int32_t vr = hr[len];
        int32_t hole = 0, child = 0;
        while (child < (len - 1) / 2) {
            child = 2 * (child + 1);
            if (hf[child] > hf[child - 1]) child--;
            hf[hole] = hf[child]; hr[hole] = hr[child];
            hole = child;
        }
        if ((len & 1) == 0 && child == (len - 2) / 2) {
            child = 2 * (child + 1);
            hf[hole] = hf[child - 1]; hr[hole] = hr[child - 1];
            hole = child - 1;
        }
        fs_astar_sift_up(hf, hr, hole, vf, vr);
    }
    --size;
    return top;
}

// the start record: all[start] = s, open.push(s) with f = 0
FS_ASTAR_HD inline void fs_astar_begin(const fs_astar_mem &m, int32_t start, int32_t &nrec, int32_t &hsize)
{
    m.rec_node[0] = start; m.rec_g[0] = 0.0; m.rec_parent[0] = -1;
    m.best[start] = 0;
    hsize = 0;
    fs_astar_push(m.heap_f, m.heap_rec, hsize, 0.0, 0);
    nrec = 1;
}

// a successor nb of the popped node cur at cost g: skipped when closed, accepted when it has no record or a strictly larger g
FS_ASTAR_HD inline bool fs_astar_accepts(const fs_astar_mem &m, int32_t nb, double g)
{
    if (m.closed[nb]) return false;
    const int32_t b = m.best[nb];
    return b < 0 || m.rec_g[b] > g;
}

// the accepted successor's record (parent all[cur]) and its push.  false: no room (nothing changed).
FS_ASTAR_HD inline bool fs_astar_commit(const fs_astar_mem &m, int32_t cur, int32_t nb, double g, double f, int32_t &nrec, int32_t &hsize)
{
    if (nrec >= m.cap) return false;
    m.rec_node[nrec] = nb; m.rec_g[nrec] = g; m.rec_parent[nrec] = m.best[cur];
    m.best[nb] = nrec;
    fs_astar_push(m.heap_f, m.heap_rec, hsize, f, nrec);
    ++nrec;
    return true;
}

// the path's length from the record of the node that passed the goal test, summed from the goal end (astar.cpp:57-63)
FS_ASTAR_HD inline double fs_astar_length(const fs_astar_mem &m, const double *xy, int32_t r)
{
    double total = 0;
    for (int32_t p = m.rec_parent[r]; p >= 0; r = p, p = m.rec_parent[r]) total += sqrt(fs_astar_sq(xy, m.rec_node[r], m.rec_node[p]));
    return total;
}

// The whole search, one successor at a time (the host form; the device evaluates a popped node's successors across a wave and
// commits them in this order).  best[] = -1 and closed[] = 0 on entry.  FS_ASTAR_FOUND with *len, FS_ASTAR_NO_PATH, or
// FS_ASTAR_OVERFLOW when the records outgrow m.cap.  *pops: records popped.
FS_ASTAR_HD inline int fs_astar_run(const fs_astar_graph &G, const fs_astar_mem &m, int32_t start, int32_t goal, double *len, int32_t *pops)
{
    int32_t nrec = 0, hsize = 0;
    *pops = 0;
    fs_astar_begin(m, start, nrec, hsize);
    const double gx = G.xy[2 * goal], gy = G.xy[2 * goal + 1];
    while (hsize > 0) {
        const int32_t r = fs_astar_pop(m.heap_f, m.heap_rec, hsize);
        ++*pops;
        const int32_t cur = m.rec_node[r];
        if (G.xy[2 * cur] == gx && G.xy[2 * cur + 1] == gy) {
            *len = fs_astar_length(m, G.xy, m.best[cur]);
            return FS_ASTAR_FOUND;
        }
        m.closed[cur] = 1;
        const double cg = m.rec_g[r];
        for (int32_t j = G.row[cur]; j < G.row[cur + 1]; ++j) {
            const int32_t nb = G.col[j];
            const double g = cg + fs_astar_sq(G.xy, cur, nb), h = fs_astar_sq(G.xy, nb, goal);
            if (!fs_astar_accepts(m, nb, g)) continue;
            if (!fs_astar_commit(m, cur, nb, g, g + h, nrec, hsize)) return FS_ASTAR_OVERFLOW;
        }
    }
    return FS_ASTAR_NO_PATH;
}
