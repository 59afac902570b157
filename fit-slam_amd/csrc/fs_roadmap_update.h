// fs_roadmap_update.h — the order-free rules of fs_roadmap_update: what UpdateRoadmapBT's sequential loops
// (populateNodes, constructNewEdges) decide, stated per item so that every item can be decided at once.  Shared by the device code
// (fs_roadmap_update.hip) and the CPU restatement test (tests/roadmap_update_ref/), like fs_roadmap_astar.h and fs_median_sort.h.
//
// Keep.     Point i of a list is kept iff no EXISTING node of the 3 x 3 hash cells around it is closer than min_d (decided alone)
//           and no EARLIER KEPT point of the list is (the unique solution of keep(i) = no conflict j < i is kept; Jacobi rounds
//           over it make only final decisions, fs_roadmap_kf.hip).  A point an existing node rejects enters the rounds as rejected.
// Cell cap. A kept point whose cell already holds FS_RU_MAX_PER_CELL nodes (existing ones plus the kept points before it) is still
//           added and ends the list: populateNodes throws after the push_back.
// Owners.   constructNewEdges works on each point's closest hash node p.  A second point with the same p changes nothing: every
//           pair (p, q) of p's list is linked by then (skipped), or failed its walk q -> p and fails it again on the unchanged
//           grid; the key flags are set already.  So only the FIRST occurrence of each closest node (the owner ranks) builds edges.
// Insert.   Candidate (p; q) — owner p, q within the radius — is inserted iff the pair was not linked either way before the call,
//           its walk q -> p is connectable, and NOT (q is an owner of earlier rank whose candidate (q; p), walked p -> q, was
//           connectable).  An unordered pair is met at most twice (once per owner end); the first connectable meeting inserts both
//           directions, which is what makes the second one skip.  An earlier FAILED meeting blocks nothing: the two walk directions
//           visit different cells.
#ifndef FS_ROADMAP_UPDATE_H
#define FS_ROADMAP_UPDATE_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define FS_RU_HD __host__ __device__ inline
#else
#define FS_RU_HD inline
#endif

#define FS_RU_MAX_PER_CELL 20           // populateNodes throws once a cell holds more (FrontierRoadmap.cpp:244-248)

enum { FS_RU_UNDECIDED = 0, FS_RU_KEPT = 1, FS_RU_REJECTED = 2 };

// FrontierRoadMap::getGridCell
FS_RU_HD int fs_ru_cell(double v, double cell) { return (int)floor(v / cell); }

// populateNodes' test of a new point (x, y) against a node (qx, qy): the node sits in the 3 x 3 cells around the point's cell and
// is closer than min_d — fs_roadmap_add_nodes' double expression
FS_RU_HD bool fs_ru_conflict(double x, double y, double qx, double qy, double cell, double min_d)
{
    const int64_t ax = (int64_t)fs_ru_cell(qx, cell) - fs_ru_cell(x, cell), ay = (int64_t)fs_ru_cell(qy, cell) - fs_ru_cell(y, cell);
    if (ax < -1 || ax > 1 || ay < -1 || ay > 1) return false;
    const double ex = x - qx, ey = y - qy;
    return sqrt(ex * ex + ey * ey) < min_d;
}

FS_RU_HD bool fs_ru_same_cell(double x, double y, double qx, double qy, double cell)
{
    return fs_ru_cell(x, cell) == fs_ru_cell(qx, cell) && fs_ru_cell(y, cell) == fs_ru_cell(qy, cell);
}

// One Jacobi step for an undecided point: conf = its conflict row (bit j: earlier point j conflicts), kept / rejected = the
// decisions of the round before, `words` 64-bit words each.  Kept once every conflict is rejected, rejected once one is kept.
FS_RU_HD int fs_ru_keep_step(const uint64_t *conf, const uint64_t *kept, const uint64_t *rejected, int32_t words)
{
    bool all_rejected = true;
    for (int32_t w = 0; w < words; ++w) {
        const uint64_t c = conf[w];
        if (c & kept[w]) return FS_RU_REJECTED;
        all_rejected = all_rejected && (c & ~rejected[w]) == 0;
    }
    return all_rejected ? FS_RU_KEPT : FS_RU_UNDECIDED;
}

// the kept point that finds `before` nodes in its cell is the one populateNodes throws on
FS_RU_HD bool fs_ru_trips(int32_t before) { return before >= FS_RU_MAX_PER_CELL; }

// getNodesWithinRadius(p) holds q: q's cell within +-cr cells of p's, cr = ceil(radius / cell), and strictly closer than the radius.
// *order = the cell's place in the scan (dx outer, dy inner); inside a cell the nodes follow in insertion (= index) order.
FS_RU_HD bool fs_ru_within(double px, double py, double qx, double qy, double cell, double radius, int32_t *order)
{
    const int64_t cr = (int64_t)ceil(radius / cell);
    const int64_t dx = (int64_t)fs_ru_cell(qx, cell) - fs_ru_cell(px, cell), dy = (int64_t)fs_ru_cell(qy, cell) - fs_ru_cell(py, cell);
    if (dx < -cr || dx > cr || dy < -cr || dy > cr) return false;
    const double ex = px - qx, ey = py - qy;
    if (!(sqrt(ex * ex + ey * ey) < radius)) return false;
    *order = (int32_t)((dx + cr) * (2 * cr + 1) + (dy + cr));
    return true;
}

// getClosestNodeInHashmap grows a square of (int)(cell * m) hash cells, m = 1, 2, ..., until one holds a node: the square it stops
// at, from the Chebyshev cell distance cmin of the nearest node (the same steps as fs_rm_closest, fs_internal.h)
FS_RU_HD int64_t fs_ru_search_radius(int64_t cmin, double cell)
{
    int64_t m = (int64_t)floor((double)cmin / cell);
    if (m < 1) m = 1;
    while (m > 1 && (int64_t)(cell * (double)(m - 1)) >= cmin) --m;
    while ((int64_t)(cell * (double)m) < cmin) ++m;
    return (int64_t)(cell * (double)m);
}

// getClosestNodeInHashmap's order between two nodes of the search square (fs_rm_closest): distance, then (dx, dy, index)
FS_RU_HD bool fs_ru_closer(double d, int64_t ax, int64_t ay, int32_t k, double bd, int64_t bx, int64_t by, int32_t bk)
{
    if (k < 0) return false;
    if (bk < 0) return true;
    if (d != bd) return d < bd;
    if (ax != bx) return ax < bx;
    if (ay != by) return ay < by;
    return k < bk;
}

// point i is the first of the list whose closest node is closest[i]
FS_RU_HD bool fs_ru_is_owner(const int32_t *closest, int32_t i)
{
    for (int32_t j = 0; j < i; ++j)
        if (closest[j] == closest[i]) return false;
    return true;
}

// isConnectable's verdict from a segment walk's outputs
FS_RU_HD bool fs_ru_connectable(uint8_t on_map, uint8_t hit, int32_t unknown, double unknown_limit)
{
    return on_map && !hit && !((double)unknown > unknown_limit);
}

// Candidate (p; q) of the owner of rank p_rank.  linked_before: q in adj[p] or p in adj[q] before the call; conn_qp: its own walk
// q -> p; q_rank: q's owner rank or -1; conn_pq: the walk p -> q of q's candidate (q; p), read only when q_rank is earlier.
FS_RU_HD bool fs_ru_inserted(bool linked_before, bool conn_qp, int32_t p_rank, int32_t q_rank, bool conn_pq)
{
    if (linked_before || !conn_qp) return false;
    return !(q_rank >= 0 && q_rank < p_rank && conn_pq);
}

#endif
