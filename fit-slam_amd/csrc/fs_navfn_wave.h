// fs_navfn_wave.h — the grid planner's per-frontier wave (NavFn::calcNavFnAstar, DEP/src/planners/planner.cpp) as the reference
// runs it, for the REFERENCE grid search (fs_set_grid_search).  The device (fs_navfn.hip) and a host test driver
// (tests/navfn_wave_ref) compile this same source, as they do fs_roadmap_astar.h.
//
// The planner runs backwards: the wave starts at the ROBOT cell (the reference's goal) and stops the moment it reaches the FRONTIER
// cell (the reference's start, planner.cpp:875).  What makes its field order-dependent, and so part of the definition:
//   - three priority buffers (cur, next, over) of `cap` cells (the reference's 10 000); a push takes five conditions in this order:
//     the cell is inside the array, not pending, not an obstacle, and the buffer has room — a push dropped at the cap does NOT set
//     pending;
//   - a cycle clears pending over cur, updates the cells of cur in buffer order, swaps cur and next and, when next was empty, raises
//     the threshold curT by 2 * COST_NEUTRAL and swaps in over;
//   - an update that lowers a cell stores it, adds the heuristic (the distance to the frontier cell, in cells, * COST_NEUTRAL) and
//     pushes the neighbours l, r, u, d whose potential exceeds the new value by more than 0.707106781 of their cost, into next when
//     value + heuristic < curT and into over otherwise;
//   - the budget is max(nx * ny / 20, nx + ny) cycles.
//
// An entry of cur is handled in two steps.  fs_nw_evaluate reads memory (five potentials, five costs, four pending bytes) and decides
// everything that depends on the entry alone.  The commit decides, in entry order, what depends on the entries before it: the
// appends with the cap (fs_nw_commit_entry) and the dedupe against pushes of earlier entries of the same chunk (fs_nw_react, which
// also flags an entry whose evaluation an earlier entry's store has made stale); fs_nw_commit_write then stores.  A chunk of width 1
// is the serial wave, statement for statement; the device walks chunks of 64, one entry per lane, and commits the prefix up to the
// first stale entry.  Cells are unique inside cur (pending), every cell of cur is free and so off the border ring: its four
// neighbours are inside the array, and a difference of +-1 between two cells of cur means the same row.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FS_NW_HD __host__ __device__
#else
#define FS_NW_HD
#endif

#define FS_NW_POT_HIGH 1.0e10f
#define FS_NW_COST_OBS 254
#define FS_NW_COST_NEUTRAL 50
#define FS_NW_CAP 10000          // PRIORITYBUFSIZE
#define FS_NW_WIDTH 64           // entries of a chunk on the device: one per lane
#define FS_NW_MAX_SIDE 4096      // the heuristic's float has been compared with libm's hypot below this side

enum { FS_NW_LIMIT_CYCLES = 1, FS_NW_LIMIT_CAP = 2 };
// fs_nw_eval::bits
enum : uint32_t { FS_NW_STORE = 1u, FS_NW_OVER = 2u, FS_NW_DEP = 4u, FS_NW_CAND = 0x10u /* << l r u d */, FS_NW_CANDS = 0xf0u,
                  FS_NW_APP = 0x100u /* << l r u d */, FS_NW_APPS = 0xf00u };

struct fs_nw_map {
    const uint8_t *cost;       // [ny][nx] the planner's costs, border ring applied
    int32_t nx, ny;
};

struct fs_nw_wave {
    float *pot;                // [ny][nx]
    uint8_t *pending;          // [ny][nx]
    int32_t *cur, *next, *over;        // [cap] each
    int32_t cur_n, next_n, over_n;
    float curT;
    int32_t cap;
    int32_t limit;             // FS_NW_LIMIT_*
    int32_t sx, sy;            // the frontier cell (the reference's start): where the wave stops
    uint64_t *hash;            // host tests: a running hash of every push (buffer, position, cell); may be null
};

struct fs_nw_eval {
    int32_t cell;
    float p;                   // the cell's new potential (FS_NW_STORE)
    uint32_t bits;
    int32_t pos[4];            // where the appended candidates go (FS_NW_APP << d)
};

// updateCell's value from the four neighbours (double literals of the quadratic evaluated in double)
FS_NW_HD inline float fs_nw_cell_update(float l, float r, float u, float d, float hf)
{
    float tc = (l < r) ? l : r;
    float ta = (u < d) ? u : d;
    float dc = tc - ta;
    if (dc < 0) { dc = -dc; ta = tc; }
    if (dc >= hf) return ta + hf;
    const float q = dc / hf;
    const float v = (float)(-0.2301 * (double)q * (double)q + 0.5307 * (double)q + 0.7040);
    return ta + hf * v;
}

// (float)(hypot(dx, dy) * COST_NEUTRAL): the integer sum is exact, the square root is IEEE; the float equals libm's for every
// |dx|, |dy| < FS_NW_MAX_SIDE (the doubles differ in the last bit for some pairs, the floats for none)
FS_NW_HD inline float fs_nw_heuristic(int32_t dx, int32_t dy)
{
    return (float)(sqrt((double)(dx * dx + dy * dy)) * (double)(float)FS_NW_COST_NEUTRAL);
}

FS_NW_HD inline int32_t fs_nw_offset(int d, int32_t nx) { return d == 0 ? -1 : d == 1 ? 1 : d == 2 ? -nx : nx; }

FS_NW_HD inline void fs_nw_hash_push(fs_nw_wave &w, int role, int32_t pos, int32_t cell)
{
#if !defined(__HIP_DEVICE_COMPILE__)
    if (w.hash) *w.hash = (*w.hash ^ (((uint64_t)role << 56) ^ ((uint64_t)(uint32_t)pos << 28) ^ (uint64_t)(uint32_t)cell)) * 0x100000001b3ull;
#endif
}

// push_cur of the set-up
FS_NW_HD inline void fs_nw_push_cur(const fs_nw_map &m, fs_nw_wave &w, int32_t n)
{
    if (n >= 0 && n < m.nx * m.ny && !w.pending[n] && m.cost[n] < FS_NW_COST_OBS) {
        if (w.cur_n < w.cap) { fs_nw_hash_push(w, 0, w.cur_n, n); w.cur[w.cur_n++] = n; w.pending[n] = 1; }
        else w.limit |= FS_NW_LIMIT_CAP;
    }
}

// setupNavFn's start of the wave on a field of POT_HIGH with nothing pending: the robot cell at 0, its four neighbours pushed,
// curT = heuristic(robot) + COST_OBS.  Returns the cycle budget.
FS_NW_HD inline int32_t fs_nw_begin(const fs_nw_map &m, fs_nw_wave &w, int32_t rx, int32_t ry)
{
    const int32_t k = rx + ry * m.nx;
    w.cur_n = w.next_n = w.over_n = 0;
    w.limit = 0;
    w.pot[k] = 0.0f;
    fs_nw_push_cur(m, w, k + 1); fs_nw_push_cur(m, w, k - 1); fs_nw_push_cur(m, w, k - m.nx); fs_nw_push_cur(m, w, k + m.nx);
    w.curT = fs_nw_heuristic(rx - w.sx, ry - w.sy) + (float)FS_NW_COST_OBS;
    const int32_t a = m.nx * m.ny / 20, b = m.nx + m.ny;
    return a > b ? a : b;
}

// Everything an entry decides from memory alone: the new value, the target buffer, the neighbours it wants pushed (the static push
// conditions and the pending byte as memory holds it now folded in).
FS_NW_HD inline fs_nw_eval fs_nw_evaluate(const fs_nw_map &m, const fs_nw_wave &w, int32_t n)
{
    fs_nw_eval e;
    e.cell = n; e.p = 0.0f; e.bits = 0u;
    e.pos[0] = e.pos[1] = e.pos[2] = e.pos[3] = 0;
    const int32_t nx = m.nx;
    const float own = w.pot[n], l = w.pot[n - 1], r = w.pot[n + 1], u = w.pot[n - nx], d = w.pot[n + nx];
    const int c = m.cost[n], cl = m.cost[n - 1], cr = m.cost[n + 1], cu = m.cost[n - nx], cd = m.cost[n + nx];
    const uint8_t pl = w.pending[n - 1], pr = w.pending[n + 1], pu = w.pending[n - nx], pd = w.pending[n + nx];
    if (c >= FS_NW_COST_OBS) return e;
    float p = fs_nw_cell_update(l, r, u, d, (float)c);
    if (!(p < own)) return e;
    const float le = (float)(0.707106781 * (double)(float)cl), re = (float)(0.707106781 * (double)(float)cr);
    const float ue = (float)(0.707106781 * (double)(float)cu), de = (float)(0.707106781 * (double)(float)cd);
    const float dist = fs_nw_heuristic(n % nx - w.sx, n / nx - w.sy);
    e.p = p;
    e.bits = FS_NW_STORE;
    p += dist;
    if (!(p < w.curT)) e.bits |= FS_NW_OVER;
    if (l > p + le && !pl && cl < FS_NW_COST_OBS) e.bits |= FS_NW_CAND << 0;
    if (r > p + re && !pr && cr < FS_NW_COST_OBS) e.bits |= FS_NW_CAND << 1;
    if (u > p + ue && !pu && cu < FS_NW_COST_OBS) e.bits |= FS_NW_CAND << 2;
    if (d > p + de && !pd && cd < FS_NW_COST_OBS) e.bits |= FS_NW_CAND << 3;
    return e;
}

// The commit of one entry, in entry order, on the fill counts (uniform over a chunk): every live candidate is appended while its
// buffer has room.  Returns the entry's bits with FS_NW_APP set for what was appended; pos[d] is where.  Written without branches:
// on the device this runs once per entry in scalar code, where a taken branch costs more than the arithmetic it skips.
FS_NW_HD inline uint32_t fs_nw_commit_entry(int32_t &next_n, int32_t &over_n, int32_t &limit, int32_t cap, uint32_t bits, int32_t pos[4])
{
    const bool over = (bits & FS_NW_OVER) != 0u;
    int32_t pe = over ? over_n : next_n;
    uint32_t dropped = 0u;
    for (int d = 0; d < 4; ++d) {
        const uint32_t want = (bits >> (4 + d)) & 1u;
        const uint32_t ok = want & (pe < cap ? 1u : 0u);
        pos[d] = pe;
        pe += (int32_t)ok;
        bits |= ok << (8 + d);
        dropped |= want ^ ok;
    }
    over_n = over ? pe : over_n;
    next_n = over ? next_n : pe;
    limit |= (int32_t)(dropped * (uint32_t)FS_NW_LIMIT_CAP);
    return bits;
}

// A later entry of the chunk meets the commit of entry j (cell_j, bits_j after fs_nw_commit_entry): a neighbour j appended is
// pending now, and a store into a 4-neighbour makes this entry's evaluation stale.  j's target dj is this entry's target d when
// cell - cell_j = offset(dj) - offset(d): the twelve pairs, by the eight differences they give (cells of cur are off the border
// ring, so a difference names one displacement).
FS_NW_HD inline uint32_t fs_nw_react(uint32_t bits, int32_t cell, int32_t nx, int32_t cell_j, uint32_t bits_j)
{
    const int32_t dlt = cell - cell_j;
    const uint32_t al = (bits_j >> 8) & 1u, ar = (bits_j >> 9) & 1u, au = (bits_j >> 10) & 1u, ad = (bits_j >> 11) & 1u;
    const uint32_t L = FS_NW_CAND, R = FS_NW_CAND << 1, U = FS_NW_CAND << 2, D = FS_NW_CAND << 3;
    uint32_t clear = 0u;
    clear |= (dlt == -2) ? al * R : 0u;
    clear |= (dlt == 2) ? ar * L : 0u;
    clear |= (dlt == -2 * nx) ? au * D : 0u;
    clear |= (dlt == 2 * nx) ? ad * U : 0u;
    clear |= (dlt == nx - 1) ? (al * U | ad * R) : 0u;
    clear |= (dlt == -nx - 1) ? (al * D | au * R) : 0u;
    clear |= (dlt == nx + 1) ? (ar * U | ad * L) : 0u;
    clear |= (dlt == 1 - nx) ? (ar * D | au * L) : 0u;
    const bool near = dlt == 1 || dlt == -1 || dlt == nx || dlt == -nx;
    return (bits & ~clear) | ((near && (bits_j & FS_NW_STORE)) ? (uint32_t)FS_NW_DEP : 0u);
}

// The stores of a committed entry: its potential, its appended neighbours and their pending bytes.
FS_NW_HD inline void fs_nw_commit_write(fs_nw_wave &w, int32_t nx, const fs_nw_eval &e)
{
    if (e.bits & FS_NW_STORE) w.pot[e.cell] = e.p;
    int32_t *q = (e.bits & FS_NW_OVER) ? w.over : w.next;
    for (int d = 0; d < 4; ++d)
        if (e.bits & (FS_NW_APP << d)) {
            const int32_t t = e.cell + fs_nw_offset(d, nx);
            fs_nw_hash_push(w, (e.bits & FS_NW_OVER) ? 2 : 1, e.pos[d], t);
            q[e.pos[d]] = t;
            w.pending[t] = 1;
        }
}

// The end of a cycle: cur <- next; when that is empty, the threshold rises and over comes in.
FS_NW_HD inline void fs_nw_end_cycle(fs_nw_wave &w)
{
    int32_t *t = w.cur;
    w.cur_n = w.next_n; w.next_n = 0;
    w.cur = w.next; w.next = t;
    if (w.cur_n == 0) {
        w.curT += (float)(2 * FS_NW_COST_NEUTRAL);
        w.cur_n = w.over_n; w.over_n = 0;
        t = w.cur; w.cur = w.over; w.over = t;
    }
}

// The whole wave on one core, cur walked in chunks of `width` entries (1: the serial wave; FS_NW_WIDTH: the device's order of
// work).  Returns whether the wave reached the frontier cell; *replays counts the chunks cut short at a stale entry.
inline bool fs_nw_run(const fs_nw_map &m, fs_nw_wave &w, int32_t rx, int32_t ry, int32_t width, int64_t *replays)
{
    const int32_t cycles = fs_nw_begin(m, w, rx, ry), start = w.sy * m.nx + w.sx;
    int32_t cycle = 0;
    for (; cycle < cycles; ++cycle) {
        if (w.cur_n == 0 && w.next_n == 0) break;
        for (int32_t i = 0; i < w.cur_n; ++i) w.pending[w.cur[i]] = 0;
        for (int32_t base = 0; base < w.cur_n;) {
            const int32_t cnt = (w.cur_n - base < width) ? w.cur_n - base : width;
            fs_nw_eval e[FS_NW_WIDTH];
            for (int32_t k = 0; k < cnt; ++k) e[k] = fs_nw_evaluate(m, w, w.cur[base + k]);
            int32_t done = cnt;
            for (int32_t j = 0; j < cnt; ++j) {
                if (e[j].bits & FS_NW_DEP) { done = j; break; }
                e[j].bits = fs_nw_commit_entry(w.next_n, w.over_n, w.limit, w.cap, e[j].bits, e[j].pos);
                for (int32_t k = j + 1; k < cnt; ++k) e[k].bits = fs_nw_react(e[k].bits, e[k].cell, m.nx, e[j].cell, e[j].bits);
            }
            for (int32_t k = 0; k < done; ++k) fs_nw_commit_write(w, m.nx, e[k]);
            if (done < cnt && replays) ++*replays;
            base += done;
        }
        fs_nw_end_cycle(w);
        if (w.pot[start] < FS_NW_POT_HIGH) break;
    }
    if (cycle >= cycles) w.limit |= FS_NW_LIMIT_CYCLES;
    return w.pot[start] < FS_NW_POT_HIGH;
}
