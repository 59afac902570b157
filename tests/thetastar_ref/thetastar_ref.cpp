// thetastar_ref.cpp — CPU restatement of the any-angle leg refinement (fs_refine_paths / fs_refine_field).  Test
// infrastructure: built by its tests with `g++ -O2 -ffp-contract=off -shared -fPIC` and loaded through ctypes.
//
// Two legs over the staged 2-D grid (raw costmap bytes):
//   field      DESIGN.md 4.12 exactly: the fp64 cost field from the start cell (Dijkstra; the fixed point does not depend on the
//              schedule), the descent from the goal in moves[] order, Theta*'s parent rule along the descended chain with the
//              integer line-of-sight sums, backtrace + linear interpolation.  The GPU is held to this leg bit for bit.
//   reference  the reference's Theta* search as it runs: a binary heap (std::priority_queue) over node pointers whose f keys are
//              mutated in place, re-pushes of closed nodes, resetParent at pop, the fp64 left-fold line-of-sight sums, std::hypot,
//              and the loop that leaves as soon as the queue is empty — a goal (or any node) popped as the last entry is never
//              examined.  `quirk` reports the legs where the same search that examines that last entry finds a path.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <functional>
#include <queue>
#include <utility>
#include <vector>

namespace {

constexpr double kInf = DBL_MAX;
constexpr int kMoves[8][2] = {{0, 1}, {0, -1}, {1, 0}, {-1, 0}, {1, -1}, {-1, 1}, {1, 1}, {-1, -1}};
enum { kOk = 0, kStartOff = 1, kGoalOff = 2, kStartUnsafe = 3, kGoalUnsafe = 4, kNoPath = 5 };

struct Grid {
    const uint8_t *c;
    int nx, ny;
    bool allow;
    double w_euc, w_trav;
    int corners;
    bool in(int x, int y) const { return x >= 0 && y >= 0 && x < nx && y < ny; }
    int raw(int x, int y) const { return c[(size_t)y * nx + x]; }
    // the two-argument isSafe: the raw byte below LETHAL, or unknown with allow_unknown
    bool safe(int x, int y) const { const int v = raw(x, y); return (v == 255 && allow) || v < 254; }
    // getTraversalCost: w * c * c / 254 / 254 with getCost's c = 26 + 0.9 * raw (unknown: 255.5)
    double trav(int x, int y) const { const double cc = 26 + 0.9 * raw(x, y); return w_trav * cc * cc / 254 / 254; }
};

// costmap worldToMap / mapToWorld
bool world_to_map(double ox, double oy, double res, int nx, int ny, double wx, double wy, int &mx, int &my)
{
    if (wx < ox || wy < oy) return false;
    const double qx = (wx - ox) / res, qy = (wy - oy) / res;
    if (!(qx < 4294967296.0) || !(qy < 4294967296.0)) return false;
    const unsigned ux = (unsigned)qx, uy = (unsigned)qy;
    if (ux >= (unsigned)nx || uy >= (unsigned)ny) return false;
    mx = (int)ux; my = (int)uy;
    return true;
}
double map_to_world(double o, double res, int m) { return o + ((unsigned)m + 0.5) * res; }

// ---------------------------------------------------------------- the field leg

// One cell of a line-of-sight walk (the three-argument isSafe): false if unsafe or off the map, else the cell's integer term
// (100 * scaled cost)^2 — (2600 + 90 raw)^2, an unknown cell (allowed) 25300^2.
bool los_cell(const Grid &g, int x, int y, int64_t &term)
{
    if (!g.in(x, y)) return false;
    const int v = g.raw(x, y);
    if (v == 255 && g.allow) { term = (int64_t)25300 * 25300; return true; }
    if (v >= 254) return false;
    const int64_t s = 2600 + 90 * (int64_t)v;
    term = s * s;
    return true;
}

// losCheck's Bresenham walk from (x0, y0) to (x1, y1): every iteration in order, its cells summed as integers
bool los_int(const Grid &g, int x0, int y0, int x1, int y1, int64_t &sum, int64_t &cells)
{
    sum = 0;
    const int dx = abs(x1 - x0), dy = abs(y1 - y0);
    const int sx = x1 > x0 ? 1 : -1, sy = y1 > y0 ? 1 : -1;
    const int ux = (sx - 1) / 2, uy = (sy - 1) / 2;
    const bool xmaj = dx >= dy;
    const int n = xmaj ? dx : dy, m = xmaj ? dy : dx;
    int cx = x0, cy = y0, f = 0;
    int64_t t = 0;
    for (int k = 0; k < n; ++k) {
        f += m;
        if (xmaj) {
            if (f >= dx) { if (!los_cell(g, cx + ux, cy + uy, t)) return false; sum += t; ++cells; cy += sy; f -= dx; }
            if (f != 0) { if (!los_cell(g, cx + ux, cy + uy, t)) return false; sum += t; ++cells; }
            if (dy == 0) {
                if (los_cell(g, cx + ux, cy, t)) sum += t;
                else if (los_cell(g, cx + ux, cy - 1, t)) sum += t;
                else return false;
                ++cells;
            }
            cx += sx;
        } else {
            if (f >= dy) { if (!los_cell(g, cx + ux, cy + uy, t)) return false; sum += t; ++cells; cx += sx; f -= dy; }
            if (f != 0) { if (!los_cell(g, cx + ux, cy + uy, t)) return false; sum += t; ++cells; }
            if (dx == 0) {
                if (los_cell(g, cx, cy + uy, t)) sum += t;
                else if (los_cell(g, cx - 1, cy + uy, t)) sum += t;
                else return false;
                ++cells;
            }
            cy += sy;
        }
    }
    return true;
}

double euc_int(const Grid &g, int ax, int ay, int bx, int by)
{
    const int64_t dx = ax - bx, dy = ay - by;
    return g.w_euc * sqrt((double)(dx * dx + dy * dy));
}

void field_dijkstra(const Grid &g, int sx, int sy, double *out)
{
    const size_t ns = (size_t)g.nx * g.ny;
    for (size_t k = 0; k < ns; ++k) out[k] = kInf;
    if (!g.safe(sx, sy)) return;
    double e[8];
    for (int i = 0; i < 8; ++i) e[i] = g.w_euc * sqrt((double)(kMoves[i][0] * kMoves[i][0] + kMoves[i][1] * kMoves[i][1]));
    typedef std::pair<double, int64_t> Item;
    std::priority_queue<Item, std::vector<Item>, std::greater<Item>> q;
    out[(size_t)sy * g.nx + sx] = g.trav(sx, sy);
    q.push(Item(out[(size_t)sy * g.nx + sx], (int64_t)sy * g.nx + sx));
    std::vector<uint8_t> done(ns, 0);
    while (!q.empty()) {
        const Item it = q.top();
        q.pop();
        if (done[it.second]) continue;
        done[it.second] = 1;
        const int ux = (int)(it.second % g.nx), uy = (int)(it.second / g.nx);
        for (int i = 0; i < g.corners; ++i) {
            const int vx = ux + kMoves[i][0], vy = uy + kMoves[i][1];
            if (!g.in(vx, vy) || !g.safe(vx, vy) || (vx == sx && vy == sy)) continue;
            const size_t v = (size_t)vy * g.nx + vx;
            const double cand = (it.first + e[i]) + g.trav(vx, vy);
            if (cand < out[v]) { out[v] = cand; q.push(Item(cand, (int64_t)v)); }
        }
    }
}

struct Leg {
    int status = kNoPath;
    double cost = kInf;
    std::vector<int> vx, vy;               // vertices, start first
    int64_t los_walks = 0;
    int64_t chain = 0;
};

void field_leg(const Grid &g, int sx, int sy, int gx, int gy, const double *F, Leg &L)
{
    const int nx = g.nx;
    if (F[(size_t)gy * nx + gx] >= kInf) { L.status = kNoPath; return; }
    double e[8];
    for (int i = 0; i < 8; ++i) e[i] = g.w_euc * sqrt((double)(kMoves[i][0] * kMoves[i][0] + kMoves[i][1] * kMoves[i][1]));
    // descent: goal first
    std::vector<int> d;
    int x = gx, y = gy;
    d.push_back(y * nx + x);
    while (!(x == sx && y == sy)) {
        const double gv = F[(size_t)y * nx + x], tv = g.trav(x, y);
        int pick = -1;
        for (int i = 0; i < g.corners && pick < 0; ++i) {
            const int ux = x + kMoves[i][0], uy = y + kMoves[i][1];
            if (!g.in(ux, uy)) continue;
            const double gu = F[(size_t)uy * nx + ux];
            if (gu >= kInf) continue;
            if ((gu + e[i]) + tv == gv) pick = i;
        }
        if (pick < 0 || d.size() > (size_t)nx * g.ny) { L.status = kNoPath; return; }   // (cannot happen on a fixed point)
        x += kMoves[pick][0]; y += kMoves[pick][1];
        d.push_back(y * nx + x);
    }
    const int P = (int)d.size() - 1;
    L.chain = P + 1;
    std::vector<int> par(P + 1, 0);
    // the chain c_0 = start ... c_P = goal; G(c_0) = trav(start), parent(c_0) = c_0
    double Gprev = g.trav(sx, sy), Gpp = Gprev;
    int pprev = 0;
    for (int i = 1; i <= P; ++i) {
        const int c = d[P - i], cp = d[P - i + 1];
        const int cx = c % nx, cy = c / nx, px = cp % nx, py = cp / nx;
        double G = (Gprev + euc_int(g, px, py, cx, cy)) + g.trav(cx, cy);
        int p = i - 1;
        double Gp = Gprev;
        const int a = d[P - pprev], ax = a % nx, ay = a / nx;
        int64_t sum = 0, cells = 0;
        ++L.los_walks;
        if (los_int(g, cx, cy, ax, ay, sum, cells)) {
            const double los = g.w_trav * (double)sum / 645160000.0;
            const double g2 = (Gpp + euc_int(g, cx, cy, ax, ay)) + los;
            if (g2 < G) { G = g2; p = pprev; Gp = Gpp; }
        }
        par[i] = p;
        Gprev = G; pprev = p; Gpp = Gp;
    }
    L.cost = Gprev;
    std::vector<int> rev;
    for (int i = P; i != 0; i = par[i]) rev.push_back(d[P - i]);
    rev.push_back(d[P]);
    for (size_t k = rev.size(); k-- > 0;) { L.vx.push_back(rev[k] % nx); L.vy.push_back(rev[k] / nx); }
    L.status = kOk;
}

// ---------------------------------------------------------------- the reference leg

struct Node {
    int x = 0, y = 0;
    double g = kInf, h = kInf;
    const Node *parent = nullptr;
    bool queued = false;
    double f = kInf;
};
struct ByF {
    bool operator()(const Node *a, const Node *b) const { return a->f > b->f; }
};

bool los_ref(const Grid &g, int x0, int y0, int x1, int y1, double &sum, int64_t &walks)
{
    ++walks;
    sum = 0;
    auto cell = [&](int x, int y) {
        if (!g.in(x, y)) return false;
        const int v = g.raw(x, y);
        double cc = 26 + 0.9 * v;
        if ((v == 255 && g.allow) || cc < 254) {
            if (v == 255) cc = 254 - 1;
            sum += g.w_trav * cc * cc / 254 / 254;
            return true;
        }
        return false;
    };
    const int dx = abs(x1 - x0), dy = abs(y1 - y0);
    const int sx = x1 > x0 ? 1 : -1, sy = y1 > y0 ? 1 : -1;
    const int ux = (sx - 1) / 2, uy = (sy - 1) / 2;
    int cx = x0, cy = y0, f = 0;
    if (dx >= dy) {
        for (; cx != x1; cx += sx) {
            f += dy;
            if (f >= dx) { if (!cell(cx + ux, cy + uy)) return false; cy += sy; f -= dx; }
            if (f != 0 && !cell(cx + ux, cy + uy)) return false;
            if (dy == 0 && !cell(cx + ux, cy) && !cell(cx + ux, cy - 1)) return false;
        }
    } else {
        for (; cy != y1; cy += sy) {
            f += dx;
            if (f >= dy) { if (!cell(cx + ux, cy + uy)) return false; cx += sx; f -= dy; }
            if (f != 0 && !cell(cx + ux, cy + uy)) return false;
            if (dx == 0 && !cell(cx, cy + uy) && !cell(cx - 1, cy + uy)) return false;
        }
    }
    return true;
}

// examine_last: 0 = the reference's loop; 1 = the same search, but the entry popped last is examined too
void reference_leg(const Grid &g, int sx, int sy, int gx, int gy, int examine_last, Leg &L)
{
    const int nx = g.nx;
    const double w_h = g.w_euc < 1.0 ? g.w_euc : 1.0;
    std::vector<Node> nodes((size_t)nx * g.ny);
    std::vector<Node *> at((size_t)nx * g.ny, nullptr);
    size_t used = 0;
    std::priority_queue<Node *, std::vector<Node *>, ByF> q;
    auto hcost = [&](int x, int y) { return w_h * std::hypot((double)(x - gx), (double)(y - gy)); };
    Node *s = &nodes[used++];
    s->x = sx; s->y = sy; s->g = g.trav(sx, sy); s->h = hcost(sx, sy); s->parent = s; s->queued = true; s->f = s->g + s->h;
    q.push(s);
    at[(size_t)sy * nx + sx] = s;
    Node *cur = s;
    bool found = false;
    for (;;) {
        if (!examine_last && q.empty()) break;      // generatePath's `while (!queue_.empty())`: the entry just popped is dropped
        if (cur->x == gx && cur->y == gy) { found = true; break; }
        // resetParent
        cur->queued = false;
        const Node *gp = cur->parent->parent;
        double los = 0;
        if (los_ref(g, cur->x, cur->y, gp->x, gp->y, los, L.los_walks)) {
            const double gc = gp->g + g.w_euc * std::hypot((double)(cur->x - gp->x), (double)(cur->y - gp->y)) + los;
            if (gc < cur->g) { cur->parent = gp; cur->g = gc; cur->f = gc + cur->h; }
        }
        // setNeighbors
        for (int i = 0; i < g.corners; ++i) {
            const int mx = cur->x + kMoves[i][0], my = cur->y + kMoves[i][1];
            if (!g.in(mx, my) || !g.safe(mx, my)) continue;
            const double gc = cur->g + g.w_euc * std::hypot((double)(cur->x - mx), (double)(cur->y - my)) + g.trav(mx, my);
            Node *&m = at[(size_t)my * nx + mx];
            if (!m) m = &nodes[used++];
            const double hc = hcost(mx, my), fc = gc + hc;
            if (m->f > fc) {
                m->g = gc; m->h = hc; m->f = fc; m->parent = cur;
                if (!m->queued) { m->x = mx; m->y = my; m->queued = true; q.push(m); }
            }
        }
        if (q.empty()) break;                 // (only reachable with examine_last: the reference's queue is never empty here)
        cur = q.top();
        q.pop();
    }
    if (!found) { L.status = kNoPath; return; }
    L.cost = cur->g;
    std::vector<const Node *> rev;
    for (const Node *n = cur; ; n = n->parent) { rev.push_back(n); if (n->parent == n) break; }
    for (size_t k = rev.size(); k-- > 0;) { L.vx.push_back(rev[k]->x); L.vy.push_back(rev[k]->y); }
    L.status = kOk;
}

// ThetaStar::backtrace (the goal twice) + linearInterpolation; use_hypot: the reference's std::hypot, else sqrt(dx^2 + dy^2)
void interpolate(const std::vector<double> &wx, const std::vector<double> &wy, double res, bool use_hypot, std::vector<double> &px,
                 std::vector<double> &py)
{
    std::vector<double> rx(wx), ry(wy);
    rx.push_back(wx.back()); ry.push_back(wy.back());
    for (size_t j = 0; j + 1 < rx.size(); ++j) {
        const double x1 = rx[j], y1 = ry[j], x2 = rx[j + 1], y2 = ry[j + 1];
        px.push_back(x1); py.push_back(y1);
        const double ex = x2 - x1, ey = y2 - y1;
        const double dist = use_hypot ? std::hypot(ex, ey) : sqrt(ex * ex + ey * ey);
        const int loops = (int)(dist / res);
        const double sa = ey / dist, ca = ex / dist;
        for (int k = 1; k < loops; ++k) {
            px.push_back(x1 + k * res * ca);
            py.push_back(y1 + k * res * sa);
        }
    }
}

}  // namespace

extern "C" {

// The field of DESIGN.md 4.12 from start cell (sx, sy): out [ny][nx], DBL_MAX where not reached (everywhere for an unsafe start).
int tr_field(const uint8_t *cells, int nx, int ny, int sx, int sy, int allow_unknown, double w_euc, double w_trav, int corners, double *out)
{
    const Grid g{cells, nx, ny, allow_unknown != 0, w_euc, w_trav, corners};
    if (!g.in(sx, sy)) return -1;
    field_dijkstra(g, sx, sy, out);
    return 0;
}

// One leg in world coordinates.  leg 0 field, 1 reference.  Outputs: status, cost, the vertex count and up to vcap vertices
// (vxy [vcap][2], world), the pose count and up to pcap poses (pxy [pcap][2]); stats: [0] LOS walks, [1] chain length,
// [2] quirk (reference leg: the search that examines its last entry finds a path, the reference's loop does not).
int tr_leg(const uint8_t *cells, int nx, int ny, double ox, double oy, double res, const double *start_xy, const double *goal_xy,
           int allow_unknown, double w_euc, double w_trav, int corners, int leg, int *status, double *cost, int *n_vertices,
           double *vxy, int vcap, int *n_poses, double *pxy, int pcap, int64_t *stats)
{
    const Grid g{cells, nx, ny, allow_unknown != 0, w_euc, w_trav, corners};
    int sx = 0, sy = 0, gx = 0, gy = 0;
    *cost = kInf; *n_vertices = 0; *n_poses = 0;
    stats[0] = stats[1] = stats[2] = 0;
    if (!world_to_map(ox, oy, res, nx, ny, start_xy[0], start_xy[1], sx, sy)) { *status = kStartOff; return 0; }
    if (!world_to_map(ox, oy, res, nx, ny, goal_xy[0], goal_xy[1], gx, gy)) { *status = kGoalOff; return 0; }
    if (!g.safe(sx, sy)) { *status = kStartUnsafe; return 0; }
    if (!g.safe(gx, gy)) { *status = kGoalUnsafe; return 0; }
    Leg L;
    if (leg == 0) {
        std::vector<double> F((size_t)nx * ny);
        field_dijkstra(g, sx, sy, F.data());
        field_leg(g, sx, sy, gx, gy, F.data(), L);
    } else {
        reference_leg(g, sx, sy, gx, gy, 0, L);
        if (L.status != kOk) {
            Leg M;
            reference_leg(g, sx, sy, gx, gy, 1, M);
            stats[2] = M.status == kOk;
        }
    }
    stats[0] = L.los_walks; stats[1] = L.chain;
    *status = L.status;
    if (L.status != kOk) return 0;
    *cost = L.cost;
    std::vector<double> wx, wy, px, py;
    for (size_t k = 0; k < L.vx.size(); ++k) { wx.push_back(map_to_world(ox, res, L.vx[k])); wy.push_back(map_to_world(oy, res, L.vy[k])); }
    interpolate(wx, wy, res, leg != 0, px, py);
    *n_vertices = (int)wx.size();
    *n_poses = (int)px.size();
    for (int k = 0; k < *n_vertices && k < vcap; ++k) { vxy[2 * k] = wx[k]; vxy[2 * k + 1] = wy[k]; }
    for (int k = 0; k < *n_poses && k < pcap; ++k) { pxy[2 * k] = px[k]; pxy[2 * k + 1] = py[k]; }
    return 0;
}

// the integer line-of-sight sum between two cells (1: line of sight, 0: blocked), for the known-answer tests
int tr_los(const uint8_t *cells, int nx, int ny, int allow_unknown, int x0, int y0, int x1, int y1, int64_t *sum, double *ref_sum)
{
    const Grid g{cells, nx, ny, allow_unknown != 0, 1.0, 1.0, 8};
    int64_t cells_n = 0, walks = 0;
    const bool a = los_int(g, x0, y0, x1, y1, *sum, cells_n);
    const bool b = los_ref(g, x0, y0, x1, y1, *ref_sum, walks);
    return (a ? 1 : 0) | (b ? 2 : 0);
}

}  // extern "C"
