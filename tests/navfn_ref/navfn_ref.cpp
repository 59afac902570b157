// navfn_ref.cpp — CPU restatement of the batched grid planner (fs_plan_paths / fs_navfn_potential).  Test
// infrastructure: built by its tests with `g++ -O2 -ffp-contract=off -shared -fPIC` and loaded through ctypes.
//
// Two legs over the same cost array (NavFn::setCostmap(isROS = true) + the border ring of setupNavFn):
//   converged        the tiled Jacobi schedule of DESIGN.md 4.9 step by step (same tiles, same sweeps, same rounds), then
//                    calcPath from every goal on that one field, then the columns.  The GPU is held to this leg bit for bit.
//   reference_astar  what the per-frontier planner computes: a new field per frontier, the bucketed best-first wave from the
//                    robot (three priority buffers, curT / priInc thresholds, conditional pushes, the 10 000-entry cap, stop
//                    at the goal cell, max(nx*ny/20, nx+ny) cycles), then calcPath.  Reports whether a limit was hit.
//
// Both legs share the path descent and the columns.  Every literal type is spelled out: the quadratic of the cell update is
// evaluated in double, calcPath's interpolation promotes (1.0 - dx) to double, hypot is (float)sqrt(double x^2 + double y^2).
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <limits>
#include <vector>

namespace {

constexpr int kTile = 32;                 // NAVFN_TILE of fs_navfn.hip
constexpr float kPotHigh = 1.0e10f;
constexpr int kObs = 254, kNeutral = 50;
constexpr int kBufCap = 10000;
constexpr float kPathStep = 0.5f;

enum : uint32_t { kChanged = 1u, kEdgeX0 = 2u, kEdgeX1 = 4u, kEdgeY0 = 8u, kEdgeY1 = 16u, kForce = 32u };

struct Map {
    int nx, ny;
    std::vector<uint8_t> cost;            // planner cost, border ring applied
};

void build_costs(const uint8_t *cells, int nx, int ny, int allow_unknown, Map &m)
{
    m.nx = nx; m.ny = ny;
    m.cost.assign((size_t)nx * ny, (uint8_t)kObs);
    for (int y = 0; y < ny; ++y)
        for (int x = 0; x < nx; ++x) {
            const size_t k = (size_t)y * nx + x;
            const int v = cells[k];
            int c = kObs;
            if (v < 253) {
                c = (int)(50 + 0.8 * v);                  // COST_NEUTRAL + COST_FACTOR * v, double, truncated
                if (c >= kObs) c = kObs - 1;
            } else if (v == 255 && allow_unknown) {
                c = kObs - 1;
            }
            if (x == 0 || y == 0 || x == nx - 1 || y == ny - 1) c = kObs;
            m.cost[k] = (uint8_t)c;
        }
}

float hyp(float x, float y) { return (float)sqrt((double)x * x + (double)y * y); }

// the planar-wave update of a free cell from its four neighbours (returns the candidate, not yet compared with the cell)
float cell_update(float l, float r, float u, float d, int cost)
{
    float tc = (l < r) ? l : r;
    float ta = (u < d) ? u : d;
    const float hf = (float)cost;
    float dc = tc - ta;
    if (dc < 0) { dc = -dc; ta = tc; }
    if (dc >= hf) return ta + hf;
    const float q = dc / hf;
    const float v = (float)(-0.2301 * (double)q * (double)q + 0.5307 * (double)q + 0.7040);
    return ta + hf * v;
}

// ------------------------------------------------------------------ the converged leg: tiled Jacobi rounds
struct Stats { int64_t rounds = 0, tile_runs = 0, sweeps = 0, max_sweeps = 0; };

void converged_field(const Map &m, int rx, int ry, std::vector<float> &out, Stats &st)
{
    const int nx = m.nx, ny = m.ny, tx = (nx + kTile - 1) / kTile, ty = (ny + kTile - 1) / kTile;
    const size_t ns = (size_t)nx * ny;
    std::vector<float> a(ns, kPotHigh);
    a[(size_t)ry * nx + rx] = 0.0f;
    std::vector<float> b = a;
    std::vector<uint32_t> prev((size_t)tx * ty, 0u), cur((size_t)tx * ty, 0u);
    prev[(size_t)(ry / kTile) * tx + rx / kTile] = kForce;
    const int W = kTile + 2;
    std::vector<float> s0((size_t)W * W), s1((size_t)W * W);
    for (;;) {
        bool any = false;
        for (int j = 0; j < ty; ++j)
            for (int i = 0; i < tx; ++i) {
                const size_t t = (size_t)j * tx + i;
                const bool active = (prev[t] & kForce) || (i > 0 && (prev[t - 1] & kEdgeX1)) || (i + 1 < tx && (prev[t + 1] & kEdgeX0)) ||
                                    (j > 0 && (prev[t - tx] & kEdgeY1)) || (j + 1 < ty && (prev[t + tx] & kEdgeY0));
                const int x0 = i * kTile, y0 = j * kTile, x1 = std::min(x0 + kTile, nx), y1 = std::min(y0 + kTile, ny);
                cur[t] = 0;
                if (!active) {
                    if (prev[t] & kChanged)
                        for (int y = y0; y < y1; ++y) for (int x = x0; x < x1; ++x) b[(size_t)y * nx + x] = a[(size_t)y * nx + x];
                    continue;
                }
                ++st.tile_runs;
                // interior + 1-cell halo from the snapshot; outside the map: POT_HIGH
                for (int ly = 0; ly < W; ++ly)
                    for (int lx = 0; lx < W; ++lx) {
                        const int x = x0 - 1 + lx, y = y0 - 1 + ly;
                        s0[(size_t)ly * W + lx] = (x >= 0 && y >= 0 && x < nx && y < ny) ? a[(size_t)y * nx + x] : kPotHigh;
                    }
                s1 = s0;
                int sweeps = 0;
                for (;;) {
                    bool ch = false;
                    for (int y = y0; y < y1; ++y)
                        for (int x = x0; x < x1; ++x) {
                            const int c = m.cost[(size_t)y * nx + x];
                            const size_t l = (size_t)(y - y0 + 1) * W + (x - x0 + 1);
                            float p = s0[l];
                            if (c < kObs) {
                                const float pot = cell_update(s0[l - 1], s0[l + 1], s0[l - W], s0[l + W], c);
                                if (pot < p) { p = pot; ch = true; }
                            }
                            s1[l] = p;
                        }
                    ++sweeps;
                    std::swap(s0, s1);
                    if (!ch) break;
                }
                st.sweeps += sweeps;
                st.max_sweeps = std::max<int64_t>(st.max_sweeps, sweeps);
                uint32_t bits = 0;
                for (int y = y0; y < y1; ++y)
                    for (int x = x0; x < x1; ++x) {
                        const size_t g = (size_t)y * nx + x;
                        const float p = s0[(size_t)(y - y0 + 1) * W + (x - x0 + 1)];
                        if (p != a[g]) {
                            bits |= kChanged;
                            if (x == x0) bits |= kEdgeX0;
                            if (x == x1 - 1) bits |= kEdgeX1;
                            if (y == y0) bits |= kEdgeY0;
                            if (y == y1 - 1) bits |= kEdgeY1;
                        }
                        b[g] = p;
                    }
                cur[t] = bits;
                if (bits) any = true;
            }
        ++st.rounds;
        std::swap(a, b);
        std::swap(prev, cur);
        if (!any) break;
    }
    out.swap(a);
}

// ------------------------------------------------------------------ the reference_astar leg: one best-first wave per frontier
struct AstarWave {
    const Map &m;
    int nx, ns;
    std::vector<float> pot;
    std::vector<uint8_t> pending;
    std::vector<int> buf[3];
    int *curP, *nextP, *overP;
    int curPe = 0, nextPe = 0, overPe = 0;
    float curT = (float)kObs;
    int start[2], goal[2];                // start = the frontier cell, goal = the robot cell (the planner runs backwards)
    bool cap_hit = false;

    explicit AstarWave(const Map &mm) : m(mm), nx(mm.nx), ns(mm.nx * mm.ny), pot((size_t)ns, kPotHigh), pending((size_t)ns, 0)
    {
        for (auto &v : buf) v.assign(kBufCap, 0);
        curP = buf[0].data(); nextP = buf[1].data(); overP = buf[2].data();
    }
    void push(int *p, int &pe, int n)
    {
        if (n >= 0 && n < ns && !pending[n] && m.cost[n] < kObs) {
            if (pe < kBufCap) { p[pe++] = n; pending[n] = 1; }
            else cap_hit = true;
        }
    }
    void update(int n)
    {
        const float l = pot[n - 1], r = pot[n + 1], u = pot[n - nx], d = pot[n + nx];
        const int c = m.cost[n];
        if (c >= kObs) return;
        float p = cell_update(l, r, u, d, c);
        if (!(p < pot[n])) return;
        const float le = (float)(0.707106781 * (double)(float)m.cost[n - 1]);
        const float re = (float)(0.707106781 * (double)(float)m.cost[n + 1]);
        const float ue = (float)(0.707106781 * (double)(float)m.cost[n - nx]);
        const float de = (float)(0.707106781 * (double)(float)m.cost[n + nx]);
        const int x = n % nx, y = n / nx;
        const float dist = (float)(hypot((double)(x - start[0]), (double)(y - start[1])) * (double)(float)kNeutral);   // libm, as the planner
        pot[n] = p;
        p += dist;
        int *q = (p < curT) ? nextP : overP;
        int &qe = (p < curT) ? nextPe : overPe;
        if (l > p + le) push(q, qe, n - 1);
        if (r > p + re) push(q, qe, n + 1);
        if (u > p + ue) push(q, qe, n - nx);
        if (d > p + de) push(q, qe, n + nx);
    }
    // returns true when the wave reached the frontier cell; *cycles_hit: the cycle budget ran out first
    bool run(bool *cycles_hit)
    {
        const int k = goal[0] + goal[1] * nx;
        pot[k] = 0.0f;
        push(curP, curPe, k + 1); push(curP, curPe, k - 1); push(curP, curPe, k - nx); push(curP, curPe, k + nx);
        const int ny = ns / nx, cycles = std::max(nx * ny / 20, nx + ny);
        const float dist = (float)(hypot((double)(goal[0] - start[0]), (double)(goal[1] - start[1])) * (double)(float)kNeutral);
        curT = dist + curT;
        const int startCell = start[1] * nx + start[0];
        int cycle = 0;
        for (; cycle < cycles; ++cycle) {
            if (curPe == 0 && nextPe == 0) break;
            for (int i = 0; i < curPe; ++i) pending[curP[i]] = 0;
            for (int i = 0; i < curPe; ++i) update(curP[i]);
            curPe = nextPe; nextPe = 0;
            std::swap(curP, nextP);
            if (curPe == 0) {
                curT += (float)(2 * kNeutral);
                curPe = overPe; overPe = 0;
                std::swap(curP, overP);
            }
            if (pot[startCell] < kPotHigh) break;
        }
        *cycles_hit = cycle >= cycles;
        return pot[startCell] < kPotHigh;
    }
};

// ------------------------------------------------------------------ calcPath + columns (both legs)
// (int)f the way x86-64 converts: a value outside the int range (POT_HIGH) becomes INT_MIN
int to_int_x86(float f) { return (f >= 2147483648.0f || f < -2147483648.0f || f != f) ? INT32_MIN : (int)f; }

struct Descent {
    const float *P;
    int nx, ns;
    float pot(long i) const { return (i >= 0 && i < ns) ? P[i] : kPotHigh; }
    void grad(int n, float &gx, float &gy) const
    {
        gx = 0.0f; gy = 0.0f;
        if (n < nx || n > ns - nx) return;
        const float cv = pot(n);
        float dx = 0.0f, dy = 0.0f;
        if (cv >= kPotHigh) {
            if (pot(n - 1) < kPotHigh) dx = -(float)kObs;
            else if (pot(n + 1) < kPotHigh) dx = (float)kObs;
            if (pot(n - nx) < kPotHigh) dy = -(float)kObs;
            else if (pot(n + nx) < kPotHigh) dy = (float)kObs;
        } else {
            if (pot(n - 1) < kPotHigh) dx += pot(n - 1) - cv;
            if (pot(n + 1) < kPotHigh) dx += cv - pot(n + 1);
            if (pot(n - nx) < kPotHigh) dy += pot(n - nx) - cv;
            if (pot(n + nx) < kPotHigh) dy += cv - pot(n + nx);
        }
        float norm = hyp(dx, dy);
        if (norm > 0) {
            norm = (float)(1.0 / (double)norm);
            gx = norm * dx;
            gy = norm * dy;
        }
    }
    // NavFn::calcPath from cell (sx, sy) down to the robot cell (gx0, gy0); the points go to px / py; returns their number, or
    // why it failed: -1 out of bounds, -2 high potential, -3 zero gradient, -4 out of cycles
    int path(int sx, int sy, int gx0, int gy0, int max_cycles, float *px, float *py) const
    {
        int stc = sy * nx + sx;
        float dx = 0.0f, dy = 0.0f;
        int npath = 0;
        for (int i = 0; i < max_cycles; ++i) {
            const long near_raw = (long)stc + (long)(int)round((double)dx) + (long)(int)((double)nx * round((double)dy));
            const long nearest = std::max(0L, std::min((long)ns - 1, near_raw));
            if (pot(nearest) < (float)kNeutral) {
                px[npath] = (float)gx0; py[npath] = (float)gy0;
                return ++npath;
            }
            if (stc < nx || stc > ns - nx) return -1;
            px[npath] = (float)(stc % nx) + dx;
            py[npath] = (float)(stc / nx) + dy;
            ++npath;
            const bool osc = npath > 2 && px[npath - 1] == px[npath - 3] && py[npath - 1] == py[npath - 3];
            const int up = stc - nx, dn = stc + nx;
            if (pot(stc) >= kPotHigh || pot(stc + 1) >= kPotHigh || pot(stc - 1) >= kPotHigh || pot(dn) >= kPotHigh || pot(dn + 1) >= kPotHigh ||
                pot(dn - 1) >= kPotHigh || pot(up) >= kPotHigh || pot(up + 1) >= kPotHigh || pot(up - 1) >= kPotHigh || osc) {
                // follow the grid: the lowest of the eight neighbours, compared against the cell's potential truncated to int
                int minc = stc;
                int minp = to_int_x86(pot(stc));
                const int cand[8] = {up - 1, up, up + 1, stc - 1, stc + 1, dn - 1, dn, dn + 1};
                for (int k = 0; k < 8; ++k)
                    if (pot(cand[k]) < (float)minp) { minp = to_int_x86(pot(cand[k])); minc = cand[k]; }
                stc = minc;
                dx = 0.0f; dy = 0.0f;
                if (pot(stc) >= kPotHigh) return -2;
            } else {
                float g[4][2];
                grad(stc, g[0][0], g[0][1]); grad(stc + 1, g[1][0], g[1][1]);
                grad(dn, g[2][0], g[2][1]); grad(dn + 1, g[3][0], g[3][1]);
                const float x1 = (float)((1.0 - (double)dx) * (double)g[0][0] + (double)(dx * g[1][0]));
                const float x2 = (float)((1.0 - (double)dx) * (double)g[2][0] + (double)(dx * g[3][0]));
                const float x = (float)((1.0 - (double)dy) * (double)x1 + (double)(dy * x2));
                const float y1 = (float)((1.0 - (double)dx) * (double)g[0][1] + (double)(dx * g[1][1]));
                const float y2 = (float)((1.0 - (double)dx) * (double)g[2][1] + (double)(dx * g[3][1]));
                const float y = (float)((1.0 - (double)dy) * (double)y1 + (double)(dy * y2));
                if (x == 0.0f && y == 0.0f) return -3;
                const float ss = kPathStep / hyp(x, y);
                dx += x * ss;
                dy += y * ss;
                if (dx > 1.0f) { ++stc; dx = (float)((double)dx - 1.0); }
                if (dx < -1.0f) { --stc; dx = (float)((double)dx + 1.0); }
                if (dy > 1.0f) { stc += nx; dy = (float)((double)dy - 1.0); }
                if (dy < -1.0f) { stc -= nx; dy = (float)((double)dy + 1.0); }
            }
        }
        return -4;
    }
};

// Costmap2D::worldToMap
bool world_to_map(double wx, double wy, double ox, double oy, double res, int nx, int ny, int &mx, int &my)
{
    if (wx < ox || wy < oy) return false;
    const double qx = (wx - ox) / res, qy = (wy - oy) / res;
    if (!(qx < 4294967296.0) || !(qy < 4294967296.0)) return false;
    const unsigned ux = (unsigned)qx, uy = (unsigned)qy;
    if (ux >= (unsigned)nx || uy >= (unsigned)ny) return false;
    mx = (int)ux; my = (int)uy;
    return true;
}

// setPlanForFrontier's heading (quatToEuler's yaw, both angles into [0, 2 pi), the smaller way round)
double heading(const double pose7[7], double gx, double gy)
{
    const double qx = pose7[3], qy = pose7[4], qz = pose7[5], qw = pose7[6];
    double ry = atan2(2.0 * (qw * qz + qx * qy), 1.0 - 2.0 * (qy * qy + qz * qz));
    if (ry < 0) ry = ry + (M_PI * 2);
    double gyaw = atan2(gy - pose7[1], gx - pose7[0]);
    if (gyaw < 0) gyaw = gyaw + (M_PI * 2);
    double h = fabs(ry - gyaw);
    if (h > M_PI) h = (2 * M_PI) - h;
    return h;
}

// the path's length in metres: cells truncated to unsigned, cell centres, segments (i, i+1) for i = len-2 .. 1 in that order
double length_m(const float *px, const float *py, int len, double ox, double oy, double res)
{
    double s = 0.0;
    double prev_x = 0, prev_y = 0;
    for (int i = len - 1; i >= 0; --i) {
        const double wx = ox + ((double)(uint32_t)(int64_t)px[i] + 0.5) * res;
        const double wy = oy + ((double)(uint32_t)(int64_t)py[i] + 0.5) * res;
        if (i != 0 && i != len - 1) {
            const double ex = wx - prev_x, ey = wy - prev_y;
            s += sqrt(ex * ex + ey * ey);
        }
        prev_x = wx; prev_y = wy;
    }
    return s;
}

}  // namespace

extern "C" {

// the converged field [ny][nx]; stats [4] = rounds, tile runs, sweeps, largest sweep count of one tile run (or NULL)
int nr_converged_field(const uint8_t *cells, int nx, int ny, int rx, int ry, int allow_unknown, float *pot, int64_t *stats)
{
    if (nx <= 0 || ny <= 0 || rx < 0 || ry < 0 || rx >= nx || ry >= ny) return -1;
    Map m;
    build_costs(cells, nx, ny, allow_unknown, m);
    std::vector<float> f;
    Stats st;
    converged_field(m, rx, ry, f, st);
    memcpy(pot, f.data(), f.size() * sizeof(float));
    if (stats) { stats[0] = st.rounds; stats[1] = st.tile_runs; stats[2] = st.sweeps; stats[3] = st.max_sweeps; }
    return 0;
}

// planner cost array [ny][nx] (setCostmap isROS + the border ring)
int nr_costs(const uint8_t *cells, int nx, int ny, int allow_unknown, uint8_t *cost)
{
    Map m;
    build_costs(cells, nx, ny, allow_unknown, m);
    memcpy(cost, m.cost.data(), m.cost.size());
    return 0;
}

// One leg over n goals.  leg 0: converged (one field), 1: reference_astar (a field per goal).  Outputs [n]; limit [n] or NULL:
// bit 0 the wave's cycle budget ran out, bit 1 a priority buffer refused a push (leg 1); bits 8.. why calcPath failed (both legs,
// 1 out of bounds, 2 high potential, 3 zero gradient, 4 out of cycles).  path_x / path_y [n][path_stride] or NULL with
// path_stride >= 4 * max(nx, ny): the points of every achievable goal's path as calcPath left them, path_length[i] of them.
static int plan(const uint8_t *cells, int nx, int ny, double ox, double oy, double res, const double robot7[7], int allow_unknown, int leg,
                int n, const double *goal_xyz, const uint8_t *achievable_in, double *path_length, double *path_length_m, double *path_heading,
                uint8_t *achievable, int32_t *limit, float *path_x, float *path_y, int path_stride)
{
    const double dmax = std::numeric_limits<double>::max();
    Map m;
    build_costs(cells, nx, ny, allow_unknown, m);
    int rx = 0, ry = 0;
    const bool robot_on = world_to_map(robot7[0], robot7[1], ox, oy, res, nx, ny, rx, ry);
    std::vector<float> field;
    if (leg == 0 && robot_on) { Stats st; converged_field(m, rx, ry, field, st); }
    const int max_cycles = 4 * std::max(nx, ny);
    if (path_x && path_stride < max_cycles) return -1;
    std::vector<float> px((size_t)max_cycles), py((size_t)max_cycles);
    for (int i = 0; i < n; ++i) {
        path_length[i] = path_length_m[i] = path_heading[i] = dmax;
        achievable[i] = 0;
        if (limit) limit[i] = 0;
        if (achievable_in && !achievable_in[i]) continue;
        const double h = heading(robot7, goal_xyz[3 * i], goal_xyz[3 * i + 1]);
        int gx = 0, gy = 0;
        if (!robot_on || !world_to_map(goal_xyz[3 * i], goal_xyz[3 * i + 1], ox, oy, res, nx, ny, gx, gy)) continue;
        const float *P = nullptr;
        std::vector<float> own;
        if (leg == 0) {
            P = field.data();
            if (!(P[(size_t)gy * nx + gx] < kPotHigh)) continue;
        } else {
            AstarWave w(m);
            w.start[0] = gx; w.start[1] = gy; w.goal[0] = rx; w.goal[1] = ry;
            bool cyc = false;
            const bool ok = w.run(&cyc);
            if (limit) limit[i] = (cyc ? 1 : 0) | (w.cap_hit ? 2 : 0);
            if (!ok) continue;
            own.swap(w.pot);
            P = own.data();
        }
        Descent d{P, nx, nx * ny};
        const int len = d.path(gx, gy, rx, ry, max_cycles, px.data(), py.data());
        if (len <= 0) {
            if (limit) limit[i] |= (-len) << 8;
            continue;
        }
        achievable[i] = 1;
        path_length[i] = (double)len;
        path_length_m[i] = length_m(px.data(), py.data(), len, ox, oy, res);
        path_heading[i] = h;
        if (path_x) memcpy(path_x + (size_t)i * path_stride, px.data(), (size_t)len * sizeof(float));
        if (path_y) memcpy(path_y + (size_t)i * path_stride, py.data(), (size_t)len * sizeof(float));
    }
    return 0;
}

int nr_plan(const uint8_t *cells, int nx, int ny, double ox, double oy, double res, const double robot7[7], int allow_unknown, int leg,
            int n, const double *goal_xyz, const uint8_t *achievable_in, double *path_length, double *path_length_m, double *path_heading,
            uint8_t *achievable, int32_t *limit)
{
    return plan(cells, nx, ny, ox, oy, res, robot7, allow_unknown, leg, n, goal_xyz, achievable_in, path_length, path_length_m, path_heading,
                achievable, limit, nullptr, nullptr, 0);
}

// nr_plan, and the path points of every leg as well (see plan above); -1 when path_stride is too small
int nr_plan_points(const uint8_t *cells, int nx, int ny, double ox, double oy, double res, const double robot7[7], int allow_unknown, int leg,
                   int n, const double *goal_xyz, const uint8_t *achievable_in, double *path_length, double *path_length_m,
                   double *path_heading, uint8_t *achievable, int32_t *limit, float *path_x, float *path_y, int path_stride)
{
    return plan(cells, nx, ny, ox, oy, res, robot7, allow_unknown, leg, n, goal_xyz, achievable_in, path_length, path_length_m, path_heading,
                achievable, limit, path_x, path_y, path_stride);
}

}  // extern "C"
