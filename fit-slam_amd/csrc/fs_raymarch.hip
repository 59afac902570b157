// fs_raymarch.hip — arrival-information kernel for gfx950 (CDNA4).
//
// Replaces the scalar loops of FrontierCostCalculator::setArrivalInformationForFrontier
// (DEP/src/CostCalculator.cpp:23-121) and its callees getTracedCells / bresenham2D /
// RayTracedCells::operator() / isRobotFootprintInLethal (DEP/src/Helpers.cpp:7-96,135-155,
// DEP/include/.../Helpers.hpp:50-77) for a whole frontier list at once.
//
// Mapping: one 64-lane wavefront per candidate, rays strided over the lanes (ray r = lane + 64*j),
// four candidates per 256-thread workgroup.  The grid and the fan-direction table were staged to HBM
// once (fs_upload_grid / fs_set_ray_params).  Per ray: the end point, the clamp, both worldToMap
// truncations, the step count `(unsigned)(scale*abs_da)` are evaluated in fp64 with the exact
// operation order of the reference (basic IEEE ops only: +, -, /, *, sqrt of an exact integer), so
// every integer cell index matches the CPU bit for bit; then an integer Bresenham walk reads one
// byte per step.  Per-yaw sums live in LDS; the FOV window maximum and its first argmax are a
// wave-shuffle reduction.  This is HBM/L2-bound byte gather: no MFMA.
#include "fs_internal.h"
#include "fs_walk.h"        // cell_quotient, world_to_map, sign_ref, minor_step, WalkLinear and its walk_init / walk_step / walk_cell / walk_visits

#ifndef FS_RAY_WAVES
#define FS_RAY_WAVES 4          // candidates per workgroup
#endif
#ifndef FS_RAY_UNROLL
#define FS_RAY_UNROLL 4         // speculative cell loads in flight per lane
#endif

namespace {

__device__ __forceinline__ double std_min(double a, double b) { return (b < a) ? b : a; }   // std::min(a,b)
__device__ __forceinline__ double std_max(double a, double b) { return (a < b) ? b : a; }   // std::max(a,b)

// Two interchangeable walks over the same cell sequence (selected per launch, FsRayArgs::layout; DESIGN.md 4.1 holds the
// measurements, including the five other formulations that were built, measured and removed):
//
// WalkLinear (fs_walk.h) — the reference's own formulation on the dense row-major image: a linear offset, constant strides per
// axis.  Cheapest in instructions; the winner for short rays (up to ~96 cells).
//
// WalkClass — on the 2-bit class image (FsGridDev::cls: bricks of 8 x 8 x 8 cells = one 128-B cache line), which has no
// constant strides.  The walk keeps the cell coordinates IN THE RAY'S OWN AXIS ORDER (a = major, b, c = minors): the major
// coordinate steps unconditionally (the reference's `offset += offset_a`), the minors on their error terms exactly as
// bresenham2D's `error_b` (DEP/src/Helpers.cpp:21-27).  A cell's address is separable over the axes,
//     A = sum over v in (a, b, c) of v * l_v + (v >> 3) * m_v,
// with per-lane constants (l, m) that say which grid axis v is — a shift and two full-rate 24-bit multiply-adds per
// axis — and a cell arrives as its class (bit 0: in the trace range, bit 1: in the obstacle range), so the visitor is two
// bit tests.  More instructions per step than WalkLinear, 4-8x fewer cache lines per ray.
struct WalkClass {
    // cell coordinates along the major and the two minor axes, each PRE-SHIFTED by its axis' position inside a brick (x: 0, y: 3,
    // z: 6 bits): coordinate << s is the axis' share of the in-brick address, so the address needs no multiply for it
    uint32_t a, b, c;
    int sga, sgb, sgc;       // sign(d) with sign(0) = -1 (Helpers.hpp:113-116), shifted likewise: what a step adds
    uint32_t abs_da, adb, adc;
    int eb, ec;
    uint32_t ha, hb, hc;     // s + 3: (coordinate << s) >> (s + 3) = the axis' brick index
    uint32_t ma, mb, mc;     // FsGridDev::cls_m[axis]: brick stride of the axis minus (8 << s)
    uint32_t end;
};

// WalkSparse — WalkClass over the SPARSE class image (FsGridDev::cls_table): the same coordinates and steps, one more
// dependent load per cell (the brick's slot in the pool).  Built as the one measurement of BASELINE.json configs[4]'s "sparse"
// (profiles/EXPERIMENTS.md holds the outcome).
struct WalkSparse : WalkClass {};

__device__ __forceinline__ void walk_step(WalkClass &w)
{
    w.a += (uint32_t)w.sga;
    minor_step(w.b, w.eb, w.adb, w.abs_da, w.sgb);
    minor_step(w.c, w.ec, w.adc, w.abs_da, w.sgc);
}

__device__ __forceinline__ void walk_step(WalkSparse &w) { walk_step(static_cast<WalkClass &>(w)); }

// the class (0..3) of the cell under the walk
__device__ __forceinline__ uint32_t walk_class(const FsGridDev &g, const WalkClass &w)
{
    // (24-bit multiplies run at full rate, 32-bit ones at a quarter of it; brick indices and strides are far below 2^24 —
    // fs_capi.hip only selects this walk where they are)
    // v * (1 << s) + (v >> 3) * m per axis: the first terms are the pre-shifted coordinates themselves (one three-operand add),
    // the second three shifts and three multiply-adds — seven instructions where products of the unshifted coordinates took eleven
    uint32_t A = w.a + w.b + w.c;
    A = (uint32_t)__umul24(w.c >> w.hc, w.mc) + A;
    A = (uint32_t)__umul24(w.b >> w.hb, w.mb) + A;
    A = (uint32_t)__umul24(w.a >> w.ha, w.ma) + A;
#ifdef FS_RAY_BOUNDS
    if (A >= g.cls_cells) { atomicMax(g.dbg, 6ull); return 0u; }
#endif
    const uint32_t word = *reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(g.cls) + ((A >> 2) & ~3u));
    return __builtin_amdgcn_ubfe(word, A << 1, 2u);            // v_bfe_u32 takes the offset modulo 32: field A & 15
}

// ... through the brick table: A >> 9 is the brick (brick-linear order), A & 511 the cell inside it
__device__ __forceinline__ uint32_t walk_class(const FsGridDev &g, const WalkSparse &w)
{
    uint32_t A = w.a + w.b + w.c;
    A = (uint32_t)__umul24(w.c >> w.hc, w.mc) + A;
    A = (uint32_t)__umul24(w.b >> w.hb, w.mb) + A;
    A = (uint32_t)__umul24(w.a >> w.ha, w.ma) + A;
#ifdef FS_RAY_BOUNDS
    if (A >= g.cls_cells) { atomicMax(g.dbg, 6ull); return 0u; }
#endif
    const uint32_t slot = *reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(g.cls_table) + ((A >> 9) << 2));
    const uint32_t B = (slot << 9) | (A & 511u);
    const uint32_t word = *reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(g.cls) + ((B >> 2) & ~3u));
    return __builtin_amdgcn_ubfe(word, A << 1, 2u);
}

__device__ __forceinline__ void walk_init(WalkClass &w, const FsGridDev &g, uint32_t x0, uint32_t y0, uint32_t z0,
                                          uint32_t x1, uint32_t y1, uint32_t z1, double max_length)
{
    const int dx = (int)(x1 - x0), dy = (int)(y1 - y0), dz = (int)(z1 - z0);
    const uint32_t adx = (uint32_t)abs(dx), ady = (uint32_t)abs(dy), adz = (uint32_t)abs(dz);
    const int sx = sign_ref(dx), sy = sign_ref(dy), sz = sign_ref(dz);
    // the axis order of walk_init(WalkLinear): the first largest extent is the major axis
    if (adx >= ady && adx >= adz) {
        w.a = x0; w.b = y0 << 3; w.c = z0 << 6; w.sga = sx; w.sgb = sy * 8; w.sgc = sz * 64; w.abs_da = adx; w.adb = ady; w.adc = adz;
        w.ha = 3; w.hb = 6; w.hc = 9; w.ma = g.cls_m[0]; w.mb = g.cls_m[1]; w.mc = g.cls_m[2];
    } else if (ady >= adz) {
        w.a = y0 << 3; w.b = x0; w.c = z0 << 6; w.sga = sy * 8; w.sgb = sx; w.sgc = sz * 64; w.abs_da = ady; w.adb = adx; w.adc = adz;
        w.ha = 6; w.hb = 3; w.hc = 9; w.ma = g.cls_m[1]; w.mb = g.cls_m[0]; w.mc = g.cls_m[2];
    } else {
        w.a = z0 << 6; w.b = x0; w.c = y0 << 3; w.sga = sz * 64; w.sgb = sx; w.sgc = sy * 8; w.abs_da = adz; w.adb = adx; w.adc = ady;
        w.ha = 9; w.hb = 3; w.hc = 6; w.ma = g.cls_m[2]; w.mb = g.cls_m[0]; w.mc = g.cls_m[1];
    }
    w.eb = w.ec = (int)(w.abs_da / 2);
    w.end = walk_visits(dx, dy, dz, w.abs_da, max_length);
}

__device__ __forceinline__ void walk_init(WalkSparse &w, const FsGridDev &g, uint32_t x0, uint32_t y0, uint32_t z0,
                                          uint32_t x1, uint32_t y1, uint32_t z1, double max_length)
{
    walk_init(static_cast<WalkClass &>(w), g, x0, y0, z0, x1, y1, z1, max_length);
}

// The start cell is the same for every ray of a fan: its worldToMap (three fp64 divisions) is done once per candidate;
// a start point off the map fails every ray, like the reference's `||` of the two conversions (Helpers.cpp:40).
template <typename Walk>
__device__ __forceinline__ bool ray_setup(const FsRayArgs &a, bool start_ok, uint32_t x0, uint32_t y0, uint32_t z0,
                                          double wx, double wy, double wz, Walk &w)
{
    uint32_t x1, y1, z1;
    if (!world_to_map(a.grid, wx, wy, wz, x1, y1, z1) || !start_ok) return false;
    walk_init(w, a.grid, x0, y0, z0, x1, y1, z1, (double)a.max_length);
    return true;
}

// RayTracedCells over the walk: number of cells in [trace_min,trace_max] seen before the first
// cell in [obst_min,obst_max]  (= cells_.size(), DEP/src/CostCalculator.cpp:57-58).
template <typename Walk>
__device__ __forceinline__ int ray_march(const FsRayArgs &a, Walk w)
{
    // the visitor's inclusive ranges, intersected with the byte range of a cell, as one unsigned compare each; an empty
    // range (e.g. the obstacle range (260, 260) of setMaxArrivalInformation) matches nothing
    const int omin = a.obst_min > 0 ? a.obst_min : 0, omax = a.obst_max < 255 ? a.obst_max : 255;
    const int tmin = a.trace_min > 0 ? a.trace_min : 0, tmax = a.trace_max < 255 ? a.trace_max : 255;
    const bool o_any = omax >= omin, t_any = tmax >= tmin;
    const uint32_t orange = o_any ? (uint32_t)(omax - omin) : 0u, trange = t_any ? (uint32_t)(tmax - tmin) : 0u;
    int count = 0;
    uint32_t visits = w.end + 1;          // loop visits + the one after the loop (Helpers.cpp:29)
    // full groups of FS_RAY_UNROLL visits first: every visit of the group exists, so the loads and steps need no per-step
    // bounds (one exec mask per group instead of one per step); the remainder (< FS_RAY_UNROLL visits) goes through the guarded
    // loop below.  Loads past an obstacle are speculative but always inside the start/end bounding box, hence in the grid.
    bool stopped = false;
    while (visits >= FS_RAY_UNROLL) {
        int c[FS_RAY_UNROLL];
#pragma unroll
        for (int u = 0; u < FS_RAY_UNROLL; ++u) {
            c[u] = walk_cell(a.grid, w);
            walk_step(w);                   // (the step behind a ray's very last visit leads nowhere that is read)
        }
        bool hit = false;
#pragma unroll
        for (int u = 0; u < FS_RAY_UNROLL; ++u) {
            const bool traced = t_any && !hit && (uint32_t)(c[u] - tmin) <= trange;
            count += traced ? 1 : 0;
            hit = hit || (o_any && (uint32_t)(c[u] - omin) <= orange);
        }
        if (hit) { stopped = true; break; }  // nothing is pushed after the first obstacle
        visits -= FS_RAY_UNROLL;
    }
    if (stopped) visits = 0;
    while (visits > 0) {
        // the last, partial group: up to FS_RAY_UNROLL - 1 independent byte loads, then classify them in order
        int c[FS_RAY_UNROLL];
        const uint32_t nb = visits < FS_RAY_UNROLL ? visits : FS_RAY_UNROLL;
#pragma unroll
        for (int u = 0; u < FS_RAY_UNROLL; ++u) {
            c[u] = -1;
            if ((uint32_t)u < nb) {
                c[u] = walk_cell(a.grid, w);
                walk_step(w);
            }
        }
        // classify in order, without branches: a cell counts if no earlier cell of the ray was an obstacle
        // (Helpers.hpp:64-71: the traced test comes before hit_obstacle is set, so an obstacle cell itself still counts
        // when the two ranges overlap); slots past `nb` hold -1 and match no range
        bool hit = false;
#pragma unroll
        for (int u = 0; u < FS_RAY_UNROLL; ++u) {
            const bool traced = t_any && !hit && (uint32_t)(c[u] - tmin) <= trange;
            count += traced ? 1 : 0;
            hit = hit || (o_any && (uint32_t)(c[u] - omin) <= orange);
        }
        if (hit) break;                    // nothing is pushed after the first obstacle
        visits -= nb;
    }
    return count;
}

// The visitor over the class image (the classes were cut with this launch's ranges: fs_capi.hip keeps them in step): bit 0
// counts while no earlier cell of the ray carried bit 1 (Helpers.hpp:64-71 — the traced test comes before hit_obstacle is set,
// so a cell in both ranges still counts).
template <typename W>
__device__ __forceinline__ int ray_march_classes(const FsRayArgs &a, W w)
{
    int count = 0;
    uint32_t visits = w.end + 1;
    uint32_t open = 1u;                              // 1 until the first obstacle
    while (visits >= FS_RAY_UNROLL) {
        uint32_t c[FS_RAY_UNROLL];
#pragma unroll
        for (int u = 0; u < FS_RAY_UNROLL; ++u) {
            c[u] = walk_class(a.grid, w);
            walk_step(w);
        }
#pragma unroll
        for (int u = 0; u < FS_RAY_UNROLL; ++u) {
            count += (int)(c[u] & open);
            open &= ~(c[u] >> 1);
        }
        if (!open) return count;
        visits -= FS_RAY_UNROLL;
    }
    if (visits > 0) {
        // the last, partial group as ONE batch of independent loads (a loop of single visits would expose a load latency
        // per step); slots past the ray's end hold class 0, which neither counts nor stops
        uint32_t c[FS_RAY_UNROLL - 1];
#pragma unroll
        for (int u = 0; u < FS_RAY_UNROLL - 1; ++u) {
            c[u] = 0u;
            if ((uint32_t)u < visits) {
                c[u] = walk_class(a.grid, w);
                walk_step(w);
            }
        }
#pragma unroll
        for (int u = 0; u < FS_RAY_UNROLL - 1; ++u) {
            count += (int)(c[u] & open);
            open &= ~(c[u] >> 1);
        }
    }
    return count;
}

__device__ __forceinline__ int ray_march(const FsRayArgs &a, WalkClass w) { return ray_march_classes(a, w); }
__device__ __forceinline__ int ray_march(const FsRayArgs &a, WalkSparse w) { return ray_march_classes(a, w); }

// Every wave of the kernel below works on LDS of its own (per-yaw sums, tile, descriptors): what it wrote must be visible to
// its own later reads — which the LDS guarantees per wave, in program order — so the points where that matters need the
// compiler to keep the order, not a workgroup barrier.  (With s_barrier there the four fans of a workgroup waited for the
// slowest of them twice, and a finished wave kept its slot until the whole workgroup was done.)
__device__ __forceinline__ void wave_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// The robot-footprint disc (isRobotFootprintInLethal, DEP/src/Helpers.cpp:135-155) in the start cell's z slice: the cells of the
// side x side square within the radius, 64 per pass of the wave.  It is the one part of the kernel that reads the row-major byte
// image behind a class walk — lines the fan has not touched, cold in L2 — so the passes go in groups of FS_RAY_DISC_GROUP
// independent loads, and what does not depend on the pass is worked out once per wave.  (Issuing the loads in front of the
// fan's rounds instead, to be folded in behind them, was built and measured: slower on C3 and on REF2D — DESIGN.md 4.1.)
#ifndef FS_RAY_DISC_GROUP
#define FS_RAY_DISC_GROUP 2     // independent loads per group (1, 2, 4 measured: profiles/r06/ray_disc.json)
#endif
struct Disc {
    const uint8_t *slice;       // the start cell's z slice of the byte image (the scan needs the cost itself: 254)
    double r2;                  // radius^2 as the reference forms it: fp64 product of the fp64 radius
    float inv_side;
    int ri, side, cells;        // (int)radius, 2 ri + 1, side^2
    uint32_t nx, ny, x0, y0;    // grid extent, start cell
};

// The cost of cell t of the disc's scan order (row-major over the square); `in`: t is a cell of the square, within the radius
// and on the grid (off-grid cells are not lethal).  Every lane loads — the others the start cell, which is on the grid, and
// their `in` discards it: a load under a per-lane condition sits in a block of its own, where the compiler waits for it on the
// spot, and a group of them arrives one after the other.
__device__ __forceinline__ uint32_t disc_cell(const Disc &d, int t, bool &in)
{
    // t / side and t % side without the integer division: the float quotient is within one of the true row for
    // t < 2^22 (side <= 2048; larger discs divide), and one step on the remainder makes it exact
    int row = d.side <= 2048 ? (int)(((float)t + 0.5f) * d.inv_side) : t / d.side;
    int col = t - row * d.side;
    if (col < 0) { --row; col += d.side; } else if (col >= d.side) { ++row; col -= d.side; }
    const int dx = row - d.ri, dy = col - d.ri;
    const uint32_t x = d.x0 + (uint32_t)dx, y = d.y0 + (uint32_t)dy;
    in = t < d.cells && (double)(dx * dx + dy * dy) <= d.r2 && x < d.nx && y < d.ny;
    return d.slice[(size_t)(in ? y : d.y0) * (size_t)d.nx + (in ? x : d.x0)];
}

#ifdef FS_RAY_WAVES_PER_EU
#define FS_RAY_OCCUPANCY __attribute__((amdgpu_waves_per_eu(FS_RAY_WAVES_PER_EU)))
#else
#define FS_RAY_OCCUPANCY
#endif
template <typename Walk>
__global__ __launch_bounds__(FS_RAY_WAVES * 64) FS_RAY_OCCUPANCY
void fs_raymarch_kernel(const FsRayArgs a)
{
    extern __shared__ int fs_ray_lds[];          // [FS_RAY_WAVES][n_yaw] per-yaw sums over the elevation rings
    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    // Workgroups are dealt round-robin over the 8 XCDs (block b -> XCD b % 8), each with its own L2.  With the
    // candidate list in spatial (Morton) order, give every XCD a contiguous run of it so that neighbouring fans
    // share cache lines in ONE L2: position p of the sorted list is served by block (p % per) * 8 + p / per.
    const int per = (int)(gridDim.x >> 3);
    const int slot_block = a.perm ? (int)(blockIdx.x & 7u) * per + (int)(blockIdx.x >> 3) : (int)blockIdx.x;
    const int slot = slot_block * FS_RAY_WAVES + wave;
    const bool active = slot < a.n;
    const int c = active ? (a.perm ? a.perm[slot] : slot) : 0;
    int *ysum = fs_ray_lds + wave * a.n_yaw;
    const int n_rays = a.n_yaw * a.n_elev;

    for (int i = lane; i < a.n_yaw; i += 64) ysum[i] = 0;
    wave_lds_fence();

    bool black = false;
    double sx = 0, sy = 0, sz = 0;
    int fsize_v = 0;
    if (active) {
        black = a.blacklisted && a.blacklisted[c];
        sx = a.goal[3 * c]; sy = a.goal[3 * c + 1]; sz = a.goal[3 * c + 2];
        if (a.frontier_size) fsize_v = a.frontier_size[c];
    }
    // (read here, with the candidate's other columns, and not behind the fan, where nothing would hide the load; the size is the
    // same in every lane: as a scalar it costs the fan no vector register and the scan's skip is one scalar branch)
    const int fsize = __builtin_amdgcn_readfirstlane(fsize_v);
    bool fail = false;
    uint32_t sxm = 0, sym = 0, szm = 0;
    const bool start_ok = active && world_to_map(a.grid, sx, sy, sz, sxm, sym, szm);
    if (active && !black) {
        for (int r = lane; r < n_rays; r += 64) {
            // ray r = e * n_yaw + i: one elevation ring per wave instruction.  (Dealing the class walk's rays ring-fastest — a
            // sector of 64 / n_elev yaws per instruction, whose rays tend to end at the same wall — measured +-1 %: r03.)
            const int i = r % a.n_yaw;
            // DEP/src/CostCalculator.cpp:42-43: wx = sx + (MAX_CAMERA_DEPTH * cos(theta))
            double wx = sx + a.dir[3 * r];
            double wy = sy + a.dir[3 * r + 1];
            double wz = sz + a.dir[3 * r + 2];
            if (a.clamp) {                                  // :47-48
                wx = std_max(a.lo_x, std_min(a.hi_x, wx));
                wy = std_max(a.lo_y, std_min(a.hi_y, wy));
                wz = std_max(a.lo_z, std_min(a.hi_z, wz));
            }
            Walk w;
            int count = 0;
            if (ray_setup(a, start_ok, sxm, sym, szm, wx, wy, wz, w)) count = ray_march(a, w);
            else fail = true;
            if (count) atomicAdd(&ysum[i], count);
            if (a.ray_counts) a.ray_counts[(size_t)c * n_rays + r] = count;
        }
    }
    const bool any_fail = __any(fail);           // :50-55 — the first failing ray aborts the candidate
    wave_lds_fence();
    if (!active) return;

    uint8_t ach = a.achievable_in ? a.achievable_in[c] : (uint8_t)1;
    if (black || any_fail) {
        if (a.ray_counts)
            for (int r = lane; r < n_rays; r += 64) a.ray_counts[(size_t)c * n_rays + r] = 0;
        if (lane == 0) {
            a.arrival[c] = 0; a.argmax[c] = 0; a.yaw[c] = 0.0; a.achievable[c] = ach;
            a.status[c] = black ? FS_STATUS_BLACKLISTED : FS_STATUS_OFF_MAP;
            if (a.records) {
                fs_record r{};
                r.flags = (ach ? FS_FLAG_ACHIEVABLE : 0u) | ((uint32_t)(black ? FS_STATUS_BLACKLISTED : FS_STATUS_OFF_MAP) << 8);
                a.records[c] = r;
            }
        }
        return;
    }

    // The footprint verdict is read in one place, `lethal && frontier_size < 10` (CostCalculator.cpp:77-82): a larger frontier
    // skips the scan altogether.  (No frontier sizes: 0, the scan runs.)
#ifdef FS_RAY_ABLATE_DISC    // timing only (tools/ray_disc_probe.py): no scan at all, `achievable` is wrong by construction
    const bool scan = false;
    (void)fsize;
#else
    const bool scan = (double)fsize < 10.0;
#endif
    if (scan) {
        Disc disc;
        disc.ri = (int)a.footprint_radius;
        disc.side = 2 * disc.ri + 1;
        disc.cells = disc.side * disc.side;
        disc.inv_side = 1.0f / (float)disc.side;
        disc.r2 = a.footprint_radius * a.footprint_radius;
        disc.slice = a.grid.cells + (size_t)szm * (size_t)a.grid.ny * (size_t)a.grid.nx;
        disc.nx = (uint32_t)a.grid.nx; disc.ny = (uint32_t)a.grid.ny; disc.x0 = sxm; disc.y0 = sym;
        bool lethal = false;
        for (int t0 = 0; t0 < disc.cells; t0 += 64 * FS_RAY_DISC_GROUP) {
            uint32_t dv[FS_RAY_DISC_GROUP];
            bool in[FS_RAY_DISC_GROUP];
#pragma unroll
            for (int u = 0; u < FS_RAY_DISC_GROUP; ++u) dv[u] = disc_cell(disc, t0 + 64 * u + lane, in[u]);
#pragma unroll
            for (int u = 0; u < FS_RAY_DISC_GROUP; ++u) lethal = lethal || (in[u] && dv[u] == 254u);
        }
        if (__any(lethal)) ach = 0;
    }

    // FOV window, no wrap-around, first maximum (CostCalculator.cpp:87-107)
    const int k = a.window;
    int best = -1, best_i = 0x7fffffff;
    for (int i = lane; i <= a.n_yaw - k; i += 64) {
        int s = 0;
        for (int j = 0; j < k; ++j) s += ysum[i + j];
        if (s > best) { best = s; best_i = i; }            // ascending i per lane: strict > keeps the first
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int ob = __shfl_xor(best, d), oi = __shfl_xor(best_i, d);
        if (ob > best || (ob == best && oi < best_i)) { best = ob; best_i = oi; }
    }
    if (lane == 0) {
        a.arrival[c] = best;                                // :112
        if ((double)best < a.min_gt) ach = 0;              // :114-118
        a.argmax[c] = best_i;
        a.yaw[c] = ((double)best_i * a.delta_theta) + a.half_fov;   // :119, half_fov = CAMERA_FOV / 2
        a.achievable[c] = ach;
        a.status[c] = FS_STATUS_OK;
        if (a.records) {
            fs_record r{};
            r.arrival = best; r.argmax = best_i;
            r.yaw = (float)(((double)best_i * a.delta_theta) + a.half_fov);
            r.flags = (ach ? FS_FLAG_ACHIEVABLE : 0u) | ((uint32_t)FS_STATUS_OK << 8);
            a.records[c] = r;
        }
    }
    // pose (goal, best yaw) of the Fisher-information stage as one 48-byte record: rotation of
    // orientationAroundZAxis(yaw) (table indexed by the argmax) and the float32 translation of getTransformFromPose
    if (a.pose12 && lane < 12) {
        const float v = lane < 9 ? a.yawR[9 * best_i + lane] : (float)a.goal[3 * (size_t)c + (lane - 9)];
        a.pose12[12 * (size_t)c + lane] = v;
    }
}

// One segment: getTracedCells(sx, sy, wx, wy, visitor, max_length, costmap) for arbitrary end points
// (DEP/src/Helpers.cpp:32-96) with every RayTracedCells accessor (Helpers.hpp:83-101).  Unlike the arrival
// fan the walk never stops early: unknown_cells_ and all_cells_count_ keep counting behind an obstacle.
struct SegResult {
    int traced, unknown, all;
    bool hit, ok;
};

template <typename Walk>
__device__ __forceinline__ SegResult segment_walk(const FsGridDev &g, double sx, double sy, double sz, double wx, double wy, double wz,
                                                  double max_length, int obst_min, int obst_max, int trace_min, int trace_max)
{
    uint32_t x1, y1, z1, x0, y0, z0;
    int traced = 0, unknown = 0, all = 0;
    bool hit = false, ok = false;
    if (world_to_map(g, wx, wy, wz, x1, y1, z1) && world_to_map(g, sx, sy, sz, x0, y0, z0)) {
        ok = true;
        Walk w;
        walk_init(w, g, x0, y0, z0, x1, y1, z1, max_length);
        for (uint32_t v = 0; v <= w.end; ++v) {
            const int c = walk_cell(g, w);
            {
                ++all;                                                    // Helpers.hpp:62
                if (c <= trace_max && c >= trace_min && !hit) ++traced;   // :64-67
                if (c >= obst_min && c <= obst_max) hit = true;           // :68-71
                if (c == 255) ++unknown;                                  // :72-75
            }
            walk_step(w);
        }
    }
    return SegResult{traced, unknown, all, hit, ok};
}

// One lane per segment
template <typename Walk>
__global__ void fs_segments_kernel(const FsSegArgs s)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= s.n) return;
    const SegResult r = segment_walk<Walk>(s.grid, s.start[3 * i], s.start[3 * i + 1], s.start[3 * i + 2], s.end[3 * i], s.end[3 * i + 1],
                                           s.end[3 * i + 2], s.max_length, s.obst_min, s.obst_max, s.trace_min, s.trace_max);
    s.ok[i] = r.ok; s.hit[i] = r.hit;
    s.traced[i] = r.traced; s.unknown[i] = r.unknown; s.all[i] = r.all;
}

// fs_line_of_sight: the line-of-sight rule of fs_set_occlusion (fs_walk.h, line_of_sight) for caller-given pairs, one lane per pair
__global__ void fs_los_kernel(const FsLosArgs s)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= s.n) return;
    const LosResult r = line_of_sight(s.grid, s.from[3 * i], s.from[3 * i + 1], s.from[3 * i + 2], s.to[3 * i], s.to[3 * i + 1], s.to[3 * i + 2],
                                      s.occ_min, s.occ_max, s.margin);
    s.ok[i] = r.ok; s.blocked[i] = r.blocked;
    if (s.tested) s.tested[i] = r.tested;
}

// FrontierRoadMap::refinePath (DEP/src/planners/FrontierRoadmap.cpp:657-714) on every route of fs_roadmap_routes,
// one wave per route.  From the kept node P[kk] the reference tries P[kk + 1], P[kk + 2], ... in turn and stops at the first that
// isConnectable (:716-737: walk ok, nothing in 253..254, unknown cells <= the limit) refuses; the last one it accepted is kept
// next.  Here lane l walks P[kk] -> P[next + l], 64 candidates a round, and a ballot finds the first refusal: the lanes behind
// it have walked for nothing, the verdicts in front of it are the sequential scan's.  A node that cannot see its own successor
// ends the list (complete = 0).
__global__ __launch_bounds__(256) void fs_route_refine_kernel(const FsRouteRefineArgs a)
{
    const int32_t r = (int32_t)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= a.n_routes) return;
    const int64_t base = a.node_off[r];
    const int32_t m = (int32_t)(a.node_off[r + 1] - base);
    const int32_t *P = a.node + base;
    int32_t *R = a.refined + base;
    const double oz = a.grid.oz;
    int32_t kk = 0, nr = m > 0 ? 1 : 0;
    uint8_t complete = 1;
    unsigned long long walks = 0;
    if (lane == 0 && m > 0) R[0] = P[0];
    while (kk < m - 1) {
        const int32_t from = P[kk];
        const double fx = a.xy[2 * from], fy = a.xy[2 * from + 1];
        int32_t next = kk + 1;
        bool refused = false;
        while (next < m && !refused) {
            const int32_t j = next + lane;
            bool bad = false;
            if (j < m) {
                const int32_t to = P[j];
                const SegResult s = segment_walk<WalkLinear>(a.grid, fx, fy, oz, a.xy[2 * to], a.xy[2 * to + 1], oz, a.max_length, 253, 254, 0, 255);
                bad = !(s.ok && !s.hit && !((double)s.unknown > a.unknown_limit));
            }
            const int32_t tried = m - next < 64 ? m - next : 64;
            walks += (unsigned long long)tried;
            const uint64_t mask = __ballot(bad);
            if (mask) { next += __builtin_ctzll(mask); refused = true; }
            else next += tried;
        }
        if (next - 1 == kk) { complete = 0; break; }
        if (lane == 0) R[nr] = P[next - 1];
        ++nr;
        kk = next - 1;
    }
    if (lane == 0) {
        a.refined_len[r] = nr;
        a.complete[r] = complete;
        if (walks) atomicAdd(a.walks, walks);
    }
}

__global__ void fs_selftest_kernel(int32_t max_abs, double *out_sqrt, double *out_div)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int side = max_abs + 1;
    if (t >= side * side) return;
    const int dx = t / side, dy = t % side;
    const long long d2 = (long long)dx * dx + (long long)dy * dy;
    const double dist = sqrt((double)d2);
    out_sqrt[t] = dist;
    out_div[t] = (dist == 0.0) ? 1.0 : 40.0 / dist;
}

}  // namespace

hipError_t fs_launch_raymarch(const FsRayArgs &a, hipStream_t s)
{
    if (a.n <= 0) return hipSuccess;
    int blocks = (a.n + FS_RAY_WAVES - 1) / FS_RAY_WAVES;
    if (a.perm) blocks = (blocks + 7) / 8 * 8;               // whole XCD rounds for the remap above
    const size_t lds = sizeof(int) * (size_t)FS_RAY_WAVES * (size_t)a.n_yaw;
    if (a.layout == 2) hipLaunchKernelGGL(fs_raymarch_kernel<WalkSparse>, dim3(blocks), dim3(FS_RAY_WAVES * 64), lds, s, a);
    else if (a.layout == 1) hipLaunchKernelGGL(fs_raymarch_kernel<WalkClass>, dim3(blocks), dim3(FS_RAY_WAVES * 64), lds, s, a);
    else hipLaunchKernelGGL(fs_raymarch_kernel<WalkLinear>, dim3(blocks), dim3(FS_RAY_WAVES * 64), lds, s, a);
    return hipGetLastError();
}

hipError_t fs_launch_segments(const FsSegArgs &a, hipStream_t s)
{
    if (a.n <= 0) return hipSuccess;
    // (the segment visitor reports unknown cells separately from its ranges: it needs the costs, hence the byte image)
    hipLaunchKernelGGL(fs_segments_kernel<WalkLinear>, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t fs_launch_los(const FsLosArgs &a, hipStream_t s)
{
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(fs_los_kernel, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t fs_launch_route_refine(const FsRouteRefineArgs &a, hipStream_t s)
{
    if (a.n_routes <= 0) return hipSuccess;
    hipLaunchKernelGGL(fs_route_refine_kernel, dim3((unsigned)((a.n_routes + 3) / 4)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t fs_launch_selftest(int32_t max_abs, double *d_sqrt, double *d_div, hipStream_t s)
{
    const int side = max_abs + 1;
    const int total = side * side;
    hipLaunchKernelGGL(fs_selftest_kernel, dim3((total + 255) / 256), dim3(256), 0, s, max_abs, d_sqrt, d_div);
    return hipGetLastError();
}
