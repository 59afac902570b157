// fs_search.hip — the order-dependent tail of FrontierSearch::buildNewFrontier (DEP/src/FrontierSearch.cpp:98-216) on the GPU, gfx950
// (DESIGN.md 4.13).  Starts from what fs_frontier_clusters' kernels leave on the device (parent_f: every frontier cell's component
// root; aux[root] == -2: a component the search found) and produces the reference's Frontier records without the label image
// leaving the device:
//   components   found roots compacted in ascending label order (a deterministic scan);
//   seeds        Nearest: per component the cell nearest the robot's cell (squared cell distance, ties to the smaller index);
//                Reference: searchFrom's outer search (:44-94) walked level by level over the expanded cells from the start
//                cell in nhood4 order, a cell going to its first claimant (the smallest queue position: one parent reaches a
//                cell through one slot only); each component's seed is the frontier neighbour of a popped cell at the smallest
//                (queue position, slot), and the components are emitted in that order;
//                or the caller's list, validated on the device (a found frontier cell, one seed per component);
//   queue order  per seed the breadth-first walk in nhood8 order, level-synchronous and exact: every unvisited neighbour n of a
//                level-L cell at queue position t takes atomicMin(key[n], 8 t + slot); a parent's won slots, in slot order, after
//                an exclusive scan over the level's parents in queue order, are the level-(L+1) queue positions;
//   pieces       queue positions [k (max + 1), (k + 1)(max + 1)), the remainder if it exceeds min (searchFrom's filter, :81);
//   goal points  getCentroidOfCells in queue order, SortByMedianFunctor's angles and libstdc++'s std::sort restated
//                (fs_median_sort.h), the middle element — one lane per piece.
// One workgroup walks one component at a time with its queue in global memory; every loop is bounded by the component's size.
// The outer walk is one workgroup too, its queue in the same array before the components' walks use it.
#include "fs_internal.h"
#include "fs_median_sort.h"

namespace {

constexpr int SCAN_THREADS = 1024;
constexpr int BFS_THREADS = 256;
constexpr int OUTER_THREADS = 1024;
constexpr int32_t KEY_NONE = 0x7fffffff;

__device__ __forceinline__ int32_t ld_agent(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned long long ld_agent64(const unsigned long long *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// exclusive scan over the workgroup (blockDim.x a multiple of 64, at most 1024); *total = the sum
__device__ int block_exclusive_scan(int v, int *s_wave, int *total)
{
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    int incl = v;
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
    }
    if (lane == 63) s_wave[wid] = incl;
    __syncthreads();
    if (wid == 0) {
        int w = lane < nw ? s_wave[lane] : 0;
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(w, d, 64);
            if (lane >= d) w += o;
        }
        if (lane < nw) s_wave[lane] = w;
    }
    __syncthreads();
    const int prefix = (wid > 0 ? s_wave[wid - 1] : 0) + incl - v;
    *total = s_wave[nw - 1];
    __syncthreads();
    return prefix;
}

// nhood8's slots (Helpers.cpp:199-252): left, right, up, down, -1-sx, -1+sx, +1-sx, +1+sx; -1 off the map
__device__ __forceinline__ int nb8(int idx, int j, int nx, int ny)
{
    const int y = idx / nx, x = idx - y * nx;
    const bool l = x > 0, r = x < nx - 1, u = y > 0, d = y < ny - 1;
    switch (j) {
    case 0: return l ? idx - 1 : -1;
    case 1: return r ? idx + 1 : -1;
    case 2: return u ? idx - nx : -1;
    case 3: return d ? idx + nx : -1;
    case 4: return (l && u) ? idx - 1 - nx : -1;
    case 5: return (l && d) ? idx - 1 + nx : -1;
    case 6: return (r && u) ? idx + 1 - nx : -1;
    default: return (r && d) ? idx + 1 + nx : -1;
    }
}

// nhood4's slots (Helpers.cpp:185-216): left, right, -nx, +nx; -1 off the map
__device__ __forceinline__ int nb4(int idx, int j, int nx, int ny)
{
    const int y = idx / nx, x = idx - y * nx;
    switch (j) {
    case 0: return x > 0 ? idx - 1 : -1;
    case 1: return x < nx - 1 ? idx + 1 : -1;
    case 2: return y > 0 ? idx - nx : -1;
    default: return y < ny - 1 ? idx + nx : -1;
    }
}

__device__ __forceinline__ bool found_cell(const FsSearchArgs &a, int i, int *root)
{
    const int r = a.parent_f[i];
    *root = r;
    return r >= 0 && a.aux[r] == -2;
}

// per cell: reset the walk's key / position, count the found roots of this block
__global__ void fss_count_kernel(const FsSearchArgs a)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = a.nx * a.ny;
    bool root = false;
    if (i < n) {
        a.key[i] = KEY_NONE;
        a.pos[i] = -1;
        int r;
        root = found_cell(a, i, &r) && r == i;
    }
    const int c = __syncthreads_count(root);
    if (threadIdx.x == 0) a.bcount[blockIdx.x] = c;
}

// one workgroup: exclusive scan of the per-block root counts; state[0] = components
__global__ void fss_scan_blocks_kernel(const FsSearchArgs a, int nb)
{
    __shared__ int s_wave[16];
    int carry = 0;
    for (int b0 = 0; b0 < nb; b0 += blockDim.x) {
        const int b = b0 + threadIdx.x;
        const int v = b < nb ? a.bcount[b] : 0;
        int total;
        const int off = block_exclusive_scan(v, s_wave, &total);
        if (b < nb) a.bcount[b] = carry + off;
        carry += total;
    }
    if (threadIdx.x == 0) {
        a.state[FSS_COMPONENTS] = carry;
        a.state[FSS_EMITTED] = a.n_seeds < 0 ? carry : a.n_seeds;
    }
}

// per cell: found roots get their component index (ascending label) and the component's slots are reset
__global__ void fss_scatter_kernel(const FsSearchArgs a)
{
    __shared__ int s_wave[16];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    bool root = false;
    if (i < a.nx * a.ny) {
        int r;
        root = found_cell(a, i, &r) && r == i;
    }
    int total;
    const int rank = block_exclusive_scan(root ? 1 : 0, s_wave, &total);
    if (root) {
        const int c = a.bcount[blockIdx.x] + rank;
        a.comp_root[c] = i;
        a.cidx[i] = c;
        a.best_d2[c] = ~0ull;
        a.best_idx[c] = KEY_NONE;
        a.csize[c] = 0;
        a.owner[c] = -1;
    }
}

// per cell: component sizes; Nearest: the smallest squared distance to the robot's cell; Reference: the outer walk's cell classes
__global__ void fss_member_kernel(const FsSearchArgs a)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.nx * a.ny) return;
    int r;
    const bool found = found_cell(a, i, &r);
    if (a.outer) a.best_idx[i] = a.parent_t[i] >= 0 ? -1 : found ? a.cidx[r] : -2;      // the outer walk's cell classes
    if (!found) return;
    const int c = a.cidx[r];
    atomicAdd(&a.csize[c], 1);
    if (a.n_seeds < 0 && !a.outer) {
        const long long ry = a.robot_cell / a.nx, rx = a.robot_cell - ry * a.nx;
        const long long y = i / a.nx, x = i - y * a.nx;
        const unsigned long long d2 = (unsigned long long)((x - rx) * (x - rx) + (y - ry) * (y - ry));
        atomicMin(&a.best_d2[c], d2);
    }
}

// Nearest: among the cells at the smallest distance, the smallest index
__global__ void fss_nearest_kernel(const FsSearchArgs a)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.nx * a.ny) return;
    int r;
    if (!found_cell(a, i, &r)) return;
    const int c = a.cidx[r];
    const long long ry = a.robot_cell / a.nx, rx = a.robot_cell - ry * a.nx;
    const long long y = i / a.nx, x = i - y * a.nx;
    const unsigned long long d2 = (unsigned long long)((x - rx) * (x - rx) + (y - ry) * (y - ry));
    if (d2 == a.best_d2[c]) atomicMin(&a.best_idx[c], i);
}

// the emission list: Nearest, component k in label order; or the caller's seed k, checked (a found frontier cell, the first
// seed of its component) — a bad seed sets state[FSS_ERROR]
__global__ void fss_emit_kernel(const FsSearchArgs a)
{
    const int n_emit = a.n_seeds < 0 ? a.state[FSS_COMPONENTS] : a.n_seeds;
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < n_emit; k += gridDim.x * blockDim.x) {
        if (a.n_seeds < 0) {
            a.emit_comp[k] = k;
            a.emit_seed[k] = a.best_idx[k];
            continue;
        }
        const int s = a.seeds[k];
        int r, c = -1;
        if (s >= 0 && s < a.nx * a.ny && found_cell(a, s, &r)) {
            c = a.cidx[r];
            if (atomicCAS(&a.owner[c], -1, k) != -1) c = -1;
        }
        if (c < 0) atomicExch(&a.state[FSS_ERROR], 1);
        a.emit_comp[k] = c;
        a.emit_seed[k] = s;
    }
}

// Reference seeds: searchFrom's outer search (DEP/src/FrontierSearch.cpp:44-94), one workgroup, level by level over E (the cells the
// clusters kernels mark expandable, parent_t >= 0, plus the start cell), from the start cell (clusters state[0]).  Scratch: the queue
// in q; per cell its class in best_idx (fss_member_kernel: -1 in E, c >= 0 a cell of found component c, -2 neither) and its claim
// in key (reset by fss_count_kernel); the components' first hits in best_d2 (reset by fss_scatter_kernel).  Per level:
//   claims  every E neighbour of a popped cell at queue position t takes atomicMin(key, t) — one parent reaches a cell through one
//           slot only, so t alone is the reference's (position, slot) order; a cell claimed at an earlier level (or the start
//           cell, key -1) keeps its smaller key, so the claim is also the visited mark;
//   hits    a frontier neighbour of found component C takes atomicMin(hit[C], 4 t + slot) (64-bit);
//   order   each parent counts, in slot order, the cells it won and the components it hit first; an exclusive scan over the level's
//           parents in queue order gives the next level's queue positions and the components' emission ranks.
// A component first hit at level L is final once level L is done, so the walk ends when every found component has been hit (exact);
// a found component never hit is an internal error (state[FSS_ERROR] = 2).  Levels and popped cells go to the state.
__global__ void __launch_bounds__(OUTER_THREADS) fss_outer_kernel(const FsSearchArgs a)
{
    __shared__ int s_wave[16];
    const int n = a.nx * a.ny, n_comp = a.state[FSS_COMPONENTS];
    if (n_comp == 0) return;                                          // (nothing to order: no levels walked)
    const int start = a.fc_state[0];
    const int32_t *cls = a.best_idx;
    unsigned long long *hit = a.best_d2;
    if (threadIdx.x == 0) { a.q[0] = start; a.key[start] = -1; }
    __syncthreads();
    int lo = 0, hi = 1, levels = 0, ranked = 0;
    for (int iter = 0; iter < n && lo < hi && ranked < n_comp; ++iter) {
        // a level of at most blockDim.x cells (the common case) keeps each lane's parent, neighbours and classes in registers
        // from the first pass to the second
        const bool one = hi - lo <= (int)blockDim.x;
        int nb[4] = {-1, -1, -1, -1}, cl[4] = {-2, -2, -2, -2};
        auto load = [&](int t) {
            const int p = a.q[t];
            for (int j = 0; j < 4; ++j) {
                nb[j] = nb4(p, j, a.nx, a.ny);
                cl[j] = nb[j] >= 0 ? cls[nb[j]] : -2;
            }
        };
        for (int t = lo + (int)threadIdx.x; t < hi; t += blockDim.x) {
            load(t);
            for (int j = 0; j < 4; ++j) {
                if (cl[j] == -1) atomicMin(&a.key[nb[j]], t);
                else if (cl[j] >= 0) atomicMin(&hit[cl[j]], (unsigned long long)t * 4 + j);
            }
        }
        __syncthreads();
        // (a claim or hit key names one parent position, which is never reused, so a key of an earlier level cannot match)
        int carry_c = 0, carry_h = 0;
        for (int t0 = lo; t0 < hi; t0 += blockDim.x) {
            const int t = t0 + (int)threadIdx.x;
            int won = 0, first = 0;
            if (t < hi) {
                if (!one) load(t);
                for (int j = 0; j < 4; ++j) {
                    if (cl[j] == -1 && ld_agent(&a.key[nb[j]]) == t) won |= 1 << j;
                    else if (cl[j] >= 0 && ld_agent64(&hit[cl[j]]) == (unsigned long long)t * 4 + j) first |= 1 << j;
                }
            }
            // both counts in one scan: per pass of blockDim.x parents each sum is at most 4 * 1024 < 2^16
            int total;
            const int off = block_exclusive_scan(__popc(won) | __popc(first) << 16, s_wave, &total);
            int w = hi + carry_c + (off & 0xffff), k = ranked + carry_h + (off >> 16);
            for (int j = 0; j < 4; ++j) {
                if ((won >> j) & 1) {
                    if (w < n) a.q[w] = nb[j];
                    ++w;
                } else if ((first >> j) & 1) {
                    if (k < n_comp) { a.emit_comp[k] = cl[j]; a.emit_seed[k] = nb[j]; }
                    ++k;
                }
            }
            carry_c += total & 0xffff;
            carry_h += total >> 16;
        }
        __syncthreads();
        ++levels;
        lo = hi;
        hi = min(hi + carry_c, n);
        ranked += carry_h;
    }
    if (threadIdx.x == 0) {
        a.state[FSS_OUTER_LEVELS] = levels;
        a.state[FSS_OUTER_POPPED] = lo;
        if (ranked != n_comp) atomicExch(&a.state[FSS_ERROR], 2);
        a.key[start] = KEY_NONE;                                      // (the start cell may be a frontier cell the walks below claim)
    }
}

// (64-bit: max_size + 1 must not wrap; the host clamps max_size to the cell count, which cuts every component the same way)
__device__ __forceinline__ int records_of(int size, int max_size, int min_size)
{
    const long long step = (long long)max_size + 1;
    const long long full = size / step, rem = size - full * step;
    return (int)((step > min_size ? full : 0) + (rem > min_size ? 1 : 0));
}

// one workgroup: queue bases and record bases in emission order; state: cells emitted, records.  After a refused seed nothing
// is emitted.
__global__ void fss_scan_emit_kernel(const FsSearchArgs a)
{
    __shared__ int s_wave[16];
    const bool err = a.state[FSS_ERROR] != 0;
    const int n_emit = err ? 0 : a.state[FSS_EMITTED];
    int carry_c = 0, carry_r = 0;
    for (int k0 = 0; k0 < n_emit; k0 += blockDim.x) {
        const int k = k0 + threadIdx.x;
        const int size = k < n_emit ? a.csize[a.emit_comp[k]] : 0;
        int tc, tr;
        const int oc = block_exclusive_scan(size, s_wave, &tc);
        const int orr = block_exclusive_scan(k < n_emit ? records_of(size, a.max_size, a.min_size) : 0, s_wave, &tr);
        if (k < n_emit) { a.emit_base[k] = carry_c + oc; a.rec_base[k] = carry_r + orr; }
        carry_c += tc;
        carry_r += tr;
    }
    if (threadIdx.x == 0) {
        a.state[FSS_EMITTED] = n_emit;
        a.state[FSS_CELLS] = carry_c;
        a.state[FSS_RECORDS] = carry_r;
    }
}

// one workgroup per emission at a time: the level-synchronous breadth-first walk (queue positions relative to the emission's base)
__global__ void __launch_bounds__(BFS_THREADS) fss_bfs_kernel(const FsSearchArgs a)
{
    __shared__ int s_wave[16];
    const int n_emit = a.state[FSS_EMITTED];
    for (int k = blockIdx.x; k < n_emit; k += gridDim.x) {
        const int c = a.emit_comp[k], seed = a.emit_seed[k], base = a.emit_base[k];
        const int size = a.csize[c], root = a.comp_root[c];
        int32_t *q = a.q + base;
        if (threadIdx.x == 0) { q[0] = seed; a.pos[seed] = 0; }
        __syncthreads();
        int lo = 0, hi = 1, levels = 1;
        for (int iter = 0; iter < size && lo < hi; ++iter) {
            // every unvisited component neighbour of the level goes to its first claimant in (queue position, slot) order
            for (int t = lo + (int)threadIdx.x; t < hi; t += blockDim.x) {
                const int p = q[t];
                for (int j = 0; j < 8; ++j) {
                    const int m = nb8(p, j, a.nx, a.ny);
                    if (m >= 0 && a.parent_f[m] == root && ld_agent(&a.pos[m]) < 0) atomicMin(&a.key[m], t * 8 + j);
                }
            }
            __syncthreads();
            // the won slots, counted per parent in slot order and scanned over the parents in queue order
            int carry = 0;
            for (int t0 = lo; t0 < hi; t0 += blockDim.x) {
                const int t = t0 + (int)threadIdx.x;
                int won = 0, cnt = 0, p = -1;
                if (t < hi) {
                    p = q[t];
                    for (int j = 0; j < 8; ++j) {
                        const int m = nb8(p, j, a.nx, a.ny);
                        if (m >= 0 && a.parent_f[m] == root && ld_agent(&a.pos[m]) < 0 && ld_agent(&a.key[m]) == t * 8 + j) { won |= 1 << j; ++cnt; }
                    }
                }
                int total;
                const int off = block_exclusive_scan(cnt, s_wave, &total);
                int w = hi + carry + off;
                for (int j = 0; j < 8; ++j) {
                    if (!((won >> j) & 1)) continue;
                    const int m = nb8(p, j, a.nx, a.ny);
                    if (w < size) { q[w] = m; a.pos[m] = w; }
                    ++w;
                }
                carry += total;
            }
            __syncthreads();
            lo = hi;
            hi = min(hi + carry, size);
            if (lo < hi) ++levels;
        }
        if (threadIdx.x == 0) atomicMax(&a.state[FSS_LEVELS], levels);
        __syncthreads();
    }
}

// one lane per record: the piece's cells, getCentroidOfCells, the angles and the restated std::sort, the middle element
__global__ void fss_pieces_kernel(const FsSearchArgs a)
{
    const int n_rec = a.state[FSS_RECORDS], n_emit = a.state[FSS_EMITTED];
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < n_rec; r += gridDim.x * blockDim.x) {
        int lo = 0, hi = n_emit;                                      // the last emission whose first record is <= r
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (a.rec_base[mid] <= r) lo = mid; else hi = mid;
        }
        const int k = lo, c = a.emit_comp[k];
        const int size = a.csize[c];
        const long long step = (long long)a.max_size + 1;
        const int start = (int)((long long)(r - a.rec_base[k]) * step);    // < size: r indexes a record of emission k
        const int sz = (int)min(step, (long long)(size - start));
        const int32_t *q = a.q + a.emit_base[k] + start;
        fs_msort_elem *e = a.sortbuf + a.emit_base[k] + start;
        // FrontierSearch.hpp:84-127 (mapToWorld of each cell, sums in queue order)
        double sx = 0, sy = 0;
        for (int t = 0; t < sz; ++t) {
            const int i = q[t], y = i / a.nx, x = i - y * a.nx;
            sx += a.ox + ((unsigned)x + 0.5) * a.res;
            sy += a.oy + ((unsigned)y + 0.5) * a.res;
        }
        double cx = sx / (double)sz, cy = sy / (double)sz;
        bool off = false;
        double vx = 0, vy = 0;
        for (int t = 0; t < sz; ++t) {
            const int i = q[t], y = i / a.nx, x = i - y * a.nx;
            const double dx = (a.ox + ((unsigned)x + 0.5) * a.res) - cx, dy = (a.oy + ((unsigned)y + 0.5) * a.res) - cy;
            if (sqrt(dx * dx + dy * dy) < a.res * 3) off = true;     // (pow(d, 2) is d * d)
            vx += fabs(dx);
            vy += fabs(dy);
        }
        const double offset = a.res * 1.414 * 2;
        if (vx > vy && off) cy -= offset;
        if (vx < vy && off) cx -= offset;
        for (int t = 0; t < sz; ++t) {
            const int i = q[t], y = i / a.nx, x = i - y * a.nx;
            e[t].angle = fs_msort_angle((a.oy + ((unsigned)y + 0.5) * a.res) - cy, (a.ox + ((unsigned)x + 0.5) * a.res) - cx);
            e[t].cell = i;
        }
        if (fs_msort_sort(e, sz)) atomicAdd(&a.state[FSS_GUARDED], 1);
        const int g = e[sz / 2].cell, gy = g / a.nx, gx = g - gy * a.nx;
        fs_frontier_record out;
        out.goal_x = a.ox + ((unsigned)gx + 0.5) * a.res;
        out.goal_y = a.oy + ((unsigned)gy + 0.5) * a.res;
        out.size = sz;
        out.label = a.comp_root[c];
        out.goal_cell = g;
        out.seed_cell = a.emit_seed[k];
        a.rec[r] = out;
        if (a.goal_xyz) { a.goal_xyz[3 * r] = out.goal_x; a.goal_xyz[3 * r + 1] = out.goal_y; a.goal_xyz[3 * r + 2] = 0.0; }
        if (a.fsize) a.fsize[r] = sz;
    }
}

// every_frontier_list: the world coordinates of every collected cell in emission order
__global__ void fss_every_kernel(const FsSearchArgs a)
{
    const int n = a.state[FSS_CELLS];
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) {
        const int i = a.q[t], y = i / a.nx, x = i - y * a.nx;
        a.every[2 * t] = a.ox + ((unsigned)x + 0.5) * a.res;
        a.every[2 * t + 1] = a.oy + ((unsigned)y + 0.5) * a.res;
    }
}

// FrontierGoalPointEquality against the caller's blacklist: the goal point equals a listed point bit for bit (the key of
// frontier_blacklist_); one lane per record
__global__ void fss_blacklist_kernel(const FsSearchArgs a, const double *black_xy, int32_t n_black, uint8_t *blacklisted)
{
    const int n_rec = a.state[FSS_RECORDS];
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < n_rec; r += gridDim.x * blockDim.x) {
        const double gx = a.rec[r].goal_x, gy = a.rec[r].goal_y;
        uint8_t hit = 0;
        for (int b = 0; b < n_black && !hit; ++b) hit = black_xy[2 * b] == gx && black_xy[2 * b + 1] == gy;
        blacklisted[r] = hit;
    }
}

// the grid planner's goal cells of n goal points (nav_world_to_map of fs_capi.hip, on the device); -1: off the map or the robot is
__global__ void fss_goal_cells_kernel(const double *goal_xyz, int32_t n, int32_t nx, int32_t ny, double ox, double oy, double res,
                                      int32_t robot_on, int32_t *cell)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const double wx = goal_xyz[3 * i], wy = goal_xyz[3 * i + 1];
        int32_t out = -1;
        if (robot_on && !(wx < ox || wy < oy)) {
            const double qx = (wx - ox) / res, qy = (wy - oy) / res;
            if (qx < 4294967296.0 && qy < 4294967296.0) {
                const unsigned ux = (unsigned)qx, uy = (unsigned)qy;
                if (ux < (unsigned)nx && uy < (unsigned)ny) out = (int32_t)(uy * (unsigned)nx + ux);
            }
        }
        cell[i] = out;
    }
}

}  // namespace

hipError_t fs_launch_search_blacklist(const FsSearchArgs &a, const double *d_black_xy, int32_t n_black, uint8_t *d_blacklisted, hipStream_t s)
{
    hipLaunchKernelGGL(fss_blacklist_kernel, dim3(64), dim3(256), 0, s, a, d_black_xy, n_black, d_blacklisted);
    return hipGetLastError();
}

hipError_t fs_launch_goal_cells(const double *d_goal_xyz, int32_t n, int32_t nx, int32_t ny, double ox, double oy, double res, int32_t robot_on,
                                int32_t *d_cell, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(fss_goal_cells_kernel, dim3((n + 255) / 256), dim3(256), 0, s, d_goal_xyz, n, nx, ny, ox, oy, res, robot_on, d_cell);
    return hipGetLastError();
}

hipError_t fs_launch_frontier_search(const FsSearchArgs &a, hipStream_t s)
{
    const int n = a.nx * a.ny;
    const int nb = (n + SCAN_THREADS - 1) / SCAN_THREADS;
    const dim3 cells_grid(nb), scan_block(SCAN_THREADS);
    hipLaunchKernelGGL(fss_count_kernel, cells_grid, scan_block, 0, s, a);
    hipLaunchKernelGGL(fss_scan_blocks_kernel, dim3(1), scan_block, 0, s, a, nb);
    hipLaunchKernelGGL(fss_scatter_kernel, cells_grid, scan_block, 0, s, a);
    hipLaunchKernelGGL(fss_member_kernel, cells_grid, scan_block, 0, s, a);
    if (a.outer) {
        hipLaunchKernelGGL(fss_outer_kernel, dim3(1), dim3(OUTER_THREADS), 0, s, a);
    } else {
        if (a.n_seeds < 0) hipLaunchKernelGGL(fss_nearest_kernel, cells_grid, scan_block, 0, s, a);
        hipLaunchKernelGGL(fss_emit_kernel, dim3(64), dim3(256), 0, s, a);
    }
    hipLaunchKernelGGL(fss_scan_emit_kernel, dim3(1), scan_block, 0, s, a);
    hipLaunchKernelGGL(fss_bfs_kernel, dim3(1024), dim3(BFS_THREADS), 0, s, a);
    hipLaunchKernelGGL(fss_pieces_kernel, dim3(256), dim3(64), 0, s, a);
    if (a.every) hipLaunchKernelGGL(fss_every_kernel, dim3(256), dim3(256), 0, s, a);
    return hipGetLastError();
}
