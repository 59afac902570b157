// fs_drive.hip — robots drive station lists through the ground-truth world, sensing at every station (fs_drive).
//
// This project's own extension, like fs_sense.hip: the reference's robot is driven by its controller server and its map comes
// from the depth camera, both outside the vendored tree.  What a drive is made of is the reference's: the move is getTracedCells'
// walk with isConnectable's visitor (DEP/src/planners/FrontierRoadmap.cpp:716-737, the 253..254 range), the sweep is the arrival
// fan of fs_sense.hip, the goal test is surroundingCellsMapped, which CheckIfGoalMapped asks while the robot drives.
//
// The host enqueues, for every step k = 0 .. K - 1 and without waiting in between,
//   step   — one wavefront per robot.  A robot that has stopped returns at once.  One that has no station k has ARRIVED.  From
//            k = 1 on the segment station k - 1 -> k is walked, every lane of the wave the same walk (the loads are one address per
//            wave): an end off the map stops the robot OFF_MAP, a staged cost in the block range BLOCKED, else a world cost in the
//            block range COLLIDED.  Otherwise the robot is at station k and sweeps from there: sense_fan (fs_sense_dev.h), marks
//            into the mark image, the station's status and count, the seen cells' box for the merge.
//   merge  — blockIdx.y = robot, over the robot's box of this step, x fastest: where the mark is set, staged = world, the cell is
//            counted and the mark is cleared.  Boxes of two robots may overlap; a marked cell is handled by the lowest robot whose
//            box of this step holds it and by nobody else, so every seen cell is counted once whoever saw it.
//   goal   — one lane per robot: a robot still driving whose goal is mapped now has stopped, MAPPED.
// Every launch ends on its own: nothing spins, nothing waits for another wave.  The stop state lives in state [R][2].  Every
// figure is an integer sum, minimum or maximum: nothing depends on the order of the robots or of the device's work.
#include "fs_internal.h"
#include "fs_walk.h"
#include "fs_sense_dev.h"

#define FS_DRIVE_WAVES 4        // robots per workgroup of the step kernel

namespace {

__global__ __launch_bounds__(FS_DRIVE_WAVES * 64)
void fs_drive_step_kernel(const FsDriveArgs a)
{
    const int lane = threadIdx.x & 63;
    const int r = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * FS_DRIVE_WAVES + (threadIdx.x >> 6)));
    if (r >= a.n_robots) return;
    if (a.state[2 * r] != FS_DRIVE_DRIVING) return;
    const int k = a.step;
    if (k >= a.n_stations[r]) {
        if (lane == 0) a.state[2 * r] = FS_DRIVE_ARRIVED;
        return;
    }
    const size_t at = (size_t)a.station_off[r] + (size_t)k;
    const double sx = a.sense.origin[3 * at], sy = a.sense.origin[3 * at + 1], sz = a.sense.origin[3 * at + 2];
    if (k >= 1) {
        // the move, as fs_trace_segments walks it (segment_walk, fs_raymarch.hip): the end point's worldToMap first
        const double px = a.sense.origin[3 * at - 3], py = a.sense.origin[3 * at - 2], pz = a.sense.origin[3 * at - 1];
        uint32_t x0, y0, z0, x1, y1, z1;
        int stop = FS_DRIVE_DRIVING;
        if (world_to_map(a.staged, sx, sy, sz, x1, y1, z1) && world_to_map(a.staged, px, py, pz, x0, y0, z0)) {
            WalkLinear w;
            walk_init(w, a.staged, x0, y0, z0, x1, y1, z1, a.move_max_length);
            bool hit_staged = false, hit_world = false;
            for (uint32_t v = 0; v <= w.end; ++v) {
                const int cs = walk_cell(a.staged, w);
#ifdef FS_RAY_BOUNDS
                if (cs == 256) break;
#endif
                const int cw = (int)a.sense.world.cells[w.offset];
                hit_staged = hit_staged || (cs >= a.block_min && cs <= a.block_max);
                hit_world = hit_world || (cw >= a.block_min && cw <= a.block_max);
                walk_step(w);
            }
            if (hit_staged) stop = FS_DRIVE_BLOCKED;
            else if (hit_world) stop = FS_DRIVE_COLLIDED;
        } else {
            stop = FS_DRIVE_OFF_MAP;
        }
        if (stop != FS_DRIVE_DRIVING) {
            if (lane == 0) a.state[2 * r] = stop;
            return;
        }
        if (lane == 0) a.state[2 * r + 1] = k;
    }
    const int first = a.sense.first_ray ? a.sense.first_ray[at] : -1;
    const SenseFan f = sense_fan(a.sense, lane, sx, sy, sz, first, nullptr);
    if (lane != 0) return;
    if (!f.ok) { a.sense.status[at] = FS_STATUS_OFF_MAP; return; }             // (seen_unknown and the box keep their presets: 0, empty)
    a.sense.seen_unknown[at] = f.total;
    a.sense.status[at] = FS_STATUS_OK;
    int32_t *box = a.station_box + 4 * at;
    box[0] = (int)f.bx0; box[1] = (int)f.by0; box[2] = (int)f.bx1; box[3] = (int)f.by1;
    atomicMin(a.union_box + 0, (int)f.bx0); atomicMin(a.union_box + 1, (int)f.by0);
    atomicMax(a.union_box + 2, (int)f.bx1); atomicMax(a.union_box + 3, (int)f.by1);
}

__global__ __launch_bounds__(256)
void fs_drive_merge_kernel(const FsDriveArgs a)
{
    const int r = (int)blockIdx.y, k = a.step;
    if (k >= a.n_stations[r]) return;                                          // (uniform over the block, as every return here)
    const int32_t *box = a.station_box + 4 * ((size_t)a.station_off[r] + (size_t)k);
    const int x0 = box[0], y0 = box[1], x1 = box[2], y1 = box[3];
    if (x1 < x0 || y1 < y0) return;                                            // the robot did not sweep in this step
    // (the step kernel's boxes come from cells it visited; a box that leaves the grid all the same touches nothing)
    if (x0 < 0 || y0 < 0 || x1 >= a.staged.nx || y1 >= a.staged.ny) return;
    const uint8_t *__restrict__ world = a.sense.world.cells;
    uint8_t *staged = const_cast<uint8_t *>(a.sense.staged), *mark = a.sense.mark;
    const unsigned sx = (unsigned)(x1 - x0 + 1), sy = (unsigned)(y1 - y0 + 1);
    const unsigned cells = sx * sy, stride = gridDim.x * 256u;
    unsigned long long v[2] = {0ull, 0ull};
    for (unsigned t = blockIdx.x * 256u + threadIdx.x; t < cells; t += stride) {
        const unsigned row = t / sx;
        const int x = x0 + (int)(t - row * sx), y = y0 + (int)row;
        const size_t at = (size_t)y * (size_t)a.staged.nx + (size_t)x;
        if (!mark[at]) continue;
        bool mine = true;                                                      // no robot before r holds the cell in its box
        for (int q = 0; q < r && mine; ++q) {
            if (k >= a.n_stations[q]) continue;
            const int32_t *b = a.station_box + 4 * ((size_t)a.station_off[q] + (size_t)k);
            if (x >= b[0] && x <= b[2] && y >= b[1] && y <= b[3]) mine = false;
        }
        if (!mine) continue;
        const uint8_t w = world[at], s = staged[at];
        staged[at] = w;
        mark[at] = (uint8_t)0;
        v[0] += 1ull;
        v[1] += (s == 255 && w != 255) ? 1ull : 0ull;
    }
    block_add<2>(v, a.counts);
}

__global__ void fs_drive_goal_kernel(const FsDriveArgs a)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.n_robots || a.state[2 * r] != FS_DRIVE_DRIVING) return;
    if (goal_mapped(a.sense.staged, a.staged.nx, a.staged.ny, a.staged.ox, a.staged.oy, a.staged.res, a.goal[3 * (size_t)r], a.goal[3 * (size_t)r + 1]))
        a.state[2 * r] = FS_DRIVE_MAPPED;
}

}  // namespace

hipError_t fs_launch_drive_step(const FsDriveArgs &a, hipStream_t s)
{
    if (a.n_robots <= 0) return hipSuccess;
    hipLaunchKernelGGL(fs_drive_step_kernel, dim3((unsigned)((a.n_robots + FS_DRIVE_WAVES - 1) / FS_DRIVE_WAVES)), dim3(FS_DRIVE_WAVES * 64), 0, s, a);
    return hipGetLastError();
}

hipError_t fs_launch_drive_merge(const FsDriveArgs &a, unsigned merge_blocks, hipStream_t s)
{
    if (a.n_robots <= 0 || merge_blocks == 0) return hipSuccess;
    if (a.n_robots > 65535) return hipErrorInvalidValue;                       // (gridDim.y; fs_drive's own cap is far below)
    hipLaunchKernelGGL(fs_drive_merge_kernel, dim3(merge_blocks < 1024u ? merge_blocks : 1024u, (unsigned)a.n_robots), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t fs_launch_drive_goal(const FsDriveArgs &a, hipStream_t s)
{
    if (a.n_robots <= 0) return hipSuccess;
    hipLaunchKernelGGL(fs_drive_goal_kernel, dim3((unsigned)((a.n_robots + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}
