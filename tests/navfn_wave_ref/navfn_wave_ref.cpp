// navfn_wave_ref.cpp — host driver of fit-slam_amd/csrc/fs_navfn_wave.h, the one definition of the REFERENCE grid search's wave that
// the device compiles too.  Test infrastructure: built by its tests with `g++ -O2 -ffp-contract=off -shared -fPIC`
// and loaded through ctypes.  The costs come from the caller (planner_ref.costs: setCostmap + the border ring).
#include <stdint.h>
#include <string.h>

#include <vector>

#include "fs_navfn_wave.h"

extern "C" {

// One wave from the robot cell (rx, ry) that stops at the frontier cell (sx, sy), cur walked in chunks of `width` entries (1: the
// serial wave, 64: the device's chunks), priority buffers of `cap` cells.  pot [ny][nx] out.  out [4]: reached, limit bits, the
// running hash of every push, chunks cut short.  Returns 0, or -1 on bad arguments.
int nw_wave(const uint8_t *cost, int nx, int ny, int rx, int ry, int sx, int sy, int width, int cap, float *pot, int64_t *out)
{
    if (nx <= 0 || ny <= 0 || rx < 0 || ry < 0 || rx >= nx || ry >= ny || sx < 0 || sy < 0 || sx >= nx || sy >= ny) return -1;
    if (width < 1 || width > FS_NW_WIDTH || cap < 1 || cap > FS_NW_CAP) return -1;
    const size_t ns = (size_t)nx * ny;
    std::vector<uint8_t> pending(ns, 0);
    std::vector<int32_t> buf((size_t)3 * cap, 0);
    for (size_t k = 0; k < ns; ++k) pot[k] = FS_NW_POT_HIGH;
    uint64_t hash = 0xcbf29ce484222325ull;
    int64_t replays = 0;
    const fs_nw_map m{cost, nx, ny};
    fs_nw_wave w{};
    w.pot = pot; w.pending = pending.data();
    w.cur = buf.data(); w.next = w.cur + cap; w.over = w.next + cap;
    w.cap = cap; w.sx = sx; w.sy = sy; w.hash = &hash;
    const bool reached = fs_nw_run(m, w, rx, ry, width, &replays);
    out[0] = reached ? 1 : 0; out[1] = w.limit; out[2] = (int64_t)hash; out[3] = replays;
    return 0;
}

// the heuristic's float for every 0 <= dx, dy < side, [side][side]
void nw_heuristic_table(int side, float *out)
{
    for (int dy = 0; dy < side; ++dy)
        for (int dx = 0; dx < side; ++dx) out[(size_t)dy * side + dx] = fs_nw_heuristic(dx, dy);
}

// ... and the reference's expression with libm's hypot
void nw_hypot_table(int side, float *out)
{
    for (int dy = 0; dy < side; ++dy)
        for (int dx = 0; dx < side; ++dx) out[(size_t)dy * side + dx] = (float)(hypot((double)dx, (double)dy) * (double)(float)FS_NW_COST_NEUTRAL);
}

}  // extern "C"
