// The host side of fit-slam_amd/csrc/fs_keepout.h behind a C interface, for tests/test_keepout_restatement.py: the rays of one
// zone on one map geometry and the indices their walks visit, as the library computes them (fs_capi.hip: ko_zone_rays; the kernel
// walks with the same fs_ko_walk).  Built as a shared object; with -DKEEPOUT_HOST_MAIN as a stand-alone program that runs the
// hand-checkable anchor (the form a sanitizer pass over this host code uses).
#include "fs_keepout.h"

#include <cstdio>
#include <set>
#include <vector>

extern "C" {

// rays [FS_KO_MAX_RAYS][4] of the zone; returns their number (0: apex off the map), -1: the size cannot be converted
int kohost_zone_rays(int kind, double wx, double wy, double yaw, double size_m, int nx, int ny, double ox, double oy, double res, int32_t *rays)
{
    int32_t ax = 0, ay = 0;
    uint32_t size_cells = 0;
    if (!fs_ko_size_in_cells(size_m, res, &size_cells)) return -1;
    if (!fs_ko_world_to_map(wx, wy, ox, oy, res, nx, ny, &ax, &ay)) return 0;
    fs_ko_ray *out = reinterpret_cast<fs_ko_ray *>(rays);
    return kind == FS_KO_FOV ? fs_ko_fov_rays(ax, ay, size_cells, yaw, nx, ny, out) : fs_ko_disc_rays(ax, ay, size_cells, nx, ny, out);
}

// the indices y * nx + x the walks of n_rays rays visit, in order, duplicates included; returns their number (at most `room`
// are stored)
long long kohost_walk(const int32_t *rays, int n_rays, int nx, long long *indices, long long room)
{
    long long n = 0;
    for (int r = 0; r < n_rays; ++r) {
        const fs_ko_ray ray{rays[4 * r], rays[4 * r + 1], rays[4 * r + 2], rays[4 * r + 3]};
        fs_ko_walk(ray, [&](int32_t x, int32_t y) {
            if (n < room) indices[n] = (long long)y * nx + x;
            ++n;
        });
    }
    return n;
}

}  // extern "C"

#ifdef KEEPOUT_HOST_MAIN
int main()
{
    // 96 x 96, origin (0, 0), resolution 0.05; apex world (0.52, 2.42), yaw 0, height 3.5 m
    std::vector<int32_t> rays(4 * FS_KO_MAX_RAYS);
    const int n = kohost_zone_rays(FS_KO_FOV, 0.52, 2.42, 0.0, 3.5, 96, 96, 0.0, 0.0, 0.05, rays.data());
    std::vector<long long> idx(1 << 16);
    const long long pushed = kohost_walk(rays.data(), n, 96, idx.data(), (long long)idx.size());
    const std::set<long long> distinct(idx.begin(), idx.begin() + pushed);
    std::printf("%d rays, apex (%d, %d), first end (%d, %d), last end (%d, %d), %lld pushed, %zu distinct\n", n, rays[0], rays[1], rays[2], rays[3],
                rays[4 * (n - 1) + 2], rays[4 * (n - 1) + 3], pushed, distinct.size());
    // a disc of 1.7 m at the border, and a fan on a 16 x 16 map where every end clamps
    const int nd = kohost_zone_rays(FS_KO_DISC, 0.1, 4.7, 0.0, 1.7, 96, 96, 0.0, 0.0, 0.05, rays.data());
    const long long pd = kohost_walk(rays.data(), nd, 96, idx.data(), (long long)idx.size());
    const int nc = kohost_zone_rays(FS_KO_FOV, 0.4, 0.4, 2.3, 3.5, 16, 16, 0.0, 0.0, 0.05, rays.data());
    const long long pc = kohost_walk(rays.data(), nc, 16, idx.data(), (long long)idx.size());
    std::printf("disc: %d rays, %lld pushed; clamped fan: %d rays, %lld pushed\n", nd, pd, nc, pc);
    return (n == 20 && pushed == 1420 && nd == 360 && nc == 20 && pd > 0 && pc > 0) ? 0 : 1;
}
#endif
