// Stand-in for nav2_costmap_2d/costmap_2d_ros.hpp when the reference's Theta* is compiled for oracle/_ref/ (oracle/ref_build.py):
// a Costmap2D over a caller's row-major uint8 array with the members the planner calls.  worldToMap and mapToWorld follow nav2:
// a point below the origin is off the map, the cell is (w - origin) / resolution truncated, a cell at or beyond the size is off
// the map; a cell's world point is its centre.
#pragma once
#include <cfloat>
#include <cstddef>

namespace nav2_costmap_2d {

class Costmap2D {
public:
    Costmap2D(const unsigned char *cells, unsigned int size_x, unsigned int size_y, double resolution, double origin_x, double origin_y)
        : cells_(cells), size_x_(size_x), size_y_(size_y), resolution_(resolution), origin_x_(origin_x), origin_y_(origin_y) {}

    unsigned char getCost(unsigned int mx, unsigned int my) const { return cells_[(size_t)my * size_x_ + mx]; }
    unsigned int getSizeInCellsX() const { return size_x_; }
    unsigned int getSizeInCellsY() const { return size_y_; }
    double getResolution() const { return resolution_; }

    bool worldToMap(double wx, double wy, unsigned int &mx, unsigned int &my) const
    {
        if (wx < origin_x_ || wy < origin_y_) return false;
        mx = static_cast<unsigned int>((wx - origin_x_) / resolution_);
        my = static_cast<unsigned int>((wy - origin_y_) / resolution_);
        return mx < size_x_ && my < size_y_;
    }
    void mapToWorld(unsigned int mx, unsigned int my, double &wx, double &wy) const
    {
        wx = origin_x_ + (mx + 0.5) * resolution_;
        wy = origin_y_ + (my + 0.5) * resolution_;
    }

private:
    const unsigned char *cells_;
    unsigned int size_x_, size_y_;
    double resolution_, origin_x_, origin_y_;
};

}  // namespace nav2_costmap_2d
