// Stand-in for nav_msgs/msg/path.hpp (and the geometry_msgs types it carries) when the reference's Theta* is compiled for
// oracle/_ref/ (oracle/ref_build.py): plain structs with the fields the planner reads and writes.
#pragma once
#include <vector>

namespace geometry_msgs { namespace msg {
struct Point { double x = 0.0, y = 0.0, z = 0.0; };
struct Quaternion { double x = 0.0, y = 0.0, z = 0.0, w = 1.0; };
struct Pose { Point position; Quaternion orientation; };
struct PoseStamped { Pose pose; };
} }

namespace nav_msgs { namespace msg {
struct Path { std::vector<geometry_msgs::msg::PoseStamped> poses; };
} }
