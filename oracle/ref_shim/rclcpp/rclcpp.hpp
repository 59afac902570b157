// Stand-in for rclcpp/rclcpp.hpp when the reference's planners are compiled for oracle/_ref/ (oracle/ref_build.py): logging only,
// and every message is dropped without evaluating its arguments.
#pragma once
namespace rclcpp { struct Logger {}; inline Logger get_logger(const char *) { return Logger{}; } }
#define RCLCPP_DEBUG(...) ((void)0)
#define RCLCPP_INFO(...) ((void)0)
#define RCLCPP_WARN(...) ((void)0)
#define RCLCPP_ERROR(...) ((void)0)
