// The library's own exception types: thrown by the host scene preparation and by the device driver alike, mapped to rrt error codes in device/rrt_api.hip.
#pragma once
#include <stdexcept>

namespace rrtd {
struct DeviceError : std::runtime_error { using std::runtime_error::runtime_error; };
struct UnsupportedError : std::runtime_error { using std::runtime_error::runtime_error; };
struct PanicError : std::runtime_error { using std::runtime_error::runtime_error; };
}  // namespace rrtd
