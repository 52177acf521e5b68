// csrc/hip_util.hpp -- HIP error checking shared by the .hip translation units
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include "gpu.hpp"

#define HIP_CHECK(expr)                                                                                   \
    do {                                                                                                  \
        hipError_t _e = (expr);                                                                           \
        if (_e != hipSuccess)                                                                             \
            throw zk::gpu::GpuError(std::string("HIP error ") + hipGetErrorString(_e) + " at " __FILE__ ":" + std::to_string(__LINE__) + " (" #expr ")"); \
    } while (0)
#define HIP_LAUNCH_CHECK() HIP_CHECK(hipGetLastError())

namespace zk {
namespace gpu {
// the launch of the one-lane-per-item kernels (the witness trace): workgroups of one wave over `lanes` lanes, on stream s, and the launch check
template <typename Kernel, typename... Args>
inline void launch_lanes(Kernel kernel, uint32_t lanes, stream_t s, Args... args) {
    hipLaunchKernelGGL(kernel, dim3((lanes + 63) / 64), dim3(64), 0, (hipStream_t)s, args...);
    HIP_LAUNCH_CHECK();
}
}  // namespace gpu
}  // namespace zk
