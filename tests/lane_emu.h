// tests/lane_emu.h -- what lets the trace kernels' headers (csrc/kernels_witness.cuh, kernels_digest.cuh, kernels_reveal.cuh) compile on the host, one call per lane with
// blockIdx.x = the lane: faithful because the trace kernels use no LDS, no barrier, no cross-lane operation and no atomics.
#pragma once
#include <cstdint>
#define __global__
#define __device__
#define __forceinline__ inline
#define __restrict__
struct D3 { unsigned x; };
static D3 blockIdx, blockDim{1}, threadIdx{0};
struct alignas(16) uint4 { uint32_t x, y, z, w; };
static inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{x, y, z, w}; }
