// csrc/kernels_reveal.hip -- the launcher of the reveal region's kernel and its argument checks.  The kernel itself, k_reveal_trace, lives in kernels_reveal.cuh, which
// only this file compiles for the device (the host emulators of tests/ include it too).
#include "hip_util.hpp"
#include "kernels_reveal.cuh"

namespace zk {
namespace gpu {

// what the entry checks before any lane runs: the reveal flag and the message length against the key's, the mask inside the header stride, the region inside the trace
// stride, and 16-byte alignment of the region and of every trace
void reveal_trace(uint8_t *trace, size_t stride, size_t reveal_off, const uint8_t *msgs, const uint8_t *hdrs, size_t hdr_stride, size_t mask_off, uint32_t nproofs, size_t msg_len, int reveal,
                  size_t key_msg_len, stream_t s) {
    if (!trace || !msgs || !hdrs) throw GpuError("reveal_trace: no trace, message or header buffer");
    if (reveal != 1) throw GpuError("reveal_trace: the key has no reveal region (R must be 1)");
    if (msg_len == 0 || msg_len > ((size_t)1 << 24)) throw GpuError("reveal_trace: the message must have 1 .. 2^24 bytes");
    if (msg_len != key_msg_len) throw GpuError("reveal_trace: the message length " + std::to_string(msg_len) + " is not the key's (" + std::to_string(key_msg_len) + ")");
    const size_t mb = TRV_MASK_BYTES(msg_len), need = TRV_REGION_BYTES(msg_len), nlanes = (msg_len + 15) / 16;
    if (mask_off > hdr_stride || hdr_stride - mask_off < mb) throw GpuError("reveal_trace: the header stride does not hold the " + std::to_string(mb) + " mask bytes");
    if (reveal_off > stride || stride - reveal_off < need)
        throw GpuError("reveal_trace: trace stride " + std::to_string(stride) + " does not hold a reveal region of " + std::to_string(need) + " bytes at offset " + std::to_string(reveal_off));
    if (reveal_off % 16 || stride % 16 || (uintptr_t)trace % 16) throw GpuError("reveal_trace: traces with a reveal region and the region's offset must be 16-byte aligned");
    if (nproofs == 0 || nproofs > (1u << 20) || (uint64_t)nproofs * nlanes > 0xffffffffull) throw GpuError("reveal_trace: 1 .. 2^20 proofs per launch");
    launch_lanes(k_reveal_trace, nproofs * (uint32_t)nlanes, s, trace, stride, reveal_off, msgs, hdrs, hdr_stride, mask_off, nproofs, (uint32_t)nlanes, (uint32_t)msg_len);
}

}  // namespace gpu
}  // namespace zk
