// csrc/kernels_reveal.hip -- the reveal region of the trace (trace_layout.h TRV_*): a proof's public mask and the message bytes it opens.
//   k_reveal_trace   one lane per 16 message bytes, launched behind the mode's kernel(s), the key-tag kernel and the digest kernel on the same stream.
//                    nproofs * ceil(L / 16) lanes; lane (p, b) reads the message bytes 16 b .. min(16 b + 16, L) - 1 from the proof's message buffer -- never one at or
//                    beyond L -- and its two mask bytes 2 b, 2 b + 1 (those below ceil(L / 8)) from the proof's public header, stores revealed[16 b .. 16 b + 15] =
//                    mask_i ? M[i] : 0 with ONE 16-byte store and its two mask bytes with one 2-byte store.
// Zero padding: a proof's last lane stores zeros behind L inside its 16-byte store, which ends the revealed sub-region (16 ceil(L / 16) bytes), and the zeros of the mask
// sub-region from byte 2 ceil(L / 16) to its end.  Every byte of the region has exactly one writer and no byte ahead of it is touched; no LDS, no barrier, no
// cross-lane operation.  The kernel is handed the message and the mask only, never a `revealed` made on the host: the host's masking (the verifier's) and the device's
// (the witness) meet in the constraints.  A mask bit at or beyond L is stored as it came: the row that pins it to zero is then unsatisfied and the proof does not verify.
#include "hip_util.hpp"
#include "trace_layout.h"

namespace zk {
namespace gpu {

// hdrs: nproofs x hdr_stride bytes, the proofs' public headers; a proof's mask is the ceil(msg_len / 8) bytes at mask_off of its header.  msgs: nproofs x msg_len bytes,
// packed.  rv_off: the reveal region's offset in a trace (16-byte aligned, as are the traces)
__global__ void k_reveal_trace(uint8_t *__restrict__ trace, size_t stride, size_t rv_off, const uint8_t *__restrict__ msgs, const uint8_t *__restrict__ hdrs, size_t hdr_stride, size_t mask_off,
                               uint32_t nproofs, uint32_t nlanes, uint32_t msg_len) {
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nproofs * nlanes) return;
    const uint32_t p = t / nlanes, b = t % nlanes, mb = TRV_MASK_BYTES(msg_len);
    const uint8_t *msg = msgs + (size_t)p * msg_len, *mask = hdrs + (size_t)p * hdr_stride + mask_off;
    uint8_t *rv = trace + (size_t)p * stride + rv_off;
    uint32_t m = 0;
    if (2 * b < mb) m = mask[2 * b];
    if (2 * b + 1 < mb) m |= (uint32_t)mask[2 * b + 1] << 8;
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const uint32_t at = 16 * b + (uint32_t)i;
        uint32_t byte = 0;
        if (at < msg_len && ((m >> i) & 1)) byte = msg[at];
        w[i / 4] |= byte << (8 * (i % 4));
    }
    *reinterpret_cast<uint4 *>(rv + TRV_REVEALED(msg_len) + 16 * (size_t)b) = make_uint4(w[0], w[1], w[2], w[3]);
    *reinterpret_cast<uint16_t *>(rv + TRV_MASK + 2 * (size_t)b) = (uint16_t)m;
    if (b + 1 == nlanes)
        for (uint32_t q = 2 * nlanes; q < TRV_REVEALED(msg_len); q += 2) *reinterpret_cast<uint16_t *>(rv + TRV_MASK + q) = 0;
}

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
    const uint32_t lanes = nproofs * (uint32_t)nlanes;
    const dim3 grid((lanes + 63) / 64), block(64);
    hipLaunchKernelGGL(k_reveal_trace, grid, block, 0, (hipStream_t)s, trace, stride, reveal_off, msgs, hdrs, hdr_stride, mask_off, nproofs, (uint32_t)nlanes, (uint32_t)msg_len);
    HIP_LAUNCH_CHECK();
}

}  // namespace gpu
}  // namespace zk
