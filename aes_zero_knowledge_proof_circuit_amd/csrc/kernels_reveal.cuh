// csrc/kernels_reveal.cuh -- the device code of the reveal region of the trace (trace_layout.h TRV_*): a proof's public mask and the message bytes it opens.
//   k_reveal_trace   one lane per 16 message bytes, launched behind the mode's kernel(s), the key-tag kernel and the digest kernel on the same stream.
//                    nproofs * ceil(L / 16) lanes; lane (p, b) reads the message bytes 16 b .. min(16 b + 16, L) - 1 from the proof's message buffer -- never one at or
//                    beyond L -- and its two mask bytes 2 b, 2 b + 1 (those below ceil(L / 8)) from the proof's public header, stores revealed[16 b .. 16 b + 15] =
//                    mask_i ? M[i] : 0 with ONE 16-byte store and its two mask bytes with one 2-byte store.
// Zero padding: a proof's last lane stores zeros behind L inside its 16-byte store, which ends the revealed sub-region (16 ceil(L / 16) bytes), and the zeros of the mask
// sub-region from byte 2 ceil(L / 16) to its end.  Every byte of the region has exactly one writer and no byte ahead of it is touched; no LDS, no barrier, no
// cross-lane operation.  The kernel is handed the message and the mask only, never a `revealed` made on the host: the host's masking (the verifier's) and the device's
// (the witness) meet in the constraints.  A mask bit at or beyond L is stored as it came: the row that pins it to zero is then unsatisfied and the proof does not verify.
// Device code only, as kernels_witness.cuh: one translation unit of the library includes this file and holds the launcher, the host emulators include it behind
// tests/lane_emu.h.  uint4 / make_uint4 are the device runtime's there and lane_emu.h's on the host.
#pragma once
#include <cstddef>
#include <cstdint>
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

}  // namespace gpu
}  // namespace zk
