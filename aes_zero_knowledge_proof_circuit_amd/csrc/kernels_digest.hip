// csrc/kernels_digest.hip -- the launchers of the digest region's kernels and their argument checks.  The kernels themselves, k_sha256_trace, k_sha256_trace_seg and k_commit_trace, live in
// kernels_digest.cuh, which only this file compiles for the device (the host emulators of tests/ include it too).
#include "hip_util.hpp"
#include "kernels_digest.cuh"

namespace zk {
namespace gpu {

// what the entry checks before any lane runs: the digest kind, the prefix, the message length against the kind, the slots inside the stride, and 16-byte alignment of the
// region and of every trace
void sha256_trace(uint8_t *trace, size_t stride, size_t digest_off, const uint8_t *msgs, const uint8_t *hdrs, size_t hdr_stride, size_t hin_off, uint32_t nproofs, size_t msg_len, int digest_kind,
                  uint64_t digest_prefix, stream_t s) {
    if (!trace || !msgs || !hdrs) throw GpuError("sha256_trace: no trace, message or header buffer");
    if (digest_kind != 1 && digest_kind != 2) throw GpuError("sha256_trace: the digest kind must be 1 (chain) or 2 (final)");
    if (msg_len == 0 || msg_len > ((size_t)1 << 31)) throw GpuError("sha256_trace: the message must have 1 .. 2^31 bytes");
    if (digest_kind == 1 && (msg_len % 64 || digest_prefix)) throw GpuError("sha256_trace: a chain key takes a multiple of 64 bytes and no prefix");
    if (digest_prefix % 64 || digest_prefix >= ((uint64_t)1 << 61) - msg_len) throw GpuError("sha256_trace: the prefix must be a multiple of 64 with prefix + length below 2^61");
    if (hin_off > hdr_stride || hdr_stride - hin_off < 32) throw GpuError("sha256_trace: the header stride does not hold H_in");
    const size_t nblk = TRD_BLOCKS(digest_kind, msg_len), need = TRD_SLOT0 + nblk * TRD_SLOT_STRIDE;
    if (digest_off > stride || stride - digest_off < need)
        throw GpuError("sha256_trace: trace stride " + std::to_string(stride) + " does not hold " + std::to_string(nblk) + " digest slots of " + std::to_string((size_t)TRD_SLOT_STRIDE) + " bytes at offset " + std::to_string(digest_off));
    if (digest_off % 16 || stride % 16 || (uintptr_t)trace % 16) throw GpuError("sha256_trace: traces with a digest and the digest offset must be 16-byte aligned");
    if (nproofs == 0 || nproofs > (1u << 20) || (uint64_t)nproofs * nblk > 0xffffffffull) throw GpuError("sha256_trace: 1 .. 2^20 proofs per launch");
    launch_lanes(k_sha256_trace, nproofs * (uint32_t)nblk, s, trace, stride, digest_off, msgs, hdrs, hdr_stride, hin_off, nproofs, (uint32_t)nblk, (uint32_t)msg_len, (uint32_t)digest_kind,
                 8 * (digest_prefix + (uint64_t)msg_len));
}

// the segment digest entry checks before any lane runs: the role, the digest kind against the role, the message length against the kind, the header stride
// against H_in and (last) total_bits, the slots -- and a last's 16 length bytes behind them -- inside the trace stride, and 16-byte alignment
void sha256_trace_seg(uint8_t *trace, size_t stride, size_t digest_off, const uint8_t *msgs, const uint8_t *hdrs, size_t hdr_stride, uint32_t nproofs, int role, size_t msg_len, size_t aad_len,
                      int digest_kind, stream_t s) {
    if (!trace || !msgs || !hdrs) throw GpuError("sha256_trace_seg: no trace, message or header buffer");
    if (role != TRS_HEAD && role != TRS_MID && role != TRS_LAST) throw GpuError("sha256_trace_seg: the role must be 0 (head), 1 (mid) or 3 (last): the closing tail has no digest");
    if (digest_kind != TRS_DG_KIND(role)) throw GpuError("sha256_trace_seg: a head or mid has a chain digest (kind 1), a last a final one (kind 2)");
    if (msg_len == 0 || msg_len > ((size_t)1 << 16) || aad_len > ((size_t)1 << 16)) throw GpuError("sha256_trace_seg: the message must have 1 .. 65536 bytes, the aad at most 65536");
    if (digest_kind == 1 && msg_len % 64) throw GpuError("sha256_trace_seg: a chain digest takes a multiple of 64 bytes");
    if (role != TRS_HEAD && aad_len) throw GpuError("sha256_trace_seg: only a head segment takes aad");
    if (hdr_stride < TRS_HDR_DG_BYTES(aad_len, digest_kind)) throw GpuError("sha256_trace_seg: the header stride does not hold H_in" + std::string(digest_kind == 2 ? " and total_bits" : ""));
    const size_t nblk = TRD_BLOCKS(digest_kind, msg_len), need = TRS_DG_BITS(nblk) + (digest_kind == 2 ? 16 : 0);
    if (digest_off > stride || stride - digest_off < need)
        throw GpuError("sha256_trace_seg: trace stride " + std::to_string(stride) + " does not hold a digest region of " + std::to_string(need) + " bytes at offset " + std::to_string(digest_off));
    if (digest_off % 16 || stride % 16 || (uintptr_t)trace % 16) throw GpuError("sha256_trace_seg: traces with a digest and the digest offset must be 16-byte aligned");
    if (nproofs == 0 || nproofs > (1u << 20)) throw GpuError("sha256_trace_seg: 1 .. 2^20 proofs per launch");
    launch_lanes(k_sha256_trace_seg, nproofs * (uint32_t)nblk, s, trace, stride, digest_off, msgs, hdrs, hdr_stride, (uint32_t)aad_len, nproofs, (uint32_t)nblk, (uint32_t)msg_len, (uint32_t)digest_kind);
}

// the commitment entry's checks ahead of the launch: the role, the key size, the segment region and Y_out inside the stride, the header stride, 16-byte alignment
void commit_trace(uint8_t *trace, size_t stride, size_t seg_off, size_t yout_off, const uint8_t *keys, size_t key_bytes, const uint8_t *hdrs, size_t hdr_stride, uint32_t nproofs, int role,
                  uint32_t nblocks, stream_t s) {
    if (!trace || !keys || !hdrs) throw GpuError("commit_trace: no trace, key or header buffer");
    if (role != TRS_HEAD && role != TRS_MID && role != TRS_TAIL && role != TRS_LAST) throw GpuError("commit_trace: the role must be 0 (head), 1 (mid), 2 (tail) or 3 (last)");
    if (key_bytes != 16 && key_bytes != 24 && key_bytes != 32) throw GpuError("commit_trace: the AES key must have 16, 24 or 32 bytes");
    if ((nblocks == 0 && role != TRS_TAIL) || nblocks > (1u << 12)) throw GpuError("commit_trace: 1 .. 4096 data blocks per segment (0 for the closing tail of a digest record)");
    if (hdr_stride < TRS_HDR_BYTES(0)) throw GpuError("commit_trace: the header stride does not hold Y_in and the salts");
    const size_t need = TRS_SEG_BYTES((size_t)nblocks);
    if (seg_off > stride || stride - seg_off < need || yout_off > seg_off || seg_off - yout_off < 16)
        throw GpuError("commit_trace: trace stride " + std::to_string(stride) + " does not hold a segment region of " + std::to_string(need) + " bytes at offset " + std::to_string(seg_off));
    if (seg_off % 16 || stride % 16 || (uintptr_t)trace % 16) throw GpuError("commit_trace: segment traces and the region's offset must be 16-byte aligned");
    if (nproofs == 0 || nproofs > (1u << 20)) throw GpuError("commit_trace: 1 .. 2^20 proofs per launch");
    launch_lanes(k_commit_trace, nproofs * ((role == TRS_MID || role == TRS_LAST) ? 2u : 1u), s, trace, stride, seg_off, yout_off, keys, (uint32_t)key_bytes, hdrs, hdr_stride, nproofs, (uint32_t)role, nblocks);
}

}  // namespace gpu
}  // namespace zk
