// csrc/kernels_digest.cuh -- the device code of the digest region of the trace (trace_layout.h TRD_*): SHA-256 over a proof's hidden message with every
// intermediate the circuit names.
//   k_sha256_trace   one lane per compression, launched behind the mode's kernel(s) and the key-tag kernel on the same stream.  nproofs * nblk lanes; lane (p, c) reads
//                    the proof's message bytes from the message buffer (for a final key it builds the padding 0x80, zeros, be64(8 (P + L)) itself), reads H_in from the
//                    proof's public header, re-walks compressions 0 .. c - 1 in registers without a store -- the way a CBC lane re-walks its chain -- then runs
//                    compression c and stores every word of its slot.  Lane c = 0 also stores H_in, the last lane H_out.  The kernel is handed message and H_in only, never
//                    a state made on the host: the host's hash and the device's meet in the constraints.
//   k_sha256_trace_seg   the digest region of a GCM segment of a digest record: k_sha256_trace's lanes, with H_in AND the padding's total_bits read per proof
//                    from the proof's segment header -- a launch may hold the last segments of records of different lengths.
//   k_commit_trace   the boundary commitments of a GCM segment: one lane per commitment, ONE compression from the initial value over key || zeros || Y ||
//                    salt through the same sha_compress, into the segment region's slots.
// Every byte of the region has exactly one writer and no byte ahead of it is touched; no LDS, no barrier, no cross-lane operation.  The 16-word schedule ring and the
// eight state words live in registers: the 64 rounds are fully unrolled, so every index into the ring is a constant.
// Device code only, as kernels_witness.cuh: one translation unit of the library includes this file and holds the launchers, the host emulators include it behind
// tests/lane_emu.h.
#pragma once
#include <cstddef>
#include <cstdint>
#include "trace_layout.h"

namespace zk {
namespace gpu {

__device__ const uint32_t SHA256_RK[64] = {      // FIPS 180-4 4.2.2
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174,
    0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967,
    0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
    0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};

__device__ __forceinline__ uint32_t sha_rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

// the 16 words of block j of the padded message.  Byte q of it is the message's below msg_len; behind it a chain key has nothing (msg_len is a multiple of 64), a final
// key has 0x80 at q = msg_len, the eight bytes of be64(total_bits) at the end of the last block and zeros between.  No byte at or beyond msg_len is read
__device__ __forceinline__ void sha_load_block(uint32_t w[16], const uint8_t *__restrict__ msg, size_t msg_len, uint32_t kind, size_t nblk, uint64_t total_bits, size_t j) {
#pragma unroll
    for (int t = 0; t < 16; t++) {
        uint32_t v = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const size_t q = 64 * j + 4 * (size_t)t + (size_t)i;
            uint32_t byte = 0;
            if (q < msg_len) byte = msg[q];
            else if (kind == 2) {
                if (q == msg_len) byte = 0x80;
                else if (q + 8 >= 64 * nblk) byte = (uint32_t)(total_bits >> (8 * (64 * nblk - 1 - q))) & 0xff;
            }
            v = (v << 8) | byte;
        }
        w[t] = v;
    }
}

// One compression: st (a .. h on entry, the feed-forward on return) over the ring w (the block's 16 words on entry).  STORE: every intermediate into the slot, as
// 32-bit words at the TRD_* byte offsets; without it nothing is stored.  Sums are taken in 64 bits so that the carries the circuit allocates fall out of the high word
template <bool STORE>
__device__ __forceinline__ void sha_compress(uint32_t st[8], uint32_t w[16], uint32_t *__restrict__ slot) {
    uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
#pragma unroll
    for (int t = 0; t < 64; t++) {
        if (t >= 16) {
            const uint32_t x = w[(t - 15) & 15], y = w[(t - 2) & 15];
            const uint32_t s0x = sha_rotr(x, 7) ^ sha_rotr(x, 18), s0 = s0x ^ (x >> 3), s1x = sha_rotr(y, 17) ^ sha_rotr(y, 19), s1 = s1x ^ (y >> 10);
            const uint64_t sum = (uint64_t)s1 + w[(t - 7) & 15] + s0 + w[t & 15];
            w[t & 15] = (uint32_t)sum;
            if (STORE) {
                uint32_t *o = slot + (TRD_SCH + TRD_SCH_STRIDE * (t - 16)) / 4;
                o[TRD_SCH_S0X / 4] = s0x; o[TRD_SCH_S0 / 4] = s0; o[TRD_SCH_S1X / 4] = s1x; o[TRD_SCH_S1 / 4] = s1; o[TRD_SCH_W / 4] = (uint32_t)sum; o[TRD_SCH_CARRY / 4] = (uint32_t)(sum >> 32);
            }
        }
        const uint32_t S1x = sha_rotr(e, 6) ^ sha_rotr(e, 11), S1 = S1x ^ sha_rotr(e, 25), ch = (e & f) | (~e & g);
        const uint32_t S0x = sha_rotr(a, 2) ^ sha_rotr(a, 13), S0 = S0x ^ sha_rotr(a, 22), ab = a ^ b, maj = (ab & c) | (~ab & a);
        const uint64_t t1 = (uint64_t)h + S1 + ch + SHA256_RK[t] + w[t & 15];
        const uint64_t se = t1 + d, sa = t1 + S0 + maj;
        if (STORE) {
            uint32_t *o = slot + (TRD_RND + TRD_RND_STRIDE * t) / 4;
            o[TRD_RND_S1X / 4] = S1x; o[TRD_RND_S1 / 4] = S1; o[TRD_RND_CH / 4] = ch; o[TRD_RND_S0X / 4] = S0x; o[TRD_RND_S0 / 4] = S0; o[TRD_RND_AB / 4] = ab; o[TRD_RND_MAJ / 4] = maj;
            o[TRD_RND_E / 4] = (uint32_t)se; o[TRD_RND_A / 4] = (uint32_t)sa; o[TRD_RND_CE / 4] = (uint32_t)(se >> 32); o[TRD_RND_CA / 4] = (uint32_t)(sa >> 32);
        }
        h = g; g = f; f = e; e = (uint32_t)se; d = c; c = b; b = a; a = (uint32_t)sa;
    }
    const uint32_t out[8] = {a, b, c, d, e, f, g, h};
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const uint64_t sum = (uint64_t)st[k] + out[k];
        st[k] = (uint32_t)sum;
        if (STORE) { slot[TRD_FF / 4 + k] = (uint32_t)sum; slot[(TRD_FF + TRD_FF_CARRY) / 4 + k] = (uint32_t)(sum >> 32); }
    }
}

// Lane (p, c) of either digest kernel, the proof's region at dg: H_in from the 32 bytes at hin, compressions 0 .. c - 1 re-walked in registers, compression c stored
// into its slot; lane c = 0 also stores H_in, the last lane H_out and -- BITS: the region of a GCM digest record's last segment -- the 16 bytes be64(total_bits) ||
// zeros behind the slots
template <bool BITS>
__device__ __forceinline__ void sha_trace_lane(uint8_t *__restrict__ dg, const uint8_t *__restrict__ msg, uint32_t msg_len, const uint8_t *__restrict__ hin, uint32_t kind, uint32_t nblk,
                                               uint64_t total_bits, uint32_t c) {
    uint32_t st[8], w[16];
#pragma unroll
    for (int k = 0; k < 8; k++) st[k] = (uint32_t)hin[4 * k] << 24 | (uint32_t)hin[4 * k + 1] << 16 | (uint32_t)hin[4 * k + 2] << 8 | (uint32_t)hin[4 * k + 3];
    if (c == 0) {
        uint32_t *o = reinterpret_cast<uint32_t *>(dg + TRD_HIN);
#pragma unroll
        for (int k = 0; k < 8; k++) o[k] = __builtin_bswap32(st[k]);                 // the head holds the big-endian serialisation
    }
    for (uint32_t j = 0; j < c; j++) {
        sha_load_block(w, msg, msg_len, kind, nblk, total_bits, j);
        sha_compress<false>(st, w, nullptr);
    }
    sha_load_block(w, msg, msg_len, kind, nblk, total_bits, c);
    sha_compress<true>(st, w, reinterpret_cast<uint32_t *>(dg + TRD_SLOT0 + (size_t)c * TRD_SLOT_STRIDE));
    if (c + 1 == nblk) {
        uint32_t *o = reinterpret_cast<uint32_t *>(dg + TRD_HOUT);
#pragma unroll
        for (int k = 0; k < 8; k++) o[k] = __builtin_bswap32(st[k]);
        if (BITS) {
            uint32_t *b = reinterpret_cast<uint32_t *>(dg + TRS_DG_BITS((size_t)nblk));
            b[0] = __builtin_bswap32((uint32_t)(total_bits >> 32)); b[1] = __builtin_bswap32((uint32_t)total_bits); b[2] = 0; b[3] = 0;
        }
    }
}

// hdrs: nproofs x hdr_stride bytes, the proofs' public headers; a proof's H_in is the 32 bytes at hin_off of its header.  msgs: nproofs x msg_len bytes, packed.
// dg_off: the digest region's offset in a trace (16-byte aligned, as are the traces: the slots are written with word stores)
__global__ void k_sha256_trace(uint8_t *__restrict__ trace, size_t stride, size_t dg_off, const uint8_t *__restrict__ msgs, const uint8_t *__restrict__ hdrs, size_t hdr_stride, size_t hin_off,
                               uint32_t nproofs, uint32_t nblk, uint32_t msg_len, uint32_t kind, uint64_t total_bits) {
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nproofs * nblk) return;
    const uint32_t p = t / nblk, c = t % nblk;
    sha_trace_lane<false>(trace + (size_t)p * stride + dg_off, msgs + (size_t)p * msg_len, msg_len, hdrs + (size_t)p * hdr_stride + hin_off, kind, nblk, total_bits, c);
}

// The digest region of a digest record's data segment (trace_layout.h TRS_DG*), launched behind k_commit_trace on the same stream.  nproofs * nblk lanes in
// k_sha256_trace's shape and with its lane body.  What differs: H_in is the 32 bytes at TRS_HDR_HIN(aad_len) of the proof's OWN header and, for a final region (kind 2,
// a last), total_bits is the be64 at TRS_HDR_BITS(aad_len) of that header -- no kernel argument, since the proofs of one launch end records of different lengths -- and
// the last lane stores those eight bytes and eight zero bytes behind the slots, where the circuit's length inputs point.  The kernel is handed message, H_in and
// total_bits only, never a state made on the host.  One writer per byte, none ahead of the region; no LDS, no barrier, no cross-lane operation.
__global__ void k_sha256_trace_seg(uint8_t *__restrict__ trace, size_t stride, size_t dg_off, const uint8_t *__restrict__ msgs, const uint8_t *__restrict__ hdrs, size_t hdr_stride, uint32_t aad_len,
                                   uint32_t nproofs, uint32_t nblk, uint32_t msg_len, uint32_t kind) {
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nproofs * nblk) return;
    const uint32_t p = t / nblk, c = t % nblk;
    const uint8_t *hdr = hdrs + (size_t)p * hdr_stride;
    uint8_t *dg = trace + (size_t)p * stride + dg_off;
    const uint8_t *msg = msgs + (size_t)p * msg_len, *hin = hdr + TRS_HDR_HIN((size_t)aad_len);
    if (kind != 2) { sha_trace_lane<false>(dg, msg, msg_len, hin, kind, nblk, 0, c); return; }
    uint64_t total_bits = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) total_bits = (total_bits << 8) | hdr[TRS_HDR_BITS((size_t)aad_len) + i];
    sha_trace_lane<true>(dg, msg, msg_len, hin, kind, nblk, total_bits, c);
}

// The boundary commitments of a GCM segment (trace_layout.h TRS_*), launched behind the segment's GHASH kernel on the same stream: com_out needs Y_out,
// the Y of the segment's last multiplication, which it reads from the trace at yout_off.  nproofs * ncom lanes, ncom = 2 for a mid (com_in, then com_out) and 1 for a
// head (com_out) or a tail (com_in).  A lane builds the one 64-byte block key || zeros to 32 bytes || Y || salt -- the key from the key buffer, Y_in and the salts from
// the proof's header -- runs the compression of k_sha256_trace from the initial value with every store into its slot, and stores the 32 commitment bytes.  It is never
// handed a commitment made on the host.  One writer per byte, no byte ahead of the segment region touched; no LDS, no barrier, no cross-lane operation.
__global__ void k_commit_trace(uint8_t *__restrict__ trace, size_t stride, size_t seg_off, size_t yout_off, const uint8_t *__restrict__ keys, uint32_t key_bytes, const uint8_t *__restrict__ hdrs,
                               size_t hdr_stride, uint32_t nproofs, uint32_t role, uint32_t nblocks) {
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t ncom = (role == TRS_MID || role == TRS_LAST) ? 2 : 1;               // (a last is a mid here: com_in, then com_out)
    if (t >= nproofs * ncom) return;
    const uint32_t p = t / ncom;
    const bool out = role == TRS_HEAD || (ncom == 2 && t % ncom == 1);
    uint8_t *tr = trace + (size_t)p * stride, *sg = tr + seg_off;
    const uint8_t *key = keys + (size_t)key_bytes * p, *hdr = hdrs + hdr_stride * p;
    const uint8_t *y = out ? tr + yout_off : hdr + TRS_HDR_YIN, *salt = hdr + (out ? TRS_HDR_SALT_OUT : TRS_HDR_SALT_IN);
    uint32_t st[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19}, w[16];      // FIPS 180-4 5.3.3
#pragma unroll
    for (int q = 0; q < 16; q++) {
        uint32_t v = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t at = 4 * (uint32_t)q + (uint32_t)i;
            const uint32_t byte = at < 32 ? (at < key_bytes ? key[at] : 0) : at < 48 ? y[at - 32] : salt[at - 48];
            v = (v << 8) | byte;
        }
        w[q] = v;
    }
    sha_compress<true>(st, w, reinterpret_cast<uint32_t *>(sg + (out ? TRS_SLOT_OUT((size_t)nblocks) : TRS_SLOT_IN((size_t)nblocks))));
    uint32_t *o = reinterpret_cast<uint32_t *>(sg + (out ? TRS_COM_OUT : TRS_COM_IN));
#pragma unroll
    for (int k = 0; k < 8; k++) o[k] = __builtin_bswap32(st[k]);                     // the big-endian serialisation, as H_in and H_out of a digest
}

}  // namespace gpu
}  // namespace zk
