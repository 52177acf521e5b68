// csrc/kernels_witness.cuh -- the device code of the byte-typed witness trace: what fills a proof's trace buffer (layout: trace_layout.h) and expands it into z.
//   k_aes_trace       one lane per block: plain AES with every intermediate byte the circuit names written to the
//                     per-proof trace buffer; the mode (ECB / CBC) is a template parameter,
//   k_aes_trace_ctr   the same for AES-CTR: a lane derives its block's counter and the incrementer's carries from the
//                     initial counter block, and the last block of a message may be partial,
//   k_aes_trace_gcm   AES-GCM's nb + 2 AES blocks (the message under inc32 counters, H, the tag mask), and behind it
//   k_ghash_trace     the GHASH half: the V table of H and, per block, the 16,384 partial products, carries and result of
//                     one multiplication in GF(2^128), sixteen lanes per multiplication, each re-walking the chain in registers,
//   k_aes_trace_gcm_seg, k_ghash_trace_seg   the same two for one segment of a GCM record longer than one proof: counters from a public ctr0 with their
//                     carries, the chain from a hidden Y_in, a tail's last multiplication over the public length block; k_commit_trace (kernels_digest.cuh) follows,
//   k_key_tag_trace   for a key with key-tag blocks, behind any of the above: AES of the constant blocks D_t under the proof's key into the slots behind the mode's tail,
//   k_witness_expand  one lane per column of z: decode the variable's descriptor (compiled once by circuit.cpp) and gather
//                     its bit -- S-box mux-tree variables are a table lookup S[(node << (level+1)) | (x & mask)].
// The trace kernels are templates on NK, the key length in words (4, 6, 8: AES-128, -192, -256), last and with default 4, so that a call without it is AES-128: NK sets
// the schedule (FIPS-197 5.2), the round count NK + 6 and, through the TRK_* macros, where everything lies in the trace.
// Device code only: no runtime header, no launch.  One translation unit of the library includes this file and holds the launchers; the host emulators of tests/ include
// it behind tests/lane_emu.h and run the same text lane by lane under the sanitizers, which is faithful because no kernel here uses LDS, a barrier or a cross-lane operation.
#pragma once
#include <cstddef>
#include <cstdint>
#include "trace_layout.h"

namespace zk {
namespace gpu {

__device__ __forceinline__ uint8_t xtime(uint8_t c) { return (uint8_t)((c << 1) ^ (((c >> 7) & 1) * 0x1B)); }

// One block's NK + 6 rounds from s = its state after round 0.  STORE: write every intermediate the circuit names into the block's trace slot `bl`; without it the
// lane only wants the ciphertext block left in s (a CBC lane walking to its chaining value).
template <bool STORE, int NK = 4>
__device__ __forceinline__ void aes_block_rounds(uint8_t s[16], const uint8_t (*w)[4], const uint8_t *__restrict__ sbox, uint8_t *__restrict__ bl) {
    uint8_t u[16], v[16];
    for (int r = 1; r <= TRK_NR(NK); r++) {
        for (int i = 0; i < 16; i++) { v[i] = sbox[s[i]]; if (STORE) bl[TRK_BL_SB(NK) + 16 * (r - 1) + i] = v[i]; }
        for (int c = 0; c < 4; c++) for (int rr = 0; rr < 4; rr++) u[4 * c + rr] = v[4 * ((c + rr) & 3) + rr];     // ShiftRows
        if (r <= TRK_NR(NK) - 1) {
            for (int c = 0; c < 4; c++) {
                uint8_t a[4], xb[4];
                for (int k = 0; k < 4; k++) { a[k] = u[4 * c + k]; xb[k] = xtime(a[k]); if (STORE) bl[TRK_BL_XT(NK) + 16 * (r - 1) + 4 * c + k] = xb[k]; }
                // left-assoc xor chains of src/aes_circuit.rs:391-426
                const uint8_t term[4][5] = {{xb[0], a[3], a[2], xb[1], a[1]}, {xb[1], a[0], a[3], xb[2], a[2]}, {xb[2], a[1], a[0], xb[3], a[3]}, {xb[3], a[2], a[1], xb[0], a[0]}};
                for (int o = 0; o < 4; o++) {
                    uint8_t acc = term[o][0];
                    for (int q = 1; q < 5; q++) { acc ^= term[o][q]; if (STORE) bl[TRK_BL_MP(NK) + 64 * (r - 1) + 4 * (4 * c + o) + (q - 1)] = acc; }
                    v[4 * c + o] = acc;
                }
            }
        } else {
            for (int i = 0; i < 16; i++) v[i] = u[i];
        }
        for (int i = 0; i < 16; i++) { s[i] = v[i] ^ w[4 * r + i / 4][i % 4]; if (STORE) bl[TRK_BL_S(NK) + 16 * r + i] = s[i]; }
    }
}

// The key schedule (src/aes_circuit.rs:83-113; FIPS-197 5.2 for NK words): words big-endian, RotWord = bytes rotate-left 1.  Every lane needs w; the one lane per proof
// that owns the key-schedule part of the trace passes `tr` and gets the SubWord bytes and the words ahead of the Rcon xor stored, the others pass null.  NK = 8 has a
// second kind of SubWord instance at i % 8 == 4, without rotation and Rcon: its word "ahead of the Rcon xor" is W_i itself (trace_layout.h TRK_KS_INST_OF).
template <int NK = 4>
__device__ __forceinline__ void aes_key_schedule(const uint8_t *__restrict__ key, const uint8_t *__restrict__ sbox, uint8_t (*w)[4], uint8_t *__restrict__ tr) {
    const uint8_t rc[10] = {0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x80, 0x1B, 0x36};
    for (int i = 0; i < NK; i++) for (int k = 0; k < 4; k++) w[i][k] = key[4 * i + k];
    for (int i = NK; i < TRK_KS_WORDS(NK); i++) {
        if (i % NK == 0) {
            int q = TRK_KS_INST_OF(NK, i);
            uint8_t sub[4], pre[4];
            for (int k = 0; k < 4; k++) sub[k] = sbox[w[i - 1][(k + 1) & 3]];
            for (int k = 0; k < 4; k++) { pre[k] = w[i - NK][k] ^ sub[k]; w[i][k] = pre[k]; }
            w[i][0] ^= rc[i / NK - 1];
            if (tr) for (int k = 0; k < 4; k++) { tr[TRK_KS_SUB(NK) + 4 * q + k] = sub[k]; tr[TRK_KS_PRE(NK) + 4 * q + k] = pre[k]; }
        } else if (NK == 8 && i % 8 == 4) {
            int q = TRK_KS_INST_OF(NK, i);
            uint8_t sub[4];
            for (int k = 0; k < 4; k++) sub[k] = sbox[w[i - 1][k]];
            for (int k = 0; k < 4; k++) w[i][k] = w[i - NK][k] ^ sub[k];
            if (tr) for (int k = 0; k < 4; k++) { tr[TRK_KS_SUB(NK) + 4 * q + k] = sub[k]; tr[TRK_KS_PRE(NK) + 4 * q + k] = w[i][k]; }
        } else {
            for (int k = 0; k < 4; k++) w[i][k] = w[i - NK][k] ^ w[i - 1][k];
        }
    }
}
// what the lane that owns the key-schedule part stores ahead of its mode's tail: the key and every schedule word
template <int NK = 4>
__device__ __forceinline__ void aes_store_schedule(uint8_t *__restrict__ tr, const uint8_t *__restrict__ key, const uint8_t (*w)[4]) {
    for (int i = 0; i < TRK_KEY_BYTES(NK); i++) tr[TR_KEY + i] = key[i];
    for (int i = 0; i < TRK_KS_WORDS(NK); i++) for (int k = 0; k < 4; k++) tr[TRK_KS_W(NK) + 4 * i + k] = w[i][k];
}

// grid: nproofs * (nblocks + 1) lanes; lane (p, 0) writes the key schedule part, lane (p, 1 + b) block b.
// CBC: lane (p, 0) also stores the proof's IV in the trace tail; lane (p, 1 + b) starts from prev = ivs[p], runs plain AES without stores over blocks 0 .. b - 1 to reach
// its own chaining value (at most nblocks - 1 extra blocks per lane), stores X_b = M_b ^ prev in the tail and goes on from s = X_b ^ key with all the usual stores.  The
// kernel is handed the chunk's IV only, never a chain made on the host.  ivs is not read in the ECB instantiation.
template <bool CBC, int NK = 4>
__global__ void k_aes_trace(uint8_t *__restrict__ trace, size_t stride, const uint8_t *__restrict__ msgs, const uint8_t *__restrict__ keys, const uint8_t *__restrict__ ivs,
                            uint32_t nproofs, uint32_t nblocks, const uint8_t *__restrict__ sbox) {
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nproofs * (nblocks + 1)) return;
    uint32_t p = t / (nblocks + 1), which = t % (nblocks + 1);
    uint8_t *tr = trace + (size_t)p * stride;
    const uint8_t *key = keys + TRK_KEY_BYTES(NK) * (size_t)p;
    uint8_t w[TRK_KS_WORDS(NK)][4];
    aes_key_schedule<NK>(key, sbox, w, which == 0 ? tr : nullptr);
    uint8_t *tail = tr + TRK_CBC(NK, (size_t)nblocks);          // (CBC only)
    if (which == 0) {
        aes_store_schedule<NK>(tr, key, w);
        if (CBC) for (int i = 0; i < 16; i++) tail[TR_CBC_IV + i] = ivs[16 * (size_t)p + i];
        return;
    }
    uint32_t b = which - 1;
    uint8_t *bl = tr + TRK_BLOCK0(NK) + (size_t)b * TRK_BLOCK_STRIDE(NK);
    const uint8_t *msg = msgs + ((size_t)p * nblocks + b) * 16;
    uint8_t s[16];
    if (CBC) {
        uint8_t prev[16];
        for (int i = 0; i < 16; i++) prev[i] = ivs[16 * (size_t)p + i];
        for (uint32_t j = 0; j < b; j++) {
            const uint8_t *mj = msgs + ((size_t)p * nblocks + j) * 16;
            for (int i = 0; i < 16; i++) s[i] = mj[i] ^ prev[i] ^ key[i];
            aes_block_rounds<false, NK>(s, w, sbox, nullptr);
            for (int i = 0; i < 16; i++) prev[i] = s[i];
        }
        for (int i = 0; i < 16; i++) {
            uint8_t x = msg[i] ^ prev[i];
            bl[TR_BL_MSG + i] = msg[i]; tail[TR_CBC_X + 16 * b + i] = x; s[i] = x ^ key[i]; bl[TR_BL_S + i] = s[i];
        }
    } else {
        for (int i = 0; i < 16; i++) { bl[TR_BL_MSG + i] = msg[i]; s[i] = msg[i] ^ key[i]; bl[TR_BL_S + i] = s[i]; }
    }
    aes_block_rounds<true, NK>(s, w, sbox, bl);
}

// out = in + n mod 2^128 over 16 big-endian bytes
__device__ __forceinline__ void ctr_add(const uint8_t *__restrict__ in, uint32_t n, uint8_t out[16]) {
    uint32_t c = n;
    for (int i = 15; i >= 0; i--) { uint32_t t = in[i] + (c & 0xff); out[i] = (uint8_t)t; c = (c >> 8) + (t >> 8); }
}

// CTR: the same grid.  Lane (p, 0) writes the key schedule part and the proof's initial counter block; lane (p, 1 + b) computes CTR_b = icbs[p] + b itself, the carries
// K_b of CTR_{b-1} + 1 (trace_layout.h), runs the block's rounds from CTR_b ^ key and stores C_b = M_b ^ S_10.  Messages are packed at msg_len bytes per proof,
// nblocks = ceil(msg_len / 16): the last block's lane reads only the bytes below msg_len and fills the rest of its message and C slots with zeros.  Blocks do not depend
// on one another, so no lane walks a chain, and the kernel is handed the counter only, never a keystream made on the host.
template <int NK = 4>
__global__ void k_aes_trace_ctr(uint8_t *__restrict__ trace, size_t stride, const uint8_t *__restrict__ msgs, const uint8_t *__restrict__ keys, const uint8_t *__restrict__ icbs,
                                uint32_t nproofs, uint32_t nblocks, uint32_t msg_len, const uint8_t *__restrict__ sbox) {
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nproofs * (nblocks + 1)) return;
    uint32_t p = t / (nblocks + 1), which = t % (nblocks + 1);
    uint8_t *tr = trace + (size_t)p * stride;
    const uint8_t *key = keys + TRK_KEY_BYTES(NK) * (size_t)p, *icb = icbs + 16 * (size_t)p;
    uint8_t w[TRK_KS_WORDS(NK)][4];
    aes_key_schedule<NK>(key, sbox, w, which == 0 ? tr : nullptr);
    uint8_t *tail = tr + TRK_CTR(NK, (size_t)nblocks);
    if (which == 0) {
        aes_store_schedule<NK>(tr, key, w);
        for (int i = 0; i < 16; i++) tail[TR_CTR_ICB + i] = icb[i];
        return;
    }
    uint32_t b = which - 1;
    uint8_t *bl = tr + TRK_BLOCK0(NK) + (size_t)b * TRK_BLOCK_STRIDE(NK), *slot = tail + TR_CTR_BLOCK0 + (size_t)b * TR_CTR_BLOCK_STRIDE;
    uint8_t ctr[16], carry[16], s[16], m[16];
    ctr_add(icb, b, ctr);
    for (int i = 0; i < 16; i++) carry[i] = 0;
    if (b) {
        uint8_t prev[16];
        ctr_add(icb, b - 1, prev);
        for (int i = 0; i < 128 && ((prev[15 - i / 8] >> (i % 8)) & 1); i++) carry[15 - i / 8] |= (uint8_t)(1u << (i % 8));
    }
    uint32_t have = msg_len - 16 * b < 16 ? msg_len - 16 * b : 16;          // (16 b < msg_len: nblocks = ceil(msg_len / 16))
    const uint8_t *msg = msgs + (size_t)p * msg_len + 16 * (size_t)b;
    for (uint32_t i = 0; i < 16; i++) m[i] = i < have ? msg[i] : 0;
    for (int i = 0; i < 16; i++) { slot[TR_CTR_BL_CTR + i] = ctr[i]; slot[TR_CTR_BL_CARRY + i] = carry[i]; bl[TR_BL_MSG + i] = m[i]; s[i] = ctr[i] ^ key[i]; bl[TR_BL_S + i] = s[i]; }
    aes_block_rounds<true, NK>(s, w, sbox, bl);
    for (uint32_t i = 0; i < 16; i++) slot[TR_CTR_BL_CT + i] = i < have ? (uint8_t)(m[i] ^ s[i]) : 0;
}

// GCM, the AES half: nproofs * (nblocks + 3) lanes, nblocks = ceil(msg_len / 16) message blocks, naad = ceil(aad_len / 16).  Lane (p, 0) writes the key schedule part, the
// proof's iv and its aad (zero-padded to whole blocks); lane (p, 1 + s) is AES slot s: the message blocks under iv || be32(s + 2) for s < nblocks, then H from the zero
// block, then J_0 = iv || 00000001.  A message lane stores C_s = M_s ^ S_10 for the bytes that exist and zeros behind them.  Messages are packed at msg_len bytes per
// proof, the public headers (iv, then aad) at 12 + aad_len bytes.  The kernel is handed key, iv, aad and message only.
template <int NK = 4>
__global__ void k_aes_trace_gcm(uint8_t *__restrict__ trace, size_t stride, const uint8_t *__restrict__ msgs, const uint8_t *__restrict__ keys, const uint8_t *__restrict__ hdrs,
                                uint32_t nproofs, uint32_t nblocks, uint32_t naad, uint32_t msg_len, uint32_t aad_len, const uint8_t *__restrict__ sbox) {
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nproofs * (nblocks + 3)) return;
    uint32_t p = t / (nblocks + 3), which = t % (nblocks + 3);
    uint8_t *tr = trace + (size_t)p * stride;
    const uint8_t *key = keys + TRK_KEY_BYTES(NK) * (size_t)p, *hdr = hdrs + (size_t)p * (12 + (size_t)aad_len);
    uint8_t w[TRK_KS_WORDS(NK)][4];
    aes_key_schedule<NK>(key, sbox, w, which == 0 ? tr : nullptr);
    uint8_t *tail = tr + TRK_GCM(NK, (size_t)nblocks);
    if (which == 0) {
        aes_store_schedule<NK>(tr, key, w);
        for (int i = 0; i < 16; i++) tail[TR_GCM_IV + i] = i < 12 ? hdr[i] : 0;
        for (uint32_t i = 0; i < 16 * naad; i++) tail[TR_GCM_AAD + i] = i < aad_len ? hdr[12 + i] : 0;
        return;
    }
    uint32_t slot = which - 1;
    uint8_t *bl = tr + TRK_BLOCK0(NK) + (size_t)slot * TRK_BLOCK_STRIDE(NK);
    uint8_t in[16], s[16], m[16];
    uint32_t ctr = slot < nblocks ? slot + 2 : 1, have = 0;
    for (int i = 0; i < 16; i++) in[i] = slot == nblocks ? 0 : (i < 12 ? hdr[i] : (uint8_t)(ctr >> (8 * (15 - i))));
    if (slot < nblocks) have = msg_len - 16 * slot < 16 ? msg_len - 16 * slot : 16;          // (16 slot < msg_len: nblocks = ceil(msg_len / 16))
    const uint8_t *msg = msgs + (size_t)p * msg_len + 16 * (size_t)(slot < nblocks ? slot : 0);      // (not read by the H and J_0 lanes: have = 0)
    for (uint32_t i = 0; i < 16; i++) m[i] = i < have ? msg[i] : 0;
    for (int i = 0; i < 16; i++) { bl[TR_BL_MSG + i] = m[i]; s[i] = in[i] ^ key[i]; bl[TR_BL_S + i] = s[i]; }
    aes_block_rounds<true, NK>(s, w, sbox, bl);
    if (slot < nblocks) for (uint32_t i = 0; i < 16; i++) tail[TR_GCM_CT(naad) + 16 * slot + i] = i < have ? (uint8_t)(m[i] ^ s[i]) : 0;
}

// GF(2^128) in GCM's convention as two words: bit k (the coefficient of alpha^k) is bit 63 - k of hi for k < 64 and bit 127 - k of lo behind; byte j of the block
// is bits 8 j .. 8 j + 7, its most significant bit first.
struct Gf128 { uint64_t hi, lo; };
struct alignas(16) Bytes16 { uint8_t b[16]; };                 // one 16-byte vector store
__device__ __forceinline__ Gf128 gf_load(const uint8_t *__restrict__ b) { Gf128 r = {0, 0}; for (int i = 0; i < 8; i++) { r.hi = (r.hi << 8) | b[i]; r.lo = (r.lo << 8) | b[8 + i]; } return r; }
__device__ __forceinline__ uint8_t gf_byte(const Gf128 &v, uint32_t j) { return (uint8_t)(j < 8 ? v.hi >> (56 - 8 * j) : v.lo >> (56 - 8 * (j - 8))); }
__device__ __forceinline__ uint32_t gf_bit(const Gf128 &v, int k) { return (uint32_t)(k < 64 ? v.hi >> (63 - k) : v.lo >> (127 - k)) & 1u; }
__device__ __forceinline__ void gf_times_alpha(Gf128 &v) {     // SP 800-38D Algorithm 1, step 3: V >> 1, xor R = 11100001 || 0^120 if the bit shifted out was set
    uint64_t lsb = v.lo & 1;
    v.lo = (v.lo >> 1) | (v.hi << 63); v.hi >>= 1;
    if (lsb) v.hi ^= 0xE100000000000000ull;
}
__device__ __forceinline__ Gf128 gf_mul(const Gf128 &x, Gf128 v) {
    Gf128 z = {0, 0};
    for (int i = 0; i < 128; i++) { if (gf_bit(x, i)) { z.hi ^= v.hi; z.lo ^= v.lo; } gf_times_alpha(v); }
    return z;
}

// What the two GHASH kernels share.  Byte column j of the V table (V_0 = v, V_{i+1} = V_i * alpha) into the 128 contiguous bytes at col, eight 16-byte stores
__device__ __forceinline__ void ghash_store_v_column(uint8_t *col, Gf128 v, uint32_t j) {
    for (int c = 0; c < 8; c++) {
        Bytes16 o;
        for (int u = 0; u < 16; u++) { o.b[u] = gf_byte(v, j); gf_times_alpha(v); }
        *reinterpret_cast<Bytes16 *>(col + 16 * c) = o;
    }
}
// Lane j's share of one multiplication Y = X * H (v = H on entry) into the multiplication's slot mul: byte j of X, byte column j of P, the q bytes of output bits
// 8 j .. 8 j + 7 and byte j of Y, which it returns
__device__ __forceinline__ uint8_t ghash_store_mul(uint8_t *mul, const Gf128 &x, Gf128 v, uint32_t j) {
    mul[TR_GCM_MUL_X + j] = gf_byte(x, j);
    uint32_t cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};                // how many of the 128 products are set, per bit of byte j
    for (int c = 0; c < 8; c++) {
        Bytes16 o;
        for (int u = 0; u < 16; u++) {
            uint8_t pb = gf_bit(x, 16 * c + u) ? gf_byte(v, j) : 0;
            o.b[u] = pb;
            for (int bit = 0; bit < 8; bit++) cnt[bit] += (pb >> bit) & 1u;
            gf_times_alpha(v);
        }
        *reinterpret_cast<Bytes16 *>(mul + TR_GCM_MUL_P + 128 * j + 16 * c) = o;
    }
    uint8_t y = 0;
    for (int bit = 0; bit < 8; bit++) {                         // output bit k = 8 j + 7 - bit
        mul[TR_GCM_MUL_Q + 8 * j + 7 - bit] = (uint8_t)(cnt[bit] >> 1);
        y |= (uint8_t)((cnt[bit] & 1u) << bit);
    }
    mul[TR_GCM_MUL_Y + j] = y;
    return y;
}

// GCM, the GHASH half, launched behind k_aes_trace_gcm on the same stream: it reads H = S_Nr of slot nblocks, the aad, every C_b and S_Nr of slot nblocks + 1 from the
// trace.  nproofs * (n_mul + 1) * 16 lanes, n_mul = naad + nblocks + 1.  Lane (p, m, j), m < n_mul, recomputes the chain Y_0 .. Y_{m-1} in registers (two words of
// state, 128 steps of shift and conditional xor per multiplication, no stores -- the way a CBC lane re-walks its chain), then stores byte j of X_m, byte column j of P_m
// (128 contiguous bytes, eight 16-byte stores), the q bytes of output bits 8 j .. 8 j + 7 and byte j of Y_m; the lanes of the last multiplication add byte j of the tag.
// Lane (p, n_mul, j) stores byte column j of the V table.  Every byte of the tail has exactly one writer; no LDS, no barrier, no cross-lane operation.
template <int NK = 4>
__global__ void k_ghash_trace(uint8_t *__restrict__ trace, size_t stride, uint32_t nproofs, uint32_t nblocks, uint32_t naad, uint32_t msg_len, uint32_t aad_len) {
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t n_mul = naad + nblocks + 1, per_proof = (n_mul + 1) * 16;
    if (t >= nproofs * per_proof) return;
    uint32_t p = t / per_proof, m = (t % per_proof) / 16, j = t % 16;
    uint8_t *tr = trace + (size_t)p * stride, *tail = tr + TRK_GCM(NK, (size_t)nblocks);
    const Gf128 h = gf_load(tr + TRK_BLOCK0(NK) + (size_t)nblocks * TRK_BLOCK_STRIDE(NK) + TRK_BL_CT(NK));
    if (m == n_mul) { ghash_store_v_column(tail + TR_GCM_V(naad, nblocks) + 128 * j, h, j); return; }
    Gf128 x = {0, 0};
    for (uint32_t mm = 0;; mm++) {
        Gf128 blk;
        if (mm < naad + nblocks) blk = gf_load(tail + TR_GCM_AAD + 16 * (size_t)mm);            // (the C_b lie right behind the aad blocks)
        else { blk.hi = 8 * (uint64_t)aad_len; blk.lo = 8 * (uint64_t)msg_len; }
        x.hi ^= blk.hi; x.lo ^= blk.lo;
        if (mm == m) break;
        x = gf_mul(x, h);
    }
    const uint8_t y = ghash_store_mul(tail + TR_GCM_MUL0(naad, nblocks) + (size_t)m * TR_GCM_MUL_STRIDE, x, h, j);
    if (m + 1 == n_mul) tail[TR_GCM_TAG(naad, nblocks) + j] = y ^ tr[TRK_BLOCK0(NK) + (size_t)(nblocks + 1) * TRK_BLOCK_STRIDE(NK) + TRK_BL_CT(NK) + j];
}

// The key tag (trace_layout.h TRK_KT), for every mode, launched behind the mode's own kernel(s) on the same stream: nproofs * ntags lanes, ntags = 1 or 2.
// Lane (p, t) runs the key schedule in registers (no schedule stores: that part of the trace belongs to the mode's lane (p, 0)), builds D_t = "zkaes-keyta" || t ||
// 00000000 and fills tag slot t at tag_off + t strides like any block slot: D_t in the message field, S_0 = D_t ^ key, every round's intermediates, S_Nr = the tag.  It is
// handed the keys only, never a tag made on the host.  Every byte of the slots has exactly one writer and no byte ahead of tag_off is touched; no LDS, no barrier, no
// cross-lane operation.
template <int NK = 4>
__global__ void k_key_tag_trace(uint8_t *__restrict__ trace, size_t stride, size_t tag_off, const uint8_t *__restrict__ keys, uint32_t nproofs, uint32_t ntags, const uint8_t *__restrict__ sbox) {
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nproofs * ntags) return;
    uint32_t p = t / ntags, which = t % ntags;
    const uint8_t *key = keys + TRK_KEY_BYTES(NK) * (size_t)p;
    uint8_t w[TRK_KS_WORDS(NK)][4];
    aes_key_schedule<NK>(key, sbox, w, nullptr);
    uint8_t *bl = trace + (size_t)p * stride + tag_off + (size_t)which * TRK_BLOCK_STRIDE(NK);
    const char prefix[] = TRK_KT_D_PREFIX;
    uint8_t s[16];
    for (int i = 0; i < 16; i++) {
        uint8_t d = i < 11 ? (uint8_t)prefix[i] : i == 11 ? (uint8_t)which : 0;
        bl[TR_BL_MSG + i] = d; s[i] = d ^ key[i]; bl[TR_BL_S + i] = s[i];
    }
    aes_block_rounds<true, NK>(s, w, sbox, bl);
}

// GCM segments (trace_layout.h TRS_*), the AES half, in the shape of k_aes_trace_gcm.  role = TRS_HEAD, TRS_MID or TRS_TAIL; nslots = nblocks + 1 AES
// slots, one more for a tail.  nproofs * (nslots + 1) lanes.  Lane (p, 0) writes the key schedule part and the proof's header: iv and ctr0 into the tail's iv slot,
// the aad (head), and Y_in, the two salts and the length block into the segment region.  Lane (p, 1 + s) is AES slot s: data block s < nblocks under
// iv || be32(ctr0 + s mod 2^32), with its counter and carry bytes stored in the segment region, then H from the zero block, then (tail) J_0 = iv || 00000001.  A data
// lane stores C_s = M_s ^ S_Nr for the bytes that exist and zeros behind them.  hdrs: nproofs x TRS_HDR_BYTES(aad_len) bytes; the kernel is handed key, iv, ctr0, aad,
// message, Y_in, the salts and the length block only.
// A digest record adds two shapes, which take the same path: role = TRS_LAST is a mid whose msg_len is a byte count, its final block cut as a tail's; and
// a tail with nblocks = 0, the closing tail, has the two lanes H (slot 0) and J_0 (slot 1) behind lane (p, 0) and reads no message byte.
template <int NK = 4>
__global__ void k_aes_trace_gcm_seg(uint8_t *__restrict__ trace, size_t stride, const uint8_t *__restrict__ msgs, const uint8_t *__restrict__ keys, const uint8_t *__restrict__ hdrs,
                                    uint32_t nproofs, uint32_t role, uint32_t nblocks, uint32_t naad, uint32_t msg_len, uint32_t aad_len, const uint8_t *__restrict__ sbox) {
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t nslots = TRS_SLOTS(role, nblocks);
    if (t >= nproofs * (nslots + 1)) return;
    uint32_t p = t / (nslots + 1), which = t % (nslots + 1);
    uint8_t *tr = trace + (size_t)p * stride;
    const uint8_t *key = keys + TRK_KEY_BYTES(NK) * (size_t)p, *hdr = hdrs + (size_t)p * TRS_HDR_BYTES((size_t)aad_len);
    uint8_t w[TRK_KS_WORDS(NK)][4];
    aes_key_schedule<NK>(key, sbox, w, which == 0 ? tr : nullptr);
    uint8_t *tail = tr + TRS_GCM(NK, role, (size_t)nblocks), *sg = tail + TRS_SEG(role, (size_t)naad, (size_t)nblocks);
    if (which == 0) {
        aes_store_schedule<NK>(tr, key, w);
        for (int i = 0; i < 16; i++) tail[TR_GCM_IV + i] = hdr[TRS_HDR_IV + i];                  // (iv, then ctr0)
        for (uint32_t i = 0; i < 16 * naad; i++) tail[TR_GCM_AAD + i] = i < aad_len ? hdr[TRS_HDR_AAD + i] : 0;
        for (int i = 0; i < 16; i++) {
            sg[TRS_YIN + i] = hdr[TRS_HDR_YIN + i]; sg[TRS_SALT_IN + i] = hdr[TRS_HDR_SALT_IN + i];
            sg[TRS_SALT_OUT + i] = hdr[TRS_HDR_SALT_OUT + i]; sg[TRS_LEN + i] = hdr[TRS_HDR_LEN + i];
        }
        return;
    }
    uint32_t slot = which - 1;
    uint8_t *bl = tr + TRK_BLOCK0(NK) + (size_t)slot * TRK_BLOCK_STRIDE(NK);
    uint8_t in[16], s[16], m[16];
    const uint32_t ctr0 = (uint32_t)hdr[TRS_HDR_CTR0] << 24 | (uint32_t)hdr[TRS_HDR_CTR0 + 1] << 16 | (uint32_t)hdr[TRS_HDR_CTR0 + 2] << 8 | hdr[TRS_HDR_CTR0 + 3];
    uint32_t ctr = slot < nblocks ? ctr0 + slot : 1, have = 0;
    for (int i = 0; i < 16; i++) in[i] = slot == nblocks ? 0 : (i < 12 ? hdr[TRS_HDR_IV + i] : (uint8_t)(ctr >> (8 * (15 - i))));
    if (slot < nblocks) {
        have = msg_len - 16 * slot < 16 ? msg_len - 16 * slot : 16;                                  // (16 slot < msg_len: nblocks = ceil(msg_len / 16))
        uint8_t *cs = sg + TRS_BLOCK_CTR0 + (size_t)slot * TRS_BLOCK_CTR_STRIDE;
        const uint32_t prev = ctr - 1;
        uint32_t carry = 0;
        if (slot) for (int i = 0; i < 31 && ((prev >> i) & 1); i++) carry |= 1u << i;              // (no carry out of position 31: the sum is mod 2^32)
        for (int i = 0; i < 4; i++) { cs[TRS_BL_CTR + i] = (uint8_t)(ctr >> (24 - 8 * i)); cs[TRS_BL_CARRY + i] = (uint8_t)(carry >> (24 - 8 * i)); }
    }
    const uint8_t *msg = msgs + (size_t)p * msg_len + 16 * (size_t)(slot < nblocks ? slot : 0);      // (not read by the H and J_0 lanes: have = 0)
    for (uint32_t i = 0; i < 16; i++) m[i] = i < have ? msg[i] : 0;
    for (int i = 0; i < 16; i++) { bl[TR_BL_MSG + i] = m[i]; s[i] = in[i] ^ key[i]; bl[TR_BL_S + i] = s[i]; }
    aes_block_rounds<true, NK>(s, w, sbox, bl);
    if (slot < nblocks) for (uint32_t i = 0; i < 16; i++) tail[TR_GCM_CT(naad) + 16 * slot + i] = i < have ? (uint8_t)(m[i] ^ s[i]) : 0;
}

// GCM segments, the GHASH half, in the shape of k_ghash_trace and launched behind k_aes_trace_gcm_seg on the same stream: it reads H, the aad, every C_b, Y_in, the
// length block and (tail) S_Nr of the J_0 slot from the trace.  nproofs * (n_mul + 1) * 16 lanes, n_mul = TRS_MULS.  The chain starts from zero for a head and from Y_in
// otherwise; the blocks are the aad (head), the C_b and, as a tail's last, the length block.  Only the lanes of a tail's last multiplication store a tag byte.  Every
// byte has exactly one writer; no LDS, no barrier, no cross-lane operation.
// A last (TRS_LAST) chains from Y_in over its nblocks C_b as a mid does (TRS_MULS); the closing tail (nblocks = 0) runs its ONE multiplication over
// X = Y_in ^ the length block and stores the tag.
template <int NK = 4>
__global__ void k_ghash_trace_seg(uint8_t *__restrict__ trace, size_t stride, uint32_t nproofs, uint32_t role, uint32_t nblocks, uint32_t naad) {
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t n_mul = TRS_MULS(role, naad, nblocks), per_proof = (n_mul + 1) * 16;
    if (t >= nproofs * per_proof) return;
    uint32_t p = t / per_proof, m = (t % per_proof) / 16, j = t % 16;
    uint8_t *tr = trace + (size_t)p * stride, *tail = tr + TRS_GCM(NK, role, (size_t)nblocks), *sg = tail + TRS_SEG(role, (size_t)naad, (size_t)nblocks);
    const Gf128 h = gf_load(tr + TRK_BLOCK0(NK) + (size_t)nblocks * TRK_BLOCK_STRIDE(NK) + TRK_BL_CT(NK));
    if (m == n_mul) { ghash_store_v_column(tail + TR_GCM_V(naad, nblocks) + 128 * j, h, j); return; }
    Gf128 x = {0, 0};
    if (role != TRS_HEAD) x = gf_load(sg + TRS_YIN);
    for (uint32_t mm = 0;; mm++) {
        const Gf128 blk = gf_load(mm < naad + nblocks ? tail + TR_GCM_AAD + 16 * (size_t)mm : sg + TRS_LEN);       // (the C_b lie right behind the aad blocks)
        x.hi ^= blk.hi; x.lo ^= blk.lo;
        if (mm == m) break;
        x = gf_mul(x, h);
    }
    const uint8_t y = ghash_store_mul(tail + TR_GCM_MUL0(naad, nblocks) + (size_t)m * TR_GCM_MUL_STRIDE, x, h, j);
    if (role == TRS_TAIL && m + 1 == n_mul) tail[TRS_TAG(role, naad, nblocks) + j] = y ^ tr[TRK_BLOCK0(NK) + (size_t)(nblocks + 1) * TRK_BLOCK_STRIDE(NK) + TRK_BL_CT(NK) + j];
}

__global__ void k_witness_expand(uint8_t *__restrict__ z, const uint32_t *__restrict__ desc, uint32_t ncols, const uint8_t *__restrict__ trace,
                                 const uint32_t *__restrict__ sbox_in_off, const uint32_t *__restrict__ sbox_tmpl, const uint8_t *__restrict__ sbox) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ncols) return;
    uint32_t d = desc[i], kind = d >> WD_KIND_SHIFT, bit;
    if (kind == WD_BYTEBIT) {
        uint32_t off = (d >> 4) & 0x3ffffff, b = (d >> 1) & 7;
        bit = ((trace[off] >> b) & 1) ^ (d & 1);
    } else if (kind == WD_SBOX) {
        uint32_t inst = (d >> 11) & 0x7ffff, te = sbox_tmpl[(d >> 1) & 0x3ff];
        uint32_t lvl = (te >> 12) & 7, node = (te >> 4) & 0xff, b = (te >> 1) & 7;
        uint32_t x = trace[sbox_in_off[inst]];
        uint32_t idx = (node << (lvl + 1)) | (x & ((2u << lvl) - 1));
        bit = ((sbox[idx] >> b) & 1) ^ (d & 1);
    } else {
        bit = d & 1;
    }
    z[i] = (uint8_t)bit;
}

}  // namespace gpu
}  // namespace zk
