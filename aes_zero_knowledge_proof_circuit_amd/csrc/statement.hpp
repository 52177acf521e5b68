// csrc/statement.hpp -- what a proof states, in one place, for the prover (marlin.cpp) and the verifiers (capi_host.cpp).  Host only, no device header.
// Every mode is "message, key, a public header of mode_header_bytes(c) bytes, optionally H_in": nothing (ECB), the iv (CBC), the initial counter block (CTR), iv then aad
// (GCM).  The public input behind the leading One is the header's bits, the ciphertext's, GCM's tag, the key tag, then H_in and H_out, then a reveal key's mask and
// revealed bytes -- each byte LSB first.  The prover
// and the verifier must agree on all of it bit for bit, so neither side has a copy of its own (tests/statement_host_check.cpp).
#pragma once
#include <cstring>
#include <initializer_list>
#include <stdexcept>
#include <string>
#include "circuit.hpp"
#include "marlin.hpp"

namespace zk {

// The header entering chunk j of a chunked job whose first chunk enters under hdr0: CBC the 16 ciphertext bytes ahead of the slice (hdr0, the iv, for j = 0), CTR
// hdr0 + j x the chunk's blocks, ECB nothing.  ct is the job's ciphertext (read for CBC, j > 0, only).  Returns the bytes written to out16: 0 or 16
inline size_t chunk_mode_header(int kind, size_t j, size_t chunk_bytes, const uint8_t *hdr0, const uint8_t *ct, uint8_t out16[16]) {
    if (kind == CIRCUIT_AES_CBC) memcpy(out16, j ? ct + chunk_bytes * j - 16 : hdr0, 16);
    else if (kind == CIRCUIT_AES_CTR) ctr_counter_add(hdr0, (uint64_t)j * (chunk_bytes / 16), out16);
    else return 0;
    return 16;
}

// The host's side of a statement by the key's mode: ct = len bytes (len = the key's message length, or a whole chunked job's), and GCM's tag where asked for
inline void host_encrypt(const Circuit &c, const uint8_t *msg, size_t len, const uint8_t *key, const uint8_t *hdr, uint8_t *ct, uint8_t *tag_or_null) {
    uint8_t tag[16];
    if (c.kind == CIRCUIT_AES) aes_ecb_encrypt_host(msg, len, key, c.key_bytes, ct);
    else if (c.kind == CIRCUIT_AES_CBC) aes128_cbc_encrypt_host(msg, len, key, hdr, ct, c.key_bytes);
    else if (c.kind == CIRCUIT_AES_CTR) aes128_ctr_crypt_host(msg, len, key, hdr, ct, c.key_bytes);
    else aes128_gcm_encrypt_host(msg, len, key, hdr, hdr + 12, c.aad_bytes, ct, tag_or_null ? tag_or_null : tag, c.key_bytes);
}

// ---- selective disclosure.  A mask over L bytes is ceil(L / 8) bytes, bit i = bit i % 8 of byte i / 8; a reveal key's public input ends in the mask's
// bits, then revealed's
inline size_t mask_bytes(size_t len) { return (len + 7) / 8; }
// the mask of chunk j of a chunked job under ONE mask over the whole job: chunk boundaries are multiples of 16 bytes, so every slice begins on a mask byte (a lone
// proof, j = 0, takes any length)
inline const uint8_t *chunk_mask_slice(const uint8_t *mask, size_t j, size_t chunk_bytes) { return mask + chunk_bytes * j / 8; }
// revealed[i] = mask_i ? msg[i] : 0
inline void reveal_bytes(const uint8_t *msg, const uint8_t *mask, size_t len, uint8_t *out) {
    for (size_t i = 0; i < len; i++) out[i] = ((mask[i / 8] >> (i % 8)) & 1) ? msg[i] : 0;
}
// what both sides refuse as an argument, not as a proof: no mask, a mask bit at or beyond the length -- and, on the verifier's side, a non-zero revealed byte whose mask
// bit is 0, which a verifier that ignored it would let a caller believe proven
inline void require_mask(const uint8_t *mask, size_t len) {
    if (!mask) throw std::invalid_argument("reveal: no mask");
    for (size_t i = len; i < 8 * mask_bytes(len); i++)
        if ((mask[i / 8] >> (i % 8)) & 1) throw std::invalid_argument("reveal: the mask has a bit set at or beyond the message length");
}
inline void require_revealed(const uint8_t *mask, const uint8_t *revealed, size_t len) {
    require_mask(mask, len);
    if (!revealed) throw std::invalid_argument("reveal: no revealed bytes");
    for (size_t i = 0; i < len; i++)
        if (revealed[i] && !((mask[i / 8] >> (i % 8)) & 1)) throw std::invalid_argument("reveal: revealed byte " + std::to_string(i) + " is non-zero but its mask bit is 0");
}

// The public input without the leading One: the bits of every part in order; a part without bytes (no aad, no key tag, no states, no mask) adds nothing
struct PublicPart { const uint8_t *bytes; size_t len; };
inline std::vector<Fr> public_input_of(std::initializer_list<PublicPart> parts) {
    std::vector<Fr> pub;
    for (const PublicPart &p : parts) {
        if (!p.bytes || !p.len) continue;
        std::vector<Fr> bits = ciphertext_to_public_input(p.bytes, p.len);
        pub.insert(pub.end(), bits.begin(), bits.end());
    }
    return pub;
}

}  // namespace zk
