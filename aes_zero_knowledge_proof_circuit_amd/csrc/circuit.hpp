// csrc/circuit.hpp -- host-side R1CS compiler for the reference's AES-128-ECB circuit.
//
// Runs once per (circuit kind, block count) inside zkaes_synthesize_keys; it symbolically executes the gates of
// /root/reference/src/lib.rs:60-114,176-293 and src/aes_circuit.rs:20-427 (+ src/helpers/mod.rs:11-64, src/ops.rs:8-29)
// under the ark-r1cs-std 0.3.1 Boolean/UInt8 gadget semantics and emits
//   * A, B, C in CSR form with final column indices (what ark-relations' to_matrices() returns, after the
//     ark-marlin padding: instance padded to a power of two, matrices squared),
//   * one 32-bit *witness descriptor* per column of z saying which bit of the AES trace that variable equals, so that
//     witness generation is a data-parallel gather on the GPU (kernels_witness.hip) rather than a replay of the synthesis.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace zk {

struct CsrMatrix {
    std::vector<uint32_t> rowptr;   // rows + 1
    std::vector<uint32_t> col;
    std::vector<int64_t> coeff;     // small integers (|c| <= 2 for AES; powers of two for ops::add)
    size_t rows() const { return rowptr.empty() ? 0 : rowptr.size() - 1; }
    size_t nnz() const { return col.size(); }
};

enum CircuitKind { CIRCUIT_AES = 0, CIRCUIT_OPS_XOR = 1, CIRCUIT_OPS_ADD = 2, CIRCUIT_AES_CBC = 3, CIRCUIT_AES_CTR = 4, CIRCUIT_AES_GCM = 5, CIRCUIT_AES_GCM_SEG = 6 };

struct Circuit {
    int kind = CIRCUIT_AES;
    size_t n_blocks = 0;
    size_t message_bytes = 0;            // the statement's byte length: 16 n_blocks, except for a CTR key, or GCM key, whose last block may be partial (0 for the ops kinds)
    size_t key_bytes = 16;               // the AES key's byte length: 16, 24 or 32 (AES-128, -192, -256); the trace is laid out for it (trace_layout.h TRK_*)
    size_t aad_bytes = 0;                // GCM keys: the byte length of the additional authenticated data, part of the statement like message_bytes
    // before padding (what debug_constraint_system_status would log, src/helpers/mod.rs:73-81)
    size_t raw_constraints = 0, raw_instance = 0, raw_witness = 0;
    // after ark-marlin padding
    size_t num_instance = 0, num_witness = 0, num_constraints = 0;
    CsrMatrix A, B, C;
    std::vector<uint32_t> desc;          // num_instance + num_witness descriptors (trace_layout.h)
    std::vector<uint32_t> sbox_in_off;   // trace offset of the input byte of every S-box instance
    std::vector<uint32_t> sbox_tmpl;     // (level, node, bit) of every allocated variable of one S-box
    size_t trace_bytes = 0;
    size_t key_tag_blocks = 0;           // T = 0, 1 or 2 key-tag blocks: the last 128 T instance bits are AES_K(D_0) (, AES_K(D_1))
    size_t key_tag_off = 0;              // trace offset of tag slot 0 (trace_layout.h TRK_KT), 0 when T = 0
    int digest_kind = 0;                 // D = 0 (none), 1 (chain) or 2 (final): the last 512 instance bits are H_in, H_out of the SHA-256 compressions over the hidden message
    uint64_t digest_prefix = 0;          // final keys: P, the message bytes hashed ahead of this proof's (a multiple of 64); the padding's length field is 8 (P + message_bytes)
    size_t digest_blocks = 0;            // compressions per proof (trace_layout.h TRD_BLOCKS), 0 when D = 0
    size_t digest_off = 0;               // trace offset of the digest region (trace_layout.h TRD), 0 when D = 0
    int reveal = 0;                      // R = 0 or 1: a reveal key's last 8 ceil(L / 8) + 8 L instance bits are a per-proof mask and revealed[i] = mask_i ? M[i] : 0, L = message_bytes
    size_t reveal_off = 0;               // trace offset of the reveal region (trace_layout.h TRV), 0 when R = 0
    int seg_role = -1;                   // a GCM segment key (kind CIRCUIT_AES_GCM_SEG): 0 head, 1 mid, 2 tail (trace_layout.h TRS_*); -1 for every other key
    size_t seg_off = 0;                  // trace offset of the segment region (trace_layout.h TRS_SEG), 0 for every other key
    int seg_digest = 0;                  // a segment key of a digest record: role 3 (last) exists, a tail is the data-less closing tail, and digest_kind is chain (head, mid), final (last) or none (tail)
    size_t num_variables() const { return num_instance + num_witness; }
};

// message_len must be a multiple of 16 (else throws std::invalid_argument with the reference's message)
// Every AES compiler takes the key size in bits, 128 (the reference's, and the default), 192 or 256; anything else is std::invalid_argument.  The statement, the
// public input and the gate order inside a round, the schedule and each mode do not depend on it; the round count (Nk + 6) and the schedule (FIPS-197 5.2) do.
// key_tag_blocks (every AES compiler, default 0 = the circuit as it was): T = 1 or 2 appends, behind everything the mode emits, per t < T the rounds of the constant block
// D_t = "zkaes-keyta" || t || 00000000 under the same key and 128 public input bits equal to its S_Nr; anything but 0, 1, 2 is std::invalid_argument
// digest_kind (every AES compiler, default DIGEST_NONE = the circuit as it was): DIGEST_CHAIN appends, behind the key tag, 256 inputs H_in, the SHA-256 compressions
// (FIPS 180-4 6.2.2) of the hidden message's 64-byte blocks from H_in, and 256 inputs H_out equal to the last feed-forward; the message must then be a non-zero multiple
// of 64 bytes.  DIGEST_FINAL does the same over message || 0x80 || zeros || be64(8 (digest_prefix + message_len)) for any message length the mode allows; digest_prefix
// is a multiple of 64 with digest_prefix + message_len < 2^61, and 0 for the other kinds.  Anything else is std::invalid_argument
// reveal (every AES compiler, default 0 = the circuit as it was): 1 appends, behind the digest, ceil(L / 8) mask bytes and L revealed bytes as inputs (the mask first),
// one row per mask bit at or beyond L that pins it to zero, and per message bit ONE row mask_i * m_ij = r_ij over the message witnesses: no new witness.
// Anything but 0 or 1 is std::invalid_argument; the ops circuits have no reveal form
enum DigestKind { DIGEST_NONE = 0, DIGEST_CHAIN = 1, DIGEST_FINAL = 2 };
Circuit compile_aes_circuit(size_t message_len, size_t key_bits = 128, size_t key_tag_blocks = 0, int digest_kind = 0, uint64_t digest_prefix = 0, int reveal = 0);
Circuit compile_ops_circuit(int kind);
// AES-128-CBC over the same gadgets (no upstream counterpart; DESIGN.md "CBC"): public = 16 IV bytes then the ciphertext, private = message and key;
// per block X_b = M_b ^ C_{b-1} (C_{-1} = IV) ahead of the block's round 0.  message_len must be a non-zero multiple of 16 (else std::invalid_argument)
Circuit compile_aes_cbc_circuit(size_t message_len, size_t key_bits = 128, size_t key_tag_blocks = 0, int digest_kind = 0, uint64_t digest_prefix = 0, int reveal = 0);
// AES-128-CTR over the same gadgets (DESIGN.md "CTR"): public = the 16 bytes of the initial counter block then the ciphertext, private = message and key;
// CTR_0 = icb, CTR_b = CTR_{b-1} + 1 mod 2^128 (big-endian, SP 800-38A B.1 with m = 128), C_b = M_b ^ AES(key, CTR_b), the last block cut to the bytes that exist.
// message_len is any byte count >= 1 (else std::invalid_argument)
Circuit compile_aes_ctr_circuit(size_t message_len, size_t key_bits = 128, size_t key_tag_blocks = 0, int digest_kind = 0, uint64_t digest_prefix = 0, int reveal = 0);
// AES-128-GCM (SP 800-38D, 96-bit IV, full tag; DESIGN.md "GCM"): public = iv (12 bytes), aad (aad_len bytes), ciphertext (message_len bytes), tag (16 bytes), private =
// message and key.  The trace holds nb + 2 AES blocks (the message blocks under iv || be32(b + 2), H = AES_K(0), AES_K(iv || 1)), the V table of H and, per GHASH block,
// one multiplication by H as 16,384 and gates and 128 parity rows.  message_len >= 1, aad_len >= 0; both are fixed by the key (else std::invalid_argument)
Circuit compile_aes_gcm_circuit(size_t message_len, size_t aad_len, size_t key_bits = 128, size_t key_tag_blocks = 0, int digest_kind = 0, uint64_t digest_prefix = 0, int reveal = 0);
// One segment of a GCM record longer than one proof.  role = 0 head, 1 mid, 2 tail; units = c, the data blocks of a head or mid segment, or Lt, the
// 1 .. 16 c bytes of a tail; aad_len = the record's whole aad (head only, else 0).  Public input, in order: iv (12 bytes), ctr0 (4, big-endian: the counter of the
// segment's first data block), head: aad, ciphertext, com_out (32); mid: ciphertext, com_in, com_out; tail: ciphertext, the length block be64(8 A) || be64(8 L) of the
// whole record (16), tag (16), com_in.  Private: message, key, Y_in (the GHASH accumulator entering a mid or tail), the salts.  A commitment is ONE SHA-256 compression
// from the initial value over key || zeros to 32 bytes || Y || salt.  Block b runs under iv || (ctr0 + b mod 2^32), by CTR's xor/and incrementer over the low 32 bits.
// No digest.  reveal = 1 appends, behind everything above, the segment's slice of the record's mask (ceil(len / 8) bytes) and of its
// revealed bytes (len), len = 16 c for a head or mid and Lt for a tail, with the rows of the lone reveal form; reveal = 0 is the circuit as it was.
// key_tag_blocks = T in 1, 2 (a HEAD only, since the commitments carry the key to every later segment) appends 9e's tag blocks: 128 T inputs behind
// com_out and ahead of the reveal inputs, their slots at TRK_KT(TRS_BYTES(..)); T = 0 is the circuit as it was.  Anything out of range is std::invalid_argument
// digest = 1: a segment of a DIGEST record, which is nd data segments and one closing tail.  A head or mid (16 units a multiple of 64) appends 512 inputs
// H_in, H_out: the chain digest over its 16 units bytes.  role 3, "last" (with the flag only): a mid whose units are Lr = 1 .. 65536 BYTES -- Y_in, com_in, com_out, no
// tag, the final block zero-padded for GHASH -- which appends H_in, H_out and the 64 inputs total_bits (8 bytes, big-endian): the final digest over its Lr bytes with
// the padding 0x80, zeros, total_bits in ceil((Lr + 9) / 64) compressions.  A tail takes units = 0 only: no data, no digest; iv, ctr0, the length block, the tag, com_in.
// digest with reveal or key_tag_blocks, a head or mid whose 16 units is no multiple of 64, and a tail with units != 0 are std::invalid_argument; digest = 0 is the
// circuit as it was, role 3 and a tail of 0 bytes refused
Circuit compile_aes_gcm_segment_circuit(int role, size_t units, size_t aad_len = 0, size_t key_bits = 128, int reveal = 0, size_t key_tag_blocks = 0, int digest = 0);
// kind = CIRCUIT_AES, CIRCUIT_AES_CBC, CIRCUIT_AES_CTR, CIRCUIT_AES_GCM, or an ops kind (message_len ignored); aad_len must be 0 for every kind but GCM, key_bits
// 128, key_tag_blocks 0 and digest_kind 0 for the ops kinds
Circuit compile_circuit(int kind, size_t message_len, size_t aad_len = 0, size_t key_bits = 128, size_t key_tag_blocks = 0, int digest_kind = 0, uint64_t digest_prefix = 0, int reveal = 0);
// SHA-256 on the host (FIPS 180-4), for the verifier and the prover's chaining alike.  A state is 32 bytes, the eight words in big-endian serialisation; h_in = nullptr is
// the initial value.  sha256_chain: h_out = the compressions of data's len / 64 blocks from h_in, no padding; len must be a multiple of 64 (else std::invalid_argument).
// sha256_finish: digest = the chain from h_in over tail || 0x80 || zeros || be64(8 (prefix_bytes + tail_len)); prefix_bytes a multiple of 64, prefix_bytes + tail_len < 2^61
void sha256_chain(const uint8_t *h_in, const uint8_t *data, size_t len, uint8_t h_out[32]);
void sha256_finish(const uint8_t *h_in, uint64_t prefix_bytes, const uint8_t *tail, size_t tail_len, uint8_t digest[32]);
// the bytes of the per-proof public header a key's mode takes ahead of a digest key's H_in: 0 (ECB), 16 (CBC, CTR), 12 + aad_bytes (GCM); for a GCM segment key the
// 80 + aad_bytes of a segment header (trace_layout.h TRS_HDR_*), which also carries that proof's witnesses Y_in and the salts (a reveal segment key's mask follows it)
size_t mode_header_bytes(const Circuit &c);
// the whole per-proof header of a GCM segment key (trace_layout.h TRS_HDR_*): mode_header_bytes, then for a digest segment key H_in (32) and for a last be64(total_bits)
// padded to 16, then a reveal key's mask
size_t segment_header_bytes(const Circuit &c);
// the ceil(message_bytes / 8) mask bytes a reveal key's per-proof header carries behind H_in, 0 for every other key
size_t reveal_mask_bytes(const Circuit &c);
// the key tag itself on the host: out = 16 tag_blocks bytes, AES_K(D_0) (|| AES_K(D_1)); key_len = 16, 24 or 32, tag_blocks = 1 or 2 (else std::invalid_argument)
void aes_key_tag_host(const uint8_t *key, size_t key_len, size_t tag_blocks, uint8_t *out);
// D_t, the constant block behind tag block t
void aes_key_tag_block(size_t t, uint8_t out[16]);
uint8_t aes_sbox_value(uint8_t x);   // the lookup table of src/aes_circuit.rs:433-694
// plain byte-wise AES-128-CBC over aes_sbox_value, host only: out = len bytes, len a multiple of 16
// (the host ciphers keep their names; key_len = 16, 24 or 32 bytes selects AES-128, -192 or -256, anything else is std::invalid_argument)
void aes128_cbc_encrypt_host(const uint8_t *msg, size_t len, const uint8_t *key, const uint8_t iv[16], uint8_t *out, size_t key_len = 16);
// plain AES-ECB of whole blocks on the host
void aes_ecb_encrypt_host(const uint8_t *msg, size_t len, const uint8_t *key, size_t key_len, uint8_t *out);
// AES-128-CTR on the host, encryption and decryption alike: out = len bytes (any len), block b under the counter icb + b
void aes128_ctr_crypt_host(const uint8_t *in, size_t len, const uint8_t *key, const uint8_t icb[16], uint8_t *out, size_t key_len = 16);
// out = counter + n mod 2^128, the 16 bytes read as one big-endian integer (out may alias counter)
void ctr_counter_add(const uint8_t counter[16], uint64_t n, uint8_t out[16]);
// AES-128-GCM encryption on the host (SP 800-38D 7.1 with a 96-bit IV): ct = len bytes (any len >= 0), tag = 16 bytes; GHASH by Algorithm 1, bit by bit
void aes128_gcm_encrypt_host(const uint8_t *msg, size_t len, const uint8_t *key, const uint8_t iv[12], const uint8_t *aad, size_t aad_len, uint8_t *ct, uint8_t tag[16], size_t key_len = 16);
// GCM segments on the host.  gcm_boundaries_host: ys = 16 (n - 1) bytes, Y_s = the GHASH accumulator of the record after the last data block of segment
// s < n - 1, n = ceil(len / (16 c)) segments of c data blocks; len >= 1, c >= 1.  gcm_commit_host: com = the one SHA-256 compression from the initial value over
// key || zeros to 32 bytes || y || salt
void gcm_boundaries_host(const uint8_t *msg, size_t len, const uint8_t *key, size_t key_len, const uint8_t iv[12], const uint8_t *aad, size_t aad_len, size_t c, uint8_t *ys);
void gcm_commit_host(const uint8_t *key, size_t key_len, const uint8_t y[16], const uint8_t salt[16], uint8_t com[32]);
// a DIGEST record's host side: nd = ceil(len / (16 c)) >= 2 data segments of c data blocks, c a multiple of 4.  ys = 16 nd bytes: the nd - 1 accumulators
// of gcm_boundaries_host and, last, the one behind the record's last data block, ahead of the length block -- what enters the closing tail.  states = 32 (nd + 1) bytes:
// states[0] = h_in (nullptr = the initial value), states[s + 1] = the chain over segment s, states[nd] = the real digest of prefix || msg, prefix a multiple of 64
void gcm_digest_plan_host(const uint8_t *msg, size_t len, const uint8_t *key, size_t key_len, const uint8_t iv[12], const uint8_t *aad, size_t aad_len, size_t c, const uint8_t *h_in, uint64_t prefix,
                          uint8_t *ys, uint8_t *states);

}  // namespace zk
