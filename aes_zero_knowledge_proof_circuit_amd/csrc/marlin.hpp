// csrc/marlin.hpp -- Marlin (AHP for R1CS + MarlinKZG10) keys, GPU prover and CPU verifier of libzkaes.
//
// Mirrors what the reference reaches through simpleworks::marlin (not under /root/reference; restated from the published
// ark-marlin 0.3.0 / ark-poly-commit 0.3.0 algorithms):
//   synthesize_keys  -> generate_universal_srs + generate_proving_and_verifying_keys   (/root/reference/src/lib.rs:138-174)
//   prove            -> generate_proof                                                 (src/lib.rs:60-114)
//   verify           -> verify_proof                                                   (src/lib.rs:116-136)
// The prover's polynomial work (witness, SpMV, NTTs, MSMs, divisions, evaluations) runs on the GPU; the Fiat-Shamir
// transcript, the <=3-term hiding MSMs and the final window sums stay on the host.  The verifier is host-only.
#pragma once
#include <cstdint>
#include <memory>
#include <string>
#include <vector>
#include "circuit.hpp"
#include "ec.cuh"
#include "pairing.hpp"

namespace zk {

using Fr = Fr377;
using G1A = Affine<Fq377>;

struct Commitment { G1A comm = G1A::inf(); bool has_shifted = false; G1A shifted = G1A::inf(); };

struct Proof {
    Commitment comms[9];   // w z_a z_b mask_poly | t g_1 h_1 | g_2 h_2
    Fr evals[4];           // g_1(beta) g_2(gamma) t(beta) z_b(beta)   (sorted by label)
    G1A w_beta, w_gamma;   // pc_proof.proof[0].w, [1].w
    Fr random_v_beta;      // pc_proof.proof[0].random_v = Some(..); [1].random_v = None
};
// ark-serialize 0.3 compressed layout of ark_marlin::Proof
std::vector<uint8_t> serialize_proof(const Proof &p);
// throws std::runtime_error on malformed input
Proof deserialize_proof(const uint8_t *bytes, size_t len);

struct SrsLiterals { size_t num_constraints = 866944, num_variables = 513, num_non_zero = 4062064; };   // src/lib.rs:141

struct VerifyingKey {
    uint64_t num_variables = 0, num_constraints = 0, num_non_zero = 0, num_instance = 0;   // IndexInfo (padded)
    size_t num_public_inputs = 0;     // unpadded instance count minus One (128 per block)
    G1A index_comms[6];               // row col a_val b_val c_val row_col
    G1A g, gamma_g;
    pairing::G2Affine h, beta_h;
    size_t degree_bounds[2] = {0, 0}; // |H|-2, |K|-2 sorted ascending
    G1A shift_powers[2];              // powers_of_g[max_degree - bound]
    size_t supported_degree = 0, max_degree = 0;
};

// the four draws of KZG10::setup from ark_std::test_rng(): trapdoor beta, base points g, gamma_g (G1) and h (G2)
void kzg_setup_points(Fr &beta, G1A &g, G1A &gamma_g, pairing::G2Affine &h);
// ark-serialize 0.3 compressed layout of ark_marlin::IndexVerifierKey (what a Rust caller gets from CanonicalSerialize::serialize)
// uncompressed = the serialize_uncompressed image (G1 96 B, G2 192 B): what deserialize_unchecked reads
std::vector<uint8_t> serialize_vk_ark(const VerifyingKey &vk, bool uncompressed = false);
VerifyingKey deserialize_vk_ark(const uint8_t *bytes, size_t len);

struct ProverTimings { double witness_ms = 0, round1_ms = 0, round2_ms = 0, round3_ms = 0, open_ms = 0, total_ms = 0; };

class ProvingKeyImpl;
class ProvingKey {
  public:
    ~ProvingKey();
    const VerifyingKey &vk() const;
    const Circuit &circuit() const;
    // the byte length of the AES key this proving key was synthesized for: 16, 24 or 32.  EVERY `key` argument below -- written key[16] from when 16 was the only size --
    // points to key_bytes() bytes, and the batch calls take n x key_bytes() key bytes
    size_t key_bytes() const;
    // T = 0, 1 or 2: the key-tag blocks this key was synthesized with.  Every proving and witness call below takes a tagged key as it is: the last 128 T
    // public-input bits of each proof are AES_K(D_0) (, AES_K(D_1)) for that proof's key, filled from the trace like every other column
    size_t key_tag_blocks() const;
    // ---- The four shapes of call, for every AES mode (statement.hpp).  kind: the mode the caller's entry point is for -- CIRCUIT_AES (ECB), _CBC, _CTR, _GCM; a key of
    // another kind is refused -- or ANY_AES_KIND.  hdr: the mode's public header, mode_header_bytes(circuit()) bytes: nothing (ECB, null), the iv (CBC), the initial
    // counter block (CTR), iv (12 bytes) then aad (GCM); headers: n of them.  aad_len: what the caller's aad argument holds, checked against the key's, or KEY_AAD.  len:
    // the key's message length (CTR and GCM: any value >= 1 the key was synthesized for).  digest: the caller is a _digest_ entry: the key must carry a
    // digest, h_in(s) are 32-byte SHA-256 states (null: the initial value) and every proof states (H_in, H_out) behind its key tag; every other caller passes false and a
    // digest key is refused, for its proofs carry two states the caller has no argument for.  A key with key-tag blocks is taken as it is.
    // mask(s): the caller is a _reveal_ entry: the key must have been synthesized with reveal = 1, and every proof states (mask, revealed) last of all; a
    // witness or batch mask is ceil(L / 8) bytes per proof, a chunked job's ONE mask of ceil(len / 8) bytes over the whole job, chunk j proven under its slice
    // (statement.hpp); a bit at or beyond the length is std::invalid_argument.  Every caller without a mask is refused a reveal key.  revealed_or_null receives
    // reveal_bytes(message, mask) per proof (n x L) or for the whole job (len)
    // zk_seed of a lone proof: a 32-byte StdRng seed, or nullptr for ark_std::test_rng()'s (what simpleworks::marlin::generate_rand() returns).  zk_seed of a batch or a
    // chunked job: proof i draws from StdRng(Blake2s(seed || (index_offset + i) as u64 LE)), so callers that split one job over several calls / ranks pass the job-global
    // index of their first proof and reuse one seed; nullptr = the reference's fixed test_rng seed for EVERY proof (byte-parity mode for tests; NOT zero-knowledge across
    // proofs).  n_contexts proofs are in flight on separate HIP streams.
    // The host computes the ciphertext (GCM: and the tag, 16 bytes) by plain AES where a buffer is given, and H_out by plain SHA-256; the device is handed message, key,
    // header and H_in only and derives the rest, so the two meet in the constraints
    enum : int { ANY_AES_KIND = -1 };
    static constexpr size_t KEY_AAD = ~(size_t)0;
    // witness generation only (the trace kernels + witness_expand): z = padded instance || witness, one byte per variable
    std::vector<uint8_t> witness(int kind, bool digest, const uint8_t *message, size_t len, const uint8_t *key, const uint8_t *hdr, size_t aad_len = KEY_AAD, const uint8_t *h_in_or_null = nullptr,
                                 const uint8_t *mask_or_null = nullptr);
    // one proof on context 0 (keys without a digest: a lone digest proof is a batch of one)
    Proof prove_lone(int kind, const uint8_t *message, size_t len, const uint8_t *key, const uint8_t *hdr, size_t aad_len, const uint8_t *zk_seed, uint8_t *ciphertext_or_null = nullptr,
                     uint8_t *tag_or_null = nullptr);
    // n independent statements: messages n x L, keys n x key_bytes(), headers n x the mode's header (null for ECB), h_ins n x 32 or null.  Receives on request the
    // ciphertexts (n x L), GCM tags (n x 16, GCM keys only) and every proof's H_out (n x 32, digest keys only)
    std::vector<Proof> prove_batch(int kind, bool digest, const uint8_t *messages, const uint8_t *keys, const uint8_t *headers, const uint8_t *h_ins_or_null, size_t n, size_t n_contexts,
                                   const uint8_t *zk_seed = nullptr, uint64_t index_offset = 0, uint8_t *ciphertexts_or_null = nullptr, uint8_t *tags_or_null = nullptr,
                                   uint8_t *h_outs_or_null = nullptr, const uint8_t *masks_or_null = nullptr, uint8_t *revealed_or_null = nullptr);
    // len / L chunk-proofs of one ECB, CBC or CTR message under one key.  hdr = the header entering this call's first chunk; chunk j is proven under chunk_mode_header(j):
    // the public chaining value entering it (CBC), hdr + j x the key's blocks (CTR: a key for whole blocks; a job split over calls passes ctr_counter_add(icb, blocks
    // before)).  Over a chain key it is also proven under (states[j], states[j + 1]), states[0] = h_in; states_or_null receives the n + 1 states, ciphertext_or_null len bytes
    std::vector<Proof> prove_chunked(int kind, bool digest, const uint8_t *message, size_t len, const uint8_t *key, const uint8_t *hdr, const uint8_t *h_in_or_null, size_t n_contexts,
                                     const uint8_t *zk_seed = nullptr, uint64_t index_offset = 0, uint8_t *ciphertext_or_null = nullptr, uint8_t *states_or_null = nullptr,
                                     const uint8_t *mask_or_null = nullptr, uint8_t *revealed_or_null = nullptr);
    Proof prove_ops(uint32_t x, uint32_t y, const uint8_t *zk_seed);
    // ---- GCM segments (keys of kind CIRCUIT_AES_GCM_SEG only, from synthesize_keys_gcm_segment; every call above refuses such a key, and the GCM calls name the segment
    // entries).  header = the segment proof's TRS_HDR_BYTES(A) bytes (trace_layout.h): iv, ctr0, Y_in, salt_in, salt_out, the length block, the aad
    // A key synthesized with reveal = 1 takes, beside the header, the segment's mask of ceil(len / 8) bytes -- its slice of the record's -- and is refused
    // without one; a key with reveal = 0 is refused with one.  masks: n x ceil(len / 8); revealed_or_null receives reveal_bytes(message, mask) per proof (n x len)
    std::vector<uint8_t> aes_witness_gcm_segment(const uint8_t *message, size_t len, const uint8_t *key, const uint8_t *header, size_t header_len, const uint8_t *mask_or_null = nullptr,
                                                 size_t mask_len = 0);
    // n independent segment proofs of this key's role, each under its own header (n x TRS_HDR_BYTES(A)), all contexts side by side; seeds as prove_batch.  The
    // caller answers for what the headers say: prove_gcm_segments below derives them from one record
    std::vector<Proof> prove_gcm_segment_batch(const uint8_t *messages, const uint8_t *keys, const uint8_t *headers, size_t n, size_t n_contexts, const uint8_t *zk_seed = nullptr,
                                               uint64_t index_offset = 0, const uint8_t *masks_or_null = nullptr, uint8_t *revealed_or_null = nullptr);
    // the same for a segment key of a DIGEST record (from synthesize_keys_gcm_segment with digest = 1, which every call above but the witness refuses,
    // as this one refuses every other key): headers = n x TRS_HDR_DG_BYTES(A, kind) bytes, the plain segment header, then H_in (head, mid, last), then a last's
    // be64(total_bits) padded to 16.  The closing tail has no message: messages may be null for it
    std::vector<Proof> prove_gcm_segment_digest_batch(const uint8_t *messages, const uint8_t *keys, const uint8_t *headers, size_t n, size_t n_contexts, const uint8_t *zk_seed = nullptr,
                                                      uint64_t index_offset = 0);
    const ProverTimings &last_timings() const;
    // one proof with the op recorder open: JSON of the transforms and MSMs the library actually launched (marlin.cpp; SURVEY.md 8d op lists)
    std::string op_lists_json(const uint8_t *message, size_t len, const uint8_t key[16], bool throughput_path);
    // test / parity hooks: copy an intermediate of the last proof to the host. names: "z" (bytes), "z_a_evals","z_b_evals",
    // polys "w","z_a","z_b","mask_poly","t","g_1","h_1","g_2","h_2" (Montgomery Fr), index "row","col","a_val","b_val","c_val","row_col"
    std::vector<uint8_t> debug_fetch(const std::string &name) const;
    // were the fixed-base window tables of the SRS built (they are skipped under KEY_NO_TABLES or when device memory is short)?  *bytes = their size
    bool tables_built(uint64_t *bytes = nullptr) const;
    // the universal SRS behind this key (one per process, device and SRS literals; shared by every key over it): out = {max_degree, points per copy, copies (1 = no
    // window tables), device bytes, keys sharing it now, bytes of the Lagrange-basis points (shared per |H|, |X|)}; secs = {seconds this key's synthesis spent BUILDING
    // the SRS (0 when it was shared), seconds of the whole synthesis}
    void srs_info(uint64_t out[6], double secs[2]) const;
    // proofs in flight per multi-proof call on this key (prove_chunked, prove_batch with n_contexts = contexts()); 0 restores the process default
    size_t contexts() const;
    void set_contexts(size_t n);
    // ark-serialize image of the arkworks IndexProverKey this key corresponds to, streamed to `path`; returns the bytes written (marlin.cpp has the layout).
    // compressed (48-byte points): what IndexProverKey::serialize writes and ::deserialize reads (square root + subgroup check per point on the Rust side);
    // uncompressed (96-byte points): serialize_uncompressed's image, read by ::deserialize_uncompressed or -- without any check -- ::deserialize_unchecked
    uint64_t serialize_ark_to_file(const std::string &path, bool uncompressed = false) const;
    // ONE commitment-sized MSM sharded by point range over ranks, on the prover's own path (the key's SRS on the twisted Edwards model, window tables, one bucket set):
    // sum_i scalars[i] * powers_of_g[offset + i], i < n_local (scalars: host, n_local x 32 B Montgomery Fr), left as ONE XYZZ point (192 B) in device memory at dev_out
    // -- the rank's row of the all-gather; gpu::msm_fold_points_device adds the ranks' rows.  Needs a key with tables.
    void msm_powers_partial_device(const uint8_t *scalars, size_t n_local, size_t offset, void *dev_out);
    ProvingKeyImpl *impl;
};

// universal_setup(literals) + index; GPU required.  flags: KEY_NO_TABLES = do not build the fixed-base window tables of the SRS (13 copies, 10-42 GB per key):
// multi-proof calls then run 15 per-window-bucket windows instead of 13 table windows (~9 % fewer blocks/s), and the key fits a GPU that is short of memory.
// Without the flag the tables are built when memory allows (hipMemGetInfo) and silently skipped otherwise.
enum : unsigned { KEY_NO_TABLES = 1u };
std::unique_ptr<ProvingKey> synthesize_keys(int circuit_kind, size_t message_len, const SrsLiterals &srs, unsigned flags = 0, size_t aad_len = 0, size_t key_bits = 128,
                                            size_t key_tag_blocks = 0, int digest_kind = 0, uint64_t digest_prefix = 0, int reveal = 0);      // (aad_len: GCM keys only; key_bits: 128, 192 or 256, key_tag_blocks: 0, 1 or 2, digest_kind: 0, 1 or 2 (circuit.hpp DigestKind), reveal: 0 or 1, the AES kinds only)
// A GCM segment key: role = 0 head, 1 mid, 2 tail; units = c data blocks (head, mid) or Lt bytes (tail); aad_len: head only.  No digest;
// reveal: 0 or 1; key_tag_blocks: 0, 1 or 2 for a head, 0 for a mid or tail
std::unique_ptr<ProvingKey> synthesize_keys_gcm_segment(int role, size_t units, size_t aad_len, size_t key_bits, const SrsLiterals &srs, unsigned flags = 0, int reveal = 0,
                                                        size_t key_tag_blocks = 0, int digest = 0);      // (digest = 1: a segment of a digest record, DESIGN.md 9m: role 3 = last, a tail takes units = 0, no reveal and no key tag)
// Segments [first_segment, first_segment + count) of ONE GCM record of len bytes as segment-proofs: n = ceil(ceil(len / 16) / c) >= 2 segments, c = the head key's data
// blocks; mid_or_null may be null when n = 2; the tail key is the one for the record's last len - 16 c (n - 1) bytes.  The host computes the record's ciphertext and tag,
// Y at every boundary and the n - 1 commitments from salts_or_null (16 (n - 1) bytes; null = fresh OS randomness, allowed only when the call covers the whole record);
// the device is handed key, iv, aad, message, ctr0, Y_in, the salts and the length block.  Segment s draws from StdRng(Blake2s(zk_seed || s)) whichever call proves it
// (nullptr = the fixed test stream, as prove_batch); the middle segments run side by side over the mid key's contexts.  Receives on request the whole record's
// ciphertext (len), tag (16) and commitments (32 (n - 1)).  mask_or_null: ONE mask of ceil(len / 8) bytes over the whole record; the three keys must then
// be reveal keys (and must not be without it), segment s is proven under chunk_mask_slice(mask, s, 16 c), a bit at or beyond len is std::invalid_argument and
// revealed_or_null receives reveal_bytes(message, mask) for the whole record (len), whichever segments the call proves
std::vector<Proof> prove_gcm_segments(ProvingKey *head, ProvingKey *mid_or_null, ProvingKey *tail, const uint8_t *message, size_t len, const uint8_t *key, const uint8_t iv[12], const uint8_t *aad,
                                      size_t aad_len, const uint8_t *salts_or_null, size_t first_segment, size_t count, const uint8_t *zk_seed, uint8_t *ciphertext_or_null = nullptr,
                                      uint8_t *tag_or_null = nullptr, uint8_t *commitments_or_null = nullptr, const uint8_t *mask_or_null = nullptr, uint8_t *revealed_or_null = nullptr);
// Proofs [first_segment, first_segment + count) of ONE GCM DIGEST record of len > 16 c bytes: nd = ceil(len / (16 c)) data segments -- head, nd - 2 mids,
// the last with len - 16 c (nd - 1) bytes -- and, as proof nd, the closing tail: nd + 1 proofs, mid_or_null may be null when nd = 2.  The host computes ciphertext, tag, Y
// behind every data segment, the nd commitments (salts_or_null: 16 nd bytes, as above) and the nd + 1 states of plain SHA-256 from h_in_or_null (null = the initial
// value) with digest_prefix bytes hashed ahead (a multiple of 64): data segment s is proven under (states[s], states[s + 1]), the last with total_bits =
// 8 (digest_prefix + len), and states[nd] is the digest of prefix || message.  Proof s draws at index s.  Receives on request ciphertext (len), tag (16), commitments
// (32 nd) and states (32 (nd + 1))
std::vector<Proof> prove_gcm_segments_digest(ProvingKey *head, ProvingKey *mid_or_null, ProvingKey *last, ProvingKey *tail, const uint8_t *message, size_t len, const uint8_t *key, const uint8_t iv[12],
                                             const uint8_t *aad, size_t aad_len, const uint8_t *salts_or_null, const uint8_t *h_in_or_null, uint64_t digest_prefix, size_t first_segment, size_t count,
                                             const uint8_t *zk_seed, uint8_t *ciphertext_or_null = nullptr, uint8_t *tag_or_null = nullptr, uint8_t *commitments_or_null = nullptr,
                                             uint8_t *states_or_null = nullptr);
// hold = true: every universal / Lagrange SRS built (or alive) from now on stays resident after its last key is freed; false: back to "freed with the last key"
void srs_hold(bool hold);
// process default of ProvingKey::contexts(): ZKAES_CONTEXTS from the environment (read once), else ZKAES_DEFAULT_CONTEXTS
size_t default_contexts();
void set_default_contexts(size_t n);       // 0 = back to the environment / built-in default; at most 64
// 32 bytes from the operating system (getrandom): the default zero-knowledge seed of the multi-proof entry points
void os_random_seed(uint8_t out[32]);

// public_input: the instance values WITHOUT the leading One (0/1 as field elements), e.g. ciphertext bits LSB-first per byte
bool verify(const VerifyingKey &vk, const std::vector<Fr> &public_input, const Proof &proof);
std::vector<Fr> ciphertext_to_public_input(const uint8_t *ct, size_t len);   // src/helpers/mod.rs:84-93 per byte

}  // namespace zk
