// csrc/verify_batch.hpp -- the batch verifier: n proofs under ONE verifying key, each with its own public input, one product of two pairings;
// and (9k) n proofs under several keys of one setup, still one product of two pairings.
// Host-only header: the protocol (parse, transcripts, scalar rows, randomizers, bisection, pairing) lives in marlin_codec.cpp and reaches the elliptic-curve work
// through BatchBackend -- the host implementation in the same file, the device one (kernels_verify.hip + the variable-base MSM) in marlin.cpp.
#pragma once
#include <cstddef>
#include <cstdint>
#include <memory>
#include <vector>
#include "marlin.hpp"

namespace zk {

constexpr size_t VB_OWN = 13;        // bases a proof brings: w z_a z_b mask_poly t g_1 g_1.shifted h_1 g_2 g_2.shifted h_2 W_beta W_gamma
constexpr size_t VB_SHARED = 10;     // bases of the key: the 6 index commitments, the 2 shift powers, g, gamma_g

// one compressed G1 point as parsed from the bytes: canonical x limbs and the sign flag
struct G1Compressed { uint32_t x[12]; uint8_t y_gt; };

struct BatchTimings { double parse_ms = 0, decompress_ms = 0, transcripts_ms = 0, xhat_ms = 0, msm_ms = 0, pairing_ms = 0, total_ms = 0; uint64_t sub_batches = 0; };

struct BatchBackend {
    virtual ~BatchBackend() {}
    // out[i], status[i] (fq_sqrt.cuh G1_OK / G1_NOT_ON_CURVE / G1_NOT_IN_SUBGROUP) for every point
    virtual void decompress(const G1Compressed *pts, size_t n, G1A *out, uint8_t *status) = 0;
    // out[i] = x^(beta_i) = sum_j L_j(beta_i) x_ij over the domain X of size 2^lg_m, x_i = [1, bits of row i (n_bits 0/1 bytes), zero padding]
    virtual void public_input_eval(int lg_m, const Fr *betas, const uint8_t *bits, size_t n, size_t n_bits, Fr *out) = 0;
    // the bases of one batch: np proofs' own points (VB_OWN each, proof-major), then the key's VB_SHARED.  Called once, ahead of every msm_*
    virtual void set_bases(const G1A *own, size_t np, const G1A *shared) = 0;
    // sum over proofs lo <= i < hi of own_scalars[i][.] * own[i][.]  +  sum of shared_scalars[.] * shared[.]
    virtual XYZZ<Fq377> msm_main(const Fr *own_scalars, size_t lo, size_t hi, const Fr *shared_scalars) = 0;
    // sum over proofs lo <= i < hi of w_scalars[i][0] * W_beta(i) + w_scalars[i][1] * W_gamma(i)   (128-bit scalars)
    virtual XYZZ<Fq377> msm_w(const Fr *w_scalars, size_t lo, size_t hi) = 0;
    // ---- the keyed forms: proofs of n_keys verifying keys in one batch
    // out[i] = x^(beta_i) over the domain of proof i's key: key k has |X| = 2^lg_m[k] and rows of n_bits[k] 0/1 bytes; proof i belongs to key key_of[i] and its row
    // starts at bits + row_off[i] (rows are ragged and may be empty)
    virtual void public_input_eval_keyed(const int *lg_m, const size_t *n_bits, size_t n_keys, const uint32_t *key_of, const Fr *betas, const uint8_t *bits, const size_t *row_off, size_t n,
                                         Fr *out) = 0;
    // set_bases for n_keys keys: np x VB_OWN own points, then n_keys x VB_SHARED key points (key-major).  msm_main then takes n_keys x VB_SHARED shared scalars:
    // per key the sums over the sub-batch's proofs of that key.  set_bases is this call with one key
    virtual void set_bases_keyed(const G1A *own, size_t np, const G1A *shared, size_t n_keys) = 0;
};
std::unique_ptr<BatchBackend> make_host_batch_backend();      // the HIP-free implementation: one object per call
std::unique_ptr<BatchBackend> make_device_batch_backend();    // marlin.cpp: kernels_verify.hip + the variable-base MSM; throws GpuError without a device

// public_input_bits: n rows of n_bits bytes (any non-zero byte is a One).  accepted[i] = 1 / 0.  Never throws on what the proof BYTES hold
std::vector<uint8_t> verify_batch(const VerifyingKey &vk, const uint8_t *proofs, const size_t *proof_lens, size_t n, const uint8_t *public_input_bits, size_t n_bits,
                                  BatchBackend &be, BatchTimings *timings = nullptr);

// The same over proofs of n_keys verifying keys that share one setup (g, gamma_g, h, beta_h: every key this library synthesizes does), DESIGN.md 9k: proof i is checked
// under vks[key_of[i]] against the row of n_bits_each[i] bytes that starts where the rows before it end.  One pairing product for the whole batch.  Throws
// std::invalid_argument for n_keys = 0, a key index out of range or keys of different setups; a row that does not pad to its own key's |X| rejects that proof alone
std::vector<uint8_t> verify_batch_keys(const VerifyingKey *const *vks, size_t n_keys, const uint32_t *key_of, const uint8_t *proofs, const size_t *proof_lens, size_t n,
                                       const uint8_t *public_input_bits, const size_t *n_bits_each, BatchBackend &be, BatchTimings *timings = nullptr);

// host probes of the pieces (tests): parse 48 compressed bytes; false = malformed (both flags, x >= q, infinity over a non-zero x).  *inf: the infinity encoding
bool g1_parse_compressed(const uint8_t bytes[48], G1Compressed &out, bool *inf);

}  // namespace zk
