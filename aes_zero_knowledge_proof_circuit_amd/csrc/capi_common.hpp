// csrc/capi_common.hpp -- what the two halves of the extern "C" boundary share: the handle structs, the thread-local error slot, the exception guard.
// capi_host.cpp holds the host-only entry points (verifier, (de)serialisation, circuit queries: no device, also built under sanitizers / libFuzzer);
// capi.cpp the ones that need a GPU; capi_kernels.hip the kernel-level ones.
#pragma once
#include "../../include/zkaes.h"
#include <cstdlib>
#include <cstring>
#include <exception>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>
#include "marlin.hpp"
#include "verify_batch.hpp"

struct zkaes_pk { std::unique_ptr<zk::ProvingKey> pk; };
struct zkaes_vk { zk::VerifyingKey vk; };

namespace zk {
void capi_set_error(const std::string &m);       // the calling thread's zkaes_last_error() message (defined in capi_host.cpp)
namespace capi {
template <class Fn> int guard(Fn &&fn) {
    try { capi_set_error(""); fn(); return 0; }
    catch (const std::exception &e) { capi_set_error(e.what()); return 1; }
    catch (...) { capi_set_error("unknown error"); return 1; }
}
inline uint8_t *give(const std::vector<uint8_t> &v) {
    uint8_t *p = (uint8_t *)malloc(v.size() ? v.size() : 1);
    if (!p) throw std::bad_alloc();
    if (!v.empty()) memcpy(p, v.data(), v.size());
    return p;
}
inline void fill_info(const Circuit &c, uint64_t out[12]) {
    out[0] = c.raw_constraints; out[1] = c.raw_instance; out[2] = c.raw_witness;
    out[3] = c.A.nnz(); out[4] = c.B.nnz(); out[5] = c.C.nnz();
    out[6] = c.num_constraints; out[7] = c.num_instance; out[8] = c.num_witness; out[9] = 0; out[10] = 0; out[11] = 0;
}
// zkaes_verify_batch and zkaes_verify_batch_gpu: the same call over the two back ends (verify_batch.hpp)
void set_last_batch_timings(const BatchTimings &t);      // the calling thread's zkaes_verify_batch_timings() (capi_host.cpp)
inline void verify_batch_call(const zkaes_vk *vk, const uint8_t *proofs, const size_t *proof_lens, size_t n, const uint8_t *bits, size_t n_bits, int *accepted_each, size_t *n_accepted,
                              BatchBackend &be) {
    if (n_accepted) *n_accepted = 0;
    if (accepted_each) for (size_t i = 0; i < n; i++) accepted_each[i] = 0;
    if (!vk || !proofs || !proof_lens || (n_bits && !bits)) throw std::invalid_argument("null argument");
    if (n == 0) throw std::invalid_argument("verify_batch: at least one proof");
    if (n_bits >= ((size_t)1 << 46)) throw std::invalid_argument("verify_batch: n_bits out of range");
    BatchTimings t;
    std::vector<uint8_t> acc = verify_batch(vk->vk, proofs, proof_lens, n, bits, n_bits, be, &t);
    set_last_batch_timings(t);
    size_t ok = 0;
    for (size_t i = 0; i < n; i++) { if (accepted_each) accepted_each[i] = acc[i]; ok += acc[i]; }
    if (n_accepted) *n_accepted = ok;
}
// zkaes_verify_batch_keys and zkaes_verify_batch_keys_gpu: the same call over the two back ends
inline void verify_batch_keys_call(const zkaes_vk *const *vks, size_t n_keys, const uint32_t *key_of, const uint8_t *proofs, const size_t *proof_lens, size_t n, const uint8_t *bits,
                                   const size_t *n_bits_each, int *accepted_each, size_t *n_accepted, BatchBackend &be) {
    if (n_accepted) *n_accepted = 0;
    if (accepted_each) for (size_t i = 0; i < n; i++) accepted_each[i] = 0;
    if (n_keys == 0) throw std::invalid_argument("verify_batch_keys: at least one verifying key");
    if (!vks || !key_of || !proofs || !proof_lens || !n_bits_each) throw std::invalid_argument("null argument");
    if (n == 0) throw std::invalid_argument("verify_batch_keys: at least one proof");
    std::vector<const VerifyingKey *> keys(n_keys);
    for (size_t k = 0; k < n_keys; k++) { if (!vks[k]) throw std::invalid_argument("null argument"); keys[k] = &vks[k]->vk; }
    size_t total = 0;
    for (size_t i = 0; i < n; i++) {
        if (n_bits_each[i] >= ((size_t)1 << 46) || total + n_bits_each[i] >= ((size_t)1 << 46)) throw std::invalid_argument("verify_batch_keys: n_bits out of range");
        total += n_bits_each[i];
    }
    if (total && !bits) throw std::invalid_argument("null argument");
    BatchTimings t;
    std::vector<uint8_t> acc = verify_batch_keys(keys.data(), n_keys, key_of, proofs, proof_lens, n, bits, n_bits_each, be, &t);
    set_last_batch_timings(t);
    size_t ok = 0;
    for (size_t i = 0; i < n; i++) { if (accepted_each) accepted_each[i] = acc[i]; ok += acc[i]; }
    if (n_accepted) *n_accepted = ok;
}
// zkaes_verify_gcm_segments_batch and _batch_gpu: the argument checks and rows of zkaes_verify_gcm_segments[_reveal], the proofs through verify_batch_keys (capi_host.cpp)
void verify_gcm_segments_batch_call(const char *entry, const zkaes_vk *head, const zkaes_vk *mid_or_null, const zkaes_vk *tail, const uint8_t *proofs, const size_t *proof_lens, size_t n_segments,
                                    size_t c, const uint8_t iv[12], const uint8_t *aad, size_t aad_len, const uint8_t *ct, size_t ct_len, const uint8_t tag[16], const uint8_t *commitments,
                                    size_t commitments_len, const uint8_t *mask, size_t mask_len, const uint8_t *revealed, size_t revealed_len, int *accepted_each, size_t *n_accepted,
                                    BatchBackend &be, const uint8_t *key_tag = nullptr, size_t key_tag_len = 0);      // (a key tag, DESIGN.md 9l: the head's row ends in its bits ahead of the mask)
inline size_t next_pow2(size_t n) { if (n > ((size_t)1 << 62)) throw std::length_error("size out of range"); size_t p = 1; while (p < n) p <<= 1; return p; }
}  // namespace capi
}  // namespace zk
