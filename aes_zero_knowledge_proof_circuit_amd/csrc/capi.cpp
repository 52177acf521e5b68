// csrc/capi.cpp -- the entry points of include/zkaes.h that need a GPU: key synthesis, the prover, key-handle queries (host-only ones: capi_host.cpp)
#include "capi_common.hpp"
#include <algorithm>
#include "gpu.hpp"
#include "fq_sqrt.cuh"

using zk::capi::guard; using zk::capi::give; using zk::capi::fill_info; using zk::capi::next_pow2;

extern "C" {

void zkaes_pk_free(zkaes_pk *pk) { delete pk; }
int zkaes_device_count(void) { return zk::gpu::device_count(); }

static int synthesize(int kind, size_t len, size_t aad_len, size_t nc, size_t nv, size_t nnz, unsigned flags, zkaes_pk **pk, zkaes_vk **vk, size_t key_bits = 128, size_t key_tag_blocks = 0,
                      unsigned digest_kind = 0, uint64_t digest_prefix = 0) {
    return guard([&] {
        if (flags & ~(unsigned)ZKAES_KEY_NO_TABLES) throw std::invalid_argument("synthesize_keys: unknown flag bits");
        if (key_bits != 128 && key_bits != 192 && key_bits != 256) throw std::invalid_argument("synthesize_keys: key_bits must be 128, 192 or 256");
        if (key_tag_blocks > 2) throw std::invalid_argument("synthesize_keys: key_tag_blocks must be 0, 1 or 2");
        if (digest_kind > 2) throw std::invalid_argument("synthesize_keys: digest_kind must be 0 (none), 1 (chain) or 2 (final)");
        zk::SrsLiterals srs; srs.num_constraints = nc; srs.num_variables = nv; srs.num_non_zero = nnz;
        auto k = zk::synthesize_keys(kind, len, srs, (flags & ZKAES_KEY_NO_TABLES) ? (unsigned)zk::KEY_NO_TABLES : 0u, aad_len, key_bits, key_tag_blocks, (int)digest_kind, digest_prefix);
        zkaes_vk *v = new zkaes_vk{k->vk()};
        zkaes_pk *p = new zkaes_pk{std::move(k)};
        if (pk) *pk = p; else delete p;
        if (vk) *vk = v; else delete v;
    });
}
int zkaes_synthesize_keys_ex2(int kind, size_t len, size_t nc, size_t nv, size_t nnz, unsigned flags, zkaes_pk **pk, zkaes_vk **vk) {
    return synthesize(kind, len, 0, nc, nv, nnz, flags, pk, vk);
}
int zkaes_synthesize_keys_gcm(size_t len, size_t aad_len, size_t nc, size_t nv, size_t nnz, unsigned flags, zkaes_pk **pk, zkaes_vk **vk) {
    return synthesize(ZKAES_CIRCUIT_AES_GCM, len, aad_len, nc, nv, nnz, flags, pk, vk);
}
int zkaes_synthesize_keys_ks(int kind, unsigned key_bits, size_t len, size_t aad_len, size_t nc, size_t nv, size_t nnz, unsigned flags, zkaes_pk **pk, zkaes_vk **vk) {
    return synthesize(kind, len, aad_len, nc, nv, nnz, flags, pk, vk, key_bits);      // (compile_circuit refuses aad outside GCM and an ops kind with another key size)
}
int zkaes_synthesize_keys_kt(int kind, unsigned key_bits, unsigned key_tag_blocks, size_t len, size_t aad_len, size_t nc, size_t nv, size_t nnz, unsigned flags, zkaes_pk **pk, zkaes_vk **vk) {
    return synthesize(kind, len, aad_len, nc, nv, nnz, flags, pk, vk, key_bits, key_tag_blocks);
}
int zkaes_pk_key_tag_blocks(const zkaes_pk *pk, size_t *n) {
    return guard([&] {
        if (!pk || !n) throw std::invalid_argument("null argument");
        *n = pk->pk->key_tag_blocks();
    });
}
int zkaes_synthesize_keys_pd(int kind, unsigned key_bits, unsigned key_tag_blocks, unsigned digest_kind, uint64_t digest_prefix, size_t len, size_t aad_len, size_t nc, size_t nv, size_t nnz,
                             unsigned flags, zkaes_pk **pk, zkaes_vk **vk) {
    return synthesize(kind, len, aad_len, nc, nv, nnz, flags, pk, vk, key_bits, key_tag_blocks, digest_kind, digest_prefix);
}
int zkaes_pk_digest_info(const zkaes_pk *pk, uint64_t out[4]) {
    return guard([&] {
        if (!pk || !out) throw std::invalid_argument("null argument");
        const zk::Circuit &c = pk->pk->circuit();
        out[0] = (uint64_t)c.digest_kind; out[1] = c.digest_prefix; out[2] = c.digest_blocks; out[3] = c.digest_off;
    });
}
int zkaes_pk_key_bytes(const zkaes_pk *pk, size_t *n) {
    return guard([&] {
        if (!pk || !n) throw std::invalid_argument("null argument");
        *n = pk->pk->key_bytes();
    });
}
int zkaes_synthesize_keys_ex(int kind, size_t len, size_t nc, size_t nv, size_t nnz, zkaes_pk **pk, zkaes_vk **vk) {
    return zkaes_synthesize_keys_ex2(kind, len, nc, nv, nnz, 0u, pk, vk);
}
int zkaes_synthesize_keys(size_t len, zkaes_pk **pk, zkaes_vk **vk) {
    zk::SrsLiterals d;
    return zkaes_synthesize_keys_ex(ZKAES_CIRCUIT_AES, len, d.num_constraints, d.num_variables, d.num_non_zero, pk, vk);
}
int zkaes_encrypt_seeded(const uint8_t *msg, size_t len, const uint8_t key[16], const zkaes_pk *pk, const uint8_t *seed, uint8_t **proof, size_t *proof_len) {
    return guard([&] {
        if (!pk || !proof || !proof_len) throw std::invalid_argument("null argument");
        zk::Proof p = pk->pk->prove_aes(msg, len, key, seed);
        auto b = zk::serialize_proof(p);
        *proof = give(b); *proof_len = b.size();
    });
}
int zkaes_encrypt(const uint8_t *msg, size_t len, const uint8_t key[16], const zkaes_pk *pk, uint8_t **proof, size_t *proof_len) {
    return zkaes_encrypt_seeded(msg, len, key, pk, nullptr, proof, proof_len);
}
static void pack_proofs(const std::vector<zk::Proof> &ps, uint8_t **proofs, size_t *proofs_len, size_t *proof_lens) {
    std::vector<uint8_t> all;
    for (size_t i = 0; i < ps.size(); i++) {
        auto b = zk::serialize_proof(ps[i]);
        if (proof_lens) proof_lens[i] = b.size();
        all.insert(all.end(), b.begin(), b.end());
    }
    *proofs = give(all); *proofs_len = all.size();
}
// the unseeded multi-proof entry points draw a fresh seed from the OS per call.  The reference's fixed ark_std::test_rng() stream for every proof (byte parity with the
// oracle; NOT zero-knowledge across proofs) is reachable only explicitly, through the *_seeded entry points with a NULL seed -- no environment variable downgrades a caller.
int zkaes_encrypt_chunked_seeded_at(const uint8_t *msg, size_t len, const uint8_t key[16], const zkaes_pk *pk, const uint8_t *zk_seed32, uint64_t first_proof_index, uint8_t **proofs,
                                    size_t *proofs_len, size_t *proof_lens, size_t n_chunks) {
    return guard([&] {
        if (!pk || !proofs || !proofs_len || !key || (!msg && len)) throw std::invalid_argument("null argument");
        size_t chunk = pk->pk->circuit().n_blocks * 16;
        if (chunk == 0 || len % chunk || len / chunk != n_chunks) throw std::invalid_argument("message length must be n_chunks * the key's plaintext length");
        pack_proofs(pk->pk->prove_aes_chunked(msg, len, key, pk->pk->contexts(), zk_seed32, first_proof_index), proofs, proofs_len, proof_lens);
    });
}
int zkaes_encrypt_chunked_seeded(const uint8_t *msg, size_t len, const uint8_t key[16], const zkaes_pk *pk, const uint8_t *zk_seed32, uint8_t **proofs, size_t *proofs_len,
                                 size_t *proof_lens, size_t n_chunks) {
    return zkaes_encrypt_chunked_seeded_at(msg, len, key, pk, zk_seed32, 0, proofs, proofs_len, proof_lens, n_chunks);
}
int zkaes_encrypt_chunked(const uint8_t *msg, size_t len, const uint8_t key[16], const zkaes_pk *pk, uint8_t **proofs, size_t *proofs_len, size_t *proof_lens, size_t n_chunks) {
    uint8_t seed[32];
    { int rc = guard([&] { zk::os_random_seed(seed); }); if (rc) return rc; }
    return zkaes_encrypt_chunked_seeded_at(msg, len, key, pk, seed, 0, proofs, proofs_len, proof_lens, n_chunks);
}
int zkaes_encrypt_batch_seeded_at(size_t n, const uint8_t *messages, size_t messages_len, const uint8_t *secret_keys, size_t secret_keys_len, const zkaes_pk *pk,
                                  const uint8_t *zk_seed32, uint64_t first_proof_index, uint8_t **proofs, size_t *proofs_len, size_t *proof_lens) {
    return guard([&] {
        if (!pk || !proofs || !proofs_len || (n && (!messages || !secret_keys))) throw std::invalid_argument("null argument");
        size_t chunk = pk->pk->circuit().n_blocks * 16;
        if (messages_len != n * chunk) throw std::invalid_argument("messages must hold n x " + std::to_string(chunk) + " bytes (the key's plaintext length)");
        if (secret_keys_len != n * pk->pk->key_bytes()) throw std::invalid_argument("secret_keys must hold n x " + std::to_string(pk->pk->key_bytes()) + " bytes");
        pack_proofs(pk->pk->prove_aes_batch(messages, secret_keys, n, pk->pk->contexts(), zk_seed32, first_proof_index), proofs, proofs_len, proof_lens);
    });
}
int zkaes_encrypt_batch_seeded(size_t n, const uint8_t *messages, size_t messages_len, const uint8_t *secret_keys, size_t secret_keys_len, const zkaes_pk *pk,
                               const uint8_t *zk_seed32, uint8_t **proofs, size_t *proofs_len, size_t *proof_lens) {
    return zkaes_encrypt_batch_seeded_at(n, messages, messages_len, secret_keys, secret_keys_len, pk, zk_seed32, 0, proofs, proofs_len, proof_lens);
}
int zkaes_encrypt_batch(size_t n, const uint8_t *messages, const uint8_t *secret_keys, const zkaes_pk *pk, uint8_t **proofs, size_t *proofs_len, size_t *proof_lens) {
    size_t chunk = pk ? pk->pk->circuit().n_blocks * 16 : 0;
    uint8_t seed[32];
    { int rc = guard([&] { zk::os_random_seed(seed); }); if (rc) return rc; }
    return zkaes_encrypt_batch_seeded_at(n, messages, n * chunk, secret_keys, n * (pk ? pk->pk->key_bytes() : 16), pk, seed, 0, proofs, proofs_len, proof_lens);
}
// ---- AES-128-CBC (include/zkaes.h): the prover side; the host-only calls (zkaes_cbc_ciphertext, the verifiers) are in capi_host.cpp
int zkaes_encrypt_cbc_seeded(const uint8_t *msg, size_t len, const uint8_t key[16], const uint8_t iv[16], const zkaes_pk *pk, const uint8_t *seed, uint8_t *ciphertext_or_null,
                             uint8_t **proof, size_t *proof_len) {
    return guard([&] {
        if (!pk || !proof || !proof_len || !msg || !key || !iv) throw std::invalid_argument("null argument");
        std::vector<uint8_t> ct(len ? len : 1);
        auto b = zk::serialize_proof(pk->pk->prove_aes_cbc(msg, len, key, iv, seed, ct.data()));
        if (ciphertext_or_null) memcpy(ciphertext_or_null, ct.data(), len);
        *proof = give(b); *proof_len = b.size();
    });
}
int zkaes_encrypt_cbc_chunked_seeded_at(const uint8_t *msg, size_t len, const uint8_t key[16], const uint8_t iv[16], const zkaes_pk *pk, const uint8_t *zk_seed32, uint64_t first_proof_index,
                                        uint8_t *ciphertext_or_null, uint8_t **proofs, size_t *proofs_len, size_t *proof_lens, size_t n_chunks) {
    return guard([&] {
        if (!pk || !proofs || !proofs_len || !key || !iv || !msg) throw std::invalid_argument("null argument");
        if (pk->pk->circuit().kind != zk::CIRCUIT_AES_CBC) throw std::invalid_argument("proving key was not synthesized for the AES-CBC circuit");
        size_t chunk = pk->pk->circuit().n_blocks * 16;
        if (chunk == 0 || len == 0 || len % chunk || len / chunk != n_chunks) throw std::invalid_argument("message length must be n_chunks * the key's plaintext length");
        std::vector<uint8_t> ct(len);
        auto ps = pk->pk->prove_aes_cbc_chunked(msg, len, key, iv, pk->pk->contexts(), zk_seed32, first_proof_index, ct.data());
        if (ciphertext_or_null) memcpy(ciphertext_or_null, ct.data(), len);
        pack_proofs(ps, proofs, proofs_len, proof_lens);
    });
}
int zkaes_encrypt_cbc_chunked(const uint8_t *msg, size_t len, const uint8_t key[16], const uint8_t iv[16], const zkaes_pk *pk, uint8_t *ciphertext_or_null, uint8_t **proofs,
                              size_t *proofs_len, size_t *proof_lens, size_t n_chunks) {
    uint8_t seed[32];
    { int rc = guard([&] { zk::os_random_seed(seed); }); if (rc) return rc; }
    return zkaes_encrypt_cbc_chunked_seeded_at(msg, len, key, iv, pk, seed, 0, ciphertext_or_null, proofs, proofs_len, proof_lens, n_chunks);
}
int zkaes_aes_witness_cbc(const zkaes_pk *pk, const uint8_t *msg, size_t len, const uint8_t key[16], const uint8_t iv[16], uint8_t *z, size_t z_cap, size_t *z_len) {
    return guard([&] {
        if (!pk) throw std::invalid_argument("null argument");
        auto v = pk->pk->aes_witness_cbc(msg, len, key, iv);
        if (z_len) *z_len = v.size();
        if (z) { if (z_cap < v.size()) throw std::invalid_argument("z buffer too small"); memcpy(z, v.data(), v.size()); }
    });
}
// ---- AES-128-CTR (include/zkaes.h): the prover side; zkaes_ctr_crypt, zkaes_ctr_counter_add and the verifiers are in capi_host.cpp
int zkaes_encrypt_ctr_seeded(const uint8_t *msg, size_t len, const uint8_t key[16], const uint8_t icb[16], const zkaes_pk *pk, const uint8_t *seed, uint8_t *ciphertext_or_null,
                             uint8_t **proof, size_t *proof_len) {
    return guard([&] {
        if (!pk || !proof || !proof_len || !msg || !key || !icb) throw std::invalid_argument("null argument");
        std::vector<uint8_t> ct(len ? len : 1);
        auto b = zk::serialize_proof(pk->pk->prove_aes_ctr(msg, len, key, icb, seed, ct.data()));
        if (ciphertext_or_null) memcpy(ciphertext_or_null, ct.data(), len);
        *proof = give(b); *proof_len = b.size();
    });
}
int zkaes_encrypt_ctr_chunked_seeded_at(const uint8_t *msg, size_t len, const uint8_t key[16], const uint8_t icb[16], const zkaes_pk *pk, const uint8_t *zk_seed32, uint64_t first_proof_index,
                                        uint8_t *ciphertext_or_null, uint8_t **proofs, size_t *proofs_len, size_t *proof_lens, size_t n_chunks) {
    return guard([&] {
        if (!pk || !proofs || !proofs_len || !key || !icb || !msg) throw std::invalid_argument("null argument");
        if (pk->pk->circuit().kind != zk::CIRCUIT_AES_CTR) throw std::invalid_argument("proving key was not synthesized for the AES-CTR circuit");
        size_t chunk = pk->pk->circuit().message_bytes;
        if (chunk == 0 || chunk % 16) throw std::invalid_argument("CTR: a chunked call needs a key for whole blocks");
        if (len == 0 || len % chunk || len / chunk != n_chunks) throw std::invalid_argument("message length must be n_chunks * the key's plaintext length");
        std::vector<uint8_t> ct(len);
        auto ps = pk->pk->prove_aes_ctr_chunked(msg, len, key, icb, pk->pk->contexts(), zk_seed32, first_proof_index, ct.data());
        if (ciphertext_or_null) memcpy(ciphertext_or_null, ct.data(), len);
        pack_proofs(ps, proofs, proofs_len, proof_lens);
    });
}
int zkaes_encrypt_ctr_chunked(const uint8_t *msg, size_t len, const uint8_t key[16], const uint8_t icb[16], const zkaes_pk *pk, uint8_t *ciphertext_or_null, uint8_t **proofs,
                              size_t *proofs_len, size_t *proof_lens, size_t n_chunks) {
    uint8_t seed[32];
    { int rc = guard([&] { zk::os_random_seed(seed); }); if (rc) return rc; }
    return zkaes_encrypt_ctr_chunked_seeded_at(msg, len, key, icb, pk, seed, 0, ciphertext_or_null, proofs, proofs_len, proof_lens, n_chunks);
}
int zkaes_aes_witness_ctr(const zkaes_pk *pk, const uint8_t *msg, size_t len, const uint8_t key[16], const uint8_t icb[16], uint8_t *z, size_t z_cap, size_t *z_len) {
    return guard([&] {
        if (!pk) throw std::invalid_argument("null argument");
        auto v = pk->pk->aes_witness_ctr(msg, len, key, icb);
        if (z_len) *z_len = v.size();
        if (z) { if (z_cap < v.size()) throw std::invalid_argument("z buffer too small"); memcpy(z, v.data(), v.size()); }
    });
}
// ---- AES-128-GCM (include/zkaes.h): the prover side; zkaes_gcm_encrypt, zkaes_gcm_decrypt and the verifier are in capi_host.cpp
int zkaes_encrypt_gcm_seeded(const uint8_t *msg, size_t len, const uint8_t key[16], const uint8_t iv[12], const uint8_t *aad, size_t aad_len, const zkaes_pk *pk, const uint8_t *seed,
                             uint8_t *ciphertext_or_null, uint8_t *tag_or_null, uint8_t **proof, size_t *proof_len) {
    return guard([&] {
        if (!pk || !proof || !proof_len || !msg || !key || !iv || (!aad && aad_len)) throw std::invalid_argument("null argument");
        std::vector<uint8_t> ct(len ? len : 1);
        uint8_t tag[16];
        auto b = zk::serialize_proof(pk->pk->prove_aes_gcm(msg, len, key, iv, aad, aad_len, seed, ct.data(), tag));
        if (ciphertext_or_null) memcpy(ciphertext_or_null, ct.data(), len);
        if (tag_or_null) memcpy(tag_or_null, tag, 16);
        *proof = give(b); *proof_len = b.size();
    });
}
int zkaes_encrypt_gcm_batch_seeded_at(size_t n, const uint8_t *messages, size_t messages_len, const uint8_t *secret_keys, size_t secret_keys_len, const uint8_t *headers, size_t headers_len,
                                      const zkaes_pk *pk, const uint8_t *zk_seed32, uint64_t first_proof_index, uint8_t *ciphertexts_or_null, uint8_t *tags_or_null, uint8_t **proofs,
                                      size_t *proofs_len, size_t *proof_lens) {
    return guard([&] {
        if (!pk || !proofs || !proofs_len || (n && (!messages || !secret_keys || !headers))) throw std::invalid_argument("null argument");
        const zk::Circuit &c = pk->pk->circuit();
        if (c.kind == zk::CIRCUIT_AES_GCM_SEG) throw std::invalid_argument("this proving key is a GCM segment key: use the segment entry points (zkaes_encrypt_gcm_segments_seeded_at, zkaes_aes_witness_gcm_seg)");
        if (c.kind != zk::CIRCUIT_AES_GCM) throw std::invalid_argument("proving key was not synthesized for the AES-GCM circuit");
        if (messages_len != n * c.message_bytes) throw std::invalid_argument("messages must hold n x " + std::to_string(c.message_bytes) + " bytes (the key's plaintext length)");
        if (secret_keys_len != n * c.key_bytes) throw std::invalid_argument("secret_keys must hold n x " + std::to_string(c.key_bytes) + " bytes");
        if (headers_len != n * (12 + c.aad_bytes)) throw std::invalid_argument("headers must hold n x " + std::to_string(12 + c.aad_bytes) + " bytes (iv, then the key's aad length)");
        pack_proofs(pk->pk->prove_aes_gcm_batch(messages, secret_keys, headers, n, pk->pk->contexts(), zk_seed32, first_proof_index, ciphertexts_or_null, tags_or_null), proofs, proofs_len,
                    proof_lens);
    });
}
int zkaes_aes_witness_gcm(const zkaes_pk *pk, const uint8_t *msg, size_t len, const uint8_t key[16], const uint8_t iv[12], const uint8_t *aad, size_t aad_len, uint8_t *z, size_t z_cap,
                          size_t *z_len) {
    return guard([&] {
        if (!pk) throw std::invalid_argument("null argument");
        auto v = pk->pk->aes_witness_gcm(msg, len, key, iv, aad, aad_len);
        if (z_len) *z_len = v.size();
        if (z) { if (z_cap < v.size()) throw std::invalid_argument("z buffer too small"); memcpy(z, v.data(), v.size()); }
    });
}
// ---- GCM segments (include/zkaes.h): the prover side; zkaes_gcm_boundaries, zkaes_gcm_commit, the circuit queries and the verifier are in capi_host.cpp
int zkaes_synthesize_keys_gcm_seg(int role, unsigned key_bits, size_t units, size_t aad_len, size_t nc, size_t nv, size_t nnz, unsigned flags, zkaes_pk **pk, zkaes_vk **vk) {
    return guard([&] {
        if (flags & ~(unsigned)ZKAES_KEY_NO_TABLES) throw std::invalid_argument("synthesize_keys: unknown flag bits");
        zk::SrsLiterals srs; srs.num_constraints = nc; srs.num_variables = nv; srs.num_non_zero = nnz;
        auto k = zk::synthesize_keys_gcm_segment(role, units, aad_len, key_bits, srs, (flags & ZKAES_KEY_NO_TABLES) ? (unsigned)zk::KEY_NO_TABLES : 0u);
        zkaes_vk *v = new zkaes_vk{k->vk()};
        zkaes_pk *p = new zkaes_pk{std::move(k)};
        if (pk) *pk = p; else delete p;
        if (vk) *vk = v; else delete v;
    });
}
int zkaes_pk_segment_info(const zkaes_pk *pk, uint64_t out[4]) {
    return guard([&] {
        if (!pk || !out) throw std::invalid_argument("null argument");
        const zk::Circuit &c = pk->pk->circuit();
        out[0] = c.kind == zk::CIRCUIT_AES_GCM_SEG ? 1 + (uint64_t)c.seg_role : 0; out[1] = c.n_blocks; out[2] = c.message_bytes; out[3] = c.aad_bytes;
    });
}
int zkaes_aes_witness_gcm_seg(const zkaes_pk *pk, const uint8_t *msg, size_t len, const uint8_t *key, const uint8_t *header, size_t header_len, uint8_t *z, size_t z_cap, size_t *z_len) {
    return guard([&] {
        if (!pk) throw std::invalid_argument("null argument");
        auto v = pk->pk->aes_witness_gcm_segment(msg, len, key, header, header_len);
        if (z_len) *z_len = v.size();
        if (z) { if (z_cap < v.size()) throw std::invalid_argument("z buffer too small"); memcpy(z, v.data(), v.size()); }
    });
}
int zkaes_encrypt_gcm_segment_batch_seeded_at(size_t n, const uint8_t *messages, size_t messages_len, const uint8_t *secret_keys, size_t secret_keys_len, const uint8_t *headers, size_t headers_len,
                                              const zkaes_pk *pk, const uint8_t *zk_seed32, uint64_t first_proof_index, uint8_t **proofs, size_t *proofs_len, size_t *proof_lens) {
    return guard([&] {
        if (!pk || !proofs || !proofs_len) throw std::invalid_argument("null argument");
        const zk::Circuit &c = pk->pk->circuit();
        if (c.kind != zk::CIRCUIT_AES_GCM_SEG) throw std::invalid_argument("the key is not a GCM segment key: the segment entry points take keys of zkaes_synthesize_keys_gcm_seg (lone records go through zkaes_encrypt_gcm_batch_seeded_at)");
        const size_t hb = zk::mode_header_bytes(c);
        if (messages_len != n * c.message_bytes) throw std::invalid_argument("messages must hold n x " + std::to_string(c.message_bytes) + " bytes (the key's plaintext length)");
        if (secret_keys_len != n * c.key_bytes) throw std::invalid_argument("secret_keys must hold n x " + std::to_string(c.key_bytes) + " bytes");
        if (headers_len != n * hb) throw std::invalid_argument("headers must hold n x " + std::to_string(hb) + " bytes (iv, ctr0, Y_in, salt_in, salt_out, length block, aad)");
        pack_proofs(pk->pk->prove_gcm_segment_batch(messages, secret_keys, headers, n, pk->pk->contexts(), zk_seed32, first_proof_index), proofs, proofs_len, proof_lens);
    });
}
int zkaes_encrypt_gcm_segments_seeded_at(const uint8_t *msg, size_t len, const uint8_t *key, const uint8_t iv[12], const uint8_t *aad, size_t aad_len, const zkaes_pk *head,
                                         const zkaes_pk *mid_or_null, const zkaes_pk *tail, const uint8_t *salts_or_null, const uint8_t *zk_seed32, size_t first_segment, size_t count,
                                         uint8_t *ciphertext_or_null, uint8_t *tag_or_null, uint8_t *commitments_or_null, uint8_t **proofs, size_t *proofs_len, size_t *proof_lens) {
    return guard([&] {
        if (!head || !tail || !proofs || !proofs_len) throw std::invalid_argument("null argument");
        pack_proofs(zk::prove_gcm_segments(head->pk.get(), mid_or_null ? mid_or_null->pk.get() : nullptr, tail->pk.get(), msg, len, key, iv, aad, aad_len, salts_or_null, first_segment, count,
                                           zk_seed32, ciphertext_or_null, tag_or_null, commitments_or_null), proofs, proofs_len, proof_lens);
    });
}
int zkaes_pk_mode(const zkaes_pk *pk, int *circuit_kind, size_t *header_bytes) {
    return guard([&] {
        if (!pk) throw std::invalid_argument("null argument");
        if (circuit_kind) *circuit_kind = pk->pk->circuit().kind;
        if (header_bytes) *header_bytes = zk::mode_header_bytes(pk->pk->circuit());
    });
}
// ---- plaintext digests (include/zkaes.h): the prover side; zkaes_sha256_chain, zkaes_sha256_finish and the verifiers are in capi_host.cpp
int zkaes_aes_witness_pd(const zkaes_pk *pk, const uint8_t *msg, size_t len, const uint8_t *key, const uint8_t *hdr, const uint8_t *h_in, uint8_t *z, size_t z_cap, size_t *z_len) {
    return guard([&] {
        if (!pk) throw std::invalid_argument("null argument");
        auto v = pk->pk->aes_witness_digest(msg, len, key, hdr, h_in);
        if (z_len) *z_len = v.size();
        if (z) { if (z_cap < v.size()) throw std::invalid_argument("z buffer too small"); memcpy(z, v.data(), v.size()); }
    });
}
int zkaes_encrypt_digest_batch_seeded_at(size_t n, const uint8_t *messages, size_t messages_len, const uint8_t *secret_keys, size_t secret_keys_len, const uint8_t *headers, size_t headers_len,
                                         const uint8_t *h_ins, const zkaes_pk *pk, const uint8_t *zk_seed32, uint64_t first_proof_index, uint8_t *ciphertexts_or_null, uint8_t *tags_or_null,
                                         uint8_t *h_outs_or_null, uint8_t **proofs, size_t *proofs_len, size_t *proof_lens) {
    return guard([&] {
        if (!pk || !proofs || !proofs_len || (n && (!messages || !secret_keys))) throw std::invalid_argument("null argument");
        const zk::Circuit &c = pk->pk->circuit();
        if (!c.digest_kind) throw std::invalid_argument("the _digest_ entry points take a proving key synthesized with a digest (digest_kind = 1 or 2)");
        const size_t hb = zk::mode_header_bytes(c);
        if (messages_len != n * c.message_bytes) throw std::invalid_argument("messages must hold n x " + std::to_string(c.message_bytes) + " bytes (the key's plaintext length)");
        if (secret_keys_len != n * c.key_bytes) throw std::invalid_argument("secret_keys must hold n x " + std::to_string(c.key_bytes) + " bytes");
        if (headers_len != n * hb || (n && hb && !headers)) throw std::invalid_argument("headers must hold n x " + std::to_string(hb) + " bytes (the mode's public header)");
        pack_proofs(pk->pk->prove_digest_batch(messages, secret_keys, hb ? headers : nullptr, h_ins, n, pk->pk->contexts(), zk_seed32, first_proof_index, ciphertexts_or_null, tags_or_null,
                                               h_outs_or_null), proofs, proofs_len, proof_lens);
    });
}
int zkaes_encrypt_digest_chunked_seeded_at(const uint8_t *msg, size_t len, const uint8_t *key, const uint8_t *hdr, const uint8_t *h_in, const zkaes_pk *pk, const uint8_t *zk_seed32,
                                           uint64_t first_proof_index, uint8_t *ciphertext_or_null, uint8_t *states_or_null, uint8_t **proofs, size_t *proofs_len, size_t *proof_lens,
                                           size_t n_chunks) {
    return guard([&] {
        if (!pk || !proofs || !proofs_len || !key || !msg) throw std::invalid_argument("null argument");
        const size_t chunk = pk->pk->circuit().message_bytes;
        if (chunk == 0 || len == 0 || len % chunk || len / chunk != n_chunks) throw std::invalid_argument("message length must be n_chunks * the key's plaintext length");
        pack_proofs(pk->pk->prove_digest_chunked(msg, len, key, hdr, h_in, pk->pk->contexts(), zk_seed32, first_proof_index, ciphertext_or_null, states_or_null), proofs, proofs_len, proof_lens);
    });
}
int zkaes_prove_ops(const zkaes_pk *pk, uint32_t x, uint32_t y, const uint8_t *seed, uint8_t **proof, size_t *proof_len) {
    return guard([&] {
        if (!pk || !proof || !proof_len) throw std::invalid_argument("null argument");
        auto b = zk::serialize_proof(pk->pk->prove_ops(x, y, seed));
        *proof = give(b); *proof_len = b.size();
    });
}
int zkaes_pk_info(const zkaes_pk *pk, uint64_t out[12]) {
    return guard([&] {
        fill_info(pk->pk->circuit(), out);
        out[9] = pk->pk->vk().num_non_zero; out[10] = next_pow2(pk->pk->vk().num_constraints); out[11] = next_pow2(pk->pk->vk().num_non_zero);
    });
}
int zkaes_pk_serialize_ark_to_file_ex(const zkaes_pk *pk, const char *path, int uncompressed, uint64_t *bytes_written) {
    return guard([&] {
        if (!pk || !path) throw std::invalid_argument("null argument");
        uint64_t n = pk->pk->serialize_ark_to_file(path, uncompressed != 0);
        if (bytes_written) *bytes_written = n;
    });
}
int zkaes_pk_serialize_ark_to_file(const zkaes_pk *pk, const char *path, uint64_t *bytes_written) { return zkaes_pk_serialize_ark_to_file_ex(pk, path, 0, bytes_written); }
int zkaes_set_default_contexts(size_t n) { return guard([&] { if (n > 64) throw std::invalid_argument("set_default_contexts: at most 64 prover contexts per key"); zk::set_default_contexts(n); }); }
int zkaes_srs_hold(int hold) { return guard([&] { zk::srs_hold(hold != 0); }); }
int zkaes_pk_set_contexts(zkaes_pk *pk, size_t n) {
    return guard([&] {
        if (!pk) throw std::invalid_argument("null argument");
        pk->pk->set_contexts(n);
    });
}
int zkaes_pk_get_contexts(const zkaes_pk *pk, size_t *n) {
    return guard([&] {
        if (!pk || !n) throw std::invalid_argument("null argument");
        *n = pk->pk->contexts();
    });
}
int zkaes_pk_srs_info(const zkaes_pk *pk, uint64_t out[6], double secs[2]) {
    return guard([&] {
        if (!pk || !out) throw std::invalid_argument("null argument");
        pk->pk->srs_info(out, secs);
    });
}
int zkaes_pk_op_lists(const zkaes_pk *pk, const uint8_t *msg, size_t len, const uint8_t key[16], int throughput_path, uint8_t **json, size_t *json_len) {
    return guard([&] {
        if (!pk || !json || !json_len || !key || (!msg && len)) throw std::invalid_argument("null argument");
        std::string o = pk->pk->op_lists_json(msg, len, key, throughput_path != 0);
        *json = give(std::vector<uint8_t>(o.begin(), o.end())); *json_len = o.size();
    });
}
int zkaes_pk_tables_built(const zkaes_pk *pk, int *built, uint64_t *table_bytes) {
    return guard([&] {
        if (!pk || !built) throw std::invalid_argument("null argument");
        *built = pk->pk->tables_built(table_bytes) ? 1 : 0;
    });
}
int zkaes_pk_msm_partial_dev(const zkaes_pk *pk, const uint8_t *scalars, size_t n_local, size_t offset, void *dev_out, size_t dev_out_bytes) {
    return guard([&] {
        if (!pk || (!scalars && n_local)) throw std::invalid_argument("null argument");
        if (!dev_out || dev_out_bytes < 192) throw std::invalid_argument("zkaes_pk_msm_partial_dev: device buffer too small for the partial sum (192 bytes)");
        pk->pk->msm_powers_partial_device(scalars, n_local, offset, dev_out);
    });
}
int zkaes_pk_debug_fetch(const zkaes_pk *pk, const char *name, uint8_t **out, size_t *len) {
    return guard([&] { auto b = pk->pk->debug_fetch(name); *out = give(b); *len = b.size(); });
}
int zkaes_aes_witness(const zkaes_pk *pk, const uint8_t *msg, size_t len, const uint8_t key[16], uint8_t *z, size_t z_cap, size_t *z_len) {
    return guard([&] {
        auto v = pk->pk->aes_witness(msg, len, key);
        if (z_len) *z_len = v.size();
        if (z) { if (z_cap < v.size()) throw std::invalid_argument("z buffer too small"); memcpy(z, v.data(), v.size()); }
    });
}
int zkaes_pk_timings(const zkaes_pk *pk, double out[6]) {
    return guard([&] { const auto &t = pk->pk->last_timings(); out[0] = t.witness_ms; out[1] = t.round1_ms; out[2] = t.round2_ms; out[3] = t.round3_ms; out[4] = t.open_ms; out[5] = t.total_ms; });
}
// ---- batch verification on the device (include/zkaes.h); the host back end, zkaes_verify_batch_timings and zkaes_chunk_public_inputs are in capi_host.cpp
int zkaes_verify_batch_gpu(const zkaes_vk *vk, const uint8_t *proofs, const size_t *proof_lens, size_t n, const uint8_t *public_input_bits, size_t n_bits, int *accepted_each,
                           size_t *n_accepted) {
    return guard([&] {
        if (n_accepted) *n_accepted = 0;
        std::unique_ptr<zk::BatchBackend> be = zk::make_device_batch_backend();
        zk::capi::verify_batch_call(vk, proofs, proof_lens, n, public_input_bits, n_bits, accepted_each, n_accepted, *be);
    });
}
// the three kernels behind it, one launch per call (tests/test_gpu_verify_batch.py)
int zkaes_g1_decompress_batch(const uint8_t *points48, size_t n, uint8_t *out_xy, uint8_t *status) {
    return guard([&] {
        if (!points48 || !out_xy || !status) throw std::invalid_argument("null argument");
        if (n == 0 || n > ((size_t)1 << 24)) throw std::invalid_argument("zkaes_g1_decompress_batch: 1 .. 2^24 points");
        std::unique_ptr<zk::BatchBackend> be = zk::make_device_batch_backend();
        std::vector<zk::G1Compressed> todo;
        std::vector<size_t> where;
        memset(out_xy, 0, 96 * n);
        for (size_t i = 0; i < n; i++) {
            zk::G1Compressed c;
            bool inf = false;
            if (!zk::g1_parse_compressed(points48 + 48 * i, c, &inf)) status[i] = zk::G1_MALFORMED;
            else if (inf) status[i] = zk::G1_INFINITY;
            else { todo.push_back(c); where.push_back(i); }
        }
        if (todo.empty()) return;
        std::vector<zk::G1A> pts(todo.size());
        std::vector<uint8_t> st(todo.size());
        be->decompress(todo.data(), todo.size(), pts.data(), st.data());
        for (size_t j = 0; j < todo.size(); j++) { status[where[j]] = st[j]; memcpy(out_xy + 96 * where[j], pts[j].x.l, 48); memcpy(out_xy + 96 * where[j] + 48, pts[j].y.l, 48); }
    });
}
int zkaes_fq_sqrt_batch(const uint8_t *in, size_t n, uint8_t *out, uint8_t *is_square) {
    return guard([&] {
        if (!in || !out || !is_square) throw std::invalid_argument("null argument");
        if (n == 0 || n > ((size_t)1 << 24)) throw std::invalid_argument("zkaes_fq_sqrt_batch: 1 .. 2^24 elements");
        for (size_t i = 0; i < n; i++) { uint32_t l[12]; memcpy(l, in + 48 * i, 48); if (zk::Fq377::geq_mod(l)) throw std::invalid_argument("zkaes_fq_sqrt_batch: limbs not below the modulus"); }
        zk::gpu::require_device();
        zk::gpu::StreamGuard s;
        zk::gpu::DevPtr<zk::Fq377> d_in(n), d_out(n);
        zk::gpu::DevPtr<uint8_t> d_ok(n);
        zk::gpu::h2d(d_in, in, 48 * n, s);
        zk::gpu::fq_sqrt_batch(d_in, n, d_out, d_ok, s);
        zk::gpu::d2h(out, d_out, 48 * n, s);
        zk::gpu::d2h(is_square, d_ok, n, s);
    });
}
int zkaes_public_input_eval(int lg_m, const uint8_t *betas, const uint8_t *bits, size_t n, size_t n_bits, uint8_t *out) {
    return guard([&] {
        if (!betas || !out || (n_bits && !bits)) throw std::invalid_argument("null argument");
        if (lg_m < 0 || lg_m > 30 || n == 0 || n > ((size_t)1 << 20) || n_bits >= ((size_t)1 << lg_m)) throw std::invalid_argument("zkaes_public_input_eval: 1 .. 2^20 rows of fewer than 2^lg_m bits, lg_m <= 30");
        std::vector<zk::Fr> b(n), o(n);
        for (size_t i = 0; i < n; i++) { memcpy(b[i].l, betas + 32 * i, 32); if (zk::Fr::geq_mod(b[i].l)) throw std::invalid_argument("zkaes_public_input_eval: limbs not below the modulus"); }
        std::unique_ptr<zk::BatchBackend> be = zk::make_device_batch_backend();
        be->public_input_eval(lg_m, b.data(), bits, n, n_bits, o.data());
        memcpy(out, o.data(), 32 * n);
    });
}
int zkaes_msm_stats(double out[5], int reset) {
    return guard([&] {
        auto s = zk::gpu::msm_stats(reset != 0);
        out[0] = s.accumulate_ms; out[1] = s.total_ms; out[2] = (double)s.points; out[3] = (double)s.launches; out[4] = (double)s.pairs;
    });
}

}  // extern "C"
