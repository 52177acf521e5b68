// csrc/capi.cpp -- the entry points of include/zkaes.h that need a GPU: key synthesis, the prover, key-handle queries (host-only ones: capi_host.cpp)
#include "capi_common.hpp"
#include <algorithm>
#include "gpu.hpp"
#include "fq_sqrt.cuh"

using zk::capi::guard; using zk::capi::give; using zk::capi::fill_info; using zk::capi::next_pow2;

namespace {
enum { ECB = zk::CIRCUIT_AES, CBC = zk::CIRCUIT_AES_CBC, CTR = zk::CIRCUIT_AES_CTR, GCM = zk::CIRCUIT_AES_GCM, ANY = zk::ProvingKey::ANY_AES_KIND };
// a fresh key pair to the caller's handles
void give_keys(std::unique_ptr<zk::ProvingKey> k, zkaes_pk **pk, zkaes_vk **vk) {
    zkaes_vk *v = new zkaes_vk{k->vk()};
    zkaes_pk *p = new zkaes_pk{std::move(k)};
    if (pk) *pk = p; else delete p;
    if (vk) *vk = v; else delete v;
}
unsigned key_flags(unsigned flags) {
    if (flags & ~(unsigned)ZKAES_KEY_NO_TABLES) throw std::invalid_argument("synthesize_keys: unknown flag bits");
    return (flags & ZKAES_KEY_NO_TABLES) ? (unsigned)zk::KEY_NO_TABLES : 0u;
}
zk::SrsLiterals srs_literals(size_t nc, size_t nv, size_t nnz) { zk::SrsLiterals srs; srs.num_constraints = nc; srs.num_variables = nv; srs.num_non_zero = nnz; return srs; }
int synthesize(int kind, size_t len, size_t aad_len, size_t nc, size_t nv, size_t nnz, unsigned flags, zkaes_pk **pk, zkaes_vk **vk, size_t key_bits = 128, size_t key_tag_blocks = 0,
               unsigned digest_kind = 0, uint64_t digest_prefix = 0, unsigned reveal = 0) {
    return guard([&] {
        const unsigned f = key_flags(flags);
        if (key_bits != 128 && key_bits != 192 && key_bits != 256) throw std::invalid_argument("synthesize_keys: key_bits must be 128, 192 or 256");
        if (key_tag_blocks > 2) throw std::invalid_argument("synthesize_keys: key_tag_blocks must be 0, 1 or 2");
        if (digest_kind > 2) throw std::invalid_argument("synthesize_keys: digest_kind must be 0 (none), 1 (chain) or 2 (final)");
        if (reveal > 1) throw std::invalid_argument("synthesize_keys: reveal must be 0 or 1");
        give_keys(zk::synthesize_keys(kind, len, srs_literals(nc, nv, nnz), f, aad_len, key_bits, key_tag_blocks, (int)digest_kind, digest_prefix, (int)reveal), pk, vk);
    });
}
// the unseeded multi-proof entry points draw a fresh seed from the OS per call and go on as their _seeded_at form.  The reference's fixed ark_std::test_rng() stream for
// every proof (byte parity with the oracle; NOT zero-knowledge across proofs) is reachable only explicitly, through the *_seeded entry points with a NULL seed -- no
// environment variable downgrades a caller
template <class Seeded> int with_os_seed(Seeded &&seeded) {
    uint8_t seed[32];
    int rc = guard([&] { zk::os_random_seed(seed); });
    return rc ? rc : seeded(seed);
}
// a witness to the caller: its length always, its bytes where there is a buffer
void give_witness(const std::vector<uint8_t> &v, uint8_t *z, size_t z_cap, size_t *z_len) {
    if (z_len) *z_len = v.size();
    if (z) { if (z_cap < v.size()) throw std::invalid_argument("z buffer too small"); memcpy(z, v.data(), v.size()); }
}
void give_proof(const zk::Proof &p, uint8_t **proof, size_t *proof_len) {
    auto b = zk::serialize_proof(p);
    *proof = give(b); *proof_len = b.size();
}
void pack_proofs(const std::vector<zk::Proof> &ps, uint8_t **proofs, size_t *proofs_len, size_t *proof_lens) {
    std::vector<uint8_t> all;
    for (size_t i = 0; i < ps.size(); i++) {
        auto b = zk::serialize_proof(ps[i]);
        if (proof_lens) proof_lens[i] = b.size();
        all.insert(all.end(), b.begin(), b.end());
    }
    *proofs = give(all); *proofs_len = all.size();
}
// the packed arrays of a batch call hold n of what the key takes each
void require_packed(const zk::Circuit &c, size_t n, size_t messages_len, size_t secret_keys_len) {
    if (messages_len != n * c.message_bytes) throw std::invalid_argument("messages must hold n x " + std::to_string(c.message_bytes) + " bytes (the key's plaintext length)");
    if (secret_keys_len != n * c.key_bytes) throw std::invalid_argument("secret_keys must hold n x " + std::to_string(c.key_bytes) + " bytes");
}
// a GCM record's header as the prover takes it: iv, then aad
std::vector<uint8_t> gcm_header(const uint8_t iv[12], const uint8_t *aad, size_t aad_len) {
    std::vector<uint8_t> h(iv, iv + 12);
    if (aad_len) h.insert(h.end(), aad, aad + aad_len);
    return h;
}
}  // namespace

extern "C" {

void zkaes_pk_free(zkaes_pk *pk) { delete pk; }
int zkaes_device_count(void) { return zk::gpu::device_count(); }

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
int zkaes_synthesize_keys_pd(int kind, unsigned key_bits, unsigned key_tag_blocks, unsigned digest_kind, uint64_t digest_prefix, size_t len, size_t aad_len, size_t nc, size_t nv, size_t nnz,
                             unsigned flags, zkaes_pk **pk, zkaes_vk **vk) {
    return synthesize(kind, len, aad_len, nc, nv, nnz, flags, pk, vk, key_bits, key_tag_blocks, digest_kind, digest_prefix);
}
int zkaes_synthesize_keys_rv(int kind, unsigned key_bits, unsigned key_tag_blocks, unsigned digest_kind, uint64_t digest_prefix, unsigned reveal, size_t len, size_t aad_len, size_t nc, size_t nv,
                             size_t nnz, unsigned flags, zkaes_pk **pk, zkaes_vk **vk) {
    return synthesize(kind, len, aad_len, nc, nv, nnz, flags, pk, vk, key_bits, key_tag_blocks, digest_kind, digest_prefix, reveal);
}
int zkaes_synthesize_keys_ex(int kind, size_t len, size_t nc, size_t nv, size_t nnz, zkaes_pk **pk, zkaes_vk **vk) {
    return zkaes_synthesize_keys_ex2(kind, len, nc, nv, nnz, 0u, pk, vk);
}
int zkaes_synthesize_keys(size_t len, zkaes_pk **pk, zkaes_vk **vk) {
    zk::SrsLiterals d;
    return zkaes_synthesize_keys_ex(ZKAES_CIRCUIT_AES, len, d.num_constraints, d.num_variables, d.num_non_zero, pk, vk);
}
int zkaes_pk_key_tag_blocks(const zkaes_pk *pk, size_t *n) {
    return guard([&] {
        if (!pk || !n) throw std::invalid_argument("null argument");
        *n = pk->pk->key_tag_blocks();
    });
}
int zkaes_pk_digest_info(const zkaes_pk *pk, uint64_t out[4]) {
    return guard([&] {
        if (!pk || !out) throw std::invalid_argument("null argument");
        const zk::Circuit &c = pk->pk->circuit();
        out[0] = (uint64_t)c.digest_kind; out[1] = c.digest_prefix; out[2] = c.digest_blocks; out[3] = c.digest_off;
    });
}
int zkaes_pk_reveal_info(const zkaes_pk *pk, uint64_t out[4]) {
    return guard([&] {
        if (!pk || !out) throw std::invalid_argument("null argument");
        const zk::Circuit &c = pk->pk->circuit();
        out[0] = (uint64_t)c.reveal; out[1] = c.reveal ? c.message_bytes : 0; out[2] = zk::reveal_mask_bytes(c); out[3] = c.reveal_off;
    });
}
int zkaes_pk_key_bytes(const zkaes_pk *pk, size_t *n) {
    return guard([&] {
        if (!pk || !n) throw std::invalid_argument("null argument");
        *n = pk->pk->key_bytes();
    });
}
int zkaes_pk_mode(const zkaes_pk *pk, int *circuit_kind, size_t *header_bytes) {
    return guard([&] {
        if (!pk) throw std::invalid_argument("null argument");
        if (circuit_kind) *circuit_kind = pk->pk->circuit().kind;
        if (header_bytes) *header_bytes = zk::mode_header_bytes(pk->pk->circuit());
    });
}
// ---- The prover's entry points: argument checks, then the one call of the shape -- witness, lone, batch, chunked -- with the mode the entry is for (marlin.hpp).  The
// host-only calls of every mode (the host ciphers, zkaes_ctr_counter_add, zkaes_sha256_*, the verifiers) are in capi_host.cpp
// -- AES-ECB
int zkaes_encrypt_seeded(const uint8_t *msg, size_t len, const uint8_t key[16], const zkaes_pk *pk, const uint8_t *seed, uint8_t **proof, size_t *proof_len) {
    return guard([&] {
        if (!pk || !proof || !proof_len) throw std::invalid_argument("null argument");
        give_proof(pk->pk->prove_lone(ECB, msg, len, key, nullptr, 0, seed), proof, proof_len);
    });
}
int zkaes_encrypt(const uint8_t *msg, size_t len, const uint8_t key[16], const zkaes_pk *pk, uint8_t **proof, size_t *proof_len) {
    return zkaes_encrypt_seeded(msg, len, key, pk, nullptr, proof, proof_len);
}
int zkaes_aes_witness(const zkaes_pk *pk, const uint8_t *msg, size_t len, const uint8_t key[16], uint8_t *z, size_t z_cap, size_t *z_len) {
    return guard([&] {
        if (!pk) throw std::invalid_argument("null argument");
        give_witness(pk->pk->witness(ECB, false, msg, len, key, nullptr), z, z_cap, z_len);
    });
}
int zkaes_encrypt_chunked_seeded_at(const uint8_t *msg, size_t len, const uint8_t key[16], const zkaes_pk *pk, const uint8_t *zk_seed32, uint64_t first_proof_index, uint8_t **proofs,
                                    size_t *proofs_len, size_t *proof_lens, size_t n_chunks) {
    return guard([&] {
        if (!pk || !proofs || !proofs_len || !key || (!msg && len)) throw std::invalid_argument("null argument");
        size_t chunk = pk->pk->circuit().n_blocks * 16;
        if (chunk == 0 || len % chunk || len / chunk != n_chunks) throw std::invalid_argument("message length must be n_chunks * the key's plaintext length");
        pack_proofs(pk->pk->prove_chunked(ECB, false, msg, len, key, nullptr, nullptr, pk->pk->contexts(), zk_seed32, first_proof_index), proofs, proofs_len, proof_lens);
    });
}
int zkaes_encrypt_chunked_seeded(const uint8_t *msg, size_t len, const uint8_t key[16], const zkaes_pk *pk, const uint8_t *zk_seed32, uint8_t **proofs, size_t *proofs_len,
                                 size_t *proof_lens, size_t n_chunks) {
    return zkaes_encrypt_chunked_seeded_at(msg, len, key, pk, zk_seed32, 0, proofs, proofs_len, proof_lens, n_chunks);
}
int zkaes_encrypt_chunked(const uint8_t *msg, size_t len, const uint8_t key[16], const zkaes_pk *pk, uint8_t **proofs, size_t *proofs_len, size_t *proof_lens, size_t n_chunks) {
    return with_os_seed([&](const uint8_t *seed) { return zkaes_encrypt_chunked_seeded_at(msg, len, key, pk, seed, 0, proofs, proofs_len, proof_lens, n_chunks); });
}
int zkaes_encrypt_batch_seeded_at(size_t n, const uint8_t *messages, size_t messages_len, const uint8_t *secret_keys, size_t secret_keys_len, const zkaes_pk *pk,
                                  const uint8_t *zk_seed32, uint64_t first_proof_index, uint8_t **proofs, size_t *proofs_len, size_t *proof_lens) {
    return guard([&] {
        if (!pk || !proofs || !proofs_len || (n && (!messages || !secret_keys))) throw std::invalid_argument("null argument");
        require_packed(pk->pk->circuit(), n, messages_len, secret_keys_len);
        pack_proofs(pk->pk->prove_batch(ECB, false, messages, secret_keys, nullptr, nullptr, n, pk->pk->contexts(), zk_seed32, first_proof_index), proofs, proofs_len, proof_lens);
    });
}
int zkaes_encrypt_batch_seeded(size_t n, const uint8_t *messages, size_t messages_len, const uint8_t *secret_keys, size_t secret_keys_len, const zkaes_pk *pk,
                               const uint8_t *zk_seed32, uint8_t **proofs, size_t *proofs_len, size_t *proof_lens) {
    return zkaes_encrypt_batch_seeded_at(n, messages, messages_len, secret_keys, secret_keys_len, pk, zk_seed32, 0, proofs, proofs_len, proof_lens);
}
int zkaes_encrypt_batch(size_t n, const uint8_t *messages, const uint8_t *secret_keys, const zkaes_pk *pk, uint8_t **proofs, size_t *proofs_len, size_t *proof_lens) {
    const size_t chunk = pk ? pk->pk->circuit().n_blocks * 16 : 0, kb = pk ? pk->pk->key_bytes() : 16;      // (this form takes the caller's word for the packed lengths)
    return with_os_seed([&](const uint8_t *seed) { return zkaes_encrypt_batch_seeded_at(n, messages, n * chunk, secret_keys, n * kb, pk, seed, 0, proofs, proofs_len, proof_lens); });
}
// -- AES-CBC and AES-CTR: one public header of 16 bytes, the iv or the initial counter block
static int encrypt_lone_16(int kind, const uint8_t *msg, size_t len, const uint8_t *key, const uint8_t *hdr, const zkaes_pk *pk, const uint8_t *seed, uint8_t *ciphertext_or_null, uint8_t **proof,
                           size_t *proof_len) {
    return guard([&] {
        if (!pk || !proof || !proof_len || !msg || !key || !hdr) throw std::invalid_argument("null argument");
        give_proof(pk->pk->prove_lone(kind, msg, len, key, hdr, 0, seed, ciphertext_or_null), proof, proof_len);
    });
}
int zkaes_encrypt_cbc_seeded(const uint8_t *msg, size_t len, const uint8_t key[16], const uint8_t iv[16], const zkaes_pk *pk, const uint8_t *seed, uint8_t *ciphertext_or_null,
                             uint8_t **proof, size_t *proof_len) {
    return encrypt_lone_16(CBC, msg, len, key, iv, pk, seed, ciphertext_or_null, proof, proof_len);
}
int zkaes_encrypt_ctr_seeded(const uint8_t *msg, size_t len, const uint8_t key[16], const uint8_t icb[16], const zkaes_pk *pk, const uint8_t *seed, uint8_t *ciphertext_or_null,
                             uint8_t **proof, size_t *proof_len) {
    return encrypt_lone_16(CTR, msg, len, key, icb, pk, seed, ciphertext_or_null, proof, proof_len);
}
int zkaes_encrypt_cbc_chunked_seeded_at(const uint8_t *msg, size_t len, const uint8_t key[16], const uint8_t iv[16], const zkaes_pk *pk, const uint8_t *zk_seed32, uint64_t first_proof_index,
                                        uint8_t *ciphertext_or_null, uint8_t **proofs, size_t *proofs_len, size_t *proof_lens, size_t n_chunks) {
    return guard([&] {
        if (!pk || !proofs || !proofs_len || !key || !iv || !msg) throw std::invalid_argument("null argument");
        if (pk->pk->circuit().kind != zk::CIRCUIT_AES_CBC) throw std::invalid_argument("proving key was not synthesized for the AES-CBC circuit");
        size_t chunk = pk->pk->circuit().n_blocks * 16;
        if (chunk == 0 || len == 0 || len % chunk || len / chunk != n_chunks) throw std::invalid_argument("message length must be n_chunks * the key's plaintext length");
        pack_proofs(pk->pk->prove_chunked(CBC, false, msg, len, key, iv, nullptr, pk->pk->contexts(), zk_seed32, first_proof_index, ciphertext_or_null), proofs, proofs_len, proof_lens);
    });
}
int zkaes_encrypt_cbc_chunked(const uint8_t *msg, size_t len, const uint8_t key[16], const uint8_t iv[16], const zkaes_pk *pk, uint8_t *ciphertext_or_null, uint8_t **proofs,
                              size_t *proofs_len, size_t *proof_lens, size_t n_chunks) {
    return with_os_seed([&](const uint8_t *seed) { return zkaes_encrypt_cbc_chunked_seeded_at(msg, len, key, iv, pk, seed, 0, ciphertext_or_null, proofs, proofs_len, proof_lens, n_chunks); });
}
int zkaes_encrypt_ctr_chunked_seeded_at(const uint8_t *msg, size_t len, const uint8_t key[16], const uint8_t icb[16], const zkaes_pk *pk, const uint8_t *zk_seed32, uint64_t first_proof_index,
                                        uint8_t *ciphertext_or_null, uint8_t **proofs, size_t *proofs_len, size_t *proof_lens, size_t n_chunks) {
    return guard([&] {
        if (!pk || !proofs || !proofs_len || !key || !icb || !msg) throw std::invalid_argument("null argument");
        if (pk->pk->circuit().kind != zk::CIRCUIT_AES_CTR) throw std::invalid_argument("proving key was not synthesized for the AES-CTR circuit");
        size_t chunk = pk->pk->circuit().message_bytes;
        if (chunk == 0 || chunk % 16) throw std::invalid_argument("CTR: a chunked call needs a key for whole blocks");
        if (len == 0 || len % chunk || len / chunk != n_chunks) throw std::invalid_argument("message length must be n_chunks * the key's plaintext length");
        pack_proofs(pk->pk->prove_chunked(CTR, false, msg, len, key, icb, nullptr, pk->pk->contexts(), zk_seed32, first_proof_index, ciphertext_or_null), proofs, proofs_len, proof_lens);
    });
}
int zkaes_encrypt_ctr_chunked(const uint8_t *msg, size_t len, const uint8_t key[16], const uint8_t icb[16], const zkaes_pk *pk, uint8_t *ciphertext_or_null, uint8_t **proofs,
                              size_t *proofs_len, size_t *proof_lens, size_t n_chunks) {
    return with_os_seed([&](const uint8_t *seed) { return zkaes_encrypt_ctr_chunked_seeded_at(msg, len, key, icb, pk, seed, 0, ciphertext_or_null, proofs, proofs_len, proof_lens, n_chunks); });
}
int zkaes_aes_witness_cbc(const zkaes_pk *pk, const uint8_t *msg, size_t len, const uint8_t key[16], const uint8_t iv[16], uint8_t *z, size_t z_cap, size_t *z_len) {
    return guard([&] {
        if (!pk) throw std::invalid_argument("null argument");
        give_witness(pk->pk->witness(CBC, false, msg, len, key, iv), z, z_cap, z_len);
    });
}
int zkaes_aes_witness_ctr(const zkaes_pk *pk, const uint8_t *msg, size_t len, const uint8_t key[16], const uint8_t icb[16], uint8_t *z, size_t z_cap, size_t *z_len) {
    return guard([&] {
        if (!pk) throw std::invalid_argument("null argument");
        give_witness(pk->pk->witness(CTR, false, msg, len, key, icb), z, z_cap, z_len);
    });
}
// -- AES-GCM: the public header is iv, then aad
int zkaes_encrypt_gcm_seeded(const uint8_t *msg, size_t len, const uint8_t key[16], const uint8_t iv[12], const uint8_t *aad, size_t aad_len, const zkaes_pk *pk, const uint8_t *seed,
                             uint8_t *ciphertext_or_null, uint8_t *tag_or_null, uint8_t **proof, size_t *proof_len) {
    return guard([&] {
        if (!pk || !proof || !proof_len || !msg || !key || !iv || (!aad && aad_len)) throw std::invalid_argument("null argument");
        give_proof(pk->pk->prove_lone(GCM, msg, len, key, gcm_header(iv, aad, aad_len).data(), aad_len, seed, ciphertext_or_null, tag_or_null), proof, proof_len);
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
        require_packed(c, n, messages_len, secret_keys_len);
        if (headers_len != n * (12 + c.aad_bytes)) throw std::invalid_argument("headers must hold n x " + std::to_string(12 + c.aad_bytes) + " bytes (iv, then the key's aad length)");
        pack_proofs(pk->pk->prove_batch(GCM, false, messages, secret_keys, headers, nullptr, n, pk->pk->contexts(), zk_seed32, first_proof_index, ciphertexts_or_null, tags_or_null), proofs,
                    proofs_len, proof_lens);
    });
}
int zkaes_aes_witness_gcm(const zkaes_pk *pk, const uint8_t *msg, size_t len, const uint8_t key[16], const uint8_t iv[12], const uint8_t *aad, size_t aad_len, uint8_t *z, size_t z_cap,
                          size_t *z_len) {
    return guard([&] {
        if (!pk || !iv || (!aad && aad_len)) throw std::invalid_argument("null argument");
        give_witness(pk->pk->witness(GCM, false, msg, len, key, gcm_header(iv, aad, aad_len).data(), aad_len), z, z_cap, z_len);
    });
}
// -- GCM segments
int zkaes_synthesize_keys_gcm_seg(int role, unsigned key_bits, size_t units, size_t aad_len, size_t nc, size_t nv, size_t nnz, unsigned flags, zkaes_pk **pk, zkaes_vk **vk) {
    return guard([&] {
        const unsigned f = key_flags(flags);
        give_keys(zk::synthesize_keys_gcm_segment(role, units, aad_len, key_bits, srs_literals(nc, nv, nnz), f), pk, vk);
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
        give_witness(pk->pk->aes_witness_gcm_segment(msg, len, key, header, header_len), z, z_cap, z_len);
    });
}
int zkaes_encrypt_gcm_segment_batch_seeded_at(size_t n, const uint8_t *messages, size_t messages_len, const uint8_t *secret_keys, size_t secret_keys_len, const uint8_t *headers, size_t headers_len,
                                              const zkaes_pk *pk, const uint8_t *zk_seed32, uint64_t first_proof_index, uint8_t **proofs, size_t *proofs_len, size_t *proof_lens) {
    return guard([&] {
        if (!pk || !proofs || !proofs_len) throw std::invalid_argument("null argument");
        const zk::Circuit &c = pk->pk->circuit();
        if (c.kind != zk::CIRCUIT_AES_GCM_SEG) throw std::invalid_argument("the key is not a GCM segment key: the segment entry points take keys of zkaes_synthesize_keys_gcm_seg (lone records go through zkaes_encrypt_gcm_batch_seeded_at)");
        const size_t hb = zk::mode_header_bytes(c);
        require_packed(c, n, messages_len, secret_keys_len);
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
// -- selective disclosure on segments: the entries above with a mask; they take keys of zkaes_synthesize_keys_gcm_seg_rv with reveal = 1 only, and the
// entries above refuse such keys
int zkaes_synthesize_keys_gcm_seg_rv(int role, unsigned key_bits, unsigned reveal, size_t units, size_t aad_len, size_t nc, size_t nv, size_t nnz, unsigned flags, zkaes_pk **pk, zkaes_vk **vk) {
    return guard([&] {
        const unsigned f = key_flags(flags);
        if (reveal > 1) throw std::invalid_argument("synthesize_keys: reveal must be 0 or 1");
        give_keys(zk::synthesize_keys_gcm_segment(role, units, aad_len, key_bits, srs_literals(nc, nv, nnz), f, (int)reveal), pk, vk);
    });
}
// -- key tags on segments: a head key with key_tag_blocks = 1 or 2; the proving and witness entries above take it as they take any head key
int zkaes_synthesize_keys_gcm_seg_kt(int role, unsigned key_bits, unsigned reveal, unsigned key_tag_blocks, size_t units, size_t aad_len, size_t nc, size_t nv, size_t nnz, unsigned flags,
                                     zkaes_pk **pk, zkaes_vk **vk) {
    return guard([&] {
        const unsigned f = key_flags(flags);
        if (reveal > 1) throw std::invalid_argument("synthesize_keys: reveal must be 0 or 1");
        if (key_tag_blocks > 2) throw std::invalid_argument("synthesize_keys: key_tag_blocks must be 0, 1 or 2");
        give_keys(zk::synthesize_keys_gcm_segment(role, units, aad_len, key_bits, srs_literals(nc, nv, nnz), f, (int)reveal, key_tag_blocks), pk, vk);
    });
}
int zkaes_aes_witness_gcm_seg_rv(const zkaes_pk *pk, const uint8_t *msg, size_t len, const uint8_t *key, const uint8_t *header, size_t header_len, const uint8_t *mask, size_t mask_len,
                                 uint8_t *z, size_t z_cap, size_t *z_len) {
    return guard([&] {
        if (!pk || !mask) throw std::invalid_argument("null argument");
        give_witness(pk->pk->aes_witness_gcm_segment(msg, len, key, header, header_len, mask, mask_len), z, z_cap, z_len);
    });
}
int zkaes_encrypt_gcm_segment_reveal_batch_seeded_at(size_t n, const uint8_t *messages, size_t messages_len, const uint8_t *secret_keys, size_t secret_keys_len, const uint8_t *headers,
                                                     size_t headers_len, const uint8_t *masks, size_t masks_len, const zkaes_pk *pk, const uint8_t *zk_seed32, uint64_t first_proof_index,
                                                     uint8_t *revealed_or_null, uint8_t **proofs, size_t *proofs_len, size_t *proof_lens) {
    return guard([&] {
        if (!pk || !proofs || !proofs_len || !masks) throw std::invalid_argument("null argument");
        const zk::Circuit &c = pk->pk->circuit();
        if (c.kind != zk::CIRCUIT_AES_GCM_SEG) throw std::invalid_argument("the key is not a GCM segment key: the segment _reveal_ entry points take keys of zkaes_synthesize_keys_gcm_seg_rv (other reveal keys go through zkaes_encrypt_reveal_batch_seeded_at)");
        if (!c.reveal) throw std::invalid_argument("the key has no reveal region: the segment _reveal_ entry points take keys synthesized with reveal = 1 (zkaes_synthesize_keys_gcm_seg_rv)");
        const size_t hb = zk::mode_header_bytes(c), mb = zk::reveal_mask_bytes(c);
        require_packed(c, n, messages_len, secret_keys_len);
        if (headers_len != n * hb) throw std::invalid_argument("headers must hold n x " + std::to_string(hb) + " bytes (iv, ctr0, Y_in, salt_in, salt_out, length block, aad)");
        if (masks_len != n * mb) throw std::invalid_argument("masks must hold n x " + std::to_string(mb) + " bytes (one bit per message byte of the segment)");
        pack_proofs(pk->pk->prove_gcm_segment_batch(messages, secret_keys, headers, n, pk->pk->contexts(), zk_seed32, first_proof_index, masks, revealed_or_null), proofs, proofs_len, proof_lens);
    });
}
int zkaes_encrypt_gcm_segments_reveal_seeded_at(const uint8_t *msg, size_t len, const uint8_t *key, const uint8_t iv[12], const uint8_t *aad, size_t aad_len, const zkaes_pk *head,
                                                const zkaes_pk *mid_or_null, const zkaes_pk *tail, const uint8_t *salts_or_null, const uint8_t *mask, size_t mask_len, const uint8_t *zk_seed32,
                                                size_t first_segment, size_t count, uint8_t *ciphertext_or_null, uint8_t *tag_or_null, uint8_t *commitments_or_null, uint8_t *revealed_or_null,
                                                uint8_t **proofs, size_t *proofs_len, size_t *proof_lens) {
    return guard([&] {
        if (!head || !tail || !proofs || !proofs_len || !mask) throw std::invalid_argument("null argument");
        if (mask_len != (len + 7) / 8) throw std::invalid_argument("ONE mask over the whole record: " + std::to_string((len + 7) / 8) + " bytes for this message");
        pack_proofs(zk::prove_gcm_segments(head->pk.get(), mid_or_null ? mid_or_null->pk.get() : nullptr, tail->pk.get(), msg, len, key, iv, aad, aad_len, salts_or_null, first_segment, count,
                                           zk_seed32, ciphertext_or_null, tag_or_null, commitments_or_null, mask, revealed_or_null), proofs, proofs_len, proof_lens);
    });
}
// -- digests on segments: keys of a digest record -- head, mid, last (role 3), the closing tail (role 2, units 0) -- and their proving entries; the
// entries above refuse such keys (zkaes_aes_witness_gcm_seg takes them with their longer header), and these refuse every other key
int zkaes_synthesize_keys_gcm_seg_dg(int role, unsigned key_bits, size_t units, size_t aad_len, size_t nc, size_t nv, size_t nnz, unsigned flags, zkaes_pk **pk, zkaes_vk **vk) {
    return guard([&] {
        const unsigned f = key_flags(flags);
        give_keys(zk::synthesize_keys_gcm_segment(role, units, aad_len, key_bits, srs_literals(nc, nv, nnz), f, 0, 0, 1), pk, vk);
    });
}
int zkaes_pk_segment_digest(const zkaes_pk *pk, int *digest, size_t *header_bytes) {
    return guard([&] {
        if (!pk) throw std::invalid_argument("null argument");
        const zk::Circuit &c = pk->pk->circuit();
        if (digest) *digest = c.kind == zk::CIRCUIT_AES_GCM_SEG ? c.seg_digest : 0;
        if (header_bytes) *header_bytes = c.kind == zk::CIRCUIT_AES_GCM_SEG ? zk::segment_header_bytes(c) : 0;
    });
}
int zkaes_encrypt_gcm_segment_digest_batch_seeded_at(size_t n, const uint8_t *messages, size_t messages_len, const uint8_t *secret_keys, size_t secret_keys_len, const uint8_t *headers,
                                                     size_t headers_len, const zkaes_pk *pk, const uint8_t *zk_seed32, uint64_t first_proof_index, uint8_t **proofs, size_t *proofs_len,
                                                     size_t *proof_lens) {
    return guard([&] {
        if (!pk || !proofs || !proofs_len) throw std::invalid_argument("null argument");
        const zk::Circuit &c = pk->pk->circuit();
        if (c.kind != zk::CIRCUIT_AES_GCM_SEG) throw std::invalid_argument("the key is not a GCM segment key: the segment _digest_ entry points take keys of zkaes_synthesize_keys_gcm_seg_dg (other digest keys go through zkaes_encrypt_digest_batch_seeded_at)");
        if (!c.seg_digest) throw std::invalid_argument("the key is a plain segment key: the segment _digest_ entry points take keys of zkaes_synthesize_keys_gcm_seg_dg (this one goes through zkaes_encrypt_gcm_segment_batch_seeded_at)");
        const size_t hb = zk::segment_header_bytes(c);
        require_packed(c, n, messages_len, secret_keys_len);
        if (headers_len != n * hb) throw std::invalid_argument("headers must hold n x " + std::to_string(hb) + " bytes (iv, ctr0, Y_in, salt_in, salt_out, length block, aad, then H_in, then a last's be64(total_bits) padded to 16)");
        pack_proofs(pk->pk->prove_gcm_segment_digest_batch(messages, secret_keys, headers, n, pk->pk->contexts(), zk_seed32, first_proof_index), proofs, proofs_len, proof_lens);
    });
}
int zkaes_encrypt_gcm_segments_digest_seeded_at(const uint8_t *msg, size_t len, const uint8_t *key, const uint8_t iv[12], const uint8_t *aad, size_t aad_len, const zkaes_pk *head,
                                                const zkaes_pk *mid_or_null, const zkaes_pk *last, const zkaes_pk *tail, const uint8_t *salts_or_null, const uint8_t *h_in_or_null,
                                                uint64_t digest_prefix, const uint8_t *zk_seed32, size_t first_segment, size_t count, uint8_t *ciphertext_or_null, uint8_t *tag_or_null,
                                                uint8_t *commitments_or_null, uint8_t *states_or_null, uint8_t **proofs, size_t *proofs_len, size_t *proof_lens) {
    return guard([&] {
        if (!head || !last || !tail || !proofs || !proofs_len) throw std::invalid_argument("null argument");
        pack_proofs(zk::prove_gcm_segments_digest(head->pk.get(), mid_or_null ? mid_or_null->pk.get() : nullptr, last->pk.get(), tail->pk.get(), msg, len, key, iv, aad, aad_len, salts_or_null,
                                                  h_in_or_null, digest_prefix, first_segment, count, zk_seed32, ciphertext_or_null, tag_or_null, commitments_or_null, states_or_null),
                    proofs, proofs_len, proof_lens);
    });
}
// -- plaintext digests: every mode through one set of entries; hdr = the mode's public header, NULL for ECB
int zkaes_aes_witness_pd(const zkaes_pk *pk, const uint8_t *msg, size_t len, const uint8_t *key, const uint8_t *hdr, const uint8_t *h_in, uint8_t *z, size_t z_cap, size_t *z_len) {
    return guard([&] {
        if (!pk) throw std::invalid_argument("null argument");
        give_witness(pk->pk->witness(ANY, true, msg, len, key, hdr, zk::ProvingKey::KEY_AAD, h_in), z, z_cap, z_len);
    });
}
int zkaes_encrypt_digest_batch_seeded_at(size_t n, const uint8_t *messages, size_t messages_len, const uint8_t *secret_keys, size_t secret_keys_len, const uint8_t *headers, size_t headers_len,
                                         const uint8_t *h_ins, const zkaes_pk *pk, const uint8_t *zk_seed32, uint64_t first_proof_index, uint8_t *ciphertexts_or_null, uint8_t *tags_or_null,
                                         uint8_t *h_outs_or_null, uint8_t **proofs, size_t *proofs_len, size_t *proof_lens) {
    return guard([&] {
        if (!pk || !proofs || !proofs_len || (n && (!messages || !secret_keys))) throw std::invalid_argument("null argument");
        const zk::Circuit &c = pk->pk->circuit();
        if (!c.digest_kind && !c.reveal) throw std::invalid_argument("the _digest_ entry points take a proving key synthesized with a digest (digest_kind = 1 or 2)");      // (a reveal key: prove_batch names its entries)
        const size_t hb = zk::mode_header_bytes(c);
        require_packed(c, n, messages_len, secret_keys_len);
        if (headers_len != n * hb || (n && hb && !headers)) throw std::invalid_argument("headers must hold n x " + std::to_string(hb) + " bytes (the mode's public header)");
        pack_proofs(pk->pk->prove_batch(ANY, true, messages, secret_keys, hb ? headers : nullptr, h_ins, n, pk->pk->contexts(), zk_seed32, first_proof_index, ciphertexts_or_null, tags_or_null,
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
        pack_proofs(pk->pk->prove_chunked(ANY, true, msg, len, key, hdr, h_in, pk->pk->contexts(), zk_seed32, first_proof_index, ciphertext_or_null, states_or_null), proofs, proofs_len, proof_lens);
    });
}
// -- selective disclosure: every mode, every digest kind through one set of entries; hdr = the mode's public header, NULL for ECB; h_in(s) are read by a
// key with a digest only
int zkaes_aes_witness_rv(const zkaes_pk *pk, const uint8_t *msg, size_t len, const uint8_t *key, const uint8_t *hdr, const uint8_t *h_in, const uint8_t *mask, size_t mask_len, uint8_t *z,
                         size_t z_cap, size_t *z_len) {
    return guard([&] {
        if (!pk || !mask) throw std::invalid_argument("null argument");
        const zk::Circuit &c = pk->pk->circuit();
        if (!c.reveal) throw std::invalid_argument("the _reveal_ entry points take a proving key synthesized with reveal = 1 (zkaes_synthesize_keys_rv)");
        if (mask_len != zk::reveal_mask_bytes(c)) throw std::invalid_argument("the mask of this key has " + std::to_string(zk::reveal_mask_bytes(c)) + " bytes");
        give_witness(pk->pk->witness(ANY, c.digest_kind != 0, msg, len, key, hdr, zk::ProvingKey::KEY_AAD, h_in, mask), z, z_cap, z_len);
    });
}
int zkaes_encrypt_reveal_batch_seeded_at(size_t n, const uint8_t *messages, size_t messages_len, const uint8_t *secret_keys, size_t secret_keys_len, const uint8_t *headers, size_t headers_len,
                                         const uint8_t *h_ins, const uint8_t *masks, size_t masks_len, const zkaes_pk *pk, const uint8_t *zk_seed32, uint64_t first_proof_index,
                                         uint8_t *ciphertexts_or_null, uint8_t *tags_or_null, uint8_t *h_outs_or_null, uint8_t *revealed_or_null, uint8_t **proofs, size_t *proofs_len,
                                         size_t *proof_lens) {
    return guard([&] {
        if (!pk || !proofs || !proofs_len || !masks || (n && (!messages || !secret_keys))) throw std::invalid_argument("null argument");
        const zk::Circuit &c = pk->pk->circuit();
        if (!c.reveal) throw std::invalid_argument("the _reveal_ entry points take a proving key synthesized with reveal = 1 (zkaes_synthesize_keys_rv)");
        const size_t hb = zk::mode_header_bytes(c), mb = zk::reveal_mask_bytes(c);
        require_packed(c, n, messages_len, secret_keys_len);
        if (headers_len != n * hb || (n && hb && !headers)) throw std::invalid_argument("headers must hold n x " + std::to_string(hb) + " bytes (the mode's public header)");
        if (masks_len != n * mb) throw std::invalid_argument("masks must hold n x " + std::to_string(mb) + " bytes (one bit per message byte)");
        pack_proofs(pk->pk->prove_batch(ANY, c.digest_kind != 0, messages, secret_keys, hb ? headers : nullptr, h_ins, n, pk->pk->contexts(), zk_seed32, first_proof_index, ciphertexts_or_null,
                                        tags_or_null, h_outs_or_null, masks, revealed_or_null), proofs, proofs_len, proof_lens);
    });
}
int zkaes_encrypt_reveal_chunked_seeded_at(const uint8_t *msg, size_t len, const uint8_t *key, const uint8_t *hdr, const uint8_t *h_in, const uint8_t *mask, size_t mask_len, const zkaes_pk *pk,
                                           const uint8_t *zk_seed32, uint64_t first_proof_index, uint8_t *ciphertext_or_null, uint8_t *states_or_null, uint8_t *revealed_or_null, uint8_t **proofs,
                                           size_t *proofs_len, size_t *proof_lens, size_t n_chunks) {
    return guard([&] {
        if (!pk || !proofs || !proofs_len || !key || !msg || !mask) throw std::invalid_argument("null argument");
        const zk::Circuit &c = pk->pk->circuit();
        if (!c.reveal) throw std::invalid_argument("the _reveal_ entry points take a proving key synthesized with reveal = 1 (zkaes_synthesize_keys_rv)");
        const size_t chunk = c.message_bytes;
        if (chunk == 0 || len == 0 || len % chunk || len / chunk != n_chunks) throw std::invalid_argument("message length must be n_chunks * the key's plaintext length");
        if (mask_len != (len + 7) / 8) throw std::invalid_argument("ONE mask over the whole job: " + std::to_string((len + 7) / 8) + " bytes for this message");
        pack_proofs(pk->pk->prove_chunked(ANY, c.digest_kind != 0, msg, len, key, hdr, h_in, pk->pk->contexts(), zk_seed32, first_proof_index, ciphertext_or_null, states_or_null, mask,
                                          revealed_or_null), proofs, proofs_len, proof_lens);
    });
}
int zkaes_prove_ops(const zkaes_pk *pk, uint32_t x, uint32_t y, const uint8_t *seed, uint8_t **proof, size_t *proof_len) {
    return guard([&] {
        if (!pk || !proof || !proof_len) throw std::invalid_argument("null argument");
        give_proof(pk->pk->prove_ops(x, y, seed), proof, proof_len);
    });
}
int zkaes_pk_info(const zkaes_pk *pk, uint64_t out[12]) {
    return guard([&] {
        if (!pk || !out) throw std::invalid_argument("null argument");
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
    return guard([&] {
        if (!pk || !name || !out || !len) throw std::invalid_argument("null argument");
        auto b = pk->pk->debug_fetch(name); *out = give(b); *len = b.size();
    });
}
int zkaes_pk_timings(const zkaes_pk *pk, double out[6]) {
    return guard([&] {
        if (!pk || !out) throw std::invalid_argument("null argument");
        const auto &t = pk->pk->last_timings(); out[0] = t.witness_ms; out[1] = t.round1_ms; out[2] = t.round2_ms; out[3] = t.round3_ms; out[4] = t.open_ms; out[5] = t.total_ms;
    });
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
// ---- batch verification across keys on the device (include/zkaes.h); the host entries are in capi_host.cpp
int zkaes_verify_batch_keys_gpu(const zkaes_vk *const *vks, size_t n_keys, const uint32_t *key_of, const uint8_t *proofs, const size_t *proof_lens, size_t n, const uint8_t *public_input_bits,
                                const size_t *n_bits_each, int *accepted_each, size_t *n_accepted) {
    return guard([&] {
        if (n_accepted) *n_accepted = 0;
        std::unique_ptr<zk::BatchBackend> be = zk::make_device_batch_backend();
        zk::capi::verify_batch_keys_call(vks, n_keys, key_of, proofs, proof_lens, n, public_input_bits, n_bits_each, accepted_each, n_accepted, *be);
    });
}
int zkaes_verify_gcm_segments_batch_gpu(const zkaes_vk *head, const zkaes_vk *mid_or_null, const zkaes_vk *tail, const uint8_t *proofs, const size_t *proof_lens, size_t n_segments, size_t c,
                                        const uint8_t iv[12], const uint8_t *aad, size_t aad_len, const uint8_t *ct, size_t ct_len, const uint8_t tag[16], const uint8_t *commitments,
                                        size_t commitments_len, const uint8_t *mask, size_t mask_len, const uint8_t *revealed, size_t revealed_len, int *accepted_each, size_t *n_accepted) {
    return guard([&] {
        if (n_accepted) *n_accepted = 0;
        std::unique_ptr<zk::BatchBackend> be = zk::make_device_batch_backend();
        zk::capi::verify_gcm_segments_batch_call("verify_gcm_segments_batch_gpu", head, mid_or_null, tail, proofs, proof_lens, n_segments, c, iv, aad, aad_len, ct, ct_len, tag, commitments,
                                                 commitments_len, mask, mask_len, revealed, revealed_len, accepted_each, n_accepted, *be);
    });
}
int zkaes_verify_gcm_segments_batch_kt_gpu(const zkaes_vk *head, const zkaes_vk *mid_or_null, const zkaes_vk *tail, const uint8_t *proofs, const size_t *proof_lens, size_t n_segments, size_t c,
                                           const uint8_t iv[12], const uint8_t *aad, size_t aad_len, const uint8_t *ct, size_t ct_len, const uint8_t tag[16], const uint8_t *commitments,
                                           size_t commitments_len, const uint8_t *key_tag, size_t key_tag_len, const uint8_t *mask, size_t mask_len, const uint8_t *revealed,
                                           size_t revealed_len, int *accepted_each, size_t *n_accepted) {
    return guard([&] {
        if (n_accepted) *n_accepted = 0;
        if (accepted_each) for (size_t s = 0; s < n_segments; s++) accepted_each[s] = 0;
        if (!key_tag) throw std::invalid_argument("null argument");
        std::unique_ptr<zk::BatchBackend> be = zk::make_device_batch_backend();
        zk::capi::verify_gcm_segments_batch_call("verify_gcm_segments_batch_kt_gpu", head, mid_or_null, tail, proofs, proof_lens, n_segments, c, iv, aad, aad_len, ct, ct_len, tag, commitments,
                                                 commitments_len, mask, mask_len, revealed, revealed_len, accepted_each, n_accepted, *be, key_tag, key_tag_len);
    });
}
// the keyed public-input kernel, one launch per call (tests/test_gpu_verify_batch_keys.py): key k has the domain 2^lg_m[k] and rows of n_bits[k] 0/1 bytes, row i belongs
// to key key_of[i] and follows row i - 1 in bits
int zkaes_public_input_eval_keyed(const int *lg_m, const size_t *n_bits, size_t n_keys, const uint32_t *key_of, const uint8_t *betas, const uint8_t *bits, size_t n, uint8_t *out) {
    return guard([&] {
        if (!lg_m || !n_bits || !key_of || !betas || !out) throw std::invalid_argument("null argument");
        if (n_keys == 0 || n_keys > ((size_t)1 << 16) || n == 0 || n > ((size_t)1 << 20)) throw std::invalid_argument("zkaes_public_input_eval_keyed: 1 .. 2^16 keys, 1 .. 2^20 rows");
        for (size_t k = 0; k < n_keys; k++)
            if (lg_m[k] < 0 || lg_m[k] > 30 || n_bits[k] >= ((size_t)1 << lg_m[k])) throw std::invalid_argument("zkaes_public_input_eval_keyed: rows of fewer than 2^lg_m bits, lg_m <= 30");
        std::vector<zk::Fr> b(n), o(n);
        std::vector<size_t> off(n);
        size_t total = 0;
        for (size_t i = 0; i < n; i++) {
            if (key_of[i] >= n_keys) throw std::invalid_argument("zkaes_public_input_eval_keyed: key index out of range");
            memcpy(b[i].l, betas + 32 * i, 32);
            if (zk::Fr::geq_mod(b[i].l)) throw std::invalid_argument("zkaes_public_input_eval_keyed: limbs not below the modulus");
            off[i] = total; total += n_bits[key_of[i]];
        }
        if (total && !bits) throw std::invalid_argument("null argument");
        std::unique_ptr<zk::BatchBackend> be = zk::make_device_batch_backend();
        be->public_input_eval_keyed(lg_m, n_bits, n_keys, key_of, b.data(), bits, off.data(), n, o.data());
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
