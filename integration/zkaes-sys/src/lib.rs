//! Bindings + safe wrappers for libzkaes (include/zkaes.h): the MI355X implementation of zk_aes::{synthesize_keys, encrypt, verify_encryption}.
//!
//! In `zk-aes` the three functions of src/lib.rs (:60, :116, :138) become one-liners over `zkaes_sys::{synthesize_keys, encrypt,
//! verify_encryption}`; proofs cross the boundary as the ark-serialize bytes of `ark_marlin::Proof`, verifying keys (optionally) as the
//! ark-serialize bytes of `IndexVerifierKey` (`VerifyingKey::to_ark_bytes`), the proving key stays a device-resident handle.
use anyhow::{anyhow, Result};
use std::ffi::CStr;
use std::os::raw::{c_char, c_int, c_uint};
use std::sync::Arc;

#[repr(C)]
pub struct zkaes_pk { _private: [u8; 0] }
#[repr(C)]
pub struct zkaes_vk { _private: [u8; 0] }

extern "C" {
    fn zkaes_last_error() -> *const c_char;
    fn zkaes_bytes_free(p: *mut u8);
    fn zkaes_pk_free(pk: *mut zkaes_pk);
    fn zkaes_vk_free(vk: *mut zkaes_vk);
    fn zkaes_synthesize_keys(plaintext_length: usize, pk: *mut *mut zkaes_pk, vk: *mut *mut zkaes_vk) -> c_int;
    fn zkaes_synthesize_keys_ex2(circuit_kind: c_int, plaintext_length: usize, srs_num_constraints: usize, srs_num_variables: usize, srs_num_non_zero: usize, flags: c_uint,
                                 pk: *mut *mut zkaes_pk, vk: *mut *mut zkaes_vk) -> c_int;
    fn zkaes_encrypt(message: *const u8, message_len: usize, secret_key: *const u8, pk: *const zkaes_pk, proof: *mut *mut u8, proof_len: *mut usize) -> c_int;
    fn zkaes_verify_encryption(vk: *const zkaes_vk, proof: *const u8, proof_len: usize, ciphertext: *const u8, ciphertext_len: usize, accepted: *mut c_int) -> c_int;
    fn zkaes_encrypt_chunked(message: *const u8, message_len: usize, secret_key: *const u8, pk: *const zkaes_pk, proofs: *mut *mut u8, proofs_len: *mut usize,
                             proof_lens: *mut usize, n_chunks: usize) -> c_int;
    fn zkaes_encrypt_chunked_seeded_at(message: *const u8, message_len: usize, secret_key: *const u8, pk: *const zkaes_pk, zk_seed32: *const u8, first_proof_index: u64,
                                       proofs: *mut *mut u8, proofs_len: *mut usize, proof_lens: *mut usize, n_chunks: usize) -> c_int;
    fn zkaes_pk_serialize_ark_to_file_ex(pk: *const zkaes_pk, path: *const c_char, uncompressed: c_int, bytes_written: *mut u64) -> c_int;
    fn zkaes_pk_set_contexts(pk: *mut zkaes_pk, n: usize) -> c_int;
    fn zkaes_pk_get_contexts(pk: *const zkaes_pk, n: *mut usize) -> c_int;
    fn zkaes_srs_hold(hold: c_int) -> c_int;
    fn zkaes_set_default_contexts(n: usize) -> c_int;
    fn zkaes_pk_srs_info(pk: *const zkaes_pk, out: *mut u64, secs: *mut f64) -> c_int;
    fn zkaes_pk_tables_built(pk: *const zkaes_pk, built: *mut c_int, table_bytes: *mut u64) -> c_int;
    fn zkaes_vk_serialize_ark(vk: *const zkaes_vk, out: *mut *mut u8, out_len: *mut usize) -> c_int;
    fn zkaes_vk_deserialize_ark(bytes: *const u8, len: usize, vk: *mut *mut zkaes_vk) -> c_int;
    // AES-128-CBC (include/zkaes.h, section "AES-128-CBC"; these declarations and the wrappers below were not compiled: no cargo in the build image)
    fn zkaes_cbc_ciphertext(message: *const u8, message_len: usize, secret_key: *const u8, iv: *const u8, ciphertext: *mut u8) -> c_int;
    fn zkaes_encrypt_cbc_seeded(message: *const u8, message_len: usize, secret_key: *const u8, iv: *const u8, pk: *const zkaes_pk, zk_seed32: *const u8,
                                ciphertext_or_null: *mut u8, proof: *mut *mut u8, proof_len: *mut usize) -> c_int;
    fn zkaes_encrypt_cbc_chunked(message: *const u8, message_len: usize, secret_key: *const u8, iv: *const u8, pk: *const zkaes_pk, ciphertext_or_null: *mut u8,
                                 proofs: *mut *mut u8, proofs_len: *mut usize, proof_lens: *mut usize, n_chunks: usize) -> c_int;
    fn zkaes_encrypt_cbc_chunked_seeded_at(message: *const u8, message_len: usize, secret_key: *const u8, iv: *const u8, pk: *const zkaes_pk, zk_seed32: *const u8,
                                           first_proof_index: u64, ciphertext_or_null: *mut u8, proofs: *mut *mut u8, proofs_len: *mut usize, proof_lens: *mut usize,
                                           n_chunks: usize) -> c_int;
    fn zkaes_aes_witness_cbc(pk: *const zkaes_pk, message: *const u8, message_len: usize, secret_key: *const u8, iv: *const u8, z: *mut u8, z_cap: usize, z_len: *mut usize) -> c_int;
    fn zkaes_verify_encryption_cbc(vk: *const zkaes_vk, proof: *const u8, proof_len: usize, iv: *const u8, ciphertext: *const u8, ciphertext_len: usize,
                                   accepted: *mut c_int) -> c_int;
    fn zkaes_verify_cbc_chunked(vk: *const zkaes_vk, proofs: *const u8, proof_lens: *const usize, n_chunks: usize, iv: *const u8, ciphertext: *const u8, ciphertext_len: usize,
                                accepted_each: *mut c_int, n_accepted: *mut usize) -> c_int;
    // AES-128-CTR (include/zkaes.h, section "AES-128-CTR"; these declarations and the wrappers below were not compiled: no cargo in the build image)
    fn zkaes_ctr_crypt(input: *const u8, len: usize, secret_key: *const u8, icb: *const u8, out: *mut u8) -> c_int;
    fn zkaes_ctr_counter_add(icb: *const u8, n_blocks: u64, out16: *mut u8) -> c_int;
    fn zkaes_encrypt_ctr_seeded(message: *const u8, message_len: usize, secret_key: *const u8, icb: *const u8, pk: *const zkaes_pk, zk_seed32: *const u8,
                                ciphertext_or_null: *mut u8, proof: *mut *mut u8, proof_len: *mut usize) -> c_int;
    fn zkaes_encrypt_ctr_chunked(message: *const u8, message_len: usize, secret_key: *const u8, icb: *const u8, pk: *const zkaes_pk, ciphertext_or_null: *mut u8,
                                 proofs: *mut *mut u8, proofs_len: *mut usize, proof_lens: *mut usize, n_chunks: usize) -> c_int;
    fn zkaes_encrypt_ctr_chunked_seeded_at(message: *const u8, message_len: usize, secret_key: *const u8, icb: *const u8, pk: *const zkaes_pk, zk_seed32: *const u8,
                                           first_proof_index: u64, ciphertext_or_null: *mut u8, proofs: *mut *mut u8, proofs_len: *mut usize, proof_lens: *mut usize,
                                           n_chunks: usize) -> c_int;
    fn zkaes_aes_witness_ctr(pk: *const zkaes_pk, message: *const u8, message_len: usize, secret_key: *const u8, icb: *const u8, z: *mut u8, z_cap: usize, z_len: *mut usize) -> c_int;
    fn zkaes_verify_encryption_ctr(vk: *const zkaes_vk, proof: *const u8, proof_len: usize, icb: *const u8, ciphertext: *const u8, ciphertext_len: usize,
                                   accepted: *mut c_int) -> c_int;
    fn zkaes_verify_ctr_chunked(vk: *const zkaes_vk, proofs: *const u8, proof_lens: *const usize, n_chunks: usize, icb: *const u8, ciphertext: *const u8, ciphertext_len: usize,
                                accepted_each: *mut c_int, n_accepted: *mut usize) -> c_int;
    // AES-128-GCM (include/zkaes.h, section "AES-128-GCM"; these declarations and the wrappers below were not compiled: no cargo in the build image)
    fn zkaes_synthesize_keys_gcm(plaintext_length: usize, aad_length: usize, srs_num_constraints: usize, srs_num_variables: usize, srs_num_non_zero: usize, flags: c_uint,
                                 pk: *mut *mut zkaes_pk, vk: *mut *mut zkaes_vk) -> c_int;
    fn zkaes_gcm_encrypt(message: *const u8, message_len: usize, secret_key: *const u8, iv12: *const u8, aad: *const u8, aad_len: usize, ciphertext: *mut u8, tag16: *mut u8) -> c_int;
    fn zkaes_gcm_decrypt(ciphertext: *const u8, ciphertext_len: usize, secret_key: *const u8, iv12: *const u8, aad: *const u8, aad_len: usize, tag16: *const u8, message: *mut u8,
                         ok: *mut c_int) -> c_int;
    fn zkaes_encrypt_gcm_seeded(message: *const u8, message_len: usize, secret_key: *const u8, iv12: *const u8, aad: *const u8, aad_len: usize, pk: *const zkaes_pk,
                                zk_seed32: *const u8, ciphertext_or_null: *mut u8, tag_or_null: *mut u8, proof: *mut *mut u8, proof_len: *mut usize) -> c_int;
    fn zkaes_encrypt_gcm_batch_seeded_at(n: usize, messages: *const u8, messages_len: usize, secret_keys: *const u8, secret_keys_len: usize, headers: *const u8, headers_len: usize,
                                         pk: *const zkaes_pk, zk_seed32: *const u8, first_proof_index: u64, ciphertexts_or_null: *mut u8, tags_or_null: *mut u8,
                                         proofs: *mut *mut u8, proofs_len: *mut usize, proof_lens: *mut usize) -> c_int;
    fn zkaes_aes_witness_gcm(pk: *const zkaes_pk, message: *const u8, message_len: usize, secret_key: *const u8, iv12: *const u8, aad: *const u8, aad_len: usize, z: *mut u8,
                             z_cap: usize, z_len: *mut usize) -> c_int;
    fn zkaes_verify_encryption_gcm(vk: *const zkaes_vk, proof: *const u8, proof_len: usize, iv12: *const u8, aad: *const u8, aad_len: usize, ciphertext: *const u8,
                                   ciphertext_len: usize, tag16: *const u8, accepted: *mut c_int) -> c_int;
    // AES-192 / AES-256 (include/zkaes.h, section "AES-192 and AES-256"; these declarations and the wrappers at the end of the file were not compiled: no cargo in the build image)
    fn zkaes_synthesize_keys_ks(circuit_kind: c_int, key_bits: c_uint, plaintext_length: usize, aad_length: usize, srs_num_constraints: usize, srs_num_variables: usize,
                                srs_num_non_zero: usize, flags: c_uint, pk: *mut *mut zkaes_pk, vk: *mut *mut zkaes_vk) -> c_int;
    fn zkaes_pk_key_bytes(pk: *const zkaes_pk, n: *mut usize) -> c_int;
    fn zkaes_circuit_info_ks(circuit_kind: c_int, key_bits: c_uint, plaintext_length: usize, aad_length: usize, out: *mut u64) -> c_int;
    fn zkaes_circuit_matrix_ks(circuit_kind: c_int, key_bits: c_uint, plaintext_length: usize, aad_length: usize, which: c_int, n_rows: *mut u64, nnz: *mut u64, rowptr: *mut u32,
                               col: *mut u32, coeff: *mut i64) -> c_int;
    fn zkaes_ecb_ciphertext_ks(message: *const u8, message_len: usize, secret_key: *const u8, key_len: usize, ciphertext: *mut u8) -> c_int;
    fn zkaes_cbc_ciphertext_ks(message: *const u8, message_len: usize, secret_key: *const u8, key_len: usize, iv: *const u8, ciphertext: *mut u8) -> c_int;
    fn zkaes_ctr_crypt_ks(input: *const u8, len: usize, secret_key: *const u8, key_len: usize, icb: *const u8, out: *mut u8) -> c_int;
    fn zkaes_gcm_encrypt_ks(message: *const u8, message_len: usize, secret_key: *const u8, key_len: usize, iv12: *const u8, aad: *const u8, aad_len: usize, ciphertext: *mut u8,
                            tag16: *mut u8) -> c_int;
    fn zkaes_gcm_decrypt_ks(ciphertext: *const u8, ciphertext_len: usize, secret_key: *const u8, key_len: usize, iv12: *const u8, aad: *const u8, aad_len: usize, tag16: *const u8,
                            message: *mut u8, ok: *mut c_int) -> c_int;
    // key tags (include/zkaes.h, section "Key tags"; these declarations and the wrappers at the end of the file were not compiled: no cargo in the build image)
    fn zkaes_synthesize_keys_kt(circuit_kind: c_int, key_bits: c_uint, key_tag_blocks: c_uint, plaintext_length: usize, aad_length: usize, srs_num_constraints: usize,
                                srs_num_variables: usize, srs_num_non_zero: usize, flags: c_uint, pk: *mut *mut zkaes_pk, vk: *mut *mut zkaes_vk) -> c_int;
    fn zkaes_pk_key_tag_blocks(pk: *const zkaes_pk, n: *mut usize) -> c_int;
    fn zkaes_key_tag(secret_key: *const u8, key_len: usize, tag_blocks: usize, out: *mut u8) -> c_int;
    fn zkaes_circuit_info_kt(circuit_kind: c_int, key_bits: c_uint, key_tag_blocks: c_uint, plaintext_length: usize, aad_length: usize, out: *mut u64) -> c_int;
    fn zkaes_circuit_matrix_kt(circuit_kind: c_int, key_bits: c_uint, key_tag_blocks: c_uint, plaintext_length: usize, aad_length: usize, which: c_int, n_rows: *mut u64, nnz: *mut u64,
                               rowptr: *mut u32, col: *mut u32, coeff: *mut i64) -> c_int;
    fn zkaes_verify_chunked_kt(vk: *const zkaes_vk, circuit_kind: c_int, proofs: *const u8, proof_lens: *const usize, n_chunks: usize, iv_or_icb: *const u8, ciphertext: *const u8,
                               ciphertext_len: usize, key_tag: *const u8, key_tag_len: usize, accepted_each: *mut c_int, n_accepted: *mut usize) -> c_int;
    fn zkaes_verify_encryption_gcm_kt(vk: *const zkaes_vk, proof: *const u8, proof_len: usize, iv12: *const u8, aad: *const u8, aad_len: usize, ciphertext: *const u8,
                                      ciphertext_len: usize, tag16: *const u8, key_tag: *const u8, key_tag_len: usize, accepted: *mut c_int) -> c_int;
    // plaintext digests (include/zkaes.h, section "plaintext digests"; declarations only, no wrappers yet, and not compiled: no cargo in the build image).  digest_kind: 0 none,
    // 1 chain, 2 final; a state (h_in, h_out, an entry of states) is 32 bytes and a null h_in is SHA-256's initial value
    fn zkaes_synthesize_keys_pd(circuit_kind: c_int, key_bits: c_uint, key_tag_blocks: c_uint, digest_kind: c_uint, digest_prefix: u64, plaintext_length: usize, aad_length: usize,
                                srs_num_constraints: usize, srs_num_variables: usize, srs_num_non_zero: usize, flags: c_uint, pk: *mut *mut zkaes_pk, vk: *mut *mut zkaes_vk) -> c_int;
    fn zkaes_circuit_info_pd(circuit_kind: c_int, key_bits: c_uint, key_tag_blocks: c_uint, digest_kind: c_uint, digest_prefix: u64, plaintext_length: usize, aad_length: usize,
                             out: *mut u64) -> c_int;
    fn zkaes_circuit_matrix_pd(circuit_kind: c_int, key_bits: c_uint, key_tag_blocks: c_uint, digest_kind: c_uint, digest_prefix: u64, plaintext_length: usize, aad_length: usize,
                               which: c_int, n_rows: *mut u64, nnz: *mut u64, rowptr: *mut u32, col: *mut u32, coeff: *mut i64) -> c_int;
    fn zkaes_pk_digest_info(pk: *const zkaes_pk, out: *mut u64) -> c_int;
    fn zkaes_pk_mode(pk: *const zkaes_pk, circuit_kind: *mut c_int, header_bytes: *mut usize) -> c_int;
    fn zkaes_sha256_chain(h_in: *const u8, data: *const u8, len: usize, h_out: *mut u8) -> c_int;
    fn zkaes_sha256_finish(h_in: *const u8, prefix_bytes: u64, tail: *const u8, tail_len: usize, digest: *mut u8) -> c_int;
    fn zkaes_aes_witness_pd(pk: *const zkaes_pk, msg: *const u8, len: usize, secret_key: *const u8, hdr: *const u8, h_in: *const u8, z: *mut u8, z_cap: usize, z_len: *mut usize) -> c_int;
    fn zkaes_encrypt_digest_batch_seeded_at(n: usize, messages: *const u8, messages_len: usize, secret_keys: *const u8, secret_keys_len: usize, headers: *const u8, headers_len: usize,
                                            h_ins: *const u8, pk: *const zkaes_pk, zk_seed32: *const u8, first_proof_index: u64, ciphertexts_or_null: *mut u8, tags_or_null: *mut u8,
                                            h_outs_or_null: *mut u8, proofs: *mut *mut u8, proofs_len: *mut usize, proof_lens: *mut usize) -> c_int;
    fn zkaes_encrypt_digest_chunked_seeded_at(msg: *const u8, len: usize, secret_key: *const u8, hdr: *const u8, h_in: *const u8, pk: *const zkaes_pk, zk_seed32: *const u8,
                                              first_proof_index: u64, ciphertext_or_null: *mut u8, states_or_null: *mut u8, proofs: *mut *mut u8, proofs_len: *mut usize,
                                              proof_lens: *mut usize, n_chunks: usize) -> c_int;
    fn zkaes_verify_digest_chunked(vk: *const zkaes_vk, circuit_kind: c_int, proofs: *const u8, proof_lens: *const usize, n_chunks: usize, iv_or_icb: *const u8, ciphertext: *const u8,
                                   ciphertext_len: usize, key_tag: *const u8, key_tag_len: usize, states: *const u8, accepted_each: *mut c_int, n_accepted: *mut usize) -> c_int;
    fn zkaes_verify_encryption_gcm_digest(vk: *const zkaes_vk, proof: *const u8, proof_len: usize, iv12: *const u8, aad: *const u8, aad_len: usize, ciphertext: *const u8,
                                          ciphertext_len: usize, tag16: *const u8, key_tag: *const u8, key_tag_len: usize, h_in: *const u8, h_out: *const u8, accepted: *mut c_int) -> c_int;
    // selective disclosure (include/zkaes.h, section "selective disclosure"; declarations only, no wrappers yet, and not compiled: no cargo in the build image).  reveal: 0 or 1;
    // a mask over L bytes is ceil(L / 8) bytes, bit i = bit i % 8 of byte i / 8; revealed is L bytes
    fn zkaes_synthesize_keys_rv(circuit_kind: c_int, key_bits: c_uint, key_tag_blocks: c_uint, digest_kind: c_uint, digest_prefix: u64, reveal: c_uint, plaintext_length: usize,
                                aad_length: usize, srs_num_constraints: usize, srs_num_variables: usize, srs_num_non_zero: usize, flags: c_uint, pk: *mut *mut zkaes_pk,
                                vk: *mut *mut zkaes_vk) -> c_int;
    fn zkaes_circuit_info_rv(circuit_kind: c_int, key_bits: c_uint, key_tag_blocks: c_uint, digest_kind: c_uint, digest_prefix: u64, reveal: c_uint, plaintext_length: usize,
                             aad_length: usize, out: *mut u64) -> c_int;
    fn zkaes_circuit_matrix_rv(circuit_kind: c_int, key_bits: c_uint, key_tag_blocks: c_uint, digest_kind: c_uint, digest_prefix: u64, reveal: c_uint, plaintext_length: usize,
                               aad_length: usize, which: c_int, n_rows: *mut u64, nnz: *mut u64, rowptr: *mut u32, col: *mut u32, coeff: *mut i64) -> c_int;
    fn zkaes_pk_reveal_info(pk: *const zkaes_pk, out: *mut u64) -> c_int;
    fn zkaes_reveal_bytes(msg: *const u8, len: usize, mask: *const u8, mask_len: usize, out: *mut u8) -> c_int;
    fn zkaes_aes_witness_rv(pk: *const zkaes_pk, msg: *const u8, len: usize, secret_key: *const u8, hdr: *const u8, h_in: *const u8, mask: *const u8, mask_len: usize, z: *mut u8,
                            z_cap: usize, z_len: *mut usize) -> c_int;
    fn zkaes_encrypt_reveal_batch_seeded_at(n: usize, messages: *const u8, messages_len: usize, secret_keys: *const u8, secret_keys_len: usize, headers: *const u8, headers_len: usize,
                                            h_ins: *const u8, masks: *const u8, masks_len: usize, pk: *const zkaes_pk, zk_seed32: *const u8, first_proof_index: u64,
                                            ciphertexts_or_null: *mut u8, tags_or_null: *mut u8, h_outs_or_null: *mut u8, revealed_or_null: *mut u8, proofs: *mut *mut u8,
                                            proofs_len: *mut usize, proof_lens: *mut usize) -> c_int;
    fn zkaes_encrypt_reveal_chunked_seeded_at(msg: *const u8, len: usize, secret_key: *const u8, hdr: *const u8, h_in: *const u8, mask: *const u8, mask_len: usize, pk: *const zkaes_pk,
                                              zk_seed32: *const u8, first_proof_index: u64, ciphertext_or_null: *mut u8, states_or_null: *mut u8, revealed_or_null: *mut u8,
                                              proofs: *mut *mut u8, proofs_len: *mut usize, proof_lens: *mut usize, n_chunks: usize) -> c_int;
    fn zkaes_verify_reveal_chunked(vk: *const zkaes_vk, circuit_kind: c_int, proofs: *const u8, proof_lens: *const usize, n_chunks: usize, iv_or_icb: *const u8, ciphertext: *const u8,
                                   ciphertext_len: usize, key_tag: *const u8, key_tag_len: usize, states: *const u8, mask: *const u8, mask_len: usize, revealed: *const u8,
                                   accepted_each: *mut c_int, n_accepted: *mut usize) -> c_int;
    fn zkaes_verify_encryption_gcm_reveal(vk: *const zkaes_vk, proof: *const u8, proof_len: usize, iv12: *const u8, aad: *const u8, aad_len: usize, ciphertext: *const u8,
                                          ciphertext_len: usize, tag16: *const u8, key_tag: *const u8, key_tag_len: usize, h_in: *const u8, h_out: *const u8, mask: *const u8,
                                          mask_len: usize, revealed: *const u8, accepted: *mut c_int) -> c_int;
    fn zkaes_chunk_public_inputs_rv(circuit_kind: c_int, n_chunks: usize, iv_or_icb: *const u8, ciphertext: *const u8, ciphertext_len: usize, key_tag: *const u8, key_tag_len: usize,
                                    states: *const u8, mask: *const u8, mask_len: usize, revealed: *const u8, out_bits: *mut u8, n_bits: *mut usize) -> c_int;
    // GCM records longer than one proof (include/zkaes.h, section "segment-proofs"; declarations only, no wrappers yet, and not compiled: no cargo in the build image).  role: 0 head,
    // 1 mid, 2 tail; units = c data blocks (head, mid) or Lt bytes (tail); a commitment is 32 bytes, a Y and a salt 16; a segment header is 80 + A bytes
    fn zkaes_synthesize_keys_gcm_seg(role: c_int, key_bits: c_uint, units: usize, aad_length: usize, srs_num_constraints: usize, srs_num_variables: usize, srs_num_non_zero: usize,
                                     flags: c_uint, pk: *mut *mut zkaes_pk, vk: *mut *mut zkaes_vk) -> c_int;
    fn zkaes_pk_segment_info(pk: *const zkaes_pk, out: *mut u64) -> c_int;
    fn zkaes_circuit_info_gcm_seg(role: c_int, key_bits: c_uint, units: usize, aad_length: usize, out: *mut u64) -> c_int;
    fn zkaes_circuit_matrix_gcm_seg(role: c_int, key_bits: c_uint, units: usize, aad_length: usize, which: c_int, n_rows: *mut u64, nnz: *mut u64, rowptr: *mut u32, col: *mut u32,
                                    coeff: *mut i64) -> c_int;
    fn zkaes_gcm_boundaries(message: *const u8, message_len: usize, secret_key: *const u8, key_len: usize, iv12: *const u8, aad: *const u8, aad_len: usize, c: usize, ys: *mut u8,
                            ys_cap: usize, n_segments: *mut usize) -> c_int;
    fn zkaes_gcm_commit(secret_key: *const u8, key_len: usize, y16: *const u8, salt16: *const u8, commitment32: *mut u8) -> c_int;
    fn zkaes_aes_witness_gcm_seg(pk: *const zkaes_pk, message: *const u8, message_len: usize, secret_key: *const u8, header: *const u8, header_len: usize, z: *mut u8, z_cap: usize,
                                 z_len: *mut usize) -> c_int;
    fn zkaes_encrypt_gcm_segment_batch_seeded_at(n: usize, messages: *const u8, messages_len: usize, secret_keys: *const u8, secret_keys_len: usize, headers: *const u8, headers_len: usize,
                                                 pk: *const zkaes_pk, zk_seed32: *const u8, first_proof_index: u64, proofs: *mut *mut u8, proofs_len: *mut usize, proof_lens: *mut usize) -> c_int;
    fn zkaes_encrypt_gcm_segments_seeded_at(message: *const u8, message_len: usize, secret_key: *const u8, iv12: *const u8, aad: *const u8, aad_len: usize, head: *const zkaes_pk,
                                            mid_or_null: *const zkaes_pk, tail: *const zkaes_pk, salts_or_null: *const u8, zk_seed32: *const u8, first_segment: usize, count: usize,
                                            ciphertext_or_null: *mut u8, tag_or_null: *mut u8, commitments_or_null: *mut u8, proofs: *mut *mut u8, proofs_len: *mut usize,
                                            proof_lens: *mut usize) -> c_int;
    fn zkaes_verify_gcm_segments(head: *const zkaes_vk, mid_or_null: *const zkaes_vk, tail: *const zkaes_vk, proofs: *const u8, proof_lens: *const usize, n_segments: usize, c: usize,
                                 iv12: *const u8, aad: *const u8, aad_len: usize, ciphertext: *const u8, ciphertext_len: usize, tag16: *const u8, commitments: *const u8,
                                 commitments_len: usize, accepted_each: *mut c_int, n_accepted: *mut usize) -> c_int;
    // selective disclosure on segmented records (include/zkaes.h, the section behind "segment-proofs"; declarations only, no wrappers yet, and not compiled: no cargo in
    // the build image).  ONE mask of ceil(L / 8) bytes and ONE revealed array of L bytes over the record; a segment's own mask is ceil(len / 8) bytes
    fn zkaes_synthesize_keys_gcm_seg_rv(role: c_int, key_bits: c_uint, reveal: c_uint, units: usize, aad_length: usize, srs_num_constraints: usize, srs_num_variables: usize,
                                        srs_num_non_zero: usize, flags: c_uint, pk: *mut *mut zkaes_pk, vk: *mut *mut zkaes_vk) -> c_int;
    fn zkaes_circuit_info_gcm_seg_rv(role: c_int, key_bits: c_uint, reveal: c_uint, units: usize, aad_length: usize, out: *mut u64) -> c_int;
    fn zkaes_circuit_matrix_gcm_seg_rv(role: c_int, key_bits: c_uint, reveal: c_uint, units: usize, aad_length: usize, which: c_int, n_rows: *mut u64, nnz: *mut u64, rowptr: *mut u32,
                                       col: *mut u32, coeff: *mut i64) -> c_int;
    fn zkaes_aes_witness_gcm_seg_rv(pk: *const zkaes_pk, message: *const u8, message_len: usize, secret_key: *const u8, header: *const u8, header_len: usize, mask: *const u8,
                                    mask_len: usize, z: *mut u8, z_cap: usize, z_len: *mut usize) -> c_int;
    fn zkaes_encrypt_gcm_segment_reveal_batch_seeded_at(n: usize, messages: *const u8, messages_len: usize, secret_keys: *const u8, secret_keys_len: usize, headers: *const u8,
                                                        headers_len: usize, masks: *const u8, masks_len: usize, pk: *const zkaes_pk, zk_seed32: *const u8, first_proof_index: u64,
                                                        revealed_or_null: *mut u8, proofs: *mut *mut u8, proofs_len: *mut usize, proof_lens: *mut usize) -> c_int;
    fn zkaes_encrypt_gcm_segments_reveal_seeded_at(message: *const u8, message_len: usize, secret_key: *const u8, iv12: *const u8, aad: *const u8, aad_len: usize, head: *const zkaes_pk,
                                                   mid_or_null: *const zkaes_pk, tail: *const zkaes_pk, salts_or_null: *const u8, mask: *const u8, mask_len: usize, zk_seed32: *const u8,
                                                   first_segment: usize, count: usize, ciphertext_or_null: *mut u8, tag_or_null: *mut u8, commitments_or_null: *mut u8,
                                                   revealed_or_null: *mut u8, proofs: *mut *mut u8, proofs_len: *mut usize, proof_lens: *mut usize) -> c_int;
    fn zkaes_verify_gcm_segments_reveal(head: *const zkaes_vk, mid_or_null: *const zkaes_vk, tail: *const zkaes_vk, proofs: *const u8, proof_lens: *const usize, n_segments: usize,
                                        c: usize, iv12: *const u8, aad: *const u8, aad_len: usize, ciphertext: *const u8, ciphertext_len: usize, tag16: *const u8,
                                        commitments: *const u8, commitments_len: usize, mask: *const u8, mask_len: usize, revealed: *const u8, revealed_len: usize,
                                        accepted_each: *mut c_int, n_accepted: *mut usize) -> c_int;
    // key tags on segmented records (include/zkaes.h, "key tags on segmented GCM records"; declarations only, no wrappers yet, and not compiled: no cargo in the build
    // image).  A HEAD key takes key_tag_blocks = 0, 1 or 2, a mid or tail 0 only; the verifiers take key_tag != NULL of 16 or 32 bytes and mask = NULL for plain keys
    fn zkaes_synthesize_keys_gcm_seg_kt(role: c_int, key_bits: c_uint, reveal: c_uint, key_tag_blocks: c_uint, units: usize, aad_length: usize, srs_num_constraints: usize,
                                        srs_num_variables: usize, srs_num_non_zero: usize, flags: c_uint, pk: *mut *mut zkaes_pk, vk: *mut *mut zkaes_vk) -> c_int;
    fn zkaes_circuit_info_gcm_seg_kt(role: c_int, key_bits: c_uint, reveal: c_uint, key_tag_blocks: c_uint, units: usize, aad_length: usize, out: *mut u64) -> c_int;
    fn zkaes_circuit_matrix_gcm_seg_kt(role: c_int, key_bits: c_uint, reveal: c_uint, key_tag_blocks: c_uint, units: usize, aad_length: usize, which: c_int, n_rows: *mut u64,
                                       nnz: *mut u64, rowptr: *mut u32, col: *mut u32, coeff: *mut i64) -> c_int;
    fn zkaes_gcm_segment_public_inputs_kt(n_segments: usize, c: usize, iv12: *const u8, aad: *const u8, aad_len: usize, ciphertext: *const u8, ciphertext_len: usize, tag16: *const u8,
                                          commitments: *const u8, commitments_len: usize, key_tag: *const u8, key_tag_len: usize, mask: *const u8, mask_len: usize,
                                          revealed: *const u8, out_bits: *mut u8, n_bits_each: *mut usize, roles: *mut c_int) -> c_int;
    fn zkaes_verify_gcm_segments_kt(head: *const zkaes_vk, mid_or_null: *const zkaes_vk, tail: *const zkaes_vk, proofs: *const u8, proof_lens: *const usize, n_segments: usize, c: usize,
                                    iv12: *const u8, aad: *const u8, aad_len: usize, ciphertext: *const u8, ciphertext_len: usize, tag16: *const u8, commitments: *const u8,
                                    commitments_len: usize, key_tag: *const u8, key_tag_len: usize, mask: *const u8, mask_len: usize, revealed: *const u8, revealed_len: usize,
                                    accepted_each: *mut c_int, n_accepted: *mut usize) -> c_int;
    fn zkaes_verify_gcm_segments_batch_kt(head: *const zkaes_vk, mid_or_null: *const zkaes_vk, tail: *const zkaes_vk, proofs: *const u8, proof_lens: *const usize, n_segments: usize,
                                          c: usize, iv12: *const u8, aad: *const u8, aad_len: usize, ciphertext: *const u8, ciphertext_len: usize, tag16: *const u8,
                                          commitments: *const u8, commitments_len: usize, key_tag: *const u8, key_tag_len: usize, mask: *const u8, mask_len: usize,
                                          revealed: *const u8, revealed_len: usize, accepted_each: *mut c_int, n_accepted: *mut usize) -> c_int;
    fn zkaes_verify_gcm_segments_batch_kt_gpu(head: *const zkaes_vk, mid_or_null: *const zkaes_vk, tail: *const zkaes_vk, proofs: *const u8, proof_lens: *const usize, n_segments: usize,
                                              c: usize, iv12: *const u8, aad: *const u8, aad_len: usize, ciphertext: *const u8, ciphertext_len: usize, tag16: *const u8,
                                              commitments: *const u8, commitments_len: usize, key_tag: *const u8, key_tag_len: usize, mask: *const u8, mask_len: usize,
                                              revealed: *const u8, revealed_len: usize, accepted_each: *mut c_int, n_accepted: *mut usize) -> c_int;
    // digests on segmented records (include/zkaes.h, "digests on segmented GCM records"; declarations only, no wrappers yet, and not compiled: no cargo in the build
    // image).  Roles 0 head, 1 mid, 3 last (units = the last data segment's bytes), 2 tail with units = 0; a record is nd data segments and the closing tail
    fn zkaes_synthesize_keys_gcm_seg_dg(role: c_int, key_bits: c_uint, units: usize, aad_length: usize, srs_num_constraints: usize, srs_num_variables: usize, srs_num_non_zero: usize,
                                        flags: c_uint, pk: *mut *mut zkaes_pk, vk: *mut *mut zkaes_vk) -> c_int;
    fn zkaes_pk_segment_digest(pk: *const zkaes_pk, digest: *mut c_int, header_bytes: *mut usize) -> c_int;
    fn zkaes_encrypt_gcm_segment_digest_batch_seeded_at(n: usize, messages: *const u8, messages_len: usize, secret_keys: *const u8, secret_keys_len: usize, headers: *const u8,
                                                        headers_len: usize, pk: *const zkaes_pk, zk_seed32: *const u8, first_proof_index: u64, proofs: *mut *mut u8, proofs_len: *mut usize,
                                                        proof_lens: *mut usize) -> c_int;
    fn zkaes_encrypt_gcm_segments_digest_seeded_at(message: *const u8, message_len: usize, secret_key: *const u8, iv12: *const u8, aad: *const u8, aad_len: usize, head: *const zkaes_pk,
                                                   mid_or_null: *const zkaes_pk, last: *const zkaes_pk, tail: *const zkaes_pk, salts_or_null: *const u8, h_in_or_null: *const u8,
                                                   digest_prefix: u64, zk_seed32: *const u8, first_segment: usize, count: usize, ciphertext_or_null: *mut u8, tag_or_null: *mut u8,
                                                   commitments_or_null: *mut u8, states_or_null: *mut u8, proofs: *mut *mut u8, proofs_len: *mut usize, proof_lens: *mut usize) -> c_int;
    fn zkaes_circuit_info_gcm_seg_dg(role: c_int, key_bits: c_uint, units: usize, aad_length: usize, out: *mut u64) -> c_int;
    fn zkaes_circuit_matrix_gcm_seg_dg(role: c_int, key_bits: c_uint, units: usize, aad_length: usize, which: c_int, n_rows: *mut u64, nnz: *mut u64, rowptr: *mut u32, col: *mut u32,
                                       coeff: *mut i64) -> c_int;
    fn zkaes_gcm_digest_plan(message: *const u8, message_len: usize, secret_key: *const u8, key_len: usize, iv12: *const u8, aad: *const u8, aad_len: usize, c: usize,
                             h_in_or_null: *const u8, digest_prefix: u64, ys: *mut u8, ys_cap: usize, states: *mut u8, states_cap: usize, n_data_segments: *mut usize) -> c_int;
    fn zkaes_gcm_segment_digest_public_inputs(n_proofs: usize, c: usize, iv12: *const u8, aad: *const u8, aad_len: usize, ciphertext: *const u8, ciphertext_len: usize, tag16: *const u8,
                                              commitments: *const u8, commitments_len: usize, states: *const u8, states_len: usize, digest_prefix: u64, out_bits: *mut u8,
                                              n_bits_each: *mut usize, roles: *mut c_int) -> c_int;
    fn zkaes_verify_gcm_segments_digest(head: *const zkaes_vk, mid_or_null: *const zkaes_vk, last: *const zkaes_vk, tail: *const zkaes_vk, proofs: *const u8, proof_lens: *const usize,
                                        n_proofs: usize, c: usize, iv12: *const u8, aad: *const u8, aad_len: usize, ciphertext: *const u8, ciphertext_len: usize, tag16: *const u8,
                                        commitments: *const u8, commitments_len: usize, states: *const u8, states_len: usize, digest_prefix: u64, accepted_each: *mut c_int,
                                        n_accepted: *mut usize) -> c_int;
    // kernel-level entries of the kernels that build a key (include/zkaes.h, "kernels that BUILD A KEY": test surface, not product API; declarations only, no wrappers, and
    // not compiled: no cargo in the build image).  A point is 96 bytes of affine x || y in Montgomery form, infinity 96 zero bytes; a field element 32 bytes; a Niels record
    // 192 bytes; every output of zkaes_index_evals holds 2^lg_k + 64 elements
    fn zkaes_fixed_base_powers(curve_id: c_int, base_xy: *const u8, beta: *const u8, from: u64, count: usize, chunk: usize, out: *mut u8) -> c_int;
    fn zkaes_fixed_base_scalars(base_xy: *const u8, scalars: *const u8, count: usize, chunk: usize, out: *mut u8) -> c_int;
    fn zkaes_table_next(curve_id: c_int, prev: *const u8, count: usize, window_bits: c_int, j: c_int, out: *mut u8) -> c_int;
    fn zkaes_build_window_tables(curve_id: c_int, bases: *const u8, n: usize, window_bits: c_int, out: *mut u8) -> c_int;
    fn zkaes_convert_bases_te(src: *const u8, n: usize, out: *mut u8) -> c_int;
    fn zkaes_index_evals(ci: *const u32, ri: *const u32, ca: *const i64, cb: *const i64, cc: *const i64, cnt: usize, lg_k: c_int, lg_n: c_int, row: *mut u8, col: *mut u8,
                         rowcol: *mut u8, va: *mut u8, vb: *mut u8, vc: *mut u8, uinv_or_null: *mut u8) -> c_int;
}

fn last_error() -> anyhow::Error {
    // thread-local message of the failing call (mirrors the anyhow::Error the reference returns)
    let msg = unsafe { CStr::from_ptr(zkaes_last_error()) }.to_string_lossy().into_owned();
    anyhow!(msg)
}
fn take_bytes(p: *mut u8, n: usize) -> Vec<u8> {
    let v = unsafe { std::slice::from_raw_parts(p, n) }.to_vec();
    unsafe { zkaes_bytes_free(p) };
    v
}

struct PkHandle(*mut zkaes_pk);
struct VkHandle(*mut zkaes_vk);
// the handles are immutable after synthesis and libzkaes serialises access to its prover contexts internally
unsafe impl Send for PkHandle {}
unsafe impl Sync for PkHandle {}
unsafe impl Send for VkHandle {}
unsafe impl Sync for VkHandle {}
impl Drop for PkHandle { fn drop(&mut self) { unsafe { zkaes_pk_free(self.0) } } }
impl Drop for VkHandle { fn drop(&mut self) { unsafe { zkaes_vk_free(self.0) } } }

/// Keys are passed by value in the reference API and callers `.clone()` them per call (tests/integration_tests.rs:330): Clone = Arc clone.
#[derive(Clone)]
pub struct ProvingKey(Arc<PkHandle>);
#[derive(Clone)]
pub struct VerifyingKey(Arc<VkHandle>);

impl ProvingKey {
    /// Streams the ark-serialize image of the arkworks `IndexProverKey` this key corresponds to, to run the reference's CPU `encrypt()` (src/lib.rs:60) on a GPU-made key.
    /// `uncompressed = true` (1.25 GB for a 16-byte key, 96-byte points): read it back with `ProvingKey::deserialize_unchecked(BufReader::new(File::open(path)?))` --
    /// in ark-serialize 0.3 `deserialize_unchecked` reads the UNCOMPRESSED layout and does no per-point work.  `uncompressed = false` (0.65 GB, 48-byte points) is what
    /// `ProvingKey::serialize` writes: read it with `ProvingKey::deserialize` (a square root and a subgroup check per SRS point -- tens of minutes for a 64-byte key).
    pub fn serialize_ark_to_file(&self, path: &std::path::Path, uncompressed: bool) -> Result<u64> {
        let c = std::ffi::CString::new(path.to_string_lossy().as_bytes()).map_err(|_| anyhow::anyhow!("path contains a NUL byte"))?;
        let mut n = 0u64;
        if unsafe { zkaes_pk_serialize_ark_to_file_ex((self.0).0, c.as_ptr(), uncompressed as c_int, &mut n) } != 0 { return Err(last_error()); }
        Ok(n)
    }
    /// Proofs in flight per `encrypt_chunked` call on this key (1..=64; 0 = the process default, 12).  Replaces the ZKAES_CONTEXTS environment round-trip.
    pub fn set_contexts(&self, n: usize) -> Result<()> {
        if unsafe { zkaes_pk_set_contexts((self.0).0, n) } != 0 { return Err(last_error()); }
        Ok(())
    }
    pub fn contexts(&self) -> Result<usize> {
        let mut n = 0usize;
        if unsafe { zkaes_pk_get_contexts((self.0).0, &mut n) } != 0 { return Err(last_error()); }
        Ok(n)
    }
    /// The universal SRS behind the key -- ONE per process, device and SRS literals, as `generate_universal_srs` at src/lib.rs:139-141 is one for every circuit size:
    /// (max_degree, points per copy, copies, device bytes, keys sharing it now, Lagrange-basis bytes)
    pub fn srs_info(&self) -> Result<[u64; 6]> {
        let mut out = [0u64; 6];
        if unsafe { zkaes_pk_srs_info((self.0).0, out.as_mut_ptr(), std::ptr::null_mut()) } != 0 { return Err(last_error()); }
        Ok(out)
    }
    /// (built, bytes): whether the key holds the fixed-base window tables of its SRS (skipped under KEY_NO_TABLES or when device memory is short)
    pub fn tables_built(&self) -> Result<(bool, u64)> {
        let (mut b, mut n) = (0 as c_int, 0u64);
        if unsafe { zkaes_pk_tables_built((self.0).0, &mut b, &mut n) } != 0 { return Err(last_error()); }
        Ok((b != 0, n))
    }
}

impl VerifyingKey {
    /// ark-serialize bytes of `ark_marlin::IndexVerifierKey` -- feed to `simpleworks::marlin::VerifyingKey::deserialize`
    pub fn to_ark_bytes(&self) -> Result<Vec<u8>> {
        let (mut p, mut n) = (std::ptr::null_mut(), 0usize);
        if unsafe { zkaes_vk_serialize_ark((self.0).0, &mut p, &mut n) } != 0 { return Err(last_error()); }
        Ok(take_bytes(p, n))
    }
    pub fn from_ark_bytes(bytes: &[u8]) -> Result<Self> {
        let mut vk = std::ptr::null_mut();
        if unsafe { zkaes_vk_deserialize_ark(bytes.as_ptr(), bytes.len(), &mut vk) } != 0 { return Err(last_error()); }
        Ok(VerifyingKey(Arc::new(VkHandle(vk))))
    }
}

/// zk_aes::synthesize_keys (src/lib.rs:138)
pub fn synthesize_keys(plaintext_length: usize) -> Result<(ProvingKey, VerifyingKey)> {
    let (mut pk, mut vk) = (std::ptr::null_mut(), std::ptr::null_mut());
    if unsafe { zkaes_synthesize_keys(plaintext_length, &mut pk, &mut vk) } != 0 { return Err(last_error()); }
    Ok((ProvingKey(Arc::new(PkHandle(pk))), VerifyingKey(Arc::new(VkHandle(vk)))))
}

/// Key synthesis options (include/zkaes.h ZKAES_KEY_*)
pub const KEY_NO_TABLES: u32 = 1;   // this key does not use (or build) the window tables of the universal SRS (31.4 GB, shared by all keys); multi-proof calls run ~9 % slower

/// `synthesize_keys` with options: `flags` = KEY_NO_TABLES to keep the key small (the tables are also skipped automatically when the device is short of memory)
pub fn synthesize_keys_with(plaintext_length: usize, flags: u32) -> Result<(ProvingKey, VerifyingKey)> {
    let (mut pk, mut vk) = (std::ptr::null_mut(), std::ptr::null_mut());
    // circuit kind 0 = the AES circuit; the universal-SRS literals of src/lib.rs:141
    if unsafe { zkaes_synthesize_keys_ex2(0, plaintext_length, 866_944, 513, 4_062_064, flags as c_uint, &mut pk, &mut vk) } != 0 { return Err(last_error()); }
    Ok((ProvingKey(Arc::new(PkHandle(pk))), VerifyingKey(Arc::new(VkHandle(vk)))))
}

/// The process default of prover contexts per key (0 = back to ZKAES_CONTEXTS / 12); lower it before synthesizing keys for much larger chunk sizes (see include/zkaes.h).
pub fn set_default_contexts(n: usize) -> Result<()> {
    if unsafe { zkaes_set_default_contexts(n) } != 0 { return Err(last_error()); }
    Ok(())
}

/// Keep the universal SRS (31.4 GB of window tables for the reference's literals) resident after the last key over it is dropped; `false` releases it again.
/// For callers that create and drop keys in turn (one key per request size): without it every first key over an idle SRS rebuilds the tables (~1.5 s).
pub fn srs_hold(hold: bool) -> Result<()> {
    if unsafe { zkaes_srs_hold(hold as c_int) } != 0 { return Err(last_error()); }
    Ok(())
}

/// zk_aes::encrypt (src/lib.rs:60): returns the ark-serialize bytes of the MarlinProof (`deserialize_proof(bytes)` gives the arkworks type)
pub fn encrypt(message: &[u8], secret_key: &[u8; 16], proving_key: &ProvingKey) -> Result<Vec<u8>> {
    let (mut p, mut n) = (std::ptr::null_mut(), 0usize);
    if unsafe { zkaes_encrypt(message.as_ptr(), message.len(), secret_key.as_ptr(), (proving_key.0).0, &mut p, &mut n) } != 0 { return Err(last_error()); }
    Ok(take_bytes(p, n))
}

/// zk_aes::verify_encryption (src/lib.rs:116): Ok(false) for a wrong ciphertext, Err only for malformed input
pub fn verify_encryption(verifying_key: &VerifyingKey, proof: &[u8], ciphertext: &[u8]) -> Result<bool> {
    let mut accepted: c_int = 0;
    if unsafe { zkaes_verify_encryption((verifying_key.0).0, proof.as_ptr(), proof.len(), ciphertext.as_ptr(), ciphertext.len(), &mut accepted) } != 0 { return Err(last_error()); }
    Ok(accepted != 0)
}

/// Prover randomness of a multi-proof call
pub enum ZkSeed<'a> {
    /// a fresh 32-byte seed from the operating system per call (the default of the C entry point): zero-knowledge across proofs
    Fresh,
    /// caller's seed; proof i of the call draws from StdRng(Blake2s(seed || (first_proof_index + i))) -- a job split over several calls / ranks under one
    /// seed passes the job-global index of each call's first proof
    Seeded { seed: &'a [u8; 32], first_proof_index: u64 },
    /// the reference's fixed `test_rng` stream in EVERY proof (src/lib.rs:65): byte-parity with the CPU path, NOT zero-knowledge across proofs -- tests only
    ReferenceParity,
}

/// Long ECB messages (not in the reference API: its SRS literal caps one proof at 96 bytes): ceil(len / chunk) independent chunk-proofs on the key of
/// `chunk` bytes, many in flight on the GPU (ECB blocks are independent, src/lib.rs:194).
pub fn encrypt_chunked(message: &[u8], secret_key: &[u8; 16], proving_key: &ProvingKey, chunk_len: usize, zk_seed: ZkSeed) -> Result<Vec<Vec<u8>>> {
    if chunk_len == 0 || message.len() % chunk_len != 0 { return Err(anyhow!("message length must be a multiple of the key's plaintext length")); }
    let n = message.len() / chunk_len;
    let (mut p, mut total) = (std::ptr::null_mut(), 0usize);
    let mut lens = vec![0usize; n.max(1)];
    let rc = match zk_seed {
        ZkSeed::Fresh => unsafe { zkaes_encrypt_chunked(message.as_ptr(), message.len(), secret_key.as_ptr(), (proving_key.0).0, &mut p, &mut total, lens.as_mut_ptr(), n) },
        ZkSeed::Seeded { seed, first_proof_index } => unsafe {
            zkaes_encrypt_chunked_seeded_at(message.as_ptr(), message.len(), secret_key.as_ptr(), (proving_key.0).0, seed.as_ptr(), first_proof_index, &mut p, &mut total, lens.as_mut_ptr(), n)
        },
        ZkSeed::ReferenceParity => unsafe {
            zkaes_encrypt_chunked_seeded_at(message.as_ptr(), message.len(), secret_key.as_ptr(), (proving_key.0).0, std::ptr::null(), 0, &mut p, &mut total, lens.as_mut_ptr(), n)
        },
    };
    if rc != 0 { return Err(last_error()); }
    let blob = take_bytes(p, total);
    let mut out = Vec::with_capacity(n);
    let mut off = 0;
    for l in lens.iter().take(n) { out.push(blob[off..off + l].to_vec()); off += l; }
    Ok(out)
}

// ---- AES-128-CBC (not in the reference API; its README names CBC as the mode to follow ECB).  NOT COMPILED: no cargo in the build image.
/// include/zkaes.h ZKAES_CIRCUIT_AES_CBC
pub const CIRCUIT_AES_CBC: c_int = 3;

/// A key for CBC chunks of `chunk_len` bytes (a non-zero multiple of 16) over the universal-SRS literals of src/lib.rs:141
pub fn synthesize_keys_cbc(chunk_len: usize, flags: u32) -> Result<(ProvingKey, VerifyingKey)> {
    let (mut pk, mut vk) = (std::ptr::null_mut(), std::ptr::null_mut());
    if unsafe { zkaes_synthesize_keys_ex2(CIRCUIT_AES_CBC, chunk_len, 866_944, 513, 4_062_064, flags as c_uint, &mut pk, &mut vk) } != 0 { return Err(last_error()); }
    Ok((ProvingKey(Arc::new(PkHandle(pk))), VerifyingKey(Arc::new(VkHandle(vk)))))
}

/// AES-128-CBC of whole blocks on the host (no GPU): the ciphertext, and the source of each call's `iv` when one job is split over several calls or ranks
pub fn cbc_ciphertext(message: &[u8], secret_key: &[u8; 16], iv: &[u8; 16]) -> Result<Vec<u8>> {
    let mut ct = vec![0u8; message.len()];
    if unsafe { zkaes_cbc_ciphertext(message.as_ptr(), message.len(), secret_key.as_ptr(), iv.as_ptr(), ct.as_mut_ptr()) } != 0 { return Err(last_error()); }
    Ok(ct)
}

/// One proof that `ciphertext` is the CBC encryption under `iv` of a hidden message with a hidden key: (ciphertext, proof bytes).  `zk_seed = None`: the fixed test_rng stream
pub fn encrypt_cbc(message: &[u8], secret_key: &[u8; 16], iv: &[u8; 16], proving_key: &ProvingKey, zk_seed: Option<&[u8; 32]>) -> Result<(Vec<u8>, Vec<u8>)> {
    let mut ct = vec![0u8; message.len().max(1)];
    let (mut p, mut n) = (std::ptr::null_mut(), 0usize);
    let seed = zk_seed.map_or(std::ptr::null(), |s| s.as_ptr());
    if unsafe { zkaes_encrypt_cbc_seeded(message.as_ptr(), message.len(), secret_key.as_ptr(), iv.as_ptr(), (proving_key.0).0, seed, ct.as_mut_ptr(), &mut p, &mut n) } != 0 {
        return Err(last_error());
    }
    ct.truncate(message.len());
    Ok((ct, take_bytes(p, n)))
}

/// Long CBC messages: (ciphertext, chunk-proofs).  `iv` = the chaining value entering this call's first chunk; the chunks are independent statements because every
/// chaining value is a public ciphertext block, so they are proven side by side exactly as `encrypt_chunked`'s.
pub fn encrypt_cbc_chunked(message: &[u8], secret_key: &[u8; 16], iv: &[u8; 16], proving_key: &ProvingKey, chunk_len: usize, zk_seed: ZkSeed) -> Result<(Vec<u8>, Vec<Vec<u8>>)> {
    if chunk_len == 0 || message.is_empty() || message.len() % chunk_len != 0 { return Err(anyhow!("message length must be a non-zero multiple of the key's plaintext length")); }
    let n = message.len() / chunk_len;
    let mut ct = vec![0u8; message.len()];
    let (mut p, mut total) = (std::ptr::null_mut(), 0usize);
    let mut lens = vec![0usize; n];
    let (m, k, v, pk) = (message.as_ptr(), secret_key.as_ptr(), iv.as_ptr(), (proving_key.0).0);
    let rc = match zk_seed {
        ZkSeed::Fresh => unsafe { zkaes_encrypt_cbc_chunked(m, message.len(), k, v, pk, ct.as_mut_ptr(), &mut p, &mut total, lens.as_mut_ptr(), n) },
        ZkSeed::Seeded { seed, first_proof_index } => unsafe {
            zkaes_encrypt_cbc_chunked_seeded_at(m, message.len(), k, v, pk, seed.as_ptr(), first_proof_index, ct.as_mut_ptr(), &mut p, &mut total, lens.as_mut_ptr(), n)
        },
        ZkSeed::ReferenceParity => unsafe {
            zkaes_encrypt_cbc_chunked_seeded_at(m, message.len(), k, v, pk, std::ptr::null(), 0, ct.as_mut_ptr(), &mut p, &mut total, lens.as_mut_ptr(), n)
        },
    };
    if rc != 0 { return Err(last_error()); }
    let blob = take_bytes(p, total);
    let mut out = Vec::with_capacity(n);
    let mut off = 0;
    for l in lens.iter() { out.push(blob[off..off + l].to_vec()); off += l; }
    Ok((ct, out))
}

/// z (padded instance + witness, one byte per variable) of a CBC key
pub fn aes_witness_cbc(proving_key: &ProvingKey, message: &[u8], secret_key: &[u8; 16], iv: &[u8; 16]) -> Result<Vec<u8>> {
    let mut n = 0usize;
    let pk = (proving_key.0).0;
    if unsafe { zkaes_aes_witness_cbc(pk, message.as_ptr(), message.len(), secret_key.as_ptr(), iv.as_ptr(), std::ptr::null_mut(), 0, &mut n) } != 0 { return Err(last_error()); }
    let mut z = vec![0u8; n];
    if unsafe { zkaes_aes_witness_cbc(pk, message.as_ptr(), message.len(), secret_key.as_ptr(), iv.as_ptr(), z.as_mut_ptr(), n, &mut n) } != 0 { return Err(last_error()); }
    Ok(z)
}

/// Ok(false) for a wrong IV or ciphertext, Err only for malformed input
pub fn verify_encryption_cbc(verifying_key: &VerifyingKey, proof: &[u8], iv: &[u8; 16], ciphertext: &[u8]) -> Result<bool> {
    let mut accepted: c_int = 0;
    if unsafe { zkaes_verify_encryption_cbc((verifying_key.0).0, proof.as_ptr(), proof.len(), iv.as_ptr(), ciphertext.as_ptr(), ciphertext.len(), &mut accepted) } != 0 {
        return Err(last_error());
    }
    Ok(accepted != 0)
}

/// One verdict per chunk-proof; chunk j is checked under `iv` (j = 0) or the 16 ciphertext bytes ahead of its slice -- derived here, from public data alone
pub fn verify_cbc_chunked(verifying_key: &VerifyingKey, proofs: &[Vec<u8>], iv: &[u8; 16], ciphertext: &[u8]) -> Result<Vec<bool>> {
    let blob: Vec<u8> = proofs.iter().flat_map(|p| p.iter().copied()).collect();
    let lens: Vec<usize> = proofs.iter().map(|p| p.len()).collect();
    let mut each = vec![0 as c_int; proofs.len().max(1)];
    let mut ok = 0usize;
    if unsafe { zkaes_verify_cbc_chunked((verifying_key.0).0, blob.as_ptr(), lens.as_ptr(), proofs.len(), iv.as_ptr(), ciphertext.as_ptr(), ciphertext.len(), each.as_mut_ptr(), &mut ok) } != 0 {
        return Err(last_error());
    }
    Ok(each.iter().take(proofs.len()).map(|&a| a != 0).collect())
}

// ---- AES-128-CTR (not in the reference API; counter mode is the encryption half of the GCM its README names).  NOT COMPILED: no cargo in the build image.
/// include/zkaes.h ZKAES_CIRCUIT_AES_CTR
pub const CIRCUIT_AES_CTR: c_int = 4;

/// A key for CTR statements of `len` bytes (any value >= 1; a multiple of 16 for the chunked call) over the universal-SRS literals of src/lib.rs:141
pub fn synthesize_keys_ctr(len: usize, flags: u32) -> Result<(ProvingKey, VerifyingKey)> {
    let (mut pk, mut vk) = (std::ptr::null_mut(), std::ptr::null_mut());
    if unsafe { zkaes_synthesize_keys_ex2(CIRCUIT_AES_CTR, len, 866_944, 513, 4_062_064, flags as c_uint, &mut pk, &mut vk) } != 0 { return Err(last_error()); }
    Ok((ProvingKey(Arc::new(PkHandle(pk))), VerifyingKey(Arc::new(VkHandle(vk)))))
}

/// AES-128-CTR of any length >= 1 on the host (no GPU); encrypts and decrypts.  The counter is one big-endian 128-bit integer (SP 800-38A B.1), not GCM's inc32
pub fn ctr_crypt(data: &[u8], secret_key: &[u8; 16], icb: &[u8; 16]) -> Result<Vec<u8>> {
    let mut out = vec![0u8; data.len()];
    if unsafe { zkaes_ctr_crypt(data.as_ptr(), data.len(), secret_key.as_ptr(), icb.as_ptr(), out.as_mut_ptr()) } != 0 { return Err(last_error()); }
    Ok(out)
}

/// icb + n_blocks mod 2^128: the counter of the block `n_blocks` behind icb's, i.e. the `icb` of a call or rank that starts there
pub fn ctr_counter_add(icb: &[u8; 16], n_blocks: u64) -> Result<[u8; 16]> {
    let mut out = [0u8; 16];
    if unsafe { zkaes_ctr_counter_add(icb.as_ptr(), n_blocks, out.as_mut_ptr()) } != 0 { return Err(last_error()); }
    Ok(out)
}

/// One proof that `ciphertext` is the CTR encryption from counter `icb` of a hidden message with a hidden key: (ciphertext, proof bytes).  `zk_seed = None`: the fixed test_rng stream
pub fn encrypt_ctr(message: &[u8], secret_key: &[u8; 16], icb: &[u8; 16], proving_key: &ProvingKey, zk_seed: Option<&[u8; 32]>) -> Result<(Vec<u8>, Vec<u8>)> {
    let mut ct = vec![0u8; message.len().max(1)];
    let (mut p, mut n) = (std::ptr::null_mut(), 0usize);
    let seed = zk_seed.map_or(std::ptr::null(), |s| s.as_ptr());
    if unsafe { zkaes_encrypt_ctr_seeded(message.as_ptr(), message.len(), secret_key.as_ptr(), icb.as_ptr(), (proving_key.0).0, seed, ct.as_mut_ptr(), &mut p, &mut n) } != 0 {
        return Err(last_error());
    }
    ct.truncate(message.len());
    Ok((ct, take_bytes(p, n)))
}

/// Long CTR messages: (ciphertext, chunk-proofs) over a key for `chunk_len` bytes (a multiple of 16).  Chunk j is proven under icb + j * chunk_len / 16; `icb` is the
/// counter of this call's first block, so any slice of a job can be proven on its own from `ctr_counter_add(icb, blocks before)`.
pub fn encrypt_ctr_chunked(message: &[u8], secret_key: &[u8; 16], icb: &[u8; 16], proving_key: &ProvingKey, chunk_len: usize, zk_seed: ZkSeed) -> Result<(Vec<u8>, Vec<Vec<u8>>)> {
    if chunk_len == 0 || chunk_len % 16 != 0 || message.is_empty() || message.len() % chunk_len != 0 {
        return Err(anyhow!("message length must be a non-zero multiple of the key's plaintext length, itself a multiple of 16"));
    }
    let n = message.len() / chunk_len;
    let mut ct = vec![0u8; message.len()];
    let (mut p, mut total) = (std::ptr::null_mut(), 0usize);
    let mut lens = vec![0usize; n];
    let (m, k, v, pk) = (message.as_ptr(), secret_key.as_ptr(), icb.as_ptr(), (proving_key.0).0);
    let rc = match zk_seed {
        ZkSeed::Fresh => unsafe { zkaes_encrypt_ctr_chunked(m, message.len(), k, v, pk, ct.as_mut_ptr(), &mut p, &mut total, lens.as_mut_ptr(), n) },
        ZkSeed::Seeded { seed, first_proof_index } => unsafe {
            zkaes_encrypt_ctr_chunked_seeded_at(m, message.len(), k, v, pk, seed.as_ptr(), first_proof_index, ct.as_mut_ptr(), &mut p, &mut total, lens.as_mut_ptr(), n)
        },
        ZkSeed::ReferenceParity => unsafe {
            zkaes_encrypt_ctr_chunked_seeded_at(m, message.len(), k, v, pk, std::ptr::null(), 0, ct.as_mut_ptr(), &mut p, &mut total, lens.as_mut_ptr(), n)
        },
    };
    if rc != 0 { return Err(last_error()); }
    let blob = take_bytes(p, total);
    let mut out = Vec::with_capacity(n);
    let mut off = 0;
    for l in lens.iter() { out.push(blob[off..off + l].to_vec()); off += l; }
    Ok((ct, out))
}

/// z (padded instance + witness, one byte per variable) of a CTR key
pub fn aes_witness_ctr(proving_key: &ProvingKey, message: &[u8], secret_key: &[u8; 16], icb: &[u8; 16]) -> Result<Vec<u8>> {
    let mut n = 0usize;
    let pk = (proving_key.0).0;
    if unsafe { zkaes_aes_witness_ctr(pk, message.as_ptr(), message.len(), secret_key.as_ptr(), icb.as_ptr(), std::ptr::null_mut(), 0, &mut n) } != 0 { return Err(last_error()); }
    let mut z = vec![0u8; n];
    if unsafe { zkaes_aes_witness_ctr(pk, message.as_ptr(), message.len(), secret_key.as_ptr(), icb.as_ptr(), z.as_mut_ptr(), n, &mut n) } != 0 { return Err(last_error()); }
    Ok(z)
}

/// Ok(false) for a wrong counter or ciphertext; Err for malformed input, which includes a ciphertext whose length is not the key's (the length is part of the statement)
pub fn verify_encryption_ctr(verifying_key: &VerifyingKey, proof: &[u8], icb: &[u8; 16], ciphertext: &[u8]) -> Result<bool> {
    let mut accepted: c_int = 0;
    if unsafe { zkaes_verify_encryption_ctr((verifying_key.0).0, proof.as_ptr(), proof.len(), icb.as_ptr(), ciphertext.as_ptr(), ciphertext.len(), &mut accepted) } != 0 {
        return Err(last_error());
    }
    Ok(accepted != 0)
}

/// One verdict per chunk-proof; chunk j is checked under icb + j * (blocks per chunk) -- derived here, from (icb, j) alone
pub fn verify_ctr_chunked(verifying_key: &VerifyingKey, proofs: &[Vec<u8>], icb: &[u8; 16], ciphertext: &[u8]) -> Result<Vec<bool>> {
    let blob: Vec<u8> = proofs.iter().flat_map(|p| p.iter().copied()).collect();
    let lens: Vec<usize> = proofs.iter().map(|p| p.len()).collect();
    let mut each = vec![0 as c_int; proofs.len().max(1)];
    let mut ok = 0usize;
    if unsafe { zkaes_verify_ctr_chunked((verifying_key.0).0, blob.as_ptr(), lens.as_ptr(), proofs.len(), icb.as_ptr(), ciphertext.as_ptr(), ciphertext.len(), each.as_mut_ptr(), &mut ok) } != 0 {
        return Err(last_error());
    }
    Ok(each.iter().take(proofs.len()).map(|&a| a != 0).collect())
}

// ---- AES-128-GCM (not in the reference API; its README names the mode).  96-bit IVs and full tags only.  NOT COMPILED: no cargo in the build image.
/// include/zkaes.h ZKAES_CIRCUIT_AES_GCM
pub const CIRCUIT_AES_GCM: c_int = 5;

/// A key for GCM records of exactly `len` message bytes (>= 1) and `aad_len` aad bytes (>= 0) over the universal-SRS literals of src/lib.rs:141 (they hold up to 64 bytes)
pub fn synthesize_keys_gcm(len: usize, aad_len: usize, flags: u32) -> Result<(ProvingKey, VerifyingKey)> {
    let (mut pk, mut vk) = (std::ptr::null_mut(), std::ptr::null_mut());
    if unsafe { zkaes_synthesize_keys_gcm(len, aad_len, 866_944, 513, 4_062_064, flags as c_uint, &mut pk, &mut vk) } != 0 { return Err(last_error()); }
    Ok((ProvingKey(Arc::new(PkHandle(pk))), VerifyingKey(Arc::new(VkHandle(vk)))))
}

/// AES-128-GCM on the host (no GPU): (ciphertext, tag)
pub fn gcm_encrypt(message: &[u8], secret_key: &[u8; 16], iv: &[u8; 12], aad: &[u8]) -> Result<(Vec<u8>, [u8; 16])> {
    let mut ct = vec![0u8; message.len().max(1)];
    let mut tag = [0u8; 16];
    if unsafe { zkaes_gcm_encrypt(message.as_ptr(), message.len(), secret_key.as_ptr(), iv.as_ptr(), aad.as_ptr(), aad.len(), ct.as_mut_ptr(), tag.as_mut_ptr()) } != 0 {
        return Err(last_error());
    }
    ct.truncate(message.len());
    Ok((ct, tag))
}

/// Ok(None) when the tag does not hold: no plaintext leaves the library then
pub fn gcm_decrypt(ciphertext: &[u8], secret_key: &[u8; 16], iv: &[u8; 12], aad: &[u8], tag: &[u8; 16]) -> Result<Option<Vec<u8>>> {
    let mut msg = vec![0u8; ciphertext.len().max(1)];
    let mut ok: c_int = 0;
    if unsafe { zkaes_gcm_decrypt(ciphertext.as_ptr(), ciphertext.len(), secret_key.as_ptr(), iv.as_ptr(), aad.as_ptr(), aad.len(), tag.as_ptr(), msg.as_mut_ptr(), &mut ok) } != 0 {
        return Err(last_error());
    }
    msg.truncate(ciphertext.len());
    Ok(if ok != 0 { Some(msg) } else { None })
}

/// One proof that (ciphertext, tag) is the GCM encryption under `iv` and `aad` of a hidden message with a hidden key: (ciphertext, tag, proof bytes)
pub fn encrypt_gcm(message: &[u8], secret_key: &[u8; 16], iv: &[u8; 12], aad: &[u8], proving_key: &ProvingKey, zk_seed: Option<&[u8; 32]>) -> Result<(Vec<u8>, [u8; 16], Vec<u8>)> {
    let mut ct = vec![0u8; message.len().max(1)];
    let mut tag = [0u8; 16];
    let (mut p, mut n) = (std::ptr::null_mut(), 0usize);
    let seed = zk_seed.map_or(std::ptr::null(), |s| s.as_ptr());
    if unsafe {
        zkaes_encrypt_gcm_seeded(message.as_ptr(), message.len(), secret_key.as_ptr(), iv.as_ptr(), aad.as_ptr(), aad.len(), (proving_key.0).0, seed, ct.as_mut_ptr(), tag.as_mut_ptr(), &mut p, &mut n)
    } != 0 {
        return Err(last_error());
    }
    ct.truncate(message.len());
    Ok((ct, tag, take_bytes(p, n)))
}

/// n independent records over one key: `messages` n x L bytes, `secret_keys` n x 16, `headers` n x (12 + A) bytes (each record's iv, then its aad).
/// Returns (ciphertexts n x L, tags n x 16, proofs).  `seed` and `first_proof_index` as in the ECB batch call
pub fn encrypt_gcm_batch(n: usize, messages: &[u8], secret_keys: &[u8], headers: &[u8], proving_key: &ProvingKey, seed: &[u8; 32], first_proof_index: u64) -> Result<(Vec<u8>, Vec<u8>, Vec<Vec<u8>>)> {
    let mut cts = vec![0u8; messages.len().max(1)];
    let mut tags = vec![0u8; (16 * n).max(1)];
    let (mut p, mut total) = (std::ptr::null_mut(), 0usize);
    let mut lens = vec![0usize; n.max(1)];
    if unsafe {
        zkaes_encrypt_gcm_batch_seeded_at(n, messages.as_ptr(), messages.len(), secret_keys.as_ptr(), secret_keys.len(), headers.as_ptr(), headers.len(), (proving_key.0).0, seed.as_ptr(),
                                          first_proof_index, cts.as_mut_ptr(), tags.as_mut_ptr(), &mut p, &mut total, lens.as_mut_ptr())
    } != 0 {
        return Err(last_error());
    }
    let blob = take_bytes(p, total);
    let mut out = Vec::with_capacity(n);
    let mut off = 0;
    for l in lens.iter().take(n) { out.push(blob[off..off + l].to_vec()); off += l; }
    cts.truncate(messages.len());
    tags.truncate(16 * n);
    Ok((cts, tags, out))
}

/// z (padded instance + witness, one byte per variable) of a GCM key
pub fn aes_witness_gcm(proving_key: &ProvingKey, message: &[u8], secret_key: &[u8; 16], iv: &[u8; 12], aad: &[u8]) -> Result<Vec<u8>> {
    let mut n = 0usize;
    let pk = (proving_key.0).0;
    if unsafe { zkaes_aes_witness_gcm(pk, message.as_ptr(), message.len(), secret_key.as_ptr(), iv.as_ptr(), aad.as_ptr(), aad.len(), std::ptr::null_mut(), 0, &mut n) } != 0 { return Err(last_error()); }
    let mut z = vec![0u8; n];
    if unsafe { zkaes_aes_witness_gcm(pk, message.as_ptr(), message.len(), secret_key.as_ptr(), iv.as_ptr(), aad.as_ptr(), aad.len(), z.as_mut_ptr(), n, &mut n) } != 0 { return Err(last_error()); }
    Ok(z)
}

/// Ok(false) for a wrong iv, aad, ciphertext or tag; Err for malformed input, which includes lengths whose sum is not the key's (they are part of the statement)
pub fn verify_encryption_gcm(verifying_key: &VerifyingKey, proof: &[u8], iv: &[u8; 12], aad: &[u8], ciphertext: &[u8], tag: &[u8; 16]) -> Result<bool> {
    let mut accepted: c_int = 0;
    if unsafe {
        zkaes_verify_encryption_gcm((verifying_key.0).0, proof.as_ptr(), proof.len(), iv.as_ptr(), aad.as_ptr(), aad.len(), ciphertext.as_ptr(), ciphertext.len(), tag.as_ptr(), &mut accepted)
    } != 0 {
        return Err(last_error());
    }
    Ok(accepted != 0)
}


// ---- AES-192 / AES-256 (include/zkaes.h "AES-192 and AES-256").  NOT COMPILED: no cargo in the build image.
// The wrappers above take `secret_key: &[u8; 16]` and stay as they are for AES-128 keys.  The library reads key_bytes(pk) bytes from the pointer, so a caller with a
// 24- or 32-byte key goes through a key from synthesize_keys_ks and passes a slice of exactly proving_key.key_bytes() bytes to the `_ks` wrappers below (ECB shown; the
// other modes follow the same pattern over the same C entry points).
/// key_bits = 128, 192 or 256; aad_len must be 0 outside CIRCUIT_AES_GCM
pub fn synthesize_keys_ks(circuit_kind: c_int, key_bits: u32, len: usize, aad_len: usize, flags: u32) -> Result<(ProvingKey, VerifyingKey)> {
    let (mut pk, mut vk) = (std::ptr::null_mut(), std::ptr::null_mut());
    if unsafe { zkaes_synthesize_keys_ks(circuit_kind, key_bits as c_uint, len, aad_len, 866_944, 513, 4_062_064, flags as c_uint, &mut pk, &mut vk) } != 0 { return Err(last_error()); }
    Ok((ProvingKey(Arc::new(PkHandle(pk))), VerifyingKey(Arc::new(VkHandle(vk)))))
}

impl ProvingKey {
    /// the byte length of the AES key this proving key takes: 16, 24 or 32
    pub fn key_bytes(&self) -> Result<usize> {
        let mut n = 0usize;
        if unsafe { zkaes_pk_key_bytes((self.0).0, &mut n) } != 0 { return Err(last_error()); }
        Ok(n)
    }
}

/// `encrypt` for a key of any size: secret_key.len() must be proving_key.key_bytes()
pub fn encrypt_ks(message: &[u8], secret_key: &[u8], proving_key: &ProvingKey) -> Result<Vec<u8>> {
    if secret_key.len() != proving_key.key_bytes()? { return Err(anyhow!("secret_key must be {} bytes", proving_key.key_bytes()?)); }
    let (mut p, mut n) = (std::ptr::null_mut(), 0usize);
    if unsafe { zkaes_encrypt(message.as_ptr(), message.len(), secret_key.as_ptr(), (proving_key.0).0, &mut p, &mut n) } != 0 { return Err(last_error()); }
    Ok(take_bytes(p, n))
}

/// AES-ECB of whole blocks on the host; the key's length (16, 24, 32) selects AES-128, -192, -256
pub fn ecb_ciphertext(message: &[u8], secret_key: &[u8]) -> Result<Vec<u8>> {
    let mut ct = vec![0u8; message.len().max(1)];
    if unsafe { zkaes_ecb_ciphertext_ks(message.as_ptr(), message.len(), secret_key.as_ptr(), secret_key.len(), ct.as_mut_ptr()) } != 0 { return Err(last_error()); }
    ct.truncate(message.len());
    Ok(ct)
}

/// AES-GCM on the host with a 16-, 24- or 32-byte key: (ciphertext, tag)
pub fn gcm_encrypt_ks(message: &[u8], secret_key: &[u8], iv: &[u8; 12], aad: &[u8]) -> Result<(Vec<u8>, [u8; 16])> {
    let mut ct = vec![0u8; message.len().max(1)];
    let mut tag = [0u8; 16];
    if unsafe { zkaes_gcm_encrypt_ks(message.as_ptr(), message.len(), secret_key.as_ptr(), secret_key.len(), iv.as_ptr(), aad.as_ptr(), aad.len(), ct.as_mut_ptr(), tag.as_mut_ptr()) } != 0 {
        return Err(last_error());
    }
    ct.truncate(message.len());
    Ok((ct, tag))
}

// ---- Key tags: every chunk-proof and record of a job bound to one AES key (include/zkaes.h, section "Key tags").  NOT COMPILED: no cargo in the build image.
/// `synthesize_keys_ks` with key_tag_blocks = 0 (no tag), 1 or 2: every proof of the key also exposes `key_tag(secret_key, key_tag_blocks)` as public input
pub fn synthesize_keys_kt(circuit_kind: c_int, key_bits: u32, key_tag_blocks: u32, len: usize, aad_len: usize, flags: u32) -> Result<(ProvingKey, VerifyingKey)> {
    let (mut pk, mut vk) = (std::ptr::null_mut(), std::ptr::null_mut());
    if unsafe { zkaes_synthesize_keys_kt(circuit_kind, key_bits as c_uint, key_tag_blocks as c_uint, len, aad_len, 866_944, 513, 4_062_064, flags as c_uint, &mut pk, &mut vk) } != 0 {
        return Err(last_error());
    }
    Ok((ProvingKey(Arc::new(PkHandle(pk))), VerifyingKey(Arc::new(VkHandle(vk)))))
}

impl ProvingKey {
    /// the key-tag blocks this proving key was synthesized with: 0, 1 or 2
    pub fn key_tag_blocks(&self) -> Result<usize> {
        let mut n = 0usize;
        if unsafe { zkaes_pk_key_tag_blocks((self.0).0, &mut n) } != 0 { return Err(last_error()); }
        Ok(n)
    }
}

/// the key tag on the host: AES_K(D_0) (|| AES_K(D_1)), D_t = "zkaes-keyta" || t || 00 00 00 00; 16 * blocks bytes, blocks = 1 or 2
pub fn key_tag(secret_key: &[u8], blocks: usize) -> Result<Vec<u8>> {
    let mut out = vec![0u8; 16 * blocks.max(1)];
    if unsafe { zkaes_key_tag(secret_key.as_ptr(), secret_key.len(), blocks, out.as_mut_ptr()) } != 0 { return Err(last_error()); }
    Ok(out)
}

/// the chunk-proofs of one ECB, CBC or CTR job against ONE key tag (16 or 32 bytes); iv_or_icb: None for ECB, the IV for CBC, the initial counter block for CTR
pub fn verify_chunked_tagged(verifying_key: &VerifyingKey, circuit_kind: c_int, proofs: &[Vec<u8>], iv_or_icb: Option<&[u8; 16]>, ciphertext: &[u8], key_tag: &[u8]) -> Result<Vec<bool>> {
    let blob: Vec<u8> = proofs.iter().flat_map(|p| p.iter().copied()).collect();
    let lens: Vec<usize> = proofs.iter().map(|p| p.len()).collect();
    let mut each = vec![0 as c_int; proofs.len().max(1)];
    let mut ok = 0usize;
    let iv = iv_or_icb.map_or(std::ptr::null(), |v| v.as_ptr());
    if unsafe { zkaes_verify_chunked_kt((verifying_key.0).0, circuit_kind, blob.as_ptr(), lens.as_ptr(), proofs.len(), iv, ciphertext.as_ptr(), ciphertext.len(), key_tag.as_ptr(), key_tag.len(),
                                        each.as_mut_ptr(), &mut ok) } != 0 {
        return Err(last_error());
    }
    Ok(each.iter().take(proofs.len()).map(|&a| a != 0).collect())
}

/// `verify_encryption_gcm` for a key with key-tag blocks: the record against its own GCM tag and the key tag every record of the session shares
pub fn verify_encryption_gcm_tagged(verifying_key: &VerifyingKey, proof: &[u8], iv: &[u8; 12], aad: &[u8], ciphertext: &[u8], tag: &[u8; 16], key_tag: &[u8]) -> Result<bool> {
    let mut acc: c_int = 0;
    if unsafe { zkaes_verify_encryption_gcm_kt((verifying_key.0).0, proof.as_ptr(), proof.len(), iv.as_ptr(), aad.as_ptr(), aad.len(), ciphertext.as_ptr(), ciphertext.len(), tag.as_ptr(),
                                               key_tag.as_ptr(), key_tag.len(), &mut acc) } != 0 {
        return Err(last_error());
    }
    Ok(acc != 0)
}
