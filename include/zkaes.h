/* include/zkaes.h -- C ABI of libzkaes, the MI355X-native drop-in for the proving hot path of
 * lambdaclass/AES_zero_knowledge_proof_circuit (crate `zk-aes`).
 *
 * The reference has no FFI / plugin interface; its seam is three Rust functions in src/lib.rs (and the crate
 * forbids `unsafe`, src/lib.rs:2, so the binding lives in a sibling -sys crate: see INTEGRATION.md).  Each entry
 * point below names the reference item it replaces.  Conventions:
 *   - return value 0 = Ok, non-zero = Err; the message of the last error on the calling thread is
 *     zkaes_last_error() (mirrors anyhow::Result, src/lib.rs:45);
 *   - keys are opaque handles that own device-resident data (SRS powers, index polynomials, circuit tables,
 *     workspace); a handle is bound to the GPU that was current when it was created;
 *   - proofs cross the boundary as bytes in the ark-serialize 0.3 compressed layout of ark_marlin::Proof
 *     (what simpleworks' (de)serialize_proof reads/writes, re-exported at src/lib.rs:52);
 *   - byte buffers returned through `uint8_t**` are owned by the library: release with zkaes_bytes_free.
 *   - keys for a plaintext of 16 bytes or more use fixed-base window tables of the universal SRS (13 copies of 192-byte records of powers_of_g[0 ..= max_degree]: 31.4 GB for the
 *     reference's literals, held ONCE per process and device and shared by every key -- zkaes_pk_srs_info; skipped when the device is short of memory or with ZKAES_KEY_NO_TABLES): multi-proof calls (zkaes_encrypt_chunked / _batch) run their
 *     large MSMs (>= 100 k points) through them (13 balanced windows of 19-20 bits over ONE bucket set instead of 15 windows with their own buckets), and so does a
 *     lone zkaes_encrypt call, which additionally runs the independent commitments of each round on four MSM lanes (streams + host threads) side by side.  The
 *     SRS points are stored on BLS12-377's twisted Edwards model (7-product bucket additions): the prover's MSMs assume prime-order-subgroup bases, as KZG's are;
 *   - host threads of a multi-proof call wait for the GPU by polling with short sleeps (a fraction of a core per prover context); a lone zkaes_encrypt call
 *     spins, for latency.  ZKAES_WAIT=spin|sleep forces one policy;
 *   - when the library is loaded it exports GPU_MAX_HW_QUEUES=16 unless the variable is already set (one hardware queue per prover context; the ROCm default of 4
 *     lets the contexts' kernels queue behind each other).  It is read at the first HIP call of the process: export it yourself if HIP is initialised earlier.
 *     ZKAES_KEEP_ENV=1 makes the library leave the environment alone (for hosts whose other threads read it while libraries load);
 *   - the library needs a HIP device (gfx950) for key synthesis and proving and FAILS (non-zero + message) when
 *     none is present -- there is no CPU fallback; zkaes_verify_* runs on the host, as in the reference.
 */
#ifndef ZKAES_H
#define ZKAES_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct zkaes_pk zkaes_pk;   /* simpleworks::marlin::ProvingKey   (src/lib.rs:55) */
typedef struct zkaes_vk zkaes_vk;   /* simpleworks::marlin::VerifyingKey (src/lib.rs:55) */

/* thread-local message of the last failing call ("" if none) */
const char *zkaes_last_error(void);
void zkaes_bytes_free(uint8_t *p);
void zkaes_pk_free(zkaes_pk *pk);
void zkaes_vk_free(zkaes_vk *vk);
/* number of visible HIP devices (0 on a host without a GPU) */
int zkaes_device_count(void);
/* select the HIP device for the CALLING THREAD (hipSetDevice semantics): key handles synthesized afterwards live on it, and the kernel-level
 * entry points below run on it.  A proving key remembers its device: zkaes_encrypt* / zkaes_prove_ops re-select it on whatever thread calls them.
 * Intended deployment: one process per GPU (the NTT twiddle cache is per process). */
int zkaes_set_device(int ordinal);

/* ---- the reference's public API ------------------------------------------------------------------------------- */
/* replaces `pub fn synthesize_keys(plaintext_length: usize) -> Result<(ProvingKey, VerifyingKey)>` (src/lib.rs:138-174):
 * universal SRS for the literals (866_944, 513, 4_062_064) of src/lib.rs:141 + index of the AES circuit for a message of
 * `plaintext_length` bytes (multiple of 16). */
int zkaes_synthesize_keys(size_t plaintext_length, zkaes_pk **pk, zkaes_vk **vk);
/* replaces `pub fn encrypt(message: &[u8], secret_key: &[u8; 16], proving_key: ProvingKey) -> Result<MarlinProof>`
 * (src/lib.rs:60-114).  The proving key is borrowed, not consumed (callers of the reference clone it per call,
 * benches/benchmark_encrypt.rs:46).  Prover randomness = generate_rand() (fixed ark_std::test_rng seed), as src/lib.rs:65. */
int zkaes_encrypt(const uint8_t *message, size_t message_len, const uint8_t secret_key[16], const zkaes_pk *pk, uint8_t **proof, size_t *proof_len);
/* replaces `pub fn verify_encryption(verifying_key: VerifyingKey, proof: &MarlinProof, ciphertext: &[u8]) -> Result<bool>`
 * (src/lib.rs:116-136): ciphertext bytes -> 8 LSB-first field elements each (src/helpers/mod.rs:84-93) -> Marlin verify.
 * A wrong ciphertext is Ok(false): returns 0 with *accepted = 0 (tests/integration_tests.rs:336). */
int zkaes_verify_encryption(const zkaes_vk *vk, const uint8_t *proof, size_t proof_len, const uint8_t *ciphertext, size_t ciphertext_len, int *accepted);
/* replaces the re-export `deserialize_proof` (src/lib.rs:52) as a validity check + canonical re-serialization */
int zkaes_proof_roundtrip(const uint8_t *proof, size_t proof_len, uint8_t **out, size_t *out_len);

/* ---- extensions ------------------------------------------------------------------------------------------------ */
#define ZKAES_CIRCUIT_AES 0      /* src/lib.rs:176-293 */
#define ZKAES_CIRCUIT_OPS_XOR 1  /* src/ops.rs:8-18 (as a BLS12-377 Marlin circuit) */
#define ZKAES_CIRCUIT_OPS_ADD 2  /* src/ops.rs:20-29 */
#define ZKAES_CIRCUIT_AES_CTR 4  /* AES-128-CTR for any byte length >= 1 (no upstream counterpart; section "AES-128-CTR" below); accepted by the same calls as ZKAES_CIRCUIT_AES_CBC */
#define ZKAES_CIRCUIT_AES_GCM 5  /* AES-128-GCM, 96-bit IV, full tag (no upstream code; section "AES-128-GCM" below); zkaes_synthesize_keys_gcm, or _ex / _ex2 for an empty aad */
#define ZKAES_CIRCUIT_AES_CBC 3  /* AES-128-CBC (no upstream counterpart; section "AES-128-CBC" below); accepted by zkaes_synthesize_keys_ex / _ex2, zkaes_circuit_info, zkaes_circuit_matrix */
/* as zkaes_synthesize_keys with an explicit circuit kind and universal-SRS literals (generate_universal_srs arguments) */
int zkaes_synthesize_keys_ex(int circuit_kind, size_t plaintext_length, size_t srs_num_constraints, size_t srs_num_variables, size_t srs_num_non_zero, zkaes_pk **pk,
                             zkaes_vk **vk);
/* the same with option flags.  ZKAES_KEY_NO_TABLES: this key does not use (and, if it is the first key over its SRS, does not build) the fixed-base window tables of the
 * universal SRS (31.4 GB of device memory for the reference's literals, shared by all keys); its multi-proof calls then use 15 per-window-bucket windows instead of
 * 13 table windows, ~9 % fewer proofs per second.  Unknown flag bits are an error. */
#define ZKAES_KEY_NO_TABLES 1u
int zkaes_synthesize_keys_ex2(int circuit_kind, size_t plaintext_length, size_t srs_num_constraints, size_t srs_num_variables, size_t srs_num_non_zero, unsigned flags,
                              zkaes_pk **pk, zkaes_vk **vk);
/* as zkaes_encrypt with an explicit 32-byte StdRng seed for the prover's zero-knowledge randomness (NULL = test_rng seed) */
int zkaes_encrypt_seeded(const uint8_t *message, size_t message_len, const uint8_t secret_key[16], const zkaes_pk *pk, const uint8_t *zk_seed32, uint8_t **proof,
                         size_t *proof_len);
/* chunked proving of a long ECB message: ceil(message_len / chunk_len) independent proofs with one key for chunk_len bytes
 * (the last chunk must be full).  proofs = concatenation, proof_lens[i] = length of proof i (caller array of n_chunks).
 * Zero-knowledge randomness: a FRESH 32-byte seed from the operating system per call (getrandom), proof i drawing from
 * StdRng(Blake2s(seed || i as u64 LE)) -- unlike the reference's encrypt(), whose every call draws from the fixed ark_std::test_rng() seed
 * (src/lib.rs:65), these extensions put hundreds of proofs under one AES key and must not share blinding factors.  The fixed stream for every proof (byte parity with the CPU
 * oracle in tests; not zero-knowledge across proofs) is reachable only explicitly: the *_seeded entry points with a NULL seed. */
int zkaes_encrypt_chunked(const uint8_t *message, size_t message_len, const uint8_t secret_key[16], const zkaes_pk *pk, uint8_t **proofs, size_t *proofs_len,
                          size_t *proof_lens, size_t n_chunks);
/* n independent (message_i, secret_key_i) pairs on one key / one SRS (BASELINE config 5: many small proofs): messages = n x plaintext
 * length bytes, secret_keys = n x 16 bytes.  Up to zkaes_pk_get_contexts(pk) proofs (zkaes_pk_set_contexts; default ZKAES_DEFAULT_CONTEXTS, the configuration bench.py
 * measures) are in flight per call, each on its own HIP stream.  Randomness as zkaes_encrypt_chunked.  This entry point cannot
 * check its buffer lengths: prefer zkaes_encrypt_batch_seeded. */
#define ZKAES_DEFAULT_CONTEXTS 12
int zkaes_encrypt_batch(size_t n, const uint8_t *messages, const uint8_t *secret_keys, const zkaes_pk *pk, uint8_t **proofs, size_t *proofs_len, size_t *proof_lens);
/* Proofs in flight per multi-proof call (zkaes_encrypt_chunked* / _batch*) on THIS key: n = 1..64 prover contexts (own stream + ~0.9 / 4.7 GB of workspace each for the
 * 1- / 6-block key, created on first use), n = 0 restores the process default -- ZKAES_DEFAULT_CONTEXTS, or the ZKAES_CONTEXTS environment variable as it stood when the
 * library first needed it (read once; later changes of the environment are ignored).  Takes effect from the next call; calls already running keep their count. */
int zkaes_pk_set_contexts(zkaes_pk *pk, size_t n);
int zkaes_pk_get_contexts(const zkaes_pk *pk, size_t *n);
/* the chunked / batch calls with explicit buffer lengths (checked: messages_len == n x plaintext length, secret_keys_len == n x 16) and a
 * caller-supplied 32-byte seed.  Proof i draws from StdRng(Blake2s(zk_seed32 || (first_proof_index + i) as u64 LE)): a caller that splits ONE job over
 * several calls or ranks under one seed passes the job-global index of the call's first proof (the *_at variants; the plain ones use 0), so that no
 * two proofs of the job share blinding factors or the mask polynomial.  zk_seed32 == NULL selects the reference's fixed test_rng() stream for every
 * proof (explicit byte-parity mode: differences of hiding commitments across proofs are then unblinded -- tests only). */
int zkaes_encrypt_chunked_seeded(const uint8_t *message, size_t message_len, const uint8_t secret_key[16], const zkaes_pk *pk, const uint8_t *zk_seed32, uint8_t **proofs,
                                 size_t *proofs_len, size_t *proof_lens, size_t n_chunks);
int zkaes_encrypt_chunked_seeded_at(const uint8_t *message, size_t message_len, const uint8_t secret_key[16], const zkaes_pk *pk, const uint8_t *zk_seed32,
                                    uint64_t first_proof_index, uint8_t **proofs, size_t *proofs_len, size_t *proof_lens, size_t n_chunks);
int zkaes_encrypt_batch_seeded(size_t n, const uint8_t *messages, size_t messages_len, const uint8_t *secret_keys, size_t secret_keys_len, const zkaes_pk *pk,
                               const uint8_t *zk_seed32, uint8_t **proofs, size_t *proofs_len, size_t *proof_lens);
int zkaes_encrypt_batch_seeded_at(size_t n, const uint8_t *messages, size_t messages_len, const uint8_t *secret_keys, size_t secret_keys_len, const zkaes_pk *pk,
                                  const uint8_t *zk_seed32, uint64_t first_proof_index, uint8_t **proofs, size_t *proofs_len, size_t *proof_lens);
/* ---- AES-128-CBC ---------------------------------------------------------------------------------------------------
 * Statement of a key synthesized with ZKAES_CIRCUIT_AES_CBC for 16 nb bytes (nb >= 1): public = iv (16 bytes) and ciphertext (16 nb bytes), private = message and
 * secret_key, with C_-1 = iv and C_b = AES-128(key, M_b ^ C_b-1).  Public-input vector (the instance without the leading One): the 128 IV bits, then the 128 nb
 * ciphertext bits, every byte as 8 LSB-first bits.  A message of 0 bytes or one that is not whole blocks is an error; there is no padding scheme.
 * A long message splits into independent chunk-proofs exactly as ECB does: the chaining value entering chunk j is the last ciphertext block of chunk j - 1, which is
 * public, so each chunk-proof takes its own IV as public input and the verifier derives every chunk's IV from (iv, ciphertext) alone.  Nothing binds the chunk-proofs
 * of one message to the same key (as in ECB).  The ECB entry points refuse a CBC key and the CBC ones refuse every other key. */
/* host only, no GPU: ciphertext (message_len bytes) = AES-128-CBC(secret_key, iv, message) */
int zkaes_cbc_ciphertext(const uint8_t *message, size_t message_len, const uint8_t secret_key[16], const uint8_t iv[16], uint8_t *ciphertext);
/* one proof over a CBC key for message_len bytes; zk_seed32 as zkaes_encrypt_seeded (NULL = test_rng seed).  ciphertext_or_null receives message_len bytes */
int zkaes_encrypt_cbc_seeded(const uint8_t *message, size_t message_len, const uint8_t secret_key[16], const uint8_t iv[16], const zkaes_pk *pk, const uint8_t *zk_seed32,
                             uint8_t *ciphertext_or_null, uint8_t **proof, size_t *proof_len);
/* chunk-proofs of a long CBC message, laid out as zkaes_encrypt_chunked's.  iv = the chaining value entering THIS call's first chunk: a job split over several calls or
 * ranks takes each call's iv from zkaes_cbc_ciphertext (the 16 ciphertext bytes ahead of the call's first chunk).  The library runs the whole chain on the host first and
 * then proves the chunks side by side; the device recomputes every chunk's chain from the chunk's IV alone.  Seeds and first_proof_index as in the ECB chunked calls:
 * the unseeded call draws a fresh OS seed, NULL in the seeded one is the fixed test_rng stream (tests only). */
int zkaes_encrypt_cbc_chunked(const uint8_t *message, size_t message_len, const uint8_t secret_key[16], const uint8_t iv[16], const zkaes_pk *pk, uint8_t *ciphertext_or_null,
                              uint8_t **proofs, size_t *proofs_len, size_t *proof_lens, size_t n_chunks);
int zkaes_encrypt_cbc_chunked_seeded_at(const uint8_t *message, size_t message_len, const uint8_t secret_key[16], const uint8_t iv[16], const zkaes_pk *pk, const uint8_t *zk_seed32,
                                        uint64_t first_proof_index, uint8_t *ciphertext_or_null, uint8_t **proofs, size_t *proofs_len, size_t *proof_lens, size_t n_chunks);
/* as zkaes_aes_witness for a CBC key */
int zkaes_aes_witness_cbc(const zkaes_pk *pk, const uint8_t *message, size_t message_len, const uint8_t secret_key[16], const uint8_t iv[16], uint8_t *z, size_t z_cap, size_t *z_len);
/* host only: as zkaes_verify_encryption over the public input (iv, ciphertext) */
int zkaes_verify_encryption_cbc(const zkaes_vk *vk, const uint8_t *proof, size_t proof_len, const uint8_t iv[16], const uint8_t *ciphertext, size_t ciphertext_len, int *accepted);
/* host only, serial: n_chunks proofs (concatenated, proof_lens[j] bytes each) against ciphertext_len = n_chunks x chunk bytes; chunk j is checked under iv (j = 0) or the
 * 16 ciphertext bytes ahead of its slice.  accepted_each (n_chunks ints) and n_accepted may be NULL; a chunk whose proof bytes do not parse counts as rejected */
int zkaes_verify_cbc_chunked(const zkaes_vk *vk, const uint8_t *proofs, const size_t *proof_lens, size_t n_chunks, const uint8_t iv[16], const uint8_t *ciphertext,
                             size_t ciphertext_len, int *accepted_each, size_t *n_accepted);
/* ---- AES-128-CTR ---------------------------------------------------------------------------------------------------
 * Statement of a key synthesized with ZKAES_CIRCUIT_AES_CTR for L bytes (any L >= 1, nb = ceil(L / 16) blocks): public = icb (the 16-byte initial counter block) and
 * ciphertext (L bytes), private = message (L bytes) and secret_key, with CTR_0 = icb, CTR_b = CTR_b-1 + 1 mod 2^128 and C_b = M_b ^ AES-128(key, CTR_b), the last block
 * cut to the bytes that exist.  The counter is ONE big-endian 128-bit integer over the 16 bytes (SP 800-38A appendix B.1 with m = 128: what OpenSSL, Go and Python's
 * cryptography do); it is not GCM's inc32, which wraps the low 32 bits only.  Public-input vector (the instance without the leading One): the 128 icb bits, then the 8 L
 * ciphertext bits, every byte as 8 LSB-first bits.  Encryption and decryption are the same function.
 * Blocks are independent, so a long message splits into chunk-proofs that are seekable: chunk j of a key for nb whole blocks is proven and verified under icb + j nb,
 * from (icb, j) alone, on any rank, with nothing serial ahead of it.  A ragged tail is one more proof under a second key of the tail's length and the advanced counter.
 * Nothing binds the chunk-proofs of one message to the same key (as in ECB and CBC).  The CTR entry points refuse every other key, and every other entry point refuses
 * a CTR key.  A verifying key carries no mode: a CBC key for 16 nb bytes takes a public input of the same shape (16 bytes, then the ciphertext), and it is the key
 * that names the relation a proof is checked against, so a verifier keeps the keys of different modes apart. */
/* host only, no GPU: out (len bytes, len >= 1) = in ^ keystream(secret_key, icb); encrypts and decrypts */
int zkaes_ctr_crypt(const uint8_t *in, size_t len, const uint8_t secret_key[16], const uint8_t icb[16], uint8_t *out);
/* host only: out16 = icb + n_blocks mod 2^128 (big-endian); the counter of the block n_blocks behind icb's.  out16 may be icb */
int zkaes_ctr_counter_add(const uint8_t icb[16], uint64_t n_blocks, uint8_t out16[16]);
/* one proof over a CTR key for exactly message_len bytes; zk_seed32 as zkaes_encrypt_seeded (NULL = test_rng seed).  ciphertext_or_null receives message_len bytes */
int zkaes_encrypt_ctr_seeded(const uint8_t *message, size_t message_len, const uint8_t secret_key[16], const uint8_t icb[16], const zkaes_pk *pk, const uint8_t *zk_seed32,
                             uint8_t *ciphertext_or_null, uint8_t **proof, size_t *proof_len);
/* chunk-proofs of a long CTR message, laid out as zkaes_encrypt_chunked's: the key's L must be a multiple of 16 and message_len exactly n_chunks x L, anything else is an
 * error.  icb = the counter of THIS call's first block: a job split over several calls or ranks passes zkaes_ctr_counter_add(icb, blocks before) and the job-global
 * first_proof_index.  Seeds as in the ECB chunked calls: the unseeded call draws a fresh OS seed, NULL in the seeded one is the fixed test_rng stream (tests only). */
int zkaes_encrypt_ctr_chunked(const uint8_t *message, size_t message_len, const uint8_t secret_key[16], const uint8_t icb[16], const zkaes_pk *pk, uint8_t *ciphertext_or_null,
                              uint8_t **proofs, size_t *proofs_len, size_t *proof_lens, size_t n_chunks);
int zkaes_encrypt_ctr_chunked_seeded_at(const uint8_t *message, size_t message_len, const uint8_t secret_key[16], const uint8_t icb[16], const zkaes_pk *pk, const uint8_t *zk_seed32,
                                        uint64_t first_proof_index, uint8_t *ciphertext_or_null, uint8_t **proofs, size_t *proofs_len, size_t *proof_lens, size_t n_chunks);
/* as zkaes_aes_witness for a CTR key */
int zkaes_aes_witness_ctr(const zkaes_pk *pk, const uint8_t *message, size_t message_len, const uint8_t secret_key[16], const uint8_t icb[16], uint8_t *z, size_t z_cap, size_t *z_len);
/* host only: as zkaes_verify_encryption over the public input (icb, ciphertext).  The byte length is part of the statement (the verifier zero-pads the public input, so a
 * ciphertext with zero bytes appended would pad to the same vector): a ciphertext_len other than the key's is an error.  A key restored by zkaes_vk_deserialize_ark
 * carries only the padded input count; with such a key the caller answers for the exact length */
int zkaes_verify_encryption_ctr(const zkaes_vk *vk, const uint8_t *proof, size_t proof_len, const uint8_t icb[16], const uint8_t *ciphertext, size_t ciphertext_len, int *accepted);
/* host only, serial: n_chunks proofs (concatenated, proof_lens[j] bytes each) against ciphertext_len = n_chunks x chunk bytes, chunk a multiple of 16 and the key's length;
 * chunk j is checked under icb + j * chunk / 16.  accepted_each (n_chunks ints) and n_accepted may be NULL; a chunk whose proof bytes do not parse counts as rejected */
int zkaes_verify_ctr_chunked(const zkaes_vk *vk, const uint8_t *proofs, const size_t *proof_lens, size_t n_chunks, const uint8_t icb[16], const uint8_t *ciphertext,
                             size_t ciphertext_len, int *accepted_each, size_t *n_accepted);
/* ---- AES-128-GCM ---------------------------------------------------------------------------------------------------
 * Statement of a key synthesized with ZKAES_CIRCUIT_AES_GCM for a message of L bytes (any L >= 1) and an AAD of A bytes (any A >= 0), both fixed by the key: public = iv
 * (12 bytes; other IV lengths are refused), aad (A bytes), ciphertext (L bytes) and tag (16 bytes; full tags only), private = message (L bytes) and secret_key, related as
 * in SP 800-38D: H = AES_K(0^128), J_0 = iv || 00000001, block b of the message is encrypted under iv || be32(b + 2), the last block cut to the bytes that exist,
 * S = GHASH_H(aad zero-padded to blocks || ciphertext zero-padded to blocks || be64(8 A) || be64(8 L)), tag = S ^ AES_K(J_0).
 * Public-input vector (the instance without the leading One): 96 iv bits, 8 A aad bits, 8 L ciphertext bits, 128 tag bits, every byte as 8 LSB-first bits; 224 + 8 A + 8 L
 * in all.  The vector does not say where the aad ends and the ciphertext begins: the length block is a constant inside the circuit, so it is the key that pins the
 * split, as it names the mode (a verifying key carries neither).  The verifier refuses a call whose A + L is not the key's.
 * One proof per (iv, aad, ciphertext, tag).  There are no chunk-proofs of one long GCM message: the chaining value of GHASH is secret, and publishing it would give H
 * away.  A long job is a batch of records (zkaes_encrypt_gcm_batch_seeded_at), which is where the prover contexts run side by side.  Nothing binds the proofs of a batch
 * to one key.  The GCM entry points refuse every other key, and every other entry point refuses a GCM key. */
/* as zkaes_synthesize_keys_ex2 for a GCM key of (plaintext_length, aad_length); _ex / _ex2 with ZKAES_CIRCUIT_AES_GCM give aad_length = 0 */
int zkaes_synthesize_keys_gcm(size_t plaintext_length, size_t aad_length, size_t srs_num_constraints, size_t srs_num_variables, size_t srs_num_non_zero, unsigned flags,
                              zkaes_pk **pk, zkaes_vk **vk);
/* host only, no GPU: ciphertext (message_len bytes) and tag16 of AES-128-GCM; message_len >= 0, aad_len >= 0 (a NULL pointer is fine where the length is 0) */
int zkaes_gcm_encrypt(const uint8_t *message, size_t message_len, const uint8_t secret_key[16], const uint8_t iv12[12], const uint8_t *aad, size_t aad_len,
                      uint8_t *ciphertext, uint8_t tag16[16]);
/* host only: *ok = 1 and message (ciphertext_len bytes) written if the tag holds, else *ok = 0 and message untouched.  The tags are compared in constant time */
int zkaes_gcm_decrypt(const uint8_t *ciphertext, size_t ciphertext_len, const uint8_t secret_key[16], const uint8_t iv12[12], const uint8_t *aad, size_t aad_len,
                      const uint8_t tag16[16], uint8_t *message, int *ok);
/* one proof over a GCM key for exactly (message_len, aad_len); zk_seed32 as zkaes_encrypt_seeded (NULL = test_rng seed).  ciphertext_or_null receives message_len bytes,
 * tag_or_null 16 */
int zkaes_encrypt_gcm_seeded(const uint8_t *message, size_t message_len, const uint8_t secret_key[16], const uint8_t iv12[12], const uint8_t *aad, size_t aad_len,
                             const zkaes_pk *pk, const uint8_t *zk_seed32, uint8_t *ciphertext_or_null, uint8_t *tag_or_null, uint8_t **proof, size_t *proof_len);
/* n independent records over one GCM key for (L, A): messages = n x L bytes, secret_keys = n x 16, headers = n x (12 + A) bytes (each record's iv, then its aad); the
 * three lengths are checked.  proofs laid out as zkaes_encrypt_batch's; seeds and first_proof_index as zkaes_encrypt_batch_seeded_at.  ciphertexts_or_null = n x L bytes,
 * tags_or_null = n x 16 */
int zkaes_encrypt_gcm_batch_seeded_at(size_t n, const uint8_t *messages, size_t messages_len, const uint8_t *secret_keys, size_t secret_keys_len, const uint8_t *headers,
                                      size_t headers_len, const zkaes_pk *pk, const uint8_t *zk_seed32, uint64_t first_proof_index, uint8_t *ciphertexts_or_null,
                                      uint8_t *tags_or_null, uint8_t **proofs, size_t *proofs_len, size_t *proof_lens);
/* as zkaes_aes_witness for a GCM key */
int zkaes_aes_witness_gcm(const zkaes_pk *pk, const uint8_t *message, size_t message_len, const uint8_t secret_key[16], const uint8_t iv12[12], const uint8_t *aad, size_t aad_len,
                          uint8_t *z, size_t z_cap, size_t *z_len);
/* host only: as zkaes_verify_encryption over the public input (iv, aad, ciphertext, tag).  aad_len + ciphertext_len must be the key's (the verifier zero-pads the input);
 * a key restored by zkaes_vk_deserialize_ark carries only the padded input count, and with such a key the caller answers for the exact lengths */
int zkaes_verify_encryption_gcm(const zkaes_vk *vk, const uint8_t *proof, size_t proof_len, const uint8_t iv12[12], const uint8_t *aad, size_t aad_len,
                                const uint8_t *ciphertext, size_t ciphertext_len, const uint8_t tag16[16], int *accepted);
/* host only: zkaes_circuit_info / zkaes_circuit_matrix of the GCM circuit for (plaintext_length, aad_length) */
int zkaes_circuit_info_gcm(size_t plaintext_length, size_t aad_length, uint64_t out[12]);
int zkaes_circuit_matrix_gcm(size_t plaintext_length, size_t aad_length, int which, uint64_t *n_rows, uint64_t *nnz, uint32_t *rowptr, uint32_t *col, int64_t *coeff);
/* ---- AES-192 and AES-256 ---------------------------------------------------------------------------------------------
 * Every mode above exists for the three key sizes of FIPS-197: key_bits = 128 (what every synthesizer above makes), 192 or 256.  The statement of a mode, its public-input
 * vector and its verifier do not change: the key size only changes the private key's length (key_bits / 8 bytes), the round count (10, 12, 14) and the key schedule inside
 * the circuit.
 * A proving key remembers its key size (zkaes_pk_key_bytes: 16, 24 or 32).  No existing function changes signature: `secret_key[16]` is a plain pointer in C, and EVERY
 * proving and witness entry point above reads zkaes_pk_key_bytes(pk) bytes from it -- 16 for every key made by zkaes_synthesize_keys, _ex, _ex2 and _gcm.  The checked
 * batch calls (zkaes_encrypt_batch_seeded*, zkaes_encrypt_gcm_batch_seeded_at) require secret_keys_len == n x zkaes_pk_key_bytes(pk); zkaes_encrypt_batch reads that many.
 * The verify functions are unchanged.  A verifying key carries no key size, just as it carries no mode (see the remark under AES-128-CTR): the public input of an AES-256
 * statement has the shape of the AES-128 one for the same lengths, and it is the key that names the relation a proof is checked against.  A proof made under a key of one
 * size does not verify under the key of another; a verifier keeps the keys of different key sizes apart as it does those of different modes. */
/* as zkaes_synthesize_keys_ex2 / _gcm with the key size: key_bits = 128, 192 or 256, anything else is an error; an ops kind takes 128 only; aad_length != 0 outside
 * ZKAES_CIRCUIT_AES_GCM is an error */
int zkaes_synthesize_keys_ks(int circuit_kind, unsigned key_bits, size_t plaintext_length, size_t aad_length, size_t srs_num_constraints, size_t srs_num_variables,
                             size_t srs_num_non_zero, unsigned flags, zkaes_pk **pk, zkaes_vk **vk);
/* *n = the byte length of the AES key this proving key takes: 16, 24 or 32 (16 for the ops kinds, which take none) */
int zkaes_pk_key_bytes(const zkaes_pk *pk, size_t *n);
/* host only: zkaes_circuit_info / zkaes_circuit_matrix for any kind, key size and (for GCM) aad length; the same refusals as zkaes_synthesize_keys_ks */
int zkaes_circuit_info_ks(int circuit_kind, unsigned key_bits, size_t plaintext_length, size_t aad_length, uint64_t out[12]);
int zkaes_circuit_matrix_ks(int circuit_kind, unsigned key_bits, size_t plaintext_length, size_t aad_length, int which, uint64_t *n_rows, uint64_t *nnz, uint32_t *rowptr,
                            uint32_t *col, int64_t *coeff);
/* host only, no GPU: the ciphers above with the key's byte length, key_len = 16, 24 or 32 (anything else is an error).  zkaes_ecb_ciphertext_ks and _cbc_ take whole
 * blocks (a non-zero multiple of 16 bytes), _ctr_ any length >= 1, the GCM pair any length >= 0, as their AES-128 namesakes */
int zkaes_ecb_ciphertext_ks(const uint8_t *message, size_t message_len, const uint8_t *secret_key, size_t key_len, uint8_t *ciphertext);
int zkaes_cbc_ciphertext_ks(const uint8_t *message, size_t message_len, const uint8_t *secret_key, size_t key_len, const uint8_t iv[16], uint8_t *ciphertext);
int zkaes_ctr_crypt_ks(const uint8_t *in, size_t len, const uint8_t *secret_key, size_t key_len, const uint8_t icb[16], uint8_t *out);
int zkaes_gcm_encrypt_ks(const uint8_t *message, size_t message_len, const uint8_t *secret_key, size_t key_len, const uint8_t iv12[12], const uint8_t *aad, size_t aad_len,
                         uint8_t *ciphertext, uint8_t tag16[16]);
int zkaes_gcm_decrypt_ks(const uint8_t *ciphertext, size_t ciphertext_len, const uint8_t *secret_key, size_t key_len, const uint8_t iv12[12], const uint8_t *aad, size_t aad_len,
                         const uint8_t tag16[16], uint8_t *message, int *ok);
/* ---- Key tags: bind every chunk-proof and record of a job to one AES key ---------------------------------------------------
 * A chunk-proof says "some key encrypts this slice"; nothing above ties the chunk-proofs of one message, or the GCM records of one session, to the SAME key.  A key
 * synthesized with key_tag_blocks = T, T = 1 or 2 (0 = every key above: nothing changes), proves beside its mode's statement
 *     tag_t = AES_K(D_t),   D_t = 7a 6b 61 65 73 2d 6b 65 79 74 61 || t || 00 00 00 00   ("zkaes-keyta", the byte t, four zero bytes),   t = 0 .. T - 1
 * and exposes the 128 T tag bits as public input BEHIND everything the mode puts there (bytes as 8 LSB-first bits, as everywhere).  Two proofs with equal tags were made
 * under the same key (ideal-cipher heuristic: about 2^64 work to break at one block, 2^128 at two); a verifier checks every chunk against ONE tag.  The tag is
 * deterministic -- a public name for the key -- and, like any known plaintext / ciphertext pair, lets anyone test a guessed key.  D_t ends in four zero bytes, so it is no
 * GCM counter block of a 96-bit IV (those end in 1, 2, ...), and begins with non-zero bytes, so it is not the block behind H.  A prover who feeds D_t to ECB, CBC or CTR
 * as a message or counter block publishes their own tag material; like nonce reuse that is the prover's business and is not policed.
 * No new proving entry points: every encrypt, chunked, batch and witness function above takes a tagged proving key as it is.  A verifying key carries no T, as it carries
 * no mode and no key size; its transport layouts do not change.  The untagged verifiers above never accept a proof of a tagged key (they raise where the key carries its
 * exact public-input count and the lengths disagree, and reject otherwise), and the tagged verifiers never accept a proof of an untagged key. */
/* as zkaes_synthesize_keys_ks with key_tag_blocks = 0, 1 or 2 (anything else, or non-zero for an ops kind, is an error) */
int zkaes_synthesize_keys_kt(int circuit_kind, unsigned key_bits, unsigned key_tag_blocks, size_t plaintext_length, size_t aad_length, size_t srs_num_constraints,
                             size_t srs_num_variables, size_t srs_num_non_zero, unsigned flags, zkaes_pk **pk, zkaes_vk **vk);
/* *n = the key-tag blocks of this proving key: 0, 1 or 2 */
int zkaes_pk_key_tag_blocks(const zkaes_pk *pk, size_t *n);
/* host only: out = 16 tag_blocks bytes, AES_K(D_0) (|| AES_K(D_1)): what a verifier is given once per key.  key_len = 16, 24 or 32, tag_blocks = 1 or 2 */
int zkaes_key_tag(const uint8_t *secret_key, size_t key_len, size_t tag_blocks, uint8_t *out);
/* host only: zkaes_circuit_info_ks / zkaes_circuit_matrix_ks with key_tag_blocks; at 0 they return what those return */
int zkaes_circuit_info_kt(int circuit_kind, unsigned key_bits, unsigned key_tag_blocks, size_t plaintext_length, size_t aad_length, uint64_t out[12]);
int zkaes_circuit_matrix_kt(int circuit_kind, unsigned key_bits, unsigned key_tag_blocks, size_t plaintext_length, size_t aad_length, int which, uint64_t *n_rows, uint64_t *nnz,
                            uint32_t *rowptr, uint32_t *col, int64_t *coeff);
/* host only: the chunk-proofs of one ECB, CBC or CTR job (circuit_kind = ZKAES_CIRCUIT_AES, _AES_CBC, _AES_CTR) against ONE key tag.  Chunk j's public input is what
 * zkaes_verify_encryption, zkaes_verify_cbc_chunked and zkaes_verify_ctr_chunked derive for it (iv_or_icb: NULL for ECB, the IV for CBC, the initial counter block for
 * CTR), then the tag bits.  n_chunks = 1 is the lone-proof form, and the only one that takes a CTR ciphertext that is not whole blocks.  key_tag_len = 16 or 32, anything
 * else is an error.  Lengths that do not fit the key's public-input count are an error where the key carries that count (every key but one read from the ark transport);
 * otherwise every chunk is rejected -- a tagged verifier never accepts on a mismatched length.  A proof that does not parse is a rejected chunk, not an error.
 * accepted_each (n_chunks ints) and n_accepted may be NULL */
int zkaes_verify_chunked_kt(const zkaes_vk *vk, int circuit_kind, const uint8_t *proofs, const size_t *proof_lens, size_t n_chunks, const uint8_t *iv_or_icb, const uint8_t *ciphertext,
                            size_t ciphertext_len, const uint8_t *key_tag, size_t key_tag_len, int *accepted_each, size_t *n_accepted);
/* host only: zkaes_verify_encryption_gcm with the key tag behind the GCM tag */
int zkaes_verify_encryption_gcm_kt(const zkaes_vk *vk, const uint8_t *proof, size_t proof_len, const uint8_t iv12[12], const uint8_t *aad, size_t aad_len, const uint8_t *ciphertext,
                                   size_t ciphertext_len, const uint8_t tag16[16], const uint8_t *key_tag, size_t key_tag_len, int *accepted);
/* ---- plaintext digests.
 * Every proof above says "some hidden message encrypts to this ciphertext"; nothing binds the message.  A key synthesized with digest_kind = ZKAES_DIGEST_CHAIN or
 * ZKAES_DIGEST_FINAL (ZKAES_DIGEST_NONE = every key above: nothing changes) proves beside its mode's statement and its key tag
 *     chain:  H_out = C(... C(C(H_in, M[0:64]), M[64:128]) ...)   over the hidden message M, C = SHA-256's compression function (FIPS 180-4 6.2.2), no padding; the
 *             plaintext length must be a non-zero multiple of 64
 *     final:  the same over M || 80 || 00 .. || be64(8 (digest_prefix + L)), ceil((L + 9) / 64) compressions, for any plaintext length L the mode allows; digest_prefix
 *             is a multiple of 64 fixed by the key (the bytes hashed ahead of this proof), digest_prefix + L < 2^61.  With H_in = the initial value and digest_prefix = 0,
 *             H_out = SHA-256(M)
 * and exposes H_in then H_out, 32 bytes each in SHA-256's big-endian word serialisation (a final H_out is the digest's byte string), as the LAST 512 public-input bits,
 * bytes as 8 LSB-first bits as everywhere.  States between the compressions of one proof are witnesses.  A chunked job runs plain SHA-256 over the message on the host
 * and proves chunk j under (states[j], states[j + 1]); a verifier who checks chunk j against those two entries of ONE array has checked the chain, and finishes the digest
 * on the host with zkaes_sha256_finish(states[n], total bytes, NULL, 0, ..).  Every public state is the unpadded hash of a prefix of the message: given states[j], a
 * low-entropy chunk j can be guessed and tested, as the final digest allows for the whole message. */
#define ZKAES_DIGEST_NONE 0
#define ZKAES_DIGEST_CHAIN 1
#define ZKAES_DIGEST_FINAL 2
/* as zkaes_synthesize_keys_kt with digest_kind and digest_prefix (digest_prefix must be 0 unless digest_kind is ZKAES_DIGEST_FINAL; at digest_kind 0 the same key) */
int zkaes_synthesize_keys_pd(int circuit_kind, unsigned key_bits, unsigned key_tag_blocks, unsigned digest_kind, uint64_t digest_prefix, size_t plaintext_length, size_t aad_length,
                             size_t srs_num_constraints, size_t srs_num_variables, size_t srs_num_non_zero, unsigned flags, zkaes_pk **pk, zkaes_vk **vk);
/* host only: zkaes_circuit_info_kt with the digest arguments; at digest_kind 0 it returns what that returns */
int zkaes_circuit_info_pd(int circuit_kind, unsigned key_bits, unsigned key_tag_blocks, unsigned digest_kind, uint64_t digest_prefix, size_t plaintext_length, size_t aad_length,
                          uint64_t out[12]);
/* host only: zkaes_circuit_matrix_kt with the digest arguments */
int zkaes_circuit_matrix_pd(int circuit_kind, unsigned key_bits, unsigned key_tag_blocks, unsigned digest_kind, uint64_t digest_prefix, size_t plaintext_length, size_t aad_length,
                            int which, uint64_t *n_rows, uint64_t *nnz, uint32_t *rowptr, uint32_t *col, int64_t *coeff);
/* out = {digest kind, digest prefix, compressions per proof, offset of the digest region in a trace}; all zero for a key without a digest */
int zkaes_pk_digest_info(const zkaes_pk *pk, uint64_t out[4]);
/* *circuit_kind = the ZKAES_CIRCUIT_* this proving key was synthesized for, *header_bytes = the public header a proof of that mode carries ahead of a digest key's H_in:
 * 0 (ECB, the ops kinds), 16 (CBC, CTR), 12 + the key's aad length (GCM).  Either pointer may be NULL */
int zkaes_pk_mode(const zkaes_pk *pk, int *circuit_kind, size_t *header_bytes);
/* host only: h_out (32 bytes) = the compressions of data's len / 64 blocks from h_in (32 bytes, NULL = SHA-256's initial value); len must be a multiple of 64 */
int zkaes_sha256_chain(const uint8_t *h_in, const uint8_t *data, size_t len, uint8_t h_out[32]);
/* host only: digest (32 bytes) = the chain from h_in (NULL = the initial value) over tail || 80 || 00 .. || be64(8 (prefix_bytes + tail_len)); prefix_bytes a multiple of 64.
 * zkaes_sha256_finish(NULL, 0, m, len, d) is SHA-256(m) */
int zkaes_sha256_finish(const uint8_t *h_in, uint64_t prefix_bytes, const uint8_t *tail, size_t tail_len, uint8_t digest[32]);
/* witness generation only, for a digest key of any mode: hdr = the mode's public header (NULL for ECB, the 16 bytes of the iv or initial counter block for CBC and CTR,
 * iv (12) then the key's aad for GCM), h_in = 32 bytes or NULL for the initial value.  z as zkaes_aes_witness */
int zkaes_aes_witness_pd(const zkaes_pk *pk, const uint8_t *msg, size_t len, const uint8_t *secret_key, const uint8_t *hdr, const uint8_t *h_in, uint8_t *z, size_t z_cap, size_t *z_len);
/* n independent proofs over a digest key of any mode: messages = n x the key's plaintext length, secret_keys = n x its key bytes, headers = n x the mode's header bytes
 * (0 for ECB: pass NULL and headers_len 0; 16 for CBC and CTR; 12 + the key's aad length for GCM), h_ins = n x 32 bytes or NULL (every proof starts from the initial
 * value).  Receives, where the pointer is not NULL, the ciphertexts (n x plaintext length), the GCM tags (n x 16, GCM keys only) and every proof's H_out (n x 32).  Seed
 * and index as zkaes_encrypt_batch_seeded_at */
int zkaes_encrypt_digest_batch_seeded_at(size_t n, const uint8_t *messages, size_t messages_len, const uint8_t *secret_keys, size_t secret_keys_len, const uint8_t *headers, size_t headers_len,
                                         const uint8_t *h_ins, const zkaes_pk *pk, const uint8_t *zk_seed32, uint64_t first_proof_index, uint8_t *ciphertexts_or_null, uint8_t *tags_or_null,
                                         uint8_t *h_outs_or_null, uint8_t **proofs, size_t *proofs_len, size_t *proof_lens);
/* the chunk-proofs of one ECB, CBC or CTR message over a CHAIN key: hdr = the header entering this call's first chunk (NULL for ECB), h_in = the state entering it (NULL =
 * the initial value); every chunk's header and state are computed on the host.  states_or_null receives the n_chunks + 1 states, 32 bytes each (states[0] = h_in); a job
 * split over calls passes the previous call's last state, the CBC chaining value or zkaes_ctr_counter_add(icb, blocks before).  Seed and index as
 * zkaes_encrypt_chunked_seeded_at */
int zkaes_encrypt_digest_chunked_seeded_at(const uint8_t *msg, size_t len, const uint8_t *secret_key, const uint8_t *hdr, const uint8_t *h_in, const zkaes_pk *pk, const uint8_t *zk_seed32,
                                           uint64_t first_proof_index, uint8_t *ciphertext_or_null, uint8_t *states_or_null, uint8_t **proofs, size_t *proofs_len, size_t *proof_lens,
                                           size_t n_chunks);
/* host only: the chunk-proofs of one ECB, CBC or CTR job over a digest key.  Chunk j's public input is what zkaes_verify_chunked_kt derives for it (without tag bits when
 * key_tag is NULL and key_tag_len 0), then states[j] and states[j + 1]; states = (n_chunks + 1) x 32 bytes.  n_chunks = 1 is the lone-proof form: (states[0], states[1]) =
 * (H_in, H_out), and a CTR ciphertext may then have any length.  Lengths that do not fit the key's public-input count are an error where the key carries that count,
 * otherwise every chunk is rejected.  A proof that does not parse is a rejected chunk, not an error.  accepted_each (n_chunks ints) and n_accepted may be NULL */
int zkaes_verify_digest_chunked(const zkaes_vk *vk, int circuit_kind, const uint8_t *proofs, const size_t *proof_lens, size_t n_chunks, const uint8_t *iv_or_icb, const uint8_t *ciphertext,
                                size_t ciphertext_len, const uint8_t *key_tag, size_t key_tag_len, const uint8_t *states, int *accepted_each, size_t *n_accepted);
/* host only: zkaes_verify_encryption_gcm_kt (key_tag NULL and key_tag_len 0 for a key without tag blocks) with h_in (NULL = the initial value) and h_out behind it */
int zkaes_verify_encryption_gcm_digest(const zkaes_vk *vk, const uint8_t *proof, size_t proof_len, const uint8_t iv12[12], const uint8_t *aad, size_t aad_len, const uint8_t *ciphertext,
                                       size_t ciphertext_len, const uint8_t tag16[16], const uint8_t *key_tag, size_t key_tag_len, const uint8_t *h_in, const uint8_t h_out[32], int *accepted);
/* ---- selective disclosure.
 * Every statement above keeps the whole message hidden.  A key synthesized with reveal = 1 (reveal = 0 = every key above: nothing changes) proves, beside its mode's
 * statement, its key tag and its digest, for a message M of L bytes
 *     revealed[i] = mask_i ? M[i] : 0,   i < L
 * and exposes, as the LAST 8 ceil(L / 8) + 8 L public-input bits, the mask (ceil(L / 8) bytes; mask_i = bit i % 8 of byte i / 8; the bits at or beyond L must be zero) and
 * then revealed (L bytes), bytes as 8 LSB-first bits as everywhere.  The mask is public INPUT chosen per proof -- one key serves every mask -- and revealed is public
 * OUTPUT.  A chunked job takes ONE mask over the whole job; chunk boundaries are multiples of 16 bytes, so chunk j is proven under mask bytes [chunk j / 8, chunk (j + 1) / 8).
 * What it leaks: in CTR and GCM a revealed byte gives away that keystream byte, as any known plaintext does; the mask itself is public; a hidden byte and a revealed zero
 * byte are told apart by the mask, not by revealed.  Every mode, key size, key-tag count and digest kind has a reveal form; GCM segment keys and the ops kinds have none.
 * Every proving and witness entry above refuses a reveal key and names the entries below; the entries below refuse a key without reveal. */
/* as zkaes_synthesize_keys_pd with reveal = 0 or 1 (at 0 the same key) */
int zkaes_synthesize_keys_rv(int circuit_kind, unsigned key_bits, unsigned key_tag_blocks, unsigned digest_kind, uint64_t digest_prefix, unsigned reveal, size_t plaintext_length,
                             size_t aad_length, size_t srs_num_constraints, size_t srs_num_variables, size_t srs_num_non_zero, unsigned flags, zkaes_pk **pk, zkaes_vk **vk);
/* host only: zkaes_circuit_info_pd / zkaes_circuit_matrix_pd with the reveal flag; at reveal 0 they return what those return */
int zkaes_circuit_info_rv(int circuit_kind, unsigned key_bits, unsigned key_tag_blocks, unsigned digest_kind, uint64_t digest_prefix, unsigned reveal, size_t plaintext_length,
                          size_t aad_length, uint64_t out[12]);
int zkaes_circuit_matrix_rv(int circuit_kind, unsigned key_bits, unsigned key_tag_blocks, unsigned digest_kind, uint64_t digest_prefix, unsigned reveal, size_t plaintext_length,
                            size_t aad_length, int which, uint64_t *n_rows, uint64_t *nnz, uint32_t *rowptr, uint32_t *col, int64_t *coeff);
/* out = {reveal flag, message bytes L, mask bytes ceil(L / 8), offset of the reveal region in a trace}; all zero for a key without reveal */
int zkaes_pk_reveal_info(const zkaes_pk *pk, uint64_t out[4]);
/* host only: out (len bytes) = revealed for (msg, mask); mask_len must be ceil(len / 8) and no mask bit at or beyond len may be set */
int zkaes_reveal_bytes(const uint8_t *msg, size_t len, const uint8_t *mask, size_t mask_len, uint8_t *out);
/* witness generation only, for a reveal key of any mode: hdr and h_in as zkaes_aes_witness_pd (h_in is read by a key with a digest only), mask = ceil(len / 8) bytes */
int zkaes_aes_witness_rv(const zkaes_pk *pk, const uint8_t *msg, size_t len, const uint8_t *secret_key, const uint8_t *hdr, const uint8_t *h_in, const uint8_t *mask, size_t mask_len,
                         uint8_t *z, size_t z_cap, size_t *z_len);
/* n independent proofs over a reveal key of any mode: messages, secret_keys, headers, h_ins as zkaes_encrypt_digest_batch_seeded_at (h_ins is read by a key with a digest
 * only), masks = n x ceil(L / 8) bytes.  Receives, where the pointer is not NULL, the ciphertexts, the GCM tags (GCM keys only), every proof's H_out (keys with a digest
 * only) and every proof's revealed bytes (n x L) */
int zkaes_encrypt_reveal_batch_seeded_at(size_t n, const uint8_t *messages, size_t messages_len, const uint8_t *secret_keys, size_t secret_keys_len, const uint8_t *headers, size_t headers_len,
                                         const uint8_t *h_ins, const uint8_t *masks, size_t masks_len, const zkaes_pk *pk, const uint8_t *zk_seed32, uint64_t first_proof_index,
                                         uint8_t *ciphertexts_or_null, uint8_t *tags_or_null, uint8_t *h_outs_or_null, uint8_t *revealed_or_null, uint8_t **proofs, size_t *proofs_len,
                                         size_t *proof_lens);
/* the chunk-proofs of one ECB, CBC or CTR message over a reveal key, ONE mask of ceil(len / 8) bytes over this call's message: hdr, h_in, states_or_null (a chain key
 * only) as zkaes_encrypt_digest_chunked_seeded_at; revealed_or_null receives len bytes.  A job split over calls passes each call its part of the message and of the mask */
int zkaes_encrypt_reveal_chunked_seeded_at(const uint8_t *msg, size_t len, const uint8_t *secret_key, const uint8_t *hdr, const uint8_t *h_in, const uint8_t *mask, size_t mask_len,
                                           const zkaes_pk *pk, const uint8_t *zk_seed32, uint64_t first_proof_index, uint8_t *ciphertext_or_null, uint8_t *states_or_null,
                                           uint8_t *revealed_or_null, uint8_t **proofs, size_t *proofs_len, size_t *proof_lens, size_t n_chunks);
/* host only: the chunk-proofs of one ECB, CBC or CTR job over a reveal key.  Chunk j's public input is what zkaes_verify_digest_chunked derives for it (key_tag NULL / 0
 * for a key without tag blocks, states NULL for a key without a digest), then its slice of mask (ceil(ciphertext_len / 8) bytes over the whole job) and of revealed
 * (ciphertext_len bytes).  n_chunks = 1 is the lone-proof form.  A mask bit at or beyond the length, or a non-zero revealed byte whose mask bit is 0, is an ERROR of the
 * call, not a rejection: ignoring such a byte would let a caller believe it proven */
int zkaes_verify_reveal_chunked(const zkaes_vk *vk, int circuit_kind, const uint8_t *proofs, const size_t *proof_lens, size_t n_chunks, const uint8_t *iv_or_icb, const uint8_t *ciphertext,
                                size_t ciphertext_len, const uint8_t *key_tag, size_t key_tag_len, const uint8_t *states, const uint8_t *mask, size_t mask_len, const uint8_t *revealed,
                                int *accepted_each, size_t *n_accepted);
/* host only: zkaes_verify_encryption_gcm_digest (h_out NULL for a key without a digest) with mask and revealed behind it; the same two errors */
int zkaes_verify_encryption_gcm_reveal(const zkaes_vk *vk, const uint8_t *proof, size_t proof_len, const uint8_t iv12[12], const uint8_t *aad, size_t aad_len, const uint8_t *ciphertext,
                                       size_t ciphertext_len, const uint8_t tag16[16], const uint8_t *key_tag, size_t key_tag_len, const uint8_t *h_in, const uint8_t *h_out,
                                       const uint8_t *mask, size_t mask_len, const uint8_t *revealed, int *accepted);
/* host only: zkaes_chunk_public_inputs for a reveal key: every row ends in the chunk's slice of mask and of revealed; the same two errors */
int zkaes_chunk_public_inputs_rv(int circuit_kind, size_t n_chunks, const uint8_t *iv_or_icb, const uint8_t *ciphertext, size_t ciphertext_len, const uint8_t *key_tag, size_t key_tag_len,
                                 const uint8_t *states, const uint8_t *mask, size_t mask_len, const uint8_t *revealed, uint8_t *out_bits, size_t *n_bits);
/* ---- GCM records longer than one proof: segment-proofs --------------------------------------------------
 * A record (iv, aad, ciphertext, tag) of L bytes whose ceil(L / 16) data blocks do not fit one proof is proven as n = ceil(ceil(L / 16) / c) >= 2 segment-proofs, c data
 * blocks each, the last with Lt = L - 16 c (n - 1) bytes.  Three roles, each with its own key: role 0 = head (fixed by c and A, the whole aad), 1 = mid (c), 2 = tail
 * (Lt).  Behind segment s < n - 1 stands the boundary commitment com_s = ONE SHA-256 compression from the initial value over key || zeros to 32 bytes || Y_s || salt_s,
 * Y_s = the GHASH accumulator after the segment's last block, salt_s = 16 random bytes: public input of segment s (com_out) and of segment s + 1 (com_in), so all n proofs
 * speak of one key and one GHASH chain, and together they are the lone GCM statement for the whole record.  Hiding of Y and the key rests on the salt.  Public-input
 * vector of a segment: 96 iv bits, 32 bits of ctr0 (big-endian bytes, the verifier sets 2 + s c), then head: 8 A aad bits, 128 c ciphertext bits, 256 com_out bits;
 * mid: 128 c ciphertext bits, com_in, com_out; tail: 8 Lt ciphertext bits, the 128 bits of the length block be64(8 A) || be64(8 L), the 128 tag bits, com_in.  L <= 2^20,
 * A <= 65536 and inside the head; 96-bit IVs and full tags only; no key tag and no digest on a segment key.  Every older GCM entry point refuses a segment key and the
 * segment entry points refuse every other key. */
#define ZKAES_CIRCUIT_AES_GCM_SEG 6   /* what zkaes_pk_mode reports for a segment key; synthesized by zkaes_synthesize_keys_gcm_seg only */
#define ZKAES_SEG_HEAD 0
#define ZKAES_SEG_MID 1
#define ZKAES_SEG_TAIL 2
/* units = c (head, mid) or Lt (tail); aad_length = A for a head, 0 otherwise; the rest as zkaes_synthesize_keys_ks */
int zkaes_synthesize_keys_gcm_seg(int role, unsigned key_bits, size_t units, size_t aad_length, size_t srs_num_constraints, size_t srs_num_variables, size_t srs_num_non_zero, unsigned flags,
                                  zkaes_pk **pk, zkaes_vk **vk);
/* out = {0 for a key that is no segment key, else 1 + role; data blocks; message bytes; aad bytes} */
int zkaes_pk_segment_info(const zkaes_pk *pk, uint64_t out[4]);
/* host only: zkaes_circuit_info / zkaes_circuit_matrix of a segment circuit.  The info query also fills out[9] = the joint matrix's non-zeros, out[10] = |H| and
 * out[11] = |K| (which zkaes_circuit_info leaves 0), so that segments can be sized against an SRS without a device */
int zkaes_circuit_info_gcm_seg(int role, unsigned key_bits, size_t units, size_t aad_length, uint64_t out[12]);
int zkaes_circuit_matrix_gcm_seg(int role, unsigned key_bits, size_t units, size_t aad_length, int which, uint64_t *n_rows, uint64_t *nnz, uint32_t *rowptr, uint32_t *col, int64_t *coeff);
/* host only: *n_segments = n for segments of c blocks; ys (NULL = the count only) receives Y_0 .. Y_{n-2}, 16 bytes each, ys_cap >= 16 (n - 1) */
int zkaes_gcm_boundaries(const uint8_t *message, size_t message_len, const uint8_t *secret_key, size_t key_len, const uint8_t iv12[12], const uint8_t *aad, size_t aad_len, size_t c,
                         uint8_t *ys, size_t ys_cap, size_t *n_segments);
/* host only: the boundary commitment of (key, y, salt) */
int zkaes_gcm_commit(const uint8_t *secret_key, size_t key_len, const uint8_t y16[16], const uint8_t salt16[16], uint8_t commitment32[32]);
/* as zkaes_aes_witness for a segment key.  header = 80 + A bytes: iv (12), ctr0 (4, big-endian), Y_in (16), salt_in (16), salt_out (16), the length block (16), the aad
 * (head); a field the key's role does not use is ignored */
int zkaes_aes_witness_gcm_seg(const zkaes_pk *pk, const uint8_t *message, size_t message_len, const uint8_t *secret_key, const uint8_t *header, size_t header_len, uint8_t *z, size_t z_cap,
                              size_t *z_len);
/* n independent segment proofs over one segment key, each under its own header (n x (80 + A) bytes, as zkaes_aes_witness_gcm_seg), side by side over the key's prover
 * contexts; seeds and first_proof_index as zkaes_encrypt_batch_seeded_at.  The caller answers for what the headers say (zkaes_gcm_boundaries, zkaes_gcm_commit give
 * the values of a real record): this is the building block for a record spread over processes or GPUs, and what the cost tool times */
int zkaes_encrypt_gcm_segment_batch_seeded_at(size_t n, const uint8_t *messages, size_t messages_len, const uint8_t *secret_keys, size_t secret_keys_len, const uint8_t *headers, size_t headers_len,
                                              const zkaes_pk *pk, const uint8_t *zk_seed32, uint64_t first_proof_index, uint8_t **proofs, size_t *proofs_len, size_t *proof_lens);
/* Segments [first_segment, first_segment + count) of one record, so that a record can be split over calls, ranks or GPUs; mid_or_null may be NULL when n = 2.  salts =
 * 16 (n - 1) bytes or NULL for OS randomness -- NULL only when the call covers the whole record, since every call of a split job must make the same commitments.
 * Segment s draws its zero-knowledge randomness from zk_seed32 at index s (NULL = the test_rng seed for every proof, as zkaes_encrypt_chunked_seeded).  The middle
 * segments run side by side over the mid key's prover contexts.  Receives, where the pointer is not NULL, the whole record's ciphertext (message_len), tag (16) and
 * commitments (32 (n - 1)); *proofs holds the call's `count` proofs back to back, proof_lens their lengths */
int zkaes_encrypt_gcm_segments_seeded_at(const uint8_t *message, size_t message_len, const uint8_t *secret_key, const uint8_t iv12[12], const uint8_t *aad, size_t aad_len, const zkaes_pk *head,
                                         const zkaes_pk *mid_or_null, const zkaes_pk *tail, const uint8_t *salts_or_null, const uint8_t *zk_seed32, size_t first_segment, size_t count,
                                         uint8_t *ciphertext_or_null, uint8_t *tag_or_null, uint8_t *commitments_or_null, uint8_t **proofs, size_t *proofs_len, size_t *proof_lens);
/* host only: the n segment-proofs of one record against ONE array of n - 1 commitments.  The verifier sets every ctr0, cuts the ciphertext, builds the length block
 * from aad_len and ciphertext_len as it sees them, and hands the tag to the tail alone.  accepted_each[s] per segment; a proof that does not parse is a rejected
 * segment; lengths that do not fit the keys, n_segments or commitments_len are an error of the call */
int zkaes_verify_gcm_segments(const zkaes_vk *head, const zkaes_vk *mid_or_null, const zkaes_vk *tail, const uint8_t *proofs, const size_t *proof_lens, size_t n_segments, size_t c,
                              const uint8_t iv12[12], const uint8_t *aad, size_t aad_len, const uint8_t *ciphertext, size_t ciphertext_len, const uint8_t tag16[16], const uint8_t *commitments,
                              size_t commitments_len, int *accepted_each, size_t *n_accepted);
/* ---- selective disclosure on segmented records.  A segment key synthesized with reveal = 1 proves, beside its role's statement above, revealed[i] =
 * mask_i ? M[i] : 0 over the segment's own len = 16 c (head, mid) or Lt (tail) bytes; its public input gains, behind everything listed above, 8 ceil(len / 8) mask bits
 * and 8 len revealed bits, in the order and bit order of the lone reveal form, and mask bits at or beyond len are pinned to zero.  There is ONE mask of ceil(L / 8) bytes
 * and ONE revealed array of L bytes over the whole record: segment boundaries are multiples of 16 bytes, so segment s is proven and checked under the mask bytes from
 * 2 c s on and the revealed bytes from 16 c s on, and head, mid and tail together are the lone reveal statement for (iv, aad, ciphertext, tag).  The aad is public and
 * not covered by the mask; commitments, salts, ctr0 and the length block are as above.  reveal = 0 is every segment key from before, bit for bit.  Every entry above
 * refuses a reveal = 1 key and the entries below refuse reveal = 0 keys and keys that are no segment keys; zkaes_pk_segment_info and zkaes_pk_reveal_info answer for
 * both.  The provers and the verifier treat a mask bit at or beyond L -- and the verifier a non-zero revealed byte under a zero mask bit -- as an invalid argument,
 * never as a rejected proof */
int zkaes_synthesize_keys_gcm_seg_rv(int role, unsigned key_bits, unsigned reveal, size_t units, size_t aad_length, size_t srs_num_constraints, size_t srs_num_variables,
                                     size_t srs_num_non_zero, unsigned flags, zkaes_pk **pk, zkaes_vk **vk);
/* host only: zkaes_circuit_info_gcm_seg / zkaes_circuit_matrix_gcm_seg with the reveal flag; reveal = 0 answers what they answer */
int zkaes_circuit_info_gcm_seg_rv(int role, unsigned key_bits, unsigned reveal, size_t units, size_t aad_length, uint64_t out[12]);
int zkaes_circuit_matrix_gcm_seg_rv(int role, unsigned key_bits, unsigned reveal, size_t units, size_t aad_length, int which, uint64_t *n_rows, uint64_t *nnz, uint32_t *rowptr, uint32_t *col,
                                    int64_t *coeff);
/* zkaes_aes_witness_gcm_seg for a reveal key: header as there (80 + A bytes), mask = the segment's ceil(len / 8) bytes */
int zkaes_aes_witness_gcm_seg_rv(const zkaes_pk *pk, const uint8_t *message, size_t message_len, const uint8_t *secret_key, const uint8_t *header, size_t header_len, const uint8_t *mask,
                                 size_t mask_len, uint8_t *z, size_t z_cap, size_t *z_len);
/* zkaes_encrypt_gcm_segment_batch_seeded_at for a reveal key: masks = n x ceil(len / 8) bytes, one mask per proof; revealed_or_null receives n x len bytes */
int zkaes_encrypt_gcm_segment_reveal_batch_seeded_at(size_t n, const uint8_t *messages, size_t messages_len, const uint8_t *secret_keys, size_t secret_keys_len, const uint8_t *headers,
                                                     size_t headers_len, const uint8_t *masks, size_t masks_len, const zkaes_pk *pk, const uint8_t *zk_seed32, uint64_t first_proof_index,
                                                     uint8_t *revealed_or_null, uint8_t **proofs, size_t *proofs_len, size_t *proof_lens);
/* zkaes_encrypt_gcm_segments_seeded_at for three reveal keys under ONE mask of ceil(message_len / 8) bytes over the record.  revealed_or_null receives the whole record's
 * message_len revealed bytes whichever segments the call proves; a job split over calls passes every call the same mask and salts and stays byte-identical to the whole */
int zkaes_encrypt_gcm_segments_reveal_seeded_at(const uint8_t *message, size_t message_len, const uint8_t *secret_key, const uint8_t iv12[12], const uint8_t *aad, size_t aad_len,
                                                const zkaes_pk *head, const zkaes_pk *mid_or_null, const zkaes_pk *tail, const uint8_t *salts_or_null, const uint8_t *mask, size_t mask_len,
                                                const uint8_t *zk_seed32, size_t first_segment, size_t count, uint8_t *ciphertext_or_null, uint8_t *tag_or_null, uint8_t *commitments_or_null,
                                                uint8_t *revealed_or_null, uint8_t **proofs, size_t *proofs_len, size_t *proof_lens);
/* host only: zkaes_verify_gcm_segments for the proofs of three reveal keys against ONE mask (mask_len = ceil(ciphertext_len / 8)) and ONE revealed array (revealed_len =
 * ciphertext_len).  Proofs of reveal = 0 keys are never accepted here, nor proofs of reveal = 1 keys by zkaes_verify_gcm_segments: a key that carries its public-input
 * count raises, any other rejects */
int zkaes_verify_gcm_segments_reveal(const zkaes_vk *head, const zkaes_vk *mid_or_null, const zkaes_vk *tail, const uint8_t *proofs, const size_t *proof_lens, size_t n_segments, size_t c,
                                     const uint8_t iv12[12], const uint8_t *aad, size_t aad_len, const uint8_t *ciphertext, size_t ciphertext_len, const uint8_t tag16[16],
                                     const uint8_t *commitments, size_t commitments_len, const uint8_t *mask, size_t mask_len, const uint8_t *revealed, size_t revealed_len,
                                     int *accepted_each, size_t *n_accepted);
/* src/ops.rs toy gates proven with Marlin (public input: none) */
int zkaes_prove_ops(const zkaes_pk *pk, uint32_t x, uint32_t y, const uint8_t *zk_seed32, uint8_t **proof, size_t *proof_len);
/* generic verify: public_input_bits = instance assignment without the leading One, one byte (0/1) per variable */
int zkaes_verify(const zkaes_vk *vk, const uint8_t *proof, size_t proof_len, const uint8_t *public_input_bits, size_t n_bits, int *accepted);
/* verifying-key transport, library-private layout v2 ("ZVK2", the unpadded public-input count, then the ark-serialize compressed image below): validated like the ark
 * path (canonical field elements, curve and prime-order-subgroup membership, index-info bounds) -- safe on untrusted bytes */
int zkaes_vk_serialize(const zkaes_vk *vk, uint8_t **out, size_t *out_len);
int zkaes_vk_deserialize(const uint8_t *bytes, size_t len, zkaes_vk **vk);
/* verifying-key transport in the ark-serialize 0.3 compressed layout of ark_marlin::IndexVerifierKey<Fr, MarlinKZG10<Bls12_377, _>>
 * (759 bytes for the AES keys): what `VerifyingKey::serialize` writes / `VerifyingKey::deserialize` reads on the Rust side of
 * src/lib.rs:116 -- SURVEY.md 8f item 1.  Layout restated from the published crates (the reference holds no VK bytes to pin it). */
int zkaes_vk_serialize_ark(const zkaes_vk *vk, uint8_t **out, size_t *out_len);
int zkaes_vk_deserialize_ark(const uint8_t *bytes, size_t len, zkaes_vk **vk);
/* the same key as serialize_uncompressed writes it (G1 as x || y = 96 B, G2 = 192 B, the infinity flag in the top bits of y's last byte; everything else identical;
 * 1,431 bytes): the form `IndexVerifierKey::deserialize_uncompressed` / `::deserialize_unchecked` read -- and the index_vk prefix of the uncompressed proving-key image */
int zkaes_vk_serialize_ark_uncompressed(const zkaes_vk *vk, uint8_t **out, size_t *out_len);

/* host-only: assemble a verifying key from an index made elsewhere over the SAME universal SRS, i.e. KZG10::setup replayed from
 * ark_std::test_rng() (the reference's generate_rand(), src/lib.rs:139): info = {num_variables, num_constraints, num_non_zero,
 * num_instance (padded), num_public_inputs, max_degree, supported_degree}; index_comms = 6 x 96 B affine Montgomery (row col a_val b_val
 * c_val row_col); beta = 32 B Montgomery Fr, must equal the replayed trapdoor (else error).  g, gamma_g, h are the replay's random curve
 * points, beta_h = beta*h, shift powers = beta^(max_degree - bound) * g. */
int zkaes_vk_from_trapdoor(const uint64_t info[7], const uint8_t *index_comms, const uint8_t *beta, zkaes_vk **vk);

/* ---- introspection used by tests / bench ----------------------------------------------------------------------- */
/* counters the reference logs through debug_constraint_system_status (src/helpers/mod.rs:73-81) and the Marlin index sizes:
 * out[0..11] = raw constraints, raw instance, raw witness, nnz A, nnz B, nnz C, padded constraints, padded instance,
 *              padded witness, joint nnz, |H|, |K| */
int zkaes_pk_info(const zkaes_pk *pk, uint64_t out[12]);
/* host-only circuit compilation (no GPU): same counters (joint nnz, |H|, |K| = 0) */
int zkaes_circuit_info(int circuit_kind, size_t plaintext_length, uint64_t out[12]);
/* host-only: CSR of matrix which (0 A, 1 B, 2 C) after padding.  Call with NULL arrays to get sizes. */
int zkaes_circuit_matrix(int circuit_kind, size_t plaintext_length, int which, uint64_t *n_rows, uint64_t *nnz, uint32_t *rowptr, uint32_t *col, int64_t *coeff);
/* copy an intermediate buffer of the LAST proof made with this key to the host ("z", "trace", "z_a_evals", "z_b_evals", "w", "z_a", "z_b",
 * "mask_poly", "t", "g_1", "h_1", "g_2", "h_2", index polys "row", "col", "a_val", "b_val", "c_val", "row_col" (+"_evals")).
 * Field elements are raw little-endian Montgomery limbs (32 B).  Returns the byte count in *len. */
int zkaes_pk_debug_fetch(const zkaes_pk *pk, const char *name, uint8_t **out, size_t *len);
/* per-phase wall times of the last proof: witness, round1, round2, round3, open, total (ms) */
int zkaes_pk_timings(const zkaes_pk *pk, double out[6]);
/* accumulated MSM statistics since the last reset, one entry per k_accumulate LAUNCH (a degree-bounded commitment = one prepared state finished against the plain and
 * the shifted powers = two launches, each booked with its own event pair, points and pairs): bucket-accumulation kernel ms (HIP events), total MSM wall ms, points,
 * launches, (point, window) pairs */
int zkaes_msm_stats(double out[5], int reset);
/* The library's ACTUAL op lists for one proof on this key ("recompute W + S + T + M from the actual op lists and print the lists"): proves `message` once with
 * the op recorder open -- throughput_path != 0: as a multi-proof call runs a proof (window tables, one lane), 0: as a lone zkaes_encrypt does -- and returns JSON (release
 * with zkaes_bytes_free): {"h","k","x","variables","constraints","nnz":[A,B,C],"blocks","path","ntt":[[points, transforms sharing the launch],...],
 * "msm":[[points,"buckets"|"second_bases"|"class_sum"],...]}.  The recorder is process-global: call it with no other proof in flight. */
int zkaes_pk_op_lists(const zkaes_pk *pk, const uint8_t *message, size_t message_len, const uint8_t secret_key[16], int throughput_path, uint8_t **json, size_t *json_len);
/* free / total device memory of the calling thread's current device (hipMemGetInfo) */
int zkaes_mem_info(uint64_t *free_bytes, uint64_t *total_bytes);

/* ---- kernel-level entry points (parity tests + roofline measurement) -------------------------------------------- */
/* field_id: 377 or 381 (BLS12-377 / BLS12-381 scalar field).  data: n x 32 B Montgomery limbs, host memory, transformed in place.
 * n must be a power of two.  inverse != 0 -> IFFT (scaled by 1/n).  Natural order in and out. */
int zkaes_ntt(int field_id, uint8_t *data, size_t n, int inverse);
/* the same transform on the coset g D of the size-n domain D, g = W^coset_c with W the primitive 2^lg_big-th root (2^lg_big > n, 0 < coset_c < 2^lg_big / n): forward =
 * the values p(g w^i) of the coefficient vector, inverse = the coefficients from those values.  The prover's second round runs on such cosets of H inside the 4|H| domain. */
int zkaes_ntt_coset(int field_id, uint8_t *data, size_t n, int inverse, int coset_c, int lg_big);
/* `count` (1..12) transforms of one shape in shared launches, as the prover's rounds 1 and 2 issue them: data = count x n x 32 B, transformed in place; coset_c[i] = 0 for a
 * plain transform, > 0 for the coset W^coset_c[i] D (coset_c may be NULL: all plain; lg_big as in zkaes_ntt_coset, ignored when no job is a coset transform). */
int zkaes_ntt_batch(int field_id, uint8_t *data, size_t n, int count, int inverse, const int *coset_c, int lg_big);
/* ---- kernel-level entry points for tests ------------------------------------------------------------------------- */
/* One call = one launch wrapper of the prover's polynomial layer (csrc/kernels_poly.hip) or of a transform entry point the prover uses and zkaes_ntt does not reach, so that
 * tests can compare every multi-launch algorithm with a big-integer model at the boundaries of its block, chunk and level constants.  Host buffers of 32-byte little-endian
 * Montgomery limbs in and out, BLS12-377 Fr unless a field_id says otherwise; every element must be canonical (< r).  Diagnostic use: each call allocates, copies and waits. */
/* q (len - m elements) = p / (X^m - 1), rem_or_null (m elements) = the remainder; needs len > m >= 1.  with_scratch != 0 hands the library the scratch its segmented
 * kernels want, which it then uses for chains of 64 and more steps; 0: one lane per residue class at every length */
int zkaes_poly_divide_by_vanishing(const uint8_t *p, size_t len, size_t m, int with_scratch, uint8_t *q, uint8_t *rem_or_null);
/* q (len - 1 elements) = p / (X - z), remainder dropped; len < 2 writes nothing */
int zkaes_poly_divide_by_linear(const uint8_t *p, size_t len, const uint8_t z[32], uint8_t *q);
/* out[i] = polys[i](x[i]) for count = 1..8 polynomials of lens[i] coefficients (0 allowed: the value is 0, polys[i] may be NULL); x, out: count elements */
int zkaes_poly_eval_multi(const uint8_t *const *polys, const size_t *lens, const uint8_t *x, int count, uint8_t *out);
/* v[i] <- post / v[i] in place (post_or_null == NULL: 1 / v[i]); zeros stay zero.  throughput_variant != 0: run as between overlapping proofs of a multi-proof call, where
 * the library picks its 16-elements-per-lane Fermat kernel; 0: as a lone call (4 per lane, Euclidean inverse, up to 2^21 elements; the other kernel above) */
int zkaes_batch_inverse(uint8_t *v, size_t n, const uint8_t *post_or_null, int throughput_variant);
/* out[i] = sum_j scalars[j] polys[j][i] for i < n, term j contributing below lens[j] <= n only; count = 1..8 */
int zkaes_poly_lincomb(const uint8_t *const *polys, const size_t *lens, const uint8_t *scalars, int count, size_t n, uint8_t *out);
/* r(a, y) = (a^n - y^n) / (a - y) at y = g[c] h_i, h_i the elements of the size-2^lg_n domain (the library's own table), for c < ncosets <= 3 cosets.
 * idx_or_null == NULL: out = ncosets x n elements, coset-major; otherwise out = ncosets x nidx elements, the values at the given indices */
int zkaes_vanishing_quotient_evals(int lg_n, const uint8_t *g, int ncosets, const uint8_t a[32], const uint32_t *idx_or_null, size_t nidx, uint8_t *out);
/* round 2 on a coset: out[i] = r[i] (eta_a A + eta_b B + eta_c A B) - t[i] Z, A = za[i] + ca, B = zb[i] + cb, Z = z[i] + cz; consts = ca, cb, cz, eta_a, eta_b, eta_c */
int zkaes_q1_coset_pointwise(const uint8_t *r, const uint8_t *za, const uint8_t *zb, const uint8_t *t, const uint8_t *z, const uint8_t consts[192], size_t n, uint8_t *out);
/* round 3 on a coset: out[i] = ((ea va + eb vb + ec vc) - (alpha_beta - alpha row - beta col + rc) f)[i] vinv; arrays = row, col, va, vb, vc, rc, f (k elements each);
 * consts = alpha, beta, alpha_beta, ea, eb, ec, vinv */
int zkaes_h2_coset(const uint8_t *const arrays[7], const uint8_t consts[224], size_t k, uint8_t *out);
/* h1 (2n) and g1 (n - 1) from the interpolants q0 (on H), q1, q3 (on W H, W^3 H) of q_1 - mask and the mask (3n coefficients); inv2 = 1/2, inv2zeta = 1/(2 zeta), zeta = W^n */
int zkaes_q1_combine(const uint8_t *q0, const uint8_t *q1, const uint8_t *q3, const uint8_t *mask, const uint8_t inv2[32], const uint8_t inv2zeta[32], size_t n, uint8_t *h1, uint8_t *g1);
/* out[j] = in[j] g^j for j < n, in zero-padded beyond in_len */
int zkaes_coset_scale(const uint8_t *in, size_t in_len, const uint8_t g[32], size_t n, uint8_t *out);
/* zp (n + 1 elements) = w (X^m - 1) + x_poly: zp[i] = w[i - m] - w[i] + x_poly[i], each term where its index exists (w: wlen, x_poly: m elements) */
int zkaes_z_poly_from_w(const uint8_t *w, size_t wlen, const uint8_t *x_poly, uint32_t m, size_t n, uint8_t *zp);
/* zkaes_ntt / zkaes_ntt_coset (coset_c > 0) of an input of in_len <= n elements that the first pass's gather pads with zeros; out: n elements */
int zkaes_ntt_padded(int field_id, const uint8_t *in, size_t in_len, size_t n, int inverse, int coset_c, int lg_big, uint8_t *out);
/* the transform on the coset g D of a generator that need not be a root of unity: forward out[i] = p(g w^i) from the in_len coefficients (table of g^i riding on the first
 * pass), inverse the coefficients from such values (table of g^-i at the last store); n = 2 .. 2^28 */
int zkaes_ntt_scaled(const uint8_t g[32], const uint8_t *in, size_t in_len, size_t n, int inverse, uint8_t *out);
/* ---- the MSM forms the prover calls (csrc/marlin.cpp), none of which zkaes_msm / zkaes_msm_table reach; test and debug entry points (tests/test_gpu_msm_forms.py).
 * BLS12-377 only.  bases: standard affine points (96 B each, Montgomery coordinates), scalars: Montgomery Fr (32 B each), as zkaes_msm takes them; every call converts the
 * bases (and builds the window tables) on the device, allocates, copies and waits.  edwards != 0: the prover's law (twisted Edwards records; the bases MUST lie in the
 * prime-order subgroup), 0: the Weierstrass law.  Results: affine x, y (96 B) + an infinity flag per point.  Null pointers, ranges outside the bases, a count outside
 * 1..8 and window bits outside [2, 22] are refused before anything is allocated. */
/* sum_i vals[v][i] * bases[i] for `count` (1..8) vectors of n int8 values (vals: count x n bytes), one after the other on ONE workspace and stream -- the Lagrange-basis
 * commitments of w, z_A, z_B.  ok_out[v] = 1 and the sum in out_xy[v], out_inf[v] when class_sum accepted vector v; 0 (outputs zeroed) when it declined: a value outside
 * [-2, 2], or on the Weierstrass law an addition of a point to itself or its negative inside a chunk.  prior_msm_points > 0 (<= n): a generic MSM over that many of the
 * same bases runs on the workspace first, so that the class sums carve their scratch from a bucket array another MSM sized (a prover context's second proof). */
int zkaes_class_sum(const uint8_t *bases, size_t n, const int8_t *vals, int count, int edwards, size_t prior_msm_points, int *ok_out, uint8_t *out_xy, int *out_inf);
/* per-window Pippenger over TWO scalar vectors in one instance (the opening witness over plain + shifted powers): sum_i scal1[i] bases[i] + sum_j scal2[j] bases[val_off2 + j];
 * n1 <= nbases, val_off2 + n2 <= nbases; either length may be 0 */
int zkaes_msm_pair(const uint8_t *bases, size_t nbases, const uint8_t *scal1, size_t n1, const uint8_t *scal2, size_t n2, size_t val_off2, int edwards, uint8_t *out_xy, int *out_inf);
/* the same in table mode over a table LONGER than the vectors: window tables of all `stride` bases, sum_i scal1[i] bases[off1 + i] + sum_j scal2[j] bases[off2 + j];
 * off1 + n1 <= stride, off2 + n2 <= stride (else "msm_table: range exceeds the table"); n2 = 0 with off1 > 0 is the single-vector offset case */
int zkaes_msm_table_pair(const uint8_t *bases, size_t stride, const uint8_t *scal1, size_t n1, size_t off1, const uint8_t *scal2, size_t n2, size_t off2, int window_bits, int edwards,
                         uint8_t *out_xy, int *out_inf);
/* ONE digit pass, two base ranges (a degree-bounded commitment: plain + shifted powers), Edwards law: out[0] = sum_i scalars[i] bases[off + i], out[1] = sum_i scalars[i]
 * bases[off + shift + i]; off + shift + n <= nbases.  window_bits = 0: per-window buckets (sequential when the two sets of window sums exceed one reduction's 64),
 * > 0: window tables of stride nbases.  out_xy: 2 x 96 B, out_inf: 2 flags */
int zkaes_msm_second_bases(const uint8_t *bases, size_t nbases, const uint8_t *scalars, size_t n, size_t off, size_t shift, int window_bits, uint8_t *out_xy, int *out_inf);
/* ---- a SEQUENCE of those forms on ONE workspace and ONE stream, as a prover context and the batch verifier run them (tests/test_gpu_msm_workspace.py): TEST SURFACE.
 * The contract under test is "any MSM form after any other on one workspace": the workspace keeps its armed words (the overflow list's counter, length and segment total,
 * the class-sum flag word, the tail kernel's ticket and the deferred count) and every index-bearing buffer of the MSM before (pairs, bucket ranges, visiting order, overflow
 * list, partition scratch) from step to step, and only ever grows.  bases: nbases standard affine points, uploaded once and converted, before the first step, to the forms
 * the steps need (Affine28 / Niels28 records, window tables of stride nbases per distinct window_bits and law).  scalars: nscalars Montgomery Fr; class_vals: nvals int8.
 * A step names its inputs by element offsets into those three arrays:
 *   ZKAES_STEP_WINDOW    msm_prepare + msm_finish on the bases from off1 on: sum_i scalars[scal1 + i] bases[off1 + i] + sum_j scalars[scal2 + j] bases[off1 + off2 + j]
 *                        (i < n1, j < n2; off2 = msm_prepare's val_off2; n2 = 0: one vector)
 *   ZKAES_STEP_TABLE     msm_prepare_table(window_bits, stride = nbases) + msm_finish: sum_i scalars[scal1 + i] bases[off1 + i] + sum_j scalars[scal2 + j] bases[off2 + j]
 *   ZKAES_STEP_SECOND    one prepared state, msm_finish2 (Edwards law only): point 0 = sum_i scalars[scal1 + i] bases[off1 + i], point 1 the same over
 *                        bases[off1 + shift + i]; window_bits = 0: per-window buckets, > 0: window tables
 *   ZKAES_STEP_CLASS     class_sum: sum_i class_vals[scal1 + i] bases[off1 + i], i < n1; accepted = 0 (point zeroed) when class_sum declines
 *   ZKAES_STEP_REFINISH  msm_finish AGAIN on the state the step before prepared (a WINDOW, TABLE, SECOND or REFINISH step that succeeded), every base index moved up by
 *                        `shift`: the sum of that step's scalars over bases[index + shift]
 * edwards selects the law of the step's accumulation (the prepared state itself belongs to neither).  poison != 0: before every step but the first the workspace's
 * ACCUMULATOR buffers (buckets, both first-level sums, the reduction's partials, the overflow partials) are filled with 0xAB bytes on the stream; the armed words and the
 * index-bearing buffers keep what the step before left, which is the state under test.
 * Refused before anything is allocated (non-zero return, zkaes_last_error): null pointers, nbases or nsteps out of range (1 .. ZKAES_MSM_SEQ_MAX_STEPS steps), an unknown
 * kind, a scalar or value range outside its array, offsets above 2^26, window bits outside [2, 22] (or more than 8 distinct ones per law), a SECOND step on the Weierstrass
 * law, a REFINISH with no preparing step before it.  Whether a step's BASE range fits is judged when the step runs, as the single-form entry points above and
 * msm_prepare_table judge it: such a step -- like any other the library refuses without touching the device -- gets status 1 and its message (nul-terminated, at most
 * ZKAES_MSM_SEQ_ERR_BYTES - 1 characters) in out_errors, zeroed points, and the sequence GOES ON with the next step.  A HIP error ends the call.
 * Per step i: out_xy[192 i ..] two points (the second one only for SECOND), out_inf[2 i ..], out_accepted[i] (1 unless a class sum was declined or the step refused),
 * out_status[i], out_errors[ZKAES_MSM_SEQ_ERR_BYTES i ..]. */
#define ZKAES_STEP_WINDOW 0
#define ZKAES_STEP_TABLE 1
#define ZKAES_STEP_SECOND 2
#define ZKAES_STEP_CLASS 3
#define ZKAES_STEP_REFINISH 4
#define ZKAES_MSM_SEQ_MAX_STEPS 32
#define ZKAES_MSM_SEQ_ERR_BYTES 128
typedef struct zkaes_msm_step {
    uint32_t kind, edwards, window_bits, reserved;      /* reserved = 0 */
    uint64_t n1, off1, scal1;                           /* first vector: length, first base, first scalar (CLASS: first value) */
    uint64_t n2, off2, scal2;                           /* second vector (WINDOW, TABLE) */
    uint64_t shift;                                     /* SECOND, REFINISH */
} zkaes_msm_step;
int zkaes_msm_sequence(const uint8_t *bases, size_t nbases, const uint8_t *scalars, size_t nscalars, const int8_t *class_vals, size_t nvals, const zkaes_msm_step *steps, size_t nsteps,
                       int poison, uint8_t *out_xy, int *out_inf, int *out_accepted, int *out_status, char *out_errors);
/* ---- kernel-level entry points of the prover's R1CS and randomness kernels (csrc/kernels_witness.hip, csrc/kernels_poly.hip): TEST SURFACE, not product API -- the layer
 * between the AES trace and the polynomials, which otherwise runs only inside whole proofs (tests/test_gpu_r1cs.py compares each with the big-integer model of
 * tests/r1cs_model.py).  BLS12-377 Fr; field elements are 32-byte Montgomery limbs, canonical (< r), not checked one by one.  Every call uploads, launches, copies back and
 * waits; every output and scratch buffer is filled with 0xAB bytes on the device first, so a slot a kernel does not write is visible.  All arguments are checked before
 * anything is allocated or launched. */
/* k_spmv_bits: out_field[r] = sum_i coeff[i] z[col[i]] over row r of the CSR triple (rowptr: rows + 1 entries from 0, non-decreasing; col[i] < ncols) for r < rows, zero for
 * rows <= r < rows_out; out_small (rows_out int8, may be NULL) = the same sums clamped to [-127, 127].  z: ncols bytes, 0 or 1.  |sum| must stay below 2^62. */
int zkaes_spmv_bits(const uint32_t *rowptr, const uint32_t *col, const int64_t *coeff, size_t rows, size_t rows_out, const uint8_t *z, size_t ncols, uint8_t *out_field, int8_t *out_small_or_null);
/* the index map "position on H -> instance / witness variable" in its three kernels and k_bits_to_field: z = m instance bytes then num_witness witness bytes (0 / 1),
 * x_evals = n elements.  out_classes (n int8) = w_classes, out_w_evals (n elements) = w_evals, out_z_evals_h (n elements) = z_evals_h, out_x_field (m elements) =
 * bits_to_field(z, m).  n, m powers of two, m < n, num_witness <= n - m. */
int zkaes_w_maps(const uint8_t *z, size_t n, size_t m, size_t num_witness, const uint8_t *x_evals, int8_t *out_classes, uint8_t *out_w_evals, uint8_t *out_z_evals_h, uint8_t *out_x_field);
/* round 2's t on H: the matrices A, B, C (index 0, 1, 2 of the three arrays; CSR triples of `rows` rows, columns < n) go through the SAME table builder as a proving key
 * (csrc/marlin_host.hpp build_t_tables), then k_t_partials / k_t_columns / k_t_heavy.  out[h] = sum over entries of column reindex(h) of eta_M coeff r_alpha[row]
 * (r_alpha: n elements, etas: eta_a, eta_b, eta_c).  stats = {segments, heavy columns, the largest segment count of one column} of the tables built. */
int zkaes_t_evals(size_t n, size_t m, size_t rows, const uint32_t *const rowptr[3], const uint32_t *const col[3], const int64_t *const coeff[3], const uint8_t *r_alpha,
                  const uint8_t etas[96], uint8_t *out, uint64_t stats[3]);
/* lagrange_scalars: out_lag[k] = L_k(beta) on the domain of size 2^lg_n, out_lag_w[k] = 0 at the multiples of 2^(lg_n - lg_m), else L_k(beta) / (beta^(2^lg_m) - 1).
 * 0 <= lg_m < lg_n <= 24.  beta^(2^lg_m) = 1 is outside the contract of out_lag_w (the inverse of zero is taken). */
int zkaes_lagrange_scalars(int lg_n, int lg_m, const uint8_t beta[32], uint8_t *out_lag, uint8_t *out_lag_w);
/* k_f_from_tables: out[i] = (ea va[i] + eb vb[i] + ec vc[i]) rb[ci[i]] ra[ri[i]] for i < k; va, vb, vc: k elements, ra, rb: n elements, ri[i], ci[i] < n */
int zkaes_f_evals_from_tables(const uint8_t *va, const uint8_t *vb, const uint8_t *vc, const uint8_t ea[32], const uint8_t eb[32], const uint8_t ec[32], const uint8_t *ra, const uint8_t *rb,
                              const uint32_t *ri, const uint32_t *ci, size_t k, size_t n, uint8_t *out);
/* chacha_field_stream: `count` field elements drawn as ark-ff's Fp::rand draws them from the ChaCha word stream of `key_words` (rounds 8, 12 or 20; 64-bit block counter)
 * from word `word_pos` on; *next_word_pos = the word after the last accepted candidate.  max_cand = 0: the prover's batch size; > 0: at most that many candidates per
 * batch, so that the refill branch runs (the results must not depend on it). */
int zkaes_chacha_field_stream(const uint32_t key_words[8], int rounds, uint64_t word_pos, size_t count, uint32_t max_cand, uint8_t *out, uint64_t *next_word_pos);
/* k_mask_fixup, in place on 3 n elements: p[0] -= p[0] + p[n] + p[2n] */
int zkaes_mask_fixup(uint8_t *p, size_t n);
/* ---- kernel-level entry points of the kernels that BUILD A KEY (csrc/kernels_msm.hip k_power_scalars, k_fixed_base, k_table_next, k_convert_bases_te; csrc/kernels_poly.hip
 * k_index_rowcol, k_index_vals): TEST SURFACE, not product API -- they run once per SRS or per key inside key synthesis and everything proved afterwards rests on their output
 * (tests/test_gpu_keysynth.py compares each with the CPU oracle and the integer model of tests/keysynth_model.py).  Field elements are 32-byte Montgomery limbs, canonical; a
 * point is 96 bytes of standard affine x || y (Montgomery coordinates) and the point at infinity is 96 ZERO bytes, in and out.  curve_id: 377 or 381.  Every call uploads,
 * launches, copies back and waits; every output buffer is filled with 0xAB bytes on the device first.  All arguments are checked before anything is allocated or launched;
 * counts are limited to 2^20. */
/* fixed_base_powers: out[i] = beta^(from + i) * base for i < count.  chunk: points per launch, 0 = the 2^20 of key synthesis; a smaller one makes the chunk loop run more than
 * once (the result must not depend on it). */
int zkaes_fixed_base_powers(int curve_id, const uint8_t base_xy[96], const uint8_t beta[32], uint64_t from, size_t count, size_t chunk, uint8_t *out);
/* fixed_base_scalars (BLS12-377): out[i] = scalars[i] * base; chunk as above */
int zkaes_fixed_base_scalars(const uint8_t base_xy[96], const uint8_t *scalars, size_t count, size_t chunk, uint8_t *out);
/* table_next: out[i] = 2^(width of window j - 1) * prev[i], window-table copy j from copy j - 1 under window_bits (2..22); 1 <= j < the number of copies */
int zkaes_table_next(int curve_id, const uint8_t *prev, size_t count, int window_bits, int j, uint8_t *out);
/* build_window_tables: out = all copies, copy j (n points) at out + 96 n j: copy 0 = bases, copy j = 2^(offset of window j) * bases */
int zkaes_build_window_tables(int curve_id, const uint8_t *bases, size_t n, int window_bits, uint8_t *out);
/* convert_bases_te (BLS12-377): out = n raw Niels28 records of ZKAES_NIELS_RECORD_BYTES each -- (y - x, y + x, 2 d x y) of the point on the twisted Edwards model as three
 * vectors of 14 little-endian 32-bit words holding 28-bit limbs (Montgomery form, radix 2^392), then padding.  Infinity gives the identity (1, 1, 0); a point of order 2 or 4
 * is refused. */
#define ZKAES_NIELS_RECORD_BYTES 192
int zkaes_convert_bases_te(const uint8_t *src, size_t n, uint8_t *out);
/* index_evals over the library's own table of the size-2^lg_n domain: entry i < cnt of the joint matrix sits at column ci[i], row ri[i] (both < 2^lg_n) with the coefficients
 * ca[i], cb[i], cc[i]; entries cnt <= i < k = 2^lg_k are padding.  Each output holds k + ZKAES_INDEX_EVALS_TAIL elements: the k values, then what the kernels left of the 0xAB
 * fill behind them (all of it, unless a kernel wrote out of its range).  uinv_or_null: the scratch vector after the batch inversion, 1 / u_H(x, x) per entry and zero on the
 * padding. */
#define ZKAES_INDEX_EVALS_TAIL 64
int zkaes_index_evals(const uint32_t *ci, const uint32_t *ri, const int64_t *ca, const int64_t *cb, const int64_t *cc, size_t cnt, int lg_k, int lg_n, uint8_t *row, uint8_t *col, uint8_t *rowcol,
                      uint8_t *va, uint8_t *vb, uint8_t *vc, uint8_t *uinv_or_null);
/* TEST-ONLY: ONE field or curve operation of csrc/ff.cuh, ff28.cuh, ff29.cuh, ec28.cuh, te28.cuh per launch, on raw limbs exactly as the operation sees them (no conversion
 * in or out, so lazy and non-canonical operands can be passed).  op: an id of csrc/arith_probe.cuh ZK_PROBE_OPS (named by api.py ARITH_OPS, which also holds the words per
 * case) or of ZK_PROBE_ZIP_OPS (api.py ARITH_ZIP_OPS: te_madd_hot's zipped products); in: n_cases x input words, out: n_cases x output words; 1 <= n_cases <= 65536.  tests/test_gpu_arith.py compares it with the big-integer model. */
int zkaes_arith_probe(int op, const uint32_t *in, size_t n_cases, uint32_t *out);

/* ---- MSM ---- */
/* curve_id 377 / 381.  bases: n x 96 B affine (x||y Montgomery), scalars: n x 32 B Montgomery Fr; out_xy 96 B, *out_inf = 1 if infinity */
int zkaes_msm(int curve_id, const uint8_t *bases, const uint8_t *scalars, size_t n, uint8_t *out_xy, int *out_inf);
/* host-side sum of n affine points (n x 96 B, inf[i] != 0 marks the point at infinity; inf may be NULL): the local EC add that follows the
 * all-gather when ONE MSM is sharded by point range over ranks (SURVEY.md 8e "inside one proof"; the upstream analogue is the final fold of the
 * per-window sums in ark-ec's VariableBaseMSM::multi_scalar_mul).  Runs on the host: a few hundred field products. */
int zkaes_g1_sum(int curve_id, const uint8_t *points_xy, const int *inf, size_t n, uint8_t *out_xy, int *out_inf);
/* ---- ONE MSM sharded by point range over the GPUs of a node with a device-resident exchange (SURVEY.md 8e "inside one proof"; north_star's "single RCCL
 * all-reduce of bucket partials over xGMI" -- EC addition is not an RCCL reduction operator, hence all-gather + local fold).  Every rank:
 *   1. zkaes_msm_sharded_plan(curve, n_total, ...)           -> window plan of the WHOLE MSM + bytes of one rank's payload (n_windows x 192 B)
 *   2. zkaes_msm_window_sums_dev(curve, bases, scalars of ITS slice, n_local, n_total, dev_out, bytes): Pippenger over the slice, the n_windows
 *      XYZZ window sums are left IN DEVICE MEMORY at dev_out (e.g. row `rank` of a [world, bytes] torch.uint8 CUDA tensor)
 *   3. one all-gather of those rows over RCCL (HBM to HBM over xGMI; torch.distributed.all_gather_into_tensor)
 *   4. zkaes_msm_fold_window_sums_dev(curve, dev_in = the gathered [world, bytes] block, world, n_total, out): per-window sum over ranks on the
 *      device, Horner over the windows -> the MSM result.  aes_zero_knowledge_proof_circuit_amd/sharding.py msm_sharded_device is this sequence. */
int zkaes_msm_sharded_plan(int curve_id, size_t n_total, int *window_bits, int *n_windows, size_t *bytes_per_rank);
int zkaes_msm_window_sums_dev(int curve_id, const uint8_t *bases, const uint8_t *scalars, size_t n_local, size_t n_total, void *dev_out, size_t dev_out_bytes);
int zkaes_msm_fold_window_sums_dev(int curve_id, const void *dev_in, int world, size_t n_total, uint8_t *out_xy, int *out_inf);
/* The same sharding on the PROVER'S OWN path, for commitments over a key's SRS (src/lib.rs:111 -> KZG10::commit): the key's powers_of_g on the curve's twisted Edwards model,
 * fixed-base window tables, ONE bucket set -- so a rank's share is ONE partial sum instead of one per window.  Every rank:
 *   1. zkaes_pk_msm_partial_dev(pk, scalars of ITS slice (n_local x 32 B Montgomery Fr), n_local, offset of the slice in powers_of_g, dev_out, 192): the slice's sum as one XYZZ
 *      point (192 B) left IN DEVICE MEMORY (row `rank` of a [world, 192] CUDA tensor); an empty share is the point at infinity
 *   2. one all-gather of the rows over RCCL
 *   3. zkaes_msm_fold_partials_dev(377, dev_in = the gathered block, world, out): sum over ranks on the device -> the commitment (affine).
 * Needs a key with tables (zkaes_pk_tables_built).  aes_zero_knowledge_proof_circuit_amd/sharding.py msm_sharded_srs_device is this sequence. */
int zkaes_pk_msm_partial_dev(const zkaes_pk *pk, const uint8_t *scalars, size_t n_local, size_t offset, void *dev_out, size_t dev_out_bytes);
int zkaes_msm_fold_partials_dev(int curve_id, const void *dev_in, int world, uint8_t *out_xy, int *out_inf);
/* The proving key as the reference would hold it (src/lib.rs:138-174 returns simpleworks' ProvingKey = ark_marlin::IndexProverKey BY VALUE): its ark-serialize 0.3 compressed
 * image -- index_vk, index_comm_rands, index (info, the padded matrices A, B, C, the six index polynomials with their evaluations on K), committer key (powers, shifted
 * powers, powers_of_gamma_g, degree bounds) -- streamed to `path` (0.65 GB for a 16-byte key).  A Rust caller reads it with
 * IndexProverKey::deserialize_unchecked(BufReader::new(File::open(path)?)) and can run the reference's own CPU encrypt() on a key that was synthesized on the GPU in seconds. */
int zkaes_pk_serialize_ark_to_file(const zkaes_pk *pk, const char *path, uint64_t *bytes_written);
/* the same with the point encoding chosen: uncompressed = 0 as above (48-byte points; `IndexProverKey::deserialize` takes a square root and a subgroup check per point --
 * tens of minutes for 16 M powers); uncompressed != 0: serialize_uncompressed's image (96-byte points, index_vk with 192-byte G2 elements; 1.25 GB for a 16-byte key),
 * which `IndexProverKey::deserialize_unchecked` -- ark-serialize 0.3: deserialize_unchecked defaults to the UNCOMPRESSED layout -- reads without any per-point work.
 * This is the image integration/rust_verify_harness/src/bin/encrypt_with_gpu_key.rs loads.  A failed write removes the partial file. */
int zkaes_pk_serialize_ark_to_file_ex(const zkaes_pk *pk, const char *path, int uncompressed, uint64_t *bytes_written);
/* *built = 1 when the key holds the fixed-base window tables of its SRS (they are skipped under ZKAES_KEY_NO_TABLES, or when device memory would not also hold the
 * default number of prover contexts); *table_bytes (may be NULL) = their size in device memory */
int zkaes_pk_tables_built(const zkaes_pk *pk, int *built, uint64_t *table_bytes);
/* The universal SRS behind the key.  src/lib.rs:139-141 builds ONE generate_universal_srs(866_944, 513, 4_062_064) for every circuit size; so does the library: per process,
 * device and SRS literals there is one array powers_of_g[0 ..= max_degree] (+ its 12 window-table copies), built by the first key that needs it and shared by all later
 * ones -- a key's plain and shifted powers are index ranges of it -- and released with the last key.  out = {max_degree, points per copy, copies (1 = no tables), device
 * bytes, keys sharing it now, bytes of the Lagrange-basis points (shared per |H|, |X|)}; secs (may be NULL) = {seconds THIS key's synthesis spent building the SRS
 * (~0 when it was shared), seconds of the whole synthesis}. */
int zkaes_pk_srs_info(const zkaes_pk *pk, uint64_t out[6], double secs[2]);
/* hold != 0: the library keeps every universal SRS (and Lagrange-basis SRS) it has built, or builds from now on, resident after the last key over it is freed -- for callers that
 * create and free keys in turn (one key per request size) and would otherwise rebuild 31.4 GB of window tables each time; hold == 0 releases them again (device memory goes
 * back once no key uses them).  Default: not held. */
int zkaes_srs_hold(int hold);
/* the PROCESS default of a key's prover contexts (what ZKAES_CONTEXTS sets at start-up; 0 = back to that; at most 64).  Besides being what keys without their own
 * zkaes_pk_set_contexts use, it sizes the device memory key synthesis leaves free beside the window tables: lower it BEFORE synthesizing a key whose contexts are several times
 * larger than the reference sizes' (e.g. 28 blocks per proof over a universal SRS four times the reference's literal: ~19 GB per context, 126 GB of tables). */
int zkaes_set_default_contexts(size_t n);
/* same sum through the precomputed-window layout the prover uses for the SRS (tables 2^(window offset j) P_i built on the fly here; one bucket set), on the
 * Weierstrass model with XYZZ buckets: correct for ANY curve points, both curves. */
int zkaes_msm_table(int curve_id, const uint8_t *bases, const uint8_t *scalars, size_t n, int window_bits, uint8_t *out_xy, int *out_inf);
/* BLS12-377 only -- exactly the prover's SRS path: the tables on the curve's twisted Edwards model (7-product bucket additions; the law is unified but not complete).
 * PRECONDITION: every base lies in the prime-order subgroup (as every KZG SRS point does).  A base of order 2 or 4 is refused; any other point outside the subgroup
 * may silently give a wrong sum -- use zkaes_msm / zkaes_msm_table for untrusted points. */
int zkaes_msm_table_srs(const uint8_t *bases, const uint8_t *scalars, size_t n, int window_bits, uint8_t *out_xy, int *out_inf);
/* device-resident variant for benchmarking: repeats the MSM `reps` times over device copies, returns ms per MSM of the whole pipeline and of
 * the bucket-accumulation kernel alone */
int zkaes_msm_bench(int curve_id, const uint8_t *bases, const uint8_t *scalars, size_t n, int reps, double *ms_total, double *ms_accumulate);
/* BLS12-377, synthetic device-made bases (powers of a fixed scalar times the generator) and xorshift scalars: window_bits = 0 per-window
 * signed-digit buckets on the Weierstrass model (the generic zkaes_msm path), < 0 the same buckets on the curve's twisted Edwards model (the prover's
 * lone-call SRS path), > 0 the precomputed-table path (Edwards).  out_xy (96 B, may be NULL) receives the sum: all paths must agree. */
int zkaes_msm_bench_synth(size_t n, int window_bits, int reps, double *ms_total, double *ms_accumulate, uint8_t *out_xy);
/* stream-copy probe: copies `bytes` device-to-device `reps` times with a plain 16 B/lane kernel and returns read+write GB/s -- the measured
 * HBM peak bench.py prints beside the nominal 8 TB/s (SURVEY.md 8d "measure achievable with a stream-copy kernel and report both") */
int zkaes_stream_copy_bench(size_t bytes, int reps, double *gb_per_s);
/* per-box calibration of the hot kernel's integer roof (measurement only; ~`seconds` of GPU time, 0 < seconds <= 30).  out[0] = Fq377 reduced-radix Montgomery products per
 * second of the isolated product stream at four waves per SIMD (x 378 = v_mad_u64_u32 per second: the "peak" of roofline.int_multiplier), out[1] = the shader clock it ran at
 * in MHz (s_memtime ticks per second of s_memrealtime, median over waves and launches); out[2] = bucket additions per second of k_accumulate<EdwardsLaw>'s own loop at the
 * production launch shape over an L2-resident table (the kernel with its gathers made free), out[3] = its shader clock, out[4] = its shader cycles per addition per wave
 * (three waves share a SIMD); out[5] = rounds measured.  Medians over the rounds. */
int zkaes_int_rate_bench(double seconds, double out[8]);
/* ---- Batch verification: n >= 1 proofs under ONE verifying key, each with its own public input, for the cost of two multi-scalar multiplications and
 * ONE product of two pairings instead of n.  proofs = the n proofs' bytes back to back, proof_lens their lengths; public_input_bits = n rows of n_bits bytes, one 0/1
 * byte per variable as zkaes_verify takes them (row i belongs to proof i; NULL when n_bits = 0).  accepted_each[i] (may be NULL) = 1 / 0, *n_accepted (may be NULL)
 * their sum: the answers n calls of zkaes_verify would give, except that bytes which do not parse are a rejected proof here, never an error of the call (as in the
 * chunked verifiers).
 *
 * For proof i the verifier redoes what zkaes_verify does up to its two KZG opening equations (at beta and at gamma) -- transcript, challenges, shape checks, the
 * combined commitments and values -- but keeps both as SCALARS over base points: 11 over the proof's commitments, 2 over its opening proofs W, and scalars over the
 * key's 6 index commitments, 2 shift powers, g and gamma_g.  With two 128-bit randomizers r per proof it accepts the batch iff
 *     e(-sum r W, beta h) * e(sum r (z W + C) - (sum r v) g - (sum r rv) gamma_g, h) = 1,
 * two MSMs (2n bases with 128-bit scalars; 13n + 10 bases with 253-bit scalars) and one pairing product.  The randomizers come from ChaCha20 keyed with SHA-256 over a
 * domain string, the key's ark-serialize bytes, n, and every proof's length, bytes and public-input bits: they are fixed only once the whole batch is.  A batch accept
 * implies each of the 2n equations with error about 2n / 2^128; zkaes_verify combines its two equations under upstream's FIXED test seed, which is weaker, so the two
 * can differ only on proofs crafted against that seed (which the batch rejects).
 *
 * Rejected on their own, before the batch, and contributing nothing to it: bytes that do not parse, a non-canonical field element, a point off the curve or outside
 * the prime-order subgroup, wrong degree-bound shapes; a public-input count that does not fit the key rejects every proof.  If the batch equation fails the survivors
 * are halved and each half checked again over the prepared scalars, down to single proofs: one bad proof costs at most 2 ceil(log2 n) further sub-batches whose sizes
 * halve, i.e. less than the work of two more full batches.
 *
 * zkaes_verify_batch runs everything on the host (no device needed); zkaes_verify_batch_gpu decompresses and checks the 13n points, evaluates the public inputs and
 * runs the MSMs on the GPU (transcripts and the pairing stay on the host).  It needs no proving key. */
int zkaes_verify_batch(const zkaes_vk *vk, const uint8_t *proofs, const size_t *proof_lens, size_t n, const uint8_t *public_input_bits, size_t n_bits, int *accepted_each,
                       size_t *n_accepted);
int zkaes_verify_batch_gpu(const zkaes_vk *vk, const uint8_t *proofs, const size_t *proof_lens, size_t n, const uint8_t *public_input_bits, size_t n_bits, int *accepted_each,
                           size_t *n_accepted);
/* where the calling thread's last batch call spent its time, in ms: out = {parse, decompress + subgroup checks, transcripts + scalar rows, public-input evaluation,
 * MSMs (with the upload of the bases), pairings, whole call, number of (sub-)batches checked} */
int zkaes_verify_batch_timings(double out[8]);
/* The public-input rows of a chunked job, for the batch verifier: row j (n_bits bytes, 0/1) is exactly what zkaes_verify_encryption (ECB), zkaes_verify_cbc_chunked,
 * zkaes_verify_ctr_chunked, zkaes_verify_chunked_kt and zkaes_verify_digest_chunked derive for chunk j -- the mode header (none; the chaining value entering the chunk;
 * icb + j x the chunk's blocks), the chunk's ciphertext bits LSB first per byte, the key tag's bits when key_tag != NULL (key_tag_len 16 or 32, else 0), and
 * (states[j], states[j + 1]) when states != NULL (32 (n_chunks + 1) bytes).  *n_bits (may be NULL) receives the row length; out_bits = NULL only asks for it. */
int zkaes_chunk_public_inputs(int circuit_kind, size_t n_chunks, const uint8_t *iv_or_icb, const uint8_t *ciphertext, size_t ciphertext_len, const uint8_t *key_tag, size_t key_tag_len,
                              const uint8_t *states, uint8_t *out_bits, size_t *n_bits);
/* The batch verifier's kernels, one launch per call (tests).  zkaes_g1_decompress_batch: n compressed BLS12-377 G1 points (48 bytes each, ark-serialize) ->
 * out_xy (96 bytes each: x, y as Montgomery limbs; zeros unless status is 0) and status: 0 ok (on the curve, in the prime-order subgroup), 1 the infinity encoding,
 * 2 x is not on the curve, 3 not in the subgroup, 4 malformed (both flags set, x >= q, infinity flag over a non-zero x; decided on the host).
 * zkaes_fq_sqrt_batch: n base-field elements (48 bytes, Montgomery limbs) -> a square root each and is_square = 1, or zeros and 0.
 * zkaes_public_input_eval: out[i] = x^(betas[i]) (32 bytes, Montgomery limbs) over the domain of size 2^lg_m for x = [1, row i of bits (n_bits 0/1 bytes), zeros]. */
int zkaes_g1_decompress_batch(const uint8_t *points48, size_t n, uint8_t *out_xy, uint8_t *status);
int zkaes_fq_sqrt_batch(const uint8_t *in, size_t n, uint8_t *out, uint8_t *is_square);
int zkaes_public_input_eval(int lg_m, const uint8_t *betas, const uint8_t *bits, size_t n, size_t n_bits, uint8_t *out);
/* ---- batch verification across keys.  zkaes_verify_batch over proofs of n_keys verifying keys: proof i is checked under vks[key_of[i]] against its own
 * row of n_bits_each[i] 0/1 bytes; the rows lie one behind the other in public_input_bits (NULL when they are all empty).  Still two MSMs and ONE pairing product per
 * (sub-)batch: every key this library synthesizes has the same g, gamma_g, h and beta_h (the setup draws them from one fixed stream whatever the SRS size), so the batch
 * equation of zkaes_verify_batch holds over proofs of different keys, with each key's 6 index commitments and 2 shift powers as further bases (13 n + 10 n_keys in all).
 * The answers are those of n calls of zkaes_verify, proof i under its own key.  Errors of the call, before any work: n_keys = 0, a key index >= n_keys, and keys whose
 * g, gamma_g, h or beta_h differ ("the keys do not share one setup").  A row that does not pad to its own key's |X| rejects that proof alone.  The randomizers are
 * drawn as zkaes_verify_batch draws them, seeded over a domain string of their own, every key's ark-serialize bytes, n, and every proof's key index, row length, length,
 * bytes and bits.  zkaes_verify_batch_timings reports the last call of either family.  The _gpu form runs the point checks, the public-input evaluation (one launch
 * over all keys) and the MSMs on the device. */
int zkaes_verify_batch_keys(const zkaes_vk *const *vks, size_t n_keys, const uint32_t *key_of, const uint8_t *proofs, const size_t *proof_lens, size_t n, const uint8_t *public_input_bits,
                            const size_t *n_bits_each, int *accepted_each, size_t *n_accepted);
int zkaes_verify_batch_keys_gpu(const zkaes_vk *const *vks, size_t n_keys, const uint32_t *key_of, const uint8_t *proofs, const size_t *proof_lens, size_t n, const uint8_t *public_input_bits,
                                const size_t *n_bits_each, int *accepted_each, size_t *n_accepted);
/* The public-input rows of a segmented GCM record (host only): row s is exactly what zkaes_verify_gcm_segments (mask = NULL) or zkaes_verify_gcm_segments_reveal (ONE mask
 * of mask_len bytes over the record and its ciphertext_len revealed bytes) checks segment s against.  The rows are ragged -- head, mid and tail differ -- and are written
 * one behind the other; n_bits_each[s] receives row s's length and roles[s] 0 (head), 1 (mid) or 2 (tail); both may be NULL.  out_bits = NULL only asks for the sizes.
 * The lengths and counts are checked as zkaes_verify_gcm_segments checks them, with the same messages. */
int zkaes_gcm_segment_public_inputs(size_t n_segments, size_t c, const uint8_t iv12[12], const uint8_t *aad, size_t aad_len, const uint8_t *ciphertext, size_t ciphertext_len,
                                    const uint8_t tag16[16], const uint8_t *commitments, size_t commitments_len, const uint8_t *mask, size_t mask_len, const uint8_t *revealed,
                                    uint8_t *out_bits, size_t *n_bits_each, int *roles);
/* zkaes_verify_gcm_segments (mask = NULL: plain keys; mask_len, revealed and revealed_len are then ignored) or zkaes_verify_gcm_segments_reveal (mask != NULL) through ONE
 * zkaes_verify_batch_keys call: the same argument and key-fit checks, the same errors and the same per-segment answers; head, mid and tail are keys 0, 1 and 2 (a record
 * of two segments has no mid key: its tail is key 1).  The three keys must share one setup. */
int zkaes_verify_gcm_segments_batch(const zkaes_vk *head, const zkaes_vk *mid_or_null, const zkaes_vk *tail, const uint8_t *proofs, const size_t *proof_lens, size_t n_segments, size_t c,
                                    const uint8_t iv12[12], const uint8_t *aad, size_t aad_len, const uint8_t *ciphertext, size_t ciphertext_len, const uint8_t tag16[16],
                                    const uint8_t *commitments, size_t commitments_len, const uint8_t *mask, size_t mask_len, const uint8_t *revealed, size_t revealed_len, int *accepted_each,
                                    size_t *n_accepted);
int zkaes_verify_gcm_segments_batch_gpu(const zkaes_vk *head, const zkaes_vk *mid_or_null, const zkaes_vk *tail, const uint8_t *proofs, const size_t *proof_lens, size_t n_segments, size_t c,
                                        const uint8_t iv12[12], const uint8_t *aad, size_t aad_len, const uint8_t *ciphertext, size_t ciphertext_len, const uint8_t tag16[16],
                                        const uint8_t *commitments, size_t commitments_len, const uint8_t *mask, size_t mask_len, const uint8_t *revealed, size_t revealed_len,
                                        int *accepted_each, size_t *n_accepted);
/* ---- key tags on segmented GCM records.  A HEAD segment key may be synthesized with key_tag_blocks = T in 1, 2: beside the head's statement it proves
 * tag_t = AES_K(D_t), t < T, for the constants D_t of the key tags above (zkaes_key_tag names them).  The 128 T tag bits are public input behind com_out and ahead of a
 * reveal key's mask and revealed bits; the tag slots lie behind the head's segment region in the trace and no other offset moves.  The boundary commitments carry the
 * head's key to every later segment, so a mid or tail key takes T = 0 only (T != 0 is an error that says so) and ONE tag covers the record.  T = 0 through these entries
 * is every entry above, bit for bit; reveal is 0 or 1 as in the _rv entries.  The proving and witness entries (zkaes_encrypt_gcm_segments[_reveal]_seeded_at,
 * zkaes_encrypt_gcm_segment[_reveal]_batch_seeded_at, zkaes_aes_witness_gcm_seg[_rv]) take a tagged head as they take any head: the tag's witness comes from the key, and
 * zkaes_pk_key_tag_blocks answers for segment keys.  The verifiers below take key_tag != NULL with key_tag_len = 16 or 32 (anything else is an error), append its bits to
 * the head's row ALONE, and are otherwise zkaes_gcm_segment_public_inputs, zkaes_verify_gcm_segments[_reveal] (mask = NULL: plain keys) and
 * zkaes_verify_gcm_segments_batch[_gpu].  A tag length that does not fit the head key -- a tag for an untagged head, 32 bytes for a T = 1 head, and, through the entries
 * without a tag above, a tagged head without one -- is an error of the call where the key carries its public-input count and rejects the head segment for a key from the
 * ark transport.  A session is bound to one AES key by checking every record's head, and every lone tagged GCM record, against ONE tag. */
int zkaes_synthesize_keys_gcm_seg_kt(int role, unsigned key_bits, unsigned reveal, unsigned key_tag_blocks, size_t units, size_t aad_length, size_t srs_num_constraints,
                                     size_t srs_num_variables, size_t srs_num_non_zero, unsigned flags, zkaes_pk **pk, zkaes_vk **vk);
/* host only */
int zkaes_circuit_info_gcm_seg_kt(int role, unsigned key_bits, unsigned reveal, unsigned key_tag_blocks, size_t units, size_t aad_length, uint64_t out[12]);
int zkaes_circuit_matrix_gcm_seg_kt(int role, unsigned key_bits, unsigned reveal, unsigned key_tag_blocks, size_t units, size_t aad_length, int which, uint64_t *n_rows, uint64_t *nnz,
                                    uint32_t *rowptr, uint32_t *col, int64_t *coeff);
int zkaes_gcm_segment_public_inputs_kt(size_t n_segments, size_t c, const uint8_t iv12[12], const uint8_t *aad, size_t aad_len, const uint8_t *ciphertext, size_t ciphertext_len,
                                       const uint8_t tag16[16], const uint8_t *commitments, size_t commitments_len, const uint8_t *key_tag, size_t key_tag_len, const uint8_t *mask,
                                       size_t mask_len, const uint8_t *revealed, uint8_t *out_bits, size_t *n_bits_each, int *roles);
int zkaes_verify_gcm_segments_kt(const zkaes_vk *head, const zkaes_vk *mid_or_null, const zkaes_vk *tail, const uint8_t *proofs, const size_t *proof_lens, size_t n_segments, size_t c,
                                 const uint8_t iv12[12], const uint8_t *aad, size_t aad_len, const uint8_t *ciphertext, size_t ciphertext_len, const uint8_t tag16[16],
                                 const uint8_t *commitments, size_t commitments_len, const uint8_t *key_tag, size_t key_tag_len, const uint8_t *mask, size_t mask_len,
                                 const uint8_t *revealed, size_t revealed_len, int *accepted_each, size_t *n_accepted);
int zkaes_verify_gcm_segments_batch_kt(const zkaes_vk *head, const zkaes_vk *mid_or_null, const zkaes_vk *tail, const uint8_t *proofs, const size_t *proof_lens, size_t n_segments, size_t c,
                                       const uint8_t iv12[12], const uint8_t *aad, size_t aad_len, const uint8_t *ciphertext, size_t ciphertext_len, const uint8_t tag16[16],
                                       const uint8_t *commitments, size_t commitments_len, const uint8_t *key_tag, size_t key_tag_len, const uint8_t *mask, size_t mask_len,
                                       const uint8_t *revealed, size_t revealed_len, int *accepted_each, size_t *n_accepted);
/* (device) */
int zkaes_verify_gcm_segments_batch_kt_gpu(const zkaes_vk *head, const zkaes_vk *mid_or_null, const zkaes_vk *tail, const uint8_t *proofs, const size_t *proof_lens, size_t n_segments,
                                           size_t c, const uint8_t iv12[12], const uint8_t *aad, size_t aad_len, const uint8_t *ciphertext, size_t ciphertext_len, const uint8_t tag16[16],
                                           const uint8_t *commitments, size_t commitments_len, const uint8_t *key_tag, size_t key_tag_len, const uint8_t *mask, size_t mask_len,
                                           const uint8_t *revealed, size_t revealed_len, int *accepted_each, size_t *n_accepted);
/* ---- digests on segmented GCM records.  A DIGEST record of L > 16 c bytes, c a multiple of 4, is nd = ceil(L / (16 c)) data segments and ONE closing tail:
 * nd + 1 proofs.  Roles: 0 head (units = c), 1 mid (units = c), 3 LAST (units = Lr = L - 16 c (nd - 1) bytes, 1 .. 16 c: a mid with a byte length, com_in and com_out, no
 * tag) and 2 tail with units = 0: no data block, the H and J_0 slots, ONE multiplication over Y_in ^ the length block, the tag, com_in.  A head or mid also proves the chain
 * digest H_out = C(..C(H_in, M[0:64])..) over its 16 c bytes, a last the FINAL digest over its Lr bytes with the padding 0x80, zeros and the 64 public input bits total_bits.
 * Public input, behind the role's of the plain segment entries: H_in (32), H_out (32) in SHA-256's big-endian serialisation; a last then the 8 bytes of total_bits,
 * big-endian; each byte LSB first.  The states between the proofs are public, as in a chunked digest job: segment s is proven under (states[s], states[s + 1]),
 * states[0] = H_in (NULL = the initial value) and states[nd] = the SHA-256 digest of prefix || M.  There are nd commitments, one behind every data segment.
 * A proof's header is the plain segment header (80 + A bytes), then H_in (32), then for a last be64(total_bits) and eight zero bytes; the closing tail's is the plain one.
 * Digest segment keys take neither reveal nor key_tag_blocks.  Every other segment entry refuses a digest segment key (zkaes_aes_witness_gcm_seg takes one, with its longer
 * header), these entries refuse every other key, and each refusal names the entry to use. */
int zkaes_synthesize_keys_gcm_seg_dg(int role, unsigned key_bits, size_t units, size_t aad_length, size_t srs_num_constraints, size_t srs_num_variables, size_t srs_num_non_zero,
                                     unsigned flags, zkaes_pk **pk, zkaes_vk **vk);
/* digest: 1 for a segment key of a digest record, else 0; header_bytes: a segment key's whole per-proof header (0 for every other key) */
int zkaes_pk_segment_digest(const zkaes_pk *pk, int *digest, size_t *header_bytes);
/* n proofs of ONE digest segment key under caller headers (n x header_bytes), as zkaes_encrypt_gcm_segment_batch_seeded_at; a closing tail takes messages_len = 0 */
int zkaes_encrypt_gcm_segment_digest_batch_seeded_at(size_t n, const uint8_t *messages, size_t messages_len, const uint8_t *secret_keys, size_t secret_keys_len, const uint8_t *headers,
                                                     size_t headers_len, const zkaes_pk *pk, const uint8_t *zk_seed32, uint64_t first_proof_index, uint8_t **proofs, size_t *proofs_len,
                                                     size_t *proof_lens);
/* proofs [first_segment, first_segment + count) of one record's nd + 1 (proof nd is the closing tail); mid_or_null may be NULL when nd = 2; salts: 16 nd bytes or NULL (whole
 * record only); h_in_or_null: states[0]; digest_prefix: bytes hashed ahead of the record, a multiple of 64.  Proof s draws its zero-knowledge randomness at index s, so a job
 * split over calls is byte-identical to the whole job.  Receives on request the record's ciphertext (L), tag (16), commitments (32 nd) and states (32 (nd + 1)). */
int zkaes_encrypt_gcm_segments_digest_seeded_at(const uint8_t *message, size_t message_len, const uint8_t *secret_key, const uint8_t iv12[12], const uint8_t *aad, size_t aad_len,
                                                const zkaes_pk *head, const zkaes_pk *mid_or_null, const zkaes_pk *last, const zkaes_pk *tail, const uint8_t *salts_or_null,
                                                const uint8_t *h_in_or_null, uint64_t digest_prefix, const uint8_t *zk_seed32, size_t first_segment, size_t count, uint8_t *ciphertext_or_null,
                                                uint8_t *tag_or_null, uint8_t *commitments_or_null, uint8_t *states_or_null, uint8_t **proofs, size_t *proofs_len, size_t *proof_lens);
/* host only */
int zkaes_circuit_info_gcm_seg_dg(int role, unsigned key_bits, size_t units, size_t aad_length, uint64_t out[12]);
int zkaes_circuit_matrix_gcm_seg_dg(int role, unsigned key_bits, size_t units, size_t aad_length, int which, uint64_t *n_rows, uint64_t *nnz, uint32_t *rowptr, uint32_t *col, int64_t *coeff);
/* the record helper: ys = the nd accumulators behind the data segments (zkaes_gcm_boundaries stops one short: the last is the one behind the record's last data block, ahead
 * of the length block), states = the nd + 1 states through zkaes_sha256_chain / _finish.  ys = states = NULL: only *n_data_segments */
int zkaes_gcm_digest_plan(const uint8_t *message, size_t message_len, const uint8_t *secret_key, size_t key_len, const uint8_t iv12[12], const uint8_t *aad, size_t aad_len, size_t c,
                          const uint8_t *h_in_or_null, uint64_t digest_prefix, uint8_t *ys, size_t ys_cap, uint8_t *states, size_t states_cap, size_t *n_data_segments);
/* the nd + 1 rows the verifier below checks the proofs against, ragged, as zkaes_gcm_segment_public_inputs; roles: 0 head, 1 mid, 3 last, 2 tail */
int zkaes_gcm_segment_digest_public_inputs(size_t n_proofs, size_t c, const uint8_t iv12[12], const uint8_t *aad, size_t aad_len, const uint8_t *ciphertext, size_t ciphertext_len,
                                           const uint8_t tag16[16], const uint8_t *commitments, size_t commitments_len, const uint8_t *states, size_t states_len, uint64_t digest_prefix,
                                           uint8_t *out_bits, size_t *n_bits_each, int *roles);
/* The verifier sets every ctr0 = 2 + s c, cuts the ciphertext, sets total_bits = 8 (digest_prefix + ciphertext_len), builds the length block and gives the tag to the closing
 * tail only; ONE commitments array (32 nd) and ONE states array (32 (nd + 1)).  Per-proof verdicts; a proof that does not parse is a rejected segment. */
int zkaes_verify_gcm_segments_digest(const zkaes_vk *head, const zkaes_vk *mid_or_null, const zkaes_vk *last, const zkaes_vk *tail, const uint8_t *proofs, const size_t *proof_lens,
                                     size_t n_proofs, size_t c, const uint8_t iv12[12], const uint8_t *aad, size_t aad_len, const uint8_t *ciphertext, size_t ciphertext_len,
                                     const uint8_t tag16[16], const uint8_t *commitments, size_t commitments_len, const uint8_t *states, size_t states_len, uint64_t digest_prefix,
                                     int *accepted_each, size_t *n_accepted);
/* The keyed public-input kernel, one launch per call (tests): zkaes_public_input_eval over rows of n_keys domains.  Key k has |X| = 2^lg_m[k] and rows of n_bits[k] 0/1
 * bytes; row i belongs to key key_of[i] and follows row i - 1 in bits.  out[i] = x^(betas[i]) over row i's own domain. */
int zkaes_public_input_eval_keyed(const int *lg_m, const size_t *n_bits, size_t n_keys, const uint32_t *key_of, const uint8_t *betas, const uint8_t *bits, size_t n, uint8_t *out);
/* AES witness only: fills z (padded instance + witness, one byte per variable) for a message under the key's circuit */
int zkaes_aes_witness(const zkaes_pk *pk, const uint8_t *message, size_t message_len, const uint8_t secret_key[16], uint8_t *z, size_t z_cap, size_t *z_len);

#ifdef __cplusplus
}
#endif
#endif
