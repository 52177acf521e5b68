"""MI355X-native drop-in for the proving hot path of lambdaclass/AES_zero_knowledge_proof_circuit.

Public surface (mirrors /root/reference/src/lib.rs): synthesize_keys, encrypt, verify_encryption.
Everything heavy lives in libzkaes.so (HIP kernels + C++ host, C ABI in include/zkaes.h); this package is the
ctypes binding a Python harness uses.  There is no CPU fallback: proving raises ZkAesError without a GPU.
"""
from .api import (ZkAesError, ProvingKey, VerifyingKey, synthesize_keys, encrypt, verify_encryption, lib, lib_path,  # noqa: F401
                  CIRCUIT_AES, CIRCUIT_OPS_XOR, CIRCUIT_OPS_ADD, CIRCUIT_AES_CBC,
                  cbc_ciphertext, encrypt_cbc, verify_encryption_cbc, verify_cbc_chunked,
                  CIRCUIT_AES_CTR, ctr_crypt, ctr_counter_add, encrypt_ctr, verify_encryption_ctr, verify_ctr_chunked,
                  CIRCUIT_AES_GCM, synthesize_keys_gcm, gcm_encrypt, gcm_decrypt, encrypt_gcm, verify_encryption_gcm,
                  ecb_ciphertext, circuit_info, circuit_matrix,
                  key_tag, verify_chunked_tagged, verify_encryption_gcm_tagged,
                  sha256_chain, sha256_finish, verify_digest_chunked, verify_encryption_gcm_digest,
                  verify_batch, chunk_public_inputs, verify_chunked_batch,
                  reveal_mask, reveal_bytes, verify_reveal_chunked, verify_encryption_gcm_reveal)
