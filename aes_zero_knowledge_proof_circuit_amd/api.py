"""ctypes binding of include/zkaes.h, mirroring the reference's public functions (src/lib.rs:60,116,138)."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CIRCUIT_AES, CIRCUIT_OPS_XOR, CIRCUIT_OPS_ADD = 0, 1, 2
CIRCUIT_AES_CBC = 3                # AES-128-CBC: public input = iv, ciphertext (include/zkaes.h, DESIGN.md "CBC")
CIRCUIT_AES_CTR = 4                # AES-128-CTR, any byte length >= 1: public input = icb, ciphertext (include/zkaes.h, DESIGN.md "CTR")
CIRCUIT_AES_GCM = 5                # AES-128-GCM, 96-bit iv, full tag: public input = iv, aad, ciphertext, tag (include/zkaes.h, DESIGN.md "GCM"); synthesize_keys_gcm
KEY_NO_TABLES = 1                  # zkaes_synthesize_keys_ex2 flag: no fixed-base window tables (saves 10-42 GB per key)
PARITY = "parity"                  # zk_seed=PARITY: the reference's fixed ark_std::test_rng() stream for every proof (byte-parity tests only)


class ZkAesError(RuntimeError):
    """The Err(..) side of the reference's anyhow::Result."""


def lib_path():
    return os.path.join(HERE, "libzkaes.so")


_lib = None


def lib():
    """Load libzkaes.so (must have been built: python -m aes_zero_knowledge_proof_circuit_amd.build)."""
    global _lib
    if _lib is None:
        path = lib_path()
        if not os.path.exists(path):
            raise ZkAesError("libzkaes.so is not built (run: python -m aes_zero_knowledge_proof_circuit_amd.build)")
        L = C.CDLL(path)
        L.zkaes_last_error.restype = C.c_char_p
        for name in ("zkaes_bytes_free", "zkaes_pk_free", "zkaes_vk_free"):
            getattr(L, name).restype = None
            getattr(L, name).argtypes = [C.c_void_p]
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise ZkAesError(lib().zkaes_last_error().decode())


def _take(ptr, n):
    data = C.string_at(ptr, n.value)
    lib().zkaes_bytes_free(ptr)
    return data


def _split(blob, lens, n):
    """the n proofs packed one behind the other in blob, proof i lens[i] bytes long"""
    proofs, off = [], 0
    for i in range(n):
        proofs.append(blob[off:off + lens[i]])
        off += lens[i]
    return proofs


def device_count():
    return lib().zkaes_device_count()


def set_device(ordinal):
    _check(lib().zkaes_set_device(int(ordinal)))


class VerifyingKey:
    def __init__(self, ptr):
        self._p = C.c_void_p(ptr)

    def clone(self):  # the reference passes keys by value; callers .clone() them (tests/integration_tests.rs:330)
        return VerifyingKey.from_bytes(self.to_bytes())

    def to_bytes(self):
        out, n = C.c_void_p(), C.c_size_t()
        _check(lib().zkaes_vk_serialize(self._p, C.byref(out), C.byref(n)))
        return _take(out, n)

    @staticmethod
    def from_bytes(b):
        p = C.c_void_p()
        _check(lib().zkaes_vk_deserialize(bytes(b), C.c_size_t(len(b)), C.byref(p)))
        return VerifyingKey(p.value)

    def to_ark_bytes(self):
        """ark-serialize 0.3 compressed IndexVerifierKey bytes (what the Rust side's CanonicalSerialize writes)"""
        out, n = C.c_void_p(), C.c_size_t()
        _check(lib().zkaes_vk_serialize_ark(self._p, C.byref(out), C.byref(n)))
        return _take(out, n)

    def to_ark_bytes_uncompressed(self):
        """serialize_uncompressed's image of the IndexVerifierKey (96-byte G1, 192-byte G2): what deserialize_unchecked reads"""
        out, n = C.c_void_p(), C.c_size_t()
        _check(lib().zkaes_vk_serialize_ark_uncompressed(self._p, C.byref(out), C.byref(n)))
        return _take(out, n)

    @staticmethod
    def from_ark_bytes(b):
        p = C.c_void_p()
        _check(lib().zkaes_vk_deserialize_ark(bytes(b), C.c_size_t(len(b)), C.byref(p)))
        return VerifyingKey(p.value)

    @staticmethod
    def from_trapdoor(info, index_comms, beta_mont):
        arr = (C.c_uint64 * 7)(*info)
        p = C.c_void_p()
        _check(lib().zkaes_vk_from_trapdoor(arr, bytes(index_comms), bytes(beta_mont), C.byref(p)))
        return VerifyingKey(p.value)

    def verify(self, proof, public_input_bits):
        acc = C.c_int()
        bits = bytes(public_input_bits)
        _check(lib().zkaes_verify(self._p, bytes(proof), C.c_size_t(len(proof)), bits, C.c_size_t(len(bits)), C.byref(acc)))
        return bool(acc.value)

    def verify_batch(self, proofs, public_inputs, device=True):
        """n proofs under this key, one public-input row each -> list of bools (api.verify_batch)"""
        return verify_batch(self, proofs, public_inputs, device=device)

    def __del__(self):
        try:
            if self._p:
                lib().zkaes_vk_free(self._p)
                self._p = None
        except Exception:
            pass


class ProvingKey:
    def __init__(self, ptr):
        self._handle = C.c_void_p(ptr)

    @property
    def _p(self):
        """the library's handle, for every call that takes this key: a key that was freed raises instead of handing the library a null pointer"""
        if not self._handle:
            raise ZkAesError("this proving key has been freed")
        return self._handle

    def _witness(self, fn, *args):
        """z of one of the library's witness entries: asked for its size, then filled"""
        n = C.c_size_t()
        _check(fn(self._p, *args, None, C.c_size_t(0), C.byref(n)))
        buf = C.create_string_buffer(n.value)
        _check(fn(self._p, *args, buf, n, C.byref(n)))
        return buf.raw

    def _encrypt_chunked(self, mode, message, secret_key, header, zk_seed, first_proof_index, n_chunks):
        """the chunked entry of mode "" (ECB, header None), "cbc_" or "ctr_" (header = the iv / initial counter block) -> (ciphertext or None for ECB, chunk-proofs)"""
        seed = self._seed_arg(zk_seed)
        lens = (C.c_size_t * max(n_chunks, 1))()
        ct = None if header is None else C.create_string_buffer(max(len(message), 1))
        out, n = C.c_void_p(), C.c_size_t()
        head = (bytes(message), C.c_size_t(len(message)), bytes(secret_key)) + (() if header is None else (bytes(header),)) + (self._p,)
        tail = (() if ct is None else (ct,)) + (C.byref(out), C.byref(n), lens, C.c_size_t(n_chunks))
        if zk_seed is None:
            _check(getattr(lib(), "zkaes_encrypt_%schunked" % mode)(*head, *tail))
        else:
            _check(getattr(lib(), "zkaes_encrypt_%schunked_seeded_at" % mode)(*head, seed, C.c_uint64(first_proof_index), *tail))
        return None if ct is None else ct.raw[:len(message)], _split(_take(out, n), lens, n_chunks)

    def clone(self):  # device-resident and immutable: a clone is the same handle (benches/benchmark_encrypt.rs:46 clones per call)
        return self

    def key_bytes(self):
        """the byte length of the AES key this proving key takes: 16, 24 or 32 (synthesize_keys(..., key_bits=))"""
        n = C.c_size_t()
        _check(lib().zkaes_pk_key_bytes(self._p, C.byref(n)))
        return int(n.value)

    def key_tag_blocks(self):
        """T = 0, 1 or 2: the key-tag blocks this proving key was synthesized with (synthesize_keys(..., key_tag_blocks=), or a head of synthesize_keys_gcm_segment(..., key_tag_blocks=));
        128 T public-input bits of every proof it makes are key_tag(secret_key, T): the last ones ahead of a digest's states and a reveal key's mask and revealed bytes"""
        n = C.c_size_t()
        _check(lib().zkaes_pk_key_tag_blocks(self._p, C.byref(n)))
        return int(n.value)

    def digest_info(self):
        """{"kind": None | "chain" | "final", "prefix": P, "compressions": SHA-256 compressions per proof, "offset": the digest region's offset in a trace} of this key
        (synthesize_keys(..., digest=, digest_prefix=)); zeros and None for a key without a digest"""
        out = (C.c_uint64 * 4)()
        _check(lib().zkaes_pk_digest_info(self._p, out))
        return {"kind": _DIGEST_NAMES[int(out[0])], "prefix": int(out[1]), "compressions": int(out[2]), "offset": int(out[3])}

    def _message_bytes(self, header_bits):
        """the key's plaintext length: the public input is One, header_bits bits of iv / counter, 8 bits per ciphertext byte, then 128 bits per key-tag block and, for a
        key with a digest, the 512 bits of H_in and H_out, and for a reveal key 8 ceil(L / 8) mask bits and 8 L revealed bits"""
        rv = self.reveal_info()
        if rv["reveal"]:
            return rv["message_bytes"]
        digest_bits = 512 if self.digest_info()["kind"] else 0
        return (self.info()["raw_instance"] - 1 - header_bits - 128 * self.key_tag_blocks() - digest_bits) // 8

    def reveal_info(self):
        """{"reveal": bool, "message_bytes": L, "mask_bytes": ceil(L / 8), "offset": the reveal region's offset in a trace} of this key (synthesize_keys(..., reveal=True);
        DESIGN.md 9i); False and zeros for a key without reveal"""
        out = (C.c_uint64 * 4)()
        _check(lib().zkaes_pk_reveal_info(self._p, out))
        return {"reveal": bool(out[0]), "message_bytes": int(out[1]), "mask_bytes": int(out[2]), "offset": int(out[3])}

    def witness_reveal(self, message, secret_key, mask, header=None, h_in=None):
        """z (padded instance + witness, one byte per variable) of a reveal key of any mode.  mask: bytes of ceil(L / 8), or byte indices / ranges (reveal_mask); header and
        h_in as witness_digest (h_in is read by a key with a digest only).  The last 8 ceil(L / 8) + 8 L instance bits are the mask and the revealed bytes the device computed"""
        self._need_key(secret_key)
        if h_in is not None and len(h_in) != 32:
            raise ZkAesError("h_in must be 32 bytes")
        hdr = self._digest_header_bytes(header)
        self._need_header(hdr)
        m = reveal_mask(mask, len(message))
        return self._witness(lib().zkaes_aes_witness_rv, bytes(message), C.c_size_t(len(message)), bytes(secret_key), hdr or None, None if h_in is None else bytes(h_in), m, C.c_size_t(len(m)))

    def encrypt_reveal_batch(self, messages, secret_keys, masks, headers=None, h_ins=None, zk_seed=None, first_proof_index=0):
        """n independent proofs over a reveal key of any mode -> (ciphertexts, gcm_tags, h_outs, revealed, proofs), five lists (gcm_tags holds None for every mode but GCM,
        h_outs None for a key without a digest).  masks: one per message, bytes of ceil(L / 8) or byte indices / ranges (reveal_mask); headers, h_ins, zk_seed and
        first_proof_index as encrypt_digest_batch"""
        n = len(messages)
        hb = self.header_bytes()
        if headers is None:
            headers = [b""] * n
        if not (len(secret_keys) == len(headers) == len(masks) == n) or (h_ins is not None and len(h_ins) != n):
            raise ZkAesError("one secret key, one header, one mask and one h_in per message")
        kb = self.key_bytes()
        if any(len(k) != kb for k in secret_keys) or any(len(h) != hb for h in headers):
            raise ZkAesError("secret_key must be %d bytes and every header %d bytes" % (kb, hb))
        if h_ins is not None and any(len(h) != 32 for h in h_ins):
            raise ZkAesError("h_in must be 32 bytes")
        if zk_seed is None:
            zk_seed = os.urandom(32)
        seed = self._seed_arg(zk_seed)
        mb, kbuf, hbuf = b"".join(bytes(m) for m in messages), b"".join(bytes(k) for k in secret_keys), b"".join(bytes(h) for h in headers)
        mk = b"".join(reveal_mask(masks[i], len(messages[i])) for i in range(n))
        cts, tags, outs, rev = (C.create_string_buffer(max(len(mb), 1)), C.create_string_buffer(max(16 * n, 1)), C.create_string_buffer(max(32 * n, 1)),
                                C.create_string_buffer(max(len(mb), 1)))
        lens = (C.c_size_t * max(n, 1))()
        out, total = C.c_void_p(), C.c_size_t()
        _check(lib().zkaes_encrypt_reveal_batch_seeded_at(C.c_size_t(n), mb, C.c_size_t(len(mb)), kbuf, C.c_size_t(len(kbuf)), hbuf or None, C.c_size_t(len(hbuf)),
                                                          None if h_ins is None else b"".join(bytes(h) for h in h_ins), mk, C.c_size_t(len(mk)), self._p, seed, C.c_uint64(first_proof_index),
                                                          cts, tags, outs, rev, C.byref(out), C.byref(total), lens))
        proofs = _split(_take(out, total), lens, n)
        size = len(mb) // n if n else 0
        gcm, dig = self.mode()[0] == CIRCUIT_AES_GCM, self.digest_info()["kind"] is not None
        return ([cts.raw[size * i:size * (i + 1)] for i in range(n)], [tags.raw[16 * i:16 * i + 16] if gcm else None for i in range(n)],
                [outs.raw[32 * i:32 * i + 32] if dig else None for i in range(n)], [rev.raw[size * i:size * (i + 1)] for i in range(n)], proofs)

    def encrypt_reveal_chunked(self, message, secret_key, mask, header=None, h_in=None, zk_seed=None, first_proof_index=0):
        """chunk-proofs of one ECB, CBC or CTR message over a reveal key under ONE mask over the whole message -> (ciphertext, states or None, revealed, proofs).  mask: bytes
        of ceil(len(message) / 8) or byte indices / ranges (reveal_mask); chunk j is proven under its slice of it.  states: the n + 1 SHA-256 states of a chain key, None for
        a key without a digest.  header, h_in, zk_seed and first_proof_index as encrypt_digest_chunked; a job split over calls passes each call its part of message and mask"""
        self._need_key(secret_key)
        if h_in is not None and len(h_in) != 32:
            raise ZkAesError("h_in must be 32 bytes")
        hdr = self._digest_header_bytes(header)
        self._need_header(hdr)
        if zk_seed is None:
            zk_seed = os.urandom(32)
        seed = self._seed_arg(zk_seed)
        chunk = self._message_bytes(8 * len(hdr))
        if chunk == 0 or len(message) == 0 or len(message) % chunk:
            raise ZkAesError("message length must be a non-zero multiple of the key's plaintext length (%d bytes)" % chunk)
        n_chunks = len(message) // chunk
        m = reveal_mask(mask, len(message))
        dig = self.digest_info()["kind"] is not None
        ct, states, rev = C.create_string_buffer(len(message)), C.create_string_buffer(32 * (n_chunks + 1)), C.create_string_buffer(len(message))
        lens = (C.c_size_t * n_chunks)()
        out, n = C.c_void_p(), C.c_size_t()
        _check(lib().zkaes_encrypt_reveal_chunked_seeded_at(bytes(message), C.c_size_t(len(message)), bytes(secret_key), hdr or None, None if h_in is None else bytes(h_in), m, C.c_size_t(len(m)),
                                                            self._p, seed, C.c_uint64(first_proof_index), ct, states if dig else None, rev, C.byref(out), C.byref(n), lens, C.c_size_t(n_chunks)))
        return (ct.raw[:len(message)], [states.raw[32 * j:32 * j + 32] for j in range(n_chunks + 1)] if dig else None, rev.raw[:len(message)], _split(_take(out, n), lens, n_chunks))

    def _digest_header_bytes(self, header):
        """how long the mode's public header is for this digest key, learned from the header itself: None or b"" (ECB), 16 bytes (CBC, CTR), 12 + aad (GCM); the library
        checks it against the key"""
        return b"" if header is None else bytes(header)

    def witness_digest(self, message, secret_key, header=None, h_in=None):
        """z (padded instance + witness, one byte per variable) of a digest key of any mode.  header: None for ECB, the iv (CBC) or initial counter block (CTR), iv + aad
        for GCM; h_in: 32 bytes, None = SHA-256's initial value.  The last 512 instance bits are h_in and the H_out the device computed"""
        self._need_key(secret_key)
        if h_in is not None and len(h_in) != 32:
            raise ZkAesError("h_in must be 32 bytes")
        hdr = self._digest_header_bytes(header)
        self._need_header(hdr)
        return self._witness(lib().zkaes_aes_witness_pd, bytes(message), C.c_size_t(len(message)), bytes(secret_key), hdr or None, None if h_in is None else bytes(h_in))

    def _need_header(self, hdr):
        """the mode's header has the length this key reads from the pointer: the public input is One, the header bits, the ciphertext bits (one byte per message byte,
        which the caller's message fixes), GCM's tag, the key tag, H_in and H_out -- so only 0, 16 or 12 + aad bytes can be right, and info() tells which"""
        want = self.header_bytes()
        if len(hdr) != want:
            raise ZkAesError("this key's mode takes a public header of %d bytes" % want)

    def header_bytes(self):
        """the byte length of the public header a proof of this key's mode carries: 0 (ECB), 16 (CBC, CTR), 12 + aad (GCM)"""
        return self.mode()[1]

    def mode(self):
        """(circuit kind, header bytes) of this key: CIRCUIT_AES .. CIRCUIT_AES_GCM or an ops kind, and the public header a proof of that mode carries"""
        kind, n = C.c_int(), C.c_size_t()
        _check(lib().zkaes_pk_mode(self._p, C.byref(kind), C.byref(n)))
        return int(kind.value), int(n.value)

    def encrypt_digest_batch(self, messages, secret_keys, headers=None, h_ins=None, zk_seed=None, first_proof_index=0):
        """n independent proofs over a digest key of any mode -> (ciphertexts, gcm_tags, h_outs, proofs), four lists (gcm_tags holds None for every mode but GCM).
        headers: None for ECB, else one per message (iv / initial counter block / iv + aad); h_ins: None (every proof starts from the initial value) or one 32-byte state
        per message.  zk_seed and first_proof_index as encrypt_batch (None = a fresh OS seed for the call)"""
        n = len(messages)
        hb = self.header_bytes()
        if headers is None:
            headers = [b""] * n
        if not (len(secret_keys) == len(headers) == n) or (h_ins is not None and len(h_ins) != n):
            raise ZkAesError("one secret key, one header and one h_in per message")
        kb = self.key_bytes()
        if any(len(k) != kb for k in secret_keys) or any(len(h) != hb for h in headers):
            raise ZkAesError("secret_key must be %d bytes and every header %d bytes" % (kb, hb))
        if h_ins is not None and any(len(h) != 32 for h in h_ins):
            raise ZkAesError("h_in must be 32 bytes")
        if zk_seed is None:
            zk_seed = os.urandom(32)
        seed = self._seed_arg(zk_seed)
        mb, kbuf, hbuf = b"".join(bytes(m) for m in messages), b"".join(bytes(k) for k in secret_keys), b"".join(bytes(h) for h in headers)
        cts, tags, outs = C.create_string_buffer(max(len(mb), 1)), C.create_string_buffer(max(16 * n, 1)), C.create_string_buffer(max(32 * n, 1))
        lens = (C.c_size_t * max(n, 1))()
        out, total = C.c_void_p(), C.c_size_t()
        _check(lib().zkaes_encrypt_digest_batch_seeded_at(C.c_size_t(n), mb, C.c_size_t(len(mb)), kbuf, C.c_size_t(len(kbuf)), hbuf or None, C.c_size_t(len(hbuf)),
                                                          None if h_ins is None else b"".join(bytes(h) for h in h_ins), self._p, seed, C.c_uint64(first_proof_index), cts, tags, outs,
                                                          C.byref(out), C.byref(total), lens))
        proofs = _split(_take(out, total), lens, n)
        size = len(mb) // n if n else 0
        gcm = self.mode()[0] == CIRCUIT_AES_GCM
        return ([cts.raw[size * i:size * (i + 1)] for i in range(n)], [tags.raw[16 * i:16 * i + 16] if gcm else None for i in range(n)],
                [outs.raw[32 * i:32 * i + 32] for i in range(n)], proofs)

    def encrypt_digest_chunked(self, message, secret_key, header=None, h_in=None, zk_seed=None, first_proof_index=0):
        """chunk-proofs of one ECB, CBC or CTR message over a chain key -> (ciphertext, states, proofs): states is the list of the n + 1 SHA-256 states, states[0] = h_in
        (None = the initial value), and chunk j is proven under (states[j], states[j + 1]).  header: None for ECB, the iv / initial counter block entering this call's
        first chunk otherwise.  A job split over calls passes the previous call's last state as h_in.  zk_seed and first_proof_index as encrypt_chunked"""
        self._need_key(secret_key)
        if h_in is not None and len(h_in) != 32:
            raise ZkAesError("h_in must be 32 bytes")
        hdr = self._digest_header_bytes(header)
        self._need_header(hdr)
        if zk_seed is None:
            zk_seed = os.urandom(32)
        seed = self._seed_arg(zk_seed)
        chunk = self._message_bytes(8 * len(hdr))
        if chunk == 0 or len(message) == 0 or len(message) % chunk:
            raise ZkAesError("message length must be a non-zero multiple of the key's plaintext length (%d bytes)" % chunk)
        n_chunks = len(message) // chunk
        ct, states = C.create_string_buffer(len(message)), C.create_string_buffer(32 * (n_chunks + 1))
        lens = (C.c_size_t * n_chunks)()
        out, n = C.c_void_p(), C.c_size_t()
        _check(lib().zkaes_encrypt_digest_chunked_seeded_at(bytes(message), C.c_size_t(len(message)), bytes(secret_key), hdr or None, None if h_in is None else bytes(h_in), self._p, seed,
                                                            C.c_uint64(first_proof_index), ct, states, C.byref(out), C.byref(n), lens, C.c_size_t(n_chunks)))
        return ct.raw[:len(message)], [states.raw[32 * j:32 * j + 32] for j in range(n_chunks + 1)], _split(_take(out, n), lens, n_chunks)

    def _need_key(self, secret_key, other=None, other_name=None, other_len=16):
        """the secret key has the length this proving key was synthesized for (and `other`, the iv / icb, its own): the library reads that many bytes from the pointer"""
        kb = self.key_bytes()
        if other is None:
            if len(secret_key) != kb:
                raise ZkAesError("secret_key must be %d bytes" % kb)
        elif len(secret_key) != kb or len(other) != other_len:
            if kb == other_len:
                raise ZkAesError("secret_key and %s must be %d bytes" % (other_name, kb))
            raise ZkAesError("secret_key must be %d bytes and %s %d bytes" % (kb, other_name, other_len))

    def info(self):
        out = (C.c_uint64 * 12)()
        _check(lib().zkaes_pk_info(self._p, out))
        keys = ["raw_constraints", "raw_instance", "raw_witness", "nnz_a", "nnz_b", "nnz_c", "constraints", "instance", "witness", "joint_nnz", "h", "k"]
        return dict(zip(keys, out))

    def timings(self):
        out = (C.c_double * 6)()
        _check(lib().zkaes_pk_timings(self._p, out))
        return dict(zip(["witness_ms", "round1_ms", "round2_ms", "round3_ms", "open_ms", "total_ms"], out))

    def debug_fetch(self, name):
        out, n = C.c_void_p(), C.c_size_t()
        _check(lib().zkaes_pk_debug_fetch(self._p, name.encode(), C.byref(out), C.byref(n)))
        return _take(out, n)

    def serialize_ark_to_file(self, path, uncompressed=False):
        """ark-serialize image of the arkworks IndexProverKey (index_vk, matrices, index polynomials + evaluations, committer key) streamed to `path`; returns its size.
        uncompressed=True: serialize_uncompressed's image (96-byte points) -- what IndexProverKey::deserialize_unchecked reads"""
        n = C.c_uint64()
        _check(lib().zkaes_pk_serialize_ark_to_file_ex(self._p, os.fsencode(path), 1 if uncompressed else 0, C.byref(n)))
        return int(n.value)

    def set_contexts(self, n):
        """proofs in flight per multi-proof call on this key (1..64; 0 = the process default)"""
        _check(lib().zkaes_pk_set_contexts(self._p, C.c_size_t(int(n))))

    def contexts(self):
        n = C.c_size_t()
        _check(lib().zkaes_pk_get_contexts(self._p, C.byref(n)))
        return int(n.value)

    def srs_info(self):
        """the universal SRS behind the key (one per process, device and SRS literals, shared by every key over it)"""
        out, secs = (C.c_uint64 * 6)(), (C.c_double * 2)()
        _check(lib().zkaes_pk_srs_info(self._p, out, secs))
        d = dict(zip(["max_degree", "points_per_copy", "copies", "bytes", "keys_sharing", "lagrange_bytes"], [int(v) for v in out]))
        d["srs_build_s"], d["setup_s"] = float(secs[0]), float(secs[1])
        return d

    def op_lists(self, message, secret_key, throughput_path=True):
        """the transforms and MSMs the library ACTUALLY launches for one proof on this key (zkaes_pk_op_lists): dict with "ntt" [[points, transforms per launch], ...] and
        "msm" [[points, kind], ...] + the circuit sizes.  Process-global recorder: no other proof may be in flight."""
        import json
        self._need_key(secret_key)
        out, n = C.c_void_p(), C.c_size_t()
        _check(lib().zkaes_pk_op_lists(self._p, bytes(message), C.c_size_t(len(message)), bytes(secret_key), 1 if throughput_path else 0, C.byref(out), C.byref(n)))
        return json.loads(_take(out, n).decode())

    def tables_built(self):
        """(built, bytes): does the key hold the fixed-base window tables of its SRS?"""
        b, n = C.c_int(), C.c_uint64()
        _check(lib().zkaes_pk_tables_built(self._p, C.byref(b), C.byref(n)))
        return bool(b.value), int(n.value)

    def msm_partial_dev(self, scalars_bytes, offset, dev_ptr, dev_bytes=192):
        """this rank's share of ONE MSM over the key's SRS powers [offset, offset + n) on the prover's own path (Edwards tables); the partial sum (one XYZZ point,
        192 B) stays in device memory at dev_ptr"""
        n = len(scalars_bytes) // 32
        _check(lib().zkaes_pk_msm_partial_dev(self._p, bytes(scalars_bytes), C.c_size_t(n), C.c_size_t(offset), C.c_void_p(dev_ptr), C.c_size_t(dev_bytes)))

    def witness(self, message, secret_key):
        self._need_key(secret_key)
        return self._witness(lib().zkaes_aes_witness, bytes(message), C.c_size_t(len(message)), bytes(secret_key))

    def witness_cbc(self, message, secret_key, iv):
        """z (padded instance + witness, one byte per variable) of a CBC key: One, the 128 IV bits, the ciphertext bits, padding, then the witness"""
        self._need_key(secret_key, iv, "iv")
        return self._witness(lib().zkaes_aes_witness_cbc, bytes(message), C.c_size_t(len(message)), bytes(secret_key), bytes(iv))

    def encrypt_cbc_chunked(self, message, secret_key, iv, zk_seed=None, first_proof_index=0):
        """(ciphertext, chunk-proofs) of a long CBC message.  iv = the chaining value entering this call's first chunk (a job split over several calls takes each call's
        from cbc_ciphertext); zk_seed and first_proof_index as encrypt_chunked"""
        self._need_key(secret_key, iv, "iv")
        chunk = self._message_bytes(128)
        if chunk <= 0:
            raise ZkAesError("proving key was not synthesized for the AES-CBC circuit")
        return self._encrypt_chunked("cbc_", message, secret_key, iv, zk_seed, first_proof_index, len(message) // chunk)

    def witness_ctr(self, message, secret_key, icb):
        """z (padded instance + witness, one byte per variable) of a CTR key: One, the 128 icb bits, the ciphertext bits, padding, then the witness"""
        self._need_key(secret_key, icb, "icb")
        return self._witness(lib().zkaes_aes_witness_ctr, bytes(message), C.c_size_t(len(message)), bytes(secret_key), bytes(icb))

    def encrypt_ctr_chunked(self, message, secret_key, icb, zk_seed=None, first_proof_index=0):
        """(ciphertext, chunk-proofs) of a long CTR message over a key for whole blocks; chunk j is proven under icb + j * (the key's blocks).  icb = the counter of this
        call's first block (a job split over several calls passes ctr_counter_add(icb, blocks before)); zk_seed and first_proof_index as encrypt_chunked"""
        self._need_key(secret_key, icb, "icb")
        chunk = self._message_bytes(128)
        if chunk <= 0 or len(message) == 0 or len(message) % chunk:
            raise ZkAesError("message length must be a non-zero multiple of the CTR key's plaintext length")
        return self._encrypt_chunked("ctr_", message, secret_key, icb, zk_seed, first_proof_index, len(message) // chunk)

    def witness_gcm(self, message, secret_key, iv, aad=b""):
        """z (padded instance + witness, one byte per variable) of a GCM key: One, the 96 iv bits, the aad, ciphertext and tag bits, padding, then the witness"""
        _gcm_args(secret_key, iv, self.key_bytes())
        return self._witness(lib().zkaes_aes_witness_gcm, bytes(message), C.c_size_t(len(message)), bytes(secret_key), bytes(iv), bytes(aad), C.c_size_t(len(aad)))

    def segment_info(self):
        """None for a key that is no GCM segment key, else {"role", "blocks", "message_bytes", "aad_bytes"}.  A segment key of a digest record
        (synthesize_keys_gcm_segment(..., digest=True)) also has "digest": True and "header_bytes", the length of its proofs' headers; its role may be
        "last", and its tail has 0 blocks and 0 message bytes"""
        out = (C.c_uint64 * 4)()
        _check(lib().zkaes_pk_segment_info(self._p, out))
        if not out[0]:
            return None
        info = {"role": ("head", "mid", "tail", "last")[out[0] - 1], "blocks": int(out[1]), "message_bytes": int(out[2]), "aad_bytes": int(out[3])}
        dg, hb = C.c_int(), C.c_size_t()
        _check(lib().zkaes_pk_segment_digest(self._p, C.byref(dg), C.byref(hb)))
        if dg.value:
            info["digest"], info["header_bytes"] = True, int(hb.value)
        return info

    def witness_gcm_segment(self, message, secret_key, header, mask=None):
        """z (padded instance + witness, one byte per variable) of a segment key; header = gcm_segment_header(...).  mask (a reveal segment key): the
        segment's own mask, bytes of ceil(len(message) / 8) or byte indices / ranges (reveal_mask) -- or a header made with gcm_segment_header(..., mask=), which ends in it"""
        self._need_key(secret_key)
        info = self.segment_info()
        if mask is None and info is not None and self.reveal_info()["reveal"] and len(header) > 80 + info["aad_bytes"]:
            header, mask = bytes(header)[:80 + info["aad_bytes"]], bytes(header)[80 + info["aad_bytes"]:]
        if mask is None:
            return self._witness(lib().zkaes_aes_witness_gcm_seg, bytes(message), C.c_size_t(len(message)), bytes(secret_key), bytes(header), C.c_size_t(len(header)))
        m = reveal_mask(mask, len(message))
        return self._witness(lib().zkaes_aes_witness_gcm_seg_rv, bytes(message), C.c_size_t(len(message)), bytes(secret_key), bytes(header), C.c_size_t(len(header)), m, C.c_size_t(len(m)))

    def encrypt_gcm_segment_reveal_batch(self, messages, secret_keys, headers, masks, zk_seed=None, first_proof_index=0):
        """encrypt_gcm_segment_batch over a reveal segment key -> (revealed, proofs), two lists.  masks: one per message, the segment's own mask as bytes
        of ceil(len / 8) or byte indices / ranges (reveal_mask); headers as encrypt_gcm_segment_batch (80 + A bytes each, without a mask)"""
        n = len(messages)
        if not len(secret_keys) == len(headers) == len(masks) == n:
            raise ZkAesError("one secret key, one header and one mask per message")
        if zk_seed is None:
            zk_seed = os.urandom(32)
        seed = self._seed_arg(zk_seed)
        mb, kb, hb = b"".join(bytes(m) for m in messages), b"".join(bytes(k) for k in secret_keys), b"".join(bytes(h) for h in headers)
        mk = b"".join(reveal_mask(masks[i], len(messages[i])) for i in range(n))
        rev = C.create_string_buffer(max(len(mb), 1))
        lens = (C.c_size_t * max(n, 1))()
        out, total = C.c_void_p(), C.c_size_t()
        _check(lib().zkaes_encrypt_gcm_segment_reveal_batch_seeded_at(C.c_size_t(n), mb, C.c_size_t(len(mb)), kb, C.c_size_t(len(kb)), hb, C.c_size_t(len(hb)), mk, C.c_size_t(len(mk)), self._p,
                                                                      seed, C.c_uint64(first_proof_index), rev, C.byref(out), C.byref(total), lens))
        size = len(mb) // n if n else 0
        return [rev.raw[size * i:size * (i + 1)] for i in range(n)], _split(_take(out, total), lens, n)

    def encrypt_gcm_segment_batch(self, messages, secret_keys, headers, zk_seed=None, first_proof_index=0):
        """n independent proofs over this segment key, each under its own gcm_segment_header -> the proofs; the caller answers for what the headers say
        (encrypt_gcm_segments derives them from one record).  zk_seed and first_proof_index as encrypt_batch"""
        n = len(messages)
        if not len(secret_keys) == len(headers) == n:
            raise ZkAesError("one secret key and one header per message")
        if zk_seed is None:
            zk_seed = os.urandom(32)
        seed = self._seed_arg(zk_seed)
        mb, kb, hb = b"".join(bytes(m) for m in messages), b"".join(bytes(k) for k in secret_keys), b"".join(bytes(h) for h in headers)
        lens = (C.c_size_t * max(n, 1))()
        out, total = C.c_void_p(), C.c_size_t()
        _check(lib().zkaes_encrypt_gcm_segment_batch_seeded_at(C.c_size_t(n), mb, C.c_size_t(len(mb)), kb, C.c_size_t(len(kb)), hb, C.c_size_t(len(hb)), self._p, seed,
                                                               C.c_uint64(first_proof_index), C.byref(out), C.byref(total), lens))
        return _split(_take(out, total), lens, n)

    def encrypt_gcm_segment_digest_batch(self, messages, secret_keys, headers, zk_seed=None, first_proof_index=0):
        """encrypt_gcm_segment_batch over a segment key of a digest record -> the proofs.  headers: gcm_segment_header(..., h_in=) for a head or mid,
        gcm_segment_header(..., h_in=, total_bits=) for a last, the plain header for the closing tail, whose messages are empty"""
        n = len(messages)
        if not len(secret_keys) == len(headers) == n:
            raise ZkAesError("one secret key and one header per message")
        if zk_seed is None:
            zk_seed = os.urandom(32)
        seed = self._seed_arg(zk_seed)
        mb, kb, hb = b"".join(bytes(m) for m in messages), b"".join(bytes(k) for k in secret_keys), b"".join(bytes(h) for h in headers)
        lens = (C.c_size_t * max(n, 1))()
        out, total = C.c_void_p(), C.c_size_t()
        _check(lib().zkaes_encrypt_gcm_segment_digest_batch_seeded_at(C.c_size_t(n), mb, C.c_size_t(len(mb)), kb, C.c_size_t(len(kb)), hb, C.c_size_t(len(hb)), self._p, seed,
                                                                      C.c_uint64(first_proof_index), C.byref(out), C.byref(total), lens))
        return _split(_take(out, total), lens, n)

    def encrypt_gcm_batch(self, messages, secret_keys, ivs, aads, zk_seed=None, first_proof_index=0):
        """n independent GCM records over this key -> (ciphertexts, tags, proofs), three lists.  Every message has the key's plaintext length, every aad the key's aad
        length, every iv 12 bytes; zk_seed and first_proof_index as encrypt_batch (None = a fresh OS seed for the call)"""
        n = len(messages)
        if not (len(secret_keys) == len(ivs) == len(aads) == n):
            raise ZkAesError("one secret key, one iv and one aad per message")
        kb = self.key_bytes()
        if any(len(k) != kb for k in secret_keys) or any(len(v) != 12 for v in ivs):
            raise ZkAesError("secret_key must be %d bytes and iv 12 bytes" % kb)
        if zk_seed is None:
            zk_seed = os.urandom(32)
        seed = self._seed_arg(zk_seed)
        mb, kb = b"".join(bytes(m) for m in messages), b"".join(bytes(k) for k in secret_keys)
        hb = b"".join(bytes(v) + bytes(a) for v, a in zip(ivs, aads))
        cts, tags = C.create_string_buffer(max(len(mb), 1)), C.create_string_buffer(max(16 * n, 1))
        lens = (C.c_size_t * max(n, 1))()
        out, total = C.c_void_p(), C.c_size_t()
        _check(lib().zkaes_encrypt_gcm_batch_seeded_at(C.c_size_t(n), mb, C.c_size_t(len(mb)), kb, C.c_size_t(len(kb)), hb, C.c_size_t(len(hb)), self._p, seed, C.c_uint64(first_proof_index),
                                                       cts, tags, C.byref(out), C.byref(total), lens))
        size = len(mb) // n if n else 0
        return [cts.raw[size * i:size * (i + 1)] for i in range(n)], [tags.raw[16 * i:16 * i + 16] for i in range(n)], _split(_take(out, total), lens, n)

    def prove_ops(self, x, y, zk_seed=None):
        out, n = C.c_void_p(), C.c_size_t()
        _check(lib().zkaes_prove_ops(self._p, C.c_uint32(x), C.c_uint32(y), zk_seed, C.byref(out), C.byref(n)))
        return _take(out, n)

    @staticmethod
    def _seed_arg(zk_seed):
        """None -> fresh OS seed per call (the unseeded C entry points); PARITY -> NULL seed = fixed test_rng stream; else 32 bytes"""
        if zk_seed is None or zk_seed == PARITY:
            return None
        if len(zk_seed) != 32:
            raise ZkAesError("zk_seed must be 32 bytes")
        return bytes(zk_seed)

    def encrypt_chunked(self, message, secret_key, zk_seed=None, first_proof_index=0):
        """chunk-proofs of a long ECB message.  zk_seed: None = a fresh OS seed per call, 32 bytes = caller's seed (proof i uses index first_proof_index + i),
        PARITY = the reference's fixed prover randomness for every proof"""
        self._need_key(secret_key)
        return self._encrypt_chunked("", message, secret_key, None, zk_seed, first_proof_index, len(message) // self._message_bytes(0))[1]

    def encrypt_batch(self, messages, secret_keys, zk_seed=None, first_proof_index=0):
        """n independent proofs: messages = list of equal-length byte strings (the key's plaintext length), secret_keys = list of keys of key_bytes() bytes each; zk_seed as encrypt_chunked"""
        n = len(messages)
        chunk = self._message_bytes(0)
        if len(secret_keys) != n:
            raise ZkAesError("one secret key per message")
        if any(len(m) != chunk for m in messages):
            raise ZkAesError("every message must be %d bytes (the key's plaintext length)" % chunk)
        kb = self.key_bytes()
        if any(len(k) != kb for k in secret_keys):
            raise ZkAesError("secret_key must be %d bytes" % kb)
        seed = self._seed_arg(zk_seed)
        lens = (C.c_size_t * max(n, 1))()
        out, total = C.c_void_p(), C.c_size_t()
        mb, kb = b"".join(bytes(m) for m in messages), b"".join(bytes(k) for k in secret_keys)
        if zk_seed is None:
            _check(lib().zkaes_encrypt_batch(C.c_size_t(n), mb, kb, self._p, C.byref(out), C.byref(total), lens))
        else:
            _check(lib().zkaes_encrypt_batch_seeded_at(C.c_size_t(n), mb, C.c_size_t(len(mb)), kb, C.c_size_t(len(kb)), self._p, seed, C.c_uint64(first_proof_index), C.byref(out), C.byref(total), lens))
        return _split(_take(out, total), lens, n)

    def free(self):
        """release the key now (device memory: index, prover contexts, and the universal SRS if this was its last key) instead of at garbage collection"""
        if self._handle:
            lib().zkaes_pk_free(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _tag_blocks(key_tag_blocks):
    if key_tag_blocks not in (0, 1, 2):
        raise ZkAesError("key_tag_blocks must be 0, 1 or 2")
    return C.c_uint(int(key_tag_blocks))


_DIGEST_NAMES = (None, "chain", "final")


def _digest_args(digest, digest_prefix):
    """(digest kind, digest prefix) as the C ABI takes them: digest = None, "chain" or "final" """
    if digest not in _DIGEST_NAMES:
        raise ZkAesError('digest must be None, "chain" or "final"')
    if int(digest_prefix) < 0:
        raise ZkAesError("digest_prefix must not be negative")
    return C.c_uint(_DIGEST_NAMES.index(digest)), C.c_uint64(int(digest_prefix))


def reveal_mask(mask, length):
    """a reveal mask over `length` message bytes as the C ABI takes it: ceil(length / 8) bytes, bit i = bit i % 8 of byte i / 8.  mask is those bytes already,
    or an iterable of byte indices and / or range objects to reveal.  The one conversion every reveal call goes through"""
    n = (int(length) + 7) // 8
    if isinstance(mask, (bytes, bytearray, memoryview)):
        if len(mask) != n:
            raise ZkAesError("a mask over %d bytes has %d bytes" % (length, n))
        return bytes(mask)
    out = bytearray(n)
    for item in mask:
        for i in (item if isinstance(item, range) else (item,)):
            if not 0 <= int(i) < length:
                raise ZkAesError("reveal: byte index %d is outside the message (%d bytes)" % (i, length))
            out[int(i) // 8] |= 1 << (int(i) % 8)
    return bytes(out)


def reveal_bytes(message, mask):
    """revealed[i] = message[i] where mask bit i is set, else 0 (zkaes_reveal_bytes; no GPU): what a reveal proof states beside its mask.  mask as reveal_mask takes it"""
    m = reveal_mask(mask, len(message))
    out = C.create_string_buffer(max(len(message), 1))
    _check(lib().zkaes_reveal_bytes(bytes(message), C.c_size_t(len(message)), m, C.c_size_t(len(m)), out))
    return out.raw[:len(message)]


def _synthesize(circuit, key_bits, plaintext_length, aad_length, srs, flags, key_tag_blocks=0, digest=None, digest_prefix=0, reveal=False):
    pk, vk = C.c_void_p(), C.c_void_p()
    _check(lib().zkaes_synthesize_keys_rv(int(circuit), C.c_uint(int(key_bits)), _tag_blocks(key_tag_blocks), *_digest_args(digest, digest_prefix), C.c_uint(int(bool(reveal))), C.c_size_t(plaintext_length),
                                          C.c_size_t(aad_length), C.c_size_t(srs[0]), C.c_size_t(srs[1]), C.c_size_t(srs[2]), C.c_uint(flags), C.byref(pk), C.byref(vk)))
    return ProvingKey(pk.value), VerifyingKey(vk.value)


def synthesize_keys(plaintext_length, circuit=CIRCUIT_AES, srs=(866_944, 513, 4_062_064), flags=0, key_bits=128, key_tag_blocks=0, digest=None, digest_prefix=0, reveal=False):
    """zk_aes::synthesize_keys (src/lib.rs:138-174) -> (ProvingKey, VerifyingKey).  flags: KEY_NO_TABLES.  key_bits: 128 (the reference's AES-128), 192 or 256 for
    the AES kinds; the proving key then takes secret keys of key_bits / 8 bytes (ProvingKey.key_bytes()).  key_tag_blocks: 0 (no key tag, the default), 1 or 2: every
    proof of the key also exposes key_tag(secret_key, key_tag_blocks) as public input, and is checked with verify_chunked_tagged.  digest: None (the
    default), "chain" or "final": every proof of the key also proves the SHA-256 compressions of its hidden message from a public H_in to a public H_out -- "chain" over
    the message's 64-byte blocks, "final" over the message with SHA-256's padding for digest_prefix + plaintext_length bytes -- is made through encrypt_digest_chunked /
    encrypt_digest_batch and checked with verify_digest_chunked.  reveal: False (the default) or True: every proof of the key also exposes a per-proof
    mask and the message bytes it opens, is made through encrypt_reveal_batch / encrypt_reveal_chunked and checked with verify_reveal_chunked"""
    return _synthesize(circuit, key_bits, plaintext_length, 0, srs, flags, key_tag_blocks, digest, digest_prefix, reveal)


def sha256_chain(data, h_in=None):
    """SHA-256's compression function over data's 64-byte blocks from the state h_in (32 bytes; None = the initial value), no padding (zkaes_sha256_chain; no GPU) -> 32 bytes"""
    if h_in is not None and len(h_in) != 32:
        raise ZkAesError("h_in must be 32 bytes")
    out = C.create_string_buffer(32)
    _check(lib().zkaes_sha256_chain(None if h_in is None else bytes(h_in), bytes(data), C.c_size_t(len(data)), out))
    return out.raw


def sha256_finish(h_in, prefix_bytes, tail):
    """the digest of a message whose first prefix_bytes bytes (a multiple of 64) led to the state h_in (None = the initial value) and which ends in `tail`
    (zkaes_sha256_finish; no GPU): sha256_finish(None, 0, m) == hashlib.sha256(m).digest()"""
    if h_in is not None and len(h_in) != 32:
        raise ZkAesError("h_in must be 32 bytes")
    out = C.create_string_buffer(32)
    _check(lib().zkaes_sha256_finish(None if h_in is None else bytes(h_in), C.c_uint64(int(prefix_bytes)), bytes(tail), C.c_size_t(len(tail)), out))
    return out.raw


def verify_digest_chunked(verifying_key, circuit, proofs, ciphertext, states, header=None, key_tag=None):
    """the chunk-proofs of one ECB, CBC or CTR job over a digest key against ONE array of states -> (list of bools, digest or None).  states: n + 1 states of 32 bytes;
    chunk j is checked as verify_chunked_tagged checks it (without tag bits when key_tag is None), with states[j] and states[j + 1] behind.  The digest is
    sha256_finish(states[-1], total bytes, b""): what the whole message hashes to if every chunk was accepted over a chain key from the initial value; None when a chunk
    was rejected.  One proof is the lone form (states = [h_in, h_out]); for a lone proof of a FINAL key states[-1] is already the digest and the second value returned
    is not meaningful"""
    n = len(proofs)
    if len(states) != n + 1 or any(len(st) != 32 for st in states):
        raise ZkAesError("states must be one 32-byte state more than there are proofs")
    if key_tag is not None and len(key_tag) not in (16, 32):
        raise ZkAesError("key_tag must be 16 or 32 bytes")
    if header is not None and len(header) != 16:
        raise ZkAesError("iv / icb must be 16 bytes")
    lens = (C.c_size_t * max(n, 1))(*[len(p) for p in proofs])
    each = (C.c_int * max(n, 1))()
    ok = C.c_size_t()
    _check(lib().zkaes_verify_digest_chunked(verifying_key._p, int(circuit), b"".join(bytes(p) for p in proofs), lens, C.c_size_t(n), None if header is None else bytes(header), bytes(ciphertext),
                                             C.c_size_t(len(ciphertext)), None if key_tag is None else bytes(key_tag), C.c_size_t(0 if key_tag is None else len(key_tag)),
                                             b"".join(bytes(st) for st in states), each, C.byref(ok)))
    accepted = [bool(each[i]) for i in range(n)]
    return accepted, (sha256_finish(states[-1], len(ciphertext), b"") if n and all(accepted) and len(ciphertext) % 64 == 0 else None)


def _verify_reveal_args(ciphertext, mask, revealed):
    m = reveal_mask(mask, len(ciphertext))
    if len(revealed) != len(ciphertext):
        raise ZkAesError("revealed must be as long as the ciphertext")
    return m, C.c_size_t(len(m)), bytes(revealed)


def verify_reveal_chunked(verifying_key, circuit, proofs, ciphertext, mask, revealed, header=None, key_tag=None, states=None):
    """the chunk-proofs of one ECB, CBC or CTR job over a reveal key against ONE mask and ONE array of revealed bytes over the whole job -> list of bools.  Chunk j is checked
    as verify_digest_chunked checks it (key_tag None for a key without tag blocks, states None for a key without a digest), with its slice of mask and revealed behind.  One
    proof is the lone form.  A mask bit at or beyond the length, or a non-zero revealed byte whose mask bit is 0, RAISES: it is not a rejection"""
    n = len(proofs)
    if states is not None and (len(states) != n + 1 or any(len(st) != 32 for st in states)):
        raise ZkAesError("states must be one 32-byte state more than there are proofs")
    if key_tag is not None and len(key_tag) not in (16, 32):
        raise ZkAesError("key_tag must be 16 or 32 bytes")
    if header is not None and len(header) != 16:
        raise ZkAesError("iv / icb must be 16 bytes")
    lens = (C.c_size_t * max(n, 1))(*[len(p) for p in proofs])
    each = (C.c_int * max(n, 1))()
    ok = C.c_size_t()
    _check(lib().zkaes_verify_reveal_chunked(verifying_key._p, int(circuit), b"".join(bytes(p) for p in proofs), lens, C.c_size_t(n), None if header is None else bytes(header), bytes(ciphertext),
                                             C.c_size_t(len(ciphertext)), None if key_tag is None else bytes(key_tag), C.c_size_t(0 if key_tag is None else len(key_tag)),
                                             None if states is None else b"".join(bytes(st) for st in states), *_verify_reveal_args(ciphertext, mask, revealed), each, C.byref(ok)))
    return [bool(each[i]) for i in range(n)]


def key_tag(secret_key, blocks=2):
    """the key tag on the host (zkaes_key_tag; no GPU): AES_K(D_0) (|| AES_K(D_1)), D_t = b"zkaes-keyta" + bytes([t, 0, 0, 0, 0]); 16 * blocks bytes, blocks = 1 or 2"""
    _host_key(secret_key)
    if blocks not in (1, 2):
        raise ZkAesError("a key tag has 1 or 2 blocks")
    out = C.create_string_buffer(16 * blocks)
    _check(lib().zkaes_key_tag(bytes(secret_key), C.c_size_t(len(secret_key)), C.c_size_t(blocks), out))
    return out.raw


def verify_chunked_tagged(verifying_key, circuit, proofs, ciphertext, key_tag, iv=None):
    """the chunk-proofs of one ECB, CBC or CTR job (circuit = CIRCUIT_AES, CIRCUIT_AES_CBC, CIRCUIT_AES_CTR) against ONE key tag -> list of bools.  iv: None for ECB, the
    IV for CBC, the initial counter block for CTR; chunk j is checked as verify_encryption / verify_cbc_chunked / verify_ctr_chunked check it, with the tag bits behind
    its ciphertext bits.  One proof is the lone-proof form (and the only one for a CTR length that is not whole blocks).  A key_tag that is not 16 or 32 bytes raises, as
    do lengths the key was not synthesized for"""
    if len(key_tag) not in (16, 32):
        raise ZkAesError("key_tag must be 16 or 32 bytes")
    if iv is not None and len(iv) != 16:
        raise ZkAesError("iv / icb must be 16 bytes")
    n = len(proofs)
    lens = (C.c_size_t * max(n, 1))(*[len(p) for p in proofs])
    each = (C.c_int * max(n, 1))()
    ok = C.c_size_t()
    _check(lib().zkaes_verify_chunked_kt(verifying_key._p, int(circuit), b"".join(bytes(p) for p in proofs), lens, C.c_size_t(n), None if iv is None else bytes(iv), bytes(ciphertext),
                                         C.c_size_t(len(ciphertext)), bytes(key_tag), C.c_size_t(len(key_tag)), each, C.byref(ok)))
    return [bool(each[i]) for i in range(n)]


def verify_batch(verifying_key, proofs, public_inputs, device=True):
    """n >= 1 proofs under ONE verifying key, each with its own public input (one 0/1 byte per variable, as VerifyingKey.verify takes it; all rows equally long)
    -> list of bools, the answers n calls of verify would give for the cost of two MSMs and ONE pairing product (include/zkaes.h).  Proof bytes that do
    not parse are a rejected proof, never an exception.  device=True runs the point checks, the public-input evaluation and the MSMs on the GPU (zkaes_verify_batch_gpu;
    no proving key needed); device=False everything on the host (zkaes_verify_batch; no GPU needed)"""
    n = len(proofs)
    if n == 0 or len(public_inputs) != n:
        raise ZkAesError("verify_batch takes at least one proof and one public-input row per proof")
    rows = [bytes(r) for r in public_inputs]
    n_bits = len(rows[0])
    if any(len(r) != n_bits for r in rows):
        raise ZkAesError("verify_batch: every public-input row must have the same length")
    lens = (C.c_size_t * n)(*[len(p) for p in proofs])
    each = (C.c_int * n)()
    ok = C.c_size_t()
    fn = lib().zkaes_verify_batch_gpu if device else lib().zkaes_verify_batch
    _check(fn(verifying_key._p, b"".join(bytes(p) for p in proofs), lens, C.c_size_t(n), b"".join(rows) if n_bits else None, C.c_size_t(n_bits), each, C.byref(ok)))
    return [bool(each[i]) for i in range(n)]


def verify_batch_keys(verifying_keys, key_of, proofs, public_inputs, device=True):
    """verify_batch over proofs of SEVERAL verifying keys (include/zkaes.h): proof i is checked under verifying_keys[key_of[i]] against public_inputs[i]
    (one 0/1 byte per variable; rows may differ in length) -> list of bools, the answers of n per-proof verify calls for two MSMs and ONE pairing product.  The keys
    must share one setup (every key this library synthesizes does); no key, a key index out of range or keys of different setups raise.  A row that does not fit its
    own key rejects that proof alone.  device as in verify_batch (zkaes_verify_batch_keys_gpu / zkaes_verify_batch_keys)"""
    n, nk = len(proofs), len(verifying_keys)
    if n == 0 or len(public_inputs) != n or len(key_of) != n:
        raise ZkAesError("verify_batch_keys takes at least one proof, and one key index and one public-input row per proof")
    if any(not 0 <= int(k) < 1 << 32 for k in key_of):
        raise ZkAesError("verify_batch_keys: a key index is a 32-bit unsigned number")
    rows = [bytes(r) for r in public_inputs]
    keys = (C.c_void_p * max(nk, 1))(*[vk._p.value for vk in verifying_keys])
    idx = (C.c_uint32 * n)(*[int(k) for k in key_of])
    lens = (C.c_size_t * n)(*[len(p) for p in proofs])
    row_lens = (C.c_size_t * n)(*[len(r) for r in rows])
    each = (C.c_int * n)()
    ok = C.c_size_t()
    fn = lib().zkaes_verify_batch_keys_gpu if device else lib().zkaes_verify_batch_keys
    bits = b"".join(rows)
    _check(fn(keys, C.c_size_t(nk), idx, b"".join(bytes(p) for p in proofs), lens, C.c_size_t(n), bits if bits else None, row_lens, each, C.byref(ok)))
    return [bool(each[i]) for i in range(n)]


def verify_batch_timings():
    """where this thread's last verify_batch spent its time (zkaes_verify_batch_timings): ms per stage and the number of (sub-)batches checked"""
    out = (C.c_double * 8)()
    _check(lib().zkaes_verify_batch_timings(out))
    names = ("parse_ms", "decompress_ms", "transcripts_ms", "xhat_ms", "msm_ms", "pairing_ms", "total_ms")
    d = {k: out[i] for i, k in enumerate(names)}
    d["sub_batches"] = int(out[7])
    return d


def chunk_public_inputs(circuit, ciphertext, header=None, key_tag=None, states=None, n_chunks=None, mask=None, revealed=None):
    """the public-input rows of a chunked ECB, CBC or CTR job, one bytes object of 0/1 per chunk: exactly what verify_encryption / verify_cbc_chunked / verify_ctr_chunked /
    verify_chunked_tagged / verify_digest_chunked derive for chunk j (zkaes_chunk_public_inputs; no GPU).  header: None for ECB, the IV for CBC, the initial counter block
    for CTR; key_tag: 16 or 32 bytes or None; states: the n + 1 digest states or None; n_chunks: default len(states) - 1 with states, else 1; mask and revealed: a reveal
    key's ONE mask and revealed bytes over the whole job (zkaes_chunk_public_inputs_rv), or None for both"""
    if n_chunks is None:
        n_chunks = len(states) - 1 if states is not None else 1
    if states is not None and (len(states) != n_chunks + 1 or any(len(st) != 32 for st in states)):
        raise ZkAesError("states must be one 32-byte state more than there are chunks")
    if header is not None and len(header) != 16:
        raise ZkAesError("iv / icb must be 16 bytes")
    args = (int(circuit), C.c_size_t(n_chunks), None if header is None else bytes(header), bytes(ciphertext), C.c_size_t(len(ciphertext)), None if key_tag is None else bytes(key_tag),
            C.c_size_t(0 if key_tag is None else len(key_tag)), None if states is None else b"".join(bytes(st) for st in states))
    n_bits = C.c_size_t()
    fn = lib().zkaes_chunk_public_inputs
    if (mask is None) != (revealed is None):
        raise ZkAesError("mask and revealed go together")
    if mask is not None:
        fn, args = lib().zkaes_chunk_public_inputs_rv, args + _verify_reveal_args(ciphertext, mask, revealed)
    _check(fn(*args, None, C.byref(n_bits)))
    out = C.create_string_buffer(max(1, n_chunks * n_bits.value))
    _check(fn(*args, out, C.byref(n_bits)))
    return [out.raw[j * n_bits.value:(j + 1) * n_bits.value] for j in range(n_chunks)]


def verify_chunked_batch(verifying_key, circuit, proofs, ciphertext, header=None, key_tag=None, states=None, device=True, mask=None, revealed=None):
    """the chunk-proofs of one ECB, CBC or CTR job through the batch verifier -> list of bools: chunk_public_inputs for the rows (with mask and revealed for a reveal key),
    verify_batch for the proofs"""
    return verify_batch(verifying_key, proofs, chunk_public_inputs(circuit, ciphertext, header, key_tag, states, n_chunks=len(proofs), mask=mask, revealed=revealed), device=device)


def g1_decompress_batch(points48):
    """kernel probe (zkaes_g1_decompress_batch): compressed BLS12-377 G1 points (n x 48 bytes) -> (n x 96 bytes x, y Montgomery limbs, list of status codes: 0 ok,
    1 infinity encoding, 2 not on the curve, 3 not in the prime-order subgroup, 4 malformed)"""
    n = len(points48) // 48
    out, st = C.create_string_buffer(96 * max(n, 1)), C.create_string_buffer(max(n, 1))
    _check(lib().zkaes_g1_decompress_batch(bytes(points48), C.c_size_t(n), out, st))
    return out.raw[:96 * n], list(st.raw[:n])


def fq_sqrt_batch(elements):
    """kernel probe (zkaes_fq_sqrt_batch): BLS12-377 base-field elements (n x 48 bytes, Montgomery limbs) -> (n x 48 bytes of roots, list of is_square flags)"""
    n = len(elements) // 48
    out, sq = C.create_string_buffer(48 * max(n, 1)), C.create_string_buffer(max(n, 1))
    _check(lib().zkaes_fq_sqrt_batch(bytes(elements), C.c_size_t(n), out, sq))
    return out.raw[:48 * n], list(sq.raw[:n])


def public_input_eval(lg_m, betas, bits_rows):
    """kernel probe (zkaes_public_input_eval): x^(beta_i) over the domain of size 2^lg_m for x = [1, row i (0/1 bytes), zeros]; betas n x 32 bytes Montgomery -> n x 32"""
    rows = [bytes(r) for r in bits_rows]
    n, n_bits = len(rows), len(rows[0]) if rows else 0
    out = C.create_string_buffer(32 * max(n, 1))
    _check(lib().zkaes_public_input_eval(int(lg_m), bytes(betas), b"".join(rows) if n_bits else None, C.c_size_t(n), C.c_size_t(n_bits), out))
    return out.raw[:32 * n]


def public_input_eval_keyed(keys, key_of, betas, bits_rows):
    """kernel probe (zkaes_public_input_eval_keyed): keys = [(lg_m, n_bits), ...]; row i (n_bits of its key 0/1 bytes) is evaluated at betas[i] over the domain of key
    key_of[i], all rows in ONE launch; betas n x 32 bytes Montgomery -> n x 32"""
    rows = [bytes(r) for r in bits_rows]
    n, nk = len(rows), len(keys)
    lg = (C.c_int * max(nk, 1))(*[int(k[0]) for k in keys])
    nb = (C.c_size_t * max(nk, 1))(*[int(k[1]) for k in keys])
    idx = (C.c_uint32 * max(n, 1))(*[int(k) for k in key_of])
    if any(0 <= k < nk and len(r) != keys[k][1] for r, k in zip(rows, key_of)):
        raise ZkAesError("public_input_eval_keyed: every row has its own key's n_bits bytes")
    out = C.create_string_buffer(32 * max(n, 1))
    bits = b"".join(rows)
    _check(lib().zkaes_public_input_eval_keyed(lg, nb, C.c_size_t(nk), idx, bytes(betas), bits if bits else None, C.c_size_t(n), out))
    return out.raw[:32 * n]


def _host_key(secret_key):
    if len(secret_key) not in (16, 24, 32):
        raise ZkAesError("secret_key must be 16, 24 or 32 bytes")


def ecb_ciphertext(message, secret_key):
    """AES-ECB of whole blocks on the host (zkaes_ecb_ciphertext_ks; no GPU); the key's length, 16, 24 or 32 bytes, selects AES-128, -192 or -256"""
    _host_key(secret_key)
    ct = C.create_string_buffer(max(len(message), 1))
    _check(lib().zkaes_ecb_ciphertext_ks(bytes(message), C.c_size_t(len(message)), bytes(secret_key), C.c_size_t(len(secret_key)), ct))
    return ct.raw[:len(message)]


def encrypt(message, secret_key, proving_key, zk_seed=None):
    """zk_aes::encrypt (src/lib.rs:60-114) -> serialized MarlinProof bytes."""
    proving_key._need_key(secret_key)
    out, n = C.c_void_p(), C.c_size_t()
    _check(lib().zkaes_encrypt_seeded(bytes(message), C.c_size_t(len(message)), bytes(secret_key), proving_key._p, zk_seed, C.byref(out), C.byref(n)))
    return _take(out, n)


def verify_encryption(verifying_key, proof, ciphertext):
    """zk_aes::verify_encryption (src/lib.rs:116-136) -> bool."""
    acc = C.c_int()
    _check(lib().zkaes_verify_encryption(verifying_key._p, bytes(proof), C.c_size_t(len(proof)), bytes(ciphertext), C.c_size_t(len(ciphertext)), C.byref(acc)))
    return bool(acc.value)


def cbc_ciphertext(message, secret_key, iv):
    """AES-CBC of whole blocks on the host (zkaes_cbc_ciphertext_ks; no GPU); a 16-, 24- or 32-byte key"""
    if len(secret_key) not in (16, 24, 32) or len(iv) != 16:
        raise ZkAesError("secret_key must be 16, 24 or 32 bytes and iv 16 bytes")
    ct = C.create_string_buffer(max(len(message), 1))
    _check(lib().zkaes_cbc_ciphertext_ks(bytes(message), C.c_size_t(len(message)), bytes(secret_key), C.c_size_t(len(secret_key)), bytes(iv), ct))
    return ct.raw[:len(message)]


def encrypt_cbc(message, secret_key, iv, proving_key, zk_seed=None):
    """one proof over a CBC key -> (ciphertext, serialized MarlinProof bytes); zk_seed as encrypt"""
    proving_key._need_key(secret_key, iv, "iv")
    ct = C.create_string_buffer(max(len(message), 1))
    out, n = C.c_void_p(), C.c_size_t()
    _check(lib().zkaes_encrypt_cbc_seeded(bytes(message), C.c_size_t(len(message)), bytes(secret_key), bytes(iv), proving_key._p, zk_seed, ct, C.byref(out), C.byref(n)))
    return ct.raw[:len(message)], _take(out, n)


def verify_encryption_cbc(verifying_key, proof, iv, ciphertext):
    """is `proof` a proof that `ciphertext` is the AES-128-CBC encryption under `iv` of a hidden message with a hidden key? -> bool"""
    if len(iv) != 16:
        raise ZkAesError("iv must be 16 bytes")
    acc = C.c_int()
    _check(lib().zkaes_verify_encryption_cbc(verifying_key._p, bytes(proof), C.c_size_t(len(proof)), bytes(iv), bytes(ciphertext), C.c_size_t(len(ciphertext)), C.byref(acc)))
    return bool(acc.value)


def verify_cbc_chunked(verifying_key, proofs, iv, ciphertext):
    """chunk-proofs of a long CBC message against (iv, ciphertext): chunk j is checked under the 16 ciphertext bytes ahead of it (iv for j = 0) -> list of bools"""
    if len(iv) != 16:
        raise ZkAesError("iv must be 16 bytes")
    n = len(proofs)
    lens = (C.c_size_t * max(n, 1))(*[len(p) for p in proofs])
    each = (C.c_int * max(n, 1))()
    ok = C.c_size_t()
    _check(lib().zkaes_verify_cbc_chunked(verifying_key._p, b"".join(bytes(p) for p in proofs), lens, C.c_size_t(n), bytes(iv), bytes(ciphertext), C.c_size_t(len(ciphertext)), each, C.byref(ok)))
    return [bool(each[i]) for i in range(n)]


def ctr_crypt(data, secret_key, icb):
    """AES-CTR of any byte length >= 1 on the host (zkaes_ctr_crypt_ks; no GPU): encrypts and decrypts; a 16-, 24- or 32-byte key"""
    if len(secret_key) not in (16, 24, 32) or len(icb) != 16:
        raise ZkAesError("secret_key must be 16, 24 or 32 bytes and icb 16 bytes")
    out = C.create_string_buffer(max(len(data), 1))
    _check(lib().zkaes_ctr_crypt_ks(bytes(data), C.c_size_t(len(data)), bytes(secret_key), C.c_size_t(len(secret_key)), bytes(icb), out))
    return out.raw[:len(data)]


def ctr_counter_add(icb, n_blocks):
    """icb + n_blocks mod 2^128, the 16 bytes as one big-endian integer: the counter of the block n_blocks behind icb's"""
    if len(icb) != 16 or not 0 <= n_blocks < 1 << 64:
        raise ZkAesError("icb must be 16 bytes and n_blocks a 64-bit count")
    out = C.create_string_buffer(16)
    _check(lib().zkaes_ctr_counter_add(bytes(icb), C.c_uint64(n_blocks), out))
    return out.raw


def encrypt_ctr(message, secret_key, icb, proving_key, zk_seed=None):
    """one proof over a CTR key -> (ciphertext, serialized MarlinProof bytes); zk_seed as encrypt"""
    proving_key._need_key(secret_key, icb, "icb")
    ct = C.create_string_buffer(max(len(message), 1))
    out, n = C.c_void_p(), C.c_size_t()
    _check(lib().zkaes_encrypt_ctr_seeded(bytes(message), C.c_size_t(len(message)), bytes(secret_key), bytes(icb), proving_key._p, zk_seed, ct, C.byref(out), C.byref(n)))
    return ct.raw[:len(message)], _take(out, n)


def verify_encryption_ctr(verifying_key, proof, icb, ciphertext):
    """is `proof` a proof that `ciphertext` is the AES-128-CTR encryption from counter `icb` of a hidden message with a hidden key? -> bool.  A ciphertext whose length is
    not the key's raises: the length is part of the statement"""
    if len(icb) != 16:
        raise ZkAesError("icb must be 16 bytes")
    acc = C.c_int()
    _check(lib().zkaes_verify_encryption_ctr(verifying_key._p, bytes(proof), C.c_size_t(len(proof)), bytes(icb), bytes(ciphertext), C.c_size_t(len(ciphertext)), C.byref(acc)))
    return bool(acc.value)


def verify_ctr_chunked(verifying_key, proofs, icb, ciphertext):
    """chunk-proofs of a long CTR message against (icb, ciphertext): chunk j is checked under icb + j * (blocks per chunk), from (icb, j) alone -> list of bools"""
    if len(icb) != 16:
        raise ZkAesError("icb must be 16 bytes")
    n = len(proofs)
    lens = (C.c_size_t * max(n, 1))(*[len(p) for p in proofs])
    each = (C.c_int * max(n, 1))()
    ok = C.c_size_t()
    _check(lib().zkaes_verify_ctr_chunked(verifying_key._p, b"".join(bytes(p) for p in proofs), lens, C.c_size_t(n), bytes(icb), bytes(ciphertext), C.c_size_t(len(ciphertext)), each, C.byref(ok)))
    return [bool(each[i]) for i in range(n)]


def _gcm_args(secret_key, iv, key_bytes=None):
    """key_bytes: what a proving key takes; None = the host ciphers, which take any of the three sizes"""
    if key_bytes is None:
        _host_key(secret_key)
    elif len(secret_key) != key_bytes:
        raise ZkAesError("secret_key must be %d bytes" % key_bytes)
    if len(iv) != 12:
        raise ZkAesError("GCM: only 96-bit (12-byte) IVs are supported")


def synthesize_keys_gcm(plaintext_length, aad_length=0, srs=(866_944, 513, 4_062_064), flags=0, key_bits=128, key_tag_blocks=0, digest=None, digest_prefix=0, reveal=False):
    """(ProvingKey, VerifyingKey) for AES-GCM records of exactly plaintext_length message bytes (>= 1) and aad_length aad bytes (>= 0).  flags: KEY_NO_TABLES;
    key_bits: 128, 192 or 256; key_tag_blocks: 0, 1 or 2 as synthesize_keys (records are then checked with verify_encryption_gcm_tagged); digest and digest_prefix as
    synthesize_keys (records are then made with encrypt_digest_batch and checked with verify_encryption_gcm_digest); reveal as synthesize_keys (records are then made
    with encrypt_reveal_batch and checked with verify_encryption_gcm_reveal)"""
    return _synthesize(CIRCUIT_AES_GCM, key_bits, plaintext_length, aad_length, srs, flags, key_tag_blocks, digest, digest_prefix, reveal)


def gcm_encrypt(message, secret_key, iv, aad=b""):
    """AES-GCM on the host (zkaes_gcm_encrypt_ks; no GPU), any message and aad length >= 0, a 16-, 24- or 32-byte key -> (ciphertext, tag)"""
    _gcm_args(secret_key, iv)
    ct, tag = C.create_string_buffer(max(len(message), 1)), C.create_string_buffer(16)
    _check(lib().zkaes_gcm_encrypt_ks(bytes(message), C.c_size_t(len(message)), bytes(secret_key), C.c_size_t(len(secret_key)), bytes(iv), bytes(aad), C.c_size_t(len(aad)), ct, tag))
    return ct.raw[:len(message)], tag.raw


def gcm_decrypt(ciphertext, secret_key, iv, aad, tag):
    """the plaintext, or None when the tag does not hold (zkaes_gcm_decrypt: constant-time compare, no plaintext released on failure)"""
    _gcm_args(secret_key, iv)
    if len(tag) != 16:
        raise ZkAesError("GCM: only full 16-byte tags are supported")
    msg, ok = C.create_string_buffer(max(len(ciphertext), 1)), C.c_int()
    _check(lib().zkaes_gcm_decrypt_ks(bytes(ciphertext), C.c_size_t(len(ciphertext)), bytes(secret_key), C.c_size_t(len(secret_key)), bytes(iv), bytes(aad), C.c_size_t(len(aad)), bytes(tag),
                                      msg, C.byref(ok)))
    if not ok.value:
        return None
    return msg.raw[:len(ciphertext)]


def encrypt_gcm(message, secret_key, iv, aad, proving_key, zk_seed=None):
    """one proof over a GCM key -> (ciphertext, tag, serialized MarlinProof bytes); zk_seed as encrypt"""
    _gcm_args(secret_key, iv, proving_key.key_bytes())
    ct, tag = C.create_string_buffer(max(len(message), 1)), C.create_string_buffer(16)
    out, n = C.c_void_p(), C.c_size_t()
    _check(lib().zkaes_encrypt_gcm_seeded(bytes(message), C.c_size_t(len(message)), bytes(secret_key), bytes(iv), bytes(aad), C.c_size_t(len(aad)), proving_key._p, zk_seed, ct, tag,
                                          C.byref(out), C.byref(n)))
    return ct.raw[:len(message)], tag.raw, _take(out, n)


def verify_encryption_gcm(verifying_key, proof, iv, aad, ciphertext, tag):
    """is `proof` a proof that (ciphertext, tag) is the AES-128-GCM encryption under `iv` and `aad` of a hidden message with a hidden key? -> bool.  Lengths whose sum
    is not the key's raise: they are part of the statement, and the key pins where the aad ends"""
    if len(iv) != 12:
        raise ZkAesError("GCM: only 96-bit (12-byte) IVs are supported")
    if len(tag) != 16:
        raise ZkAesError("GCM: only full 16-byte tags are supported")
    acc = C.c_int()
    _check(lib().zkaes_verify_encryption_gcm(verifying_key._p, bytes(proof), C.c_size_t(len(proof)), bytes(iv), bytes(aad), C.c_size_t(len(aad)), bytes(ciphertext),
                                             C.c_size_t(len(ciphertext)), bytes(tag), C.byref(acc)))
    return bool(acc.value)


def verify_encryption_gcm_tagged(verifying_key, proof, iv, aad, ciphertext, tag, key_tag):
    """verify_encryption_gcm for a key with key-tag blocks: the record against its own GCM tag AND the key tag (16 or 32 bytes) every record of the session shares"""
    if len(iv) != 12:
        raise ZkAesError("GCM: only 96-bit (12-byte) IVs are supported")
    if len(tag) != 16:
        raise ZkAesError("GCM: only full 16-byte tags are supported")
    if len(key_tag) not in (16, 32):
        raise ZkAesError("key_tag must be 16 or 32 bytes")
    acc = C.c_int()
    _check(lib().zkaes_verify_encryption_gcm_kt(verifying_key._p, bytes(proof), C.c_size_t(len(proof)), bytes(iv), bytes(aad), C.c_size_t(len(aad)), bytes(ciphertext),
                                                C.c_size_t(len(ciphertext)), bytes(tag), bytes(key_tag), C.c_size_t(len(key_tag)), C.byref(acc)))
    return bool(acc.value)


def verify_encryption_gcm_digest(verifying_key, proof, iv, aad, ciphertext, tag, h_out, h_in=None, key_tag=None):
    """verify_encryption_gcm for a key with a digest: the record against its GCM tag, the key tag (None for a key without tag blocks) and the SHA-256 states
    (h_in, None = the initial value; h_out) of its hidden plaintext"""
    if len(iv) != 12:
        raise ZkAesError("GCM: only 96-bit (12-byte) IVs are supported")
    if len(tag) != 16:
        raise ZkAesError("GCM: only full 16-byte tags are supported")
    if key_tag is not None and len(key_tag) not in (16, 32):
        raise ZkAesError("key_tag must be 16 or 32 bytes")
    if len(h_out) != 32 or (h_in is not None and len(h_in) != 32):
        raise ZkAesError("h_in and h_out must be 32 bytes")
    acc = C.c_int()
    _check(lib().zkaes_verify_encryption_gcm_digest(verifying_key._p, bytes(proof), C.c_size_t(len(proof)), bytes(iv), bytes(aad), C.c_size_t(len(aad)), bytes(ciphertext),
                                                    C.c_size_t(len(ciphertext)), bytes(tag), None if key_tag is None else bytes(key_tag), C.c_size_t(0 if key_tag is None else len(key_tag)),
                                                    None if h_in is None else bytes(h_in), bytes(h_out), C.byref(acc)))
    return bool(acc.value)


# ---- GCM records longer than one proof: segment-proofs over hidden commitments (include/zkaes.h)
CIRCUIT_AES_GCM_SEG = 6            # what ProvingKey.mode() reports for a segment key
SEG_HEAD, SEG_MID, SEG_TAIL = 0, 1, 2
SEG_LAST = 3                       # digest records only: the segment with the record's last data bytes, a mid with a byte length
_SEG_ROLES = {"head": SEG_HEAD, "mid": SEG_MID, "tail": SEG_TAIL, SEG_HEAD: SEG_HEAD, SEG_MID: SEG_MID, SEG_TAIL: SEG_TAIL}
_SEG_DIGEST_ROLES = dict(_SEG_ROLES, **{"last": SEG_LAST})
_SEG_DIGEST_ROLES[SEG_LAST] = SEG_LAST
# the c (data blocks per segment) of a DIGEST record over the default SRS literal (the capacity table; tests/test_gcm_segments_digest_host.py asserts it): a
# digest segment holds whole 64-byte blocks, so c is a multiple of 4, and only AES-128 fits c = 4 there; 192- and 256-bit keys take an explicit c and a larger srs=
GCM_SEGMENT_DIGEST_DEFAULT_C = {128: 4}
# the largest c (data blocks per segment) at which all three roles stay inside the default SRS literal, per key size (tests/test_gcm_segments_host.py)
GCM_SEGMENT_DEFAULT_C = {128: 4, 192: 3, 256: 2}
GCM_SEGMENT_REVEAL_DEFAULT_C = dict(GCM_SEGMENT_DEFAULT_C)      # reveal segment keys fit the same c (the capacity table; tests/test_gcm_segments_reveal_host.py asserts it)
# the same per key-tag blocks T of the head (the capacity table; tests/test_gcm_segments_keytag_host.py asserts it): one tag block fits the default c of
# every key size, with and without reveal, up to 13 bytes of aad; two tag blocks need one block less per segment
GCM_SEGMENT_KEYTAG_DEFAULT_C = {0: dict(GCM_SEGMENT_DEFAULT_C), 1: {128: 4, 192: 3, 256: 2}, 2: {128: 3, 192: 2, 256: 1}}


def verify_encryption_gcm_reveal(verifying_key, proof, iv, aad, ciphertext, tag, mask, revealed, key_tag=None, h_out=None, h_in=None):
    """verify_encryption_gcm_digest for a reveal key (h_out None for a key without a digest, key_tag None for one without tag blocks) with the record's mask and revealed
    bytes behind.  A mask bit at or beyond the length, or a non-zero revealed byte whose mask bit is 0, raises"""
    if len(iv) != 12 or len(tag) != 16:
        raise ZkAesError("iv must be 12 bytes and tag 16 bytes")
    if (h_out is not None and len(h_out) != 32) or (h_in is not None and len(h_in) != 32):
        raise ZkAesError("h_in and h_out must be 32 bytes")
    if key_tag is not None and len(key_tag) not in (16, 32):
        raise ZkAesError("key_tag must be 16 or 32 bytes")
    acc = C.c_int()
    _check(lib().zkaes_verify_encryption_gcm_reveal(verifying_key._p, bytes(proof), C.c_size_t(len(proof)), bytes(iv), bytes(aad), C.c_size_t(len(aad)), bytes(ciphertext),
                                                    C.c_size_t(len(ciphertext)), bytes(tag), None if key_tag is None else bytes(key_tag), C.c_size_t(0 if key_tag is None else len(key_tag)),
                                                    None if h_in is None else bytes(h_in), None if h_out is None else bytes(h_out), *_verify_reveal_args(ciphertext, mask, revealed),
                                                    C.byref(acc)))
    return bool(acc.value)


def _seg_role(role, digest=False):
    if digest:
        if role not in _SEG_DIGEST_ROLES:
            raise ZkAesError('role must be "head", "mid", "last" or "tail"')
        return _SEG_DIGEST_ROLES[role]
    if role not in _SEG_ROLES:
        raise ZkAesError('role must be "head", "mid" or "tail" ("last" belongs to a digest record: pass digest=True)')
    return _SEG_ROLES[role]


def _seg_digest_args(digest, reveal, key_tag_blocks):
    """digest=True with reveal or key-tag blocks is refused here as the library refuses it"""
    if digest and reveal:
        raise ZkAesError("a digest segment key has no reveal form: use a reveal segment key without a digest, or a lone GCM key with digest= and reveal=True for a record of one proof")
    if digest and _seg_key_tag_blocks(key_tag_blocks):
        raise ZkAesError("a digest segment key takes no key_tag_blocks (a tagged digest head does not fit the default SRS): use a tagged head without a digest")
    return bool(digest)


def _seg_key_tag_blocks(key_tag_blocks):
    if key_tag_blocks not in (0, 1, 2):
        raise ZkAesError("key_tag_blocks must be 0, 1 or 2")
    return int(key_tag_blocks)


def synthesize_keys_gcm_segment(role, units, aad_length=0, srs=(866_944, 513, 4_062_064), flags=0, key_bits=128, reveal=False, key_tag_blocks=0, digest=False):
    """(ProvingKey, VerifyingKey) of one segment role.  role: "head", "mid" or "tail"; units: c, the data blocks per segment, for a head or mid, and Lt, the bytes of
    the record's last segment (1 .. 16 c), for a tail; aad_length: the record's whole aad, head only.  flags and key_bits as synthesize_keys; no digest.
    reveal: False (the default) or True: every proof of the key also exposes the segment's slice of the record's mask and of its revealed bytes, is made through
    encrypt_gcm_segments(..., mask=) and checked with verify_gcm_segments(..., mask=, revealed=).
    key_tag_blocks: 0 (the default: the key as it was), 1 or 2 for a HEAD: every proof of the key also exposes key_tag(secret_key, key_tag_blocks) and is
    checked with verify_gcm_segments(..., key_tag=); the proving calls are the same.  A mid or tail with key_tag_blocks != 0 raises: the head carries the record's tag
    and the boundary commitments carry the key to every later segment.
    digest: False (the default: the key as it was) or True: a segment key of a DIGEST record, which is nd data segments and one closing tail.  role
    may then be "last", units = Lr, the bytes of the record's last data segment (1 .. 16 c); a "head" or "mid" takes c a multiple of 4 (whole 64-byte blocks) and
    also proves the SHA-256 chain over its bytes; a "tail" takes units = 0 only.  The proofs are made through encrypt_gcm_segments_digest and checked with
    verify_gcm_segments_digest against the record's states; states[-1] is hashlib.sha256(message).digest().  No reveal and no key_tag_blocks with digest=True"""
    pk, vk = C.c_void_p(), C.c_void_p()
    if _seg_digest_args(digest, reveal, key_tag_blocks):
        _check(lib().zkaes_synthesize_keys_gcm_seg_dg(_seg_role(role, True), C.c_uint(int(key_bits)), C.c_size_t(units), C.c_size_t(aad_length), C.c_size_t(srs[0]), C.c_size_t(srs[1]),
                                                      C.c_size_t(srs[2]), C.c_uint(flags), C.byref(pk), C.byref(vk)))
        return ProvingKey(pk.value), VerifyingKey(vk.value)
    if _seg_key_tag_blocks(key_tag_blocks):
        _check(lib().zkaes_synthesize_keys_gcm_seg_kt(_seg_role(role), C.c_uint(int(key_bits)), C.c_uint(int(bool(reveal))), C.c_uint(key_tag_blocks), C.c_size_t(units), C.c_size_t(aad_length),
                                                      C.c_size_t(srs[0]), C.c_size_t(srs[1]), C.c_size_t(srs[2]), C.c_uint(flags), C.byref(pk), C.byref(vk)))
        return ProvingKey(pk.value), VerifyingKey(vk.value)
    _check(lib().zkaes_synthesize_keys_gcm_seg_rv(_seg_role(role), C.c_uint(int(key_bits)), C.c_uint(int(bool(reveal))), C.c_size_t(units), C.c_size_t(aad_length), C.c_size_t(srs[0]),
                                                  C.c_size_t(srs[1]), C.c_size_t(srs[2]), C.c_uint(flags), C.byref(pk), C.byref(vk)))
    return ProvingKey(pk.value), VerifyingKey(vk.value)


def circuit_info_gcm_segment(role, units, aad_length=0, key_bits=128, reveal=False, key_tag_blocks=0, digest=False):
    out = (C.c_uint64 * 12)()
    if _seg_digest_args(digest, reveal, key_tag_blocks):
        _check(lib().zkaes_circuit_info_gcm_seg_dg(_seg_role(role, True), C.c_uint(int(key_bits)), C.c_size_t(units), C.c_size_t(aad_length), out))
    elif _seg_key_tag_blocks(key_tag_blocks):
        _check(lib().zkaes_circuit_info_gcm_seg_kt(_seg_role(role), C.c_uint(int(key_bits)), C.c_uint(int(bool(reveal))), C.c_uint(key_tag_blocks), C.c_size_t(units), C.c_size_t(aad_length), out))
    else:
        _check(lib().zkaes_circuit_info_gcm_seg_rv(_seg_role(role), C.c_uint(int(key_bits)), C.c_uint(int(bool(reveal))), C.c_size_t(units), C.c_size_t(aad_length), out))
    keys = ["raw_constraints", "raw_instance", "raw_witness", "nnz_a", "nnz_b", "nnz_c", "constraints", "instance", "witness", "joint_nnz", "h", "k"]
    return dict(zip(keys, out))


def circuit_matrix_gcm_segment(role, units, which, aad_length=0, key_bits=128, reveal=False, key_tag_blocks=0, digest=False):
    rows, nnz = C.c_uint64(), C.c_uint64()
    dg = _seg_digest_args(digest, reveal, key_tag_blocks)
    fn, head = lib().zkaes_circuit_matrix_gcm_seg_rv, (_seg_role(role, dg), C.c_uint(int(key_bits)), C.c_uint(int(bool(reveal))), C.c_size_t(units), C.c_size_t(aad_length), which)
    if dg:
        fn, head = lib().zkaes_circuit_matrix_gcm_seg_dg, head[:2] + head[3:]
    elif _seg_key_tag_blocks(key_tag_blocks):
        fn, head = lib().zkaes_circuit_matrix_gcm_seg_kt, head[:3] + (C.c_uint(key_tag_blocks),) + head[3:]
    _check(fn(*head, C.byref(rows), C.byref(nnz), None, None, None))
    rowptr = np.zeros(rows.value + 1, dtype=np.uint32)
    col = np.zeros(max(nnz.value, 1), dtype=np.uint32)
    coeff = np.zeros(max(nnz.value, 1), dtype=np.int64)
    _check(fn(*head, None, None, rowptr.ctypes.data_as(C.c_void_p), col.ctypes.data_as(C.c_void_p), coeff.ctypes.data_as(C.c_void_p)))
    return rowptr, col[:nnz.value], coeff[:nnz.value]


def gcm_segment_plan(length, aad_length=0, c=None, key_bits=128, reveal=False, key_tag_blocks=0, digest=False):
    """how a record of `length` bytes splits into segments of c data blocks (None = GCM_SEGMENT_DEFAULT_C[key_bits]) -> {"n", "c", "aad", "tail_bytes", "segments"};
    a segment is {"role", "offset", "bytes", "ctr0"}.  The keys the record needs: head (c, aad_length), mid (c) when n > 2, tail (tail_bytes).  reveal: the plan for
    reveal segment keys: the default c is GCM_SEGMENT_REVEAL_DEFAULT_C[key_bits] -- equal to the plain one, the capacity table of 9j has the room -- and
    every segment also carries "mask_offset" and "mask_bytes", its slice of the record's mask.  key_tag_blocks: the plan for a head with that many key-tag blocks
    (DESIGN.md 9l): the default c is GCM_SEGMENT_KEYTAG_DEFAULT_C[key_tag_blocks][key_bits], with and without reveal -- the plain one for one block, one less for two.
    digest=True: the plan of a DIGEST record -> {"n", "nd", "c", "aad", "last_bytes", "tail_bytes": 0, "segments"}: nd = ceil(length / (16 c)) data
    segments -- roles "head", "mid" and, for the one with the record's last "last_bytes" = 1 .. 16 c bytes, "last" -- and the closing "tail" of 0 bytes: n = nd + 1 proofs.
    The keys the record needs: head (c, aad_length), mid (c) when nd > 2, last (last_bytes), tail (0), all with digest=True.  c is a multiple of 4 and defaults to
    GCM_SEGMENT_DIGEST_DEFAULT_C[key_bits], which has 128-bit keys only: 192- and 256-bit keys must pass c, and their digest segment keys need a larger srs= than the
    default literal.  A record with length <= 16 c raises: it fits one proof of a lone GCM key with digest="final" (synthesize_keys_gcm)"""
    if digest:
        _seg_digest_args(digest, reveal, key_tag_blocks)
        if c is None:
            if key_bits not in GCM_SEGMENT_DIGEST_DEFAULT_C:
                raise ZkAesError("GCM digest segments: no default c for %d-bit keys over the default SRS: pass c (a multiple of 4) and synthesize the keys over a larger srs=" % key_bits)
            c = GCM_SEGMENT_DIGEST_DEFAULT_C[key_bits]
        if c < 1 or c % 4 or not 1 <= length <= 1 << 20 or not 0 <= aad_length <= 1 << 16:
            raise ZkAesError("GCM digest segments: a record has 1 .. 2^20 bytes, at most 65536 bytes of aad, and c is a multiple of 4 (a digest segment holds whole 64-byte blocks)")
        if length <= 16 * c:
            raise ZkAesError("GCM digest segments: this record fits one segment; a record that fits one proof goes through the lone digest key, synthesize_keys_gcm(..., digest=\"final\")")
        nd = (length + 16 * c - 1) // (16 * c)
        segs = [{"role": "head" if s == 0 else "last" if s == nd - 1 else "mid", "offset": 16 * c * s, "bytes": min(16 * c, length - 16 * c * s), "ctr0": 2 + s * c} for s in range(nd)]
        segs.append({"role": "tail", "offset": length, "bytes": 0, "ctr0": 2 + nd * c})
        return {"n": nd + 1, "nd": nd, "c": c, "aad": aad_length, "last_bytes": segs[nd - 1]["bytes"], "tail_bytes": 0, "segments": segs}
    if c is None:
        if _seg_key_tag_blocks(key_tag_blocks):
            c = GCM_SEGMENT_KEYTAG_DEFAULT_C[key_tag_blocks][key_bits]
        else:
            c = (GCM_SEGMENT_REVEAL_DEFAULT_C if reveal else GCM_SEGMENT_DEFAULT_C)[key_bits]
    if c < 1 or not 1 <= length <= 1 << 20 or not 0 <= aad_length <= 1 << 16:
        raise ZkAesError("GCM segments: a record has 1 .. 2^20 bytes, at most 65536 bytes of aad, and a segment at least one block")
    nb = (length + 15) // 16
    n = (nb + c - 1) // c
    if n < 2:
        raise ZkAesError("GCM segments: this record fits one segment; a record that fits one proof goes through synthesize_keys_gcm")
    segs = [{"role": "head" if s == 0 else "tail" if s == n - 1 else "mid", "offset": 16 * c * s, "bytes": min(16 * c, length - 16 * c * s), "ctr0": 2 + s * c} for s in range(n)]
    if reveal:
        for seg in segs:
            seg["mask_offset"], seg["mask_bytes"] = seg["offset"] // 8, (seg["bytes"] + 7) // 8
    return {"n": n, "c": c, "aad": aad_length, "tail_bytes": segs[-1]["bytes"], "segments": segs}


def gcm_boundaries(message, secret_key, iv, aad, c):
    """Y_0 .. Y_{n-2}: the record's GHASH accumulator behind the last block of every segment but the last (host only)"""
    _gcm_args(secret_key, iv)
    n = C.c_size_t()
    args = (bytes(message), C.c_size_t(len(message)), bytes(secret_key), C.c_size_t(len(secret_key)), bytes(iv), bytes(aad), C.c_size_t(len(aad)), C.c_size_t(c))
    _check(lib().zkaes_gcm_boundaries(*args, None, C.c_size_t(0), C.byref(n)))
    ys = C.create_string_buffer(max(16 * (n.value - 1), 1))
    _check(lib().zkaes_gcm_boundaries(*args, ys, C.c_size_t(16 * (n.value - 1)), C.byref(n)))
    return [ys.raw[16 * s:16 * s + 16] for s in range(n.value - 1)]


def gcm_commit(secret_key, y, salt):
    """the boundary commitment: one SHA-256 compression from the initial value over key || zeros to 32 bytes || y || salt (host only)"""
    _host_key(secret_key)
    if len(y) != 16 or len(salt) != 16:
        raise ZkAesError("y and salt must be 16 bytes")
    out = C.create_string_buffer(32)
    _check(lib().zkaes_gcm_commit(bytes(secret_key), C.c_size_t(len(secret_key)), bytes(y), bytes(salt), out))
    return out.raw


def gcm_length_block(aad_length, length):
    return (8 * aad_length).to_bytes(8, "big") + (8 * length).to_bytes(8, "big")


def gcm_segment_header(iv, ctr0, y_in=None, salt_in=None, salt_out=None, length_block=None, aad=b"", mask=None, h_in=None, total_bits=None):
    """the 80 + A bytes a segment witness takes: iv, ctr0, Y_in, salt_in, salt_out, the length block, the aad; a field the role does not use may stay None.  mask (a
    reveal segment key): the segment's own mask as bytes of ceil(len / 8), appended last: the 80 + A + ceil(len / 8) bytes of a reveal segment proof's header.
    h_in (a digest segment key): the 32-byte state entering the segment, behind the aad; total_bits (a last): 8 x the bytes hashed up to the record's end,
    appended as be64 and eight zero bytes.  The closing tail of a digest record takes neither"""
    if (h_in is not None and len(h_in) != 32) or (total_bits is not None and (h_in is None or not 0 <= int(total_bits) < 1 << 64)):
        raise ZkAesError("h_in is 32 bytes, and total_bits (below 2^64) goes with h_in")
    if h_in is not None and mask is not None:
        raise ZkAesError("a digest segment key has no reveal form: h_in and mask do not go together")
    if len(iv) != 12:
        raise ZkAesError("GCM: only 96-bit (12-byte) IVs are supported")
    parts = [bytes(iv), int(ctr0).to_bytes(4, "big")]
    for field in (y_in, salt_in, salt_out, length_block):
        field = bytes(16) if field is None else bytes(field)
        if len(field) != 16:
            raise ZkAesError("Y_in, the salts and the length block are 16 bytes each")
        parts.append(field)
    dg = b"" if h_in is None else bytes(h_in) + (b"" if total_bits is None else int(total_bits).to_bytes(8, "big") + bytes(8))
    return b"".join(parts) + bytes(aad) + dg + (b"" if mask is None else bytes(mask))


def encrypt_gcm_segments(message, secret_key, iv, aad, keys, salts=None, first_segment=0, count=None, zk_seed=None, mask=None):
    """segments [first_segment, first_segment + count) of one record as segment-proofs -> (ciphertext, tag, commitments, proofs): the WHOLE record's ciphertext and tag,
    its n - 1 commitments (32 bytes each) and the call's proofs.  keys = (head, mid or None, tail) proving keys; count None = to the record's end; salts = n - 1 strings
    of 16 bytes or None for os.urandom (a job split over calls passes them: every call must make the same commitments); zk_seed as encrypt_batch, segment s drawing at
    index s whichever call proves it.  mask (three reveal segment keys): ONE mask over the whole record, bytes of ceil(len(message) / 8) or byte indices /
    ranges (reveal_mask); the call then returns (ciphertext, tag, commitments, revealed, proofs), revealed = reveal_bytes(message, mask) for the whole record"""
    head, mid, tail = keys
    _gcm_args(secret_key, iv, head.key_bytes())
    info = head.segment_info()
    if info is None:
        raise ZkAesError("the head key is not a GCM segment key: the segment entry points take keys of synthesize_keys_gcm_segment (a lone record goes through encrypt_gcm, zkaes_encrypt_gcm_seeded)")
    c = info["blocks"]
    n = gcm_segment_plan(len(message), len(aad), c)["n"]
    if count is None:
        count = n - first_segment
    if salts is None:
        salts = [os.urandom(16) for _ in range(n - 1)]
    if len(salts) != n - 1 or any(len(s) != 16 for s in salts):
        raise ZkAesError("salts: one 16-byte salt per boundary, %d for this record" % (n - 1))
    if zk_seed is None:
        zk_seed = os.urandom(32)
    seed = ProvingKey._seed_arg(zk_seed)
    ct, tag, coms = C.create_string_buffer(len(message)), C.create_string_buffer(16), C.create_string_buffer(32 * (n - 1))
    lens = (C.c_size_t * max(count, 1))()
    out, total = C.c_void_p(), C.c_size_t()
    if mask is not None:
        m, rev = reveal_mask(mask, len(message)), C.create_string_buffer(len(message))
        _check(lib().zkaes_encrypt_gcm_segments_reveal_seeded_at(bytes(message), C.c_size_t(len(message)), bytes(secret_key), bytes(iv), bytes(aad), C.c_size_t(len(aad)), head._p,
                                                                 None if mid is None else mid._p, tail._p, b"".join(bytes(s) for s in salts), m, C.c_size_t(len(m)), seed, C.c_size_t(first_segment),
                                                                 C.c_size_t(count), ct, tag, coms, rev, C.byref(out), C.byref(total), lens))
        return ct.raw[:len(message)], tag.raw, [coms.raw[32 * s:32 * s + 32] for s in range(n - 1)], rev.raw[:len(message)], _split(_take(out, total), lens, count)
    _check(lib().zkaes_encrypt_gcm_segments_seeded_at(bytes(message), C.c_size_t(len(message)), bytes(secret_key), bytes(iv), bytes(aad), C.c_size_t(len(aad)), head._p,
                                                      None if mid is None else mid._p, tail._p, b"".join(bytes(s) for s in salts), seed, C.c_size_t(first_segment), C.c_size_t(count), ct, tag,
                                                      coms, C.byref(out), C.byref(total), lens))
    return ct.raw[:len(message)], tag.raw, [coms.raw[32 * s:32 * s + 32] for s in range(n - 1)], _split(_take(out, total), lens, count)


def gcm_digest_plan(message, secret_key, iv, aad, c, h_in=None, digest_prefix=0):
    """(ys, states) of a DIGEST record (host only): the nd GHASH accumulators behind its data segments -- gcm_boundaries stops one short; the last one here is
    the accumulator behind the record's last data block, ahead of the length block, which enters the closing tail -- and the nd + 1 SHA-256 states, states[0] = h_in
    (None = the initial value), states[nd] = the digest of (digest_prefix bytes hashed into h_in) || message: hashlib.sha256(message).digest() with the defaults"""
    _gcm_args(secret_key, iv)
    if h_in is not None and len(h_in) != 32:
        raise ZkAesError("h_in must be 32 bytes")
    nd = C.c_size_t()
    args = (bytes(message), C.c_size_t(len(message)), bytes(secret_key), C.c_size_t(len(secret_key)), bytes(iv), bytes(aad), C.c_size_t(len(aad)), C.c_size_t(c),
            None if h_in is None else bytes(h_in), C.c_uint64(digest_prefix))
    _check(lib().zkaes_gcm_digest_plan(*args, None, C.c_size_t(0), None, C.c_size_t(0), C.byref(nd)))
    ys, st = C.create_string_buffer(16 * nd.value), C.create_string_buffer(32 * (nd.value + 1))
    _check(lib().zkaes_gcm_digest_plan(*args, ys, C.c_size_t(len(ys)), st, C.c_size_t(len(st)), C.byref(nd)))
    return [ys.raw[16 * s:16 * s + 16] for s in range(nd.value)], [st.raw[32 * s:32 * s + 32] for s in range(nd.value + 1)]


def encrypt_gcm_segments_digest(message, secret_key, iv, aad, keys, salts=None, first_segment=0, count=None, zk_seed=None, h_in=None, digest_prefix=0):
    """proofs [first_segment, first_segment + count) of one DIGEST record -> (ciphertext, tag, commitments, states, proofs): the WHOLE record's ciphertext
    and tag, its nd commitments (one behind every data segment), its nd + 1 states and the call's proofs, of the record's nd + 1 (the last is the closing tail).
    keys = (head, mid or None, last, tail) proving keys of synthesize_keys_gcm_segment(..., digest=True); count None = to the record's end; salts = nd strings of 16
    bytes or None for os.urandom (a job split over calls passes them); zk_seed as encrypt_batch, proof s drawing at index s whichever call makes it, so a split job is
    byte-identical to the whole one.  h_in: states[0], None = SHA-256's initial value; digest_prefix: the bytes hashed into h_in ahead of the record, a multiple of 64.
    states[-1] is the SHA-256 digest of prefix || message: hashlib.sha256(message).digest() with the defaults"""
    head, mid, last, tail = keys
    _gcm_args(secret_key, iv, head.key_bytes())
    info = head.segment_info()
    if info is None:
        raise ZkAesError("the head key is not a GCM segment key: the segment _digest_ entry points take keys of synthesize_keys_gcm_segment(..., digest=True)")
    if h_in is not None and len(h_in) != 32:
        raise ZkAesError("h_in must be 32 bytes")
    c = info["blocks"]
    if not info.get("digest"):
        raise ZkAesError("the head key is a plain segment key: encrypt_gcm_segments_digest takes keys of synthesize_keys_gcm_segment(..., digest=True) (this one goes through encrypt_gcm_segments)")
    plan = gcm_segment_plan(len(message), len(aad), c, digest=True)
    n, nd = plan["n"], plan["nd"]
    if count is None:
        count = n - first_segment
    if salts is None:
        salts = [os.urandom(16) for _ in range(nd)]
    if len(salts) != nd or any(len(x) != 16 for x in salts):
        raise ZkAesError("salts: one 16-byte salt behind every data segment, %d for this record" % nd)
    if zk_seed is None:
        zk_seed = os.urandom(32)
    seed = ProvingKey._seed_arg(zk_seed)
    ct, tag, coms, st = C.create_string_buffer(len(message)), C.create_string_buffer(16), C.create_string_buffer(32 * nd), C.create_string_buffer(32 * (nd + 1))
    lens = (C.c_size_t * max(count, 1))()
    out, total = C.c_void_p(), C.c_size_t()
    _check(lib().zkaes_encrypt_gcm_segments_digest_seeded_at(bytes(message), C.c_size_t(len(message)), bytes(secret_key), bytes(iv), bytes(aad), C.c_size_t(len(aad)), head._p,
                                                             None if mid is None else mid._p, last._p, tail._p, b"".join(bytes(x) for x in salts), None if h_in is None else bytes(h_in),
                                                             C.c_uint64(digest_prefix), seed, C.c_size_t(first_segment), C.c_size_t(count), ct, tag, coms, st, C.byref(out), C.byref(total), lens))
    return (ct.raw[:len(message)], tag.raw, [coms.raw[32 * s:32 * s + 32] for s in range(nd)], [st.raw[32 * s:32 * s + 32] for s in range(nd + 1)],
            _split(_take(out, total), lens, count))


def _gcm_digest_args(iv, tag, commitments, states):
    if len(iv) != 12:
        raise ZkAesError("GCM: only 96-bit (12-byte) IVs are supported")
    if len(tag) != 16:
        raise ZkAesError("GCM: only full 16-byte tags are supported")
    if any(len(x) != 32 for x in commitments) or any(len(x) != 32 for x in states):
        raise ZkAesError("a commitment and a state are 32 bytes each")
    return b"".join(bytes(x) for x in commitments), b"".join(bytes(x) for x in states)


def verify_gcm_segments_digest(vks, proofs, iv, aad, ciphertext, tag, commitments, c, states, digest_prefix=0):
    """the nd + 1 proofs of one DIGEST record against ONE list of nd commitments and ONE list of nd + 1 states -> a list of nd + 1 bools.  vks = (head,
    mid or None, last, tail) verifying keys; c = the data blocks per segment.  The verifier sets every ctr0 = 2 + s c, cuts the ciphertext, sets total_bits =
    8 (digest_prefix + len(ciphertext)), builds the length block from the lengths it sees and hands the tag to the closing tail alone; data segment s is checked under
    (states[s], states[s + 1]).  Accepted throughout, the record's plaintext has the SHA-256 digest states[-1] when hashed from states[0] behind digest_prefix bytes:
    the caller compares states[0] with the state it started from (sha256_chain(b"") is the initial value) and states[-1] with the digest it expects.  Lengths that do
    not fit the keys, the proof count, the commitment count or the state count raise; a proof that does not parse is a rejected segment"""
    coms, st = _gcm_digest_args(iv, tag, commitments, states)
    head, mid, last, tail = vks
    n = len(proofs)
    lens = (C.c_size_t * max(n, 1))(*[len(p) for p in proofs])
    each, ok = (C.c_int * max(n, 1))(), C.c_size_t()
    _check(lib().zkaes_verify_gcm_segments_digest(head._p, None if mid is None else mid._p, last._p, tail._p, b"".join(bytes(p) for p in proofs), lens, C.c_size_t(n), C.c_size_t(c), bytes(iv),
                                                  bytes(aad), C.c_size_t(len(aad)), bytes(ciphertext), C.c_size_t(len(ciphertext)), bytes(tag), coms, C.c_size_t(len(coms)), st,
                                                  C.c_size_t(len(st)), C.c_uint64(digest_prefix), each, C.byref(ok)))
    return [bool(each[i]) for i in range(n)]


def gcm_segment_digest_public_inputs(n_proofs, iv, aad, ciphertext, tag, commitments, c, states, digest_prefix=0):
    """the public-input rows of a DIGEST record -> (key_of, rows): per proof the index of its key in (head, mid, last, tail) -- 0, 1, 2 or 3 -- and one bytes object of
    0/1, exactly what verify_gcm_segments_digest checks it against (zkaes_gcm_segment_digest_public_inputs; no GPU).  With them the record's nd + 1 proofs go through
    verify_batch_keys([head, mid, last, tail], key_of, proofs, rows) in one pairing check; a record without a mid (nd = 2) passes its three keys and
    [k if k == 0 else k - 1 for k in key_of]"""
    coms, st = _gcm_digest_args(iv, tag, commitments, states)
    n = int(n_proofs)
    lens, roles = (C.c_size_t * max(n, 1))(), (C.c_int * max(n, 1))()
    args = (C.c_size_t(n), C.c_size_t(c), bytes(iv), bytes(aad), C.c_size_t(len(aad)), bytes(ciphertext), C.c_size_t(len(ciphertext)), bytes(tag), coms, C.c_size_t(len(coms)), st,
            C.c_size_t(len(st)), C.c_uint64(digest_prefix))
    _check(lib().zkaes_gcm_segment_digest_public_inputs(*args, None, lens, roles))
    out = C.create_string_buffer(max(1, sum(lens[s] for s in range(n))))
    _check(lib().zkaes_gcm_segment_digest_public_inputs(*args, out, lens, roles))
    rows, off = [], 0
    for s in range(n):
        rows.append(out.raw[off:off + lens[s]])
        off += lens[s]
    return [{SEG_HEAD: 0, SEG_MID: 1, SEG_LAST: 2, SEG_TAIL: 3}[roles[s]] for s in range(n)], rows


def _seg_key_tag(key_tag):
    if key_tag is not None and len(key_tag) not in (16, 32):
        raise ZkAesError("key_tag must be 16 or 32 bytes")
    return None if key_tag is None else bytes(key_tag)


def verify_gcm_segments(vks, proofs, iv, aad, ciphertext, tag, commitments, c, mask=None, revealed=None, key_tag=None):
    """the n segment-proofs of one record against ONE list of n - 1 commitments -> a list of n bools.  vks = (head, mid or None, tail) verifying keys; c = the data
    blocks per segment.  The verifier sets every segment's ctr0 = 2 + s c, cuts the ciphertext, builds the length block from the lengths it sees and hands the tag to
    the tail alone; lengths that do not fit the keys, the proof count or the commitment count raise.  mask and revealed (proofs of reveal segment keys):
    ONE mask over the record (reveal_mask) and its len(ciphertext) revealed bytes, both or neither; a mask bit at or beyond the length, or a non-zero revealed byte whose
    mask bit is 0, raises.  key_tag (a head synthesized with key_tag_blocks = 1 or 2): the 16 or 32 bytes every record of the session is checked
    against, key_tag(secret_key, blocks) for an honest prover; its bits enter the head's row alone.  The cross cases are 9e's: a tagged head without key_tag, an
    untagged head with one, or a key_tag of the other length RAISES for a head key of this process or of serialize_vk / deserialize_vk (it carries its public-input
    count) and REJECTS the head segment for a key from the ark transport; a key_tag that is not 16 or 32 bytes always raises"""
    if len(iv) != 12:
        raise ZkAesError("GCM: only 96-bit (12-byte) IVs are supported")
    if len(tag) != 16:
        raise ZkAesError("GCM: only full 16-byte tags are supported")
    if any(len(x) != 32 for x in commitments):
        raise ZkAesError("a commitment is 32 bytes")
    head, mid, tail = vks
    n = len(proofs)
    lens = (C.c_size_t * max(n, 1))(*[len(p) for p in proofs])
    each, ok = (C.c_int * max(n, 1))(), C.c_size_t()
    coms = b"".join(bytes(x) for x in commitments)
    if (mask is None) != (revealed is None):
        raise ZkAesError("verify_gcm_segments: mask and revealed go together")
    kt = _seg_key_tag(key_tag)
    if kt is not None:
        m = None if mask is None else reveal_mask(mask, len(ciphertext))
        _check(lib().zkaes_verify_gcm_segments_kt(head._p, None if mid is None else mid._p, tail._p, b"".join(bytes(p) for p in proofs), lens, C.c_size_t(n), C.c_size_t(c), bytes(iv), bytes(aad),
                                                  C.c_size_t(len(aad)), bytes(ciphertext), C.c_size_t(len(ciphertext)), bytes(tag), coms, C.c_size_t(len(coms)), kt, C.c_size_t(len(kt)), m,
                                                  C.c_size_t(0 if m is None else len(m)), None if m is None else bytes(revealed), C.c_size_t(0 if m is None else len(revealed)), each,
                                                  C.byref(ok)))
        return [bool(each[i]) for i in range(n)]
    if mask is not None:
        m = reveal_mask(mask, len(ciphertext))
        _check(lib().zkaes_verify_gcm_segments_reveal(head._p, None if mid is None else mid._p, tail._p, b"".join(bytes(p) for p in proofs), lens, C.c_size_t(n), C.c_size_t(c), bytes(iv),
                                                      bytes(aad), C.c_size_t(len(aad)), bytes(ciphertext), C.c_size_t(len(ciphertext)), bytes(tag), coms, C.c_size_t(len(coms)), m,
                                                      C.c_size_t(len(m)), bytes(revealed), C.c_size_t(len(revealed)), each, C.byref(ok)))
        return [bool(each[i]) for i in range(n)]
    _check(lib().zkaes_verify_gcm_segments(head._p, None if mid is None else mid._p, tail._p, b"".join(bytes(p) for p in proofs), lens, C.c_size_t(n), C.c_size_t(c), bytes(iv), bytes(aad),
                                           C.c_size_t(len(aad)), bytes(ciphertext), C.c_size_t(len(ciphertext)), bytes(tag), coms, C.c_size_t(len(coms)), each, C.byref(ok)))
    return [bool(each[i]) for i in range(n)]


def _gcm_segment_args(iv, aad, ciphertext, tag, commitments, mask, revealed):
    if len(iv) != 12:
        raise ZkAesError("GCM: only 96-bit (12-byte) IVs are supported")
    if len(tag) != 16:
        raise ZkAesError("GCM: only full 16-byte tags are supported")
    if any(len(x) != 32 for x in commitments):
        raise ZkAesError("a commitment is 32 bytes")
    if (mask is None) != (revealed is None):
        raise ZkAesError("GCM segments: mask and revealed go together")
    coms = b"".join(bytes(x) for x in commitments)
    m = None if mask is None else reveal_mask(mask, len(ciphertext))
    if m is not None and len(revealed) != len(ciphertext):
        raise ZkAesError("GCM segments: ONE revealed array over the whole record, %d bytes for this ciphertext" % len(ciphertext))
    return coms, m


def gcm_segment_public_inputs(n_segments, iv, aad, ciphertext, tag, commitments, c, mask=None, revealed=None, key_tag=None):
    """the public-input rows of a segmented GCM record -> (rows, roles): one bytes object of 0/1 per segment -- exactly what verify_gcm_segments checks segment s against
    -- and its role "head", "mid" or "tail" (zkaes_gcm_segment_public_inputs; no GPU).  The rows differ in length.  mask and revealed as in verify_gcm_segments.
    key_tag (16 or 32 bytes): its bits, LSB first per byte, in the HEAD's row behind com_out and ahead of the mask; the other rows are unchanged"""
    coms, m = _gcm_segment_args(iv, aad, ciphertext, tag, commitments, mask, revealed)
    n = int(n_segments)
    lens, roles = (C.c_size_t * max(n, 1))(), (C.c_int * max(n, 1))()
    args = (C.c_size_t(n), C.c_size_t(c), bytes(iv), bytes(aad), C.c_size_t(len(aad)), bytes(ciphertext), C.c_size_t(len(ciphertext)), bytes(tag), coms, C.c_size_t(len(coms)), m,
            C.c_size_t(0 if m is None else len(m)), None if m is None else bytes(revealed))
    fn = lib().zkaes_gcm_segment_public_inputs
    kt = _seg_key_tag(key_tag)
    if kt is not None:
        args, fn = args[:10] + (kt, C.c_size_t(len(kt))) + args[10:], lib().zkaes_gcm_segment_public_inputs_kt
    _check(fn(*args, None, lens, roles))
    out = C.create_string_buffer(max(1, sum(lens[s] for s in range(n))))
    _check(fn(*args, out, lens, roles))
    rows, off = [], 0
    for s in range(n):
        rows.append(out.raw[off:off + lens[s]])
        off += lens[s]
    return rows, [("head", "mid", "tail")[roles[s]] for s in range(n)]


def verify_gcm_segments_batch(vks, proofs, iv, aad, ciphertext, tag, commitments, c, mask=None, revealed=None, device=True, key_tag=None):
    """verify_gcm_segments through ONE multi-key batch: the same arguments, checks, errors and answers, for two MSMs and one pairing product instead of
    one pairing product per segment.  device as in verify_batch (zkaes_verify_gcm_segments_batch_gpu / zkaes_verify_gcm_segments_batch).  key_tag as in
    verify_gcm_segments, with the same cross cases"""
    coms, m = _gcm_segment_args(iv, aad, ciphertext, tag, commitments, mask, revealed)
    head, mid, tail = vks
    n = len(proofs)
    lens = (C.c_size_t * max(n, 1))(*[len(p) for p in proofs])
    each, ok = (C.c_int * max(n, 1))(), C.c_size_t()
    kt = _seg_key_tag(key_tag)
    if kt is not None:
        fn = lib().zkaes_verify_gcm_segments_batch_kt_gpu if device else lib().zkaes_verify_gcm_segments_batch_kt
        _check(fn(head._p, None if mid is None else mid._p, tail._p, b"".join(bytes(p) for p in proofs), lens, C.c_size_t(n), C.c_size_t(c), bytes(iv), bytes(aad), C.c_size_t(len(aad)),
                  bytes(ciphertext), C.c_size_t(len(ciphertext)), bytes(tag), coms, C.c_size_t(len(coms)), kt, C.c_size_t(len(kt)), m, C.c_size_t(0 if m is None else len(m)),
                  None if m is None else bytes(revealed), C.c_size_t(0 if m is None else len(revealed)), each, C.byref(ok)))
        return [bool(each[i]) for i in range(n)]
    fn = lib().zkaes_verify_gcm_segments_batch_gpu if device else lib().zkaes_verify_gcm_segments_batch
    _check(fn(head._p, None if mid is None else mid._p, tail._p, b"".join(bytes(p) for p in proofs), lens, C.c_size_t(n), C.c_size_t(c), bytes(iv), bytes(aad), C.c_size_t(len(aad)),
              bytes(ciphertext), C.c_size_t(len(ciphertext)), bytes(tag), coms, C.c_size_t(len(coms)), m, C.c_size_t(0 if m is None else len(m)), None if m is None else bytes(revealed),
              C.c_size_t(0 if m is None else len(revealed)), each, C.byref(ok)))
    return [bool(each[i]) for i in range(n)]


def verify_gcm_records_batch(records, device=True, key_tag=None):
    """the segment-proofs of SEVERAL records in ONE verify_batch_keys call -> one list of bools per record.  A record is the argument tuple of verify_gcm_segments_batch
    without device: (vks, proofs, iv, aad, ciphertext, tag, commitments, c[, mask, revealed]).  Key objects that several records share (the same head and mid keys, say)
    enter the batch once: they are told apart by identity.  The rows come from gcm_segment_public_inputs, which raises where verify_gcm_segments would for a record's
    lengths and counts; that a key fits its segment is left to the proof, which is rejected under a key of another shape.  key_tag: ONE tag of 16 or 32
    bytes for every record of the call -- the session's -- whose bits enter every head's row; a record made under another AES key has its head rejected, and so has a head
    whose key_tag_blocks do not fit the tag's length (here the cross cases reject and never raise, as every key-fit question of this call)"""
    keys, key_index, key_of, proofs, rows, counts = [], {}, [], [], [], []
    for rec in records:
        vks, rec_proofs, iv, aad, ciphertext, tag, commitments, c = rec[:8]
        mask, revealed = (tuple(rec[8:]) + (None, None))[:2]
        rec_rows, roles = gcm_segment_public_inputs(len(rec_proofs), iv, aad, ciphertext, tag, commitments, c, mask=mask, revealed=revealed, key_tag=key_tag)
        by_role = dict(zip(("head", "mid", "tail"), vks))
        for proof, row, role in zip(rec_proofs, rec_rows, roles):
            vk = by_role[role]
            if vk is None:
                raise ZkAesError("GCM segments: a record of more than two segments needs the mid key")
            if id(vk) not in key_index:
                key_index[id(vk)] = len(keys)
                keys.append(vk)
            key_of.append(key_index[id(vk)])
            proofs.append(proof)
            rows.append(row)
        counts.append(len(rec_proofs))
    if not proofs:
        return [[] for _ in counts]
    flat = verify_batch_keys(keys, key_of, proofs, rows, device=device)
    out, off = [], 0
    for k in counts:
        out.append(flat[off:off + k])
        off += k
    return out


def proof_roundtrip(proof):
    out, n = C.c_void_p(), C.c_size_t()
    _check(lib().zkaes_proof_roundtrip(bytes(proof), C.c_size_t(len(proof)), C.byref(out), C.byref(n)))
    return _take(out, n)


def circuit_info(circuit, plaintext_length, aad_length=0, key_bits=128, key_tag_blocks=0, digest=None, digest_prefix=0, reveal=False):
    """aad_length: GCM circuits only; key_bits: 128, 192 or 256, key_tag_blocks: 0, 1 or 2 and digest: None, "chain" or "final" (with digest_prefix) for the AES kinds"""
    out = (C.c_uint64 * 12)()
    _check(lib().zkaes_circuit_info_rv(int(circuit), C.c_uint(int(key_bits)), _tag_blocks(key_tag_blocks), *_digest_args(digest, digest_prefix), C.c_uint(int(bool(reveal))), C.c_size_t(plaintext_length),
                                       C.c_size_t(aad_length), out))
    keys = ["raw_constraints", "raw_instance", "raw_witness", "nnz_a", "nnz_b", "nnz_c", "constraints", "instance", "witness", "joint_nnz", "h", "k"]
    return dict(zip(keys, out))


def circuit_matrix(circuit, plaintext_length, which, aad_length=0, key_bits=128, key_tag_blocks=0, digest=None, digest_prefix=0, reveal=False):
    rows, nnz = C.c_uint64(), C.c_uint64()
    head = (int(circuit), C.c_uint(int(key_bits)), _tag_blocks(key_tag_blocks), *_digest_args(digest, digest_prefix), C.c_uint(int(bool(reveal))), C.c_size_t(plaintext_length), C.c_size_t(aad_length), which)
    _check(lib().zkaes_circuit_matrix_rv(*head, C.byref(rows), C.byref(nnz), None, None, None))
    rowptr = np.zeros(rows.value + 1, dtype=np.uint32)
    col = np.zeros(max(nnz.value, 1), dtype=np.uint32)
    coeff = np.zeros(max(nnz.value, 1), dtype=np.int64)
    _check(lib().zkaes_circuit_matrix_rv(*head, None, None, rowptr.ctypes.data_as(C.c_void_p), col.ctypes.data_as(C.c_void_p), coeff.ctypes.data_as(C.c_void_p)))
    return rowptr, col[:nnz.value], coeff[:nnz.value]


def ntt(field_id, data_mont_bytes, inverse=False):
    n = len(data_mont_bytes) // 32
    buf = C.create_string_buffer(bytes(data_mont_bytes), len(data_mont_bytes))
    _check(lib().zkaes_ntt(int(field_id), buf, C.c_size_t(n), 1 if inverse else 0))
    return buf.raw


def ntt_coset(field_id, data_mont_bytes, coset_c, lg_big, inverse=False):
    n = len(data_mont_bytes) // 32
    buf = C.create_string_buffer(bytes(data_mont_bytes), len(data_mont_bytes))
    _check(lib().zkaes_ntt_coset(int(field_id), buf, C.c_size_t(n), 1 if inverse else 0, int(coset_c), int(lg_big)))
    return buf.raw


def ntt_batch(field_id, vectors, cosets=None, lg_big=0, inverse=False):
    """several transforms of one size in shared launches: vectors = list of equal-length Montgomery byte strings, cosets[i] = 0 (plain) or the coset index of vector i"""
    count, n = len(vectors), len(vectors[0]) // 32
    if any(len(v) != 32 * n for v in vectors):
        raise ZkAesError("ntt_batch: vectors of one length")
    buf = C.create_string_buffer(b"".join(bytes(v) for v in vectors), 32 * n * count)
    cs = (C.c_int * count)(*[int(c) for c in cosets]) if cosets is not None else None
    _check(lib().zkaes_ntt_batch(int(field_id), buf, C.c_size_t(n), count, 1 if inverse else 0, cs, int(lg_big)))
    return [buf.raw[32 * n * i:32 * n * (i + 1)] for i in range(count)]


# ---- kernel-level entry points for tests (include/zkaes.h): one call = one launch wrapper of the prover's polynomial layer; 32-byte Montgomery limbs in and out
def _ptr_array(bufs):
    """(array of const uint8_t *, array of size_t lengths in elements) for a list of byte strings; the list itself keeps the buffers alive"""
    n = len(bufs)
    return (C.c_char_p * n)(*[bytes(b) if len(b) else None for b in bufs]), (C.c_size_t * n)(*[len(b) // 32 for b in bufs])


def poly_divide_by_vanishing(p, m, with_scratch=False, want_rem=True):
    """(quotient, remainder or None) of p / (X^m - 1)"""
    n = len(p) // 32
    q = C.create_string_buffer(32 * max(n - m, 0) or 1)
    rem = C.create_string_buffer(32 * m or 1) if want_rem else None
    _check(lib().zkaes_poly_divide_by_vanishing(bytes(p), C.c_size_t(n), C.c_size_t(m), 1 if with_scratch else 0, q, rem))
    return q.raw[:32 * (n - m)], (rem.raw[:32 * m] if want_rem else None)


def poly_divide_by_linear(p, z):
    n = len(p) // 32
    q = C.create_string_buffer(32 * max(n - 1, 0) or 1)
    _check(lib().zkaes_poly_divide_by_linear(bytes(p), C.c_size_t(n), bytes(z), q))
    return q.raw[:32 * max(n - 1, 0)]


def poly_eval_multi(polys, xs):
    """[p(x) for p, x in zip(polys, xs)] as 32-byte strings; 1..8 polynomials"""
    count = len(polys)
    ptrs, lens = _ptr_array(polys)
    out = C.create_string_buffer(32 * max(count, 1))
    _check(lib().zkaes_poly_eval_multi(ptrs, lens, b"".join(bytes(x) for x in xs), count, out))
    return [out.raw[32 * i:32 * i + 32] for i in range(count)]


def batch_inverse(v, post=None, throughput_variant=False):
    n = len(v) // 32
    buf = C.create_string_buffer(bytes(v), max(len(v), 1))
    _check(lib().zkaes_batch_inverse(buf, C.c_size_t(n), None if post is None else bytes(post), 1 if throughput_variant else 0))
    return buf.raw[:32 * n]


def poly_lincomb(polys, scalars, n):
    count = len(polys)
    ptrs, lens = _ptr_array(polys)
    out = C.create_string_buffer(32 * n or 1)
    _check(lib().zkaes_poly_lincomb(ptrs, lens, b"".join(bytes(x) for x in scalars), count, C.c_size_t(n), out))
    return out.raw[:32 * n]


def vanishing_quotient_evals(lg_n, gs, a, indices=None):
    """one byte string per coset g in gs: the whole table (2^lg_n elements), or the values at `indices`"""
    ncosets, per = len(gs), (1 << lg_n) if indices is None else len(indices)
    out = C.create_string_buffer(32 * per * ncosets or 1)
    idx = None if indices is None else (C.c_uint32 * max(per, 1))(*indices)
    _check(lib().zkaes_vanishing_quotient_evals(int(lg_n), b"".join(bytes(g) for g in gs), ncosets, bytes(a), idx, C.c_size_t(0 if indices is None else per), out))
    return [out.raw[32 * per * c:32 * per * (c + 1)] for c in range(ncosets)]


def q1_coset_pointwise(r, za, zb, t, z, ca, cb, cz, eta_a, eta_b, eta_c):
    n = len(r) // 32
    out = C.create_string_buffer(32 * n or 1)
    consts = b"".join(bytes(x) for x in (ca, cb, cz, eta_a, eta_b, eta_c))
    _check(lib().zkaes_q1_coset_pointwise(bytes(r), bytes(za), bytes(zb), bytes(t), bytes(z), consts, C.c_size_t(n), out))
    return out.raw[:32 * n]


def h2_coset(row, col, va, vb, vc, rc, f, alpha, beta, alpha_beta, ea, eb, ec, vinv):
    k = len(row) // 32
    out = C.create_string_buffer(32 * k or 1)
    arrays = (C.c_char_p * 7)(*[bytes(x) for x in (row, col, va, vb, vc, rc, f)])
    consts = b"".join(bytes(x) for x in (alpha, beta, alpha_beta, ea, eb, ec, vinv))
    _check(lib().zkaes_h2_coset(arrays, consts, C.c_size_t(k), out))
    return out.raw[:32 * k]


def q1_combine(q0, q1, q3, mask, inv2, inv2zeta):
    """(h1: 2n elements, g1: n - 1 elements)"""
    n = len(q0) // 32
    h1, g1 = C.create_string_buffer(64 * n or 1), C.create_string_buffer(32 * max(n - 1, 0) or 1)
    _check(lib().zkaes_q1_combine(bytes(q0), bytes(q1), bytes(q3), bytes(mask), bytes(inv2), bytes(inv2zeta), C.c_size_t(n), h1, g1))
    return h1.raw[:64 * n], g1.raw[:32 * max(n - 1, 0)]


def coset_scale(data, g, n):
    out = C.create_string_buffer(32 * n or 1)
    _check(lib().zkaes_coset_scale(bytes(data), C.c_size_t(len(data) // 32), bytes(g), C.c_size_t(n), out))
    return out.raw[:32 * n]


def z_poly_from_w(w, x_poly, n):
    """w (X^m - 1) + x_poly with m = len(x_poly): n + 1 coefficients"""
    out = C.create_string_buffer(32 * (n + 1))
    _check(lib().zkaes_z_poly_from_w(bytes(w), C.c_size_t(len(w) // 32), bytes(x_poly), C.c_uint32(len(x_poly) // 32), C.c_size_t(n), out))
    return out.raw


def ntt_padded(field_id, data_mont_bytes, n, inverse=False, coset_c=0, lg_big=0):
    """the transform of a short input that the first pass's gather pads with zeros to n elements"""
    out = C.create_string_buffer(32 * n)
    _check(lib().zkaes_ntt_padded(int(field_id), bytes(data_mont_bytes), C.c_size_t(len(data_mont_bytes) // 32), C.c_size_t(n), 1 if inverse else 0, int(coset_c), int(lg_big), out))
    return out.raw


def ntt_scaled(g, data_mont_bytes, n, inverse=False):
    """BLS12-377: forward = the values on g D of the (zero-padded) coefficients, inverse = the coefficients from such values"""
    out = C.create_string_buffer(32 * n)
    _check(lib().zkaes_ntt_scaled(bytes(g), bytes(data_mont_bytes), C.c_size_t(len(data_mont_bytes) // 32), C.c_size_t(n), 1 if inverse else 0, out))
    return out.raw


# ---- TEST-ONLY: one field / curve operation per launch on raw limbs (include/zkaes.h zkaes_arith_probe, csrc/arith_probe.cuh ZK_PROBE_OPS).
# ARITH_OPS: name -> (op id, input words per case, output words per case).  tests/test_arith_model.py checks this table against the one compiled into the probes.
def _arith_ops():
    t = {}
    for base, f, n in ((0, "fr377", 8), (16, "fr381", 8), (32, "fq377", 12), (48, "fq381", 12)):
        for i, (name, nin) in enumerate((("mul", 2 * n), ("add", 2 * n), ("sub", 2 * n), ("neg", n), ("dbl", n), ("inverse", n), ("from_i64", 2), ("pow_u64", n + 2), ("from_raw", n), ("to_raw", n))):
            t["%s.%s" % (f, name)] = (base + i, nin, n)
    for base, f in ((64, "fq377x28"), (96, "fq381x28")):
        ops = [("mul", 28, 14), ("sqr", 14, 14), ("fma2", 56, 14), ("add", 28, 14), ("add_lazy", 28, 14), ("dbl_lazy", 14, 14)]
        ops += [("sub%d" % k, 28, 14) for k in (2, 3, 4, 5, 6, 7)] + [("sub_lazy%d" % k, 28, 14) for k in (2, 3)]
        ops += [("canonical", 14, 14), ("product_is_zero", 14, 1), ("is_zero_mod_p", 14, 1), ("from_std", 12, 14), ("to_std", 14, 12)]
        if f == "fq377x28":
            ops.append(("mul_biased", 28, 14))
        for i, (name, nin, nout) in enumerate(ops):
            t["%s.%s" % (f, name)] = (base + i, nin, nout)
    for base, f in ((128, "fr377x29"), (160, "fr381x29")):
        ops = [("mul", 18, 9), ("dot2", 36, 9), ("dot3", 54, 9), ("dot4", 72, 9), ("add", 18, 9), ("add_lazy", 18, 9)]
        ops += [("sub%d" % k, 18, 9) for k in (1, 2, 4, 8)] + [("sub_lazy2", 18, 9), ("normalized", 9, 9), ("shl5", 9, 9)]
        ops += [("canonical%d" % k, 9, 9) for k in (0, 1, 4)] + [("reduce_by_top_limb", 9, 9), ("twiddle_from_std", 8, 9), ("split", 8, 9), ("pack", 9, 8)]
        for i, (name, nin, nout) in enumerate(ops):
            t["%s.%s" % (f, name)] = (base + i, nin, nout)
    for i, (name, nin, nout) in enumerate((("te_madd", 98, 56), ("te_add", 112, 56), ("te_dbl", 56, 56), ("te_neg", 56, 56), ("te_to_std_point", 56, 48), ("niels_from_weierstrass", 24, 43),
                                           ("te_madd_hot", 142, 98), ("te_add_quad", 112, 56), ("te_dbl_quad", 56, 56))):
        t["te377.%s" % name] = (192 + i, nin, nout)
    for base, f in ((208, "w377"), (216, "w381")):
        for i, (name, nin, nout) in enumerate((("madd28", 84, 57), ("add28", 112, 56), ("dbl28", 56, 56), ("neg28", 56, 56), ("to_std_point", 56, 48))):
            t["%s.%s" % (f, name)] = (base + i, nin, nout)
    return t


ARITH_OPS = _arith_ops()
# the zipped products of te_madd_hot (arith_probe.cuh ZK_PROBE_ZIP_OPS; device only, outside ARITH_OPS: tests/test_gpu_lower_seed.py).  Per case: a_0 b_0 a_1 b_1 ... in,
# the products out; the digits are the bound products (in units of 2^56) of the operand pairs each probe was instantiated for.
ARITH_ZIP_OPS = {"fq377x28.mul_zip_12": (232, 28, 14), "fq377x28.mul_zip_8": (233, 28, 14), "fq377x28.mul_zip_5_2_1": (234, 84, 42), "fq377x28.mul_zip_12_8_6_12": (235, 112, 56)}
ARITH_QUAD_OPS = ("te377.te_add_quad", "te377.te_dbl_quad")      # four lanes per case on the device; no host body


def arith_probe(op_name, cases):
    """cases: bytes of little-endian 32-bit words, a whole number of cases (1 .. 65536) of ARITH_OPS[op_name][1] words each -> the output words as bytes"""
    op, nin, nout = ARITH_OPS[op_name] if op_name in ARITH_OPS else ARITH_ZIP_OPS[op_name]
    cases = bytes(cases)
    n, rest = divmod(len(cases), 4 * nin)
    if rest:
        raise ZkAesError("arith_probe: %s takes %d words per case" % (op_name, nin))
    out = C.create_string_buffer(4 * nout * n or 1)
    _check(lib().zkaes_arith_probe(int(op), cases, C.c_size_t(n), out))
    return out.raw[:4 * nout * n]


def msm(curve_id, bases_bytes, scalars_bytes):
    n = len(scalars_bytes) // 32
    out = C.create_string_buffer(96)
    inf = C.c_int()
    _check(lib().zkaes_msm(int(curve_id), bytes(bases_bytes), bytes(scalars_bytes), C.c_size_t(n), out, C.byref(inf)))
    return out.raw, bool(inf.value)


def g1_sum(curve_id, points):
    """Host-side sum of [(xy_bytes96, is_inf), ...] -> (xy_bytes96, is_inf)."""
    n = len(points)
    buf = b"".join(bytes(p[0]) for p in points)
    inf = (C.c_int * max(n, 1))(*[1 if p[1] else 0 for p in points])
    out = C.create_string_buffer(96)
    oinf = C.c_int()
    _check(lib().zkaes_g1_sum(int(curve_id), buf, inf, C.c_size_t(n), out, C.byref(oinf)))
    return out.raw, bool(oinf.value)


def msm_sharded_plan(curve_id, n_total):
    """(window_bits, n_windows, bytes_per_rank) of a point-range-sharded MSM over n_total points"""
    c, w, b = C.c_int(), C.c_int(), C.c_size_t()
    _check(lib().zkaes_msm_sharded_plan(int(curve_id), C.c_size_t(n_total), C.byref(c), C.byref(w), C.byref(b)))
    return c.value, w.value, b.value


def msm_window_sums_dev(curve_id, bases_bytes, scalars_bytes, n_total, dev_ptr, dev_bytes):
    """Pippenger over this rank's slice; the window sums stay in device memory at dev_ptr (an int device address, e.g. tensor.data_ptr())"""
    n = len(scalars_bytes) // 32
    _check(lib().zkaes_msm_window_sums_dev(int(curve_id), bytes(bases_bytes), bytes(scalars_bytes), C.c_size_t(n), C.c_size_t(n_total), C.c_void_p(dev_ptr), C.c_size_t(dev_bytes)))


def msm_fold_window_sums_dev(curve_id, dev_ptr, world, n_total):
    out = C.create_string_buffer(96)
    inf = C.c_int()
    _check(lib().zkaes_msm_fold_window_sums_dev(int(curve_id), C.c_void_p(dev_ptr), int(world), C.c_size_t(n_total), out, C.byref(inf)))
    return out.raw, bool(inf.value)


def msm_fold_partials_dev(curve_id, dev_ptr, world):
    out = C.create_string_buffer(96)
    inf = C.c_int()
    _check(lib().zkaes_msm_fold_partials_dev(int(curve_id), C.c_void_p(dev_ptr), int(world), out, C.byref(inf)))
    return out.raw, bool(inf.value)


def msm_table(curve_id, bases_bytes, scalars_bytes, window_bits, srs=False):
    """precomputed-window MSM.  srs=True (377 only): the prover's SRS path on the twisted Edwards model -- bases MUST lie in the prime-order subgroup"""
    n = len(scalars_bytes) // 32
    out = C.create_string_buffer(96)
    inf = C.c_int()
    if srs:
        if int(curve_id) != 377:
            raise ValueError("the SRS (twisted Edwards) table path exists for BLS12-377 only")
        _check(lib().zkaes_msm_table_srs(bytes(bases_bytes), bytes(scalars_bytes), C.c_size_t(n), int(window_bits), out, C.byref(inf)))
    else:
        _check(lib().zkaes_msm_table(int(curve_id), bytes(bases_bytes), bytes(scalars_bytes), C.c_size_t(n), int(window_bits), out, C.byref(inf)))
    return out.raw, bool(inf.value)


# ---- TEST / DEBUG: the MSM forms the prover calls (include/zkaes.h; BLS12-377).  bases: 96-byte standard affine points as bytes or a C-contiguous uint8 numpy array
# (a million tiled points need no copy); scalars: 32-byte Montgomery limbs; edwards=True is the prover's law.  Points come back as (xy bytes, is_infinity).
def _host(buf):
    if isinstance(buf, np.ndarray):
        if not buf.flags["C_CONTIGUOUS"]:
            raise ValueError("array arguments must be C-contiguous")
        return buf.ctypes.data_as(C.c_void_p)
    return bytes(buf)


def _nbytes(buf):
    return buf.nbytes if isinstance(buf, np.ndarray) else len(buf)


def class_sum(bases, vals, edwards=True, prior_msm_points=0):
    """vals: 1..8 int8 arrays of one length n = len(bases) / 96 -> [(accepted, xy, is_inf), ...], the vectors summed one after the other on one workspace"""
    n, count = _nbytes(bases) // 96, len(vals)
    v = np.ascontiguousarray(np.stack([np.asarray(x, dtype=np.int8) for x in vals])) if count else np.zeros((0, n), dtype=np.int8)
    if count and v.shape[1] != n:
        raise ValueError("every value vector needs one value per base")
    ok, inf, out = (C.c_int * max(count, 1))(), (C.c_int * max(count, 1))(), C.create_string_buffer(96 * max(count, 1))
    _check(lib().zkaes_class_sum(_host(bases), C.c_size_t(n), v.ctypes.data_as(C.c_void_p), int(count), 1 if edwards else 0, C.c_size_t(prior_msm_points), ok, out, inf))
    return [(bool(ok[i]), out.raw[96 * i:96 * i + 96], bool(inf[i])) for i in range(count)]


def msm_pair(bases, scal1, scal2, val_off2, edwards=True):
    """sum scal1[i] bases[i] + sum scal2[j] bases[val_off2 + j] as ONE per-window Pippenger instance"""
    out, inf = C.create_string_buffer(96), C.c_int()
    _check(lib().zkaes_msm_pair(_host(bases), C.c_size_t(_nbytes(bases) // 96), bytes(scal1), C.c_size_t(len(scal1) // 32), bytes(scal2), C.c_size_t(len(scal2) // 32), C.c_size_t(val_off2),
                                1 if edwards else 0, out, C.byref(inf)))
    return out.raw, bool(inf.value)


def msm_table_pair(bases, scal1, off1, scal2, off2, window_bits, edwards=True):
    """the same in table mode: window tables over ALL the bases (the stride), the vectors over the ranges starting at off1 and off2"""
    out, inf = C.create_string_buffer(96), C.c_int()
    _check(lib().zkaes_msm_table_pair(_host(bases), C.c_size_t(_nbytes(bases) // 96), bytes(scal1), C.c_size_t(len(scal1) // 32), C.c_size_t(off1), bytes(scal2), C.c_size_t(len(scal2) // 32),
                                      C.c_size_t(off2), int(window_bits), 1 if edwards else 0, out, C.byref(inf)))
    return out.raw, bool(inf.value)


def msm_second_bases(bases, scalars, off, shift, window_bits=0):
    """one digit pass, two base ranges (Edwards law): [sum scalars[i] bases[off + i], sum scalars[i] bases[off + shift + i]]; window_bits = 0: per-window buckets"""
    out, inf = C.create_string_buffer(192), (C.c_int * 2)()
    _check(lib().zkaes_msm_second_bases(_host(bases), C.c_size_t(_nbytes(bases) // 96), bytes(scalars), C.c_size_t(len(scalars) // 32), C.c_size_t(off), C.c_size_t(shift), int(window_bits), out, inf))
    return [(out.raw[96 * i:96 * i + 96], bool(inf[i])) for i in range(2)]


STEP_WINDOW, STEP_TABLE, STEP_SECOND, STEP_CLASS, STEP_REFINISH = 0, 1, 2, 3, 4
MSM_SEQ_MAX_STEPS, MSM_SEQ_ERR_BYTES = 32, 128


class MsmStep(C.Structure):
    """zkaes_msm_step (include/zkaes.h): lengths and offsets in elements of the bases, the scalars and the class values of the call"""
    _fields_ = [("kind", C.c_uint32), ("edwards", C.c_uint32), ("window_bits", C.c_uint32), ("reserved", C.c_uint32),
                ("n1", C.c_uint64), ("off1", C.c_uint64), ("scal1", C.c_uint64), ("n2", C.c_uint64), ("off2", C.c_uint64), ("scal2", C.c_uint64), ("shift", C.c_uint64)]


def msm_sequence(bases, scalars, class_vals, steps, poison=False):
    """`steps` (MsmStep or dicts of its fields) in order on ONE workspace and stream -> per step a dict: status (0, or 1 for a step the library refused: the sequence
    went on), error (its message), accepted (False: a class sum declined, or the step was refused), points [(xy, is_inf), (xy, is_inf)] (the second one: STEP_SECOND)"""
    st = (MsmStep * max(len(steps), 1))(*[s if isinstance(s, MsmStep) else MsmStep(**s) for s in steps])
    v = np.ascontiguousarray(class_vals, dtype=np.int8)
    k = max(len(steps), 1)
    out, inf, ok, status, err = C.create_string_buffer(192 * k), (C.c_int * (2 * k))(), (C.c_int * k)(), (C.c_int * k)(), C.create_string_buffer(MSM_SEQ_ERR_BYTES * k)
    _check(lib().zkaes_msm_sequence(_host(bases), C.c_size_t(_nbytes(bases) // 96), bytes(scalars), C.c_size_t(len(scalars) // 32), v.ctypes.data_as(C.c_void_p), C.c_size_t(v.size),
                                    st, C.c_size_t(len(steps)), 1 if poison else 0, out, inf, ok, status, err))
    res = []
    for i in range(len(steps)):
        msg = err.raw[MSM_SEQ_ERR_BYTES * i:MSM_SEQ_ERR_BYTES * (i + 1)].split(b"\0")[0].decode()
        res.append({"status": int(status[i]), "error": msg, "accepted": bool(ok[i]),
                    "points": [(out.raw[192 * i + 96 * j:192 * i + 96 * j + 96], bool(inf[2 * i + j])) for j in range(2)]})
    return res


# ---- TEST SURFACE, not product API: the prover's R1CS and randomness kernels, one entry per kernel group (include/zkaes.h; tests/test_gpu_r1cs.py).  Field elements are
# 32-byte Montgomery limbs; a matrix is a CSR triple (rowptr uint32[rows + 1], col uint32[nnz], coeff int64[nnz]).  Arguments are passed on as they are: the C side refuses.
def _csr(rowptr, col, coeff):
    """C-contiguous arrays of the ABI's types (never empty, so that their pointers are valid); the caller keeps them alive"""
    fix = lambda a, t: np.ascontiguousarray(a, dtype=t) if len(a) else np.zeros(1, dtype=t)
    return fix(rowptr, np.uint32), fix(col, np.uint32), fix(coeff, np.int64)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def spmv_bits(rowptr, col, coeff, rows, rows_out, z, want_small=True):
    """(field sums: 32 rows_out bytes, int8 classes clamped to +-127 or None)"""
    rp, cl, co = _csr(rowptr, col, coeff)
    zz = np.ascontiguousarray(z, dtype=np.uint8)
    out = C.create_string_buffer(32 * max(rows_out, 1))
    small = np.zeros(max(rows_out, 1), dtype=np.int8) if want_small else None
    _check(lib().zkaes_spmv_bits(_p(rp), _p(cl), _p(co), C.c_size_t(rows), C.c_size_t(rows_out), _p(zz) if len(zz) else None, C.c_size_t(len(zz)), out, _p(small) if want_small else None))
    return out.raw[:32 * rows_out], (small[:rows_out] if want_small else None)


def w_maps(z, n, m, num_witness, x_evals):
    """(w_classes int8[n], w_evals, z_evals_h, bits_to_field(z, m)) for z = m instance bits then num_witness witness bits"""
    zz = np.ascontiguousarray(z, dtype=np.uint8)
    classes = np.zeros(max(n, 1), dtype=np.int8)
    w, zh, xf = C.create_string_buffer(32 * max(n, 1)), C.create_string_buffer(32 * max(n, 1)), C.create_string_buffer(32 * max(m, 1))
    _check(lib().zkaes_w_maps(_p(zz), C.c_size_t(n), C.c_size_t(m), C.c_size_t(num_witness), bytes(x_evals), _p(classes), w, zh, xf))
    return classes[:n], w.raw[:32 * n], zh.raw[:32 * n], xf.raw[:32 * m]


def t_evals(n, m, rows, mats, r_alpha, eta_a, eta_b, eta_c):
    """mats = the CSR triples of A, B, C -> (t on H: 32 n bytes, {"nseg", "n_heavy", "max_segments"} of the tables built by the prover's own builder)"""
    held = [_csr(*t) for t in mats]
    ptrs = [(C.c_void_p * 3)(*[h[j].ctypes.data for h in held]) for j in range(3)]
    out, stats = C.create_string_buffer(32 * max(n, 1)), (C.c_uint64 * 3)()
    _check(lib().zkaes_t_evals(C.c_size_t(n), C.c_size_t(m), C.c_size_t(rows), ptrs[0], ptrs[1], ptrs[2], bytes(r_alpha), bytes(eta_a) + bytes(eta_b) + bytes(eta_c), out, stats))
    return out.raw[:32 * n], dict(zip(("nseg", "n_heavy", "max_segments"), (int(x) for x in stats)))


def lagrange_scalars(lg_n, lg_m, beta):
    """(L_k(beta), the same over v_X(beta) and zero on X) on the domain of size 2^lg_n"""
    size = 32 << lg_n if 0 <= lg_n <= 24 else 32
    lag, lag_w = C.create_string_buffer(size), C.create_string_buffer(size)
    _check(lib().zkaes_lagrange_scalars(int(lg_n), int(lg_m), bytes(beta), lag, lag_w))
    return lag.raw, lag_w.raw


def f_evals_from_tables(va, vb, vc, ea, eb, ec, ra, rb, ri, ci):
    k, n = len(va) // 32, len(ra) // 32
    ria, cia = np.ascontiguousarray(ri, dtype=np.uint32), np.ascontiguousarray(ci, dtype=np.uint32)
    out = C.create_string_buffer(32 * max(k, 1))
    _check(lib().zkaes_f_evals_from_tables(bytes(va), bytes(vb), bytes(vc), bytes(ea), bytes(eb), bytes(ec), bytes(ra), bytes(rb), _p(ria), _p(cia), C.c_size_t(k), C.c_size_t(n), out))
    return out.raw[:32 * k]


def chacha_field_stream(key_words, rounds, word_pos, count, max_cand=0):
    """(count field elements as bytes, the stream position in words after the last accepted candidate)"""
    key = (C.c_uint32 * 8)(*key_words)
    out, nxt = C.create_string_buffer(32 * max(count, 1)), C.c_uint64()
    _check(lib().zkaes_chacha_field_stream(key, int(rounds), C.c_uint64(word_pos), C.c_size_t(count), C.c_uint32(max_cand), out, C.byref(nxt)))
    return out.raw[:32 * count], int(nxt.value)


def mask_fixup(p, n):
    buf = C.create_string_buffer(bytes(p), max(len(p), 1))
    _check(lib().zkaes_mask_fixup(buf, C.c_size_t(n)))
    return buf.raw[:len(p)]


# ---- TEST SURFACE, not product API: the kernels that build a key (include/zkaes.h; tests/test_gpu_keysynth.py).  A point is 96 bytes of standard affine x || y, infinity 96 zero
# bytes, in and out; counts and chunks are passed on as they are: the C side refuses.
def fixed_base_powers(curve_id, base_xy, beta, start, count, chunk=0):
    """beta^(start + i) * base for i < count -> 96 count bytes; chunk = points per launch (0: key synthesis's 2^20)"""
    out = C.create_string_buffer(96 * count if 0 < count <= 1 << 20 else 1)
    _check(lib().zkaes_fixed_base_powers(int(curve_id), bytes(base_xy), bytes(beta), C.c_uint64(start), C.c_size_t(count), C.c_size_t(chunk), out))
    return out.raw[:96 * count]


def fixed_base_scalars(base_xy, scalars, chunk=0):
    """BLS12-377: scalars[i] * base -> 96 bytes per scalar"""
    count = len(scalars) // 32
    out = C.create_string_buffer(96 * count if 0 < count <= 1 << 20 else 1)
    _check(lib().zkaes_fixed_base_scalars(bytes(base_xy), bytes(scalars), C.c_size_t(count), C.c_size_t(chunk), out))
    return out.raw[:96 * count]


def table_next(curve_id, prev, window_bits, j):
    """window-table copy j from copy j - 1: 2^(width of window j - 1) * prev[i]"""
    count = len(prev) // 96
    out = C.create_string_buffer(96 * count or 1)
    _check(lib().zkaes_table_next(int(curve_id), bytes(prev), C.c_size_t(count), int(window_bits), int(j), out))
    return out.raw[:96 * count]


def table_windows(curve_id, window_bits):
    """the number of window-table copies: ceil((bits of r + 1) / window_bits)"""
    return -(-({377: 253, 381: 255}[int(curve_id)] + 1) // int(window_bits))


def build_window_tables(curve_id, bases, window_bits):
    """all window-table copies of the bases, copy j at 96 n j"""
    n = len(bases) // 96
    total = n * table_windows(curve_id, window_bits) if int(curve_id) in (377, 381) and 2 <= int(window_bits) <= 22 and n <= 1 << 20 else 0
    out = C.create_string_buffer(96 * total or 1)
    _check(lib().zkaes_build_window_tables(int(curve_id), bytes(bases), C.c_size_t(n), int(window_bits), out))
    return out.raw[:96 * total]


NIELS_RECORD_BYTES = 192


def convert_bases_te(points):
    """BLS12-377: the Niels records of the points -> [(y - x, y + x, 2 d x y), ...], each coordinate a list of fourteen 28-bit limbs as stored; the records' padding is ignored"""
    n = len(points) // 96
    out = C.create_string_buffer(NIELS_RECORD_BYTES * n if 0 < n <= 1 << 20 else 1)
    _check(lib().zkaes_convert_bases_te(bytes(points), C.c_size_t(n), out))
    words = np.frombuffer(out.raw[:NIELS_RECORD_BYTES * n], dtype="<u4").reshape(n, NIELS_RECORD_BYTES // 4)
    return [tuple([int(x) for x in rec[14 * i:14 * i + 14]] for i in range(3)) for rec in words]


INDEX_EVALS_TAIL = 64


def index_evals(ci, ri, ca, cb, cc, lg_k, lg_n):
    """the index polynomials' values on K of a joint matrix of len(ci) entries -> {"row", "col", "row_col", "val_a", "val_b", "val_c", "u_inv": 32 k bytes each,
    "tails": what the kernels left of the poison fill behind the seven arrays (INDEX_EVALS_TAIL elements each, all 0xAB unless a kernel wrote out of its range)}"""
    cnt = len(ci)
    idx = [np.ascontiguousarray(a, dtype=np.uint32) if cnt else np.zeros(1, dtype=np.uint32) for a in (ci, ri)]
    co = [np.ascontiguousarray(a, dtype=np.int64) if cnt else np.zeros(1, dtype=np.int64) for a in (ca, cb, cc)]
    k = 1 << lg_k if 0 <= lg_k <= 20 else 0
    outs = [C.create_string_buffer(32 * (k + INDEX_EVALS_TAIL)) for _ in range(7)]
    _check(lib().zkaes_index_evals(_p(idx[0]), _p(idx[1]), _p(co[0]), _p(co[1]), _p(co[2]), C.c_size_t(cnt), int(lg_k), int(lg_n), *outs))
    res = {name: o.raw[:32 * k] for name, o in zip(("row", "col", "row_col", "val_a", "val_b", "val_c", "u_inv"), outs)}
    res["tails"] = b"".join(o.raw[32 * k:] for o in outs)
    return res


def msm_bench(curve_id, bases_bytes, scalars_bytes, reps=3):
    n = len(scalars_bytes) // 32
    t, a = C.c_double(), C.c_double()
    _check(lib().zkaes_msm_bench(int(curve_id), bytes(bases_bytes), bytes(scalars_bytes), C.c_size_t(n), int(reps), C.byref(t), C.byref(a)))
    return t.value, a.value


def msm_bench_synth(n, window_bits=0, reps=3, want_point=False):
    t, a = C.c_double(), C.c_double()
    out = C.create_string_buffer(96)
    _check(lib().zkaes_msm_bench_synth(C.c_size_t(n), int(window_bits), int(reps), C.byref(t), C.byref(a), out))
    return (t.value, a.value, out.raw) if want_point else (t.value, a.value)


def set_default_contexts(n):
    """zkaes_set_default_contexts: the process default of prover contexts per key (0 = back to ZKAES_CONTEXTS / 12); also what key synthesis reserves beside the window tables"""
    _check(lib().zkaes_set_default_contexts(C.c_size_t(n)))


def srs_hold(hold=True):
    """zkaes_srs_hold: keep every universal / Lagrange SRS resident after its last key is freed (hold=False releases them again)"""
    _check(lib().zkaes_srs_hold(1 if hold else 0))


def int_rate_bench(seconds=0.5):
    """zkaes_int_rate_bench: per-box calibration of the integer roof (include/zkaes.h)"""
    out = (C.c_double * 8)()
    _check(lib().zkaes_int_rate_bench(C.c_double(seconds), out))
    return {"fq_products_per_s": out[0], "fq_stream_sclk_mhz": out[1], "mad_per_s": 378.0 * out[0], "hot_loop_l2_additions_per_s": out[2], "hot_loop_l2_sclk_mhz": out[3],
            "hot_loop_cycles_per_addition_per_wave": out[4], "rounds": int(out[5])}


def stream_copy_bench(nbytes=1 << 30, reps=20):
    """Measured HBM stream-copy rate (read + write GB/s) of a plain 16 B/lane copy kernel -- printed beside the nominal peak."""
    g = C.c_double()
    _check(lib().zkaes_stream_copy_bench(C.c_size_t(nbytes), int(reps), C.byref(g)))
    return g.value


def mem_info():
    """(free, total) bytes of the current device"""
    f, t = C.c_uint64(), C.c_uint64()
    _check(lib().zkaes_mem_info(C.byref(f), C.byref(t)))
    return int(f.value), int(t.value)


def msm_stats(reset=False):
    out = (C.c_double * 5)()
    _check(lib().zkaes_msm_stats(out, 1 if reset else 0))
    return dict(accumulate_ms=out[0], total_ms=out[1], points=int(out[2]), launches=int(out[3]), pairs=int(out[4]))
