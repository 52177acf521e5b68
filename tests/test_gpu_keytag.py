"""Key tags on the GPU: k_key_tag_trace behind each mode's trace kernel(s), the witness against the tagged circuit's own matrices, lone, chunked and batch proofs
checked against ONE tag, and the splice this feature exists to stop.

A key synthesized with key_tag_blocks = T proves tag_t = AES_K(D_t), t < T, beside its mode's statement; the 128 T tag bits are the last public inputs.
Correctness rests on the pure-Python model of test_keysize_host.py and a row-by-row check of (A z) o (B z) = C z in int64 numpy over the matrices
circuit_matrix(..., key_tag_blocks=T) returns.  The shapes are the smallest at which the new kernel or layout can go wrong: one tag lane (ECB-128 16 B T = 1), the second
lane at the slot stride (T = 2), NK = 8 with slots that begin 8 mod 16 before the rounding (ECB-256 32 B T = 2), the slots behind the CBC tail (CBC-192 32 B), behind a
ragged CTR tail (CTR-128 17 B) and behind the GHASH tail (GCM-256 (17, 5)).  Every key is synthesized over an SRS sized from its own circuit, without window tables, once
per module.
"""
import os

import numpy as np
import pytest

from test_gpu_keysize import bits, flip, kind_of, layout, model_public, statement, witness
from test_keysize_host import ks_cbc, ks_ctr, ks_ecb, ks_gcm
from test_keytag_host import D, model_key_tag

pytestmark = pytest.mark.gpu

# (mode, key_bits, L, A, T)
SHAPES = [("ecb", 128, 16, 0, 1), ("ecb", 128, 16, 0, 2), ("ecb", 256, 32, 0, 2), ("cbc", 192, 32, 0, 1), ("ctr", 128, 17, 0, 1), ("gcm", 256, 17, 5, 1)]
_keys, _mats = {}, {}


@pytest.fixture(scope="module")
def kt_key(api):
    """(pk, vk) for (mode, key_bits, L, A, T) over an SRS sized from the circuit's own counts, no window tables; one per shape for the module"""
    def get(mode, key_bits, length, alen, blocks):
        shape = (mode, key_bits, length, alen, blocks)
        if shape not in _keys:
            ci = api.circuit_info(kind_of(api, mode), length, alen, key_bits=key_bits, key_tag_blocks=blocks)
            srs = (int(ci["constraints"]), int(ci["instance"]), int(ci["nnz_a"] + ci["nnz_b"] + ci["nnz_c"]))
            if mode == "gcm":
                _keys[shape] = api.synthesize_keys_gcm(length, alen, srs=srs, flags=api.KEY_NO_TABLES, key_bits=key_bits, key_tag_blocks=blocks)
            else:
                _keys[shape] = api.synthesize_keys(length, circuit=kind_of(api, mode), srs=srs, flags=api.KEY_NO_TABLES, key_bits=key_bits, key_tag_blocks=blocks)
            assert _keys[shape][0].key_tag_blocks() == blocks
        return _keys[shape]
    yield get
    for pk, _ in _keys.values():
        pk.free()
    _keys.clear()
    _mats.clear()


def unsatisfied_rows(api, shape, z):
    """indices of the rows where (A z) * (B z) != C z, in int64 (coefficients are small integers, z is 0/1)"""
    mode, key_bits, length, alen, blocks = shape
    if shape not in _mats:
        _mats[shape] = [api.circuit_matrix(kind_of(api, mode), length, which, alen, key_bits=key_bits, key_tag_blocks=blocks) for which in range(3)]
    zz = np.frombuffer(z, dtype=np.uint8).astype(np.int64)
    prods = []
    for rowptr, col, coeff in _mats[shape]:
        assert len(zz) == len(rowptr) - 1                                    # square after padding
        cs = np.concatenate([[0], np.cumsum(coeff * zz[col])])
        prods.append(cs[rowptr[1:].astype(np.int64)] - cs[rowptr[:-1].astype(np.int64)])
    return np.nonzero(prods[0] * prods[1] != prods[2])[0]


def ids(shape):
    return "%s%d-L%d-A%d-T%d" % shape


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_witness_and_trace(api, kt_key, shape):
    """the witness satisfies every row of the tagged circuit, its instance is One, the mode's public bits from the model, then the bits of the model's tag; the tag slots of
    the trace hold D_t, D_t ^ key and S_Nr = the tag at key_tag_off + t strides; the bytes ahead of them are the untagged key's trace for the same inputs"""
    mode, key_bits, length, alen, blocks = shape
    base = shape[:4]
    pk, _ = kt_key(*shape)
    plain_pk, _ = kt_key(*base, 0)
    info, plain_info = pk.info(), plain_pk.info()
    assert (pk.key_tag_blocks(), plain_pk.key_tag_blocks()) == (blocks, 0)
    assert info["raw_instance"] == plain_info["raw_instance"] + 128 * blocks
    lay = layout(key_bits // 32)
    nr = key_bits // 32 + 6
    for seed in (0x7A6 + length, 0x7A7 + key_bits):
        msg, key, header, extra = statement(base, seed)
        want_tag = model_key_tag(key, blocks)
        assert api.key_tag(key, blocks) == want_tag
        z = witness(pk, shape, msg, key, extra)
        tr = pk.debug_fetch("trace")
        assert len(z) == info["instance"] + info["witness"] and set(z) <= {0, 1}
        public = header + model_public(base, msg, key, extra)
        assert 1 + 8 * len(public) + 128 * blocks == info["raw_instance"]
        assert z[0] == 1
        assert z[1:1 + 8 * len(public)] == bits(public)                      # the mode's own public bits: where they were
        assert z[1 + 8 * len(public):info["raw_instance"]] == bits(want_tag)  # the instance tail
        assert not any(z[info["raw_instance"]:info["instance"]])
        bad = unsatisfied_rows(api, shape, z)
        assert len(bad) == 0, bad[:10]
        zf = bytearray(z)                                                    # the checker itself can fail: one tag bit flipped is one equality row
        zf[info["raw_instance"] - 3] ^= 1
        assert len(unsatisfied_rows(api, shape, bytes(zf))) == 1
        # ---- the trace
        plain_z = witness(plain_pk, base, msg, key, extra)                    # (checked by its own suites; run here for its trace and its public bits)
        assert plain_z[:1 + 8 * len(public)] == z[:1 + 8 * len(public)]
        plain_tr = plain_pk.debug_fetch("trace")
        off = (len(plain_tr) + 15) // 16 * 16
        assert len(tr) == off + blocks * lay["stride"] and len(tr) % 16 == 0
        assert tr[:len(plain_tr)] == plain_tr
        for t in range(blocks):
            slot = tr[off + t * lay["stride"]:off + (t + 1) * lay["stride"]]
            assert slot[:16] == D[t]
            assert slot[16:32] == bytes(d ^ k for d, k in zip(D[t], key[:16]))
            assert slot[16 + 16 * nr:32 + 16 * nr] == want_tag[16 * t:16 * t + 16]
    if shape[:3] == ("ecb", 128, 16):
        assert off == 272 + 1072
    if shape[:3] == ("ecb", 256, 32):
        assert off == 376 + 2 * 1520 + 8                                     # the blocks end 8 mod 16


def other_key(key):
    return bytes([key[0] ^ 0x80]) + key[1:]


def test_lone_proof_ecb_two_tag_blocks(api, kt_key):
    shape = ("ecb", 128, 16, 0, 2)
    pk, vk = kt_key(*shape)
    msg, key, _, _ = statement(shape[:4], 0xE2)
    proof = api.encrypt(msg, key, pk)
    ct, tag = ks_ecb(msg, key), api.key_tag(key, 2)
    assert tag == model_key_tag(key, 2)
    check = lambda c, t: api.verify_chunked_tagged(vk, api.CIRCUIT_AES, [proof], c, t)
    assert check(ct, tag) == [True]
    assert check(ct, flip(tag, 31)) == [False] and check(ct, flip(tag, 0, 0x01)) == [False]          # a bit of either tag block
    assert check(ct, api.key_tag(other_key(key), 2)) == [False]
    assert check(flip(ct, 15), tag) == [False]
    with pytest.raises(api.ZkAesError):                                                             # one tag block for a T = 2 key: the key tells, the call raises
        check(ct, tag[:16])


def test_lone_proof_ctr_ragged(api, kt_key):
    shape = ("ctr", 128, 17, 0, 1)
    pk, vk = kt_key(*shape)
    msg, key, icb, _ = statement(shape[:4], 0xC7)
    ct, proof = api.encrypt_ctr(msg, key, icb, pk)
    assert ct == ks_ctr(msg, key, icb)
    tag = api.key_tag(key, 1)
    check = lambda c, t, i=icb: api.verify_chunked_tagged(vk, api.CIRCUIT_AES_CTR, [proof], c, t, iv=i)
    assert check(ct, tag) == [True]
    assert check(ct, flip(tag, 7)) == [False]
    assert check(ct, api.key_tag(other_key(key), 1)) == [False]
    assert check(flip(ct, 16), tag) == [False]                                                      # in the partial block's only byte
    assert check(ct, tag, b"\xff" * 16) == [False]
    with pytest.raises(api.ZkAesError):
        check(ct, api.key_tag(key, 2))                                                              # key_tag_len 32 for a T = 1 key
    with pytest.raises(api.ZkAesError):
        check(ct[:16], tag)                                                                         # the length is part of the statement


def test_lone_proof_gcm(api, kt_key):
    shape = ("gcm", 256, 17, 5, 1)
    pk, vk = kt_key(*shape)
    msg, key, _, (iv, aad) = statement(shape[:4], 0x6C)
    ct, gtag, proof = api.encrypt_gcm(msg, key, iv, aad, pk)
    assert (ct, gtag) == ks_gcm(msg, key, iv, aad)
    tag = api.key_tag(key, 1)
    check = lambda c=ct, g=gtag, t=tag: api.verify_encryption_gcm_tagged(vk, proof, iv, aad, c, g, t)
    assert check() is True
    assert check(t=flip(tag, 3)) is False
    assert check(t=api.key_tag(other_key(key), 1)) is False
    assert check(c=flip(ct, 16)) is False
    assert check(g=flip(gtag, 9)) is False
    with pytest.raises(api.ZkAesError):
        check(t=api.key_tag(key, 2))


def test_the_splice_ecb(api, kt_key):
    """three 16-byte chunks proven under the keys (K, K', K): without key tags every chunk-proof verifies -- today's gap, asserted -- and with them one tag tells which
    chunks were made under which key"""
    rs = np.random.RandomState(0x5911CE)
    msg, k1, k2 = rs.bytes(48), rs.bytes(16), rs.bytes(16)
    chunks, keys = [msg[16 * j:16 * j + 16] for j in range(3)], [k1, k2, k1]
    ct = b"".join(ks_ecb(m, k) for m, k in zip(chunks, keys))
    seed = bytes(range(32))
    plain_pk, plain_vk = kt_key("ecb", 128, 16, 0, 0)
    pk, vk = kt_key("ecb", 128, 16, 0, 1)
    for key_pair in (plain_pk, pk):
        key_pair.set_contexts(2)
    try:
        loose = plain_pk.encrypt_batch(chunks, keys, zk_seed=seed)
        assert [api.verify_encryption(plain_vk, loose[j], ct[16 * j:16 * j + 16]) for j in range(3)] == [True, True, True]      # the gap: nothing tells the keys differ
        proofs = pk.encrypt_batch(chunks, keys, zk_seed=seed)
        assert api.verify_chunked_tagged(vk, api.CIRCUIT_AES, proofs, ct, api.key_tag(k1, 1)) == [True, False, True]
        assert api.verify_chunked_tagged(vk, api.CIRCUIT_AES, proofs, ct, api.key_tag(k2, 1)) == [False, True, False]
        # the honest job: one key, every chunk under its tag; a call split by first_proof_index reproduces the same proof bytes
        honest = pk.encrypt_chunked(msg, k1, zk_seed=seed)
        assert api.verify_chunked_tagged(vk, api.CIRCUIT_AES, honest, ks_ecb(msg, k1), api.key_tag(k1, 1)) == [True, True, True]
        assert honest[0] == proofs[0] and honest[2] == proofs[2] and honest[1] != proofs[1]
        assert pk.encrypt_chunked(msg[:16], k1, zk_seed=seed) + pk.encrypt_chunked(msg[16:], k1, zk_seed=seed, first_proof_index=1) == honest
    finally:
        for key_pair in (plain_pk, pk):
            key_pair.set_contexts(0)


def test_the_splice_ctr(api, kt_key):
    """three 16-byte CTR chunks; chunk 1 is made under another key by a seek to its counter.  Also: the seek into chunk 2 reproduces the job's own proof, and swapped
    chunks are rejected"""
    rs = np.random.RandomState(0x5911C7)
    msg, k1, k2, icb = rs.bytes(48), rs.bytes(16), rs.bytes(16), b"\xff" * 15 + b"\xfe"               # the counter wraps inside the job
    seed = bytes(range(1, 33))
    for blocks in (0, 1):
        pk, vk = kt_key("ctr", 128, 16, 0, blocks)
        ct, proofs = pk.encrypt_ctr_chunked(msg, k1, icb, zk_seed=seed)
        assert ct == ks_ctr(msg, k1, icb)
        ct_mid, mid = pk.encrypt_ctr_chunked(msg[16:32], k2, api.ctr_counter_add(icb, 1), zk_seed=seed, first_proof_index=1)
        assert ct_mid == ks_ctr(msg, k2, icb)[16:32]
        spliced_ct, spliced = ct[:16] + ct_mid + ct[32:], [proofs[0], mid[0], proofs[2]]
        if blocks == 0:
            assert api.verify_ctr_chunked(vk, spliced, icb, spliced_ct) == [True, True, True]       # the gap
            continue
        check = lambda p, c, k: api.verify_chunked_tagged(vk, api.CIRCUIT_AES_CTR, p, c, api.key_tag(k, 1), iv=icb)
        assert check(proofs, ct, k1) == [True, True, True]
        assert check(spliced, spliced_ct, k1) == [True, False, True]
        assert check(spliced, spliced_ct, k2) == [False, True, False]
        ct_tail, tail = pk.encrypt_ctr_chunked(msg[32:], k1, api.ctr_counter_add(icb, 2), zk_seed=seed, first_proof_index=2)      # a seek into chunk 2
        assert ct_tail == ct[32:] and tail == proofs[2:]
        assert check([proofs[1], proofs[0], proofs[2]], ct, k1) == [False, False, True]
        assert api.verify_chunked_tagged(vk, api.CIRCUIT_AES_CTR, [proofs[2]], ct[32:], api.key_tag(k1, 1), iv=api.ctr_counter_add(icb, 2)) == [True]      # any chunk alone, from (icb, j)


def test_the_splice_cbc(api, kt_key):
    """three 32-byte CBC-192 chunks; chunk 1 is made under another key from the public chaining value, chunk 2 goes on from the spliced ciphertext"""
    rs = np.random.RandomState(0x5911CB)
    msg, k1, k2, iv = rs.bytes(96), rs.bytes(24), rs.bytes(24), rs.bytes(16)
    seed = bytes(range(2, 34))
    for blocks in (0, 1):
        pk, vk = kt_key("cbc", 192, 32, 0, blocks)
        ct, proofs = pk.encrypt_cbc_chunked(msg, k1, iv, zk_seed=seed)
        assert ct == ks_cbc(msg, k1, iv) and len(proofs) == 3
        ct_mid, mid = pk.encrypt_cbc_chunked(msg[32:64], k2, ct[16:32], zk_seed=seed, first_proof_index=1)
        ct_tail, tail = pk.encrypt_cbc_chunked(msg[64:], k1, ct_mid[16:], zk_seed=seed, first_proof_index=2)
        spliced_ct, spliced = ct[:32] + ct_mid + ct_tail, [proofs[0], mid[0], tail[0]]
        if blocks == 0:
            assert api.verify_cbc_chunked(vk, spliced, iv, spliced_ct) == [True, True, True]        # the gap
            continue
        check = lambda p, c, k: api.verify_chunked_tagged(vk, api.CIRCUIT_AES_CBC, p, c, api.key_tag(k, 1), iv=iv)
        assert check(proofs, ct, k1) == [True, True, True]
        assert check(spliced, spliced_ct, k1) == [True, False, True]
        assert check(spliced, spliced_ct, k2) == [False, True, False]
        assert pk.encrypt_cbc_chunked(msg[32:], k1, ct[16:32], zk_seed=seed, first_proof_index=1)[1] == proofs[1:]      # the seeded split call


def test_gcm_batch_against_one_tag(api, kt_key):
    shape = ("gcm", 256, 17, 5, 1)
    pk, vk = kt_key(*shape)
    recs = [statement(shape[:4], 0xBA7 + i) for i in range(3)]
    session, intruder = recs[0][1], recs[2][1]
    msgs, keys = [r[0] for r in recs], [session, session, intruder]
    ivs, aads = [r[3][0] for r in recs], [r[3][1] for r in recs]
    pk.set_contexts(2)
    try:
        cts, tags, proofs = pk.encrypt_gcm_batch(msgs, keys, ivs, aads, zk_seed=bytes(range(32)))
    finally:
        pk.set_contexts(0)
    for i in range(3):
        assert (cts[i], tags[i]) == ks_gcm(msgs[i], keys[i], ivs[i], aads[i])
    under = lambda tag: [api.verify_encryption_gcm_tagged(vk, proofs[i], ivs[i], aads[i], cts[i], tags[i], tag) for i in range(3)]
    assert under(api.key_tag(session, 1)) == [True, True, False]
    assert under(api.key_tag(intruder, 1)) == [False, False, True]


def never_accepts(call):
    try:
        got = call()
    except Exception as e:                                                                          # ZkAesError: a refusal
        assert type(e).__name__ == "ZkAesError"
        return True
    return got in (False, [False])


def test_tagged_and_untagged_do_not_mix(api, kt_key):
    rs = np.random.RandomState(0x313)
    msg, key = rs.bytes(16), rs.bytes(16)
    ct = ks_ecb(msg, key)
    plain_pk, plain_vk = kt_key("ecb", 128, 16, 0, 0)
    for blocks in (1, 2):
        pk, vk = kt_key("ecb", 128, 16, 0, blocks)
        tag = api.key_tag(key, blocks)
        tagged, plain = api.encrypt(msg, key, pk), api.encrypt(msg, key, plain_pk)
        assert api.verify_chunked_tagged(vk, api.CIRCUIT_AES, [tagged], ct, tag) == [True] and api.verify_encryption(plain_vk, plain, ct) is True
        assert never_accepts(lambda: api.verify_encryption(vk, tagged, ct))                          # tagged proof, untagged verifier, either key
        assert never_accepts(lambda: api.verify_encryption(plain_vk, tagged, ct))
        assert never_accepts(lambda: api.verify_chunked_tagged(vk, api.CIRCUIT_AES, [plain], ct, tag))          # untagged proof, tagged verifier, either key
        assert never_accepts(lambda: api.verify_chunked_tagged(plain_vk, api.CIRCUIT_AES, [plain], ct, tag))
        assert never_accepts(lambda: api.verify_chunked_tagged(plain_vk, api.CIRCUIT_AES, [tagged], ct, tag))
    # the other modes' untagged verifiers with a tagged key
    pk, vk = kt_key("ctr", 128, 17, 0, 1)
    m17, icb = rs.bytes(17), rs.bytes(16)
    c17, p17 = api.encrypt_ctr(m17, key, icb, pk)
    assert never_accepts(lambda: api.verify_encryption_ctr(vk, p17, icb, c17))
    pk, vk = kt_key("gcm", 256, 17, 5, 1)
    k32, iv, aad = rs.bytes(32), rs.bytes(12), rs.bytes(5)
    cg, tg, pg = api.encrypt_gcm(m17, k32, iv, aad, pk)
    assert never_accepts(lambda: api.verify_encryption_gcm(vk, pg, iv, aad, cg, tg))


def test_untagged_proof_bytes_do_not_move(api, kt_key, vectors):
    """with tagged keys alive in the process, an untagged AES-128 ECB key over the default SRS literals still emits the committed proof bytes under the reference's fixed
    prover seed"""
    kt_key("ecb", 128, 16, 0, 1)
    pk, vk = api.synthesize_keys(16, flags=api.KEY_NO_TABLES)
    try:
        assert pk.key_tag_blocks() == 0
        proof = api.encrypt(bytes(vectors["plaintext"]), bytes(vectors["key"]), pk, zk_seed=None)  # (None = the reference's fixed prover stream: byte parity)
        gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
        assert proof == open(os.path.join(gold, "gpu_aes16_proof.bin"), "rb").read()
        assert vk.to_bytes() == open(os.path.join(gold, "gpu_aes16_vk.bin"), "rb").read()
    finally:
        pk.free()
