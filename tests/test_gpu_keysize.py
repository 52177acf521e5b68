"""AES-192 and AES-256 proving on the GPU: the trace kernels' NK = 6 and 8 instantiations, the witness against the circuit's own matrices, lone, chunked and batch
proofs in every mode, AES-128 unchanged.

There is no upstream circuit for these key sizes and no oracle, so nothing here is byte parity with a reference.  Correctness rests on the pure-Python model of
test_keysize_host.py (checked there against FIPS-197 appendix C, SP 800-38A and the McGrew-Viega vectors) and a row-by-row check of (A z) o (B z) = C z in int64 numpy
over the matrices zkaes_circuit_matrix_ks returns.  The shapes are the smallest where a kernel can go wrong: one block (the schedule lane and one block lane), two
blocks (a second block lane at the new stride), a CBC lane that re-walks one block, a CTR counter that wraps, and the two GCM shapes whose GHASH lanes read H and the
tag mask at the new offsets.  Every key is synthesized over an SRS sized from its own circuit, without window tables, once per module.
"""
import ctypes as C

import numpy as np
import pytest

from test_keysize_host import FIPS, FIPS_PT, INSTANCES, expand_key, ks_cbc, ks_ctr, ks_ecb, ks_gcm
from test_cbc_host import SBOX

pytestmark = pytest.mark.gpu

ICB_FE = b"\xff" * 15 + b"\xfe"                                             # wraps at the second increment
ICB_ONES = b"\xff" * 16


def bits(data):
    """8 LSB-first bits per byte, one byte (0/1) each: the public-input encoding"""
    return bytes((b >> i) & 1 for b in data for i in range(8))


def layout(nk):
    """csrc/trace_layout.h TRK_*: offsets of the schedule words, the SubWord bytes, the words ahead of the Rcon xor, the first block; the block stride"""
    nr, inst = nk + 6, INSTANCES[nk]
    ks_w = 4 * nk
    ks_sub = ks_w + 16 * (nr + 1)
    ks_pre = ks_sub + 4 * inst
    return dict(ks_w=ks_w, ks_sub=ks_sub, ks_pre=ks_pre, block0=ks_pre + 4 * inst, stride=112 * nr - 48, s=16)


def kind_of(api, mode):
    return {"ecb": api.CIRCUIT_AES, "cbc": api.CIRCUIT_AES_CBC, "ctr": api.CIRCUIT_AES_CTR, "gcm": api.CIRCUIT_AES_GCM}[mode]


def small_srs(api, mode, key_bits, length, alen=0):
    ci = api.circuit_info(kind_of(api, mode), length, alen, key_bits=key_bits)
    return (int(ci["constraints"]), int(ci["instance"]), int(ci["nnz_a"] + ci["nnz_b"] + ci["nnz_c"]))


_keys = {}


@pytest.fixture(scope="module")
def ks_key(api):
    """(pk, vk) for (mode, key_bits, L, A) over an SRS sized from the circuit's own counts, no window tables; one per shape for the module"""
    def get(mode, key_bits, length, alen=0):
        shape = (mode, key_bits, length, alen)
        if shape not in _keys:
            srs = small_srs(api, mode, key_bits, length, alen)
            if mode == "gcm":
                _keys[shape] = api.synthesize_keys_gcm(length, alen, srs=srs, flags=api.KEY_NO_TABLES, key_bits=key_bits)
            else:
                _keys[shape] = api.synthesize_keys(length, circuit=kind_of(api, mode), srs=srs, flags=api.KEY_NO_TABLES, key_bits=key_bits)
        return _keys[shape]
    yield get
    for pk, _ in _keys.values():
        pk.free()
    _keys.clear()


_mats = {}


def unsatisfied_rows(api, shape, z):
    """indices of the rows where (A z) * (B z) != C z, in int64 (coefficients are small integers, z is 0/1)"""
    mode, key_bits, length, alen = shape
    if shape not in _mats:
        _mats[shape] = [api.circuit_matrix(kind_of(api, mode), length, which, alen, key_bits=key_bits) for which in range(3)]
    zz = np.frombuffer(z, dtype=np.uint8).astype(np.int64)
    prods = []
    for rowptr, col, coeff in _mats[shape]:
        assert len(zz) == len(rowptr) - 1                                    # square after padding
        cs = np.concatenate([[0], np.cumsum(coeff * zz[col])])
        prods.append(cs[rowptr[1:].astype(np.int64)] - cs[rowptr[:-1].astype(np.int64)])
    return np.nonzero(prods[0] * prods[1] != prods[2])[0]


SHAPES = [("ecb", 256, 16, 0), ("ecb", 256, 32, 0), ("ecb", 192, 16, 0), ("cbc", 256, 32, 0), ("ctr", 256, 17, 0), ("gcm", 256, 1, 0), ("gcm", 256, 17, 5)]


def statement(shape, seed):
    """(message, key, public bytes ahead of the ciphertext, (iv / icb, aad)) of a random statement of this shape; CTR runs under ff..fe"""
    mode, key_bits, length, alen = shape
    rs = np.random.RandomState(seed)
    msg, key = rs.bytes(length), rs.bytes(key_bits // 8)
    if mode == "ecb":
        return msg, key, b"", ()
    if mode == "cbc":
        iv = rs.bytes(16)
        return msg, key, iv, (iv,)
    if mode == "ctr":
        return msg, key, ICB_FE, (ICB_FE,)
    iv, aad = rs.bytes(12), rs.bytes(alen)
    return msg, key, iv + aad, (iv, aad)


def model_public(shape, msg, key, extra):
    """the public bytes behind the header, from the model: the ciphertext (and, for GCM, the tag)"""
    mode = shape[0]
    if mode == "ecb":
        return ks_ecb(msg, key)
    if mode == "cbc":
        return ks_cbc(msg, key, extra[0])
    if mode == "ctr":
        return ks_ctr(msg, key, extra[0])
    ct, tag = ks_gcm(msg, key, extra[0], extra[1])
    return ct + tag


def witness(pk, shape, msg, key, extra):
    mode = shape[0]
    if mode == "ecb":
        return pk.witness(msg, key)
    if mode == "cbc":
        return pk.witness_cbc(msg, key, extra[0])
    if mode == "ctr":
        return pk.witness_ctr(msg, key, extra[0])
    return pk.witness_gcm(msg, key, extra[0], extra[1])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%s%d-L%d-A%d" % s)
def test_witness_satisfies_every_constraint(api, ks_key, shape):
    mode, key_bits, length, alen = shape
    pk, _ = ks_key(*shape)
    info = pk.info()
    assert pk.key_bytes() == key_bits // 8
    for seed in (0x4B5 + length, 0x4B6 + key_bits):
        msg, key, header, extra = statement(shape, seed)
        z = witness(pk, shape, msg, key, extra)
        assert len(z) == info["instance"] + info["witness"] and set(z) <= {0, 1}
        public = header + model_public(shape, msg, key, extra)
        assert 1 + 8 * len(public) == info["raw_instance"]
        assert z[0] == 1
        assert z[1:1 + 8 * len(public)] == bits(public)
        assert not any(z[1 + 8 * len(public):info["instance"]])              # the instance padding
        bad = unsatisfied_rows(api, shape, z)
        assert len(bad) == 0, bad[:10]
        # the checker itself can fail: a bit of the last ciphertext byte of the instance flipped
        zf = bytearray(z)
        zf[1 + 8 * len(header) + 8 * (length - 1) + 4] ^= 1
        assert len(unsatisfied_rows(api, shape, bytes(zf))) >= 1


def test_trace_of_the_fips_vector_aes256(api, ks_key):
    """after one ECB-256 proof of FIPS-197 C.3: the trace has the length the layout gives, S_0 = M ^ key[0:16], S_14 is the published ciphertext, W_59 and the 13
    SubWord instances (bytes and the words ahead of the Rcon xor) are the model's"""
    nk, nr = 8, 14
    pk, vk = ks_key("ecb", 256, 16)
    key, want = bytes(range(32)), bytes.fromhex(FIPS[32])
    proof = api.encrypt(FIPS_PT, key, pk)
    assert api.verify_encryption(vk, proof, want) is True
    lay = layout(nk)
    assert (lay["ks_w"], lay["ks_sub"], lay["ks_pre"], lay["block0"], lay["stride"]) == (32, 272, 324, 376, 1520)
    tr = pk.debug_fetch("trace")
    assert len(tr) == lay["block0"] + lay["stride"]
    assert tr[:32] == key
    base = lay["block0"]
    assert tr[base:base + 16] == FIPS_PT
    assert tr[base + 16:base + 32] == bytes(m ^ k for m, k in zip(FIPS_PT, key[:16]))
    assert tr[base + 16 + 16 * nr:base + 32 + 16 * nr] == want
    w, rks = expand_key(key)
    assert len(w) == 60
    for i in range(60):
        assert tr[lay["ks_w"] + 4 * i:lay["ks_w"] + 4 * i + 4] == bytes(w[i]), i
    assert tr[lay["ks_w"] + 4 * 59:lay["ks_w"] + 4 * 60] == bytes(w[59])
    seen = 0
    for i in range(8, 60):
        if i % 8 == 0:
            sub = [SBOX[w[i - 1][(k + 1) % 4]] for k in range(4)]
        elif i % 8 == 4:
            sub = [SBOX[v] for v in w[i - 1]]
        else:
            continue
        q = i // 4 - 2
        assert q == seen
        pre = [a ^ b for a, b in zip(w[i - 8], sub)]
        assert tr[lay["ks_sub"] + 4 * q:lay["ks_sub"] + 4 * q + 4] == bytes(sub), i
        assert tr[lay["ks_pre"] + 4 * q:lay["ks_pre"] + 4 * q + 4] == bytes(pre), i
        if i % 8 == 4:
            assert bytes(pre) == bytes(w[i])                                  # no Rcon on these: the word ahead of the xor is W_i itself
        seen += 1
    assert seen == 13
    # the S-box outputs of round 1 sit behind the 15 states
    sb1 = base + 16 + 16 * (nr + 1)
    assert tr[sb1:sb1 + 16] == bytes(SBOX[v] for v in tr[base + 16:base + 32])


def flip(data, at, mask=0x10):
    out = bytearray(data)
    out[at] ^= mask
    return bytes(out)


def test_lone_proofs_ecb(api, ks_key):
    for key_bits in (256, 192):
        shape = ("ecb", key_bits, 16, 0)
        pk, vk = ks_key(*shape)
        msg, key, _, _ = statement(shape, 0xE0 + key_bits)
        proof = api.encrypt(msg, key, pk)
        ct = ks_ecb(msg, key)
        assert ct == api.ecb_ciphertext(msg, key)
        assert api.verify_encryption(vk, proof, ct) is True
        assert api.verify_encryption(vk, proof, flip(ct, 15)) is False
        assert api.verify_encryption(vk, proof, ks_ecb(msg, key[:16])) is False          # the AES-128 encryption under the key's first half


def test_lone_proof_cbc(api, ks_key):
    shape = ("cbc", 256, 32, 0)
    pk, vk = ks_key(*shape)
    msg, key, iv, _ = statement(shape, 0xCBC)
    ct, proof = api.encrypt_cbc(msg, key, iv, pk)
    assert ct == ks_cbc(msg, key, iv)
    assert api.verify_encryption_cbc(vk, proof, iv, ct) is True
    assert api.verify_encryption_cbc(vk, proof, iv, flip(ct, 31)) is False
    assert api.verify_encryption_cbc(vk, proof, flip(iv, 0), ct) is False


def test_lone_proof_ctr(api, ks_key):
    shape = ("ctr", 256, 17, 0)
    pk, vk = ks_key(*shape)
    msg, key, icb, _ = statement(shape, 0xC72)
    ct, proof = api.encrypt_ctr(msg, key, icb, pk)
    assert ct == ks_ctr(msg, key, icb) and ct == api.ctr_crypt(msg, key, icb)
    assert api.verify_encryption_ctr(vk, proof, icb, ct) is True
    assert api.verify_encryption_ctr(vk, proof, icb, flip(ct, 16)) is False              # in the partial block's only byte
    assert api.verify_encryption_ctr(vk, proof, ICB_ONES, ct) is False


@pytest.mark.parametrize("shape", [("gcm", 256, 1, 0), ("gcm", 256, 17, 5)], ids=lambda s: "L%d-A%d" % s[2:])
def test_lone_proof_gcm(api, ks_key, shape):
    pk, vk = ks_key(*shape)
    msg, key, _, (iv, aad) = statement(shape, 0x6C + shape[2])
    ct, tag, proof = api.encrypt_gcm(msg, key, iv, aad, pk)
    assert (ct, tag) == ks_gcm(msg, key, iv, aad) == api.gcm_encrypt(msg, key, iv, aad)
    assert api.verify_encryption_gcm(vk, proof, iv, aad, ct, tag) is True
    assert api.verify_encryption_gcm(vk, proof, iv, aad, flip(ct, len(ct) - 1), tag) is False
    assert api.verify_encryption_gcm(vk, proof, iv, aad, ct, flip(tag, 7)) is False
    assert api.verify_encryption_gcm(vk, proof, flip(iv, 11), aad, ct, tag) is False


def test_chunked_ecb_and_ctr(api, ks_key):
    """two 16-byte chunks each; the CTR job starts at ff..ff, so the counter wraps to zero between the chunks"""
    rs = np.random.RandomState(0xC4)
    msg, key = rs.bytes(32), rs.bytes(32)
    pk, vk = ks_key("ecb", 256, 16)
    proofs = pk.encrypt_chunked(msg, key, zk_seed=bytes(32))
    ct = ks_ecb(msg, key)
    assert len(proofs) == 2
    for j in range(2):
        assert api.verify_encryption(vk, proofs[j], ct[16 * j:16 * j + 16]) is True
        assert api.verify_encryption(vk, proofs[j], ct[16 * (1 - j):16 * (1 - j) + 16]) is False
    pk, vk = ks_key("ctr", 256, 16)
    ct, proofs = pk.encrypt_ctr_chunked(msg, key, ICB_ONES, zk_seed=bytes(32))
    assert ct == ks_ctr(msg, key, ICB_ONES) and len(proofs) == 2
    assert api.verify_ctr_chunked(vk, proofs, ICB_ONES, ct) == [True, True]
    assert api.verify_encryption_ctr(vk, proofs[0], ICB_ONES, ct[:16]) is True
    assert api.verify_encryption_ctr(vk, proofs[1], bytes(16), ct[16:]) is True          # chunk 1 under the wrapped counter, from (icb, 1) alone
    assert api.verify_encryption_ctr(vk, proofs[1], ICB_ONES, ct[16:]) is False
    assert api.verify_ctr_chunked(vk, proofs[::-1], ICB_ONES, ct) == [False, False]


def test_gcm_batch_two_records_two_keys(api, ks_key):
    shape = ("gcm", 256, 17, 5)
    pk, vk = ks_key(*shape)
    recs = [statement(shape, 0xBA7 + i) for i in range(2)]
    msgs, keys = [r[0] for r in recs], [r[1] for r in recs]
    ivs, aads = [r[3][0] for r in recs], [r[3][1] for r in recs]
    assert keys[0] != keys[1] and len(keys[0]) == 32
    pk.set_contexts(2)
    try:
        cts, tags, proofs = pk.encrypt_gcm_batch(msgs, keys, ivs, aads, zk_seed=bytes(range(32)))
    finally:
        pk.set_contexts(0)
    for i in range(2):
        assert (cts[i], tags[i]) == ks_gcm(msgs[i], keys[i], ivs[i], aads[i])
        assert api.verify_encryption_gcm(vk, proofs[i], ivs[i], aads[i], cts[i], tags[i]) is True
        assert api.verify_encryption_gcm(vk, proofs[i], ivs[1 - i], aads[1 - i], cts[1 - i], tags[1 - i]) is False
    with pytest.raises(api.ZkAesError):                                      # keys at the AES-128 stride
        pk.encrypt_gcm_batch(msgs, [k[:16] for k in keys], ivs, aads, zk_seed=bytes(32))


def old_synthesize(api, length, srs):
    """a key through the entry point that predates the key-size argument"""
    pk, vk = C.c_void_p(), C.c_void_p()
    rc = api.lib().zkaes_synthesize_keys_ex2(api.CIRCUIT_AES, C.c_size_t(length), C.c_size_t(srs[0]), C.c_size_t(srs[1]), C.c_size_t(srs[2]), C.c_uint(api.KEY_NO_TABLES), C.byref(pk), C.byref(vk))
    assert rc == 0, api.lib().zkaes_last_error()
    return api.ProvingKey(pk.value), api.VerifyingKey(vk.value)


def test_aes128_unchanged_and_key_sizes_do_not_mix(api, ks_key):
    srs = small_srs(api, "ecb", 128, 16)
    msg, key = FIPS_PT, bytes(range(16))
    made = [api.synthesize_keys(16, srs=srs, flags=api.KEY_NO_TABLES, key_bits=128), api.synthesize_keys(16, srs=srs, flags=api.KEY_NO_TABLES), old_synthesize(api, 16, srs)]
    try:
        proofs = [api.encrypt(msg, key, pk, zk_seed=None) for pk, _ in made]               # (None = the reference's fixed prover stream: byte parity)
        assert proofs[0] == proofs[1] == proofs[2]
        assert [pk.key_bytes() for pk, _ in made] == [16, 16, 16]
        assert made[0][1].to_bytes() == made[1][1].to_bytes() == made[2][1].to_bytes()
        vk128 = made[0][1]
        assert api.verify_encryption(vk128, proofs[0], bytes.fromhex(FIPS[16])) is True
        tr = made[0][0].debug_fetch("trace")
        assert len(tr) == 272 + 1072 and tr[272 + 16 + 160:272 + 16 + 176] == bytes.fromhex(FIPS[16])
        # a proof under the 256-bit key of the same length: its own key takes it, the 128-bit key does not (same public-input shape, another relation)
        pk256, vk256 = ks_key("ecb", 256, 16)
        key256 = bytes(range(32))
        proof256 = api.encrypt(msg, key256, pk256)
        ct256 = bytes.fromhex(FIPS[32])
        assert api.verify_encryption(vk256, proof256, ct256) is True
        assert api.verify_encryption(vk128, proof256, ct256) is False
        assert api.verify_encryption(vk256, proofs[0], bytes.fromhex(FIPS[16])) is False
    finally:
        for pk, _ in made:
            pk.free()


def test_refusals(api, ks_key):
    pk, _ = ks_key("ecb", 256, 16)
    assert pk.key_bytes() == 32
    for call in (lambda: api.encrypt(bytes(16), bytes(16), pk), lambda: pk.witness(bytes(16), bytes(16)), lambda: pk.encrypt_chunked(bytes(16), bytes(24), zk_seed=bytes(32)),
                 lambda: pk.encrypt_batch([bytes(16)], [bytes(16)], zk_seed=bytes(32))):
        with pytest.raises(api.ZkAesError, match="secret_key must be 32 bytes"):
            call()
    pk_cbc, _ = ks_key("cbc", 256, 32)
    with pytest.raises(api.ZkAesError, match="secret_key must be 32 bytes"):
        api.encrypt_cbc(bytes(32), bytes(16), bytes(16), pk_cbc)
    pk_gcm, _ = ks_key("gcm", 256, 1, 0)
    with pytest.raises(api.ZkAesError, match="secret_key must be 32 bytes"):
        api.encrypt_gcm(b"x", bytes(16), bytes(12), b"", pk_gcm)
    # the checked batch call counts key bytes by the key's size at the C boundary too
    out, total = C.c_void_p(), C.c_size_t()
    lens = (C.c_size_t * 1)()
    rc = api.lib().zkaes_encrypt_batch_seeded_at(C.c_size_t(1), bytes(16), C.c_size_t(16), bytes(16), C.c_size_t(16), pk._p, bytes(32), C.c_uint64(0), C.byref(out), C.byref(total), lens)
    assert rc != 0 and b"n x 32 bytes" in api.lib().zkaes_last_error()
    # modes still refuse each other's keys, whatever the key size
    with pytest.raises(api.ZkAesError, match="not synthesized for"):
        api.encrypt_cbc(bytes(16), bytes(32), bytes(16), pk)
    with pytest.raises(api.ZkAesError):
        api.synthesize_keys(16, key_bits=100)
    with pytest.raises(api.ZkAesError):
        api.synthesize_keys(0, circuit=api.CIRCUIT_OPS_XOR, srs=(200, 200, 600), key_bits=256)
