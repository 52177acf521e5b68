"""AES-128-GCM proving on the GPU: the two GCM trace kernels, the witness against the circuit's own matrices, lone proofs, batches of records, the cross-mode refusals.

There is no upstream GCM circuit and no oracle for it, so nothing here is byte parity.  Correctness rests on the published vectors (McGrew-Viega test cases 1-4), the
pure-Python model of test_gcm_host.py (FIPS-197 block, GHASH from SP 800-38D Algorithm 1 over Python integers) and a row-by-row check of (A z) o (B z) = C z in int64
numpy over the matrices zkaes_circuit_matrix_gcm returns.  The shapes are the smallest where the kernels can go wrong: (L, A) = (1, 0), one partial block and two
multiplications; (17, 5), a partial aad block, a whole and a partial ciphertext block, four multiplications; (16, 20), two aad blocks, the second partial.  Every key but
the last test's is synthesized over an SRS sized for its own circuit, without window tables, so each test takes seconds.
"""
import numpy as np
import pytest

from test_cbc_host import model_cbc, model_ecb
from test_ctr_host import model_ctr
from test_gcm_host import TC3_CT, TC3_IV, TC3_KEY, TC3_PT, TC4_AAD, VECTORS, gf_mul, model_gcm, model_ghash_chain

pytestmark = pytest.mark.gpu

TR_BLOCK0, TR_BLOCK_STRIDE, TR_BL_S = 272, 1072, 16                        # csrc/trace_layout.h
TR_GCM_MUL_STRIDE, TR_GCM_MUL_X, TR_GCM_MUL_P, TR_GCM_MUL_Q, TR_GCM_MUL_Y = 2208, 0, 16, 2064, 2192
SHAPES = [(1, 0), (17, 5), (16, 20)]


def bits(data):
    """8 LSB-first bits per byte, one byte (0/1) each: the public-input encoding"""
    return bytes((b >> i) & 1 for b in data for i in range(8))


def small_srs(api, kind, length, alen=0):
    ci = api.circuit_info(kind, length, alen)
    return (int(ci["constraints"]), int(ci["instance"]), int(ci["nnz_a"] + ci["nnz_b"] + ci["nnz_c"]))


_keys = {}


@pytest.fixture(scope="module")
def gcm_key(api):
    """(pk, vk) for an (L, A) GCM statement over an SRS sized from the circuit's own counts, no window tables; one per shape for the module"""
    def get(length, alen):
        if (length, alen) not in _keys:
            _keys[length, alen] = api.synthesize_keys_gcm(length, alen, srs=small_srs(api, api.CIRCUIT_AES_GCM, length, alen), flags=api.KEY_NO_TABLES)
        return _keys[length, alen]
    yield get
    for pk, _ in _keys.values():
        pk.free()
    _keys.clear()


_mats = {}


def unsatisfied_rows(api, shape, z):
    """indices of the rows where (A z) * (B z) != C z, in int64 (coefficients are small integers, z is 0/1)"""
    if shape not in _mats:
        _mats[shape] = [api.circuit_matrix(api.CIRCUIT_AES_GCM, shape[0], which, shape[1]) for which in range(3)]
    zz = np.frombuffer(z, dtype=np.uint8).astype(np.int64)
    prods = []
    for rowptr, col, coeff in _mats[shape]:
        assert len(zz) == len(rowptr) - 1                                    # square after padding
        cs = np.concatenate([[0], np.cumsum(coeff * zz[col])])
        prods.append(cs[rowptr[1:].astype(np.int64)] - cs[rowptr[:-1].astype(np.int64)])
    return np.nonzero(prods[0] * prods[1] != prods[2])[0]


@pytest.mark.parametrize("shape", SHAPES)
def test_witness_satisfies_every_constraint(api, gcm_key, shape):
    length, alen = shape
    pk, _ = gcm_key(length, alen)
    info = pk.info()
    assert info["raw_instance"] == 225 + 8 * (alen + length)
    rs = np.random.RandomState(0x6C + 32 * length + alen)
    cases = [(TC3_PT[:length], TC3_KEY, TC3_IV, TC4_AAD[:alen]), (rs.bytes(length), rs.bytes(16), rs.bytes(12), rs.bytes(alen)), (bytes(length), bytes(16), rs.bytes(12), rs.bytes(alen))]
    for msg, key, iv, aad in cases:
        z = pk.witness_gcm(msg, key, iv, aad)
        assert len(z) == info["instance"] + info["witness"] and set(z) <= {0, 1}
        ct, tag = model_gcm(msg, key, iv, aad)
        public = bits(iv) + bits(aad) + bits(ct) + bits(tag)
        assert z[0] == 1 and z[1:1 + len(public)] == public
        assert len(public) + 1 == info["raw_instance"] and not any(z[1 + len(public):info["instance"]])       # the instance padding
        bad = unsatisfied_rows(api, shape, z)
        assert len(bad) == 0, bad[:10]
        # the checker itself can fail: one tag bit of the instance flipped, then one bit of the last aad byte (of the last ciphertext byte where the key has no aad)
        tag_at = 1 + 96 + 8 * (alen + length)
        for at in (tag_at + 8 * 9 + 2, 1 + 96 + 8 * alen - 3 if alen else tag_at - 3):
            zf = bytearray(z)
            zf[at] ^= 1
            assert len(unsatisfied_rows(api, shape, bytes(zf))) >= 1
    assert TC3_CT[:length] == model_gcm(*cases[0])[0]                        # (the keystream of test cases 3 and 4)


def test_trace_tail_h_v_table_chain_and_tag(api, gcm_key):
    """after one proof at (17, 5): H = AES_K(0) in S_10 of slot nb, V_1 = H alpha and V_127, every X_m, P_m column sum and Y_m against the model, q <= 64, the tag"""
    length, alen, nb, na = 17, 5, 2, 1
    n_mul = na + nb + 1
    pk, vk = gcm_key(length, alen)
    rs = np.random.RandomState(0x7A61)
    msg, key, iv, aad = rs.bytes(length), rs.bytes(16), rs.bytes(12), rs.bytes(alen)
    ct, tag, proof = api.encrypt_gcm(msg, key, iv, aad, pk)
    assert (ct, tag) == model_gcm(msg, key, iv, aad) and api.verify_encryption_gcm(vk, proof, iv, aad, ct, tag)
    tr = pk.debug_fetch("trace")
    tail = TR_BLOCK0 + (nb + 2) * TR_BLOCK_STRIDE
    v_off = tail + 16 + 16 * na + 16 * nb
    mul0 = v_off + 2048
    assert len(tr) == mul0 + n_mul * TR_GCM_MUL_STRIDE + 16
    s10 = lambda slot: tr[TR_BLOCK0 + slot * TR_BLOCK_STRIDE + TR_BL_S + 160:TR_BLOCK0 + slot * TR_BLOCK_STRIDE + TR_BL_S + 176]
    h_bytes = model_ecb(bytes(16), key)
    assert s10(nb) == h_bytes and s10(nb + 1) == model_ecb(iv + b"\0\0\0\1", key)
    assert tr[tail:tail + 16] == iv + bytes(4)
    assert tr[tail + 16:tail + 32] == aad + bytes(16 - alen)
    assert tr[tail + 32:tail + 64] == ct + bytes(32 - length)
    h = int.from_bytes(h_bytes, "big")
    v_row = lambda i: int.from_bytes(bytes(tr[v_off + 128 * j + i] for j in range(16)), "big")
    alpha = 1 << 126                                                         # the element alpha: bit 1 of the standard's numbering
    v = h
    for i in range(128):
        if i in (0, 1, 2, 64, 127):
            assert v_row(i) == v, i
        v = gf_mul(v, alpha)
    assert v_row(1) == gf_mul(h, alpha) and v_row(1) == (h >> 1) ^ (0xE1 << 120 if h & 1 else 0)
    ys = model_ghash_chain(h, aad, ct)
    assert len(ys) == n_mul
    y_prev = 0
    for m, y in enumerate(ys):
        mul = mul0 + m * TR_GCM_MUL_STRIDE
        assert int.from_bytes(tr[mul + TR_GCM_MUL_Y:mul + TR_GCM_MUL_Y + 16], "big") == y, m
        x = int.from_bytes(tr[mul + TR_GCM_MUL_X:mul + TR_GCM_MUL_X + 16], "big")
        blocks = (aad + bytes(11)) + (ct + bytes(15)) + (8 * alen).to_bytes(8, "big") + (8 * length).to_bytes(8, "big")
        assert x == y_prev ^ int.from_bytes(blocks[16 * m:16 * m + 16], "big"), m
        q = tr[mul + TR_GCM_MUL_Q:mul + TR_GCM_MUL_Q + 128]
        assert max(q) <= 64
        # column sums of P: bit k of the product is the parity of sum_i p_{i,k}, and q_k its half
        p = np.frombuffer(tr[mul + TR_GCM_MUL_P:mul + TR_GCM_MUL_P + 2048], dtype=np.uint8).reshape(16, 128)
        for k in (0, 7, 8, 63, 127):
            total = int(((p[k // 8] >> (7 - k % 8)) & 1).sum())
            assert total == 2 * q[k] + ((y >> (127 - k)) & 1), (m, k)
        y_prev = y
    assert tr[-16:] == tag == bytes(a ^ b for a, b in zip(ys[-1].to_bytes(16, "big"), s10(nb + 1)))


@pytest.mark.parametrize("shape", [(1, 0), (17, 5)])
def test_lone_proof_and_its_rejections(api, gcm_key, shape):
    length, alen = shape
    pk, vk = gcm_key(length, alen)
    msg, key, iv, aad = TC3_PT[:length], TC3_KEY, TC3_IV, TC4_AAD[:alen]
    ct, tag, proof = api.encrypt_gcm(msg, key, iv, aad, pk)
    assert (ct, tag) == model_gcm(msg, key, iv, aad) and ct == TC3_CT[:length]
    assert api.verify_encryption_gcm(vk, proof, iv, aad, ct, tag) is True
    assert vk.verify(proof, bits(iv) + bits(aad) + bits(ct) + bits(tag)) is True        # the layout, independently of the new verifier
    assert api.proof_roundtrip(proof) == proof
    flip = lambda d, i, bit: d[:i] + bytes([d[i] ^ bit]) + d[i + 1:]
    assert api.verify_encryption_gcm(vk, proof, iv, aad, ct, flip(tag, 15, 0x01)) is False
    assert api.verify_encryption_gcm(vk, proof, iv, aad, ct, flip(tag, 0, 0x80)) is False
    assert api.verify_encryption_gcm(vk, proof, flip(iv, 11, 0x01), aad, ct, tag) is False
    assert api.verify_encryption_gcm(vk, proof, iv, aad, flip(ct, length - 1, 0x10), tag) is False
    if alen:
        assert api.verify_encryption_gcm(vk, proof, iv, flip(aad, alen - 1, 0x02), ct, tag) is False
    # another record: its own proof holds, its tag does not fit the first record and the first tag does not fit it
    iv2 = flip(iv, 0, 0x01)
    ct2, tag2, proof2 = api.encrypt_gcm(msg, key, iv2, aad, pk)
    assert (ct2, tag2) == model_gcm(msg, key, iv2, aad) and tag2 != tag
    assert api.verify_encryption_gcm(vk, proof2, iv2, aad, ct2, tag2) is True
    assert api.verify_encryption_gcm(vk, proof, iv, aad, ct, tag2) is False
    assert api.verify_encryption_gcm(vk, proof2, iv2, aad, ct2, tag) is False
    assert api.verify_encryption_gcm(vk, proof2, iv, aad, ct, tag) is False
    with pytest.raises(api.ZkAesError):                                      # the lengths are part of the statement
        api.verify_encryption_gcm(vk, proof, iv, aad, ct + b"\0", tag)
    with pytest.raises(api.ZkAesError):
        api.verify_encryption_gcm(vk, proof, iv, aad + b"\0", ct, tag)
    # a caller's seed gives a different, still valid proof of the same statement
    ct3, tag3, proof3 = api.encrypt_gcm(msg, key, iv, aad, pk, zk_seed=bytes(range(32)))
    assert (ct3, tag3) == (ct, tag) and proof3 != proof and api.verify_encryption_gcm(vk, proof3, iv, aad, ct, tag)
    for n, a in ((length + 1, alen), (length, alen + 1), (0, alen)):          # wrong lengths on this key
        with pytest.raises(api.ZkAesError):
            api.encrypt_gcm(bytes(n), key, iv, bytes(a), pk)
        with pytest.raises(api.ZkAesError):
            pk.witness_gcm(bytes(n), key, iv, bytes(a))


def test_batch_three_records_two_contexts(api, gcm_key):
    length, alen = 17, 5
    pk, vk = gcm_key(length, alen)
    rs = np.random.RandomState(0xBA7C)
    msgs, keys = [rs.bytes(length) for _ in range(3)], [rs.bytes(16) for _ in range(3)]
    ivs, aads = [rs.bytes(12) for _ in range(3)], [rs.bytes(alen) for _ in range(3)]
    want = [model_gcm(m, k, v, a) for m, k, v, a in zip(msgs, keys, ivs, aads)]
    pk.set_contexts(2)
    try:
        seed = bytes(range(100, 132))
        cts, tags, proofs = pk.encrypt_gcm_batch(msgs, keys, ivs, aads, zk_seed=seed)
        assert list(zip(cts, tags)) == want and len(proofs) == 3 and len({bytes(p) for p in proofs}) == 3
        for i in range(3):
            assert api.verify_encryption_gcm(vk, proofs[i], ivs[i], aads[i], cts[i], tags[i]) is True
        # a swapped pair: proof 0 under record 1's header, proof 1 under record 0's
        assert api.verify_encryption_gcm(vk, proofs[0], ivs[1], aads[1], cts[1], tags[1]) is False
        assert api.verify_encryption_gcm(vk, proofs[1], ivs[0], aads[0], cts[0], tags[0]) is False
        assert api.verify_encryption_gcm(vk, proofs[0], ivs[1], aads[0], cts[0], tags[0]) is False          # record 0 with record 1's iv alone
        assert api.verify_encryption_gcm(vk, proofs[0], ivs[0], aads[1], cts[0], tags[0]) is False          # ... with its aad alone
        # the same seeded call split in two: the second call's first proof has the job-global index 1
        c_a, t_a, p_a = pk.encrypt_gcm_batch(msgs[:1], keys[:1], ivs[:1], aads[:1], zk_seed=seed)
        c_b, t_b, p_b = pk.encrypt_gcm_batch(msgs[1:], keys[1:], ivs[1:], aads[1:], zk_seed=seed, first_proof_index=1)
        assert c_a + c_b == cts and t_a + t_b == tags and p_a + p_b == proofs
        with pytest.raises(api.ZkAesError):
            pk.encrypt_gcm_batch(msgs, keys, ivs, [a + b"\0" for a in aads], zk_seed=seed)
        with pytest.raises(api.ZkAesError):
            pk.encrypt_gcm_batch(msgs, keys[:2], ivs, aads, zk_seed=seed)
        assert pk.encrypt_gcm_batch([], [], [], [], zk_seed=seed) == ([], [], [])
    finally:
        pk.set_contexts(0)


def test_test_case_3_over_the_default_srs(api):
    """McGrew-Viega test case 3 (L = 64, A = 0: six AES blocks, five multiplications, 1,014,781 constraints) fits the reference's SRS literal, the default of
    synthesize_keys_gcm: |H| = 2^20, |K| = 2^22, |X| = 1024 as the 6-block ECB chunk the benchmark proves.  64 bytes is the largest message the literal holds"""
    key, iv, pt, aad, ct_want, tag_want = VECTORS[2]
    pk, vk = api.synthesize_keys_gcm(64, 0, flags=api.KEY_NO_TABLES)
    try:
        info = pk.info()
        assert (info["raw_constraints"], info["raw_instance"], info["h"], info["k"], info["instance"]) == (1_014_781, 737, 1 << 20, 1 << 22, 1024)
        assert info["joint_nnz"] == 4_013_852
        ct, tag, proof = api.encrypt_gcm(pt, key, iv, aad, pk, zk_seed=bytes(32))
        assert (ct, tag) == (ct_want, tag_want)
        assert api.verify_encryption_gcm(vk, proof, iv, aad, ct, tag) is True
        assert api.verify_encryption_gcm(vk, proof, iv, aad, ct, VECTORS[3][5]) is False                    # test case 4's tag
        with pytest.raises(api.ZkAesError):                                  # 65 bytes are a seventh AES block: |K| = 2^23
            api.synthesize_keys_gcm(65, 0, flags=api.KEY_NO_TABLES)
    finally:
        pk.free()


def test_entry_points_refuse_the_other_modes(api, gcm_key):
    pk_gcm, vk_gcm = gcm_key(16, 20)
    msg, key, iv16, iv, aad = TC3_PT[:16], TC3_KEY, TC3_IV + b"\0\0\0\2", TC3_IV, TC4_AAD
    for call in (lambda: api.encrypt(msg, key, pk_gcm), lambda: pk_gcm.encrypt_chunked(msg, key, zk_seed=api.PARITY), lambda: pk_gcm.encrypt_batch([msg], [key], zk_seed=api.PARITY),
                 lambda: pk_gcm.witness(msg, key), lambda: pk_gcm.prove_ops(1, 2), lambda: pk_gcm.op_lists(msg, key),
                 lambda: api.encrypt_cbc(msg, key, iv16, pk_gcm), lambda: pk_gcm.encrypt_cbc_chunked(msg, key, iv16, zk_seed=api.PARITY), lambda: pk_gcm.witness_cbc(msg, key, iv16),
                 lambda: api.encrypt_ctr(msg, key, iv16, pk_gcm), lambda: pk_gcm.encrypt_ctr_chunked(msg, key, iv16, zk_seed=api.PARITY), lambda: pk_gcm.witness_ctr(msg, key, iv16)):
        with pytest.raises(api.ZkAesError):
            call()
    others = {"ecb": api.synthesize_keys(16, srs=small_srs(api, api.CIRCUIT_AES, 16), flags=api.KEY_NO_TABLES),
              "cbc": api.synthesize_keys(16, circuit=api.CIRCUIT_AES_CBC, srs=small_srs(api, api.CIRCUIT_AES_CBC, 16), flags=api.KEY_NO_TABLES),
              "ctr": api.synthesize_keys(16, circuit=api.CIRCUIT_AES_CTR, srs=small_srs(api, api.CIRCUIT_AES_CTR, 16), flags=api.KEY_NO_TABLES),
              "ops": api.synthesize_keys(0, circuit=api.CIRCUIT_OPS_XOR, srs=(200, 200, 600))}
    try:
        for name, (pk, _) in others.items():
            for call in (lambda: api.encrypt_gcm(msg, key, iv, b"", pk), lambda: api.encrypt_gcm(msg, key, iv, aad, pk), lambda: pk.witness_gcm(msg, key, iv, b""),
                         lambda: pk.encrypt_gcm_batch([msg], [key], [iv], [b""], zk_seed=api.PARITY)):
                with pytest.raises(api.ZkAesError):
                    call()
        # every key still proves its own mode, and no key, through its own verifier, takes another mode's proof
        (pk_ecb, vk_ecb), (pk_cbc, vk_cbc), (pk_ctr, vk_ctr) = others["ecb"], others["cbc"], others["ctr"]
        proof_ecb = api.encrypt(msg, key, pk_ecb)
        ct_cbc, proof_cbc = api.encrypt_cbc(msg, key, iv16, pk_cbc)
        ct_ctr, proof_ctr = api.encrypt_ctr(msg, key, iv16, pk_ctr)
        ct_gcm, tag_gcm, proof_gcm = api.encrypt_gcm(msg, key, iv, aad, pk_gcm)
        assert api.verify_encryption(vk_ecb, proof_ecb, model_ecb(msg, key)) is True
        assert ct_cbc == model_cbc(msg, key, iv16) and api.verify_encryption_cbc(vk_cbc, proof_cbc, iv16, ct_cbc) is True
        assert ct_ctr == model_ctr(msg, key, iv16) and api.verify_encryption_ctr(vk_ctr, proof_ctr, iv16, ct_ctr) is True
        assert (ct_gcm, tag_gcm) == model_gcm(msg, key, iv, aad) and api.verify_encryption_gcm(vk_gcm, proof_gcm, iv, aad, ct_gcm, tag_gcm) is True
        assert ct_gcm == ct_ctr                                              # GCM's first message block runs under iv || 2: the CTR key proved the same keystream block
        for other in (proof_ecb, proof_cbc, proof_ctr):
            assert api.verify_encryption_gcm(vk_gcm, other, iv, aad, ct_gcm, tag_gcm) is False
        assert api.verify_encryption(vk_ecb, proof_gcm, ct_gcm) is False
        assert api.verify_encryption_cbc(vk_cbc, proof_gcm, iv16, ct_gcm) is False
        assert api.verify_encryption_ctr(vk_ctr, proof_gcm, iv16, ct_gcm) is False
        # the other keys' statements have 128 or 256 public bits, which no GCM shape has: a wrong A + L at the GCM verifier is an error
        for vk_other, proof_other in ((vk_ecb, proof_ecb), (vk_cbc, proof_cbc), (vk_ctr, proof_ctr)):
            with pytest.raises(api.ZkAesError):
                api.verify_encryption_gcm(vk_other, proof_other, iv, aad, ct_gcm, tag_gcm)
    finally:
        for pk, _ in others.values():
            pk.free()
