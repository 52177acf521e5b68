"""GCM records longer than one proof on the GPU: segment-proofs over hidden commitments.

A record of n >= 2 segments is proven by a head key, n - 2 proofs of one mid key and a tail key; segment s exposes com_{s-1} and com_s, salted SHA-256 commitments to
(key, Y), so that the n proofs together are the lone GCM statement for the whole record.  Correctness rests on the published vectors (McGrew-Viega test case 4), the
pure-Python model (tests/gcm_segment_model.py), row-by-row constraint checks in numpy and the rejections below.  Every key lives over the default SRS literal without
window tables, so the module builds one SRS; the proving shapes are c = 1 and c = 2 (|H| = 2^19 .. 2^20).
"""
import os

import numpy as np
import pytest

import gcm_segment_model as model
from test_gcm_host import TC3_CT, TC3_IV, TC3_KEY, TC3_PT, TC4_AAD, VECTORS, model_gcm

pytestmark = pytest.mark.gpu

TR_BLOCK0, TR_BLOCK_STRIDE = 272, 1072                                      # csrc/trace_layout.h, AES-128
TR_GCM_MUL_STRIDE, TR_GCM_MUL_X, TR_GCM_MUL_Y = 2208, 0, 2192
TRS_YIN, TRS_COM_IN, TRS_COM_OUT, TRS_BLOCK_CTR0 = 0, 64, 96, 128
SEED = bytes(range(40, 72))


def bits(data):
    """8 LSB-first bits per byte, one byte (0/1) each: the public-input encoding"""
    return bytes((b >> i) & 1 for b in data for i in range(8))


_keys = {}


@pytest.fixture(scope="module")
def seg_key(api):
    """(pk, vk) of a segment key over the default SRS literal, no window tables; one per (role, units, aad, key bits) for the module"""
    api.srs_hold(True)

    def get(role, units, aad=0, bits_=128):
        at = (role, units, aad, bits_)
        if at not in _keys:
            _keys[at] = api.synthesize_keys_gcm_segment(role, units, aad, flags=api.KEY_NO_TABLES, key_bits=bits_)
        return _keys[at]
    yield get
    for pk, _ in _keys.values():
        pk.free()
    _keys.clear()
    api.srs_hold(False)


def record_keys(seg_key, c, aad, tail_bytes, mid=True, bits_=128):
    ks = [seg_key("head", c, aad, bits_), seg_key("mid", c, 0, bits_) if mid else (None, None), seg_key("tail", tail_bytes, 0, bits_)]
    return tuple(k[0] for k in ks), tuple(k[1] for k in ks)


def record(seed, length, alen, key_bytes=16):
    rs = np.random.RandomState(seed)
    return rs.bytes(length), rs.bytes(key_bytes), rs.bytes(12), rs.bytes(alen)


def salts_for(n, seed=7):
    rs = np.random.RandomState(0x5A17 + seed)
    return [rs.bytes(16) for _ in range(n - 1)]


def test_the_gap_a_65_byte_record(api, seg_key):
    """65 bytes are a seventh AES block of a lone GCM key: over the default SRS that key does not exist, and the record is proven as five segments of one block"""
    with pytest.raises(api.ZkAesError, match="IndexTooLarge"):
        api.synthesize_keys_gcm(65, 0, flags=api.KEY_NO_TABLES)
    pks, vks = record_keys(seg_key, 1, 5, 1)
    msg, key, iv, aad = record(0x65, 65, 5)
    ct, tag, coms, proofs = api.encrypt_gcm_segments(msg, key, iv, aad, pks, zk_seed=SEED)
    assert (ct, tag) == model_gcm(msg, key, iv, aad) == api.gcm_encrypt(msg, key, iv, aad) and len(proofs) == 5 and len(coms) == 4
    assert api.verify_gcm_segments(vks, proofs, iv, aad, ct, tag, coms, 1) == [True] * 5
    assert api.gcm_decrypt(ct, key, iv, aad, tag) == msg


_mats = {}


def unsatisfied_rows(api, role, units, aad, z):
    at = (role, units, aad)
    if at not in _mats:
        _mats[at] = [api.circuit_matrix_gcm_segment(role, units, which, aad) for which in range(3)]
    zz = np.frombuffer(z, dtype=np.uint8).astype(np.int64)
    prods = []
    for rowptr, col, coeff in _mats[at]:
        assert len(zz) == len(rowptr) - 1                                    # square after padding
        cs = np.concatenate([[0], np.cumsum(coeff * zz[col])])
        prods.append(cs[rowptr[1:].astype(np.int64)] - cs[rowptr[:-1].astype(np.int64)])
    return np.nonzero(prods[0] * prods[1] != prods[2])[0]


def segment_case(api, role, seed):
    """the 39-byte record's segment of that role: (message slice, key, header, expected public input)"""
    msg, key, iv, aad = record(seed, 39, 5)
    ct, tag, ys = model.segmented_gcm(msg, key, iv, aad, 1)
    salts = salts_for(3, seed)
    coms = [model.commitment(key, y, s) for y, s in zip(ys, salts)]
    lenblk = model.length_block(5, 39)
    if role == "head":
        return msg[:16], key, api.gcm_segment_header(iv, 2, salt_out=salts[0], aad=aad), bits(iv + (2).to_bytes(4, "big") + aad + ct[:16] + coms[0])
    if role == "mid":
        return msg[16:32], key, api.gcm_segment_header(iv, 3, ys[0], salts[0], salts[1]), bits(iv + (3).to_bytes(4, "big") + ct[16:32] + coms[0] + coms[1])
    return msg[32:], key, api.gcm_segment_header(iv, 4, ys[1], salts[1], length_block=lenblk), bits(iv + (4).to_bytes(4, "big") + ct[32:] + lenblk + tag + coms[1])


@pytest.mark.parametrize("role", ["head", "mid", "tail"])
def test_witness_satisfies_every_constraint(api, seg_key, role):
    """(A z) o (B z) = C z row by row in numpy, for head (A = 5, c = 1), mid (c = 1) and tail (Lt = 7); the instance is the model's"""
    units, a = {"head": (1, 5), "mid": (1, 0), "tail": (7, 0)}[role]
    pk, _ = seg_key(role, units, a)
    info = pk.info()
    for seed in (0x39, 0x3A):
        m, key, header, public = segment_case(api, role, seed)
        z = pk.witness_gcm_segment(m, key, header)
        assert len(z) == info["instance"] + info["witness"] and set(z) <= {0, 1}
        assert z[0] == 1 and z[1:1 + len(public)] == public and len(public) + 1 == info["raw_instance"] and not any(z[1 + len(public):info["instance"]])
        bad = unsatisfied_rows(api, role, units, a, z)
        assert len(bad) == 0, bad[:10]
        for at in (1 + 96 + 5, len(public) - 9):                                 # the checker itself can fail: a ctr0 bit, a bit of the last commitment
            zf = bytearray(z)
            zf[at] ^= 1
            assert len(unsatisfied_rows(api, role, units, a, bytes(zf))) >= 1
    with pytest.raises(api.ZkAesError):
        pk.witness_gcm_segment(m + b"\0", key, header)
    with pytest.raises(api.ZkAesError):
        pk.witness_gcm_segment(m, key, header + b"\0")


def test_trace_region_of_a_mid(api, seg_key):
    """the trace of a mid (c = 1) against the Python model: iv and ctr0, the ciphertext block, Y_in, X_0 = Y_in ^ C_0 and Y_0, the block's counter bytes, both
    commitments"""
    pk, _ = seg_key("mid", 1)
    m, key, header, _ = segment_case(api, "mid", 0x7A)
    msg, _, iv, aad = record(0x7A, 39, 5)
    ct, _, ys = model.segmented_gcm(msg, key, iv, aad, 1)
    salts = salts_for(3, 0x7A)
    want = model.segment_trace("mid", m, key, iv, 3, ys[0])
    pk.witness_gcm_segment(m, key, header)
    tr = pk.debug_fetch("trace")
    gcm = TR_BLOCK0 + 2 * TR_BLOCK_STRIDE                                    # two AES slots: the data block, H
    mul0 = gcm + 16 + 16 + 2048
    sg = mul0 + TR_GCM_MUL_STRIDE + 16
    assert len(tr) == sg + 144 + 2 * 4032
    assert tr[gcm:gcm + 16] == iv + (3).to_bytes(4, "big") and tr[gcm + 16:gcm + 32] == ct[16:32] == want["ct"]
    assert tr[sg + TRS_YIN:sg + 16] == ys[0]
    assert int.from_bytes(tr[mul0 + TR_GCM_MUL_X:mul0 + 16], "big") == want["xs"][0] == int.from_bytes(ys[0], "big") ^ int.from_bytes(ct[16:32], "big")
    assert tr[mul0 + TR_GCM_MUL_Y:mul0 + TR_GCM_MUL_Y + 16] == ys[1] == want["ys"][0].to_bytes(16, "big")
    assert tr[sg + TRS_BLOCK_CTR0:sg + TRS_BLOCK_CTR0 + 8] == want["counters"][0] + want["carries"][0] == (3).to_bytes(4, "big") + bytes(4)
    assert tr[sg + TRS_COM_IN:sg + TRS_COM_IN + 32] == model.commitment(key, ys[0], salts[0]) == api.gcm_commit(key, ys[0], salts[0])
    assert tr[sg + TRS_COM_OUT:sg + TRS_COM_OUT + 32] == model.commitment(key, ys[1], salts[1])
    # the last feed-forward of each compression slot is its commitment (little-endian words in the slot, big-endian bytes in the commitment)
    for slot, com in ((sg + 144, TRS_COM_IN), (sg + 144 + 4032, TRS_COM_OUT)):
        ff = np.frombuffer(tr[slot + 3968:slot + 4000], dtype="<u4")
        assert ff.astype(">u4").tobytes() == tr[sg + com:sg + com + 32]


def test_a_39_byte_record_and_its_rejections(api, seg_key):
    """A = 5, c = 1: head + mid + tail"""
    pks, vks = record_keys(seg_key, 1, 5, 7)
    msg, key, iv, aad = record(0x39, 39, 5)
    salts = salts_for(3)
    ct, tag, coms, proofs = api.encrypt_gcm_segments(msg, key, iv, aad, pks, salts=salts, zk_seed=SEED)
    assert (ct, tag) == api.gcm_encrypt(msg, key, iv, aad) == model_gcm(msg, key, iv, aad)
    ys = model.segmented_gcm(msg, key, iv, aad, 1)[2]
    assert coms == [model.commitment(key, y, s) for y, s in zip(ys, salts)]
    verify = lambda **kw: api.verify_gcm_segments(kw.get("vks", vks), kw.get("proofs", proofs), kw.get("iv", iv), kw.get("aad", aad), kw.get("ct", ct), kw.get("tag", tag), kw.get("coms", coms), 1)
    assert verify() == [True, True, True]
    # the layout, independently of the new verifier: the mid's public input by hand
    assert vks[1].verify(proofs[1], bits(iv + (3).to_bytes(4, "big") + ct[16:32] + coms[0] + coms[1])) is True
    flip = lambda d, i, bit: d[:i] + bytes([d[i] ^ bit]) + d[i + 1:]
    assert verify(tag=flip(tag, 3, 0x20)) == [True, True, False]
    assert verify(iv=flip(iv, 11, 0x01)) == [False, False, False]
    assert verify(coms=coms[::-1]) == [False, False, False]                  # two commitments swapped
    assert verify(coms=[coms[0], flip(coms[1], 31, 0x01)]) == [True, False, False]
    assert verify(ct=ct[16:32] + ct[:16] + ct[32:]) == [False, False, True]  # segment slices exchanged: each runs under the other's ctr0
    assert verify(ct=flip(ct, 38, 0x40)) == [True, True, False]
    assert verify(proofs=[proofs[1], proofs[1], proofs[2]]) == [False, True, True]
    assert verify(proofs=[proofs[0], b"\x01\x02\x03", proofs[2]]) == [True, False, True]          # a proof that does not parse is a rejected segment
    # the mid made under another key: it holds against that key's ciphertext slice and commitments, and nowhere does it join the first key's chain
    key2 = bytes(x ^ 0x5A for x in key)
    ct2, tag2, coms2, proofs2 = api.encrypt_gcm_segments(msg, key2, iv, aad, pks, salts=salts, zk_seed=SEED)
    assert api.verify_gcm_segments(vks, proofs2, iv, aad, ct2, tag2, coms2, 1) == [True, True, True]
    mixed_ct, mixed = ct[:16] + ct2[16:32] + ct[32:], [proofs[0], proofs2[1], proofs[2]]
    assert verify(proofs=mixed) == [True, False, True]
    assert verify(proofs=mixed, ct=mixed_ct) == [True, False, True]
    assert verify(proofs=mixed, ct=mixed_ct, coms=coms2) == [False, True, False]
    assert verify(proofs=mixed, ct=mixed_ct, coms=[coms[0], coms2[1]]) == [True, False, False]
    # a changed A or L: the keys pin the lengths (an error); after the ark transport they know |X| only, and the length block the verifier builds does the rejecting
    for changed in ({"aad": aad + b"\0"}, {"ct": ct + b"\0"}, {"ct": ct[:-1]}):
        with pytest.raises(api.ZkAesError):
            verify(**changed)
    ark = tuple(api.VerifyingKey.from_ark_bytes(vk.to_ark_bytes()) for vk in vks)
    assert verify(vks=ark) == [True, True, True]
    assert verify(vks=ark, aad=aad + b"\0") == [False, True, False]
    assert verify(vks=ark, aad=aad[:-1]) == [False, True, False]
    assert verify(vks=ark, ct=ct + b"\0") == [True, True, False]
    with pytest.raises(api.ZkAesError):                                      # one commitment short
        verify(coms=coms[:1])
    with pytest.raises(api.ZkAesError):
        verify(proofs=proofs[:2])
    with pytest.raises(api.ZkAesError):                                      # a record whose last segment is not the tail key's
        api.encrypt_gcm_segments(msg + b"\0", key, iv, aad, pks, salts=salts, zk_seed=SEED)
    with pytest.raises(api.ZkAesError):
        api.encrypt_gcm_segments(msg, key, iv, aad + b"\0", pks, salts=salts, zk_seed=SEED)


def test_test_case_4_as_head_and_tail(api, seg_key):
    """McGrew-Viega test case 4 (L = 60, A = 20) at c = 2: head + tail, no mid key; the published ciphertext and tag"""
    key, iv, pt, aad, ct_want, tag_want = VECTORS[3]
    assert (key, iv, pt, aad) == (TC3_KEY, TC3_IV, TC3_PT[:60], TC4_AAD) and ct_want == TC3_CT[:60]
    pks, vks = record_keys(seg_key, 2, 20, 28, mid=False)
    ct, tag, coms, proofs = api.encrypt_gcm_segments(pt, key, iv, aad, pks, zk_seed=SEED)
    assert (ct, tag) == (ct_want, tag_want) and len(coms) == 1 and len(proofs) == 2
    assert api.verify_gcm_segments(vks, proofs, iv, aad, ct, tag, coms, 2) == [True, True]
    assert api.verify_gcm_segments(vks, proofs, iv, aad, ct, VECTORS[2][5], coms, 2) == [True, False]           # test case 3's tag
    assert api.verify_gcm_segments(vks, proofs[::-1], iv, aad, ct, tag, coms, 2) == [False, False]


def test_four_segments_two_contexts_and_split_calls(api, seg_key):
    """55 bytes at c = 1: the two mids run in one multi-proof call over two contexts; the same job split over two calls with first_segment gives the same proofs byte for
    byte under passed salts and one zk seed"""
    pks, vks = record_keys(seg_key, 1, 5, 7)
    msg, key, iv, aad = record(0x55, 55, 5)
    salts = salts_for(4)
    pks[1].set_contexts(2)
    try:
        ct, tag, coms, proofs = api.encrypt_gcm_segments(msg, key, iv, aad, pks, salts=salts, zk_seed=SEED)
        assert (ct, tag) == model_gcm(msg, key, iv, aad) and len(proofs) == 4 and len({bytes(p) for p in proofs}) == 4
        assert api.verify_gcm_segments(vks, proofs, iv, aad, ct, tag, coms, 1) == [True] * 4
        assert api.verify_gcm_segments(vks, [proofs[0], proofs[2], proofs[1], proofs[3]], iv, aad, ct, tag, coms, 1) == [True, False, False, True]
        ct_a, tag_a, coms_a, first = api.encrypt_gcm_segments(msg, key, iv, aad, pks, salts=salts, zk_seed=SEED, count=2)
        ct_b, tag_b, coms_b, second = api.encrypt_gcm_segments(msg, key, iv, aad, pks, salts=salts, zk_seed=SEED, first_segment=2)
        assert (ct_a, tag_a, coms_a) == (ct_b, tag_b, coms_b) == (ct, tag, coms) and len(first) == len(second) == 2
        assert api.verify_gcm_segments(vks, first + second, iv, aad, ct, tag, coms, 1) == [True] * 4
        assert first + second == proofs
        with pytest.raises(api.ZkAesError):                                  # past the record's end
            api.encrypt_gcm_segments(msg, key, iv, aad, pks, salts=salts, zk_seed=SEED, first_segment=3, count=2)
        out = api.lib().zkaes_encrypt_gcm_segments_seeded_at                 # a split job without salts would commit differently in every call: refused
        import ctypes as C
        p, n, lens = C.c_void_p(), C.c_size_t(), (C.c_size_t * 4)()
        assert out(msg, C.c_size_t(55), key, iv, aad, C.c_size_t(5), pks[0]._p, pks[1]._p, pks[2]._p, None, SEED, C.c_size_t(0), C.c_size_t(2), None, None, None, C.byref(p), C.byref(n), lens) != 0
    finally:
        pks[1].set_contexts(0)


def test_aes_256_head_and_tail(api, seg_key):
    pks, vks = record_keys(seg_key, 1, 0, 5, mid=False, bits_=256)
    msg, key, iv, aad = record(0x256, 21, 0, key_bytes=32)
    ct, tag, coms, proofs = api.encrypt_gcm_segments(msg, key, iv, aad, pks, zk_seed=SEED)
    assert (ct, tag) == api.gcm_encrypt(msg, key, iv, aad) and api.gcm_decrypt(ct, key, iv, aad, tag) == msg
    assert api.verify_gcm_segments(vks, proofs, iv, aad, ct, tag, coms, 1) == [True, True]
    assert api.verify_gcm_segments(vks, proofs, iv, aad, ct, tag, [bytes(32)], 1) == [False, False]
    with pytest.raises(api.ZkAesError):                                      # a 16-byte key on AES-256 keys
        api.encrypt_gcm_segments(msg, key[:16], iv, aad, pks, zk_seed=SEED)


def test_a_mid_at_the_default_c_with_window_tables(api):
    """one mid proof at c = 4, the default of AES-128, over the default SRS with window tables: |H| = 2^20, |K| = 2^22"""
    c = api.GCM_SEGMENT_DEFAULT_C[128]
    pk, vk = api.synthesize_keys_gcm_segment("mid", c)
    try:
        info = pk.info()
        assert (info["raw_constraints"], info["raw_instance"], info["h"], info["k"], info["joint_nnz"]) == (902_652, 1153, 1 << 20, 1 << 22, 3_581_221)
        assert pk.segment_info() == {"role": "mid", "blocks": c, "message_bytes": 16 * c, "aad_bytes": 0} and pk.tables_built()[0]
        rs = np.random.RandomState(0xDC)
        m, key, iv, y_in, s_in, s_out = rs.bytes(16 * c), rs.bytes(16), rs.bytes(12), rs.bytes(16), rs.bytes(16), rs.bytes(16)
        ctr0 = 2 + 3 * c
        want = model.segment_trace("mid", m, key, iv, ctr0, y_in)
        com_in, com_out = model.commitment(key, y_in, s_in), model.commitment(key, want["ys"][-1].to_bytes(16, "big"), s_out)
        public = bits(iv + ctr0.to_bytes(4, "big") + want["ct"] + com_in + com_out)
        header = api.gcm_segment_header(iv, ctr0, y_in, s_in, s_out)
        z = pk.witness_gcm_segment(m, key, header)
        assert z[1:1 + len(public)] == public
        [proof] = pk.encrypt_gcm_segment_batch([m], [key], [header], zk_seed=SEED)                 # one segment alone: the caller's header, the generic verifier
        assert vk.verify(proof, public) is True
        assert vk.verify(proof, public[:-1] + bytes([public[-1] ^ 1])) is False                    # a com_out bit
        assert vk.verify(proof, public[:96 + 31] + bytes([public[96 + 31] ^ 1]) + public[96 + 32:]) is False      # a ctr0 bit
    finally:
        pk.free()


def test_cross_refusals(api, seg_key, vectors):
    """every older GCM entry refuses a segment key and names the segment entries; the segment entries refuse every other key and name the lone entry; the other modes'
    entries refuse a segment key as they refuse each other's"""
    pks, vks = record_keys(seg_key, 1, 5, 7)
    msg, key, iv, aad = record(0x2EF, 39, 5)
    for pk in pks:
        m = bytes(pk.segment_info()["message_bytes"])
        for call in (lambda: api.encrypt_gcm(m, key, iv, b"", pk), lambda: pk.witness_gcm(m, key, iv, b""), lambda: pk.encrypt_gcm_batch([m], [key], [iv], [b""], zk_seed=api.PARITY)):
            with pytest.raises(api.ZkAesError, match="segment key.*zkaes_encrypt_gcm_segments_seeded_at"):
                call()
        for call in (lambda: api.encrypt(m, key, pk), lambda: pk.witness(m, key), lambda: pk.encrypt_chunked(m, key, zk_seed=api.PARITY), lambda: pk.encrypt_batch([m], [key], zk_seed=api.PARITY),
                     lambda: pk.op_lists(m, key), lambda: pk.prove_ops(1, 2), lambda: pk.witness_digest(m, key, iv), lambda: pk.encrypt_digest_batch([m], [key], [iv], zk_seed=api.PARITY),
                     lambda: api.encrypt_cbc(m, key, iv + bytes(4), pk), lambda: api.encrypt_ctr(m, key, iv + bytes(4), pk), lambda: pk.witness_ctr(m, key, iv + bytes(4))):
            with pytest.raises(api.ZkAesError):
                call()
        assert pk.mode()[0] == api.CIRCUIT_AES_GCM_SEG and pk.key_tag_blocks() == 0 and pk.digest_info()["kind"] is None
    others = {"gcm": api.synthesize_keys_gcm(16, 5, flags=api.KEY_NO_TABLES), "ecb": api.synthesize_keys(16, flags=api.KEY_NO_TABLES)}
    try:
        for name, (pk, _) in others.items():
            assert pk.segment_info() is None
            header = api.gcm_segment_header(iv, 3)
            for call in (lambda: pk.witness_gcm_segment(msg[:16], key, header), lambda: pk.encrypt_gcm_segment_batch([msg[:16]], [key], [header], zk_seed=SEED)):
                with pytest.raises(api.ZkAesError, match="not a GCM segment key"):
                    call()
            for keys in ((pk, pks[1], pks[2]), (pks[0], pk, pks[2]), (pks[0], pks[1], pk)):
                with pytest.raises(api.ZkAesError, match="not a GCM segment key.*zkaes_encrypt_gcm_seeded"):
                    api.encrypt_gcm_segments(msg, key, iv, aad, keys, zk_seed=SEED)
        for keys in ((pks[1], pks[1], pks[2]), (pks[0], pks[0], pks[2]), (pks[0], pks[1], pks[0]), (pks[0], None, pks[2])):      # a role in another's place; three segments without a mid
            with pytest.raises(api.ZkAesError, match="role|mid"):
                api.encrypt_gcm_segments(msg, key, iv, aad, keys, zk_seed=SEED)
        # parity: with segment keys alive in the process, the ECB key over the default SRS literals still emits the committed proof bytes under the fixed prover seed
        proof = api.encrypt(bytes(vectors["plaintext"]), bytes(vectors["key"]), others["ecb"][0], zk_seed=None)
        gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
        assert proof == open(os.path.join(gold, "gpu_aes16_proof.bin"), "rb").read()
    finally:
        for pk, _ in others.values():
            pk.free()
