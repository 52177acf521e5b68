"""Selective disclosure on segmented GCM records on the GPU: a record longer than one proof opens chosen plaintext bytes.

Segment keys synthesized with reveal = True prove, beside the segment statement of DESIGN.md 9g, their slice of ONE record-wide mask and of ONE revealed array, so that
head, mid and tail together are the lone reveal statement of DESIGN.md 9i for (iv, aad, ciphertext, tag).  Correctness rests on the pure-Python models
(tests/gcm_segment_model.py, tests/gcm_segment_reveal_model.py), row-by-row constraint checks in numpy and the rejections below.  Every key but the last test's lives over
the default SRS literal without window tables, as in tests/test_gpu_gcm_segments.py, so the module builds one SRS; the proving shapes are c = 1 and c = 2.  No message
holds a zero byte: a hidden byte and a revealed zero byte are told apart by the mask alone.
"""
import os

import numpy as np
import pytest

import gcm_segment_model as seg_model
import gcm_segment_reveal_model as model
from test_gcm_host import model_gcm

pytestmark = pytest.mark.gpu

SEED = bytes(range(60, 92))
bits = model.bits
_keys = {}


@pytest.fixture(scope="module")
def seg_key(api):
    """(pk, vk) of a segment key over the default SRS literal, no window tables; one per (role, units, aad, key bits, reveal) for the module"""
    api.srs_hold(True)

    def get(role, units, aad=0, bits_=128, reveal=True):
        at = (role, units, aad, bits_, reveal)
        if at not in _keys:
            _keys[at] = api.synthesize_keys_gcm_segment(role, units, aad, flags=api.KEY_NO_TABLES, key_bits=bits_, reveal=reveal)
        return _keys[at]
    yield get
    for pk, _ in _keys.values():
        pk.free()
    _keys.clear()
    api.srs_hold(False)


def record_keys(seg_key, c, aad, tail_bytes, mid=True, bits_=128, reveal=True):
    ks = [seg_key("head", c, aad, bits_, reveal), seg_key("mid", c, 0, bits_, reveal) if mid else (None, None), seg_key("tail", tail_bytes, 0, bits_, reveal)]
    return tuple(k[0] for k in ks), tuple(k[1] for k in ks)


def record(seed, length, alen, key_bytes=16):
    rs = np.random.RandomState(seed)
    return bytes(b | 1 for b in rs.bytes(length)), rs.bytes(key_bytes), rs.bytes(12), rs.bytes(alen)


def salts_for(n, seed=7):
    rs = np.random.RandomState(0x5A19 + seed)
    return [rs.bytes(16) for _ in range(n - 1)]


OPEN_39 = [range(14, 19), 38]                                               # across the head / mid boundary, and the record's last byte


def test_the_gap_plain_segments_say_nothing_of_the_plaintext(api, seg_key):
    """a record of 39 bytes proven as three plain segments verifies for two different messages' ciphertexts alike: the verifier's input is (iv, aad, ciphertext, tag,
    commitments), nothing of the plaintext, and a plain key has no way to state a byte of it"""
    pks, vks = record_keys(seg_key, 1, 13, 7, reveal=False)
    msg, key, iv, aad = record(0x6A9, 39, 13)
    other = bytes(b ^ 0x42 for b in msg)
    for m in (msg, other):
        ct, tag, coms, proofs = api.encrypt_gcm_segments(m, key, iv, aad, pks, zk_seed=SEED)
        assert api.verify_gcm_segments(vks, proofs, iv, aad, ct, tag, coms, 1) == [True] * 3
        with pytest.raises(api.ZkAesError, match="no reveal region"):
            api.verify_gcm_segments(vks, proofs, iv, aad, ct, tag, coms, 1, mask=api.reveal_mask(OPEN_39, 39), revealed=api.reveal_bytes(m, OPEN_39))
    with pytest.raises(api.ZkAesError, match="no reveal region"):
        api.encrypt_gcm_segments(msg, key, iv, aad, pks, zk_seed=SEED, mask=OPEN_39)


def test_a_39_byte_record_opens_bytes_across_a_boundary(api, seg_key):
    """A = 13, c = 1, Lt = 7 under a mask that opens bytes 14 .. 18 and byte 38; then the rejections, each at the segment it belongs to, and the two invalid arguments"""
    pks, vks = record_keys(seg_key, 1, 13, 7)
    msg, key, iv, aad = record(0x39, 39, 13)
    salts = salts_for(3)
    mask = api.reveal_mask(OPEN_39, 39)
    ct, tag, coms, revealed, proofs = api.encrypt_gcm_segments(msg, key, iv, aad, pks, salts=salts, zk_seed=SEED, mask=OPEN_39)
    assert (ct, tag) == api.gcm_encrypt(msg, key, iv, aad) == model_gcm(msg, key, iv, aad)
    assert revealed == api.reveal_bytes(msg, mask) == model.revealed_of(msg, mask) and revealed[14:19] == msg[14:19] and revealed[38] == msg[38] and not any(revealed[:14] + revealed[19:38])
    ys = seg_model.segmented_gcm(msg, key, iv, aad, 1)[2]
    assert coms == [seg_model.commitment(key, y, s) for y, s in zip(ys, salts)]
    verify = lambda **kw: api.verify_gcm_segments(kw.get("vks", vks), kw.get("proofs", proofs), iv, aad, kw.get("ct", ct), tag, coms, 1, mask=kw.get("mask", mask), revealed=kw.get("revealed", revealed))
    assert verify() == [True, True, True]
    # the layout, independently of the new verifier: every segment's public input by the Python restatement through the generic verifier
    for s in range(3):
        assert vks[s].verify(proofs[s], model.public_input(s, 3, 1, iv, aad, ct, tag, coms, mask, revealed)) is True
        assert vks[s].verify(proofs[s], model.public_input(s, 3, 1, iv, aad, ct, tag, coms)) is False
    # ---- a changed revealed byte: rejected by the segment that holds it, and by no other
    change = lambda d, i, v: d[:i] + bytes([v]) + d[i + 1:]
    assert verify(revealed=change(revealed, 15, revealed[15] ^ 0x10)) == [False, True, True]
    assert verify(revealed=change(revealed, 17, revealed[17] ^ 0x01)) == [True, False, True]
    assert verify(revealed=change(revealed, 38, revealed[38] ^ 0x80)) == [True, True, False]
    # ---- a mask bit flipped over a non-zero byte: byte 16 declared hidden (its revealed byte zero, or the argument would be invalid), byte 20 declared open and zero
    hide16 = api.reveal_mask([range(14, 16), range(17, 19), 38], 39)
    assert verify(mask=hide16, revealed=change(revealed, 16, 0)) == [True, False, True]
    open20 = api.reveal_mask([range(14, 19), 20, 38], 39)
    assert msg[20] != 0 and verify(mask=open20) == [True, False, True]
    assert verify(mask=open20, revealed=change(revealed, 20, msg[20])) == [True, False, True]       # even with the right byte: the proof was made under another mask
    # ---- exchanged mask slices (with their revealed slices, or the argument would be invalid): head and mid each under the other's
    swapped_mask = mask[2:4] + mask[0:2] + mask[4:]
    swapped_rev = revealed[16:32] + revealed[0:16] + revealed[32:]
    assert verify(mask=swapped_mask, revealed=swapped_rev) == [False, False, True]
    assert verify(ct=change(ct, 38, ct[38] ^ 0x40)) == [True, True, False]                          # the 9g rejections stand
    assert verify(proofs=[proofs[0], b"\x01\x02\x03", proofs[2]]) == [True, False, True]
    # ---- the two invalid arguments raise, on both sides
    beyond = bytes([0, 0xc0, 0x07, 0, 0xc0])                                                        # bit 39 of a 39-byte record
    with pytest.raises(api.ZkAesError, match="at or beyond"):
        verify(mask=beyond)
    with pytest.raises(api.ZkAesError, match="at or beyond"):
        api.encrypt_gcm_segments(msg, key, iv, aad, pks, salts=salts, zk_seed=SEED, mask=beyond)
    with pytest.raises(api.ZkAesError, match="mask bit is 0"):
        verify(revealed=change(revealed, 3, 0x55))
    with pytest.raises(api.ZkAesError):
        verify(mask=mask[:-1])
    with pytest.raises(api.ZkAesError):
        verify(revealed=revealed[:-1])
    # nothing opened and everything opened are statements like any other
    for opened in ([], [range(39)]):
        ct2, tag2, coms2, rev2, proofs2 = api.encrypt_gcm_segments(msg, key, iv, aad, pks, salts=salts, zk_seed=SEED, mask=opened)
        assert (ct2, tag2, coms2) == (ct, tag, coms) and rev2 == (msg if opened else bytes(39))
        assert api.verify_gcm_segments(vks, proofs2, iv, aad, ct, tag, coms, 1, mask=opened, revealed=rev2) == [True] * 3
        assert api.verify_gcm_segments(vks, proofs2, iv, aad, ct, tag, coms, 1, mask=mask, revealed=revealed) == [False, False, False]


def test_a_49_byte_record_at_c_2(api, seg_key):
    """head (c = 2) + tail (Lt = 17): the tail's mask has three bytes, seven padding bits and a second reveal lane"""
    pks, vks = record_keys(seg_key, 2, 0, 17, mid=False)
    msg, key, iv, aad = record(0x49, 49, 0)
    opened = [range(30, 35), 47, 48]
    ct, tag, coms, revealed, proofs = api.encrypt_gcm_segments(msg, key, iv, aad, pks, zk_seed=SEED, mask=opened)
    assert (ct, tag) == api.gcm_encrypt(msg, key, iv, aad) and revealed == api.reveal_bytes(msg, opened) and len(proofs) == 2 and len(coms) == 1
    assert api.verify_gcm_segments(vks, proofs, iv, aad, ct, tag, coms, 2, mask=opened, revealed=revealed) == [True, True]
    wrong = revealed[:48] + bytes([revealed[48] ^ 1])
    assert api.verify_gcm_segments(vks, proofs, iv, aad, ct, tag, coms, 2, mask=opened, revealed=wrong) == [True, False]
    wrong = revealed[:31] + bytes([revealed[31] ^ 1]) + revealed[32:]
    assert api.verify_gcm_segments(vks, proofs, iv, aad, ct, tag, coms, 2, mask=opened, revealed=wrong) == [False, True]


def test_aes_256_head_and_tail(api, seg_key):
    pks, vks = record_keys(seg_key, 1, 0, 5, mid=False, bits_=256)
    msg, key, iv, aad = record(0x256, 21, 0, key_bytes=32)
    opened = [0, range(15, 18), 20]
    ct, tag, coms, revealed, proofs = api.encrypt_gcm_segments(msg, key, iv, aad, pks, zk_seed=SEED, mask=opened)
    assert (ct, tag) == api.gcm_encrypt(msg, key, iv, aad) and api.gcm_decrypt(ct, key, iv, aad, tag) == msg and revealed == api.reveal_bytes(msg, opened)
    assert api.verify_gcm_segments(vks, proofs, iv, aad, ct, tag, coms, 1, mask=opened, revealed=revealed) == [True, True]
    assert api.verify_gcm_segments(vks, proofs, iv, aad, ct, tag, coms, 1, mask=opened, revealed=revealed[:20] + bytes([revealed[20] ^ 2])) == [True, False]


def test_four_segments_two_contexts_and_split_calls(api, seg_key):
    """55 bytes at c = 1: the two mids run in one multi-proof call over two contexts, each under its own mask slice; the same job split over two calls with first_segment
    gives the same proofs byte for byte under passed salts, one zk seed and the one mask"""
    pks, vks = record_keys(seg_key, 1, 13, 7)
    msg, key, iv, aad = record(0x55, 55, 13)
    salts = salts_for(4)
    opened = [range(10, 20), range(30, 34), 54]
    pks[1].set_contexts(2)
    try:
        ct, tag, coms, revealed, proofs = api.encrypt_gcm_segments(msg, key, iv, aad, pks, salts=salts, zk_seed=SEED, mask=opened)
        assert (ct, tag) == model_gcm(msg, key, iv, aad) and len(proofs) == 4 and len({bytes(p) for p in proofs}) == 4 and revealed == api.reveal_bytes(msg, opened)
        assert api.verify_gcm_segments(vks, proofs, iv, aad, ct, tag, coms, 1, mask=opened, revealed=revealed) == [True] * 4
        assert api.verify_gcm_segments(vks, [proofs[0], proofs[2], proofs[1], proofs[3]], iv, aad, ct, tag, coms, 1, mask=opened, revealed=revealed) == [True, False, False, True]
        a = api.encrypt_gcm_segments(msg, key, iv, aad, pks, salts=salts, zk_seed=SEED, count=2, mask=opened)
        b = api.encrypt_gcm_segments(msg, key, iv, aad, pks, salts=salts, zk_seed=SEED, first_segment=2, mask=opened)
        assert a[:4] == b[:4] == (ct, tag, coms, revealed) and len(a[4]) == len(b[4]) == 2
        assert a[4] + b[4] == proofs
    finally:
        pks[1].set_contexts(0)


_mats = {}


def unsatisfied_rows(api, role, units, aad, z):
    at = (role, units, aad)
    if at not in _mats:
        _mats[at] = [api.circuit_matrix_gcm_segment(role, units, which, aad, reveal=True) for which in range(3)]
    zz = np.frombuffer(z, dtype=np.uint8).astype(np.int64)
    prods = []
    for rowptr, col, coeff in _mats[at]:
        assert len(zz) == len(rowptr) - 1                                    # square after padding
        cs = np.concatenate([[0], np.cumsum(coeff * zz[col])])
        prods.append(cs[rowptr[1:].astype(np.int64)] - cs[rowptr[:-1].astype(np.int64)])
    return np.nonzero(prods[0] * prods[1] != prods[2])[0]


def test_device_witness_of_a_mid(api, seg_key):
    """the device witness of the 39-byte record's mid under its mask slice satisfies (A z) o (B z) = C z row by row, and its instance is the host's public input; the
    reveal region of the trace is (mask, zeros, revealed, zeros) behind the two compression slots; a kernel handed a changed mask gives another instance"""
    pk, _ = seg_key("mid", 1)
    assert pk.segment_info() == {"role": "mid", "blocks": 1, "message_bytes": 16, "aad_bytes": 0}
    rv = pk.reveal_info()
    assert rv["reveal"] and rv["message_bytes"] == 16 and rv["mask_bytes"] == 2 and rv["offset"] % 16 == 0
    info = pk.info()
    for seed in (0x39, 0x3B):
        msg, key, iv, aad = record(seed, 39, 13)
        ct, tag, ys = seg_model.segmented_gcm(msg, key, iv, aad, 1)
        salts = salts_for(3, seed)
        coms = [seg_model.commitment(key, y, s) for y, s in zip(ys, salts)]
        mask = api.reveal_mask(OPEN_39, 39)
        revealed = model.revealed_of(msg, mask)
        public = model.public_input(1, 3, 1, iv, aad, ct, tag, coms, mask, revealed)
        header = api.gcm_segment_header(iv, 3, ys[0], salts[0], salts[1])
        z = pk.witness_gcm_segment(msg[16:32], key, header, mask=mask[2:4])
        assert z == pk.witness_gcm_segment(msg[16:32], key, api.gcm_segment_header(iv, 3, ys[0], salts[0], salts[1], mask=mask[2:4]))      # the header that ends in the mask
        assert len(z) == info["instance"] + info["witness"] and set(z) <= {0, 1}
        assert z[0] == 1 and z[1:1 + len(public)] == public and len(public) + 1 == info["raw_instance"] and not any(z[1 + len(public):info["instance"]])
        bad = unsatisfied_rows(api, "mid", 1, 0, z)
        assert len(bad) == 0, bad[:10]
        tr = pk.debug_fetch("trace")
        assert len(tr) == rv["offset"] + 32 and tr[rv["offset"]:] == mask[2:4] + bytes(14) + revealed[16:32]
        for at in (len(public) - 128 - 16 + 1, len(public) - 8 * 15 + 3):                            # the checker itself can fail: mask bit 1 (byte 17, open), a revealed bit of byte 17
            zf = bytearray(z)
            zf[1 + at] ^= 1
            assert len(unsatisfied_rows(api, "mid", 1, 0, bytes(zf))) >= 1
        other = pk.witness_gcm_segment(msg[16:32], key, header, mask=bytes([0x07, 0x80]))
        assert other[1:len(public) - 143] == z[1:len(public) - 143] and other[len(public) - 143:1 + len(public)] == bits(bytes([0x07, 0x80]) + model.revealed_of(msg[16:32], bytes([0x07, 0x80])))
    with pytest.raises(api.ZkAesError, match="at or beyond"):
        seg_key("tail", 7)[0].witness_gcm_segment(msg[32:], key, api.gcm_segment_header(iv, 4, ys[1], salts[1]), mask=bytes([0x80]))
    with pytest.raises(api.ZkAesError):
        pk.witness_gcm_segment(msg[16:32], key, header, mask=bytes(3))


def test_cross_refusals(api, seg_key, vectors):
    """every segment entry from before refuses a reveal segment key and names the _reveal_ entries; the _reveal_ entries refuse plain segment keys and keys that are no
    segment keys; the verifiers refuse each other's proofs -- raising where the key carries its public-input count, rejecting otherwise.  Last, parity: with reveal
    segment keys alive, the ECB key over the default SRS literals still emits the committed proof bytes under the fixed prover seed"""
    rv_pks, rv_vks = record_keys(seg_key, 1, 13, 7)
    pl_pks, pl_vks = record_keys(seg_key, 1, 13, 7, reveal=False)
    msg, key, iv, aad = record(0x2EF, 39, 13)
    header = api.gcm_segment_header(iv, 3)
    # ---- plain entries, reveal keys
    with pytest.raises(api.ZkAesError, match="reveals plaintext bytes.*zkaes_encrypt_gcm_segments_reveal_seeded_at"):
        api.encrypt_gcm_segments(msg, key, iv, aad, rv_pks, zk_seed=SEED)
    for keys in ((pl_pks[0], rv_pks[1], pl_pks[2]), (pl_pks[0], pl_pks[1], rv_pks[2])):
        with pytest.raises(api.ZkAesError, match="reveals plaintext bytes"):
            api.encrypt_gcm_segments(msg, key, iv, aad, keys, zk_seed=SEED)
    with pytest.raises(api.ZkAesError, match="reveals plaintext bytes.*zkaes_aes_witness_gcm_seg_rv"):
        rv_pks[1].witness_gcm_segment(msg[16:32], key, header)
    with pytest.raises(api.ZkAesError, match="reveals plaintext bytes.*_reveal_"):
        rv_pks[1].encrypt_gcm_segment_batch([msg[16:32]], [key], [header], zk_seed=SEED)
    for pk in rv_pks:                                                                                # the older entries of every mode, the lone reveal entries among them
        m = bytes(pk.segment_info()["message_bytes"])
        for call in (lambda: api.encrypt_gcm(m, key, iv, b"", pk), lambda: pk.witness_gcm(m, key, iv, b""), lambda: api.encrypt(m, key, pk), lambda: pk.witness(m, key),
                     lambda: pk.witness_digest(m, key, iv), lambda: pk.witness_reveal(m, key, [0], header=header), lambda: pk.encrypt_reveal_batch([m], [key], [[0]], headers=[iv], zk_seed=SEED)):
            with pytest.raises(api.ZkAesError):
                call()
        assert pk.mode()[0] == api.CIRCUIT_AES_GCM_SEG and pk.reveal_info()["reveal"] and pk.reveal_info()["mask_bytes"] == (pk.segment_info()["message_bytes"] + 7) // 8
    with pytest.raises(api.ZkAesError, match="segment key.*zkaes_aes_witness_gcm_seg_rv"):
        rv_pks[1].witness_reveal(msg[16:32], key, [0], header=header)
    # ---- reveal entries, plain keys and keys that are no segment keys
    for keys in ((pl_pks[0], rv_pks[1], rv_pks[2]), (rv_pks[0], pl_pks[1], rv_pks[2]), (rv_pks[0], rv_pks[1], pl_pks[2])):
        with pytest.raises(api.ZkAesError, match="no reveal region.*zkaes_synthesize_keys_gcm_seg_rv"):
            api.encrypt_gcm_segments(msg, key, iv, aad, keys, zk_seed=SEED, mask=OPEN_39)
    with pytest.raises(api.ZkAesError, match="no reveal region"):
        pl_pks[1].witness_gcm_segment(msg[16:32], key, header, mask=bytes(2))
    with pytest.raises(api.ZkAesError, match="no reveal region"):
        pl_pks[1].encrypt_gcm_segment_reveal_batch([msg[16:32]], [key], [header], [bytes(2)], zk_seed=SEED)
    assert not pl_pks[1].reveal_info()["reveal"] and pl_pks[1].reveal_info()["offset"] == 0
    others = {"ecb-reveal": api.synthesize_keys(16, flags=api.KEY_NO_TABLES, reveal=True), "ecb": api.synthesize_keys(16, flags=api.KEY_NO_TABLES)}
    try:
        for pk, _ in others.values():
            assert pk.segment_info() is None
            for call in (lambda: pk.witness_gcm_segment(msg[16:32], key, header, mask=bytes(2)), lambda: pk.encrypt_gcm_segment_reveal_batch([msg[16:32]], [key], [header], [bytes(2)], zk_seed=SEED),
                         lambda: api.encrypt_gcm_segments(msg, key, iv, aad, (rv_pks[0], pk, rv_pks[2]), zk_seed=SEED, mask=OPEN_39)):
                with pytest.raises(api.ZkAesError, match="not a GCM segment key"):
                    call()
        # ---- the verifiers
        salts = salts_for(3)
        ct, tag, coms, revealed, rv_proofs = api.encrypt_gcm_segments(msg, key, iv, aad, rv_pks, salts=salts, zk_seed=SEED, mask=OPEN_39)
        ct_p, tag_p, coms_p, pl_proofs = api.encrypt_gcm_segments(msg, key, iv, aad, pl_pks, salts=salts, zk_seed=SEED)
        assert (ct_p, tag_p, coms_p) == (ct, tag, coms)
        mask = api.reveal_mask(OPEN_39, 39)
        with pytest.raises(api.ZkAesError, match="reveals plaintext bytes.*zkaes_verify_gcm_segments_reveal"):
            api.verify_gcm_segments(rv_vks, rv_proofs, iv, aad, ct, tag, coms, 1)
        with pytest.raises(api.ZkAesError, match="no reveal region"):
            api.verify_gcm_segments(pl_vks, pl_proofs, iv, aad, ct, tag, coms, 1, mask=mask, revealed=revealed)
        ark = lambda vks: tuple(api.VerifyingKey.from_ark_bytes(vk.to_ark_bytes()) for vk in vks)
        assert api.verify_gcm_segments(ark(rv_vks), rv_proofs, iv, aad, ct, tag, coms, 1, mask=mask, revealed=revealed) == [True] * 3
        assert api.verify_gcm_segments(ark(rv_vks), rv_proofs, iv, aad, ct, tag, coms, 1) == [False] * 3
        assert api.verify_gcm_segments(ark(pl_vks), pl_proofs, iv, aad, ct, tag, coms, 1) == [True] * 3
        assert api.verify_gcm_segments(ark(pl_vks), pl_proofs, iv, aad, ct, tag, coms, 1, mask=mask, revealed=revealed) == [False] * 3
        assert api.verify_gcm_segments(ark(rv_vks), pl_proofs, iv, aad, ct, tag, coms, 1, mask=mask, revealed=revealed) == [False] * 3
        assert api.verify_gcm_segments(ark(pl_vks), rv_proofs, iv, aad, ct, tag, coms, 1) == [False] * 3
        # ---- parity
        proof = api.encrypt(bytes(vectors["plaintext"]), bytes(vectors["key"]), others["ecb"][0], zk_seed=None)
        gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
        assert proof == open(os.path.join(gold, "gpu_aes16_proof.bin"), "rb").read()
    finally:
        for pk, _ in others.values():
            pk.free()


def test_a_mid_at_the_default_c_with_window_tables(api):
    """one mid proof at c = 4, the default of AES-128 with reveal as without, over the default SRS with window tables: |H| = 2^20, |K| = 2^22, every second byte open"""
    c = api.GCM_SEGMENT_REVEAL_DEFAULT_C[128]
    assert c == api.gcm_segment_plan(16384, 13, reveal=True)["c"] == 4
    pk, vk = api.synthesize_keys_gcm_segment("mid", c, reveal=True)
    try:
        info = pk.info()
        assert (info["raw_constraints"], info["raw_instance"], info["h"], info["k"], info["joint_nnz"]) == (902_652 + 1088, 1153 + 576, 1 << 20, 1 << 22, 3_583_909)
        assert pk.segment_info() == {"role": "mid", "blocks": c, "message_bytes": 16 * c, "aad_bytes": 0} and pk.tables_built()[0]
        rs = np.random.RandomState(0xDD)
        m, key, iv, y_in, s_in, s_out = bytes(b | 1 for b in rs.bytes(16 * c)), rs.bytes(16), rs.bytes(12), rs.bytes(16), rs.bytes(16), rs.bytes(16)
        ctr0 = 2 + 3 * c
        want = seg_model.segment_trace("mid", m, key, iv, ctr0, y_in)
        com_in, com_out = seg_model.commitment(key, y_in, s_in), seg_model.commitment(key, want["ys"][-1].to_bytes(16, "big"), s_out)
        mask = api.reveal_mask(range(0, 16 * c, 2), 16 * c)
        revealed = model.revealed_of(m, mask)
        public = bits(iv + ctr0.to_bytes(4, "big") + want["ct"] + com_in + com_out + mask + revealed)
        header = api.gcm_segment_header(iv, ctr0, y_in, s_in, s_out)
        z = pk.witness_gcm_segment(m, key, header, mask=mask)
        assert z[1:1 + len(public)] == public
        [rev], [proof] = pk.encrypt_gcm_segment_reveal_batch([m], [key], [header], [mask], zk_seed=SEED)      # one segment alone: the caller's header and mask, the generic verifier
        assert rev == revealed
        assert vk.verify(proof, public) is True
        assert vk.verify(proof, public[:-1] + bytes([public[-1] ^ 1])) is False                    # a revealed bit
        at = len(public) - 8 * 16 * c - 8 * 2 * c                                                  # mask bit 0
        assert vk.verify(proof, public[:at] + bytes([public[at] ^ 1]) + public[at + 1:]) is False
    finally:
        pk.free()
