"""Key tags on segmented GCM records on the GPU: the records of a session are bound to one AES key.

A HEAD segment key synthesized with key_tag_blocks = T proves, beside the head's statement of DESIGN.md 9g, tag_t = AES_K(D_t), t < T (k_key_tag_trace behind the three
segment kernels, on the same stream); the boundary commitments carry the head's key to the mid and tail segments, so checking every record's head -- and every lone
tagged GCM record of DESIGN.md 9e -- against ONE tag binds the session to one key.  Correctness rests on the pure-Python models (tests/gcm_segment_model.py,
tests/gcm_segment_keytag_model.py, the FIPS-197 model behind them), row-by-row constraint checks in numpy and the rejections below.  Every key but the last test's lives
over the default SRS literal without window tables, as in tests/test_gpu_gcm_segments.py, so the module builds one SRS; the proving shapes are c = 1.
"""
import os

import numpy as np
import pytest

import gcm_segment_keytag_model as model
import gcm_segment_model as seg_model
import gcm_segment_reveal_model as rv_model
from test_gcm_host import model_gcm

pytestmark = pytest.mark.gpu

SEED = bytes(range(70, 102))
TR_BLOCK_STRIDE, NR = 1072, 10                                              # csrc/trace_layout.h, AES-128
SALT_20 = [bytes(range(16, 32))]                                            # the one boundary of a 20-byte record at c = 1
bits = rv_model.bits
_keys, _first = {}, {}


@pytest.fixture(scope="module")
def seg_key(api):
    """(pk, vk) of a segment key over the default SRS literal, no window tables; one per (role, units, aad, key-tag blocks, reveal) for the module"""
    api.srs_hold(True)

    def get(role, units, aad=0, blocks=0, reveal=False):
        at = (role, units, aad, blocks, reveal)
        if at not in _keys:
            _keys[at] = api.synthesize_keys_gcm_segment(role, units, aad, flags=api.KEY_NO_TABLES, reveal=reveal, key_tag_blocks=blocks)
            assert _keys[at][0].key_tag_blocks() == blocks
        return _keys[at]
    yield get
    for pk, _ in _keys.values():
        pk.free()
    _keys.clear()
    _first.clear()
    api.srs_hold(False)


def record_keys(seg_key, aad, tail_bytes, blocks, mid=False, reveal=False):
    """c = 1: a head with `blocks` tag blocks; the mid and tail keys are the untagged ones whatever the head"""
    ks = [seg_key("head", 1, aad, blocks, reveal), seg_key("mid", 1, 0, 0, reveal) if mid else (None, None), seg_key("tail", tail_bytes, 0, 0, reveal)]
    return tuple(k[0] for k in ks), tuple(k[1] for k in ks)


def record(seed, length, alen):
    rs = np.random.RandomState(seed)
    return bytes(b | 1 for b in rs.bytes(length)), rs.bytes(16), rs.bytes(12), rs.bytes(alen)


def other_key(key):
    return bytes([key[0] ^ 0x80]) + key[1:]


def two_records(api, pks):
    """two 20-byte records (head + tail, A = 5) under K and K': [(key, iv, aad, ct, tag, coms, proofs)]"""
    out = []
    for seed, flip in ((0x201, False), (0x202, True)):
        msg, key, iv, aad = record(seed, 20, 5)
        key = other_key(record(0x201, 20, 5)[1]) if flip else key
        ct, tag, coms, proofs = api.encrypt_gcm_segments(msg, key, iv, aad, pks, salts=SALT_20, zk_seed=SEED)      # (salts passed: the proofs are a function of the arguments)
        assert (ct, tag) == model_gcm(msg, key, iv, aad) and len(proofs) == 2
        out.append((key, iv, aad, ct, tag, coms, proofs))
    return out


def test_the_gap_two_keys_in_one_batch(api, seg_key):
    """two records made under K and K' with untagged segment keys, verified in ONE verify_gcm_records_batch call: every segment is accepted, and nothing tells that the
    session's records come from two keys.  (Passes before and after key tags on segments: it documents the gap)"""
    pks, vks = record_keys(seg_key, 5, 4, 0)
    recs = two_records(api, pks)
    assert recs[0][0] != recs[1][0]
    _first["untagged_head_proof"] = (recs[0], bytes(recs[0][6][0]))                               # made before any tagged segment key of this module exists
    batch = [(vks, proofs, iv, aad, ct, tag, coms, 1) for _, iv, aad, ct, tag, coms, proofs in recs]
    assert api.verify_gcm_records_batch(batch) == [[True, True], [True, True]]


def test_one_tag_tells_the_keys_apart(api, seg_key):
    """the same two records with a T = 1 head (the untagged tail key reused): under key_tag(K, 1) K's record is [True, True] and K''s [False, True]; under key_tag(K', 1)
    mirrored; verify_gcm_segments and verify_gcm_segments_batch agree, on the device and on the host; the cross cases raise"""
    pks, vks = record_keys(seg_key, 5, 4, 1)
    assert pks[2] is record_keys(seg_key, 5, 4, 0)[0][2] and pks[0].key_tag_blocks() == 1 and pks[2].key_tag_blocks() == 0
    recs = two_records(api, pks)
    (k1, k2) = recs[0][0], recs[1][0]
    batch = [(vks, proofs, iv, aad, ct, tag, coms, 1) for _, iv, aad, ct, tag, coms, proofs in recs]
    t1, t2 = api.key_tag(k1, 1), api.key_tag(k2, 1)
    assert t1 == model.key_tag(k1, 1) and t2 == model.key_tag(k2, 1) and t1 != t2
    assert api.verify_gcm_records_batch(batch, key_tag=t1) == [[True, True], [False, True]]
    assert api.verify_gcm_records_batch(batch, key_tag=t2) == [[False, True], [True, True]]
    assert api.verify_gcm_records_batch(batch, device=False, key_tag=t1) == [[True, True], [False, True]]
    for tag_, want in ((t1, [[True, True], [False, True]]), (t2, [[False, True], [True, True]])):
        for r, (_, iv, aad, ct, tag, coms, proofs) in enumerate(recs):
            assert api.verify_gcm_segments(vks, proofs, iv, aad, ct, tag, coms, 1, key_tag=tag_) == want[r]
            for device in (True, False):
                assert api.verify_gcm_segments_batch(vks, proofs, iv, aad, ct, tag, coms, 1, device=device, key_tag=tag_) == want[r]
    # the cross cases, as DESIGN.md 9e's: the key of this process carries its public-input count and raises; after the ark transport the head is rejected
    _, iv, aad, ct, tag, coms, proofs = recs[0]
    pl_vks = record_keys(seg_key, 5, 4, 0)[1]
    ark = lambda ks: tuple(None if vk is None else api.VerifyingKey.from_ark_bytes(vk.to_ark_bytes()) for vk in ks)
    for fn in (api.verify_gcm_segments, api.verify_gcm_segments_batch):
        with pytest.raises(api.ZkAesError, match="key_tag_blocks = 1"):
            fn(vks, proofs, iv, aad, ct, tag, coms, 1)                                             # a tagged head without a tag
        with pytest.raises(api.ZkAesError, match="key_tag_blocks = 1"):
            fn(vks, proofs, iv, aad, ct, tag, coms, 1, key_tag=api.key_tag(k1, 2))                 # 32 bytes for a T = 1 head
        with pytest.raises(api.ZkAesError, match="key_tag_blocks = 0"):
            fn(pl_vks, proofs, iv, aad, ct, tag, coms, 1, key_tag=t1)                              # an untagged head with a tag
        assert fn(ark(vks), proofs, iv, aad, ct, tag, coms, 1, key_tag=t1) == [True, True]
        assert fn(ark(vks), proofs, iv, aad, ct, tag, coms, 1) == [False, True]
        assert fn(ark(vks), proofs, iv, aad, ct, tag, coms, 1, key_tag=api.key_tag(k1, 2)) == [False, True]
        assert fn(ark(pl_vks), proofs, iv, aad, ct, tag, coms, 1, key_tag=t1) == [False, True]
    assert api.verify_gcm_records_batch([batch[0]]) == [[False, True]]                            # the records batch leaves every key-fit question to the proof


def test_a_mixed_session_under_one_tag(api, seg_key):
    """a session of one 16-byte record under a lone tagged GCM key and one 36-byte record (head, mid, tail) under a tagged head: both are checked against
    the same 16-byte tag, and a record made under another key fails it in either form"""
    pks, vks = record_keys(seg_key, 5, 4, 1, mid=True)
    msg, key, iv, aad = record(0x301, 36, 5)
    session = api.key_tag(key, 1)
    lone_pk, lone_vk = api.synthesize_keys_gcm(16, 5, flags=api.KEY_NO_TABLES, key_tag_blocks=1)
    try:
        ct, tag, coms, proofs = api.encrypt_gcm_segments(msg, key, iv, aad, pks, zk_seed=SEED)
        assert (ct, tag) == model_gcm(msg, key, iv, aad) and len(proofs) == 3
        m16, _, iv16, aad16 = record(0x302, 16, 5)
        for k, ok in ((key, True), (other_key(key), False)):
            ct16, tag16, proof16 = api.encrypt_gcm(m16, k, iv16, aad16, lone_pk)
            assert api.verify_encryption_gcm_tagged(lone_vk, proof16, iv16, aad16, ct16, tag16, session) is ok
        assert api.verify_gcm_segments(vks, proofs, iv, aad, ct, tag, coms, 1, key_tag=session) == [True, True, True]
        assert api.verify_gcm_records_batch([(vks, proofs, iv, aad, ct, tag, coms, 1)], key_tag=session) == [[True, True, True]]
        ct2, tag2, coms2, proofs2 = api.encrypt_gcm_segments(msg, other_key(key), iv, aad, pks, zk_seed=SEED)
        assert api.verify_gcm_segments(vks, proofs2, iv, aad, ct2, tag2, coms2, 1, key_tag=session) == [False, True, True]
        # a head of K spliced onto K''s mid and tail: the head's com_out is over K, the mid's com_in over K'
        assert api.verify_gcm_segments(vks, [proofs[0]] + proofs2[1:], iv, aad, ct[:16] + ct2[16:], tag2, [coms[0], coms2[1]], 1, key_tag=session) == [True, False, True]
        assert api.verify_gcm_segments(vks, [proofs[0]] + proofs2[1:], iv, aad, ct[:16] + ct2[16:], tag2, coms2, 1, key_tag=session) == [False, True, True]
    finally:
        lone_pk.free()


_mats = {}


def unsatisfied_rows(api, aad, blocks, reveal, z):
    at = (aad, blocks, reveal)
    if at not in _mats:
        _mats.clear()
        _mats[at] = [api.circuit_matrix_gcm_segment("head", 1, which, aad, reveal=reveal, key_tag_blocks=blocks) for which in range(3)]
    zz = np.frombuffer(z, dtype=np.uint8).astype(np.int64)
    prods = []
    for rowptr, col, coeff in _mats[at]:
        assert len(zz) == len(rowptr) - 1                                    # square after padding
        cs = np.concatenate([[0], np.cumsum(coeff * zz[col])])
        prods.append(cs[rowptr[1:].astype(np.int64)] - cs[rowptr[:-1].astype(np.int64)])
    return np.nonzero(prods[0] * prods[1] != prods[2])[0]


def head_case(api, seed, aad_len=5):
    """the head of a 36-byte record at c = 1: (message slice, key, header, public input without tag, key)"""
    msg, key, iv, aad = record(seed, 36, aad_len)
    ct, tag, ys = seg_model.segmented_gcm(msg, key, iv, aad, 1)
    rs = np.random.RandomState(0x5A1B + seed)
    salt = rs.bytes(16)
    com = seg_model.commitment(key, ys[0], salt)
    return msg[:16], key, api.gcm_segment_header(iv, 2, salt_out=salt, aad=aad), bits(iv + (2).to_bytes(4, "big") + aad + ct[:16] + com)


def test_witness_and_trace_of_a_tagged_head(api, seg_key):
    """the device witness of a T = 1 head satisfies (A z) o (B z) = C z row by row; its instance is the untagged head's, then the model's tag bits; the tag slot holds
    D_0, D_0 ^ key and S_Nr = the tag at the untagged trace's length; the trace ahead of the slot is the untagged head's for the same inputs"""
    pk, _ = seg_key("head", 1, 5, 1)
    plain_pk, _ = seg_key("head", 1, 5, 0)
    info, plain_info = pk.info(), plain_pk.info()
    assert info["raw_instance"] == plain_info["raw_instance"] + 128 and info["raw_witness"] == plain_info["raw_witness"] + 147_760
    assert pk.segment_info() == {"role": "head", "blocks": 1, "message_bytes": 16, "aad_bytes": 5}
    for seed in (0x401, 0x402):
        m, key, header, public = head_case(api, seed)
        want_tag = model.key_tag(key, 1)
        z = pk.witness_gcm_segment(m, key, header)
        tr = pk.debug_fetch("trace")
        assert len(z) == info["instance"] + info["witness"] and set(z) <= {0, 1}
        assert z[0] == 1 and z[1:1 + len(public)] == public and z[1 + len(public):info["raw_instance"]] == bits(want_tag) and 1 + len(public) + 128 == info["raw_instance"]
        assert not any(z[info["raw_instance"]:info["instance"]])
        bad = unsatisfied_rows(api, 5, 1, False, z)
        assert len(bad) == 0, bad[:10]
        zf = bytearray(z)                                                    # the checker itself can fail: one tag bit flipped is one equality row
        zf[info["raw_instance"] - 3] ^= 1
        assert len(unsatisfied_rows(api, 5, 1, False, bytes(zf))) == 1
        plain_z = plain_pk.witness_gcm_segment(m, key, header)
        assert plain_z[:1 + len(public)] == z[:1 + len(public)]
        plain_tr = plain_pk.debug_fetch("trace")
        assert len(plain_tr) % 16 == 0 and len(tr) == len(plain_tr) + TR_BLOCK_STRIDE and tr[:len(plain_tr)] == plain_tr
        slot = tr[len(plain_tr):]
        assert slot[:16] == model.tag_constant(0) and slot[16:32] == bytes(d ^ k for d, k in zip(model.tag_constant(0), key))
        assert slot[16 + 16 * NR:32 + 16 * NR] == want_tag


def test_a_head_with_two_tag_blocks(api, seg_key):
    """AES-128, c = 1, T = 2: the 32-byte tag; a flipped byte of either block rejects the head only"""
    pks, vks = record_keys(seg_key, 5, 4, 2)
    msg, key, iv, aad = record(0x501, 20, 5)
    ct, tag, coms, proofs = api.encrypt_gcm_segments(msg, key, iv, aad, pks, zk_seed=SEED)
    kt = api.key_tag(key, 2)
    assert kt == model.key_tag(key, 2) and len(kt) == 32
    check = lambda t, **kw: api.verify_gcm_segments(vks, proofs, iv, aad, ct, tag, coms, 1, key_tag=t, **kw)
    assert check(kt) == [True, True]
    for at in (3, 16 + 9):
        flipped = kt[:at] + bytes([kt[at] ^ 0x10]) + kt[at + 1:]
        assert check(flipped) == [False, True]
        assert api.verify_gcm_segments_batch(vks, proofs, iv, aad, ct, tag, coms, 1, key_tag=flipped) == [False, True]
    assert check(api.key_tag(other_key(key), 2)) == [False, True]
    with pytest.raises(api.ZkAesError, match="key_tag_blocks = 2"):
        check(kt[:16])
    z = pks[0].witness_gcm_segment(msg[:16], key, api.gcm_segment_header(iv, 2, salt_out=bytes(16), aad=aad))
    ri = pks[0].info()["raw_instance"]
    assert z[ri - 256:ri] == bits(kt)
    tr = pks[0].debug_fetch("trace")
    assert tr[-TR_BLOCK_STRIDE:][:16] == model.tag_constant(1) and tr[-TR_BLOCK_STRIDE:][16 + 16 * NR:32 + 16 * NR] == kt[16:]


def test_a_tagged_reveal_head(api, seg_key):
    """a T = 1 head with reveal = True (and a reveal tail): the mask and the revealed bytes are still checked, and the tag bits sit behind com_out and ahead of the mask"""
    pks, vks = record_keys(seg_key, 5, 4, 1, reveal=True)
    msg, key, iv, aad = record(0x601, 20, 5)
    opened = [range(3, 9), 19]
    ct, tag, coms, revealed, proofs = api.encrypt_gcm_segments(msg, key, iv, aad, pks, zk_seed=SEED, mask=opened)
    mask, kt = api.reveal_mask(opened, 20), api.key_tag(key, 1)
    assert revealed == rv_model.revealed_of(msg, mask) and (ct, tag) == model_gcm(msg, key, iv, aad)
    check = lambda t=kt, m=mask, r=revealed: api.verify_gcm_segments(vks, proofs, iv, aad, ct, tag, coms, 1, mask=m, revealed=r, key_tag=t)
    assert check() == [True, True]
    assert api.verify_gcm_records_batch([(vks, proofs, iv, aad, ct, tag, coms, 1, mask, revealed)], key_tag=kt) == [[True, True]]
    assert check(t=api.key_tag(other_key(key), 1)) == [False, True]
    assert check(r=revealed[:4] + bytes([revealed[4] ^ 1]) + revealed[5:]) == [False, True]         # a revealed byte of the head
    hide = api.reveal_mask([range(4, 9), 19], 20)
    assert check(m=hide, r=rv_model.revealed_of(msg, hide)) == [False, True]                        # another mask than the proof's
    with pytest.raises(api.ZkAesError, match="key_tag_blocks = 1"):
        api.verify_gcm_segments(vks, proofs, iv, aad, ct, tag, coms, 1, mask=mask, revealed=revealed)
    # the documented position, in the rows and in the device witness
    rows, _ = api.gcm_segment_public_inputs(2, iv, aad, ct, tag, coms, 1, mask=mask, revealed=revealed, key_tag=kt)
    com_end = 128 + 40 + 128 + 256
    assert rows[0] == model.public_input(0, 2, 1, iv, aad, ct, tag, coms, kt, mask, revealed)
    assert rows[0][com_end:com_end + 128] == bits(kt) and rows[0][com_end + 128:] == bits(mask[:2]) + bits(revealed[:16])
    salt = bytes(range(16))
    z = pks[0].witness_gcm_segment(msg[:16], key, api.gcm_segment_header(iv, 2, salt_out=salt, aad=aad), mask=mask[:2])
    info, rv = pks[0].info(), pks[0].reveal_info()
    assert z[1 + com_end:info["raw_instance"]] == bits(kt) + bits(mask[:2]) + bits(revealed[:16])
    assert len(unsatisfied_rows(api, 5, 1, True, z)) == 0
    tr = pks[0].debug_fetch("trace")
    plain_len = rv["offset"] - TR_BLOCK_STRIDE                                                     # the reveal region begins where the tag slot ends
    assert plain_len % 16 == 0 and tr[plain_len:plain_len + 16] == model.tag_constant(0) and tr[rv["offset"]:] == mask[:2] + bytes(14) + revealed[:16]


def test_a_split_job_is_the_whole_job(api, seg_key):
    """a 36-byte record under a tagged head split over two calls with first_segment / count and passed salts gives the whole job's proofs byte for byte"""
    pks, vks = record_keys(seg_key, 5, 4, 1, mid=True)
    msg, key, iv, aad = record(0x701, 36, 5)
    rs = np.random.RandomState(0x702)
    salts = [rs.bytes(16), rs.bytes(16)]
    whole = api.encrypt_gcm_segments(msg, key, iv, aad, pks, salts=salts, zk_seed=SEED)
    a = api.encrypt_gcm_segments(msg, key, iv, aad, pks, salts=salts, zk_seed=SEED, count=1)
    b = api.encrypt_gcm_segments(msg, key, iv, aad, pks, salts=salts, zk_seed=SEED, first_segment=1)
    assert a[:3] == b[:3] == whole[:3] and len(a[3]) == 1 and len(b[3]) == 2
    assert a[3] + b[3] == whole[3]
    assert api.verify_gcm_segments(vks, whole[3], iv, aad, whole[0], whole[1], whole[2], 1, key_tag=api.key_tag(key, 1)) == [True] * 3


def test_parity_with_tagged_segment_keys_alive(api, seg_key, vectors):
    """with tagged segment keys alive in the process the parity-mode ECB proof is still the committed one, and an untagged head proof under a fixed zk_seed is byte for
    byte the one made before a tagged key was synthesized"""
    pks, _ = record_keys(seg_key, 5, 4, 0)
    msg, key, iv, aad = record(0x201, 20, 5)
    before = api.encrypt_gcm_segments(msg, key, iv, aad, pks, salts=SALT_20, zk_seed=SEED)
    fresh = api.synthesize_keys_gcm_segment("head", 1, 0, flags=api.KEY_NO_TABLES, key_tag_blocks=1)
    ecb = api.synthesize_keys(16, flags=api.KEY_NO_TABLES)
    try:
        assert fresh[0].key_tag_blocks() == 1 and pks[0].key_tag_blocks() == 0
        seg_key("head", 1, 5, 1)
        after = api.encrypt_gcm_segments(msg, key, iv, aad, pks, salts=SALT_20, zk_seed=SEED)
        assert after == before
        if "untagged_head_proof" in _first:                                                        # the module's first proof, made before any tagged segment key existed
            assert bytes(after[3][0]) == _first["untagged_head_proof"][1]
        proof = api.encrypt(bytes(vectors["plaintext"]), bytes(vectors["key"]), ecb[0], zk_seed=None)
        gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
        assert proof == open(os.path.join(gold, "gpu_aes16_proof.bin"), "rb").read()
    finally:
        fresh[0].free()
        ecb[0].free()


def test_a_tagged_head_at_the_default_c_with_window_tables(api):
    """one T = 1 head at c = 4, the default of AES-128 with one tag block as without, A = 13, over the default SRS with window tables: |H| = 2^20, |K| = 2^22 and the
    joint non-zeros of DESIGN.md 9l's table; the proof is accepted under the key's tag and under no other"""
    c = api.GCM_SEGMENT_KEYTAG_DEFAULT_C[1][128]
    assert c == api.gcm_segment_plan(16384, 13, key_tag_blocks=1)["c"] == 4
    pk, vk = api.synthesize_keys_gcm_segment("head", c, 13, key_tag_blocks=1)
    try:
        info = pk.info()
        assert (info["raw_constraints"], info["raw_instance"], info["h"], info["k"], info["joint_nnz"]) == (1_038_584, 1129, 1 << 20, 1 << 22, 4_112_567)
        assert pk.segment_info() == {"role": "head", "blocks": c, "message_bytes": 16 * c, "aad_bytes": 13} and pk.tables_built()[0] and pk.key_tag_blocks() == 1
        rs = np.random.RandomState(0x9D)
        m, key, iv, aad, salt = rs.bytes(16 * c), rs.bytes(16), rs.bytes(12), rs.bytes(13), rs.bytes(16)
        want = seg_model.segment_trace("head", m, key, iv, 2, aad=aad)
        com = seg_model.commitment(key, want["ys"][-1].to_bytes(16, "big"), salt)
        kt = model.key_tag(key, 1)
        public = bits(iv + (2).to_bytes(4, "big") + aad + want["ct"] + com + kt)
        header = api.gcm_segment_header(iv, 2, salt_out=salt, aad=aad)
        [proof] = pk.encrypt_gcm_segment_batch([m], [key], [header], zk_seed=SEED)                 # one segment alone: the caller's header, the generic verifier
        assert vk.verify(proof, public) is True
        assert vk.verify(proof, public[:-1] + bytes([public[-1] ^ 1])) is False                    # a tag bit
        assert vk.verify(proof, public[:-128] + bits(model.key_tag(other_key(key), 1))) is False
    finally:
        pk.free()
