"""Digests on segmented GCM records on the GPU: a record longer than one proof is bound to the SHA-256 digest of its plaintext.

A digest record is nd data segments -- head, mids, the LAST with the record's final Lr bytes -- and one closing tail without data: nd + 1 proofs under nd commitments and
nd + 1 public states.  Every data segment also proves the SHA-256 compressions over its hidden bytes between two states (k_sha256_trace_seg behind the three segment
kernels, on the same stream); the last carries the final padding with the public bit count, so states[-1] is hashlib's digest of the plaintext.  Correctness rests on
hashlib, the pure-Python models (tests/gcm_segment_model.py, tests/gcm_segment_digest_model.py, tests/sha256_model.py), row-by-row constraint checks in numpy and the
rejections below.  AES-128 at c = 4 -- the smallest c a digest segment can have -- over the default SRS literal without window tables; the keys are made once per module.
Records: 65 bytes (head + last(1) + tail), 120 (last(56): two compressions), 128 (last(64)) and 145 (head + mid + last(17) + tail), all with 13 bytes of aad.
"""
import hashlib
import os

import numpy as np
import pytest

import gcm_segment_digest_model as model
import sha256_model
from test_gcm_host import model_gcm

pytestmark = pytest.mark.gpu

SEED = bytes(range(90, 122))
C4, AAD = 4, 13
bits = model.bits
_keys, _mats, _recs = {}, {}, {}


@pytest.fixture(scope="module")
def dg_key(api):
    """(pk, vk) of a digest segment key over the default SRS literal, no window tables; one per (role, units) for the module"""
    api.srs_hold(True)

    def get(role, units):
        if (role, units) not in _keys:
            _keys[(role, units)] = api.synthesize_keys_gcm_segment(role, units, AAD if role == "head" else 0, flags=api.KEY_NO_TABLES, digest=True)
        return _keys[(role, units)]
    yield get
    for pk, _ in _keys.values():
        pk.free()
    _keys.clear()
    _recs.clear()
    api.srs_hold(False)


def record_keys(dg_key, length):
    nd, lr = model.plan(length, C4)
    ks = [dg_key("head", C4), dg_key("mid", C4) if nd > 2 else (None, None), dg_key("last", lr), dg_key("tail", 0)]
    return tuple(k[0] for k in ks), tuple(k[1] for k in ks)


def record(seed, length):
    rs = np.random.RandomState(seed)
    return bytes(b | 1 for b in rs.bytes(length)), rs.bytes(16), rs.bytes(12), rs.bytes(AAD)


def salts_for(nd, seed):
    return [bytes([(seed + 16 * s + i) & 0xff for i in range(16)]) for s in range(nd)]


def proven(api, dg_key, seed, length):
    """the record of that seed and length, proven once for the module: (msg, key, iv, aad, ct, tag, coms, states, proofs)"""
    if (seed, length) not in _recs:
        msg, key, iv, aad = record(seed, length)
        pks, _ = record_keys(dg_key, length)
        out = api.encrypt_gcm_segments_digest(msg, key, iv, aad, pks, salts=salts_for(model.plan(length, C4)[0], seed), zk_seed=SEED)
        _recs[(seed, length)] = (msg, key, iv, aad) + out
    return _recs[(seed, length)]


def unsatisfied_rows(api, role, units, z):
    at = (role, units)
    if at not in _mats:
        _mats[at] = [api.circuit_matrix_gcm_segment(role, units, which, AAD if role == "head" else 0, digest=True) for which in range(3)]
    zz = np.frombuffer(z, dtype=np.uint8).astype(np.int64)
    prods = []
    for rowptr, col, coeff in _mats[at]:
        assert len(zz) == len(rowptr) - 1                                    # square after padding
        cs = np.concatenate([[0], np.cumsum(coeff * zz[col])])
        prods.append(cs[rowptr[1:].astype(np.int64)] - cs[rowptr[:-1].astype(np.int64)])
    return np.nonzero(prods[0] * prods[1] != prods[2])[0]


def test_the_gap_a_segmented_record_names_its_plaintext(api, dg_key):
    """a digest mid key exists (the call that fails before digests on segments: synthesize_keys_gcm_segment knows no digest=), and its public input ends in the two states
    a plain mid's lacks: before, no verifier input names the plaintext of a record longer than one proof"""
    pk, vk = dg_key("mid", C4)
    plain = api.circuit_info_gcm_segment("mid", C4)
    info = pk.info()
    assert info["raw_instance"] == plain["raw_instance"] + 512 and (info["h"], info["k"]) == (1 << 20, 1 << 22) and info["joint_nnz"] == 3_695_173
    assert pk.segment_info() == {"role": "mid", "blocks": C4, "message_bytes": 64, "aad_bytes": 0, "digest": True, "header_bytes": 112}
    assert pk.digest_info() == {"kind": "chain", "prefix": 0, "compressions": 1, "offset": pk.digest_info()["offset"]} and pk.digest_info()["offset"] % 16 == 0
    last, tail = dg_key("last", 56)[0], dg_key("tail", 0)[0]
    assert last.segment_info() == {"role": "last", "blocks": 4, "message_bytes": 56, "aad_bytes": 0, "digest": True, "header_bytes": 128}
    assert last.digest_info()["kind"] == "final" and last.digest_info()["compressions"] == 2
    assert tail.segment_info() == {"role": "tail", "blocks": 0, "message_bytes": 0, "aad_bytes": 0, "digest": True, "header_bytes": 80} and tail.digest_info()["kind"] is None
    assert tail.info()["k"] == 1 << 21


@pytest.mark.parametrize("role", ["head", "mid", "last", "tail"])
def test_witness_and_trace(api, dg_key, role):
    """proof `role` of the 145-byte record: the device witness satisfies every row, its instance is the model's row, one flipped H_out bit is exactly one unsatisfied
    row; a last's digest region holds H_in, the record's real digest, and behind its slot the bit count"""
    msg, key, iv, aad = record(0x145, 145)
    nd, lr = model.plan(145, C4)
    s = {"head": 0, "mid": 1, "last": 2, "tail": 3}[role]
    units = {"head": C4, "mid": C4, "last": lr, "tail": 0}[role]
    pk, _ = dg_key(role, units)
    ys, states = api.gcm_digest_plan(msg, key, iv, aad, C4)
    ct, tag = model_gcm(msg, key, iv, aad)
    salts = salts_for(nd, 0x145)
    coms = [api.gcm_commit(key, y, x) for y, x in zip(ys, salts)]
    header = api.gcm_segment_header(iv, 2 + s * C4, ys[s - 1] if s else None, salts[s - 1] if s else None, salts[s] if s < nd else None, api.gcm_length_block(AAD, 145), aad if s == 0 else b"",
                                    h_in=states[s] if s < nd else None, total_bits=8 * 145 if s == nd - 1 else None)
    assert len(header) == pk.segment_info()["header_bytes"]
    part = msg[64 * s:64 * s + (lr if s == nd - 1 else 64)] if s < nd else b""
    z = pk.witness_gcm_segment(part, key, header)
    tr = pk.debug_fetch("trace")
    info = pk.info()
    public = model.public_input(s, 145, C4, iv, aad, ct, tag, coms, states)
    assert len(z) == info["instance"] + info["witness"] and set(z) <= {0, 1} and z[0] == 1
    assert 1 + len(public) == info["raw_instance"] and z[1:info["raw_instance"]] == public and not any(z[info["raw_instance"]:info["instance"]])
    bad = unsatisfied_rows(api, role, units, z)
    assert len(bad) == 0, bad[:10]
    zf = bytearray(z)                                                        # the checker itself can fail
    zf[info["raw_instance"] - (3 if role != "last" else 64 + 3)] ^= 1        # an H_out bit (the closing tail: a com_in bit): its equality row
    assert len(unsatisfied_rows(api, role, units, bytes(zf))) == 1
    if role == "tail":
        return
    off = pk.digest_info()["offset"]
    assert tr[off:off + 32] == states[s] and tr[off + 32:off + 64] == states[s + 1]
    if role == "last":
        assert states[s + 1] == hashlib.sha256(msg).digest() == sha256_model.finish(states[s], 128, msg[128:])
        assert len(tr) == off + 64 + 4032 + 16 and tr[off + 64 + 4032:] == (8 * 145).to_bytes(8, "big") + bytes(8)
        zf = bytearray(z)
        zf[info["raw_instance"] - 5] ^= 1                                    # a total_bits bit: the rows of the schedule words it enters
        assert len(unsatisfied_rows(api, role, units, bytes(zf))) >= 1
    else:
        assert len(tr) == off + 64 + 4032 and states[s + 1] == sha256_model.chain(part, states[s])


def test_record_of_145_bytes(api, dg_key):
    """head + mid + last(17) + closing tail: accepted; ciphertext || tag is gcm_encrypt's; the last state is hashlib's digest; every wrong public value rejects exactly
    the proofs that state it"""
    msg, key, iv, aad, ct, tag, coms, states, proofs = proven(api, dg_key, 0x145, 145)
    _, vks = record_keys(dg_key, 145)
    assert len(proofs) == 4 and len(coms) == 3 and len(states) == 4
    assert (ct, tag) == api.gcm_encrypt(msg, key, iv, aad) == model_gcm(msg, key, iv, aad)
    assert states[0] == sha256_model.IV and states[-1] == hashlib.sha256(msg).digest() and states == model.states(msg, C4)
    check = lambda **kw: api.verify_gcm_segments_digest(kw.get("vks", vks), kw.get("proofs", proofs), iv, aad, kw.get("ct", ct), kw.get("tag", tag), kw.get("coms", coms), C4, kw.get("states", states),
                                                        digest_prefix=kw.get("prefix", 0))
    assert check() == [True] * 4
    flip = lambda b: bytes([b[0] ^ 1]) + b[1:]
    # a wrong states[j] rejects exactly the two data segments beside it; a wrong final digest the last only
    assert check(states=[flip(states[0])] + states[1:]) == [False, True, True, True]
    assert check(states=states[:1] + [flip(states[1])] + states[2:]) == [False, False, True, True]
    assert check(states=states[:2] + [flip(states[2])] + states[3:]) == [True, False, False, True]
    assert check(states=states[:3] + [flip(states[3])]) == [True, True, False, True]
    assert check(states=states[:3] + [hashlib.sha256(msg[:-1] + b"\0").digest()]) == [True, True, False, True]
    # the verifier sets total_bits itself: the right states behind a prefix the prover did not hash reject the last only
    assert check(prefix=64) == [True, True, False, True]
    # the tag belongs to the closing tail alone, a ciphertext byte to its own segment
    assert check(tag=flip(tag)) == [True, True, True, False]
    assert check(ct=ct[:70] + bytes([ct[70] ^ 1]) + ct[71:]) == [True, False, True, True]
    assert check(ct=ct[:-1] + bytes([ct[-1] ^ 1])) == [True, True, False, True]
    # a ciphertext one byte shorter: another last key's length, and another length block -- raised where the keys carry their counts
    with pytest.raises(api.ZkAesError, match="lengths"):
        check(ct=ct[:-1])
    # swapped commitments are rejected at the boundaries they sit on: coms[0] (head | mid), coms[1] (mid | last), coms[2] (last | tail)
    assert check(coms=[coms[1], coms[0], coms[2]]) == [False, False, False, True]
    assert check(coms=[coms[0], coms[2], coms[1]]) == [True, False, False, False]
    # another message's proofs under this message's states (same key, iv, aad and salts: its ciphertext and commitments differ too, so hand those over with the proofs)
    other = bytes([msg[0] ^ 2]) + msg[1:]
    pks, _ = record_keys(dg_key, 145)
    ct2, tag2, coms2, states2, proofs2 = api.encrypt_gcm_segments_digest(other, key, iv, aad, pks, salts=salts_for(3, 0x145), zk_seed=SEED)
    assert states2[1:] != states[1:] and api.verify_gcm_segments_digest(vks, proofs2, iv, aad, ct2, tag2, coms2, C4, states2) == [True] * 4
    assert api.verify_gcm_segments_digest(vks, proofs2, iv, aad, ct2, tag2, coms2, C4, states) == [False, False, False, True]      # (the head's H_out, the mid's both, the last's both)
    # counts that do not fit the record raise; a proof that does not parse is a rejected segment
    for kw in (dict(proofs=proofs[:3]), dict(coms=coms[:2]), dict(states=states[:3]), dict(prefix=32), dict(vks=(vks[0], None, vks[2], vks[3]))):
        with pytest.raises(api.ZkAesError):
            check(**kw)
    assert check(proofs=[proofs[0], proofs[1][:-7], proofs[2], b"junk"]) == [True, False, True, False]


@pytest.mark.parametrize("length", [65, 120, 128])
def test_short_records(api, dg_key, length):
    """head + last + closing tail, no mid key: last(1), last(56) with two compressions, last(64); and the record hashed behind a 64-byte prefix"""
    msg, key, iv, aad, ct, tag, coms, states, proofs = proven(api, dg_key, 0x500 + length, length)
    pks, vks = record_keys(dg_key, length)
    assert pks[1] is None and len(proofs) == 3 and pks[2].digest_info()["compressions"] == (2 if length == 120 else 1 if length == 65 else 2)
    assert (ct, tag) == model_gcm(msg, key, iv, aad) and states[-1] == hashlib.sha256(msg).digest()
    assert api.verify_gcm_segments_digest(vks, proofs, iv, aad, ct, tag, coms, C4, states) == [True] * 3
    assert api.verify_gcm_segments_digest(vks, proofs, iv, aad, ct, tag, coms, C4, states[:2] + [hashlib.sha256(msg + b"\0").digest()]) == [True, False, True]
    if length == 120:                                                        # the same keys serve the record behind a prefix: total_bits comes from the header, not the key
        prefix = bytes(range(64))
        h1 = api.sha256_chain(prefix)
        ct2, tag2, coms2, states2, proofs2 = api.encrypt_gcm_segments_digest(msg, key, iv, aad, pks, zk_seed=SEED, h_in=h1, digest_prefix=64)
        assert (ct2, tag2) == (ct, tag) and states2[0] == h1 and states2[-1] == hashlib.sha256(prefix + msg).digest()
        assert api.verify_gcm_segments_digest(vks, proofs2, iv, aad, ct2, tag2, coms2, C4, states2, digest_prefix=64) == [True] * 3
        assert api.verify_gcm_segments_digest(vks, proofs2, iv, aad, ct2, tag2, coms2, C4, states2) == [True, False, True]


def test_split_calls_are_byte_identical(api, dg_key):
    """the 145-byte record over two calls with passed salts: the same ciphertext, tag, commitments, states and proof bytes as the whole job"""
    msg, key, iv, aad, ct, tag, coms, states, proofs = proven(api, dg_key, 0x145, 145)
    pks, _ = record_keys(dg_key, 145)
    salts = salts_for(3, 0x145)
    a = api.encrypt_gcm_segments_digest(msg, key, iv, aad, pks, salts=salts, first_segment=0, count=2, zk_seed=SEED)
    b = api.encrypt_gcm_segments_digest(msg, key, iv, aad, pks, salts=salts, first_segment=2, zk_seed=SEED)
    assert a[:4] == b[:4] == (ct, tag, coms, states) and len(a[4]) == 2 and len(b[4]) == 2
    assert a[4] + b[4] == proofs
    with pytest.raises(api.ZkAesError):                                      # the record has 4 proofs
        api.encrypt_gcm_segments_digest(msg, key, iv, aad, pks, salts=salts, first_segment=3, count=2, zk_seed=SEED)
    with pytest.raises(api.ZkAesError, match="salt"):
        api.encrypt_gcm_segments_digest(msg, key, iv, aad, pks, salts=salts[:2], zk_seed=SEED)


def test_one_pairing_check_for_the_record(api, dg_key):
    """gcm_segment_digest_public_inputs through verify_batch_keys, on the device and on the host: the serial answers, honest and with a wrong state"""
    msg, key, iv, aad, ct, tag, coms, states, proofs = proven(api, dg_key, 0x145, 145)
    _, vks = record_keys(dg_key, 145)
    key_of, rows = api.gcm_segment_digest_public_inputs(4, iv, aad, ct, tag, coms, C4, states)
    assert key_of == [0, 1, 2, 3] and rows == [model.public_input(s, 145, C4, iv, aad, ct, tag, coms, states) for s in range(4)]
    assert [vk.verify(p, r) for vk, p, r in zip(vks, proofs, rows)] == [True] * 4
    wrong = states[:2] + [bytes([states[2][5] ^ 4]) * 32] + states[3:]
    _, wrong_rows = api.gcm_segment_digest_public_inputs(4, iv, aad, ct, tag, coms, C4, wrong)
    serial = api.verify_gcm_segments_digest(vks, proofs, iv, aad, ct, tag, coms, C4, wrong)
    assert serial == [True, False, False, True]
    for device in (True, False):
        assert api.verify_batch_keys(list(vks), key_of, proofs, rows, device=device) == [True] * 4
        assert api.verify_batch_keys(list(vks), key_of, proofs, wrong_rows, device=device) == serial


def test_cross_refusals(api, dg_key, vectors):
    """every older segment entry refuses a digest segment key and names the digest entries; the digest entries refuse a plain segment key and every other key and name
    theirs; the other modes' entries refuse a digest segment key as they refuse any segment key; and the parity ECB proof is still the committed one"""
    msg, key, iv, aad, ct, tag, coms, states, proofs = proven(api, dg_key, 0x500 + 65, 65)
    pks, vks = record_keys(dg_key, 65)
    plain = {"head": api.synthesize_keys_gcm_segment("head", C4, AAD, flags=api.KEY_NO_TABLES), "tail": api.synthesize_keys_gcm_segment("tail", 1, flags=api.KEY_NO_TABLES),
             "ecb": api.synthesize_keys(16, flags=api.KEY_NO_TABLES)}
    try:
        for pk in (pks[0], pks[2], pks[3]):
            info = pk.segment_info()
            m, hdr = bytes(info["message_bytes"]), api.gcm_segment_header(iv, 2, aad=bytes(info["aad_bytes"]))
            with pytest.raises(api.ZkAesError, match="digest record.*zkaes_encrypt_gcm_segment_digest_batch_seeded_at"):
                pk.encrypt_gcm_segment_batch([m], [key], [hdr], zk_seed=SEED)
            with pytest.raises(api.ZkAesError):                              # a plain header for a key whose header carries H_in; the closing tail's header is the plain one
                pk.witness_gcm_segment(m, key, hdr) if info["role"] != "tail" else pk.witness_gcm_segment(m, key, hdr + bytes(32))
            for call in (lambda: api.encrypt_gcm(m or b"\0", key, iv, b"", pk), lambda: pk.witness_gcm(m or b"\0", key, iv, b""), lambda: api.encrypt(bytes(16), key, pk),
                         lambda: pk.encrypt_digest_batch([m], [key], [iv], zk_seed=api.PARITY), lambda: pk.witness_digest(m, key, iv), lambda: pk.encrypt_batch([bytes(16)], [key], zk_seed=api.PARITY)):
                with pytest.raises(api.ZkAesError):
                    call()
            assert pk.mode()[0] == api.CIRCUIT_AES_GCM_SEG
        with pytest.raises(api.ZkAesError, match="digest record.*zkaes_encrypt_gcm_segments_digest_seeded_at"):
            api.encrypt_gcm_segments(msg, key, iv, aad, (pks[0], None, pks[3]), zk_seed=SEED)
        with pytest.raises(api.ZkAesError, match="digest record.*zkaes_verify_gcm_segments_digest"):
            api.verify_gcm_segments((vks[0], None, plain["tail"][1]), proofs[:2], iv, aad, ct, tag, coms[:1], C4)
        # the digest entries and the other keys
        with pytest.raises(api.ZkAesError, match="plain segment key.*encrypt_gcm_segments"):
            api.encrypt_gcm_segments_digest(msg, key, iv, aad, (plain["head"][0], None, pks[2], pks[3]), zk_seed=SEED)
        with pytest.raises(api.ZkAesError, match="plain segment key.*zkaes_synthesize_keys_gcm_seg_dg"):
            api.encrypt_gcm_segments_digest(msg, key, iv, aad, (pks[0], None, pks[2], plain["tail"][0]), zk_seed=SEED)
        with pytest.raises(api.ZkAesError, match="plain segment key.*zkaes_encrypt_gcm_segment_batch_seeded_at"):
            plain["tail"][0].encrypt_gcm_segment_digest_batch([b"\1"], [key], [api.gcm_segment_header(iv, 6)], zk_seed=SEED)
        with pytest.raises(api.ZkAesError, match="not a GCM segment key"):
            plain["ecb"][0].encrypt_gcm_segment_digest_batch([bytes(16)], [key], [api.gcm_segment_header(iv, 2)], zk_seed=SEED)
        with pytest.raises(api.ZkAesError, match="not a GCM segment key"):
            api.encrypt_gcm_segments_digest(msg, key, iv, aad, (plain["ecb"][0], None, pks[2], pks[3]), zk_seed=SEED)
        with pytest.raises(api.ZkAesError, match="plain segment key.*zkaes_verify_gcm_segments"):
            api.verify_gcm_segments_digest((plain["head"][1], None, vks[2], vks[3]), proofs, iv, aad, ct, tag, coms, C4, states)
        for keys in ((pks[0], None, pks[0], pks[3]), (pks[0], None, pks[2], pks[2])):      # a role in another's place
            with pytest.raises(api.ZkAesError, match="role"):
                api.encrypt_gcm_segments_digest(msg, key, iv, aad, keys, zk_seed=SEED)
        # one digest segment proof alone through the batch entry under the caller's header: byte-identical to the record's proof at the same index
        nd, lr = model.plan(65, C4)
        ys, st = api.gcm_digest_plan(msg, key, iv, aad, C4)
        salts = salts_for(nd, 0x500 + 65)
        hdr = api.gcm_segment_header(iv, 2 + C4, ys[0], salts[0], salts[1], api.gcm_length_block(AAD, 65), h_in=st[1], total_bits=8 * 65)
        assert pks[2].encrypt_gcm_segment_digest_batch([msg[64:]], [key], [hdr], zk_seed=SEED, first_proof_index=1) == [proofs[1]]
        # parity: with digest segment keys alive in the process, the ECB key over the default SRS literals still emits the committed proof bytes under the fixed prover seed
        proof = api.encrypt(bytes(vectors["plaintext"]), bytes(vectors["key"]), plain["ecb"][0], zk_seed=None)
        gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
        assert proof == open(os.path.join(gold, "gpu_aes16_proof.bin"), "rb").read()
    finally:
        for pk, _ in plain.values():
            pk.free()
