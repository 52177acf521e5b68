"""Plaintext digests on the GPU: k_sha256_trace behind each mode's trace kernel(s) and the tag kernel, the witness against the digest circuit's own matrices, lone, chunked
and batch proofs checked against public SHA-256 states, and the gap this feature exists to close.

A key synthesized with digest = "chain" or "final" proves H_out = the SHA-256 compressions of its hidden message from H_in beside its mode's statement and its key tag;
H_in and H_out are the last 512 public inputs.  Correctness rests on hashlib, the pure-Python model of sha256_model.py (checked against hashlib in
test_digest_host.py) and a row-by-row check of (A z) o (B z) = C z in int64 numpy over the matrices circuit_matrix(..., digest=) returns.  The shapes are the smallest at
which the new kernel or layout can go wrong: one lane over a block of variables (ECB-128 64 B), a second lane that re-walks (128 B, witness only), padding inside the
block behind a tag slot (CTR-128 17 B), the one- / two-compression boundary (CTR-128 56 B), an H_in that is not the initial value behind the CBC tail (CBC-192 64 B), the
region behind the GHASH tail with a prefix (GCM-256 (17, 5), P = 64) and NK = 8 with two tag slots (ECB-256 64 B).  Every key is synthesized over an SRS sized from its
own circuit, without window tables, once per module.
"""
import hashlib
import os

import numpy as np
import pytest

import sha256_model as model
from test_gpu_keysize import bits, flip, kind_of, model_public, statement
from test_keysize_host import ks_ctr, ks_ecb, ks_gcm

pytestmark = pytest.mark.gpu

# (mode, key_bits, L, A, T, digest, P)
WITNESS_SHAPES = [("ecb", 128, 64, 0, 0, "chain", 0), ("ecb", 128, 128, 0, 0, "chain", 0), ("ctr", 128, 17, 0, 1, "final", 0), ("ctr", 128, 56, 0, 0, "final", 0),
                  ("cbc", 192, 64, 0, 1, "chain", 0), ("gcm", 256, 17, 5, 1, "final", 64), ("ecb", 256, 64, 0, 2, "chain", 0)]
PROVING_SHAPES = [s for s in WITNESS_SHAPES if s[:3] != ("ecb", 128, 128)]
_keys, _mats = {}, {}


@pytest.fixture(scope="module")
def dg_key(api):
    """(pk, vk) for (mode, key_bits, L, A, T, digest, P) over an SRS sized from the circuit's own counts, no window tables; one per shape for the module"""
    def get(*shape):
        mode, key_bits, length, alen, blocks, kind, prefix = shape
        if shape not in _keys:
            ci = api.circuit_info(kind_of(api, mode), length, alen, key_bits, blocks, kind, prefix)
            srs = (int(ci["constraints"]), int(ci["instance"]), int(ci["nnz_a"] + ci["nnz_b"] + ci["nnz_c"]))
            if mode == "gcm":
                _keys[shape] = api.synthesize_keys_gcm(length, alen, srs=srs, flags=api.KEY_NO_TABLES, key_bits=key_bits, key_tag_blocks=blocks, digest=kind, digest_prefix=prefix)
            else:
                _keys[shape] = api.synthesize_keys(length, circuit=kind_of(api, mode), srs=srs, flags=api.KEY_NO_TABLES, key_bits=key_bits, key_tag_blocks=blocks, digest=kind,
                                                   digest_prefix=prefix)
            info = _keys[shape][0].digest_info()
            assert (info["kind"], info["prefix"], info["compressions"]) == (kind, prefix, model.compressions(kind, length) if kind else 0)
        return _keys[shape]
    yield get
    for pk, _ in _keys.values():
        pk.free()
    _keys.clear()
    _mats.clear()


def unsatisfied_rows(api, shape, z):
    """indices of the rows where (A z) * (B z) != C z, in int64, as test_gpu_keytag.py checks them (the sums' coefficients reach 2^34 and z is 0/1: no overflow)"""
    mode, key_bits, length, alen, blocks, kind, prefix = shape
    if shape not in _mats:
        _mats[shape] = [api.circuit_matrix(kind_of(api, mode), length, which, alen, key_bits, blocks, kind, prefix) for which in range(3)]
    zz = np.frombuffer(z, dtype=np.uint8).astype(np.int64)
    prods = []
    for rowptr, col, coeff in _mats[shape]:
        assert len(zz) == len(rowptr) - 1                                    # square after padding
        cs = np.concatenate([[0], np.cumsum(coeff * zz[col])])
        prods.append(cs[rowptr[1:].astype(np.int64)] - cs[rowptr[:-1].astype(np.int64)])
    return np.nonzero(prods[0] * prods[1] != prods[2])[0]


def ids(shape):
    return "%s%d-L%d-A%d-T%d-%s-P%d" % shape


def header_of(shape, extra):
    """the mode's public header as the digest entry points take it: None (ECB), the iv / icb, iv + aad"""
    return {"ecb": None, "cbc": extra[0] if extra else None, "ctr": extra[0] if extra else None}.get(shape[0], b"".join(extra))


def h_in_of(shape, seed):
    """CBC-192 runs from a state that is not the initial value; the others alternate"""
    return np.random.RandomState(seed).bytes(32) if shape[0] == "cbc" or seed % 2 else None


def tag_of(api, shape, key):
    return api.key_tag(key, shape[4]) if shape[4] else None


def verify_lone(api, vk, shape, proof, extra, ct, gtag, key_tag, h_in, h_out):
    mode = shape[0]
    if mode == "gcm":
        return api.verify_encryption_gcm_digest(vk, proof, extra[0], extra[1], ct, gtag, h_out, h_in=h_in, key_tag=key_tag)
    states = [model.IV if h_in is None else h_in, h_out]
    return api.verify_digest_chunked(vk, kind_of(api, mode), [proof], ct, states, header=None if mode == "ecb" else extra[0], key_tag=key_tag)[0] == [True]


def test_the_gap_this_closes(api, dg_key):
    """without a digest a proof says "this decrypts to something": two different messages both verify and nothing a verifier holds names either; with a final key the
    proof for message B is rejected under sha256(A)"""
    base = ("ctr", 128, 56, 0)
    plain_pk, plain_vk = dg_key(*base, 0, None, 0)
    pk, vk = dg_key(*base, 0, "final", 0)
    _, key, icb, _ = statement(base, 0x6A9)
    rs = np.random.RandomState(0x6AA)
    a, b = rs.bytes(56), rs.bytes(56)
    ct_a, ct_b = ks_ctr(a, key, icb), ks_ctr(b, key, icb)
    proof_a, proof_b = api.encrypt_ctr(a, key, icb, plain_pk)[1], api.encrypt_ctr(b, key, icb, plain_pk)[1]
    assert api.verify_encryption_ctr(plain_vk, proof_a, icb, ct_a) is True and api.verify_encryption_ctr(plain_vk, proof_b, icb, ct_b) is True      # the gap: no input names a plaintext
    cts, _, h_outs, proofs = pk.encrypt_digest_batch([a, b], [key, key], headers=[icb, icb], zk_seed=bytes(range(32)))
    assert cts == [ct_a, ct_b] and h_outs == [hashlib.sha256(a).digest(), hashlib.sha256(b).digest()]
    check = lambda proof, ct, digest: api.verify_digest_chunked(vk, api.CIRCUIT_AES_CTR, [proof], ct, [model.IV, digest], header=icb)[0]
    assert check(proofs[1], ct_b, hashlib.sha256(a).digest()) == [False]                                                      # B's proof does not carry A's digest
    assert check(proofs[1], ct_b, hashlib.sha256(b).digest()) == [True] and check(proofs[0], ct_a, hashlib.sha256(a).digest()) == [True]


@pytest.mark.parametrize("shape", WITNESS_SHAPES, ids=ids)
def test_witness(api, dg_key, shape):
    """the witness satisfies every row of the digest circuit; its instance is One, the mode's public bits and the key tag from the model, H_in, then the model's H_out;
    one flipped H_out bit is exactly one unsatisfied row, one flipped H_in bit at least one; the trace's digest head holds both states"""
    mode, key_bits, length, alen, blocks, kind, prefix = shape
    base = shape[:4]
    pk, _ = dg_key(*shape)
    info, dinfo = pk.info(), pk.digest_info()
    assert pk.key_tag_blocks() == blocks and dinfo["compressions"] == model.compressions(kind, length) and dinfo["offset"] % 16 == 0
    assert pk.mode() == (kind_of(api, mode), {"ecb": 0, "cbc": 16, "ctr": 16, "gcm": 12 + alen}[mode])
    for seed in (0xD16 + length, 0xD17 + key_bits):
        msg, key, header, extra = statement(base, seed)
        h_in = h_in_of(shape, seed)
        z = pk.witness_digest(msg, key, header_of(shape, extra), h_in)
        tr = pk.debug_fetch("trace")
        assert len(z) == info["instance"] + info["witness"] and set(z) <= {0, 1}
        want_out = model.h_out(kind, msg, h_in, prefix)
        public = header + model_public(base, msg, key, extra) + (tag_of(api, shape, key) or b"") + (h_in or model.IV) + want_out
        assert 1 + 8 * len(public) == info["raw_instance"]
        assert z[0] == 1
        assert z[1:info["raw_instance"] - 512] == bits(public[:-64])          # the mode's and the tag's bits: where they were
        assert z[info["raw_instance"] - 512:info["raw_instance"]] == bits(public[-64:])      # the instance tail: H_in, H_out
        assert not any(z[info["raw_instance"]:info["instance"]])
        bad = unsatisfied_rows(api, shape, z)
        assert len(bad) == 0, bad[:10]
        zf = bytearray(z)                                                    # the checker itself can fail
        zf[info["raw_instance"] - 3] ^= 1
        assert len(unsatisfied_rows(api, shape, bytes(zf))) == 1              # an H_out bit: its equality row
        zf = bytearray(z)
        zf[info["raw_instance"] - 512 + 77] ^= 1
        assert len(unsatisfied_rows(api, shape, bytes(zf))) >= 1              # an H_in bit: every row it enters
        off = dinfo["offset"]
        assert len(tr) == off + 64 + 4032 * dinfo["compressions"]
        assert tr[off:off + 32] == (h_in or model.IV) and tr[off + 32:off + 64] == want_out
        if kind == "final" and prefix == 0 and h_in is None:
            assert want_out == hashlib.sha256(msg).digest()


@pytest.mark.parametrize("shape", PROVING_SHAPES, ids=ids)
def test_lone_proof(api, dg_key, shape):
    mode, key_bits, length, alen, blocks, kind, prefix = shape
    base = shape[:4]
    pk, vk = dg_key(*shape)
    msg, key, header, extra = statement(base, 0x10E + length + key_bits)
    other_msg = statement(base, 0x5EED + length)[0]
    h_in = h_in_of(shape, 1)
    hdr = header_of(shape, extra)
    cts, gtags, h_outs, proofs = pk.encrypt_digest_batch([msg], [key], headers=None if hdr is None else [hdr], h_ins=None if h_in is None else [h_in], zk_seed=bytes(range(3, 35)))
    pub = model_public(base, msg, key, extra)
    ct, gtag, h_out, proof = cts[0], gtags[0], h_outs[0], proofs[0]
    assert ct == pub[:length] and (gtag is None if mode != "gcm" else gtag == pub[length:])
    assert h_out == model.h_out(kind, msg, h_in, prefix)
    tag = tag_of(api, shape, key)
    check = lambda c=ct, hi=h_in, ho=h_out: verify_lone(api, vk, shape, proof, extra, c, gtag, tag, hi, ho)
    assert check() is True
    assert check(ho=flip(h_out, 31)) is False and check(ho=flip(h_out, 0, 0x01)) is False
    assert check(hi=flip(h_in or model.IV, 5)) is False
    assert check(ho=model.h_out(kind, other_msg, h_in, prefix)) is False
    other_ct = model_public(base, other_msg, key, extra)[:length]                                    # another message's ciphertext paired with the right digest
    assert other_ct != ct and check(c=other_ct) is False


def test_chunked_job_ecb(api, dg_key):
    shape = ("ecb", 128, 64, 0, 0, "chain", 0)
    pk, vk = dg_key(*shape)
    rs = np.random.RandomState(0xC4A1)
    msg, key = rs.bytes(192), rs.bytes(16)
    pk.set_contexts(2)
    try:
        ct, states, proofs = pk.encrypt_digest_chunked(msg, key, zk_seed=bytes(range(32)))
    finally:
        pk.set_contexts(0)
    assert ct == ks_ecb(msg, key) and len(proofs) == 3
    assert states == [model.chain(msg[:64 * j]) for j in range(4)]
    accepted, digest = api.verify_digest_chunked(vk, api.CIRCUIT_AES, proofs, ct, states)
    assert accepted == [True] * 3 and digest == hashlib.sha256(msg).digest()
    # two chunks swapped, proofs and ciphertext slices together: ECB alone accepts that, the chain does not
    swapped_ct, swapped = ct[64:128] + ct[:64] + ct[128:], [proofs[1], proofs[0], proofs[2]]
    accepted, digest = api.verify_digest_chunked(vk, api.CIRCUIT_AES, swapped, swapped_ct, states)
    assert accepted == [False, False, True] and digest is None
    assert api.verify_digest_chunked(vk, api.CIRCUIT_AES, [proofs[1]], ct[64:128], states[1:3])[0] == [True]      # any chunk alone, from its two states


def test_ctr_job_split_over_two_calls(api, dg_key):
    shape = ("ctr", 128, 64, 0, 0, "chain", 0)
    pk, vk = dg_key(*shape)
    rs = np.random.RandomState(0xC7C7)
    msg, key, icb = rs.bytes(192), rs.bytes(16), b"\xff" * 15 + b"\xfd"                               # the counter wraps inside the job
    seed = bytes(range(1, 33))
    ct1, st1, p1 = pk.encrypt_digest_chunked(msg[:64], key, header=icb, zk_seed=seed)
    ct2, st2, p2 = pk.encrypt_digest_chunked(msg[64:], key, header=api.ctr_counter_add(icb, 4), h_in=st1[-1], zk_seed=seed, first_proof_index=1)
    assert ct1 + ct2 == ks_ctr(msg, key, icb) and st1[-1] == st2[0]
    states = st1 + st2[1:]
    accepted, digest = api.verify_digest_chunked(vk, api.CIRCUIT_AES_CTR, p1 + p2, ct1 + ct2, states, header=icb)
    assert accepted == [True] * 3 and digest == hashlib.sha256(msg).digest()
    wrong = [states[0], states[2], states[1], states[3]]
    assert api.verify_digest_chunked(vk, api.CIRCUIT_AES_CTR, p1 + p2, ct1 + ct2, wrong, header=icb)[0] == [False, False, False]


def test_gcm_batch_under_one_key_tag(api, dg_key):
    shape = ("gcm", 256, 17, 5, 1, "final", 64)
    pk, vk = dg_key(*shape)
    recs = [statement(shape[:4], 0xBA8 + i) for i in range(3)]
    session = recs[0][1]
    msgs, ivs, aads = [r[0] for r in recs], [r[3][0] for r in recs], [r[3][1] for r in recs]
    h_ins = [model.chain(np.random.RandomState(0xF00 + i).bytes(64)) for i in range(3)]              # each record's own 64-byte prefix
    pk.set_contexts(2)
    try:
        cts, gtags, h_outs, proofs = pk.encrypt_digest_batch(msgs, [session] * 3, headers=[iv + aad for iv, aad in zip(ivs, aads)], h_ins=h_ins, zk_seed=bytes(range(32)))
    finally:
        pk.set_contexts(0)
    tag = api.key_tag(session, 1)
    for i in range(3):
        assert (cts[i], gtags[i]) == ks_gcm(msgs[i], session, ivs[i], aads[i])
        assert h_outs[i] == model.finish(h_ins[i], 64, msgs[i])
    under = lambda outs, t=tag: [api.verify_encryption_gcm_digest(vk, proofs[i], ivs[i], aads[i], cts[i], gtags[i], outs[i], h_in=h_ins[i], key_tag=t) for i in range(3)]
    assert under(h_outs) == [True, True, True]
    assert under([h_outs[1], h_outs[0], h_outs[2]]) == [False, False, True]
    assert under(h_outs, api.key_tag(recs[1][1], 1)) == [False, False, False]


def test_digest_and_plain_keys_do_not_mix(api, dg_key):
    """every entry point from before refuses a digest key with a message that names the _digest_ entries; the digest entries refuse a key without one"""
    rs = np.random.RandomState(0x3D3)
    key, icb = rs.bytes(16), rs.bytes(16)
    pk, _ = dg_key("ecb", 128, 64, 0, 0, "chain", 0)
    m64 = rs.bytes(64)
    for call in (lambda: api.encrypt(m64, key, pk), lambda: pk.witness(m64, key), lambda: pk.encrypt_chunked(m64, key), lambda: pk.encrypt_batch([m64], [key])):
        with pytest.raises(api.ZkAesError, match="_digest_"):
            call()
    pk, _ = dg_key("ctr", 128, 56, 0, 0, "final", 0)
    m56 = rs.bytes(56)
    for call in (lambda: api.encrypt_ctr(m56, key, icb, pk), lambda: pk.witness_ctr(m56, key, icb)):
        with pytest.raises(api.ZkAesError, match="_digest_"):
            call()
    with pytest.raises(api.ZkAesError, match="chain key"):                                          # a final key proves one lone tail
        pk.encrypt_digest_chunked(m56, key, header=icb)
    pk, _ = dg_key("gcm", 256, 17, 5, 1, "final", 64)
    k32, iv, aad, m17 = rs.bytes(32), rs.bytes(12), rs.bytes(5), rs.bytes(17)
    for call in (lambda: api.encrypt_gcm(m17, k32, iv, aad, pk), lambda: pk.witness_gcm(m17, k32, iv, aad), lambda: pk.encrypt_gcm_batch([m17], [k32], [iv], [aad])):
        with pytest.raises(api.ZkAesError, match="_digest_"):
            call()
    plain_pk, plain_vk = dg_key("ctr", 128, 56, 0, 0, None, 0)
    assert plain_pk.digest_info() == {"kind": None, "prefix": 0, "compressions": 0, "offset": 0}
    for call in (lambda: plain_pk.witness_digest(m56, key, icb), lambda: plain_pk.encrypt_digest_batch([m56], [key], headers=[icb])):
        with pytest.raises(api.ZkAesError, match="digest"):
            call()
    # a plain proof never passes a digest verifier, whichever key checks it
    ct, proof = api.encrypt_ctr(m56, key, icb, plain_pk)
    for k in (plain_vk, dg_key("ctr", 128, 56, 0, 0, "final", 0)[1]):
        try:
            got = api.verify_digest_chunked(k, api.CIRCUIT_AES_CTR, [proof], ct, [model.IV, hashlib.sha256(m56).digest()], header=icb)[0]
        except api.ZkAesError:
            got = [False]
        assert got == [False]


def test_plain_proof_bytes_do_not_move(api, dg_key, vectors):
    """with digest keys alive in the process, an AES-128 ECB key over the default SRS literals still emits the committed proof bytes under the reference's fixed prover seed"""
    dg_key("ecb", 128, 64, 0, 0, "chain", 0)
    pk, vk = api.synthesize_keys(16, flags=api.KEY_NO_TABLES)
    try:
        assert pk.digest_info()["kind"] is None
        proof = api.encrypt(bytes(vectors["plaintext"]), bytes(vectors["key"]), pk, zk_seed=None)  # (None = the reference's fixed prover stream: byte parity)
        gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
        assert proof == open(os.path.join(gold, "gpu_aes16_proof.bin"), "rb").read()
        assert vk.to_bytes() == open(os.path.join(gold, "gpu_aes16_vk.bin"), "rb").read()
    finally:
        pk.free()
