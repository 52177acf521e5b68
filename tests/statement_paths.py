"""The calls that pin every host statement path: one entry per (mode, shape) of the prover's lone, batch, chunked and segment forms, each made twice -- under a caller's
seed at first_proof_index = 3 and under the reference's fixed prover stream (PARITY) -- and answered with the SHA-256 of every proof and every returned ciphertext, tag,
state and commitment in hex.  tests/golden/make_statement_paths.py records the answers into tests/golden/statement_paths.json; tests/test_gpu_statement_paths.py replays
the same calls and asserts equality.  Every key lives over an SRS sized from its circuit's own counts, without window tables, and is freed behind its entry.

The shapes are the smallest that reach every branch of the statement layer: a chunked ECB job and a batch, CBC over three chunks (iv, then two ciphertext blocks), CTR
over three chunks whose counter carries across byte 8, a lone CTR slice that is no whole block, lone and batched GCM, chain digests of the three chunked modes, a final
digest over GCM, a CBC key with two key-tag blocks, CTR-256, and a 40-byte GCM record as head, mid and tail segments, whole and split at first_segment = 1.
"""
import hashlib

import numpy as np

SEED = bytes(range(32))
FIRST_INDEX = 3
ICB_CARRY = bytes(8) + b"\xff" * 7 + b"\xfe"                                # + 2 carries across byte 8


def sha(proofs):
    return [hashlib.sha256(p).hexdigest() for p in proofs]


def hexes(items):
    return [None if x is None else bytes(x).hex() for x in items]


def small_srs(*infos):
    """SRS literals that hold every one of the circuits: (constraints, instance, non-zeros), the largest of each"""
    return tuple(max(int(v) for v in col) for col in zip(*[(ci["constraints"], ci["instance"], ci["nnz_a"] + ci["nnz_b"] + ci["nnz_c"]) for ci in infos]))


def seeds(api):
    """(label, keywords of a multi-proof call, zk_seed of a lone call: None is the fixed stream there)"""
    return [("seeded", dict(zk_seed=SEED, first_proof_index=FIRST_INDEX), SEED), ("parity", dict(zk_seed=api.PARITY), None)]


def key_for(api, circuit, length, alen=0, key_bits=128, key_tag_blocks=0, digest=None):
    srs = small_srs(api.circuit_info(circuit, length, alen, key_bits, key_tag_blocks, digest, 0))
    if circuit == api.CIRCUIT_AES_GCM:
        return api.synthesize_keys_gcm(length, alen, srs=srs, flags=api.KEY_NO_TABLES, key_bits=key_bits, key_tag_blocks=key_tag_blocks, digest=digest)
    return api.synthesize_keys(length, circuit=circuit, srs=srs, flags=api.KEY_NO_TABLES, key_bits=key_bits, key_tag_blocks=key_tag_blocks, digest=digest)


def ecb(api, rs):
    pk, vk = key_for(api, api.CIRCUIT_AES, 16)
    msg, key, key2 = rs.bytes(32), rs.bytes(16), rs.bytes(16)
    out = {}
    for label, kw, _ in seeds(api):
        chunked = pk.encrypt_chunked(msg, key, **kw)
        batch = pk.encrypt_batch([msg[:16], msg[16:]], [key, key2], **kw)
        cts = [api.ecb_ciphertext(msg[:16], key), api.ecb_ciphertext(msg[16:], key), api.ecb_ciphertext(msg[16:], key2)]
        out[label] = {"chunked": sha(chunked), "batch": sha(batch),
                      "accepted": [api.verify_encryption(vk, p, ct) for p, ct in zip(chunked + batch[1:], cts)]}
    pk.free()
    return out


def cbc(api, rs, n_chunks=3, key_tag_blocks=0):
    pk, vk = key_for(api, api.CIRCUIT_AES_CBC, 16, key_tag_blocks=key_tag_blocks)
    msg, key, iv = rs.bytes(16 * n_chunks), rs.bytes(16), rs.bytes(16)
    out = {}
    for label, kw, _ in seeds(api):
        ct, proofs = pk.encrypt_cbc_chunked(msg, key, iv, **kw)
        if key_tag_blocks:
            accepted = api.verify_chunked_tagged(vk, api.CIRCUIT_AES_CBC, proofs, ct, api.key_tag(key, key_tag_blocks), iv=iv)
        else:
            accepted = api.verify_cbc_chunked(vk, proofs, iv, ct)
        out[label] = {"ciphertext": ct.hex(), "proofs": sha(proofs), "accepted": accepted}
    pk.free()
    return out


def ctr(api, rs, n_chunks, key_bits=128):
    pk, vk = key_for(api, api.CIRCUIT_AES_CTR, 16, key_bits=key_bits)
    msg, key = rs.bytes(16 * n_chunks), rs.bytes(key_bits // 8)
    out = {}
    for label, kw, _ in seeds(api):
        ct, proofs = pk.encrypt_ctr_chunked(msg, key, ICB_CARRY, **kw)
        out[label] = {"ciphertext": ct.hex(), "proofs": sha(proofs), "accepted": api.verify_ctr_chunked(vk, proofs, ICB_CARRY, ct)}
    pk.free()
    return out


def ctr_lone(api, rs):
    pk, vk = key_for(api, api.CIRCUIT_AES_CTR, 17)
    msg, key, icb = rs.bytes(17), rs.bytes(16), rs.bytes(16)
    out = {}
    for label, _, lone_seed in seeds(api):
        ct, proof = api.encrypt_ctr(msg, key, icb, pk, zk_seed=lone_seed)
        out[label] = {"ciphertext": ct.hex(), "proofs": sha([proof]), "accepted": [api.verify_encryption_ctr(vk, proof, icb, ct)]}
    pk.free()
    return out


def gcm(api, rs):
    pk, vk = key_for(api, api.CIRCUIT_AES_GCM, 17, 5)
    msgs, keys, ivs, aads = [rs.bytes(17) for _ in range(2)], [rs.bytes(16) for _ in range(2)], [rs.bytes(12) for _ in range(2)], [rs.bytes(5) for _ in range(2)]
    out = {}
    for label, kw, lone_seed in seeds(api):
        ct, tag, proof = api.encrypt_gcm(msgs[0], keys[0], ivs[0], aads[0], pk, zk_seed=lone_seed)
        cts, tags, proofs = pk.encrypt_gcm_batch(msgs, keys, ivs, aads, **kw)
        out[label] = {"lone": {"ciphertext": ct.hex(), "tag": tag.hex(), "proofs": sha([proof]), "accepted": [api.verify_encryption_gcm(vk, proof, ivs[0], aads[0], ct, tag)]},
                      "batch": {"ciphertexts": hexes(cts), "tags": hexes(tags), "proofs": sha(proofs),
                                "accepted": [api.verify_encryption_gcm(vk, proofs[i], ivs[i], aads[i], cts[i], tags[i]) for i in range(2)]}}
    pk.free()
    return out


def chain(api, rs, circuit):
    pk, vk = key_for(api, circuit, 64, digest="chain")
    msg, key = rs.bytes(128), rs.bytes(16)
    header = None if circuit == api.CIRCUIT_AES else ICB_CARRY if circuit == api.CIRCUIT_AES_CTR else rs.bytes(16)
    h_in = rs.bytes(32) if circuit == api.CIRCUIT_AES_CBC else None               # one mode from a state that is not the initial value
    out = {}
    for label, kw, _ in seeds(api):
        ct, states, proofs = pk.encrypt_digest_chunked(msg, key, header=header, h_in=h_in, **kw)
        accepted, digest = api.verify_digest_chunked(vk, circuit, proofs, ct, states, header=header)
        out[label] = {"ciphertext": ct.hex(), "states": hexes(states), "proofs": sha(proofs), "accepted": accepted, "digest": None if digest is None else digest.hex()}
    pk.free()
    return out


def final_gcm(api, rs):
    pk, vk = key_for(api, api.CIRCUIT_AES_GCM, 17, 5, digest="final")
    msg, key, iv, aad = rs.bytes(17), rs.bytes(16), rs.bytes(12), rs.bytes(5)
    out = {}
    for label, kw, _ in seeds(api):
        cts, tags, h_outs, proofs = pk.encrypt_digest_batch([msg], [key], headers=[iv + aad], **kw)
        out[label] = {"ciphertexts": hexes(cts), "tags": hexes(tags), "states": hexes(h_outs), "proofs": sha(proofs),
                      "accepted": [api.verify_encryption_gcm_digest(vk, proofs[0], iv, aad, cts[0], tags[0], h_outs[0])]}
    pk.free()
    return out


def segments(api, rs):
    """c = 1, a 40-byte record with 5 bytes of aad: head, mid and an 8-byte tail over one SRS that holds all three"""
    shapes = [("head", 1, 5), ("mid", 1, 0), ("tail", 8, 0)]
    srs = small_srs(*[api.circuit_info_gcm_segment(role, units, aad) for role, units, aad in shapes])
    keys = [api.synthesize_keys_gcm_segment(role, units, aad, srs=srs, flags=api.KEY_NO_TABLES) for role, units, aad in shapes]
    pks, vks = tuple(k[0] for k in keys), tuple(k[1] for k in keys)
    msg, key, iv, aad, salts = rs.bytes(40), rs.bytes(16), rs.bytes(12), rs.bytes(5), [rs.bytes(16) for _ in range(2)]
    out = {}
    for label, seed in (("seeded", SEED), ("parity", api.PARITY)):
        ct, tag, coms, proofs = api.encrypt_gcm_segments(msg, key, iv, aad, pks, salts=salts, zk_seed=seed)
        ct2, tag2, coms2, rest = api.encrypt_gcm_segments(msg, key, iv, aad, pks, salts=salts, first_segment=1, zk_seed=seed)
        out[label] = {"whole": {"ciphertext": ct.hex(), "tag": tag.hex(), "commitments": hexes(coms), "proofs": sha(proofs),
                                "accepted": api.verify_gcm_segments(vks, proofs, iv, aad, ct, tag, coms, 1)},
                      "from_1": {"ciphertext": ct2.hex(), "tag": tag2.hex(), "commitments": hexes(coms2), "proofs": sha(rest)}}
    for pk in pks:
        pk.free()
    return out


ENTRIES = [
    ("ecb_16x2_and_batch_2", lambda api, rs: ecb(api, rs)),
    ("cbc_16x3", lambda api, rs: cbc(api, rs, 3)),
    ("ctr_16x3_carry", lambda api, rs: ctr(api, rs, 3)),
    ("ctr_lone_17", lambda api, rs: ctr_lone(api, rs)),
    ("gcm_17_5_lone_and_batch_2", lambda api, rs: gcm(api, rs)),
    ("chain_ecb_64x2", lambda api, rs: chain(api, rs, api.CIRCUIT_AES)),
    ("chain_cbc_64x2", lambda api, rs: chain(api, rs, api.CIRCUIT_AES_CBC)),
    ("chain_ctr_64x2", lambda api, rs: chain(api, rs, api.CIRCUIT_AES_CTR)),
    ("final_gcm_17_5_batch_1", lambda api, rs: final_gcm(api, rs)),
    ("cbc_16x2_keytag_2", lambda api, rs: cbc(api, rs, 2, key_tag_blocks=2)),
    ("ctr256_16x2", lambda api, rs: ctr(api, rs, 2, key_bits=256)),
    ("gcm_segments_c1_40", lambda api, rs: segments(api, rs)),
]
NAMES = [name for name, _ in ENTRIES]


def run(api, name):
    """the answers of one entry; its inputs come from a stream seeded by the entry's place in the list"""
    at = NAMES.index(name)
    return ENTRIES[at][1](api, np.random.RandomState(0x57A7 + at))
