"""Selective disclosure on the GPU: k_reveal_trace behind each mode's trace kernel(s), the tag kernel and the digest kernel; the witness against the reveal
circuit's own matrices; lone, chunked and batch proofs checked against (mask, revealed); batch verification at the larger |X|; and the gap this feature exists to close.

A key synthesized with reveal = True proves revealed[i] = mask_i ? M[i] : 0 beside its mode's statement, its key tag and its digest, for a mask chosen per proof; the
mask and the revealed bytes are the last public inputs.  Correctness rests on a Python one-liner for the masking, on r1cs_audit's value propagation over the reveal rows
(and over the whole system at the smallest shape), and on a row-by-row check of (A z) o (B z) = C z in int64 numpy over the matrices circuit_matrix(..., reveal=True)
returns.  The shapes are the emulator's (tests/reveal_trace_emu.cpp): one lane (ECB-128 16 B), a lone byte and a second lane of one byte behind a tag slot and a digest
region (CTR-128 1 and 17 B, T = 1, final), two lanes behind the CBC tail at NK = 6 (CBC-192 32 B), the region behind the GHASH tail at NK = 8 (GCM-256 (17, 5)), four lanes
and 8 mask bytes behind two tag slots and a chain digest (ECB-256 64 B).  Every key is synthesized over an SRS sized from its own circuit, without window tables, once per
module.  Messages have no zero byte where a test flips a mask bit: over a zero byte, mask bit 0 and mask bit 1 state the same revealed byte, and both are true.
"""
import os

import numpy as np
import pytest

import r1cs_audit as ra
import sha256_model as model
from test_gpu_keysize import bits, flip, kind_of, model_public, statement
from test_keysize_host import ks_ctr, ks_ecb, ks_gcm

pytestmark = pytest.mark.gpu

# (mode, key_bits, L, A, T, digest)
SHAPES = [("ecb", 128, 16, 0, 0, None), ("ctr", 128, 1, 0, 1, "final"), ("ctr", 128, 17, 0, 1, "final"), ("cbc", 192, 32, 0, 0, None), ("gcm", 256, 17, 5, 0, None), ("ecb", 256, 64, 0, 2, "chain")]
PROVING_SHAPES = [("ecb", 128, 16, 0, 0, None), ("ctr", 128, 17, 0, 1, "final"), ("cbc", 192, 32, 0, 0, None), ("gcm", 128, 1, 0, 0, None), ("gcm", 256, 17, 5, 1, None)]
MASKS = ["zero", "ones", "first", "last", "15+16", "alternating"]
_keys, _mats = {}, {}


def mask_of(api, name, n):
    return api.reveal_mask({"zero": [], "ones": range(n), "first": [0], "last": [n - 1], "15+16": [i for i in (15, 16) if i < n], "alternating": range(0, n, 2)}[name], n)


def masked(msg, mask):
    """the one-liner the library's masking is held against"""
    return bytes(msg[i] if (mask[i // 8] >> (i % 8)) & 1 else 0 for i in range(len(msg)))


@pytest.fixture(scope="module")
def rv_key(api):
    """(pk, vk) for (mode, key_bits, L, A, T, digest) and a reveal flag over an SRS sized from the circuit's own counts, no window tables; one per shape for the module"""
    def get(shape, reveal=True):
        mode, key_bits, length, alen, blocks, kind = shape
        at = shape + (reveal,)
        if at not in _keys:
            ci = api.circuit_info(kind_of(api, mode), length, alen, key_bits, blocks, kind, 0, reveal=reveal)
            srs = (int(ci["constraints"]), int(ci["instance"]), int(ci["nnz_a"] + ci["nnz_b"] + ci["nnz_c"]))
            if mode == "gcm":
                _keys[at] = api.synthesize_keys_gcm(length, alen, srs=srs, flags=api.KEY_NO_TABLES, key_bits=key_bits, key_tag_blocks=blocks, digest=kind, reveal=reveal)
            else:
                _keys[at] = api.synthesize_keys(length, circuit=kind_of(api, mode), srs=srs, flags=api.KEY_NO_TABLES, key_bits=key_bits, key_tag_blocks=blocks, digest=kind, reveal=reveal)
            info = _keys[at][0].reveal_info()
            assert (info["reveal"], info["message_bytes"], info["mask_bytes"]) == ((True, length, (length + 7) // 8) if reveal else (False, 0, 0))
        return _keys[at]
    yield get
    for pk, _ in _keys.values():
        pk.free()
    _keys.clear()
    _mats.clear()


def matrices(api, shape):
    mode, key_bits, length, alen, blocks, kind = shape
    if shape not in _mats:
        _mats[shape] = [api.circuit_matrix(kind_of(api, mode), length, which, alen, key_bits, blocks, kind, 0, reveal=True) for which in range(3)]
    return _mats[shape]


def side_sums(mats, zz):
    out = []
    for rowptr, col, coeff in mats:
        assert len(zz) == len(rowptr) - 1                                    # square after padding
        cs = np.concatenate([[0], np.cumsum(coeff * zz[col])])
        out.append(cs[rowptr[1:].astype(np.int64)] - cs[rowptr[:-1].astype(np.int64)])
    return out


def unsatisfied_rows(api, shape, z):
    """indices of the rows where (A z) * (B z) != C z, in int64 (the sums' coefficients reach 2^34 and z is 0/1: no overflow)"""
    a, b, c = side_sums(matrices(api, shape), np.frombuffer(z, dtype=np.uint8).astype(np.int64))
    return np.nonzero(a * b != c)[0]


def unnoticed(api, shape, z, variables):
    """the (variable, replacement) pairs among `variables` x (1 - z, 2, -1) that leave every row satisfied: r1cs_audit.unperturbable's arithmetic over these variables
    only -- for each, the rows that hold it are recomputed as A z + a d, B z + b d, C z + c d.  |z| <= 2 and the variables' coefficients stay below 2^32: int64 is exact"""
    mats = matrices(api, shape)
    zz = np.frombuffer(z, dtype=np.uint8).astype(np.int64)
    sums = side_sums(mats, zz)
    n = len(zz)
    pick = np.zeros(n, dtype=bool)
    pick[list(variables)] = True
    keys, sides, coeffs = [], [], []
    for s, (rowptr, col, coeff) in enumerate(mats):
        at = np.nonzero(pick[col])[0]
        rows = np.searchsorted(rowptr, at, side="right") - 1
        keys.append(col[at].astype(np.int64) * n + rows)
        sides.append(np.full(len(at), s))
        coeffs.append(coeff[at])
    keys, sides, coeffs = np.concatenate(keys), np.concatenate(sides), np.concatenate(coeffs)
    uniq, inv = np.unique(keys, return_inverse=True)
    pv, pr = uniq // n, uniq % n
    c = np.zeros((3, len(uniq)), dtype=np.int64)
    np.add.at(c, (sides, inv), coeffs)
    assert set(pv.tolist()) == set(variables)                                # every one of them occurs in a row
    left = []
    for name, new in (("1 - z", 1 - zz), ("2", np.full_like(zz, 2)), ("-1", np.full_like(zz, -1))):
        d = (new - zz)[pv]
        na, nb, nc = (sums[s][pr] + c[s] * d for s in range(3))
        broken = np.zeros(n, dtype=bool)
        broken[pv[na * nb != nc]] = True
        left += [(int(v), name) for v in variables if not broken[v]]
    return left


def reveal_columns(api, shape):
    """(first instance column of the mask, of revealed, first witness column of the message, the plain circuit's raw row count) from the statement's definition"""
    mode, key_bits, length, alen, blocks, kind = shape
    if ("columns", shape) not in _mats:
        plain = api.circuit_info(kind_of(api, mode), length, alen, key_bits, blocks, kind)
        info = api.circuit_info(kind_of(api, mode), length, alen, key_bits, blocks, kind, 0, reveal=True)
        mb = (length + 7) // 8
        assert info["raw_instance"] == plain["raw_instance"] + 8 * mb + 8 * length
        _mats[("columns", shape)] = (int(plain["raw_instance"]), int(plain["raw_instance"]) + 8 * mb, int(info["instance"]), int(plain["raw_constraints"]))
    return _mats[("columns", shape)]


def replay_reveal_rows(api, shape, mask, msg):
    """the revealed bits by r1cs_audit's value propagation from the reveal rows of the matrices alone -- One, the mask's bits and the message's bits seeded; no trace, no
    descriptor, no layout"""
    mode, key_bits, length, alen, blocks, kind = shape
    mask_at, rev_at, msg_at, r0 = reveal_columns(api, shape)
    mb = (length + 7) // 8
    r1 = r0 + 16 * mb + 15 * length
    sub = []
    for rowptr, col, coeff in matrices(api, shape):
        lo, hi = int(rowptr[r0]), int(rowptr[r1])
        sub.append((rowptr[r0:r1 + 1].astype(np.int64) - lo, col[lo:hi], coeff[lo:hi]))
    s = ra.System(sub, len(matrices(api, shape)[0][0]) - 1)
    seeded = {0: 1}
    seeded.update(zip(range(mask_at, mask_at + 8 * mb), bits(mask)))
    seeded.update(zip(range(msg_at, msg_at + 8 * length), bits(msg)))
    z, _ = ra.solve(s, seeded)
    return bytes(z[rev_at:rev_at + 8 * length])


def ids(shape):
    return "%s%d-L%d-A%d-T%d-%s" % shape


def nonzero_message(shape, seed):
    msg, key, header, extra = statement(shape[:4], seed)
    return bytes(b | 1 for b in msg), key, header, extra


def header_of(shape, extra):
    return {"ecb": None, "cbc": extra[0] if extra else None, "ctr": extra[0] if extra else None}.get(shape[0], b"".join(extra))


def verify_lone(api, vk, shape, proof, extra, ct, gtag, key_tag, h_in, h_out, mask, revealed):
    mode = shape[0]
    if mode == "gcm":
        return api.verify_encryption_gcm_reveal(vk, proof, extra[0], extra[1], ct, gtag, mask, revealed, key_tag=key_tag, h_out=h_out, h_in=h_in)
    states = None if h_out is None else [model.IV if h_in is None else h_in, h_out]
    return api.verify_reveal_chunked(vk, kind_of(api, mode), [proof], ct, mask, revealed, header=None if mode == "ecb" else extra[0], key_tag=key_tag, states=states) == [True]


def test_the_gap_this_closes(api, rv_key):
    """without reveal no verifier input names a plaintext byte: two different messages both verify and the verifier's whole input is (icb, ciphertext).  With a reveal key
    the proof verifies under reveal_bytes(M, mask) and under nothing else"""
    base = ("ctr", 128, 17, 0, 0, None)
    plain_pk, plain_vk = rv_key(base, False)
    pk, vk = rv_key(base)
    _, key, icb, _ = statement(base[:4], 0x7E1)
    rs = np.random.RandomState(0x7E2)
    a, b = bytes(x | 1 for x in rs.bytes(17)), bytes(x | 1 for x in rs.bytes(17))
    ct_a, ct_b = ks_ctr(a, key, icb), ks_ctr(b, key, icb)
    proof_a, proof_b = api.encrypt_ctr(a, key, icb, plain_pk)[1], api.encrypt_ctr(b, key, icb, plain_pk)[1]
    assert api.verify_encryption_ctr(plain_vk, proof_a, icb, ct_a) is True and api.verify_encryption_ctr(plain_vk, proof_b, icb, ct_b) is True      # the gap
    assert plain_vk.verify(proof_a, bits(icb + ct_a)) is True                # the verifier's whole input: no bit of it is a plaintext bit
    mask = api.reveal_mask(range(4, 12), 17)
    cts, _, h_outs, revealed, proofs = pk.encrypt_reveal_batch([a, b], [key, key], [mask, mask], headers=[icb, icb], zk_seed=bytes(range(32)))
    assert cts == [ct_a, ct_b] and h_outs == [None, None]
    assert revealed == [api.reveal_bytes(a, mask), api.reveal_bytes(b, mask)] == [masked(a, mask), masked(b, mask)] and revealed[0][4:12] == a[4:12] and not any(revealed[0][:4] + revealed[0][12:])
    check = lambda proof, ct, m, r: api.verify_reveal_chunked(vk, api.CIRCUIT_AES_CTR, [proof], ct, m, r, header=icb)
    assert check(proofs[0], ct_a, mask, revealed[0]) == [True] and check(proofs[1], ct_b, mask, revealed[1]) == [True]
    assert check(proofs[0], ct_a, mask, flip(revealed[0], 7, 0x01)) == [False]                       # one revealed byte changed
    cleared = api.reveal_mask(range(5, 12), 17)
    assert check(proofs[0], ct_a, cleared, masked(a, cleared)) == [False]                           # one mask bit cleared and its byte zeroed
    wider = api.reveal_mask(range(4, 13), 17)
    assert a[12] != 0 and check(proofs[0], ct_a, wider, revealed[0]) == [False]                     # one mask bit set on a non-zero byte, revealed left 0
    assert check(proofs[0], ct_b, mask, revealed[0]) == [False]                                     # under another message's ciphertext
    assert check(proofs[0], ct_a, mask, revealed[1]) == [False]


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_witness_and_trace(api, rv_key, shape):
    """for every mask of the emulator: the device z satisfies every row; its reveal columns equal the replay of the reveal rows from the matrices alone; every other
    column, and the trace ahead of the region, equal the R = 0 key's; the region is (mask, zeros, revealed, zeros); every variable of a reveal row, replaced by 1 - z, 2
    and -1, leaves a row unsatisfied.  At the smallest shape the whole z also equals the solver's over the whole system"""
    mode, key_bits, length, alen, blocks, kind = shape
    pk, _ = rv_key(shape)
    plain_pk, _ = rv_key(shape, False)
    info, pinfo, rinfo = pk.info(), plain_pk.info(), pk.reveal_info()
    mb = (length + 7) // 8
    mask_at, rev_at, msg_at, _ = reveal_columns(api, shape)
    assert rinfo["offset"] % 16 == 0 and rinfo["mask_bytes"] == mb and info["raw_witness"] == pinfo["raw_witness"]
    msg, key, header, extra = nonzero_message(shape, 0x4E7 + length + key_bits)
    h_in = np.random.RandomState(length).bytes(32) if kind == "chain" else None
    hdr = header_of(shape, extra)
    if kind:
        zp = plain_pk.witness_digest(msg, key, hdr, h_in)
    else:
        zp = {"ecb": lambda: plain_pk.witness(msg, key), "cbc": lambda: plain_pk.witness_cbc(msg, key, extra[0]), "ctr": lambda: plain_pk.witness_ctr(msg, key, extra[0]),
              "gcm": lambda: plain_pk.witness_gcm(msg, key, extra[0], extra[1])}[mode]()
    plain_trace = plain_pk.debug_fetch("trace")
    for name in MASKS:
        mask = mask_of(api, name, length)
        z = pk.witness_reveal(msg, key, mask, hdr, h_in)
        tr = pk.debug_fetch("trace")
        want = masked(msg, mask)
        assert len(z) == info["instance"] + info["witness"] and set(z) <= {0, 1}
        assert len(unsatisfied_rows(api, shape, z)) == 0, name
        # the reveal columns: the replay of the reveal rows, the one-liner, the library's host masking
        assert z[rev_at:rev_at + 8 * length] == replay_reveal_rows(api, shape, mask, msg) == bits(want) == bits(api.reveal_bytes(msg, mask)), name
        assert z[mask_at:rev_at] == bits(mask) and rev_at + 8 * length == info["raw_instance"] and not any(z[info["raw_instance"]:info["instance"]])
        assert z[msg_at:msg_at + 8 * length] == bits(msg)
        # everything else is the R = 0 key's witness, column for column, and the trace ahead of the region its trace, byte for byte
        assert z[:mask_at] == zp[:mask_at] and z[info["instance"]:info["instance"] + info["raw_witness"]] == zp[pinfo["instance"]:pinfo["instance"] + pinfo["raw_witness"]]
        off = rinfo["offset"]
        assert tr[:len(plain_trace)] == plain_trace and off == (len(plain_trace) + 15) // 16 * 16 and not any(tr[len(plain_trace):off])
        pad = lambda data: data + bytes(-len(data) % 16)
        assert tr[off:] == pad(mask) + pad(want), name
        # the variables of the reveal rows, one at a time
        variables = list(range(mask_at, rev_at + 8 * length)) + list(range(msg_at, msg_at + 8 * length))
        left = unnoticed(api, shape, z, variables)
        assert left == [], (name, left[:8])
    if shape == SHAPES[0]:
        from test_r1cs_audit_reveal import RevealShape
        from test_r1cs_audit import replay
        sh = RevealShape(mode, key_bits, length)
        mask = mask_of(api, "alternating", length)
        full, s, _, _ = replay_whole(api, sh, replay, msg, key, mask)
        dev = pk.witness_reveal(msg, key, mask, hdr, h_in)
        real = s.occurs
        differ = np.nonzero((np.frombuffer(dev, dtype=np.uint8).astype(np.int64) != np.array(full, dtype=np.int64)) & real)[0]
        assert len(differ) == 0, differ[:8].tolist()


def replay_whole(api, sh, replay, msg, key, mask):
    """test_r1cs_audit.replay over the whole reveal system of an ECB shape: z from One, the mask and the hidden inputs alone; its outputs against the models"""
    return replay(api, sh, {"msg": msg, "key": key, "ct": ks_ecb(msg, key), "mask": mask, "revealed": masked(msg, mask)})


@pytest.mark.parametrize("shape", PROVING_SHAPES, ids=ids)
def test_lone_proof(api, rv_key, shape):
    mode, key_bits, length, alen, blocks, kind = shape
    pk, vk = rv_key(shape)
    msg, key, header, extra = nonzero_message(shape, 0x10E + length + key_bits)
    other_msg = nonzero_message(shape, 0x5EED + length)[0]
    hdr = header_of(shape, extra)
    mask = api.reveal_mask([0] if length == 1 else range(length // 3, length - length // 4), length)
    cts, gtags, h_outs, revs, proofs = pk.encrypt_reveal_batch([msg], [key], [mask], headers=None if hdr is None else [hdr], zk_seed=bytes(range(3, 35)))
    pub = model_public(shape[:4], msg, key, extra)
    ct, gtag, h_out, revealed, proof = cts[0], gtags[0], h_outs[0], revs[0], proofs[0]
    assert ct == pub[:length] and (gtag is None if mode != "gcm" else gtag == pub[length:])
    assert revealed == masked(msg, mask) and (h_out is None if kind is None else h_out == model.h_out(kind, msg, None, 0))
    tag = api.key_tag(key, blocks) if blocks else None
    check = lambda c=ct, m=mask, r=revealed: verify_lone(api, vk, shape, proof, extra, c, gtag, tag, None, h_out, m, r)
    assert check() is True
    shown = next(i for i in range(length) if (mask[i // 8] >> (i % 8)) & 1)
    assert check(r=flip(revealed, shown, 0x04)) is False
    hide = bytes(b & ~(1 << (shown % 8)) & 0xff if i == shown // 8 else b for i, b in enumerate(mask))
    assert check(m=hide, r=masked(msg, hide)) is False                                               # the byte withdrawn: another statement than the one proven
    assert check(r=masked(other_msg, mask)) is False or masked(other_msg, mask) == revealed
    if length > 1:
        hidden = next(i for i in range(length) if not (mask[i // 8] >> (i % 8)) & 1)
        show = bytes(b | (1 << (hidden % 8)) if i == hidden // 8 else b for i, b in enumerate(mask))
        assert check(m=show, r=revealed) is False                                                    # a non-zero byte declared revealed as zero
        assert check(m=show, r=masked(msg, show)) is False                                           # even its true value: the proof is of the other mask
        other_ct = model_public(shape[:4], other_msg, key, extra)[:length]
        assert other_ct != ct and check(c=other_ct) is False


def ecb_job(api, rv_key):
    shape = ("ecb", 128, 16, 0, 0, None)
    pk, vk = rv_key(shape)
    rs = np.random.RandomState(0xC4A1)
    msg, key = bytes(b | 1 for b in rs.bytes(48)), rs.bytes(16)
    mask = api.reveal_mask(range(12, 36), 48)                                                        # straddles both chunk boundaries
    if "ecb_job" not in _mats:
        pk.set_contexts(2)
        try:
            _mats["ecb_job"] = pk.encrypt_reveal_chunked(msg, key, mask, zk_seed=bytes(range(32)))
        finally:
            pk.set_contexts(0)
    return vk, msg, key, mask, _mats["ecb_job"]


def test_chunked_job_ecb(api, rv_key):
    vk, msg, key, mask, (ct, states, revealed, proofs) = ecb_job(api, rv_key)
    assert ct == ks_ecb(msg, key) and states is None and len(proofs) == 3 and revealed == masked(msg, mask) and revealed[12:36] == msg[12:36]
    assert api.verify_reveal_chunked(vk, api.CIRCUIT_AES, proofs, ct, mask, revealed) == [True] * 3
    for at, chunk in ((13, 0), (16, 1), (35, 2)):
        got = api.verify_reveal_chunked(vk, api.CIRCUIT_AES, proofs, ct, mask, flip(revealed, at, 0x80))
        assert got == [j != chunk for j in range(3)], (at, got)                                      # rejected at exactly its chunk
    assert api.verify_reveal_chunked(vk, api.CIRCUIT_AES, [proofs[1]], ct[16:32], mask[2:4], revealed[16:32]) == [True]      # any chunk alone, under its slice


def test_ctr_job_split_over_two_calls(api, rv_key):
    """16 + 16 + 1 bytes under ONE mask over 33 bytes: two chunk-proofs of a 16-byte key and the ragged tail, a lone proof of a 1-byte key under icb + 2 and mask byte 4"""
    pk, vk = rv_key(("ctr", 128, 16, 0, 0, None))
    tail_pk, tail_vk = rv_key(("ctr", 128, 1, 0, 1, "final"))
    rs = np.random.RandomState(0xC7C7)
    msg, key, icb = bytes(b | 1 for b in rs.bytes(33)), rs.bytes(16), b"\xff" * 15 + b"\xfe"          # the counter wraps inside the job
    mask = api.reveal_mask(range(10, 33), 33)                                                        # straddles both boundaries
    seed = bytes(range(1, 33))
    ct, _, revealed, proofs = pk.encrypt_reveal_chunked(msg[:32], key, mask[:4], header=icb, zk_seed=seed)
    ct1, _, rev1, p1 = pk.encrypt_reveal_chunked(msg[:16], key, mask[:2], header=icb, zk_seed=seed)
    ct2, _, rev2, p2 = pk.encrypt_reveal_chunked(msg[16:32], key, mask[2:4], header=api.ctr_counter_add(icb, 1), zk_seed=seed, first_proof_index=1)
    assert p1 + p2 == proofs and ct1 + ct2 == ct == ks_ctr(msg, key, icb)[:32] and rev1 + rev2 == revealed == masked(msg, mask)[:32]
    icb2 = api.ctr_counter_add(icb, 2)
    cts, _, h_outs, revs, tail = tail_pk.encrypt_reveal_batch([msg[32:]], [key], [mask[4:]], headers=[icb2], zk_seed=seed, first_proof_index=2)
    whole_ct, whole_rev = ct + cts[0], revealed + revs[0]
    assert whole_ct == ks_ctr(msg, key, icb) and whole_rev == masked(msg, mask) and mask[4:] == b"\x01"
    tail_check = lambda r: api.verify_reveal_chunked(tail_vk, api.CIRCUIT_AES_CTR, tail, whole_ct[32:], mask[4:], r, header=icb2, key_tag=api.key_tag(key, 1),
                                                     states=[model.IV, h_outs[0]])
    under = lambda r: api.verify_reveal_chunked(vk, api.CIRCUIT_AES_CTR, proofs, whole_ct[:32], mask[:4], r[:32], header=icb) + tail_check(r[32:])
    assert under(whole_rev) == [True] * 3
    for at, chunk in ((10, 0), (16, 1), (32, 2)):
        assert under(flip(whole_rev, at, 0x02)) == [j != chunk for j in range(3)], at


def test_gcm_batch_three_masks(api, rv_key):
    shape = ("gcm", 256, 17, 5, 1, None)
    pk, vk = rv_key(shape)
    recs = [nonzero_message(shape, 0xBA8 + i) for i in range(3)]
    session = recs[0][1]
    msgs, ivs, aads = [r[0] for r in recs], [r[3][0] for r in recs], [r[3][1] for r in recs]
    masks = [api.reveal_mask(range(0, 4), 17), api.reveal_mask([16], 17), api.reveal_mask(range(1, 17, 3), 17)]
    pk.set_contexts(2)
    try:
        cts, gtags, h_outs, revs, proofs = pk.encrypt_reveal_batch(msgs, [session] * 3, masks, headers=[iv + aad for iv, aad in zip(ivs, aads)], zk_seed=bytes(range(32)))
    finally:
        pk.set_contexts(0)
    tag = api.key_tag(session, 1)
    for i in range(3):
        assert (cts[i], gtags[i]) == ks_gcm(msgs[i], session, ivs[i], aads[i]) and revs[i] == masked(msgs[i], masks[i]) and h_outs[i] is None
    under = lambda ms, rs, t=tag: [api.verify_encryption_gcm_reveal(vk, proofs[i], ivs[i], aads[i], cts[i], gtags[i], ms[i], rs[i], key_tag=t) for i in range(3)]
    assert under(masks, revs) == [True, True, True]
    swapped = [masks[1], masks[0], masks[2]]
    assert under(swapped, [masked(msgs[i], swapped[i]) for i in range(3)]) == [False, False, True]   # true bytes under the wrong mask: not the statement proven
    assert under(masks, revs, api.key_tag(recs[1][1], 1)) == [False, False, False]


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_batch_verification(api, rv_key, device):
    """verify_chunked_batch over the ECB job: the rows end in each chunk's slice of mask and revealed.  |X| = 512 here (1 + 128 + 16 + 128 inputs), lg |X| = 9: the first
    use of the GPU public-input evaluation beyond the ciphertext-only rows of this chunk size (|X| = 256)"""
    vk, msg, key, mask, (ct, _, revealed, proofs) = ecb_job(api, rv_key)
    rows = api.chunk_public_inputs(api.CIRCUIT_AES, ct, n_chunks=3, mask=mask, revealed=revealed)
    assert [len(r) for r in rows] == [128 + 16 + 128] * 3 and rows[1] == bits(ct[16:32] + mask[2:4] + revealed[16:32])
    assert api.verify_chunked_batch(vk, api.CIRCUIT_AES, proofs, ct, device=device, mask=mask, revealed=revealed) == [True] * 3
    assert api.verify_chunked_batch(vk, api.CIRCUIT_AES, proofs, ct, device=device, mask=mask, revealed=flip(revealed, 20, 0x01)) == [True, False, True]
    with pytest.raises(api.ZkAesError, match="mask bit is 0"):
        api.verify_chunked_batch(vk, api.CIRCUIT_AES, proofs, ct, device=device, mask=mask, revealed=flip(revealed, 40, 0x01))      # byte 40 is hidden: an error, not a rejection


def test_reveal_and_plain_keys_do_not_mix(api, rv_key):
    """every entry point from before refuses a reveal key with a message that names the _reveal_ entries; the reveal entries refuse a key without it; op_lists takes
    either; no verifier accepts the other kind's proof"""
    rs = np.random.RandomState(0x3D3)
    key, icb, m16, m17 = rs.bytes(16), rs.bytes(16), rs.bytes(16), rs.bytes(17)
    pk, vk = rv_key(("ecb", 128, 16, 0, 0, None))
    for call in (lambda: api.encrypt(m16, key, pk), lambda: pk.witness(m16, key), lambda: pk.encrypt_chunked(m16, key), lambda: pk.encrypt_batch([m16], [key]),
                 lambda: pk.witness_digest(m16, key), lambda: pk.encrypt_digest_batch([m16], [key]), lambda: pk.encrypt_digest_chunked(m16, key)):
        with pytest.raises(api.ZkAesError, match="_reveal_"):
            call()
    pk17, _ = rv_key(("ctr", 128, 17, 0, 1, "final"))
    for call in (lambda: api.encrypt_ctr(m17, key, icb, pk17), lambda: pk17.witness_ctr(m17, key, icb), lambda: pk17.witness_digest(m17, key, icb),
                 lambda: pk17.encrypt_digest_batch([m17], [key], headers=[icb])):
        with pytest.raises(api.ZkAesError, match="_reveal_"):
            call()
    with pytest.raises(api.ZkAesError, match="chain key"):                                          # a final key proves one lone tail, with or without reveal
        pk17.encrypt_reveal_chunked(m17, key, [0], header=icb)
    gpk, _ = rv_key(("gcm", 256, 17, 5, 0, None))
    k32, iv, aad = rs.bytes(32), rs.bytes(12), rs.bytes(5)
    for call in (lambda: api.encrypt_gcm(m17, k32, iv, aad, gpk), lambda: gpk.witness_gcm(m17, k32, iv, aad), lambda: gpk.encrypt_gcm_batch([m17], [k32], [iv], [aad])):
        with pytest.raises(api.ZkAesError, match="_reveal_"):
            call()
    with pytest.raises(api.ZkAesError, match="at or beyond"):                                       # the prover refuses what the verifier refuses
        pk17.encrypt_reveal_batch([m17], [key], [bytes([0, 0, 0x80])], headers=[icb])
    plain_pk, plain_vk = rv_key(("ecb", 128, 16, 0, 0, None), False)
    assert plain_pk.reveal_info() == {"reveal": False, "message_bytes": 0, "mask_bytes": 0, "offset": 0}
    for call in (lambda: plain_pk.witness_reveal(m16, key, [0]), lambda: plain_pk.encrypt_reveal_batch([m16], [key], [[0]]), lambda: plain_pk.encrypt_reveal_chunked(m16, key, [0])):
        with pytest.raises(api.ZkAesError, match="reveal = 1"):
            call()
    # op_lists takes either; the reveal key's first transform runs over the larger |X| and nothing else in the lists differs
    a, b = plain_pk.op_lists(m16, key), pk.op_lists(m16, key)
    assert (a["h"], a["k"]) == (b["h"], b["k"]) and (a["x"], b["x"]) == (256, 512)
    for what in ("ntt", "msm"):
        assert len(a[what]) == len(b[what])
        differ = [(p, q) for p, q in zip(a[what], b[what]) if p != q]
        print("op-list difference, plain vs reveal ECB-128 16 B,", what, differ)
        assert all(p[1] == q[1] and abs(p[0] - q[0]) <= 256 for p, q in differ), differ           # the same launches; only a count that |X| enters moves, by |X|'s growth at most
    assert [p for p, q in zip(a["ntt"], b["ntt"]) if p != q and p[0] == 256 and q[0] == 512]       # the transform over X itself
    # a plain proof never passes a reveal verifier and a reveal proof never passes a verifier from before, whichever key checks it
    proof = api.encrypt(m16, key, plain_pk)
    ct = ks_ecb(m16, key)
    none = bytes(2)
    _, _, rev, (rproof,) = pk.encrypt_reveal_chunked(m16, key, none, zk_seed=bytes(32))
    assert rev == bytes(16) and api.verify_reveal_chunked(vk, api.CIRCUIT_AES, [rproof], ct, none, rev) == [True]
    for k in (plain_vk, vk):
        try:
            got = api.verify_reveal_chunked(k, api.CIRCUIT_AES, [proof], ct, none, bytes(16))
        except api.ZkAesError:
            got = [False]
        assert got == [False]
        try:
            old = api.verify_encryption(k, rproof, ct)
        except api.ZkAesError:
            old = False
        assert old is False


def test_plain_proof_bytes_do_not_move(api, rv_key, vectors):
    """with reveal keys alive in the process, an AES-128 ECB key over the default SRS literals still emits the committed proof bytes under the reference's fixed prover seed"""
    rv_key(("ecb", 128, 16, 0, 0, None))
    pk, vk = api.synthesize_keys(16, flags=api.KEY_NO_TABLES)
    try:
        assert pk.reveal_info()["reveal"] is False
        proof = api.encrypt(bytes(vectors["plaintext"]), bytes(vectors["key"]), pk, zk_seed=None)  # (None = the reference's fixed prover stream: byte parity)
        gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
        assert proof == open(os.path.join(gold, "gpu_aes16_proof.bin"), "rb").read()
        assert vk.to_bytes() == open(os.path.join(gold, "gpu_aes16_vk.bin"), "rb").read()
    finally:
        pk.free()
