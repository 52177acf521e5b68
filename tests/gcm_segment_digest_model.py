"""Digests on segmented GCM records in pure Python, beside tests/gcm_segment_model.py and tests/sha256_model.py (which it leaves as they are): the plan
of a digest record, its states and boundary accumulators, the size of every role's circuit restated from 9f's and 9g's closed forms, and the public input of every proof.

A digest record of L > 16 c bytes, c a multiple of 4, is nd = ceil(L / (16 c)) data segments -- head, mids, and the LAST with Lr = L - 16 c (nd - 1) bytes -- and one
closing tail without data: nd + 1 proofs, nd commitments, nd + 1 states.

    head, mid   9g's circuit, then 9f's chain digest over its 16 c bytes: 512 inputs H_in, H_out
    last        9g's mid with the byte length Lr (the ragged path is the tail's), then 9f's FINAL digest over its Lr bytes whose eight length bytes are INPUTS: 64 more
                inputs with their booleanity rows, and the schedule of the last block sees W_14, W_15 as variables
    tail        no data block: the H and J_0 slots, ONE multiplication over X = Y_in ^ the 128 length-block inputs, the tag, com_in
"""
import hashlib

import gcm_segment_model as seg
import sha256_model as sha


def plan(length, c):
    """(nd, Lr)"""
    assert c % 4 == 0 and length > 16 * c
    nd = -(-length // (16 * c))
    return nd, length - 16 * c * (nd - 1)


def states(msg, c, h_in=None, prefix=0):
    """the nd + 1 states: plain SHA-256, cut at the segment boundaries; the last is a real digest"""
    nd, _ = plan(len(msg), c)
    st = [sha.IV if h_in is None else h_in]
    for s in range(nd - 1):
        st.append(sha.chain(msg[16 * c * s:16 * c * (s + 1)], st[-1]))
    st.append(sha.finish(st[-1], prefix + 16 * c * (nd - 1), msg[16 * c * (nd - 1):]))
    return st


def boundaries(msg, key, iv, aad, c):
    """the nd accumulators behind the data segments: segmented_gcm's n - 1 and, last, the one behind the record's last data block, ahead of the length block"""
    from test_cbc_host import _encrypt_block, _round_keys
    ct, tag, ys = seg.segmented_gcm(msg, key, iv, aad, c)[:3]
    h = int.from_bytes(_encrypt_block(bytes(16), _round_keys(key)), "big")
    nd, lr = plan(len(msg), c)
    y = seg.ghash_from(h, int.from_bytes(ys[nd - 2], "big"), ct[16 * c * (nd - 1):])[-1]
    return ct, tag, list(ys[:nd - 1]) + [y.to_bytes(16, "big")]


def final_digest_size(length):
    """(rows, witnesses) of a last's digest part: sha256_model.digest_size("final", length) with the eight length bytes as inputs -- 64 more booleanity rows, no witness,
    and the last block's final two words are variables"""
    n = sha.compressions("final", length)
    rows, adds = sha.HEAD_ROWS + 64, 0
    for j in range(n):
        masks = []
        for t in range(16):
            m = 0
            for i in range(32):
                q = 64 * j + 4 * t + 3 - i // 8
                if q < length or q >= 64 * n - 8:
                    m |= 1 << i
            masks.append(m)
        r, a = sha.schedule_rows(masks)
        rows += r + 64 * sha.ROUND_ROWS + sha.FEED_FORWARD_ROWS
        adds += a + 128 + 8
    return rows, rows - sha.HEAD_ROWS - 64 - adds


def segment_size(role, units, aad_len, key_bits, ecb_info):
    """(raw_constraints, raw_instance, raw_witness) of a digest record's segment circuit: head and mid from gcm_segment_model.segment_size plus the chain digest; the last
    and the closing tail from 9g's closed form restated for their shapes (ecb_info as there)"""
    if role in ("head", "mid"):
        rows, inst, wits = seg.segment_size(role, units, aad_len, key_bits, ecb_info)
        dr, dw = sha.digest_size("chain", 16 * units)
        return rows + dr, inst + 512, wits + dw
    crow, cwit = seg.commitment_size(key_bits)
    if role == "last":
        length, nb = units, (units + 15) // 16
        slots, m = nb + 1, nb
        g = (1152 + 16384) * m + 8 * length
        common = 128 * nb + 61 * (nb - 1) + 381 + 256 + 128
        e_rows, e_wits = ecb_info(slots)
        dr, dw = final_digest_size(length)
        return (e_rows - 512 * slots + 32 * length + 128 + common + g + 2 * crow + dr, 1 + 128 + 8 * length + 512 + 512 + 64, e_wits - 256 * slots + 16 * length + common + (g - 128 * m) + 2 * cwit + dw)
    assert role == "tail" and units == 0 and aad_len == 0
    g = 1152 + 16384 + 128                                                                            # one multiplication; the 128 chain xors over the length-block inputs
    common = 96 + 381 + 256                                                                           # J_0's round 0, the V table, Y_in and salt_in
    e_rows, e_wits = ecb_info(2)
    return e_rows - 512 * 2 + 128 + common + g + (128 + 384) + crow, 1 + 128 + 256 + 256, e_wits - 256 * 2 + common + (g - 128) + 128 + cwit


def bits(data):
    return bytes((b >> k) & 1 for b in data for k in range(8))


def public_input(s, length, c, iv, aad, ct, tag, commitments, st, prefix=0):
    """proof s's public input without the leading One, one byte per bit, LSB first per byte"""
    nd, lr = plan(length, c)
    hd = iv + (2 + s * c).to_bytes(4, "big")
    if s == nd:
        return bits(hd + seg.length_block(len(aad), length) + tag + commitments[nd - 1])
    out = hd + (aad if s == 0 else b"") + ct[16 * c * s:16 * c * s + (lr if s == nd - 1 else 16 * c)] + (commitments[s - 1] if s else b"") + commitments[s] + st[s] + st[s + 1]
    if s == nd - 1:
        out += (8 * (prefix + length)).to_bytes(8, "big")
    return bits(out)


def digest(msg, prefix_bytes=b""):
    return hashlib.sha256(prefix_bytes + msg).digest()
