"""Selective disclosure on GCM segments in pure Python, beside tests/gcm_segment_model.py (which it leaves as it is): the size of a segment circuit with
reveal = 1 in closed form, the record-wide mask cut into segment slices, and a segment's public input restated from the statement.

A segment of len bytes (16 c for a head or mid, Lt for a tail) with mb = ceil(len / 8) adds, behind everything DESIGN.md 9g lists for its role: 8 mb mask inputs and
8 len revealed inputs with a booleanity row each, 8 mb - len rows that pin the mask bits at or beyond len to zero, 8 len product rows mask_i * m_ij = r_ij, no witness:

    rows     = the 9g rows     + 16 mb + 15 len
    instance = the 9g instance +  8 mb +  8 len
    witness  = the 9g witness
"""
import gcm_segment_model as base


def segment_bytes(role, units):
    return units if role == "tail" else 16 * units


def reveal_size(length):
    """(rows, instance variables, witnesses) the reveal gates add for a segment of `length` bytes"""
    mb = (length + 7) // 8
    return 16 * mb + 15 * length, 8 * mb + 8 * length, 0


def segment_size(role, units, aad_len, key_bits, ecb_info, reveal=True):
    """(raw_constraints, raw_instance, raw_witness) of a segment circuit: gcm_segment_model.segment_size, plus reveal_size for reveal = True"""
    rows, inst, wits = base.segment_size(role, units, aad_len, key_bits, ecb_info)
    if not reveal:
        return rows, inst, wits
    r, i, w = reveal_size(segment_bytes(role, units))
    return rows + r, inst + i, wits + w


def mask_of(indices, length):
    """ceil(length / 8) bytes, bit i = bit i % 8 of byte i / 8"""
    out = bytearray((length + 7) // 8)
    for i in indices:
        assert 0 <= i < length
        out[i // 8] |= 1 << (i % 8)
    return bytes(out)


def revealed_of(message, mask):
    return bytes(b if (mask[i // 8] >> (i % 8)) & 1 else 0 for i, b in enumerate(message))


def slices(mask, revealed, length, c):
    """[(mask slice, revealed slice)] per segment of a record of `length` bytes cut every c blocks: boundaries are multiples of 16 bytes, so a slice begins on mask byte
    2 c s; the mask slice of a segment of n bytes has ceil(n / 8) bytes"""
    out = []
    for off, size in base.plan(length, c)[1]:
        out.append((mask[off // 8:off // 8 + (size + 7) // 8], revealed[off:off + size]))
    return out


def bits(data):
    return bytes((b >> i) & 1 for b in data for i in range(8))


def public_input(s, n, c, iv, aad, ct, tag, commitments, mask=None, revealed=None):
    """segment s's public input without the leading One, one byte per bit: iv, ctr0 = 2 + s c, then by role what DESIGN.md 9g lists, then -- with a mask -- the
    segment's mask slice and its revealed slice"""
    off, size = base.plan(len(ct), c)[1][s]
    out = bits(iv) + bits((2 + s * c).to_bytes(4, "big"))
    if s == 0:
        out += bits(aad)
    out += bits(ct[off:off + size])
    if s == n - 1:
        out += bits(base.length_block(len(aad), len(ct))) + bits(tag)
    if s > 0:
        out += bits(commitments[s - 1])
    if s < n - 1:
        out += bits(commitments[s])
    if mask is not None:
        m, r = slices(mask, revealed, len(ct), c)[s]
        out += bits(m) + bits(r)
    return out
