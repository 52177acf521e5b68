"""Key tags on GCM segments in pure Python, beside tests/gcm_segment_model.py and tests/gcm_segment_reveal_model.py (which it leaves as they are): what
T key-tag blocks add to a HEAD circuit in closed form, the tag itself from the FIPS-197 model, and a head's public input restated from the statement.

A head with T in 1, 2 tag blocks adds, behind com_out and ahead of the reveal inputs, per block the rounds of the constant block D_t = b"zkaes-keyta" + bytes([t, 0, 0,
0, 0]) under the head's key -- round 0 costs no gate, as for GCM's H block -- and 128 inputs equal to its last state (DESIGN.md 9e's table):

    rows     per block: 148,016 / 177,680 / 207,344 for AES-128 / -192 / -256
    witness  per block: 147,760 / 177,424 / 207,088
    instance per block: 128
"""
import gcm_segment_reveal_model as rv_model
from test_keytag_host import D, model_key_tag

PER_BLOCK = {128: (148_016, 128, 147_760), 192: (177_680, 128, 177_424), 256: (207_344, 128, 207_088)}


def tag_constant(t):
    assert D[t] == b"zkaes-keyta" + bytes([t, 0, 0, 0, 0])
    return D[t]


def key_tag(key, blocks):
    """AES_K(D_0) (|| AES_K(D_1)) from the FIPS-197 model of tests/test_keysize_host.py (DESIGN.md 9e's tag: test_keytag_host.model_key_tag), any key size"""
    return model_key_tag(key, blocks)


def key_tag_size(key_bits, blocks):
    """(rows, instance variables, witnesses) that `blocks` tag blocks add to a head"""
    r, i, w = PER_BLOCK[key_bits]
    return blocks * r, blocks * i, blocks * w


def public_input(s, n, c, iv, aad, ct, tag, commitments, key_tag_bytes=None, mask=None, revealed=None):
    """segment s's public input without the leading One, one byte per bit: gcm_segment_reveal_model.public_input, with the key tag's bits -- LSB first per byte -- in the
    HEAD's row behind com_out and ahead of the mask and revealed slices; the rows of the other segments do not change"""
    plain = rv_model.public_input(s, n, c, iv, aad, ct, tag, commitments)
    out = plain + (rv_model.bits(key_tag_bytes) if s == 0 and key_tag_bytes is not None else b"")
    if mask is not None:
        out += rv_model.public_input(s, n, c, iv, aad, ct, tag, commitments, mask, revealed)[len(plain):]
    return out
