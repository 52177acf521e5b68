"""GCM segments in pure Python -- the model the segment tests compare against: the GHASH chain cut at segment boundaries with the public length block
last, the boundary commitment, what a segment's trace region holds, and the size of a segment circuit, counted independently of the compiler.

The block cipher and GHASH are test_gcm_host.py's (FIPS-197 and SP 800-38D Algorithm 1 over Python integers), the compression function is sha256_model.py's.
"""
import sha256_model as sha
from test_cbc_host import _encrypt_block, _round_keys
from test_gcm_host import gf_mul

ROLES = ("head", "mid", "tail")


def length_block(aad_len, length):
    return (8 * aad_len).to_bytes(8, "big") + (8 * length).to_bytes(8, "big")


def keystream_ct(msg, key, iv, ctr0):
    """C = M ^ AES_K(iv || ctr0 + b mod 2^32), block by block"""
    rks, out = _round_keys(key), b""
    for b, off in enumerate(range(0, len(msg), 16)):
        stream = _encrypt_block(iv + ((ctr0 + b) & 0xffffffff).to_bytes(4, "big"), rks)
        out += bytes(x ^ s for x, s in zip(msg[off:off + 16], stream))
    return out


def ghash_from(h, y, data):
    """the accumulator after absorbing data (zero-padded to whole blocks) from y -> every Y on the way"""
    ys = []
    data = data + bytes(-len(data) % 16)
    for off in range(0, len(data), 16):
        y = gf_mul(y ^ int.from_bytes(data[off:off + 16], "big"), h)
        ys.append(y)
    return ys


def plan(length, c):
    nb = (length + 15) // 16
    n = (nb + c - 1) // c
    return n, [(16 * c * s, min(16 * c, length - 16 * c * s)) for s in range(n)]


def segmented_gcm(msg, key, iv, aad, c):
    """the record as n segments of c blocks: (ciphertext, tag, [Y_0 .. Y_{n-2}]).  Each segment computes only what its proof states: its own keystream from ctr0 = 2 +
    s c, the chain from the Y it is handed, and -- the last one -- the multiplication over the length block and the tag"""
    rks = _round_keys(key)
    h = int.from_bytes(_encrypt_block(bytes(16), rks), "big")
    n, cuts = plan(len(msg), c)
    ct, ys, y = b"", [], 0
    for s, (off, size) in enumerate(cuts):
        seg_ct = keystream_ct(msg[off:off + size], key, iv, 2 + s * c)
        ct += seg_ct
        if s == 0 and aad:
            y = ghash_from(h, y, aad)[-1]
        y = ghash_from(h, y, seg_ct)[-1]
        if s + 1 < n:
            ys.append(y)
    s_final = ghash_from(h, y, length_block(len(aad), len(msg)))[-1]
    mask = int.from_bytes(_encrypt_block(iv + (1).to_bytes(4, "big"), rks), "big")
    return ct, (s_final ^ mask).to_bytes(16, "big"), [v.to_bytes(16, "big") for v in ys]


def commitment(key, y, salt):
    """ONE compression from the initial value over the one 64-byte block key || zeros to 32 bytes || y || salt: no padding block"""
    assert len(key) in (16, 24, 32) and len(y) == 16 and len(salt) == 16
    return sha.compress(sha.IV, bytes(key) + bytes(32 - len(key)) + bytes(y) + bytes(salt))


def segment_trace(role, msg, key, iv, ctr0, y_in=None, aad=b"", lenblk=None):
    """what the trace of one segment holds beside the AES slots: ciphertext, per data block the counter's low word and the carries of (counter - 1) + 1, every X and Y of
    the chain (integers), and a tail's tag"""
    rks = _round_keys(key)
    h = int.from_bytes(_encrypt_block(bytes(16), rks), "big")
    ct = keystream_ct(msg, key, iv, ctr0)
    nb = (len(msg) + 15) // 16
    counters, carries = [], []
    for b in range(nb):
        ctr = (ctr0 + b) & 0xffffffff
        prev, carry = (ctr - 1) & 0xffffffff, 0
        if b:
            i = 0
            while i < 31 and (prev >> i) & 1:
                carry |= 1 << i
                i += 1
        counters.append(ctr.to_bytes(4, "big"))
        carries.append(carry.to_bytes(4, "big"))
    pad = lambda d: d + bytes(-len(d) % 16)
    data = (pad(aad) if role == "head" else b"") + pad(ct) + (lenblk if role == "tail" else b"")
    y = 0 if role == "head" else int.from_bytes(y_in, "big")
    xs, ys = [], []
    for off in range(0, len(data), 16):
        x = y ^ int.from_bytes(data[off:off + 16], "big")
        y = gf_mul(x, h)
        xs.append(x)
        ys.append(y)
    out = {"h": h, "ct": ct, "counters": counters, "carries": carries, "xs": xs, "ys": ys}
    if role == "tail":
        mask = int.from_bytes(_encrypt_block(iv + (1).to_bytes(4, "big"), rks), "big")
        out["tag"] = (ys[-1] ^ mask).to_bytes(16, "big")
    return out


# ---- the size of a segment circuit.  A row is one R1CS constraint.  The compression is counted bit by bit with the compiler's folding rules restated: an xor gate costs
# a row and a witness only between two variables; a select with a constant condition is a re-wiring, with a variable condition over two constants it is a constant
# (equal) or the condition or its negation (unequal), otherwise one gate; an addition of constants is a constant, any other 32 result bits + its carry bits (a booleanity
# row each) + one row.  A bit is 0, 1 or V.
V = "v"


class _Count:
    def __init__(self):
        self.rows = self.wits = 0

    def gate(self):
        self.rows += 1
        self.wits += 1
        return V

    def xor(self, a, b):
        if a == V and b == V:
            return self.gate()
        return V if V in (a, b) else a ^ b

    def select(self, c, t, f):
        if c != V:
            return t if c else f
        if t != V and f != V:
            return t if t == f else V
        return self.gate()

    def xor_w(self, x, y):
        return [self.xor(a, b) for a, b in zip(x, y)]

    def add(self, ops, konst, carry_bits):
        if all(b != V for w in ops for b in w):
            return word((konst + sum(sum(b << i for i, b in enumerate(w)) for w in ops)) & sha.M32)
        self.rows += 32 + carry_bits + 1
        self.wits += 32 + carry_bits
        return [V] * 32


def word(v):
    return [(v >> i) & 1 for i in range(32)]


def _rotr(w, n):
    return [w[(i + n) % 32] for i in range(32)]


def _shr(w, n):
    return [w[i + n] if i + n < 32 else 0 for i in range(32)]


def compression_size(block_words, state_words):
    """(rows, witnesses) of one compression over words that are lists of 32 bits, each 0, 1 or V"""
    k = _Count()
    w = list(block_words)
    for t in range(16, 64):
        x, y = w[t - 15], w[t - 2]
        s0 = k.xor_w(k.xor_w(_rotr(x, 7), _rotr(x, 18)), _shr(x, 3))
        s1 = k.xor_w(k.xor_w(_rotr(y, 17), _rotr(y, 19)), _shr(y, 10))
        w.append(k.add([s1, w[t - 7], s0, w[t - 16]], 0, 2))
    a, b, c, d, e, f, g, h = state_words
    for t in range(64):
        s1 = k.xor_w(k.xor_w(_rotr(e, 6), _rotr(e, 11)), _rotr(e, 25))
        ch = [k.select(ci, ti, fi) for ci, ti, fi in zip(e, f, g)]
        s0 = k.xor_w(k.xor_w(_rotr(a, 2), _rotr(a, 13)), _rotr(a, 22))
        ab = k.xor_w(a, b)
        maj = [k.select(ci, ti, fi) for ci, ti, fi in zip(ab, c, a)]
        e2 = k.add([d, h, s1, ch, w[t]], sha.K[t], 3)
        a2 = k.add([h, s1, ch, w[t], s0, maj], sha.K[t], 3)
        a, b, c, d, e, f, g, h = a2, a, b, c, e2, e, f, g
    for st, out in zip(state_words, (a, b, c, d, e, f, g, h)):
        k.add([st, out], 0, 1)
    return k.rows, k.wits


def commitment_size(key_bits):
    """(rows, witnesses) of one boundary commitment: 256 inputs with their booleanity rows, the compression from the CONSTANT initial value over key || zeros || Y ||
    salt (the zero words of a short key are constants), 256 equalities"""
    import struct
    kw = key_bits // 32
    block = [[V] * 32 if t < kw or t >= 8 else word(0) for t in range(16)]
    rows, wits = compression_size(block, [word(v) for v in struct.unpack(">8I", sha.IV)])
    return 256 + rows + 256, wits


def segment_size(role, units, aad_len, key_bits, ecb_info):
    """closed forms for (raw_constraints, raw_instance, raw_witness) of a segment circuit, relative to ECB over the same number of AES slots -- ecb_info(blocks) ->
    (raw_constraints, raw_witness) of the ECB circuit for that many blocks at key_bits -- in the way test_gcm_host.py states the lone circuit:

        slots = nb + 1 (+ 1 for a tail: J_0); a head or mid has len = 16 c bytes, a tail len = Lt; M = na + nb (head), nb (mid), nb + 1 (tail)
        GHASH  G = 1152 M + 16384 (M - 1) + 1024 f + 8 (A + len - f)        head, f = the bytes of its first block (min(A, 16) with aad, else 16)
               G = (1152 + 16384) M + 8 len (+ 128 for a tail)              mid, tail: every X is Y ^ block, so all 128 bits of every X are variables; a tail's
                                                                             length block is 128 INPUT bits, one chain xor each
        rows   = E - 512 slots + 32 len + 128 + 8 A + 128 nb + 96 [tail] + 61 (nb - 1) + 381 + G + (128 + 384) [tail] + 256 [not head] + 128 [not tail] + commitments
        wits   = W - 256 slots + 16 len + 128 nb + 96 [tail] + 61 (nb - 1) + 381 + (G - 128 M) + 128 [tail] + 256 [not head] + 128 [not tail] + commitments
        inst   = 1 + 128 + 8 A + 8 len + 256 [tail] + 256 commitments

    (32 len: message witness, xor gate, input and equality per bit; 128: the iv and ctr0 inputs; 128 per data block: its round-0 xor with the key -- all 128 bits of
    iv || counter are variables, where the lone circuit's counters are constants; 96: the J_0 block's; 61: the incrementer, 31 xor and 30 and gates; 381: the V table;
    128 + 384: the length-block inputs, the tag's xor gates, inputs and equalities; 256: the Y_in and salt_in witnesses; 128: salt_out.)"""
    head, tail = role == "head", role == "tail"
    length = units if tail else 16 * units
    nb, na = (length + 15) // 16, (aad_len + 15) // 16
    slots = nb + 1 + (1 if tail else 0)
    m = na + nb if head else nb + 1 if tail else nb
    if head:
        f = min(aad_len, 16) if aad_len else 16
        g = 1152 * m + 16384 * (m - 1) + 1024 * f + 8 * (aad_len + length - f)
    else:
        g = (1152 + 16384) * m + 8 * length + (128 if tail else 0)
    ncom = 2 if role == "mid" else 1
    crow, cwit = commitment_size(key_bits)
    e_rows, e_wits = ecb_info(slots)
    common = 128 * nb + (96 if tail else 0) + 61 * (nb - 1) + 381 + (0 if head else 256) + (0 if tail else 128)
    rows = e_rows - 512 * slots + 32 * length + 128 + 8 * aad_len + common + g + (128 + 384 if tail else 0) + ncom * crow
    wits = e_wits - 256 * slots + 16 * length + common + (g - 128 * m) + (128 if tail else 0) + ncom * cwit
    inst = 1 + 128 + 8 * aad_len + 8 * length + (256 if tail else 0) + 256 * ncom
    return rows, inst, wits
