"""Pure-Python SHA-256 (FIPS 180-4) with the state exposed, and the closed-form size of the digest gadget -- the model the digest tests compare against.

A state is 32 bytes: the eight words in big-endian serialisation, so that a finished state is the digest's byte string.
"""
import struct

K = [0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174,
     0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967,
     0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
     0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2]
IV = struct.pack(">8I", 0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19)
M32 = 0xffffffff


def rotr(x, n):
    return ((x >> n) | (x << (32 - n))) & M32


def compress(state, block):
    """one compression: state (32 bytes) over block (64 bytes) -> state"""
    assert len(state) == 32 and len(block) == 64
    w = list(struct.unpack(">16I", block))
    for t in range(16, 64):
        s0 = rotr(w[t - 15], 7) ^ rotr(w[t - 15], 18) ^ (w[t - 15] >> 3)
        s1 = rotr(w[t - 2], 17) ^ rotr(w[t - 2], 19) ^ (w[t - 2] >> 10)
        w.append((s1 + w[t - 7] + s0 + w[t - 16]) & M32)
    st = struct.unpack(">8I", state)
    a, b, c, d, e, f, g, h = st
    for t in range(64):
        t1 = (h + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g & M32)) + K[t] + w[t]) & M32
        t2 = ((rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c))) & M32
        a, b, c, d, e, f, g, h = (t1 + t2) & M32, a, b, c, (d + t1) & M32, e, f, g
    return struct.pack(">8I", *[(x + y) & M32 for x, y in zip(st, (a, b, c, d, e, f, g, h))])


def padding(total_len):
    """what SHA-256 appends to a message of total_len bytes"""
    return b"\x80" + b"\x00" * ((55 - total_len) % 64) + struct.pack(">Q", 8 * total_len)


def chain(data, h_in=None):
    assert len(data) % 64 == 0
    st = IV if h_in is None else bytes(h_in)
    for off in range(0, len(data), 64):
        st = compress(st, data[off:off + 64])
    return st


def finish(h_in, prefix_bytes, tail):
    assert prefix_bytes % 64 == 0
    return chain(bytes(tail) + padding(prefix_bytes + len(tail)), h_in)


def h_out(kind, message, h_in=None, prefix=0):
    """what a proof of a "chain" / "final" key exposes as H_out for this message"""
    return chain(message, h_in) if kind == "chain" else finish(h_in, prefix, message)


def compressions(kind, length):
    return length // 64 if kind == "chain" else (length + 9 + 63) // 64


# ---- the gadget's size.  A row is one R1CS constraint; every gate row allocates one witness, every addition row 32 result bits and its carry bits (each with a
# booleanity row).  Counted from which bits of the block are variables: an xor or select with a constant operand is a re-wiring, and an addition of constants a constant.
ROUND_ROWS = 64 + 32 + 64 + 32 + 32 + (32 + 3 + 1) + (32 + 3 + 1)      # Sigma_1, Ch, Sigma_0, a ^ b, Maj, e', a'  = 296
FEED_FORWARD_ROWS = 8 * (32 + 1 + 1)                                     # 272
SCHEDULE_WORD_ROWS = (32 + 29) + (32 + 22) + (32 + 2 + 1)                # sigma_0, sigma_1, W_t over variables = 150
COMPRESSION_ROWS = 48 * SCHEDULE_WORD_ROWS + 64 * ROUND_ROWS + FEED_FORWARD_ROWS       # 26,416 over a block of variables
HEAD_ROWS = 256 + 256 + 256                                              # booleanity of H_in and H_out, H_out == the last feed-forward


def _pop(x):
    return bin(x).count("1")


def _sigma_rows(v, r1, r2, s):
    """gates of (rotr r1 ^ rotr r2) ^ shr s over a word whose variable bits are the mask v -> (gates, mask of the result's variable bits)"""
    x, y = rotr(v, r1), rotr(v, r2)
    inter = x | y
    return _pop(x & y) + _pop(inter & (v >> s)), inter | (v >> s)


def schedule_rows(var_masks):
    """(rows, addition rows) of one block's message schedule; var_masks = per word W_0 .. W_15 the mask of its bits that are variables (bit i of weight 2^i)"""
    v = list(var_masks)
    rows = adds = 0
    for t in range(16, 64):
        g0, m0 = _sigma_rows(v[t - 15], 7, 18, 3)
        g1, m1 = _sigma_rows(v[t - 2], 17, 19, 10)
        rows += g0 + g1
        if m0 | m1 | v[t - 7] | v[t - 16]:
            rows += 32 + 2 + 1
            adds += 1
            v.append(M32)
        else:
            v.append(0)
    return rows, adds


def digest_size(kind, length):
    """(rows, witnesses) the digest part adds to a circuit whose hidden message has `length` bytes"""
    n = compressions(kind, length)
    rows, adds = HEAD_ROWS, 0
    for j in range(n):
        masks = []
        for t in range(16):
            m = 0
            for i in range(32):
                if 64 * j + 4 * t + 3 - i // 8 < length:
                    m |= 1 << i
            masks.append(m)
        r, a = schedule_rows(masks)
        rows += r + 64 * ROUND_ROWS + FEED_FORWARD_ROWS
        adds += a + 128 + 8
    return rows, rows - HEAD_ROWS - adds
