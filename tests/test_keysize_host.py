"""AES-192 and AES-256 on the host: the published vectors through an independent model and through the library's host ciphers, the circuits' counts against closed
forms, AES-128 unchanged through the key-size entry points, and the trace kernels' source for NK = 6 and 8 run lane by lane under sanitizers (no GPU, no oracle).

The model is a pure-Python AES with the key length in words, Nk, as a parameter: FIPS-197 5.2's key expansion written from the standard (it shares the S-box and the
field multiplication of test_cbc_host.py, which are key-size independent, and nothing else).  It is checked against FIPS-197 appendix C, SP 800-38A F.1 / F.2 / F.5 and
the McGrew-Viega GCM test cases before anything is compared with it.

The closed forms come from Builder's per-gate costs, which do not depend on the data: an allocated bit is one row (and one variable), an xor of two
non-constant bits one row and one witness, an xor with a constant nothing, an equality one row, an S-box s = 884 rows and witnesses, xtime x = 3 (bits 1, 3, 4 of
2 a ^ 0x1b a_7; bit 0 is a_7 itself).  With Nr = Nk + 6, I = 10, 8, 13 SubWord instances for Nk = 4, 6, 8:

    KS(Nk) = 32 Nk + 32 (4 (Nr + 1) - Nk) + 4 s I            the key bits, four xor bytes per derived word, four S-boxes per instance
    C(Nr)  = 16 s Nr + (16 x + 512) (Nr - 1) + 128 Nr        a block from its round 1 on: SubBytes, xtime and the four chain xors per byte of MixColumns, AddRoundKey
           = 14832 Nr - 560

    mode   raw_constraints                                                       raw_witness                                    raw_instance
    ECB    KS + nb (C + 512)                                                     KS + nb (C + 256)                              1 + 128 nb
    CBC    KS + 128 + nb (C + 640)                                               KS + nb (C + 384)                              129 + 128 nb
    CTR    KS + 128 + nb (C + 128) + 253 (nb - 1) + 32 L                         KS + nb (C + 128) + 253 (nb - 1) + 16 L        129 + 8 L
    GCM    KS + (nb + 2) C + 96 (nb + 1) + 32 L + 8 A + 861 + G                  KS + (nb + 2) C + 96 (nb + 1) + 16 L + 509     225 + 8 (A + L)
                                                                                    + G - 128 M
           G = 1152 M + 16384 (M - 1) + 1024 f + 8 (A + L - f),  M = na + nb + 1,  f = min(A, 16) if A else min(L, 16)           (test_gcm_host.py)

(512 = message witnesses, round-0 xor, ciphertext inputs, equalities, 128 each; CBC adds the X_b xor per block and the IV inputs; CTR's 253 is one increment; GCM's
861 = 96 iv inputs + 381 V-table xors + 384 for the tag.)

The non-zero counts of A, B and C are NOT a function of the gate counts: a row's width depends on the polarity of its literals (and / nor / and-not, the three forms
of an equality), and the polarities follow the Rcon constants through the schedule and from there into every block.  For ECB they are still exactly affine in nb,
nnz = ks(Nk) + nb blk(Nk), with the constants of ECB_NNZ below -- recorded from the compiler, not derived; for the chained modes a block's polarities depend on the
block before it, so the tests pin the figures of the listed shapes (NNZ_PINS) and, for AES-128, require the matrices themselves to equal the old entry points'.
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from test_cbc_host import CSRC, ROOT, SBOX, _gmul, model_cbc, model_ecb
from test_ctr_host import NIST_CTR_CT, NIST_ICB, model_ctr
from test_cbc_host import NIST_CT as NIST_CBC128_CT, NIST_IV, NIST_KEY as NIST_KEY128, NIST_PT
from test_gcm_host import TC3_IV, TC3_KEY, TC3_PT, TC4_AAD, gf_mul, ghash_blocks, model_gcm

KEY_BITS = (128, 192, 256)
INSTANCES = {4: 10, 6: 8, 8: 13}


# ---- the model
def expand_key(key):
    """FIPS-197 5.2 -> Nr + 1 round keys of 16 bytes; len(key) = 4 Nk"""
    nk = len(key) // 4
    assert len(key) in (16, 24, 32)
    nr = nk + 6
    w = [list(key[4 * i:4 * i + 4]) for i in range(nk)]
    rcon = 1
    for i in range(nk, 4 * (nr + 1)):
        t = list(w[i - 1])
        if i % nk == 0:
            t = [SBOX[t[1]] ^ rcon, SBOX[t[2]], SBOX[t[3]], SBOX[t[0]]]
            rcon = _gmul(rcon, 2)
        elif nk > 6 and i % nk == 4:
            t = [SBOX[v] for v in t]
        w.append([a ^ b for a, b in zip(w[i - nk], t)])
    return w, [sum(w[4 * r:4 * r + 4], []) for r in range(nr + 1)]


def encrypt_block(block, rks):
    nr = len(rks) - 1
    s = [a ^ b for a, b in zip(block, rks[0])]
    for r in range(1, nr + 1):
        s = [SBOX[v] for v in s]
        s = [s[4 * ((c + row) % 4) + row] for c in range(4) for row in range(4)]
        if r < nr:
            s = sum(([_gmul(col[k], 2) ^ _gmul(col[(k + 1) % 4], 3) ^ col[(k + 2) % 4] ^ col[(k + 3) % 4] for k in range(4)]
                     for col in (s[4 * c:4 * c + 4] for c in range(4))), [])
        s = [a ^ b for a, b in zip(s, rks[r])]
    return bytes(s)


def ks_ecb(msg, key):
    rks = expand_key(key)[1]
    return b"".join(encrypt_block(msg[o:o + 16], rks) for o in range(0, len(msg), 16))


def ks_cbc(msg, key, iv):
    rks, prev, out = expand_key(key)[1], bytes(iv), b""
    for off in range(0, len(msg), 16):
        prev = encrypt_block(bytes(a ^ b for a, b in zip(msg[off:off + 16], prev)), rks)
        out += prev
    return out


def ks_ctr(msg, key, icb):
    rks, n, out = expand_key(key)[1], int.from_bytes(icb, "big"), b""
    for b, off in enumerate(range(0, len(msg), 16)):
        stream = encrypt_block(((n + b) % (1 << 128)).to_bytes(16, "big"), rks)
        out += bytes(x ^ s for x, s in zip(msg[off:off + 16], stream))
    return out


def ks_gcm(msg, key, iv, aad=b""):
    """SP 800-38D 7.1 for a 96-bit IV over the GHASH of test_gcm_host.py -> (ciphertext, tag)"""
    rks = expand_key(key)[1]
    h = int.from_bytes(encrypt_block(bytes(16), rks), "big")
    ct = b""
    for b, off in enumerate(range(0, len(msg), 16)):
        stream = encrypt_block(iv + (b + 2).to_bytes(4, "big"), rks)
        ct += bytes(x ^ s for x, s in zip(msg[off:off + 16], stream))
    y = 0
    for blk in ghash_blocks(aad, ct):
        y = gf_mul(y ^ blk, h)
    mask = int.from_bytes(encrypt_block(iv + (1).to_bytes(4, "big"), rks), "big")
    return ct, (y ^ mask).to_bytes(16, "big")


# ---- published vectors
FIPS_PT = bytes.fromhex("00112233445566778899aabbccddeeff")
FIPS = {24: "dda97ca4864cdfe06eaf70a0ec0d7191", 32: "8ea2b7ca516745bfeafc49904b496089", 16: "69c4e0d86a7b0430d8cdb78070b4c55a"}
K256 = bytes.fromhex("603deb1015ca71be2b73aef0857d77811f352c073b6108d72d9810a30914dff4")
K192 = bytes.fromhex("8e73b0f7da0e6452c810f32b809079e562f8ead2522c6b7b")
SP800_38A = {      # (mode, key) -> the four ciphertext blocks of SP 800-38A F.1.3 / F.1.5, F.2.3 / F.2.5, F.5.3 / F.5.5
    ("ecb", 32): "f3eed1bdb5d2a03c064b5a7e3db181f8" "591ccb10d410ed26dc5ba74a31362870" "b6ed21b99ca6f4f9f153e7b1beafed1d" "23304b7a39f9f3ff067d8d8f9e24ecc7",
    ("cbc", 32): "f58c4c04d6e5f1ba779eabfb5f7bfbd6" "9cfc4e967edb808d679f777bc6702c7d" "39f23369a9d9bacfa530e26304231461" "b2eb05e2c39be9fcda6c19078c6a9d1b",
    ("ctr", 32): "601ec313775789a5b7a7f504bbf3d228" "f443e3ca4d62b59aca84e990cacaf5c5" "2b0930daa23de94ce87017ba2d84988d" "dfc9c58db67aada613c2dd08457941a6",
    ("ecb", 24): "bd334f1d6e45f25ff712a214571fa5cc" "974104846d0ad3ad7734ecb3ecee4eef" "ef7afd2270e2e60adce0ba2face6444e" "9a4b41ba738d6c72fb16691603c18e0e",
    ("cbc", 24): "4f021db243bc633d7178183a9fa071e8" "b4d9ada9ad7dedf4e5e738763f69145a" "571b242012fb7ae07fa9baac3df102e0" "08b0e27988598881d920a9e64f5615cd",
    ("ctr", 24): "1abc932417521ca24f2b0459fe7e6e0b" "090339ec0aa6faefd5ccc2c6f4ce8e94" "1e36b26bd1ebc670d1bd1d665620abf7" "4f78a7f6d29809585a97daec58c6b050",
}
GCM_VECTORS = {    # McGrew-Viega appendix B: name -> (key, iv, plaintext, aad, ciphertext or None, tag)
    "tc13": (bytes(32), bytes(12), b"", b"", b"", "530f8afbc74536b9a963b4f1c4cb738b"),
    "tc14": (bytes(32), bytes(12), bytes(16), b"", bytes.fromhex("cea7403d4d606b6e074ec5d3baf39d18"), "d0d1c8a799996bf0265b98b5d48ab919"),
    "tc16": (TC3_KEY * 2, TC3_IV, TC3_PT[:60], TC4_AAD, None, "76fc6ece0f4e1768cddf8853bb2d551b"),
    "tc8": (bytes(24), bytes(12), bytes(16), b"", bytes.fromhex("98e7247c07f0fe411c267e4384b0f600"), "2ff58d80033927ab8ef4d4587514f0fb"),
    "tc10": ((TC3_KEY * 2)[:24], TC3_IV, TC3_PT[:60], TC4_AAD, None, "2519498e80f1478f37ba55bd6d27618c"),
}


@pytest.mark.parametrize("klen", [16, 24, 32])
def test_fips197_appendix_c(api, klen):
    key, want = bytes(range(klen)), bytes.fromhex(FIPS[klen])
    assert ks_ecb(FIPS_PT, key) == want
    assert api.ecb_ciphertext(FIPS_PT, key) == want
    if klen == 16:
        assert model_ecb(FIPS_PT, key) == want                                  # the Nk = 4 instance of the model is the older model


@pytest.mark.parametrize("case", sorted(SP800_38A))
def test_sp800_38a_all_four_blocks(api, case):
    mode, klen = case
    key, want = (K256 if klen == 32 else K192), bytes.fromhex(SP800_38A[case])
    assert len(key) == klen and len(want) == 64
    if mode == "ecb":
        assert ks_ecb(NIST_PT, key) == want and api.ecb_ciphertext(NIST_PT, key) == want
    elif mode == "cbc":
        assert ks_cbc(NIST_PT, key, NIST_IV) == want and api.cbc_ciphertext(NIST_PT, key, NIST_IV) == want
    else:
        assert ks_ctr(NIST_PT, key, NIST_ICB) == want and api.ctr_crypt(NIST_PT, key, NIST_ICB) == want
        assert api.ctr_crypt(want, key, NIST_ICB) == NIST_PT
        assert api.ctr_crypt(NIST_PT[:17], key, NIST_ICB) == want[:17]


def test_aes128_behaviour_of_the_host_ciphers_is_unchanged(api):
    assert api.cbc_ciphertext(NIST_PT, NIST_KEY128, NIST_IV) == NIST_CBC128_CT == ks_cbc(NIST_PT, NIST_KEY128, NIST_IV) == model_cbc(NIST_PT, NIST_KEY128, NIST_IV)
    assert api.ctr_crypt(NIST_PT, NIST_KEY128, NIST_ICB) == NIST_CTR_CT == ks_ctr(NIST_PT, NIST_KEY128, NIST_ICB) == model_ctr(NIST_PT, NIST_KEY128, NIST_ICB)
    assert api.gcm_encrypt(TC3_PT[:60], TC3_KEY, TC3_IV, TC4_AAD) == ks_gcm(TC3_PT[:60], TC3_KEY, TC3_IV, TC4_AAD) == model_gcm(TC3_PT[:60], TC3_KEY, TC3_IV, TC4_AAD)
    # the old C entry points and the new ones with key_len = 16 give the same bytes
    out_a, out_b = C.create_string_buffer(64), C.create_string_buffer(64)
    assert api.lib().zkaes_cbc_ciphertext(NIST_PT, C.c_size_t(64), NIST_KEY128, NIST_IV, out_a) == 0
    assert api.lib().zkaes_cbc_ciphertext_ks(NIST_PT, C.c_size_t(64), NIST_KEY128, C.c_size_t(16), NIST_IV, out_b) == 0
    assert out_a.raw == out_b.raw == NIST_CBC128_CT


@pytest.mark.parametrize("name", sorted(GCM_VECTORS))
def test_gcm_vectors_through_model_and_library(api, name):
    key, iv, pt, aad, ct, tag = GCM_VECTORS[name]
    tag = bytes.fromhex(tag)
    got = ks_gcm(pt, key, iv, aad)
    assert got[1] == tag and (ct is None or got[0] == ct)
    assert api.gcm_encrypt(pt, key, iv, aad) == got
    assert api.gcm_decrypt(got[0], key, iv, aad, tag) == pt
    flipped = bytes([tag[0] ^ 0x01]) + tag[1:]
    assert api.gcm_decrypt(got[0], key, iv, aad, flipped) is None
    if pt:
        assert api.gcm_decrypt(bytes([got[0][0] ^ 0x80]) + got[0][1:], key, iv, aad, tag) is None


@pytest.mark.parametrize("klen", [24, 32])
def test_host_ciphers_match_the_model_on_ragged_lengths(api, klen):
    rs = np.random.RandomState(0x5A00 + klen)
    for length, alen in ((1, 0), (17, 5), (33, 16), (48, 20)):
        msg, key, iv, icb, aad = rs.bytes(length), rs.bytes(klen), rs.bytes(12), rs.bytes(16), rs.bytes(alen)
        assert api.ctr_crypt(msg, key, icb) == ks_ctr(msg, key, icb)
        assert api.ctr_crypt(msg, key, b"\xff" * 16) == ks_ctr(msg, key, b"\xff" * 16)          # the counter wraps at the first increment
        ct, tag = api.gcm_encrypt(msg, key, iv, aad)
        assert (ct, tag) == ks_gcm(msg, key, iv, aad)
        assert api.gcm_decrypt(ct, key, iv, aad, tag) == msg
        whole = msg + bytes(-length % 16)
        assert api.ecb_ciphertext(whole, key) == ks_ecb(whole, key)
        assert api.cbc_ciphertext(whole, key, icb) == ks_cbc(whole, key, icb)


@pytest.mark.parametrize("klen", [0, 15, 20, 33])
def test_wrong_key_lengths_raise(api, klen):
    key = bytes(klen)
    for call in (lambda: api.ecb_ciphertext(bytes(16), key), lambda: api.cbc_ciphertext(bytes(16), key, bytes(16)), lambda: api.ctr_crypt(b"x", key, bytes(16)),
                 lambda: api.gcm_encrypt(b"x", key, bytes(12)), lambda: api.gcm_decrypt(b"x", key, bytes(12), b"", bytes(16))):
        with pytest.raises(api.ZkAesError):
            call()
    # and at the C boundary itself, which the Python checks above never reach
    out, tag, ok = C.create_string_buffer(16), C.create_string_buffer(16), C.c_int()
    L = api.lib()
    buf = bytes(max(klen, 1))
    assert L.zkaes_ecb_ciphertext_ks(bytes(16), C.c_size_t(16), buf, C.c_size_t(klen), out) != 0
    assert L.zkaes_cbc_ciphertext_ks(bytes(16), C.c_size_t(16), buf, C.c_size_t(klen), bytes(16), out) != 0
    assert L.zkaes_ctr_crypt_ks(bytes(16), C.c_size_t(16), buf, C.c_size_t(klen), bytes(16), out) != 0
    assert L.zkaes_gcm_encrypt_ks(bytes(16), C.c_size_t(16), buf, C.c_size_t(klen), bytes(12), None, C.c_size_t(0), out, tag) != 0
    assert L.zkaes_gcm_decrypt_ks(bytes(16), C.c_size_t(16), buf, C.c_size_t(klen), bytes(12), None, C.c_size_t(0), bytes(16), out, C.byref(ok)) != 0
    assert b"16, 24 or 32" in L.zkaes_last_error()


def test_ecb_ciphertext_takes_whole_blocks_only(api):
    for n in (0, 15, 17):
        with pytest.raises(api.ZkAesError):
            api.ecb_ciphertext(bytes(n), bytes(32))


# ---- circuits
S_BOX, XTIME = 884, 3


def ks_rows(nk):
    nr = nk + 6
    return 32 * nk + 32 * (4 * (nr + 1) - nk) + 4 * S_BOX * INSTANCES[nk]


def core_rows(nk):
    nr = nk + 6
    return 16 * S_BOX * nr + (16 * XTIME + 512) * (nr - 1) + 128 * nr


def closed_form(api, kind, nk, length, alen=0):
    """(raw_constraints, raw_witness, raw_instance) from the module docstring's table"""
    ks, c, nb, na = ks_rows(nk), core_rows(nk), (length + 15) // 16, (alen + 15) // 16
    if kind == api.CIRCUIT_AES:
        return ks + nb * (c + 512), ks + nb * (c + 256), 1 + 128 * nb
    if kind == api.CIRCUIT_AES_CBC:
        return ks + 128 + nb * (c + 640), ks + nb * (c + 384), 129 + 128 * nb
    if kind == api.CIRCUIT_AES_CTR:
        return ks + 128 + nb * (c + 128) + 253 * (nb - 1) + 32 * length, ks + nb * (c + 128) + 253 * (nb - 1) + 16 * length, 129 + 8 * length
    m, f = na + nb + 1, (min(alen, 16) if alen else min(length, 16))
    g = 1152 * m + 16384 * (m - 1) + 1024 * f + 8 * (alen + length - f)
    return (ks + (nb + 2) * c + 96 * (nb + 1) + 32 * length + 8 * alen + 861 + g, ks + (nb + 2) * c + 96 * (nb + 1) + 16 * length + 509 + g - 128 * m,
            225 + 8 * (alen + length))


def shapes(api):
    return [(api.CIRCUIT_AES, 16, 0), (api.CIRCUIT_AES, 32, 0), (api.CIRCUIT_AES_CBC, 32, 0), (api.CIRCUIT_AES_CTR, 17, 0), (api.CIRCUIT_AES_GCM, 17, 5)]


def old_info(api, kind, length, alen):
    out = (C.c_uint64 * 12)()
    if kind == api.CIRCUIT_AES_GCM:
        assert api.lib().zkaes_circuit_info_gcm(C.c_size_t(length), C.c_size_t(alen), out) == 0
    else:
        assert api.lib().zkaes_circuit_info(int(kind), C.c_size_t(length), out) == 0
    return list(out)


def old_matrix(api, kind, length, alen, which):
    L = api.lib()
    rows, nnz = C.c_uint64(), C.c_uint64()
    call = (lambda *a: L.zkaes_circuit_matrix_gcm(C.c_size_t(length), C.c_size_t(alen), which, *a)) if kind == api.CIRCUIT_AES_GCM else \
           (lambda *a: L.zkaes_circuit_matrix(int(kind), C.c_size_t(length), which, *a))
    assert call(C.byref(rows), C.byref(nnz), None, None, None) == 0
    rowptr, col, coeff = np.zeros(rows.value + 1, dtype=np.uint32), np.zeros(nnz.value, dtype=np.uint32), np.zeros(nnz.value, dtype=np.int64)
    assert call(None, None, rowptr.ctypes.data_as(C.c_void_p), col.ctypes.data_as(C.c_void_p), coeff.ctypes.data_as(C.c_void_p)) == 0
    return rowptr, col, coeff


@pytest.mark.parametrize("shape", range(5))
def test_key_bits_128_is_the_old_circuit(api, shape):
    """the info and all three matrices of the key-size entry points at 128 bits equal those of the entry points that predate them, element for element"""
    kind, length, alen = shapes(api)[shape]
    out = (C.c_uint64 * 12)()
    assert api.lib().zkaes_circuit_info_ks(int(kind), C.c_uint(128), C.c_size_t(length), C.c_size_t(alen), out) == 0
    assert list(out) == old_info(api, kind, length, alen)
    for which in range(3):
        new, old = api.circuit_matrix(kind, length, which, alen, key_bits=128), old_matrix(api, kind, length, alen, which)
        for a, b in zip(new, old):
            assert a.dtype == b.dtype and np.array_equal(a, b)


@pytest.mark.parametrize("key_bits", KEY_BITS)
@pytest.mark.parametrize("shape", range(5))
def test_counts_equal_the_closed_forms(api, shape, key_bits):
    kind, length, alen = shapes(api)[shape]
    ci = api.circuit_info(kind, length, alen, key_bits=key_bits)
    print(kind, length, alen, key_bits, {k: int(v) for k, v in ci.items()})
    want = closed_form(api, kind, key_bits // 32, length, alen)
    assert (ci["raw_constraints"], ci["raw_witness"], ci["raw_instance"]) == want
    assert ci["constraints"] == ci["instance"] + ci["witness"]                                 # square after padding
    if key_bits == 128:                                                                        # the Nk = 4 instance of each formula is what the existing circuits give
        old = old_info(api, kind, length, alen)
        assert (old[0], old[2], old[1]) == want
    assert ci["raw_instance"] == api.circuit_info(kind, length, alen)["raw_instance"]          # the public input does not know the key size


# ks(Nk), blk(Nk) of the ECB circuit's non-zero counts (A, B, C): recorded from the compiler (module docstring), exactly affine in nb
ECB_NNZ = {4: ((39_805, 67_253, 67_978), (160_410, 270_491, 276_065)), 6: ((32_463, 54_332, 55_722), (192_350, 324_548, 331_495)),
           8: ((51_883, 87_472, 88_318), (224_139, 378_287, 386_640))}
# (kind name, key_bits, L, A) -> (nnz A, B, C) of the chained modes' listed shapes
NNZ_PINS = {("cbc", 128, 32, 0): (361_183, 608_657, 620_904), ("cbc", 192, 32, 0): (417_710, 703_865, 719_530), ("cbc", 256, 32, 0): (500_710, 844_486, 862_407),
            ("ctr", 128, 17, 0): (360_540, 608_401, 621_039), ("ctr", 192, 17, 0): (417_078, 703_594, 719_643), ("ctr", 256, 17, 0): (500_076, 844_212, 862_529),
            ("gcm", 128, 17, 5): (801_796, 1_218_909, 1_228_246), ("gcm", 192, 17, 5): (922_451, 1_424_891, 1_437_710), ("gcm", 256, 17, 5): (1_068_967, 1_672_410, 1_690_886)}


@pytest.mark.parametrize("key_bits", KEY_BITS)
def test_non_zero_counts(api, key_bits):
    nk = key_bits // 32
    ks, blk = ECB_NNZ[nk]
    for nb in (0, 1, 2, 3):
        ci = api.circuit_info(api.CIRCUIT_AES, 16 * nb, key_bits=key_bits)
        assert (ci["nnz_a"], ci["nnz_b"], ci["nnz_c"]) == tuple(k + nb * b for k, b in zip(ks, blk)), nb
    for name, kind, length, alen in (("cbc", api.CIRCUIT_AES_CBC, 32, 0), ("ctr", api.CIRCUIT_AES_CTR, 17, 0), ("gcm", api.CIRCUIT_AES_GCM, 17, 5)):
        ci = api.circuit_info(kind, length, alen, key_bits=key_bits)
        assert (ci["nnz_a"], ci["nnz_b"], ci["nnz_c"]) == NNZ_PINS[(name, key_bits, length, alen)], name
    if key_bits == 128:                                                                        # the same numbers the older tests record: 16-byte ECB, GCM (17, 5)
        old = old_info(api, api.CIRCUIT_AES, 16, 0)
        assert tuple(old[3:6]) == tuple(k + b for k, b in zip(ks, blk))
        assert tuple(old_info(api, api.CIRCUIT_AES_GCM, 17, 5)[3:6]) == NNZ_PINS[("gcm", 128, 17, 5)]


def test_circuit_refusals(api):
    for bad in (0, 64, 127, 160, 512):
        with pytest.raises(api.ZkAesError):
            api.circuit_info(api.CIRCUIT_AES, 16, key_bits=bad)
        with pytest.raises(api.ZkAesError):
            api.circuit_matrix(api.CIRCUIT_AES_GCM, 16, 0, 0, key_bits=bad)
    for kind in (api.CIRCUIT_OPS_XOR, api.CIRCUIT_OPS_ADD):
        assert api.circuit_info(kind, 0)["raw_instance"] == 1
        assert api.circuit_info(kind, 0, key_bits=128) == api.circuit_info(kind, 0)
        for bits in (192, 256):
            with pytest.raises(api.ZkAesError):
                api.circuit_info(kind, 0, key_bits=bits)
    for kind in (api.CIRCUIT_AES, api.CIRCUIT_AES_CBC, api.CIRCUIT_AES_CTR):                   # aad outside GCM
        with pytest.raises(api.ZkAesError):
            api.circuit_info(kind, 16, 5, key_bits=256)
    with pytest.raises(api.ZkAesError, match="no HIP device|key_bits"):                        # the synthesizer refuses the same things (ahead of, or without, a device)
        api.synthesize_keys(16, key_bits=200)


def test_layout_macros_at_nk_4_6_8():
    """trace_layout.h through the preprocessor: its own static_asserts hold (it compiles), and the strides are 112 Nr - 48"""
    src = '#include "trace_layout.h"\n#include <cstdio>\nint main() { for (int nk = 4; nk <= 8; nk += 2) printf("%d %d %d %d %d %d\\n", nk, TRK_BLOCK0(nk), TRK_BLOCK_STRIDE(nk), ' \
          'TRK_BL_SB(nk), TRK_SBOX_KS(nk), (int)TRK_GCM_BYTES(nk, 1, 2)); return 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "layout.cpp"), "w").write(src)
        exe = os.path.join(d, "layout")
        subprocess.check_call(["g++", "-std=c++17", "-I", CSRC, os.path.join(d, "layout.cpp"), "-o", exe])
        rows = [tuple(int(v) for v in line.split()) for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()]
    assert [r[:5] for r in rows] == [(4, 272, 1072, 192, 40), (6, 296, 1296, 224, 32), (8, 376, 1520, 256, 52)]
    assert all(r[2] == 112 * (r[0] + 6) - 48 for r in rows)
    assert all(r[5] % 16 == 0 for r in rows)                                                  # GCM traces stay 16-byte multiples: the GHASH lanes store 16 bytes at a time


# ---- the kernels' source on the host
def test_keysize_trace_kernels_emulated_on_the_host():
    """the five trace kernels and k_witness_expand, the very header the library compiles for the device (csrc/kernels_witness.cuh), instantiated for NK = 6 and 8 and run lane by lane on the
    host under ASan + UBSan (tests/keysize_trace_emu.cpp, a stand-alone program: nothing is loaded into python): ECB nb = 1, 2, CBC nb = 2, CTR L = 17 under ff..ff,
    GCM (17, 5) and (1, 0), two proofs with different keys per launch, heap-exact message and key buffers, guard bytes behind the traces"""
    text = open(os.path.join(CSRC, "kernels_witness.cuh")).read()
    assert "hip" not in text.lower()
    for word in ("__shared__", "__syncthreads", "__shfl", "atomic"):                           # no LDS, no barrier, no cross-lane operation: what makes this emulation faithful
        assert word not in text
    for name in ("k_aes_trace", "k_aes_trace_ctr", "k_aes_trace_gcm", "k_ghash_trace", "aes_key_schedule", "k_witness_expand"):
        assert name in text
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "keysize_trace_emu")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC, "-I", os.path.join(ROOT, "tests"),
                               os.path.join(ROOT, "tests", "keysize_trace_emu.cpp")] + [os.path.join(CSRC, f) for f in ("circuit.cpp", "marlin_codec.cpp", "capi_host.cpp")] + ["-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
        print(out.stdout)
        lines = out.stdout.splitlines()
        assert lines[-1] == "total bad 0"
        # 2 key sizes x 6 shapes x 2 proofs
        assert out.stdout.count("unsatisfied 0, instance mismatches 0, rows unsatisfied after a ciphertext flip 1, after a flip of the last key byte") == 24
        assert out.stdout.count("surplus lanes wrote nothing") == 12
