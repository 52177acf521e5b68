"""AES-128-GCM on the host: gcm_encrypt / gcm_decrypt, the circuit's counts against ECB's, the matrices' shape, the host-only verifier, and the two trace kernels'
source run lane by lane under sanitizers (no GPU, no oracle).

Correctness of the GCM statement rests on the published vectors (McGrew-Viega test cases 1-4 for AES-128), an independent model (the FIPS-197 block of test_cbc_host.py
plus GHASH written from SP 800-38D Algorithm 1 over Python integers) and row-by-row constraint checks -- here through the host emulation of the kernels, on the GPU in
test_gpu_gcm.py; there is no upstream GCM circuit to be byte-identical to.
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from test_cbc_host import CLANG, CSRC, GOLD, ROOT, _encrypt_block, _pow2, _round_keys

# McGrew-Viega, "The Galois/Counter Mode of Operation (GCM)", appendix B, test cases 1-4: (key, iv, plaintext, aad, ciphertext, tag)
TC3_KEY = bytes.fromhex("feffe9928665731c6d6a8f9467308308")
TC3_IV = bytes.fromhex("cafebabefacedbaddecaf888")
TC3_PT = bytes.fromhex("d9313225f88406e5a55909c5aff5269a" "86a7a9531534f7da2e4c303d8a318a72" "1c3c0c95956809532fcf0e2449a6b525" "b16aedf5aa0de657ba637b391aafd255")
TC3_CT = bytes.fromhex("42831ec2217774244b7221b784d0d49c" "e3aa212f2c02a4e035c17e2329aca12e" "21d514b25466931c7d8f6a5aac84aa05" "1ba30b396a0aac973d58e091473f5985")
TC4_AAD = bytes.fromhex("feedfacedeadbeeffeedfacedeadbeefabaddad2")
VECTORS = [
    (bytes(16), bytes(12), b"", b"", b"", bytes.fromhex("58e2fccefa7e3061367f1d57a4e7455a")),
    (bytes(16), bytes(12), bytes(16), b"", bytes.fromhex("0388dace60b6a392f328c2b971b2fe78"), bytes.fromhex("ab6e47d42cec13bdf53a67b21257bddf")),
    (TC3_KEY, TC3_IV, TC3_PT, b"", TC3_CT, bytes.fromhex("4d5c2af327cd64a62cf35abd2ba6fab4")),
    (TC3_KEY, TC3_IV, TC3_PT[:60], TC4_AAD, TC3_CT[:60], bytes.fromhex("5bc94fbc3221a5db94fae95ae7121a47")),
]

# (L, A) -> raw_constraints, raw_instance, raw_witness, (nnz A, B, C), joint non-zeros, |H|, |K|, |X|: the figures DESIGN.md 9c records
COUNTS = {
    (1, 0): (500_845, 233, 500_221, (560_854, 901_325, 914_594), 1_975_153, 1 << 19, 1 << 21, 256),
    (16, 0): (516_685, 353, 515_821, (592_633, 920_762, 930_314), 2_041_390, 1 << 19, 1 << 21, 512),
    (17, 5): (688_557, 401, 687_381, (801_796, 1_218_909, 1_228_246), 2_721_342, 1 << 20, 1 << 22, 512),
    (16, 20): (552_077, 513, 550_797, (664_832, 961_647, 963_562), 2_185_155, 1 << 20, 1 << 22, 1024),
    (64, 0): (1_014_781, 737, 1_012_765, (1_182_868, 1_798_045, 1_809_713), 4_013_852, 1 << 20, 1 << 22, 1024),
}


def gf_mul(x, y):
    """SP 800-38D Algorithm 1 over Python integers: blocks are 128-bit integers read big-endian, so bit i of the standard (the leftmost is bit 0) is bit 127 - i here"""
    z, v = 0, y
    for i in range(128):
        if (x >> (127 - i)) & 1:
            z ^= v
        v = (v >> 1) ^ (0xE1 << 120 if v & 1 else 0)
    return z


def ghash_blocks(aad, ct):
    pad = lambda d: d + bytes(-len(d) % 16)
    data = pad(aad) + pad(ct) + (8 * len(aad)).to_bytes(8, "big") + (8 * len(ct)).to_bytes(8, "big")
    return [int.from_bytes(data[o:o + 16], "big") for o in range(0, len(data), 16)]


def model_ghash_chain(h, aad, ct):
    """Y_1 .. Y_M of SP 800-38D 6.4 as integers"""
    ys, y = [], 0
    for blk in ghash_blocks(aad, ct):
        y = gf_mul(y ^ blk, h)
        ys.append(y)
    return ys


def model_gcm(msg, key, iv, aad=b""):
    """SP 800-38D 7.1 for a 96-bit IV -> (ciphertext, tag)"""
    assert len(iv) == 12
    rks = _round_keys(key)
    h = int.from_bytes(_encrypt_block(bytes(16), rks), "big")
    ct = b""
    for b, off in enumerate(range(0, len(msg), 16)):
        stream = _encrypt_block(iv + (b + 2).to_bytes(4, "big"), rks)
        ct += bytes(x ^ s for x, s in zip(msg[off:off + 16], stream))
    s = model_ghash_chain(h, aad, ct)[-1]
    mask = int.from_bytes(_encrypt_block(iv + (1).to_bytes(4, "big"), rks), "big")
    return ct, (s ^ mask).to_bytes(16, "big")


@pytest.mark.parametrize("tc", range(4))
def test_published_vectors_through_model_and_library(api, tc):
    key, iv, pt, aad, ct, tag = VECTORS[tc]
    assert model_gcm(pt, key, iv, aad) == (ct, tag)
    assert api.gcm_encrypt(pt, key, iv, aad) == (ct, tag)
    assert api.gcm_decrypt(ct, key, iv, aad, tag) == pt


@pytest.mark.parametrize("alen", [0, 5, 16, 20])
@pytest.mark.parametrize("length", [0, 1, 15, 16, 17, 33])
def test_gcm_encrypt_matches_the_python_model(api, length, alen):
    rs = np.random.RandomState(0x6C30 + 64 * length + alen)
    for _ in range(2):
        msg, key, iv, aad = rs.bytes(length), rs.bytes(16), rs.bytes(12), rs.bytes(alen)
        ct, tag = api.gcm_encrypt(msg, key, iv, aad)
        assert (ct, tag) == model_gcm(msg, key, iv, aad)
        assert api.gcm_decrypt(ct, key, iv, aad, tag) == msg


def test_gcm_decrypt_fails_closed(api):
    """a flipped tag, ciphertext or aad byte: ok = 0 and not one byte of plaintext in the caller's buffer (through the C entry point, whose buffer the test owns)"""
    key, iv, pt, aad, ct, tag = VECTORS[3]
    flip = lambda d, i: d[:i] + bytes([d[i] ^ 0x04]) + d[i + 1:]
    for ct2, aad2, tag2 in ((ct, aad, flip(tag, 0)), (ct, aad, flip(tag, 15)), (flip(ct, 0), aad, tag), (flip(ct, 59), aad, tag), (ct, flip(aad, 19), tag), (ct, aad[:19], tag), (ct[:59], aad, tag)):
        assert api.gcm_decrypt(ct2, key, iv, aad2, tag2) is None
        out, ok = C.create_string_buffer(b"\xee" * 60, 60), C.c_int(7)
        rc = api.lib().zkaes_gcm_decrypt(ct2, C.c_size_t(len(ct2)), key, iv, aad2, C.c_size_t(len(aad2)), tag2, out, C.byref(ok))
        assert rc == 0 and ok.value == 0 and out.raw == b"\xee" * 60
    out, ok = C.create_string_buffer(b"\xee" * 60, 60), C.c_int(7)
    assert api.lib().zkaes_gcm_decrypt(ct, C.c_size_t(60), key, iv, aad, C.c_size_t(20), tag, out, C.byref(ok)) == 0 and ok.value == 1 and out.raw == pt


def test_gcm_refusals(api):
    key, iv = TC3_KEY, TC3_IV
    for bad_iv in (bytes(16), bytes(11), bytes(13), b""):                                      # only 96-bit IVs
        with pytest.raises(api.ZkAesError):
            api.gcm_encrypt(b"x", key, bad_iv)
        with pytest.raises(api.ZkAesError):
            api.gcm_decrypt(b"x", key, bad_iv, b"", bytes(16))
        with pytest.raises(api.ZkAesError):
            api.verify_encryption_gcm(None, b"", bad_iv, b"", b"x", bytes(16))
    for bad_key in (bytes(15), bytes(17)):
        with pytest.raises(api.ZkAesError):
            api.gcm_encrypt(b"x", bad_key, iv)
    for bad_tag in (bytes(12), bytes(15), bytes(17)):                                          # full tags only
        with pytest.raises(api.ZkAesError):
            api.gcm_decrypt(b"x", key, iv, b"", bad_tag)
        with pytest.raises(api.ZkAesError):
            api.verify_encryption_gcm(None, b"", iv, b"", b"x", bad_tag)
    with pytest.raises(api.ZkAesError):                                                        # a key's message has at least one byte
        api.circuit_info(api.CIRCUIT_AES_GCM, 0, 5)
    with pytest.raises(api.ZkAesError):
        api.circuit_matrix(api.CIRCUIT_AES_GCM, 0, 0)
    out = (C.c_uint64 * 12)()                                                                  # the generic query builds a GCM circuit without aad
    assert api.lib().zkaes_circuit_info(api.CIRCUIT_AES_GCM, C.c_size_t(16), out) == 0 and out[1] == 225 + 128
    assert api.lib().zkaes_circuit_info(api.CIRCUIT_AES_GCM, C.c_size_t(0), out) != 0


@pytest.mark.parametrize("shape", sorted(COUNTS))
def test_circuit_counts_relative_to_ecb(api, shape):
    """Relative to ECB at nb + 2 blocks (the message blocks, H and J_0; nb = ceil(L / 16), na = ceil(A / 16), M = na + nb + 1 multiplications, f = the bytes of the
    first GHASH block: min(A, 16) if there is aad, else min(L, 16)):

        GHASH   G  = 1152 M + 16384 (M - 1) + 1024 f + 8 (A + L - f)       (128 y + 896 q booleans + 128 parity rows per multiplication; 128 and gates per
                                                                             non-constant bit of X_m: all 128 from the second on; one chain xor per data bit)
        raw_constraints = E + 32 L + 8 A + 96 + 96 (nb + 1) + 381 + 384 + G - 512 (nb + 2)
        raw_witness     = W + 16 L + 96 (nb + 1) + 381 + 128 + (G - 128 M) - 256 (nb + 2)
        raw_instance    = 225 + 8 (A + L)

    (32 L: message witness, xor gate, input and equality per bit; 96: the iv inputs; 96 per counter block: its round-0 xor with the key, where ECB has 128 and the H
    block none; 381: the V table; 384: the tag's xor gates, inputs and equalities; 512 per block: ECB's message witnesses, round-0 xors, inputs and equalities.)"""
    length, alen = shape
    nb, na = (length + 15) // 16, (alen + 15) // 16
    m, f = na + nb + 1, (min(alen, 16) if alen else min(length, 16))
    e, c = api.circuit_info(api.CIRCUIT_AES, 16 * (nb + 2)), api.circuit_info(api.CIRCUIT_AES_GCM, length, alen)
    print(shape, {k: int(c[k]) for k in c})
    g = 1152 * m + 16384 * (m - 1) + 1024 * f + 8 * (alen + length - f)
    assert c["raw_constraints"] == e["raw_constraints"] + 32 * length + 8 * alen + 96 + 96 * (nb + 1) + 381 + 384 + g - 512 * (nb + 2)
    assert c["raw_witness"] == e["raw_witness"] + 16 * length + 96 * (nb + 1) + 381 + 128 + (g - 128 * m) - 256 * (nb + 2)
    assert c["raw_instance"] == 225 + 8 * (alen + length)
    want = COUNTS[shape]
    assert (c["raw_constraints"], c["raw_instance"], c["raw_witness"]) == want[:3]
    assert (c["nnz_a"], c["nnz_b"], c["nnz_c"]) == want[3]
    assert c["instance"] == want[7] and _pow2(int(c["constraints"])) == want[5]
    assert c["constraints"] == c["instance"] + c["witness"]                                    # square after padding


@pytest.mark.parametrize("shape", [(16, 0), (64, 0)])
def test_joint_non_zeros_and_domains(api, shape):
    """|K| from the joint matrix; the 64-byte record (test case 3's shape: six AES blocks, five multiplications) has the benchmark chunk's |H| = 2^20, |K| = 2^22 and
    |X| = 1024, inside the reference's SRS literal"""
    length, alen = shape
    keys = []
    for which in range(3):
        rowptr, col, coeff = api.circuit_matrix(api.CIRCUIT_AES_GCM, length, which, alen)
        rows = np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr.astype(np.int64)))
        keys.append(rows * (1 << 32) + col.astype(np.int64))
        assert int(np.abs(coeff).max()) <= (128 if which == 0 else 2)                          # the parity rows live in A; -128 is the weight of q's top bit
    joint = len(np.unique(np.concatenate(keys)))
    assert joint == COUNTS[shape][4] and _pow2(joint) == COUNTS[shape][6]
    if shape == (64, 0):
        assert joint <= 4_062_064


@pytest.mark.parametrize("which", [0, 1, 2])
def test_circuit_matrix_shape(api, which):
    ci = api.circuit_info(api.CIRCUIT_AES_GCM, 17, 5)
    rowptr, col, coeff = api.circuit_matrix(api.CIRCUIT_AES_GCM, 17, which, 5)
    assert len(rowptr) - 1 == ci["constraints"]
    assert rowptr[0] == 0 and rowptr[-1] == len(col) == len(coeff) == ci[("nnz_a", "nnz_b", "nnz_c")[which]]
    assert np.all(np.diff(rowptr.astype(np.int64)) >= 0)
    assert int(col.max()) < ci["instance"] + ci["witness"]
    assert ci["raw_instance"] == 225 + 8 * 22 and ci["instance"] == 512
    if which == 0:                    # 4 multiplications x 128 parity rows: y, seven q and 128 products each -- 40 in the first, whose X is the 5 aad bytes and constant zeros
        width = np.diff(rowptr.astype(np.int64))
        assert int(np.sum(width >= 48)) == 4 * 128 and int(np.sum(width >= 136)) == 3 * 128 and int(width.max()) <= 138


def test_verifier_does_not_accept_the_ecb_fixture(api):
    """the committed ECB verifying key and proof through the GCM verifier: never accepted, no crash.  The stored key carries its own public-input count (128), which no
    GCM shape has, so every call raises -- a wrong A + L at the verifier is an error; after the ark transport the key knows |X| only, and the verifier rejects instead"""
    vk = api.VerifyingKey.from_bytes(open(os.path.join(GOLD, "gpu_aes16_vk.bin"), "rb").read())
    proof = open(os.path.join(GOLD, "gpu_aes16_proof.bin"), "rb").read()
    ecb_ct = bytes.fromhex("3925841d02dc09fbdc118597196a0b32")
    tag = VECTORS[2][5]
    assert api.verify_encryption(vk, proof, ecb_ct) is True
    for aad, ct in ((b"", ecb_ct), (b"", ecb_ct[:1]), (TC4_AAD, ecb_ct), (TC4_AAD[:5], ecb_ct + b"\0"), (b"", TC3_CT), (b"", b"")):
        with pytest.raises(api.ZkAesError):
            api.verify_encryption_gcm(vk, proof, TC3_IV, aad, ct, tag)
    ark = api.VerifyingKey.from_ark_bytes(vk.to_ark_bytes())
    for aad, ct in ((b"", ecb_ct), (b"", ecb_ct[:3]), (b"ab", ecb_ct[:1]), (TC4_AAD, ecb_ct), (b"", TC3_CT)):
        assert api.verify_encryption_gcm(ark, proof, TC3_IV, aad, ct, tag) is False
        assert api.verify_encryption_gcm(ark, proof, bytes(12), aad, ct, bytes(16)) is False
    with pytest.raises(api.ZkAesError):
        api.verify_encryption_gcm(ark, proof, TC3_IV, b"", b"", tag)
    with pytest.raises(api.ZkAesError):
        api.verify_encryption_gcm(ark, proof[:-1], TC3_IV, b"", ecb_ct[:2], tag)


def test_host_entry_points_under_asan_ubsan():
    """tests/gcm_host_check.cpp with the three host-only sources under -fsanitize=address,undefined: the four vectors and 24 (L, A) shapes through zkaes_gcm_encrypt /
    zkaes_gcm_decrypt in buffers of exactly the sizes that exist, the fail-closed decrypt, the ECB fixtures whole and truncated at every length through the GCM verifier.
    A stand-alone program: nothing is loaded into python."""
    cxx = CLANG if os.path.exists(CLANG) else "g++"
    srcs = [os.path.join(ROOT, "tests", "gcm_host_check.cpp")] + [os.path.join(CSRC, f) for f in ("circuit.cpp", "marlin_codec.cpp", "capi_host.cpp")]
    flags = ["-x", "c++", "-O1", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC]
    if cxx == CLANG:
        flags += ["-mllvm", "-asan-globals=0"]        # (as tests/test_fuzz_host.py: this toolchain's ASan trips over its own registration of merged string literals)
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "gcm_host_check")
        subprocess.check_call([cxx] + flags + srcs + ["-o", exe])
        env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
        out = subprocess.run([exe, GOLD], capture_output=True, text=True, env=env, timeout=900)
        assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
        assert out.stdout.split() == ["gcm_host_check", "ok"]


def test_gcm_trace_kernels_emulated_on_the_host():
    """k_aes_trace_gcm, k_ghash_trace (with the helpers they share with the other trace kernels) and k_witness_expand, the very header the library compiles for the device
    (csrc/kernels_witness.cuh), run lane by lane on the host under ASan + UBSan (tests/gcm_trace_emu.cpp): (L, A) = (1, 0), (16, 0), (17, 5), (16, 20), (33, 16), two proofs
    per launch; message and header buffers hold exactly the bytes that exist, so an over-read of a partial block is a sanitizer report"""
    text = open(os.path.join(CSRC, "kernels_witness.cuh")).read()
    assert "hip" not in text.lower() and "k_aes_trace_gcm" in text and "k_ghash_trace" in text and "k_witness_expand" in text
    for word in ("__shared__", "__syncthreads", "__shfl", "atomic"):                            # no LDS, no barrier, no cross-lane operation: what makes this emulation faithful
        assert word not in text
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "gcm_trace_emu")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC, "-I", os.path.join(ROOT, "tests"),
                               os.path.join(ROOT, "tests", "gcm_trace_emu.cpp")] + [os.path.join(CSRC, f) for f in ("circuit.cpp", "marlin_codec.cpp", "capi_host.cpp")] + ["-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
        print(out.stdout)
        lines = out.stdout.splitlines()
        assert lines[-1] == "total bad 0"
        assert out.stdout.count("unsatisfied 0, instance mismatches 0, tail mismatches 0, rows unsatisfied after a tag flip 1,") == 10
