"""Key tags on the host: the tag's value, the tagged circuits' counts against closed forms, T = 0 unchanged through the new entry points, the chunk shape over the
default SRS, k_key_tag_trace's source run lane by lane under sanitizers, and the host-only verifiers under sanitizers (no GPU, no oracle).

A key synthesized with key_tag_blocks = T (1 or 2) proves, beside its mode's statement, tag_t = AES_K(D_t) for t < T and exposes the 128 T tag bits as the LAST public
inputs.  D_t is spelled out below, byte by byte.  The model is the pure-Python AES of test_keysize_host.py (checked there against FIPS-197 appendix C).

Closed forms, over the per-gate costs of test_keysize_host.py, with C(Nr) = 14,832 Nr - 560 the rows (= witnesses) of a block from its round 1 on: a tag
block's round 0 is constant ^ key and costs no gate, its rounds cost C(Nr), its 128 inputs 128 allocation rows and 128 equality rows.  Per tag block, in every mode:

    raw_constraints + C(Nr) + 256        raw_witness + C(Nr)        raw_instance + 128        S-box instances + 16 Nr
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from test_cbc_host import CLANG, CSRC, GOLD, ROOT, _pow2
from test_keysize_host import FIPS_PT, FIPS, expand_key, encrypt_block, ks_ecb

D = [bytes([0x7a, 0x6b, 0x61, 0x65, 0x73, 0x2d, 0x6b, 0x65, 0x79, 0x74, 0x61, t, 0x00, 0x00, 0x00, 0x00]) for t in (0, 1)]


def model_key_tag(key, blocks=2):
    rks = expand_key(key)[1]
    return b"".join(encrypt_block(D[t], rks) for t in range(blocks))


def test_the_constant_blocks():
    assert D[0][:11] == D[1][:11] == b"zkaes-keyta" and all(D[0][:11])                          # no zero byte ahead of t: D_t is not the zero block behind GCM's H
    assert (D[0][11], D[1][11]) == (0, 1)
    assert D[0][12:] == D[1][12:] == bytes(4)                                                   # a GCM counter block of a 96-bit IV ends in be32(n), n >= 1


@pytest.mark.parametrize("klen", [16, 24, 32])
def test_tag_value(api, klen):
    key = bytes(range(klen))                                                                    # FIPS-197 appendix C.1, C.2, C.3
    assert ks_ecb(FIPS_PT, key) == bytes.fromhex(FIPS[klen])                                    # (the model is the checked one)
    want = model_key_tag(key)
    assert len(want) == 32 and want[:16] != want[16:]
    assert api.ecb_ciphertext(D[0] + D[1], key) == want
    assert api.key_tag(key) == api.key_tag(key, 2) == want
    assert api.key_tag(key, 1) == want[:16]
    other = bytes([key[0] ^ 1]) + key[1:]
    assert api.key_tag(other, 2)[:16] != want[:16] and api.key_tag(other, 2)[16:] != want[16:]


def test_tag_refusals(api):
    for klen in (0, 15, 20, 33):
        with pytest.raises(api.ZkAesError):
            api.key_tag(bytes(klen), 1)
    for blocks in (0, 3, -1):
        with pytest.raises(api.ZkAesError):
            api.key_tag(bytes(16), blocks)
    # and at the C boundary itself, which the Python checks above never reach
    out = C.create_string_buffer(48)
    L = api.lib()
    assert L.zkaes_key_tag(bytes(20), C.c_size_t(20), C.c_size_t(1), out) != 0 and b"16, 24 or 32" in L.zkaes_last_error()
    for blocks in (0, 3):
        assert L.zkaes_key_tag(bytes(16), C.c_size_t(16), C.c_size_t(blocks), out) != 0
    for bad in (3, 7):
        with pytest.raises(api.ZkAesError):
            api.circuit_info(api.CIRCUIT_AES, 16, key_tag_blocks=bad)
        with pytest.raises(api.ZkAesError):
            api.circuit_matrix(api.CIRCUIT_AES, 16, 0, key_tag_blocks=bad)
        rows = (C.c_uint64 * 12)()
        assert L.zkaes_circuit_info_kt(api.CIRCUIT_AES, C.c_uint(128), C.c_uint(bad), C.c_size_t(16), C.c_size_t(0), rows) != 0
        with pytest.raises(api.ZkAesError, match="no HIP device|key_tag_blocks"):              # the synthesizer refuses the same (ahead of, or without, a device)
            api.synthesize_keys(16, key_tag_blocks=bad)
    for kind in (api.CIRCUIT_OPS_XOR, api.CIRCUIT_OPS_ADD):                                     # the ops kinds have no key to tag
        assert api.circuit_info(kind, 0, key_tag_blocks=0) == api.circuit_info(kind, 0)
        with pytest.raises(api.ZkAesError):
            api.circuit_info(kind, 0, key_tag_blocks=1)


def shapes(api):
    return [(api.CIRCUIT_AES, 16, 0), (api.CIRCUIT_AES_CBC, 32, 0), (api.CIRCUIT_AES_CTR, 17, 0), (api.CIRCUIT_AES_GCM, 17, 5)]


def ks_matrix(api, kind, key_bits, length, alen, which):
    L = api.lib()
    rows, nnz = C.c_uint64(), C.c_uint64()
    head = (int(kind), C.c_uint(key_bits), C.c_size_t(length), C.c_size_t(alen), which)
    assert L.zkaes_circuit_matrix_ks(*head, C.byref(rows), C.byref(nnz), None, None, None) == 0
    rowptr, col, coeff = np.zeros(rows.value + 1, dtype=np.uint32), np.zeros(nnz.value, dtype=np.uint32), np.zeros(nnz.value, dtype=np.int64)
    assert L.zkaes_circuit_matrix_ks(*head, None, None, rowptr.ctypes.data_as(C.c_void_p), col.ctypes.data_as(C.c_void_p), coeff.ctypes.data_as(C.c_void_p)) == 0
    return rowptr, col, coeff


@pytest.mark.parametrize("key_bits", [128, 256])
@pytest.mark.parametrize("shape", range(4))
def test_no_tag_blocks_is_todays_circuit(api, shape, key_bits):
    """the info and all three matrices through the key-tag entry points at T = 0 equal those of zkaes_circuit_info_ks / zkaes_circuit_matrix_ks, element for element"""
    kind, length, alen = shapes(api)[shape]
    new, old = (C.c_uint64 * 12)(), (C.c_uint64 * 12)()
    assert api.lib().zkaes_circuit_info_kt(int(kind), C.c_uint(key_bits), C.c_uint(0), C.c_size_t(length), C.c_size_t(alen), new) == 0
    assert api.lib().zkaes_circuit_info_ks(int(kind), C.c_uint(key_bits), C.c_size_t(length), C.c_size_t(alen), old) == 0
    assert list(new) == list(old)
    for which in range(3):
        a, b = api.circuit_matrix(kind, length, which, alen, key_bits=key_bits, key_tag_blocks=0), ks_matrix(api, kind, key_bits, length, alen, which)
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and np.array_equal(x, y)


def core_rows(nr):
    return 14_832 * nr - 560


@pytest.mark.parametrize("key_bits", [128, 192, 256])
@pytest.mark.parametrize("blocks", [1, 2])
@pytest.mark.parametrize("shape", range(4))
def test_counts_equal_the_closed_forms(api, shape, blocks, key_bits):
    kind, length, alen = shapes(api)[shape]
    nr = key_bits // 32 + 6
    assert core_rows(nr) == 16 * 884 * nr + (16 * 3 + 512) * (nr - 1) + 128 * nr               # the per-gate costs of test_keysize_host.py
    base = api.circuit_info(kind, length, alen, key_bits=key_bits)
    ci = api.circuit_info(kind, length, alen, key_bits=key_bits, key_tag_blocks=blocks)
    print(kind, length, alen, key_bits, blocks, {k: int(v) for k, v in ci.items()})
    assert ci["raw_constraints"] == base["raw_constraints"] + blocks * (core_rows(nr) + 256)
    assert ci["raw_witness"] == base["raw_witness"] + blocks * core_rows(nr)
    assert ci["raw_instance"] == base["raw_instance"] + 128 * blocks
    assert ci["constraints"] == ci["instance"] + ci["witness"]                                  # square after padding
    assert ci["instance"] == _pow2(int(ci["raw_instance"]))
    # S-box instances: every one is 884 witnesses and nothing else in a block is, so the witness count pins them: 16 Nr more per tag block
    xtime_and_xors = (16 * 3 + 512) * (nr - 1) + 128 * nr
    assert (int(ci["raw_witness"]) - int(base["raw_witness"]) - blocks * xtime_and_xors) == 884 * 16 * nr * blocks


def _joint_nnz(api, kind, length, blocks):
    keys = []
    for which in range(3):
        rowptr, col, _ = api.circuit_matrix(kind, length, which, key_tag_blocks=blocks)
        rows = np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr.astype(np.int64)))
        keys.append(rows * (1 << 32) + col.astype(np.int64))
    return len(np.unique(np.concatenate(keys)))


@pytest.mark.parametrize("mode", ["ecb", "ctr"])
def test_chunk_shape_is_the_six_block_chunk(api, mode):
    """4 data blocks + 2 tag blocks, and 5 + 1, of AES-128 have the shape of today's 6-block chunk: |H| = 2^20, |K| = 2^22, |X| = 1024, so the default universal SRS holds
    them and the transform and MSM op lists have the same sizes.  circuit_info is host-only and leaves h, k to the key, so they are derived as the prover derives them
    (test_cbc_host.py): |H| = the padded constraint count rounded up to a power of two, |K| likewise from the joint matrix's non-zeros.  The padded constraint count
    itself is NOT equal: a tag block has no message witnesses and no round-0 xor gates, 256 rows fewer than a data block (926,400 / 926,144 / 925,888 for ECB 6 + 0,
    5 + 1, 4 + 2); what the issue's 2^20 names is that count rounded up to the domain."""
    kind = api.CIRCUIT_AES if mode == "ecb" else api.CIRCUIT_AES_CTR
    cases = [(96, 0), (64, 2)] + ([(80, 1)] if mode == "ecb" else [])
    got = {}
    for length, blocks in cases:
        ci = api.circuit_info(kind, length, key_tag_blocks=blocks)
        joint = _joint_nnz(api, kind, length, blocks)
        got[(length, blocks)] = (_pow2(int(ci["constraints"])), int(ci["instance"]), _pow2(int(ci["constraints"])), _pow2(joint))
        print(mode, length, blocks, "constraints", int(ci["constraints"]), "raw_instance", int(ci["raw_instance"]), "joint nnz", joint, got[(length, blocks)])
        assert ci["raw_instance"] == (1 if mode == "ecb" else 129) + 8 * length + 128 * blocks
    for case in cases:
        assert got[case] == got[(96, 0)] == (1 << 20, 1024, 1 << 20, 1 << 22), case
    if mode == "ecb":
        c = [int(api.circuit_info(kind, length, key_tag_blocks=blocks)["constraints"]) for length, blocks in cases]
        assert c == [926_400, 925_888, 926_144]


def test_layout_macros_with_tag_slots():
    """trace_layout.h through the preprocessor: its static_asserts hold (it compiles); slot 0 is the mode's length rounded up to 16, slots follow at the block stride,
    T = 0 leaves every length what it was"""
    src = '#include "trace_layout.h"\n#include <cstdio>\nint main() { for (int nk = 4; nk <= 8; nk += 2) { long m[4] = {TRK_ECB_BYTES(nk, 2), TRK_CBC_BYTES(nk, 2), TRK_CTR_BYTES(nk, 2), ' \
          '(long)TRK_GCM_BYTES(nk, 1, 2)}; for (int i = 0; i < 4; i++) printf("%d %ld %ld %ld %ld %ld\\n", nk, m[i], (long)TRK_KT(m[i]), (long)TRK_KT_BYTES(nk, m[i], 0), ' \
          '(long)TRK_KT_BYTES(nk, m[i], 1), (long)TRK_KT_BYTES(nk, m[i], 2)); } return 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "layout.cpp"), "w").write(src)
        exe = os.path.join(d, "layout")
        subprocess.check_call(["g++", "-std=c++17", "-I", CSRC, os.path.join(d, "layout.cpp"), "-o", exe])
        rows = [tuple(int(v) for v in line.split()) for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()]
    assert len(rows) == 12
    for nk, mode_bytes, slot0, t0, t1, t2 in rows:
        stride = 112 * (nk + 6) - 48
        assert slot0 == (mode_bytes + 15) // 16 * 16 and t0 == mode_bytes and t1 == slot0 + stride and t2 == slot0 + 2 * stride
        assert t1 % 16 == 0 and t2 % 16 == 0
    assert rows[0][:3] == (4, 272 + 2 * 1072, 272 + 2 * 1072) and rows[8][:3] == (8, 376 + 2 * 1520, 376 + 2 * 1520 + 8)       # ECB-256 ends 8 mod 16


# ---- the kernel's source on the host
def test_key_tag_kernel_emulated_on_the_host():
    """the mode's trace kernel(s), k_key_tag_trace and k_witness_expand, the very header the library compiles for the device (csrc/kernels_witness.cuh), run lane by lane on
    the host under ASan + UBSan (tests/keytag_trace_emu.cpp, a stand-alone program: nothing is loaded into python): ECB-128 16 B T = 1, ECB-256 16 B T = 2, CBC-192 32 B T = 1,
    CTR-128 17 B T = 2, GCM-256 (17, 5) T = 1, two proofs with different keys per launch"""
    text = open(os.path.join(CSRC, "kernels_witness.cuh")).read()
    assert "hip" not in text.lower() and "k_witness_expand" in text
    assert text.count("void k_key_tag_trace(") == 1
    kernel = text[text.index("void k_key_tag_trace("):]
    kernel = kernel[:kernel.index("\n}\n")]
    for word in ("__shared__", "__syncthreads", "__shfl", "atomic"):                           # no LDS, no barrier, no cross-lane operation: what makes this emulation faithful
        assert word not in text
    assert "aes_key_schedule<NK>(key, sbox, w, nullptr)" in kernel and "aes_block_rounds<true, NK>" in kernel      # the schedule in registers, no schedule stores
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "keytag_trace_emu")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC, "-I", os.path.join(ROOT, "tests"),
                               os.path.join(ROOT, "tests", "keytag_trace_emu.cpp")] + [os.path.join(CSRC, f) for f in ("circuit.cpp", "marlin_codec.cpp", "capi_host.cpp")] + ["-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
        print(out.stdout)
        assert out.stdout.splitlines()[-1] == "total bad 0"
        assert out.stdout.count("unsatisfied 0, instance mismatches 0, rows unsatisfied after a tag flip 1") == 10       # 5 shapes x 2 proofs
        assert out.stdout.count("bytes whose writer count is off 0") == 5
        assert out.stdout.count("bytes outside the slots touched 0, slot bytes the mode's kernels wrote 0, proofs whose head differs from the untagged trace 0") == 5


def test_host_entry_points_under_asan_ubsan():
    """tests/keytag_host_check.cpp with the three host-only sources under -fsanitize=address,undefined: zkaes_key_tag into exactly sized buffers, the circuit queries, and
    the committed ECB fixture proof -- whole, truncated at every length, garbage -- through zkaes_verify_chunked_kt and zkaes_verify_encryption_gcm_kt under the stored
    key, the transported key and a key whose |X| fits a tagged statement: never accepted.  A stand-alone program: nothing is loaded into python."""
    cxx = CLANG if os.path.exists(CLANG) else "g++"
    srcs = [os.path.join(ROOT, "tests", "keytag_host_check.cpp")] + [os.path.join(CSRC, f) for f in ("circuit.cpp", "marlin_codec.cpp", "capi_host.cpp")]
    flags = ["-x", "c++", "-O1", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC]
    if cxx == CLANG:
        flags += ["-mllvm", "-asan-globals=0"]        # (as tests/test_fuzz_host.py: this toolchain's ASan trips over its own registration of merged string literals)
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "keytag_host_check")
        subprocess.check_call([cxx] + flags + srcs + ["-o", exe])
        env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
        out = subprocess.run([exe, GOLD], capture_output=True, text=True, env=env, timeout=900)
        assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
        assert out.stdout.split() == ["keytag_host_check", "ok"]


def test_tagged_verifiers_never_accept_the_ecb_fixture(api):
    """the committed ECB verifying key and proof through the Python forms of the tagged verifiers: raises or rejects, never accepts"""
    vk = api.VerifyingKey.from_bytes(open(os.path.join(GOLD, "gpu_aes16_vk.bin"), "rb").read())
    vk_ark = api.VerifyingKey.from_ark_bytes(open(os.path.join(GOLD, "gpu_aes16_vk_ark.bin"), "rb").read())
    proof = open(os.path.join(GOLD, "gpu_aes16_proof.bin"), "rb").read()
    ecb_ct = bytes.fromhex("3925841d02dc09fbdc118597196a0b32")
    assert api.verify_encryption(vk, proof, ecb_ct) is True
    tag = api.key_tag(bytes.fromhex("2b7e151628aed2a6abf7158809cf4f3c"), 2)
    for t in (tag[:16], tag):
        with pytest.raises(api.ZkAesError):                                                     # the stored key knows its 128 public bits
            api.verify_chunked_tagged(vk, api.CIRCUIT_AES, [proof], ecb_ct, t)
        with pytest.raises(api.ZkAesError):
            api.verify_encryption_gcm_tagged(vk, proof, bytes(12), b"", ecb_ct, bytes(16), t)
        assert api.verify_chunked_tagged(vk_ark, api.CIRCUIT_AES, [proof, proof], ecb_ct * 2, t) == [False, False]
        assert api.verify_chunked_tagged(vk_ark, api.CIRCUIT_AES_CTR, [proof], ecb_ct + b"x", t, iv=bytes(16)) == [False]
        assert api.verify_encryption_gcm_tagged(vk_ark, proof, bytes(12), b"", ecb_ct, bytes(16), t) is False
    for bad in (b"", tag[:15], tag + b"\0"):
        with pytest.raises(api.ZkAesError):
            api.verify_chunked_tagged(vk_ark, api.CIRCUIT_AES, [proof], ecb_ct, bad)
        with pytest.raises(api.ZkAesError):
            api.verify_encryption_gcm_tagged(vk_ark, proof, bytes(12), b"", ecb_ct, bytes(16), bad)
    with pytest.raises(api.ZkAesError):
        api.verify_chunked_tagged(vk_ark, api.CIRCUIT_AES_GCM, [proof], ecb_ct, tag)
    with pytest.raises(api.ZkAesError):
        api.verify_chunked_tagged(vk_ark, api.CIRCUIT_AES, [proof], ecb_ct, tag, iv=bytes(16))     # ECB takes no iv
    with pytest.raises(api.ZkAesError):
        api.verify_chunked_tagged(vk_ark, api.CIRCUIT_AES_CBC, [proof], ecb_ct, tag)               # CBC needs one
