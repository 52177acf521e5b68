"""Selective disclosure on the host: reveal = 0 unchanged through the new entry points, the closed forms of the reveal gates against the builder's counts,
the chunk shape over the default SRS, reveal_bytes against a one-liner, the refusals that need no device, the verifier's two invalid-argument cases, and three stand-alone
programs under sanitizers -- k_reveal_trace's source run lane by lane, the statement layer's mask slices, the host-only verifiers (no GPU, no oracle).

A key synthesized with reveal = True proves, beside its mode's statement, its key tag and its digest, revealed[i] = mask_i ? M[i] : 0 for a message of L bytes and a mask
chosen per proof, and exposes the mask (ceil(L / 8) bytes), then revealed (L bytes), as the LAST public inputs.

Closed forms (csrc/circuit.cpp reveal()), with mb = ceil(L / 8): 8 mb + 8 L inputs and their booleanity rows, 8 mb - L rows that pin the mask bits at or
beyond L to zero, 8 L product rows mask_i * m_ij = r_ij -- rows 16 mb + 15 L (17 L when 8 divides L), witnesses 0, instance 8 mb + 8 L (9 L when 8 divides L).
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from test_cbc_host import CLANG, CSRC, GOLD, ROOT

HOST_SOURCES = [os.path.join(CSRC, f) for f in ("circuit.cpp", "marlin_codec.cpp", "capi_host.cpp")]


def _msg(n, salt=0):
    return bytes((37 * i + 11 + salt) & 0xff for i in range(n))


def shapes(api):
    """(circuit, key bits, L, A, T, digest): the emulator's shapes, and the closed forms' lengths over CTR (the mode that takes every length)"""
    return [(api.CIRCUIT_AES, 128, 16, 0, 0, None), (api.CIRCUIT_AES_CTR, 128, 1, 0, 1, "final"), (api.CIRCUIT_AES_CTR, 128, 17, 0, 1, "final"), (api.CIRCUIT_AES_CBC, 192, 32, 0, 0, None),
            (api.CIRCUIT_AES_GCM, 256, 17, 5, 0, None), (api.CIRCUIT_AES, 256, 64, 0, 2, "chain")] + [(api.CIRCUIT_AES_CTR, 128, n, 0, 0, None) for n in (1, 16, 17, 32, 64)]


def test_reveal_zero_is_the_digest_query(api):
    """reveal = 0 through the _rv entry points answers element for element what the _pd entry points answer"""
    L = api.lib()
    for circuit, bits, n, a, t, digest in shapes(api)[:6]:
        d = api._DIGEST_NAMES.index(digest)
        pd, rv = (C.c_uint64 * 12)(), (C.c_uint64 * 12)()
        assert L.zkaes_circuit_info_pd(circuit, C.c_uint(bits), C.c_uint(t), C.c_uint(d), C.c_uint64(0), C.c_size_t(n), C.c_size_t(a), pd) == 0
        assert L.zkaes_circuit_info_rv(circuit, C.c_uint(bits), C.c_uint(t), C.c_uint(d), C.c_uint64(0), C.c_uint(0), C.c_size_t(n), C.c_size_t(a), rv) == 0
        assert list(pd) == list(rv)
        assert api.circuit_info(circuit, n, a, bits, t, digest, 0, reveal=False) == api.circuit_info(circuit, n, a, bits, t, digest)
    circuit, bits, n, a, t = api.CIRCUIT_AES_CTR, 128, 17, 0, 1
    for which in range(3):
        rows, nnz = C.c_uint64(), C.c_uint64()
        assert L.zkaes_circuit_matrix_pd(circuit, C.c_uint(bits), C.c_uint(t), C.c_uint(2), C.c_uint64(0), C.c_size_t(n), C.c_size_t(a), which, C.byref(rows), C.byref(nnz), None, None, None) == 0
        rowptr, col, coeff = np.zeros(rows.value + 1, np.uint32), np.zeros(nnz.value, np.uint32), np.zeros(nnz.value, np.int64)
        assert L.zkaes_circuit_matrix_pd(circuit, C.c_uint(bits), C.c_uint(t), C.c_uint(2), C.c_uint64(0), C.c_size_t(n), C.c_size_t(a), which, None, None, rowptr.ctypes.data_as(C.c_void_p),
                                         col.ctypes.data_as(C.c_void_p), coeff.ctypes.data_as(C.c_void_p)) == 0
        got = api.circuit_matrix(circuit, n, which, a, bits, t, "final", 0, reveal=False)
        assert (got[0] == rowptr).all() and (got[1] == col).all() and (got[2] == coeff).all()


def reveal_size(n):
    """(rows, witnesses, instance variables) the reveal gates add for a message of n bytes"""
    mb = (n + 7) // 8
    return 16 * mb + 15 * n, 0, 8 * mb + 8 * n


def test_closed_form_counts(api):
    assert [reveal_size(n) for n in (8, 16, 64)] == [(17 * n, 0, 9 * n) for n in (8, 16, 64)]            # the issue's form for 8 | L
    assert reveal_size(1) == (31, 0, 16) and reveal_size(17) == (303, 0, 160)
    for circuit, bits, n, a, t, digest in shapes(api):
        plain = api.circuit_info(circuit, n, a, bits, t, digest)
        got = api.circuit_info(circuit, n, a, bits, t, digest, 0, reveal=True)
        rows, wits, inst = reveal_size(n)
        print(circuit, bits, n, a, t, digest, "reveal rows", rows, "witnesses", wits, "instance", inst, "->", got["raw_constraints"], got["raw_witness"], got["raw_instance"])
        assert got["raw_constraints"] == plain["raw_constraints"] + rows
        assert got["raw_witness"] == plain["raw_witness"] + wits
        assert got["raw_instance"] == plain["raw_instance"] + inst


def test_reveal_rows_are_what_the_design_says(api):
    """CTR-128 17 B: behind the R = 0 circuit's rows come 24 booleanity rows of the mask, 7 pins (mask bits 17 .. 23, A = the bit, B = One, C empty), then per message byte
    8 booleanity rows of its revealed bits and 8 product rows with ONE entry a side: the byte's mask input in A, the message witness (witness 8 i + k: the message is
    allocated first) in B, the revealed input in C"""
    n, mb = 17, 3
    plain = api.circuit_info(api.CIRCUIT_AES_CTR, n)
    info = api.circuit_info(api.CIRCUIT_AES_CTR, n, reveal=True)
    A, B, Cm = [api.circuit_matrix(api.CIRCUIT_AES_CTR, n, which, reveal=True) for which in range(3)]
    r0, ri0, ni = int(plain["raw_constraints"]), int(plain["raw_instance"]), int(info["instance"])
    row = lambda m, r: list(zip(m[1][m[0][r]:m[0][r + 1]].tolist(), m[2][m[0][r]:m[0][r + 1]].tolist()))
    for i in range(n, 8 * mb):
        r = r0 + 8 * mb + (i - n)
        assert row(A, r) == [(ri0 + i, 1)] and row(B, r) == [(0, 1)] and row(Cm, r) == []
    at = r0 + 8 * mb + (8 * mb - n)
    for i in range(n):
        for k in range(8):
            r = at + 16 * i + 8 + k
            assert row(A, r) == [(ri0 + i, 1)] and row(B, r) == [(ni + 8 * i + k, 1)] and row(Cm, r) == [(ri0 + 8 * mb + 8 * i + k, 1)]
    assert at + 16 * n == info["raw_constraints"]


def _joint_nnz(api, n):
    seen = []
    for which in range(3):
        rowptr, col, _ = api.circuit_matrix(api.CIRCUIT_AES, n, which, reveal=True)
        rows = np.repeat(np.arange(len(rowptr) - 1, dtype=np.uint64), np.diff(rowptr).astype(np.int64))
        seen.append((rows << np.uint64(32)) | col.astype(np.uint64))
    return len(np.unique(np.concatenate(seen)))


@pytest.mark.parametrize("n", [64, 96])
def test_chunk_shape_over_the_default_srs(api, n):
    """ECB-128 64 B and 96 B with reveal stay inside |H| = 2^20 and |K| = 2^22, the domains of today's headline chunks; |X| grows from 1024 to 2048 (1 + 8 n + n + 8 n
    inputs: 1089 and 1633).  h and k derived as the prover derives them (test_digest_host.py)"""
    info = api.circuit_info(api.CIRCUIT_AES, n, reveal=True)
    h = 1
    while h < max(info["constraints"], info["instance"] + info["witness"]):
        h *= 2
    joint = _joint_nnz(api, n)
    k = 1
    while k < joint:
        k *= 2
    print("L =", n, "rows", info["raw_constraints"], "padded", info["constraints"], "joint non-zeros", joint, "|H|", h, "|K|", k, "|X|", info["instance"])
    assert h == 1 << 20 and k == 1 << 22
    assert info["raw_instance"] - 1 == 8 * n + n + 8 * n and info["instance"] == 2048
    assert api.circuit_info(api.CIRCUIT_AES, n)["instance"] == 1024


def test_reveal_bytes_is_the_one_liner(api):
    for n in (1, 7, 8, 16, 17, 64):
        m = _msg(n, n)
        for mask in (bytes((n + 7) // 8), api.reveal_mask(range(n), n), api.reveal_mask([0], n), api.reveal_mask([n - 1], n), api.reveal_mask(range(0, n, 2), n), api.reveal_mask([i for i in (15, 16) if i < n], n)):
            assert api.reveal_bytes(m, mask) == bytes(m[i] if (mask[i // 8] >> (i % 8)) & 1 else 0 for i in range(n))
    # the one conversion: bytes, indices, ranges
    assert api.reveal_mask([0, range(3, 5), 9], 10) == bytes([0x19, 0x02]) == api.reveal_mask(bytes([0x19, 0x02]), 10)
    assert api.reveal_bytes(b"abcdefghij", [0, range(3, 5), 9]) == b"a\0\0de\0\0\0\0j"
    assert api.reveal_mask([], 17) == bytes(3) and api.reveal_mask(range(40, 72), 100)[5:9] == b"\xff" * 4
    for bad in ([10], [-1], [range(8, 12)]):
        with pytest.raises(api.ZkAesError):
            api.reveal_mask(bad, 10)
    with pytest.raises(api.ZkAesError):
        api.reveal_mask(bytes(3), 10)
    with pytest.raises(api.ZkAesError, match="at or beyond"):
        api.reveal_bytes(b"abcdefghij", bytes([0, 0x04]))                                           # bit 10 of a 10-byte message


def test_refusals(api):
    L = api.lib()
    out = (C.c_uint64 * 12)()
    assert L.zkaes_circuit_info_rv(api.CIRCUIT_AES, C.c_uint(128), C.c_uint(0), C.c_uint(0), C.c_uint64(0), C.c_uint(2), C.c_size_t(16), C.c_size_t(0), out) != 0
    assert b"reveal must be 0 or 1" in L.zkaes_last_error()
    for kind in (api.CIRCUIT_OPS_XOR, api.CIRCUIT_OPS_ADD):
        assert api.circuit_info(kind, 0, reveal=False) == api.circuit_info(kind, 0)
        with pytest.raises(api.ZkAesError, match="reveal must be 0"):
            api.circuit_info(kind, 0, reveal=True)
        with pytest.raises(api.ZkAesError):
            api.circuit_matrix(kind, 0, 0, reveal=True)
    with pytest.raises(api.ZkAesError, match="no reveal form"):                                    # a GCM segment circuit: kind 6 through the plain query
        api.circuit_info(6, 16, reveal=True)
    with pytest.raises(api.ZkAesError, match="multiple of 64"):                                     # the digest's own refusals stand
        api.circuit_info(api.CIRCUIT_AES, 16, digest="chain", reveal=True)
    with pytest.raises(api.ZkAesError):
        api.circuit_info(api.CIRCUIT_AES, 17, reveal=True)
    with pytest.raises(api.ZkAesError, match="no HIP device|reveal must be 0"):                     # the synthesizer refuses the same (ahead of, or without, a device)
        api.synthesize_keys(0, circuit=api.CIRCUIT_OPS_XOR, reveal=True)


def test_verifiers_refuse_the_two_invalid_arguments(api):
    """a mask bit at or beyond the length and a non-zero revealed byte under a zero mask bit RAISE in every entry that takes (mask, revealed), whatever the key; and the
    committed ECB proof, a proof of a key without reveal, is never accepted by a reveal verifier"""
    vk = api.VerifyingKey.from_bytes(open(os.path.join(GOLD, "gpu_aes16_vk.bin"), "rb").read())
    proof = open(os.path.join(GOLD, "gpu_aes16_proof.bin"), "rb").read()
    ct = bytes.fromhex("3925841d02dc09fbdc118597196a0b32")
    iv = bytes(range(12))
    assert api.verify_encryption(vk, proof, ct)
    hidden_but_shown = (bytes([0xfe, 0xff]), bytes([1]) + bytes(15))
    for mask, revealed in (hidden_but_shown, (bytes(2), bytes(15) + b"\x01")):
        with pytest.raises(api.ZkAesError, match="mask bit is 0"):
            api.verify_reveal_chunked(vk, api.CIRCUIT_AES, [proof], ct, mask, revealed)
        with pytest.raises(api.ZkAesError, match="mask bit is 0"):
            api.verify_encryption_gcm_reveal(vk, proof, iv, b"", ct, bytes(16), mask, revealed)
        with pytest.raises(api.ZkAesError, match="mask bit is 0"):
            api.chunk_public_inputs(api.CIRCUIT_AES, ct, mask=mask, revealed=revealed)
    beyond = bytes([0, 0, 0x02])
    with pytest.raises(api.ZkAesError, match="at or beyond"):
        api.verify_reveal_chunked(vk, api.CIRCUIT_AES_CTR, [proof], ct + b"\x00", beyond, bytes(17), header=bytes(16))
    with pytest.raises(api.ZkAesError, match="at or beyond"):
        api.verify_encryption_gcm_reveal(vk, proof, iv, b"", ct + b"\x00", bytes(16), beyond, bytes(17))
    with pytest.raises(api.ZkAesError, match="at or beyond"):
        api.chunk_public_inputs(api.CIRCUIT_AES_CTR, ct + b"\x00", header=bytes(16), mask=beyond, revealed=bytes(17))
    with pytest.raises(api.ZkAesError):
        api.verify_reveal_chunked(vk, api.CIRCUIT_AES, [proof], ct, bytes(2), bytes(15))            # revealed of another length
    with pytest.raises(api.ZkAesError):
        api.chunk_public_inputs(api.CIRCUIT_AES, ct, mask=bytes(2))                                 # mask without revealed
    # well-formed arguments: the stored key knows its 128 public bits, so a reveal statement is an error; the same key through the ark transport (|X| alone) rejects
    with pytest.raises(api.ZkAesError, match="not the ones this key was synthesized for"):
        api.verify_reveal_chunked(vk, api.CIRCUIT_AES, [proof], ct, bytes(2), bytes(16))
    ark = api.VerifyingKey.from_ark_bytes(vk.to_ark_bytes())
    assert api.verify_reveal_chunked(ark, api.CIRCUIT_AES, [proof], ct, bytes(2), bytes(16)) == [False]
    assert api.verify_encryption_gcm_reveal(ark, proof, iv, b"", ct, bytes(16), bytes(2), bytes(16)) is False
    # the rows batch verification gets: the plain row, then the mask's bits, then revealed's
    m = _msg(32, 3)
    mask = api.reveal_mask(range(12, 20), 32)
    rows = api.chunk_public_inputs(api.CIRCUIT_AES, m, n_chunks=2, mask=mask, revealed=api.reveal_bytes(m, mask))
    plain = api.chunk_public_inputs(api.CIRCUIT_AES, m, n_chunks=2)
    bits = lambda data: bytes((b >> i) & 1 for b in data for i in range(8))
    for j in range(2):
        assert rows[j] == plain[j] + bits(mask[2 * j:2 * j + 2]) + bits(api.reveal_bytes(m, mask)[16 * j:16 * j + 16])


def _signature(text, kernel):
    a = text.index("__global__ void %s(" % kernel)
    return text[a:text.index(") {", a)]


def test_reveal_trace_kernel_on_host_under_sanitizers():
    """k_reveal_trace (csrc/kernels_reveal.cuh), behind the mode kernels and the tag kernel of csrc/kernels_witness.cuh and k_sha256_trace of csrc/kernels_digest.cuh and
    ahead of k_witness_expand -- the very headers the library compiles for the device -- compiled for the host and run lane by lane under ASan + UBSan
    (tests/reveal_trace_emu.cpp, a stand-alone program: nothing is loaded into python), over the shapes and masks listed there, two proofs per launch"""
    wit, dig, rev = (open(os.path.join(CSRC, "kernels_%s.cuh" % name)).read() for name in ("witness", "digest", "reveal"))
    assert "k_reveal_trace" in rev and "k_sha256_trace" in dig and "k_witness_expand" in wit
    for word in ("atomic", "__shared__", "__syncthreads", "__shfl", "hipLaunch"):                   # one writer per byte needs no atomics; no LDS, barrier or cross-lane operation
        assert word not in rev and word not in dig and word not in wit
    assert "revealed" not in _signature(rev, "k_reveal_trace")                                     # the kernel is never handed `revealed`
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "reveal_trace_emu")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wno-unknown-pragmas", "-I", CSRC, "-I", os.path.join(ROOT, "tests"),
                               os.path.join(ROOT, "tests", "reveal_trace_emu.cpp")] + HOST_SOURCES + ["-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=1800)
        assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
        print(out.stdout)
        assert out.stdout.splitlines()[-1] == "total bad 0"


def _run_standalone(name, args=()):
    cxx = CLANG if os.path.exists(CLANG) else "g++"
    flags = ["-x", "c++", "-O1", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC]
    if cxx == CLANG:
        flags += ["-mllvm", "-asan-globals=0"]        # (as tests/test_fuzz_host.py: this toolchain's ASan trips over its own registration of merged string literals)
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, name)
        subprocess.check_call([cxx] + flags + [os.path.join(ROOT, "tests", name + ".cpp")] + HOST_SOURCES + ["-o", exe])
        env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
        out = subprocess.run([exe] + list(args), capture_output=True, text=True, env=env, timeout=900)
        assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
        assert out.stdout.split() == [name, "ok"]


def test_statement_layer_under_sanitizers():
    """tests/reveal_statement_check.cpp: zk::chunk_mask_slice and zk::reveal_bytes (the prover's side) against the tail of every row of zkaes_chunk_public_inputs_rv (the
    verifier's), under ASan + UBSan.  A stand-alone program: nothing is loaded into python"""
    _run_standalone("reveal_statement_check")


def test_host_entry_points_under_sanitizers():
    """tests/reveal_host_check.cpp: the circuit queries and the committed ECB fixture proof -- whole, truncated at every length, garbage -- through
    zkaes_verify_reveal_chunked and zkaes_verify_encryption_gcm_reveal under the stored key, the transported key and a key whose |X| fits a reveal statement: never
    accepted.  A stand-alone program: nothing is loaded into python"""
    _run_standalone("reveal_host_check", [GOLD])
