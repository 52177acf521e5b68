"""Plaintext digests on the host: the host's SHA-256 against hashlib and the pure-Python model, the digest circuits' counts against closed forms, digest kind 0 unchanged
through the new entry points, the chunk shape over the default SRS, k_sha256_trace's source run lane by lane under sanitizers, and the host-only verifiers under
sanitizers (no GPU, no oracle).

A key synthesized with digest = "chain" or "final" proves, beside its mode's statement and its key tag, H_out = the SHA-256 compressions of its hidden message from H_in
 and exposes H_in then H_out as the LAST 512 public inputs.

Closed forms (tests/sha256_model.py).  Over a block of variables a compression is 48 schedule words of 150 rows (sigma_0 61 xor gates, sigma_1 54, the sum
32 result bits + 2 carry bits + 1 row), 64 rounds of 296 (Sigma_1 64, Ch 32, Sigma_0 64, a ^ b 32, Maj 32, e' and a' 32 + 3 + 1 each) and 8 feed-forward sums of 34:
26,416 rows.  H_in and H_out cost 256 booleanity rows each and H_out 256 equalities.  In a final key's padded blocks an xor with a constant bit is a re-wiring and a
schedule word whose operands are all constants is a constant: sha256_model.schedule_rows counts what is left from the masks of variable bits.
"""
import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import pytest

import sha256_model as model
from test_cbc_host import CLANG, CSRC, GOLD, ROOT

LENGTHS = [0, 1, 55, 56, 63, 64, 65, 119, 120, 128]


def _msg(n, salt=0):
    return bytes((37 * i + 11 + salt) & 0xff for i in range(n))


def test_model_is_sha256():
    for n in LENGTHS + [200]:
        m = _msg(n)
        assert model.finish(None, 0, m) == hashlib.sha256(m).digest()
    assert model.compressions("final", 55) == 1 and model.compressions("final", 56) == 2 and model.compressions("chain", 128) == 2
    assert model.COMPRESSION_ROWS == 48 * 150 + 64 * 296 + 8 * 34 == 26416


@pytest.mark.parametrize("n", LENGTHS)
def test_host_finish_is_hashlib(api, n):
    m = _msg(n)
    assert api.sha256_finish(None, 0, m) == hashlib.sha256(m).digest()


def test_host_chain_then_finish(api):
    m = _msg(64 + 37, 5)
    mid = api.sha256_chain(m[:64])
    assert mid == model.chain(m[:64]) and mid != hashlib.sha256(m[:64]).digest()                  # an unpadded state, not a digest
    assert api.sha256_finish(mid, 64, m[64:]) == hashlib.sha256(m).digest()
    assert api.sha256_chain(m[64:64], mid) == mid and api.sha256_chain(b"") == model.IV
    long = _msg(256, 9)
    assert api.sha256_chain(long[128:], api.sha256_chain(long[:128])) == api.sha256_chain(long) == model.chain(long)
    assert api.sha256_finish(api.sha256_chain(long), 256, b"") == hashlib.sha256(long).digest()
    for bad in (1, 63, 65):
        with pytest.raises(api.ZkAesError):
            api.sha256_chain(bytes(bad))
    with pytest.raises(api.ZkAesError):
        api.sha256_finish(None, 32, b"x")
    with pytest.raises(api.ZkAesError):
        api.sha256_finish(None, 1 << 61, b"x")
    with pytest.raises(api.ZkAesError):
        api.sha256_chain(bytes(64), bytes(31))


def shapes(api):
    """(circuit, key bits, L, A, T, digest, P): the issue's shapes"""
    return [(api.CIRCUIT_AES, 128, 64, 0, 0, "chain", 0), (api.CIRCUIT_AES, 128, 128, 0, 0, "chain", 0), (api.CIRCUIT_AES_CTR, 128, 17, 0, 1, "final", 0),
            (api.CIRCUIT_AES_CTR, 128, 55, 0, 0, "final", 0), (api.CIRCUIT_AES_CTR, 128, 56, 0, 0, "final", 0), (api.CIRCUIT_AES_CBC, 192, 64, 0, 1, "chain", 0),
            (api.CIRCUIT_AES_GCM, 256, 17, 5, 1, "final", 64), (api.CIRCUIT_AES, 256, 64, 0, 2, "chain", 0)]


def test_kind_zero_is_the_tagged_query(api):
    """digest = None through the _pd entry points answers element for element what the _kt entry points answer"""
    L = api.lib()
    for circuit, bits, n, a, t, _, _ in shapes(api)[2:]:
        kt, pd = (C.c_uint64 * 12)(), (C.c_uint64 * 12)()
        assert L.zkaes_circuit_info_kt(circuit, C.c_uint(bits), C.c_uint(t), C.c_size_t(n), C.c_size_t(a), kt) == 0
        assert L.zkaes_circuit_info_pd(circuit, C.c_uint(bits), C.c_uint(t), C.c_uint(0), C.c_uint64(0), C.c_size_t(n), C.c_size_t(a), pd) == 0
        assert list(kt) == list(pd)
    import numpy as np
    circuit, bits, n, a, t = api.CIRCUIT_AES_CTR, 128, 17, 0, 1
    for which in range(3):
        rows, nnz = C.c_uint64(), C.c_uint64()
        assert L.zkaes_circuit_matrix_kt(circuit, C.c_uint(bits), C.c_uint(t), C.c_size_t(n), C.c_size_t(a), which, C.byref(rows), C.byref(nnz), None, None, None) == 0
        rowptr, col, coeff = np.zeros(rows.value + 1, np.uint32), np.zeros(nnz.value, np.uint32), np.zeros(nnz.value, np.int64)
        assert L.zkaes_circuit_matrix_kt(circuit, C.c_uint(bits), C.c_uint(t), C.c_size_t(n), C.c_size_t(a), which, None, None, rowptr.ctypes.data_as(C.c_void_p), col.ctypes.data_as(C.c_void_p),
                                         coeff.ctypes.data_as(C.c_void_p)) == 0
        got = api.circuit_matrix(circuit, n, which, a, bits, t, None, 0)
        assert (got[0] == rowptr).all() and (got[1] == col).all() and (got[2] == coeff).all()


def test_closed_form_counts(api):
    for circuit, bits, n, a, t, kind, prefix in shapes(api):
        plain = api.circuit_info(circuit, n, a, bits, t)
        got = api.circuit_info(circuit, n, a, bits, t, kind, prefix)
        rows, wits = model.digest_size(kind, n)
        print(circuit, bits, n, a, t, kind, prefix, "digest rows", rows, "witnesses", wits, "->", got["raw_constraints"], got["raw_witness"])
        assert got["raw_instance"] == plain["raw_instance"] + 512
        assert got["raw_constraints"] == plain["raw_constraints"] + rows
        assert got["raw_witness"] == plain["raw_witness"] + wits
    # a block of variables, and what folds away: the all-padding second block of a 56-byte final key has no schedule rows at all
    assert model.digest_size("chain", 64) == (768 + 26416, 26416 - 48 - 128 - 8)
    assert model.digest_size("chain", 128)[0] == 768 + 2 * 26416
    assert model.digest_size("final", 56)[0] - model.digest_size("final", 55)[0] >= 64 * 296 + 8 * 34                # (and one more message byte's worth of schedule gates in block 0)
    assert model.schedule_rows([0] * 16) == (0, 0) and model.schedule_rows([0xffffffff] * 16) == (7200, 48)
    # the prefix moves constants only
    assert api.circuit_info(api.CIRCUIT_AES_CTR, 17, 0, 128, 1, "final", 64)["raw_constraints"] == api.circuit_info(api.CIRCUIT_AES_CTR, 17, 0, 128, 1, "final", 0)["raw_constraints"]


def test_chunk_shape_over_the_default_srs(api):
    """ECB-128, 64 bytes, chain: with T = 0 and with T = 2 the chunk stays inside |H| = 2^20 and |K| = 2^22, the domains of today's headline chunk.  circuit_info is
    host-only and leaves h, k to the key, so they are derived as the prover derives them (test_keytag_host.py): |H| from the padded constraint count, |K| from the joint
    matrix's non-zeros"""
    for t in (0, 2):
        info = api.circuit_info(api.CIRCUIT_AES, 64, 0, 128, t, "chain")
        h = 1
        while h < max(info["constraints"], info["instance"] + info["witness"]):
            h *= 2
        joint = _joint_nnz(api, t)
        k = 1
        while k < joint:
            k *= 2
        print("T =", t, "rows", info["raw_constraints"], "padded", info["constraints"], "joint non-zeros", joint, "|H|", h, "|K|", k)
        assert h == 1 << 20 and k == 1 << 22
        assert info["raw_instance"] - 1 == 512 + 128 * t + 512


def _joint_nnz(api, t):
    """non-zeros of the joint matrix: the positions where A, B or C has an entry"""
    import numpy as np
    seen = []
    for which in range(3):
        rowptr, col, _ = api.circuit_matrix(api.CIRCUIT_AES, 64, which, 0, 128, t, "chain")
        rows = np.repeat(np.arange(len(rowptr) - 1, dtype=np.uint64), np.diff(rowptr).astype(np.int64))
        seen.append((rows << np.uint64(32)) | col.astype(np.uint64))
    return len(np.unique(np.concatenate(seen)))


def test_refusals(api):
    with pytest.raises(api.ZkAesError):
        api.circuit_info(api.CIRCUIT_AES, 64, digest="sponge")
    for n in (16, 48, 80):                                                                          # a chain key takes whole SHA-256 blocks
        with pytest.raises(api.ZkAesError, match="multiple of 64"):
            api.circuit_info(api.CIRCUIT_AES, n, digest="chain")
    with pytest.raises(api.ZkAesError):
        api.circuit_info(api.CIRCUIT_AES, 64, digest="chain", digest_prefix=64)                     # a prefix belongs to a final key
    with pytest.raises(api.ZkAesError):
        api.circuit_info(api.CIRCUIT_AES, 64, digest=None, digest_prefix=64)
    for prefix in (1, 32, 100, 1 << 61, (1 << 61) - 64):                                            # multiples of 64 with P + L < 2^61
        with pytest.raises(api.ZkAesError):
            api.circuit_info(api.CIRCUIT_AES, 64, digest="final", digest_prefix=prefix)
    for kind in (api.CIRCUIT_OPS_XOR, api.CIRCUIT_OPS_ADD):
        assert api.circuit_info(kind, 0, digest=None) == api.circuit_info(kind, 0)
        with pytest.raises(api.ZkAesError):
            api.circuit_info(kind, 0, digest="final")
    with pytest.raises(api.ZkAesError, match="no HIP device|multiple of 64"):                       # the synthesizer refuses the same (ahead of, or without, a device)
        api.synthesize_keys(16, digest="chain")


def test_digest_trace_kernel_on_host_under_sanitizers():
    """k_sha256_trace (csrc/kernels_digest.cuh), behind the mode kernels and the tag kernel of csrc/kernels_witness.cuh and ahead of k_witness_expand -- the very headers
    the library compiles for the device -- compiled for the host and run lane by lane under ASan + UBSan (tests/digest_trace_emu.cpp, a stand-alone program: nothing is
    loaded into python), over the shapes listed there, two proofs per launch"""
    wit = open(os.path.join(CSRC, "kernels_witness.cuh")).read()
    dig = open(os.path.join(CSRC, "kernels_digest.cuh")).read()
    assert "k_sha256_trace" in dig and "sha_compress" in dig and "k_witness_expand" in wit
    for word in ("atomic", "__shared__", "__syncthreads", "__shfl", "hipLaunch"):                   # one writer per byte needs no atomics; no LDS, barrier or cross-lane operation
        assert word not in dig and word not in wit
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "digest_trace_emu")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wno-unknown-pragmas", "-I", CSRC, "-I", os.path.join(ROOT, "tests"),
                               os.path.join(ROOT, "tests", "digest_trace_emu.cpp")] + [os.path.join(CSRC, f) for f in ("circuit.cpp", "marlin_codec.cpp", "capi_host.cpp")] + ["-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=1800)
        assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
        print(out.stdout)
        assert out.stdout.splitlines()[-1] == "total bad 0"


def test_host_entry_points_under_sanitizers():
    """tests/digest_host_check.cpp with the three host-only sources under -fsanitize=address,undefined: the host SHA-256 into exactly sized buffers, the circuit queries,
    and the committed ECB fixture proof -- whole, truncated at every length, garbage -- through zkaes_verify_digest_chunked and zkaes_verify_encryption_gcm_digest under the
    stored key, the transported key and a key whose |X| fits a digest statement: never accepted.  A stand-alone program: nothing is loaded into python."""
    cxx = CLANG if os.path.exists(CLANG) else "g++"
    srcs = [os.path.join(ROOT, "tests", "digest_host_check.cpp")] + [os.path.join(CSRC, f) for f in ("circuit.cpp", "marlin_codec.cpp", "capi_host.cpp")]
    flags = ["-x", "c++", "-O1", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC]
    if cxx == CLANG:
        flags += ["-mllvm", "-asan-globals=0"]        # (as tests/test_fuzz_host.py: this toolchain's ASan trips over its own registration of merged string literals)
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "digest_host_check")
        subprocess.check_call([cxx] + flags + srcs + ["-o", exe])
        env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
        out = subprocess.run([exe, GOLD], capture_output=True, text=True, env=env, timeout=900)
        assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
        assert out.stdout.split() == ["digest_host_check", "ok"]
