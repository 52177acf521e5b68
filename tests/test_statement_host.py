"""The statement layer on the host (csrc/statement.hpp; no GPU): the rule that says which public header chunk j of a job is proven and checked under has one definition,
zk::chunk_mode_header, which the prover calls directly and every chunked verifier reaches through zkaes_chunk_public_inputs' row builder.  The two must agree bit for
bit; tests/statement_host_check.cpp holds them against each other and against headers written out by hand.
"""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aes_zero_knowledge_proof_circuit_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def test_a_key_without_a_handle_is_an_error_not_a_crash(api):
    """the four entry points that used to dereference a NULL key answer with an error, and a ProvingKey whose handle is gone (free() has run) raises before the library
    is called at all"""
    import ctypes as C
    L = api.lib()
    assert L.zkaes_pk_info(None, (C.c_uint64 * 12)()) != 0 and b"null" in L.zkaes_last_error()
    assert L.zkaes_pk_timings(None, (C.c_double * 6)()) != 0 and b"null" in L.zkaes_last_error()
    out, n = C.c_void_p(), C.c_size_t()
    assert L.zkaes_pk_debug_fetch(None, b"z", C.byref(out), C.byref(n)) != 0 and b"null" in L.zkaes_last_error()
    assert L.zkaes_aes_witness(None, bytes(16), C.c_size_t(16), bytes(16), None, C.c_size_t(0), C.byref(n)) != 0 and b"null" in L.zkaes_last_error()
    pk = api.ProvingKey(None)
    pk.free()                                                                # (twice is fine)
    for call in (pk.info, pk.timings, pk.key_bytes, pk.mode, lambda: pk.debug_fetch("z"), lambda: pk.witness(bytes(16), bytes(16)), lambda: api.encrypt(bytes(16), bytes(16), pk),
                 lambda: pk.encrypt_chunked(bytes(16), bytes(16)), lambda: pk.encrypt_digest_batch([bytes(16)], [bytes(16)])):
        with pytest.raises(api.ZkAesError, match="freed"):
            call()


def test_chunk_headers_on_both_sides_under_asan_ubsan():
    """tests/statement_host_check.cpp with the three host-only sources under -fsanitize=address,undefined, built as test_cbc_host.py builds its program: ECB, CBC and CTR,
    slices of 16 and 32 bytes, 1 to 3 chunks, no key tag and 16 and 32 tag bytes, with and without states; by hand the CBC chaining blocks, the CTR counter that wraps
    to zero, the one whose carry crosses byte 8, and the lone 17-byte CTR slice.  A stand-alone program: nothing is loaded into python."""
    cxx = CLANG if os.path.exists(CLANG) else "g++"
    srcs = [os.path.join(ROOT, "tests", "statement_host_check.cpp")] + [os.path.join(CSRC, f) for f in ("circuit.cpp", "marlin_codec.cpp", "capi_host.cpp")]
    flags = ["-x", "c++", "-O1", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC]
    if cxx == CLANG:
        flags += ["-mllvm", "-asan-globals=0"]        # (as tests/test_fuzz_host.py: this toolchain's ASan trips over its own registration of merged string literals)
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "statement_host_check")
        subprocess.check_call([cxx] + flags + srcs + ["-o", exe])
        env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
        out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
        assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
        assert out.stdout.split() == ["statement_host_check", "ok"]
