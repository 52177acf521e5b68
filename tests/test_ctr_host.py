"""AES-128-CTR on the host: ctr_crypt and ctr_counter_add, the circuit's counts against ECB's, the matrices' shape, the host-only verifiers, and the trace kernel's
source run lane by lane under sanitizers (no GPU, no oracle).

Correctness of the CTR statement rests on an independent model (pure-Python CTR over the FIPS-197 model of test_cbc_host.py, counters as Python integers), the NIST
vector (SP 800-38A F.5.1) and -- on the GPU, in test_gpu_ctr.py -- a constraint check in numpy; there is no upstream CTR circuit to be byte-identical to.
"""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from test_cbc_host import CLANG, CSRC, GOLD, NIST_KEY, NIST_PT, ROOT, _encrypt_block, _joint_nnz, _pow2, _round_keys

# NIST SP 800-38A F.5.1, CTR-AES128.Encrypt (key and plaintext are F.2.1's)
NIST_ICB = bytes.fromhex("f0f1f2f3f4f5f6f7f8f9fafbfcfdfeff")
NIST_CTR_CT = bytes.fromhex("874d6191b620e3261bef6864990db6ce" "9806f66b7970fdff8617187bb9fffdff" "5ae4df3edbd5d35e5b4f09020db03eab" "1e031dda2fbe03d1792170a0f3009cee")

# counters whose increment carries furthest: ..00ff, ..00 ffffffff (the carry must reach byte 11; GCM's inc32 would wrap to ..00 00000000), ff..ff (wraps to zero)
WRAP_ICBS = [bytes(15) + b"\xff", bytes(12) + b"\xff" * 4, b"\xff" * 16]
# (A, B, C non-zeros are asserted at 16 and 96 bytes only; these are the issue's figures)
COUNTS_16 = dict(raw_constraints=185_296, raw_instance=257, nnz=(200_599, 338_000, 344_427))
COUNTS_96 = dict(raw_constraints=928_561, raw_instance=897, raw_witness=926_897, nnz=(1_004_592, 1_692_444, 1_729_288), joint=3_654_753)


def model_counter(icb, n):
    """icb + n mod 2^128, big-endian, through Python integers"""
    return ((int.from_bytes(icb, "big") + n) % (1 << 128)).to_bytes(16, "big")


def model_ctr(data, key, icb):
    """AES-128-CTR, SP 800-38A 6.5 with the standard incrementing function over all 128 bits (appendix B.1, m = 128)"""
    rks, out = _round_keys(key), b""
    for b, off in enumerate(range(0, len(data), 16)):
        stream = _encrypt_block(model_counter(icb, b), rks)
        out += bytes(x ^ s for x, s in zip(data[off:off + 16], stream))
    return out


def test_model_reproduces_the_nist_vector():
    assert model_ctr(NIST_PT, NIST_KEY, NIST_ICB) == NIST_CTR_CT
    assert len(NIST_CTR_CT) == 64


def test_ctr_crypt_nist_vector_and_prefixes(api):
    assert api.ctr_crypt(NIST_PT, NIST_KEY, NIST_ICB) == NIST_CTR_CT
    for n in (1, 15, 17, 33):
        assert api.ctr_crypt(NIST_PT[:n], NIST_KEY, NIST_ICB) == NIST_CTR_CT[:n], n


@pytest.mark.parametrize("n", [1, 15, 16, 17, 31, 100])
def test_ctr_crypt_matches_the_python_model(api, n):
    rs = np.random.RandomState(0xC7A0 + n)
    for _ in range(3):
        msg, key, icb = rs.bytes(n), rs.bytes(16), rs.bytes(16)
        ct = api.ctr_crypt(msg, key, icb)
        assert ct == model_ctr(msg, key, icb)
        assert api.ctr_crypt(ct, key, icb) == msg                                  # its own inverse


@pytest.mark.parametrize("icb", WRAP_ICBS, ids=lambda b: b.hex())
def test_counter_wrap_around(api, icb):
    rs = np.random.RandomState(0xC7A1)
    msg, key = rs.bytes(48), rs.bytes(16)
    ct = api.ctr_crypt(msg, key, icb)
    assert ct == model_ctr(msg, key, icb)
    if icb == WRAP_ICBS[1]:                                                          # what inc32 would give for block 1 is NOT what comes out
        inc32 = icb[:12] + bytes(4)
        assert ct[16:32] != bytes(m ^ s for m, s in zip(msg[16:32], _encrypt_block(inc32, _round_keys(key))))
        assert api.ctr_counter_add(icb, 1) == bytes(11) + b"\x01" + bytes(4)


def test_ctr_counter_add_against_python_integers(api):
    for icb in WRAP_ICBS + [NIST_ICB, bytes(16)]:
        for n in (0, 1, 1 << 32, (1 << 64) - 1):
            assert api.ctr_counter_add(icb, n) == model_counter(icb, n), (icb.hex(), n)
    assert api.ctr_counter_add(b"\xff" * 16, 1) == bytes(16)


def test_a_job_split_in_two_calls(api):
    rs = np.random.RandomState(0xC7A2)
    msg, key = rs.bytes(16 * 5 + 7), rs.bytes(16)
    for icb in (NIST_ICB, b"\xff" * 15 + b"\xfe"):
        whole = api.ctr_crypt(msg, key, icb)
        assert whole == model_ctr(msg, key, icb)
        for blocks_before in (1, 2, 5):
            cut = 16 * blocks_before
            assert api.ctr_crypt(msg[:cut], key, icb) + api.ctr_crypt(msg[cut:], key, api.ctr_counter_add(icb, blocks_before)) == whole


def test_ctr_refusals(api):
    with pytest.raises(api.ZkAesError):
        api.circuit_info(api.CIRCUIT_AES_CTR, 0)
    with pytest.raises(api.ZkAesError):
        api.circuit_matrix(api.CIRCUIT_AES_CTR, 0, 0)
    with pytest.raises(api.ZkAesError):
        api.ctr_crypt(b"", NIST_KEY, NIST_ICB)
    for key, icb in ((bytes(15), NIST_ICB), (bytes(17), NIST_ICB), (NIST_KEY, bytes(15)), (NIST_KEY, bytes(17))):
        with pytest.raises(api.ZkAesError):
            api.ctr_crypt(bytes(16), key, icb)
    with pytest.raises(api.ZkAesError):
        api.ctr_counter_add(bytes(15), 1)
    with pytest.raises(api.ZkAesError):
        api.ctr_counter_add(bytes(16), 1 << 64)


@pytest.mark.parametrize("n", [1, 16, 17, 33, 48, 96])
def test_circuit_counts_relative_to_ecb(api, n):
    """Relative to ECB at 16 nb bytes (nb = ceil(L / 16)): 128 icb input bits (one constraint each), per block 128 xor gates C = M ^ S_10, per block after the first the
    incrementer's 127 xor + 126 and gates, and per byte the last block lacks 8 message witnesses, 8 xor gates, 8 ciphertext inputs and 8 equalities less:

        raw_constraints = E + 128 + 128 nb + 253 (nb - 1) - 32 (16 nb - L),    raw_instance = 129 + 8 L.

    The 16-byte and the 96-byte figures (constraints, instance, witnesses, the non-zeros of A, B and C) are asserted exactly."""
    nb = (n + 15) // 16
    e, c = api.circuit_info(api.CIRCUIT_AES, 16 * nb), api.circuit_info(api.CIRCUIT_AES_CTR, n)
    print(n, {k: int(c[k]) for k in c})
    assert c["raw_constraints"] == e["raw_constraints"] + 128 + 128 * nb + 253 * (nb - 1) - 32 * (16 * nb - n)
    assert c["raw_instance"] == 129 + 8 * n
    # witnesses: ECB's, one per xor gate of C, 253 per increment, and 16 less per missing byte (8 message bits, 8 xor results)
    assert c["raw_witness"] == e["raw_witness"] + 128 * nb + 253 * (nb - 1) - 16 * (16 * nb - n)
    want = {1: 184_816, 16: 185_296, 17: 333_469, 33: 482_122, 48: 482_602, 96: 928_561}[n]
    assert c["raw_constraints"] == want
    if n == 16:
        assert (c["raw_constraints"], c["raw_instance"]) == (COUNTS_16["raw_constraints"], COUNTS_16["raw_instance"])
        assert (c["nnz_a"], c["nnz_b"], c["nnz_c"]) == COUNTS_16["nnz"]
    if n == 96:
        assert (c["raw_constraints"], c["raw_instance"], c["raw_witness"]) == (COUNTS_96["raw_constraints"], COUNTS_96["raw_instance"], COUNTS_96["raw_witness"])
        assert (c["nnz_a"], c["nnz_b"], c["nnz_c"]) == COUNTS_96["nnz"]
        assert c["instance"] == e["instance"] == 1024                                           # |X|


def test_six_block_domains_equal_ecb(api):
    """|H| and |K| of the 96-byte CTR chunk equal those of the 6-block ECB chunk the benchmark proves, derived as test_cbc_host.test_six_block_domains_equal_ecb derives
    them; the joint non-zeros are the issue's 3,654,753, inside the reference's SRS literal (4,062,064)"""
    hk = {}
    for kind in (api.CIRCUIT_AES, api.CIRCUIT_AES_CTR):
        joint = _joint_nnz(api, kind, 96)
        hk[kind] = (_pow2(int(api.circuit_info(kind, 96)["constraints"])), _pow2(joint))
        print(kind, "joint nnz", joint, "h, k", hk[kind])
        if kind == api.CIRCUIT_AES_CTR:
            assert joint == COUNTS_96["joint"] and joint <= 4_062_064
    assert hk[api.CIRCUIT_AES_CTR] == hk[api.CIRCUIT_AES] == (1 << 20, 1 << 22)
    assert api.circuit_info(api.CIRCUIT_AES_CTR, 96)["instance"] == 1024


@pytest.mark.parametrize("which", [0, 1, 2])
def test_circuit_matrix_shape(api, which):
    ci = api.circuit_info(api.CIRCUIT_AES_CTR, 17)
    rowptr, col, coeff = api.circuit_matrix(api.CIRCUIT_AES_CTR, 17, which)
    assert len(rowptr) - 1 == ci["constraints"]
    assert rowptr[0] == 0 and rowptr[-1] == len(col) == len(coeff) == ci[("nnz_a", "nnz_b", "nnz_c")[which]]
    assert np.all(np.diff(rowptr.astype(np.int64)) >= 0)
    assert int(col.max()) < ci["instance"] + ci["witness"]
    assert ci["constraints"] == ci["instance"] + ci["witness"]                                   # square after padding
    assert ci["raw_instance"] == 129 + 8 * 17 and ci["instance"] == 512


def test_verifiers_do_not_accept_the_ecb_fixture(api):
    """the committed ECB verifying key and proof through the CTR verifiers: never accepted, no crash.  The stored key carries its own public-input count (128), which no
    CTR length has, so every ciphertext length raises; after the ark transport the key knows |X| only, and the verifier rejects instead"""
    vk = api.VerifyingKey.from_bytes(open(os.path.join(GOLD, "gpu_aes16_vk.bin"), "rb").read())
    proof = open(os.path.join(GOLD, "gpu_aes16_proof.bin"), "rb").read()
    ecb_ct = bytes.fromhex("3925841d02dc09fbdc118597196a0b32")
    assert api.verify_encryption(vk, proof, ecb_ct) is True
    for ct in (ecb_ct, ecb_ct[:15], ecb_ct[:1], ecb_ct + b"\0", NIST_CTR_CT, b""):
        with pytest.raises(api.ZkAesError):
            api.verify_encryption_ctr(vk, proof, NIST_ICB, ct)
    with pytest.raises(api.ZkAesError):
        api.verify_ctr_chunked(vk, [proof, proof], NIST_ICB, NIST_CTR_CT[:32])
    ark = api.VerifyingKey.from_ark_bytes(vk.to_ark_bytes())
    for ct in (ecb_ct, ecb_ct[:15], ecb_ct + b"\0", NIST_CTR_CT):
        assert api.verify_encryption_ctr(ark, proof, NIST_ICB, ct) is False
        assert api.verify_encryption_ctr(ark, proof, bytes(16), ct) is False
    assert api.verify_ctr_chunked(ark, [proof, proof], NIST_ICB, NIST_CTR_CT[:32]) == [False, False]
    assert api.verify_ctr_chunked(ark, [proof[:100]], NIST_ICB, ecb_ct) == [False]
    with pytest.raises(api.ZkAesError):
        api.verify_encryption_ctr(ark, proof, NIST_ICB, b"")
    with pytest.raises(api.ZkAesError):
        api.verify_encryption_ctr(ark, proof[:-1], NIST_ICB, ecb_ct)
    with pytest.raises(api.ZkAesError):
        api.verify_ctr_chunked(ark, [proof, proof], NIST_ICB, NIST_CTR_CT[:48])
    with pytest.raises(api.ZkAesError):
        api.verify_encryption_ctr(ark, proof, NIST_ICB[:15], ecb_ct)


def test_host_entry_points_under_asan_ubsan():
    """tests/ctr_host_check.cpp with the three host-only sources under -fsanitize=address,undefined: the NIST vector and its prefixes through zkaes_ctr_crypt in buffers of
    exactly the message's size, zkaes_ctr_counter_add, the ECB fixtures whole and truncated at every length through both CTR verifiers.  A stand-alone program: nothing is
    loaded into python."""
    cxx = CLANG if os.path.exists(CLANG) else "g++"
    srcs = [os.path.join(ROOT, "tests", "ctr_host_check.cpp")] + [os.path.join(CSRC, f) for f in ("circuit.cpp", "marlin_codec.cpp", "capi_host.cpp")]
    flags = ["-x", "c++", "-O1", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC]
    if cxx == CLANG:
        flags += ["-mllvm", "-asan-globals=0"]        # (as tests/test_fuzz_host.py: this toolchain's ASan trips over its own registration of merged string literals)
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "ctr_host_check")
        subprocess.check_call([cxx] + flags + srcs + ["-o", exe])
        env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
        out = subprocess.run([exe, GOLD], capture_output=True, text=True, env=env, timeout=900)
        assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
        assert out.stdout.split() == ["ctr_host_check", "ok"]


def test_ctr_trace_kernel_emulated_on_the_host():
    """k_aes_trace_ctr (with the key-schedule helper it shares with k_aes_trace) and k_witness_expand, the very header the library compiles for the device (csrc/kernels_witness.cuh), run lane by
    lane on the host under ASan + UBSan (tests/ctr_trace_emu.cpp): L = 1, 16, 17, 33, 48 with two proofs per launch under different counters, the wrap-around ones among
    them; the message buffer is exactly nproofs x L bytes, so an over-read of the partial block is a sanitizer report"""
    text = open(os.path.join(CSRC, "kernels_witness.cuh")).read()
    assert "hip" not in text.lower() and "k_aes_trace_ctr" in text and "aes_key_schedule" in text and "k_witness_expand" in text
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "ctr_trace_emu")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC, "-I", os.path.join(ROOT, "tests"),
                               os.path.join(ROOT, "tests", "ctr_trace_emu.cpp")] + [os.path.join(CSRC, f) for f in ("circuit.cpp", "marlin_codec.cpp", "capi_host.cpp")] + ["-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
        print(out.stdout)
        lines = out.stdout.splitlines()
        assert lines[-1] == "total bad 0" and out.stdout.count("unsatisfied 0, instance mismatches 0, rows unsatisfied after a ciphertext flip 1,") == 10
