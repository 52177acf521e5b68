"""AES-128-CBC on the host: the ciphertext entry point, the circuit's counts against ECB's, the matrices' shape, and the host-only verifiers (no GPU, no oracle).

Correctness of the CBC statement rests on an independent model (the pure-Python AES-CBC below), the NIST vector (SP 800-38A F.2.1) and -- on the GPU, in
test_gpu_cbc.py -- a constraint check in numpy; there is no upstream CBC circuit to be byte-identical to.
"""
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aes_zero_knowledge_proof_circuit_amd", "csrc")
GOLD = os.path.join(ROOT, "tests", "golden")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

# NIST SP 800-38A F.2.1, CBC-AES128.Encrypt
NIST_KEY = bytes.fromhex("2b7e151628aed2a6abf7158809cf4f3c")
NIST_IV = bytes.fromhex("000102030405060708090a0b0c0d0e0f")
NIST_PT = bytes.fromhex("6bc1bee22e409f96e93d7e117393172a" "ae2d8a571e03ac9c9eb76fac45af8e51" "30c81c46a35ce411e5fbc1191a0a52ef" "f69f2445df4f9b17ad2b417be66c3710")
NIST_CT = bytes.fromhex("7649abac8119b246cee98e9b12e9197d" "5086cb9b507219ee95db113a917678b2" "73bed6b8e3c1743b7116e69e22229516" "3ff1caa1681fac09120eca307586e1a7")


# ---- the model: AES-128-CBC from FIPS-197's definitions (S-box from the field inverse and the affine map, column-major state), sharing no code with the library
def _gmul(a, b):
    p = 0
    for _ in range(8):
        if b & 1:
            p ^= a
        a = ((a << 1) ^ (0x11B if a & 0x80 else 0)) & 0x1FF
        b >>= 1
    return p & 0xFF


def _make_sbox():
    box = []
    for x in range(256):
        inv = next((y for y in range(1, 256) if _gmul(x, y) == 1), 0)
        r = inv
        for i in range(1, 5):
            r ^= ((inv << i) | (inv >> (8 - i))) & 0xFF
        box.append(r ^ 0x63)
    return box


SBOX = _make_sbox()


def _round_keys(key):
    w = [list(key[4 * i:4 * i + 4]) for i in range(4)]
    rcon = 1
    for i in range(4, 44):
        t = list(w[i - 1])
        if i % 4 == 0:
            t = [SBOX[t[1]] ^ rcon, SBOX[t[2]], SBOX[t[3]], SBOX[t[0]]]
            rcon = _gmul(rcon, 2)
        w.append([a ^ b for a, b in zip(w[i - 4], t)])
    return [sum(w[4 * r:4 * r + 4], []) for r in range(11)]


def _encrypt_block(block, rks):
    s = [a ^ b for a, b in zip(block, rks[0])]
    for r in range(1, 11):
        s = [SBOX[v] for v in s]
        s = [s[4 * ((c + row) % 4) + row] for c in range(4) for row in range(4)]         # ShiftRows on the column-major state
        if r < 10:
            s = sum(([_gmul(col[k], 2) ^ _gmul(col[(k + 1) % 4], 3) ^ col[(k + 2) % 4] ^ col[(k + 3) % 4] for k in range(4)]
                     for col in (s[4 * c:4 * c + 4] for c in range(4))), [])
        s = [a ^ b for a, b in zip(s, rks[r])]
    return bytes(s)


def model_cbc(msg, key, iv):
    rks, prev, out = _round_keys(key), bytes(iv), b""
    for off in range(0, len(msg), 16):
        prev = _encrypt_block(bytes(a ^ b for a, b in zip(msg[off:off + 16], prev)), rks)
        out += prev
    return out


def model_ecb(msg, key):
    rks = _round_keys(key)
    return b"".join(_encrypt_block(msg[off:off + 16], rks) for off in range(0, len(msg), 16))


def test_model_reproduces_the_nist_vector():
    assert model_cbc(NIST_PT, NIST_KEY, NIST_IV) == NIST_CT


def test_cbc_ciphertext_nist_vector(api):
    assert api.cbc_ciphertext(NIST_PT, NIST_KEY, NIST_IV) == NIST_CT
    assert NIST_CT.hex().endswith("7586e1a7")
    for nb in (1, 2, 3):
        assert api.cbc_ciphertext(NIST_PT[:16 * nb], NIST_KEY, NIST_IV) == NIST_CT[:16 * nb]
    # a job split over several calls: each call's iv is the ciphertext block ahead of it
    assert api.cbc_ciphertext(NIST_PT[32:], NIST_KEY, NIST_CT[16:32]) == NIST_CT[32:]


@pytest.mark.parametrize("nb", [1, 2, 3, 7])
def test_cbc_ciphertext_matches_the_python_model(api, nb):
    rs = np.random.RandomState(0xCBC0 + nb)
    for _ in range(3):
        msg, key, iv = rs.bytes(16 * nb), rs.bytes(16), rs.bytes(16)
        ct = api.cbc_ciphertext(msg, key, iv)
        assert ct == model_cbc(msg, key, iv)
        assert nb == 1 or ct != model_ecb(msg, key)


def test_cbc_ciphertext_rejects_bad_lengths(api):
    for n in (0, 17, 15, 31):
        with pytest.raises(api.ZkAesError):
            api.cbc_ciphertext(bytes(n), NIST_KEY, NIST_IV)
    with pytest.raises(api.ZkAesError):
        api.cbc_ciphertext(bytes(16), bytes(15), NIST_IV)
    with pytest.raises(api.ZkAesError):
        api.cbc_ciphertext(bytes(16), NIST_KEY, bytes(17))


@pytest.mark.parametrize("nb", [1, 2, 3, 6])
def test_circuit_counts_relative_to_ecb(api, nb):
    """Relative to ECB at the same length: 128 nb xor gates (one constraint, one witness each) and 128 IV input bits (one constraint, one instance variable each).

    Constraints, instance and witness: the relations hold exactly at every nb.

    Non-zeros: every xor gate adds 1 / 1 / 3 entries to A / B / C and every IV input bit 2 / 1 / 0, i.e. (128 nb + 256, 128 nb + 128, 384 nb).  That is ALL the difference
    for nb = 1, and the 16-byte figures 200,599 / 338,000 / 344,427 are asserted exactly.  From the second block on it is a lower bound: X_b = M_b ^ C_{b-1} inherits the
    negations of C_{b-1}'s bits (Boolean::Not literals, which come from the constant Rcon xors of the key schedule), where ECB's round 0 sees plain message bits; the
    gates behind a negated literal are the same gates but spell 1 - x instead of x, one more entry of the One column each (measured excess over the formula, A / B / C:
    46 / 38 / 28 at nb = 2, 230 / 190 / 140 at nb = 6).  The 6-block totals -- 927,296 constraints, 897 instance variables, 4,421,616 non-zeros -- are asserted exactly."""
    e, c = api.circuit_info(api.CIRCUIT_AES, 16 * nb), api.circuit_info(api.CIRCUIT_AES_CBC, 16 * nb)
    print(nb, {k: (int(c[k]), int(c[k]) - int(e[k])) for k in c})
    assert c["raw_constraints"] == e["raw_constraints"] + 128 * nb + 128
    assert c["raw_instance"] == 129 + 128 * nb
    assert c["raw_witness"] == e["raw_witness"] + 128 * nb
    extra = [int(c[k]) - int(e[k]) for k in ("nnz_a", "nnz_b", "nnz_c")]
    formula = [128 * nb + 256, 128 * nb + 128, 384 * nb]
    if nb == 1:
        assert extra == formula
        assert (c["raw_constraints"], c["raw_instance"], c["raw_witness"]) == (185_296, 257, 184_912)
        assert (c["nnz_a"], c["nnz_b"], c["nnz_c"]) == (200_599, 338_000, 344_427)
    else:
        assert all(x >= f for x, f in zip(extra, formula))
    if nb == 6:
        assert (c["raw_constraints"], c["raw_instance"]) == (927_296, 897)
        assert c["nnz_a"] + c["nnz_b"] + c["nnz_c"] == 4_421_616
        assert c["instance"] == e["instance"] == 1024                                           # |X|


def _joint_nnz(api, kind, length):
    keys = []
    for which in range(3):
        rowptr, col, _ = api.circuit_matrix(kind, length, which)
        rows = np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr.astype(np.int64)))
        keys.append(rows * (1 << 32) + col.astype(np.int64))
    return len(np.unique(np.concatenate(keys)))


def _pow2(n):
    p = 1
    while p < n:
        p <<= 1
    return p


def test_six_block_domains_equal_ecb(api):
    """h and k of the 6-block CBC chunk equal those of the 6-block ECB chunk the benchmark proves (|X| = 1024 for both is asserted above): the same universal SRS holds it
    and the transform and MSM op lists have the same shapes.  circuit_info is host-only and leaves h, k to the key, so they are derived here as the prover derives them:
    |H| = the padded constraint count rounded up to a power of two, |K| likewise from the joint matrix's non-zeros (the union of the three supports, row by row)"""
    hk = {}
    for kind in (api.CIRCUIT_AES, api.CIRCUIT_AES_CBC):
        joint = _joint_nnz(api, kind, 96)
        hk[kind] = (_pow2(int(api.circuit_info(kind, 96)["constraints"])), _pow2(joint))
        print(kind, "joint nnz", joint, "h, k", hk[kind])
    assert hk[api.CIRCUIT_AES_CBC] == hk[api.CIRCUIT_AES]
    assert hk[api.CIRCUIT_AES_CBC][0] == 1 << 20                 # 927,296 constraints


def test_circuit_info_rejects_bad_lengths(api):
    for n in (0, 17):
        with pytest.raises(api.ZkAesError):
            api.circuit_info(api.CIRCUIT_AES_CBC, n)
        with pytest.raises(api.ZkAesError):
            api.circuit_matrix(api.CIRCUIT_AES_CBC, n, 0)


@pytest.mark.parametrize("which", [0, 1, 2])
def test_circuit_matrix_shape(api, which):
    ci = api.circuit_info(api.CIRCUIT_AES_CBC, 32)
    rowptr, col, coeff = api.circuit_matrix(api.CIRCUIT_AES_CBC, 32, which)
    assert len(rowptr) - 1 == ci["constraints"]
    assert rowptr[0] == 0 and rowptr[-1] == len(col) == len(coeff) == ci[("nnz_a", "nnz_b", "nnz_c")[which]]
    assert np.all(np.diff(rowptr.astype(np.int64)) >= 0)
    assert int(col.max()) < ci["instance"] + ci["witness"]
    assert ci["constraints"] == ci["instance"] + ci["witness"]                                   # square after padding


def test_verifiers_do_not_accept_the_ecb_fixture(api):
    """the committed ECB verifying key and proof through the CBC verifiers: a different statement (and instance size), so never accepted, and no crash"""
    vk = api.VerifyingKey.from_bytes(open(os.path.join(GOLD, "gpu_aes16_vk.bin"), "rb").read())
    proof = open(os.path.join(GOLD, "gpu_aes16_proof.bin"), "rb").read()
    ecb_ct = bytes.fromhex("3925841d02dc09fbdc118597196a0b32")
    assert api.verify_encryption(vk, proof, ecb_ct) is True
    assert api.verify_encryption_cbc(vk, proof, NIST_IV, ecb_ct) is False
    assert api.verify_encryption_cbc(vk, proof, bytes(16), ecb_ct) is False
    assert api.verify_encryption_cbc(vk, proof, NIST_IV, NIST_CT) is False
    assert api.verify_cbc_chunked(vk, [proof, proof], NIST_IV, NIST_CT[:32]) == [False, False]
    assert api.verify_cbc_chunked(vk, [proof[:100]], NIST_IV, ecb_ct) == [False]
    for bad in (b"", ecb_ct[:15], ecb_ct + b"\0"):
        with pytest.raises(api.ZkAesError):
            api.verify_encryption_cbc(vk, proof, NIST_IV, bad)
    with pytest.raises(api.ZkAesError):
        api.verify_encryption_cbc(vk, proof[:-1], NIST_IV, ecb_ct)
    with pytest.raises(api.ZkAesError):
        api.verify_cbc_chunked(vk, [proof, proof], NIST_IV, NIST_CT[:48])


def test_host_entry_points_under_asan_ubsan():
    """tests/cbc_host_check.cpp with the three host-only sources under -fsanitize=address,undefined: the NIST vector through zkaes_cbc_ciphertext, the ECB fixtures whole and
    truncated at every length through both CBC verifiers.  A stand-alone program: nothing is loaded into python."""
    cxx = CLANG if os.path.exists(CLANG) else "g++"
    srcs = [os.path.join(ROOT, "tests", "cbc_host_check.cpp")] + [os.path.join(CSRC, f) for f in ("circuit.cpp", "marlin_codec.cpp", "capi_host.cpp")]
    flags = ["-x", "c++", "-O1", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC]
    if cxx == CLANG:
        flags += ["-mllvm", "-asan-globals=0"]        # (as tests/test_fuzz_host.py: this toolchain's ASan trips over its own registration of merged string literals)
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "cbc_host_check")
        subprocess.check_call([cxx] + flags + srcs + ["-o", exe])
        env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
        out = subprocess.run([exe, GOLD], capture_output=True, text=True, env=env, timeout=900)
        assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
        assert out.stdout.split() == ["cbc_host_check", "ok"]


def test_trace_and_expand_kernels_emulated_on_the_host():
    """k_aes_trace<ECB / CBC> and k_witness_expand, the very header the library compiles for the device (csrc/kernels_witness.cuh), run lane by lane on the host under
    ASan + UBSan (tests/cbc_trace_emu.cpp): every constraint satisfied at nb = 1, 2, 3 with two proofs per launch, the instance equal to (IV,) host ciphertext, no write
    outside the traces"""
    text = open(os.path.join(CSRC, "kernels_witness.cuh")).read()
    assert "hip" not in text.lower() and "k_aes_trace" in text and "k_witness_expand" in text
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "cbc_trace_emu")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC, "-I", os.path.join(ROOT, "tests"),
                               os.path.join(ROOT, "tests", "cbc_trace_emu.cpp"), os.path.join(CSRC, "circuit.cpp"), "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
        assert out.stdout.splitlines()[-1] == "total bad 0" and out.stdout.count("unsatisfied 0, instance mismatches 0") == 12
